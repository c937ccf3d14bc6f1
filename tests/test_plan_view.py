"""Plan-view maps on the GPU (pcs_plan_view*), byte for byte against the restatement of DESIGN.md section 3 (tests/np_plan_view.py)
over the cases of tests/plan_view_cases.py: all four rasters and the statistics block. Both 2-byte payload phases, 0xA5 guards in
front of and behind every raster and the block, the counted form with garbage behind the count, the host form, two runs, a small
map in a large map's workspace, a shuffled record order, the cluster filter's output fed straight in, a stitched frame-set, one
working-size cloud, one timing interval per launch, every refusal."""
import ctypes as C

import numpy as np
import pytest

import np_plan_view as NP
import plan_view_cases as K
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import ClusterParams, PLAN_VIEW_LAUNCHES, PlanMaps, PlanParams, PlanStats

pytestmark = pytest.mark.gpu

GUARD = 64
N_MAX = 1 << 20
CELLS_MAX = 1 << 18                 # the arena's rasters: 4096 x 64 and 400 x 400 fit
NAMES = sorted(K.CASES)


def c_params(P, reserved=(0, 0, 0)):
    return PlanParams.make(P["up_axis"], P["up_sign"], P["cell_mm"], P["width"], P["height"], P["origin_u"], P["origin_v"], P["band_lo"],
                           P["band_hi"], reserved)


class Arena:
    """Device buffers shared by the tests of this module: a payload at any 2-byte phase, the count word, and one block that holds the
    four rasters and the statistics block, each between two guards of 0xA5."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.inp = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.words = ctx.device_malloc(64)
        self.out = ctx.device_malloc(self.layout(CELLS_MAX)[-1])
        assert self.inp % 16 == 0 and self.out % 256 == 0

    def free(self):
        for p in (self.inp, self.words, self.out):
            self.ctx.device_free(p)

    @staticmethod
    def layout(cells):
        """Offsets of count, top, bottom, rgb, stats (each behind a guard, 8-byte aligned) and the block's size."""
        at, offs = 0, []
        for size in (4 * cells, 2 * cells, 2 * cells, 3 * cells, 64):
            at += GUARD
            offs.append(at)
            at = (at + size + 7) & ~7
        return offs + [at + GUARD]

    def maps(self, cells):
        o = self.layout(cells)
        return PlanMaps.make(*(self.out + v for v in o[:5]))

    def upload(self, rec, in_phase=4):
        if rec.shape[0]:
            self.ctx.memcpy_h2d(self.inp + in_phase, np.ascontiguousarray(rec))
        return self.inp + in_phase

    def fetch(self, P):
        """The block back from the device: the guards checked, the five pieces cut out."""
        W, H = P["width"], P["height"]
        cells = W * H
        o = self.layout(cells)
        raw = np.empty(o[5], np.uint8)
        self.ctx.memcpy_d2h(raw, self.out)
        sizes = (4 * cells, 2 * cells, 2 * cells, 3 * cells, 64)
        edges = [0]
        for at, size in zip(o[:5], sizes):
            assert (raw[edges[-1]:at] == 0xA5).all(), "bytes between the outputs were written"
            edges.append(at + size)
        assert (raw[edges[-1]:] == 0xA5).all(), "bytes behind the statistics block were written"
        cut = lambda k, dt: raw[o[k]:o[k] + sizes[k]].copy().view(dt)
        stats = cut(4, np.int64)
        assert not stats[5:].any(), "the reserved statistics words are 0"
        return (cut(0, np.uint32).reshape(H, W), cut(1, np.int16).reshape(H, W), cut(2, np.int16).reshape(H, W), cut(3, np.uint8).reshape(H, W, 3),
                dict(zip(NP.STATS_FIELDS, (int(v) for v in stats[:5]))))

    def run(self, case, in_phase=4, d_count=None, max_points=None, extra=None, uploaded=False):
        """One call on the device forms -> (count, top, bottom, rgb, stats). extra: records behind the count of the counted form."""
        ctx = self.ctx
        rec = case.rec if extra is None else np.concatenate([case.rec, extra])
        n, cells = rec.shape[0], case.P["width"] * case.P["height"]
        assert n <= N_MAX and cells <= CELLS_MAX
        d_in = self.inp + in_phase if uploaded else self.upload(rec, in_phase)
        ctx.memcpy_h2d(self.out, np.full(self.layout(cells)[5], 0xA5, np.uint8))
        ctx.memcpy_h2d(self.words, np.array([0 if d_count is None else d_count, 0x5A5A5A5A], np.int32))
        if d_count is None:
            ctx.plan_view_device(d_in, n, c_params(case.P), self.maps(cells))
        else:
            ctx.plan_view_device_counted(d_in, self.words, max_points, c_params(case.P), self.maps(cells))
        ctx.synchronize()
        words = np.empty(2, np.int32)
        ctx.memcpy_d2h(words, self.words)
        assert words.tolist() == [0 if d_count is None else d_count, 0x5A5A5A5A]
        return self.fetch(case.P)


@pytest.fixture(scope="module")
def ctx():
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs) as c:
        yield c


@pytest.fixture(scope="module")
def arena(ctx):
    a = Arena(ctx)
    yield a
    a.free()


_GOT, _WANT = {}, {}


def gpu_maps(arena, name):
    """The plain device form's output of a case — computed once, shared, never changed."""
    if name not in _GOT:
        _GOT[name] = arena.run(K.CASES[name])
    return _GOT[name]


def want_maps(name):
    if name not in _WANT:
        _WANT[name] = NP.plan_np(K.CASES[name].rec, K.CASES[name].P)
    return _WANT[name]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


@pytest.mark.parametrize("name", NAMES)
def test_every_case_against_the_restatement(arena, name):
    got = gpu_maps(arena, name)
    NP.compare(got, want_maps(name), name)
    print(f"{name}: {got[4]}")


def test_the_wall_cells(arena):
    count, top, bottom, rgb, stats = gpu_maps(arena, "wall_equal")
    assert stats == dict(considered=65536, in_band=65536, mapped=65536, occupied=1, fullest=65536)
    cell = np.argwhere(count > 0)[0]
    rec = K.CASES["wall_equal"].rec
    assert count[tuple(cell)] == 65536 and top[tuple(cell)] == bottom[tuple(cell)] == 77
    assert rgb[tuple(cell)].tolist() == [int(rec[0, 3]) & 0xFF, (int(rec[0, 3]) >> 8) & 0xFF, int(rec[0, 4]) & 0xFF]       # index 0 wins
    count, top, bottom, rgb, stats = gpu_maps(arena, "wall_ends")
    rec = K.CASES["wall_ends"].rec
    assert count[tuple(cell)] == 65536 and top[tuple(cell)] == 78 and bottom[tuple(cell)] == 76
    assert rgb[tuple(cell)].tolist() == [int(rec[-1, 3]) & 0xFF, (int(rec[-1, 3]) >> 8) & 0xFF, int(rec[-1, 4]) & 0xFF]    # the last index is higher


def test_an_empty_map_says_so_in_count_alone(arena):
    for name in ("empty", "band_excludes_all"):
        count, top, bottom, rgb, stats = gpu_maps(arena, name)
        assert not count.any() and not top.any() and not bottom.any() and not rgb.any() and stats["occupied"] == 0 and stats["fullest"] == 0
    assert gpu_maps(arena, "band_excludes_all")[4]["considered"] == 14 and gpu_maps(arena, "band_excludes_all")[4]["in_band"] == 0


def test_both_payload_phases_and_two_runs(arena):
    for name in ("n_8193", "up_-z_corner", "raster_order", "table_overflow", "two_cells_4096"):
        want = gpu_maps(arena, name)
        for phase in (0, 2, 4, 6):
            assert same(arena.run(K.CASES[name], in_phase=phase), want), (name, phase)


def test_a_shuffled_record_order(arena):
    """The shuffled input against ITS restatement (rgb follows the lowest index of the new order); count, top and bottom against the
    unshuffled result as well."""
    for name in ("raster_order", "table_overflow", "up_+x", "wall_ends"):
        c = K.CASES[name]
        order = np.random.default_rng(12).permutation(c.rec.shape[0])
        shuffled = K.Case(c.rec[order], c.P)
        got = arena.run(shuffled)
        NP.compare(got, NP.plan_np(shuffled.rec, c.P), name + " shuffled")
        first = gpu_maps(arena, name)
        assert all(got[k].tobytes() == first[k].tobytes() for k in range(3)) and got[4] == first[4], name


def test_counted_form(arena):
    """Records behind the count are never read; counts of 0, negative and above max_points."""
    c = K.CASES["raster_order"]
    n = c.rec.shape[0]
    want = gpu_maps(arena, "raster_order")
    garbage = K.cloud(700, 99, -300, 300)
    assert same(arena.run(c, d_count=n, max_points=n + 700, extra=garbage), want)
    assert same(arena.run(c, d_count=n + 12345, max_points=n), want)              # clamped to max_points
    assert same(arena.run(c, d_count=2 ** 31 - 1, max_points=n), want)
    head = K.Case(c.rec[:2500], c.P)
    got = arena.run(c, d_count=2500, max_points=n)
    NP.compare(got, NP.plan_np(head.rec, c.P), "raster_order[:2500]")
    empty = NP.plan_np(np.zeros((0, 5), np.int16), c.P)
    for count, cap in ((0, n), (-1, n), (-2 ** 31, n), (n, 0)):
        NP.compare(arena.run(c, d_count=count, max_points=cap), empty, f"count {count} of {cap}")


def test_host_form(arena):
    for name in ("raster_order", "up_-y", "wall_ends", "empty", "grid_37x29", "borders_c32767"):
        c = K.CASES[name]
        got = arena.ctx.plan_view(c.rec, c_params(c.P))
        NP.compare(got, want_maps(name), name + " (host form)")


def test_a_small_map_after_a_large_one(arena):
    """The workspace keeps a large map's keys: the next call clears what it reads."""
    big = K.Case(K.cloud(20000, 3, -2000, 2000), NP.params(cell_mm=8, width=512, height=512))
    NP.compare(arena.run(big), NP.plan_np(big.rec, big.P), "512 x 512")
    for name in ("grid_37x29", "wave_64_cells", "one_record", "empty"):
        assert same(arena.run(K.CASES[name]), gpu_maps(arena, name)), name
        NP.compare(arena.run(K.CASES[name]), want_maps(name), name)


def test_fed_from_the_cluster_filter(arena):
    """pcs_cluster_filter_device_counted -> pcs_plan_view_device_counted with no host round trip in between."""
    ctx = arena.ctx
    rng = np.random.default_rng(5)
    blobs = np.concatenate([rng.integers(-15, 16, (400, 3)) + centre for centre in ((-200, 0, 50), (150, 120, 0), (0, -250, -40))] +
                           [rng.integers(-1000, 1000, (150, 3))])
    rec = K.records(blobs[rng.permutation(blobs.shape[0])], 5)
    n = rec.shape[0]
    P = NP.params(cell_mm=10, width=64, height=64)
    d_mid = ctx.device_malloc(10 * n + 64)
    d_n = ctx.device_malloc(64)
    try:
        d_in = arena.upload(rec)
        ctx.memcpy_h2d(arena.words, np.array([n, 0], np.int32))
        ctx.memcpy_h2d(arena.out, np.full(arena.layout(64 * 64)[5], 0xA5, np.uint8))
        ctx.cluster_filter_device_counted(d_in, arena.words, n, ClusterParams.make(12, 100, 0), d_mid, 5 * n, d_n, 0)
        ctx.plan_view_device_counted(d_mid, d_n, n, c_params(P), arena.maps(64 * 64))
        ctx.synchronize()
        kept_n = np.empty(1, np.int32)
        ctx.memcpy_d2h(kept_n, d_n)
        kept = np.empty((int(kept_n[0]), 5), np.int16)
        ctx.memcpy_d2h(kept, d_mid)
    finally:
        ctx.device_free(d_mid)
        ctx.device_free(d_n)
    assert 1000 <= kept.shape[0] < n                       # the three blobs stay, the scattered records go
    NP.compare(arena.fetch(P), NP.plan_np(kept, P), "behind the cluster filter")


def test_a_stitched_frame_set(arena):
    """Eight synthetic 64 x 48 streams through a context of their own, the payload never leaving the device."""
    cfgs, depth, color = S.synth_frame_set(8, 64, 48)
    with PcsContext(cfgs) as ctx8:
        buf, counts, size = ctx8.process_frames(depth, color, write_header=True)
        rec = np.ascontiguousarray(buf[2:2 + size // 2].reshape(-1, 5))
        assert rec.shape[0] == 8 * 64 * 48
        for up, cell in (("+y", 50), ("-z", 20)):
            P = NP.params(up=up, cell_mm=cell, width=128, height=96)
            got = ctx8.plan_view(rec, c_params(P))
            NP.compare(got, NP.plan_np(rec, P), f"stitched {up}")
            assert got[4]["occupied"] > 10
    case = K.Case(rec, NP.params(up="+y", cell_mm=50, width=128, height=96))
    NP.compare(arena.run(case), NP.plan_np(rec, case.P), "stitched, device form")


def test_working_size(arena):
    """2^20 records over 400 x 400 cells with a 100 000-record column in one cell."""
    case = K.working_size()
    want = NP.plan_np(case.rec, case.P)
    assert want[4]["fullest"] >= 100000 and want[4]["occupied"] > 150000
    NP.compare(arena.run(case), want, "working size")
    NP.compare(arena.run(case, in_phase=2, uploaded=False), want, "working size, phase 2")


def test_kernel_timing_counts_the_launches(arena):
    """One finite interval >= 0 per launch: every call 3 in all three forms, whatever the counts — and timing changes no byte."""
    ctx = arena.ctx
    c = K.CASES["raster_order"]
    want = gpu_maps(arena, "raster_order")
    ctx.synchronize()
    ctx.kernel_times_ms()
    ctx.kernel_timing(True)
    try:
        def launches(fn):
            out = fn()
            ctx.synchronize()
            t = ctx.kernel_times_ms()
            assert np.isfinite(t).all() and (t >= 0).all()
            return t.shape[0], out
        k, got = launches(lambda: arena.run(c))
        assert k == len(PLAN_VIEW_LAUNCHES) == 3 and same(got, want)
        assert launches(lambda: arena.run(c, d_count=100, max_points=c.rec.shape[0]))[0] == 3
        assert launches(lambda: arena.run(K.CASES["empty"]))[0] == 3
        assert launches(lambda: arena.run(c, d_count=5, max_points=0))[0] == 3
        k, got = launches(lambda: ctx.plan_view(c.rec, c_params(c.P)))
        assert k == 3 and same(got, want)
    finally:
        ctx.kernel_timing(False)


def test_refusals_launch_nothing_and_write_nothing(arena):
    ctx = arena.ctx
    c = K.CASES["grid_37x29"]
    n, cells = c.rec.shape[0], 37 * 29
    arena.run(c)
    d_in, d_n = arena.inp + 4, arena.words
    block = arena.layout(cells)[5]
    ctx.memcpy_h2d(arena.out, np.full(block, 0xA5, np.uint8))
    ctx.memcpy_h2d(arena.words, np.array([n, 7], np.int32))
    ctx.synchronize()
    ctx.kernel_times_ms()
    ctx.kernel_timing(True)
    good, m = c_params(c.P), arena.maps(cells)
    too_many = (2 ** 31 - 1) // 10 + 1

    def changed(**kw):
        P = dict(c.P)
        reserved = kw.pop("reserved", (0, 0, 0))
        P.update(kw)
        return c_params(P, reserved)

    def moved(**kw):
        fields = {name: getattr(m, name) or 0 for name, _ in PlanMaps._fields_}
        fields.update(kw)
        return PlanMaps.make(**fields)

    bad_params = [(changed(up_axis=3), "up_axis"), (changed(up_axis=-1), "up_axis"), (changed(up_sign=0), "up_sign"), (changed(up_sign=2), "up_sign"),
                  (changed(cell_mm=0), "cell_mm"), (changed(cell_mm=32768), "cell_mm"), (changed(origin_u=-32769), "origin_u"),
                  (changed(origin_u=32768), "origin_u"), (changed(origin_v=-32769), "origin_v"), (changed(origin_v=32768), "origin_v"),
                  (changed(width=0), "width"), (changed(width=4097), "width"), (changed(height=0), "height"), (changed(height=4097), "height"),
                  (changed(width=4096, height=1025), "height"), (changed(band_lo=-32769), "band_lo"), (changed(band_hi=32768), "band_hi"),
                  (changed(band_lo=5, band_hi=4), "band_hi"), (changed(reserved=(1, 0, 0)), "reserved[0]"), (changed(reserved=(0, 0, 9)), "reserved[2]")]
    bad_maps = [(moved(count=0), "maps->count"), (moved(count=m.count + 2), "maps->count"), (moved(top=0), "maps->top"),
                (moved(top=m.top + 1), "maps->top"), (moved(bottom=0), "maps->bottom"), (moved(bottom=m.bottom + 1), "maps->bottom"),
                (moved(rgb=0), "maps->rgb"), (moved(stats=0), "maps->stats"), (moved(stats=m.stats + 4), "maps->stats"),
                (moved(count=d_in + 4), "overlaps"), (moved(rgb=d_in + 10 * n - 1), "overlaps"), (moved(top=m.count + 4), "overlaps"),
                (moved(stats=m.rgb + 3 * cells - 1 - (m.rgb + 3 * cells - 1) % 8), "overlaps"), (moved(bottom=m.top + 2 * cells - 2), "overlaps")]
    plain = [((d_in, -1, good, m), "n_points"), ((d_in, too_many, good, m), "n_points"), ((0, n, good, m), "d_payload"),
             ((d_in + 1, n, good, m), "d_payload"), ((d_in, n, None, m), "params"), ((d_in, n, good, None), "maps")]
    plain += [((d_in, n, p, m), word) for p, word in bad_params] + [((d_in, n, good, mm), word) for mm, word in bad_maps]
    for args, word in plain:
        with pytest.raises(PcsError) as e:
            ctx.plan_view_device(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_plan_view_device:" in str(e.value), (word, str(e.value))
    counted = [((d_in, 0, n, good, m), "d_n_points"), ((d_in, d_n + 2, n, good, m), "d_n_points"), ((d_in, d_n, -1, good, m), "max_points"),
               ((d_in, d_n, too_many, good, m), "max_points"), ((0, d_n, n, good, m), "d_payload"), ((d_in, d_n, n, changed(cell_mm=-4), m), "cell_mm"),
               ((d_in, d_n, n, good, moved(top=m.top + 1)), "maps->top"), ((d_in, d_n, n, good, moved(count=d_n)), "overlaps"),
               ((d_in, d_n, n, good, moved(stats=d_n - 8)), "overlaps")]
    for args, word in counted:
        with pytest.raises(PcsError) as e:
            ctx.plan_view_device_counted(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_plan_view_device_counted:" in str(e.value), (word, str(e.value))
    # the host form
    lib, h = ctx._lib, ctx._h
    p = np.ascontiguousarray(c.rec)
    host = np.full(16 * cells + 128, 0x5A, np.uint8)
    base = host.ctypes.data + (-host.ctypes.data) % 8
    hm = PlanMaps.make(base, base + 4 * cells + 4, base + 6 * cells + 8, base + 8 * cells + 12, base + 11 * cells + 16 + (-(11 * cells)) % 8)
    hmoved = lambda **kw: PlanMaps.make(**{**{name: getattr(hm, name) or 0 for name, _ in PlanMaps._fields_}, **kw})
    for args, word in (((p.ctypes.data, -3, C.byref(good), C.byref(hm)), "n_points"), ((None, n, C.byref(good), C.byref(hm)), "payload"),
                       ((p.ctypes.data + 1, n, C.byref(good), C.byref(hm)), "payload"), ((p.ctypes.data, n, None, C.byref(hm)), "params"),
                       ((p.ctypes.data, n, C.byref(good), None), "maps"), ((p.ctypes.data, n, C.byref(changed(cell_mm=40000)), C.byref(hm)), "cell_mm"),
                       ((p.ctypes.data, n, C.byref(good), C.byref(hmoved(count=0))), "maps->count"),
                       ((p.ctypes.data, n, C.byref(good), C.byref(hmoved(stats=hm.stats + 2))), "maps->stats"),
                       ((p.ctypes.data, n, C.byref(good), C.byref(hmoved(rgb=p.ctypes.data + 16))), "overlaps"),
                       ((p.ctypes.data, n, C.byref(good), C.byref(hmoved(bottom=hm.top + 2))), "overlaps")):
        assert lib.pcs_plan_view(h, *args) == -1
        text = lib.pcs_last_error(h).decode()
        assert word in text and "pcs_plan_view:" in text, text
    assert (host == 0x5A).all()
    ctx.synchronize()
    assert ctx.kernel_times_ms().shape[0] == 0                      # nothing was launched
    ctx.kernel_timing(False)
    out = np.empty(block, np.uint8)
    words = np.empty(2, np.int32)
    ctx.memcpy_d2h(out, arena.out)
    ctx.memcpy_d2h(words, arena.words)
    assert (out == 0xA5).all() and words.tolist() == [n, 7]
    assert same(arena.run(c), gpu_maps(arena, "grid_37x29"))       # ... and the next call is what it was
