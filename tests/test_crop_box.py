"""The world-frame crop box (pcs_set_crop_box_mm, pcs_crop_payloads_device) against an independent restatement: the CPU oracle's
UNCROPPED cloud, split by its per-stream counts, masked with numpy on columns 0..2, every d-th kept row per stream, concatenated.
The box is defined on the record's three shorts (after the int16 wrap), so that restatement is exact."""
import ctypes as C

import numpy as np
import pytest

from pointcloud_stitching_amd import lib as L
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import (FLAG_CUTOFF, FLAG_CUTOFF_COMPAT, FLAG_DROP_INVALID, FLAG_FORCE_IEEE, FLAG_SCALAR_ARITH,
                                            HEADER_SHORTS, TRANSFORMS, make_intrinsics, make_stream_config)

BOX_A = ((-1100, 0, -1100), (1100, 2000, 300))
BOX_B = ((-2300, 2850, 300), (-2150, 3000, 450))        # holds stream 0's camera position, where invalid pixels pack to
BOX_E = ((-32768, -32768, -200), (32767, 32767, -200))  # a single plane
BOX_FULL = ((-32768,) * 3, (32767,) * 3)
CC = FLAG_CUTOFF | FLAG_CUTOFF_COMPAT

_frames, _uncropped = {}, {}


def frames(n, w, h):
    """S.synth_frame_set(n, w, h) with rows [100h/480, 140h/480) of each depth integer-divided by 4 (computed once, never changed)."""
    if (n, w, h) not in _frames:
        cfgs, depth, color = S.synth_frame_set(n, w, h)
        for d in depth:
            d[100 * h // 480:140 * h // 480, :] //= 4
        _frames[(n, w, h)] = (cfgs, depth, color)
    return _frames[(n, w, h)]


def uncropped(oracle, key, cfgs, depth, color, flags):
    if (key, flags) not in _uncropped:
        _uncropped[(key, flags)] = oracle.process_frames(cfgs, depth, color, flags, 1)
    return _uncropped[(key, flags)]


def mask_rows(part, box):
    lo, hi = np.array(box[0], np.int32), np.array(box[1], np.int32)
    xyz = part[:, :3].astype(np.int32)
    return ((xyz >= lo) & (xyz <= hi)).all(axis=1)


def reference(oracle, key, cfgs, depth, color, flags, box, ds):
    """(cropped cloud, counts written per stream, kept per stream before the stride, uncropped total)."""
    full, counts = uncropped(oracle, key, cfgs, depth, color, flags)
    out, written, kept, o = [], [], [], 0
    for c in counts:
        part = full[o:o + c]
        o += c
        m = mask_rows(part, box) if box is not None else np.ones(c, bool)
        rows = part[m][::ds]
        out.append(rows)
        written.append(rows.shape[0])
        kept.append(int(m.sum()))
    return np.concatenate(out).reshape(-1, 5), written, kept, full.shape[0]


def ref_frames(oracle, n, w, h, flags, box, ds):
    return reference(oracle, (n, w, h), *frames(n, w, h), flags, box, ds)


def assert_same(got, want):
    got, want = np.asarray(got).reshape(-1, 5), np.asarray(want).reshape(-1, 5)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {want.shape[0]} records differ, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def host_run(ctx, depth, color):
    buf, counts, size = ctx.process_frames(depth, color, write_header=True)
    assert size == 10 * sum(counts)
    assert int.from_bytes(buf[:2].tobytes(), "little", signed=True) == size
    return buf[HEADER_SHORTS:HEADER_SHORTS + 5 * sum(counts)].reshape(-1, 5), counts


class Dev:
    """Rasters of a frame-set on the device, a payload buffer and a counts buffer."""

    def __init__(self, ctx, depth, color, payload_shorts=None, n_counts=None):
        self.ctx = ctx
        self.dd = [ctx.device_malloc(max(d.nbytes, 16)) for d in depth]
        self.dc = [ctx.device_malloc(max(c.nbytes, 16)) for c in color]
        for p, a in zip(self.dd + self.dc, list(depth) + list(color)):
            ctx.memcpy_h2d(p, np.ascontiguousarray(a))
        self.shorts = payload_shorts if payload_shorts is not None else ctx.max_payload_shorts
        self.out = ctx.device_malloc(self.shorts * 2 + 64)
        self.n_counts = n_counts if n_counts is not None else ctx.n_streams + 1
        self.cnt = ctx.device_malloc(4 * self.n_counts)

    def fill(self, value, skew=0):
        self.ctx.memcpy_h2d(self.out + skew, np.full(self.shorts, value, np.int16))

    def run(self, skew=0):
        self.ctx.process_frames_device(self.dd, self.dc, self.out + skew, self.shorts, self.cnt)

    def counts(self):
        self.ctx.synchronize()
        c = np.empty(self.n_counts, np.int32)
        self.ctx.memcpy_d2h(c, self.cnt)
        return [int(x) for x in c]

    def payload(self, shorts=None, skew=0):
        self.ctx.synchronize()
        got = np.empty(self.shorts if shorts is None else shorts, np.int16)
        if got.size:
            self.ctx.memcpy_d2h(got, self.out + skew)
        return got

    def result(self, skew=0):
        c = self.counts()
        assert c[-1] == sum(c[:-1])
        return self.payload(5 * c[-1], skew).reshape(-1, 5), c[:-1]


# ---------------------------------------------------------------------------------------------
# the helper itself (no GPU): the kept counts the issue states for 3 x 640x480
# ---------------------------------------------------------------------------------------------
TABLE = [(BOX_A, 0, [27515, 68134, 27941]), (BOX_A, FLAG_DROP_INVALID, [27515, 68134, 27941]), (BOX_A, FLAG_CUTOFF, [0, 26541, 76]),
         (BOX_A, CC, [48, 23855, 129]), (BOX_B, 0, [34757, 0, 0]), (BOX_B, CC, [8553, 0, 0]), (BOX_B, FLAG_DROP_INVALID, [0, 0, 0]),
         (BOX_E, 0, [117, 132, 133])]


def test_reference_helper_reproduces_the_stated_counts(oracle):
    for box, flags, want in TABLE:
        assert ref_frames(oracle, 3, 640, 480, flags, box, 1)[2] == want, (box, flags)
    assert ref_frames(oracle, 3, 321, 243, 0, BOX_A, 1)[2] == [5909, 15937, 6585]
    assert ref_frames(oracle, 2, 64, 48, 0, BOX_A, 1)[2] == [166, 221]
    assert sum(ref_frames(oracle, 2, 64, 48, 0, BOX_E, 1)[2]) == 0
    # the stride runs over the KEPT rows of each stream
    rows, written, kept, _ = ref_frames(oracle, 3, 640, 480, 0, BOX_A, 3)
    assert written == [(k + 2) // 3 for k in kept] and rows.shape[0] == sum(written)


# ---------------------------------------------------------------------------------------------
# 1. the fused path
# ---------------------------------------------------------------------------------------------
PAIRS = [(BOX_A, 0), (BOX_A, FLAG_DROP_INVALID), (BOX_A, FLAG_CUTOFF), (BOX_A, CC), (BOX_A, FLAG_CUTOFF | FLAG_DROP_INVALID),
         (BOX_B, 0), (BOX_B, CC), (BOX_E, 0), (BOX_E, FLAG_DROP_INVALID)]


# (the plane E holds no point of the 64x48 frame-set: not a case there)
CASES = [(shape, box, flags) for shape in [(3, 640, 480), (3, 321, 243), (2, 64, 48)] for box, flags in PAIRS
         if not (box is BOX_E and shape == (2, 64, 48))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,box,flags", CASES)
def test_fused_path_against_the_reference(oracle, shape, box, flags):
    cfgs, depth, color = frames(*shape)
    for ds in (1, 3):
        want, wcounts, _, total = ref_frames(oracle, *shape, flags, box, ds)
        assert 0 < sum(wcounts) < total
        with PcsContext(cfgs, flags=flags, downsample=ds) as ctx:
            ctx.set_crop_box_mm(*box)
            got, counts = host_run(ctx, depth, color)
        assert counts == wcounts, (ds, counts, wcounts)
        assert_same(got, want)


# ---------------------------------------------------------------------------------------------
# 2. empty, full, set and clear
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_result_writes_nothing(oracle):
    cfgs, depth, color = frames(3, 640, 480)
    assert sum(ref_frames(oracle, 3, 640, 480, FLAG_DROP_INVALID, BOX_B, 1)[1]) == 0
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        ctx.set_crop_box_mm(*BOX_B)
        dev = Dev(ctx, depth, color)
        dev.fill(0x5A5A)
        dev.run()
        assert dev.counts() == [0, 0, 0, 0]
        assert (dev.payload() == 0x5A5A).all()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, FLAG_DROP_INVALID])
def test_full_range_box_and_set_then_clear(oracle, flags):
    cfgs, depth, color = frames(3, 321, 243)
    want, wcounts = uncropped(oracle, (3, 321, 243), cfgs, depth, color, flags)
    with PcsContext(cfgs, flags=flags) as fresh:
        plain, pcounts = host_run(fresh, depth, color)
    assert pcounts == wcounts
    with PcsContext(cfgs, flags=flags) as ctx:
        assert ctx.crop_box_mm() is None
        ctx.set_crop_box_mm(*BOX_FULL)
        assert ctx.crop_box_mm() == BOX_FULL
        got, counts = host_run(ctx, depth, color)
        assert counts == pcounts
        assert_same(got, plain)
        ctx.set_crop_box_mm(*BOX_A)
        assert ctx.crop_box_mm() == BOX_A
        assert sum(host_run(ctx, depth, color)[1]) < sum(pcounts)
        ctx.set_crop_box_mm(None, None)
        assert ctx.crop_box_mm() is None
        got, counts = host_run(ctx, depth, color)
        assert counts == pcounts
        assert_same(got, plain)


# ---------------------------------------------------------------------------------------------
# 3. the box changes between calls
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_box_changes_between_calls(oracle):
    cfgs, depth, color = frames(3, 640, 480)
    with PcsContext(cfgs) as ctx:
        dev = Dev(ctx, depth, color)
        for box in (BOX_A, BOX_B, None, BOX_A):
            if box is None:
                ctx.set_crop_box_mm(None, None)
            else:
                ctx.set_crop_box_mm(*box)
            want, wcounts, _, _ = ref_frames(oracle, 3, 640, 480, 0, box, 1)
            dev.run()
            got, counts = dev.result()
            assert counts == wcounts
            assert_same(got, want)
            got, counts = host_run(ctx, depth, color)
            assert counts == wcounts
            assert_same(got, want)


# ---------------------------------------------------------------------------------------------
# 4. the device call: payload skews, idempotence, d_counts, capacity
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_call_skews_idempotence_counts_capacity(oracle):
    cfgs, depth, color = frames(3, 640, 480)
    want, wcounts, _, _ = ref_frames(oracle, 3, 640, 480, 0, BOX_A, 1)
    with PcsContext(cfgs) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        dev = Dev(ctx, depth, color)
        for skew in (0, 4, 2, 10):
            dev.run(skew)
            dev.run(skew)
            got, counts = dev.result(skew)
            assert counts == wcounts
            assert_same(got, want)
        with pytest.raises(PcsError) as e:
            ctx.process_frames_device(dev.dd, dev.dc, dev.out, ctx.max_payload_shorts - 5, dev.cnt)
        assert e.value.status == -5


# ---------------------------------------------------------------------------------------------
# 5. every host route
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_routes_pageable_page_locked_and_pipelined(oracle):
    cfgs, depth, color = frames(3, 640, 480)
    want, wcounts, _, _ = ref_frames(oracle, 3, 640, 480, 0, BOX_A, 1)
    with PcsContext(cfgs) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        got, counts = host_run(ctx, depth, color)                   # pageable: staged
        assert counts == wcounts
        assert_same(got, want)
        pd = [ctx.host_array(d.shape, np.uint16) for d in depth]    # page-locked on every side: zero copy
        pc = [ctx.host_array(c.shape, np.uint8) for c in color]
        for a, b in zip(pd + pc, depth + color):
            a[...] = b
        out = ctx.host_array((HEADER_SHORTS + ctx.max_payload_shorts,), np.int16)
        out[:] = 0
        buf, counts, size = ctx.process_frames(pd, pc, out=out)
        assert counts == wcounts and size == 10 * sum(wcounts)
        assert_same(buf[HEADER_SHORTS:HEADER_SHORTS + 5 * sum(counts)], want)
        t0 = ctx.submit_frames(depth, color)                        # two deep
        t1 = ctx.submit_frames(depth, color)
        for t in (t0, t1):
            buf, counts, size = ctx.collect_frames(t)
            assert counts == wcounts and size == 10 * sum(wcounts)
            assert_same(buf[HEADER_SHORTS:HEADER_SHORTS + 5 * sum(counts)], want)


@pytest.mark.gpu
def test_box_changed_between_submit_and_collect(oracle):
    """A frame-set is collected as it was SUBMITTED: the setter between the two calls must change neither its counts nor its bytes
    (nothing enqueued earlier sees the change), in either direction."""
    cfgs, depth, color = frames(3, 640, 480)
    want_a, counts_a, _, _ = ref_frames(oracle, 3, 640, 480, 0, BOX_A, 1)
    want_0, counts_0, _, _ = ref_frames(oracle, 3, 640, 480, 0, None, 1)
    assert 0 < sum(counts_a) < sum(counts_0)

    def collect(ctx, t, want, wcounts):
        buf, counts, size = ctx.collect_frames(t)
        assert counts == wcounts and size == 10 * sum(wcounts)
        assert int.from_bytes(buf[:2].tobytes(), "little", signed=True) == size
        assert_same(buf[HEADER_SHORTS:HEADER_SHORTS + size // 2], want)

    with PcsContext(cfgs) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        t0 = ctx.submit_frames(depth, color)                        # two deep under box A ...
        t1 = ctx.submit_frames(depth, color)
        ctx.set_crop_box_mm(None, None)                             # ... cleared before either is collected
        collect(ctx, t0, want_a, counts_a)
        collect(ctx, t1, want_a, counts_a)
        t0 = ctx.submit_frames(depth, color)                        # the reverse: submitted without a box (into the slots the
        t1 = ctx.submit_frames(depth, color)                        # cropped frame-sets used), box A set before the collect
        ctx.set_crop_box_mm(*BOX_A)
        collect(ctx, t0, want_0, counts_0)
        t2 = ctx.submit_frames(depth, color)                        # and one submitted under the box while an unboxed one is in flight
        collect(ctx, t1, want_0, counts_0)
        collect(ctx, t2, want_a, counts_a)


# ---------------------------------------------------------------------------------------------
# 6. batch
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, FLAG_DROP_INVALID])
def test_batch_equals_single_calls(oracle, flags):
    shapes = [(1280, 720), (321, 243), (64, 48), (640, 480)]
    n_sets = 5
    cfgs = [S.synth_stream_config(w, h, s) for s, (w, h) in enumerate(shapes)]
    sets = []
    for k in range(n_sets):
        depth = [S.synth_depth(w, h, 10 * k + s) for s, (w, h) in enumerate(shapes)]
        for d, (w, h) in zip(depth, shapes):
            d[100 * h // 480:140 * h // 480, :] //= 4
        sets.append((depth, [S.synth_color(w, h, 10 * k + s) for s, (w, h) in enumerate(shapes)]))
    with PcsContext(cfgs, flags=flags) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        devs = [Dev(ctx, d, c) for d, c in sets]
        singles = []
        for dev in devs:
            dev.run()
            singles.append(dev.result())
            dev.fill(0)
            ctx.memcpy_h2d(dev.cnt, np.full(dev.n_counts, -1, np.int32))
        assert all(0 < sum(c) < sum(cf.n_points for cf in cfgs) for _, c in singles)
        ctx.process_frames_device_batch([d.dd for d in devs], [d.dc for d in devs], [d.out for d in devs], ctx.max_payload_shorts,
                                        [d.cnt for d in devs])
        for dev, (want, wcounts) in zip(devs, singles):
            got, counts = dev.result()
            assert counts == wcounts
            assert_same(got, want)
    # and the single calls are the reference's
    want, wcounts, _, _ = reference(oracle, ("batch", 0), cfgs, *sets[0], flags, BOX_A, 1)
    assert singles[0][1] == wcounts
    assert_same(singles[0][0], want)


# ---------------------------------------------------------------------------------------------
# 7. count and emit agree where the coordinates wrap and where the conversion is redone
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tx,box", [(40.0, ((-27000, -32768, -32768), (-24500, 32767, 32767))),      # 40 m: the shorts wrap
                                    (3.0e6, ((0, -32768, -32768), (0, 32767, 32767)))])              # 3000 km: ExactCvt's INT_MIN -> 0
def test_wrapped_and_redone_coordinates(oracle, tx, box):
    cfgs, depth, color = S.synth_frame_set(2, 64, 48)
    cfgs[1].cam_to_world[3] = tx
    full, fcounts = oracle.process_frames(cfgs, depth, color, 0, 1)
    want, wcounts, _, total = reference(oracle, ("wrap", tx), cfgs, depth, color, 0, box, 1)
    assert wcounts[1] > 0 and sum(wcounts) < total          # the box holds points of the moved stream, and not every point
    for flags in (0, FLAG_FORCE_IEEE):
        with PcsContext(cfgs, flags=flags) as ctx:
            ctx.set_crop_box_mm(*box)
            got, counts = host_run(ctx, depth, color)
        assert counts == wcounts
        assert_same(got, want)


def _random_config(rng, w, h, cw, ch, wild):
    f = rng.uniform(0.5, 1.5) * w
    di = make_intrinsics(w, h, f, f * rng.uniform(0.98, 1.02), w / 2 + rng.uniform(-20, 20), h / 2 + rng.uniform(-20, 20))
    fc = rng.uniform(0.5, 1.5) * cw
    cdist = rng.random() < 0.3
    ci = make_intrinsics(cw, ch, fc, fc * rng.uniform(0.98, 1.02), cw / 2 + rng.uniform(-20, 20), ch / 2 + rng.uniform(-20, 20),
                         model=1 if cdist else 0, coeffs=list(rng.normal(0, 0.02, 5)) if cdist else None)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = 0.0 if rng.random() < 0.3 else rng.normal(0, 0.6 if wild else 0.02)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    t = rng.normal(0, 0.5 if wild else 0.02, 3)
    if rng.random() < 0.3:
        t[rng.integers(0, 3)] = 0.0
    scale = float(10.0 ** rng.uniform(-4, -2)) if wild else 0.001
    m = TRANSFORMS[rng.integers(0, 8)].copy()
    return make_stream_config(di, ci, cam_to_world=m, rotation=list(Rm.T.reshape(-1)), translation=list(t), depth_scale=scale)


@pytest.mark.gpu
@pytest.mark.parametrize("wild", [False, True])
def test_fuzzed_rigs_both_policies(oracle, wild):
    """Random rigs, the box from the 25th and 75th percentiles of the reference's own uncropped columns: under the policy the
    certificate picks and under the forced IEEE one, the count pass and the emit pass must agree with each other and with numpy."""
    rng = np.random.default_rng(4242 + wild)
    shares = []
    for trial in range(16):
        w, h = [(64, 48), (128, 96), (104, 40), (200, 37)][trial % 4]
        cw, ch = [(64, 48), (192, 108), (100, 75), (320, 180)][(trial // 4) % 4]
        sc = _random_config(rng, w, h, cw, ch, wild)
        depth = S.synth_depth(w, h, trial, mode="random" if trial % 3 == 0 else "scene")
        color = S.synth_color(cw, ch, trial)
        full, _ = oracle.process_frames([sc], [depth], [color], 0, 1)
        lo = [int(np.percentile(full[:, a], 25)) for a in range(3)]
        hi = [int(np.percentile(full[:, a], 75)) for a in range(3)]
        m = mask_rows(full, (lo, hi))
        assert 0 < m.sum() < full.shape[0]
        shares.append(m.mean())
        ds = 1 + trial % 3
        want = full[m][::ds]
        for flags in (0, FLAG_FORCE_IEEE):
            with PcsContext([sc], flags=flags, downsample=ds) as ctx:
                ctx.set_crop_box_mm(lo, hi)
                got, counts = host_run(ctx, [depth], [color])
            assert counts == [want.shape[0]], (trial, flags)
            assert_same(got, want)


# ---------------------------------------------------------------------------------------------
# 8. the centre side
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_centre_side_crop_of_packed_payloads(oracle):
    cfgs, depth, color = frames(3, 640, 480)
    full, fcounts = uncropped(oracle, (3, 640, 480), cfgs, depth, color, 0)
    parts = [full[0:fcounts[0]], full[:0], full[fcounts[0]:fcounts[0] + fcounts[1]], full[fcounts[0] + fcounts[1]:][:2049],
             full[fcounts[0] + fcounts[1]:]]
    n = [p.shape[0] for p in parts]
    assert n[1] == 0 and n[3] == 2049
    with PcsContext(cfgs) as ctx:
        src = [ctx.device_malloc(p.nbytes + 64) for p in parts]
        for ptr, p in zip(src, parts):
            if p.size:
                ctx.memcpy_h2d(ptr + 4, np.ascontiguousarray(p))
        ins = [ptr + 4 for ptr in src]
        shorts = 5 * sum(n)
        out = ctx.device_malloc(2 * shorts + 64)
        cnt = ctx.device_malloc(4 * (len(parts) + 1))

        def crop(ds, skew=4):
            ctx.crop_payloads_device(ins, n, ds, out + skew, shorts, cnt)
            ctx.crop_payloads_device(ins, n, ds, out + skew, shorts, cnt)      # idempotent
            ctx.synchronize()
            c = np.empty(len(parts) + 1, np.int32)
            ctx.memcpy_d2h(c, cnt)
            got = np.empty(5 * int(c[-1]), np.int16)
            if got.size:
                ctx.memcpy_d2h(got, out + skew)
            assert int(c[-1]) == int(c[:-1].sum())
            return got.reshape(-1, 5), [int(x) for x in c[:-1]]

        # no box: pcs_stitch_device's bytes
        for ds in (1, 3):
            want = oracle.stitch(parts, ds)
            got, counts = crop(ds)
            assert counts == [(k + ds - 1) // ds for k in n]
            assert_same(got, want)
            total = ctx.stitch_device(ins, n, ds, out, shorts)
            ctx.synchronize()
            st = np.empty(5 * total, np.int16)
            ctx.memcpy_d2h(st, out)
            assert_same(st, got)
        ctx.set_crop_box_mm(*BOX_A)
        for ds in (1, 2, 7):
            rows = [p[mask_rows(p, BOX_A)][::ds] for p in parts]
            got, counts = crop(ds, skew=(0, 4, 10)[ds % 3])
            assert counts == [r.shape[0] for r in rows]
            assert_same(got, np.concatenate(rows))
            assert 0 < sum(counts) < sum(n)
        # ... and what the fused path writes for the same box and stride (cameras = the three streams)
        three = [parts[0], parts[2], parts[4]]
        ins3, n3 = [ins[0], ins[2], ins[4]], [n[0], n[2], n[4]]
        for ds in (1, 2, 7):
            ctx.crop_payloads_device(ins3, n3, ds, out + 4, shorts, cnt)
            ctx.synchronize()
            c = np.empty(4, np.int32)
            ctx.memcpy_d2h(c, cnt)
            got = np.empty(5 * int(c[3]), np.int16)
            ctx.memcpy_d2h(got, out + 4)
            with PcsContext(cfgs, downsample=ds) as edge:
                edge.set_crop_box_mm(*BOX_A)
                fused, fc = host_run(edge, depth, color)
            assert [int(x) for x in c[:3]] == fc
            assert_same(got, fused)
        # refusals: overlap of an input with the output, capacity below the worst case
        with pytest.raises(PcsError) as e:
            ctx.crop_payloads_device(ins, n, 1, ins[2] + 10 * 100, shorts, cnt)
        assert e.value.status == -1 and "overlap" in str(e.value)
        with pytest.raises(PcsError) as e:
            ctx.crop_payloads_device(ins, n, 1, out, shorts - 5, cnt)
        assert e.value.status == -5


@pytest.mark.gpu
def test_centre_side_crop_second_pass_of_the_scan():
    """One camera of 2 099 201 records = 1026 tiles: the per-camera scan of pcs_crop_payloads_device carries its running total into a
    second pass of 1024 tiles. Random records over the whole int16 range, a box that keeps about half of them, every third kept
    record written."""
    n, ds = 2099201, 3
    box = ((-32768, -20000, -32768), (32767, 32767, 7000))
    rng = np.random.default_rng(41)
    rec = rng.integers(-32768, 32768, (n, 5)).astype(np.int16)
    keep = mask_rows(rec, box)
    want = rec[keep][::ds]
    assert 0.4 * n < keep.sum() < 0.6 * n and 0 < keep[:1024 * 2048].sum() < keep.sum()
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs) as ctx:
        ctx.set_crop_box_mm(*box)
        src = ctx.device_malloc(rec.nbytes + 64)
        ctx.memcpy_h2d(src + 4, rec)
        out = ctx.device_malloc(rec.nbytes + 64)
        cnt = ctx.device_malloc(4 * 2)
        ctx.crop_payloads_device([src + 4], [n], ds, out + 4, 5 * n, cnt)
        ctx.synchronize()
        c = np.empty(2, np.int32)
        ctx.memcpy_d2h(c, cnt)
        assert list(c) == [want.shape[0], want.shape[0]]
        got = np.empty((want.shape[0], 5), np.int16)
        ctx.memcpy_d2h(got, out + 4)
        assert_same(got, want)


# ---------------------------------------------------------------------------------------------
# 9. crop, then voxel
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_crop_then_voxel_grid(oracle):
    cfgs, depth, color = frames(2, 64, 48)
    cropped, wcounts, _, total = ref_frames(oracle, 2, 64, 48, 0, BOX_A, 1)
    want = oracle.voxel_grid(cropped, 50)
    assert 0 < want.shape[0] < cropped.shape[0]
    n_max = sum(c.n_points for c in cfgs)
    with PcsContext(cfgs) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        dev = Dev(ctx, depth, color)
        d_vox = ctx.device_malloc(n_max * 10 + 64)
        d_nv = ctx.device_malloc(4)

        def voxels():
            ctx.synchronize()
            nv = np.empty(1, np.int32)
            ctx.memcpy_d2h(nv, d_nv)
            got = np.empty(5 * int(nv[0]), np.int16)
            ctx.memcpy_d2h(got, d_vox)
            return got.reshape(-1, 5)

        ctx.process_frames_voxel_device(dev.dd, dev.dc, 50, d_vox, n_max * 5, d_nv)
        assert_same(voxels(), want)
        ctx.memcpy_h2d(d_nv, np.zeros(1, np.int32))
        dev.run()
        ctx.voxel_grid_device_counted(dev.out, dev.cnt + 4 * 2, n_max, 50, d_vox, n_max * 5, d_nv)
        assert_same(voxels(), want)


@pytest.mark.gpu
def test_crop_then_voxel_partials_and_sink(oracle):
    """The other two voxel entries that start from rasters, with a box set: partials (then the grid from them) and the sink."""
    cfgs, depth, color = frames(2, 64, 48)
    cropped, _, _, _ = ref_frames(oracle, 2, 64, 48, 0, BOX_A, 1)
    want = oracle.voxel_grid(cropped, 50)
    assert 0 < want.shape[0] < cropped.shape[0]
    with PcsContext(cfgs) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        dev = Dev(ctx, depth, color)
        cap = ctx.max_payload_shorts // 5
        d_keys, d_parts = ctx.device_malloc(cap * 8 + 64), ctx.device_malloc(cap * 32 + 64)
        d_np, d_nv = ctx.device_malloc(64), ctx.device_malloc(64)
        d_vox = ctx.device_malloc(cap * 10 + 64)

        def voxels():
            ctx.synchronize()
            nv = np.empty(1, np.int32)
            ctx.memcpy_d2h(nv, d_nv)
            assert 0 <= int(nv[0]) <= cap
            got = np.empty(5 * int(nv[0]), np.int16)
            if got.size:
                ctx.memcpy_d2h(got, d_vox)
            return got.reshape(-1, 5)

        ctx.process_frames_voxel_partials_device(dev.dd, dev.dc, 50, d_keys, d_parts, cap, d_np)
        ctx.synchronize()
        m = np.empty(1, np.int32)
        ctx.memcpy_d2h(m, d_np)
        assert want.shape[0] <= int(m[0]) <= cropped.shape[0]         # partials of the cropped cloud, not of the whole one
        ctx.voxel_grid_from_partials_device(d_keys, d_parts, int(m[0]), 50, d_vox, cap * 5, d_nv)
        assert_same(voxels(), want)
        ctx.memcpy_h2d(d_nv, np.zeros(1, np.int32))
        sink = ctx.voxel_sink_begin(cap, 50)
        ctx.process_frames_voxel_into_sink_device(dev.dd, dev.dc, sink)
        ctx.voxel_sink_finish(sink, d_vox, cap * 5, d_nv)
        assert_same(voxels(), want)


# ---------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_setter_argument_errors():
    cfgs, _, _ = frames(2, 64, 48)
    lib = L.load()
    lo, hi = (C.c_int16 * 3)(0, 0, 0), (C.c_int16 * 3)(5, -1, 5)
    with PcsContext(cfgs) as ctx:
        assert lib.pcs_set_crop_box_mm(ctx._h, lo, hi) == -1
        assert lib.pcs_set_crop_box_mm(ctx._h, lo, None) == -1
        assert lib.pcs_set_crop_box_mm(ctx._h, None, lo) == -1
        assert ctx.crop_box_mm() is None
        with pytest.raises(PcsError) as e:
            ctx.set_crop_box_mm((0, 0, 1), (0, 0, 0))
        assert e.value.status == -1
        assert lib.pcs_get_crop_box_mm(ctx._h, lo, hi) == 0
    with PcsContext(cfgs, flags=FLAG_SCALAR_ARITH) as ctx:
        with pytest.raises(PcsError) as e:
            ctx.set_crop_box_mm(*BOX_A)
        assert e.value.status == -4 and "PCS_FLAG_SCALAR_ARITH" in str(e.value)
        assert ctx.crop_box_mm() is None


@pytest.mark.gpu
def test_calls_that_refuse_while_a_box_is_set(oracle):
    cfgs, depth, color = frames(2, 64, 48)
    n = cfgs[0].n_points
    rng = np.random.default_rng(5)
    vtx = rng.normal(0, 1, (n, 3)).astype(np.float32)
    tex = rng.random((n, 2), dtype=np.float32)
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        dev = Dev(ctx, depth, color)
        dev.fill(0x1234)
        ctx.memcpy_h2d(dev.cnt, np.full(3, -7, np.int32))
        d_kept = ctx.device_malloc(4 * 16)
        d_v, d_t = ctx.device_malloc(vtx.nbytes), ctx.device_malloc(tex.nbytes)
        ctx.memcpy_h2d(d_v, vtx)
        ctx.memcpy_h2d(d_t, tex)

        def refused(call):
            with pytest.raises(PcsError) as e:
                call()
            assert e.value.status == -4 and "crop box" in str(e.value)

        refused(lambda: ctx.process_frames_device_counted(dev.dd, dev.dc, d_kept, dev.out, dev.shorts, dev.cnt))
        refused(lambda: ctx.copy_pointcloud_xyzrgb_to_buffer_device(0, d_v, d_t, n, dev.dc[0], dev.out, dev.cnt))
        refused(lambda: ctx.copy_pointclouds_xyzrgb_to_buffer_device([(0, n, d_v, d_t, dev.dc[0], dev.out)], dev.cnt))
        assert (dev.payload() == 0x1234).all()
        assert dev.counts() == [-7, -7, -7]
        host = np.full((n, 5), 0x1234, np.int16)
        refused(lambda: ctx.copy_pointcloud_xyzrgb_to_buffer(0, vtx, tex, color[0], host))
        buf = np.full(2 + 5 * n, 0x1234, np.int16)
        refused(lambda: ctx.send_xyzrgb_pointcloud(0, vtx, tex, color[0], buf))
        assert (host == 0x1234).all() and (buf == 0x1234).all()
        # cleared: they work again
        ctx.set_crop_box_mm(None, None)
        ctx.copy_pointcloud_xyzrgb_to_buffer(0, vtx, tex, color[0], host)


# ---------------------------------------------------------------------------------------------
# the ABI (no GPU): header, exported symbols and the Python mirror hold the three new names
# ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["pcs_set_crop_box_mm", "pcs_get_crop_box_mm", "pcs_crop_payloads_device"]


def test_new_symbols_in_header_library_and_mirror():
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pcs_hip.h")).read()
    L.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    mirrored = [s[0] for s in L.SYMBOLS]
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert re.search(r" T %s$" % name, exported, re.M), name
        assert name in mirrored
