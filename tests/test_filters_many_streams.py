"""The three depth stages of csrc/pcs_kernels_filter.hip (decimation, spatial filter, temporal / hole-fill pre-filter) on 17 and on 64
streams per launch, every stream of its own size (tests/many_stream_shapes.py), and pcs_crop_payloads_device on 17 and 64 cameras.
Every comparison is np.array_equal against the numpy restatements (np_decimation, np_spatial_filter, np_depth_filter): there are no
tolerances. Every device raster sits in one slab filled with a sentinel, with at least 128 uint16 of it on both sides of the raster;
after a call every uint16 of the slab that is not inside an output raster must still be the sentinel."""
import numpy as np
import pytest

import many_stream_shapes as M
import np_decimation as D
import np_depth_filter as F
import np_spatial_filter as SP
import test_crop_box as CB
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, FLAG_SCALAR_ARITH

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
SENTINEL = 0xABCD
PAD = 128                                   # uint16 on each side of every raster (256 bytes: the raster keeps its alignment)
PARAMS = SP.PARAMS


class Slab:
    """Rasters of `shapes` (h, w) in one device allocation: raster s starts `skew` bytes behind a 256-byte boundary, PAD uint16 of
    SENTINEL or more lie in front of it and behind it. The host keeps a mirror, so one copy each way moves everything and every
    uint16 outside the rasters is checked."""

    def __init__(self, ctx, shapes, skew=0):
        self.ctx, self.shapes = ctx, [tuple(s) for s in shapes]
        self.start, pos = [], 0
        for h, w in self.shapes:
            begin = (pos + PAD - 1) // PAD * PAD + PAD + skew // 2
            self.start.append(begin)
            pos = begin + h * w + PAD
        self.size = pos
        self.raw = ctx.device_malloc(2 * self.size + 512)
        self.base = (self.raw + 255) & ~255
        self.ptr = [self.base + 2 * b for b in self.start]
        assert all(p % 256 == skew for p in self.ptr)
        self.inside = np.zeros(self.size, bool)
        for b, (h, w) in zip(self.start, self.shapes):
            self.inside[b:b + h * w] = True
        self.fill()

    def fill(self, rasters=None):
        """The whole slab to SENTINEL, then `rasters` (if any) into their places."""
        host = np.full(self.size, SENTINEL, np.uint16)
        for b, shape, a in zip(self.start, self.shapes, rasters or []):
            assert a.shape == shape and a.dtype == np.uint16
            host[b:b + a.size] = a.reshape(-1)
        self.ctx.memcpy_h2d(self.base, host)
        self.sent = host

    def read(self):
        """The rasters as they are on the device now; nothing outside them may have changed."""
        self.ctx.synchronize()
        back = np.empty(self.size, np.uint16)
        self.ctx.memcpy_d2h(back, self.base)
        outside = ~self.inside
        assert (back[outside] == SENTINEL).all(), "the call wrote outside its rasters"
        return [back[b:b + h * w].reshape(h, w).copy() for b, (h, w) in zip(self.start, self.shapes)]

    def unchanged(self):
        back = np.empty(self.size, np.uint16)
        self.ctx.synchronize()
        self.ctx.memcpy_d2h(back, self.base)
        return np.array_equal(back, self.sent)

    def free(self):
        self.ctx.device_free(self.raw)


def same(got, want, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (what, "stream", s, w.shape, int((g != w).sum()), "pixels differ")


def shapes_of(name):
    return [(h, w) for w, h in M.TABLES[name]]


@pytest.fixture(scope="module")
def contexts():
    """ctx(name): one context per shape table (default flags), created when first asked for and shared by the module."""
    made = {}

    def ctx(name):
        if name not in made:
            made[name] = PcsContext(M.configs(M.TABLES[name]))
        return made[name]

    yield ctx
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def spatial_want():
    """want(name, params): the restated outputs of table `name`'s rasters, computed once."""
    cache, rasters = {}, {}

    def want(name, params):
        if name not in rasters:
            rasters[name] = M.spatial_rasters(name)
        if (name, params) not in cache:
            cache[(name, params)] = [SP.spatial_filter(r, **PARAMS[params])[0] for r in rasters[name]]
        return rasters[name], cache[(name, params)]

    return want


# ---------------------------------------------------------------------------------------------
# the limit itself
# ---------------------------------------------------------------------------------------------
def test_64_streams_are_accepted_and_65_refused(contexts):
    for name in ("NARROW", "WIDE"):
        ctx = contexts(name)
        assert ctx.n_streams == M.PCS_MAX_STREAMS
        assert [ctx.stream_points(s) for s in range(64)] == [w * h for w, h in M.TABLES[name]]
    with pytest.raises(PcsError) as e:
        PcsContext(M.configs(M.NARROW + [(8, 8)]))
    assert e.value.status == INVALID_ARG and "n_streams 65 outside 1..64" in str(e.value)


# ---------------------------------------------------------------------------------------------
# spatial filter
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew", [0, 2])
@pytest.mark.parametrize("name,params", [("NARROW", "radius2"), ("WIDE", "radius2"), ("MIXED17", "radius2"), ("WIDE", "five-iterations")])
def test_spatial_filter(contexts, spatial_want, name, params, skew):
    """skew 2: every raster two bytes off a 256-byte boundary, so every width takes the 2-byte row path; skew 0: the widths that are
    multiples of 8 take the 16-byte one. Out of place (the inputs unchanged afterwards), then in place."""
    ctx = contexts(name)
    rasters, want = spatial_want(name, params)
    d_in, d_out = Slab(ctx, shapes_of(name), skew), Slab(ctx, shapes_of(name), skew)
    try:
        d_in.fill(rasters)
        ctx.spatial_filter_depth_device(d_in.ptr, d_out.ptr, **PARAMS[params])
        same(d_out.read(), want, "out of place")
        assert d_in.unchanged()
        d_out.fill(rasters)
        ctx.spatial_filter_depth_device(d_out.ptr, d_out.ptr, **PARAMS[params])
        same(d_out.read(), want, "in place")
    finally:
        d_in.free()
        d_out.free()
    assert sum(not np.array_equal(w, r) for w, r in zip(want, rasters)) >= len(rasters) - 4          # the filter did something


# ---------------------------------------------------------------------------------------------
# decimation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(2, 9))
@pytest.mark.parametrize("name", ["NARROW", "WIDE", "MIXED17"])
def test_decimation(contexts, name, n):
    """The table's shapes are the decimated sizes, so one context serves every scale; the sources are s % n columns and (s // 2) % n
    rows larger than n times the output. Skew 0 and 2 bytes on sources and outputs."""
    ctx = contexts(name)
    sources = M.decimation_sources(name, n)
    want = [D.decimate(a, n) for a in sources]
    assert [w.shape for w in want] == shapes_of(name)
    for skew in (0, 2):
        d_src, d_out = Slab(ctx, M.source_shapes(name, n), skew), Slab(ctx, shapes_of(name), skew)
        try:
            d_src.fill(sources)
            ctx.decimate_depth_device(n, M.source_shapes(name, n), d_src.ptr, d_out.ptr)
            same(d_out.read(), want, f"scale {n}, skew {skew}")
            assert d_src.unchanged()
        finally:
            d_src.free()
            d_out.free()


# ---------------------------------------------------------------------------------------------
# temporal + hole fill
# ---------------------------------------------------------------------------------------------
FILTERS = {"temporal+fill": dict(temporal=True, alpha=0.4, delta=20, persistence=3, hole_fill=1),
           "temporal": dict(temporal=True, alpha=0.25, delta=33, persistence=5, hole_fill=0),
           "fill": dict(temporal=False, hole_fill=1)}


def restate_frames(frames, states, kw):
    """frames[k][s] through states[s], in order."""
    kw = dict(kw)
    kw["temporal_on"] = kw.pop("temporal")
    return [[F.filter_frame(a, st, **kw) for a, st in zip(per_stream, states)] for per_stream in frames]


@pytest.fixture(scope="module")
def temporal_frames():
    cache = {}

    def frames(name):
        if name not in cache:
            cache[name] = M.temporal_frames(name)
        return cache[name]

    return frames


@pytest.mark.parametrize("which", sorted(FILTERS))
@pytest.mark.parametrize("name", ["NARROW", "MIXED17"])
def test_temporal_and_hole_fill(contexts, temporal_frames, name, which):
    """Six frames, a reset after the third: frames 1..3 against one restated state, frames 4..6 against a fresh one. Once out of
    place and once in place (setting the filter again starts the state over)."""
    ctx, kw, frames, shapes = contexts(name), FILTERS[which], temporal_frames(name), shapes_of(name)
    want = restate_frames(frames[:3], [F.State(s) for s in shapes], kw) + restate_frames(frames[3:], [F.State(s) for s in shapes], kw)
    stateless = [restate_frames([f], [F.State(s) for s in shapes], kw)[0] for f in frames]
    differs = sum(not np.array_equal(a, b) for k in range(3, 6) for a, b in zip(want[k], stateless[k]))
    if kw["temporal"]:
        assert differs > len(shapes)                                  # the state mattered in frames 4..6
        carried = restate_frames(frames, [F.State(s) for s in shapes], kw)
        assert any(not np.array_equal(a, b) for a, b in zip(carried[3], want[3]))          # and so did the reset
    else:
        assert differs == 0                                           # hole fill alone has no state
    d_in, d_out = Slab(ctx, shapes), Slab(ctx, shapes)
    try:
        for in_place in (False, True):
            ctx.set_depth_filter(**kw)
            for k in range(6):
                if k == 3:
                    ctx.reset_depth_filter()
                if in_place:
                    d_out.fill(frames[k])
                    ctx.filter_depth_device(d_out.ptr, d_out.ptr)
                else:
                    d_in.fill(frames[k])
                    d_out.fill()
                    ctx.filter_depth_device(d_in.ptr, d_out.ptr)
                same(d_out.read(), want[k], f"frame {k + 1}, in place {in_place}")
                assert in_place or d_in.unchanged()
    finally:
        ctx.set_depth_filter(None)
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------
# tile counts across stitch launches
# ---------------------------------------------------------------------------------------------
def device_payload(ctx, d_depth, color, counted=0):
    n_max = ctx.max_payload_shorts
    d_color = []
    for c in color:
        p = ctx.device_malloc(c.nbytes)
        ctx.memcpy_h2d(p, c)
        d_color.append(p)
    d_pay, d_cnt = ctx.device_malloc(2 * n_max + 64), ctx.device_malloc(4 * (ctx.n_streams + 1))
    if counted:
        ctx.process_frames_device_counted(d_depth, d_color, counted, d_pay, n_max, d_cnt)
    else:
        ctx.process_frames_device(d_depth, d_color, d_pay, n_max, d_cnt)
    ctx.synchronize()
    cnt = np.empty(ctx.n_streams + 1, np.int32)
    ctx.memcpy_d2h(cnt, d_cnt)
    assert int(cnt[-1]) == int(cnt[:-1].sum())
    pay = np.empty(5 * int(cnt[-1]), np.int16)
    if pay.size:
        ctx.memcpy_d2h(pay, d_pay)
    for p in d_color + [d_pay, d_cnt]:
        ctx.device_free(p)
    return pay.reshape(-1, 5), [int(v) for v in cnt[:-1]]


def mixed17_color():
    return [S.synth_color(64, 48, s) for s in range(len(M.MIXED17))]


def test_tile_counts_across_stitch_launches(oracle, temporal_frames):
    """17 streams under PCS_FLAG_DROP_INVALID: the filter's per-tile counts are the restated rasters' for every stream (the last
    stream's tile_base is served by the second stitch launch), and the counted and the uncounted stitch both give the oracle's bytes."""
    cfgs, shapes, frames = M.configs(M.MIXED17), shapes_of("MIXED17"), temporal_frames("MIXED17")[:3]
    kw = FILTERS["temporal+fill"]
    want = restate_frames(frames, [F.State(s) for s in shapes], kw)
    color = mixed17_color()
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        ctx.set_depth_filter(**kw)
        n_tiles = ctx.stream_tile_base(ctx.n_streams)
        per_stream = [(w * h + F.TILE_POINTS - 1) // F.TILE_POINTS for w, h in M.MIXED17]
        assert [ctx.stream_tile_base(s) for s in range(18)] == [sum(per_stream[:s]) for s in range(18)] and n_tiles == sum(per_stream)
        d_kept = ctx.device_malloc(4 * (n_tiles + 2 * PAD))
        d_in, d_out = Slab(ctx, shapes), Slab(ctx, shapes)
        for k in range(3):
            ctx.memcpy_h2d(d_kept, np.full(n_tiles + 2 * PAD, 0xDEADBEEF, np.uint32))
            d_in.fill(frames[k])
            d_out.fill()
            ctx.filter_depth_device(d_in.ptr, d_out.ptr, d_kept + 4 * PAD)
            same(d_out.read(), want[k], f"frame {k + 1}")
            kept = np.empty(n_tiles + 2 * PAD, np.uint32)
            ctx.memcpy_d2h(kept, d_kept)
            assert (kept[:PAD] == 0xDEADBEEF).all() and (kept[PAD + n_tiles:] == 0xDEADBEEF).all()
            assert np.array_equal(kept[PAD:PAD + n_tiles], F.tile_counts(want[k])), k
        last = kept[PAD + ctx.stream_tile_base(16):PAD + n_tiles]
        assert last.size == 2 and 0 < last.sum() < 68 * 48               # the last stream keeps some pixels and drops some
        ref, n_ref = oracle.process_frames(cfgs, want[2], color, flags=FLAG_DROP_INVALID)
        counted, n_counted = device_payload(ctx, d_out.ptr, color, counted=d_kept + 4 * PAD)
        plain, n_plain = device_payload(ctx, d_out.ptr, color)
        assert n_counted == n_ref and n_plain == n_ref
        assert n_ref == [int((w != 0).sum()) for w in want[2]]
        CB.assert_same(counted, ref)
        CB.assert_same(plain, ref)
        ctx.device_free(d_kept)
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------------------------------------
# decimate 3 -> spatial -> temporal + holes -> stitch
# ---------------------------------------------------------------------------------------------
CHAIN_N, CHAIN_FRAMES = 3, 3


@pytest.fixture(scope="module")
def chain():
    """MIXED17's shapes as the decimated sizes, three frames, the three restatements chained in numpy; computed once."""
    shapes = shapes_of("MIXED17")
    sources = [M.decimation_sources("MIXED17", CHAIN_N, frame=k) for k in range(CHAIN_FRAMES)]
    decimated = [[D.decimate(a, CHAIN_N) for a in per_stream] for per_stream in sources]
    smoothed = [[SP.spatial_filter(a, **PARAMS["radius2"])[0] for a in per_stream] for per_stream in decimated]
    filtered = restate_frames(smoothed, [F.State(s) for s in shapes], FILTERS["temporal+fill"])
    return sources, decimated, smoothed, filtered


@pytest.mark.parametrize("scalar", [False, True])
def test_decimate_spatial_temporal_stitch_chain(oracle, chain, scalar):
    sources, decimated, smoothed, filtered = chain
    cfgs, shapes, color = M.configs(M.MIXED17), shapes_of("MIXED17"), mixed17_color()
    src_shapes = M.source_shapes("MIXED17", CHAIN_N)
    with PcsContext(cfgs, flags=FLAG_SCALAR_ARITH if scalar else 0) as ctx:
        ctx.set_depth_filter(**FILTERS["temporal+fill"])
        d_src, d_dec, d_out = Slab(ctx, src_shapes), Slab(ctx, shapes), Slab(ctx, shapes)
        for k in range(CHAIN_FRAMES):
            d_src.fill(sources[k])
            d_dec.fill()
            d_out.fill()
            ctx.decimate_depth_device(CHAIN_N, src_shapes, d_src.ptr, d_dec.ptr)
            ctx.spatial_filter_depth_device(d_dec.ptr, d_out.ptr, **PARAMS["radius2"])
            same(d_dec.read(), decimated[k], f"frame {k + 1}: decimation")
            same(d_out.read(), smoothed[k], f"frame {k + 1}: spatial filter")
            ctx.filter_depth_device(d_out.ptr, d_out.ptr)
            same(d_out.read(), filtered[k], f"frame {k + 1}: temporal filter")
        got, counts = device_payload(ctx, d_out.ptr, color)
        for slab in (d_src, d_dec, d_out):
            slab.free()
    if scalar:
        parts = []
        for sc, d, c in zip(cfgs, filtered[-1], color):
            v, t = oracle.deproject(sc, d, 0)
            parts.append(oracle.pack_scalar_variant(sc, v, t, c))
        want, want_counts = np.concatenate(parts), [p.shape[0] for p in parts]
    else:
        want, want_counts = oracle.process_frames(cfgs, filtered[-1], color)
    assert counts == want_counts == [w * h for w, h in M.MIXED17]
    CB.assert_same(got, want)
    changed = lambda a, b: sum(not np.array_equal(x, y) for x, y in zip(a, b))
    assert changed(smoothed[-1], decimated[-1]) >= 15                  # the spatial filter mattered
    assert changed(filtered[-1], smoothed[-1]) >= 15                   # and so did the temporal one


# ---------------------------------------------------------------------------------------------
# host forms: staging slabs carved for 17 and 64 streams
# ---------------------------------------------------------------------------------------------
HOST_N = 3
SMALL3 = [(68, 50), (64, 48), (161, 97)]


def host_forms_equal_device_forms(ctx, name):
    shapes, src_shapes = shapes_of(name), M.source_shapes(name, HOST_N)
    sources, rasters, frames = M.decimation_sources(name, HOST_N), M.spatial_rasters(name), M.temporal_frames(name, 2)
    d_src, d_in, d_out = Slab(ctx, src_shapes), Slab(ctx, shapes), Slab(ctx, shapes)
    try:
        d_src.fill(sources)
        ctx.decimate_depth_device(HOST_N, src_shapes, d_src.ptr, d_out.ptr)
        device = d_out.read()
        host = ctx.decimate_depth(HOST_N, sources)
        assert all(a.dtype == np.uint16 for a in host)
        same(host, device, "decimate_depth")
        assert sum(int(a.any()) for a in device) >= len(shapes) - 2

        d_in.fill(rasters)
        d_out.fill()
        ctx.spatial_filter_depth_device(d_in.ptr, d_out.ptr, **PARAMS["radius2"])
        device = d_out.read()
        same(ctx.spatial_filter_depth(rasters, **PARAMS["radius2"]), device, "spatial_filter_depth")
        assert sum(not np.array_equal(a, b) for a, b in zip(device, rasters)) >= len(shapes) - 4

        kw = FILTERS["temporal+fill"]
        ctx.set_depth_filter(**kw)
        device = []
        for f in frames:
            d_in.fill(f)
            d_out.fill()
            ctx.filter_depth_device(d_in.ptr, d_out.ptr)
            device.append(d_out.read())
        ctx.set_depth_filter(**kw)                                     # the state starts over
        for k, f in enumerate(frames):
            same(ctx.filter_depth(f), device[k], f"filter_depth, frame {k + 1}")
        assert sum(not np.array_equal(a, b) for a, b in zip(device[1], frames[1])) >= len(shapes) - 4
    finally:
        ctx.set_depth_filter(None)
        for slab in (d_src, d_in, d_out):
            slab.free()


def test_host_forms_on_17_streams(contexts):
    host_forms_equal_device_forms(contexts("MIXED17"), "MIXED17")


def test_host_forms_on_64_streams_after_a_3_stream_context(contexts):
    """A 3-stream context's host calls first, against the restatements; then the 64-stream context's, in the same process: nothing
    the library keeps per process is left at the first context's sizes."""
    rng = np.random.default_rng(3)
    with PcsContext(M.configs(SMALL3)) as small:
        sources = [SP.scene(HOST_N * w + 1, HOST_N * h + 2, 50 + s) for s, (w, h) in enumerate(SMALL3)]
        for a in sources:
            a[rng.random(a.shape) < 0.3] = 0
        rasters = [SP.scene(w, h, 60 + s) for s, (w, h) in enumerate(SMALL3)]
        same(small.decimate_depth(HOST_N, sources), [D.decimate(a, HOST_N) for a in sources], "3 streams: decimate_depth")
        same(small.spatial_filter_depth(rasters, **PARAMS["radius2"]), [SP.spatial_filter(a, **PARAMS["radius2"])[0] for a in rasters],
             "3 streams: spatial_filter_depth")
        small.set_depth_filter(**FILTERS["temporal+fill"])
        states = [F.State(a.shape) for a in rasters]
        for k in range(2):
            frame = [SP.scene(w, h, 60 + 10 * k + s) for s, (w, h) in enumerate(SMALL3)]
            same(small.filter_depth(frame), restate_frames([frame], states, FILTERS["temporal+fill"])[0], f"3 streams: filter_depth {k}")
        host_forms_equal_device_forms(contexts("NARROW"), "NARROW")


# ---------------------------------------------------------------------------------------------
# crop payloads with many cameras
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cams", [17, 64])
def test_crop_payloads_of_many_cameras(oracle, n_cams):
    """n_cams packed 64 x 48 payloads through pcs_crop_payloads_device (two and four launches of kLaunchStreams = 16 cameras) against the crop-box
    tests' reference: the oracle's uncropped cloud, masked per camera, every d-th kept row."""
    cfgs, depth, color = CB.frames(n_cams, 64, 48)
    full, fcounts = CB.uncropped(oracle, (n_cams, 64, 48), cfgs, depth, color, 0)
    assert fcounts == [64 * 48] * n_cams
    parts = [full[64 * 48 * i:64 * 48 * (i + 1)] for i in range(n_cams)]
    n = [p.shape[0] for p in parts]
    shorts = 5 * sum(n)
    with PcsContext(cfgs[:2]) as ctx:
        ctx.set_crop_box_mm(*CB.BOX_A)
        raw = [ctx.device_malloc(p.nbytes + 64) for p in parts]
        ins = [ptr + 4 for ptr in raw]
        for ptr, p in zip(ins, parts):
            ctx.memcpy_h2d(ptr, np.ascontiguousarray(p))
        out, cnt = ctx.device_malloc(2 * (shorts + 2 * PAD)), ctx.device_malloc(4 * (n_cams + 1))
        for ds in (1, 3):
            want, written, kept, total = CB.ref_frames(oracle, n_cams, 64, 48, 0, CB.BOX_A, ds)
            assert total == sum(n) and 0 < sum(written) < total and sum(1 for k in kept if k) > n_cams // 2
            ctx.memcpy_h2d(out, np.full(shorts + 2 * PAD, 0x5A5A, np.int16))
            ctx.crop_payloads_device(ins, n, ds, out + 2 * PAD, shorts, cnt)
            ctx.synchronize()
            c = np.empty(n_cams + 1, np.int32)
            ctx.memcpy_d2h(c, cnt)
            assert [int(x) for x in c[:-1]] == written and int(c[-1]) == sum(written)
            back = np.empty(shorts + 2 * PAD, np.int16)
            ctx.memcpy_d2h(back, out)
            CB.assert_same(back[PAD:PAD + 5 * sum(written)], want)
            assert (back[:PAD] == 0x5A5A).all() and (back[PAD + shorts:] == 0x5A5A).all()          # nothing outside the capacity
        for ptr in raw + [out, cnt]:
            ctx.device_free(ptr)
