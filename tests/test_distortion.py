"""Every kernel family that carries the two Brown-Conrady branches, on the GPU and bit for bit against the C
oracle, over the case table of tests/distortion_cases.py (whose conditions tests/test_distortion_cpu.py asserts without a GPU). Every
case runs under the arithmetic the certificate picks and under PCS_FLAG_FORCE_IEEE, and pcs_stream_math is asserted, so that no test
passes on the fall-back alone: a depth-distorted stream reports 0, a colour-only one a certified policy, and no distorted stream the
no-overflow or the row-constant form."""
import numpy as np
import pytest

import distortion_cases as DC
from test_gpu_parity import compaction_path          # noqa: F401  (the fixture that forces each compaction implementation)
from np_restatement import deproject_np, distortion_active
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import (FLAG_CUTOFF, FLAG_CUTOFF_COMPAT, FLAG_DROP_INVALID, FLAG_FORCE_IEEE, FLAG_SCALAR_ARITH,
                                            TRANSFORMS, make_intrinsics, make_stream_config)

pytestmark = pytest.mark.gpu
POLICIES = (0, FLAG_FORCE_IEEE)
CC = FLAG_CUTOFF | FLAG_CUTOFF_COMPAT
LENS_CASES = [c for c in DC.CASES if not c.identity]


def _is_identity(sc):
    return [float(x) for x in sc.depth_to_color.rotation] == [1, 0, 0, 0, 1, 0, 0, 0, 1]


def check_math(ctx, cfgs, flags, drawn=False):
    """pcs_stream_math / pcs_stream_color_row_const of every stream, as the lens of the stream demands. Returns the values.
    `drawn`: a random rig, which the certificate may refuse for its geometry alone."""
    got = [ctx.stream_math(s) for s in range(len(cfgs))]
    for s, sc in enumerate(cfgs):
        dd, cd = distortion_active(sc.depth), distortion_active(sc.color)
        if dd or cd:
            assert not ctx.stream_color_row_const(s), s
        if flags & FLAG_FORCE_IEEE or dd:
            assert got[s] == 0, (s, got)
        elif cd:                                  # certified, with the identity shortcut where R = I; never the no-overflow form
            assert got[s] in ((0, 1, 2) if drawn else (2 if _is_identity(sc) else 1,)), (s, got)
        else:
            assert drawn or got[s] > 0, (s, got)
    return got


def expected(oracle, cfgs, depth, color, flags=0, ds=1):
    return oracle.process_frames(cfgs, depth, color, flags & ~FLAG_FORCE_IEEE, ds)


# ---------------------------------------------------------------------------------------------------------------------
# pcs_deproject
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.CASES + [DC.CUT_WIDE, DC.CUT_NARROW], ids=lambda c: c.name)
def test_deproject_every_case(oracle, case):
    v0, t0 = DC.oracle_deproject(oracle, case)
    v1, t1 = deproject_np(case.sc, case.depth)
    for flags in POLICIES:
        with PcsContext([case.sc], flags=flags) as ctx:
            check_math(ctx, [case.sc], flags)
            v, t = ctx.deproject(0, case.depth)
        assert DC.same_bits(v, v0) and DC.same_bits(t, t0), flags
        assert DC.same_bits(v, v1) and DC.same_bits(t, t1), flags


# ---------------------------------------------------------------------------------------------------------------------
# dense: pcs_process_frames and pcs_process_frames_device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LENS_CASES + [c for c in DC.CASES if c.identity][:2], ids=lambda c: c.name)
def test_dense_one_stream(oracle, case):
    """One-stream contexts: depth only, colour model 1 and 2, both, under the identity and under a rotation pick <true,false>,
    <false,true> and <true,true> under IeeeMath and <false,true> under both CertMath forms; then the rest of the table."""
    want = DC.oracle_records(oracle, case)
    for flags in POLICIES:
        with PcsContext([case.sc], flags=flags) as ctx:
            check_math(ctx, [case.sc], flags)
            got, counts = DC.host_run(ctx, [case.depth], [case.color])
            assert counts == [case.sc.n_points]
            DC.assert_same(got, want, f"host, flags {flags}")
            dev = DC.Dev(ctx, [case.depth], [case.color])
            dev.run()
            got, counts = dev.result()
            assert counts == [case.sc.n_points]
            DC.assert_same(got, want, f"device, flags {flags}")
            dev.free()
    if not case.identity:
        assert DC.records_differ(want, DC.oracle_records(oracle, case, twin=True)).any()


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 0, 1)], ids=["in_order", "permuted"])
@pytest.mark.parametrize("ragged", [False, True], ids=["aligned", "ragged"])
def test_dense_mixed_frame_set(oracle, ragged, order):
    """[depth-only, colour model 2, no lens, both] with another raster per stream: the per-stream gates inside one <true,true> launch
    each decide for themselves, and the stream without a lens keeps the records it has on its own."""
    cfgs, depth, color = DC.mixed_frame_set(ragged, order)
    want, wcounts = expected(oracle, cfgs, depth, color)
    plain = order.index(2)
    alone, _ = expected(oracle, cfgs[plain:plain + 1], depth[plain:plain + 1], color[plain:plain + 1])
    at = sum(wcounts[:plain])
    for flags in POLICIES:
        with PcsContext(cfgs, flags=flags) as ctx:
            check_math(ctx, cfgs, flags)
            got, counts = DC.host_run(ctx, depth, color)
            assert counts == wcounts
            DC.assert_same(got, want, f"host, flags {flags}")
            DC.assert_same(got[at:at + wcounts[plain]], alone, "the stream without a lens")
            for depth_skew, skew in ((0, 0), (2, 4), (0, 10), (2, 0)):      # rasters 2 bytes off 16 (fast() false), payload off 16
                dev = DC.Dev(ctx, depth, color, depth_skew)
                dev.run(skew)
                got, counts = dev.result(skew)
                assert counts == wcounts
                DC.assert_same(got, want, f"device, flags {flags}, skews {depth_skew} {skew}")
                DC.assert_same(got[at:at + wcounts[plain]], alone, "the stream without a lens")
                dev.free()


def _small(stream, **kw):
    c = DC._case(f"small{stream}", shape=(64, 16), cshape=(64, 16), stream=stream, **kw)
    c.sc.cam_to_world[3] = float(stream)
    return c.sc, S.synth_depth(64, 48, stream)[:16].copy(), c.color


def test_dense_more_streams_than_one_launch(oracle):
    """Nineteen streams, sixteen per launch: the distorted ones are in the second launch."""
    streams = [_small(s) for s in range(16)] + [_small(16, dmodel=2, dk=DC.D_COEFFS), _small(17, cmodel=2, ck=DC.C_COEFFS, rot="ident"),
                                                _small(18, dmodel=2, dk=DC.D_STRONG, cmodel=1, ck=DC.C_STRONG)]
    cfgs, depth, color = [s[0] for s in streams], [s[1] for s in streams], [s[2] for s in streams]
    for flags, ds in ((0, 1), (FLAG_DROP_INVALID, 1), (CC, 1), (0, 3)):
        want, wcounts = expected(oracle, cfgs, depth, color, flags, ds)
        for policy in POLICIES:
            with PcsContext(cfgs, flags=flags | policy, downsample=ds) as ctx:
                check_math(ctx, cfgs, policy)
                got, counts = DC.host_run(ctx, depth, color)
            assert counts == wcounts
            DC.assert_same(got, want, f"flags {flags} policy {policy} stride {ds}")


# ---------------------------------------------------------------------------------------------------------------------
# ordered compaction and stride: count and emit must reach the same verdict where the lens moves x and the world coordinates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [FLAG_DROP_INVALID, FLAG_CUTOFF, CC, CC | FLAG_DROP_INVALID], ids=["drop", "cut", "cut_compat",
                                                                                                     "cut_compat_drop"])
@pytest.mark.parametrize("ds", [1, 3])
def test_compaction_and_stride(oracle, flags, ds, compaction_path):
    cfgs, depth, color = DC.cut_frame_set()
    want, wcounts = expected(oracle, cfgs, depth, color, flags, ds)
    assert all(0 < c < sc.n_points for c, sc in zip(wcounts, cfgs))
    for policy in POLICIES:
        with PcsContext(cfgs, flags=flags | policy, downsample=ds) as ctx:
            check_math(ctx, cfgs, policy)
            got, counts = DC.host_run(ctx, depth, color)
            assert counts == wcounts and sum(counts) == want.shape[0], (policy, counts, wcounts)
            DC.assert_same(got, want, f"host, policy {policy}")
            dev = DC.Dev(ctx, depth, color)
            dev.run(4)
            got, counts = dev.result(4)
            assert counts == wcounts
            DC.assert_same(got, want, f"device, policy {policy}")
            dev.free()


@pytest.mark.parametrize("ds", [2, 3])
def test_stride_alone(oracle, ds):
    cfgs, depth, color = DC.mixed_frame_set(ragged=True)
    want, wcounts = expected(oracle, cfgs, depth, color, 0, ds)
    for policy in POLICIES:
        with PcsContext(cfgs, flags=policy, downsample=ds) as ctx:
            check_math(ctx, cfgs, policy)
            got, counts = DC.host_run(ctx, depth, color)
        assert counts == wcounts == [-(-sc.n_points // ds) for sc in cfgs]
        DC.assert_same(got, want, f"policy {policy}")


@pytest.mark.parametrize("case", [DC.CUT_WIDE, DC.CUT_NARROW], ids=lambda c: c.name)
def test_cut_depends_on_the_lens_one_stream(oracle, case, compaction_path):
    """The wide lens, where |x| <= 2 cuts inside the 1.5 m range, and the narrow one, whose undistorted twin may be counted from the
    Z16 word: counts and bytes of the lens, which differ from the twin's."""
    for flags in (FLAG_CUTOFF, CC, FLAG_CUTOFF | FLAG_DROP_INVALID):
        want, wcounts = expected(oracle, [case.sc], [case.depth], [case.color], flags)
        twin, tcounts = expected(oracle, [case.twin], [case.depth], [case.color], flags)
        assert wcounts != tcounts
        for policy in POLICIES:
            with PcsContext([case.sc], flags=flags | policy) as ctx:
                check_math(ctx, [case.sc], policy)
                got, counts = DC.host_run(ctx, [case.depth], [case.color])
            assert counts == wcounts, (flags, policy, counts, wcounts, tcounts)
            DC.assert_same(got, want, f"flags {flags} policy {policy}")
            with PcsContext([case.twin], flags=flags | policy) as ctx:
                got, counts = DC.host_run(ctx, [case.depth], [case.color])
            assert counts == tcounts
            DC.assert_same(got, twin, f"twin, flags {flags} policy {policy}")


# ---------------------------------------------------------------------------------------------------------------------
# K frame-sets per call
# ---------------------------------------------------------------------------------------------------------------------
def _three_sets(depth, color):
    return [([np.ascontiguousarray(np.roll(d, 3 * k, axis=0)) for d in depth], [np.roll(c, 7 * k) for c in color]) for k in range(3)]


def _one_case_frame_set(name):
    c = DC.BY_NAME[name]
    return [c.sc], [c.depth], [c.color]


@pytest.mark.parametrize("flags", [0, FLAG_DROP_INVALID], ids=["dense", "drop"])
@pytest.mark.parametrize("which", ["mixed", "depth_only_roll", "colour2_ident", "colour1_rot"])
def test_batch_of_three_frame_sets(oracle, flags, which):
    """pcs_process_frames_device_batch: the mixed frame-set (<true,true>), and one-stream contexts that pick the batch twins of
    <true,false> under IeeeMath and of <false,true> under both CertMath forms and IeeeMath."""
    cfgs, depth, color = DC.mixed_frame_set() if which == "mixed" else _one_case_frame_set(which)
    sets = _three_sets(depth, color)
    wants = [expected(oracle, cfgs, d, c, flags) for d, c in sets]
    assert DC.first_diff(wants[0][0][:100], wants[1][0][:100])
    for policy in POLICIES:
        with PcsContext(cfgs, flags=flags | policy) as ctx:
            check_math(ctx, cfgs, policy)
            devs = [DC.Dev(ctx, d, c) for d, c in sets]
            ctx.process_frames_device_batch([d.dd for d in devs], [d.dc for d in devs], [d.out + 4 for d in devs],
                                            ctx.max_payload_shorts, [d.cnt for d in devs])
            for k, (dev, (want, wcounts)) in enumerate(zip(devs, wants)):
                got, counts = dev.result(4)
                assert counts == wcounts, (policy, k)
                DC.assert_same(got, want, f"policy {policy} set {k}")
            for dev in devs:
                dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# PCS_FLAG_SCALAR_ARITH: pack_scalar_variant over oracle.deproject, as tests/test_scalar_arith.py builds it
# ---------------------------------------------------------------------------------------------------------------------
def _a3_keep(V):
    with np.errstate(all="ignore"):
        return (V[:, 2] != 0) & (V[:, 0] != 0) & ~(V[:, 2] > np.float32(1.5))


def scalar_expected(oracle, cfgs, depth, color, cut=False, ds=1):
    parts, counts, skipped = [], [], 0
    for sc, d, c in zip(cfgs, depth, color):
        v, t = oracle.deproject(sc, d)
        rec = oracle.pack_scalar_variant(sc, v, t, c).copy()
        if cut:
            rec[~_a3_keep(v)] = 0
            skipped += int((~_a3_keep(v)).sum())
        rec = rec[::ds]
        parts.append(rec)
        counts.append(rec.shape[0])
    return np.concatenate(parts), counts, skipped


@pytest.mark.parametrize("cut,ds", [(False, 1), (True, 1), (False, 3)], ids=["dense", "cut", "stride3"])
def test_scalar_arithmetic(oracle, cut, ds):
    cfgs, depth, color = DC.cut_frame_set()
    want, wcounts, skipped = scalar_expected(oracle, cfgs, depth, color, cut, ds)
    assert not cut or 0 < skipped < want.shape[0]
    dense, _ = expected(oracle, cfgs, depth, color, 0, ds)
    assert cut or DC.records_differ(want, dense).any()                 # not the -m bytes
    for policy in POLICIES:
        with PcsContext(cfgs, flags=FLAG_SCALAR_ARITH | policy | (FLAG_CUTOFF if cut else 0), downsample=ds) as ctx:
            check_math(ctx, cfgs, policy)
            got, counts = DC.host_run(ctx, depth, color)
            assert counts == wcounts
            DC.assert_same(got, want, f"host, policy {policy}")
            dev = DC.Dev(ctx, depth, color)
            dev.run(4)
            got, counts = dev.result(4)
            assert counts == wcounts
            DC.assert_same(got, want, f"device, policy {policy}")
            dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# crop box: the uncropped oracle cloud, masked with numpy per stream, every d-th kept row (as tests/test_crop_box.py)
# ---------------------------------------------------------------------------------------------------------------------
def _mask(part, box):
    xyz = part[:, :3].astype(np.int32)
    return ((xyz >= np.array(box[0], np.int32)) & (xyz <= np.array(box[1], np.int32))).all(axis=1)


def crop_expected(oracle, cfgs, depth, color, flags, box, ds):
    full, counts = expected(oracle, cfgs, depth, color, flags)
    out, written, o = [], [], 0
    for c in counts:
        rows = full[o:o + c][_mask(full[o:o + c], box)][::ds]
        o += c
        out.append(rows)
        written.append(rows.shape[0])
    return np.concatenate(out).reshape(-1, 5), written, full.shape[0]


def _crop_frame_set():
    a, b = DC.BY_NAME["depth_only_roll"], DC.BY_NAME["both_rot"]
    return [a.sc, b.sc], [a.depth, b.depth], [a.color, b.color]


def _box_through(oracle, cfgs, depth, color):
    full, _ = expected(oracle, cfgs, depth, color, FLAG_DROP_INVALID)
    return ([int(np.percentile(full[:, a], 20)) for a in range(3)], [int(np.percentile(full[:, a], 80)) for a in range(3)])


@pytest.mark.parametrize("flags", [0, FLAG_DROP_INVALID], ids=["dense", "drop"])
@pytest.mark.parametrize("ds", [1, 3])
@pytest.mark.parametrize("form", ["host", "batch"])
def test_crop_box_cuts_through_the_distorted_cloud(oracle, flags, ds, form):
    cfgs, depth, color = _crop_frame_set()
    box = _box_through(oracle, cfgs, depth, color)
    want, wcounts, total = crop_expected(oracle, cfgs, depth, color, flags, box, ds)
    assert all(c > 16 for c in wcounts) and sum(wcounts) * ds < total
    untwinned = crop_expected(oracle, [DC.BY_NAME["depth_only_roll"].twin, DC.BY_NAME["both_rot"].twin], depth, color, flags, box, ds)
    assert untwinned[1] != wcounts                                     # the box's verdict depends on the lens
    sets = _three_sets(depth, color)[:2]
    wants = [crop_expected(oracle, cfgs, d, c, flags, box, ds) for d, c in sets]
    for policy in POLICIES:
        with PcsContext(cfgs, flags=flags | policy, downsample=ds) as ctx:
            check_math(ctx, cfgs, policy)
            ctx.set_crop_box_mm(*box)
            if form == "host":
                got, counts = DC.host_run(ctx, depth, color)
                assert counts == wcounts, (policy, counts, wcounts)
                DC.assert_same(got, want, f"host, policy {policy}")
                continue
            devs = [DC.Dev(ctx, d, c) for d, c in sets]
            ctx.process_frames_device_batch([d.dd for d in devs], [d.dc for d in devs], [d.out for d in devs],
                                            ctx.max_payload_shorts, [d.cnt for d in devs])
            for k, (dev, (w, wc, _)) in enumerate(zip(devs, wants)):
                got, counts = dev.result()
                assert counts == wc, (policy, k)
                DC.assert_same(got, w, f"batch, policy {policy} set {k}")
            for dev in devs:
                dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# voxel grid from rasters: the oracle's voxel grid of the oracle's stitched payload
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["bucket", "bucket-cold", "lsd"])
def voxel_tail(request, monkeypatch):
    """test_voxel_grid.py's fixture of the same name, restated: that one is autouse, and importing it would run every test of this
    module three times."""
    monkeypatch.setenv("PCS_VOXEL_TAIL", "bucket" if request.param.startswith("bucket") else request.param)
    monkeypatch.setenv("PCS_VOXEL_REGIONS", "0" if request.param == "bucket-cold" else "1")
    return request.param


def _fetch_voxels(ctx, d_vox, d_nv, cap):
    ctx.synchronize()
    nv = np.empty(1, np.int32)
    ctx.memcpy_d2h(nv, d_nv)
    assert 0 <= int(nv[0]) <= cap
    got = np.empty(5 * int(nv[0]), np.int16)
    if got.size:
        ctx.memcpy_d2h(got, d_vox)
    return got.reshape(-1, 5)


@pytest.mark.parametrize("ragged", [False, True], ids=["aligned", "ragged"])
@pytest.mark.parametrize("entry", ["one_call", "partials", "sink"])
def test_voxel_grid_from_distorted_rasters(oracle, ragged, entry, voxel_tail):
    """pcs_process_frames_voxel_device, the partials pair, and the sink over two contexts (the lens-free and the colour-only stream
    on one, the depth-distorted ones on the other)."""
    cfgs, depth, color = DC.mixed_frame_set(ragged, (2, 1, 0, 3))
    cap = sum(sc.n_points for sc in cfgs)
    stitched, _ = expected(oracle, cfgs, depth, color, FLAG_DROP_INVALID)
    for policy in POLICIES:
        flags = FLAG_DROP_INVALID | policy
        with PcsContext(cfgs, flags=flags) as ctx, PcsContext(cfgs[:2], flags=flags) as a, PcsContext(cfgs[2:], flags=flags) as b:
            check_math(ctx, cfgs, policy)
            dev = DC.Dev(ctx, depth, color)
            d_vox = ctx.device_malloc(cap * 10 + 64); d_nv = ctx.device_malloc(64)
            d_keys = ctx.device_malloc(cap * 8 + 64); d_parts = ctx.device_malloc(cap * 32 + 64); d_np = ctx.device_malloc(64)
            for leaf in (40, 200):
                want = oracle.voxel_grid(stitched, leaf)
                assert 1 < want.shape[0] < stitched.shape[0]
                if entry == "one_call":
                    ctx.process_frames_voxel_device(dev.dd, dev.dc, leaf, d_vox, cap * 5, d_nv)
                    DC.assert_same(_fetch_voxels(ctx, d_vox, d_nv, cap), want, f"one call, leaf {leaf} policy {policy}")
                    continue
                if entry == "partials":
                    ctx.process_frames_voxel_partials_device(dev.dd, dev.dc, leaf, d_keys, d_parts, cap, d_np)
                    ctx.voxel_grid_from_partials_device(d_keys, d_parts, cap, leaf, d_vox, cap * 5, d_nv, d_n_partials=d_np)
                    DC.assert_same(_fetch_voxels(ctx, d_vox, d_nv, cap), want, f"partials, leaf {leaf} policy {policy}")
                    continue
                # the sink: a's workspace, b's rasters poured into it; the host orders the three steps
                sink = a.voxel_sink_begin(cap, leaf)
                a.synchronize()
                a.process_frames_voxel_into_sink_device(dev.dd[:2], dev.dc[:2], sink)
                b.process_frames_voxel_into_sink_device(dev.dd[2:], dev.dc[2:], sink)
                a.synchronize(); b.synchronize()
                a.voxel_sink_finish(sink, d_vox, cap * 5, d_nv)
                DC.assert_same(_fetch_voxels(a, d_vox, d_nv, cap), want, f"sink, leaf {leaf} policy {policy}")
            for p in (d_vox, d_nv, d_keys, d_parts, d_np):
                ctx.device_free(p)
            dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# the software-pipelined host form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, FLAG_DROP_INVALID], ids=["dense", "drop"])
def test_submit_collect_two_tickets(oracle, flags):
    case = DC.BY_NAME["both_roll"]
    sets = _three_sets([case.depth], [case.color])[:2]
    for policy in POLICIES:
        with PcsContext([case.sc], flags=flags | policy) as ctx:
            check_math(ctx, [case.sc], policy)
            tickets = [ctx.submit_frames(d, c) for d, c in sets]
            for t, (d, c) in zip(tickets, sets):
                buf, counts, size = ctx.collect_frames(t)
                want, wcounts = expected(oracle, [case.sc], d, c, flags)
                assert counts == wcounts and size == want.nbytes
                DC.assert_same(buf[2:2 + want.size], want, f"policy {policy}")


# ---------------------------------------------------------------------------------------------------------------------
# the node library: two virtual peers of one GPU, the second one's camera with a depth lens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,ds", [(0, 1), (FLAG_DROP_INVALID, 1), (CC, 1), (0, 3)], ids=["dense", "drop", "cut_compat", "stride3"])
def test_node_stitch_with_a_depth_distorted_peer(oracle, flags, ds):
    _node_with_a_depth_distorted_peer(oracle, flags, ds, "stitch")


@pytest.mark.parametrize("flags", [0, FLAG_DROP_INVALID], ids=["dense", "drop"])
def test_node_voxel_routes_with_a_depth_distorted_peer(oracle, flags):
    _node_with_a_depth_distorted_peer(oracle, flags, 1, "voxel")


def _node_with_a_depth_distorted_peer(oracle, flags, ds, what):
    from pointcloud_stitching_amd.node import PcsNode, VOXEL_PARTIALS, VOXEL_PAYLOADS
    a, b = DC.BY_NAME["colour2_ident"], DC.BY_NAME["both_rot"]
    cfgs = [a.sc, b.sc]
    depth = [a.depth // 2, b.depth // 2]                               # part of the scene inside 1.5 m
    color = [a.color, b.color]
    want, wcounts = expected(oracle, cfgs, depth, color, flags, ds)
    for policy in POLICIES:
        for sc in cfgs:                                                # a node has no accessor: a peer's context is made like this one
            with PcsContext([sc], flags=flags | policy, downsample=ds) as ctx:
                check_math(ctx, [sc], policy)
        with PcsNode(cfgs, devices=[0, 0], flags=flags | policy, downsample=ds) as node:
            if what == "stitch":
                buf, counts, size = node.process(depth, color)
                assert counts == wcounts and size == want.nbytes, policy
                DC.assert_same(buf[2:2 + want.size], want, f"stitch, policy {policy}")
                continue
            for route in (VOXEL_PARTIALS, VOXEL_PAYLOADS):
                got, _ = node.process_voxel(depth, color, 40, route)
                DC.assert_same(got, oracle.voxel_grid(want, 40), f"voxel route {route}, policy {policy}")


# ---------------------------------------------------------------------------------------------------------------------
# a fuzz that draws lenses
# ---------------------------------------------------------------------------------------------------------------------
def _random_lens_config(rng, w, h, cw, ch):
    """test_gpu_parity._random_config (tame) with a depth model 2 in a third of the draws, colour model 1 or 2 in half, and
    coefficients from normal(0, 0.05)."""
    f = rng.uniform(0.5, 1.5) * w
    ddist = rng.random() < 1 / 3
    di = make_intrinsics(w, h, f, f * rng.uniform(0.98, 1.02), w / 2 + rng.uniform(-20, 20), h / 2 + rng.uniform(-20, 20),
                         model=2 if ddist else 0, coeffs=list(rng.normal(0, 0.05, 5)) if ddist else None)
    fc = rng.uniform(0.5, 1.5) * cw
    cmodel = int(rng.integers(1, 3)) if rng.random() < 0.5 else 0
    ci = make_intrinsics(cw, ch, fc, fc * rng.uniform(0.98, 1.02), cw / 2 + rng.uniform(-20, 20), ch / 2 + rng.uniform(-20, 20),
                         model=cmodel, coeffs=list(rng.normal(0, 0.05, 5)) if cmodel else None)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    ang = 0.0 if rng.random() < 0.3 else rng.normal(0, 0.02)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    t = rng.normal(0, 0.02, 3)
    if rng.random() < 0.3:
        t[rng.integers(0, 3)] = 0.0
    m = TRANSFORMS[rng.integers(0, 8)].copy()
    return make_stream_config(di, ci, cam_to_world=m, rotation=list(Rm.T.reshape(-1)), translation=list(t), depth_scale=0.001)


def test_fuzzed_lenses_both_policies(oracle):
    rng = np.random.default_rng(355)
    picked, drawn, colour_only, lens_free = [], set(), [], []
    for trial in range(40):
        w, h = 64, 16
        cw, ch = [(64, 16), (48, 40), (128, 8), (100, 75)][trial % 4]
        sc = _random_lens_config(rng, w, h, cw, ch)
        drawn.add((distortion_active(sc.depth), int(sc.color.model) if distortion_active(sc.color) else 0))
        depth = S.synth_depth(w, 48, trial)[:h].copy() if trial % 3 else S.synth_depth(w, h, trial, mode="random")
        color = S.synth_color(cw, ch, trial)
        flags = [0, FLAG_DROP_INVALID, FLAG_CUTOFF, CC | FLAG_DROP_INVALID][trial % 4]
        want, wcounts = expected(oracle, [sc], [depth], [color], flags)
        for policy in POLICIES:
            with PcsContext([sc], flags=flags | policy) as ctx:
                math = check_math(ctx, [sc], policy, drawn=True)[0]
                if policy == 0:
                    picked.append(math)
                    if not distortion_active(sc.depth):
                        (colour_only if distortion_active(sc.color) else lens_free).append(math)
                got, counts = DC.host_run(ctx, [depth], [color])
            assert counts == wcounts, (trial, policy)
            d = DC.first_diff(got, want)
            assert d is None, f"trial {trial} flags {flags} policy {policy} math {math}: {d}"
    assert any(p == 0 for p in picked) and any(p > 0 for p in picked)      # refused and certified configurations both occurred
    assert any(p in (1, 2) for p in colour_only), colour_only              # ... a colour-only lens among the certified ones
    assert any(p > 0 for p in lens_free), lens_free                        # ... and a rig without a lens
    assert {(True, 0), (True, 1), (True, 2), (False, 1), (False, 2), (False, 0)} <= drawn
