"""Extrinsics refinement on the GPU (pcs_align_sums_device, pcs_align_sums, pcs_align_payloads_device): all eighteen int64 and all of
dist2 bit for bit against the brute-force restatement of DESIGN.md section 3 (tests/np_align.py) over the clouds of
tests/align_cases.py — the wave, workgroup and reduce-loop edges, empty inputs, ties, the radius edge, cell corners, the ends of the
int16 range, sums beyond 32 bits, random clouds — with 0xA5 guard bytes in front of and behind d_sums and d_dist2; at every 2-byte
phase of both payloads, twice for determinism, under two target orders, through the host form, in a workspace a larger call left
behind, with one timing interval per launch, and through every refusal. Then the loop on the synthetic scene, replayed iteration by
iteration from its trace: the sums exactly, the matrices within a few float ulps, convergence against the truth."""
import functools

import numpy as np
import pytest

import align_cases as K
import np_align as N
from np_restatement import transform_payload_np
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import (ALIGN_INDEX_LAUNCHES, ALIGN_ITERATION_LAUNCHES, ALIGN_STOP_CONVERGED, ALIGN_STOP_ITERATIONS,
                                            ALIGN_STOP_REFUSED, ALIGN_SUMS_LAUNCHES, FLAG_SCALAR_ARITH)

pytestmark = pytest.mark.gpu

GUARD = 64
N_MAX = K.TWO_PASSES + 64
CASES = {c[0]: c for c in K.cases()}
INVALID, UNSUPPORTED = -1, -4
# |F_k+1 - (float)(solve_np(S_k) T_k)| per entry: two double solvers on the same exact C differ far below a float ulp (6e-8 at 1),
# so the two roundings to float differ by at most an ulp or two where a double lands beside a rounding boundary
MATRIX_TOL = 2e-7


class Arena:
    """Device buffers shared by the tests of this module: a source and a target payload at any 2-byte phase, d_sums and d_dist2
    between guard bytes."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.src = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.tgt = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.sums = ctx.device_malloc(GUARD + 144 + GUARD)
        self.dist2 = ctx.device_malloc(GUARD + 4 * N_MAX + GUARD)
        assert all(p % 16 == 0 for p in (self.src, self.tgt, self.sums, self.dist2))

    def free(self):
        for p in (self.src, self.tgt, self.sums, self.dist2):
            self.ctx.device_free(p)

    def upload(self, source, target, s_phase=4, t_phase=4):
        if source.shape[0]:
            self.ctx.memcpy_h2d(self.src + s_phase, np.ascontiguousarray(source))
        if target.shape[0]:
            self.ctx.memcpy_h2d(self.tgt + t_phase, np.ascontiguousarray(target))
        return self.src + s_phase, self.tgt + t_phase

    def paint(self, n):
        self.ctx.memcpy_h2d(self.sums, np.full(GUARD + 144 + GUARD, 0xA5, np.uint8))
        self.ctx.memcpy_h2d(self.dist2, np.full(GUARD + 4 * n + GUARD, 0xA5, np.uint8))

    def read(self, n):
        """(sums bytes, dist2 bytes) with the guards checked."""
        a, b = np.empty(GUARD + 144 + GUARD, np.uint8), np.empty(GUARD + 4 * n + GUARD, np.uint8)
        self.ctx.memcpy_d2h(a, self.sums)
        self.ctx.memcpy_d2h(b, self.dist2)
        assert (a[:GUARD] == 0xA5).all() and (a[GUARD + 144:] == 0xA5).all(), "bytes around d_sums were written"
        assert (b[:GUARD] == 0xA5).all() and (b[GUARD + 4 * n:] == 0xA5).all(), "bytes around d_dist2 were written"
        return a[GUARD:GUARD + 144].copy(), b[GUARD:GUARD + 4 * n].copy()

    def run(self, source, target, r, s_phase=4, t_phase=4, dist2=True):
        """-> (the eighteen sums as Python integers, dist2 uint32 [n] or None)."""
        n = source.shape[0]
        d_s, d_t = self.upload(source, target, s_phase, t_phase)
        self.paint(n)
        self.ctx.align_sums_device(d_s if n else 0, n, d_t if target.shape[0] else 0, target.shape[0], r, self.sums + GUARD,
                                   self.dist2 + GUARD if dist2 else 0)
        self.ctx.synchronize()
        a, b = self.read(n)
        if not dist2:
            assert (b == 0xA5).all(), "d_dist2 was not given and was written"
        return [int(v) for v in a.view(np.int64)], (b.view(np.uint32) if dist2 else None)


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


@functools.lru_cache(maxsize=None)
def reference(name):
    _, source, target, r, expected = CASES[name]
    sums, dist2 = N.sums_np(source, target, r)
    if expected is not None:
        want, want_d2 = K.expected_sums(source, expected)
        assert sums == want and (dist2 == want_d2).all()
    return sums, dist2


@pytest.mark.parametrize("name", list(CASES))
def test_device_form_matches_the_restatement(arena, name):
    _, source, target, r, _ = CASES[name]
    want, want_d2 = reference(name)
    for s_phase, t_phase in ((4, 4), (0, 0)):               # buffer + 2 shorts; 16-byte aligned
        got, d2 = arena.run(source, target, r, s_phase, t_phase)
        assert got == want, (name, got, want)
        assert (d2 == want_d2).all(), name
    got, _ = arena.run(source, target, r, dist2=False)
    assert got == want


def test_the_cases_cover_what_they_are_for():
    assert reference("size6161")[0][1] > 1000 and reference("size6161")[0][1] < 6161          # matched and unmatched records
    assert K.TWO_PASSES > 256 * K.REDUCE_WIDTH                                              # more partials than the reduce is wide
    assert reference("reduce_two_passes")[0][1] > 256 * K.REDUCE_WIDTH // 2
    for name in ("source0", "target0", "both0"):
        n = CASES[name][1].shape[0]
        assert reference(name)[0] == [n] + [0] * 17 and (reference(name)[1] == 0xFFFFFFFF).all()
    assert max(abs(v) for v in reference("width")[0]) > 2 ** 41
    for k in range(len(K.RANDOM)):
        name = [c for c in CASES if c.startswith(f"random{k}_")][0]
        s = reference(name)[0]
        assert 0 < s[1] <= s[0], name


def test_every_phase_of_both_payloads(arena):
    name = [c for c in CASES if c.startswith("random2_")][0]
    _, source, target, r, _ = CASES[name]
    want, want_d2 = reference(name)
    assert 0 < want[1] < want[0]
    for s_phase in range(0, 16, 2):
        for t_phase in range(0, 16, 2):
            got, d2 = arena.run(source, target, r, s_phase, t_phase)
            assert got == want and (d2 == want_d2).all(), (s_phase, t_phase)


def test_two_runs_give_identical_bytes(arena):
    for name in [c for c in CASES if c.startswith("random")] + ["size6161"]:
        _, source, target, r, _ = CASES[name]
        a, da = arena.run(source, target, r)
        b, db = arena.run(source, target, r)
        assert a == b and da.tobytes() == db.tobytes(), name


def test_two_target_orders_give_identical_sums(arena):
    for name in ("size6161", "tie5_duplicates", [c for c in CASES if c.startswith("random0_")][0]):
        _, source, target, r, _ = CASES[name]
        order = np.random.default_rng(8).permutation(target.shape[0])
        a, da = arena.run(source, target, r)
        b, db = arena.run(source, np.ascontiguousarray(target[order]), r)
        assert a == b and (da == db).all(), name
        sorder = np.random.default_rng(9).permutation(source.shape[0])
        c, dc = arena.run(np.ascontiguousarray(source[sorder]), target, r)
        assert c == a and (dc == da[sorder]).all(), name


def test_host_form_agrees_with_the_device_form(arena):
    for name in ("size2049", "tie5", "source0", "target0", "both0", "width", "extremes_r1000"):
        _, source, target, r, _ = CASES[name]
        want, want_d2 = reference(name)
        sums, d2 = arena.ctx.align_sums(source, target, r, want_dist2=True)
        assert [int(v) for v in sums.as_array()] == want and (d2 == want_d2).all(), name
        assert arena.ctx.align_sums(source, target, r).as_array().tolist() == want


def test_small_call_after_a_large_one(arena):
    """The workspace a large call left behind is larger than the small call's carve: every piece still lies where its reader looks."""
    big = "reduce_two_passes"
    _, source, target, r, _ = CASES[big]
    assert arena.run(source, target, r)[0] == reference(big)[0]
    for name in ("size65", "tie5", "size6161"):
        _, source, target, r, _ = CASES[name]
        got, d2 = arena.run(source, target, r)
        assert got == reference(name)[0] and (d2 == reference(name)[1]).all(), name


def test_one_timing_interval_per_launch(arena):
    ctx = arena.ctx
    ctx.kernel_timing(True)
    try:
        ctx.kernel_times_ms()
        for name, launches in (("size257", ALIGN_SUMS_LAUNCHES), ("target0", 2), ("source0", 1)):
            _, source, target, r, _ = CASES[name]
            arena.run(source, target, r)
            ms = ctx.kernel_times_ms()
            assert ms.shape[0] == launches and (ms >= 0).all(), (name, ms)
        source, target, _ = K.scene()
        d_s, d_t = arena.upload(source, target)
        _, rep = ctx.align_payloads_device(d_s, source.shape[0], d_t, target.shape[0], max_dist_mm=K.SCENE_MAX_DIST, iterations=3)
        assert rep.iterations == 3
        assert ctx.kernel_times_ms().shape[0] == ALIGN_INDEX_LAUNCHES + 3 * ALIGN_ITERATION_LAUNCHES
    finally:
        ctx.kernel_timing(False)


def test_contexts_with_a_crop_box_or_scalar_arithmetic_are_no_reason_to_refuse():
    name = "size257"
    _, source, target, r, _ = CASES[name]
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    for flags, box in ((0, True), (FLAG_SCALAR_ARITH, False)):
        with PcsContext(cfgs, flags=flags) as c:
            if box:
                c.set_crop_box_mm((-10, -10, -10), (10, 10, 10))
            assert c.align_sums(source, target, r).as_array().tolist() == reference(name)[0]
            m, rep = c.align_payloads(source, target, max_dist_mm=r, iterations=2)
            assert rep.iterations == 2 and rep.status == 0 and np.isfinite(m).all()


def test_every_refusal_leaves_the_outputs_untouched(arena):
    ctx = arena.ctx
    _, source, target, r, _ = CASES["size257"]
    n, m = source.shape[0], target.shape[0]
    d_s, d_t = arena.upload(source, target)
    d_sums, d_d2 = arena.sums + GUARD, arena.dist2 + GUARD
    too_many = (2 ** 31 - 1) // 10 + 1
    bad = [
        ((d_s, n, d_t, m, 0, d_sums, d_d2), "max_dist_mm"),
        ((d_s, n, d_t, m, 1001, d_sums, d_d2), "max_dist_mm"),
        ((d_s, -1, d_t, m, r, d_sums, d_d2), "n_source"),
        ((d_s, n, d_t, -1, r, d_sums, d_d2), "n_target"),
        ((d_s, too_many, d_t, m, r, d_sums, d_d2), "n_source"),
        ((d_s, n, d_t, too_many, r, d_sums, d_d2), "n_target"),
        ((0, n, d_t, m, r, d_sums, d_d2), "d_source is NULL"),
        ((d_s, n, 0, m, r, d_sums, d_d2), "d_target is NULL"),
        ((d_s, n, d_t, m, r, 0, d_d2), "d_sums is NULL"),
        ((d_s + 1, n, d_t, m, r, d_sums, d_d2), "d_source is not 2-byte aligned"),
        ((d_s, n, d_t + 1, m, r, d_sums, d_d2), "d_target is not 2-byte aligned"),
        ((d_s, n, d_t, m, r, d_sums + 4, d_d2), "d_sums is not 8-byte aligned"),
        ((d_s, n, d_t, m, r, d_sums, d_d2 + 2), "d_dist2 is not 4-byte aligned"),
        ((d_s, n, d_t, m, r, d_s + 4, d_d2), "d_sums overlaps"),
        ((d_s, n, d_t, m, r, d_t + 10 * m // 8 * 8 - 4, d_d2), "d_sums overlaps"),
        ((d_s, n, d_t, m, r, d_sums, d_t + 12), "d_dist2 overlaps"),
        ((d_s, n, d_t, m, r, d_sums, d_s + 10 * n - 2), "d_dist2 overlaps"),
        ((d_s, n, d_t, m, r, d_sums, d_sums + 140), "d_dist2 overlaps d_sums"),
    ]
    before_s, before_t = np.empty(10 * n, np.uint8), np.empty(10 * m, np.uint8)
    ctx.memcpy_d2h(before_s, d_s)
    ctx.memcpy_d2h(before_t, d_t)
    for args, text in bad:
        arena.paint(n)
        with pytest.raises(PcsError) as e:
            ctx.align_sums_device(*args)
        assert e.value.status == INVALID and text in str(e.value), (text, str(e.value))
        ctx.synchronize()
        a, b = arena.read(n)
        assert (a == 0xA5).all() and (b == 0xA5).all(), text
    after_s, after_t = np.empty(10 * n, np.uint8), np.empty(10 * m, np.uint8)
    ctx.memcpy_d2h(after_s, d_s)
    ctx.memcpy_d2h(after_t, d_t)
    assert (after_s == before_s).all() and (after_t == before_t).all()
    # the loop's own
    ok = dict(max_dist_mm=r, iterations=3)
    for kw, text in ((dict(ok, max_dist_mm=0), "max_dist_mm"), (dict(ok, iterations=0), "iterations"), (dict(ok, iterations=101), "iterations"),
                     (dict(ok, source_stride=0), "source_stride"), (dict(ok, eps_rot_rad=-1.0), "eps_rot_rad"),
                     (dict(ok, eps_trans_mm=float("nan")), "eps_trans_mm"),
                     (dict(ok, init=np.full((4, 4), np.inf, np.float32)), "init[0] is not finite"),
                     (dict(ok, init=np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, np.nan, 0, 0, 0, 1], np.float32)), "init[11] is not finite")):
        with pytest.raises(PcsError) as e:
            ctx.align_payloads_device(d_s, n, d_t, m, **kw)
        assert e.value.status == INVALID and text in str(e.value), (text, str(e.value))
    with pytest.raises(PcsError) as e:
        ctx.align_payloads_device(d_s + 1, n, d_t, m, **ok)
    assert e.value.status == INVALID and "d_source is not 2-byte aligned" in str(e.value)


# ---- the loop ----------------------------------------------------------------------------------------------
def replay(arena, source, target, stride, out, rep, init=None):
    """Every recorded iteration of a loop call against the restatement; returns T_K rebuilt in double from the traced sums."""
    T = np.eye(4) if init is None else np.asarray(init, np.float32).astype(np.float64)
    assert len(rep.trace_sums) == rep.trace_transforms.shape[0] == rep.iterations
    for k in range(rep.iterations):
        F = rep.trace_transforms[k]
        assert np.abs(F.astype(np.float64) - T).max() <= MATRIX_TOL, (k, np.abs(F.astype(np.float64) - T).max())
        moved = transform_payload_np(source, F.reshape(-1), stride)
        assert moved.shape[0] == source.shape[0] // stride
        want, _ = N.sums_np(moved, target, K.SCENE_MAX_DIST)
        S_k = [int(v) for v in rep.trace_sums[k].as_array()]
        assert S_k == want, (k, S_k, want)
        alone, _ = arena.run(moved, target, K.SCENE_MAX_DIST)
        assert alone == S_k, k
        solved = N.solve_np(S_k)
        if solved is None:
            assert k == rep.iterations - 1 and rep.stop_reason == ALIGN_STOP_REFUSED
            break
        T = solved[0] @ T
    assert np.abs(out.astype(np.float64) - T).max() <= MATRIX_TOL
    first, last = rep.trace_sums[0], rep.trace_sums[-1]
    assert (rep.first_matched, rep.first_considered) == (first.matched, first.considered)
    assert (rep.last_matched, rep.last_considered) == (last.matched, last.considered)
    assert abs(rep.first_rms_mm - (first.sd2 / first.matched) ** 0.5) <= 1e-9 and abs(rep.last_rms_mm - (last.sd2 / last.matched) ** 0.5) <= 1e-9
    return T


def test_the_loop_on_the_synthetic_scene(arena):
    source, target, truth = K.scene()
    d_s, d_t = arena.upload(source, target)
    out, rep = arena.ctx.align_payloads_device(d_s, source.shape[0], d_t, target.shape[0], max_dist_mm=K.SCENE_MAX_DIST,
                                               iterations=K.SCENE_ITERATIONS, trace=K.SCENE_ITERATIONS)
    assert rep.status == 0 and rep.stop_reason == ALIGN_STOP_ITERATIONS and rep.iterations == K.SCENE_ITERATIONS
    replay(arena, source, target, 1, out, rep)
    rot0, trans0 = K.pose_error(np.eye(4), truth)
    rot, trans = K.pose_error(out, truth)
    print(f"scene on the GPU: {rot0:.3f} deg / {trans0:.2f} mm -> {rot:.3f} deg / {trans:.2f} mm, rms {rep.first_rms_mm:.2f} -> {rep.last_rms_mm:.2f}")
    assert rot <= rot0 / 4 and trans <= trans0 / 4
    # the host-array convenience is the same call
    out2, rep2 = arena.ctx.align_payloads(source, target, max_dist_mm=K.SCENE_MAX_DIST, iterations=K.SCENE_ITERATIONS)
    assert out2.tobytes() == out.tobytes() and rep2.iterations == rep.iterations and rep2.trace_transforms.shape[0] == 0


def test_the_loop_with_stride_4_and_an_initial_matrix(arena):
    source, target, truth = K.scene()
    init = K.rigid(0.3, (1, 0, 0), (2, 0, -1)).astype(np.float32)
    d_s, d_t = arena.upload(source, target)
    out, rep = arena.ctx.align_payloads_device(d_s, source.shape[0], d_t, target.shape[0], max_dist_mm=K.SCENE_MAX_DIST, iterations=12,
                                               source_stride=4, init=init, trace=12)
    assert rep.status == 0 and rep.iterations == 12 and rep.first_considered == source.shape[0] // 4
    assert (rep.trace_transforms[0] == init).all()
    replay(arena, source, target, 4, out, rep, init)
    # a trace shorter than the run simply stops recording (the replay's stand-alone calls used the arena's source buffer: upload again)
    d_s, d_t = arena.upload(source, target)
    out2, rep2 = arena.ctx.align_payloads_device(d_s, source.shape[0], d_t, target.shape[0], max_dist_mm=K.SCENE_MAX_DIST, iterations=12,
                                                 source_stride=4, init=init, trace=5)
    assert out2.tobytes() == out.tobytes() and rep2.iterations == 12 and len(rep2.trace_sums) == 5
    assert (rep2.trace_transforms == rep.trace_transforms[:5]).all()
    assert [s.as_array().tolist() for s in rep2.trace_sums] == [s.as_array().tolist() for s in rep.trace_sums[:5]]


def test_early_stop_agrees_with_the_trace(arena):
    source, target, _ = K.scene()
    eps_rot, eps_trans = 2e-3, 1.0
    d_s, d_t = arena.upload(source, target)
    out, rep = arena.ctx.align_payloads_device(d_s, source.shape[0], d_t, target.shape[0], max_dist_mm=K.SCENE_MAX_DIST,
                                               iterations=K.SCENE_ITERATIONS, eps_rot_rad=eps_rot, eps_trans_mm=eps_trans,
                                               trace=K.SCENE_ITERATIONS)
    assert rep.status == 0 and rep.stop_reason == ALIGN_STOP_CONVERGED and 1 < rep.iterations < K.SCENE_ITERATIONS
    small = [N.rotation_angle(d) <= eps_rot and N.translation_mm(d) <= eps_trans
             for d in (N.solve_np(s.as_array())[0] for s in rep.trace_sums)]
    assert small == [False] * (rep.iterations - 1) + [True]
    replay(arena, source, target, 1, out, rep)


def test_a_source_with_no_overlap_is_refused_with_out_equal_to_init(arena):
    source, target, _ = K.scene()
    away = K.far_away(source)
    init = K.rigid(1.0, (0, 1, 0), (3, 4, 5)).astype(np.float32)
    d_s, d_t = arena.upload(away, target)
    out, rep = arena.ctx.align_payloads_device(d_s, away.shape[0], d_t, target.shape[0], max_dist_mm=K.SCENE_MAX_DIST, iterations=5,
                                               init=init, trace=5)
    assert rep.status == UNSUPPORTED and rep.stop_reason == ALIGN_STOP_REFUSED and rep.iterations == 1
    assert "matched 0 < 3" in rep.detail
    assert out.tobytes() == init.tobytes()
    assert rep.trace_sums[0].as_array().tolist() == [away.shape[0]] + [0] * 17 and rep.first_rms_mm == 0.0
    # an empty source and an empty target end the same way
    for ns, nt in ((0, target.shape[0]), (away.shape[0], 0), (3, target.shape[0])):
        out, rep = arena.ctx.align_payloads_device(d_s if ns else 0, ns, d_t if nt else 0, nt, max_dist_mm=K.SCENE_MAX_DIST, iterations=5,
                                                   source_stride=4 if ns == 3 else 1, init=init)
        assert rep.status == UNSUPPORTED and rep.iterations == 1 and out.tobytes() == init.tobytes()
