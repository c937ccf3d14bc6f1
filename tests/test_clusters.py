"""Euclidean cluster extraction on the GPU (pcs_cluster_filter_device and its siblings, pcs_cluster_labels_device), byte for byte and
word for word against the brute-force restatement of DESIGN.md section 3 (tests/np_clusters.py) over the clouds of
tests/cluster_cases.py: at the reference's `buffer + 2` shorts and at 16-byte alignment, at every 2-byte phase of input and output
for one cloud, with guard bytes in front of the output, behind the kept records and behind the worst-case output, twice for
determinism, with and without a statistics block, through the counted form, the host forms, the labels forms, between the other two
filters on one context, in front of the voxel grid, and through every refusal. Clouds of at most 4 096 records against the brute
force, one lattice of 65 536 against its own arithmetic, capacities up to 65 536. There is no tolerance anywhere.
Clouds of one to 2.7 million records, where the scans take a second chunk and the union-find is contended: tests/test_clusters_scale.py."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as K
import np_clusters as N
import np_radius_outlier as NR
import np_stat_outlier as NS
import radius_outlier_cases as RC
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import (CLUSTER_LABEL_LAUNCHES, CLUSTER_LAUNCHES, CLUSTER_STATS_FIELDS, FLAG_CUTOFF, FLAG_DROP_INVALID,
                                            FLAG_SCALAR_ARITH, POINT_SHORTS, ClusterParams, ClusterStatsC)

pytestmark = pytest.mark.gpu

GUARD = 64                      # bytes of 0xA5 in front of the output, behind the kept records and behind the worst-case output
N_MAX = 65536
CASES = {c[0]: c for c in K.cases()}
RANDOM = [c[0] for c in K.random_cases()]
SENTINEL = 0x5A5A5A5A
STATS_SENTINEL = 0x5A5A5A5A5A5A5A5A


class Arena:
    """Device buffers shared by the tests of this module: an input and an output payload at any 2-byte phase, count words, a
    statistics block, and two int32 arrays for labels and sizes."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.inp = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.out = ctx.device_malloc(GUARD + 64 + 10 * N_MAX + GUARD + 64)
        self.words = ctx.device_malloc(64)          # [0] the kept count, [4] the counted form's input count
        self.stats = ctx.device_malloc(64 + 64)     # the block, and eight guard words behind it
        self.labels = ctx.device_malloc(4 * 4200 + GUARD)
        self.sizes = ctx.device_malloc(4 * 4200 + GUARD)
        assert self.inp % 16 == 0 and self.out % 16 == 0 and self.stats % 8 == 0

    def free(self):
        for p in (self.inp, self.out, self.words, self.stats, self.labels, self.sizes):
            self.ctx.device_free(p)

    def run(self, rec, params, in_phase=4, out_phase=4, d_count=None, max_points=None, with_stats=True):
        """rec at phase in_phase (bytes mod 16) -> (kept records, kept count, stats dict or None) written at out_phase; everything
        around the kept records must stay 0xA5. d_count: run the counted form with that count on the device and max_points as its
        capacity."""
        ctx = self.ctx
        cap = rec.shape[0] if d_count is None else max_points
        d_in, d_out = self.inp + in_phase, self.out + GUARD + out_phase
        if rec.shape[0]:
            ctx.memcpy_h2d(d_in, np.ascontiguousarray(rec))
        span = GUARD + out_phase + 10 * cap + GUARD
        ctx.memcpy_h2d(self.out, np.full(span, 0xA5, np.uint8))
        ctx.memcpy_h2d(self.words, np.array([SENTINEL, 0 if d_count is None else d_count], np.int32))
        ctx.memcpy_h2d(self.stats, np.full(16, STATS_SENTINEL, np.int64))
        P = ClusterParams.make(*params)
        d_stats = self.stats if with_stats else 0
        if d_count is None:
            ctx.cluster_filter_device(d_in, cap, P, d_out, POINT_SHORTS * cap, self.words, d_stats)
        else:
            ctx.cluster_filter_device_counted(d_in, self.words + 4, cap, P, d_out, POINT_SHORTS * cap, self.words, d_stats)
        ctx.synchronize()
        got = np.empty(span, np.uint8)
        ctx.memcpy_d2h(got, self.out)
        words = np.empty(2, np.int32)
        ctx.memcpy_d2h(words, self.words)
        block = np.empty(16, np.int64)
        ctx.memcpy_d2h(block, self.stats)
        kept = int(words[0])
        assert 0 <= kept <= cap, kept
        lo = GUARD + out_phase
        assert (got[:lo] == 0xA5).all(), "bytes in front of d_out were written"
        assert (got[lo + 10 * kept:] == 0xA5).all(), "bytes behind the kept records were written"
        assert (block[8:] == STATS_SENTINEL).all(), "words behind the statistics block were written"
        if not with_stats:
            assert (block == STATS_SENTINEL).all()
        else:
            assert (block[5:8] == 0).all(), "the block's reserved words are zero"
        stats = dict(zip(CLUSTER_STATS_FIELDS, (int(v) for v in block[:5]))) if with_stats else None
        return got[lo:lo + 10 * kept].copy().view(np.int16).reshape(kept, 5), kept, stats

    def run_labels(self, rec, tol, with_sizes=True):
        """-> (labels, sizes or None, n_clusters); the words behind record n of both arrays must stay untouched."""
        ctx = self.ctx
        n = rec.shape[0]
        assert n <= 4200
        if n:
            ctx.memcpy_h2d(self.inp + 4, np.ascontiguousarray(rec))
        fill = np.full(n + GUARD // 4, SENTINEL, np.int32)
        ctx.memcpy_h2d(self.labels, fill)
        ctx.memcpy_h2d(self.sizes, fill)
        ctx.memcpy_h2d(self.words, np.array([SENTINEL, SENTINEL], np.int32))
        ctx.cluster_labels_device(self.inp + 4, n, tol, self.labels, self.sizes if with_sizes else 0, self.words)
        ctx.synchronize()
        lab, siz, words = np.empty_like(fill), np.empty_like(fill), np.empty(2, np.int32)
        ctx.memcpy_d2h(lab, self.labels)
        ctx.memcpy_d2h(siz, self.sizes)
        ctx.memcpy_d2h(words, self.words)
        assert (lab[n:] == SENTINEL).all() and (siz[n if with_sizes else 0:] == SENTINEL).all() and words[1] == SENTINEL
        return lab[:n].copy(), siz[:n].copy() if with_sizes else None, int(words[0])


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


def want_of(name):
    _, rec, params, _ = CASES[name]
    want, keep, stats, lab, sizes = K.reference(name)
    K.check_expected(name, keep, stats, lab)
    return rec, params, want, stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_form_matches_the_restatement(arena, name):
    rec, params, want, stats = want_of(name)
    for in_phase, out_phase in ((4, 4), (0, 0)):            # buffer + 2 shorts; 16-byte aligned
        got, kept, block = arena.run(rec, params, in_phase, out_phase)
        assert kept == want.shape[0], (name, kept, want.shape[0])
        assert (got == want).all(), name
        assert block == stats, (name, block, stats)


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_sizes_and_cluster_count_are_exact(arena, name):
    _, rec, params, _ = CASES[name]
    _, _, stats, lab, sizes = K.reference(name)
    got_lab, got_sizes, n_clusters = arena.run_labels(rec, params[0])
    assert (got_lab == lab).all() and (got_sizes == sizes).all() and n_clusters == stats["clusters"], name


def test_sizes_are_optional_in_the_labels_form(arena):
    for name in ("count2049", "chain_cut", "count1"):
        _, rec, params, _ = CASES[name]
        _, _, stats, lab, _ = K.reference(name)
        got_lab, none, n_clusters = arena.run_labels(rec, params[0], with_sizes=False)
        assert none is None and (got_lab == lab).all() and n_clusters == stats["clusters"], name


def test_every_phase_of_input_and_output(arena):
    rec, params, want, stats = want_of("count2049")
    assert 0 < want.shape[0] < rec.shape[0]
    for in_phase in range(0, 16, 2):
        for out_phase in range(0, 16, 2):
            got, kept, block = arena.run(rec, params, in_phase, out_phase)
            assert kept == want.shape[0] and (got == want).all() and block == stats, (in_phase, out_phase)


@pytest.mark.parametrize("name", RANDOM + ["chain", "lattice_joined", "duplicates"])
def test_two_runs_give_identical_bytes(arena, name):
    _, rec, params, _ = CASES[name]
    a, na, sa = arena.run(rec, params)
    b, nb, sb = arena.run(rec, params)
    assert na == nb and a.tobytes() == b.tobytes() and sa == sb
    la, za, ca = arena.run_labels(rec, params[0])
    lb, zb, cb = arena.run_labels(rec, params[0])
    assert la.tobytes() == lb.tobytes() and za.tobytes() == zb.tobytes() and ca == cb


def test_stats_are_optional(arena):
    for name in ("count2049", "pair_t5_in", "sizes_33_64"):
        rec, params, want, _ = want_of(name)
        got, kept, block = arena.run(rec, params, with_stats=False)
        assert block is None and kept == want.shape[0] and (got == want).all(), name


def test_counted_form_reads_its_count_on_the_device(arena):
    name = "count2049"
    _, rec, params, _ = CASES[name]
    n = rec.shape[0]
    for d_count, cap in ((257, n), (n, n), (0, n), (n + 1000, n), (-5, n), (2**31 - 1, 2048)):
        used = max(0, min(d_count, cap))
        want, _, stats = N.cluster_filter(rec[:used], *params) if used != n else K.reference(name)[:3]
        got, kept, block = arena.run(rec[:cap], params, d_count=d_count, max_points=cap)
        assert kept == want.shape[0] and (got == want).all() and block == stats, (d_count, cap)
        got, kept, block = arena.run(rec[:cap], params, d_count=d_count, max_points=cap, with_stats=False)
        assert kept == want.shape[0] and (got == want).all(), (d_count, cap)


def test_counted_form_with_a_capacity_far_above_the_count(arena):
    """Capacity 65 536, 1000 records: the grids cover the capacity, nothing at or beyond the count is read as a record — what
    lies there is a lattice that would be one more cluster, kept whole."""
    _, rec, params, _ = CASES["count2047"]
    n = 1000
    want, _, stats = N.cluster_filter(rec[:n], *params)
    assert 0 < want.shape[0] < n
    i = np.arange(N_MAX - n)
    big = np.concatenate([rec[:n], RC.with_colour(np.stack([9 * (i % 64) + 5000, 9 * ((i // 64) % 64) + 5000, 9 * (i // 4096) + 5000], axis=1))])
    got, kept, block = arena.run(big, params, d_count=n, max_points=N_MAX)
    assert kept == want.shape[0] and (got == want).all() and block == stats


def test_host_forms_agree_with_the_device_forms(arena):
    for name in ("count2049", "sizes_33_64", "count0", "count1", "chain_cut", "extremes_t1000"):
        rec, params, want, stats = want_of(name)
        _, _, _, lab, sizes = K.reference(name)
        got, block = arena.ctx.cluster_filter(rec, *params)
        dev, _, dev_block = arena.run(rec, params)
        assert got.shape == want.shape and (got == want).all() and (got == dev).all(), name
        assert block == stats and dev_block == stats, name
        got_lab, got_sizes, n_clusters = arena.ctx.cluster_labels(rec, params[0])
        assert (got_lab == lab).all() and (got_sizes == sizes).all() and n_clusters == stats["clusters"], name
    # stats NULL, sizes NULL in the host forms
    rec, params, want, stats = want_of("count2049")
    out = np.zeros((rec.shape[0], 5), np.int16)
    cnt = C.c_int(-1)
    P = ClusterParams.make(*params)
    p = np.ascontiguousarray(rec)
    lib, h = arena.ctx._lib, arena.ctx._h
    assert lib.pcs_cluster_filter(h, p.ctypes.data, rec.shape[0], C.byref(P), out.ctypes.data, out.size, C.byref(cnt), None) == 0
    assert cnt.value == want.shape[0] and (out[:cnt.value] == want).all()
    lab = np.full(rec.shape[0] + 4, SENTINEL, np.int32)
    assert lib.pcs_cluster_labels(h, p.ctypes.data, rec.shape[0], params[0], lab.ctypes.data, None, C.byref(cnt)) == 0
    assert cnt.value == stats["clusters"] and (lab[:-4] == K.reference("count2049")[3]).all() and (lab[-4:] == SENTINEL).all()


def test_works_on_any_context(arena):
    """No context predicate is read: a PCS_FLAG_SCALAR_ARITH context, and one with flags, downsample and a crop box, give the same
    bytes."""
    rec, params, want, stats = want_of("count2048")
    _, _, _, lab, sizes = K.reference("count2048")
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    for kwargs, box in (({"flags": FLAG_SCALAR_ARITH}, False), ({"flags": FLAG_CUTOFF | FLAG_DROP_INVALID, "downsample": 3}, True)):
        with PcsContext(cfgs, **kwargs) as c:
            if box:
                c.set_crop_box_mm((-10, -10, -10), (10, 10, 10))
            got, block = c.cluster_filter(rec, *params)
            got_lab, got_sizes, n_clusters = c.cluster_labels(rec, params[0])
        assert got.shape == want.shape and (got == want).all() and block == stats
        assert (got_lab == lab).all() and (got_sizes == sizes).all() and n_clusters == stats["clusters"]


def test_workspace_is_shared_with_the_other_filters(arena):
    """A radius-outlier call, a cluster call and a statistical-outlier call on one context, one slab: each against its own
    restatement, in both orders."""
    ctx = arena.ctx
    rec, params, want, stats = want_of("count2049")
    cube = RC.cube(400, 1)[:2049]
    for _ in range(2):
        assert (ctx.radius_outlier(cube, 20, 3) == NR.radius_outlier(cube, 20, 3)).all()
        got, block = ctx.cluster_filter(rec, *params)
        assert got.shape == want.shape and (got == want).all() and block == stats
        s_want, _, s_stats = NS.stat_outlier(cube, 3, 1000, 100)
        s_got, s_block = ctx.stat_outlier(cube, 3, 1000, 100)
        assert s_got.shape == s_want.shape and (s_got == s_want).all() and s_block == s_stats
        got, block = ctx.cluster_filter(rec, *params)
        assert got.shape == want.shape and (got == want).all() and block == stats


def test_small_call_in_a_workspace_a_large_call_left_behind(arena):
    """65 536 records on a lattice of pitch 3 (one cluster at tolerance 3, every word of the large carve written), then small clouds."""
    i = np.arange(N_MAX)
    big = RC.with_colour(np.stack([3 * (i % 64) - 96, 3 * ((i // 64) % 32) + 32000, 3 * (i // 2048) - 32768], axis=1))
    got, kept, block = arena.run(big, (3, N_MAX, N_MAX))
    assert kept == N_MAX and (got == big).all() and block == {"considered": N_MAX, "clusters": 1, "kept_clusters": 1, "largest": N_MAX,
                                                               "kept": N_MAX}
    got, kept, block = arena.run(big, (2, 1, 1))
    assert kept == N_MAX and block["clusters"] == N_MAX and block["largest"] == 1
    for name in ("pair_t5_in", "count65", "chain_cut"):
        rec, params, want, stats = want_of(name)
        got, kept, block = arena.run(rec, params)
        assert kept == want.shape[0] and (got == want).all() and block == stats, name
        lab, sizes, n_clusters = arena.run_labels(rec, params[0])
        assert (lab == K.reference(name)[3]).all() and (sizes == K.reference(name)[4]).all() and n_clusters == stats["clusters"]


def test_chain_behind_the_radius_filter_into_the_voxel_grid(arena):
    """pcs_radius_outlier_device_counted -> pcs_cluster_filter_device_counted -> pcs_voxel_grid_device_counted, no host round trip in
    between, equals the voxel grid of the two restatements applied in turn."""
    ctx = arena.ctx
    _, rec, params, _ = CASES["count2049"]
    r, k = 20, 1
    first = NR.radius_outlier(rec, r, k)
    want, _, stats = N.cluster_filter(first, *params)
    assert 0 < want.shape[0] < first.shape[0] < rec.shape[0]
    n, leaf = rec.shape[0], 40
    d_a, d_b = ctx.device_malloc(10 * n + 64), ctx.device_malloc(10 * n + 64)
    try:
        ctx.memcpy_h2d(arena.inp, np.ascontiguousarray(rec))
        ctx.memcpy_h2d(arena.words, np.array([n, SENTINEL, SENTINEL, SENTINEL], np.int32))
        ctx.radius_outlier_device_counted(arena.inp, arena.words, n, r, k, d_a, POINT_SHORTS * n, arena.words + 4)
        ctx.cluster_filter_device_counted(d_a, arena.words + 4, n, ClusterParams.make(*params), d_b, POINT_SHORTS * n, arena.words + 8,
                                          arena.stats)
        ctx.voxel_grid_device_counted(d_b, arena.words + 8, n, leaf, arena.out, POINT_SHORTS * n, arena.words + 12)
        ctx.synchronize()
        words = np.empty(4, np.int32)
        ctx.memcpy_d2h(words, arena.words)
        block = np.empty(8, np.int64)
        ctx.memcpy_d2h(block, arena.stats)
        assert words[1] == first.shape[0] and words[2] == want.shape[0]
        assert dict(zip(CLUSTER_STATS_FIELDS, (int(v) for v in block[:5]))) == stats
        ref = ctx.voxel_grid(want, leaf)
        assert 0 < ref.shape[0] < want.shape[0] and words[3] == ref.shape[0]
        got = np.empty((ref.shape[0], 5), np.int16)
        ctx.memcpy_d2h(got, arena.out)
        assert (got == ref).all()
    finally:
        ctx.device_free(d_a)
        ctx.device_free(d_b)


def test_kernel_timing_yields_one_interval_per_launch(arena):
    ctx = arena.ctx
    rec, params, want, stats = want_of("count257")
    ctx.kernel_timing(True)
    try:
        for with_stats, launches in ((True, CLUSTER_LAUNCHES), (False, CLUSTER_LAUNCHES - 1)):
            ctx.kernel_times_ms()                # drain
            got, kept, _ = arena.run(rec, params, with_stats=with_stats)
            times = ctx.kernel_times_ms()
            assert len(times) == launches and all(t >= 0 for t in times) and kept == want.shape[0]
        ctx.kernel_times_ms()
        arena.run_labels(rec, params[0])
        assert len(ctx.kernel_times_ms()) == CLUSTER_LABEL_LAUNCHES
    finally:
        ctx.kernel_timing(False)


def test_refusals_launch_nothing_and_write_nothing(arena):
    ctx = arena.ctx
    _, rec, params, _ = CASES["count2049"]
    n = rec.shape[0]
    d_in, d_out, d_cnt, d_n, d_st = arena.inp + 4, arena.out + 4, arena.words, arena.words + 4, arena.stats
    ctx.memcpy_h2d(d_in, np.ascontiguousarray(rec))
    ctx.memcpy_h2d(arena.out, np.full(4 + 10 * n + GUARD, 0xA5, np.uint8))
    ctx.memcpy_h2d(arena.words, np.array([SENTINEL, n], np.int32))
    ctx.memcpy_h2d(arena.stats, np.full(16, STATS_SENTINEL, np.int64))
    fill = np.full(n + GUARD // 4, SENTINEL, np.int32)
    ctx.memcpy_h2d(arena.labels, fill)
    ctx.memcpy_h2d(arena.sizes, fill)
    shorts = POINT_SHORTS * n
    tol, lo, hi = 20, 5, 9
    good = ClusterParams.make(tol, lo, hi)
    bad_params = [(ClusterParams.make(0, lo, hi), "tolerance_mm"), (ClusterParams.make(1001, lo, hi), "tolerance_mm"),
                  (ClusterParams.make(-1, lo, hi), "tolerance_mm"), (ClusterParams.make(tol, 0, hi), "min_size"),
                  (ClusterParams.make(tol, -3, 0), "min_size"), (ClusterParams.make(tol, lo, -1), "max_size"),
                  (ClusterParams.make(tol, lo, 1), "max_size"), (ClusterParams.make(tol, lo, lo - 1), "max_size"),
                  (ClusterParams.make(tol, lo, hi, reserved=1), "reserved"), (None, "params")]
    plain = [((d_in, n, P, d_out, shorts, d_cnt, d_st), word) for P, word in bad_params] + [
        ((d_in, -1, good, d_out, shorts, d_cnt, d_st), "n_points"),
        ((0, n, good, d_out, shorts, d_cnt, d_st), "d_payload"),
        ((d_in, n, good, 0, shorts, d_cnt, d_st), "d_out"),
        ((d_in, n, good, d_out, shorts, 0, d_st), "d_out_points"),
        ((d_in + 1, n, good, d_out, shorts, d_cnt, d_st), "d_payload"),
        ((d_in, n, good, d_out + 1, shorts, d_cnt, d_st), "d_out"),
        ((d_in, n, good, d_out, shorts, d_cnt + 2, d_st), "d_out_points"),
        ((d_in, n, good, d_out, shorts, d_cnt, d_st + 4), "d_stats"),
        ((d_in, n, good, d_out, shorts - 1, d_cnt, d_st), "out_shorts"),
        ((d_in, n, good, d_in, shorts, d_cnt, d_st), "overlap"),                 # in place
        ((d_in, n, good, d_in + 10 * n - 2, shorts, d_cnt, d_st), "overlap"),    # the input's last bytes
        ((d_in, n, good, d_in - 10 * n + 2, shorts, d_cnt, d_st), "overlap"),    # the input's first bytes
        ((d_in, n, good, d_out, shorts, d_out + 8, d_st), "overlap"),            # the count inside the output
        ((d_in, n, good, d_out, shorts, d_in + 8, d_st), "overlap"),             # ... inside the input
        ((d_in, n, good, d_out, shorts, d_cnt, d_out + 4), "overlap"),           # the block inside the output
        ((d_in, n, good, d_out, shorts, d_cnt, d_in + 12), "overlap"),           # ... inside the input
        ((d_in, n, good, d_out, shorts, d_st + 8, d_st), "overlap"),             # ... over the count
    ]
    for args, word in plain:
        with pytest.raises(PcsError) as e:
            ctx.cluster_filter_device(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_cluster_filter_device:" in str(e.value), (args, str(e.value))
    counted = [((d_in, d_n, n, P, d_out, shorts, d_cnt, d_st), word) for P, word in bad_params] + [
        ((d_in, 0, n, good, d_out, shorts, d_cnt, d_st), "d_n_points"),
        ((d_in, d_n + 2, n, good, d_out, shorts, d_cnt, d_st), "d_n_points"),
        ((d_in, d_n, -1, good, d_out, shorts, d_cnt, d_st), "max_points"),
        ((d_in, d_n, n, good, d_out, shorts - 1, d_cnt, d_st), "out_shorts"),
        ((d_in, d_n, n, good, d_out, shorts, d_cnt, d_st + 4), "d_stats"),
        ((d_in, d_n, n, good, d_in + 10, shorts, d_cnt, d_st), "overlap"),
        ((d_in, d_out + 8, n, good, d_out, shorts, d_cnt, d_st), "overlap"),
        ((d_in, d_cnt, n, good, d_out, shorts, d_cnt, d_st), "overlap"),
        ((d_in, d_st + 16, n, good, d_out, shorts, d_cnt, d_st), "overlap"),
    ]
    for args, word in counted:
        with pytest.raises(PcsError) as e:
            ctx.cluster_filter_device_counted(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_cluster_filter_device_counted:" in str(e.value), (args, str(e.value))
    d_lab, d_siz = arena.labels, arena.sizes
    labelled = [((d_in, n, 0, d_lab, d_siz, d_cnt), "tolerance_mm"), ((d_in, n, 1001, d_lab, d_siz, d_cnt), "tolerance_mm"),
                ((d_in, -1, tol, d_lab, d_siz, d_cnt), "n_points"), ((0, n, tol, d_lab, d_siz, d_cnt), "d_payload"),
                ((d_in, n, tol, 0, d_siz, d_cnt), "d_labels"), ((d_in, n, tol, d_lab, d_siz, 0), "d_n_clusters"),
                ((d_in + 1, n, tol, d_lab, d_siz, d_cnt), "d_payload"), ((d_in, n, tol, d_lab + 2, d_siz, d_cnt), "d_labels"),
                ((d_in, n, tol, d_lab, d_siz + 2, d_cnt), "d_sizes"), ((d_in, n, tol, d_lab, d_siz, d_cnt + 2), "d_n_clusters"),
                ((d_in, n, tol, d_in + 8, d_siz, d_cnt), "overlap"), ((d_in, n, tol, d_lab, d_in + 4 * n, d_cnt), "overlap"),
                ((d_in, n, tol, d_lab, d_lab + 4 * n - 4, d_cnt), "overlap"), ((d_in, n, tol, d_lab, d_siz, d_lab + 8), "overlap"),
                ((d_in, n, tol, d_lab, d_siz, d_in + 8), "overlap")]
    for args, word in labelled:
        with pytest.raises(PcsError) as e:
            ctx.cluster_labels_device(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_cluster_labels_device:" in str(e.value), (args, str(e.value))
    host_out = np.full((n, 5), 0x5A5A, np.uint16).view(np.int16)
    host_lab = np.full(n, SENTINEL, np.int32)
    cnt = C.c_int(SENTINEL)
    st = ClusterStatsC(*([STATS_SENTINEL] * 5))
    lib, h = ctx._lib, ctx._h
    p = np.ascontiguousarray(rec)
    ho = host_out.ctypes.data
    g = C.byref(good)
    host = [((p.ctypes.data, n, C.byref(P) if P is not None else None, ho, shorts, C.byref(cnt), C.byref(st)), word) for P, word in bad_params] + [
        ((p.ctypes.data, -3, g, ho, shorts, C.byref(cnt), C.byref(st)), "n_points"),
        ((None, n, g, ho, shorts, C.byref(cnt), C.byref(st)), "payload"),
        ((p.ctypes.data, n, g, None, shorts, C.byref(cnt), C.byref(st)), "out"),
        ((p.ctypes.data, n, g, ho, shorts, None, C.byref(st)), "out_points"),
        ((p.ctypes.data + 1, n, g, ho, shorts, C.byref(cnt), C.byref(st)), "payload"),
        ((p.ctypes.data, n, g, ho, shorts - 1, C.byref(cnt), C.byref(st)), "out_shorts"),
        ((p.ctypes.data, n, g, p.ctypes.data + 20, shorts, C.byref(cnt), C.byref(st)), "overlap"),
        ((p.ctypes.data, n, g, ho, shorts, C.byref(cnt), C.cast(ho + 16, C.POINTER(ClusterStatsC))), "overlap")]
    for args, word in host:
        assert lib.pcs_cluster_filter(h, *args) == -1
        text = lib.pcs_last_error(h).decode()
        assert word in text and "pcs_cluster_filter:" in text, text
    hl = host_lab.ctypes.data
    host_labels = [((p.ctypes.data, n, 0, hl, None, C.byref(cnt)), "tolerance_mm"), ((p.ctypes.data, n, tol, None, None, C.byref(cnt)), "labels"),
                   ((p.ctypes.data, n, tol, hl, None, None), "n_clusters"), ((None, n, tol, hl, None, C.byref(cnt)), "payload"),
                   ((p.ctypes.data, n, tol, hl + 2, None, C.byref(cnt)), "labels"), ((p.ctypes.data, n, tol, hl, hl + 8, C.byref(cnt)), "overlap"),
                   ((p.ctypes.data, n, tol, p.ctypes.data + 8, None, C.byref(cnt)), "overlap")]
    for args, word in host_labels:
        assert lib.pcs_cluster_labels(h, *args) == -1
        text = lib.pcs_last_error(h).decode()
        assert word in text and "pcs_cluster_labels:" in text, text
    assert cnt.value == SENTINEL and (host_out.view(np.uint16) == 0x5A5A).all() and st.considered == STATS_SENTINEL and st.kept == STATS_SENTINEL
    assert (host_lab == SENTINEL).all() and (p == rec).all()
    ctx.synchronize()
    out = np.empty(4 + 10 * n + GUARD, np.uint8)
    words = np.empty(2, np.int32)
    back = np.empty((n, 5), np.int16)
    block = np.empty(16, np.int64)
    lab, siz = np.empty_like(fill), np.empty_like(fill)
    ctx.memcpy_d2h(out, arena.out)
    ctx.memcpy_d2h(words, arena.words)
    ctx.memcpy_d2h(back, d_in)
    ctx.memcpy_d2h(block, arena.stats)
    ctx.memcpy_d2h(lab, arena.labels)
    ctx.memcpy_d2h(siz, arena.sizes)
    assert (out == 0xA5).all() and words[0] == SENTINEL and words[1] == n and (back == rec).all() and (block == STATS_SENTINEL).all()
    assert (lab == SENTINEL).all() and (siz == SENTINEL).all()


def test_zero_records_write_a_zero_count_and_a_zeroed_block(arena):
    zero = dict.fromkeys(CLUSTER_STATS_FIELDS, 0)
    empty = np.zeros((0, 5), np.int16)
    got, kept, block = arena.run(empty, (20, 1, 0))
    assert kept == 0 and block == zero
    got, kept, block = arena.run(empty, (20, 1, 0), d_count=7, max_points=0)
    assert kept == 0 and block == zero
    ctx = arena.ctx                 # with no records, payload and outputs may be NULL
    ctx.memcpy_h2d(arena.words, np.array([SENTINEL, SENTINEL], np.int32))
    ctx.cluster_filter_device(0, 0, ClusterParams.make(20, 1, 0), 0, 0, arena.words, 0)
    ctx.cluster_labels_device(0, 0, 20, 0, 0, arena.words + 4)
    ctx.synchronize()
    w = np.empty(2, np.int32)
    ctx.memcpy_d2h(w, arena.words)
    assert w[0] == 0 and w[1] == 0
    got, block = ctx.cluster_filter(empty, 20, 1, 0)
    assert got.shape == (0, 5) and block == zero
    lab, sizes, n_clusters = ctx.cluster_labels(empty, 20)
    assert lab.shape == (0,) and sizes.shape == (0,) and n_clusters == 0
