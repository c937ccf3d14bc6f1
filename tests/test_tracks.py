"""Object tracks on the GPU (pcs_tracker_*), byte for byte against the restatement of DESIGN.md section 3 (tests/np_tracks.py: Python
dicts and the rules literally) over the sequences of tests/track_cases.py: every update's tracks, statistics block and info; the
payload at the reference's `buffer + 2` shorts and at 16-byte alignment; 0xA5 guards in front of tracks and behind entry m, a
sentinel block behind the statistics; the counted and host forms; two runs; an update fed straight from the object table behind the
background subtraction with no host round trip; every refusal; the launch counts."""
import ctypes as C

import numpy as np
import pytest

import np_tracks as N
import track_cases as K
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import (BackgroundParams, ClusterObjectsOut, ClusterParams, POINT_SHORTS, TRACK_DTYPE, TRACK_STATS_FIELDS,
                                            TRACK_UPDATE_LAUNCHES, Track, TrackParams, TrackStats)

pytestmark = pytest.mark.gpu

GUARD = 64
N_MAX = 16384
M_MAX = 128
STATS_SENTINEL = 0x5A5A5A5A5A5A5A5A
NAMES = sorted(K.CASES)


def test_the_bindings_and_the_restatement_agree_on_the_layout():
    assert TRACK_DTYPE == N.TRACK_DTYPE and TRACK_STATS_FIELDS == N.STATS_FIELDS and len(TRACK_UPDATE_LAUNCHES) == 4


class Arena:
    """Device buffers shared by the tests of this module: a payload at any 2-byte phase, object_of, the count words, guarded tracks,
    a statistics block with a sentinel block behind it."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.inp = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.obj = ctx.device_malloc(4 * N_MAX + 64)
        self.words = ctx.device_malloc(64)          # [0] n_objects, [4] the counted form's record count
        self.tracks = ctx.device_malloc(GUARD + 24 * M_MAX + GUARD)
        self.stats = ctx.device_malloc(128)
        assert self.inp % 16 == 0 and self.tracks % 8 == 0

    def free(self):
        for p in (self.inp, self.obj, self.words, self.tracks, self.stats):
            self.ctx.device_free(p)

    def update(self, tr, s, in_phase=4, d_count=None, max_points=None, stats=True, extra=None):
        """One step on the device forms -> (tracks[m], statistics dict or None). extra: (records, object_of) behind the count of the
        counted form. Everything around tracks[0..m) must stay 0xA5, everything behind the block the sentinel."""
        ctx = self.ctx
        rec, obj = (s.rec, s.object_of) if extra is None else (np.concatenate([s.rec, extra[0]]), np.concatenate([s.object_of, extra[1]]))
        n = rec.shape[0]
        assert n <= N_MAX and s.max_objects <= M_MAX
        d_in = self.inp + in_phase
        if n:
            ctx.memcpy_h2d(d_in, np.ascontiguousarray(rec))
            ctx.memcpy_h2d(self.obj, np.ascontiguousarray(obj))
        span = GUARD + 24 * s.max_objects + GUARD
        ctx.memcpy_h2d(self.tracks, np.full(span, 0xA5, np.uint8))
        ctx.memcpy_h2d(self.words, np.array([s.n_objects, 0 if d_count is None else d_count], np.int32))
        ctx.memcpy_h2d(self.stats, np.full(16, STATS_SENTINEL, np.uint64))
        P = TrackParams.make(s.min_votes)
        d_tracks, d_stats = self.tracks + GUARD, self.stats if stats else 0
        if d_count is None:
            tr.update_device(d_in, n, self.obj, self.words, s.max_objects, P, d_tracks, d_stats)
        else:
            tr.update_device_counted(d_in, self.words + 4, max_points, self.obj, self.words, s.max_objects, P, d_tracks, d_stats)
        ctx.synchronize()
        got = np.empty(span, np.uint8)
        ctx.memcpy_d2h(got, self.tracks)
        block = np.empty(16, np.uint64)
        ctx.memcpy_d2h(block, self.stats)
        words = np.empty(2, np.int32)
        ctx.memcpy_d2h(words, self.words)
        assert words[0] == s.n_objects and words[1] == (0 if d_count is None else d_count)
        m = min(max(s.n_objects, 0), s.max_objects)
        assert (got[:GUARD] == 0xA5).all(), "bytes in front of d_tracks were written"
        assert (got[GUARD + 24 * m:] == 0xA5).all(), "bytes at or behind entry m were written"
        assert (block[8:] == STATS_SENTINEL).all(), "bytes behind the statistics block were written"
        if stats:
            st = dict(zip(TRACK_STATS_FIELDS, block[:8].astype(np.int64).tolist()))
        else:
            assert (block == STATS_SENTINEL).all()
            st = None
        return got[GUARD:GUARD + 24 * m].copy().view(TRACK_DTYPE), st


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


_REFERENCE = {}


def reference(name):
    """The restatement's (tracks, stats, info) per step of a case — computed once, shared, never changed."""
    if name not in _REFERENCE:
        case = K.CASES[name]
        tr, out = N.Tracker(case.cell_mm, case.max_cells, case.max_objects), []
        for s in case.steps:
            if s.reset is not None:
                tr.reset(s.reset)
            out.append(tr.update(s.rec, s.object_of, s.n_objects, s.max_objects, s.min_votes) + (tr.info(),))
        _REFERENCE[name] = out
    return _REFERENCE[name]


def run_case(arena, name, **kw):
    case = K.CASES[name]
    out = []
    with arena.ctx.tracker_create(case.cell_mm, case.max_cells, case.max_objects) as tr:
        for s in case.steps:
            if s.reset is not None:
                tr.reset(s.reset)
            out.append(arena.update(tr, s, **kw) + (tr.info(),))
    return out


def check_case(name, got):
    want = reference(name)
    assert len(got) == len(want)
    for t, ((tracks, st, info), (w_tracks, w_st, w_info)) in enumerate(zip(got, want)):
        assert tracks.tobytes() == w_tracks.tobytes(), (name, t, tracks, w_tracks)
        assert st is None or st == w_st, (name, t, st, w_st)
        assert info == w_info, (name, t, info, w_info)


@pytest.mark.parametrize("name", NAMES)
def test_every_update_matches_the_restatement(arena, name):
    """first / still, moved, runs, split and merge, shared cell, min_votes, range ends, ignored records, collisions, both overflows,
    reset, zero: tracks, statistics and info of every update, payload at buffer + 2 shorts."""
    check_case(name, run_case(arena, name))


def test_hand_written_expectations_hold_on_the_device(arena):
    for name in ("split_50_50", "merge_50_50", "chain", "reset_ids", "alternating"):
        for (tracks, _, _), rows in zip(run_case(arena, name), K.CASES[name].expect):
            assert tracks.tobytes() == K.expected_tracks(rows).tobytes(), (name, tracks)


@pytest.mark.parametrize("name", ["moved", "collisions", "run200", "range_ends_cell1"])
def test_sixteen_byte_aligned_payload_and_no_statistics(arena, name):
    check_case(name, run_case(arena, name, in_phase=0, stats=False))


def test_ids_survive_a_shuffled_record_order(arena):
    got = run_case(arena, "moved")
    perm = [3, 0, 4, 1, 2]
    assert [int(got[1][0]["id"][perm[k]]) for k in range(5)] == [1, 2, 3, 4, 5]
    assert got[2][0]["id"].tolist() == [1, 2, 3, 4, 5] and got[2][0]["age"].tolist() == [2] * 5


def test_overflow_words(arena):
    cells = run_case(arena, "overflow_cells")
    assert [st["overflow"] for _, st, _ in cells] == [0, 0, 2, 0] and [i["overflow"] for _, _, i in cells] == [0, 4, 2, 0]
    assert cells[2][1]["born"] == 3 and cells[2][1]["continued"] == 0 and cells[3][1]["continued"] == 3
    pairs = run_case(arena, "overflow_pairs")
    assert [st["overflow"] for _, st, _ in pairs] == [0, 1, 0, 0] and pairs[1][1]["born"] == 80 and pairs[2][1]["continued"] == 40


def test_two_runs_are_identical(arena):
    for name in ("collisions", "many_workgroups", "overflow_pairs"):
        a, b = run_case(arena, name), run_case(arena, name)
        for (ta, sa, ia), (tb, sb, ib) in zip(a, b):
            assert ta.tobytes() == tb.tobytes() and sa == sb and ia == ib


def test_counted_form(arena):
    """The count on the device: copies of members behind the count are not read; counts of 0, negative and above max_points."""
    case = K.CASES["moved"]
    want = reference("moved")
    with arena.ctx.tracker_create(case.cell_mm, case.max_cells, case.max_objects) as tr:
        for t, s in enumerate(case.steps):
            n = s.rec.shape[0]
            extra = (s.rec[:40].copy(), np.zeros(40, np.int32))            # members of object 0 behind the count
            tracks, st = arena.update(tr, s, d_count=n, max_points=n + 40, extra=extra)
            assert tracks.tobytes() == want[t][0].tobytes() and st == want[t][1] and tr.info() == want[t][2]
    s = case.steps[0]
    n = s.rec.shape[0]
    for d_count, seen in ((0, 0), (-5, 0), (n + 1000, n), (17, 17)):
        ref = N.Tracker(case.cell_mm, case.max_cells, case.max_objects)
        with arena.ctx.tracker_create(case.cell_mm, case.max_cells, case.max_objects) as tr:
            for _ in range(2):
                tracks, st = arena.update(tr, s, d_count=d_count, max_points=n)
                w_tracks, w_st = ref.update(s.rec[:seen], s.object_of[:seen], s.n_objects, s.max_objects, s.min_votes)
                assert tracks.tobytes() == w_tracks.tobytes() and st == w_st and tr.info() == ref.info(), (d_count, st, w_st)


def test_host_form(arena):
    for name in ("moved", "zero", "ignored", "reset_ids"):
        case, want = K.CASES[name], reference(name)
        with arena.ctx.tracker_create(case.cell_mm, case.max_cells, case.max_objects) as tr:
            for t, s in enumerate(case.steps):
                if s.reset is not None:
                    tr.reset(s.reset)
                tracks, st = tr.update(s.rec, s.object_of, s.n_objects, s.max_objects, s.min_votes)
                assert tracks.tobytes() == want[t][0].tobytes() and st == want[t][1] and tr.info() == want[t][2], (name, t)


def test_fed_from_the_library(arena):
    """counted subtract -> pcs_cluster_objects_device_counted -> pcs_tracker_update_device_counted over three frame-sets with no host
    round trip in between: the restatement's tracks for the restatements' objects."""
    import background_cases as BK
    import np_cluster_objects as NO
    ctx = arena.ctx
    case = BK.CASES["min_seen_groups"]
    model = BK.model_of("min_seen_groups")
    rec = case.payload
    n, tol, min_size, M = rec.shape[0], 60, 3, M_MAX
    assert n <= N_MAX
    frames = [rec, np.ascontiguousarray(rec[::-1]), rec]
    ref = N.Tracker(100, 4096, M)
    d_mid, d_table = ctx.device_malloc(10 * n + 64), ctx.device_malloc(80 * M)
    bg = ctx.background_create(case.cell_mm, case.max_cells)
    try:
        for f in case.frames:
            bg.learn(f)
        with ctx.tracker_create(100, 4096, M) as tr:
            for t, frame in enumerate(frames):
                kept = frame[model.subtract_mask(frame, 3, 0)]
                _, n_objects, object_of = NO.cluster_objects(kept, tol, min_size)
                assert 1 < n_objects <= M
                w_tracks, w_st = ref.update(kept, object_of, n_objects, M)
                ctx.memcpy_h2d(arena.inp, np.ascontiguousarray(frame))
                ctx.memcpy_h2d(arena.words, np.array([-1, n, -1], np.int32))
                ctx.memcpy_h2d(arena.tracks, np.full(GUARD + 24 * M + GUARD, 0xA5, np.uint8))
                bg.subtract_device_counted(arena.inp, arena.words + 4, n, BackgroundParams.make(3, 0), d_mid, POINT_SHORTS * n, arena.words)
                ctx.cluster_objects_device_counted(d_mid, arena.words, n, ClusterParams.make(tol, min_size, 0),
                                                   ClusterObjectsOut.make(objects=d_table, max_objects=M, n_objects=arena.words + 8,
                                                                          object_of=arena.obj))
                tr.update_device_counted(d_mid, arena.words, n, arena.obj, arena.words + 8, M, TrackParams.make(1), arena.tracks + GUARD,
                                         arena.stats)
                ctx.synchronize()
                got = np.empty(GUARD + 24 * M + GUARD, np.uint8)
                ctx.memcpy_d2h(got, arena.tracks)
                block = np.empty(8, np.int64)
                ctx.memcpy_d2h(block, arena.stats)
                assert got[GUARD:GUARD + 24 * n_objects].tobytes() == w_tracks.tobytes(), t
                assert (got[:GUARD] == 0xA5).all() and (got[GUARD + 24 * n_objects:] == 0xA5).all()
                assert dict(zip(TRACK_STATS_FIELDS, block.tolist())) == w_st, t
            assert w_st["continued"] + w_st["born"] == n_objects and w_st["continued"] > 0
    finally:
        bg.close()
        ctx.device_free(d_mid)
        ctx.device_free(d_table)


def test_refusals_launch_nothing_and_write_nothing(arena):
    ctx = arena.ctx
    case = K.CASES["moved"]
    s = case.steps[0]
    n, M = s.rec.shape[0], s.max_objects
    tr = ctx.tracker_create(case.cell_mm, case.max_cells, case.max_objects)
    arena.update(tr, s)
    before = tr.info()
    d_in, d_obj, d_m, d_n, d_tr, d_st = arena.inp + 4, arena.obj, arena.words, arena.words + 4, arena.tracks + GUARD, arena.stats
    ctx.memcpy_h2d(arena.tracks, np.full(GUARD + 24 * M + GUARD, 0xA5, np.uint8))
    ctx.memcpy_h2d(arena.stats, np.full(16, STATS_SENTINEL, np.uint64))
    ctx.memcpy_h2d(arena.words, np.array([s.n_objects, n], np.int32))
    ctx.kernel_timing(True)
    good = TrackParams.make(1)
    bad_params = [(TrackParams.make(0), "min_votes"), (TrackParams.make((1 << 30) + 1), "min_votes"), (TrackParams.make(1, (0, 1, 0)), "reserved"),
                  (TrackParams.make(1, (0, 0, 7)), "reserved"), (None, "params")]
    plain = [((d_in, n, d_obj, d_m, M, P, d_tr, d_st), word) for P, word in bad_params] + [
        ((d_in, -1, d_obj, d_m, M, good, d_tr, d_st), "n_points"),
        ((0, n, d_obj, d_m, M, good, d_tr, d_st), "d_payload"),
        ((d_in + 1, n, d_obj, d_m, M, good, d_tr, d_st), "d_payload"),
        ((d_in, n, 0, d_m, M, good, d_tr, d_st), "d_object_of"),
        ((d_in, n, d_obj + 2, d_m, M, good, d_tr, d_st), "d_object_of"),
        ((d_in, n, d_obj, 0, M, good, d_tr, d_st), "d_n_objects"),
        ((d_in, n, d_obj, d_m + 2, M, good, d_tr, d_st), "d_n_objects"),
        ((d_in, n, d_obj, d_m, -1, good, d_tr, d_st), "max_objects"),
        ((d_in, n, d_obj, d_m, case.max_objects + 1, good, d_tr, d_st), "max_objects"),
        ((d_in, n, d_obj, d_m, M, good, 0, d_st), "d_tracks"),
        ((d_in, n, d_obj, d_m, M, good, d_tr + 4, d_st), "d_tracks"),
        ((d_in, n, d_obj, d_m, M, good, d_tr, d_st + 4), "d_stats"),
        ((d_in, n, d_obj, d_m, M, good, d_in + 4, d_st), "overlap"),
        ((d_in, n, d_obj, d_m, M, good, d_obj + 8, d_st), "overlap"),
        ((d_in, n, d_obj, d_tr + 8, M, good, d_tr, d_st), "overlap"),
        ((d_in, n, d_obj, d_m, M, good, d_tr, d_tr + 16), "overlap"),
        ((d_in, n, d_obj, d_m, M, good, d_tr, d_m - 32), "overlap"),
        ((d_in, n, d_obj, d_m, M, good, d_tr, d_in + 12), "overlap"),
    ]
    for args, word in plain:
        with pytest.raises(PcsError) as e:
            tr.update_device(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_tracker_update_device:" in str(e.value), (word, str(e.value))
    counted = [((d_in, d_n, n, d_obj, d_m, M, P, d_tr, d_st), word) for P, word in bad_params] + [
        ((d_in, 0, n, d_obj, d_m, M, good, d_tr, d_st), "d_n_points"),
        ((d_in, d_n + 2, n, d_obj, d_m, M, good, d_tr, d_st), "d_n_points"),
        ((d_in, d_n, -1, d_obj, d_m, M, good, d_tr, d_st), "max_points"),
        ((d_in, d_n, n, d_obj, d_m, case.max_objects + 1, good, d_tr, d_st), "max_objects"),
        ((d_in, d_tr + 8, n, d_obj, d_m, M, good, d_tr, d_st), "overlap"),
        ((d_in, d_st + 16, n, d_obj, d_m, M, good, d_tr, d_st), "overlap"),
    ]
    for args, word in counted:
        with pytest.raises(PcsError) as e:
            tr.update_device_counted(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_tracker_update_device_counted:" in str(e.value), (word, str(e.value))
    lib, h = ctx._lib, ctx._h
    assert lib.pcs_tracker_update_device(h, None, d_in, n, d_obj, d_m, M, C.byref(good), d_tr, d_st) == -1
    assert "pcs_tracker_update_device: tr is NULL" in lib.pcs_last_error(h).decode()
    assert lib.pcs_tracker_reset(h, None, 1) == -1 and lib.pcs_tracker_destroy(h, None) == -1 and lib.pcs_tracker_info(h, None, None) == -1
    assert lib.pcs_tracker_info(h, tr.handle, None) == -1
    for first_id in (0, -1, (1 << 62) + 1):
        with pytest.raises(PcsError) as e:
            tr.reset(first_id)
        assert e.value.status == -1 and "first_id" in str(e.value)
    for args, word in (((0, 64, 4), "cell_mm"), ((1001, 64, 4), "cell_mm"), ((100, 0, 4), "max_cells"), ((100, (1 << 26) + 1, 4), "max_cells"),
                       ((100, 64, 0), "max_objects"), ((100, 64, 65537), "max_objects")):
        with pytest.raises(PcsError) as e:
            ctx.tracker_create(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_tracker_create" in str(e.value)
    # the host form
    p, o = np.ascontiguousarray(s.rec), np.ascontiguousarray(s.object_of)
    host_tracks = np.full(24 * M, 0x5A, np.uint8)
    host_stats = TrackStats(*([-7] * 8))
    ht, g = host_tracks.ctypes.data_as(C.POINTER(Track)), C.byref(good)
    for args, word in (((p.ctypes.data, n, o.ctypes.data, s.n_objects, M, C.byref(bad_params[0][0]), ht, C.byref(host_stats)), "min_votes"),
                       ((p.ctypes.data, -3, o.ctypes.data, s.n_objects, M, g, ht, C.byref(host_stats)), "n_points"),
                       ((None, n, o.ctypes.data, s.n_objects, M, g, ht, C.byref(host_stats)), "payload"),
                       ((p.ctypes.data + 1, n, o.ctypes.data, s.n_objects, M, g, ht, C.byref(host_stats)), "payload"),
                       ((p.ctypes.data, n, None, s.n_objects, M, g, ht, C.byref(host_stats)), "object_of"),
                       ((p.ctypes.data, n, o.ctypes.data, s.n_objects, case.max_objects + 1, g, ht, C.byref(host_stats)), "max_objects"),
                       ((p.ctypes.data, n, o.ctypes.data, s.n_objects, M, g, None, C.byref(host_stats)), "tracks"),
                       ((p.ctypes.data, n, o.ctypes.data, s.n_objects, M, g, C.cast(p.ctypes.data + 16, C.POINTER(Track)), C.byref(host_stats)),
                        "overlap")):
        assert lib.pcs_tracker_update(h, tr.handle, *args) == -1
        text = lib.pcs_last_error(h).decode()
        assert word in text and "pcs_tracker_update:" in text, text
    assert (host_tracks == 0x5A).all() and host_stats.as_dict() == dict.fromkeys(TRACK_STATS_FIELDS, -7)
    ctx.synchronize()
    assert ctx.kernel_times_ms().shape[0] == 0                      # nothing was launched
    ctx.kernel_timing(False)
    out = np.empty(GUARD + 24 * M + GUARD, np.uint8)
    block = np.empty(16, np.uint64)
    words = np.empty(2, np.int32)
    ctx.memcpy_d2h(out, arena.tracks)
    ctx.memcpy_d2h(block, arena.stats)
    ctx.memcpy_d2h(words, arena.words)
    assert (out == 0xA5).all() and (block == STATS_SENTINEL).all() and words.tolist() == [s.n_objects, n]
    assert tr.info() == before                                      # the tracker is what it was
    tracks, st = arena.update(tr, s)                                # ... and goes on as if nothing had been asked
    assert st["continued"] == s.n_objects and st["frames"] == 2
    tr.destroy()


def test_kernel_timing_counts_the_launches(arena):
    """One finite interval >= 0 per launch: every update 4 in all three forms, whatever the counts; create 1, reset 1 — and timing
    changes no byte."""
    ctx = arena.ctx
    case, want = K.CASES["moved"], reference("moved")
    empty = K.Step(np.zeros((0, 5), np.int16), np.zeros(0, np.int32), 0, 4, 1, None)
    ctx.kernel_timing(True)
    try:
        def launches(fn):
            out = fn()
            ctx.synchronize()
            t = ctx.kernel_times_ms()
            assert np.isfinite(t).all() and (t >= 0).all()
            return t.shape[0], out
        k, tr = launches(lambda: ctx.tracker_create(case.cell_mm, case.max_cells, case.max_objects))
        assert k == 1
        for t, s in enumerate(case.steps):
            k, (tracks, st) = launches(lambda: arena.update(tr, s))
            assert k == len(TRACK_UPDATE_LAUNCHES) == 4 and tracks.tobytes() == want[t][0].tobytes() and st == want[t][1]
        assert launches(lambda: arena.update(tr, case.steps[0], stats=False))[0] == 4
        assert launches(lambda: arena.update(tr, case.steps[0], d_count=3, max_points=case.steps[0].rec.shape[0]))[0] == 4
        assert launches(lambda: arena.update(tr, empty))[0] == 4
        assert launches(lambda: arena.update(tr, empty, d_count=5, max_points=0))[0] == 4
        assert launches(lambda: tr.update(case.steps[0].rec, case.steps[0].object_of, 5, 16))[0] == 4
        assert launches(lambda: tr.reset(9))[0] == 1
        assert tr.info() == dict(want[0][2], objects=0, frames=0, next_id=9, overflow=0)
        tr.destroy()
    finally:
        ctx.kernel_timing(False)


def test_destroying_the_context_frees_its_trackers():
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    s = K.CASES["first_still"].steps[0]
    with PcsContext(cfgs) as c:
        left = [c.tracker_create(100, 1 << 12, 64) for _ in range(3)]
        left[1].destroy()
        tracks, st = left[0].update(s.rec, s.object_of, s.n_objects, s.max_objects)
        assert st["born"] == 5
    left[0].destroy()           # destroying a tracker after its context is a no-op on the Python side
