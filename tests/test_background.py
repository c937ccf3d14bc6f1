"""The background model and its subtraction on the GPU (pcs_background_*), byte for byte against the restatement of DESIGN.md section
3 (tests/np_background.py: a Python dict and brute force over the up-to-27 cells) over the clouds of tests/background_cases.py: at the
reference's `buffer + 2` shorts and at 16-byte alignment, at every 2-byte phase of input and output for one cloud, with guard bytes in
front of the output, behind the kept records and behind the worst case, a sentinel in the count word; the model's exported bytes
against the restatement's; permuted and doubled frame-sets; export -> import -> export; the counted, host and device forms; both modes;
overflow; into the voxel grid and the object table with no host round trip; every refusal; zero records; kernel timing."""
import ctypes as C

import numpy as np
import pytest

import background_cases as K
import np_background as N
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError, background_validate
from pointcloud_stitching_amd.types import (BACKGROUND_MODE_KEEP, BACKGROUND_MODE_REMOVE, BACKGROUND_STATS_FIELDS, BackgroundParams,
                                            ClusterObjectsOut, ClusterParams, FLAG_CUTOFF, FLAG_DROP_INVALID, FLAG_SCALAR_ARITH, POINT_SHORTS)

pytestmark = pytest.mark.gpu

GUARD = 64                      # bytes of 0xA5 in front of the output, behind the kept records and behind the worst-case output
N_MAX = 65536
SENTINEL = 0x5A5A5A5A
STATS_SENTINEL = 0x5A5A5A5A5A5A5A5A
NAMES = sorted(K.CASES)


class Arena:
    """Device buffers shared by the tests of this module: an input and an output payload at any 2-byte phase, the count words, a
    statistics block."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.inp = ctx.device_malloc(64 + 10 * 2 * N_MAX + 64)
        self.out = ctx.device_malloc(GUARD + 64 + 10 * N_MAX + GUARD + 64)
        self.words = ctx.device_malloc(64)          # [0] the kept count, [4] the counted form's input count
        self.stats = ctx.device_malloc(128)
        assert self.inp % 16 == 0 and self.out % 16 == 0

    def free(self):
        for p in (self.inp, self.out, self.words, self.stats):
            self.ctx.device_free(p)

    def learn(self, bg, rec, d_count=None, max_points=None):
        ctx = self.ctx
        if rec.shape[0]:
            ctx.memcpy_h2d(self.inp + 4, np.ascontiguousarray(rec))
        if d_count is None:
            bg.learn_device(self.inp + 4, rec.shape[0])
        else:
            ctx.memcpy_h2d(self.words + 4, np.array([d_count], np.int32))
            bg.learn_device_counted(self.inp + 4, self.words + 4, max_points)
        ctx.synchronize()

    def model(self, case, frames=None):
        bg = self.ctx.background_create(case.cell_mm, case.max_cells)
        for rec in (case.frames if frames is None else frames):
            self.learn(bg, rec)
        return bg

    def run(self, bg, rec, min_seen, dilate, mode=0, in_phase=4, out_phase=4, d_count=None, max_points=None, stats=True):
        """rec at phase in_phase (bytes mod 16) -> (kept records, kept count, statistics dict) written at out_phase; everything around
        the kept records must stay 0xA5. d_count: the counted form with that count on the device and max_points as its capacity."""
        ctx = self.ctx
        cap = rec.shape[0] if d_count is None else max_points
        d_in, d_out = self.inp + in_phase, self.out + GUARD + out_phase
        if rec.shape[0]:
            ctx.memcpy_h2d(d_in, np.ascontiguousarray(rec))
        span = GUARD + out_phase + 10 * cap + GUARD
        ctx.memcpy_h2d(self.out, np.full(span, 0xA5, np.uint8))
        ctx.memcpy_h2d(self.words, np.array([SENTINEL, 0 if d_count is None else d_count, SENTINEL], np.int32))
        ctx.memcpy_h2d(self.stats, np.full(16, STATS_SENTINEL, np.uint64))
        P = BackgroundParams.make(min_seen, dilate, mode)
        d_stats = self.stats if stats else 0
        if d_count is None:
            bg.subtract_device(d_in, cap, P, d_out, POINT_SHORTS * cap, self.words, d_stats)
        else:
            bg.subtract_device_counted(d_in, self.words + 4, cap, P, d_out, POINT_SHORTS * cap, self.words, d_stats)
        ctx.synchronize()
        got = np.empty(span, np.uint8)
        ctx.memcpy_d2h(got, self.out)
        words = np.empty(3, np.int32)
        ctx.memcpy_d2h(words, self.words)
        block = np.empty(16, np.uint64)
        ctx.memcpy_d2h(block, self.stats)
        kept = int(words[0])
        assert 0 <= kept <= cap, kept
        assert words[1] == (0 if d_count is None else d_count) and words[2] == SENTINEL
        lo = GUARD + out_phase
        assert (got[:lo] == 0xA5).all(), "bytes in front of d_out were written"
        assert (got[lo + 10 * kept:] == 0xA5).all(), "bytes behind the kept records were written"
        assert (block[8:] == STATS_SENTINEL).all(), "bytes behind the statistics block were written"
        if stats:
            st = dict(zip(BACKGROUND_STATS_FIELDS, block[:7].astype(np.int64).tolist()))
            assert block[7] == 0
        else:
            assert (block == STATS_SENTINEL).all()
            st = None
        return got[lo:lo + 10 * kept].copy().view(np.int16).reshape(kept, 5), kept, st


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


@pytest.fixture(scope="module")
def models(arena):
    """One learned model per case, shared and never changed by the tests that take it."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = arena.model(K.CASES[name])
        return made[name]
    yield get
    for bg in made.values():
        bg.close()


def check_stats(st, case, want_kept, n, min_seen, mode=0):
    m = K.model_of(case.name)
    assert st == {"considered": n, "kept": want_kept, "background": want_kept if mode else n - want_kept, "cells": len(m.seen),
                  "frames": m.frames, "min_seen": min_seen, "overflow": 0}, st


def test_the_cases_keep_and_drop():
    K.check()


@pytest.mark.parametrize("name", NAMES)
def test_model_and_subtract_match_the_restatement(arena, models, name):
    case, bg = K.CASES[name], models(name)
    assert bg.export() == K.model_of(name).export()
    assert bg.info() == {"cell_mm": case.cell_mm, "max_cells": case.max_cells, "cells": len(K.model_of(name).seen), "frames": len(case.frames),
                         "overflow": 0}
    rec = case.payload
    for (min_seen, dilate), is_bg in K.reference(name).items():
        want = rec[~is_bg]
        for in_phase, out_phase in ((4, 4), (0, 0)):            # buffer + 2 shorts; 16-byte aligned
            got, kept, st = arena.run(bg, rec, min_seen, dilate, in_phase=in_phase, out_phase=out_phase)
            assert kept == want.shape[0], (name, min_seen, dilate, kept, want.shape[0])
            assert (got == want).all(), (name, min_seen, dilate)
            if rec.shape[0]:
                check_stats(st, case, kept, rec.shape[0], min_seen)
            else:
                assert set(st.values()) == {0}                  # nothing launched: a zeroed block
    assert bg.export() == K.model_of(name).export()             # subtract changes nothing


def test_every_phase_of_input_and_output(arena, models):
    case, bg = K.CASES["count2049"], models("count2049")
    is_bg = K.reference("count2049")[(3, 1)]
    want = case.payload[~is_bg]
    assert 0 < want.shape[0] < case.payload.shape[0]
    for in_phase in range(0, 16, 2):
        for out_phase in range(0, 16, 2):
            got, kept, _ = arena.run(bg, case.payload, 3, 1, in_phase=in_phase, out_phase=out_phase, stats=False)
            assert kept == want.shape[0] and (got == want).all(), (in_phase, out_phase)


def test_keep_mode_is_the_complement(arena, models):
    for name, p in (("count6161", (3, 1)), ("dilate_shapes", (1, 1)), ("range_ends_cell1", (1, 1))):
        case, bg = K.CASES[name], models(name)
        is_bg = K.reference(name)[p]
        removed, _, st0 = arena.run(bg, case.payload, *p, mode=BACKGROUND_MODE_REMOVE)
        kept_bg, _, st1 = arena.run(bg, case.payload, *p, mode=BACKGROUND_MODE_KEEP)
        assert (removed == case.payload[~is_bg]).all() and (kept_bg == case.payload[is_bg]).all()
        assert removed.shape[0] + kept_bg.shape[0] == case.payload.shape[0]
        check_stats(st1, case, kept_bg.shape[0], case.payload.shape[0], p[0], mode=1)
        assert st0["background"] == st1["background"] == int(is_bg.sum())


def test_identical_records_are_one_cell():
    """65 536 identical records: one cell, seen += 1 per learn call; subtract drops all of them or none by min_seen."""
    rec = K.identical(N_MAX)
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs) as c:
        a = Arena(c)
        try:
            with c.background_create(25, 16) as bg:
                for _ in range(3):
                    a.learn(bg, rec)
                assert bg.export() == N.learned(25, 16, [rec[:1]] * 3).export()
                got, kept, st = a.run(bg, rec, 3, 0)
                assert kept == 0 and st["background"] == N_MAX and st["cells"] == 1 and st["frames"] == 3
                got, kept, st = a.run(bg, rec, 4, 1)
                assert kept == N_MAX and (got == rec).all() and st["background"] == 0
        finally:
            a.free()


def test_the_model_is_order_free_and_idempotent_within_a_frame(arena):
    case = K.CASES["count6161"]
    want = K.model_of("count6161").export()
    rng = np.random.default_rng(3)
    permuted = [rec[rng.permutation(rec.shape[0])] for rec in case.frames]
    doubled = [np.concatenate([rec, rec]) for rec in case.frames]
    sorted_by_cell = [rec[np.lexsort(N.cells_of(rec, case.cell_mm).T)] for rec in case.frames]      # long runs of equal keys in a wave
    for frames in (permuted, doubled, sorted_by_cell):
        with arena.model(case, frames) as bg:
            assert bg.export() == want


def test_two_runs_give_identical_bytes(arena, models):
    case = K.CASES["count6161"]
    with arena.model(case) as a, arena.model(case) as b:
        assert a.export() == b.export() == a.export()
        ra, na, _ = arena.run(a, case.payload, 3, 1)
        rb, nb, _ = arena.run(b, case.payload, 3, 1)
        rc, nc, _ = arena.run(a, case.payload, 3, 1)
    assert na == nb == nc and ra.tobytes() == rb.tobytes() == rc.tobytes()


def test_export_import_export_is_the_identity(arena, models):
    for name, p in (("count6161", (3, 1)), ("wrap_probes", (2, 1)), ("min_seen_groups", (3, 0))):
        case, bg = K.CASES[name], models(name)
        blob = bg.export()
        assert background_validate(blob) == {"cell_mm": case.cell_mm, "max_cells": len(K.model_of(name).seen), "cells": len(K.model_of(name).seen),
                                             "frames": len(case.frames), "overflow": 0}
        before, nb, _ = arena.run(bg, case.payload, *p)
        with arena.ctx.background_import(blob, case.max_cells) as twin:
            assert twin.export() == blob
            assert twin.info() == bg.info()
            after, na, st = arena.run(twin, case.payload, *p)
            assert na == nb and after.tobytes() == before.tobytes()
            check_stats(st, case, na, case.payload.shape[0], p[0])
            # an imported model goes on learning where the exported one stopped
            arena.learn(twin, case.payload)
            m = N.learned(case.cell_mm, case.max_cells, list(case.frames) + [case.payload])
            if not m.overflow:
                assert twin.export() == m.export()
    empty = arena.ctx.background_create(7, 5)
    blob = empty.export()
    assert blob == N.Model(7, 5).export() and len(blob) == 32
    with arena.ctx.background_import(blob, 5) as twin:
        assert twin.export() == blob
    empty.close()
    with pytest.raises(PcsError) as e:
        arena.ctx.background_import(models("count6161").export(), 100)
    assert e.value.status == -5 and "max_cells" in str(e.value)
    bad = bytearray(models("dilate_shapes").export())
    bad[32 + 6] = 1
    with pytest.raises(PcsError) as e:
        arena.ctx.background_import(bytes(bad), 64)
    assert e.value.status == -1 and "padding" in str(e.value) and "pcs_background_import" in str(e.value)


def test_counted_forms_read_their_count_on_the_device(arena, models):
    case, bg = K.CASES["count6161"], models("count6161")
    rec, n = case.payload, case.payload.shape[0]
    m = K.model_of("count6161")
    for d_count, cap in ((2049, n), (n, n), (0, n), (n + 1000, n), (-5, n), (2**31 - 1, 2049)):
        used = max(0, min(d_count, cap))
        want = rec[:used][~m.background_mask(rec[:used], 3, 1)]
        got, kept, st = arena.run(bg, rec[:cap], 3, 1, d_count=d_count, max_points=cap)
        assert kept == want.shape[0] and (got == want).all(), (d_count, cap)
        assert st["considered"] == used and st["kept"] == kept
    frame = case.frames[0]
    nf = frame.shape[0]
    for d_count, cap in ((2049, nf), (nf, nf), (0, nf), (nf + 1000, nf), (-5, nf), (2**31 - 1, 2049)):
        used = max(0, min(d_count, cap))
        with arena.ctx.background_create(case.cell_mm, case.max_cells) as one:
            arena.learn(one, frame[:cap], d_count=d_count, max_points=cap)
            assert one.export() == N.learned(case.cell_mm, case.max_cells, [frame[:used]]).export(), (d_count, cap)


def test_host_forms_agree_with_the_device_forms(arena, models):
    for name, p in (("count6161", (3, 1)), ("count0", (3, 0)), ("count1", (1, 0)), ("range_ends_cell1", (1, 1))):
        case, bg = K.CASES[name], models(name)
        want = case.payload[~K.reference(name)[p]]
        got, st = bg.subtract(case.payload, *p)
        dev, _, dst = arena.run(bg, case.payload, *p)
        assert got.shape == want.shape and (got == want).all() and (got == dev).all(), name
        if case.payload.shape[0]:
            assert st == dst
        with arena.ctx.background_create(case.cell_mm, case.max_cells) as host_learned:
            for rec in case.frames:
                host_learned.learn(rec)
            assert host_learned.export() == bg.export()


def test_works_on_any_context(models):
    """No context predicate is read: a PCS_FLAG_SCALAR_ARITH context, and one with flags and a crop box, give the same bytes."""
    case = K.CASES["count2049"]
    want_blob = K.model_of("count2049").export()
    want = case.payload[~K.reference("count2049")[(3, 1)]]
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs, flags=FLAG_SCALAR_ARITH) as c:
        with c.background_create(case.cell_mm, case.max_cells) as bg:
            for rec in case.frames:
                bg.learn(rec)
            assert bg.export() == want_blob
            got, _ = bg.subtract(case.payload, 3, 1)
    assert got.shape == want.shape and (got == want).all()
    with PcsContext(cfgs, flags=FLAG_CUTOFF | FLAG_DROP_INVALID, downsample=3) as c:
        c.set_crop_box_mm((-10, -10, -10), (10, 10, 10))
        bg = c.background_import(want_blob, case.max_cells)
        got, _ = bg.subtract(case.payload, 3, 1)
        assert bg.export() == want_blob
        # (left open: the context's close frees it)
    assert got.shape == want.shape and (got == want).all()


def test_reset_gives_the_freshly_created_model(arena):
    case = K.CASES["min_seen_groups"]
    with arena.model(case) as bg:
        bg.reset()
        assert bg.export() == N.Model(case.cell_mm, case.max_cells).export()
        assert bg.info()["cells"] == 0 and bg.info()["frames"] == 0
        for rec in case.frames:
            arena.learn(bg, rec)
        assert bg.export() == K.model_of(case.name).export()


def test_overflow_is_sticky_and_keeps_everything(arena):
    rec65 = K.distinct_cells(65)
    with arena.ctx.background_create(100, 64) as bg:
        arena.learn(bg, rec65[:64])
        assert bg.info()["overflow"] == 0 and bg.info()["cells"] == 64
        assert bg.export() == N.learned(100, 64, [rec65[:64]]).export()
        arena.learn(bg, rec65)
        info = bg.info()
        assert info["overflow"] == 1 and info["frames"] == 2 and info["cells"] >= 65
        with pytest.raises(PcsError) as e:
            bg.export()
        assert e.value.status == -5 and "overflow" in str(e.value)
        for mode in (0, 1):
            got, kept, st = arena.run(bg, rec65, 1, 1, mode=mode)
            assert kept == 65 and (got == rec65).all()
            assert st["overflow"] == 1 and st["background"] == 0 and st["considered"] == st["kept"] == 65
        got, st = bg.subtract(rec65, 1, 0)
        assert got.shape[0] == 65 and st["overflow"] == 1
        arena.learn(bg, rec65[:3])
        assert bg.info()["overflow"] == 1                       # sticky
        bg.reset()
        assert bg.info() == {"cell_mm": 100, "max_cells": 64, "cells": 0, "frames": 0, "overflow": 0}
        arena.learn(bg, rec65[1:])
        assert bg.export() == N.learned(100, 64, [rec65[1:]]).export()
    # far more cells than slots: every probe loop ends, the flag is set, nothing is written outside the table (the models around it)
    flood = K.with_colour(np.random.default_rng(8).integers(-32768, 32768, (N_MAX, 3)))
    with arena.ctx.background_create(1, 64) as small, arena.ctx.background_create(1, 64) as neighbour:
        arena.learn(neighbour, rec65[:10])
        arena.learn(small, flood)
        assert small.info()["overflow"] == 1
        got, kept, _ = arena.run(small, flood[:6161], 1, 1)
        assert kept == 6161 and (got == flood[:6161]).all()
        assert neighbour.export() == N.learned(1, 64, [rec65[:10]]).export()


def test_chain_into_the_voxel_grid(arena, models):
    """counted subtract -> pcs_voxel_grid_device_counted, no host round trip in between, equals the voxel grid of the restatement's
    kept records."""
    ctx = arena.ctx
    case, bg = K.CASES["count6161"], models("count6161")
    rec = case.payload
    want = rec[~K.reference("count6161")[(3, 1)]]
    n, leaf = rec.shape[0], 40
    d_mid = ctx.device_malloc(10 * n + 64)
    try:
        ctx.memcpy_h2d(arena.inp, np.ascontiguousarray(rec))
        ctx.memcpy_h2d(arena.words, np.array([SENTINEL, n, SENTINEL], np.int32))
        bg.subtract_device_counted(arena.inp, arena.words + 4, n, BackgroundParams.make(3, 1), d_mid, POINT_SHORTS * n, arena.words)
        ctx.voxel_grid_device_counted(d_mid, arena.words, n, leaf, arena.out, POINT_SHORTS * n, arena.words + 8)
        ctx.synchronize()
        words = np.empty(3, np.int32)
        ctx.memcpy_d2h(words, arena.words)
        assert words[0] == want.shape[0]
        ref = ctx.voxel_grid(want, leaf)
        assert 0 < ref.shape[0] < want.shape[0] and words[2] == ref.shape[0]
        got = np.empty((ref.shape[0], 5), np.int16)
        ctx.memcpy_d2h(got, arena.out)
        assert (got == ref).all()
    finally:
        ctx.device_free(d_mid)


def test_chain_into_the_object_table(arena, models):
    """counted subtract -> pcs_cluster_objects_device_counted with no host round trip: the table of the restatement's kept records."""
    import np_cluster_objects as NO
    ctx = arena.ctx
    case, bg = K.CASES["min_seen_groups"], models("min_seen_groups")
    rec = case.payload
    want = rec[~K.reference("min_seen_groups")[(3, 0)]]
    n, tol, min_size, M = rec.shape[0], 60, 3, 512
    table, n_objects, _ = NO.cluster_objects(want, tol, min_size)
    assert 1 < n_objects <= M
    d_mid, d_table = ctx.device_malloc(10 * n + 64), ctx.device_malloc(80 * M)
    try:
        ctx.memcpy_h2d(arena.inp, np.ascontiguousarray(rec))
        ctx.memcpy_h2d(arena.words, np.array([SENTINEL, n, SENTINEL], np.int32))
        bg.subtract_device_counted(arena.inp, arena.words + 4, n, BackgroundParams.make(3, 0), d_mid, POINT_SHORTS * n, arena.words)
        ctx.cluster_objects_device_counted(d_mid, arena.words, n, ClusterParams.make(tol, min_size, 0),
                                           ClusterObjectsOut.make(objects=d_table, max_objects=M, n_objects=arena.words + 8))
        ctx.synchronize()
        words = np.empty(3, np.int32)
        ctx.memcpy_d2h(words, arena.words)
        assert words[0] == want.shape[0] and words[2] == n_objects
        raw = np.empty(80 * n_objects, np.uint8)
        ctx.memcpy_d2h(raw, d_table)
        assert raw.tobytes() == table.tobytes()
    finally:
        ctx.device_free(d_mid)
        ctx.device_free(d_table)


def test_refusals_launch_nothing_and_write_nothing(arena):
    ctx = arena.ctx
    case = K.CASES["count2049"]
    rec, n = case.payload, case.payload.shape[0]
    bg = arena.model(case)
    blob = bg.export()
    d_in, d_out, d_cnt, d_n, d_st = arena.inp + 4, arena.out + 4, arena.words, arena.words + 4, arena.stats
    ctx.memcpy_h2d(d_in, np.ascontiguousarray(rec))
    ctx.memcpy_h2d(arena.out, np.full(4 + 10 * n + GUARD, 0xA5, np.uint8))
    ctx.memcpy_h2d(arena.words, np.array([SENTINEL, n], np.int32))
    ctx.memcpy_h2d(arena.stats, np.full(16, STATS_SENTINEL, np.uint64))
    ctx.kernel_timing(True)
    shorts = POINT_SHORTS * n
    good = BackgroundParams.make(3, 1)
    bad_params = [(BackgroundParams.make(0, 1), "min_seen"), (BackgroundParams.make(65536, 1), "min_seen"), (BackgroundParams.make(3, 2), "dilate"),
                  (BackgroundParams.make(3, -1), "dilate"), (BackgroundParams.make(3, 1, 2), "mode"), (BackgroundParams.make(3, 1, 0, 1), "reserved"),
                  (None, "params")]
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
        ((d_in, n, good, d_in, shorts, d_cnt, d_st), "overlap"),
        ((d_in, n, good, d_in + 10 * n - 2, shorts, d_cnt, d_st), "overlap"),
        ((d_in, n, good, d_out, shorts, d_out + 8, d_st), "overlap"),
        ((d_in, n, good, d_out, shorts, d_in + 8, d_st), "overlap"),
        ((d_in, n, good, d_out, shorts, d_cnt, d_out + 4), "overlap"),
        ((d_in, n, good, d_out, shorts, d_cnt, d_cnt - 32), "overlap"),
    ]
    for args, word in plain:
        with pytest.raises(PcsError) as e:
            bg.subtract_device(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_background_subtract_device:" in str(e.value), (word, str(e.value))
    counted = [((d_in, d_n, n, P, d_out, shorts, d_cnt, d_st), word) for P, word in bad_params] + [
        ((d_in, 0, n, good, d_out, shorts, d_cnt, d_st), "d_n_points"),
        ((d_in, d_n + 2, n, good, d_out, shorts, d_cnt, d_st), "d_n_points"),
        ((d_in, d_n, -1, good, d_out, shorts, d_cnt, d_st), "max_points"),
        ((d_in, d_n, n, good, d_out, shorts - 1, d_cnt, d_st), "out_shorts"),
        ((d_in, d_n, n, good, d_in + 10, shorts, d_cnt, d_st), "overlap"),
        ((d_in, d_out + 8, n, good, d_out, shorts, d_cnt, d_st), "overlap"),
        ((d_in, d_cnt, n, good, d_out, shorts, d_cnt, d_st), "overlap"),
        ((d_in, d_st + 16, n, good, d_out, shorts, d_cnt, d_st), "overlap"),
    ]
    for args, word in counted:
        with pytest.raises(PcsError) as e:
            bg.subtract_device_counted(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_background_subtract_device_counted:" in str(e.value), (word, str(e.value))
    for fn, args, word in ((bg.learn_device, (d_in, -1), "n_points"), (bg.learn_device, (0, n), "d_payload"), (bg.learn_device, (d_in + 1, n), "d_payload"),
                           (bg.learn_device_counted, (d_in, 0, n), "d_n_points"), (bg.learn_device_counted, (d_in, d_n + 2, n), "d_n_points"),
                           (bg.learn_device_counted, (d_in, d_n, -1), "max_points"), (bg.learn_device_counted, (0, d_n, n), "d_payload")):
        with pytest.raises(PcsError) as e:
            fn(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_background_learn_device" in str(e.value), (word, str(e.value))
    # a NULL model, bad constants
    lib, h = ctx._lib, ctx._h
    assert lib.pcs_background_learn_device(h, None, d_in, n) == -1 and "bg is NULL" in lib.pcs_last_error(h).decode()
    assert lib.pcs_background_subtract_device(h, None, d_in, n, C.byref(good), d_out, shorts, d_cnt, d_st) == -1
    assert "pcs_background_subtract_device: bg is NULL" in lib.pcs_last_error(h).decode()
    assert lib.pcs_background_reset(h, None) == -1 and lib.pcs_background_destroy(h, None) == -1
    for cell_mm, max_cells, word in ((0, 64, "cell_mm"), (1001, 64, "cell_mm"), (20, 0, "max_cells"), (20, (1 << 26) + 1, "max_cells")):
        with pytest.raises(PcsError) as e:
            ctx.background_create(cell_mm, max_cells)
        assert e.value.status == -1 and word in str(e.value) and "pcs_background_create" in str(e.value)
    # the host forms
    host_out = np.full((n, 5), 0x5A5A, np.uint16).view(np.int16)
    cnt = C.c_int(SENTINEL)
    p = np.ascontiguousarray(rec)
    g = C.byref(good)
    for args, word in (((p.ctypes.data, n, C.byref(bad_params[0][0]), host_out.ctypes.data, shorts, C.byref(cnt), None), "min_seen"),
                       ((p.ctypes.data, -3, g, host_out.ctypes.data, shorts, C.byref(cnt), None), "n_points"),
                       ((None, n, g, host_out.ctypes.data, shorts, C.byref(cnt), None), "payload"),
                       ((p.ctypes.data, n, g, None, shorts, C.byref(cnt), None), "out"),
                       ((p.ctypes.data, n, g, host_out.ctypes.data, shorts, None, None), "out_points"),
                       ((p.ctypes.data + 1, n, g, host_out.ctypes.data, shorts, C.byref(cnt), None), "payload"),
                       ((p.ctypes.data, n, g, host_out.ctypes.data, shorts - 1, C.byref(cnt), None), "out_shorts"),
                       ((p.ctypes.data, n, g, p.ctypes.data + 20, shorts, C.byref(cnt), None), "overlap")):
        assert lib.pcs_background_subtract(h, bg.handle, *args) == -1
        text = lib.pcs_last_error(h).decode()
        assert word in text and "pcs_background_subtract:" in text, text
    assert lib.pcs_background_learn(h, bg.handle, None, n) == -1 and "pcs_background_learn: payload" in lib.pcs_last_error(h).decode()
    assert cnt.value == SENTINEL and (host_out.view(np.uint16) == 0x5A5A).all()
    ctx.synchronize()
    assert ctx.kernel_times_ms().shape[0] == 0                      # nothing was launched
    ctx.kernel_timing(False)
    out = np.empty(4 + 10 * n + GUARD, np.uint8)
    words = np.empty(2, np.int32)
    back = np.empty((n, 5), np.int16)
    block = np.empty(16, np.uint64)
    ctx.memcpy_d2h(out, arena.out)
    ctx.memcpy_d2h(words, arena.words)
    ctx.memcpy_d2h(back, d_in)
    ctx.memcpy_d2h(block, arena.stats)
    assert (out == 0xA5).all() and words[0] == SENTINEL and words[1] == n and (back == rec).all() and (block == STATS_SENTINEL).all()
    assert bg.info()["frames"] == len(case.frames) and bg.export() == blob                  # the model is what it was
    bg.close()


def test_zero_records(arena):
    """learn still advances frames; subtract writes a zero count and a zeroed block; payload and output may be NULL."""
    empty = np.zeros((0, 5), np.int16)
    ctx = arena.ctx
    with ctx.background_create(20, 64) as bg:
        arena.learn(bg, empty)
        bg.learn_device(0, 0)
        arena.learn(bg, empty, d_count=7, max_points=0)
        bg.learn(empty)
        assert bg.info() == {"cell_mm": 20, "max_cells": 64, "cells": 0, "frames": 4, "overflow": 0}
        assert bg.export() == N.learned(20, 64, [empty] * 4).export()
        got, kept, st = arena.run(bg, empty, 1, 1)
        assert kept == 0 and set(st.values()) == {0}
        got, kept, st = arena.run(bg, empty, 1, 1, d_count=7, max_points=0)
        assert kept == 0
        ctx.memcpy_h2d(arena.words, np.array([SENTINEL], np.int32))
        bg.subtract_device(0, 0, BackgroundParams.make(1, 1), 0, 0, arena.words)
        ctx.synchronize()
        w = np.empty(1, np.int32)
        ctx.memcpy_d2h(w, arena.words)
        assert w[0] == 0
        got, st = bg.subtract(empty, 1, 1)
        assert got.shape[0] == 0
        # a count of zero on the device, capacity above it: the launches run and keep nothing
        rec = K.CASES["count65"].payload
        got, kept, st = arena.run(bg, rec, 1, 1, d_count=0, max_points=65)
        assert kept == 0 and st["considered"] == 0 and st["frames"] == 4


def test_kernel_timing_counts_the_launches(arena, models):
    """One finite interval >= 0 per launch: subtract 5 with a statistics block and 4 without, learn 1, create / reset 1, export 1,
    import 2, none for zero records — and timing changes no byte."""
    ctx = arena.ctx
    case, bg = K.CASES["count2049"], models("count2049")
    is_bg = K.reference("count2049")[(3, 1)]
    plain, n_plain, _ = arena.run(bg, case.payload, 3, 1)
    ctx.kernel_timing(True)
    try:
        def launches(fn):
            out = fn()
            ctx.synchronize()
            t = ctx.kernel_times_ms()
            assert np.isfinite(t).all() and (t >= 0).all()
            return t.shape[0], out
        k, (timed, n_timed, _) = launches(lambda: arena.run(bg, case.payload, 3, 1))
        assert k == 5 and n_timed == n_plain and timed.tobytes() == plain.tobytes() and (timed == case.payload[~is_bg]).all()
        assert launches(lambda: arena.run(bg, case.payload, 3, 1, stats=False))[0] == 4
        assert launches(lambda: arena.run(bg, case.payload, 3, 1, d_count=100, max_points=2049))[0] == 5
        assert launches(lambda: arena.run(bg, case.payload[:0], 3, 1))[0] == 0
        k, fresh = launches(lambda: ctx.background_create(case.cell_mm, case.max_cells))
        assert k == 1
        assert launches(lambda: arena.learn(fresh, case.frames[0]))[0] == 1
        assert launches(lambda: arena.learn(fresh, case.frames[0][:0]))[0] == 0
        assert launches(fresh.reset)[0] == 1
        fresh.close()
        k, blob = launches(bg.export)
        assert k == 1 and blob == K.model_of("count2049").export()
        k, twin = launches(lambda: ctx.background_import(blob, case.max_cells))
        assert k == 2
        twin.close()
    finally:
        ctx.kernel_timing(False)


def test_destroying_the_context_frees_its_models():
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs) as c:
        left = [c.background_create(20, 1 << 16) for _ in range(3)]
        left[1].close()
        left[0].learn(K.CASES["count65"].payload)
    # closing a model after its context is a no-op on the Python side
    left[0].close()
