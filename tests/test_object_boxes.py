"""Object boxes on the GPU (pcs_object_boxes*), against the restatement of DESIGN.md section 3 (tests/np_object_boxes.py: Python
integers and numpy's eigh) over the cases of tests/object_box_cases.py. The sums and the rank byte for byte; the extents byte for
byte against the restatement fed the GPU's own axis shorts; the axes within 1 short of rint(16384 e) after aligning signs (the
derivation of that 1 and of the invariants' bound of about 28 400: tests/test_object_boxes_cpu.py); every member's projection inside
[ext_lo, ext_hi] with both ends attained. Both 2-byte payload phases, 0xA5 guards around the entries, the counted and host forms,
two runs, a shuffled record order, an object table fed straight in with no host round trip, a small call in a large call's
workspace, one timing interval per launch, every refusal."""
import ctypes as C

import numpy as np
import pytest

import np_object_boxes as NB
import object_box_cases as K
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import (CLUSTER_OBJECT_DTYPE, ClusterObjectsOut, ClusterParams, OBJECT_BOX_DTYPE, OBJECT_BOXES_LAUNCHES,
                                            ObjectBox)

pytestmark = pytest.mark.gpu

GUARD = 64
N_MAX = 131072
M_MAX = 64
NAMES = sorted(K.CASES)


class Arena:
    """Device buffers shared by the tests of this module: a payload at any 2-byte phase, object_of, the count words, guarded boxes."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.inp = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.obj = ctx.device_malloc(4 * N_MAX + 64)
        self.words = ctx.device_malloc(64)          # [0] n_objects, [4] the counted form's record count
        self.boxes = ctx.device_malloc(GUARD + 128 * M_MAX + GUARD)
        assert self.inp % 16 == 0 and self.boxes % 8 == 0

    def free(self):
        for p in (self.inp, self.obj, self.words, self.boxes):
            self.ctx.device_free(p)

    def run(self, case, in_phase=4, d_count=None, max_points=None, extra=None):
        """One call on the device forms -> entries[m]. extra: (records, object_of) behind the count of the counted form. Everything
        around boxes[0..m) must stay 0xA5 and the count words what they were."""
        ctx = self.ctx
        rec, obj = (case.rec, case.object_of) if extra is None else (np.concatenate([case.rec, extra[0]]), np.concatenate([case.object_of, extra[1]]))
        n, M = rec.shape[0], case.max_objects
        assert n <= N_MAX and M <= M_MAX
        d_in = self.inp + in_phase
        if n:
            ctx.memcpy_h2d(d_in, np.ascontiguousarray(rec))
            ctx.memcpy_h2d(self.obj, np.ascontiguousarray(obj))
        span = GUARD + 128 * M + GUARD
        ctx.memcpy_h2d(self.boxes, np.full(span, 0xA5, np.uint8))
        ctx.memcpy_h2d(self.words, np.array([case.n_objects, 0 if d_count is None else d_count], np.int32))
        d_boxes = self.boxes + GUARD if M else 0
        if d_count is None:
            ctx.object_boxes_device(d_in, n, self.obj, self.words, M, d_boxes)
        else:
            ctx.object_boxes_device_counted(d_in, self.words + 4, max_points, self.obj, self.words, M, d_boxes)
        ctx.synchronize()
        got = np.empty(span, np.uint8)
        ctx.memcpy_d2h(got, self.boxes)
        words = np.empty(2, np.int32)
        ctx.memcpy_d2h(words, self.words)
        assert words[0] == case.n_objects and words[1] == (0 if d_count is None else d_count)
        m = min(max(case.n_objects, 0), M)
        assert (got[:GUARD] == 0xA5).all(), "bytes in front of d_boxes were written"
        assert (got[GUARD + 128 * m:] == 0xA5).all(), "bytes at or behind entry m were written"
        return got[GUARD:GUARD + 128 * m].copy().view(OBJECT_BOX_DTYPE)


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


_GOT = {}


def gpu_entries(arena, name):
    """The plain device form's entries of a case — computed once, shared, never changed."""
    if name not in _GOT:
        _GOT[name] = arena.run(K.CASES[name])
        _GOT[name].flags.writeable = False
    return _GOT[name]


def check(name, got, case=None):
    case = K.CASES[name] if case is None else case
    compared = NB.compare(got, case.rec, case.object_of, case.n_objects, case.max_objects, where=name, axes=case.axes)
    NB.check_members(got, case.rec, case.object_of, case.n_objects, case.max_objects, where=name)
    return compared


def test_the_bindings_and_the_restatement_agree_on_the_layout():
    assert OBJECT_BOX_DTYPE == NB.OBJECT_BOX_DTYPE and C.sizeof(ObjectBox) == 128 and len(OBJECT_BOXES_LAUNCHES) == 4


@pytest.mark.parametrize("name", NAMES)
def test_every_case_against_the_restatement(arena, name):
    got = gpu_entries(arena, name)
    compared = check(name, got)
    if K.CASES[name].axes:
        assert compared == 3 * int((got["count"] > 0).sum()), (name, compared)       # no axis was left out
    print(f"{name}: {got.shape[0]} entries, {compared} axes compared")


def test_the_corner_and_the_degenerate_shapes(arena):
    eye = (16384 * np.eye(3, dtype=np.int64)).tolist()
    for name, rank in (("one_record", 0), ("corner_2", 0), ("corner_5", 0), ("point_x50", 0), ("line", 1), ("grid_plane", 2), ("cube", 3)):
        got = gpu_entries(arena, name)
        assert got.shape[0] == 1 and int(got[0]["rank"]) == rank, (name, got[0]["rank"])
        if rank == 0:
            assert got[0]["axis"].tolist() == eye, name
    g = gpu_entries(arena, "corner_2")[0]
    assert g["count"] == 2 and g["m2"].tolist()[:2] == [2 ** 31, 2 ** 31] and g["m2"].tolist()[2] == -2 * 32768 * 32767
    assert g["ext_lo"].tolist() == g["ext_hi"].tolist() == [-32768 * 16384, -32768 * 16384, 32767 * 16384]
    g = gpu_entries(arena, "corner_5")[0]
    assert g["m2"].tolist() == [5 * 2 ** 30, 5 * 2 ** 30, -5 * 32768 * 32767, 5 * 2 ** 30, -5 * 32768 * 32767, 5 * 32767 ** 2]


def test_an_axis_aligned_lattice_and_an_entry_without_a_member(arena):
    c = K.CASES["aligned"]
    got = gpu_entries(arena, "aligned")[0]
    assert got["axis"].tolist() == (16384 * np.eye(3, dtype=np.int64)).tolist() and got["rank"] == 3
    xyz = c.rec[:, :3].astype(np.int64)
    # 16384 x the object table's lo / hi
    assert got["ext_lo"].tolist() == (16384 * xyz.min(axis=0)).tolist() and got["ext_hi"].tolist() == (16384 * xyz.max(axis=0)).tolist()
    got = gpu_entries(arena, "ignored")
    empty = NB.boxes_np(np.zeros((0, 5), np.int16), [], 1, 1)[0][0]
    assert got.shape[0] == 4 and got[2].tobytes() == empty.tobytes() and (got["count"][[0, 1, 3]] > 0).all()
    assert empty["axis"].tolist() == (16384 * np.eye(3, dtype=np.int64)).tolist() and not empty["ext_lo"].any() and not empty["ext_hi"].any()
    for name in ("no_records",):
        got = gpu_entries(arena, name)
        assert got.shape[0] == 3 and all(e.tobytes() == empty.tobytes() for e in got)


def test_lattices_of_131072_against_their_own_arithmetic(arena):
    """The object table's lattice (64 x 64 x 32 at pitch 1 against the x = 32767 and y = -32768 faces), and 512 x 256 records on
    the face x = -32768 itself: sum xx = 2^17 * 2^30 = 2^47 exactly, every sum from closed forms."""
    def squares(a, b):                                          # sum of v^2 for v in a..b
        f = lambda t: t * (t + 1) * (2 * t + 1) // 6
        assert 0 <= a <= b
        return f(b) - f(a - 1)
    order = np.random.default_rng(31).permutation(N_MAX)
    g = (np.indices((64, 64, 32)).reshape(3, -1).T + np.array([32704, -32768, -16]))[order]
    got = arena.run(K.one(g, axes=False))
    assert got.shape[0] == 1
    e = got[0]
    assert e["count"] == N_MAX and e["sum_xyz"].tolist() == [N_MAX * (32704 + 32767) // 2, -N_MAX * (32768 + 32705) // 2, -N_MAX // 2]
    sxx, syy, szz = 2048 * squares(32704, 32767), 2048 * squares(32705, 32768), 4096 * (squares(0, 15) + squares(1, 16))
    sx, sy, sz = (int(v) for v in e["sum_xyz"])
    # the lattice is a product: sum ab = (sum a)(sum b) / n
    assert e["m2"].tolist() == [sxx, sx * sy // N_MAX, sx * sz // N_MAX, syy, sy * sz // N_MAX, szz]
    assert sxx > 2 ** 46 and e["rank"] == 3
    NB.check_invariants(got, "lattice")
    NB.check_members(got, K.with_colour(g), np.zeros(N_MAX, np.int32), 1, 4, "lattice")
    f = (np.indices((1, 512, 256)).reshape(3, -1).T + np.array([-32768, -256, 1000]))[order]
    got = arena.run(K.one(f, axes=False))
    e = got[0]
    assert e["count"] == N_MAX and e["m2"][0] == 2 ** 47 and e["sum_xyz"][0] == -2 ** 32 and e["rank"] == 2
    assert e["m2"].tolist() == [2 ** 47, -32768 * int(e["sum_xyz"][1]), -32768 * int(e["sum_xyz"][2]), 256 * (squares(0, 255) + squares(1, 256)),
                                int(e["sum_xyz"][1]) * int(e["sum_xyz"][2]) // N_MAX, 512 * squares(1000, 1255)]
    NB.check_invariants(got, "face")
    NB.check_members(got, K.with_colour(f), np.zeros(N_MAX, np.int32), 1, 4, "face")


def test_both_payload_phases_and_two_runs(arena):
    for name in ("rotated", "dominant", "count_2049", "ignored", "pairs_33"):
        want = gpu_entries(arena, name).tobytes()
        for phase in (0, 2, 4, 6):
            assert arena.run(K.CASES[name], in_phase=phase).tobytes() == want, (name, phase)


def test_a_shuffled_record_order_changes_no_byte(arena):
    for name in ("rotated", "dominant", "ignored", "alternating"):
        c = K.CASES[name]
        order = np.random.default_rng(12).permutation(c.rec.shape[0])
        again = arena.run(K.Case(c.rec[order], c.object_of[order], c.n_objects, c.max_objects, c.axes))
        assert again.tobytes() == gpu_entries(arena, name).tobytes(), name


def test_counted_form(arena):
    """Members behind the count are never read; counts of 0, negative and above max_points."""
    c = K.CASES["rotated"]
    n = c.rec.shape[0]
    want = gpu_entries(arena, "rotated").tobytes()
    behind = (K.with_colour(K.blob(500, 77, (-15000, -15000, -15000))), np.arange(500, dtype=np.int32) % 9)
    assert arena.run(c, d_count=n, max_points=n + 500, extra=behind).tobytes() == want
    assert arena.run(c, d_count=n + 12345, max_points=n).tobytes() == want                # clamped to max_points
    assert arena.run(c, d_count=2 ** 31 - 1, max_points=n).tobytes() == want
    head = K.Case(c.rec[:3000], c.object_of[:3000], c.n_objects, c.max_objects, c.axes)
    got = arena.run(c, d_count=3000, max_points=n)
    assert got.tobytes() == arena.run(head).tobytes()
    check("rotated[:3000]", got, head)
    empty = NB.boxes_np(np.zeros((0, 5), np.int16), [], 1, 1)[0][0].tobytes()
    for count, cap in ((0, n), (-1, n), (-2 ** 31, n), (n, 0)):
        got = arena.run(c, d_count=count, max_points=cap)
        assert got.shape[0] == 9 and all(e.tobytes() == empty for e in got), (count, cap)


def test_host_form(arena):
    for name in ("rotated", "dominant", "ignored", "corner_5", "no_records", "none_found", "negative_count", "no_table"):
        c = K.CASES[name]
        got = arena.ctx.object_boxes(c.rec, c.object_of, c.n_objects, c.max_objects)
        assert got.dtype == OBJECT_BOX_DTYPE and got.tobytes() == gpu_entries(arena, name).tobytes(), name


def test_fed_from_the_object_table(arena):
    """pcs_cluster_objects_device_counted -> pcs_object_boxes_device_counted with no host round trip in between: count == size and
    sum_xyz == the object table's, and the entries are the restatement's for the table's object_of."""
    ctx = arena.ctx
    c = K.CASES["rotated"]
    rec = np.ascontiguousarray(c.rec)
    n, M = rec.shape[0], 16
    d_table = ctx.device_malloc(80 * M)
    try:
        ctx.memcpy_h2d(arena.inp, rec)
        ctx.memcpy_h2d(arena.words, np.array([-1, n, -1], np.int32))
        ctx.memcpy_h2d(arena.boxes, np.full(GUARD + 128 * M + GUARD, 0xA5, np.uint8))
        ctx.cluster_objects_device_counted(arena.inp, arena.words + 4, n, ClusterParams.make(30, 50, 0),
                                           ClusterObjectsOut.make(objects=d_table, max_objects=M, n_objects=arena.words, object_of=arena.obj))
        ctx.object_boxes_device_counted(arena.inp, arena.words + 4, n, arena.obj, arena.words, M, arena.boxes + GUARD)
        ctx.synchronize()
        words = np.empty(3, np.int32)
        ctx.memcpy_d2h(words, arena.words)
        table = np.empty(M, CLUSTER_OBJECT_DTYPE)
        ctx.memcpy_d2h(table, d_table)
        object_of = np.empty(n, np.int32)
        ctx.memcpy_d2h(object_of, arena.obj)
        got = np.empty(GUARD + 128 * M + GUARD, np.uint8)
        ctx.memcpy_d2h(got, arena.boxes)
    finally:
        ctx.device_free(d_table)
    m = int(words[0])
    assert m == 9 and words[1] == n                             # the nine lattices, 20 mm pitch under a 30 mm tolerance
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + 128 * m:] == 0xA5).all()
    boxes = got[GUARD:GUARD + 128 * m].copy().view(OBJECT_BOX_DTYPE)
    assert boxes["count"].tolist() == table["size"][:m].tolist() and boxes["sum_xyz"].tolist() == table["sum_xyz"][:m].tolist()
    fed = K.Case(rec, object_of, m, M, True)
    assert check("fed", boxes, fed) == 27
    # 16384 x the table's box contains the extents' box corners only for an aligned object; what always holds: the centroid's
    # projection lies inside the extents
    for k in range(m):
        centre = boxes[k]["sum_xyz"].astype(np.float64) / float(boxes[k]["count"])
        proj = boxes[k]["axis"].astype(np.float64) @ centre
        assert (proj >= boxes[k]["ext_lo"] - 1).all() and (proj <= boxes[k]["ext_hi"] + 1).all()


def test_a_small_call_in_a_large_calls_workspace(arena):
    ctx = arena.ctx
    c = K.CASES["pairs_33"]
    big = K.Case(c.rec, c.object_of, 33, M_MAX, False)
    assert arena.run(big).tobytes() == gpu_entries(arena, "pairs_33").tobytes()
    for name in ("ignored", "corner_2", "rotated"):
        assert arena.run(K.CASES[name]).tobytes() == gpu_entries(arena, name).tobytes(), name
    # the largest table there is, then a small one again: the slab grew in between
    d_big = ctx.device_malloc(128 * 65536)
    try:
        ctx.memcpy_h2d(arena.inp, np.ascontiguousarray(c.rec))
        ctx.memcpy_h2d(arena.obj, np.ascontiguousarray(c.object_of))
        ctx.memcpy_h2d(arena.words, np.array([33, 0], np.int32))
        ctx.object_boxes_device(arena.inp, c.rec.shape[0], arena.obj, arena.words, 65536, d_big)
        ctx.synchronize()
        got = np.empty(33, OBJECT_BOX_DTYPE)
        ctx.memcpy_d2h(got, d_big)
    finally:
        ctx.device_free(d_big)
    assert got.tobytes() == gpu_entries(arena, "pairs_33").tobytes()
    assert arena.run(K.CASES["dominant"]).tobytes() == gpu_entries(arena, "dominant").tobytes()


def test_kernel_timing_counts_the_launches(arena):
    """One finite interval >= 0 per launch: every call 4 in all three forms, whatever the counts — and timing changes no byte."""
    ctx = arena.ctx
    want = gpu_entries(arena, "dominant").tobytes()
    c = K.CASES["dominant"]
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
        assert k == len(OBJECT_BOXES_LAUNCHES) == 4 and got.tobytes() == want
        assert launches(lambda: arena.run(c, d_count=100, max_points=c.rec.shape[0]))[0] == 4
        assert launches(lambda: arena.run(K.CASES["no_records"]))[0] == 4
        assert launches(lambda: arena.run(K.CASES["no_table"]))[0] == 4
        assert launches(lambda: arena.run(K.CASES["none_found"], d_count=5, max_points=0))[0] == 4
        k, got = launches(lambda: ctx.object_boxes(c.rec, c.object_of, c.n_objects, c.max_objects))
        assert k == 4 and got.tobytes() == want
    finally:
        ctx.kernel_timing(False)


def test_refusals_launch_nothing_and_write_nothing(arena):
    ctx = arena.ctx
    c = K.CASES["ignored"]
    n, M = c.rec.shape[0], c.max_objects
    arena.run(c)
    d_in, d_obj, d_m, d_n, d_bx = arena.inp + 4, arena.obj, arena.words, arena.words + 4, arena.boxes + GUARD
    ctx.memcpy_h2d(arena.boxes, np.full(GUARD + 128 * M + GUARD, 0xA5, np.uint8))
    ctx.memcpy_h2d(arena.words, np.array([c.n_objects, n], np.int32))
    ctx.synchronize()
    ctx.kernel_times_ms()
    ctx.kernel_timing(True)
    too_many = (2 ** 31 - 1) // 10 + 1
    plain = [
        ((d_in, -1, d_obj, d_m, M, d_bx), "n_points"),
        ((d_in, too_many, d_obj, d_m, M, d_bx), "n_points"),
        ((0, n, d_obj, d_m, M, d_bx), "d_payload"),
        ((d_in + 1, n, d_obj, d_m, M, d_bx), "d_payload"),
        ((d_in, n, 0, d_m, M, d_bx), "d_object_of"),
        ((d_in, n, d_obj + 2, d_m, M, d_bx), "d_object_of"),
        ((d_in, n, d_obj, 0, M, d_bx), "d_n_objects"),
        ((d_in, n, d_obj, d_m + 2, M, d_bx), "d_n_objects"),
        ((d_in, n, d_obj, d_m, -1, d_bx), "max_objects"),
        ((d_in, n, d_obj, d_m, 65537, d_bx), "max_objects"),
        ((d_in, n, d_obj, d_m, M, 0), "d_boxes"),
        ((d_in, n, d_obj, d_m, M, d_bx + 4), "d_boxes"),
        ((d_in, n, d_obj, d_m, M, d_in + 4), "overlap"),
        ((d_in, n, d_obj, d_m, M, d_obj + 8), "overlap"),
        ((d_in, n, d_obj, d_bx + 8, M, d_bx), "overlap"),
        ((d_in, n, d_obj, d_m, M, d_m - 8), "overlap"),
    ]
    for args, word in plain:
        with pytest.raises(PcsError) as e:
            ctx.object_boxes_device(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_object_boxes_device:" in str(e.value), (word, str(e.value))
    counted = [
        ((d_in, 0, n, d_obj, d_m, M, d_bx), "d_n_points"),
        ((d_in, d_n + 2, n, d_obj, d_m, M, d_bx), "d_n_points"),
        ((d_in, d_n, -1, d_obj, d_m, M, d_bx), "max_points"),
        ((d_in, d_n, too_many, d_obj, d_m, M, d_bx), "max_points"),
        ((0, d_n, n, d_obj, d_m, M, d_bx), "d_payload"),
        ((d_in, d_n, n, 0, d_m, M, d_bx), "d_object_of"),
        ((d_in, d_n, n, d_obj, 0, M, d_bx), "d_n_objects"),
        ((d_in, d_n, n, d_obj, d_m, 65537, d_bx), "max_objects"),
        ((d_in, d_n, n, d_obj, d_m, M, d_bx + 2), "d_boxes"),
        ((d_in, d_bx + 8, n, d_obj, d_m, M, d_bx), "overlap"),
        ((d_in, d_n, n, d_obj, d_m, M, d_m), "overlap"),
    ]
    for args, word in counted:
        with pytest.raises(PcsError) as e:
            ctx.object_boxes_device_counted(*args)
        assert e.value.status == -1 and word in str(e.value) and "pcs_object_boxes_device_counted:" in str(e.value), (word, str(e.value))
    # the host form
    lib, h = ctx._lib, ctx._h
    p, o = np.ascontiguousarray(c.rec), np.ascontiguousarray(c.object_of)
    host_boxes = np.full(128 * M, 0x5A, np.uint8)
    hb = host_boxes.ctypes.data_as(C.POINTER(ObjectBox))
    for args, word in (((p.ctypes.data, -3, o.ctypes.data, c.n_objects, M, hb), "n_points"),
                       ((None, n, o.ctypes.data, c.n_objects, M, hb), "payload"),
                       ((p.ctypes.data + 1, n, o.ctypes.data, c.n_objects, M, hb), "payload"),
                       ((p.ctypes.data, n, None, c.n_objects, M, hb), "object_of"),
                       ((p.ctypes.data, n, o.ctypes.data, c.n_objects, 65537, hb), "max_objects"),
                       ((p.ctypes.data, n, o.ctypes.data, c.n_objects, -1, hb), "max_objects"),
                       ((p.ctypes.data, n, o.ctypes.data, c.n_objects, M, None), "boxes"),
                       ((p.ctypes.data, n, o.ctypes.data, c.n_objects, M, C.cast(host_boxes.ctypes.data + 4, C.POINTER(ObjectBox))), "boxes"),
                       ((p.ctypes.data, n, o.ctypes.data, c.n_objects, M, C.cast(p.ctypes.data + 16, C.POINTER(ObjectBox))), "overlap")):
        assert lib.pcs_object_boxes(h, *args) == -1
        text = lib.pcs_last_error(h).decode()
        assert word in text and "pcs_object_boxes:" in text, text
    assert (host_boxes == 0x5A).all()
    ctx.synchronize()
    assert ctx.kernel_times_ms().shape[0] == 0                      # nothing was launched
    ctx.kernel_timing(False)
    out = np.empty(GUARD + 128 * M + GUARD, np.uint8)
    words = np.empty(2, np.int32)
    ctx.memcpy_d2h(out, arena.boxes)
    ctx.memcpy_d2h(words, arena.words)
    assert (out == 0xA5).all() and words.tolist() == [c.n_objects, n]
    assert arena.run(c).tobytes() == gpu_entries(arena, "ignored").tobytes()      # ... and the next call is what it was
