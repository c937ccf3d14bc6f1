"""Object boxes without a GPU: the kernels' own arithmetic (csrc/pcs_boxes_math.h, compiled for the host by tools/boxes_host.cpp
behind a plain loop) against the restatement (tests/np_object_boxes.py: Python integers, numpy's eigh) over every case of
tests/object_box_cases.py; the restatement's own pieces against plain Python; the bindings' layout.

The comparison (np_object_boxes.compare): count, sum_xyz, m2 and rank equal; the extents equal to the restatement's when both are
given the host build's shorts; every axis within 1 short of rint(16384 e) after aligning signs — Jacobi and eigh agree to about
1e-16 lambda_max / gap in a vector, 16384 times that is far below the 0.5 of the rounding, so two correctly computed shorts differ
by at most one — except an axis whose eigenvalue lies within 1e-3 lambda_max of a neighbour's, and fewer than 1 % of a case's objects
may be left out so (none is, in the cases that compare axes).

The invariants hold for every entry, degenerate or not. Each component of a written axis is within h = 0.5 + 1e-9 of 16384 times a
unit vector's, so with s = 16384 u and an error vector e, |e_c| <= h:
    | |axis|^2 - 2^28 |  = | 2 s.e + e.e |                <= 2 * 16384 * sqrt(3) * h + 3 h^2 = 28 378.7
    | axis_a . axis_b |  = | s_a.e_b + s_b.e_a + e_a.e_b | <= the same
np_object_boxes.INVARIANT_BOUND is that figure plus one: about 28 400."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_object_boxes as NB
import object_box_cases as K
from pointcloud_stitching_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("boxes_host") / "libboxes_host.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
           os.path.join(ROOT, "pointcloud_stitching_amd", "csrc"), os.path.join(ROOT, "tools", "boxes_host.cpp"), "-o", so]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    lib = C.CDLL(so)
    lib.boxes_host.restype = C.c_int
    lib.boxes_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]

    def run(case):
        rec, obj = np.ascontiguousarray(case.rec), np.ascontiguousarray(case.object_of)
        out = np.full(max(case.max_objects, 1), 0, NB.OBJECT_BOX_DTYPE)
        m = lib.boxes_host(rec.ctypes.data, rec.shape[0], obj.ctypes.data, case.n_objects, case.max_objects, out.ctypes.data)
        assert m == min(max(case.n_objects, 0), case.max_objects)
        return out[:m].copy()
    return run


def test_the_layout_of_the_bindings_and_of_the_restatement():
    assert T.OBJECT_BOX_DTYPE == NB.OBJECT_BOX_DTYPE and C.sizeof(T.ObjectBox) == 128
    assert T.OBJECT_BOXES_LAUNCHES == ("clear", "moments", "axes", "extents")
    assert 28378 < NB.INVARIANT_BOUND < 28400
    flat = [name for name, _ in T.ObjectBox._fields_]
    assert flat == list(NB.OBJECT_BOX_DTYPE.names)
    assert sum(int(np.prod(NB.OBJECT_BOX_DTYPE[name].shape, dtype=np.int64)) for name in flat) == 27       # the integers of an entry


def test_the_restatement_against_plain_python():
    rng = np.random.default_rng(2)
    xyz = rng.integers(-32768, 32768, (50, 3))
    xyz[:3] = K.CORNER
    count, s1, m2 = NB.sums_np(xyz)
    q = xyz.tolist()
    assert count == 50 and s1.tolist() == [sum(p[a] for p in q) for a in range(3)]
    assert m2.tolist() == [sum(p[a] * p[b] for p in q) for a, b in NB.PAIRS]
    c = NB.covariance_int(count, s1, m2)
    # count^2 times the covariance, from the definition in exact rationals
    for a in range(3):
        for b in range(3):
            assert c[a][b] == sum((count * p[a] - int(s1[a])) * (count * p[b] - int(s1[b])) for p in q) // count
    two = NB.sums_np([K.CORNER] * 2)
    assert two[2].tolist() == [2 ** 31, 2 ** 31, -2 * 32768 * 32767, 2 ** 31, -2 * 32768 * 32767, 2 * 32767 ** 2]
    assert NB.sign_rule(np.array([-3.0, 1.0, 3.0])).tolist() == [-3.0, 1.0, 3.0]        # z wins the tie
    assert NB.sign_rule(np.array([3.0, -3.0, 1.0])).tolist() == [-3.0, 3.0, -1.0]       # y before x
    assert NB.sign_rule(np.array([-3.0, 1.0, 1.0])).tolist() == [3.0, -1.0, -1.0]
    lo, hi = NB.extents_int([[1, 2, 3], [-4, 5, 6]], [[16384, 0, 0], [0, -16384, 0], [1, 1, 1]])
    assert lo.tolist() == [-65536, -81920, 6] and hi.tolist() == [16384, -32768, 7]


def test_the_cases_are_what_they_say():
    assert len(K.AXES_CASES) >= 10
    c = K.CASES["dominant"]
    assert c.rec.shape[0] == 9200 and np.bincount(c.object_of).tolist()[0] == 9000 and (np.bincount(c.object_of)[1:] > 0).all()
    assert np.bincount(c.object_of)[1:].sum() == 200
    c = K.CASES["rotated"]
    assert np.bincount(c.object_of).tolist() == [1386] * 3 + [2944] * 3 + [105] * 3
    c = K.CASES["ignored"]
    assert (c.object_of == 2).sum() == 0 and (c.object_of == -1).any() and (c.object_of == 4).any() and (c.object_of > 4).any()
    # no object of a case that compares axes is near an eigenvalue crossing: relative gaps of 0.1 and more
    for name in K.AXES_CASES:
        c = K.CASES[name]
        m, idx = NB.members(c.object_of, c.n_objects, c.max_objects)
        for k in range(m):
            if idx[k].shape[0] == 0:
                continue
            _, w, rank, sure = NB.axes_np(*NB.sums_np(c.rec[idx[k], :3]))
            assert rank == 3 and sure.all() and min(w[0] - w[1], w[1] - w[2]) > 0.05 * w[0], (name, k, w)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_the_kernel_arithmetic_on_the_host_matches_the_restatement(host, name):
    case = K.CASES[name]
    got = host(case)
    compared = NB.compare(got, case.rec, case.object_of, case.n_objects, case.max_objects, where=name, axes=case.axes)
    NB.check_members(got, case.rec, case.object_of, case.n_objects, case.max_objects, where=name)
    worst = 0.0
    if case.axes:
        want, _ = NB.boxes_np(case.rec, case.object_of, case.n_objects, case.max_objects)
        assert compared == 3 * int((want["count"] > 0).sum()), (name, compared)     # nothing was left out
        m, idx = NB.members(case.object_of, case.n_objects, case.max_objects)
        for k in range(m):
            if idx[k].shape[0] == 0:
                continue
            axes, _, _, _ = NB.axes_np(*NB.sums_np(case.rec[idx[k], :3]))
            for a in range(3):
                g = got[k]["axis"][a].astype(np.float64)
                e = axes[a] if g @ axes[a] >= 0 else -axes[a]
                worst = max(worst, float(np.abs(16384.0 * e - g).max()))
        assert worst <= 0.5 + 1e-6, (name, worst)
    print(f"{name}: {got.shape[0]} entries, {compared} axes compared, worst |16384 e - axis| {worst:.3f}")


def test_the_degenerate_shapes(host):
    eye = (16384 * np.eye(3, dtype=np.int64)).tolist()
    for name, rank in (("one_record", 0), ("corner_2", 0), ("corner_5", 0), ("point_x50", 0), ("line", 1), ("grid_plane", 2), ("cube", 3)):
        got = host(K.CASES[name])
        assert got.shape[0] == 1 and int(got[0]["rank"]) == rank, (name, got[0]["rank"])
        if rank == 0:
            assert got[0]["axis"].tolist() == eye, name
    g = host(K.CASES["corner_2"])[0]
    assert g["m2"].tolist()[:2] == [2 ** 31, 2 ** 31] and g["ext_lo"].tolist() == g["ext_hi"].tolist() == [-32768 * 16384, -32768 * 16384, 32767 * 16384]
    line = host(K.CASES["line"])[0]
    d = np.array([10, 20, -30]) / np.sqrt(1400.0)
    assert np.abs(np.abs(line["axis"][0] @ d) / 16384.0 - 1.0) < 1e-4              # the one axis that means something
    plane = host(K.CASES["grid_plane"])[0]
    assert abs(int(plane["axis"][2][2])) == 16384 and plane["ext_lo"][2] == plane["ext_hi"][2]


def test_an_axis_aligned_lattice_and_an_entry_without_a_member(host):
    c = K.CASES["aligned"]
    got = host(c)[0]
    assert got["axis"].tolist() == (16384 * np.eye(3, dtype=np.int64)).tolist() and got["rank"] == 3
    xyz = c.rec[:, :3].astype(np.int64)
    assert got["ext_lo"].tolist() == (16384 * xyz.min(axis=0)).tolist() and got["ext_hi"].tolist() == (16384 * xyz.max(axis=0)).tolist()
    got = host(K.CASES["ignored"])
    assert got.shape[0] == 4 and got[2].tobytes() == NB.boxes_np(np.zeros((0, 5), np.int16), [], 1, 1)[0][0].tobytes()
    empty = got[2]
    assert empty["count"] == 0 and not empty["sum_xyz"].any() and not empty["m2"].any() and empty["rank"] == 0
    assert empty["axis"].tolist() == (16384 * np.eye(3, dtype=np.int64)).tolist() and not empty["ext_lo"].any() and not empty["ext_hi"].any()


def test_a_permutation_of_the_records_changes_no_byte(host):
    for name in ("rotated", "dominant", "ignored"):
        c = K.CASES[name]
        order = np.random.default_rng(12).permutation(c.rec.shape[0])
        again = host(K.Case(c.rec[order], c.object_of[order], c.n_objects, c.max_objects, c.axes))
        assert again.tobytes() == host(c).tobytes(), name
