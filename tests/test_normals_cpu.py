"""Surface normals without a GPU: the restatement (tests/np_normals.py) against a plain double loop, and the kernel's own arithmetic
(csrc/pcs_normals_math.h, compiled for the host by tools/normals_host.cpp over a brute-force neighbour search) against the
restatement over every case of tests/plane_cases.py — validity equal, every short within one unit, the sign rules, and under 1 % of a
case's records too close to a threshold or an eigenvalue crossing to compare."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import np_normals as NN
import plane_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c[0]: c for c in PC.normal_cases()}


@functools.lru_cache(maxsize=None)
def reference(name, viewpoint=None):
    _, payload, (radius, min_nb, flat) = CASES[name]
    return NN.normals_np(payload, radius, min_nb, flat, viewpoint)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("normals_host") / "libnormals_host.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
           os.path.join(ROOT, "pointcloud_stitching_amd", "csrc"), os.path.join(ROOT, "tools", "normals_host.cpp"), "-o", so]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    lib = C.CDLL(so)
    lib.normals_host.restype = C.c_int
    lib.normals_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def run(payload, radius, min_nb, flat, viewpoint=None):
        p = np.ascontiguousarray(payload, np.int16)
        out = np.empty((p.shape[0], 4), np.int16)
        vp = np.asarray(viewpoint if viewpoint is not None else (0, 0, 0), np.int32)
        valid = lib.normals_host(p.ctypes.data, p.shape[0], radius, min_nb, flat, int(viewpoint is not None), vp.ctypes.data, out.ctypes.data)
        assert valid == int((out[:, 3] != 0).sum())
        return out
    return run


def test_the_neighbour_sums_against_a_plain_double_loop():
    rng = np.random.default_rng(1)
    for n, side, radius in ((1, 10, 5), (40, 30, 9), (120, 60, 25), (60, 65536, 1000)):
        lo = -(side // 2)
        pts = rng.integers(lo, lo + side, (n, 3))
        pts[n // 2:n // 2 + 3] = pts[0]                      # equal records are each other's neighbours
        payload = PC.with_colour(pts, n)
        m, S1, S2 = NN.neighbour_sums_np(payload, radius)
        q = pts.tolist()
        for i in range(n):
            mm, s1, s2 = 0, [0] * 3, [0] * 6
            for j in range(n):
                d = [q[j][a] - q[i][a] for a in range(3)]
                if sum(v * v for v in d) > radius * radius:
                    continue
                mm += 1
                s1 = [s + v for s, v in zip(s1, d)]
                s2 = [s + d[a] * d[b] for s, (a, b) in zip(s2, ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))]
            assert (mm, s1, s2) == (int(m[i]), S1[i].tolist(), S2[i].tolist()), (n, i)
            assert mm >= 1
        C3 = NN.covariance_np(m, S1, S2)
        for i in range(n):
            for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                assert C3[i, a, b] == C3[i, b, a] == int(m[i]) * int(S2[i][k]) - int(S1[i][a]) * int(S1[i][b])


@pytest.mark.parametrize("name", list(CASES))
def test_the_kernel_arithmetic_on_the_host_matches_the_restatement(host, name):
    _, payload, (radius, min_nb, flat) = CASES[name]
    ref = reference(name)
    got = host(payload, radius, min_nb, flat)
    compared = NN.compare(got, ref, name)
    print(f"{name}: n {payload.shape[0]}, valid {int(ref.valid.sum())}, unsure {int(ref.unsure.sum())}, compared {compared}")


def test_the_cases_cover_what_they_are_for():
    for name in ("line", "one_point_50", "identical_4096", "size1", "size2"):
        assert not reference(name).valid.any() and not reference(name).unsure.any(), name
    for name in ("size63", "size257", "size2049", "size6161", "scene"):
        v = reference(name).valid
        assert v.any() and not v.all(), name                      # valid and invalid records
    gated, open_ = reference("scene"), reference("scene_no_gate")
    assert gated.valid.sum() < open_.valid.sum() and not (gated.valid & ~open_.valid).any()
    for axis, name in enumerate(("grid_x", "grid_y", "grid_z")):
        ref = reference(name)
        want = [0, 0, 0]
        want[axis] = 16384
        assert ref.valid.all() and (ref.shorts[:, :3] == want).all(), name
    assert (reference("int16_high_end").shorts[:, :3] == [0, 0, 16384]).all()
    assert (reference("int16_low_end").shorts[:, :3] == [16384, 0, 0]).all()
    assert reference("identical_4096").m.min() == 4096 and reference("size6161").m.max() < 32767


def test_the_sign_rules_on_the_host(host):
    _, payload, (radius, min_nb, flat) = CASES["scene"]
    q = payload[:, :3].astype(np.int64)
    got = host(payload, radius, min_nb, flat, PC.SCENE_CENTRE)
    ok = got[:, 3] != 0
    assert ok.sum() > 1000
    towards = (got[ok, :3].astype(np.int64) * (np.asarray(PC.SCENE_CENTRE) - q[ok])).sum(axis=1)
    assert (towards > 0).all()
    NN.compare(got, reference("scene", PC.SCENE_CENTRE), "scene towards its centre")
    # without a viewpoint: the component of largest magnitude is positive, checked where it leads by more than 2
    for name in ("scene", "tilted", "size6161"):
        _, payload, (radius, min_nb, flat) = CASES[name]
        got = host(payload, radius, min_nb, flat)
        g = got[got[:, 3] != 0, :3].astype(np.int64)
        a = np.sort(np.abs(g), axis=1)
        clear = a[:, 2] - a[:, 1] > 2
        lead = g[np.arange(g.shape[0]), np.abs(g).argmax(axis=1)]
        assert clear.sum() > 0 and (lead[clear] > 0).all(), name


def test_equal_records_and_payload_order_on_the_host(host):
    _, payload, (radius, min_nb, flat) = CASES["size2049"]
    doubled = np.concatenate([payload, payload[::3]])
    got = host(doubled, radius, min_nb, flat)
    assert (got[2049:] == got[:2049:3]).all()
    order = np.random.default_rng(4).permutation(doubled.shape[0])
    again = host(np.ascontiguousarray(doubled[order]), radius, min_nb, flat)
    assert (again == got[order]).all()
