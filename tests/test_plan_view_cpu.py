"""Plan-view maps without a GPU: the restatement (tests/np_plan_view.py) against its own plain-loop statement; the kernels' arithmetic
(csrc/pcs_plan_math.h) and the option parser and Netpbm writers of cli/pcs_planview.h, compiled for the host by tools/plan_host.cpp,
against the restatement over every case of tests/plan_view_cases.py — cells and keys per record, and the whole maps behind a plain
loop; the division swept in C over all 65 536 numerators x all 32 767 cell edges; the bindings' layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_plan_view as NP
import plan_view_cases as K
from pointcloud_stitching_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(K.CASES)


def c_params(P, reserved=(0, 0, 0)):
    return T.PlanParams.make(P["up_axis"], P["up_sign"], P["cell_mm"], P["width"], P["height"], P["origin_u"], P["origin_v"], P["band_lo"],
                             P["band_hi"], reserved)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("plan_host") / "libplan_host.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "pointcloud_stitching_amd", "csrc"),
           "-I", os.path.join(ROOT, "pointcloud_stitching_amd", "cli"), os.path.join(ROOT, "tools", "plan_host.cpp"), "-o", so]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    lib = C.CDLL(so)
    lib.plan_host_bad_param.restype = C.c_int
    lib.plan_host_bad_param.argtypes = [C.POINTER(T.PlanParams)]
    lib.plan_host_records.restype = None
    lib.plan_host_records.argtypes = [C.c_void_p, C.c_int, C.POINTER(T.PlanParams)] + [C.c_void_p] * 4
    lib.plan_host_maps.restype = None
    lib.plan_host_maps.argtypes = [C.c_void_p, C.c_int, C.POINTER(T.PlanParams)] + [C.c_void_p] * 5
    lib.plan_host_sweep.restype = C.c_longlong
    lib.plan_host_sweep.argtypes = [C.c_int, C.c_int]
    lib.plan_host_parse.restype = C.c_int
    lib.plan_host_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(T.PlanParams), C.c_char_p, C.c_int]
    lib.plan_host_write.restype = C.c_int
    lib.plan_host_write.argtypes = [C.c_char_p, C.POINTER(T.PlanParams)] + [C.c_void_p] * 3
    return lib


def host_maps(host, rec, P):
    rec = np.ascontiguousarray(rec, np.int16)
    W, H = P["width"], P["height"]
    count, top, bottom = np.full((H, W), 0xA5A5A5A5, np.uint32), np.full((H, W), 0x5A5A, np.int16), np.full((H, W), 0x5A5A, np.int16)
    rgb, stats = np.full((H, W, 3), 0xA5, np.uint8), np.full(8, -1, np.int64)
    host.plan_host_maps(rec.ctypes.data, rec.shape[0], C.byref(c_params(P)), count.ctypes.data, top.ctypes.data, bottom.ctypes.data, rgb.ctypes.data,
                        stats.ctypes.data)
    assert not stats[5:].any()
    return count, top, bottom, rgb, dict(zip(NP.STATS_FIELDS, (int(v) for v in stats[:5])))


def test_the_layout_of_the_bindings():
    assert C.sizeof(T.PlanParams) == 48 and C.sizeof(T.PlanStats) == 64 and C.sizeof(T.PlanMaps) == 40
    assert [name for name, _ in T.PlanParams._fields_] == ["up_axis", "up_sign", "cell_mm", "origin_u", "origin_v", "width", "height", "band_lo",
                                                           "band_hi", "reserved"]
    assert [getattr(T.PlanParams, name).offset for name, _ in T.PlanParams._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]
    assert [name for name, _ in T.PlanStats._fields_] == list(NP.STATS_FIELDS) + ["reserved"] == list(T.PLAN_STATS_FIELDS) + ["reserved"]
    assert [name for name, _ in T.PlanMaps._fields_] == ["count", "top", "bottom", "rgb", "stats"]
    assert [getattr(T.PlanMaps, name).offset for name, _ in T.PlanMaps._fields_] == [0, 8, 16, 24, 32]
    assert T.PLAN_VIEW_LAUNCHES == ("clear", "accumulate", "resolve")
    assert (T.PLAN_SIDE_MAX, T.PLAN_CELLS_MAX) == (NP.SIDE_MAX, NP.CELLS_MAX) == (4096, 1 << 22)
    p = T.PlanParams.make(2, 1, 10, 401, 300)
    assert (p.origin_u, p.origin_v, p.band_lo, p.band_hi) == (-2005, -1500, -32768, 32767) and list(p.reserved) == [0, 0, 0]


@pytest.mark.parametrize("name", [n for n in NAMES if K.CASES[n].rec.shape[0] <= 70000])
def test_the_restatement_against_the_plain_loop(name):
    c = K.CASES[name]
    NP.compare(NP.plan_np(c.rec, c.P), NP.plan_loop(c.rec, c.P), name)


def test_the_restatement_on_inputs_worked_by_hand():
    rec = K.records([[0, 0, 5], [9, 9, 7], [10, 0, -3], [0, 0, 7], [-1, 0, 100], [0, 0, 1]])
    P = NP.params(cell_mm=10, width=2, height=1, origin=(0, 0))
    count, top, bottom, rgb, stats = NP.plan_np(rec, P)
    assert count.tolist() == [[4, 1]] and top.tolist() == [[7, -3]] and bottom.tolist() == [[1, -3]]
    assert rgb[0, 0].tolist() == [int(rec[1, 3]) & 0xFF, (int(rec[1, 3]) >> 8) & 0xFF, int(rec[1, 4]) & 0xFF]      # index 1 before index 3
    assert stats == dict(considered=6, in_band=6, mapped=5, occupied=2, fullest=4)
    count, top, bottom, _, _ = NP.plan_np(rec, dict(P, up_sign=-1))
    assert top.tolist() == [[1, -3]] and bottom.tolist() == [[7, -3]]                                            # seen from below
    kt, kb = NP.keys_np(K.records([[0, 0, -32768]]), dict(P, up_sign=-1))
    assert int(kt[0]) == (65536 << 32) | 0xFFFFFFFF and int(kb[0]) == 0xFFFFFFFF                               # h = 32768; a key is never 0
    kt, kb = NP.keys_np(K.records([[0, 0, -32768]]), P)
    assert int(kt[0]) == 0xFFFFFFFF and int(kb[0]) == (65536 << 32) | 0xFFFFFFFF


def test_the_cases_are_what_they_say():
    assert K.CASES["n_8193"].rec.shape[0] == K.TILE + 1 == 8193
    c = K.CASES["table_overflow"]
    _, cell = NP.cells_np(c.rec, c.P)
    assert np.unique(cell[:K.TILE]).shape[0] == K.TILE > K.TABLE_SLOTS and (cell >= 0).all()       # a tile's records: a cell each
    c = K.CASES["wave_64_cells"]
    assert np.unique(NP.cells_np(c.rec, c.P)[1]).shape[0] == 64
    c = K.CASES["wave_two_cells"]
    cell = NP.cells_np(c.rec, c.P)[1]
    assert np.unique(cell).shape[0] == 2 and (cell[::2] == cell[0]).all() and (cell[1::2] == cell[1]).all()
    c = K.CASES["wall_equal"]
    assert np.unique(c.rec[:, :3], axis=0).shape[0] == 1 and np.unique(c.rec[:, 3:], axis=0).shape[0] > 60000
    for up in ("-x", "-y", "-z"):
        c = K.CASES[f"up_{up}"]
        assert (NP.keys_np(c.rec, c.P)[0] >> np.uint64(32)).max() == 65536                            # h = 32768 is met
    for cell in (1, 2, 3, 7, 10, 1000, 32767):
        assert f"borders_c{cell}" in K.CASES
    w = K.working_size()
    assert w.rec.shape[0] == 1 << 20 and (w.P["width"], w.P["height"]) == (400, 400)


@pytest.mark.parametrize("name", NAMES)
def test_cells_and_keys_of_every_record(host, name):
    c = K.CASES[name]
    rec = np.ascontiguousarray(c.rec)
    n = rec.shape[0]
    in_band, cell, kt, kb = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    host.plan_host_records(rec.ctypes.data, n, C.byref(c_params(c.P)), in_band.ctypes.data, cell.ctypes.data, kt.ctypes.data, kb.ctypes.data)
    want_band, want_cell = NP.cells_np(rec, c.P)
    want_kt, want_kb = NP.keys_np(rec, c.P)
    assert (in_band.astype(bool) == want_band).all() and (cell == want_cell).all(), name
    assert (kt == want_kt).all() and (kb == want_kb).all(), name
    assert (kt > 0).all() and (kb > 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_the_maps_behind_a_plain_loop(host, name):
    c = K.CASES[name]
    NP.compare(host_maps(host, c.rec, c.P), NP.plan_np(c.rec, c.P), name)


def test_the_working_size_case_on_the_host(host):
    c = K.working_size()
    NP.compare(host_maps(host, c.rec, c.P), NP.plan_np(c.rec, c.P), "working size")


def test_the_division_for_every_numerator_and_every_cell(host):
    assert host.plan_host_sweep(1, 32767) == 0
    # the multiply-shift is not exact by luck: a magic one too small fails the same sweep's comparison
    d = np.arange(65536, dtype=np.uint64)
    for c in (3, 7, 10, 641, 32767):
        m = np.uint64((1 << 32) // c + 1)
        assert (((d * m) >> np.uint64(32)) == d // np.uint64(c)).all()
        assert not (((d * (m - np.uint64(1))) >> np.uint64(32)) == d // np.uint64(c)).all()


def test_the_parameter_ranges(host):
    good = NP.params()
    assert host.plan_host_bad_param(C.byref(c_params(good))) == 0
    for k, (field, values) in enumerate((("up_axis", (-1, 3)), ("up_sign", (0, 2, -2)), ("cell_mm", (0, -1, 32768)), ("origin_u", (-32769, 32768)),
                                         ("origin_v", (-32769, 32768)), ("width", (0, 4097)), ("height", (0, 4097)), ("band_lo", (-32769, 32768)),
                                         ("band_hi", (32768, -32769)))):
        for v in values:
            assert host.plan_host_bad_param(C.byref(c_params(dict(good, **{field: v})))) == k + 1, (field, v)
    assert host.plan_host_bad_param(C.byref(c_params(dict(good, band_lo=5, band_hi=4)))) == 9
    assert host.plan_host_bad_param(C.byref(c_params(dict(good, width=4096, height=1025)))) == 7
    assert host.plan_host_bad_param(C.byref(c_params(dict(good, width=4096, height=1024)))) == 0
    assert host.plan_host_bad_param(C.byref(c_params(dict(good, width=1, height=4096, cell_mm=32767, origin_u=32767, origin_v=-32768, band_lo=7, band_hi=7)))) == 0
    for k in range(3):
        reserved = [0, 0, 0]
        reserved[k] = 1
        assert host.plan_host_bad_param(C.byref(c_params(good, reserved))) == 10 + k


def parse(host, arg):
    prefix, why, p = C.create_string_buffer(256), C.create_string_buffer(512), T.PlanParams()
    ok = host.plan_host_parse(arg.encode(), prefix, 256, C.byref(p), why, 512)
    return bool(ok), prefix.value.decode(), p, why.value.decode()


def test_the_option_parser(host):
    ok, prefix, p, _ = parse(host, "out/map,+z,10,400x300")
    assert ok and prefix == "out/map"
    assert [getattr(p, f) for f in ("up_axis", "up_sign", "cell_mm", "origin_u", "origin_v", "width", "height", "band_lo", "band_hi")] == \
        [2, 1, 10, -2000, -1500, 400, 300, -32768, 32767] and list(p.reserved) == [0, 0, 0]
    for up, (a, s) in NP.UP_NAMES.items():
        ok, _, p, _ = parse(host, f"m,{up},7,3x5")
        assert ok and (p.up_axis, p.up_sign) == (a, s) and (p.origin_u, p.origin_v) == (-10, -17)       # -(3 * 7) / 2, -(5 * 7) / 2
    ok, _, p, _ = parse(host, "m,-y,25,7x5,-80,-60")
    assert ok and (p.origin_u, p.origin_v, p.band_lo, p.band_hi) == (-80, -60, -32768, 32767)
    ok, _, p, _ = parse(host, "m,-y,32767,1x1,-32768,32767,-100,900")
    assert ok and (p.cell_mm, p.origin_u, p.origin_v, p.band_lo, p.band_hi) == (32767, -32768, 32767, -100, 900)
    ok, _, p, _ = parse(host, "m,+x,1,4096x1024,0,0,5,5")
    assert ok and (p.width, p.height, p.band_lo, p.band_hi) == (4096, 1024, 5, 5)
    for arg, word in (("", "expected"), ("m", "expected"), ("m,+z,10", "expected"), ("m,+z,10,4x4,1", "expected"), ("m,+z,10,4x4,1,2,3", "expected"),
                      ("m,+z,10,4x4,1,2,3,4,5", "expected"), (",+z,10,4x4", "prefix"), ("-m,+z,10,4x4", "prefix"), ("m,z,10,4x4", "<up>"),
                      ("m,+w,10,4x4", "<up>"), ("m,+zz,10,4x4", "<up>"), ("m,+z,ten,4x4", "cell_mm"), ("m,+z, 10,4x4", "cell_mm"),
                      ("m,+z,10mm,4x4", "cell_mm"), ("m,+z,0,4x4", "cell_mm"), ("m,+z,32768,4x4", "cell_mm"), ("m,+z,10,4", "<W>x<H>"),
                      ("m,+z,10,4x", "<W>x<H>"), ("m,+z,10,x4", "<W>x<H>"), ("m,+z,10,4x4x4", "<W>x<H>"), ("m,+z,10,0x4", "W and H"),
                      ("m,+z,10,4097x1", "W and H"), ("m,+z,10,4096x1025", "W and H"), ("m,+z,10,4x4,a,0", "<u0>,<v0>"),
                      ("m,+z,10,4x4,70000,0", "origin"), ("m,+z,10,4x4,0,-32769", "origin"), ("m,+z,100,4000x10", "origin"),
                      ("m,+z,10,4x4,1,2,lo,4", "<lo>,<hi>"), ("m,+z,10,4x4,1,2,5,4", "band"), ("m,+z,10,4x4,1,2,-40000,4", "band"),
                      ("m,+z,10,4x4,1,2,3,32768", "band")):
        ok, _, _, why = parse(host, arg)
        assert not ok and word in why, (arg, why)


def test_the_three_files(host, tmp_path):
    """The bytes of the three files for a small map against bytes built in Python: row r is cv = r, no flip; the grey maps big-endian;
    a saturated count, a clamped height at both ends, an empty cell."""
    P = NP.params(up="-z", cell_mm=10, width=5, height=3, origin=(0, 0))
    xyz = [[1, 1, 32767], [1, 2, -32768], [12, 1, 0], [45, 25, -5], [45, 25, 9], [22, 15, 100]]
    rec = np.concatenate([K.records(xyz, 3), K.records([[33, 5, 7]] * 70000, 4)])
    count, top, bottom, rgb, stats = NP.plan_np(rec, P)
    assert count[0, 3] == 70000 and count[0, 0] == 2 and top[0, 0] == -32768 and count[2, 0] == 0 and stats["occupied"] == 5
    prefix = str(tmp_path / "map")
    assert host.plan_host_write(prefix.encode(), C.byref(c_params(P)), np.ascontiguousarray(count).ctypes.data, np.ascontiguousarray(top).ctypes.data,
                                np.ascontiguousarray(rgb).ctypes.data) == 0
    want = NP.netpbm_bytes(count, top, rgb, P)
    for suffix, data in zip((".rgb.ppm", ".top.pgm", ".count.pgm"), want):
        with open(prefix + suffix, "rb") as f:
            assert f.read() == data, suffix
    # ... and those bytes spelled out, independent of netpbm_bytes
    assert want[0][:11] == b"P6\n5 3\n255\n" and len(want[0]) == 11 + 45 and want[0][11:14] == bytes(rgb[0, 0].tolist())
    assert want[1][:13] == b"P5\n5 3\n65535\n" and len(want[1]) == 13 + 30
    grey = np.frombuffer(want[1][13:], ">u2").reshape(3, 5)
    assert grey[0, 0] == 65535 and grey[0, 1] == 32768 and grey[2, 0] == 0 and grey[2, 4] == 32768 + 5 and grey[1, 2] == 32768 - 100
    sat = np.frombuffer(want[2][13:], ">u2").reshape(3, 5)
    assert sat[0, 3] == 65535 and sat[0, 0] == 2 and sat[2, 4] == 2 and sat[2, 0] == 0
    # seen from above the lowest raw coordinate clamps at 1, not 0: 0 is the empty cell
    Pz = dict(P, up_sign=1)
    one = K.records([[1, 1, -32768]])
    c1, t1, _, r1, _ = NP.plan_np(one, Pz)
    assert host.plan_host_write(prefix.encode(), C.byref(c_params(Pz)), np.ascontiguousarray(c1).ctypes.data, np.ascontiguousarray(t1).ctypes.data,
                                np.ascontiguousarray(r1).ctypes.data) == 0
    with open(prefix + ".top.pgm", "rb") as f:
        data = f.read()
    assert data == NP.netpbm_bytes(c1, t1, r1, Pz)[1] and np.frombuffer(data[13:], ">u2")[0] == 1
