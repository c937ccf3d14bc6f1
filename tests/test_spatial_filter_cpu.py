"""The spatial filter without a GPU: the two forms of the numpy restatement (tests/np_spatial_filter.py) against each other and
against hand-worked vectors, the census that shows the test scene reaches every branch of the step, the config struct as the
header, ctypes and the symbol table see it, and pcs-camera-optimized's -S, which refuses a bad spec with status 2 before a
context exists."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_spatial_filter as SP
from pointcloud_stitching_amd import api, lib as L
from pointcloud_stitching_amd.types import SpatialFilterConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
EDGE = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-camera-optimized")
FIELDS = ["alpha", "delta", "iterations", "hole_radius"]

SCENE_SHAPES, CENSUS_SHAPES, PARAMS, FULL_RANGE, full_range_raster = (SP.SCENE_SHAPES, SP.CENSUS_SHAPES, SP.PARAMS, SP.FULL_RANGE,
                                                                     SP.full_range_raster)


@pytest.fixture(scope="module")
def edge():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert os.path.exists(EDGE)
    return EDGE


@pytest.mark.parametrize("name", sorted(PARAMS))
@pytest.mark.parametrize("w,h", SCENE_SHAPES)
def test_loop_and_vectorised_forms_agree(w, h, name):
    d = SP.scene(w, h, 3)
    assert d.shape == (h, w) and d.dtype == np.uint16
    got, _ = SP.spatial_filter(d, **PARAMS[name])
    assert np.array_equal(got, SP.spatial_filter_loop(d, **PARAMS[name]))


def test_forms_agree_on_the_full_range_and_special_rasters():
    d = full_range_raster()
    got, census = SP.spatial_filter(d, **FULL_RANGE)
    assert np.array_equal(got, SP.spatial_filter_loop(d, **FULL_RANGE))
    assert census["blend"] > 0 and census["fill"] > 0 and census["fill_exhausted"] > 0
    row = d[5].copy()                                # the blend at the top of the range: 65534 against 65535 rounds to 65535
    SP.line_pass_loop(row, FULL_RANGE["alpha"], FULL_RANGE["delta"], FULL_RANGE["hole_radius"], True)
    assert row[9] == 0 and row[10:14].tolist() == [65535, 65535, 65535, 65535]
    for special in (np.zeros((9, 17), np.uint16), np.full((9, 17), 1234, np.uint16)):
        got, census = SP.spatial_filter(special, **PARAMS["radius2"])
        assert np.array_equal(got, special) and np.array_equal(SP.spatial_filter_loop(special, **PARAMS["radius2"]), special)
        assert census["blend"] == census["edge"] == census["fill"] == census["fill_exhausted"] == 0


@pytest.mark.parametrize("w,h", CENSUS_SHAPES)
def test_the_scene_reaches_every_branch(w, h):
    d = SP.scene(w, h, 3)
    out, census = SP.spatial_filter(d, **PARAMS["radius2"])
    print(w, h, census)
    assert all(census[b] > 0 for b in SP.BRANCHES), census
    assert not np.array_equal(out, d)
    _, census0 = SP.spatial_filter(d, **PARAMS["defaults"])
    assert census0["fill"] == 0 and census0["fill_exhausted"] > 0 and census0["blend"] > 0


ROW = [100, 110, 105, 500, 0, 0, 0, 300]


def test_hand_worked_row():
    """alpha 0.5, delta 20, radius 2. Forward: 110 against 100 blends to fl(55 + 50) + 0.5 = 105.5 -> 105; the next 105 ties
    (d = 0: untouched); 500 is an edge; the gap of three takes two pixels and leaves the third, after which v0 is 0 and 300 comes
    through untouched. Backward: the open pixel is filled from the right (300), 500 / 105 are edges, 100 against 105 blends to
    fl(50 + 52.5) + 0.5 = 103."""
    x = np.array(ROW, np.uint16)
    SP.line_pass_loop(x, 0.5, 20, 2, True)
    assert x.tolist() == [100, 105, 105, 500, 500, 500, 0, 300]
    SP.line_pass_loop(x[::-1], 0.5, 20, 2, True)
    assert x.tolist() == [103, 105, 105, 500, 500, 500, 300, 300]
    for form in (SP.spatial_filter_loop, lambda *a, **k: SP.spatial_filter(*a, **k)[0]):
        got = form(np.array([ROW], np.uint16), alpha=0.5, delta=20, iterations=1, hole_radius=2)
        assert got.tolist() == [[103, 105, 105, 500, 500, 500, 300, 300]]
    _, census = SP.spatial_filter(np.array([ROW], np.uint16), alpha=0.5, delta=20, iterations=1, hole_radius=2)
    assert census == {"blend": 2, "equal": 4, "edge": 3, "fill": 3, "fill_exhausted": 1}


def test_hand_worked_column_fills_nothing():
    """The same values down a column: the column passes never fill, so the gap stays and 500 meets no valid neighbour below it."""
    x = np.array(ROW, np.uint16)
    SP.line_pass_loop(x, 0.5, 20, 2, False)
    assert x.tolist() == [100, 105, 105, 500, 0, 0, 0, 300]
    for form in (SP.spatial_filter_loop, lambda *a, **k: SP.spatial_filter(*a, **k)[0]):
        got = form(np.array(ROW, np.uint16).reshape(8, 1), alpha=0.5, delta=20, iterations=1, hole_radius=2)
        assert got.reshape(-1).tolist() == [103, 105, 105, 500, 0, 0, 0, 300]
    one = np.array([[7]], np.uint16)
    assert SP.spatial_filter_loop(one).tolist() == [[7]] and SP.spatial_filter(one)[0].tolist() == [[7]]


def test_header_ctypes_and_symbols_agree_on_the_config_struct(tmp_path):
    prog = tmp_path / "sizes.cpp"
    prog.write_text('#include <cstddef>\n#include <cstdio>\n#include "pcs_hip.h"\nint main() {\n'
                    '  printf("%zu", sizeof(pcs_spatial_filter_config));\n'
                    + "".join(f'  printf(" %zu", offsetof(pcs_spatial_filter_config, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["g++", "-I", L.INCLUDE_DIR, str(prog), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(SpatialFilterConfig) == 16
    assert got[1:] == [getattr(SpatialFilterConfig, f).offset for f in FIELDS]
    assert [n for n, _ in SpatialFilterConfig._fields_] == FIELDS
    assert SpatialFilterConfig.alpha.size == 4 and dict(SpatialFilterConfig._fields_)["alpha"] is C.c_float
    assert api.SpatialFilterConfig is SpatialFilterConfig
    sym = {name: args for name, _, args in L.SYMBOLS}
    for name in ("pcs_spatial_filter_depth_device", "pcs_spatial_filter_depth"):
        assert sym[name][1] is C.POINTER(SpatialFilterConfig) and len(sym[name]) == 4
        assert hasattr(L.load(), name)
    for method in ("spatial_filter_depth_device", "spatial_filter_depth"):
        assert callable(getattr(api.PcsContext, method))


def run(*args, timeout=120):
    return subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_help_lists_the_spatial_flag(edge):
    r = run(edge, "-h")
    assert r.returncode == 0
    assert "-S <alpha:delta:iterations[:radius] | default>" in r.stdout


MALFORMED = ["", "0:20:2", "1.5:20:2", "nan:20:2", "0.5:0:2", "0.5:20:0", "0.5:20:6", "0.5:20", "0.5:20:2:-1", "0.5:20:2:70000", "foo"]


@pytest.mark.parametrize("arg", MALFORMED)
def test_malformed_spatial_spec_exits_2_before_any_context(edge, arg):
    r = run(edge, "-f", "synth:64x48", "-m", "-r", "1", "-S", arg)
    assert r.returncode == 2, r.stderr
    assert "-S" in r.stderr and "pcs_create" not in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1
