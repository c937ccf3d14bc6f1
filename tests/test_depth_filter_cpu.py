"""The depth pre-filter without a GPU: the restatement agrees with itself, the persistence table is the documented one, the header,
the ctypes mirror and the bound symbols agree on pcs_depth_filter_config, and pcs-camera-optimized's -F is listed and refuses every
malformed spec with status 2 before a context exists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import np_depth_filter as F
from pointcloud_stitching_amd import api, lib as L, synthetic as S
from pointcloud_stitching_amd.types import DepthFilterConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
EDGE = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-camera-optimized")
FIELDS = ["temporal", "alpha", "delta", "persistence", "hole_fill"]


@pytest.fixture(scope="module")
def edge():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert os.path.exists(EDGE)
    return EDGE


def run(*args, timeout=120):
    return subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_loop_and_vectorised_fill_agree():
    rng = np.random.default_rng(5)
    cases = [S.synth_depth(68, 12, 0), S.synth_depth(64, 9, 1, mode="random"), np.zeros((3, 17), np.uint16),
             np.full((2, 5), 7, np.uint16)]
    sparse = S.synth_depth(133, 7, 2, mode="random")
    sparse[rng.random(sparse.shape) < 0.9] = 0
    cases.append(sparse)
    for d in cases:
        a, b = F.fill_left(d), F.fill_left_loop(d)
        assert a.dtype == np.uint16 and np.array_equal(a, b)
        assert np.array_equal(a[d != 0], d[d != 0])                       # valid pixels are never touched
    hand = np.array([[0, 0, 5, 0, 0, 9, 0], [0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0]], np.uint16)
    want = np.array([[0, 0, 5, 5, 5, 9, 9], [0, 0, 0, 0, 0, 0, 0], [3, 3, 3, 3, 3, 3, 3]], np.uint16)
    assert np.array_equal(F.fill_left(hand), want)


def test_persistence_table_is_the_documented_one():
    """DESIGN.md section 3 and the header list the rules in words; the restatement's table and the library's (read from its source)
    are that list."""
    assert F.PERSISTENCE == [(9, 8), (8, 8), (2, 3), (2, 4), (2, 8), (1, 2), (1, 5), (1, 8), (0, 8)]
    src = open(os.path.join(L.CSRC_DIR, "pcs_capi.cpp")).read()
    m = re.search(r"kPersistM\[9\]\s*=\s*\{([^}]*)\}", src)
    l = re.search(r"kPersistL\[9\]\s*=\s*\{([^}]*)\}", src)
    assert m and l
    pairs = list(zip([int(v) for v in m.group(1).split(",")], [int(v) for v in l.group(1).split(",")]))
    assert pairs == F.PERSISTENCE
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "(9,8)" in design and "(8,8), (2,3), (2,4), (2,8), (1,2), (1,5), (1,8)" in design and "(0,8)" in design
    # what the rules mean, on scripted histories: a pixel last seen valid, then invalid
    for persistence, (m_need, l_span) in enumerate(F.PERSISTENCE):
        for hist in range(256):
            st = F.State((1, 1))
            st.last[...] = 1234
            st.hist[...] = hist
            out = F.temporal(np.zeros((1, 1), np.uint16), st, persistence=persistence)
            seen = bin(hist & ((1 << l_span) - 1)).count("1")
            assert int(out[0, 0]) == (1234 if seen >= m_need else 0)
            assert int(st.last[0, 0]) == 1234 and int(st.hist[0, 0]) == (hist << 1) & 0xFF


def test_header_ctypes_and_symbols_agree_on_the_config_struct(tmp_path):
    prog = tmp_path / "sizes.cpp"
    prog.write_text('#include <cstddef>\n#include <cstdio>\n#include "pcs_hip.h"\nint main() {\n'
                    '  printf("%zu", sizeof(pcs_depth_filter_config));\n'
                    + "".join(f'  printf(" %zu", offsetof(pcs_depth_filter_config, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["g++", "-I", L.INCLUDE_DIR, str(prog), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(DepthFilterConfig) == 20
    assert got[1:] == [getattr(DepthFilterConfig, f).offset for f in FIELDS]
    assert [n for n, _ in DepthFilterConfig._fields_] == FIELDS
    assert api.DepthFilterConfig is DepthFilterConfig
    sym = {name: args for name, _, args in L.SYMBOLS}
    assert sym["pcs_set_depth_filter"][1] is C.POINTER(DepthFilterConfig)
    assert sym["pcs_get_depth_filter"][1] is C.POINTER(DepthFilterConfig)
    for name in ("pcs_reset_depth_filter", "pcs_filter_depth_device", "pcs_filter_depth"):
        assert name in sym
    for method in ("set_depth_filter", "depth_filter", "reset_depth_filter", "filter_depth_device", "filter_depth"):
        assert callable(getattr(api.PcsContext, method))


def test_help_lists_the_filter_flag(edge):
    r = run(edge, "-h")
    assert r.returncode == 0
    assert "-F <temporal[=alpha:delta:persistence],holes[=left]>" in r.stdout


MALFORMED = ["", "temporal=", "temporal=0:20:3", "temporal=1.5:20:3", "temporal=0.4:0:3", "temporal=0.4:20:9", "temporal=0.4:20",
             "holes=right", "holes=around", "foo", "temporal=nan:20:3"]


@pytest.mark.parametrize("arg", MALFORMED)
def test_malformed_filter_spec_exits_2_before_any_context(edge, arg):
    r = run(edge, "-f", "synth:64x48", "-m", "-r", "1", "-F", arg)
    assert r.returncode == 2, r.stderr
    assert "-F" in r.stderr and "pcs_create" not in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1
