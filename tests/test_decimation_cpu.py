"""The depth decimation without a GPU: the numpy restatement against a brute-force loop, pcs_decimated_stream_config (pure host
arithmetic in the library) against the restatement's double-then-float formulas bit for bit, the geometry those formulas promise,
and pcs-camera-optimized's -D, which refuses a bad scale with status 2 before a context exists."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_decimation as D
from pointcloud_stitching_amd import api, lib as L, synthetic as S
from pointcloud_stitching_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
EDGE = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-camera-optimized")
INVALID_ARG = -1


@pytest.fixture(scope="module")
def edge():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert os.path.exists(EDGE)
    return EDGE


def brute(d, n):
    """The definition, pixel by pixel, in plain Python integers."""
    h, w = len(d) // n, len(d[0]) // n
    out = [[0] * w for _ in range(h)]
    for r in range(h):
        for c in range(w):
            valid = sorted(d[n * r + a][n * c + b] for a in range(n) for b in range(n) if d[n * r + a][n * c + b] != 0)
            k = len(valid)
            if k:
                out[r][c] = valid[(k - 1) >> 1] if n <= 3 else sum(valid) // k
    return out


@pytest.mark.parametrize("n", range(2, 9))
def test_restatement_against_the_brute_force_loop(n):
    rng = np.random.default_rng(100 + n)
    d = rng.integers(1, 65536, (24, 24)).astype(np.uint16)
    d[rng.random(d.shape) < 1 / 3] = 0
    d[1, 1], d[2, 5] = 1, 65535
    got = D.decimate(d, n)
    assert got.dtype == np.uint16 and got.shape == (24 // n, 24 // n)
    assert got.tolist() == brute(d.tolist(), n)
    assert (d == 0).any() and (got != 0).any()


def distorted_config():
    di = T.make_intrinsics(1280, 720, 911.37, 909.82, 641.3, 358.9, T.DISTORTION_BROWN_CONRADY, [0.11, -0.23, 0.0013, -0.0007, 0.071])
    ci = T.make_intrinsics(1920, 1080, 1380.5, 1379.1, 962.2, 541.7, T.DISTORTION_INVERSE_BROWN_CONRADY, [0.05, -0.02, 0.001, 0.002, 0.01])
    return T.make_stream_config(di, ci, translation=(0.0148, 0.0002, -0.0003), color_bpp=4)


CONFIGS = {"1280x720": lambda: S.synth_stream_config(1280, 720, 2), "68x48": lambda: S.synth_stream_config(68, 48, 0, single=True),
           "distorted": distorted_config}


def raw(cfg):
    return bytes(C.string_at(C.addressof(cfg), C.sizeof(cfg)))


def bits(x):
    return np.float32(x).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("n", range(1, 9))
def test_decimated_stream_config_matches_the_restatement_bit_for_bit(name, n):
    lib = L.load()
    cfg = CONFIGS[name]()
    before = raw(cfg)
    want = D.decimated_config(cfg, n)
    got = T.StreamConfig()
    assert lib.pcs_decimated_stream_config(C.byref(cfg), n, C.byref(got)) == 0
    assert raw(cfg) == before
    for f in ("fx", "fy", "ppx", "ppy"):
        assert bits(getattr(got.depth, f)) == bits(getattr(want.depth, f)), f
    assert (got.depth.width, got.depth.height) == (cfg.depth.width // n, cfg.depth.height // n)
    assert got.depth.model == cfg.depth.model and list(got.depth.coeffs) == list(cfg.depth.coeffs)
    assert raw(got) == raw(want)                       # every other byte too: colour, extrinsics, scale, stride, cam_to_world
    assert raw(got.color) == raw(cfg.color) and raw(got.depth_to_color) == raw(cfg.depth_to_color)
    assert raw(T.decimated_stream_config(cfg, n)) == raw(want)        # the Python wrapper is the same function
    if n == 1:
        assert raw(got) == before
    else:
        assert raw(got) != before
    same = CONFIGS[name]()                              # in == out is allowed
    assert lib.pcs_decimated_stream_config(C.byref(same), n, C.byref(same)) == 0
    assert raw(same) == raw(want)


def test_decimated_stream_config_refusals():
    lib = L.load()
    cfg, out = S.synth_stream_config(68, 48), T.StreamConfig()
    blank = raw(out)
    for n in (0, 9, -1):
        assert lib.pcs_decimated_stream_config(C.byref(cfg), n, C.byref(out)) == INVALID_ARG
        assert b"scale" in lib.pcs_last_error(None)
    tiny = S.synth_stream_config(1, 1)
    assert lib.pcs_decimated_stream_config(C.byref(tiny), 1, C.byref(out)) == 0
    out = T.StreamConfig()
    assert lib.pcs_decimated_stream_config(C.byref(tiny), 2, C.byref(out)) == INVALID_ARG
    assert lib.pcs_decimated_stream_config(C.byref(S.synth_stream_config(68, 7)), 8, C.byref(out)) == INVALID_ARG
    assert lib.pcs_decimated_stream_config(None, 2, C.byref(out)) == INVALID_ARG
    assert lib.pcs_decimated_stream_config(C.byref(cfg), 2, None) == INVALID_ARG
    assert raw(out) == blank                            # a refusal writes nothing
    for n in (0, 9):
        with pytest.raises(ValueError):
            T.decimated_stream_config(cfg, n)
    with pytest.raises(ValueError):
        T.decimated_stream_config(tiny, 2)
    for method in ("decimate_depth_device", "decimate_depth"):
        assert callable(getattr(api.PcsContext, method))


@pytest.mark.parametrize("n", range(2, 9))
def test_a_decimated_pixel_looks_along_the_centre_of_its_block(n):
    """fp32 (i - ppx') / fx' against the double mean over the block's source columns of (c - ppx) / fx. 2e-6 absolute: half an ulp
    of ppx' (<= 3e-5 at |ppx'| < 512) over fx' >= 37 is below 1e-6, and the subtract and the divide add relative 2^-23 each to
    |mx| < 2."""
    cfg = S.synth_stream_config(1280, 720)
    assert cfg.depth.model == T.DISTORTION_NONE
    dec = T.decimated_stream_config(cfg, n)
    for size, pp, f, pp_d, f_d in ((1280, cfg.depth.ppx, cfg.depth.fx, dec.depth.ppx, dec.depth.fx),
                                   (720, cfg.depth.ppy, cfg.depth.fy, dec.depth.ppy, dec.depth.fy)):
        m = size // n
        i = np.arange(m, dtype=np.float32)
        got = (i - np.float32(pp_d)) / np.float32(f_d)
        assert got.dtype == np.float32
        src = (np.arange(n * m, dtype=np.float64) - np.float64(pp)) / np.float64(f)
        want = src.reshape(m, n).mean(axis=1)
        worst = float(np.abs(got.astype(np.float64) - want).max())
        print(f"n = {n}, size {size}: worst |difference| {worst:.3g}")
        assert worst <= 2e-6
        assert np.abs(want).max() < 2 and np.float32(f_d) >= 37


def run(*args, timeout=120):
    return subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_help_lists_the_decimation_flag(edge):
    r = run(edge, "-h")
    assert r.returncode == 0 and "-D <n>" in r.stdout


@pytest.mark.parametrize("arg", ["9", "x", "0", "", "2x", "-3", "2.5"])
def test_bad_decimation_scale_exits_2_before_any_context(edge, arg):
    r = run(edge, "-f", "synth:64x48", "-m", "-r", "1", "-D", arg)
    assert r.returncode == 2, r.stderr
    assert "-D" in r.stderr and "pcs_create" not in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1
