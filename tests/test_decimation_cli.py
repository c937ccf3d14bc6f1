"""pcs-camera-optimized -D on the GPU: `-f synth:128x96 -m -n 2 -D 2 -F temporal,holes -r 4` dumps what the library chain
(decimate, filter, stitch) gives for the last of the same four synthetic frames, and `-D 1` is a run without -D."""
import os
import subprocess

import numpy as np
import pytest

import np_decimation as D
import np_depth_filter as F
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import HEADER_SHORTS, decimated_stream_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
EDGE = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-camera-optimized")
W, H, N_STREAMS, FRAMES = 128, 96, 2, 4


def edge(*args):
    r = subprocess.run([EDGE, "-f", f"synth:{W}x{H}", "-m", "-n", str(N_STREAMS), "-r", str(FRAMES), *args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"### Total Frames = {FRAMES}" in r.stdout
    return r.stdout


@pytest.mark.gpu
def test_edge_cli_decimates_like_the_library(tmp_path):
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = str(tmp_path / "dump.bin")
    text = edge("-D", "2", "-F", "temporal,holes", "-o", out)
    assert f"### Depth Frames H x W : {H // 2} x {W // 2}" in text and "### Depth decimation : 2 x 2" in text
    full = [S.synth_stream_config(W, H, s) for s in range(N_STREAMS)]
    frames = [([S.synth_depth(W, H, s, seed=S.SEED + 7919 * k) for s in range(N_STREAMS)],
               [S.synth_color(W, H, s, seed=S.SEED + 7919 * k) for s in range(N_STREAMS)]) for k in range(FRAMES)]
    with PcsContext([decimated_stream_config(c, 2) for c in full]) as ctx:
        ctx.set_depth_filter(temporal=True, alpha=0.4, delta=20, persistence=3, hole_fill=1)
        states = [F.State((H // 2, W // 2)) for _ in range(N_STREAMS)]
        for depth, color in frames:
            filtered = ctx.filter_depth(ctx.decimate_depth(2, depth))
            for s in range(N_STREAMS):
                assert np.array_equal(filtered[s], F.filter_frame(D.decimate(depth[s], 2), states[s], hole_fill=1))
        buf, counts, size = ctx.process_frames(filtered, frames[-1][1])
    n = N_STREAMS * (W // 2) * (H // 2)
    assert sum(counts) == n
    want = buf[HEADER_SHORTS:HEADER_SHORTS + 5 * n].reshape(-1, 5)
    got = np.fromfile(out, dtype=np.uint8)[4:].view(np.int16).reshape(-1, 5)
    assert got.shape == want.shape == (n, 5) and np.array_equal(got, want)


@pytest.mark.gpu
def test_scale_one_is_off(tmp_path):
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    with_one, without = str(tmp_path / "one.bin"), str(tmp_path / "none.bin")
    text = edge("-D", "1", "-o", with_one)
    edge("-o", without)
    assert f"### Depth Frames H x W : {H} x {W}" in text and "Depth decimation" not in text
    a, b = np.fromfile(with_one, dtype=np.uint8), np.fromfile(without, dtype=np.uint8)
    assert a.size == 4 + 10 * N_STREAMS * W * H and np.array_equal(a, b)
