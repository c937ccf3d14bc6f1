"""pcs-camera-optimized -F on the GPU: a four-frame .pcsraw through `-F temporal=0.4:20:3,holes` dumps what the library gives for the
last frame of the same sequence (filter state carried over all four frames, then the stitch)."""
import os
import subprocess

import numpy as np
import pytest

import np_depth_filter as F
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import HEADER_SHORTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
EDGE = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-camera-optimized")


@pytest.mark.gpu
def test_edge_cli_filters_like_the_library(tmp_path):
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    w, h = 64, 48
    cfgs = [S.synth_stream_config(w, h, 0, single=True)]
    frames = [([S.synth_depth(w, h, 0, seed=S.SEED + k)], [S.synth_color(w, h, 0, seed=S.SEED + k)]) for k in range(4)]
    raw, out = str(tmp_path / "frames.pcsraw"), str(tmp_path / "dump.bin")
    S.write_pcsraw(raw, cfgs, frames)
    r = subprocess.run([EDGE, "-f", raw, "-m", "-r", "4", "-F", "temporal=0.4:20:3,holes", "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "### Total Frames = 4" in r.stdout
    with PcsContext(cfgs) as ctx:
        ctx.set_depth_filter(temporal=True, alpha=0.4, delta=20, persistence=3, hole_fill=1)
        state = F.State((h, w))
        for depth, color in frames:
            filtered = ctx.filter_depth(depth)
            assert np.array_equal(filtered[0], F.filter_frame(depth[0], state, hole_fill=1))
        buf, counts, size = ctx.process_frames(filtered, frames[3][1])
        want = buf[HEADER_SHORTS:HEADER_SHORTS + 5 * sum(counts)].reshape(-1, 5)
        unfiltered, _, _ = ctx.process_frames(frames[3][0], frames[3][1])
    got = np.fromfile(out, dtype=np.uint8)[4:].view(np.int16).reshape(-1, 5)
    assert got.shape == want.shape == (w * h, 5) and np.array_equal(got, want)
    assert not np.array_equal(want, unfiltered[HEADER_SHORTS:HEADER_SHORTS + 5 * w * h].reshape(-1, 5))      # the filter mattered
