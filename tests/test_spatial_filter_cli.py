"""pcs-camera-optimized -S on the GPU: a four-frame .pcsraw through `-S 0.5:20:2:2 -F temporal=0.4:20:3,holes` dumps what the
library calls give for the last frame of the same sequence (spatial filter, then the temporal state carried over all four frames,
then the stitch), and something else than the run without -S."""
import os
import subprocess

import numpy as np
import pytest

import np_depth_filter as F
import np_spatial_filter as SP
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import HEADER_SHORTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
EDGE = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-camera-optimized")


def dump_records(path):
    return np.fromfile(path, dtype=np.uint8)[4:].view(np.int16).reshape(-1, 5)


@pytest.mark.gpu
def test_edge_cli_filters_spatially_like_the_library(tmp_path):
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    w, h = 64, 48
    cfgs = [S.synth_stream_config(w, h, 0, single=True)]
    frames = [([SP.scene(w, h, 40 + k)], [S.synth_color(w, h, 0, seed=S.SEED + k)]) for k in range(4)]
    raw, out, plain = str(tmp_path / "frames.pcsraw"), str(tmp_path / "dump.bin"), str(tmp_path / "plain.bin")
    S.write_pcsraw(raw, cfgs, frames)
    for extra, path in ((["-S", "0.5:20:2:2"], out), ([], plain)):
        r = subprocess.run([EDGE, "-f", raw, "-m", "-r", "4", *extra, "-F", "temporal=0.4:20:3,holes", "-o", path],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "### Total Frames = 4" in r.stdout
    with PcsContext(cfgs) as ctx:
        ctx.set_depth_filter(temporal=True, alpha=0.4, delta=20, persistence=3, hole_fill=1)
        state = F.State((h, w))
        for depth, color in frames:
            smoothed = ctx.spatial_filter_depth(depth, alpha=0.5, delta=20, iterations=2, hole_radius=2)
            assert np.array_equal(smoothed[0], SP.spatial_filter(depth[0], alpha=0.5, delta=20, iterations=2, hole_radius=2)[0])
            filtered = ctx.filter_depth(smoothed)
            assert np.array_equal(filtered[0], F.filter_frame(smoothed[0], state, hole_fill=1))
        buf, counts, size = ctx.process_frames(filtered, frames[3][1])
        want = buf[HEADER_SHORTS:HEADER_SHORTS + 5 * sum(counts)].reshape(-1, 5)
    got = dump_records(out)
    assert got.shape == want.shape == (w * h, 5) and np.array_equal(got, want)
    assert not np.array_equal(got, dump_records(plain))                       # -S mattered
