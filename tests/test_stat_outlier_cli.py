"""-K (statistical outlier removal) of pcs-multicamera-optimized, end to end on the GPU: two edge servers on loopback into the centre
with -K (alone, behind -O, in front of -V), the cameras of the node itself with -i -Z -K, each against the brute-force restatement
(tests/np_stat_outlier.py) of what the stage in front of the filter produced, the -t line's numbers against the restatement's
statistics. (The flag surface needs no GPU: tests/test_stat_outlier_cpu.py.)"""
import subprocess

import numpy as np
import pytest

import np_radius_outlier as NR
import np_stat_outlier as N
from test_wire import CENTRAL, CLI_DIR, EDGE, frame_inputs, free_port, retry_server_start, wait_listening
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, HEADER_SHORTS

pytestmark = pytest.mark.gpu

STAR = (8, 2000, 200)      # mean_k, std_mul_milli, max_dist_mm for two 64x48 edge payloads (dense: the zero-depth pixels sit on one point)
RADIUS = (100, 5)          # the -O in front of it
LOCAL = (8, 1000, 300)     # ... for three 64x48 cameras of the node with invalid depth dropped


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


@pytest.fixture(scope="module")
def edge_payload(oracle):
    cfgs, depth, color = frame_inputs(1, 64, 48, 0, single=True)
    cam, _ = oracle.process_frames(cfgs, depth, color)
    return cam


def dump(path):
    raw = np.fromfile(path, dtype=np.uint8)
    assert int.from_bytes(raw[:4].tobytes(), "little") == raw.size - 4
    return raw[4:].view(np.int16).reshape(-1, 5)


def star_dump(tmp_path, extra):
    """Two pull-mode edges (the same camera twice) into a centre that dumps its one frame-set; returns (records, stdout)."""
    out = str(tmp_path / "dump.bin")
    p1, p2 = free_port(), free_port()
    edges = [subprocess.Popen([EDGE, "-f", "synth:64x48", "-m", "-r", "2", "-p", str(p), "-P"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for p in (p1, p2)]
    central = None
    try:
        wait_listening([p1, p2], procs=edges)
        central = subprocess.Popen([CENTRAL, "-c", f"127.0.0.1:{p1},127.0.0.1:{p2}", "-q", "-r", "1", "-o", out] + extra,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        stdout, err = central.communicate(timeout=150)
        assert central.returncode == 0, err
        return dump(out), stdout
    finally:
        for p in edges + ([central] if central else []):
            if p.poll() is None:
                p.kill()


def filtered(rec, params):
    kept, keep, stats = N.stat_outlier(rec, *params)
    assert 0 < keep.sum() < rec.shape[0], "the fixture must have kept and dropped records"
    return kept, stats


def line_of(stats):
    return (f"Statistical outlier removal: {stats['considered']} -> {stats['kept']} points (dense {stats['dense']}, threshold "
            f"{stats['threshold']}/256 per k)")


@retry_server_start
def test_star_with_stat_outlier_removal(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    want, stats = filtered(stitched, STAR)
    got, stdout = star_dump(tmp_path, ["-K", "%d,%d,%d" % STAR, "-t"])
    assert got.shape == want.shape and (got == want).all()
    assert line_of(stats) in stdout.splitlines()


@retry_server_start
def test_star_behind_radius_outlier_removal(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    first = NR.radius_outlier(stitched, *RADIUS)
    assert 0 < first.shape[0] < stitched.shape[0]
    want, stats = filtered(first, STAR)
    got, stdout = star_dump(tmp_path, ["-O", "%d,%d" % RADIUS, "-K", "%d,%d,%d" % STAR, "-t"])
    assert got.shape == want.shape and (got == want).all()
    assert f"Outlier removal: {stitched.shape[0]} -> {first.shape[0]} points" in stdout.splitlines()
    assert line_of(stats) in stdout.splitlines()


@pytest.mark.parametrize("timer", [False, True])
@retry_server_start
def test_star_with_stat_outlier_removal_then_voxel_grid(edge_payload, oracle, tmp_path, timer):
    stitched = np.concatenate([edge_payload, edge_payload])
    kept, stats = filtered(stitched, STAR)
    want = oracle.voxel_grid(kept, 100)
    got, stdout = star_dump(tmp_path, ["-K", "%d,%d,%d" % STAR, "-V", "100"] + (["-t"] if timer else []))
    assert 0 < want.shape[0] < kept.shape[0]
    assert got.shape == want.shape and (got == want).all()
    assert (line_of(stats) in stdout.splitlines()) == timer


@pytest.mark.parametrize("leaf", [0, 100])
def test_local_cameras_with_stat_outlier_removal(oracle, tmp_path, leaf):
    """-i synth: -Z -K [-V]: the restatement applied to what pcs_process_frames_device writes for the same frames."""
    cfgs, depth, color = S.synth_frame_set(3, 64, 48)
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        buf, counts, size = ctx.process_frames(depth, color)
    payload = buf[HEADER_SHORTS:HEADER_SHORTS + size // 2].reshape(-1, 5).copy()
    assert 0 < payload.shape[0] < 3 * 64 * 48
    kept, stats = filtered(payload, LOCAL)
    want = oracle.voxel_grid(kept, leaf) if leaf else kept
    out = str(tmp_path / "dump.bin")
    r = subprocess.run([CENTRAL, "-i", "synth:64x48", "-N", "3", "-Z", "-K", "%d,%d,%d" % LOCAL, "-q", "-r", "1", "-t", "-o", out]
                       + (["-V", str(leaf)] if leaf else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    got = dump(out)
    assert got.shape == want.shape and (got == want).all()
    assert line_of(stats) in r.stdout.splitlines()
    assert "Outlier removal:" not in r.stdout.replace("Statistical outlier removal:", "")
