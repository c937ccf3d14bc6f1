"""-O (radius outlier removal) of pcs-multicamera-optimized, end to end on the GPU: two edge servers on loopback into the centre with
-O (alone, behind -B, in front of -V), the cameras of the node itself with -i -Z -O, all against the brute-force restatement
(tests/np_radius_outlier.py) of what the stage in front of the filter produced; and without -O the dump is pcs_stitch_device's bytes.
(The flag surface needs no GPU: tests/test_radius_outlier_cpu.py.)"""
import subprocess

import numpy as np
import pytest

import np_radius_outlier as N
from test_wire import CENTRAL, CLI_DIR, EDGE, frame_inputs, free_port, retry_server_start, wait_listening
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, HEADER_SHORTS

pytestmark = pytest.mark.gpu

STAR = (100, 5)         # radius_mm, min_neighbors for two 64x48 edge payloads (dense: their zero-depth pixels sit on one point)
LOCAL = (200, 5)        # ... for three 64x48 cameras of the node with invalid depth dropped
# everything but the plane y = 3416 the edges' zero-depth pixels land on
BOX = "-32768,32767,-32768,3415,-32768,32767"


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


def filtered(rec, r, k):
    mask = N.keep_mask(rec, r, k)
    assert 0 < mask.sum() < rec.shape[0], "the fixture must have kept and dropped records"
    return rec[mask]


@retry_server_start
def test_star_with_outlier_removal(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    want = filtered(stitched, *STAR)
    got, stdout = star_dump(tmp_path, ["-O", "%d,%d" % STAR, "-t"])
    assert got.shape == want.shape and (got == want).all()
    assert f"Outlier removal: {stitched.shape[0]} -> {want.shape[0]} points" in stdout.splitlines()


@retry_server_start
def test_star_with_crop_box_then_outlier_removal(edge_payload, tmp_path):
    cropped = edge_payload[edge_payload[:, 1] <= 3415]
    assert 0 < cropped.shape[0] < edge_payload.shape[0]
    want = filtered(np.concatenate([cropped, cropped]), *STAR)
    got, _ = star_dump(tmp_path, ["-B", BOX, "-O", "%d,%d" % STAR])
    assert got.shape == want.shape and (got == want).all()


@pytest.mark.parametrize("timer", [False, True])
@retry_server_start
def test_star_with_outlier_removal_then_voxel_grid(edge_payload, oracle, tmp_path, timer):
    stitched = np.concatenate([edge_payload, edge_payload])
    kept = filtered(stitched, *STAR)
    want = oracle.voxel_grid(kept, 100)
    got, stdout = star_dump(tmp_path, ["-O", "%d,%d" % STAR, "-V", "100"] + (["-t"] if timer else []))
    assert 0 < want.shape[0] < kept.shape[0]
    assert got.shape == want.shape and (got == want).all()
    assert (f"Outlier removal: {stitched.shape[0]} -> {kept.shape[0]} points" in stdout.splitlines()) == timer


@pytest.mark.parametrize("leaf", [0, 100])
def test_local_cameras_with_outlier_removal(oracle, tmp_path, leaf):
    """-i synth: -Z -O [-V]: the restatement applied to what pcs_process_frames_device writes for the same frames."""
    cfgs, depth, color = S.synth_frame_set(3, 64, 48)
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        buf, counts, size = ctx.process_frames(depth, color)
    payload = buf[HEADER_SHORTS:HEADER_SHORTS + size // 2].reshape(-1, 5).copy()
    assert 0 < payload.shape[0] < 3 * 64 * 48
    kept = filtered(payload, *LOCAL)
    want = oracle.voxel_grid(kept, leaf) if leaf else kept
    out = str(tmp_path / "dump.bin")
    r = subprocess.run([CENTRAL, "-i", "synth:64x48", "-N", "3", "-Z", "-O", "%d,%d" % LOCAL, "-q", "-r", "1", "-t", "-o", out]
                       + (["-V", str(leaf)] if leaf else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    got = dump(out)
    assert got.shape == want.shape and (got == want).all()
    assert f"Outlier removal: {payload.shape[0]} -> {kept.shape[0]} points" in r.stdout.splitlines()


@retry_server_start
def test_without_the_option_nothing_changes(edge_payload, tmp_path):
    """No -O: the dump is what pcs_stitch_device writes for the edges' payloads, and no line about the filter is printed."""
    n = edge_payload.shape[0]
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs) as ctx:
        d_cam, d_out = ctx.device_malloc(10 * n), ctx.device_malloc(20 * n + 64)
        ctx.memcpy_h2d(d_cam, np.ascontiguousarray(edge_payload))
        total = ctx.stitch_device([d_cam, d_cam], [n, n], 1, d_out, 10 * n)
        ctx.synchronize()
        want = np.empty((total, 5), np.int16)
        ctx.memcpy_d2h(want, d_out)
        ctx.device_free(d_cam); ctx.device_free(d_out)
    assert total == 2 * n
    got, stdout = star_dump(tmp_path, ["-t"])
    assert got.tobytes() == want.tobytes()
    assert "Outlier" not in stdout
