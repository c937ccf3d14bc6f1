"""-E (Euclidean cluster filter) of pcs-multicamera-optimized, end to end on the GPU: two edge servers on loopback into the centre
with -E (alone, behind -B, behind -O and -K and in front of -V), the cameras of the node itself with -i -Z -E, each against the
brute-force restatement (tests/np_clusters.py) of what the stage in front of the filter produced — that stage restated by the
existing numpy restatements — the -t line's numbers against the restatement's statistics, and without -E the dump of today. (The
flag surface needs no GPU: tests/test_clusters_cpu.py.)"""
import subprocess

import numpy as np
import pytest

import np_clusters as N
import np_radius_outlier as NR
import np_stat_outlier as NS
from test_wire import CENTRAL, CLI_DIR, EDGE, frame_inputs, free_port, retry_server_start, wait_listening
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, HEADER_SHORTS

pytestmark = pytest.mark.gpu

STAR = (100, 50, 3000)     # tolerance_mm, min_size, max_size for two 64x48 edge payloads: the zero-depth pile (3708 records on one
#                            point) is above max_size, the scatter below min_size
RADIUS = (100, 5)          # the -O in front of it
STAT = (8, 2000, 200)      # ... and the -K
BOX = (-3000, 4000, -2000, 3000, -2000, 3000)   # the -B in front of it (drops the pile: it sits at y = 3416, the camera's origin)
LOCAL = (150, 30, 0)       # ... for three 64x48 cameras of the node with invalid depth dropped


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
    kept, keep, stats = N.cluster_filter(rec, *params)
    assert 0 < keep.sum() < rec.shape[0], "the fixture must have kept and dropped records"
    return kept, stats


def line_of(stats):
    return (f"Cluster filter: {stats['considered']} -> {stats['kept']} points ({stats['clusters']} clusters, {stats['kept_clusters']} kept, "
            f"largest {stats['largest']})")


def option(params):
    return ",".join(str(v) for v in params)


@retry_server_start
def test_star_with_cluster_filter(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    want, stats = filtered(stitched, STAR)
    got, stdout = star_dump(tmp_path, ["-E", option(STAR), "-t"])
    assert got.shape == want.shape and (got == want).all()
    assert line_of(stats) in stdout.splitlines()


@retry_server_start
def test_star_without_the_option_is_unchanged(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    got, stdout = star_dump(tmp_path, ["-t"])
    assert got.shape == stitched.shape and (got == stitched).all() and "Cluster filter" not in stdout


@retry_server_start
def test_star_behind_the_crop_box(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    xyz = stitched[:, :3].astype(np.int64)
    lo, hi = np.array(BOX[0::2]), np.array(BOX[1::2])
    boxed = stitched[((xyz >= lo) & (xyz <= hi)).all(axis=1)]
    assert 0 < boxed.shape[0] < stitched.shape[0]
    params = (STAR[0], STAR[1], 0)
    want, stats = filtered(boxed, params)
    got, stdout = star_dump(tmp_path, ["-B", option(BOX), "-E", option(params[:2]), "-t"])
    assert got.shape == want.shape and (got == want).all()
    assert line_of(stats) in stdout.splitlines()


@pytest.mark.parametrize("timer", [False, True])
@retry_server_start
def test_star_behind_both_outlier_filters_then_voxel_grid(edge_payload, oracle, tmp_path, timer):
    stitched = np.concatenate([edge_payload, edge_payload])
    first = NR.radius_outlier(stitched, *RADIUS)
    second, _, _ = NS.stat_outlier(first, *STAT)
    assert 0 < second.shape[0] < first.shape[0] < stitched.shape[0]
    kept, stats = filtered(second, STAR)
    want = oracle.voxel_grid(kept, 100)
    got, stdout = star_dump(tmp_path, ["-O", option(RADIUS), "-K", option(STAT), "-E", option(STAR), "-V", "100"] + (["-t"] if timer else []))
    assert 0 < want.shape[0] < kept.shape[0]
    assert got.shape == want.shape and (got == want).all()
    assert (line_of(stats) in stdout.splitlines()) == timer


@retry_server_start
def test_star_behind_the_radius_filter_alone(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    first = NR.radius_outlier(stitched, *RADIUS)
    want, stats = filtered(first, STAR)
    got, stdout = star_dump(tmp_path, ["-O", option(RADIUS), "-E", option(STAR), "-t"])
    assert got.shape == want.shape and (got == want).all()
    assert f"Outlier removal: {stitched.shape[0]} -> {first.shape[0]} points" in stdout.splitlines()
    assert line_of(stats) in stdout.splitlines()


@pytest.mark.parametrize("leaf", [0, 100])
def test_local_cameras_with_cluster_filter(oracle, tmp_path, leaf):
    """-i synth: -Z -E [-V]: the restatement applied to what pcs_process_frames_device writes for the same frames."""
    cfgs, depth, color = S.synth_frame_set(3, 64, 48)
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        buf, counts, size = ctx.process_frames(depth, color)
    payload = buf[HEADER_SHORTS:HEADER_SHORTS + size // 2].reshape(-1, 5).copy()
    assert 0 < payload.shape[0] < 3 * 64 * 48
    kept, stats = filtered(payload, LOCAL)
    want = oracle.voxel_grid(kept, leaf) if leaf else kept
    out = str(tmp_path / "dump.bin")
    r = subprocess.run([CENTRAL, "-i", "synth:64x48", "-N", "3", "-Z", "-E", option(LOCAL), "-q", "-r", "1", "-t", "-o", out]
                       + (["-V", str(leaf)] if leaf else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    got = dump(out)
    assert got.shape == want.shape and (got == want).all()
    assert line_of(stats) in r.stdout.splitlines()
    assert "Outlier removal:" not in r.stdout


def test_local_cameras_behind_the_statistical_filter(oracle, tmp_path):
    """-i synth: -Z -K -E: each stage takes the one in front of it by its device count."""
    cfgs, depth, color = S.synth_frame_set(3, 64, 48)
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        buf, counts, size = ctx.process_frames(depth, color)
    payload = buf[HEADER_SHORTS:HEADER_SHORTS + size // 2].reshape(-1, 5).copy()
    first, _, _ = NS.stat_outlier(payload, 8, 1000, 300)
    assert 0 < first.shape[0] < payload.shape[0]
    want, stats = filtered(first, LOCAL)
    out = str(tmp_path / "dump.bin")
    r = subprocess.run([CENTRAL, "-i", "synth:64x48", "-N", "3", "-Z", "-K", "8,1000,300", "-E", option(LOCAL), "-q", "-r", "1", "-t", "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    got = dump(out)
    assert got.shape == want.shape and (got == want).all()
    assert line_of(stats) in r.stdout.splitlines()
