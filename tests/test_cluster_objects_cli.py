"""-L (the object table of the -E stage) of pcs-multicamera-optimized, end to end on the GPU: two edge servers on loopback into the
centre with -E -L (alone, behind -O and -K and in front of -V), the cameras of the node itself with -i -Z -K -E -L: the file against
the restatement (tests/np_cluster_objects.py) of what the stage in front of the filter produced, the dump byte for byte what -E alone
gives, the `Objects:` line, a table smaller than the object count, and without -L no line and no file. (The flag surface needs no
GPU: tests/test_cluster_objects_cpu.py.)"""
import os
import subprocess

import numpy as np
import pytest

import np_cluster_objects as NO
import np_clusters as N
import np_radius_outlier as NR
import np_stat_outlier as NS
from test_wire import CENTRAL, CLI_DIR, EDGE, frame_inputs, free_port, retry_server_start, wait_listening
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, HEADER_SHORTS

pytestmark = pytest.mark.gpu

STAR = (100, 50, 3000)     # tests/test_clusters_cli.py's: the zero-depth pile is above max_size, the scatter below min_size
RADIUS = (100, 5)
STAT = (8, 2000, 200)
LOCAL = (150, 30, 0)
HEADER = "# k label size lo_x lo_y lo_z hi_x hi_y hi_z sum_x sum_y sum_z sum_r sum_g sum_b"


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


def star_dump(tmp_path, extra, name="dump.bin"):
    """Two pull-mode edges (the same camera twice) into a centre that dumps its one frame-set; returns (records, stdout)."""
    out = str(tmp_path / name)
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


def option(params):
    return ",".join(str(v) for v in params)


def lines_of(table, written=None):
    """The file's lines for the first `written` objects of a restated table."""
    out = [HEADER]
    for k, o in enumerate(table[:written]):
        values = [k, o["label"], o["size"], *o["lo"], *o["hi"], *o["sum_xyz"], *o["sum_rgb"]]
        out.append(" ".join(str(int(v)) for v in values))
    return out


def read_lines(path):
    with open(path) as f:
        text = f.read()
    assert text.endswith("\n")
    return text[:-1].split("\n")


@retry_server_start
def test_star_with_the_object_table(edge_payload, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    table, n_objects, _ = NO.cluster_objects(stitched, *STAR)
    assert n_objects == 4 and sorted(table["size"].tolist()) == [94, 94, 134, 256]
    path = str(tmp_path / "objects.txt")
    got, stdout = star_dump(tmp_path, ["-E", option(STAR), "-L", path, "-t"])
    alone, alone_stdout = star_dump(tmp_path, ["-E", option(STAR), "-t"], name="alone.bin")
    assert got.tobytes() == alone.tobytes() and got.shape[0] == int(table["size"].sum())
    assert read_lines(path) == lines_of(table)
    lines = stdout.splitlines()
    assert "Objects: 4 (4 written)" in lines and lines[lines.index("Objects: 4 (4 written)") - 1].startswith("Cluster filter: ")
    assert "Objects:" not in alone_stdout


@retry_server_start
def test_star_behind_both_outlier_filters_then_voxel_grid(edge_payload, oracle, tmp_path):
    stitched = np.concatenate([edge_payload, edge_payload])
    first = NR.radius_outlier(stitched, *RADIUS)
    second, _, _ = NS.stat_outlier(first, *STAT)
    assert 0 < second.shape[0] < first.shape[0] < stitched.shape[0]
    table, n_objects, _ = NO.cluster_objects(second, *STAR)
    kept, _, _ = N.cluster_filter(second, *STAR)
    want = oracle.voxel_grid(kept, 100)
    assert n_objects > 0 and 0 < want.shape[0] < kept.shape[0]
    path = str(tmp_path / "objects.txt")
    got, stdout = star_dump(tmp_path, ["-O", option(RADIUS), "-K", option(STAT), "-E", option(STAR), "-L", path, "-V", "100", "-t"])
    assert got.shape == want.shape and (got == want).all()
    assert read_lines(path) == lines_of(table)
    assert f"Objects: {n_objects} ({n_objects} written)" in stdout.splitlines()


def local_payload():
    cfgs, depth, color = S.synth_frame_set(3, 64, 48)
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        buf, counts, size = ctx.process_frames(depth, color)
    return buf[HEADER_SHORTS:HEADER_SHORTS + size // 2].reshape(-1, 5).copy()


def test_local_cameras_behind_the_statistical_filter(tmp_path):
    """-i synth: -Z -K -E -L: the counted route; the expectation is the restatement of what -K produced."""
    payload = local_payload()
    assert NO.cluster_objects(payload, *LOCAL)[1] == 13
    first, _, _ = NS.stat_outlier(payload, 8, 1000, 300)
    assert 0 < first.shape[0] < payload.shape[0]
    table, n_objects, _ = NO.cluster_objects(first, *LOCAL)
    want, _, _ = N.cluster_filter(first, *LOCAL)
    assert n_objects > 1
    out, path = str(tmp_path / "dump.bin"), str(tmp_path / "objects.txt")
    r = subprocess.run([CENTRAL, "-i", "synth:64x48", "-N", "3", "-Z", "-K", "8,1000,300", "-E", option(LOCAL), "-L", path, "-q", "-r", "1",
                        "-t", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    got = dump(out)
    assert got.shape == want.shape and (got == want).all()
    assert read_lines(path) == lines_of(table)
    assert f"Objects: {n_objects} ({n_objects} written)" in r.stdout.splitlines()


def test_a_table_of_two_and_no_option(tmp_path):
    payload = local_payload()
    table, n_objects, _ = NO.cluster_objects(payload, *LOCAL)
    assert n_objects == 13
    out, path = str(tmp_path / "dump.bin"), str(tmp_path / "objects.txt")
    base = [CENTRAL, "-i", "synth:64x48", "-N", "3", "-Z", "-E", option(LOCAL), "-q", "-r", "1", "-t", "-o", out]
    r = subprocess.run(base + ["-L", path + ",2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    assert read_lines(path) == lines_of(table, 2) and len(read_lines(path)) == 3
    assert "Objects: 13 (2 written)" in r.stdout.splitlines()
    with_table = dump(out)
    # - is stdout
    r = subprocess.run(base + ["-L", "-,2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-3:] == lines_of(table, 2)
    # without -L: no line, no file, the same dump
    os.remove(path)
    r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    assert "Objects:" not in r.stdout and not os.path.exists(path) and os.listdir(str(tmp_path)) == ["dump.bin"]
    assert dump(out).tobytes() == with_table.tobytes()
