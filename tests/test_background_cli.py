"""-X (background model and subtraction) of pcs-multicamera-optimized, end to end on the GPU: a .pcsraw of three 64x48 cameras and
four frame-sets — three of the static scene, learned with `-X learn:`, and the same scene with a block of depth pixels of one camera
pulled 500 mm closer, subtracted with `-X FILE` (alone, in front of -E -L, in front of -V) — against the restatement
(tests/np_background.py) of what pcs_process_frames gives for the same frames; two edge servers on loopback into a centre with -X; and
without -X the dump is pcs_stitch_device's bytes. (The flag surface needs no GPU: tests/test_background_cpu.py.)"""
import subprocess

import numpy as np
import pytest

import np_background as N
from test_wire import CENTRAL, CLI_DIR, EDGE, frame_inputs, free_port, retry_server_start, wait_listening
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, HEADER_SHORTS

pytestmark = pytest.mark.gpu

CELL = 40
CLUSTER = (150, 5)      # -E behind the subtraction: tolerance_mm, min_size


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def dump(path):
    raw = np.fromfile(path, dtype=np.uint8)
    assert int.from_bytes(raw[:4].tobytes(), "little") == raw.size - 4
    return raw[4:].view(np.int16).reshape(-1, 5)


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    """(configs, the four frame-sets, their payloads under FLAG_DROP_INVALID, the .pcsraw of all four, the .pcsraw of the fourth)."""
    tmp = tmp_path_factory.mktemp("background_cli")
    cfgs, depth, color = S.synth_frame_set(3, 64, 48)
    rng = np.random.default_rng(31)
    frames = []
    for k in range(3):          # the static scene, with a few millimetres of depth noise from the second frame-set on
        noisy = [np.where(d > 0, d + (rng.integers(-3, 4, d.shape) if k else 0), 0).astype(np.uint16) for d in depth]
        frames.append((noisy, color))
    moved = [d.copy() for d in depth]
    block = moved[1][0:20, 0:24]          # 364 valid pixels of camera 1
    block[block > 600] -= 500
    frames.append((moved, color))
    payloads = []
    with PcsContext(cfgs, flags=FLAG_DROP_INVALID) as ctx:
        for d, c in frames:
            buf, _, size = ctx.process_frames(d, c)
            payloads.append(buf[HEADER_SHORTS:HEADER_SHORTS + size // 2].reshape(-1, 5).copy())
    all_four, fourth = str(tmp / "frames.pcsraw"), str(tmp / "fourth.pcsraw")
    S.write_pcsraw(all_four, cfgs, frames)
    S.write_pcsraw(fourth, cfgs, frames[3:])
    return cfgs, frames, payloads, all_four, fourth


@pytest.fixture(scope="module")
def learned(rig, tmp_path_factory):
    """The model file `-X learn:` writes for the first three frame-sets, and the restatement's model of them."""
    _, _, payloads, all_four, _ = rig
    path = str(tmp_path_factory.mktemp("background_model") / "bg.pcb")
    r = subprocess.run([CENTRAL, "-i", all_four, "-Z", "-X", f"learn:{path},{CELL}", "-r", "3", "-q", "-t"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    return path, N.learned(CELL, 4194304, payloads[:3]), r.stdout


def test_learn_writes_the_restatements_model(learned):
    path, model, stdout = learned
    assert open(path, "rb").read() == model.export()
    assert f"Background learned: 3 frame-sets, {len(model.seen)} cells of {CELL} mm" in stdout.splitlines()
    assert stdout.count("Background learned") == 1 and "Background subtraction" not in stdout


@pytest.mark.parametrize("behind", ["", "cluster", "voxel"])
def test_subtract_the_learned_model(rig, learned, oracle, tmp_path, behind):
    import np_cluster_objects as NO
    _, _, payloads, _, fourth = rig
    path, model, _ = learned
    payload = payloads[3]
    keep = model.subtract_mask(payload, 3, 1)                   # 100 % of three frame-sets
    kept = payload[keep]
    assert 0 < kept.shape[0] < payload.shape[0], "the fixture must have kept and dropped records"
    out, objects = str(tmp_path / "dump.bin"), str(tmp_path / "objects.txt")
    want, extra = kept, []
    if behind == "cluster":
        _, n_objects, object_of = NO.cluster_objects(kept, *CLUSTER)
        want = kept[object_of >= 0]
        assert n_objects >= 1 and 0 < want.shape[0]
        extra = ["-E", "%d,%d" % CLUSTER, "-L", objects]
    elif behind == "voxel":
        want = oracle.voxel_grid(kept, 100)
        assert 0 < want.shape[0] < kept.shape[0]
        extra = ["-V", "100"]
    r = subprocess.run([CENTRAL, "-i", fourth, "-Z", "-X", f"{path},100,1", "-q", "-r", "1", "-t", "-o", out] + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    got = dump(out)
    assert got.shape == want.shape and (got == want).all()
    line = f"Background subtraction: {payload.shape[0]} -> {kept.shape[0]} points ({len(model.seen)} cells, seen >= 3 of 3, dilate 1)"
    assert line in r.stdout.splitlines(), r.stdout
    if behind == "cluster":
        assert f"Objects: {n_objects} ({n_objects} written)" in r.stdout.splitlines()
        assert len(open(objects).read().splitlines()) == 1 + n_objects


def test_defaults_are_fifty_percent_and_dilate_one(rig, learned, tmp_path):
    _, _, payloads, _, fourth = rig
    path, model, _ = learned
    kept = payloads[3][model.subtract_mask(payloads[3], 2, 1)]     # ceil(3 x 50 / 100) = 2
    out = str(tmp_path / "dump.bin")
    r = subprocess.run([CENTRAL, "-i", fourth, "-Z", "-X", path, "-q", "-r", "1", "-t", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    assert (dump(out) == kept).all() and "seen >= 2 of 3, dilate 1)" in r.stdout


def test_an_overflowed_model_ends_the_run_with_status_1(rig, tmp_path):
    path = str(tmp_path / "small.pcb")
    r = subprocess.run([CENTRAL, "-i", rig[3], "-Z", "-X", f"learn:{path},{CELL},64", "-r", "1", "-q", "-t"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=150)
    assert r.returncode == 1 and "max_cells 64" in r.stderr and "Background learned" not in r.stdout
    import os
    assert not os.path.exists(path)


@pytest.fixture(scope="module")
def edge_payload(oracle):
    cfgs, depth, color = frame_inputs(1, 64, 48, 0, single=True)
    cam, _ = oracle.process_frames(cfgs, depth, color)
    return cam


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


@retry_server_start
def test_star_with_background_subtraction(edge_payload, tmp_path):
    """The host-count route: the stitched payload of two edges against a model the restatement wrote (the records left of the middle of
    the cloud, learned twice)."""
    stitched = np.concatenate([edge_payload, edge_payload])
    upper = edge_payload[edge_payload[:, 0] <= int(np.median(edge_payload[:, 0]))]
    model = N.learned(CELL, 65536, [upper, upper])
    path = str(tmp_path / "upper.pcb")
    open(path, "wb").write(model.export())
    keep = model.subtract_mask(stitched, 2, 0)
    assert 0 < keep.sum() < stitched.shape[0]
    got, stdout = star_dump(tmp_path, ["-X", f"{path},100,0", "-t"])
    assert got.shape[0] == keep.sum() and (got == stitched[keep]).all()
    assert (f"Background subtraction: {stitched.shape[0]} -> {int(keep.sum())} points ({len(model.seen)} cells, seen >= 2 of 2, dilate 0)"
            in stdout.splitlines())


@retry_server_start
def test_without_the_option_nothing_changes(edge_payload, tmp_path):
    """No -X: the dump is what pcs_stitch_device writes for the edges' payloads, and no line about the model is printed."""
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
    assert "Background" not in stdout
