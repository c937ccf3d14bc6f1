"""-B (crop box) of pcs-multicamera-optimized and pcs-camera-optimized: the flag surface without a GPU (help text, every malformed
form refused with status 2 before a context is created), and on the GPU the dumps against the library's result for the same box."""
import os
import subprocess

import numpy as np
import pytest

import test_wire as W
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import HEADER_SHORTS, TRANSFORMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
CENTRAL = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-multicamera-optimized")
EDGE = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-camera-optimized")
BOX_A = ((-1100, 0, -1100), (1100, 2000, 300))
ARG_A = "-1100,1100,0,2000,-1100,300"


@pytest.fixture(scope="module")
def clis():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert os.path.exists(CENTRAL) and os.path.exists(EDGE)
    return CENTRAL, EDGE


def run(*args, timeout=120):
    return subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_help_lists_the_crop_box_flag(clis):
    for prog in clis:
        r = run(prog, "-h")
        assert r.returncode == 0
        assert "-B <xlo,xhi,ylo,yhi,zlo,zhi>" in r.stdout


MALFORMED = ["", "1,2,3", "1,2,3,4,5", "1,2,3,4,5,6,7", "1,2,3,4,5,x", "1,2,3,4,5,6x", "1;2;3;4;5;6", "0,1,0,1,0,32768", "-32769,1,0,1,0,1",
             "5,1,0,1,0,1", "0,1,3,2,0,1", "0,1,0,1,1,0", "0.5,1,0,1,0,1", "99999999999999999999,1,0,1,0,1"]


@pytest.mark.parametrize("arg", MALFORMED)
def test_malformed_box_exits_2_before_any_context(clis, arg):
    central, edge = clis
    for cmd in ([central, "-i", "synth:64x48", "-N", "2", "-q", "-r", "1", "-B", arg],
                [central, "-c", "127.0.0.1:1", "-q", "-B", arg],
                [edge, "-f", "synth:64x48", "-m", "-r", "1", "-B", arg]):
        r = run(*cmd)
        assert r.returncode == 2, (cmd, r.stderr)
        assert "-B" in r.stderr and "pcs_create" not in r.stderr and "Connection failed" not in r.stderr


def test_box_with_sharding_or_without_simd_arithmetic_is_refused_in_one_line(clis):
    central, edge = clis
    r = run(central, "-i", "synth:64x48", "-N", "2", "-q", "-G", "2", "-B", ARG_A)
    assert r.returncode == 2 and "-G" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = run(edge, "-f", "synth:64x48", "-r", "1", "-B", ARG_A)       # no -m: the reference's default loop has no crop
    assert r.returncode == 2 and "-m" in r.stderr and "pcs_create" not in r.stderr


def _library_result(voxel_leaf=0):
    cfgs, depth, color = S.synth_frame_set(3, 640, 480)
    with PcsContext(cfgs) as ctx:
        ctx.set_crop_box_mm(*BOX_A)
        buf, counts, size = ctx.process_frames(depth, color)
        cloud = buf[HEADER_SHORTS:HEADER_SHORTS + 5 * sum(counts)].reshape(-1, 5).copy()
        if not voxel_leaf:
            return cloud
        n_max = sum(c.n_points for c in cfgs)
        dd = [ctx.device_malloc(d.nbytes) for d in depth]
        dc = [ctx.device_malloc(c.nbytes) for c in color]
        for p, a in zip(dd + dc, depth + color):
            ctx.memcpy_h2d(p, a)
        d_vox, d_nv = ctx.device_malloc(n_max * 10 + 64), ctx.device_malloc(4)
        ctx.process_frames_voxel_device(dd, dc, voxel_leaf, d_vox, n_max * 5, d_nv)
        ctx.synchronize()
        nv = np.empty(1, np.int32)
        ctx.memcpy_d2h(nv, d_nv)
        vox = np.empty(5 * int(nv[0]), np.int16)
        ctx.memcpy_d2h(vox, d_vox)
        return vox.reshape(-1, 5)


def _dump(path, header_required=True):
    raw = np.fromfile(path, dtype=np.uint8)
    size = int.from_bytes(raw[:4].tobytes(), "little")
    if header_required:
        assert size == raw.size - 4
    return raw[4:].view(np.int16).reshape(-1, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("leaf", [0, 50])
def test_central_cli_crops_like_the_library(clis, oracle, tmp_path, leaf):
    out = str(tmp_path / "dump.bin")
    r = run(clis[0], "-i", "synth:640x480", "-N", "3", "-B", ARG_A, "-q", "-r", "1", "-o", out, *(["-V", str(leaf)] if leaf else []))
    assert r.returncode == 0, r.stderr
    want = _library_result(leaf)
    got = _dump(out)
    assert 0 < want.shape[0] < 3 * 640 * 480
    assert got.shape == want.shape and (got == want).all()
    if leaf:        # the library's one-call route and the CLI's two-call route, both against the oracle's voxel grid of the cropped cloud
        ref = oracle.voxel_grid(_library_result(0), leaf)
        assert got.shape == ref.shape and (got == ref).all()


@pytest.mark.gpu
def test_edge_cli_crops_like_the_library(clis, tmp_path):
    out = str(tmp_path / "dump.bin")
    r = run(clis[1], "-f", "synth:640x480", "-m", "-n", "3", "-r", "1", "-B", ARG_A, "-o", out)
    assert r.returncode == 0, r.stderr
    want = _library_result()
    got = _dump(out, header_required=False)          # (the header is only written under -s)
    assert got.shape == want.shape and (got == want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("transform,stride", [(False, 1), (False, 2), (True, 1), (True, 2)])
@W.retry_server_start
def test_star_with_the_centre_side_crop(clis, oracle, tmp_path, transform, stride):
    """`pcs-multicamera-optimized -c <edges> -B <box> [-T transforms.txt] [-d n]`: legacy edge servers cannot crop, so the centre does
    (pcs_crop_payloads_device) — after -T where both are given, -d the stride over the kept records of each camera. Against the
    oracle's payloads masked with numpy; the box runs from the 25th to the 75th percentile of the uncropped cloud's own columns, so
    the kept share is strictly between 0 and 1 by construction."""
    cfgs, depth, color = W.frame_inputs(1, 128, 96, 0, single=True)
    cam, _ = oracle.process_frames(cfgs, depth, color)
    cams = [oracle.transform_payload(cam, TRANSFORMS[i], 1) if transform else cam for i in range(2)]      # both edges: the same config
    xyz = np.concatenate(cams)[:, :3].astype(np.int32)
    lo, hi = np.percentile(xyz, 25, axis=0).astype(np.int32), np.percentile(xyz, 75, axis=0).astype(np.int32)
    kept = [c[((c[:, :3] >= lo) & (c[:, :3] <= hi)).all(axis=1)] for c in cams]
    want = np.concatenate([k[::stride] for k in kept])
    assert 0 < sum(k.shape[0] for k in kept) < 2 * cam.shape[0] and all(k.shape[0] for k in kept)
    args = ["-B", ",".join(str(int(v)) for a in range(3) for v in (lo[a], hi[a])), "-d", str(stride)]
    if transform:
        tf = tmp_path / "transforms.txt"
        tf.write_text("\n".join(" ".join(repr(float(v)) for v in np.asarray(TRANSFORMS[i], np.float32).reshape(-1)) for i in range(2)) + "\n")
        args += ["-T", str(tf)]
    p1, p2, p3 = W.free_port(), W.free_port(), W.free_port()
    edges = [subprocess.Popen([clis[1], "-f", "synth:128x96", "-m", "-r", "2", "-p", str(p), "-P"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for p in (p1, p2)]
    central = None
    try:
        W.wait_listening([p1, p2], procs=edges)
        central = subprocess.Popen([clis[0], "-c", f"127.0.0.1:{p1},127.0.0.1:{p2}", "-p", str(p3), "-r", "1"] + args,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        consumer = W.connect(p3, procs=[central] + edges)
        consumer.sendall(b"Z")
        got = W.read_frame(consumer)
        consumer.close()
        assert got.shape == want.shape and (got == want).all()
        _, err = central.communicate(timeout=60)
        assert central.returncode == 0, err
    finally:
        for p in edges + ([central] if central else []):
            if p.poll() is None:
                p.kill()
