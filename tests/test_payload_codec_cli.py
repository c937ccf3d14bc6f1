"""-z end to end: pcs-camera-optimized -z dumps a PCZ1 container that numpy decodes to the oracle's payload, the loopback
star of tests/test_wire.py serves the same cloud with -z on every hop as without, and a centre with -z refuses a raw edge with the
validator's words."""
import struct
import subprocess

import numpy as np
import pytest

import np_payload_codec as N
from test_wire import CENTRAL, CLI_DIR, EDGE, connect, frame_inputs, free_port, read_frame, retry_server_start, wait_listening

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def test_edge_dump_decodes_to_the_oracle_payload(oracle, tmp_path):
    out = str(tmp_path / "dump.bin")
    r = subprocess.run([EDGE, "-f", "synth:64x48", "-m", "-n", "2", "-r", "2", "-z", "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint8).tobytes()
    (size,) = struct.unpack("<i", raw[:4])
    assert size == len(raw) - 4
    cfgs, depth, color = frame_inputs(2, 64, 48, 1, single=False)          # the last of the two frames
    want, _ = oracle.process_frames(cfgs, depth, color)
    got = N.decode(raw[4:])
    assert got.shape == want.shape and (got == want).all()
    assert raw[4:] == N.encode(want)
    # the summary reports container bytes
    assert "### Sending Compressed Stream" in r.stdout and "### AVG Compression Ratio" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("### AVG Bytes/Frame:")]
    assert len(line) == 1
    assert 0 < size < want.nbytes                                           # (the synthetic scene does compress)
    last = [ln for ln in r.stdout.splitlines() if "Buffer size:" in ln][-1]
    assert abs(float(last.split("Buffer size:")[1].split()[0]) - size / (1 << 20)) < 1e-3 * max(1.0, size / (1 << 20))


def run_star(z):
    """Two pull-mode edges and a centre on loopback; returns the two clouds the consumer was served."""
    p1, p2, p3 = free_port(), free_port(), free_port()
    flag = ["-z"] if z else []
    edges = [subprocess.Popen([EDGE, "-f", "synth:128x96", "-m", "-r", "4", "-p", str(p), "-P"] + flag,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for p in (p1, p2)]
    central = None
    try:
        wait_listening([p1, p2], procs=edges)
        central = subprocess.Popen([CENTRAL, "-c", f"127.0.0.1:{p1},127.0.0.1:{p2}", "-d", "2", "-p", str(p3), "-r", "2"] + flag,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        consumer = connect(p3, procs=[central] + edges)
        clouds = []
        for _ in range(2):
            consumer.sendall(b"Z")
            clouds.append(read_frame(consumer))
        consumer.close()
        _, err = central.communicate(timeout=60)
        assert central.returncode == 0, err
        for e in edges:
            e.communicate(timeout=60)
            assert e.returncode == 0
        return clouds
    finally:
        for p in edges + ([central] if central else []):
            if p.poll() is None:
                p.kill()


@retry_server_start
def test_star_serves_the_same_cloud_with_and_without_z(oracle):
    plain, packed = run_star(False), run_star(True)
    for frame in range(2):
        assert plain[frame].shape == packed[frame].shape and (plain[frame] == packed[frame]).all()
        cfgs, depth, color = frame_inputs(1, 128, 96, frame, single=True)
        cam, _ = oracle.process_frames(cfgs, depth, color)
        want = oracle.stitch([cam, cam], 2)
        assert packed[frame].shape == want.shape and (packed[frame] == want).all()


@retry_server_start
def test_centre_with_z_refuses_a_raw_edge():
    p1, p3 = free_port(), free_port()
    edge = subprocess.Popen([EDGE, "-f", "synth:64x48", "-m", "-r", "4", "-p", str(p1), "-P"],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    central = None
    try:
        wait_listening([p1], procs=[edge])
        central = subprocess.Popen([CENTRAL, "-c", f"127.0.0.1:{p1}", "-N", "1", "-p", str(p3), "-r", "1", "-q", "-z"],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        _, err = central.communicate(timeout=150)
        assert central.returncode == 1, err
        assert "magic" in err and "PCZ1" in err            # the validator's message
    finally:
        for p in [edge] + ([central] if central else []):
            if p.poll() is None:
                p.kill()
