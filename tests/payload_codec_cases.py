"""Payloads for the PCZ1 codec tests: the content classes and record counts the CPU and GPU tests share. Everything is
deterministic; a case is (name, (n, 5) int16 records)."""
import numpy as np

# blocks the encoder's offsets kernel scans per pass of its one workgroup (csrc/pcs_device.h: kCodecScanBlocks)
SCAN_BLOCKS = 1024
COUNTS = (0, 1, 2, 63, 64, 65, 127, 129, 255, 256, 257, 4099)
# one pass, one more block, and a partial one
N_PAST_SCAN = 64 * SCAN_BLOCKS + 64 + 5


def _records(x, y, z, r, g, b, p):
    """Seven channel arrays -> (n, 5) int16 records."""
    u = lambda a, m: np.asarray(a, np.int64) & m                                   # noqa: E731
    out = np.empty((len(x), 5), np.uint16)
    out[:, 0], out[:, 1], out[:, 2] = u(x, 0xFFFF), u(y, 0xFFFF), u(z, 0xFFFF)
    out[:, 3] = u(r, 0xFF) | (u(g, 0xFF) << 8)
    out[:, 4] = u(b, 0xFF) | (u(p, 0xFF) << 8)
    return out.view(np.int16)


def equal(n):
    one = np.array([[1234, -5, 30000, 0x4321, 0x0065]], np.int16)
    return np.repeat(one, n, axis=0)


def ramp(n):
    i = np.arange(n)
    return _records(i, 3 * i - 700, 40000 - 2 * i, i, 255 - i, 5 * i, 0 * i)


def alternating(n):
    """v alternates 0 / 0x8000 (k = 16) and 0 / 0x80 (k = 8): every residual is -2^(k-1), every width maximal."""
    a = np.arange(n) & 1
    return _records(a * 0x8000, a * 0x8000, a * 0x8000, a * 0x80, a * 0x80, a * 0x80, a * 0x80)


def int16_wrap(n):
    a = np.arange(n) & 1
    v = np.where(a == 1, 32767, -32768)
    return _records(v, -v - 1, v, 0 * a, 255 * a, 0 * a, 0 * a)


def nonzero_p(n):
    i = np.arange(n)
    return _records(i, i, i, i, i, i, 7 * i + 1)


def outlier(n, at):
    """All records equal but record `at` of every block."""
    rec = equal(n).copy()
    idx = np.arange(at, n, 64)
    rec[idx] = np.array([-32768, 32767, 1, -1, 0x00FF], np.int16)
    return rec


def block_jump(n):
    """A jump exactly between two blocks: it must cost nothing (every width 0)."""
    blk = np.arange(n) // 64
    return _records(blk * 12345, blk * -321, blk * 77, blk * 9, blk * 13, blk * 101, blk * 0)


def uniform(n, seed=20240917):
    return np.random.default_rng(seed + n).integers(-32768, 32768, (n, 5)).astype(np.int16)


CLASSES = {
    "equal": equal, "ramp": ramp, "alternating": alternating, "int16_wrap": int16_wrap, "nonzero_p": nonzero_p,
    "outlier0": lambda n: outlier(n, 0), "outlier1": lambda n: outlier(n, 1), "outlier62": lambda n: outlier(n, 62),
    "outlier63": lambda n: outlier(n, 63), "block_jump": block_jump, "uniform": uniform,
}
