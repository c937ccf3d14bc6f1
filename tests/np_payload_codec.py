"""The "PCZ1" payload container in numpy: encoder, decoder and validator written from DESIGN.md section 4 (the format's text), not
from the C++. The GPU encoder is held to encode()'s bytes, the GPU decoder to the payload, the C validator to validate()'s verdicts.

    0  uint32 magic = 0x315A4350    4  uint32 n_points    8  uint32 n_blocks = ceil(n / 64)    12  uint32 total_bytes
   16  uint32 block_end[n_blocks]   then the blocks
   block = 16-byte header (v0 of x y z: uint16; v0 of R G B P: uint8; uint32 widths; 2 zero bytes) + 7 bit strings
"""
import numpy as np

MAGIC = 0x315A4350
BLOCK = 64
BITS = (16, 16, 16, 8, 8, 8, 8)          # x y z R G B P
WIDTH_SHIFT = (0, 5, 10, 15, 19, 23, 27)
WIDTH_FIELD = (5, 5, 5, 4, 4, 4, 4)
INT32_MAX = 2 ** 31 - 1


class Malformed(ValueError):
    pass


def bound(n):
    return 16 + 660 * ((n + BLOCK - 1) // BLOCK)


def channels(records):
    """(n, 5) int16 / uint16 records -> (7, n) int64 channels."""
    s = np.asarray(records).reshape(-1, 5).view(np.uint16).astype(np.int64)
    return np.stack([s[:, 0], s[:, 1], s[:, 2], s[:, 3] & 0xFF, s[:, 3] >> 8, s[:, 4] & 0xFF, s[:, 4] >> 8])


def records_of(ch):
    """(7, n) channels -> (n, 5) int16 records."""
    out = np.empty((ch.shape[1], 5), dtype=np.uint16)
    out[:, 0], out[:, 1], out[:, 2] = ch[0], ch[1], ch[2]
    out[:, 3] = ch[3] | (ch[4] << 8)
    out[:, 4] = ch[5] | (ch[6] << 8)
    return out.view(np.int16)


def _zigzag(v, k):
    """Residuals of one channel of one block: z_0 = 0, z_i = zigzag((v_i - v_{i-1}) mod 2^k read as signed)."""
    z = np.zeros(len(v), dtype=np.int64)
    d = (v[1:] - v[:-1]) % (1 << k)
    s = np.where(d >= (1 << (k - 1)), d - (1 << k), d)
    z[1:] = np.where(s >= 0, 2 * s, -2 * s - 1)
    return z


def _pack(z, w):
    """z_i at bits [i w, (i + 1) w) of a string of ceil(m w / 32) uint32 words, bit j = bit j % 32 of word j / 32."""
    m = len(z)
    words = (m * w + 31) // 32
    if words == 0:
        return np.zeros(0, dtype=np.uint32)
    bits = np.zeros(words * 32, dtype=np.uint8)
    bits[:m * w] = ((z[:, None] >> np.arange(w)) & 1).reshape(-1)
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u4")


def _unpack(words, m, w):
    if w == 0:
        return np.zeros(m, dtype=np.int64)
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    z = bits[:m * w].reshape(m, w).astype(np.int64)
    return (z << np.arange(w)).sum(axis=1)


def encode_block(ch):
    """(7, m) channels of one block -> bytes."""
    m = ch.shape[1]
    head = np.zeros(16, dtype=np.uint8)
    head[0:6] = ch[0:3, 0].astype("<u2").view(np.uint8)
    head[6:10] = ch[3:7, 0].astype(np.uint8)
    widths, strings = 0, []
    for k in range(7):
        z = _zigzag(ch[k], BITS[k])
        w = int(np.bitwise_or.reduce(z)).bit_length()
        widths |= w << WIDTH_SHIFT[k]
        strings.append(_pack(z, w).tobytes())
    head[10:14] = np.array([widths], dtype="<u4").view(np.uint8)
    return head.tobytes() + b"".join(strings)


def encode(records):
    """(n, 5) int16 records (or a flat int16 array of 5 n) -> the container's bytes."""
    ch = channels(records)
    n = ch.shape[1]
    nb = (n + BLOCK - 1) // BLOCK
    blocks = [encode_block(ch[:, b * BLOCK:min(n, (b + 1) * BLOCK)]) for b in range(nb)]
    ends, pos = [], 16 + 4 * nb
    for blk in blocks:
        pos += len(blk)
        ends.append(pos)
    head = np.array([MAGIC, n, nb, pos] + ends, dtype="<u4").tobytes()
    out = head + b"".join(blocks)
    assert len(out) == pos and pos % 4 == 0 and pos <= bound(n)
    return out


def validate(buf):
    """Everything a decoder relies on; returns (n_points, n_blocks, total_bytes, data_offset) or raises Malformed."""
    buf = bytes(buf)
    if len(buf) < 16:
        raise Malformed("shorter than the header")
    magic, n, nb, total = (int(v) for v in np.frombuffer(buf, dtype="<u4", count=4))
    if magic != MAGIC:
        raise Malformed("magic")
    if n > INT32_MAX // 10:
        raise Malformed("n_points too large")
    if nb != (n + BLOCK - 1) // BLOCK:
        raise Malformed("n_blocks")
    if total != len(buf) or total % 4:
        raise Malformed("total_bytes")
    data = 16 + 4 * nb
    if data > len(buf):
        raise Malformed("table does not fit")
    ends = np.frombuffer(buf, dtype="<u4", count=nb, offset=16).astype(np.int64)
    start = data
    for b in range(nb):
        end = int(ends[b])
        if end > total:
            raise Malformed("block_end past the end")
        if end <= start:
            raise Malformed("table not increasing")
        if end - start < 16:
            raise Malformed("block shorter than its header")
        word = int.from_bytes(buf[start + 10:start + 14], "little")
        m = BLOCK if b + 1 < nb else n - BLOCK * (nb - 1)
        size = 16
        for k in range(7):
            w = (word >> WIDTH_SHIFT[k]) & ((1 << WIDTH_FIELD[k]) - 1)
            if w > BITS[k]:
                raise Malformed("width")
            size += 4 * ((m * w + 31) // 32)
        if word >> 31 or buf[start + 14] or buf[start + 15]:
            raise Malformed("reserved bits")
        if end - start != size:
            raise Malformed("block size disagrees with its widths")
        start = end
    if start != total:
        raise Malformed("blocks do not end at total_bytes")
    return n, nb, total, data


def decode(buf):
    """Container bytes -> (n, 5) int16 records. Validates first."""
    buf = bytes(buf)
    n, nb, _, data = validate(buf)
    ends = np.frombuffer(buf, dtype="<u4", count=nb, offset=16).astype(np.int64)
    ch = np.zeros((7, n), dtype=np.int64)
    start = data
    for b in range(nb):
        m = BLOCK if b + 1 < nb else n - BLOCK * (nb - 1)
        v0 = list(np.frombuffer(buf, dtype="<u2", count=3, offset=start).astype(np.int64)) + list(buf[start + 6:start + 10])
        word = int.from_bytes(buf[start + 10:start + 14], "little")
        pos = start + 16
        for k in range(7):
            w = (word >> WIDTH_SHIFT[k]) & ((1 << WIDTH_FIELD[k]) - 1)
            nw = (m * w + 31) // 32
            z = _unpack(np.frombuffer(buf, dtype="<u4", count=nw, offset=pos), m, w)
            pos += 4 * nw
            s = (z >> 1) ^ -(z & 1)
            s[0] = 0
            ch[k, b * BLOCK:b * BLOCK + m] = (int(v0[k]) + np.cumsum(s)) % (1 << BITS[k])
        start = int(ends[b])
    return records_of(ch)
