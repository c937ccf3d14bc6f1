"""numpy restatement of the depth pre-filter ("Depth pre-filter"), written from that text and from nothing
else: the temporal stage, the fill from left (vectorised, and as the plain loop the text describes), and the per-tile counts the
filter hands to pcs_process_frames_device_counted. The GPU kernels (csrc/pcs_kernels_filter.hip) are held to this bit for bit.

Not a test module: the depth-filter tests import it."""
import numpy as np

TILE_POINTS = 2048

# persistence 0..8 -> (M, L): "valid in M of the last L frames". 0 never fills, 8 always does.
PERSISTENCE = [(9, 8), (8, 8), (2, 3), (2, 4), (2, 8), (1, 2), (1, 5), (1, 8), (0, 8)]

_POPCOUNT8 = np.array([bin(v).count("1") for v in range(256)], np.int32)


class State:
    """One stream's temporal state: `last` uint16 and `hist` uint8 per pixel, all zero after set or reset."""

    def __init__(self, shape):
        self.last = np.zeros(shape, np.uint16)
        self.hist = np.zeros(shape, np.uint8)

    def reset(self):
        self.last[...] = 0
        self.hist[...] = 0


def temporal(c, state, alpha=0.4, delta=20, persistence=3):
    """The temporal stage on one raster; advances `state` by one frame and returns the stage's output."""
    c = np.asarray(c, np.uint16)
    a = np.float32(alpha)
    oma = np.float32(1.0) - a                    # fp32, computed once
    m_need, l_span = PERSISTENCE[persistence]
    p, h = state.last, state.hist.astype(np.int32)
    ci, pi = c.astype(np.int32), p.astype(np.int32)
    valid = c != 0
    agree = valid & (p != 0) & (np.abs(ci - pi) < int(delta))
    f = (a * c.astype(np.float32)).astype(np.float32) + (oma * p.astype(np.float32)).astype(np.float32)     # two products, one sum
    r = np.minimum(f.astype(np.float32).astype(np.int32), 65535)                                              # the cast truncates
    seen = _POPCOUNT8[h & ((1 << l_span) - 1)]
    persist = (p != 0) & (seen >= m_need)
    out = np.where(agree, r, np.where(valid, ci, np.where(persist, pi, 0)))
    new_last = np.where(agree, r, np.where(valid, ci, pi))
    new_hist = np.where(agree, ((h << 1) | 1) & 0xFF, np.where(valid, 1, (h << 1) & 0xFF))
    state.last = new_last.astype(np.uint16)
    state.hist = new_hist.astype(np.uint8)
    return out.astype(np.uint16)


def fill_left(d):
    """Fill from left, vectorised: a zero pixel takes the nearest non-zero pixel to its left in its row; none: it stays 0."""
    d = np.asarray(d, np.uint16)
    cols = np.arange(d.shape[1], dtype=np.int64)[None, :]
    src = np.maximum.accumulate(np.where(d != 0, cols, -1), axis=1)         # column of the nearest non-zero at or left of each pixel
    filled = np.take_along_axis(d, np.maximum(src, 0), axis=1)
    return np.where(src >= 0, filled, 0).astype(np.uint16)


def fill_left_loop(d):
    """The same as the text says it, pixel by pixel."""
    d = np.asarray(d, np.uint16)
    out = d.copy()
    for r in range(d.shape[0]):
        run = 0
        for x in range(d.shape[1]):
            if out[r, x] == 0:
                out[r, x] = run
            else:
                run = out[r, x]
    return out


def filter_frame(c, state, temporal_on=True, alpha=0.4, delta=20, persistence=3, hole_fill=0):
    """One raster through the configured stages (temporal first, then the fill; the state sees the temporal stage alone)."""
    out = temporal(c, state, alpha, delta, persistence) if temporal_on else np.asarray(c, np.uint16).copy()
    return fill_left(out) if hole_fill else out


def tile_counts(rasters):
    """Non-zero pixels per TILE_POINTS tile, streams in order, every stream's tiles row-major and its last one short."""
    parts = []
    for d in rasters:
        flat = (np.asarray(d).reshape(-1) != 0)
        n_tiles = (flat.size + TILE_POINTS - 1) // TILE_POINTS
        padded = np.zeros(n_tiles * TILE_POINTS, bool)
        padded[:flat.size] = flat
        parts.append(padded.reshape(n_tiles, TILE_POINTS).sum(axis=1))
    return np.concatenate(parts).astype(np.uint32)
