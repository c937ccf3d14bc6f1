"""Radius outlier removal (include/pcs_hip.h) restated as brute force: every pair, in int64, in chunks of 1024
rows. Nothing cleverer — this is what the kernels, the C ABI and the CLI are held to, byte for byte."""
import numpy as np

CHUNK = 1024


def keep_mask(records, radius_mm, min_neighbors):
    """records: (n, 5) int16. True where record i has at least min_neighbors records j != i with squared distance <= radius_mm^2."""
    assert 1 <= radius_mm <= 1000 and 1 <= min_neighbors <= 255
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    p = rec[:, :3].astype(np.int64)
    n = p.shape[0]
    keep = np.zeros(n, bool)
    r2 = int(radius_mm) ** 2
    for a in range(0, n, CHUNK):
        d = p[a:a + CHUNK, None] - p[None]
        within = ((d * d).sum(axis=2) <= r2).sum(axis=1) - 1        # (minus the record itself: j != i is by index)
        keep[a:a + CHUNK] = within >= min_neighbors
    return keep


def radius_outlier(records, radius_mm, min_neighbors):
    """The kept records, input order, all five shorts unchanged."""
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    return rec[keep_mask(rec, radius_mm, min_neighbors)].copy()
