"""Radius outlier removal (include/pcs_hip.h) restated as brute force: every pair, in int64, in chunks of 1024
rows. Nothing cleverer — this is what the kernels, the C ABI and the CLI are held to, byte for byte.
keep_mask_dense_box states the same rule a third time, for clouds of a million records in a small box, where the pair loop cannot go."""
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


DENSE_BOX_CELLS = 2 ** 25


def keep_mask_dense_box(records, radius_mm, min_neighbors):
    """The definition a third time, for clouds in a small box: an int32 array of how many records sit on each integer point of the
    bounding box (padded by the radius on every side), the sum of its copies shifted by every integer offset of squared length
    <= radius_mm^2 — the number of records within the radius of each point, multiplicities and all — minus one for the record itself,
    compared with min_neighbors at each record's own point. No cells, no hashing, no pairs. The padded box holds at most
    DENSE_BOX_CELLS points: asserted, not waited for."""
    assert 1 <= radius_mm <= 1000 and 1 <= min_neighbors <= 255
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    if rec.shape[0] == 0:
        return np.zeros(0, bool)
    r = int(radius_mm)
    p = rec[:, :3].astype(np.int64)
    lo = p.min(axis=0) - r
    extent = p.max(axis=0) + r - lo + 1
    assert int(extent[0]) * int(extent[1]) * int(extent[2]) <= DENSE_BOX_CELLS, ("the padded box is too large", tuple(extent))
    at = tuple((p - lo).T)
    occupancy = np.zeros(tuple(extent), np.int32)
    np.add.at(occupancy, at, 1)
    within = np.zeros_like(occupancy)
    inner = tuple(slice(r, int(e) - r) for e in extent)         # the unpadded box: every shift of it stays inside the array
    span = np.arange(-r, r + 1)
    for dx in span:
        for dy in span:
            for dz in span:
                if dx * dx + dy * dy + dz * dz <= r * r:
                    shifted = tuple(slice(s.start + d, s.stop + d) for s, d in zip(inner, (dx, dy, dz)))
                    within[inner] += occupancy[shifted]
    return within[at] - 1 >= min_neighbors
