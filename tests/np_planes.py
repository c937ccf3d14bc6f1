"""Brute-force restatement of DESIGN.md section 3 "Plane segmentation" (pcs_plane_segment*, pcs_plane_labels*,
pcs_plane_count_inliers_device, pcs_plane_from_points): the hash, the draws, N, off and the threshold in Python integers
(math.isqrt), the inlier dots in int64 numpy (they stay below 2^53). Shares nothing with the library: no tiles, no compaction — a
round's cloud is a boolean index into the input."""
import math

import numpy as np

MASK = (1 << 64) - 1
MODEL_WORDS = ("nx", "ny", "nz", "off", "threshold", "inliers")
STATS_FIELDS = ("considered", "planes", "inliers_total", "kept", "largest_plane", "degenerate_hypotheses")
ZERO_MODEL = {"nx": 0, "ny": 0, "nz": 0, "off": 0, "threshold": 0, "inliers": 0, "sample": (0, 0, 0), "hypothesis": 0}


def splitmix64(key):
    z = (key + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, r, h, k, m):
    """Position k (0..2) of hypothesis h of round r among m records."""
    key = (seed << 32) | (r << 20) | (h << 2) | k
    return ((splitmix64(key) >> 32) * m) >> 32


def plane(p0, p1, p2, distance_mm):
    """(nx, ny, nz, off, T) of three records (sequences of ints), or None for a degenerate triple."""
    a = [int(p1[k]) - int(p0[k]) for k in range(3)]
    b = [int(p2[k]) - int(p0[k]) for k in range(3)]
    n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    if n == (0, 0, 0):
        return None
    off = sum(n[k] * int(p0[k]) for k in range(3))
    return n + (off, math.isqrt(int(distance_mm) ** 2 * sum(v * v for v in n)))


def inliers(xyz, eq):
    """The mask of |N . p - off| <= T over int64 [m, 3]."""
    nx, ny, nz, off, t = eq
    assert max(abs(nx), abs(ny), abs(nz)) <= 1 << 34 and abs(off) <= 1 << 52 and 0 <= t <= 1 << 52
    d = xyz[:, 0] * np.int64(nx) + xyz[:, 1] * np.int64(ny) + xyz[:, 2] * np.int64(nz) - np.int64(off)
    return np.abs(d) <= np.int64(t)


def count_inliers(records, eqs):
    xyz = np.asarray(records, np.int16).reshape(-1, 5)[:, :3].astype(np.int64)
    return np.array([int(inliers(xyz, eq).sum()) for eq in eqs], np.int64)


def round_scores(cloud, distance_mm, iterations, seed, r):
    """Every hypothesis of round r over int64 [m, 3] (m >= 3): a list of (score, eq or None, positions, mask or None)."""
    m = cloud.shape[0]
    out = []
    for h in range(iterations):
        at = [draw(seed, r, h, k, m) for k in range(3)]
        eq = plane(cloud[at[0]], cloud[at[1]], cloud[at[2]], distance_mm)
        mask = inliers(cloud, eq) if eq is not None else None
        out.append((int(mask.sum()) if eq is not None else 0, eq, at, mask))
    return out


def segment(records, distance_mm, iterations, min_inliers=3, max_planes=1, seed=1, mode=0):
    """(labels int32 [n], n_planes, models: max_planes dicts, stats dict, kept records [k, 5] in input order)."""
    assert 1 <= distance_mm <= 1000 and 1 <= iterations <= 4096 and min_inliers >= 3 and 1 <= max_planes <= 8
    assert 0 <= seed < 1 << 32 and mode in (0, 1)
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    xyz = rec[:, :3].astype(np.int64)
    n = rec.shape[0]
    labels = np.full(n, -1, np.int32)
    models, degenerate = [], 0
    for r in range(max_planes):
        origin = np.nonzero(labels < 0)[0]           # the round's cloud, input order
        m = origin.shape[0]
        if m < 3:
            break
        cloud = xyz[origin]
        best = None
        for h, (score, eq, at, mask) in enumerate(round_scores(cloud, distance_mm, iterations, seed, r)):
            if eq is None:
                degenerate += 1
            elif best is None or score > best[0]:    # h ascends: a tie keeps the smaller h
                best = (score, h, eq, at, mask)
        if best is None or best[0] < min_inliers:
            break
        score, h, eq, at, mask = best
        labels[origin[mask]] = r
        models.append(dict(zip(MODEL_WORDS, eq + (score,)), sample=tuple(int(origin[a]) for a in at), hypothesis=h))
    n_planes = len(models)
    total = sum(mod["inliers"] for mod in models)
    keep = labels >= 0 if mode else labels < 0
    stats = {"considered": n, "planes": n_planes, "inliers_total": total, "kept": int(keep.sum()),
             "largest_plane": max((mod["inliers"] for mod in models), default=0), "degenerate_hypotheses": degenerate}
    assert stats["kept"] == (total if mode else n - total)
    return labels, n_planes, models + [dict(ZERO_MODEL)] * (max_planes - n_planes), stats, rec[keep]
