"""Brute-force restatement of DESIGN.md section 3 "Euclidean clusters" (pcs_cluster_filter*, pcs_cluster_labels*): records i and j
are adjacent iff their squared distance, in Python / int64 integers from the sign-extended shorts, is at most tolerance_mm^2; a
cluster is a connected component; size(i) its record count; label(i) its smallest input index; the filter keeps record i iff
min_size <= size(i) and (max_size == 0 or size(i) <= max_size). The adjacency is all pairs, O(n^2), in numpy chunks; the components
come from a plain-Python union-find. Shares nothing with the library: no grid, no cells."""
import numpy as np

CHUNK = 512
INT_MAX = 2 ** 31 - 1


def _xyz(records):
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    return rec, rec[:, :3].astype(np.int64)


def labels(records, tolerance_mm):
    """(labels int32 [n], sizes int32 [n], n_clusters)."""
    assert 1 <= tolerance_mm <= 1000
    rec, xyz = _xyz(records)
    n = rec.shape[0]
    t2 = int(tolerance_mm) ** 2
    parent = list(range(n))

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    for a in range(0, n, CHUNK):
        d = xyz[a:a + CHUNK, None, :] - xyz[None, :, :]
        near = (d * d).sum(axis=2) <= t2
        for row, i in enumerate(range(a, min(a + CHUNK, n))):
            ri = find(i)
            for j in np.nonzero(near[row, :i])[0].tolist():           # every pair once, by its larger index
                rj = find(j)
                if rj != ri:
                    lo, hi = (ri, rj) if ri < rj else (rj, ri)         # the smaller index stays the root
                    parent[hi] = lo
                    ri = lo
    lab = np.array([find(i) for i in range(n)], np.int32).reshape(n)
    sizes = np.bincount(lab, minlength=max(n, 1))[lab].astype(np.int32) if n else np.zeros(0, np.int32)
    return lab, sizes, int((lab == np.arange(n)).sum())


def filter_from_labels(records, lab, sizes, min_size, max_size=0):
    """The size filter over labels() of the same records: (kept records [m, 5] in input order, keep mask [n], statistics dict)."""
    assert 1 <= min_size <= INT_MAX and (max_size == 0 or min_size <= max_size <= INT_MAX)
    rec, _ = _xyz(records)
    keep = (sizes >= min_size).reshape(-1)
    if max_size:
        keep &= sizes <= max_size
    first = lab == np.arange(rec.shape[0])
    stats = {"considered": rec.shape[0], "clusters": int(first.sum()), "kept_clusters": int((first & keep).sum()),
             "largest": int(sizes.max(initial=0)), "kept": int(keep.sum())}
    return rec[keep].copy(), keep, stats


def cluster_filter(records, tolerance_mm, min_size, max_size=0):
    """(kept records [m, 5] in input order, keep mask [n], statistics dict)."""
    lab, sizes, _ = labels(records, tolerance_mm)
    return filter_from_labels(records, lab, sizes, min_size, max_size)
