"""Clouds for the Euclidean cluster tests, shared by the CPU tier, the GPU tests and the CLI test. Everything is deterministic. A case
is (name, (n, 5) int16 records, (tolerance_mm, min_size, max_size), expected) where `expected` is a dict of what is known WITHOUT
the brute force — any of the statistics words ("clusters", "kept_clusters", "largest", "kept"), "keep" (the mask), "sizes" (the sorted
cluster sizes) — or None where only tests/np_clusters.py says. The colour shorts are random (radius_outlier_cases.with_colour)."""
import functools

import numpy as np

import radius_outlier_cases as RC

COUNTS = (63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
# the random clouds: n records uniform in a cube sized for a mean of RANDOM_DEGREE records within the tolerance of a record — below
# the percolation threshold (about 2.7), so clusters of many sizes occur — and kept from RANDOM_MIN records up
RANDOM_TOL, RANDOM_DEGREE, RANDOM_MIN = 20, 1.8, 3
CHAIN_TOL, CHAIN_N, CHAIN_CUT = 7, 3000, 1234
DUPLICATES = 2049       # no larger: a cell of m members costs m^2 / 2 distance tests by definition, in the library and in the brute force


def shuffled(xyz, seed):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    return xyz[np.random.default_rng(seed).permutation(xyz.shape[0])]


def random_cloud(n):
    side = max(2, int(round((n * 4.0 / 3.0 * np.pi * RANDOM_TOL ** 3 / RANDOM_DEGREE) ** (1.0 / 3.0))))
    return RC.with_colour(np.random.default_rng(1000 + n).integers(-side // 2, side - side // 2, (n, 3)))


def pair(offset):
    return RC.with_colour(np.array([[-3, 40, -2], np.array([-3, 40, -2]) + np.array(offset)]))


def extremes():
    """Pairs 65535 mm apart on one axis, everything else equal: one apart if a difference wrapped at 16 bits."""
    xyz = []
    for axis in range(3):
        a = np.array([5000, -7000, 9000]) + 2500 * axis
        a[axis] = 32767
        b = a.copy()
        b[axis] = -32768
        xyz += [a, b]
    return RC.with_colour(np.array(xyz))


def range_ends():
    """Four clusters, every record within sqrt(3) of its cluster's others: eight records around the origin, on both sides of 0 on all
    three axes (cell flooring of negatives); four on the -32768 face of x; four on the 32767 face of z; two in the (+, +, +) corner."""
    origin = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    low = [(x, y, 77) for x in (-32768, -32767) for y in (100, 101)]
    high = [(-500, y, z) for y in (-32768, -32767) for z in (32766, 32767)]
    corner = [(32767, 32767, 32767), (32766, 32767, 32767)]
    return RC.with_colour(shuffled(origin + low + high + corner, 21))


def chain(cut=None):
    """CHAIN_N records on a zigzag whose links are exactly CHAIN_TOL long ((2, +-3, 6): 4 + 9 + 36 = 49), records two links apart
    at least 12 apart; in shuffled input order. cut: that link is (1, 0, 7) instead, d^2 = 50 = tol^2 + 1."""
    steps = np.tile(np.array([[2, 3, 6], [2, -3, 6]]), (CHAIN_N // 2, 1))[:CHAIN_N - 1]
    if cut is not None:
        steps[cut] = (1, 0, 7)
    xyz = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(steps, axis=0)]) + np.array([-3000, 0, -9000])
    return RC.with_colour(shuffled(xyz, 22))


def bridge(with_bridge):
    """Two 10 x 10 x 10 slabs of pitch 3, 12 apart in x, and (optionally) one record halfway, 6 from a node of either: tolerance 6."""
    g = 3 * np.indices((10, 10, 10)).reshape(3, -1).T
    parts = [g + np.array([-100, 50, -20]), g + np.array([-100 + 27 + 12, 50, -20])]
    if with_bridge:
        parts.append(np.array([[-100 + 27 + 6, 50 + 12, -20 + 15]]))
    return RC.with_colour(shuffled(np.concatenate(parts), 23))


def lattice(pitch):
    return RC.with_colour(shuffled(pitch * np.indices((16, 16, 16)).reshape(3, -1).T + np.array([-70, 32767 - 15 * pitch, -32768]), 24))


def sizes_cloud():
    """Clusters of 1 .. 70 records (lines of pitch 2 along x, tolerance 2), 100 apart, the records interleaved: 2485 records.
    Returns (records, the size of every record's cluster)."""
    xyz, size = [], []
    for k in range(1, 71):
        xyz += [(2 * j - 60, 100 * k - 3500, -100 * k + 3000) for j in range(k)]
        size += [k] * k
    order = np.random.default_rng(25).permutation(len(size))
    return RC.with_colour(np.array(xyz)[order]), np.array(size)[order]


def duplicates():
    return RC.with_colour(np.concatenate([np.tile(np.array([[-7, 1234, -32768]]), (DUPLICATES, 1)), np.array([[-7, 1234, -32700]])]))


@functools.lru_cache(maxsize=None)
def random_cases():
    """The random clouds: (name, records, params)."""
    return tuple((f"count{n}", random_cloud(n), (RANDOM_TOL, RANDOM_MIN, 0)) for n in COUNTS)


@functools.lru_cache(maxsize=None)
def cases():
    out = [("count0", np.zeros((0, 5), np.int16), (20, 1, 0), {"clusters": 0, "kept": 0, "largest": 0, "kept_clusters": 0}),
           ("count1", random_cloud(1), (20, 1, 0), {"clusters": 1, "kept": 1, "largest": 1, "kept_clusters": 1}),
           ("count1_min2", random_cloud(1), (20, 2, 0), {"clusters": 1, "kept": 0, "largest": 1, "kept_clusters": 0})]
    joined = {"clusters": 1, "kept": 2, "largest": 2, "kept_clusters": 1}
    apart = {"clusters": 2, "kept": 0, "largest": 1, "kept_clusters": 0}
    for tol, inside, outside in ((5, (3, 4, 0), (5, 1, 0)), (1, (0, -1, 0), (1, 0, 1)), (1000, (-600, 0, 800), (1000, 0, -1))):
        out.append((f"pair_t{tol}_in", pair(inside), (tol, 2, 0), joined))
        out.append((f"pair_t{tol}_out", pair(outside), (tol, 2, 0), apart))
    out.append(("pair_equal", pair((0, 0, 0)), (1, 2, 2), joined))
    for tol in (1, 1000):
        out.append((f"extremes_t{tol}", extremes(), (tol, 2, 0), {"clusters": 6, "kept": 0, "largest": 1, "sizes": [1] * 6}))
    for tol in (2, 7):
        out.append((f"range_ends_t{tol}", range_ends(), (tol, 4, 4), {"clusters": 4, "kept": 8, "largest": 8, "kept_clusters": 2,
                                                                     "sizes": [2, 4, 4, 8]}))
    out.append(("chain", chain(), (CHAIN_TOL, 1, 0), {"clusters": 1, "kept": CHAIN_N, "largest": CHAIN_N}))
    long_part = max(CHAIN_CUT + 1, CHAIN_N - CHAIN_CUT - 1)
    out.append(("chain_cut", chain(CHAIN_CUT), (CHAIN_TOL, CHAIN_N // 2, 0),
                {"clusters": 2, "kept": long_part, "largest": long_part, "kept_clusters": 1, "sizes": sorted([CHAIN_CUT + 1, CHAIN_N - CHAIN_CUT - 1])}))
    out.append(("bridge", bridge(True), (6, 1500, 0), {"clusters": 1, "kept": 2001, "largest": 2001}))
    out.append(("bridge_gone", bridge(False), (6, 1500, 0), {"clusters": 2, "kept": 0, "largest": 1000, "sizes": [1000, 1000]}))
    out.append(("lattice_joined", lattice(10), (10, 4096, 4096), {"clusters": 1, "kept": 4096, "largest": 4096}))
    out.append(("lattice_apart", lattice(11), (10, 1, 1), {"clusters": 4096, "kept": 4096, "largest": 1, "kept_clusters": 4096}))
    rec, size = sizes_cloud()
    for lo, hi in ((33, 64), (64, 0), (65, 0)):
        keep = (size >= lo) & ((size <= hi) if hi else True)
        out.append((f"sizes_{lo}_{hi}", rec, (2, lo, hi), {"clusters": 70, "largest": 70, "keep": keep, "kept": int(keep.sum()),
                                                          "kept_clusters": (hi or 70) - lo + 1, "sizes": list(range(1, 71))}))
    out.append(("duplicates", duplicates(), (1, 2, 0), {"clusters": 2, "kept": DUPLICATES, "largest": DUPLICATES, "kept_clusters": 1,
                                                        "keep": np.arange(DUPLICATES + 1) < DUPLICATES}))
    out += [(name, rec, params, None) for name, rec, params in random_cases()]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute-force restatement of a case, computed once per process and shared (read-only):
    (kept records, keep mask, stats, labels, sizes)."""
    import np_clusters as N
    _, rec, params, _ = next(c for c in cases() if c[0] == name)
    lab, sizes, _ = N.labels(rec, params[0])
    out, keep, stats = N.filter_from_labels(rec, lab, sizes, params[1], params[2])
    for a in (out, keep, lab, sizes):
        a.setflags(write=False)
    return out, keep, stats, lab, sizes


def check_expected(name, keep, stats, lab):
    """The analytic expectations of a case against a result."""
    expected = next(c for c in cases() if c[0] == name)[3] or {}
    for key, value in expected.items():
        if key == "keep":
            assert (keep == value).all(), name
        elif key == "sizes":
            counts = np.bincount(lab, minlength=1)
            assert sorted(counts[counts > 0].tolist()) == sorted(value), name
        else:
            assert stats[key] == value, (name, key, stats[key], value)
