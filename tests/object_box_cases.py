"""The clouds of the object-box tests (tests/test_object_boxes_cpu.py without a GPU, tests/test_object_boxes.py with one): per case
the packed records, object_of, n_objects, max_objects and whether its axes can be compared with eigh's (a case built to be
degenerate compares sums, rank, extents and the invariants alone). The smallest shapes at which each mechanism can go wrong."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "rec object_of n_objects max_objects axes")
CORNER = (-32768, -32768, 32767)


def with_colour(xyz, seed=5):
    """int [n,3] -> int16 [n,5] with colour shorts that no box may depend on (the high byte of short 4 set)."""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    assert xyz.min(initial=0) >= -32768 and xyz.max(initial=0) <= 32767
    rng = np.random.default_rng(seed)
    rec = np.empty((xyz.shape[0], 5), np.int16)
    rec[:, :3] = xyz
    rec[:, 3:] = rng.integers(-32768, 32768, (xyz.shape[0], 2))
    return rec


def rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def lattice(size_mm, pitch=20):
    """The points of a box of size_mm at `pitch`, centred on the origin, float64 [n,3]."""
    ax = [np.arange(0, s + 1, pitch) - s / 2 for s in size_mm]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


LATTICES = ((400, 200, 100), (900, 300, 60), (120, 80, 40))
ROTATIONS = (rot(2, 30), rot(0, 20) @ rot(2, 30), rot(1, -73) @ rot(0, 47) @ rot(2, 30))


def one(xyz, axes=True):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return Case(with_colour(xyz), np.zeros(xyz.shape[0], np.int32), 1, 4, axes)


def blob(n, seed, centre=(0, 0, 0), scale=(900, 300, 80), turn=None):
    """n records of an elongated cloud: well-separated spreads, rotated, rounded to millimetres."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)) * np.array(scale)
    r = ROTATIONS[seed % 3] if turn is None else turn
    return np.rint(p @ r.T + np.array(centre)).astype(np.int64)


def rotated():
    """Nine objects: every lattice under every rotation, each about its own centre, the records in a shuffled order."""
    parts, ids = [], []
    for li, size in enumerate(LATTICES):
        for ri, r in enumerate(ROTATIONS):
            centre = np.array([(li - 1) * 9000 + 300, (ri - 1) * 7000 - 200, 1500 * (li + ri) - 4000])
            parts.append(np.rint(lattice(size) @ r.T + centre))
            ids.append(np.full(parts[-1].shape[0], 3 * li + ri, np.int32))
    xyz, obj = np.concatenate(parts), np.concatenate(ids)
    order = np.random.default_rng(9).permutation(xyz.shape[0])
    return Case(with_colour(xyz[order]), obj[order], 9, 16, True)


def dominant():
    """One object of 9 000 records with 200 records of 7 others scattered through it: the held path and the grouped path."""
    big = blob(9000, 3, (1000, -2000, 500), (2500, 700, 150))
    small = [blob(200 // 7 + (k < 200 % 7), 10 + k, (8000 + 900 * k, 3000 - 700 * k, -2500 + 400 * k), (300, 90, 25)) for k in range(7)]
    xyz = np.concatenate([big] + small)
    obj = np.concatenate([np.zeros(9000, np.int32)] + [np.full(s.shape[0], k + 1, np.int32) for k, s in enumerate(small)])
    assert xyz.shape[0] == 9200
    rng = np.random.default_rng(4)
    where = np.sort(rng.choice(9200, 200, replace=False))
    order = np.empty(9200, np.int64)
    mask = np.zeros(9200, bool)
    mask[where] = True
    order[~mask], order[mask] = np.arange(9000), 9000 + rng.permutation(200)
    xyz, obj = xyz[order], obj[order]
    assert obj[0] == 0                                    # (the first record's object is the one a wave holds)
    return Case(with_colour(xyz), obj, 8, 8, True)


def ignored():
    """object_of of -1, of max_objects and beyond, *n_objects above max_objects, and an entry with no member (k = 2)."""
    parts = [blob(70, 1, (0, 0, 0)), blob(90, 2, (5000, 0, 0)), blob(60, 3, (0, 5000, 0)), blob(50, 4, (0, 0, 3000)), blob(40, 5, (-5000, 0, 0))]
    ids = [0, 1, 3, 4, 5]
    xyz = np.concatenate(parts)
    obj = np.concatenate([np.full(p.shape[0], k, np.int32) for p, k in zip(parts, ids)])
    obj[::7] = -1
    obj[3::11] = 4          # == max_objects
    obj[5::13] = 1 << 20
    obj[6::17] = -(1 << 31)
    order = np.random.default_rng(8).permutation(xyz.shape[0])
    return Case(with_colour(xyz[order]), obj[order], 9, 4, True)


def build():
    c = {}
    c["one_record"] = one([[7, -9, 1200]], axes=False)
    for n in (2, 5):
        c[f"corner_{n}"] = one([CORNER] * n, axes=False)
    for n in (64, 65, 256, 257, 2049):
        c[f"count_{n}"] = one(blob(n, n, (-20000, 15000, 9000)))
    a, b = blob(300, 1, (-3000, 0, 0)), blob(300, 2, (4000, 1000, -500))
    xyz = np.empty((600, 3), np.int64)
    xyz[0::2], xyz[1::2] = a, b
    c["alternating"] = Case(with_colour(xyz), np.tile(np.array([0, 1], np.int32), 300), 2, 2, True)
    pairs = np.concatenate([np.array([[100 * k, 40 * k - 700, 3 * k], [100 * k + 30 + k, 40 * k - 690, 3 * k + 7]]) for k in range(33)])
    c["pairs_33"] = Case(with_colour(pairs), np.repeat(np.arange(33, dtype=np.int32), 2), 33, 64, False)
    c["dominant"] = dominant()
    c["rotated"] = rotated()
    g = lattice((400, 200, 100)) + np.array([1000, -700, 2300])
    c["aligned"] = one(g)
    c["point_x50"] = one([[123, -456, 789]] * 50, axes=False)
    c["line"] = one([[10 * t - 300, 20 * t + 5, -30 * t + 1000] for t in range(40)], axes=False)
    c["grid_plane"] = one([[20 * i, 20 * j - 300, 1500] for i in range(20) for j in range(30)], axes=False)
    c["cube"] = one(lattice((200, 200, 200)) + np.array([0, 0, 2000]), axes=False)
    c["ignored"] = ignored()
    c["none_found"] = Case(with_colour(blob(100, 1)), np.zeros(100, np.int32), 0, 4, False)
    c["negative_count"] = Case(with_colour(blob(100, 1)), np.zeros(100, np.int32), -3, 4, False)
    c["no_table"] = Case(with_colour(blob(100, 1)), np.zeros(100, np.int32), 2, 0, False)
    c["no_records"] = Case(np.zeros((0, 5), np.int16), np.zeros(0, np.int32), 3, 4, False)
    return c


CASES = build()
# the cases whose axes the tests hold to eigh's: none of their objects may be near an eigenvalue crossing
AXES_CASES = sorted(name for name, case in CASES.items() if case.axes)
