"""Clouds for the radius outlier removal tests, shared by the CPU tier, the GPU tests and the CLI test. Everything is deterministic.
A case is (name, (n, 5) int16 records, radius_mm, min_neighbors, expected) where `expected` is the keep mask known WITHOUT the brute
force (None where only tests/np_radius_outlier.py says). The colour shorts are random; the high byte of short 4 is never zero (the
filter copies all ten bytes of a record).
tiled_cubes and lattice_box are the clouds of working size (two and one million records): they are not in cases(), whose brute force
must stay affordable, and return their expectation with the records."""
import itertools
import functools

import numpy as np


def with_colour(xyz, seed=99):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    assert xyz.min(initial=0) >= -32768 and xyz.max(initial=0) <= 32767
    rng = np.random.default_rng(seed + xyz.shape[0])
    rec = np.empty((xyz.shape[0], 5), np.uint16)
    rec[:, :3] = xyz & 0xFFFF
    rec[:, 3] = rng.integers(0, 65536, xyz.shape[0])
    rec[:, 4] = rng.integers(0, 256, xyz.shape[0]) | (rng.integers(1, 256, xyz.shape[0]) << 8)
    return rec.view(np.int16)


def cube(side, seed, n=6161):
    return with_colour(np.random.default_rng(seed).integers(-side // 2, side // 2, (n, 3)))


# (side, radius, min_neighbors, seed, kept share in percent by the brute-force restatement): 6161 = 3 x 2048 + 17
CUBES = ((400, 20, 3, 1, 58.3), (400, 20, 1, 1, 95.0), (400, 20, 8, 1, 1.3), (64, 1, 1, 3, 15.8))
FULL_RANGE = (4097, 2, 1000, 1, 6.2)        # n, seed, radius, min_neighbors, share: many distinct cells, every sign combination
COUNTS = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049)
# The clouds of working size (tests/test_radius_outlier_scale.py); none of them is in cases(): their expectations need no pair loop.
# (copies per axis, pitch, records, kept share in percent at CUBES[0]'s (20, 3): the small cloud's, copy by copy)
TILED = (7, 427, 7 ** 3 * 6161, 58.3)         # 1 231 713 records kept
# (shape, origin, records, ((radius, min_neighbors, kept share in percent), ...)): one record per integer point, y up to +32767, z from
# -32768. Radius 1: faces and interior / interior only, by index arithmetic; radius 2: the records with all 32 neighbours inside.
LATTICE = ((128, 128, 65), (-64, 32640, -32768), 128 * 128 * 65, ((1, 5, 99.9), (1, 6, 93.9), (2, 32, 88.1)))


def full_range():
    n, seed = FULL_RANGE[:2]
    return with_colour(np.random.default_rng(seed).integers(-32768, 32768, (n, 3)))


def surface_scatter():
    """5000 records on the plane z = 1500 + x // 8 (a 100 x 50 lattice, pitch 6 x 12 mm, x, y in [-300, 300)) and 300 records uniform in
    a 4 m cube, shuffled: (25, 4) keeps the surface and drops the scatter. Returns (records, is_surface)."""
    i = np.arange(5000)
    x, y = -300 + 6 * (i % 100), -300 + 12 * (i // 100)
    surface = np.stack([x, y, 1500 + x // 8], axis=1)
    rng = np.random.default_rng(7)
    order = rng.permutation(5300)
    scatter = rng.integers(-2000, 2000, (300, 3))
    xyz = np.concatenate([surface, scatter])[order]
    return with_colour(xyz), (order < 5000)


def _pairs(radius, offsets_in, offsets_out):
    """Isolated pairs on a lattice of pitch 8 radius (cell-aligned, the origin among its nodes; a pair reaches at most 3 radius from its
    node, so pairs of different nodes are more than a radius apart): each offset under every sign and translated so that the pair
    straddles a cell boundary (0 and +-r of the node) on each axis, the axes rotated from pair to pair. In-pairs keep each other at
    min_neighbors 1, out-pairs do not. Returns (xyz, expected); the lattice's last node, (3, 3, 3), is left free."""
    r = radius
    shifts = ((0, 0, 0), (-1, -1, -1), (-r, -r, -r), (-r - 1, 0, r - 1), (r, -1, -r + 1))
    nodes = itertools.product((0, -1, 1, -2, 2, -3, 3), repeat=3)
    xyz, want, turn = [], [], 0
    for kept, offsets in ((True, offsets_in), (False, offsets_out)):
        for off, sign, sh in itertools.product(offsets, itertools.product((1, -1), repeat=3), shifts):
            d = np.roll(np.array(off) * np.array(sign), turn % 3)
            turn += 1
            a = np.array(next(nodes)) * 8 * r + np.array(sh)
            xyz += [a, a + d]
            want += [kept, kept]
    assert len(want) < 2 * 342
    return np.array(xyz), np.array(want)


def boundary(s):
    """(0,0,0) and (3s,4s,0) are neighbours at radius 5s; (r,0,0) is in, (r,1,0) is out."""
    r = 5 * s
    xyz, want = _pairs(r, ((3 * s, 4 * s, 0), (r, 0, 0), (0, 0, 0)), ((r, 1, 0), (3 * s, 4 * s, 1)))
    return with_colour(xyz), want


def cell_corners(r):
    """Records of ADJACENT cells that lie more than r apart must not count: (0,0,0) and (2r-1,0,0) (r >= 2), and the diagonal."""
    xyz, want = _pairs(r, ((0, r, 0),), ((2 * r - 1, 0, 0), (2 * r - 1, 2 * r - 1, 2 * r - 1)))
    # the diagonal through a cell corner: node - h and node + (a - h) are a apart on every axis, a the smallest with 3 a^2 > r^2
    a = 1
    while 3 * a * a <= r * r:
        a += 1
    h = a // 2
    node = np.array([3, 3, 3]) * 8 * r
    extra = np.array([node - h, node + (a - h)])
    return with_colour(np.concatenate([xyz, extra])), np.concatenate([want, [False, False]])


def extremes():
    """Records at the ends of the int16 range, near pairs (1 mm apart) and lone ones; ends of one axis 65535 mm apart — one apart if
    anything wrapped at 16 bits — are never neighbours. Returns (records, expected at min_neighbors 1 for radius 1 and 1000)."""
    hi, lo = 32767, -32768
    xyz, want = [], []
    for axis in range(3):
        for end, step in ((hi, -1), (lo, 1)):
            a = np.array([0, 0, 0]); a[axis] = end
            b = a.copy(); b[axis] += step
            xyz += [a, b]; want += [True, True]
    for corner in itertools.product((hi, lo), repeat=3):
        a = np.array(corner)
        b = a.copy(); b[0] += -1 if corner[0] == hi else 1
        xyz += [a, b]; want += [True, True]
    for axis in range(3):                              # both ends of an axis at once, everything else equal
        a = np.array([5000, -7000, 9000]) + 2500 * axis; a[axis] = hi
        b = a.copy(); b[axis] = lo
        xyz += [a, b]; want += [False, False]
    return with_colour(np.array(xyz)), np.array(want)


def duplicates(m):
    return with_colour(np.tile(np.array([[-7, 1234, -32768]]), (m, 1)))


def saturation():
    """1000 records inside one radius (a cube of side 100, diagonal 173 < 200)."""
    return with_colour(np.random.default_rng(11).integers(-50, 50, (1000, 3)) + np.array([30000, -30000, 77]))


def identical(n=65536):
    """The early-exit case: n x 255 distance tests, not n^2."""
    return with_colour(np.tile(np.array([[123, -456, 789]]), (n, 1)))


@functools.lru_cache(maxsize=None)
def tiled_cubes(copies_per_axis=TILED[0], pitch=TILED[1]):
    """CUBES[0]'s cloud (side 400, radius 20, min_neighbors 3) copied to every node of a copies_per_axis^3 lattice of that pitch, node
    (i, j, k) at (i - copies_per_axis // 2) * pitch per axis, every copy with colour shorts of its own, the records shuffled by one fixed
    permutation: 7^3 x 6161 = 2 113 223 records, 1032 record tiles, 2064 slot tiles. Records of different copies are at least
    pitch - 399 apart, more than the radius, and the definition does not change under translation: the keep mask is the small cloud's
    (reference("cube400_r20_k3")), copy by copy, permuted. The pitch is no multiple of the radius: every copy meets the cell grid at
    another phase. Returns (records, expected keep mask), both read-only."""
    side, radius, k, seed, _ = CUBES[0]
    assert pitch - (side - 1) > radius, "neighbouring copies must be more than a radius apart"
    small = cube(side, seed)
    small_mask = reference(f"cube{side}_r{radius}_k{k}")
    n = small.shape[0]
    parts = []
    for c, node in enumerate(itertools.product(range(copies_per_axis), repeat=3)):
        offset = (np.array(node) - copies_per_axis // 2) * pitch
        parts.append(with_colour(small[:, :3].astype(np.int64) + offset, seed=1000 + c))
    order = np.random.default_rng(12).permutation(n * len(parts))
    rec = np.concatenate(parts)[order]
    mask = np.tile(small_mask, len(parts))[order]
    for a in range(0, rec.shape[0], 2048):
        assert 0 < mask[a:a + 2048].sum() < mask[a:a + 2048].shape[0], "a record tile with nothing kept, or nothing dropped"
    rec.setflags(write=False)
    mask.setflags(write=False)
    return rec, mask


@functools.lru_cache(maxsize=None)
def lattice_box(shape=LATTICE[0], origin=LATTICE[1]):
    """One record on every integer point of origin + [0, shape), shuffled by one fixed permutation. Returns (records, inside), both
    read-only: inside[i] = how many of record i's six lattice neighbours lie in the box, per axis (index > 0) + (index < extent - 1) —
    its neighbour count at radius 1, where every record is a cell of its own."""
    idx = np.indices(shape).reshape(3, -1).T
    inside = ((idx > 0).astype(np.int64) + (idx < np.array(shape) - 1)).sum(axis=1)
    order = np.random.default_rng(13).permutation(idx.shape[0])
    rec = with_colour((idx + np.array(origin))[order])
    inside = inside[order]
    rec.setflags(write=False)
    inside.setflags(write=False)
    return rec, inside


@functools.lru_cache(maxsize=None)
def random_cases():
    """The cases that have both kept and dropped records: (name, records, radius, min_neighbors, share in percent)."""
    out = [(f"cube{S}_r{r}_k{k}", cube(S, seed), r, k, share) for S, r, k, seed, share in CUBES]
    n, seed, r, k, share = FULL_RANGE
    out.append(("full_range", full_range(), r, k, share))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case but the 65 536 identical records: (name, records, radius_mm, min_neighbors, expected mask or None)."""
    out = [(name, rec, r, k, None) for name, rec, r, k, _ in random_cases()]
    rec, is_surface = surface_scatter()
    out.append(("surface_scatter", rec, 25, 4, is_surface))
    first = random_cases()[0]
    for n in COUNTS:
        out.append((f"count{n}", first[1][:n].copy(), first[2], first[3], None))
    for s in (1, 7, 200):
        rec, want = boundary(s)
        out.append((f"boundary_s{s}", rec, 5 * s, 1, want))
    rec, want = extremes()
    out.append(("extremes_r1", rec, 1, 1, want))
    out.append(("extremes_r1000", rec, 1000, 1, want))
    for m in (2, 65, 256):
        out.append((f"duplicates{m}_keep", duplicates(m), 1, min(m - 1, 255), np.ones(m, bool)))
        if m <= 255:
            out.append((f"duplicates{m}_drop", duplicates(m), 1, m, np.zeros(m, bool)))
    for r in (2, 10, 1000):
        rec, want = cell_corners(r)
        out.append((f"cell_corners_r{r}", rec, r, 1, want))
    out.append(("saturation", saturation(), 200, 255, np.ones(1000, bool)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute-force restatement's keep mask of a case, computed once per process and shared (read-only)."""
    import np_radius_outlier as N
    _, rec, r, k, _ = next(c for c in cases() if c[0] == name)
    mask = N.keep_mask(rec, r, k)
    mask.setflags(write=False)
    return mask
