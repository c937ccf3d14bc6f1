"""Clouds for the plane segmentation tests, shared by the CPU tier, the GPU tests and the CLI test. Everything is deterministic. A
case is (name, (n, 5) int16 records, params) with params = dict(distance_mm, iterations, min_inliers, max_planes, seed, mode), the
keyword arguments of np_planes.segment. The colour shorts are random (radius_outlier_cases.with_colour). What a scene case claims
(how many planes, about how many inliers) is stated in CLAIMS and checked on the restatement alone by tests/test_planeseg_cpu.py:
a GPU test never rests on an unchecked draw."""
import functools

import numpy as np

import radius_outlier_cases as RC

TILE, GROUP = 2048, 256                          # the score kernel's tile and workgroup
COUNTS = (63, 64, 65, GROUP - 1, GROUP, GROUP + 1, TILE - 1, TILE, TILE + 1)
ITERATIONS = (1, 63, 64, 65, 4096)
FLOOR_SEEDS = (1, 2, 3, 12345)
BIG = 20000                                      # the one multi-workgroup cloud


def params(distance_mm, iterations, min_inliers=3, max_planes=1, seed=1, mode=0):
    return dict(distance_mm=distance_mm, iterations=iterations, min_inliers=min_inliers, max_planes=max_planes, seed=seed, mode=mode)


def tilted(n, seed, share=0.6, noise=2, half=3000):
    """n records: `share` of them within +-noise of the plane 3 x + 4 y - 50 z = 0 (z rounded), the rest uniform in the cube; shuffled."""
    rng = np.random.default_rng(seed)
    on = int(round(n * share))
    xy = rng.integers(-half, half + 1, (on, 2))
    z = np.floor_divide(3 * xy[:, 0] + 4 * xy[:, 1], 50) + rng.integers(-noise, noise + 1, on)
    xyz = np.concatenate([np.column_stack([xy, z]), rng.integers(-half, half + 1, (n - on, 3))])
    return RC.with_colour(xyz[rng.permutation(n)])


def floor_scene():
    """A floor of 2 000 records within +-2 mm of z = -1200 plus 500 records scattered over the room."""
    rng = np.random.default_rng(7)
    floor = np.column_stack([rng.integers(-4000, 4001, (2000, 2)), -1200 + rng.integers(-2, 3, 2000)])
    scatter = np.column_stack([rng.integers(-4000, 4001, (500, 2)), rng.integers(-1100, 1500, 500)])
    xyz = np.concatenate([floor, scatter])
    return RC.with_colour(xyz[rng.permutation(2500)])


def slabs_scene():
    """Two slabs — 1 500 records within +-1 of z = -900 and 900 within +-1 of x = 2500 — and 300 scattered records: with
    min_inliers 400 the segmentation takes the two slabs, larger first, and stops in round 2 whatever max_planes allows."""
    rng = np.random.default_rng(8)
    a = np.column_stack([rng.integers(-3000, 2400, (1500, 2)), -900 + rng.integers(-1, 2, 1500)])
    b = np.column_stack([2500 + rng.integers(-1, 2, 900), rng.integers(-3000, 3001, 900), rng.integers(-800, 2500, 900)])
    c = np.column_stack([rng.integers(-3000, 2400, (300, 2)), rng.integers(-800, 2500, 300)])
    xyz = np.concatenate([a, b, c])
    return RC.with_colour(xyz[rng.permutation(xyz.shape[0])])


def tie_scene():
    """Two parallel exact slabs of 400 records each, z = 0 and z = 700 over the same 20 x 20 lattice of pitch 50, interleaved: every
    hypothesis with three non-collinear draws from one slab scores exactly 400 at distance 1, whichever slab it is."""
    g = 50 * np.indices((20, 20)).reshape(2, -1).T - 500
    xyz = np.concatenate([np.column_stack([g, np.zeros(400, np.int64)]), np.column_stack([g, np.full(400, 700)])])
    return RC.with_colour(xyz[np.random.default_rng(9).permutation(800)])


def big_scene():
    """BIG records over ten tiles: half on the tilted plane, a quarter within +-2 of x = -2500, a quarter scattered."""
    rng = np.random.default_rng(12)
    a = tilted(BIG // 2, 60, share=1.0)[:, :3].astype(np.int64)
    b = np.column_stack([-2500 + rng.integers(-2, 3, BIG // 4), rng.integers(-3000, 3001, (BIG // 4, 2))])
    c = rng.integers(-3000, 3001, (BIG // 4, 3))
    xyz = np.concatenate([a, b, c])
    return RC.with_colour(xyz[rng.permutation(BIG)])


def collinear(n):
    """n records on the line (3, -2, 7) t: every triple is collinear."""
    t = np.random.default_rng(10).integers(-4000, 4001, n)
    return RC.with_colour(np.column_stack([3 * t, -2 * t, 7 * t]))


def equal(n):
    return RC.with_colour(np.tile(np.array([[123, -4567, 32767]]), (n, 1)))


def three():
    return RC.with_colour(np.array([[0, 0, 0], [100, 0, 5], [0, 100, -5]]))


@functools.lru_cache(maxsize=None)
def cases():
    out = [("count0", np.zeros((0, 5), np.int16), params(6, 64)),
           ("count1", tilted(1, 31), params(6, 64)),
           ("count2", tilted(2, 32), params(6, 64)),
           ("count3", three(), params(6, 64)),
           ("count3_two_planes", three(), params(6, 64, max_planes=2)),
           ("collinear", collinear(500), params(10, 64, max_planes=2)),
           ("equal", equal(300), params(10, 64))]
    out += [(f"count{n}", tilted(n, 100 + n), params(6, 64, min_inliers=20)) for n in COUNTS]
    out += [(f"iterations{k}", tilted(300, 50), params(6, k, min_inliers=5, max_planes=2, seed=77)) for k in ITERATIONS]
    out += [(f"floor_seed{s}", floor_scene(), params(6, 64, min_inliers=1000, seed=s)) for s in FLOOR_SEEDS]
    out += [(f"slabs_max{p}", slabs_scene(), params(4, 128, min_inliers=400, max_planes=p, seed=5)) for p in (1, 2, 8)]
    out += [(f"slabs_keep_max{p}", slabs_scene(), params(4, 128, min_inliers=400, max_planes=p, seed=5, mode=1)) for p in (1, 8)]
    out.append(("tie", tie_scene(), params(1, 600, min_inliers=400, seed=2)))
    out.append(("big", big_scene(), params(8, 64, min_inliers=1000, max_planes=3, seed=11)))
    return tuple(out)


# what a case claims about itself: planes accepted, and bounds on each plane's inliers (lo, hi), in order
CLAIMS = {
    "count0": (0, []), "count1": (0, []), "count2": (0, []), "count3": (1, [(3, 3)]), "count3_two_planes": (1, [(3, 3)]),
    "collinear": (0, []), "equal": (0, []),
    **{f"floor_seed{s}": (1, [(2000, 2010)]) for s in FLOOR_SEEDS},
    "slabs_max1": (1, [(1500, 1520)]), "slabs_max2": (2, [(1500, 1520), (900, 915)]), "slabs_max8": (2, [(1500, 1520), (900, 915)]),
    "slabs_keep_max1": (1, [(1500, 1520)]), "slabs_keep_max8": (2, [(1500, 1520), (900, 915)]),
    "tie": (1, [(400, 400)]),
    "big": (2, [(BIG // 2, BIG // 2 + 200), (BIG // 4, BIG // 4 + 200)]),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute-force restatement of a case, computed once per process and shared (read-only):
    (labels, n_planes, models, stats, kept records)."""
    import np_planes as N
    _, rec, P = next(c for c in cases() if c[0] == name)
    labels, n_planes, models, stats, kept = N.segment(rec, **P)
    labels.setflags(write=False)
    kept.setflags(write=False)
    return labels, n_planes, tuple(models), stats, kept


# ---- planes chosen by hand for pcs_plane_count_inliers_device: (name, records, [(nx, ny, nz, off, T)], the counts known by hand) -----
def chosen_planes():
    import np_planes as N
    out = []
    # an axis-aligned plane z = 100, N = (0, 0, 7), distance 5: T = 35; records at distance exactly 5 (in) and 6 (out), both sides
    rec = RC.with_colour(np.array([[10, 20, 105], [-10, 3, 95], [0, 0, 106], [5, 5, 94], [1, 2, 100]]))
    out.append(("axis", rec, [(0, 0, 7, 700, 35)], [3]))
    # a 3-4-5 normal: a = (-4, 3, 0), b = (0, 0, 1) give N = (3, 4, 0), |N| = 5; distance 7: T = 35 exactly
    eq = N.plane((0, 0, 0), (-4, 3, 0), (0, 0, 1), 7)
    assert eq == (3, 4, 0, 0, 35)
    rec = RC.with_colour(np.array([[5, 5, 9], [1, 8, 0], [-5, -5, 3], [-1, -8, -4], [0, 0, 32767]]))      # dots 35, 35, -35, -35, 0
    out.append(("three_four_five", rec, [eq], [5]))
    rec = RC.with_colour(np.array([[5, 5, 9], [4, 6, 0], [-5, -5, 3], [-4, -6, -4], [0, 0, -32768], [10, 1, 0], [-12, 0, 5]]))
    out.append(("three_four_five_out", rec, [eq], [4]))          # dots 35, 36, -35, -36, 0, 34, -36
    # planes through corners of the cube, records on the far corners: the largest N, off and dot; nothing may wrap
    lo, hi = -32768, 32767
    corners = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)])
    eqs = [N.plane((lo, lo, lo), (hi, lo, hi), (lo, hi, hi), d) for d in (1, 1000)]
    eqs += [N.plane((hi, hi, hi), (lo, hi, lo), (hi, lo, lo), 1), N.plane((lo, lo, hi), (hi, hi, hi), (hi, lo, lo), 1000)]
    assert all(e is not None for e in eqs) and max(abs(v) for e in eqs for v in e[:3]) == 65535 ** 2      # a triangle in a square of side L: |N| <= L^2
    out.append(("cube", RC.with_colour(corners), eqs, None))
    return out
