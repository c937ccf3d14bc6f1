"""Clouds for the alignment tests, shared by the CPU tier, the GPU tests and the CLI test. Everything is deterministic.
A case is (name, source (n, 5) int16, target (m, 5) int16, max_dist_mm, expected) where `expected` is None or the list of matched
target coordinates per source record known WITHOUT the brute force (None for an unmatched record). The colour shorts are random:
the match does not read them.
scene() is the synthetic scene of the loop tests: two independent samples of the same surfaces seen through a known offset."""
import functools
import math

import numpy as np

from radius_outlier_cases import with_colour

SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 6161)      # n_source against the 6 161-record target
REDUCE_WIDTH = 256                                                    # lanes of the reduce kernel: one partial each per pass
TWO_PASSES = 256 * REDUCE_WIDTH + 300                                 # source records: 258 partials, the reduce loop runs twice
RANDOM = ((500, 1, 16), (900, 3, 40), (1500, 20, 300), (2049, 250, 3000), (4000, 1000, 20000), (3000, 20, 250), (700, 1000, 65536),
          (2500, 3, 30))                                              # (records, max_dist, cube side)


def cloud(n, side, seed):
    lo = -(side // 2)
    return with_colour(np.random.default_rng(seed).integers(lo, lo + side, (n, 3)), seed)


def rec(points, seed=5):
    return with_colour(np.asarray(points, np.int64).reshape(-1, 3), seed)


@functools.lru_cache(maxsize=None)
def big_target():
    return cloud(6161, 400, 1)


@functools.lru_cache(maxsize=None)
def big_source():
    return cloud(6161, 400, 2)


def tie_target():
    return [(5, 0, 0), (-5, 0, 0), (0, 5, 0), (0, 0, -5), (0, 0, 5)]


def cases():
    out = []
    for n in SIZES:
        out.append((f"size{n}", big_source()[:n], big_target(), 20, None))
    out.append(("reduce_two_passes", cloud(TWO_PASSES, 200, 3), cloud(300, 200, 4), 20, None))
    out.append(("target1", cloud(500, 40, 5), rec([(3, -2, 7)]), 20, None))
    out.append(("source0", big_source()[:0], big_target()[:100], 20, None))
    out.append(("target0", big_source()[:300], big_target()[:0], 20, None))
    out.append(("both0", big_source()[:0], big_target()[:0], 20, None))
    # ties: five records at distance 5; (z, y, x) order picks the lowest z
    out.append(("tie5", rec([(0, 0, 0)]), rec(tie_target()), 10, [(0, 0, -5)]))
    out.append(("tie5_shuffled", rec([(0, 0, 0)]), rec([tie_target()[k] for k in (4, 2, 0, 3, 1)]), 10, [(0, 0, -5)]))
    out.append(("tie5_duplicates", rec([(0, 0, 0)] * 3), rec(tie_target() * 3 + [(0, 0, -5)]), 10, [(0, 0, -5)] * 3))
    out.append(("tie_z_then_y_then_x", rec([(0, 0, 0)]), rec([(3, 4, 0), (4, 3, 0), (-4, 3, 0), (0, 5, 0), (5, 0, 0)]), 5, [(5, 0, 0)]))
    # a tie between the own cell ([0, 10) on x) and the cell below / above it: the lower x wins, wherever it lies
    out.append(("tie_own_vs_neighbour_cell", rec([(2, 5, 5), (7, 1005, 5)]), rec([(5, 5, 5), (-1, 5, 5), (4, 1005, 5), (10, 1005, 5)]), 10,
                [(-1, 5, 5), (4, 1005, 5)]))
    # the radius edge: d^2 = max_dist^2 matches, max_dist^2 + 1 does not (the second pair sits 5 000 mm away on y)
    for r in (1, 7, 1000):
        out.append((f"edge_r{r}", rec([(0, 0, 0), (0, 5000, 0)]), rec([(r, 0, 0), (r, 5000, 1)]), r, [(r, 0, 0), None]))
    out.append(("edge_r7_offaxis", rec([(0, 0, 0), (100, 0, 0)]), rec([(2, 3, 6), (102, 3, 6), (103, 3, 6)]), 7, [(2, 3, 6), (102, 3, 6)]))
    # cell corners, cells of 10: the own cell holds a candidate at distance r - 1, a neighbour cell one much nearer — across a face,
    # across an edge, across the corner. The nearer one wins: what a pruning rule that trusts the own cell breaks.
    out.append(("corner_face", rec([(9, 5, 5)]), rec([(0, 5, 5), (10, 5, 5)]), 10, [(10, 5, 5)]))
    out.append(("corner_edge", rec([(9, 9, 5)]), rec([(0, 9, 5), (10, 10, 5)]), 10, [(10, 10, 5)]))
    out.append(("corner_diagonal", rec([(9, 9, 9)]), rec([(0, 9, 9), (10, 10, 10)]), 10, [(10, 10, 10)]))
    out.append(("corner_diagonal_low", rec([(0, 0, 0)]), rec([(9, 0, 0), (-1, -1, -1)]), 10, [(-1, -1, -1)]))
    # and a tie across the corner: equal d^2 = 3 in the own cell and in the diagonal one
    out.append(("corner_tie_own_wins", rec([(9, 9, 9)]), rec([(10, 10, 10), (8, 8, 8)]), 10, [(8, 8, 8)]))
    out.append(("corner_tie_diagonal_wins", rec([(0, 0, 0)]), rec([(1, 1, 1), (-1, -1, -1)]), 10, [(-1, -1, -1)]))
    # extremes: the ends of the int16 range on every axis; cells beyond 0..65535 do not exist, nothing wraps (32767 and -32768 are
    # 65 535 mm apart, not 1)
    ends = [(x, y, z) for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)]
    inward = [tuple(v + (3 if v < 0 else -3) if a == k % 3 else v for a, v in enumerate(e)) for k, e in enumerate(ends)]
    for r in (1, 5, 1000):
        out.append((f"extremes_r{r}", rec(ends + inward), rec(ends + inward + [(0, 0, 0)]), r, None))
        out.append((f"extremes_apart_r{r}", rec(ends), rec(inward), r, [i if r >= 3 else None for i in inward]))
    out.append(("extremes_no_wrap", rec([(32767, 0, 0), (0, -32768, 0)]), rec([(-32768, 0, 0), (0, 32767, 0)]), 1000, [None, None]))
    # the width of the sums: products of +-2^30 x 4 096
    out.append(("width", rec([(32767, -32768, 32767)] * 4096), rec([(32767, -32768, 32766)]), 1, [(32767, -32768, 32766)] * 4096))
    for k, (n, r, side) in enumerate(RANDOM):
        hi = min(side, 65536)
        out.append((f"random{k}_n{n}_r{r}", cloud(n, hi, 100 + k), cloud(max(n - 137, 1), hi, 200 + k), r, None))
    return out


def expected_sums(source, expected):
    """The eighteen sums from a hand-written list of matches (None: unmatched), in Python integers."""
    p = np.asarray(source).reshape(-1, 5)[:, :3].astype(np.int64).tolist()
    s = [len(p), 0] + [0] * 16
    dist2 = []
    for pi, q in zip(p, expected):
        if q is None:
            dist2.append(0xFFFFFFFF)
            continue
        d2 = sum((a - b) ** 2 for a, b in zip(pi, q))
        s[1] += 1
        for a in range(3):
            s[2 + a] += pi[a]
            s[5 + a] += q[a]
            for b in range(3):
                s[8 + 3 * a + b] += pi[a] * q[b]
        s[17] += d2
        dist2.append(d2)
    return s, np.array(dist2, np.uint32)


# ---- the synthetic scene ---------------------------------------------------------------------------------
SCENE_POINTS = 3000
SCENE_MAX_DIST, SCENE_ITERATIONS = 60, 20
TRUE_ANGLE_DEG, TRUE_AXIS, TRUE_TRANS_MM = 2.0, (0.3, -0.5, 0.81), (9.0, -8.0, 9.0)       # about 2 degrees and 15 mm


def rigid(angle_deg, axis, trans_mm):
    """Row-major 4x4 in metres (float64): the rotation by angle_deg about axis, then the translation."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(angle_deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T[:3, 3] = np.asarray(trans_mm, np.float64) / 1000.0
    return T


def surfaces(n, seed):
    """n points (float64 mm) on three mutually perpendicular planes meeting at (-600, -600, -600), 1 300 mm a side, and a patch
    raised 120 mm off the floor: 30 % per plane, 10 % on the patch."""
    rng = np.random.default_rng(seed)
    per = (3 * n) // 10
    pts = []
    for axis in range(3):
        uv = rng.uniform(-600, 700, (per, 2))
        p = np.full((per, 3), -600.0)
        p[:, [k for k in range(3) if k != axis]] = uv
        if axis == 2:                       # the floor z = -600: no floor under the patch
            inside = (abs(uv[:, 0] - 100) < 200) & (abs(uv[:, 1] - 50) < 150)
            p[inside, 2] = -480.0
        pts.append(p)
    m = n - 3 * per
    patch = np.stack([rng.uniform(-100, 300, m), rng.uniform(-100, 200, m), np.full(m, -480.0)], axis=1)
    pts.append(patch)
    return np.concatenate(pts)


@functools.lru_cache(maxsize=None)
def scene():
    """(source records, target records, truth): the target is SCENE_POINTS points of the surfaces rounded to mm; the source an
    independent sample of the same surfaces seen from a frame that `truth` (float64 4x4, metres) maps onto the target's."""
    truth = rigid(TRUE_ANGLE_DEG, TRUE_AXIS, TRUE_TRANS_MM)
    target = np.rint(surfaces(SCENE_POINTS, 11)).astype(np.int64)
    world = surfaces(SCENE_POINTS, 12)
    inv = np.linalg.inv(truth)
    local = (inv[:3, :3] @ world.T).T + 1000.0 * inv[:3, 3]
    return with_colour(np.rint(local).astype(np.int64), 21), with_colour(target, 22), truth


def pose_error(m, truth):
    """(rotation error in degrees, translation error in mm) of a 4x4 in metres against the truth."""
    m, truth = np.asarray(m, np.float64).reshape(4, 4), np.asarray(truth, np.float64)
    R = m[:3, :3] @ truth[:3, :3].T
    sx, sy, sz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    ang = math.atan2(0.5 * math.sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (np.trace(R) - 1.0))
    return math.degrees(ang), 1000.0 * float(np.linalg.norm(m[:3, 3] - truth[:3, 3]))


def far_away(records, shift=(20000, 0, 0)):
    """The same records moved where nothing of the scene is within max_dist: a source with no overlap."""
    r = np.array(records, copy=True)
    r[:, :3] = (r[:, :3].astype(np.int64) + np.asarray(shift)).astype(np.int16)
    return r
