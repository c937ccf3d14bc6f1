"""Clouds for the surface-normal and point-to-plane tests, shared by the CPU tier and the GPU tests. Everything is deterministic.
A normals case is (name, payload (n, 5) int16, (radius_mm, min_neighbors, flatness)). The colour shorts are random: nothing reads
them. The scene is align_cases.scene(); SCENE_NORMALS are the settings the point-to-plane loop is measured with."""
import functools

import numpy as np

import align_cases as K
from radius_outlier_cases import with_colour

SCENE_NORMALS = (120, 6, 20)                 # radius_mm, min_neighbors, flatness
SCENE_CENTRE = (50, 50, 50)                  # inside the corner the scene's three planes make: every surface faces it
NORMAL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2049, 6161)


def size_params(n):
    """Prefixes of big_target() (a uniform cloud in a 400 mm cube): a radius at which valid and invalid records both occur."""
    return (110, 5, 0) if n <= 65 else (70, 5, 0) if n <= 257 else (35, 5, 0) if n <= 2049 else (25, 5, 0)


def grid_plane(axis, at, lo, count=20, pitch=10):
    """count x count integer grid points on the plane `axis` = at, the other two coordinates lo, lo + pitch, ..."""
    u, v = np.meshgrid(lo + pitch * np.arange(count), lo + pitch * np.arange(count), indexing="ij")
    p = np.full((count * count, 3), at, np.int64)
    p[:, [k for k in range(3) if k != axis]] = np.stack([u.reshape(-1), v.reshape(-1)], axis=1)
    return p


def tilted_plane(n, seed):
    """n points of the plane through (300, -200, 100) with normal (1, 2, 3), 800 mm across, rounded to millimetres."""
    rng = np.random.default_rng(seed)
    nrm = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    e1 = np.cross(nrm, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    uv = rng.uniform(-400, 400, (n, 2))
    return np.rint(np.array([300.0, -200.0, 100.0]) + uv[:, :1] * e1 + uv[:, 1:] * e2).astype(np.int64)


@functools.lru_cache(maxsize=None)
def normal_cases():
    out = []
    for n in NORMAL_SIZES:
        out.append((f"size{n}", K.big_target()[:n], size_params(n)))
    target = K.scene()[1]
    out.append(("scene", target, SCENE_NORMALS))
    out.append(("scene_no_gate", target, SCENE_NORMALS[:2] + (0,)))
    for axis, name in enumerate("xyz"):
        out.append((f"grid_{name}", with_colour(grid_plane(axis, 70 - 30 * axis, -95), 30 + axis), (25, 6, 20)))
    out.append(("line", with_colour(np.arange(100)[:, None] * np.array([3, 1, 2]), 33), (50, 3, 0)))
    out.append(("one_point_50", with_colour([(7, -8, 9)] * 50, 34), (10, 3, 0)))
    out.append(("identical_4096", with_colour([(100, -200, 300)] * 4096, 35), (10, 3, 20)))
    out.append(("int16_high_end", with_colour(grid_plane(2, 32767, 32767 - 190), 36), (25, 6, 20)))
    out.append(("int16_low_end", with_colour(grid_plane(0, -32768, -32768), 37), (25, 6, 20)))
    out.append(("tilted", with_colour(tilted_plane(1500, 38), 38), (100, 6, 20)))
    return tuple(out)


def normal_case(name):
    return [c for c in normal_cases() if c[0] == name][0]


# ---- the plane sums ----------------------------------------------------------------------------------------
def random_normals(m, seed, invalid=0.2):
    """int16 [m, 4]: caller-made normals, any int16 in every short; short 3 is 0 (no valid normal) for about `invalid` of them."""
    rng = np.random.default_rng(seed)
    nrm = rng.integers(-32768, 32768, (m, 4)).astype(np.int16)
    nrm[(nrm[:, 3] == 0) | (rng.random(m) < invalid), 3] = 0
    keep = nrm[:, 3] != 0
    assert m < 8 or (keep.any() and not keep.all())
    return nrm


def overflow_case():
    """4 096 source records at one corner of the int16 range against one target record one millimetre away: |p x n| is about
    2^29.5 x 1.41, its square passes 2^59, the sum of 4 096 of them 2^70: a lone 64-bit accumulator anywhere fails."""
    return ("overflow", K.rec([(32767, -32768, 32767)] * 4096), K.rec([(32767, -32768, 32766)]), np.array([[0, 11585, 11585, 5]], np.int16), 1)


@functools.lru_cache(maxsize=None)
def plane_sum_cases():
    """(name, source, target, target normals int16 [m, 4], max_dist_mm): every cloud of align_cases.cases() with caller-made random
    normals, then the cases the normals are for."""
    out = []
    for k, (name, source, target, r, _) in enumerate(K.cases()):
        out.append((name, source, target, random_normals(target.shape[0], 500 + k), r))
    # equal target records that carry different normals: the smallest valid word is the one used, wherever it sits
    dup_t = K.rec([(5, 0, 0)] * 4 + [(0, 7, 0)] * 3 + [(0, 0, -6)] * 2)
    dup_n = np.array([[9, 9, 9, 3], [1, 2, 3, 0], [-5, 4, 3, 2], [7, 7, 7, 2],          # (5, 0, 0): word order is by short 3 first
                      [1, 1, 1, 0], [-32768, 32767, -1, -1], [2, 2, 2, 0],              # (0, 7, 0): one valid record, all bits set
                      [3, 3, 3, 0], [4, 4, 4, 0]], np.int16)                            # (0, 0, -6): none valid
    dup_s = K.rec([(4, 1, 0), (6, -1, 1), (1, 7, 1), (0, 6, -1), (1, 0, -6), (300, 300, 300)])
    out.append(("duplicates", dup_s, dup_t, dup_n, 10))
    out.append(("duplicates_reversed", dup_s[::-1].copy(), dup_t[::-1].copy(), dup_n[::-1].copy(), 10))
    name, source, target, r, _ = [c for c in K.cases() if c[0] == "size257"][0]
    none = random_normals(target.shape[0], 600)
    none[:, 3] = 0
    out.append(("all_invalid", source, target, none, r))
    ones = np.full((target.shape[0], 4), -1, np.int16)                                  # every word all ones: valid, and the largest
    out.append(("all_ones", source, target, ones, r))
    out.append(overflow_case())
    return tuple(out)


def plane_sum_case(name):
    return [c for c in plane_sum_cases() if c[0] == name][0]


def one_plane(n=1500, seed=41):
    """A target that is one plane (z = -600, rounded samples) and a source sampled from it a few millimetres off: the pose along
    the plane is not determined."""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.uniform(-500, 500, n), rng.uniform(-500, 500, n), np.full(n, -600.0)], axis=1)
    s = np.stack([rng.uniform(-500, 500, n), rng.uniform(-500, 500, n), np.full(n, -597.0)], axis=1)
    return with_colour(np.rint(s).astype(np.int64), seed), with_colour(np.rint(t).astype(np.int64), seed + 1)


def two_parallel_planes(n=1500, seed=43):
    rng = np.random.default_rng(seed)
    z = np.where(rng.random(n) < 0.5, -600.0, 300.0)
    t = np.stack([rng.uniform(-500, 500, n), rng.uniform(-500, 500, n), z], axis=1)
    s = np.stack([rng.uniform(-500, 500, n), rng.uniform(-500, 500, n), z + 3.0], axis=1)
    return with_colour(np.rint(s).astype(np.int64), seed), with_colour(np.rint(t).astype(np.int64), seed + 1)
