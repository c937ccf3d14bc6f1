"""Clouds for the statistical outlier removal tests, shared by the CPU tier, the GPU tests and the CLI test; the clouds themselves
are tests/radius_outlier_cases.py's where it has them. Everything is deterministic. A case is (name, (n, 5) int16 records,
(mean_k, std_mul_milli, max_dist_mm), expected) where `expected` is a dict of what is known WITHOUT the brute force — any of the
statistics words, "keep" (the mask), "on_threshold" (how many records have D == T) — or None where only tests/np_stat_outlier.py
says."""
import functools

import numpy as np

import radius_outlier_cases as RC

COUNTS = RC.COUNTS
# (params, kept) of the random cases by a prototype of the definition: every one has 0 < kept < n
SURFACE = (((8, 1000, 100), 4704), ((16, 1000, 200), 4608))                       # of 5300; the second has D^2 >= 2^32
CUBE = (((3, 1000, 40), 5209), ((8, 500, 60), 4433), ((64, 0, 200), 3753))        # of 6161; the first has one sparse record


def line():
    """2600 records 5 mm apart on a line, more than one tile: the two nearest of an interior record are 5 and 5 away, of an end
    5 and 10."""
    i = np.arange(2600)
    return RC.with_colour(np.stack([-6500 + 5 * i, np.full(2600, 7), np.full(2600, -3)], axis=1))


def three():
    return RC.with_colour(np.array([[0, 0, 0], [10, 0, 0], [-10, 0, 0]]))


def identical(n):
    return RC.with_colour(np.tile(np.array([[123, -456, 789]]), (n, 1)))


def case_name(prefix, params):
    return f"{prefix}_k{params[0]}_m{params[1]}_d{params[2]}"


@functools.lru_cache(maxsize=None)
def random_cases():
    """The cases with kept and dropped records both: (name, records, params, kept by the prototype)."""
    surface = RC.surface_scatter()[0]
    cube = RC.cube(400, 1)
    return tuple([(case_name("surface", p), surface, p, kept) for p, kept in SURFACE] +
                 [(case_name("cube400", p), cube, p, kept) for p, kept in CUBE])


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    ends = np.ones(2600, bool)
    ends[[0, -1]] = False
    out.append(("line", line(), (2, 0, 10), {"dense": 2600, "s1": 6658560, "s2_lo": 17055744000, "s2_hi": 0, "threshold": 2560,
                                             "kept": 2598, "keep": ends, "on_threshold": 2598}))
    out.append(("three", three(), (2, 1000, 10), {"dense": 1, "s1": 5120, "threshold": 5120, "kept": 1,
                                                  "keep": np.array([True, False, False])}))
    out.append(("identical300", identical(300), (64, 0, 1), {"dense": 300, "s1": 0, "threshold": 0, "kept": 300, "keep": np.ones(300, bool)}))
    out.append(("identical65", identical(65), (64, 0, 1), {"dense": 65, "s1": 0, "threshold": 0, "kept": 65, "keep": np.ones(65, bool)}))
    out.append(("identical64", identical(64), (64, 0, 1), {"dense": 0, "s1": 0, "threshold": 0, "kept": 0, "keep": np.zeros(64, bool)}))
    for name, rec, params, kept in random_cases():
        out.append((name, rec, params, {"kept": kept}))
    cube = RC.cube(400, 1)
    for n in COUNTS:
        out.append((f"count{n}", cube[:n].copy(), (3, 1000, 100), None))
    out.append(("cube400_k1_m10000_d40", cube, (1, 10000, 40), None))
    rec = RC.extremes()[0]
    out.append(("extremes_d1", rec, (1, 1000, 1), None))
    out.append(("extremes_d1000", rec, (1, 0, 1000), None))
    for r in (2, 10, 1000):
        out.append((f"cell_corners_d{r}", RC.cell_corners(r)[0], (1, 1000, r), None))
    for s in (1, 7, 200):
        out.append((f"boundary_d{5 * s}", RC.boundary(s)[0], (1, 1000, 5 * s), None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute-force restatement of a case, computed once per process and shared (read-only): (kept records, keep mask, stats)."""
    import np_stat_outlier as N
    _, rec, params, _ = next(c for c in cases() if c[0] == name)
    out, keep, stats = N.stat_outlier(rec, *params)
    out.setflags(write=False)
    keep.setflags(write=False)
    return out, keep, stats
