"""Clouds for the background model's tests, shared by the CPU tier and the GPU tests. Everything is deterministic. A case is a Case:
the model's constants, the frame-sets to learn, the payload to subtract from, the (min_seen, dilate) pairs to subtract at, and — where
it is known WITHOUT the restatement — the expected background mask per pair. Coordinates come from seeded generators, colours from
radius_outlier_cases.with_colour: the high byte of short 4 is never zero (the filter copies all ten bytes of a record).
check() asserts, on the CPU, that every non-degenerate case both keeps and drops records under the restatement: a case where the
filter does nothing proves nothing."""
import collections
import functools
import itertools

import numpy as np

import np_background as N
from radius_outlier_cases import with_colour

TILE = 2048
COUNTS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 6161)          # a ragged last ballot word, one full tile plus one record, three tiles

Case = collections.namedtuple("Case", "name cell_mm max_cells frames payload params expected degenerate")


def case(name, cell_mm, max_cells, frames, payload, params, expected=None, degenerate=False):
    return Case(name, cell_mm, max_cells, tuple(frames), payload, tuple(params), expected, degenerate)


# ---- csrc/pcs_outlier_index.h's table arithmetic, restated (as tests/test_radius_outlier_scale.py describes it): used to BUILD the
# ---- cloud whose probe sequences wrap, never for an expectation
def table_slots(max_cells):
    return (max(2 * max_cells, 1) + TILE - 1) // TILE * TILE


def cell_key(cx, cy, cz):
    return np.asarray(cx, np.uint64) | np.asarray(cy, np.uint64) << np.uint64(16) | np.asarray(cz, np.uint64) << np.uint64(32)


def first_slot(key, slots):
    k = np.array(key, np.uint64)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)                               # (modulo 2^64, as the kernel's)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return ((k & np.uint64(0xFFFFFFFF)) * np.uint64(slots)) >> np.uint64(32)


# ---- the scene of the count cases ---------------------------------------------------------------------------------------------------
def scene():
    """Five frame-sets, each about 70 % of 4000 "static" records in a cube of side 400 (cell 20: seen runs from 0 to 5 over the cells),
    and a payload of 6161 records: half drawn from the static records, half uniform in a cube of side 600, shuffled."""
    rng = np.random.default_rng(5)
    static = rng.integers(-200, 200, (4000, 3))
    frames = [with_colour(static[rng.random(4000) < 0.7], seed=20 + k) for k in range(5)]
    xyz = np.concatenate([static[rng.integers(0, 4000, 3080)], rng.integers(-300, 300, (3081, 3))])
    payload = with_colour(xyz[rng.permutation(6161)])
    return frames, payload


def identical(n=65536):
    return with_colour(np.tile(np.array([[123, -456, 789]]), (n, 1)))


def range_ends():
    """cell_mm 1: cells 0 and 65535 exist. Background at the LOW end of each axis (and at the all-low corner); the payload holds those
    records (background), their neighbours one cell inwards (background only with dilate 1), the records at the HIGH end of the same
    axis — one cell away if anything wrapped at 16 bits — and the mirror image: background at the high end of y only, a record at its
    low end. Returns (frames, payload, {(min_seen, dilate): background mask})."""
    lo, hi = -32768, 32767
    bg = [(lo, 5, 5), (5, lo, 5), (5, 5, lo), (lo, lo, lo), (77, hi, -9)]
    pay, d0, d1 = [], [], []
    for b in bg:
        pay.append(b); d0.append(True); d1.append(True)
    for b in bg[:3]:
        axis = b.index(lo)
        inward = list(b); inward[axis] = lo + 1
        pay.append(tuple(inward)); d0.append(False); d1.append(True)
        far = list(b); far[axis] = hi
        pay.append(tuple(far)); d0.append(False); d1.append(False)          # cell 65535 against cell 0: they must not meet
        near_far = list(b); near_far[axis] = hi - 1
        pay.append(tuple(near_far)); d0.append(False); d1.append(False)
    pay.append((hi, hi, hi)); d0.append(False); d1.append(False)            # against the all-low corner, every axis at once
    pay.append((lo + 1, lo + 1, lo + 1)); d0.append(False); d1.append(True)
    pay.append((77, lo, -9)); d0.append(False); d1.append(False)            # against (77, hi, -9)
    pay.append((78, hi - 1, -10)); d0.append(False); d1.append(True)
    frames = [with_colour(np.array(bg))]
    return frames, with_colour(np.array(pay)), {(1, 0): np.array(d0), (1, 1): np.array(d1)}


def floors():
    """cell_mm 1000: -1 and 0 lie in different cells (a truncating division would put both into cell 0), -1000 and -1001 too; the ends
    of the range are cells 32735 and 32800."""
    bg = [(-1, 500, 500), (500, -1000, 500), (-32768, -32768, 32767)]
    pay = [(-1, 500, 500), (0, 500, 500), (-1000, 500, 500), (-1001, 500, 500), (500, -1000, 500), (500, -1001, 500), (500, -1, 500),
           (500, 0, 500), (-32768, -32768, 32767), (-32001, -32001, 32000), (-31999, -32768, 32767), (32767, 32767, -32768)]
    d0 = [True, False, True, False, True, False, True, False, True, True, False, False]
    return [with_colour(np.array(bg))], with_colour(np.array(pay)), {(1, 0): np.array(d0)}


def min_seen_groups():
    """Five frame-sets; group j (1..5) is 40 cells of edge 50 that frame-sets 0 .. j-1 hold, the groups three cells apart and more; the
    payload holds five records of every cell and 200 records of cells nobody learned. Background at min_seen m, dilate 0: the groups
    j >= m; at 6 nothing."""
    rng = np.random.default_rng(9)
    cells = rng.permutation(np.stack(np.meshgrid(*[np.arange(-6, 6)] * 3, indexing="ij"), -1).reshape(-1, 3))[:240] * 4      # pitch 4 cells
    group = np.repeat(np.arange(1, 7), 40)                           # 6: never learned
    centre = cells * 50 + 25
    frames = [with_colour(centre[(group <= 5) & (group > k)] + rng.integers(-20, 20, 3), seed=40 + k) for k in range(5)]
    xyz = np.repeat(centre, 5, axis=0) + rng.integers(-24, 25, (1200, 3))
    g = np.repeat(group, 5)
    order = rng.permutation(1200)
    expected = {(m, 0): (g[order] >= m) & (g[order] <= 5) for m in (1, 3, 5, 6)}
    return frames, with_colour(xyz[order]), expected


def dilate_shapes():
    """Isolated background cells (edge 30, ten cells apart); around each a foreground record one cell away on a face, on an edge and on
    a corner, and one two cells away, under every sign. dilate 0: none is background; dilate 1: all but the two-away ones."""
    nodes = np.array(list(itertools.product((-2, -1, 0, 1), repeat=3))) * 10
    signs = list(itertools.product((1, -1), repeat=3))
    bg, pay, d1 = [], [], []
    for i, node in enumerate(nodes):
        s = np.array(signs[i % 8])
        bg.append(node * 30 + 15)
        for off, near in (((1, 0, 0), True), ((1, 1, 0), True), ((1, 1, 1), True), ((2, 0, 0), False), ((2, 1, 1), False)):
            o = np.roll(np.array(off), i % 3) * s
            pay.append((node + o) * 30 + (i * 7) % 30)
            d1.append(near)
        pay.append(node * 30 + 29); d1.append(True)                  # in the background cell itself
    d1 = np.array(d1)
    d0 = np.zeros_like(d1); d0[5::6] = True
    return [with_colour(np.array(bg))], with_colour(np.array(pay)), {(1, 0): d0, (1, 1): d1}


WRAP_CELL, WRAP_MAX_CELLS = 1000, 1024


def wrap_probes():
    """A table of 2048 slots (max_cells 1024) at cell_mm 1000: twelve learned cells whose probe sequences start at slot 2047 and twelve
    at 2046 — their run wraps past the last slot to slots 0 .. 21 — and, in the payload, records of those cells (background), records of
    OTHER cells that start at 2046 / 2047 and were never learned (a miss has to walk the wrapped run to its end), and records of cells
    that start at slots 0 .. 8, inside the run."""
    slots = table_slots(WRAP_MAX_CELLS)
    q = np.arange(-33, 33)
    cells = np.stack(np.meshgrid(q, q, q, indexing="ij"), axis=-1).reshape(-1, 3)
    start = first_slot(cell_key(*(cells + 32768).T), slots)
    assert slots == 2048
    a, b, low = cells[start == 2047], cells[start == 2046], cells[start <= 8]
    assert a.shape[0] >= 24 and b.shape[0] >= 24 and low.shape[0] >= 24
    learned = np.concatenate([a[:12], b[:12], low[:6]])
    missed = np.concatenate([a[12:24], b[12:24], low[6:24]])
    rng = np.random.default_rng(21)

    def records(c, per):
        xyz = np.repeat(c, per, axis=0) * 1000 + rng.integers(0, 1000, (c.shape[0] * per, 3))
        return np.clip(xyz, -32768, 32767)
    frames = [with_colour(records(learned, 2)[rng.permutation(60)], seed=60 + k) for k in range(2)]
    xyz = np.concatenate([records(learned, 3), records(missed, 3)])
    order = rng.permutation(xyz.shape[0])
    is_bg = (np.arange(xyz.shape[0]) < learned.shape[0] * 3)[order]
    payload = with_colour(xyz[order])
    got = N.cells_of(payload, WRAP_CELL) - 32768                      # (the clip moved nobody out of its cell)
    assert (got == np.concatenate([np.repeat(learned, 3, axis=0), np.repeat(missed, 3, axis=0)])[order]).all()
    return frames, payload, {(2, 0): is_bg, (3, 0): np.zeros_like(is_bg)}


def distinct_cells(n, cell_mm=100):
    """n records in n distinct cells."""
    i = np.arange(n)
    return with_colour(np.stack([(i % 9 - 4) * cell_mm + 7, (i // 9 - 4) * cell_mm + 50, np.full(n, -3 * cell_mm + 1)], axis=1))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    frames, payload = scene()
    for n in COUNTS:
        out.append(case(f"count{n}", 20, 8192, frames, payload[:n].copy(), ((3, 0), (3, 1), (1, 0), (5, 1)), degenerate=n < 2))
    frames, payload, exp = range_ends()
    out.append(case("range_ends_cell1", 1, 64, frames, payload, exp, exp))
    frames, payload, exp = floors()
    out.append(case("floors_cell1000", 1000, 64, frames, payload, list(exp) + [(1, 1)], exp))
    frames, payload, exp = min_seen_groups()
    out.append(case("min_seen_groups", 50, 1024, frames, payload, exp, exp))
    frames, payload, exp = dilate_shapes()
    out.append(case("dilate_shapes", 30, 64, frames, payload, exp, exp))
    frames, payload, exp = wrap_probes()
    out.append(case("wrap_probes", WRAP_CELL, WRAP_MAX_CELLS, frames, payload, list(exp) + [(1, 1), (2, 1)], exp))
    out.append(case("exactly_max_cells", 100, 64, [distinct_cells(64)], distinct_cells(65), ((1, 0),),
                    {(1, 0): np.arange(65) < 64}))
    return tuple(out)


CASES = {c.name: c for c in cases()}


@functools.lru_cache(maxsize=None)
def model_of(name):
    """The restatement's model of a case after its frame-sets, computed once per process and shared: nobody changes it."""
    c = CASES[name]
    return N.learned(c.cell_mm, c.max_cells, c.frames)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{(min_seen, dilate): background mask} of a case's payload by the restatement (read-only), checked against what is known."""
    c, m = CASES[name], model_of(name)
    out = {}
    for p in c.params:
        mask = m.background_mask(c.payload, *p)
        mask.setflags(write=False)
        if c.expected is not None and p in c.expected:
            assert (mask == c.expected[p]).all(), (name, p)
        out[p] = mask
    return out


def check():
    """Every non-degenerate case both keeps and drops records, at one of its parameter pairs at least — and, for the count cases of a
    tile or more, at every pair."""
    for c in cases():
        masks = reference(c.name)
        if c.degenerate:
            continue
        mixed = [0 < int(m.sum()) < m.shape[0] for m in masks.values()]
        assert any(mixed), c.name
        if c.name.startswith("count") and c.payload.shape[0] >= 63:
            assert all(mixed), c.name
