"""Radius outlier removal at the sizes it runs at (tests/test_radius_outlier.py stops at 65 536 records): clouds of one and two
million records whose keep masks need no pair loop (tests/radius_outlier_cases.py: tiled_cubes, lattice_box), so that
  the slot scan      (pcs_outlier_cell_scan_kernel) takes a second and a third pass of 1024 slot tiles and its carry lane holds data,
  the tile scan      (pcs_scan_kernel over the control block's one-entry table) takes a second chunk, the emit launch a 1 025th tile,
  the hash table     is filled to its design load — one cell per record, half the slots — with whole faces of the cloud on the ends of
                     the int16 range, where the flag kernel skips the cells that do not exist,
  a probe sequence   runs off slot `slots - 1` back to slot 0, in the insert and in the flag kernel's lookups (the hash is restated
                     here, in numpy, only to BUILD that input),
  the workspace      serves a small call after a large one.
Every comparison is bytes and counts. Expectations: the brute-force restatement (tests/np_radius_outlier.py keep_mask) of the small
cloud, tiled; index arithmetic; the dense-box restatement (keep_mask_dense_box), which tests/test_radius_outlier_cpu.py pins to brute
force; the CPU oracle's voxel grid."""
import functools

import numpy as np
import pytest

import np_radius_outlier as N
import radius_outlier_cases as K
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import POINT_SHORTS

pytestmark = pytest.mark.gpu

GUARD = 64                      # bytes of 0xA5 in front of the output, behind the kept records and behind the worst-case output
N_MAX = K.TILED[2]              # 2 113 223
SENTINEL = 0x5A5A5A5A
TILE = 2048                     # records per tile, slots per slot tile (kTilePoints)
SCAN_LANES = 1024               # tiles per pass of either scan


# ---- csrc/pcs_kernels_outlier.hip's index arithmetic, restated: used to say which passes a size reaches and to build the wrap-around
# ---- cloud, never for an expectation
def outlier_slots(capacity):
    return (max(2 * capacity, 1) + TILE - 1) // TILE * TILE


def cell_of(v, r):
    return np.asarray(v, np.int64) // r + 32768                      # floor, 0 .. 65535


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


def passes(tiles):
    return (tiles + SCAN_LANES - 1) // SCAN_LANES


class Arena:
    """An input and an output payload of N_MAX records at any 2-byte phase, two count words."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.inp = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.out = ctx.device_malloc(GUARD + 64 + 10 * N_MAX + GUARD + 64)
        self.words = ctx.device_malloc(64)          # [0] the kept count, [4] the counted form's input count
        assert self.inp % 16 == 0 and self.out % 16 == 0

    def free(self):
        for p in (self.inp, self.out, self.words):
            self.ctx.device_free(p)

    def run(self, rec, r, k, in_phase=4, out_phase=4, d_count=None, max_points=None):
        """rec at phase in_phase (bytes mod 16; 4 = the reference's buffer + 2 shorts) -> (kept records, kept count) written at
        out_phase; everything in front of d_out, behind the kept records and behind the worst-case output must stay 0xA5. d_count: the
        counted form with that count on the device and max_points as its capacity (rec may be shorter than the capacity)."""
        ctx = self.ctx
        cap = rec.shape[0] if d_count is None else max_points
        assert rec.shape[0] <= cap <= N_MAX
        d_in, d_out = self.inp + in_phase, self.out + GUARD + out_phase
        if rec.shape[0]:
            ctx.memcpy_h2d(d_in, np.ascontiguousarray(rec))
        span = GUARD + out_phase + 10 * cap + GUARD
        ctx.memcpy_h2d(self.out, np.full(span, 0xA5, np.uint8))
        ctx.memcpy_h2d(self.words, np.array([SENTINEL, 0 if d_count is None else d_count], np.int32))
        if d_count is None:
            ctx.radius_outlier_device(d_in, cap, r, k, d_out, POINT_SHORTS * cap, self.words)
        else:
            ctx.radius_outlier_device_counted(d_in, self.words + 4, cap, r, k, d_out, POINT_SHORTS * cap, self.words)
        ctx.synchronize()
        got = np.empty(span, np.uint8)
        ctx.memcpy_d2h(got, self.out)
        words = np.empty(2, np.int32)
        ctx.memcpy_d2h(words, self.words)
        kept = int(words[0])
        assert 0 <= kept <= cap, kept
        lo = GUARD + out_phase
        assert (got[:lo] == 0xA5).all(), "bytes in front of d_out were written"
        assert (got[lo + 10 * kept:] == 0xA5).all(), "bytes behind the kept records were written"
        return got[lo:lo + 10 * kept].copy().view(np.int16).reshape(kept, 5), kept


@pytest.fixture(scope="module")
def ctx():
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs) as c:
        yield c


@pytest.fixture(scope="module")
def arena(ctx):
    a = Arena(ctx)
    yield a
    a.free()


def assert_kept(got, kept, want, what):
    assert kept == want.shape[0], (what, kept, want.shape[0])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {kept} kept records differ, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


@functools.lru_cache(maxsize=None)
def lattice_dense(n, r, k):
    """keep_mask_dense_box of the lattice box's first n records, once per process."""
    mask = N.keep_mask_dense_box(K.lattice_box()[0][:n], r, k)
    mask.setflags(write=False)
    return mask


def small(name):
    _, rec, r, k, _ = next(c for c in K.cases() if c[0] == name)
    return rec, r, k, rec[K.reference(name)]


def test_the_sizes_reach_the_second_passes():
    """What the cases of this module are for, from the restated arithmetic: passes of the slot scan, chunks of the tile scan."""
    tiles = (N_MAX + TILE - 1) // TILE
    assert (tiles, passes(tiles)) == (1032, 2) and (outlier_slots(N_MAX) // TILE, passes(outlier_slots(N_MAX) // TILE)) == (2064, 3)
    n = K.LATTICE[2]
    assert (outlier_slots(n) // TILE, passes(outlier_slots(n) // TILE)) == (1040, 2)
    assert outlier_slots(1048576) // TILE == 1024 and outlier_slots(1048577) // TILE == 1025
    assert outlier_slots(1024) == 2048 and outlier_slots(0) == 2048


def test_tiled_cubes_whole(arena):
    """2 113 223 records at (20, 3): three passes of the slot scan, two chunks of the tile scan, 1032 emit tiles; 1 231 713 kept."""
    rec, mask = K.tiled_cubes()
    want = rec[mask]
    assert rec.shape[0] == N_MAX and want.shape[0] == 1231713
    got, kept = arena.run(rec, 20, 3)
    assert_kept(got, kept, want, "tiled cubes")
    again, kept_again = arena.run(rec, 20, 3)
    assert kept_again == kept and again.tobytes() == got.tobytes()


@pytest.mark.parametrize("cap", [1048576, 1048577])
def test_counted_form_large_capacity_small_count(arena, cap):
    """What the centre does on every frame: a capacity of a million, a count of a few thousand. 1 048 576: exactly 1024 slot tiles, one
    full pass whose carry lane holds a tile; 1 048 577: one tile in a second pass."""
    rec, r, k, want = small("cube400_r20_k3")
    got, kept = arena.run(rec, r, k, d_count=rec.shape[0], max_points=cap)
    assert_kept(got, kept, want, cap)


def test_counted_form_large_capacity_zero_and_clamped_count(arena):
    cap = 1048577
    rec, r, k, _ = small("cube400_r20_k3")
    got, kept = arena.run(rec, r, k, d_count=0, max_points=cap)
    assert kept == 0
    lattice = K.lattice_box()[0][:cap]
    want = lattice[lattice_dense(cap, 1, 5)]
    assert 0 < want.shape[0] < cap
    got, kept = arena.run(lattice, 1, 5, d_count=cap + 5, max_points=cap)
    assert_kept(got, kept, want, "clamped")


@pytest.mark.parametrize("r,k", [(r, k) for r, k, _ in K.LATTICE[3]])
def test_lattice_box(arena, r, k):
    """1 064 960 records, at radius 1 as many cells: the table at half load, 1040 slot tiles, the faces y = 32767 and z = -32768
    looking for cells that do not exist. Radius 1 by index arithmetic, radius 2 by the dense-box restatement."""
    rec, inside = K.lattice_box()
    mask = inside >= k if r == 1 else lattice_dense(rec.shape[0], r, k)
    assert 0 < mask.sum() < rec.shape[0]
    got, kept = arena.run(rec, r, k)
    assert_kept(got, kept, rec[mask], (r, k))


def test_chain_into_the_voxel_grid_at_size(arena, oracle):
    """counted outlier removal -> pcs_voxel_grid_device_counted on the tiled cloud, nothing waited for in between, against the CPU
    oracle's voxel grid of the expected records."""
    ctx = arena.ctx
    rec, mask = K.tiled_cubes()
    n, leaf = rec.shape[0], 40
    want = oracle.voxel_grid(np.ascontiguousarray(rec[mask]), leaf)
    assert 0 < want.shape[0] < mask.sum()
    d_mid = ctx.device_malloc(10 * n + 64)
    try:
        ctx.memcpy_h2d(arena.inp + 4, np.ascontiguousarray(rec))
        ctx.memcpy_h2d(arena.words, np.array([SENTINEL, n, SENTINEL], np.int32))
        ctx.radius_outlier_device_counted(arena.inp + 4, arena.words + 4, n, 20, 3, d_mid, POINT_SHORTS * n, arena.words)
        ctx.voxel_grid_device_counted(d_mid, arena.words, n, leaf, arena.out, POINT_SHORTS * n, arena.words + 8)
        ctx.synchronize()
        words = np.empty(3, np.int32)
        ctx.memcpy_d2h(words, arena.words)
        assert words[0] == mask.sum() and words[2] == want.shape[0], (words, mask.sum(), want.shape[0])
        got = np.empty((want.shape[0], 5), np.int16)
        ctx.memcpy_d2h(got, arena.out)
        assert_kept(got, got.shape[0], want, "voxels")
    finally:
        ctx.device_free(d_mid)


def test_small_calls_after_a_large_one(arena):
    """The workspace does not shrink: after the 2.1 M call its keep words, table and starts hold that call's values where a small
    call's layout puts other arrays."""
    rec, mask = K.tiled_cubes()
    got, kept = arena.run(rec, 20, 3)
    assert kept == mask.sum()
    for name in ("count2049", "extremes_r1"):
        rec, r, k, want = small(name)
        got, kept = arena.run(rec, r, k, 4, 4)
        assert_kept(got, kept, want, name)


# ---- probe sequences that wrap ------------------------------------------------------------------------
WRAP_CAP, WRAP_RADIUS = 1024, 1000


def wrap_cloud():
    """1024 records at radius 1000 whose table has 2048 slots: sixteen cells whose probe sequences start at slot 2047 or 2046 (eight
    each, of the 147 and 154 such cells the int16 range has at that radius; interior, no two within three cells of each other or of the
    filler), two records 1 mm apart in the middle of each — each other's only neighbour unless one was added: for the first four cells of
    each set a lone record 600 mm away, in the next cell along x, which has to find the wrapped cell from outside. The rest: a random
    cube of side 400 around the origin. Returns (records, index of the pairs' records, of the pairs with a lone neighbour, of the
    lone records)."""
    slots = outlier_slots(WRAP_CAP)
    q = np.arange(-33, 33)                                           # cells per axis: floor(v / 1000) for v in -32768 .. 32767
    assert (np.unique(cell_of(np.arange(-32768, 32768), WRAP_RADIUS)) == q + 32768).all()
    cells = np.stack(np.meshgrid(q, q, q, indexing="ij"), axis=-1).reshape(-1, 3)
    start = first_slot(cell_key(*(cells + 32768).T), slots)
    assert slots == 2048 and (start == 2047).sum() == 147 and (start == 2046).sum() == 154
    interior = (np.abs(cells + 0.5) < 32).all(axis=1) & ~(np.abs(cells + 0.5) < 4).all(axis=1)
    chosen = []
    for s in (2047, 2046):
        mine = []
        for c in cells[(start == s) & interior]:
            if all(np.abs(c - o).max() >= 3 for o in chosen + mine):
                mine.append(c)
            if len(mine) == 8:
                break
        chosen += mine
    chosen = np.array(chosen)
    # the precondition: sixteen cells, at most two start slots, both at the table's end — their probe sequences pass slot slots - 1
    assert chosen.shape == (16, 3)
    mid = chosen * WRAP_RADIUS + 500
    assert set(first_slot(cell_key(*cell_of(mid, WRAP_RADIUS).T), slots).tolist()) == {slots - 1, slots - 2}
    xyz, pairs, helped, lone = [], [], [], []
    for i, m in enumerate(mid):
        pairs += [len(xyz), len(xyz) + 1]
        xyz += [m, m + (1, 0, 0)]
        if i % 8 < 4:
            helped += pairs[-2:]
            lone.append(len(xyz))
            xyz.append(m + (600, 0, 0))
    assert (cell_of(np.array(xyz)[lone], WRAP_RADIUS) == cell_of(mid[np.arange(16) % 8 < 4], WRAP_RADIUS) + (1, 0, 0)).all()
    filler = K.cube(400, 5, n=WRAP_CAP - len(xyz))
    rec = np.concatenate([K.with_colour(np.array(xyz)), filler])
    return rec, np.array(pairs), np.array(helped), np.array(lone)


def test_probe_sequences_that_wrap_past_the_last_slot(arena):
    rec, pairs, helped, lone = wrap_cloud()
    n = rec.shape[0]
    assert n == WRAP_CAP
    orders = (np.arange(n), np.random.default_rng(17).permutation(n))
    for k in (1, 2):
        mask = N.keep_mask(rec, WRAP_RADIUS, k)
        # what the cloud was built for: a pair's record is kept at 1 only if its partner is found, at 2 only with the lone record too
        expect = np.ones(n, bool)
        if k == 2:
            expect[pairs] = False
            expect[helped] = True
        assert (mask == expect).all() and mask[lone].all()
        for order in orders:
            got, kept = arena.run(rec[order], WRAP_RADIUS, k, d_count=n, max_points=WRAP_CAP)
            assert_kept(got, kept, rec[order][mask[order]], (k, "order", int(order[0])))
