"""Radius outlier removal without a GPU: the brute-force restatement (tests/np_radius_outlier.py) against a second, independently
written formulation (a dictionary of cells in plain Python) over every shared case; the random cases' kept shares, so that none
degenerates silently; the analytic expectations of the constructed cases; and the -O flag surface of pcs-multicamera-optimized
(help text, every malformed form refused with status 2 before a context is created)."""
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

import np_radius_outlier as N
import radius_outlier_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
CENTRAL = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-multicamera-optimized")
CASES = {c[0]: c for c in K.cases()}


def cells_keep_mask(records, radius_mm, min_neighbors):
    """The definition once more, sharing nothing with the restatement: Python integers, a dictionary of cells of edge radius_mm
    (floor division), the 27 cells around each record."""
    pts = [tuple(int(v) for v in row[:3]) for row in np.asarray(records, np.int16).reshape(-1, 5)]
    r, r2 = int(radius_mm), int(radius_mm) ** 2
    cells = defaultdict(list)
    for i, (x, y, z) in enumerate(pts):
        cells[(x // r, y // r, z // r)].append(i)
    keep = np.zeros(len(pts), bool)
    for i, (x, y, z) in enumerate(pts):
        cx, cy, cz = x // r, y // r, z // r
        found = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    for j in cells.get((cx + dx, cy + dy, cz + dz), ()):
                        if j != i:
                            a, b, c = pts[j]
                            found += (x - a) ** 2 + (y - b) ** 2 + (z - c) ** 2 <= r2
        keep[i] = found >= min_neighbors
    return keep


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_agrees_with_a_dictionary_of_cells(name):
    _, rec, r, k, expected = CASES[name]
    mask = K.reference(name)
    assert (cells_keep_mask(rec, r, k) == mask).all()
    if expected is not None:
        assert (mask == expected).all()
    kept = N.radius_outlier(rec, r, k)
    assert kept.dtype == np.int16 and (kept == rec[mask]).all()           # all five shorts, input order


def test_random_cases_keep_and_drop():
    for name, rec, r, k, share in K.random_cases():
        mask = K.reference(name)
        assert 0 < mask.sum() < rec.shape[0], name
        assert abs(100.0 * mask.mean() - share) <= 2.0, (name, 100.0 * mask.mean(), share)


def test_constructed_cases_say_what_they_are_for():
    rec, is_surface = K.surface_scatter()
    assert is_surface.sum() == 5000 and (K.reference("surface_scatter") == is_surface).all()
    rec, want = K.extremes()
    # the lone records come in pairs 65535 mm apart on one axis, equal on the others: one apart if a difference wrapped at 16 bits
    lone = rec[~want]
    d = lone[0::2, :3].astype(np.int64) - lone[1::2, :3].astype(np.int64)
    assert lone.shape[0] == 6 and sorted(np.abs(d).sum(axis=1)) == [65535] * 3 and ((d != 0).sum(axis=1) == 1).all()
    assert (np.abs(d.astype(np.int16)).sum(axis=1) == 1).all()
    for m in (2, 65, 256):
        assert (K.duplicates(m)[:, :3] == K.duplicates(m)[0, :3]).all()
    sat = K.saturation()[:, :3].astype(np.int64)
    assert ((sat[:, None] - sat[None]) ** 2).sum(axis=2).max() <= 200 ** 2
    with pytest.raises(AssertionError):
        N.keep_mask(K.duplicates(256), 1, 256)                            # 256 is not a legal min_neighbors
    assert (K.identical(4)[:, :3] == K.identical(4)[0, :3]).all()


def test_result_does_not_depend_on_record_order():
    _, rec, r, k, _ = CASES["count2049"]
    perm = np.random.default_rng(5).permutation(rec.shape[0])
    assert (N.keep_mask(rec[perm], r, k) == K.reference("count2049")[perm]).all()


# ---- the dense-box restatement, and the clouds of working size ------------------------------------
def counts_that_matter(rec, r, spread=False):
    """Every min_neighbors at which the brute-force mask of rec changes, and one beyond the last (legal ones only); spread: at most six
    of them, both ends among them."""
    p = rec[:, :3].astype(np.int64)
    within = (((p[:, None] - p[None]) ** 2).sum(axis=2) <= r * r).sum(axis=1) - 1
    ks = sorted({int(k) for k in within if k >= 1} | {int(within.max()) + 1})
    ks = [k for k in ks if 1 <= k <= 255]
    return ks if len(ks) <= 6 or not spread else [ks[i * (len(ks) - 1) // 5] for i in range(6)]


def small_lattice():
    return K.lattice_box((11, 9, 7), (-5, 32759, -32768))[0]


def random_60():
    return K.with_colour(np.random.default_rng(21).integers(-30, 30, (3000, 3)) + np.array([0, -32738, 32737]))


DENSE = ([("saturation", K.saturation, r, k) for r, k in ((1, 1), (6, 1), (6, 2), (6, 5))] +
         [("duplicates65", lambda: K.duplicates(65), 1, k) for k in (64, 65)] + [("duplicates65", lambda: K.duplicates(65), 3, 64)] +
         [("lattice_11x9x7", small_lattice, r, None) for r in (1, 2, 3)] +
         [("random_60", random_60, r, "spread") for r in (1, 2, 5)])


@pytest.mark.parametrize("name,cloud,r,k", DENSE, ids=[f"{d[0]}_r{d[2]}_k{d[3]}" for d in DENSE])
def test_dense_box_restatement_agrees_with_brute_force(name, cloud, r, k):
    """keep_mask_dense_box is pinned to the pair loop before anything is held to it. k None: every min_neighbors that changes the
    answer; "spread": six of those. (saturation() at its own radius of 200 is beyond the size condition — 500^3 points — and is asked at radii the box holds.)"""
    rec = cloud()
    ks = [k] if isinstance(k, int) else counts_that_matter(rec, r, spread=k == "spread")
    kept = set()
    for m in ks:
        want = N.keep_mask(rec, r, m)
        assert (N.keep_mask_dense_box(rec, r, m) == want).all(), (name, r, m)
        kept.add(int(want.sum()))
    assert isinstance(k, int) or len(kept) > 1                   # (the sweep really moves the answer)


def test_dense_box_restatement_refuses_a_box_it_cannot_hold():
    with pytest.raises(AssertionError):
        N.keep_mask_dense_box(K.saturation(), 200, 255)
    assert N.keep_mask_dense_box(np.zeros((0, 5), np.int16), 5, 1).shape == (0,)


def test_tiled_cubes_pairs_of_copies_by_brute_force():
    """tiled_cubes(2), 8 copies, 49 288 records: the per-copy-pair form. The padded box of the whole cloud is 827^3, beyond the dense-box
    restatement, so for each axis in turn the two copies that differ along it only (12 322 records, whole copies, everything else more
    than a radius away) go through the pair loop and must give the expected mask's rows. About 7 s per axis here."""
    rec, want = K.tiled_cubes(2)
    side, r, k, _, share = K.CUBES[0]
    assert rec.shape[0] == 8 * 6161 and abs(100.0 * want.mean() - share) <= 2.0
    xyz = rec[:, :3].astype(np.int64)
    upper = xyz >= -(side // 2)                          # per axis: in the copy at offset 0 (the other one ends below -227)
    assert (upper.sum(axis=0) == 4 * 6161).all()
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        pick = upper[:, others[0]] & upper[:, others[1]]
        assert pick.sum() == 2 * 6161 and 0 < upper[pick, axis].sum() < pick.sum()
        assert (N.keep_mask(rec[pick], r, k) == want[pick]).all(), axis


def test_tiled_cubes_refuses_copies_within_a_radius():
    with pytest.raises(AssertionError):
        K.tiled_cubes(2, 419)                            # a gap of exactly the radius


def test_lattice_box_analytic_mask_and_conditions():
    shape, origin, n, table = K.LATTICE
    rec, inside = K.lattice_box()
    assert rec.shape[0] == n > 1048576
    xyz = rec[:, :3].astype(np.int64)
    assert xyz[:, 1].max() == 32767 and xyz[:, 2].min() == -32768                  # both ends of the int16 range occur
    assert np.unique(xyz, axis=0).shape[0] == n                                      # one record per point: n cells at radius 1
    assert sorted(np.unique(inside)) == [3, 4, 5, 6]
    shares = {}
    for k in (5, 6):
        want = inside >= k
        assert (N.keep_mask_dense_box(rec, 1, k) == want).all(), k
        shares[(1, k)] = 100.0 * want.mean()
    interior = tuple(e - 4 for e in shape)
    mask = N.keep_mask_dense_box(rec, 2, 32)
    assert mask.sum() == interior[0] * interior[1] * interior[2]                   # two layers off every face
    shares[(2, 32)] = 100.0 * mask.mean()
    for r, k, share in table:
        assert abs(shares[(r, k)] - share) <= 0.1, (r, k, shares[(r, k)])


# ---- the CLI's flag surface ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def central():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert os.path.exists(CENTRAL)
    return CENTRAL


def run(*args, timeout=120):
    return subprocess.run(list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_help_lists_the_option(central):
    r = run(central, "-h")
    assert r.returncode == 0 and "-O <radius_mm,min_neighbors>" in r.stdout


MALFORMED = ["", "20", "20,", ",3", "20,3,1", "20;3", "20,3x", "x,3", "0,3", "1001,3", "20,0", "20,256", "-5,3", "20,-1", "2.5,3",
             "99999999999999999999,3", "20, 3 "]


@pytest.mark.parametrize("arg", MALFORMED)
def test_malformed_option_exits_2_before_any_context(central, arg):
    for cmd in ([central, "-i", "synth:64x48", "-N", "2", "-q", "-r", "1", "-O", arg],
                [central, "-c", "127.0.0.1:1", "-q", "-O", arg]):
        r = run(*cmd)
        assert r.returncode == 2, (cmd, r.stderr)
        assert "-O" in r.stderr and "pcs_create" not in r.stderr and "Connection failed" not in r.stderr


def test_option_with_sharding_is_refused_in_one_line(central):
    r = run(central, "-i", "synth:64x48", "-N", "2", "-q", "-G", "2", "-O", "20,3")
    assert r.returncode == 2 and "-G" in r.stderr and "-O" in r.stderr and len(r.stderr.strip().splitlines()) == 1


def test_well_formed_option_gets_past_the_parser(central):
    """A good -O is not what stops the program: with an edge that does not exist it fails at the connection, status 1."""
    r = run(central, "-c", "127.0.0.1:1", "-q", "-O", "1000,255")
    assert r.returncode == 1 and "Connection failed" in r.stderr and "-O" not in r.stderr
