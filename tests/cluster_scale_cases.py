"""Clouds of working size for the Euclidean cluster and object-table tests (tests/test_clusters_scale.py on the GPU,
tests/test_cluster_scale_cases_cpu.py without one): one to 2.7 million records whose clusters are known WITHOUT a pair loop. Every
builder is deterministic, cached, and returns (records [n, 5] int16, tolerance_mm, labels int32 [n], sizes int32 [n]), all read-only:
labels[i] is the smallest input index of record i's cluster, sizes[i] its record count. Both come from a COMPONENT ID that the
construction knows (from_components: np.minimum.at and np.bincount); no builder tests a distance. The input order of every cloud but
the unshuffled bricks is one fixed permutation, so cluster order, input order and cell order all differ. Colours: with_colour.
Every builder takes its size as parameters — tests/test_cluster_scale_cases_cpu.py runs the same code at 4 096 records and fewer
against the brute force — and checks what its full size is FOR (tiles, size spectrum, faces) where the size is large enough to ask."""
import functools

import numpy as np

import cluster_cases as K
import radius_outlier_cases as RC

TILE = 2048                     # records per tile (kTilePoints)
# (copies per axis, records of the small cloud, pitch, permutation seed): 11^3 x 2049 = 2 727 219 records, 1 332 tiles
TILED = (11, 2049, 363, 41)
# (records per row, rows per layer, layers): 1024 rows of 1021 and 1023 bridges of 3 = 1 048 573 records
SNAKE = (1021, 32, 32)
# (slab shape, dust shape, one dumbbell per so many dust nodes): 1 048 576 + 499 200 + 3 900 = 1 551 676 records
GIANT = ((128, 128, 64), (80, 80, 78), 128)
# (bricks, records per axis of a brick): 400 x 3000 = 1 200 000 records
BRICKS = (400, (10, 10, 30))


def from_components(comp):
    """(labels, sizes) of records whose component ids (any integers in 0 .. n - 1) are comp: the smallest index of every id, its count."""
    comp = np.asarray(comp, np.int64)
    n = comp.shape[0]
    assert n == 0 or (comp.min() >= 0 and comp.max() < n)
    first = np.full(n, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    labels = first[comp].astype(np.int32)
    sizes = np.bincount(comp, minlength=max(n, 1))[comp].astype(np.int32)
    return labels, sizes


def _done(rec, tol, comp):
    labels, sizes = from_components(comp)
    rec = np.ascontiguousarray(rec)
    for a in (rec, labels, sizes):
        a.setflags(write=False)
    return rec, tol, labels, sizes


def tiles_of(mask):
    """A boolean per record -> the count of set records per tile of 2048, and the tiles' record counts."""
    starts = np.arange(0, mask.shape[0], TILE)
    return np.add.reduceat(mask.astype(np.int64), starts), np.minimum(TILE, mask.shape[0] - starts)


@functools.lru_cache(maxsize=None)
def tiled_random(copies_per_axis=TILED[0], n_small=TILED[1], pitch=TILED[2], seed=TILED[3]):
    """cluster_cases.random_cloud(n_small) (tolerance 20, mean degree 1.8: clusters of many sizes) copied to every node of a
    copies_per_axis^3 lattice of that pitch, node (i, j, k) at (i - copies_per_axis // 2) * pitch per axis, every copy with colour
    shorts of its own, the records shuffled by one fixed permutation. Records of different copies are at least pitch - (side - 1)
    apart, more than the tolerance, and the definition does not change under translation: the components are the small cloud's
    (cluster_cases.reference("count<n_small>")), copy by copy. The pitch is no multiple of the tolerance: every copy meets the cell
    grid at another phase. With min_size 3 every complete tile of 2048 records has kept and dropped records."""
    tol = K.RANDOM_TOL
    small = K.random_cloud(n_small)
    xyz = small[:, :3].astype(np.int64)
    side = int((xyz.max(axis=0) - xyz.min(axis=0)).max()) + 1
    assert pitch - (side - 1) > tol, "neighbouring copies must be more than the tolerance apart"
    assert pitch % tol != 0, "every copy at another phase of the cell grid"
    small_labels = np.asarray(K.reference(f"count{n_small}")[3], np.int64)
    copies = copies_per_axis ** 3
    parts = []
    for c in range(copies):
        node = np.array([c // copies_per_axis ** 2, (c // copies_per_axis) % copies_per_axis, c % copies_per_axis])
        parts.append(RC.with_colour(xyz + (node - copies_per_axis // 2) * pitch, seed=1000 + c))
    comp = (np.arange(copies)[:, None] * n_small + small_labels[None, :]).reshape(-1)
    order = np.random.default_rng(seed).permutation(copies * n_small)
    rec, tol, labels, sizes = _done(np.concatenate(parts)[order], tol, comp[order])
    kept, pts = tiles_of(sizes >= K.RANDOM_MIN)
    full = pts == TILE
    assert ((kept[full] > 0) & (kept[full] < TILE)).all(), "a tile of 2048 records with nothing kept, or nothing dropped"
    return rec, tol, labels, sizes


def snake_cuts(bridges):
    """The bridges the cut variant removes: the first, the last, two adjacent ones in the middle, and every fourth of the first three
    quarters — the last quarter stays one piece."""
    return tuple(sorted({0, bridges - 1, bridges // 2, bridges // 2 + 1} | set(range(3, 3 * bridges // 4, 4))))


@functools.lru_cache(maxsize=None)
def snake(cut=False, row=SNAKE[0], rows_per_layer=SNAKE[1], layers=SNAKE[2]):
    """ONE path at tolerance 3: rows of `row` records along x at pitch 1, rows 4 apart in y, layers 4 apart in z (rows are not adjacent
    to each other); row R is joined to row R + 1 at alternating ends — the right end behind an even row — by a BRIDGE of three records
    on the straight line between the two row ends, 1, 2 and 3 from the first: in y within a layer (up in even layers, back down in odd
    ones), in z from a layer's last row to the next layer's first. The rows start on the x = -32768 face, the last row of every even
    layer lies on the y = +32767 face. cut: the bridges of snake_cuts() are left out, all three records of each: the component id of a
    row, and of the bridge behind it, is the number of removed bridges in front of it, so a component is a run of consecutive rows.
    Shuffled by one fixed permutation."""
    tol = 3
    rows = rows_per_layer * layers
    removed = np.zeros(rows - 1, bool)
    if cut:
        removed[list(snake_cuts(rows - 1))] = True
    R = np.arange(rows)
    layer = R // rows_per_layer
    yi = np.where(layer % 2 == 0, R % rows_per_layer, rows_per_layer - 1 - R % rows_per_layer)
    x0, y0, z0 = -32768, 32767 - 4 * (rows_per_layer - 1), -100
    at = np.stack([np.zeros(rows, np.int64), y0 + 4 * yi, z0 + 4 * layer], axis=1)          # a row's y and z
    comp_of_row = np.concatenate([[0], np.cumsum(removed)])
    row_xyz = np.repeat(at, row, axis=0)
    row_xyz[:, 0] = x0 + np.tile(np.arange(row), rows)
    kept = np.nonzero(~removed)[0]
    end_x = np.where(kept % 2 == 0, x0 + row - 1, x0)
    step = (at[kept + 1] - at[kept]) // 4                                                # one of (0, +-1, 0), (0, 0, 1)
    assert (np.abs(step).sum(axis=1) == 1).all() and (step * 4 == at[kept + 1] - at[kept]).all()
    bridge_xyz = (at[kept][:, None, :] + step[:, None, :] * np.arange(1, 4)[None, :, None]).reshape(-1, 3)
    bridge_xyz[:, 0] = np.repeat(end_x, 3)
    xyz = np.concatenate([row_xyz, bridge_xyz])
    comp = np.concatenate([np.repeat(comp_of_row, row), np.repeat(comp_of_row[kept], 3)])
    n = xyz.shape[0]
    assert n == rows * row + 3 * kept.shape[0]
    order = np.random.default_rng(42).permutation(n)
    rec, tol, labels, sizes = _done(RC.with_colour(xyz[order]), tol, comp[order])
    # the sizes are arithmetic: a component of m consecutive rows has m rows and m - 1 bridges
    runs = np.diff(np.concatenate([[0], np.nonzero(removed)[0] + 1, [rows]]))
    assert sorted(np.unique(labels, return_counts=True)[1].tolist()) == sorted((runs * row + 3 * (runs - 1)).tolist())
    assert xyz[:, 0].min() == -32768 and xyz[:, 1].max() == 32767
    if cut:
        assert (runs == 1).any(), "one component of a single row"
        assert runs.shape[0] == removed.sum() + 1
        if n > 4 * 64 * TILE:
            assert (runs * row + 3 * (runs - 1)).max() > 64 * TILE, "one component of more than 64 tiles of records"
    return rec, tol, labels, sizes


@functools.lru_cache(maxsize=None)
def giant_and_dust(slab=GIANT[0], dust=GIANT[1], dumbbell_every=GIANT[2]):
    """A slab: a lattice of pitch 2 at tolerance 2, ONE cluster, placed where its x and y sums leave 32 bits in either sign; beside it
    dust on a lattice of pitch 7, every record a cluster of its own, but every dumbbell_every-th node a DUMBBELL: a second record 2
    along x (5 from the next node). Dust and slab are 12 apart. Shuffled: every tile of 2048 records holds slab records, which share
    one root across all workgroups, among hundreds of other roots."""
    tol = 2
    corner = np.array([20000, -20000 - 2 * (slab[1] - 1), -64])
    s = 2 * np.indices(slab).reshape(3, -1).T + corner
    d = 7 * np.indices(dust).reshape(3, -1).T + corner + np.array([2 * (slab[0] - 1) + 12, 0, 0])
    twins = np.arange(0, d.shape[0], dumbbell_every)
    xyz = np.concatenate([s, d, d[twins] + np.array([2, 0, 0])])
    comp = np.concatenate([np.zeros(s.shape[0], np.int64), 1 + np.arange(d.shape[0]), 1 + twins])
    order = np.random.default_rng(43).permutation(xyz.shape[0])
    rec, tol, labels, sizes = _done(RC.with_colour(xyz[order]), tol, comp[order])
    assert np.unique(sizes).tolist() == [1, 2, s.shape[0]]
    if xyz.shape[0] >= 64 * TILE:
        in_slab, pts = tiles_of(sizes == s.shape[0])
        assert (in_slab > 0).all() and (pts - in_slab >= 100)[pts == TILE].all(), "a tile without the slab, or without a hundred others"
        assert s[:, 0].sum() > 2 ** 32 and s[:, 1].sum() < -2 ** 32
    return rec, tol, labels, sizes


@functools.lru_cache(maxsize=None)
def bricks(n_bricks=BRICKS[0], dims=BRICKS[1], shuffled=False, count=None):
    """n_bricks bricks, each a dims lattice of pitch 3 at tolerance 3 (x fastest, then y, then z), on a 10 x 10 x (as many as it
    takes) lattice of bricks with gaps of 13 and more. NOT shuffled, brick after brick: a brick of 3000 records spans two or three
    consecutive tiles of 2048 and the tile borders fall inside clusters; shuffled=True: the same cloud under one fixed permutation.
    count: the first `count` records of the unshuffled cloud only — a prefix of a lattice in raster order is whole layers, whole rows
    and a piece of one row, connected, so the cut brick stays one (smaller) cluster and the component id is still the brick."""
    tol = 3
    per = dims[0] * dims[1] * dims[2]
    cell = np.indices(dims[::-1]).reshape(3, -1).T[:, ::-1]                              # x fastest
    b = np.arange(n_bricks)
    pitch = 3 * (np.array(dims) - 1) + 13
    origin = np.stack([b % 10, (b // 10) % 10, b // 100], axis=1) * pitch + np.array([-300, 32767 - 10 * pitch[1], -32768])
    xyz = (origin[:, None, :] + 3 * cell[None, :, :]).reshape(-1, 3)
    comp = np.repeat(b, per)
    if shuffled:
        assert count is None
        order = np.random.default_rng(44).permutation(xyz.shape[0])
        xyz, comp = xyz[order], comp[order]
    rec = RC.with_colour(xyz)
    if count is not None:
        assert 0 < count <= rec.shape[0] and count % per != 0, "the prefix cuts a brick"
        rec, comp = rec[:count], comp[:count]
    rec, tol, labels, sizes = _done(rec, tol, comp)
    if not shuffled and per > TILE:
        last, first = labels[TILE - 1::TILE], labels[TILE::TILE]                          # either side of every tile border
        assert (last[:first.shape[0]] == first).mean() > 0.9, "tile borders inside clusters"
    return rec, tol, labels, sizes


def behind_the_count(n):
    """n records on a lattice of pitch 3 far from every cloud of this module: one more cluster at any tolerance from 3 up, if read."""
    i = np.arange(n)
    return RC.with_colour(np.stack([3 * (i % 64) - 20000, 3 * ((i // 64) % 64) + 5000, 3 * (i // 4096) + 20000], axis=1), seed=7)
