"""The expectations of tests/cluster_scale_cases.py, checked without a GPU. Every builder, at a size parameter of at most 4 096
records (fewer copies, shorter rows, smaller bricks: the same code path as the full size), equals the brute force
(tests/np_clusters.py labels): labels, sizes and the cluster count. objects_from_labels_grouped equals objects_from_labels, the
definition, byte for byte on every case of cluster_cases.cases() and on windows that keep nothing and everything. At full size every
builder's labels equal an independent neighbour-graph labelling where scipy imports (cKDTree.query_pairs at tolerance + 0.5, the pairs
re-checked as integers, connected_components, the labels by np.minimum.at), and the builders' own asserts hold: the tile conditions,
the size spectrum, the faces touched.
Time on an 8-core build machine without a GPU, one process: 32 s for the whole file — the neighbour graphs at full size 23 s of it
(tiled_random 5.3 s, the others 2.3 to 3.7 s each, the builders' own time included), the reduced sizes against the brute force 3 s,
the grouped restatement 5 s, the full-size asserts 1 s with the builders cached."""
import numpy as np
import pytest

import cluster_cases as K
import cluster_scale_cases as SC
import np_cluster_objects as NO
import np_clusters as N

# name -> (builder, arguments of the reduced size, arguments of the full size)
BUILDERS = {
    "tiled_random": (SC.tiled_random, (2, 257), ()),
    "snake": (SC.snake, (False, 61, 8, 8), (False,)),
    "snake_cut": (SC.snake, (True, 61, 8, 8), (True,)),
    "giant_and_dust": (SC.giant_and_dust, ((12, 12, 8), (12, 12, 12), 16), ()),
    "bricks": (SC.bricks, (27, (4, 4, 9)), ()),
    "bricks_shuffled": (SC.bricks, (27, (4, 4, 9), True), (SC.BRICKS[0], SC.BRICKS[1], True)),
    "bricks_prefix": (SC.bricks, (27, (4, 4, 9), False, 20 * 144 + 77), (700, SC.BRICKS[1], False, 2097153)),
}


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_reduced_builder_equals_the_brute_force(name):
    build, reduced, _ = BUILDERS[name]
    rec, tol, labels, sizes = build(*reduced)
    n = rec.shape[0]
    assert 1000 < n <= 4096 and labels.shape == sizes.shape == (n,) and labels.dtype == sizes.dtype == np.int32
    assert not rec.flags.writeable and not labels.flags.writeable and not sizes.flags.writeable
    lab, siz, n_clusters = N.labels(rec, tol)
    assert (labels == lab).all() and (sizes == siz).all()
    assert int((labels == np.arange(n)).sum()) == n_clusters > 0
    assert ((rec[:, 4].astype(np.int64) & 0xFF00) != 0).all(), "the high byte of short 4 is set on every record"


def test_reduced_sizes_keep_what_the_clouds_are_for():
    """More than one cluster size in every reduced cloud but the whole snake and the bricks, a cut brick in the prefix."""
    spectrum = {name: sorted(set(b(*reduced)[3].tolist())) for name, (b, reduced, _) in BUILDERS.items()}
    assert len(spectrum["tiled_random"]) > 5 and spectrum["snake"] == [64 * 61 + 63 * 3] and spectrum["giant_and_dust"] == [1, 2, 1152]
    assert spectrum["snake_cut"][0] == 61 and len(spectrum["snake_cut"]) >= 4
    assert spectrum["bricks"] == spectrum["bricks_shuffled"] == [144] and spectrum["bricks_prefix"] == [77, 144]


WINDOWS = ((1, 0), (1, 1), (2, 0), (2, 5), (3, 0), (70, 0), (5000, 0), (33, 64), (2 ** 31 - 1, 2 ** 31 - 1))


@pytest.mark.parametrize("name", sorted(c[0] for c in K.cases()))
def test_grouped_restatement_is_the_loop_restatement(name):
    _, rec, params, _ = next(c for c in K.cases() if c[0] == name)
    _, _, _, lab, sizes = K.reference(name)
    nothing = everything = False
    for lo, hi in (params[1:],) + WINDOWS:
        table, object_of = NO.objects_from_labels(rec, lab, sizes, lo, hi)
        g_table, g_object_of = NO.objects_from_labels_grouped(rec, lab, sizes, lo, hi)
        assert g_table.dtype == table.dtype and g_table.shape == table.shape and g_table.tobytes() == table.tobytes(), (name, lo, hi)
        assert g_object_of.dtype == object_of.dtype and g_object_of.tobytes() == object_of.tobytes(), (name, lo, hi)
        nothing |= table.shape[0] == 0
        everything |= rec.shape[0] > 0 and bool((object_of >= 0).all())
    assert nothing and (everything or rec.shape[0] == 0)


def test_grouped_restatement_on_a_reduced_cloud_of_every_builder():
    for name, (build, reduced, _) in BUILDERS.items():
        rec, _, labels, sizes = build(*reduced)
        for lo, hi in ((1, 0), (2, 0), (2, 2), (62, 200), (145, 0)):
            table, object_of = NO.objects_from_labels(rec, labels, sizes, lo, hi)
            g_table, g_object_of = NO.objects_from_labels_grouped(rec, labels, sizes, lo, hi)
            assert g_table.tobytes() == table.tobytes() and g_object_of.tobytes() == object_of.tobytes(), (name, lo, hi)


def neighbour_graph_labels(rec, tol):
    """(labels, sizes) from the graph of all pairs within tol: a k-d tree proposes the pairs within tol + 0.5, integers decide."""
    spatial = pytest.importorskip("scipy.spatial")
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    xyz = rec[:, :3].astype(np.int64)
    n = xyz.shape[0]
    pairs = spatial.cKDTree(xyz.astype(np.float64)).query_pairs(tol + 0.5, output_type="ndarray")
    d = xyz[pairs[:, 0]] - xyz[pairs[:, 1]]
    pairs = pairs[(d * d).sum(axis=1) <= tol * tol]
    graph = sparse.coo_matrix((np.ones(pairs.shape[0], np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    first = np.full(n, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp], np.bincount(comp)[comp]


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_full_size_builder_equals_a_neighbour_graph_labelling(name):
    build, _, full = BUILDERS[name]
    rec, tol, labels, sizes = build(*full)
    lab, siz = neighbour_graph_labels(rec, tol)
    assert (labels == lab).all() and (sizes == siz).all()


def test_full_size_clouds_are_what_the_gpu_tests_need():
    """The builders assert their tile conditions themselves; here: the counts, the spectra and the faces."""
    T = SC.TILE
    rec, tol, labels, sizes = SC.tiled_random()
    n = rec.shape[0]
    assert n == 11 ** 3 * 2049 == 2727219 and (n + T - 1) // T == 1332 > 1025 and tol == 20
    kept, pts = SC.tiles_of(sizes >= 3)
    assert ((kept > 0) & (kept < pts)).all(), "the last, partial tile too"
    firsts = labels == np.arange(n)
    assert firsts.sum() > 4 * 65536 and (firsts[1024 * T:].sum() > 0) and len(set(sizes.tolist())) > 20
    per_tile, _ = SC.tiles_of(firsts)
    assert per_tile.min() > 0 and np.cumsum(per_tile)[1023] > 65536        # ranks beyond max_objects in most tiles, past tile 1024 too
    rec, tol, labels, sizes = SC.snake()
    assert rec.shape[0] == 1024 * 1021 + 1023 * 3 == 1048573 and (sizes == rec.shape[0]).all() and (labels == 0).all() and tol == 3
    assert rec[:, 0].min() == -32768 and rec[:, 1].max() == 32767
    rec, tol, labels, sizes = SC.snake(True)
    cuts = SC.snake_cuts(1023)
    assert 190 <= len(cuts) <= 210 and {0, 1022, 511, 512} <= set(cuts) and rec.shape[0] == 1048573 - 3 * len(cuts)
    spectrum = sorted(set(sizes.tolist()))
    assert spectrum[0] == 1021 and spectrum[-1] > 64 * T and len(spectrum) >= 4 and (labels == np.arange(rec.shape[0])).sum() == len(cuts) + 1
    rec, tol, labels, sizes = SC.giant_and_dust()
    assert rec.shape[0] == 1048576 + 499200 + 3900 and sorted(set(sizes.tolist())) == [1, 2, 1048576] and tol == 2
    assert (sizes == 2).sum() == 2 * 3900 and (sizes == 1).sum() == 499200 - 3900
    for shuffled in (False, True):
        rec, tol, labels, sizes = SC.bricks(shuffled=shuffled)
        assert rec.shape[0] == 1200000 and (sizes == 3000).all() and (labels == np.arange(rec.shape[0])).sum() == 400 and tol == 3
        assert rec[:, 1].max() <= 32767 and rec[:, 2].min() == -32768
    border = np.arange(T, 1200000, T)
    lab = SC.bricks()[2]
    assert (lab[border - 1] == lab[border]).sum() >= border.shape[0] - 4, "all tile borders but those on multiples of 3000 lie inside a brick"
    rec, tol, labels, sizes = SC.bricks(700, SC.BRICKS[1], False, 2097153)
    assert rec.shape[0] == 2097153 == 1024 * T + 1 and sorted(set(sizes.tolist())) == [153, 3000] and (sizes == 153).sum() == 153
    assert (rec == SC.bricks(700)[0][:2097153]).all()
