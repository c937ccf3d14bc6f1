"""Euclidean clusters without a GPU: the brute-force restatement (tests/np_clusters.py) against a second, independently written
formulation (a dictionary of cells and a breadth-first search in plain Python integers) over every shared case; the analytic cases
by their stated numbers; that every random cloud has clusters on both sides of its threshold; invariance under a permutation of the
records; the -E flag surface of pcs-multicamera-optimized (help text, every malformed form refused with status 2 before a context
is created); and the ABI names in the header, the library's export table and lib.py."""
import os
import re
import subprocess
from collections import defaultdict, deque

import numpy as np
import pytest

import cluster_cases as K
import np_clusters as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
CENTRAL = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-multicamera-optimized")
CASES = {c[0]: c for c in K.cases()}
ABI = ("pcs_cluster_filter_device", "pcs_cluster_filter_device_counted", "pcs_cluster_filter", "pcs_cluster_labels_device",
       "pcs_cluster_labels")


def cells_clusters(records, tolerance_mm):
    """The definition once more, sharing nothing with the restatement: a dictionary of cells of edge tolerance_mm (floor division),
    a breadth-first search from every unvisited record in input order over the 27 cells around each record, distances in Python
    integers. Returns (labels, sizes) as lists."""
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    pts = [tuple(int(v) for v in row[:3]) for row in rec]
    e, e2 = int(tolerance_mm), int(tolerance_mm) ** 2
    cells = defaultdict(list)
    for i, (x, y, z) in enumerate(pts):
        cells[(x // e, y // e, z // e)].append(i)
    label = [-1] * len(pts)
    size = [0] * len(pts)
    for seed in range(len(pts)):
        if label[seed] >= 0:
            continue
        label[seed] = seed                       # input order: the seed is the smallest index of its component
        members, queue = [seed], deque([seed])
        while queue:
            x, y, z = pts[queue.popleft()]
            cx, cy, cz = x // e, y // e, z // e
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dz in (-1, 0, 1):
                        for j in cells.get((cx + dx, cy + dy, cz + dz), ()):
                            if label[j] < 0 and (pts[j][0] - x) ** 2 + (pts[j][1] - y) ** 2 + (pts[j][2] - z) ** 2 <= e2:
                                label[j] = seed
                                members.append(j)
                                queue.append(j)
        for j in members:
            size[j] = len(members)
    return label, size


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_agrees_with_cells_and_breadth_first_search(name):
    _, rec, (tol, lo, hi), _ = CASES[name]
    want, keep, stats, lab, sizes = K.reference(name)
    lab2, sizes2 = cells_clusters(rec, tol)
    assert lab.tolist() == lab2 and sizes.tolist() == sizes2
    assert (lab <= np.arange(rec.shape[0])).all() and (lab[lab] == lab).all()        # label(i) <= i; a cluster's first labels itself
    keep2 = np.array([s >= lo and (hi == 0 or s <= hi) for s in sizes2], bool).reshape(-1)
    assert (keep2 == keep).all()
    assert want.dtype == np.int16 and (want == rec[keep]).all()                       # all five shorts, input order
    assert stats == {"considered": rec.shape[0], "clusters": len(set(lab2)), "kept_clusters": len({l for l, k in zip(lab2, keep2) if k}),
                     "largest": max(sizes2, default=0), "kept": int(keep2.sum())}
    K.check_expected(name, keep, stats, lab)


def test_analytic_cases_differ_where_they_should():
    a, b = K.reference("sizes_64_0")[2], K.reference("sizes_65_0")[2]
    assert a["kept_clusters"] - b["kept_clusters"] == 1 and a["kept"] - b["kept"] == 64
    assert K.reference("sizes_33_64")[2]["kept"] == sum(range(33, 65))
    assert K.reference("chain")[2]["clusters"] == 1 and K.reference("chain_cut")[2]["clusters"] == 2
    lo, hi = sorted([K.CHAIN_CUT + 1, K.CHAIN_N - K.CHAIN_CUT - 1])
    assert lo < CASES["chain_cut"][2][1] <= hi                                        # min_size lies between the two parts
    assert K.reference("bridge")[2]["clusters"] == 1 and K.reference("bridge_gone")[2]["clusters"] == 2
    with pytest.raises(AssertionError):
        N.cluster_filter(K.pair((1, 0, 0)), 1, 3, 2)                                  # max_size below min_size is not legal
    with pytest.raises(AssertionError):
        N.cluster_filter(K.pair((1, 0, 0)), 1001, 1, 0)


def test_random_clouds_have_clusters_on_both_sides_of_the_threshold():
    for name, rec, (tol, lo, hi) in K.random_cases():
        _, keep, stats, lab, sizes = K.reference(name)
        per_cluster = sizes[lab == np.arange(rec.shape[0])]
        assert (per_cluster < lo).sum() >= 3 and (per_cluster >= lo).sum() >= 3, name
        assert 0 < stats["kept"] < rec.shape[0], name
        assert len(set(per_cluster.tolist())) >= 4, name                              # clusters of many sizes


@pytest.mark.parametrize("name", ["count2049", "sizes_33_64", "chain_cut", "range_ends_t7"])
def test_result_does_not_depend_on_record_order(name):
    _, rec, params, _ = CASES[name]
    want, keep, stats, lab, sizes = K.reference(name)
    perm = np.random.default_rng(5).permutation(rec.shape[0])
    lab_p, sizes_p, n_p = N.labels(rec[perm], params[0])
    out_p, keep_p, stats_p = N.filter_from_labels(rec[perm], lab_p, sizes_p, params[1], params[2])
    assert (keep_p == keep[perm]).all() and stats_p == stats and (sizes_p == sizes[perm]).all()
    assert sorted(map(bytes, out_p)) == sorted(map(bytes, want))                      # the kept multiset
    # the labels are the same partition, renamed: records share a label after the permutation iff they did before
    pairs = set(zip(lab[perm].tolist(), lab_p.tolist()))
    assert len(pairs) == stats["clusters"] == n_p
    for old, new in pairs:                                                            # the new label is the first record of the old cluster
        assert new == int(np.nonzero(lab[perm] == old)[0].min())


# ---- the ABI names ------------------------------------------------------------------------------
def test_abi_names_in_header_library_and_python():
    from pointcloud_stitching_amd import lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(L.INCLUDE_DIR, "pcs_hip.h")).read(), flags=re.S)
    L.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r" T (pcs_[a-z0-9_]+)", nm))
    bound = {name for name, _, _ in L.SYMBOLS}
    for name in ABI:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported and name in bound, name
    assert "typedef struct pcs_cluster_params" in header and "struct pcs_cluster_stats" in header
    from pointcloud_stitching_amd.api import PcsContext
    from pointcloud_stitching_amd.types import ClusterParams, ClusterStatsC
    import ctypes as C
    assert C.sizeof(ClusterParams) == 16 and C.sizeof(ClusterStatsC) == 64
    for method in ("cluster_filter", "cluster_filter_device", "cluster_filter_device_counted", "cluster_labels", "cluster_labels_device"):
        assert callable(getattr(PcsContext, method))


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
    assert r.returncode == 0 and "-E <tolerance_mm,min_size[,max_size]>" in r.stdout


MALFORMED = ["", "20", "20,", ",5", "20,,5", "20,5,", "20,5,9,1", "20;5", "20,5x", "x,5", "20,5 ", " 20,5", "20, 5", "0,5", "1001,5", "20,0",
             "20,-1", "-20,5", "20,5,-1", "20,5,4", "20,5,1", "20.5,5", "20,5.0", "20,5,9.5", "99999999999999999999,5",
             "20,99999999999999999999", "20,5,99999999999999999999", "20,2147483648", "20,5,2147483648"]


@pytest.mark.parametrize("arg", MALFORMED)
def test_malformed_option_exits_2_before_any_context(central, arg):
    for cmd in ([central, "-i", "synth:64x48", "-N", "2", "-q", "-r", "1", "-E", arg],
                [central, "-c", "127.0.0.1:1", "-q", "-E", arg]):
        r = run(*cmd)
        assert r.returncode == 2, (cmd, r.stderr)
        assert "-E" in r.stderr and "pcs_create" not in r.stderr and "Connection failed" not in r.stderr


def test_option_with_sharding_is_refused_in_one_line(central):
    r = run(central, "-i", "synth:64x48", "-N", "2", "-q", "-G", "2", "-E", "20,5")
    assert r.returncode == 2 and "-G" in r.stderr and "-E" in r.stderr and len(r.stderr.strip().splitlines()) == 1


def test_well_formed_option_gets_past_the_parser(central):
    """A good -E is not what stops the program: with an edge that does not exist it fails at the connection, status 1."""
    for arg in ("1000,2147483647,2147483647", "1,1", "20,5,0", "20,5,5"):
        r = run(central, "-c", "127.0.0.1:1", "-q", "-E", arg)
        assert r.returncode == 1 and "Connection failed" in r.stderr and "-E" not in r.stderr
