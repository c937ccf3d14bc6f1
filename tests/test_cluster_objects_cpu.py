"""Cluster objects without a GPU: the restatement (tests/np_cluster_objects.py) against an independent plain-Python accumulation
(the cells and breadth-first search of tests/test_clusters_cpu.py, dictionaries of Python integers) over every shared case; analytic
checks on the lines of `sizes_cloud`; invariance of the table's multiset under a permutation of the records; the -L flag surface of
pcs-multicamera-optimized (help text, every refusal with status 2 before a context is created); the ABI names in the header, the
library's export table and lib.py; and pcs_cluster_object's size and field offsets against a host program compiled from the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as K
import np_cluster_objects as NO
import np_clusters as N
from test_clusters_cpu import cells_clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
CENTRAL = os.path.join(ROOT, "pointcloud_stitching_amd", "bin", "pcs-multicamera-optimized")
CASES = {c[0]: c for c in K.cases()}
ABI = ("pcs_cluster_objects_device", "pcs_cluster_objects_device_counted", "pcs_cluster_objects")


def plain_objects(records, tolerance_mm, min_size, max_size):
    """The definition in dictionaries of Python integers: (list of dicts by ascending label, object_of list)."""
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    label, size = cells_clusters(rec, tolerance_mm)
    acc = {}
    for i, row in enumerate(rec.tolist()):
        if size[i] < min_size or (max_size and size[i] > max_size):
            continue
        x, y, z, s3, s4 = row
        s3, s4 = s3 % 65536, s4 % 65536
        colour = (s3 % 256, s3 // 256, s4 % 256)                 # the high byte of short 4 is not read
        o = acc.setdefault(label[i], {"label": label[i], "size": 0, "lo": [x, y, z], "hi": [x, y, z], "sum_xyz": [0, 0, 0], "sum_rgb": [0, 0, 0]})
        o["size"] += 1
        for a, v in enumerate((x, y, z)):
            o["lo"][a] = min(o["lo"][a], v)
            o["hi"][a] = max(o["hi"][a], v)
            o["sum_xyz"][a] += v
            o["sum_rgb"][a] += colour[a]
    order = sorted(acc)
    rank = {lab: k for k, lab in enumerate(order)}
    return [acc[lab] for lab in order], [rank.get(label[i], -1) for i in range(rec.shape[0])]


def as_dicts(table):
    return [{"label": int(o["label"]), "size": int(o["size"]), "lo": o["lo"].tolist(), "hi": o["hi"].tolist(), "sum_xyz": o["sum_xyz"].tolist(),
             "sum_rgb": o["sum_rgb"].tolist()} for o in table]


def restated(name):
    _, rec, params, _ = CASES[name]
    _, _, stats, lab, sizes = K.reference(name)
    table, object_of = NO.objects_from_labels(rec, lab, sizes, params[1], params[2])
    return rec, params, table, object_of, stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_agrees_with_a_plain_python_accumulation(name):
    rec, (tol, lo, hi), table, object_of, stats = restated(name)
    want, want_of = plain_objects(rec, tol, lo, hi)
    assert as_dicts(table) == want and object_of.tolist() == want_of
    assert table.shape[0] == stats["kept_clusters"] and (table["reserved0"] == 0).all() and (table["reserved1"] == 0).all()
    assert (np.diff(table["label"]) > 0).all()                                        # ascending label
    assert int(table["size"].sum()) == stats["kept"] and (object_of >= 0).sum() == stats["kept"]
    assert table.dtype.itemsize == 80


def test_the_cases_span_one_object_to_many_and_the_range_ends():
    for name in ("lattice_joined", "duplicates", "chain_cut"):
        assert restated(name)[2].shape[0] == 1, name
    assert restated("sizes_33_64")[2].shape[0] == 32 and restated("count2049")[2].shape[0] == 218
    for name in ("range_ends_t2", "range_ends_t7"):
        t = restated(name)[2]
        assert t["lo"].min() == -32768 and t["hi"].max() == 32767
    t, _, _ = NO.cluster_objects(CASES["extremes_t1"][1], 1, 1, 0)
    assert t.shape[0] == 6 and t["lo"].min() == -32768 and t["hi"].max() == 32767 and (t["lo"] == t["hi"]).all()
    for name in ("count2049", "sizes_33_64"):                                          # a kernel that reads B as a short fails
        assert ((CASES[name][1][:, 4].astype(np.int64) & 0xFF00) != 0).all()


def test_lines_of_the_sizes_cloud_by_their_arithmetic():
    rec, _ = K.sizes_cloud()
    _, _, _, lab, sizes = K.reference("sizes_33_64")
    table, object_of = NO.objects_from_labels(rec, lab, sizes, 2, 0)
    assert table.shape[0] == 69 and sorted(table["size"].tolist()) == list(range(2, 71))
    for o in table:
        s = int(o["size"])
        assert int(o["hi"][0]) - int(o["lo"][0]) == 2 * (s - 1) and int(o["lo"][0]) == -60
        assert o["lo"][1] == o["hi"][1] == 100 * s - 3500 and o["lo"][2] == o["hi"][2] == -100 * s + 3000
        assert int(o["sum_xyz"][1]) == s * (100 * s - 3500) and int(o["sum_xyz"][2]) == s * (-100 * s + 3000)
        assert int(o["sum_xyz"][0]) == s * (s - 1) - 60 * s
    table, _ = NO.objects_from_labels(rec, lab, sizes, 33, 0)
    assert table.shape[0] == 38


@pytest.mark.parametrize("name", ["count2049", "sizes_33_64", "range_ends_t7"])
def test_multiset_does_not_depend_on_record_order(name):
    rec, params, table, object_of, _ = restated(name)
    perm = np.random.default_rng(6).permutation(rec.shape[0])
    table_p, n_p, object_of_p = NO.cluster_objects(rec[perm], *params)
    assert n_p == table.shape[0] and NO.multiset(table_p) == NO.multiset(table)
    # the same partition into objects, renumbered by the permuted records' first members
    pairs = set(zip(object_of[perm].tolist(), object_of_p.tolist()))
    assert len(pairs) == table.shape[0] + int((object_of < 0).any())
    for k in range(n_p):
        assert int(table_p[k]["label"]) == int(np.nonzero(object_of_p == k)[0].min())


# ---- the ABI -------------------------------------------------------------------------------------
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
    assert "typedef struct pcs_cluster_object {" in header and "typedef struct pcs_cluster_objects_out {" in header
    assert re.search(r"#define\s+PCS_CLUSTER_OBJECTS_MAX\s+65536\b", header)
    from pointcloud_stitching_amd import types as T
    from pointcloud_stitching_amd.api import PcsContext
    assert T.CLUSTER_OBJECTS_MAX == 65536 and T.CLUSTER_OBJECT_LAUNCHES == len(T.CLUSTER_OBJECT_STAGES) == 15
    assert T.CLUSTER_OBJECT_OUT_LAUNCHES == len(T.CLUSTER_OBJECT_OUT_STAGES) == 19
    for method in ("cluster_objects", "cluster_objects_device", "cluster_objects_device_counted"):
        assert callable(getattr(PcsContext, method))


def test_struct_size_and_offsets_against_the_header(tmp_path):
    from pointcloud_stitching_amd import lib as L
    from pointcloud_stitching_amd.types import CLUSTER_OBJECT_DTYPE, ClusterObject, ClusterObjectsOut
    fields = ("label", "size", "lo", "hi", "reserved0", "sum_xyz", "sum_rgb", "reserved1")
    out_fields = ("objects", "max_objects", "reserved", "n_objects", "object_of", "out", "out_shorts", "out_points", "stats")
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pcs_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(pcs_cluster_object), sizeof(pcs_cluster_objects_out));\n'
                   + "".join(f'  printf(" %zu", offsetof(pcs_cluster_object, {f}));\n' for f in fields)
                   + "".join(f'  printf(" %zu", offsetof(pcs_cluster_objects_out, {f}));\n' for f in out_fields)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "offsets")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", L.INCLUDE_DIR, str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == 80 == C.sizeof(ClusterObject) == CLUSTER_OBJECT_DTYPE.itemsize == NO.OBJECT_DTYPE.itemsize
    assert got[1] == C.sizeof(ClusterObjectsOut)
    assert got[2:2 + len(fields)] == [getattr(ClusterObject, f).offset for f in fields] == [0, 4, 8, 14, 20, 24, 48, 72]
    assert got[2:2 + len(fields)] == [CLUSTER_OBJECT_DTYPE.fields[f][1] for f in fields] == [NO.OBJECT_DTYPE.fields[f][1] for f in fields]
    assert got[2 + len(fields):] == [getattr(ClusterObjectsOut, f).offset for f in out_fields]
    assert C.alignment(ClusterObject) == 8


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
    assert r.returncode == 0 and "-L <file>[,<max_objects>]" in r.stdout


REFUSED = ["", ",5", "file,", "file,0", "file,-1", "file,65537", "file,5x", "file,5 ", "file, 5", "file,x", "file,5.0", "file,5,",
           "file,99999999999999999999", "file,+5"]


@pytest.mark.parametrize("arg", REFUSED)
def test_malformed_option_exits_2_before_any_context(central, arg):
    for cmd in ([central, "-i", "synth:64x48", "-N", "2", "-q", "-r", "1", "-E", "20,5", "-L", arg],
                [central, "-c", "127.0.0.1:1", "-q", "-E", "20,5", "-L", arg]):
        r = run(*cmd)
        assert r.returncode == 2, (cmd, r.stderr)
        assert "-L" in r.stderr and "pcs_create" not in r.stderr and "Connection failed" not in r.stderr


def test_option_without_the_cluster_filter_is_refused(central, tmp_path):
    path = str(tmp_path / "objects.txt")
    for cmd in ([central, "-i", "synth:64x48", "-N", "2", "-q", "-r", "1", "-L", path],
                [central, "-c", "127.0.0.1:1", "-q", "-O", "20,2", "-L", path]):
        r = run(*cmd)
        assert r.returncode == 2 and "-L" in r.stderr and "-E" in r.stderr and "Connection failed" not in r.stderr, r.stderr
    assert not os.path.exists(path)


def test_option_with_sharding_is_refused_in_one_line(central, tmp_path):
    path = str(tmp_path / "objects.txt")
    r = run(central, "-i", "synth:64x48", "-N", "2", "-q", "-G", "2", "-E", "20,5", "-L", path)
    assert r.returncode == 2 and "-G" in r.stderr and "-L" in r.stderr and "the node library has no object table" in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1 and not os.path.exists(path)


def test_well_formed_option_gets_past_the_parser(central, tmp_path):
    """A good -L is not what stops the program: with an edge that does not exist it fails at the connection, status 1."""
    for arg in (str(tmp_path / "objects.txt"), str(tmp_path / "objects.txt") + ",1", str(tmp_path / "o.txt") + ",65536", "-", "-,7"):
        r = run(central, "-c", "127.0.0.1:1", "-q", "-E", "20,5", "-L", arg)
        assert r.returncode == 1 and "Connection failed" in r.stderr and "-L" not in r.stderr, r.stderr
