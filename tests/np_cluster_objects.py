"""Restatement of DESIGN.md section 3 "Cluster objects" (pcs_cluster_objects*): the clusters of tests/np_clusters.py that pass the size
filter, numbered by ascending label, each with its inclusive box and its integer sums over the member records. Labels and sizes come
from np_clusters.labels (brute force); the grouping is numpy int64. Shares nothing with the library."""
import numpy as np

import np_clusters as N

# pcs_cluster_object, for a table built here or read back from the library
OBJECT_DTYPE = np.dtype({"names": ["label", "size", "lo", "hi", "reserved0", "sum_xyz", "sum_rgb", "reserved1"],
                         "formats": ["<i4", "<i4", ("<i2", 3), ("<i2", 3), "<i4", ("<i8", 3), ("<i8", 3), "<i8"],
                         "offsets": [0, 4, 8, 14, 20, 24, 48, 72], "itemsize": 80})
VALUE_FIELDS = ("size", "lo", "hi", "sum_xyz", "sum_rgb")


def rgb(records):
    """(R, G, B) int64 [n, 3]: R = short3 & 0xFF, G = (short3 >> 8) & 0xFF, B = short4 & 0xFF; the high byte of short 4 is not read."""
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    s3 = rec[:, 3].astype(np.int64) & 0xFFFF
    s4 = rec[:, 4].astype(np.int64) & 0xFFFF
    return np.stack([s3 & 0xFF, (s3 >> 8) & 0xFF, s4 & 0xFF], axis=1)


def objects_from_labels(records, lab, sizes, min_size, max_size=0):
    """(table [n_objects] of OBJECT_DTYPE, the FULL table; object_of int32 [n])."""
    assert 1 <= min_size <= N.INT_MAX and (max_size == 0 or min_size <= max_size <= N.INT_MAX)
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    n = rec.shape[0]
    lab = np.asarray(lab, np.int64).reshape(n)
    sizes = np.asarray(sizes, np.int64).reshape(n)
    passes = sizes >= min_size
    if max_size:
        passes &= sizes <= max_size
    firsts = np.nonzero((lab == np.arange(n)) & passes)[0]                 # ascending label
    table = np.zeros(firsts.shape[0], OBJECT_DTYPE)
    object_of = np.full(n, -1, np.int32)
    xyz = rec[:, :3].astype(np.int64)
    colour = rgb(rec)
    for k, first in enumerate(firsts.tolist()):
        members = lab == first
        object_of[members] = k
        table[k]["label"] = first
        table[k]["size"] = int(members.sum())
        table[k]["lo"] = xyz[members].min(axis=0)
        table[k]["hi"] = xyz[members].max(axis=0)
        table[k]["sum_xyz"] = xyz[members].sum(axis=0)
        table[k]["sum_rgb"] = colour[members].sum(axis=0)
    return table, object_of


def objects_from_labels_grouped(records, lab, sizes, min_size, max_size=0):
    """objects_from_labels (the definition) without its loop over the objects, for clouds of millions of records: the passing records
    sorted by label (stable), one reduceat per word over the runs of equal labels, in int64. The same return, byte for byte
    (tests/test_cluster_scale_cases_cpu.py)."""
    assert 1 <= min_size <= N.INT_MAX and (max_size == 0 or min_size <= max_size <= N.INT_MAX)
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    n = rec.shape[0]
    lab = np.asarray(lab, np.int64).reshape(n)
    sizes = np.asarray(sizes, np.int64).reshape(n)
    passes = sizes >= min_size
    if max_size:
        passes &= sizes <= max_size
    members = np.nonzero(passes)[0]
    members = members[np.argsort(lab[members], kind="stable")]
    by_label = lab[members]
    starts = np.nonzero(np.concatenate([[True], by_label[1:] != by_label[:-1]]))[0] if members.size else np.zeros(0, np.int64)
    table = np.zeros(starts.shape[0], OBJECT_DTYPE)
    object_of = np.full(n, -1, np.int32)
    if starts.size:
        xyz = rec[members, :3].astype(np.int64)
        colour = rgb(rec[members])
        counts = np.diff(np.concatenate([starts, [members.size]]))
        object_of[members] = np.repeat(np.arange(starts.shape[0], dtype=np.int32), counts)
        table["label"] = by_label[starts]                                  # ascending: the runs of a sort by label
        table["size"] = counts
        table["lo"] = np.minimum.reduceat(xyz, starts, axis=0)
        table["hi"] = np.maximum.reduceat(xyz, starts, axis=0)
        table["sum_xyz"] = np.add.reduceat(xyz, starts, axis=0)
        table["sum_rgb"] = np.add.reduceat(colour, starts, axis=0)
    return table, object_of


def cluster_objects(records, tolerance_mm, min_size, max_size=0):
    """(the full table, n_objects, object_of)."""
    lab, sizes, _ = N.labels(records, tolerance_mm)
    table, object_of = objects_from_labels(records, lab, sizes, min_size, max_size)
    return table, table.shape[0], object_of


def multiset(table):
    """The table without what follows a permutation of the records: the sorted tuples of (size, lo, hi, sum_xyz, sum_rgb)."""
    return sorted(tuple(int(v) for f in VALUE_FIELDS for v in np.atleast_1d(row[f]).tolist()) for row in table)
