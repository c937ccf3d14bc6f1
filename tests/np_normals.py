"""Restatement of DESIGN.md section 3 "Surface normals" in numpy and Python integers: what pcs_estimate_normals* is held to. Brute
force over all pairs; nothing here knows about cells, and the eigen-decomposition is numpy's eigh, not a Jacobi.

    neighbour_sums_np(payload, radius)      per record: m [n], S1 [n, 3], S2 [n, 6] (xx, xy, xz, yy, yz, zz) as int64, exact
    covariance_np(m, S1, S2)                C = m S2 - S1 S1^T as Python integers, object array [n, 3, 3]
    normals_np(payload, radius, min_neighbors, flatness, viewpoint=None)
                                            a Normals: validity, the signed unit normal in double, the shorts, the eigenvalues and
                                            `unsure` — the records a comparison leaves out (below)
    compare(got, ref)                       the assertion of the GPU tests: validity equal, shorts within 1 after aligning signs

What a comparison leaves out, and why the rest is held to one unit of a short: a double Jacobi and eigh on the same C agree to about
1e-16 lambda2 in the eigenvalues and to about 1e-16 lambda2 / (lambda1 - lambda0) in the eigenvector of lambda0. A record is `unsure`
when (lambda1 - lambda0) < 1e-3 lambda2 (the vector is then only known to 1e-13, and below that gap not at all), or when one of the
two eigenvalue thresholds is met within a relative 1e-9 (|a - b| <= 1e-9 max(|a|, |b|) for the two sides a, b of the comparison).
Everywhere else the vectors differ by about 1e-13, so 16384 v differs by 2e-9: only a rounding boundary can move a short, by one.
Two cases are exact and never unsure: m < min_neighbors (an integer comparison), and a C of rank 0 or 1 in integers (every 2 x 2
minor vanishes: the neighbours coincide or lie on one line). There lambda1 is 0, either solver returns it as a few 1e-16 lambda2, four
orders below the 1e-12 lambda2 it is compared with: such a record is invalid, with certainty."""
import dataclasses

import numpy as np

RANK = 1e-12            # lambda1 <= RANK lambda2: collinear or coincident neighbours
GAP = 1e-3              # (lambda1 - lambda0) < GAP lambda2: left out of a comparison
NEAR = 1e-9             # a threshold met within this relative distance: left out of a comparison
UNSURE_CAP = 0.01       # of a case's records


@dataclasses.dataclass
class Normals:
    valid: np.ndarray       # bool [n]
    v: np.ndarray           # float64 [n, 3]: the signed unit normal (zeros where invalid)
    shorts: np.ndarray      # int16 [n, 4]: what the call writes, from eigh
    m: np.ndarray           # int64 [n]
    lam: np.ndarray         # float64 [n, 3] ascending
    unsure: np.ndarray      # bool [n]


def neighbour_sums_np(payload, radius, chunk=512):
    """m, S1, S2 of every record. d^2 = |p|^2 + |q|^2 - 2 p.q as one float64 matrix product (every operand and partial sum an
    integer below 2^35: exact, as in np_align.match_np); the sums as int64 matrix products of the 0/1 mask with the coordinates and
    their products, then moved to the record: sum delta = sum x - m q, sum delta delta^T = sum x x^T - q (sum x)^T - (sum x) q^T +
    m q q^T. Every term stays below 2^31 records x 2^30: the caller's clouds are far inside int64."""
    t = np.asarray(payload).reshape(-1, 5)[:, :3].astype(np.int64)
    n = t.shape[0]
    m, S1, S2 = np.zeros(n, np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 6), np.int64)
    if n == 0:
        return m, S1, S2
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    xx = np.stack([t[:, a] * t[:, b] for a, b in pairs], axis=1)
    tf = t.astype(np.float64)
    tt = (tf * tf).sum(axis=1)
    r2 = int(radius) * int(radius)
    for a0 in range(0, n, chunk):
        q = t[a0:a0 + chunk]
        qf = tf[a0:a0 + chunk]
        d = ((qf * qf).sum(axis=1)[:, None] + tt[None, :] - 2.0 * (qf @ tf.T)).astype(np.int64)
        mask = (d <= r2).astype(np.int64)
        mm = mask.sum(axis=1)
        sx = mask @ t
        sxx = mask @ xx
        m[a0:a0 + chunk] = mm
        S1[a0:a0 + chunk] = sx - mm[:, None] * q
        for k, (a, b) in enumerate(pairs):
            S2[a0:a0 + chunk, k] = sxx[:, k] - q[:, a] * sx[:, b] - sx[:, a] * q[:, b] + mm * q[:, a] * q[:, b]
    return m, S1, S2


def covariance_np(m, S1, S2):
    """C = m S2 - S1 S1^T in Python integers (it passes 2^64 for large neighbourhoods), object array [n, 3, 3]."""
    n = m.shape[0]
    mo, s1, s2 = m.astype(object), S1.astype(object), S2.astype(object)
    C = np.empty((n, 3, 3), object)
    k = 0
    for a in range(3):
        for b in range(a, 3):
            C[:, a, b] = C[:, b, a] = mo * s2[:, k] - s1[:, a] * s1[:, b]
            k += 1
    return C


def line_or_point(c):
    """C (3 x 3 Python integers, symmetric) has rank 0 or 1: every 2 x 2 minor is zero."""
    return all(c[a][b] * c[d][e] == c[a][e] * c[d][b] for a in range(3) for d in range(a + 1, 3) for b in range(3) for e in range(b + 1, 3))


def canonical_flip(v):
    """Where the component of largest magnitude is negative, ties preferring z, then y, then x: bool [n]."""
    a = np.abs(v)
    lead = np.where((a[:, 2] >= a[:, 0]) & (a[:, 2] >= a[:, 1]), v[:, 2], np.where(a[:, 1] >= a[:, 0], v[:, 1], v[:, 0]))
    return lead < 0


def normals_np(payload, radius, min_neighbors, flatness, viewpoint=None):
    q = np.asarray(payload).reshape(-1, 5)[:, :3].astype(np.int64)
    n = q.shape[0]
    m, S1, S2 = neighbour_sums_np(payload, radius)
    Cint = covariance_np(m, S1, S2)
    zero = np.array([line_or_point(Cint[i]) for i in range(n)], bool)
    C = np.array([[float(v) for v in Cint[i].reshape(-1)] for i in range(n)], np.float64).reshape(n, 3, 3)      # rounded once
    lam, vec = (np.linalg.eigh(C) if n else (np.zeros((0, 3)), np.zeros((0, 3, 3))))
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    enough = m >= min_neighbors
    valid = enough & ~zero & (l1 > RANK * l2)
    if flatness > 0:
        valid &= ~(flatness * l0 > l1)

    def near(a, b):
        return np.abs(a - b) <= NEAR * np.maximum(np.abs(a), np.abs(b))
    unsure = (l1 - l0) < GAP * l2
    unsure |= near(l1, RANK * l2)
    if flatness > 0:
        unsure |= near(flatness * l0, l1)
    unsure &= enough & ~zero
    v = vec[:, :, 0].copy()
    flip = canonical_flip(v)
    if viewpoint is not None:
        dot = (v * (np.asarray(viewpoint, np.float64)[None, :] - q)).sum(axis=1)
        flip = np.where(dot != 0, dot < 0, flip)
    v[flip] = -v[flip]
    v[~valid] = 0.0
    shorts = np.zeros((n, 4), np.int16)
    shorts[:, :3] = np.rint(16384.0 * v).astype(np.int16)
    shorts[:, 3] = np.where(valid, np.minimum(m, 32767), 0).astype(np.int16)
    return Normals(valid, v, shorts, m, lam, unsure)


def compare(got, ref, what=""):
    """got: int16 [n, 4] from the library; ref: a Normals. Validity equal and, after aligning signs, every component within 1 —
    over the records that are not `unsure`, which are under UNSURE_CAP of the case. The neighbour count is an integer: it is compared
    on every valid record, unsure or not. Returns the number of records compared."""
    got = np.asarray(got).reshape(-1, 4)
    n = got.shape[0]
    assert n == ref.valid.shape[0], what
    assert ref.unsure.sum() <= UNSURE_CAP * n, (what, int(ref.unsure.sum()), n)
    sure = ~ref.unsure
    got_valid = got[:, 3] != 0
    assert (got[~got_valid] == 0).all(), (what, "an invalid record is not four zero shorts")
    assert (got_valid[sure] == ref.valid[sure]).all(), (what, np.nonzero(sure & (got_valid != ref.valid))[0][:10])
    both = got_valid & ref.valid
    assert (got[both, 3] == ref.shorts[both, 3]).all(), (what, "neighbour counts differ")
    pick = both & sure
    g = got[pick, :3].astype(np.int64)
    want = ref.shorts[pick, :3].astype(np.int64)
    sign = np.where((g * want).sum(axis=1) < 0, -1, 1)[:, None]
    worst = int(np.abs(g - sign * want).max()) if g.size else 0
    assert worst <= 1, (what, worst)
    return int(pick.sum())
