"""Object boxes restated (DESIGN.md section 3 "Object boxes"): grouping in int64 numpy, the covariance in Python integers, numpy's
eigh for the axes, and the extents from GIVEN axis shorts in plain integers. Independent of the kernels' arithmetic: no Jacobi
here. The comparison rules of the tests live here too, so that the CPU tier, the GPU tier and the CLI test apply the same ones."""
import numpy as np

OBJECT_BOX_DTYPE = np.dtype({"names": ["count", "sum_xyz", "m2", "axis", "rank", "ext_lo", "ext_hi", "reserved"],
                             "formats": ["<i8", ("<i8", 3), ("<i8", 6), ("<i2", (3, 3)), "<i2", ("<i4", 3), ("<i4", 3), "<i4"],
                             "offsets": [0, 8, 32, 80, 98, 100, 112, 124], "itemsize": 128})
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
RANK_EPS = 1e-12
GAP_EPS = 1e-3          # an axis is compared only where both neighbouring eigenvalue gaps exceed this x lambda_max
# Every component of a written axis is within 0.5 + 1e-9 of 16384 x a unit vector's (rint, and the double's own error). With
# s = 16384 u, |s| = 16384 and e the error vector, |e_c| <= h = 0.5 + 1e-9:
#   | |axis|^2 - 2^28 | = | 2 s.e + e.e | <= 2 * 16384 * sqrt(3) h + 3 h^2        = 28 378.6...
#   | axis_a . axis_b | = | s_a.e_b + s_b.e_a + e_a.e_b | <= the same bound (s_a . s_b = 0 up to 1e-9 of 2^28, counted in h)
INVARIANT_BOUND = 2 * 16384 * 3 ** 0.5 * (0.5 + 1e-9) + 3 * (0.5 + 1e-9) ** 2 + 1.0


def members(object_of, n_objects, max_objects):
    """m and, per k < m, the indices of the taking-part records with object_of == k (ascending)."""
    m = min(max(int(n_objects), 0), int(max_objects))
    o = np.asarray(object_of, np.int64)
    return m, [np.flatnonzero(o == k) for k in range(m)]


def sums_np(xyz):
    """count, S1 [3], M2 [6] of int64 [n,3] coordinates, exact in int64 (|product| <= 2^30, n < 2^28)."""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    s1 = p.sum(axis=0)
    m2 = np.array([(p[:, a] * p[:, b]).sum() for a, b in PAIRS], np.int64)
    return p.shape[0], s1, m2


def covariance_int(count, s1, m2):
    """C = count M2 - S1 S1^T as a 3 x 3 of Python integers."""
    c = [[0] * 3 for _ in range(3)]
    for w, (a, b) in enumerate(PAIRS):
        c[a][b] = c[b][a] = int(count) * int(m2[w]) - int(s1[a]) * int(s1[b])
    return c


def sign_rule(v):
    """The component of largest magnitude positive, ties preferring z, then y, then x."""
    a = np.abs(v)
    lead = v[2] if a[2] >= a[0] and a[2] >= a[1] else v[1] if a[1] >= a[0] else v[0]
    return -v if lead < 0 else v


def axes_np(count, s1, m2):
    """-> (unit axes [3,3] float64 by descending eigenvalue with the sign rule and a right-handed third, eigenvalues descending,
    rank, sure [3]: whether axis a's eigenvalue is separated from its neighbours by more than GAP_EPS x lambda_max)."""
    c = np.array(covariance_int(count, s1, m2), dtype=object)
    scale = max(1, max(abs(int(v)) for v in c.reshape(-1)))
    w, v = np.linalg.eigh((c / scale).astype(np.float64))           # ascending
    w, v = w[::-1] * float(scale), v[:, ::-1]
    lmax = float(w[0])
    rank = 0 if not lmax > 0 else int((w > RANK_EPS * lmax).sum())
    if rank == 0:
        return np.eye(3), w, 0, np.zeros(3, bool)
    v0, v1 = sign_rule(v[:, 0]), sign_rule(v[:, 1])
    axes = np.stack([v0, v1, np.cross(v0, v1)])
    gap = np.array([w[0] - w[1], min(w[0] - w[1], w[1] - w[2]), w[1] - w[2]])
    sure = gap > GAP_EPS * lmax
    sure[2] = sure[0] and sure[1] and sure[2]                       # the third is the cross product of the other two
    return axes, w, rank, sure


def extents_int(xyz, axis):
    """ext_lo [3], ext_hi [3] of the members under the given axis shorts, in Python-exact int64."""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros(3, np.int32), np.zeros(3, np.int32)
    d = p @ np.asarray(axis, np.int64).T                            # [n, 3]: column a = axis[a] . p
    assert np.abs(d).max() < 2 ** 31
    return d.min(axis=0).astype(np.int32), d.max(axis=0).astype(np.int32)


def boxes_np(payload, object_of, n_objects, max_objects, axis_shorts=None):
    """The restatement -> (entries as OBJECT_BOX_DTYPE [m], sure [m,3]). The entries' axis is rint(16384 e) of eigh's vectors and
    the extents are computed from it, unless axis_shorts ([m,3,3], the implementation's own) is given: then the extents are those
    shorts' (the definition makes them a function of the written shorts)."""
    rec = np.asarray(payload, np.int16).reshape(-1, 5)
    m, idx = members(object_of, n_objects, max_objects)
    out = np.zeros(m, OBJECT_BOX_DTYPE)
    sure = np.zeros((m, 3), bool)
    for k in range(m):
        xyz = rec[idx[k], :3].astype(np.int64)
        count, s1, m2 = sums_np(xyz)
        out[k]["count"], out[k]["sum_xyz"], out[k]["m2"] = count, s1, m2
        axes, _, rank, sure[k] = axes_np(count, s1, m2)
        out[k]["rank"] = rank
        out[k]["axis"] = np.rint(16384.0 * axes).astype(np.int16)
        lo, hi = extents_int(xyz, out[k]["axis"] if axis_shorts is None else axis_shorts[k])
        out[k]["ext_lo"], out[k]["ext_hi"] = lo, hi
    return out, sure


def check_invariants(got, where=""):
    """What holds for every entry, degenerate or not: near-orthonormal rows, a positive determinant, the sign rule of axes 0 and 1
    where the two largest components differ by more than 2, reserved 0."""
    for k, e in enumerate(got):
        a = e["axis"].astype(np.int64)
        for i in range(3):
            assert abs(int(a[i] @ a[i]) - (1 << 28)) <= INVARIANT_BOUND, (where, k, i, a.tolist())
            for j in range(i + 1, 3):
                assert abs(int(a[i] @ a[j])) <= INVARIANT_BOUND, (where, k, i, j, a.tolist())
        assert round(float(np.linalg.det(a.astype(np.float64)))) > 0, (where, k, a.tolist())
        for i in (0, 1):
            mag = np.abs(a[i])
            order = sorted(range(3), key=lambda c: (mag[c], c))      # ascending; ties: the higher component last (z, then y, then x)
            if mag[order[2]] - mag[order[1]] > 2:
                assert a[i][order[2]] > 0, (where, k, i, a.tolist())
        assert int(e["reserved"]) == 0 and 0 <= int(e["rank"]) <= 3, (where, k)


def check_members(got, payload, object_of, n_objects, max_objects, where=""):
    """Every member's projection lies in [ext_lo, ext_hi] and both ends are attained — that is: the extents are those of the
    entry's own shorts."""
    rec = np.asarray(payload, np.int16).reshape(-1, 5)
    m, idx = members(object_of, n_objects, max_objects)
    assert got.shape[0] == m, (where, got.shape[0], m)
    for k in range(m):
        lo, hi = extents_int(rec[idx[k], :3], got[k]["axis"])
        assert got[k]["ext_lo"].tolist() == lo.tolist() and got[k]["ext_hi"].tolist() == hi.tolist(), (where, k)


def compare(got, payload, object_of, n_objects, max_objects, where="", axes=True, max_unsure=0.01):
    """got (OBJECT_BOX_DTYPE [m]) against the restatement: sums and rank equal, extents equal to the restatement's fed got's own
    shorts, the invariants, and (axes=True) every sure axis within 1 short of rint(16384 e) after aligning signs, with fewer than
    max_unsure of the case's objects left out of that one comparison. -> the number of axes compared."""
    got = np.asarray(got).view(OBJECT_BOX_DTYPE).reshape(-1)
    want, sure = boxes_np(payload, object_of, n_objects, max_objects, axis_shorts=None if got.shape[0] == 0 else got["axis"])
    assert got.shape[0] == want.shape[0], (where, got.shape[0], want.shape[0])
    for name in ("count", "sum_xyz", "m2", "rank", "ext_lo", "ext_hi", "reserved"):
        assert got[name].tobytes() == want[name].tobytes(), (where, name, got[name].tolist(), want[name].tolist())
    check_invariants(got, where)
    compared = 0
    if axes and got.shape[0]:
        left_out = 0
        for k in range(got.shape[0]):
            if int(want[k]["rank"]) == 0:
                assert got[k]["axis"].tolist() == (16384 * np.eye(3, dtype=np.int64)).tolist(), (where, k)
                continue
            if not sure[k].all():
                left_out += 1
            for a in range(3):
                if not sure[k][a]:
                    continue
                g, w = got[k]["axis"][a].astype(np.int64), want[k]["axis"][a].astype(np.int64)
                if int(g @ w) < 0:
                    w = -w                                          # (a sign the rule decides on a near tie of components)
                assert np.abs(g - w).max() <= 1, (where, k, a, g.tolist(), w.tolist())
                compared += 1
        assert left_out <= max_unsure * got.shape[0], (where, left_out, got.shape[0])
    return compared
