"""Restatement of DESIGN.md section 3 "Alignment sums", "Solve" and "Loop" in numpy and Python integers: what pcs_align_sums*,
pcs_align_solve and pcs_align_payloads_device are held to. Brute force over all pairs; nothing here knows about cells.

    match_np(source, target, max_dist)         per source record: the matched target coordinates and d^2 (-1: unmatched)
    sums_np(source, target, max_dist)          the eighteen sums as Python integers (struct order), and dist2 as uint32
    solve_np(sums)                             (delta [4, 4] float64 in metres, rms_mm), or None where the definition refuses
    loop_np(source, target, ...)               the whole loop; with a trace of F_k: the replay of every recorded iteration
"""
import math

import numpy as np

from np_restatement import transform_payload_np

UNMATCHED = 0xFFFFFFFF
DEGENERATE = 1e-9           # second singular value / first, at or below which the rotation is not unique


def match_np(source, target, max_dist, chunk=2048):
    """The match of every source record: the target record minimising (d^2, z, y, x) among those with d^2 <= max_dist^2. All pairs,
    `chunk` source records at a time. The minimum d^2 first; then, among the records at that distance, the tuple order — never a
    packed d^2 * 2^48 word: d^2 of arbitrary pairs reaches 3 * 65535^2 > 2^33, and the product would leave int64.
    d^2 = |p|^2 + |q|^2 - 2 p.q with the dot products as one float64 matrix product: every operand, partial sum and result is an
    integer below 2^35, far inside the 2^53 up to which doubles hold every integer, so each operation is exact and the int64 it is
    converted to is the integer d^2.
    Returns (q [n, 3] int64 — zeros where unmatched, d2 [n] int64 — -1 where unmatched)."""
    p = np.asarray(source).reshape(-1, 5)[:, :3].astype(np.int64)
    t = np.asarray(target).reshape(-1, 5)[:, :3].astype(np.int64)
    n = p.shape[0]
    q = np.zeros((n, 3), np.int64)
    d2 = np.full(n, -1, np.int64)
    if n == 0 or t.shape[0] == 0:
        return q, d2
    # every target record's place in the (z, y, x) order, equal records equal keys: 48 bits
    tkey = ((t[:, 2] + 32768) << 32) | ((t[:, 1] + 32768) << 16) | (t[:, 0] + 32768)
    r2 = int(max_dist) * int(max_dist)
    big = np.int64(1) << 62
    tf = t.astype(np.float64)
    tt = (tf * tf).sum(axis=1)
    for a in range(0, n, chunk):
        pf = p[a:a + chunk].astype(np.float64)
        d = ((pf * pf).sum(axis=1)[:, None] + tt[None, :] - 2.0 * (pf @ tf.T)).astype(np.int64)      # [chunk, n_target]
        dmin = d.min(axis=1)
        ok = dmin <= r2
        cand = np.where(d == dmin[:, None], tkey[None, :], big)              # the tuple order among the minima
        j = cand.argmin(axis=1)
        q[a:a + chunk][ok] = t[j[ok]]
        d2[a:a + chunk][ok] = dmin[ok]
    return q, d2


def sums_np(source, target, max_dist):
    """(the eighteen sums as a list of Python integers in struct order, dist2 [n] uint32)."""
    p = np.asarray(source).reshape(-1, 5)[:, :3].astype(np.int64)
    q, d2 = match_np(source, target, max_dist)
    m = d2 >= 0
    pm, qm = p[m].astype(object), q[m].astype(object)        # Python integers: the products and sums cannot overflow
    sp = [int(sum(pm[:, a], 0)) for a in range(3)]
    sq = [int(sum(qm[:, a], 0)) for a in range(3)]
    spq = [int(sum(pm[:, a] * qm[:, b], 0)) for a in range(3) for b in range(3)]
    sd2 = int(sum(d2[m].astype(object), 0))
    dist2 = np.where(m, d2, UNMATCHED).astype(np.uint32)
    return [int(p.shape[0]), int(m.sum())] + sp + sq + spq + [sd2], dist2


def covariance(sums):
    """C[a][b] = n spq[3a+b] - sp[a] sq[b] in Python integers (exact), as a list of lists."""
    s = [int(v) for v in sums]
    n, sp, sq, spq = s[1], s[2:5], s[5:8], s[8:17]
    return [[n * spq[3 * a + b] - sp[a] * sq[b] for b in range(3)] for a in range(3)]


def solve_np(sums):
    """(delta float64 [4, 4] in metres, rms_mm), or None where the definition refuses: matched < 3, or the second singular value of
    C at most 1e-9 of the first."""
    s = [int(v) for v in sums]
    n = s[1]
    if n < 3:
        return None
    C = np.array([[float(v) for v in row] for row in covariance(s)], np.float64)      # exact integers, rounded once
    if not C.any():
        return None
    U, S, Vt = np.linalg.svd(C)
    if S[1] <= DEGENERATE * S[0]:
        return None
    V = Vt.T
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(V @ U.T)))])
    R = V @ D @ U.T
    pbar = np.array([s[2 + a] / n for a in range(3)])
    qbar = np.array([s[5 + a] / n for a in range(3)])
    delta = np.eye(4)
    delta[:3, :3] = R
    delta[:3, 3] = (qbar - R @ pbar) / 1000.0
    return delta, math.sqrt(s[17] / n)


def rotation_angle(delta):
    """The rotation angle of a 4x4's upper-left block, from the trace and the antisymmetric part (good at small angles)."""
    R = np.asarray(delta, np.float64)[:3, :3]
    sx, sy, sz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    return math.atan2(0.5 * math.sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (np.trace(R) - 1.0))


def translation_mm(delta):
    return 1000.0 * float(np.linalg.norm(np.asarray(delta, np.float64)[:3, 3]))


def loop_np(source, target, max_dist, iterations, stride=1, init=None, eps_rot_rad=0.0, eps_trans_mm=0.0):
    """The loop of DESIGN.md section 3 with transform_payload_np as the move. Returns a dict: `out` float32 [4, 4] = (float)T_K,
    `F` (the F_k used, float32 [K, 4, 4]), `S` (the sums of every iteration), `T` (T_0 .. T_K in double), `reason` (0 iterations,
    1 converged, 2 refused), `iterations`."""
    T = np.eye(4) if init is None else np.asarray(init, np.float32).astype(np.float64).reshape(4, 4)
    F_all, S_all, T_all, reason = [], [], [T.copy()], 0
    may_stop = eps_rot_rad > 0 or eps_trans_mm > 0
    for _ in range(iterations):
        F = T.astype(np.float32)
        moved = transform_payload_np(source, F.reshape(-1), stride)
        S, _ = sums_np(moved, target, max_dist)
        F_all.append(F)
        S_all.append(S)
        solved = solve_np(S)
        if solved is None:
            reason = 2
            break
        T = solved[0] @ T
        T_all.append(T.copy())
        if may_stop and rotation_angle(solved[0]) <= eps_rot_rad and translation_mm(solved[0]) <= eps_trans_mm:
            reason = 1
            break
    return {"out": T.astype(np.float32), "F": np.array(F_all, np.float32).reshape(-1, 4, 4), "S": S_all, "T": T_all,
            "reason": reason, "iterations": len(S_all)}
