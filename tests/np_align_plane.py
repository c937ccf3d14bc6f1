"""Restatement of DESIGN.md section 3 "Plane sums", "Plane solve" and "Plane loop" in numpy and Python integers: what
pcs_align_plane_sums*, pcs_align_plane_solve and pcs_align_payloads_plane_device are held to. The match is np_align.match_np's
(brute force over all pairs); nothing here knows about cells, atomics or partial sums.

    normal_words(normals)                      the four shorts of every target record as one unsigned 64-bit little-endian integer
    plane_sums_np(source, target, normals, max_dist)
                                               (the sixty sums as Python integers in struct order, dist2 [n] uint32)
    recombine(sums)                            (AtA [6][6], Atb [6], sb2) as Python integers: hi 2^32 + lo
    solve_plane_np(sums)                       (delta [4, 4] float64 in metres, rms_mm), or None where the definition refuses
    loop_plane_np(source, target, normals, ...)  the whole loop
"""
import math

import numpy as np

import np_align as N
from np_restatement import transform_payload_np

TERMS = 60
DEGENERATE = 1e-9           # smallest eigenvalue of the scaled A^T A / largest, at or below which the pose is not determined
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]         # the upper triangle, row-major: 21 entries
# struct pcs_align_plane_sums as sixty int64 words
CONSIDERED, MATCHED, USED, ATA_LO, ATA_HI, ATB_LO, ATB_HI, SB2_LO, SB2_HI, SD2 = 0, 1, 2, 3, 24, 45, 51, 57, 58, 59


def normal_words(normals):
    """int16 [m, 4] -> Python integers: short 0 the least significant 16 bits, short 3 the most."""
    s = np.asarray(normals).reshape(-1, 4).astype(np.int64) & 0xFFFF
    return [int(a) | int(b) << 16 | int(c) << 32 | int(d) << 48 for a, b, c, d in s.tolist()]


def split(t):
    """A term as the two halves that are summed separately: (t & 0xFFFFFFFF as unsigned, t >> 32 as an arithmetic shift)."""
    return t & 0xFFFFFFFF, t >> 32


def plane_sums_np(source, target, normals, max_dist):
    """The normal of a match is the smallest VALID (short 3 != 0) word among the target records whose coordinates equal the match's;
    none: the pair is matched, not used."""
    p = np.asarray(source).reshape(-1, 5)[:, :3].astype(np.int64)
    t = np.asarray(target).reshape(-1, 5)[:, :3].astype(np.int64)
    words = normal_words(normals)
    assert len(words) == t.shape[0]
    best = {}
    for xyz, w in zip(map(tuple, t.tolist()), words):
        if w >> 48 and (xyz not in best or w < best[xyz]):
            best[xyz] = w
    q, d2 = N.match_np(source, target, max_dist)
    s = [0] * TERMS
    s[CONSIDERED] = int(p.shape[0])
    hit = d2 >= 0
    s[MATCHED] = int(hit.sum())
    s[SD2] = sum(d2[hit].tolist())
    w = [best.get(tuple(qi)) if ok else None for qi, ok in zip(q.tolist(), hit.tolist())]
    use = np.array([v is not None for v in w], bool)
    s[USED] = int(use.sum())
    if s[USED]:
        # per pair everything fits int64 (|c| < 2^31, |b| < 2^28: a product below 2^62); the SUMS are Python integers
        wu = np.array([v for v in w if v is not None], np.uint64)
        n = np.stack([((wu >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int64) for k in range(3)], axis=1)
        pu, qu = p[use], q[use]
        a = np.concatenate([np.cross(pu, n), n], axis=1)
        b = (n * (qu - pu)).sum(axis=1)

        def halves(t):
            return sum((t & 0xFFFFFFFF).tolist()), sum((t >> 32).tolist())          # (>> on int64: arithmetic)
        for k, (i, j) in enumerate(PAIRS):
            s[ATA_LO + k], s[ATA_HI + k] = halves(a[:, i] * a[:, j])
        for i in range(6):
            s[ATB_LO + i], s[ATB_HI + i] = halves(a[:, i] * b)
        s[SB2_LO], s[SB2_HI] = halves(b * b)
    return s, np.where(hit, d2, N.UNMATCHED).astype(np.uint32)


def plane_sums_loop(source, target, normals, max_dist):
    """The same sums by a plain double loop in Python integers, match and all: what plane_sums_np is checked against. Returns
    (the three counts, the exact A^T A upper triangle, A^T b, sum b^2, sum d^2) — totals, not halves."""
    p = np.asarray(source).reshape(-1, 5)[:, :3].astype(np.int64).tolist()
    t = np.asarray(target).reshape(-1, 5)[:, :3].astype(np.int64).tolist()
    nrm = np.asarray(normals).reshape(-1, 4).astype(np.int64).tolist()
    words = normal_words(normals)
    matched = used = sd2 = sb2 = 0
    ata, atb = [0] * 21, [0] * 6
    for pi in p:
        key = None
        for j, qj in enumerate(t):
            d = sum((pi[k] - qj[k]) ** 2 for k in range(3))
            if d <= max_dist * max_dist and (key is None or (d, qj[2], qj[1], qj[0]) < key[:4]):
                key = (d, qj[2], qj[1], qj[0], j)
        if key is None:
            continue
        matched += 1
        sd2 += key[0]
        qi = t[key[4]]
        same = [j for j, qj in enumerate(t) if qj == qi and nrm[j][3] != 0]
        if not same:
            continue
        used += 1
        n = nrm[min(same, key=lambda j: words[j])][:3]
        c = [pi[1] * n[2] - pi[2] * n[1], pi[2] * n[0] - pi[0] * n[2], pi[0] * n[1] - pi[1] * n[0]]
        a = c + n
        b = sum(n[k] * (qi[k] - pi[k]) for k in range(3))
        for k, (i, j) in enumerate(PAIRS):
            ata[k] += a[i] * a[j]
        for i in range(6):
            atb[i] += a[i] * b
        sb2 += b * b
    return (len(p), matched, used), ata, atb, sb2, sd2


def recombine(sums):
    """(A^T A as a full symmetric [6][6], A^T b [6], sum b^2) in Python integers from the sixty words."""
    s = [int(v) for v in sums]
    ata = [[0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(PAIRS):
        ata[i][j] = ata[j][i] = (s[ATA_HI + k] << 32) + s[ATA_LO + k]
    atb = [(s[ATB_HI + i] << 32) + s[ATB_LO + i] for i in range(6)]
    return ata, atb, (s[SB2_HI] << 32) + s[SB2_LO]


def scaled(sums):
    """(the A^T A scaled to a unit diagonal, the scaled right-hand side, sqrt of the diagonal) in float64, or None with a zero
    diagonal entry. The integers are exact; each is rounded to double once."""
    ata, atb, _ = recombine(sums)
    M = np.array([[float(v) for v in row] for row in ata], np.float64)
    r = np.array([float(v) for v in atb], np.float64)
    d = np.diag(M).copy()
    if (d <= 0).any():
        return None
    w = np.sqrt(d)
    return M / np.outer(w, w), r / w, w


def condition(sums):
    """Smallest over largest eigenvalue of the scaled A^T A (0 with a zero diagonal entry)."""
    sc = scaled(sums)
    if sc is None:
        return 0.0
    lam = np.linalg.eigvalsh(sc[0])
    return float(lam[0] / lam[-1])


def exp_so3(w):
    """Rodrigues: exp([w]x), with the series below 1e-4 rad."""
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-4:
        A, B = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th)
    return np.eye(3) + A * K + B * (K @ K)


def solve_plane_np(sums):
    """(delta float64 [4, 4] in metres, rms_mm), or None where the definition refuses: used < 6, a zero diagonal entry, or the
    scaled matrix's smallest eigenvalue at most 1e-9 of its largest. x = (omega, t) from numpy.linalg.solve."""
    s = [int(v) for v in sums]
    if s[USED] < 6:
        return None
    sc = scaled(s)
    if sc is None or condition(s) <= DEGENERATE:
        return None
    Ms, rs, w = sc
    x = np.linalg.solve(Ms, rs) / w
    delta = np.eye(4)
    delta[:3, :3] = exp_so3(x[:3])
    delta[:3, 3] = x[3:] / 1000.0
    return delta, math.sqrt(recombine(s)[2] / s[USED]) / 16384.0


def loop_plane_np(source, target, normals, max_dist, iterations, stride=1, init=None, eps_rot_rad=0.0, eps_trans_mm=0.0):
    """np_align.loop_np with the plane sums and the plane solve; `normals` are the target's (int16 [m, 4])."""
    T = np.eye(4) if init is None else np.asarray(init, np.float32).astype(np.float64).reshape(4, 4)
    F_all, S_all, T_all, reason = [], [], [T.copy()], 0
    may_stop = eps_rot_rad > 0 or eps_trans_mm > 0
    for _ in range(iterations):
        F = T.astype(np.float32)
        moved = transform_payload_np(source, F.reshape(-1), stride)
        S, _ = plane_sums_np(moved, target, normals, max_dist)
        F_all.append(F)
        S_all.append(S)
        solved = solve_plane_np(S)
        if solved is None:
            reason = 2
            break
        T = solved[0] @ T
        T_all.append(T.copy())
        if may_stop and N.rotation_angle(solved[0]) <= eps_rot_rad and N.translation_mm(solved[0]) <= eps_trans_mm:
            reason = 1
            break
    return {"out": T.astype(np.float32), "F": np.array(F_all, np.float32).reshape(-1, 4, 4), "S": S_all, "T": T_all,
            "reason": reason, "iterations": len(S_all)}
