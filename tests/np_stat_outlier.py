"""Statistical outlier removal (include/pcs_hip.h) restated as brute force: every pair, in int64, in chunks of
1024 rows; math.isqrt; Python integers for S1, S2, W, sigma_q and T. Nothing cleverer — this is what the kernels, the C ABI and the
CLI are held to, byte for byte and word for word."""
import math

import numpy as np

CHUNK = 1024
SPARSE = -1          # D of a sparse record in values()
STATS_FIELDS = ("considered", "dense", "s1", "s2_lo", "s2_hi", "threshold", "kept", "reserved")


def check_params(mean_k, std_mul_milli, max_dist_mm):
    assert 1 <= mean_k <= 64 and 0 <= std_mul_milli <= 10000 and 1 <= max_dist_mm <= 1000


def values(records, mean_k, max_dist_mm):
    """records: (n, 5) int16. D_i as a list of Python integers: the sum of isqrt(65536 d2) over the mean_k smallest d2 <= max_dist_mm^2
    among the records j != i (by index), SPARSE where there are fewer than mean_k."""
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    p = rec[:, :3].astype(np.int64)
    n = p.shape[0]
    r2 = int(max_dist_mm) ** 2
    beyond = np.int64(2 ** 62)
    out = []
    for a in range(0, n, CHUNK):
        d = p[a:a + CHUNK, None] - p[None]
        d2 = (d * d).sum(axis=2)
        rows = np.arange(d2.shape[0])
        d2[rows, a + rows] = beyond                          # j != i is by index
        d2[d2 > r2] = beyond
        d2.sort(axis=1)
        for row in d2:
            nearest = row[:mean_k]
            if nearest.shape[0] < mean_k or nearest[-1] == beyond:
                out.append(SPARSE)
            else:
                out.append(sum(math.isqrt(65536 * int(v)) for v in nearest))
    return out


def threshold(dvalues, std_mul_milli):
    """(M, S1, S2, T) of the non-sparse values, Python integers throughout."""
    dense = [d for d in dvalues if d != SPARSE]
    M, S1, S2 = len(dense), sum(dense), sum(d * d for d in dense)
    if M == 0:
        return 0, 0, 0, 0
    sigma_q = 0
    if M >= 2:
        W = M * S2 - S1 * S1
        assert W >= 0
        sigma_q = math.isqrt((W << 16) // (M * (M - 1)))
    T = (256000 * S1 + std_mul_milli * M * sigma_q) // (256000 * M)
    return M, S1, S2, T


def stat_outlier(records, mean_k, std_mul_milli, max_dist_mm):
    """(the kept records, input order, all five shorts unchanged; the keep mask; the statistics block as a dict)."""
    check_params(mean_k, std_mul_milli, max_dist_mm)
    rec = np.asarray(records, np.int16).reshape(-1, 5)
    D = values(rec, mean_k, max_dist_mm)
    M, S1, _, T = threshold(D, std_mul_milli)
    keep = np.array([d != SPARSE and d <= T for d in D], bool).reshape(-1)
    squares = [d * d for d in D if d != SPARSE]
    stats = {"considered": rec.shape[0], "dense": M, "s1": S1, "s2_lo": sum(t & 0xFFFFFFFF for t in squares),
             "s2_hi": sum(t >> 32 for t in squares), "threshold": T, "kept": int(keep.sum()), "reserved": 0}
    return rec[keep].copy(), keep, stats
