// pcs_normals_math.h — what one lane of the normal estimator does once its ten integer sums are in (DESIGN.md section 3 "Surface
// normals"): the exact covariance in 128-bit integers, one conversion to double, a cyclic Jacobi eigen-decomposition of the 3 x 3,
// the validity rules, the sign rule and the rounding to shorts. Plain C++ with every array index a compile-time constant (nothing
// here may become a runtime-indexed private array on the device); host and device compile the same text, so a CPU program can run
// the arithmetic of pcs_normals_estimate_kernel record by record. Included by pcs_kernels_normals.hip, never compiled alone there.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PCS_HD __host__ __device__ __forceinline__
#else
#define PCS_HD inline
#endif

namespace pcs {

// pcs_normal_params as the kernels take it (checked by the host layer: radius 1..1000, min_neighbors 3..32767, flatness 0..1000)
struct NormalRule {
    int32_t radius, min_neighbors, flatness, use_viewpoint;
    int32_t vx, vy, vz;
};

constexpr int    kNormalSweeps   = 12;        // the bound of the Jacobi loop: a 3 x 3 is down to rounding after 4 to 6 sweeps
constexpr double kNormalOffDiag  = 1e-18;     // ... which ends when sum |off-diagonal| <= this x sum |diagonal|
constexpr double kNormalRank     = 1e-12;     // lambda1 <= this x lambda2: collinear or coincident neighbours

// One Jacobi rotation that zeroes A[P][Q] (A symmetric, both halves kept), accumulated into the columns of V.
template <int P, int Q>
PCS_HD void normal_rotate(double (&A)[3][3], double (&V)[3][3])
{
    constexpr int R = 3 - P - Q;
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    // (a tiny apq against the diagonal's gap: theta^2 may be +inf, t is then 0 and the rotation the identity)
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double vp = V[i][P], vq = V[i][Q];
        V[i][P] = c * vp - s * vq;
        V[i][Q] = s * vp + c * vq;
    }
}

// The four output shorts of a record as one little-endian word (nx | ny << 16 | nz << 32 | count << 48), 0 when it is invalid.
// m = the neighbourhood's size, s1 = sum of delta, s2 = sum of delta delta^T as xx, xy, xz, yy, yz, zz, (qx, qy, qz) the record.
PCS_HD unsigned long long normal_word(long long m, const long long (&s1)[3], const long long (&s2)[6], const NormalRule& rule, int qx,
                                      int qy, int qz)
{
    if (m < rule.min_neighbors) return 0ull;
    // C = m S2 - S1 S1^T, exact: m S2 passes 2^64 for large neighbourhoods
    const __int128 mm = m;
    double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    A[0][0] = (double)(mm * s2[0] - (__int128)s1[0] * s1[0]);
    A[0][1] = A[1][0] = (double)(mm * s2[1] - (__int128)s1[0] * s1[1]);
    A[0][2] = A[2][0] = (double)(mm * s2[2] - (__int128)s1[0] * s1[2]);
    A[1][1] = (double)(mm * s2[3] - (__int128)s1[1] * s1[1]);
    A[1][2] = A[2][1] = (double)(mm * s2[4] - (__int128)s1[1] * s1[2]);
    A[2][2] = (double)(mm * s2[5] - (__int128)s1[2] * s1[2]);
#pragma unroll 1
    for (int sweep = 0; sweep < kNormalSweeps; sweep++) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off <= kNormalOffDiag * (fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]))) break;
        normal_rotate<0, 1>(A, V);
        normal_rotate<0, 2>(A, V);
        normal_rotate<1, 2>(A, V);
    }
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
    const double l0 = fmin(d0, fmin(d1, d2)), l2 = fmax(d0, fmax(d1, d2));
    const double l1 = fmax(fmin(d0, d1), fmin(fmax(d0, d1), d2));
    if (!(l1 > kNormalRank * l2)) return 0ull;
    if (rule.flatness > 0 && (double)rule.flatness * l0 > l1) return 0ull;
    const bool c0 = d0 <= d1 && d0 <= d2, c1 = !c0 && d1 <= d2;         // the column of lambda0
    double vx = c0 ? V[0][0] : c1 ? V[0][1] : V[0][2];
    double vy = c0 ? V[1][0] : c1 ? V[1][1] : V[1][2];
    double vz = c0 ? V[2][0] : c1 ? V[2][1] : V[2][2];
    // the sign: towards the viewpoint; without one (or at a right angle to it) the component of largest magnitude is positive,
    // ties preferring z, then y, then x
    const double ax = fabs(vx), ay = fabs(vy), az = fabs(vz);
    const double lead = (az >= ax && az >= ay) ? vz : (ay >= ax) ? vy : vx;
    bool flip = lead < 0.0;
    if (rule.use_viewpoint) {
        const double dot = vx * ((double)rule.vx - (double)qx) + vy * ((double)rule.vy - (double)qy) + vz * ((double)rule.vz - (double)qz);
        if (dot != 0.0) flip = dot < 0.0;
    }
    if (flip) { vx = -vx; vy = -vy; vz = -vz; }
    const int nx = (int)rint(16384.0 * vx), ny = (int)rint(16384.0 * vy), nz = (int)rint(16384.0 * vz);
    const long long cnt = m < 32767 ? m : 32767;
    return (unsigned long long)(uint16_t)(int16_t)nx | (unsigned long long)(uint16_t)(int16_t)ny << 16 |
           (unsigned long long)(uint16_t)(int16_t)nz << 32 | (unsigned long long)cnt << 48;
}

}  // namespace pcs
