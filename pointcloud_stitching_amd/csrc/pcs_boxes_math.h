// pcs_boxes_math.h — what one lane of the object boxes' axes launch does once an object's ten integer sums are in (DESIGN.md section
// 3 "Object boxes"): the exact covariance in 128-bit integers, one conversion to double, the normals' cyclic Jacobi (normal_rotate,
// its stop rule and its sweep bound, from pcs_normals_math.h as they stand), the eigenvalues ordered descending, the sign rule, the
// third axis as a cross product, the rounding to shorts and the rank; and the projection that the extents launch takes per record.
// Plain C++ with every array index a compile-time constant (nothing here may become a runtime-indexed private array on the device);
// host and device compile the same text: tools/boxes_host.cpp runs it behind a plain loop. Included by pcs_kernels_boxes.hip, never
// compiled alone there.
#pragma once

#include "pcs_normals_math.h"

namespace pcs {

// the nine axis shorts of an entry, axis a's component c in a[3 * a + c], and its rank
struct BoxAxes {
    int16_t a00, a01, a02, a10, a11, a12, a20, a21, a22;
    int16_t rank;
};

// the sign of an axis: its component of largest magnitude is positive, ties preferring z, then y, then x (the normals' rule)
PCS_HD void box_sign(double& vx, double& vy, double& vz)
{
    const double ax = fabs(vx), ay = fabs(vy), az = fabs(vz);
    const double lead = (az >= ax && az >= ay) ? vz : (ay >= ax) ? vy : vx;
    if (lead < 0.0) { vx = -vx; vy = -vy; vz = -vz; }
}

// The entry's axes from the eigenvectors: columns I0 and I1 of V are the directions of the largest and the second spread.
template <int I0, int I1>
PCS_HD BoxAxes box_round(const double (&V)[3][3], int rank)
{
    double ux = V[0][I0], uy = V[1][I0], uz = V[2][I0];
    double vx = V[0][I1], vy = V[1][I1], vz = V[2][I1];
    box_sign(ux, uy, uz);
    box_sign(vx, vy, vz);
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;      // right-handed by construction
    BoxAxes out;
    out.a00 = (int16_t)(int)rint(16384.0 * ux); out.a01 = (int16_t)(int)rint(16384.0 * uy); out.a02 = (int16_t)(int)rint(16384.0 * uz);
    out.a10 = (int16_t)(int)rint(16384.0 * vx); out.a11 = (int16_t)(int)rint(16384.0 * vy); out.a12 = (int16_t)(int)rint(16384.0 * vz);
    out.a20 = (int16_t)(int)rint(16384.0 * wx); out.a21 = (int16_t)(int)rint(16384.0 * wy); out.a22 = (int16_t)(int)rint(16384.0 * wz);
    out.rank = (int16_t)rank;
    return out;
}

// count = the object's members, s1 = sum of p, m2 = sum of p p^T as xx, xy, xz, yy, yz, zz. An object without spread (count 0 or 1,
// or every member equal) has C = 0: the loop ends at once, V stays the identity and so do the axes; rank 0.
PCS_HD BoxAxes box_axes(long long count, const long long (&s1)[3], const long long (&m2)[6])
{
    // C = count M2 - S1 S1^T, exact: count M2 passes 2^64 for large objects
    const __int128 mm = count;
    double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    A[0][0] = (double)(mm * m2[0] - (__int128)s1[0] * s1[0]);
    A[0][1] = A[1][0] = (double)(mm * m2[1] - (__int128)s1[0] * s1[1]);
    A[0][2] = A[2][0] = (double)(mm * m2[2] - (__int128)s1[0] * s1[2]);
    A[1][1] = (double)(mm * m2[3] - (__int128)s1[1] * s1[1]);
    A[1][2] = A[2][1] = (double)(mm * m2[4] - (__int128)s1[1] * s1[2]);
    A[2][2] = (double)(mm * m2[5] - (__int128)s1[2] * s1[2]);
#pragma unroll 1
    for (int sweep = 0; sweep < kNormalSweeps; sweep++) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off <= kNormalOffDiag * (fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]))) break;
        normal_rotate<0, 1>(A, V);
        normal_rotate<0, 2>(A, V);
        normal_rotate<1, 2>(A, V);
    }
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
    // descending, a tie to the lower column: i0 the column of the largest, then (p, q), p < q, the two that are left
    const int i0 = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2) ? 1 : 2;
    const int p = i0 == 0 ? 1 : 0, q = i0 == 2 ? 1 : 2;
    const double dp = i0 == 0 ? d1 : d0, dq = i0 == 2 ? d1 : d2;
    const int i1 = dp >= dq ? p : q;
    const double lmax = i0 == 0 ? d0 : i0 == 1 ? d1 : d2;
    int rank = 0;
    if (lmax > 0.0) rank = (int)(d0 > kNormalRank * lmax) + (int)(d1 > kNormalRank * lmax) + (int)(d2 > kNormalRank * lmax);
    // (one call per order of the columns: a column picked by a runtime index would put V into scratch on the device)
    if (i0 == 0) return i1 == 1 ? box_round<0, 1>(V, rank) : box_round<0, 2>(V, rank);
    if (i0 == 1) return i1 == 0 ? box_round<1, 0>(V, rank) : box_round<1, 2>(V, rank);
    return i1 == 0 ? box_round<2, 0>(V, rank) : box_round<2, 1>(V, rank);
}

// axis . p in int32, exact: |.| <= 3 * 16384 * 32768 < 2^31
PCS_HD int box_project(int ax, int ay, int az, int x, int y, int z) { return ax * x + ay * y + az * z; }

}  // namespace pcs
