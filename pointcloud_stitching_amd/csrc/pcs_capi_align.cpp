// pcs_capi_align.cpp — extrinsics refinement's part of the C ABI (include/pcs_hip.h, "extrinsics refinement" and "extrinsics
// refinement, point to plane"): the argument checks, the workspace and the launches of pcs_kernels_align.hip over the outlier filter's
// index (the definition: DESIGN.md section 3 "Alignment sums" and "Plane sums"; the kernels: section 5), the two fits on the host
// (pcs_align_solve: exact 128-bit covariance, a one-sided Jacobi SVD in double; pcs_align_plane_solve: the 6 x 6 normal equations) and
// the ICP loop, written once for both. The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do
// not matter: the loop moves the source through launch_transform_payloads itself, pcs_transform_payloads_device's arithmetic without
// its context checks. The plane forms have the target's normals beside the index: everything else is shared, told apart by the
// number of int64 terms of the sums (kAlignTerms / kPlaneTerms).

#include <cmath>
#include <cstring>
#include <exception>

#include "pcs_host.h"

using namespace pcs_host;

using AlignSums = struct pcs_align_sums;          // (the bare names are the host forms, functions)
using PlaneSums = struct pcs_align_plane_sums;

static_assert(sizeof(AlignSums) == kAlignTerms * sizeof(int64_t), "pcs_align_sums is kAlignTerms int64 words, no padding");
static_assert(sizeof(PlaneSums) == kPlaneTerms * sizeof(int64_t), "pcs_align_plane_sums is kPlaneTerms int64 words, no padding");
static_assert(sizeof(pcs_align_plane_params) == 64, "pcs_align_plane_params: pcs_align_params' fields, then pcs_normal_params");

namespace {

// What the sums forms and the loop check about their payloads; `who` names the entry point.
int check_payloads(pcs_ctx* c, const char* who, const void* source, const char* s_name, int n_source, const void* target,
                   const char* t_name, int n_target, int max_dist_mm)
{
    if (max_dist_mm < PCS_ALIGN_DIST_MIN || max_dist_mm > PCS_ALIGN_DIST_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: max_dist_mm %d is outside %d..%d", who, max_dist_mm, PCS_ALIGN_DIST_MIN, PCS_ALIGN_DIST_MAX);
    if (n_source < 0 || n_source > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: n_source %d is outside 0..%d", who, n_source, kMaxPoints);
    if (n_target < 0 || n_target > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: n_target %d is outside 0..%d", who, n_target, kMaxPoints);
    if (n_source && !source) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, s_name);
    if (n_target && !target) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, t_name);
    if ((uintptr_t)source & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, s_name);
    if ((uintptr_t)target & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, t_name);
    return PCS_OK;
}

int check_sums_args(pcs_ctx* c, const char* who, const void* source, const char* s_name, int n_source, const void* target,
                    const char* t_name, int n_target, int max_dist_mm, const void* sums, const char* sums_name, const void* dist2,
                    const char* dist2_name)
{
    if (int rc = check_payloads(c, who, source, s_name, n_source, target, t_name, n_target, max_dist_mm)) return rc;
    if (!sums) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, sums_name);
    if ((uintptr_t)sums & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, sums_name);
    if ((uintptr_t)dist2 & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, dist2_name);
    const size_t sb = (size_t)n_source * PCS_POINT_BYTES, tb = (size_t)n_target * PCS_POINT_BYTES, db = (size_t)n_source * 4;
    if (ranges_overlap(sums, sizeof(AlignSums), source, sb) || ranges_overlap(sums, sizeof(AlignSums), target, tb))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s or %s", who, sums_name, s_name, t_name);
    if (ranges_overlap(dist2, db, source, sb) || ranges_overlap(dist2, db, target, tb))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s or %s", who, dist2_name, s_name, t_name);
    if (ranges_overlap(dist2, db, sums, sizeof(AlignSums)))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, dist2_name, sums_name);
    return PCS_OK;
}

int check_plane_sums_args(pcs_ctx* c, const char* who, const void* source, const char* s_name, int n_source, const void* target,
                          const char* t_name, int n_target, const void* normals, const char* n_name, int max_dist_mm, const void* sums,
                          const char* sums_name, const void* dist2, const char* dist2_name)
{
    if (int rc = check_payloads(c, who, source, s_name, n_source, target, t_name, n_target, max_dist_mm)) return rc;
    if (n_target && !normals) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, n_name);
    if ((uintptr_t)normals & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, n_name);
    if (!sums) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, sums_name);
    if ((uintptr_t)sums & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, sums_name);
    if ((uintptr_t)dist2 & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, dist2_name);
    const size_t sb = (size_t)n_source * PCS_POINT_BYTES, tb = (size_t)n_target * PCS_POINT_BYTES, db = (size_t)n_source * 4,
                 nb = (size_t)n_target * PCS_NORMAL_BYTES;
    if (ranges_overlap(sums, sizeof(PlaneSums), source, sb) || ranges_overlap(sums, sizeof(PlaneSums), target, tb) ||
        ranges_overlap(sums, sizeof(PlaneSums), normals, nb))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s, %s or %s", who, sums_name, s_name, t_name, n_name);
    if (ranges_overlap(dist2, db, source, sb) || ranges_overlap(dist2, db, target, tb) || ranges_overlap(dist2, db, normals, nb))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s, %s or %s", who, dist2_name, s_name, t_name, n_name);
    if (ranges_overlap(dist2, db, sums, sizeof(PlaneSums)))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, dist2_name, sums_name);
    return PCS_OK;
}

// One call's carve of the align workspace: the target's index first (outlier_workspace_bytes(n_target), 256-byte aligned as the slab
// is), then the partials (`terms` int64 each), the plane forms' normals in cell order, then what the form asked for.
struct AlignWs {
    void*               index = nullptr;  size_t index_bytes = 0;
    long long*          partials = nullptr;
    unsigned long long* pnorm = nullptr;  size_t pnorm_bytes = 0;      // plane: parallel to the index's xyz[]
    int16_t*            moved = nullptr;          // the loop's moved source
    long long*          sums = nullptr;           // the loop's / the host form's sums, `terms` words
    uint32_t*           dist2 = nullptr;          // the host form's dist2
    int16_t*            normals = nullptr;        // plane: the host form's staged / the loop's estimated target normals (record order)
};
enum : unsigned { kWsMoved = 1, kWsSums = 2, kWsDist2 = 4, kWsNormals = 8 };
int carve_align_ws(pcs_ctx* c, int terms, int n_source, int n_target, unsigned want, AlignWs* ws)
{
    const size_t index_bytes = n_target ? up256(outlier_workspace_bytes((uint32_t)n_target)) : 0;
    const size_t part_bytes = up256((size_t)align_partials((uint32_t)n_source) * terms * sizeof(long long));
    const size_t pnorm_bytes = terms == kPlaneTerms ? up256((size_t)n_target * PCS_NORMAL_BYTES) : 0;
    const size_t moved_bytes = (want & kWsMoved) ? up256((size_t)n_source * PCS_POINT_BYTES) : 0;
    const size_t sums_bytes = (want & kWsSums) ? up256((size_t)terms * sizeof(long long)) : 0;
    const size_t dist2_bytes = (want & kWsDist2) ? up256((size_t)n_source * 4) : 0;
    const size_t normals_bytes = (want & kWsNormals) ? up256((size_t)n_target * PCS_NORMAL_BYTES) : 0;
    if (int rc = ensure_ws(c, c->s_align_ws, c->s_align_ws_cap,
                           index_bytes + part_bytes + pnorm_bytes + moved_bytes + sums_bytes + dist2_bytes + normals_bytes))
        return rc;
    uint8_t* w = static_cast<uint8_t*>(c->s_align_ws);
    ws->index = w; ws->index_bytes = index_bytes; w += index_bytes;
    ws->partials = reinterpret_cast<long long*>(w); w += part_bytes;
    ws->pnorm = reinterpret_cast<unsigned long long*>(w); ws->pnorm_bytes = (size_t)n_target * PCS_NORMAL_BYTES; w += pnorm_bytes;
    ws->moved = reinterpret_cast<int16_t*>(w); w += moved_bytes;
    ws->sums = reinterpret_cast<long long*>(w); w += sums_bytes;
    ws->dist2 = reinterpret_cast<uint32_t*>(w); w += dist2_bytes;
    ws->normals = reinterpret_cast<int16_t*>(w);
    return PCS_OK;
}

// The target's cell index, cell edge max_dist_mm, and with d_target_normals (the plane forms) those normals scattered beside it:
// pnorm set to all ones on the stream, then one launch. n_target == 0: nothing launched, *have = false.
int build_target_index(pcs_ctx* c, const int16_t* d_target, int n_target, const int16_t* d_target_normals, int max_dist_mm, const AlignWs& ws,
                       OutlierIndexView* view, bool* have)
{
    *have = n_target > 0;
    if (!*have) return PCS_OK;
    if (int rc = build_cell_index(c, d_target, n_target, max_dist_mm, ws.index, ws.index_bytes, view)) return rc;
    if (!d_target_normals) return PCS_OK;
    HIPCHK(c, hipMemsetAsync(ws.pnorm, 0xFF, ws.pnorm_bytes, c->stream));
    PCS_TIMED(c, launch_align_plane_scatter(d_target, d_target_normals, (uint32_t)n_target, *view, max_dist_mm, ws.pnorm, c->stream));
    return PCS_OK;
}

// match + reduce of n_source records at d_source into d_sums[terms] (and d_dist2): two launches, one with an empty source.
int run_match(pcs_ctx* c, int terms, const int16_t* d_source, int n_source, const OutlierIndexView* view, int max_dist_mm, const AlignWs& ws,
              long long* d_sums, uint32_t* d_dist2)
{
    const uint32_t n = (uint32_t)n_source;
    if (terms == kPlaneTerms) {
        if (n) PCS_TIMED(c, launch_align_plane_match(d_source, n, view, ws.pnorm, max_dist_mm, ws.partials, d_dist2, c->stream));
        PCS_TIMED(c, launch_align_plane_reduce(ws.partials, align_partials(n), d_sums, c->stream));
    } else {
        if (n) PCS_TIMED(c, launch_align_match(d_source, n, view, max_dist_mm, ws.partials, d_dist2, c->stream));
        PCS_TIMED(c, launch_align_reduce(ws.partials, align_partials(n), d_sums, c->stream));
    }
    return PCS_OK;
}

// The sums forms behind their checks. Device: d_target_normals is the caller's (nullptr: point to point). Host: source, target and
// normals staged (the normals in the align workspace), the sums and dist2 fetched; *out is written whole, at the end.
int sums_device(pcs_ctx* c, int terms, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                const int16_t* d_target_normals, int max_dist_mm, void* d_sums, uint32_t* d_dist2)
{
    DeviceGuard guard(c->device);
    AlignWs ws;
    if (int rc = carve_align_ws(c, terms, n_source, n_source ? n_target : 0, 0, &ws)) return rc;
    OutlierIndexView view{};
    bool have = false;
    if (n_source)          // (an empty source needs no index)
        if (int rc = build_target_index(c, d_target, n_target, d_target_normals, max_dist_mm, ws, &view, &have)) return rc;
    return run_match(c, terms, d_source, n_source, have ? &view : nullptr, max_dist_mm, ws, static_cast<long long*>(d_sums), d_dist2);
}

int sums_host(pcs_ctx* c, int terms, const int16_t* source, int n_source, const int16_t* target, int n_target, const int16_t* target_normals,
              int max_dist_mm, void* out, uint32_t* dist2)
{
    DeviceGuard guard(c->device);
    const bool plane = terms == kPlaneTerms;
    const size_t tb = (size_t)n_target * PCS_POINT_BYTES;
    if (int rc = stage_payload(c, source, (size_t)n_source * PCS_POINT_BYTES, tb)) return rc;
    AlignWs ws;
    if (int rc = carve_align_ws(c, terms, n_source, n_source ? n_target : 0, kWsSums | (dist2 ? kWsDist2 : 0) | (plane ? kWsNormals : 0), &ws))
        return rc;
    if (tb && n_source) {
        HIPCHK(c, hipMemcpyAsync(c->s_voxel_out, target, tb, hipMemcpyHostToDevice, c->stream));
        if (plane) HIPCHK(c, hipMemcpyAsync(ws.normals, target_normals, (size_t)n_target * PCS_NORMAL_BYTES, hipMemcpyHostToDevice, c->stream));
    }
    OutlierIndexView view{};
    bool have = false;
    if (n_source)
        if (int rc = build_target_index(c, c->s_voxel_out, n_target, plane ? ws.normals : nullptr, max_dist_mm, ws, &view, &have)) return rc;
    if (int rc = run_match(c, terms, c->s_voxel_in, n_source, have ? &view : nullptr, max_dist_mm, ws, ws.sums, dist2 ? ws.dist2 : nullptr)) return rc;
    long long got[kPlaneTerms];
    if (int rc = fetch(c, got, ws.sums, (size_t)terms * sizeof(long long))) return rc;
    if (dist2 && n_source) HIPCHK(c, hipMemcpy(dist2, ws.dist2, (size_t)n_source * 4, hipMemcpyDeviceToHost));
    std::memcpy(out, got, (size_t)terms * sizeof(long long));
    return PCS_OK;
}

// ---- the rigid fit -----------------------------------------------------------------------------------
// One-sided Jacobi (Hestenes) on the columns of A (3 x 3, row-major): A V -> columns orthogonal, V the accumulated rotations. Then
// sigma_j = |column j|. Small singular values come out with high relative accuracy, which the degeneracy test below needs (an
// eigen-decomposition of A^T A would square the condition number past double precision at the 1e-9 threshold).
void jacobi_columns(double A[9], double V[9])
{
    for (int k = 0; k < 9; k++) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < 3; i++) {
                    alpha += A[3 * i + p] * A[3 * i + p];
                    beta  += A[3 * i + q] * A[3 * i + q];
                    gamma += A[3 * i + p] * A[3 * i + q];
                }
                if (gamma == 0.0 || std::fabs(gamma) <= 1e-16 * std::sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < 3; i++) {
                    const double ap = A[3 * i + p], aq = A[3 * i + q];
                    A[3 * i + p] = cs * ap - sn * aq;
                    A[3 * i + q] = sn * ap + cs * aq;
                    const double vp = V[3 * i + p], vq = V[3 * i + q];
                    V[3 * i + p] = cs * vp - sn * vq;
                    V[3 * i + q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
}

void cross3(const double a[3], const double b[3], double out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

bool normalise3(double v[3])
{
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(n > 0)) return false;
    v[0] /= n; v[1] /= n; v[2] /= n;
    return true;
}

int solve_sums(const AlignSums& s, double delta[16], double* rms_mm)
{
    static const char who[] = "pcs_align_solve";
    if (s.matched < 3) return fail(nullptr, PCS_ERR_UNSUPPORTED, "%s: matched %lld < 3: no rigid fit", who, (long long)s.matched);
    const __int128 n = s.matched;
    double A[9], V[9], scale = 0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const __int128 cab = n * (__int128)s.spq[3 * a + b] - (__int128)s.sp[a] * (__int128)s.sq[b];     // exact
            A[3 * a + b] = (double)cab;
            scale = std::max(scale, std::fabs(A[3 * a + b]));
        }
    if (scale == 0.0)
        return fail(nullptr, PCS_ERR_UNSUPPORTED, "%s: degenerate: the covariance is zero (all matched points of one side coincide)", who);
    for (double& v : A) v /= scale;
    jacobi_columns(A, V);              // C / scale = U S V^T with A = U S
    double sig[3];
    int order[3] = {0, 1, 2};
    for (int j = 0; j < 3; j++) sig[j] = std::sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    std::sort(order, order + 3, [&](int x, int y) { return sig[x] > sig[y]; });
    if (!(sig[order[1]] > 1e-9 * sig[order[0]]))
        return fail(nullptr, PCS_ERR_UNSUPPORTED, "%s: degenerate: the covariance's second singular value is at most 1e-9 of its first "
                    "(collinear or coincident points): the rotation is not unique", who);
    // u1, u2, v1, v2 from the two largest singular values; u3 = u1 x u2 and v3 = v1 x v2 make det U = det V = +1, which IS the
    // diag(1, 1, det(V U^T)) of the definition: flipping u3 or v3 flips that determinant with it, the product v3 u3^T d stays.
    double u[3][3], v[3][3];
    for (int k = 0; k < 2; k++) {
        const int j = order[k];
        for (int i = 0; i < 3; i++) { u[k][i] = A[3 * i + j] / sig[j]; v[k][i] = V[3 * i + j]; }
    }
    const double dot = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];        // (~1e-16: what the sweeps left)
    for (int i = 0; i < 3; i++) u[1][i] -= dot * u[0][i];
    if (!normalise3(u[0]) || !normalise3(u[1]) || !normalise3(v[0]) || !normalise3(v[1]))
        return fail(nullptr, PCS_ERR_UNSUPPORTED, "%s: degenerate: a singular vector vanished", who);
    cross3(u[0], u[1], u[2]);
    cross3(v[0], v[1], v[2]);
    double R[9];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) R[3 * a + b] = v[0][a] * u[0][b] + v[1][a] * u[1][b] + v[2][a] * u[2][b];
    const double nd = (double)s.matched;
    const double pb[3] = {(double)s.sp[0] / nd, (double)s.sp[1] / nd, (double)s.sp[2] / nd};
    const double qb[3] = {(double)s.sq[0] / nd, (double)s.sq[1] / nd, (double)s.sq[2] / nd};
    for (int a = 0; a < 3; a++) {
        const double t_mm = qb[a] - (R[3 * a] * pb[0] + R[3 * a + 1] * pb[1] + R[3 * a + 2] * pb[2]);
        delta[4 * a] = R[3 * a]; delta[4 * a + 1] = R[3 * a + 1]; delta[4 * a + 2] = R[3 * a + 2];
        delta[4 * a + 3] = t_mm / 1000.0;
    }
    delta[12] = delta[13] = delta[14] = 0.0; delta[15] = 1.0;
    if (rms_mm) *rms_mm = std::sqrt((double)s.sd2 / nd);
    return PCS_OK;
}

// ---- the 6 x 6 solve ----------------------------------------------------------------------------------
// Cyclic Jacobi on a symmetric n x n (row-major, n = 6): A -> diagonal, V the accumulated rotations (columns: eigenvectors).
void jacobi_symmetric6(double A[36], double V[36])
{
    constexpr int n = 6;
    for (int k = 0; k < n * n; k++) V[k] = (k % (n + 1) == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
        for (int i = 0; i < n; i++) {
            diag += std::fabs(A[n * i + i]);
            for (int j = i + 1; j < n; j++) off += std::fabs(A[n * i + j]);
        }
        if (off <= 1e-18 * diag) break;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[n * p + q];
                if (apq == 0.0) continue;
                const double theta = (A[n * q + q] - A[n * p + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                A[n * p + p] -= t * apq;
                A[n * q + q] += t * apq;
                A[n * p + q] = A[n * q + p] = 0.0;
                for (int r = 0; r < n; r++) {
                    if (r != p && r != q) {
                        const double arp = A[n * r + p], arq = A[n * r + q];
                        A[n * r + p] = A[n * p + r] = cs * arp - sn * arq;
                        A[n * r + q] = A[n * q + r] = sn * arp + cs * arq;
                    }
                    const double vp = V[n * r + p], vq = V[n * r + q];
                    V[n * r + p] = cs * vp - sn * vq;
                    V[n * r + q] = sn * vp + cs * vq;
                }
            }
    }
}

inline double recombine(int64_t hi, int64_t lo) { return (double)((__int128)hi * ((__int128)1 << 32) + (__int128)lo); }

int solve_plane_sums(const PlaneSums& s, double delta[16], double* rms_mm)
{
    static const char who[] = "pcs_align_plane_solve";
    if (s.used < PCS_ALIGN_PLANE_USED_MIN)
        return fail(nullptr, PCS_ERR_UNSUPPORTED, "%s: used %lld < %d: six unknowns", who, (long long)s.used, PCS_ALIGN_PLANE_USED_MIN);
    double M[36], r[6], w[6];
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++, k++) M[6 * i + j] = M[6 * j + i] = recombine(s.ata_hi[k], s.ata_lo[k]);      // exact, rounded once
    for (int i = 0; i < 6; i++) {
        r[i] = recombine(s.atb_hi[i], s.atb_lo[i]);
        if (!(M[7 * i] > 0.0))
            return fail(nullptr, PCS_ERR_UNSUPPORTED, "%s: degenerate: diagonal entry %d of A^T A is zero (%s)", who, i,
                        i < 3 ? "every used p x n has no such component" : "every used normal has no such component");
        w[i] = std::sqrt(M[7 * i]);
    }
    double A[36], V[36];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) A[6 * i + j] = i == j ? 1.0 : M[6 * i + j] / (w[i] * w[j]);
    jacobi_symmetric6(A, V);
    double lmin = A[0], lmax = A[0];
    for (int i = 1; i < 6; i++) { lmin = std::min(lmin, A[7 * i]); lmax = std::max(lmax, A[7 * i]); }
    if (!(lmin > 1e-9 * lmax))
        return fail(nullptr, PCS_ERR_UNSUPPORTED, "%s: degenerate: the smallest eigenvalue of the scaled A^T A is at most 1e-9 of its largest "
                    "(the used normals do not span the pose: one plane, or parallel planes)", who);
    // x = W^-1 V diag(1 / lambda) V^T W^-1 r
    double y[6], x[6];
    for (int j = 0; j < 6; j++) {
        double dot = 0;
        for (int i = 0; i < 6; i++) dot += V[6 * i + j] * (r[i] / w[i]);
        y[j] = dot / A[7 * j];
    }
    for (int i = 0; i < 6; i++) {
        double v = 0;
        for (int j = 0; j < 6; j++) v += V[6 * i + j] * y[j];
        x[i] = v / w[i];
    }
    // Rodrigues: R = I + a K + b K^2, K = [omega]x
    const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], th = std::sqrt(th2);
    const double ca = th < 1e-4 ? 1.0 - th2 / 6.0 : std::sin(th) / th;
    const double cb = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2;
    const double K[9] = {0, -x[2], x[1], x[2], 0, -x[0], -x[1], x[0], 0};
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) {
            const double k2 = K[3 * a] * K[b] + K[3 * a + 1] * K[3 + b] + K[3 * a + 2] * K[6 + b];
            delta[4 * a + b] = (a == b ? 1.0 : 0.0) + ca * K[3 * a + b] + cb * k2;
        }
        delta[4 * a + 3] = x[3 + a] / 1000.0;
    }
    delta[12] = delta[13] = delta[14] = 0.0; delta[15] = 1.0;
    if (rms_mm) *rms_mm = std::sqrt(recombine(s.sb2_hi, s.sb2_lo) / (double)s.used) / 16384.0;
    return PCS_OK;
}

template <class Sums>
double rms_of(const Sums& s) { return s.matched > 0 ? std::sqrt((double)s.sd2 / (double)s.matched) : 0.0; }

// ---- the ICP loop ------------------------------------------------------------------------------------
// What the two loops differ in: the types, how the target is prepared once per call, the solve, and the `used` words of the report.
// Params begins with max_dist_mm, iterations, source_stride, eps_rot_rad, eps_trans_mm in both (the static_assert above).
struct PointLoop {
    using Sums = AlignSums; using Params = pcs_align_params; using Report = pcs_align_report;
    static constexpr const char* who = "pcs_align_payloads_device";
    static constexpr int      terms = kAlignTerms;
    static constexpr unsigned want = kWsMoved | kWsSums;
    static int check(pcs_ctx*, const Params&) { return PCS_OK; }
    static int prepare(pcs_ctx* c, const int16_t* d_target, int n_target, const Params& P, const AlignWs& ws, OutlierIndexView* view, bool* have)
    {
        return build_target_index(c, d_target, n_target, nullptr, P.max_dist_mm, ws, view, have);
    }
    static int solve(const Sums& s, double D[16]) { return solve_sums(s, D, nullptr); }
    static void used(Report&, const Sums&, bool) {}
};
struct PlaneLoop {
    using Sums = PlaneSums; using Params = pcs_align_plane_params; using Report = pcs_align_plane_report;
    static constexpr const char* who = "pcs_align_payloads_plane_device";
    static constexpr int      terms = kPlaneTerms;
    static constexpr unsigned want = kWsMoved | kWsSums | kWsNormals;
    static int check(pcs_ctx* c, const Params& P) { return check_normal_params(c, who, &P.normals); }
    // the target's normals, its index, the normals beside it
    static int prepare(pcs_ctx* c, const int16_t* d_target, int n_target, const Params& P, const AlignWs& ws, OutlierIndexView* view, bool* have)
    {
        if (n_target)
            if (int rc = run_normals_device(c, d_target, n_target, P.normals, ws.normals, nullptr)) return rc;
        return build_target_index(c, d_target, n_target, ws.normals, P.max_dist_mm, ws, view, have);
    }
    static int solve(const Sums& s, double D[16]) { return solve_plane_sums(s, D, nullptr); }
    static void used(Report& r, const Sums& s, bool first) { (first ? r.first_used : r.last_used) = s.used; }
};

template <class K>
int align_loop(pcs_ctx* c, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target, const typename K::Params* params,
               const float init[16], float out[16], typename K::Report* report)
{
    using Sums = typename K::Sums;
    const char* const who = K::who;
    if (!c) return PCS_ERR_INVALID_ARG;
    if (!params) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (int rc = check_payloads(c, who, d_source, "d_source", n_source, d_target, "d_target", n_target, params->max_dist_mm)) return rc;
    if (params->iterations < 1 || params->iterations > PCS_ALIGN_ITERATIONS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: iterations %d is outside 1..%d", who, params->iterations, PCS_ALIGN_ITERATIONS_MAX);
    if (params->source_stride < 1) return fail(c, PCS_ERR_INVALID_ARG, "%s: source_stride %d < 1", who, params->source_stride);
    if (!(params->eps_rot_rad >= 0) || !std::isfinite(params->eps_rot_rad))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: eps_rot_rad is negative or not finite", who);
    if (!(params->eps_trans_mm >= 0) || !std::isfinite(params->eps_trans_mm))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: eps_trans_mm is negative or not finite", who);
    if (int rc = K::check(c, *params)) return rc;
    if (!init) return fail(c, PCS_ERR_INVALID_ARG, "%s: init is NULL", who);
    if (!out) return fail(c, PCS_ERR_INVALID_ARG, "%s: out is NULL", who);
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(init[k])) return fail(c, PCS_ERR_INVALID_ARG, "%s: init[%d] is not finite", who, k);
    int trace_cap = 0;
    if (report) {
        if (report->trace_capacity < 0) return fail(c, PCS_ERR_INVALID_ARG, "%s: report->trace_capacity %d < 0", who, report->trace_capacity);
        trace_cap = report->trace_capacity;
    }
    float* const trace_f = report ? report->trace_transforms : nullptr;
    Sums* const trace_s = report ? report->trace_sums : nullptr;
    const NamedRange ins[] = {{d_source, (size_t)n_source * PCS_POINT_BYTES, "d_source"}, {d_target, (size_t)n_target * PCS_POINT_BYTES, "d_target"},
                              {init, 16 * sizeof(float), "init"}, {params, sizeof *params, "params"}};
    const NamedRange outs[] = {{out, 16 * sizeof(float), "out"}, {report, sizeof *report, "report"},
                               {trace_f, (size_t)trace_cap * 16 * sizeof(float), "report->trace_transforms"},
                               {trace_s, (size_t)trace_cap * sizeof(Sums), "report->trace_sums"}};
    const NamedRange* with = nullptr;
    if (const NamedRange* bad = first_overlap(outs, 4, ins, 4, &with))
        return with ? fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, bad->name, with->name)
                    : fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps an input", who, bad->name);

    DeviceGuard guard(c->device);
    const typename K::Params P = *params;
    const int n_moved = n_source / P.source_stride;          // FLOOR, pcs_transform_payloads_device's rule
    AlignWs ws;
    if (int rc = carve_align_ws(c, K::terms, n_moved, n_moved ? n_target : 0, K::want, &ws)) return rc;
    OutlierIndexView view{};
    bool have = false;
    if (n_moved)
        if (int rc = K::prepare(c, d_target, n_target, P, ws, &view, &have)) return rc;      // once per call

    double T[16];
    for (int k = 0; k < 16; k++) T[k] = init[k];
    typename K::Report rep{};
    rep.trace_capacity = trace_cap; rep.trace_transforms = trace_f; rep.trace_sums = trace_s;
    rep.stop_reason = PCS_ALIGN_STOP_ITERATIONS;
    int status = PCS_OK;
    const bool may_stop = P.eps_rot_rad > 0 || P.eps_trans_mm > 0;
    for (int k = 0; k < P.iterations; k++) {
        float F[16];
        for (int j = 0; j < 16; j++) F[j] = (float)T[j];
        if (n_moved) {
            XformBatch xb;
            std::memset(&xb, 0, sizeof xb);
            xb.c[0].in = d_source;
            xb.c[0].out = reinterpret_cast<uint8_t*>(ws.moved);
            xb.c[0].n_out = (uint32_t)n_moved;
            xb.c[0].ds = (uint32_t)P.source_stride;
            std::memcpy(xb.c[0].M, F, sizeof xb.c[0].M);
            PCS_TIMED(c, launch_transform_payloads(xb, 1, (uint32_t)n_moved, c->stream));
        }
        if (int rc = run_match(c, K::terms, ws.moved, n_moved, have ? &view : nullptr, P.max_dist_mm, ws, ws.sums, nullptr)) return rc;
        Sums S;
        if (int rc = fetch(c, &S, ws.sums, sizeof S)) return rc;
        if (k < trace_cap) {
            if (trace_f) std::memcpy(trace_f + 16 * (size_t)k, F, sizeof F);
            if (trace_s) trace_s[k] = S;
            rep.trace_count = k + 1;
        }
        rep.iterations = k + 1;
        if (k == 0) { rep.first_matched = S.matched; rep.first_considered = S.considered; rep.first_rms_mm = rms_of(S); K::used(rep, S, true); }
        rep.last_matched = S.matched; rep.last_considered = S.considered; rep.last_rms_mm = rms_of(S); K::used(rep, S, false);
        double D[16];
        const int rc = K::solve(S, D);
        if (rc) {
            // the solve speaks through pcs_last_error(NULL); the loop's caller has a context
            status = fail(c, rc, "%s: iteration %d: %s", who, k, pcs_last_error(nullptr));
            rep.stop_reason = PCS_ALIGN_STOP_REFUSED;
            break;
        }
        double N[16];
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) N[4 * a + b] = D[4 * a] * T[b] + D[4 * a + 1] * T[4 + b] + D[4 * a + 2] * T[8 + b] + D[4 * a + 3] * T[12 + b];
        std::memcpy(T, N, sizeof T);
        if (may_stop) {
            // the angle from both the trace and the antisymmetric part: exact for small angles, where acos(trace) is not
            const double sx = D[9] - D[6], sy = D[2] - D[8], sz = D[4] - D[1];
            const double angle = std::atan2(0.5 * std::sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (D[0] + D[5] + D[10] - 1.0));
            const double trans_mm = 1000.0 * std::sqrt(D[3] * D[3] + D[7] * D[7] + D[11] * D[11]);
            if (angle <= P.eps_rot_rad && trans_mm <= P.eps_trans_mm) { rep.stop_reason = PCS_ALIGN_STOP_CONVERGED; break; }
        }
    }
    for (int j = 0; j < 16; j++) out[j] = (float)T[j];
    if (report) *report = rep;
    return status;
}

}  // namespace

extern "C" {

int pcs_align_sums_device(pcs_ctx* c, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target, int max_dist_mm,
                          AlignSums* d_sums, uint32_t* d_dist2)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_sums_args(c, "pcs_align_sums_device", d_source, "d_source", n_source, d_target, "d_target", n_target, max_dist_mm,
                                 d_sums, "d_sums", d_dist2, "d_dist2"))
        return rc;
    return sums_device(c, kAlignTerms, d_source, n_source, d_target, n_target, nullptr, max_dist_mm, d_sums, d_dist2);
}

int pcs_align_sums(pcs_ctx* c, const int16_t* source, int n_source, const int16_t* target, int n_target, int max_dist_mm,
                   AlignSums* out, uint32_t* dist2)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_sums_args(c, "pcs_align_sums", source, "source", n_source, target, "target", n_target, max_dist_mm, out, "out",
                                 dist2, "dist2"))
        return rc;
    return sums_host(c, kAlignTerms, source, n_source, target, n_target, nullptr, max_dist_mm, out, dist2);
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_align_sums: host allocation failed (%s)", ex.what());
}

int pcs_align_solve(const AlignSums* sums, double delta[16], double* rms_mm)
{
    if (!sums) return fail(nullptr, PCS_ERR_INVALID_ARG, "pcs_align_solve: sums is NULL");
    if (!delta) return fail(nullptr, PCS_ERR_INVALID_ARG, "pcs_align_solve: delta is NULL");
    if (sums->matched < 0 || sums->considered < sums->matched)
        return fail(nullptr, PCS_ERR_INVALID_ARG, "pcs_align_solve: matched %lld is outside 0..considered %lld", (long long)sums->matched,
                    (long long)sums->considered);
    double d[16], rms = 0;
    if (int rc = solve_sums(*sums, d, &rms)) return rc;
    std::memcpy(delta, d, sizeof d);
    if (rms_mm) *rms_mm = rms;
    return PCS_OK;
}

int pcs_align_payloads_device(pcs_ctx* c, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                              const pcs_align_params* params, const float init[16], float out[16], pcs_align_report* report)
{
    return align_loop<PointLoop>(c, d_source, n_source, d_target, n_target, params, init, out, report);
}

int pcs_align_plane_sums_device(pcs_ctx* c, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                                const int16_t* d_target_normals, int max_dist_mm, PlaneSums* d_sums, uint32_t* d_dist2)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_plane_sums_args(c, "pcs_align_plane_sums_device", d_source, "d_source", n_source, d_target, "d_target", n_target,
                                       d_target_normals, "d_target_normals", max_dist_mm, d_sums, "d_sums", d_dist2, "d_dist2"))
        return rc;
    return sums_device(c, kPlaneTerms, d_source, n_source, d_target, n_target, d_target_normals, max_dist_mm, d_sums, d_dist2);
}

int pcs_align_plane_sums(pcs_ctx* c, const int16_t* source, int n_source, const int16_t* target, int n_target, const int16_t* target_normals,
                         int max_dist_mm, PlaneSums* out, uint32_t* dist2)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_plane_sums_args(c, "pcs_align_plane_sums", source, "source", n_source, target, "target", n_target, target_normals,
                                       "target_normals", max_dist_mm, out, "out", dist2, "dist2"))
        return rc;
    return sums_host(c, kPlaneTerms, source, n_source, target, n_target, target_normals, max_dist_mm, out, dist2);
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_align_plane_sums: host allocation failed (%s)", ex.what());
}

int pcs_align_plane_solve(const PlaneSums* sums, double delta[16], double* rms_mm)
{
    if (!sums) return fail(nullptr, PCS_ERR_INVALID_ARG, "pcs_align_plane_solve: sums is NULL");
    if (!delta) return fail(nullptr, PCS_ERR_INVALID_ARG, "pcs_align_plane_solve: delta is NULL");
    if (sums->used < 0 || sums->matched < sums->used || sums->considered < sums->matched)
        return fail(nullptr, PCS_ERR_INVALID_ARG, "pcs_align_plane_solve: used %lld, matched %lld, considered %lld are not 0 <= used <= matched "
                    "<= considered", (long long)sums->used, (long long)sums->matched, (long long)sums->considered);
    double d[16], rms = 0;
    if (int rc = solve_plane_sums(*sums, d, &rms)) return rc;
    std::memcpy(delta, d, sizeof d);
    if (rms_mm) *rms_mm = rms;
    return PCS_OK;
}

int pcs_align_payloads_plane_device(pcs_ctx* c, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                                    const pcs_align_plane_params* params, const float init[16], float out[16], pcs_align_plane_report* report)
{
    return align_loop<PlaneLoop>(c, d_source, n_source, d_target, n_target, params, init, out, report);
}

}  // extern "C"
