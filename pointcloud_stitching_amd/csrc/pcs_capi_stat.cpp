// pcs_capi_stat.cpp — statistical outlier removal's part of the C ABI (include/pcs_hip.h, "statistical outlier removal"): the
// argument checks, the workspace and the launches of pcs_kernels_stat.hip (the definition: DESIGN.md section 3; the kernels:
// section 5). The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter: they move
// records, like pcs_radius_outlier_device.

#include <climits>
#include <exception>

#include "pcs_host.h"

using namespace pcs_host;

namespace {

constexpr int    kMaxPoints  = INT_MAX / PCS_POINT_BYTES;      // a payload's byte count fits an int32 (as pcs_radius_outlier's)
constexpr size_t kStatsBytes = sizeof(pcs_stat_outlier_stats);
static_assert(kStatsBytes == 64, "the statistics block is eight int64");

// [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// What every form checks first; `who` names the entry point, the *_name its own argument names. stats may be NULL.
int check_args(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const char* n_name,
               const pcs_stat_outlier_params* params, const void* out, const char* out_name, size_t out_shorts, const void* out_points,
               const char* points_name, unsigned points_align, const void* stats, const char* stats_name)
{
    if (!params) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (params->mean_k < PCS_STAT_K_MIN || params->mean_k > PCS_STAT_K_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->mean_k %d is outside %d..%d", who, params->mean_k, PCS_STAT_K_MIN, PCS_STAT_K_MAX);
    if (params->std_mul_milli < 0 || params->std_mul_milli > PCS_STAT_MUL_MILLI_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->std_mul_milli %d is outside 0..%d", who, params->std_mul_milli, PCS_STAT_MUL_MILLI_MAX);
    if (params->max_dist_mm < PCS_STAT_DIST_MIN || params->max_dist_mm > PCS_STAT_DIST_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->max_dist_mm %d is outside %d..%d", who, params->max_dist_mm, PCS_STAT_DIST_MIN,
                    PCS_STAT_DIST_MAX);
    if (params->reserved != 0) return fail(c, PCS_ERR_INVALID_ARG, "%s: params->reserved %d is not 0", who, params->reserved);
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside 0..%d", who, n_name, n_points, kMaxPoints);
    if (!out_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, points_name);
    if (n_points && !in) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, in_name);
    if (n_points && !out) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, out_name);
    if ((uintptr_t)in & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, in_name);
    if ((uintptr_t)out & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, out_name);
    if ((uintptr_t)out_points & (points_align - 1u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not %u-byte aligned", who, points_name, points_align);
    if ((uintptr_t)stats & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, stats_name);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    if (out_shorts < (size_t)n_points * PCS_POINT_SHORTS)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: out_shorts %zu: %s must hold the worst case, every one of %d records kept: %zu shorts", who,
                    out_shorts, out_name, n_points, (size_t)n_points * PCS_POINT_SHORTS);
    if (ranges_overlap(in, bytes, out, bytes)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s and %s overlap", who, in_name, out_name);
    if (ranges_overlap(out_points, 4, out, bytes) || ranges_overlap(out_points, 4, in, bytes))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s or %s", who, points_name, in_name, out_name);
    const size_t sb = stats ? kStatsBytes : 0;
    if (ranges_overlap(stats, sb, out, bytes) || ranges_overlap(stats, sb, in, bytes) || ranges_overlap(stats, sb, out_points, 4))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s, %s or %s", who, stats_name, in_name, out_name, points_name);
    return PCS_OK;
}

// The filter's workspace is the radius filter's slab, asked for a larger size: pcs_capi_outlier.cpp's ensure_outlier_ws and its policy
// (a quarter of headroom when it grows; growing waits for the stream; it never shrinks).
int ensure_stat_ws(pcs_ctx* c, size_t need)
{
    if (need <= c->s_outlier_ws_cap && c->s_outlier_ws) return PCS_OK;
    const size_t exact = need;
    if (c->s_outlier_ws) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        need += need / 4;
    }
    int rc = ensure(c, c->s_outlier_ws, c->s_outlier_ws_cap, need);
    if (rc == PCS_ERR_NOMEM && need != exact) rc = ensure(c, c->s_outlier_ws, c->s_outlier_ws_cap, exact);      // the headroom is a wish
    return rc;
}

// The launches, behind the checks. capacity: n_points, or the counted form's max_points. d_stats NULL: no block, one launch fewer.
// stage_stats: the host form's — the block goes to the 64 bytes behind the workspace's own, *d_staged says where.
int run_device(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const pcs_stat_outlier_params& P,
               int16_t* d_out, int32_t* d_out_points, pcs_stat_outlier_stats* d_stats, pcs_stat_outlier_stats** d_staged = nullptr)
{
    DeviceGuard guard(c->device);
    if (capacity == 0) {         // nothing to launch: a zero count, a zeroed block
        HIPCHK(c, hipMemsetAsync(d_out_points, 0, sizeof(int32_t), c->stream));
        if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, kStatsBytes, c->stream));
        return PCS_OK;
    }
    const size_t need = stat_workspace_bytes((uint32_t)capacity);
    if (int rc = ensure_stat_ws(c, need)) return rc;
    if (d_staged) *d_staged = d_stats = reinterpret_cast<pcs_stat_outlier_stats*>(static_cast<uint8_t*>(c->s_outlier_ws) + need - 128);
    for (int stage = 0; stage < kStatStages - (d_stats ? 0 : 1); stage++) {
        // one bracket per launch: pcs_kernel_times_ms hands back one interval per launch, in launch order
        KernelTimer timer(c);
        if (timer.rc) return timer.rc;
        HIPCHK(c, launch_stat_stage(stage, d_payload, (uint32_t)capacity, d_n_points, (uint32_t)capacity, P.mean_k, P.std_mul_milli,
                                    P.max_dist_mm, c->s_outlier_ws, c->s_outlier_ws_cap, d_out, d_out_points,
                                    reinterpret_cast<long long*>(d_stats), c->stream));
        if (int rc = timer.finish()) return rc;
    }
    return PCS_OK;
}

}  // namespace

extern "C" {

int pcs_stat_outlier_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_stat_outlier_params* params, int16_t* d_out,
                            size_t out_shorts, int32_t* d_out_points, pcs_stat_outlier_stats* d_stats)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, "pcs_stat_outlier_device", d_payload, "d_payload", n_points, "n_points", params, d_out, "d_out", out_shorts,
                            d_out_points, "d_out_points", 4, d_stats, "d_stats"))
        return rc;
    return run_device(c, d_payload, n_points, nullptr, *params, d_out, d_out_points, d_stats);
}

int pcs_stat_outlier_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                    const pcs_stat_outlier_params* params, int16_t* d_out, size_t out_shorts, int32_t* d_out_points,
                                    pcs_stat_outlier_stats* d_stats)
{
    static const char who[] = "pcs_stat_outlier_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, who, d_payload, "d_payload", max_points, "max_points", params, d_out, "d_out", out_shorts, d_out_points,
                            "d_out_points", 4, d_stats, "d_stats"))
        return rc;
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if ((uintptr_t)d_n_points & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    if (ranges_overlap(d_n_points, 4, d_out, (size_t)max_points * PCS_POINT_BYTES) || ranges_overlap(d_n_points, 4, d_out_points, 4) ||
        ranges_overlap(d_n_points, 4, d_stats, d_stats ? kStatsBytes : 0))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points overlaps d_out, d_out_points or d_stats", who);
    return run_device(c, d_payload, max_points, d_n_points, *params, d_out, d_out_points, d_stats);
}

int pcs_stat_outlier(pcs_ctx* c, const int16_t* payload, int n_points, const pcs_stat_outlier_params* params, int16_t* out,
                     size_t out_shorts, int* out_points, pcs_stat_outlier_stats* stats)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, "pcs_stat_outlier", payload, "payload", n_points, "n_points", params, out, "out", out_shorts, out_points,
                            "out_points", (unsigned)alignof(int), stats, "stats"))
        return rc;
    if (n_points == 0) {
        *out_points = 0;
        if (stats) *stats = pcs_stat_outlier_stats{};
        return PCS_OK;
    }
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    // the host forms' payload staging (pcs_voxel_grid's and pcs_radius_outlier's: all synchronous, none leaves anything in it)
    int rc;
    if ((rc = ensure_idle(c, c->s_voxel_in, c->s_voxel_in_cap, bytes))) return rc;
    if ((rc = ensure_idle(c, c->s_voxel_out, c->s_voxel_out_cap, bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->s_voxel_in, payload, bytes, hipMemcpyHostToDevice, c->stream));
    pcs_stat_outlier_stats* d_block = nullptr;
    if ((rc = run_device(c, c->s_voxel_in, n_points, nullptr, *params, c->s_voxel_out, c->d_counts, nullptr, stats ? &d_block : nullptr)))
        return rc;
    int32_t kept = 0;
    pcs_stat_outlier_stats got{};
    HIPCHK(c, hipMemcpyAsync(&kept, c->d_counts, sizeof kept, hipMemcpyDeviceToHost, c->stream));
    if (d_block) HIPCHK(c, hipMemcpyAsync(&got, d_block, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (kept < 0 || kept > n_points) return fail(c, PCS_ERR_HIP, "pcs_stat_outlier: the kernels reported %d of %d records kept", kept, n_points);
    if (kept) HIPCHK(c, hipMemcpy(out, c->s_voxel_out, (size_t)kept * PCS_POINT_BYTES, hipMemcpyDeviceToHost));
    *out_points = kept;
    if (stats) *stats = got;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_stat_outlier: host allocation failed (%s)", ex.what());
}

}  // extern "C"
