// pcs_capi_stat.cpp — statistical outlier removal's part of the C ABI (include/pcs_hip.h, "statistical outlier removal"): the
// argument checks, the workspace and the launches of pcs_kernels_stat.hip (the definition: DESIGN.md section 3; the kernels:
// section 5). The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter: they move
// records, like pcs_radius_outlier_device.

#include <exception>

#include "pcs_host.h"

using namespace pcs_host;

namespace {

constexpr size_t kStatsBytes = sizeof(pcs_stat_outlier_stats);
static_assert(kStatsBytes == 64, "the statistics block is eight int64");

// What every form checks first: the filter's own parameters, then check_payload_io with the statistics block (stats may be NULL);
// `who` names the entry point, the *_name its own argument names.
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
    return check_payload_io(c, who, in, in_name, n_points, n_name, out, out_name, out_shorts, out_points, points_name, points_align, stats,
                            stats_name, kStatsBytes);
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
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, need)) return rc;      // the radius filter's slab, asked for more
    if (d_staged) *d_staged = d_stats = reinterpret_cast<pcs_stat_outlier_stats*>(static_cast<uint8_t*>(c->s_outlier_ws) + need - 128);
    // one bracket per launch: pcs_kernel_times_ms hands back one interval per launch, in launch order
    for (int stage = 0; stage < kStatStages - (d_stats ? 0 : 1); stage++)
        PCS_TIMED(c, launch_stat_stage(stage, d_payload, (uint32_t)capacity, d_n_points, (uint32_t)capacity, P.mean_k, P.std_mul_milli,
                                       P.max_dist_mm, c->s_outlier_ws, c->s_outlier_ws_cap, d_out, d_out_points,
                                       reinterpret_cast<long long*>(d_stats), c->stream));
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
        ranges_overlap(d_n_points, 4, d_stats, kStatsBytes))
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
    if (int rc = stage_payload(c, payload, bytes, bytes)) return rc;
    pcs_stat_outlier_stats* d_block = nullptr;
    if (int rc = run_device(c, c->s_voxel_in, n_points, nullptr, *params, c->s_voxel_out, c->d_counts, nullptr, stats ? &d_block : nullptr))
        return rc;
    int32_t kept = 0;
    pcs_stat_outlier_stats got{};
    if (d_block) HIPCHK(c, hipMemcpyAsync(&got, d_block, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    if (int rc = fetch_count(c, "pcs_stat_outlier", n_points, "kept", &kept)) return rc;
    if (kept) HIPCHK(c, hipMemcpy(out, c->s_voxel_out, (size_t)kept * PCS_POINT_BYTES, hipMemcpyDeviceToHost));
    *out_points = kept;
    if (stats) *stats = got;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_stat_outlier: host allocation failed (%s)", ex.what());
}

}  // extern "C"
