// pcs_capi_cluster.cpp — Euclidean cluster extraction's part of the C ABI (include/pcs_hip.h, "Euclidean cluster extraction"): the
// argument checks, the workspace and the launches of pcs_kernels_cluster.hip (the definition: DESIGN.md section 3; the kernels:
// section 5). The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter: they move
// or label records, like pcs_radius_outlier_device.

#include <exception>

#include "pcs_host.h"

using namespace pcs_host;

namespace {

constexpr size_t kStatsBytes = sizeof(pcs_cluster_stats);
static_assert(kStatsBytes == 64, "the statistics block is eight int64");
static_assert(sizeof(pcs_cluster_params) == 4 * sizeof(int32_t), "pcs_cluster_params is four int32 words, no padding");

int check_tolerance(pcs_ctx* c, const char* who, const char* name, int tolerance_mm)
{
    if (tolerance_mm < PCS_CLUSTER_TOLERANCE_MIN || tolerance_mm > PCS_CLUSTER_TOLERANCE_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside %d..%d", who, name, tolerance_mm, PCS_CLUSTER_TOLERANCE_MIN,
                    PCS_CLUSTER_TOLERANCE_MAX);
    return PCS_OK;
}

// What every filter form checks first: the filter's own parameters, then check_payload_io with the statistics block (stats may be
// NULL); `who` names the entry point, the *_name its own argument names.
int check_args(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const char* n_name,
               const pcs_cluster_params* params, const void* out, const char* out_name, size_t out_shorts, const void* out_points,
               const char* points_name, unsigned points_align, const void* stats, const char* stats_name)
{
    if (!params) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (int rc = check_tolerance(c, who, "params->tolerance_mm", params->tolerance_mm)) return rc;
    if (params->min_size < 1) return fail(c, PCS_ERR_INVALID_ARG, "%s: params->min_size %d is below 1", who, params->min_size);
    if (params->max_size < 0 || (params->max_size && params->max_size < params->min_size))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->max_size %d is neither 0 nor at least min_size %d", who, params->max_size,
                    params->min_size);
    if (params->reserved != 0) return fail(c, PCS_ERR_INVALID_ARG, "%s: params->reserved %d is not 0", who, params->reserved);
    return check_payload_io(c, who, in, in_name, n_points, n_name, out, out_name, out_shorts, out_points, points_name, points_align, stats,
                            stats_name, kStatsBytes);
}

// The filter's launches, behind the checks. capacity: n_points, or the counted form's max_points. d_stats NULL: no block, one launch
// fewer. stage_stats: the host form's — the block goes to the first 64 bytes of the workspace's last 256, *d_staged says where.
int run_filter(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const pcs_cluster_params& P, int16_t* d_out,
               int32_t* d_out_points, pcs_cluster_stats* d_stats, pcs_cluster_stats** d_staged = nullptr)
{
    DeviceGuard guard(c->device);
    if (capacity == 0) {         // nothing to launch: a zero count, a zeroed block
        HIPCHK(c, hipMemsetAsync(d_out_points, 0, sizeof(int32_t), c->stream));
        if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, kStatsBytes, c->stream));
        return PCS_OK;
    }
    const size_t need = cluster_workspace_bytes((uint32_t)capacity);
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, need)) return rc;      // the radius filter's slab, asked for more
    if (d_staged) *d_staged = d_stats = reinterpret_cast<pcs_cluster_stats*>(static_cast<uint8_t*>(c->s_outlier_ws) + need - 256);
    // one bracket per launch: pcs_kernel_times_ms hands back one interval per launch, in launch order
    for (int stage = 0; stage < kClusterStages - (d_stats ? 0 : 1); stage++)
        PCS_TIMED(c, launch_cluster_stage(stage, d_payload, (uint32_t)capacity, d_n_points, (uint32_t)capacity, P.tolerance_mm, P.min_size,
                                          P.max_size, c->s_outlier_ws, c->s_outlier_ws_cap, d_out, d_out_points,
                                          reinterpret_cast<long long*>(d_stats), nullptr, nullptr, nullptr, c->stream));
    return PCS_OK;
}

// What both labels forms check; labels / sizes / clusters are the caller's names for them.
int check_labels(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, int tolerance_mm, const void* labels,
                 const char* labels_name, const void* sizes, const char* sizes_name, const void* clusters, const char* clusters_name,
                 unsigned clusters_align)
{
    if (int rc = check_tolerance(c, who, "tolerance_mm", tolerance_mm)) return rc;
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: n_points %d is outside 0..%d", who, n_points, kMaxPoints);
    if (!clusters) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, clusters_name);
    if (n_points && !in) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, in_name);
    if (n_points && !labels) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, labels_name);
    if ((uintptr_t)in & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, in_name);
    if ((uintptr_t)labels & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, labels_name);
    if ((uintptr_t)sizes & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, sizes_name);
    if ((uintptr_t)clusters & (clusters_align - 1u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not %u-byte aligned", who, clusters_name, clusters_align);
    const NamedRange ins[] = {{in, (size_t)n_points * PCS_POINT_BYTES, in_name}};
    const NamedRange outs[] = {{labels, (size_t)n_points * sizeof(int32_t), labels_name}, {sizes, (size_t)n_points * sizeof(int32_t), sizes_name},
                               {clusters, sizeof(int32_t), clusters_name}};
    const NamedRange* with = nullptr;
    if (const NamedRange* bad = first_overlap(outs, 3, ins, 1, &with))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, bad->name, with ? with->name : in_name);
    return PCS_OK;
}

int run_labels(pcs_ctx* c, const int16_t* d_payload, int n_points, int tolerance_mm, int32_t* d_labels, int32_t* d_sizes, int32_t* d_n_clusters)
{
    DeviceGuard guard(c->device);
    if (n_points == 0) {
        HIPCHK(c, hipMemsetAsync(d_n_clusters, 0, sizeof(int32_t), c->stream));
        return PCS_OK;
    }
    const size_t need = cluster_workspace_bytes((uint32_t)n_points);
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, need)) return rc;
    for (int k = 0; k < kClusterLabelStages; k++)
        PCS_TIMED(c, launch_cluster_stage(cluster_label_stage(k), d_payload, (uint32_t)n_points, nullptr, (uint32_t)n_points, tolerance_mm, 1, 0,
                                          c->s_outlier_ws, c->s_outlier_ws_cap, nullptr, nullptr, nullptr, d_labels, d_sizes, d_n_clusters,
                                          c->stream));
    return PCS_OK;
}

}  // namespace

extern "C" {

int pcs_cluster_filter_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_cluster_params* params, int16_t* d_out,
                              size_t out_shorts, int32_t* d_out_points, pcs_cluster_stats* d_stats)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, "pcs_cluster_filter_device", d_payload, "d_payload", n_points, "n_points", params, d_out, "d_out", out_shorts,
                            d_out_points, "d_out_points", 4, d_stats, "d_stats"))
        return rc;
    return run_filter(c, d_payload, n_points, nullptr, *params, d_out, d_out_points, d_stats);
}

int pcs_cluster_filter_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                      const pcs_cluster_params* params, int16_t* d_out, size_t out_shorts, int32_t* d_out_points,
                                      pcs_cluster_stats* d_stats)
{
    static const char who[] = "pcs_cluster_filter_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, who, d_payload, "d_payload", max_points, "max_points", params, d_out, "d_out", out_shorts, d_out_points,
                            "d_out_points", 4, d_stats, "d_stats"))
        return rc;
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if ((uintptr_t)d_n_points & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    if (ranges_overlap(d_n_points, 4, d_out, (size_t)max_points * PCS_POINT_BYTES) || ranges_overlap(d_n_points, 4, d_out_points, 4) ||
        ranges_overlap(d_n_points, 4, d_stats, kStatsBytes))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points overlaps d_out, d_out_points or d_stats", who);
    return run_filter(c, d_payload, max_points, d_n_points, *params, d_out, d_out_points, d_stats);
}

int pcs_cluster_filter(pcs_ctx* c, const int16_t* payload, int n_points, const pcs_cluster_params* params, int16_t* out, size_t out_shorts,
                       int* out_points, pcs_cluster_stats* stats)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, "pcs_cluster_filter", payload, "payload", n_points, "n_points", params, out, "out", out_shorts, out_points,
                            "out_points", (unsigned)alignof(int), stats, "stats"))
        return rc;
    if (n_points == 0) {
        *out_points = 0;
        if (stats) *stats = pcs_cluster_stats{};
        return PCS_OK;
    }
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    if (int rc = stage_payload(c, payload, bytes, bytes)) return rc;
    pcs_cluster_stats* d_block = nullptr;
    if (int rc = run_filter(c, c->s_voxel_in, n_points, nullptr, *params, c->s_voxel_out, c->d_counts, nullptr, stats ? &d_block : nullptr))
        return rc;
    int32_t kept = 0;
    pcs_cluster_stats got{};
    if (d_block) HIPCHK(c, hipMemcpyAsync(&got, d_block, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    if (int rc = fetch_count(c, "pcs_cluster_filter", n_points, "kept", &kept)) return rc;
    if (kept) HIPCHK(c, hipMemcpy(out, c->s_voxel_out, (size_t)kept * PCS_POINT_BYTES, hipMemcpyDeviceToHost));
    *out_points = kept;
    if (stats) *stats = got;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_cluster_filter: host allocation failed (%s)", ex.what());
}

int pcs_cluster_labels_device(pcs_ctx* c, const int16_t* d_payload, int n_points, int tolerance_mm, int32_t* d_labels, int32_t* d_sizes,
                              int32_t* d_n_clusters)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_labels(c, "pcs_cluster_labels_device", d_payload, "d_payload", n_points, tolerance_mm, d_labels, "d_labels", d_sizes,
                              "d_sizes", d_n_clusters, "d_n_clusters", 4))
        return rc;
    return run_labels(c, d_payload, n_points, tolerance_mm, d_labels, d_sizes, d_n_clusters);
}

int pcs_cluster_labels(pcs_ctx* c, const int16_t* payload, int n_points, int tolerance_mm, int32_t* labels, int32_t* sizes, int* n_clusters)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_labels(c, "pcs_cluster_labels", payload, "payload", n_points, tolerance_mm, labels, "labels", sizes, "sizes", n_clusters,
                              "n_clusters", (unsigned)alignof(int)))
        return rc;
    if (n_points == 0) { *n_clusters = 0; return PCS_OK; }
    DeviceGuard guard(c->device);
    // labels, then sizes, in the staged output: 8 bytes per record (4-byte aligned: the slab is 256-byte aligned)
    const size_t words = (size_t)n_points * sizeof(int32_t);
    if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, 2 * words)) return rc;
    int32_t* const d_labels = reinterpret_cast<int32_t*>(c->s_voxel_out);
    int32_t* const d_sizes = sizes ? d_labels + n_points : nullptr;
    if (int rc = run_labels(c, c->s_voxel_in, n_points, tolerance_mm, d_labels, d_sizes, c->d_counts)) return rc;
    int32_t count = 0;
    if (int rc = fetch_count(c, "pcs_cluster_labels", n_points, "their cluster's first", &count)) return rc;
    HIPCHK(c, hipMemcpy(labels, d_labels, words, hipMemcpyDeviceToHost));
    if (sizes) HIPCHK(c, hipMemcpy(sizes, d_sizes, words, hipMemcpyDeviceToHost));
    *n_clusters = count;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_cluster_labels: host allocation failed (%s)", ex.what());
}

}  // extern "C"
