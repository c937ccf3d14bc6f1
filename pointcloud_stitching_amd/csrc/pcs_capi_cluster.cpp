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

// ---- the object table ---------------------------------------------------------------------------------------------------------------
static_assert(sizeof(pcs_cluster_object) == 80 && alignof(pcs_cluster_object) == 8, "pcs_cluster_object is 80 bytes, 8-byte aligned");

// What both device forms of the objects call check: the filter's checks over the filtered payload where one is asked for (without
// one, the filter's checks of the parameters, the count and the input), then the table's own arguments and every overlap.
// n_points is the counted form's max_points; count / count_name its count word (an input: nothing may be written over it).
int check_objects(pcs_ctx* c, const char* who, const void* in, int n_points, const char* n_name, const pcs_cluster_params* params,
                  const pcs_cluster_objects_out* out, const void* count = nullptr, const char* count_name = nullptr)
{
    if (!out) return fail(c, PCS_ERR_INVALID_ARG, "%s: out is NULL", who);
    if ((out->out != nullptr) != (out->out_points != nullptr))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: out->out and out->out_points go together: %s is NULL", who, out->out ? "out->out_points" : "out->out");
    if (out->out) {
        if (int rc = check_args(c, who, in, "d_payload", n_points, n_name, params, out->out, "out->out", out->out_shorts, out->out_points,
                                "out->out_points", 4, out->stats, "out->stats"))
            return rc;
    } else {
        // the same checks with the count word standing in for the filter's: no payload output, so no worst case to hold
        if (int rc = check_args(c, who, in, "d_payload", 0, n_name, params, nullptr, "out->out", 0, out->n_objects, "out->n_objects", 4,
                                out->stats, "out->stats"))
            return rc;
        if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside 0..%d", who, n_name, n_points, kMaxPoints);
        if (n_points && !in) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_payload is NULL", who);
    }
    if (out->max_objects < 0 || out->max_objects > PCS_CLUSTER_OBJECTS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: out->max_objects %d is outside 0..%d", who, out->max_objects, PCS_CLUSTER_OBJECTS_MAX);
    if (out->max_objects && !out->objects) return fail(c, PCS_ERR_INVALID_ARG, "%s: out->objects is NULL with out->max_objects %d", who, out->max_objects);
    if ((uintptr_t)out->objects & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: out->objects is not 8-byte aligned", who);
    if (out->reserved != 0) return fail(c, PCS_ERR_INVALID_ARG, "%s: out->reserved %d is not 0", who, out->reserved);
    if (!out->n_objects) return fail(c, PCS_ERR_INVALID_ARG, "%s: out->n_objects is NULL", who);
    if ((uintptr_t)out->n_objects & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: out->n_objects is not 4-byte aligned", who);
    if ((uintptr_t)out->object_of & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: out->object_of is not 4-byte aligned", who);
    if (count_name) {
        if (!count) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, count_name);
        if ((uintptr_t)count & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, count_name);
    }
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    const NamedRange ins[] = {{in, bytes, "d_payload"}, {count, sizeof(int32_t), count_name}};
    const NamedRange outs[] = {{out->objects, (size_t)out->max_objects * sizeof(pcs_cluster_object), "out->objects"},
                               {out->n_objects, sizeof(int32_t), "out->n_objects"},
                               {out->object_of, (size_t)n_points * sizeof(int32_t), "out->object_of"},
                               {out->out, bytes, "out->out"},
                               {out->out_points, sizeof(int32_t), "out->out_points"},
                               {out->stats, kStatsBytes, "out->stats"}};
    const NamedRange* with = nullptr;
    if (const NamedRange* bad = first_overlap(outs, 6, ins, 2, &with)) {
        if (!with) with = ranges_overlap(bad->p, bad->n, ins[0].p, ins[0].n) ? &ins[0] : &ins[1];
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, bad->name, with->name);
    }
    return PCS_OK;
}

// The objects call's launches, behind the checks. capacity: n_points, or the counted form's max_points.
int run_objects(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const pcs_cluster_params& P,
                const pcs_cluster_objects_out& O)
{
    DeviceGuard guard(c->device);
    if (capacity == 0) {         // nothing to launch: no objects, a zero count, a zeroed block
        HIPCHK(c, hipMemsetAsync(O.n_objects, 0, sizeof(int32_t), c->stream));
        if (O.out_points) HIPCHK(c, hipMemsetAsync(O.out_points, 0, sizeof(int32_t), c->stream));
        if (O.stats) HIPCHK(c, hipMemsetAsync(O.stats, 0, kStatsBytes, c->stream));
        return PCS_OK;
    }
    const uint32_t cap = (uint32_t)capacity, max_objects = (uint32_t)O.max_objects;
    const size_t need = cluster_objects_workspace_bytes(cap, max_objects);
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, need)) return rc;
    // the filter's stages: 0 to 8 always; flag, tile count and tile scan where somebody reads the kept count; emit with `out`; stats
    int32_t* const d_kept = O.out_points ? O.out_points : cluster_objects_scratch_word(cap, max_objects, c->s_outlier_ws);
    const int filter_end = O.out ? 13 : O.stats ? 12 : 9;
    for (int stage = 0; stage < kClusterStages; stage++) {
        if (stage >= filter_end && !(stage == 13 && O.stats)) continue;
        PCS_TIMED(c, launch_cluster_stage(stage, d_payload, cap, d_n_points, cap, P.tolerance_mm, P.min_size, P.max_size, c->s_outlier_ws,
                                          c->s_outlier_ws_cap, O.out, d_kept, reinterpret_cast<long long*>(O.stats), nullptr, nullptr, nullptr,
                                          c->stream));
    }
    for (int k = 0; k < kClusterObjectStages; k++)
        PCS_TIMED(c, launch_cluster_object_stage(kClusterObjectStage0 + k, d_payload, cap, P.tolerance_mm, P.min_size, P.max_size, max_objects,
                                                 c->s_outlier_ws, c->s_outlier_ws_cap, O.objects, O.n_objects, O.object_of, c->stream));
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

int pcs_cluster_objects_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_cluster_params* params,
                               const pcs_cluster_objects_out* out)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_objects(c, "pcs_cluster_objects_device", d_payload, n_points, "n_points", params, out)) return rc;
    return run_objects(c, d_payload, n_points, nullptr, *params, *out);
}

int pcs_cluster_objects_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                       const pcs_cluster_params* params, const pcs_cluster_objects_out* out)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_objects(c, "pcs_cluster_objects_device_counted", d_payload, max_points, "max_points", params, out, d_n_points, "d_n_points"))
        return rc;
    return run_objects(c, d_payload, max_points, d_n_points, *params, *out);
}

int pcs_cluster_objects(pcs_ctx* c, const int16_t* payload, int n_points, const pcs_cluster_params* params, pcs_cluster_object* objects,
                        int max_objects, int* n_objects, int32_t* object_of)
try {
    static const char who[] = "pcs_cluster_objects";
    if (!c) return PCS_ERR_INVALID_ARG;
    // the device form's checks over the host ranges (its names for them: the struct's), the count word's alignment the host's
    pcs_cluster_objects_out host{};
    host.objects = objects;
    host.max_objects = max_objects;
    host.n_objects = reinterpret_cast<int32_t*>(n_objects);
    host.object_of = object_of;
    if (int rc = check_objects(c, who, payload, n_points, "n_points", params, &host)) return rc;
    if (n_points == 0) { *n_objects = 0; return PCS_OK; }
    DeviceGuard guard(c->device);
    // the table, then object_of, in the staged output (8-byte aligned: the slab is 256-byte aligned, an entry 80 bytes)
    const size_t table = (size_t)max_objects * sizeof(pcs_cluster_object), words = (size_t)n_points * sizeof(int32_t);
    if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, table + words)) return rc;
    pcs_cluster_objects_out dev{};
    dev.objects = max_objects ? reinterpret_cast<pcs_cluster_object*>(c->s_voxel_out) : nullptr;
    dev.max_objects = max_objects;
    dev.n_objects = c->d_counts;
    dev.object_of = object_of ? reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(c->s_voxel_out) + table) : nullptr;
    if (int rc = run_objects(c, c->s_voxel_in, n_points, nullptr, *params, dev)) return rc;
    int32_t count = 0;
    if (int rc = fetch_count(c, who, n_points, "their object's first", &count)) return rc;
    const size_t written = (size_t)std::min(count, max_objects);
    if (written) HIPCHK(c, hipMemcpy(objects, dev.objects, written * sizeof(pcs_cluster_object), hipMemcpyDeviceToHost));
    if (object_of) HIPCHK(c, hipMemcpy(object_of, dev.object_of, words, hipMemcpyDeviceToHost));
    *n_objects = count;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_cluster_objects: host allocation failed (%s)", ex.what());
}

}  // extern "C"
