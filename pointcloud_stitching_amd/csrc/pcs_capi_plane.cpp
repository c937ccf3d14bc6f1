// pcs_capi_plane.cpp — plane segmentation's part of the C ABI (include/pcs_hip.h, "RANSAC plane segmentation"): the argument checks,
// the workspace and the launches of pcs_kernels_plane.hip (the definition: DESIGN.md section 3; the kernels: section 5). The calls
// read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter: they move or label records, like
// pcs_radius_outlier_device. pcs_plane_from_points runs pcs_plane_math.h on the host: no context, no device.

#include <exception>
#include <vector>

#include "pcs_host.h"
#include "pcs_plane_math.h"

using namespace pcs_host;

namespace {

constexpr size_t kStatsBytes = sizeof(pcs_plane_stats);
constexpr size_t kModelBytes = sizeof(pcs_plane_model);
static_assert(kStatsBytes == 64, "the statistics block is eight int64");
static_assert(kModelBytes == 64, "a model block is six int64 and four int32");
static_assert(sizeof(pcs_plane_params) == 8 * sizeof(int32_t), "pcs_plane_params is eight 32-bit words, no padding");
static_assert(PCS_PLANE_ITERATIONS_MAX == kPlaneMaxHypotheses && PCS_PLANE_MAX_PLANES == kPlaneMaxPlanes, "the kernels' arrays");

constexpr long long kNormalMax = 1ll << 34, kOffsetMax = 1ll << 52;       // a caller's own plane (pcs_plane_count_inliers_device)

int check_params(pcs_ctx* c, const char* who, const pcs_plane_params* p)
{
    if (!p) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (p->distance_mm < PCS_PLANE_DISTANCE_MIN || p->distance_mm > PCS_PLANE_DISTANCE_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->distance_mm %d is outside %d..%d", who, p->distance_mm, PCS_PLANE_DISTANCE_MIN,
                    PCS_PLANE_DISTANCE_MAX);
    if (p->iterations < 1 || p->iterations > PCS_PLANE_ITERATIONS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->iterations %d is outside 1..%d", who, p->iterations, PCS_PLANE_ITERATIONS_MAX);
    if (p->min_inliers < 3) return fail(c, PCS_ERR_INVALID_ARG, "%s: params->min_inliers %d is below 3", who, p->min_inliers);
    if (p->max_planes < 1 || p->max_planes > PCS_PLANE_MAX_PLANES)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->max_planes %d is outside 1..%d", who, p->max_planes, PCS_PLANE_MAX_PLANES);
    if (p->mode != PCS_PLANE_MODE_REMOVE && p->mode != PCS_PLANE_MODE_KEEP)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->mode %d is neither 0 (remove the planes) nor 1 (keep them)", who, p->mode);
    if (p->reserved[0] != 0 || p->reserved[1] != 0)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->reserved %d, %d is not 0", who, p->reserved[0], p->reserved[1]);
    return PCS_OK;
}

// The optional model blocks: alignment, and no byte shared with the payloads, the count or the statistics block.
int check_models(pcs_ctx* c, const char* who, const void* models, const char* models_name, int max_planes, const NamedRange* others,
                 size_t n_others)
{
    if ((uintptr_t)models & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, models_name);
    const NamedRange out[] = {{models, (size_t)max_planes * kModelBytes, models_name}};
    const NamedRange* with = nullptr;
    if (first_overlap(out, 1, others, n_others, &with))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps another argument's range", who, models_name);
    return PCS_OK;
}

// What every filter form checks: the parameters, check_payload_io with the statistics block, the model blocks.
int check_filter(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const char* n_name,
                 const pcs_plane_params* params, const void* out, const char* out_name, size_t out_shorts, const void* out_points,
                 const char* points_name, unsigned points_align, const void* models, const char* models_name, const void* stats,
                 const char* stats_name)
{
    if (int rc = check_params(c, who, params)) return rc;
    if (int rc = check_payload_io(c, who, in, in_name, n_points, n_name, out, out_name, out_shorts, out_points, points_name, points_align,
                                  stats, stats_name, kStatsBytes))
        return rc;
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    const NamedRange others[] = {{in, bytes, in_name}, {out, bytes, out_name}, {out_points, 4, points_name}, {stats, kStatsBytes, stats_name}};
    return check_models(c, who, models, models_name, params->max_planes, others, 4);
}

// What both labels forms check.
int check_labels(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const pcs_plane_params* params,
                 const void* labels, const char* labels_name, const void* planes, const char* planes_name, unsigned planes_align,
                 const void* models, const char* models_name, const void* stats, const char* stats_name)
{
    if (int rc = check_params(c, who, params)) return rc;
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: n_points %d is outside 0..%d", who, n_points, kMaxPoints);
    if (!planes) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, planes_name);
    if (n_points && !in) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, in_name);
    if (n_points && !labels) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, labels_name);
    if ((uintptr_t)in & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, in_name);
    if ((uintptr_t)labels & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, labels_name);
    if ((uintptr_t)planes & (planes_align - 1u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not %u-byte aligned", who, planes_name, planes_align);
    if ((uintptr_t)stats & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, stats_name);
    const NamedRange ins[] = {{in, (size_t)n_points * PCS_POINT_BYTES, in_name}};
    const NamedRange outs[] = {{labels, (size_t)n_points * sizeof(int32_t), labels_name}, {planes, sizeof(int32_t), planes_name},
                               {stats, kStatsBytes, stats_name}};
    const NamedRange* with = nullptr;
    if (const NamedRange* bad = first_overlap(outs, 3, ins, 1, &with))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, bad->name, with ? with->name : in_name);
    const NamedRange others[] = {ins[0], outs[0], outs[1], outs[2]};
    return check_models(c, who, models, models_name, params->max_planes, others, 4);
}

// The launches of one call, behind the checks: one bracket per launch, in launch order. A job with d_out_points is the filter form.
int run(pcs_ctx* c, PlaneJob job)
{
    const size_t need = plane_workspace_bytes(job.capacity);
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, need)) return rc;      // the radius filter's slab, asked for more
    job.d_ws = c->s_outlier_ws;
    job.ws_bytes = c->s_outlier_ws_cap;
    PCS_TIMED(c, launch_plane_step(job, kPlaneInit, 0, c->stream));
    for (int r = 0; r < job.max_planes; r++) {
        for (int step = kPlaneHypotheses; step <= kPlaneMark; step++) PCS_TIMED(c, launch_plane_step(job, step, r, c->stream));
        if (r + 1 == job.max_planes) break;                  // nobody reads a cloud behind the last round
        for (int step = kPlaneTileCount; step <= kPlaneOrigins; step++) PCS_TIMED(c, launch_plane_step(job, step, r, c->stream));
    }
    PCS_TIMED(c, launch_plane_step(job, kPlaneFinish, 0, c->stream));
    if (job.d_out_points)
        for (int step = kPlaneOutCount; step <= kPlaneOutEmit; step++) PCS_TIMED(c, launch_plane_step(job, step, 0, c->stream));
    return PCS_OK;
}

PlaneJob make_job(const int16_t* d_in, int n_points, const int32_t* d_n_points, int capacity, const pcs_plane_params& P)
{
    PlaneJob job{};
    job.d_in = d_in;
    job.n_points = (uint32_t)n_points;
    job.d_n_points = d_n_points;
    job.capacity = (uint32_t)capacity;
    job.distance_mm = P.distance_mm; job.iterations = P.iterations; job.min_inliers = P.min_inliers; job.max_planes = P.max_planes;
    job.seed = P.seed;
    job.mode = P.mode;
    return job;
}

// capacity 0: nothing to launch — zero counts, zeroed blocks
int run_empty(pcs_ctx* c, int max_planes, int32_t* d_count, void* d_models, void* d_stats)
{
    HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(int32_t), c->stream));
    if (d_models) HIPCHK(c, hipMemsetAsync(d_models, 0, (size_t)max_planes * kModelBytes, c->stream));
    if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, kStatsBytes, c->stream));
    return PCS_OK;
}

int run_filter(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const pcs_plane_params& P, int16_t* d_out,
               int32_t* d_out_points, pcs_plane_model* d_models, pcs_plane_stats* d_stats)
{
    DeviceGuard guard(c->device);
    if (capacity == 0) return run_empty(c, P.max_planes, d_out_points, d_models, d_stats);
    PlaneJob job = make_job(d_payload, d_n_points ? 0 : capacity, d_n_points, capacity, P);
    job.d_out = d_out;
    job.d_out_points = d_out_points;
    job.d_models = d_models;
    job.d_stats = reinterpret_cast<long long*>(d_stats);
    return run(c, job);
}

int run_labels(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_plane_params& P, int32_t* d_labels, int32_t* d_n_planes,
               pcs_plane_model* d_models, pcs_plane_stats* d_stats)
{
    DeviceGuard guard(c->device);
    if (n_points == 0) return run_empty(c, P.max_planes, d_n_planes, d_models, d_stats);
    PlaneJob job = make_job(d_payload, n_points, nullptr, n_points, P);
    job.d_labels = d_labels;
    job.d_n_planes = d_n_planes;
    job.d_models = d_models;
    job.d_stats = reinterpret_cast<long long*>(d_stats);
    return run(c, job);
}

// A host form's models, statistics and n_planes on the device: the workspace's staging, once it is large enough for the call.
struct Staging {
    pcs_plane_model* models;
    pcs_plane_stats* stats;
    int32_t*         n_planes;
};
int staging(pcs_ctx* c, int n_points, Staging* s)
{
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, plane_workspace_bytes((uint32_t)n_points))) return rc;
    uint8_t* base = static_cast<uint8_t*>(plane_host_staging((uint32_t)n_points, c->s_outlier_ws));
    *s = Staging{reinterpret_cast<pcs_plane_model*>(base), reinterpret_cast<pcs_plane_stats*>(base + 512), reinterpret_cast<int32_t*>(base + 576)};
    return PCS_OK;
}

}  // namespace

extern "C" {

int pcs_plane_segment_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_plane_params* params, int16_t* d_out,
                             size_t out_shorts, int32_t* d_out_points, pcs_plane_model* d_models, pcs_plane_stats* d_stats)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_filter(c, "pcs_plane_segment_device", d_payload, "d_payload", n_points, "n_points", params, d_out, "d_out", out_shorts,
                              d_out_points, "d_out_points", 4, d_models, "d_models", d_stats, "d_stats"))
        return rc;
    return run_filter(c, d_payload, n_points, nullptr, *params, d_out, d_out_points, d_models, d_stats);
}

int pcs_plane_segment_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                     const pcs_plane_params* params, int16_t* d_out, size_t out_shorts, int32_t* d_out_points,
                                     pcs_plane_model* d_models, pcs_plane_stats* d_stats)
{
    static const char who[] = "pcs_plane_segment_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_filter(c, who, d_payload, "d_payload", max_points, "max_points", params, d_out, "d_out", out_shorts, d_out_points,
                              "d_out_points", 4, d_models, "d_models", d_stats, "d_stats"))
        return rc;
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if ((uintptr_t)d_n_points & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    if (ranges_overlap(d_n_points, 4, d_out, (size_t)max_points * PCS_POINT_BYTES) || ranges_overlap(d_n_points, 4, d_out_points, 4) ||
        ranges_overlap(d_n_points, 4, d_stats, kStatsBytes) || ranges_overlap(d_n_points, 4, d_models, (size_t)params->max_planes * kModelBytes))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points overlaps d_out, d_out_points, d_models or d_stats", who);
    return run_filter(c, d_payload, max_points, d_n_points, *params, d_out, d_out_points, d_models, d_stats);
}

int pcs_plane_segment(pcs_ctx* c, const int16_t* payload, int n_points, const pcs_plane_params* params, int16_t* out, size_t out_shorts,
                      int* out_points, pcs_plane_model* models, pcs_plane_stats* stats)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_filter(c, "pcs_plane_segment", payload, "payload", n_points, "n_points", params, out, "out", out_shorts, out_points,
                              "out_points", (unsigned)alignof(int), models, "models", stats, "stats"))
        return rc;
    if (n_points == 0) {
        *out_points = 0;
        if (models) std::fill(models, models + params->max_planes, pcs_plane_model{});
        if (stats) *stats = pcs_plane_stats{};
        return PCS_OK;
    }
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    if (int rc = stage_payload(c, payload, bytes, bytes)) return rc;
    Staging s{};
    if (int rc = staging(c, n_points, &s)) return rc;
    if (int rc = run_filter(c, c->s_voxel_in, n_points, nullptr, *params, c->s_voxel_out, c->d_counts, s.models, s.stats)) return rc;
    pcs_plane_model got_models[PCS_PLANE_MAX_PLANES] = {};
    pcs_plane_stats got{};
    HIPCHK(c, hipMemcpyAsync(got_models, s.models, (size_t)params->max_planes * kModelBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&got, s.stats, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    int32_t kept = 0;
    if (int rc = fetch_count(c, "pcs_plane_segment", n_points, "kept", &kept)) return rc;
    if (kept) HIPCHK(c, hipMemcpy(out, c->s_voxel_out, (size_t)kept * PCS_POINT_BYTES, hipMemcpyDeviceToHost));
    *out_points = kept;
    if (models) std::copy(got_models, got_models + params->max_planes, models);
    if (stats) *stats = got;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_plane_segment: host allocation failed (%s)", ex.what());
}

int pcs_plane_labels_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_plane_params* params, int32_t* d_labels,
                            int32_t* d_n_planes, pcs_plane_model* d_models, pcs_plane_stats* d_stats)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_labels(c, "pcs_plane_labels_device", d_payload, "d_payload", n_points, params, d_labels, "d_labels", d_n_planes,
                              "d_n_planes", 4, d_models, "d_models", d_stats, "d_stats"))
        return rc;
    return run_labels(c, d_payload, n_points, *params, d_labels, d_n_planes, d_models, d_stats);
}

int pcs_plane_labels(pcs_ctx* c, const int16_t* payload, int n_points, const pcs_plane_params* params, int32_t* labels, int* n_planes,
                     pcs_plane_model* models, pcs_plane_stats* stats)
try {
    static const char who[] = "pcs_plane_labels";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_labels(c, who, payload, "payload", n_points, params, labels, "labels", n_planes, "n_planes", (unsigned)alignof(int),
                              models, "models", stats, "stats"))
        return rc;
    if (n_points == 0) {
        *n_planes = 0;
        if (models) std::fill(models, models + params->max_planes, pcs_plane_model{});
        if (stats) *stats = pcs_plane_stats{};
        return PCS_OK;
    }
    DeviceGuard guard(c->device);
    const size_t words = (size_t)n_points * sizeof(int32_t);      // the labels in the staged output (4-byte aligned: the slab is 256-byte aligned)
    if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, words)) return rc;
    Staging s{};
    if (int rc = staging(c, n_points, &s)) return rc;
    int32_t* const d_labels = reinterpret_cast<int32_t*>(c->s_voxel_out);
    if (int rc = run_labels(c, c->s_voxel_in, n_points, *params, d_labels, s.n_planes, s.models, s.stats)) return rc;
    pcs_plane_model got_models[PCS_PLANE_MAX_PLANES] = {};
    pcs_plane_stats got{};
    int32_t count = -1;
    HIPCHK(c, hipMemcpyAsync(got_models, s.models, (size_t)params->max_planes * kModelBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&got, s.stats, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    if (int rc = fetch(c, &count, s.n_planes, sizeof count)) return rc;
    if (count < 0 || count > params->max_planes)
        return fail(c, PCS_ERR_HIP, "%s: the kernels reported %d planes of at most %d", who, count, params->max_planes);
    HIPCHK(c, hipMemcpy(labels, d_labels, words, hipMemcpyDeviceToHost));
    *n_planes = count;
    if (models) std::copy(got_models, got_models + params->max_planes, models);
    if (stats) *stats = got;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_plane_labels: host allocation failed (%s)", ex.what());
}

int pcs_plane_count_inliers_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_plane_model* models, int n_models,
                                   int64_t* d_counts)
try {
    static const char who[] = "pcs_plane_count_inliers_device";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: n_points %d is outside 0..%d", who, n_points, kMaxPoints);
    if (n_models < 1 || n_models > PCS_PLANE_ITERATIONS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: n_models %d is outside 1..%d", who, n_models, PCS_PLANE_ITERATIONS_MAX);
    if (!models) return fail(c, PCS_ERR_INVALID_ARG, "%s: models is NULL", who);
    if (!d_counts) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_counts is NULL", who);
    if (n_points && !d_payload) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_payload is NULL", who);
    if ((uintptr_t)d_payload & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_payload is not 2-byte aligned", who);
    if ((uintptr_t)d_counts & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_counts is not 8-byte aligned", who);
    if (ranges_overlap(d_counts, (size_t)n_models * sizeof(int64_t), d_payload, (size_t)n_points * PCS_POINT_BYTES))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: d_counts overlaps d_payload", who);
    std::vector<long long> eqs((size_t)n_models * 5);
    for (int j = 0; j < n_models; j++) {
        const pcs_plane_model& m = models[j];
        const int64_t n3[3] = {m.nx, m.ny, m.nz};
        static const char* const names[3] = {"nx", "ny", "nz"};
        for (int k = 0; k < 3; k++)
            if (n3[k] < -kNormalMax || n3[k] > kNormalMax)
                return fail(c, PCS_ERR_INVALID_ARG, "%s: models[%d].%s %lld is outside -2^34..2^34", who, j, names[k], (long long)n3[k]);
        if (m.off < -kOffsetMax || m.off > kOffsetMax)
            return fail(c, PCS_ERR_INVALID_ARG, "%s: models[%d].off %lld is outside -2^52..2^52", who, j, (long long)m.off);
        if (m.threshold < 0 || m.threshold > kOffsetMax)
            return fail(c, PCS_ERR_INVALID_ARG, "%s: models[%d].threshold %lld is outside 0..2^52", who, j, (long long)m.threshold);
        if (m.nx == 0 && m.ny == 0 && m.nz == 0) return fail(c, PCS_ERR_INVALID_ARG, "%s: models[%d] has a zero normal", who, j);
        long long* w = &eqs[(size_t)j * 5];
        w[0] = m.nx; w[1] = m.ny; w[2] = m.nz; w[3] = m.off; w[4] = m.threshold;
    }
    DeviceGuard guard(c->device);
    HIPCHK(c, hipMemsetAsync(d_counts, 0, (size_t)n_models * sizeof(int64_t), c->stream));
    if (n_points == 0) return PCS_OK;
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, plane_count_workspace_bytes())) return rc;
    // the planes leave the host before the call returns: the copy is waited for, the scoring is not
    HIPCHK(c, hipMemcpyAsync(plane_count_planes(c->s_outlier_ws), eqs.data(), eqs.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    PCS_TIMED(c, launch_plane_count(d_payload, (uint32_t)n_points, c->s_outlier_ws, c->s_outlier_ws_cap, (uint32_t)n_models,
                                    reinterpret_cast<unsigned long long*>(d_counts), c->stream));
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_plane_count_inliers_device: host allocation failed (%s)", ex.what());
}

int pcs_plane_from_points(const int16_t* p0, const int16_t* p1, const int16_t* p2, int distance_mm, pcs_plane_model* model)
{
    if (!p0 || !p1 || !p2 || !model || distance_mm < PCS_PLANE_DISTANCE_MIN || distance_mm > PCS_PLANE_DISTANCE_MAX) return PCS_ERR_INVALID_ARG;
    PlaneEq e{};
    const bool ok = plane_from_records(p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2], distance_mm, e);
    *model = pcs_plane_model{};
    if (!ok) return PCS_ERR_INVALID_ARG;
    model->nx = e.nx; model->ny = e.ny; model->nz = e.nz; model->off = e.off; model->threshold = e.t;
    model->sample[1] = 1;
    model->sample[2] = 2;
    return PCS_OK;
}

}  // extern "C"
