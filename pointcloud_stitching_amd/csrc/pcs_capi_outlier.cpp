// pcs_capi_outlier.cpp — radius outlier removal's part of the C ABI (include/pcs_hip.h, "radius outlier removal"): the argument
// checks, the workspace and the launches of pcs_kernels_outlier.hip (the definition: DESIGN.md section 3; the kernels: section 5).
// The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter: they move records, like
// pcs_stitch_device.

#include <exception>

#include "pcs_host.h"

using namespace pcs_host;

namespace {

// What every form checks first: the filter's own parameters, then check_payload_io.
int check_params(pcs_ctx* c, const char* who, int radius_mm, int min_neighbors)
{
    if (radius_mm < PCS_OUTLIER_RADIUS_MIN || radius_mm > PCS_OUTLIER_RADIUS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: radius_mm %d is outside %d..%d", who, radius_mm, PCS_OUTLIER_RADIUS_MIN, PCS_OUTLIER_RADIUS_MAX);
    if (min_neighbors < PCS_OUTLIER_NEIGHBORS_MIN || min_neighbors > PCS_OUTLIER_NEIGHBORS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: min_neighbors %d is outside %d..%d", who, min_neighbors, PCS_OUTLIER_NEIGHBORS_MIN,
                    PCS_OUTLIER_NEIGHBORS_MAX);
    return PCS_OK;
}

// The launches, behind the checks. capacity: n_points, or the counted form's max_points.
int run_device(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, int radius_mm, int min_neighbors,
               int16_t* d_out, int32_t* d_out_points)
{
    DeviceGuard guard(c->device);
    if (capacity == 0) {         // nothing to launch: a zero count
        HIPCHK(c, hipMemsetAsync(d_out_points, 0, sizeof(int32_t), c->stream));
        return PCS_OK;
    }
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, outlier_workspace_bytes((uint32_t)capacity))) return rc;
    // one bracket per launch: pcs_kernel_times_ms hands back kOutlierStages intervals per call, in launch order
    for (int stage = 0; stage < kOutlierStages; stage++)
        PCS_TIMED(c, launch_outlier_stage(stage, d_payload, (uint32_t)capacity, d_n_points, (uint32_t)capacity, radius_mm, min_neighbors,
                                          c->s_outlier_ws, c->s_outlier_ws_cap, d_out, d_out_points, c->stream));
    return PCS_OK;
}

}  // namespace

extern "C" {

int pcs_radius_outlier_device(pcs_ctx* c, const int16_t* d_payload, int n_points, int radius_mm, int min_neighbors, int16_t* d_out,
                              size_t out_shorts, int32_t* d_out_points)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    static const char who[] = "pcs_radius_outlier_device";
    if (int rc = check_params(c, who, radius_mm, min_neighbors)) return rc;
    if (int rc = check_payload_io(c, who, d_payload, "d_payload", n_points, "n_points", d_out, "d_out", out_shorts, d_out_points, "d_out_points", 4))
        return rc;
    return run_device(c, d_payload, n_points, nullptr, radius_mm, min_neighbors, d_out, d_out_points);
}

int pcs_radius_outlier_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points, int radius_mm,
                                      int min_neighbors, int16_t* d_out, size_t out_shorts, int32_t* d_out_points)
{
    static const char who[] = "pcs_radius_outlier_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_params(c, who, radius_mm, min_neighbors)) return rc;
    if (int rc = check_payload_io(c, who, d_payload, "d_payload", max_points, "max_points", d_out, "d_out", out_shorts, d_out_points, "d_out_points", 4))
        return rc;
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if ((uintptr_t)d_n_points & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    if (ranges_overlap(d_n_points, 4, d_out, (size_t)max_points * PCS_POINT_BYTES) || ranges_overlap(d_n_points, 4, d_out_points, 4))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points overlaps d_out or d_out_points", who);
    return run_device(c, d_payload, max_points, d_n_points, radius_mm, min_neighbors, d_out, d_out_points);
}

int pcs_radius_outlier(pcs_ctx* c, const int16_t* payload, int n_points, int radius_mm, int min_neighbors, int16_t* out, size_t out_shorts,
                       int* out_points)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    static const char who[] = "pcs_radius_outlier";
    if (int rc = check_params(c, who, radius_mm, min_neighbors)) return rc;
    if (int rc = check_payload_io(c, who, payload, "payload", n_points, "n_points", out, "out", out_shorts, out_points, "out_points",
                                  (unsigned)alignof(int)))
        return rc;
    if (n_points == 0) { *out_points = 0; return PCS_OK; }
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    if (int rc = stage_payload(c, payload, bytes, bytes)) return rc;
    if (int rc = run_device(c, c->s_voxel_in, n_points, nullptr, radius_mm, min_neighbors, c->s_voxel_out, c->d_counts)) return rc;
    int32_t kept = 0;
    if (int rc = fetch_count(c, who, n_points, "kept", &kept)) return rc;
    if (kept) HIPCHK(c, hipMemcpy(out, c->s_voxel_out, (size_t)kept * PCS_POINT_BYTES, hipMemcpyDeviceToHost));
    *out_points = kept;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_radius_outlier: host allocation failed (%s)", ex.what());
}

}  // extern "C"
