// pcs_capi_outlier.cpp — radius outlier removal's part of the C ABI (include/pcs_hip.h, "radius outlier removal"): the argument
// checks, the workspace and the launches of pcs_kernels_outlier.hip (the definition: DESIGN.md section 3; the kernels: section 5).
// The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter: they move records, like
// pcs_stitch_device.

#include <climits>
#include <exception>

#include "pcs_host.h"

using namespace pcs_host;

namespace {

constexpr int kMaxPoints = INT_MAX / PCS_POINT_BYTES;      // a payload's byte count fits an int32 (as the PCZ1 container's)

// [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// What every form checks first; `who` names the entry point, in / out / out_points its own argument names.
int check_args(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const char* n_name, int radius_mm,
               int min_neighbors, const void* out, const char* out_name, size_t out_shorts, const void* out_points,
               const char* points_name, unsigned points_align)
{
    if (radius_mm < PCS_OUTLIER_RADIUS_MIN || radius_mm > PCS_OUTLIER_RADIUS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: radius_mm %d is outside %d..%d", who, radius_mm, PCS_OUTLIER_RADIUS_MIN, PCS_OUTLIER_RADIUS_MAX);
    if (min_neighbors < PCS_OUTLIER_NEIGHBORS_MIN || min_neighbors > PCS_OUTLIER_NEIGHBORS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: min_neighbors %d is outside %d..%d", who, min_neighbors, PCS_OUTLIER_NEIGHBORS_MIN,
                    PCS_OUTLIER_NEIGHBORS_MAX);
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside 0..%d", who, n_name, n_points, kMaxPoints);
    if (!out_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, points_name);
    if (n_points && !in) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, in_name);
    if (n_points && !out) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, out_name);
    if ((uintptr_t)in & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, in_name);
    if ((uintptr_t)out & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, out_name);
    if ((uintptr_t)out_points & (points_align - 1u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not %u-byte aligned", who, points_name, points_align);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    if (out_shorts < (size_t)n_points * PCS_POINT_SHORTS)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: out_shorts %zu: %s must hold the worst case, every one of %d records kept: %zu shorts", who,
                    out_shorts, out_name, n_points, (size_t)n_points * PCS_POINT_SHORTS);
    if (ranges_overlap(in, bytes, out, bytes)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s and %s overlap", who, in_name, out_name);
    if (ranges_overlap(out_points, 4, out, bytes) || ranges_overlap(out_points, 4, in, bytes))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s or %s", who, points_name, in_name, out_name);
    return PCS_OK;
}

// The outlier workspace of a context, at least `need` bytes: grows with a quarter of headroom, and growing waits for the stream
// (ensure_voxel_ws's policy).
int ensure_outlier_ws(pcs_ctx* c, size_t need)
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

// The launches, behind the checks. capacity: n_points, or the counted form's max_points.
int run_device(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, int radius_mm, int min_neighbors,
               int16_t* d_out, int32_t* d_out_points)
{
    DeviceGuard guard(c->device);
    if (capacity == 0) {         // nothing to launch: a zero count
        HIPCHK(c, hipMemsetAsync(d_out_points, 0, sizeof(int32_t), c->stream));
        return PCS_OK;
    }
    if (int rc = ensure_outlier_ws(c, outlier_workspace_bytes((uint32_t)capacity))) return rc;
    for (int stage = 0; stage < kOutlierStages; stage++) {
        // one bracket per launch: pcs_kernel_times_ms hands back kOutlierStages intervals per call, in launch order
        KernelTimer timer(c);
        if (timer.rc) return timer.rc;
        HIPCHK(c, launch_outlier_stage(stage, d_payload, (uint32_t)capacity, d_n_points, (uint32_t)capacity, radius_mm, min_neighbors,
                                       c->s_outlier_ws, c->s_outlier_ws_cap, d_out, d_out_points, c->stream));
        if (int rc = timer.finish()) return rc;
    }
    return PCS_OK;
}

}  // namespace

extern "C" {

int pcs_radius_outlier_device(pcs_ctx* c, const int16_t* d_payload, int n_points, int radius_mm, int min_neighbors, int16_t* d_out,
                              size_t out_shorts, int32_t* d_out_points)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, "pcs_radius_outlier_device", d_payload, "d_payload", n_points, "n_points", radius_mm, min_neighbors, d_out,
                            "d_out", out_shorts, d_out_points, "d_out_points", 4))
        return rc;
    return run_device(c, d_payload, n_points, nullptr, radius_mm, min_neighbors, d_out, d_out_points);
}

int pcs_radius_outlier_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points, int radius_mm,
                                      int min_neighbors, int16_t* d_out, size_t out_shorts, int32_t* d_out_points)
{
    static const char who[] = "pcs_radius_outlier_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, who, d_payload, "d_payload", max_points, "max_points", radius_mm, min_neighbors, d_out, "d_out", out_shorts,
                            d_out_points, "d_out_points", 4))
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
    if (int rc = check_args(c, "pcs_radius_outlier", payload, "payload", n_points, "n_points", radius_mm, min_neighbors, out, "out", out_shorts,
                            out_points, "out_points", (unsigned)alignof(int)))
        return rc;
    if (n_points == 0) { *out_points = 0; return PCS_OK; }
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    // the host forms' payload staging (pcs_voxel_grid's: both calls are synchronous, neither leaves anything in it)
    int rc;
    if ((rc = ensure_idle(c, c->s_voxel_in, c->s_voxel_in_cap, bytes))) return rc;
    if ((rc = ensure_idle(c, c->s_voxel_out, c->s_voxel_out_cap, bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->s_voxel_in, payload, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_device(c, c->s_voxel_in, n_points, nullptr, radius_mm, min_neighbors, c->s_voxel_out, c->d_counts))) return rc;
    int32_t kept = 0;
    HIPCHK(c, hipMemcpyAsync(&kept, c->d_counts, sizeof kept, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (kept < 0 || kept > n_points) return fail(c, PCS_ERR_HIP, "pcs_radius_outlier: the kernels reported %d of %d records kept", kept, n_points);
    if (kept) HIPCHK(c, hipMemcpy(out, c->s_voxel_out, (size_t)kept * PCS_POINT_BYTES, hipMemcpyDeviceToHost));
    *out_points = kept;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_radius_outlier: host allocation failed (%s)", ex.what());
}

}  // extern "C"
