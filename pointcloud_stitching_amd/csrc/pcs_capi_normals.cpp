// pcs_capi_normals.cpp — surface normals' part of the C ABI (include/pcs_hip.h, "surface normals"): the argument checks, the
// workspace and the launches of pcs_kernels_normals.hip over the outlier filter's index (the definition: DESIGN.md section 3; the
// kernels: section 5). The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter.

#include <exception>

#include "pcs_host.h"
#include "pcs_normals_math.h"

using namespace pcs_host;

static_assert(sizeof(pcs_normal_params) == 8 * sizeof(int32_t), "pcs_normal_params is eight int32 words, no padding");

namespace {

// What both forms check first; `who` names the entry point, in / out / valid its own argument names.
int check_args(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const pcs_normal_params* params,
               const void* out, const char* out_name, const void* valid, const char* valid_name, unsigned valid_align)
{
    if (int rc = check_normal_params(c, who, params)) return rc;
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: n_points %d is outside 0..%d", who, n_points, kMaxPoints);
    if (n_points && !in) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, in_name);
    if (n_points && !out) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, out_name);
    if ((uintptr_t)in & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, in_name);
    if ((uintptr_t)out & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, out_name);
    if ((uintptr_t)valid & (valid_align - 1u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not %u-byte aligned", who, valid_name, valid_align);
    const size_t ib = (size_t)n_points * PCS_POINT_BYTES, ob = (size_t)n_points * PCS_NORMAL_BYTES;
    if (ranges_overlap(in, ib, out, ob)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, out_name, in_name);
    if (ranges_overlap(valid, 4, in, ib) || ranges_overlap(valid, 4, out, ob))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s or %s", who, valid_name, in_name, out_name);
    if (ranges_overlap(params, sizeof *params, out, ob) || ranges_overlap(params, sizeof *params, valid, 4))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params overlaps %s or %s", who, out_name, valid_name);
    return PCS_OK;
}

}  // namespace

namespace pcs_host {

int check_normal_params(pcs_ctx* c, const char* who, const pcs_normal_params* params)
{
    if (!params) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (params->radius_mm < PCS_NORMAL_RADIUS_MIN || params->radius_mm > PCS_NORMAL_RADIUS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: radius_mm %d is outside %d..%d", who, params->radius_mm, PCS_NORMAL_RADIUS_MIN,
                    PCS_NORMAL_RADIUS_MAX);
    if (params->min_neighbors < PCS_NORMAL_NEIGHBORS_MIN || params->min_neighbors > PCS_NORMAL_NEIGHBORS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: min_neighbors %d is outside %d..%d", who, params->min_neighbors, PCS_NORMAL_NEIGHBORS_MIN,
                    PCS_NORMAL_NEIGHBORS_MAX);
    if (params->flatness < 0 || params->flatness > PCS_NORMAL_FLATNESS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: flatness %d is outside 0..%d", who, params->flatness, PCS_NORMAL_FLATNESS_MAX);
    if (params->use_viewpoint != 0 && params->use_viewpoint != 1)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: use_viewpoint %d is neither 0 nor 1", who, params->use_viewpoint);
    if (params->reserved != 0) return fail(c, PCS_ERR_INVALID_ARG, "%s: reserved %d is not 0", who, params->reserved);
    return PCS_OK;
}

// The launches, behind the checks: the index (six), estimate, gather — one timing bracket each. n_points 0: a zero count, no launch.
int run_normals_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_normal_params& P, int16_t* d_normals, int32_t* d_valid)
{
    DeviceGuard guard(c->device);
    if (d_valid) HIPCHK(c, hipMemsetAsync(d_valid, 0, sizeof(int32_t), c->stream));
    if (n_points == 0) return PCS_OK;
    // one call's carve: the payload's index first (outlier_workspace_bytes(n_points), 256-byte aligned as the slab is), then the
    // normals in cell order
    const size_t index_bytes = up256(outlier_workspace_bytes((uint32_t)n_points));
    if (int rc = ensure_ws(c, c->s_normals_ws, c->s_normals_ws_cap, index_bytes + up256((size_t)n_points * PCS_NORMAL_BYTES))) return rc;
    void* const index = c->s_normals_ws;
    unsigned long long* const cell_normals = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(c->s_normals_ws) + index_bytes);
    OutlierIndexView view{};
    if (int rc = build_cell_index(c, d_payload, n_points, P.radius_mm, index, index_bytes, &view)) return rc;
    const NormalRule rule{P.radius_mm, P.min_neighbors, P.flatness, P.use_viewpoint, P.viewpoint_mm[0], P.viewpoint_mm[1], P.viewpoint_mm[2]};
    PCS_TIMED(c, launch_normals_estimate((uint32_t)n_points, view, rule, cell_normals, c->stream));
    PCS_TIMED(c, launch_normals_gather(d_payload, (uint32_t)n_points, P.radius_mm, view, cell_normals,
                                       reinterpret_cast<unsigned long long*>(d_normals), d_valid, c->stream));
    return PCS_OK;
}

}  // namespace pcs_host

extern "C" {

int pcs_estimate_normals_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_normal_params* params, int16_t* d_normals,
                                int32_t* d_valid)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_args(c, "pcs_estimate_normals_device", d_payload, "d_payload", n_points, params, d_normals, "d_normals", d_valid,
                            "d_valid", 4))
        return rc;
    return run_normals_device(c, d_payload, n_points, *params, d_normals, d_valid);
}

int pcs_estimate_normals(pcs_ctx* c, const int16_t* payload, int n_points, const pcs_normal_params* params, int16_t* normals, int* valid)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    // (host memory: the shorts are stored one by one, 2-byte alignment of `normals` would do; the device form's rule is kept)
    if (int rc = check_args(c, "pcs_estimate_normals", payload, "payload", n_points, params, normals, "normals", valid, "valid",
                            (unsigned)alignof(int)))
        return rc;
    if (n_points == 0) { if (valid) *valid = 0; return PCS_OK; }
    DeviceGuard guard(c->device);
    const pcs_normal_params P = *params;
    const size_t ob = (size_t)n_points * PCS_NORMAL_BYTES;
    if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, ob)) return rc;
    if (int rc = run_normals_device(c, c->s_voxel_in, n_points, P, reinterpret_cast<int16_t*>(c->s_voxel_out), c->d_counts)) return rc;
    int32_t count = 0;
    if (int rc = fetch_count(c, "pcs_estimate_normals", n_points, "valid", &count)) return rc;
    HIPCHK(c, hipMemcpy(normals, c->s_voxel_out, ob, hipMemcpyDeviceToHost));
    if (valid) *valid = count;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_estimate_normals: host allocation failed (%s)", ex.what());
}

}  // extern "C"
