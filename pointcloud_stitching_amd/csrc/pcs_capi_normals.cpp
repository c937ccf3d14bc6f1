// pcs_capi_normals.cpp — surface normals' part of the C ABI (include/pcs_hip.h, "surface normals"): the argument checks, the
// workspace and the launches of pcs_kernels_normals.hip over the outlier filter's index (the definition: DESIGN.md section 3; the
// kernels: section 5). The calls read no context predicate — flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH do not matter.

#include <climits>
#include <exception>

#include "pcs_host.h"
#include "pcs_normals_math.h"

using namespace pcs_host;

static_assert(sizeof(pcs_normal_params) == 8 * sizeof(int32_t), "pcs_normal_params is eight int32 words, no padding");

namespace {

constexpr int kMaxPoints = INT_MAX / PCS_POINT_BYTES;      // a payload's byte count fits an int32

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

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

// The normals workspace of a context, at least `need` bytes: ensure_outlier_ws's policy (a quarter of headroom when it grows; growing
// waits for the stream; it never shrinks).
int ensure_normals_ws(pcs_ctx* c, size_t need)
{
    if (need <= c->s_normals_ws_cap && c->s_normals_ws) return PCS_OK;
    const size_t exact = need;
    if (c->s_normals_ws) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        need += need / 4;
    }
    int rc = ensure(c, c->s_normals_ws, c->s_normals_ws_cap, need);
    if (rc == PCS_ERR_NOMEM && need != exact) rc = ensure(c, c->s_normals_ws, c->s_normals_ws_cap, exact);      // the headroom is a wish
    return rc;
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
    if (int rc = ensure_normals_ws(c, index_bytes + up256((size_t)n_points * PCS_NORMAL_BYTES))) return rc;
    void* const index = c->s_normals_ws;
    unsigned long long* const cell_normals = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(c->s_normals_ws) + index_bytes);
    for (int stage = 0; stage <= 5; stage++) {
        KernelTimer timer(c);
        if (timer.rc) return timer.rc;
        // (min_neighbors: stages 0 to 5 do not read it; 1 passes the launcher's range check)
        HIPCHK(c, launch_outlier_stage(stage, d_payload, (uint32_t)n_points, nullptr, (uint32_t)n_points, P.radius_mm, 1, index, index_bytes,
                                       nullptr, nullptr, c->stream));
        if (int rc = timer.finish()) return rc;
    }
    OutlierIndexView view{};
    HIPCHK(c, outlier_index_view((uint32_t)n_points, index, index_bytes, &view));
    const NormalRule rule{P.radius_mm, P.min_neighbors, P.flatness, P.use_viewpoint, P.viewpoint_mm[0], P.viewpoint_mm[1], P.viewpoint_mm[2]};
    {
        KernelTimer timer(c);
        if (timer.rc) return timer.rc;
        HIPCHK(c, launch_normals_estimate((uint32_t)n_points, view, rule, cell_normals, c->stream));
        if (int rc = timer.finish()) return rc;
    }
    KernelTimer timer(c);
    if (timer.rc) return timer.rc;
    HIPCHK(c, launch_normals_gather(d_payload, (uint32_t)n_points, P.radius_mm, view, cell_normals,
                                    reinterpret_cast<unsigned long long*>(d_normals), d_valid, c->stream));
    return timer.finish();
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
    const size_t ib = (size_t)n_points * PCS_POINT_BYTES, ob = (size_t)n_points * PCS_NORMAL_BYTES;
    // the host forms' payload staging (pcs_voxel_grid's and pcs_radius_outlier's: all synchronous, none leaves anything in it)
    int rc;
    if ((rc = ensure_idle(c, c->s_voxel_in, c->s_voxel_in_cap, ib))) return rc;
    if ((rc = ensure_idle(c, c->s_voxel_out, c->s_voxel_out_cap, ob))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->s_voxel_in, payload, ib, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_normals_device(c, c->s_voxel_in, n_points, P, reinterpret_cast<int16_t*>(c->s_voxel_out), c->d_counts))) return rc;
    int32_t count = 0;
    HIPCHK(c, hipMemcpyAsync(&count, c->d_counts, sizeof count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (count < 0 || count > n_points)
        return fail(c, PCS_ERR_HIP, "pcs_estimate_normals: the kernels reported %d of %d records valid", count, n_points);
    HIPCHK(c, hipMemcpy(normals, c->s_voxel_out, ob, hipMemcpyDeviceToHost));
    if (valid) *valid = count;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_estimate_normals: host allocation failed (%s)", ex.what());
}

}  // extern "C"
