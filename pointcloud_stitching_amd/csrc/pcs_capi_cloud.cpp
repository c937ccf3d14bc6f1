// pcs_capi_cloud.cpp — what the payload-cloud family of the C ABI shares (pcs_capi_outlier.cpp, pcs_capi_stat.cpp,
// pcs_capi_normals.cpp, pcs_capi_align.cpp; declared in pcs_host.h): the payload checks of the two filters, the cell index's build
// and the host forms' staging. Nothing here is exported.

#include "pcs_host.h"

namespace pcs_host {

int check_payload_io(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const char* n_name, const void* out,
                     const char* out_name, size_t out_shorts, const void* out_points, const char* points_name, unsigned points_align,
                     const void* stats, const char* stats_name, size_t stats_bytes)
{
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
    if (ranges_overlap(stats, stats_bytes, out, bytes) || ranges_overlap(stats, stats_bytes, in, bytes) || ranges_overlap(stats, stats_bytes, out_points, 4))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s, %s or %s", who, stats_name, in_name, out_name, points_name);
    return PCS_OK;
}

int build_cell_index(pcs_ctx* c, const int16_t* d_payload, int n, int cell_mm, void* index, size_t index_bytes, OutlierIndexView* view)
{
    for (int stage = 0; stage < kIndexStages; stage++)
        PCS_TIMED(c, launch_cell_index_stage(stage, d_payload, (uint32_t)n, nullptr, (uint32_t)n, cell_mm, index, index_bytes, c->stream));
    HIPCHK(c, outlier_index_view((uint32_t)n, index, index_bytes, view));
    return PCS_OK;
}

int stage_payload(pcs_ctx* c, const void* in, size_t in_bytes, size_t out_bytes)
{
    if (int rc = ensure_idle(c, c->s_voxel_in, c->s_voxel_in_cap, in_bytes)) return rc;
    if (int rc = ensure_idle(c, c->s_voxel_out, c->s_voxel_out_cap, out_bytes)) return rc;
    if (in_bytes) HIPCHK(c, hipMemcpyAsync(c->s_voxel_in, in, in_bytes, hipMemcpyHostToDevice, c->stream));
    return PCS_OK;
}

int fetch(pcs_ctx* c, void* dst, const void* d_src, size_t bytes)
{
    HIPCHK(c, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PCS_OK;
}

int fetch_count(pcs_ctx* c, const char* who, int n_points, const char* what, int32_t* count)
{
    if (int rc = fetch(c, count, c->d_counts, sizeof *count)) return rc;
    if (*count < 0 || *count > n_points)
        return fail(c, PCS_ERR_HIP, "%s: the kernels reported %d of %d records %s", who, *count, n_points, what);
    return PCS_OK;
}

}  // namespace pcs_host
