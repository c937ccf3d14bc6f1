// pcs_capi_plan.cpp — the plan-view maps' part of the C ABI (include/pcs_hip.h, "plan-view maps"): the argument checks, the workspace
// and the launches of pcs_kernels_plan.hip (the definition: DESIGN.md section 3; the kernels: section 5). The calls read no context
// predicate; the keys of one call live in the context's s_plan_ws slab, which every call clears for itself.

#include "pcs_host.h"

using namespace pcs_host;

namespace {

static_assert(sizeof(pcs_plan_params) == kPlanParamWords * sizeof(int32_t), "pcs_plan_params is twelve int32 words, no padding");
static_assert(sizeof(pcs_plan_stats) == 64, "pcs_plan_stats is 64 bytes");
static_assert(kPlanLaunches == PCS_PLAN_VIEW_LAUNCHES, "the header states the launches of a call");
static_assert(kPlanSideMax == PCS_PLAN_SIDE_MAX && kPlanCellsMax == PCS_PLAN_CELLS_MAX, "the header states the caps");

const char* const kParamNames[kPlanParamWords] = {"up_axis", "up_sign", "cell_mm", "origin_u", "origin_v", "width", "height", "band_lo",
                                                  "band_hi", "reserved[0]", "reserved[1]", "reserved[2]"};
const char* const kParamRanges[kPlanParamWords] = {"outside 0..2", "neither +1 nor -1", "outside 1..32767", "outside -32768..32767",
                                                   "outside -32768..32767", "outside 1..4096", "outside 1..4096, or width * height above 4194304",
                                                   "outside -32768..32767", "outside band_lo..32767", "not 0", "not 0", "not 0"};

// The multiply-shift of the cell edge in use, over every numerator it can meet: the sweep of tools/plan_host.cpp says it cannot fail,
// and the call that would launch with a wrong one does not. Once per context and cell edge.
bool division_is_exact(int32_t c)
{
    const uint32_t m = plan_magic(c);
    for (uint32_t d = 0; d < 65536u; d++)
        if (plan_div(d, c, m) != d / (uint32_t)c) return false;
    return true;
}

// What every form checks. d_n_points is the counted form's word (or NULL); n_name the count's own name.
int check_plan(pcs_ctx* c, const char* who, const char* payload_name, const void* payload, int n_points, const char* n_name,
               const pcs_plan_params* params, const pcs_plan_maps* maps, const void* d_n_points, PlanArgs* args)
{
    if (n_points < 0 || n_points > kMaxPoints)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside 0..%d", who, n_name, n_points, kMaxPoints);
    if (n_points && !payload) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, payload_name);
    if ((uintptr_t)payload & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, payload_name);
    if (d_n_points && ((uintptr_t)d_n_points & 3u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    if (!params) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (!maps) return fail(c, PCS_ERR_INVALID_ARG, "%s: maps is NULL", who);
    const int32_t* w = reinterpret_cast<const int32_t*>(params);
    if (const int bad = plan_bad_param(w))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->%s %d is %s", who, kParamNames[bad - 1], w[bad - 1], kParamRanges[bad - 1]);
    const struct { const void* p; unsigned mask; const char* name; } ptrs[] = {
        {maps->count, 3u, "maps->count"}, {maps->top, 1u, "maps->top"}, {maps->bottom, 1u, "maps->bottom"}, {maps->rgb, 0u, "maps->rgb"},
        {maps->stats, 7u, "maps->stats"}};
    for (const auto& q : ptrs) {
        if (!q.p) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, q.name);
        if ((uintptr_t)q.p & q.mask) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not %u-byte aligned", who, q.name, q.mask + 1u);
    }
    const size_t cells = (size_t)params->width * params->height;
    const NamedRange outs[] = {{maps->count, 4 * cells, "maps->count"}, {maps->top, 2 * cells, "maps->top"}, {maps->bottom, 2 * cells, "maps->bottom"},
                               {maps->rgb, 3 * cells, "maps->rgb"}, {maps->stats, sizeof(pcs_plan_stats), "maps->stats"}};
    const NamedRange ins[] = {{payload, (size_t)n_points * PCS_POINT_BYTES, payload_name}, {d_n_points, 4, "d_n_points"},
                              {params, sizeof *params, "params"}, {maps, sizeof *maps, "maps"}};
    const NamedRange* with = nullptr;
    if (const NamedRange* bad = first_overlap(outs, 5, ins, 4, &with))
        return with ? fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, bad->name, with->name)
                    : fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps an input", who, bad->name);
    if (c->plan_cell_checked != params->cell_mm) {
        if (!division_is_exact(params->cell_mm))
            return fail(c, PCS_ERR_INVALID_ARG, "%s: params->cell_mm %d: the multiply-shift division is not exact", who, params->cell_mm);
        c->plan_cell_checked = params->cell_mm;
    }
    *args = PlanArgs{params->up_axis, params->up_sign, params->cell_mm, plan_magic(params->cell_mm), params->origin_u, params->origin_v,
                     params->width, params->height, params->band_lo, params->band_hi};
    return PCS_OK;
}

// A call behind the checks: kPlanLaunches launches, one bracket each. capacity: n_points, or the counted form's max_points. d_ws:
// plan_workspace_bytes(cells) bytes of the context's slab.
int launch_plan(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const PlanArgs& P, void* d_ws,
                const pcs_plan_maps& m)
{
    const uint32_t cap = (uint32_t)capacity, n = d_n_points ? 0u : cap;
    long long* const stats = reinterpret_cast<long long*>(m.stats);
    PCS_TIMED(c, launch_plan_clear(n, d_n_points, cap, P, d_ws, m.count, stats, c->stream));
    PCS_TIMED(c, launch_plan_accumulate(d_payload, n, d_n_points, cap, P, d_ws, m.count, stats, c->stream));
    PCS_TIMED(c, launch_plan_resolve(d_payload, cap, P, d_ws, m.count, m.top, m.bottom, m.rgb, stats, c->stream));
    return PCS_OK;
}

int run_plan_device(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const PlanArgs& P, const pcs_plan_maps& m)
{
    DeviceGuard guard(c->device);
    if (int rc = ensure_ws(c, c->s_plan_ws, c->s_plan_ws_cap, plan_workspace_bytes((uint32_t)(P.width * P.height)))) return rc;
    return launch_plan(c, d_payload, capacity, d_n_points, P, c->s_plan_ws, m);
}

}  // namespace

extern "C" {

int pcs_plan_view_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_plan_params* params, const pcs_plan_maps* maps)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    PlanArgs P;
    if (int rc = check_plan(c, "pcs_plan_view_device", "d_payload", d_payload, n_points, "n_points", params, maps, nullptr, &P)) return rc;
    return run_plan_device(c, d_payload, n_points, nullptr, P, *maps);
}

int pcs_plan_view_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                 const pcs_plan_params* params, const pcs_plan_maps* maps)
{
    static const char who[] = "pcs_plan_view_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    PlanArgs P;
    if (int rc = check_plan(c, who, "d_payload", d_payload, max_points, "max_points", params, maps, d_n_points, &P)) return rc;
    return run_plan_device(c, d_payload, max_points, d_n_points, P, *maps);
}

int pcs_plan_view(pcs_ctx* c, const int16_t* payload, int n_points, const pcs_plan_params* params, const pcs_plan_maps* host_maps)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    PlanArgs P;
    if (int rc = check_plan(c, "pcs_plan_view", "payload", payload, n_points, "n_points", params, host_maps, nullptr, &P)) return rc;
    DeviceGuard guard(c->device);
    if (n_points)
        if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, 0)) return rc;
    // the slab of this call: the keys, then the four rasters and the statistics block
    const size_t cells = (size_t)P.width * P.height;
    const size_t at_count = up256(plan_workspace_bytes((uint32_t)cells)), at_top = at_count + up256(4 * cells), at_bottom = at_top + up256(2 * cells),
                 at_rgb = at_bottom + up256(2 * cells), at_stats = at_rgb + up256(3 * cells), bytes = at_stats + 256;
    if (int rc = ensure_ws(c, c->s_plan_ws, c->s_plan_ws_cap, bytes)) return rc;
    uint8_t* const base = static_cast<uint8_t*>(c->s_plan_ws);
    const pcs_plan_maps d{reinterpret_cast<uint32_t*>(base + at_count), reinterpret_cast<int16_t*>(base + at_top),
                          reinterpret_cast<int16_t*>(base + at_bottom), base + at_rgb, reinterpret_cast<pcs_plan_stats*>(base + at_stats)};
    if (int rc = launch_plan(c, c->s_voxel_in, n_points, nullptr, P, base, d)) return rc;
    HIPCHK(c, hipMemcpyAsync(host_maps->count, d.count, 4 * cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(host_maps->top, d.top, 2 * cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(host_maps->bottom, d.bottom, 2 * cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(host_maps->rgb, d.rgb, 3 * cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(host_maps->stats, d.stats, sizeof(pcs_plan_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PCS_OK;
}

}  // extern "C"
