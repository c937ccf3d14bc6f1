// pcs_capi_boxes.cpp — the object boxes' part of the C ABI (include/pcs_hip.h, "object boxes"): the argument checks, the workspace
// and the launches of pcs_kernels_boxes.hip (the definition: DESIGN.md section 3; the kernels: section 5). The calls read no context
// predicate; the sums of one call live in the context's s_boxes_ws slab, which every call clears for itself.

#include <algorithm>

#include "pcs_host.h"

using namespace pcs_host;

namespace {

static_assert(sizeof(pcs_object_box) == 128, "pcs_object_box is 128 bytes, no padding");
static_assert(kBoxLaunches == PCS_OBJECT_BOXES_LAUNCHES, "the header states the launches of a call");

// What every form checks. The names are the form's own argument names; d_n_points is the counted form's word (or NULL).
struct BoxNames { const char *payload, *n_points, *object_of, *n_objects, *boxes; };
int check_boxes(pcs_ctx* c, const char* who, const BoxNames& nm, const void* payload, int n_points, const void* object_of,
                const void* n_objects, bool need_n_objects, int max_objects, const void* boxes, const void* d_n_points)
{
    if (n_points < 0 || n_points > kMaxPoints)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside 0..%d", who, nm.n_points, n_points, kMaxPoints);
    if (n_points && !payload) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.payload);
    if ((uintptr_t)payload & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, nm.payload);
    if (n_points && !object_of) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.object_of);
    if ((uintptr_t)object_of & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, nm.object_of);
    if (need_n_objects && !n_objects) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.n_objects);
    if ((uintptr_t)n_objects & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, nm.n_objects);
    if (max_objects < 0 || max_objects > PCS_CLUSTER_OBJECTS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: max_objects %d is outside 0..%d", who, max_objects, PCS_CLUSTER_OBJECTS_MAX);
    if (max_objects && !boxes) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.boxes);
    if ((uintptr_t)boxes & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, nm.boxes);
    if (d_n_points && ((uintptr_t)d_n_points & 3u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    const NamedRange outs[] = {{boxes, (size_t)max_objects * sizeof(pcs_object_box), nm.boxes}};
    const NamedRange ins[] = {{payload, (size_t)n_points * PCS_POINT_BYTES, nm.payload}, {object_of, (size_t)n_points * 4, nm.object_of},
                              {n_objects, 4, nm.n_objects}, {d_n_points, 4, "d_n_points"}};
    const NamedRange* with = nullptr;
    if (const NamedRange* bad = first_overlap(outs, 1, ins, 4, &with))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps an input", who, bad->name);
    return PCS_OK;
}

// A call behind the checks: kBoxLaunches launches, one bracket each. capacity: n_points, or the counted form's max_points. d_ws:
// boxes_workspace_bytes(max_objects) bytes of the context's slab.
int launch_boxes(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const int32_t* d_object_of,
                 const int32_t* d_n_objects, int max_objects, void* d_ws, pcs_object_box* d_boxes)
{
    const uint32_t cap = (uint32_t)capacity, n = d_n_points ? 0u : cap, mo = (uint32_t)max_objects;
    PCS_TIMED(c, launch_boxes_clear(d_n_objects, mo, d_ws, c->stream));
    PCS_TIMED(c, launch_boxes_moments(d_payload, n, d_n_points, cap, d_object_of, d_n_objects, mo, d_ws, c->stream));
    PCS_TIMED(c, launch_boxes_axes(d_n_objects, mo, d_ws, d_boxes, c->stream));
    PCS_TIMED(c, launch_boxes_extents(d_payload, n, d_n_points, cap, d_object_of, d_n_objects, mo, d_boxes, c->stream));
    return PCS_OK;
}

int run_boxes_device(pcs_ctx* c, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const int32_t* d_object_of,
                     const int32_t* d_n_objects, int max_objects, pcs_object_box* d_boxes)
{
    DeviceGuard guard(c->device);
    if (int rc = ensure_ws(c, c->s_boxes_ws, c->s_boxes_ws_cap, boxes_workspace_bytes((uint32_t)max_objects))) return rc;
    return launch_boxes(c, d_payload, capacity, d_n_points, d_object_of, d_n_objects, max_objects, c->s_boxes_ws, d_boxes);
}

}  // namespace

extern "C" {

int pcs_object_boxes_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const int32_t* d_object_of, const int32_t* d_n_objects,
                            int max_objects, pcs_object_box* d_boxes)
{
    static const BoxNames nm{"d_payload", "n_points", "d_object_of", "d_n_objects", "d_boxes"};
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_boxes(c, "pcs_object_boxes_device", nm, d_payload, n_points, d_object_of, d_n_objects, true, max_objects, d_boxes,
                             nullptr))
        return rc;
    return run_boxes_device(c, d_payload, n_points, nullptr, d_object_of, d_n_objects, max_objects, d_boxes);
}

int pcs_object_boxes_device_counted(pcs_ctx* c, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                    const int32_t* d_object_of, const int32_t* d_n_objects, int max_objects, pcs_object_box* d_boxes)
{
    static const char who[] = "pcs_object_boxes_device_counted";
    static const BoxNames nm{"d_payload", "max_points", "d_object_of", "d_n_objects", "d_boxes"};
    if (!c) return PCS_ERR_INVALID_ARG;
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if (int rc = check_boxes(c, who, nm, d_payload, max_points, d_object_of, d_n_objects, true, max_objects, d_boxes, d_n_points)) return rc;
    return run_boxes_device(c, d_payload, max_points, d_n_points, d_object_of, d_n_objects, max_objects, d_boxes);
}

int pcs_object_boxes(pcs_ctx* c, const int16_t* payload, int n_points, const int32_t* object_of, int n_objects, int max_objects,
                     pcs_object_box* boxes)
{
    static const char who[] = "pcs_object_boxes";
    static const BoxNames nm{"payload", "n_points", "object_of", "n_objects", "boxes"};
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_boxes(c, who, nm, payload, n_points, object_of, nullptr, false, max_objects, boxes, nullptr)) return rc;
    DeviceGuard guard(c->device);
    if (n_points)
        if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, 0)) return rc;
    // the slab of this call: the sums, the entries, the object count, object_of
    const size_t at_boxes = up256(boxes_workspace_bytes((uint32_t)max_objects)),
                 at_m = at_boxes + up256((size_t)max_objects * sizeof(pcs_object_box)), at_object_of = at_m + 256,
                 bytes = at_object_of + (size_t)n_points * 4;
    if (int rc = ensure_ws(c, c->s_boxes_ws, c->s_boxes_ws_cap, bytes)) return rc;
    uint8_t* const base = static_cast<uint8_t*>(c->s_boxes_ws);
    pcs_object_box* const d_boxes = reinterpret_cast<pcs_object_box*>(base + at_boxes);
    int32_t* const d_m = reinterpret_cast<int32_t*>(base + at_m);
    int32_t* const d_object_of = reinterpret_cast<int32_t*>(base + at_object_of);
    const int32_t m_word = n_objects;
    HIPCHK(c, hipMemcpyAsync(d_m, &m_word, 4, hipMemcpyHostToDevice, c->stream));
    if (n_points) HIPCHK(c, hipMemcpyAsync(d_object_of, object_of, (size_t)n_points * 4, hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_boxes(c, c->s_voxel_in, n_points, nullptr, d_object_of, d_m, max_objects, base, d_boxes)) return rc;
    const int m = std::min(std::max(n_objects, 0), max_objects);
    if (m) HIPCHK(c, hipMemcpyAsync(boxes, d_boxes, (size_t)m * sizeof(pcs_object_box), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PCS_OK;
}

}  // extern "C"
