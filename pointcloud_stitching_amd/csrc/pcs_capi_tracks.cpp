// pcs_capi_tracks.cpp — the object tracker's part of the C ABI (include/pcs_hip.h, "object tracks"): the tracker object, the argument
// checks and the launches of pcs_kernels_tracks.hip (the definition: DESIGN.md section 3; the kernels: section 5). The calls read no
// context predicate and borrow no context slab: a tracker's tables are its own allocation, as a background model's table is.

#include <algorithm>
#include <exception>
#include <new>

#include "pcs_host.h"

using namespace pcs_host;

// `frames` and the parity live on the host: every update adds exactly one and swaps the two maps, whatever the device finds.
struct pcs_tracker {
    pcs_ctx*  owner = nullptr;      // the context that created it and whose pcs_destroy frees it if nobody did
    int       device = 0;
    int       cell_mm = 0, max_cells = 0, max_objects = 0;
    long long frames = 0;
    int       parity = 0;           // which map holds P(t-1)
    bool      torn = false;         // an update failed between its launches: the tables are half built until a reset
    void*     d_mem = nullptr;
};

namespace {

constexpr size_t kStatsBytes = sizeof(pcs_track_stats);
static_assert(kStatsBytes == 64, "the statistics block is eight int64");
static_assert(sizeof(pcs_track) == 24, "pcs_track is 24 bytes");
static_assert(sizeof(pcs_track_params) == 4 * sizeof(int32_t), "pcs_track_params is four 32-bit words, no padding");
static_assert(sizeof(struct pcs_tracker_info) == 40, "pcs_tracker_info is 40 bytes, no padding");

TrackerView view_of(const pcs_tracker* tr)
{
    return tracker_view(tr->d_mem, tr->cell_mm, (uint32_t)tr->max_cells, (uint32_t)tr->max_objects, tr->parity);
}

int check_tracker(pcs_ctx* c, const char* who, const pcs_tracker* tr)
{
    if (!tr) return fail(c, PCS_ERR_INVALID_ARG, "%s: tr is NULL", who);
    if (tr->device != c->device)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: tr lives on device %d, the context on device %d", who, tr->device, c->device);
    return PCS_OK;
}

// What every update form checks. The names are the form's own argument names; d_n_points is the counted form's word (or NULL).
struct UpdateNames { const char *payload, *n_points, *object_of, *n_objects, *tracks, *stats; };
int check_update(pcs_ctx* c, const char* who, const UpdateNames& nm, const pcs_tracker* tr, const void* payload, int n_points,
                 const void* object_of, const void* n_objects, bool need_n_objects, int max_objects, const pcs_track_params* params,
                 const void* tracks, const void* stats, const void* d_n_points)
{
    if (int rc = check_tracker(c, who, tr)) return rc;
    if (tr->torn)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: an earlier update of tr failed between its launches: pcs_tracker_reset it first", who);
    if (!params) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (params->min_votes < 1 || params->min_votes > PCS_TRACKER_MIN_VOTES_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->min_votes %d is outside 1..%d", who, params->min_votes, PCS_TRACKER_MIN_VOTES_MAX);
    if (params->reserved[0] || params->reserved[1] || params->reserved[2])
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->reserved is not 0", who);
    if (n_points < 0 || n_points > kMaxPoints)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside 0..%d", who, nm.n_points, n_points, kMaxPoints);
    if (n_points && !payload) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.payload);
    if ((uintptr_t)payload & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, nm.payload);
    if (n_points && !object_of) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.object_of);
    if ((uintptr_t)object_of & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, nm.object_of);
    if (need_n_objects && !n_objects) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.n_objects);
    if ((uintptr_t)n_objects & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", who, nm.n_objects);
    if (max_objects < 0 || max_objects > tr->max_objects)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: max_objects %d is outside 0..%d, the tracker's", who, max_objects, tr->max_objects);
    if (max_objects && !tracks) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, nm.tracks);
    if ((uintptr_t)tracks & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, nm.tracks);
    if ((uintptr_t)stats & 7u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 8-byte aligned", who, nm.stats);
    if (d_n_points && ((uintptr_t)d_n_points & 3u)) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    const NamedRange outs[] = {{tracks, (size_t)max_objects * sizeof(pcs_track), nm.tracks}, {stats, kStatsBytes, nm.stats}};
    const NamedRange ins[] = {{payload, (size_t)n_points * PCS_POINT_BYTES, nm.payload}, {object_of, (size_t)n_points * 4, nm.object_of},
                              {n_objects, 4, nm.n_objects}, {d_n_points, 4, "d_n_points"}};
    const NamedRange* with = nullptr;
    if (const NamedRange* bad = first_overlap(outs, 2, ins, 4, &with))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: %s overlaps %s", who, bad->name, with ? with->name : "an input");
    return PCS_OK;
}

// An update behind the checks: kTrackLaunches launches, one bracket each. capacity: n_points, or the counted form's max_points.
int launch_update(pcs_ctx* c, pcs_tracker* tr, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const int32_t* d_object_of,
               const int32_t* d_n_objects, int max_objects, const pcs_track_params& P, pcs_track* d_tracks, pcs_track_stats* d_stats)
{
    DeviceGuard guard(c->device);
    const TrackerView t = view_of(tr);
    const uint32_t cap = (uint32_t)capacity, mo = (uint32_t)max_objects;
    PCS_TIMED(c, launch_track_records(t, d_payload, d_n_points ? 0u : cap, d_n_points, cap, d_object_of, d_n_objects, mo, c->stream));
    PCS_TIMED(c, launch_track_choose(t, c->stream));
    PCS_TIMED(c, launch_track_claim(t, d_n_objects, mo, c->stream));
    PCS_TIMED(c, launch_track_assign(t, d_n_objects, mo, (uint32_t)P.min_votes, tr->frames + 1, d_tracks, reinterpret_cast<long long*>(d_stats),
                                     c->stream));
    return PCS_OK;
}

// ... and the host's half of the state: a frame and the maps swapped, or, where a launch failed, the tracker marked torn (the record
// pass may have filled the new map and the pair table already: nothing may vote against them).
int run_update(pcs_ctx* c, pcs_tracker* tr, const int16_t* d_payload, int capacity, const int32_t* d_n_points, const int32_t* d_object_of,
               const int32_t* d_n_objects, int max_objects, const pcs_track_params& P, pcs_track* d_tracks, pcs_track_stats* d_stats)
{
    const int rc = launch_update(c, tr, d_payload, capacity, d_n_points, d_object_of, d_n_objects, max_objects, P, d_tracks, d_stats);
    if (rc != PCS_OK) { tr->torn = true; return rc; }
    tr->frames++;
    tr->parity ^= 1;
    return PCS_OK;
}

// A device allocation that lives as long as one call.
struct Scratch {
    void* p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
};

void forget(pcs_tracker* tr)
{
    if (!tr->owner) return;
    auto& v = tr->owner->trackers;
    v.erase(std::remove(v.begin(), v.end(), tr), v.end());
}

}  // namespace

namespace pcs_host {

void free_trackers(pcs_ctx* c)
{
    for (pcs_tracker* tr : c->trackers) {
        if (tr->d_mem) (void)hipFree(tr->d_mem);
        delete tr;
    }
    c->trackers.clear();
}

}  // namespace pcs_host

extern "C" {

int pcs_tracker_create(pcs_ctx* c, int cell_mm, int max_cells, int max_objects, pcs_tracker** out)
{
    static const char who[] = "pcs_tracker_create";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (!out) return fail(c, PCS_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (cell_mm < PCS_BACKGROUND_CELL_MIN || cell_mm > PCS_BACKGROUND_CELL_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: cell_mm %d is outside %d..%d", who, cell_mm, PCS_BACKGROUND_CELL_MIN, PCS_BACKGROUND_CELL_MAX);
    if (max_cells < 1 || max_cells > PCS_TRACKER_MAX_CELLS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: max_cells %d is outside 1..%d", who, max_cells, PCS_TRACKER_MAX_CELLS_MAX);
    if (max_objects < 1 || max_objects > PCS_CLUSTER_OBJECTS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: max_objects %d is outside 1..%d", who, max_objects, PCS_CLUSTER_OBJECTS_MAX);
    DeviceGuard guard(c->device);
    pcs_tracker* tr = new (std::nothrow) pcs_tracker;
    if (!tr) return fail(c, PCS_ERR_NOMEM, "%s: host allocation failed", who);
    tr->owner = c; tr->device = c->device; tr->cell_mm = cell_mm; tr->max_cells = max_cells; tr->max_objects = max_objects;
    const size_t bytes = tracker_bytes((uint32_t)max_cells, (uint32_t)max_objects);
    if (hipError_t e = hipMalloc(&tr->d_mem, bytes)) {
        (void)hipGetLastError();
        delete tr;
        return fail(c, PCS_ERR_NOMEM, "%s: hipMalloc(%zu) for max_cells %d, max_objects %d failed: %s", who, bytes, max_cells, max_objects,
                    hipGetErrorString(e));
    }
    const auto undo = [&](int rc) { (void)hipFree(tr->d_mem); delete tr; return rc; };
    try { c->trackers.push_back(tr); } catch (const std::exception&) { return undo(fail(c, PCS_ERR_NOMEM, "%s: host allocation failed", who)); }
    const auto clear = [&]() -> int { PCS_TIMED(c, launch_track_clear(view_of(tr), 1, c->stream)); return PCS_OK; };
    if (int rc = clear()) { c->trackers.pop_back(); return undo(rc); }
    *out = tr;
    return PCS_OK;
}

int pcs_tracker_destroy(pcs_ctx* c, pcs_tracker* tr)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_tracker(c, "pcs_tracker_destroy", tr)) return rc;
    DeviceGuard guard(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));           // a launch on this stream may still use the tables
    if (tr->owner && tr->owner != c && tr->owner->stream) HIPCHK(c, hipStreamSynchronize(tr->owner->stream));
    forget(tr);
    if (tr->d_mem) (void)hipFree(tr->d_mem);
    delete tr;
    return PCS_OK;
}

int pcs_tracker_reset(pcs_ctx* c, pcs_tracker* tr, int64_t first_id)
{
    static const char who[] = "pcs_tracker_reset";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_tracker(c, who, tr)) return rc;
    if (first_id < 1 || first_id > PCS_TRACKER_FIRST_ID_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: first_id %lld is outside 1..2^62", who, (long long)first_id);
    DeviceGuard guard(c->device);
    PCS_TIMED(c, launch_track_clear(view_of(tr), first_id, c->stream));
    tr->frames = 0;
    tr->parity = 0;
    tr->torn = false;
    return PCS_OK;
}

int pcs_tracker_update_device(pcs_ctx* c, pcs_tracker* tr, const int16_t* d_payload, int n_points, const int32_t* d_object_of,
                              const int32_t* d_n_objects, int max_objects, const pcs_track_params* params, pcs_track* d_tracks,
                              pcs_track_stats* d_stats)
{
    static const UpdateNames nm{"d_payload", "n_points", "d_object_of", "d_n_objects", "d_tracks", "d_stats"};
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_update(c, "pcs_tracker_update_device", nm, tr, d_payload, n_points, d_object_of, d_n_objects, true, max_objects, params,
                              d_tracks, d_stats, nullptr))
        return rc;
    return run_update(c, tr, d_payload, n_points, nullptr, d_object_of, d_n_objects, max_objects, *params, d_tracks, d_stats);
}

int pcs_tracker_update_device_counted(pcs_ctx* c, pcs_tracker* tr, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                      const int32_t* d_object_of, const int32_t* d_n_objects, int max_objects,
                                      const pcs_track_params* params, pcs_track* d_tracks, pcs_track_stats* d_stats)
{
    static const char who[] = "pcs_tracker_update_device_counted";
    static const UpdateNames nm{"d_payload", "max_points", "d_object_of", "d_n_objects", "d_tracks", "d_stats"};
    if (!c) return PCS_ERR_INVALID_ARG;
    if (tr && !d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if (int rc = check_update(c, who, nm, tr, d_payload, max_points, d_object_of, d_n_objects, true, max_objects, params, d_tracks, d_stats,
                              d_n_points))
        return rc;
    return run_update(c, tr, d_payload, max_points, d_n_points, d_object_of, d_n_objects, max_objects, *params, d_tracks, d_stats);
}

int pcs_tracker_update(pcs_ctx* c, pcs_tracker* tr, const int16_t* payload, int n_points, const int32_t* object_of, int n_objects,
                       int max_objects, const pcs_track_params* params, pcs_track* tracks, pcs_track_stats* stats)
{
    static const char who[] = "pcs_tracker_update";
    static const UpdateNames nm{"payload", "n_points", "object_of", "n_objects", "tracks", "stats"};
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_update(c, who, nm, tr, payload, n_points, object_of, nullptr, false, max_objects, params, tracks, stats, nullptr))
        return rc;
    DeviceGuard guard(c->device);
    if (n_points)
        if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, 0)) return rc;
    // one allocation for this call: the statistics block, the tracks, the object count, object_of
    const size_t tracks_bytes = (size_t)max_objects * sizeof(pcs_track), at_tracks = up256(kStatsBytes), at_m = at_tracks + up256(tracks_bytes),
                 at_object_of = at_m + 256, bytes = at_object_of + (size_t)n_points * 4;
    Scratch mem;
    if (hipError_t e = hipMalloc(&mem.p, bytes)) {
        (void)hipGetLastError();
        return fail(c, PCS_ERR_NOMEM, "%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(e));
    }
    uint8_t* const base = static_cast<uint8_t*>(mem.p);
    pcs_track_stats* const d_stats = reinterpret_cast<pcs_track_stats*>(base);
    pcs_track* const d_tracks = reinterpret_cast<pcs_track*>(base + at_tracks);
    int32_t* const d_m = reinterpret_cast<int32_t*>(base + at_m);
    int32_t* const d_object_of = reinterpret_cast<int32_t*>(base + at_object_of);
    const int32_t m_word = n_objects;
    HIPCHK(c, hipMemcpyAsync(d_m, &m_word, 4, hipMemcpyHostToDevice, c->stream));
    if (n_points) HIPCHK(c, hipMemcpyAsync(d_object_of, object_of, (size_t)n_points * 4, hipMemcpyHostToDevice, c->stream));
    if (int rc = run_update(c, tr, c->s_voxel_in, n_points, nullptr, d_object_of, d_m, max_objects, *params, d_tracks, d_stats)) return rc;
    const int m = std::min(std::max(n_objects, 0), max_objects);
    pcs_track_stats got{};
    HIPCHK(c, hipMemcpyAsync(&got, d_stats, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    if (m) HIPCHK(c, hipMemcpyAsync(tracks, d_tracks, (size_t)m * sizeof(pcs_track), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (stats) *stats = got;
    return PCS_OK;
}

int pcs_tracker_info(pcs_ctx* c, pcs_tracker* tr, struct pcs_tracker_info* info)
{
    static const char who[] = "pcs_tracker_info";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_tracker(c, who, tr)) return rc;
    if (!info) return fail(c, PCS_ERR_INVALID_ARG, "%s: info is NULL", who);
    DeviceGuard guard(c->device);
    TrackCtl ctl{};
    if (int rc = fetch(c, &ctl, view_of(tr).ctl, sizeof ctl)) return rc;
    info->cell_mm = tr->cell_mm; info->max_cells = tr->max_cells; info->max_objects = tr->max_objects;
    info->objects = (int32_t)ctl.m; info->frames = tr->frames; info->next_id = ctl.next_id;
    info->overflow = (int32_t)(ctl.last_overflow | (ctl.prev_overflow ? 4u : 0u)); info->reserved = 0;
    return PCS_OK;
}

}  // extern "C"
