// pcs_capi_background.cpp — the background model's part of the C ABI (include/pcs_hip.h, "background model and subtraction"): the
// model object, the argument checks and the launches of pcs_kernels_background.hip (the definition: DESIGN.md section 3; the kernels:
// section 5; the container: section 4 and pcs_background_format.h). The calls read no context predicate — flags, crop box, downsample
// and PCS_FLAG_SCALAR_ARITH do not matter: they move records, like pcs_radius_outlier_device. A model's table is its own allocation;
// subtract borrows the radius filter's slab of the calling context for the keep bits and the tile words, as pcs_capi_plane.cpp does.

#include <algorithm>
#include <exception>
#include <new>
#include <vector>

#include "pcs_background_format.h"
#include "pcs_host.h"

using namespace pcs_host;
namespace fmt = pcs_background_format;

// `frames` lives on the host: every learn call adds exactly one, whatever the device finds, so no call has to ask the device for it.
struct pcs_background {
    pcs_ctx*        owner = nullptr;      // the context that created it and whose pcs_destroy frees it if nobody did
    int             device = 0;
    int             cell_mm = 0, max_cells = 0;
    uint32_t        frames = 0;
    void*           d_table = nullptr;
    BackgroundTable t{};
};

namespace {

constexpr size_t kStatsBytes = sizeof(pcs_background_stats);
static_assert(kStatsBytes == 64, "the statistics block is eight int64");
static_assert(sizeof(pcs_background_params) == 4 * sizeof(int32_t), "pcs_background_params is four 32-bit words, no padding");
static_assert(sizeof(struct pcs_background_info) == 6 * sizeof(int32_t), "pcs_background_info is six 32-bit words, no padding");
static_assert(PCS_BACKGROUND_CELL_MIN == fmt::kCellMin && PCS_BACKGROUND_CELL_MAX == fmt::kCellMax &&
              PCS_BACKGROUND_FRAMES_MAX == fmt::kFramesMax && PCS_BACKGROUND_MAX_CELLS_MAX == fmt::kMaxCellsMax, "the container's limits");

int check_model(pcs_ctx* c, const char* who, const pcs_background* bg)
{
    if (!bg) return fail(c, PCS_ERR_INVALID_ARG, "%s: bg is NULL", who);
    if (bg->device != c->device)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: bg lives on device %d, the context on device %d", who, bg->device, c->device);
    return PCS_OK;
}

int check_sizes(pcs_ctx* c, const char* who, int cell_mm, int max_cells)
{
    if (cell_mm < PCS_BACKGROUND_CELL_MIN || cell_mm > PCS_BACKGROUND_CELL_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: cell_mm %d is outside %d..%d", who, cell_mm, PCS_BACKGROUND_CELL_MIN, PCS_BACKGROUND_CELL_MAX);
    if (max_cells < 1 || max_cells > PCS_BACKGROUND_MAX_CELLS_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: max_cells %d is outside 1..%d", who, max_cells, PCS_BACKGROUND_MAX_CELLS_MAX);
    return PCS_OK;
}

int check_params(pcs_ctx* c, const char* who, const pcs_background_params* p)
{
    if (!p) return fail(c, PCS_ERR_INVALID_ARG, "%s: params is NULL", who);
    if (p->min_seen < 1 || p->min_seen > PCS_BACKGROUND_FRAMES_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->min_seen %d is outside 1..%d", who, p->min_seen, PCS_BACKGROUND_FRAMES_MAX);
    if (p->dilate != 0 && p->dilate != 1) return fail(c, PCS_ERR_INVALID_ARG, "%s: params->dilate %d is neither 0 nor 1", who, p->dilate);
    if (p->mode != PCS_BACKGROUND_MODE_REMOVE && p->mode != PCS_BACKGROUND_MODE_KEEP)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: params->mode %d is neither 0 (remove the background) nor 1 (keep it)", who, p->mode);
    if (p->reserved != 0) return fail(c, PCS_ERR_INVALID_ARG, "%s: params->reserved %d is not 0", who, p->reserved);
    return PCS_OK;
}

// What every learn form checks: the model, the frames cap, the count's range, the payload pointer.
int check_learn(pcs_ctx* c, const char* who, const pcs_background* bg, const void* in, const char* in_name, int n_points, const char* n_name)
{
    if (int rc = check_model(c, who, bg)) return rc;
    if (n_points < 0 || n_points > kMaxPoints) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s %d is outside 0..%d", who, n_name, n_points, kMaxPoints);
    if (n_points && !in) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is NULL", who, in_name);
    if ((uintptr_t)in & 1u) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s is not 2-byte aligned", who, in_name);
    if (bg->frames >= PCS_BACKGROUND_FRAMES_MAX)
        return fail(c, PCS_ERR_INVALID_ARG, "%s: bg has learned PCS_BACKGROUND_FRAMES_MAX = %d frame-sets already", who, PCS_BACKGROUND_FRAMES_MAX);
    return PCS_OK;
}

int check_subtract(pcs_ctx* c, const char* who, const pcs_background* bg, const void* in, const char* in_name, int n_points,
                   const char* n_name, const pcs_background_params* params, const void* out, const char* out_name, size_t out_shorts,
                   const void* out_points, const char* points_name, unsigned points_align, const void* stats, const char* stats_name)
{
    if (int rc = check_model(c, who, bg)) return rc;
    if (int rc = check_params(c, who, params)) return rc;
    return check_payload_io(c, who, in, in_name, n_points, n_name, out, out_name, out_shorts, out_points, points_name, points_align, stats,
                            stats_name, kStatsBytes);
}

// The count word of a counted form: given, aligned, and none of its bytes shared with what the call writes.
int check_count_word(pcs_ctx* c, const char* who, const int32_t* d_n_points, int max_points, const void* d_out, const void* d_out_points,
                     const void* d_stats)
{
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if ((uintptr_t)d_n_points & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    if (ranges_overlap(d_n_points, 4, d_out, (size_t)max_points * PCS_POINT_BYTES) || ranges_overlap(d_n_points, 4, d_out_points, 4) ||
        ranges_overlap(d_n_points, 4, d_stats, kStatsBytes))
        return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points overlaps d_out, d_out_points or d_stats", who);
    return PCS_OK;
}

// A new model behind the checks: the table allocated and cleared (one launch), the owner told.
int make_model(pcs_ctx* c, const char* who, int cell_mm, int max_cells, pcs_background** out)
{
    pcs_background* bg = new (std::nothrow) pcs_background;
    if (!bg) return fail(c, PCS_ERR_NOMEM, "%s: host allocation failed", who);
    bg->owner = c; bg->device = c->device; bg->cell_mm = cell_mm; bg->max_cells = max_cells;
    const size_t bytes = background_table_bytes((uint32_t)max_cells);
    if (hipError_t e = hipMalloc(&bg->d_table, bytes)) {
        (void)hipGetLastError();
        delete bg;
        return fail(c, PCS_ERR_NOMEM, "%s: hipMalloc(%zu) for a table of max_cells %d failed: %s", who, bytes, max_cells, hipGetErrorString(e));
    }
    bg->t = background_table(bg->d_table, cell_mm, (uint32_t)max_cells);
    const auto undo = [&](int rc) { (void)hipFree(bg->d_table); delete bg; return rc; };
    try { c->backgrounds.push_back(bg); } catch (const std::exception&) { return undo(fail(c, PCS_ERR_NOMEM, "%s: host allocation failed", who)); }
    const auto clear = [&]() -> int { PCS_TIMED(c, launch_background_clear(bg->t, c->stream)); return PCS_OK; };
    if (int rc = clear()) { c->backgrounds.pop_back(); return undo(rc); }
    *out = bg;
    return PCS_OK;
}

// learn behind the checks. capacity: n_points, or the counted form's max_points. A frame even with nothing to launch.
int run_learn(pcs_ctx* c, pcs_background* bg, const int16_t* d_payload, int capacity, const int32_t* d_n_points)
{
    DeviceGuard guard(c->device);
    if (capacity)
        PCS_TIMED(c, launch_background_learn(bg->t, d_payload, d_n_points ? 0u : (uint32_t)capacity, d_n_points, (uint32_t)capacity,
                                             bg->frames + 1u, c->stream));
    bg->frames++;
    return PCS_OK;
}

// subtract behind the checks: flag, the radius filter's three compaction launches and, with d_stats, the block; one bracket per launch.
int run_subtract(pcs_ctx* c, pcs_background* bg, const int16_t* d_payload, int capacity, const int32_t* d_n_points,
                 const pcs_background_params& P, int16_t* d_out, int32_t* d_out_points, pcs_background_stats* d_stats)
{
    DeviceGuard guard(c->device);
    if (capacity == 0) {         // nothing to launch: a zero count, a zeroed block
        HIPCHK(c, hipMemsetAsync(d_out_points, 0, sizeof(int32_t), c->stream));
        if (d_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, kStatsBytes, c->stream));
        return PCS_OK;
    }
    const uint32_t cap = (uint32_t)capacity;
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, outlier_workspace_bytes(cap))) return rc;
    PCS_TIMED(c, launch_background_flag(bg->t, d_payload, d_n_points ? 0u : cap, d_n_points, cap, P.min_seen, P.dilate, P.mode,
                                        c->s_outlier_ws, c->s_outlier_ws_cap, c->stream));
    for (int stage = 7; stage <= 9; stage++)
        PCS_TIMED(c, launch_outlier_compact_stage(stage, d_payload, cap, c->s_outlier_ws, c->s_outlier_ws_cap, d_out, d_out_points, c->stream));
    if (d_stats)
        PCS_TIMED(c, launch_background_stats(bg->t, cap, c->s_outlier_ws, c->s_outlier_ws_cap, d_out_points, bg->frames, P.min_seen, P.mode,
                                             reinterpret_cast<long long*>(d_stats), c->stream));
    return PCS_OK;
}

int read_ctl(pcs_ctx* c, const pcs_background* bg, BackgroundCtl* ctl) { return fetch(c, ctl, bg->t.ctl, sizeof *ctl); }

// A device allocation that lives as long as one call.
struct Scratch {
    void* p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
};

void forget(pcs_background* bg)
{
    if (!bg->owner) return;
    auto& v = bg->owner->backgrounds;
    v.erase(std::remove(v.begin(), v.end(), bg), v.end());
}

}  // namespace

namespace pcs_host {

void free_backgrounds(pcs_ctx* c)
{
    for (pcs_background* bg : c->backgrounds) {
        if (bg->d_table) (void)hipFree(bg->d_table);
        delete bg;
    }
    c->backgrounds.clear();
}

}  // namespace pcs_host

extern "C" {

int pcs_background_create(pcs_ctx* c, int cell_mm, int max_cells, pcs_background** out)
{
    static const char who[] = "pcs_background_create";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (!out) return fail(c, PCS_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (int rc = check_sizes(c, who, cell_mm, max_cells)) return rc;
    DeviceGuard guard(c->device);
    return make_model(c, who, cell_mm, max_cells, out);
}

int pcs_background_destroy(pcs_ctx* c, pcs_background* bg)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_model(c, "pcs_background_destroy", bg)) return rc;
    DeviceGuard guard(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));           // a launch on this stream may still read the table
    if (bg->owner && bg->owner != c && bg->owner->stream) HIPCHK(c, hipStreamSynchronize(bg->owner->stream));
    forget(bg);
    if (bg->d_table) (void)hipFree(bg->d_table);
    delete bg;
    return PCS_OK;
}

int pcs_background_reset(pcs_ctx* c, pcs_background* bg)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_model(c, "pcs_background_reset", bg)) return rc;
    DeviceGuard guard(c->device);
    PCS_TIMED(c, launch_background_clear(bg->t, c->stream));
    bg->frames = 0;
    return PCS_OK;
}

int pcs_background_learn_device(pcs_ctx* c, pcs_background* bg, const int16_t* d_payload, int n_points)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_learn(c, "pcs_background_learn_device", bg, d_payload, "d_payload", n_points, "n_points")) return rc;
    return run_learn(c, bg, d_payload, n_points, nullptr);
}

int pcs_background_learn_device_counted(pcs_ctx* c, pcs_background* bg, const int16_t* d_payload, const int32_t* d_n_points, int max_points)
{
    static const char who[] = "pcs_background_learn_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_learn(c, who, bg, d_payload, "d_payload", max_points, "max_points")) return rc;
    if (!d_n_points) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is NULL", who);
    if ((uintptr_t)d_n_points & 3u) return fail(c, PCS_ERR_INVALID_ARG, "%s: d_n_points is not 4-byte aligned", who);
    return run_learn(c, bg, d_payload, max_points, d_n_points);
}

int pcs_background_learn(pcs_ctx* c, pcs_background* bg, const int16_t* payload, int n_points)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_learn(c, "pcs_background_learn", bg, payload, "payload", n_points, "n_points")) return rc;
    DeviceGuard guard(c->device);
    if (n_points)
        if (int rc = stage_payload(c, payload, (size_t)n_points * PCS_POINT_BYTES, 0)) return rc;
    if (int rc = run_learn(c, bg, c->s_voxel_in, n_points, nullptr)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PCS_OK;
}

int pcs_background_subtract_device(pcs_ctx* c, pcs_background* bg, const int16_t* d_payload, int n_points, const pcs_background_params* params,
                                   int16_t* d_out, size_t out_shorts, int32_t* d_out_points, pcs_background_stats* d_stats)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_subtract(c, "pcs_background_subtract_device", bg, d_payload, "d_payload", n_points, "n_points", params, d_out, "d_out",
                                out_shorts, d_out_points, "d_out_points", 4, d_stats, "d_stats"))
        return rc;
    return run_subtract(c, bg, d_payload, n_points, nullptr, *params, d_out, d_out_points, d_stats);
}

int pcs_background_subtract_device_counted(pcs_ctx* c, pcs_background* bg, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                           const pcs_background_params* params, int16_t* d_out, size_t out_shorts, int32_t* d_out_points,
                                           pcs_background_stats* d_stats)
{
    static const char who[] = "pcs_background_subtract_device_counted";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_subtract(c, who, bg, d_payload, "d_payload", max_points, "max_points", params, d_out, "d_out", out_shorts, d_out_points,
                                "d_out_points", 4, d_stats, "d_stats"))
        return rc;
    if (int rc = check_count_word(c, who, d_n_points, max_points, d_out, d_out_points, d_stats)) return rc;
    return run_subtract(c, bg, d_payload, max_points, d_n_points, *params, d_out, d_out_points, d_stats);
}

int pcs_background_subtract(pcs_ctx* c, pcs_background* bg, const int16_t* payload, int n_points, const pcs_background_params* params,
                            int16_t* out, size_t out_shorts, int* out_points, pcs_background_stats* stats)
{
    static const char who[] = "pcs_background_subtract";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_subtract(c, who, bg, payload, "payload", n_points, "n_points", params, out, "out", out_shorts, out_points, "out_points",
                                (unsigned)alignof(int), stats, "stats"))
        return rc;
    if (n_points == 0) {
        *out_points = 0;
        if (stats) *stats = pcs_background_stats{};
        return PCS_OK;
    }
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)n_points * PCS_POINT_BYTES;
    if (int rc = stage_payload(c, payload, bytes, bytes)) return rc;
    // the host form's block: 256 bytes behind the radius filter's carve of the slab (asked for here, so that run_subtract finds it)
    const size_t carve = outlier_workspace_bytes((uint32_t)n_points);
    if (int rc = ensure_ws(c, c->s_outlier_ws, c->s_outlier_ws_cap, carve + 256)) return rc;
    pcs_background_stats* const d_block = stats ? reinterpret_cast<pcs_background_stats*>(static_cast<uint8_t*>(c->s_outlier_ws) + carve) : nullptr;
    if (int rc = run_subtract(c, bg, c->s_voxel_in, n_points, nullptr, *params, c->s_voxel_out, c->d_counts, d_block)) return rc;
    pcs_background_stats got{};
    if (d_block) HIPCHK(c, hipMemcpyAsync(&got, d_block, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    int32_t kept = 0;
    if (int rc = fetch_count(c, who, n_points, "kept", &kept)) return rc;
    if (kept) HIPCHK(c, hipMemcpy(out, c->s_voxel_out, (size_t)kept * PCS_POINT_BYTES, hipMemcpyDeviceToHost));
    *out_points = kept;
    if (stats) *stats = got;
    return PCS_OK;
}

int pcs_background_info(pcs_ctx* c, pcs_background* bg, struct pcs_background_info* info)
{
    static const char who[] = "pcs_background_info";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_model(c, who, bg)) return rc;
    if (!info) return fail(c, PCS_ERR_INVALID_ARG, "%s: info is NULL", who);
    DeviceGuard guard(c->device);
    BackgroundCtl ctl{};
    if (int rc = read_ctl(c, bg, &ctl)) return rc;
    info->cell_mm = bg->cell_mm; info->max_cells = bg->max_cells;
    info->cells = ctl.cells; info->frames = bg->frames;
    info->overflow = ctl.overflow ? 1 : 0; info->reserved = 0;
    return PCS_OK;
}

size_t pcs_background_export_bound(int max_cells)
{
    return fmt::bound(max_cells < 0 ? 0u : (uint32_t)max_cells);
}

int pcs_background_export(pcs_ctx* c, pcs_background* bg, void* out, size_t capacity, size_t* out_bytes)
try {
    static const char who[] = "pcs_background_export";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (int rc = check_model(c, who, bg)) return rc;
    if (!out) return fail(c, PCS_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (!out_bytes) return fail(c, PCS_ERR_INVALID_ARG, "%s: out_bytes is NULL", who);
    DeviceGuard guard(c->device);
    BackgroundCtl ctl{};
    if (int rc = read_ctl(c, bg, &ctl)) return rc;
    if (ctl.overflow)
        return fail(c, PCS_ERR_CAPACITY, "%s: the model overflowed its max_cells %d: which cells it holds is unspecified (reset it, or learn "
                    "into a larger one)", who, bg->max_cells);
    if (ctl.cells > (uint32_t)bg->max_cells)
        return fail(c, PCS_ERR_HIP, "%s: the kernels reported %u cells of at most %d without the overflow flag", who, ctl.cells, bg->max_cells);
    const size_t need = fmt::bound(ctl.cells);
    if (capacity < need) return fail(c, PCS_ERR_CAPACITY, "%s: out holds %zu bytes, %u cells need %zu", who, capacity, ctl.cells, need);
    std::vector<uint32_t> got((size_t)ctl.cells * 4);
    if (ctl.cells) {
        Scratch staging;
        if (hipError_t e = hipMalloc(&staging.p, got.size() * sizeof(uint32_t))) {
            (void)hipGetLastError();
            return fail(c, PCS_ERR_NOMEM, "%s: hipMalloc(%zu) failed: %s", who, got.size() * sizeof(uint32_t), hipGetErrorString(e));
        }
        HIPCHK(c, hipMemsetAsync(&bg->t.ctl->cursor, 0, sizeof(uint32_t), c->stream));
        PCS_TIMED(c, launch_background_gather(bg->t, staging.p, ctl.cells, c->stream));
        HIPCHK(c, hipMemcpyAsync(got.data(), staging.p, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        BackgroundCtl after{};
        if (int rc = read_ctl(c, bg, &after)) return rc;
        if (after.cursor != ctl.cells)
            return fail(c, PCS_ERR_HIP, "%s: the gather found %u occupied slots, the model counts %u cells", who, after.cursor, ctl.cells);
    }
    struct Entry { uint64_t key; uint32_t seen; };
    std::vector<Entry> entries(ctl.cells);
    for (size_t e = 0; e < entries.size(); e++) entries[e] = Entry{(uint64_t)got[4 * e] | (uint64_t)got[4 * e + 1] << 32, got[4 * e + 2]};
    std::sort(entries.begin(), entries.end(), [](const Entry& a, const Entry& b) { return a.key < b.key; });
    uint8_t* w = static_cast<uint8_t*>(out);
    fmt::write_header(w, bg->cell_mm, bg->frames, ctl.cells);
    for (size_t e = 0; e < entries.size(); e++) fmt::write_entry(w + fmt::kHeaderBytes + fmt::kEntryBytes * e, entries[e].key, entries[e].seen);
    *out_bytes = need;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_background_export: host allocation failed (%s)", ex.what());
}

int pcs_background_import(pcs_ctx* c, const void* bytes, size_t n_bytes, int max_cells, pcs_background** out)
{
    static const char who[] = "pcs_background_import";
    if (!c) return PCS_ERR_INVALID_ARG;
    if (!out) return fail(c, PCS_ERR_INVALID_ARG, "%s: out is NULL", who);
    fmt::Info info;
    char why[256];
    if (!fmt::validate(bytes, n_bytes, &info, why, sizeof why)) return fail(c, PCS_ERR_INVALID_ARG, "%s: %s", who, why);
    if (int rc = check_sizes(c, who, info.cell_mm, max_cells)) return rc;
    if (info.cells > (uint32_t)max_cells)
        return fail(c, PCS_ERR_CAPACITY, "%s: the container holds %u cells, max_cells is %d", who, info.cells, max_cells);
    DeviceGuard guard(c->device);
    Scratch entries;
    const size_t entry_bytes = (size_t)info.cells * fmt::kEntryBytes;
    if (info.cells) {
        if (hipError_t e = hipMalloc(&entries.p, entry_bytes)) {
            (void)hipGetLastError();
            return fail(c, PCS_ERR_NOMEM, "%s: hipMalloc(%zu) failed: %s", who, entry_bytes, hipGetErrorString(e));
        }
    }
    pcs_background* bg = nullptr;
    if (int rc = make_model(c, who, info.cell_mm, max_cells, &bg)) return rc;
    const auto fill = [&]() -> int {
        if (!info.cells) return PCS_OK;
        HIPCHK(c, hipMemcpyAsync(entries.p, static_cast<const uint8_t*>(bytes) + fmt::kHeaderBytes, entry_bytes, hipMemcpyHostToDevice, c->stream));
        PCS_TIMED(c, launch_background_import(bg->t, entries.p, info.cells, c->stream));
        return PCS_OK;
    };
    int rc = fill();
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PCS_ERR_HIP, "%s: hipStreamSynchronize failed", who);
    if (rc) {
        forget(bg);
        (void)hipFree(bg->d_table);
        delete bg;
        return rc;
    }
    bg->frames = info.frames;
    *out = bg;
    return PCS_OK;
}

int pcs_background_validate(const void* bytes, size_t n_bytes, struct pcs_background_info* info)
{
    fmt::Info got;
    char why[256];
    if (!fmt::validate(bytes, n_bytes, &got, why, sizeof why)) return fail(nullptr, PCS_ERR_INVALID_ARG, "%s", why);
    if (info) {
        info->cell_mm = got.cell_mm; info->max_cells = (int32_t)std::min<uint32_t>(got.cells, INT32_MAX);
        info->cells = got.cells; info->frames = got.frames; info->overflow = 0; info->reserved = 0;
    }
    return PCS_OK;
}

}  // extern "C"
