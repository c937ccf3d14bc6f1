// pcs_host.h — what the translation units of the C ABI share: the context itself and the helpers more than one of them calls.
// pcs_capi.cpp: contexts, the a1 / a2 twins, the fused path, host forms, plumbing; pcs_capi_voxel.cpp: the voxel grid, partials, sinks;
// pcs_capi_codec.cpp: the payload codec; and the payload-cloud family over the cell index — pcs_capi_outlier.cpp, pcs_capi_stat.cpp,
// pcs_capi_normals.cpp, pcs_capi_align.cpp, pcs_capi_cluster.cpp, and pcs_capi_plane.cpp and pcs_capi_background.cpp, which use the family's compaction alone — whose common checks, slab policy, index build and staging live in pcs_capi_cloud.cpp.
// Internal to libpcs_hip.so; nothing here is exported.
#ifndef PCS_HOST_H
#define PCS_HOST_H

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "pcs_device.h"

using namespace pcs;

struct Certificate {
    bool   fast = false, ident_r = false;
    double xb = 0, yb = 0, zb = 0;      // |X|,|Y|,|Z| upper bounds over valid depths
    double a_max[3] = {0, 0, 0};        // |P_i| upper bounds
    double p2_low = 0;                  // P2 lower bound (> 0) over valid depths
};

struct pcs_background;      // pcs_capi_background.cpp
struct pcs_tracker;         // pcs_capi_tracks.cpp

struct pcs_ctx {
    int                             device = 0;
    int                             n_streams = 0;
    uint32_t                        flags = 0;
    int                             downsample = 1;
    std::vector<pcs_stream_config>  cfg;
    std::vector<StreamParams>       h_params;
    StreamParams*                   d_params = nullptr;
    std::vector<float*>             d_lut;            // 2 per stream (mx, my)
    uint32_t                        total_tiles = 0;
    uint32_t*                       d_tile_counts = nullptr;
    uint32_t*                       d_tile_prefix = nullptr;
    uint32_t*                       d_stream_base = nullptr;   // n_streams + 1 (kept points per stream)
    uint32_t*                       d_arrive = nullptr;        // scan arrival counter (self-resetting)
    int32_t*                        d_counts = nullptr;        // n_streams + 1 (internal, for host APIs)
    int32_t*                        d_static_counts = nullptr; // n_streams + 1: ceil(n/downsample) per stream, total
    // batched compaction scratch (pcs_process_frames_device_batch with a predicate): one slab, rows per frame-set
    uint32_t*                       d_batch_scratch = nullptr;
    int                             batch_scratch_sets = 0;
    // single-pass compaction state (pcs_fused_compact_kernel)
    unsigned long long*             d_ticket = nullptr;        // never reset
    unsigned long long              tickets_issued = 0;
    uint64_t*                       d_desc = nullptr;          // one per tile
    uint32_t*                       d_stream_end = nullptr;    // n_streams
    uint32_t*                       d_error = nullptr;
    uint32_t                        compact_seq = 0;
    bool                            single_pass_ok = true;     // cleared if a placement wait ever timed out
    bool                            compact_tickets = false;   // tile ids by atomic ticket instead of blockIdx
    int                             compact_path = 0;          // 0 count + scan + emit (default), 1 single pass by blockIdx (opt-in)
    bool                            dense_ok = false;          // every stream has n % 8 == 0
    bool                            any_ddist = false, any_cdist = false;
    std::vector<int>                math;                      // per stream: 0 IEEE, 1 certified, 2 + identity R, 3/4 = 1/2 + no-overflow
    std::vector<Certificate>        cert;
    uint32_t                        max_points = 0;
    size_t                          max_payload_points = 0;

    hipStream_t                     own_stream = nullptr;
    hipStream_t                     stream = nullptr;
    hipEvent_t                      ev_begin = nullptr, ev_end = nullptr;
    bool                            kernel_timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;    // recorded pairs awaiting drain
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free;

    // lazily sized staging for the host-pointer entry points
    // Rasters of all streams are carved from ONE slab at 256-byte granularity. Separate hipMalloc()s hand
    // out 2 MiB-aligned bases; the streams' tiles advance in lockstep, so equal offsets from power-of-two
    // aligned bases compete for the same sets of the memory-side Infinity Cache: with inputs that were just
    // written (and so sit in that cache) the 8x720p launch measured 22.7 us vs 19.0 us (tools/lab/kernel_lab.hip,
    // "allocation mode", 6-set ring). With cold inputs streamed from HBM the layout makes no difference.
    uint8_t*                        s_slab = nullptr;
    std::vector<uint16_t*>          s_depth;
    std::vector<uint8_t*>           s_color;
    int16_t*                        s_payload = nullptr;  size_t s_payload_cap = 0;   // bytes
    float*                          s_vertices = nullptr; size_t s_vertices_cap = 0;
    float*                          s_texcoords = nullptr; size_t s_texcoords_cap = 0;
    void*                           s_voxel_ws = nullptr; size_t s_voxel_ws_cap = 0;
    VoxelWsState                    vox_state;          // which control block of s_voxel_ws the next voxel call uses
    bool                            sink_open = false;  // pcs_voxel_sink_begin without its pcs_voxel_sink_finish yet
    int                             voxel_reruns = 0;   // calls that ended flagged (-1) and latched the LSD tail (pcs_voxel_tail_reruns)
    int16_t*                        s_voxel_in = nullptr; size_t s_voxel_in_cap = 0;
    int16_t*                        s_voxel_out = nullptr; size_t s_voxel_out_cap = 0;
    uint32_t*                       s_pack_counts = nullptr; uint32_t* s_pack_prefix = nullptr; size_t s_pack_tiles = 0;

    // pcs_submit_frames / pcs_collect_frames: device slots, download stream
    struct PipeSlot {
        uint8_t*               slab = nullptr;
        std::vector<uint16_t*> depth;
        std::vector<uint8_t*>  color;
        int16_t*               payload = nullptr;
        int32_t*               counts = nullptr;       // device, n_streams + 1
        hipEvent_t             done = nullptr;
        bool                   busy = false;
        bool                   pred = false;           // submitted under a predicate (flags or box): the counts are on the device.
                                                       // Kept per slot: pcs_set_crop_box_mm may change the context between submit and collect
        int                    ticket = -1;
    };
    PipeSlot                        pipe[PCS_PIPELINE_DEPTH];
    hipStream_t                     dl_stream = nullptr;
    int                             next_ticket = 0, next_collect = 0;

    struct ZcEntry { const void* host; size_t bytes; void* dev; int verdict; };
    std::vector<ZcEntry>            zc_cache;                  // zero-copy eligibility verdicts (host_device_view)

    // pcs_set_crop_box_mm: the box (flags carries PCS_KFLAG_CROP_BOX while one is set) and pcs_crop_payloads_device's scratch
    int16_t                         box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
    CropBoxArg                      box{};
    StreamParams*                   d_crop_tab = nullptr;      // PCS_MAX_STREAMS entries (n_points, tile_base of each camera)
    uint32_t*                       d_crop_tiles = nullptr; size_t crop_tiles_cap = 0;   // bytes: counts, prefixes, kept per camera

    // pcs_set_depth_filter: the configuration, the per-stream table on the device and the temporal state (one slab: every stream's
    // last [n] uint16 then hist [n] uint8, each carved at 256 bytes; nullptr for hole fill alone)
    bool                            filter_set = false;
    pcs_depth_filter_config         filter_cfg{};
    FilterArgs                      filter_args{};
    FilterStream*                   d_filter_tab = nullptr;
    uint8_t*                        d_filter_state = nullptr; size_t filter_state_bytes = 0;
    uint32_t                        filter_max_rows = 0, filter_max_width = 0;      // the launch's grid and workgroup size

    // pcs_decimate_depth (host pointers): the full-size source rasters' staging, one slab carved at 256 bytes per stream; allocated on
    // first use, grown when a later call needs more. (The decimated outputs land in s_depth, which is decimated-size already.)
    uint8_t*                        d_decim_src = nullptr; size_t decim_src_cap = 0;

    // payload codec (pcs_capi_codec.cpp): the encoder's block sizes, one word per 64 records, grown on demand; the container staged on
    // the device by the host forms (pcs_decompress_payload uploads into it, pcs_process_frames_compressed downloads from it) and
    // their 4-byte byte count
    uint32_t*                       d_codec_sizes = nullptr; size_t codec_sizes_cap = 0;
    uint8_t*                        d_codec_buf = nullptr; size_t codec_buf_cap = 0;
    uint32_t*                       d_codec_bytes = nullptr; size_t codec_bytes_cap = 0;

    // radius outlier removal (pcs_capi_outlier.cpp): the cell index, keep bits and tile words of one call, sized from the call's
    // n_points / max_points alone (outlier_workspace_bytes), grown on demand by ensure_ws as the voxel workspace is
    // (statistical outlier removal, pcs_capi_stat.cpp, asks the same slab for stat_workspace_bytes: the index in front, its own words behind;
    // Euclidean clusters, pcs_capi_cluster.cpp, for cluster_workspace_bytes, carved the same way; plane segmentation,
    // pcs_capi_plane.cpp, for plane_workspace_bytes: its own words in front, the filter's carve behind them for the control block, keep
    // bits and tile words. Every call builds what it reads anew: nothing of one tenant's is read by the next)
    void*                           s_outlier_ws = nullptr; size_t s_outlier_ws_cap = 0;

    // alignment sums and the ICP loop (pcs_capi_align.cpp): the target's cell index (the outlier filter's layout), the match
    // launch's per-workgroup partials, the loop's moved source and sums, the host form's sums and dist2 — one slab carved per call,
    // grown on demand by ensure_ws
    void*                           s_align_ws = nullptr; size_t s_align_ws_cap = 0;

    // surface normals (pcs_capi_normals.cpp): the payload's cell index (the outlier filter's layout) and the normals in cell order,
    // 8 bytes per record — one slab carved per call, grown on demand by ensure_ws
    void*                           s_normals_ws = nullptr; size_t s_normals_ws_cap = 0;

    // background models created on this context and not destroyed yet (pcs_capi_background.cpp): pcs_destroy frees what is left
    std::vector<pcs_background*>    backgrounds;
    // trackers created on this context and not destroyed yet (pcs_capi_tracks.cpp): likewise
    std::vector<pcs_tracker*>       trackers;

    // object boxes (pcs_capi_boxes.cpp): the ten sums per object of one call, boxes_workspace_bytes(max_objects), grown on demand by
    // ensure_ws; the host form's staged object_of, count word and entries ride behind them
    void*                           s_boxes_ws = nullptr; size_t s_boxes_ws_cap = 0;

    // plan-view maps (pcs_capi_plan.cpp): the two keys per cell of one call, plan_workspace_bytes(cells), grown on demand by
    // ensure_ws; the host form's rasters and statistics block ride behind them. plan_cell_checked: the cell edge whose multiply-shift
    // division the host has swept (0: none yet)
    void*                           s_plan_ws = nullptr; size_t s_plan_ws_cap = 0;
    int32_t                         plan_cell_checked = 0;

    std::string                     err;
};

namespace pcs_host {

int fail(pcs_ctx* c, int status, const char* fmt, ...);

#define HIPCHK(c, expr)                                                                     \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return fail((c), PCS_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));   \
    } while (0)

// A compacting predicate is active. Not under PCS_FLAG_SCALAR_ARITH: a3's -c loop leaves record i in slot i, so nothing is compacted,
// the counts are the configuration's and the launches are the predicate-free ones with a per-point select.
inline bool has_pred(uint32_t flags)
{
    return !(flags & PCS_FLAG_SCALAR_ARITH) && (flags & (PCS_FLAG_CUTOFF | PCS_FLAG_DROP_INVALID | PCS_KFLAG_CROP_BOX)) != 0;
}
inline bool has_box(const pcs_ctx* c) { return (c->flags & PCS_KFLAG_CROP_BOX) != 0; }
inline bool scalar_arith(const pcs_ctx* c) { return (c->flags & PCS_FLAG_SCALAR_ARITH) != 0; }
inline bool scalar_cut(const pcs_ctx* c) { return scalar_arith(c) && (c->flags & PCS_FLAG_CUTOFF) != 0; }

// A context created with PCS_FLAG_SCALAR_ARITH returns a3's bytes or fails before anything is launched: no call may hand back -m bytes
// from it. The entry points that have no a3 form refuse such a context first thing.
#define PCS_NO_SCALAR_ARITH(c, name)                                                                                        \
    do {                                                                                                                    \
        if (pcs_host::scalar_arith(c))                                                                                      \
            return pcs_host::fail((c), PCS_ERR_UNSUPPORTED, "%s is not available on a context created with "               \
                                  "PCS_FLAG_SCALAR_ARITH: the reference's default arithmetic covers the a1 / a2 twins and " \
                                  "pcs_process_frames, pcs_process_frames_device, pcs_submit_frames / pcs_collect_frames", name); \
    } while (0)

// The calls that cannot honour a crop box refuse while one is set, before anything is launched or written: a producer's tile counts
// cannot know the world predicate (pcs_process_frames_device_counted), and the a1 / a2 twins are signature twins of reference functions
// that have no such argument.
#define PCS_NO_CROP_BOX(c, name)                                                                                            \
    do {                                                                                                                    \
        if (pcs_host::has_box(c))                                                                                           \
            return pcs_host::fail((c), PCS_ERR_UNSUPPORTED, "%s is not available while a crop box is set "                  \
                                  "(pcs_set_crop_box_mm(ctx, NULL, NULL) clears it)", name);                                \
    } while (0)

template <class T>
int ensure(pcs_ctx* c, T*& p, size_t& cap, size_t bytes)
{
    if (bytes <= cap && p) return PCS_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 256));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, PCS_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
    p = static_cast<T*>(q);
    cap = std::max<size_t>(bytes, 256);
    return PCS_OK;
}

// ensure() for scratch that launches already on the context's stream may still be using: growing waits for the stream first.
template <class T>
int ensure_idle(pcs_ctx* c, T*& p, size_t& cap, size_t bytes)
{
    if (bytes <= cap && p) return PCS_OK;
    if (p) HIPCHK(c, hipStreamSynchronize(c->stream));
    return ensure(c, p, cap, bytes);
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// A workspace slab of a context, at least `need` bytes. Growing it means: wait for the stream (the old one may be in use), free,
// allocate — a device-wide stall. A caller whose sizes creep upwards must not pay that at every new maximum: a slab that has to grow
// takes a quarter more than asked. It never shrinks.
template <class T>
int ensure_ws(pcs_ctx* c, T*& p, size_t& cap, size_t need)
{
    if (need <= cap && p) return PCS_OK;
    const size_t exact = need;
    if (p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        need += need / 4;
    }
    int rc = ensure(c, p, cap, need);
    if (rc == PCS_ERR_NOMEM && need != exact) rc = ensure(c, p, cap, exact);      // the headroom is a wish
    return rc;
}

// pcs_destroy's part of pcs_capi_background.cpp: the tables and objects of c->backgrounds.
void free_backgrounds(pcs_ctx* c);
// pcs_destroy's part of pcs_capi_tracks.cpp: the tables and objects of c->trackers.
void free_trackers(pcs_ctx* c);

// The voxel workspace of a context, at least `need` bytes: ensure_ws, and the control block's state forgotten when it moves.
int ensure_voxel_ws(pcs_ctx* c, size_t need);
int acquire_event_pair(pcs_ctx* c, std::pair<hipEvent_t, hipEvent_t>& pr);

// Surface normals for a caller inside the library (pcs_capi_normals.cpp; the point-to-plane loop estimates its target's): the
// parameter ranges of pcs_normal_params, `who` naming the entry point, and pcs_estimate_normals_device behind its checks.
int check_normal_params(pcs_ctx* c, const char* who, const pcs_normal_params* params);
int run_normals_device(pcs_ctx* c, const int16_t* d_payload, int n_points, const pcs_normal_params& P, int16_t* d_normals, int32_t* d_valid);

// The kernel-timing bracket (pcs_kernel_timing) around the launches of one call: constructed before the first launch, finish() after the
// last. One bracket is one interval of pcs_kernel_times_ms. Every exit between the two, a HIPCHK return included, hands the pair back.
struct KernelTimer {
    pcs_ctx*                          c;
    std::pair<hipEvent_t, hipEvent_t> ev{};
    bool                              open = false;
    int                               rc = PCS_OK;      // of the construction: the caller returns it if non-zero

    explicit KernelTimer(pcs_ctx* ctx) : c(ctx) { if (c->kernel_timing) rc = start(); }
    KernelTimer(const KernelTimer&) = delete;
    KernelTimer& operator=(const KernelTimer&) = delete;
    ~KernelTimer()
    {
        if (!open) return;
        try { c->ev_free.push_back(ev); } catch (...) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    }
    int finish()
    {
        if (!open) return PCS_OK;
        HIPCHK(c, hipEventRecord(ev.second, c->stream));
        c->ev_pool.push_back(ev);
        open = false;
        return PCS_OK;
    }

private:
    int start()
    {
        const int r = acquire_event_pair(c, ev);
        if (r) return r;
        open = true;
        HIPCHK(c, hipEventRecord(ev.first, c->stream));
        return PCS_OK;
    }
};

// One launch inside one bracket: the four lines every per-launch bracket is. Returns from the calling function on every failure, as
// HIPCHK does (whose message names the launch as written); the timer's destructor hands the pair back then.
#define PCS_TIMED(c, launch)                              \
    do {                                                  \
        pcs_host::KernelTimer _timer(c);                  \
        if (_timer.rc) return _timer.rc;                  \
        HIPCHK((c), launch);                              \
        if (int _rc = _timer.finish()) return _rc;        \
    } while (0)

// ---- the payload-cloud family (radius / statistical outlier removal, surface normals, alignment): pcs_capi_cloud.cpp -------------
constexpr int kMaxPoints = INT_MAX / PCS_POINT_BYTES;      // a payload's byte count fits an int32 (as the PCZ1 container's)

// [a, a + na) and [b, b + nb) share a byte. A NULL pointer is no range: it shares none, whatever length rides beside it.
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// The first output range, in table order, that shares a byte with an input (*with = nullptr) or with an earlier output (*with).
struct NamedRange { const void* p; size_t n; const char* name; };
inline const NamedRange* first_overlap(const NamedRange* outs, size_t n_outs, const NamedRange* ins, size_t n_ins, const NamedRange** with)
{
    for (size_t i = 0; i < n_outs; i++) {
        *with = nullptr;
        for (size_t k = 0; k < n_ins; k++)
            if (ranges_overlap(outs[i].p, outs[i].n, ins[k].p, ins[k].n)) return &outs[i];
        for (size_t j = 0; j < i; j++)
            if (ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) { *with = &outs[j]; return &outs[i]; }
    }
    return nullptr;
}

// What a filter of packed records checks about its payloads once its own parameters passed: the count's range, NULLs, 2-byte
// alignment, the count word's alignment, out_shorts against the worst case, and that nothing overlaps. `who` names the entry point,
// the *_name its own argument names; stats (optional, 8-byte aligned, stats_bytes long) may be NULL.
int check_payload_io(pcs_ctx* c, const char* who, const void* in, const char* in_name, int n_points, const char* n_name, const void* out,
                     const char* out_name, size_t out_shorts, const void* out_points, const char* points_name, unsigned points_align,
                     const void* stats = nullptr, const char* stats_name = nullptr, size_t stats_bytes = 0);

// The kIndexStages launches of the cell index over n > 0 records, cell edge cell_mm, one timing bracket each; its view into *view.
int build_cell_index(pcs_ctx* c, const int16_t* d_payload, int n, int cell_mm, void* index, size_t index_bytes, OutlierIndexView* view);

// The host forms' payload staging (pcs_voxel_grid's: every such call is synchronous, none leaves anything in it): s_voxel_in sized and
// filled with in_bytes of `in` on the stream, s_voxel_out sized for out_bytes.
int stage_payload(pcs_ctx* c, const void* in, size_t in_bytes, size_t out_bytes);
// bytes from the device once the stream has run dry / the count word the kernels left in d_counts[0], refused outside 0..n_points
// ("the kernels reported %d of %d records <what>").
int fetch(pcs_ctx* c, void* dst, const void* d_src, size_t bytes);
int fetch_count(pcs_ctx* c, const char* who, int n_points, const char* what, int32_t* count);

// What the streams [s0, s0 + nl) of one launch have in common: the AND of their certificates, the OR of their distortions, the largest
// raster. Every launch site of the fused path takes its arithmetic from this one fold (launch_math) and states its own reduction.
struct LaunchTraits {
    uint32_t max_points = 0, max_w = 0, max_h = 0;
    bool     fast = true, ident = true, noovf = true;     // every stream: cert_fast / ident_r / no_overflow
    bool     any_ddist = false, any_cdist = false;        // (cdist: or the half-pixel texture convention, which runs on the CDIST path)
    bool     row_const = true;          // every stream has ident_r == 2: the colour-row table the voxel reader uses (CertRowConst)
    bool     row_const_tile = true;     // ... its raster rows whole 8-pixel runs, its colour raster 16 bytes or more: the dense tile
};
inline LaunchTraits launch_traits(const pcs_ctx* c, int s0, int nl)
{
    LaunchTraits t;
    for (int s = s0; s < s0 + nl; s++) {
        const StreamParams& q = c->h_params[s];
        t.max_points = std::max(t.max_points, q.n_points);
        t.max_w = std::max(t.max_w, (uint32_t)q.W); t.max_h = std::max(t.max_h, q.n_points / (uint32_t)q.W);
        t.fast &= q.cert_fast != 0; t.ident &= q.ident_r != 0; t.noovf &= q.no_overflow != 0;
        t.any_ddist |= q.ddist != 0;
        t.any_cdist |= q.cdist != 0 || q.tex_half != 0;
        t.row_const &= q.ident_r == 2;
        t.row_const_tile &= q.ident_r == 2 && (q.W & 7) == 0 && q.color_bytes >= 16;
    }
    return t;
}
inline MathSel launch_math(const LaunchTraits& t)
{
    return !t.fast ? MathSel::Ieee
         : t.noovf ? (t.ident ? MathSel::CertIdentRNoOvf : MathSel::CertNoOvf)
                   : (t.ident ? MathSel::CertIdentR : MathSel::Cert);
}

// The raster pointers of streams [s0, s0 + nl) as one launch takes them / of frame-sets [k0, k0 + nk) as a K-set launch does.
inline FramePtrs frame_ptrs(const uint16_t* const* d_depth, const uint8_t* const* d_color, int s0, int nl)
{
    FramePtrs fp{};
    for (int k = 0; k < nl; k++) { fp.depth[k] = d_depth[s0 + k]; fp.color[k] = d_color[s0 + k]; }
    return fp;
}
inline BatchPtrs batch_ptrs(int S, const uint16_t* const* d_depth, const uint8_t* const* d_color, int16_t* const* d_payload, int k0, int nk)
{
    BatchPtrs bp{};
    for (int k = 0; k < nk; k++) {
        bp.payload[k] = reinterpret_cast<uint8_t*>(d_payload[k0 + k]);
        for (int s = 0; s < S; s++) {
            bp.depth[k * S + s] = d_depth[(size_t)(k0 + k) * S + s];
            bp.color[k * S + s] = d_color[(size_t)(k0 + k) * S + s];
        }
    }
    return bp;
}

// The per-stream raster pointer arrays of an entry point (n_sets frame-sets, entry k * n_streams + s): none NULL, and every depth
// raster 2-byte aligned where a kernel reads it. A batch call's messages name the frame-set too. (Colour: whatever rides beside.)
template <class Color>
int check_rasters(pcs_ctx* c, const uint16_t* const* depth, Color* const* color, bool need_depth_alignment, int n_sets = 1,
                  bool name_set = false)
{
    for (int k = 0; k < n_sets; k++)
        for (int s = 0; s < c->n_streams; s++) {
            const size_t i = (size_t)k * c->n_streams + s;
            const char* what = (!depth[i] || !color[i]) ? "NULL raster pointer"
                             : (need_depth_alignment && ((uintptr_t)depth[i] & 1u)) ? "depth pointer not 2-byte aligned" : nullptr;
            if (!what) continue;
            return name_set ? fail(c, PCS_ERR_INVALID_ARG, "frame-set %d stream %d: %s", k, s, what)
                            : fail(c, PCS_ERR_INVALID_ARG, "stream %d: %s", s, what);
        }
    return PCS_OK;
}

// The fused path for device-resident rasters. Counts end up in d_counts (if non-null).
int run_fused_device(pcs_ctx* c, const uint16_t* const* d_depth, const uint8_t* const* d_color, int16_t* d_payload, size_t payload_shorts,
                     int32_t* d_counts, bool force_three_pass = false, const uint32_t* d_tile_kept = nullptr);

}  // namespace pcs_host

#endif
