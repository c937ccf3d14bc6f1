// pcs_device.h — structures shared by the HIP kernels (pcs_kernels.hip, pcs_kernels_voxel.hip, pcs_kernels_filter.hip, pcs_voxel.hip) and the C-ABI host layer
// (pcs_capi.cpp). Internal; the public surface is include/pcs_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcs_hip.h"
#include "pcs_plan_math.h"

namespace pcs {

// Geometry of one launch tile: a 256-thread workgroup owns 2048 consecutive points of one stream,
// 8 consecutive points per lane, 512 per wavefront.
constexpr int      kBlockThreads   = 256;
constexpr int      kPointsPerLane  = 8;
constexpr uint32_t kTilePoints     = kBlockThreads * kPointsPerLane;   // 2048
constexpr int      kLaunchStreams  = 16;                               // streams per launch (blockIdx.y)

// Per-stream constants. One table entry per camera, uploaded at pcs_create / pcs_set_cam_to_world.
// Every field is wave-uniform (indexed by blockIdx.y), so the kernels read them with scalar loads
// and they live in SGPRs — the CDNA counterpart of the reference's broadcast __m128 globals
// (src/pcs-camera-optimized.cpp:69-72, 390-408).
struct alignas(16) StreamParams {
    float    M[12];          // top three rows of cam_to_world (tf_mat), row-major
    float    R[9];           // depth->colour rotation, column-major (rs2_extrinsics)
    float    t[3];           // depth->colour translation
    float    depth_scale;
    float    d_ppx, d_ppy, d_fx, d_fy;
    float    c_fx, c_fy, c_ppx, c_ppy;
    float    c_w_f, c_h_f;   // (float)colour width / height
    float    c_wm1_f, c_hm1_f; // (float)(colour width - 1) / (height - 1)
    float    c_rw, c_rh;     // RN(1/c_w_f), RN(1/c_h_f) — for the verified constant-divisor quotient
    float    dk[5];          // depth distortion coefficients
    float    ck[5];          // colour distortion coefficients
    int32_t  W, H;           // depth raster
    int32_t  cW, cH;         // colour raster
    int32_t  bpp, stride;    // colour bytes per pixel / per row
    uint32_t color_bytes;    // stride * cH
    uint32_t n_points;       // W * H
    int32_t  ddist, cdist;   // distortion active (non-zero coefficients)
    uint32_t out_base;       // first output point of this stream in the stitched payload when no
                             // predicate is active: sum over earlier streams of ceil(n/downsample)
    uint32_t tile_base;      // index of this stream's first tile in the per-tile count arrays
    uint32_t w_magic, w_shift; // floor(i / W) == umulhi(i, w_magic) >> w_shift for i < 2^31 (0 = use '/')
    int32_t  cert_fast;      // host+device certified for CertMath (see pcs_capi.cpp)
    int32_t  ident_r;        // depth->colour rotation is exactly I, translation has no -0; 2: and the colour ROW of a pixel is certified
                             // independent of its depth value — my[H .. 2H) holds the row of every raster row (CertRowConst)
    int32_t  no_overflow;    // certified: no converted value (world mm, colour column/row) can reach 2^31
    int32_t  z_zero_iff_d_zero; // depth_scale finite and depth_scale*1 != 0: (z == 0) == (d == 0)
    uint32_t cut_dmax;       // -c from the Z16 word alone: in range <=> 1 <= d <= cut_dmax (0 = not certified, deproject)
    int32_t  tex_half;       // PCS_FLAG_TEXCOORD_HALF_PIXEL: u = (px + 0.5)/W (handled on the CDIST code path)
    const float* mx;         // [W]  (c - ppx) / fx   — IEEE division done once on the host
    const float* my;         // [H]  (r - ppy) / fy; behind it [H] int32: the colour row of raster row r (valid when ident_r == 2),
                             // then int32 {kx, bx_lo, bx_hi}: the dense kernel's colour window (pcs_capi.cpp: color_window_params)
};

// Per-call raster pointers, passed by value in the kernarg segment (no per-frame H2D of a table).
struct FramePtrs {
    const uint16_t* depth[kLaunchStreams];
    const uint8_t*  color[kLaunchStreams];
};

struct VertexPtrs {          // a2 twin: one stream per launch
    const float*   vertices;   // n x {x,y,z}
    const float*   texcoords;  // n x {u,v}
    const uint8_t* color;
    uint32_t       n_points;
};

// Batched dense launch: K frame-sets of the same S streams in ONE launch (blockIdx.z = frame-set). A 23 us
// launch spends a large share of its life filling and draining the machine; K sets per launch amortise that
// (throughput form, pcs_process_frames_device_batch). Entry z*S + y holds the rasters of stream y in set z.
constexpr int kBatchEntries = 64;                                      // S * K <= 64
constexpr int kBatchSets    = 16;
struct BatchPtrs {
    const uint16_t* depth[kBatchEntries];
    const uint8_t*  color[kBatchEntries];
    uint8_t*        payload[kBatchSets];                               // payload base of frame-set z
};
// Where the per-stream counts [S] and the total [S] of frame-set z go (batched compaction).
struct BatchCounts {
    int32_t* counts[kBatchSets];
};

// Batched a2 twin: several cameras' rs2::points arrays in ONE launch (blockIdx.y = cloud).
constexpr int kPackBatch = 16;
struct PackBatch {
    VertexPtrs v[kPackBatch];
    uint8_t*   out[kPackBatch];
    int32_t    stream[kPackBatch];                                     // which StreamParams entry (extrinsic, colour geometry)
};

// Which arithmetic policy a launch may use (the AND over the streams of the launch).
enum class MathSel { Ieee = 0, Cert = 1, CertIdentR = 2, CertNoOvf = 3, CertIdentRNoOvf = 4,
                     CertRowConst = 5 /* voxel reader only: CertIdentR + the colour row from a per-row table (ident_r == 2) */,
                     CertRowConstNoOvf = 6 /* dense kernel only: CertIdentRNoOvf + the row table + the colour window */ };

// Launchers (defined in pcs_kernels.hip). All enqueue on `st` and return the hipError of the launch.
hipError_t launch_fused_dense(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                              bool any_ddist, bool any_cdist, MathSel math, const FramePtrs& fp, int16_t* d_payload,
                              hipStream_t st);

// Generic path: predicate / downsample / unaligned payload / W % 8 != 0.
//   d_tile_counts, d_tile_prefix : one uint32 per tile of every stream (StreamParams::tile_base indexes them)
//   d_stream_kept                : n_total_streams uint32 (kept points per stream, before the stride)
//   d_arrive                     : nullptr for the fused path (the per-stream counts come from the scan, the grand total
//                                  from the first emit launch: d_total_out); the a2 twin's launch_pack_scan passes one
//                                  zero-initialised uint32 (arrival counter, self-resetting) and gets the total from the scan
//   d_counts (optional)          : n_total_streams + 1 int32 handed back to the caller
// launch_pack_scan: d_out_points receives 2 int32 (kept, total)
hipError_t launch_fused_count(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                              uint32_t flags, const FramePtrs& fp, uint32_t* d_tile_counts, hipStream_t st);
hipError_t launch_scan(const StreamParams* d_params, int n_streams, int downsample,
                       const uint32_t* d_tile_counts, uint32_t* d_tile_prefix, uint32_t* d_stream_kept,
                       int32_t* d_counts, uint32_t* d_arrive, hipStream_t st);
hipError_t launch_fused_emit(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                             uint32_t flags, int downsample, MathSel math, const FramePtrs& fp,
                             const uint32_t* d_tile_prefix, const uint32_t* d_stream_kept,
                             int16_t* d_payload, int32_t* d_total_out, int n_total_streams, hipStream_t st);
// Single-pass ordered compaction (predicate, stride 1). See pcs_fused_compact_kernel.
struct CompactLaunch {
    unsigned long long* d_ticket;       // device counter, never reset
    unsigned long long  ticket_base;    // tickets issued before this launch
    uint64_t*           d_desc;         // launch_tiles descriptors
    uint64_t*           d_stream_desc;  // all streams: per-stream totals
    uint32_t*           d_stream_end;   // all streams
    const uint32_t*     d_chain_in;     // total of earlier launches of the same frame-set, or nullptr
    uint32_t*           d_error;
    uint32_t            gen;
    uint32_t            flags;
    int32_t*            d_counts;       // n_total + 1 ints: per-stream kept counts and the total (written by the kernel)
    int32_t             n_total;        // streams of the whole frame-set
    int32_t             last_launch;    // this launch holds the frame-set's last stream
};
hipError_t launch_fused_compact(const StreamParams* d_params, int stream0, int n_launch, uint32_t launch_tiles,
                                MathSel math, const FramePtrs& fp, const CompactLaunch& cl, int16_t* d_payload,
                                hipStream_t st);

// K frame-sets per launch (dense path only).
hipError_t launch_fused_dense_batch(const StreamParams* d_params, int n_streams, int n_sets, uint32_t max_points,
                                    bool any_ddist, bool any_cdist, MathSel math, const BatchPtrs& bp, hipStream_t st);
// K frame-sets per launch, ordered compaction (stride 1): count, scan and emit each cover all K sets.
// d_tile_counts / d_tile_prefix hold n_sets * total_tiles words, d_stream_kept n_sets * n_streams.
hipError_t launch_compact_batch(const StreamParams* d_params, int n_streams, int n_sets, uint32_t max_points,
                                uint32_t total_tiles, uint32_t flags, MathSel math, const BatchPtrs& bp,
                                const BatchCounts& bc, uint32_t* d_tile_counts, uint32_t* d_tile_prefix,
                                uint32_t* d_stream_kept, hipStream_t st);
hipError_t launch_verify_div_const(float c, float rc, int32_t dim, unsigned long long* d_bad, hipStream_t st);
// CertRowConst's certificate for one stream of an uploaded parameter table: d_crow[rows] = colour row of every raster row at depth 1,
// *d_bad += (row, depth) pairs over all 65 535 depth values whose row differs (pcs_kernels.hip)
hipError_t launch_certify_color_row(const StreamParams* d_params, int stream, int rows, int32_t* d_crow, unsigned long long* d_bad, hipStream_t st);

// a2 twin.
hipError_t launch_pack_dense(const StreamParams* d_params, int stream, const VertexPtrs& vp,
                             int16_t* d_out, hipStream_t st);
hipError_t launch_pack_count(const StreamParams* d_params, int stream, const VertexPtrs& vp, uint32_t flags,
                             uint32_t* d_tile_counts, hipStream_t st);
hipError_t launch_pack_scan(uint32_t n_tiles, const uint32_t* d_tile_counts, uint32_t* d_tile_prefix,
                            int32_t* d_out_points, uint32_t* d_arrive, hipStream_t st);
hipError_t launch_pack_emit(const StreamParams* d_params, int stream, const VertexPtrs& vp, uint32_t flags,
                            const uint32_t* d_tile_prefix, int16_t* d_out, hipStream_t st);

// batched a2 twin (no predicate): n clouds in one launch; `aligned` = every out pointer is 16-byte aligned
hipError_t launch_pack_batch(const StreamParams* d_params, const PackBatch& pb, int n, uint32_t max_points, bool aligned,
                             hipStream_t st);

// a3, PCS_FLAG_SCALAR_ARITH (the reference's default arithmetic). The fused launch: `dense` as for launch_fused_dense (stride 1,
// 16-byte aligned payload, every stream a multiple of 8 points), otherwise the general form; `cut`: a point a3's -c loop skips gives
// the zero record. Counts are the configuration's (nothing is compacted). The a2 twin: n clouds in one launch without -c; with it,
// one cloud whose skipped slots keep the bytes of d_out.
hipError_t launch_fused_scalar(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points, bool dense, bool cut,
                               int downsample, MathSel math, const FramePtrs& fp, int16_t* d_payload, hipStream_t st);
hipError_t launch_pack_scalar(const StreamParams* d_params, const PackBatch& pb, int n, uint32_t max_points, bool aligned,
                              hipStream_t st);
hipError_t launch_pack_scalar_cut(const StreamParams* d_params, int stream, const VertexPtrs& vp, int16_t* d_out, hipStream_t st);

// Crop box (pcs_set_crop_box_mm): the box as the three dwords the kernels take (pcs_kernels_common.h: CropBox) —
// w[0] = lo_x | lo_y << 16, w[1] = lo_z | span_z << 16, w[2] = span_x | span_y << 16, span = hi - lo. Always count + scan + emit
// (launch_scan is the existing one); `math` is the emit launch's policy, whose conversion ladder the count pass shares.
// PCS_KFLAG_CROP_BOX: an internal bit of a context's flag word (never accepted from pcs_config.flags): a box is set.
constexpr uint32_t PCS_KFLAG_CROP_BOX = 0x40000000u;
struct CropBoxArg { uint32_t w[3]; };
inline CropBoxArg crop_box_arg(const int16_t lo[3], const int16_t hi[3])
{
    const uint32_t l[3] = {(uint16_t)lo[0], (uint16_t)lo[1], (uint16_t)lo[2]};
    const uint32_t sp[3] = {(uint32_t)(hi[0] - lo[0]), (uint32_t)(hi[1] - lo[1]), (uint32_t)(hi[2] - lo[2])};
    return CropBoxArg{{l[0] | l[1] << 16, l[2] | sp[2] << 16, sp[0] | sp[1] << 16}};
}
hipError_t launch_fused_count_crop(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points, uint32_t flags,
                                   const CropBoxArg& box, const FramePtrs& fp, uint32_t* d_tile_counts, hipStream_t st);
hipError_t launch_fused_emit_crop(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points, uint32_t flags,
                                  const CropBoxArg& box, int downsample, MathSel math, const FramePtrs& fp, const uint32_t* d_tile_prefix,
                                  const uint32_t* d_stream_kept, int16_t* d_payload, int32_t* d_total_out, int n_total_streams,
                                  hipStream_t st);
// K frame-sets (stride 1): count, scan, emit each cover all of them, as launch_compact_batch.
hipError_t launch_crop_batch(const StreamParams* d_params, int n_streams, int n_sets, uint32_t max_points, uint32_t total_tiles,
                             uint32_t flags, const CropBoxArg& box, MathSel math, const BatchPtrs& bp, const BatchCounts& bc,
                             uint32_t* d_tile_counts, uint32_t* d_tile_prefix, uint32_t* d_stream_kept, hipStream_t st);
// Centre side (pcs_crop_payloads_device): n_cams <= PCS_MAX_STREAMS packed payloads -> one stitched payload. d_tab: n_cams table
// entries (filled here, on the stream); d_tile_counts / d_tile_prefix: one word per input tile; d_cam_kept: n_cams; d_counts: n_cams + 1.
hipError_t launch_crop_payloads(StreamParams* d_tab, const int16_t* const* d_in, const uint32_t* n_points, int n_cams,
                                const CropBoxArg& box, int downsample, uint32_t* d_tile_counts, uint32_t* d_tile_prefix,
                                uint32_t* d_cam_kept, int16_t* d_out, int32_t* d_counts, hipStream_t st);

// a5 alone.
hipError_t launch_deproject(const StreamParams* d_params, int stream, uint32_t n_points, const uint16_t* d_depth,
                            float* d_vertices, float* d_texcoords, hipStream_t st);

// Voxel-grid downsample (pcs_voxel.hip).
struct VoxelWsState;
size_t     voxel_workspace_bytes(uint32_t n_points, int level = 2);      // level: voxel_workspace_level (0 LSD .. 2 warm bucket)
int        voxel_workspace_level(uint32_t n_points, int leaf_mm, const VoxelWsState& ws, bool from_partials);
// What the owner of a voxel workspace keeps between calls (pcs_voxel.hip: plan_for): which of the workspace's two control
// blocks the next call uses, and whether both are known to be in the state that call expects.
struct VoxelWsState {
    const void* base = nullptr;
    uint32_t    phase = 0;
    bool        clean = false;
    int         spl_leaf = 0;       // bucket tail: the leaf the workspace's splitters were made for (0: none)
    uint32_t    bkt_calls = 0;      // bucket-tail calls enqueued on this workspace (tags their published counts)
    int         tail_pref = 0;      // pcs_set_voxel_tail: 0 by the leaf, 1 bucket, 2 LSD (the environment overrides)
    bool        stalled = false;    // a bucket-tail call of this owner ended flagged (-1): LSD from here on, whatever the environment says
};
hipError_t launch_voxel_grid(const int16_t* d_payload, uint32_t n_points, const int32_t* d_n_points, int leaf_mm, void* d_ws,
                             size_t ws_bytes, VoxelWsState* ws, int16_t* d_out, int32_t* d_out_points, hipStream_t st);

// The same pipeline fed from the rasters (pcs_process_frames_voxel_device): voxel_begin carves the workspace and clears
// the counters, launch_fused_voxel_partials (pcs_kernels_voxel.hip) appends the partials, voxel_finish sorts and reduces.
struct VoxelStage {
    unsigned long long* keys;
    unsigned int*       idx;           // nullptr with idx_bits == 0: raw keys only (exchange format)
    void*               part;          // VoxelPartial[capacity]
    unsigned int*       n_runs;        // partials appended so far
    uint32_t            leaf, bits, idx_bits;
    float               div_inv, div_c;   // voxel index of a coordinate: (unsigned)fmaf(v, div_inv, div_c) (pcs_voxel_agg.h: VoxelDiv)
    uint32_t            track_bits;    // record which key bits vary (the sort may then skip a pass); 0: the host declared all of them varying
    // Warm bucket tail (pcs_voxel.hip, "regions"): the workgroup finds each partial's bucket itself (the previous call's splitters)
    // and appends it to that bucket's REGION — reg[0] buckets of reg[1] slots each, filled through cursor[bucket] — so the
    // partition kernels (histogram, column scan, scatter) are not launched. A partial whose region is full goes to keys / part as
    // before, with its bucket id in bucket_of: the tail's first workgroup sorts those few in.
    uint32_t                  regions;       // 0: every partial to keys / part
    uint32_t                  region_slots;  // capacity of keys_r / part_r (a call whose reg[] asks for more uses no regions)
    const unsigned long long* spl;           // kVoxBuckets - 1 ascending splitters (+ one unused word)
    const unsigned int*       reg;           // {buckets in use, slots per region}: written by the previous call's tail
    unsigned int*             cursor;        // [kVoxBuckets] partials offered to each bucket so far (zero at launch)
    unsigned long long*       keys_r;
    void*                     part_r;
    unsigned short*           bucket_of;
};
hipError_t voxel_begin(uint32_t capacity_points, int leaf_mm, void* d_ws, size_t ws_bytes, VoxelWsState* ws, VoxelStage* stage,
                       hipStream_t st);
hipError_t voxel_finish(uint32_t capacity_points, int leaf_mm, void* d_ws, size_t ws_bytes, VoxelWsState* ws, int16_t* d_out,
                        int32_t* d_out_points, hipStream_t st);
// Partials as an exchange format (multi-GPU config 5): a stage that appends (raw voxel key, sums) to caller arrays
// (d_count: one word = partials appended), and the sort + segmented mean over caller-held partials from any number of
// such stages (same leaf).
hipError_t voxel_partials_stage(int leaf_mm, unsigned long long* d_keys, void* d_partials, unsigned int* d_count, VoxelStage* stage,
                                hipStream_t st);
hipError_t launch_voxel_from_partials(const unsigned long long* d_keys, const void* d_partials, uint32_t n_partials,
                                      const int32_t* d_n_partials, int leaf_mm, void* d_ws, size_t ws_bytes, VoxelWsState* ws,
                                      int16_t* d_out, int32_t* d_out_points, hipStream_t st);
// fault injection: the next `launches` bucket-tail launches end flagged (*out_points = -1), as after a stalled workgroup
void inject_voxel_stall(int launches);
// the same table fed from a 16-byte aligned payload (pcs_kernels_voxel.hip; the unaligned forms stay in pcs_voxel.hip)
hipError_t launch_payload_voxel_partials(const int16_t* d_payload, uint32_t n_points, const int32_t* d_n_points,
                                         const VoxelStage& vs, hipStream_t st);
// max_w / max_h: the largest raster of the launch; patch_ok: every raster's width is a multiple of 8 (square patches)
hipError_t launch_fused_voxel_partials(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                                       uint32_t max_w, uint32_t max_h, bool patch_ok, bool any_dist, uint32_t flags,
                                       MathSel math, const FramePtrs& fp, const VoxelStage& vs, hipStream_t st);

// Centre-side re-transform of already packed payloads (src/pcs-multicamera-optimized.cpp:226-265, 289): n clouds in one launch
// (blockIdx.y = cloud), each decoded, moved by its own 3x4 and re-packed at its camera-order offset of one stitched payload.
constexpr int kXformBatch = 16;
struct XformCloud {
    const int16_t* in;          // the camera's payload as received
    uint8_t*       out;         // where its first kept record goes
    uint32_t       n_out;       // records written = floor(n_in / ds): the decoded cloud's width (:230)
    uint32_t       ds;          // keep every ds-th record (i % downsample == 0, :236)
    float          M[12];       // top three rows of transform[i], row-major
};
struct XformBatch { XformCloud c[kXformBatch]; };
hipError_t launch_transform_payloads(const XformBatch& xb, int n, uint32_t max_out, hipStream_t st);

// Depth pre-filter (pcs_set_depth_filter, pcs_kernels_filter.hip): temporal smoothing and fill-from-left, Z16 -> Z16, every stream of
// a context in one launch (blockIdx.y = stream). The table lives in device memory (one entry per stream, uploaded when the filter is
// set); the per-call raster pointers travel in the kernel's arguments.
struct FilterStream {
    uint16_t* last;          // [n_points] the temporal stage's previous output (nullptr: hole fill alone, no state)
    uint8_t*  hist;          // [n_points] validity shift register, bit 0 = the most recent frame
    uint32_t  W, H;          // depth raster
    uint32_t  tile_base;     // as StreamParams::tile_base
    uint32_t  pad;
};
struct FilterPtrs {
    const uint16_t* in[PCS_MAX_STREAMS];
    uint16_t*       out[PCS_MAX_STREAMS];      // out[s] == in[s] is allowed
};
struct FilterArgs {
    float    a, oma;         // (float)alpha and 1.0f - a, each rounded once on the host
    int32_t  delta;
    uint32_t l_mask;         // (1 << L) - 1 of the persistence rule "valid in M of the last L"
    int32_t  m;
};
// A workgroup owns one row of one stream; its tile counts are gathered in kFilterSlots LDS words, so W <= kFilterRowPixels for every
// stream (pcs_set_depth_filter refuses wider rows). max_rows / max_width: the tallest and the widest raster of the launch.
constexpr int      kFilterSlots     = 64;
constexpr uint32_t kFilterRowPixels = (kFilterSlots - 2) * kTilePoints;
hipError_t launch_depth_filter(const FilterStream* d_tab, int n_streams, uint32_t max_rows, uint32_t max_width, bool temporal,
                               bool fill, const FilterPtrs& fp, const FilterArgs& fa, uint32_t* d_tile_kept, hipStream_t st);

// Depth decimation (pcs_decimate_depth_device, pcs_kernels_filter.hip): every scale x scale block of a Z16 raster to one pixel, the
// lower median of its non-zero values (scale 2, 3) or their truncated mean (4..8); every stream of a context in one launch
// (blockIdx.y = stream). The call is stateless and the source sizes are the caller's, per call: the per-stream table travels in the
// kernel's arguments with the raster pointers (1792 bytes), so nothing is uploaded and nothing in the context can go stale.
struct DecimArgs {
    const uint16_t* in[PCS_MAX_STREAMS];       // source raster, Ws pixels per row
    uint16_t*       out[PCS_MAX_STREAMS];      // Wd x Hd, tightly packed
    uint32_t        Ws[PCS_MAX_STREAMS];       // source row pitch in pixels (columns >= scale * Wd are never read)
    uint32_t        Wd[PCS_MAX_STREAMS], Hd[PCS_MAX_STREAMS];
};
// max_rows / max_width: the tallest and the widest OUTPUT raster of the launch. scale outside 2..8 is hipErrorInvalidValue.
hipError_t launch_decimate_depth(int scale, int n_streams, uint32_t max_rows, uint32_t max_width, const DecimArgs& da, hipStream_t st);

// Spatial filter (pcs_spatial_filter_depth_device, pcs_kernels_filter.hip): the edge-preserving recurrence along every row (both
// directions, with the bounded hole fill) and then along every column (both directions), `iterations` times: 2 x iterations launches,
// each over every stream of a context (blockIdx.y = stream), one lane per line. The first row launch reads in[] and writes out[];
// every later launch runs in place on out[] (in[s] == out[s] is allowed). Stateless, like the decimation: the per-call table travels in
// the kernels' arguments (1552 bytes), nothing is uploaded, nothing is stored in the context.
struct SpatialArgs {
    const uint16_t* in[PCS_MAX_STREAMS];
    uint16_t*       out[PCS_MAX_STREAMS];
    uint32_t        W[PCS_MAX_STREAMS], H[PCS_MAX_STREAMS];
    float           a, oma;                    // (float)alpha and 1.0f - a, each rounded once on the host
    float           delta;                     // 1..65535, exact in fp32: the recurrence compares in floats
    uint32_t        radius;                    // hole_radius: pixels filled per gap and direction in the row passes (0: none)
};
// max_rows / max_width: the tallest and the widest raster of the launch. iterations < 1 is hipErrorInvalidValue.
hipError_t launch_spatial_filter(int n_streams, int iterations, uint32_t max_rows, uint32_t max_width, const SpatialArgs& sa, hipStream_t st);

// Payload codec (pcs_compress_payload_device / pcs_decompress_payload_device, pcs_kernels_codec.hip): the "PCZ1" container of
// DESIGN.md section 4, 64 records per block, one wavefront per block. Encode is three launches — count (every block's byte size
// into d_sizes[ceil(n / 64)]), offsets (ONE workgroup scans the sizes, kCodecScanBlocks per pass, and writes block_end[], the
// container header and, if non-NULL, *d_out_bytes) and emit — and writes at most 16 + 660 ceil(n / 64) bytes; with n == 0 only the
// offsets launch runs (a 16-byte container). Decode is one launch; it reads nothing at or beyond in_bytes and writes nothing at or
// beyond record n_points whatever the bytes say (16 + 4 ceil(n / 64) > in_bytes is hipErrorInvalidValue, nothing launched).
// Payload and container pointers are 4-byte aligned.
constexpr uint32_t kCodecScanBlocks = 1024;
hipError_t launch_codec_encode(const int16_t* d_payload, uint32_t n_points, uint32_t* d_sizes, void* d_out, uint32_t* d_out_bytes,
                               hipStream_t st);
hipError_t launch_codec_decode(const void* d_in, uint32_t in_bytes, uint32_t n_points, int16_t* d_payload, hipStream_t st);

// 256-byte granularity: how every workspace slab of the payload-cloud family is carved, on the host and in the launchers alike
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Radius outlier removal (pcs_radius_outlier_device, pcs_kernels_outlier.hip): kOutlierStages launches on one stream, each its own
// call so that the host layer can bracket them one by one (pcs_kernel_timing). `capacity` (n_points, or max_points of the counted
// form) sizes every grid and the workspace; the record count the kernels use is n_points, or *d_n_points clamped to 0..capacity when
// that pointer is given — read by stage 0, on the device. d_ws: outlier_workspace_bytes(capacity) bytes, 256-byte aligned. Stage 8
// is launch_scan over the control block's one-entry table: it writes the kept count to d_out_points[0].
// The stages are three groups, each with an entry point of its own for the callers that want only that group: 0 to 5 build the cell
// index (launch_cell_index_stage: no filter parameter), 6 is this filter's flag, 7 to 9 compact by the keep bits
// (launch_outlier_compact_stage, the filter's numbering). launch_outlier_stage runs any of the ten and forwards the two groups.
constexpr int kOutlierStages = 10;
constexpr int kIndexStages   = 6;
struct OutlierCtl { StreamParams tab; };     // entry 0 of a scan table: n_points = the record count, tile_base = 0
uint32_t    outlier_slots(uint32_t capacity);
size_t      outlier_workspace_bytes(uint32_t capacity);
const char* outlier_stage_name(int stage);
hipError_t  launch_cell_index_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                    int cell_mm, void* d_ws, size_t ws_bytes, hipStream_t st);
hipError_t  launch_outlier_compact_stage(int stage, const int16_t* d_in, uint32_t capacity, void* d_ws, size_t ws_bytes, int16_t* d_out,
                                         int32_t* d_out_points, hipStream_t st);
hipError_t  launch_outlier_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                 int radius_mm, int min_neighbors, void* d_ws, size_t ws_bytes, int16_t* d_out, int32_t* d_out_points,
                                 hipStream_t st);
// What the kIndexStages launches of launch_cell_index_stage leave in a workspace, for a reader other than the flag kernel
// (pcs_kernels_align.hip, pcs_kernels_normals.hip, pcs_kernels_stat.hip): cell key of slot s in keys[s] (all ones: empty; probe from
// first_slot, pcs_outlier_index.h), the cell's members at xyz[start[s] .. start[s + 1]) (x | y << 16, z), slots + 1 starts. Nothing
// is launched.
struct OutlierIndexView {
    const unsigned long long* keys;
    const uint32_t*           start;
    const uint2*              xyz;
    uint32_t                  slots, capacity;
};
hipError_t  outlier_index_view(uint32_t capacity, void* d_ws, size_t ws_bytes, OutlierIndexView* view);
// What stage 0 leaves and launch_outlier_compact_stage reads, for a flag kernel other than the radius filter's (pcs_kernels_stat.hip):
// the control block (the record count) and keep_bits[w] = the keep bits of records 64 w .. 64 w + 63, a bit at or beyond the count 0;
// tile_prefix[t] = what the tile scan leaves: the kept records in front of tile t (pcs_kernels_plane.hip moves its origin indices by it).
struct OutlierKeepView {
    const OutlierCtl*   ctl;
    unsigned long long* keep_bits;
    const uint32_t*     tile_prefix;
};
hipError_t  outlier_keep_view(uint32_t capacity, void* d_ws, size_t ws_bytes, OutlierKeepView* view);

// Statistical outlier removal (pcs_stat_outlier_device, pcs_kernels_stat.hip; the definition: DESIGN.md section 3 "Statistical
// outlier removal"): kStatStages launches on one stream, each its own call as launch_outlier_stage's are. Stages 0 to 5 are the cell
// index with cell edge max_dist_mm (launch_cell_index_stage), 6 to 9 knn, sums, threshold and flag, 10 to 12 the radius filter's tile
// count, tile scan and emit (launch_outlier_compact_stage), 13 (only with d_stats: eight int64, 8-byte aligned) the statistics block. d_ws: stat_workspace_bytes(capacity) bytes,
// 256-byte aligned; count and capacity as launch_outlier_stage's.
constexpr int kStatStages = 14;
size_t      stat_workspace_bytes(uint32_t capacity);
const char* stat_stage_name(int stage);
hipError_t  launch_stat_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity, int mean_k,
                              int std_mul_milli, int max_dist_mm, void* d_ws, size_t ws_bytes, int16_t* d_out, int32_t* d_out_points,
                              long long* d_stats, hipStream_t st);

// Euclidean clusters (pcs_cluster_filter_device, pcs_cluster_labels_device, pcs_kernels_cluster.hip; the definition: DESIGN.md section 3
// "Euclidean clusters"): each launch its own call as launch_outlier_stage's are. The filter form runs stages 0 to kClusterStages - 1:
// 0 to 5 the cell index with cell edge tolerance_mm (launch_cell_index_stage), 6 to 9 init, union, roots and flag, 10 to 12 the radius
// filter's tile count, tile scan and emit (launch_outlier_compact_stage), 13 (only with d_stats: eight int64, 8-byte aligned, also
// given to stage 6, which zeroes it) the statistics block. The labels form runs kClusterLabelStages launches, cluster_label_stage(k)
// of them: 0 to 8, then 14 (label roots) and 15 (labels) with d_labels (n_points int32), d_sizes (optional) and d_n_clusters; it has
// no counted variant (d_n_points NULL). d_ws: cluster_workspace_bytes(capacity) bytes, 256-byte aligned; count and capacity as
// launch_outlier_stage's. cluster_stage_name names all sixteen, and the object table's six behind them.
constexpr int kClusterStages      = 14;
constexpr int kClusterLabelStages = 11;
inline int  cluster_label_stage(int k) { return k < 9 ? k : k + 5; }
size_t      cluster_workspace_bytes(uint32_t capacity);
const char* cluster_stage_name(int stage);
hipError_t  launch_cluster_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                 int tolerance_mm, int min_size, int max_size, void* d_ws, size_t ws_bytes, int16_t* d_out,
                                 int32_t* d_out_points, long long* d_stats, int32_t* d_labels, int32_t* d_sizes, int32_t* d_n_clusters,
                                 hipStream_t st);
// The object table (pcs_cluster_objects_device; DESIGN.md section 3 "Cluster objects"): stages 16 to 21 — record roots, firsts, first
// scan, slots, accumulate, finish — behind stages 0 to 8 of launch_cluster_stage (and, for the filtered payload, its 9 to 13) over the
// same workspace, which must hold cluster_objects_workspace_bytes(capacity, max_objects). The record count is the one stage 0 left
// in the control block. d_objects: max_objects entries (NULL with 0); d_n_objects required; d_object_of optional, `capacity` int32.
// cluster_objects_scratch_word: an int32 of the workspace for a caller that needs the compaction's count and has no word of its own.
constexpr int kClusterAllStages    = 22;     // what cluster_stage_name names
constexpr int kClusterObjectStage0 = 16;
constexpr int kClusterObjectStages = 6;
size_t      cluster_objects_workspace_bytes(uint32_t capacity, uint32_t max_objects);
int32_t*    cluster_objects_scratch_word(uint32_t capacity, uint32_t max_objects, void* d_ws);
hipError_t  launch_cluster_object_stage(int stage, const int16_t* d_in, uint32_t capacity, int tolerance_mm, int min_size, int max_size,
                                        uint32_t max_objects, void* d_ws, size_t ws_bytes, pcs_cluster_object* d_objects,
                                        int32_t* d_n_objects, int32_t* d_object_of, hipStream_t st);

// Plane segmentation (pcs_plane_segment_device, pcs_plane_labels_device, pcs_plane_count_inliers_device, pcs_kernels_plane.hip; the
// definition: DESIGN.md section 3 "Plane segmentation"): each launch its own call, so that the host layer can bracket them one by one.
// A call is kPlaneInit, then per round r = 0 .. max_planes - 1 kPlaneHypotheses, kPlaneScore, kPlaneSelect, kPlaneMark and — in front
// of another round — kPlaneTileCount, kPlaneTileScan, kPlaneEmit (launch_outlier_compact_stage from the round's cloud into the next
// round's) and kPlaneOrigins; then kPlaneFinish and, in the filter form, kPlaneOutCount, kPlaneOutScan, kPlaneOutEmit (the same
// compaction from the input into d_out / d_out_points). The record count is n_points, or *d_n_points clamped to 0..capacity when that
// pointer is given, read by kPlaneInit on the device. d_ws: plane_workspace_bytes(capacity) bytes, 256-byte aligned. d_labels NULL
// (the filter form): the workspace's own. d_models (max_planes blocks of 64 bytes), d_stats (eight int64), d_n_planes: optional,
// written by kPlaneFinish. launch_plane_count: the score launch alone over n_models planes of five int64 (PlaneEq) at
// plane_count_planes(d_ws) — the front of the workspace, plane_count_workspace_bytes() bytes of it — into d_counts (zeroed by the
// caller). plane_host_staging: 1024 bytes of the workspace for a host form's models (at 0), statistics (at 512) and n_planes (at 576).
constexpr int kPlaneMaxHypotheses = 4096;
constexpr int kPlaneMaxPlanes     = 8;
enum PlaneStep : int {
    kPlaneInit, kPlaneHypotheses, kPlaneScore, kPlaneSelect, kPlaneMark, kPlaneTileCount, kPlaneTileScan, kPlaneEmit, kPlaneOrigins,
    kPlaneFinish, kPlaneOutCount, kPlaneOutScan, kPlaneOutEmit, kPlaneSteps
};
struct PlaneJob {
    const int16_t* d_in;
    uint32_t       n_points;
    const int32_t* d_n_points;
    uint32_t       capacity;
    int32_t        distance_mm, iterations, min_inliers, max_planes;
    uint32_t       seed;
    int32_t        mode;
    void*          d_ws;
    size_t         ws_bytes;
    int16_t*       d_out;
    int32_t*       d_out_points;
    int32_t*       d_labels;
    int32_t*       d_n_planes;
    void*          d_models;
    long long*     d_stats;
};
size_t      plane_workspace_bytes(uint32_t capacity);
size_t      plane_count_workspace_bytes();
long long*  plane_count_planes(void* d_ws);
void*       plane_host_staging(uint32_t capacity, void* d_ws);
const char* plane_step_name(int step);
hipError_t  launch_plane_step(const PlaneJob& job, int step, int round, hipStream_t st);
hipError_t  launch_plane_count(const int16_t* d_in, uint32_t n_points, void* d_ws, size_t ws_bytes, uint32_t n_models,
                               unsigned long long* d_counts, hipStream_t st);

// Background model and subtraction (pcs_background_*, pcs_kernels_background.hip; the definition: DESIGN.md section 3 "Background model
// and subtraction"). The table is one allocation of background_table_bytes(max_cells) bytes, 256-byte aligned, carved by
// background_table: the control block, keys[slots] (all ones: empty; probe from first_slot), seen[slots], stamp[slots];
// slots = background_slots(max_cells) = 2048 ceil(2 max_cells / 2048). Each launch is its own call, so that the host layer can bracket
// them one by one. learn: `frame` 1..65535 is the call's number; the record count is n_points, or *d_n_points clamped to 0..capacity
// when that pointer is given, read on the device; capacity > 0 sizes the grid. flag: the same count rule; d_ws is the radius filter's
// workspace (outlier_workspace_bytes(capacity)), whose control block receives the count and whose keep bits the launch writes, for
// launch_outlier_compact_stage 7, 8, 9 behind it. stats: after stage 8, d_out_points is its kept count. gather: occupied slots as
// (key low, key high, seen, 0) into d_staging[room] (16-byte aligned) through ctl->cursor, which the caller zeroes first and which ends
// at the number of occupied slots. import: n_entries > 0 entries of 12 bytes (a validated PCB1 container's, 4-byte aligned).
struct BackgroundCtl { uint32_t cells, overflow, cursor, reserved; };
struct BackgroundTable {
    unsigned long long* keys;
    uint32_t*           seen;
    uint32_t*           stamp;
    BackgroundCtl*      ctl;
    uint32_t            slots, max_cells;
    int32_t             cell_mm;
};
uint32_t        background_slots(uint32_t max_cells);
size_t          background_table_bytes(uint32_t max_cells);
BackgroundTable background_table(void* d_table, int cell_mm, uint32_t max_cells);
const char*     background_launch_name(int launch);      // of a subtract call: flag, tile count, tile scan, emit, stats
hipError_t launch_background_clear(const BackgroundTable& t, hipStream_t st);
hipError_t launch_background_learn(const BackgroundTable& t, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points,
                                   uint32_t capacity, uint32_t frame, hipStream_t st);
hipError_t launch_background_import(const BackgroundTable& t, const void* d_entries, uint32_t n_entries, hipStream_t st);
hipError_t launch_background_flag(const BackgroundTable& t, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points,
                                  uint32_t capacity, int min_seen, int dilate, int mode, void* d_ws, size_t ws_bytes, hipStream_t st);
hipError_t launch_background_stats(const BackgroundTable& t, uint32_t capacity, void* d_ws, size_t ws_bytes, const int32_t* d_out_points,
                                   uint32_t frames, int min_seen, int mode, long long* d_stats, hipStream_t st);
hipError_t launch_background_gather(const BackgroundTable& t, void* d_staging, uint32_t room, hipStream_t st);

// Object tracks (pcs_tracker_*, pcs_kernels_tracks.hip; the definition: DESIGN.md section 3 "Object tracks"). The tracker is one
// allocation of tracker_bytes(max_cells, max_objects) bytes, 256-byte aligned, carved by tracker_view: the control block, two cell
// maps (keys[slots], all ones: empty; val[slots], all ones: no object), the pair table (keys k << 32 | j, counts), id and age twice,
// best[max_objects], keeper[max_objects] and the striped counters; slots = background_slots(max_cells). `parity` says which map and which id / age arrays
// hold update t - 1: the host flips it after every update. An update is the four launches below in this order, each its own call so
// that the host layer can bracket them; every one is launched for every update, whatever the counts. The record count is n_points,
// or *d_n_points clamped to 0..capacity when that pointer is given, read on the device; m = *d_n_objects clamped to 0..max_objects.
struct TrackCtl {
    long long next_id;
    uint32_t  m;                         // of the last update (0: fresh)
    uint32_t  pair_overflow;             // the pair table ran full in the update in flight; zero between updates
    uint32_t  cur_overflow;              // the map the update in flight builds ran full
    uint32_t  prev_overflow;             // the map of the last update overflowed: the next continues nothing
    uint32_t  last_overflow;             // the overflow word of the last update's statistics
    uint32_t  reserved;
};
// The update's four counts (taking-part records, voted records, claimed cells, claimed pairs) are sums over kTrackStripes words 128
// bytes apart each, so that no two waves' adds queue on one address; assign folds and zeroes them.
constexpr uint32_t kTrackStripes = 64, kTrackStripeWords = 32, kTrackCounters = 4;
constexpr uint32_t kTrackCounterWords = kTrackCounters * kTrackStripes * kTrackStripeWords;
struct TrackerView {
    unsigned long long* prev_keys;  uint32_t* prev_val;      // P(t-1): read by the record pass, emptied by choose
    unsigned long long* cur_keys;   uint32_t* cur_val;       // P(t): empty when the update starts
    unsigned long long* pair_keys;  uint32_t* pair_count;    // empty between updates
    const long long*    prev_id;    const int32_t* prev_age;
    long long*          cur_id;     int32_t*       cur_age;
    unsigned long long* best;                                // [max_objects], zero between updates
    unsigned long long* keeper;
    TrackCtl*           ctl;
    uint32_t*           counters;                            // [kTrackCounterWords], zero between updates
    uint32_t            slots, max_cells, max_objects;
    int32_t             cell_mm;
};
constexpr int kTrackLaunches = 4;            // record pass, choose, claim, assign
size_t      tracker_bytes(uint32_t max_cells, uint32_t max_objects);
TrackerView tracker_view(void* d_tracker, int cell_mm, uint32_t max_cells, uint32_t max_objects, int parity);
hipError_t launch_track_clear(const TrackerView& t, long long first_id, hipStream_t st);
hipError_t launch_track_records(const TrackerView& t, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                const int32_t* d_object_of, const int32_t* d_n_objects, uint32_t max_objects, hipStream_t st);
hipError_t launch_track_choose(const TrackerView& t, hipStream_t st);
hipError_t launch_track_claim(const TrackerView& t, const int32_t* d_n_objects, uint32_t max_objects, hipStream_t st);
hipError_t launch_track_assign(const TrackerView& t, const int32_t* d_n_objects, uint32_t max_objects, uint32_t min_votes, long long frames,
                               void* d_tracks, long long* d_stats, hipStream_t st);

// Object boxes (pcs_object_boxes_device*, pcs_kernels_boxes.hip; the definition: DESIGN.md section 3 "Object boxes"). The workspace
// is kBoxWsWords int64 per object of max_objects (the ten sums of an object; 8-byte aligned). A call is the four launches below in
// this order, every one launched whatever the counts. The record count is n_points, or *d_n_points clamped to 0..capacity when that
// pointer is given, read on the device; m = *d_n_objects clamped to 0..max_objects. Extents are folded into d_boxes itself, whose
// entries the axes launch wrote whole.
constexpr uint32_t kBoxWsWords = 16;
constexpr int kBoxLaunches = 4;              // clear, moments, axes, extents
inline size_t boxes_workspace_bytes(uint32_t max_objects) { return (size_t)max_objects * kBoxWsWords * sizeof(long long); }
hipError_t launch_boxes_clear(const int32_t* d_n_objects, uint32_t max_objects, void* d_ws, hipStream_t st);
hipError_t launch_boxes_moments(const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                const int32_t* d_object_of, const int32_t* d_n_objects, uint32_t max_objects, void* d_ws, hipStream_t st);
hipError_t launch_boxes_axes(const int32_t* d_n_objects, uint32_t max_objects, const void* d_ws, pcs_object_box* d_boxes, hipStream_t st);
hipError_t launch_boxes_extents(const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                const int32_t* d_object_of, const int32_t* d_n_objects, uint32_t max_objects, pcs_object_box* d_boxes,
                                hipStream_t st);

// Plan-view maps (pcs_plan_view_device*, pcs_kernels_plan.hip; the definition: DESIGN.md section 3 "Plan-view maps"; the arithmetic:
// pcs_plan_math.h). The workspace is one 64-bit key per cell for the top and one for the bottom, each carved at 256 bytes (8-byte
// aligned); the count raster is accumulated in place and the statistics block folded in place (eight int64). A call is the three
// launches below in this order, every one launched whatever the counts. The record count is n_points, or *d_n_points clamped to
// 0..capacity when that pointer is given, read on the device. P.magic = plan_magic(P.cell_mm).
constexpr int kPlanLaunches = 3;             // clear, accumulate, resolve
size_t plan_workspace_bytes(uint32_t cells);
hipError_t launch_plan_clear(uint32_t n_points, const int32_t* d_n_points, uint32_t capacity, const PlanArgs& P, void* d_ws, uint32_t* d_count,
                             long long* d_stats, hipStream_t st);
hipError_t launch_plan_accumulate(const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity, const PlanArgs& P,
                                  void* d_ws, uint32_t* d_count, long long* d_stats, hipStream_t st);
hipError_t launch_plan_resolve(const int16_t* d_in, uint32_t capacity, const PlanArgs& P, const void* d_ws, const uint32_t* d_count,
                               int16_t* d_top, int16_t* d_bottom, uint8_t* d_rgb, long long* d_stats, hipStream_t st);

// Alignment sums (pcs_align_sums_device, pcs_kernels_align.hip; the definition: DESIGN.md section 3 "Alignment sums"). The target's
// index is the outlier filter's, cell edge max_dist_mm (launch_cell_index_stage over the target; `index` is its view, or nullptr for
// an empty target: nobody matches). launch_align_match: one lane per source record, one 144-byte partial per
// workgroup of kBlockThreads records into d_partials[align_partials(n_source)], dist2 (optional) written here.
// launch_align_reduce: one workgroup sums the partials and writes *d_sums whole (n_partials 0: a zeroed struct).
constexpr int kAlignTerms = 18;              // pcs_align_sums as int64 words
inline uint32_t align_partials(uint32_t n_source) { return (n_source + kBlockThreads - 1) / kBlockThreads; }
hipError_t launch_align_match(const int16_t* d_source, uint32_t n_source, const OutlierIndexView* index, int max_dist_mm,
                              long long* d_partials, uint32_t* d_dist2, hipStream_t st);
hipError_t launch_align_reduce(const long long* d_partials, uint32_t n_partials, long long* d_sums, hipStream_t st);

// Point-to-plane sums (pcs_align_plane_sums_device, pcs_kernels_align.hip; the definition: DESIGN.md section 3 "Plane sums"): the same
// index and match. launch_align_plane_scatter: the target's normals (4 shorts per record, 8-byte aligned) into d_pnorm[n_target],
// parallel to xyz[] — the caller set it to all ones on the same stream first. launch_align_plane_match: one 480-byte partial per
// workgroup into d_partials[align_partials(n_source)] (index nullptr for an empty target: d_pnorm is not read).
// launch_align_plane_reduce: one workgroup sums the partials and writes *d_sums whole (n_partials 0: a zeroed struct).
constexpr int kPlaneTerms = 60;              // pcs_align_plane_sums as int64 words
hipError_t launch_align_plane_scatter(const int16_t* d_target, const int16_t* d_target_normals, uint32_t n_target,
                                      const OutlierIndexView& index, int max_dist_mm, unsigned long long* d_pnorm, hipStream_t st);
hipError_t launch_align_plane_match(const int16_t* d_source, uint32_t n_source, const OutlierIndexView* index, const unsigned long long* d_pnorm,
                                    int max_dist_mm, long long* d_partials, uint32_t* d_dist2, hipStream_t st);
hipError_t launch_align_plane_reduce(const long long* d_partials, uint32_t n_partials, long long* d_sums, hipStream_t st);

// Surface normals (pcs_estimate_normals_device, pcs_kernels_normals.hip; the definition: DESIGN.md section 3 "Surface normals"). The
// payload's index is the outlier filter's, cell edge radius_mm (launch_cell_index_stage over the payload; `index` is its view). launch_normals_estimate: one lane per xyz[] entry, its four shorts as one word into d_cell_normals[n_points], parallel
// to xyz[] (cell order). launch_normals_gather: one lane per input record copies its word to d_normals[i] (8-byte aligned) and adds
// the valid records to *d_valid (optional; zeroed by the caller on the same stream). NormalRule: pcs_normals_math.h.
struct NormalRule;
constexpr int kNormalLaunches = 2;           // estimate, gather (behind the index's six)
hipError_t launch_normals_estimate(uint32_t n_points, const OutlierIndexView& index, const NormalRule& rule,
                                   unsigned long long* d_cell_normals, hipStream_t st);
hipError_t launch_normals_gather(const int16_t* d_in, uint32_t n_points, int radius_mm, const OutlierIndexView& index,
                                 const unsigned long long* d_cell_normals, unsigned long long* d_normals, int32_t* d_valid, hipStream_t st);

// a7 with stride.
hipError_t launch_stitch(const int16_t* d_src, uint32_t src_points, int downsample,
                         int16_t* d_dst, hipStream_t st);

}  // namespace pcs
