/*
 * pcs_hip.h — C ABI of libpcs_hip.so, the MI355X (gfx950) implementation of the
 * per-frame hot path of conix-center/pointcloud_stitching:
 *
 *     Z16 depth raster ──deproject──► XYZ (camera frame) ──4x4 rigid──► world
 *     RGB8 colour raster ──texcoord gather──► RGB
 *     ──► [x_mm y_mm z_mm R|G<<8 B] int16 x5 records (10 B / point)
 *     ──► N cameras concatenated in camera order (the "stitched" buffer)
 *
 * Citations are relative to the reference checkout (read for behaviour only):
 *   a1  sendXYZRGBPointcloud                 src/pcs-camera-optimized.cpp:669-723
 *   a2  copyPointCloudXYZRGBToBufferSIMD     src/pcs-camera-optimized.cpp:363-616   (-m path = parity target)
 *   a4  tf_mat / transform[i]                src/pcs-camera-optimized.cpp:64-72,
 *                                            src/pcs-multicamera-optimized.cpp:417-455
 *   a5  rs2::pointcloud::calculate / map_to  call sites src/pcs-camera-optimized.cpp:198-199, 288-289
 *       (third-party librealsense2; arithmetic restated in DESIGN.md "Deprojection contract")
 *   a6  buffer layout: BUF_SIZE, header      src/pcs-camera-optimized.cpp:27, 690, 715-720
 *   a7  sendStitchToUnity (concatenate)      src/pcs-multicamera-client.cpp:373-409
 *
 * The reference has no FFI; its seam is the C++ function pair a1/a2, which reads its inputs
 * through six rs2:: accessors and takes the extrinsic, thread count and flags from globals.
 * This header is what a maintainer would bind instead: plain pointers and
 * sizes, no C++ types, no exceptions across the boundary, every call returns a pcs_status.
 *
 * Conventions
 *   - All entry points return PCS_OK (0) or a negative pcs_status. Nothing calls exit().
 *   - The caller owns every buffer it passes. The context owns its device staging buffers,
 *     its per-stream constant tables and its HIP stream.
 *   - One context per host thread (the reference's kernel is not re-entrant either,
 *     src/pcs-camera-optimized.cpp:349-360). Contexts are independent of each other.
 *   - Functions suffixed _device take DEVICE pointers, enqueue on the context's HIP stream and
 *     return without synchronising (use pcs_synchronize). All others take HOST pointers and
 *     are synchronous.
 *   - There is no CPU fallback: without a usable HIP device pcs_create fails with
 *     PCS_ERR_NO_DEVICE.
 */
#ifndef PCS_HIP_H
#define PCS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCS_ABI_VERSION 1

/* a6: the wire/buffer constants of the reference (src/pcs-camera-optimized.cpp:27-30). */
#define PCS_POINT_SHORTS   5          /* x y z (R|G<<8) B                                   */
#define PCS_POINT_BYTES    10
#define PCS_HEADER_SHORTS  2          /* payload starts at buffer + 2 shorts = byte 4  :690  */
#define PCS_REF_BUF_SIZE   5000000    /* BUF_SIZE: shorts malloc'd, BYTES memset        :27,157,673 */
#define PCS_MAX_STREAMS    64

typedef enum pcs_status {
    PCS_OK               =  0,
    PCS_ERR_INVALID_ARG  = -1,
    PCS_ERR_NO_DEVICE    = -2,   /* no HIP device / device index out of range */
    PCS_ERR_HIP          = -3,   /* a HIP runtime call failed; see pcs_last_error */
    PCS_ERR_UNSUPPORTED  = -4,   /* e.g. distortion model not covered, bpp < 3 */
    PCS_ERR_CAPACITY     = -5,   /* caller's buffer too small for the result */
    PCS_ERR_NOMEM        = -6
} pcs_status;

/* Same numbering as rs2_distortion for the models covered. */
typedef enum pcs_distortion {
    PCS_DISTORTION_NONE                   = 0,
    PCS_DISTORTION_MODIFIED_BROWN_CONRADY = 1,
    PCS_DISTORTION_INVERSE_BROWN_CONRADY  = 2,
    PCS_DISTORTION_FTHETA                 = 3,  /* unsupported unless coeffs are all zero */
    PCS_DISTORTION_BROWN_CONRADY          = 4   /* unsupported unless coeffs are all zero */
} pcs_distortion;

/* Field order of rs2_intrinsics so a binding can memcpy one into the other. */
typedef struct pcs_intrinsics {
    int32_t width, height;
    float   ppx, ppy;
    float   fx, fy;
    int32_t model;          /* pcs_distortion */
    float   coeffs[5];      /* k1 k2 p1 p2 k3 */
} pcs_intrinsics;

/* rs2_extrinsics: rotation is a COLUMN-major 3x3, translation in metres. */
typedef struct pcs_extrinsics {
    float rotation[9];
    float translation[3];
} pcs_extrinsics;

/* Everything the reference takes from librealsense profile queries and from its globals,
 * for one camera stream. */
typedef struct pcs_stream_config {
    pcs_intrinsics depth;            /* depth stream geometry + pinhole model                    */
    pcs_intrinsics color;            /* colour stream geometry + pinhole model (map_to target)   */
    pcs_extrinsics depth_to_color;   /* rs2 get_extrinsics(depth -> colour)                      */
    float          depth_scale;      /* metres per Z16 unit; 0.001f on D400                      */
    int32_t        color_bpp;        /* video_frame::get_bytes_per_pixel      (>= 3)     :374    */
    int32_t        color_stride;     /* video_frame::get_stride_in_bytes                 :375    */
    float          cam_to_world[16]; /* row-major 4x4, metres, last row unused = tf_mat  :64-67  */
} pcs_stream_config;

/* pcs_config.flags */
#define PCS_FLAG_CUTOFF         0x1u  /* -c: keep iff 0<z<=1.5 && -2<x<=2 (camera frame), compacted in
                                         ascending point order (= the reference's -c -m -t1 order) :499-577 */
#define PCS_FLAG_CUTOFF_COMPAT  0x2u  /* with CUTOFF: reproduce the reference's lane-reversed mask (point k of
                                         each aligned group of 4 is gated by point 3-k)  :501-502,519 */
#define PCS_FLAG_DROP_INVALID   0x4u  /* drop depth==0 pixels (not in the reference; north-star compaction) */
#define PCS_FLAG_FORCE_IEEE     0x8u  /* never use the certified reduced-instruction arithmetic (A/B testing);
                                         results are identical either way */
#define PCS_FLAG_TEXCOORD_HALF_PIXEL 0x10u /* deprojection: u = (px + 0.5)/W, v = (py + 0.5)/H as older librealsense
                                         releases computed texture coordinates; default is
                                         u = px/W, v = py/H. The reference's +0.5 and clamp (:434-444) follow either way */
#define PCS_FLAG_SCALAR_ARITH   0x20u /* the reference's DEFAULT (no -m) arithmetic, copyPointCloudXYZRGBToBuffer :620-667, bit for
                                         bit as its build compiles it: m1*y rounded, m0*x and m2*z fused, + t rounded, * 1000.0 in
                                         double, cvttsd2si. With CUTOFF its loop (:640-646): record i stays in slot i, a skipped
                                         slot is not written (a1 / a2 twins) or reads as ten zero bytes (fused calls), the count
                                         is n_points; CUTOFF_COMPAT changes nothing. Fixed for the life of the context. Not with
                                         DROP_INVALID; the _batch, _counted, voxel, partials, sink and payload re-transform calls
                                         return PCS_ERR_UNSUPPORTED on such a context (it returns these bytes or fails) */

typedef struct pcs_config {
    int32_t                  device;      /* HIP device ordinal */
    int32_t                  n_streams;   /* 1..PCS_MAX_STREAMS */
    const pcs_stream_config* streams;     /* n_streams entries, copied by pcs_create */
    uint32_t                 flags;       /* PCS_FLAG_* */
    int32_t                  downsample;  /* a7: keep every downsample-th kept point per stream; >= 1
                                             (src/pcs-multicamera-client.cpp:375,388) */
} pcs_config;

typedef struct pcs_ctx pcs_ctx;

/* ---- lifecycle ------------------------------------------------------------------------- */
int          pcs_abi_version(void);
int          pcs_device_count(void);                 /* >= 0, or a negative pcs_status */
int          pcs_create(pcs_ctx** out, const pcs_config* cfg);
void         pcs_destroy(pcs_ctx* ctx);
const char*  pcs_strerror(int status);
const char*  pcs_last_error(const pcs_ctx* ctx);     /* detail of the last failure on this ctx */

/* Replace one stream's camera->world matrix (the reference edits tf_mat in source, :64-67). */
int          pcs_set_cam_to_world(pcs_ctx* ctx, int stream, const float m16[16]);

/* ---- crop box: keep what lies inside a box in the WORLD frame (not in the reference) ----------------------------- *
 * A context may carry one crop box: inclusive bounds lo[a] <= hi[a], int16 millimetres, world frame, axis order x, y, z. It is
 * defined ON THE RECORD, the integer domain the voxel grid is defined in: a point is kept iff every one of its record's three
 * shorts s_a satisfies lo[a] <= s_a <= hi[a], where s_a is what -m arithmetic writes — the low 16 bits of the converted
 * coordinate, read as signed, i.e. AFTER the int16 wrap. A point 70 m out wraps to 4.464 m, and a box around that keeps it: the
 * price of "cropping at the edge == cropping the same payload at the centre" (pcs_crop_payloads_device), which holds bit for bit.
 *   - The box is ANDed with whatever the context's flags gate (CUTOFF, DROP_INVALID). CUTOFF_COMPAT's lane reversal applies to
 *     the cutoff's own range bit only, never to the box bit.
 *   - downsample keeps every downsample-th KEPT point per stream; output order is ascending point index per stream, streams in
 *     index order; counts are device-known, exactly as under DROP_INVALID (the payload needs its worst-case capacity).
 *   - Honoured by pcs_process_frames (staged and zero-copy), pcs_submit_frames / pcs_collect_frames, pcs_process_frames_device,
 *     pcs_process_frames_device_batch and every voxel entry that starts from rasters (one call, partials, sink: they build the
 *     cropped payload first and read that). Always count + scan + emit: PCS_COMPACT_PATH does not apply to a boxed context.
 *   - Refused with PCS_ERR_UNSUPPORTED ("crop box" in pcs_last_error) while a box is set, nothing launched, nothing written:
 *     pcs_process_frames_device_counted (a producer cannot know the world predicate) and the a1 / a2 twins in all forms (they
 *     are signature twins of reference functions that have no such argument).
 *   - pcs_stitch_device and pcs_transform_payloads_device move payloads and read no context predicate: unaffected.
 * pcs_set_crop_box_mm: both pointers NULL clears the box; lo[a] > hi[a] or exactly one NULL is PCS_ERR_INVALID_ARG; on a
 * PCS_FLAG_SCALAR_ARITH context PCS_ERR_UNSUPPORTED (such a context returns a3's bytes or fails). Ordering as
 * pcs_set_cam_to_world: the context's stream is synchronised first, so no call enqueued earlier sees the change.
 * pcs_get_crop_box_mm: 1 and the bounds if a box is set, 0 (lo / hi untouched) if not.                                            */
int          pcs_set_crop_box_mm(pcs_ctx* ctx, const int16_t lo[3], const int16_t hi[3]);
int          pcs_get_crop_box_mm(const pcs_ctx* ctx, int16_t lo[3], int16_t hi[3]);

/* Which arithmetic the fused kernels use for `stream`: 0 = IEEE expansion, 1 = certified reduced-instruction
 * form, 2 = certified + identity depth->colour rotation shortcut; 3 / 4 = 1 / 2 plus the no-overflow certificate
 * (conversions cannot reach 2^31, so no running maximum is kept) (DESIGN.md "Certified arithmetic"). The
 * results are bit-identical; this is a diagnostic. */
int          pcs_stream_math(const pcs_ctx* ctx, int stream);
/* 1 when the stream's colour ROW is certified independent of the depth value (depth->colour R = I, t_y = t_z = 0, no distortion, and a
 * sweep over every raster row x every Z16 value on the device at pcs_create found no exception): the voxel reader then takes the row
 * from a per-row table instead of computing it per pixel. Same bytes either way; PCS_ROW_CONST=0 at pcs_create turns it off (A/B). */
int          pcs_stream_color_row_const(const pcs_ctx* ctx, int stream);

/* Number of points one frame of `stream` deprojects to (= depth width*height). */
int          pcs_stream_points(const pcs_ctx* ctx, int stream);
/* Upper bound of the stitched payload in shorts for the current config (no header). */
size_t       pcs_max_payload_shorts(const pcs_ctx* ctx);

/* ---- a2 twin: bit-exact replacement of copyPointCloudXYZRGBToBufferSIMD (:363-616) ------ *
 * vertices  = pts.get_vertices()            n_points x {float x,y,z}
 * texcoords = pts.get_texture_coordinates() n_points x {float u,v}
 * color     = color.get_data(); geometry (w,h,bpp,stride) and tf_mat come from stream's config
 * pc_buffer = the reference's `buffer + 2` (payload pointer); needs 5*n_points shorts
 * returns the number of points written in *out_points (n_points, or the kept count under -c).
 * Any n_points >= 0 is accepted (the reference needs n % 4 == 0, :414).                      */
int pcs_copy_pointcloud_xyzrgb_to_buffer(pcs_ctx* ctx, int stream,
                                         const float* vertices, const float* texcoords, int n_points,
                                         const uint8_t* color, int16_t* pc_buffer, int* out_points);
int pcs_copy_pointcloud_xyzrgb_to_buffer_device(pcs_ctx* ctx, int stream,
                                         const float* d_vertices, const float* d_texcoords, int n_points,
                                         const uint8_t* d_color, int16_t* d_pc_buffer, int* d_out_points);

/* Batched device form of the a2 twin: n_clouds cameras' rs2::points arrays packed by ONE launch (per group of 16)
 * instead of one latency-bound launch per camera — the reference runs copyPointCloudXYZRGBToBufferSIMD once per
 * camera process (src/pcs-camera-optimized.cpp:363); a node that hosts all cameras hands them over together.
 * `clouds` is a HOST array whose pointer fields are DEVICE pointers; cloud i is packed exactly as
 * pcs_copy_pointcloud_xyzrgb_to_buffer_device(ctx, clouds[i].stream, ...) would. d_out_points (optional, device)
 * receives n_clouds ints. Under -c (a predicate) the clouds are processed one after the other.                  */
typedef struct pcs_cloud_desc {
    int32_t        stream;      /* which stream's tf_mat / colour geometry applies                               */
    int32_t        n_points;    /* pts.size()                                                                     */
    const float*   vertices;    /* pts.get_vertices()                                                             */
    const float*   texcoords;   /* pts.get_texture_coordinates()                                                  */
    const uint8_t* color;       /* color.get_data()                                                               */
    int16_t*       pc_buffer;   /* the reference's buffer + 2; 5*n_points shorts                                  */
} pcs_cloud_desc;
int pcs_copy_pointclouds_xyzrgb_to_buffer_device(pcs_ctx* ctx, int n_clouds, const pcs_cloud_desc* clouds,
                                                 int* d_out_points);

/* ---- a1 twin: sendXYZRGBPointcloud (:669-723) without the socket ----------------------- *
 * buffer must hold buffer_shorts shorts (the reference mallocs PCS_REF_BUF_SIZE). On return:
 * payload at buffer+2 shorts; if write_header, int32 LE payload byte count at byte 0 (:718);
 * every other byte below min(PCS_REF_BUF_SIZE, 2*buffer_shorts) is zero (:673).
 * *out_size_bytes = 5*count*sizeof(short) (:697).                                            */
int pcs_send_xyzrgb_pointcloud(pcs_ctx* ctx, int stream,
                               const float* vertices, const float* texcoords, int n_points,
                               const uint8_t* color, int16_t* buffer, size_t buffer_shorts,
                               int write_header, int* out_size_bytes);

/* ---- fused a5+a2 for all streams, output in a7's stitched layout ------------------------ *
 * depth[s]  : stream s Z16 raster, depth.width*depth.height uint16, row-major, tightly packed
 * color[s]  : stream s colour raster, color.height rows of color_stride bytes
 * stitched  : [int32 payload bytes][stream 0 points][stream 1 points]...   (header only if write_header;
 *             payload always starts at stitched + 2 shorts)
 * points_per_stream[s] (optional) = points stream s contributed; *out_size_bytes = payload bytes.
 * Synchronous. Pageable buffers are staged (upload, kernel, download: 2.2 ms for 8 x 1280x720). When EVERY raster and
 * the stitched buffer are page-locked and device-addressable (pcs_host_malloc / hipHostMalloc / hipHostRegister) and the
 * stitched buffer has room for the worst case, the kernels read and write the host memory directly — both directions of the
 * link at once, no staging copies: 1.6 ms (the link's own duplex limit for these volumes is 1.47 ms). PCS_ZERO_COPY=0
 * forces the staged route. */
int pcs_process_frames(pcs_ctx* ctx, const uint16_t* const* depth, const uint8_t* const* color,
                       int16_t* stitched, size_t stitched_shorts, int write_header,
                       int* points_per_stream, int* out_size_bytes);

/* Software-pipelined form of pcs_process_frames for frame loops (same inputs, same stitched layout, same
 * bytes). pcs_submit_frames queues the uploads and the kernel(s) of one frame-set into one of
 * PCS_PIPELINE_DEPTH device slots and returns a ticket; pcs_collect_frames waits for that frame-set and
 * downloads it. Writing the loop as  submit(k+1); collect(k);  lets the upload of the next frame-set run
 * while the previous payload downloads (PCIe is full duplex; the two directions use separate HIP streams).
 * The overlap needs page-locked host buffers (pcs_host_malloc): with pageable memory the runtime copies
 * synchronously and the pair simply costs what pcs_process_frames costs. depth[s] / color[s] must stay
 * valid and unmodified until the matching collect returns. Tickets must be collected in submission order.
 * PCS_ERR_CAPACITY from submit = all slots in flight (collect first).                              */
#define PCS_PIPELINE_DEPTH 2
int pcs_submit_frames(pcs_ctx* ctx, const uint16_t* const* depth, const uint8_t* const* color, int* ticket);
int pcs_collect_frames(pcs_ctx* ctx, int ticket, int16_t* stitched, size_t stitched_shorts, int write_header,
                       int* points_per_stream, int* out_size_bytes);

/* Device-resident form: pointers are device pointers, d_payload is the PAYLOAD pointer
 * (no header), payload_shorts its capacity. d_counts (optional) receives n_streams+1 int32:
 * per-stream point counts followed by the total. Asynchronous on the context stream.
 * Without CUTOFF/DROP_INVALID the counts are known on the host (pcs_stream_points) and
 * d_counts may be NULL.                                                                       */
int pcs_process_frames_device(pcs_ctx* ctx, const uint16_t* const* d_depth, const uint8_t* const* d_color,
                              int16_t* d_payload, size_t payload_shorts, int32_t* d_counts);

/* The same with the per-tile kept counts HANDED IN by a producer that already knows them (whatever wrote the depth image on
 * the GPU — a decoder, a filter, a simulator — can count as it writes): the count pass, and with it the second read of the
 * Z16 rasters, does not run (8 x 1280x720 with invalid-depth drop: 5.3 us of kernel time and 14.7 MB of reads per frame-set
 * less; in a back-to-back frame loop, where the next call's count pass hides behind the tail of the previous emit launch
 * anyway, 32.1 -> 31.2 us per frame-set).
 * A tile is PCS_TILE_POINTS consecutive pixels of one stream (row-major, the last tile of a stream may be short);
 * d_tile_kept[pcs_stream_tile_base(ctx, s) + t] = how many pixels of tile t of stream s the context's predicate keeps
 * (PCS_FLAG_DROP_INVALID alone: its non-zero depth words). pcs_stream_tile_base(ctx, n_streams) = entries in all. The counts
 * must be exact for the output to be the stitched cloud; WRONG counts garble the cloud but cannot write outside the payload's
 * worst-case capacity (they are clamped to a tile). Without CUTOFF / DROP_INVALID the counts are ignored.              */
#define PCS_TILE_POINTS 2048
int pcs_stream_tile_base(const pcs_ctx* ctx, int stream);
int pcs_process_frames_device_counted(pcs_ctx* ctx, const uint16_t* const* d_depth, const uint8_t* const* d_color,
                                      const uint32_t* d_tile_kept, int16_t* d_payload, size_t payload_shorts, int32_t* d_counts);

/* ---- depth pre-filter: temporal smoothing and hole filling, Z16 -> Z16 on the device --------------------------------------- *
 * The two librealsense post-processing blocks the reference leaves as TODOs at its a1 seam (rs2_create_temporal_filter_block,
 * rs2_create_hole_filling_filter_block: src/pcs-camera-optimized.cpp:682-684), as ONE stateful launch over every stream of the
 * context, upstream of everything else: it writes Z16 rasters the stitch calls then read. The definition is this project's own
 * (DESIGN.md §3 "Depth pre-filter": modelled on librealsense's published filters, parity with librealsense unpinned); the GPU
 * output is held bit for bit to a numpy restatement of that text (tests/np_depth_filter.py).
 *   temporal   per pixel, with c the input, p the stage's previous output and an 8-frame validity history: c and p valid and
 *              |c - p| < delta -> alpha*c + (1-alpha)*p (fp32: two rounded products, one rounded sum, truncated, clamped to 65535);
 *              c valid otherwise -> c; c == 0 -> p if p was valid in M of the last L frames (persistence 0..8: never, 8/8, 2/3,
 *              2/4, 2/8, 1/2, 1/5, 1/8, always), else 0.
 *   hole_fill  1 = fill from left: after the temporal stage a zero pixel takes the nearest non-zero pixel to its left in its
 *              row; nothing crosses a row or a stream; filled values never enter the temporal state. librealsense's other two
 *              modes are raster-order recurrences over two dimensions with no parallel form of the same output: values other
 *              than 0 and 1 are PCS_ERR_UNSUPPORTED.
 * pcs_set_depth_filter: validates (NaN, alpha <= 0 or > 1, delta outside 1..65535, persistence outside 0..8, both stages off:
 *   PCS_ERR_INVALID_ARG; hole_fill not 0 / 1: PCS_ERR_UNSUPPORTED; the temporal parameters are checked whether or not that stage
 *   is on, so fill the defaults in), synchronises the context's stream (pcs_set_cam_to_world's
 *   rule), allocates 3 bytes per depth pixel per stream of state when temporal is on (failure: PCS_ERR_NOMEM, the context is left
 *   without a filter) and zeroes it: setting a filter again resets the state. NULL clears the filter and frees the state, as
 *   pcs_destroy does. Works on every context (PCS_FLAG_SCALAR_ARITH included: the filter sits upstream of the arithmetic).
 * pcs_get_depth_filter: 1 and the configuration if a filter is set, 0 (out untouched) if not.
 * pcs_reset_depth_filter: zeroes the state of every stream (a recording that loops, a scene cut). Asynchronous on the stream.
 * pcs_filter_depth_device: asynchronous on the context's stream, one launch for all streams; EVERY call advances the state by one
 *   frame. d_in[s] / d_out[s]: device pointers, 2-byte aligned, depth.width*depth.height uint16, row-major, tightly packed — what
 *   pcs_process_frames_device asks of d_depth[s]; 16-byte aligned rasters whose width is a multiple of 8 take the wide accesses.
 *   d_out[s] == d_in[s] (in place) is allowed; any other overlap, between or within streams, is the caller's error. Without a
 *   filter: PCS_ERR_INVALID_ARG ("depth filter" in pcs_last_error).
 *   d_tile_kept (optional, 4-byte aligned, pcs_stream_tile_base(ctx, n_streams) words): the call zeroes it on the stream and
 *   writes the number of NON-ZERO OUTPUT pixels of every PCS_TILE_POINTS tile, in the layout pcs_process_frames_device_counted
 *   takes — on a PCS_FLAG_DROP_INVALID context the next stitch then needs no count pass. With PCS_FLAG_CUTOFF or a crop box the
 *   counts would need the deprojection: non-NULL is PCS_ERR_UNSUPPORTED there, nothing launched, nothing written. On a dense
 *   context the counts are written and correct; the stitch ignores them. Measured (8 x 1280x720): the counts
 *   cost this call 7.4 us (a memset launch and per-tile atomics), more than the 5.3 us count pass they spare the stitch: on one
 *   device filter + counted stitch is no faster than filter + pcs_process_frames_device. The counts are for producers that must
 *   not read the rasters twice.
 * pcs_filter_depth: host pointers, synchronous: upload, pcs_filter_depth_device in place on the context's staging rasters,
 *   download (in[s] == out[s] is fine). For the CLI and for tests; no zero-copy route.
 * HBM traffic per pixel: 10 B with the temporal stage (2 in + 2 out + 4 state value + 2 history), 4 B for hole fill alone.      */
typedef struct pcs_depth_filter_config {
    int32_t temporal;      /* 0 off, 1 on */
    float   alpha;         /* (0,1]; librealsense's default 0.4 */
    int32_t delta;         /* 1..65535 Z16 units; default 20 */
    int32_t persistence;   /* 0..8; default 3 */
    int32_t hole_fill;     /* 0 off, 1 fill from left */
} pcs_depth_filter_config;
int pcs_set_depth_filter(pcs_ctx* ctx, const pcs_depth_filter_config* cfg);
int pcs_get_depth_filter(const pcs_ctx* ctx, pcs_depth_filter_config* out);
int pcs_reset_depth_filter(pcs_ctx* ctx);
int pcs_filter_depth_device(pcs_ctx* ctx, const uint16_t* const* d_in, uint16_t* const* d_out, uint32_t* d_tile_kept);
int pcs_filter_depth(pcs_ctx* ctx, const uint16_t* const* in, uint16_t* const* out);

/* ---- depth decimation: every n x n block of a Z16 raster to one pixel, on the device --------------------------------------- *
 * The first block of librealsense's post-processing chain (decimation, then spatial / temporal, then hole filling), as ONE
 * stateless launch over every stream of the context, upstream of the depth pre-filter above and of the stitch calls: the payload
 * shrinks by n*n and loses noise instead of keeping whatever the n-th point happens to be (pcs_config.downsample). The definition
 * is this project's own (DESIGN.md section 3 "Depth decimation": modelled on librealsense's decimation filter, parity with
 * librealsense unpinned - the reference never calls the block); the GPU output is held bit for bit to a numpy restatement of that
 * text (tests/np_decimation.py).
 *   scale n in 2..8; source W x H uint16, row-major, tightly packed; output Wd x Hd with Wd = W / n, Hd = H / n (integer division).
 *   Source columns >= n*Wd and rows >= n*Hd are never read. The output is NOT padded (librealsense pads its output dimensions up
 *   to a multiple of 4). Output pixel (r, c) is taken from the k non-zero values of the block in[n r + a][n c + b], a, b in [0, n):
 *     k = 0       0
 *     n = 2, 3    the lower median: with the non-zero values sorted ascending v_0 <= ... <= v_(k-1), v_((k-1) >> 1) (two valid
 *                 pixels: the nearer surface)
 *     n >= 4      floor(sum of the non-zero values / k), an integer division
 *   Nothing crosses a block or a stream; there is no state.
 * pcs_decimated_stream_config: the stream a decimated raster belongs to. Pure host arithmetic: no context, no device, works on a
 *   machine without a GPU. The integer pixel index is the pixel's centre (mx = ((float)c - ppx) / fx) and
 *   decimated column i stands for source columns n i .. n i + n - 1, so
 *     fx'  = (float)((double)fx / n)                       fy'  likewise
 *     ppx' = (float)(((double)ppx - (n - 1) / 2.0) / n)    ppy' likewise          width' = W / n, height' = H / n
 *   each computed in double from the float fields and rounded to float once. model and coeffs are unchanged (they act on the
 *   normalised mx, my); color, depth_to_color, depth_scale, color_bpp, color_stride and cam_to_world are copied: the colour raster
 *   is NOT decimated - texture coordinates come from projecting the 3-D point into the colour camera, so the full-resolution
 *   colour image keeps working. scale 1 copies in to out; in == out is allowed. scale outside 1..8, a NULL pointer, or a raster
 *   with no pixel left (W / scale == 0 or H / scale == 0): PCS_ERR_INVALID_ARG (pcs_last_error(NULL) says which).
 * pcs_decimate_depth_device: ctx is the context that will CONSUME the output, created from decimated stream configs (stream s has
 *   depth.width = Wd_s, depth.height = Hd_s); src_width[s] / src_height[s] (host arrays, n_streams entries) are the source rasters'
 *   sizes. Stateless: nothing is set, nothing is stored in the context. Validated on the host before anything is launched: scale
 *   in 2..8; src_width[s] / scale == depth.width and src_height[s] / scale == depth.height for every stream; pointers non-NULL and
 *   2-byte aligned; no d_out[s] shares a byte with any d_in[t] (in place is impossible) - PCS_ERR_INVALID_ARG, and pcs_last_error
 *   names the stream and the quantity. Asynchronous on the context's stream, one launch for all streams whatever their sizes; rows
 *   of any width. Works on every context (PCS_FLAG_SCALAR_ARITH included: decimation sits upstream of the arithmetic). d_out[s] is
 *   what pcs_filter_depth_device and pcs_process_frames_device* take as d_depth[s]. Source rasters whose width is a multiple of 8
 *   at a 16-byte aligned address are read with 16-byte loads, outputs likewise written with 16-byte stores; anything else works,
 *   2 bytes at a time.
 * pcs_decimate_depth: host pointers, synchronous: upload, pcs_decimate_depth_device, download. For the CLI and for tests. The
 *   full-size staging is allocated on first use, grown when a later call is larger and freed by pcs_destroy; an allocation failure
 *   is PCS_ERR_NOMEM and leaves the context usable.
 * HBM traffic per stream: 2 W H bytes in + 2 Wd Hd bytes out. Measured (python tools/decimate_probe.py 200 20; 8 x 1280x720, one
 *   MI355X, sources cold from HBM, per-call event pairs, median / minimum of 200 calls): scale 2 8.5 / 8.0 us, scale 3 11.6 / 11.1,
 *   scale 4 9.0 / 8.6, scale 8 13.0 / 12.5 - latency-bound (the traffic floor is about 2 us). decimate + pcs_process_frames_device
 *   on the decimated context against pcs_process_frames_device on the full-size one: 18.1 / 19.6 / 15.1 / 19.4 us against 23.2.
 *   DESIGN.md section 10 (f6).                                                                                                   */
int pcs_decimated_stream_config(const pcs_stream_config* in, int scale, pcs_stream_config* out);
int pcs_decimate_depth_device(pcs_ctx* ctx, int scale, const int32_t* src_width, const int32_t* src_height,
                              const uint16_t* const* d_in, uint16_t* const* d_out);
int pcs_decimate_depth(pcs_ctx* ctx, int scale, const int32_t* src_width, const int32_t* src_height,
                       const uint16_t* const* in, uint16_t* const* out);

/* ---- spatial filter: edge-preserving smoothing along rows and columns, Z16 -> Z16 on the device ----------------------------- *
 * The second block of librealsense's chain (decimation, then SPATIAL, then temporal, then hole filling): call it between
 * pcs_decimate_depth_device and pcs_filter_depth_device. Stateless; 2 x iterations launches over every stream of the context.
 * The definition is this project's own (DESIGN.md section 3 "Spatial filter": modelled on librealsense's spatial filter, parity
 * with librealsense unpinned); the GPU output is held bit for bit to a numpy restatement of that text
 * (tests/np_spatial_filter.py). With a = (float)alpha and oma = 1.0f - a computed once on the host in fp32:
 *   a line pass over x[0..n-1], fill on or off: v0 = x[0], run = 0; for u = 1..n-1 in order, v1 = x[u]:
 *     v1 != 0                                 run = 0
 *     v0, v1 != 0 and 1 <= |v1 - v0| <= delta x[u] = v1 = min((int)(fl(fl(a v1) + fl(oma v0)) + 0.5f), 65535): two rounded products,
 *                                             two rounded sums, no FMA, truncated (d = 0 and an edge d > delta leave x[u] alone)
 *     v0 != 0, v1 == 0, fill on, run < hole_radius    run += 1, x[u] = v1 = v0
 *     then v0 = v1
 *   one iteration: every row left to right (fill on), every row right to left (fill on), every column top to bottom (fill off),
 *   every column bottom to top (fill off), each reading what the one before wrote; the filter is `iterations` of those. Nothing
 *   crosses a stream; no state between calls. Unlike librealsense: the forward pass reaches the last pixel, run resets at every
 *   valid input pixel, hole_radius is a pixel count (up to exactly that many per gap and direction), Z16 domain only.
 * pcs_spatial_filter_depth_device: stream sizes are the context's depth.width x depth.height (after decimation: the decimated
 *   ones). Nothing is set in the context and a depth filter that is set is not disturbed. Validated on the host before anything
 *   is launched, PCS_ERR_INVALID_ARG with the quantity (and for a pointer the stream) in pcs_last_error: NULL config; NaN,
 *   alpha <= 0 or > 1; delta outside 1..65535; iterations outside 1..5; hole_radius outside 0..65535; NULL or odd pointers; a
 *   d_out[s] that shares a byte with any d_in[t] other than d_out[s] == d_in[s] (in place). Asynchronous on the context's stream.
 *   The first row launch reads d_in and writes d_out, everything after it runs in place on d_out. Rows of any width; rasters
 *   whose width is a multiple of 8 at 16-byte aligned addresses take 16-byte accesses in the row launches. Works on every context
 *   (PCS_FLAG_SCALAR_ARITH included).
 * pcs_spatial_filter_depth: host pointers, synchronous: upload to the context's staging rasters, in place there, download
 *   (in[s] == out[s] is fine). For the CLI and for tests.
 * Cost: one lane walks one line, so a launch is a chain of 2 W (rows) or 2 H (columns) dependent steps and is bound by that
 *   chain, not by its 4 B/pixel of traffic: iterations x 4000 steps at 1280x720. Not measured yet (python
 *   tools/spatial_filter_probe.py 200 20 is the measurement); the estimate from the kernels' instruction counts, about 35 ns per
 *   step and so about 150 us per iteration at 8 x 1280x720, is in DESIGN.md section 10 (f7). It pays after a decimation.         */
typedef struct pcs_spatial_filter_config {
    float   alpha;         /* (0,1]; default 0.5 */
    int32_t delta;         /* 1..65535 Z16 units; default 20 */
    int32_t iterations;    /* 1..5; default 2 */
    int32_t hole_radius;   /* 0..65535 pixels filled per gap and direction in the row passes; default 0 (off) */
} pcs_spatial_filter_config;
int pcs_spatial_filter_depth_device(pcs_ctx* ctx, const pcs_spatial_filter_config* cfg, const uint16_t* const* d_in,
                                    uint16_t* const* d_out);
int pcs_spatial_filter_depth(pcs_ctx* ctx, const pcs_spatial_filter_config* cfg, const uint16_t* const* in, uint16_t* const* out);

/* Throughput form: n_sets frame-sets of the SAME streams per call. d_depth / d_color hold n_sets * n_streams device
 * pointers, frame-set major (entry k*n_streams + s = stream s of frame-set k); d_payload[k] is frame-set k's payload
 * pointer (each with payload_shorts capacity), d_counts (optional) n_sets pointers as in pcs_process_frames_device.
 * Each payload receives exactly the bytes pcs_process_frames_device would write. On the dense path (no
 * CUTOFF/DROP_INVALID, downsample 1, 16-byte aligned payloads) up to 64 / n_streams frame-sets share ONE kernel
 * launch, which amortises the fill and drain of a ~23 us launch (8 x 1280x720: 58 % -> ~68 % of HBM peak). With
 * CUTOFF/DROP_INVALID (downsample 1, n_streams <= 16) the same number of frame-sets share THREE launches — count,
 * scan, emit, each covering every set — instead of three per set (8 x 1280x720: 34 -> 25 us per frame-set, 39 % ->
 * 50 %), with no assumption about workgroup dispatch order. Other configurations are processed set by set. A caller
 * that must hand a frame-set on as soon as it is complete keeps using pcs_process_frames_device: batching trades
 * latency for throughput.                                                                                       */
int pcs_process_frames_device_batch(pcs_ctx* ctx, int n_sets, const uint16_t* const* d_depth,
                                    const uint8_t* const* d_color, int16_t* const* d_payload, size_t payload_shorts,
                                    int32_t* const* d_counts);

/* Deprojection only (a5 restated): Z16 -> vertices (N x 3 float) and texcoords (N x 2 float),
 * i.e. what rs2::pointcloud::calculate + map_to hand to a2. Host pointers. For parity tests
 * and for callers that still want the intermediate rs2::points arrays.                       */
int pcs_deproject(pcs_ctx* ctx, int stream, const uint16_t* depth, float* vertices, float* texcoords);

/* ---- a7: stitch already-packed per-camera payloads (sendStitchToUnity, :373-409) -------- *
 * Keeps every downsample-th 10-byte point of each camera, cameras in index order.
 * Device pointers; *total_points is written on the HOST (counts are host-known).             */
int pcs_stitch_device(pcs_ctx* ctx, const int16_t* const* d_cam_payload, const int* cam_points, int n_cams,
                      int downsample, int16_t* d_stitched_payload, size_t stitched_shorts, int* total_points);

/* ---- the centre-side crop: the context's crop box over already packed per-camera payloads ------------------------- *
 * For edge servers that cannot crop. Cameras are written in index order into one stitched payload; per camera the records
 * inside the context's box (see pcs_set_crop_box_mm: the same predicate on the same shorts) are kept in order, and every
 * downsample-th KEPT one is written (kept index % downsample == 0). Without a box every record is inside: pcs_stitch_device's
 * bytes. d_counts: n_cams + 1 int32 on the DEVICE (written per camera, then the total) — the counts are data dependent.
 * Inputs and output are 2-byte aligned device pointers (the reference's `buffer + 2` shorts makes them 4 mod 16);
 * cam_points[i] == 0 is legal; n_cams <= PCS_MAX_STREAMS. stitched_shorts is checked on the host against the WORST case, the
 * sum of ceil(cam_points[i] / downsample) records; any overlap of an input with that output range is refused.
 * 10 B read twice + 10 B written per kept record.                                                                              */
int pcs_crop_payloads_device(pcs_ctx* ctx, const int16_t* const* d_cam_payload, const int* cam_points, int n_cams,
                             int downsample, int16_t* d_stitched_payload, size_t stitched_shorts, int32_t* d_counts);

/* ---- the centre's re-transform of already packed payloads (src/pcs-multicamera-optimized.cpp:226-265, 289) ---------------- *
 * What the reference's pcs-multicamera-optimized does with every camera's payload before it concatenates them
 * (updateCloudXYZRGB, :268-299; send_stitchedXYZRGB, :301-318) — in contrast with pcs-multicamera-client, which copies the
 * records as they are (pcs_stitch_device). Per kept record (i % downsample == 0, :236):
 *   x,y,z = (float)int16 / 1000.0f                     CONV_RATE is `const float CONV_RATE = 1000.0` in THAT file (:46)
 *   p'    = ((m0*x + m1*y) + m2*z) + m3 per row         pcl::transformPointCloud(cloud, cloud, transform[i]) (:289): PCL 1.8
 *                                                       transforms.hpp's expression; products and sums individually rounded
 *                                                       (the target is built without -mfma). THIRD-PARTY: this association
 *                                                       is restated, parity with PCL unpinned.
 *   int16 = low 16 bits of cvttss2si(p' * 1000.0f)      static_cast<short>(x * CONV_RATE) (:255-257)
 *   colour: short 3 (R | G<<8) survives bit for bit, short 4 becomes B with a zero high byte (:240-242, :258-259)
 * PINNED to the compiled reference (tests/test_reference_pin_centre.py, tests/golden/ref_centre/: both centre programs compiled
 * against declaration-only PCL stand-ins): the decode, the encode, the stride rule, the count where the stride divides it, and the
 * framing (header, payload at short 2). NOT pinned: PCL's association above — which does not matter for a matrix whose rows hold
 * one entry of +-1 plus a translation (one rounding under any order; those cases are pinned end to end) — and FLOOR at
 * n_points % downsample != 0, where the compiled reference cannot be driven (see below).
 * The round trip is LOSSY (decode, move, truncate) — it is the reference program's behaviour, not an improvement; the default
 * of the work-alike CLI stays the lossless concatenation. Cameras are written in index order into ONE stitched
 * payload (what `*stitched_cloud += *cloud_ptr[i]`, :361-364, and convertPointCloudXYZRGBToBuffer produce); all cameras of a
 * call share launches of up to 16 clouds. `cams` is a HOST array whose payload pointers are DEVICE pointers. A camera may be
 * transformed in place (its output slice starting exactly at its input, downsample 1); any other overlap of an input with an
 * output slice is refused. points_per_cam (optional, host) and *total_points are host-known: FLOOR(n_points / downsample) —
 * the reference sizes its cloud with size / downsample, rounded down (:230); when size % downsample != 0 its loop writes one
 * element past the vector (:235-246, undefined behaviour that never grows it), and transformPointCloud, += and
 * convertPointCloudXYZRGBToBuffer (`i < cloud->width`, :253) all iterate the width: the last partial stride's record is not
 * sent. (pcs_stitch_device keeps CEIL(n / downsample): that is the other program's loop, `j += 5 * downsample` while
 * j < buf_len, src/pcs-multicamera-client.cpp:388.) 20 B of HBM traffic per kept record.                                      */
typedef struct pcs_payload_desc {
    const int16_t* d_payload;      /* the camera's packed records (no header), device memory                             */
    int32_t        n_points;
    float          transform[16];  /* transform[i], row-major 4x4 in metres; the last row is not used                    */
} pcs_payload_desc;
int pcs_transform_payloads_device(pcs_ctx* ctx, int n_cams, const pcs_payload_desc* cams, int downsample,
                                  int16_t* d_stitched_payload, size_t stitched_shorts, int* points_per_cam, int* total_points);

/* ---- voxel-grid downsample of a packed payload (BASELINE config 5) ------------------------------ *
 * NOT in the reference (it includes pcl/filters/voxel_grid.h but never instantiates it). Defined in the
 * payload's integer millimetre domain: voxel = floor(coord / leaf_mm) per axis; one output point per occupied
 * voxel = integer mean of x,y,z (truncating) and of R,G,B; output sorted by (z,y,x) voxel, x fastest.
 * The output needs room for n_points points in the worst case. *d_out_points / *out_points = voxels written. The device forms
 * write -1 there if the bucket tail gave up waiting for one of its own workgroups after ~0.5 s (a stalled or preempted device; the
 * wait is bounded so that a launch can end wrong but never hang; it has not been observed outside pcs_inject_voxel_stall): the
 * bytes of such a call are NOT valid. Whoever reads a negative count calls pcs_set_voxel_tail(ctx, PCS_VOXEL_TAIL_LSD_LATCHED) and
 * runs the call again — the LSD tail waits for nobody. Every form of this library that reads the count itself does exactly that
 * (pcs_voxel_grid, libpcs_node's waits, the CLIs) and reports PCS_ERR_HIP only if the second run is negative too: a negative
 * length never reaches a caller's size arithmetic or the wire (src/pcs-multicamera-client.cpp:394-403).
 * The device form is fully asynchronous on the context stream (pre-aggregation, radix sort and segmented mean are
 * hand-written kernels that read their sizes from device memory; no host round trip in the middle).            */
int pcs_voxel_grid_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, int leaf_mm,
                          int16_t* d_out, size_t out_shorts, int32_t* d_out_points);
/* Counted form for device pipelines: the number of points is READ FROM DEVICE MEMORY when the kernels run (e.g. the total
 * pcs_process_frames_device left in d_counts[n_streams] under CUTOFF / DROP_INVALID), max_points is the capacity of the
 * payload (it sizes the workspace; the output needs room for max_points points). BASELINE config 5 — compaction, stitch,
 * voxel grid — then is two asynchronous calls with no host round trip between them.                                */
int pcs_voxel_grid_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                  int leaf_mm, int16_t* d_out, size_t out_shorts, int32_t* d_out_points);
/* Which tail the voxel calls of this context take behind the pre-aggregation. Both give the same bytes for every input:
 *   PCS_VOXEL_TAIL_BUCKET  one partition of the partials into <= 1024 key ranges + one workgroup per range with an LDS table
 *                          (built for the ~1 M partials of BASELINE configs[4] at leaves of a few centimetres and up). The first
 *                          call of a context for a leaf partitions in launches of its own (4 in all); every later call of
 *                          pcs_voxel_grid_device[_counted] / pcs_process_frames_voxel_device has the pre-aggregation put its
 *                          partials into the ranges' regions itself — sized, like the splitters, by the call before — and the tail
 *                          is ONE launch. A cloud that moved costs that call speed (regions overflow into a list that is gathered),
 *                          never bytes. PCS_VOXEL_REGIONS=0 (read at every call) keeps every call on the first call's chain;
 *   PCS_VOXEL_TAIL_LSD     LSD radix sort of (key, partial) + segmented mean (12 launches; the better tool for many millions of
 *                          partials, and the lighter neighbour when the tail runs BESIDE another frame-set's pre-aggregation on the
 *                          same GPU: libpcs_node picks it for its root when one GPU holds every camera);
 *   PCS_VOXEL_TAIL_AUTO    (default) by the leaf: bucket from 34 mm.
 * The environment variable PCS_VOXEL_TAIL=bucket|lsd, read at every call, overrides both (the test-suite runs every voxel
 * test under each).                                                                                                      */
#define PCS_VOXEL_TAIL_AUTO   0
#define PCS_VOXEL_TAIL_BUCKET 1
#define PCS_VOXEL_TAIL_LSD    2
/* after a flagged call (*out_points == -1): LSD from here on for this context, NOT overridable by the environment, both control
 * blocks of the workspace cleared before the next call; counted by pcs_voxel_tail_reruns. AUTO / BUCKET / LSD lift the latch. */
#define PCS_VOXEL_TAIL_LSD_LATCHED 3
int pcs_set_voxel_tail(pcs_ctx* ctx, int tail);
int pcs_voxel_tail_reruns(const pcs_ctx* ctx);     /* how often LSD_LATCHED was set on this context (by the library or the caller) */
/* Fault injection (tests; the CLIs: environment PCS_BKT_INJECT_STALL=<launches>, read once): the next `launches` bucket-tail
 * launches of this PROCESS run with their first workgroup asleep for 0.4 ms and a 20 us wait bound, i.e. they give up and end
 * flagged exactly as a launch on a stalled device would. 0 clears.                                                          */
int pcs_inject_voxel_stall(int launches);

/* Rasters -> voxel grid in one asynchronous call, WITHOUT materialising the stitched cloud: the result (bytes and
 * *d_out_points) is exactly pcs_voxel_grid_device applied to the payload pcs_process_frames_device would write for the
 * same rasters under the context's flags (CUTOFF / DROP_INVALID honoured; the voxel sums are integers, so the order of
 * the points is irrelevant and neither the ordered placement nor the 10-byte records ever touch HBM; 16 x 1920x1080 at
 * a 50 mm leaf: 0.245 ms instead of 0.37 ms for pcs_process_frames_device + pcs_voxel_grid_device_counted). The output
 * needs room for every pixel of the frame-set in the worst case (sum of the streams' n_points). With a downsample
 * stride the stitched cloud is built internally first (the stride is defined on the kept points' ORDER).             */
int pcs_process_frames_voxel_device(pcs_ctx* ctx, const uint16_t* const* d_depth, const uint8_t* const* d_color,
                                    int leaf_mm, int16_t* d_out, size_t out_shorts, int32_t* d_out_points);
int pcs_voxel_grid(pcs_ctx* ctx, const int16_t* payload, int n_points, int leaf_mm,
                   int16_t* out, size_t out_shorts, int* out_points);

/* ---- voxel PARTIALS: the exchange format of a multi-GPU voxel grid (BASELINE configs[4]: 16 streams, 2 per GPU) ---------- *
 * The voxel sums are integers, so the grid of a stitched cloud is the grid of the UNION of its cameras' points in any
 * order: each GPU pre-aggregates its own cameras into partials — one per voxel seen by a patch of pixels: the voxel's key
 * (z, y, x voxel indices packed, a function of leaf_mm alone) and the seven sums — the partials of all GPUs are
 * concatenated on the root (keys with keys, sums with sums; ~40 B per occupied voxel and patch instead of 10 B per point,
 * 7x fewer bytes over xGMI for 16 x 1920x1080 at 50 mm) and ONE sort + segmented mean there gives exactly the bytes
 * pcs_voxel_grid_device would give for the stitched cloud. The reference concatenates the cameras' full payloads on the
 * centre (src/pcs-multicamera-client.cpp:373-409) and has no voxel grid (src/pcs-multicamera-optimized.cpp:17 only
 * includes the header); libpcs_node / pointcloud_stitching_amd.stitch drive the exchange.                                */
typedef struct pcs_voxel_partial {          /* 32 bytes */
    int32_t  sx, sy, sz;                    /* sums of the int16 millimetre coordinates of the points of this partial      */
    uint32_t r, g, b;                       /* sums of the colour bytes                                                      */
    uint32_t n;                             /* points summed (>= 1)                                                          */
    uint32_t pad;
} pcs_voxel_partial;
#define PCS_VOXEL_PARTIAL_WIRE_BYTES 40     /* one uint64 key + one pcs_voxel_partial                                        */

/* Rasters -> partials of this context's streams under its flags (CUTOFF / DROP_INVALID / downsample honoured exactly as
 * pcs_process_frames_voxel_device does). d_keys / d_partials need room for `capacity` >= pcs_max_payload_shorts / 5 entries
 * (worst case: every kept point its own partial); *d_n_partials (device, 4-byte aligned) receives how many were written:
 * it is the kernels' own append counter, cleared by the call — valid once the call's work on the stream is complete, not
 * before. Asynchronous.                                                                                                   */
int pcs_process_frames_voxel_partials_device(pcs_ctx* ctx, const uint16_t* const* d_depth, const uint8_t* const* d_color,
                                             int leaf_mm, uint64_t* d_keys, pcs_voxel_partial* d_partials, size_t capacity,
                                             int32_t* d_n_partials);
/* Partials (of any number of pcs_process_frames_voxel_partials_device calls with the SAME leaf_mm, concatenated in any
 * order) -> the voxel grid. n_partials entries are read, or *d_n_partials (device, <= n_partials, which then is the
 * capacity) when that pointer is given. The output needs room for n_partials points. The partials must be ones this library
 * produced (or obey its bounds: 1 <= n <= 32 768 points per partial, i.e. colour sums < 2^23): 256 of them are summed in 32
 * bits; a voxel whose partials have n == 0 throughout is written with its sums undivided.
 * Asynchronous.                                                                                                           */
int pcs_voxel_grid_from_partials_device(pcs_ctx* ctx, const uint64_t* d_keys, const pcs_voxel_partial* d_partials,
                                        int n_partials, const int32_t* d_n_partials, int leaf_mm, int16_t* d_out,
                                        size_t out_shorts, int32_t* d_out_points);

/* ---- voxel SINK: several contexts of ONE device pre-aggregate into one context's workspace ------------------------------ *
 * pcs_process_frames_voxel_device in three steps, the middle one callable on OTHER contexts of the same device: the partials of
 * every such context land where the sink context's own would — in its buckets' regions on a warm call — so nothing is exchanged,
 * concatenated or placed, and the tail is the one launch of a warm call. libpcs_node takes this route for peers that share the
 * root's GPU (a device id that repeats); peers on OTHER GPUs exchange partials (above): the pre-aggregation's atomics are
 * device-scope and a sink refuses a context of another device.
 *   pcs_voxel_sink_begin   on the sink context's stream: workspace for `capacity_points` (the sum of every participating context's
 *                          pixels), control blocks; fills *sink (opaque; valid until the finish). One sink per context at a time — a
 *                          second begin abandons the first.
 *   pcs_process_frames_voxel_into_sink_device   on ctx's stream: ctx's rasters under ctx's flags (CUTOFF / DROP_INVALID / downsample,
 *                          as pcs_process_frames_voxel_partials_device) into the sink. The CALLER orders the streams: this launch behind
 *                          the begin (when sink->work_enqueued) and behind the sink's previous finish, the finish behind every such
 *                          launch — events, as libpcs_node does (csrc/pcs_node.cpp: enqueue_sink_ticket).
 *   pcs_voxel_sink_finish  on the sink context's stream: the tail; bytes, *d_out_points and the -1 convention exactly as
 *                          pcs_process_frames_voxel_device over the union of the participating rasters. d_out needs room for
 *                          capacity_points points.                                                                                  */
typedef struct pcs_voxel_sink {
    uint64_t opaque[23];
    uint32_t work_enqueued;   /* begin put work on the sink's stream (the clear of a workspace's control blocks: its first call, or after a
                                 call that failed half-way) that the pre-aggregations must run behind; 0: nothing to order against the begin */
    uint32_t reserved;
} pcs_voxel_sink;
int pcs_voxel_sink_begin(pcs_ctx* sink_ctx, size_t capacity_points, int leaf_mm, pcs_voxel_sink* sink);
int pcs_process_frames_voxel_into_sink_device(pcs_ctx* ctx, const uint16_t* const* d_depth, const uint8_t* const* d_color,
                                              const pcs_voxel_sink* sink);
int pcs_voxel_sink_finish(pcs_ctx* sink_ctx, const pcs_voxel_sink* sink, int16_t* d_out, size_t out_shorts, int32_t* d_out_points);

/* ---- payload compression for the wire: the "PCZ1" container (not in the reference: its -z is a TODO, :55, 145-147) ------------- *
 * Lossless and deterministic: a payload has exactly one container, so encoders are compared byte for byte (the GPU's against
 * tests/np_payload_codec.py). The format is this project's own; DESIGN.md section 4 defines it precisely enough to write a decoder
 * from. Everything little-endian; a payload of n records (n >= 0) is cut into blocks of 64 consecutive records:
 *    0 uint32 magic 0x315A4350 ("PCZ1")   4 uint32 n_points   8 uint32 n_blocks = ceil(n / 64)   12 uint32 total_bytes (multiple of 4)
 *   16 uint32 block_end[n_blocks]: byte offset from the container's start of the END of block b; then the blocks, back to back.
 *   A block: 16-byte header (record 0's seven channels x, y, z: uint16, R, G, B, P: uint8; a uint32 of the channels' bit widths; two
 *   zero bytes), then per channel the zigzag deltas of records 1.. against their predecessor in the block, bit-packed at the width of
 *   the largest. Nothing crosses a block. P is the high byte of a record's fifth short (0 in what this library writes).
 * pcs_compressed_bound: 16 + 660 ceil(n / 64): the largest container of n records (no GPU, no context; 0 for n < 0).
 * pcs_compressed_info: pure host code, no context, no GPU: validates EVERYTHING a decoder relies on — size >= 16, magic, n_blocks,
 *   n_points <= INT32_MAX / 10, total_bytes == n_bytes and a multiple of 4, the table inside the container, block_end strictly
 *   increasing from the data's start and ending at total_bytes, per block the widths (<= 16 / <= 8), the reserved bits and the size
 *   its widths imply; padding bits inside words are not checked — and fills *out (optional). PCS_ERR_INVALID_ARG with the first
 *   violation in pcs_last_error(NULL).
 * pcs_compress_payload_device: asynchronous on the context's stream, three launches (block sizes, offsets, emit). d_payload: n_points
 *   records; d_out: the container, at most pcs_compressed_bound(n_points) bytes are written; *d_out_bytes (device, optional) its size,
 *   which is also at byte 12 of the container. out_capacity < pcs_compressed_bound(n_points) is PCS_ERR_CAPACITY up front: capacity is
 *   never data dependent. All three pointers 4-byte aligned (the reference's `buffer + 2` shorts is); d_payload sharing a byte with
 *   d_out's first pcs_compressed_bound(n_points) bytes is PCS_ERR_INVALID_ARG. n_points 0 gives the 16-byte container. The block-size
 *   scratch (4 bytes per 64 records) lives in the context and grows on demand.
 * pcs_decompress_payload_device: asynchronous, one launch. The CALLER VOUCHES for the container (pcs_compressed_info accepted these
 *   in_bytes bytes and reported n_points); the host checks what it can see (alignment, payload_shorts >= 5 n_points, the table fits
 *   in_bytes) and the kernel reads nothing at or beyond in_bytes and writes nothing at or beyond record n_points whatever the bytes
 *   say — a container that was never validated decodes to garbage, not out of bounds.
 * pcs_decompress_payload: `in` is HOST memory: pcs_compressed_info first (its status and text are returned, nothing is uploaded or
 *   launched on failure), upload, decode into d_payload (device), *n_points = records written. Synchronous.
 * pcs_process_frames_compressed: pcs_process_frames with the payload kept on the device and compressed there; only the container
 *   crosses the link. out (host): [int32 container bytes, written if write_header][container at byte 4]; *out_bytes = container
 *   bytes; counts as points_per_stream. out_capacity < 4 + pcs_compressed_bound(pcs_max_payload_shorts / 5) is PCS_ERR_CAPACITY up
 *   front. Synchronous; rasters are staged (no zero-copy route).
 * All of these work on every context: flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH only decide which records exist.
 * Measured (python tools/codec_probe.py 200 20; 8 x 1280x720 = 7.37 M records, one MI355X, payloads and containers cold from HBM,
 *   per-call event pairs, median / minimum of 200 calls): container / raw bytes 0.766 for the synthetic scene, 0.567 with invalid-depth
 *   drop (0.737 / 0.328 with a smooth colour raster; ratios depend on the data, none is promised); encode 200.2 / 198.1 us, decode
 *   69.3 / 68.1 us (with the drop: 180.3 / 179.0 and 60.3 / 59.3) against byte floors of 25.5 and 16.3 us - correct, bounded, and far
 *   from the floor. pcs_process_frames_compressed against pcs_process_frames, page-locked buffers: 2.08 against 1.69 ms dense (the
 *   uncompressed call runs zero copy: compression does NOT pay on the host link there), 1.75 against 1.84 ms with the drop. The wire
 *   saving stands on the byte count alone. DESIGN.md section 10 (f8).                                                               */
struct pcs_compressed_info {
    uint32_t n_points;
    uint32_t n_blocks;
    uint32_t total_bytes;
    uint32_t data_offset;      /* where block 0 starts: 16 + 4 n_blocks */
};
size_t pcs_compressed_bound(int n_points);
int pcs_compressed_info(const void* bytes, size_t n_bytes, struct pcs_compressed_info* out);
int pcs_compress_payload_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, void* d_out, size_t out_capacity,
                                uint32_t* d_out_bytes);
int pcs_decompress_payload_device(pcs_ctx* ctx, const void* d_in, size_t in_bytes, int n_points, int16_t* d_payload,
                                  size_t payload_shorts);
int pcs_decompress_payload(pcs_ctx* ctx, const void* in, size_t in_bytes, int16_t* d_payload, size_t payload_shorts, int* n_points);
int pcs_process_frames_compressed(pcs_ctx* ctx, const uint16_t* const* depth, const uint8_t* const* color, void* out,
                                  size_t out_capacity, int write_header, int* counts, int* out_bytes);

/* ---- radius outlier removal on a packed payload (not in the reference: its centre programs include PCL's filters, unused) -------- *
 * Record i of n (5 shorts; 0..2 = x, y, z as signed int16 millimetres, 3..4 colour, not looked at) is KEPT iff
 *     |{ j != i : (xi-xj)^2 + (yi-yj)^2 + (zi-zj)^2 <= radius_mm^2 }| >= min_neighbors
 * in integers of 32 bits or more from the sign-extended shorts (32767 and -32768 are 65535 mm apart; nothing wraps at 16 bits; no
 * floats anywhere). j != i is by index: a record with another's coordinates is its neighbour at distance 0. The output is the kept
 * records in input order, all 10 bytes of each unchanged (the high byte of short 4 included), and their count. Exact and
 * deterministic: the same bytes for the same input on every run (tests/np_radius_outlier.py restates it as brute force). Modelled on
 * PCL's RadiusOutlierRemoval; parity with PCL is unpinned. DESIGN.md section 3 has the definition and what follows from it: the
 * filter knows nothing of invalid depth (a dense payload's zero-depth pixels all sit on their camera's origin and keep each other:
 * run it behind PCS_FLAG_DROP_INVALID or a crop box), and the result does not depend on record order except for the output's own.
 * radius_mm 1..1000, min_neighbors 1..255.
 * pcs_radius_outlier_device: asynchronous on the context's stream, ten launches, no host round trip (a uniform grid of cell edge
 *   radius_mm in an open-addressing table built per call, a scatter into cell order, one lane per record over its 27 cells with an
 *   exit at min_neighbors, then the ordered compaction). d_out needs room for the worst case, n_points records: out_shorts >=
 *   5 n_points is checked up front; nothing outside the first 10 * kept bytes of d_out is written. *d_out_points (device, 4-byte
 *   aligned, required) receives kept. n_points 0 launches nothing and writes a zero count.
 * pcs_radius_outlier_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when the kernels run, clamped to
 *   0..max_points; max_points sizes the workspace, the grids and the output check. What a compaction's or another filter's device
 *   count feeds; its own output and count feed pcs_voxel_grid_device_counted.
 * pcs_radius_outlier: host pointers, staged through the context, synchronous.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the argument), nothing launched, nothing written: radius_mm or
 *   min_neighbors out of range, a negative count, a NULL pointer (payload and output may be NULL with a count of 0), an odd payload
 *   or output address, a misaligned count word, out_shorts below the worst case, any overlap of the input, output and count ranges.
 * Works on every context: flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH are not read. The workspace (40.2 bytes per record
 *   of n_points / max_points: csrc/pcs_kernels_outlier.hip) lives in the context and grows on demand. A record costs at most the
 *   population of its 27 cells; n identical records cost n (min_neighbors + 1) distance tests. With pcs_kernel_timing enabled a call
 *   yields one interval per launch (10). Measured: DESIGN.md section 10 (f9), profiles/outlier_probe.txt.                          */
#define PCS_OUTLIER_RADIUS_MIN     1
#define PCS_OUTLIER_RADIUS_MAX     1000
#define PCS_OUTLIER_NEIGHBORS_MIN  1
#define PCS_OUTLIER_NEIGHBORS_MAX  255
int pcs_radius_outlier_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, int radius_mm, int min_neighbors,
                              int16_t* d_out, size_t out_shorts, int32_t* d_out_points);
int pcs_radius_outlier_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                      int radius_mm, int min_neighbors, int16_t* d_out, size_t out_shorts, int32_t* d_out_points);
int pcs_radius_outlier(pcs_ctx* ctx, const int16_t* payload, int n_points, int radius_mm, int min_neighbors,
                       int16_t* out, size_t out_shorts, int* out_points);   /* host pointers, staged, synchronous */

/* ---- statistical outlier removal on a packed payload (not in the reference) ------------------------------------------------------ *
 * The radius filter's threshold is absolute; this one is relative to the cloud's own density. n records of 5 shorts (0..2 = x, y, z
 * as signed int16 millimetres; colour is not read), mean_k 1..64, std_mul_milli 0..10000 (thousandths), max_dist_mm 1..1000 (the
 * cell edge of the index and the search bound). Everything is integer; no float is converted, compared or stored.
 *   N_i       = { j != i : d2_ij <= max_dist_mm^2 }, d2 in integers of 32 bits or more from the sign-extended shorts (nothing wraps
 *               at 16 bits); j != i is by index: a record with another's coordinates is its neighbour at distance 0.
 *   SPARSE    record i iff |N_i| < mean_k: dropped, and not part of the statistics.
 *   D_i       otherwise: the sum of isqrt(65536 d2) over the mean_k smallest d2 of N_i (a multiset: ties are interchangeable), isqrt
 *               the exact integer floor square root. Unit 1/256 mm, summed, not divided by mean_k; below 2^24.
 *   M, S1, S2 the number of non-sparse records, sum D_i, sum D_i^2 (exact: each D_i^2 as t & 0xFFFFFFFF and t >> 32, summed apart:
 *               S2 = s2_lo + 2^32 s2_hi). W = M S2 - S1^2 in 128-bit integers.
 *   T         sigma_q = isqrt(floor((W << 16) / (M (M - 1)))) for M >= 2, else 0 (the sample deviation in 1/256 of a D unit);
 *               T = floor((256000 S1 + std_mul_milli M sigma_q) / (256000 M)), 0 when M = 0.
 *   KEPT      record i iff it is not sparse and D_i <= T.
 * The output is the kept records in input order, all 10 bytes of each unchanged, their count, and (optional) the statistics block
 * of eight int64: considered, dense (= M), s1, s2_lo, s2_hi, threshold (= T), kept, reserved (0). Exact and deterministic: a function
 * of the payload as a multiset except for the output's own order, the same bytes on every run (tests/np_stat_outlier.py restates it
 * as brute force). Modelled on PCL's StatisticalOutlierRemoval; parity with PCL is unpinned. DESIGN.md section 3 has the definition
 * and what follows from it: a dense payload's zero-depth pixels sit on one point, have D = 0 and drag the mean down (run the filter
 * behind PCS_FLAG_DROP_INVALID or a crop box); max_dist_mm bounds both the cost and who counts as sparse; std_mul_milli 0 drops
 * about half of a smooth cloud.
 * pcs_stat_outlier_device: asynchronous on the context's stream, no host round trip: the radius filter's cell index with edge
 *   max_dist_mm (six launches), a k-nearest search per record over its 27 cells, the sums, the threshold (one lane, 128-bit
 *   integers), the keep bits, then that filter's ordered compaction (three launches) and, with d_stats, the block: 14 launches, 13
 *   without. d_out needs room for the worst case: out_shorts >= 5 n_points is checked up front; nothing outside the first 10 * kept
 *   bytes of d_out is written. *d_out_points (device, 4-byte aligned, required) receives kept; d_stats (device, 8-byte aligned,
 *   optional) the block. n_points 0 launches nothing and writes a zero count and a zeroed block (considered = 0).
 * pcs_stat_outlier_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when the kernels run, clamped to
 *   0..max_points; max_points sizes the workspace, the grids and the output check. It takes pcs_radius_outlier_device_counted's
 *   output and count, and its own feed pcs_voxel_grid_device_counted.
 * pcs_stat_outlier: host pointers, staged through the context, synchronous; stats optional.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: a
 *   parameter out of range or reserved != 0, NULL params, a negative count, a NULL pointer (payload and output may be NULL with a
 *   count of 0), an odd payload or output address, a misaligned count or stats address, out_shorts below the worst case, any
 *   overlap among the input, output, count and stats ranges.
 * Works on every context: flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH are not read. The workspace (the radius filter's
 *   40.2 bytes per record of n_points / max_points plus 4.1: csrc/pcs_kernels_stat.hip) lives in the context and grows on demand.
 *   Cost: a record costs the population of the cells around it that it cannot rule out (a cell whose nearest corner is no nearer
 *   than the record's mean_k-th value so far is skipped), plus 2 log2(mean_k + 1) list reads per value that enters its full list;
 *   there is no early exit: n identical records cost n^2 distance tests. With pcs_kernel_timing enabled a call yields one
 *   interval per launch. Measured: DESIGN.md section 10 (f12), profiles/stat_outlier_probe.txt.                                    */
#define PCS_STAT_K_MIN          1
#define PCS_STAT_K_MAX          64
#define PCS_STAT_MUL_MILLI_MAX  10000
#define PCS_STAT_DIST_MIN       1
#define PCS_STAT_DIST_MAX       1000
typedef struct pcs_stat_outlier_params {
    int32_t mean_k, std_mul_milli, max_dist_mm, reserved;   /* reserved is 0 */
} pcs_stat_outlier_params;
struct pcs_stat_outlier_stats {
    int64_t considered, dense, s1, s2_lo, s2_hi, threshold, kept, reserved;
};
int pcs_stat_outlier_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_stat_outlier_params* params,
                            int16_t* d_out, size_t out_shorts, int32_t* d_out_points, struct pcs_stat_outlier_stats* d_stats);
int pcs_stat_outlier_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                    const pcs_stat_outlier_params* params, int16_t* d_out, size_t out_shorts,
                                    int32_t* d_out_points, struct pcs_stat_outlier_stats* d_stats);
int pcs_stat_outlier(pcs_ctx* ctx, const int16_t* payload, int n_points, const pcs_stat_outlier_params* params,
                     int16_t* out, size_t out_shorts, int* out_points, struct pcs_stat_outlier_stats* stats);   /* host pointers, staged, synchronous */

/* ---- Euclidean cluster extraction and size filter on a packed payload (not in the reference) ------------------------------------ *
 * Both outlier filters judge a record by its own neighbourhood; a DENSE blob of stray records passes both. This one finds the
 * connected components and judges them by their size. n records of 5 shorts (0..2 = x, y, z as signed int16 millimetres; colour is
 * not read), tolerance_mm 1..1000 (the cell edge of the index). Everything is integer; no float anywhere.
 *   i ~ j     iff (xi-xj)^2 + (yi-yj)^2 + (zi-zj)^2 <= tolerance_mm^2, in integers of 32 bits or more from the sign-extended shorts
 *               (nothing wraps at 16 bits). A record with another's coordinates is adjacent to it at distance 0.
 *   CLUSTER   a connected component of ~. size(i) = the number of records in i's cluster (duplicates count one each).
 *   label(i)  the smallest input index in i's cluster: label(i) <= i, a cluster's first record labels itself;
 *               n_clusters = |{ i : label(i) == i }|.
 *   KEPT      record i iff min_size <= size(i) and (max_size == 0 or size(i) <= max_size). min_size 1..INT_MAX; max_size 0 (no upper
 *               bound) or >= min_size.
 * The filter's output is the kept records in input order, all 10 bytes of each unchanged, their count, and (optional) the statistics
 * block of eight int64: considered, clusters, kept_clusters, largest (the largest cluster's size), kept, reserved (0, 0, 0). Exact and
 * deterministic: the same bytes on every run, whatever order the atomics arrive in; a function of the payload as a multiset except
 * for the output's own order (and the labels' renaming under a permutation). tests/np_clusters.py restates it as brute force.
 * Modelled on PCL's EuclideanClusterExtraction; parity with PCL is unpinned. DESIGN.md section 3 has the definition and what follows
 * from it: the filter knows nothing of invalid depth (a dense payload's zero-depth pixels form one huge cluster on their camera's
 * origin: run it behind PCS_FLAG_DROP_INVALID or a crop box).
 * pcs_cluster_filter_device: asynchronous on the context's stream, no host round trip: the radius filter's cell index with edge
 *   tolerance_mm (six launches), init, union (a lock-free union-find over the index's entries: one lane per entry unites it with
 *   every entry below it within the tolerance), roots (every entry's final root, the sizes), flag (the keep bits), then that
 *   filter's ordered compaction (three launches) and, with d_stats, the block: 14 launches, 13 without. d_out needs room for the
 *   worst case: out_shorts >= 5 n_points is checked up front; nothing outside the first 10 * kept bytes of d_out is written.
 *   *d_out_points (device, 4-byte aligned, required) receives kept; d_stats (device, 8-byte aligned, optional) the block. n_points 0
 *   launches nothing and writes a zero count and a zeroed block.
 * pcs_cluster_filter_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when the kernels run, clamped to
 *   0..max_points; max_points sizes the workspace, the grids and the output check. It takes the other filters' output and count,
 *   and its own feed pcs_voxel_grid_device_counted.
 * pcs_cluster_filter: host pointers, staged through the context, synchronous; stats optional.
 * pcs_cluster_labels_device: labels instead of a filtered payload: d_labels (device, 4-byte aligned, n_points int32, required with
 *   n_points > 0) receives label(i), d_sizes (the same shape, optional) size(i), *d_n_clusters (device, 4-byte aligned, required)
 *   n_clusters; nothing at or beyond word n_points of either array is written. 11 launches. n_points 0 launches nothing and writes
 *   zero clusters. pcs_cluster_labels: the host form, synchronous.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: a
 *   parameter out of range, reserved != 0, max_size in 1..min_size-1, NULL params, a negative count, a NULL pointer (payload and
 *   outputs may be NULL with a count of 0), an odd payload or output address, a misaligned count, stats, labels or sizes address,
 *   out_shorts below the worst case, any overlap among the input and output ranges.
 * Works on every context: flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH are not read. The workspace (the radius filter's
 *   40.2 bytes per record of n_points / max_points plus 12: csrc/pcs_kernels_cluster.hip) lives in the context and grows on demand.
 *   Cost: a record costs the population of the cells around it that it cannot rule out and two root searches per adjacent record;
 *   there is no early exit: a cell of m records costs m^2 / 2 distance tests by definition (n identical records: n^2 / 2). With
 *   pcs_kernel_timing enabled a call yields one interval per launch. Measured: DESIGN.md section 10 (f13),
 *   profiles/cluster_probe.txt.                                                                                                    */
#define PCS_CLUSTER_TOLERANCE_MIN  1
#define PCS_CLUSTER_TOLERANCE_MAX  1000
typedef struct pcs_cluster_params {
    int32_t tolerance_mm, min_size, max_size, reserved;   /* max_size 0: no upper bound; reserved is 0 */
} pcs_cluster_params;
struct pcs_cluster_stats {
    int64_t considered, clusters, kept_clusters, largest, kept, reserved[3];
};
int pcs_cluster_filter_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_cluster_params* params,
                              int16_t* d_out, size_t out_shorts, int32_t* d_out_points, struct pcs_cluster_stats* d_stats);
int pcs_cluster_filter_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                      const pcs_cluster_params* params, int16_t* d_out, size_t out_shorts,
                                      int32_t* d_out_points, struct pcs_cluster_stats* d_stats);
int pcs_cluster_filter(pcs_ctx* ctx, const int16_t* payload, int n_points, const pcs_cluster_params* params,
                       int16_t* out, size_t out_shorts, int* out_points, struct pcs_cluster_stats* stats);   /* host pointers, staged, synchronous */
int pcs_cluster_labels_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, int tolerance_mm, int32_t* d_labels,
                              int32_t* d_sizes, int32_t* d_n_clusters);
int pcs_cluster_labels(pcs_ctx* ctx, const int16_t* payload, int n_points, int tolerance_mm, int32_t* labels, int32_t* sizes,
                       int* n_clusters);   /* host pointers, staged, synchronous */

/* ---- Cluster objects: per-cluster box and sums (not in the reference) -------------------------------------------------------------- *
 * What the clusters that pass the size filter ARE, from the call that filters: one index build and one union. Adjacency, clusters,
 * size(i), label(i) and KEPT are those above with the same pcs_cluster_params. Integer only; no float anywhere.
 *   OBJECT        a cluster with min_size <= size and (max_size == 0 or size <= max_size). Objects are numbered k = 0 .. n_objects-1
 *                   by ascending label (the input index of their first record); n_objects equals the filter's kept_clusters.
 *   object_of(i)  the k of record i's cluster, -1 where it is no object: the true k, also where k >= max_objects.
 *   object k      over its member records, coordinates sign-extended from the shorts: label, size; lo[a] / hi[a] the minimum /
 *                   maximum of coordinate a (an inclusive box); sum_xyz[a] the sum of coordinate a (|sum| < 2^47);
 *                   sum_rgb = (sum R, sum G, sum B) with R = short3 & 0xFF, G = (short3 >> 8) & 0xFF, B = short4 & 0xFF (the high
 *                   byte of short 4 is not read). Sums, not means: they are exact and add across shards; the consumer divides.
 * The table holds the first min(n_objects, max_objects) objects, each entry written whole (80 bytes, reserved words 0);
 * *n_objects always receives the full count. Nothing at or beyond entry min(n_objects, max_objects), and nothing at or beyond word
 * n of object_of, is written. Exact and deterministic: the same bytes on every run, whatever order the atomics arrive in; under a
 * permutation of the records the table is the same multiset of (size, lo, hi, sum_xyz, sum_rgb), only label, the order and object_of
 * follow the permutation. tests/np_cluster_objects.py restates it.
 * pcs_cluster_objects_device: asynchronous on the context's stream, no host round trip. `out` is a HOST struct of device pointers,
 *   read at call time: objects (8-byte aligned, max_objects entries; NULL iff max_objects == 0), max_objects 0..PCS_CLUSTER_OBJECTS_MAX,
 *   reserved 0, n_objects (required, 4-byte aligned), object_of (optional, n int32, 4-byte aligned), out / out_shorts / out_points
 *   (optional, both pointers or neither: the filtered payload, whose bytes, count and rule out_shorts >= 5 n are exactly
 *   pcs_cluster_filter_device's for the same arguments), stats (optional, that filter's block, unchanged meaning; without `out`
 *   its `kept` is still the kept record count). Launches: the filter's index, init, union and roots (9), then record roots, firsts,
 *   first scan, slots, accumulate, finish (6): 15; with `out` the filter's flag, tile count, tile scan and emit in between: 19;
 *   with stats one more (and, without `out`, flag, tile count and tile scan for its kept count: 19). n_points 0 launches nothing and
 *   writes n_objects = 0, a zero out_points and a zeroed block.
 * pcs_cluster_objects_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when the kernels run, clamped to
 *   0..max_points; max_points sizes the workspace, the grids and the output checks; records at or beyond the count are never read
 *   as records, object_of is written below the device count only.
 * pcs_cluster_objects: host pointers, staged through the context, synchronous; object_of optional.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: every
 *   refusal of pcs_cluster_filter_device*; a NULL out struct; max_objects outside 0..PCS_CLUSTER_OBJECTS_MAX; objects NULL with
 *   max_objects > 0 or not 8-byte aligned; reserved != 0; out without out_points or the reverse; n_objects NULL or misaligned; a
 *   misaligned object_of; any overlap among the input and all output ranges.
 * Works on every context: flags, crop box and downsample are not read. The workspace is the cluster filter's plus 8.13 bytes per
 *   record of n_points / max_points (the record's root, its root's object, the firsts' bitmap and tile words) and 80 bytes per object
 *   of max_objects, in the same slab of the context, grown on demand. With pcs_kernel_timing enabled a call yields one interval per
 *   launch. Measured: DESIGN.md section 10 (f15), profiles/objects_probe.txt.                                                      */
#define PCS_CLUSTER_OBJECTS_MAX 65536
typedef struct pcs_cluster_object {          /* 80 bytes, 8-byte aligned */
    int32_t label, size;
    int16_t lo[3], hi[3];
    int32_t reserved0;                       /* 0 */
    int64_t sum_xyz[3];
    int64_t sum_rgb[3];
    int64_t reserved1;                       /* 0 */
} pcs_cluster_object;
typedef struct pcs_cluster_objects_out {     /* host struct of device pointers, read at call time */
    pcs_cluster_object* objects; int32_t max_objects; int32_t reserved;   /* objects may be NULL iff max_objects == 0 */
    int32_t* n_objects;                      /* required, 4-byte aligned */
    int32_t* object_of;                      /* optional, n int32 */
    int16_t* out; size_t out_shorts; int32_t* out_points;   /* optional filtered payload: out and out_points both or neither */
    struct pcs_cluster_stats* stats;         /* optional, the filter's block, unchanged meaning */
} pcs_cluster_objects_out;
int pcs_cluster_objects_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_cluster_params* params,
                               const pcs_cluster_objects_out* out);
int pcs_cluster_objects_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                       const pcs_cluster_params* params, const pcs_cluster_objects_out* out);
int pcs_cluster_objects(pcs_ctx* ctx, const int16_t* payload, int n_points, const pcs_cluster_params* params,
                        pcs_cluster_object* objects, int max_objects, int* n_objects, int32_t* object_of);   /* host pointers, staged, synchronous */

/* ---- RANSAC plane segmentation on a packed payload (not in the reference) --------------------------------------------------------- *
 * Connectivity is transitive: everything that stands on a floor is one cluster through the floor. This call takes the dominant planes
 * (floor, walls, a table) out of the cloud, or hands them out, between the outlier filters and the cluster filter. n records of 5
 * shorts (0..2 = x, y, z as signed int16 millimetres; colour is not read). Everything is integer; no float anywhere.
 *   ROUND r   works on the m records that are in no plane accepted so far, in input order (round 0: all of them). Hypothesis h
 *               (0 .. iterations - 1) draws three positions i_k = ((splitmix64(key) >> 32) * m) >> 32, key = seed << 32 | r << 20 |
 *               h << 2 | k, k = 0, 1, 2 (splitmix64: z = key + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *               z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31, modulo 2^64).
 *   PLANE     of the drawn records p0, p1, p2: N = (p1 - p0) x (p2 - p0) (|component| <= 2 * 65535^2, int64), off = N . p0,
 *               T = isqrt(distance_mm^2 * |N|^2), the exact integer square root of a value below 2^88. N = 0 (equal or collinear
 *               draws): the hypothesis is DEGENERATE and scores nothing. The sign of N is whatever the draws give.
 *   INLIER    record p iff |N . p - off| <= T in int64: exactly (N . (p - p0))^2 <= distance_mm^2 |N|^2, a distance to the plane of at
 *               most distance_mm.
 *   WINNER    the hypothesis with the most inliers among the round's m records; on a tie the smallest h. m < 3, or a winner with fewer
 *               than min_inliers inliers (every hypothesis degenerate: 0), ends the segmentation: n_planes = r. Otherwise plane r is
 *               accepted: its inliers get label r and leave the cloud. No refit of the winner on its inliers. max_planes rounds at most.
 *   OUTPUT    labels forms: int32 label(i) in {-1, 0, .., n_planes - 1} per record, and n_planes. Filter forms: the kept records in
 *               input order, all 10 bytes of each unchanged, and their count; kept = the records in NO accepted plane (mode 0) or in
 *               one (mode 1). Both: (optional) max_planes blocks of pcs_plane_model, those from n_planes on zeroed (sample[] = the INPUT
 *               indices of the drawn records), and (optional) the statistics block of eight int64: considered, planes, inliers_total,
 *               kept, largest_plane, degenerate_hypotheses (over the rounds that drew: those with m >= 3), 0, 0.
 * Exact and deterministic: a function of the payload in its order, the parameters and the seed; the same bytes on every run, whatever
 * order the atomics arrive in. tests/np_planes.py restates it as brute force. Modelled on PCL's SACSegmentation with SACMODEL_PLANE;
 * parity with PCL is unpinned. DESIGN.md section 3 has the definition and what follows from it.
 * pcs_plane_segment_device: asynchronous on the context's stream, no host round trip: init, then per round hypotheses (one lane per
 *   hypothesis), score (iterations x m inlier tests: the hot launch), select and mark, between two rounds the radius filter's ordered
 *   compaction (three launches) and the origin indices behind it; at the end finish (the keep bits of the whole input by label, the
 *   model and statistics blocks) and that compaction once more: 8 max_planes + 1 launches. A round after the segmentation ended
 *   launches and does nothing; no count leaves the device between rounds. d_out needs room for the worst case: out_shorts >=
 *   5 n_points is checked up front; nothing outside the first 10 * kept bytes of d_out is written. *d_out_points (device, 4-byte
 *   aligned, required) receives kept; d_models (device, 8-byte aligned, optional) max_planes blocks; d_stats (device, 8-byte aligned,
 *   optional) the block. n_points 0 launches nothing and writes a zero count and zeroed blocks.
 * pcs_plane_segment_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when the kernels run, clamped to
 *   0..max_points; max_points sizes the workspace, the grids and the output check. It takes the other filters' output and count,
 *   and its own feed pcs_cluster_filter_device_counted and pcs_voxel_grid_device_counted.
 * pcs_plane_segment: host pointers, staged through the context, synchronous; models and stats optional.
 * pcs_plane_labels_device: labels instead of a filtered payload: d_labels (device, 4-byte aligned, n_points int32, required with
 *   n_points > 0), *d_n_planes (device, 4-byte aligned, required); nothing at or beyond word n_points of d_labels is written.
 *   8 max_planes - 2 launches. pcs_plane_labels: the host form, synchronous.
 * pcs_plane_count_inliers_device: the caller's own candidate planes, n_models (1..4096) blocks in HOST memory (nx, ny, nz, off and
 *   threshold are read), scored by the same score launch over a device payload: d_counts[j] (device, 8-byte aligned, n_models int64)
 *   = the number of records with |N_j . p - off_j| <= threshold_j. The models leave the host before the call returns (the copy
 *   waits for the stream's earlier work); the scoring is asynchronous. n_points 0 writes zero counts.
 *   Refused: |nx|, |ny| or |nz| above 2^34, |off| above 2^52, threshold outside 0..2^52, nx = ny = nz = 0.
 * pcs_plane_from_points: no context, no device: the model of three records p0, p1, p2 (3 shorts each are read) at distance_mm, as a
 *   hypothesis that drew them would build it (inliers 0, sample 0 1 2, hypothesis 0). PCS_ERR_INVALID_ARG for a NULL pointer, a
 *   distance out of range or a degenerate triple (*model is zeroed for the latter).
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: a
 *   parameter out of range, a reserved word != 0, NULL params, a negative count, a NULL pointer (payload and outputs may be NULL with a
 *   count of 0), an odd payload or output address, a misaligned count, labels, models, counts or stats address, out_shorts below the
 *   worst case, any overlap among the input and output ranges.
 * Works on every context: flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH are not read. The workspace (the radius filter's
 *   plus 32 bytes per record of n_points / max_points and 0.25 MB: csrc/pcs_kernels_plane.hip) lives in the context and grows on
 *   demand. Cost: iterations x m inlier tests per round. With pcs_kernel_timing enabled a call yields one interval per launch.
 *   Measured: DESIGN.md section 10 (f14), profiles/plane_probe.txt.                                                                 */
#define PCS_PLANE_DISTANCE_MIN     1
#define PCS_PLANE_DISTANCE_MAX     1000
#define PCS_PLANE_ITERATIONS_MAX   4096
#define PCS_PLANE_MAX_PLANES       8
#define PCS_PLANE_MODE_REMOVE      0
#define PCS_PLANE_MODE_KEEP        1
typedef struct pcs_plane_params {
    int32_t  distance_mm, iterations, min_inliers, max_planes;
    uint32_t seed;
    int32_t  mode, reserved[2];                           /* reserved words are 0 */
} pcs_plane_params;
typedef struct pcs_plane_model {
    int64_t nx, ny, nz, off, threshold, inliers;
    int32_t sample[3], hypothesis;
} pcs_plane_model;
struct pcs_plane_stats {
    int64_t considered, planes, inliers_total, kept, largest_plane, degenerate_hypotheses, reserved[2];
};
int pcs_plane_segment_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_plane_params* params, int16_t* d_out,
                             size_t out_shorts, int32_t* d_out_points, pcs_plane_model* d_models, struct pcs_plane_stats* d_stats);
int pcs_plane_segment_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                     const pcs_plane_params* params, int16_t* d_out, size_t out_shorts, int32_t* d_out_points,
                                     pcs_plane_model* d_models, struct pcs_plane_stats* d_stats);
int pcs_plane_segment(pcs_ctx* ctx, const int16_t* payload, int n_points, const pcs_plane_params* params, int16_t* out, size_t out_shorts,
                      int* out_points, pcs_plane_model* models, struct pcs_plane_stats* stats);   /* host pointers, staged, synchronous */
int pcs_plane_labels_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_plane_params* params, int32_t* d_labels,
                            int32_t* d_n_planes, pcs_plane_model* d_models, struct pcs_plane_stats* d_stats);
int pcs_plane_labels(pcs_ctx* ctx, const int16_t* payload, int n_points, const pcs_plane_params* params, int32_t* labels, int* n_planes,
                     pcs_plane_model* models, struct pcs_plane_stats* stats);   /* host pointers, staged, synchronous */
int pcs_plane_count_inliers_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_plane_model* models, int n_models,
                                   int64_t* d_counts);
int pcs_plane_from_points(const int16_t* p0, const int16_t* p1, const int16_t* p2, int distance_mm, pcs_plane_model* model);

/* ---- background model and subtraction on packed payloads (not in the reference) --------------------------------------------------- *
 * The plane filter takes out a floor and a wall; a fixed rig also sees shelves, a truss, tables, a net — in every frame-set. This is a
 * change detector against a LEARNED background: one persistent table, learned once, probed per record, no index build per call.
 * Everything is in the payload's integer millimetres (shorts 0..2 = x, y, z signed; colour is not read); no float anywhere.
 *   CELL      of a record: floor(v / cell_mm) + 32768 per axis, 0..65535; cell_mm 1..1000. Negative coordinates floor.
 *   MODEL     a map cell -> seen (uint32 >= 1), a counter `frames`, a sticky `overflow` flag, and its constants cell_mm and max_cells.
 *   LEARN     of a payload: frames += 1; every DISTINCT cell that holds at least one of its records gets seen += 1 (a new cell enters
 *               with seen = 1). Zero records still count as a frame. The result depends neither on the record order nor on how often
 *               a cell is hit within one call. frames stops at PCS_BACKGROUND_FRAMES_MAX: a learn call at the cap is refused.
 *   OVERFLOW  set when a learn call takes the number of distinct cells above max_cells; it stays set until reset. Which of the surplus
 *               cells got in is unspecified (and `cells` may then exceed max_cells). There is no hang and no write outside the table.
 *   SUBTRACT  record i in cell c is BACKGROUND iff some cell c' with |c' - c| <= dilate on every axis has seen[c'] >= min_seen; c' stays
 *               inside 0..65535 per axis, nothing wraps at the ends of the int16 range. min_seen 1..65535, dilate 0 or 1, mode
 *               PCS_BACKGROUND_MODE_REMOVE (keep what is NOT background) or PCS_BACKGROUND_MODE_KEEP. With overflow set every record is
 *               kept, in both modes: a filter must never silently eat a scene because a table was sized too small.
 * The output of subtract is the kept records in input order, all 10 bytes of each unchanged, their count, and (optional) the statistics
 * block of eight int64: considered, kept, background (0 on an overflowed model), cells, frames, min_seen, overflow, reserved (0).
 * Exact and deterministic: the same bytes on every run, whatever order the atomics arrive in (tests/np_background.py restates it as
 * a Python dict and brute force). DESIGN.md section 3 has the definition and what follows from it.
 * pcs_background_create: a model on the context's device, empty (frames 0, no cell). cell_mm 1..1000, max_cells
 *   1..PCS_BACKGROUND_MAX_CELLS_MAX. The table is the model's own allocation, not a context slab: 2048 ceil(2 max_cells / 2048) slots of
 *   16 bytes, about 32 bytes per max_cells (PCS_ERR_NOMEM if the device has no room). One launch (clear). A model belongs to the
 *   context that created it: pcs_background_destroy it first, or leave it to that context's pcs_destroy, which frees what is left
 *   (the pointer is dead afterwards). Any context on the same device may learn into it or subtract with it; calls on one model from
 *   several contexts are ordered by the caller (streams). pcs_background_reset: the freshly created model again, one launch.
 * pcs_background_learn_device: asynchronous on the context's stream, no host round trip, one launch (none with n_points 0, which
 *   still counts as a frame). pcs_background_learn_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when
 *   the kernel runs, clamped to 0..max_points (max_points 0: nothing launched, a frame). pcs_background_learn: host pointers, staged
 *   through the context, synchronous.
 * pcs_background_subtract_device: asynchronous, no host round trip: flag (one probe sequence per record for background, up to 27 with
 *   dilate 1 for foreground), then the radius filter's ordered compaction (three launches) and, with d_stats, the block: 5 launches, 4
 *   without. d_out needs room for the worst case: out_shorts >= 5 n_points is checked up front; nothing outside the first 10 * kept
 *   bytes of d_out is written. *d_out_points (device, 4-byte aligned, required) receives kept; d_stats (device, 8-byte aligned,
 *   optional) the block. n_points 0 launches nothing and writes a zero count and a zeroed block.
 *   pcs_background_subtract_device_counted: the count from *d_n_points as above; max_points sizes the workspace, the grids and the
 *   output check. It takes any counted filter's output and count, and its own feed pcs_voxel_grid_device_counted and the other
 *   counted filters. pcs_background_subtract: host pointers, staged, synchronous; stats optional (with n_points 0 it reads nothing
 *   from the device: cells, frames and overflow of the block are 0 then).
 * pcs_background_info: synchronous (waits for the context's stream): what the model holds now.
 * pcs_background_export: synchronous; the canonical "PCB1" container: a 32-byte header {"PCB1", uint32 version 1,
 *   int32 cell_mm, uint32 frames, uint32 cells, 12 zero bytes}, then `cells` entries of 12 bytes {uint16 cx, cy, cz, uint16 0, uint32
 *   seen}, strictly ascending by key (cx | cy << 16 | cz << 32): the same model is the same bytes on every run and every machine.
 *   capacity < 32 + 12 cells is PCS_ERR_CAPACITY (pcs_background_export_bound(max_cells) always suffices); an overflowed model is
 *   PCS_ERR_CAPACITY too: what it holds is unspecified. One gather launch (none for a model without cells); the host sorts.
 * pcs_background_import: validates (below), then a new model with the container's cell_mm, frames and cells; cells > max_cells is
 *   PCS_ERR_CAPACITY. Two launches (clear, import; one for an empty container). Synchronous.
 * pcs_background_validate: host only, no context, no GPU: everything an importer relies on. PCS_ERR_INVALID_ARG with the first violation
 *   in pcs_last_error(NULL) for: bad magic or version, cell_mm outside 1..1000, frames above the cap, non-zero header padding, a length
 *   that is not 32 + 12 cells, non-zero entry padding, seen outside 1..frames, keys that do not ascend strictly. Fills *info (optional;
 *   max_cells = cells, overflow = 0).
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: a NULL
 *   model, a model on another device than the context's, a parameter out of range, reserved != 0, NULL params, a negative count, a
 *   NULL pointer (payload and output may be NULL with a count of 0), an odd payload or output address, a misaligned count or stats
 *   address, out_shorts below the worst case, any overlap among the input, output, count and stats ranges, a learn call at the
 *   frames cap.
 * Works on every context: flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH are not read. subtract's workspace is the radius
 *   filter's slab in the context. With pcs_kernel_timing enabled a call yields one interval per launch: create 1, reset 1, learn 1
 *   (0 with no record capacity), subtract 5 or 4 (0 with no capacity), export 1 (0 for a model without cells), import 2 (1 for a
 *   container without cells). Measured: DESIGN.md section 10 (f16), profiles/background_probe.txt.                                   */
#define PCS_BACKGROUND_CELL_MIN       1
#define PCS_BACKGROUND_CELL_MAX       1000
#define PCS_BACKGROUND_FRAMES_MAX     65535
#define PCS_BACKGROUND_MAX_CELLS_MAX  (1 << 26)
#define PCS_BACKGROUND_MODE_REMOVE    0
#define PCS_BACKGROUND_MODE_KEEP      1
typedef struct pcs_background pcs_background;               /* opaque; lives on the context's device */
typedef struct pcs_background_params {
    int32_t min_seen, dilate, mode, reserved;               /* reserved is 0 */
} pcs_background_params;
struct pcs_background_info {     /* (a tag only: pcs_background_info is also the call's name, as pcs_compressed_info) */
    int32_t  cell_mm, max_cells;
    uint32_t cells, frames;
    int32_t  overflow, reserved;
};
struct pcs_background_stats {
    int64_t considered, kept, background, cells, frames, min_seen, overflow, reserved;
};
int pcs_background_create(pcs_ctx* ctx, int cell_mm, int max_cells, pcs_background** out);
int pcs_background_destroy(pcs_ctx* ctx, pcs_background* bg);
int pcs_background_reset(pcs_ctx* ctx, pcs_background* bg);
int pcs_background_learn_device(pcs_ctx* ctx, pcs_background* bg, const int16_t* d_payload, int n_points);
int pcs_background_learn_device_counted(pcs_ctx* ctx, pcs_background* bg, const int16_t* d_payload, const int32_t* d_n_points,
                                        int max_points);
int pcs_background_learn(pcs_ctx* ctx, pcs_background* bg, const int16_t* payload, int n_points);   /* host pointer, staged, synchronous */
int pcs_background_subtract_device(pcs_ctx* ctx, pcs_background* bg, const int16_t* d_payload, int n_points,
                                   const pcs_background_params* params, int16_t* d_out, size_t out_shorts, int32_t* d_out_points,
                                   struct pcs_background_stats* d_stats);
int pcs_background_subtract_device_counted(pcs_ctx* ctx, pcs_background* bg, const int16_t* d_payload, const int32_t* d_n_points,
                                           int max_points, const pcs_background_params* params, int16_t* d_out, size_t out_shorts,
                                           int32_t* d_out_points, struct pcs_background_stats* d_stats);
int pcs_background_subtract(pcs_ctx* ctx, pcs_background* bg, const int16_t* payload, int n_points, const pcs_background_params* params,
                            int16_t* out, size_t out_shorts, int* out_points, struct pcs_background_stats* stats);   /* host pointers, staged, synchronous */
int pcs_background_info(pcs_ctx* ctx, pcs_background* bg, struct pcs_background_info* info);
size_t pcs_background_export_bound(int max_cells);
int pcs_background_export(pcs_ctx* ctx, pcs_background* bg, void* out, size_t capacity, size_t* out_bytes);
int pcs_background_import(pcs_ctx* ctx, const void* bytes, size_t n_bytes, int max_cells, pcs_background** out);
int pcs_background_validate(const void* bytes, size_t n_bytes, struct pcs_background_info* info);

/* ---- object tracks: persistent identities across frame-sets (not in the reference) ------------------------------------------------ *
 * An object's number k in pcs_cluster_objects_device* is "rank by first record": it changes whenever the record order does. A tracker
 * is a PERSISTENT device object that gives every object an identity that survives from one frame-set to the next. The evidence is
 * per record: which of the last frame-set's objects occupied the cell this record is in now. Everything is integer; no float anywhere.
 * The inputs of one UPDATE are what pcs_cluster_objects_device* leaves on the device: the payload it clustered (n records of 5 shorts;
 * shorts 0..2 are read, colour is not), object_of (n int32), *n_objects and the max_objects that call was given. m = *n_objects
 * clamped to 0..max_objects. A record TAKES PART iff 0 <= object_of(i) < m; every other value is ignored.
 *   CELL        floor(v / cell_mm) + 32768 per axis, cell_mm 1..1000: the background model's cell.
 *   STATE       after update t: m_t; per object j < m_t an id (int64, >= 1) and an age (int32); the map P_t: cell -> the SMALLEST j
 *                 among the taking-part records in that cell; next_id; frames. Fresh or reset: m = 0, an empty map, frames = 0,
 *                 next_id = first_id (pcs_tracker_create: 1; pcs_tracker_reset: 1..2^62).
 *   VOTES       votes(k, j) = the number of taking-part records i with object_of(i) = k and P_{t-1}(cell(i)) = j.
 *   CHOICE      choice(k) = the j with the most votes(k, j) > 0, on a tie the smallest j; with no vote there is none.
 *   KEEPER      keeper(j) = among the k with choice(k) = j the one with the most votes(k, j), on a tie the smallest k.
 *   CONTINUED   k continues j iff choice(k) = j, keeper(j) = k and votes(k, j) >= min_votes (1..2^30): id(k) = id_{t-1}(j),
 *                 age(k) = min(age_{t-1}(j) + 1, INT32_MAX), prev = j, votes = votes(k, j). A merge keeps the majority's identity;
 *                 a split leaves the identity with the larger part.
 *   BORN        every other k < m: id(k) = next_id + r, r its rank among the born by ascending k; age 0, prev -1, votes 0. Then
 *                 next_id += born.
 *   LOST        the number of j < m_{t-1} that no k continues.
 *   OVERFLOW    (a) an update needs more than max_cells distinct (k, j) pairs: this update continues nothing, all m are born
 *                 (statistics overflow bit 0). (b) an update's taking-part records occupy more than max_cells distinct cells: the
 *                 NEXT update continues nothing (bit 1, reported by the update that suffers it). Which surplus cells or pairs got in
 *                 is unspecified and cannot influence any output: the affected update reads neither. No hang, no write outside the
 *                 tables.
 * Output: tracks[k] for k < m (24 bytes each, reserved 0; nothing at or beyond entry m is written) and an optional block of eight
 * int64: considered (taking-part records), voted (those whose cell was in P_{t-1}; 0 where that map had overflowed), objects (m),
 * continued, born, lost, overflow, frames (after this update). Exact and deterministic: the same bytes on every run, whatever order
 * the atomics arrive in; under a permutation of the records that keeps object_of consistent the outputs are unchanged. An update with
 * m = 0 or with no record is still an update: frames + 1, the map emptied, every previous object lost. tests/np_tracks.py restates it.
 * pcs_tracker_create: a tracker on the context's device: cell_mm 1..1000, max_cells 1..2^26, max_objects 1..PCS_CLUSTER_OBJECTS_MAX.
 *   It owns its memory (not a context slab): three tables of 2048 ceil(2 max_cells / 2048) slots of 12 bytes (two cell maps used
 *   alternately as P_{t-1} and P_t, and the pair table), 40 bytes per object of max_objects, 32 KB of striped counters and a
 *   256-byte control block. It belongs to the context that
 *   created it: pcs_tracker_destroy it first, or leave it to that context's pcs_destroy, which frees what is left.
 *   pcs_tracker_reset: the fresh tracker again with next_id = first_id, one launch.
 * pcs_tracker_update_device: asynchronous on the context's stream, no host round trip. d_object_of and d_n_objects are 4-byte
 *   aligned, d_tracks (max_objects entries; NULL iff max_objects == 0) and d_stats (optional) 8-byte aligned; max_objects 0 .. the
 *   tracker's. pcs_tracker_update_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when the kernels run,
 *   clamped to 0..max_points; records at or beyond the count are never read. pcs_tracker_update: host pointers, staged, synchronous;
 *   n_objects by value.
 * pcs_tracker_info: synchronous (waits for the context's stream). overflow: the last update's overflow word, and bit 2 where the
 *   map that update built overflowed (the next update will continue nothing).
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: a NULL
 *   tracker, a tracker on another device than the context's, NULL params, min_votes out of range, a reserved word != 0, a negative
 *   count, a NULL pointer (payload and object_of may be NULL with a count of 0), an odd payload address, max_objects outside
 *   0 .. the tracker's, a misaligned object_of, n_objects, count, tracks or stats address, an output (tracks, stats) that shares a
 *   byte with an input or with the other output (inputs are only read: they may overlap each other), a tracker one of whose updates
 *   failed between its launches (PCS_ERR_HIP then; its tables are half built: pcs_tracker_reset it).
 * Launches, every update, all three forms, whatever the counts: 4 (record pass, choose, claim, assign); create 1, reset 1. Nothing is
 *   cleared by a launch of its own: the record pass zeroes what the folds behind it need, choose empties the pair table and the map
 *   it has read, assign the control block and the counters. With pcs_kernel_timing enabled a call yields one interval per launch.
 *   Measured: DESIGN.md section 10 (f17), profiles/track_probe.txt.                                                                  */
#define PCS_TRACKER_MAX_CELLS_MAX   (1 << 26)
#define PCS_TRACKER_MIN_VOTES_MAX   (1 << 30)
#define PCS_TRACKER_FIRST_ID_MAX    ((int64_t)1 << 62)
typedef struct pcs_tracker pcs_tracker;                     /* opaque; lives on the context's device */
typedef struct pcs_track {                                  /* 24 bytes, 8-byte aligned */
    int64_t id;
    int32_t age, prev, votes, reserved;                     /* reserved is 0 */
} pcs_track;
typedef struct pcs_track_params {
    int32_t min_votes, reserved[3];                         /* reserved words are 0 */
} pcs_track_params;
struct pcs_track_stats {
    int64_t considered, voted, objects, continued, born, lost, overflow, frames;
};
struct pcs_tracker_info {        /* (a tag only: pcs_tracker_info is also the call's name) */
    int32_t cell_mm, max_cells, max_objects, objects;
    int64_t frames, next_id;
    int32_t overflow, reserved;
};
int pcs_tracker_create(pcs_ctx* ctx, int cell_mm, int max_cells, int max_objects, pcs_tracker** out);
int pcs_tracker_destroy(pcs_ctx* ctx, pcs_tracker* tr);
int pcs_tracker_reset(pcs_ctx* ctx, pcs_tracker* tr, int64_t first_id);
int pcs_tracker_update_device(pcs_ctx* ctx, pcs_tracker* tr, const int16_t* d_payload, int n_points, const int32_t* d_object_of,
                              const int32_t* d_n_objects, int max_objects, const pcs_track_params* params, pcs_track* d_tracks,
                              struct pcs_track_stats* d_stats);
int pcs_tracker_update_device_counted(pcs_ctx* ctx, pcs_tracker* tr, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                      const int32_t* d_object_of, const int32_t* d_n_objects, int max_objects,
                                      const pcs_track_params* params, pcs_track* d_tracks, struct pcs_track_stats* d_stats);
int pcs_tracker_update(pcs_ctx* ctx, pcs_tracker* tr, const int16_t* payload, int n_points, const int32_t* object_of, int n_objects,
                       int max_objects, const pcs_track_params* params, pcs_track* tracks, struct pcs_track_stats* stats);   /* host pointers, staged, synchronous */
int pcs_tracker_info(pcs_ctx* ctx, pcs_tracker* tr, struct pcs_tracker_info* info);

/* ---- object boxes: second moments, axes and extents per object (not in the reference) --------------------------------------------- *
 * The object table says where an object is; a box says which way it lies. The inputs are what pcs_cluster_objects_device* leaves on
 * the device and what pcs_tracker_update_device* takes: the payload (n records of 5 shorts; shorts 0..2 are read, colour is not),
 * object_of (n int32), *n_objects and max_objects (0..PCS_CLUSTER_OBJECTS_MAX). m = *n_objects clamped to 0..max_objects. A record
 * TAKES PART iff 0 <= object_of(i) < m; every other value is ignored.
 * Output: boxes[k] for k < m, 128 bytes each, written whole; nothing at or beyond entry m is written.
 *   SUMS        count, sum_xyz, m2 (xx, xy, xz, yy, yz, zz) over the members, exact in int64 (every sum stays below 2^58).
 *   AXES        C = count M2 - S1 S1^T exactly in 128-bit integers, converted to double once; a cyclic Jacobi in a fixed order with
 *                 the normals' stop rule and twelve-sweep bound; eigenvalues descending, a tie to the lower column; the component of
 *                 largest magnitude of axis 0 and of axis 1 is positive (ties prefer z, then y, then x); axis 2 = axis 0 x axis 1;
 *                 axis[a][c] = rint(16384 v_a[c]). rank = the number of eigenvalues > 1e-12 lambda_max, 0 when lambda_max <= 0 (one
 *                 record, or all members equal: the axes are then the identity). No entry is "invalid": a line or a plane gets an
 *                 orthonormal triple like any other object and rank says how many of its axes mean something.
 *   EXTENTS     ext_lo[a] / ext_hi[a] = the minimum / maximum over the members of axis[a] . p in int32 (exact), units of mm / 16384:
 *                 a function of the WRITTEN shorts, projections from the origin. The box centre along axis a is
 *                 (ext_lo[a] + ext_hi[a]) / 2 / 16384.
 *   NO MEMBER   an entry k < m that no record names: count 0, zero sums, identity axes, rank 0, ext_lo = ext_hi = 0.
 * Deterministic: the same bytes on every run, whatever order the atomics arrive in; under a permutation of the records that keeps
 * object_of consistent every entry is byte-identical. tests/np_object_boxes.py restates it.
 * pcs_object_boxes_device: asynchronous on the context's stream, no host round trip. d_object_of and d_n_objects are 4-byte aligned,
 *   d_boxes (max_objects entries; NULL iff max_objects == 0) 8-byte aligned. pcs_object_boxes_device_counted: the count is read from
 *   *d_n_points (device, 4-byte aligned) when the kernels run, clamped to 0..max_points; records at or beyond the count are never
 *   read. pcs_object_boxes: host pointers, staged, synchronous; n_objects by value. A count of 0 is a normal call in every form: it
 *   writes the m empty entries.
 * Workspace: 128 bytes per object of max_objects in a slab of the context, grown on demand.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: a count
 *   outside 0 .. INT_MAX / 10, a NULL pointer (payload and object_of may be NULL with a count of 0, boxes with max_objects 0), an odd
 *   payload address, a misaligned object_of, n_objects, count or boxes address, max_objects outside 0..PCS_CLUSTER_OBJECTS_MAX, boxes
 *   sharing a byte with an input.
 * Launches, every call, all three forms, whatever the counts: PCS_OBJECT_BOXES_LAUNCHES (clear, moments, axes, extents). With
 *   pcs_kernel_timing enabled a call yields one interval per launch. Measured: DESIGN.md section 10 (f18).                           */
#define PCS_OBJECT_BOXES_LAUNCHES 4
typedef struct pcs_object_box {                             /* 128 bytes, 8-byte aligned */
    int64_t count;
    int64_t sum_xyz[3];
    int64_t m2[6];                                          /* xx, xy, xz, yy, yz, zz */
    int16_t axis[3][3];                                     /* axis[a] = rint(16384 unit vector a) */
    int16_t rank;                                           /* 0..3 */
    int32_t ext_lo[3], ext_hi[3];                           /* min / max of axis[a] . p, units of mm / 16384 */
    int32_t reserved;                                       /* 0 */
} pcs_object_box;
int pcs_object_boxes_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const int32_t* d_object_of, const int32_t* d_n_objects,
                            int max_objects, pcs_object_box* d_boxes);
int pcs_object_boxes_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                    const int32_t* d_object_of, const int32_t* d_n_objects, int max_objects, pcs_object_box* d_boxes);
int pcs_object_boxes(pcs_ctx* ctx, const int16_t* payload, int n_points, const int32_t* object_of, int n_objects, int max_objects,
                     pcs_object_box* boxes);               /* host pointers, staged, synchronous */

/* ---- plan-view maps: an orthographic raster of the cloud along a coordinate axis (not in the reference) ---------------------------- *
 * Every other output of the centre side is a table; this one is a picture: what is occupied and how high it is, seen along an axis.
 * DESIGN.md section 3 "Plan-view maps" has the definition; all of it is integer arithmetic on the records' shorts.
 * Input: n records of PCS_POINT_SHORTS shorts (x, y, z, R | G << 8, B) at any 2-byte phase; i = a record's position. The call knows
 *   nothing of invalid depth: a dense payload's zero-depth pixels sit on their camera's origin and pile into one cell (give
 *   PCS_FLAG_DROP_INVALID / -Z or a crop box first).
 * pcs_plan_params: up_axis a in 0..2 and up_sign s in {+1, -1}: the map axes are u = (a + 1) % 3 and v = (a + 2) % 3, a record's
 *   height is h = s p[a]. cell_mm c in 1..32767. origin_u, origin_v in -32768..32767: the low corner of cell (0, 0). width W and
 *   height H in 1..PCS_PLAN_SIDE_MAX with W H <= PCS_PLAN_CELLS_MAX. band_lo <= band_hi inside int16: a record TAKES PART iff
 *   band_lo <= p[a] <= band_hi (the raw coordinate, both ends inclusive). reserved words 0.
 * Mapping: cu = floor((p[u] - origin_u) / c), cv = floor((p[v] - origin_v) / c); the record is ON THE MAP iff 0 <= cu < W and
 *   0 <= cv < H; its cell is cv W + cu.
 * Output, W H cells each, nothing written outside them:
 *   count   uint32: the in-band, on-map records of the cell.
 *   top     int16: p[a] (raw) of the cell's top record, the member of greatest h, among equal h the one of LOWEST index.
 *   bottom  int16: p[a] of the member of least h, among equal h the one of lowest index.
 *   rgb     3 bytes R, G, B: the top record's colour bytes.
 *   An empty cell has count 0, top = bottom = 0 and rgb = 0, 0, 0: count is what says "empty".
 *   stats   considered (= n), in_band, mapped, occupied (cells with count > 0), fullest (the largest count), reserved 0.
 * Deterministic: counts and extremes over integers with an index tie-break; the bytes depend on the input bytes alone.
 *   tests/np_plan_view.py restates it.
 * pcs_plan_view_device: asynchronous on the context's stream, no host round trip; every pointer a device pointer, all five of
 *   pcs_plan_maps required: count 4-byte aligned, top and bottom 2-byte, stats 8-byte; the payload 2-byte aligned (NULL only with a
 *   count of 0). pcs_plan_view_device_counted: the count is read from *d_n_points (device, 4-byte aligned) when the kernels run,
 *   clamped to 0..max_points; records at or beyond it are never read. pcs_plan_view: host pointers, staged, synchronous. A count of
 *   0 is a normal call in every form: it writes the empty map.
 * Workspace: 16 bytes per cell in a slab of the context, grown on demand (the host form's rasters ride behind it).
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the function and the argument), nothing launched, nothing written: a
 *   parameter out of range or a reserved word that is not 0, a count outside 0 .. INT_MAX / 10, a NULL or misaligned pointer, an
 *   output sharing a byte with an input or with another output.
 * Launches, every call, all three forms, whatever the counts: PCS_PLAN_VIEW_LAUNCHES (clear, accumulate, resolve). With
 *   pcs_kernel_timing enabled a call yields one interval per launch. Measured: DESIGN.md section 10 (f19).                           */
#define PCS_PLAN_VIEW_LAUNCHES 3
#define PCS_PLAN_SIDE_MAX 4096
#define PCS_PLAN_CELLS_MAX (1 << 22)
typedef struct pcs_plan_params {                            /* 48 bytes */
    int32_t up_axis, up_sign;
    int32_t cell_mm;
    int32_t origin_u, origin_v;
    int32_t width, height;
    int32_t band_lo, band_hi;
    int32_t reserved[3];                                    /* 0 */
} pcs_plan_params;
struct pcs_plan_stats {                                     /* 64 bytes, 8-byte aligned */
    int64_t considered, in_band, mapped, occupied, fullest;
    int64_t reserved[3];                                    /* 0 */
};
typedef struct pcs_plan_maps {                              /* a host struct of pointers, all required */
    uint32_t* count;
    int16_t*  top;
    int16_t*  bottom;
    uint8_t*  rgb;
    struct pcs_plan_stats* stats;
} pcs_plan_maps;
int pcs_plan_view_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_plan_params* params, const pcs_plan_maps* maps);
int pcs_plan_view_device_counted(pcs_ctx* ctx, const int16_t* d_payload, const int32_t* d_n_points, int max_points,
                                 const pcs_plan_params* params, const pcs_plan_maps* maps);
int pcs_plan_view(pcs_ctx* ctx, const int16_t* payload, int n_points, const pcs_plan_params* params,
                  const pcs_plan_maps* host_maps);         /* host pointers, staged, synchronous */

/* ---- extrinsics refinement: nearest-neighbour alignment sums, the rigid fit, the ICP loop (not in the reference) ---------------- *
 * transform[i] comes from four surveyed markers (calibration.py); these calls refine it from the data: move one camera's payload
 * onto another's where they overlap. DESIGN.md section 3 "Alignment sums" has the definition and what follows from it.
 * SUMS. n_source and n_target records of 5 shorts (0..2 = x, y, z signed int16 mm; colour is not read), max_dist_mm 1..1000. The
 *   MATCH of source record p is the target record q that minimises (d^2, q.z, q.y, q.x), lexicographic, signed, d^2 =
 *   (px-qx)^2 + (py-qy)^2 + (pz-qz)^2 in integers of 32 bits or more, among the q with d^2 <= max_dist_mm^2; none: p is unmatched.
 *   The tie-break is by value: equal target records are interchangeable, the order of neither payload matters, many p may share
 *   one q. The result is pcs_align_sums, eighteen int64, exact (|p_a q_b| <= 2^30, fewer than 2^28 records: nothing reaches 2^63);
 *   optionally dist2[i] = the match's d^2 of source record i, 0xFFFFFFFF when unmatched. No floats in these kernels; the same bits on
 *   every run (tests/np_align.py restates it as brute force).
 * pcs_align_sums_device: asynchronous on the context's stream, no host round trip: the outlier filter's cell index over the target
 *   (6 launches), match, reduce. Payload pointers 2-byte aligned, d_sums 8-byte, d_dist2 (optional) 4-byte with room for n_source
 *   words. *d_sums is written whole (never needs zeroing). n_source == 0 or n_target == 0: a zeroed struct with considered =
 *   n_source, dist2 all 0xFFFFFFFF. With pcs_kernel_timing one interval per launch (8; 2 with an empty target, 1 with an empty source).
 * pcs_align_sums: host pointers, staged through the context, synchronous.
 * SOLVE. pcs_align_solve: host code, no context, errors in pcs_last_error(NULL). With n = matched, C[a][b] = n spq[3a+b] - sp[a] sq[b]
 *   exactly (128-bit integers), then double: C = U S V^T, R = V diag(1, 1, det(V U^T)) U^T — the proper rotation minimising
 *   sum |R p + t - q|^2 — and t = qbar - R pbar. delta: row-major 4x4 in METRES (t / 1000), last row 0 0 0 1; *rms_mm (optional) =
 *   sqrt(sd2 / n). PCS_ERR_UNSUPPORTED when matched < 3, or when C's second singular value is at most 1e-9 of its first (collinear or
 *   coincident points: the rotation is not unique).
 * LOOP. pcs_align_payloads_device: T_0 = init in double; for k = 0 ..: F_k = (float)T_k; the source moved by F_k with
 *   pcs_transform_payloads_device's arithmetic and stride source_stride (FLOOR(n / stride) records; records leaving int16 wrap, as
 *   there); S_k = sums(moved, target); delta_k = solve(S_k); T_k+1 = delta_k T_k. Stops after `iterations` steps
 *   (PCS_ALIGN_STOP_ITERATIONS); after the step whose delta has a rotation angle <= eps_rot_rad and a translation <= eps_trans_mm,
 *   unless both are 0 (PCS_ALIGN_STOP_CONVERGED; that delta is applied); when the solve refuses (PCS_ALIGN_STOP_REFUSED: the call
 *   returns the solve's status and out = the last good (float)T_k — init if the first solve refused). out = (float)T_K otherwise.
 *   Synchronous; the target's index is built once; per iteration three launches and one 144-byte copy to the host. The report
 *   (optional) carries the iterations run, matched / considered / rms of the first and the last of them, the stop reason, and
 *   — the caller fills trace_capacity, trace_transforms (16 floats each) and trace_sums before the call; NULL / 0: none — F_k and
 *   S_k of iterations 0 .. min(iterations run, trace_capacity) - 1, trace_count of them.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the argument), nothing launched, nothing written: a parameter out of range,
 *   a NULL or misaligned pointer (a payload may be NULL with a count of 0), a count outside 0..INT_MAX/10, any output overlapping an
 *   input or another output, a non-finite value in init.
 * These calls read no context predicate (flags, crop box, downsample, PCS_FLAG_SCALAR_ARITH). They know nothing of invalid depth: a
 *   dense payload's zero-depth pixels sit on the camera origin — align payloads made with PCS_FLAG_DROP_INVALID, or cropped. The
 *   workspace (the index, 40.2 bytes per target record; the moved source, 10 per source record; 144 per 256 source records) lives in
 *   the context and grows on demand. A source record costs the population of the cells around it that it cannot rule out;
 *   source_stride is the lever. Measured: DESIGN.md section 10 (f10).                                                              */
#define PCS_ALIGN_DIST_MIN         1
#define PCS_ALIGN_DIST_MAX         1000
#define PCS_ALIGN_ITERATIONS_MAX   100
#define PCS_ALIGN_STOP_ITERATIONS  0
#define PCS_ALIGN_STOP_CONVERGED   1
#define PCS_ALIGN_STOP_REFUSED     2
struct pcs_align_sums {     /* (a tag only: pcs_align_sums is also the host form's name, as pcs_compressed_info) */
    int64_t considered;     /* the source records looked at                    */
    int64_t matched;        /* the source records that found a match           */
    int64_t sp[3];          /* sum of p over the matched pairs                 */
    int64_t sq[3];          /* sum of q                                        */
    int64_t spq[9];         /* spq[3a+b] = sum of p_a q_b                      */
    int64_t sd2;            /* sum of d^2                                      */
};
typedef struct pcs_align_params {
    int32_t max_dist_mm;    /* 1..1000 */
    int32_t iterations;     /* 1..100  */
    int32_t source_stride;  /* >= 1    */
    int32_t reserved;       /* 0       */
    double  eps_rot_rad;    /* >= 0; with eps_trans_mm: both 0 = never stop early */
    double  eps_trans_mm;   /* >= 0    */
} pcs_align_params;
typedef struct pcs_align_report {
    int32_t iterations;                       /* out: sums computed                                     */
    int32_t stop_reason;                      /* out: PCS_ALIGN_STOP_*                                  */
    int64_t first_matched, first_considered;  /* out: of iteration 0                                    */
    int64_t last_matched, last_considered;    /* out: of the last iteration run                         */
    double  first_rms_mm, last_rms_mm;        /* out: sqrt(sd2 / matched), 0 with nothing matched       */
    int32_t trace_capacity;                   /* in                                                     */
    int32_t trace_count;                      /* out                                                    */
    float*  trace_transforms;                 /* in, optional: trace_capacity x 16 floats (host)        */
    struct pcs_align_sums* trace_sums;               /* in, optional: trace_capacity entries (host)            */
} pcs_align_report;
int pcs_align_sums_device(pcs_ctx* ctx, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                          int max_dist_mm, struct pcs_align_sums* d_sums, uint32_t* d_dist2);
int pcs_align_sums(pcs_ctx* ctx, const int16_t* source, int n_source, const int16_t* target, int n_target, int max_dist_mm,
                   struct pcs_align_sums* out, uint32_t* dist2);                  /* host pointers, staged, synchronous */
int pcs_align_solve(const struct pcs_align_sums* sums, double delta[16], double* rms_mm);
int pcs_align_payloads_device(pcs_ctx* ctx, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                              const pcs_align_params* params, const float init[16], float out[16], pcs_align_report* report);

/* ---- surface normals of a packed payload (not in the reference; modelled on PCL's NormalEstimation, parity unpinned) ------------- *
 * n_points records of 5 shorts (0..2 = x, y, z signed int16 mm; colour is not read). The NEIGHBOURHOOD of record q is every record x
 * of the payload with |x - q|^2 <= radius_mm^2 in integers of 32 bits or more — q itself and records equal to it included; m is its
 * size. With delta = x - q: S1 = sum delta, S2 = sum delta delta^T (int64, exact), C = m S2 - S1 S1^T formed exactly in 128-bit
 * integers and converted to double once; lambda0 <= lambda1 <= lambda2 and their unit eigenvectors from a cyclic Jacobi
 * eigen-decomposition in double on the device; v = the eigenvector of lambda0. DESIGN.md section 3 "Surface normals" has the
 * definition and what follows from it. A record is INVALID when m < min_neighbors, or lambda1 <= 1e-12 lambda2 (collinear or
 * coincident neighbours), or flatness > 0 and flatness lambda0 > lambda1 (the neighbourhood is not flat enough to call it a plane).
 * The sign of v: with use_viewpoint, v . (viewpoint_mm - q) >= 0 (at exactly 0 the rule below decides); without, the component of
 * largest magnitude is positive, ties preferring z, then y, then x.
 * Output: 4 shorts per record in record order — rint(16384 v_x), rint(16384 v_y), rint(16384 v_z), min(m, 32767) — or four zero
 * shorts for an invalid record (short 3 is never 0 for a valid one). A record's shorts are a function of its coordinates and the
 * payload as a multiset: equal records get equal shorts, the payload's order does not matter, every run gives the same bytes
 * (tests/np_normals.py restates the definition with numpy's eigh; the two agree to one unit of a short).
 * pcs_estimate_normals_device: asynchronous on the context's stream, no host round trip: the outlier filter's cell index over the
 *   payload with cell edge radius_mm (6 launches), estimate (one lane per record in cell order), gather (back to record order).
 *   d_payload 2-byte aligned; d_normals 8-byte aligned with room for 4 n_points shorts; *d_valid (optional, device, 4-byte aligned)
 *   receives the number of valid records. n_points 0 launches nothing and writes a zero count. With pcs_kernel_timing one
 *   interval per launch (8).
 * pcs_estimate_normals: host pointers, staged through the context, synchronous.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the argument), nothing launched, nothing written: a parameter out of range
 *   (radius_mm 1..1000, min_neighbors 3..32767, flatness 0..1000, use_viewpoint 0 or 1, reserved 0), a NULL, odd or misaligned
 *   pointer (payload and output may be NULL with a count of 0), a count outside 0..INT_MAX/10, any overlap of the ranges.
 * Works on every context: flags, crop box, downsample and PCS_FLAG_SCALAR_ARITH are not read. The calls know nothing of invalid
 *   depth (a dense payload's zero-depth pixels sit on the camera origin): use payloads made with PCS_FLAG_DROP_INVALID, or cropped.
 *   The workspace (the index, 40.2 bytes per record, and 8 more) lives in the context and grows on demand. A record costs the
 *   population of the cells around it that it cannot rule out; there is no early exit, n identical records cost n^2 tests.          */
#define PCS_NORMAL_RADIUS_MIN      1
#define PCS_NORMAL_RADIUS_MAX      1000
#define PCS_NORMAL_NEIGHBORS_MIN   3
#define PCS_NORMAL_NEIGHBORS_MAX   32767
#define PCS_NORMAL_FLATNESS_MAX    1000
#define PCS_NORMAL_SHORTS          4
#define PCS_NORMAL_BYTES           8
typedef struct pcs_normal_params {
    int32_t radius_mm;        /* 1..1000                                                     */
    int32_t min_neighbors;    /* 3..32767: the neighbourhood's least size, the record included */
    int32_t flatness;         /* 0 = off, else 1..1000: invalid when flatness lambda0 > lambda1 */
    int32_t use_viewpoint;    /* 0 or 1                                                      */
    int32_t viewpoint_mm[3];  /* the point valid normals are turned towards                  */
    int32_t reserved;         /* 0                                                           */
} pcs_normal_params;
int pcs_estimate_normals_device(pcs_ctx* ctx, const int16_t* d_payload, int n_points, const pcs_normal_params* params,
                                int16_t* d_normals, int32_t* d_valid);
int pcs_estimate_normals(pcs_ctx* ctx, const int16_t* payload, int n_points, const pcs_normal_params* params,
                         int16_t* normals, int* valid);                           /* host pointers, staged, synchronous */

/* ---- extrinsics refinement, point to plane: plane sums, the 6 x 6 solve, the loop (not in the reference) ------------------------ *
 * Point-to-point alignment of two independent samples of a surface ends at the sampling pitch; against the target's surface normals
 * it ends far below it. DESIGN.md section 3 "Plane sums" has the definitions and what follows from them.
 * SUMS. Source and target payloads and max_dist_mm as for pcs_align_sums_device, plus target_normals: 4 shorts per target record,
 *   8-byte aligned, what pcs_estimate_normals_device writes — or any int16 values, the call does not check them; a target record
 *   has a valid normal iff its short 3 != 0. The MATCH of source record p is pcs_align_sums_device's, exactly. The NORMAL of a match
 *   is the smallest valid four-short word, compared as one unsigned 64-bit little-endian number, among the target records whose
 *   coordinates equal the match's; none: the pair is matched but not USED. By value: neither payload's order reaches the result.
 *   Per used pair, in integers: n = the word's first three shorts, c = p x n, a = (c_x, c_y, c_z, n_x, n_y, n_z), b = n . (q - p).
 *   Every a_i a_j, a_i b and b^2 fits int64 (|c| < 2^31) but their sums over a payload do not: each product t is summed as two
 *   halves, lo = t & 0xFFFFFFFF (unsigned) and hi = t >> 32 (arithmetic), each below 2^60 for fewer than 2^28 records; the value is
 *   hi 2^32 + lo in 128 bits. The result is pcs_align_plane_sums, sixty int64, exact, the same bits on every run
 *   (tests/np_align_plane.py restates it); dist2 as pcs_align_sums_device's, over the matched pairs whether used or not.
 * pcs_align_plane_sums_device: asynchronous on the context's stream, no host round trip: the index over the target (6 launches), the
 *   normals scattered into cell order, match, reduce. *d_sums (8-byte aligned) is written whole. n_source == 0 or n_target == 0: a
 *   zeroed struct with considered = n_source. With pcs_kernel_timing one interval per launch (9; 2 with an empty target, 1 with an
 *   empty source). pcs_align_plane_sums: host pointers, staged through the context, synchronous.
 * SOLVE. pcs_align_plane_solve: host code, no context, errors in pcs_last_error(NULL). The sums recombined in 128-bit integers, then
 *   double; A^T A scaled symmetrically to a unit diagonal; a Jacobi eigen-decomposition of the scaled 6 x 6; x = (omega, t) solves
 *   A^T A x = A^T b. delta: rotation exp([omega]x) (Rodrigues, a series below 1e-4 rad), translation t / 1000 METRES, row-major 4x4,
 *   last row 0 0 0 1; *rms_mm (optional) = sqrt(sb2 / used) / 16384, the distance to the planes. PCS_ERR_UNSUPPORTED when used < 6,
 *   when a diagonal entry is zero, or when the scaled matrix's smallest eigenvalue is at most 1e-9 of its largest: the pose is not
 *   determined — a target that is one plane, or parallel planes, is the case users meet.
 * LOOP. pcs_align_payloads_plane_device: pcs_align_payloads_device's loop with the plane sums and the plane solve. The target's
 *   normals are estimated once per call (params->normals; their sign does not matter), the index is built and the normals scattered
 *   once; per iteration three launches (transform, match, reduce) and one 480-byte copy to the host. The stop rules, the refusals
 *   and out = the last good (float)T_k are pcs_align_payloads_device's; the report carries `used` beside `matched`, and its rms is
 *   still sqrt(sd2 / matched). With pcs_kernel_timing: 15 intervals once, 3 per iteration.
 * Refused with PCS_ERR_INVALID_ARG (pcs_last_error names the argument), nothing launched, nothing written: as the point-to-point
 *   calls, and a NULL or misaligned d_target_normals (it may be NULL with n_target 0), a normal parameter out of range.            */
struct pcs_align_plane_sums {   /* (a tag only, as pcs_align_sums) */
    int64_t considered;         /* the source records looked at                                  */
    int64_t matched;            /* ... that found a match                                        */
    int64_t used;               /* ... whose match has a valid normal                            */
    int64_t ata_lo[21];         /* sum of (a_i a_j) & 0xFFFFFFFF, upper triangle row-major        */
    int64_t ata_hi[21];         /* sum of (a_i a_j) >> 32                                        */
    int64_t atb_lo[6];          /* sum of (a_i b) & 0xFFFFFFFF                                   */
    int64_t atb_hi[6];          /* sum of (a_i b) >> 32                                          */
    int64_t sb2_lo, sb2_hi;     /* sum of b^2, likewise                                          */
    int64_t sd2;                /* sum of d^2 over the matched pairs                             */
};
typedef struct pcs_align_plane_params {
    int32_t max_dist_mm;        /* 1..1000 */
    int32_t iterations;         /* 1..100  */
    int32_t source_stride;      /* >= 1    */
    int32_t reserved;           /* 0       */
    double  eps_rot_rad;        /* >= 0; with eps_trans_mm: both 0 = never stop early */
    double  eps_trans_mm;       /* >= 0    */
    pcs_normal_params normals;  /* how the target's normals are estimated             */
} pcs_align_plane_params;
typedef struct pcs_align_plane_report {
    int32_t iterations;                                   /* out: sums computed                               */
    int32_t stop_reason;                                  /* out: PCS_ALIGN_STOP_*                            */
    int64_t first_matched, first_used, first_considered;  /* out: of iteration 0                              */
    int64_t last_matched, last_used, last_considered;     /* out: of the last iteration run                   */
    double  first_rms_mm, last_rms_mm;                    /* out: sqrt(sd2 / matched), 0 with nothing matched */
    int32_t trace_capacity;                               /* in                                               */
    int32_t trace_count;                                  /* out                                              */
    float*  trace_transforms;                             /* in, optional: trace_capacity x 16 floats (host)  */
    struct pcs_align_plane_sums* trace_sums;              /* in, optional: trace_capacity entries (host)      */
} pcs_align_plane_report;
#define PCS_ALIGN_PLANE_USED_MIN   6
int pcs_align_plane_sums_device(pcs_ctx* ctx, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                                const int16_t* d_target_normals, int max_dist_mm, struct pcs_align_plane_sums* d_sums,
                                uint32_t* d_dist2);
int pcs_align_plane_sums(pcs_ctx* ctx, const int16_t* source, int n_source, const int16_t* target, int n_target,
                         const int16_t* target_normals, int max_dist_mm, struct pcs_align_plane_sums* out,
                         uint32_t* dist2);                                        /* host pointers, staged, synchronous */
int pcs_align_plane_solve(const struct pcs_align_plane_sums* sums, double delta[16], double* rms_mm);
int pcs_align_payloads_plane_device(pcs_ctx* ctx, const int16_t* d_source, int n_source, const int16_t* d_target, int n_target,
                                    const pcs_align_plane_params* params, const float init[16], float out[16],
                                    pcs_align_plane_report* report);

/* ---- stream / timing plumbing ----------------------------------------------------------- */
int   pcs_set_stream(pcs_ctx* ctx, void* hip_stream);   /* adopt a caller-owned hipStream_t (NULL = own stream) */
void* pcs_get_stream(pcs_ctx* ctx);
/* Two contexts of one device used IN TURN overlap — the tail of one call beside the head of the next (BASELINE configs[4]: the voxel
 * pipeline's bucket tail beside the next frame-set's pre-aggregation, 0.169 -> 0.152 ms per 16 x 1080p frame-set) — only if their streams
 * sit on different hardware queues; the runtime deals streams onto a few queues round robin, so that is luck. pcs_use_stream_beside
 * replaces ctx's OWN stream by one that is SEEN to run beside other's current stream (a no-op must finish while a 300 us spin occupies
 * the other; up to six candidates; ~2 ms, once). Returns 1 when such a stream was found and taken, 0 when none was (ctx keeps its
 * stream), a negative status on error. pcs_pick_concurrent_stream is the same probe on raw hipStream_t handles of the CURRENT device
 * (*out_stream = NULL when none overlapped; the caller owns the stream it gets). libpcs_node uses both.                              */
int   pcs_use_stream_beside(pcs_ctx* ctx, pcs_ctx* other);
int   pcs_pick_concurrent_stream(void* busy_hip_stream, void** out_stream);
int   pcs_synchronize(pcs_ctx* ctx);
/* hipEvent bracket on the context stream: begin; enqueue work; end; elapsed = GPU ms between them. */
int   pcs_timer_begin(pcs_ctx* ctx);
int   pcs_timer_end(pcs_ctx* ctx);
int   pcs_timer_elapsed_ms(pcs_ctx* ctx, float* ms);    /* synchronises on the end event */
/* Per-launch kernel timing: when enabled every fused-kernel launch is bracketed by its own
 * event pair; pcs_kernel_times_ms drains them (synchronising) into ms[0..*n).                 */
int   pcs_kernel_timing(pcs_ctx* ctx, int enable);
int   pcs_kernel_times_ms(pcs_ctx* ctx, float* ms, int capacity, int* n);

/* Page-locked host memory for the buffers that cross PCIe every frame (the reference mallocs its `buffer`
 * once, src/pcs-camera-optimized.cpp:157). When every buffer of a host call is page-locked the call runs zero copy
 * (pcs_process_frames: 1.6 instead of 2.25 ms per 8x720p frame-set; pcs_copy_pointcloud_xyzrgb_to_buffer likewise);
 * with pageable memory the calls stage through device buffers. What is really expensive is handing over a freshly
 * allocated buffer every call (first-touch page faults, 7.5 ms). */
int   pcs_host_malloc(pcs_ctx* ctx, void** h_ptr, size_t bytes);
int   pcs_host_free(pcs_ctx* ctx, void* h_ptr);
/* Page-lock memory the caller already owns (the reference's `buffer = (short*)malloc(sizeof(short) * BUF_SIZE)`,
 * src/pcs-camera-optimized.cpp:157; a capture pipeline's frame pool) so that the host entry points run zero copy on it.
 * Register once, unregister before free(). */
int   pcs_host_register(pcs_ctx* ctx, void* h_ptr, size_t bytes);
int   pcs_host_unregister(pcs_ctx* ctx, void* h_ptr);

/* Thin device-memory helpers so a C/C++ host needs no HIP headers. */
int   pcs_device_malloc(pcs_ctx* ctx, void** d_ptr, size_t bytes);
int   pcs_device_free(pcs_ctx* ctx, void* d_ptr);
int   pcs_memcpy_h2d(pcs_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int   pcs_memcpy_d2h(pcs_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* PCS_HIP_H */
