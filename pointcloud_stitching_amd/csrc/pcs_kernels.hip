// pcs_kernels.hip — hand-written gfx950 (CDNA4) kernels for the deproject -> rigid transform ->
// RGB attach -> XYZRGB int16 pack hot path of conix-center/pointcloud_stitching.
//
// What is replaced (reference file:line, read for behaviour only):
//   a5 rs2::pointcloud::calculate/map_to   call sites src/pcs-camera-optimized.cpp:198-199, 288-289
//   a2 copyPointCloudXYZRGBToBufferSIMD    src/pcs-camera-optimized.cpp:363-616
//   a7 sendStitchToUnity's concatenate     src/pcs-multicamera-client.cpp:385-392
//
// Shape of the work: per point ~15 algorithmic bytes (2 B Z16 in, 3 B RGB in, 10 B out) against a few
// dozen FP32 ops -> HBM-bound, no MFMA. What matters on CDNA4:
//   * every global access is a lane-contiguous 16 B vector access: the Z16 raster is read as uint4
//     (8 pixels / lane, 1 KiB / wavefront-instruction); the 10-byte records, which no lane can store
//     on its own at a 16 B boundary, are transposed through LDS so a wavefront writes 5 x 1 KiB;
//   * per-camera constants (3x4 extrinsic, 3x3+t depth->colour, intrinsics) are wave-uniform and sit
//     in SGPRs via scalar loads; the per-column / per-row deprojection LUTs are L2-resident;
//   * the colour gather is one (possibly unaligned) dword per point through L1/L2;
//   * invalid-depth / cutoff compaction is order-preserving: per-lane popcount -> wavefront scan ->
//     4-entry LDS cross-wave scan -> tile prefix from a count pass (deterministic, = `-c -m -t1` order).
//
// Two translation units, two files (Makefile): this one is pcs_kernels.o (everything but the voxel readers, SLP vectorisation
// off — packed FP32 measured 1-2 % slower on the HBM-bound kernels); pcs_kernels_voxel.hip is pcs_kernels_voxel.o (the raster /
// payload voxel readers, SLP on; the reasons are at its top). What both share, bit-exactness rules included: pcs_kernels_common.h.

#include <algorithm>
#include <type_traits>

#include "pcs_kernels_common.h"

#ifndef EMIT_WAVES
#define EMIT_WAVES 6      // 7 fits 72 VGPRs only with scratch spills in some instantiations and measured no faster
#endif

#ifndef PCS_SCALAR_FP64
#define PCS_SCALAR_FP64 0     // 1: a3's conversion in FP64 for every point (A/B at build time; DESIGN.md section 8 has the measurement)
#endif
#ifndef SCALAR_DENSE_WAVES
#define SCALAR_DENSE_WAVES 7  // the residual form holds the dense kernel's 72 VGPRs without scratch; the FP64 form wants 95 (5)
#endif
#ifndef SCALAR_EMIT_CUT_WAVES
#define SCALAR_EMIT_CUT_WAVES 5   // the general form with a3's -c select: 87-90 VGPRs; at EMIT_WAVES (80) it spills 28-32 bytes
#endif

namespace pcs {

namespace {

constexpr uint32_t kDenseStageBytes = kTilePoints * PCS_POINT_BYTES;        // 20 480 B -> 8 workgroups / CU
constexpr uint32_t kStageBytes      = kTilePoints * PCS_POINT_BYTES + 32;   // + head skew + tail pad

// Park one record at a 2-byte aligned LDS byte offset using ALIGNED accesses only. (gfx950 does take an
// unaligned ds_write_b64, but it stalls the LDS pipe: SQ_LDS_UNALIGNED_STALL 5.2 M per launch and 3.5 us on
// the 8x720p emit.) The 10 bytes are cut by the parity of the offset's dword phase:
//   offset % 4 == 0 :  [x y]@+0 (b32)  [z c0]@+4 (b32)  [c1]@+8 (b16)
//   offset % 4 == 2 :  [x]@+0 (b16)    [y z]@+2 (b32)   [c0 c1]@+6 (b32)
// expressed as one b16 and two b32 writes whose addresses and values are selected, not branched.
__device__ __forceinline__ void stage_record(uint8_t* lds, uint32_t off, const Record& r)
{
    const bool odd = (off & 2u) != 0u;
    const uint32_t yz = perm(r.zc, r.xy, kHiLo);
    const uint32_t cc = perm(r.b, r.zc, kHiLo);
    const uint32_t h_val = odd ? r.xy : r.b;                 // low 16 bits are what is written
    const uint32_t a_val = odd ? yz : r.xy;
    const uint32_t b_val = odd ? cc : r.zc;
    const uint32_t h_off = odd ? off : off + 8u;
    const uint32_t a_off = odd ? off + 2u : off;
    *reinterpret_cast<uint16_t*>(lds + h_off) = (uint16_t)h_val;
    *reinterpret_cast<uint32_t*>(lds + a_off) = a_val;
    *reinterpret_cast<uint32_t*>(lds + a_off + 4u) = b_val;
}

// One point -> one record. short(float) (:581-583) keeps the low 16 bits of the converted value.
// Arith: which of the reference's loops the world coordinates follow (pcs_kernels_common.h). Under ScalarArith the Cvt policy converts
// the colour coordinates only; the world values take the FP32 residual form under a policy that keeps a running maximum (whose redo
// is the exact policy) and the FP64 form under any other. With its CUT a point the loop skips gives the all-zero record.
template <class Arith = SimdArith, class Cvt>
__device__ __forceinline__ Record make_record(const StreamParams& P, const uint8_t* __restrict__ color,
                                              const PointIn& p, Cvt& cv)
{
    float xf, yf;
    uint32_t x, y, z;
    if constexpr (Arith::kScalar) {
        const float ax = world_scalar(P.M + 0, p.X, p.Y, p.Z);
        const float ay = world_scalar(P.M + 4, p.X, p.Y, p.Z);
        const float az = world_scalar(P.M + 8, p.X, p.Y, p.Z);
        color_coords(P, p.u, p.v, xf, yf);
        if constexpr (Cvt::kTracks && !PCS_SCALAR_FP64) {
            constexpr float k = 131072.0f;       // 2^17: the policy's 2^31 is |a| = 2^14, the residual form's reach
            cv.note(__fmul_rn(__builtin_fabsf(ax), k), __fmul_rn(__builtin_fabsf(ay), k), __fmul_rn(__builtin_fabsf(az), k), xf, yf);
            x = mm_scalar_residual(ax); y = mm_scalar_residual(ay); z = mm_scalar_residual(az);
        } else {
            cv.note(0.0f, 0.0f, 0.0f, xf, yf);
            x = mm_scalar_exact(ax); y = mm_scalar_exact(ay); z = mm_scalar_exact(az);
        }
    } else {
        const float ax = world_mm(P.M + 0, p.X, p.Y, p.Z);
        const float ay = world_mm(P.M + 4, p.X, p.Y, p.Z);
        const float az = world_mm(P.M + 8, p.X, p.Y, p.Z);
        color_coords(P, p.u, p.v, xf, yf);
        cv.note(ax, ay, az, xf, yf);
        x = (uint32_t)cv.cvt(ax); y = (uint32_t)cv.cvt(ay); z = (uint32_t)cv.cvt(az);
    }
    const uint32_t w = color_fetch(P, color, cv.pixel(xf, P.cW - 1, P.c_wm1_f), cv.pixel(yf, P.cH - 1, P.c_hm1_f), cv);
    Record r;
    r.xy = perm(y, x, kLoLo);                    // short(x) | short(y) << 16  — the low 16 bits of each (:581-583)
    r.zc = perm(w, z, kLoLo);                    // short(z) | (R | G<<8) << 16
    r.b  = __builtin_amdgcn_ubfe(w, 16, 8);      // B, high byte 0 (:585)
    if constexpr (Arith::kCut) {
        const bool keep = scalar_cut_keeps(p.X, p.Z);
        r.xy = keep ? r.xy : 0u; r.zc = keep ? r.zc : 0u; r.b = keep ? r.b : 0u;
    }
    return r;
}

// rs2::points arrays (vertices + texcoords) -> points (the a2 twin's input), read straight into registers: a lane's 8 points
// are 96 contiguous bytes of vertices and 64 of texcoords (six + four 16-byte loads, all in flight together). A wavefront's
// k-th load touches 64 separate 16-byte pieces, but its six vertex loads cover the same 48 cache lines back to back, so the
// L1 does the merging. (Rounds 1-2 transposed the arrays through 40 KB of LDS with lane-contiguous loads — textbook
// coalescing, but the LDS round trip, its barrier and the fat workgroups cost far more than the L1 does: one 1280x720 cloud
// per launch 11.0 -> 7.1 us = 34 -> 53 % of HBM peak, eight clouds in one launch 61 -> 71 %.)
struct VertexSource {
    using Math = IeeeMath;
    const float* __restrict__ vertices;
    const float* __restrict__ texcoords;

    __device__ __forceinline__ void load8(const StreamParams&, uint32_t i0, uint32_t n, PointIn (&p)[8]) const
    {
        if (i0 + 8u <= n && ((((uintptr_t)vertices) | ((uintptr_t)texcoords)) & 15u) == 0u) {
            const float4* gv = reinterpret_cast<const float4*>(vertices + (size_t)i0 * 3);
            const float4* gt = reinterpret_cast<const float4*>(texcoords + (size_t)i0 * 2);
            float4 v[6], t[4];
#pragma unroll
            for (int k = 0; k < 6; k++) v[k] = gv[k];
#pragma unroll
            for (int k = 0; k < 4; k++) t[k] = gt[k];
            const float* fv = reinterpret_cast<const float*>(v);
            const float* ft = reinterpret_cast<const float*>(t);
#pragma unroll
            for (int k = 0; k < 8; k++) p[k] = PointIn{fv[3 * k], fv[3 * k + 1], fv[3 * k + 2], ft[2 * k], ft[2 * k + 1]};
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const size_t i = (size_t)i0 + k;
                if (i < n) p[k] = PointIn{vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2], texcoords[2 * i], texcoords[2 * i + 1]};
                else p[k] = PointIn{0, 0, 0, 0, 0};
            }
        }
    }
};

// ------------------------------------------------------------------------------------------------
// Staged store: LDS bytes [head, head+nbytes) -> global bytes [g, g+nbytes), where (g - head) is
// 16-byte aligned. Interior goes out as lane-contiguous 16-byte stores; the ragged ends (which may
// share a 16-byte line with a neighbouring tile's bytes) go out as 2-byte stores.
// ------------------------------------------------------------------------------------------------
template <uint32_t THREADS = kBlockThreads>
__device__ __forceinline__ void store_staged(const uint8_t* lds, uint32_t head, uint32_t nbytes, uint8_t* g)
{
    uint8_t* g0 = g - head;                                  // 16-byte aligned
    const uint32_t end = head + nbytes;
    const uint32_t first_full = (head + 15u) >> 4;           // first chunk entirely inside
    const uint32_t last_full = end >> 4;                     // one past the last chunk entirely inside
    // nontemporal: the payload is written once and never re-read by this kernel; keeping it out of the
    // caches' way measured +7 % on the store-dominated stream (tools/lab/kernel_lab.hip, skeleton nt-store)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (uint32_t j = first_full + threadIdx.x; j < last_full; j += THREADS)
        __builtin_nontemporal_store(reinterpret_cast<const u32x4*>(lds)[j], reinterpret_cast<u32x4*>(g0) + j);
    // ragged head: shorts in [head, min(first_full*16, end)); ragged tail: [max(last_full*16, head), end)
    const uint32_t head_end = min(first_full << 4, end);
    for (uint32_t b = head + 2u * threadIdx.x; b < head_end; b += 2u * THREADS)
        *reinterpret_cast<uint16_t*>(g0 + b) = *reinterpret_cast<const uint16_t*>(lds + b);
    if (last_full >= first_full) {
        const uint32_t tail_begin = max(last_full << 4, head_end);
        for (uint32_t b = tail_begin + 2u * threadIdx.x; b < end; b += 2u * THREADS)
            *reinterpret_cast<uint16_t*>(g0 + b) = *reinterpret_cast<const uint16_t*>(lds + b);
    }
}

// ------------------------------------------------------------------------------------------------
// DENSE tile kernel: no predicate, downsample 1, 16-byte aligned payload, every stream's point count
// a multiple of 8 (so every lane's 80-byte output run starts on a 16-byte boundary).
// Lane l of the workgroup produces 8 records = 5 x uint4 and parks them at LDS[l*80]; the workgroup
// then streams the tile's 20 480 bytes out with lane-contiguous 16-byte stores.
// ------------------------------------------------------------------------------------------------
// THREADS: lanes per workgroup = 8-point runs per tile (kBlockThreads: 2048-point tiles; 64: one wavefront per 512-point tile, what
// a launch that cannot fill the chip with 256-lane workgroups takes — launch_fused_dense).
template <class Src, uint32_t THREADS = kBlockThreads, class Arith = SimdArith>
__device__ __forceinline__ void dense_tile(const StreamParams& P, const Src& src, const uint8_t* __restrict__ color,
                                           uint32_t tile0, uint32_t n, uint8_t* __restrict__ out_bytes,
                                           uint4* stage)
{
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    PointIn p[8];
    src.load8(P, i0, n, p);

    uint32_t w[20];
    auto fill = [&](auto& cv) {
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            const Record a = make_record<Arith>(P, color, p[k], cv);
            const Record b = make_record<Arith>(P, color, p[k + 1], cv);
            uint32_t* o = w + (k >> 1) * 5;
            o[0] = a.xy;
            o[1] = a.zc;
            o[2] = perm(b.xy, a.b, kLoLo);
            o[3] = perm(b.zc, b.xy, kHiLo);
            o[4] = perm(b.b, b.zc, kHiLo);
        }
    };
    if (Src::Math::kCvtMode == 2) {
        FastCvt<false> fast;
        fill(fast);
        if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    } else if (Src::Math::kCvtMode == 1) {
        FastCvt<true> fast;
        fill(fast);
        if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    } else {
        ExactCvt exact;
        fill(exact);
    }
    uint4* mine = stage + threadIdx.x * 5;
#pragma unroll
    for (int k = 0; k < 5; k++) mine[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    __syncthreads();

    const uint32_t pts = min(THREADS * kPointsPerLane, n - tile0);
    store_staged<THREADS>(reinterpret_cast<const uint8_t*>(stage), 0u, pts * PCS_POINT_BYTES,
                          out_bytes + (size_t)tile0 * PCS_POINT_BYTES);
}

// ------------------------------------------------------------------------------------------------
// DENSE tile for launches whose streams are all row-constant (CertRowConstNoOvf, StreamParams::ident_r == 2): the colour
// bytes are requested beside the depth instead of behind it.
//
// A pixel's colour ROW is its raster row's entry of the certified table; only its COLUMN depends on the depth, and for depths
// beyond the stream's d_win it lies within a margin of the depth column's image (pcs_capi.cpp: color_window_params). A wave's
// 512 pixels lie on at most two raster rows, so the wave knows — from its first and last pixel and two scalar loads of the
// table — the one or two stretches of colour bytes its pixels will read before any depth value has arrived. It requests them
// by LDS-DMA into the front of its own 5 120 bytes of `stage` (where its records are parked later), right after the Z16 and
// LUT loads: the two round trips run together, and deprojection waits for the depth with the window still in flight.
// A pixel then reads its dword from LDS when the dword lies inside the window, or pixel (0, 0)'s word — what every invalid
// pixel carries, parked by the wave at the end of its part of `stage` — when its byte index is 0; any other pixel (a depth
// nearer than d_win, a row the window does not cover, the raster's last pixel) takes the global gather with the exact
// slide-back, exec-masked to its lanes. The window is a cache keyed by byte address: a wrong guess costs time, never bits.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kWaveStageBytes = 64u * kPointsPerLane * PCS_POINT_BYTES;        // 5 120: one wave's records
constexpr uint32_t kWinPieces      = 3;                                             // 16-byte LDS-DMA requests per lane
constexpr uint32_t kWinBytes       = kWinPieces * 64u * 16u;                        // 3 072: the wave's windows together
constexpr uint32_t kWinZeroWord    = kWaveStageBytes - 16u;                         // pixel (0, 0)'s word, past the windows
static_assert(kWinBytes + 8u <= kWinZeroWord, "the windows, the dword read past their end and the zero word fit one wave's stage");

template <class T> using cptr = const __attribute__((address_space(4))) T*;         // read-only for the kernel's life: scalar loads

// One colour stretch of a wave: the bytes of colour row `crow` that depth columns [c0, c1] can reach at depths beyond d_win,
// 16-aligned, inside the raster's whole 16-byte pieces, at most `room` bytes. Wave-uniform (scalar) arithmetic.
__device__ __forceinline__ void color_stretch(const StreamParams& P, const int32_t (&wp)[3], int32_t crow, int32_t c0, int32_t c1,
                                              uint32_t room, uint32_t& ws, uint32_t& len)
{
    const int32_t lo = min(max((c0 * wp[0] + wp[1]) >> 12, 0), P.cW - 1);
    const int32_t hi = min(max((c1 * wp[0] + wp[2]) >> 12, 0), P.cW - 1);
    const uint32_t row = (uint32_t)crow * (uint32_t)P.stride;
    ws = (row + (uint32_t)lo * (uint32_t)P.bpp) & ~15u;
    const uint32_t we = min((row + (uint32_t)hi * (uint32_t)P.bpp + 4u + 15u) & ~15u, P.color_bytes & ~15u);
    len = min(we > ws ? we - ws : 0u, room);
}

// The row-constant tile's vector loads, written as asm. hipcc does not wait for an LDS-DMA request by count: with one in flight it
// waits vmcnt(0) at the first use of any load, which would hold deprojection until the colour window has landed. So the tile issues
// its own five loads (Z16 quad, two LUT quads, my, colour row) and its three window requests here, outside the compiler's
// bookkeeping, and waits for them itself: vmcnt(kWinPieces) before deprojection (everything but the window, naming the five
// destinations so that nothing reads them earlier) and vmcnt(0) before the first read of the window.
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
// ONCE: bytes this lane alone reads, once per launch (its Z16 quad) are asked for nontemporal — they do not push the LUT and the colour
// rows, which neighbouring waves read again, out of the caches' way.
template <bool ONCE = false>
__device__ __forceinline__ u32x4v load16_asm(const void* base, uint32_t off)
{
    u32x4v v;
    if constexpr (ONCE) asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(v) : "v"(off), "s"(base));
    else                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(v) : "v"(off), "s"(base));
    return v;
}
__device__ __forceinline__ uint32_t load4_asm(const void* base, uint32_t off)
{
    uint32_t v;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(off), "s"(base));
    return v;
}
// One LDS-DMA request: this lane's 16 bytes at color + off -> LDS byte lds + 16 * lane (M0 set and restored in the statement).
__device__ __forceinline__ void window_piece(const uint8_t* color, uint32_t off, uint32_t lds)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(off), "s"(color), "s"(lds) : "memory");
}

// deproject_pixel_rowc (pcs_kernels_common.h; the other kernels keep it) in this tile's own form: X, Y, Z and the texture column u of
// EVERY pixel, a hole's included, and no row. The tile reads u for the colour column alone and selects a hole's byte index to 0
// afterwards: one select per pixel instead of one on u and one on the row. A hole's u is whatever 0 / 0 gives (NaN); FastCvt<false>
// clamps and converts it (v_med3_f32, v_cvt_i32_f32: no trap, no flag read anywhere) and keeps no state — it has no redo() in this
// tile — so nothing but the discarded index depends on it.
template <class Mth>
__device__ __forceinline__ PointIn deproject_pixel_win(const StreamParams& P, uint32_t d, float mx, float my)
{
    const float z = __fmul_rn(P.depth_scale, (float)d);
    PointIn p;
    p.X = __fmul_rn(z, mx);
    p.Y = __fmul_rn(z, my);
    p.Z = z;
    const float P0 = __fadd_rn(p.X, P.t[0]);
    const float P2 = p.Z;                                // z + t_z: a row-constant stream has t_z = +-0 (pcs_capi.cpp), so this is z for every z != 0
    float x, y_unused;
    Mth::div2(P0, P0, P2, x, y_unused);                  // (the second quotient is dead code)
    const float px = __fadd_rn(__fmul_rn(x, P.c_fx), P.c_ppx);
    p.u = Mth::div_const(px, P.c_w_f, P.c_rw);
    p.v = 0.0f;
    return p;
}

template <class Mth, uint32_t THREADS = kBlockThreads>
__device__ __forceinline__ void dense_tile_rowc(const StreamParams& P, const uint16_t* __restrict__ depth,
                                                const uint8_t* __restrict__ color, uint32_t tile0, uint32_t n,
                                                uint8_t* __restrict__ out_bytes, uint4* stage)
{
    static_assert(Mth::kRowConst && Mth::kCvtMode == 2, "the no-overflow row-constant policy");
    // (src.fast(P) holds: launch_fused_dense takes this tile only for 16-aligned rasters with W % 8 == 0)
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    const uint32_t ic = min(i0, n - kPointsPerLane);        // a lane past the stream's end reads its last quad; its records are not stored
    const uint32_t r = P.w_magic ? (__umulhi(ic, P.w_magic) >> P.w_shift) : ic / (uint32_t)P.W;
    const uint32_t c0 = ic - r * (uint32_t)P.W;
    u32x4v dv = load16_asm<true>(depth, ic * 2u);           // what src.fetch() requests, in its order, then the colour row
    u32x4v ma = load16_asm(P.mx, c0 * 4u);
    u32x4v mb = load16_asm(P.mx, c0 * 4u + 16u);
    uint32_t myb = load4_asm(P.my, r * 4u);
    uint32_t crow = load4_asm(P.my, ((uint32_t)P.H + r) * 4u);

    // The wave's windows (wave-uniform): the rows of its first and last pixel (lanes 0 and 63), their colour rows, the stretches.
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t iw = tile0 + wave * 64u * kPointsPerLane;
    const uint32_t il = min(iw + 64u * kPointsPerLane, n) - 1u;
    const uint32_t ra = __builtin_amdgcn_readfirstlane(r), rb = __builtin_amdgcn_readlane(r, 63);
    const cptr<int32_t> tab = (cptr<int32_t>)(uintptr_t)(P.my + P.H);          // [H] colour rows, then the window constants
    const int32_t wp[3] = {tab[P.H], tab[P.H + 1], tab[P.H + 2]};
    const uint32_t lrel = wave * kWaveStageBytes;                                // the wave's part of stage
    uint32_t wsa = 0, lena = 0, wsb = 0, lenb = 0;
    if (iw < n) {    // (a wave past the stream's end has no pixel to stage)
        color_stretch(P, wp, tab[ra], (int32_t)(iw - ra * (uint32_t)P.W), ra == rb ? (int32_t)(il - ra * (uint32_t)P.W) : P.W - 1,
                      kWinBytes, wsa, lena);
        if (rb != ra) color_stretch(P, wp, tab[rb], 0, (int32_t)(il - rb * (uint32_t)P.W), kWinBytes - lena, wsb, lenb);
    }
    // Both stretches back to back, one 16-byte piece per lane per request (piece j -> the wave's stage + 16 j); lanes past the last
    // piece repeat it (nothing past the last piece is read).
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pieces = max((lena + lenb) >> 4, 1u), pa = lena >> 4;     // (no window: piece 0 = the raster's first 16 bytes)
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)stage + lrel;
#pragma unroll
    for (uint32_t k = 0; k < kWinPieces; k++) {
        const uint32_t j = min(k * 64u + lane, pieces - 1u);
        window_piece(color, j < pa ? wsa + 16u * j : wsb + 16u * (j - pa), lds0 + k * 1024u);
    }
    if (lane == 0) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(stage) + lrel + kWinZeroWord) = *(cptr<uint32_t>)(uintptr_t)color;
    // The constants read after the depth has arrived, asked for HERE and held in SGPRs across the wait: the wait is an asm statement,
    // which kept hipcc from issuing their scalar loads before it — every wave paid that round trip between its depth and its first
    // arithmetic. Now it runs beside the Z16 one.
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = P.M[k];
    float c_wm1_f = P.c_wm1_f;
    uint32_t bpp = (uint32_t)P.bpp, stride = (uint32_t)P.stride;
    asm volatile("" : "+s"(M[0]), "+s"(M[1]), "+s"(M[2]), "+s"(M[3]), "+s"(M[4]), "+s"(M[5]), "+s"(M[6]), "+s"(M[7]), "+s"(M[8]),
                      "+s"(M[9]), "+s"(M[10]), "+s"(M[11]), "+s"(c_wm1_f), "+s"(bpp), "+s"(stride));
    static_assert(kWinPieces == 3, "the wait below leaves the window's requests in flight");
    asm volatile("s_waitcnt vmcnt(3)" : "+v"(dv), "+v"(ma), "+v"(mb), "+v"(myb), "+v"(crow));
    PointIn p[8];
    {
        const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w};
        const uint32_t mxs[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t d = (k & 1) ? (dw[k >> 1] >> 16) : (dw[k >> 1] & 0xFFFFu);
            p[k] = deproject_pixel_win<Mth>(P, d, __uint_as_float(mxs[k]), __uint_as_float(myb));
        }
    }
    // The record fields of make_record, and each pixel's colour byte index: 0 for a hole (what u = v = 0 gives in make_record).
    FastCvt<false> cv;
    uint32_t xy[8], zz[8], ci[8];
    const uint32_t row_off = __umul24(crow, stride);     // the lane's colour row, in bytes: one product for its 8 pixels
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float ax = world_mm(M + 0, p[k].X, p[k].Y, p[k].Z);
        const float ay = world_mm(M + 4, p[k].X, p[k].Y, p[k].Z);
        const float az = world_mm(M + 8, p[k].X, p[k].Y, p[k].Z);
        xy[k] = perm((uint32_t)cv.cvt(ay), (uint32_t)cv.cvt(ax), kLoLo);
        zz[k] = (uint32_t)cv.cvt(az);
        const int32_t xi = cv.pixel(__fmaf_rn(p[k].u, P.c_w_f, 0.5f), P.cW - 1, c_wm1_f);
        ci[k] = p[k].Z != 0.0f ? __umul24((uint32_t)xi, bpp) + row_off : 0u;
    }
    // The colour dwords: from the lane's window (the wave's first row's or its last row's), pixel (0, 0)'s word for byte 0; a
    // lane with any other pixel gathers those from the raster as make_record does, with the exact slide-back at its end.
    const bool in_a = r == ra;
    const uint32_t ws = in_a ? wsa : wsb, len = in_a ? lena : lenb;
    const uint32_t wn = len > 3u ? len - 3u : 0u;           // a dword at ws + o lies inside for o < wn
    const uint32_t lb = lrel + (in_a ? 0u : lena), lz = lrel + kWinZeroWord;
    // the window has landed (after the byte indices: the wait is not to be hoisted above the arithmetic)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(ci[0]), "+v"(ci[1]), "+v"(ci[2]), "+v"(ci[3]), "+v"(ci[4]), "+v"(ci[5]), "+v"(ci[6]),
                 "+v"(ci[7]) :: "memory");
    uint32_t wc[8];
    bool miss = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t o = ci[k] - ws;
        const bool in = o < wn;        // a hit never needs the slide-back: the window ends inside the raster
        const uint32_t* qa = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(stage) + (in ? (lb + o) & ~3u : lz));
        wc[k] = __builtin_amdgcn_alignbyte(qa[1], qa[0], ci[k]);      // bytes ci .. ci+3 (window starts are 16-aligned; byte 0: the word)
        miss |= !in && ci[k] != 0u;
    }
    if (__builtin_expect(miss, 0)) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (!(ci[k] - ws < wn) && ci[k] != 0u) {
                ExactCvt exact;
                uint32_t shift;
                const uint32_t off = exact.window(ci[k], P.color_bytes - 4u, shift);
                uint32_t g;
                __builtin_memcpy(&g, color + off, 4);
                wc[k] = g >> shift;
            }
        }
    }
    uint32_t w[20];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const Record a{xy[k], perm(wc[k], zz[k], kLoLo), __builtin_amdgcn_ubfe(wc[k], 16, 8)};
        const Record b{xy[k + 1], perm(wc[k + 1], zz[k + 1], kLoLo), __builtin_amdgcn_ubfe(wc[k + 1], 16, 8)};
        uint32_t* o = w + (k >> 1) * 5;
        o[0] = a.xy;
        o[1] = a.zc;
        o[2] = perm(b.xy, a.b, kLoLo);
        o[3] = perm(b.zc, b.xy, kHiLo);
        o[4] = perm(b.b, b.zc, kHiLo);
    }
    uint4* mine = stage + threadIdx.x * 5;       // over the wave's window: the wave's reads of it are done (their values are in wc)
#pragma unroll
    for (int k = 0; k < 5; k++) mine[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    __syncthreads();

    const uint32_t pts = min(THREADS * kPointsPerLane, n - tile0);
    store_staged<THREADS>(reinterpret_cast<const uint8_t*>(stage), 0u, pts * PCS_POINT_BYTES,
                          out_bytes + (size_t)tile0 * PCS_POINT_BYTES);
}

// ------------------------------------------------------------------------------------------------
// GENERIC tile: predicate and/or downsample and/or unaligned payload. Order-preserving.
//   g0        kept-index (within the stream) of the tile's first kept point
//   out_first output point index (within the whole payload) of kept-index 0 of this stream
// A kept point with kept-index g is written iff g % ds == 0, to output point out_first + g / ds.
// ------------------------------------------------------------------------------------------------
template <class Src, bool PRED, bool DS1, class Arith = SimdArith>
__device__ __forceinline__ void generic_tile(const StreamParams& P, const Src& src, const uint8_t* __restrict__ color,
                                             uint32_t tile0, uint32_t n, uint32_t flags, uint32_t ds,
                                             uint32_t g0, uint32_t out_first, uint8_t* __restrict__ payload_bytes,
                                             uint8_t* stage, uint32_t* wsum)
{
    if (DS1) ds = 1u;
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    PointIn p[8];
    src.load8(P, i0, n, p);

    uint32_t keep, ex = 0;
    if (PRED) {
        keep = keep_mask8(p, i0, n, flags);
        uint32_t wave_total;
        ex = wave_exclusive_scan(__popc(keep), wave_total);
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = wave_total;
    } else {
        const uint32_t mine = (i0 < n) ? min(8u, n - i0) : 0u;
        keep = (1u << mine) - 1u;
    }

    // Records for all 8 points, straight-line (a branch per point would serialise the lane's pixels and put
    // the colour gather behind it); the predicate and the stride only gate the LDS staging below. They are
    // computed BEFORE the barrier of the cross-wave scan so that the colour gathers are in flight while the
    // workgroup waits for its slowest wavefront.
    Record rec[8];
    auto fill = [&](auto& cv) {
#pragma unroll
        for (int k = 0; k < 8; k++) rec[k] = make_record<Arith>(P, color, p[k], cv);
    };
    if (Src::Math::kCvtMode == 2) {
        FastCvt<false> fast;
        fill(fast);
        if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    } else if (Src::Math::kCvtMode == 1) {
        FastCvt<true> fast;
        fill(fast);
        if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    } else {
        ExactCvt exact;
        fill(exact);
    }

    uint32_t lane_first, tile_kept;
    if (PRED) {
        __syncthreads();
        const int wave = threadIdx.x >> 6;
        uint32_t before = 0;
        for (int w = 0; w < wave; w++) before += wsum[w];
        tile_kept = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        lane_first = before + ex;
    } else {
        const uint32_t pts = min(kTilePoints, n - tile0);
        lane_first = min(threadIdx.x * kPointsPerLane, pts);
        tile_kept = pts;
    }

    // output range of the tile, in points: q = out_first + ceil(g/ds) for g in [g0, g0 + tile_kept)
    const uint32_t q_lo = out_first + (DS1 ? g0 : (g0 + ds - 1) / ds);
    const uint32_t q_hi = out_first + (DS1 ? g0 + tile_kept : (g0 + tile_kept + ds - 1) / ds);
    uint8_t* gdst = payload_bytes + (size_t)q_lo * PCS_POINT_BYTES;
    const uint32_t head = (uint32_t)((uintptr_t)gdst & 15u);

    // kept-index of the lane's first kept point, and (for a stride) its quotient / remainder once per lane
    uint32_t g = g0 + lane_first;
    uint32_t gq = DS1 ? g : g / ds, gr = DS1 ? 0u : g - gq * ds;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if ((keep >> k) & 1u) {
            if (gr == 0u) {
                stage_record(stage, head + (out_first + gq - q_lo) * PCS_POINT_BYTES, rec[k]);
            }
            if (DS1) gq++;
            else if (++gr == ds) { gr = 0u; gq++; }
        }
    }
    __syncthreads();
    store_staged(stage, head, (q_hi - q_lo) * PCS_POINT_BYTES, gdst);
}

// ------------------------------------------------------------------------------------------------
// SINGLE-PASS ordered compaction (predicate active, stride 1): one launch instead of count + scan + emit,
// and the Z16 raster is read once.
//
//  * Tile ids are handed out by an atomic ticket in the order workgroups START, never by blockIdx: a tile
//    only ever waits for lower tickets, whose workgroups are already running -> no dependence on the
//    (unspecified) dispatch order, no deadlock.
//  * Every tile publishes ONE 64-bit descriptor {[63:34] launch generation, [33:32] ready, [31:0] kept
//    count} as soon as it has counted — flag and payload travel in one naturally aligned agent-scope 8-byte
//    store, stale descriptors of earlier launches read as "not ready", nothing is ever cleared.
//  * Placement is a DIRECT SUM, not a chained scan: a tile adds up the counts of its own stream's earlier
//    tiles (all 256 lanes stride over <= a few hundred descriptors) plus one total per earlier stream
//    (published by that stream's last tile). Nobody waits on anything but first-level publications, which
//    happen within the first microseconds of a workgroup's life; a chained look-back, which this replaces,
//    crawled ~64 tiles per microsecond through ~1500 resident tiles (65-70 us per frame-set).
//  * Every wait is bounded; on expiry the error word is set and the host re-runs the frame with the
//    three-pass path.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kDescReady = 1u;
constexpr uint32_t kSpinLimit = 1u << 18;

__device__ __forceinline__ uint64_t desc_pack(uint32_t gen, uint32_t status, uint32_t value)
{
    return ((uint64_t)((gen << 2) | status) << 32) | (uint64_t)value;
}

// Value of a descriptor once its writer has published it for this launch generation (bounded wait).
__device__ __forceinline__ uint32_t desc_wait(const uint64_t* __restrict__ d, uint32_t gen, uint32_t* __restrict__ error)
{
    for (uint32_t spins = 0;; spins++) {
        const uint64_t v = __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t hi = (uint32_t)(v >> 32);
        if ((hi >> 2) == gen && (hi & 3u) == kDescReady) return (uint32_t)v;
        if (spins > kSpinLimit) { atomicExch(error, 1u); return 0u; }
        __builtin_amdgcn_s_sleep(2);
    }
}

struct CompactArgs {
    unsigned long long* ticket;       // never reset; ticket_base = its value when this launch was enqueued
    unsigned long long  ticket_base;
    uint64_t*           desc;         // one descriptor per tile of this launch: the tile's kept count
    uint64_t*           stream_desc;  // [stream] kept count of the whole stream (published by its last tile)
    uint32_t*           stream_end;   // [stream] inclusive global prefix at the stream's last tile (plain, for counts)
    const uint32_t*     chain_in;     // output points written by earlier launches of this frame-set (or null)
    uint32_t*           error;
    uint32_t            gen;
    uint32_t            flags;
    int32_t*            counts;       // [n_total + 1] per-stream kept counts + total, written by each launch's last tile
    int32_t             n_total;      // streams of the whole frame-set
    int32_t             last_launch;  // this launch holds the frame-set's last stream
};

template <class Mth>
__global__ __launch_bounds__(kBlockThreads)
void pcs_fused_compact_kernel(const StreamParams* __restrict__ params, int stream0, int n_launch, FramePtrs fp,
                              CompactArgs a, uint8_t* __restrict__ payload_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t psum[8];
    __shared__ uint32_t bcast[1];

    uint32_t gtile;
    if (a.ticket) {         // tile ids in workgroup START order (dispatch-order independent, but 3600 returning
        if (threadIdx.x == 0) bcast[0] = (uint32_t)(atomicAdd(a.ticket, 1ull) - a.ticket_base);   // atomics on one line)
        __syncthreads();
        gtile = bcast[0];
    } else {
        gtile = blockIdx.x; // relies on in-order dispatch for progress; the bounded waits catch anything else
    }

    // ticket -> (stream, tile): tiles are numbered stream-major
    int s = 0;
    uint32_t t = gtile, tiles_s = 0;
    for (;; s++) {
        tiles_s = (params[stream0 + s].n_points + kTilePoints - 1) / kTilePoints;
        if (t < tiles_s || s == n_launch - 1) break;
        t -= tiles_s;
    }
    const StreamParams& P = params[stream0 + s];
    const uint32_t n = P.n_points;
    const uint32_t tile0 = t * kTilePoints;
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    const uint8_t* __restrict__ color = fp.color[s];

    DepthSource<true, true, Mth> src{fp.depth[s]};
    PointIn p[8];
    src.load8(P, i0, n, p);
    const uint32_t keep = keep_mask8(p, i0, n, a.flags);

    uint32_t wave_total;
    const uint32_t ex = wave_exclusive_scan(__popc(keep), wave_total);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 63) wsum[wave] = wave_total;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += wsum[w];
    const uint32_t tile_kept = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const uint32_t lane_first = before + ex;

    // publish this tile's kept count as early as possible: later tiles only ever wait for this store
    if (threadIdx.x == 0)
        __hip_atomic_store(a.desc + gtile, desc_pack(a.gen, kDescReady, tile_kept), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);

    // records for all 8 points, straight-line (the predicate only gates the staging below); the tiles in
    // front of this one publish their counts meanwhile
    Record rec[8];
    auto fill = [&](auto& cv) {
#pragma unroll
        for (int k = 0; k < 8; k++) rec[k] = make_record(P, color, p[k], cv);
    };
    if (Mth::kCvtMode == 2) {
        FastCvt<false> fast;
        fill(fast);
        if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    } else if (Mth::kCvtMode == 1) {
        FastCvt<true> fast;
        fill(fast);
        if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    } else {
        ExactCvt exact;
        fill(exact);
    }

    // placement: kept points of this stream's earlier tiles (<= a few hundred descriptors, all 256 lanes
    // stride over them) + the totals of the earlier streams (published once by each stream's last tile).
    // No chain: nobody waits for anything but first-level publications. (Issuing these loads before the
    // records, to hide their round trip, measured 38-42 us instead of 27-29: most of the neighbours have not
    // published yet at that point and everything is polled twice.)
    uint32_t own = 0, tot = 0;
    const uint32_t first = gtile - t;
    for (uint32_t j = first + threadIdx.x; j < gtile; j += kBlockThreads) own += desc_wait(a.desc + j, a.gen, a.error);
    if ((int)threadIdx.x < s) tot = desc_wait(a.stream_desc + stream0 + threadIdx.x, a.gen, a.error);
    const uint32_t tot_lane = tot;     // lane e < s: kept points of stream stream0 + e
    own = wave_sum(own);
    tot = wave_sum(tot);
    if (lane == 0) { psum[wave] = own; psum[4 + wave] = tot; }
    __syncthreads();
    const uint32_t own_excl = psum[0] + psum[1] + psum[2] + psum[3];
    const uint32_t chain = a.chain_in ? *a.chain_in : 0u;
    const uint32_t q_lo = chain + psum[4] + psum[5] + psum[6] + psum[7] + own_excl;   // global output point index
    if (threadIdx.x == 0 && t == tiles_s - 1) {
        __hip_atomic_store(a.stream_desc + stream0 + s, desc_pack(a.gen, kDescReady, own_excl + tile_kept), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        a.stream_end[stream0 + s] = q_lo + tile_kept;
    }
    // The launch's very last tile has every stream total of the launch in its lanes: it hands the counts back itself
    // (a separate one-workgroup kernel for this cost 4.8 us of launch latency per frame-set).
    if (a.counts && s == n_launch - 1 && t == tiles_s - 1) {
        if ((int)threadIdx.x < s) a.counts[stream0 + threadIdx.x] = (int32_t)tot_lane;
        if (threadIdx.x == 0) {
            a.counts[stream0 + s] = (int32_t)(own_excl + tile_kept);
            if (a.last_launch) a.counts[a.n_total] = (int32_t)(q_lo + tile_kept);
        }
    }

    uint8_t* gdst = payload_bytes + (size_t)q_lo * PCS_POINT_BYTES;
    const uint32_t head = (uint32_t)((uintptr_t)gdst & 15u);
    uint32_t rank = lane_first;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if ((keep >> k) & 1u) {
            stage_record(stage, head + rank * PCS_POINT_BYTES, rec[k]);
            rank++;
        }
    }
    __syncthreads();
    store_staged(stage, head, tile_kept * PCS_POINT_BYTES, gdst);
}


// ------------------------------------------------------------------------------------------------
// Kernels
// ------------------------------------------------------------------------------------------------

template <bool DDIST, bool CDIST, class Mth, uint32_t THREADS = kBlockThreads>
__global__ __launch_bounds__(THREADS, 7)     // <= 72 VGPRs for every instantiation (one landed on 73 -> 6 waves/SIMD); A/B on one box: no measurable change, 8 spills and is slower
                                             // (the row-constant tile, 56 VGPRs, fits 8 once its constants take <= 80 SGPRs: measured slower too)
void pcs_fused_dense_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp,
                            uint8_t* __restrict__ payload_bytes)
{
    __shared__ uint4 stage[THREADS * kPointsPerLane * PCS_POINT_BYTES / 16];
    const int s = blockIdx.y;
    const StreamParams& P = params[stream0 + s];
    request_constants(P, fp.depth[s], fp.color[s], payload_bytes);
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * (THREADS * kPointsPerLane);
    if (tile0 >= n) return;
    if constexpr (Mth::kRowConst) {
        dense_tile_rowc<Mth, THREADS>(P, fp.depth[s], fp.color[s], tile0, n, payload_bytes + (size_t)P.out_base * PCS_POINT_BYTES, stage);
    } else {
        DepthSource<DDIST, CDIST, Mth> src{fp.depth[s]};
        dense_tile<DepthSource<DDIST, CDIST, Mth>, THREADS>(P, src, fp.color[s], tile0, n, payload_bytes + (size_t)P.out_base * PCS_POINT_BYTES, stage);
    }
}

// K frame-sets of the same streams in one launch: blockIdx.z = frame-set, blockIdx.y = stream. Same tile code, same
// bytes; only the fill/drain of the launch is shared by K sets (pcs_process_frames_device_batch).
template <bool DDIST, bool CDIST, class Mth>
__global__ __launch_bounds__(kBlockThreads, 7)
void pcs_fused_dense_batch_kernel(const StreamParams* __restrict__ params, BatchPtrs bp)
{
    __shared__ uint4 stage[kDenseStageBytes / 16];
    const int s = blockIdx.y;
    const StreamParams& P = params[s];
    const int e = blockIdx.z * gridDim.y + s;
    request_constants(P, bp.depth[e], bp.color[e], bp.payload[blockIdx.z]);
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    if constexpr (Mth::kRowConst) {
        dense_tile_rowc<Mth>(P, bp.depth[e], bp.color[e], tile0, n, bp.payload[blockIdx.z] + (size_t)P.out_base * PCS_POINT_BYTES, stage);
    } else {
        DepthSource<DDIST, CDIST, Mth> src{bp.depth[e]};
        dense_tile(P, src, bp.color[e], tile0, n, bp.payload[blockIdx.z] + (size_t)P.out_base * PCS_POINT_BYTES, stage);
    }
}

// Count pass: kept points per tile. (Folding the per-stream scan into this launch through a last-arriver
// counter was measured and is slower — 450 returning atomics per counter line cost more than the separate
// 5 us scan launch)
// A workgroup counts kCountTiles consecutive tiles, their (independent) Z16 loads issued back to back with no branch
// between them. Measured on 8 x 720p (14.7 MB of Z16, rocprofv3 average): 1 tile 5.4 us, 2 tiles 5.4 us, 4 tiles
// 5.9 us, 8 tiles 6.9 us — latency, not bandwidth; 2 halves the workgroups at no cost.
constexpr int kCountTiles = 2;
template <bool DDIST, bool CDIST>
__device__ __forceinline__ void count_tiles(const StreamParams& P, const uint16_t* __restrict__ dp, uint32_t flags,
                                            uint32_t* __restrict__ tile_counts, uint32_t (*wsum)[4])
{
    const uint32_t n = P.n_points;
    const uint32_t tile_first = blockIdx.x * kCountTiles;
    if (tile_first * kTilePoints >= n) return;
    uint32_t c[kCountTiles];
    const bool cut = (flags & PCS_FLAG_CUTOFF) != 0;
    if (P.z_zero_iff_d_zero && (!cut || P.cut_dmax != 0u)) {
        // The predicate from the Z16 words alone, no deprojection:
        //  * z = depth_scale * d is zero exactly when d is (the host checked the scale: finite, and scale*1 != 0);
        //  * -c (:504-511) keeps 0 < z <= 1.5 and -2 < x <= 2. z is monotone in d, so the z test is 1 <= d <= cut_dmax
        //    (the host found the largest d with fl(depth_scale * d) <= 1.5f), and cut_dmax is only non-zero when the host
        //    has also shown that |x| = |fl(z * mx)| < 2 for every column whenever z <= 1.5 (no depth distortion,
        //    1.5 * max|mx| < 2 with slack) — true for any lens narrower than 106 degrees.
        const uint32_t dmax = cut ? P.cut_dmax : 0xFFFFu;
        uint4 dv[kCountTiles];
        const bool aligned = ((uintptr_t)dp & 15) == 0 && n >= 8;      // uniform over the launch
        if (aligned) {
            // branch-free: a lane past the end re-reads the stream's first 16 bytes (and gathers below), so the four
            // loads are issued back to back with no wait between them
#pragma unroll
            for (int q = 0; q < kCountTiles; q++) {
                const uint32_t i0 = (tile_first + q) * kTilePoints + threadIdx.x * kPointsPerLane;
                dv[q] = *reinterpret_cast<const uint4*>(dp + ((i0 + 8 <= n) ? i0 : 0u));
            }
        } else {
#pragma unroll
            for (int q = 0; q < kCountTiles; q++) dv[q] = make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < kCountTiles; q++) {
            const uint32_t i0 = (tile_first + q) * kTilePoints + threadIdx.x * kPointsPerLane;
            uint32_t dw[4] = {dv[q].x, dv[q].y, dv[q].z, dv[q].w};
            if (!(aligned && i0 + 8 <= n)) {            // ragged end / unaligned raster: gather the halfwords one by one
                dw[0] = dw[1] = dw[2] = dw[3] = 0u;
                for (uint32_t k = 0; k < 8 && i0 + k < n; k++) dw[k >> 1] |= (uint32_t)dp[i0 + k] << ((k & 1u) * 16u);
            }
            uint32_t rng = 0, nz = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t d = (k & 1) ? (dw[k >> 1] >> 16) : (dw[k >> 1] & 0xFFFFu);
                nz  |= (uint32_t)(d != 0u) << k;
                rng |= (uint32_t)(d != 0u && d <= dmax) << k;
            }
            c[q] = __popc(keep_from_bits(rng, nz, i0, n, flags));
        }
    } else {
        DepthSource<DDIST, CDIST> src{dp};
#pragma unroll
        for (int q = 0; q < kCountTiles; q++) {
            const uint32_t i0 = (tile_first + q) * kTilePoints + threadIdx.x * kPointsPerLane;
            PointIn p[8];
            src.load8(P, i0, n, p);
            c[q] = __popc(keep_mask8(p, i0, n, flags));
        }
    }
#pragma unroll
    for (int q = 0; q < kCountTiles; q++) {
        const uint32_t w = wave_sum(c[q]);
        if ((threadIdx.x & 63) == 0) wsum[q][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x < kCountTiles && (tile_first + threadIdx.x) * kTilePoints < n)
        tile_counts[P.tile_base + tile_first + threadIdx.x] =
            wsum[threadIdx.x][0] + wsum[threadIdx.x][1] + wsum[threadIdx.x][2] + wsum[threadIdx.x][3];
}

template <bool DDIST, bool CDIST>
__global__ __launch_bounds__(kBlockThreads)
void pcs_fused_count_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp, uint32_t flags,
                            uint32_t* __restrict__ tile_counts)
{
    __shared__ uint32_t wsum[kCountTiles][4];
    const int s = blockIdx.y;
    // (no request_constants here: the usual route needs four words of the stream's constants, and 98 SGPRs would cap the
    // kernel at 6 workgroups per CU where 8 fit)
    count_tiles<DDIST, CDIST>(params[stream0 + s], fp.depth[s], flags, tile_counts, wsum);
}

// K frame-sets: blockIdx.z = frame-set, its tile counts at tile_counts + z * total_tiles.
template <bool DDIST, bool CDIST>
__global__ __launch_bounds__(kBlockThreads)
void pcs_fused_count_batch_kernel(const StreamParams* __restrict__ params, BatchPtrs bp, uint32_t flags,
                                  uint32_t* __restrict__ tile_counts, uint32_t total_tiles)
{
    __shared__ uint32_t wsum[kCountTiles][4];
    const int s = blockIdx.y;
    count_tiles<DDIST, CDIST>(params[s], bp.depth[blockIdx.z * gridDim.y + s], flags,
                              tile_counts + (size_t)blockIdx.z * total_tiles, wsum);
}

// (Placing the emit tiles straight from per-chunk totals of the count pass — no scan launch, four extra L2-resident loads
// per lane riding on the tile's existing barrier — was built and measured: 32.4 vs 32.5 us on 8 x 720p and 127 vs 107 us
// on 16 x 1080p. Whatever the scan launch costs, extra memory instructions in the emit tile cost at least as much.)
template <bool PRED, bool DS1, class Mth>
__global__ __launch_bounds__(kBlockThreads, EMIT_WAVES)
void pcs_fused_emit_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp, uint32_t flags,
                           uint32_t ds, const uint32_t* __restrict__ tile_prefix,
                           const uint32_t* __restrict__ stream_kept, uint8_t* __restrict__ payload_bytes,
                           int32_t* __restrict__ total_out, int n_total_streams)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y;
    if (PRED && total_out && blockIdx.x == 0 && stream0 + s == 0 && threadIdx.x == 0) {
        // the grand total rides on the first workgroup of the first emit launch (the scan kernel used to compute it
        // with a last-arriver atomic: a third of its 4.8 us)
        uint32_t tot = 0;
        for (int e = 0; e < n_total_streams; e++) tot += DS1 ? stream_kept[e] : (stream_kept[e] + ds - 1) / ds;
        *total_out = (int32_t)tot;
    }
    const StreamParams& P = params[stream0 + s];
    request_constants<true, Mth::kIdentR>(P, fp.depth[s], fp.color[s], payload_bytes);
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    DepthSource<true, true, Mth> src{fp.depth[s]};
    const uint32_t g0 = PRED ? tile_prefix[P.tile_base + blockIdx.x] : tile0;
    uint32_t out_first = P.out_base;
    if (PRED) {     // a7: this camera starts after the strided kept points of all earlier cameras
        out_first = 0;
        for (int e = 0; e < stream0 + s; e++) out_first += DS1 ? stream_kept[e] : (stream_kept[e] + ds - 1) / ds;
    }
    generic_tile<DepthSource<true, true, Mth>, PRED, DS1>(P, src, fp.color[s], tile0, n, flags, ds, g0, out_first,
                                                  payload_bytes, stage, wsum);
}

// K frame-sets of ordered compaction (stride 1): blockIdx.z = frame-set. Prefixes at tile_prefix + z * total_tiles, the
// per-stream kept totals at stream_kept + z * S; frame-set z's total is written by its first workgroup.
template <class Mth>
__global__ __launch_bounds__(kBlockThreads, 6)
void pcs_fused_emit_batch_kernel(const StreamParams* __restrict__ params, BatchPtrs bp, uint32_t flags,
                                 const uint32_t* __restrict__ tile_prefix, const uint32_t* __restrict__ stream_kept,
                                 uint32_t total_tiles, BatchCounts bc)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y, S = gridDim.y, z = blockIdx.z;
    const uint32_t* __restrict__ kept = stream_kept + z * S;
    if (blockIdx.x == 0 && s == 0 && threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int e = 0; e < S; e++) tot += kept[e];
        bc.counts[z][S] = (int32_t)tot;
    }
    const StreamParams& P = params[s];
    // (no request_constants here: with it hipcc settles on 76 VGPRs = 6 waves/SIMD instead of 72 = 7, 27.5 vs 25.0 us per
    // set; this launch is 4 x as long as a one-set launch, so its first wave of workgroups matters a quarter as much)
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    DepthSource<true, true, Mth> src{bp.depth[z * S + s]};
    const uint32_t g0 = tile_prefix[(size_t)z * total_tiles + P.tile_base + blockIdx.x];
    uint32_t out_first = 0;
    for (int e = 0; e < s; e++) out_first += kept[e];
    generic_tile<DepthSource<true, true, Mth>, true, true>(P, src, bp.color[z * S + s], tile0, n, flags, 1u, g0, out_first,
                                                           bp.payload[z], stage, wsum);
}

// Exclusive scan of the tile counts, one workgroup of 1024 lanes PER STREAM (streams scan concurrently).
// Writes the tile prefixes, the stream's kept total and its output count ceil(kept / stride); the
// stream's base in the stitched payload is summed from the totals by the emit kernel, and the grand total
// by whichever workgroup arrives last (agent-scope counter).
__global__ __launch_bounds__(1024)
void pcs_scan_kernel(const StreamParams* __restrict__ params, int stream0, int n_streams, uint32_t override_n,
                     uint32_t ds, const uint32_t* __restrict__ tile_counts, uint32_t* __restrict__ tile_prefix,
                     uint32_t* __restrict__ stream_kept, int32_t* __restrict__ counts, uint32_t* __restrict__ arrive)
{
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t carry_s;
    const int s = blockIdx.x;
    const uint32_t n = override_n ? override_n : params[stream0 + s].n_points;
    const uint32_t tiles = (n + kTilePoints - 1) / kTilePoints;
    const uint32_t tb = override_n ? 0u : params[stream0 + s].tile_base;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < tiles; t0 += 1024) {
        const uint32_t t = t0 + threadIdx.x;
        // (a count can never exceed a tile: clamped, so that counts handed in by a caller — pcs_process_frames_device_counted —
        // cannot steer a tile's stores past the payload's worst-case capacity whatever they contain)
        const uint32_t c = (t < tiles) ? min(tile_counts[tb + t], min(kTilePoints, n - t * kTilePoints)) : 0u;
        uint32_t wave_total;
        const uint32_t ex = wave_exclusive_scan(c, wave_total);
        if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = wave_total;
        __syncthreads();
        uint32_t before = carry_s;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wtot[w];
        if (t < tiles) tile_prefix[tb + t] = before + ex;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + ex + c;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t kept = carry_s;
        const uint32_t outc = (kept + ds - 1) / ds;
        if (stream_kept) stream_kept[stream0 + s] = kept;
        if (counts && !arrive) {
            counts[stream0 + s] = (int32_t)outc;      // the emit kernel that follows adds up the grand total
        } else if (counts) {
            // grand total: the last workgroup to arrive adds up the per-stream outputs. The per-stream
            // counts are written with agent-scope stores and read back with agent-scope loads, and the
            // arrival counter is an agent-scope atomic, so the last arriver sees every other write.
            __hip_atomic_store(counts + stream0 + s, (int32_t)outc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t ticket = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ticket == (uint32_t)n_streams - 1u) {
                    int32_t tot = 0;
                for (int e = 0; e < n_streams; e++)
                    tot += __hip_atomic_load(counts + stream0 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                counts[stream0 + n_streams] = tot;
                __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            }
        }
    }
}

// The scan of K frame-sets: blockIdx.x = stream, blockIdx.y = frame-set (stride 1, no grand-total atomic: the emit
// launch that follows adds the totals).
__global__ __launch_bounds__(1024)
void pcs_scan_batch_kernel(const StreamParams* __restrict__ params, const uint32_t* __restrict__ tile_counts,
                           uint32_t* __restrict__ tile_prefix, uint32_t* __restrict__ stream_kept, uint32_t total_tiles,
                           BatchCounts bc)
{
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t carry_s;
    const int s = blockIdx.x, z = blockIdx.y;
    const uint32_t n = params[s].n_points;
    const uint32_t tiles = (n + kTilePoints - 1) / kTilePoints;
    const size_t tb = (size_t)z * total_tiles + params[s].tile_base;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < tiles; t0 += 1024) {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = (t < tiles) ? tile_counts[tb + t] : 0u;
        uint32_t wave_total;
        const uint32_t ex = wave_exclusive_scan(c, wave_total);
        if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = wave_total;
        __syncthreads();
        uint32_t before = carry_s;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wtot[w];
        if (t < tiles) tile_prefix[tb + t] = before + ex;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + ex + c;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stream_kept[z * gridDim.x + s] = carry_s;
        bc.counts[z][s] = (int32_t)carry_s;
    }
}


// ---- a2 twin -----------------------------------------------------------------------------------
template <uint32_t THREADS = kBlockThreads>
__global__ __launch_bounds__(THREADS)
void pcs_pack_dense_kernel(const StreamParams* __restrict__ params, int stream, VertexPtrs vp,
                                  uint8_t* __restrict__ out_bytes)
{
    __shared__ uint4 stage[THREADS * kPointsPerLane * PCS_POINT_BYTES / 16];
    const StreamParams& P = params[stream];
    const uint32_t n = vp.n_points;
    const uint32_t tile0 = blockIdx.x * (THREADS * kPointsPerLane);
    if (tile0 >= n) return;
    VertexSource src{vp.vertices, vp.texcoords};
    dense_tile<VertexSource, THREADS>(P, src, vp.color, tile0, n, out_bytes, stage);
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_pack_count_kernel(const StreamParams* __restrict__ params, int stream, VertexPtrs vp, uint32_t flags,
                           uint32_t* __restrict__ tile_counts)
{
    __shared__ uint32_t wsum[4];
    const uint32_t n = vp.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    // the predicate needs x and z only; read them straight from global (12-byte stride)
    PointIn p[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t i = i0 + k;
        p[k] = PointIn{0, 0, 0, 0, 0};
        if (i < n) { p[k].X = vp.vertices[3 * (size_t)i]; p[k].Z = vp.vertices[3 * (size_t)i + 2]; }
    }
    uint32_t c = __popc(keep_mask8(p, i0, n, flags));
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    (void)params; (void)stream;
}

template <bool PRED>
__global__ __launch_bounds__(kBlockThreads)
void pcs_pack_emit_kernel(const StreamParams* __restrict__ params, int stream, VertexPtrs vp, uint32_t flags,
                          const uint32_t* __restrict__ tile_prefix, uint8_t* __restrict__ out_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const StreamParams& P = params[stream];
    const uint32_t n = vp.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    VertexSource src{vp.vertices, vp.texcoords};
    const uint32_t g0 = PRED ? tile_prefix[blockIdx.x] : tile0;
    generic_tile<VertexSource, PRED, true>(P, src, vp.color, tile0, n, flags, 1u, g0, 0u, out_bytes, stage, wsum);
}

// Batched a2 twin (no predicate): blockIdx.y = cloud. One launch for all cameras of a frame-set instead of one
// latency-bound launch per camera (the reference calls copyPointCloudXYZRGBToBufferSIMD once per camera process).
template <bool ALIGNED>
__global__ __launch_bounds__(kBlockThreads)
void pcs_pack_batch_kernel(const StreamParams* __restrict__ params, PackBatch pb)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int e = blockIdx.y;
    const VertexPtrs vp = pb.v[e];
    const StreamParams& P = params[pb.stream[e]];
    const uint32_t n = vp.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    VertexSource src{vp.vertices, vp.texcoords};
    if (ALIGNED)
        dense_tile(P, src, vp.color, tile0, n, pb.out[e], reinterpret_cast<uint4*>(stage));
    else
        generic_tile<VertexSource, false, true>(P, src, vp.color, tile0, n, 0u, 1u, tile0, 0u, pb.out[e], stage, wsum);
}

// ---- a5 alone ----------------------------------------------------------------------------------
template <bool DDIST, bool CDIST>
__global__ __launch_bounds__(kBlockThreads)
void pcs_deproject_kernel(const StreamParams* __restrict__ params, int stream, const uint16_t* __restrict__ depth,
                          float* __restrict__ vertices, float* __restrict__ texcoords)
{
    const StreamParams& P = params[stream];
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= P.n_points) return;
    const uint32_t r = i / (uint32_t)P.W;
    const uint32_t c = i - r * (uint32_t)P.W;
    const PointIn p = deproject_pixel<DDIST, CDIST, IeeeMath>(P, depth[i], as_global(P.mx)[c], as_global(P.my)[r]);
    vertices[3 * (size_t)i + 0] = p.X;
    vertices[3 * (size_t)i + 1] = p.Y;
    vertices[3 * (size_t)i + 2] = p.Z;
    texcoords[2 * (size_t)i + 0] = p.u;
    texcoords[2 * (size_t)i + 1] = p.v;
}

// ---- the centre's re-transform of packed payloads (src/pcs-multicamera-optimized.cpp:226-265, 289) -------------------------
// What pcs-multicamera-optimized does to every camera's payload before it concatenates them: int16 millimetres -> float metres
// (`(float)buffer[..] / CONV_RATE`, CONV_RATE a `const float` 1000.0 in that file, :46, :237-239), pcl::transformPointCloud with
// transform[thread_num] (:289), float metres -> int16 millimetres (`static_cast<short>(x * CONV_RATE)`, :255-257), colour bytes
// re-packed (:240-242, :258-259: R | G<<8 survives as it is, the high byte of the B short is cleared). The affine is evaluated in
// the order of PCL 1.8's transforms.hpp (Ubuntu 18.04's libpcl-dev, Dockerfile:1,24) — ((m0*x + m1*y) + m2*z) + m3, every product
// and sum individually rounded (the target is built without -mfma, src/CMakeLists.txt) — third-party, so "parity unpinned".
// HBM-bound: 10 B in + 10 B out per kept record. One tile = 2048 output records: the tile's input bytes come in as
// lane-contiguous 16-byte loads into LDS at the input's 16-byte phase, every lane takes its 8 records into registers, and the
// results are parked at the OUTPUT's phase and leave as 16-byte nontemporal stores (store_staged) — the same LDS buffer twice.
__device__ __forceinline__ void load_staged(uint8_t* lds, uint32_t head, uint32_t nbytes, const uint8_t* g)
{
    const uint8_t* g0 = g - head;                            // 16-byte aligned
    const uint32_t end = head + nbytes;
    const uint32_t first_full = (head + 15u) >> 4, last_full = end >> 4;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (uint32_t j = first_full + threadIdx.x; j < last_full; j += kBlockThreads)
        reinterpret_cast<u32x4*>(lds)[j] = reinterpret_cast<const u32x4*>(g0)[j];
    const uint32_t head_end = min(first_full << 4, end);     // ragged ends as 2-byte loads: never a byte outside [g, g + nbytes)
    for (uint32_t b = head + 2u * threadIdx.x; b < head_end; b += 2u * kBlockThreads)
        *reinterpret_cast<uint16_t*>(lds + b) = *reinterpret_cast<const uint16_t*>(g0 + b);
    if (last_full >= first_full) {
        const uint32_t tail_begin = max(last_full << 4, head_end);
        for (uint32_t b = tail_begin + 2u * threadIdx.x; b < end; b += 2u * kBlockThreads)
            *reinterpret_cast<uint16_t*>(lds + b) = *reinterpret_cast<const uint16_t*>(g0 + b);
    }
}

// stage_record read backwards: one record from a 2-byte aligned LDS offset with aligned accesses only.
__device__ __forceinline__ Record unstage_record(const uint8_t* lds, uint32_t off)
{
    const bool odd = (off & 2u) != 0u;
    const uint32_t h_off = odd ? off : off + 8u;
    const uint32_t a_off = odd ? off + 2u : off;
    const uint32_t h = *reinterpret_cast<const uint16_t*>(lds + h_off);
    const uint32_t a = *reinterpret_cast<const uint32_t*>(lds + a_off);
    const uint32_t b = *reinterpret_cast<const uint32_t*>(lds + a_off + 4u);
    Record r;
    r.xy = odd ? perm(a, h, kLoLo) : a;
    r.zc = odd ? perm(b, a, kHiLo) : b;
    r.b = odd ? (b >> 16) : h;
    return r;
}

__device__ __forceinline__ uint32_t retransform_mm(const float* __restrict__ Mr, float x, float y, float z)
{
    const float a = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Mr[0], x), __fmul_rn(Mr[1], y)), __fmul_rn(Mr[2], z)), Mr[3]);
    return (uint32_t)cvtt_x86(__fmul_rn(a, 1000.0f)) & 0xFFFFu;          // static_cast<short>: cvttss2si, low 16 bits
}

__device__ __forceinline__ Record retransform_record(const float* __restrict__ M, const Record& r)
{
    const float x = (float)(int32_t)(int16_t)(r.xy & 0xFFFFu) / 1000.0f;  // correctly rounded division (TU flag)
    const float y = (float)((int32_t)r.xy >> 16) / 1000.0f;
    const float z = (float)(int32_t)(int16_t)(r.zc & 0xFFFFu) / 1000.0f;
    Record o;
    o.xy = retransform_mm(M + 0, x, y, z) | (retransform_mm(M + 4, x, y, z) << 16);
    o.zc = retransform_mm(M + 8, x, y, z) | (r.zc & 0xFFFF0000u);
    o.b = r.b & 0xFFu;
    return o;
}

template <bool DS1>
__global__ __launch_bounds__(kBlockThreads)
void pcs_transform_payload_kernel(XformBatch xb)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const XformCloud& C = xb.c[blockIdx.y];
    const uint32_t n_out = C.n_out;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n_out) return;
    const uint32_t pts = min(kTilePoints, n_out - tile0);
    uint8_t* gdst = C.out + (size_t)tile0 * PCS_POINT_BYTES;
    const uint32_t ohead = (uint32_t)((uintptr_t)gdst & 15u);
    Record rec[kPointsPerLane];
    if (DS1 && pts == kTilePoints && ohead == 0u &&
        (((uintptr_t)C.in + (size_t)tile0 * PCS_POINT_BYTES) & 15u) == 0u) {
        // FULL, 16-byte aligned tile (every tile but the last of a camera whose payload starts on a 16-byte boundary — what
        // hipMalloc and the stitched offsets of standard rasters give): a lane reads its own 8 consecutive records, 80 contiguous
        // bytes, as five 16-byte loads straight into registers (the a2 twin's reader: the L1 merges the wavefront's 64 x 5 pieces),
        // transforms them there and parks 5 x 16 bytes at LDS[lane * 80] (conflict-free); one LDS trip and one barrier instead
        // of two of each.
        const uint4* q = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(C.in) + (size_t)tile0 * PCS_POINT_BYTES) +
                         threadIdx.x * 5u;
        uint32_t w[20];
#pragma unroll
        for (int j = 0; j < 5; j++) { const uint4 v = q[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
#pragma unroll
        for (int k = 0; k < 8; k += 2) {                          // two records = five dwords: xy zc b|x' y'|z' c'|b'
            uint32_t* o = w + (k >> 1) * 5;
            Record a, b;
            a.xy = o[0]; a.zc = o[1]; a.b = o[2] & 0xFFFFu;
            b.xy = perm(o[3], o[2], kHiLo); b.zc = perm(o[4], o[3], kHiLo); b.b = o[4] >> 16;
            a = retransform_record(C.M, a);
            b = retransform_record(C.M, b);
            o[0] = a.xy; o[1] = a.zc;
            o[2] = perm(b.xy, a.b, kLoLo);
            o[3] = perm(b.zc, b.xy, kHiLo);
            o[4] = perm(b.b, b.zc, kHiLo);
        }
        uint4* mine = reinterpret_cast<uint4*>(stage) + threadIdx.x * 5u;
#pragma unroll
        for (int j = 0; j < 5; j++) mine[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
        __syncthreads();
        store_staged(stage, 0u, kTilePoints * PCS_POINT_BYTES, gdst);
        return;
    }
    if (DS1) {
        const uint8_t* gsrc = reinterpret_cast<const uint8_t*>(C.in) + (size_t)tile0 * PCS_POINT_BYTES;
        const uint32_t ihead = (uint32_t)((uintptr_t)gsrc & 15u);
        load_staged(stage, ihead, pts * PCS_POINT_BYTES, gsrc);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPointsPerLane; k++) {
            const uint32_t j = threadIdx.x + (uint32_t)k * kBlockThreads;
            if (j < pts) rec[k] = unstage_record(stage, ihead + j * PCS_POINT_BYTES);
        }
        __syncthreads();                                     // everybody holds its records: the buffer may be overwritten
    } else {
        const uint32_t ds = C.ds;
#pragma unroll
        for (int k = 0; k < kPointsPerLane; k++) {
            const uint32_t j = threadIdx.x + (uint32_t)k * kBlockThreads;
            if (j < pts) {
                const uint16_t* s = reinterpret_cast<const uint16_t*>(C.in) + (size_t)(tile0 + j) * ds * PCS_POINT_SHORTS;
                rec[k].xy = (uint32_t)s[0] | ((uint32_t)s[1] << 16);
                rec[k].zc = (uint32_t)s[2] | ((uint32_t)s[3] << 16);
                rec[k].b = s[4];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kPointsPerLane; k++) {
        const uint32_t j = threadIdx.x + (uint32_t)k * kBlockThreads;
        if (j < pts) stage_record(stage, ohead + j * PCS_POINT_BYTES, retransform_record(C.M, rec[k]));
    }
    __syncthreads();
    store_staged(stage, ohead, pts * PCS_POINT_BYTES, gdst);
}

// ---- a7 with stride ----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_stitch_kernel(const uint16_t* __restrict__ src, uint32_t out_points, uint32_t ds, uint8_t* __restrict__ dst)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= out_points) return;
    const uint32_t pts = min(kTilePoints, out_points - tile0);
    uint8_t* gdst = dst + (size_t)tile0 * PCS_POINT_BYTES;
    const uint32_t head = (uint32_t)((uintptr_t)gdst & 15u);
    for (uint32_t j = threadIdx.x; j < pts; j += kBlockThreads) {
        const uint16_t* s = src + (size_t)(tile0 + j) * ds * PCS_POINT_SHORTS;
        uint16_t* o = reinterpret_cast<uint16_t*>(stage + head + j * PCS_POINT_BYTES);
#pragma unroll
        for (int k = 0; k < PCS_POINT_SHORTS; k++) o[k] = s[k];
    }
    __syncthreads();
    store_staged(stage, head, pts * PCS_POINT_BYTES, gdst);
}

// ---- a3: PCS_FLAG_SCALAR_ARITH ------------------------------------------------------------------
// The reference's default (no -m) arithmetic through the same tiles: ScalarArith in place of SimdArith (pcs_kernels_common.h). Kernels of
// their own, so that every -m kernel keeps its name and its code. One deprojection policy per kernel — the policies give identical
// bits: the certified general one (CertMath<false>) where every stream of the launch certifies, the IEEE one otherwise — over the
// DepthSource<true, true> that decides about distortion once per lane. The row-constant tile carries its own copy of the transform
// and is not selected. Under -c nothing is compacted (a3's loop, :640-646, leaves record i in slot i): the fused launches are the
// dense / emit launch with a per-point select to the zero record, no count, no scan.
template <class Mth, bool CUT>
__global__ __launch_bounds__(kBlockThreads, SCALAR_DENSE_WAVES)
void pcs_fused_dense_scalar_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp,
                                   uint8_t* __restrict__ payload_bytes)
{
    __shared__ uint4 stage[kDenseStageBytes / 16];
    const int s = blockIdx.y;
    const StreamParams& P = params[stream0 + s];
    request_constants(P, fp.depth[s], fp.color[s], payload_bytes);
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    DepthSource<true, true, Mth> src{fp.depth[s]};
    dense_tile<DepthSource<true, true, Mth>, kBlockThreads, ScalarArith<CUT>>(P, src, fp.color[s], tile0, n,
                                                                             payload_bytes + (size_t)P.out_base * PCS_POINT_BYTES, stage);
}

// The general form: any stride, any payload alignment, any raster width (generic_tile without a predicate: every point of a stream is
// in the sequence the stride runs over, a skipped one as its zero record).
template <bool DS1, class Mth, bool CUT>
__global__ __launch_bounds__(kBlockThreads, CUT ? SCALAR_EMIT_CUT_WAVES : EMIT_WAVES)
void pcs_fused_emit_scalar_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp, uint32_t ds,
                                  uint8_t* __restrict__ payload_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y;
    const StreamParams& P = params[stream0 + s];
    request_constants<true, Mth::kIdentR>(P, fp.depth[s], fp.color[s], payload_bytes);
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    DepthSource<true, true, Mth> src{fp.depth[s]};
    generic_tile<DepthSource<true, true, Mth>, false, DS1, ScalarArith<CUT>>(P, src, fp.color[s], tile0, n, 0u, ds, tile0, P.out_base,
                                                                             payload_bytes, stage, wsum);
}

// a2 twin, no -c: blockIdx.y = cloud (one for the single-cloud calls).
template <bool ALIGNED>
__global__ __launch_bounds__(kBlockThreads)
void pcs_pack_scalar_kernel(const StreamParams* __restrict__ params, PackBatch pb)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int e = blockIdx.y;
    const VertexPtrs vp = pb.v[e];
    const StreamParams& P = params[pb.stream[e]];
    const uint32_t n = vp.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    VertexSource src{vp.vertices, vp.texcoords};
    if (ALIGNED)
        dense_tile<VertexSource, kBlockThreads, ScalarArith<false>>(P, src, vp.color, tile0, n, pb.out[e], reinterpret_cast<uint4*>(stage));
    else
        generic_tile<VertexSource, false, true, ScalarArith<false>>(P, src, vp.color, tile0, n, 0u, 1u, tile0, 0u, pb.out[e], stage, wsum);
}

// a2 twin under -c: record i goes to slot i and a skipped slot keeps what the buffer held. The tile's own output bytes come into LDS
// first (lane-contiguous 16-byte loads, 2-byte ones at its ragged ends: never a byte of a neighbouring tile), the kept records are
// parked over them, and the whole range goes out again as 16-byte stores — a skipped slot is rewritten with its own bytes.
__global__ __launch_bounds__(kBlockThreads)
void pcs_pack_scalar_cut_kernel(const StreamParams* __restrict__ params, int stream, VertexPtrs vp, uint8_t* __restrict__ out_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const StreamParams& P = params[stream];
    const uint32_t n = vp.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    const uint32_t pts = min(kTilePoints, n - tile0);
    uint8_t* gdst = out_bytes + (size_t)tile0 * PCS_POINT_BYTES;
    const uint32_t head = (uint32_t)((uintptr_t)gdst & 15u);
    load_staged(stage, head, pts * PCS_POINT_BYTES, gdst);
    VertexSource src{vp.vertices, vp.texcoords};
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    PointIn p[8];
    src.load8(P, i0, n, p);
    Record rec[8];
    auto fill = [&](auto& cv) {
#pragma unroll
        for (int k = 0; k < 8; k++) rec[k] = make_record<ScalarArith<false>>(P, vp.color, p[k], cv);
    };
    FastCvt<true> fast;
    fill(fast);
    if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (i0 + k < n && scalar_cut_keeps(p[k].X, p[k].Z))
            stage_record(stage, head + (threadIdx.x * kPointsPerLane + k) * PCS_POINT_BYTES, rec[k]);
    __syncthreads();
    store_staged(stage, head, pts * PCS_POINT_BYTES, gdst);
}

// ---- crop box: pcs_set_crop_box_mm ------------------------------------------------------------------
// A world-frame box on the record's three shorts (CropBox, pcs_kernels_common.h), ANDed with whatever the context's flags gate. Kernels of
// their own, so that every other kernel keeps its name and its code. Always count + scan + emit (the scan kernels are the existing ones):
//   count  deprojects (the Z16-only shortcut of count_tiles cannot decide a world predicate), runs the three world_mm chains and the
//          conversion through world_ints — no colour arithmetic (dead without the gather), no gather, no store;
//   emit   generic_tile's order turned round: the records first (their colour gathers in flight), then the keep mask from them, then
//          the wave scan; the same two barriers.
// Both passes take a point's coordinates from world_ints under the same Cvt ladder: FastCvt<true> with its redo() into ExactCvt, the
// ladder of every policy the emit launch selects (crop_tile asserts it). The
// emit tile's redo is wider — a colour coordinate or the raster's last dword can send a lane through ExactCvt as well — but a lane
// redone for those alone converts world values below 2^31, where the two conversions agree in the low 16 bits the box reads (and
// NaN gives 0 / INT_MIN: the same 16 bits); a world value from 2^31 up sends the lane through ExactCvt in both passes.
__device__ __forceinline__ uint32_t crop_bits8(const StreamParams& P, const PointIn (&p)[8], const CropBox& box)
{
    auto bits = [&](auto& cv) {
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float f[3];
            uint32_t w[3];
            world_ints(P, p[k], cv, f, w);
            cv.note(f[0], f[1], f[2], 0.0f, 0.0f);
            m |= (uint32_t)box_keeps(box, perm(w[1], w[0], kLoLo), w[2]) << k;
        }
        return m;
    };
    FastCvt<true> fast;
    uint32_t m = bits(fast);
    if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; m = bits(exact); }
    return m;
}

__device__ __forceinline__ void crop_count_tile(const StreamParams& P, const uint16_t* __restrict__ dp, uint32_t flags, const CropBox& box,
                                                uint32_t* __restrict__ tile_counts, uint32_t* wsum)
{
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    DepthSource<true, false> src{dp};          // (X, Y, Z depend on the depth-side distortion alone; u, v are dead here)
    PointIn p[8];
    src.load8(P, i0, n, p);
    const uint32_t keep = keep_mask8(p, i0, n, flags) & crop_bits8(P, p, box);
    const uint32_t w = wave_sum(__popc(keep));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[P.tile_base + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_fused_count_crop_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp, uint32_t flags, CropBox box,
                                 uint32_t* __restrict__ tile_counts)
{
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y;
    crop_count_tile(params[stream0 + s], fp.depth[s], flags, box, tile_counts, wsum);
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_fused_count_crop_batch_kernel(const StreamParams* __restrict__ params, BatchPtrs bp, uint32_t flags, CropBox box,
                                       uint32_t* __restrict__ tile_counts, uint32_t total_tiles)
{
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y;
    crop_count_tile(params[s], bp.depth[blockIdx.z * gridDim.y + s], flags, box,
                              tile_counts + (size_t)blockIdx.z * total_tiles, wsum);
}

// make_record's -m form over world_ints: the record the boxed emit tile writes, its coordinates from the very function the count
// pass calls. (make_record itself is left as it is: routing it through world_ints moved the code of 53 existing kernels.)
template <class Cvt>
__device__ __forceinline__ Record make_record_box(const StreamParams& P, const uint8_t* __restrict__ color, const PointIn& p, Cvt& cv)
{
    float a[3], xf, yf;
    uint32_t q[3];
    world_ints(P, p, cv, a, q);
    color_coords(P, p.u, p.v, xf, yf);
    cv.note(a[0], a[1], a[2], xf, yf);
    const uint32_t w = color_fetch(P, color, cv.pixel(xf, P.cW - 1, P.c_wm1_f), cv.pixel(yf, P.cH - 1, P.c_hm1_f), cv);
    Record r;
    r.xy = perm(q[1], q[0], kLoLo);
    r.zc = perm(w, q[2], kLoLo);
    r.b  = __builtin_amdgcn_ubfe(w, 16, 8);
    return r;
}

// generic_tile with the box: PRED always, the keep mask after the records.
template <class Src, bool DS1>
__device__ __forceinline__ void crop_tile(const StreamParams& P, const Src& src, const uint8_t* __restrict__ color,
                                          uint32_t tile0, uint32_t n, uint32_t flags, const CropBox& box, uint32_t ds,
                                          uint32_t g0, uint32_t out_first, uint8_t* __restrict__ payload_bytes,
                                          uint8_t* stage, uint32_t* wsum)
{
    if (DS1) ds = 1u;
    const uint32_t i0 = tile0 + threadIdx.x * kPointsPerLane;
    PointIn p[8];
    src.load8(P, i0, n, p);
    uint32_t keep = keep_mask8(p, i0, n, flags);      // what the flags gate (the -c reversal included): the box bit is ANDed below

    Record rec[8];
    auto fill = [&](auto& cv) {
#pragma unroll
        for (int k = 0; k < 8; k++) rec[k] = make_record_box(P, color, p[k], cv);
    };
    static_assert(Src::Math::kCvtMode == 1, "the count pass (crop_bits8) runs this ladder and no other");
    FastCvt<true> fast;
    fill(fast);
    if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
    uint32_t in_box = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) in_box |= (uint32_t)box_keeps(box, rec[k].xy, rec[k].zc) << k;
    keep &= in_box;
    uint32_t wave_total;
    const uint32_t ex = wave_exclusive_scan(__popc(keep), wave_total);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += wsum[w];
    const uint32_t tile_kept = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const uint32_t lane_first = before + ex;

    const uint32_t q_lo = out_first + (DS1 ? g0 : (g0 + ds - 1) / ds);
    const uint32_t q_hi = out_first + (DS1 ? g0 + tile_kept : (g0 + tile_kept + ds - 1) / ds);
    uint8_t* gdst = payload_bytes + (size_t)q_lo * PCS_POINT_BYTES;
    const uint32_t head = (uint32_t)((uintptr_t)gdst & 15u);
    uint32_t g = g0 + lane_first;
    uint32_t gq = DS1 ? g : g / ds, gr = DS1 ? 0u : g - gq * ds;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if ((keep >> k) & 1u) {
            if (gr == 0u) stage_record(stage, head + (out_first + gq - q_lo) * PCS_POINT_BYTES, rec[k]);
            if (DS1) gq++;
            else if (++gr == ds) { gr = 0u; gq++; }
        }
    }
    __syncthreads();
    store_staged(stage, head, (q_hi - q_lo) * PCS_POINT_BYTES, gdst);
}

#ifndef CROP_EMIT_WAVES
#define CROP_EMIT_WAVES EMIT_WAVES    // DESIGN.md section 8 has the VGPR / scratch figures of every instantiation
#endif
template <bool DS1, class Mth>
__global__ __launch_bounds__(kBlockThreads, CROP_EMIT_WAVES)
void pcs_fused_emit_crop_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp, uint32_t flags, CropBox box,
                                uint32_t ds, const uint32_t* __restrict__ tile_prefix, const uint32_t* __restrict__ stream_kept,
                                uint8_t* __restrict__ payload_bytes, int32_t* __restrict__ total_out, int n_total_streams)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y;
    if (total_out && blockIdx.x == 0 && stream0 + s == 0 && threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int e = 0; e < n_total_streams; e++) tot += DS1 ? stream_kept[e] : (stream_kept[e] + ds - 1) / ds;
        *total_out = (int32_t)tot;
    }
    const StreamParams& P = params[stream0 + s];
    request_constants<true, Mth::kIdentR>(P, fp.depth[s], fp.color[s], payload_bytes);
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    DepthSource<true, true, Mth> src{fp.depth[s]};
    const uint32_t g0 = tile_prefix[P.tile_base + blockIdx.x];
    uint32_t out_first = 0;
    for (int e = 0; e < stream0 + s; e++) out_first += DS1 ? stream_kept[e] : (stream_kept[e] + ds - 1) / ds;
    crop_tile<DepthSource<true, true, Mth>, DS1>(P, src, fp.color[s], tile0, n, flags, box, ds, g0, out_first, payload_bytes, stage, wsum);
}

template <class Mth>
__global__ __launch_bounds__(kBlockThreads, CROP_EMIT_WAVES)
void pcs_fused_emit_crop_batch_kernel(const StreamParams* __restrict__ params, BatchPtrs bp, uint32_t flags, CropBox box,
                                      const uint32_t* __restrict__ tile_prefix, const uint32_t* __restrict__ stream_kept,
                                      uint32_t total_tiles, BatchCounts bc)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y, S = gridDim.y, z = blockIdx.z;
    const uint32_t* __restrict__ kept = stream_kept + z * S;
    if (blockIdx.x == 0 && s == 0 && threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int e = 0; e < S; e++) tot += kept[e];
        bc.counts[z][S] = (int32_t)tot;
    }
    const StreamParams& P = params[s];
    const uint32_t n = P.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    DepthSource<true, true, Mth> src{bp.depth[z * S + s]};
    const uint32_t g0 = tile_prefix[(size_t)z * total_tiles + P.tile_base + blockIdx.x];
    uint32_t out_first = 0;
    for (int e = 0; e < s; e++) out_first += kept[e];
    crop_tile<DepthSource<true, true, Mth>, true>(P, src, bp.color[z * S + s], tile0, n, flags, box, 1u, g0, out_first, bp.payload[z],
                                                  stage, wsum);
}

// ---- centre side: pcs_crop_payloads_device ----------------------------------------------------------
// The same box over payloads that are already packed (edge servers that cannot crop): count, the scan kernel above, emit. A tile is
// kTilePoints input records of one camera; its bytes come into LDS at the input's 16-byte phase (load_staged: never a byte outside
// the camera's payload), lane l takes records 8 l .. 8 l + 7 (ascending order per lane, as in generic_tile), and the kept ones are
// parked at the OUTPUT's phase and leave through store_staged. `tab` is a table of the scan kernel's type of which only n_points and
// tile_base are filled (pcs_crop_table_kernel): entry i = camera i.
struct CropCams { const int16_t* in[kLaunchStreams]; };
struct CropTable { uint32_t n_points[PCS_MAX_STREAMS]; uint32_t tile_base[PCS_MAX_STREAMS]; };

__global__ __launch_bounds__(64)
void pcs_crop_table_kernel(StreamParams* __restrict__ tab, CropTable t, int n)
{
    if ((int)threadIdx.x < n) { tab[threadIdx.x].n_points = t.n_points[threadIdx.x]; tab[threadIdx.x].tile_base = t.tile_base[threadIdx.x]; }
}

// unstage_record, as a copy of this section's own: with the re-transform kernel's function called from here as well, hipcc swapped the
// operands of eight adds in THAT kernel, and every existing kernel keeps its code byte for byte (tools/isa_compare.py).
__device__ __forceinline__ Record unstage_record_crop(const uint8_t* lds, uint32_t off)
{
    const bool odd = (off & 2u) != 0u;
    const uint32_t h_off = odd ? off : off + 8u;
    const uint32_t a_off = odd ? off + 2u : off;
    const uint32_t h = *reinterpret_cast<const uint16_t*>(lds + h_off);
    const uint32_t a = *reinterpret_cast<const uint32_t*>(lds + a_off);
    const uint32_t b = *reinterpret_cast<const uint32_t*>(lds + a_off + 4u);
    Record r;
    r.xy = odd ? perm(a, h, kLoLo) : a;
    r.zc = odd ? perm(b, a, kHiLo) : b;
    r.b = odd ? (b >> 16) : h;
    return r;
}
// The tile's records into registers; returns the lane's keep mask. (Ends behind a barrier: everybody holds its records.)
__device__ __forceinline__ uint32_t crop_load_tile(const int16_t* __restrict__ in, uint32_t tile0, uint32_t n, const CropBox& box,
                                                   uint8_t* stage, Record (&rec)[8])
{
    const uint32_t pts = min(kTilePoints, n - tile0);
    const uint8_t* gsrc = reinterpret_cast<const uint8_t*>(in) + (size_t)tile0 * PCS_POINT_BYTES;
    const uint32_t ihead = (uint32_t)((uintptr_t)gsrc & 15u);
    load_staged(stage, ihead, pts * PCS_POINT_BYTES, gsrc);
    __syncthreads();
    uint32_t keep = 0;
#pragma unroll
    for (int k = 0; k < kPointsPerLane; k++) {
        const uint32_t j = threadIdx.x * kPointsPerLane + (uint32_t)k;
        rec[k] = Record{0u, 0u, 0u};
        if (j < pts) {
            rec[k] = unstage_record_crop(stage, ihead + j * PCS_POINT_BYTES);
            keep |= (uint32_t)box_keeps(box, rec[k].xy, rec[k].zc) << k;
        }
    }
    __syncthreads();
    return keep;
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_crop_count_kernel(const StreamParams* __restrict__ tab, int cam0, CropCams cc, CropBox box, uint32_t* __restrict__ tile_counts)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const int s = blockIdx.y;
    const uint32_t n = tab[cam0 + s].n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    Record rec[8];
    const uint32_t keep = crop_load_tile(cc.in[s], tile0, n, box, stage, rec);
    const uint32_t w = wave_sum(__popc(keep));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[tab[cam0 + s].tile_base + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

template <bool DS1>
__global__ __launch_bounds__(kBlockThreads)
void pcs_crop_emit_kernel(const StreamParams* __restrict__ tab, int cam0, CropCams cc, CropBox box, uint32_t ds,
                          const uint32_t* __restrict__ tile_prefix, const uint32_t* __restrict__ cam_kept,
                          uint8_t* __restrict__ payload_bytes, int32_t* __restrict__ total_out, int n_cams)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    if (DS1) ds = 1u;
    const int s = blockIdx.y;
    if (blockIdx.x == 0 && cam0 + s == 0 && threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int e = 0; e < n_cams; e++) tot += (cam_kept[e] + ds - 1) / ds;
        *total_out = (int32_t)tot;
    }
    const uint32_t n = tab[cam0 + s].n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    Record rec[8];
    const uint32_t keep = crop_load_tile(cc.in[s], tile0, n, box, stage, rec);
    uint32_t wave_total;
    const uint32_t ex = wave_exclusive_scan(__popc(keep), wave_total);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += wsum[w];
    const uint32_t tile_kept = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const uint32_t g0 = tile_prefix[tab[cam0 + s].tile_base + blockIdx.x];
    uint32_t out_first = 0;
    for (int e = 0; e < cam0 + s; e++) out_first += (cam_kept[e] + ds - 1) / ds;

    const uint32_t q_lo = out_first + (g0 + ds - 1) / ds;
    const uint32_t q_hi = out_first + (g0 + tile_kept + ds - 1) / ds;
    uint8_t* gdst = payload_bytes + (size_t)q_lo * PCS_POINT_BYTES;
    const uint32_t head = (uint32_t)((uintptr_t)gdst & 15u);
    const uint32_t g = g0 + before + ex;
    uint32_t gq = g / ds, gr = g - gq * ds;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if ((keep >> k) & 1u) {
            if (gr == 0u) stage_record(stage, head + (out_first + gq - q_lo) * PCS_POINT_BYTES, rec[k]);
            if (++gr == ds) { gr = 0u; gq++; }
        }
    }
    __syncthreads();
    store_staged(stage, head, (q_hi - q_lo) * PCS_POINT_BYTES, gdst);
}

// Certificate of CertRowConst for one stream: row r's colour row through the IEEE chain for EVERY Z16 value 1 .. 65 535 (one workgroup
// per raster row). crow[r] = the row for d = 1; *bad counts the (row, depth) pairs that give another one. The chain is the product's
// own code (deproject_pixel + color_coords + the exact conversion), so the sweep cannot disagree with what the kernels would compute.
__global__ __launch_bounds__(256)
void pcs_certify_color_row_kernel(const StreamParams* __restrict__ params, int stream, int32_t* __restrict__ crow,
                                  unsigned long long* __restrict__ bad)
{
    const StreamParams& P = params[stream];
    const uint32_t r = blockIdx.x;
    if (r >= (uint32_t)P.H) return;
    const float my = as_global(P.my)[r];
    auto row_of = [&](uint32_t d) {
        const PointIn p = deproject_pixel<false, false, IeeeMath>(P, d, 0.0f, my);
        float xf, yf;
        color_coords(P, p.u, p.v, xf, yf);
        ExactCvt ex;
        return ex.pixel(yf, P.cH - 1, P.c_hm1_f);
    };
    const int32_t want = row_of(1u);
    uint32_t local = 0;
    for (uint32_t d = 1u + threadIdx.x; d < 65536u; d += 256u) local += row_of(d) != want;
    if (local) atomicAdd(bad, (unsigned long long)local);
    if (threadIdx.x == 0) crow[r] = want;
}


// Device-side certificate for CertMath::div_const: over ALL 2^32 numerators a, the pixel coordinate that
// the pack derives from a quotient by the raster dimension c — clamp(cvttss2si(fma(a/c, c, 0.5)), 0, c-1)
// — is the same with Markstein's quotient as with the IEEE one. Run once per distinct dimension when a
// context is created (about a millisecond); any difference disables CertMath for that stream.
__global__ __launch_bounds__(256)
void pcs_verify_div_const_kernel(float c, float rc, int32_t dim, unsigned long long* __restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t local = 0;
    for (uint64_t bits = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; bits < (1ull << 32); bits += stride) {
        const float a = __uint_as_float((uint32_t)bits);
        const float f1 = __fmaf_rn(IeeeMath::div_const(a, c, rc), c, 0.5f);
        const float f2 = __fmaf_rn(CertMath<false>::div_const(a, c, rc), c, 0.5f);
        const int32_t i1 = min(max(cvtt_x86(f1), 0), dim - 1);
        const int32_t i2 = min(max(cvtt_x86(f2), 0), dim - 1);
        // the lazy convert must also agree whenever it is the one used (f2 < 2^31 or NaN)
        const int32_t i3 = (f2 >= 2147483648.0f) ? i2 : min(max(cvt_sat(f2), 0), dim - 1);
        local += (i1 != i2) | (i2 != i3);
    }
    if (local) atomicAdd(bad, (unsigned long long)local);
}


// The small-launch shape of the dense kernels (dense_tile<Src, 64>: one wavefront per 512-point tile) — an A/B knob, NOT taken by
// default. One 1280 x 720 stream is 450 workgroups of 2048 points on a chip that holds 1 792; four times as many one-wavefront
// workgroups were measured on it (round 6, rocprofv3 average over 3 000 cold launches): fused 6.95 -> 7.44 us, two streams 8.54 ->
// 8.30 us, the a2 twin 7.28 -> 7.77 us; hipEvent period of back-to-back launches 6.09 -> 6.22 us. The lone launch is a chain of
// dependent round trips (constants, Z16 + LUT, the colour gather, the store drain: ~5 us before the first stream's bytes count,
// ~2.3 us per further stream), which the tile size does not shorten. PCS_SMALL_TILES=1 forces it (the parity suite runs under it).
constexpr uint32_t kSmallThreads = 64, kSmallTilePoints = kSmallThreads * kPointsPerLane;
inline bool small_launch(uint32_t, int)
{
    const char* v = getenv("PCS_SMALL_TILES");      // (read at every call: bench.py times both shapes in one process)
    return v && v[0] == '1';
}

inline dim3 tile_grid(uint32_t max_points, int n_launch)
{
    return dim3((max_points + kTilePoints - 1) / kTilePoints, (unsigned)n_launch, 1);
}

// A launcher's ladder from run-time choices to a template instantiation: the choice arrives at a generic lambda as a tag value
// (decltype(tag)::value / ::type), and only the combinations a ladder names are instantiated.
template <class M> struct MathTag { using type = M; };
constexpr std::true_type  kYes{};
constexpr std::false_type kNo{};

template <class F> void with_flag(bool b, F&& f) { if (b) f(kYes); else f(kNo); }

// <DDIST, CDIST, Math> of the dense kernels (launch_fused_dense, launch_fused_dense_batch). CertRowConstNoOvf: after dense_row_const.
template <class F>
void with_dense_form(MathSel math, bool any_ddist, bool any_cdist, F&& f)
{
    if (math == MathSel::CertRowConstNoOvf) { f(kNo, kNo, MathTag<CertRowConstNoOvf>{}); return; }
    if (math != MathSel::Ieee && !any_ddist) {
        const bool ident = (math == MathSel::CertIdentR || math == MathSel::CertIdentRNoOvf);
        const bool noovf = (math == MathSel::CertNoOvf || math == MathSel::CertIdentRNoOvf) && !any_cdist;
        if (noovf)      { if (ident) f(kNo, kNo, MathTag<CertIdentNoOvf>{}); else f(kNo, kNo, MathTag<CertNoOvf>{}); }
        else if (ident) { if (any_cdist) f(kNo, kYes, MathTag<CertMath<true>>{}); else f(kNo, kNo, MathTag<CertMath<true>>{}); }
        else            { if (any_cdist) f(kNo, kYes, MathTag<CertMath<false>>{}); else f(kNo, kNo, MathTag<CertMath<false>>{}); }
    } else {
        if (any_ddist) { if (any_cdist) f(kYes, kYes, MathTag<IeeeMath>{}); else f(kYes, kNo, MathTag<IeeeMath>{}); }
        else           { if (any_cdist) f(kNo, kYes, MathTag<IeeeMath>{}); else f(kNo, kNo, MathTag<IeeeMath>{}); }
    }
}

// The row-constant tile requests its colour window in 16-byte pieces and pixel (0, 0)'s word by a scalar load, a lane's Z16 quad by one
// 16-byte load (DepthSource::fast): 16-aligned rasters only, every one of the launch's n; otherwise CertIdentNoOvf's kernel.
inline MathSel dense_row_const(MathSel math, bool any_ddist, bool any_cdist, const uint16_t* const* depth, const uint8_t* const* color, int n)
{
    if (math != MathSel::CertRowConstNoOvf) return math;
    bool aligned = !any_ddist && !any_cdist;
    for (int k = 0; k < n; k++) aligned &= ((((uintptr_t)color[k]) | ((uintptr_t)depth[k])) & 15u) == 0;
    return aligned ? math : MathSel::CertIdentRNoOvf;
}

// Math of the emit kernels (the single-set and the K-set ones, with and without a crop box): they have no no-overflow forms.
template <class F>
void with_emit_math(MathSel math, F&& f)
{
    const bool ident = (math == MathSel::CertIdentR || math == MathSel::CertIdentRNoOvf);
    if (math == MathSel::Ieee) f(MathTag<IeeeMath>{}); else if (ident) f(MathTag<CertMath<true>>{}); else f(MathTag<CertMath<false>>{});
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------------

hipError_t launch_fused_dense(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                              bool any_ddist, bool any_cdist, MathSel math, const FramePtrs& fp, int16_t* d_payload,
                              hipStream_t st)
{
    if (n_launch <= 0 || max_points == 0) return hipSuccess;
    // (PCS_SMALL_TILES=1: one wavefront per 512-point tile — measured no faster on the launches it was meant for, see small_launch)
    const bool small = small_launch(max_points, n_launch);
    const dim3 grid = small ? dim3((max_points + kSmallTilePoints - 1) / kSmallTilePoints, (unsigned)n_launch, 1) : tile_grid(max_points, n_launch);
    math = dense_row_const(math, any_ddist, any_cdist, fp.depth, fp.color, n_launch);
    uint8_t* out = reinterpret_cast<uint8_t*>(d_payload);
    with_dense_form(math, any_ddist, any_cdist, [&](auto dd, auto cd, auto m) {
        constexpr bool DD = decltype(dd)::value, CD = decltype(cd)::value;
        using M = typename decltype(m)::type;
        if (small) hipLaunchKernelGGL((pcs_fused_dense_kernel<DD, CD, M, kSmallThreads>), grid, dim3(kSmallThreads), 0, st, d_params, stream0, fp, out);
        else       hipLaunchKernelGGL((pcs_fused_dense_kernel<DD, CD, M>), grid, dim3(kBlockThreads), 0, st, d_params, stream0, fp, out);
    });
    return hipGetLastError();
}

hipError_t launch_fused_count(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                              uint32_t flags, const FramePtrs& fp, uint32_t* d_tile_counts, hipStream_t st)
{
    if (n_launch <= 0 || max_points == 0) return hipSuccess;
    const uint32_t tiles = (max_points + kTilePoints - 1) / kTilePoints;
    const dim3 grid((tiles + kCountTiles - 1) / kCountTiles, (unsigned)n_launch, 1);
    // the predicate depends on depth-side distortion only through x; always run the general form
    hipLaunchKernelGGL((pcs_fused_count_kernel<true, false>), grid, dim3(kBlockThreads), 0, st,
                       d_params, stream0, fp, flags, d_tile_counts);
    return hipGetLastError();
}

hipError_t launch_scan(const StreamParams* d_params, int n_streams, int downsample,
                       const uint32_t* d_tile_counts, uint32_t* d_tile_prefix, uint32_t* d_stream_kept,
                       int32_t* d_counts, uint32_t* d_arrive, hipStream_t st)
{
    hipLaunchKernelGGL(pcs_scan_kernel, dim3((unsigned)n_streams), dim3(1024), 0, st, d_params, 0, n_streams, 0u,
                       (uint32_t)downsample, d_tile_counts, d_tile_prefix, d_stream_kept, d_counts, d_arrive);
    return hipGetLastError();
}

hipError_t launch_fused_emit(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                             uint32_t flags, int downsample, MathSel math, const FramePtrs& fp,
                             const uint32_t* d_tile_prefix, const uint32_t* d_stream_kept,
                             int16_t* d_payload, int32_t* d_total_out, int n_total_streams, hipStream_t st)
{
    if (n_launch <= 0 || max_points == 0) return hipSuccess;
    const dim3 grid = tile_grid(max_points, n_launch);
    const bool pred = (flags & (PCS_FLAG_CUTOFF | PCS_FLAG_DROP_INVALID)) != 0;
    const bool ds1 = downsample == 1;
    uint8_t* out = reinterpret_cast<uint8_t*>(d_payload);
    with_emit_math(math, [&](auto m) { with_flag(pred, [&](auto pr) { with_flag(ds1, [&](auto d1) {
        hipLaunchKernelGGL((pcs_fused_emit_kernel<decltype(pr)::value, decltype(d1)::value, typename decltype(m)::type>), grid, dim3(kBlockThreads),
                           0, st, d_params, stream0, fp, flags, (uint32_t)downsample, d_tile_prefix, d_stream_kept, out, d_total_out, n_total_streams);
    }); }); });
    return hipGetLastError();
}

hipError_t launch_fused_compact(const StreamParams* d_params, int stream0, int n_launch, uint32_t launch_tiles,
                                MathSel math, const FramePtrs& fp, const CompactLaunch& cl, int16_t* d_payload,
                                hipStream_t st)
{
    if (n_launch <= 0 || launch_tiles == 0) return hipSuccess;
    CompactArgs a;
    a.ticket = cl.d_ticket; a.ticket_base = cl.ticket_base; a.desc = cl.d_desc; a.stream_desc = cl.d_stream_desc;
    a.stream_end = cl.d_stream_end;
    a.chain_in = cl.d_chain_in; a.error = cl.d_error; a.gen = cl.gen & 0x3FFFFFFFu; a.flags = cl.flags;
    a.counts = cl.d_counts; a.n_total = cl.n_total; a.last_launch = cl.last_launch;
    uint8_t* out = reinterpret_cast<uint8_t*>(d_payload);
    if (math != MathSel::Ieee)
        hipLaunchKernelGGL((pcs_fused_compact_kernel<CertMath<false>>), dim3(launch_tiles), dim3(kBlockThreads), 0, st,
                           d_params, stream0, n_launch, fp, a, out);
    else
        hipLaunchKernelGGL((pcs_fused_compact_kernel<IeeeMath>), dim3(launch_tiles), dim3(kBlockThreads), 0, st,
                           d_params, stream0, n_launch, fp, a, out);
    return hipGetLastError();
}

hipError_t launch_fused_dense_batch(const StreamParams* d_params, int n_streams, int n_sets, uint32_t max_points,
                                    bool any_ddist, bool any_cdist, MathSel math, const BatchPtrs& bp, hipStream_t st)
{
    if (n_streams <= 0 || n_sets <= 0 || max_points == 0) return hipSuccess;
    if (n_streams * n_sets > kBatchEntries || n_sets > kBatchSets) return hipErrorInvalidValue;
    const dim3 grid((max_points + kTilePoints - 1) / kTilePoints, (unsigned)n_streams, (unsigned)n_sets);
    math = dense_row_const(math, any_ddist, any_cdist, bp.depth, bp.color, n_streams * n_sets);      // (every set's rasters)
    with_dense_form(math, any_ddist, any_cdist, [&](auto dd, auto cd, auto m) {
        hipLaunchKernelGGL((pcs_fused_dense_batch_kernel<decltype(dd)::value, decltype(cd)::value, typename decltype(m)::type>), grid,
                           dim3(kBlockThreads), 0, st, d_params, bp);
    });
    return hipGetLastError();
}

hipError_t launch_compact_batch(const StreamParams* d_params, int n_streams, int n_sets, uint32_t max_points,
                                uint32_t total_tiles, uint32_t flags, MathSel math, const BatchPtrs& bp,
                                const BatchCounts& bc, uint32_t* d_tile_counts, uint32_t* d_tile_prefix,
                                uint32_t* d_stream_kept, hipStream_t st)
{
    if (n_streams <= 0 || n_sets <= 0 || max_points == 0) return hipSuccess;
    if (n_streams * n_sets > kBatchEntries || n_sets > kBatchSets) return hipErrorInvalidValue;
    const uint32_t tiles = (max_points + kTilePoints - 1) / kTilePoints;
    hipLaunchKernelGGL((pcs_fused_count_batch_kernel<true, false>),
                       dim3((tiles + kCountTiles - 1) / kCountTiles, (unsigned)n_streams, (unsigned)n_sets),
                       dim3(kBlockThreads), 0, st, d_params, bp, flags, d_tile_counts, total_tiles);
    hipLaunchKernelGGL(pcs_scan_batch_kernel, dim3((unsigned)n_streams, (unsigned)n_sets), dim3(1024), 0, st, d_params,
                       d_tile_counts, d_tile_prefix, d_stream_kept, total_tiles, bc);
    const dim3 grid(tiles, (unsigned)n_streams, (unsigned)n_sets);
    with_emit_math(math, [&](auto m) {
        hipLaunchKernelGGL((pcs_fused_emit_batch_kernel<typename decltype(m)::type>), grid, dim3(kBlockThreads), 0, st, d_params, bp, flags,
                           d_tile_prefix, d_stream_kept, total_tiles, bc);
    });
    return hipGetLastError();
}

hipError_t launch_pack_batch(const StreamParams* d_params, const PackBatch& pb, int n, uint32_t max_points, bool aligned,
                             hipStream_t st)
{
    if (n <= 0 || max_points == 0) return hipSuccess;
    if (n > kPackBatch) return hipErrorInvalidValue;
    const dim3 grid = tile_grid(max_points, n);
    if (aligned) hipLaunchKernelGGL((pcs_pack_batch_kernel<true>), grid, dim3(kBlockThreads), 0, st, d_params, pb);
    else         hipLaunchKernelGGL((pcs_pack_batch_kernel<false>), grid, dim3(kBlockThreads), 0, st, d_params, pb);
    return hipGetLastError();
}

hipError_t launch_certify_color_row(const StreamParams* d_params, int stream, int rows, int32_t* d_crow, unsigned long long* d_bad, hipStream_t st)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(pcs_certify_color_row_kernel, dim3((unsigned)rows), dim3(256), 0, st, d_params, stream, d_crow, d_bad);
    return hipGetLastError();
}

hipError_t launch_verify_div_const(float c, float rc, int32_t dim, unsigned long long* d_bad, hipStream_t st)
{
    hipLaunchKernelGGL(pcs_verify_div_const_kernel, dim3(8192), dim3(256), 0, st, c, rc, dim, d_bad);
    return hipGetLastError();
}

hipError_t launch_pack_dense(const StreamParams* d_params, int stream, const VertexPtrs& vp,
                             int16_t* d_out, hipStream_t st)
{
    if (vp.n_points == 0) return hipSuccess;
    if (small_launch(vp.n_points, 1))       // (A/B knob only)
        hipLaunchKernelGGL((pcs_pack_dense_kernel<kSmallThreads>), dim3((vp.n_points + kSmallTilePoints - 1) / kSmallTilePoints),
                           dim3(kSmallThreads), 0, st, d_params, stream, vp, reinterpret_cast<uint8_t*>(d_out));
    else
        hipLaunchKernelGGL((pcs_pack_dense_kernel<kBlockThreads>), tile_grid(vp.n_points, 1), dim3(kBlockThreads), 0, st,
                           d_params, stream, vp, reinterpret_cast<uint8_t*>(d_out));
    return hipGetLastError();
}

hipError_t launch_pack_count(const StreamParams* d_params, int stream, const VertexPtrs& vp, uint32_t flags,
                             uint32_t* d_tile_counts, hipStream_t st)
{
    if (vp.n_points == 0) return hipSuccess;
    hipLaunchKernelGGL(pcs_pack_count_kernel, tile_grid(vp.n_points, 1), dim3(kBlockThreads), 0, st,
                       d_params, stream, vp, flags, d_tile_counts);
    return hipGetLastError();
}

hipError_t launch_pack_scan(uint32_t n_tiles, const uint32_t* d_tile_counts, uint32_t* d_tile_prefix,
                            int32_t* d_out_points, uint32_t* d_arrive, hipStream_t st)
{
    // override_n makes the scan kernel ignore the params table (one segment of n_tiles tiles at index 0);
    // counts[0] = kept, counts[1] = total — d_out_points must hold 2 ints.
    hipLaunchKernelGGL(pcs_scan_kernel, dim3(1), dim3(1024), 0, st, (const StreamParams*)nullptr, 0, 1,
                       n_tiles * kTilePoints, 1u, d_tile_counts, d_tile_prefix, (uint32_t*)nullptr, d_out_points, d_arrive);
    return hipGetLastError();
}

hipError_t launch_pack_emit(const StreamParams* d_params, int stream, const VertexPtrs& vp, uint32_t flags,
                            const uint32_t* d_tile_prefix, int16_t* d_out, hipStream_t st)
{
    if (vp.n_points == 0) return hipSuccess;
    const bool pred = (flags & (PCS_FLAG_CUTOFF | PCS_FLAG_DROP_INVALID)) != 0;
    uint8_t* out = reinterpret_cast<uint8_t*>(d_out);
    if (pred)
        hipLaunchKernelGGL((pcs_pack_emit_kernel<true>), tile_grid(vp.n_points, 1), dim3(kBlockThreads), 0, st,
                           d_params, stream, vp, flags, d_tile_prefix, out);
    else
        hipLaunchKernelGGL((pcs_pack_emit_kernel<false>), tile_grid(vp.n_points, 1), dim3(kBlockThreads), 0, st,
                           d_params, stream, vp, flags, d_tile_prefix, out);
    return hipGetLastError();
}

// ---- a3: PCS_FLAG_SCALAR_ARITH ----
hipError_t launch_fused_scalar(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points, bool dense, bool cut,
                               int downsample, MathSel math, const FramePtrs& fp, int16_t* d_payload, hipStream_t st)
{
    if (n_launch <= 0 || max_points == 0) return hipSuccess;
    const dim3 grid = tile_grid(max_points, n_launch);
    uint8_t* out = reinterpret_cast<uint8_t*>(d_payload);
    const bool ieee = math == MathSel::Ieee;
#define LD(M, C) hipLaunchKernelGGL((pcs_fused_dense_scalar_kernel<M, C>), grid, dim3(kBlockThreads), 0, st, d_params, stream0, fp, out)
#define LE(D1, M, C) hipLaunchKernelGGL((pcs_fused_emit_scalar_kernel<D1, M, C>), grid, dim3(kBlockThreads), 0, st, d_params, stream0, fp, \
                                        (uint32_t)downsample, out)
#define LEM(M, C) do { if (downsample == 1) LE(true, M, C); else LE(false, M, C); } while (0)
    if (dense) {
        if (ieee) { if (cut) LD(IeeeMath, true); else LD(IeeeMath, false); }
        else      { if (cut) LD(CertMath<false>, true); else LD(CertMath<false>, false); }
    } else {
        if (ieee) { if (cut) LEM(IeeeMath, true); else LEM(IeeeMath, false); }
        else      { if (cut) LEM(CertMath<false>, true); else LEM(CertMath<false>, false); }
    }
#undef LEM
#undef LE
#undef LD
    return hipGetLastError();
}

hipError_t launch_pack_scalar(const StreamParams* d_params, const PackBatch& pb, int n, uint32_t max_points, bool aligned,
                              hipStream_t st)
{
    if (n <= 0 || max_points == 0) return hipSuccess;
    if (n > kPackBatch) return hipErrorInvalidValue;
    const dim3 grid = tile_grid(max_points, n);
    if (aligned) hipLaunchKernelGGL((pcs_pack_scalar_kernel<true>), grid, dim3(kBlockThreads), 0, st, d_params, pb);
    else         hipLaunchKernelGGL((pcs_pack_scalar_kernel<false>), grid, dim3(kBlockThreads), 0, st, d_params, pb);
    return hipGetLastError();
}

hipError_t launch_pack_scalar_cut(const StreamParams* d_params, int stream, const VertexPtrs& vp, int16_t* d_out, hipStream_t st)
{
    if (vp.n_points == 0) return hipSuccess;
    hipLaunchKernelGGL(pcs_pack_scalar_cut_kernel, tile_grid(vp.n_points, 1), dim3(kBlockThreads), 0, st, d_params, stream, vp,
                       reinterpret_cast<uint8_t*>(d_out));
    return hipGetLastError();
}

hipError_t launch_deproject(const StreamParams* d_params, int stream, uint32_t n_points,
                            const uint16_t* d_depth, float* d_vertices, float* d_texcoords, hipStream_t st)
{
    if (n_points == 0) return hipSuccess;
    const dim3 grid((n_points + kBlockThreads - 1) / kBlockThreads);
    hipLaunchKernelGGL((pcs_deproject_kernel<true, true>), grid, dim3(kBlockThreads), 0, st,
                       d_params, stream, d_depth, d_vertices, d_texcoords);
    return hipGetLastError();
}

hipError_t launch_transform_payloads(const XformBatch& xb, int n, uint32_t max_out, hipStream_t st)
{
    if (n <= 0 || max_out == 0) return hipSuccess;
    if (n > kXformBatch) return hipErrorInvalidValue;
    bool ds1 = true;
    for (int i = 0; i < n; i++) ds1 = ds1 && xb.c[i].ds == 1u;
    const dim3 grid = tile_grid(max_out, n);
    if (ds1) hipLaunchKernelGGL((pcs_transform_payload_kernel<true>), grid, dim3(kBlockThreads), 0, st, xb);
    else     hipLaunchKernelGGL((pcs_transform_payload_kernel<false>), grid, dim3(kBlockThreads), 0, st, xb);
    return hipGetLastError();
}

hipError_t launch_stitch(const int16_t* d_src, uint32_t src_points, int downsample,
                         int16_t* d_dst, hipStream_t st)
{
    const uint32_t ds = downsample < 1 ? 1u : (uint32_t)downsample;
    const uint32_t out_points = (src_points + ds - 1) / ds;
    if (out_points == 0) return hipSuccess;
    hipLaunchKernelGGL(pcs_stitch_kernel, tile_grid(out_points, 1), dim3(kBlockThreads), 0, st,
                       reinterpret_cast<const uint16_t*>(d_src), out_points, ds, reinterpret_cast<uint8_t*>(d_dst));
    return hipGetLastError();
}

// ---- crop box ----
namespace {
inline CropBox crop_box(const CropBoxArg& b) { return CropBox{b.w[0], b.w[1], b.w[2]}; }
}  // namespace

hipError_t launch_fused_count_crop(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points, uint32_t flags,
                                   const CropBoxArg& box, const FramePtrs& fp, uint32_t* d_tile_counts, hipStream_t st)
{
    if (n_launch <= 0 || max_points == 0) return hipSuccess;
    hipLaunchKernelGGL(pcs_fused_count_crop_kernel, tile_grid(max_points, n_launch), dim3(kBlockThreads), 0, st, d_params, stream0, fp,
                       flags, crop_box(box), d_tile_counts);
    return hipGetLastError();
}

hipError_t launch_fused_emit_crop(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points, uint32_t flags,
                                  const CropBoxArg& box, int downsample, MathSel math, const FramePtrs& fp, const uint32_t* d_tile_prefix,
                                  const uint32_t* d_stream_kept, int16_t* d_payload, int32_t* d_total_out, int n_total_streams,
                                  hipStream_t st)
{
    if (n_launch <= 0 || max_points == 0) return hipSuccess;
    const dim3 grid = tile_grid(max_points, n_launch);
    uint8_t* out = reinterpret_cast<uint8_t*>(d_payload);
    with_emit_math(math, [&](auto m) { with_flag(downsample == 1, [&](auto d1) {
        hipLaunchKernelGGL((pcs_fused_emit_crop_kernel<decltype(d1)::value, typename decltype(m)::type>), grid, dim3(kBlockThreads), 0, st, d_params,
                           stream0, fp, flags, crop_box(box), (uint32_t)downsample, d_tile_prefix, d_stream_kept, out, d_total_out, n_total_streams);
    }); });
    return hipGetLastError();
}

hipError_t launch_crop_batch(const StreamParams* d_params, int n_streams, int n_sets, uint32_t max_points, uint32_t total_tiles,
                             uint32_t flags, const CropBoxArg& box, MathSel math, const BatchPtrs& bp, const BatchCounts& bc,
                             uint32_t* d_tile_counts, uint32_t* d_tile_prefix, uint32_t* d_stream_kept, hipStream_t st)
{
    if (n_streams <= 0 || n_sets <= 0 || max_points == 0) return hipSuccess;
    if (n_streams * n_sets > kBatchEntries || n_sets > kBatchSets) return hipErrorInvalidValue;
    const uint32_t tiles = (max_points + kTilePoints - 1) / kTilePoints;
    const dim3 grid(tiles, (unsigned)n_streams, (unsigned)n_sets);
    hipLaunchKernelGGL(pcs_fused_count_crop_batch_kernel, grid, dim3(kBlockThreads), 0, st, d_params, bp, flags, crop_box(box),
                       d_tile_counts, total_tiles);
    hipLaunchKernelGGL(pcs_scan_batch_kernel, dim3((unsigned)n_streams, (unsigned)n_sets), dim3(1024), 0, st, d_params,
                       d_tile_counts, d_tile_prefix, d_stream_kept, total_tiles, bc);
    with_emit_math(math, [&](auto m) {
        hipLaunchKernelGGL((pcs_fused_emit_crop_batch_kernel<typename decltype(m)::type>), grid, dim3(kBlockThreads), 0, st, d_params, bp, flags,
                           crop_box(box), d_tile_prefix, d_stream_kept, total_tiles, bc);
    });
    return hipGetLastError();
}

hipError_t launch_crop_payloads(StreamParams* d_tab, const int16_t* const* d_in, const uint32_t* n_points, int n_cams,
                                const CropBoxArg& box, int downsample, uint32_t* d_tile_counts, uint32_t* d_tile_prefix,
                                uint32_t* d_cam_kept, int16_t* d_out, int32_t* d_counts, hipStream_t st)
{
    if (n_cams <= 0 || n_cams > PCS_MAX_STREAMS) return hipErrorInvalidValue;
    CropTable t{};
    uint32_t tb = 0;
    for (int i = 0; i < n_cams; i++) { t.n_points[i] = n_points[i]; t.tile_base[i] = tb; tb += (n_points[i] + kTilePoints - 1) / kTilePoints; }
    hipLaunchKernelGGL(pcs_crop_table_kernel, dim3(1), dim3(64), 0, st, d_tab, t, n_cams);
    for (int c0 = 0; c0 < n_cams; c0 += kLaunchStreams) {
        const int nl = std::min(kLaunchStreams, n_cams - c0);
        CropCams cc{};
        uint32_t mp = 0;
        for (int k = 0; k < nl; k++) { cc.in[k] = d_in[c0 + k]; mp = std::max(mp, n_points[c0 + k]); }
        if (mp) hipLaunchKernelGGL(pcs_crop_count_kernel, tile_grid(mp, nl), dim3(kBlockThreads), 0, st, d_tab, c0, cc, crop_box(box), d_tile_counts);
    }
    hipLaunchKernelGGL(pcs_scan_kernel, dim3((unsigned)n_cams), dim3(1024), 0, st, d_tab, 0, n_cams, 0u, (uint32_t)downsample,
                       d_tile_counts, d_tile_prefix, d_cam_kept, d_counts, (uint32_t*)nullptr);
    // the grand total rides on the first workgroup of camera 0's launch
    for (int c0 = 0; c0 < n_cams; c0 += kLaunchStreams) {
        const int nl = std::min(kLaunchStreams, n_cams - c0);
        CropCams cc{};
        uint32_t mp = 0;
        for (int k = 0; k < nl; k++) { cc.in[k] = d_in[c0 + k]; mp = std::max(mp, n_points[c0 + k]); }
        if (c0 == 0 && mp == 0) mp = 1;         // (one workgroup per camera that writes the total and returns)
        if (!mp) continue;
        if (downsample == 1)
            hipLaunchKernelGGL((pcs_crop_emit_kernel<true>), tile_grid(mp, nl), dim3(kBlockThreads), 0, st, d_tab, c0, cc, crop_box(box), 1u,
                               d_tile_prefix, d_cam_kept, reinterpret_cast<uint8_t*>(d_out), d_counts + n_cams, n_cams);
        else
            hipLaunchKernelGGL((pcs_crop_emit_kernel<false>), tile_grid(mp, nl), dim3(kBlockThreads), 0, st, d_tab, c0, cc, crop_box(box),
                               (uint32_t)downsample, d_tile_prefix, d_cam_kept, reinterpret_cast<uint8_t*>(d_out), d_counts + n_cams, n_cams);
    }
    return hipGetLastError();
}


}  // namespace pcs
