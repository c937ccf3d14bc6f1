// pcs_kernels_common.h — what both kernel translation units use, pcs_kernels.hip (the stitch / pack kernels) and pcs_kernels_voxel.hip
// (the raster / payload voxel readers): conversion and arithmetic policies, per-pixel deprojection, colour lookup, rigid transform, keep
// mask, wave scans, the depth source, the batched request of a stream's constants. Included by those two, never compiled alone. A
// definition belongs here only if both use it (the policy families stay whole); everything else lives in the file that does.
//
// Bit-exactness: compiled with -ffp-contract=off; every fused op is an explicit __fmaf_rn and every
// other product/sum/quotient is individually rounded (IEEE divide), mirroring oracle/pcs_oracle_impl.h.
// Float->int follows x86 cvttss2si including its "integer indefinite" result for NaN / out of range,
// which v_cvt_i32_f32 (saturating) does not give by itself.
#pragma once

#include <cstddef>

#include "pcs_device.h"

namespace pcs {

namespace {

// Pointers that reach a kernel through memory (the StreamParams table) have no address space the
// compiler can see and would be accessed with flat_load; they are always HBM, so say so.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <class T> using gptr = const __attribute__((address_space(1))) T*;
template <class T> __device__ __forceinline__ gptr<T> as_global(const T* p)
{
    return (gptr<T>)(uintptr_t)p;
}

struct PointIn {
    float X, Y, Z;   // camera-frame vertex (rs2::vertex)
    float u, v;      // texture coordinate  (rs2::texture_coordinate)
};

// cvttss2si / _mm_cvttps_epi32: truncate; NaN or |f| >= 2^31 -> 0x80000000.
__device__ __forceinline__ int32_t cvtt_x86(float f)
{
    return (__builtin_fabsf(f) < 2147483648.0f) ? (int32_t)f : (int32_t)0x80000000;
}

// v_cvt_i32_f32 as the hardware does it: truncate, saturate, NaN -> 0.
__device__ __forceinline__ int32_t cvt_sat(float f)
{
    int32_t i;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(i) : "v"(f));
    return i;
}

// Float->int conversion policies. The five conversions of a point (world x,y,z; colour column,row) are
// consumed only as `& 0xFFFF` or as clamp(., 0, dim-1). Under those two uses the saturating hardware
// convert differs from cvttss2si in exactly one case: f >= 2^31 (hardware INT_MAX, x86 INT_MIN); NaN
// gives 0 vs INT_MIN, which agree both in the low 16 bits and after the clamp. FastCvt therefore uses
// the 1-instruction hardware convert and keeps a running maximum of everything it converted (v_max3
// ignores NaN); the tile code re-does a lane's points with ExactCvt in the (practically never taken)
// case that the maximum reached 2^31.
struct ExactCvt {
    [[maybe_unused]] static constexpr bool kTracks = false;              // (no running maximum: make_record's a3 branch then converts exactly)
    [[maybe_unused]] static constexpr bool kCoordsInShort = false;       // a converted coordinate may lie outside int16: the record keeps its low 16 bits
    __device__ __forceinline__ void note(float, float, float, float, float) {}
    __device__ __forceinline__ int32_t cvt(float f) const { return cvtt_x86(f); }
    // colour column / row: clamp(cvttss2si(f), 0, dim-1)   (:438-444)
    __device__ __forceinline__ int32_t pixel(float f, int32_t dim_m1, float) const
    {
        return min(max(cvtt_x86(f), 0), dim_m1);
    }
    // One dword covers R,G,B. Never read past the raster: slide the window back at the very end of it and
    // shift the wanted bytes down.
    __device__ __forceinline__ uint32_t window(uint32_t idx, uint32_t lim, uint32_t& shift)
    {
        const uint32_t off = min(idx, lim);
        shift = (idx - off) * 8u;
        return off;
    }
    __device__ __forceinline__ bool redo() const { return false; }
};

// TRACK = false is for streams whose certificate also proves that no converted value can reach 2^31
// (pcs_capi.cpp: certify_no_overflow): then the running maximum is not needed at all.
template <bool TRACK>
struct FastCvt {
    [[maybe_unused]] static constexpr bool kTracks = TRACK;
    [[maybe_unused]] static constexpr bool kCoordsInShort = false;
    float    hi = 0.0f;
    uint32_t max_idx = 0;
    uint32_t lim = 0xFFFFFFFFu;
    __device__ __forceinline__ void note(float a, float b, float c, float d, float e)
    {
        if (TRACK) {
            hi = __builtin_fmaxf(__builtin_fmaxf(hi, a), b);
            hi = __builtin_fmaxf(__builtin_fmaxf(hi, c), d);
            hi = __builtin_fmaxf(hi, e);
        }
    }
    __device__ __forceinline__ int32_t cvt(float f) const { return cvt_sat(f); }
    // Clamp in the float domain first (one v_med3_f32; NaN -> 0 like the x86 path), then convert: for
    // f < 2^31 this equals clamp(trunc(f), 0, dim-1); f >= 2^31 is the case redo() reports.
    __device__ __forceinline__ int32_t pixel(float f, int32_t, float dim_m1_f) const
    {
        return cvt_sat(__builtin_amdgcn_fmed3f(f, 0.0f, dim_m1_f));
    }
    // The window only ever slides for the raster's very last pixel: clamp the address (so nothing past the
    // raster is read), remember the largest index seen, and let redo() send the lane through the exact path
    // if any index actually needed the slide.
    __device__ __forceinline__ uint32_t window(uint32_t idx, uint32_t l, uint32_t& shift)
    {
        max_idx = max(max_idx, idx);
        lim = l;
        shift = 0u;
        return min(idx, l);
    }
    __device__ __forceinline__ bool redo() const { return (TRACK && hi >= 2147483648.0f) || max_idx > lim; }
};
using LazyCvt = FastCvt<true>;
using LazyCvt = FastCvt<true>;

// The voxel readers consume a point's coordinates as numbers, not as the record's 16-bit fields: when every converted
// coordinate of the lane lies inside int16 the converted value IS the record's field (no pack, no sign extension per point).
// This policy keeps a second running maximum, of |x|, |y|, |z| in millimetres (the same three instructions as FastCvt<true>'s
// one maximum over five values), and sends the lane through the exact path — whose values are then wrapped like the record's —
// when it reached 2^15. The colour coordinates keep their 2^31 check (TRACK) as in FastCvt.
template <bool TRACK>
struct VoxCvt : FastCvt<TRACK> {
    static constexpr bool kCoordsInShort = true;
    float hc = 0.0f;
    __device__ __forceinline__ void note(float a, float b, float c, float d, float e)
    {
        hc = __builtin_fmaxf(__builtin_fmaxf(hc, __builtin_fabsf(a)), __builtin_fabsf(b));
        hc = __builtin_fmaxf(hc, __builtin_fabsf(c));
        if (TRACK) this->hi = __builtin_fmaxf(__builtin_fmaxf(this->hi, d), e);
    }
    __device__ __forceinline__ bool redo() const { return hc >= 32768.0f || FastCvt<TRACK>::redo(); }
};

// Arithmetic policy of the depth->colour projection. Every policy the product launches is bit-identical
// to IeeeMath on the inputs it is launched for (see "certification" in pcs_capi.cpp and DESIGN.md);
// tools/lab/kernel_lab.hip holds the exhaustive / fuzz checks and the measurements behind each choice.
struct IeeeMath {
    static constexpr bool kIdentR = false;
    static constexpr bool kRowConst = false;
    // 0 exact conversions, 1 fast with overflow tracking, 2 fast, overflow certified impossible.
    // The tracked fast form is exact for every input (its redo path IS the exact form), so even the
    // fallback policy uses it; only the quotients stay on the IEEE expansion here.
    static constexpr int kCvtMode = 1;
    // rs2_transform_point_to_point: R column-major, products and sums individually rounded, left to right
    static __device__ __forceinline__ void d2c(const StreamParams& P, float X, float Y, float Z,
                                               float& P0, float& P1, float& P2)
    {
        P0 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.R[0], X), __fmul_rn(P.R[3], Y)), __fmul_rn(P.R[6], Z)), P.t[0]);
        P1 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.R[1], X), __fmul_rn(P.R[4], Y)), __fmul_rn(P.R[7], Z)), P.t[1]);
        P2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(P.R[2], X), __fmul_rn(P.R[5], Y)), __fmul_rn(P.R[8], Z)), P.t[2]);
    }
    // two quotients over one denominator (rs2_project_point_to_pixel: x = P0/P2, y = P1/P2)
    static __device__ __forceinline__ void div2(float a0, float a1, float b, float& q0, float& q1)
    {
        q0 = __fdiv_rn(a0, b);
        q1 = __fdiv_rn(a1, b);
    }
    // quotient by a wave-uniform constant (pixel_to_texcoord: px / width); rc = host-computed RN(1/c)
    static __device__ __forceinline__ float div_const(float a, float c, float /*rc*/) { return __fdiv_rn(a, c); }
};

// CertMath: the same results with fewer instructions, launched only for streams whose configuration
// the host has certified (pcs_capi.cpp: certify_stream) and, for div_const, the device has verified.
//  * div2 is the IEEE-754 division expansion of this compiler (v_rcp, one Newton step on the
//    reciprocal, multiply, two fused corrections) WITHOUT v_div_scale / v_div_fmas / v_div_fixup, with
//    the refined reciprocal shared by both numerators. v_div_scale only ever rescales operands whose
//    exponents lie outside a window; the host proves from the configuration (depth scale, LUT ranges,
//    R, t) that every valid pixel's P0,P1,P2 lie inside it, and the pixels it cannot speak for (depth 0)
//    have their quotients discarded. Inside the window the two sequences are the same arithmetic (lab fuzz:
//    0 differences in 3.4e10 triples incl. adversarial mantissas) with ONE exception: for a numerator of
//    -0 this returns +0 where IEEE returns -0 (v_div_fixup restores the sign). The pack cannot observe it:
//    x = +-0 gives px = +-0*fx + ppx, and u = +-0 gives fma(u, W, .5) = .5 either way. pcs_deproject, which
//    exposes u and v themselves, always uses IeeeMath.
//  * div_const is Markstein's quotient: with y = RN(1/c), q0 = RN(a*y), r = a - c*q0 (exact in one fma),
//    q = RN(q0 + r*y). It is consumed only through trunc(fma(q, c, 0.5)) clamped to [0, c-1]; that
//    composite is compared with the IEEE one over ALL 2^32 numerators on the device when the context
//    is created (pcs_verify_div_const_kernel) and CertMath is used only if no numerator differs.
//  * IDENT_R: depth->colour rotation is exactly the identity (and t has no negative zeros), so
//    R*p + t is p + t: the dropped products are exact (1*x) or signed zeros that cannot change a sum.
template <bool IDENT_R, bool NO_OVERFLOW = false>
struct CertMath {
    static constexpr bool kIdentR = IDENT_R;
    static constexpr bool kRowConst = false;
    static constexpr int kCvtMode = NO_OVERFLOW ? 2 : 1;
    static __device__ __forceinline__ void d2c(const StreamParams& P, float X, float Y, float Z,
                                               float& P0, float& P1, float& P2)
    {
        if (IDENT_R) {
            P0 = __fadd_rn(X, P.t[0]);
            P1 = __fadd_rn(Y, P.t[1]);
            P2 = __fadd_rn(Z, P.t[2]);
        } else {
            IeeeMath::d2c(P, X, Y, Z, P0, P1, P2);
        }
    }
    static __device__ __forceinline__ void div2(float a0, float a1, float b, float& q0, float& q1)
    {
        float y = __builtin_amdgcn_rcpf(b);
        const float e = __fmaf_rn(-b, y, 1.0f);
        y = __fmaf_rn(e, y, y);
        float q = __fmul_rn(a0, y);
        float r = __fmaf_rn(-b, q, a0);
        q = __fmaf_rn(r, y, q);
        r = __fmaf_rn(-b, q, a0);
        q0 = __fmaf_rn(r, y, q);
        q = __fmul_rn(a1, y);
        r = __fmaf_rn(-b, q, a1);
        q = __fmaf_rn(r, y, q);
        r = __fmaf_rn(-b, q, a1);
        q1 = __fmaf_rn(r, y, q);
    }
    static __device__ __forceinline__ float div_const(float a, float c, float rc)
    {
        const float q0 = __fmul_rn(a, rc);
        const float r = __fmaf_rn(-c, q0, a);
        return __fmaf_rn(r, rc, q0);
    }
};

using CertNoOvf = CertMath<false, true>;
using CertIdentNoOvf = CertMath<true, true>;

// CertRowConst: CertMath<IDENT_R> for streams whose COLOUR ROW does not depend on the depth value (StreamParams::ident_r == 2). With
// R = I and t_y = t_z = 0 a pixel's colour row is trunc(fma(((z * my) / z * fy + ppy) / H, H, 0.5)) clamped — mathematically a function of
// its raster row alone, in floats almost one: the rounding of (z * my) / z moves py by ~1e-4 of a pixel, which changes the integer only for a
// row whose py lies that close to k - 0.5. Whether any row of a stream does is not argued but SWEPT when the context is created
// (pcs_certify_color_row_kernel: every row x every Z16 value 1 .. 65 535 through the IEEE chain); where none does, the row index of each
// raster row is a table (behind the my LUT) and the second quotient, its projection, texture coordinate, scale, clamp and conversion —
// 13 of the ~70 VALU instructions of a pixel — are one load per lane and one select per pixel. Used by the voxel reader (VALU-bound).
struct CertRowConst : CertMath<true, false> {
    [[maybe_unused]] static constexpr bool kRowConst = true;
};
// The same over the no-overflow form: the dense kernel's policy for launches whose streams are all row-constant (dense_tile_rowc).
struct CertRowConstNoOvf : CertMath<true, true> {
    [[maybe_unused]] static constexpr bool kRowConst = true;
};

// a2 colour lookup (src/pcs-camera-optimized.cpp:431-452, 584-585): texcoord -> byte index of the pixel.
__device__ __forceinline__ void color_coords(const StreamParams& P, float u, float v, float& xf, float& yf)
{
    xf = __fmaf_rn(u, P.c_w_f, 0.5f);
    yf = __fmaf_rn(v, P.c_h_f, 0.5f);
}

// Returns R | G<<8 | B<<16 in the low 24 bits (the top byte is whatever followed in memory): shorts 3 and 4
// of the record are its low half and byte 2.
template <class Cvt>
__device__ __forceinline__ uint32_t color_fetch(const StreamParams& P, const uint8_t* __restrict__ color,
                                                int32_t xi, int32_t yi, Cvt& cv)
{
    // xi < 2^24, bpp small, yi < 2^24, stride < 2^24: 24-bit multiplies are exact in 32 bits and full rate
    const uint32_t idx = __umul24((uint32_t)xi, (uint32_t)P.bpp) + __umul24((uint32_t)yi, (uint32_t)P.stride);
    uint32_t shift;
    const uint32_t off = cv.window(idx, P.color_bytes - 4u, shift);
    uint32_t w;
    __builtin_memcpy(&w, color + off, 4);
    return w >> shift;                   // R | G<<8 | B<<16 | (don't care)<<24
}

// a2 rigid transform + scale (src/pcs-camera-optimized.cpp:455-491).
// Order matters: x*col0 + t first, then + y*col1, then + z*col2; then a separately rounded * 1000.0f.
__device__ __forceinline__ float world_mm(const float* __restrict__ Mr, float X, float Y, float Z)
{
    float a = __fmaf_rn(X, Mr[0], Mr[3]);
    a = __fmaf_rn(Y, Mr[1], a);
    a = __fmaf_rn(Z, Mr[2], a);
    return __fmul_rn(a, 1000.0f);
}

// a3, the reference's default (no -m) loop (src/pcs-camera-optimized.cpp:654-660), as its build compiles it (g++ -O3 -mfma, contraction
// on; oracle/pcs_oracle.c: pcs_oracle_pack_scalar_variant restates that compile and is pinned to its bytes): the textbook order
// ((m0*x + m1*y) + m2*z) + t with m1*y the one rounded product, m0*x and m2*z fused into the sums, + t a rounded sum; then `* CONV_RATE`
// in DOUBLE — exact, 24 + 10 bits — and static_cast<short> of it, cvttsd2si: truncate, NaN or outside [-2^31, 2^31) -> 0x80000000.
__device__ __forceinline__ float world_scalar(const float* __restrict__ Mr, float X, float Y, float Z)
{
    float a = __fmul_rn(Mr[1], Y);
    a = __fmaf_rn(Mr[0], X, a);
    a = __fmaf_rn(Mr[2], Z, a);
    return __fadd_rn(a, Mr[3]);
}
// The conversion as written, for every a. Returns the converted value; the record keeps its low 16 bits. v_cvt_i32_f64 saturates,
// which agrees with cvttsd2si in those bits for NaN (0 / INT_MIN) and below -2^31 (INT_MIN both) but not from 2^31 up (INT_MAX: 0xFFFF
// where x86 leaves 0). a * 1000 >= 2^31 <=> a >= 2147483.648, and floats of that size are 0.25 apart: <=> a >= 2147483.75f — one FP32
// compare; a NaN fails it and converts to 0.
__device__ __forceinline__ uint32_t mm_scalar_exact(float a)
{
    const double s = __dmul_rn((double)a, 1000.0);
    int32_t q;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(q) : "v"(s));
    return a >= 2147483.75f ? 0u : (uint32_t)q;
}
// The same bits without FP64, for |a| < 2^14 (16 km; NaN included): with p = RN(a * 1000) and e = fma(a, 1000, -p) the product is
// p + e exactly, so its round-towards-zero float is p itself, or — where e points back towards zero — p's neighbour on that side
// (one less in the integer reading of its bits, either sign). |a * 1000| < 2^24, where every integer is a float: the truncation of
// the product lies between that float and zero, so truncating the float gives it. (p * e cannot underflow to zero where it matters:
// |p| >= 1 there and |e| >= 2^-149.) Callers take the exact form for anything larger: the Cvt policy's running maximum is told
// |a| * 2^17, which reaches its 2^31 where |a| reaches 2^14.
__device__ __forceinline__ uint32_t mm_scalar_residual(float a)
{
    const float p = __fmul_rn(a, 1000.0f);
    const float e = __fmaf_rn(a, 1000.0f, -p);
    const bool back = __fmul_rn(p, e) < 0.0f;
    return (uint32_t)cvt_sat(__int_as_float(__float_as_int(p) - (int32_t)back));
}

// Pack arithmetic policies: which of the reference's two loops a record's world coordinates follow. The colour index is the same in
// both (fma(u, W, .5f), truncate, clamp).
//   SimdArith        -m, copyPointCloudXYZRGBToBufferSIMD (a2): world_mm and the Cvt policy's conversion. The default everywhere.
//   ScalarArith<CUT> the default loop (a3): world_scalar and mm_scalar_residual / mm_scalar_exact. CUT: its -c test (:640-646) — a point is written iff z != 0 && x != 0 &&
//                    !(z > 1.5) on the camera-frame floats (`-2 < x < 2` is always true; a NaN z or x passes) — there is no
//                    compaction, so the fused tiles select a skipped point's record to zero and the a2 twin does not store it.
struct SimdArith {
    static constexpr bool kScalar = false, kCut = false;
};
template <bool CUT>
struct ScalarArith {
    static constexpr bool kScalar = true, kCut = CUT;
};
__device__ __forceinline__ bool scalar_cut_keeps(float X, float Z)
{
    return Z != 0.0f && X != 0.0f && !(Z > 1.5f);
}

// v_perm_b32: every result byte picks one of the 8 bytes of {hi, lo} (lo = bytes 0-3, hi = bytes 4-7).
// Two selectors cover all the 16-bit shuffles of the record packing in ONE instruction each, with no
// masks or shifts around them:
//   kLoLo: lo.lo16 | hi.lo16 << 16          kHiLo: lo.hi16 | hi.lo16 << 16
constexpr uint32_t kLoLo = 0x05040100u, kHiLo = 0x05040302u;
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

struct Record {              // one 10-byte point as three pieces
    uint32_t xy;             // x | y << 16
    uint32_t zc;             // z | (R | G<<8) << 16
    uint32_t b;              // B            (low 16 bits valid)
};

// Brown-Conrady terms shared by deprojection (inverse model) and projection (modified model);
// evaluation order as in librealsense's rsutil.h, each op rounded.
__device__ __forceinline__ float bc_radial(const float* k, float r2)
{
    // 1 + k0*r2 + k1*r2*r2 + k4*r2*r2*r2, left to right
    float f = __fadd_rn(1.0f, __fmul_rn(k[0], r2));
    f = __fadd_rn(f, __fmul_rn(__fmul_rn(k[1], r2), r2));
    f = __fadd_rn(f, __fmul_rn(__fmul_rn(__fmul_rn(k[4], r2), r2), r2));
    return f;
}
// a + 2*kA*x*y + kB*(r2 + 2*a_axis*a_axis)
__device__ __forceinline__ float bc_tangential(float a, float kA, float kB, float x, float y, float r2, float axis)
{
    float s = __fadd_rn(a, __fmul_rn(__fmul_rn(__fmul_rn(2.0f, kA), x), y));
    return __fadd_rn(s, __fmul_rn(kB, __fadd_rn(r2, __fmul_rn(__fmul_rn(2.0f, axis), axis))));
}

// a5 for one pixel: depth value d, normalised ray (mx,my) from the LUTs.
template <bool DDIST, bool CDIST, class Mth>
__device__ __forceinline__ PointIn deproject_pixel(const StreamParams& P, uint32_t d, float mx, float my)
{
    const float z = __fmul_rn(P.depth_scale, (float)d);
    if (DDIST && P.ddist) {   // template gate compiles it in; the per-stream flag is wave-uniform
        const float r2 = __fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my));
        const float f = bc_radial(P.dk, r2);
        const float ux = bc_tangential(__fmul_rn(mx, f), P.dk[2], P.dk[3], mx, my, r2, mx);
        const float uy = bc_tangential(__fmul_rn(my, f), P.dk[3], P.dk[2], mx, my, r2, my);
        mx = ux; my = uy;
    }
    PointIn p;
    p.X = __fmul_rn(z, mx);
    p.Y = __fmul_rn(z, my);
    p.Z = z;
    float P0, P1, P2;
    Mth::d2c(P, p.X, p.Y, p.Z, P0, P1, P2);
    // rs2_project_point_to_pixel
    float x, y;
    Mth::div2(P0, P1, P2, x, y);
    if (CDIST && P.cdist) {
        const float r2 = __fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y));
        const float f = bc_radial(P.ck, r2);
        x = __fmul_rn(x, f); y = __fmul_rn(y, f);
        const float dx = bc_tangential(x, P.ck[2], P.ck[3], x, y, r2, x);
        const float dy = bc_tangential(y, P.ck[3], P.ck[2], x, y, r2, y);
        x = dx; y = dy;
    }
    float px = __fadd_rn(__fmul_rn(x, P.c_fx), P.c_ppx);
    float py = __fadd_rn(__fmul_rn(y, P.c_fy), P.c_ppy);
    if (CDIST && P.tex_half) {      // older librealsense pixel_to_texcoord: (pixel + 0.5) / size. Rides on the CDIST
        px = __fadd_rn(px, 0.5f);   // instantiation (the host routes such streams there) so the common path pays nothing.
        py = __fadd_rn(py, 0.5f);
    }
    // pixel_to_texcoord; invalid depth (z == 0) -> texcoord (0,0). The quotients are computed
    // unconditionally and then selected: a conditional here becomes a divergent branch per pixel, which
    // stops the scheduler from interleaving the 8 pixels of a lane.
    const float qu = Mth::div_const(px, P.c_w_f, P.c_rw);
    const float qv = Mth::div_const(py, P.c_h_f, P.c_rh);
    const bool valid = (z != 0.0f);
    p.u = valid ? qu : 0.0f;
    p.v = valid ? qv : 0.0f;
    return p;
}

// The same pixel under CertRowConst (R = I, t_y = t_z = 0, no distortion; see the policy): X, Y, Z and u as above, and in place of v the
// pixel's colour ROW itself — `crow`, the table's entry for the raster row, 0 for an invalid pixel — carried in p.v as an INTEGER. A
// function of its own, so that the instantiations every other kernel uses keep exactly the code they had (an if inside deproject_pixel
// cost the distortion instantiation of the dense kernel 800 instructions: the two copies of its tail no longer merged).
template <class Mth>
__device__ __forceinline__ PointIn deproject_pixel_rowc(const StreamParams& P, uint32_t d, float mx, float my, int crow)
{
    const float z = __fmul_rn(P.depth_scale, (float)d);
    PointIn p;
    p.X = __fmul_rn(z, mx);
    p.Y = __fmul_rn(z, my);
    p.Z = z;
    const float P0 = __fadd_rn(p.X, P.t[0]);
    const float P2 = __fadd_rn(p.Z, P.t[2]);
    float x, y_unused;
    Mth::div2(P0, P0, P2, x, y_unused);                  // (the second quotient is dead code)
    const float px = __fadd_rn(__fmul_rn(x, P.c_fx), P.c_ppx);
    const float qu = Mth::div_const(px, P.c_w_f, P.c_rw);
    const bool valid = (z != 0.0f);
    p.u = valid ? qu : 0.0f;
    p.v = __int_as_float(valid ? crow : 0);
    return p;
}

// -c predicate on camera-frame z and x (src/pcs-camera-optimized.cpp:398-401, 504-511).
__device__ __forceinline__ bool in_range(float X, float Z)
{
    return Z > 0.0f && Z <= 1.5f && X > -2.0f && X <= 2.0f;
}

// Keep mask for a lane's 8 consecutive points (point index i0 + k, i0 % 8 == 0).
// Keep mask from the per-point predicate bits: rng = -c range test, nz = depth valid (bit k = point i0 + k).
__device__ __forceinline__ uint32_t keep_from_bits(uint32_t rng, uint32_t nz, uint32_t i0, uint32_t n, uint32_t flags)
{
    uint32_t live = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) live |= (uint32_t)(i0 + k < n) << k;
    uint32_t keep = live;
    if (flags & PCS_FLAG_CUTOFF) {
        uint32_t gate = rng;
        if (flags & PCS_FLAG_CUTOFF_COMPAT) {
            // the reference gates point k of each aligned group of four with point 3-k's test
            // (lane-reversed mask, :501-502 vs :519); groups that run past n use their own test.
            uint32_t rev = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) rev |= ((rng >> ((k & 4) | (3 - (k & 3)))) & 1u) << k;
            const uint32_t full_lo = (i0 + 3 < n) ? 0x0Fu : 0u;
            const uint32_t full_hi = (i0 + 7 < n) ? 0xF0u : 0u;
            const uint32_t full = full_lo | full_hi;
            gate = (rev & full) | (rng & ~full);
        }
        keep &= gate;
    }
    if (flags & PCS_FLAG_DROP_INVALID) keep &= nz;
    return keep;
}

// Keep mask for a lane's 8 consecutive points (point index i0 + k, i0 % 8 == 0).
__device__ __forceinline__ uint32_t keep_mask8(const PointIn (&p)[8], uint32_t i0, uint32_t n, uint32_t flags)
{
    uint32_t rng = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        rng |= (uint32_t)in_range(p[k].X, p[k].Z) << k;
        nz  |= (uint32_t)(p[k].Z != 0.0f) << k;
    }
    return keep_from_bits(rng, nz, i0, n, flags);
}

// ---- crop box (pcs_set_crop_box_mm) -----------------------------------------------------------------
// The world-frame box on the RECORD: a point is kept iff each of its three shorts s_a (the low 16 bits of the converted coordinate, read
// as signed: after the int16 wrap) lies in [lo_a, hi_a]. The box reaches a kernel as three dwords in its arguments (SGPRs), never
// through StreamParams:  xy = lo_x | lo_y << 16,  zz = lo_z | span_z << 16,  sp = span_x | span_y << 16,  span_a = hi_a - lo_a (0 .. 65535).
// Per axis ((s - lo) & 0xFFFF) <= span in 16-bit modular arithmetic is lo <= s <= hi for signed shorts with lo <= hi.
struct CropBox { uint32_t xy, zz, sp; };
__device__ __forceinline__ bool box_keeps(const CropBox& b, uint32_t rxy, uint32_t rzc)
{
    const uint32_t dx = (rxy - b.xy) & 0xFFFFu;                      // a borrow out of the low half cannot reach it
    const uint32_t dy = ((rxy >> 16) - (b.xy >> 16)) & 0xFFFFu;
    const uint32_t dz = (rzc - b.zz) & 0xFFFFu;
    return dx <= (b.sp & 0xFFFFu) && dy <= (b.sp >> 16) && dz <= (b.zz >> 16);
}

// The three converted world coordinates of a point under -m arithmetic (world_mm and the Cvt policy's conversion): what make_record
// packs into the record's first three shorts. The boxed count pass and the boxed emit tile both call this and nothing else for them,
// under the same Cvt ladder, so the two passes agree on every bit. `noted`: the floats the policy's running maximum must be told.
template <class Cvt>
__device__ __forceinline__ void world_ints(const StreamParams& P, const PointIn& p, const Cvt& cv, float (&noted)[3], uint32_t (&w)[3])
{
    noted[0] = world_mm(P.M + 0, p.X, p.Y, p.Z);
    noted[1] = world_mm(P.M + 4, p.X, p.Y, p.Z);
    noted[2] = world_mm(P.M + 8, p.X, p.Y, p.Z);
    w[0] = (uint32_t)cv.cvt(noted[0]); w[1] = (uint32_t)cv.cvt(noted[1]); w[2] = (uint32_t)cv.cvt(noted[2]);
}

// Wavefront-wide inclusive prefix sum (64 lanes, all active) by DPP: four row_shr steps scan each row of 16 lanes,
// row_bcast:15 / row_bcast:31 carry the row totals across (the gfx9 sequence). No lane-index registers, no LDS
// crossbar (ds_bpermute, which __shfl_up compiles to) — and nothing loop-invariant for the compiler to hoist out of
// a persistent tile loop and spill.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x)
{
    uint32_t v = x;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

// Wavefront-wide exclusive prefix sum of a small per-lane count; wave_total is wave-uniform (an SGPR).
__device__ __forceinline__ uint32_t wave_exclusive_scan(uint32_t c, uint32_t& wave_total)
{
    const uint32_t inc = wave_inclusive_scan(c);
    wave_total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    return inc - c;
}

// Wavefront-wide sum (wave-uniform).
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(v), 63);
}

// ------------------------------------------------------------------------------------------------
// Point sources. A source hands each lane its 8 consecutive points of the tile.
// ------------------------------------------------------------------------------------------------

// Z16 raster + LUTs -> points (the fused a5 stage).
template <bool DDIST, bool CDIST, class Mth = IeeeMath>
struct DepthSource {
    using Math = Mth;
    const uint16_t* __restrict__ depth;

    // The distortion decision is taken ONCE per lane, outside the pixel loop: a (wave-uniform) test per
    // pixel splits the lane's code into 16 basic blocks, which stops the scheduler from interleaving the
    // pixels and the compiler from packing pairs of them into v_pk_* instructions (measured: the emit
    // kernel ran 27 us with per-pixel tests vs 19 us for the dense kernel without them).
    // The fast path in two steps, for kernels that want to do something between requesting a lane's inputs and using them
    // (the single-pass compaction counts and publishes from the raw Z16 words first): fast() says whether it applies
    // (uniform over the launch's stream), fetch() issues the loads, deproject() consumes them.
    struct Raw { uint4 dv; f32x4 ma, mb; float my; };
    __device__ __forceinline__ bool fast(const StreamParams& P) const { return (P.W & 7) == 0 && ((uintptr_t)depth & 15) == 0; }
    __device__ __forceinline__ Raw fetch(const StreamParams& P, uint32_t i0) const
    {
        // all 8 pixels on one raster row; one 16-byte depth load, two 16-byte LUT loads
        // floor(i0 / W) by the host-verified multiply-shift (i0 < 2^31)
        const uint32_t r = P.w_magic ? (__umulhi(i0, P.w_magic) >> P.w_shift) : i0 / (uint32_t)P.W;
        const uint32_t c0 = i0 - r * (uint32_t)P.W;
        Raw q;
        q.dv = *reinterpret_cast<const uint4*>(depth + i0);
        const gptr<float> lut_x = as_global(P.mx);
        q.ma = *reinterpret_cast<gptr<f32x4>>(lut_x + c0);
        q.mb = *reinterpret_cast<gptr<f32x4>>(lut_x + c0 + 4);
        q.my = as_global(P.my)[r];
        return q;
    }
    template <bool DD, bool CD>
    __device__ __forceinline__ void deproject(const StreamParams& P, const Raw& q, PointIn (&p)[8]) const
    {
        const uint32_t dw[4] = {q.dv.x, q.dv.y, q.dv.z, q.dv.w};
        const float mxs[8] = {q.ma.x, q.ma.y, q.ma.z, q.ma.w, q.mb.x, q.mb.y, q.mb.z, q.mb.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t d = (k & 1) ? (dw[k >> 1] >> 16) : (dw[k >> 1] & 0xFFFFu);
            p[k] = deproject_pixel<DD, CD, Mth>(P, d, mxs[k], q.my);
        }
    }

    template <bool DD, bool CD>
    __device__ __forceinline__ void load8_impl(const StreamParams& P, uint32_t i0, uint32_t n, PointIn (&p)[8]) const
    {
        if (fast(P)) {
            deproject<DD, CD>(P, fetch(P, i0), p);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t i = min(i0 + k, n - 1);
                const uint32_t r = i / (uint32_t)P.W;
                const uint32_t c = i - r * (uint32_t)P.W;
                p[k] = deproject_pixel<DD, CD, Mth>(P, depth[i], as_global(P.mx)[c], as_global(P.my)[r]);
            }
        }
    }

    // CertRowConst: the colour row of raster row r lies behind the H floats of the my LUT (StreamParams::my)
    __device__ __forceinline__ void load8_rowc(const StreamParams& P, uint32_t i0, uint32_t n, PointIn (&p)[8]) const
    {
        const gptr<float> lut_y = as_global(P.my);
        if (fast(P)) {
            const Raw q = fetch(P, i0);
            const uint32_t r = P.w_magic ? (__umulhi(i0, P.w_magic) >> P.w_shift) : i0 / (uint32_t)P.W;
            const int crow = __float_as_int(lut_y[(uint32_t)P.H + r]);
            const uint32_t dw[4] = {q.dv.x, q.dv.y, q.dv.z, q.dv.w};
            const float mxs[8] = {q.ma.x, q.ma.y, q.ma.z, q.ma.w, q.mb.x, q.mb.y, q.mb.z, q.mb.w};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t d = (k & 1) ? (dw[k >> 1] >> 16) : (dw[k >> 1] & 0xFFFFu);
                p[k] = deproject_pixel_rowc<Mth>(P, d, mxs[k], q.my, crow);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t i = min(i0 + k, n - 1);
                const uint32_t r = i / (uint32_t)P.W;
                const uint32_t c = i - r * (uint32_t)P.W;
                p[k] = deproject_pixel_rowc<Mth>(P, depth[i], as_global(P.mx)[c], lut_y[r], __float_as_int(lut_y[(uint32_t)P.H + r]));
            }
        }
    }

    // The same with the lane's eight Z16 values already in registers (requested a round earlier: fast(P) rasters only).
    __device__ __forceinline__ Raw fetch_luts(const StreamParams& P, uint32_t i0, const uint4& dv) const
    {
        const uint32_t r = P.w_magic ? (__umulhi(i0, P.w_magic) >> P.w_shift) : i0 / (uint32_t)P.W;
        const uint32_t c0 = i0 - r * (uint32_t)P.W;
        Raw q;
        q.dv = dv;
        const gptr<float> lut_x = as_global(P.mx);
        q.ma = *reinterpret_cast<gptr<f32x4>>(lut_x + c0);
        q.mb = *reinterpret_cast<gptr<f32x4>>(lut_x + c0 + 4);
        q.my = as_global(P.my)[r];
        return q;
    }
    __device__ __forceinline__ void load8_pre(const StreamParams& P, uint32_t i0, uint32_t n, const uint4& dv, PointIn (&p)[8]) const
    {
        if (i0 >= n) {
#pragma unroll
            for (int k = 0; k < 8; k++) p[k] = PointIn{0, 0, 0, 0, 0};
            return;
        }
        const Raw q = fetch_luts(P, i0, dv);
        if constexpr (Mth::kRowConst) {
            const uint32_t r = P.w_magic ? (__umulhi(i0, P.w_magic) >> P.w_shift) : i0 / (uint32_t)P.W;
            const int crow = __float_as_int(as_global(P.my)[(uint32_t)P.H + r]);
            const uint32_t dw[4] = {q.dv.x, q.dv.y, q.dv.z, q.dv.w};
            const float mxs[8] = {q.ma.x, q.ma.y, q.ma.z, q.ma.w, q.mb.x, q.mb.y, q.mb.z, q.mb.w};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t d = (k & 1) ? (dw[k >> 1] >> 16) : (dw[k >> 1] & 0xFFFFu);
                p[k] = deproject_pixel_rowc<Mth>(P, d, mxs[k], q.my, crow);
            }
        } else {
            if ((DDIST || CDIST) && (P.ddist | P.cdist | P.tex_half)) deproject<DDIST, CDIST>(P, q, p);
            else deproject<false, false>(P, q, p);
        }
    }

    __device__ __forceinline__ void load8(const StreamParams& P, uint32_t i0, uint32_t n, PointIn (&p)[8]) const
    {
        if (i0 >= n) {
#pragma unroll
            for (int k = 0; k < 8; k++) p[k] = PointIn{0, 0, 0, 0, 0};
            return;
        }
        if constexpr (Mth::kRowConst) {
            load8_rowc(P, i0, n, p);
        } else {
            if ((DDIST || CDIST) && (P.ddist | P.cdist | P.tex_half)) load8_impl<DDIST, CDIST>(P, i0, n, p);
            else load8_impl<false, false>(P, i0, n, p);
        }
    }
};

// Request a stream's constants (and this launch's raster pointers) with ONE batch of scalar loads at the top of a
// kernel. Left alone, hipcc asks for them one dependent group at a time — the kernarg, then n_points for the early
// exit, then the raster pointers and the width, then the LUT pointers — four scalar round trips before the first
// Z16 load of a workgroup can be issued, paid in full by the first wave of workgroups of every launch (1.8 rounds of
// them make up an 8 x 720p launch). The empty asm only says "these are needed HERE".
// LEAN: leave out the two quads that hold nothing but distortion coefficients (dk[1..4], ck[0..3]; a stream that has any
// fetches them when it gets there) and, for IDENT_R policies, the two quads of the depth->colour rotation that p + t never
// reads. What this buys is SGPRs at the point where the most of them are live: the hardware admits a 256-lane workgroup per
// CU only while its waves' SGPR allocation allows it — 7 per CU up to 96 SGPRs, 6 from 97 (MI355X_MICROARCH.md, residency) —
// and the emit kernel's extra arguments had pushed it to 103.
template <bool LEAN = false, bool IDENT_R = false>
__device__ __forceinline__ void request_constants(const StreamParams& P, const void* a, const void* b, const void* c = nullptr)
{
    static_assert(sizeof(StreamParams) == 19 * 16, "request_constants covers the struct in 19 quads");
    static_assert(offsetof(StreamParams, dk) == 39 * 4 && offsetof(StreamParams, ck) == 44 * 4 && offsetof(StreamParams, R) == 12 * 4,
                  "quads 10, 11 = dk[1..4], ck[0..3]; quads 3, 4 = R[0..7]");
    typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));
    const u32x4s* q = reinterpret_cast<const u32x4s*>(&P);
    if (LEAN && IDENT_R)
        asm volatile("" :: "s"(q[0]), "s"(q[1]), "s"(q[2]), "s"(q[5]), "s"(q[6]), "s"(q[7]), "s"(q[8]), "s"(q[9]),
                           "s"(q[12]), "s"(q[13]), "s"(q[14]), "s"(q[15]), "s"(q[16]), "s"(q[17]), "s"(q[18]),
                           "s"(a), "s"(b), "s"(c));
    else if (LEAN)
        asm volatile("" :: "s"(q[0]), "s"(q[1]), "s"(q[2]), "s"(q[3]), "s"(q[4]), "s"(q[5]), "s"(q[6]), "s"(q[7]), "s"(q[8]), "s"(q[9]),
                           "s"(q[12]), "s"(q[13]), "s"(q[14]), "s"(q[15]), "s"(q[16]), "s"(q[17]), "s"(q[18]),
                           "s"(a), "s"(b), "s"(c));
    else
        asm volatile("" :: "s"(q[0]), "s"(q[1]), "s"(q[2]), "s"(q[3]), "s"(q[4]), "s"(q[5]), "s"(q[6]), "s"(q[7]), "s"(q[8]), "s"(q[9]),
                           "s"(q[10]), "s"(q[11]), "s"(q[12]), "s"(q[13]), "s"(q[14]), "s"(q[15]), "s"(q[16]), "s"(q[17]), "s"(q[18]),
                           "s"(a), "s"(b), "s"(c));
}

}  // namespace

}  // namespace pcs
