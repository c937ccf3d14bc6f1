/*
 * ref_harness.cpp — C ABI around the reference's own sendXYZRGBPointcloud. TEST INFRASTRUCTURE ONLY.
 *
 * The reference translation unit is included BY PATH at build time (-DPCS_REF_TU='"<dir>/src/pcs-camera-optimized.cpp"',
 * see ../Makefile target `ref`), so none of its text lives in this tree; the product, oracle/_ref/libpcs_ref.so,
 * is never committed. Everything a record's bytes depend on is computed by the reference's functions; this file only
 * stores the caller's arguments into the globals those functions read.
 */
#ifndef PCS_REF_TU
#error "build with -DPCS_REF_TU='\"<reference>/src/pcs-camera-optimized.cpp\"' (oracle/Makefile, target ref)"
#endif
#ifndef PCS_REF_FLAGS
#define PCS_REF_FLAGS "unknown"
#endif

#define main pcs_ref_tu_main
#include PCS_REF_TU
#undef main

extern "C" {

/* The reference's BUF_SIZE: the byte count its a1 clears at the head of the buffer on every call. */
int pcs_ref_buf_size(void) { return BUF_SIZE; }

/* Compiler and flags this library was built with: short(float) of NaN / out-of-range values is formally undefined,
 * so fixtures that hold such values say which compile produced them. */
const char* pcs_ref_compiler(void) { return __VERSION__; }
const char* pcs_ref_flags(void) { return PCS_REF_FLAGS; }

/* One call of sendXYZRGBPointcloud. m16 = row-major 4x4 (tf_mat's layout). The caller owns `buffer`, which must hold
 * max(BUF_SIZE, 4 + 10 * n) bytes and then some: the reference clears BUF_SIZE bytes and bounds nothing.
 * n must be a multiple of 4 when simd != 0 (the loop reads four points per step). Not reentrant: geometry is global. */
int pcs_ref_send(const float* vertices, const float* texcoords, int n, const unsigned char* color, int w, int h, int bpp,
                 int stride, const float* m16, int simd, int cut, int threads, short* buffer)
{
    for (int i = 0; i < 16; i++) tf_mat[i] = m16[i];
    /* rebuild the four column vectors the reference derives from tf_mat once, at static-initialisation time:
     * lane r of column c holds row r of the matrix, the fourth lane is zero */
    __m128* const column[4] = { &ss_a, &ss_b, &ss_c, &ss_d };
    for (int c = 0; c < 4; c++) *column[c] = _mm_setr_ps(m16[c], m16[4 + c], m16[8 + c], 0.0f);
    use_simd = simd != 0;
    cutoff = cut != 0;
    num_of_threads = threads;
    send_buffer = false;      /* no socket */
    initialized = false;      /* the raster geometry is cached in globals on the first call: take this call's */

    rs2::points pts;
    pts.v = reinterpret_cast<const rs2::vertex*>(vertices);
    pts.t = reinterpret_cast<const rs2::texture_coordinate*>(texcoords);
    pts.n = (size_t)n;
    rs2::video_frame col;
    col.data = color; col.w = w; col.h = h; col.bpp = bpp; col.stride = stride;
    return sendXYZRGBPointcloud(pts, col, buffer);
}

}  // extern "C"
