// pcs_kernels_filter.hip — the depth pre-filter (pcs_set_depth_filter / pcs_filter_depth_device): temporal smoothing and
// fill-from-left on Z16 rasters, every stream of a context in one launch. The definition is DESIGN.md §3 "Depth pre-filter"; it is
// this project's own (modelled on librealsense's temporal and hole-filling blocks, parity with librealsense unpinned) and
// tests/np_depth_filter.py restates it in numpy; the kernel is held to that restatement bit for bit.
//
// Shape: a workgroup owns one whole row of one stream (in place is safe: a lane stores exactly the pixels it loaded; the fill's
// carry never leaves the workgroup). One pass of its 256 lanes covers 2048 pixels of the row, 8 consecutive pixels per lane; a wider
// row loops and carries one value in a register; a launch whose widest row needs fewer lanes starts fewer waves (whole ones). One
// row per workgroup measured faster than 2, 4 or 8 (8 x 1280x720, both stages, 256 lanes: 24.5 / 26.0 / 28.4 / 36.6 us; with the
// three waves a 1280-pixel row fills, 23.8): the kernel waits on memory, and more, shorter workgroups keep more requests in flight.
// Nontemporal stores of the state measured the same as plain ones (28.3 vs 28.4 us at four rows per workgroup): plain stores stay. Rows whose width is a multiple of 8 with 16-byte aligned rasters
// move 16 bytes per lane (in, last, out) and 8 bytes of hist; every other row takes 2-byte accesses.
//
// Bytes per pixel: 10 with the temporal stage (2 in + 2 out + 4 last read/write + 2 hist read/write), 4 for hole fill alone.
//
// Second half of the file: the depth decimation (pcs_decimate_depth_device), the stage ahead of the filter; its own comment is there.
#include <algorithm>

#include "pcs_device.h"

namespace pcs {

namespace {

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

template <bool TEMPORAL, bool FILL, bool COUNT>
__global__ __launch_bounds__(kBlockThreads)
void pcs_depth_filter_kernel(const FilterStream* __restrict__ tab, FilterPtrs fp, FilterArgs fa, uint32_t* __restrict__ tile_kept)
{
    __shared__ uint32_t s_last[2][4];               // per pass parity: each wave's last non-zero value (0: none)
    __shared__ uint32_t s_tiles[kFilterSlots];      // non-zero output pixels per tile this workgroup touches
    const int s = blockIdx.y;
    const FilterStream F = tab[s];
    const uint32_t W = F.W;
    const uint32_t r = blockIdx.x;
    if (r >= F.H) return;                           // (uniform: before any barrier)
    const uint16_t* in = fp.in[s];
    uint16_t* out = fp.out[s];
    const bool vec = (W & 7u) == 0 && ((((uintptr_t)in) | ((uintptr_t)out)) & 15u) == 0;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const uint32_t pass_pixels = blockDim.x * kPointsPerLane;      // <= kTilePoints: a pass touches at most two tiles
    const uint64_t row0 = (uint64_t)r * W;
    const uint32_t tile_first = (uint32_t)(row0 / kTilePoints);
    if (COUNT) {
        if (threadIdx.x < kFilterSlots) s_tiles[threadIdx.x] = 0;
        __syncthreads();
    }
    uint32_t parity = 0;
    uint32_t carry = 0;                         // the fill's carry: starts at zero with the row
    for (uint32_t c0 = 0; c0 < W; c0 += pass_pixels, parity ^= 1u) {
        const uint32_t col = c0 + threadIdx.x * kPointsPerLane;
        const uint32_t nv = col < W ? min((uint32_t)kPointsPerLane, W - col) : 0u;      // vec: 0 or 8
        const uint64_t i0 = row0 + col;
        uint32_t o[8], l[8], h[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { o[j] = 0; l[j] = 0; h[j] = 0; }
        if (vec) {
            if (nv) {
                const uint4 v = *reinterpret_cast<const uint4*>(in + i0);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; j++) { o[2 * j] = w[j] & 0xFFFFu; o[2 * j + 1] = w[j] >> 16; }
                if (TEMPORAL) {
                    const uint4 q = *reinterpret_cast<const uint4*>(F.last + i0);
                    const uint2 b = *reinterpret_cast<const uint2*>(F.hist + i0);
                    const uint32_t lw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int j = 0; j < 4; j++) { l[2 * j] = lw[j] & 0xFFFFu; l[2 * j + 1] = lw[j] >> 16; }
#pragma unroll
                    for (int j = 0; j < 4; j++) { h[j] = (b.x >> (8 * j)) & 0xFFu; h[4 + j] = (b.y >> (8 * j)) & 0xFFu; }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((uint32_t)j < nv) {
                    o[j] = in[i0 + j];
                    if (TEMPORAL) { l[j] = F.last[i0 + j]; h[j] = F.hist[i0 + j]; }
                }
        }
        if (TEMPORAL) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t c = o[j], p = l[j], hh = h[j];
                if (c != 0) {
                    int d = (int)c - (int)p;
                    d = d < 0 ? -d : d;
                    if (p != 0 && d < fa.delta) {
                        // two rounded multiplies and one rounded add: no FMA
                        const float f = __fadd_rn(__fmul_rn(fa.a, (float)c), __fmul_rn(fa.oma, (float)p));
                        const uint32_t rr = (uint32_t)min((int)f, 65535);
                        o[j] = rr; l[j] = rr; h[j] = ((hh << 1) | 1u) & 0xFFu;
                    } else {
                        l[j] = c; h[j] = 1u;
                    }
                } else {
                    o[j] = (p != 0 && (int)__popc(hh & fa.l_mask) >= fa.m) ? p : 0u;
                    h[j] = (hh << 1) & 0xFFu;
                }
            }
            // the state sees the temporal stage alone: stored before the fill touches o[]
            if (vec) {
                if (nv) {
                    uint4 q;
                    q.x = l[0] | l[1] << 16; q.y = l[2] | l[3] << 16; q.z = l[4] | l[5] << 16; q.w = l[6] | l[7] << 16;
                    uint2 b;
                    b.x = h[0] | h[1] << 8 | h[2] << 16 | h[3] << 24;
                    b.y = h[4] | h[5] << 8 | h[6] << 16 | h[7] << 24;
                    *reinterpret_cast<uint4*>(F.last + i0) = q;
                    *reinterpret_cast<uint2*>(F.hist + i0) = b;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if ((uint32_t)j < nv) { F.last[i0 + j] = (uint16_t)l[j]; F.hist[i0 + j] = (uint8_t)h[j]; }
            }
        }
        if (FILL) {
            // a scan with the operator b ? b : a. Each lane reduces its 8 pixels; one ballot of "lane holds a non-zero" finds,
            // for every lane, the nearest such lane below it; the four waves meet in four LDS words behind one barrier.
            uint32_t run = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) run = o[j] ? o[j] : run;
            const unsigned long long m = __ballot(run != 0);
            const unsigned long long below = m & ((1ull << lane) - 1ull);
            const uint32_t prev = (uint32_t)__shfl((int)run, below ? 63 - __clzll((long long)below) : 0);
            const uint32_t wlast = (uint32_t)__shfl((int)run, m ? 63 - __clzll((long long)m) : 0);
            if (lane == 0) s_last[parity][wave] = m ? wlast : 0u;
            __syncthreads();
            uint32_t win = carry, mine = carry;
#pragma unroll
            for (uint32_t w = 0; w < 4; w++) {
                if (w == wave) mine = win;
                const uint32_t v = w < n_waves ? s_last[parity][w] : 0u;
                win = v ? v : win;
            }
            carry = win;
            uint32_t inc = below ? prev : mine;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (o[j] == 0) o[j] = inc; else inc = o[j];
            }
        }
        if (vec) {
            if (nv) {
                uint4 v;
                v.x = o[0] | o[1] << 16; v.y = o[2] | o[3] << 16; v.z = o[4] | o[5] << 16; v.w = o[6] | o[7] << 16;
                *reinterpret_cast<uint4*>(out + i0) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((uint32_t)j < nv) out[i0 + j] = (uint16_t)o[j];
        }
        if (COUNT) {
            // a pass is at most 2048 consecutive pixels: it touches the tile of its first pixel and at most the next one
            const uint32_t tile_a = (uint32_t)((row0 + c0) / kTilePoints);
            const uint64_t edge = ((uint64_t)tile_a + 1) * kTilePoints;
            uint32_t packed = 0;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((uint32_t)j < nv && o[j] != 0) packed += (i0 + j < edge) ? 1u : 0x10000u;
            packed = wave_sum32(packed);         // <= 512 in each half
            const uint32_t slot = tile_a - tile_first;
            if (lane == 0) {
                if ((packed & 0xFFFFu) && slot < (uint32_t)kFilterSlots) atomicAdd(&s_tiles[slot], packed & 0xFFFFu);
                if ((packed >> 16) && slot + 1 < (uint32_t)kFilterSlots) atomicAdd(&s_tiles[slot + 1], packed >> 16);
            }
        }
    }
    if (COUNT) {
        __syncthreads();
        if (threadIdx.x < kFilterSlots) {
            const uint32_t v = s_tiles[threadIdx.x];
            if (v) atomicAdd(&tile_kept[F.tile_base + tile_first + threadIdx.x], v);       // one per tile touched
        }
    }
}

}  // namespace

hipError_t launch_depth_filter(const FilterStream* d_tab, int n_streams, uint32_t max_rows, uint32_t max_width, bool temporal,
                               bool fill, const FilterPtrs& fp, const FilterArgs& fa, uint32_t* d_tile_kept, hipStream_t st)
{
    if (n_streams <= 0 || max_rows == 0 || max_width == 0) return hipSuccess;
    if (n_streams > PCS_MAX_STREAMS || (!temporal && !fill)) return hipErrorInvalidValue;
    const dim3 grid(max_rows, (unsigned)n_streams);
    // whole waves, as many as the widest row of the launch fills in one pass (at most the four of a 2048-pixel pass)
    const unsigned lanes = (max_width + kPointsPerLane - 1) / kPointsPerLane;
    const dim3 block(std::min<unsigned>(kBlockThreads, (lanes + 63u) & ~63u));
#define L(T, F, C) hipLaunchKernelGGL((pcs_depth_filter_kernel<T, F, C>), grid, block, 0, st, d_tab, fp, fa, d_tile_kept)
#define LC(T, F) do { if (d_tile_kept) L(T, F, true); else L(T, F, false); } while (0)
    if (temporal && fill) LC(true, true); else if (temporal) LC(true, false); else LC(false, true);
#undef LC
#undef L
    return hipGetLastError();
}

// ---- depth decimation (pcs_decimate_depth_device) ---------------------------------------------------------------------------------
// DESIGN.md §3 "Depth decimation": output pixel (r, c) of scale N is taken from the non-zero values of the source block
// in[N r + a][N c + b]: their lower median for N = 2, 3, floor(sum / count) for N >= 4, 0 when there is none. This project's own
// definition (modelled on librealsense's decimation block, parity with librealsense unpinned); tests/np_decimation.py restates it.
//
// Shape, from the filter's: a lane owns 8 consecutive OUTPUT pixels of one output row, that is 8 N consecutive source pixels of each
// of N source rows; a wave belongs to one output row; a workgroup is the whole waves the widest output row of the launch fills
// (a 640-pixel row: two), times as many rows as fit kDecimGroupLanes lanes; a wider row than one pass loops (nothing is carried). No
// LDS, no barrier. Source rows whose width is a multiple of 8, in a 16-byte aligned raster, are read as N 16-byte loads per lane and
// row; output rows whose width is a multiple of 8, in a 16-byte aligned raster, are written as one 16-byte store per lane; each side
// falls back to 2-byte accesses on its own, and so does the one lane whose 8 outputs straddle the end of a row that is read wide.
namespace {

#ifndef PCS_DECIMATE_GROUP_LANES
#define PCS_DECIMATE_GROUP_LANES 256          // (a build-time constant so that a lab build can measure others)
#endif
constexpr unsigned kDecimGroupLanes = PCS_DECIMATE_GROUP_LANES;
static_assert(kDecimGroupLanes >= 64 && kDecimGroupLanes <= 1024 && kDecimGroupLanes % 64 == 0, "whole waves");

__device__ __forceinline__ void cswap(uint32_t& a, uint32_t& b)
{
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo; b = hi;
}

// pixel p (a compile-time constant once unrolled) of a lane's slice of one source row: 8 N pixels held as 4 N packed words
template <int N>
__device__ __forceinline__ uint32_t slice_px(const uint32_t (&w)[4 * N], int p)
{
    return (p & 1) ? w[p >> 1] >> 16 : w[p >> 1] & 0xFFFFu;
}

// A lane's slice of one source row. wide: N aligned 16-byte loads. Otherwise 2-byte loads of the first n_px pixels, zeros behind
// them (zeros are invalid pixels, and they only reach outputs that are not stored).
template <int N>
__device__ __forceinline__ void load_slice(const uint16_t* p, bool wide, uint32_t n_px, uint32_t (&w)[4 * N])
{
    if (wide) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4 * N; q++) {
            const uint32_t lo = (uint32_t)(2 * q) < n_px ? p[2 * q] : 0u;
            const uint32_t hi = (uint32_t)(2 * q + 1) < n_px ? p[2 * q + 1] : 0u;
            w[q] = lo | hi << 16;
        }
    }
}

// N = 2, 3: the block is held (N x N uint4 per lane), zeros become 65536 so that they sort last, a fixed compare-exchange network
// sorts the 4 or 9 values and a chain of selects picks element (k - 1) >> 1 — no register array is indexed by a run-time value.
template <int N>
__device__ __forceinline__ void decimate_median(const uint16_t* src, size_t pitch, bool wide, uint32_t n_px, uint32_t (&o)[8])
{
    static_assert(N == 2 || N == 3, "the median scales");
    uint32_t w[N][4 * N];
#pragma unroll
    for (int a = 0; a < N; a++) load_slice<N>(src + a * pitch, wide, n_px, w[a]);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t v[N * N], k = 0;
#pragma unroll
        for (int a = 0; a < N; a++)
#pragma unroll
            for (int b = 0; b < N; b++) {
                const uint32_t x = slice_px<N>(w[a], N * j + b);
                k += x != 0 ? 1u : 0u;
                v[a * N + b] = x != 0 ? x : 65536u;
            }
        uint32_t m;
        if (N == 2) {
            cswap(v[0], v[1]); cswap(v[2], v[3]); cswap(v[0], v[2]); cswap(v[1], v[3]); cswap(v[1], v[2]);
            m = k >= 3 ? v[1] : v[0];                                   // (k - 1) >> 1 is 0 for k = 1, 2 and 1 for k = 3, 4
        } else {
            // 25 compare-exchanges in 7 layers (a 0-1-principle check over all 512 inputs passes)
            cswap(v[0], v[3]); cswap(v[1], v[7]); cswap(v[2], v[5]); cswap(v[4], v[8]);
            cswap(v[0], v[7]); cswap(v[2], v[4]); cswap(v[3], v[8]); cswap(v[5], v[6]);
            cswap(v[0], v[2]); cswap(v[1], v[3]); cswap(v[4], v[5]); cswap(v[7], v[8]);
            cswap(v[1], v[4]); cswap(v[3], v[6]); cswap(v[5], v[7]);
            cswap(v[0], v[1]); cswap(v[2], v[4]); cswap(v[3], v[5]); cswap(v[6], v[8]);
            cswap(v[2], v[3]); cswap(v[4], v[5]); cswap(v[6], v[7]);
            cswap(v[1], v[2]); cswap(v[3], v[4]); cswap(v[5], v[6]);
            const uint32_t idx = (k - 1u) >> 1;                        // 0..4 for k = 1..9
            m = v[0];
            m = idx == 1u ? v[1] : m;
            m = idx == 2u ? v[2] : m;
            m = idx == 3u ? v[3] : m;
            m = idx == 4u ? v[4] : m;
        }
        o[j] = k != 0 ? m : 0u;
    }
}

// N >= 4: the block is not held (N = 8 would be 64 uint4 per lane, and left to itself the compiler does hold it: 256 VGPRs). Eight
// 32-bit sums (at most 64 x 65535) and eight counts grow source row by source row over two slices that take turns: while one is
// added the other's loads are in flight. The row loop is kept a loop for that; everything inside it unrolls. The division is the
// integer one.
template <int N>
__device__ __forceinline__ void accumulate_slice(const uint32_t (&w)[4 * N], uint32_t (&sum)[8], uint32_t (&cnt)[8])
{
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int b = 0; b < N; b++) {
            const uint32_t x = slice_px<N>(w, N * j + b);
            sum[j] += x;
            cnt[j] += x != 0 ? 1u : 0u;
        }
}

template <int N>
__device__ __forceinline__ void decimate_mean(const uint16_t* src, size_t pitch, bool wide, uint32_t n_px, uint32_t (&o)[8])
{
    static_assert(N >= 4 && N <= 8, "the mean scales");
    uint32_t sum[8], cnt[8], even[4 * N], odd[4 * N];
#pragma unroll
    for (int j = 0; j < 8; j++) { sum[j] = 0; cnt[j] = 0; }
    load_slice<N>(src, wide, n_px, even);
#pragma unroll 1
    for (int a = 0; a < N; a += 2) {
        if (a + 1 < N) load_slice<N>(src + (size_t)(a + 1) * pitch, wide, n_px, odd);
        accumulate_slice<N>(even, sum, cnt);
        if (a + 2 < N) load_slice<N>(src + (size_t)(a + 2) * pitch, wide, n_px, even);
        if (a + 1 < N) accumulate_slice<N>(odd, sum, cnt);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = cnt[j] != 0 ? sum[j] / cnt[j] : 0u;
}

template <int N>
__global__ __launch_bounds__(kDecimGroupLanes > (unsigned)kBlockThreads ? kDecimGroupLanes : (unsigned)kBlockThreads)
void pcs_decimate_depth_kernel(DecimArgs da)
{
    const int s = blockIdx.y;
    const uint32_t Ws = da.Ws[s], Wd = da.Wd[s];
    const uint32_t r = blockIdx.x * blockDim.y + threadIdx.y;          // (blockDim.x is whole waves: a wave has one r)
    if (r >= da.Hd[s]) return;
    const uint16_t* in = da.in[s];
    uint16_t* out = da.out[s];
    const bool wide_in = (Ws & 7u) == 0 && (((uintptr_t)in) & 15u) == 0;
    const bool wide_out = (Wd & 7u) == 0 && (((uintptr_t)out) & 15u) == 0;
    const uint16_t* src_row = in + (size_t)r * N * Ws;
    uint16_t* out_row = out + (size_t)r * Wd;
    const uint32_t pass_pixels = blockDim.x * kPointsPerLane;
    for (uint32_t c0 = 0; c0 < Wd; c0 += pass_pixels) {
        const uint32_t col = c0 + threadIdx.x * kPointsPerLane;
        if (col >= Wd) continue;
        const uint32_t nv = min((uint32_t)kPointsPerLane, Wd - col);    // wide_out: always 8
        const uint16_t* src = src_row + (size_t)col * N;
        uint32_t o[8];
        if constexpr (N <= 3) decimate_median<N>(src, Ws, wide_in && nv == 8u, nv * N, o);
        else decimate_mean<N>(src, Ws, wide_in && nv == 8u, nv * N, o);
        if (wide_out) {
            uint4 v;
            v.x = o[0] | o[1] << 16; v.y = o[2] | o[3] << 16; v.z = o[4] | o[5] << 16; v.w = o[6] | o[7] << 16;
            *reinterpret_cast<uint4*>(out_row + col) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((uint32_t)j < nv) out_row[col + j] = (uint16_t)o[j];
        }
    }
}

}  // namespace

hipError_t launch_decimate_depth(int scale, int n_streams, uint32_t max_rows, uint32_t max_width, const DecimArgs& da, hipStream_t st)
{
    if (scale < 2 || scale > 8 || n_streams < 0 || n_streams > PCS_MAX_STREAMS) return hipErrorInvalidValue;
    if (n_streams == 0 || max_rows == 0 || max_width == 0) return hipSuccess;
    // whole waves, as many as the widest output row fills in one pass (at most four); then as many rows as fit the group
    const unsigned lanes = (max_width + kPointsPerLane - 1) / kPointsPerLane;
    const unsigned bx = std::min<unsigned>(kBlockThreads, (lanes + 63u) & ~63u);
    const unsigned by = std::max(1u, kDecimGroupLanes / bx);
    const dim3 grid((max_rows + by - 1) / by, (unsigned)n_streams), block(bx, by);
#define L(N) case N: hipLaunchKernelGGL((pcs_decimate_depth_kernel<N>), grid, block, 0, st, da); break
    switch (scale) { L(2); L(3); L(4); L(5); L(6); L(7); L(8); }
#undef L
    return hipGetLastError();
}

// ---- spatial filter (pcs_spatial_filter_depth_device) ------------------------------------------------------------------------------
// DESIGN.md §3 "Spatial filter": an edge-preserving recursive smoother that is a recurrence along ONE line at a time - every row left
// to right and right to left (with the bounded hole fill), then every column down and up, `iterations` times. This project's own
// definition (modelled on librealsense's spatial filter, parity with librealsense unpinned); tests/np_spatial_filter.py restates it.
//
// Shape: one lane owns one line and walks it in both directions, so in place is safe (a lane reads and writes its own line only; the
// second direction reads what the same lane stored, in program order). A workgroup is one wave: 8 x 720p is about 90 row waves and 160
// column waves for 1024 SIMDs, so single waves spread furthest, and with a SIMD to itself a wave issues one vector instruction every
// four cycles whether or not it depends on the one before - a pass costs (instructions per step) x 4 cycles x (2 x line length), and
// the only lever is the instruction count of the step. The recurrence stays in fp32 (every Z16 value, difference and rounded blend is
// an exact float): compares, blend and floor never leave the float pipe; values are converted once when they are unpacked and once
// when they are packed.
//   rows     a lane's row is contiguous: it takes 8 pixels per 16-byte load / store when the width is a multiple of 8 and both rasters
//            are 16-byte aligned (every row segment is then aligned), 2-byte accesses otherwise. The 64 lanes of a load touch 64
//            different 128-byte lines, each line serves 8 consecutive loads of its lane (64 x 128 B = 8 KiB per wave: it stays in the
//            vector L1), and kSpatialRowAhead chunks are requested ahead of the walk, so the walk never waits on them. No LDS: staging
//            128-byte segments through LDS coalesces the global accesses but costs two LDS instructions per pixel and direction in the
//            one instruction stream that is the bottleneck.
//   columns  lane = column, so every access of a wave is one coalesced 128-byte row segment; 2-byte accesses always (any width, any
//            2-byte alignment), kSpatialColAhead rows requested ahead of the walk.
// A line's first pixel needs no special case: from the state (v0 = 0, nothing filled) a step leaves any pixel as it is and takes it
// as v0.
namespace {

constexpr int kSpatialRowAhead = 4;           // 8-pixel chunks of a row in flight ahead of the walk
constexpr int kSpatialColAhead = 32;          // rows of a column in flight ahead of the walk

struct SpatialConst { float a, oma, delta; uint32_t radius; };

// One step of a line pass: v1 is the pixel, (v0, left) the state; returns what the pixel becomes.
//   blend   v0, v1 valid and 1 <= |v1 - v0| <= delta: fl(fl(fl(a v1) + fl(oma v0)) + 0.5f), truncated - floorf for these positive
//           values. The definition's min(.., 65535) cannot fire: a + oma <= 1 + 2^-25, two rounded products and a rounded sum of
//           values <= 65535 stay below 65535.01, plus 0.5f below 65536 - so it is not computed. A blend is never 0 either (it is at
//           least (1 - 2^-23) min(v0, v1) + 0.5, truncated), so "v1 is 0" after the blend is "the pixel was 0".
//   fill    (rows only) the pixel is 0, v0 is valid and fewer than `radius` pixels of this gap were filled: it takes v0.
template <bool FILL>
__device__ __forceinline__ float spatial_step(float v1, float& v0, uint32_t& left, const SpatialConst& k)
{
    const float d = fabsf(__fsub_rn(v1, v0));
    // v0, v1 and d are non-negative whole numbers: all three are >= 1 exactly when their minimum is not 0
    const bool blend = fminf(fminf(v0, v1), d) != 0.0f && d <= k.delta;
    // two rounded multiplies and two rounded adds: no FMA
    const float f = __fadd_rn(__fmul_rn(k.a, v1), __fmul_rn(k.oma, v0));
    float r = blend ? floorf(__fadd_rn(f, 0.5f)) : v1;
    if (FILL) {
        // left: how many more pixels the gap at hand may take - hole_radius - run while v0 is valid, 0 before a line's first valid
        // pixel and once a gap was left open (v0 is 0 from there to the next valid pixel), so "v0 != 0 and run < hole_radius" is
        // "left != 0"
        const bool valid = v1 != 0.0f;
        const bool fill = !valid && left != 0u;
        left = valid ? k.radius : left - (fill ? 1u : 0u);
        r = fill ? v0 : r;
    }
    v0 = r;
    return r;
}

// 8 consecutive pixels of a row as four packed words. VEC: one aligned 16-byte access; otherwise the first n (1..8) pixels by 2-byte
// accesses (the words' other halves are zero on a load and ignored on a store). FULL: n is 8, nothing is tested.
template <bool VEC, bool FULL>
__device__ __forceinline__ void load_px8(const uint16_t* p, uint32_t n, uint32_t (&w)[4])
{
    if (VEC) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t lo = (FULL || (uint32_t)(2 * q) < n) ? p[2 * q] : 0u;
            const uint32_t hi = (FULL || (uint32_t)(2 * q + 1) < n) ? p[2 * q + 1] : 0u;
            w[q] = lo | hi << 16;
        }
    }
}
template <bool VEC, bool FULL>
__device__ __forceinline__ void store_px8(uint16_t* p, uint32_t n, const uint32_t (&w)[4])
{
    if (VEC) {
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (FULL || (uint32_t)j < n) p[j] = (uint16_t)((j & 1) ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu);
    }
}

// The n (FULL: 8) pixels of one chunk through the recurrence, from the first (forward) or from the last (BACK); packed in, packed out.
template <bool BACK, bool FULL>
__device__ __forceinline__ void spatial_walk8(uint32_t (&w)[4], uint32_t n, float& v0, uint32_t& left, const SpatialConst& k)
{
    float x[8];
#pragma unroll
    for (int q = 0; q < 4; q++) { x[2 * q] = (float)(w[q] & 0xFFFFu); x[2 * q + 1] = (float)(w[q] >> 16); }
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const int p = BACK ? 7 - t : t;
        if (FULL || (uint32_t)p < n) x[p] = spatial_step<true>(x[p], v0, left, k);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) w[q] = (uint32_t)x[2 * q] | (uint32_t)x[2 * q + 1] << 16;
}

// One direction over one row. Chunk i of the sweep is 8 i pixels from the row's start (forward) or from its end (BACK), so the one
// short chunk of a ragged row (VEC: there is none) is always the last of the sweep. src may be dst: a chunk is requested
// kSpatialRowAhead chunks before it is walked and stored, and no chunk is requested twice. The main loop runs while the chunks walked
// AND the chunks requested are whole ones: neither it nor the requests ahead of it have a condition in them, so the compiler's wait
// counts leave the requests in flight (with a conditional load anywhere on the way in, it waits for all of them at the top of the
// loop); the tail loop (fewer than 2 kSpatialRowAhead chunks) tests everything. Every condition is the same for all lanes of the
// wave (one stream, one width).
template <bool BACK, bool VEC>
__device__ __forceinline__ void spatial_sweep_row(const uint16_t* src, uint16_t* dst, uint32_t W, const SpatialConst& k)
{
    constexpr uint32_t K = kSpatialRowAhead;
    const uint32_t nch = (W + 7u) >> 3, nfull = W >> 3;
    const auto col_of = [&](uint32_t i) { return BACK ? (W >= 8u * (i + 1u) ? W - 8u * (i + 1u) : 0u) : 8u * i; };
    const auto n_of = [&](uint32_t i) { return min(8u, W - 8u * i); };
    uint32_t ring[K][4];
    float v0 = 0.0f;
    uint32_t left = 0;
    uint32_t i0 = 0;
    if (2u * K <= nfull) {
#pragma unroll
        for (uint32_t j = 0; j < K; j++) load_px8<VEC, true>(src + col_of(j), 8u, ring[j]);
        for (; i0 + 2u * K <= nfull; i0 += K) {
#pragma unroll
            for (uint32_t j = 0; j < K; j++) {
                spatial_walk8<BACK, true>(ring[j], 8u, v0, left, k);
                store_px8<VEC, true>(dst + col_of(i0 + j), 8u, ring[j]);
                load_px8<VEC, true>(src + col_of(i0 + j + K), 8u, ring[j]);
            }
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < K; j++) {
#pragma unroll
            for (int q = 0; q < 4; q++) ring[j][q] = 0;
            if (j < nch) load_px8<VEC, false>(src + col_of(j), n_of(j), ring[j]);
        }
    }
    for (; i0 < nch; i0 += K) {
#pragma unroll
        for (uint32_t j = 0; j < K; j++) {
            const uint32_t i = i0 + j;
            if (i >= nch) break;
            spatial_walk8<BACK, false>(ring[j], n_of(i), v0, left, k);
            store_px8<VEC, false>(dst + col_of(i), n_of(i), ring[j]);
            if (i + K < nch) load_px8<VEC, false>(src + col_of(i + K), n_of(i + K), ring[j]);
        }
    }
}

__global__ __launch_bounds__(64)
void pcs_spatial_rows_kernel(SpatialArgs sa)
{
    const int s = blockIdx.y;
    const uint32_t W = sa.W[s];
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= sa.H[s]) return;                                   // (no barrier anywhere: lanes past the last row just leave)
    const SpatialConst k{sa.a, sa.oma, sa.delta, sa.radius};
    const size_t row0 = (size_t)r * W;
    const uint16_t* in = sa.in[s] + row0;
    uint16_t* out = sa.out[s] + row0;
    if ((W & 7u) == 0 && ((((uintptr_t)sa.in[s]) | ((uintptr_t)sa.out[s])) & 15u) == 0) {
        spatial_sweep_row<false, true>(in, out, W, k);
        spatial_sweep_row<true, true>(out, out, W, k);
    } else {
        spatial_sweep_row<false, false>(in, out, W, k);
        spatial_sweep_row<true, false>(out, out, W, k);
    }
}

// One direction over one column: row i of the sweep is raster row i (down) or H - 1 - i (BACK). Byte offsets from the raster's base
// fit 32 bits (a context's raster has fewer than 2^31 pixels), so the base stays scalar and a step's address is one 32-bit add. Main
// loop and tail loop as in the row sweep.
template <bool BACK>
__device__ __forceinline__ void spatial_sweep_col(uint16_t* x, uint32_t W, uint32_t H, uint32_t c, const SpatialConst& k)
{
    constexpr uint32_t K = kSpatialColAhead;
    const auto off_of = [&](uint32_t i) { return ((BACK ? H - 1u - i : i) * W + c) * 2u; };
    const auto px = [&](uint32_t off) -> uint16_t& { return *reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(x) + off); };
    uint32_t ring[K];
    float v0 = 0.0f;
    uint32_t left = 0;
    uint32_t i0 = 0;
    if (2u * K <= H) {
#pragma unroll
        for (uint32_t j = 0; j < K; j++) ring[j] = px(off_of(j));
        for (; i0 + 2u * K <= H; i0 += K) {
#pragma unroll
            for (uint32_t j = 0; j < K; j++) {
                px(off_of(i0 + j)) = (uint16_t)(uint32_t)spatial_step<false>((float)ring[j], v0, left, k);
                ring[j] = px(off_of(i0 + j + K));
            }
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < K; j++) ring[j] = j < H ? px(off_of(j)) : 0u;
    }
    for (; i0 < H; i0 += K) {
#pragma unroll
        for (uint32_t j = 0; j < K; j++) {
            const uint32_t i = i0 + j;
            if (i >= H) break;
            px(off_of(i)) = (uint16_t)(uint32_t)spatial_step<false>((float)ring[j], v0, left, k);
            if (i + K < H) ring[j] = px(off_of(i + K));
        }
    }
}

__global__ __launch_bounds__(64)
void pcs_spatial_cols_kernel(SpatialArgs sa)
{
    const int s = blockIdx.y;
    const uint32_t W = sa.W[s], H = sa.H[s];
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= W) return;
    const SpatialConst k{sa.a, sa.oma, sa.delta, sa.radius};
    spatial_sweep_col<false>(sa.out[s], W, H, c, k);            // (the column launches always run in place on the output)
    spatial_sweep_col<true>(sa.out[s], W, H, c, k);
}

}  // namespace

hipError_t launch_spatial_filter(int n_streams, int iterations, uint32_t max_rows, uint32_t max_width, const SpatialArgs& sa, hipStream_t st)
{
    if (n_streams < 0 || n_streams > PCS_MAX_STREAMS || iterations < 1) return hipErrorInvalidValue;
    if (n_streams == 0 || max_rows == 0 || max_width == 0) return hipSuccess;
    const dim3 block(64), row_grid((max_rows + 63u) / 64u, (unsigned)n_streams), col_grid((max_width + 63u) / 64u, (unsigned)n_streams);
    SpatialArgs in_place = sa;
    for (int s = 0; s < n_streams; s++) in_place.in[s] = sa.out[s];
    for (int it = 0; it < iterations; it++) {
        hipLaunchKernelGGL(pcs_spatial_rows_kernel, row_grid, block, 0, st, it == 0 ? sa : in_place);
        hipLaunchKernelGGL(pcs_spatial_cols_kernel, col_grid, block, 0, st, in_place);
    }
    return hipGetLastError();
}

}  // namespace pcs
