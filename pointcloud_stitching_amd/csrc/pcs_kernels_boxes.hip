// pcs_kernels_boxes.hip — oriented object boxes: per object of pcs_cluster_objects_device* the count, the first and second moments,
// three orthonormal axes from the covariance, a rank, and the extents of the members along those axes (pcs_object_boxes_device;
// DESIGN.md section 3 "Object boxes" and section 5). Not in the reference: the definition is this project's own. The inputs are the
// tracker's: the payload, object_of, *n_objects, max_objects; m = *n_objects clamped to 0..max_objects.
//   clear      the m accumulators of the workspace (16 int64 words per object, ten of them used) to zero
//   moments    one lane per record, a tile of 2048 per workgroup: count, sum p and sum p p^T per object. A wave's lanes are grouped
//              by k as pcs_cluster_accumulate_kernel groups them; the first object a wave meets is HELD over the tile in per-lane
//              partials, reduced once, combined over the workgroup's waves through LDS and flushed once per tile and word; every
//              other group is reduced across the wave at once. One 64-bit add without return per word and group, lanes 0..9 a word
//              each; a zero addend is not sent.
//   axes       one lane per k < m: pcs_boxes_math.h on the ten sums; the entry written whole with its extent words at their
//              identities (INT_MAX / INT_MIN; 0 / 0 for an entry without a member, which the extents launch never touches)
//   extents    one lane per record again: the group's nine axis shorts fetched once (wave-uniform), three int32 projections per
//              member, minima and maxima held / reduced as the sums are, conditional atomicMin / atomicMax on the entry's six words
// Properties:
//   32 bits up to the flush   a product p = a b (|p| <= 2^30) is carried as p & 0xFFFF (0..65535) and p >> 16 (|.| <= 2^14), each
//              summed in int32: a lane's eight records reach 2^19 and 2^17, a wave 2^25 and 2^23, the workgroup 2^27 and 2^25. The
//              flush recombines hi * 65536 + lo in 64 bits. Every word of a round is then a 32-bit wave_sum.
//   determinism   integer sums, minima and maxima alone cross lanes; the doubles run in one lane per object on exact inputs.
//   bounds     a record index stays below the clamped count, an object index below m <= max_objects. No scratch.

#include <algorithm>
#include <climits>

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"
#include "pcs_boxes_math.h"

namespace pcs {

namespace {

static_assert(sizeof(pcs_object_box) == 128, "pcs_object_box is 128 bytes");
static_assert(sizeof(pcs_object_box) == kBoxWsWords * sizeof(long long), "the workspace has an entry's bytes per object");

constexpr int kWaves = kBlockThreads / 64;
constexpr int kMomentWords = 10;            // count, sum x y z, sum xx xy xz yy yz zz

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint32_t clamped_count(const int32_t* d_n, uint32_t n_host, uint32_t capacity)
{
    if (!d_n) return n_host;
    const int32_t v = *d_n;
    return v < 0 ? 0u : min((uint32_t)v, capacity);
}

// Wavefront-wide minimum / maximum (wave-uniform): wave_inclusive_scan's moves with the fold's identity where a lane has no source.
__device__ __forceinline__ int wave_min(int x)
{
    int v = x;
    v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ int wave_max(int x)
{
    int v = x;
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v, 63);
}

// ---- clear ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_boxes_clear_kernel(const int32_t* __restrict__ d_m, uint32_t max_objects, long long* __restrict__ acc)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i < clamped_count(d_m, 0u, max_objects) * kBoxWsWords) acc[i] = 0ll;
}

// ---- moments ----------------------------------------------------------------------------------------
// A lane's sixteen 32-bit partials: 0 the count, 1..3 the coordinate sums, 4..9 the products' low 16 bits, 10..15 their high parts.
__device__ __forceinline__ void moment_terms(bool in, const Xyz& p, int (&t)[16])
{
    const int pr[6] = {p.x * p.x, p.x * p.y, p.x * p.z, p.y * p.y, p.y * p.z, p.z * p.z};
    t[0] = in ? 1 : 0;
    t[1] = in ? p.x : 0; t[2] = in ? p.y : 0; t[3] = in ? p.z : 0;
#pragma unroll
    for (int q = 0; q < 6; q++) {
        t[4 + q] = in ? (pr[q] & 0xFFFF) : 0;
        t[10 + q] = in ? (pr[q] >> 16) : 0;
    }
}

// lane j's 64-bit word (j < kMomentWords) of sixteen wave-uniform partials, the products recombined (a select chain: a register
// array indexed by the lane would live in scratch)
__device__ __forceinline__ long long moment_word_of_lane(const int (&t)[16])
{
    long long v = 0ll;
#pragma unroll
    for (int q = 0; q < 4; q++) v = lane_id() == (uint32_t)q ? (long long)t[q] : v;
#pragma unroll
    for (int q = 0; q < 6; q++) v = lane_id() == (uint32_t)(4 + q) ? (long long)t[10 + q] * 65536 + (long long)t[4 + q] : v;
    return v;
}

__device__ __forceinline__ void add_word(long long* word, long long v)
{
    if (v != 0ll)
        (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(word), (unsigned long long)v, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_boxes_moments_kernel(const int16_t* __restrict__ in, const int32_t* __restrict__ d_n, uint32_t n_host, uint32_t capacity,
                              const int32_t* __restrict__ object_of, const int32_t* __restrict__ d_m, uint32_t max_objects,
                              long long* __restrict__ acc)
{
    __shared__ long long part[kWaves][kMomentWords];
    __shared__ int held_of[kWaves];
    const uint32_t n = clamped_count(d_n, n_host, capacity);
    const uint32_t m = clamped_count(d_m, 0u, max_objects);
    int held = -1;                                           // wave-uniform
    int h[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t i = (blockIdx.x * kPointsPerLane + c) * kBlockThreads + threadIdx.x;
        const bool live = i < n;
        if (!__ballot(live)) break;                          // (records ascend: nothing live behind this either)
        int k = -1;
        Xyz p{0, 0, 0};
        if (live) {
            k = object_of[i];
            if ((uint32_t)k < m) p = load_xyz(in, i);
        }
        const bool counts = live && (uint32_t)k < m;         // -1 and everything at or beyond m: ignored
        unsigned long long todo = __ballot(counts);
        if (held < 0 && todo) held = __builtin_amdgcn_readlane(k, __ffsll((long long)todo) - 1);
        const bool mine = counts && k == held;
        {
            int t[16];
            moment_terms(mine, p, t);
#pragma unroll
            for (int q = 0; q < 16; q++) h[q] += t[q];
        }
        todo &= ~__ballot(mine);
        while (todo) {                                       // wave-uniform: one round per other object among the wave's lanes
            const int k0 = __builtin_amdgcn_readlane(k, __ffsll((long long)todo) - 1);
            const bool in_group = counts && k == k0;
            int t[16];
            moment_terms(in_group, p, t);
#pragma unroll
            for (int q = 0; q < 16; q++) t[q] = (int)wave_sum((uint32_t)t[q]);
            const long long w = moment_word_of_lane(t);
            if (lane_id() < (uint32_t)kMomentWords) add_word(acc + (size_t)k0 * kBoxWsWords + lane_id(), w);
            todo &= ~__ballot(in_group);
        }
    }
#pragma unroll
    for (int q = 0; q < 16; q++) h[q] = (int)wave_sum((uint32_t)h[q]);
    const uint32_t wave = threadIdx.x >> 6, j = lane_id();
    {
        const long long w = moment_word_of_lane(h);
        if (j < (uint32_t)kMomentWords) part[wave][j] = w;
        if (j == 0u) held_of[wave] = held;
    }
    __syncthreads();
    if (j >= (uint32_t)kMomentWords) return;
    const int h0 = held_of[0];
    if (wave == 0u) {
        if (h0 < 0) return;
        long long total = part[0][j];
        for (int w = 1; w < kWaves; w++)
            if (held_of[w] == h0) total += part[w][j];
        add_word(acc + (size_t)h0 * kBoxWsWords + j, total);
    } else {
        const int hw = held_of[wave];
        if (hw >= 0 && hw != h0) add_word(acc + (size_t)hw * kBoxWsWords + j, part[wave][j]);
    }
}

// ---- axes -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_boxes_axes_kernel(const int32_t* __restrict__ d_m, uint32_t max_objects, const long long* __restrict__ acc,
                           pcs_object_box* __restrict__ boxes)
{
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    if (k >= clamped_count(d_m, 0u, max_objects)) return;
    const long long* a = acc + (size_t)k * kBoxWsWords;
    const long long count = a[0];
    const long long s1[3] = {a[1], a[2], a[3]};
    const long long m2[6] = {a[4], a[5], a[6], a[7], a[8], a[9]};
    const BoxAxes ax = box_axes(count, s1, m2);
    // the entry as its sixteen little-endian 64-bit words (a local struct of shorts would live in scratch)
    const auto s16 = [](int16_t v) { return (unsigned long long)(uint16_t)v; };
    const auto s32 = [](int v) { return (unsigned long long)(uint32_t)v; };
    const int lo = count > 0 ? INT_MAX : 0, hi = count > 0 ? INT_MIN : 0;
    unsigned long long* o = reinterpret_cast<unsigned long long*>(boxes + k);
    o[0] = (unsigned long long)count;
    o[1] = (unsigned long long)s1[0]; o[2] = (unsigned long long)s1[1]; o[3] = (unsigned long long)s1[2];
    o[4] = (unsigned long long)m2[0]; o[5] = (unsigned long long)m2[1]; o[6] = (unsigned long long)m2[2];
    o[7] = (unsigned long long)m2[3]; o[8] = (unsigned long long)m2[4]; o[9] = (unsigned long long)m2[5];
    o[10] = s16(ax.a00) | s16(ax.a01) << 16 | s16(ax.a02) << 32 | s16(ax.a10) << 48;
    o[11] = s16(ax.a11) | s16(ax.a12) << 16 | s16(ax.a20) << 32 | s16(ax.a21) << 48;
    o[12] = s16(ax.a22) | s16(ax.rank) << 16 | s32(lo) << 32;       // axis[2][2], rank, ext_lo[0]
    o[13] = s32(lo) | s32(lo) << 32;                                // ext_lo[1], ext_lo[2]
    o[14] = s32(hi) | s32(hi) << 32;                                // ext_hi[0], ext_hi[1]
    o[15] = s32(hi);                                                // ext_hi[2], reserved 0
}

// ---- extents ----------------------------------------------------------------------------------------
struct AxisShorts { int a[9]; };

// the nine axis shorts of entry k (k wave-uniform: one fetch per group)
__device__ __forceinline__ AxisShorts load_axes(const pcs_object_box* boxes, int k)
{
    const int16_t* s = &boxes[k].axis[0][0];
    AxisShorts r;
#pragma unroll
    for (int q = 0; q < 9; q++) r.a[q] = s[q];
    return r;
}

// word j of an entry's six: 0..2 ext_lo (minimum), 3..5 ext_hi (maximum). A value that the word already meets is not sent.
__device__ __forceinline__ void flush_extent(pcs_object_box* b, uint32_t j, int v)
{
    if (j < 3u) {
        if (__hip_atomic_load(b->ext_lo + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(b->ext_lo + j, v);
    } else {
        if (__hip_atomic_load(b->ext_hi + (j - 3u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(b->ext_hi + (j - 3u), v);
    }
}

__device__ __forceinline__ int extent_word_of_lane(const int (&t)[6])
{
    int v = 0;
#pragma unroll
    for (int q = 0; q < 6; q++) v = lane_id() == (uint32_t)q ? t[q] : v;
    return v;
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_boxes_extents_kernel(const int16_t* __restrict__ in, const int32_t* __restrict__ d_n, uint32_t n_host, uint32_t capacity,
                              const int32_t* __restrict__ object_of, const int32_t* __restrict__ d_m, uint32_t max_objects,
                              pcs_object_box* boxes)
{
    __shared__ int part[kWaves][6];
    __shared__ int held_of[kWaves];
    const uint32_t n = clamped_count(d_n, n_host, capacity);
    const uint32_t m = clamped_count(d_m, 0u, max_objects);
    int held = -1;                                           // wave-uniform
    AxisShorts ha{};
    int h[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t i = (blockIdx.x * kPointsPerLane + c) * kBlockThreads + threadIdx.x;
        const bool live = i < n;
        if (!__ballot(live)) break;
        int k = -1;
        Xyz p{0, 0, 0};
        if (live) {
            k = object_of[i];
            if ((uint32_t)k < m) p = load_xyz(in, i);
        }
        const bool counts = live && (uint32_t)k < m;
        unsigned long long todo = __ballot(counts);
        if (held < 0 && todo) {
            held = __builtin_amdgcn_readlane(k, __ffsll((long long)todo) - 1);
            ha = load_axes(boxes, held);
        }
        const bool mine = counts && k == held;
        if (mine) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int d = box_project(ha.a[3 * a], ha.a[3 * a + 1], ha.a[3 * a + 2], p.x, p.y, p.z);
                h[a] = min(h[a], d);
                h[3 + a] = max(h[3 + a], d);
            }
        }
        todo &= ~__ballot(mine);
        while (todo) {
            const int k0 = __builtin_amdgcn_readlane(k, __ffsll((long long)todo) - 1);
            const bool in_group = counts && k == k0;
            const AxisShorts ga = load_axes(boxes, k0);
            int t[6];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int d = box_project(ga.a[3 * a], ga.a[3 * a + 1], ga.a[3 * a + 2], p.x, p.y, p.z);
                t[a] = wave_min(in_group ? d : INT_MAX);
                t[3 + a] = wave_max(in_group ? d : INT_MIN);
            }
            const int w = extent_word_of_lane(t);
            if (lane_id() < 6u) flush_extent(boxes + k0, lane_id(), w);
            todo &= ~__ballot(in_group);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        h[a] = wave_min(h[a]);
        h[3 + a] = wave_max(h[3 + a]);
    }
    const uint32_t wave = threadIdx.x >> 6, j = lane_id();
    {
        const int w = extent_word_of_lane(h);
        if (j < 6u) part[wave][j] = w;
        if (j == 0u) held_of[wave] = held;
    }
    __syncthreads();
    if (j >= 6u) return;
    const int h0 = held_of[0];
    if (wave == 0u) {
        if (h0 < 0) return;
        int total = part[0][j];
        for (int w = 1; w < kWaves; w++) {
            if (held_of[w] != h0) continue;
            const int o = part[w][j];
            total = j < 3u ? min(total, o) : max(total, o);
        }
        flush_extent(boxes + h0, j, total);
    } else {
        const int hw = held_of[wave];
        if (hw >= 0 && hw != h0) flush_extent(boxes + hw, j, part[wave][j]);
    }
}

dim3 grid_over(uint32_t n) { return dim3((std::max(n, 1u) + kBlockThreads - 1) / kBlockThreads); }
dim3 tiles_over(uint32_t n) { return dim3((std::max(n, 1u) + kTilePoints - 1) / kTilePoints); }

bool bad_records(const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity, const int32_t* d_object_of,
                 const int32_t* d_n_objects, uint32_t max_objects)
{
    return !d_n_objects || max_objects > (uint32_t)PCS_CLUSTER_OBJECTS_MAX || (capacity && (!d_in || !d_object_of)) ||
           (!d_n_points && n_points > capacity);
}

}  // namespace

hipError_t launch_boxes_clear(const int32_t* d_n_objects, uint32_t max_objects, void* d_ws, hipStream_t st)
{
    if (!d_n_objects || max_objects > (uint32_t)PCS_CLUSTER_OBJECTS_MAX || (max_objects && !d_ws)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_boxes_clear_kernel, grid_over(max_objects * kBoxWsWords), dim3(kBlockThreads), 0, st, d_n_objects, max_objects,
                       static_cast<long long*>(d_ws));
    return hipGetLastError();
}

hipError_t launch_boxes_moments(const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                const int32_t* d_object_of, const int32_t* d_n_objects, uint32_t max_objects, void* d_ws, hipStream_t st)
{
    if (bad_records(d_in, n_points, d_n_points, capacity, d_object_of, d_n_objects, max_objects) || (max_objects && !d_ws))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_boxes_moments_kernel, tiles_over(capacity), dim3(kBlockThreads), 0, st, d_in, d_n_points, n_points, capacity,
                       d_object_of, d_n_objects, max_objects, static_cast<long long*>(d_ws));
    return hipGetLastError();
}

hipError_t launch_boxes_axes(const int32_t* d_n_objects, uint32_t max_objects, const void* d_ws, pcs_object_box* d_boxes, hipStream_t st)
{
    if (!d_n_objects || max_objects > (uint32_t)PCS_CLUSTER_OBJECTS_MAX || (max_objects && (!d_ws || !d_boxes)) || ((uintptr_t)d_boxes & 7u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_boxes_axes_kernel, grid_over(max_objects), dim3(kBlockThreads), 0, st, d_n_objects, max_objects,
                       static_cast<const long long*>(d_ws), d_boxes);
    return hipGetLastError();
}

hipError_t launch_boxes_extents(const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                const int32_t* d_object_of, const int32_t* d_n_objects, uint32_t max_objects, pcs_object_box* d_boxes,
                                hipStream_t st)
{
    if (bad_records(d_in, n_points, d_n_points, capacity, d_object_of, d_n_objects, max_objects) || (max_objects && !d_boxes) ||
        ((uintptr_t)d_boxes & 7u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_boxes_extents_kernel, tiles_over(capacity), dim3(kBlockThreads), 0, st, d_in, d_n_points, n_points, capacity,
                       d_object_of, d_n_objects, max_objects, d_boxes);
    return hipGetLastError();
}

}  // namespace pcs
