// pcs_kernels_stat.hip — statistical outlier removal on a packed payload (pcs_stat_outlier_device, DESIGN.md section 3 "Statistical
// outlier removal" and section 5): record i has the value D_i = the sum of isqrt(65536 d^2) over its mean_k nearest OTHER records
// within max_dist_mm (fewer than mean_k: the record is SPARSE and dropped), and is kept iff D_i <= T, the threshold
// mean + std_mul x deviation of the D of the non-sparse records, everything in integers. Not in the reference; modelled on PCL's
// StatisticalOutlierRemoval, parity unpinned.
//
// The neighbour search walks the radius filter's index (launch_cell_index_stage's six launches with cell edge max_dist_mm,
// pcs_outlier_index.h); the keep bits go where that filter's flag kernel puts them, so its stages 7 to 9 (tile count, scan, emit) run
// unchanged behind these launches:
//   knn        one lane per record, in record order: the own cell first, then the 26 others; keeps the mean_k + 1 smallest d^2 <=
//              max_dist^2 (the record finds itself in its own cell exactly once, at 0) in an LDS list, column-major
//              (list[j x 128 + lane]: a lane's entries are its own, lanes of a wave never share a bank, no barrier): appended to
//              while it fills, a binary max-heap from then on, its maximum also in a register; a smaller d^2 takes the maximum's
//              place and sifts down, log2(mean_k + 1) steps. A cell whose nearest corner is no nearer than the list's maximum (or
//              beyond max_dist while the list fills) is skipped.
//              D_i, or all ones for a sparse record, into a 4-byte word per record.
//   sums       per workgroup of 256 records: M, S1, and S2 as the sums of the low and the high 32 bits of every D^2 (exact)
//   threshold  one workgroup adds the partials; lane 0 computes T in 128-bit integers and writes the statistics block whole
//   flag       D_i <= T to the wave's ballot: keep_bits[] of the radius filter's layout
//   finish     (behind stage 8) the kept count into the block, the block to the caller's d_stats
// Properties:
//   determinism   the k + 1 smallest d^2 are a multiset: which of two equal values a list drops, and the order a cell's members
//                 arrive in (it shapes the heap), reach neither D nor anything behind it; the sums are integer
//   cost          a record costs the population of the cells around it that it cannot rule out, and up to 2 log2(mean_k + 1) LDS
//                 reads for every value that enters a full list. No early exit: n identical records cost n^2 distance tests.
// Workspace behind the radius filter's (outlier_workspace_bytes): 4 N (D) + 32 ceil(N / 256) (partials) + 256 (the block in the first
// 64 bytes, the host form's copy of it 128 bytes in) = 4.1 bytes per record. Integer arithmetic throughout: no float is converted, compared or stored anywhere in this file.

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"

namespace pcs {

namespace {

constexpr uint32_t kStatThreads = 128;                    // the knn workgroup: (mean_k + 1) x 512 bytes of LDS, 33 280 at k = 64
constexpr uint32_t kStatSparse  = 0xFFFFFFFFu;            // D of a sparse record; above every D (< 2^24)

// dpp_move64 / wave_sum64: copies of pcs_kernels_align.hip's (every existing kernel keeps its code byte for byte).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ long long dpp_move64(long long v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(unsigned long long)v, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((unsigned long long)v >> 32), CTRL, ROW_MASK, 0xf, false);
    return (long long)((unsigned long long)(uint32_t)lo | (unsigned long long)(uint32_t)hi << 32);
}

// Wavefront-wide sum of a 64-bit integer (64 lanes, all active), wave-uniform.
__device__ __forceinline__ long long wave_sum64(long long v)
{
    v += dpp_move64<0x111, 0xf>(v);      // row_shr:1
    v += dpp_move64<0x112, 0xf>(v);      // row_shr:2
    v += dpp_move64<0x114, 0xf>(v);      // row_shr:4
    v += dpp_move64<0x118, 0xf>(v);      // row_shr:8
    v += dpp_move64<0x142, 0xa>(v);      // row_bcast:15 -> rows 1, 3
    v += dpp_move64<0x143, 0xc>(v);      // row_bcast:31 -> rows 2, 3
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(unsigned long long)v, 63);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), 63);
    return (long long)((unsigned long long)lo | (unsigned long long)hi << 32);
}

// floor(sqrt(65536 d2)) for d2 <= 10^6, exact: the 10 bits of floor(sqrt(d2)) in 32-bit integers, then 8 more bits below them
// against 65536 d2 (below 2^37) in 64-bit ones. The result is below 2^18.
__device__ __forceinline__ uint32_t isqrt_q8(uint32_t d2)
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 9; b >= 0; b--) {
        const uint32_t t = r | 1u << b;
        if (t * t <= d2) r = t;
    }
    const unsigned long long x = (unsigned long long)d2 << 16;
    r <<= 8;
#pragma unroll
    for (int b = 7; b >= 0; b--) {
        const uint32_t t = r | 1u << b;
        if ((unsigned long long)t * t <= x) r = t;
    }
    return r;
}

// floor(sqrt(x)), exact, for x below 2^66: the result below 2^33.
__device__ unsigned long long isqrt128(unsigned __int128 x)
{
    unsigned long long r = 0;
    for (int b = 32; b >= 0; b--) {
        const unsigned long long t = r | 1ull << b;
        if ((unsigned __int128)t * t <= x) r = t;
    }
    return r;
}

// The list of a lane, entry j at mine[j x kStatThreads], as a binary max-heap of `need` entries (children of j: 2 j + 1, 2 j + 2): the
// value v goes into the hole at entry `at`, larger children moving up — at most log2(need) steps, two reads and a write each.
__device__ __forceinline__ void heap_sift_down(uint32_t* mine, uint32_t need, uint32_t at, uint32_t v)
{
    for (;;) {
        const uint32_t l = 2u * at + 1u;
        if (l >= need) break;
        uint32_t c = l, cv = mine[l * kStatThreads];
        if (l + 1u < need) {
            const uint32_t rv = mine[(l + 1u) * kStatThreads];
            if (rv > cv) { c = l + 1u; cv = rv; }
        }
        if (cv <= v) break;
        mine[at * kStatThreads] = cv;
        at = c;
    }
    mine[at * kStatThreads] = v;
}

// ---- knn --------------------------------------------------------------------------------------------
// need = mean_k + 1. Differences of members of adjacent cells are below 2 max_dist + 1 <= 2001, their squares' sum below 2^24.
// No barrier anywhere: a lane beyond the count leaves at once, and a lane's list entries are read and written by that lane alone.
__global__ __launch_bounds__(kStatThreads)
void pcs_stat_knn_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, int radius, uint32_t need,
                         const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ start, uint32_t slots,
                         const uint2* __restrict__ xyz, uint32_t capacity, uint32_t* __restrict__ dsum)
{
    extern __shared__ uint32_t list[];                    // need x kStatThreads words
    const uint32_t i = blockIdx.x * kStatThreads + threadIdx.x;
    if (i >= ctl->tab.n_points) return;
    uint32_t* const mine = list + threadIdx.x;            // entry j at mine[j * kStatThreads]
    const Xyz p = load_xyz(in, i);
    const int cx = cell_of(p.x, radius), cy = cell_of(p.y, radius), cz = cell_of(p.z, radius);
    const uint32_t r2 = (uint32_t)(radius * radius);
    // per axis: how far a member of the cell one step down / in the same cell / one step up is at least (the align match kernel's)
    const int fx = p.x - (cx - 32768) * radius, fy = p.y - (cy - 32768) * radius, fz = p.z - (cz - 32768) * radius;
    const auto gap = [radius](int f, int o) { return o == 0 ? f + 1 : o == 1 ? 0 : radius - f; };
    uint32_t cnt = 0, worst = 0;                          // entries in the list; once it is full, their maximum
    for (int c = 0; c < 27; c++) {
        const int cc = c + 13 < 27 ? c + 13 : c - 14;     // 13 = (0, 0, 0): the own cell first
        const int ox = cc % 3, oy = (cc / 3) % 3, oz = cc / 9;
        const int ex = gap(fx, ox), ey = gap(fy, oy), ez = gap(fz, oz);
        const uint32_t low = (uint32_t)(ex * ex + ey * ey + ez * ez);
        if (cnt == need ? low >= worst : low > r2) continue;           // nothing in it would enter the list
        const int ax = cx + ox - 1, ay = cy + oy - 1, az = cz + oz - 1;
        if ((uint32_t)ax > 65535u || (uint32_t)ay > 65535u || (uint32_t)az > 65535u) continue;   // no such cell: skipped, never wrapped
        const unsigned long long key = cell_key(ax, ay, az);
        uint32_t s = first_slot(key, slots), at = kNoSlot;
        for (uint32_t probe = 0; probe < slots; probe++) {              // ends at the key or at the first empty slot; at most `slots` steps
            const unsigned long long k = keys[s];
            if (k == key) at = s;
            if (k == key || k == kEmptyKey) break;
            s = s + 1u == slots ? 0u : s + 1u;
        }
        if (at == kNoSlot) continue;
        const uint32_t e = min(start[at + 1u], capacity);
        for (uint32_t m = start[at]; m < e; m++) {
            const uint2 q = xyz[m];
            const int dx = p.x - (int)(int16_t)(q.x & 0xFFFFu), dy = p.y - (int)(int16_t)(q.x >> 16), dz = p.z - (int)(int16_t)(q.y & 0xFFFFu);
            const uint32_t d2 = (uint32_t)(dx * dx + dy * dy + dz * dz);
            if (d2 > r2) continue;                                      // beyond max_dist: never entered
            if (cnt < need) {
                mine[cnt * kStatThreads] = d2;
                cnt++;
                if (cnt == need) {                                      // full: the entries become a heap, once per record
                    for (uint32_t j = need / 2u; j-- > 0u;) heap_sift_down(mine, need, j, mine[j * kStatThreads]);
                    worst = mine[0];
                }
            } else if (d2 < worst) {                                    // d2 takes the maximum's place
                heap_sift_down(mine, need, 0u, d2);
                worst = mine[0];
            }
        }
    }
    uint32_t d = kStatSparse;
    if (cnt == need) {
        d = 0;
        for (uint32_t j = 0; j < need; j++) d += isqrt_q8(mine[j * kStatThreads]);      // (the record's own 0 adds nothing)
    }
    dsum[i] = d;
}

// ---- sums -------------------------------------------------------------------------------------------
// partials[4 b + 0 .. 3] = M, S1, sum of (D^2 & 0xFFFFFFFF), sum of (D^2 >> 32) over records 256 b .. 256 b + 255.
__global__ __launch_bounds__(kBlockThreads)
void pcs_stat_sums_kernel(const OutlierCtl* __restrict__ ctl, const uint32_t* __restrict__ dsum, long long* __restrict__ partials)
{
    __shared__ long long wsum[(kBlockThreads / 64) * 4];
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    long long term[4] = {0, 0, 0, 0};
    if (i < ctl->tab.n_points) {
        const uint32_t d = dsum[i];
        if (d != kStatSparse) {
            const unsigned long long t = (unsigned long long)d * d;
            term[0] = 1;
            term[1] = (long long)d;
            term[2] = (long long)(t & 0xFFFFFFFFull);
            term[3] = (long long)(t >> 32);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const long long w = wave_sum64(term[t]);
        if ((threadIdx.x & 63) == 0) wsum[(threadIdx.x >> 6) * 4 + t] = w;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        long long total = 0;
        for (uint32_t w = 0; w < kBlockThreads / 64; w++) total += wsum[w * 4 + threadIdx.x];
        partials[(size_t)blockIdx.x * 4 + threadIdx.x] = total;
    }
}

// ---- threshold --------------------------------------------------------------------------------------
// One workgroup. The partials' count follows the capacity; those of workgroups beyond the record count are zeros the sums kernel wrote.
// block[] = considered, dense, s1, s2_lo, s2_hi, threshold, kept (0 here: the finish kernel has it), reserved (0).
__global__ __launch_bounds__(kBlockThreads)
void pcs_stat_threshold_kernel(const OutlierCtl* __restrict__ ctl, const long long* __restrict__ partials, uint32_t n_partials,
                               int std_mul_milli, long long* __restrict__ block)
{
    __shared__ long long wsum[(kBlockThreads / 64) * 4];
    long long term[4] = {0, 0, 0, 0};
    for (uint32_t t0 = 0; t0 < n_partials; t0 += kBlockThreads) {
        const uint32_t j = t0 + threadIdx.x;
        if (j < n_partials) {
#pragma unroll
            for (int t = 0; t < 4; t++) term[t] += partials[(size_t)j * 4 + t];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const long long w = wave_sum64(term[t]);
        if ((threadIdx.x & 63) == 0) wsum[(threadIdx.x >> 6) * 4 + t] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tot[4];
        for (int t = 0; t < 4; t++) {
            tot[t] = 0;
            for (uint32_t w = 0; w < kBlockThreads / 64; w++) tot[t] += wsum[w * 4 + t];
        }
        typedef unsigned __int128 u128;
        const u128 M = (u128)(unsigned long long)tot[0], S1 = (u128)(unsigned long long)tot[1];
        const u128 S2 = (u128)(unsigned long long)tot[2] + ((u128)(unsigned long long)tot[3] << 32);
        long long T = 0;
        if (tot[0] > 0) {
            unsigned long long sigma_q = 0;
            if (tot[0] >= 2) {
                const u128 W = M * S2 - S1 * S1;                        // M < 2^28, S2 < 2^76, S1 < 2^52: non-negative, below 2^104
                sigma_q = isqrt128((W << 16) / (M * (M - 1)));
            }
            T = (long long)(unsigned long long)((256000 * S1 + (u128)(unsigned)std_mul_milli * M * sigma_q) / (256000 * M));
        }
        block[0] = (long long)ctl->tab.n_points;
        block[1] = tot[0];
        block[2] = tot[1];
        block[3] = tot[2];
        block[4] = tot[3];
        block[5] = T;
        block[6] = 0;
        block[7] = 0;
    }
}

// ---- flag -------------------------------------------------------------------------------------------
// keep_bits[w] = the ballot of records 64 w .. 64 w + 63 (a bit at or beyond the count is 0): the radius filter's layout.
__global__ __launch_bounds__(kBlockThreads)
void pcs_stat_flag_kernel(const OutlierCtl* __restrict__ ctl, const uint32_t* __restrict__ dsum, const long long* __restrict__ block,
                          unsigned long long* __restrict__ keep_bits)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    bool keep = false;
    if (i < ctl->tab.n_points) {
        const uint32_t d = dsum[i];
        keep = d != kStatSparse && (long long)d <= block[5];
    }
    const unsigned long long bits = __ballot(keep);
    if ((threadIdx.x & 63) == 0) keep_bits[i >> 6] = bits;
}

// ---- finish -----------------------------------------------------------------------------------------
// One wave: the kept count the scan wrote into the block's word 6, the eight words to the caller.
__global__ __launch_bounds__(64)
void pcs_stat_finish_kernel(const long long* __restrict__ block, const int32_t* __restrict__ kept, long long* __restrict__ stats)
{
    if (threadIdx.x < 8) stats[threadIdx.x] = threadIdx.x == 6 ? (long long)*kept : block[threadIdx.x];
}

inline uint32_t stat_partials(uint32_t capacity) { return (capacity + kBlockThreads - 1) / kBlockThreads; }

}  // namespace

size_t stat_workspace_bytes(uint32_t capacity)
{
    return up256(outlier_workspace_bytes(capacity)) + up256(4 * (size_t)capacity) + up256(32 * (size_t)stat_partials(capacity)) + 256;
}

const char* stat_stage_name(int stage)
{
    static const char* const names[kStatStages] = {"clear", "insert", "cell sums", "cell scan", "cell starts", "scatter", "knn", "sums",
                                                   "threshold", "flag", "tile count", "tile scan", "emit", "finish"};
    return stage >= 0 && stage < kStatStages ? names[stage] : "?";
}

hipError_t launch_stat_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity, int mean_k,
                             int std_mul_milli, int max_dist_mm, void* d_ws, size_t ws_bytes, int16_t* d_out, int32_t* d_out_points,
                             long long* d_stats, hipStream_t st)
{
    if (!capacity || mean_k < PCS_STAT_K_MIN || mean_k > PCS_STAT_K_MAX || std_mul_milli < 0 || std_mul_milli > PCS_STAT_MUL_MILLI_MAX ||
        max_dist_mm < PCS_STAT_DIST_MIN || max_dist_mm > PCS_STAT_DIST_MAX || ws_bytes < stat_workspace_bytes(capacity) ||
        ((uintptr_t)d_ws & 255u) || (!d_n_points && n_points > capacity))
        return hipErrorInvalidValue;
    // over the front of the workspace: the cell index (0 to 5) and the radius filter's compaction (its 7 to 9)
    const size_t index_bytes = up256(outlier_workspace_bytes(capacity));
    if (stage >= 0 && stage < kIndexStages)
        return launch_cell_index_stage(stage, d_in, n_points, d_n_points, capacity, max_dist_mm, d_ws, index_bytes, st);
    if (stage >= 10 && stage <= 12) return launch_outlier_compact_stage(stage - 3, d_in, capacity, d_ws, index_bytes, d_out, d_out_points, st);
    OutlierIndexView view{};
    OutlierKeepView kv{};
    if (hipError_t e = outlier_index_view(capacity, d_ws, index_bytes, &view)) return e;
    if (hipError_t e = outlier_keep_view(capacity, d_ws, index_bytes, &kv)) return e;
    uint8_t* w = static_cast<uint8_t*>(d_ws) + index_bytes;
    uint32_t* const dsum = reinterpret_cast<uint32_t*>(w);            w += up256(4 * (size_t)capacity);
    long long* const partials = reinterpret_cast<long long*>(w);      w += up256(32 * (size_t)stat_partials(capacity));
    long long* const block = reinterpret_cast<long long*>(w);
    const dim3 per_record(stat_partials(capacity)), threads(kBlockThreads);
    switch (stage) {
    case 6:
        hipLaunchKernelGGL(pcs_stat_knn_kernel, dim3((capacity + kStatThreads - 1) / kStatThreads), dim3(kStatThreads),
                           ((size_t)mean_k + 1) * kStatThreads * sizeof(uint32_t), st, d_in, kv.ctl, max_dist_mm, (uint32_t)mean_k + 1u, view.keys,
                           view.start, view.slots, view.xyz, capacity, dsum);
        break;
    case 7:
        hipLaunchKernelGGL(pcs_stat_sums_kernel, per_record, threads, 0, st, kv.ctl, dsum, partials);
        break;
    case 8:
        hipLaunchKernelGGL(pcs_stat_threshold_kernel, dim3(1), threads, 0, st, kv.ctl, partials, stat_partials(capacity), std_mul_milli, block);
        break;
    case 9:
        hipLaunchKernelGGL(pcs_stat_flag_kernel, per_record, threads, 0, st, kv.ctl, dsum, block, kv.keep_bits);
        break;
    case 13:
        if (!d_stats || !d_out_points) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pcs_stat_finish_kernel, dim3(1), dim3(64), 0, st, block, d_out_points, d_stats);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pcs
