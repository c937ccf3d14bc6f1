// pcs_kernels_align.hip — the correspondence step of extrinsics refinement (pcs_align_sums_device, DESIGN.md section 3 "Alignment
// sums" and section 5): for every source record p the nearest target record q within max_dist_mm, and the pairs reduced to the
// eighteen integer sums a rigid fit needs. Not in the reference; this project's own definition, everything in the payload's integer
// millimetres.
//
// The match of p is the target record that minimises (d^2, q.z, q.y, q.x), lexicographic, signed, among those with
// d^2 <= max_dist_mm^2. A lane keeps the minimum of the pair
//     (d^2,  (z + 32768) << 32 | (y + 32768) << 16 | (x + 32768))              d^2 <= 10^6 < 2^20, the coordinates 48 bits
// compared d^2 first, then the coordinate word as ONE unsigned number — which is the order (z, y, x) of the signed coordinates. (The
// two do not fit one 64-bit word: 20 + 48 bits. A single word d^2 << 48 | ... holds d^2 only up to max_dist_mm 255.) The winner's
// coordinates come back out of the word: the tie-break is by value, never by position in xyz[] — which slot a cell took and the
// order of its members (decided by the order atomics arrived in while the index was built) reach no output bit.
//
// The index is the outlier filter's (pcs_kernels_outlier.hip, stages 0 to 5 over the TARGET with cell edge max_dist_mm), read
// through OutlierIndexView; the probe is pcs_outlier_index.h's. A candidate lies in p's own cell or one of the 26 around it.
//   match    one lane per source record; own cell first. A cell whose nearest possible member is farther than the best so far (or
//            than the radius) is not probed: with f_a = p_a - (cell's low edge) in 0 .. r - 1, a member of the cell one step down
//            on axis a is at least f_a + 1 away on that axis, one step up at least r - f_a, the same cell 0; the squares' sum is a
//            lower bound for every member. A cell is skipped only if that bound EXCEEDS the best d^2: a bound equal to it may hold
//            a tie that wins on (z, y, x). So pruning cannot change a bit.
//            Each lane's eighteen int64 terms are summed over the wave by DPP (the wave scan's row_shr / row_bcast sequence on both
//            halves of a word), over the workgroup's four waves through LDS: one 144-byte partial per workgroup.
//   reduce   one workgroup adds the partials (each lane a strided share, then the same wave / LDS sum) and writes *d_sums whole:
//            nobody zeroes it first, no atomics, integer addition — the result does not depend on any order.
// No hang: every probe loop runs at most `slots` steps (an empty slot ends every miss, as in the flag kernel). Bounds: a lane reads
// source record i < n_source, keys[s] with s < slots, start[at] and start[at + 1] with at < slots (slots + 1 starts), xyz[m] with
// m < min(start[at + 1], capacity); it writes dist2[i] with i < n_source and partial blockIdx.x < align_partials(n_source).
// Cost: a source record costs the population of the cells it could not prune, and up to 27 probe sequences.
// Integer arithmetic throughout: no float is converted, compared or stored anywhere in this file.

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"

namespace pcs {

namespace {

constexpr uint32_t kNoMatch       = 0xFFFFFFFFu;          // dist2 of an unmatched record; above every d^2 (<= 10^6)
constexpr uint32_t kReduceThreads = kBlockThreads;        // the reduce workgroup: partials beyond this many make its loop run again

// A 64-bit word from the lane the DPP control names (0 where there is none), half by half.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ long long dpp_move64(long long v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(unsigned long long)v, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((unsigned long long)v >> 32), CTRL, ROW_MASK, 0xf, false);
    return (long long)((unsigned long long)(uint32_t)lo | (unsigned long long)(uint32_t)hi << 32);
}

// Wavefront-wide sum of a 64-bit integer (64 lanes, all active), wave-uniform: wave_inclusive_scan's sequence, lane 63 read back.
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

// The workgroup's sum of every lane's kAlignTerms terms, term t in lanes t < kAlignTerms of the return value (others: 0).
// WAVES = blockDim.x / 64; `lds` holds WAVES x kAlignTerms words. All lanes of the workgroup call it.
template <int WAVES>
__device__ __forceinline__ long long block_sum_terms(const long long (&term)[kAlignTerms], long long* lds)
{
#pragma unroll
    for (int t = 0; t < kAlignTerms; t++) {
        const long long w = wave_sum64(term[t]);
        if ((threadIdx.x & 63) == 0) lds[(threadIdx.x >> 6) * kAlignTerms + t] = w;
    }
    __syncthreads();
    long long total = 0;
    if (threadIdx.x < kAlignTerms)
        for (int w = 0; w < WAVES; w++) total += lds[w * kAlignTerms + threadIdx.x];
    return total;
}

// ---- match ------------------------------------------------------------------------------------------
// keys == nullptr: an empty target, nobody matches (no index was built).
__global__ __launch_bounds__(kBlockThreads)
void pcs_align_match_kernel(const int16_t* __restrict__ source, uint32_t n_source, int radius,
                            const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ start, uint32_t slots,
                            const uint2* __restrict__ xyz, uint32_t capacity, long long* __restrict__ partials,
                            uint32_t* __restrict__ dist2)
{
    __shared__ long long wsum[(kBlockThreads / 64) * kAlignTerms];
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    long long term[kAlignTerms];
#pragma unroll
    for (int t = 0; t < kAlignTerms; t++) term[t] = 0;
    if (i < n_source) {
        const Xyz p = load_xyz(source, i);
        uint32_t best_d2 = kNoMatch;                  // the minimum so far: (best_d2, best_q), kNoMatch while nobody is within the radius
        unsigned long long best_q = 0;
        if (keys) {
            const int cx = cell_of(p.x, radius), cy = cell_of(p.y, radius), cz = cell_of(p.z, radius);
            const int r2 = radius * radius;
            // per axis: how far a member of the cell one step down / in the same cell / one step up is at least
            const int fx = p.x - (cx - 32768) * radius, fy = p.y - (cy - 32768) * radius, fz = p.z - (cz - 32768) * radius;
            const auto gap = [radius](int f, int o) { return o == 0 ? f + 1 : o == 1 ? 0 : radius - f; };
            uint32_t bound = (uint32_t)r2;                               // min(r^2, the best d^2 so far)
            for (int c = 0; c < 27; c++) {
                const int cc = c + 13 < 27 ? c + 13 : c - 14;           // 13 = (0, 0, 0): the own cell first
                const int ox = cc % 3, oy = (cc / 3) % 3, oz = cc / 9;
                const int ex = gap(fx, ox), ey = gap(fy, oy), ez = gap(fz, oz);
                const uint32_t low = (uint32_t)(ex * ex + ey * ey + ez * ez);
                if (low > bound) continue;                              // (equal: it may hold a tie)
                const int ax = cx + ox - 1, ay = cy + oy - 1, az = cz + oz - 1;
                if ((uint32_t)ax > 65535u || (uint32_t)ay > 65535u || (uint32_t)az > 65535u) continue;   // no such cell: skipped, never wrapped
                const unsigned long long key = cell_key(ax, ay, az);
                uint32_t s = first_slot(key, slots), at = kNoSlot;
                for (uint32_t probe = 0; probe < slots; probe++) {       // ends at the key or at the first empty slot; at most `slots` steps
                    const unsigned long long k = keys[s];
                    if (k == key) at = s;
                    if (k == key || k == kEmptyKey) break;
                    s = s + 1u == slots ? 0u : s + 1u;
                }
                if (at == kNoSlot) continue;
                const uint32_t e = min(start[at + 1u], capacity);
                for (uint32_t m = start[at]; m < e; m++) {
                    const uint2 q = xyz[m];
                    const int qx = (int)(int16_t)(q.x & 0xFFFFu), qy = (int)(int16_t)(q.x >> 16), qz = (int)(int16_t)(q.y & 0xFFFFu);
                    const int dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
                    // members of adjacent cells: each difference below 2 r + 1 <= 2001, the sum below 2^24
                    const uint32_t d2 = (uint32_t)(dx * dx + dy * dy + dz * dz);
                    if (d2 > (uint32_t)r2) continue;                    // beyond the radius: never entered
                    const unsigned long long word = (unsigned long long)(uint32_t)(qz + 32768) << 32 |
                                                    (unsigned long long)(uint32_t)(qy + 32768) << 16 | (unsigned long long)(uint32_t)(qx + 32768);
                    if (d2 < best_d2 || (d2 == best_d2 && word < best_q)) { best_d2 = d2; best_q = word; }
                }
                if (best_d2 != kNoMatch) bound = best_d2;
            }
        }
        term[0] = 1;                                                     // considered
        if (best_d2 != kNoMatch) {
            const long long qx = (long long)(uint32_t)(best_q & 0xFFFFu) - 32768, qy = (long long)(uint32_t)((best_q >> 16) & 0xFFFFu) - 32768,
                            qz = (long long)(uint32_t)((best_q >> 32) & 0xFFFFu) - 32768;
            const long long px = p.x, py = p.y, pz = p.z;
            term[1] = 1;                                                 // matched
            term[2] = px; term[3] = py; term[4] = pz;                    // sp
            term[5] = qx; term[6] = qy; term[7] = qz;                    // sq
            term[8]  = px * qx; term[9]  = px * qy; term[10] = px * qz;  // spq[3 a + b] = p_a q_b
            term[11] = py * qx; term[12] = py * qy; term[13] = py * qz;
            term[14] = pz * qx; term[15] = pz * qy; term[16] = pz * qz;
            term[17] = (long long)best_d2;                               // sd2
        }
        if (dist2) dist2[i] = best_d2;                                   // (kNoMatch is the unmatched word)
    }
    const long long total = block_sum_terms<kBlockThreads / 64>(term, wsum);
    if (threadIdx.x < kAlignTerms) partials[(size_t)blockIdx.x * kAlignTerms + threadIdx.x] = total;
}

// ---- reduce -----------------------------------------------------------------------------------------
// One workgroup. Lane l adds partials l, l + kReduceThreads, ... (the loop runs once per kReduceThreads partials), then the lanes'
// sums are added the way the match kernel adds its lanes' terms.
__global__ __launch_bounds__(kReduceThreads)
void pcs_align_reduce_kernel(const long long* __restrict__ partials, uint32_t n_partials, long long* __restrict__ sums)
{
    __shared__ long long wsum[(kReduceThreads / 64) * kAlignTerms];
    long long term[kAlignTerms];
#pragma unroll
    for (int t = 0; t < kAlignTerms; t++) term[t] = 0;
    for (uint32_t t0 = 0; t0 < n_partials; t0 += kReduceThreads) {
        const uint32_t j = t0 + threadIdx.x;
        if (j < n_partials) {
            const long long* q = partials + (size_t)j * kAlignTerms;
#pragma unroll
            for (int t = 0; t < kAlignTerms; t++) term[t] += q[t];
        }
    }
    const long long total = block_sum_terms<kReduceThreads / 64>(term, wsum);
    if (threadIdx.x < kAlignTerms) sums[threadIdx.x] = total;
}

}  // namespace

hipError_t launch_align_match(const int16_t* d_source, uint32_t n_source, const OutlierIndexView* index, int max_dist_mm,
                              long long* d_partials, uint32_t* d_dist2, hipStream_t st)
{
    if (!n_source || !d_source || !d_partials || max_dist_mm < PCS_ALIGN_DIST_MIN || max_dist_mm > PCS_ALIGN_DIST_MAX)
        return hipErrorInvalidValue;
    if (index && (!index->keys || !index->start || !index->xyz || !index->slots || !index->capacity)) return hipErrorInvalidValue;
    const OutlierIndexView none{nullptr, nullptr, nullptr, 0u, 0u};
    const OutlierIndexView& v = index ? *index : none;
    hipLaunchKernelGGL(pcs_align_match_kernel, dim3(align_partials(n_source)), dim3(kBlockThreads), 0, st, d_source, n_source, max_dist_mm,
                       v.keys, v.start, v.slots, v.xyz, v.capacity, d_partials, d_dist2);
    return hipGetLastError();
}

hipError_t launch_align_reduce(const long long* d_partials, uint32_t n_partials, long long* d_sums, hipStream_t st)
{
    if (!d_sums || (n_partials && !d_partials)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_align_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, st, d_partials, n_partials, d_sums);
    return hipGetLastError();
}

}  // namespace pcs

// ---- point to plane -----------------------------------------------------------------------------------
// pcs_align_plane_sums_device (DESIGN.md section 3 "Plane sums"): the same match, and per pair the row a = (p x n, n), b = n . (q - p)
// of the linearised point-to-plane problem, n the three shorts of the match's normal; the pairs reduced to A^T A (upper triangle), A^T b,
// sum b^2. |p x n| < 2^31 and |b| < 2^28 for any int16 normal, so every product fits int64; their SUM over a payload does not, so
// each product t travels as two halves — t & 0xFFFFFFFF (unsigned) and t >> 32 (arithmetic) — summed separately (each below 2^60 for
// fewer than 2^28 records) and recombined on the host as hi 2^32 + lo.
//   scatter  the target's normals into cell order beside xyz[]: pnorm[] starts as all ones (the host layer's memset); one lane per
//            target record with a valid normal (short 3 != 0) walks its own cell's run and does a 64-bit atomicMin of its key into
//            every entry whose coordinates equal its own. The key is the four shorts as one little-endian number minus 2^48: valid
//            words are exactly those >= 2^48, so the order is kept and all ones stays free to mean "no valid normal". Every entry
//            of equal coordinates ends with the same key, the smallest: the order the atomics arrive in reaches no output bit.
//   match    pcs_align_match_kernel's probe, pruning and (d^2, coordinate word) comparison, line for line, and the winner's position
//            in xyz[] kept beside it: any position with the winner's coordinates holds the same key. The sixty terms are formed and
//            summed over the wave one at a time (sixty live 64-bit words are not a register budget): one 480-byte partial per
//            workgroup.
//   reduce   one workgroup of 1 024: lane (g, t) adds term t of partials g, g + 16, ..., the sixteen groups meet in LDS; *d_sums is
//            written whole.
// Bounds: as the match above; pnorm[m] wherever xyz[m] is read or written (m < min(start[at + 1], capacity)), normals[i] with
// i < n_target, partial blockIdx.x < align_partials(n_source). No floats.

namespace pcs {

namespace {

constexpr unsigned long long kNoNormal   = ~0ull;
constexpr unsigned long long kNormalBase = 1ull << 48;          // the smallest valid word: short 3 = 1, the rest 0
constexpr uint32_t kPlaneReduceThreads = 1024;                   // the plane reduce workgroup: sixteen groups of 64 lanes, a term each
constexpr int kAtaLo = 3, kAtaHi = 24, kAtbLo = 45, kAtbHi = 51, kSb2Lo = 57, kSb2Hi = 58, kPlaneSd2 = 59;      // pcs_align_plane_sums

static_assert(kPlaneTerms == 60 && kPlaneTerms <= 64, "the reduce kernel gives a term to each of 64 lanes");

__global__ __launch_bounds__(kBlockThreads)
void pcs_align_plane_scatter_kernel(const int16_t* __restrict__ target, const unsigned long long* __restrict__ normals, uint32_t n_target,
                                    int radius, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ start,
                                    uint32_t slots, const uint2* __restrict__ xyz, uint32_t capacity, unsigned long long* __restrict__ pnorm)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n_target) return;
    const unsigned long long word = normals[i];
    if (word < kNormalBase) return;                                      // short 3 == 0: not a valid normal
    const Xyz p = load_xyz(target, i);
    const uint2 want = make_uint2((uint32_t)(uint16_t)p.x | (uint32_t)(uint16_t)p.y << 16, (uint32_t)(uint16_t)p.z);
    const unsigned long long key = cell_key(cell_of(p.x, radius), cell_of(p.y, radius), cell_of(p.z, radius));
    uint32_t s = first_slot(key, slots), at = kNoSlot;
    for (uint32_t probe = 0; probe < slots; probe++) {                   // ends at the key or at the first empty slot; at most `slots` steps
        const unsigned long long k = keys[s];
        if (k == key) at = s;
        if (k == key || k == kEmptyKey) break;
        s = s + 1u == slots ? 0u : s + 1u;
    }
    if (at == kNoSlot) return;                                           // (cannot happen: the index holds every target record)
    const uint32_t e = min(start[at + 1u], capacity);
    for (uint32_t m = start[at]; m < e; m++) {
        const uint2 q = xyz[m];
        if (q.x == want.x && q.y == want.y) atomicMin(pnorm + m, word - kNormalBase);
    }
}

// One term of the workgroup's partial: its wave sum into the wave's row of `lds`.
__device__ __forceinline__ void put_term(long long* lds, int t, long long v)
{
    const long long w = wave_sum64(v);
    if ((threadIdx.x & 63) == 0) lds[(threadIdx.x >> 6) * kPlaneTerms + t] = w;
}

// a product's two halves into terms lo and hi
__device__ __forceinline__ void put_split(long long* lds, int lo, int hi, long long v)
{
    put_term(lds, lo, (long long)((unsigned long long)v & 0xFFFFFFFFull));
    put_term(lds, hi, v >> 32);
}

// keys == nullptr: an empty target, nobody matches (no index was built).
__global__ __launch_bounds__(kBlockThreads)
void pcs_align_plane_match_kernel(const int16_t* __restrict__ source, uint32_t n_source, int radius,
                                  const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ start, uint32_t slots,
                                  const uint2* __restrict__ xyz, const unsigned long long* __restrict__ pnorm, uint32_t capacity,
                                  long long* __restrict__ partials, uint32_t* __restrict__ dist2)
{
    __shared__ long long wsum[(kBlockThreads / 64) * kPlaneTerms];
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    long long considered = 0, matched = 0, used = 0, sd2 = 0, b = 0;
    long long a[6] = {0, 0, 0, 0, 0, 0};
    if (i < n_source) {
        const Xyz p = load_xyz(source, i);
        uint32_t best_d2 = kNoMatch, best_m = 0;      // the minimum so far: (best_d2, best_q) at xyz[best_m]
        unsigned long long best_q = 0;
        if (keys) {
            const int cx = cell_of(p.x, radius), cy = cell_of(p.y, radius), cz = cell_of(p.z, radius);
            const int r2 = radius * radius;
            const int fx = p.x - (cx - 32768) * radius, fy = p.y - (cy - 32768) * radius, fz = p.z - (cz - 32768) * radius;
            const auto gap = [radius](int f, int o) { return o == 0 ? f + 1 : o == 1 ? 0 : radius - f; };
            uint32_t bound = (uint32_t)r2;                               // min(r^2, the best d^2 so far)
            for (int c = 0; c < 27; c++) {
                const int cc = c + 13 < 27 ? c + 13 : c - 14;           // 13 = (0, 0, 0): the own cell first
                const int ox = cc % 3, oy = (cc / 3) % 3, oz = cc / 9;
                const int ex = gap(fx, ox), ey = gap(fy, oy), ez = gap(fz, oz);
                const uint32_t low = (uint32_t)(ex * ex + ey * ey + ez * ez);
                if (low > bound) continue;                              // (equal: it may hold a tie)
                const int ax = cx + ox - 1, ay = cy + oy - 1, az = cz + oz - 1;
                if ((uint32_t)ax > 65535u || (uint32_t)ay > 65535u || (uint32_t)az > 65535u) continue;   // no such cell: skipped, never wrapped
                const unsigned long long key = cell_key(ax, ay, az);
                uint32_t s = first_slot(key, slots), at = kNoSlot;
                for (uint32_t probe = 0; probe < slots; probe++) {       // ends at the key or at the first empty slot; at most `slots` steps
                    const unsigned long long k = keys[s];
                    if (k == key) at = s;
                    if (k == key || k == kEmptyKey) break;
                    s = s + 1u == slots ? 0u : s + 1u;
                }
                if (at == kNoSlot) continue;
                const uint32_t e = min(start[at + 1u], capacity);
                for (uint32_t m = start[at]; m < e; m++) {
                    const uint2 q = xyz[m];
                    const int qx = (int)(int16_t)(q.x & 0xFFFFu), qy = (int)(int16_t)(q.x >> 16), qz = (int)(int16_t)(q.y & 0xFFFFu);
                    const int dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
                    const uint32_t d2 = (uint32_t)(dx * dx + dy * dy + dz * dz);
                    if (d2 > (uint32_t)r2) continue;                    // beyond the radius: never entered
                    const unsigned long long word = (unsigned long long)(uint32_t)(qz + 32768) << 32 |
                                                    (unsigned long long)(uint32_t)(qy + 32768) << 16 | (unsigned long long)(uint32_t)(qx + 32768);
                    if (d2 < best_d2 || (d2 == best_d2 && word < best_q)) { best_d2 = d2; best_q = word; best_m = m; }
                }
                if (best_d2 != kNoMatch) bound = best_d2;
            }
        }
        considered = 1;
        if (best_d2 != kNoMatch) {
            matched = 1;
            sd2 = (long long)best_d2;
            const unsigned long long nk = pnorm[best_m];                 // (best_m < capacity: it indexed xyz[])
            if (nk != kNoNormal) {
                const unsigned long long w = nk + kNormalBase;
                const long long nx = (int16_t)(uint16_t)w, ny = (int16_t)(uint16_t)(w >> 16), nz = (int16_t)(uint16_t)(w >> 32);
                const long long qx = (long long)(uint32_t)(best_q & 0xFFFFu) - 32768, qy = (long long)(uint32_t)((best_q >> 16) & 0xFFFFu) - 32768,
                                qz = (long long)(uint32_t)((best_q >> 32) & 0xFFFFu) - 32768;
                const long long px = p.x, py = p.y, pz = p.z;
                used = 1;
                a[0] = py * nz - pz * ny; a[1] = pz * nx - px * nz; a[2] = px * ny - py * nx;      // c = p x n
                a[3] = nx; a[4] = ny; a[5] = nz;
                b = nx * (qx - px) + ny * (qy - py) + nz * (qz - pz);
            }
        }
        if (dist2) dist2[i] = best_d2;                                   // (kNoMatch is the unmatched word)
    }
    put_term(wsum, 0, considered);
    put_term(wsum, 1, matched);
    put_term(wsum, 2, used);
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int c = r; c < 6; c++, k++) put_split(wsum, kAtaLo + k, kAtaHi + k, a[r] * a[c]);       // (an unused pair: a = 0)
    }
#pragma unroll
    for (int r = 0; r < 6; r++) put_split(wsum, kAtbLo + r, kAtbHi + r, a[r] * b);
    put_split(wsum, kSb2Lo, kSb2Hi, b * b);
    put_term(wsum, kPlaneSd2, sd2);
    __syncthreads();
    if (threadIdx.x < kPlaneTerms) {
        long long total = 0;
        for (int w = 0; w < (int)(kBlockThreads / 64); w++) total += wsum[w * kPlaneTerms + threadIdx.x];
        partials[(size_t)blockIdx.x * kPlaneTerms + threadIdx.x] = total;
    }
}

// One workgroup of kPlaneReduceThreads: lane (g, t) adds term t of partials g, g + 16, ... (a wave reads 480 contiguous bytes of one
// partial; eight loads in flight per lane), the sixteen groups meet in LDS.
__global__ __launch_bounds__(kPlaneReduceThreads)
void pcs_align_plane_reduce_kernel(const long long* __restrict__ partials, uint32_t n_partials, long long* __restrict__ sums)
{
    constexpr uint32_t kGroups = kPlaneReduceThreads / 64;
    __shared__ long long gsum[kGroups * 64];
    const uint32_t t = threadIdx.x & 63u, g = threadIdx.x >> 6;
    long long total = 0;
    if (t < (uint32_t)kPlaneTerms) {
#pragma unroll 8
        for (uint32_t j = g; j < n_partials; j += kGroups) total += partials[(size_t)j * kPlaneTerms + t];
    }
    gsum[threadIdx.x] = total;
    __syncthreads();
    if (threadIdx.x < (uint32_t)kPlaneTerms) {
        long long all = 0;
        for (uint32_t w = 0; w < kGroups; w++) all += gsum[w * 64 + threadIdx.x];
        sums[threadIdx.x] = all;
    }
}

}  // namespace

hipError_t launch_align_plane_scatter(const int16_t* d_target, const int16_t* d_target_normals, uint32_t n_target,
                                      const OutlierIndexView& index, int max_dist_mm, unsigned long long* d_pnorm, hipStream_t st)
{
    if (!n_target || !d_target || !d_target_normals || ((uintptr_t)d_target_normals & 7u) || !d_pnorm || !index.keys || !index.start ||
        !index.xyz || !index.slots || n_target > index.capacity || max_dist_mm < PCS_ALIGN_DIST_MIN || max_dist_mm > PCS_ALIGN_DIST_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_align_plane_scatter_kernel, dim3((n_target + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st,
                       d_target, reinterpret_cast<const unsigned long long*>(d_target_normals), n_target, max_dist_mm, index.keys, index.start,
                       index.slots, index.xyz, index.capacity, d_pnorm);
    return hipGetLastError();
}

hipError_t launch_align_plane_match(const int16_t* d_source, uint32_t n_source, const OutlierIndexView* index, const unsigned long long* d_pnorm,
                                    int max_dist_mm, long long* d_partials, uint32_t* d_dist2, hipStream_t st)
{
    if (!n_source || !d_source || !d_partials || max_dist_mm < PCS_ALIGN_DIST_MIN || max_dist_mm > PCS_ALIGN_DIST_MAX)
        return hipErrorInvalidValue;
    if (index && (!index->keys || !index->start || !index->xyz || !index->slots || !index->capacity || !d_pnorm)) return hipErrorInvalidValue;
    const OutlierIndexView none{nullptr, nullptr, nullptr, 0u, 0u};
    const OutlierIndexView& v = index ? *index : none;
    hipLaunchKernelGGL(pcs_align_plane_match_kernel, dim3(align_partials(n_source)), dim3(kBlockThreads), 0, st, d_source, n_source,
                       max_dist_mm, v.keys, v.start, v.slots, v.xyz, d_pnorm, v.capacity, d_partials, d_dist2);
    return hipGetLastError();
}

hipError_t launch_align_plane_reduce(const long long* d_partials, uint32_t n_partials, long long* d_sums, hipStream_t st)
{
    if (!d_sums || (n_partials && !d_partials)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_align_plane_reduce_kernel, dim3(1), dim3(kPlaneReduceThreads), 0, st, d_partials, n_partials, d_sums);
    return hipGetLastError();
}

}  // namespace pcs
