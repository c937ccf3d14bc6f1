// pcs_kernels_outlier.hip — radius outlier removal on a packed payload (pcs_radius_outlier_device, DESIGN.md section 3 "Radius outlier
// removal" and section 5): record i is kept iff at least min_neighbors OTHER records lie within radius_mm of it, everything in the
// payload's integer millimetres. Not in the reference (its centre programs include PCL's filters and never use them); modelled on
// PCL's RadiusOutlierRemoval, parity unpinned.
//
// The neighbour search is a uniform grid of cell edge radius_mm: cell coordinate = floor(v / radius_mm) + 32768 per axis (0..65535 at
// radius 1), key = the three side by side (48 bits, no aliasing). A record's neighbours lie in its own cell and the 26 around it.
// One call builds the index from nothing and throws it away:
//   0 clear    keys[] = empty, count[] = 0; the record count (clamped to 0..capacity) into the control block
//   1 insert   one lane per record: find or claim the cell's slot in an open-addressing table (linear probing, a 64-bit
//              compare-and-swap on the key), count[slot]++ — the value the add returns is the record's rank in its cell
//   2-4        exclusive scan of count[] over the SLOTS, in place (tile sums, one workgroup over the sums, tile scan): start[]
//   5 scatter  x, y, z of record i to xyz[start[slot] + rank] (8 bytes): a cell's members are one contiguous run
//   6 flag     one lane per record: own cell first, then the 26 others; counts members within the radius (itself included: it is
//              in its own cell exactly once) and stops at min_neighbors + 1; the wave's ballot is 64 keep bits
//   7 count    kept records per 2048-record tile (popcount of 32 words)
//   8 scan     pcs_scan_kernel (pcs_kernels.hip, launch_scan) over a one-stream table: tile prefixes and the kept count
//   9 emit     order-preserving compaction through LDS, modelled on pcs_crop_payloads_device's emit
// Properties:
//   determinism   the keep bit is a comparison of a COUNT; the order atomics arrive in decides which slot of a probe sequence a cell
//                 takes and the order of a cell's members in xyz[], nothing that reaches the output
//   no hang       every probe loop runs at most `slots` steps; slots >= 2 x capacity and at most `capacity` cells exist, so an empty
//                 slot ends every miss and the table cannot fill
//   cost          a record costs at most the population of its 27 cells (and 27 probe sequences). Adversarial: many records just
//                 outside each other's radius — a lattice of pitch radius + 1 puts 8 to 27 records into every lane's walk and keeps
//                 none, and a cell holding m records none of which reaches min_neighbors costs m per record: O(m^2) for the cell
//   early exit    a cloud of n identical records costs n x (min_neighbors + 1) distance tests, not n^2
// Workspace, from the capacity N (n_points / max_points) alone, with slots = 2048 ceil(2 N / 2048):
//   8 slots (keys) + 4 (slots + 1) (count / start) + 4 N (slot of a record) + 4 N (rank) + 8 N (xyz) + N / 8 (keep bits)
//   + 8 ceil(N / 2048) (tile counts and prefixes) + 4 slots / 2048 (slot-tile sums) + 512 (control)  =  40.2 bytes per record.
// Integer arithmetic throughout: no float is converted, compared or stored anywhere in this file.

#include <algorithm>

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"

namespace pcs {

namespace {

constexpr uint32_t           kStageBytes = kTilePoints * PCS_POINT_BYTES + 32;   // + head skew + tail pad

// stage_record / unstage_record / load_staged / store_staged: copies of pcs_kernels.hip's, as unstage_record_crop is one — every
// existing kernel keeps its code byte for byte (tools/isa_compare.py), so nothing there is routed through a shared helper.
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
    r.b = odd ? (b >> 16) : h;                               // all 16 bits of short 4: its high byte travels unchanged
    return r;
}

// LDS bytes [head, head + nbytes) <- / -> global bytes [g, g + nbytes), (g - head) 16-byte aligned: the interior as lane-contiguous
// 16-byte accesses, the ragged ends as 2-byte ones — never a byte outside [g, g + nbytes).
__device__ __forceinline__ void load_staged(uint8_t* lds, uint32_t head, uint32_t nbytes, const uint8_t* g)
{
    const uint8_t* g0 = g - head;
    const uint32_t end = head + nbytes;
    const uint32_t first_full = (head + 15u) >> 4, last_full = end >> 4;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (uint32_t j = first_full + threadIdx.x; j < last_full; j += kBlockThreads)
        reinterpret_cast<u32x4*>(lds)[j] = reinterpret_cast<const u32x4*>(g0)[j];
    const uint32_t head_end = min(first_full << 4, end);
    for (uint32_t b = head + 2u * threadIdx.x; b < head_end; b += 2u * kBlockThreads)
        *reinterpret_cast<uint16_t*>(lds + b) = *reinterpret_cast<const uint16_t*>(g0 + b);
    if (last_full >= first_full) {
        const uint32_t tail_begin = max(last_full << 4, head_end);
        for (uint32_t b = tail_begin + 2u * threadIdx.x; b < end; b += 2u * kBlockThreads)
            *reinterpret_cast<uint16_t*>(lds + b) = *reinterpret_cast<const uint16_t*>(g0 + b);
    }
}

__device__ __forceinline__ void store_staged(const uint8_t* lds, uint32_t head, uint32_t nbytes, uint8_t* g)
{
    uint8_t* g0 = g - head;
    const uint32_t end = head + nbytes;
    const uint32_t first_full = (head + 15u) >> 4, last_full = end >> 4;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (uint32_t j = first_full + threadIdx.x; j < last_full; j += kBlockThreads)
        __builtin_nontemporal_store(reinterpret_cast<const u32x4*>(lds)[j], reinterpret_cast<u32x4*>(g0) + j);
    const uint32_t head_end = min(first_full << 4, end);
    for (uint32_t b = head + 2u * threadIdx.x; b < head_end; b += 2u * kBlockThreads)
        *reinterpret_cast<uint16_t*>(g0 + b) = *reinterpret_cast<const uint16_t*>(lds + b);
    if (last_full >= first_full) {
        const uint32_t tail_begin = max(last_full << 4, head_end);
        for (uint32_t b = tail_begin + 2u * threadIdx.x; b < end; b += 2u * kBlockThreads)
            *reinterpret_cast<uint16_t*>(g0 + b) = *reinterpret_cast<const uint16_t*>(lds + b);
    }
}

// ---- cells: cell_of, cell_key, first_slot, load_xyz and the empty key live in pcs_outlier_index.h (the alignment sums share them) ----

// ---- 0: clear ---------------------------------------------------------------------------------------
// (d_n non-null: the counted form — the count is read here, when the kernels run, and clamped.) Entry 0 of `tab` is all the scan
// kernel reads: n_points and tile_base.
__global__ __launch_bounds__(kBlockThreads)
void pcs_outlier_clear_kernel(OutlierCtl* __restrict__ ctl, const int32_t* __restrict__ d_n, uint32_t n_host, uint32_t capacity,
                              unsigned long long* __restrict__ keys, uint32_t* __restrict__ count, uint32_t slots)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i == 0) {
        uint32_t n = n_host;
        if (d_n) { const int32_t v = *d_n; n = v < 0 ? 0u : min((uint32_t)v, capacity); }
        ctl->tab.n_points = n;
        ctl->tab.tile_base = 0u;
    }
    if (i < slots) keys[i] = kEmptyKey;
    if (i <= slots) count[i] = 0u;
}

// ---- 1: insert --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_outlier_insert_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, int radius,
                               unsigned long long* __restrict__ keys, uint32_t* __restrict__ count, uint32_t slots,
                               uint32_t* __restrict__ slot_of, uint32_t* __restrict__ rank)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= ctl->tab.n_points) return;
    const Xyz p = load_xyz(in, i);
    const unsigned long long key = cell_key(cell_of(p.x, radius), cell_of(p.y, radius), cell_of(p.z, radius));
    uint32_t s = first_slot(key, slots), found = kNoSlot;
    // A slot's key is written once (empty -> key) and never again: a key read here is final, an "empty" read may be stale and the
    // compare-and-swap settles it. At most `slots` steps.
    for (uint32_t probe = 0; probe < slots; probe++) {
        unsigned long long k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kEmptyKey) {
            unsigned long long expected = kEmptyKey;
            k = __hip_atomic_compare_exchange_strong(keys + s, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                    ? key : expected;
        }
        if (k == key) { found = s; break; }
        s = s + 1u == slots ? 0u : s + 1u;
    }
    // (found == kNoSlot cannot happen: fewer cells than slots. Such a record would be left out of the index, not written anywhere.)
    slot_of[i] = found;
    rank[i] = found != kNoSlot ? __hip_atomic_fetch_add(count + found, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}

// ---- 2-4: count[] -> start[] ------------------------------------------------------------------------
// slots is a multiple of kTilePoints: a workgroup owns 2048 slots, 8 per lane.
__global__ __launch_bounds__(kBlockThreads)
void pcs_outlier_cell_sums_kernel(const uint32_t* __restrict__ count, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t wsum[4];
    const uint4* c = reinterpret_cast<const uint4*>(count + (size_t)blockIdx.x * kTilePoints + threadIdx.x * 8u);
    const uint4 a = c[0], b = c[1];
    const uint32_t w = wave_sum(a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup: sums[0 .. tiles) to their exclusive prefixes in place; the total into count[slots] (one past the last cell's start).
__global__ __launch_bounds__(1024)
void pcs_outlier_cell_scan_kernel(uint32_t* __restrict__ sums, uint32_t tiles, uint32_t* __restrict__ total)
{
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < tiles; t0 += 1024) {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = t < tiles ? sums[t] : 0u;
        uint32_t wave_total;
        const uint32_t ex = wave_exclusive_scan(c, wave_total);
        if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = wave_total;
        __syncthreads();
        uint32_t before = carry_s;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wtot[w];
        if (t < tiles) sums[t] = before + ex;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + ex + c;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_outlier_cell_starts_kernel(uint32_t* __restrict__ count, const uint32_t* __restrict__ prefix)
{
    __shared__ uint32_t wsum[4];
    uint4* c = reinterpret_cast<uint4*>(count + (size_t)blockIdx.x * kTilePoints + threadIdx.x * 8u);
    uint4 a = c[0], b = c[1];
    const uint32_t lane_total = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
    uint32_t wave_total;
    const uint32_t ex = wave_exclusive_scan(lane_total, wave_total);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    uint32_t run = prefix[blockIdx.x] + ex;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) run += wsum[w];
    uint32_t v;
    v = a.x; a.x = run; run += v;  v = a.y; a.y = run; run += v;  v = a.z; a.z = run; run += v;  v = a.w; a.w = run; run += v;
    v = b.x; b.x = run; run += v;  v = b.y; b.y = run; run += v;  v = b.z; b.z = run; run += v;  v = b.w; b.w = run; run += v;
    c[0] = a; c[1] = b;
}

// ---- 5: scatter -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_outlier_scatter_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, const uint32_t* __restrict__ start,
                                const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ rank, uint32_t capacity,
                                uint2* __restrict__ xyz)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= ctl->tab.n_points) return;
    const uint32_t s = slot_of[i];
    if (s == kNoSlot) return;
    const uint32_t at = start[s] + rank[i];
    if (at >= capacity) return;                 // (cannot happen: the starts and ranks of n records add up to n)
    const Xyz p = load_xyz(in, i);
    xyz[at] = make_uint2((uint32_t)(uint16_t)p.x | (uint32_t)(uint16_t)p.y << 16, (uint32_t)(uint16_t)p.z);
}

// ---- 6: flag ----------------------------------------------------------------------------------------
// need = min_neighbors + 1: the record finds itself in its own cell, once, at distance 0. Differences of members of adjacent cells are
// below 2 radius_mm + 1 <= 2001, their squares' sum below 2^24: 32-bit integers hold everything. keep_bits[w] = the ballot of records
// 64 w .. 64 w + 63 (a bit at or beyond the count is 0): as bytes, byte b = records 8 b .. 8 b + 7, what a lane of the emit takes.
__global__ __launch_bounds__(kBlockThreads)
void pcs_outlier_flag_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, int radius, uint32_t need,
                             const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ start, uint32_t slots,
                             const uint2* __restrict__ xyz, uint32_t capacity, unsigned long long* __restrict__ keep_bits)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    bool keep = false;
    if (i < ctl->tab.n_points) {
        const Xyz p = load_xyz(in, i);
        const int cx = cell_of(p.x, radius), cy = cell_of(p.y, radius), cz = cell_of(p.z, radius);
        const int r2 = radius * radius;
        uint32_t found = 0;
        for (int c = 0; c < 27 && found < need; c++) {
            const int cc = c + 13 < 27 ? c + 13 : c - 14;           // 13 = (0, 0, 0): the own cell first
            const int ax = cx + cc % 3 - 1, ay = cy + (cc / 3) % 3 - 1, az = cz + cc / 9 - 1;
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
            for (uint32_t m = start[at]; m < e && found < need; m++) {
                const uint2 q = xyz[m];
                const int dx = p.x - (int)(int16_t)(q.x & 0xFFFFu), dy = p.y - (int)(int16_t)(q.x >> 16), dz = p.z - (int)(int16_t)(q.y & 0xFFFFu);
                found += (uint32_t)(dx * dx + dy * dy + dz * dz <= r2);
            }
        }
        keep = found >= need;
    }
    const unsigned long long bits = __ballot(keep);
    if ((threadIdx.x & 63) == 0) keep_bits[i >> 6] = bits;
}

// ---- 7: kept records per tile -----------------------------------------------------------------------
__global__ __launch_bounds__(64)
void pcs_outlier_count_kernel(const OutlierCtl* __restrict__ ctl, const unsigned long long* __restrict__ keep_bits,
                              uint32_t* __restrict__ tile_counts)
{
    const uint32_t n = ctl->tab.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    const uint32_t pts = min(kTilePoints, n - tile0);
    // (a word whose first record is at or beyond the count may never have been written)
    const uint32_t c = threadIdx.x * 64u < pts ? (uint32_t)__popcll(keep_bits[(size_t)blockIdx.x * (kTilePoints / 64) + threadIdx.x]) : 0u;
    const uint32_t w = wave_sum(c);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = w;
}

// ---- 9: emit ----------------------------------------------------------------------------------------
// A tile's bytes into LDS at the INPUT's 16-byte phase, lane l takes records 8 l .. 8 l + 7 into registers, the kept ones are parked at
// the OUTPUT's phase and leave through store_staged: all 10 bytes of a record as they came, input order, nothing outside
// [out, out + 10 kept).
__global__ __launch_bounds__(kBlockThreads)
void pcs_outlier_emit_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, const uint8_t* __restrict__ keep_bytes,
                             const uint32_t* __restrict__ tile_prefix, uint8_t* __restrict__ out_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t wsum[4];
    const uint32_t n = ctl->tab.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    const uint32_t pts = min(kTilePoints, n - tile0);
    const uint8_t* gsrc = reinterpret_cast<const uint8_t*>(in) + (size_t)tile0 * PCS_POINT_BYTES;
    const uint32_t ihead = (uint32_t)((uintptr_t)gsrc & 15u);
    load_staged(stage, ihead, pts * PCS_POINT_BYTES, gsrc);
    __syncthreads();
    const uint32_t j0 = threadIdx.x * kPointsPerLane;
    const uint32_t keep = j0 < pts ? keep_bytes[(size_t)blockIdx.x * kBlockThreads + threadIdx.x] : 0u;
    Record rec[8];
#pragma unroll
    for (int k = 0; k < kPointsPerLane; k++) {
        rec[k] = Record{0u, 0u, 0u};
        if (j0 + (uint32_t)k < pts) rec[k] = unstage_record(stage, ihead + (j0 + (uint32_t)k) * PCS_POINT_BYTES);
    }
    uint32_t wave_total;
    const uint32_t ex = wave_exclusive_scan(__popc(keep), wave_total);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();                             // (and: everybody holds its records, the buffer is free)
    uint32_t before = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wsum[w];
    const uint32_t tile_kept = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    uint8_t* gdst = out_bytes + (size_t)tile_prefix[blockIdx.x] * PCS_POINT_BYTES;
    const uint32_t head = (uint32_t)((uintptr_t)gdst & 15u);
    uint32_t q = before + ex;
#pragma unroll
    for (int k = 0; k < kPointsPerLane; k++)
        if ((keep >> k) & 1u) stage_record(stage, head + (q++) * PCS_POINT_BYTES, rec[k]);
    __syncthreads();
    store_staged(stage, head, tile_kept * PCS_POINT_BYTES, gdst);
}

}  // namespace

uint32_t outlier_slots(uint32_t capacity)
{
    const uint64_t want = std::max<uint64_t>(2ull * capacity, 1);
    return (uint32_t)((want + kTilePoints - 1) / kTilePoints * kTilePoints);
}

size_t outlier_workspace_bytes(uint32_t capacity)
{
    const size_t slots = outlier_slots(capacity), tiles = (capacity + kTilePoints - 1) / kTilePoints;
    return up256(sizeof(OutlierCtl)) + up256(8 * slots) + up256(4 * (slots + 1)) + up256(4 * (slots / kTilePoints)) +
           2 * up256(4 * (size_t)capacity) + up256(8 * (size_t)capacity) + up256(tiles * kBlockThreads) + 2 * up256(4 * tiles);
}

namespace {

// Where the pieces of a workspace lie: the one carve the stage launchers and the two views read.
struct OutlierCarve {
    uint32_t            slots, tiles;
    OutlierCtl*         ctl;
    unsigned long long* keys;
    uint32_t*           count;
    uint32_t*           sums;
    uint32_t*           slot_of;
    uint32_t*           rank;
    uint2*              xyz;
    unsigned long long* keep_bits;
    uint32_t*           tile_counts;
    uint32_t*           tile_prefix;

    OutlierCarve(uint32_t capacity, void* d_ws) : slots(outlier_slots(capacity)), tiles((capacity + kTilePoints - 1) / kTilePoints)
    {
        uint8_t* w = static_cast<uint8_t*>(d_ws);
        auto carve = [&](size_t bytes) { uint8_t* p = w; w += up256(bytes); return p; };
        ctl         = reinterpret_cast<OutlierCtl*>(carve(sizeof(OutlierCtl)));
        keys        = reinterpret_cast<unsigned long long*>(carve(8 * (size_t)slots));
        count       = reinterpret_cast<uint32_t*>(carve(4 * ((size_t)slots + 1)));
        sums        = reinterpret_cast<uint32_t*>(carve(4 * (size_t)(slots / kTilePoints)));
        slot_of     = reinterpret_cast<uint32_t*>(carve(4 * (size_t)capacity));
        rank        = reinterpret_cast<uint32_t*>(carve(4 * (size_t)capacity));
        xyz         = reinterpret_cast<uint2*>(carve(8 * (size_t)capacity));
        keep_bits   = reinterpret_cast<unsigned long long*>(carve((size_t)tiles * kBlockThreads));
        tile_counts = reinterpret_cast<uint32_t*>(carve(4 * (size_t)tiles));
        tile_prefix = reinterpret_cast<uint32_t*>(carve(4 * (size_t)tiles));
    }
};

}  // namespace

const char* outlier_stage_name(int stage)
{
    static const char* const names[kOutlierStages] = {"clear", "insert", "cell sums", "cell scan", "cell starts", "scatter", "flag",
                                                      "tile count", "tile scan", "emit"};
    return stage >= 0 && stage < kOutlierStages ? names[stage] : "?";
}

namespace {

// What every stage launcher refuses: no capacity, a workspace too small or off the slab's 256-byte granularity.
bool bad_workspace(uint32_t capacity, const void* d_ws, size_t ws_bytes)
{
    return !capacity || ws_bytes < outlier_workspace_bytes(capacity) || ((uintptr_t)d_ws & 255u);
}

}  // namespace

hipError_t launch_cell_index_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                   int cell_mm, void* d_ws, size_t ws_bytes, hipStream_t st)
{
    if (bad_workspace(capacity, d_ws, ws_bytes) || cell_mm < 1 || cell_mm > 1000 || (!d_n_points && n_points > capacity))
        return hipErrorInvalidValue;
    const OutlierCarve cv(capacity, d_ws);
    const dim3 per_record((capacity + kBlockThreads - 1) / kBlockThreads), per_slot_tile(cv.slots / kTilePoints), block(kBlockThreads);
    switch (stage) {
    case 0:
        hipLaunchKernelGGL(pcs_outlier_clear_kernel, dim3(cv.slots / kBlockThreads + 1), block, 0, st, cv.ctl, d_n_points, n_points, capacity,
                           cv.keys, cv.count, cv.slots);
        break;
    case 1:
        hipLaunchKernelGGL(pcs_outlier_insert_kernel, per_record, block, 0, st, d_in, cv.ctl, cell_mm, cv.keys, cv.count, cv.slots, cv.slot_of,
                           cv.rank);
        break;
    case 2:
        hipLaunchKernelGGL(pcs_outlier_cell_sums_kernel, per_slot_tile, block, 0, st, cv.count, cv.sums);
        break;
    case 3:
        hipLaunchKernelGGL(pcs_outlier_cell_scan_kernel, dim3(1), dim3(1024), 0, st, cv.sums, cv.slots / kTilePoints, cv.count + cv.slots);
        break;
    case 4:
        hipLaunchKernelGGL(pcs_outlier_cell_starts_kernel, per_slot_tile, block, 0, st, cv.count, cv.sums);
        break;
    case 5:
        hipLaunchKernelGGL(pcs_outlier_scatter_kernel, per_record, block, 0, st, d_in, cv.ctl, cv.count, cv.slot_of, cv.rank, capacity, cv.xyz);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_outlier_compact_stage(int stage, const int16_t* d_in, uint32_t capacity, void* d_ws, size_t ws_bytes, int16_t* d_out,
                                        int32_t* d_out_points, hipStream_t st)
{
    if (bad_workspace(capacity, d_ws, ws_bytes)) return hipErrorInvalidValue;
    const OutlierCarve cv(capacity, d_ws);
    switch (stage) {
    case 7:
        hipLaunchKernelGGL(pcs_outlier_count_kernel, dim3(cv.tiles), dim3(64), 0, st, cv.ctl, cv.keep_bits, cv.tile_counts);
        break;
    case 8:     // the kept count is the scan's per-stream count: d_out_points[0], nothing behind it
        return launch_scan(&cv.ctl->tab, 1, 1, cv.tile_counts, cv.tile_prefix, nullptr, d_out_points, nullptr, st);
    case 9:
        hipLaunchKernelGGL(pcs_outlier_emit_kernel, dim3(cv.tiles), dim3(kBlockThreads), 0, st, d_in, cv.ctl,
                           reinterpret_cast<const uint8_t*>(cv.keep_bits), cv.tile_prefix, reinterpret_cast<uint8_t*>(d_out));
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_outlier_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                int radius_mm, int min_neighbors, void* d_ws, size_t ws_bytes, int16_t* d_out, int32_t* d_out_points,
                                hipStream_t st)
{
    if (bad_workspace(capacity, d_ws, ws_bytes) || radius_mm < 1 || radius_mm > 1000 || min_neighbors < 1 || min_neighbors > 255 ||
        (!d_n_points && n_points > capacity))
        return hipErrorInvalidValue;
    if (stage >= 0 && stage < kIndexStages)
        return launch_cell_index_stage(stage, d_in, n_points, d_n_points, capacity, radius_mm, d_ws, ws_bytes, st);
    if (stage != 6) return launch_outlier_compact_stage(stage, d_in, capacity, d_ws, ws_bytes, d_out, d_out_points, st);
    const OutlierCarve cv(capacity, d_ws);
    hipLaunchKernelGGL(pcs_outlier_flag_kernel, dim3((capacity + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, d_in, cv.ctl,
                       radius_mm, (uint32_t)min_neighbors + 1u, cv.keys, cv.count, cv.slots, cv.xyz, capacity, cv.keep_bits);
    return hipGetLastError();
}

hipError_t outlier_index_view(uint32_t capacity, void* d_ws, size_t ws_bytes, OutlierIndexView* view)
{
    if (!capacity || !view || ws_bytes < outlier_workspace_bytes(capacity) || ((uintptr_t)d_ws & 255u)) return hipErrorInvalidValue;
    const OutlierCarve cv(capacity, d_ws);
    *view = OutlierIndexView{cv.keys, cv.count, cv.xyz, cv.slots, capacity};
    return hipSuccess;
}

hipError_t outlier_keep_view(uint32_t capacity, void* d_ws, size_t ws_bytes, OutlierKeepView* view)
{
    if (!capacity || !view || ws_bytes < outlier_workspace_bytes(capacity) || ((uintptr_t)d_ws & 255u)) return hipErrorInvalidValue;
    const OutlierCarve cv(capacity, d_ws);
    *view = OutlierKeepView{cv.ctl, cv.keep_bits, cv.tile_prefix};
    return hipSuccess;
}

}  // namespace pcs
