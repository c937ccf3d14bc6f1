// pcs_kernels_plan.hip — plan-view maps of a packed payload: an orthographic projection along a coordinate axis into a dense raster of
// W x H cells, per cell the record count, the raw up coordinate of its top and of its bottom record and the top record's colour
// (pcs_plan_view_device; DESIGN.md section 3 "Plan-view maps" and section 5). Not in the reference: the definition is this project's
// own. The arithmetic per record is pcs_plan_math.h; the workspace holds one 64-bit key per cell for the top and one for the bottom.
//   clear       one lane per cell: both keys and the count raster's word to zero; lane 0 writes the statistics block (considered = n)
//   accumulate  one lane per record, a tile of kPlanTilePoints = 8192 per workgroup (32 per lane: four times the other families' tile,
//               because what a tile combines on chip it does not send: consecutive raster rows land in the same cells). Equal cells
//               are combined on chip before anything leaves the CU: up to kPlanRounds = 2 groups of a wave's lanes (the cell of the first lane still to do, as pcs_boxes_moments_kernel groups
//               lanes by object) are reduced across the wave — a count, a DPP maximum and minimum of the height, the lowest lane among
//               the equals — and one lane carries the group; every lane left over carries its own record. Either way the update goes
//               into the workgroup's LDS table (kPlanSlots = 1024 slots keyed by cell, a multiplicative hash, at most kPlanProbes = 4
//               linear probes), with LDS atomics: add, 64-bit unsigned max twice. A record that finds no slot goes to the global words itself:
//               a crowded table costs speed, never bits. At the tile's end every occupied slot is flushed once: one global add without
//               return on the count word, and a 64-bit unsigned max without return per key that the word does not already meet.
//   resolve     one lane per cell: the keys decoded, the top record's colour fetched from the payload, the three other rasters
//               written, occupied / fullest reduced per workgroup and folded into the statistics block
// Properties:
//   determinism   a count, an unsigned maximum over keys that carry the index as the tie-break: associative and commutative, so the
//               bytes depend on nothing but the input, whatever order the atomics arrive in and whichever path a record took.
//   bounds      a record index stays below the clamped count; a cell index comes from plan_cell (< W * H) alone; an LDS slot is
//               masked; resolve reads the payload at an index a key carries, which is the index of a record accumulate read.
//   No scratch.

#include <algorithm>
#include <climits>

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"
#include "pcs_plan_math.h"

namespace pcs {

namespace {

constexpr int kWaves = kBlockThreads / 64;
constexpr uint32_t kPlanSlots = 1024;         // 24 bytes each: 24 KiB of LDS per workgroup
constexpr uint32_t kPlanSlotBits = 10;
constexpr int kPlanProbes = 4;
constexpr uint32_t kPlanPointsPerLane = 32;
constexpr uint32_t kPlanTilePoints = kPlanPointsPerLane * kBlockThreads;      // 8192 (tests/plan_view_cases.py: TILE)
constexpr int kPlanRounds = 2;
constexpr uint32_t kNoCell = 0xFFFFFFFFu;
static_assert(kPlanSlots == 1u << kPlanSlotBits, "the hash keeps the product's top bits");
static_assert(kPlanSlots % kBlockThreads == 0, "init and flush walk the table in whole strides");

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint32_t clamped_count(const int32_t* d_n, uint32_t n_host, uint32_t capacity)
{
    if (!d_n) return n_host;
    const int32_t v = *d_n;
    return v < 0 ? 0u : min((uint32_t)v, capacity);
}

// Wavefront-wide minimum / maximum (wave-uniform), all 64 lanes active: wave_inclusive_scan's moves with the fold's identity where a
// lane has no source.
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
void pcs_plan_clear_kernel(const int32_t* __restrict__ d_n, uint32_t n_host, uint32_t capacity, uint32_t cells,
                           unsigned long long* __restrict__ top, unsigned long long* __restrict__ bottom, uint32_t* __restrict__ count,
                           long long* __restrict__ stats)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i < cells) {
        top[i] = 0ull;
        bottom[i] = 0ull;
        count[i] = 0u;
    }
    if (i < 8u) stats[i] = i == 0u ? (long long)clamped_count(d_n, n_host, capacity) : 0ll;
}

// ---- accumulate -------------------------------------------------------------------------------------
// The cell's three global words: the count without return, a key only where the word does not meet it yet (a relaxed look first: a wall
// cell is met after its first few tiles, and what is not sent does not queue on its address).
__device__ __forceinline__ void global_update(uint32_t cell, uint32_t cnt, unsigned long long kt, unsigned long long kb,
                                              unsigned long long* top, unsigned long long* bottom, uint32_t* count)
{
    (void)__hip_atomic_fetch_add(count + cell, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_load(top + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kt)
        (void)__hip_atomic_fetch_max(top + cell, kt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_load(bottom + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kb)
        (void)__hip_atomic_fetch_max(bottom + cell, kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct PlanTable {
    unsigned long long top[kPlanSlots], bottom[kPlanSlots];
    uint32_t cell[kPlanSlots], count[kPlanSlots];
};

// cnt records of `cell` with the keys kt / kb into the workgroup's table; past kPlanProbes taken slots, into the global words.
__device__ __forceinline__ void table_update(PlanTable& t, uint32_t cell, uint32_t cnt, unsigned long long kt, unsigned long long kb,
                                             unsigned long long* top, unsigned long long* bottom, uint32_t* count)
{
    uint32_t slot = (cell * 2654435761u) >> (32u - kPlanSlotBits);
    for (int probe = 0; probe < kPlanProbes; probe++) {
        const uint32_t was = atomicCAS(&t.cell[slot], kNoCell, cell);
        if (was == kNoCell || was == cell) {
            (void)__hip_atomic_fetch_add(&t.count[slot], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            (void)__hip_atomic_fetch_max(&t.top[slot], kt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            (void)__hip_atomic_fetch_max(&t.bottom[slot], kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return;
        }
        slot = (slot + 1u) & (kPlanSlots - 1u);
    }
    global_update(cell, cnt, kt, kb, top, bottom, count);
}

__global__ __launch_bounds__(kBlockThreads)
void pcs_plan_accumulate_kernel(const int16_t* __restrict__ in, const int32_t* __restrict__ d_n, uint32_t n_host, uint32_t capacity,
                                PlanArgs P, unsigned long long* top, unsigned long long* bottom, uint32_t* count, long long* stats)
{
    __shared__ PlanTable table;
    __shared__ uint32_t part[kWaves][2];
    for (uint32_t s = threadIdx.x; s < kPlanSlots; s += kBlockThreads) {
        table.cell[s] = kNoCell;
        table.count[s] = 0u;
        table.top[s] = 0ull;
        table.bottom[s] = 0ull;
    }
    __syncthreads();
    const uint32_t n = clamped_count(d_n, n_host, capacity);
    uint32_t in_band = 0u, mapped = 0u;
    for (uint32_t c = 0; c < kPlanPointsPerLane; c++) {
        const uint32_t i = (blockIdx.x * kPlanPointsPerLane + c) * kBlockThreads + threadIdx.x;
        const bool live = i < n;
        if (!__ballot(live)) break;                          // (records ascend: nothing live behind this either)
        int cell = -1, hb = 0;
        if (live) {
            const Xyz p = load_xyz(in, i);
            const int up = plan_up(P, p.x, p.y, p.z);
            if (plan_in_band(P, up)) {
                in_band++;
                cell = plan_cell(P, p.x, p.y, p.z);
                hb = plan_hb(P, up);
            }
        }
        bool todo_lane = cell >= 0;
        mapped += todo_lane ? 1u : 0u;
        unsigned long long todo = __ballot(todo_lane);
        const uint32_t i0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i - lane_id()));      // lane L holds record i0 + L
        for (int round = 0; round < kPlanRounds && todo; round++) {       // wave-uniform
            const int lead = __ffsll((long long)todo) - 1;
            const int c0 = __builtin_amdgcn_readlane(cell, lead);
            const bool in_group = todo_lane && cell == c0;
            const unsigned long long group = __ballot(in_group);
            const int hi = wave_max(in_group ? hb : INT_MIN), lo = wave_min(in_group ? hb : INT_MAX);
            const int lane_hi = __ffsll((long long)__ballot(in_group && hb == hi)) - 1;
            const int lane_lo = __ffsll((long long)__ballot(in_group && hb == lo)) - 1;
            if (lane_id() == (uint32_t)lead)
                table_update(table, (uint32_t)c0, (uint32_t)__popcll(group), plan_top_key(hi, i0 + (uint32_t)lane_hi),
                             plan_bottom_key(lo, i0 + (uint32_t)lane_lo), top, bottom, count);
            todo_lane = todo_lane && !in_group;
            todo &= ~group;
        }
        if (todo_lane) table_update(table, (uint32_t)cell, 1u, plan_top_key(hb, i), plan_bottom_key(hb, i), top, bottom, count);
    }
    in_band = wave_sum(in_band);
    mapped = wave_sum(mapped);
    if (lane_id() == 0u) {
        part[threadIdx.x >> 6][0] = in_band;
        part[threadIdx.x >> 6][1] = mapped;
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kPlanSlots; s += kBlockThreads) {
        const uint32_t cell = table.cell[s];
        if (cell != kNoCell) global_update(cell, table.count[s], table.top[s], table.bottom[s], top, bottom, count);
    }
    if (threadIdx.x < 2u) {
        uint32_t total = 0u;
        for (int w = 0; w < kWaves; w++) total += part[w][threadIdx.x];
        if (total)
            (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(stats + 1 + threadIdx.x), (unsigned long long)total,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- resolve ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_plan_resolve_kernel(const int16_t* __restrict__ in, uint32_t capacity, PlanArgs P, uint32_t cells,
                             const unsigned long long* __restrict__ top, const unsigned long long* __restrict__ bottom,
                             const uint32_t* __restrict__ count, int16_t* __restrict__ top_out, int16_t* __restrict__ bottom_out,
                             uint8_t* __restrict__ rgb, long long* stats)
{
    __shared__ uint32_t part[kWaves][2];
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t cnt = 0u;
    if (i < cells) {
        cnt = count[i];
        const unsigned long long kt = top[i], kb = bottom[i];
        int t = 0, b = 0;
        uint32_t r = 0u, g = 0u, bl = 0u;
        const uint32_t at = plan_key_index(kt);
        if (cnt && kt && kb && at < capacity) {
            t = plan_top_raw(P, kt);
            b = plan_bottom_raw(P, kb);
            const uint16_t* rec = reinterpret_cast<const uint16_t*>(in) + (size_t)at * PCS_POINT_SHORTS;
            const uint32_t rg = rec[3];
            r = rg & 0xFFu; g = rg >> 8; bl = rec[4] & 0xFFu;
        }
        top_out[i] = (int16_t)t;
        bottom_out[i] = (int16_t)b;
        rgb[3 * (size_t)i] = (uint8_t)r;
        rgb[3 * (size_t)i + 1] = (uint8_t)g;
        rgb[3 * (size_t)i + 2] = (uint8_t)bl;
    }
    const uint32_t occupied = wave_sum(cnt ? 1u : 0u);
    const int fullest = wave_max((int)cnt);                  // a count is at most kMaxPoints < 2^31
    if (lane_id() == 0u) {
        part[threadIdx.x >> 6][0] = occupied;
        part[threadIdx.x >> 6][1] = (uint32_t)fullest;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t occ = 0u, full = 0u;
        for (int w = 0; w < kWaves; w++) {
            occ += part[w][0];
            full = max(full, part[w][1]);
        }
        if (occ) {
            (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(stats + 3), (unsigned long long)occ, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned long long)__hip_atomic_load(stats + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < full)
                (void)__hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(stats + 4), (unsigned long long)full, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

dim3 grid_over(uint32_t n) { return dim3((std::max(n, 1u) + kBlockThreads - 1) / kBlockThreads); }
dim3 tiles_over(uint32_t n) { return dim3((std::max(n, 1u) + kPlanTilePoints - 1) / kPlanTilePoints); }

struct PlanWs { unsigned long long *top, *bottom; };
PlanWs carve(void* d_ws, uint32_t cells)
{
    uint8_t* w = static_cast<uint8_t*>(d_ws);
    return PlanWs{reinterpret_cast<unsigned long long*>(w), reinterpret_cast<unsigned long long*>(w + up256(8 * (size_t)cells))};
}

bool bad_map(const PlanArgs& P, const void* d_ws, const uint32_t* d_count, const long long* d_stats)
{
    return P.width < 1 || P.height < 1 || P.width > kPlanSideMax || P.height > kPlanSideMax || (int64_t)P.width * P.height > kPlanCellsMax ||
           !d_ws || ((uintptr_t)d_ws & 7u) || !d_count || ((uintptr_t)d_count & 3u) || !d_stats || ((uintptr_t)d_stats & 7u);
}

}  // namespace

size_t plan_workspace_bytes(uint32_t cells) { return 2 * up256(8 * (size_t)cells); }

hipError_t launch_plan_clear(uint32_t n_points, const int32_t* d_n_points, uint32_t capacity, const PlanArgs& P, void* d_ws, uint32_t* d_count,
                             long long* d_stats, hipStream_t st)
{
    if (bad_map(P, d_ws, d_count, d_stats) || (!d_n_points && n_points > capacity)) return hipErrorInvalidValue;
    const uint32_t cells = (uint32_t)(P.width * P.height);
    const PlanWs ws = carve(d_ws, cells);
    hipLaunchKernelGGL(pcs_plan_clear_kernel, grid_over(cells), dim3(kBlockThreads), 0, st, d_n_points, n_points, capacity, cells, ws.top,
                       ws.bottom, d_count, d_stats);
    return hipGetLastError();
}

hipError_t launch_plan_accumulate(const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity, const PlanArgs& P,
                                  void* d_ws, uint32_t* d_count, long long* d_stats, hipStream_t st)
{
    if (bad_map(P, d_ws, d_count, d_stats) || (capacity && !d_in) || ((uintptr_t)d_in & 1u) || (!d_n_points && n_points > capacity) ||
        P.cell_mm < 1 || P.cell_mm > 32767 || P.magic != plan_magic(P.cell_mm) || P.up_axis < 0 || P.up_axis > 2)
        return hipErrorInvalidValue;
    const PlanWs ws = carve(d_ws, (uint32_t)(P.width * P.height));
    hipLaunchKernelGGL(pcs_plan_accumulate_kernel, tiles_over(capacity), dim3(kBlockThreads), 0, st, d_in, d_n_points, n_points, capacity, P,
                       ws.top, ws.bottom, d_count, d_stats);
    return hipGetLastError();
}

hipError_t launch_plan_resolve(const int16_t* d_in, uint32_t capacity, const PlanArgs& P, const void* d_ws, const uint32_t* d_count,
                               int16_t* d_top, int16_t* d_bottom, uint8_t* d_rgb, long long* d_stats, hipStream_t st)
{
    if (bad_map(P, d_ws, d_count, d_stats) || (capacity && !d_in) || ((uintptr_t)d_in & 1u) || !d_top || ((uintptr_t)d_top & 1u) || !d_bottom ||
        ((uintptr_t)d_bottom & 1u) || !d_rgb)
        return hipErrorInvalidValue;
    const uint32_t cells = (uint32_t)(P.width * P.height);
    const PlanWs ws = carve(const_cast<void*>(d_ws), cells);
    hipLaunchKernelGGL(pcs_plan_resolve_kernel, grid_over(cells), dim3(kBlockThreads), 0, st, d_in, capacity, P, cells, ws.top, ws.bottom,
                       d_count, d_top, d_bottom, d_rgb, d_stats);
    return hipGetLastError();
}

}  // namespace pcs
