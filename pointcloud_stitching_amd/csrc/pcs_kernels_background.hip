// pcs_kernels_background.hip — a learned background model of a fixed rig and its subtraction from a packed payload
// (pcs_background_learn_device, pcs_background_subtract_device; DESIGN.md section 3 "Background model and subtraction" and section 5).
// Not in the reference, and no PCL filter stands behind it: the definition is this project's own. Everything is in the payload's
// integer millimetres: cell coordinate = floor(v / cell_mm) + 32768 per axis, key = the three side by side (cell_of, cell_key of
// pcs_outlier_index.h). The model is a PERSISTENT open-addressing table key -> seen, probed from first_slot as the cell index is:
// learned once, probed per record, no index build per call.
//   clear      keys[] = empty, seen[] = stamp[] = 0, the control block zeroed (create, reset)
//   learn      one lane per record: find or claim the cell's slot (linear probing, a 64-bit compare-and-swap on the key), then
//              old = exchange(stamp[slot], frame): only a lane that sees old != frame adds 1 to seen[slot] — one lane per cell and call
//   flag       one lane per record: the own cell first, with dilate the 26 others (clipped at 0 and 65535, never wrapped), out at the
//              first cell with seen >= min_seen; the wave's ballot is 64 keep bits in the radius filter's layout (OutlierKeepView);
//              lane 0 of the grid leaves the clamped record count in that filter's control block, as its stage 0 does
//   (compaction: launch_outlier_compact_stage's three launches, pcs_kernels_outlier.hip — no emit kernel here)
//   stats      one lane: the eight int64 of the statistics block
//   gather     one lane per slot: occupied slots through an atomic cursor into a staging array, any order (the host sorts by key)
//   import     learn's find-or-claim over a container's entries, storing seen
// In learn and flag a lane whose key equals its lower neighbour's in the wave (neighbouring records are neighbouring pixels) does not
// probe: a cross-lane move of the key (DPP, no LDS), and in flag the run's first lane's answer taken from the ballots.
// Properties:
//   determinism   seen[] is a count of CALLS: the exchange on stamp[] lets exactly one lane per cell and call add, whatever the arrival
//                 order and however many records share the cell (skipped lanes included: their run's first lane stands for them). Which
//                 slot of a probe sequence a cell takes depends on arrival order; nothing that leaves the table does (export sorts).
//   no hang       every probe loop runs at most `slots` steps. A lane that finds neither its key nor an empty slot sets the sticky
//                 overflow flag and gives up; so does a claim that takes the cell count above max_cells. No write outside the table.
//   overflow      a model with the flag set keeps every record in subtract (both modes) and says so in the statistics
//   cost          learn: one probe sequence, one exchange and at most one add per run of equal keys in a wave. flag: one probe sequence
//                 per run for background (the bulk on a static rig), up to 27 for foreground with dilate 1.
//   workspace     the table is the model's own allocation, not a context slab: slots = 2048 ceil(2 max_cells / 2048), 8 (key) + 4 (seen)
//                 + 4 (stamp) bytes per slot = about 32 bytes per max_cells, plus a 256-byte control block. subtract borrows the radius
//                 filter's slab for the keep bits and tile words (outlier_workspace_bytes). No scratch memory in any kernel.
// Integer arithmetic throughout: no float is converted, compared or stored anywhere in this file.

#include <algorithm>

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"

namespace pcs {

namespace {

// the value of lane - 1 (lane 0 of the wave: 0). All 64 lanes must be active.
__device__ __forceinline__ unsigned long long lower_lane(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xf, 0xf, false);           // wave_shr:1
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xf, 0xf, false);
    return (unsigned long long)lo | (unsigned long long)hi << 32;
}

__device__ __forceinline__ uint32_t clamped_count(const int32_t* d_n, uint32_t n_host, uint32_t capacity)
{
    if (!d_n) return n_host;
    const int32_t v = *d_n;
    return v < 0 ? 0u : min((uint32_t)v, capacity);
}

__device__ __forceinline__ void set_overflow(BackgroundCtl* ctl)
{
    __hip_atomic_store(&ctl->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot of `key`, claimed if the table does not hold it yet (the cell count goes up by one then). kNoSlot: the table is full.
// A slot's key is written once (empty -> key) and never again until a clear: a key read here is final, an "empty" read may be stale
// and the compare-and-swap settles it.
__device__ __forceinline__ uint32_t find_or_claim(const BackgroundTable& t, unsigned long long key)
{
    uint32_t s = first_slot(key, t.slots);
    for (uint32_t probe = 0; probe < t.slots; probe++) {
        unsigned long long k = __hip_atomic_load(t.keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kEmptyKey) {
            unsigned long long expected = kEmptyKey;
            if (__hip_atomic_compare_exchange_strong(t.keys + s, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                k = key;
                if (__hip_atomic_fetch_add(&t.ctl->cells, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= t.max_cells) set_overflow(t.ctl);
            } else {
                k = expected;
            }
        }
        if (k == key) return s;
        s = s + 1u == t.slots ? 0u : s + 1u;
    }
    set_overflow(t.ctl);
    return kNoSlot;
}

// ---- clear ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_background_clear_kernel(BackgroundTable t)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i == 0) *t.ctl = BackgroundCtl{0u, 0u, 0u, 0u};
    if (i < t.slots) {
        t.keys[i] = kEmptyKey;
        t.seen[i] = 0u;
        t.stamp[i] = 0u;
    }
}

// ---- learn ------------------------------------------------------------------------------------------
// frame: 1 .. 65535, this call's number; stamp[] holds the last call that touched a cell (0: none since the clear or the import).
__global__ __launch_bounds__(kBlockThreads)
void pcs_background_learn_kernel(BackgroundTable t, const int16_t* __restrict__ in, const int32_t* __restrict__ d_n, uint32_t n_host,
                                 uint32_t capacity, uint32_t frame)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t n = clamped_count(d_n, n_host, capacity);
    const bool valid = i < n;
    unsigned long long key = kEmptyKey;
    if (valid) {
        const Xyz p = load_xyz(in, i);
        key = cell_key(cell_of(p.x, t.cell_mm), cell_of(p.y, t.cell_mm), cell_of(p.z, t.cell_mm));
    }
    const unsigned long long below = lower_lane(key);
    if (!valid || ((threadIdx.x & 63u) != 0u && below == key)) return;       // the lower lane holds the same cell: it, or its run's first, learns it
    const uint32_t s = find_or_claim(t, key);
    if (s == kNoSlot) return;
    if (__hip_atomic_exchange(t.stamp + s, frame, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != frame)
        __hip_atomic_fetch_add(t.seen + s, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- import -----------------------------------------------------------------------------------------
// entries: a validated container's, 12 bytes each at a 4-byte aligned address: cx | cy << 16, cz (| 0 << 16), seen. The keys are
// distinct (strictly ascending): every lane claims a slot of its own.
__global__ __launch_bounds__(kBlockThreads)
void pcs_background_import_kernel(BackgroundTable t, const uint32_t* __restrict__ entries, uint32_t n_entries)
{
    const uint32_t e = blockIdx.x * kBlockThreads + threadIdx.x;
    if (e >= n_entries) return;
    const uint32_t w0 = entries[3 * (size_t)e], w1 = entries[3 * (size_t)e + 1], w2 = entries[3 * (size_t)e + 2];
    const uint32_t s = find_or_claim(t, (unsigned long long)w0 | (unsigned long long)(w1 & 0xFFFFu) << 32);
    if (s != kNoSlot) t.seen[s] = w2;
}

// ---- flag -------------------------------------------------------------------------------------------
// keep_bits[w] = the ballot of records 64 w .. 64 w + 63, a bit at or beyond the count 0 (pcs_outlier_flag_kernel's layout).
// keep_background: PCS_BACKGROUND_MODE_KEEP. The table is only read: nothing learns on the stream while this runs.
__global__ __launch_bounds__(kBlockThreads)
void pcs_background_flag_kernel(BackgroundTable t, const int16_t* __restrict__ in, OutlierCtl* __restrict__ ctl,
                                const int32_t* __restrict__ d_n, uint32_t n_host, uint32_t capacity, uint32_t min_seen, int dilate,
                                bool keep_background, unsigned long long* __restrict__ keep_bits)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t n = clamped_count(d_n, n_host, capacity);
    if (i == 0) {
        ctl->tab.n_points = n;
        ctl->tab.tile_base = 0u;
    }
    const bool valid = i < n;
    const bool overflow = t.ctl->overflow != 0u;
    int cx = 0, cy = 0, cz = 0;
    unsigned long long own = kEmptyKey;
    if (valid) {
        const Xyz p = load_xyz(in, i);
        cx = cell_of(p.x, t.cell_mm); cy = cell_of(p.y, t.cell_mm); cz = cell_of(p.z, t.cell_mm);
        own = cell_key(cx, cy, cz);
    }
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = lower_lane(own);                  // (every lane of the wave is still here)
    const bool head = valid && (lane == 0u || below != own);
    bool background = false;
    if (head && !overflow) {
        const int cells = dilate ? 27 : 1;
        for (int c = 0; c < cells && !background; c++) {
            const int cc = c + 13 < 27 ? c + 13 : c - 14;               // 13 = (0, 0, 0): the own cell first
            const int ax = cx + cc % 3 - 1, ay = cy + (cc / 3) % 3 - 1, az = cz + cc / 9 - 1;
            if ((uint32_t)ax > 65535u || (uint32_t)ay > 65535u || (uint32_t)az > 65535u) continue;   // no such cell: skipped, never wrapped
            const unsigned long long key = cell_key(ax, ay, az);
            uint32_t s = first_slot(key, t.slots);
            for (uint32_t probe = 0; probe < t.slots; probe++) {       // ends at the key or at the first empty slot; at most `slots` steps
                const unsigned long long k = t.keys[s];
                if (k == key) background = t.seen[s] >= min_seen;
                if (k == key || k == kEmptyKey) break;
                s = s + 1u == t.slots ? 0u : s + 1u;
            }
        }
    }
    // a lane's answer is its run's first lane's: the highest head at or below it (validity is monotone in the lane: lane 0 of a
    // wave with any valid lane is a head)
    const unsigned long long heads = __ballot(head), answers = __ballot(background);
    const unsigned long long at_or_below = heads & (~0ull >> (63u - lane));
    const uint32_t first = at_or_below ? 63u - (uint32_t)__clzll((long long)at_or_below) : 0u;
    const bool mine = ((answers >> first) & 1ull) != 0ull;
    const bool keep = valid && (overflow || mine == keep_background);
    const unsigned long long bits = __ballot(keep);
    if (lane == 0u) keep_bits[i >> 6] = bits;
}

// ---- stats ------------------------------------------------------------------------------------------
// considered, kept, background, cells, frames, min_seen, overflow, reserved (0). An overflowed model judged nothing: background 0.
__global__ __launch_bounds__(64)
void pcs_background_stats_kernel(BackgroundTable t, const OutlierCtl* __restrict__ ctl, const int32_t* __restrict__ d_kept, uint32_t frames,
                                 uint32_t min_seen, bool keep_background, long long* __restrict__ stats)
{
    if (threadIdx.x != 0) return;
    const long long n = ctl->tab.n_points, kept = *d_kept;
    const bool overflow = t.ctl->overflow != 0u;
    stats[0] = n;
    stats[1] = kept;
    stats[2] = overflow ? 0 : keep_background ? kept : n - kept;
    stats[3] = t.ctl->cells;
    stats[4] = frames;
    stats[5] = min_seen;
    stats[6] = overflow ? 1 : 0;
    stats[7] = 0;
}

// ---- export gather ----------------------------------------------------------------------------------
// staging[j] = (key low, key high, seen, 0) of the j-th occupied slot to arrive; entries beyond `room` are counted, not written.
__global__ __launch_bounds__(kBlockThreads)
void pcs_background_gather_kernel(BackgroundTable t, uint4* __restrict__ staging, uint32_t room)
{
    const uint32_t s = blockIdx.x * kBlockThreads + threadIdx.x;
    if (s >= t.slots) return;
    const unsigned long long k = t.keys[s];
    if (k == kEmptyKey) return;
    const uint32_t j = __hip_atomic_fetch_add(&t.ctl->cursor, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j < room) staging[j] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), t.seen[s], 0u);
}

bool bad_table(const BackgroundTable& t)
{
    return !t.keys || !t.seen || !t.stamp || !t.ctl || !t.slots || t.slots % kTilePoints || t.slots != background_slots(t.max_cells) ||
           t.cell_mm < 1 || t.cell_mm > 1000;
}

dim3 grid_over(uint32_t n) { return dim3((n + kBlockThreads - 1) / kBlockThreads); }

}  // namespace

uint32_t background_slots(uint32_t max_cells)
{
    const uint64_t want = std::max<uint64_t>(2ull * max_cells, 1);
    return (uint32_t)((want + kTilePoints - 1) / kTilePoints * kTilePoints);
}

size_t background_table_bytes(uint32_t max_cells)
{
    const size_t slots = background_slots(max_cells);
    return up256(sizeof(BackgroundCtl)) + up256(8 * slots) + 2 * up256(4 * slots);
}

BackgroundTable background_table(void* d_table, int cell_mm, uint32_t max_cells)
{
    BackgroundTable t{};
    t.slots = background_slots(max_cells);
    t.max_cells = max_cells;
    t.cell_mm = cell_mm;
    uint8_t* w = static_cast<uint8_t*>(d_table);
    auto carve = [&](size_t bytes) { uint8_t* p = w; w += up256(bytes); return p; };
    t.ctl   = reinterpret_cast<BackgroundCtl*>(carve(sizeof(BackgroundCtl)));
    t.keys  = reinterpret_cast<unsigned long long*>(carve(8 * (size_t)t.slots));
    t.seen  = reinterpret_cast<uint32_t*>(carve(4 * (size_t)t.slots));
    t.stamp = reinterpret_cast<uint32_t*>(carve(4 * (size_t)t.slots));
    return t;
}

const char* background_launch_name(int launch)
{
    static const char* const names[] = {"flag", "tile count", "tile scan", "emit", "stats"};
    return launch >= 0 && launch < 5 ? names[launch] : "?";
}

hipError_t launch_background_clear(const BackgroundTable& t, hipStream_t st)
{
    if (bad_table(t)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_background_clear_kernel, grid_over(t.slots), dim3(kBlockThreads), 0, st, t);
    return hipGetLastError();
}

hipError_t launch_background_learn(const BackgroundTable& t, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points,
                                   uint32_t capacity, uint32_t frame, hipStream_t st)
{
    if (bad_table(t) || !capacity || !d_in || frame < 1 || frame > 65535 || (!d_n_points && n_points > capacity)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_background_learn_kernel, grid_over(capacity), dim3(kBlockThreads), 0, st, t, d_in, d_n_points, n_points, capacity,
                       frame);
    return hipGetLastError();
}

hipError_t launch_background_import(const BackgroundTable& t, const void* d_entries, uint32_t n_entries, hipStream_t st)
{
    if (bad_table(t) || !n_entries || n_entries > t.max_cells || !d_entries || ((uintptr_t)d_entries & 3u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_background_import_kernel, grid_over(n_entries), dim3(kBlockThreads), 0, st, t,
                       static_cast<const uint32_t*>(d_entries), n_entries);
    return hipGetLastError();
}

hipError_t launch_background_flag(const BackgroundTable& t, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points,
                                  uint32_t capacity, int min_seen, int dilate, int mode, void* d_ws, size_t ws_bytes, hipStream_t st)
{
    if (bad_table(t) || !capacity || !d_in || min_seen < 1 || min_seen > 65535 || (dilate != 0 && dilate != 1) || (mode != 0 && mode != 1) ||
        (!d_n_points && n_points > capacity))
        return hipErrorInvalidValue;
    OutlierKeepView kv{};
    if (hipError_t e = outlier_keep_view(capacity, d_ws, ws_bytes, &kv)) return e;
    hipLaunchKernelGGL(pcs_background_flag_kernel, grid_over(capacity), dim3(kBlockThreads), 0, st, t, d_in,
                       const_cast<OutlierCtl*>(kv.ctl) /* the workspace is this call's */, d_n_points, n_points, capacity, (uint32_t)min_seen,
                       dilate, mode == 1, kv.keep_bits);
    return hipGetLastError();
}

hipError_t launch_background_stats(const BackgroundTable& t, uint32_t capacity, void* d_ws, size_t ws_bytes, const int32_t* d_out_points,
                                   uint32_t frames, int min_seen, int mode, long long* d_stats, hipStream_t st)
{
    if (bad_table(t) || !d_out_points || !d_stats) return hipErrorInvalidValue;
    OutlierKeepView kv{};
    if (hipError_t e = outlier_keep_view(capacity, d_ws, ws_bytes, &kv)) return e;
    hipLaunchKernelGGL(pcs_background_stats_kernel, dim3(1), dim3(64), 0, st, t, kv.ctl, d_out_points, frames, (uint32_t)min_seen, mode == 1,
                       d_stats);
    return hipGetLastError();
}

hipError_t launch_background_gather(const BackgroundTable& t, void* d_staging, uint32_t room, hipStream_t st)
{
    if (bad_table(t) || !d_staging || ((uintptr_t)d_staging & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_background_gather_kernel, grid_over(t.slots), dim3(kBlockThreads), 0, st, t, static_cast<uint4*>(d_staging), room);
    return hipGetLastError();
}

}  // namespace pcs
