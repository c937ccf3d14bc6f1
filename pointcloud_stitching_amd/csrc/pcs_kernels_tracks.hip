// pcs_kernels_tracks.hip — object tracks: persistent identities for the objects of pcs_cluster_objects_device* across frame-sets
// (pcs_tracker_update_device; DESIGN.md section 3 "Object tracks" and section 5). Not in the reference: the definition is this
// project's own. The evidence is per record: which of the last frame-set's objects occupied the cell this record is in now. Cells
// are the background model's (cell_of, cell_key of pcs_outlier_index.h); both tables are open-addressing tables probed from
// first_slot, as that model's is.
//   clear      both maps and the pair table empty, id / age / best / keeper zero, the control block fresh (create, reset)
//   records    the hot path, one lane per record: the key once; P(t-1) probed read-only; the cell found or claimed in P(t) and k
//              folded into it by an atomic minimum. A lane whose (key, k) equals its lower neighbour's in the wave does neither: the
//              run's first lane does, once (DPP compare, ballots, clz). Every lane then takes its run head's j, and the wave finds
//              or claims each DISTINCT pair (k, j) it holds once and adds the number of its lanes that vote for it: a wave mostly
//              holds one. The launch also zeroes best[] and keeper[] for the launches behind it.
//   choose     one lane per pair slot: best[k] = max(votes << 32 | ~j): most votes, then the smallest j. The lane empties its pair
//              slot and its slot of P(t-1) behind it, so that no clear launch stands in an update.
//   claim      one lane per k: keeper[j] = max(votes << 32 | ~k) over the k whose choice is j: most votes, then the smallest k
//   assign     one workgroup: k continues j iff keeper[choice(k)] names k and the votes reach min_votes; a ballot scan ranks the born;
//              tracks[], the new id / age arrays, next_id, the statistics block; the control block made ready for the next update
// Properties:
//   determinism   counts are sums and the folds are max / min: no output depends on arrival order or on which slot a key took.
//   no hang       every probe loop runs at most `slots` steps; a lane that finds neither its key nor an empty slot sets the table's
//                 overflow flag and gives up; assign sets it where the claims of the update exceed max_cells. No write outside the tables.
//   overflow      pairs: this update continues nothing. cells of P(t): the next update reads neither that map nor the pair table.
//   counters      the update's four counts (taking-part, voted, claimed cells, claimed pairs) are striped over 64 words 128 bytes
//                 apart: one add per wave or per claim, none of them queueing on one address (with one word each the record
//                 pass took 2.6 ms instead of 0.8: DESIGN.md section 10, f17); assign folds them
//   workspace     the tracker's own allocation (tracker_bytes): 36 bytes per slot, 40 per object, 32 KB of counters, a 256-byte
//                 control block. No scratch.
// Integer arithmetic throughout: no float is converted, compared or stored anywhere in this file.

#include <algorithm>

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"

namespace pcs {

namespace {

constexpr uint32_t kNoObject = 0xFFFFFFFFu;

struct Track { long long id; int32_t age, prev, votes, reserved; };
static_assert(sizeof(Track) == sizeof(pcs_track), "pcs_track is 24 bytes");

// the value of lane - 1 (lane 0 of the wave: 0). All 64 lanes must be active.
__device__ __forceinline__ uint32_t lower_lane32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);           // wave_shr:1
}

__device__ __forceinline__ uint32_t clamped_count(const int32_t* d_n, uint32_t n_host, uint32_t capacity)
{
    if (!d_n) return n_host;
    const int32_t v = *d_n;
    return v < 0 ? 0u : min((uint32_t)v, capacity);
}

enum Counter : uint32_t { kConsidered = 0, kVoted = 1, kCells = 2, kPairs = 3 };

// stripe `stripe` of counter `which`: one word per 128 bytes, so that the adds of different waves do not queue on one address
__device__ __forceinline__ uint32_t* counter(const TrackerView& t, Counter which, uint32_t stripe)
{
    return t.counters + ((uint32_t)which * kTrackStripes + (stripe & (kTrackStripes - 1u))) * kTrackStripeWords;
}

// The slot of `key` in keys[slots], claimed if the table does not hold it yet (the stripe of `claims` that the slot picks goes up by
// one then; assign compares their sum with max_cells). kNoSlot: the table is full (flag set). A slot's key is written once between
// two clears: a key read here is final, an "empty" read may be stale and the compare-and-swap settles it.
__device__ __forceinline__ uint32_t find_or_claim(const TrackerView& t, unsigned long long* keys, uint32_t slots, unsigned long long key,
                                                  Counter claims, uint32_t* overflow)
{
    uint32_t s = first_slot(key, slots);
    for (uint32_t probe = 0; probe < slots; probe++) {
        unsigned long long k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kEmptyKey) {
            unsigned long long expected = kEmptyKey;
            if (__hip_atomic_compare_exchange_strong(keys + s, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                k = key;
                __hip_atomic_fetch_add(counter(t, claims, s), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                k = expected;
            }
        }
        if (k == key) return s;
        s = s + 1u == slots ? 0u : s + 1u;
    }
    __hip_atomic_store(overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return kNoSlot;
}

// ---- clear ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_track_clear_kernel(TrackerView t, long long first_id)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i == 0) {
        TrackCtl fresh{};
        fresh.next_id = first_id;
        *t.ctl = fresh;
    }
    if (i < t.slots) {
        t.prev_keys[i] = kEmptyKey; t.prev_val[i] = kNoObject;
        t.cur_keys[i] = kEmptyKey;  t.cur_val[i] = kNoObject;
        t.pair_keys[i] = kEmptyKey; t.pair_count[i] = 0u;
    }
    if (i < t.max_objects) {
        const_cast<long long*>(t.prev_id)[i] = 0; const_cast<int32_t*>(t.prev_age)[i] = 0;
        t.cur_id[i] = 0; t.cur_age[i] = 0;
        t.best[i] = 0ull; t.keeper[i] = 0ull;
    }
    if (i < kTrackCounterWords) t.counters[i] = 0u;
}

// ---- records ----------------------------------------------------------------------------------------
// The grid covers max(capacity, t.max_objects) lanes. No lane leaves before the cross-lane moves.
__global__ __launch_bounds__(kBlockThreads)
void pcs_track_records_kernel(TrackerView t, const int16_t* __restrict__ in, const int32_t* __restrict__ d_n, uint32_t n_host,
                              uint32_t capacity, const int32_t* __restrict__ object_of, const int32_t* __restrict__ d_m, uint32_t max_objects)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i < t.max_objects) {                                           // what choose, claim and assign of this update fold into
        t.best[i] = 0ull;
        t.keeper[i] = 0ull;
    }
    const uint32_t n = clamped_count(d_n, n_host, capacity);
    const uint32_t m = clamped_count(d_m, 0u, max_objects);
    const bool probe_prev = t.ctl->m != 0u && t.ctl->prev_overflow == 0u;
    uint32_t k = kNoObject;
    unsigned long long key = kEmptyKey;
    bool active = false;
    if (i < n) {
        k = (uint32_t)object_of[i];
        active = k < m;                                                // -1 and everything at or beyond m: ignored
        if (active) {
            const Xyz p = load_xyz(in, i);
            key = cell_key(cell_of(p.x, t.cell_mm), cell_of(p.y, t.cell_mm), cell_of(p.z, t.cell_mm));
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t below_lo = lower_lane32((uint32_t)key), below_hi = lower_lane32((uint32_t)(key >> 32)), below_k = lower_lane32(k);
    const bool same = below_lo == (uint32_t)key && below_hi == (uint32_t)(key >> 32) && below_k == k;
    const bool head = active && (lane == 0u || !same);
    const unsigned long long heads = __ballot(head), actives = __ballot(active);
    uint32_t j = kNoObject;
    if (head) {
        if (probe_prev) {
            uint32_t s = first_slot(key, t.slots);
            for (uint32_t probe = 0; probe < t.slots; probe++) {       // ends at the key or at the first empty slot; at most `slots` steps
                const unsigned long long pk = t.prev_keys[s];
                if (pk == key) j = t.prev_val[s];
                if (pk == key || pk == kEmptyKey) break;
                s = s + 1u == t.slots ? 0u : s + 1u;
            }
        }
        const uint32_t cs = find_or_claim(t, t.cur_keys, t.slots, key, kCells, &t.ctl->cur_overflow);
        if (cs != kNoSlot) __hip_atomic_fetch_min(t.cur_val + cs, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // a taking-part lane's answer is its run's first lane's: the highest head at or below it (an ignored lane's is not used)
    const unsigned long long at_or_below = heads & (~0ull >> (63u - lane));
    const uint32_t first = at_or_below ? 63u - (uint32_t)__clzll((long long)at_or_below) : 0u;
    const uint32_t j_mine = (uint32_t)__shfl((int)j, (int)first);
    const bool votes = active && j_mine != kNoObject;
    const unsigned long long voted = __ballot(votes);
    // one add per distinct pair of the wave, not one per run: the lanes of a wave mostly vote for one pair, and every run's add
    // would queue on that pair's count (measured: 0.79 ms per run against 0.28 ms per pair). `left` is wave-uniform: every lane walks the loop.
    for (unsigned long long left = voted; left;) {
        const int leader = __builtin_ctzll(left);
        const uint32_t lk = (uint32_t)__shfl((int)k, leader), lj = (uint32_t)__shfl((int)j_mine, leader);
        const unsigned long long same_pair = __ballot(votes && k == lk && j_mine == lj);
        if (lane == (uint32_t)leader) {
            const uint32_t ps = find_or_claim(t, t.pair_keys, t.slots, (unsigned long long)lk << 32 | lj, kPairs, &t.ctl->pair_overflow);
            if (ps != kNoSlot)
                __hip_atomic_fetch_add(t.pair_count + ps, (uint32_t)__popcll(same_pair), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        left &= ~same_pair;
    }
    if (lane == 0u && actives) {
        const uint32_t wave = i >> 6;
        __hip_atomic_fetch_add(counter(t, kConsidered, wave), (uint32_t)__popcll(actives), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (voted) __hip_atomic_fetch_add(counter(t, kVoted, wave), (uint32_t)__popcll(voted), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- choose -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_track_choose_kernel(TrackerView t)
{
    const uint32_t s = blockIdx.x * kBlockThreads + threadIdx.x;
    if (s >= t.slots) return;
    const unsigned long long pair = t.pair_keys[s];
    if (pair != kEmptyKey) {
        const uint32_t k = (uint32_t)(pair >> 32), j = (uint32_t)pair, votes = t.pair_count[s];
        if (votes && k < t.max_objects)
            __hip_atomic_fetch_max(t.best + k, (unsigned long long)votes << 32 | (0xFFFFFFFFu - j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t.pair_keys[s] = kEmptyKey;
        t.pair_count[s] = 0u;
    }
    if (t.prev_keys[s] != kEmptyKey) {                                 // P(t-1) has been read: the next update builds its map here
        t.prev_keys[s] = kEmptyKey;
        t.prev_val[s] = kNoObject;
    }
}

// ---- claim ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_track_claim_kernel(TrackerView t, const int32_t* __restrict__ d_m, uint32_t max_objects)
{
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    if (k >= clamped_count(d_m, 0u, max_objects)) return;
    const unsigned long long b = t.best[k];
    if (!b) return;
    const uint32_t j = 0xFFFFFFFFu - (uint32_t)b;
    if (j < t.max_objects)
        __hip_atomic_fetch_max(t.keeper + j, (b & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFu - k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- assign -----------------------------------------------------------------------------------------
// One workgroup. stats: considered, voted, objects, continued, born, lost, overflow, frames.
__global__ __launch_bounds__(kBlockThreads)
void pcs_track_assign_kernel(TrackerView t, const int32_t* __restrict__ d_m, uint32_t max_objects, uint32_t min_votes, long long frames,
                             Track* __restrict__ tracks, long long* __restrict__ stats)
{
    constexpr int kWaves = kBlockThreads / 64;
    static_assert(kWaves == (int)kTrackCounters && kTrackStripes == 64u, "one wave folds one counter, one lane per stripe");
    __shared__ uint32_t wave_born[kWaves], wave_continued[kWaves], counts[kTrackCounters];
    TrackCtl* const ctl = t.ctl;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    {   // the four striped counts, folded and zeroed for the next update
        uint32_t* const word = t.counters + threadIdx.x * kTrackStripeWords;
        uint32_t v = *word;
        *word = 0u;
        for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0u) counts[wave] = v;
        __syncthreads();
    }
    const uint32_t m = clamped_count(d_m, 0u, max_objects);
    const uint32_t m_prev = ctl->m;
    const bool pair_overflow = ctl->pair_overflow != 0u || counts[kPairs] > t.max_cells, prev_overflow = ctl->prev_overflow != 0u;
    const bool cur_overflow = ctl->cur_overflow != 0u || counts[kCells] > t.max_cells;
    const bool none = pair_overflow || prev_overflow || m_prev == 0u;
    const long long next_id = ctl->next_id;
    uint32_t born_before = 0u, continued = 0u;
    for (uint32_t base = 0; base < m; base += kBlockThreads) {
        const uint32_t k = base + threadIdx.x;
        const bool in = k < m;
        bool cont = false;
        uint32_t j = 0u, votes = 0u;
        if (in && !none) {
            const unsigned long long b = t.best[k];
            if (b) {
                votes = (uint32_t)(b >> 32);
                j = 0xFFFFFFFFu - (uint32_t)b;
                cont = j < m_prev && votes >= min_votes && t.keeper[j] == ((b & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFu - k));
            }
        }
        const unsigned long long born_bits = __ballot(in && !cont), cont_bits = __ballot(cont);
        if (lane == 0u) {
            wave_born[wave] = (uint32_t)__popcll(born_bits);
            wave_continued[wave] = (uint32_t)__popcll(cont_bits);
        }
        __syncthreads();
        uint32_t rank = born_before + (uint32_t)__popcll(born_bits & ((1ull << lane) - 1ull));
        for (int w = 0; w < kWaves; w++) {
            if ((uint32_t)w < wave) rank += wave_born[w];
            born_before += wave_born[w];
            continued += wave_continued[w];
        }
        if (in) {
            Track tr;
            if (cont) {
                const int32_t age = t.prev_age[j];
                tr = Track{t.prev_id[j], age == INT32_MAX ? INT32_MAX : age + 1, (int32_t)j, (int32_t)votes, 0};
            } else {
                tr = Track{next_id + (long long)rank, 0, -1, 0, 0};
            }
            tracks[k] = tr;
            t.cur_id[k] = tr.id;
            t.cur_age[k] = tr.age;
        }
        __syncthreads();
    }
    __syncthreads();                       // (with m = 0 no step above has one: every lane has read the control block by now)
    if (threadIdx.x != 0) return;
    const long long overflow = (pair_overflow ? 1 : 0) | (prev_overflow ? 2 : 0);
    if (stats) {
        stats[0] = counts[kConsidered];
        stats[1] = counts[kVoted];
        stats[2] = m;
        stats[3] = continued;
        stats[4] = born_before;
        stats[5] = m_prev - continued;
        stats[6] = overflow;
        stats[7] = frames;
    }
    TrackCtl next{};
    next.next_id = next_id + (long long)born_before;
    next.m = m;
    next.prev_overflow = cur_overflow ? 1u : 0u;
    next.last_overflow = (uint32_t)overflow;
    *ctl = next;
}

bool bad_view(const TrackerView& t)
{
    return !t.prev_keys || !t.prev_val || !t.cur_keys || !t.cur_val || !t.pair_keys || !t.pair_count || !t.prev_id || !t.prev_age ||
           !t.cur_id || !t.cur_age || !t.best || !t.keeper || !t.ctl || !t.counters || !t.slots || t.slots != background_slots(t.max_cells) ||
           !t.max_objects || t.max_objects > PCS_CLUSTER_OBJECTS_MAX || t.cell_mm < 1 || t.cell_mm > 1000;
}

dim3 grid_over(uint32_t n) { return dim3((std::max(n, 1u) + kBlockThreads - 1) / kBlockThreads); }

}  // namespace

size_t tracker_bytes(uint32_t max_cells, uint32_t max_objects)
{
    const size_t slots = background_slots(max_cells);
    return up256(sizeof(TrackCtl)) + 3 * (up256(8 * slots) + up256(4 * slots)) + 4 * up256(8 * (size_t)max_objects) +
           2 * up256(4 * (size_t)max_objects) + up256(4 * (size_t)kTrackCounterWords);
}

TrackerView tracker_view(void* d_tracker, int cell_mm, uint32_t max_cells, uint32_t max_objects, int parity)
{
    TrackerView t{};
    t.slots = background_slots(max_cells);
    t.max_cells = max_cells;
    t.max_objects = max_objects;
    t.cell_mm = cell_mm;
    uint8_t* w = static_cast<uint8_t*>(d_tracker);
    auto carve = [&](size_t bytes) { uint8_t* p = w; w += up256(bytes); return p; };
    t.ctl = reinterpret_cast<TrackCtl*>(carve(sizeof(TrackCtl)));
    unsigned long long* keys[2]; uint32_t* val[2]; long long* id[2]; int32_t* age[2];
    for (int p = 0; p < 2; p++) {
        keys[p] = reinterpret_cast<unsigned long long*>(carve(8 * (size_t)t.slots));
        val[p]  = reinterpret_cast<uint32_t*>(carve(4 * (size_t)t.slots));
    }
    t.pair_keys  = reinterpret_cast<unsigned long long*>(carve(8 * (size_t)t.slots));
    t.pair_count = reinterpret_cast<uint32_t*>(carve(4 * (size_t)t.slots));
    for (int p = 0; p < 2; p++) id[p] = reinterpret_cast<long long*>(carve(8 * (size_t)max_objects));
    for (int p = 0; p < 2; p++) age[p] = reinterpret_cast<int32_t*>(carve(4 * (size_t)max_objects));
    t.best   = reinterpret_cast<unsigned long long*>(carve(8 * (size_t)max_objects));
    t.keeper = reinterpret_cast<unsigned long long*>(carve(8 * (size_t)max_objects));
    t.counters = reinterpret_cast<uint32_t*>(carve(4 * (size_t)kTrackCounterWords));
    const int prev = parity & 1, cur = prev ^ 1;
    t.prev_keys = keys[prev]; t.prev_val = val[prev]; t.prev_id = id[prev]; t.prev_age = age[prev];
    t.cur_keys  = keys[cur];  t.cur_val  = val[cur];  t.cur_id  = id[cur];  t.cur_age  = age[cur];
    return t;
}

hipError_t launch_track_clear(const TrackerView& t, long long first_id, hipStream_t st)
{
    if (bad_view(t) || first_id < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_track_clear_kernel, grid_over(std::max({t.slots, t.max_objects, kTrackCounterWords})), dim3(kBlockThreads), 0, st, t, first_id);
    return hipGetLastError();
}

hipError_t launch_track_records(const TrackerView& t, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                const int32_t* d_object_of, const int32_t* d_n_objects, uint32_t max_objects, hipStream_t st)
{
    if (bad_view(t) || !d_n_objects || max_objects > t.max_objects || (capacity && (!d_in || !d_object_of)) ||
        (!d_n_points && n_points > capacity))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_track_records_kernel, grid_over(std::max(capacity, t.max_objects)), dim3(kBlockThreads), 0, st, t, d_in,
                       d_n_points, n_points, capacity, d_object_of, d_n_objects, max_objects);
    return hipGetLastError();
}

hipError_t launch_track_choose(const TrackerView& t, hipStream_t st)
{
    if (bad_view(t)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_track_choose_kernel, grid_over(t.slots), dim3(kBlockThreads), 0, st, t);
    return hipGetLastError();
}

hipError_t launch_track_claim(const TrackerView& t, const int32_t* d_n_objects, uint32_t max_objects, hipStream_t st)
{
    if (bad_view(t) || !d_n_objects || max_objects > t.max_objects) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_track_claim_kernel, grid_over(max_objects), dim3(kBlockThreads), 0, st, t, d_n_objects, max_objects);
    return hipGetLastError();
}

hipError_t launch_track_assign(const TrackerView& t, const int32_t* d_n_objects, uint32_t max_objects, uint32_t min_votes, long long frames,
                               void* d_tracks, long long* d_stats, hipStream_t st)
{
    if (bad_view(t) || !d_n_objects || max_objects > t.max_objects || (max_objects && !d_tracks) || ((uintptr_t)d_tracks & 7u) || !min_votes)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_track_assign_kernel, dim3(1), dim3(kBlockThreads), 0, st, t, d_n_objects, max_objects, min_votes, frames,
                       static_cast<Track*>(d_tracks), d_stats);
    return hipGetLastError();
}

}  // namespace pcs
