// pcs_kernels_cluster.hip — Euclidean cluster extraction on a packed payload (pcs_cluster_filter_device, pcs_cluster_labels_device;
// DESIGN.md section 3 "Euclidean clusters" and section 5): records i and j are adjacent iff d^2 <= tolerance_mm^2, a cluster is a
// connected component of that relation, size(i) its record count, label(i) the smallest input index in it; the filter keeps the
// records of the clusters whose size lies in min_size..max_size (max_size 0: no upper bound). Everything in the payload's integer
// millimetres. Not in the reference; modelled on PCL's EuclideanClusterExtraction, parity unpinned.
//
// The neighbour search walks the radius filter's index (launch_cell_index_stage's six launches with cell edge tolerance_mm,
// pcs_outlier_index.h). The components come from a lock-free union-find over CELL-ORDER POSITIONS p, the entries of xyz[]:
//   init       parent[p] = p, size[p] = 0, minrec[p] = all ones; the statistics block (where one is asked for) zeroed, considered set
//   union      one lane per xyz[] entry, in cell order (a wave's lanes are members of the same few cells and walk the same few runs):
//              its 27 cells, minus those whose nearest possible member is beyond the tolerance; every member q < p within the
//              tolerance is united with p. Each adjacent pair is seen once, by its larger position.
//   roots      parent[p] = p's root (a walk without stores), final: the union launch is complete. size[root] += 1, one add per
//              distinct root of a wave, the first root a wave meets saved up over a tile of 2048 positions.
//   flag       (filter) one lane per input record: its position is any entry of its cell's run with its coordinates (equal records
//              share a root); the size of its root against min_size / max_size to the wave's ballot: keep_bits[] of the radius
//              filter's layout, whose stages 7 to 9 (tile count, scan, emit) run unchanged behind it
//   stats      (filter, optional) over the positions: the roots counted, those of kept clusters, the largest size, one atomic per
//              tile of 2048 positions and word into the caller's block; the kept count from the scan's word
//   label roots  (labels) one lane per input record: its root into labels[i], minrec[root] = min(minrec[root], i)
//   labels     (labels) labels[i] = minrec[labels[i]], sizes[i] = size[root], the records that label themselves counted
//
// The union-find. parent[] holds positions; parent[p] <= p always, equality marks a root. Three kinds of access in the union launch,
// all relaxed agent-scope atomics (one L2 per XCD: a plain load may be served by a line another XCD has since written):
//   link     compare-and-swap parent[hi]: hi -> lo with lo < hi. It succeeds only while hi is a root, so only roots are ever linked.
//   halve    store parent[p] = g, where a = parent[p] != p and g = parent[a] != a were read before. It targets non-roots only.
//   read     a load may return an OLDER value of the word than the newest.
// Why any interleaving gives the components:
//   (1) A non-root never becomes a root again: both writes store a value smaller than the word's index.
//   (2) No cycle: every edge points to a smaller position.
//   (3) "x and y are in one tree" (they reach the same root), once true, stays true. A link joins two trees whole. A halve moves p
//       under g, which was an ancestor of p when it was read — in p's tree then, so by (3) itself at the time of the store: p's
//       subtree moves inside its own tree. Hence a stale read only ever yields an older ancestor, a member of the same tree.
//   (4) Trees only ever join records that a chain of adjacent pairs connects (a link joins the trees of an adjacent pair), and when
//       unite(p, q) returns, p and q are in one tree: it returns on equal roots or on its own successful link. A "root" that find
//       returns from a stale read may no longer be one: as `hi` the compare-and-swap refuses it and hands back the newer parent, from
//       which the loop goes on; as `lo` it still is a member of q's (or p's) tree below hi, which is all a link needs.
//   (5) So at the launch's end the trees are exactly the components, and by (2) a tree's root is its smallest position.
//   Progress: a failed compare-and-swap means another lane linked hi; at most n - 1 links ever succeed.
// Properties:
//   determinism   which lane links which root, the shape of the trees and the order of a cell's run depend on timing; the partition,
//                 the sizes (integer adds) and the smallest input index of a cluster (an integer minimum) do not. The labels form
//                 renames the roots by that minimum; the filter reads sizes only.
//   no hang       every probe loop runs at most `slots` steps; find walks strictly downwards; unite: see Progress
//   bounds        a lane reads xyz[p], p < n; runs are clipped to min(start[at + 1], n), so every position that enters parent[] is
//                 below n, where init wrote; parent[], size[], minrec[] have `capacity` >= n words. Nothing at or beyond the count is
//                 read as a record; labels[], sizes[] are written below n only.
//   cost          a record costs the population of the cells around it that it cannot rule out, and two finds per adjacent member
//                 below it. No early exit: a cell of m members costs m^2 / 2 distance tests by definition (n identical records: n^2 / 2).
// Workspace behind the radius filter's (outlier_workspace_bytes): 4 N (parent) + 4 N (size) + 4 N (minrec) + 256 (the host form's
// statistics block in its first 64 bytes) = 12 bytes per record. Integer arithmetic throughout: no float anywhere in this file.
//
// The object table (pcs_cluster_objects_device; DESIGN.md section 3 "Cluster objects"): six launches behind `roots`, stages 16 to 21
// of launch_cluster_object_stage. An OBJECT is a cluster whose size passes the filter; objects are numbered by ascending label.
//   record roots  one lane per input record below the device count: rootof[i] = its root (position_of, as `label roots`),
//                 minrec[root] = min(i) by the same ballot / readlane grouping, the load in front of the atomic minimum
//   firsts        per tile of 2048 records: first_bits[] (keep_bits' layout, a bitmap of its own) = "i is the first record of an
//                 object" (minrec[root] == i and the size passes), the tile's count; a first of a cluster that is no object writes
//                 slot[root] = -1
//   first scan    launch_scan over those counts: the tile prefixes, the total into the caller's n_objects
//   slots         a first's rank among the firsts, in record order, is its object's k: slot[root] = k; for k < max_objects the
//                 accumulator acc[k] is set up (an empty box, zero sums, the root)
//   accumulate    one lane per input record: k = slot[rootof[i]] to object_of[i]; the wave's lanes grouped by k, a group reduced in
//                 registers and sent as one atomic per word; the first object a wave meets is held back over the tile, combined
//                 across the workgroup through LDS and sent once per tile and word. k >= max_objects has no accumulator: skipped.
//   finish        one lane per k < min(n_objects, max_objects): the 80-byte entry from acc[k], minrec[root] and size[root]
// Properties of these launches:
//   determinism   minrec[root] is an integer minimum; the firsts' bitmap is indexed by the record, so a first's rank — k — depends on
//                 the partition and the record order alone. Every accumulator word is the minimum, the maximum or the 64-bit sum of
//                 the same multiset of integers however the lanes are grouped and whatever order the atomics arrive in: integer
//                 min, max and add are associative and commutative, and nothing wraps (a tile's partial is below 2^26 in 32 bits,
//                 |sum| < 2^47 in 64). So the table, n_objects and object_of are the same bytes on every run.
//   no hang       position_of's probe and run loops are bounded as above; every ballot loop clears at least its leader's bit per
//                 round: at most 64 rounds; the other loops run kPointsPerLane or four times
//   bounds        rootof[], slot[], object_of[] are indexed below the device count n <= capacity (slot[] by a root, a position below
//                 n); first_bits[] has a word per 64 records of capacity, tile words one per tile of capacity; acc[] is indexed by
//                 k < max_objects only; objects[] by k < min(n_objects, max_objects) only
// Workspace behind the above (cluster_objects_workspace_bytes): 4 N (rootof) + 4 N (slot) + N / 8 (first_bits) + 8 per tile of 2048
// records + 80 per object of max_objects + 256 = 8.13 bytes per record and 80 per object.

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"

namespace pcs {

namespace {

constexpr uint32_t kNoRecord = 0xFFFFFFFFu;

// the slot of a cell's key, kNoSlot where the index has no such cell (pcs_kernels_normals.hip's)
__device__ __forceinline__ uint32_t find_slot(const unsigned long long* __restrict__ keys, uint32_t slots, unsigned long long key)
{
    uint32_t s = first_slot(key, slots);
    for (uint32_t probe = 0; probe < slots; probe++) {       // ends at the key or at the first empty slot; at most `slots` steps
        const unsigned long long k = keys[s];
        if (k == key) return s;
        if (k == kEmptyKey) break;
        s = s + 1u == slots ? 0u : s + 1u;
    }
    return kNoSlot;
}

__device__ __forceinline__ uint32_t uf_load(const uint32_t* parent, uint32_t p)
{
    return __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A root of p's tree (the root, unless the last load was stale), halving the path on the way: every store targets a word that was
// read as a non-root and writes an ancestor read behind it.
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t p)
{
    for (;;) {
        const uint32_t a = uf_load(parent, p);
        if (a == p) return p;
        const uint32_t g = uf_load(parent, a);
        if (g == a) return a;
        __hip_atomic_store(parent + p, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        p = g;
    }
}

// p's and q's trees become one; returns a root of it (the smaller of the two, or the common one).
__device__ __forceinline__ uint32_t uf_unite(uint32_t* parent, uint32_t p, uint32_t q)
{
    for (;;) {
        const uint32_t a = uf_find(parent, p), b = uf_find(parent, q);
        if (a == b) return a;
        const uint32_t hi = max(a, b), lo = min(a, b);
        uint32_t expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return lo;
        p = expected;            // hi was linked meanwhile: go on from its parent
        q = lo;
    }
}

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// ---- init -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_init_kernel(const OutlierCtl* __restrict__ ctl, uint32_t* __restrict__ parent, uint32_t* __restrict__ size,
                             uint32_t* __restrict__ minrec, long long* __restrict__ stats)
{
    const uint32_t p = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t n = ctl->tab.n_points;
    if (stats && p < 8u) stats[p] = p == 0u ? (long long)n : 0ll;
    if (p >= n) return;
    parent[p] = p;
    size[p] = 0u;
    minrec[p] = kNoRecord;
}

// ---- union ------------------------------------------------------------------------------------------
// Differences of members of adjacent cells are below 2 tolerance_mm + 1 <= 2001, their squares' sum below 2^24.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_union_kernel(const OutlierCtl* __restrict__ ctl, int tol, const unsigned long long* __restrict__ keys,
                              const uint32_t* __restrict__ start, uint32_t slots, const uint2* __restrict__ xyz, uint32_t* parent)
{
    const uint32_t p = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t n = ctl->tab.n_points;
    if (p >= n) return;
    const uint2 w = xyz[p];
    const int px = (int)(int16_t)(w.x & 0xFFFFu), py = (int)(int16_t)(w.x >> 16), pz = (int)(int16_t)(w.y & 0xFFFFu);
    const int t2 = tol * tol;
    const int cx = cell_of(px, tol), cy = cell_of(py, tol), cz = cell_of(pz, tol);
    // per axis: how far a member of the cell one step down / in the same cell / one step up is at least (the normals kernel's)
    const int fx = px - (cx - 32768) * tol, fy = py - (cy - 32768) * tol, fz = pz - (cz - 32768) * tol;
    const auto gap = [tol](int f, int o) { return o == 0 ? f + 1 : o == 1 ? 0 : tol - f; };
    uint32_t mine = p;                                       // a member of p's tree, its root as of the last unite
    for (int c = 0; c < 27; c++) {
        const int ox = c % 3, oy = (c / 3) % 3, oz = c / 9;
        const int ex = gap(fx, ox), ey = gap(fy, oy), ez = gap(fz, oz);
        if (ex * ex + ey * ey + ez * ez > t2) continue;
        const int ax = cx + ox - 1, ay = cy + oy - 1, az = cz + oz - 1;
        if ((uint32_t)ax > 65535u || (uint32_t)ay > 65535u || (uint32_t)az > 65535u) continue;   // no such cell: skipped, never wrapped
        const uint32_t at = find_slot(keys, slots, cell_key(ax, ay, az));
        if (at == kNoSlot) continue;
        const uint32_t end = min(min(start[at + 1u], n), p);             // members below p only: a pair belongs to its larger position
        for (uint32_t q = start[at]; q < end; q++) {
            const uint2 v = xyz[q];
            const int dx = (int)(int16_t)(v.x & 0xFFFFu) - px, dy = (int)(int16_t)(v.x >> 16) - py, dz = (int)(int16_t)(v.y & 0xFFFFu) - pz;
            if (dx * dx + dy * dy + dz * dz > t2) continue;
            mine = uf_unite(parent, mine, q);
        }
    }
}

// ---- roots ------------------------------------------------------------------------------------------
// The forest is final when this launch starts: nobody links any more, a word read as a root is one. The walk stores nothing (a
// halving store of one lane could land on parent[p] after lane p's own and leave a mere ancestor there); parent[p] is written by
// lane p alone, with the root, so a walk through it reads the old parent or the root (atomics: lanes read words others store).
// size[]: a workgroup takes a tile of 2048 positions, 256 at a time. The lanes of a wave that share a root add once, by the first of
// them; the first root a wave meets is HELD: its count is saved up over the tile and added once at the end (one cluster that holds most
// of the cloud would otherwise take an add per wave and 256 positions on one word: 1.2 ms of the launch at 6.7 M records).
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_roots_kernel(const OutlierCtl* __restrict__ ctl, uint32_t* parent, uint32_t* __restrict__ size)
{
    const uint32_t n = ctl->tab.n_points;
    uint32_t held = kNoRecord, held_count = 0u;              // wave-uniform
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t p = (blockIdx.x * kPointsPerLane + c) * kBlockThreads + threadIdx.x;
        const bool live = p < n;
        uint32_t r = 0u;
        if (live) {
            r = p;
            for (uint32_t up = uf_load(parent, r); up != r; up = uf_load(parent, r)) r = up;
            if (r != p) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned long long todo = __ballot(live);
        if (!todo) break;                                    // (positions ascend: nothing live behind this either)
        if (held == kNoRecord) held = (uint32_t)__builtin_amdgcn_readlane((int)r, __ffsll((long long)todo) - 1);
        const unsigned long long mine = __ballot(live && r == held);
        held_count += (uint32_t)__popcll(mine);
        todo &= ~mine;
        while (todo) {                                       // wave-uniform: one round per other distinct root among the wave's lanes
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);
            const unsigned long long same = __ballot(live && r == r0);
            if ((int)lane_id() == leader) atomicAdd(size + r0, (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
    if (held != kNoRecord && lane_id() == 0u) atomicAdd(size + held, held_count);
}

// the position of record (x, y, z) in the index: any entry of its cell's run with its coordinates; kNoRecord: none (cannot happen)
__device__ __forceinline__ uint32_t position_of(const Xyz& p, int tol, const unsigned long long* __restrict__ keys,
                                                const uint32_t* __restrict__ start, uint32_t slots, const uint2* __restrict__ xyz, uint32_t n)
{
    const uint2 want = make_uint2((uint32_t)(uint16_t)p.x | (uint32_t)(uint16_t)p.y << 16, (uint32_t)(uint16_t)p.z);
    const uint32_t at = find_slot(keys, slots, cell_key(cell_of(p.x, tol), cell_of(p.y, tol), cell_of(p.z, tol)));
    if (at == kNoSlot) return kNoRecord;
    const uint32_t end = min(start[at + 1u], n);
    for (uint32_t k = start[at]; k < end; k++) {
        const uint2 q = xyz[k];
        if (q.x == want.x && q.y == want.y) return k;
    }
    return kNoRecord;
}

// ---- flag -------------------------------------------------------------------------------------------
// keep_bits[w] = the ballot of records 64 w .. 64 w + 63 (a bit at or beyond the count is 0): the radius filter's layout.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_flag_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, int tol, uint32_t min_size, uint32_t max_size,
                             const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ start, uint32_t slots,
                             const uint2* __restrict__ xyz, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                             unsigned long long* __restrict__ keep_bits)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t n = ctl->tab.n_points;
    bool keep = false;
    if (i < n) {
        const uint32_t k = position_of(load_xyz(in, i), tol, keys, start, slots, xyz, n);
        if (k != kNoRecord) {
            const uint32_t r = parent[k];
            const uint32_t s = r < n ? size[r] : 0u;
            keep = s >= min_size && (max_size == 0u || s <= max_size);
        }
    }
    const unsigned long long bits = __ballot(keep);
    if ((threadIdx.x & 63) == 0) keep_bits[i >> 6] = bits;
}

// ---- stats ------------------------------------------------------------------------------------------
// stats[] = considered (init wrote it), clusters, kept_clusters, largest, kept, 0, 0, 0; init zeroed words 1 to 7. A workgroup takes a
// tile of 2048 positions and adds once per word.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_stats_kernel(const OutlierCtl* __restrict__ ctl, uint32_t min_size, uint32_t max_size, const uint32_t* __restrict__ parent,
                              const uint32_t* __restrict__ size, const int32_t* __restrict__ kept, unsigned long long* __restrict__ stats)
{
    __shared__ uint32_t wsum[(kBlockThreads / 64) * 3];
    const uint32_t n = ctl->tab.n_points;
    uint32_t roots = 0u, passing = 0u, largest = 0u;
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t p = (blockIdx.x * kPointsPerLane + c) * kBlockThreads + threadIdx.x;
        if (p < n && parent[p] == p) {
            const uint32_t s = size[p];
            roots++;
            passing += (uint32_t)(s >= min_size && (max_size == 0u || s <= max_size));
            largest = max(largest, s);
        }
    }
    roots = wave_sum(roots);
    passing = wave_sum(passing);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) largest = max(largest, (uint32_t)__shfl_xor((int)largest, d, 64));
    if (lane_id() == 0u) {
        wsum[(threadIdx.x >> 6) * 3 + 0] = roots;
        wsum[(threadIdx.x >> 6) * 3 + 1] = passing;
        wsum[(threadIdx.x >> 6) * 3 + 2] = largest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot[3] = {0u, 0u, 0u};
        for (uint32_t w = 0; w < kBlockThreads / 64; w++) {
            tot[0] += wsum[w * 3 + 0];
            tot[1] += wsum[w * 3 + 1];
            tot[2] = max(tot[2], wsum[w * 3 + 2]);
        }
        if (tot[0]) {
            atomicAdd(stats + 1, (unsigned long long)tot[0]);
            if (tot[1]) atomicAdd(stats + 2, (unsigned long long)tot[1]);
            atomicMax(stats + 3, (unsigned long long)tot[2]);
        }
        if (blockIdx.x == 0) stats[4] = (unsigned long long)(long long)*kept;
    }
}

// ---- label roots ------------------------------------------------------------------------------------
// labels[i] = the root's position for the next launch; minrec[root] = the smallest i. A wave's records ascend with the lane, so the
// first lane of those that share a root holds their minimum.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_label_roots_kernel(const int16_t* __restrict__ in, uint32_t n, int tol, const unsigned long long* __restrict__ keys,
                                    const uint32_t* __restrict__ start, uint32_t slots, const uint2* __restrict__ xyz,
                                    const uint32_t* __restrict__ parent, uint32_t* __restrict__ minrec, int32_t* __restrict__ labels,
                                    int32_t* __restrict__ n_clusters)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i == 0u) *n_clusters = 0;
    uint32_t r = kNoRecord;
    if (i < n) {
        const uint32_t k = position_of(load_xyz(in, i), tol, keys, start, slots, xyz, n);
        if (k != kNoRecord) { r = parent[k]; if (r >= n) r = kNoRecord; }
        labels[i] = (int32_t)r;
    }
    unsigned long long todo = __ballot(r != kNoRecord);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);
        const unsigned long long same = __ballot(r == r0);
        // (waves run roughly in record order: most find a smaller index already there and leave the word alone)
        if ((int)lane_id() == leader && uf_load(minrec, r0) > i) atomicMin(minrec + r0, i);
        todo &= ~same;
    }
}

// ---- labels -----------------------------------------------------------------------------------------
// A workgroup takes a tile of 2048 records and adds its count once. (A record the index does not hold cannot happen: it would label
// itself with size 0.)
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_labels_kernel(uint32_t n, const uint32_t* __restrict__ minrec, const uint32_t* __restrict__ size,
                               int32_t* __restrict__ labels, int32_t* __restrict__ sizes, int32_t* __restrict__ n_clusters)
{
    __shared__ uint32_t wsum[kBlockThreads / 64];
    uint32_t firsts = 0u;
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t i = (blockIdx.x * kPointsPerLane + c) * kBlockThreads + threadIdx.x;
        if (i >= n) break;
        const uint32_t r = (uint32_t)labels[i];
        const uint32_t label = r < n ? minrec[r] : i;
        labels[i] = (int32_t)label;
        if (sizes) sizes[i] = r < n ? (int32_t)size[r] : 0;
        firsts += (uint32_t)(label == i);
    }
    firsts = wave_sum(firsts);
    if (lane_id() == 0u) wsum[threadIdx.x >> 6] = firsts;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (total) atomicAdd(n_clusters, (int32_t)total);
    }
}

// ==== the object table (pcs_cluster_objects_device) =====================================================================================
// An object's accumulator in the workspace: the box as int32 (integer atomic min / max), the sums as int64, the root for `finish`.
struct ObjAcc {
    int32_t   lo[3], hi[3];
    uint32_t  root, pad;
    long long sum[6];            // x, y, z, R, G, B
};
static_assert(sizeof(ObjAcc) == 80, "80 bytes per object in the workspace");
static_assert(sizeof(pcs_cluster_object) == 80 && alignof(pcs_cluster_object) == 8, "pcs_cluster_object is 80 bytes, 8-byte aligned");

__device__ __forceinline__ bool size_passes(uint32_t s, uint32_t min_size, uint32_t max_size)
{
    return s >= min_size && (max_size == 0u || s <= max_size);
}

// ---- record roots -----------------------------------------------------------------------------------
// `label roots` with the device count: rootof[i] = the root's position (kNoRecord: none, cannot happen), minrec[root] = the smallest i.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_record_roots_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, int tol,
                                     const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ start, uint32_t slots,
                                     const uint2* __restrict__ xyz, const uint32_t* __restrict__ parent, uint32_t* __restrict__ minrec,
                                     uint32_t* __restrict__ rootof)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t n = ctl->tab.n_points;
    uint32_t r = kNoRecord;
    if (i < n) {
        const uint32_t k = position_of(load_xyz(in, i), tol, keys, start, slots, xyz, n);
        if (k != kNoRecord) { r = parent[k]; if (r >= n) r = kNoRecord; }
        rootof[i] = r;
    }
    unsigned long long todo = __ballot(r != kNoRecord);
    while (todo) {                                           // one round per distinct root among the wave's lanes
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);
        const unsigned long long same = __ballot(r == r0);
        if ((int)lane_id() == leader && uf_load(minrec, r0) > i) atomicMin(minrec + r0, i);
        todo &= ~same;
    }
}

// ---- firsts -----------------------------------------------------------------------------------------
// first_bits[w] = the ballot of records 64 w .. 64 w + 63 that are the first record of an OBJECT (keep_bits' layout, a bitmap of its
// own: the filter output reads keep_bits behind this); a word whose first record is at or beyond the count is not written. The first
// record of a cluster that is no object writes slot[root] = -1, so that every root's slot is written once per call. tile_counts[t] =
// the firsts of tile t.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_firsts_kernel(const OutlierCtl* __restrict__ ctl, uint32_t min_size, uint32_t max_size, const uint32_t* __restrict__ rootof,
                               const uint32_t* __restrict__ minrec, const uint32_t* __restrict__ size, int32_t* __restrict__ slot,
                               unsigned long long* __restrict__ first_bits, uint32_t* __restrict__ tile_counts)
{
    __shared__ uint32_t wsum[kBlockThreads / 64];
    const uint32_t n = ctl->tab.n_points;
    uint32_t firsts = 0u;                                    // wave-uniform
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t i = (blockIdx.x * kPointsPerLane + c) * kBlockThreads + threadIdx.x;
        bool first = false;
        if (i < n) {
            const uint32_t r = rootof[i];
            if (r != kNoRecord && minrec[r] == i) {
                first = size_passes(size[r], min_size, max_size);
                if (!first) slot[r] = -1;
            }
        }
        const unsigned long long bits = __ballot(first);
        if (lane_id() == 0u && i < n) first_bits[i >> 6] = bits;
        firsts += (uint32_t)__popcll(bits);
    }
    if (lane_id() == 0u) wsum[threadIdx.x >> 6] = firsts;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---- slots ------------------------------------------------------------------------------------------
// A first record's rank among the firsts, in record order, is its object's k: the tile's prefix, the firsts of the tile's words in
// front of its own, the bits below its own. slot[root] = k; for k < max_objects the accumulator is set up: an empty box, zero sums.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_slots_kernel(const OutlierCtl* __restrict__ ctl, const uint32_t* __restrict__ rootof,
                              const unsigned long long* __restrict__ first_bits, const uint32_t* __restrict__ tile_prefix,
                              int32_t* __restrict__ slot, ObjAcc* __restrict__ acc, uint32_t max_objects)
{
    __shared__ uint32_t pre[kTilePoints / 64];
    const uint32_t n = ctl->tab.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    const uint32_t pts = min(kTilePoints, n - tile0);
    if (threadIdx.x < 64u) {
        const bool has = threadIdx.x < kTilePoints / 64 && threadIdx.x * 64u < pts;
        const uint32_t c = has ? (uint32_t)__popcll(first_bits[(size_t)blockIdx.x * (kTilePoints / 64) + threadIdx.x]) : 0u;
        uint32_t total;
        const uint32_t ex = wave_exclusive_scan(c, total);
        if (threadIdx.x < kTilePoints / 64) pre[threadIdx.x] = ex;
    }
    __syncthreads();
    const uint32_t base = tile_prefix[blockIdx.x];
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t j = c * kBlockThreads + threadIdx.x;
        if (j >= pts) break;
        const uint32_t i = tile0 + j;
        const unsigned long long word = first_bits[i >> 6];
        if (!((word >> (i & 63u)) & 1ull)) continue;
        const uint32_t k = base + pre[j >> 6] + (uint32_t)__popcll(word & ((1ull << (i & 63u)) - 1ull));
        const uint32_t r = rootof[i];                        // (a first has a root below n: firsts saw it)
        slot[r] = (int32_t)k;
        if (k < max_objects) {
            ObjAcc a;
            a.lo[0] = a.lo[1] = a.lo[2] = INT_MAX;
            a.hi[0] = a.hi[1] = a.hi[2] = INT_MIN;
            a.root = r;
            a.pad = 0u;
            for (int q = 0; q < 6; q++) a.sum[q] = 0ll;
            acc[k] = a;
        }
    }
}

// ---- accumulate -------------------------------------------------------------------------------------
// word j of an object's twelve: 0..2 the box's lower corner (minimum), 3..5 its upper (maximum), 6..11 the sums (add). A minimum or
// maximum that the word already meets, and a zero addend, are not sent. Relaxed agent-scope integer atomics: any order, one result.
__device__ __forceinline__ void flush_word(ObjAcc* a, uint32_t j, int v)
{
    if (j < 3u) {
        if (__hip_atomic_load(a->lo + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(a->lo + j, v);
    } else if (j < 6u) {
        if (__hip_atomic_load(a->hi + (j - 3u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(a->hi + (j - 3u), v);
    } else if (v != 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(a->sum + (j - 6u)), (unsigned long long)(long long)v);
    }
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// t[0..11] reduced over the whole wave, word by word (lanes outside a group hand in the identities)
__device__ __forceinline__ void wave_reduce12(int (&t)[12])
{
#pragma unroll
    for (int q = 0; q < 3; q++) t[q] = wave_min(t[q]);
#pragma unroll
    for (int q = 3; q < 6; q++) t[q] = wave_max(t[q]);
#pragma unroll
    for (int q = 6; q < 12; q++) t[q] = (int)wave_sum((uint32_t)t[q]);
}

// lane j's word of twelve wave-uniform ones (a select chain: a register array indexed by the lane would live in scratch)
__device__ __forceinline__ int word_of_lane(const int (&t)[12])
{
    int v = 0;
#pragma unroll
    for (int q = 0; q < 12; q++) v = lane_id() == (uint32_t)q ? t[q] : v;
    return v;
}

// One lane per input record, a tile of 2048 per workgroup, 256 at a time. k = slot[rootof[i]] is the record's object (or -1), written
// to object_of[i] as it is; only k < max_objects has an accumulator. A wave's lanes are grouped by k; a group is reduced across the
// wave and leaves as one atomic per word, lanes 0..11 taking a word each. The first object a wave meets is HELD instead: every lane
// keeps its own twelve partials over the tile (no cross-lane traffic per round), the wave reduces them once, the workgroup's waves
// that hold wave 0's object are combined through LDS and flushed once per tile and word — one cluster that holds most of the cloud
// would otherwise take twelve atomics per wave and round on the same twelve words. 32-bit arithmetic up to the tile
// (2048 * 32768 = 2^26); the global adds are 64-bit.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_accumulate_kernel(const int16_t* __restrict__ in, const OutlierCtl* __restrict__ ctl, const uint32_t* __restrict__ rootof,
                                   const int32_t* __restrict__ slot, uint32_t max_objects, ObjAcc* acc, int32_t* __restrict__ object_of)
{
    __shared__ int part[kBlockThreads / 64][13];
    const uint32_t n = ctl->tab.n_points;
    int held = -1;                                           // wave-uniform
    int h[12] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0, 0, 0, 0, 0};
    for (uint32_t c = 0; c < (uint32_t)kPointsPerLane; c++) {
        const uint32_t i = (blockIdx.x * kPointsPerLane + c) * kBlockThreads + threadIdx.x;
        const bool live = i < n;
        if (!__ballot(live)) break;                          // (records ascend: nothing live behind this either)
        int k = -1;
        int v[6] = {0, 0, 0, 0, 0, 0};
        if (live) {
            const uint32_t r = rootof[i];
            if (r != kNoRecord) k = slot[r];
            if (object_of) object_of[i] = k;
            const int16_t* p = in + (size_t)i * PCS_POINT_SHORTS;
            const uint32_t c3 = (uint16_t)p[3], c4 = (uint16_t)p[4];
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
            v[3] = (int)(c3 & 0xFFu); v[4] = (int)(c3 >> 8); v[5] = (int)(c4 & 0xFFu);      // the high byte of short 4 is not read
        }
        const bool counts = live && k >= 0 && (uint32_t)k < max_objects;
        unsigned long long todo = __ballot(counts);
        if (held < 0 && todo) held = __builtin_amdgcn_readlane(k, __ffsll((long long)todo) - 1);
        const bool mine = counts && k == held;
        if (mine) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                h[q] = min(h[q], v[q]);
                h[3 + q] = max(h[3 + q], v[q]);
            }
#pragma unroll
            for (int q = 0; q < 6; q++) h[6 + q] += v[q];
        }
        todo &= ~__ballot(mine);
        while (todo) {                                       // wave-uniform: one round per other object among the wave's lanes
            const int k0 = __builtin_amdgcn_readlane(k, __ffsll((long long)todo) - 1);
            const bool in_group = counts && k == k0;
            int t[12];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                t[q] = in_group ? v[q] : INT_MAX;
                t[3 + q] = in_group ? v[q] : INT_MIN;
            }
#pragma unroll
            for (int q = 0; q < 6; q++) t[6 + q] = in_group ? v[q] : 0;
            wave_reduce12(t);
            const int w = word_of_lane(t);
            if (lane_id() < 12u) flush_word(acc + k0, lane_id(), w);
            todo &= ~__ballot(in_group);
        }
    }
    wave_reduce12(h);
    const uint32_t wave = threadIdx.x >> 6;
    {
        const int w = word_of_lane(h);
        if (lane_id() < 12u) part[wave][lane_id()] = w;
        if (lane_id() == 12u) part[wave][12] = held;
    }
    __syncthreads();
    const uint32_t j = lane_id();
    if (j >= 12u) return;
    const int h0 = part[0][12];
    if (wave == 0u) {
        if (h0 < 0) return;
        int total = part[0][j];
        for (uint32_t w = 1; w < kBlockThreads / 64; w++) {
            if (part[w][12] != h0) continue;
            const int o = part[w][j];
            total = j < 3u ? min(total, o) : j < 6u ? max(total, o) : total + o;
        }
        flush_word(acc + h0, j, total);
    } else {
        const int hw = part[wave][12];
        if (hw >= 0 && hw != h0) flush_word(acc + hw, j, part[wave][j]);
    }
}

// ---- finish -----------------------------------------------------------------------------------------
// One lane per written entry: all 80 bytes, the reserved words zero. Nothing at or beyond min(n_objects, max_objects) is written.
__global__ __launch_bounds__(kBlockThreads)
void pcs_cluster_finish_kernel(const int32_t* __restrict__ n_objects, uint32_t max_objects, const ObjAcc* __restrict__ acc,
                               const uint32_t* __restrict__ minrec, const uint32_t* __restrict__ size, pcs_cluster_object* __restrict__ objects)
{
    const uint32_t k = blockIdx.x * kBlockThreads + threadIdx.x;
    const int32_t found = *n_objects;
    if (found <= 0 || k >= min((uint32_t)found, max_objects)) return;
    const ObjAcc a = acc[k];
    pcs_cluster_object o;
    o.label = (int32_t)minrec[a.root];
    o.size = (int32_t)size[a.root];
    for (int q = 0; q < 3; q++) {
        o.lo[q] = (int16_t)a.lo[q];
        o.hi[q] = (int16_t)a.hi[q];
        o.sum_xyz[q] = a.sum[q];
        o.sum_rgb[q] = a.sum[3 + q];
    }
    o.reserved0 = 0;
    o.reserved1 = 0;
    objects[k] = o;
}

// Where the object table's words lie behind the cluster workspace.
struct ObjectCarve {
    uint32_t*           rootof;
    int32_t*            slot;
    unsigned long long* first_bits;
    uint32_t*           tile_counts;
    uint32_t*           tile_prefix;
    ObjAcc*             acc;
    int32_t*            scratch;

    ObjectCarve(uint32_t capacity, uint32_t max_objects, void* d_ws)
    {
        const size_t tiles = (capacity + kTilePoints - 1) / kTilePoints;
        uint8_t* w = static_cast<uint8_t*>(d_ws) + cluster_workspace_bytes(capacity);
        auto carve = [&](size_t bytes) { uint8_t* p = w; w += up256(bytes); return p; };
        rootof      = reinterpret_cast<uint32_t*>(carve(4 * (size_t)capacity));
        slot        = reinterpret_cast<int32_t*>(carve(4 * (size_t)capacity));
        first_bits  = reinterpret_cast<unsigned long long*>(carve(tiles * kBlockThreads));
        tile_counts = reinterpret_cast<uint32_t*>(carve(4 * tiles));
        tile_prefix = reinterpret_cast<uint32_t*>(carve(4 * tiles));
        acc         = reinterpret_cast<ObjAcc*>(carve(sizeof(ObjAcc) * (size_t)max_objects));
        scratch     = reinterpret_cast<int32_t*>(carve(256));
    }
};

}  // namespace

size_t cluster_workspace_bytes(uint32_t capacity)
{
    return up256(outlier_workspace_bytes(capacity)) + 3 * up256(4 * (size_t)capacity) + 256;
}

size_t cluster_objects_workspace_bytes(uint32_t capacity, uint32_t max_objects)
{
    const size_t tiles = (capacity + kTilePoints - 1) / kTilePoints;
    return cluster_workspace_bytes(capacity) + 2 * up256(4 * (size_t)capacity) + up256(tiles * kBlockThreads) + 2 * up256(4 * tiles) +
           up256(sizeof(ObjAcc) * (size_t)max_objects) + 256;
}

const char* cluster_stage_name(int stage)
{
    static const char* const names[kClusterAllStages] = {"clear", "insert", "cell sums", "cell scan", "cell starts", "scatter", "init", "union",
                                                         "roots", "flag", "tile count", "tile scan", "emit", "stats", "label roots", "labels",
                                                         "record roots", "firsts", "first scan", "slots", "accumulate", "finish"};
    return stage >= 0 && stage < kClusterAllStages ? names[stage] : "?";
}

hipError_t launch_cluster_stage(int stage, const int16_t* d_in, uint32_t n_points, const int32_t* d_n_points, uint32_t capacity,
                                int tolerance_mm, int min_size, int max_size, void* d_ws, size_t ws_bytes, int16_t* d_out,
                                int32_t* d_out_points, long long* d_stats, int32_t* d_labels, int32_t* d_sizes, int32_t* d_n_clusters,
                                hipStream_t st)
{
    if (!capacity || tolerance_mm < PCS_CLUSTER_TOLERANCE_MIN || tolerance_mm > PCS_CLUSTER_TOLERANCE_MAX || min_size < 1 || max_size < 0 ||
        (max_size && max_size < min_size) || ws_bytes < cluster_workspace_bytes(capacity) || ((uintptr_t)d_ws & 255u) ||
        (!d_n_points && n_points > capacity))
        return hipErrorInvalidValue;
    // over the front of the workspace: the cell index (0 to 5) and the radius filter's compaction (its 7 to 9)
    const size_t index_bytes = up256(outlier_workspace_bytes(capacity));
    if (stage >= 0 && stage < kIndexStages)
        return launch_cell_index_stage(stage, d_in, n_points, d_n_points, capacity, tolerance_mm, d_ws, index_bytes, st);
    if (stage >= 10 && stage <= 12) return launch_outlier_compact_stage(stage - 3, d_in, capacity, d_ws, index_bytes, d_out, d_out_points, st);
    OutlierIndexView view{};
    OutlierKeepView kv{};
    if (hipError_t e = outlier_index_view(capacity, d_ws, index_bytes, &view)) return e;
    if (hipError_t e = outlier_keep_view(capacity, d_ws, index_bytes, &kv)) return e;
    uint8_t* w = static_cast<uint8_t*>(d_ws) + index_bytes;
    uint32_t* const parent = reinterpret_cast<uint32_t*>(w);          w += up256(4 * (size_t)capacity);
    uint32_t* const size = reinterpret_cast<uint32_t*>(w);            w += up256(4 * (size_t)capacity);
    uint32_t* const minrec = reinterpret_cast<uint32_t*>(w);
    const dim3 per_record((capacity + kBlockThreads - 1) / kBlockThreads), per_tile((capacity + kTilePoints - 1) / kTilePoints), threads(kBlockThreads);
    const uint32_t lo = (uint32_t)min_size, hi = (uint32_t)max_size;
    switch (stage) {
    case 6:
        hipLaunchKernelGGL(pcs_cluster_init_kernel, per_record, threads, 0, st, kv.ctl, parent, size, minrec, d_stats);
        break;
    case 7:
        hipLaunchKernelGGL(pcs_cluster_union_kernel, per_record, threads, 0, st, kv.ctl, tolerance_mm, view.keys, view.start, view.slots, view.xyz,
                           parent);
        break;
    case 8:
        hipLaunchKernelGGL(pcs_cluster_roots_kernel, per_tile, threads, 0, st, kv.ctl, parent, size);
        break;
    case 9:
        hipLaunchKernelGGL(pcs_cluster_flag_kernel, per_record, threads, 0, st, d_in, kv.ctl, tolerance_mm, lo, hi, view.keys, view.start,
                           view.slots, view.xyz, parent, size, kv.keep_bits);
        break;
    case 13:
        if (!d_stats || !d_out_points) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pcs_cluster_stats_kernel, per_tile, threads, 0, st, kv.ctl, lo, hi, parent, size, d_out_points,
                           reinterpret_cast<unsigned long long*>(d_stats));
        break;
    case 14:                     // the labels form has no counted variant: the count is n_points
        if (d_n_points || !d_labels || !d_n_clusters) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pcs_cluster_label_roots_kernel, per_record, threads, 0, st, d_in, n_points, tolerance_mm, view.keys, view.start,
                           view.slots, view.xyz, parent, minrec, d_labels, d_n_clusters);
        break;
    case 15:
        if (d_n_points || !d_labels || !d_n_clusters) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pcs_cluster_labels_kernel, per_tile, threads, 0, st, n_points, minrec, size, d_labels, d_sizes, d_n_clusters);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

int32_t* cluster_objects_scratch_word(uint32_t capacity, uint32_t max_objects, void* d_ws)
{
    return ObjectCarve(capacity, max_objects, d_ws).scratch;
}

hipError_t launch_cluster_object_stage(int stage, const int16_t* d_in, uint32_t capacity, int tolerance_mm, int min_size, int max_size,
                                       uint32_t max_objects, void* d_ws, size_t ws_bytes, pcs_cluster_object* d_objects,
                                       int32_t* d_n_objects, int32_t* d_object_of, hipStream_t st)
{
    if (!capacity || tolerance_mm < PCS_CLUSTER_TOLERANCE_MIN || tolerance_mm > PCS_CLUSTER_TOLERANCE_MAX || min_size < 1 || max_size < 0 ||
        (max_size && max_size < min_size) || max_objects > (uint32_t)PCS_CLUSTER_OBJECTS_MAX || (max_objects && !d_objects) || !d_n_objects ||
        ws_bytes < cluster_objects_workspace_bytes(capacity, max_objects) || ((uintptr_t)d_ws & 255u))
        return hipErrorInvalidValue;
    const size_t index_bytes = up256(outlier_workspace_bytes(capacity));
    OutlierIndexView view{};
    OutlierKeepView kv{};
    if (hipError_t e = outlier_index_view(capacity, d_ws, index_bytes, &view)) return e;
    if (hipError_t e = outlier_keep_view(capacity, d_ws, index_bytes, &kv)) return e;
    uint8_t* w = static_cast<uint8_t*>(d_ws) + index_bytes;
    uint32_t* const parent = reinterpret_cast<uint32_t*>(w);          w += up256(4 * (size_t)capacity);
    uint32_t* const size = reinterpret_cast<uint32_t*>(w);            w += up256(4 * (size_t)capacity);
    uint32_t* const minrec = reinterpret_cast<uint32_t*>(w);
    const ObjectCarve oc(capacity, max_objects, d_ws);
    const dim3 per_record((capacity + kBlockThreads - 1) / kBlockThreads), per_tile((capacity + kTilePoints - 1) / kTilePoints), threads(kBlockThreads);
    switch (stage) {
    case 16:
        hipLaunchKernelGGL(pcs_cluster_record_roots_kernel, per_record, threads, 0, st, d_in, kv.ctl, tolerance_mm, view.keys, view.start,
                           view.slots, view.xyz, parent, minrec, oc.rootof);
        break;
    case 17:
        hipLaunchKernelGGL(pcs_cluster_firsts_kernel, per_tile, threads, 0, st, kv.ctl, (uint32_t)min_size, (uint32_t)max_size, oc.rootof, minrec,
                           size, oc.slot, oc.first_bits, oc.tile_counts);
        break;
    case 18:     // the firsts' count is the scan's per-stream count: d_n_objects[0], nothing behind it
        return launch_scan(&kv.ctl->tab, 1, 1, oc.tile_counts, oc.tile_prefix, nullptr, d_n_objects, nullptr, st);
    case 19:
        hipLaunchKernelGGL(pcs_cluster_slots_kernel, per_tile, threads, 0, st, kv.ctl, oc.rootof, oc.first_bits, oc.tile_prefix, oc.slot, oc.acc,
                           max_objects);
        break;
    case 20:
        hipLaunchKernelGGL(pcs_cluster_accumulate_kernel, per_tile, threads, 0, st, d_in, kv.ctl, oc.rootof, oc.slot, max_objects, oc.acc,
                           d_object_of);
        break;
    case 21:
        // (max_objects 0: one workgroup that writes nothing, so that a call's launch count does not depend on it)
        hipLaunchKernelGGL(pcs_cluster_finish_kernel, dim3(max_objects ? (max_objects + kBlockThreads - 1) / kBlockThreads : 1u), threads, 0, st, d_n_objects,
                           max_objects, oc.acc, minrec, size, d_objects);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pcs
