// pcs_kernels_voxel.hip — the voxel pipeline's readers for gfx950 (CDNA4): rasters or a packed payload -> voxel partials, their LDS
// table and their launchers. A point is made exactly as in the stitch kernels of pcs_kernels.hip: that code is pcs_kernels_common.h.
// A translation unit of its own (pcs_kernels_voxel.o) for its flags (Makefile): SLP vectorisation stays ON — these kernels are VALU-bound
// and v_pk_fma_f32 / v_pk_mul_f32 take 15 % of their vector instructions away: 146 -> 140 us per 16 x 1080p frame-set. A packed op is two
// independent, individually rounded IEEE operations: the bits do not change.

#include "pcs_kernels_common.h"

namespace pcs {

namespace {

// ---- rasters -> voxel partials (config 5 without the stitched payload) ---------------------------------------------
// pcs_process_frames_voxel_device: the voxel grid of the cloud pcs_process_frames_device would stitch, without writing
// that cloud (10 B per kept point out, 10 B back in for the pre-aggregation) and without its ordered placement (count
// and scan passes): the voxel sums are integers, so the order of the points is irrelevant. A workgroup of 1024 lanes
// takes 8192 consecutive pixels of one camera; a lane deprojects, transforms and packs its 8 consecutive pixels exactly
// as the stitch kernels do (same records, bit for bit), sums runs of equal voxel keys among them in registers (8
// neighbouring pixels mostly share a voxel) and adds each run to the workgroup's LDS hash table (pcs_voxel.hip, step 1);
// one partial per occupied slot is appended to the same arrays the payload reader fills, and pcs_voxel.hip's sort and
// segmented mean run unchanged.
#include "pcs_voxel_agg.h"
#include "pcs_vox_tiling.h"

#ifndef PCS_VOX_THREADS
#define PCS_VOX_THREADS 512
#endif
#ifndef PCS_VOX_SLOTS
#define PCS_VOX_SLOTS 2048
#endif
#ifndef PCS_VOX_PREFETCH
#define PCS_VOX_PREFETCH 1
#endif
// Workgroup shape of the raster / payload readers: 512 lanes (8 wavefronts) and a 2048-slot table (72 KiB): two workgroups per
// CU, 4 wavefronts per SIMD at 120 - 126 VGPRs (~105 when these measurements were taken, with packed records). Round 5 measured the two ways to a FIFTH wavefront per SIMD (<= 96 VGPRs), 16 x 1080p
// at 50 mm, one call, A/B on one box:
//   640 lanes x 2 workgroups           0.266 vs 0.197 ms — a workgroup's 10 wavefronts are dealt to the SIMDs 3-3-2-2 and two such
//                                      workgroups need six slots on two SIMDs: only ONE fits a CU (a workgroup must be a multiple of
//                                      four wavefronts);
//   256 lanes x 5 workgroups, 896-slot 0.213 vs 0.205 ms — five wavefronts per SIMD are reached (96 VGPRs, no spill, 31.5 KiB per
//   tables (-DPCS_VOX_THREADS=256      table, same 128 x 64 patch per table in four rounds), and the launch is slower: the kernel is
//   -DPCS_VOX_SLOTS=896)               not short of wavefronts to issue from.
// Both shapes still build (the code below is generic in the two constants); neither is used.
// The same point for the voxel readers: coordinates as sign-correct integers (the record's int16 fields, widened), the colour
// dword as fetched (R | G<<8 | B<<16 | don't care). Cvt::kCoordsInShort: the policy vouches that the converted values lie in
// int16 (VoxCvt); otherwise the low 16 bits are sign-extended here, as the record would hold them.
struct VoxPoint {
    int32_t x, y, z;
    uint32_t w;
};
template <bool ROWC = false, class Cvt>
__device__ __forceinline__ VoxPoint make_vox_point(const StreamParams& P, const uint8_t* __restrict__ color,
                                                   const PointIn& p, Cvt& cv)
{
    const float ax = world_mm(P.M + 0, p.X, p.Y, p.Z);
    const float ay = world_mm(P.M + 4, p.X, p.Y, p.Z);
    const float az = world_mm(P.M + 8, p.X, p.Y, p.Z);
    float xf, yf;
    color_coords(P, p.u, p.v, xf, yf);
    cv.note(ax, ay, az, xf, ROWC ? xf : yf);
    const int32_t x = cv.cvt(ax), y = cv.cvt(ay), z = cv.cvt(az);
    // (ROWC: p.v IS the row, certified at pcs_create for every depth value — whatever conversion policy the lane runs under)
    const int32_t yi = ROWC ? __float_as_int(p.v) : cv.pixel(yf, P.cH - 1, P.c_hm1_f);
    const uint32_t w = color_fetch(P, color, cv.pixel(xf, P.cW - 1, P.c_wm1_f), yi, cv);
    if (Cvt::kCoordsInShort) return VoxPoint{x, y, z, w};
    return VoxPoint{(int32_t)(int16_t)x, (int32_t)(int16_t)y, (int32_t)(int16_t)z, w};
}
// what vox_table_round reads of a point, for both forms
__device__ __forceinline__ int pt_x(const Record& r) { return (int)(short)(r.xy & 0xFFFFu); }
__device__ __forceinline__ int pt_y(const Record& r) { return (int)(short)(r.xy >> 16); }
__device__ __forceinline__ int pt_z(const Record& r) { return (int)(short)(r.zc & 0xFFFFu); }
__device__ __forceinline__ unsigned int pt_red(const Record& r) { return (r.zc >> 16) & 0xFFu; }
__device__ __forceinline__ unsigned int pt_green(const Record& r) { return r.zc >> 24; }
__device__ __forceinline__ unsigned int pt_blue(const Record& r) { return r.b & 0xFFu; }
__device__ __forceinline__ int pt_x(const VoxPoint& r) { return r.x; }
__device__ __forceinline__ int pt_y(const VoxPoint& r) { return r.y; }
__device__ __forceinline__ int pt_z(const VoxPoint& r) { return r.z; }
__device__ __forceinline__ unsigned int pt_red(const VoxPoint& r) { return r.w & 0xFFu; }
__device__ __forceinline__ unsigned int pt_green(const VoxPoint& r) { return (r.w >> 8) & 0xFFu; }
__device__ __forceinline__ unsigned int pt_blue(const VoxPoint& r) { return (r.w >> 16) & 0xFFu; }

// Which of a lane's 8 points take part. (Eight predicates held in the condition registers instead of the mask's bits, for the
// reader without the -c test, measured: 4 % fewer VALU instructions with the wide points below, no faster — and the round's code twice.)
struct KeepBits {
    uint32_t m;
    __device__ __forceinline__ bool operator()(int k) const { return (m >> k) & 1u; }
};

constexpr int kVoxThreads = PCS_VOX_THREADS;
constexpr int kVoxSlots = PCS_VOX_SLOTS;
constexpr uint32_t kVoxRows = kVoxThreads / 8;    // a round = kVoxRows rows of 64 pixels (8 lanes x 8 pixels)
constexpr int kVoxOwn = (kVoxSlots + kVoxThreads - 1) / kVoxThreads;      // table slots a lane flushes
constexpr uint32_t kVoxRoundPoints = kVoxThreads * kPointsPerLane;      // 4096 points per round; `rounds` of them share one table

// The workgroup's LDS table: slot = key + the seven sums in three 64-bit words and one 32-bit word: (x, y), (z, count),
// (R, G), B — four LDS adds per run instead of seven. Coordinates are summed BIASED (+32768, so every term is
// non-negative and a 64-bit add never carries between its halves: <= 32 768 points x 65 535 < 2^31); the bias leaves at
// the output.
// Probe sequence in a table of kVoxSlots slots (not a power of two): start = the hash's top 16 bits scaled into the table
// with one 24-bit multiply, odd stride, wrap by a conditional subtract. A run that finds no slot within kProbe probes goes out
// as a partial of its own, so the sequence need not visit every slot.
struct VoxProbe {
    unsigned int first, step;
    __device__ __forceinline__ explicit VoxProbe(unsigned long long key)
    {
        const unsigned int lo = (unsigned int)key, hi = (unsigned int)(key >> 32);
        const unsigned int m = __umul24(lo, 0x9E3779u) + __umul24(__builtin_amdgcn_alignbit(hi, lo, 24), 0x85EBCBu);
        if (kVoxSlots == kSlots) {                                         // the 2^11 table: VoxelProbe's sequence (pcs_voxel_agg.h)
            first = m >> 21;
            step = ((m >> 10) & (unsigned)(kSlots - 1)) | 1u;
        } else {
            first = __umul24(m >> 16, (unsigned int)kVoxSlots) >> 16;      // top 16 bits scaled into the table (the product stays below 2^32)
            step = ((m >> 3) & 0x7Fu) | 1u;                                // odd, < 128
        }
    }
    __device__ __forceinline__ unsigned int next(unsigned int h) const
    {
        if (kVoxSlots == kSlots) return (h + step) & (unsigned)(kSlots - 1);
        h += step;
        return h >= (unsigned int)kVoxSlots ? h - (unsigned int)kVoxSlots : h;
    }
};

struct VoxTable {
    unsigned long long *skey, *sxy, *szn, *srg;
    unsigned int *sbl, *wtot, *base_s, *flag, *kor;       // kor[4]: OR of the keys written (lo, hi), OR of their complements
};
#define PCS_VOX_TABLE_DECL                                                                             \
    __shared__ unsigned long long skey_[kVoxSlots];                                                       \
    __shared__ unsigned long long sxy_[kVoxSlots], szn_[kVoxSlots], srg_[kVoxSlots];                            \
    __shared__ unsigned int sbl_[kVoxSlots];                                                              \
    __shared__ unsigned int wtot_[kVoxThreads / 64];                                                   \
    __shared__ unsigned int base_s_, flag_, kor_[4];                                                   \
    const VoxTable T{skey_, sxy_, szn_, srg_, sbl_, wtot_, &base_s_, &flag_, kor_};                    \
    unsigned long long key_or = 0ull, key_orn = 0ull

// Warm bucket tail (vs.regions): the geometry of this call's regions, and one partial put into its bucket's region by a lane on
// its own (a run that found no slot in the workgroup's table: a few dozen per frame-set) — the bucket by binary search in
// the global splitters (ten dependent trips to L2: a few dozen lanes per frame-set take them), the slot by a returning add on
// the bucket's cursor. The workgroup's flush does the same for all the table's partials at once (vox_table_flush_regions).
struct VoxRegions {
    unsigned int B, cap, stride;
    __device__ __forceinline__ explicit VoxRegions(const VoxelStage& vs)
    {
        B = vs.reg[0]; cap = vs.reg[1];
        if (B == 0u || B > kVoxBuckets) B = kVoxBuckets;
        // (the tail applies the same rule. The regions hold any cloud of THIS call's capacity; the sizes come from the previous
        // call, which may have had a larger one: then nothing fits and everything goes to the general list)
        if ((unsigned long long)B * cap > vs.region_slots) cap = 0u;
        stride = kVoxBuckets / B;
    }
    // bucket j ends below splitter j (the last one is open)
    __device__ __forceinline__ unsigned long long splitter(const VoxelStage& vs, unsigned int j) const
    {
        return (j + 1u < B) ? vs.spl[(j + 1u) * stride - 1u] : kEmptyKey;
    }
};
__device__ __forceinline__ void vox_region_put(const VoxelStage& vs, unsigned long long key, const VoxelPartial& v)
{
    // (Measured and not kept: half of the splitters in LDS for this search — 4 KiB per workgroup, stored behind a barrier before the
    // first round — and one returning add per wavefront and bucket instead of one per run: +4 .. 7 us on every 16 x 1080p
    // frame-set for 0.3 ms off a call on a cloud of scattered points, whose runs mostly fail.)
    const VoxRegions R(vs);
    unsigned int b = 0;
#pragma unroll 1
    for (unsigned int step = kVoxBuckets / 2; step; step >>= 1)
        if (R.splitter(vs, b + step - 1u) <= key) b += step;
    const unsigned int at = atomicAdd(&vs.cursor[b], 1u);
    if (at < R.cap) {
        const size_t dst = (size_t)b * R.cap + at;
        vs.keys_r[dst] = key;
        static_cast<VoxelPartial*>(vs.part_r)[dst] = v;
    } else {
        const unsigned int e = atomicAdd(vs.n_runs, 1u);
        vs.keys[e] = key;
        static_cast<VoxelPartial*>(vs.part)[e] = v;
        vs.bucket_of[e] = (unsigned short)b;
    }
}

__device__ __forceinline__ void vox_table_init(const VoxTable& T)
{
    for (int j = threadIdx.x; j < kVoxSlots; j += kVoxThreads) {
        T.skey[j] = kEmptyKey;
        T.sxy[j] = T.szn[j] = T.srg[j] = 0ull;
        T.sbl[j] = 0u;
    }
    if (threadIdx.x == 0) *T.flag = 0u;
    if (threadIdx.x < 4) T.kor[threadIdx.x] = 0u;
    __syncthreads();
}

// One round: a lane's 8 consecutive records (bit k of `keep`: record k takes part) -> the table.
template <class Pt, class Keep>
__device__ __forceinline__ void vox_table_round(const VoxTable& T, const VoxelStage& vs, const Pt (&rec)[8], const Keep& keep,
                                                bool crowded, unsigned long long& key_or, unsigned long long& key_orn)
{
    unsigned long long* const skey = T.skey; unsigned long long* const sxy = T.sxy; unsigned long long* const szn = T.szn;
    unsigned long long* const srg = T.srg; unsigned int* const sbl = T.sbl;
    const VoxelDiv dv{vs.div_inv, vs.div_c};
    const unsigned int bits = vs.bits, idx_bits = vs.idx_bits;
    VoxelPartial* __restrict__ part = static_cast<VoxelPartial*>(vs.part);
    const int lane = threadIdx.x & 63;
    auto key_of = [&](const Pt& r) { return voxel_key(dv, pt_x(r), pt_y(r), pt_z(r), bits); };
    // runs of equal keys among the lane's 8 pixels: summed in registers, the run's LAST point adds them to the table
    unsigned int ax = 0, ay = 0, az = 0;                     // biased: sums of (coordinate + 32768)
    unsigned int ar = 0, ag = 0, ab = 0, an = 0, failed = 0;
    bool cont = false;                                       // point k continues the run of point k-1
    unsigned long long kcur = key_of(rec[0]);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const bool live = keep(k);
        const bool live_next = k < 7 && keep(k < 7 ? k + 1 : 7);
        const unsigned long long knext = k < 7 ? key_of(rec[k + 1]) : 0ull;
        const int x = pt_x(rec[k]), y = pt_y(rec[k]), z = pt_z(rec[k]);
        if (!cont) { ax = ay = az = 0u; ar = ag = ab = an = 0u; }
        ax += (unsigned int)(x + 32768); ay += (unsigned int)(y + 32768); az += (unsigned int)(z + 32768);
        ar += pt_red(rec[k]); ag += pt_green(rec[k]); ab += pt_blue(rec[k]); an += 1u;
        const bool same_next = live_next && knext == kcur;
        const bool actor = live && !same_next;
        if (actor) {
            const VoxProbe pr(kcur);
            unsigned int h = pr.first;
            // first probe straight-line (it succeeds for all but a few per cent of the runs), the rest in a loop
            unsigned long long old = atomicCAS(&skey[h], kEmptyKey, kcur);
            bool placed = old == kEmptyKey || old == kcur;
            if (__builtin_expect(!placed, 0)) {
                for (int t = 1; t < kProbe; t++) {
                    h = pr.next(h);
                    old = atomicCAS(&skey[h], kEmptyKey, kcur);
                    if (old == kEmptyKey || old == kcur) { placed = true; break; }
                }
            }
            if (placed) {
                atomicAdd(&sxy[h], (unsigned long long)ax | ((unsigned long long)ay << 32));
                atomicAdd(&szn[h], (unsigned long long)az | ((unsigned long long)an << 32));
                atomicAdd(&srg[h], (unsigned long long)ar | ((unsigned long long)ag << 32));
                atomicAdd(&sbl[h], ab);
            } else {
                failed |= 1u << k;                           // the run ending at k goes out as a partial of its own
            }
        }
        cont = live && same_next;
        kcur = knext;
    }
    // Runs that found no slot (more voxels under this table than it can take: leaves of a few pixels) are appended as
    // partials of their own. The sums are rebuilt from the records: a failed run is the maximal stretch of kept points with
    // the same key that ends at its bit. Where they go is reserved
    //  * crowded (the launcher expects full tables: leaves below 30 mm): with ONE returning global atomic per workgroup and
    //    round, and only when it happens — the workgroup learns that with one barrier per round (3 - 8 % of the kernel
    //    when nothing ever fails, hence the switch);
    //  * otherwise: with one atomic per wavefront that has a failed run — free when there is none, but serialised on the
    //    counter's line when most wavefronts have one (65 k per 16 x 1080p frame-set at 10 mm: 490 us of the kernel's 627).
    const unsigned long long any_failed = __ballot(failed != 0u);    // (all lanes: not inside a short-circuit)
    unsigned int pos = 0;
    bool emit = false;
    const bool to_regions = vs.regions != 0u;                         // uniform over the launch: every failed run finds its own place
    if (to_regions) {
        emit = any_failed != 0ull;
    } else if (crowded) {                                             // uniform over the launch
        if (lane == 0 && any_failed) *T.flag = 1u;
        __syncthreads();
        if (*T.flag) {                                                // workgroup-uniform
            const int wave = threadIdx.x >> 6;
            const unsigned int c = __popc(failed);
            const unsigned int inc = wave_inclusive_scan(c);
            if (lane == 63) T.wtot[wave] = inc;
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned int tot = 0;
                for (int w = 0; w < kVoxThreads / 64; w++) { const unsigned int t = T.wtot[w]; T.wtot[w] = tot; tot += t; }
                *T.base_s = atomicAdd(vs.n_runs, tot);
                *T.flag = 0u;
            }
            __syncthreads();
            pos = *T.base_s + T.wtot[wave] + inc - c;
            emit = true;
        }
    } else if (any_failed) {
        const unsigned int c = __popc(failed);
        const unsigned int inc = wave_inclusive_scan(c);
        unsigned int base = 0;
        if (lane == 63) base = atomicAdd(vs.n_runs, inc);
        pos = (unsigned int)__builtin_amdgcn_readlane((int)base, 63) + inc - c;
        emit = true;
    }
    if (emit) {
        int sx = 0, sy = 0, sz = 0;
        unsigned int r = 0, g = 0, b = 0, cnt = 0;
        unsigned long long kprev = 0ull;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool live = keep(k);
            const int x = pt_x(rec[k]), y = pt_y(rec[k]), z = pt_z(rec[k]);
            const unsigned long long key = voxel_key(dv, x, y, z, bits);
            const bool joins = k > 0 && live && keep(k > 0 ? k - 1 : 0) && key == kprev;
            if (!joins) { sx = sy = sz = 0; r = g = b = cnt = 0u; }
            sx += x; sy += y; sz += z; r += pt_red(rec[k]); g += pt_green(rec[k]); b += pt_blue(rec[k]); cnt += 1u;
            kprev = key;
            if ((failed >> k) & 1u) {
                const VoxelPartial v{sx, sy, sz, r, g, b, cnt, 0u};
                if (to_regions) {
                    vox_region_put(vs, key, v);
                } else {
                    if (idx_bits) vs.keys[pos] = (key << idx_bits) | pos;
                    else { vs.keys[pos] = key; if (vs.idx) vs.idx[pos] = pos; }
                    part[pos] = v;
                    key_or |= key; key_orn |= ~key;
                    pos++;
                }
            }
        }
    }
    if (crowded) __syncthreads();         // wtot / base_s are free again before the next round (or the flush) uses them
}

// End of the workgroup on a WARM bucket tail (vs.regions): every partial straight into its bucket's region. The key array of the
// table is dead once each lane holds its slots' keys, and becomes: this call's splitters (8 KiB) | the workgroup's count per
// bucket (4 KiB) | where its partials start in each region (4 KiB). Ten dependent LDS reads per key find the bucket (the lane's
// keys side by side), a returning LDS add ranks the partial among the workgroup's for that bucket, ONE returning global add per
// bucket the workgroup touches (a 128 x 64-pixel patch touches a few dozen) reserves the slots. A partial that finds its region
// full goes to the general list (keys / part / bucket_of) with a returning add of its own.
__device__ __forceinline__ void vox_table_flush_regions(const VoxTable& T, const VoxelStage& vs)
{
    if (kVoxSlots < 2 * (int)kVoxBuckets) __builtin_trap();                 // (the lab shapes with small tables: no room for the arrays below)
    unsigned long long* const spl = T.skey;
    unsigned int* const hist = reinterpret_cast<unsigned int*>(T.skey + kVoxBuckets);
    unsigned int* const rbase = hist + kVoxBuckets;
    VoxelPartial* __restrict__ part = static_cast<VoxelPartial*>(vs.part);
    VoxelPartial* __restrict__ part_r = static_cast<VoxelPartial*>(vs.part_r);
    const VoxRegions R(vs);
    const unsigned int cap = R.cap;
    // (requesting the splitters when the workgroup starts — two dependent trips to L2 that the rounds would hide — costs four
    // registers through the rounds and measured no gain at 40 / 50 mm, 2 us more at 100 / 200 mm)
    constexpr int kSplPer = ((int)kVoxBuckets + kVoxThreads - 1) / kVoxThreads;
    unsigned long long sp[kSplPer];
#pragma unroll
    for (int i = 0; i < kSplPer; i++) sp[i] = R.splitter(vs, threadIdx.x + (unsigned int)(i * kVoxThreads));
    __syncthreads();                                                        // the last round's adds are in
    unsigned long long key[kVoxOwn];
#pragma unroll
    for (int q = 0; q < kVoxOwn; q++) { const int j = threadIdx.x * kVoxOwn + q; key[q] = j < kVoxSlots ? T.skey[j] : kEmptyKey; }
    __syncthreads();                                                        // every key is in a register: the array is free
#pragma unroll
    for (int i = 0; i < kSplPer; i++) {
        const unsigned int j = threadIdx.x + (unsigned int)(i * kVoxThreads);
        if (j < kVoxBuckets) { spl[j] = sp[i]; hist[j] = 0u; }
    }
    __syncthreads();
    unsigned int bk[kVoxOwn], rk[kVoxOwn];
#pragma unroll
    for (int q = 0; q < kVoxOwn; q++) bk[q] = 0u;
#pragma unroll
    for (unsigned int step = kVoxBuckets / 2; step; step >>= 1) {
#pragma unroll
        for (int q = 0; q < kVoxOwn; q++)
            if (spl[bk[q] + step - 1u] <= key[q]) bk[q] += step;
    }
#pragma unroll
    for (int q = 0; q < kVoxOwn; q++) {
        rk[q] = 0u;
        if (key[q] != kEmptyKey) rk[q] = atomicAdd(&hist[bk[q]], 1u);
    }
    __syncthreads();
    for (unsigned int j = threadIdx.x; j < kVoxBuckets; j += kVoxThreads) {
        const unsigned int c = hist[j];
        rbase[j] = c ? atomicAdd(&vs.cursor[j], c) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kVoxOwn; q++) {
        const int j = threadIdx.x * kVoxOwn + q;
        if (key[q] == kEmptyKey) continue;
        const unsigned long long xy = T.sxy[j], zn = T.szn[j], rg = T.srg[j];
        const unsigned int cnt = (unsigned int)(zn >> 32);
        const int bias = (int)(cnt << 15);
        const VoxelPartial v{(int)(unsigned int)xy - bias, (int)(unsigned int)(xy >> 32) - bias, (int)(unsigned int)zn - bias,
                             (unsigned int)rg, (unsigned int)(rg >> 32), T.sbl[j], cnt, 0u};
        const unsigned int at = rbase[bk[q]] + rk[q];
        if (at < cap) {
            const size_t dst = (size_t)bk[q] * cap + at;
            vs.keys_r[dst] = key[q];
            part_r[dst] = v;
        } else {
            // (the region is full: one returning add for all the lanes of the wavefront that are here)
            const unsigned long long peers = __ballot(1);
            const unsigned int rank = (unsigned int)__popcll(peers & ((1ull << (threadIdx.x & 63u)) - 1ull));
            unsigned int e = 0;
            if (rank == 0u) e = atomicAdd(vs.n_runs, (unsigned int)__popcll(peers));
            e = (unsigned int)__shfl((int)e, __ffsll((long long)peers) - 1) + rank;
            vs.keys[e] = key[q];
            part[e] = v;
            vs.bucket_of[e] = (unsigned short)bk[q];
        }
    }
}

// End of the workgroup: one partial per occupied slot, one returning global atomic for all of them.
__device__ __forceinline__ void vox_table_flush(const VoxTable& T, const VoxelStage& vs, unsigned long long key_or,
                                                unsigned long long key_orn)
{
    if (vs.regions) { vox_table_flush_regions(T, vs); return; }            // (uniform over the launch)
    unsigned long long* const skey = T.skey; unsigned long long* const sxy = T.sxy; unsigned long long* const szn = T.szn;
    unsigned long long* const srg = T.srg; unsigned int* const sbl = T.sbl; unsigned int* const wtot = T.wtot;
    unsigned int& base_s = *T.base_s;
    const unsigned int idx_bits = vs.idx_bits;
    VoxelPartial* __restrict__ part = static_cast<VoxelPartial*>(vs.part);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    // every lane owns four slots; one partial per occupied slot
    unsigned int c = 0;
#pragma unroll
    for (int q = 0; q < kVoxOwn; q++) { const int j = threadIdx.x * kVoxOwn + q; c += j < kVoxSlots && skey[j] != kEmptyKey; }
    const unsigned int inc = wave_inclusive_scan(c);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int tot = 0;
        for (int w = 0; w < kVoxThreads / 64; w++) { const unsigned int t = wtot[w]; wtot[w] = tot; tot += t; }
        base_s = tot ? atomicAdd(vs.n_runs, tot) : 0u;
    }
    __syncthreads();
    unsigned int pos = base_s + wtot[wave] + inc - c;
#pragma unroll
    for (int q = 0; q < kVoxOwn; q++) {
        const int j = threadIdx.x * kVoxOwn + q;
        if (j < kVoxSlots && skey[j] != kEmptyKey) {
            if (idx_bits) vs.keys[pos] = (skey[j] << idx_bits) | pos;
            else { vs.keys[pos] = skey[j]; if (vs.idx) vs.idx[pos] = pos; }
            const unsigned long long xy = sxy[j], zn = szn[j], rg = srg[j];
            const unsigned int cnt = (unsigned int)(zn >> 32);
            const int bias = (int)(cnt << 15);                   // count x 32768 (count <= 32 768)
            part[pos] = VoxelPartial{(int)(unsigned int)xy - bias, (int)(unsigned int)(xy >> 32) - bias, (int)(unsigned int)zn - bias,
                                     (unsigned int)rg, (unsigned int)(rg >> 32), sbl[j], cnt, 0u};
            key_or |= skey[j]; key_orn |= ~skey[j];
            pos++;
        }
    }
    // which key bits vary at all (pcs_voxel.hip's sort drops the others): OR of every key this workgroup wrote and of
    // every complement -> wavefront (DPP) -> LDS -> global ORs. Only when the launcher asked for it: the extra barrier and
    // the read of the global words at the very end of every workgroup cost the 16 x 1080p launch 9 us (6 %), which a
    // skipped pass repays three times over — where one can be skipped (pcs_voxel.hip: plan_for).
    if (!vs.track_bits) return;
    unsigned int v[4] = {(unsigned int)key_or, (unsigned int)(key_or >> 32), (unsigned int)key_orn, (unsigned int)(key_orn >> 32)};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        unsigned int x = v[q];
        x |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
        x |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);   // row_shr:2
        x |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);   // row_shr:4
        x |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);   // row_shr:8
        x |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);   // row_bcast:15
        x |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);   // row_bcast:31
        if (lane == 63 && x) atomicOr(&T.kor[q], x);
    }
    __syncthreads();
    // The words live on their own 128-byte line (kVoxCtlOr), away from the partial counter every workgroup adds to, and a
    // workgroup only issues an atomic if it has a bit the word does not show yet (a stale read costs a redundant OR,
    // nothing else): after the first few workgroups almost none do. (Four unconditional ORs per workgroup on the
    // counter's own line cost the 16 x 1080p launch 10 us.)
    if (threadIdx.x < 4) {
        unsigned int* g = vs.n_runs + kVoxCtlOr + threadIdx.x;
        const unsigned int mine = T.kor[threadIdx.x];
        if (mine & ~__builtin_nontemporal_load(g)) atomicOr(g, mine);
    }
}

// 512 lanes x several rounds rather than 1024 x 1: the raster reader needs > 100 VGPRs (the stitch kernels' 8 points in
// flight plus the table phase), which leaves room for one 1024-lane workgroup per CU — its load phase and its LDS phase
// then have nothing to overlap with. Two 512-lane workgroups fit, and there is no barrier between the rounds.
template <bool DD, bool CD, class Mth>
__global__ __launch_bounds__(kVoxThreads) __attribute__((amdgpu_waves_per_eu(4)))     // two workgroups per CU: <= 128 VGPRs
void pcs_fused_voxel_partials_kernel(const StreamParams* __restrict__ params, int stream0, FramePtrs fp, uint32_t flags,
                                     VoxelStage vs, int rounds, VoxTiling tl, int crowded)
{
    PCS_VOX_TABLE_DECL;
    int s = blockIdx.y;
    uint32_t sq_x0 = 0, sq_y0 = 0, nrx = 1, nry = (uint32_t)rounds;          // rx == 0: `rounds` runs of 4096 consecutive pixels
    if (tl.rx) {
        const uint32_t lin = blockIdx.y * gridDim.x + blockIdx.x;
        PCS_VOX_TILING_DECODE(tl, lin, gridDim.y, s, sq_x0, sq_y0, nrx, nry);
    }
    const StreamParams& P = params[stream0 + s];
    request_constants(P, fp.depth[s], fp.color[s]);
    const uint32_t n = P.n_points;
    const uint32_t W = (uint32_t)P.W, Hh = n / W;
    const uint32_t tile0 = blockIdx.x * (kVoxRoundPoints * (uint32_t)rounds);
    if (tl.rx ? (sq_y0 * kVoxRows >= Hh || sq_x0 * 64u >= W) : (tile0 >= n)) return;      // (a smaller raster than the launch's largest)
    const uint8_t* __restrict__ color = fp.color[s];
    DepthSource<DD, CD, Mth> src{fp.depth[s]};

    // The rounds of this workgroup, in the order (yy, xx) of its patch. A square-row below the raster ends the workgroup, a square
    // beside the raster ends its square-row — uniform over the workgroup, so the barriers of a crowded round stay matched. Where a
    // round has no barrier, a WAVEFRONT whose 8 rows lie below the raster (the last 8 of 1080 = 16 x 64 + 56) passes too.
    // PCS_VOX_PREFETCH: the lane's Z16 quad of the NEXT round is requested before this round's deprojection and table phase (rasters
    // read in 16-byte quads only): the one load of a round that comes from HBM then has a whole round to arrive in.
    auto lane_index = [&](uint32_t yy, uint32_t xx) -> uint32_t {         // this lane's first pixel of round (yy, xx); n: nothing to read
        if (!tl.rx) return tile0 + yy * kVoxRoundPoints + threadIdx.x * kPointsPerLane;
        const uint32_t row = (sq_y0 + yy) * kVoxRows + (threadIdx.x >> 3);
        const uint32_t col = (sq_x0 + xx) * 64u + (threadIdx.x & 7u) * 8u;
        return (row < Hh && col < W) ? row * W + col : n;                // W % 8 == 0: a lane is inside the row or outside it
    };
    const bool prefetch = PCS_VOX_PREFETCH != 0 && src.fast(P);          // uniform over the launch's stream
    uint32_t yy = 0, xx = 0;
    bool have = nry > 0u && nrx > 0u && !(tl.rx && (sq_y0 * kVoxRows >= Hh || sq_x0 * 64u >= W));
    uint32_t i0 = have ? lane_index(0u, 0u) : n;
    uint4 dv = make_uint4(0u, 0u, 0u, 0u);
    if (prefetch && i0 < n) dv = *reinterpret_cast<const uint4*>(fp.depth[s] + i0);      // (on its way while the table is cleared)
    vox_table_init(T);
    while (have) {
        uint32_t ny = yy, nx = xx + 1u;
        if (nx >= nrx || (tl.rx && (sq_x0 + nx) * 64u >= W)) { nx = 0u; ny = yy + 1u; }
        const bool have_next = ny < nry && !(tl.rx && (sq_y0 + ny) * kVoxRows >= Hh);
        const uint32_t i0n = have_next ? lane_index(ny, nx) : n;
        uint4 dvn = make_uint4(0u, 0u, 0u, 0u);
        if (prefetch && i0n < n) dvn = *reinterpret_cast<const uint4*>(fp.depth[s] + i0n);
        const uint32_t row0 = (sq_y0 + yy) * kVoxRows;
        if (!(tl.rx && !crowded && row0 + ((threadIdx.x >> 6) << 3) >= Hh)) {
            PointIn p[8];
            if (prefetch) src.load8_pre(P, i0, n, dv, p);
            else src.load8(P, i0, n, p);
            const KeepBits keep{keep_mask8(p, i0, n, flags)};

            VoxPoint rec[8];
            auto fill = [&](auto& cv) {
#pragma unroll
                for (int k = 0; k < 8; k++) rec[k] = make_vox_point<Mth::kRowConst>(P, color, p[k], cv);
            };
            if (Mth::kCvtMode == 2) {
                VoxCvt<false> fast;
                fill(fast);
                if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
            } else if (Mth::kCvtMode == 1) {
                VoxCvt<true> fast;
                fill(fast);
                if (__builtin_expect(fast.redo(), 0)) { ExactCvt exact; fill(exact); }
            } else {
                ExactCvt exact;
                fill(exact);
            }
            vox_table_round(T, vs, rec, keep, crowded != 0, key_or, key_orn);
        }
        yy = ny; xx = nx; i0 = i0n; dv = dvn; have = have_next;
    }
    vox_table_flush(T, vs, key_or, key_orn);
}

// The same table fed from a packed payload (16-byte aligned): a lane's 8 consecutive records are 80 contiguous bytes,
// five 16-byte loads. (Requested one round ahead like the raster reader's Z16 quad — 20 registers carried over the table phase, 116
// VGPRs — the voxel grid of the 16 x 1080p cloud measured 0.199-0.201 vs 0.202-0.203 ms at 50 mm, 0.096-0.097 vs 0.094 at 200 mm: not kept.) The point count comes from the host or (counted form) from device memory.
__global__ __launch_bounds__(kVoxThreads)
void pcs_payload_voxel_partials_kernel(const int16_t* __restrict__ payload, uint32_t n_host, const int32_t* __restrict__ n_dev,
                                       VoxelStage vs, int rounds, int crowded)
{
    PCS_VOX_TABLE_DECL;
    const uint32_t n = n_dev ? (uint32_t)max(*n_dev, 0) : n_host;
    const uint32_t tile0 = blockIdx.x * (kVoxRoundPoints * (uint32_t)rounds);
    if (tile0 >= n) return;
    vox_table_init(T);
    for (int round = 0; round < rounds; round++) {
        const uint32_t i0 = tile0 + round * kVoxRoundPoints + threadIdx.x * kPointsPerLane;
        uint32_t w[20];
        if (i0 + 8u <= n) {
            const uint4* q = reinterpret_cast<const uint4*>(payload + (size_t)i0 * PCS_POINT_SHORTS);
#pragma unroll
            for (int j = 0; j < 5; j++) { const uint4 v = q[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
        } else {
#pragma unroll
            for (int j = 0; j < 20; j++) {                        // ragged end: halfword by halfword, zeros past the end
                const uint32_t h0 = (uint32_t)(2 * j), h1 = h0 + 1u;
                const size_t base = (size_t)i0 * PCS_POINT_SHORTS;
                const uint32_t lo = (i0 < n && base + h0 < (size_t)n * PCS_POINT_SHORTS) ? (uint16_t)payload[base + h0] : 0u;
                const uint32_t hi = (i0 < n && base + h1 < (size_t)n * PCS_POINT_SHORTS) ? (uint16_t)payload[base + h1] : 0u;
                w[j] = lo | (hi << 16);
            }
        }
        Record rec[8];
#pragma unroll
        for (int k = 0; k < 8; k += 2) {                          // two records = five dwords: xy zc b|x' y'|z' c'|b'
            const uint32_t* o = w + (k >> 1) * 5;
            rec[k].xy = o[0]; rec[k].zc = o[1]; rec[k].b = o[2] & 0xFFFFu;
            rec[k + 1].xy = perm(o[3], o[2], kHiLo); rec[k + 1].zc = perm(o[4], o[3], kHiLo); rec[k + 1].b = o[4] >> 16;
        }
        uint32_t keep = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) keep |= (uint32_t)(i0 + k < n) << k;
        vox_table_round(T, vs, rec, KeepBits{keep}, crowded != 0, key_or, key_orn);
    }
    vox_table_flush(T, vs, key_or, key_orn);
}


}  // namespace

// ------------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------------

hipError_t launch_fused_voxel_partials(const StreamParams* d_params, int stream0, int n_launch, uint32_t max_points,
                                       uint32_t max_w, uint32_t max_h, bool patch_ok, bool any_dist, uint32_t flags,
                                       MathSel math, const FramePtrs& fp, const VoxelStage& vs, hipStream_t st)
{
    if (n_launch <= 0 || max_points == 0) return hipSuccess;
    // Rounds (4096 pixels each) that share one 2048-slot table. More rounds = fewer partials for the sort, as long as
    // the voxels under one table stay below its slots: a leaf spans leaf / (depth / focal) pixels, so the voxels per
    // round fall roughly with the square of the leaf. A wrong guess costs speed, never correctness (runs that find no
    // slot go out as partials of their own). Capped so that the launch still fills the chip twice over. The packed sums
    // of the table hold at most 8 rounds.
    // (`rounds` below counts SQUARES of 4096 pixels, the unit these measurements were taken in; a workgroup of kVoxThreads lanes
    // covers one in kSub rounds of kVoxRoundPoints pixels — converted just before the launch)
    constexpr int kSub = 4096 / (int)kVoxRoundPoints;
    const uint64_t launch_tiles = (uint64_t)((max_points + 4095u) / 4096u) * (uint64_t)n_launch;
    const uint64_t fill_cap = std::max<uint64_t>(1, (launch_tiles + launch_tiles / 32) / 1024);   // (3 % slack: 16 x 1080p = 8112 squares, 8 per table still fill the chip twice)
    int rounds, rx = 0;
    if (patch_ok) {
        // square patches: 64 x 64 per round, (rx x ry) rounds per workgroup. 16 x 1080p, ms per frame-set with 1 / 2 / 4 /
        // 8 rounds: 10 mm 1.64 / 1.84 / - / -, 25 mm 0.52 / 0.53 / - / -, 36 mm 0.33 / 0.32 / 0.34 / 0.46, 50 mm 0.30 / 0.26 /
        // 0.28 / 0.33, 100 mm 0.26 / 0.23 / 0.23 / 0.25, 200 mm 0.26 / 0.23 / 0.23 / 0.24: two squares (128 x 64) per table
        // from 30 mm up, one below. (Voxels per 128 x 64 patch on the synthetic scene: 780 / 240 / 80 / 30 at 25 / 50 /
        // 100 / 200 mm.)
        // Re-measured after the workgroups were re-ordered (VoxTiling: the chip's last round no longer waits for full patches
        // behind short ones, which is what had made more squares per table lose), 16 x 1080p, ms per call with 2 / 4 / 8 squares:
        //   warm bucket tail   36 mm 0.230 / 0.236 / -, 40 mm 0.217 / 0.210 / -, 45 mm 0.199 / 0.183 / 0.250, 50 mm 0.187 / 0.174 / 0.216,
        //                      100 mm 0.160 / 0.144 / 0.159, 150 mm 0.149 / 0.138 / 0.135, 200 mm 0.147 / 0.136 / 0.135, 300 mm 0.147 / 0.137 / 0.133
        //   its cold chain     40 mm 0.243 / 0.246 / 0.309, 50 mm 0.197 / 0.193 / 0.221, 100 mm 0.167 / 0.158 / 0.163, 200 mm 0.154 / 0.148 / 0.149
        //   LSD tail           30 mm 0.378 / 0.402, 36 mm 0.269 / 0.277, 50 mm 0.227 / 0.222, 100 mm 0.193 / 0.183, 200 mm 0.176 / 0.169
        // (25 mm: one square 0.456, two 0.453; 30 mm: 0.404 / 0.375.) A warm call ends every workgroup with a dearer flush (bucket
        // search, a returning add per bucket it touches, scattered writes), so it gains most from fewer, larger tables.
        const VoxPatchShape shape = vox_patch_shape(vs.leaf, vs.regions != 0u, launch_tiles, 0);      // pcs_vox_tiling.h
        rounds = shape.squares; rx = shape.rx;
    } else {
        const uint64_t by_leaf = std::min<uint64_t>(8, std::max<uint64_t>(3, ((uint64_t)vs.leaf * vs.leaf) / 625u));
        rounds = (int)std::min<uint64_t>(by_leaf, fill_cap);
    }
    rounds *= kSub;
    dim3 grid;
    VoxTiling tl{};
    if (rx) {
        // Two tiers (VoxTiling): the head in (rx x ry) patches; the square-rows that do not fill a head patch (1080 rows = 16
        // square-rows + 56 rows: one of 17 with ry = 2) in (rxb x 1) patches, dealt after all the head patches. Moving MORE of
        // the raster into the tail of small items does not pay — every workgroup costs a table clear and a flush — 16 x 1080p,
        // one warm call, ms with 0 / 25 / 40 / 60 / 100 % of the square-rows in the tail (one box): 50 mm 0.174 / 0.176 / 0.178 /
        // 0.183 / 0.187, 100 mm 0.146 / 0.149 / 0.151 / 0.155 / 0.161.
        tl = vox_tiling_make(max_w, max_h, kVoxRows, (unsigned)rx, (unsigned)rounds / (unsigned)rx, 0);
        grid = dim3((unsigned)(tl.na + tl.nb), (unsigned)n_launch, 1);
    } else {
        const uint32_t tile_points = kVoxRoundPoints * (uint32_t)rounds;
        grid = dim3((max_points + tile_points - 1) / tile_points, (unsigned)n_launch, 1);
    }
    // no stream of the context has a distortion model (or the half-pixel texture convention): the instantiation without
    // their (uniform, but not free in a VALU-bound kernel) tests
#define L(D, M) hipLaunchKernelGGL((pcs_fused_voxel_partials_kernel<D, D, M>), grid, dim3(kVoxThreads), 0, st, d_params, stream0, fp, flags, vs, rounds, tl, vs.leaf < 30u ? 1 : 0)
    const bool ident = (math == MathSel::CertIdentR || math == MathSel::CertIdentRNoOvf || math == MathSel::CertRowConst);
    if (math == MathSel::Ieee) L(true, IeeeMath);
    else if (math == MathSel::CertRowConst && !any_dist) L(false, CertRowConst);
    else if (any_dist) { if (ident) L(true, CertMath<true>); else L(true, CertMath<false>); }
    else               { if (ident) L(false, CertMath<true>); else L(false, CertMath<false>); }
#undef L
    return hipGetLastError();
}

hipError_t launch_payload_voxel_partials(const int16_t* d_payload, uint32_t n_points, const int32_t* d_n_points,
                                         const VoxelStage& vs, hipStream_t st)
{
    if (n_points == 0) return hipSuccess;
    // Rounds of 4096 consecutive records per table (the stitched order is all a payload offers: no square patches).
    // 29.8 M-point config-5 cloud, ms for the voxel grid with 2 / 3 / 4 / 6 rounds: 36 mm 0.48 / 0.40 / 0.46 / 0.60,
    // 50 mm 0.35 / 0.31 / 0.26 / 0.26, 100 mm 0.22 / 0.19 / 0.18 / 0.17 (the 1024-lane reader of pcs_voxel.hip: 0.52 / 0.36 /
    // 0.25). Below 30 mm the tables are crowded and runs are passed through per workgroup (vox_table_round): 10 mm 1.97 ms
    // with 2 rounds (that reader: 2.43), 15 mm 1.35 (1.56), 25 mm 0.72 with 3 rounds (0.81).
    const uint64_t tiles = (n_points + 4095u) / 4096u;                   // (rounds in units of 4096 records, as measured)
    const uint64_t by_leaf = vs.leaf >= 80 ? 6 : vs.leaf >= 44 ? 4 : vs.leaf >= 23 ? 3 : 2;
    int rounds = (int)std::min<uint64_t>(by_leaf, std::max<uint64_t>(1, tiles / 1024));
    rounds *= 4096 / (int)kVoxRoundPoints;
    const uint32_t tile_points = kVoxRoundPoints * (uint32_t)rounds;
    hipLaunchKernelGGL(pcs_payload_voxel_partials_kernel, dim3((n_points + tile_points - 1) / tile_points), dim3(kVoxThreads), 0, st,
                       d_payload, n_points, d_n_points, vs, rounds, vs.leaf < 30u ? 1 : 0);
    return hipGetLastError();
}


}  // namespace pcs
