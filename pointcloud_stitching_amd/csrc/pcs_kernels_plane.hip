// pcs_kernels_plane.hip — RANSAC plane segmentation on a packed payload (pcs_plane_segment_device, pcs_plane_labels_device,
// pcs_plane_count_inliers_device; DESIGN.md section 3 "Plane segmentation" and section 5): per round, `iterations` hypotheses each draw
// three records of the round's cloud (the records in no plane accepted so far, input order) by a counter hash, the plane through them
// is scored by its inliers |N . p - off| <= T over the whole cloud, the best (ties: the smallest hypothesis) is accepted if it has
// min_inliers, its inliers get the round's number as their label and leave the cloud. Everything in the payload's integer millimetres;
// the arithmetic both sides must agree on is pcs_plane_math.h. Not in the reference; modelled on PCL's SACSegmentation, parity unpinned.
//
//   init         the control block (count, round count m, stopped, planes, degenerate), the models zeroed, labels[i] = -1
//   hypotheses   one lane per hypothesis: three draws from m, the records through the round's cloud, their input indices through its
//                origin array; N, off, T as five int64 — or the degenerate mark (N = 0, T = -1: nobody passes the test) — and a zeroed
//                score. The family's control block gets the round's m for the compaction behind the round.
//   score        THE HOT LAUNCH: iterations x m inlier tests. A workgroup holds a tile of 2048 records in registers (eight per lane,
//                lane-interleaved: one 10-byte stride across a wave per load) and walks the hypotheses; a hypothesis's five words are
//                wave-uniform (scalar loads); a wave counts its inliers by ballot and popcount (a scalar), one lane adds them to the
//                workgroup's LDS word of the hypothesis; at the end one global add per hypothesis and workgroup that has any.
//                The int64 dot is three 64 x 32 products over coordinates biased to be unsigned, and the two-sided test one unsigned
//                compare (the kernel's comment has the identity: the same bits for every input).
//   select       one workgroup: the largest score, ties to the smallest h; m < 3 or a score below min_inliers stops the segmentation
//                (stopped = 1, the family's count = 0: the compaction launches behind it find nothing to do); else model block r.
//   mark         one lane per record of the round's cloud: an inlier of model r gets labels[origin] = r; the keep bits (not an inlier)
//                in the radius filter's layout, whose tile count, tile scan and emit run unchanged behind it: the next round's cloud,
//                its count straight into m
//   origins      the next round's origin indices: the same ranks as emit's (keep byte per lane, wave scan, the scan's tile prefix)
//   finish       filter form: keep bits over the INPUT by label and mode, the family's count = the input's, so that the same
//                compaction emits the result; both forms: the model blocks, the statistics block, n_planes to the caller
//
// Properties:
//   determinism  scores are integer adds, the argmax has a total order (score, then h), labels are written by value r once per record
//                and round: nothing depends on the order in which atomics arrive.
//   no hang      no loop waits on another lane; every loop is bounded by iterations, by the tile or by 44 (the square root).
//   bounds       a draw is below m by construction (a 32 x 32 -> high 32 product); clouds and origins hold `capacity` >= m entries;
//                an origin is a position of the input below its count, so labels[] is written below the count only; eqs, scores and
//                samples hold kPlaneMaxHypotheses entries and iterations is checked against it by the launcher; models hold
//                kPlaneMaxPlanes blocks and round < max_planes <= kPlaneMaxPlanes.
//   a round after the stop   every kernel here returns on `stopped`; the three compaction launches see a count of 0.
// Workspace: 247 552 bytes (planes, scores, samples, control, models, the host forms' staging) + the radius filter's
// (outlier_workspace_bytes: its control block, keep bits and tile words are used) + per record 4 (labels) + 2 x 10 (the rounds' clouds,
// ping-pong) + 2 x 4 (their origins) = 32 bytes. Integer arithmetic throughout: no float anywhere in this file.

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"
#include "pcs_plane_math.h"

namespace pcs {

namespace {

struct PlaneCtl {
    uint32_t           n0, m, stopped, n_planes;     // the input's count; the round's; the segmentation ended; accepted so far
    unsigned long long degenerate;                   // hypotheses with N = 0, over the rounds that drew
};

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ PlaneEq load_eq(const long long* __restrict__ w)
{
    return PlaneEq{w[0], w[1], w[2], w[3], w[4]};
}

// ---- init -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_plane_init_kernel(PlaneCtl* __restrict__ pc, OutlierCtl* __restrict__ ctl, const int32_t* __restrict__ d_n, uint32_t n_host,
                           uint32_t capacity, long long* __restrict__ models, int32_t* __restrict__ labels)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t n = n_host;
    if (d_n) { const int32_t v = *d_n; n = v < 0 ? 0u : min((uint32_t)v, capacity); }
    if (i == 0u) {
        pc->n0 = n; pc->m = n; pc->stopped = 0u; pc->n_planes = 0u; pc->degenerate = 0ull;
        ctl->tab.n_points = n;
        ctl->tab.tile_base = 0u;
    }
    if (i < 8u * kPlaneMaxPlanes) models[i] = 0ll;
    if (i < n) labels[i] = -1;
}

// ---- hypotheses -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_plane_hypotheses_kernel(const int16_t* __restrict__ cloud, const uint32_t* __restrict__ origin, PlaneCtl* pc,
                                 OutlierCtl* __restrict__ ctl, uint32_t round, uint32_t seed, int distance_mm, uint32_t iterations,
                                 long long* __restrict__ eqs, unsigned long long* __restrict__ scores, int32_t* __restrict__ samples)
{
    if (pc->stopped) return;
    const uint32_t h = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t m = pc->m;
    if (h == 0u) {               // what the compaction behind this round counts, scans and emits
        ctl->tab.n_points = m;
        ctl->tab.tile_base = 0u;
    }
    bool degenerate = false;
    if (h < iterations) {
        PlaneEq e{0, 0, 0, 0, -1};
        uint32_t at[3] = {0u, 0u, 0u};
        if (m >= 3u) {
            Xyz p[3];
#pragma unroll
            for (uint32_t k = 0; k < 3u; k++) {
                const uint32_t pos = plane_draw(seed, round, h, k, m);
                p[k] = load_xyz(cloud, pos);
                at[k] = origin ? origin[pos] : pos;
            }
            degenerate = !plane_from_records(p[0].x, p[0].y, p[0].z, p[1].x, p[1].y, p[1].z, p[2].x, p[2].y, p[2].z, distance_mm, e);
        }
        long long* w = eqs + 5u * h;
        w[0] = e.nx; w[1] = e.ny; w[2] = e.nz; w[3] = e.off; w[4] = e.t;
        scores[h] = 0ull;
        samples[3u * h] = (int32_t)at[0]; samples[3u * h + 1u] = (int32_t)at[1]; samples[3u * h + 2u] = (int32_t)at[2];
    }
    const unsigned long long bal = __ballot(degenerate);
    if (bal && lane_id() == 0u) atomicAdd(&pc->degenerate, (unsigned long long)__popcll(bal));
}

// ---- score ------------------------------------------------------------------------------------------
// pc NULL (pcs_plane_count_inliers_device): the count is n_host and nothing stops. scores[h] += the tile's inliers of plane h.
// The test |N . p - off| <= T in the form the loop runs, the same bits for every input (all of it is arithmetic modulo 2^64 on a value
// that fits: |N . p - off| + T < 2^54 for everything the host lets in):
//   coordinates biased to u = p + 32768 (0 .. 65535, zero-extended), so that a 64 x 32 product is one 32 x 32 -> 64 multiply-add of the
//   low word and one 24-bit multiply of the high word (|n| <= 2^34: it is -4 .. 4), with no sign to carry:
//   N . p = N . u - 32768 (nx + ny + nz);
//   |d| <= T  <=>  0 <= d + T <= 2 T  <=>  (unsigned)(d + T) <= 2 T for T >= 0 (a negative d + T reads as 2^63 or more): no absolute
//   value; the wave-uniform start value base = T - off - 32768 (nx + ny + nz) carries everything that does not depend on the record;
//   the degenerate mark (N = 0, off = 0, T = -1) gets start -1 and span 0: (unsigned)(-1) <= 0 is false for everybody.
// A record at or beyond m is masked out of the ballot by its slot's wave-uniform live mask: no branch in the loop.
__global__ __launch_bounds__(kBlockThreads)
void pcs_plane_score_kernel(const int16_t* __restrict__ in, const PlaneCtl* __restrict__ pc, uint32_t n_host,
                            const long long* __restrict__ eqs, uint32_t n_eqs, unsigned long long* __restrict__ scores)
{
    __shared__ uint32_t acc[kPlaneMaxHypotheses];
    if (pc && pc->stopped) return;
    const uint32_t m = pc ? pc->m : n_host;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= m) return;
    for (uint32_t h = threadIdx.x; h < n_eqs; h += kBlockThreads) acc[h] = 0u;
    uint32_t ux[kPointsPerLane], uy[kPointsPerLane], uz[kPointsPerLane];
    unsigned long long live[kPointsPerLane];                             // wave-uniform
#pragma unroll
    for (int k = 0; k < kPointsPerLane; k++) {
        const uint32_t i = tile0 + (uint32_t)k * kBlockThreads + threadIdx.x;
        ux[k] = uy[k] = uz[k] = 0u;
        if (i < m) {
            const Xyz p = load_xyz(in, i);
            ux[k] = (uint32_t)(p.x + 32768); uy[k] = (uint32_t)(p.y + 32768); uz[k] = (uint32_t)(p.z + 32768);
        }
        live[k] = __ballot(i < m);
    }
    __syncthreads();
    for (uint32_t h = 0; h < n_eqs; h++) {
        const PlaneEq e = load_eq(eqs + 5u * h);                         // wave-uniform
        const unsigned long long nx = (unsigned long long)e.nx, ny = (unsigned long long)e.ny, nz = (unsigned long long)e.nz;
        const unsigned long long span = e.t < 0 ? 0ull : 2ull * (unsigned long long)e.t;
        const unsigned long long base = (unsigned long long)(e.t < 0 ? -1ll : e.t) - (unsigned long long)e.off - 32768ull * (nx + ny + nz);
        // n = nh 2^32 + nl with nl unsigned and nh = n >> 32 arithmetic, |nh| <= 4: n u = nl u + (nh u) 2^32, the second a 24-bit product
        const uint32_t nxl = (uint32_t)nx, nyl = (uint32_t)ny, nzl = (uint32_t)nz;
        const int nxh = (int)(e.nx >> 32), nyh = (int)(e.ny >> 32), nzh = (int)(e.nz >> 32);
        uint32_t count = 0u;                                             // wave-uniform
#pragma unroll
        for (int k = 0; k < kPointsPerLane; k++) {
            const uint32_t high = (uint32_t)(__mul24(nxh, (int)ux[k]) + __mul24(nyh, (int)uy[k]) + __mul24(nzh, (int)uz[k]));
            const unsigned long long v = base + (unsigned long long)nxl * ux[k] + (unsigned long long)nyl * uy[k] +
                                         (unsigned long long)nzl * uz[k] + ((unsigned long long)high << 32);
            count += (uint32_t)__popcll(__ballot(v <= span) & live[k]);
        }
        if (count && lane_id() == 0u) atomicAdd(&acc[h], count);
    }
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < n_eqs; h += kBlockThreads) {
        const uint32_t v = acc[h];
        if (v) atomicAdd(scores + h, (unsigned long long)v);
    }
}

// ---- select -----------------------------------------------------------------------------------------
// A model block is eight int64: nx, ny, nz, off, threshold, inliers, sample[0] | sample[1] << 32, sample[2] | hypothesis << 32.
__global__ __launch_bounds__(kBlockThreads)
void pcs_plane_select_kernel(PlaneCtl* pc, OutlierCtl* __restrict__ ctl, uint32_t round, uint32_t iterations, uint32_t min_inliers,
                             const long long* __restrict__ eqs, const unsigned long long* __restrict__ scores,
                             const int32_t* __restrict__ samples, long long* __restrict__ models)
{
    __shared__ unsigned long long best_score[kBlockThreads];
    __shared__ uint32_t best_h[kBlockThreads];
    if (pc->stopped) return;
    unsigned long long bs = 0ull;
    uint32_t bh = 0xFFFFFFFFu;
    for (uint32_t h = threadIdx.x; h < iterations; h += kBlockThreads) {       // h ascends: a later equal score does not replace
        const unsigned long long s = scores[h];
        if (s > bs) { bs = s; bh = h; }
    }
    best_score[threadIdx.x] = bs;
    best_h[threadIdx.x] = bh;
    __syncthreads();
    for (uint32_t stride = kBlockThreads / 2; stride >= 1u; stride >>= 1) {
        if (threadIdx.x < stride) {
            const unsigned long long os = best_score[threadIdx.x + stride];
            const uint32_t oh = best_h[threadIdx.x + stride];
            if (os > best_score[threadIdx.x] || (os == best_score[threadIdx.x] && oh < best_h[threadIdx.x])) {
                best_score[threadIdx.x] = os;
                best_h[threadIdx.x] = oh;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0u) return;
    bs = best_score[0];
    bh = best_h[0];
    if (pc->m < 3u || bs < (unsigned long long)min_inliers || bh >= iterations) {
        pc->stopped = 1u;
        ctl->tab.n_points = 0u;
        return;
    }
    long long* M = models + 8u * round;
    const long long* w = eqs + 5u * bh;
    M[0] = w[0]; M[1] = w[1]; M[2] = w[2]; M[3] = w[3]; M[4] = w[4];
    M[5] = (long long)bs;
    M[6] = (long long)((unsigned long long)(uint32_t)samples[3u * bh] | (unsigned long long)(uint32_t)samples[3u * bh + 1u] << 32);
    M[7] = (long long)((unsigned long long)(uint32_t)samples[3u * bh + 2u] | (unsigned long long)bh << 32);
    pc->n_planes = round + 1u;
}

// ---- mark -------------------------------------------------------------------------------------------
// keep_bits[w] = the ballot of positions 64 w .. 64 w + 63 of the round's cloud (a bit at or beyond m is 0): the radius filter's layout.
__global__ __launch_bounds__(kBlockThreads)
void pcs_plane_mark_kernel(const int16_t* __restrict__ cloud, const uint32_t* __restrict__ origin, const PlaneCtl* __restrict__ pc,
                           uint32_t round, const long long* __restrict__ models, int32_t* __restrict__ labels,
                           unsigned long long* __restrict__ keep_bits)
{
    if (pc->stopped) return;
    const uint32_t p = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t m = pc->m;
    const PlaneEq e = load_eq(models + 8u * round);
    bool keep = false;
    if (p < m) {
        const Xyz q = load_xyz(cloud, p);
        const bool inlier = plane_inlier(e, q.x, q.y, q.z);
        if (inlier) labels[origin ? origin[p] : p] = (int32_t)round;
        keep = !inlier;
    }
    const unsigned long long bits = __ballot(keep);
    if (lane_id() == 0u) keep_bits[p >> 6] = bits;
}

// ---- origins ----------------------------------------------------------------------------------------
// The kept positions' origins to the ranks the emit launch gave their records: lane l of a tile's workgroup owns positions 8 l .. 8 l + 7
// and keep byte l, as there.
__global__ __launch_bounds__(kBlockThreads)
void pcs_plane_origins_kernel(const PlaneCtl* __restrict__ pc, const OutlierCtl* __restrict__ ctl, const uint8_t* __restrict__ keep_bytes,
                              const uint32_t* __restrict__ tile_prefix, const uint32_t* __restrict__ origin_in,
                              uint32_t* __restrict__ origin_out)
{
    __shared__ uint32_t wsum[kBlockThreads / 64];
    if (pc->stopped) return;
    const uint32_t n = ctl->tab.n_points;
    const uint32_t tile0 = blockIdx.x * kTilePoints;
    if (tile0 >= n) return;
    const uint32_t pts = min(kTilePoints, n - tile0);
    const uint32_t j0 = threadIdx.x * kPointsPerLane;
    const uint32_t keep = j0 < pts ? keep_bytes[(size_t)blockIdx.x * kBlockThreads + threadIdx.x] : 0u;
    uint32_t wave_total;
    const uint32_t ex = wave_exclusive_scan(__popc(keep), wave_total);
    if (lane_id() == 63u) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    uint32_t q = tile_prefix[blockIdx.x] + ex;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) q += wsum[w];
#pragma unroll
    for (int k = 0; k < kPointsPerLane; k++)
        if ((keep >> k) & 1u) {
            const uint32_t i = tile0 + j0 + (uint32_t)k;
            origin_out[q++] = origin_in ? origin_in[i] : i;
        }
}

// ---- finish -----------------------------------------------------------------------------------------
// keep_bits NULL: the labels form (one workgroup). stats[] = considered, planes, inliers_total, kept, largest_plane,
// degenerate_hypotheses, 0, 0.
__global__ __launch_bounds__(kBlockThreads)
void pcs_plane_finish_kernel(const PlaneCtl* __restrict__ pc, OutlierCtl* __restrict__ ctl, int mode, uint32_t max_planes,
                             const long long* __restrict__ models, const int32_t* __restrict__ labels,
                             unsigned long long* __restrict__ keep_bits, long long* __restrict__ out_models, long long* __restrict__ stats,
                             int32_t* __restrict__ n_planes)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t n0 = pc->n0;
    if (keep_bits) {
        bool keep = false;
        if (i < n0) keep = mode ? labels[i] >= 0 : labels[i] < 0;
        const unsigned long long bits = __ballot(keep);
        if (lane_id() == 0u) keep_bits[i >> 6] = bits;
    }
    if (out_models && i < 8u * max_planes) out_models[i] = models[i];
    if (i != 0u) return;
    ctl->tab.n_points = n0;
    ctl->tab.tile_base = 0u;
    const uint32_t planes = pc->n_planes;
    if (n_planes) *n_planes = (int32_t)planes;
    if (stats) {
        long long total = 0, largest = 0;
        for (uint32_t r = 0; r < planes; r++) {
            const long long c = models[8u * r + 5u];
            total += c;
            largest = max(largest, c);
        }
        stats[0] = (long long)n0;
        stats[1] = (long long)planes;
        stats[2] = total;
        stats[3] = mode ? total : (long long)n0 - total;
        stats[4] = largest;
        stats[5] = (long long)pc->degenerate;
        stats[6] = 0ll;
        stats[7] = 0ll;
    }
}

constexpr size_t kEqBytes      = (size_t)kPlaneMaxHypotheses * 5 * sizeof(long long);       // 163 840
constexpr size_t kScoreBytes   = (size_t)kPlaneMaxHypotheses * sizeof(unsigned long long);  //  32 768
constexpr size_t kSampleBytes  = (size_t)kPlaneMaxHypotheses * 3 * sizeof(int32_t);         //  49 152
constexpr size_t kModelBytes   = (size_t)kPlaneMaxPlanes * 64;                              //     512
constexpr size_t kStagingBytes = 1024;                                                      // models, statistics, n_planes of a host form
constexpr size_t kFixedBytes   = kEqBytes + kScoreBytes + kSampleBytes + 256 + kModelBytes + kStagingBytes;
static_assert(kFixedBytes % 256 == 0 && kEqBytes % 256 == 0, "the slab is carved at 256 bytes");

// Where the pieces of a workspace lie.
struct PlaneCarve {
    long long*          eqs;
    unsigned long long* scores;
    int32_t*            samples;
    PlaneCtl*           pc;
    long long*          models;
    uint8_t*            staging;
    void*               index;
    size_t              index_bytes;
    int32_t*            labels;
    int16_t*            cloud[2];
    uint32_t*           origin[2];

    PlaneCarve(uint32_t capacity, void* d_ws) : index_bytes(up256(outlier_workspace_bytes(capacity)))
    {
        uint8_t* w = static_cast<uint8_t*>(d_ws);
        auto carve = [&](size_t bytes) { uint8_t* p = w; w += up256(bytes); return p; };
        eqs     = reinterpret_cast<long long*>(carve(kEqBytes));
        scores  = reinterpret_cast<unsigned long long*>(carve(kScoreBytes));
        samples = reinterpret_cast<int32_t*>(carve(kSampleBytes));
        pc      = reinterpret_cast<PlaneCtl*>(carve(sizeof(PlaneCtl)));
        models  = reinterpret_cast<long long*>(carve(kModelBytes));
        staging = carve(kStagingBytes);
        index   = carve(index_bytes);
        labels  = reinterpret_cast<int32_t*>(carve(4 * (size_t)capacity));
        for (int k = 0; k < 2; k++) cloud[k] = reinterpret_cast<int16_t*>(carve((size_t)PCS_POINT_BYTES * capacity));
        for (int k = 0; k < 2; k++) origin[k] = reinterpret_cast<uint32_t*>(carve(4 * (size_t)capacity));
    }
};

}  // namespace

size_t plane_workspace_bytes(uint32_t capacity)
{
    return kFixedBytes + up256(outlier_workspace_bytes(capacity)) + 3 * up256(4 * (size_t)capacity) +
           2 * up256((size_t)PCS_POINT_BYTES * capacity);
}

size_t plane_count_workspace_bytes() { return kEqBytes; }

long long* plane_count_planes(void* d_ws) { return static_cast<long long*>(d_ws); }

void* plane_host_staging(uint32_t capacity, void* d_ws) { return PlaneCarve(capacity, d_ws).staging; }

const char* plane_step_name(int step)
{
    static const char* const names[kPlaneSteps] = {"init", "hypotheses", "score", "select", "mark", "tile count", "tile scan", "emit", "origins",
                                                   "finish", "out tile count", "out tile scan", "out emit"};
    return step >= 0 && step < kPlaneSteps ? names[step] : "?";
}

hipError_t launch_plane_step(const PlaneJob& job, int step, int round, hipStream_t st)
{
    const uint32_t capacity = job.capacity;
    if (!capacity || job.distance_mm < PCS_PLANE_DISTANCE_MIN || job.distance_mm > PCS_PLANE_DISTANCE_MAX || job.iterations < 1 ||
        job.iterations > kPlaneMaxHypotheses || job.min_inliers < 3 || job.max_planes < 1 || job.max_planes > kPlaneMaxPlanes ||
        (job.mode != PCS_PLANE_MODE_REMOVE && job.mode != PCS_PLANE_MODE_KEEP) || round < 0 || round >= job.max_planes ||
        job.ws_bytes < plane_workspace_bytes(capacity) || ((uintptr_t)job.d_ws & 255u) || (!job.d_n_points && job.n_points > capacity))
        return hipErrorInvalidValue;
    const PlaneCarve cv(capacity, job.d_ws);
    OutlierKeepView kv{};
    if (hipError_t e = outlier_keep_view(capacity, cv.index, cv.index_bytes, &kv)) return e;
    OutlierCtl* const ctl = const_cast<OutlierCtl*>(kv.ctl);                       // the workspace is this call's
    int32_t* const labels = job.d_labels ? job.d_labels : cv.labels;
    // round r reads the input (r = 0: positions are input indices, no origin array) or what round r - 1 emitted, and emits into the other
    const int16_t* const cloud = round == 0 ? job.d_in : cv.cloud[(round - 1) & 1];
    const uint32_t* const origin = round == 0 ? nullptr : cv.origin[(round - 1) & 1];
    const dim3 per_record((capacity + kBlockThreads - 1) / kBlockThreads), per_tile((capacity + kTilePoints - 1) / kTilePoints), threads(kBlockThreads);
    switch (step) {
    case kPlaneInit:
        hipLaunchKernelGGL(pcs_plane_init_kernel, per_record, threads, 0, st, cv.pc, ctl, job.d_n_points, job.n_points, capacity, cv.models, labels);
        break;
    case kPlaneHypotheses:
        hipLaunchKernelGGL(pcs_plane_hypotheses_kernel, dim3(((uint32_t)job.iterations + kBlockThreads - 1) / kBlockThreads), threads, 0, st, cloud,
                           origin, cv.pc, ctl, (uint32_t)round, job.seed, job.distance_mm, (uint32_t)job.iterations, cv.eqs, cv.scores, cv.samples);
        break;
    case kPlaneScore:
        hipLaunchKernelGGL(pcs_plane_score_kernel, per_tile, threads, 0, st, cloud, cv.pc, 0u, cv.eqs, (uint32_t)job.iterations, cv.scores);
        break;
    case kPlaneSelect:
        hipLaunchKernelGGL(pcs_plane_select_kernel, dim3(1), threads, 0, st, cv.pc, ctl, (uint32_t)round, (uint32_t)job.iterations,
                           (uint32_t)job.min_inliers, cv.eqs, cv.scores, cv.samples, cv.models);
        break;
    case kPlaneMark:
        hipLaunchKernelGGL(pcs_plane_mark_kernel, per_record, threads, 0, st, cloud, origin, cv.pc, (uint32_t)round, cv.models, labels, kv.keep_bits);
        break;
    case kPlaneTileCount: case kPlaneTileScan: case kPlaneEmit:      // the next round's cloud; its count lands in m
        return launch_outlier_compact_stage(7 + (step - kPlaneTileCount), cloud, capacity, cv.index, cv.index_bytes, cv.cloud[round & 1],
                                            reinterpret_cast<int32_t*>(&cv.pc->m), st);
    case kPlaneOrigins:
        hipLaunchKernelGGL(pcs_plane_origins_kernel, per_tile, threads, 0, st, cv.pc, kv.ctl, reinterpret_cast<const uint8_t*>(kv.keep_bits),
                           kv.tile_prefix, origin, cv.origin[round & 1]);
        break;
    case kPlaneFinish: {
        const bool filter = job.d_out_points != nullptr;
        hipLaunchKernelGGL(pcs_plane_finish_kernel, filter ? per_record : dim3(1), threads, 0, st, cv.pc, ctl, job.mode, (uint32_t)job.max_planes,
                           cv.models, labels, filter ? kv.keep_bits : nullptr, static_cast<long long*>(job.d_models), job.d_stats, job.d_n_planes);
        break;
    }
    case kPlaneOutCount: case kPlaneOutScan: case kPlaneOutEmit:
        if (!job.d_out_points) return hipErrorInvalidValue;
        return launch_outlier_compact_stage(7 + (step - kPlaneOutCount), job.d_in, capacity, cv.index, cv.index_bytes, job.d_out, job.d_out_points,
                                            st);
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_plane_count(const int16_t* d_in, uint32_t n_points, void* d_ws, size_t ws_bytes, uint32_t n_models,
                              unsigned long long* d_counts, hipStream_t st)
{
    if (!n_points || !n_models || n_models > (uint32_t)kPlaneMaxHypotheses || ws_bytes < plane_count_workspace_bytes() ||
        ((uintptr_t)d_ws & 255u) || !d_counts)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_plane_score_kernel, dim3((n_points + kTilePoints - 1) / kTilePoints), dim3(kBlockThreads), 0, st, d_in,
                       static_cast<const PlaneCtl*>(nullptr), n_points, plane_count_planes(d_ws), n_models, d_counts);
    return hipGetLastError();
}

}  // namespace pcs
