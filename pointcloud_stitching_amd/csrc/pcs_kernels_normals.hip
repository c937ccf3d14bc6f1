// pcs_kernels_normals.hip — per-record surface normals of a packed payload (pcs_estimate_normals_device, DESIGN.md section 3 "Surface
// normals" and section 5). Not in the reference; this project's own definition, parity with PCL's NormalEstimation unpinned.
//
// The neighbourhood of a record q is every record x of the payload with |x - q|^2 <= radius_mm^2 (q itself and its equals included),
// m of them. With delta = x - q: S1 = sum delta, S2 = sum delta delta^T (ten integers with m; |delta_a| <= 1000, int64 is exact),
// C = m S2 - S1 S1^T formed in 128-bit integers, converted to double once; the normal is the eigenvector of C's smallest eigenvalue
// (pcs_normals_math.h: cyclic Jacobi, the validity rules, the sign, the rounding to shorts).
//
// The index is the outlier filter's (pcs_kernels_outlier.hip, stages 0 to 5 over the payload with cell edge radius_mm), read through
// OutlierIndexView; the probe is pcs_outlier_index.h's. A neighbour lies in q's own cell or one of the 26 around it.
//   estimate  one lane per xyz[] entry, in CELL order: a wave's lanes are members of the same few cells and walk the same few runs.
//             A cell whose nearest possible member is beyond the radius is not probed (the match kernel's bound: it can only leave
//             out records that would fail the distance test). The lane's 8 bytes go to cell_normals[e], parallel to xyz[].
//   gather    one lane per input record: its own cell's run is searched for an entry with its coordinates (equal records have
//             equal words, any of them serves) and the 8 bytes are copied to normals[i]; the valid records are counted by wave
//             ballot and one integer atomic add per wave into *valid, which the host layer zeroed on the stream beforehand.
// Determinism: the ten sums are integers (no order reaches them), C is exact, and the double arithmetic behind it is one fixed
// sequence per record: a record's word is a function of its coordinates and the payload as a multiset.
// No hang: every probe loop runs at most `slots` steps (an empty slot ends every miss, as in the flag kernel); the Jacobi loop runs
// at most kNormalSweeps sweeps. Bounds: a lane reads xyz[e] with e < n <= capacity, keys[s] with s < slots, start[at] and
// start[at + 1] with at < slots (slots + 1 starts), xyz[m] with m < min(start[at + 1], capacity), cell_normals[m] likewise; it
// writes cell_normals[e] with e < n, normals[i] with i < n, and *valid.
// Cost: a record costs the population of the cells around it that it cannot rule out, and up to 27 probe sequences; n identical
// records cost n^2 distance tests (there is no early exit: every neighbour enters the sums).

#include "pcs_kernels_common.h"
#include "pcs_outlier_index.h"
#include "pcs_normals_math.h"

namespace pcs {

namespace {

// the slot of a cell's key, kNoSlot where the index has no such cell
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

// ---- estimate ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_normals_estimate_kernel(uint32_t n, NormalRule rule, const unsigned long long* __restrict__ keys,
                                 const uint32_t* __restrict__ start, uint32_t slots, const uint2* __restrict__ xyz, uint32_t capacity,
                                 unsigned long long* __restrict__ cell_normals)
{
    const uint32_t e = blockIdx.x * kBlockThreads + threadIdx.x;
    if (e >= n) return;
    const uint2 w = xyz[e];
    const int px = (int)(int16_t)(w.x & 0xFFFFu), py = (int)(int16_t)(w.x >> 16), pz = (int)(int16_t)(w.y & 0xFFFFu);
    const int radius = rule.radius, r2 = radius * radius;
    const int cx = cell_of(px, radius), cy = cell_of(py, radius), cz = cell_of(pz, radius);
    // per axis: how far a member of the cell one step down / in the same cell / one step up is at least
    const int fx = px - (cx - 32768) * radius, fy = py - (cy - 32768) * radius, fz = pz - (cz - 32768) * radius;
    const auto gap = [radius](int f, int o) { return o == 0 ? f + 1 : o == 1 ? 0 : radius - f; };
    long long m = 0, s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 27; c++) {
        const int ox = c % 3, oy = (c / 3) % 3, oz = c / 9;
        const int ex = gap(fx, ox), ey = gap(fy, oy), ez = gap(fz, oz);
        if (ex * ex + ey * ey + ez * ez > r2) continue;
        const int ax = cx + ox - 1, ay = cy + oy - 1, az = cz + oz - 1;
        if ((uint32_t)ax > 65535u || (uint32_t)ay > 65535u || (uint32_t)az > 65535u) continue;   // no such cell: skipped, never wrapped
        const uint32_t at = find_slot(keys, slots, cell_key(ax, ay, az));
        if (at == kNoSlot) continue;
        const uint32_t end = min(start[at + 1u], capacity);
        for (uint32_t k = start[at]; k < end; k++) {
            const uint2 q = xyz[k];
            // members of adjacent cells: each difference below 2 r + 1 <= 2001, the squares' sum below 2^24
            const int dx = (int)(int16_t)(q.x & 0xFFFFu) - px, dy = (int)(int16_t)(q.x >> 16) - py, dz = (int)(int16_t)(q.y & 0xFFFFu) - pz;
            if (dx * dx + dy * dy + dz * dz > r2) continue;
            m += 1;
            s1[0] += dx; s1[1] += dy; s1[2] += dz;
            s2[0] += dx * dx; s2[1] += dx * dy; s2[2] += dx * dz;          // (|delta_a| <= 1000: a product fits 32 bits)
            s2[3] += dy * dy; s2[4] += dy * dz; s2[5] += dz * dz;
        }
    }
    cell_normals[e] = normal_word(m, s1, s2, rule, px, py, pz);
}

// ---- gather -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads)
void pcs_normals_gather_kernel(const int16_t* __restrict__ in, uint32_t n, int radius, const unsigned long long* __restrict__ keys,
                               const uint32_t* __restrict__ start, uint32_t slots, const uint2* __restrict__ xyz, uint32_t capacity,
                               const unsigned long long* __restrict__ cell_normals, unsigned long long* __restrict__ normals,
                               int32_t* __restrict__ valid)
{
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const Xyz p = load_xyz(in, i);
        const uint2 want = make_uint2((uint32_t)(uint16_t)p.x | (uint32_t)(uint16_t)p.y << 16, (uint32_t)(uint16_t)p.z);
        unsigned long long word = 0ull;      // (a record the index does not hold cannot happen: it would read as invalid)
        const uint32_t at = find_slot(keys, slots, cell_key(cell_of(p.x, radius), cell_of(p.y, radius), cell_of(p.z, radius)));
        if (at != kNoSlot) {
            const uint32_t end = min(start[at + 1u], capacity);
            for (uint32_t k = start[at]; k < end; k++) {
                const uint2 q = xyz[k];
                if (q.x == want.x && q.y == want.y) { word = cell_normals[k]; break; }
            }
        }
        normals[i] = word;
        ok = word != 0ull;
    }
    if (valid) {
        const unsigned long long bits = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && bits) atomicAdd(valid, (int32_t)__popcll(bits));
    }
}

bool view_ok(const OutlierIndexView& v) { return v.keys && v.start && v.xyz && v.slots && v.capacity; }

}  // namespace

hipError_t launch_normals_estimate(uint32_t n_points, const OutlierIndexView& index, const NormalRule& rule,
                                   unsigned long long* d_cell_normals, hipStream_t st)
{
    if (!n_points || !view_ok(index) || n_points > index.capacity || !d_cell_normals || rule.radius < 1 || rule.radius > 1000)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_normals_estimate_kernel, dim3((n_points + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st,
                       n_points, rule, index.keys, index.start, index.slots, index.xyz, index.capacity, d_cell_normals);
    return hipGetLastError();
}

hipError_t launch_normals_gather(const int16_t* d_in, uint32_t n_points, int radius_mm, const OutlierIndexView& index,
                                 const unsigned long long* d_cell_normals, unsigned long long* d_normals, int32_t* d_valid, hipStream_t st)
{
    if (!n_points || !d_in || !view_ok(index) || n_points > index.capacity || !d_cell_normals || !d_normals || radius_mm < 1 ||
        radius_mm > 1000 || ((uintptr_t)d_normals & 7u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pcs_normals_gather_kernel, dim3((n_points + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, d_in,
                       n_points, radius_mm, index.keys, index.start, index.slots, index.xyz, index.capacity, d_cell_normals, d_normals,
                       d_valid);
    return hipGetLastError();
}

}  // namespace pcs
