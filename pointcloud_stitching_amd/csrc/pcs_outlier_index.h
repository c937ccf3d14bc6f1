// pcs_outlier_index.h — the uniform-grid neighbour index's device-side vocabulary: what a kernel needs to find a cell's run in the
// index that the kIndexStages launches of launch_cell_index_stage build (pcs_kernels_outlier.hip has the build and its description).
// Included by pcs_kernels_outlier.hip (radius outlier removal), pcs_kernels_stat.hip (statistical outlier removal),
// pcs_kernels_align.hip (alignment sums), pcs_kernels_normals.hip (surface normals), pcs_kernels_cluster.hip (Euclidean clusters)
// and pcs_kernels_plane.hip (plane segmentation: load_xyz alone), never compiled alone.
#pragma once

#include "pcs_kernels_common.h"

namespace pcs {

namespace {

constexpr unsigned long long kEmptyKey   = ~0ull;                                // (a key has 48 bits)
constexpr uint32_t           kNoSlot     = 0xFFFFFFFFu;

// ---- cells ------------------------------------------------------------------------------------------
struct Xyz { int x, y, z; };

// the three coordinate shorts of record i, sign-extended (2-byte loads: a payload may sit at any 2-byte phase)
__device__ __forceinline__ Xyz load_xyz(const int16_t* __restrict__ in, uint32_t i)
{
    const int16_t* p = in + (size_t)i * PCS_POINT_SHORTS;
    return Xyz{p[0], p[1], p[2]};
}

// floor(v / r) + 32768 for r >= 1: 0 .. 65535 (C++ division truncates; negative coordinates must floor)
__device__ __forceinline__ int cell_of(int v, int r)
{
    const int q = v / r;
    return q - (int)(v - q * r < 0) + 32768;
}

__device__ __forceinline__ unsigned long long cell_key(int cx, int cy, int cz)
{
    return (unsigned long long)(uint32_t)cx | (unsigned long long)(uint32_t)cy << 16 | (unsigned long long)(uint32_t)cz << 32;
}

// where a key's probe sequence starts: a 64-bit finaliser's top bits scaled to [0, slots)
// (restated in numpy by tests/test_radius_outlier_scale.py, with cell_of, cell_key and outlier_slots, to build a cloud whose probes wrap)
__device__ __forceinline__ uint32_t first_slot(unsigned long long k, uint32_t slots)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return __umulhi((uint32_t)k, slots);
}

}  // namespace

}  // namespace pcs
