// pcs_plane_math.h — the arithmetic of plane segmentation that the device and the host must agree on bit for bit (DESIGN.md section 3
// "Plane segmentation"): the hash and the draw, the plane through three records with its exact integer threshold (a 128-bit integer
// square root), and the inlier test. Plain C++, integers only; host and device compile the same text, so a CPU program
// (tools/plane_host.cpp) can run what pcs_kernels_plane.hip runs, and pcs_plane_from_points needs no device. Included by
// pcs_kernels_plane.hip and pcs_capi_plane.cpp.
#pragma once

#include <cstdint>

#ifndef PCS_HD
#if defined(__HIPCC__)
#define PCS_HD __host__ __device__ __forceinline__
#else
#define PCS_HD inline
#endif
#endif

namespace pcs {

// A plane as the score kernel reads it, five int64 words: a record p is an inlier iff |n . p - off| <= t. A degenerate hypothesis is
// n = 0, off = 0, t = -1: nobody is an inlier of it, with no branch in the test.
struct PlaneEq {
    long long nx, ny, nz, off, t;
};

PCS_HD uint64_t plane_splitmix64(uint64_t key)
{
    uint64_t z = key + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// draw k (0..2) of hypothesis h (0..4095) of round r (0..7): a position in 0..m-1 (m >= 1)
PCS_HD uint32_t plane_draw(uint32_t seed, uint32_t r, uint32_t h, uint32_t k, uint32_t m)
{
    const uint64_t key = (uint64_t)seed << 32 | (uint64_t)r << 20 | (uint64_t)h << 2 | (uint64_t)k;
    return (uint32_t)(((plane_splitmix64(key) >> 32) * (uint64_t)m) >> 32);
}

// floor(sqrt(v)) for v < 2^88: bit by bit from bit 43 down, one 128-bit product and compare per step; no division.
PCS_HD uint64_t plane_isqrt(unsigned __int128 v)
{
    uint64_t r = 0;
    for (int bit = 43; bit >= 0; bit--) {
        const uint64_t t = r | 1ull << bit;
        if ((unsigned __int128)t * t <= v) r = t;
    }
    return r;
}

// The plane through three records (sign-extended shorts) with inlier distance distance_mm (1..1000). false: the normal is zero (equal
// or collinear records) and e is the degenerate mark. |a|, |b| <= 65535 per component, |n| <= 2 * 65535^2 < 2^34, |off| < 2^51,
// distance_mm^2 * |n|^2 < 2^20 * 3 * 2^66 < 2^88.
PCS_HD bool plane_from_records(int x0, int y0, int z0, int x1, int y1, int z1, int x2, int y2, int z2, int distance_mm, PlaneEq& e)
{
    const long long ax = x1 - x0, ay = y1 - y0, az = z1 - z0, bx = x2 - x0, by = y2 - y0, bz = z2 - z0;
    const long long nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    if (nx == 0 && ny == 0 && nz == 0) {
        e = PlaneEq{0, 0, 0, 0, -1};
        return false;
    }
    const unsigned __int128 n2 = (unsigned __int128)((unsigned long long)(nx < 0 ? -nx : nx)) * (unsigned long long)(nx < 0 ? -nx : nx) +
                                 (unsigned __int128)((unsigned long long)(ny < 0 ? -ny : ny)) * (unsigned long long)(ny < 0 ? -ny : ny) +
                                 (unsigned __int128)((unsigned long long)(nz < 0 ? -nz : nz)) * (unsigned long long)(nz < 0 ? -nz : nz);
    const unsigned long long d2 = (unsigned long long)distance_mm * (unsigned long long)distance_mm;
    e = PlaneEq{nx, ny, nz, nx * x0 + ny * y0 + nz * z0, (long long)plane_isqrt(n2 * d2)};
    return true;
}

// |n . p - off| <= t in int64: three products of a 35-bit by a 16-bit signed value and their sum stay below 2^51, |off| and t are at
// most 2^52 (the library's own planes stay far below; a caller's are checked): nothing wraps.
PCS_HD bool plane_inlier(const PlaneEq& e, int x, int y, int z)
{
    const long long d = e.nx * x + e.ny * y + e.nz * z - e.off;
    return (d < 0 ? -d : d) <= e.t;
}

}  // namespace pcs
