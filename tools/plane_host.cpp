// plane_host.cpp — the arithmetic of pcs_kernels_plane.hip on the CPU: the same pcs_plane_math.h the kernels compile (the hash, the
// draw, the plane through three records with its 128-bit integer square root, the inlier test), behind a C surface for ctypes.
// tests/test_planeseg_cpu.py builds it with the host compiler and holds it to tests/np_planes.py (Python integers, math.isqrt) where
// no GPU is present; the GPU tests hold the library to the same restatement.
//
//     g++ -O2 -std=c++17 -shared -fPIC -I pointcloud_stitching_amd/csrc tools/plane_host.cpp -o libplane_host.so
#include <cstdint>

#include "pcs_plane_math.h"

extern "C" {

uint64_t plane_host_hash(uint64_t key) { return pcs::plane_splitmix64(key); }

uint32_t plane_host_draw(uint32_t seed, uint32_t r, uint32_t h, uint32_t k, uint32_t m) { return pcs::plane_draw(seed, r, h, k, m); }

// floor(sqrt(hi * 2^64 + lo)), for a value below 2^88
uint64_t plane_host_isqrt(uint64_t hi, uint64_t lo) { return pcs::plane_isqrt((unsigned __int128)hi << 64 | lo); }

// eq[5] = nx, ny, nz, off, T of three records (3 shorts each are read); 0: a degenerate triple (eq is the degenerate mark)
int plane_host_plane(const int16_t* p0, const int16_t* p1, const int16_t* p2, int distance_mm, long long* eq)
{
    pcs::PlaneEq e{};
    const bool ok = pcs::plane_from_records(p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2], distance_mm, e);
    eq[0] = e.nx; eq[1] = e.ny; eq[2] = e.nz; eq[3] = e.off; eq[4] = e.t;
    return ok ? 1 : 0;
}

// mask[i] = record i of n (5 shorts each) is an inlier of eq; returns their number
int plane_host_inliers(const int16_t* payload, int n, const long long* eq, uint8_t* mask)
{
    const pcs::PlaneEq e{eq[0], eq[1], eq[2], eq[3], eq[4]};
    int count = 0;
    for (int i = 0; i < n; i++) {
        mask[i] = pcs::plane_inlier(e, payload[5 * i], payload[5 * i + 1], payload[5 * i + 2]) ? 1 : 0;
        count += mask[i];
    }
    return count;
}

}  // extern "C"
