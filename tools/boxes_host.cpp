// boxes_host.cpp — the arithmetic of the object boxes on the CPU: the same pcs_boxes_math.h that pcs_boxes_axes_kernel compiles, fed
// by a plain loop over the records instead of the grouped wave reductions. tests/test_object_boxes_cpu.py builds it with the host
// compiler and holds it to tests/np_object_boxes.py (Python integers, numpy's eigh) where no GPU is present; the GPU tests hold the
// library to the same restatement.
//
//     g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I pointcloud_stitching_amd/csrc tools/boxes_host.cpp -o libboxes_host.so
#include <climits>
#include <cstdint>
#include <cstring>

#include "pcs_boxes_math.h"

// out: m entries of 128 bytes in pcs_object_box's layout (sixteen little-endian 64-bit words). Returns m.
extern "C" int boxes_host(const int16_t* payload, int n, const int32_t* object_of, int n_objects, int max_objects, void* out)
{
    const int m = n_objects < 0 ? 0 : n_objects < max_objects ? n_objects : max_objects;
    for (int k = 0; k < m; k++) {
        long long count = 0, s1[3] = {0, 0, 0}, m2[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n; i++) {
            if (object_of[i] != k) continue;
            const long long x = payload[5 * i], y = payload[5 * i + 1], z = payload[5 * i + 2];
            count += 1;
            s1[0] += x; s1[1] += y; s1[2] += z;
            m2[0] += x * x; m2[1] += x * y; m2[2] += x * z;
            m2[3] += y * y; m2[4] += y * z; m2[5] += z * z;
        }
        const pcs::BoxAxes ax = pcs::box_axes(count, s1, m2);
        const int16_t axis[3][3] = {{ax.a00, ax.a01, ax.a02}, {ax.a10, ax.a11, ax.a12}, {ax.a20, ax.a21, ax.a22}};
        int32_t lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            lo[a] = count ? INT_MAX : 0;
            hi[a] = count ? INT_MIN : 0;
        }
        for (int i = 0; i < n; i++) {
            if (object_of[i] != k) continue;
            for (int a = 0; a < 3; a++) {
                const int d = pcs::box_project(axis[a][0], axis[a][1], axis[a][2], payload[5 * i], payload[5 * i + 1], payload[5 * i + 2]);
                lo[a] = d < lo[a] ? d : lo[a];
                hi[a] = d > hi[a] ? d : hi[a];
            }
        }
        uint8_t* e = static_cast<uint8_t*>(out) + (size_t)k * 128;
        const int32_t zero = 0;
        std::memcpy(e, &count, 8);
        std::memcpy(e + 8, s1, 24);
        std::memcpy(e + 32, m2, 48);
        std::memcpy(e + 80, axis, 18);
        std::memcpy(e + 98, &ax.rank, 2);
        std::memcpy(e + 100, lo, 12);
        std::memcpy(e + 112, hi, 12);
        std::memcpy(e + 124, &zero, 4);
    }
    return m;
}
