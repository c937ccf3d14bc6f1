// host_helpers_check.cpp — the pure helpers of csrc/pcs_host.h and csrc/pcs_device.h (ranges_overlap, first_overlap, up256) under the
// host sanitizers. A stand-alone program: no GPU, no library, nothing loaded into Python; it calls nothing of HIP.
//
//   make -C pointcloud_stitching_amd/csrc ../../tools/bin/host_helpers_check && tools/bin/host_helpers_check
#include <cstdio>
#include <cstdlib>

#include "../pointcloud_stitching_amd/csrc/pcs_host.h"

using namespace pcs_host;

static int g_failed = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } } while (0)

int main()
{
    // ---- ranges_overlap: addresses only, nothing is dereferenced
    char* const buf = static_cast<char*>(malloc(64));
    EXPECT(ranges_overlap(buf, 16, buf, 16));
    EXPECT(ranges_overlap(buf, 16, buf + 15, 1) && ranges_overlap(buf + 15, 1, buf, 16));            // the last byte
    EXPECT(!ranges_overlap(buf, 16, buf + 16, 16) && !ranges_overlap(buf + 16, 16, buf, 16));         // abutting
    EXPECT(ranges_overlap(buf, 64, buf + 20, 4) && ranges_overlap(buf + 20, 4, buf, 64));             // nested
    EXPECT(!ranges_overlap(buf, 0, buf, 16) && !ranges_overlap(buf, 16, buf, 0) && !ranges_overlap(buf + 8, 0, buf, 16));   // zero length
    EXPECT(!ranges_overlap(nullptr, 16, buf, 16) && !ranges_overlap(buf, 16, nullptr, 16) && !ranges_overlap(nullptr, 16, nullptr, 16));
    EXPECT(!ranges_overlap(nullptr, 0, buf, 16) && !ranges_overlap(nullptr, (size_t)-1, buf, 16));    // NULL with any length
    const void* const low = reinterpret_cast<const void*>((uintptr_t)8);                               // a range that would cover address 8
    EXPECT(!ranges_overlap(nullptr, 4096, low, 4));
    EXPECT(kMaxPoints == 214748364 && (long long)kMaxPoints * PCS_POINT_BYTES <= INT_MAX && ((long long)kMaxPoints + 1) * PCS_POINT_BYTES > INT_MAX);

    // ---- up256
    EXPECT(up256(0) == 0 && up256(1) == 256 && up256(255) == 256 && up256(256) == 256 && up256(257) == 512);
    EXPECT(up256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256);

    // ---- first_overlap: the loop's table — every output against every input, then against the outputs in front of it
    const NamedRange ins[] = {{buf, 16, "in0"}, {buf + 16, 8, "in1"}, {nullptr, 8, "absent"}};
    const NamedRange* with = nullptr;
    {
        const NamedRange outs[] = {{buf + 24, 8, "a"}, {buf + 32, 8, "b"}, {nullptr, 32, "none"}, {buf + 40, 0, "empty"}};
        EXPECT(first_overlap(outs, 4, ins, 3, &with) == nullptr);
    }
    {
        const NamedRange outs[] = {{buf + 24, 8, "a"}, {buf + 20, 4, "b"}};                           // b inside in1
        const NamedRange* bad = first_overlap(outs, 2, ins, 3, &with);
        EXPECT(bad == &outs[1] && with == nullptr);
    }
    {
        const NamedRange outs[] = {{buf + 24, 8, "a"}, {buf + 40, 8, "b"}, {buf + 31, 10, "c"}};      // c meets a and b: a is named
        const NamedRange* bad = first_overlap(outs, 3, ins, 3, &with);
        EXPECT(bad == &outs[2] && with == &outs[0]);
    }
    {
        const NamedRange outs[] = {{buf + 24, 8, "a"}, {buf + 15, 20, "b"}};                          // an input goes before an output
        const NamedRange* bad = first_overlap(outs, 2, ins, 3, &with);
        EXPECT(bad == &outs[1] && with == nullptr);
    }
    EXPECT(first_overlap(nullptr, 0, ins, 3, &with) == nullptr);
    free(buf);
    printf(g_failed ? "host_helpers_check: %d check(s) FAILED\n" : "host_helpers_check: all checks passed, no report\n", g_failed);
    return g_failed ? 1 : 0;
}
