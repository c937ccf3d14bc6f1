// background_validate_fuzz.cpp — the PCB1 validator (csrc/pcs_background_format.h) under the host sanitizers. A stand-alone program:
// no GPU, no library, nothing loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I pointcloud_stitching_amd/csrc
//       tools/background_validate_fuzz.cpp -o tools/bin/background_validate_fuzz_san && tools/bin/background_validate_fuzz_san [seed] [mutations]
//   (make -C pointcloud_stitching_amd/csrc background-fuzz builds and runs it; ../../tools/bin/background_validate_fuzz is the plain build)
//
// It writes containers with a small writer of its own, checks that the validator accepts them, applies each
// malformed class — every header field, a truncation, a trailing byte, two swapped entries, a repeated key, padding, seen 0 and
// seen > frames — and then seeded random byte, bit and length mutations. Every candidate is validated in a heap allocation of EXACTLY
// its size, so a read outside the buffer is an AddressSanitizer report; a candidate the validator accepts is walked as an importer
// would walk it (every entry inside the buffer, keys ascending, seen in 1..frames), by code that trusts nothing but the verdict.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pcs_background_format.h"

namespace {

namespace F = pcs_background_format;

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

void put16(std::vector<uint8_t>& v, size_t off, uint32_t x) { v[off] = (uint8_t)x; v[off + 1] = (uint8_t)(x >> 8); }
void put32(std::vector<uint8_t>& v, size_t off, uint32_t x) { for (int i = 0; i < 4; i++) v[off + i] = (uint8_t)(x >> (8 * i)); }

// `cells` entries with ascending keys (random gaps), seen in 1..frames
std::vector<uint8_t> container(Rng& rng, uint32_t cells, int32_t cell_mm, uint32_t frames)
{
    std::vector<uint8_t> out(32 + 12 * (size_t)cells, 0);
    memcpy(out.data(), "PCB1", 4);
    put32(out, 4, 1); put32(out, 8, (uint32_t)cell_mm); put32(out, 12, frames); put32(out, 16, cells);
    uint64_t key = rng.below(1000);
    for (uint32_t e = 0; e < cells; e++) {
        const size_t at = 32 + 12 * (size_t)e;
        put16(out, at, (uint32_t)(key & 0xFFFF)); put16(out, at + 2, (uint32_t)(key >> 16 & 0xFFFF)); put16(out, at + 4, (uint32_t)(key >> 32 & 0xFFFF));
        put32(out, at + 8, 1 + rng.below(frames));
        key += 1 + ((uint64_t)rng.next() << (rng.below(3) * 8)) % ((1ull << 47) / (cells + 1));
    }
    return out;
}

int failures = 0;
long accepted = 0, refused = 0;

// The verdict on a candidate, in an allocation of exactly its size; an accepted one is walked inside that allocation.
bool judge(const std::vector<uint8_t>& cand, char* why, size_t why_len)
{
    std::unique_ptr<uint8_t[]> exact(new uint8_t[cand.size() ? cand.size() : 1]);
    if (!cand.empty()) memcpy(exact.get(), cand.data(), cand.size());
    F::Info info;
    if (!F::validate(cand.empty() ? nullptr : exact.get(), cand.size(), &info, why, why_len)) { refused++; return false; }
    accepted++;
    const uint8_t* p = exact.get();
    const size_t n = cand.size();
    bool ok = n == 32 + 12 * (size_t)info.cells && info.cell_mm >= 1 && info.cell_mm <= 1000 && info.frames <= 65535;
    uint64_t prev = 0;
    for (uint32_t e = 0; ok && e < info.cells; e++) {
        const size_t at = 32 + 12 * (size_t)e;
        if (at + 12 > n) { ok = false; break; }
        const uint64_t key = (uint64_t)p[at] | (uint64_t)p[at + 1] << 8 | (uint64_t)p[at + 2] << 16 | (uint64_t)p[at + 3] << 24 |
                             (uint64_t)p[at + 4] << 32 | (uint64_t)p[at + 5] << 40;
        const uint32_t seen = F::load32(p + at + 8);
        ok = ok && !(p[at + 6] | p[at + 7]) && seen >= 1 && seen <= info.frames && (e == 0 || key > prev);
        prev = key;
    }
    if (!ok) { failures++; fprintf(stderr, "FAIL: the validator accepted a container an importer cannot trust (%zu bytes)\n", n); }
    return true;
}

void must(bool accept, const std::vector<uint8_t>& cand, const char* what, const char* word = nullptr)
{
    char why[256] = "";
    const bool got = judge(cand, why, sizeof why);
    if (got != accept || (word && !strstr(why, word))) {
        failures++;
        fprintf(stderr, "FAIL: %s: %s (\"%s\")\n", what, got ? "accepted" : "refused", why);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    Rng rng{argc > 1 ? strtoull(argv[1], nullptr, 0) : 1};
    const long mutations = argc > 2 ? atol(argv[2]) : 20000;
    std::vector<std::vector<uint8_t>> valid;
    for (uint32_t cells : {0u, 1u, 2u, 7u, 64u, 1000u}) valid.push_back(container(rng, cells, 1 + (int32_t)rng.below(1000), 1 + rng.below(65535)));
    valid.push_back(container(rng, 0, 40, 0));
    valid.push_back(container(rng, 5, 1000, 65535));
    for (const auto& v : valid) must(true, v, "a valid container");

    const auto& base = valid[3];                    // 7 cells
    auto with32 = [&](size_t off, uint32_t x) { auto m = base; put32(m, off, x); return m; };
    must(false, with32(0, 0x31424351u), "bad magic", "magic");
    must(false, with32(4, 2), "bad version", "version");
    must(false, with32(8, 0), "cell_mm 0", "cell_mm");
    must(false, with32(8, 1001), "cell_mm 1001", "cell_mm");
    must(false, with32(8, 0xFFFFFFFFu), "cell_mm -1", "cell_mm");
    must(false, with32(12, 65536), "frames above the cap", "frames");
    must(false, with32(16, 6), "cells too small for the length", "bytes");
    must(false, with32(16, 8), "cells too large for the length", "bytes");
    must(false, with32(16, 0xFFFFFFFFu), "cells 2^32 - 1", "bytes");
    for (size_t k = 20; k < 32; k++) { auto m = base; m[k] = 1; must(false, m, "header padding", "header byte"); }
    { auto m = base; m.pop_back(); must(false, m, "a truncation", "bytes"); }
    { auto m = base; m.resize(31); must(false, m, "a truncated header", "header"); }
    { auto m = base; m.push_back(0); must(false, m, "a trailing byte", "bytes"); }
    must(false, {}, "no bytes at all");
    { auto m = base; for (int k = 0; k < 12; k++) std::swap(m[32 + 12 * 2 + k], m[32 + 12 * 3 + k]); must(false, m, "two swapped entries", "ascend"); }
    { auto m = base; memcpy(&m[32 + 12 * 4], &m[32 + 12 * 3], 8); must(false, m, "a repeated key", "ascend"); }
    { auto m = base; m[32 + 12 * 5 + 6] = 1; must(false, m, "entry padding", "padding"); }
    { auto m = base; put32(m, 32 + 12 * 1 + 8, 0); must(false, m, "seen 0", "seen"); }
    { auto m = base; put32(m, 32 + 12 * 6 + 8, F::load32(&m[12]) + 1); must(false, m, "seen above frames", "seen"); }

    for (long i = 0; i < mutations; i++) {
        auto m = valid[rng.below((uint32_t)valid.size())];
        const uint32_t kind = rng.below(6), edits = 1 + rng.below(3);
        for (uint32_t e = 0; e < edits && !m.empty(); e++) {
            const uint32_t at = rng.below(4) ? rng.below((uint32_t)m.size()) : rng.below(32);     // the header more often than its share
            switch (kind) {
            case 0: m[at] = (uint8_t)rng.next(); break;
            case 1: m[at] ^= (uint8_t)(1u << rng.below(8)); break;
            case 2: m.resize(rng.below((uint32_t)m.size() + 1)); break;
            case 3: m.resize(m.size() + 1 + rng.below(24), (uint8_t)rng.next()); break;
            case 4: if (m.size() >= 20) put32(m, 16, rng.below(2) ? rng.next() : (uint32_t)((m.size() - 32) / 12 + rng.below(3) - 1)); break;
            default: if (m.size() >= 32 + 24) { const size_t a = 32 + 12 * rng.below((uint32_t)((m.size() - 32) / 12)), b = 32 + 12 * rng.below((uint32_t)((m.size() - 32) / 12));
                                                for (int k = 0; k < 12; k++) std::swap(m[a + k], m[b + k]); } break;
            }
        }
        char why[256];
        judge(m, why, sizeof why);
    }
    printf("background_validate_fuzz: %ld accepted, %ld refused, %d failures\n", accepted, refused, failures);
    return failures ? 1 : 0;
}
