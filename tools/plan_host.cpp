// plan_host.cpp — the plan-view maps on the CPU: the same pcs_plan_math.h that pcs_kernels_plan.hip compiles, fed by a plain loop over
// the records instead of the LDS table and the atomics, and the option parser and Netpbm writers of cli/pcs_planview.h.
// tests/test_plan_view_cpu.py builds it with the host compiler and holds it to tests/np_plan_view.py where no GPU is present; the GPU
// tests hold the library to the same restatement.
//
//     g++ -O2 -std=c++17 -shared -fPIC -I pointcloud_stitching_amd/csrc -I pointcloud_stitching_amd/cli tools/plan_host.cpp -o libplan_host.so
//
// With -DPLAN_HOST_MAIN it is a program of its own (for the host sanitizers): the division sweep, a parse and the three files of a small
// map into the directory given as its argument.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "pcs_planview.h"

namespace {

pcs::PlanArgs args_of(const pcs_plan_params& p)
{
    return pcs::PlanArgs{p.up_axis, p.up_sign, p.cell_mm, pcs::plan_magic(p.cell_mm), p.origin_u, p.origin_v, p.width, p.height, p.band_lo, p.band_hi};
}

}  // namespace

extern "C" {

// 0, or 1 + the index of the first parameter word out of range
int plan_host_bad_param(const pcs_plan_params* p) { return pcs::plan_bad_param(reinterpret_cast<const int32_t*>(p)); }

// per record: in_band (0 / 1), the cell (-1: out of band or off the map) and both keys
void plan_host_records(const int16_t* payload, int n, const pcs_plan_params* p, uint8_t* in_band, int32_t* cell, uint64_t* top_key,
                       uint64_t* bottom_key)
{
    const pcs::PlanArgs P = args_of(*p);
    for (int i = 0; i < n; i++) {
        const int x = payload[5 * i], y = payload[5 * i + 1], z = payload[5 * i + 2];
        const int up = pcs::plan_up(P, x, y, z);
        in_band[i] = pcs::plan_in_band(P, up) ? 1 : 0;
        cell[i] = in_band[i] ? pcs::plan_cell(P, x, y, z) : -1;
        const int hb = pcs::plan_hb(P, up);
        top_key[i] = pcs::plan_top_key(hb, (uint32_t)i);
        bottom_key[i] = pcs::plan_bottom_key(hb, (uint32_t)i);
    }
}

// the whole call behind a plain loop: the rasters (width * height cells) and the eight statistics words
void plan_host_maps(const int16_t* payload, int n, const pcs_plan_params* p, uint32_t* count, int16_t* top, int16_t* bottom, uint8_t* rgb,
                    int64_t* stats)
{
    const pcs::PlanArgs P = args_of(*p);
    const size_t cells = (size_t)P.width * P.height;
    std::vector<unsigned long long> kt(cells, 0ull), kb(cells, 0ull);
    std::memset(count, 0, 4 * cells);
    std::memset(stats, 0, 64);
    stats[0] = n;
    for (int i = 0; i < n; i++) {
        const int x = payload[5 * i], y = payload[5 * i + 1], z = payload[5 * i + 2];
        const int up = pcs::plan_up(P, x, y, z);
        if (!pcs::plan_in_band(P, up)) continue;
        stats[1]++;
        const int c = pcs::plan_cell(P, x, y, z);
        if (c < 0) continue;
        stats[2]++;
        count[c]++;
        const int hb = pcs::plan_hb(P, up);
        const unsigned long long t = pcs::plan_top_key(hb, (uint32_t)i), b = pcs::plan_bottom_key(hb, (uint32_t)i);
        kt[c] = t > kt[c] ? t : kt[c];
        kb[c] = b > kb[c] ? b : kb[c];
    }
    for (size_t c = 0; c < cells; c++) {
        top[c] = bottom[c] = 0;
        rgb[3 * c] = rgb[3 * c + 1] = rgb[3 * c + 2] = 0;
        if (!count[c]) continue;
        stats[3]++;
        stats[4] = count[c] > stats[4] ? count[c] : stats[4];
        top[c] = (int16_t)pcs::plan_top_raw(P, kt[c]);
        bottom[c] = (int16_t)pcs::plan_bottom_raw(P, kb[c]);
        const uint16_t* rec = reinterpret_cast<const uint16_t*>(payload) + (size_t)pcs::plan_key_index(kt[c]) * 5;
        rgb[3 * c] = (uint8_t)(rec[3] & 0xFFu);
        rgb[3 * c + 1] = (uint8_t)(rec[3] >> 8);
        rgb[3 * c + 2] = (uint8_t)(rec[4] & 0xFFu);
    }
}

// plan_div against the quotient counted up, for every numerator 0..65535 and every cell edge c_lo..c_hi: the mismatches (0 wanted)
long long plan_host_sweep(int c_lo, int c_hi)
{
    long long bad = 0;
    for (int c = c_lo; c <= c_hi; c++) {
        const uint32_t m = pcs::plan_magic(c);
        uint32_t q = 0, r = 0;                               // d = q c + r, 0 <= r < c, without a division
        for (uint32_t d = 0; d < 65536u; d++) {
            bad += pcs::plan_div(d, c, m) != q;
            if (++r == (uint32_t)c) { r = 0; q++; }
        }
    }
    return bad;
}

// cli/pcs_planview.h's parse: 1 and the prefix / params, or 0 and why
int plan_host_parse(const char* arg, char* prefix, int prefix_cap, pcs_plan_params* params, char* why, int why_cap)
{
    std::string pre, w;
    pcs_plan_params p{};
    const bool ok = pcs_planview::parse(arg, pre, p, w);
    std::snprintf(prefix, (size_t)prefix_cap, "%s", pre.c_str());
    std::snprintf(why, (size_t)why_cap, "%s", w.c_str());
    if (ok) *params = p;
    return ok ? 1 : 0;
}

// the three files of a map as the program writes them: 0, or the number of files that could not be written
int plan_host_write(const char* prefix, const pcs_plan_params* p, const uint32_t* count, const int16_t* top, const uint8_t* rgb)
{
    int bad = 0;
    {
        std::ofstream f(std::string(prefix) + ".rgb.ppm", std::ios::binary);
        pcs_planview::write_rgb_ppm(f, p->width, p->height, rgb);
        f.flush();
        bad += !f.good();
    }
    {
        std::ofstream f(std::string(prefix) + ".top.pgm", std::ios::binary);
        pcs_planview::write_top_pgm(f, *p, count, top);
        f.flush();
        bad += !f.good();
    }
    {
        std::ofstream f(std::string(prefix) + ".count.pgm", std::ios::binary);
        pcs_planview::write_count_pgm(f, p->width, p->height, count);
        f.flush();
        bad += !f.good();
    }
    return bad;
}

}  // extern "C"

#ifdef PLAN_HOST_MAIN
int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const long long bad = plan_host_sweep(1, 32767);
    std::printf("division sweep: %lld mismatches\n", bad);
    char prefix[256], why[256];
    pcs_plan_params p{};
    const std::string arg = dir + "/map,-y,25,7x5,-80,-60,-100,900";
    if (!plan_host_parse(arg.c_str(), prefix, sizeof prefix, &p, why, sizeof why)) { std::printf("parse: %s\n", why); return 1; }
    const char* refused[] = {"", "m", "m,+z,10", "m,+z,10,4x", "m,z,10,4x4", "m,+z,0,4x4", "m,+z,10,4097x1", "m,+z,10,4x4,1", "m,+z,10,4x4,1,2,3",
                             "m,+z,10,4x4,1,2,5,4", "m,+z,10,4x4,70000,0", "-m,+z,10,4x4", "m,+z,10,4x4,1,2,3,4,5", "m,+z, 10,4x4"};
    for (const char* r : refused)
        if (plan_host_parse(r, prefix, sizeof prefix, &p, why, sizeof why)) { std::printf("accepted: %s\n", r); return 1; }
    if (!plan_host_parse(arg.c_str(), prefix, sizeof prefix, &p, why, sizeof why)) return 1;
    std::vector<int16_t> rec;
    for (int i = 0; i < 500; i++) {
        const int16_t r[5] = {(int16_t)(i * 37 % 200 - 100), (int16_t)(i * 53 % 1200 - 200), (int16_t)(i * 11 % 150 - 70), (int16_t)(i * 259), (int16_t)(i & 0xFF)};
        rec.insert(rec.end(), r, r + 5);
    }
    const size_t cells = (size_t)p.width * p.height;
    std::vector<uint32_t> count(cells);
    std::vector<int16_t> top(cells), bottom(cells);
    std::vector<uint8_t> rgb(3 * cells);
    int64_t stats[8];
    plan_host_maps(rec.data(), 500, &p, count.data(), top.data(), bottom.data(), rgb.data(), stats);
    std::printf("map: %lld in band, %lld on the map, %lld occupied, fullest %lld\n", (long long)stats[1], (long long)stats[2], (long long)stats[3],
                (long long)stats[4]);
    const int unwritten = plan_host_write(prefix, &p, count.data(), top.data(), rgb.data());
    return bad || unwritten ? 1 : 0;
}
#endif
