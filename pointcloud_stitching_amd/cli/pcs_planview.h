// pcs_planview.h — the -H option of pcs-multicamera-optimized: `-H <prefix>,<up>,<cell_mm>,<W>x<H>[,<u0>,<v0>[,<lo>,<hi>]]`, the
// plan-view maps of the cloud that leaves the filter chain (include/pcs_hip.h: pcs_plan_view_device): the option's words into
// pcs_plan_params, and the three Netpbm files of the last frame-set's maps. Parsed before any context exists, so a malformed option
// costs no device. tools/plan_host.cpp compiles this header for the host alone; tests/test_plan_view_cpu.py holds it to Python.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <ostream>
#include <string>
#include <vector>

#include "../../include/pcs_hip.h"
#include "../csrc/pcs_plan_math.h"

namespace pcs_planview {

inline const char* help()
{
    return " -H <prefix>,<up>,<cell_mm>,<W>x<H>[,<u0>,<v0>[,<lo>,<hi>]]  plan-view maps of the cloud that leaves the chain (behind the last of\n"
           "                  -X -O -K -M -E, ahead of -V; the stitched cloud if none is given): seen along <up> (one of +x -x +y -y +z -z),\n"
           "                  W x H cells of cell_mm (1..32767) millimetres, W and H up to 4096 and W*H up to 4194304; the map axes are the\n"
           "                  two that follow <up> cyclically (up z: u = x, v = y). <u0>,<v0>: the low corner of cell (0, 0) in mm, default\n"
           "                  -(W*cell_mm)/2, -(H*cell_mm)/2: the map centred on 0. <lo>,<hi>: only records whose <up> coordinate lies in\n"
           "                  lo..hi (inclusive) take part, default all. After the last frame-set three files are written: <prefix>.rgb.ppm\n"
           "                  (P6: the colour of each cell's highest record), <prefix>.top.pgm (P5, maxval 65535, big-endian: 0 for an empty\n"
           "                  cell, else its greatest height + 32768 clamped to 1..65535) and <prefix>.count.pgm (P5, maxval 65535: the\n"
           "                  records per cell, saturated). File row r is map row cv = r, column cu: low v at the top, no flip. -t prints\n"
           "                  `Plan view: ...` with the records considered, in the band, on the map, the occupied cells and the fullest;\n"
           "                  drops nothing; give -Z or -B first (zero-depth pixels pile into one cell); not with -G\n";
}

// One integer of the option, the whole token: no sign but a leading '-', no blanks, nothing behind it.
inline bool whole_int(const std::string& t, long& v)
{
    if (t.empty() || t[0] == ' ' || t[0] == '\t' || t[0] == '+') return false;
    char* end = nullptr;
    errno = 0;
    v = strtol(t.c_str(), &end, 10);
    return end != t.c_str() && !*end && !errno;
}

// The option's argument into prefix and params. On failure `why` says what is wrong. The prefix holds no comma.
inline bool parse(const char* arg, std::string& prefix, pcs_plan_params& params, std::string& why)
{
    static const char shape[] = "expected <prefix>,<up>,<cell_mm>,<W>x<H>[,<u0>,<v0>[,<lo>,<hi>]]";
    std::vector<std::string> tok(1);
    for (const char* p = arg ? arg : ""; *p; p++) {
        if (*p == ',') tok.emplace_back();
        else tok.back().push_back(*p);
    }
    if (tok.size() != 4 && tok.size() != 6 && tok.size() != 8) { why = shape; return false; }
    if (tok[0].empty()) { why = std::string(shape) + ": the prefix is empty"; return false; }
    if (tok[0][0] == '-') { why = std::string(shape) + ": the prefix is not another option"; return false; }
    const std::string& up = tok[1];
    if (up.size() != 2 || (up[0] != '+' && up[0] != '-') || up[1] < 'x' || up[1] > 'z') {
        why = "<up> is one of +x -x +y -y +z -z, not '" + up + "'";
        return false;
    }
    long cell = 0, w = 0, h = 0, u0 = 0, v0 = 0, lo = -32768, hi = 32767;
    if (!whole_int(tok[2], cell)) { why = std::string(shape) + ", cell_mm an integer"; return false; }
    const size_t x = tok[3].find('x');
    if (x == std::string::npos || !whole_int(tok[3].substr(0, x), w) || !whole_int(tok[3].substr(x + 1), h)) {
        why = std::string(shape) + ", <W>x<H> two integers";
        return false;
    }
    if (cell < 1 || cell > 32767) { why = "cell_mm " + std::to_string(cell) + " is outside 1..32767"; return false; }
    if (w < 1 || w > PCS_PLAN_SIDE_MAX || h < 1 || h > PCS_PLAN_SIDE_MAX || w * h > PCS_PLAN_CELLS_MAX) {
        why = tok[3] + ": W and H are 1.." + std::to_string(PCS_PLAN_SIDE_MAX) + " each and W*H at most " + std::to_string(PCS_PLAN_CELLS_MAX);
        return false;
    }
    u0 = -((w * cell) / 2);
    v0 = -((h * cell) / 2);
    if (tok.size() >= 6 && (!whole_int(tok[4], u0) || !whole_int(tok[5], v0))) { why = std::string(shape) + ", <u0>,<v0> two integers"; return false; }
    if (u0 < -32768 || u0 > 32767 || v0 < -32768 || v0 > 32767) {
        why = "the origin " + std::to_string(u0) + "," + std::to_string(v0) + " is outside -32768..32767" +
              (tok.size() < 6 ? " (the centred default of a map this large: give <u0>,<v0>)" : "");
        return false;
    }
    if (tok.size() == 8 && (!whole_int(tok[6], lo) || !whole_int(tok[7], hi))) { why = std::string(shape) + ", <lo>,<hi> two integers"; return false; }
    if (lo < -32768 || hi > 32767 || lo > hi) { why = "the band " + std::to_string(lo) + "," + std::to_string(hi) + " is not lo <= hi inside -32768..32767"; return false; }
    pcs_plan_params q{};
    q.up_axis = up[1] - 'x'; q.up_sign = up[0] == '+' ? 1 : -1; q.cell_mm = (int32_t)cell;
    q.origin_u = (int32_t)u0; q.origin_v = (int32_t)v0; q.width = (int32_t)w; q.height = (int32_t)h;
    q.band_lo = (int32_t)lo; q.band_hi = (int32_t)hi;
    if (const int bad = pcs::plan_bad_param(reinterpret_cast<const int32_t*>(&q))) {      // (the library's own ranges: nothing above may be wider)
        why = "parameter word " + std::to_string(bad - 1) + " is out of range";
        return false;
    }
    prefix = tok[0];
    params = q;
    return true;
}

// The three files. Row r of a file is map row cv = r, column cu; no flip.
inline void write_rgb_ppm(std::ostream& os, int w, int h, const uint8_t* rgb)
{
    os << "P6\n" << w << ' ' << h << "\n255\n";
    os.write(reinterpret_cast<const char*>(rgb), (std::streamsize)3 * w * h);
}

inline void put_be16(std::string& row, uint32_t v)
{
    row.push_back((char)(v >> 8));
    row.push_back((char)(v & 0xFFu));
}

// 0 for an empty cell, else clamp(h + 32768, 1, 65535), h = up_sign * top
inline void write_top_pgm(std::ostream& os, const pcs_plan_params& p, const uint32_t* count, const int16_t* top)
{
    os << "P5\n" << p.width << ' ' << p.height << "\n65535\n";
    std::string row;
    for (int r = 0; r < p.height; r++) {
        row.clear();
        for (int c = 0; c < p.width; c++) {
            const size_t i = (size_t)r * p.width + c;
            const int v = p.up_sign * (int)top[i] + 32768;
            put_be16(row, count[i] ? (uint32_t)(v < 1 ? 1 : v > 65535 ? 65535 : v) : 0u);
        }
        os.write(row.data(), (std::streamsize)row.size());
    }
}

inline void write_count_pgm(std::ostream& os, int w, int h, const uint32_t* count)
{
    os << "P5\n" << w << ' ' << h << "\n65535\n";
    std::string row;
    for (int r = 0; r < h; r++) {
        row.clear();
        for (int c = 0; c < w; c++) {
            const uint32_t v = count[(size_t)r * w + c];
            put_be16(row, v > 65535u ? 65535u : v);
        }
        os.write(row.data(), (std::streamsize)row.size());
    }
}

inline void report(std::ostream& os, const pcs_plan_params& p, const pcs_plan_stats& st)
{
    os << "Plan view: " << (long long)st.considered << " considered, " << (long long)st.in_band << " in band, " << (long long)st.mapped
       << " on the map, " << (long long)st.occupied << " occupied of " << p.width << " x " << p.height << " cells, fullest "
       << (long long)st.fullest << std::endl;
}

}  // namespace pcs_planview
