// pcs_cropbox.h — the -B option of both CLIs: `-B xlo,xhi,ylo,yhi,zlo,zhi`, six integers in millimetres, world frame, inclusive
// (include/pcs_hip.h: pcs_set_crop_box_mm). Parsed before any context exists, so a malformed box costs no device.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace pcs_cropbox {

// Exactly six integers separated by commas, each inside int16, lo <= hi per axis. On failure `why` says what is wrong.
inline bool parse(const char* arg, int16_t lo[3], int16_t hi[3], std::string& why)
{
    long v[6];
    const char* p = arg;
    for (int k = 0; k < 6; k++) {
        char* end = nullptr;
        errno = 0;
        v[k] = strtol(p, &end, 10);
        if (end == p || errno) { why = "expected six integers xlo,xhi,ylo,yhi,zlo,zhi (millimetres)"; return false; }
        if (v[k] < -32768 || v[k] > 32767) { why = "value " + std::to_string(v[k]) + " is outside int16 millimetres (-32768..32767)"; return false; }
        p = end;
        if (k < 5) {
            if (*p != ',') { why = "expected six integers xlo,xhi,ylo,yhi,zlo,zhi (millimetres)"; return false; }
            p++;
        }
    }
    if (*p) { why = "expected six integers xlo,xhi,ylo,yhi,zlo,zhi (millimetres), nothing after them"; return false; }
    for (int a = 0; a < 3; a++) {
        if (v[2 * a] > v[2 * a + 1]) { why = std::string("lower bound above upper bound on axis ") + "xyz"[a]; return false; }
        lo[a] = (int16_t)v[2 * a]; hi[a] = (int16_t)v[2 * a + 1];
    }
    return true;
}

}  // namespace pcs_cropbox
