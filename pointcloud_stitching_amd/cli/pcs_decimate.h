// pcs_decimate.h — the -D option of pcs-camera-optimized: `-D <n>`, the depth decimation's scale (include/pcs_hip.h:
// pcs_decimate_depth). Parsed before any context exists, so a malformed value costs no device.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <string>

namespace pcs_decimate {

// A whole number 1..8; 1 is off. On failure `why` says what is wrong.
inline bool parse(const char* arg, int& scale, std::string& why)
{
    const char* p = arg ? arg : "";
    char* end = nullptr;
    errno = 0;
    const long v = strtol(p, &end, 10);
    if (end == p || *end != '\0' || errno) { why = "expected a whole number 1..8 (1 = off)"; return false; }
    if (v < 1 || v > 8) { why = "the scale must lie in 1..8 (1 = off)"; return false; }
    scale = (int)v;
    return true;
}

}  // namespace pcs_decimate
