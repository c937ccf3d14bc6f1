// pcs_outlier.h — the -O option of pcs-multicamera-optimized: `-O radius_mm,min_neighbors`, two integers (include/pcs_hip.h:
// pcs_radius_outlier_device). Parsed before any context exists, so a malformed option costs no device.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <string>

#include "../../include/pcs_hip.h"

namespace pcs_outlier {

inline const char* help()
{
    return " -O <radius_mm,min_neighbors>  radius outlier removal on the stitched cloud: a record stays iff at least min_neighbors\n"
           "                  others lie within radius_mm (1..1000, 1..255); after -T and -B / -d, before -V; not with -G\n";
}

// Exactly two integers separated by a comma, each inside the library's range. On failure `why` says what is wrong.
inline bool parse(const char* arg, int& radius_mm, int& min_neighbors, std::string& why)
{
    static const char shape[] = "expected two integers radius_mm,min_neighbors";
    long v[2];
    const char* p = arg;
    for (int k = 0; k < 2; k++) {
        char* end = nullptr;
        errno = 0;
        v[k] = strtol(p, &end, 10);
        if (end == p || errno) { why = shape; return false; }
        p = end;
        if (k == 0) {
            if (*p != ',') { why = shape; return false; }
            p++;
        }
    }
    if (*p) { why = std::string(shape) + ", nothing after them"; return false; }
    if (v[0] < PCS_OUTLIER_RADIUS_MIN || v[0] > PCS_OUTLIER_RADIUS_MAX) {
        why = "radius_mm " + std::to_string(v[0]) + " is outside " + std::to_string(PCS_OUTLIER_RADIUS_MIN) + ".." + std::to_string(PCS_OUTLIER_RADIUS_MAX);
        return false;
    }
    if (v[1] < PCS_OUTLIER_NEIGHBORS_MIN || v[1] > PCS_OUTLIER_NEIGHBORS_MAX) {
        why = "min_neighbors " + std::to_string(v[1]) + " is outside " + std::to_string(PCS_OUTLIER_NEIGHBORS_MIN) + ".." + std::to_string(PCS_OUTLIER_NEIGHBORS_MAX);
        return false;
    }
    radius_mm = (int)v[0]; min_neighbors = (int)v[1];
    return true;
}

}  // namespace pcs_outlier
