// pcs_statoutlier.h — the -K option of pcs-multicamera-optimized: `-K mean_k,std_mul_milli,max_dist_mm`, three integers
// (include/pcs_hip.h: pcs_stat_outlier_device). Parsed before any context exists, so a malformed option costs no device.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <string>

#include "../../include/pcs_hip.h"

namespace pcs_statoutlier {

inline const char* help()
{
    return " -K <mean_k,std_mul_milli,max_dist_mm>  statistical outlier removal on the stitched cloud: a record stays iff it has mean_k\n"
           "                  others within max_dist_mm (1..64, 1..1000) and its summed distance to the nearest mean_k is at most the\n"
           "                  cloud's mean + std_mul_milli / 1000 (0..10000) deviations; after -T, -B / -d and -O, before -V; not with -G\n";
}

// Exactly three integers separated by commas, each inside the library's range. On failure `why` says what is wrong.
inline bool parse(const char* arg, pcs_stat_outlier_params& params, std::string& why)
{
    static const char shape[] = "expected three integers mean_k,std_mul_milli,max_dist_mm";
    static const char* const names[3] = {"mean_k", "std_mul_milli", "max_dist_mm"};
    static const long lo[3] = {PCS_STAT_K_MIN, 0, PCS_STAT_DIST_MIN}, hi[3] = {PCS_STAT_K_MAX, PCS_STAT_MUL_MILLI_MAX, PCS_STAT_DIST_MAX};
    long v[3];
    const char* p = arg;
    for (int k = 0; k < 3; k++) {
        if (*p == ' ' || *p == '\t') { why = shape; return false; }         // (strtol would skip it)
        char* end = nullptr;
        errno = 0;
        v[k] = strtol(p, &end, 10);
        if (end == p || errno) { why = shape; return false; }
        p = end;
        if (k < 2) {
            if (*p != ',') { why = shape; return false; }
            p++;
        }
    }
    if (*p) { why = std::string(shape) + ", nothing after them"; return false; }
    for (int k = 0; k < 3; k++)
        if (v[k] < lo[k] || v[k] > hi[k]) {
            why = std::string(names[k]) + " " + std::to_string(v[k]) + " is outside " + std::to_string(lo[k]) + ".." + std::to_string(hi[k]);
            return false;
        }
    params = pcs_stat_outlier_params{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], 0};
    return true;
}

}  // namespace pcs_statoutlier
