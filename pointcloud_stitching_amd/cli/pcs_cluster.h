// pcs_cluster.h — the -E option of pcs-multicamera-optimized: `-E tolerance_mm,min_size[,max_size]`, two or three integers
// (include/pcs_hip.h: pcs_cluster_filter_device). Parsed before any context exists, so a malformed option costs no device.
#pragma once

#include <cerrno>
#include <climits>
#include <cstdlib>
#include <string>

#include "../../include/pcs_hip.h"

namespace pcs_cluster {

inline const char* help()
{
    return " -E <tolerance_mm,min_size[,max_size]>  Euclidean cluster filter on the stitched cloud: records within tolerance_mm (1..1000) of\n"
           "                  each other are connected; a record stays iff its connected component holds at least min_size records (and at\n"
           "                  most max_size, if given and not 0); after -T, -B / -d, -O and -K, before -V; not with -G\n";
}

// Two or three integers separated by commas, each inside the library's range. On failure `why` says what is wrong.
inline bool parse(const char* arg, pcs_cluster_params& params, std::string& why)
{
    static const char shape[] = "expected two or three integers tolerance_mm,min_size[,max_size]";
    static const char* const names[3] = {"tolerance_mm", "min_size", "max_size"};
    static const long lo[3] = {PCS_CLUSTER_TOLERANCE_MIN, 1, 0}, hi[3] = {PCS_CLUSTER_TOLERANCE_MAX, INT_MAX, INT_MAX};
    long v[3] = {0, 0, 0};
    int got = 0;
    const char* p = arg;
    for (int k = 0; k < 3; k++) {
        if (*p == ' ' || *p == '\t') { why = shape; return false; }         // (strtol would skip it)
        char* end = nullptr;
        errno = 0;
        v[k] = strtol(p, &end, 10);
        if (end == p || errno) { why = shape; return false; }
        p = end;
        got = k + 1;
        if (*p != ',') break;
        if (k == 2) { why = std::string(shape) + ", nothing after them"; return false; }
        p++;
    }
    if (got < 2) { why = shape; return false; }
    if (*p) { why = std::string(shape) + ", nothing after them"; return false; }
    for (int k = 0; k < got; k++)
        if (v[k] < lo[k] || v[k] > hi[k]) {
            why = std::string(names[k]) + " " + std::to_string(v[k]) + " is outside " + std::to_string(lo[k]) + ".." + std::to_string(hi[k]);
            return false;
        }
    if (v[2] != 0 && v[2] < v[1]) {
        why = "max_size " + std::to_string(v[2]) + " is neither 0 nor at least min_size " + std::to_string(v[1]);
        return false;
    }
    params = pcs_cluster_params{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], 0};
    return true;
}

}  // namespace pcs_cluster
