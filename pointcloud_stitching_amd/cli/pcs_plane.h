// pcs_plane.h — the -M option of pcs-multicamera-optimized: `-M distance_mm,iterations[,min_inliers[,max_planes[,seed]]]`, two to five
// integers (include/pcs_hip.h: pcs_plane_segment_device). Parsed before any context exists, so a malformed option costs no device.
#pragma once

#include <cerrno>
#include <climits>
#include <cstdlib>
#include <string>

#include "../../include/pcs_hip.h"

namespace pcs_plane {

inline const char* help()
{
    return " -M <distance_mm,iterations[,min_inliers[,max_planes[,seed]]]>  plane segmentation on the stitched cloud: up to max_planes (1..8,\n"
           "                  default 1) times the plane through three drawn records that has the most records within distance_mm (1..1000)\n"
           "                  out of `iterations` (1..4096) such planes is taken out of the cloud, while it has min_inliers (>= 3, default 3)\n"
           "                  records; seed (default 1) seeds the draws; after -T, -B / -d, -O and -K, before -E and -V; not with -G\n";
}

// Two to five integers separated by commas, each inside the library's range. On failure `why` says what is wrong.
inline bool parse(const char* arg, pcs_plane_params& params, std::string& why)
{
    static const char shape[] = "expected two to five integers distance_mm,iterations[,min_inliers[,max_planes[,seed]]]";
    static const char* const names[5] = {"distance_mm", "iterations", "min_inliers", "max_planes", "seed"};
    static const long long lo[5] = {PCS_PLANE_DISTANCE_MIN, 1, 3, 1, 0};
    static const long long hi[5] = {PCS_PLANE_DISTANCE_MAX, PCS_PLANE_ITERATIONS_MAX, INT_MAX, PCS_PLANE_MAX_PLANES, 4294967295ll};
    long long v[5] = {0, 0, 3, 1, 1};
    int got = 0;
    const char* p = arg;
    for (int k = 0; k < 5; k++) {
        if (*p == ' ' || *p == '\t' || *p == '+') { why = shape; return false; }         // (strtoll would skip or accept it)
        char* end = nullptr;
        errno = 0;
        v[k] = strtoll(p, &end, 10);
        if (end == p || errno) { why = shape; return false; }
        p = end;
        got = k + 1;
        if (*p != ',') break;
        if (k == 4) { why = std::string(shape) + ", nothing after them"; return false; }
        p++;
    }
    if (got < 2) { why = shape; return false; }
    if (*p) { why = std::string(shape) + ", nothing after them"; return false; }
    for (int k = 0; k < got; k++)
        if (v[k] < lo[k] || v[k] > hi[k]) {
            why = std::string(names[k]) + " " + std::to_string(v[k]) + " is outside " + std::to_string(lo[k]) + ".." + std::to_string(hi[k]);
            return false;
        }
    params = pcs_plane_params{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (uint32_t)v[4], PCS_PLANE_MODE_REMOVE, {0, 0}};
    return true;
}

}  // namespace pcs_plane
