// pcs_spatialfilter.h — the -S option of pcs-camera-optimized: `-S <alpha:delta:iterations[:radius] | default>`, the spatial filter's
// parameters (include/pcs_hip.h: pcs_spatial_filter_depth). Parsed before any context exists, so a malformed spec costs no device.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pcs_hip.h"

namespace pcs_spatialfilter {

// `default` (0.5:20:2, no hole fill) or alpha:delta:iterations[:radius]: alpha in (0,1], delta 1..65535 (Z16 units), iterations 1..5,
// radius 0..65535 (pixels filled per gap and direction in the row passes; 0 or absent: none). On failure `why` says what is wrong.
inline bool parse(const char* arg, pcs_spatial_filter_config& cfg, std::string& why)
{
    cfg.alpha = 0.5f; cfg.delta = 20; cfg.iterations = 2; cfg.hole_radius = 0;
    const char* p = arg ? arg : "";
    if (strcmp(p, "default") == 0) return true;
    const char* shape = "expected alpha:delta:iterations[:radius] or default, e.g. 0.5:20:2";
    char* end = nullptr;
    errno = 0;
    const float alpha = strtof(p, &end);
    if (end == p || errno || *end != ':') { why = shape; return false; }
    long v[3] = {0, 0, 0};
    int got = 0;
    while (got < 3 && *end == ':') {
        p = end + 1;
        errno = 0;
        v[got] = strtol(p, &end, 10);
        if (end == p || errno) { why = shape; return false; }
        got++;
    }
    if (got < 2 || *end != '\0') { why = shape; return false; }
    if (!(alpha > 0.0f && alpha <= 1.0f)) { why = "alpha must lie in (0, 1]"; return false; }      // (refuses NaN too)
    if (v[0] < 1 || v[0] > 65535) { why = "delta must lie in 1..65535 (Z16 units)"; return false; }
    if (v[1] < 1 || v[1] > 5) { why = "iterations must lie in 1..5"; return false; }
    if (v[2] < 0 || v[2] > 65535) { why = "radius must lie in 0..65535 (pixels)"; return false; }
    cfg.alpha = alpha; cfg.delta = (int32_t)v[0]; cfg.iterations = (int32_t)v[1]; cfg.hole_radius = (int32_t)v[2];
    return true;
}

}  // namespace pcs_spatialfilter
