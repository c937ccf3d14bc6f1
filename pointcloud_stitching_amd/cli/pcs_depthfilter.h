// pcs_depthfilter.h — the -F option of pcs-camera-optimized: `-F temporal[=alpha:delta:persistence],holes[=left]`, the depth
// pre-filter's stages (include/pcs_hip.h: pcs_set_depth_filter). Parsed before any context exists, so a malformed spec costs no device.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pcs_hip.h"

namespace pcs_depthfilter {

// A comma list of `temporal`, `temporal=<alpha>:<delta>:<persistence>`, `holes`, `holes=left`; each stage at most once, at least one.
// alpha in (0,1], delta 1..65535, persistence 0..8; without values librealsense's defaults 0.4:20:3. On failure `why` says what is wrong.
inline bool parse(const char* arg, pcs_depth_filter_config& cfg, std::string& why)
{
    cfg.temporal = 0; cfg.alpha = 0.4f; cfg.delta = 20; cfg.persistence = 3; cfg.hole_fill = 0;
    const std::string spec(arg ? arg : "");
    if (spec.empty()) { why = "expected temporal[=alpha:delta:persistence] and / or holes[=left], separated by a comma"; return false; }
    size_t pos = 0;
    while (pos <= spec.size()) {
        const size_t comma = std::min(spec.find(',', pos), spec.size());
        const std::string item = spec.substr(pos, comma - pos);
        pos = comma + 1;
        const size_t eq = item.find('=');
        const std::string name = item.substr(0, eq), val = eq == std::string::npos ? "" : item.substr(eq + 1);
        if (name == "temporal") {
            if (cfg.temporal) { why = "temporal given twice"; return false; }
            cfg.temporal = 1;
            if (eq == std::string::npos) continue;
            const char* p = val.c_str();
            char* end = nullptr;
            errno = 0;
            const float alpha = strtof(p, &end);
            if (end == p || errno || *end != ':') { why = "temporal wants alpha:delta:persistence, e.g. temporal=0.4:20:3"; return false; }
            if (!(alpha > 0.0f && alpha <= 1.0f)) { why = "alpha must lie in (0, 1]"; return false; }      // (refuses NaN too)
            long v[2];
            for (int k = 0; k < 2; k++) {
                p = end + 1;
                errno = 0;
                v[k] = strtol(p, &end, 10);
                if (end == p || errno || *end != (k == 0 ? ':' : '\0')) { why = "temporal wants alpha:delta:persistence, e.g. temporal=0.4:20:3"; return false; }
            }
            if (v[0] < 1 || v[0] > 65535) { why = "delta must lie in 1..65535 (Z16 units)"; return false; }
            if (v[1] < 0 || v[1] > 8) { why = "persistence must lie in 0..8"; return false; }
            cfg.alpha = alpha; cfg.delta = (int32_t)v[0]; cfg.persistence = (int32_t)v[1];
        } else if (name == "holes") {
            if (cfg.hole_fill) { why = "holes given twice"; return false; }
            if (eq != std::string::npos && val != "left") { why = "holes=" + val + ": only fill from left is built (holes or holes=left)"; return false; }
            cfg.hole_fill = 1;
        } else {
            why = "unknown stage '" + item + "': expected temporal[=alpha:delta:persistence] and / or holes[=left]";
            return false;
        }
    }
    return true;
}

}  // namespace pcs_depthfilter
