// pcs_objects.h — the -L option of pcs-multicamera-optimized: `-L <file>[,<max_objects>]`, the object table of the -E stage
// (include/pcs_hip.h: pcs_cluster_objects_device): where it goes, how many entries it holds, and the file's lines. Parsed before any
// context exists, so a malformed option costs no device.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <ostream>
#include <string>

#include "../../include/pcs_hip.h"

namespace pcs_objects {

constexpr int kDefaultMaxObjects = 1024;

inline const char* help()
{
    return " -L <file>[,<max_objects>]  with -E: the clusters that stay, as objects: after the last frame-set <file> (- for stdout) gets one\n"
           "                  header line and one line per object of that frame-set, by first record: label, size, bounding box and the\n"
           "                  integer sums of coordinates and colours, at most max_objects (1..65536, default 1024) of them; -t prints\n"
           "                  `Objects: <n> (<written> written)`; not with -G\n";
}

// <file> or <file>,<max_objects>: the part behind the LAST comma is the count if there is a comma. On failure `why` says what is wrong.
inline bool parse(const char* arg, std::string& file, int& max_objects, std::string& why)
{
    static const char shape[] = "expected <file>[,<max_objects>]";
    const char* comma = strrchr(arg, ',');
    long v = kDefaultMaxObjects;
    if (comma) {
        const char* p = comma + 1;
        if (*p == ' ' || *p == '\t' || *p == '+') { why = std::string(shape) + ", max_objects an integer"; return false; }
        char* end = nullptr;
        errno = 0;
        v = strtol(p, &end, 10);
        if (end == p || errno) { why = std::string(shape) + ", max_objects an integer"; return false; }
        if (*end) { why = std::string(shape) + ", nothing after them"; return false; }
        if (v < 1 || v > PCS_CLUSTER_OBJECTS_MAX) {
            why = "max_objects " + std::to_string(v) + " is outside 1.." + std::to_string(PCS_CLUSTER_OBJECTS_MAX);
            return false;
        }
    }
    file.assign(arg, comma ? (size_t)(comma - arg) : strlen(arg));
    if (file.empty()) { why = std::string(shape) + ": the file name is empty"; return false; }
    max_objects = (int)v;
    return true;
}

// The file: raw integers separated by one space, nothing derived.
inline void write(std::ostream& os, const pcs_cluster_object* objects, int written)
{
    os << "# k label size lo_x lo_y lo_z hi_x hi_y hi_z sum_x sum_y sum_z sum_r sum_g sum_b\n";
    for (int k = 0; k < written; k++) {
        const pcs_cluster_object& o = objects[k];
        os << k << ' ' << o.label << ' ' << o.size;
        for (int a = 0; a < 3; a++) os << ' ' << o.lo[a];
        for (int a = 0; a < 3; a++) os << ' ' << o.hi[a];
        for (int a = 0; a < 3; a++) os << ' ' << (long long)o.sum_xyz[a];
        for (int a = 0; a < 3; a++) os << ' ' << (long long)o.sum_rgb[a];
        os << '\n';
    }
}

}  // namespace pcs_objects
