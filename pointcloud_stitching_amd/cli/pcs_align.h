// pcs_align.h — the command line of pcs-align-extrinsics (include/pcs_hip.h: pcs_align_payloads_device, pcs_align_payloads_plane_device):
//     pcs-align-extrinsics -T in.txt -o out.txt [-A max_dist_mm,iterations[,stride]] [-p radius_mm,min_neighbors[,flatness]] [-R ref]
//                          [-g gpu] [-t] cam0.bin cam1.bin ...
// Parsed before any context exists, so a malformed option costs no device.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <string>
#include <vector>

#include <getopt.h>

#include "../../include/pcs_hip.h"

namespace pcs_align {

struct Options {
    const char*              in_path = nullptr;      // -T: one line of 16 values per camera
    const char*              out_path = nullptr;     // -o: the same format
    int                      max_dist_mm = 60, iterations = 30, stride = 1;      // -A
    bool                     plane = false;          // -p: point to plane, against normals of the target estimated with ...
    int                      normal_radius_mm = 0, normal_min_neighbors = 0, normal_flatness = 0;
    int                      ref = 0;                // -R: the camera every other one is moved onto
    int                      gpu = 0;                // -g
    bool                     timing = false;         // -t
    std::vector<const char*> cams;                   // [int32 bytes][records] files, one per camera
};

// -A: two or three integers separated by commas, each inside the library's range. On failure `why` says what is wrong.
inline bool parse_a(const char* arg, int& max_dist_mm, int& iterations, int& stride, std::string& why)
{
    static const char shape[] = "expected integers max_dist_mm,iterations[,stride]";
    long v[3] = {0, 0, 1};
    const char* p = arg;
    int got = 0;
    for (int k = 0; k < 3; k++) {
        char* end = nullptr;
        errno = 0;
        v[k] = strtol(p, &end, 10);
        if (end == p || errno) { why = shape; return false; }
        p = end;
        got++;
        if (*p != ',') break;
        p++;
        if (k == 2) { why = std::string(shape) + ", nothing after them"; return false; }
    }
    if (*p || got < 2) { why = *p ? std::string(shape) + ", nothing after them" : shape; return false; }
    if (v[0] < PCS_ALIGN_DIST_MIN || v[0] > PCS_ALIGN_DIST_MAX) {
        why = "max_dist_mm " + std::to_string(v[0]) + " is outside " + std::to_string(PCS_ALIGN_DIST_MIN) + ".." + std::to_string(PCS_ALIGN_DIST_MAX);
        return false;
    }
    if (v[1] < 1 || v[1] > PCS_ALIGN_ITERATIONS_MAX) {
        why = "iterations " + std::to_string(v[1]) + " is outside 1.." + std::to_string(PCS_ALIGN_ITERATIONS_MAX);
        return false;
    }
    if (v[2] < 1 || v[2] > 1000000) { why = "stride " + std::to_string(v[2]) + " is outside 1..1000000"; return false; }
    max_dist_mm = (int)v[0]; iterations = (int)v[1]; stride = (int)v[2];
    return true;
}

// -p: two or three integers separated by commas, each inside pcs_normal_params' range. On failure `why` says what is wrong.
inline bool parse_p(const char* arg, int& radius_mm, int& min_neighbors, int& flatness, std::string& why)
{
    static const char shape[] = "expected integers radius_mm,min_neighbors[,flatness]";
    long v[3] = {0, 0, 0};
    const char* p = arg;
    int got = 0;
    for (int k = 0; k < 3; k++) {
        char* end = nullptr;
        errno = 0;
        v[k] = strtol(p, &end, 10);
        if (end == p || errno) { why = shape; return false; }
        p = end;
        got++;
        if (*p != ',') break;
        p++;
        if (k == 2) { why = std::string(shape) + ", nothing after them"; return false; }
    }
    if (*p || got < 2) { why = *p ? std::string(shape) + ", nothing after them" : shape; return false; }
    if (v[0] < PCS_NORMAL_RADIUS_MIN || v[0] > PCS_NORMAL_RADIUS_MAX) {
        why = "radius_mm " + std::to_string(v[0]) + " is outside " + std::to_string(PCS_NORMAL_RADIUS_MIN) + ".." + std::to_string(PCS_NORMAL_RADIUS_MAX);
        return false;
    }
    if (v[1] < PCS_NORMAL_NEIGHBORS_MIN || v[1] > PCS_NORMAL_NEIGHBORS_MAX) {
        why = "min_neighbors " + std::to_string(v[1]) + " is outside " + std::to_string(PCS_NORMAL_NEIGHBORS_MIN) + ".." +
              std::to_string(PCS_NORMAL_NEIGHBORS_MAX);
        return false;
    }
    if (v[2] < 0 || v[2] > PCS_NORMAL_FLATNESS_MAX) {
        why = "flatness " + std::to_string(v[2]) + " is outside 0.." + std::to_string(PCS_NORMAL_FLATNESS_MAX);
        return false;
    }
    radius_mm = (int)v[0]; min_neighbors = (int)v[1]; flatness = (int)v[2];
    return true;
}

inline bool parse_int(const char* arg, int lo, int hi, int& out)
{
    char* end = nullptr;
    errno = 0;
    const long v = strtol(arg, &end, 10);
    if (end == arg || *end || errno || v < lo || v > hi) return false;
    out = (int)v;
    return true;
}

// The whole command line. False: `why` says what is wrong (the caller prints it with the usage and exits 2).
inline bool parse(int argc, char** argv, Options& o, std::string& why)
{
    optind = 1;
    opterr = 0;
    int c;
    while ((c = getopt(argc, argv, "T:o:A:p:R:g:t")) != -1) {
        switch (c) {
            case 'T': o.in_path = optarg; break;
            case 'o': o.out_path = optarg; break;
            case 'A': {
                std::string w;
                if (!parse_a(optarg, o.max_dist_mm, o.iterations, o.stride, w)) { why = std::string("-A ") + optarg + ": " + w; return false; }
                break;
            }
            case 'p': {
                std::string w;
                if (!parse_p(optarg, o.normal_radius_mm, o.normal_min_neighbors, o.normal_flatness, w)) {
                    why = std::string("-p ") + optarg + ": " + w;
                    return false;
                }
                o.plane = true;
                break;
            }
            case 'R': if (!parse_int(optarg, 0, PCS_MAX_STREAMS - 1, o.ref)) { why = std::string("-R ") + optarg + ": expected a camera index"; return false; } break;
            case 'g': if (!parse_int(optarg, 0, 1023, o.gpu)) { why = std::string("-g ") + optarg + ": expected a device index"; return false; } break;
            case 't': o.timing = true; break;
            default:  why = std::string("unknown option or missing argument: -") + (char)optopt; return false;
        }
    }
    for (int i = optind; i < argc; i++) o.cams.push_back(argv[i]);
    if (!o.in_path) { why = "-T in.txt is required"; return false; }
    if (!o.out_path) { why = "-o out.txt is required"; return false; }
    if (o.cams.size() < 2) { why = "at least two camera files are needed"; return false; }
    if (o.cams.size() > (size_t)PCS_MAX_STREAMS) { why = "at most " + std::to_string(PCS_MAX_STREAMS) + " cameras"; return false; }
    if (o.ref >= (int)o.cams.size()) { why = "-R " + std::to_string(o.ref) + " is outside 0.." + std::to_string(o.cams.size() - 1); return false; }
    return true;
}

}  // namespace pcs_align
