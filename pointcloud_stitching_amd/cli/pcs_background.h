// pcs_background.h — the -X option of pcs-multicamera-optimized, two forms (include/pcs_hip.h: pcs_background_*):
//   -X learn:FILE,cell_mm[,max_cells]    learn every frame-set of the run into a background model, write it to FILE at the end
//   -X FILE[,min_percent[,dilate]]       subtract the model of FILE from every frame-set (a stage of the filter chain, in front of -O)
// Parsed before any context exists, so a malformed option costs no device; FILE of the second form is read and validated on the host
// (pcs_background_validate) before one is created, too.
#pragma once

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pcs_hip.h"

namespace pcs_background_cli {

constexpr int kDefaultMaxCells = 4194304, kDefaultPercent = 50, kDefaultDilate = 1;

inline const char* help()
{
    return " -X learn:<file>,<cell_mm>[,<max_cells>]  learn the background of a fixed rig: every frame-set of the run (after -T, -B / -d) marks\n"
           "                  the cells of edge cell_mm (1..1000) it touches; the frame-sets pass on unchanged; <file> gets the model (a PCB1\n"
           "                  container) when the run ends; max_cells (default 4194304) sizes the table: the run ends with status 1 if the\n"
           "                  scene has more cells; not with -G\n"
           " -X <file>[,<min_percent>[,<dilate>]]  background subtraction on the stitched cloud: a record goes iff its cell — with dilate 1\n"
           "                  (default; 0: the cell alone) one of the 27 around it — was seen in at least min_percent (1..100, default 50) of\n"
           "                  the learned frame-sets; after -T, -B / -d, before -O, -K, -M, -E and -V; not with -G\n";
}

// ",a[,b]" behind the file name: `n_max` integers at the most, each inside lo..hi. The FILE is everything in front of the first comma
// that is followed by integers and commas alone (a file name may hold commas, as -L's).
inline bool split(const char* arg, int n_min, int n_max, const char* const* names, const long long* lo, const long long* hi, std::string& file,
                  long long* v, int& got, const char* shape, std::string& why)
{
    const std::string s = arg;
    size_t cut = s.size();
    int fields = 0;
    while (fields < n_max) {                     // peel integer fields off the end
        const size_t comma = s.rfind(',', cut ? cut - 1 : 0);
        if (comma == std::string::npos || comma + 1 >= cut) break;
        const std::string f = s.substr(comma + 1, cut - comma - 1);
        if (f.find_first_not_of("0123456789-") != std::string::npos) break;
        cut = comma;
        fields++;
    }
    if (fields < n_min || cut == 0) { why = shape; return false; }
    file = s.substr(0, cut);
    got = fields;
    const char* p = s.c_str() + cut;
    for (int k = 0; k < fields; k++) {
        p++;                                     // the comma
        char* end = nullptr;
        errno = 0;
        v[k] = strtoll(p, &end, 10);
        if (end == p || errno || (*end && *end != ',')) { why = shape; return false; }
        p = end;
        if (v[k] < lo[k] || v[k] > hi[k]) {
            why = std::string(names[k]) + " " + std::to_string(v[k]) + " is outside " + std::to_string(lo[k]) + ".." + std::to_string(hi[k]);
            return false;
        }
    }
    return true;
}

// "FILE,cell_mm[,max_cells]" (what follows "learn:")
inline bool parse_learn(const char* arg, std::string& file, int& cell_mm, int& max_cells, std::string& why)
{
    static const char shape[] = "expected learn:<file>,<cell_mm>[,<max_cells>]";
    static const char* const names[2] = {"cell_mm", "max_cells"};
    static const long long lo[2] = {PCS_BACKGROUND_CELL_MIN, 1}, hi[2] = {PCS_BACKGROUND_CELL_MAX, PCS_BACKGROUND_MAX_CELLS_MAX};
    long long v[2] = {0, kDefaultMaxCells};
    int got = 0;
    if (!split(arg, 1, 2, names, lo, hi, file, v, got, shape, why)) return false;
    cell_mm = (int)v[0];
    max_cells = (int)v[1];
    return true;
}

// "FILE[,min_percent[,dilate]]"
inline bool parse_subtract(const char* arg, std::string& file, int& min_percent, int& dilate, std::string& why)
{
    static const char shape[] = "expected <file>[,<min_percent>[,<dilate>]]";
    static const char* const names[2] = {"min_percent", "dilate"};
    static const long long lo[2] = {1, 0}, hi[2] = {100, 1};
    long long v[2] = {kDefaultPercent, kDefaultDilate};
    int got = 0;
    if (!*arg) { why = shape; return false; }
    if (!split(arg, 0, 2, names, lo, hi, file, v, got, shape, why)) return false;
    min_percent = (int)v[0];
    dilate = (int)v[1];
    return true;
}

// min_seen = max(1, ceil(frames min_percent / 100))
inline int min_seen_of(uint32_t frames, int min_percent)
{
    const long long m = ((long long)frames * min_percent + 99) / 100;
    return m < 1 ? 1 : (int)m;
}

// FILE's bytes, validated on the host. false: `why` names the file and what the validator found.
inline bool load(const std::string& file, std::vector<char>& bytes, struct pcs_background_info& info, std::string& why)
{
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) { why = "cannot read " + file; return false; }
    bytes.clear();
    char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);
    if (pcs_background_validate(bytes.data(), bytes.size(), &info) != PCS_OK) {
        const char* text = pcs_last_error(nullptr);
        why = file + ": " + (text ? text : "not a background model");
        return false;
    }
    return true;
}

}  // namespace pcs_background_cli
