// pcs_tracks.h — the -J option of pcs-multicamera-optimized: `-J <file>[,<cell_mm>[,<min_votes>]]`, the trajectory log of the -E
// stage's objects (include/pcs_hip.h: pcs_tracker_update_device): where it goes, the tracker's cell and vote threshold, and the
// file's lines. Parsed before any context exists, so a malformed option costs no device.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <ostream>
#include <string>

#include "../../include/pcs_hip.h"

namespace pcs_tracks {

constexpr int kDefaultCellMm = 100;
constexpr int kDefaultMinVotes = 1;

inline const char* help()
{
    return " -J <file>[,<cell_mm>[,<min_votes>]]  with -E: persistent identities for the clusters that stay: after EVERY frame-set <file>\n"
           "                  (- for stdout) gets one line per object, by first record: frame, k, id, age, prev, votes, then the object's\n"
           "                  label, size, bounding box and coordinate sums (one header line first); an object keeps its id while the\n"
           "                  majority of its records stand in cells (cell_mm 1..1000, default 100) its predecessor occupied, with at least\n"
           "                  min_votes (1..2^30, default 1) of them; -t prints `Tracks: <born> born, <continued> continued, <lost> lost`;\n"
           "                  without -L the object table holds 1024 objects; not with -G\n";
}

// One strict decimal integer in [lo, hi] from [p, end). false: `why` names `what`.
inline bool number(const char* p, const char* end, const char* what, long lo, long hi, long& v, std::string& why)
{
    static const char shape[] = "expected <file>[,<cell_mm>[,<min_votes>]]";
    const std::string text(p, end);
    char* stop = nullptr;
    errno = 0;
    v = strtol(text.c_str(), &stop, 10);
    if (text.empty() || text[0] == ' ' || text[0] == '\t' || text[0] == '+' || stop == text.c_str() || errno || *stop) {
        why = std::string(shape) + ", " + what + " an integer";
        return false;
    }
    if (v < lo || v > hi) {
        why = std::string(what) + " " + std::to_string(v) + " is outside " + std::to_string(lo) + ".." + std::to_string(hi);
        return false;
    }
    return true;
}

// <file>, <file>,<cell_mm> or <file>,<cell_mm>,<min_votes>: the file name ends at the first comma. On failure `why` says what is wrong.
inline bool parse(const char* arg, std::string& file, int& cell_mm, int& min_votes, std::string& why)
{
    const char* end = arg + strlen(arg);
    const char* c1 = strchr(arg, ',');
    const char* c2 = c1 ? strchr(c1 + 1, ',') : nullptr;
    if (c2 && strchr(c2 + 1, ',')) { why = "expected <file>[,<cell_mm>[,<min_votes>]], nothing after them"; return false; }
    long cell = kDefaultCellMm, votes = kDefaultMinVotes;
    if (c1 && !number(c1 + 1, c2 ? c2 : end, "cell_mm", PCS_BACKGROUND_CELL_MIN, PCS_BACKGROUND_CELL_MAX, cell, why)) return false;
    if (c2 && !number(c2 + 1, end, "min_votes", 1, PCS_TRACKER_MIN_VOTES_MAX, votes, why)) return false;
    file.assign(arg, c1 ? (size_t)(c1 - arg) : strlen(arg));
    if (file.empty()) { why = "expected <file>[,<cell_mm>[,<min_votes>]]: the file name is empty"; return false; }
    cell_mm = (int)cell; min_votes = (int)votes;
    return true;
}

inline void write_header(std::ostream& os)
{
    os << "# frame k id age prev votes label size lo_x lo_y lo_z hi_x hi_y hi_z sum_x sum_y sum_z\n";
}

// One frame-set's lines: raw integers separated by one space, nothing derived.
inline void write(std::ostream& os, long long frame, const pcs_track* tracks, const pcs_cluster_object* objects, int written)
{
    for (int k = 0; k < written; k++) {
        const pcs_track& t = tracks[k];
        const pcs_cluster_object& o = objects[k];
        os << frame << ' ' << k << ' ' << (long long)t.id << ' ' << t.age << ' ' << t.prev << ' ' << t.votes << ' ' << o.label << ' ' << o.size;
        for (int a = 0; a < 3; a++) os << ' ' << o.lo[a];
        for (int a = 0; a < 3; a++) os << ' ' << o.hi[a];
        for (int a = 0; a < 3; a++) os << ' ' << (long long)o.sum_xyz[a];
        os << '\n';
    }
}

}  // namespace pcs_tracks
