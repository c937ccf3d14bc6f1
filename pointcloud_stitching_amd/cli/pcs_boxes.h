// pcs_boxes.h — the -W option of pcs-multicamera-optimized: `-W <file>`, the oriented boxes of the -E stage's objects
// (include/pcs_hip.h: pcs_object_boxes_device): where they go and the file's lines. Parsed before any context exists, so a malformed
// option costs no device.
#pragma once

#include <cstring>
#include <ostream>
#include <string>

#include "../../include/pcs_hip.h"

namespace pcs_boxes {

inline const char* help()
{
    return " -W <file>        with -E: which way the clusters that stay lie: after EVERY frame-set <file> (- for stdout) gets one line per\n"
           "                  object, by first record: frame, k, then the box's integers as they are: count, the coordinate sums, the six\n"
           "                  second moments, three axes of three shorts (16384 = 1), rank, and the members' extents along the axes in\n"
           "                  mm/16384, lower then upper (one header line first; a line joins -J's on frame and k); -t prints\n"
           "                  `Boxes: <objects> objects, <r> of rank 3`; without -L the object table holds 1024 objects; not with -G\n";
}

// <file>: a name, nothing else. On failure `why` says what is wrong. (A comma is refused: the option has no parameters, and a name
// that begins with '-' other than "-" itself is an option that swallowed its neighbour.)
inline bool parse(const char* arg, std::string& file, std::string& why)
{
    if (!arg || !*arg) { why = "expected <file>: the file name is empty"; return false; }
    if (strchr(arg, ',')) { why = "expected <file>, nothing after it: the option has no parameters"; return false; }
    if (arg[0] == '-' && arg[1]) { why = "expected <file> (or - for stdout), not another option"; return false; }
    file = arg;
    return true;
}

inline void write_header(std::ostream& os)
{
    os << "# frame k count sum_x sum_y sum_z m_xx m_xy m_xz m_yy m_yz m_zz a0_x a0_y a0_z a1_x a1_y a1_z a2_x a2_y a2_z rank "
          "lo_0 lo_1 lo_2 hi_0 hi_1 hi_2 reserved\n";
}

// One frame-set's lines: raw integers separated by one space, nothing derived: frame, k and the entry's 27 in the struct's order.
inline void write(std::ostream& os, long long frame, const pcs_object_box* boxes, int written)
{
    for (int k = 0; k < written; k++) {
        const pcs_object_box& b = boxes[k];
        os << frame << ' ' << k << ' ' << (long long)b.count;
        for (int a = 0; a < 3; a++) os << ' ' << (long long)b.sum_xyz[a];
        for (int a = 0; a < 6; a++) os << ' ' << (long long)b.m2[a];
        for (int a = 0; a < 3; a++)
            for (int c = 0; c < 3; c++) os << ' ' << b.axis[a][c];
        os << ' ' << b.rank;
        for (int a = 0; a < 3; a++) os << ' ' << b.ext_lo[a];
        for (int a = 0; a < 3; a++) os << ' ' << b.ext_hi[a];
        os << ' ' << b.reserved << '\n';
    }
}

}  // namespace pcs_boxes
