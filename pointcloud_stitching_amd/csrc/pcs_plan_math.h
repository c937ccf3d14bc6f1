// pcs_plan_math.h — the integer arithmetic of the plan-view maps (DESIGN.md section 3 "Plan-view maps"): the parameter ranges, the cell
// of a record (an exact unsigned 16-bit division by the cell edge as one multiply and shift), and the 64-bit keys whose unsigned
// maximum settles a cell's top and bottom record and the tie between equal heights at once. Plain C++ without a dependency; host and
// device compile the same text: pcs_kernels_plan.hip takes it per record, pcs_capi_plan.cpp for the checks, tools/plan_host.cpp runs
// it behind a plain loop and sweeps the division over every numerator and every cell edge.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCS_PLAN_HD __host__ __device__ __forceinline__
#else
#define PCS_PLAN_HD inline
#endif

namespace pcs {

constexpr int kPlanSideMax = 4096;              // width and height, each
constexpr int kPlanCellsMax = 1 << 22;          // width * height: 64 MiB of keys, 44 MiB of rasters at the most
constexpr int kPlanParamWords = 12;             // pcs_plan_params as int32 words, in the struct's order

// What a launch takes of pcs_plan_params, behind the checks: `magic` = plan_magic(cell_mm).
struct PlanArgs {
    int32_t  up_axis, up_sign, cell_mm;
    uint32_t magic;
    int32_t  origin_u, origin_v, width, height, band_lo, band_hi;
};

// 0, or 1 + the index of the first word of pcs_plan_params (up_axis, up_sign, cell_mm, origin_u, origin_v, width, height, band_lo,
// band_hi, reserved[3]) that is out of range. width * height beyond kPlanCellsMax is height's fault; band_lo > band_hi is band_hi's.
PCS_PLAN_HD int plan_bad_param(const int32_t* w)
{
    if (w[0] < 0 || w[0] > 2) return 1;
    if (w[1] != 1 && w[1] != -1) return 2;
    if (w[2] < 1 || w[2] > 32767) return 3;
    if (w[3] < -32768 || w[3] > 32767) return 4;
    if (w[4] < -32768 || w[4] > 32767) return 5;
    if (w[5] < 1 || w[5] > kPlanSideMax) return 6;
    if (w[6] < 1 || w[6] > kPlanSideMax || (int64_t)w[5] * w[6] > kPlanCellsMax) return 7;
    if (w[7] < -32768 || w[7] > 32767) return 8;
    if (w[8] < -32768 || w[8] > 32767 || w[8] < w[7]) return 9;
    if (w[9] != 0) return 10;
    if (w[10] != 0) return 11;
    if (w[11] != 0) return 12;
    return 0;
}

// floor(d / c) for d in 0..65535 as (d * m) >> 32 with m = floor(2^32 / c) + 1, exact for every d and every c in 2..32767
// (tools/plan_host.cpp sweeps all of them; the host checks the c in use again before the first launch with it). c = 1: d itself,
// m = 2^32 + 1 has no 32-bit form.
PCS_PLAN_HD uint32_t plan_magic(int32_t c) { return c >= 2 ? (uint32_t)(0x100000000ull / (uint32_t)c) + 1u : 0u; }
PCS_PLAN_HD uint32_t plan_div(uint32_t d, int32_t c, uint32_t magic)
{
    return c == 1 ? d : (uint32_t)(((uint64_t)d * magic) >> 32);
}

// the coordinate along the up axis / the first / the second map axis: u = (a + 1) % 3, v = (a + 2) % 3 (selects: no indexed array)
PCS_PLAN_HD int plan_up(const PlanArgs& P, int x, int y, int z) { return P.up_axis == 0 ? x : P.up_axis == 1 ? y : z; }
PCS_PLAN_HD int plan_u(const PlanArgs& P, int x, int y, int z) { return P.up_axis == 0 ? y : P.up_axis == 1 ? z : x; }
PCS_PLAN_HD int plan_v(const PlanArgs& P, int x, int y, int z) { return P.up_axis == 0 ? z : P.up_axis == 1 ? x : y; }

PCS_PLAN_HD bool plan_in_band(const PlanArgs& P, int up) { return up >= P.band_lo && up <= P.band_hi; }

// The cell cv * width + cu of a record, or -1 when it is off the map. A negative difference is off the map before any division; a
// non-negative one is at most 32767 + 32768 = 65535.
PCS_PLAN_HD int plan_cell(const PlanArgs& P, int x, int y, int z)
{
    const int du = plan_u(P, x, y, z) - P.origin_u, dv = plan_v(P, x, y, z) - P.origin_v;
    if (du < 0 || dv < 0) return -1;
    const uint32_t cu = plan_div((uint32_t)du, P.cell_mm, P.magic), cv = plan_div((uint32_t)dv, P.cell_mm, P.magic);
    if (cu >= (uint32_t)P.width || cv >= (uint32_t)P.height) return -1;
    return (int)(cv * (uint32_t)P.width + cu);
}

// The keys. h = up_sign * p[up_axis] in -32768 .. 32768, hb = h + 32768 in 0 .. 65536; i the record's index (< 2^31, so the low
// word is never 0 and a key is never 0: 0 is the empty cell). Under an unsigned maximum the top key prefers the greater h, the bottom
// key the lesser, and both the LOWER index among equals.
PCS_PLAN_HD int plan_hb(const PlanArgs& P, int up) { return P.up_sign * up + 32768; }
PCS_PLAN_HD unsigned long long plan_top_key(int hb, uint32_t i) { return (unsigned long long)(uint32_t)hb << 32 | (0xFFFFFFFFu - i); }
PCS_PLAN_HD unsigned long long plan_bottom_key(int hb, uint32_t i) { return (unsigned long long)(uint32_t)(65536 - hb) << 32 | (0xFFFFFFFFu - i); }
PCS_PLAN_HD uint32_t plan_key_index(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }
// the raw coordinate p[up_axis] a key stands for (up_sign is +-1: h * up_sign undoes it)
PCS_PLAN_HD int plan_top_raw(const PlanArgs& P, unsigned long long key) { return P.up_sign * ((int)(key >> 32) - 32768); }
PCS_PLAN_HD int plan_bottom_raw(const PlanArgs& P, unsigned long long key) { return P.up_sign * (32768 - (int)(key >> 32)); }

}  // namespace pcs
