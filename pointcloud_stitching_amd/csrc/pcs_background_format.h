// pcs_background_format.h — the "PCB1" container of a background model: constants, size arithmetic and the
// host-side validator. Plain C++ with no dependency on HIP or on the rest of the library, so that a stand-alone program can include it
// (tools/background_validate_fuzz.cpp). pcs_background_validate (pcs_capi_background.cpp) is a thin wrapper around validate().
//
//    0  "PCB1" (uint32 0x31424350)    4  uint32 version = 1    8  int32 cell_mm (1..1000)    12  uint32 frames (0..65535)
//   16  uint32 cells                 20  12 zero bytes        32  cells entries of 12 bytes:
//   entry: uint16 cx, cy, cz, uint16 0, uint32 seen (1..frames) — strictly ascending by key = cx | cy << 16 | cz << 32
// Everything little-endian. One model is one byte string: the entries are sorted, nothing in the container is unspecified.
#ifndef PCS_BACKGROUND_FORMAT_H
#define PCS_BACKGROUND_FORMAT_H

#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace pcs_background_format {

constexpr uint32_t kMagic       = 0x31424350u;
constexpr uint32_t kVersion     = 1;
constexpr uint32_t kHeaderBytes = 32;
constexpr uint32_t kEntryBytes  = 12;
constexpr int32_t  kCellMin     = 1, kCellMax = 1000;
constexpr uint32_t kFramesMax   = 65535;
constexpr uint32_t kMaxCellsMax = 1u << 26;            // what a model may be created for: a 2 GiB table

struct Info {
    int32_t  cell_mm = 0;
    uint32_t frames = 0, cells = 0;
};

inline size_t bound(uint32_t max_cells) { return (size_t)kHeaderBytes + (size_t)kEntryBytes * max_cells; }

inline uint32_t load16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t load32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void store16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
inline void store32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// the key of the entry at p: cx | cy << 16 | cz << 32, the kernels' cell_key
inline uint64_t entry_key(const uint8_t* p) { return (uint64_t)load16(p) | (uint64_t)load16(p + 2) << 16 | (uint64_t)load16(p + 4) << 32; }

inline void write_header(uint8_t* out, int32_t cell_mm, uint32_t frames, uint32_t cells)
{
    store32(out, kMagic); store32(out + 4, kVersion); store32(out + 8, (uint32_t)cell_mm); store32(out + 12, frames); store32(out + 16, cells);
    for (int k = 20; k < 32; k++) out[k] = 0;
}
inline void write_entry(uint8_t* out, uint64_t key, uint32_t seen)
{
    store16(out, (uint32_t)(key & 0xFFFFu)); store16(out + 2, (uint32_t)(key >> 16 & 0xFFFFu)); store16(out + 4, (uint32_t)(key >> 32 & 0xFFFFu));
    store16(out + 6, 0); store32(out + 8, seen);
}

// Everything an importer relies on. Returns true and fills *out, or false with the first violation in why[why_len]. Reads
// bytes[0 .. n_bytes) only.
inline bool validate(const void* bytes_, size_t n_bytes, Info* out, char* why, size_t why_len)
{
    const uint8_t* bytes = static_cast<const uint8_t*>(bytes_);
#define PCS_BG_FAIL(...) do { if (why && why_len) snprintf(why, why_len, __VA_ARGS__); return false; } while (0)
    if (!bytes) PCS_BG_FAIL("background model: NULL pointer");
    if (n_bytes < kHeaderBytes) PCS_BG_FAIL("background model: %zu bytes, shorter than the 32-byte header", n_bytes);
    const uint32_t magic = load32(bytes), version = load32(bytes + 4), frames = load32(bytes + 12), cells = load32(bytes + 16);
    const int32_t cell_mm = (int32_t)load32(bytes + 8);
    if (magic != kMagic) PCS_BG_FAIL("background model: magic 0x%08X is not 0x%08X (\"PCB1\")", magic, kMagic);
    if (version != kVersion) PCS_BG_FAIL("background model: version %u is not %u", version, kVersion);
    if (cell_mm < kCellMin || cell_mm > kCellMax) PCS_BG_FAIL("background model: cell_mm %d is outside %d..%d", cell_mm, kCellMin, kCellMax);
    if (frames > kFramesMax) PCS_BG_FAIL("background model: frames %u exceeds %u", frames, kFramesMax);
    for (int k = 20; k < 32; k++)
        if (bytes[k]) PCS_BG_FAIL("background model: header byte %d is 0x%02X, not zero", k, bytes[k]);
    const uint64_t want = (uint64_t)kHeaderBytes + (uint64_t)kEntryBytes * cells;
    if (want != n_bytes) PCS_BG_FAIL("background model: %u cells need %llu bytes but %zu were given", cells, (unsigned long long)want, n_bytes);
    uint64_t prev = 0;
    for (uint32_t e = 0; e < cells; e++) {
        const uint8_t* p = bytes + kHeaderBytes + (size_t)kEntryBytes * e;
        const uint64_t key = entry_key(p);
        const uint32_t pad = load16(p + 6), seen = load32(p + 8);
        if (pad) PCS_BG_FAIL("entry %u: padding 0x%04X is not zero", e, pad);
        if (seen < 1 || seen > frames) PCS_BG_FAIL("entry %u: seen %u is outside 1..frames (%u)", e, seen, frames);
        if (e && key <= prev) PCS_BG_FAIL("entry %u: key 0x%012llX does not lie above entry %u's 0x%012llX (the keys must ascend strictly)", e,
                                          (unsigned long long)key, e - 1, (unsigned long long)prev);
        prev = key;
    }
#undef PCS_BG_FAIL
    if (out) { out->cell_mm = cell_mm; out->frames = frames; out->cells = cells; }
    return true;
}

}  // namespace pcs_background_format

#endif
