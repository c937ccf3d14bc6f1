// pcs_codec_format.h — the "PCZ1" container: constants, size arithmetic and the host-side validator. Plain
// C++ with no dependency on HIP or on the rest of the library, so that a stand-alone program can include it
// (tools/codec_validate_fuzz.cpp). pcs_compressed_info (pcs_capi_codec.cpp) is a thin wrapper around validate().
//
//    0  uint32 magic = 0x315A4350 ("PCZ1")     4  uint32 n_points     8  uint32 n_blocks = ceil(n_points / 64)
//   12  uint32 total_bytes (multiple of 4)    16  uint32 block_end[n_blocks]    then the blocks, back to back
//   block: 16-byte header {v0 of x, y, z (uint16), v0 of R, G, B, P (uint8), uint32 widths, 2 zero bytes}, then the bit strings of
//          the seven channels, each ceil(m * w / 32) uint32 words
#ifndef PCS_CODEC_FORMAT_H
#define PCS_CODEC_FORMAT_H

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace pcs_codec {

constexpr uint32_t kMagic        = 0x315A4350u;
constexpr uint32_t kBlockRecords = 64;
constexpr uint32_t kHeaderBytes  = 16;                 // of the container, and of a block
constexpr uint32_t kMaxBlockBytes = 16 + 8 * (3 * 16 + 4 * 8);      // 656
constexpr uint32_t kMaxPoints    = 0x7FFFFFFF / 10;    // a payload's byte count fits an int32 (the wire's length word)

struct Info {
    uint32_t n_points = 0, n_blocks = 0, total_bytes = 0, data_offset = 0;
};

inline uint32_t blocks_of(uint32_t n_points) { return (n_points + kBlockRecords - 1) / kBlockRecords; }
inline size_t bound(uint32_t n_points) { return (size_t)kHeaderBytes + (size_t)(kMaxBlockBytes + 4) * blocks_of(n_points); }

inline uint32_t load32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The seven widths of a block's width word: x, y, z at bits 0, 5, 10 (5 bits each), R, G, B, P at bits 15, 19, 23, 27 (4 bits each).
inline void widths_of(uint32_t word, uint32_t (&w)[7])
{
    for (int k = 0; k < 3; k++) w[k] = (word >> (5 * k)) & 31u;
    for (int k = 0; k < 4; k++) w[3 + k] = (word >> (15 + 4 * k)) & 15u;
}
// Bytes of a block of m records with these widths.
inline uint32_t block_bytes(uint32_t m, const uint32_t (&w)[7])
{
    uint32_t words = 0;
    for (int k = 0; k < 7; k++) words += (m * w[k] + 31) / 32;
    return kHeaderBytes + 4 * words;
}

// Everything a decoder relies on (padding bits inside words are not checked). Returns true and fills *out, or false with the first
// violation in why[why_len]. Reads bytes[0 .. n_bytes) only.
inline bool validate(const void* bytes_, size_t n_bytes, Info* out, char* why, size_t why_len)
{
    const uint8_t* bytes = static_cast<const uint8_t*>(bytes_);
#define PCS_CODEC_FAIL(...) do { if (why && why_len) snprintf(why, why_len, __VA_ARGS__); return false; } while (0)
    if (n_bytes < kHeaderBytes) PCS_CODEC_FAIL("container: %zu bytes, shorter than the 16-byte header", n_bytes);
    if (!bytes) PCS_CODEC_FAIL("container: NULL pointer");
    const uint32_t magic = load32(bytes), n = load32(bytes + 4), nb = load32(bytes + 8), total = load32(bytes + 12);
    if (magic != kMagic) PCS_CODEC_FAIL("container: magic 0x%08X is not 0x%08X (\"PCZ1\")", magic, kMagic);
    if (n > kMaxPoints) PCS_CODEC_FAIL("container: n_points %u exceeds %u", n, kMaxPoints);
    if (nb != blocks_of(n)) PCS_CODEC_FAIL("container: n_blocks %u is not ceil(n_points %u / 64) = %u", nb, n, blocks_of(n));
    if (total != n_bytes) PCS_CODEC_FAIL("container: total_bytes %u but %zu bytes were given", total, n_bytes);
    if (total & 3u) PCS_CODEC_FAIL("container: total_bytes %u is not a multiple of 4", total);
    const uint64_t data = (uint64_t)kHeaderBytes + 4ull * nb;
    if (data > n_bytes) PCS_CODEC_FAIL("container: the table of %u blocks ends at byte %llu, past the %zu bytes given", nb,
                                       (unsigned long long)data, n_bytes);
    uint32_t start = (uint32_t)data;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t end = load32(bytes + kHeaderBytes + 4 * (size_t)b);
        if (end > total) PCS_CODEC_FAIL("block %u: block_end %u lies past total_bytes %u", b, end, total);
        if (end <= start) PCS_CODEC_FAIL("block %u: block_end %u does not lie above its start %u (the table must increase)", b, end, start);
        if (end - start < kHeaderBytes) PCS_CODEC_FAIL("block %u: %u bytes, shorter than a block header", b, end - start);
        const uint8_t* h = bytes + start;
        const uint32_t word = load32(h + 10);
        uint32_t w[7];
        widths_of(word, w);
        static const char* const names = "xyzRGBP";
        for (int k = 0; k < 7; k++)
            if (w[k] > (k < 3 ? 16u : 8u)) PCS_CODEC_FAIL("block %u: width %u of channel %c exceeds %u", b, w[k], names[k], k < 3 ? 16u : 8u);
        if ((word >> 31) || h[14] || h[15]) PCS_CODEC_FAIL("block %u: reserved bits of the header are not zero", b);
        const uint32_t m = (b + 1 < nb) ? kBlockRecords : n - kBlockRecords * (nb - 1);
        const uint32_t want = block_bytes(m, w);
        if (end - start != want) PCS_CODEC_FAIL("block %u: %u bytes, but its widths and %u records need %u", b, end - start, m, want);
        start = end;
    }
    if (start != total) PCS_CODEC_FAIL("container: the blocks end at byte %u, not at total_bytes %u", start, total);
#undef PCS_CODEC_FAIL
    if (out) { out->n_points = n; out->n_blocks = nb; out->total_bytes = total; out->data_offset = (uint32_t)data; }
    return true;
}

}  // namespace pcs_codec

#endif
