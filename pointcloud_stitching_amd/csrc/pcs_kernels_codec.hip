// pcs_kernels_codec.hip — lossless payload compression for the wire ("PCZ1"; pcs_codec_format.h holds the
// container's layout and the host validator). A block is 64 consecutive 10-byte records = one wavefront, a lane is one record; a
// workgroup holds kCodecWaves blocks. Per block and channel (x, y, z: 16 bits; R, G, B, P: 8 bits) the records are delta-coded
// against their predecessor IN THE BLOCK, zigzag-mapped, and packed at the bit length of the OR of the block's residuals.
//
//   encode = count (block sizes) -> offsets (one workgroup: exclusive scan, block_end[], container header) -> emit (pack + store)
//   decode = one launch: unpack, inclusive wave prefix sum mod 2^k, records out
//
// No workgroup waits on another inside a launch. Every global access is a 4-byte access at a 4-byte aligned address, lane l at
// dword l of the block (coalesced), staged through LDS on both sides — except the last 2 bytes of a payload with an odd number of
// records, which are moved as one uint16 so that nothing at or beyond record n_points is read or written.
#include "pcs_device.h"
#include "pcs_kernels_common.h"

namespace pcs {

namespace {

constexpr int      kCodecWaves     = 4;                        // blocks per workgroup
constexpr int      kCodecThreads   = 64 * kCodecWaves;
constexpr uint32_t kRecDwords      = 160;                      // 64 records x 10 bytes
constexpr uint32_t kBlkDwords      = 164;                      // the largest block: 656 bytes
constexpr uint32_t kCodecMagic     = 0x315A4350u;              // "PCZ1"
constexpr uint32_t kScanThreads    = 1024;                     // blocks per pass of the offsets kernel (pcs_device.h: kCodecScanBlocks)
static_assert(kScanThreads == kCodecScanBlocks, "the offsets kernel covers kCodecScanBlocks blocks per pass");

struct Channels { uint32_t v[7]; };      // x y z R G B P of one record

// Wavefront-wide OR, valid in lane 63 (the DPP ladder of wave_inclusive_scan with | for +; all lanes active).
__device__ __forceinline__ uint32_t wave_or_lane63(uint32_t x)
{
    uint32_t v = x;
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_or_lane63(x), 63); }

__device__ __forceinline__ uint32_t bit_length(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }

// The first m records of block `blk` of the payload into rec[0 .. 160) (dwords past the block's last byte are zero). All 64 lanes.
__device__ __forceinline__ void load_block(const uint8_t* __restrict__ payload, size_t blk, uint32_t m, uint32_t lane, uint32_t* rec)
{
    const uint8_t* src = payload + blk * (size_t)(kRecDwords * 4);
    const uint32_t bytes = m * PCS_POINT_BYTES, full = bytes >> 2;
    for (uint32_t j = lane; j < kRecDwords; j += 64) {
        uint32_t w = 0;
        if (j < full) w = reinterpret_cast<const uint32_t*>(src)[j];
        else if (j == full && (bytes & 2u)) w = reinterpret_cast<const uint16_t*>(src)[2 * j];
        rec[j] = w;
    }
}

// Record `lane` out of rec[] as its seven channels.
__device__ __forceinline__ Channels read_record(const uint32_t* rec, uint32_t lane)
{
    const uint32_t d = (5 * lane) >> 1;                 // 157 for lane 63: d + 2 <= 159
    const uint32_t w0 = rec[d], w1 = rec[d + 1], w2 = rec[d + 2];
    uint32_t a, b, c;                                   // shorts 0|1, 2|3, 4
    if (lane & 1) { a = __builtin_amdgcn_alignbit(w1, w0, 16); b = __builtin_amdgcn_alignbit(w2, w1, 16); c = w2 >> 16; }
    else          { a = w0; b = w1; c = w2 & 0xFFFFu; }
    Channels ch;
    ch.v[0] = a & 0xFFFFu; ch.v[1] = a >> 16; ch.v[2] = b & 0xFFFFu;
    ch.v[3] = (b >> 16) & 0xFFu; ch.v[4] = b >> 24; ch.v[5] = c & 0xFFu; ch.v[6] = c >> 8;
    return ch;
}

// The zigzag residuals of this lane's record against the previous lane's (0 for record 0 and for lanes at or past m), and the
// block's width word. own: this lane's channels. All 64 lanes.
__device__ __forceinline__ uint32_t residuals(const Channels& own, uint32_t lane, uint32_t m, Channels& z, uint32_t (&w)[7])
{
    // the predecessor comes from the neighbouring lane: three packed dwords through the cross-lane network
    const uint32_t p0 = own.v[0] | own.v[1] << 16, p1 = own.v[2] | own.v[3] << 16 | own.v[4] << 24, p2 = own.v[5] | own.v[6] << 8;
    const uint32_t q0 = (uint32_t)__shfl_up((int)p0, 1), q1 = (uint32_t)__shfl_up((int)p1, 1), q2 = (uint32_t)__shfl_up((int)p2, 1);
    Channels prev;
    prev.v[0] = q0 & 0xFFFFu; prev.v[1] = q0 >> 16; prev.v[2] = q1 & 0xFFFFu;
    prev.v[3] = (q1 >> 16) & 0xFFu; prev.v[4] = q1 >> 24; prev.v[5] = q2 & 0xFFu; prev.v[6] = q2 >> 8;
    const bool coded = lane >= 1 && lane < m;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const int bits = k < 3 ? 16 : 8;
        // s = the difference mod 2^k read as signed; zigzag: s >= 0 ? 2 s : -2 s - 1
        const int32_t s = (int32_t)((own.v[k] - prev.v[k]) << (32 - bits)) >> (32 - bits);
        const uint32_t zz = ((uint32_t)s << 1) ^ (uint32_t)(s >> 31);
        z.v[k] = coded ? (zz & ((1u << bits) - 1u)) : 0u;
    }
    // OR-reduce the seven residuals across the wave, three packed dwords
    const uint32_t o0 = wave_or(z.v[0] | z.v[1] << 16), o1 = wave_or(z.v[2] | z.v[3] << 16 | z.v[4] << 24), o2 = wave_or(z.v[5] | z.v[6] << 8);
    w[0] = bit_length(o0 & 0xFFFFu); w[1] = bit_length(o0 >> 16); w[2] = bit_length(o1 & 0xFFFFu);
    w[3] = bit_length((o1 >> 16) & 0xFFu); w[4] = bit_length(o1 >> 24); w[5] = bit_length(o2 & 0xFFu); w[6] = bit_length(o2 >> 8);
    return w[0] | w[1] << 5 | w[2] << 10 | w[3] << 15 | w[4] << 19 | w[5] << 23 | w[6] << 27;
}

__device__ __forceinline__ uint32_t block_words(uint32_t m, const uint32_t (&w)[7])
{
    uint32_t words = 4;
#pragma unroll
    for (int k = 0; k < 7; k++) words += (m * w[k] + 31) >> 5;
    return words;
}

// ---- encode 1: the byte size of every block ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCodecThreads)
void pcs_codec_count_kernel(const uint8_t* __restrict__ payload, uint32_t n_points, uint32_t n_blocks, uint32_t* __restrict__ sizes)
{
    __shared__ uint32_t rec_s[kCodecWaves][kRecDwords];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t blk = blockIdx.x * kCodecWaves + wv;
    const bool active = blk < n_blocks;                                   // wave-uniform
    const uint32_t m = active ? min(64u, n_points - blk * 64u) : 0u;
    uint32_t* rec = rec_s[wv];
    load_block(payload, active ? blk : 0, m, lane, rec);
    __syncthreads();
    const Channels own = read_record(rec, lane);
    Channels z;
    uint32_t w[7];
    residuals(own, lane, m, z, w);
    if (active && lane == 0) sizes[blk] = 4u * block_words(m, w);
}

// ---- encode 2: offsets. ONE workgroup: exclusive scan of the block sizes, kScanThreads blocks per pass; writes block_end[], the
// container's 16-byte header and (optionally) *out_bytes ------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads)
void pcs_codec_offsets_kernel(const uint32_t* __restrict__ sizes, uint32_t n_points, uint32_t n_blocks, uint32_t* __restrict__ container,
                              uint32_t* __restrict__ out_bytes)
{
    __shared__ uint32_t wtot[kScanThreads / 64];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 16u + 4u * n_blocks;                  // where block 0 starts
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += kScanThreads) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t c = b < n_blocks ? sizes[b] : 0u;
        uint32_t wave_total;
        const uint32_t ex = wave_exclusive_scan(c, wave_total);
        if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = wave_total;
        __syncthreads();
        uint32_t before = carry_s;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wtot[w];
        if (b < n_blocks) container[4 + b] = before + ex + c;             // block_end[b]
        __syncthreads();
        if (threadIdx.x == kScanThreads - 1) carry_s = before + ex + c;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t total = carry_s;
        container[0] = kCodecMagic; container[1] = n_points; container[2] = n_blocks; container[3] = total;
        if (out_bytes) *out_bytes = total;
    }
}

// ---- encode 3: recompute, pack in LDS, store -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCodecThreads)
void pcs_codec_emit_kernel(const uint8_t* __restrict__ payload, uint32_t n_points, uint32_t n_blocks, uint32_t* __restrict__ container)
{
    __shared__ uint32_t rec_s[kCodecWaves][kRecDwords];
    __shared__ uint32_t out_s[kCodecWaves][kBlkDwords];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t blk = blockIdx.x * kCodecWaves + wv;
    const bool active = blk < n_blocks;                                   // wave-uniform
    const uint32_t m = active ? min(64u, n_points - blk * 64u) : 0u;
    uint32_t* rec = rec_s[wv];
    uint32_t* out = out_s[wv];
    load_block(payload, active ? blk : 0, m, lane, rec);
    for (uint32_t j = lane; j < kBlkDwords; j += 64) out[j] = 0;
    __syncthreads();
    const Channels own = read_record(rec, lane);
    Channels z;
    uint32_t w[7];
    const uint32_t wword = residuals(own, lane, m, z, w);
    if (lane == 0) {                                                      // record 0 is the block's v0
        out[0] = own.v[0] | own.v[1] << 16;
        out[1] = own.v[2] | own.v[3] << 16 | own.v[4] << 24;
        out[2] = own.v[5] | own.v[6] << 8 | (wword & 0xFFFFu) << 16;
        out[3] = wword >> 16;
    }
    uint32_t off = 4;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const uint32_t bit = lane * w[k], word = off + (bit >> 5), sh = bit & 31u;
        if (z.v[k]) {                                                     // (a non-zero residual implies w > 0 and 1 <= lane < m)
            atomicOr(&out[word], z.v[k] << sh);
            if (sh + w[k] > 32u) atomicOr(&out[word + 1], z.v[k] >> (32u - sh));
        }
        off += (m * w[k] + 31) >> 5;
    }
    __syncthreads();
    if (!active) return;
    // block b starts where block b - 1 ends (the offsets launch wrote the table into the container itself)
    const uint32_t start = blk ? container[4 + blk - 1] : 16u + 4u * n_blocks;
    uint32_t* dst = container + (start >> 2);
    for (uint32_t j = lane; j < off; j += 64) dst[j] = out[j];
}

// ---- decode: one wave per block ----------------------------------------------------------------------------------------------------
// Reads nothing at or beyond in_bytes and writes nothing at or beyond record n_points, whatever the bytes say: the block's extent is
// clamped to the container, the block is copied to LDS (zero past its end), the widths are clamped, and every later read is an LDS
// read below kBlkDwords.
__global__ __launch_bounds__(kCodecThreads)
void pcs_codec_decode_kernel(const uint32_t* __restrict__ container, uint32_t in_bytes, uint32_t n_points, uint32_t n_blocks,
                             uint8_t* __restrict__ payload)
{
    __shared__ uint32_t blk_s[kCodecWaves][kBlkDwords];
    __shared__ uint32_t rec_s[kCodecWaves][kRecDwords];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t blk = blockIdx.x * kCodecWaves + wv;
    const bool active = blk < n_blocks;                                   // wave-uniform
    const uint32_t m = active ? min(64u, n_points - blk * 64u) : 0u;
    uint32_t* in = blk_s[wv];
    uint32_t* rec = rec_s[wv];
    const uint32_t in_dwords = in_bytes >> 2;
    const uint32_t data = 4u + n_blocks;                                  // (the host checked 16 + 4 n_blocks <= in_bytes)
    uint32_t start = 0, end = 0;                                          // in dwords
    if (active) {
        start = blk ? container[4 + blk - 1] >> 2 : data;
        end = container[4 + blk] >> 2;
        start = min(start, in_dwords); end = min(end, in_dwords);
        if (end < start) end = start;
    }
    for (uint32_t j = lane; j < kBlkDwords; j += 64) in[j] = (j < end - start) ? container[start + j] : 0u;
    for (uint32_t j = lane; j < kRecDwords; j += 64) rec[j] = 0;
    __syncthreads();
    uint32_t w[7];
    {
        const uint32_t wword = in[2] >> 16 | in[3] << 16;
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = min((wword >> (5 * k)) & 31u, 16u);
#pragma unroll
        for (int k = 0; k < 4; k++) w[3 + k] = min((wword >> (15 + 4 * k)) & 15u, 8u);
    }
    const uint32_t v0[7] = {in[0] & 0xFFFFu, in[0] >> 16, in[1] & 0xFFFFu, (in[1] >> 16) & 0xFFu, in[1] >> 24, in[2] & 0xFFu, (in[2] >> 8) & 0xFFu};
    Channels v;
    uint32_t off = 4;                                                     // at most 4 + 3 * 32 + 4 * 16 = 164 after the last channel
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const uint32_t bit = lane * w[k], word = off + (bit >> 5), sh = bit & 31u;
        // z from at most two words; word <= off + 31 < kBlkDwords for a channel with w > 0
        const uint32_t lo = in[min(word, kBlkDwords - 1)], hi = in[min(word + 1, kBlkDwords - 1)];
        const uint32_t zz = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & ((1u << w[k]) - 1u);
        const uint32_t s = (lane >= 1 && lane < m) ? ((zz >> 1) ^ (0u - (zz & 1u))) : 0u;
        // v_i = v_0 + the inclusive prefix sum of the signed residuals, mod 2^k
        v.v[k] = (v0[k] + wave_inclusive_scan(s)) & (k < 3 ? 0xFFFFu : 0xFFu);
        off += (m * w[k] + 31) >> 5;
    }
    if (lane < m) {
        uint16_t* r16 = reinterpret_cast<uint16_t*>(rec) + 5 * lane;
        r16[0] = (uint16_t)v.v[0]; r16[1] = (uint16_t)v.v[1]; r16[2] = (uint16_t)v.v[2];
        r16[3] = (uint16_t)(v.v[3] | v.v[4] << 8); r16[4] = (uint16_t)(v.v[5] | v.v[6] << 8);
    }
    __syncthreads();
    if (!active) return;
    uint8_t* dst = payload + (size_t)blk * (kRecDwords * 4);
    const uint32_t bytes = m * PCS_POINT_BYTES, full = bytes >> 2;
    for (uint32_t j = lane; j < kRecDwords; j += 64) {
        if (j < full) reinterpret_cast<uint32_t*>(dst)[j] = rec[j];
        else if (j == full && (bytes & 2u)) reinterpret_cast<uint16_t*>(dst)[2 * j] = (uint16_t)rec[j];
    }
}

}  // namespace

hipError_t launch_codec_encode(const int16_t* d_payload, uint32_t n_points, uint32_t* d_sizes, void* d_out, uint32_t* d_out_bytes,
                               hipStream_t st)
{
    const uint32_t nb = (n_points + 63) / 64;
    const uint8_t* in = reinterpret_cast<const uint8_t*>(d_payload);
    uint32_t* out = static_cast<uint32_t*>(d_out);
    const dim3 grid((nb + kCodecWaves - 1) / kCodecWaves);
    if (nb) hipLaunchKernelGGL(pcs_codec_count_kernel, grid, dim3(kCodecThreads), 0, st, in, n_points, nb, d_sizes);
    hipLaunchKernelGGL(pcs_codec_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, d_sizes, n_points, nb, out, d_out_bytes);
    if (nb) hipLaunchKernelGGL(pcs_codec_emit_kernel, grid, dim3(kCodecThreads), 0, st, in, n_points, nb, out);
    return hipGetLastError();
}

hipError_t launch_codec_decode(const void* d_in, uint32_t in_bytes, uint32_t n_points, int16_t* d_payload, hipStream_t st)
{
    const uint32_t nb = (n_points + 63) / 64;
    if (!nb) return hipSuccess;
    if ((uint64_t)16 + 4ull * nb > in_bytes) return hipErrorInvalidValue;      // the table itself must lie inside the container
    hipLaunchKernelGGL(pcs_codec_decode_kernel, dim3((nb + kCodecWaves - 1) / kCodecWaves), dim3(kCodecThreads), 0, st,
                       static_cast<const uint32_t*>(d_in), in_bytes, n_points, nb, reinterpret_cast<uint8_t*>(d_payload));
    return hipGetLastError();
}

}  // namespace pcs
