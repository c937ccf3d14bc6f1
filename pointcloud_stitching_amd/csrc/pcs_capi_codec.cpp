// pcs_capi_codec.cpp — the payload codec's part of the C ABI (include/pcs_hip.h, "payload compression for the wire"): the size bound,
// the host validator (pcs_codec_format.h), the device encode / decode calls over pcs_kernels_codec.hip and the host-pointer decode.
// pcs_process_frames_compressed lives beside pcs_process_frames in pcs_capi.cpp, whose staging it shares.

#include <exception>

#include "pcs_codec_format.h"
#include "pcs_host.h"

using namespace pcs_host;

extern "C" {

size_t pcs_compressed_bound(int n_points)
{
    return n_points < 0 ? 0 : pcs_codec::bound((uint32_t)n_points);
}

int pcs_compressed_info(const void* bytes, size_t n_bytes, struct pcs_compressed_info* out)
{
    pcs_codec::Info info;
    char why[256];
    if (!pcs_codec::validate(bytes, n_bytes, &info, why, sizeof why)) return fail(nullptr, PCS_ERR_INVALID_ARG, "%s", why);
    if (out) { out->n_points = info.n_points; out->n_blocks = info.n_blocks; out->total_bytes = info.total_bytes; out->data_offset = info.data_offset; }
    return PCS_OK;
}

int pcs_compress_payload_device(pcs_ctx* c, const int16_t* d_payload, int n_points, void* d_out, size_t out_capacity, uint32_t* d_out_bytes)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (n_points < 0 || (uint32_t)n_points > pcs_codec::kMaxPoints)
        return fail(c, PCS_ERR_INVALID_ARG, "pcs_compress_payload_device: n_points %d is outside 0..%u", n_points, pcs_codec::kMaxPoints);
    if (!d_out || (!d_payload && n_points)) return fail(c, PCS_ERR_INVALID_ARG, "pcs_compress_payload_device: NULL pointer");
    if (((uintptr_t)d_payload | (uintptr_t)d_out | (uintptr_t)d_out_bytes) & 3u)
        return fail(c, PCS_ERR_INVALID_ARG, "pcs_compress_payload_device: d_payload, d_out and d_out_bytes must be 4-byte aligned");
    const size_t bound = pcs_codec::bound((uint32_t)n_points);
    if (out_capacity < bound)
        return fail(c, PCS_ERR_CAPACITY, "pcs_compress_payload_device: d_out holds %zu bytes, pcs_compressed_bound(%d) = %zu needed",
                    out_capacity, n_points, bound);
    if (ranges_overlap(d_payload, (size_t)n_points * PCS_POINT_BYTES, d_out, bound) ||
        (d_out_bytes && (ranges_overlap(d_out_bytes, 4, d_out, bound) || ranges_overlap(d_out_bytes, 4, d_payload, (size_t)n_points * PCS_POINT_BYTES))))
        return fail(c, PCS_ERR_INVALID_ARG, "pcs_compress_payload_device: d_payload, d_out and d_out_bytes must not overlap");
    DeviceGuard guard(c->device);
    const size_t nb = pcs_codec::blocks_of((uint32_t)n_points);
    if (int rc = ensure_idle(c, c->d_codec_sizes, c->codec_sizes_cap, std::max<size_t>(nb, 1) * sizeof(uint32_t))) return rc;
    HIPCHK(c, launch_codec_encode(d_payload, (uint32_t)n_points, c->d_codec_sizes, d_out, d_out_bytes, c->stream));
    return PCS_OK;
}

int pcs_decompress_payload_device(pcs_ctx* c, const void* d_in, size_t in_bytes, int n_points, int16_t* d_payload, size_t payload_shorts)
{
    if (!c) return PCS_ERR_INVALID_ARG;
    if (n_points < 0 || (uint32_t)n_points > pcs_codec::kMaxPoints)
        return fail(c, PCS_ERR_INVALID_ARG, "pcs_decompress_payload_device: n_points %d is outside 0..%u", n_points, pcs_codec::kMaxPoints);
    if (!d_in || (!d_payload && n_points)) return fail(c, PCS_ERR_INVALID_ARG, "pcs_decompress_payload_device: NULL pointer");
    if (((uintptr_t)d_in | (uintptr_t)d_payload) & 3u)
        return fail(c, PCS_ERR_INVALID_ARG, "pcs_decompress_payload_device: d_in and d_payload must be 4-byte aligned");
    const size_t nb = pcs_codec::blocks_of((uint32_t)n_points);
    if (in_bytes < pcs_codec::kHeaderBytes + 4 * nb || in_bytes > pcs_codec::bound((uint32_t)n_points) || (in_bytes & 3u))
        return fail(c, PCS_ERR_INVALID_ARG, "pcs_decompress_payload_device: %zu bytes cannot be a container of %d records "
                    "(a multiple of 4 in %zu..%zu)", in_bytes, n_points, pcs_codec::kHeaderBytes + 4 * nb, pcs_codec::bound((uint32_t)n_points));
    if (payload_shorts < (size_t)n_points * PCS_POINT_SHORTS)
        return fail(c, PCS_ERR_CAPACITY, "pcs_decompress_payload_device: d_payload holds %zu shorts, %zu needed", payload_shorts,
                    (size_t)n_points * PCS_POINT_SHORTS);
    if (ranges_overlap(d_in, in_bytes, d_payload, (size_t)n_points * PCS_POINT_BYTES))
        return fail(c, PCS_ERR_INVALID_ARG, "pcs_decompress_payload_device: d_in and d_payload must not overlap");
    DeviceGuard guard(c->device);
    HIPCHK(c, launch_codec_decode(d_in, (uint32_t)in_bytes, (uint32_t)n_points, d_payload, c->stream));
    return PCS_OK;
}

int pcs_decompress_payload(pcs_ctx* c, const void* in, size_t in_bytes, int16_t* d_payload, size_t payload_shorts, int* n_points)
try {
    if (!c) return PCS_ERR_INVALID_ARG;
    if (!n_points) return fail(c, PCS_ERR_INVALID_ARG, "pcs_decompress_payload: n_points is NULL");
    // nothing malformed reaches a kernel: the validator's verdict (and its text) first
    pcs_codec::Info info;
    char why[256];
    if (!pcs_codec::validate(in, in_bytes, &info, why, sizeof why)) return fail(c, PCS_ERR_INVALID_ARG, "%s", why);
    if (payload_shorts < (size_t)info.n_points * PCS_POINT_SHORTS)
        return fail(c, PCS_ERR_CAPACITY, "pcs_decompress_payload: d_payload holds %zu shorts, the container's %u records need %zu",
                    payload_shorts, info.n_points, (size_t)info.n_points * PCS_POINT_SHORTS);
    DeviceGuard guard(c->device);
    if (int rc = ensure_idle(c, c->d_codec_buf, c->codec_buf_cap, in_bytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_codec_buf, in, in_bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = pcs_decompress_payload_device(c, c->d_codec_buf, in_bytes, (int)info.n_points, d_payload, payload_shorts)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_points = (int)info.n_points;
    return PCS_OK;
} catch (const std::exception& ex) {
    return fail(c, PCS_ERR_NOMEM, "pcs_decompress_payload: host allocation failed (%s)", ex.what());
}

}  // extern "C"
