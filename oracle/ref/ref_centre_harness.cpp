/*
 * ref_centre_harness.cpp — C ABI around the reference's two CENTRE programs. TEST INFRASTRUCTURE ONLY.
 *
 * Like ref_harness.cpp: the reference translation unit is included BY PATH at build time (-DPCS_REF_TU=..., see ../Makefile
 * target `ref`), so none of its text lives in this tree, and the products, oracle/_ref/libpcs_ref_centre_opt.so (from
 * pcs-multicamera-optimized.cpp, -DPCS_REF_CENTRE_OPT) and oracle/_ref/libpcs_ref_centre_client.so (from
 * pcs-multicamera-client.cpp, -DPCS_REF_CENTRE_CLIENT), are never committed. The pcl/ headers beside this file are our own
 * declaration-only stand-ins.
 *
 * Every export stores its arguments into the globals the reference reads, calls the reference's function, and copies out what it
 * left: nothing in a record is computed here. The socket-driven functions run over socketpairs that stand for sockfd_array[0]
 * (the camera) and client_sockfd (the consumer); a writer and a reader thread keep a payload larger than a socket buffer from
 * blocking. Not reentrant: the reference's state is global (oracle/ref_centre.py serialises calls).
 */
#ifndef PCS_REF_TU
#error "build with -DPCS_REF_TU='\"<reference>/src/pcs-multicamera-{optimized,client}.cpp\"' (oracle/Makefile, target ref)"
#endif
#if !defined(PCS_REF_CENTRE_OPT) && !defined(PCS_REF_CENTRE_CLIENT)
#error "build with -DPCS_REF_CENTRE_OPT or -DPCS_REF_CENTRE_CLIENT"
#endif
#ifndef PCS_REF_FLAGS
#define PCS_REF_FLAGS "unknown"
#endif

#define main pcs_ref_centre_tu_main
#include PCS_REF_TU
#undef main

#include <vector>

namespace {

struct Wire {
    int cam[2];         /* cam[0] = sockfd_array[0], cam[1] = the camera's end */
    int cli[2];         /* cli[0] = client_sockfd,   cli[1] = the consumer's end */
    std::thread writer, reader;
    std::vector<char> got;
    bool ok;
};

void write_all(int fd, const char* p, size_t n)
{
    while (n > 0) {
        ssize_t w = write(fd, p, n);
        if (w <= 0) return;
        p += w; n -= (size_t)w;
    }
}

/* Open both pairs, queue the consumer's 'Z' request, start feeding `wire` (the camera's [int32 size][records]) and draining
 * whatever the reference writes to the consumer. */
bool wire_open(Wire& w, const char* wire, size_t wire_len)
{
    w.ok = false;
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, w.cam) != 0) return false;
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, w.cli) != 0) { close(w.cam[0]); close(w.cam[1]); return false; }
    sockfd_array[0] = w.cam[0];
    client_sockfd = w.cli[0];
    const char z = PULL_XYZRGB;
    write_all(w.cli[1], &z, 1);
    w.writer = std::thread(write_all, w.cam[1], wire, wire_len);
    w.reader = std::thread([&w]() {
        char chunk[65536];
        ssize_t r;
        while ((r = read(w.cli[1], chunk, sizeof chunk)) > 0) w.got.insert(w.got.end(), chunk, chunk + r);
    });
    w.ok = true;
    return true;
}

/* Close the reference's ends (the reader then sees the end of the stream), join, hand the bytes over. */
long wire_close(Wire& w, unsigned char* out, size_t out_cap)
{
    w.writer.join();
    close(w.cli[0]);
    w.reader.join();
    close(w.cli[1]); close(w.cam[0]); close(w.cam[1]);
    sockfd_array[0] = 0; client_sockfd = 0;
    if (w.got.size() > out_cap) return -2;
    memcpy(out, w.got.data(), w.got.size());
    return (long)w.got.size();
}

/* the camera's frame is well formed and within what the reference's fixed buffers hold */
bool wire_ok(const unsigned char* wire, size_t wire_len, int* n_points)
{
    int size;
    if (wire_len < sizeof(int)) return false;
    memcpy(&size, wire, sizeof(int));
    if (size < 0 || (size_t)size + sizeof(int) != wire_len || size % (5 * (int)sizeof(short)) != 0) return false;
    if ((size_t)size > sizeof(short) * (size_t)BUF_SIZE) return false;
    *n_points = size / (int)sizeof(short) / 5;
    return true;
}

}  // namespace

extern "C" {

const char* pcs_refc_compiler(void) { return __VERSION__; }
const char* pcs_refc_flags(void) { return PCS_REF_FLAGS; }
#ifdef PCS_REF_CENTRE_OPT
const char* pcs_refc_unit(void) { return "pcs-multicamera-optimized.cpp"; }
#else
const char* pcs_refc_unit(void) { return "pcs-multicamera-client.cpp"; }
#endif

/* convertBufferToPointCloudXYZRGB(payload, n_points) under `downsample`. xyz_out: 3 floats, rgb_out: 3 bytes per decoded point,
 * room for n_points / downsample of them. Returns the cloud's width, or -1 for what the harness refuses: n_points % downsample != 0,
 * where the reference's loop writes one element past its vector (undefined behaviour; never executed here). */
int pcs_refc_decode(const short* payload, int n_points, int ds, float* xyz_out, unsigned char* rgb_out)
{
    if (ds < 1 || n_points < 0 || n_points % ds != 0) return -1;
    downsample = ds;
    pointCloudXYZRGB::Ptr cloud = convertBufferToPointCloudXYZRGB(const_cast<short*>(payload), n_points);
    for (size_t i = 0; i < cloud->points.size(); i++) {
        xyz_out[3 * i + 0] = cloud->points[i].x; xyz_out[3 * i + 1] = cloud->points[i].y; xyz_out[3 * i + 2] = cloud->points[i].z;
        rgb_out[3 * i + 0] = cloud->points[i].r; rgb_out[3 * i + 1] = cloud->points[i].g; rgb_out[3 * i + 2] = cloud->points[i].b;
    }
    return (int)cloud->width;
}

/* convertPointCloudXYZRGBToBuffer on a cloud of `width` caller points: any float goes through static_cast<short> as compiled.
 * shorts_out: 5 * width shorts. Returns the size the reference returns. */
int pcs_refc_encode(const float* xyz, const unsigned char* rgb, int width, short* shorts_out)
{
    if (width < 0) return -1;
    pointCloudXYZRGB::Ptr cloud(new pointCloudXYZRGB);
    cloud->width = (uint32_t)width; cloud->height = 1; cloud->is_dense = false;
    cloud->points.resize((size_t)width);
    for (int i = 0; i < width; i++) {
        cloud->points[i].x = xyz[3 * i + 0]; cloud->points[i].y = xyz[3 * i + 1]; cloud->points[i].z = xyz[3 * i + 2];
        cloud->points[i].r = rgb[3 * i + 0]; cloud->points[i].g = rgb[3 * i + 1]; cloud->points[i].b = rgb[3 * i + 2];
    }
    return convertPointCloudXYZRGBToBuffer(cloud, shorts_out);
}

#ifdef PCS_REF_CENTRE_OPT
/* One camera through pcs-multicamera-optimized's frame: updateCloudXYZRGB (read the frame, decode, pcl::transformPointCloud with
 * transform[0] = m16 row-major), *stitched += *cloud, send_stitchedXYZRGB. `wire` = the camera's [int32 size][records]. Returns the
 * bytes the reference wrote to the consumer (header included), copied to `out`; -1 for a frame the harness refuses (malformed, too
 * large for BUF_SIZE, or n_points % downsample != 0, see pcs_refc_decode), -2 when `out` is too small. */
long pcs_refc_update_and_send(const unsigned char* wire, size_t wire_len, const float* m16, int ds, unsigned char* out, size_t out_cap)
{
    int n_points;
    if (ds < 1 || !wire_ok(wire, wire_len, &n_points) || n_points % ds != 0) return -1;
    if (!stitched_buf) stitched_buf = (short*)malloc(sizeof(short) * STITCHED_BUF_SIZE);
    if (!stitched_buf) return -1;
    downsample = ds;
    timer = false;
    for (int i = 0; i < 16; i++) transform[0].m[i] = m16[i];
    Wire w;
    if (!wire_open(w, (const char*)wire, wire_len)) return -1;
    {
        pointCloudXYZRGB::Ptr cloud(new pointCloudXYZRGB);
        pointCloudXYZRGB::Ptr stitched_cloud(new pointCloudXYZRGB);
        updateCloudXYZRGB(0, sockfd_array[0], cloud);
        *stitched_cloud += *cloud;
        send_stitchedXYZRGB(stitched_cloud);
    }
    return wire_close(w, out, out_cap);
}
#endif

#ifdef PCS_REF_CENTRE_CLIENT
/* One camera through pcs-multicamera-client's frame: sendStitchToUnity (readCloud, the `j += 5 * downsample` loop, the header, the
 * write). Any n_points is legal here. Returns as pcs_refc_update_and_send. */
long pcs_refc_stitch(const unsigned char* wire, size_t wire_len, int ds, unsigned char* out, size_t out_cap)
{
    int n_points;
    if (ds < 1 || !wire_ok(wire, wire_len, &n_points)) return -1;
    if (!stitched_buf) stitched_buf = (short*)malloc(sizeof(short) * STITCHED_BUF_SIZE);
    if (!pc_buf[0]) pc_buf[0] = (short*)malloc(sizeof(short) * BUF_SIZE);
    if (!stitched_buf || !pc_buf[0]) return -1;
    downsample = ds;
    timer = false;
    Wire w;
    if (!wire_open(w, (const char*)wire, wire_len)) return -1;
    sendStitchToUnity();
    return wire_close(w, out, out_cap);
}
#endif

}  // extern "C"
