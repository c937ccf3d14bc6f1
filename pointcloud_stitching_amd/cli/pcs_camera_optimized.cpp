// pcs-camera-optimized (MI355X) — work-alike of the reference's edge benchmark/server
// (src/pcs-camera-optimized.cpp) on top of libpcs_hip.so. Host code only: getopt surface, frame loop,
// timing, stdout lines and the TCP push are kept; the per-frame work goes through the C ABI.
//
//   reference flags (getopt "hf:vst:cmz", :122):  -h  -f <file>  -v  -s  -t <n>  -c  -m  -z
//     -z is a TODO in the reference (its snappy call is commented out, :145-147, 333-337, 699-709); here it compresses the stitched
//     payload on the GPU, losslessly (pcs_process_frames_compressed, the PCZ1 container of DESIGN.md section 4): what -s / -P send
//     and -o dumps is [int32 container bytes][container], and the summary's byte figures are the container's
//   additions:  -g <dev>  -n <streams>  -d <stride>  -i (drop invalid depth)  -C (-c without the reference's lane quirk)
//               -r <frames>  -o <file> (dump last stitched buffer)  -p <port>
//               -e <file> (camera-to-world matrices instead of the ones pasted into the reference's sources)
//               -H (texture coordinates as older librealsense releases computed them: (pixel + 0.5) / size)
//               -B <xlo,xhi,ylo,yhi,zlo,zhi> (crop box in millimetres, world frame, inclusive: an edge that crops before it sends;
//                  pcs_set_crop_box_mm; needs -m)
//               -F <temporal[=alpha:delta:persistence],holes[=left]> (depth pre-filter on the GPU: the two librealsense blocks the
//                  reference leaves as TODOs in sendXYZRGBPointcloud, :682-684; pcs_set_depth_filter)
//               -D <n> (depth decimation on the GPU, ahead of -F as in librealsense's chain: every n x n block of the Z16 raster to
//                  one pixel, median of the valid for n = 2, 3, mean of the valid for n = 4..8; 1 = off; pcs_decimate_depth. The
//                  definition is this project's own; parity with librealsense unpinned)
//               -S <alpha:delta:iterations[:radius] | default> (spatial edge-preserving filter on the GPU, after -D and ahead of -F as in
//                  librealsense's chain: a recursive smoother along every row and column that stops at depth steps larger than delta;
//                  pcs_spatial_filter_depth. This project's own definition; parity with librealsense unpinned)
//
//   -f takes "synth:<W>x<H>" (deterministic synthetic frames; the reference's bags are LFS stubs and
//   need librealsense), a .pcsraw dump (see pointcloud_stitching_amd/synthetic.py: write_pcsraw) or a
//   librealsense recording (.bag, read by pcs_bag.h — validated only against this repo's own writer).
//   Without -f the reference grabs from a live RealSense camera; that needs librealsense and a camera,
//   neither of which this build has: it says so and exits non-zero.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <getopt.h>
#include <signal.h>
#include <sys/socket.h>
#include <unistd.h>

#include "pcs_bag.h"
#include "pcs_cropbox.h"
#include "pcs_decimate.h"
#include "pcs_depthfilter.h"
#include "pcs_spatialfilter.h"
#include "pcs_synth.h"
#include "pcs_wire.h"

typedef std::chrono::high_resolution_clock clockTime;
typedef std::chrono::duration<double, std::milli> timeMilli;

static const char* filename = nullptr;
static bool display_updates = false, send_buffer = false, cutoff = false, use_hip = false, compress = false;
static bool cutoff_compat = false, drop_invalid = false, pull_mode = false, half_pixel = false, pageable = false;
static int num_of_threads = 1, device = 0, n_streams = 1, downsample = 1, max_frames = 60, port = 8000;
static const char* dump_path = nullptr;
static const char* extrinsics_path = nullptr;
static bool crop = false;
static int16_t crop_lo[3], crop_hi[3];
static bool depth_filter = false;
static pcs_depth_filter_config filter_cfg;
static int decimate = 1;
static bool spatial_filter = false;
static pcs_spatial_filter_config spatial_cfg;
static int client_sock = 0, sockfd = 0;

static void print_usage()
{
    printf("\nUsage: pcs-camera-optimized -f <synth:WxH | frames.pcsraw | recording.bag> [-m] [-t n] [-c] [-s] [-n streams] [-g gpu]\n"
           "  -f <src>  frame source (synthetic generator or raw dump)\n"
           "  -s        send data to central camera server if available (TCP push on port 8000)\n"
           "  -m        the reference's SIMD arithmetic; without it, its default scalar arithmetic - both on the GPU\n"
           "  -t <n>    OpenMP threads of the reference path; accepted, inert on the HIP path\n"
           "  -c        cutoff 0<z<=1.5, -2<x<=2 with compaction, exactly as the reference's -c -m computes it (point k of an\n"
           "            aligned group of four is gated by point 3-k's test)   -C  every point by its own test\n"
           "            without -m, the default loop's -c: z != 0, x != 0, z <= 1.5, nothing compacted (a skipped point is a zero record)\n"
           "  -i        drop invalid-depth pixels   -d <n> keep every n-th point   -n <N> camera streams\n"
           "  -g <dev>  GPU ordinal   -r <frames>   -o <file> dump last stitched buffer   -p <port>\n"
           "  -z        compress the payload on the GPU (lossless PCZ1 container, DESIGN.md section 4): -s / -P send and -o dumps\n"
           "            [int32 container bytes][container]; the centre decodes it with its own -z\n"
           "  -P        serve frames on 'Z' pull requests (the live server's protocol) instead of pushing them\n"
           "  -e <file> camera-to-world matrices, 16 row-major floats per line (python -m pointcloud_stitching_amd.calibration)\n"
           "  -H        texture coordinates as older librealsense releases: (pixel + 0.5) / size\n"
           "  -B <xlo,xhi,ylo,yhi,zlo,zhi>  crop box: keep the points inside these inclusive bounds, millimetres in the WORLD frame\n"
           "            (after the camera-to-world transform; ANDed with -c / -i; -d keeps every n-th KEPT point); needs -m\n"
           "  -F <temporal[=alpha:delta:persistence],holes[=left]>  depth pre-filter on the GPU, inside the timed region: temporal\n"
           "            smoothing (defaults 0.4:20:3 = librealsense's) and / or hole filling from the left, e.g. -F temporal=0.4:20:3,holes\n"
           "  -D <n>    depth decimation on the GPU, inside the timed region and ahead of -F: every n x n block of the depth raster to one\n"
           "            pixel (n = 2, 3: median of the valid pixels; n = 4..8: their mean; 1 = off); everything downstream sees the\n"
           "            smaller cloud, the colour image stays as it is\n"
           "  -S <alpha:delta:iterations[:radius] | default>  spatial edge-preserving depth filter on the GPU, inside the timed region,\n"
           "            after -D and ahead of -F: every row and every column is smoothed recursively in both directions, `iterations`\n"
           "            times; a step between neighbours larger than delta (Z16 units) is kept as an edge; radius > 0 also fills up to\n"
           "            that many zero pixels per gap and direction along the rows (default = 0.5:20:2, no fill)\n"
           "  -M        hand the frames over in ordinary pageable memory, as librealsense owns them in the reference's timed region\n"
           "            (:291-293): uploads are staged then. Default: frames copied to page-locked rasters BEFORE the timer starts\n"
           "            (zero copy) - the printed times then belong to a capture pipeline that delivers page-locked frames\n\n");
}

static void parseArgs(int argc, char** argv)
{
    int c;
    while ((c = getopt(argc, argv, "hf:vst:cmzg:n:d:iCr:o:p:e:PHMB:F:D:S:")) != -1) {
        switch (c) {
            case 'h': print_usage(); exit(0);
            case 'f': filename = optarg; break;
            case 'v': display_updates = true; break;
            case 's': send_buffer = true; break;
            case 't': num_of_threads = atoi(optarg); break;
            case 'c': cutoff = true; cutoff_compat = true; break;     // the reference's -c -m payload, lane quirk included (:501-502, 519)
            case 'C': cutoff = true; cutoff_compat = false; break;    // every point by its own range test
            case 'H': half_pixel = true; break;
            case 'm': use_hip = true; break;
            case 'z': compress = true; break;
            case 'g': device = atoi(optarg); break;
            case 'n': n_streams = atoi(optarg); break;
            case 'd': downsample = atoi(optarg); break;
            case 'i': drop_invalid = true; break;
            case 'r': max_frames = atoi(optarg); break;
            case 'o': dump_path = optarg; break;
            case 'p': port = atoi(optarg); break;
            case 'e': extrinsics_path = optarg; break;
            case 'P': pull_mode = true; send_buffer = true; break;
            case 'M': pageable = true; break;
            case 'B': {
                std::string why;
                if (!pcs_cropbox::parse(optarg, crop_lo, crop_hi, why)) { std::cerr << "-B " << optarg << ": " << why << std::endl; exit(2); }
                crop = true;
                break;
            }
            case 'F': {
                std::string why;
                if (!pcs_depthfilter::parse(optarg, filter_cfg, why)) { std::cerr << "-F " << optarg << ": " << why << std::endl; exit(2); }
                depth_filter = true;
                break;
            }
            case 'D': {
                std::string why;
                if (!pcs_decimate::parse(optarg, decimate, why)) { std::cerr << "-D " << optarg << ": " << why << std::endl; exit(2); }
                break;
            }
            case 'S': {
                std::string why;
                if (!pcs_spatialfilter::parse(optarg, spatial_cfg, why)) { std::cerr << "-S " << optarg << ": " << why << std::endl; exit(2); }
                spatial_filter = true;
                break;
            }
            default: print_usage(); exit(2);
        }
    }
}

// One consumer per edge server, as in the reference (:75-105): listen on the port, take the first client.
static bool openServer(int p)
{
    sockfd = pcs_wire::listen_on(p);
    if (sockfd < 0) { std::cerr << "\ncannot listen on port " << p << std::endl; return false; }
    std::cout << "Waiting for client..." << std::endl;
    client_sock = ::accept(sockfd, nullptr, nullptr);
    if (client_sock < 0) { std::cerr << "\nConnection failed" << std::endl; return false; }
    std::cout << "Established connection with client_sock: " << client_sock << std::endl;
    return true;
}

static void sigintHandler(int) { std::cout << "\n Exiting \n " << std::endl; exit(0); }

struct FrameSource {
    std::vector<pcs_stream_config> cfg;
    std::vector<std::vector<uint16_t>> depth;     // per stream, current frame
    std::vector<std::vector<uint8_t>> color;
    FILE* fp = nullptr;
    int frames_in_file = 0, W = 0, H = 0;
    bool synth = false, bag = false;
    pcs_bag::Recording rec;            // -f <recording.bag>: librealsense ROS bag (what the reference plays, :168-176)

    bool open(const char* spec)
    {
        if (strncmp(spec, "synth:", 6) == 0) {
            if (sscanf(spec + 6, "%dx%d", &W, &H) != 2 || W <= 0 || H <= 0) return false;
            synth = true;
            for (int s = 0; s < n_streams; s++) cfg.push_back(pcs_synth::stream_config(W, H, s, n_streams == 1));
        } else if (strlen(spec) > 4 && strcmp(spec + strlen(spec) - 4, ".bag") == 0) {
            std::string err;
            if (!rec.open(spec, err)) { std::cerr << spec << ": " << err << std::endl; return false; }
            bag = true; n_streams = 1; frames_in_file = rec.frames;
            cfg.push_back(rec.config);
            memcpy(cfg[0].cam_to_world, pcs_synth::stream_config(8, 8, 0, true).cam_to_world, sizeof cfg[0].cam_to_world);   // tf_mat :64-67
            W = cfg[0].depth.width; H = cfg[0].depth.height;
        } else {
            fp = fopen(spec, "rb");
            if (!fp) return false;
            char magic[8]; int32_t ns = 0, nf = 0;
            if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, "PCSRAW1", 8) != 0) return false;
            if (fread(&ns, 4, 1, fp) != 1 || fread(&nf, 4, 1, fp) != 1 || ns < 1 || ns > PCS_MAX_STREAMS) return false;
            n_streams = ns; frames_in_file = nf;
            cfg.resize(ns);
            if (fread(cfg.data(), sizeof(pcs_stream_config), ns, fp) != (size_t)ns) return false;
            W = cfg[0].depth.width; H = cfg[0].depth.height;
        }
        depth.resize(n_streams); color.resize(n_streams);
        return true;
    }
    // frame `frame` is the source's first frame again: a .pcsraw / .bag that loops (a synthetic source never repeats)
    bool at_first_frame(int frame) const { return !synth && frames_in_file > 0 && frame % frames_in_file == 0; }
    bool next(int frame)
    {
        if (synth) {
            for (int s = 0; s < n_streams; s++) {
                pcs_synth::depth(W, H, s, pcs_synth::kSeed + 7919u * (uint32_t)frame, depth[s]);
                pcs_synth::color(W, H, s, pcs_synth::kSeed + 7919u * (uint32_t)frame, color[s]);
            }
            return true;
        }
        if (frame >= frames_in_file) return false;          // the reference stops when the bag loops (:276)
        if (bag) {
            std::string err;
            if (!rec.read(frame, depth[0], color[0], err)) { std::cerr << "frame " << frame << ": " << err << std::endl; return false; }
            return true;
        }
        for (int s = 0; s < n_streams; s++) {
            depth[s].resize((size_t)cfg[s].depth.width * cfg[s].depth.height);
            color[s].resize((size_t)cfg[s].color_stride * cfg[s].color.height);
            if (fread(depth[s].data(), 2, depth[s].size(), fp) != depth[s].size()) return false;
            if (fread(color[s].data(), 1, color[s].size(), fp) != color[s].size()) return false;
        }
        return true;
    }
};

int main(int argc, char** argv)
{
    parseArgs(argc, argv);
    signal(SIGINT, sigintHandler);
    if (filename == NULL) {
        std::cerr << "Live capture needs librealsense2 and a RealSense camera, which this build does not link.\n"
                     "Use -f synth:<W>x<H>, -f <frames.pcsraw> or -f <recording.bag>." << std::endl;
        return 2;
    }
    if (crop && !use_hip) { std::cerr << "-B needs -m: the reference's default loop (no -m) has no crop" << std::endl; return 2; }
    std::cout << "Reading Frames from File: " << filename << std::endl;
    FrameSource src;
    if (!src.open(filename)) { std::cerr << "cannot open frame source " << filename << std::endl; return 2; }
    std::cout << "Camera Info: synthetic D400-like stream x" << n_streams << " FW ver:n/a" << std::endl;
    if (num_of_threads) std::cout << "OpenMP Threads: " << num_of_threads << std::endl;

    if (extrinsics_path) {      // replaces editing tf_mat / transform[i] in source (:64-67)
        FILE* f = fopen(extrinsics_path, "r");
        if (!f) { std::cerr << "cannot open extrinsics file " << extrinsics_path << std::endl; return 2; }
        char line[1024];
        int cam = 0;
        while (cam < n_streams && fgets(line, sizeof line, f)) {
            char* hash = strchr(line, '#');
            if (hash) *hash = 0;
            float m[16];
            int got = 0, pos = 0, adv = 0;
            while (got < 16 && sscanf(line + pos, " %f%n", &m[got], &adv) == 1) { got++; pos += adv; if (line[pos] == ',') pos++; }
            if (got == 0) continue;
            if (got != 16) { std::cerr << extrinsics_path << ": expected 16 values per line" << std::endl; return 2; }
            memcpy(src.cfg[cam++].cam_to_world, m, sizeof m);
        }
        fclose(f);
        if (cam < n_streams) { std::cerr << extrinsics_path << ": only " << cam << " matrices for " << n_streams << " streams" << std::endl; return 2; }
    }

    // -D: the context is created from the decimated streams; the source's own sizes go to pcs_decimate_depth with every frame
    std::vector<pcs_stream_config> ctx_cfg = src.cfg;
    std::vector<int32_t> src_w(n_streams), src_h(n_streams);
    for (int s = 0; s < n_streams; s++) {
        src_w[s] = src.cfg[s].depth.width; src_h[s] = src.cfg[s].depth.height;
        if (decimate > 1 && pcs_decimated_stream_config(&src.cfg[s], decimate, &ctx_cfg[s]) != PCS_OK) {
            std::cerr << "-D " << decimate << ": stream " << s << ": " << pcs_last_error(nullptr) << std::endl; return 2;
        }
    }

    pcs_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.device = device; cfg.n_streams = n_streams; cfg.streams = ctx_cfg.data(); cfg.downsample = downsample;
    cfg.flags = (cutoff ? PCS_FLAG_CUTOFF : 0u) | (cutoff_compat ? PCS_FLAG_CUTOFF_COMPAT : 0u) | (drop_invalid ? PCS_FLAG_DROP_INVALID : 0u) |
                (half_pixel ? PCS_FLAG_TEXCOORD_HALF_PIXEL : 0u) |
                (use_hip ? 0u : PCS_FLAG_SCALAR_ARITH);      // no -m: copyPointCloudXYZRGBToBuffer's arithmetic (:620-667, 688-694)
    pcs_ctx* ctx = nullptr;
    int rc = pcs_create(&ctx, &cfg);
    if (rc != PCS_OK) { std::cerr << "pcs_create: " << pcs_strerror(rc) << ": " << pcs_last_error(nullptr) << std::endl; return 1; }

    if (crop && (rc = pcs_set_crop_box_mm(ctx, crop_lo, crop_hi)) != PCS_OK) {
        std::cerr << "pcs_set_crop_box_mm: " << pcs_strerror(rc) << ": " << pcs_last_error(ctx) << std::endl; return 1;
    }

    if (depth_filter && (rc = pcs_set_depth_filter(ctx, &filter_cfg)) != PCS_OK) {
        std::cerr << "pcs_set_depth_filter: " << pcs_strerror(rc) << ": " << pcs_last_error(ctx) << std::endl; return 1;
    }

    const size_t buf_shorts = PCS_HEADER_SHORTS + pcs_max_payload_shorts(ctx);
    short* buffer = nullptr;                                               // the reference mallocs BUF_SIZE shorts (:157);
    if (pcs_host_malloc(ctx, (void**)&buffer, sizeof(short) * buf_shorts) != PCS_OK) {   // page-locked: D2H at link speed
        std::cerr << pcs_last_error(ctx) << std::endl; return 1;
    }
    // -z: what is sent instead, [int32 container bytes][PCZ1 container] (pcs_process_frames_compressed), sized for the worst case
    const size_t zbuf_bytes = sizeof(int32_t) + pcs_compressed_bound((int)(pcs_max_payload_shorts(ctx) / PCS_POINT_SHORTS));
    short* zbuffer = nullptr;
    if (compress && pcs_host_malloc(ctx, (void**)&zbuffer, zbuf_bytes) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
    short* const wire = compress ? zbuffer : buffer;
    std::vector<const uint16_t*> dptr(n_streams);
    std::vector<uint16_t*> fptr(n_streams);           // -S, -F: the same rasters, filtered in place
    std::vector<const uint8_t*> cptr(n_streams);
    std::vector<int> counts(n_streams);
    pcs_kernel_timing(ctx, 1);
    // The frames are handed over in page-locked rasters (as a capture pipeline that owns its buffers would deliver them):
    // with the buffer above page-locked too, pcs_process_frames runs zero copy. Filling them is the frame source's job
    // and, like the reference's wait_for_frames / pointcloud::calculate, outside the timed region (:291-293).
    std::vector<uint16_t*> pin_d(n_streams, nullptr);
    std::vector<uint8_t*> pin_c(n_streams, nullptr);
    std::vector<size_t> pin_db(n_streams, 0), pin_cb(n_streams, 0);
    // -D: the decimated rasters (page-locked like the frames, pageable under -M); what -F and the stitch then read
    std::vector<uint16_t*> dec_d(n_streams, nullptr);
    std::vector<std::vector<uint16_t>> dec_pageable(n_streams);
    std::vector<const uint16_t*> sptr(n_streams);     // -D: the source rasters
    for (int s = 0; decimate > 1 && s < n_streams; s++) {
        const size_t px = (size_t)ctx_cfg[s].depth.width * ctx_cfg[s].depth.height;
        if (pageable) { dec_pageable[s].resize(px); dec_d[s] = dec_pageable[s].data(); }
        else if (pcs_host_malloc(ctx, (void**)&dec_d[s], px * sizeof(uint16_t)) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
    }

    int i = 0, buff_size = 0;
    double duration_sum = 0, buff_size_sum = 0;
    size_t points_in = 0;
    if (send_buffer && !openServer(port)) return 1;

    while (i < max_frames && src.next(i)) {
        i++;
        for (int s = 0; s < n_streams; s++) {
            const size_t db = src.depth[s].size() * sizeof(uint16_t), cb = src.color[s].size();
            if (!pageable && db > pin_db[s]) {
                if (pin_d[s]) pcs_host_free(ctx, pin_d[s]);
                if (pcs_host_malloc(ctx, (void**)&pin_d[s], db) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                pin_db[s] = db;
            }
            if (!pageable && cb > pin_cb[s]) {
                if (pin_c[s]) pcs_host_free(ctx, pin_c[s]);
                if (pcs_host_malloc(ctx, (void**)&pin_c[s], cb) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                pin_cb[s] = cb;
            }
            if (pageable) {       // -M: the frame source's own (pageable) memory goes straight in, like librealsense's frames do
                dptr[s] = fptr[s] = src.depth[s].data(); cptr[s] = src.color[s].data();
                continue;
            }
            memcpy(pin_d[s], src.depth[s].data(), db);
            memcpy(pin_c[s], src.color[s].data(), cb);
            dptr[s] = fptr[s] = pin_d[s]; cptr[s] = pin_c[s];
        }
        if (decimate > 1)
            for (int s = 0; s < n_streams; s++) { sptr[s] = dptr[s]; dptr[s] = fptr[s] = dec_d[s]; }
        // A source that loops back to its first frame is a scene cut for the temporal state. (As the reference, :276, this program
        // stops where a recording ends, so no source reaches this today; one that loops resets here.)
        if (depth_filter && src.at_first_frame(i - 1) && i > 1 && (rc = pcs_reset_depth_filter(ctx)) != PCS_OK) {
            std::cerr << "pcs_reset_depth_filter: " << pcs_last_error(ctx) << std::endl; return 1;
        }
        auto time_start = clockTime::now();                                   // :291
        if (decimate > 1 && (rc = pcs_decimate_depth(ctx, decimate, src_w.data(), src_h.data(), sptr.data(), fptr.data())) != PCS_OK) {
            std::cerr << "pcs_decimate_depth: " << pcs_last_error(ctx) << std::endl; return 1;
        }
        if (spatial_filter && (rc = pcs_spatial_filter_depth(ctx, &spatial_cfg, dptr.data(), fptr.data())) != PCS_OK) {
            std::cerr << "pcs_spatial_filter_depth: " << pcs_last_error(ctx) << std::endl; return 1;
        }
        if (depth_filter && (rc = pcs_filter_depth(ctx, dptr.data(), fptr.data())) != PCS_OK) {
            std::cerr << "pcs_filter_depth: " << pcs_last_error(ctx) << std::endl; return 1;
        }
        if (compress)       // the payload stays on the device and is compressed there: buff_size is the container's
            rc = pcs_process_frames_compressed(ctx, dptr.data(), cptr.data(), zbuffer, zbuf_bytes, 1, counts.data(), &buff_size);
        else
            rc = pcs_process_frames(ctx, dptr.data(), cptr.data(), buffer, buf_shorts, send_buffer ? 1 : 0, counts.data(), &buff_size);
        auto time_end = clockTime::now();                                     // :293
        if (rc != PCS_OK) { std::cerr << (compress ? "pcs_process_frames_compressed: " : "pcs_process_frames: ") << pcs_last_error(ctx) << std::endl; return 1; }
        if (pull_mode) {      // the live server's protocol (:180-184): one 'Z' per frame, anything else is fatal
            int req = pcs_wire::recv_pull(client_sock);
            if (req < 0) { std::cout << "Client disconnected" << std::endl; break; }
            if (req != pcs_wire::kPullXYZRGB) { std::cerr << "Faulty pull request" << std::endl; return 1; }
        }
        if (send_buffer && !pcs_wire::send_frame(client_sock, wire, buff_size)) { std::cout << "Client disconnected" << std::endl; break; }   // :719
        const double ms = timeMilli(time_end - time_start).count();
        std::cout << "Frame Time: " << ms << " ms " << "FPS: " << 1000.0 / ms
                  << "\t Buffer size: " << float(buff_size) / (1 << 20) << " MBytes" << std::endl;       // :295-297
        duration_sum += ms;
        buff_size_sum += buff_size;
        for (int s = 0; s < n_streams; s++) points_in += (size_t)pcs_stream_points(ctx, s);
    }
    if (send_buffer) { close(client_sock); close(sockfd); }
    if (i == 0) { std::cerr << "no frames" << std::endl; return 1; }

    std::vector<float> kms(i);
    int nk = 0;
    pcs_kernel_times_ms(ctx, kms.data(), i, &nk);
    double ksum = 0; for (int k = 0; k < nk && k < i; k++) ksum += kms[k];
    const double kavg = nk ? ksum / (nk < i ? nk : i) : 0.0;
    const size_t pts = points_in / i;

    // summary block — same lines as :317-342
    std::cout << "\n### Video Frames H x W : " << ctx_cfg[0].color.height << " x " << ctx_cfg[0].color.width << std::endl;
    std::cout << "### Depth Frames H x W : " << ctx_cfg[0].depth.height << " x " << ctx_cfg[0].depth.width << std::endl;
    if (decimate > 1) std::cout << "### Depth decimation : " << decimate << " x " << decimate << " (source " << src_h[0] << " x " << src_w[0] << ")" << std::endl;
    std::cout << "### # Points : " << pts << std::endl;
    std::cout << "\n### Total Frames = " << i << std::endl;
    std::cout << "### AVG Frame Time: " << duration_sum / i << " ms" << std::endl;
    std::cout << "### AVG FPS: " << 1000.0 / (duration_sum / i) << std::endl;
    if (num_of_threads) std::cout << "### OpenMP Threads : " << num_of_threads << std::endl;
    else std::cout << "### Running Serialized" << std::endl;
    if (compress) {
        std::cout << "\n### Sending Compressed Stream" << std::endl;
        std::cout << "### AVG Bytes/Frame: " << float(buff_size_sum) / (i * 1000000.0) << " MBytes" << std::endl;
        std::cout << "### AVG Compression Ratio " << float(buff_size_sum) / ((pts / 100.0) * 5 * sizeof(short) * i) << " %" << std::endl;
    } else {
        std::cout << "\n### AVG Bytes/Frame: " << float(buff_size_sum) / (i * 1000000.0) << " MBytes" << std::endl;
        std::cout << "### AVG Filter Compress Ratio " << float(buff_size_sum) / ((pts / 100.0) * 5 * sizeof(short) * i) << " %" << std::endl;
    }
    // additions
    std::cout << "\n### HIP streams : " << n_streams << " on GPU " << device << " (arithmetic policy " << pcs_stream_math(ctx, 0) << ")" << std::endl;
    // every buffer handed to pcs_process_frames is page-locked, so unless PCS_ZERO_COPY=0 the kernels read the rasters and
    // write the payload over PCIe themselves: their time then is a link figure, not an HBM one
    const char* zc_env = getenv("PCS_ZERO_COPY");
    const bool zero_copy = !(zc_env && atoi(zc_env) == 0) && !pageable;
    std::cout << "### Frame hand-over : " << (pageable ? "pageable rasters (-M): staged uploads inside the timed region, as the reference's frames"
                                                       : "page-locked rasters filled before the timer starts (zero copy)") << std::endl;
    if (zero_copy) {
        std::cout << "### AVG Kernel Time: " << kavg << " ms  (hipEvent; zero copy: rasters read from and payload written to host memory over PCIe)" << std::endl;
        if (kavg > 0)
            std::cout << "### Kernel PCIe GB/s (15 B/point, both directions): " << pts * 15.0 / kavg / 1e6 << std::endl;
    } else {
        std::cout << "### AVG Kernel Time: " << kavg << " ms  (hipEvent, deproject+transform+pack only)" << std::endl;
        if (kavg > 0) {
            std::cout << "### Kernel Mpoints/s: " << pts / kavg / 1e3 << std::endl;
            std::cout << "### Kernel HBM GB/s (15 B/point algorithmic): " << pts * 15.0 / kavg / 1e6
                      << "  = " << pts * 15.0 / kavg / 1e6 / 80.0 << " % of 8 TB/s" << std::endl;
        }
    }
    std::cout << "### Host-API Mpoints/s (PCIe both ways included): " << pts / (duration_sum / i) / 1e3 << std::endl;

    if (dump_path) {
        FILE* f = fopen(dump_path, "wb");
        if (f) { fwrite(wire, 1, (size_t)buff_size + 4, f); fclose(f); }
    }
    pcs_host_free(ctx, buffer);
    if (zbuffer) pcs_host_free(ctx, zbuffer);
    for (int s = 0; s < n_streams; s++) { if (pin_d[s]) pcs_host_free(ctx, pin_d[s]); if (pin_c[s]) pcs_host_free(ctx, pin_c[s]); }
    for (int s = 0; !pageable && s < n_streams; s++) if (dec_d[s]) pcs_host_free(ctx, dec_d[s]);
    pcs_destroy(ctx);
    return 0;
}
