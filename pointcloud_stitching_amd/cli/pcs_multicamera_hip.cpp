// pcs-multicamera-optimized — the central stitcher (src/pcs-multicamera-optimized.cpp / pcs-multicamera-client.cpp,
// non-visual path) on MI355X. Installed under the reference's program name; `pcs-multicamera-hip` is a link to it.
//
// Two ways to feed it:
//   -i synth:<W>x<H> | frames.pcsraw   all cameras' rasters are on this node: ONE fused launch produces the
//                                       stitched buffer (edge + central collapsed)
//   -c host:port[,host:port...]         existing edge servers (the reference's, or pcs-camera-optimized -s):
//                                       one reader thread per camera like readCloud (:363-371); payloads are
//                                       concatenated on the GPU with the stride -d (sendStitchToUnity :373-395)
// The stitched cloud is served exactly like the reference: wait for 'Z' on port 9000, write
// [int32 bytes][points] (:397-403). -t prints the running average like runStitching (:417-430).
//
//   reference flags (getopt "hftsvd:n", src/pcs-multicamera-optimized.cpp:90): -h -f -t -s -v -d <n> -n
//     -f is the reference's boolean "fast" switch (:96-98; it only dropped colour in the PCL viewer): accepted, inert,
//     with a one-line notice — an existing `-f -t -d2` invocation keeps working. -s (save PLY), -v (PCL visualiser)
//     and -n belong to the PCL viewer, which this build does not have: refused with a reason.
//   additions: -i <src>  -c <list>  -N <streams>  -g <gpu>  -p <serve port>  -r <frame-sets>  -o <file>  -q (no server)
//              -G <n>  shard the cameras of -i over n GPUs: libpcs_node (ncclCommInitAll + one grouped send/recv to GPU 0)
//              -G <id,id,...>  the same with explicit device ids, one per peer; an id that repeats makes virtual peers of one GPU
//                      (their transfers are RCCL self send/recv pairs): `-G 0,0,0,0` runs the 4-GPU flow on a one-GPU box
//              -V <mm> serve the voxel-grid downsample (leaf in mm, BASELINE config 5) of the stitched cloud instead of the
//                      cloud itself: with -i one device call from the rasters (pcs_process_frames_voxel_device), with -c the
//                      voxel grid of the concatenated payloads;  -Z  drop invalid-depth pixels (PCS_FLAG_DROP_INVALID, -i only)
//              -G <n> -V <mm>  BASELINE configs[4]: cameras sharded over n GPUs, per-GPU voxel partials, one RCCL exchange, sort +
//                      segmented mean on GPU 0 (libpcs_node: pcs_node_process_voxel); -R payloads gathers the packed payloads instead
//              -P      (with -G and -i synth:) the frame loop of a node whose rasters are already on their GPUs: a ring of synthetic
//                      frame-sets is uploaded once, then pcs_node_submit_device(k+1); pcs_node_wait(k) (with -V: the voxel
//                      tickets) keeps two frame-sets in flight for -r iterations; prints the period per frame-set and where a
//                      frame-set's time went on GPU 0 (pcs_node_last_stats). -o dumps the last frame-set like the other modes.
//              -T <file>  (with -c) what the reference's pcs-multicamera-optimized does and pcs-multicamera-client does not: every
//                      camera's payload is decoded to metres, moved by transform[i] (line i of the file: 16 values, row-major,
//                      the format of pcs-camera-optimized -e) and re-encoded before the concatenation
//                      (src/pcs-multicamera-optimized.cpp:226-265, 289; pcs_transform_payloads_device). Lossy, like the
//                      reference's round trip; default off = pcs-multicamera-client's lossless concatenation.
//              -B <xlo,xhi,ylo,yhi,zlo,zhi>  crop box in millimetres, world frame, inclusive (pcs_set_crop_box_mm): with -i the fused
//                      path crops (with -V the cropped payload goes to pcs_voxel_grid_device_counted); with -c the received
//                      payloads are cropped on the GPU (pcs_crop_payloads_device, after -T if both are given; -d is the crop
//                      call's stride: every d-th KEPT record per camera). Not with -G: the node library has no setter.
//              -z      (with -c) the edges run pcs-camera-optimized -z: every frame is a PCZ1 container, validated
//                      on the host and decoded on the GPU into the camera's device payload (pcs_decompress_payload) ahead of the
//                      stitch / -T / -B / -V paths, which see what they always saw; a frame that fails validation ends the run with
//                      the validator's message. What is served on -p stays raw.
//              -X learn:<file>,<cell_mm>[,<max_cells>]  learn the background of a fixed rig (pcs_background_learn_device, counted where the
//                      cloud's count is on the device — the chain's own rule): every frame-set of the run, as it enters the chain (after
//                      -T and -B / -d), marks the cells of edge cell_mm it touches in a model of at most max_cells cells (default
//                      4194304); the frame-sets pass on unchanged. When the run ends <file> gets the model as a PCB1 container
//                       and -t prints `Background learned: <frames> frame-sets, <cells> cells of <cell_mm> mm`. A
//                      scene with more cells than max_cells ends the run with status 1 and no file.
//              -X <file>[,<min_percent>[,<dilate>]]  background subtraction (pcs_background_subtract_device): the chain's first stage, in
//                      front of -O. <file> is validated (pcs_background_validate: a refusal is a usage error that names what it found)
//                      and imported at start-up; a record goes iff its cell — with dilate 1 (default) one of the 27 around it — was seen
//                      in min_seen = max(1, ceil(frames x min_percent / 100)) of the learned frame-sets (min_percent 1..100, default 50).
//                      -t prints `Background subtraction: <in> -> <kept> points (<cells> cells, seen >= <min_seen> of <frames>, dilate
//                      <d>)`. One run takes one form of -X, once. Not with -G: the node library has no background model.
//              -O -K -M -E  the post-stitch filters, one chain (pcs_filter_chain.h) in that fixed order, after -T and -B / -d, before -V. A
//                      stage reads the output of the stage in front of it: through the counted form, with that stage's count word,
//                      wherever the count is on the device (every -i payload, every stage behind another), else through the plain
//                      form with the host's count. No count leaves the device in between; the last one is fetched only when no -V
//                      reads it there (pcs_voxel_grid_device_counted). With -c the chain runs on the stitched device payload; with -i
//                      the payload is built on the device (pcs_process_frames_device). -t prints each stage's line(s) per frame-set,
//                      in stage order. None with -G: the node library has no such filters.
//              -O <radius_mm,min_neighbors>  radius outlier removal on the stitched cloud (pcs_radius_outlier_device: a record stays iff
//                      at least min_neighbors others lie within radius_mm of it). -t prints `Outlier removal: <in> -> <kept> points`.
//                      The filter knows nothing of invalid depth: with -i give -Z (or -B).
//              -K <mean_k,std_mul_milli,max_dist_mm>  statistical outlier removal on the stitched cloud (pcs_stat_outlier_device: a
//                      record stays iff it has mean_k others within max_dist_mm and the summed distance to the nearest mean_k is at
//                      most the cloud's mean + std_mul_milli / 1000 deviations). -t prints `Statistical outlier removal: <in> ->
//                      <kept> points (dense <M>, threshold <T>/256 per k)`. Zero-depth pixels sit on one point and drag the mean
//                      down: with -i give -Z (or -B).
//              -M <distance_mm,iterations[,min_inliers[,max_planes[,seed]]]>  plane segmentation on the stitched cloud
//                      (pcs_plane_segment_device, mode 0: up to max_planes rounds, each takes the plane through three drawn records that
//                      has the most records within distance_mm, out of `iterations` such planes, out of the cloud while it has
//                      min_inliers records; defaults 3, 1 and seed 1). -t prints `Plane segmentation: <in> -> <kept> points (<planes>
//                      planes, <inliers> inliers)` and one line `Plane <r>: <inliers> inliers, normal (<nx>, <ny>, <nz>), offset <off>,
//                      hypothesis <h>` per accepted plane.
//              -E <tolerance_mm,min_size[,max_size]>  Euclidean cluster filter on the stitched cloud (pcs_cluster_filter_device: records
//                      within tolerance_mm of each other are connected; a record stays iff its connected component holds min_size to
//                      max_size records, max_size 0 or absent: no upper bound). -t prints `Cluster filter: <in> -> <kept> points
//                      (<clusters> clusters, <kept_clusters> kept, largest <largest>)`. Zero-depth pixels form one huge cluster on
//                      their camera's origin: with -i give -Z (or -B).
//              -L <file>[,<max_objects>]  (with -E) what the clusters that stay ARE: the E stage calls pcs_cluster_objects_device (plain or
//                      counted by the chain's rule) with its usual output buffer, count word and statistics block, so the cloud that
//                      leaves the stage, and everything behind it, is byte for byte what -E alone gives; the object table (objects by
//                      ascending first record: label, size, inclusive box, integer sums of coordinates and colours) stays on the
//                      device. -t prints `Objects: <n_objects> (<written> written)` behind the `Cluster filter:` line. After the last
//                      frame-set <file> (`-`: stdout) gets one header line `# k label size lo_x lo_y lo_z hi_x hi_y hi_z sum_x sum_y
//                      sum_z sum_r sum_g sum_b` and one line of raw integers per written object of that frame-set, at most max_objects
//                      (1..65536, default 1024). Refused without -E and with -G (the node library has no object table).
//              -J <file>[,<cell_mm>[,<min_votes>]]  (with -E) the same object in every frame-set: behind the E stage's objects call
//                      (the table at -L's default size if -L is not given, and object_of) one pcs_tracker_update_device, plain or
//                      counted by the chain's rule, over the cloud that stage read; max_cells is the chain's record capacity. After
//                      EVERY frame-set <file> (`-`: stdout) gets one line of raw integers per object, by ascending k, under the header
//                      `# frame k id age prev votes label size lo_x lo_y lo_z hi_x hi_y hi_z sum_x sum_y sum_z`. -t prints `Tracks:
//                      <born> born, <continued> continued, <lost> lost` over the run. Refused without -E and with -G.
//              -W <file>  (with -E) which way an object lies: behind the E stage's objects call (and -J's update, where given) one
//                      pcs_object_boxes_device, plain or counted by the chain's rule, over the cloud that stage read and its object_of.
//                      After EVERY frame-set <file> (`-`: stdout) gets one line of raw integers per object, by ascending k: frame, k
//                      and the entry's 27 integers in the struct's order, under one header line; a line joins -J's on (frame, k). -t
//                      prints `Boxes: <objects> objects, <r> of rank 3` over the run. Refused without -E and with -G.
//              -H <prefix>,<up>,<cell_mm>,<W>x<H>[,<u0>,<v0>[,<lo>,<hi>]]  plan-view maps (pcs_planview.h): no stage, drops nothing. Each
//                      frame-set one pcs_plan_view_device, plain or counted by the chain's rule, over the cloud that LEAVES the chain
//                      (the stitched cloud if no stage is on), ahead of -V. After the last frame-set <prefix>.rgb.ppm, <prefix>.top.pgm
//                      and <prefix>.count.pgm are written: file row r is map row cv = r, no flip. -t prints `Plan view: <n> considered,
//                      <b> in band, <m> on the map, <o> occupied of <W> x <H> cells, fullest <f>` per frame-set. Refused with -G.
//     with neither -i nor -c the cameras are 8 synthetic 1280x720 streams on this node (there are no live cameras here).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <thread>
#include <functional>
#include <vector>

#include <getopt.h>
#include <signal.h>

#include "pcs_cropbox.h"
#include "pcs_filter_chain.h"
#include "pcs_synth.h"
#include "pcs_wire.h"
#include "../../include/pcs_node.h"

typedef std::chrono::high_resolution_clock clockTime;
typedef std::chrono::duration<double, std::milli> timeMilli;

static bool timer = false, serve = true;
static int downsample = 1, n_streams = 8, device = 0, serve_port = 9000, max_sets = 30, n_gpus = 0, voxel_leaf = 0;
static bool drop_invalid = false, pipelined = false, compressed = false;
static std::vector<int> gpu_ids;
static int voxel_route = PCS_NODE_VOXEL_PARTIALS;
static const char* source = nullptr;
static const char* cameras = nullptr;
static const char* dump_path = nullptr;
static const char* transform_path = nullptr;
static bool crop = false;
static int16_t crop_lo[3], crop_hi[3];
static pcs_filter_chain::Chain chain;      // -X -O -K -M -E
using pcs_filter_chain::Cloud;

static void usage()
{
    std::string filters;
    for (const auto& stage : pcs_filter_chain::kStages) filters += stage.help();
    std::cout << "\nMulticamera pointcloud stitching (MI355X)\nUsage: pcs-multicamera-optimized [options]\n\nOptions:\n"
              << " -h (help)        Display command line options\n"
              << " -f (fast)        Accepted for compatibility (it thinned the reference's PCL viewer); no effect\n"
              << " -t (timer)       Displays the runtime of certain functions\n"
              << " -d (downsample)  Downsamples the stitched pointcloud by the specified integer\n"
              << " -i <src>         cameras on this node: synth:<W>x<H> or frames.pcsraw (default synth:1280x720)\n"
              << " -c <list>        edge servers host:port,... (pull 'Z' protocol)\n"
              << " -N <n> streams   -g <gpu>   -p <port> (default 9000)   -r <frame-sets>   -o <file>   -q no server\n"
              << " -G <n>           shard the -i cameras over n GPUs of this node (one process, RCCL gather to GPU 0)\n"
              << " -G <id,id,...>   the same with explicit device ids per peer (a repeated id = virtual peers of one GPU)\n"
              << " -V <mm>          serve the voxel-grid downsample (leaf in millimetres) of the stitched cloud;  -Z drop invalid depth\n"
              << "                  with -G: every GPU pre-aggregates its cameras, ONE exchange of the voxel partials, reduced on GPU 0\n"
              << "                  (-R payloads: gather the packed payloads instead and downsample the stitched cloud on GPU 0)\n"
              << " -T <file>        with -c: re-transform every camera's payload by transform[i] (16 values per line) before stitching,\n"
              << "                  as the reference's pcs-multicamera-optimized does (decode, pcl::transformPointCloud, re-encode)\n"
              << " -B <xlo,xhi,ylo,yhi,zlo,zhi>  crop box, millimetres in the world frame, inclusive: -i crops in the fused path, -c crops the\n"
              << "                  received payloads (after -T; -d then keeps every d-th KEPT record per camera); not with -G\n"
              << filters << pcs_objects::help() << pcs_tracks::help() << pcs_boxes::help() << pcs_planview::help()
              << " -z               with -c: every edge sends a compressed frame (pcs-camera-optimized -z: a PCZ1 container); each is validated\n"
              << "                  and decoded on the GPU before the stitch; what is served on -p stays raw\n"
              << " -P               with -G and -i synth:<W>x<H>: device-resident frame loop, two frame-sets in flight (submit / wait)\n"
              << " -s / -v / -n     PCL viewer features of the reference; not available in this build\n";
}

int main(int argc, char** argv)
{
    signal(SIGPIPE, SIG_IGN);
    int c;
    while ((c = getopt(argc, argv, "hftsvd:nc:N:g:p:r:o:qG:i:V:ZR:PT:B:zO:K:E:M:L:X:J:W:H:")) != -1) {
        switch (c) {
            case 't': timer = true; break;
            case 'd': downsample = atoi(optarg); break;
            case 'f':      // src/pcs-multicamera-optimized.cpp:96-98
                std::cerr << "-f (fast) only thinned the reference's PCL viewer; accepted, no effect on the stitched cloud" << std::endl;
                break;
            case 'i': source = optarg; break;
            case 'c': cameras = optarg; break;
            case 'N': n_streams = atoi(optarg); break;
            case 'g': device = atoi(optarg); break;
            case 'p': serve_port = atoi(optarg); break;
            case 'r': max_sets = atoi(optarg); break;
            case 'o': dump_path = optarg; break;
            case 'q': serve = false; break;
            case 'G':
                if (strchr(optarg, ',')) {
                    for (const char* q = optarg; *q;) { gpu_ids.push_back(atoi(q)); q = strchr(q, ','); if (!q) break; q++; }
                    n_gpus = (int)gpu_ids.size();
                } else {
                    n_gpus = atoi(optarg);
                }
                break;
            case 'V': voxel_leaf = atoi(optarg); break;
            case 'R': voxel_route = (optarg[0] == 'p' && optarg[1] == 'a' && optarg[2] == 'y') ? PCS_NODE_VOXEL_PAYLOADS : PCS_NODE_VOXEL_PARTIALS; break;
            case 'Z': drop_invalid = true; break;
            case 'P': pipelined = true; break;
            case 'z': compressed = true; break;
            case 'T': transform_path = optarg; break;
            case 'B': {
                std::string why;
                if (!pcs_cropbox::parse(optarg, crop_lo, crop_hi, why)) { std::cerr << "-B " << optarg << ": " << why << std::endl; return 2; }
                crop = true;
                break;
            }
            case 'O': case 'K': case 'M': case 'E': {
                std::string why;
                if (!chain.parse(c, optarg, why)) { std::cerr << "-" << (char)c << " " << optarg << ": " << why << std::endl; return 2; }
                break;
            }
            case 'X': {
                std::string why;
                if (!chain.parse_background(optarg, why)) { std::cerr << "-X " << optarg << ": " << why << std::endl; return 2; }
                break;
            }
            case 'L': {
                std::string why;
                if (!chain.parse_objects(optarg, why)) { std::cerr << "-L " << optarg << ": " << why << std::endl; return 2; }
                break;
            }
            case 'J': {
                std::string why;
                if (!chain.parse_tracks(optarg, why)) { std::cerr << "-J " << optarg << ": " << why << std::endl; return 2; }
                break;
            }
            case 'W': {
                std::string why;
                if (!chain.parse_boxes(optarg, why)) { std::cerr << "-W " << optarg << ": " << why << std::endl; return 2; }
                break;
            }
            case 'H': {
                std::string why;
                if (!chain.parse_plan(optarg, why)) { std::cerr << "-H " << optarg << ": " << why << std::endl; return 2; }
                break;
            }
            case 's': case 'v': case 'n':
                std::cerr << "-" << (char)c << " drives the reference's PCL viewer / PLY writer, which this build does not include" << std::endl;
                return 2;
            default: usage(); return c == 'h' ? 0 : 2;
        }
    }
    if (downsample < 1) { std::cerr << "downsample must be >= 1" << std::endl; return 2; }
    if (crop && n_gpus > 0) { std::cerr << "-B is not available with -G: the node library has no crop box setter" << std::endl; return 2; }
    chain.finish_options();
    if (chain.tracks() && n_gpus > 0) { std::cerr << "-J is not available with -G: the node library has no object tracker" << std::endl; return 2; }
    if (chain.boxes() && n_gpus > 0) { std::cerr << "-W is not available with -G: the node library has no object boxes" << std::endl; return 2; }
    if (chain.plan_view() && n_gpus > 0) { std::cerr << "-H is not available with -G: the node library has no plan view" << std::endl; return 2; }
    if (chain.objects() && n_gpus > 0) { std::cerr << "-L is not available with -G: the node library has no object table" << std::endl; return 2; }
    for (int k = 0; k < pcs_filter_chain::kStageCount; k++)
        if (chain.enabled[k] && n_gpus > 0) {
            const auto& stage = pcs_filter_chain::kStages[k];
            std::cerr << "-" << stage.letter << " is not available with -G: the node library has no " << stage.refusal << std::endl; return 2;
        }
    if (chain.learning() && n_gpus > 0) { std::cerr << "-X is not available with -G: the node library has no background model" << std::endl; return 2; }
    if (chain.enabled[pcs_filter_chain::kBackgroundStage]) {      // the model's file, before any device is touched
        std::string why;
        if (!chain.load_background(why)) { std::cerr << "-X " << why << std::endl; return 2; }
    }
    if (chain.objects() && !chain.enabled[pcs_filter_chain::kClusterStage]) {
        std::cerr << "-L writes the objects of the cluster filter: it needs -E <tolerance_mm,min_size[,max_size]>" << std::endl; return 2;
    }
    if (chain.tracks() && !chain.enabled[pcs_filter_chain::kClusterStage]) {
        std::cerr << "-J tracks the objects of the cluster filter: it needs -E <tolerance_mm,min_size[,max_size]>" << std::endl; return 2;
    }
    if (chain.boxes() && !chain.enabled[pcs_filter_chain::kClusterStage]) {
        std::cerr << "-W boxes the objects of the cluster filter: it needs -E <tolerance_mm,min_size[,max_size]>" << std::endl; return 2;
    }
    if (compressed && !cameras) { std::cerr << "-z decodes the frames of edge servers: it needs -c <edge list>" << std::endl; return 2; }
    if (source && cameras) { std::cerr << "give at most one of -i <src> or -c <edge list>" << std::endl; usage(); return 2; }
    if (!source && !cameras) source = "synth:1280x720";      // no live cameras on this node: the synthetic generator
    if (voxel_leaf < 0 || voxel_leaf > 32767) { std::cerr << "-V leaf must be 1..32767 mm" << std::endl; return 2; }
    if (optind < argc) {      // a leftover positional argument: most likely the pre-round-2 `-f <src>` spelling
        std::cerr << "unexpected argument '" << argv[optind] << "': the frame source is given with -i <src> (-f is the reference's "
                     "boolean switch)" << std::endl;
        usage();
        return 2;
    }
    if (voxel_leaf && n_gpus > 0 && cameras) { std::cerr << "-G shards cameras of this node (-i), not edge servers (-c)" << std::endl; return 2; }
    if (transform_path && !cameras) { std::cerr << "-T re-transforms payloads received from edge servers (-c); cameras of this node (-i) "
                                                   "get their extrinsic in the fused kernel" << std::endl; return 2; }
    if (drop_invalid && !source) { std::cerr << "-Z applies to cameras on this node (-i); edge servers drop with their own -c" << std::endl; return 2; }

    // ---- frame source / edge connections -------------------------------------------------------
    std::vector<pcs_stream_config> cfgs;
    std::vector<int> cam_fd;
    int W = 0, H = 0;
    FILE* raw = nullptr; int raw_frames = 0;
    if (source) {
        if (strncmp(source, "synth:", 6) == 0) {
            if (sscanf(source + 6, "%dx%d", &W, &H) != 2) { std::cerr << "bad synth spec" << std::endl; return 2; }
            for (int s = 0; s < n_streams; s++) cfgs.push_back(pcs_synth::stream_config(W, H, s, false));
        } else {
            raw = fopen(source, "rb");
            char magic[8]; int32_t ns = 0;
            if (!raw || fread(magic, 1, 8, raw) != 8 || memcmp(magic, "PCSRAW1", 8) != 0 || fread(&ns, 4, 1, raw) != 1 ||
                fread(&raw_frames, 4, 1, raw) != 1 || ns < 1 || ns > PCS_MAX_STREAMS) { std::cerr << "cannot read " << source << std::endl; return 2; }
            n_streams = ns; cfgs.resize(ns);
            if (fread(cfgs.data(), sizeof(pcs_stream_config), ns, raw) != (size_t)ns) return 2;
        }
    } else {
        std::string list = cameras;
        size_t pos = 0;
        while (pos < list.size()) {
            size_t comma = list.find(',', pos);
            std::string item = list.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
            pos = comma == std::string::npos ? list.size() : comma + 1;
            size_t colon = item.rfind(':');
            if (colon == std::string::npos) { std::cerr << "edge entry needs host:port: " << item << std::endl; return 2; }
            int fd = pcs_wire::connect_to(item.substr(0, colon).c_str(), atoi(item.c_str() + colon + 1));
            if (fd < 0) { std::cerr << "Connection failed at " << item << std::endl; return 1; }       // :201-204
            cam_fd.push_back(fd);
        }
        n_streams = (int)cam_fd.size();
        // the stitch-only context needs a config; geometry is irrelevant for pcs_stitch_device
        cfgs.push_back(pcs_synth::stream_config(64, 48, 0, false));
    }

    std::vector<pcs_payload_desc> xf;           // -T: transform[i] per camera (src/pcs-multicamera-optimized.cpp:417-455 as a file)
    if (transform_path) {
        FILE* f = fopen(transform_path, "r");
        if (!f) { std::cerr << "cannot open transform file " << transform_path << std::endl; return 2; }
        char line[1024];
        while ((int)xf.size() < n_streams && fgets(line, sizeof line, f)) {
            char* hash = strchr(line, '#');
            if (hash) *hash = 0;
            pcs_payload_desc d; memset(&d, 0, sizeof d);
            int got = 0, pos = 0, adv = 0;
            while (got < 16 && sscanf(line + pos, " %f%n", &d.transform[got], &adv) == 1) { got++; pos += adv; if (line[pos] == ',') pos++; }
            if (got == 0) continue;
            if (got != 16) { std::cerr << transform_path << ": expected 16 values per line" << std::endl; fclose(f); return 2; }
            xf.push_back(d);
        }
        fclose(f);
        if ((int)xf.size() < n_streams) { std::cerr << transform_path << ": only " << xf.size() << " matrices for " << n_streams << " cameras" << std::endl; return 2; }
    }

    pcs_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.device = device; cfg.n_streams = (int)cfgs.size(); cfg.streams = cfgs.data();
    cfg.downsample = source ? downsample : 1;
    cfg.flags = (source && drop_invalid) ? PCS_FLAG_DROP_INVALID : 0u;
    pcs_ctx* ctx = nullptr;
    int rc = pcs_create(&ctx, &cfg);
    if (rc != PCS_OK) { std::cerr << "pcs_create: " << pcs_strerror(rc) << ": " << pcs_last_error(nullptr) << std::endl; return 1; }

    if (crop && (rc = pcs_set_crop_box_mm(ctx, crop_lo, crop_hi)) != PCS_OK) {
        std::cerr << "pcs_set_crop_box_mm: " << pcs_strerror(rc) << ": " << pcs_last_error(ctx) << std::endl; return 1;
    }

    pcs_node* node = nullptr;
    if (n_gpus > 0) {
        if (!source) { std::cerr << "-G applies to cameras on this node (-i)" << std::endl; return 2; }
        if (n_streams % n_gpus) { std::cerr << "-N " << n_streams << " streams do not divide over -G " << n_gpus << " GPUs" << std::endl; return 2; }
        std::vector<int> ids(n_gpus);
        for (int g = 0; g < n_gpus; g++) ids[g] = gpu_ids.empty() ? device + g : gpu_ids[g];
        rc = pcs_node_create(&node, n_gpus, ids.data(), n_streams / n_gpus, cfgs.data(), cfg.flags, downsample);
        if (rc != PCS_OK) { std::cerr << "pcs_node_create: " << pcs_strerror(rc) << ": " << pcs_node_last_error(nullptr) << std::endl; return 1; }
        std::cout << "Sharding " << n_streams << " cameras over " << n_gpus << " GPU(s), RCCL gather to GPU " << ids[0]
                  << " (communicator of " << pcs_node_rccl_ranks(node) << " rank(s))" << std::endl;
    }

    // ---- buffers -------------------------------------------------------------------------------
    int size_bytes = 0;
    const size_t cam_cap_bytes = (size_t)10 * 4u * 1000 * 1000;           // per-camera receive buffer (reference: 10 MB, :554)
    size_t stitched_shorts = source ? PCS_HEADER_SHORTS + pcs_max_payload_shorts(ctx)
                                    : PCS_HEADER_SHORTS + (size_t)n_streams * cam_cap_bytes / 2;
    // page-locked, like the rasters handed to pcs_process_frames below: the call then runs zero copy (the kernels read
    // the rasters and write the stitched payload over PCIe themselves)
    struct Pinned {
        pcs_ctx* ctx; int16_t* p = nullptr; size_t n = 0;
        explicit Pinned(pcs_ctx* c) : ctx(c) {}
        void release() { if (p) pcs_host_free(ctx, p); p = nullptr; n = 0; }     // before pcs_destroy
        bool resize(size_t shorts)
        {
            if (shorts <= n) return true;
            if (p) pcs_host_free(ctx, p);
            p = nullptr; n = 0;
            if (pcs_host_malloc(ctx, (void**)&p, shorts * sizeof(int16_t)) != PCS_OK) return false;
            n = shorts;
            return true;
        }
        int16_t* data() { return p; }
        size_t size() const { return n; }
    } stitched(ctx);
    if (!stitched.resize(stitched_shorts)) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
    std::vector<uint16_t*> pin_d(source ? n_streams : 0, nullptr);
    std::vector<uint8_t*> pin_c(source ? n_streams : 0, nullptr);
    std::vector<size_t> pin_db(pin_d.size(), 0), pin_cb(pin_c.size(), 0);
    std::vector<std::vector<uint16_t>> depth(source ? n_streams : 0);
    std::vector<std::vector<uint8_t>> color(source ? n_streams : 0);
    std::vector<std::vector<uint8_t>> cam_buf(source ? 0 : n_streams, std::vector<uint8_t>(source ? 0 : cam_cap_bytes));
    std::vector<void*> d_cam(source ? 0 : n_streams, nullptr);
    void* d_stitched = nullptr;
    if (!source) {
        for (int i = 0; i < n_streams; i++) if (pcs_device_malloc(ctx, &d_cam[i], cam_cap_bytes) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
        if (pcs_device_malloc(ctx, &d_stitched, (size_t)n_streams * cam_cap_bytes + 64) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
    }

    // -B with -c: the crop's output (its inputs are the cameras' buffers, or d_stitched's slices behind -T) and its device counts
    void *d_cropped = nullptr, *d_crop_counts = nullptr;
    if (crop && !source) {
        if (pcs_device_malloc(ctx, &d_cropped, (size_t)n_streams * cam_cap_bytes + 64) != PCS_OK ||
            pcs_device_malloc(ctx, &d_crop_counts, sizeof(int32_t) * (n_streams + 1)) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
    }
    // -B with -i -V, and the chain with -i: the payload and its counts stay on the device between the calls
    void *d_pay = nullptr, *d_pay_counts = nullptr;
    if (source && ((crop && voxel_leaf) || chain.any())) {
        if (pcs_device_malloc(ctx, &d_pay, pcs_max_payload_shorts(ctx) * sizeof(int16_t) + 64) != PCS_OK ||
            pcs_device_malloc(ctx, &d_pay_counts, sizeof(int32_t) * (n_streams + 1)) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
    }

    // -X -O -K -M -E: the chain's buffers hold the largest cloud that can enter it (and -X's model is created or imported)
    if (chain.any() && chain.allocate(ctx, source ? pcs_max_payload_shorts(ctx) : (size_t)n_streams * cam_cap_bytes / 2) != PCS_OK) {
        std::cerr << pcs_last_error(ctx) << std::endl; return 1;
    }
    if (chain.tracks() && !chain.open_tracks()) { std::cerr << "-J: cannot write " << chain.tracks_file << std::endl; return 1; }
    if (chain.boxes() && !chain.open_boxes()) { std::cerr << "-W: cannot write " << chain.boxes_file << std::endl; return 1; }

    // -V: device-resident rasters (with -i) and the voxel cloud
    std::vector<void*> d_depth, d_color;
    void *d_vox = nullptr, *d_nvox = nullptr;
    size_t vox_cap_points = 0;
    if (voxel_leaf) {
        vox_cap_points = source ? pcs_max_payload_shorts(ctx) / PCS_POINT_SHORTS : (size_t)n_streams * cam_cap_bytes / PCS_POINT_BYTES;
        if (source && cfg.downsample != 1) {
            vox_cap_points = 0;
            for (auto& sc : cfgs) vox_cap_points += (size_t)sc.depth.width * sc.depth.height;
        }
        if (!node && (pcs_device_malloc(ctx, &d_vox, vox_cap_points * PCS_POINT_BYTES + 64) != PCS_OK ||
                      pcs_device_malloc(ctx, &d_nvox, 64) != PCS_OK)) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
        if (!stitched.resize(PCS_HEADER_SHORTS + vox_cap_points * PCS_POINT_SHORTS)) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
    }
    if ((voxel_leaf || chain.any()) && source && !node) {      // (with -G the node library stages the rasters on their owning GPUs itself)
        d_depth.resize(n_streams, nullptr); d_color.resize(n_streams, nullptr);
        for (int s = 0; s < n_streams; s++) {
            const size_t db = (size_t)cfgs[s].depth.width * cfgs[s].depth.height * 2;
            const size_t cb = (size_t)cfgs[s].color_stride * cfgs[s].color.height;
            if (pcs_device_malloc(ctx, &d_depth[s], db + 64) != PCS_OK || pcs_device_malloc(ctx, &d_color[s], cb + 64) != PCS_OK) {
                std::cerr << pcs_last_error(ctx) << std::endl; return 1;
            }
        }
    }
    // the voxel cloud of whatever d_vox / d_nvox hold -> stitched (header + records). `again` repeats the device call that filled
    // them: a count of -1 (the bucket tail gave up on a stalled device, include/pcs_hip.h) is answered by one more run on the LSD
    // tail; a negative length never reaches the size arithmetic below or the wire (the reference sends `size` as it is, :394-403)
    auto fetch_voxels = [&](const std::function<int()>& again) -> bool {
        int32_t nv = 0;
        if (pcs_memcpy_d2h(ctx, &nv, d_nvox, sizeof nv) != PCS_OK || pcs_synchronize(ctx) != PCS_OK) return false;
        if (nv < 0) {
            std::cerr << "voxel grid: the bucket tail gave up waiting for a workgroup; running the frame-set again on the LSD tail" << std::endl;
            if (pcs_set_voxel_tail(ctx, PCS_VOXEL_TAIL_LSD_LATCHED) != PCS_OK || again() != PCS_OK) return false;
            if (pcs_memcpy_d2h(ctx, &nv, d_nvox, sizeof nv) != PCS_OK || pcs_synchronize(ctx) != PCS_OK) return false;
            if (nv < 0) { std::cerr << "voxel grid: negative count on the LSD tail too" << std::endl; return false; }
        }
        size_bytes = nv * PCS_POINT_BYTES;
        if (size_bytes && pcs_memcpy_d2h(ctx, stitched.data() + PCS_HEADER_SHORTS, d_vox, (size_t)size_bytes) != PCS_OK) return false;
        if (pcs_synchronize(ctx) != PCS_OK) return false;
        memcpy(stitched.data(), &size_bytes, sizeof(int));
        return true;
    };

    // -O -K -M -E over `in`, then what is served -> stitched: with -V the voxel grid of the chain's output, on its device count where
    // it has one; else the records themselves, their count fetched once. Then the chain's -t lines, after the frame-set's last launch.
    // (`again` of fetch_voxels repeats the voxel call alone.)
    auto filter_to_stitched = [&](const Cloud& in) -> bool {
        const Cloud c = chain.run(ctx, in);
        if (chain.status != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return false; }
        if (chain.plan_view() && chain.run_plan(ctx, c) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return false; }     // -H
        if (voxel_leaf) {
            auto run_voxel = [&]() {
                int16_t* out = static_cast<int16_t*>(d_vox);
                const size_t out_shorts = vox_cap_points * PCS_POINT_SHORTS;
                return c.d_n ? pcs_voxel_grid_device_counted(ctx, c.d, c.d_n, c.capacity, voxel_leaf, out, out_shorts, static_cast<int32_t*>(d_nvox))
                             : pcs_voxel_grid_device(ctx, c.d, c.n, voxel_leaf, out, out_shorts, static_cast<int32_t*>(d_nvox));
            };
            if (run_voxel() != PCS_OK || !fetch_voxels(run_voxel)) { std::cerr << pcs_last_error(ctx) << std::endl; return false; }
        } else {
            int32_t n = c.n;
            if (c.d_n && (pcs_memcpy_d2h(ctx, &n, c.d_n, sizeof n) != PCS_OK || pcs_synchronize(ctx) != PCS_OK)) {
                std::cerr << pcs_last_error(ctx) << std::endl; return false;
            }
            size_bytes = n * PCS_POINT_BYTES;
            if (size_bytes && pcs_memcpy_d2h(ctx, stitched.data() + PCS_HEADER_SHORTS, c.d, (size_t)size_bytes) != PCS_OK) return false;
            pcs_synchronize(ctx);
            memcpy(stitched.data(), &size_bytes, sizeof(int));                                             // :394-395
        }
        if (timer && !chain.report(std::cout)) { std::cerr << pcs_last_error(ctx) << std::endl; return false; }
        if (timer && chain.plan_view() && !chain.report_plan(std::cout)) { std::cerr << pcs_last_error(ctx) << std::endl; return false; }
        if (chain.tracks()) {      // -J: this frame-set's lines
            std::string why;
            if (!chain.write_tracks(why)) { std::cerr << "-J: " << (why.empty() ? pcs_last_error(ctx) : why.c_str()) << std::endl; return false; }
        }
        if (chain.boxes()) {       // -W: this frame-set's lines
            std::string why;
            if (!chain.write_boxes(why)) { std::cerr << "-W: " << (why.empty() ? pcs_last_error(ctx) : why.c_str()) << std::endl; return false; }
        }
        return true;
    };

    if (pipelined) {
        // ---- the frame loop of a node with device-resident rasters: submit(k+1); wait(k) ------------------------------------
        if (!node || !source || raw) { std::cerr << "-P needs -G <n> and -i synth:<W>x<H>" << std::endl; return 2; }
        const int per = n_streams / n_gpus, ring = 3;
        std::vector<int> ids(n_gpus);
        for (int g = 0; g < n_gpus; g++) ids[g] = gpu_ids.empty() ? device + g : gpu_ids[g];
        // one small context per peer for its device memory (the node's own contexts are private to it)
        std::vector<pcs_ctx*> mem(n_gpus, nullptr);
        for (int g = 0; g < n_gpus; g++) {
            pcs_config mc; memset(&mc, 0, sizeof mc);
            mc.device = ids[g]; mc.n_streams = 1; mc.streams = cfgs.data(); mc.downsample = 1;
            if (pcs_create(&mem[g], &mc) != PCS_OK) { std::cerr << "pcs_create: " << pcs_last_error(nullptr) << std::endl; return 1; }
        }
        std::vector<std::vector<const uint16_t*>> rd(ring, std::vector<const uint16_t*>(n_streams));
        std::vector<std::vector<const uint8_t*>> rc_(ring, std::vector<const uint8_t*>(n_streams));
        std::vector<uint16_t> hd; std::vector<uint8_t> hc;
        for (int k = 0; k < ring; k++)
            for (int s = 0; s < n_streams; s++) {
                pcs_ctx* m = mem[s / per];
                pcs_synth::depth(W, H, s, pcs_synth::kSeed + 7919u * (uint32_t)k, hd);
                pcs_synth::color(W, H, s, pcs_synth::kSeed + 7919u * (uint32_t)k, hc);
                void *dd = nullptr, *dc = nullptr;
                if (pcs_device_malloc(m, &dd, hd.size() * 2 + 64) != PCS_OK || pcs_device_malloc(m, &dc, hc.size() + 64) != PCS_OK ||
                    pcs_memcpy_h2d(m, dd, hd.data(), hd.size() * 2) != PCS_OK || pcs_memcpy_h2d(m, dc, hc.data(), hc.size()) != PCS_OK) {
                    std::cerr << pcs_last_error(m) << std::endl; return 1;
                }
                rd[k][s] = static_cast<const uint16_t*>(dd); rc_[k][s] = static_cast<const uint8_t*>(dc);
            }
        const size_t cap = pcs_node_max_payload_shorts(node);
        void* d_out[2] = {nullptr, nullptr};
        for (int k = 0; k < 2; k++)
            if (pcs_device_malloc(mem[0], &d_out[k], cap * sizeof(int16_t) + 64) != PCS_OK) { std::cerr << pcs_last_error(mem[0]) << std::endl; return 1; }
        pcs_node_set_timing(node, timer ? 1 : 0);
        auto submit = [&](int k, int* t) {
            return voxel_leaf ? pcs_node_submit_voxel_device(node, rd[k % ring].data(), rc_[k % ring].data(), voxel_leaf,
                                                             static_cast<int16_t*>(d_out[k & 1]), cap, t)
                              : pcs_node_submit_device(node, rd[k % ring].data(), rc_[k % ring].data(), static_cast<int16_t*>(d_out[k & 1]), cap, t);
        };
        int last_n = 0;
        auto wait = [&](int t) {
            return voxel_leaf ? pcs_node_wait_voxel(node, t, &last_n) : pcs_node_wait(node, t, nullptr, &last_n);
        };
        const int warm = 5, iters = max_sets < 1 ? 1 : max_sets;
        int t_prev = -1, t_cur = -1;
        clockTime::time_point t0;
        pcs_node_stats st; memset(&st, 0, sizeof st);
        double k_ms = 0, x_ms = 0, r_ms = 0;
        for (int k = 0; k < warm + iters; k++) {
            if (k == warm) {                                    // drain, then time `iters` steady-state periods
                if (t_prev >= 0 && wait(t_prev) != PCS_OK) { std::cerr << pcs_node_last_error(node) << std::endl; return 1; }
                t_prev = -1;
                t0 = clockTime::now();
            }
            if (submit(k, &t_cur) != PCS_OK) { std::cerr << pcs_node_last_error(node) << std::endl; return 1; }
            if (t_prev >= 0) {
                if (wait(t_prev) != PCS_OK) { std::cerr << pcs_node_last_error(node) << std::endl; return 1; }
                if (timer && k > warm) { pcs_node_last_stats(node, &st); k_ms += st.kernels_ms; x_ms += st.exchange_ms; r_ms += st.root_ms; }
            }
            t_prev = t_cur;
        }
        if (wait(t_prev) != PCS_OK) { std::cerr << pcs_node_last_error(node) << std::endl; return 1; }
        const double ms = timeMilli(clockTime::now() - t0).count() / iters;
        const double mpix = (double)n_streams * W * H / 1e6;
        std::cout << "Pipelined " << (voxel_leaf ? "voxel grid" : "stitch") << " over " << n_gpus << " peer(s): " << ms << " ms per frame-set, "
                  << mpix / ms * 1e3 << " Mpoints/s in, " << last_n << (voxel_leaf ? " voxels" : " points") << std::endl;
        if (voxel_leaf && pcs_node_voxel_reruns(node) > 0)
            std::cout << "Voxel frame-sets run again on the LSD tail after a flagged bucket tail: " << pcs_node_voxel_reruns(node) << std::endl;
        if (timer && iters > 1)
            std::cout << "GPU " << ids[0] << " per frame-set: kernels " << k_ms / (iters - 1) << " ms, exchange " << x_ms / (iters - 1)
                      << " ms, root " << r_ms / (iters - 1) << " ms (" << st.exchanged_bytes << " B into the root)" << std::endl;
        if (dump_path) {       // the last frame-set, in the wire format of the other modes
            size_bytes = last_n * PCS_POINT_BYTES;
            if (!stitched.resize(PCS_HEADER_SHORTS + (size_t)last_n * PCS_POINT_SHORTS + 8)) return 1;
            if (size_bytes && pcs_memcpy_d2h(mem[0], stitched.data() + PCS_HEADER_SHORTS, d_out[(warm + iters - 1) & 1], (size_t)size_bytes) != PCS_OK) return 1;
            memcpy(stitched.data(), &size_bytes, sizeof(int));
            FILE* f = fopen(dump_path, "wb");
            if (f) { fwrite(stitched.data(), 1, (size_t)size_bytes + 4, f); fclose(f); }
        }
        pcs_node_destroy(node);
        for (int k = 0; k < ring; k++)
            for (int s = 0; s < n_streams; s++) { pcs_device_free(mem[s / per], const_cast<uint16_t*>(rd[k][s])); pcs_device_free(mem[s / per], const_cast<uint8_t*>(rc_[k][s])); }
        for (int k = 0; k < 2; k++) pcs_device_free(mem[0], d_out[k]);
        for (pcs_ctx* m : mem) pcs_destroy(m);
        stitched.release();
        pcs_destroy(ctx);
        return 0;
    }

    int listen_fd = -1, client_fd = -1;
    if (serve) {
        listen_fd = pcs_wire::listen_on(serve_port);
        if (listen_fd < 0) { std::cerr << "Couldn't bind server sockfd" << std::endl; return 1; }            // :226-229
        std::cout << "Waiting for client..." << std::endl;
        client_fd = ::accept(listen_fd, NULL, NULL);
        if (client_fd < 0) { std::cerr << "Connection failed" << std::endl; return 1; }
        std::cout << "Established connection with client_sock: " << client_fd << std::endl;
    }

    // the reference primes each camera with one pull before its loop (:557 sendPullRequest)
    for (int fd : cam_fd) pcs_wire::send_pull(fd);

    double total = 0;
    int loop_count = 1;
    for (int set = 0; set < max_sets; set++) {
        auto stitch_start = clockTime::now();
        if (source) {
            if (raw) {
                if (set >= raw_frames) break;
                for (int s = 0; s < n_streams; s++) {
                    depth[s].resize((size_t)cfgs[s].depth.width * cfgs[s].depth.height);
                    color[s].resize((size_t)cfgs[s].color_stride * cfgs[s].color.height);
                    if (fread(depth[s].data(), 2, depth[s].size(), raw) != depth[s].size() ||
                        fread(color[s].data(), 1, color[s].size(), raw) != color[s].size()) { std::cerr << "short read" << std::endl; return 1; }
                }
            } else {
                for (int s = 0; s < n_streams; s++) {
                    pcs_synth::depth(W, H, s, pcs_synth::kSeed + 7919u * (uint32_t)set, depth[s]);
                    pcs_synth::color(W, H, s, pcs_synth::kSeed + 7919u * (uint32_t)set, color[s]);
                }
                stitch_start = clockTime::now();                   // generation is not part of the stitch
            }
            std::vector<const uint16_t*> dp(n_streams); std::vector<const uint8_t*> cp(n_streams);
            for (int s = 0; s < n_streams; s++) {
                const size_t db = depth[s].size() * sizeof(uint16_t), cb = color[s].size();
                if (db > pin_db[s]) {
                    if (pin_d[s]) pcs_host_free(ctx, pin_d[s]);
                    if (pcs_host_malloc(ctx, (void**)&pin_d[s], db) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                    pin_db[s] = db;
                }
                if (cb > pin_cb[s]) {
                    if (pin_c[s]) pcs_host_free(ctx, pin_c[s]);
                    if (pcs_host_malloc(ctx, (void**)&pin_c[s], cb) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                    pin_cb[s] = cb;
                }
                memcpy(pin_d[s], depth[s].data(), db);
                memcpy(pin_c[s], color[s].data(), cb);
                dp[s] = pin_d[s]; cp[s] = pin_c[s];
            }
            if (!raw) stitch_start = clockTime::now();             // handing the frames over is the source's part, not the stitch
            if (voxel_leaf && node) {
                // BASELINE configs[4]: the cameras' voxel partials are pre-aggregated on their GPUs, exchanged once, reduced on GPU 0
                pcs_node_voxel_stats vstats;
                rc = pcs_node_process_voxel(node, dp.data(), cp.data(), voxel_leaf, voxel_route, stitched.data(), stitched.size(), 1,
                                            &size_bytes, &vstats);
                if (rc != PCS_OK) { std::cerr << pcs_node_last_error(node) << std::endl; return 1; }
                if (timer)
                    std::cout << "Voxel grid over " << n_gpus << " GPU(s): kernels " << vstats.kernels_ms << " ms, exchange " << vstats.exchange_ms
                              << " ms (" << vstats.exchanged_bytes << " B), root " << vstats.root_voxel_ms << " ms, " << vstats.partials
                              << (voxel_route == PCS_NODE_VOXEL_PARTIALS ? " partials -> " : " points -> ") << vstats.voxels << " voxels" << std::endl;
            } else if (chain.any()) {
                // the payload on the device (under -Z / -B / -d as ever), the chain on its device count, then the voxel grid on the
                // chain's device count or the kept records out: no count leaves the device in between
                for (int s = 0; s < n_streams; s++) {
                    if (pcs_memcpy_h2d(ctx, d_depth[s], depth[s].data(), depth[s].size() * 2) != PCS_OK ||
                        pcs_memcpy_h2d(ctx, d_color[s], color[s].data(), color[s].size()) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                }
                const size_t max_shorts = pcs_max_payload_shorts(ctx);
                rc = pcs_process_frames_device(ctx, reinterpret_cast<const uint16_t* const*>(d_depth.data()),
                                               reinterpret_cast<const uint8_t* const*>(d_color.data()), static_cast<int16_t*>(d_pay), max_shorts,
                                               static_cast<int32_t*>(d_pay_counts));
                if (rc != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                if (!filter_to_stitched({static_cast<const int16_t*>(d_pay), static_cast<const int32_t*>(d_pay_counts) + n_streams, 0,
                                         (int)(max_shorts / PCS_POINT_SHORTS)})) return 1;
            } else if (voxel_leaf) {
                for (int s = 0; s < n_streams; s++) {
                    if (pcs_memcpy_h2d(ctx, d_depth[s], depth[s].data(), depth[s].size() * 2) != PCS_OK ||
                        pcs_memcpy_h2d(ctx, d_color[s], color[s].data(), color[s].size()) != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                }
                auto run_voxel = [&]() {
                    if (crop) {     // the cropped payload, then its voxel grid: the point count never leaves the device
                        int r = pcs_process_frames_device(ctx, reinterpret_cast<const uint16_t* const*>(d_depth.data()),
                                                          reinterpret_cast<const uint8_t* const*>(d_color.data()), static_cast<int16_t*>(d_pay),
                                                          pcs_max_payload_shorts(ctx), static_cast<int32_t*>(d_pay_counts));
                        if (r != PCS_OK) return r;
                        return pcs_voxel_grid_device_counted(ctx, static_cast<const int16_t*>(d_pay), static_cast<const int32_t*>(d_pay_counts) + n_streams,
                                                             (int)(pcs_max_payload_shorts(ctx) / PCS_POINT_SHORTS), voxel_leaf, static_cast<int16_t*>(d_vox),
                                                             vox_cap_points * PCS_POINT_SHORTS, static_cast<int32_t*>(d_nvox));
                    }
                    return pcs_process_frames_voxel_device(ctx, reinterpret_cast<const uint16_t* const*>(d_depth.data()),
                                                           reinterpret_cast<const uint8_t* const*>(d_color.data()), voxel_leaf,
                                                           static_cast<int16_t*>(d_vox), vox_cap_points * PCS_POINT_SHORTS, static_cast<int32_t*>(d_nvox));
                };
                rc = run_voxel();
                if (rc != PCS_OK || !fetch_voxels(run_voxel)) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
            } else if (node) {
                rc = pcs_node_process(node, dp.data(), cp.data(), stitched.data(), stitched.size(), 1, nullptr, &size_bytes);
                if (rc != PCS_OK) { std::cerr << pcs_node_last_error(node) << std::endl; return 1; }
            } else {
                rc = pcs_process_frames(ctx, dp.data(), cp.data(), stitched.data(), stitched.size(), 1, nullptr, &size_bytes);
                if (rc != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
            }
        } else {
            // one reader thread per camera, joined in camera order (:381-386)
            std::vector<int32_t> got(n_streams, -1);
            std::vector<std::thread> th;
            for (int i = 0; i < n_streams; i++)
                th.emplace_back([&, i]() {
                    got[i] = pcs_wire::recv_frame(cam_fd[i], cam_buf[i].data(), cam_buf[i].size());
                    if (got[i] >= 0) pcs_wire::send_pull(cam_fd[i]);                    // :370 next pull right away
                });
            for (auto& t : th) t.join();
            std::vector<int> pts(n_streams);
            std::vector<const int16_t*> dptr(n_streams);
            bool ok = true;
            for (int i = 0; i < n_streams; i++) {
                if (got[i] < 0) { ok = false; break; }
                if (compressed) {      // the frame is a container: validated on the host, decoded into the camera's device payload
                    rc = pcs_decompress_payload(ctx, cam_buf[i].data(), (size_t)got[i], static_cast<int16_t*>(d_cam[i]), cam_cap_bytes / 2, &pts[i]);
                    if (rc != PCS_OK) { std::cerr << "camera " << i << ": " << pcs_strerror(rc) << ": " << pcs_last_error(ctx) << std::endl; return 1; }
                    dptr[i] = static_cast<const int16_t*>(d_cam[i]);
                    continue;
                }
                pts[i] = got[i] / PCS_POINT_BYTES;
                if (got[i] && pcs_memcpy_h2d(ctx, d_cam[i], cam_buf[i].data(), (size_t)got[i]) != PCS_OK) ok = false;
                dptr[i] = static_cast<const int16_t*>(d_cam[i]);
            }
            if (!ok) { std::cout << "camera stream ended" << std::endl; break; }
            int total_pts = 0;
            const int16_t* d_result = static_cast<const int16_t*>(d_stitched);
            if (crop) {
                // -T first (every record, stride 1), then the box over the moved payloads with the stride -d
                if (transform_path) {
                    std::vector<int> per(n_streams);
                    for (int i = 0; i < n_streams; i++) { xf[i].d_payload = dptr[i]; xf[i].n_points = pts[i]; }
                    rc = pcs_transform_payloads_device(ctx, n_streams, xf.data(), 1, static_cast<int16_t*>(d_stitched),
                                                       (size_t)n_streams * cam_cap_bytes / 2, per.data(), &total_pts);
                    if (rc != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
                    size_t first = 0;
                    for (int i = 0; i < n_streams; i++) { dptr[i] = static_cast<const int16_t*>(d_stitched) + first * PCS_POINT_SHORTS; pts[i] = per[i]; first += (size_t)per[i]; }
                }
                rc = pcs_crop_payloads_device(ctx, dptr.data(), pts.data(), n_streams, downsample, static_cast<int16_t*>(d_cropped),
                                              (size_t)n_streams * cam_cap_bytes / 2, static_cast<int32_t*>(d_crop_counts));
                if (rc == PCS_OK) {
                    std::vector<int32_t> kept(n_streams + 1, 0);
                    rc = pcs_memcpy_d2h(ctx, kept.data(), d_crop_counts, kept.size() * sizeof(int32_t));
                    if (rc == PCS_OK) rc = pcs_synchronize(ctx);
                    total_pts = kept[n_streams];
                }
                d_result = static_cast<const int16_t*>(d_cropped);
            } else if (transform_path) {       // the reference program's own semantics: decode, transform[i], re-encode, concatenate
                for (int i = 0; i < n_streams; i++) { xf[i].d_payload = dptr[i]; xf[i].n_points = pts[i]; }
                rc = pcs_transform_payloads_device(ctx, n_streams, xf.data(), downsample, static_cast<int16_t*>(d_stitched),
                                                   (size_t)n_streams * cam_cap_bytes / 2, nullptr, &total_pts);
            } else
            rc = pcs_stitch_device(ctx, dptr.data(), pts.data(), n_streams, downsample, static_cast<int16_t*>(d_stitched),
                                   (size_t)n_streams * cam_cap_bytes / 2, &total_pts);
            if (rc != PCS_OK) { std::cerr << pcs_last_error(ctx) << std::endl; return 1; }
            if (!filter_to_stitched({d_result, nullptr, total_pts, total_pts})) return 1;
        }
        if (serve) {
            int req = pcs_wire::recv_pull(client_fd);                                                      // :398
            if (req < 0) { std::cout << "Client disconnected" << std::endl; break; }
            if (req != pcs_wire::kPullXYZRGB) { std::cerr << "Faulty pull request" << std::endl; return 1; }   // :405-408
            if (!pcs_wire::send_frame(client_fd, stitched.data(), size_bytes)) { std::cout << "Client disconnected" << std::endl; break; }
        }
        if (timer) {
            total += timeMilli(clockTime::now() - stitch_start).count();
            std::cout << "Stitching: " << total / loop_count << " ms, " << "Frame: " << loop_count << std::endl;   // :426-428
            loop_count++;
        }
    }
    if (dump_path) {
        FILE* f = fopen(dump_path, "wb");
        if (f) { fwrite(stitched.data(), 1, (size_t)size_bytes + 4, f); fclose(f); }
    }
    const int learn_status = chain.finish_learning(std::cout, std::cerr, timer);      // -X learn: the model into its file
    if (chain.objects()) {      // -L: the last frame-set's object table
        bool ok;
        if (chain.objects_file == "-") {
            ok = chain.write_objects(std::cout);
        } else {
            std::ofstream f(chain.objects_file);
            ok = f.good() && chain.write_objects(f);
            if (!f.good()) std::cerr << "-L: cannot write " << chain.objects_file << std::endl;
        }
        if (!ok) std::cerr << "-L: " << pcs_last_error(ctx) << std::endl;
    }
    int plan_status = 0;
    if (chain.plan_view()) {    // -H: the last frame-set's maps
        std::string why;
        if (!chain.write_plan(why)) { std::cerr << "-H: " << (why.empty() ? pcs_last_error(ctx) : why.c_str()) << std::endl; plan_status = 1; }
    }
    if (chain.tracks() && timer)
        std::cout << "Tracks: " << chain.tracks_born << " born, " << chain.tracks_continued << " continued, " << chain.tracks_lost << " lost" << std::endl;
    if (chain.boxes() && timer) std::cout << "Boxes: " << chain.boxes_objects << " objects, " << chain.boxes_rank3 << " of rank 3" << std::endl;
    for (int fd : cam_fd) ::close(fd);
    if (client_fd >= 0) ::close(client_fd);
    if (listen_fd >= 0) ::close(listen_fd);
    for (void* p : d_cam) if (p) pcs_device_free(ctx, p);
    for (void* p : pin_d) if (p) pcs_host_free(ctx, p);
    for (void* p : pin_c) if (p) pcs_host_free(ctx, p);
    for (void* p : d_depth) if (p) pcs_device_free(ctx, p);
    for (void* p : d_color) if (p) pcs_device_free(ctx, p);
    if (d_vox) pcs_device_free(ctx, d_vox);
    if (d_nvox) pcs_device_free(ctx, d_nvox);
    if (d_stitched) pcs_device_free(ctx, d_stitched);
    for (void* p : {d_cropped, d_crop_counts, d_pay, d_pay_counts}) if (p) pcs_device_free(ctx, p);
    chain.release();
    if (node) pcs_node_destroy(node);
    stitched.release();
    pcs_destroy(ctx);
    return learn_status ? learn_status : plan_status;
}
