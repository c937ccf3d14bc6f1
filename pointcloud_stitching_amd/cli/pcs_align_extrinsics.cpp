// pcs-align-extrinsics — refine the extrinsics of a multi-camera rig from the cameras' own payloads (include/pcs_hip.h:
// pcs_align_payloads_device, pcs_align_payloads_plane_device; DESIGN.md section 3 "Alignment sums", "Plane sums"). Sits between
// calibration.py, which places every camera from four surveyed markers, and the -T of pcs-multicamera-optimized, which consumes one
// matrix per camera:
//
//     pcs-align-extrinsics -T in.txt -o out.txt [-A max_dist_mm,iterations[,stride]] [-p radius_mm,min_neighbors[,flatness]] [-R ref]
//                          [-g gpu] [-t] cam0.bin cam1.bin ...
//
//   cam*.bin   [int32 bytes][records], what `pcs-camera-optimized -o` writes: one file, one camera, in its own frame. Records whose
//              three coordinates are all zero (zero-depth pixels: the only way to get one) are dropped before upload, and counted.
//   -T / -o    one line of 16 values per camera, row-major 4x4 in metres (the -T format of pcs-multicamera-optimized).
//   -R ref     the camera the others are moved onto (default 0): the target is its payload moved by in[ref]. Its line is copied.
//   -A         max_dist_mm 1..1000 (default 60), iterations 1..100 (default 30), every stride-th source record (default 1).
//   -p         point to plane instead of point to point: the target's surface normals are estimated from its neighbours within
//              radius_mm 1..1000, at least min_neighbors 3..32767 of them, and kept where flatness (0 = off, else 1..1000) times the
//              smallest eigenvalue of the neighbourhood does not exceed the middle one. Far fewer iterations reach a far smaller
//              rotation error on independently sampled surfaces (-A 60,6 -p 120,6,20 is a start). Without -p nothing changes.
//   -t         per camera: iterations, matched share, first and last rms (with -p: the method, and the share with a normal).
// Every other camera is refined from in[i]; out.txt gets (float)T_K printed with %.9g, so the float survives the round trip. A camera
// whose loop ends refused keeps in[i], with a `# camera i not refined: <reason>` comment before its line and a warning on stderr.
// Exit status: 0 all cameras refined, 3 some camera not refined, 2 usage, 1 anything else.

#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "pcs_align.h"
#include "pcs_synth.h"

static void usage()
{
    std::cerr << "usage: pcs-align-extrinsics -T in.txt -o out.txt [-A max_dist_mm,iterations[,stride]] [-p radius_mm,min_neighbors[,flatness]]\n"
              << "                            [-R ref] [-g gpu] [-t] cam0.bin cam1.bin ...\n"
              << " -T <file>   initial extrinsics, one line of 16 values per camera (row-major 4x4, metres)\n"
              << " -o <file>   refined extrinsics, same format\n"
              << " -A a,b[,c]  max_dist_mm 1..1000 (60), iterations 1..100 (30), source stride (1)\n"
              << " -p a,b[,c]  point to plane: target normals from radius_mm 1..1000, min_neighbors 3..32767, flatness 0..1000 (0 = off)\n"
              << " -R <n>      reference camera (0): the others are moved onto it\n"
              << " -g <n>      GPU (0)\n"
              << " -t          per camera: iterations, matched share, first and last rms (with -p: the method and the used share)\n"
              << " cam*.bin    [int32 bytes][records] as written by pcs-camera-optimized -o\n";
}

// [int32 bytes][records] -> the records with a non-zero coordinate; false: `why` says what is wrong.
static bool load_camera(const char* path, std::vector<int16_t>& rec, size_t& dropped, std::string& why)
{
    FILE* f = fopen(path, "rb");
    if (!f) { why = "cannot open"; return false; }
    int32_t bytes = 0;
    if (fread(&bytes, 4, 1, f) != 1) { fclose(f); why = "no length word"; return false; }
    if (bytes < 0 || bytes % PCS_POINT_BYTES) { fclose(f); why = "length word " + std::to_string(bytes) + " is not a whole number of records"; return false; }
    std::vector<int16_t> all((size_t)bytes / 2);
    if (bytes && fread(all.data(), 1, (size_t)bytes, f) != (size_t)bytes) { fclose(f); why = "shorter than its length word"; return false; }
    fclose(f);
    rec.clear();
    dropped = 0;
    for (size_t i = 0; i + PCS_POINT_SHORTS <= all.size(); i += PCS_POINT_SHORTS) {
        if (all[i] == 0 && all[i + 1] == 0 && all[i + 2] == 0) { dropped++; continue; }
        rec.insert(rec.end(), all.begin() + i, all.begin() + i + PCS_POINT_SHORTS);
    }
    return true;
}

static bool load_matrices(const char* path, size_t n, std::vector<std::vector<float>>& m, std::string& why)
{
    FILE* f = fopen(path, "r");
    if (!f) { why = "cannot open"; return false; }
    char line[1024];
    while (m.size() < n && fgets(line, sizeof line, f)) {
        char* hash = strchr(line, '#');
        if (hash) *hash = 0;
        std::vector<float> v(16);
        int got = 0, pos = 0, adv = 0;
        while (got < 16 && sscanf(line + pos, " %f%n", &v[got], &adv) == 1) { got++; pos += adv; if (line[pos] == ',') pos++; }
        if (got == 0) continue;
        if (got != 16) { fclose(f); why = "expected 16 values per line"; return false; }
        m.push_back(v);
    }
    fclose(f);
    if (m.size() < n) { why = "only " + std::to_string(m.size()) + " matrices for " + std::to_string(n) + " cameras"; return false; }
    return true;
}

int main(int argc, char** argv)
{
    pcs_align::Options opt;
    std::string why;
    if (!pcs_align::parse(argc, argv, opt, why)) { std::cerr << why << std::endl; usage(); return 2; }
    const size_t n = opt.cams.size();

    std::vector<std::vector<float>> in;
    if (!load_matrices(opt.in_path, n, in, why)) { std::cerr << opt.in_path << ": " << why << std::endl; return 2; }
    std::vector<std::vector<int16_t>> rec(n);
    for (size_t i = 0; i < n; i++) {
        size_t dropped = 0;
        if (!load_camera(opt.cams[i], rec[i], dropped, why)) { std::cerr << opt.cams[i] << ": " << why << std::endl; return 2; }
        std::cout << "Camera " << i << ": " << rec[i].size() / PCS_POINT_SHORTS << " records, " << dropped << " all-zero records dropped" << std::endl;
    }

    // the calls used here read nothing of a stream: one small synthetic one makes the context
    pcs_stream_config sc = pcs_synth::stream_config(64, 48, 0, false);
    pcs_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.device = opt.gpu; cfg.n_streams = 1; cfg.streams = &sc; cfg.downsample = 1;
    pcs_ctx* ctx = nullptr;
    int rc = pcs_create(&ctx, &cfg);
    if (rc != PCS_OK) { std::cerr << "pcs_create: " << pcs_strerror(rc) << ": " << pcs_last_error(nullptr) << std::endl; return 1; }
    const auto die = [&](const char* what) {
        std::cerr << what << ": " << pcs_strerror(rc) << ": " << pcs_last_error(ctx) << std::endl;
        pcs_destroy(ctx);
        return 1;
    };

    // the target: camera ref moved by in[ref]
    const int ref = opt.ref;
    const int n_target = (int)(rec[ref].size() / PCS_POINT_SHORTS);
    void *d_raw = nullptr, *d_target = nullptr, *d_source = nullptr;
    const size_t tb = rec[ref].size() * 2;
    if ((rc = pcs_device_malloc(ctx, &d_raw, tb + 16)) || (rc = pcs_device_malloc(ctx, &d_target, tb + 16))) return die("pcs_device_malloc");
    if (tb && (rc = pcs_memcpy_h2d(ctx, d_raw, rec[ref].data(), tb))) return die("pcs_memcpy_h2d");
    pcs_payload_desc pd;
    memset(&pd, 0, sizeof pd);
    pd.d_payload = static_cast<const int16_t*>(d_raw); pd.n_points = n_target;
    memcpy(pd.transform, in[ref].data(), sizeof pd.transform);
    int total = 0;
    if ((rc = pcs_transform_payloads_device(ctx, 1, &pd, 1, static_cast<int16_t*>(d_target), (size_t)n_target * PCS_POINT_SHORTS, nullptr, &total)))
        return die("pcs_transform_payloads_device");
    if ((rc = pcs_synchronize(ctx))) return die("pcs_synchronize");
    pcs_device_free(ctx, d_raw);

    pcs_align_params params;
    memset(&params, 0, sizeof params);
    params.max_dist_mm = opt.max_dist_mm; params.iterations = opt.iterations; params.source_stride = opt.stride;
    pcs_align_plane_params plane;
    memset(&plane, 0, sizeof plane);
    plane.max_dist_mm = opt.max_dist_mm; plane.iterations = opt.iterations; plane.source_stride = opt.stride;
    plane.normals.radius_mm = opt.normal_radius_mm; plane.normals.min_neighbors = opt.normal_min_neighbors;
    plane.normals.flatness = opt.normal_flatness;

    std::vector<std::vector<float>> out = in;
    std::vector<std::string> note(n);
    int not_refined = 0;
    for (size_t i = 0; i < n; i++) {
        if ((int)i == ref) continue;
        const int ns = (int)(rec[i].size() / PCS_POINT_SHORTS);
        const size_t sb = rec[i].size() * 2;
        if ((rc = pcs_device_malloc(ctx, &d_source, sb + 16))) return die("pcs_device_malloc");
        if (sb && (rc = pcs_memcpy_h2d(ctx, d_source, rec[i].data(), sb))) return die("pcs_memcpy_h2d");
        float refined[16];
        pcs_align_report rep;
        pcs_align_plane_report prep;
        memset(&rep, 0, sizeof rep);
        memset(&prep, 0, sizeof prep);
        if (opt.plane)
            rc = pcs_align_payloads_plane_device(ctx, static_cast<const int16_t*>(d_source), ns, static_cast<const int16_t*>(d_target), n_target,
                                                 &plane, in[i].data(), refined, &prep);
        else
            rc = pcs_align_payloads_device(ctx, static_cast<const int16_t*>(d_source), ns, static_cast<const int16_t*>(d_target), n_target, &params,
                                           in[i].data(), refined, &rep);
        pcs_device_free(ctx, d_source);
        if (rc == PCS_ERR_UNSUPPORTED) {
            note[i] = pcs_last_error(ctx);
            std::cerr << "warning: camera " << i << " not refined: " << note[i] << std::endl;
            not_refined++;
        } else if (rc != PCS_OK) {
            return die(opt.plane ? "pcs_align_payloads_plane_device" : "pcs_align_payloads_device");
        } else {
            out[i].assign(refined, refined + 16);
        }
        if (opt.timing && opt.plane) {
            const double share = prep.last_considered ? 100.0 * (double)prep.last_matched / (double)prep.last_considered : 0.0;
            const double used = prep.last_considered ? 100.0 * (double)prep.last_used / (double)prep.last_considered : 0.0;
            printf("Camera %zu: point to plane, %d iterations, matched %lld of %lld (%.1f %%), with a normal %lld (%.1f %%), rms %.3f -> %.3f mm\n",
                   i, prep.iterations, (long long)prep.last_matched, (long long)prep.last_considered, share, (long long)prep.last_used, used,
                   prep.first_rms_mm, prep.last_rms_mm);
        } else if (opt.timing) {
            const double share = rep.last_considered ? 100.0 * (double)rep.last_matched / (double)rep.last_considered : 0.0;
            printf("Camera %zu: %d iterations, matched %lld of %lld (%.1f %%), rms %.3f -> %.3f mm\n", i, rep.iterations,
                   (long long)rep.last_matched, (long long)rep.last_considered, share, rep.first_rms_mm, rep.last_rms_mm);
        }
    }
    pcs_device_free(ctx, d_target);
    pcs_destroy(ctx);

    FILE* f = fopen(opt.out_path, "w");
    if (!f) { std::cerr << "cannot write " << opt.out_path << std::endl; return 1; }
    for (size_t i = 0; i < n; i++) {
        if (!note[i].empty()) fprintf(f, "# camera %zu not refined: %s\n", i, note[i].c_str());
        for (int k = 0; k < 16; k++) fprintf(f, "%.9g%c", (double)out[i][k], k == 15 ? '\n' : ' ');
    }
    if (fclose(f)) { std::cerr << "cannot write " << opt.out_path << std::endl; return 1; }
    return not_refined ? 3 : 0;
}
