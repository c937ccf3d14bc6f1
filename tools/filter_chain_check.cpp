// filter_chain_check.cpp — pointcloud_stitching_amd/cli/pcs_filter_chain.h over host-memory fakes of the pcs_* calls it makes: which
// entry point every stage gets, with which pointers, counts and sizes, what comes out and what -t prints, over all 16 subsets of
// -O -K -M -E and a host-count or device-count start, and every subset with -E again with -L (the objects form of the cluster call: the same
// cloud out, the table and its count in blocks of the chain's own, the `Objects:` line and the file's lines). A stand-alone program: no GPU, no library, nothing loaded into Python.
//
//   make -C pointcloud_stitching_amd/cli ../../tools/bin/filter_chain_check && tools/bin/filter_chain_check
//   (.../filter_chain_check_asan: the same under the host sanitizers)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <vector>

#include "../pointcloud_stitching_amd/cli/pcs_filter_chain.h"

using namespace pcs_filter_chain;

static int g_failed = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d (%s): %s\n", __LINE__, g_case, #cond); g_failed++; } } while (0)
static char g_case[64] = "";

// ---- the fakes: "device" memory is host memory -------------------------------------------------------------------------------------
struct pcs_ctx { int unused; };

static std::map<const void*, size_t> g_live;      // what pcs_device_malloc handed out and pcs_device_free has not seen yet
static int g_bad_frees = 0, g_syncs = 0;

struct Call {
    int stage; bool counted;
    const int16_t* in; const int32_t* d_n; int n_points, max_points, tag;
    int16_t* out; size_t out_shorts; int32_t* d_n_out; void *block, *models;
    pcs_cluster_object* objects = nullptr; int max_objects = 0; int32_t* d_n_objects = nullptr;      // the objects form of the cluster call; else nullptr, 0, nullptr
};
static std::vector<Call> g_calls;

extern "C" {
int pcs_device_malloc(pcs_ctx*, void** d_ptr, size_t bytes)
{
    *d_ptr = malloc(bytes);      // exactly the request: one byte past it is the sanitizer's
    g_live[*d_ptr] = bytes;
    return PCS_OK;
}
int pcs_device_free(pcs_ctx*, void* d_ptr)
{
    if (!g_live.erase(d_ptr)) { g_bad_frees++; return PCS_ERR_INVALID_ARG; }
    free(d_ptr);
    return PCS_OK;
}
int pcs_memcpy_d2h(pcs_ctx*, void* h_dst, const void* d_src, size_t bytes) { memcpy(h_dst, d_src, bytes); return PCS_OK; }
int pcs_synchronize(pcs_ctx*) { g_syncs++; return PCS_OK; }
}

// Stage s drops every record whose first short is s; the library's own refusals for the output size and in == out.
static int fake_stage(Call c, int* considered, int* kept)
{
    const int n = c.counted ? (*c.d_n < 0 ? 0 : *c.d_n > c.max_points ? c.max_points : *c.d_n) : c.n_points;
    g_calls.push_back(c);
    if (c.out_shorts < (size_t)PCS_POINT_SHORTS * (size_t)(c.counted ? c.max_points : c.n_points) || c.in == c.out) return PCS_ERR_INVALID_ARG;
    int k = 0;
    for (int i = 0; i < n; i++)
        if (c.in[i * PCS_POINT_SHORTS] != c.stage) memcpy(c.out + (k++) * PCS_POINT_SHORTS, c.in + i * PCS_POINT_SHORTS, PCS_POINT_BYTES);
    *c.d_n_out = k; *considered = n; *kept = k;
    return PCS_OK;
}
static void fill(pcs_stat_outlier_stats* st, int considered, int kept)
{
    *st = pcs_stat_outlier_stats{considered, 7000 + kept, 1, 2, 3, 900 + considered, kept, 0};
}
static void fill(pcs_plane_model* models, pcs_plane_stats* st, const pcs_plane_params* p, int considered, int kept)
{
    *st = pcs_plane_stats{considered, p->max_planes, considered - kept, kept, 5, 6, {0, 0}};
    for (int r = 0; r < p->max_planes; r++) models[r] = pcs_plane_model{10 + r, -20 - r, 30 + r, 4000 + r, 50, 600 + r, {1, 2, 3}, 70 + r};
}
static void fill(pcs_cluster_stats* st, int considered, int kept)
{
    *st = pcs_cluster_stats{considered, 80 + considered, 3, 12 + kept, kept, {0, 0, 0}};
}

extern "C" {
int pcs_radius_outlier_device(pcs_ctx*, const int16_t* in, int n, int radius_mm, int, int16_t* out, size_t out_shorts, int32_t* d_n_out)
{
    int a, b;
    return fake_stage({0, false, in, nullptr, n, 0, radius_mm, out, out_shorts, d_n_out, nullptr, nullptr}, &a, &b);
}
int pcs_radius_outlier_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, int radius_mm, int, int16_t* out,
                                      size_t out_shorts, int32_t* d_n_out)
{
    int a, b;
    return fake_stage({0, true, in, d_n, 0, max_points, radius_mm, out, out_shorts, d_n_out, nullptr, nullptr}, &a, &b);
}
int pcs_stat_outlier_device(pcs_ctx*, const int16_t* in, int n, const pcs_stat_outlier_params* p, int16_t* out, size_t out_shorts,
                            int32_t* d_n_out, pcs_stat_outlier_stats* st)
{
    int a, b;
    const int rc = fake_stage({1, false, in, nullptr, n, 0, p->mean_k, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
int pcs_stat_outlier_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_stat_outlier_params* p,
                                    int16_t* out, size_t out_shorts, int32_t* d_n_out, pcs_stat_outlier_stats* st)
{
    int a, b;
    const int rc = fake_stage({1, true, in, d_n, 0, max_points, p->mean_k, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
int pcs_plane_segment_device(pcs_ctx*, const int16_t* in, int n, const pcs_plane_params* p, int16_t* out, size_t out_shorts, int32_t* d_n_out,
                             pcs_plane_model* models, pcs_plane_stats* st)
{
    int a, b;
    const int rc = fake_stage({2, false, in, nullptr, n, 0, p->distance_mm, out, out_shorts, d_n_out, st, models}, &a, &b);
    if (rc == PCS_OK) fill(models, st, p, a, b);
    return rc;
}
int pcs_plane_segment_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_plane_params* p, int16_t* out,
                                     size_t out_shorts, int32_t* d_n_out, pcs_plane_model* models, pcs_plane_stats* st)
{
    int a, b;
    const int rc = fake_stage({2, true, in, d_n, 0, max_points, p->distance_mm, out, out_shorts, d_n_out, st, models}, &a, &b);
    if (rc == PCS_OK) fill(models, st, p, a, b);
    return rc;
}
int pcs_cluster_filter_device(pcs_ctx*, const int16_t* in, int n, const pcs_cluster_params* p, int16_t* out, size_t out_shorts,
                              int32_t* d_n_out, pcs_cluster_stats* st)
{
    int a, b;
    const int rc = fake_stage({3, false, in, nullptr, n, 0, p->tolerance_mm, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
int pcs_cluster_filter_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_cluster_params* p,
                                      int16_t* out, size_t out_shorts, int32_t* d_n_out, pcs_cluster_stats* st)
{
    int a, b;
    const int rc = fake_stage({3, true, in, d_n, 0, max_points, p->tolerance_mm, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
// the objects form: the filter's fake over the struct's output, and kFakeObjects objects of which the table takes what it holds
static const int kFakeObjects = 5;
static pcs_cluster_object fake_object(int k, int kept)
{
    return pcs_cluster_object{10 * k, kept + k, {(int16_t)-k, (int16_t)(k - 7), 3}, {(int16_t)(k + 1), 8, (int16_t)(9 * k)}, 0,
                              {-1000000000000ll * k, 5ll * k, -6}, {255ll * k, 1, 70000000000ll}, 0};
}
static int fake_objects(Call c, const pcs_cluster_objects_out* o)
{
    int a, b;
    c.out = o->out; c.out_shorts = o->out_shorts; c.d_n_out = o->out_points; c.block = o->stats;
    c.objects = o->objects; c.max_objects = o->max_objects; c.d_n_objects = o->n_objects;
    const int rc = fake_stage(c, &a, &b);
    if (rc != PCS_OK) return rc;
    fill(o->stats, a, b);
    *o->n_objects = kFakeObjects;
    for (int k = 0; k < kFakeObjects && k < o->max_objects; k++) o->objects[k] = fake_object(k, b);
    return rc;
}
int pcs_cluster_objects_device(pcs_ctx*, const int16_t* in, int n, const pcs_cluster_params* p, const pcs_cluster_objects_out* o)
{
    return fake_objects({3, false, in, nullptr, n, 0, p->tolerance_mm, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr}, o);
}
int pcs_cluster_objects_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_cluster_params* p,
                                       const pcs_cluster_objects_out* o)
{
    return fake_objects({3, true, in, d_n, 0, max_points, p->tolerance_mm, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr}, o);
}
}

// ---- the check ---------------------------------------------------------------------------------------------------------------------
enum Start { kHost, kDeviceFewer, kDeviceFull };
static const char* const kStartName[] = {"host count", "device count below capacity", "device count at capacity"};
static const int kTag[kStageCount] = {11, 22, 33, 44};      // radius_mm, mean_k, distance_mm, tolerance_mm

// max_objects: 0 without -L, else the table's size (below and above the fakes' object count)
static void check(int subset, Start start, int max_objects = 0)
{
    snprintf(g_case, sizeof g_case, "%s%s%s%s%s%s, %s", subset ? "" : "none", subset & 1 ? "O" : "", subset & 2 ? "K" : "", subset & 4 ? "M" : "",
             subset & 8 ? "E" : "", max_objects ? "L" : "", kStartName[start]);
    pcs_ctx ctx{0};
    const int capacity = 41, n_in = start == kDeviceFewer ? 29 : capacity;
    // the cloud that enters: first shorts 0..5 in turn (every stage drops some and keeps some), the rest tells the records apart
    int16_t* const cloud = static_cast<int16_t*>(malloc((size_t)capacity * PCS_POINT_BYTES));
    for (int i = 0; i < capacity; i++)
        for (int k = 0; k < PCS_POINT_SHORTS; k++) cloud[i * PCS_POINT_SHORTS + k] = (int16_t)(k ? 100 * i + k : i % 6);
    int32_t* const count = static_cast<int32_t*>(malloc(sizeof(int32_t)));
    *count = n_in;
    const Cloud in{cloud, start == kHost ? nullptr : count, start == kHost ? n_in : -12345, capacity};

    Chain chain;
    std::string why;
    int n_enabled = 0;
    const char* const args[kStageCount] = {"11,2", "22,1000,30", "33,16,3,2,5", "44,3"};
    for (int s = 0; s < kStageCount; s++)
        if (subset >> s & 1) { EXPECT(chain.parse(kStages[s].letter, args[s], why)); n_enabled++; }
    EXPECT(!chain.parse('V', "1", why) && chain.any() == (subset != 0));
    EXPECT(!chain.objects());
    if (max_objects) {
        const std::string arg = "some,file.txt," + std::to_string(max_objects);
        EXPECT(chain.parse_objects(arg.c_str(), why) && chain.objects() && chain.objects_file == "some,file.txt" &&
               chain.params.objects.max_objects == max_objects);
    }
    const size_t out_shorts = (size_t)capacity * PCS_POINT_SHORTS;
    g_live.clear();
    if (subset) EXPECT(chain.allocate(&ctx, out_shorts) == PCS_OK);
    const size_t want_blocks = (size_t)(n_enabled < 2 ? n_enabled : 2) + n_enabled + (subset >> 1 & 1) + (subset >> 2 & 1) + (subset >> 3 & 1);
    EXPECT(g_live.size() == want_blocks + (max_objects ? 2 : 0));      // -L: the table and its count word
    if (max_objects) EXPECT(g_live.count(chain.d_objects) && g_live[chain.d_objects] == (size_t)max_objects * sizeof(pcs_cluster_object) &&
                            g_live.count(chain.d_n_objects) && g_live[chain.d_n_objects] == 64);

    // what the fakes' rule predicts, stage by stage
    std::vector<std::vector<int16_t>> want(1, std::vector<int16_t>(cloud, cloud + (size_t)n_in * PCS_POINT_SHORTS));
    std::ostringstream lines;
    for (int s = 0; s < kStageCount; s++) {
        if (!(subset >> s & 1)) continue;
        const std::vector<int16_t>& prev = want.back();
        std::vector<int16_t> next;
        for (size_t i = 0; i < prev.size(); i += PCS_POINT_SHORTS)
            if (prev[i] != s) next.insert(next.end(), prev.begin() + i, prev.begin() + i + PCS_POINT_SHORTS);
        const long long a = (long long)(prev.size() / PCS_POINT_SHORTS), b = (long long)(next.size() / PCS_POINT_SHORTS);
        if (s == 0) lines << "Outlier removal: " << a << " -> " << b << " points\n";
        if (s == 1) lines << "Statistical outlier removal: " << a << " -> " << b << " points (dense " << 7000 + b << ", threshold " << 900 + a << "/256 per k)\n";
        if (s == 2) {
            lines << "Plane segmentation: " << a << " -> " << b << " points (2 planes, " << a - b << " inliers)\n";
            for (int r = 0; r < 2; r++)
                lines << "Plane " << r << ": " << 600 + r << " inliers, normal (" << 10 + r << ", " << -20 - r << ", " << 30 + r << "), offset " << 4000 + r
                      << ", hypothesis " << 70 + r << "\n";
        }
        if (s == 3) lines << "Cluster filter: " << a << " -> " << b << " points (" << 80 + a << " clusters, 3 kept, largest " << 12 + b << ")\n";
        if (s == 3 && max_objects) lines << "Objects: " << kFakeObjects << " (" << (max_objects < kFakeObjects ? max_objects : kFakeObjects) << " written)\n";
        EXPECT(b > 0 && b < a);      // (a stage that keeps everything or nothing would hide a wrong pointer)
        want.push_back(next);
    }

    for (int frame = 0; frame < 2; frame++) {      // the second frame-set goes through the same buffers
        g_calls.clear();
        const Cloud out = chain.run(&ctx, in);
        EXPECT(chain.status == PCS_OK && (int)g_calls.size() == n_enabled);
        if (!subset) {
            EXPECT(out.d == in.d && out.d_n == in.d_n && out.n == in.n && out.capacity == in.capacity);
        } else if ((int)g_calls.size() == n_enabled) {
            Cloud prev = in;
            int k = 0;
            for (int s = 0; s < kStageCount; s++) {
                if (!(subset >> s & 1)) continue;
                const Call& c = g_calls[k++];
                EXPECT(c.stage == s && c.tag == kTag[s]);                                           // O, K, M, E order, each once, its own parameters
                EXPECT(c.counted == (prev.d_n != nullptr));                                         // the counted form iff the count is on the device
                EXPECT(c.counted == (k > 1 || start != kHost));
                EXPECT(c.in == prev.d && c.d_n == prev.d_n);                                        // reads what the stage in front wrote
                if (c.counted) EXPECT(c.max_points == capacity); else EXPECT(c.n_points == n_in);
                EXPECT(c.in != c.out && c.out != cloud && c.d_n_out != c.d_n);
                EXPECT(g_live.count(c.out) && c.out_shorts * sizeof(int16_t) <= g_live[c.out]);     // no more than the buffer holds
                EXPECT(g_live.count(c.d_n_out) && g_live[c.d_n_out] == 64);
                EXPECT((c.block != nullptr) == (s != 0) && (c.models != nullptr) == (s == 2));
                if (c.block) EXPECT(g_live.count(c.block) && g_live[c.block] == kStages[s].block_bytes);
                if (c.models) EXPECT((char*)c.models >= (char*)c.block + sizeof(pcs_plane_stats) &&
                                     (char*)(static_cast<pcs_plane_model*>(c.models) + PCS_PLANE_MAX_PLANES) <= (char*)c.block + g_live[c.block]);
                // the objects form for the cluster stage under -L alone, with the chain's own table and count word
                EXPECT((c.objects != nullptr) == (s == 3 && max_objects != 0));
                if (c.objects) EXPECT(c.objects == chain.d_objects && c.d_n_objects == chain.d_n_objects && c.max_objects == max_objects);
                prev = Cloud{c.out, c.d_n_out, 0, capacity};
            }
            const std::vector<int16_t>& last = want.back();
            EXPECT(out.d == prev.d && out.d_n == prev.d_n && out.capacity == capacity);
            EXPECT(out.d_n && *out.d_n == (int32_t)(last.size() / PCS_POINT_SHORTS));
            EXPECT(out.d_n && *out.d_n >= 0 && memcmp(out.d, last.data(), last.size() * sizeof(int16_t)) == 0);
        }
        std::ostringstream got;
        const int syncs = g_syncs;
        EXPECT(chain.report(got) && got.str() == lines.str());
        EXPECT(g_calls.size() == (size_t)n_enabled && g_syncs - syncs <= (subset ? 1 : 0));      // report launches nothing
        if (max_objects) {      // the file: the header, then the written objects as raw integers
            std::ostringstream file, file_want;
            const int kept = (int)(want.back().size() / PCS_POINT_SHORTS);
            std::vector<pcs_cluster_object> table;
            for (int k = 0; k < kFakeObjects && k < max_objects; k++) table.push_back(fake_object(k, kept));
            pcs_objects::write(file_want, table.data(), (int)table.size());
            EXPECT(chain.write_objects(file) && file.str() == file_want.str() && g_calls.size() == (size_t)n_enabled);
            EXPECT(file.str().rfind("# k label size lo_x lo_y lo_z hi_x hi_y hi_z sum_x sum_y sum_z sum_r sum_g sum_b\n", 0) == 0);
            if (max_objects >= 2) EXPECT(file.str().find("\n1 10 " + std::to_string(kept + 1) + " -1 -6 3 2 8 9 -1000000000000 5 -6 255 1 70000000000\n") != std::string::npos);
        }
        for (int i = 0; i < capacity; i++)                                                           // the caller's cloud is read only
            for (int k = 0; k < PCS_POINT_SHORTS; k++) EXPECT(cloud[i * PCS_POINT_SHORTS + k] == (int16_t)(k ? 100 * i + k : i % 6));
    }
    chain.release();
    EXPECT(g_live.empty() && g_bad_frees == 0);
    chain.release();      // (nothing left to free)
    EXPECT(g_bad_frees == 0);
    free(cloud);
    free(count);
}

int main()
{
    for (int subset = 0; subset < 16; subset++)
        for (Start start : {kHost, kDeviceFewer, kDeviceFull}) {
            check(subset, start);
            if (subset & 8)
                for (int max_objects : {3, 5, 1024}) check(subset, start, max_objects);
        }
    printf(g_failed ? "filter_chain_check: %d check(s) FAILED\n" : "filter_chain_check: all checks passed, no report\n", g_failed);
    fflush(stdout);      // (a leak report at exit must not swallow the lines above)
    return g_failed ? 1 : 0;
}
