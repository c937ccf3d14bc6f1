// filter_chain_check.cpp — pointcloud_stitching_amd/cli/pcs_filter_chain.h over host-memory fakes of the pcs_* calls it makes: which
// entry point every stage gets, with which pointers, counts and sizes, what comes out and what -t prints, over all 32 subsets of
// -X -O -K -M -E and a host-count or device-count start (-X FILE over a fake of the model calls: the imported model and the option's
// parameters reach the subtract call; -X learn: the cloud that enters is learned by the plain or the counted call and passes unchanged), and every subset with -E again with -L (the objects form of the cluster call: the same
// cloud out, the table and its count in blocks of the chain's own, the `Objects:` line and the file's lines), and -J over three subsets with and without -L
// (the table either way, object_of out of the cluster call, one tracker update over the cloud that call read, the file's lines), and -W
// with and without -J and -L (one boxes call behind the cluster call and the tracker's, over the same cloud, object_of and count word,
// into a block of the chain's own; the file's lines; the run's totals), and -H over four subsets, the empty one among them (no stage: one
// plan-view call over the cloud that LEAVES the chain, counted iff that cloud has a device count, into one block of the chain's own; the
// -t line and the three files). A stand-alone program: no GPU, no library, nothing loaded into Python.
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
static char g_case[96] = "";

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
    return fake_stage({1, false, in, nullptr, n, 0, radius_mm, out, out_shorts, d_n_out, nullptr, nullptr}, &a, &b);
}
int pcs_radius_outlier_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, int radius_mm, int, int16_t* out,
                                      size_t out_shorts, int32_t* d_n_out)
{
    int a, b;
    return fake_stage({1, true, in, d_n, 0, max_points, radius_mm, out, out_shorts, d_n_out, nullptr, nullptr}, &a, &b);
}
int pcs_stat_outlier_device(pcs_ctx*, const int16_t* in, int n, const pcs_stat_outlier_params* p, int16_t* out, size_t out_shorts,
                            int32_t* d_n_out, pcs_stat_outlier_stats* st)
{
    int a, b;
    const int rc = fake_stage({2, false, in, nullptr, n, 0, p->mean_k, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
int pcs_stat_outlier_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_stat_outlier_params* p,
                                    int16_t* out, size_t out_shorts, int32_t* d_n_out, pcs_stat_outlier_stats* st)
{
    int a, b;
    const int rc = fake_stage({2, true, in, d_n, 0, max_points, p->mean_k, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
int pcs_plane_segment_device(pcs_ctx*, const int16_t* in, int n, const pcs_plane_params* p, int16_t* out, size_t out_shorts, int32_t* d_n_out,
                             pcs_plane_model* models, pcs_plane_stats* st)
{
    int a, b;
    const int rc = fake_stage({3, false, in, nullptr, n, 0, p->distance_mm, out, out_shorts, d_n_out, st, models}, &a, &b);
    if (rc == PCS_OK) fill(models, st, p, a, b);
    return rc;
}
int pcs_plane_segment_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_plane_params* p, int16_t* out,
                                     size_t out_shorts, int32_t* d_n_out, pcs_plane_model* models, pcs_plane_stats* st)
{
    int a, b;
    const int rc = fake_stage({3, true, in, d_n, 0, max_points, p->distance_mm, out, out_shorts, d_n_out, st, models}, &a, &b);
    if (rc == PCS_OK) fill(models, st, p, a, b);
    return rc;
}
int pcs_cluster_filter_device(pcs_ctx*, const int16_t* in, int n, const pcs_cluster_params* p, int16_t* out, size_t out_shorts,
                              int32_t* d_n_out, pcs_cluster_stats* st)
{
    int a, b;
    const int rc = fake_stage({4, false, in, nullptr, n, 0, p->tolerance_mm, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
int pcs_cluster_filter_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_cluster_params* p,
                                      int16_t* out, size_t out_shorts, int32_t* d_n_out, pcs_cluster_stats* st)
{
    int a, b;
    const int rc = fake_stage({4, true, in, d_n, 0, max_points, p->tolerance_mm, out, out_shorts, d_n_out, st, nullptr}, &a, &b);
    if (rc == PCS_OK) fill(st, a, b);
    return rc;
}
// the background model: a model is a heap block that remembers what made it; subtract is the usual fake with the model checked
struct pcs_background { int cell_mm, max_cells; const void* bytes; size_t n_bytes; int learned; };
static std::map<pcs_background*, int> g_models;      // live models
struct LearnCall { pcs_background* bg; bool counted; const int16_t* in; const int32_t* d_n; int n_points, max_points; };
static std::vector<LearnCall> g_learns;
static const int kFakeCells = 321, kFakeFrames = 9;
static void fill(pcs_background_stats* st, const pcs_background_params* p, int considered, int kept)
{
    *st = pcs_background_stats{considered, kept, considered - kept, kFakeCells, kFakeFrames, p->min_seen, 0, 0};
}
int pcs_background_create(pcs_ctx*, int cell_mm, int max_cells, pcs_background** out)
{
    *out = new pcs_background{cell_mm, max_cells, nullptr, 0, 0};
    g_models[*out] = 1;
    return PCS_OK;
}
int pcs_background_import(pcs_ctx*, const void* bytes, size_t n_bytes, int max_cells, pcs_background** out)
{
    *out = new pcs_background{0, max_cells, bytes, n_bytes, 0};
    g_models[*out] = 1;
    return PCS_OK;
}
int pcs_background_destroy(pcs_ctx*, pcs_background* bg)
{
    if (!g_models.erase(bg)) { g_bad_frees++; return PCS_ERR_INVALID_ARG; }
    delete bg;
    return PCS_OK;
}
int pcs_background_learn_device(pcs_ctx*, pcs_background* bg, const int16_t* in, int n)
{
    g_learns.push_back({bg, false, in, nullptr, n, 0});
    bg->learned++;
    return PCS_OK;
}
int pcs_background_learn_device_counted(pcs_ctx*, pcs_background* bg, const int16_t* in, const int32_t* d_n, int max_points)
{
    g_learns.push_back({bg, true, in, d_n, 0, max_points});
    bg->learned++;
    return PCS_OK;
}
int pcs_background_subtract_device(pcs_ctx*, pcs_background* bg, const int16_t* in, int n, const pcs_background_params* p, int16_t* out,
                                   size_t out_shorts, int32_t* d_n_out, pcs_background_stats* st)
{
    int a, b;
    if (!g_models.count(bg)) return PCS_ERR_INVALID_ARG;
    const int rc = fake_stage({0, false, in, nullptr, n, 0, p->min_seen, out, out_shorts, d_n_out, st, bg}, &a, &b);
    if (rc == PCS_OK) fill(st, p, a, b);
    return rc;
}
int pcs_background_subtract_device_counted(pcs_ctx*, pcs_background* bg, const int16_t* in, const int32_t* d_n, int max_points,
                                           const pcs_background_params* p, int16_t* out, size_t out_shorts, int32_t* d_n_out,
                                           pcs_background_stats* st)
{
    int a, b;
    if (!g_models.count(bg)) return PCS_ERR_INVALID_ARG;
    const int rc = fake_stage({0, true, in, d_n, 0, max_points, p->min_seen, out, out_shorts, d_n_out, st, bg}, &a, &b);
    if (rc == PCS_OK) fill(st, p, a, b);
    return rc;
}
int pcs_background_info(pcs_ctx*, pcs_background* bg, struct pcs_background_info* info)
{
    *info = {bg->cell_mm, bg->max_cells, (uint32_t)kFakeCells, (uint32_t)bg->learned, bg->max_cells == 7 ? 1 : 0, 0};      // max_cells 7: "overflowed"
    return PCS_OK;
}
size_t pcs_background_export_bound(int max_cells) { return 32 + 12 * (size_t)max_cells; }
int pcs_background_export(pcs_ctx*, pcs_background* bg, void* out, size_t capacity, size_t* n)
{
    if (capacity < 32) return PCS_ERR_CAPACITY;
    memset(out, 0, 32);
    memcpy(out, "PCB1", 4);
    static_cast<char*>(out)[8] = (char)bg->cell_mm;
    *n = 32;
    return PCS_OK;
}
int pcs_background_validate(const void*, size_t n_bytes, struct pcs_background_info* info)
{
    *info = {40, 0, (uint32_t)((n_bytes - 32) / 12), (uint32_t)kFakeFrames, 0, 0};
    return n_bytes >= 32 ? PCS_OK : PCS_ERR_INVALID_ARG;
}
const char* pcs_last_error(const pcs_ctx*) { return "fake"; }
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
    return fake_objects({4, false, in, nullptr, n, 0, p->tolerance_mm, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr}, o);
}
int pcs_cluster_objects_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_cluster_params* p,
                                       const pcs_cluster_objects_out* o)
{
    return fake_objects({4, true, in, d_n, 0, max_points, p->tolerance_mm, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr}, o);
}
// the object tracker (-J): a heap block that remembers what made it; an update is recorded, and writes what the file's lines are made of
struct pcs_tracker { int cell_mm, max_cells, max_objects, updates; };
static std::map<pcs_tracker*, int> g_trackers;
struct TrackCall {
    pcs_tracker* tr; bool counted; const int16_t* in; const int32_t* d_n; int n_points, max_points;
    const int32_t *object_of, *d_n_objects; int max_objects, min_votes; pcs_track* tracks; pcs_track_stats* stats;
};
static std::vector<TrackCall> g_track_calls;
static pcs_track fake_track(int k, int update) { return pcs_track{(1ll << 33) + k, update, k - 1, 7 * k, 0}; }
static int fake_update(TrackCall c)
{
    g_track_calls.push_back(c);
    for (int k = 0; k < kFakeObjects && k < c.max_objects; k++) c.tracks[k] = fake_track(k, c.tr->updates);
    *c.stats = pcs_track_stats{40, 30, kFakeObjects, 3, 2, 1, 0, ++c.tr->updates};
    return PCS_OK;
}
int pcs_tracker_create(pcs_ctx*, int cell_mm, int max_cells, int max_objects, pcs_tracker** out)
{
    *out = new pcs_tracker{cell_mm, max_cells, max_objects, 0};
    g_trackers[*out] = 1;
    return PCS_OK;
}
int pcs_tracker_destroy(pcs_ctx*, pcs_tracker* tr)
{
    if (!g_trackers.erase(tr)) { g_bad_frees++; return PCS_ERR_INVALID_ARG; }
    delete tr;
    return PCS_OK;
}
int pcs_tracker_update_device(pcs_ctx*, pcs_tracker* tr, const int16_t* in, int n, const int32_t* object_of, const int32_t* d_m, int max_objects,
                              const pcs_track_params* p, pcs_track* tracks, pcs_track_stats* st)
{
    return fake_update({tr, false, in, nullptr, n, 0, object_of, d_m, max_objects, p->min_votes, tracks, st});
}
int pcs_tracker_update_device_counted(pcs_ctx*, pcs_tracker* tr, const int16_t* in, const int32_t* d_n, int max_points, const int32_t* object_of,
                                      const int32_t* d_m, int max_objects, const pcs_track_params* p, pcs_track* tracks, pcs_track_stats* st)
{
    return fake_update({tr, true, in, d_n, 0, max_points, object_of, d_m, max_objects, p->min_votes, tracks, st});
}
}
// object boxes (-W): a call is recorded, with how many tracker updates and cluster calls stood in front of it, and writes what the
// file's lines are made of
struct BoxCall {
    bool counted; const int16_t* in; const int32_t* d_n; int n_points, max_points;
    const int32_t *object_of, *d_n_objects; int max_objects; pcs_object_box* boxes; size_t calls_before, updates_before;
};
static std::vector<BoxCall> g_box_calls;
static pcs_object_box fake_box(int k, int call)
{
    pcs_object_box b{};
    b.count = 100 + k; b.sum_xyz[0] = -7ll * k; b.sum_xyz[1] = 1ll << 40; b.sum_xyz[2] = call;
    for (int q = 0; q < 6; q++) b.m2[q] = (1ll << 47) - q * k;
    for (int a = 0; a < 3; a++)
        for (int c = 0; c < 3; c++) b.axis[a][c] = (int16_t)(a == c ? 16384 : -(3 * a + c));
    b.rank = (int16_t)(k % 2 ? 3 : 2);
    for (int a = 0; a < 3; a++) { b.ext_lo[a] = -536870912 + a; b.ext_hi[a] = 536854528 - k; }
    return b;
}
static int fake_boxes(BoxCall c)
{
    c.calls_before = g_calls.size(); c.updates_before = g_track_calls.size();
    g_box_calls.push_back(c);
    for (int k = 0; k < kFakeObjects && k < c.max_objects; k++) c.boxes[k] = fake_box(k, (int)g_box_calls.size() - 1);
    return PCS_OK;
}
extern "C" {
int pcs_object_boxes_device(pcs_ctx*, const int16_t* in, int n, const int32_t* object_of, const int32_t* d_m, int max_objects, pcs_object_box* boxes)
{
    return fake_boxes({false, in, nullptr, n, 0, object_of, d_m, max_objects, boxes, 0, 0});
}
int pcs_object_boxes_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const int32_t* object_of, const int32_t* d_m,
                                    int max_objects, pcs_object_box* boxes)
{
    return fake_boxes({true, in, d_n, 0, max_points, object_of, d_m, max_objects, boxes, 0, 0});
}
}

// ---- the check ---------------------------------------------------------------------------------------------------------------------
enum Start { kHost, kDeviceFewer, kDeviceFull };
// plan-view maps (-H): a call is recorded with how many stage calls stood in front of it, and fills the rasters with what the files show
struct PlanCall {
    bool counted; const int16_t* in; const int32_t* d_n; int n_points, max_points; pcs_plan_params params; pcs_plan_maps maps; size_t calls_before;
};
static std::vector<PlanCall> g_plan_calls;
static int fake_plan(PlanCall c)
{
    c.calls_before = g_calls.size();
    const int cells = c.params.width * c.params.height, call = (int)g_plan_calls.size();
    for (int i = 0; i < cells; i++) {
        c.maps.count[i] = i % 3 == 2 ? 0u : (uint32_t)(70000 * (i % 2) + i + call);
        c.maps.top[i] = (int16_t)(i % 3 == 2 ? 0 : 300 * i - 32768 + call);
        c.maps.bottom[i] = (int16_t)-i;
        for (int k = 0; k < 3; k++) c.maps.rgb[3 * i + k] = (uint8_t)(i % 3 == 2 ? 0 : 16 * i + k + call);
    }
    *c.maps.stats = pcs_plan_stats{c.counted ? *c.d_n : c.n_points, 1000 + call, 900 + call, cells - cells / 3, 70000, {0, 0, 0}};
    g_plan_calls.push_back(c);
    return PCS_OK;
}
extern "C" {
int pcs_plan_view_device(pcs_ctx*, const int16_t* in, int n, const pcs_plan_params* p, const pcs_plan_maps* m)
{
    return fake_plan({false, in, nullptr, n, 0, *p, *m, 0});
}
int pcs_plan_view_device_counted(pcs_ctx*, const int16_t* in, const int32_t* d_n, int max_points, const pcs_plan_params* p, const pcs_plan_maps* m)
{
    return fake_plan({true, in, d_n, 0, max_points, *p, *m, 0});
}
}

static const char* const kStartName[] = {"host count", "device count below capacity", "device count at capacity"};
static const int kTag[kStageCount] = {5, 11, 22, 33, 44};      // min_seen, radius_mm, mean_k, distance_mm, tolerance_mm

// max_objects: 0 without -L, else the table's size (below and above the fakes' object count)
static void check(int subset, Start start, int max_objects = 0)
{
    snprintf(g_case, sizeof g_case, "%s%s%s%s%s%s%s, %s", subset ? "" : "none", subset & 1 ? "X" : "", subset & 2 ? "O" : "", subset & 4 ? "K" : "",
             subset & 8 ? "M" : "", subset & 16 ? "E" : "", max_objects ? "L" : "", kStartName[start]);
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
    const char* const args[kStageCount] = {"some,model.pcb,50,0", "11,2", "22,1000,30", "33,16,3,2,5", "44,3"};
    for (int s = 0; s < kStageCount; s++)
        if (subset >> s & 1) { EXPECT(s ? chain.parse(kStages[s].letter, args[s], why) : chain.parse_background(args[s], why)); n_enabled++; }
    if (subset & 1) {      // -X FILE: the option's words, then the file (a fake container of 3 cells: the fake validator says 9 frames)
        EXPECT(chain.params.background.file == "some,model.pcb" && chain.params.background.min_percent == 50 && chain.params.background.dilate == 0);
        EXPECT(!chain.parse_background("other.pcb", why) && why.find("twice") != std::string::npos);
        EXPECT(!chain.parse_background("learn:other.pcb,40", why) && why.find("one form") != std::string::npos);
        chain.background_bytes.assign(32 + 3 * 12, 0);
        struct pcs_background_info info{};
        pcs_background_validate(chain.background_bytes.data(), chain.background_bytes.size(), &info);
        chain.params.background.frames = info.frames;
        chain.params.background.params = pcs_background_params{pcs_background_cli::min_seen_of(info.frames, 50), 0, PCS_BACKGROUND_MODE_REMOVE, 0};
        EXPECT(chain.params.background.params.min_seen == 5);      // ceil(9 x 50 / 100)
    }
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
    const size_t want_blocks = (size_t)(n_enabled < 2 ? n_enabled : 2) + n_enabled + (subset & 1) + (subset >> 2 & 1) + (subset >> 3 & 1) + (subset >> 4 & 1);
    EXPECT(g_live.size() == want_blocks + (max_objects ? 2 : 0));      // -L: the table and its count word
    EXPECT(g_models.size() == (size_t)(subset & 1));      // -X FILE: the model imported once, from the file's bytes, with room for its cells
    if (subset & 1) EXPECT(g_models.count(chain.params.background.model) && chain.params.background.model->bytes == chain.background_bytes.data() &&
                           chain.params.background.model->n_bytes == chain.background_bytes.size() && chain.params.background.model->max_cells == 3);
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
        if (s == 0) lines << "Background subtraction: " << a << " -> " << b << " points (" << kFakeCells << " cells, seen >= 5 of " << kFakeFrames << ", dilate 0)\n";
        if (s == 1) lines << "Outlier removal: " << a << " -> " << b << " points\n";
        if (s == 2) lines << "Statistical outlier removal: " << a << " -> " << b << " points (dense " << 7000 + b << ", threshold " << 900 + a << "/256 per k)\n";
        if (s == 3) {
            lines << "Plane segmentation: " << a << " -> " << b << " points (2 planes, " << a - b << " inliers)\n";
            for (int r = 0; r < 2; r++)
                lines << "Plane " << r << ": " << 600 + r << " inliers, normal (" << 10 + r << ", " << -20 - r << ", " << 30 + r << "), offset " << 4000 + r
                      << ", hypothesis " << 70 + r << "\n";
        }
        if (s == 4) lines << "Cluster filter: " << a << " -> " << b << " points (" << 80 + a << " clusters, 3 kept, largest " << 12 + b << ")\n";
        if (s == 4 && max_objects) lines << "Objects: " << kFakeObjects << " (" << (max_objects < kFakeObjects ? max_objects : kFakeObjects) << " written)\n";
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
                EXPECT(g_learns.empty());
                EXPECT(c.in == prev.d && c.d_n == prev.d_n);                                        // reads what the stage in front wrote
                if (c.counted) EXPECT(c.max_points == capacity); else EXPECT(c.n_points == n_in);
                EXPECT(c.in != c.out && c.out != cloud && c.d_n_out != c.d_n);
                EXPECT(g_live.count(c.out) && c.out_shorts * sizeof(int16_t) <= g_live[c.out]);     // no more than the buffer holds
                EXPECT(g_live.count(c.d_n_out) && g_live[c.d_n_out] == 64);
                EXPECT((c.block != nullptr) == (s != 1) && (c.models != nullptr) == (s == 3 || s == 0));
                if (s == 0) EXPECT(c.models == chain.params.background.model);                      // (the fake keeps the model where the plane call keeps its models)
                if (c.block) EXPECT(g_live.count(c.block) && g_live[c.block] == kStages[s].block_bytes);
                if (c.models && s == 3) EXPECT((char*)c.models >= (char*)c.block + sizeof(pcs_plane_stats) &&
                                     (char*)(static_cast<pcs_plane_model*>(c.models) + PCS_PLANE_MAX_PLANES) <= (char*)c.block + g_live[c.block]);
                // the objects form for the cluster stage under -L alone, with the chain's own table and count word
                EXPECT((c.objects != nullptr) == (s == 4 && max_objects != 0));
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
    EXPECT(g_live.empty() && g_models.empty() && g_bad_frees == 0);
    chain.release();      // (nothing left to free)
    EXPECT(g_bad_frees == 0);
    free(cloud);
    free(count);
}

// -X learn: over the stages of `subset` (none of them X): the cloud that enters is learned once per frame-set, by the counted call iff its
// count is on the device, and the stages see what they see without it; the model goes to its file when the run ends.
static void check_learn(int subset, Start start, int max_cells)
{
    snprintf(g_case, sizeof g_case, "learn over subset %d, %s, max_cells %d", subset, kStartName[start], max_cells);
    pcs_ctx ctx{0};
    const int capacity = 41, n_in = start == kDeviceFewer ? 29 : capacity;
    std::vector<int16_t> cloud((size_t)capacity * PCS_POINT_SHORTS);
    for (int i = 0; i < capacity; i++)
        for (int k = 0; k < PCS_POINT_SHORTS; k++) cloud[i * PCS_POINT_SHORTS + k] = (int16_t)(k ? 100 * i + k : i % 6);
    int32_t count = n_in;
    const Cloud in{cloud.data(), start == kHost ? nullptr : &count, start == kHost ? n_in : -12345, capacity};
    Chain chain;
    std::string why;
    const char* const args[kStageCount] = {"", "11,2", "22,1000,30", "33,16,3,2,5", "44,3"};
    int n_enabled = 0;
    for (int s = 1; s < kStageCount; s++)
        if (subset >> s & 1) { EXPECT(chain.parse(kStages[s].letter, args[s], why)); n_enabled++; }
    const std::string file = "filter_chain_check_model.tmp";
    EXPECT(!chain.parse_background("learn:model.pcb", why) && !chain.parse_background("learn:model.pcb,0", why) && why.find("cell_mm") != std::string::npos);
    EXPECT(!chain.parse_background("learn:model.pcb,40,x", why) && !chain.learning());
    EXPECT(chain.parse_background(("learn:" + file + ",40," + std::to_string(max_cells)).c_str(), why) && chain.learning() && chain.any());
    EXPECT(chain.learn.file == file && chain.learn.cell_mm == 40 && chain.learn.max_cells == max_cells);
    EXPECT(!chain.parse_background("learn:again.pcb,40", why) && why.find("twice") != std::string::npos);
    EXPECT(!chain.parse_background("model.pcb", why) && why.find("one form") != std::string::npos);
    g_live.clear(); g_learns.clear();
    EXPECT(chain.allocate(&ctx, (size_t)capacity * PCS_POINT_SHORTS) == PCS_OK);
    EXPECT(g_models.size() == 1 && g_models.count(chain.learn.model) && chain.learn.model->cell_mm == 40 && chain.learn.model->max_cells == max_cells);
    for (int frame = 0; frame < 3; frame++) {
        g_calls.clear();
        const Cloud out = chain.run(&ctx, in);
        EXPECT(chain.status == PCS_OK && (int)g_calls.size() == n_enabled && (int)g_learns.size() == frame + 1);
        const LearnCall& l = g_learns.back();
        EXPECT(l.bg == chain.learn.model && l.counted == (start != kHost) && l.in == cloud.data() && l.d_n == in.d_n);
        if (l.counted) EXPECT(l.max_points == capacity); else EXPECT(l.n_points == n_in);
        if (!n_enabled) EXPECT(out.d == in.d && out.d_n == in.d_n && out.n == in.n && out.capacity == in.capacity);      // unchanged
        else EXPECT(g_calls[0].in == cloud.data() && g_calls[0].d_n == in.d_n);                                           // the first stage reads the same cloud
    }
    std::ostringstream said, err;
    remove(file.c_str());
    const int status = chain.finish_learning(said, err, true);
    FILE* f = fopen(file.c_str(), "rb");
    if (max_cells == 7) {      // the fake's "overflowed" model: status 1, a message, no file
        EXPECT(status == 1 && said.str().empty() && err.str().find("max_cells 7") != std::string::npos && !f);
    } else {
        char head[40] = "";
        EXPECT(status == 0 && err.str().empty() && f && fread(head, 1, 40, f) == 32 && memcmp(head, "PCB1", 4) == 0 && head[8] == 40);
        EXPECT(said.str() == "Background learned: 3 frame-sets, " + std::to_string(kFakeCells) + " cells of 40 mm\n");
    }
    if (f) fclose(f);
    remove(file.c_str());
    std::ostringstream quiet;
    if (max_cells != 7) EXPECT(chain.finish_learning(quiet, err, false) == 0 && quiet.str().empty());
    remove(file.c_str());
    chain.release();
    EXPECT(g_live.empty() && g_models.empty() && g_bad_frees == 0);
    g_learns.clear();
}

// -J over the stages of `subset` (E among them, X not), with -L (max_objects) or without (0): the table is made either way, the E stage
// hands object_of out, and behind it one tracker update reads the cloud THAT stage read, counted iff that stage's call was; the
// file gets the header once and every frame-set's lines; release() leaves nothing.
static void check_tracks(int subset, Start start, int max_objects)
{
    snprintf(g_case, sizeof g_case, "tracks over subset %d, %s, -L %d", subset, kStartName[start], max_objects);
    pcs_ctx ctx{0};
    const int capacity = 41, n_in = start == kDeviceFewer ? 29 : capacity;
    std::vector<int16_t> cloud((size_t)capacity * PCS_POINT_SHORTS);
    for (int i = 0; i < capacity; i++)
        for (int k = 0; k < PCS_POINT_SHORTS; k++) cloud[i * PCS_POINT_SHORTS + k] = (int16_t)(k ? 100 * i + k : i % 6);
    int32_t count = n_in;
    const Cloud in{cloud.data(), start == kHost ? nullptr : &count, start == kHost ? n_in : -12345, capacity};
    Chain chain;
    std::string why;
    const char* const args[kStageCount] = {"", "11,2", "22,1000,30", "33,16,3,2,5", "44,3"};
    int n_enabled = 0;
    for (int s = 1; s < kStageCount; s++)
        if (subset >> s & 1) { EXPECT(chain.parse(kStages[s].letter, args[s], why)); n_enabled++; }
    const std::string file = "filter_chain_check_tracks.tmp";
    EXPECT(!chain.tracks() && !chain.parse_tracks("t.txt,0", why) && why.find("cell_mm") != std::string::npos && !chain.tracks());
    EXPECT(!chain.parse_tracks("t.txt,100,x", why) && !chain.parse_tracks(",100", why) && !chain.parse_tracks("t.txt,1,2,3", why));
    EXPECT(chain.parse_tracks((file + ",250,7").c_str(), why) && chain.tracks() && chain.tracks_file == file);
    EXPECT(chain.params.tracks.cell_mm == 250 && chain.params.tracks.params.min_votes == 7);
    if (max_objects) EXPECT(chain.parse_objects(("objects.txt," + std::to_string(max_objects)).c_str(), why));
    chain.finish_options();
    const int table = max_objects ? max_objects : pcs_objects::kDefaultMaxObjects;      // without -L: the table at -L's default size
    EXPECT(chain.params.objects.max_objects == table && chain.objects() == (max_objects != 0));
    g_live.clear(); g_track_calls.clear();
    EXPECT(chain.allocate(&ctx, (size_t)capacity * PCS_POINT_SHORTS) == PCS_OK);
    pcs_tracker* const tr = chain.params.tracks.tracker;
    EXPECT(g_trackers.size() == 1 && g_trackers.count(tr) && tr->cell_mm == 250 && tr->max_cells == capacity && tr->max_objects == table);
    EXPECT(g_live.count(chain.d_object_of) && g_live[chain.d_object_of] >= (size_t)capacity * sizeof(int32_t));
    EXPECT(g_live.count(chain.d_tracks) && g_live[chain.d_tracks] == (size_t)table * sizeof(pcs_track));
    EXPECT(g_live.count(chain.d_track_stats) && g_live[chain.d_track_stats] == sizeof(pcs_track_stats));
    EXPECT(g_live.count(chain.d_objects) && g_live[chain.d_objects] == (size_t)table * sizeof(pcs_cluster_object));
    remove(file.c_str());
    EXPECT(chain.open_tracks());
    std::ostringstream want;
    pcs_tracks::write_header(want);
    for (int frame = 0; frame < 3; frame++) {
        g_calls.clear();
        const Cloud out = chain.run(&ctx, in);
        EXPECT(chain.status == PCS_OK && (int)g_calls.size() == n_enabled && (int)g_track_calls.size() == frame + 1 && out.d_n);
        const Call& e = g_calls.back();
        const TrackCall& t = g_track_calls.back();
        EXPECT(e.stage == 4 && e.objects == chain.d_objects && e.max_objects == table);
        EXPECT(t.tr == tr && t.in == e.in && t.d_n == e.d_n && t.counted == e.counted);          // the cloud the E stage read, by the same rule
        EXPECT(t.counted == (n_enabled > 1 || start != kHost));
        if (t.counted) EXPECT(t.max_points == capacity); else EXPECT(t.n_points == n_in);
        EXPECT(t.object_of == chain.d_object_of && t.d_n_objects == chain.d_n_objects && t.max_objects == table && t.min_votes == 7);
        EXPECT(t.tracks == chain.d_tracks && t.stats == chain.d_track_stats);
        EXPECT(chain.write_tracks(why) && g_track_calls.size() == (size_t)frame + 1);               // (writing launches nothing)
        std::vector<pcs_cluster_object> objects;
        std::vector<pcs_track> tracks;
        for (int k = 0; k < kFakeObjects && k < table; k++) { objects.push_back(fake_object(k, *out.d_n)); tracks.push_back(fake_track(k, frame)); }
        pcs_tracks::write(want, frame, tracks.data(), objects.data(), (int)tracks.size());
        std::ostringstream lines;
        EXPECT(chain.report(lines) && (lines.str().find("Objects:") != std::string::npos) == (max_objects != 0));
    }
    EXPECT(chain.tracks_frames == 3 && chain.tracks_born == 6 && chain.tracks_continued == 9 && chain.tracks_lost == 3);
    std::ifstream f(file);
    std::stringstream got;
    got << f.rdbuf();
    EXPECT(got.str() == want.str());
    EXPECT(got.str().rfind("# frame k id age prev votes label size lo_x lo_y lo_z hi_x hi_y hi_z sum_x sum_y sum_z\n", 0) == 0);
    if (table >= 2) EXPECT(got.str().find("\n2 1 8589934593 2 0 7 10 ") != std::string::npos);
    chain.release();
    EXPECT(g_live.empty() && g_trackers.empty() && g_bad_frees == 0);
    chain.release();      // (nothing left to free)
    EXPECT(g_bad_frees == 0);
    chain.tracks_stream.close();
    remove(file.c_str());
}

// -W over the stages of `subset` (E among them, X not), with -J or without, with -L (max_objects) or without (0): the table and
// object_of are made either way; behind the E stage's call, and behind the tracker's update where -J is given, one boxes call reads
// the cloud THAT stage read, counted iff that stage's call was, with the stage's object_of and count word; the file gets the header
// once and every frame-set's lines; release() leaves nothing.
static void check_boxes(int subset, Start start, int max_objects, bool with_tracks)
{
    snprintf(g_case, sizeof g_case, "boxes over subset %d, %s, -L %d, -J %d", subset, kStartName[start], max_objects, (int)with_tracks);
    pcs_ctx ctx{0};
    const int capacity = 41, n_in = start == kDeviceFewer ? 29 : capacity;
    std::vector<int16_t> cloud((size_t)capacity * PCS_POINT_SHORTS);
    for (int i = 0; i < capacity; i++)
        for (int k = 0; k < PCS_POINT_SHORTS; k++) cloud[i * PCS_POINT_SHORTS + k] = (int16_t)(k ? 100 * i + k : i % 6);
    int32_t count = n_in;
    const Cloud in{cloud.data(), start == kHost ? nullptr : &count, start == kHost ? n_in : -12345, capacity};
    Chain chain;
    std::string why;
    const char* const args[kStageCount] = {"", "11,2", "22,1000,30", "33,16,3,2,5", "44,3"};
    int n_enabled = 0;
    for (int s = 1; s < kStageCount; s++)
        if (subset >> s & 1) { EXPECT(chain.parse(kStages[s].letter, args[s], why)); n_enabled++; }
    const std::string file = "filter_chain_check_boxes.tmp", tracks_file = "filter_chain_check_boxes_tracks.tmp";
    EXPECT(!chain.boxes() && !chain.parse_boxes("", why) && why.find("empty") != std::string::npos && !chain.boxes());
    EXPECT(!chain.parse_boxes("b.txt,5", why) && !chain.parse_boxes("-E", why) && !chain.parse_boxes(",", why) && !chain.boxes());
    EXPECT(chain.parse_boxes("-", why) && chain.boxes() && chain.boxes_file == "-");
    EXPECT(chain.parse_boxes(file.c_str(), why) && chain.boxes() && chain.boxes_file == file);
    if (with_tracks) EXPECT(chain.parse_tracks((tracks_file + ",250,7").c_str(), why));
    if (max_objects) EXPECT(chain.parse_objects(("objects.txt," + std::to_string(max_objects)).c_str(), why));
    chain.finish_options();
    const int table = max_objects ? max_objects : pcs_objects::kDefaultMaxObjects;      // without -L: the table at -L's default size
    EXPECT(chain.params.objects.max_objects == table && chain.objects() == (max_objects != 0) && chain.tracks() == with_tracks);
    g_live.clear(); g_track_calls.clear(); g_box_calls.clear();
    EXPECT(chain.allocate(&ctx, (size_t)capacity * PCS_POINT_SHORTS) == PCS_OK);
    EXPECT(g_trackers.size() == (with_tracks ? 1u : 0u));
    EXPECT(g_live.count(chain.d_object_of) && g_live[chain.d_object_of] >= (size_t)capacity * sizeof(int32_t));
    EXPECT(g_live.count(chain.d_boxes) && g_live[chain.d_boxes] == (size_t)table * sizeof(pcs_object_box));
    EXPECT(g_live.count(chain.d_objects) && g_live[chain.d_objects] == (size_t)table * sizeof(pcs_cluster_object));
    EXPECT(with_tracks ? g_live.count(chain.d_tracks) == 1 : chain.d_tracks == nullptr && chain.d_track_stats == nullptr);
    remove(file.c_str());
    EXPECT(chain.open_boxes());
    if (with_tracks) EXPECT(chain.open_tracks());
    std::ostringstream want;
    pcs_boxes::write_header(want);
    long long rank3 = 0;
    for (int frame = 0; frame < 3; frame++) {
        g_calls.clear();
        const Cloud out = chain.run(&ctx, in);
        EXPECT(chain.status == PCS_OK && (int)g_calls.size() == n_enabled && (int)g_box_calls.size() == frame + 1 && out.d_n);
        EXPECT((int)g_track_calls.size() == (with_tracks ? frame + 1 : 0));
        const Call& e = g_calls.back();
        const BoxCall& b = g_box_calls.back();
        EXPECT(e.stage == 4 && e.objects == chain.d_objects && e.max_objects == table);
        EXPECT(b.calls_before == (size_t)n_enabled && b.updates_before == g_track_calls.size());    // behind the E stage's call and the tracker's
        EXPECT(b.in == e.in && b.d_n == e.d_n && b.counted == e.counted);                          // the cloud the E stage read, by the same rule
        EXPECT(b.counted == (n_enabled > 1 || start != kHost));
        if (b.counted) EXPECT(b.max_points == capacity); else EXPECT(b.n_points == n_in);
        EXPECT(b.object_of == chain.d_object_of && b.d_n_objects == chain.d_n_objects && b.max_objects == table && b.boxes == chain.d_boxes);
        if (with_tracks) EXPECT(g_track_calls.back().object_of == b.object_of && g_track_calls.back().in == b.in);
        EXPECT(chain.write_boxes(why) && g_box_calls.size() == (size_t)frame + 1);                  // (writing launches nothing)
        if (with_tracks) EXPECT(chain.write_tracks(why));
        std::vector<pcs_object_box> entries;
        for (int k = 0; k < kFakeObjects && k < table; k++) { entries.push_back(fake_box(k, frame)); rank3 += entries.back().rank == 3; }
        pcs_boxes::write(want, frame, entries.data(), (int)entries.size());
    }
    const int written = kFakeObjects < table ? kFakeObjects : table;
    EXPECT(chain.boxes_frames == 3 && chain.boxes_objects == 3 * written && chain.boxes_rank3 == rank3);
    std::ifstream f(file);
    std::stringstream got;
    got << f.rdbuf();
    EXPECT(got.str() == want.str());
    EXPECT(got.str().rfind("# frame k count sum_x sum_y sum_z m_xx m_xy m_xz m_yy m_yz m_zz a0_x a0_y a0_z a1_x a1_y a1_z a2_x a2_y a2_z rank "
                           "lo_0 lo_1 lo_2 hi_0 hi_1 hi_2 reserved\n", 0) == 0);
    if (table >= 2)
        EXPECT(got.str().find("\n2 1 101 -7 1099511627776 2 140737488355328 140737488355327 140737488355326 140737488355325 140737488355324 "
                              "140737488355323 16384 -1 -2 -3 16384 -5 -6 -7 16384 3 -536870912 -536870911 -536870910 536854527 536854527 "
                              "536854527 0\n") != std::string::npos);
    {   // every line: 29 integers
        std::string line;
        std::getline(got, line);
        while (std::getline(got, line)) {
            int fields = 1;
            for (char ch : line) fields += ch == ' ';
            EXPECT(fields == 29);
        }
    }
    chain.release();
    EXPECT(g_live.empty() && g_trackers.empty() && g_bad_frees == 0);
    chain.release();      // (nothing left to free)
    EXPECT(g_bad_frees == 0);
    chain.boxes_stream.close();
    chain.tracks_stream.close();
    remove(file.c_str());
    remove(tracks_file.c_str());
}

// -H over the stages of `subset` (X not among them), the empty subset included: any() is true for -H alone; one block holds the four
// rasters and the statistics block; behind run() one plan-view call reads the cloud run() RETURNED, counted iff that cloud has a device
// count; the -t line and the three files are the header's own writers over what the last call left; release() leaves nothing.
static void check_plan(int subset, Start start)
{
    snprintf(g_case, sizeof g_case, "plan view over subset %d, %s", subset, kStartName[start]);
    pcs_ctx ctx{0};
    const int capacity = 41, n_in = start == kDeviceFewer ? 29 : capacity;
    std::vector<int16_t> cloud((size_t)capacity * PCS_POINT_SHORTS);
    for (int i = 0; i < capacity; i++)
        for (int k = 0; k < PCS_POINT_SHORTS; k++) cloud[i * PCS_POINT_SHORTS + k] = (int16_t)(k ? 100 * i + k : i % 6);
    int32_t count = n_in;
    const Cloud in{cloud.data(), start == kHost ? nullptr : &count, start == kHost ? n_in : -12345, capacity};
    Chain chain;
    std::string why;
    const char* const args[kStageCount] = {"", "11,2", "22,1000,30", "33,16,3,2,5", "44,3"};
    int n_enabled = 0;
    for (int s = 1; s < kStageCount; s++)
        if (subset >> s & 1) { EXPECT(chain.parse(kStages[s].letter, args[s], why)); n_enabled++; }
    EXPECT(chain.any() == (n_enabled > 0) && !chain.plan_view());
    EXPECT(!chain.parse_plan("m,+z,10", why) && !chain.parse_plan("m,up,10,4x4", why) && !chain.parse_plan("m,+z,0,4x4", why) && !chain.plan_view());
    const std::string prefix = "filter_chain_check_plan.tmp";
    EXPECT(chain.parse_plan((prefix + ",-y,25,7x5,-80,-60,-100,900").c_str(), why) && chain.plan_view() && chain.any());
    EXPECT(!chain.parse_plan((prefix + ",+z,10,4x4").c_str(), why) && why.find("twice") != std::string::npos);
    const pcs_plan_params& P = chain.plan.params;
    EXPECT(P.up_axis == 1 && P.up_sign == -1 && P.cell_mm == 25 && P.width == 7 && P.height == 5 && P.origin_u == -80 && P.origin_v == -60 &&
           P.band_lo == -100 && P.band_hi == 900 && !P.reserved[0] && !P.reserved[1] && !P.reserved[2]);
    chain.finish_options();
    g_live.clear(); g_plan_calls.clear();
    EXPECT(chain.allocate(&ctx, (size_t)capacity * PCS_POINT_SHORTS) == PCS_OK);
    const pcs_plan_maps& m = chain.plan.maps;
    const uint8_t* base = static_cast<const uint8_t*>(chain.d_plan);
    EXPECT(g_live.count(chain.d_plan) && g_live[chain.d_plan] == 5 * 256 && (const uint8_t*)m.count == base && (const uint8_t*)m.top == base + 256 &&
           (const uint8_t*)m.bottom == base + 512 && m.rgb == base + 768 && (const uint8_t*)m.stats == base + 1024);
    for (int frame = 0; frame < 2; frame++) {
        g_calls.clear();
        const Cloud out = chain.run(&ctx, in);
        EXPECT(chain.status == PCS_OK && (int)g_calls.size() == n_enabled && (int)g_plan_calls.size() == frame);      // run() itself makes no map
        EXPECT(chain.run_plan(&ctx, out) == PCS_OK && (int)g_plan_calls.size() == frame + 1);
        const PlanCall& c = g_plan_calls.back();
        EXPECT(c.calls_before == (size_t)n_enabled && c.in == out.d && c.d_n == out.d_n && c.counted == (out.d_n != nullptr));
        EXPECT(c.counted == (n_enabled > 0 || start != kHost));
        if (!n_enabled) EXPECT(c.in == cloud.data());                                                                  // no stage: the cloud that entered
        if (c.counted) EXPECT(c.max_points == capacity); else EXPECT(c.n_points == n_in);
        EXPECT(memcmp(&c.params, &P, sizeof P) == 0 && memcmp(&c.maps, &m, sizeof m) == 0);
        std::ostringstream line, want_line;
        EXPECT(chain.report_plan(line) && g_plan_calls.size() == (size_t)frame + 1);
        want_line << "Plan view: " << (c.counted ? *c.d_n : n_in) << " considered, " << 1000 + frame << " in band, " << 900 + frame
                  << " on the map, 24 occupied of 7 x 5 cells, fullest 70000\n";
        EXPECT(line.str() == want_line.str());
    }
    EXPECT(chain.write_plan(why) && g_plan_calls.size() == 2);                                                         // (writing launches nothing)
    std::ostringstream rgb, top, cnt;
    pcs_planview::write_rgb_ppm(rgb, 7, 5, m.rgb);
    pcs_planview::write_top_pgm(top, P, m.count, m.top);
    pcs_planview::write_count_pgm(cnt, 7, 5, m.count);
    const std::string want[3] = {rgb.str(), top.str(), cnt.str()};
    const char* const suffix[3] = {".rgb.ppm", ".top.pgm", ".count.pgm"};
    for (int k = 0; k < 3; k++) {
        std::ifstream f(prefix + suffix[k], std::ios::binary);
        std::stringstream got;
        got << f.rdbuf();
        EXPECT(got.str() == want[k] && got.str().size() == (k == 0 ? 11u + 105u : 13u + 70u));
        remove((prefix + suffix[k]).c_str());
    }
    // the last call: cell 0 has count 1 and top -32767, seen along -y h = 32767, grey 65535; cell 1 top -32467, grey 65235 = 0xFED3, its count
    // saturated; cell 2 is empty
    EXPECT(want[1].substr(13, 6) == std::string("\xFF\xFF\xFE\xD3\x00\x00", 6) && want[2].substr(13, 6) == std::string("\x00\x01\xFF\xFF\x00\x00", 6));
    chain.release();
    EXPECT(g_live.empty() && g_bad_frees == 0 && !chain.d_plan && !chain.plan.maps.count);
    chain.release();      // (nothing left to free)
    EXPECT(g_bad_frees == 0);
}

int main()
{
    for (int subset = 0; subset < 32; subset++)
        for (Start start : {kHost, kDeviceFewer, kDeviceFull}) {
            check(subset, start);
            if (subset & 16)
                for (int max_objects : {3, 5, 1024}) check(subset, start, max_objects);
        }
    for (int subset : {0, 2, 12, 30})
        for (Start start : {kHost, kDeviceFewer, kDeviceFull})
            for (int max_cells : {1000, 7}) check_learn(subset, start, max_cells);
    for (int subset : {16, 18, 30})
        for (Start start : {kHost, kDeviceFewer, kDeviceFull})
            for (int max_objects : {0, 3, 1024}) check_tracks(subset, start, max_objects);
    for (int subset : {16, 18, 30})
        for (Start start : {kHost, kDeviceFewer, kDeviceFull})
            for (int max_objects : {0, 3, 1024})
                for (bool with_tracks : {false, true}) check_boxes(subset, start, max_objects, with_tracks);
    for (int subset : {0, 2, 16, 30})
        for (Start start : {kHost, kDeviceFewer, kDeviceFull}) check_plan(subset, start);
    printf(g_failed ? "filter_chain_check: %d check(s) FAILED\n" : "filter_chain_check: all checks passed, no report\n", g_failed);
    fflush(stdout);      // (a leak report at exit must not swallow the lines above)
    return g_failed ? 1 : 0;
}
