// pcs_filter_chain.h — the post-stitch filters of pcs-multicamera-optimized, -X -O -K -M -E in that order, as one chain ahead of -V.
// Plain C++17 over include/pcs_hip.h. The rule every stage follows, stated once:
//
//   A stage reads the output of the stage in front of it. If that stage left its record count on the device, the counted form is
//   called with that count word and max_points = the number of records that entered the chain; otherwise the plain form with the
//   host's count. The stage writes its own output and its own count word. Nothing is copied to the host in between: whoever needs
//   the last count fetches it once.
//
// Two output buffers alternate between the stages (stage k reads what stage k-1 wrote and writes the other one, so no call sees
// overlapping input and output; the first stage's input belongs to the caller). Every enabled stage keeps a 64-byte count word and
// its own statistics / model block, which report() reads after the frame-set's last launch.
//
// -L (pcs_objects.h) adds nothing to the order: with it the E stage calls the objects form of the cluster filter — plain or counted by
// the same rule, the stage's usual output buffer, count word and statistics block in its `out` struct — so the cloud that leaves the
// stage is what -E alone gives, and the object table and its count land in two device blocks of the chain's own.
//
// -J (pcs_tracks.h) rides on the same call: the table (at -L's default size if -L is not given) and object_of, and behind the stage's
// call one pcs_tracker_update_device* over the cloud the stage read, on the same count rule. Nothing comes to the host for it;
// write_tracks() copies the tracks and the table after the frame-set's launches and appends the frame-set's lines.
//
// -W (pcs_boxes.h) stands beside it: the same table and object_of, and behind the stage's call (and the tracker's, where -J is given
// too) one pcs_object_boxes_device* over the cloud the stage read, on the same count rule, into a device block of the chain's own.
// write_boxes() copies the entries after the frame-set's launches and appends the frame-set's lines.
//
// -H (pcs_planview.h) is no stage and drops nothing: behind run(), ahead of -V, plan_view() reads the cloud that leaves the chain (the
// last enabled stage's output, or what entered if none is on) with one pcs_plan_view_device*, on the same count rule, into a device
// block of the chain's own. write_plan() copies the rasters after the run's last frame-set and writes the three files.
#pragma once

#include <cstring>
#include <fstream>
#include <iostream>
#include <ostream>
#include <string>
#include <vector>

#include "pcs_background.h"
#include "pcs_boxes.h"
#include "pcs_cluster.h"
#include "pcs_objects.h"
#include "pcs_outlier.h"
#include "pcs_plane.h"
#include "pcs_planview.h"
#include "pcs_statoutlier.h"
#include "pcs_tracks.h"

namespace pcs_filter_chain {

struct Cloud {
    const int16_t* d;       // device: the records
    const int32_t* d_n;     // device: their count, or nullptr when only the host knows it
    int n;                  // the host's count (read only when d_n is nullptr)
    int capacity;           // the records that entered the chain: max_points of every counted call
};

struct Params {
    // -X FILE: the option's words, then what allocate() makes of them and the file (the model on the device, min_seen from its frames)
    struct {
        std::string file;
        int min_percent = 0, dilate = 0;
        pcs_background* model = nullptr;
        pcs_background_params params{};
        uint32_t frames = 0;
    } background;
    int radius_mm = 0, min_neighbors = 0;
    pcs_stat_outlier_params stat{};
    pcs_plane_params plane{};
    pcs_cluster_params cluster{};
    // -L: max_objects 0 = not given; the table and its count word on the device (Chain::allocate)
    struct { int max_objects = 0; pcs_cluster_object* d_table = nullptr; int32_t* d_n = nullptr; } objects;
    // -J: cell_mm 0 = not given; the tracker, and views of the chain's three blocks for it (Chain::allocate): object_of of the E stage's
    // input, the tracks and the statistics block
    struct {
        int cell_mm = 0;
        pcs_track_params params{};
        pcs_tracker* tracker = nullptr;
        int32_t* d_object_of = nullptr;
        pcs_track* d_tracks = nullptr;
        pcs_track_stats* d_stats = nullptr;
    } tracks;
    // -W: on = given; views of the chain's blocks for it (Chain::allocate): object_of of the E stage's input (the tracker's where -J is
    // given too) and the entries
    struct { bool on = false; int32_t* d_object_of = nullptr; pcs_object_box* d_boxes = nullptr; } boxes;
};

// -M's block: the statistics, then the models
struct PlaneBlock {
    pcs_plane_stats stats;
    pcs_plane_model models[PCS_PLANE_MAX_PLANES];
};

struct Stage {
    char letter;
    const char* refusal;       // "-G: the node library has no <refusal>"
    const char* (*help)();
    bool (*parse)(const char* arg, Params& p, std::string& why);
    size_t block_bytes;        // the statistics / model block on the device (0: none)
    // the plain or the counted library entry, by whether `in` has a device count
    int (*call)(pcs_ctx* ctx, const Params& p, const Cloud& in, int16_t* d_out, size_t out_shorts, int32_t* d_n_out, void* d_block);
    // the -t line(s): `block` is the host's copy, n_in / n_kept the counts in front of and behind the stage
    void (*print)(std::ostream& os, const Params& p, const void* block, int n_in, int n_kept);
};

inline const Stage kStages[] = {
    {'X', "background model", pcs_background_cli::help,
     [](const char* arg, Params& p, std::string& why) {
         return pcs_background_cli::parse_subtract(arg, p.background.file, p.background.min_percent, p.background.dilate, why);
     }, sizeof(pcs_background_stats),
     [](pcs_ctx* ctx, const Params& p, const Cloud& in, int16_t* d_out, size_t out_shorts, int32_t* d_n_out, void* d_block) {
         pcs_background_stats* d_stats = static_cast<pcs_background_stats*>(d_block);
         const auto& b = p.background;
         return in.d_n ? pcs_background_subtract_device_counted(ctx, b.model, in.d, in.d_n, in.capacity, &b.params, d_out, out_shorts, d_n_out, d_stats)
                       : pcs_background_subtract_device(ctx, b.model, in.d, in.n, &b.params, d_out, out_shorts, d_n_out, d_stats);
     },
     [](std::ostream& os, const Params& p, const void* block, int, int) {
         pcs_background_stats st;
         memcpy(&st, block, sizeof st);
         os << "Background subtraction: " << st.considered << " -> " << st.kept << " points (" << st.cells << " cells, seen >= " << st.min_seen
            << " of " << st.frames << ", dilate " << p.background.dilate << ")" << std::endl;
     }},
    {'O', "outlier filter", pcs_outlier::help,
     [](const char* arg, Params& p, std::string& why) { return pcs_outlier::parse(arg, p.radius_mm, p.min_neighbors, why); }, 0,
     [](pcs_ctx* ctx, const Params& p, const Cloud& in, int16_t* d_out, size_t out_shorts, int32_t* d_n_out, void*) {
         return in.d_n ? pcs_radius_outlier_device_counted(ctx, in.d, in.d_n, in.capacity, p.radius_mm, p.min_neighbors, d_out, out_shorts, d_n_out)
                       : pcs_radius_outlier_device(ctx, in.d, in.n, p.radius_mm, p.min_neighbors, d_out, out_shorts, d_n_out);
     },
     [](std::ostream& os, const Params&, const void*, int n_in, int n_kept) { os << "Outlier removal: " << n_in << " -> " << n_kept << " points" << std::endl; }},
    {'K', "outlier filter", pcs_statoutlier::help,
     [](const char* arg, Params& p, std::string& why) { return pcs_statoutlier::parse(arg, p.stat, why); }, sizeof(pcs_stat_outlier_stats),
     [](pcs_ctx* ctx, const Params& p, const Cloud& in, int16_t* d_out, size_t out_shorts, int32_t* d_n_out, void* d_block) {
         pcs_stat_outlier_stats* d_stats = static_cast<pcs_stat_outlier_stats*>(d_block);
         return in.d_n ? pcs_stat_outlier_device_counted(ctx, in.d, in.d_n, in.capacity, &p.stat, d_out, out_shorts, d_n_out, d_stats)
                       : pcs_stat_outlier_device(ctx, in.d, in.n, &p.stat, d_out, out_shorts, d_n_out, d_stats);
     },
     [](std::ostream& os, const Params&, const void* block, int, int) {
         pcs_stat_outlier_stats st;
         memcpy(&st, block, sizeof st);
         os << "Statistical outlier removal: " << st.considered << " -> " << st.kept << " points (dense " << st.dense << ", threshold "
            << st.threshold << "/256 per k)" << std::endl;
     }},
    {'M', "plane segmentation", pcs_plane::help,
     [](const char* arg, Params& p, std::string& why) { return pcs_plane::parse(arg, p.plane, why); }, sizeof(PlaneBlock),
     [](pcs_ctx* ctx, const Params& p, const Cloud& in, int16_t* d_out, size_t out_shorts, int32_t* d_n_out, void* d_block) {
         PlaneBlock* b = static_cast<PlaneBlock*>(d_block);
         return in.d_n ? pcs_plane_segment_device_counted(ctx, in.d, in.d_n, in.capacity, &p.plane, d_out, out_shorts, d_n_out, b->models, &b->stats)
                       : pcs_plane_segment_device(ctx, in.d, in.n, &p.plane, d_out, out_shorts, d_n_out, b->models, &b->stats);
     },
     [](std::ostream& os, const Params&, const void* block, int, int) {
         PlaneBlock b;
         memcpy(&b, block, sizeof b);
         const pcs_plane_stats& st = b.stats;
         os << "Plane segmentation: " << st.considered << " -> " << st.kept << " points (" << st.planes << " planes, " << st.inliers_total
            << " inliers)" << std::endl;
         for (int r = 0; r < (int)st.planes && r < PCS_PLANE_MAX_PLANES; r++)
             os << "Plane " << r << ": " << b.models[r].inliers << " inliers, normal (" << b.models[r].nx << ", " << b.models[r].ny << ", "
                << b.models[r].nz << "), offset " << b.models[r].off << ", hypothesis " << b.models[r].hypothesis << std::endl;
     }},
    {'E', "cluster filter", pcs_cluster::help,
     [](const char* arg, Params& p, std::string& why) { return pcs_cluster::parse(arg, p.cluster, why); }, sizeof(pcs_cluster_stats),
     [](pcs_ctx* ctx, const Params& p, const Cloud& in, int16_t* d_out, size_t out_shorts, int32_t* d_n_out, void* d_block) {
         pcs_cluster_stats* d_stats = static_cast<pcs_cluster_stats*>(d_block);
         if (p.objects.max_objects) {      // -L: the same filter, and the object table beside it
             pcs_cluster_objects_out o{};
             o.objects = p.objects.d_table; o.max_objects = p.objects.max_objects; o.n_objects = p.objects.d_n;
             o.out = d_out; o.out_shorts = out_shorts; o.out_points = d_n_out; o.stats = d_stats;
             const auto& t = p.tracks;
             const auto& b = p.boxes;
             o.object_of = t.d_object_of ? t.d_object_of : b.d_object_of;
             int rc = in.d_n ? pcs_cluster_objects_device_counted(ctx, in.d, in.d_n, in.capacity, &p.cluster, &o)
                             : pcs_cluster_objects_device(ctx, in.d, in.n, &p.cluster, &o);
             // -J: the objects of the cloud this stage read, tracked where they stand
             if (rc == PCS_OK && t.tracker)
                 rc = in.d_n ? pcs_tracker_update_device_counted(ctx, t.tracker, in.d, in.d_n, in.capacity, t.d_object_of, o.n_objects,
                                                                 o.max_objects, &t.params, t.d_tracks, t.d_stats)
                             : pcs_tracker_update_device(ctx, t.tracker, in.d, in.n, t.d_object_of, o.n_objects, o.max_objects, &t.params,
                                                         t.d_tracks, t.d_stats);
             // -W: ... and boxed where they stand
             if (rc == PCS_OK && b.on)
                 rc = in.d_n ? pcs_object_boxes_device_counted(ctx, in.d, in.d_n, in.capacity, o.object_of, o.n_objects, o.max_objects, b.d_boxes)
                             : pcs_object_boxes_device(ctx, in.d, in.n, o.object_of, o.n_objects, o.max_objects, b.d_boxes);
             return rc;
         }
         return in.d_n ? pcs_cluster_filter_device_counted(ctx, in.d, in.d_n, in.capacity, &p.cluster, d_out, out_shorts, d_n_out, d_stats)
                       : pcs_cluster_filter_device(ctx, in.d, in.n, &p.cluster, d_out, out_shorts, d_n_out, d_stats);
     },
     [](std::ostream& os, const Params&, const void* block, int, int) {
         pcs_cluster_stats st;
         memcpy(&st, block, sizeof st);
         os << "Cluster filter: " << st.considered << " -> " << st.kept << " points (" << st.clusters << " clusters, " << st.kept_clusters
            << " kept, largest " << st.largest << ")" << std::endl;
     }},
};
constexpr int kStageCount = sizeof kStages / sizeof kStages[0];
constexpr int kBackgroundStage = 0;                 // 'X': the stage of -X FILE
constexpr int kClusterStage = kStageCount - 1;      // 'E': the stage -L rides on
static_assert(kStageCount == 5, "X O K M E");

struct Chain {
    Params params;
    bool enabled[kStageCount] = {};
    pcs_ctx* ctx = nullptr;
    size_t out_shorts = 0;                 // what each of d_buf holds
    void* d_buf[2] = {};
    void* d_count[kStageCount] = {};
    void* d_block[kStageCount] = {};
    Cloud entered{};                       // what the last run() was given
    int status = PCS_OK;                   // of the last run(): the first stage that failed ends it
    std::string objects_file;              // -L: where the table goes ("-": stdout); empty: no -L
    void* d_objects = nullptr;             // ... the table (params.objects.max_objects entries) and its count word
    void* d_n_objects = nullptr;
    void* d_object_of = nullptr;           // -J, -W: one int32 per record that can enter the chain; -J: max_objects tracks, the statistics block
    void* d_tracks = nullptr;
    void* d_track_stats = nullptr;
    // -J: where the lines go ("-": stdout), the stream, the frame-sets written and the run's totals for -t
    std::string tracks_file;
    std::ofstream tracks_stream;
    long long tracks_frames = 0, tracks_born = 0, tracks_continued = 0, tracks_lost = 0;
    // -W: the entries (max_objects of them), where the lines go ("-": stdout), the stream, the frame-sets written and the run's totals for -t
    void* d_boxes = nullptr;
    std::string boxes_file;
    std::ofstream boxes_stream;
    long long boxes_frames = 0, boxes_objects = 0, boxes_rank3 = 0;
    // -H: the option's words, the device block that holds the four rasters and the statistics block (views of it in plan_maps), and
    // whether a frame-set went through
    struct { bool on = false; std::string prefix; pcs_plan_params params{}; pcs_plan_maps maps{}; bool ran = false; } plan;
    void* d_plan = nullptr;
    // -X learn: the option's words and the model allocate() creates; -X FILE: the file's bytes (load_background), imported by allocate()
    struct { std::string file; int cell_mm = 0, max_cells = 0; pcs_background* model = nullptr; } learn;
    std::vector<char> background_bytes;

    bool learning() const { return learn.cell_mm != 0; }
    bool any() const
    {
        for (bool e : enabled) if (e) return true;
        return learning() || plan.on;
    }

    // -X's argument, either form. false: `why` says what is wrong with it.
    bool parse_background(const char* arg, std::string& why)
    {
        const bool is_learn = strncmp(arg, "learn:", 6) == 0;
        if (learning() || enabled[kBackgroundStage]) {
            why = is_learn == learning() ? "the option was given twice" : "one run either learns a model or subtracts one: give one form of -X";
            return false;
        }
        if (is_learn) return pcs_background_cli::parse_learn(arg + 6, learn.file, learn.cell_mm, learn.max_cells, why);
        return parse('X', arg, why);
    }

    // -X FILE: the file read and validated on the host, before any context exists. false: `why` names the file and what was found.
    bool load_background(std::string& why)
    {
        struct pcs_background_info info{};
        if (!pcs_background_cli::load(params.background.file, background_bytes, info, why)) return false;
        params.background.frames = info.frames;
        params.background.params = pcs_background_params{pcs_background_cli::min_seen_of(info.frames, params.background.min_percent),
                                                         params.background.dilate, PCS_BACKGROUND_MODE_REMOVE, 0};
        return true;
    }

    // An option of the table's: its argument into the parameters, the stage switched on. false: `why` says what is wrong with it.
    bool parse(int letter, const char* arg, std::string& why)
    {
        for (int s = 0; s < kStageCount; s++)
            if (kStages[s].letter == letter) return enabled[s] = kStages[s].parse(arg, params, why);
        return false;
    }

    // -L's argument: the file and the table's size. false: `why` says what is wrong with it.
    bool parse_objects(const char* arg, std::string& why)
    {
        return pcs_objects::parse(arg, objects_file, params.objects.max_objects, why);
    }
    bool objects() const { return !objects_file.empty(); }

    // -J's argument: the file, the cell and the vote threshold. false: `why` says what is wrong with it. Without -L the object table is
    // still made, at -L's default size (finish_options, once every option has been read).
    bool parse_tracks(const char* arg, std::string& why)
    {
        int min_votes = 0;
        if (!pcs_tracks::parse(arg, tracks_file, params.tracks.cell_mm, min_votes, why)) return false;
        params.tracks.params = pcs_track_params{min_votes, {0, 0, 0}};
        return true;
    }
    bool tracks() const { return params.tracks.cell_mm != 0; }
    // -W's argument: the file. false: `why` says what is wrong with it. Without -L the object table is made as for -J.
    bool parse_boxes(const char* arg, std::string& why)
    {
        return params.boxes.on = pcs_boxes::parse(arg, boxes_file, why);
    }
    bool boxes() const { return params.boxes.on; }
    // -H's argument: the prefix and the map. false: `why` says what is wrong with it.
    bool parse_plan(const char* arg, std::string& why)
    {
        if (plan.on) { why = "the option was given twice"; return false; }
        return plan.on = pcs_planview::parse(arg, plan.prefix, plan.params, why);
    }
    bool plan_view() const { return plan.on; }
    void finish_options()
    {
        if ((tracks() || boxes()) && !params.objects.max_objects) params.objects.max_objects = pcs_objects::kDefaultMaxObjects;
    }

    // Buffers for clouds of up to out_shorts shorts: one per enabled stage, two at the most.
    int allocate(pcs_ctx* c, size_t shorts)
    {
        ctx = c; out_shorts = shorts;
        int n = 0, rc = PCS_OK;
        for (int s = 0; s < kStageCount && rc == PCS_OK; s++) {
            if (!enabled[s]) continue;
            if (n < 2) rc = pcs_device_malloc(ctx, &d_buf[n++], out_shorts * sizeof(int16_t) + 64);
            if (rc == PCS_OK) rc = pcs_device_malloc(ctx, &d_count[s], 64);
            if (rc == PCS_OK && kStages[s].block_bytes) rc = pcs_device_malloc(ctx, &d_block[s], kStages[s].block_bytes);
        }
        if (rc == PCS_OK && enabled[kBackgroundStage]) {      // a table with room for the file's cells, no more
            const size_t cells = background_bytes.size() > 32 ? (background_bytes.size() - 32) / 12 : 1;
            rc = pcs_background_import(ctx, background_bytes.data(), background_bytes.size(), (int)cells, &params.background.model);
        }
        if (rc == PCS_OK && learning()) rc = pcs_background_create(ctx, learn.cell_mm, learn.max_cells, &learn.model);
        if (rc == PCS_OK && params.objects.max_objects) {
            rc = pcs_device_malloc(ctx, &d_objects, (size_t)params.objects.max_objects * sizeof(pcs_cluster_object));
            if (rc == PCS_OK) rc = pcs_device_malloc(ctx, &d_n_objects, 64);
            params.objects.d_table = static_cast<pcs_cluster_object*>(d_objects);
            params.objects.d_n = static_cast<int32_t*>(d_n_objects);
        }
        const size_t records = out_shorts / PCS_POINT_SHORTS;
        if (rc == PCS_OK && (tracks() || boxes())) rc = pcs_device_malloc(ctx, &d_object_of, (records + 1) * sizeof(int32_t));
        if (rc == PCS_OK && boxes()) {
            rc = pcs_device_malloc(ctx, &d_boxes, (size_t)params.objects.max_objects * sizeof(pcs_object_box));
            params.boxes.d_object_of = static_cast<int32_t*>(d_object_of); params.boxes.d_boxes = static_cast<pcs_object_box*>(d_boxes);
        }
        if (rc == PCS_OK && plan.on) {       // one block: count, top, bottom, rgb, statistics, each at 256 bytes
            const size_t cells = (size_t)plan.params.width * plan.params.height;
            auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
            const size_t at_top = up(4 * cells), at_bottom = at_top + up(2 * cells), at_rgb = at_bottom + up(2 * cells), at_stats = at_rgb + up(3 * cells);
            rc = pcs_device_malloc(ctx, &d_plan, at_stats + 256);
            uint8_t* const b = static_cast<uint8_t*>(d_plan);
            if (rc == PCS_OK)
                plan.maps = pcs_plan_maps{reinterpret_cast<uint32_t*>(b), reinterpret_cast<int16_t*>(b + at_top), reinterpret_cast<int16_t*>(b + at_bottom),
                                          b + at_rgb, reinterpret_cast<pcs_plan_stats*>(b + at_stats)};
        }
        if (rc == PCS_OK && tracks()) {      // max_cells: the records that can enter the chain
            auto& t = params.tracks;
            const int max_cells = (int)(records < 1 ? 1 : records > (size_t)PCS_TRACKER_MAX_CELLS_MAX ? (size_t)PCS_TRACKER_MAX_CELLS_MAX : records);
            rc = pcs_tracker_create(ctx, t.cell_mm, max_cells, params.objects.max_objects, &t.tracker);
            if (rc == PCS_OK) rc = pcs_device_malloc(ctx, &d_tracks, (size_t)params.objects.max_objects * sizeof(pcs_track));
            if (rc == PCS_OK) rc = pcs_device_malloc(ctx, &d_track_stats, sizeof(pcs_track_stats));
            t.d_object_of = static_cast<int32_t*>(d_object_of); t.d_tracks = static_cast<pcs_track*>(d_tracks);
            t.d_stats = static_cast<pcs_track_stats*>(d_track_stats);
        }
        return rc;
    }

    // The enabled stages over `in`, launched in order; returns the last one's output (or `in`). Copies nothing to the host.
    Cloud run(pcs_ctx* c, Cloud in)
    {
        entered = in; status = PCS_OK;
        if (learning())
            status = in.d_n ? pcs_background_learn_device_counted(c, learn.model, in.d, in.d_n, in.capacity)
                            : pcs_background_learn_device(c, learn.model, in.d, in.n);
        int k = 0;
        for (int s = 0; s < kStageCount && status == PCS_OK; s++) {
            if (!enabled[s]) continue;
            int16_t* d_out = static_cast<int16_t*>(d_buf[k++ & 1]);
            int32_t* d_n_out = static_cast<int32_t*>(d_count[s]);
            status = kStages[s].call(c, params, in, d_out, out_shorts, d_n_out, d_block[s]);
            in = Cloud{d_out, d_n_out, 0, in.capacity};
        }
        return in;
    }

    // -H: the maps of `out`, the cloud run() returned, on the chain's count rule. Launches only; copies nothing to the host.
    int run_plan(pcs_ctx* c, const Cloud& out)
    {
        plan.ran = true;
        return out.d_n ? pcs_plan_view_device_counted(c, out.d, out.d_n, out.capacity, &plan.params, &plan.maps)
                       : pcs_plan_view_device(c, out.d, out.n, &plan.params, &plan.maps);
    }

    // -H's -t line of the last run_plan(). false: a copy failed (pcs_last_error has it).
    bool report_plan(std::ostream& os) const
    {
        pcs_plan_stats st{};
        if (pcs_memcpy_d2h(ctx, &st, plan.maps.stats, sizeof st) != PCS_OK || pcs_synchronize(ctx) != PCS_OK) return false;
        pcs_planview::report(os, plan.params, st);
        return true;
    }

    // -H's three files from the last run_plan() (an empty map if no frame-set went through). false: a copy failed (pcs_last_error has
    // it) or a file cannot be written (`why` names it).
    bool write_plan(std::string& why) const
    {
        const int w = plan.params.width, h = plan.params.height;
        const size_t cells = (size_t)w * h;
        std::vector<uint32_t> count(cells, 0u);
        std::vector<int16_t> top(cells, 0);
        std::vector<uint8_t> rgb(3 * cells, 0);
        if (plan.ran && (pcs_memcpy_d2h(ctx, count.data(), plan.maps.count, 4 * cells) != PCS_OK ||
                         pcs_memcpy_d2h(ctx, top.data(), plan.maps.top, 2 * cells) != PCS_OK ||
                         pcs_memcpy_d2h(ctx, rgb.data(), plan.maps.rgb, 3 * cells) != PCS_OK || pcs_synchronize(ctx) != PCS_OK))
            return false;
        const char* const names[3] = {".rgb.ppm", ".top.pgm", ".count.pgm"};
        for (int k = 0; k < 3; k++) {
            const std::string file = plan.prefix + names[k];
            std::ofstream f(file, std::ios::binary);
            if (k == 0) pcs_planview::write_rgb_ppm(f, w, h, rgb.data());
            else if (k == 1) pcs_planview::write_top_pgm(f, plan.params, count.data(), top.data());
            else pcs_planview::write_count_pgm(f, w, h, count.data());
            f.flush();
            if (!f.good()) { why = "cannot write " + file; return false; }
        }
        return true;
    }

    // The -t lines of the last run(), in stage order. false: a copy failed (pcs_last_error has it).
    bool report(std::ostream& os) const
    {
        if (!any()) return true;
        int32_t n[kStageCount + 1] = {entered.n};
        std::vector<char> block[kStageCount];
        bool ok = !entered.d_n || pcs_memcpy_d2h(ctx, &n[0], entered.d_n, sizeof n[0]) == PCS_OK;
        for (int s = 0; s < kStageCount && ok; s++) {
            if (!enabled[s]) continue;
            block[s].resize(kStages[s].block_bytes);
            ok = pcs_memcpy_d2h(ctx, &n[s + 1], d_count[s], sizeof n[0]) == PCS_OK &&
                 (block[s].empty() || pcs_memcpy_d2h(ctx, block[s].data(), d_block[s], block[s].size()) == PCS_OK);
        }
        int32_t n_objects = 0;
        if (ok && objects()) ok = pcs_memcpy_d2h(ctx, &n_objects, d_n_objects, sizeof n_objects) == PCS_OK;
        if (!ok || pcs_synchronize(ctx) != PCS_OK) return false;
        int n_in = n[0];
        for (int s = 0; s < kStageCount; s++) {
            if (!enabled[s]) continue;
            kStages[s].print(os, params, block[s].data(), n_in, n[s + 1]);
            if (s == kClusterStage && objects())
                os << "Objects: " << n_objects << " (" << (n_objects < params.objects.max_objects ? n_objects : params.objects.max_objects)
                   << " written)" << std::endl;
            n_in = n[s + 1];
        }
        return true;
    }

    // -L's lines of the last run(): the header and one line per written object. false: a copy failed (pcs_last_error has it).
    bool write_objects(std::ostream& os) const
    {
        int32_t n_objects = 0;
        if (!entered.d) { pcs_objects::write(os, nullptr, 0); return true; }      // no frame-set went through: the header alone
        if (pcs_memcpy_d2h(ctx, &n_objects, d_n_objects, sizeof n_objects) != PCS_OK || pcs_synchronize(ctx) != PCS_OK) return false;
        const int written = n_objects < 0 ? 0 : n_objects < params.objects.max_objects ? n_objects : params.objects.max_objects;
        std::vector<pcs_cluster_object> table((size_t)written);
        if (written && (pcs_memcpy_d2h(ctx, table.data(), d_objects, table.size() * sizeof table[0]) != PCS_OK || pcs_synchronize(ctx) != PCS_OK))
            return false;
        pcs_objects::write(os, table.data(), written);
        return true;
    }

    // -J: the file opened and its header written, before the first frame-set. false: it cannot be written.
    bool open_tracks()
    {
        if (tracks_file != "-") tracks_stream.open(tracks_file);
        std::ostream& os = tracks_file == "-" ? std::cout : tracks_stream;
        pcs_tracks::write_header(os);
        os.flush();
        return os.good();
    }

    // -J's lines of the last run(), appended; the run's totals kept for -t. false: a copy failed (pcs_last_error has it) or the file
    // cannot be written (`why` says so).
    bool write_tracks(std::string& why)
    {
        int32_t n_objects = 0;
        pcs_track_stats st{};
        if (pcs_memcpy_d2h(ctx, &n_objects, d_n_objects, sizeof n_objects) != PCS_OK ||
            pcs_memcpy_d2h(ctx, &st, params.tracks.d_stats, sizeof st) != PCS_OK || pcs_synchronize(ctx) != PCS_OK) return false;
        const int written = n_objects < 0 ? 0 : n_objects < params.objects.max_objects ? n_objects : params.objects.max_objects;
        std::vector<pcs_cluster_object> table((size_t)written);
        std::vector<pcs_track> ids((size_t)written);
        if (written && (pcs_memcpy_d2h(ctx, table.data(), d_objects, table.size() * sizeof table[0]) != PCS_OK ||
                        pcs_memcpy_d2h(ctx, ids.data(), params.tracks.d_tracks, ids.size() * sizeof ids[0]) != PCS_OK ||
                        pcs_synchronize(ctx) != PCS_OK))
            return false;
        std::ostream& os = tracks_file == "-" ? std::cout : tracks_stream;
        pcs_tracks::write(os, tracks_frames++, ids.data(), table.data(), written);
        os.flush();
        tracks_born += st.born; tracks_continued += st.continued; tracks_lost += st.lost;
        if (!os.good()) { why = "cannot write " + tracks_file; return false; }
        return true;
    }

    // -W: the file opened and its header written, before the first frame-set. false: it cannot be written.
    bool open_boxes()
    {
        if (boxes_file != "-") boxes_stream.open(boxes_file);
        std::ostream& os = boxes_file == "-" ? std::cout : boxes_stream;
        pcs_boxes::write_header(os);
        os.flush();
        return os.good();
    }

    // -W's lines of the last run(), appended; the run's totals kept for -t. false: a copy failed (pcs_last_error has it) or the file
    // cannot be written (`why` says so).
    bool write_boxes(std::string& why)
    {
        int32_t n_objects = 0;
        if (pcs_memcpy_d2h(ctx, &n_objects, d_n_objects, sizeof n_objects) != PCS_OK || pcs_synchronize(ctx) != PCS_OK) return false;
        const int written = n_objects < 0 ? 0 : n_objects < params.objects.max_objects ? n_objects : params.objects.max_objects;
        std::vector<pcs_object_box> entries((size_t)written);
        if (written && (pcs_memcpy_d2h(ctx, entries.data(), d_boxes, entries.size() * sizeof entries[0]) != PCS_OK || pcs_synchronize(ctx) != PCS_OK))
            return false;
        std::ostream& os = boxes_file == "-" ? std::cout : boxes_stream;
        pcs_boxes::write(os, boxes_frames++, entries.data(), written);
        os.flush();
        boxes_objects += written;
        for (const pcs_object_box& b : entries) boxes_rank3 += b.rank == 3;
        if (!os.good()) { why = "cannot write " + boxes_file; return false; }
        return true;
    }

    // -X learn: when the run ends: the model into its file, and with `say` the line. 0, or the status the program ends with (1) after a
    // message on `err`: an overflowed model, a failed call, a file that cannot be written.
    int finish_learning(std::ostream& os, std::ostream& err, bool say)
    {
        if (!learning() || !learn.model) return 0;
        struct pcs_background_info info{};
        if (pcs_background_info(ctx, learn.model, &info) != PCS_OK) { err << "-X learn: " << pcs_last_error(ctx) << std::endl; return 1; }
        if (info.overflow) {
            err << "-X learn: the scene has more than max_cells " << learn.max_cells << " cells of " << learn.cell_mm
                << " mm: no model written (give a larger max_cells or a larger cell_mm)" << std::endl;
            return 1;
        }
        std::vector<char> bytes(pcs_background_export_bound((int)info.cells));
        size_t n = 0;
        if (pcs_background_export(ctx, learn.model, bytes.data(), bytes.size(), &n) != PCS_OK) { err << "-X learn: " << pcs_last_error(ctx) << std::endl; return 1; }
        FILE* f = fopen(learn.file.c_str(), "wb");
        const bool ok = f && fwrite(bytes.data(), 1, n, f) == n;
        if (f && fclose(f) != 0) { err << "-X learn: cannot write " << learn.file << std::endl; return 1; }
        if (!ok) { err << "-X learn: cannot write " << learn.file << std::endl; return 1; }
        if (say) os << "Background learned: " << info.frames << " frame-sets, " << info.cells << " cells of " << info.cell_mm << " mm" << std::endl;
        return 0;
    }

    void release()
    {
        if (params.background.model) pcs_background_destroy(ctx, params.background.model);
        if (learn.model) pcs_background_destroy(ctx, learn.model);
        params.background.model = learn.model = nullptr;
        if (params.tracks.tracker) pcs_tracker_destroy(ctx, params.tracks.tracker);
        params.tracks.tracker = nullptr;
        auto drop = [this](void*& p) { if (p) pcs_device_free(ctx, p); p = nullptr; };
        for (void*& p : d_buf) drop(p);
        for (void*& p : d_count) drop(p);
        for (void*& p : d_block) drop(p);
        drop(d_objects);
        drop(d_n_objects);
        drop(d_object_of);
        drop(d_tracks);
        drop(d_track_stats);
        drop(d_boxes);
        drop(d_plan);
        plan.maps = pcs_plan_maps{};
        params.boxes.d_object_of = nullptr; params.boxes.d_boxes = nullptr;
        params.tracks.d_object_of = nullptr; params.tracks.d_tracks = nullptr; params.tracks.d_stats = nullptr;
    }
};

}  // namespace pcs_filter_chain
