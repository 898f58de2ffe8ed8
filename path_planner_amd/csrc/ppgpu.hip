// ppgpu.hip — C ABI (include/ppgpu.h) over the gfx950 kernels in pp_kernels.h / pp_sampler.h.
//
// Build (see __graft_entry__.build()):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared ppgpu.hip -o libppgpu.so
// -ffp-contract=off is part of the contract: the reference rounds every product and sum
// separately (baseline x86-64), and so must the device code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ppgpu.h"
#include "pp_kernels.h"
#include "pp_sampler.h"

static thread_local std::string g_err = "";
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(call)                                                                              \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(PPGPU_EHIP, std::string(#call) + ": " + hipGetErrorString(_e));            \
    } while (0)

// Workspace of one costing slice: PPEdgeSetup + what the pose sweep leaves for the cover sweep, (256 + 2 * ngp + 12 * nch + 16)
// bytes per edge (~3.6 KB per edge for a 1 500-step horizon: 0.9 GB for the 236 140 edges of the bench step; the Gaussian
// obstacle model adds 8 bytes per step).  A launch whose workspace
// would exceed PP_SLICE_BYTES runs as consecutive slices.  (Running slice i's cover sweep next to slice i+1's pose sweep
// on a second stream was measured and gains nothing: both sweeps are bound by fp64 VALU issue.)
#ifndef PP_PREPASS_MIN_EDGES
#define PP_PREPASS_MIN_EDGES 8192   // launches below this skip pp_k_plan_skips / pp_k_approach_events (their results are optional)
#endif
#ifndef PP_SLICE_BYTES
#define PP_SLICE_BYTES (32ull << 30)
#endif
// Device / pinned allocations made after start-up are what a real-time caller must know about (a hipMalloc or hipHostMalloc inside a
// 100 ms planning cycle costs milliseconds): every growth of a library buffer is counted, with the wall time it took
// (ppgpu_growth_stats; process-wide, the host planner reports the difference over a plan() call).
#include <atomic>
#include <chrono>
static std::atomic<unsigned long long> g_growth_count{0}, g_growth_ns{0};
struct GrowthTimer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~GrowthTimer() {
        g_growth_count.fetch_add(1, std::memory_order_relaxed);
        g_growth_ns.fetch_add((unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(), std::memory_order_relaxed);
    }
};
// A grow-only device array that frees itself (with its owner: the device must be current then).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int reserve(size_t n, bool keep, hipStream_t s) {
        if (n <= cap) return PPGPU_OK;
        GrowthTimer growth;
        size_t ncap = cap ? cap : 64;
        while (ncap < n) ncap *= 2;
        T* np = nullptr;
        HIP_TRY(hipMalloc((void**)&np, ncap * sizeof(T)));
        // from here on a failure gives the new block back: the buffer stays what it was
        hipError_t e = hipSuccess;
        if (keep && p && cap) {
            e = hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
        }
        if (e == hipSuccess && p) e = hipFree(p);
        if (e != hipSuccess) {
            (void)hipFree(np);
            return fail(PPGPU_EHIP, std::string("DevBuf::reserve: ") + hipGetErrorString(e));
        }
        p = np; cap = ncap;
        return PPGPU_OK;
    }
};

// The workspace of the push-order pipeline (pp_k_expand.h; the arrays are described at PPExpandArgs), sized for nv open vertices,
// ns stored samples and k winners per list.
struct ExpandWork {
    DevBuf<double> lengths;             // near lengths of the pipeline; ppgpu_select_nearest's full rows of lengths
    DevBuf<double> probe_min, groupmin, bound, key, len;
    DevBuf<int> near_idx, near_count, groupcnt, count, val, idx;   // idx: the output, [nv][2][k]
    DevBuf<unsigned> fallbacks;
    static long long list_cap(long long ns) {          // candidates per list; pp_k_expand_order filters them down to at most PP_ORD_CAP
        long long cap = 64;
        while (cap < ns && cap < 65536) cap <<= 1;
        return cap;
    }
    static size_t groups_row(long long ns) { return (size_t)((ns + 255) / 256) * (256 / PP_NEAR_GROUP); }
    int reserve(size_t nv, long long ns, int k, hipStream_t st) {
        const size_t lists = nv * 2 * (size_t)list_cap(ns), groups = nv * groups_row(ns);
        int rc;
        if ((rc = lengths.reserve(nv * (size_t)ns * 2, false, st)) || (rc = probe_min.reserve(nv * 2 * PP_PROBE_GROUPS, false, st)) ||
            (rc = near_idx.reserve(nv * (size_t)ns, false, st)) || (rc = near_count.reserve(nv, false, st)) ||
            (rc = groupmin.reserve(groups * 2, false, st)) || (rc = groupcnt.reserve(groups, false, st)) ||
            (rc = bound.reserve(nv * 2, false, st)) || (rc = count.reserve(nv * 2, false, st)) ||
            (rc = key.reserve(lists, false, st)) || (rc = val.reserve(lists, false, st)) || (rc = len.reserve(lists, false, st)) ||
            (rc = idx.reserve(nv * 2 * (size_t)k, false, st)) || (rc = fallbacks.reserve(1, false, st)))
            return rc;
        return PPGPU_OK;
    }
};

#define PP_TIMING_RING 8
// The events around the kernel of a trace call (ppgpu_last_trace_timing, ppgpu_last_cover_trace_timing, ppgpu_last_contact_trace_timing,
// ppgpu_last_clearance_trace_timing).
struct TraceTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_earlier = 0;              // ... of the slices before the last one
    bool timed = false;
};
// The events of one timed costing launch, in stream order except EV_APPROACHED (recorded between EV_POSED and the cover sweep).
// A sliced launch records EV_BEGIN .. EV_COVERED and EV_APPROACHED once per slice, EV_END once.
enum { EV_BEGIN, EV_SOLVED, EV_POSED, EV_COVERED, EV_END, EV_APPROACHED, EV_COUNT };
// The device arrays (DevBuf) free themselves; ~ppgpu_ctx releases the streams, events and pinned blocks.  ppgpu_destroy makes the
// device current and waits for the stream first.
struct ppgpu_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t side_stream = nullptr;                 // pp_k_heuristic_listed runs beside the lane heuristic (cost_heuristic_tail)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool have_cfg = false;
    ppgpu_config cfg{};
    // Map
    DevBuf<uint32_t> grid;
    DevBuf<unsigned char> grid_clear, grid_rowclear;   // clearance map of the grid (PPGrid::clearance) and its row pass
    int rows = 0, cols = 0, wpr = 0;
    double res = 0;
    DevBuf<uint16_t> grid_dist;         // distance map of the grid (ppgpu.h, "chart clearance"): built by the first call that needs it ...
    bool grid_dist_built = false;       // ... after a ppgpu_set_grid (grid_distance)
    // keep-out margin (ppgpu.h, "chart clearance").  `grid` is always the grid as set: the distance map is built from it.  With
    // keepout_limit2 > 0 the launches read grid_keepout instead (grid_bits), and grid_clear is the map of that grid.
    uint32_t keepout_limit2 = 0;
    DevBuf<uint32_t> grid_keepout;      // the effective grid, allocated by the first non-zero limit on a grid
    // reachable water (ppgpu.h): nothing here is allocated, launched or timed before the first call of that section
    DevBuf<uint32_t> reach_labels;      // canonical component labels of the effective grid, built by the first call that needs them ...
    bool reach_labels_built = false;    // ... after a ppgpu_set_grid or a changed keep-out limit (reach_labels_ready)
    DevBuf<unsigned long long> reach_words;   // PP_RW_*: the counters and the sticky error word of the labelling and the reach set
    unsigned long long reach_free = 0, reach_components = 0, reach_cells = 0;
    bool reach_have_seed = false;       // ppgpu_set_reach_seed was called: the seed stays across grids and limits
    double reach_seed_x = 0, reach_seed_y = 0;
    uint32_t reach_seed_label = PPGPU_REACH_NONE;   // of the labels as built last (reach_seed_ready looks it up again after a rebuild)
    bool reach_seed_fresh = false;
    DevBuf<uint32_t> reach_bits;        // the cells with reach_set_label, PPGrid's layout ...
    DevBuf<uint16_t> reach_gap;         // ... and the reach-gap map over them
    bool reach_set_built = false;
    uint32_t reach_set_label = PPGPU_REACH_NONE;
    DevBuf<double> reach_ribbons;       // {sx, sy, ex, ey, len, n} per ribbon of the last ppgpu_ribbon_reach_host
    DevBuf<ppgpu_ribbon_reach_record> reach_records;
    TraceTimer t_reach_labels, t_reach_gap, t_reach_ribbons;   // (events made by the first timed use, like t_keepout's)
    // distance by water (ppgpu.h): nothing here is allocated, launched or timed before the first call of that section
    DevBuf<uint32_t> water_wd;          // the map of water_map_cell, built by the first call that needs it ...
    bool water_built = false;           // ... after a ppgpu_set_grid, a changed keep-out limit or a seed in another cell (water_ready)
    DevBuf<uint32_t> water_ctl;         // [2][tiles] dirty flags (this round's, the next round's), then water_batch words of active tiles
    DevBuf<unsigned long long> water_words;   // PP_WW_*
    unsigned* water_pinned = nullptr;   // the active counts of a batch of rounds, read back in one copy
    int water_batch = 16;               // rounds issued between two reads (PPGPU_WATER_BATCH, 1 .. 64): the map does not depend on it
    bool water_have_seed = false;       // ppgpu_set_water_seed was called: the seed stays across grids and limits
    double water_seed_x = 0, water_seed_y = 0;
    uint32_t water_map_cell = PPGPU_WATER_NONE;   // the seed's cell of the map as built (NONE: a blocked seed, all NONE)
    ppgpu_water_info water_info{};      // of the map as built; builds counts on
    DevBuf<double> water_ribbons;       // {sx, sy, ex, ey, len, n} per ribbon of the last ppgpu_ribbon_water_host
    DevBuf<ppgpu_ribbon_water_record> water_records;
    TraceTimer t_water_map, t_water_ribbons;
    // route by water (ppgpu.h): derived from the water map; nothing here is allocated, launched or timed before the first call of that section
    DevBuf<uint8_t> route_dirs;         // the step map of the water map whose build number is route_dirs_build (0: none yet)
    uint32_t route_dirs_build = 0;
    DevBuf<double> route_points;        // {x, y} per query of the last ppgpu_water_routes_host
    DevBuf<ppgpu_water_route_record> route_records;
    DevBuf<uint32_t> route_vertices;    // [n][vertex_stride]
    TraceTimer t_route_dirs, t_routes;
    // dynamic obstacles
    DevBuf<PPObst> obst;
    int n_obst = 0;
    int obst_model = PPGPU_OBST_NONE;
    // open vertices
    DevBuf<ppgpu_vertex> verts;
    DevBuf<double> ribbons, tgrid;
    int nverts = 0, nribbons = 0, ng = 0;
    // sample (target state) store, SoA
    DevBuf<double> sx, sy, sh;
    long long n_samples = 0;
    long long n_extra = 0;              // explicit target states appended behind the samples (ppgpu_set_extra_targets)
    // sampler (StateGenerator) state
    PPSamplerState sampler{};
    DevBuf<double> samp_ribbons;
    DevBuf<unsigned long long> samp_pos;           // groups of 8 words: [0] stream position (pair slots consumed), [1] sticky chain error, [2..3] report of the last
                                                   // add (pp_k_sampler_advance).  ppgpu_sampler_init moves on to the next group — all zero: "position 0, no error" —
                                                   // and zeroes the whole array again when it wraps: a fresh generator costs no launch of its own
    int samp_group = -1;
    unsigned long long* pinned_counts = nullptr;   // 64 bytes of pinned host memory for the sampler's count read-backs
    std::vector<double> samp_ribbons_host;   // what samp_ribbons holds (ppgpu_sampler_init skips the upload of an unchanged table)
    DevBuf<unsigned char> s_bytes;      // scan / compaction scratch
    DevBuf<unsigned long long> s_u64;
    DevBuf<unsigned> s_u32a, s_u32b;
    DevBuf<double> s_cand;              // candidate states before the map filter
    // scratch for host-convenience entry points and reductions
    DevBuf<unsigned long long> tmp_edges, partial;
    DevBuf<ppgpu_wrapper_edge> tmp_wedges;
    DevBuf<ppgpu_edge_result> tmp_results;
    DevBuf<double> tmp_child, tmp_lengths, tmp_len_out, int_child;
    DevBuf<unsigned char> tmp_trace;       // device end of the host forms of the traces: the step, cover, contact or clearance records of one trace slice
    DevBuf<ppgpu_cover_summary> tmp_summaries;   // ... of ppgpu_trace_cover_*: the summaries and final lists of the whole list
    DevBuf<double> tmp_cover_child;
    DevBuf<int> tmp_counts;
    TraceTimer t_steps, t_cover, t_contacts, t_clearance;   // around pp_k_trace_steps / pp_k_trace_cover / pp_k_trace_contacts / pp_k_trace_clearance
    TraceTimer t_tsp;                   // around the table pass (tsp_table_pass)
    TraceTimer t_dist;                  // around the two passes of the distance map (grid_distance)
    TraceTimer t_keepout;               // around pp_k_keepout_bits and the rebuild of grid_clear (apply_keepout)
    TraceTimer t_arc_stops;             // around pp_k_arc_stops (launch_cost; events made by the first timed use, like t_keepout's)
    bool quiet_finish = true;           // env PPGPU_QUIET_FINISH=0: every edge's phase C stays with its wave
    bool solve_all_words = false;       // env PPGPU_SOLVE_ALL_WORDS=1: the solver evaluates all six words correctly rounded (tests compare the two)
    bool lane_split = true;             // env PPGPU_LANE_SPLIT=0: the wave makes every split itself (tests compare the two)
    bool lane_finish = true;            // env PPGPU_LANE_FINISH=0: every wave of the cover sweep finishes its own edges (tests compare the two)
    bool plan_spans = true;             // env PPGPU_PLAN_SPANS=0: the skip planner tests every obstacle of an edge's list per chunk (the tests compare the two)
    bool lane_heuristic = true;         // env PPGPU_LANE_HEURISTIC=0: large launches keep the wave-per-edge enumeration too (tests compare the two)
    long long prepass_min_edges = PP_PREPASS_MIN_EDGES;   // env PPGPU_PREPASS_MIN_EDGES overrides (tests run the prepasses on small launches too)
    bool share_sweeps = true;           // env PPGPU_SHARE_SWEEPS=0: every edge of a large launch is swept itself (A/B runs, and the tests compare the two)
    bool use_sweep_list = true;         // env PPGPU_SWEEP_LIST=0: the skip planner and the pose sweep walk every edge of a launch with shared sweeps too (A/B runs, and the tests compare the two)
    bool approach_list = true;          // env PPGPU_APPROACH_LIST=0: pp_k_approach_events walks every edge of a slice although the launch has a sweep list (A/B runs: profiles/sweep_list.txt)
    size_t slice_bytes = PP_SLICE_BYTES; // workspace budget of one costing slice (env PPGPU_SLICE_BYTES overrides: tests)
    DevBuf<PPEdgeSetup> setup;          // workspace of the current costing slice: phase-0 records ...
    DevBuf<unsigned short> track_hits;  // ... and the pose sweep's track (see PPParams)
    DevBuf<unsigned long long> track_eq;
    DevBuf<unsigned> track_chunk_hits;
    DevBuf<PPTrackSummary> track_summary;
    DevBuf<int2> track_far;
    DevBuf<unsigned char> track_skip;
    DevBuf<PPLaunchWords> words;        // the counters the kernels of a launch hand to one another (one 128-byte line)
    DevBuf<unsigned> defer_list, live_list, hw_list;
    DevBuf<unsigned> share_head, share_of;   // shared sweeps: the head of each class, and whose results each edge of the launch takes (see PPParams)
    bool share_head_stale = true;            // share_head is not known to be all-ones: it is new, or a launch that shares began and did not get as
                                             // far as pp_k_share_fanout, which leaves it so.  The next launch that shares fills it first
    bool last_launch_shared = false;         // the last costing launch ran with shared sweeps (share_of then holds last_launch_edges entries)
    DevBuf<unsigned> sweep_list;             // ... and the slice positions of the edges the skip planner and the pose sweep walk (pp_k_mark_sweeps)
    long long last_launch_slices = 0, last_slice_edges = 0;   // how the last costing launch was cut (ppgpu_last_slices)
    bool last_launch_listed = false;         // the last costing launch ran with that list (words->swept_total then counts its entries over all slices)
    bool share_tracks = true;                // env PPGPU_SHARE_TRACKS=0: no stop classes, every swept edge is planned and posed itself (A/B runs, and the tests compare the two)
    DevBuf<int> arc_stop;                    // shared tracks: per class the step at which its first arc is blocked (pp_k_arc_stops; see PPParams) ...
    bool arc_stops_stale = true;             // ... which is not known to hold for the vertices, grid, keep-out limit and configuration now set:
                                             // the next launch that shares tracks queues pp_k_arc_stops first
    DevBuf<unsigned> stop_list, stop_of;     // ... and the stop members of the current slice, packed, and per member its head (pp_k_mark_sweeps)
    bool last_launch_tracks = false;         // the last costing launch shared tracks (words->stop_total then counts its stop members)
    DevBuf<PPCoverState> cover_state;
    DevBuf<unsigned long long> work;    // queue heads of the cover sweep's resident grid (pp_next_edge)
    int n_cu = 0;
    int resident[2] = {0, 0};           // workgroups of pp_k_cover_sweep / pp_k_cover_sweep_gaussian the device holds at once (0 = not asked yet)
    DevBuf<double> track_pen, track_chunk_pen;   // Gaussian obstacle model only
    // optional per-kernel timing of costing launches (ppgpu_enable_timing)
    bool timing = false;
    // a ring of event sets: the last PP_TIMING_RING launches can be read back without a host wait between them
    hipEvent_t ev_ring[PP_TIMING_RING][EV_COUNT] = {};
    double ms_ring[PP_TIMING_RING][4] = {};    // solve / pose / cover / approach time of the slices before the last one of a sliced launch (slice_durations)
    int ev_slot = 0;                           // the set of the launch being recorded / recorded last
    long long last_launch_edges = 0;           // edges of the last costing launch, and whether its cover sweep took a packed list
    bool last_launch_packed = false;           // (then the list's length is words->live_count: last slice)
    long long live_earlier_slices = 0;
    long long ev_launches = 0;                 // timed launches so far
    int max_vertex_ribbons = 0;
    DevBuf<int> tmp_idx;
    ExpandWork expand;                  // the push-order pipeline's workspace (launch_expand_order)
    unsigned long long order_fallbacks = 0;   // (vertex, radius) lists of ppgpu_expand_host / ppgpu_expand_order that fell back to ascending length
    DevBuf<unsigned char> dstage_in, dstage_out;            // device ends of ppgpu_expand_host's single upload / download
    void* stage_in = nullptr; size_t stage_in_cap = 0;      // pinned host staging of ppgpu_expand_host
    void* stage_out = nullptr; size_t stage_out_cap = 0;
    DevBuf<unsigned long long> gather;
    void* comm = nullptr;               // ncclComm_t owned by the handle (ppgpu_comm_init_rank / ppgpu_comm_init_all)
    // ppgpu_copy_engine_read: the HSA agents of this device and of the host, the completion signal of the copy in flight
    unsigned long long hsa_gpu = 0, hsa_cpu = 0, hsa_signal = 0;
    bool copy_pending = false;
    // the table pass over long child lists (ppgpu_set_tsp_table): 0 = off
    int tsp_table_min = 0, tsp_table_max = 0;
    int tsp_dubins_min = 0, tsp_dubins_max = 0;   // ... over those of the Dubins-TSP heuristics (ppgpu_set_dubins_tsp_table): 0 = off
    int tsp_table_cap = 0;              // the workspace holds at least one slot for a list of this many ribbons
    DevBuf<unsigned char> tsp_slots;
    DevBuf<unsigned> tsp_list;
    DevBuf<double> tsp_T;               // Dubins switch only: the Dubins-length tables of the listed records (PP_TT_TCAP of them)
    DevBuf<unsigned long long> tsp_words;   // [0] lists answered, [1] lists refused, [2] length of the list of the launch under way

    __attribute__((visibility("hidden"))) ~ppgpu_ctx() {          // (the library exports nothing new)
        for (void* pinned : {(void*)pinned_counts, (void*)water_pinned, stage_in, stage_out}) if (pinned) (void)hipHostFree(pinned);
        for (auto& set : ev_ring) for (hipEvent_t e : set) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {t_steps.ev[0], t_steps.ev[1], t_cover.ev[0], t_cover.ev[1], t_contacts.ev[0], t_contacts.ev[1], t_clearance.ev[0], t_clearance.ev[1], t_tsp.ev[0], t_tsp.ev[1], t_dist.ev[0], t_dist.ev[1], t_keepout.ev[0], t_keepout.ev[1], t_arc_stops.ev[0], t_arc_stops.ev[1],
                             t_reach_labels.ev[0], t_reach_labels.ev[1], t_reach_gap.ev[0], t_reach_gap.ev[1], t_reach_ribbons.ev[0], t_reach_ribbons.ev[1],
                             t_water_map.ev[0], t_water_map.ev[1], t_water_ribbons.ev[0], t_water_ribbons.ev[1],
                             t_route_dirs.ev[0], t_route_dirs.ev[1], t_routes.ev[0], t_routes.ev[1], ev_fork, ev_join}) if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {side_stream, own_stream}) if (s) (void)hipStreamDestroy(s);
    }
};

static int require_cfg(ppgpu_ctx* c) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (!c->have_cfg) return fail(PPGPU_ESTATE, "ppgpu_set_config must be called first");
    return PPGPU_OK;
}

// the forms that take their curves from the caller need open vertices but no targets
static int require_vertices(ppgpu_ctx* c) {
    int rc = require_cfg(c);
    if (rc) return rc;
    if (c->nverts <= 0) return fail(PPGPU_ESTATE, "ppgpu_set_vertices must be called (after ppgpu_set_config)");
    return PPGPU_OK;
}

static int require_world(ppgpu_ctx* c) {
    int rc = require_vertices(c);
    if (rc) return rc;
    if (c->n_samples + c->n_extra <= 0) return fail(PPGPU_ESTATE, "no targets: call ppgpu_sampler_add, ppgpu_set_samples or ppgpu_set_extra_targets");
    return PPGPU_OK;
}

// Checks of what an entry point was handed; `who` is its name in the message.
static int check_open_vertices(const ppgpu_ctx* c, const char* who, int n, const ppgpu_vertex* hv, int n_ribbons, int* max_ribbons) {
    *max_ribbons = 0;
    for (int i = 0; i < n; i++) {
        if (hv[i].ribbon_count < 0 || hv[i].ribbon_offset < 0 || hv[i].ribbon_offset + hv[i].ribbon_count > n_ribbons)
            return fail(PPGPU_EINVAL, std::string(who) + ": ribbon range outside the pool");
        if (hv[i].ribbon_count > PP_WAVE) return fail(PPGPU_ECAPACITY, std::string(who) + ": more than 64 ribbons on one vertex");
        if (hv[i].time < c->cfg.start_state_time) return fail(PPGPU_EINVAL, std::string(who) + ": vertex time before start_state_time");
        if (hv[i].ribbon_count > *max_ribbons) *max_ribbons = hv[i].ribbon_count;
    }
    return PPGPU_OK;
}

static int check_wrapper_edges(const ppgpu_ctx* c, const char* who, int64_t n, const ppgpu_wrapper_edge* w) {
    for (int64_t i = 0; i < n; i++) {
        if (!(w[i].rho > 0) || !(w[i].speed > 0)) return fail(PPGPU_EINVAL, std::string(who) + ": rho and speed must be positive");
        if (w[i].vertex < 0 || w[i].vertex >= c->nverts) return fail(PPGPU_EINVAL, std::string(who) + ": vertex out of range");
    }
    return PPGPU_OK;
}

namespace { struct CtxDelete { void operator()(ppgpu_ctx* c) const { delete c; } }; }     // (internal linkage: ppgpu_create's guard)
static void ppgpu_copy_engine_release(ppgpu_ctx* c);      // (further down, with the HSA entry points)
extern "C" int ppgpu_copy_engine_wait(ppgpu_ctx* c);

extern "C" {

const char* ppgpu_last_error(void) { return g_err.c_str(); }

int ppgpu_create(int device, ppgpu_ctx** out) {
    if (!out) return fail(PPGPU_EINVAL, "out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(PPGPU_ENODEV, "no HIP device visible");
    if (device < 0 || device >= n) return fail(PPGPU_ENODEV, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PPGPU_ENODEV, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    std::unique_ptr<ppgpu_ctx, CtxDelete> c(new ppgpu_ctx());      // (an early return below frees what was made so far)
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIP_TRY(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc((void**)&c->pinned_counts, 64, hipHostMallocDefault));
    if (const char* pm = std::getenv("PPGPU_PREPASS_MIN_EDGES")) c->prepass_min_edges = std::atoll(pm);
    if (const char* lh = std::getenv("PPGPU_LANE_HEURISTIC")) c->lane_heuristic = std::atoi(lh) != 0;
    if (const char* qf = std::getenv("PPGPU_QUIET_FINISH")) c->quiet_finish = std::atoi(qf) != 0;
    if (const char* lf = std::getenv("PPGPU_LANE_FINISH")) c->lane_finish = std::atoi(lf) != 0;
    if (const char* ls = std::getenv("PPGPU_LANE_SPLIT")) c->lane_split = std::atoi(ls) != 0;
    if (const char* aw = std::getenv("PPGPU_SOLVE_ALL_WORDS")) c->solve_all_words = std::atoi(aw) != 0;
    if (const char* ps = std::getenv("PPGPU_PLAN_SPANS")) c->plan_spans = std::atoi(ps) != 0;
    if (const char* ss = std::getenv("PPGPU_SHARE_SWEEPS")) c->share_sweeps = std::atoi(ss) != 0;
    if (const char* sl = std::getenv("PPGPU_SWEEP_LIST")) c->use_sweep_list = std::atoi(sl) != 0;
    if (const char* al = std::getenv("PPGPU_APPROACH_LIST")) c->approach_list = std::atoi(al) != 0;
    if (const char* tr = std::getenv("PPGPU_SHARE_TRACKS")) c->share_tracks = std::atoi(tr) != 0;
    if (const char* wb = std::getenv("PPGPU_WATER_BATCH")) c->water_batch = std::min(64, std::max(1, std::atoi(wb)));
    if (const char* sb = std::getenv("PPGPU_SLICE_BYTES")) {
        const long long v = std::atoll(sb);
        if (v > 0) c->slice_bytes = (size_t)v;
    }
    *out = c.release();
    return PPGPU_OK;
}

int ppgpu_destroy(ppgpu_ctx* c) {
    if (!c) return PPGPU_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)ppgpu_comm_destroy(c);
    if (c->copy_pending) (void)ppgpu_copy_engine_wait(c);
    ppgpu_copy_engine_release(c);
    delete c;
    return PPGPU_OK;
}

int ppgpu_set_stream(ppgpu_ctx* c, void* s) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return PPGPU_OK;
}

int ppgpu_enable_timing(ppgpu_ctx* c, int32_t on) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (on && !c->ev_ring[0][0])
        for (int r = 0; r < PP_TIMING_RING; r++) for (int i = 0; i < EV_COUNT; i++) HIP_TRY(hipEventCreate(&c->ev_ring[r][i]));
    for (TraceTimer* tm : {&c->t_steps, &c->t_cover, &c->t_contacts, &c->t_clearance, &c->t_tsp, &c->t_dist}) {
        if (on && !tm->ev[0])
            for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreate(&tm->ev[i]));
        tm->timed = false;
    }
    c->t_keepout.timed = false;         // (its events are made by the first timed change of the keep-out: apply_keepout)
    c->t_arc_stops.timed = false;       // (... by the first timed walk of the classes' arcs: launch_cost)
    c->t_reach_labels.timed = c->t_reach_gap.timed = c->t_reach_ribbons.timed = false;   // (... by the first timed build or walk)
    c->t_water_map.timed = c->t_water_ribbons.timed = false;
    c->t_route_dirs.timed = c->t_routes.timed = false;
    c->timing = on != 0;
    c->ev_launches = 0;
    return PPGPU_OK;
}

// Solve, pose sweep, cover sweep and approach prepass of the slice an event set recorded last (its EV_COVERED has been waited for).
// The cover sweep alone: from EV_APPROACHED.
static int slice_durations(hipEvent_t* ev, float ms[4]) {
    HIP_TRY(hipEventElapsedTime(&ms[0], ev[EV_BEGIN], ev[EV_SOLVED]));
    HIP_TRY(hipEventElapsedTime(&ms[1], ev[EV_SOLVED], ev[EV_POSED]));
    HIP_TRY(hipEventElapsedTime(&ms[2], ev[EV_APPROACHED], ev[EV_COVERED]));
    HIP_TRY(hipEventElapsedTime(&ms[3], ev[EV_POSED], ev[EV_APPROACHED]));
    return PPGPU_OK;
}

int ppgpu_past_timing(ppgpu_ctx* c, int32_t back, double* ms_solve, double* ms_pose, double* ms_cover, double* ms_heuristic) {
    if (!c || !ms_solve || !ms_pose || !ms_cover || !ms_heuristic) return fail(PPGPU_EINVAL, "null argument");
    if (!c->timing || c->ev_launches == 0) return fail(PPGPU_ESTATE, "no timed costing launch (ppgpu_enable_timing, then cost edges)");
    if (back < 0 || back >= PP_TIMING_RING || back >= c->ev_launches) return fail(PPGPU_EINVAL, "past_timing: that launch is no longer (or not yet) in the ring");
    HIP_TRY(hipSetDevice(c->device));
    const int slot = (c->ev_slot - back + PP_TIMING_RING) % PP_TIMING_RING;
    hipEvent_t* ev = c->ev_ring[slot];
    HIP_TRY(hipEventSynchronize(ev[EV_END]));
    float t[4] = {0, 0, 0, 0}, tail = 0;
    int rc = slice_durations(ev, t);
    if (rc) return rc;
    HIP_TRY(hipEventElapsedTime(&tail, ev[EV_COVERED], ev[EV_END]));
    *ms_solve = t[0] + c->ms_ring[slot][0]; *ms_pose = t[1] + c->ms_ring[slot][1]; *ms_cover = t[2] + c->ms_ring[slot][2];
    *ms_heuristic = tail + t[3] + c->ms_ring[slot][3];               // the heuristic tail and the approach prepass
    return PPGPU_OK;
}
int ppgpu_last_timing(ppgpu_ctx* c, double* ms_solve, double* ms_pose, double* ms_cover, double* ms_heuristic) {
    return ppgpu_past_timing(c, 0, ms_solve, ms_pose, ms_cover, ms_heuristic);
}

int ppgpu_last_cover_edges(ppgpu_ctx* c, int64_t* n_edges) {
    if (!c || !n_edges) return fail(PPGPU_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    *n_edges = c->last_launch_edges;
    if (c->last_launch_packed) {
        unsigned live = 0;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(&live, &c->words.p->live_count, sizeof(unsigned), hipMemcpyDeviceToHost));
        *n_edges = (int64_t)live + c->live_earlier_slices;
    }
    return PPGPU_OK;
}

int ppgpu_last_shared_edges(ppgpu_ctx* c, int64_t* n_edges) {
    if (!c || !n_edges) return fail(PPGPU_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    *n_edges = 0;
    if (!c->last_launch_shared || c->last_launch_edges <= 0) return PPGPU_OK;
    std::vector<unsigned> of((size_t)c->last_launch_edges);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(of.data(), c->share_of.p, of.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (unsigned h : of) n += (h != PP_SHARE_NONE);
    *n_edges = n;
    return PPGPU_OK;
}

int ppgpu_last_slices(ppgpu_ctx* c, int64_t* n_slices, int64_t* last_slice_edges) {
    if (!c || !n_slices || !last_slice_edges) return fail(PPGPU_EINVAL, "null argument");
    *n_slices = c->last_launch_slices; *last_slice_edges = c->last_slice_edges;
    return PPGPU_OK;
}

int ppgpu_last_swept_edges(ppgpu_ctx* c, int64_t* n_edges) {
    if (!c || !n_edges) return fail(PPGPU_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    *n_edges = c->last_launch_edges;
    if (c->last_launch_listed) {
        unsigned swept = 0;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(&swept, &c->words.p->swept_total, sizeof(unsigned), hipMemcpyDeviceToHost));
        *n_edges = (int64_t)swept;
    }
    return PPGPU_OK;
}

int ppgpu_last_stop_members(ppgpu_ctx* c, int64_t* n_edges) {
    if (!c || !n_edges) return fail(PPGPU_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    *n_edges = 0;
    if (c->last_launch_tracks) {
        unsigned members = 0;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(&members, &c->words.p->stop_total, sizeof(unsigned), hipMemcpyDeviceToHost));
        *n_edges = (int64_t)members;
    }
    return PPGPU_OK;
}

int ppgpu_reserve_samples(ppgpu_ctx* c, int64_t max_samples, int32_t max_vertices) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (max_samples <= 0 || max_vertices <= 0) return fail(PPGPU_EINVAL, "reserve_samples: sizes must be positive");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t ns = (size_t)max_samples, nv = (size_t)max_vertices;
    const size_t nq = 6 * (size_t)524288 + 8;                   // the sampler's largest batch (ppgpu_sampler_add)
    int rc;
    if ((rc = c->sx.reserve(ns + nv, true, st)) || (rc = c->sy.reserve(ns + nv, true, st)) || (rc = c->sh.reserve(ns + nv, true, st)) ||
        (rc = c->s_cand.reserve((size_t)524288 * 3, false, st)) || (rc = c->s_bytes.reserve(nq + 64, false, st)) || (rc = c->s_u32a.reserve(nq + 64, false, st)) ||
        (rc = c->expand.reserve(nv, max_samples, 0, st)))           // (the output grows with the k of the first call)
        return rc;
    return PPGPU_OK;
}

int ppgpu_growth_stats(ppgpu_ctx* c, uint64_t* count, double* seconds) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (count) *count = g_growth_count.load(std::memory_order_relaxed);
    if (seconds) *seconds = 1e-9 * (double)g_growth_ns.load(std::memory_order_relaxed);
    return PPGPU_OK;
}

// The two switches of the table pass: one workspace (slots sized for the larger of the two ranges, grow-only), one range each.
static int set_table_range(ppgpu_ctx* c, int32_t min_ribbons, int32_t max_ribbons, int& range_min, int& range_max, bool dubins) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (min_ribbons < 0 || max_ribbons < 0 || max_ribbons > PP_TSP_TABLE_MAX || (max_ribbons > 0 && min_ribbons > max_ribbons))
        return fail(PPGPU_EINVAL, "set_tsp_table: 0 <= min_ribbons <= max_ribbons <= 16 (max_ribbons = 0: off)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));            // no launch under way reads the fields or the slots
    if (max_ribbons > 0) {
        // as many slots as the budget holds, each for lists of max_ribbons (grow-only: a later, smaller range keeps the larger slots)
        int rc = c->tsp_words.p ? PPGPU_OK : c->tsp_words.reserve(4, false, c->stream);
        if (rc) return rc;
        if (c->tsp_table_cap == 0) HIP_TRY(hipMemsetAsync(c->tsp_words.p, 0, 4 * sizeof(unsigned long long), c->stream));
        const int cap = max_ribbons > c->tsp_table_cap ? max_ribbons : c->tsp_table_cap;
        size_t slots = (size_t)PP_TSP_TABLE_BYTES / pp_tt_slot_bytes(cap);
        if (slots > PP_TT_GRID) slots = PP_TT_GRID;
        if (slots < 1) return fail(PPGPU_ECAPACITY, "set_tsp_table: PP_TSP_TABLE_BYTES holds no slot");
        if (cap != c->tsp_table_cap) {
            // (exactly what is asked for: DevBuf rounds up to a power of two of its first size, so the first size is the whole)
            if (c->tsp_slots.p) { HIP_TRY(hipFree(c->tsp_slots.p)); c->tsp_slots.p = nullptr; c->tsp_slots.cap = 0; }
            GrowthTimer growth;
            HIP_TRY(hipMalloc((void**)&c->tsp_slots.p, slots * pp_tt_slot_bytes(cap)));
            c->tsp_slots.cap = slots * pp_tt_slot_bytes(cap);
            c->tsp_table_cap = cap;
        }
        // room for a million listed records per launch, allocated here and never in a costing call; what does not fit stays with the host
        if ((rc = c->tsp_list.reserve(1u << 20, false, c->stream))) return rc;
        if (dubins && (rc = c->tsp_T.reserve((size_t)PP_TT_TCAP * PP_TT_TSTRIDE, false, c->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    range_min = min_ribbons; range_max = max_ribbons;
    return PPGPU_OK;
}

int ppgpu_set_tsp_table(ppgpu_ctx* c, int32_t min_ribbons, int32_t max_ribbons) {
    return c ? set_table_range(c, min_ribbons, max_ribbons, c->tsp_table_min, c->tsp_table_max, false) : fail(PPGPU_EINVAL, "null context");
}

int ppgpu_set_dubins_tsp_table(ppgpu_ctx* c, int32_t min_ribbons, int32_t max_ribbons) {
    return c ? set_table_range(c, min_ribbons, max_ribbons, c->tsp_dubins_min, c->tsp_dubins_max, true) : fail(PPGPU_EINVAL, "null context");
}

int ppgpu_tsp_table_stats(ppgpu_ctx* c, uint64_t* lists, uint64_t* refused) {
    if (!c || !lists || !refused) return fail(PPGPU_EINVAL, "null argument");
    unsigned long long w[2] = {0, 0};
    if (c->tsp_words.p) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpyAsync(w, c->tsp_words.p, sizeof(w), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *lists = w[0]; *refused = w[1];
    return PPGPU_OK;
}

int ppgpu_synchronize(ppgpu_ctx* c) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

int ppgpu_device_alloc(ppgpu_ctx* c, uint64_t bytes, void** d_out) {
    if (!c || !d_out || bytes == 0) return fail(PPGPU_EINVAL, "device_alloc: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(d_out, (size_t)bytes));
    return PPGPU_OK;
}
int ppgpu_device_free(ppgpu_ctx* c, void* d_ptr) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (!d_ptr) return PPGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(d_ptr));
    return PPGPU_OK;
}
int ppgpu_device_read(ppgpu_ctx* c, void* h_dst, const void* d_src, uint64_t bytes) {
    if (!c || !h_dst || !d_src) return fail(PPGPU_EINVAL, "device_read: null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

int ppgpu_set_config(ppgpu_ctx* c, const ppgpu_config* cfg) {
    if (!c || !cfg) return fail(PPGPU_EINVAL, "null argument");
    if (!(cfg->max_speed > 0) || !(cfg->collision_checking_increment > 0) || !(cfg->turning_radius > 0) ||
        !(cfg->coverage_turning_radius > 0) || !(cfg->time_horizon > 0))
        return fail(PPGPU_EINVAL, "config: speeds, radii, increment and horizon must be positive");
    if (cfg->heuristic < PPGPU_H_MAX_DISTANCE || cfg->heuristic > PPGPU_H_TSP_DUBINS_K)
        return fail(PPGPU_EINVAL, "config: unknown heuristic");
    if ((cfg->heuristic == PPGPU_H_TSP_DUBINS_ALL || cfg->heuristic == PPGPU_H_TSP_DUBINS_K) && !(cfg->heuristic_turning_radius > 0))
        return fail(PPGPU_EINVAL, "config: the Dubins-TSP heuristics need heuristic_turning_radius > 0 "
                                  "(RibbonManager throws \"Cannot compute ribbon dubins distance with unset turning radius\")");
    double steps = cfg->time_horizon / (cfg->collision_checking_increment / cfg->max_speed);
    if (!(steps < 60000.0)) return fail(PPGPU_ECAPACITY, "config: more than 60000 collision-check steps per edge");
    c->cfg = *cfg;
    c->have_cfg = true;
    c->ng = (int)steps + 8;
    c->nverts = 0;  // time grids depend on the config: vertices must be set again
    c->arc_stops_stale = true;
    return PPGPU_OK;
}

// The bit grid the launches read (PPGrid::bits): the grid as set, or the effective grid of the keep-out.
static const uint32_t* grid_bits(const ppgpu_ctx* c) { return c->keepout_limit2 ? c->grid_keepout.p : c->grid.p; }
// The chessboard clearance map of `bits` into grid_clear (two separable passes on the stream).
static void launch_grid_clear(ppgpu_ctx* c, const uint32_t* bits, int rows, int cols, int wpr) {
    const long long ncell = (long long)rows * cols;
    hipLaunchKernelGGL(pp_k_grid_row_clear, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, c->stream, bits, rows, cols, wpr, c->grid_rowclear.p);
    hipLaunchKernelGGL(pp_k_grid_clear, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, c->stream, c->grid_rowclear.p, rows, cols, c->grid_clear.p);
}
static int apply_keepout(ppgpu_ctx* c);                  // (further down, with the distance map it thresholds)

int ppgpu_set_grid(ppgpu_ctx* c, const uint8_t* cells, int32_t rows, int32_t cols, double res) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipSetDevice(c->device));
    c->grid_dist_built = false;
    c->arc_stops_stale = true;                          // (the first launch that shares tracks walks the classes' arcs over the new grid)
    c->reach_labels_built = false;                      // (stale: the first call that needs the labels builds them)
    c->water_built = false;                             // (likewise the distance by water)
    if (rows == 0) { c->rows = c->cols = c->wpr = 0; c->res = 0; return PPGPU_OK; }
    if (!cells || rows < 0 || cols <= 0 || !(res > 0)) return fail(PPGPU_EINVAL, "grid: bad shape or resolution");
    int wpr = (cols + 31) / 32;
    std::vector<uint32_t> bits((size_t)rows * wpr, 0u);
    for (int r = 0; r < rows; r++) {
        const uint8_t* row = cells + (size_t)r * cols;
        uint32_t* brow = bits.data() + (size_t)r * wpr;
        for (int x = 0; x < cols; x++)
            if (row[x]) brow[x >> 5] |= 1u << (x & 31);
    }
    int rc = c->grid.reserve(bits.size(), false, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->grid.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    // clearance map: chessboard distance to the nearest blocked-or-outside cell, capped (two separable passes on the device)
    if ((rc = c->grid_clear.reserve((size_t)rows * cols, false, c->stream)) || (rc = c->grid_rowclear.reserve((size_t)rows * cols, false, c->stream)))
        return rc;
    if (c->keepout_limit2) {                            // the kernels read the effective grid: the map is built over that one
        c->rows = rows; c->cols = cols; c->wpr = wpr; c->res = res;
        return apply_keepout(c);
    }
    launch_grid_clear(c, c->grid.p, rows, cols, wpr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->rows = rows; c->cols = cols; c->wpr = wpr; c->res = res;
    return PPGPU_OK;
}

int ppgpu_get_grid_clearance(ppgpu_ctx* c, uint8_t* h_out, int64_t capacity) {
    if (!c || !h_out) return fail(PPGPU_EINVAL, "grid clearance: null argument");
    if (c->rows == 0) return fail(PPGPU_EINVAL, "grid clearance: no grid is set");
    const int64_t ncell = (int64_t)c->rows * c->cols;
    if (capacity < ncell) return fail(PPGPU_EINVAL, "grid clearance: capacity below rows * cols");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(h_out, c->grid_clear.p, (size_t)ncell, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ chart clearance
// The distance map of the grid that is set (rows > 0), built on the stream by the first caller after a ppgpu_set_grid and kept
// until the next: the column pass into a scratch array that lives for the build only, then the row pass (pp_k_distance.h).
static int grid_distance(ppgpu_ctx* c) {
    if (c->grid_dist_built) return PPGPU_OK;
    const size_t ncell = (size_t)c->rows * c->cols;
    int rc = c->grid_dist.reserve(ncell, false, c->stream);
    if (rc) return rc;
    DevBuf<uint16_t> v;
    if ((rc = v.reserve(ncell, false, c->stream))) return rc;
    const unsigned ctiles = (unsigned)((c->cols + 255) / 256), rtiles = (unsigned)((c->rows + PP_DIST_TILE - 1) / PP_DIST_TILE);
    if (ctiles > 65535u || rtiles > 65535u) return fail(PPGPU_ECAPACITY, "grid distance: the grid is too large for the map's launch shape");
    c->t_dist.ms_earlier = 0;
    c->t_dist.timed = false;
    if (c->timing) HIP_TRY(hipEventRecord(c->t_dist.ev[0], c->stream));
    hipLaunchKernelGGL(pp_k_dist_cols<true>, dim3(ctiles, rtiles), dim3(256), 0, c->stream, c->grid.p, c->rows, c->cols, c->wpr, v.p);
    hipLaunchKernelGGL(pp_k_dist_rows<true>, dim3((unsigned)c->rows, ctiles), dim3(256), 0, c->stream, v.p, c->rows, c->cols, c->grid_dist.p);
    if (c->timing) { HIP_TRY(hipEventRecord(c->t_dist.ev[1], c->stream)); c->t_dist.timed = true; }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));       // the scratch goes with this scope
    c->grid_dist_built = true;
    return PPGPU_OK;
}

int ppgpu_get_grid_distance(ppgpu_ctx* c, uint16_t* h_out, int64_t capacity) {
    if (!c || !h_out) return fail(PPGPU_EINVAL, "grid distance: null argument");
    if (c->rows == 0) return fail(PPGPU_EINVAL, "grid distance: no grid is set");
    const int64_t ncell = (int64_t)c->rows * c->cols;
    if (capacity < ncell) return fail(PPGPU_EINVAL, "grid distance: capacity below rows * cols");
    HIP_TRY(hipSetDevice(c->device));
    int rc = grid_distance(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h_out, c->grid_dist.p, (size_t)ncell * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

int ppgpu_grid_clearance_at(ppgpu_ctx* c, int64_t n, const double* h_xy2, double* h_clearance, uint32_t* h_gap2) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (n < 0 || (n > 0 && !h_xy2)) return fail(PPGPU_EINVAL, "grid_clearance_at: bad arguments");
    if (n == 0 || (!h_clearance && !h_gap2)) return PPGPU_OK;
    if (c->rows == 0) {                             // the base Map charts nothing
        for (int64_t i = 0; i < n; i++) {
            if (h_clearance) h_clearance[i] = DBL_MAX;
            if (h_gap2) h_gap2[i] = PPGPU_DIST_CAP2;
        }
        return PPGPU_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc = grid_distance(c);
    if (rc || (rc = c->tmp_lengths.reserve((size_t)n * 2, false, st)) || (h_clearance && (rc = c->tmp_len_out.reserve((size_t)n, false, st))) ||
        (h_gap2 && (rc = c->tmp_counts.reserve((size_t)n, false, st))))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->tmp_lengths.p, h_xy2, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    const PPGrid g{c->grid.p, c->rows, c->cols, c->wpr, c->res, 1.0 / c->res, nullptr};
    hipLaunchKernelGGL(pp_k_grid_clearance_at, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, c->grid_dist.p, (long long)n, c->tmp_lengths.p,
                       h_clearance ? c->tmp_len_out.p : nullptr, h_gap2 ? (unsigned*)c->tmp_counts.p : nullptr);
    HIP_TRY(hipGetLastError());
    if (h_clearance) HIP_TRY(hipMemcpyAsync(h_clearance, c->tmp_len_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (h_gap2) HIP_TRY(hipMemcpyAsync(h_gap2, c->tmp_counts.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ keep-out margin
int ppgpu_keepout_limit2(double resolution, double margin, uint32_t* limit2) {
    if (!limit2) return fail(PPGPU_EINVAL, "keepout_limit2: null argument");
    if (margin != margin) return fail(PPGPU_EINVAL, "keepout_limit2: the margin is not a number");
    *limit2 = 0;
    if (!(margin > 0)) return PPGPU_OK;
    if (!(resolution > 0)) return fail(PPGPU_EINVAL, "keepout_limit2: the resolution must be positive");
    if (margin > PPGPU_DIST_CAP * resolution) return fail(PPGPU_EINVAL, "keepout_limit2: margin above 255 cells");
    const double q = margin / resolution;           // the real answer is ceil(q * q); the roundings move it by a few at most
    long long k = (long long)(q * q) - 2;
    if (k < 0) k = 0;
    while (resolution * std::sqrt((double)k) < margin) k++;                   // (ends by PPGPU_DIST_CAP2: the check above)
    while (k > 0 && resolution * std::sqrt((double)(k - 1)) >= margin) k--;
    *limit2 = (uint32_t)k;
    return PPGPU_OK;
}

// The grid that is set (rows > 0) follows keepout_limit2 from here on: the effective bits (pp_k_keepout_bits over the distance
// map; at limit 0 they are the grid as set, no copy) and the chessboard clearance map over them, which the skip planner culls with.
static int apply_keepout(ppgpu_ctx* c) {
    hipStream_t st = c->stream;
    int rc = PPGPU_OK;
    c->arc_stops_stale = true;                          // the arcs stop on the effective grid
    c->reach_labels_built = false;                      // the labels are those of the effective grid
    c->water_built = false;                             // ... and so is the distance by water
    if (c->keepout_limit2) {
        const unsigned ctiles = (unsigned)((c->cols + 255) / 256);
        if (ctiles > 65535u) return fail(PPGPU_ECAPACITY, "keep-out: the grid is too wide for the kernel's launch shape");
        if ((rc = grid_distance(c)) || (rc = c->grid_keepout.reserve((size_t)c->rows * c->wpr, false, st)) ||
            (rc = c->grid_clear.reserve((size_t)c->rows * c->cols, false, st)) || (rc = c->grid_rowclear.reserve((size_t)c->rows * c->cols, false, st)))
            return rc;
    }
    TraceTimer& tm = c->t_keepout;
    tm.ms_earlier = 0;
    tm.timed = false;
    if (c->timing) {
        if (!tm.ev[0])
            for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreate(&tm.ev[i]));
        HIP_TRY(hipEventRecord(tm.ev[0], st));
    }
    if (c->keepout_limit2)
        hipLaunchKernelGGL(pp_k_keepout_bits, dim3((unsigned)c->rows, (unsigned)((c->cols + 255) / 256)), dim3(256), 0, st, c->grid_dist.p, c->rows, c->cols,
                           c->wpr, c->keepout_limit2, c->grid_keepout.p);
    launch_grid_clear(c, grid_bits(c), c->rows, c->cols, c->wpr);
    if (c->timing) { HIP_TRY(hipEventRecord(tm.ev[1], st)); tm.timed = true; }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return PPGPU_OK;
}

int ppgpu_set_keepout_limit2(ppgpu_ctx* c, uint32_t limit2) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (limit2 > PPGPU_DIST_CAP2) return fail(PPGPU_EINVAL, "set_keepout_limit2: limit2 above PPGPU_DIST_CAP2");
    if (limit2 == c->keepout_limit2) return PPGPU_OK;
    if (c->rows == 0) { c->keepout_limit2 = limit2; return PPGPU_OK; }      // the base Map charts nothing: kept for the next grid
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));       // launches under way still read the bits and the map this call rewrites
    const uint32_t was = c->keepout_limit2;
    c->keepout_limit2 = limit2;
    const int rc = apply_keepout(c);
    if (rc && was == 0) c->keepout_limit2 = 0;      // (the effective grid may not exist: the launches stay on the grid as set)
    return rc;
}

int ppgpu_get_keepout_limit2(ppgpu_ctx* c, uint32_t* limit2) {
    if (!c || !limit2) return fail(PPGPU_EINVAL, "get_keepout_limit2: null argument");
    *limit2 = c->keepout_limit2;
    return PPGPU_OK;
}

int ppgpu_get_grid_blocked(ppgpu_ctx* c, uint8_t* h_out, int64_t capacity) {
    if (!c || !h_out) return fail(PPGPU_EINVAL, "grid blocked: null argument");
    if (c->rows == 0) return fail(PPGPU_EINVAL, "grid blocked: no grid is set");
    const int64_t ncell = (int64_t)c->rows * c->cols;
    if (capacity < ncell) return fail(PPGPU_EINVAL, "grid blocked: capacity below rows * cols");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint32_t> bits((size_t)c->rows * c->wpr);
    HIP_TRY(hipMemcpyAsync(bits.data(), grid_bits(c), bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int r = 0; r < c->rows; r++)
        for (int x = 0; x < c->cols; x++) h_out[(size_t)r * c->cols + x] = (uint8_t)((bits[(size_t)r * c->wpr + (x >> 5)] >> (x & 31)) & 1u);
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ reachable water
// Events of a reach timer are made by its first timed use; begin / end go around the launches on the stream.
static int reach_timer_begin(ppgpu_ctx* c, TraceTimer& tm) {
    tm.ms_earlier = 0;
    tm.timed = false;
    if (!c->timing) return PPGPU_OK;
    if (!tm.ev[0])
        for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreate(&tm.ev[i]));
    HIP_TRY(hipEventRecord(tm.ev[0], c->stream));
    return PPGPU_OK;
}
static int reach_timer_end(ppgpu_ctx* c, TraceTimer& tm) {
    if (c->timing) { HIP_TRY(hipEventRecord(tm.ev[1], c->stream)); tm.timed = true; }
    return PPGPU_OK;
}
// The PP_RW_* words of the launches just issued, after a wait for the stream.
static int reach_read_words(ppgpu_ctx* c, unsigned long long* h_words) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_words, c->reach_words.p, PP_RW_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

// What the getters of this section refuse (rows > 0 from here on).
static int reach_check_grid(const ppgpu_ctx* c, const char* who, const void* h_out, int64_t capacity) {
    if (!c || !h_out) return fail(PPGPU_EINVAL, std::string(who) + ": null argument");
    if (c->rows == 0) return fail(PPGPU_EINVAL, std::string(who) + ": no grid is set");
    const int64_t ncell = (int64_t)c->rows * c->cols;
    if (capacity < ncell) return fail(PPGPU_EINVAL, std::string(who) + ": capacity below rows * cols");
    if (ncell >= 0xFFFFFFFFll) return fail(PPGPU_EINVAL, std::string(who) + ": rows * cols must be below 2^32 - 1 (a label is a 32-bit cell index)");
    return PPGPU_OK;
}

// The labels of the effective grid (rows > 0, rows * cols < 2^32 - 1): three launches whatever the grid holds (pp_k_reach.h), then
// one read-back of the counters and of the error word.
static int reach_labels_ready(ppgpu_ctx* c) {
    if (c->reach_labels_built) return PPGPU_OK;
    hipStream_t st = c->stream;
    const long long ncell = (long long)c->rows * c->cols;
    int rc;
    if ((rc = c->reach_labels.reserve((size_t)ncell, false, st)) || (rc = c->reach_words.reserve(PP_RW_COUNT, false, st))) return rc;
    const unsigned tx = (unsigned)((c->cols + PP_REACH_TILE - 1) / PP_REACH_TILE), ty = (unsigned)((c->rows + PP_REACH_TILE - 1) / PP_REACH_TILE);
    if (ty > 65535u) return fail(PPGPU_ECAPACITY, "reach labels: the grid is too tall for the tile kernel's launch shape");
    const long long hcells = (long long)((c->rows - 1) / PP_REACH_TILE) * c->cols;
    const long long total = hcells + (long long)((c->cols - 1) / PP_REACH_TILE) * c->rows;
    c->reach_set_built = false;
    c->reach_seed_fresh = false;
    HIP_TRY(hipMemsetAsync(c->reach_words.p, 0, PP_RW_COUNT * sizeof(unsigned long long), st));
    if ((rc = reach_timer_begin(c, c->t_reach_labels))) return rc;
    hipLaunchKernelGGL(pp_k_reach_tiles, dim3(tx, ty), dim3(PP_REACH_TILE * PP_REACH_TILE), 0, st, grid_bits(c), c->rows, c->cols, c->wpr, c->reach_labels.p,
                       c->reach_words.p);
    if (total > 0)
        hipLaunchKernelGGL(pp_k_reach_merge, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, grid_bits(c), c->rows, c->cols, c->wpr, c->reach_labels.p,
                           hcells, total, c->reach_words.p);
    hipLaunchKernelGGL(pp_k_reach_flatten, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, c->reach_labels.p, ncell, c->reach_words.p);
    if ((rc = reach_timer_end(c, c->t_reach_labels))) return rc;
    unsigned long long w[PP_RW_COUNT];
    if ((rc = reach_read_words(c, w))) return rc;
    if (w[PP_RW_ERROR]) return fail(PPGPU_ECAPACITY, "reach labels: a union-find loop ran into its iteration cap");
    c->reach_free = w[PP_RW_FREE];
    c->reach_components = w[PP_RW_COMPONENTS];
    c->reach_labels_built = true;
    return PPGPU_OK;
}

// The seed's label in the labels as they stand, and the reach bits and the reach-gap map of that label (rows > 0, a seed is set).
static int reach_seed_ready(ppgpu_ctx* c) {
    int rc = reach_labels_ready(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    if (!c->reach_seed_fresh) {
        // the cell Map::isBlocked puts the seed in (GridWorldMap.cpp:84-93): size_t(x / res), outside when x < 0 or x / res >= cols
        const double x = c->reach_seed_x, y = c->reach_seed_y;
        c->reach_seed_label = PPGPU_REACH_NONE;
        if (!(x < 0 || x / c->res >= (double)c->cols || y < 0 || y / c->res >= (double)c->rows)) {
            const size_t cell = (size_t)(y / c->res) * (size_t)c->cols + (size_t)(x / c->res);
            HIP_TRY(hipMemcpyAsync(&c->reach_seed_label, c->reach_labels.p + cell, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        c->reach_seed_fresh = true;
    }
    if (c->reach_set_built && c->reach_set_label == c->reach_seed_label) return PPGPU_OK;
    const size_t ncell = (size_t)c->rows * c->cols;
    const unsigned ctiles = (unsigned)((c->cols + 255) / 256), rtiles = (unsigned)((c->rows + PP_DIST_TILE - 1) / PP_DIST_TILE);
    if (ctiles > 65535u || rtiles > 65535u) return fail(PPGPU_ECAPACITY, "reach gap: the grid is too large for the map's launch shape");
    DevBuf<uint16_t> v;
    if ((rc = c->reach_bits.reserve((size_t)c->rows * c->wpr, false, st)) || (rc = c->reach_gap.reserve(ncell, false, st)) || (rc = v.reserve(ncell, false, st)))
        return rc;
    c->reach_set_built = false;
    HIP_TRY(hipMemsetAsync(c->reach_words.p + PP_RW_REACHABLE, 0, sizeof(unsigned long long), st));
    if ((rc = reach_timer_begin(c, c->t_reach_gap))) return rc;
    hipLaunchKernelGGL(pp_k_reach_bits, dim3((unsigned)c->rows, ctiles), dim3(256), 0, st, c->reach_labels.p, c->rows, c->cols, c->wpr, c->reach_seed_label,
                       c->reach_bits.p, c->reach_words.p);
    hipLaunchKernelGGL(pp_k_dist_cols<false>, dim3(ctiles, rtiles), dim3(256), 0, st, c->reach_bits.p, c->rows, c->cols, c->wpr, v.p);
    hipLaunchKernelGGL(pp_k_dist_rows<false>, dim3((unsigned)c->rows, ctiles), dim3(256), 0, st, v.p, c->rows, c->cols, c->reach_gap.p);
    if ((rc = reach_timer_end(c, c->t_reach_gap))) return rc;
    unsigned long long w[PP_RW_COUNT];
    if ((rc = reach_read_words(c, w))) return rc;       // (the wait also lets the scratch go with this scope)
    c->reach_cells = c->reach_seed_label == PPGPU_REACH_NONE ? 0ull : w[PP_RW_REACHABLE];
    c->reach_set_label = c->reach_seed_label;
    c->reach_set_built = true;
    return PPGPU_OK;
}

int ppgpu_get_grid_labels(ppgpu_ctx* c, uint32_t* h_out, int64_t capacity) {
    int rc = reach_check_grid(c, "grid labels", h_out, capacity);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = reach_labels_ready(c))) return rc;
    HIP_TRY(hipMemcpyAsync(h_out, c->reach_labels.p, (size_t)c->rows * c->cols * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

int ppgpu_set_reach_seed(ppgpu_ctx* c, double x, double y, ppgpu_reach_info* out) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (x != x || y != y) return fail(PPGPU_EINVAL, "set_reach_seed: the seed is not a number");
    ppgpu_reach_info info{};
    if (c->rows == 0) {                                 // the base Map charts nothing
        info.seed_label = PPGPU_REACH_NONE;
        info.flags = PPGPU_REACH_NO_MAP;
    } else {
        if ((long long)c->rows * c->cols >= 0xFFFFFFFFll) return fail(PPGPU_EINVAL, "set_reach_seed: rows * cols must be below 2^32 - 1 (a label is a 32-bit cell index)");
        HIP_TRY(hipSetDevice(c->device));
    }
    const bool had = c->reach_have_seed;
    const double was_x = c->reach_seed_x, was_y = c->reach_seed_y;
    c->reach_have_seed = true;
    c->reach_seed_x = x; c->reach_seed_y = y;
    c->reach_seed_fresh = false;
    if (c->rows > 0) {
        const int rc = reach_seed_ready(c);
        if (rc) { c->reach_have_seed = had; c->reach_seed_x = was_x; c->reach_seed_y = was_y; return rc; }
        info.free_cells = c->reach_free;
        info.reachable_cells = c->reach_cells;
        info.components = (uint32_t)c->reach_components;
        info.seed_label = c->reach_seed_label;
        info.flags = c->reach_seed_label == PPGPU_REACH_NONE ? PPGPU_REACH_SEED_BLOCKED : 0u;
    }
    if (out) *out = info;
    return PPGPU_OK;
}

int ppgpu_get_grid_reach_gap(ppgpu_ctx* c, uint16_t* h_out, int64_t capacity) {
    int rc = reach_check_grid(c, "grid reach gap", h_out, capacity);
    if (rc) return rc;
    if (!c->reach_have_seed) return fail(PPGPU_ESTATE, "grid reach gap: ppgpu_set_reach_seed must be called first");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = reach_seed_ready(c))) return rc;
    HIP_TRY(hipMemcpyAsync(h_out, c->reach_gap.p, (size_t)c->rows * c->cols * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

int ppgpu_ribbon_reach_host(ppgpu_ctx* c, int32_t n, const double* h_ribbons4, double ribbon_width, ppgpu_ribbon_reach_record* h_records) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (n < 0 || (n > 0 && (!h_ribbons4 || !h_records))) return fail(PPGPU_EINVAL, "ribbon_reach: bad arguments");
    if (ribbon_width != ribbon_width) return fail(PPGPU_EINVAL, "ribbon_reach: the ribbon width is not a number");
    if (!c->reach_have_seed) return fail(PPGPU_ESTATE, "ribbon_reach: ppgpu_set_reach_seed must be called first");
    const bool nomap = c->rows == 0;
    uint32_t lim2 = 0;
    if (!nomap) {
        if ((long long)c->rows * c->cols >= 0xFFFFFFFFll) return fail(PPGPU_EINVAL, "ribbon_reach: rows * cols must be below 2^32 - 1 (a label is a 32-bit cell index)");
        if (ppgpu_keepout_limit2(c->res, ribbon_width + 0.25 * c->res, &lim2)) return fail(PPGPU_EINVAL, "ribbon_reach: ribbon_width + resolution / 4 above 255 cells");
    }
    // len and n of every ribbon, by the rule ppgpu.h states (the base Map has no resolution: one sample per ribbon end)
    std::vector<double> rib((size_t)n * 6);
    for (int32_t i = 0; i < n; i++) {
        const double* q = h_ribbons4 + 4 * (size_t)i;
        for (int j = 0; j < 4; j++)
            if (q[j] != q[j]) return fail(PPGPU_EINVAL, "ribbon_reach: a ribbon coordinate is not a number");
        const double dx = q[2] - q[0], dy = q[3] - q[1];
        const double len = std::sqrt(dx * dx + dy * dy);
        double nd = nomap ? 1.0 : std::ceil(len / (0.5 * c->res));
        if (!(nd >= 1.0)) nd = 1.0;
        if (!(nd < 4194304.0)) return fail(PPGPU_EINVAL, "ribbon_reach: a ribbon has more than 2^22 samples");
        double* o = rib.data() + 6 * (size_t)i;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = len; o[5] = nd;
    }
    if (n == 0) return PPGPU_OK;
    if (!nomap) {
        HIP_TRY(hipSetDevice(c->device));
        const int rc = reach_seed_ready(c);
        if (rc) return rc;
    }
    if (nomap || c->reach_seed_label == PPGPU_REACH_NONE) {          // nothing is judged
        for (int32_t i = 0; i < n; i++) {
            const double len = rib[6 * (size_t)i + 4], nd = rib[6 * (size_t)i + 5];
            ppgpu_ribbon_reach_record r{};
            r.length = len;
            r.pitch = len == 0.0 ? 0.0 : len / nd;
            r.samples = len == 0.0 ? 1u : (uint32_t)nd + 1u;
            r.first_out = r.last_out = -1;
            r.lim2 = lim2;
            r.flags = (nomap ? PPGPU_RB_NO_MAP : PPGPU_RB_NO_SEED) | (len == 0.0 ? PPGPU_RB_DEGENERATE : 0u);
            h_records[i] = r;
        }
        return PPGPU_OK;
    }
    hipStream_t st = c->stream;
    int rc;
    if ((rc = c->reach_ribbons.reserve((size_t)n * 6, false, st)) || (rc = c->reach_records.reserve((size_t)n, false, st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->reach_ribbons.p, rib.data(), rib.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const PPGrid g{nullptr, c->rows, c->cols, c->wpr, c->res, 1.0 / c->res, nullptr};
    if ((rc = reach_timer_begin(c, c->t_reach_ribbons))) return rc;
    hipLaunchKernelGGL(pp_k_reach_ribbons, dim3((unsigned)((n + PP_REACH_WPB - 1) / PP_REACH_WPB)), dim3(PP_REACH_WPB * 64), 0, st, g, c->reach_gap.p, (int)n,
                       c->reach_ribbons.p, lim2, c->reach_records.p);
    if ((rc = reach_timer_end(c, c->t_reach_ribbons))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_records, c->reach_records.p, (size_t)n * sizeof(ppgpu_ribbon_reach_record), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PPGPU_OK;
}

int ppgpu_last_reach_timing(ppgpu_ctx* c, double* ms_labels, double* ms_reach_gap, double* ms_ribbons) {
    if (!c || !ms_labels || !ms_reach_gap || !ms_ribbons) return fail(PPGPU_EINVAL, "last_reach_timing: null argument");
    if (!c->timing) return fail(PPGPU_ESTATE, "last_reach_timing: timing is off (ppgpu_enable_timing)");
    HIP_TRY(hipSetDevice(c->device));
    TraceTimer* tms[3] = {&c->t_reach_labels, &c->t_reach_gap, &c->t_reach_ribbons};
    double* outs[3] = {ms_labels, ms_reach_gap, ms_ribbons};
    for (int i = 0; i < 3; i++) {
        *outs[i] = -1.0;
        if (!tms[i]->timed) continue;
        float ms = 0;
        HIP_TRY(hipEventSynchronize(tms[i]->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, tms[i]->ev[0], tms[i]->ev[1]));
        *outs[i] = ms;
    }
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ distance by water
// What every call of this section refuses on a grid (rows > 0): a path cost must stay below PPGPU_WATER_NONE.
static int water_check_size(const ppgpu_ctx* c, const char* who) {
    if ((unsigned long long)PPGPU_WATER_DIAG * (unsigned long long)c->rows * (unsigned long long)c->cols >= 0xFFFFFFFFull)
        return fail(PPGPU_EINVAL, std::string(who) + ": 17 * rows * cols must be below 2^32 - 1 (a water distance is 32 bits)");
    return PPGPU_OK;
}
// The cell Map::isBlocked puts the seed in (GridWorldMap.cpp:84-93), PPGPU_WATER_NONE outside the grid (rows > 0).
static uint32_t water_seed_cell(const ppgpu_ctx* c) {
    const double x = c->water_seed_x, y = c->water_seed_y;
    if (x < 0 || x / c->res >= (double)c->cols || y < 0 || y / c->res >= (double)c->rows) return PPGPU_WATER_NONE;
    return (uint32_t)((size_t)(y / c->res) * (size_t)c->cols + (size_t)(x / c->res));
}

// The map of the current seed on the effective grid as it stands (rows > 0, a seed is set, the size was checked): nothing when the
// cached map is that of the seed's cell.  Otherwise the fill, the seed, rounds of pp_k_water_round in batches of water_batch launches
// (the rounds' active counts come back in one copy per batch; a round past the last one that had work is a grid of workgroups that
// return), and the totals.  The seed's cell is looked up in the effective bits: a blocked seed leaves the map all NONE.
static int water_ready(ppgpu_ctx* c) {
    hipStream_t st = c->stream;
    uint32_t cell = water_seed_cell(c);
    const size_t ncell = (size_t)c->rows * c->cols;
    if (c->water_built && c->water_map_cell != PPGPU_WATER_NONE && cell == c->water_map_cell) return PPGPU_OK;
    if (cell != PPGPU_WATER_NONE) {                     // blocked in the effective grid?
        uint32_t word = 0;
        const size_t r = cell / (size_t)c->cols, x = cell % (size_t)c->cols;
        HIP_TRY(hipMemcpyAsync(&word, grid_bits(c) + r * c->wpr + (x >> 5), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((word >> (x & 31)) & 1u) cell = PPGPU_WATER_NONE;
    }
    if (c->water_built && cell == c->water_map_cell) return PPGPU_OK;      // (a blocked seed on a map that is all NONE already)
    const unsigned tx = (unsigned)((c->cols + PP_WATER_TILE - 1) / PP_WATER_TILE), ty = (unsigned)((c->rows + PP_WATER_TILE - 1) / PP_WATER_TILE);
    if (ty > 65535u) return fail(PPGPU_ECAPACITY, "water map: the grid is too tall for the tile kernel's launch shape");
    const size_t tiles = (size_t)tx * ty;
    const int batch = c->water_batch;
    int rc;
    if ((rc = c->water_wd.reserve(ncell, false, st)) || (rc = c->water_ctl.reserve(2 * tiles + 64, false, st)) || (rc = c->water_words.reserve(PP_WW_COUNT, false, st)))
        return rc;
    if (!c->water_pinned) {
        GrowthTimer growth;
        HIP_TRY(hipHostMalloc((void**)&c->water_pinned, 64 * sizeof(unsigned), hipHostMallocDefault));
    }
    c->water_built = false;
    TraceTimer& tm = c->t_water_map;
    if ((rc = reach_timer_begin(c, tm))) return rc;
    HIP_TRY(hipMemsetAsync(c->water_wd.p, 0xFF, ncell * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(c->water_words.p, 0, PP_WW_COUNT * sizeof(unsigned long long), st));
    uint32_t* flags = c->water_ctl.p;
    unsigned* counts = (unsigned*)(c->water_ctl.p + 2 * tiles);
    unsigned long long rounds = 0;
    if (cell != PPGPU_WATER_NONE) {
        HIP_TRY(hipMemsetAsync(flags, 0, 2 * tiles * sizeof(uint32_t), st));
        hipLaunchKernelGGL(pp_k_water_seed, dim3(1), dim3(64), 0, st, c->water_wd.p, cell, c->cols, (int)tx, (int)ty, flags);
        const unsigned long long cap = (unsigned long long)ncell + 1ull;          // a round that has work lowers a cell: it cannot take more
        bool done = false;
        for (unsigned long long issued = 0; !done; issued += (unsigned)batch) {
            if (issued >= cap) return fail(PPGPU_ECAPACITY, "water map: the relaxation ran into its cap of rows * cols + 1 rounds");
            HIP_TRY(hipMemsetAsync(counts, 0, (size_t)batch * sizeof(unsigned), st));
            for (int k = 0; k < batch; k++) {
                const unsigned long long round = issued + (unsigned)k;
                hipLaunchKernelGGL(pp_k_water_round, dim3(tx, ty), dim3(PP_WATER_TILE * PP_WATER_TILE), 0, st, grid_bits(c), c->rows, c->cols, c->wpr, c->water_wd.p,
                                   flags + (round & 1ull) * tiles, flags + ((round + 1ull) & 1ull) * tiles, counts + k, c->water_words.p);
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c->water_pinned, counts, (size_t)batch * sizeof(unsigned), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (int k = 0; k < batch && !done; k++) {
                if (c->water_pinned[k] == 0u) done = true;                        // (no tile was dirty: none is in any later round)
                else rounds++;
            }
        }
        hipLaunchKernelGGL(pp_k_water_totals, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, c->water_wd.p, (long long)ncell, c->water_words.p);
    }
    if ((rc = reach_timer_end(c, tm))) return rc;
    unsigned long long w[PP_WW_COUNT];
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w, c->water_words.p, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (w[PP_WW_ERROR]) return fail(PPGPU_ECAPACITY, "water map: a tile's relaxation ran into its cap of sweeps");
    ppgpu_water_info& info = c->water_info;
    info.wet_cells = w[PP_WW_WET];
    info.max_wd = info.wet_cells ? (uint32_t)(w[PP_WW_FARTHEST] >> 32) : 0u;
    info.farthest_cell = info.wet_cells ? ~(uint32_t)w[PP_WW_FARTHEST] : PPGPU_WATER_NONE;
    info.seed_cell = cell;
    info.flags = cell == PPGPU_WATER_NONE ? PPGPU_WATER_SEED_BLOCKED : 0u;
    info.rounds = (uint32_t)rounds;
    info.builds++;
    c->water_map_cell = cell;
    c->water_built = true;
    return PPGPU_OK;
}

int ppgpu_set_water_seed(ppgpu_ctx* c, double x, double y, ppgpu_water_info* out) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (x != x || y != y) return fail(PPGPU_EINVAL, "set_water_seed: the seed is not a number");
    if (c->rows > 0) {
        const int rc = water_check_size(c, "set_water_seed");
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
    }
    const bool had = c->water_have_seed;
    const double was_x = c->water_seed_x, was_y = c->water_seed_y;
    c->water_have_seed = true;
    c->water_seed_x = x; c->water_seed_y = y;
    ppgpu_water_info info{};
    if (c->rows == 0) {                                 // the base Map charts nothing
        info.farthest_cell = info.seed_cell = PPGPU_WATER_NONE;
        info.flags = PPGPU_WATER_NO_MAP;
        info.builds = c->water_info.builds;
    } else {
        const int rc = water_ready(c);
        if (rc) { c->water_have_seed = had; c->water_seed_x = was_x; c->water_seed_y = was_y; return rc; }
        info = c->water_info;
    }
    if (out) *out = info;
    return PPGPU_OK;
}

int ppgpu_get_grid_water(ppgpu_ctx* c, uint32_t* h_out, int64_t capacity) {
    if (!c || !h_out) return fail(PPGPU_EINVAL, "grid water: null argument");
    if (c->rows == 0) return fail(PPGPU_EINVAL, "grid water: no grid is set");
    if (capacity < (int64_t)c->rows * c->cols) return fail(PPGPU_EINVAL, "grid water: capacity below rows * cols");
    int rc = water_check_size(c, "grid water");
    if (rc) return rc;
    if (!c->water_have_seed) return fail(PPGPU_ESTATE, "grid water: ppgpu_set_water_seed must be called first");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = water_ready(c))) return rc;
    HIP_TRY(hipMemcpyAsync(h_out, c->water_wd.p, (size_t)c->rows * c->cols * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

int ppgpu_water_distance_at(ppgpu_ctx* c, int64_t n, const double* h_xy2, double* h_metres, uint32_t* h_wd) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (n < 0 || (n > 0 && !h_xy2)) return fail(PPGPU_EINVAL, "water_distance_at: bad arguments");
    if (!c->water_have_seed) return fail(PPGPU_ESTATE, "water_distance_at: ppgpu_set_water_seed must be called first");
    if (n == 0 || (!h_metres && !h_wd)) return PPGPU_OK;
    if (c->rows == 0) {                             // the base Map charts nothing
        for (int64_t i = 0; i < n; i++) {
            if (h_metres) h_metres[i] = INFINITY;
            if (h_wd) h_wd[i] = PPGPU_WATER_NONE;
        }
        return PPGPU_OK;
    }
    int rc = water_check_size(c, "water_distance_at");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if ((rc = water_ready(c)) || (rc = c->tmp_lengths.reserve((size_t)n * 2, false, st)) || (h_metres && (rc = c->tmp_len_out.reserve((size_t)n, false, st))) ||
        (h_wd && (rc = c->tmp_counts.reserve((size_t)n, false, st))))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->tmp_lengths.p, h_xy2, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    const PPGrid g{nullptr, c->rows, c->cols, c->wpr, c->res, 1.0 / c->res, nullptr};
    hipLaunchKernelGGL(pp_k_water_distance_at, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, c->water_wd.p, (long long)n, c->tmp_lengths.p,
                       h_metres ? c->tmp_len_out.p : nullptr, h_wd ? (unsigned*)c->tmp_counts.p : nullptr);
    HIP_TRY(hipGetLastError());
    if (h_metres) HIP_TRY(hipMemcpyAsync(h_metres, c->tmp_len_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (h_wd) HIP_TRY(hipMemcpyAsync(h_wd, c->tmp_counts.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PPGPU_OK;
}

int ppgpu_ribbon_water_host(ppgpu_ctx* c, int32_t n, const double* h_ribbons4, double ribbon_width, ppgpu_ribbon_water_record* h_records) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (n < 0 || (n > 0 && (!h_ribbons4 || !h_records))) return fail(PPGPU_EINVAL, "ribbon_water: bad arguments");
    if (ribbon_width != ribbon_width) return fail(PPGPU_EINVAL, "ribbon_water: the ribbon width is not a number");
    if (!c->water_have_seed) return fail(PPGPU_ESTATE, "ribbon_water: ppgpu_set_water_seed must be called first");
    const bool nomap = c->rows == 0;
    uint32_t lim2 = 0;
    if (!nomap) {
        const int rc = water_check_size(c, "ribbon_water");
        if (rc) return rc;
        if (ppgpu_keepout_limit2(c->res, ribbon_width + 0.25 * c->res, &lim2)) return fail(PPGPU_EINVAL, "ribbon_water: ribbon_width + resolution / 4 above 255 cells");
        if (lim2 > PPGPU_WATER_MAX_LIM2) return fail(PPGPU_EINVAL, "ribbon_water: lim2 above PPGPU_WATER_MAX_LIM2 (the window of a sample would exceed 67 x 67 cells)");
    }
    // len and n of every ribbon, by the rule ppgpu.h states under "reachable water" (the base Map has no resolution: one sample per ribbon end)
    std::vector<double> rib((size_t)n * 6);
    for (int32_t i = 0; i < n; i++) {
        const double* q = h_ribbons4 + 4 * (size_t)i;
        for (int j = 0; j < 4; j++)
            if (q[j] != q[j]) return fail(PPGPU_EINVAL, "ribbon_water: a ribbon coordinate is not a number");
        const double dx = q[2] - q[0], dy = q[3] - q[1];
        const double len = std::sqrt(dx * dx + dy * dy);
        double nd = nomap ? 1.0 : std::ceil(len / (0.5 * c->res));
        if (!(nd >= 1.0)) nd = 1.0;
        if (!(nd < 4194304.0)) return fail(PPGPU_EINVAL, "ribbon_water: a ribbon has more than 2^22 samples");
        double* o = rib.data() + 6 * (size_t)i;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = len; o[5] = nd;
    }
    if (n == 0) return PPGPU_OK;
    if (!nomap) {
        HIP_TRY(hipSetDevice(c->device));
        const int rc = water_ready(c);
        if (rc) return rc;
    }
    if (nomap || c->water_map_cell == PPGPU_WATER_NONE) {            // nothing is judged
        for (int32_t i = 0; i < n; i++) {
            const double len = rib[6 * (size_t)i + 4], nd = rib[6 * (size_t)i + 5];
            ppgpu_ribbon_water_record r{};
            r.length = len;
            r.pitch = len == 0.0 ? 0.0 : len / nd;
            r.samples = len == 0.0 ? 1u : (uint32_t)nd + 1u;
            r.nearest_sample = r.farthest_sample = -1;
            r.min_ad = r.max_ad = r.start_ad = r.end_ad = PPGPU_WATER_NONE;
            r.lim2 = lim2;
            r.flags = (nomap ? PPGPU_RW_NO_MAP : PPGPU_RW_NO_SEED) | (len == 0.0 ? PPGPU_RW_DEGENERATE : 0u);
            r.nearest_metres = INFINITY;
            h_records[i] = r;
        }
        return PPGPU_OK;
    }
    int reach = 0;                                                   // the largest d with (d - 1)^2 < lim2: |dr|, |dc| of a window cell (0 for lim2 0)
    while ((unsigned)(reach * reach) < lim2) reach++;
    hipStream_t st = c->stream;
    int rc;
    if ((rc = c->water_ribbons.reserve((size_t)n * 6, false, st)) || (rc = c->water_records.reserve((size_t)n, false, st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->water_ribbons.p, rib.data(), rib.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const PPGrid g{nullptr, c->rows, c->cols, c->wpr, c->res, 1.0 / c->res, nullptr};
    if ((rc = reach_timer_begin(c, c->t_water_ribbons))) return rc;
    hipLaunchKernelGGL(pp_k_water_ribbons, dim3((unsigned)((n + PP_WATER_WPB - 1) / PP_WATER_WPB)), dim3(PP_WATER_WPB * 64), 0, st, g, c->water_wd.p, (int)n,
                       c->water_ribbons.p, lim2, reach, c->water_records.p);
    if ((rc = reach_timer_end(c, c->t_water_ribbons))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_records, c->water_records.p, (size_t)n * sizeof(ppgpu_ribbon_water_record), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PPGPU_OK;
}

int ppgpu_last_water_timing(ppgpu_ctx* c, double* ms_map, double* ms_ribbons) {
    if (!c || !ms_map || !ms_ribbons) return fail(PPGPU_EINVAL, "last_water_timing: null argument");
    if (!c->timing) return fail(PPGPU_ESTATE, "last_water_timing: timing is off (ppgpu_enable_timing)");
    HIP_TRY(hipSetDevice(c->device));
    TraceTimer* tms[2] = {&c->t_water_map, &c->t_water_ribbons};
    double* outs[2] = {ms_map, ms_ribbons};
    for (int i = 0; i < 2; i++) {
        *outs[i] = -1.0;
        if (!tms[i]->timed) continue;
        float ms = 0;
        HIP_TRY(hipEventSynchronize(tms[i]->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, tms[i]->ev[0], tms[i]->ev[1]));
        *outs[i] = ms;
    }
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ route by water
// The step map of the water map as it stands (rows > 0, a seed is set, the size was checked): water_ready first, then nothing when the
// step map is that of the water map's build; otherwise one launch of pp_k_water_dirs.  A rebuilt water map has a new build number,
// whatever made it stale (a moved seed, a new grid, a changed keep-out limit).
static int route_dirs_ready(ppgpu_ctx* c) {
    int rc = water_ready(c);
    if (rc) return rc;
    if (c->route_dirs_build == c->water_info.builds) return PPGPU_OK;
    hipStream_t st = c->stream;
    const size_t ncell = (size_t)c->rows * c->cols;
    if ((rc = c->route_dirs.reserve(ncell, false, st))) return rc;
    if ((rc = reach_timer_begin(c, c->t_route_dirs))) return rc;
    hipLaunchKernelGGL(pp_k_water_dirs, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, c->water_wd.p, c->rows, c->cols, (long long)ncell, c->route_dirs.p);
    if ((rc = reach_timer_end(c, c->t_route_dirs))) return rc;
    HIP_TRY(hipGetLastError());
    c->route_dirs_build = c->water_info.builds;
    return PPGPU_OK;
}

int ppgpu_get_grid_water_dirs(ppgpu_ctx* c, uint8_t* h_out, int64_t capacity) {
    if (!c || !h_out) return fail(PPGPU_EINVAL, "grid water dirs: null argument");
    if (c->rows == 0) return fail(PPGPU_EINVAL, "grid water dirs: no grid is set");
    if (capacity < (int64_t)c->rows * c->cols) return fail(PPGPU_EINVAL, "grid water dirs: capacity below rows * cols");
    int rc = water_check_size(c, "grid water dirs");
    if (rc) return rc;
    if (!c->water_have_seed) return fail(PPGPU_ESTATE, "grid water dirs: ppgpu_set_water_seed must be called first");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = route_dirs_ready(c))) return rc;
    HIP_TRY(hipMemcpyAsync(h_out, c->route_dirs.p, (size_t)c->rows * c->cols, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

int ppgpu_water_routes_host(ppgpu_ctx* c, int64_t n, const double* h_xy2, uint32_t lim2, int32_t vertex_stride, ppgpu_water_route_record* h_records,
                            uint32_t* h_vertices) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (n < 0 || (n > 0 && (!h_xy2 || !h_records))) return fail(PPGPU_EINVAL, "water_routes: bad arguments");
    if (vertex_stride < 0 || (vertex_stride > 0 && !h_vertices)) return fail(PPGPU_EINVAL, "water_routes: a vertex stride without a vertices array, or below 0");
    if (lim2 > PPGPU_WATER_MAX_LIM2) return fail(PPGPU_EINVAL, "water_routes: lim2 above PPGPU_WATER_MAX_LIM2 (the window of a point would exceed 67 x 67 cells)");
    for (int64_t i = 0; i < 2 * n; i++)
        if (h_xy2[i] != h_xy2[i]) return fail(PPGPU_EINVAL, "water_routes: a point is not a number");
    if (!c->water_have_seed) return fail(PPGPU_ESTATE, "water_routes: ppgpu_set_water_seed must be called first");
    if (n == 0) return PPGPU_OK;
    const bool nomap = c->rows == 0;
    if (!nomap) {
        int rc = water_check_size(c, "water_routes");
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = water_ready(c))) return rc;
    }
    if (nomap || c->water_map_cell == PPGPU_WATER_NONE) {            // nothing is judged
        ppgpu_water_route_record r{};
        r.point_cell = r.from_cell = r.wd = r.min_gap2 = r.min_gap2_cell = PPGPU_WATER_NONE;
        r.lim2 = lim2;
        r.first_dir = PPGPU_ROUTE_NONE | ((nomap ? PPGPU_WR_NO_MAP : PPGPU_WR_NO_SEED) << 8);
        r.metres = r.narrowest_metres = INFINITY;
        for (int64_t i = 0; i < n; i++) h_records[i] = r;
        return PPGPU_OK;
    }
    int reach = 0;                                                   // as for the ribbon walk: |dr|, |dc| of a window cell (0 for lim2 0)
    while ((unsigned)(reach * reach) < lim2) reach++;
    hipStream_t st = c->stream;
    const size_t stride = (size_t)vertex_stride;
    int rc;
    if ((rc = grid_distance(c)) || (rc = route_dirs_ready(c)) || (rc = c->route_points.reserve((size_t)n * 2, false, st)) ||
        (rc = c->route_records.reserve((size_t)n, false, st)) || (stride && (rc = c->route_vertices.reserve((size_t)n * stride, false, st))))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->route_points.p, h_xy2, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    const PPGrid g{nullptr, c->rows, c->cols, c->wpr, c->res, 1.0 / c->res, nullptr};
    if ((rc = reach_timer_begin(c, c->t_routes))) return rc;
    hipLaunchKernelGGL(pp_k_water_routes, dim3((unsigned)((n + PP_WATER_WPB - 1) / PP_WATER_WPB)), dim3(PP_WATER_WPB * 64), 0, st, g, c->water_wd.p, c->route_dirs.p,
                       c->grid_dist.p, (long long)n, c->route_points.p, c->water_map_cell, lim2, reach, (unsigned)vertex_stride, c->route_records.p,
                       stride ? c->route_vertices.p : nullptr, c->water_words.p);
    if ((rc = reach_timer_end(c, c->t_routes))) return rc;
    HIP_TRY(hipGetLastError());
    // the vertices come back whole and only the slots a route wrote are handed on: the others stay as the caller left them
    std::vector<uint32_t> verts((size_t)n * stride);
    unsigned long long error_word = 0;
    HIP_TRY(hipMemcpyAsync(h_records, c->route_records.p, (size_t)n * sizeof(ppgpu_water_route_record), hipMemcpyDeviceToHost, st));
    if (stride) HIP_TRY(hipMemcpyAsync(verts.data(), c->route_vertices.p, verts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&error_word, c->water_words.p + PP_WW_ERROR, sizeof error_word, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (error_word) return fail(PPGPU_ECAPACITY, "water_routes: a walk ran into its bound of wd / 12 + 2 rounds");
    for (int64_t i = 0; i < n && stride; i++) {
        const size_t count = std::min((size_t)h_records[i].vertices_written, stride);
        std::copy_n(verts.data() + (size_t)i * stride, count, h_vertices + (size_t)i * stride);
    }
    return PPGPU_OK;
}

int ppgpu_last_water_route_timing(ppgpu_ctx* c, double* ms_dirs, double* ms_routes) {
    if (!c || !ms_dirs || !ms_routes) return fail(PPGPU_EINVAL, "last_water_route_timing: null argument");
    if (!c->timing) return fail(PPGPU_ESTATE, "last_water_route_timing: timing is off (ppgpu_enable_timing)");
    HIP_TRY(hipSetDevice(c->device));
    TraceTimer* tms[2] = {&c->t_route_dirs, &c->t_routes};
    double* outs[2] = {ms_dirs, ms_routes};
    for (int i = 0; i < 2; i++) {
        *outs[i] = -1.0;
        if (!tms[i]->timed) continue;
        float ms = 0;
        HIP_TRY(hipEventSynchronize(tms[i]->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, tms[i]->ev[0], tms[i]->ev[1]));
        *outs[i] = ms;
    }
    return PPGPU_OK;
}

int ppgpu_set_obstacles(ppgpu_ctx* c, int32_t model, int32_t n, const double* o7) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (model == PPGPU_OBST_NONE || n == 0) { c->n_obst = 0; c->obst_model = PPGPU_OBST_NONE; return PPGPU_OK; }
    if (model == PPGPU_OBST_GAUSSIAN) return fail(PPGPU_EINVAL, "obstacles: the Gaussian model takes its rows through ppgpu_set_gaussian_obstacles");
    if (model != PPGPU_OBST_BINARY) return fail(PPGPU_EINVAL, "obstacles: unknown model");
    if (n < 0 || !o7) return fail(PPGPU_EINVAL, "obstacles: bad arguments");
    std::vector<PPObst> h((size_t)n);
    for (int i = 0; i < n; i++) {
        const double* o = o7 + 7 * (size_t)i;
        // Obstacle(x, y, heading, speed, time, width, length): Yaw = M_PI_2 - heading
        // (BinaryDynamicObstaclesManager.h:17-19); strict: Width += 2, Length += 2 (.cpp:8-11)
        double yaw = M_PI_2 - o[2];
        h[i].X = o[0]; h[i].Y = o[1];
        h[i].cosYaw = std::cos(yaw); h[i].sinYaw = std::sin(yaw);
        h[i].Speed = o[3]; h[i].Time = o[4];
        h[i].halfW = (o[5] + 2) / 2;
        h[i].halfL = (o[6] + 2) / 2;
        h[i].reach = std::sqrt(h[i].halfW * h[i].halfW + h[i].halfL * h[i].halfL) * (1.0 + 1e-12);
        h[i].pad[0] = h[i].pad[1] = h[i].pad[2] = 0;
    }
    int rc = c->obst.reserve((size_t)n, false, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->obst.p, h.data(), h.size() * sizeof(PPObst), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_obst = n;
    c->obst_model = PPGPU_OBST_BINARY;
    return PPGPU_OK;
}

int ppgpu_set_gaussian_obstacles(ppgpu_ctx* c, int32_t n, const double* rows, int32_t covariance_given) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) { c->n_obst = 0; c->obst_model = PPGPU_OBST_NONE; return PPGPU_OK; }
    if (n < 0 || !rows) return fail(PPGPU_EINVAL, "gaussian obstacles: bad arguments");
    static_assert(sizeof(PPGauss) == sizeof(PPObst), "both obstacle records share one buffer and the culling fields");
    std::vector<PPGauss> h((size_t)n);
    const int stride = covariance_given ? 9 : 5;
    for (int i = 0; i < n; i++) {
        const double* o = rows + (size_t)stride * i;
        // Obstacle(x, y, heading, speed, time[, covariance]): Yaw = M_PI_2 - heading, default covariance
        // [[30,10],[10,30]] (GaussianDynamicObstaclesManager.h:23-29)
        const double yaw = M_PI_2 - o[2];
        double c00 = 30, c01 = 10, c10 = 10, c11 = 30;
        if (covariance_given) { c00 = o[5]; c01 = o[6]; c10 = o[7]; c11 = o[8]; }
        // pdf(): covariance.inverse() and covariance.determinant() of a fixed 2x2 (Eigen's closed forms), norm = 1/2pi/sqrt(det)
        const double det = c00 * c11 - c10 * c01;
        const double invdet = 1.0 / det;
        PPGauss& g = h[i];
        g.X = o[0]; g.Y = o[1]; g.cosYaw = std::cos(yaw); g.sinYaw = std::sin(yaw); g.Speed = o[3]; g.Time = o[4];
        g.i00 = c11 * invdet; g.i10 = -c10 * invdet; g.i01 = -c01 * invdet; g.i11 = c00 * invdet;
        const double twoPi = 2 * M_PI;
        g.norm = 1.0 / twoPi / std::sqrt(det);
        // culling radius: pdf <= |norm| exp(-lmin d^2 / 2), lmin = smallest eigenvalue of the symmetric part of the inverse;
        // beyond reach it is below 1e-13 (collisionExists floors its SUM at 1e-5).  Not positive definite: never culled.
        const double sa = g.i00, sc = g.i11, sb = 0.5 * (g.i01 + g.i10);
        const double lmin = 0.5 * (sa + sc) - std::sqrt(0.25 * (sa - sc) * (sa - sc) + sb * sb);
        if (!(det > 0) || !(lmin > 0) || !std::isfinite(g.norm)) g.reach = 1e300;
        else if (!(std::fabs(g.norm) > 1e-13)) g.reach = 0;
        else g.reach = std::sqrt(2.0 * std::log(std::fabs(g.norm) / 1e-13) / lmin) * (1.0 + 1e-9);
    }
    int rc = c->obst.reserve((size_t)n, false, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->obst.p, h.data(), h.size() * sizeof(PPGauss), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_obst = n;
    c->obst_model = PPGPU_OBST_GAUSSIAN;
    return PPGPU_OK;
}

int ppgpu_set_vertices(ppgpu_ctx* c, int32_t n, const ppgpu_vertex* hv, int32_t n_ribbons, const double* hr) {
    int rc = require_cfg(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (n <= 0 || !hv || n_ribbons < 0 || (n_ribbons > 0 && !hr)) return fail(PPGPU_EINVAL, "vertices: bad arguments");
    if (n >= (1 << 24)) return fail(PPGPU_ECAPACITY, "vertices: at most 2^24-1 open vertices");
    int maxr = 0;
    if ((rc = check_open_vertices(c, "vertices", n, hv, n_ribbons, &maxr))) return rc;
    if ((rc = c->verts.reserve((size_t)n, false, c->stream))) return rc;
    if ((rc = c->ribbons.reserve((size_t)(n_ribbons > 0 ? n_ribbons : 1) * 4, false, c->stream))) return rc;
    if ((rc = c->tgrid.reserve((size_t)n * c->ng, false, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(c->verts.p, hv, (size_t)n * sizeof(ppgpu_vertex), hipMemcpyHostToDevice, c->stream));
    if (n_ribbons > 0)
        HIP_TRY(hipMemcpyAsync(c->ribbons.p, hr, (size_t)n_ribbons * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pp_k_time_grid, dim3((unsigned)n), dim3(64), 0, c->stream, c->verts.p, n, c->cfg.start_state_time,
                       c->cfg.collision_checking_increment, c->cfg.max_speed, c->ng, c->tgrid.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // the host arrays may go away after return
    c->nverts = n; c->nribbons = n_ribbons; c->max_vertex_ribbons = maxr;
    c->arc_stops_stale = true;
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ samples
int ppgpu_set_samples(ppgpu_ctx* c, int64_t n, const double* hx, const double* hy, const double* hh) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (n < 0 || (n > 0 && (!hx || !hy || !hh))) return fail(PPGPU_EINVAL, "samples: bad arguments");
    if (n >= (1ll << 32)) return fail(PPGPU_ECAPACITY, "samples: at most 2^32-1");
    int rc;
    size_t need = (size_t)(n > 0 ? n : 1);
    if ((rc = c->sx.reserve(need, false, c->stream)) || (rc = c->sy.reserve(need, false, c->stream)) ||
        (rc = c->sh.reserve(need, false, c->stream)))
        return rc;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(c->sx.p, hx, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sy.p, hy, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sh.p, hh, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->n_samples = n;
    c->n_extra = 0;
    return PPGPU_OK;
}

int ppgpu_set_extra_targets(ppgpu_ctx* c, int32_t n, const double* hx, const double* hy, const double* hh, int64_t* first_index) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (n < 0 || (n > 0 && (!hx || !hy || !hh))) return fail(PPGPU_EINVAL, "extra_targets: bad arguments");
    int rc;
    size_t need = (size_t)(c->n_samples + n > 0 ? c->n_samples + n : 1);
    if ((rc = c->sx.reserve(need, true, c->stream)) || (rc = c->sy.reserve(need, true, c->stream)) ||
        (rc = c->sh.reserve(need, true, c->stream)))
        return rc;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(c->sx.p + c->n_samples, hx, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sy.p + c->n_samples, hy, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sh.p + c->n_samples, hh, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->n_extra = n;
    if (first_index) *first_index = c->n_samples;
    return PPGPU_OK;
}

int ppgpu_get_samples(ppgpu_ctx* c, int64_t first, int64_t n, double* out5) {
    int rc = require_cfg(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (first < 0 || n < 0 || first + n > c->n_samples || (n > 0 && !out5)) return fail(PPGPU_EINVAL, "get_samples: range");
    if (n == 0) return PPGPU_OK;
    std::vector<double> x((size_t)n), y((size_t)n), h((size_t)n);
    HIP_TRY(hipMemcpyAsync(x.data(), c->sx.p + first, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(y.data(), c->sy.p + first, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h.data(), c->sh.p + first, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; i++) {
        out5[5 * i] = x[(size_t)i]; out5[5 * i + 1] = y[(size_t)i]; out5[5 * i + 2] = h[(size_t)i];
        // speed is not stored per sample: expand() overwrites it with maxSpeed before any use
        // (SamplingBasedPlanner.cpp:113), so the store keeps x, y, heading only.
        out5[5 * i + 3] = c->cfg.max_speed;
        out5[5 * i + 4] = 0;   // State(..., 0) (StateGenerator.cpp:16-20)
    }
    return PPGPU_OK;
}

int64_t ppgpu_num_samples(ppgpu_ctx* c) { return c ? c->n_samples : 0; }

int ppgpu_sampler_init(ppgpu_ctx* c, const double* b6, uint64_t seed, int32_t n_ribbons, const double* hr) {
    int rc = require_cfg(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!b6) return fail(PPGPU_EINVAL, "sampler: bounds are null");
    if (n_ribbons > 0 && !hr) return fail(PPGPU_EINVAL, "sampler: ribbons are null");
    if (n_ribbons > 1024) return fail(PPGPU_ECAPACITY, "sampler: more than 1024 ribbons");
    PPSamplerState& s = c->sampler;
    for (int i = 0; i < 6; i++) s.b[i] = b6[i];
    // std::linear_congruential_engine::seed: c == 0 and s mod m == 0 -> 1
    unsigned long long x = seed % 2147483647ull;
    s.seed = (unsigned)(x == 0 ? 1 : x);
    s.on_ribbons = n_ribbons >= 0 ? 1 : 0;   // the ribbon constructor sets m_SampleOnRibbons even for an empty manager
    s.n_ribbons = n_ribbons > 0 ? n_ribbons : 0;
    const int kPosGroups = 1024;
    if (!c->samp_pos.p) c->samp_group = -1;
    if ((rc = c->samp_pos.reserve((size_t)8 * kPosGroups, false, c->stream))) return rc;
    c->samp_group = (c->samp_group + 1) % kPosGroups;
    if (c->samp_group == 0)      // (in stream order after everything that used the old groups: no host wait)
        HIP_TRY(hipMemsetAsync(c->samp_pos.p, 0, (size_t)8 * kPosGroups * sizeof(unsigned long long), c->stream));
    s.d_pos = c->samp_pos.p + (size_t)8 * c->samp_group;
    s.initialised = 1;
    if (n_ribbons > 0) {
        // the generator of every iteration of a plan() call is built from the same ribbon manager (AStarPlanner.cpp:34): the table is
        // uploaded (one host round trip) only when it differs from the one already on the device
        const size_t nd = (size_t)n_ribbons * 4;
        if (c->samp_ribbons_host.size() != nd || std::memcmp(c->samp_ribbons_host.data(), hr, nd * sizeof(double)) != 0) {
            if ((rc = c->samp_ribbons.reserve(nd, false, c->stream))) return rc;
            c->samp_ribbons_host.clear();             // not valid until the copy below is known to have happened
            HIP_TRY(hipMemcpyAsync(c->samp_ribbons.p, hr, nd * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->samp_ribbons_host.assign(hr, hr + nd);
        }
    }
    c->n_samples = 0;
    c->n_extra = 0;
    return PPGPU_OK;
}

// Steps 1-3 of the sampler: which stream slots do the next n samples start at?  Leaves qpos[0..n)
// (relative slots) in c->s_u32a, the projection bits in c->s_bytes and the relative slot of sample n
// (= where the stream resumes) in *d_end (device).  Without ribbons the layout is fixed (4 slots per sample).
static int sampler_chain(ppgpu_ctx* c, long long n, long long& nq, int& nblk_q, unsigned long long** d_end, bool skip = false) {
    PPSamplerState& s = c->sampler;
    hipStream_t st = c->stream;
    int rc;
    nq = s.on_ribbons ? (6 * n + 8) : n;   // worst case every sample is projected: 6 slots per sample
    nblk_q = (int)((nq + PP_SCAN_TILE - 1) / PP_SCAN_TILE);
    if (nblk_q > PP_SCAN_TILE) return fail(PPGPU_ECAPACITY, "sampler: batch too large for the two-level scan (max ~690k samples per call)");
    if ((rc = c->s_bytes.reserve((size_t)nq + 64 + (size_t)n + 64, false, st))) return rc;   // projection / visited bits, then the keep flags
    if ((rc = c->s_u64.reserve((size_t)nblk_q + 64, false, st))) return rc;
    if ((rc = c->s_u32a.reserve((size_t)nq + 64, false, st))) return rc;
    {   // per-tile counts of the chain scan, later (ppgpu_sampler_add) per-workgroup counts of the compaction: sized for both now,
        // so that nothing is re-allocated while launches that use it are in flight
        const size_t nblk_n = (size_t)((n + 255) / 256);
        if ((rc = c->s_u32b.reserve(((size_t)nblk_q > nblk_n ? (size_t)nblk_q : nblk_n) + 64, false, st))) return rc;
    }
    *d_end = c->s_u64.p + nblk_q + 8;
    if (!s.on_ribbons) { HIP_TRY(hipMemsetAsync(c->s_u64.p + nblk_q + 8, 0, 16 * sizeof(unsigned long long), st)); return PPGPU_OK; }
    unsigned char* proj = c->s_bytes.p;
    unsigned* tilefn = reinterpret_cast<unsigned*>(c->s_u64.p);      // one 18-bit function per tile (the first nblk_q words' worth of s_u64)
    // 1. proj[q] for every slot in range (LCG jump-ahead) + 2a. the function of every tile of PP_SCAN_TILE slots: the chain
    //    q -> q + 5 + proj[q] as a scan over compositions of functions on its six states (also zeroes the end slot / total of this call)
    hipLaunchKernelGGL(pp_k_proj_reduce, dim3(nblk_q), dim3(256), 0, st, s.seed, s.d_pos, nq, proj, tilefn, c->s_u64.p + nblk_q + 8);
    // 2b. visited[q] + 3a. visited slots per tile
    hipLaunchKernelGGL(pp_k_chain_apply_count, dim3(nblk_q), dim3(256), 0, st, proj, nq, tilefn, c->s_u32b.p);
    // 3b. rank the visited slots: slot of each sample, and of sample n
    hipLaunchKernelGGL(pp_k_chain_positions_scan, dim3(nblk_q), dim3(256), 0, st, proj, nq, c->s_u32b.p, n, c->s_u32a.p, *d_end,
                       skip ? const_cast<unsigned long long*>(s.d_pos) : (unsigned long long*)nullptr);
    HIP_TRY(hipGetLastError());
    return PPGPU_OK;
}

int ppgpu_sampler_skip(ppgpu_ctx* c, int64_t n_attempts) {
    int rc = require_cfg(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->sampler.initialised) return fail(PPGPU_ESTATE, "ppgpu_sampler_init must be called first");
    if (n_attempts < 0) return fail(PPGPU_EINVAL, "sampler: negative count");
    PPSamplerState& s = c->sampler;
    // Launches only: the position after the skip is data-dependent (which samples were projected onto a ribbon), but it stays on the
    // device (samp_pos); a chain that does not reach the end of its batch raises samp_pos[1], which the next ppgpu_sampler_add reports.
    long long left = n_attempts;
    while (left > 0) {
        long long n = left < 524288 ? left : 524288;
        long long nq = 0; int nblk_q = 0; unsigned long long* d_end = nullptr;
        if (s.on_ribbons) {
            // three launches; the last of them (pp_k_chain_positions_scan) advances the position itself
            if ((rc = sampler_chain(c, n, nq, nblk_q, &d_end, true))) return rc;
        } else {
            hipLaunchKernelGGL(pp_k_sampler_advance, dim3(1), dim3(1), 0, c->stream, const_cast<unsigned long long*>(s.d_pos), d_end, (const unsigned long long*)nullptr,
                               4ull * (unsigned long long)n, 0);
            HIP_TRY(hipGetLastError());
        }
        left -= n;
    }
    return PPGPU_OK;
}

int ppgpu_sampler_add(ppgpu_ctx* c, int64_t n_attempts, int64_t* n_total_out) {
    int rc = require_cfg(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->sampler.initialised) return fail(PPGPU_ESTATE, "ppgpu_sampler_init must be called first");
    if (n_attempts < 0) return fail(PPGPU_EINVAL, "sampler: negative count");
    if (n_attempts == 0) { if (n_total_out) *n_total_out = c->n_samples; return PPGPU_OK; }
    if (n_attempts > 524288) return fail(PPGPU_ECAPACITY, "sampler: at most 524288 attempts per call");
    const long long n = n_attempts;
    PPSamplerState& s = c->sampler;
    hipStream_t st = c->stream;
    size_t need_samples = (size_t)(c->n_samples + n);
    if ((rc = c->sx.reserve(need_samples, true, st)) || (rc = c->sy.reserve(need_samples, true, st)) ||
        (rc = c->sh.reserve(need_samples, true, st)))
        return rc;
    if ((rc = c->s_cand.reserve((size_t)n * 3, false, st))) return rc;
    long long nq; int nblk_q; unsigned long long* d_end;
    if ((rc = sampler_chain(c, n, nq, nblk_q, &d_end))) return rc;
    const int nblk_n = (int)((n + 255) / 256);
    unsigned char* proj = c->s_bytes.p;
    unsigned* qpos = c->s_u32a.p;
    unsigned* blk32 = c->s_u32b.p;
    // 4. generate the n candidate states (thread per sample) + 5a. SamplingBasedPlanner::addSamples' map filter
    PPGrid g{grid_bits(c), c->rows, c->cols, c->wpr, c->res, c->res > 0 ? 1.0 / c->res : 0.0, nullptr};
    unsigned char* keep = c->s_bytes.p + (size_t)nq + 64;          // (the projection bits are still being read by this launch)
    hipLaunchKernelGGL(pp_k_generate_keep, dim3((unsigned)nblk_n), dim3(256), 0, st, s, s.on_ribbons ? qpos : nullptr, s.on_ribbons ? proj : nullptr,
                       c->samp_ribbons.p, n, c->s_cand.p, g, keep, blk32);
    // 5b. order-preserving compaction into the store
    unsigned long long* d_total = d_end + 8;
    hipLaunchKernelGGL(pp_k_compact_scan, dim3((unsigned)nblk_n), dim3(256), 0, st, keep, n, blk32, c->s_cand.p, c->sx.p, c->sy.p,
                       c->sh.p, c->n_samples, d_total);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pp_k_sampler_advance, dim3(1), dim3(1), 0, st, const_cast<unsigned long long*>(s.d_pos), d_end, d_total, 4ull * (unsigned long long)n, s.on_ribbons);
    HIP_TRY(hipGetLastError());
    // {chain error, kept, slots consumed} come back in one copy through pinned memory (a copy to pageable memory waits for the
    // stream by itself); the position itself stays on the device
    volatile unsigned long long* h2 = c->pinned_counts;
    h2[0] = 0; h2[1] = 0; h2[2] = 0;
    HIP_TRY(hipMemcpyAsync((void*)&h2[0], s.d_pos + 1, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h2[0] != 0) return fail(PPGPU_EHIP, "sampler: chain scan did not reach the end of the batch (this call or a ppgpu_sampler_skip before it)");
    c->n_samples += (long long)h2[1];
    c->n_extra = 0;                        // the appended samples overwrote any explicit targets
    if (n_total_out) *n_total_out = c->n_samples;
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ edge generation
static void fill_params(ppgpu_ctx* c, PPParams& p) {
    const ppgpu_config& g = c->cfg;
    p.max_speed = g.max_speed;
    p.slow_speed = g.slow_speed <= 0 ? g.max_speed : g.slow_speed;   // PlannerConfig::slowSpeed()
    p.rho = g.turning_radius; p.rho_cov = g.coverage_turning_radius;
    p.horizon = g.time_horizon; p.tmin = g.time_minimum; p.inc_d = g.collision_checking_increment;
    p.sst = g.start_state_time; p.ribw = g.ribbon_width;
    p.inv_inc_d = 1.0 / p.inc_d;
    p.cpf = g.collision_penalty_factor; p.tpf = g.time_penalty_factor;
    p.heuristic = g.heuristic; p.tsp_k = g.tsp_k; p.h_rho = g.heuristic_turning_radius;
    p.fuse_h = 0;
    p.lane_split = 0; p.defer_h = 0; p.defer_list = nullptr; p.quiet_finish = 0; p.live_list = nullptr; p.cover_state = nullptr; p.hw_list = nullptr; p.words = nullptr; p.reset_words = 0;
    p.share_head = nullptr; p.share_of = nullptr; p.sweep_list = nullptr; p.approach_list = 0;
    p.arc_stop = nullptr; p.stop_of = nullptr; p.stop_list = nullptr;
    p.grid = PPGrid{grid_bits(c), c->rows, c->cols, c->wpr, c->res, c->res > 0 ? 1.0 / c->res : 0.0, c->rows > 0 ? c->grid_clear.p : nullptr};
    p.obst = c->obst.p; p.n_obst = c->n_obst; p.obst_model = c->obst_model;
    p.verts = c->verts.p; p.ribbons = c->ribbons.p; p.tgrid = c->tgrid.p; p.ng = c->ng; p.nverts = c->nverts;
    p.sx = c->sx.p; p.sy = c->sy.p; p.sh = c->sh.p; p.n_samples = c->n_samples + c->n_extra;
}

int ppgpu_dubins_lengths(ppgpu_ctx* c, int32_t v0, int32_t nv, double* d_lengths) {
    int rc = require_world(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (v0 < 0 || nv <= 0 || v0 + nv > c->nverts || !d_lengths) return fail(PPGPU_EINVAL, "dubins_lengths: vertex range");
    if (nv > 65535) return fail(PPGPU_ECAPACITY, "dubins_lengths: at most 65535 vertices per call");
    const long long ns = c->n_samples;
    if (ns <= 0) return fail(PPGPU_ESTATE, "dubins_lengths: the sample store is empty");
    hipLaunchKernelGGL(pp_k_dubins_lengths, dim3((unsigned)((ns + 255) / 256), (unsigned)nv), dim3(256), 0, c->stream, c->verts.p,
                       v0, c->sx.p, c->sy.p, c->sh.p, ns, c->cfg.turning_radius, c->cfg.coverage_turning_radius,
                       c->cfg.collision_checking_increment, d_lengths);
    HIP_TRY(hipGetLastError());
    return PPGPU_OK;
}

int ppgpu_select_nearest(ppgpu_ctx* c, int32_t v0, int32_t nv, int32_t k, int32_t* h_idx, double* h_len) {
    int rc = require_world(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (k <= 0 || !h_idx || !h_len) return fail(PPGPU_EINVAL, "select_nearest: bad arguments");
    const long long ns = c->n_samples;
    if ((rc = c->expand.lengths.reserve((size_t)nv * ns * 2, false, c->stream))) return rc;
    if ((rc = ppgpu_dubins_lengths(c, v0, nv, c->expand.lengths.p))) return rc;
    size_t nout = (size_t)nv * 2 * k;
    if ((rc = c->tmp_idx.reserve(nout, false, c->stream)) || (rc = c->tmp_len_out.reserve(nout, false, c->stream))) return rc;
    hipLaunchKernelGGL(pp_k_select_nearest, dim3((unsigned)(nv * 2)), dim3(256), 0, c->stream, c->expand.lengths.p, ns, k,
                       c->tmp_idx.p, c->tmp_len_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_idx, c->tmp_idx.p, nout * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_len, c->tmp_len_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PPGPU_OK;
}

// The loops of SamplingBasedPlanner::expand a configuration asks for: both speeds (SamplingBasedPlanner.cpp:57-59), both radii (:60-63).
struct ExpandLoops { int two_speeds, two_radii; };
static ExpandLoops expand_loops(const ppgpu_config& g) {
    const double slow = g.slow_speed <= 0 ? g.max_speed : g.slow_speed;     // PlannerConfig::slowSpeed()
    return {slow != g.max_speed ? 1 : 0, g.coverage_turning_radius != g.turning_radius ? 1 : 0};
}

// The k winners of every (vertex, radius) of vertices [0, nv) in the reference's push order -> c->expand.idx: the six kernels of
// pp_k_expand.h on one argument block.  Asynchronous; *c->expand.fallbacks.p counts lists that kept ascending length.
static int launch_expand_order(ppgpu_ctx* c, int nv, int k, bool zero_fallbacks = true) {
    const long long ns = c->n_samples;
    ExpandWork& w = c->expand;
    hipStream_t st = c->stream;
    int rc;
    if ((rc = w.reserve((size_t)nv, ns, k, st))) return rc;
    if (zero_fallbacks) HIP_TRY(hipMemsetAsync(w.fallbacks.p, 0, sizeof(unsigned), st));      // (ppgpu_expand_host: its unpack kernel does it)
    const ppgpu_config& g = c->cfg;
    PPExpandArgs a{};
    a.verts = c->verts.p; a.sx = c->sx.p; a.sy = c->sy.p; a.sh = c->sh.p; a.ns = ns;
    a.k = k; a.two_radii = expand_loops(g).two_radii;
    a.rho = g.turning_radius; a.rho_cov = g.coverage_turning_radius; a.inc_d = g.collision_checking_increment;
    a.max_speed = g.max_speed; a.tpf = g.time_penalty_factor;
    a.probe_min = w.probe_min.p; a.near_idx = w.near_idx.p; a.near_count = w.near_count.p; a.lengths = w.lengths.p;
    a.groupmin = w.groupmin.p; a.groupcnt = w.groupcnt.p; a.groups_row = (int)ExpandWork::groups_row(ns);
    a.bound = w.bound.p; a.cand_count = w.count.p;
    a.g_key = w.key.p; a.g_val = w.val.p; a.g_len = w.len.p; a.g_cap = ExpandWork::list_cap(ns);
    a.out_idx = w.idx.p; a.fallbacks = w.fallbacks.p;
    const dim3 per_sample((unsigned)((ns + 255) / 256), (unsigned)nv), per_list((unsigned)(nv * 2));
    hipLaunchKernelGGL(pp_k_expand_probe, dim3((unsigned)(PP_PROBE / 256), (unsigned)nv), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pp_k_expand_near, dim3((unsigned)((ns + 256 * PP_NEAR_PER - 1) / (256 * PP_NEAR_PER)), (unsigned)nv), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pp_k_near_lengths, per_sample, dim3(256), 0, st, a);
    hipLaunchKernelGGL(pp_k_expand_bound, per_list, dim3(256), 0, st, a);
    hipLaunchKernelGGL(pp_k_expand_candidates, per_sample, dim3(256), 0, st, a);
    hipLaunchKernelGGL(pp_k_expand_order, per_list, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return PPGPU_OK;
}

int ppgpu_expand_order(ppgpu_ctx* c, int32_t v0, int32_t nv, int32_t k, int32_t* h_idx, uint32_t* h_fallbacks) {
    int rc = require_world(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (k <= 0 || !h_idx || v0 != 0 || nv <= 0 || nv > c->nverts) return fail(PPGPU_EINVAL, "expand_order: bad arguments (v0 must be 0)");
    if (nv > 65535) return fail(PPGPU_ECAPACITY, "expand_order: at most 65535 vertices per call");
    if (c->n_samples <= 0) return fail(PPGPU_ESTATE, "expand_order: the sample store is empty");
    const size_t nout = (size_t)nv * 2 * k;
    if ((rc = launch_expand_order(c, nv, k))) return rc;
    unsigned fb = 0;
    HIP_TRY(hipMemcpyAsync(h_idx, c->expand.idx.p, nout * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&fb, c->expand.fallbacks.p, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->order_fallbacks += fb;
    if (h_fallbacks) *h_fallbacks = fb;
    return PPGPU_OK;
}

uint64_t ppgpu_order_fallbacks(ppgpu_ctx* c) { return c ? c->order_fallbacks : 0; }

// ------------------------------------------------------------------------------ edge costing
int64_t ppgpu_dense_edge_count(int32_t nv, int64_t ns, uint32_t cfg_mask) {
    return (int64_t)nv * ns * (int64_t)__builtin_popcount(cfg_mask & 0xFu);
}

// Grid of a cover sweep: as many workgroups as the device keeps resident (its waves pull edges from the queues), or fewer
// when the launch has fewer edges than that.
static unsigned resident_grid(ppgpu_ctx* c, bool gaussian, long long n_edges) {
    int& resident = c->resident[gaussian ? 1 : 0];
    if (resident == 0) {
        const void* kernel = gaussian ? (const void*)pp_k_cover_sweep_gaussian : (const void*)pp_k_cover_sweep;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, PP_WPB * 64, 0) != hipSuccess || per_cu <= 0) per_cu = 2;
        resident = per_cu * (c->n_cu > 0 ? c->n_cu : 256);
    }
    const long long need = (n_edges + PP_WPB - 1) / PP_WPB;
    return (unsigned)(need < resident ? need : resident);
}

// "Cost this list of n edges": packed descriptors on the device (d_edges), or wrapper edges on the device (d_wedges).  Records go
// to d_out, child ribbon lists to d_child at `stride` ribbons per edge (NULL: the launch keeps them in a scratch of its own).
static PPParams list_params(ppgpu_ctx* c, long long n, const unsigned long long* d_edges, const ppgpu_wrapper_edge* d_wedges,
                            ppgpu_edge_result* d_out, double* d_child, int stride) {
    PPParams p;
    fill_params(c, p);
    p.edges = d_edges; p.wedges = d_wedges;
    p.v0 = 0; p.nv = 0; p.s0 = 0; p.ns = 1; p.cfg_mask = 0; p.per = 1;
    p.n_edges = n;
    p.out = d_out; p.child = d_child; p.stride = stride;
    return p;
}

// One costing launch.  How it runs is decided once (cost_modes), before anything is reserved or launched; once launch_cost has
// returned, this is also what the code that runs next (launch_trace) may rely on.
struct CostLaunch {
    PPParams p;          // the whole list as it is launched: n_edges = all of it, e_base = 0, the workspace pointers wired
                         // (cost_workspace), child / stride = the launch's own scratch where the caller gave none
    bool gaussian;       // the Gaussian obstacle model: its own planner and sweeps, two more track arrays, no lane kernels
    bool prepasses;      // a large launch: pp_k_approach_events runs (a planner round trip of a few hundred edges is latency-bound) ...
    bool skip_chunks;    // ... and so does the chunk-skip planner
    bool packed;         // the cover sweep takes the packed list of the edges it still has to visit (live_list)
    bool lane_finish;    // phase C of those edges: one lane per edge (pp_k_cover_finish)
    bool fuse_h;         // the cover sweep computes h itself
    bool defer_h;        // ... but leaves the TSP enumerations to pp_k_heuristic_lanes
    bool quiet_finish, lane_split;   // what the handle's PPGPU_QUIET_FINISH / PPGPU_LANE_SPLIT switches allow, on large launches
    bool forked;         // pp_k_heuristic_listed runs on the side stream
    bool share;          // shared sweeps: one member of each class of edges with the same sweep is swept, the others take its results (pp_k_solve.h)
    bool share_child;    // ... and its child ribbons, where the caller asked for them
    bool sweep_list;     // ... and the skip planner and the pose sweep walk the packed list of the edges that are swept (pp_k_mark_sweeps)
    bool tracks;         // shared tracks: edges that a blocked cell stops on their class's first arc take their track from one of them (pp_k_solve.h)
    int nch, ngp;        // 64-step chunks per edge, and the steps they hold
    long long slice;     // edges per workspace slice (>= p.n_edges: one piece, the setup records of the whole list are still there)
};

static void cost_modes(const ppgpu_ctx* c, CostLaunch& m) {
    const PPParams& p = m.p;
    const long long total = p.n_edges;
    m.gaussian = p.n_obst > 0 && p.obst_model == PPGPU_OBST_GAUSSIAN;
    m.nch = (p.ng + PP_WAVE - 1) / PP_WAVE;
    if (m.nch < 1) m.nch = 1;
    m.ngp = m.nch * PP_WAVE;
    const size_t per_edge = sizeof(PPEdgeSetup) + (size_t)m.ngp * sizeof(unsigned short) +
                            (size_t)m.nch * (sizeof(unsigned long long) + sizeof(unsigned)) + sizeof(PPTrackSummary) +
                            (m.gaussian ? (size_t)(m.ngp + m.nch) * sizeof(double) : 0);
    m.slice = (long long)(c->slice_bytes / per_edge);
    if (m.slice < PP_WPB) m.slice = PP_WPB;
    if (m.slice > total) m.slice = total;
    // both prepasses pay for themselves on large launches only; chunk skipping also needs the clearance map (or no grid at all)
    // and solved curves (a given curve may start late or end early)
    m.prepasses = total >= c->prepass_min_edges;
    m.skip_chunks = m.prepasses && !p.wedges && (c->rows == 0 || c->grid_clear.p) && p.ng >= PP_WAVE;
    // fuse_h / defer_h: decided here and nowhere else; every kernel that routes a child list reads them through pp_h_route (pp_device.h)
    const bool dubinsH = p.heuristic == PPGPU_H_TSP_DUBINS_ALL || p.heuristic == PPGPU_H_TSP_DUBINS_K;
    m.fuse_h = PP_FUSE_HEUR && !dubinsH && !m.gaussian;
    m.defer_h = m.fuse_h && m.prepasses && c->lane_heuristic && total < (1ll << 32) &&
                (p.heuristic == PPGPU_H_TSP_POINT_ALL || p.heuristic == PPGPU_H_TSP_POINT_K);
    m.quiet_finish = m.prepasses && c->quiet_finish;
    m.lane_split = m.prepasses && c->lane_split && !m.gaussian;
    m.packed = m.prepasses && total < (1ll << 32);
#if defined(PP_DBG_COUNTS)
    const bool laneFinishBuilt = false;     // (those builds keep every edge with its wave: pp_cover_sweep_edge)
#else
    const bool laneFinishBuilt = true;
#endif
    m.lane_finish = laneFinishBuilt && m.packed && c->lane_finish && !m.gaussian;
    m.forked = m.lane_finish && m.fuse_h && p.heuristic != PPGPU_H_MAX_DISTANCE;
    // shared sweeps: large launches of solved curves (a given curve is its caller's); positions and class keys are 32-bit words, and the
    // table of heads, a 128-byte line per class, stays within 256 MB (262 144 open vertices: beyond that every edge is swept itself)
    m.share = m.prepasses && m.packed && !p.wedges && c->share_sweeps && (long long)p.nverts * PP_SHARE_KEYS * PP_SHARE_STRIDE <= (1ll << 26);
    m.share_child = m.share && p.child != nullptr;
    // the sweep list: exactly where sweeps are shared.  Any other launch has a handful of unsweepable edges at most, and the kernel
    // that builds the list would cost it more than they do
    m.sweep_list = m.share && c->use_sweep_list;
    // shared tracks: where there is a list to put the members behind, a grid to stop on, and room for the stop classes' half of the
    // table of heads.  The Gaussian model has its own track arrays and forms no stop classes
    m.tracks = m.sweep_list && c->share_tracks && !m.gaussian && c->rows > 0 && (long long)p.nverts * 2 * PP_SHARE_KEYS * PP_SHARE_STRIDE <= (1ll << 26);
}

// Reserves the workspace of the launch and wires it, and the modes the kernels look at, into m.p.
static int cost_workspace(ppgpu_ctx* c, CostLaunch& m) {
    PPParams& p = m.p;
    const size_t total = (size_t)p.n_edges, ws = (size_t)m.slice;
    hipStream_t st = c->stream;
    int rc;
    if (!p.child) {
        // the heuristic kernel reads the child ribbon lists: keep them in a scratch the caller never sees
        int stride = c->max_vertex_ribbons + 8;
        if (stride > PP_WAVE) stride = PP_WAVE;
        if ((rc = c->int_child.reserve(total * stride * 4, false, st))) return rc;
        p.child = c->int_child.p;
        p.stride = stride;
    }
    p.nch = m.nch; p.ngp = m.ngp;
    if ((rc = c->setup.reserve(ws, false, st)) || (rc = c->track_hits.reserve(ws * p.ngp, false, st)) ||
        (rc = c->track_eq.reserve(ws * p.nch, false, st)) || (rc = c->track_chunk_hits.reserve(ws * p.nch, false, st)) ||
        (rc = c->track_summary.reserve(ws, false, st)) || (rc = c->track_far.reserve(ws, false, st)) ||
        (rc = c->track_skip.reserve(ws * p.nch, false, st)))
        return rc;
    if (m.gaussian && ((rc = c->track_pen.reserve(ws * p.ngp, false, st)) || (rc = c->track_chunk_pen.reserve(ws * p.nch, false, st))))
        return rc;
    if ((rc = c->words.reserve(1, false, st)) || (rc = c->work.reserve(PP_WORK_WORDS, false, st))) return rc;
    p.setup = c->setup.p; p.track_hits = c->track_hits.p; p.track_eq = c->track_eq.p;
    p.track_chunk_hits = c->track_chunk_hits.p; p.track_summary = c->track_summary.p;
    p.track_far = m.prepasses ? c->track_far.p : nullptr;
    p.track_skip = m.skip_chunks ? c->track_skip.p : nullptr;
    p.track_pen = c->track_pen.p; p.track_chunk_pen = c->track_chunk_pen.p;
    p.words = c->words.p; p.reset_words = 1;      // cleared by pp_k_solve_edges (pp_launch_reset)
    p.work = c->work.p;
    p.fuse_h = m.fuse_h; p.defer_h = m.defer_h; p.quiet_finish = m.quiet_finish; p.lane_split = m.lane_split;
    if (m.packed) {
        if ((rc = c->live_list.reserve(ws * 2, false, st))) return rc;
        p.live_list = c->live_list.p;
    }
    if (m.lane_finish) {
        if ((rc = c->cover_state.reserve(ws, false, st)) || (rc = c->hw_list.reserve(total, false, st))) return rc;
        p.cover_state = c->cover_state.p; p.hw_list = c->hw_list.p;
    }
    if (m.defer_h) {
        if ((rc = c->defer_list.reserve(total * PP_HL_MAX_N, false, st))) return rc;
        p.defer_list = c->defer_list.p;
    }
    if (m.share) {
        const unsigned* const table_was = c->share_head.p;
        // (with shared tracks the table has a second half, the stop classes')
        if ((rc = c->share_head.reserve((size_t)p.nverts * (m.tracks ? 2 : 1) * PP_SHARE_KEYS * PP_SHARE_STRIDE, false, st)) || (rc = c->share_of.reserve(total, false, st))) return rc;
        if (c->share_head.p != table_was) c->share_head_stale = true;      // (a grown table is a new one: nothing is kept)
        p.share_head = c->share_head.p; p.share_of = c->share_of.p;
    }
    if (m.sweep_list) {
        if ((rc = c->sweep_list.reserve(ws + PP_WPB, false, st))) return rc;      // (every wave of the pose sweep's grid reads "its" entry)
        p.sweep_list = c->sweep_list.p;
        p.approach_list = c->approach_list ? 1 : 0;       // (m.share: the prepasses run and the live list exists)
    }
    if (m.tracks) {
        const int* const stops_was = c->arc_stop.p;
        if ((rc = c->arc_stop.reserve((size_t)p.nverts * PP_SHARE_KEYS, false, st)) || (rc = c->stop_of.reserve(ws, false, st)) || (rc = c->stop_list.reserve(ws, false, st))) return rc;
        if (c->arc_stop.p != stops_was) c->arc_stops_stale = true;
        p.arc_stop = c->arc_stop.p; p.stop_of = c->stop_of.p; p.stop_list = c->stop_list.p;
    }
    return PPGPU_OK;
}

// A sliced launch re-uses its events: bank the durations of the slice before (timing is a measurement aid: the wait costs the
// overlap between slices, nothing else).
static int bank_slice_timing(ppgpu_ctx* c, bool packed) {
    hipEvent_t* ev = c->ev_ring[c->ev_slot];
    HIP_TRY(hipEventSynchronize(ev[EV_COVERED]));
    float ms[4] = {0, 0, 0, 0};
    int rc = slice_durations(ev, ms);
    if (rc) return rc;
    for (int i = 0; i < 4; i++) c->ms_ring[c->ev_slot][i] += ms[i];
    if (packed) { unsigned live = 0; HIP_TRY(hipMemcpy(&live, &c->words.p->live_count, sizeof(unsigned), hipMemcpyDeviceToHost)); c->live_earlier_slices += live; }
    return PPGPU_OK;
}

// The kernels of one slice (p.e_base, p.n_edges): solve, [plan skips,] pose sweep, [approach prepass,] cover sweep[, lane finish].
static int cost_slice(ppgpu_ctx* c, const CostLaunch& m) {
    const PPParams& p = m.p;
    hipStream_t st = c->stream;
    hipEvent_t* ev = c->ev_ring[c->ev_slot];
    if (c->timing) HIP_TRY(hipEventRecord(ev[EV_BEGIN], st));
    hipLaunchKernelGGL(c->solve_all_words ? pp_k_solve_edges_all_words : pp_k_solve_edges, dim3((unsigned)((p.n_edges + 255) / 256)), dim3(256), 0, st, p);
    if (m.share) {                                               // timed with the solve
        const unsigned mark_threads = m.sweep_list ? PP_MARK_THREADS : PP_MARK_THREADS_PLAIN;
        hipLaunchKernelGGL(pp_k_mark_sweeps, dim3((unsigned)((p.n_edges + mark_threads - 1) / mark_threads)), dim3(mark_threads), 0, st, p);
    }
    if (c->timing) HIP_TRY(hipEventRecord(ev[EV_SOLVED], st));
    if (m.skip_chunks) {                                         // timed with the pose sweep
        // one workgroup per epw consecutive edges (of the sweep list, where the launch has one: the grid is then the one for "every
        // edge of the slice is on it", and the workgroups past the list's end leave at once): as many as give it 256 (edge, chunk) threads
        int epw = 256 / p.nch;
        if (epw < 1) epw = 1;
        if (epw > PP_PLAN_EDGES_MAX) epw = PP_PLAN_EDGES_MAX;
        const unsigned blocks = (unsigned)((p.n_edges + epw - 1) / epw);
        const bool many = p.n_obst > PP_WAVE;
        // (each in two instantiations: over the sweep list, or `_direct` over the slice)
        void (*planner)(PPParams, int);
        if (m.sweep_list) planner = m.gaussian ? (many ? pp_k_plan_skips_gaussian_many : (c->plan_spans ? pp_k_plan_skips_gaussian : pp_k_plan_skips_gaussian_chunkwise))
                                               : (many ? pp_k_plan_skips_many : (c->plan_spans ? pp_k_plan_skips : pp_k_plan_skips_chunkwise));
        else planner = m.gaussian ? (many ? pp_k_plan_skips_gaussian_many_direct : (c->plan_spans ? pp_k_plan_skips_gaussian_direct : pp_k_plan_skips_gaussian_chunkwise_direct))
                                  : (many ? pp_k_plan_skips_many_direct : (c->plan_spans ? pp_k_plan_skips_direct : pp_k_plan_skips_chunkwise_direct));
        hipLaunchKernelGGL(planner, dim3(blocks, (unsigned)((epw * p.nch + 255) / 256)), dim3(256), 0, st, p, epw);
    }
    void (*pose)(PPParams) = m.sweep_list ? (m.gaussian ? pp_k_pose_sweep_gaussian : pp_k_pose_sweep) : (m.gaussian ? pp_k_pose_sweep_gaussian_direct : pp_k_pose_sweep_direct);
    hipLaunchKernelGGL(pose, dim3((unsigned)((p.n_edges + PP_WPB - 1) / PP_WPB)), dim3(PP_WPB * 64), 0, st, p);   // a wave per edge
    // (timed with the pose sweep: the stop members take their head's track; the count is on the device, the grid strides over it)
    if (m.tracks) {
        const long long need = (p.n_edges + 256 / PP_TF_LANES - 1) / (256 / PP_TF_LANES);
        hipLaunchKernelGGL(pp_k_track_fanout, dim3((unsigned)(need < PP_TF_GRID ? need : PP_TF_GRID)), dim3(256), 0, st, p);
    }
    if (c->timing) HIP_TRY(hipEventRecord(ev[EV_POSED], st));
    if (m.prepasses) hipLaunchKernelGGL(p.approach_list ? pp_k_approach_events : pp_k_approach_events_direct, dim3((unsigned)((p.n_edges + PP_APPROACH_THREADS - 1) / PP_APPROACH_THREADS)), dim3(PP_APPROACH_THREADS), 0, st, p);
    if (c->timing) HIP_TRY(hipEventRecord(ev[EV_APPROACHED], st));
    hipLaunchKernelGGL(m.gaussian ? pp_k_cover_sweep_gaussian : pp_k_cover_sweep, dim3(resident_grid(c, m.gaussian, p.n_edges)), dim3(PP_WPB * 64), 0, st, p);
    if (m.lane_finish)       // (the list's length is on the device: a grid for "every edge of the slice is on it", whose spare workgroups leave at once)
        hipLaunchKernelGGL(pp_k_cover_finish, dim3((unsigned)((p.n_edges + PP_FINISH_THREADS - 1) / PP_FINISH_THREADS)), dim3(PP_FINISH_THREADS), 0, st, p);
    if (c->timing) HIP_TRY(hipEventRecord(ev[EV_COVERED], st));
    return PPGPU_OK;
}

// The table pass over the child lists the enumeration declined (ppgpu_set_tsp_table), last of all: the records to take are listed
// on the device, then a workgroup per listed record, striding, each with its own slot of workspace.  Nothing is launched while the
// switch of the launch's heuristic is off (the point-robot TSP heuristics have one, the Dubins-TSP heuristics another), for
// MaxDistance, or for a launch that keeps no child lists.
static int tsp_table_pass(ppgpu_ctx* c, const PPParams& p) {
    const bool point = p.heuristic == PPGPU_H_TSP_POINT_ALL || p.heuristic == PPGPU_H_TSP_POINT_K;
    const bool dubins = p.heuristic == PPGPU_H_TSP_DUBINS_ALL || p.heuristic == PPGPU_H_TSP_DUBINS_K;
    if (!point && !dubins) return PPGPU_OK;
    const int range_min = dubins ? c->tsp_dubins_min : c->tsp_table_min, range_max = dubins ? c->tsp_dubins_max : c->tsp_table_max;
    if (range_max <= 0 || !p.child || p.stride <= 0 || p.n_edges <= 0) return PPGPU_OK;
    hipStream_t st = c->stream;
    PPTspTableArgs q;
    q.out = p.out; q.child = p.child; q.stride = p.stride; q.n_edges = p.n_edges;
    q.heuristic = p.heuristic; q.tsp_k = p.tsp_k; q.ribw = p.ribw; q.max_speed = p.max_speed; q.tpf = p.tpf; q.h_rho = p.h_rho;
    q.min_ribbons = range_min; q.max_ribbons = range_max;
    q.list = c->tsp_list.p; q.list_cap = (unsigned)c->tsp_list.cap; q.count = (unsigned*)(c->tsp_words.p + 2); q.stats = c->tsp_words.p;
    q.slots = c->tsp_slots.p; q.bytes = c->tsp_slots.cap;
    q.T = dubins ? c->tsp_T.p : nullptr;
    if (dubins && q.list_cap > PP_TT_TCAP) q.list_cap = PP_TT_TCAP;               // a table of Dubins lengths per listed record
    if (c->timing) HIP_TRY(hipEventRecord(c->t_tsp.ev[0], st));
    HIP_TRY(hipMemsetAsync(c->tsp_words.p + 2, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(pp_k_tsp_table_list, dim3((unsigned)((p.n_edges + 255) / 256)), dim3(256), 0, st, q);
    const long long grid = p.n_edges < PP_TT_GRID ? p.n_edges : PP_TT_GRID;       // (how many of them work: see the kernel)
    if (dubins) hipLaunchKernelGGL(pp_k_tsp_table_dubins_T, dim3((unsigned)grid), dim3(256), 0, st, q);
    hipLaunchKernelGGL(dubins ? pp_k_tsp_table_dubins : pp_k_tsp_table, dim3((unsigned)grid), dim3(PP_TT_THREADS), 0, st, q);
    if (c->timing) { HIP_TRY(hipEventRecord(c->t_tsp.ev[1], st)); c->t_tsp.ms_earlier = 0; c->t_tsp.timed = true; }
    return PPGPU_OK;
}

// What is left of h once every slice is swept (p: the whole list again).
static int cost_heuristic_tail(ppgpu_ctx* c, const CostLaunch& m) {
    const PPParams& p = m.p;
    const long long total = p.n_edges;
    hipStream_t st = c->stream;
    const dim3 per_wave((unsigned)((total + PP_H_WPB - 1) / PP_H_WPB));            // a wave per edge
    if (p.heuristic == PPGPU_H_TSP_DUBINS_ALL || p.heuristic == PPGPU_H_TSP_DUBINS_K)
        hipLaunchKernelGGL(pp_k_heuristic_dubins, per_wave, dim3(PP_H_WPB * 64), 0, st, p);
    else if (!m.fuse_h)
        hipLaunchKernelGGL(pp_k_heuristic, per_wave, dim3(PP_H_WPB * 64), 0, st, p);
    // The edges whose TSP enumeration the sweeps deferred: packed into one list per ribbon count, then a few lanes each
    // (pp_k_heuristic_lanes).  The rare edge pp_k_cover_finish left to a whole wave (pp_k_heuristic_listed: 7 or 8 child ribbons,
    // ~1 100 of config 3's 236 140 edges, each a single wave's work for ~170 us) runs on a second stream BESIDE it: the lane kernel
    // fills the rest of the machine meanwhile, and the two touch different records.  The main stream waits for the side stream
    // before the launch is over.
    if (m.forked) {
        HIP_TRY(hipEventRecord(c->ev_fork, st));
        HIP_TRY(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
        // (the list's length is on the device: the grid pp_k_heuristic would get, whose workgroups beyond the list leave at once)
        hipLaunchKernelGGL(pp_k_heuristic_listed, per_wave, dim3(PP_H_WPB * 64), 0, c->side_stream, p);
        HIP_TRY(hipEventRecord(c->ev_join, c->side_stream));
    }
    if (m.defer_h) {
        hipLaunchKernelGGL(pp_k_deferred_list, dim3((unsigned)((total + 256 * PP_DL_PER - 1) / (256 * PP_DL_PER))), dim3(256), 0, st, p);
        hipLaunchKernelGGL(pp_k_heuristic_lanes, dim3((unsigned)((total * PP_HL_SPLIT + PP_HL_THREADS - 1) / PP_HL_THREADS) + PP_HL_MAX_N), dim3(PP_HL_THREADS), 0, st, p);
    }
    // child lists of 9..12 ribbons under the K variant: a second pass that touches only those edges (the others cost it one
    // 8-byte read each); a workgroup per edge, striding
    if (p.heuristic == PPGPU_H_TSP_POINT_K)
        hipLaunchKernelGGL(pp_k_heuristic_big, dim3((unsigned)(total < PP_BIG_GRID ? total : PP_BIG_GRID)), dim3(PP_BIG_WPB * 64), 0, st, p);
    if (m.forked) HIP_TRY(hipStreamWaitEvent(st, c->ev_join, 0));
    int rc = tsp_table_pass(c, p);
    if (rc) return rc;
    // last of all, when every head's record is final: the other members of each class take their head's results (16 lanes per record)
    if (m.share) hipLaunchKernelGGL(pp_k_share_fanout, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, p, m.share_child ? 1 : 0);
    return PPGPU_OK;
}

// Costs the edges `asked` describes (list_params, or the dense form's own): modes, workspace, the slices one after the other, the
// heuristic tail.  Asynchronous.  `done`: what the launch leaves for a trace of the same list.
static int launch_cost(ppgpu_ctx* c, const PPParams& asked, CostLaunch* done = nullptr) {
    CostLaunch local;
    CostLaunch& m = done ? *done : local;
    m.p = asked;
    PPParams& p = m.p;
    const long long total = p.n_edges;
    if (total <= 0) return PPGPU_OK;
    p.total_edges = total;
    if ((total + PP_WPB - 1) / PP_WPB > 0x3fffffffll) return fail(PPGPU_ECAPACITY, "cost_edges: too many edges for one launch");
    cost_modes(c, m);
    int rc = cost_workspace(c, m);
    if (rc) return rc;
    if (c->timing) c->ev_slot = (int)(c->ev_launches % PP_TIMING_RING);     // the next set of the ring
    for (double& ms : c->ms_ring[c->ev_slot]) ms = 0;
    c->live_earlier_slices = 0;
    c->last_launch_shared = false; c->last_launch_listed = false; c->last_launch_tracks = false;
    // the heads of the classes: none yet.  Per launch, not per slice: a member in a later slice finds the head of an earlier one.
    // The launch before left the table so (pp_k_share_fanout, its last kernel); only a table that is new, or that a launch which
    // failed between its slices may have left with heads in it, is filled here, all of it.  Stale until this launch's fan-out is queued.
    if (m.share) {
        if (c->share_head_stale) HIP_TRY(hipMemsetAsync(c->share_head.p, 0xff, c->share_head.cap * sizeof(unsigned), c->stream));
        c->share_head_stale = true;
    }
    // the stops of the classes' first arcs, where the vertices, the grid, the keep-out limit or the configuration changed since they
    // were last walked (a wave per class; a planner's round trip pays it once per vertex set, a loop over one vertex set once)
    if (m.tracks && c->arc_stops_stale) {
        TraceTimer& tm = c->t_arc_stops;
        tm.ms_earlier = 0;
        tm.timed = false;
        if (c->timing) {
            if (!tm.ev[0])
                for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreate(&tm.ev[i]));
            HIP_TRY(hipEventRecord(tm.ev[0], c->stream));
        }
        hipLaunchKernelGGL(pp_k_arc_stops, dim3((unsigned)(((long long)p.nverts * PP_SHARE_KEYS + PP_WPB - 1) / PP_WPB)), dim3(PP_WPB * 64), 0, c->stream, p);
        if (c->timing) { HIP_TRY(hipEventRecord(tm.ev[1], c->stream)); tm.timed = true; }
        c->arc_stops_stale = false;
    }
    c->last_launch_slices = 0;
    for (long long e0 = 0; e0 < total; e0 += m.slice) {
        p.e_base = e0; p.ws_base = 0; p.n_edges = (total - e0 < m.slice) ? (total - e0) : m.slice;
        c->last_launch_slices++; c->last_slice_edges = p.n_edges;
        if (c->timing && e0 > 0 && (rc = bank_slice_timing(c, m.packed))) return rc;
        if ((rc = cost_slice(c, m))) return rc;
    }
    p.e_base = 0;
    p.n_edges = total;
    if ((rc = cost_heuristic_tail(c, m))) return rc;
    c->last_launch_edges = total; c->last_launch_packed = m.packed; c->last_launch_shared = m.share; c->last_launch_listed = m.sweep_list; c->last_launch_tracks = m.tracks;
    if (c->timing) { HIP_TRY(hipEventRecord(c->ev_ring[c->ev_slot][EV_END], c->stream)); c->ev_launches++; }
    HIP_TRY(hipGetLastError());
    if (m.share) c->share_head_stale = false;             // (pp_k_share_fanout is in the stream)
    return PPGPU_OK;
}

int ppgpu_cost_edges_dense(ppgpu_ctx* c, int32_t v0, int32_t nv, int64_t s0, int64_t ns, uint32_t cfg_mask,
                           ppgpu_edge_result* d_results, double* d_child, int32_t stride) {
    int rc = require_world(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    cfg_mask &= 0xFu;
    if (v0 < 0 || nv <= 0 || v0 + nv > c->nverts) return fail(PPGPU_EINVAL, "cost_edges_dense: vertex range");
    if (s0 < 0 || ns <= 0 || s0 + ns > c->n_samples) return fail(PPGPU_EINVAL, "cost_edges_dense: sample range");
    if (!cfg_mask || !d_results) return fail(PPGPU_EINVAL, "cost_edges_dense: empty configuration mask or null results");
    if (d_child && stride <= 0) return fail(PPGPU_EINVAL, "cost_edges_dense: ribbon_stride must be positive");
    PPParams p;
    fill_params(c, p);
    p.edges = nullptr; p.wedges = nullptr;
    p.v0 = v0; p.nv = nv; p.s0 = s0; p.ns = ns; p.cfg_mask = cfg_mask; p.per = __builtin_popcount(cfg_mask);
    p.n_edges = (long long)nv * ns * p.per;
    p.out = d_results; p.child = d_child; p.stride = stride;
    return launch_cost(c, p);
}

int ppgpu_cost_edges_list(ppgpu_ctx* c, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, double* d_child,
                          int32_t stride) {
    int rc = require_world(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (n < 0 || (n > 0 && (!d_edges || !d_results))) return fail(PPGPU_EINVAL, "cost_edges_list: bad arguments");
    if (d_child && stride <= 0) return fail(PPGPU_EINVAL, "cost_edges_list: ribbon_stride must be positive");
    return launch_cost(c, list_params(c, n, (const unsigned long long*)d_edges, nullptr, d_results, d_child, stride));
}

// ------------------------------------------------------------------------------ edge traces
// One trace of an edge list: which kernel, and where its output goes.  The _list entries fill it with the caller's device arrays,
// the host forms with the caller's host arrays (cost_host_list then swaps in the device ends of all but the records).
enum TraceKind { TRACE_STEPS, TRACE_COVER, TRACE_CONTACTS, TRACE_CLEARANCE };
struct TraceRequest {
    TraceKind kind;
    int32_t stride;                     // step and cover records per edge (a contact trace has n_obst records per edge, a clearance trace one)
    int32_t* counts;                    // steps of each edge
    void* records;                      // ppgpu_step_record / ppgpu_cover_record / ppgpu_contact_record / ppgpu_clearance_record ...
    size_t rec_bytes;                   // ... of this size
    ppgpu_cover_summary* summaries;     // coverage traces only: one summary per edge,
    double* child;                      // the final lists (may be NULL)
    int32_t ribbon_stride;
    uint32_t limit2;                    // clearance traces only: a step is below the margin iff its gap2 < limit2
};
static TraceRequest steps_request(int32_t stride, int32_t* counts, ppgpu_step_record* steps) {
    return TraceRequest{TRACE_STEPS, stride, counts, steps, sizeof(ppgpu_step_record), nullptr, nullptr, 0, 0};
}
static TraceRequest cover_request(int32_t stride, int32_t* counts, ppgpu_cover_record* cover, ppgpu_cover_summary* summaries, double* child, int32_t ribbon_stride) {
    return TraceRequest{TRACE_COVER, stride, counts, cover, sizeof(ppgpu_cover_record), summaries, child, ribbon_stride, 0};
}
static TraceRequest contacts_request(int32_t* counts, ppgpu_contact_record* contacts) {
    return TraceRequest{TRACE_CONTACTS, 0, counts, contacts, sizeof(ppgpu_contact_record), nullptr, nullptr, 0, 0};
}
static TraceRequest clearance_request(int32_t* counts, ppgpu_clearance_record* clearance, uint32_t limit2) {
    return TraceRequest{TRACE_CLEARANCE, 1, counts, clearance, sizeof(ppgpu_clearance_record), nullptr, nullptr, 0, limit2};
}
// limit2 of a trace call's margin in metres (ppgpu_keepout_limit2 states the rule), so that the device compares integers only.
// Without a grid, or with a margin that is not above 0 (a NaN among them), no step is ever below: 0.
static int clearance_limit2(const ppgpu_ctx* c, const char* who, double margin, uint32_t* limit2) {
    *limit2 = 0;
    if (c->rows == 0 || !(margin > 0)) return PPGPU_OK;
    if (ppgpu_keepout_limit2(c->res, margin, limit2)) return fail(PPGPU_EINVAL, std::string(who) + ": margin above 255 cells");
    return PPGPU_OK;
}

// What a trace entry was handed; `who` is its name in the message.  `device`: a _list entry (device arrays, the records stored
// 16 bytes at a time; it needs the results array).  Contact records may be missing only when there is no obstacle to report on.
static int trace_request_args(const ppgpu_ctx* c, const char* who, bool device, int64_t n, const void* edges, const void* results, const TraceRequest& r) {
    static const char* const records_name[] = {"d_steps", "d_cover", "d_contacts", "d_clearance"};
    const bool cover = r.kind == TRACE_COVER, contacts = r.kind == TRACE_CONTACTS;
    if (n < 0 || (n > 0 && (!edges || !r.counts || ((!contacts || c->n_obst > 0) && !r.records)))) return fail(PPGPU_EINVAL, std::string(who) + ": bad arguments");
    if (!contacts && (r.stride <= 0 || r.stride > 65535)) return fail(PPGPU_EINVAL, std::string(who) + ": step_stride must be in 1 .. 65535");
    if (device) {
        if (n > 0 && (!results || (cover && !r.summaries))) return fail(PPGPU_EINVAL, std::string(who) + (cover ? ": null results or summaries" : ": null results"));
    } else if (cover && n > 0 && !r.summaries) {
        return fail(PPGPU_EINVAL, std::string(who) + ": null summaries");
    }
    if (cover && r.child && r.ribbon_stride <= 0) return fail(PPGPU_EINVAL, std::string(who) + ": ribbon_stride must be positive");
    if (device && ((unsigned long long)r.records & 15ull) != 0ull)
        return fail(PPGPU_EINVAL, std::string(who) + ": " + records_name[r.kind] + " must be 16-byte aligned");
    return PPGPU_OK;
}

// the trace kernel of r on one slice q, its records going to dst[(edge - rec_base) * stride + k]
static void trace_kernel(ppgpu_ctx* c, const CostLaunch& L, const PPParams& q, const TraceRequest& r, void* dst, long long rec_base) {
    const dim3 grid((unsigned)((q.n_edges + PP_TRACE_WPB - 1) / PP_TRACE_WPB)), block(PP_TRACE_WPB * 64);
    switch (r.kind) {
    case TRACE_STEPS:
        hipLaunchKernelGGL(L.gaussian ? pp_k_trace_steps_gaussian : pp_k_trace_steps, grid, block, 0, c->stream, q, (ppgpu_step_record*)dst, rec_base, r.stride, r.counts);
        break;
    case TRACE_COVER:
        hipLaunchKernelGGL(pp_k_trace_cover, grid, block, 0, c->stream, q, (ppgpu_cover_record*)dst, rec_base, r.stride, r.counts, r.summaries, r.child,
                           r.child ? r.ribbon_stride : 0);
        break;
    case TRACE_CONTACTS:
        hipLaunchKernelGGL(L.gaussian ? pp_k_trace_contacts_gaussian : pp_k_trace_contacts, grid, block, 0, c->stream, q, (ppgpu_contact_record*)dst, rec_base, r.counts);
        break;
    case TRACE_CLEARANCE:
        hipLaunchKernelGGL(pp_k_trace_clearance, grid, block, 0, c->stream, q, c->grid_dist.p, r.limit2, (ppgpu_clearance_record*)dst, rec_base, r.counts);
        break;
    }
}

// A trace of the list the launch L just costed, `stride` records per edge to `recs`.  A trace kernel reads the PPEdgeSetup records of
// the costing launch: they are all still in the workspace when that launch ran as one slice; a launch that ran as several has only
// its last slice's left, and pp_k_solve_edges writes them again, slice by slice (a fraction of the time the records take to write).
// Host form (`host`: recs is a host array): the records of one pass go through tmp_trace, at most the handle's slice budget at a
// time; what the caller's array holds beyond an edge's count stays as it is (the pass starts from the caller's bytes).
static int trace_passes(ppgpu_ctx* c, const CostLaunch& L, const TraceRequest& r, TraceTimer& tm, int stride, unsigned char* recs, bool host) {
    const PPParams& p = L.p;
    const long long total = p.n_edges;            // (> 0: an empty list never gets as far as a launch)
    const bool reuse = L.slice >= total;
    const size_t edge_bytes = (size_t)stride * r.rec_bytes;
    long long pass = reuse ? total : L.slice;
    if (host) {
        long long cap = (long long)(c->slice_bytes / edge_bytes);
        if (cap < 1) cap = 1;
        if (pass > cap) pass = cap;
        int rc = c->tmp_trace.reserve((size_t)pass * edge_bytes, false, c->stream);
        if (rc) return rc;
    }
    tm.ms_earlier = 0;
    tm.timed = false;
    for (long long e0 = 0; e0 < total; e0 += pass) {
        PPParams q = p;
        q.e_base = e0; q.n_edges = (total - e0 < pass) ? (total - e0) : pass;
        q.ws_base = reuse ? e0 : 0;
        if (!reuse) {
            q.reset_words = 0;       // (the counters are the costing launch's: ppgpu_last_cover_edges still reads them)
            q.share_head = nullptr;  // (a trace walks every edge itself: no class is elected again)
            hipLaunchKernelGGL(c->solve_all_words ? pp_k_solve_edges_all_words : pp_k_solve_edges, dim3((unsigned)((q.n_edges + 255) / 256)), dim3(256), 0, c->stream, q);
        }
        unsigned char* dst = host ? c->tmp_trace.p : recs;
        const size_t bytes = (size_t)q.n_edges * edge_bytes;
        if (host) HIP_TRY(hipMemcpyAsync(dst, recs + (size_t)e0 * edge_bytes, bytes, hipMemcpyHostToDevice, c->stream));
        if (c->timing && tm.timed) {                    // a further slice re-uses the events: bank the one before
            float ms = 0;
            HIP_TRY(hipEventSynchronize(tm.ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms, tm.ev[0], tm.ev[1]));
            tm.ms_earlier += ms;
        }
        if (c->timing) HIP_TRY(hipEventRecord(tm.ev[0], c->stream));
        trace_kernel(c, L, q, r, dst, host ? e0 : 0ll);
        if (c->timing) { HIP_TRY(hipEventRecord(tm.ev[1], c->stream)); tm.timed = true; }
        HIP_TRY(hipGetLastError());
        if (host) {
            HIP_TRY(hipMemcpyAsync(recs + (size_t)e0 * edge_bytes, dst, bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));   // the next pass writes the same buffer
        }
    }
    return PPGPU_OK;
}

static int trace_timing(ppgpu_ctx* c, TraceTimer& tm, double* ms_out) {
    if (!c || !ms_out) return fail(PPGPU_EINVAL, "null argument");
    if (!c->timing || !tm.timed) return fail(PPGPU_ESTATE, "no timed trace launch (ppgpu_enable_timing, then trace edges)");
    HIP_TRY(hipSetDevice(c->device));
    float ms = 0;
    HIP_TRY(hipEventSynchronize(tm.ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms, tm.ev[0], tm.ev[1]));
    *ms_out = ms + tm.ms_earlier;
    return PPGPU_OK;
}

// The trace r over the list of L; r's counts (summaries, child) are device arrays, its records the caller's host array when
// `host_records`.  A contact trace has n_obst records per edge; without obstacles the kernel still runs, for the counts, and is
// handed no records.
static int launch_trace(ppgpu_ctx* c, const CostLaunch& L, const TraceRequest& r, bool host_records) {
    TraceTimer& tm = r.kind == TRACE_STEPS ? c->t_steps : r.kind == TRACE_COVER ? c->t_cover : r.kind == TRACE_CONTACTS ? c->t_contacts : c->t_clearance;
    if (r.kind == TRACE_CLEARANCE && c->rows > 0) {       // the walk reads the distance map: the first one after a ppgpu_set_grid builds it
        const int rc = grid_distance(c);
        if (rc) return rc;
    }
    if (r.kind != TRACE_CONTACTS) return trace_passes(c, L, r, tm, r.stride, (unsigned char*)r.records, host_records);
    const bool none = L.p.n_obst <= 0;
    return trace_passes(c, L, r, tm, none ? 1 : L.p.n_obst, none ? nullptr : (unsigned char*)r.records, host_records && !none);
}

int ppgpu_last_trace_timing(ppgpu_ctx* c, double* ms_trace) { return c ? trace_timing(c, c->t_steps, ms_trace) : fail(PPGPU_EINVAL, "null argument"); }
int ppgpu_last_cover_trace_timing(ppgpu_ctx* c, double* ms) { return c ? trace_timing(c, c->t_cover, ms) : fail(PPGPU_EINVAL, "null argument"); }
int ppgpu_last_contact_trace_timing(ppgpu_ctx* c, double* ms) { return c ? trace_timing(c, c->t_contacts, ms) : fail(PPGPU_EINVAL, "null argument"); }
int ppgpu_last_clearance_trace_timing(ppgpu_ctx* c, double* ms) { return c ? trace_timing(c, c->t_clearance, ms) : fail(PPGPU_EINVAL, "null argument"); }
int ppgpu_last_grid_distance_timing(ppgpu_ctx* c, double* ms) { return c ? trace_timing(c, c->t_dist, ms) : fail(PPGPU_EINVAL, "null argument"); }
int ppgpu_last_keepout_timing(ppgpu_ctx* c, double* ms) { return c ? trace_timing(c, c->t_keepout, ms) : fail(PPGPU_EINVAL, "null argument"); }
int ppgpu_last_arc_stops_timing(ppgpu_ctx* c, double* ms) { return c ? trace_timing(c, c->t_arc_stops, ms) : fail(PPGPU_EINVAL, "null argument"); }
int ppgpu_last_tsp_table_timing(ppgpu_ctx* c, double* ms) { return c ? trace_timing(c, c->t_tsp, ms) : fail(PPGPU_EINVAL, "null argument"); }

// A device list in, device records out: cost the list, then trace it.
static int trace_device_list(ppgpu_ctx* c, const char* who, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, const TraceRequest& r) {
    int rc = require_world(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = trace_request_args(c, who, true, n, d_edges, d_results, r))) return rc;
    if (n == 0) return PPGPU_OK;
    CostLaunch L;
    if ((rc = launch_cost(c, list_params(c, n, (const unsigned long long*)d_edges, nullptr, d_results, nullptr, 0), &L))) return rc;
    return launch_trace(c, L, r, false);
}

int ppgpu_trace_edges_list(ppgpu_ctx* c, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, int32_t stride,
                           int32_t* d_counts, ppgpu_step_record* d_steps) {
    return trace_device_list(c, "trace_edges_list", n, d_edges, d_results, steps_request(stride, d_counts, d_steps));
}

int ppgpu_trace_cover_list(ppgpu_ctx* c, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, int32_t stride, int32_t* d_counts,
                           ppgpu_cover_record* d_cover, ppgpu_cover_summary* d_summaries, double* d_child, int32_t ribbon_stride) {
    return trace_device_list(c, "trace_cover_list", n, d_edges, d_results, cover_request(stride, d_counts, d_cover, d_summaries, d_child, ribbon_stride));
}

int ppgpu_trace_contacts_list(ppgpu_ctx* c, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, int32_t* d_counts,
                              ppgpu_contact_record* d_contacts) {
    return trace_device_list(c, "trace_contacts_list", n, d_edges, d_results, contacts_request(d_counts, d_contacts));
}

int ppgpu_trace_clearance_list(ppgpu_ctx* c, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, int32_t* d_counts,
                               ppgpu_clearance_record* d_clearance, double margin) {
    uint32_t limit2;
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (int rc = clearance_limit2(c, "trace_clearance_list", margin, &limit2)) return rc;
    return trace_device_list(c, "trace_clearance_list", n, d_edges, d_results, clearance_request(d_counts, d_clearance, limit2));
}

int ppgpu_obstacle_count(ppgpu_ctx* c, int32_t* n, int32_t* model) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (n) *n = c->n_obst;
    if (model) *model = c->n_obst > 0 ? c->obst_model : PPGPU_OBST_NONE;
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ host lists
// A host list in, host records out: `who`'s n packed descriptors, or wrapper edges (`wrapper`), go up to tmp_edges / tmp_wedges,
// are costed into tmp_results (child ribbons into a zeroed tmp_child when the caller wants them) and, for the trace forms (`trace`:
// the caller's host arrays), traced; records, child ribbons and counts come home, a coverage trace's summaries and final lists as
// well; one synchronise at the end.  h_results may be NULL for a trace.
static int cost_host_list(ppgpu_ctx* c, const char* who, bool wrapper, int64_t n, const void* h_list, ppgpu_edge_result* h_results,
                          double* h_child, int32_t stride, const TraceRequest* trace = nullptr) {
    int rc = wrapper ? require_vertices(c) : require_world(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (trace) {
        if ((rc = trace_request_args(c, who, false, n, h_list, nullptr, *trace))) return rc;
    } else if (n < 0 || (n > 0 && (!h_list || !h_results))) {
        return fail(PPGPU_EINVAL, std::string(who) + ": bad arguments");
    }
    if (n == 0) return PPGPU_OK;
    if (h_child && stride <= 0) return fail(PPGPU_EINVAL, std::string(who) + ": ribbon_stride must be positive");
    if (wrapper && (rc = check_wrapper_edges(c, who, n, (const ppgpu_wrapper_edge*)h_list))) return rc;
    hipStream_t st = c->stream;
    const bool cover = trace && trace->kind == TRACE_COVER;
    const size_t child_bytes = h_child ? (size_t)n * stride * 4 * sizeof(double) : 0;
    if ((rc = wrapper ? c->tmp_wedges.reserve((size_t)n, false, st) : c->tmp_edges.reserve((size_t)n, false, st)) ||
        (rc = c->tmp_results.reserve((size_t)n, false, st)) || (h_child && (rc = c->tmp_child.reserve((size_t)n * stride * 4, false, st))) ||
        (trace && (rc = c->tmp_counts.reserve((size_t)n, false, st))))
        return rc;
    const size_t final_bytes = (cover && trace->child) ? (size_t)n * trace->ribbon_stride * 4 * sizeof(double) : 0;
    if (cover && ((rc = c->tmp_summaries.reserve((size_t)n, false, st)) ||
                  (final_bytes && (rc = c->tmp_cover_child.reserve(final_bytes / sizeof(double), false, st)))))
        return rc;
    if (wrapper) HIP_TRY(hipMemcpyAsync(c->tmp_wedges.p, h_list, (size_t)n * sizeof(ppgpu_wrapper_edge), hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpyAsync(c->tmp_edges.p, h_list, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (h_child) HIP_TRY(hipMemsetAsync(c->tmp_child.p, 0, child_bytes, st));
    CostLaunch L;
    if ((rc = launch_cost(c, list_params(c, n, wrapper ? nullptr : c->tmp_edges.p, wrapper ? c->tmp_wedges.p : nullptr, c->tmp_results.p,
                                         h_child ? c->tmp_child.p : nullptr, stride), &L)))
        return rc;
    if (h_results) HIP_TRY(hipMemcpyAsync(h_results, c->tmp_results.p, (size_t)n * sizeof(ppgpu_edge_result), hipMemcpyDeviceToHost, st));
    if (h_child) HIP_TRY(hipMemcpyAsync(h_child, c->tmp_child.p, child_bytes, hipMemcpyDeviceToHost, st));
    if (trace) {
        TraceRequest d = *trace;                    // the caller's records, the device ends of the rest
        d.counts = c->tmp_counts.p;
        if (cover) { d.summaries = c->tmp_summaries.p; d.child = final_bytes ? c->tmp_cover_child.p : nullptr; }
        if (final_bytes) HIP_TRY(hipMemsetAsync(c->tmp_cover_child.p, 0, final_bytes, st));
        if ((rc = launch_trace(c, L, d, true))) return rc;
        HIP_TRY(hipMemcpyAsync(trace->counts, c->tmp_counts.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (cover) HIP_TRY(hipMemcpyAsync(trace->summaries, c->tmp_summaries.p, (size_t)n * sizeof(ppgpu_cover_summary), hipMemcpyDeviceToHost, st));
        if (final_bytes) HIP_TRY(hipMemcpyAsync(trace->child, c->tmp_cover_child.p, final_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return PPGPU_OK;
}

int ppgpu_cost_edges_host(ppgpu_ctx* c, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results, double* h_child,
                          int32_t stride) {
    return cost_host_list(c, "cost_edges_host", false, n, h_edges, h_results, h_child, stride);
}

int ppgpu_cost_wrapper_edges_host(ppgpu_ctx* c, int64_t n, const ppgpu_wrapper_edge* h_edges, ppgpu_edge_result* h_results,
                                  double* h_child, int32_t stride) {
    return cost_host_list(c, "cost_wrapper_edges_host", true, n, h_edges, h_results, h_child, stride);
}

int ppgpu_trace_edges_host(ppgpu_ctx* c, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results, int32_t stride,
                           int32_t* h_counts, ppgpu_step_record* h_steps) {
    const TraceRequest trace = steps_request(stride, h_counts, h_steps);
    return cost_host_list(c, "trace_edges_host", false, n, h_edges, h_results, nullptr, 0, &trace);
}

int ppgpu_trace_wrapper_edges_host(ppgpu_ctx* c, int64_t n, const ppgpu_wrapper_edge* h_edges, ppgpu_edge_result* h_results,
                                   int32_t stride, int32_t* h_counts, ppgpu_step_record* h_steps) {
    const TraceRequest trace = steps_request(stride, h_counts, h_steps);
    return cost_host_list(c, "trace_wrapper_edges_host", true, n, h_edges, h_results, nullptr, 0, &trace);
}

int ppgpu_trace_cover_host(ppgpu_ctx* c, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results, int32_t stride, int32_t* h_counts,
                           ppgpu_cover_record* h_cover, ppgpu_cover_summary* h_summaries, double* h_child, int32_t ribbon_stride) {
    const TraceRequest trace = cover_request(stride, h_counts, h_cover, h_summaries, h_child, ribbon_stride);
    return cost_host_list(c, "trace_cover_host", false, n, h_edges, h_results, nullptr, 0, &trace);
}

int ppgpu_trace_cover_wrapper_edges_host(ppgpu_ctx* c, int64_t n, const ppgpu_wrapper_edge* h_edges, ppgpu_edge_result* h_results, int32_t stride,
                                         int32_t* h_counts, ppgpu_cover_record* h_cover, ppgpu_cover_summary* h_summaries, double* h_child,
                                         int32_t ribbon_stride) {
    const TraceRequest trace = cover_request(stride, h_counts, h_cover, h_summaries, h_child, ribbon_stride);
    return cost_host_list(c, "trace_cover_wrapper_edges_host", true, n, h_edges, h_results, nullptr, 0, &trace);
}

int ppgpu_trace_contacts_host(ppgpu_ctx* c, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results, int32_t* h_counts,
                              ppgpu_contact_record* h_contacts) {
    const TraceRequest trace = contacts_request(h_counts, h_contacts);
    return cost_host_list(c, "trace_contacts_host", false, n, h_edges, h_results, nullptr, 0, &trace);
}

int ppgpu_trace_contacts_wrapper_edges_host(ppgpu_ctx* c, int64_t n, const ppgpu_wrapper_edge* h_edges, ppgpu_edge_result* h_results,
                                            int32_t* h_counts, ppgpu_contact_record* h_contacts) {
    const TraceRequest trace = contacts_request(h_counts, h_contacts);
    return cost_host_list(c, "trace_contacts_wrapper_edges_host", true, n, h_edges, h_results, nullptr, 0, &trace);
}

int ppgpu_trace_clearance_host(ppgpu_ctx* c, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results, int32_t* h_counts,
                               ppgpu_clearance_record* h_clearance, double margin) {
    uint32_t limit2;
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (int rc = clearance_limit2(c, "trace_clearance_host", margin, &limit2)) return rc;
    const TraceRequest trace = clearance_request(h_counts, h_clearance, limit2);
    return cost_host_list(c, "trace_clearance_host", false, n, h_edges, h_results, nullptr, 0, &trace);
}

int ppgpu_trace_clearance_wrapper_edges_host(ppgpu_ctx* c, int64_t n, const ppgpu_wrapper_edge* h_edges, ppgpu_edge_result* h_results,
                                             int32_t* h_counts, ppgpu_clearance_record* h_clearance, double margin) {
    uint32_t limit2;
    if (!c) return fail(PPGPU_EINVAL, "null context");
    if (int rc = clearance_limit2(c, "trace_clearance_wrapper_edges_host", margin, &limit2)) return rc;
    const TraceRequest trace = clearance_request(h_counts, h_clearance, limit2);
    return cost_host_list(c, "trace_clearance_wrapper_edges_host", true, n, h_edges, h_results, nullptr, 0, &trace);
}

// ------------------------------------------------------------------------------ heuristic on its own
int ppgpu_heuristic_host(ppgpu_ctx* c, int32_t n, const double* poses3, const int32_t* counts, const double* ribbons, double* h_out, uint32_t* h_flags) {
    int rc = require_cfg(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (n <= 0 || !poses3 || !counts || !h_out) return fail(PPGPU_EINVAL, "heuristic_host: bad arguments");
    int stride = 1;
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (counts[i] < 0 || counts[i] > PP_WAVE) return fail(PPGPU_ECAPACITY, "heuristic_host: between 0 and 64 ribbons per pose");
        if (counts[i] > stride) stride = counts[i];
        total += (size_t)counts[i];
    }
    if (total > 0 && !ribbons) return fail(PPGPU_EINVAL, "heuristic_host: ribbons are null");
    // records as the cover sweep would leave them: end pose, g = 0, ribbon count; child ribbons at `stride` per record
    std::vector<ppgpu_edge_result> rec((size_t)n);
    std::vector<double> child((size_t)n * stride * 4, 0.0);
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        std::memset(&rec[i], 0, sizeof(ppgpu_edge_result));
        rec[i].info = (uint32_t)counts[i] << 8;
        rec[i].end_x = poses3[3 * i]; rec[i].end_y = poses3[3 * i + 1]; rec[i].end_heading = poses3[3 * i + 2];
        if (counts[i] > 0) std::memcpy(child.data() + (size_t)i * stride * 4, ribbons + off * 4, (size_t)counts[i] * 4 * sizeof(double));
        off += (size_t)counts[i];
    }
    if ((rc = c->tmp_results.reserve((size_t)n, false, c->stream)) || (rc = c->tmp_child.reserve(child.size(), false, c->stream)) ||
        (rc = c->words.reserve(1, false, c->stream)))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->tmp_results.p, rec.data(), rec.size() * sizeof(ppgpu_edge_result), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->tmp_child.p, child.data(), child.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const unsigned one = 1u;       // let the 12-ribbon pass look at every record
    HIP_TRY(hipMemcpyAsync(&c->words.p->need_big, &one, sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    PPParams p;
    fill_params(c, p);
    p.edges = nullptr; p.wedges = nullptr; p.n_edges = n; p.total_edges = n; p.e_base = 0; p.ws_base = 0;
    p.out = c->tmp_results.p; p.child = c->tmp_child.p; p.stride = stride; p.words = c->words.p;
    const dim3 grid((unsigned)((n + PP_H_WPB - 1) / PP_H_WPB)), block(PP_H_WPB * 64);   // n is small: never more than fits
    if (p.heuristic == PPGPU_H_TSP_DUBINS_ALL || p.heuristic == PPGPU_H_TSP_DUBINS_K) hipLaunchKernelGGL(pp_k_heuristic_dubins, grid, block, 0, c->stream, p);
    else hipLaunchKernelGGL(pp_k_heuristic, grid, block, 0, c->stream, p);
    if (p.heuristic == PPGPU_H_TSP_POINT_K)
        hipLaunchKernelGGL(pp_k_heuristic_big, dim3((unsigned)(n < PP_BIG_GRID ? n : PP_BIG_GRID)), dim3(PP_BIG_WPB * 64), 0, c->stream, p);
    if ((rc = tsp_table_pass(c, p))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rec.data(), c->tmp_results.p, rec.size() * sizeof(ppgpu_edge_result), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) {
        h_out[i] = rec[i].h;
        if (h_flags) h_flags[i] = rec[i].flags;
    }
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ expand
int64_t ppgpu_expand_capacity(int32_t nv, int32_t k) {
    if (nv <= 0) return 0;
    if (k < 0) k = 0;
    return (int64_t)nv * (4 + 4 * (int64_t)k);
}

// grow-only pinned staging: one H2D in, one D2H out per call instead of a dozen pageable copies
static int stage_reserve(void** p, size_t* cap, size_t n) {
    if (n <= *cap) return PPGPU_OK;
    GrowthTimer growth;
    size_t ncap = *cap ? *cap : 4096;
    while (ncap < n) ncap *= 2;
    if (*p) HIP_TRY(hipHostFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(hipHostMalloc(p, ncap, hipHostMallocDefault));
    *cap = ncap;
    return PPGPU_OK;
}

int ppgpu_expand_host(ppgpu_ctx* c, int32_t nv, const ppgpu_vertex* hv, int32_t n_ribbons, const double* hr, const double* h_nearest,
                      int32_t k, int64_t* n_edges, uint64_t* h_edges, ppgpu_edge_result* h_results, double* h_child, int32_t stride) {
    int rc = require_cfg(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (nv <= 0 || !hv || n_ribbons < 0 || (n_ribbons > 0 && !hr) || k < 0 || !n_edges || !h_edges || !h_results)
        return fail(PPGPU_EINVAL, "expand_host: bad arguments");
    if (h_child && stride <= 0) return fail(PPGPU_EINVAL, "expand_host: ribbon_stride must be positive");
    if (nv > 65535) return fail(PPGPU_ECAPACITY, "expand_host: at most 65535 vertices per call");
    int maxr = 0;
    if ((rc = check_open_vertices(c, "expand_host", nv, hv, n_ribbons, &maxr))) return rc;
    const long long ns = c->n_samples;
    const bool select = ns > 0 && k > 0;
    const int E = 4 + 4 * k;
    const long long cap = (long long)nv * E;
    hipStream_t st = c->stream;
    // ---- stage in: one block (PPExpandBlock)
    const PPExpandBlock in(nv, n_ribbons);
    const size_t in_bytes = in.bytes;
    if ((rc = stage_reserve(&c->stage_in, &c->stage_in_cap, in_bytes))) return rc;
    char* sin = (char*)c->stage_in;
    std::memcpy(sin + in.verts, hv, (size_t)nv * sizeof(ppgpu_vertex));
    if (n_ribbons > 0) std::memcpy(sin + in.ribbons, hr, (size_t)n_ribbons * 4 * sizeof(double));
    for (int i = 0; i < nv; i++) {
        const bool has = h_nearest && !std::isnan(h_nearest[3 * i]);
        ((double*)(sin + in.x))[i] = has ? h_nearest[3 * i] : 0.0;
        ((double*)(sin + in.y))[i] = has ? h_nearest[3 * i + 1] : 0.0;
        ((double*)(sin + in.heading))[i] = has ? h_nearest[3 * i + 2] : 0.0;
        ((unsigned char*)(sin + in.flags))[i] = has ? 1 : 0;
    }
    const size_t need = (size_t)(ns + nv);
    if ((rc = c->verts.reserve((size_t)nv, false, st)) || (rc = c->ribbons.reserve((size_t)(n_ribbons > 0 ? n_ribbons : 1) * 4, false, st)) ||
        (rc = c->tgrid.reserve((size_t)nv * c->ng, false, st)) || (rc = c->sx.reserve(need, true, st)) || (rc = c->sy.reserve(need, true, st)) ||
        (rc = c->sh.reserve(need, true, st)) || (rc = c->s_bytes.reserve((size_t)nv, false, st)))
        return rc;
    // ---- stage out (device end): header {push-order fallbacks} | descriptors | records | child ribbons, one block, one download
    const size_t q_e = 128, q_r = q_e + (size_t)cap * sizeof(uint64_t), q_c = q_r + (size_t)cap * sizeof(ppgpu_edge_result),
                 out_bytes = q_c + (h_child ? (size_t)cap * stride * 4 * sizeof(double) : 0);
    if ((rc = c->dstage_out.reserve(out_bytes, false, st))) return rc;
    unsigned long long* d_header = (unsigned long long*)c->dstage_out.p;
    unsigned long long* d_edges = (unsigned long long*)(c->dstage_out.p + q_e);
    ppgpu_edge_result* d_results = (ppgpu_edge_result*)(c->dstage_out.p + q_r);
    double* d_child = h_child ? (double*)(c->dstage_out.p + q_c) : nullptr;
    if ((rc = c->dstage_in.reserve(in_bytes, false, st)) || (rc = c->expand.fallbacks.reserve(1, false, st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->dstage_in.p, sin, in_bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pp_k_expand_unpack, dim3((unsigned)((in_bytes / 8 + nv + 255) / 256)), dim3(256), 0, st, c->dstage_in.p, nv, n_ribbons,
                       c->verts.p, c->ribbons.p, c->sx.p + ns, c->sy.p + ns, c->sh.p + ns, c->s_bytes.p, c->expand.fallbacks.p);
    c->nverts = nv; c->nribbons = n_ribbons; c->max_vertex_ribbons = maxr; c->n_extra = nv;
    c->arc_stops_stale = true;
    hipLaunchKernelGGL(pp_k_time_grid, dim3((unsigned)nv), dim3(64), 0, st, c->verts.p, nv, c->cfg.start_state_time,
                       c->cfg.collision_checking_increment, c->cfg.max_speed, c->ng, c->tgrid.p);
    // ---- k nearest per (vertex, radius), on the device
    if (select && (rc = launch_expand_order(c, nv, k, false))) return rc;   // the k winners per (vertex, radius) in the order expand() pushes them
    const ExpandLoops loops = expand_loops(c->cfg);
    hipLaunchKernelGGL(pp_k_build_expand_edges, dim3((unsigned)((nv + 63) / 64)), dim3(64), 0, st, nv, k, select ? c->expand.idx.p : nullptr,
                       c->s_bytes.p, ns, loops.two_speeds, loops.two_radii, E, d_edges, select ? c->expand.fallbacks.p : nullptr, d_header);
    HIP_TRY(hipGetLastError());
    // ---- cost the whole list.  (The child block is NOT cleared on the device: an edge's slots beyond its own ribbon count are
    // written by nobody and read by nobody there; the copy-out below hands the caller zeros for them.)
    if ((rc = launch_cost(c, list_params(c, cap, d_edges, nullptr, d_results, d_child, stride)))) return rc;
    if ((rc = stage_reserve(&c->stage_out, &c->stage_out_cap, out_bytes))) return rc;
    char* sout = (char*)c->stage_out;
    HIP_TRY(hipMemcpyAsync(sout, c->dstage_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->order_fallbacks += *(const unsigned long long*)sout;
    const uint64_t* se = (const uint64_t*)(sout + q_e);
    const ppgpu_edge_result* sr = (const ppgpu_edge_result*)(sout + q_r);
    const double* sc = (const double*)(sout + q_c);
    int64_t n = 0;
    for (long long i = 0; i < cap; i++) {
        if (se[i] == ~0ull) continue;
        h_edges[n] = se[i];
        h_results[n] = sr[i];
        if (h_child) {
            // the edge's own ribbons, zeros behind them (a record that reports more ribbons than the stride holds: the stride's worth)
            int have = (int)((sr[i].info >> 8) & 0xffu);
            if (have > stride || (sr[i].flags & PPGPU_F_THROWS)) have = (sr[i].flags & PPGPU_F_THROWS) ? 0 : stride;
            double* dst = h_child + (size_t)n * stride * 4;
            std::memcpy(dst, sc + (size_t)i * stride * 4, (size_t)have * 4 * sizeof(double));
            std::memset(dst + (size_t)have * 4, 0, (size_t)(stride - have) * 4 * sizeof(double));
        }
        n++;
    }
    *n_edges = n;
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ plan chains
// Depth d of the call costs leg d of every plan that has one, as ONE wrapper-edge launch; pp_k_chain_advance then makes each
// plan's record the open vertex of its next leg and pp_k_time_grid builds that vertex's row.  Plans are handled most legs first,
// so "the plans with more than d legs" is a prefix [0, n_d) and the legs, records and child slots of a depth are contiguous.
// Running vertices live BEHIND the caller's open vertices (verts / tgrid rows nverts + j, ribbons from nribbons on, one stride
// per plan); c->nverts and c->nribbons are never touched, so the handle is what the caller left once the call returns.
int ppgpu_cost_plans_host(ppgpu_ctx* c, int32_t n_plans, const int32_t* offs, const ppgpu_wrapper_edge* h_legs, ppgpu_edge_result* h_results,
                          double* h_child, int32_t stride, int32_t* h_costed, uint32_t* h_stop) {
    int rc = require_vertices(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (n_plans < 0 || (n_plans > 0 && (!offs || !h_costed || !h_stop))) return fail(PPGPU_EINVAL, "cost_plans_host: bad arguments");
    if (stride <= 0 || stride > PP_WAVE) return fail(PPGPU_EINVAL, "cost_plans_host: ribbon_stride must be in 1 .. 64");
    if (n_plans == 0) return PPGPU_OK;
    if (offs[0] < 0) return fail(PPGPU_EINVAL, "cost_plans_host: negative leg offset");
    for (int p = 0; p < n_plans; p++)
        if (offs[p + 1] < offs[p]) return fail(PPGPU_EINVAL, "cost_plans_host: leg offsets must not decrease");
    if (offs[n_plans] > offs[0] && (!h_legs || !h_results)) return fail(PPGPU_EINVAL, "cost_plans_host: null legs or results");
    if (offs[n_plans] > offs[0] && (rc = check_wrapper_edges(c, "cost_plans_host", offs[n_plans] - offs[0], h_legs + offs[0]))) return rc;
    for (int i = offs[0]; i < offs[n_plans]; i++) {
        const ppgpu_wrapper_edge& w = h_legs[i];
        if (w.rho != (w.coverage_allowed ? c->cfg.coverage_turning_radius : c->cfg.turning_radius))
            return fail(PPGPU_EINVAL, "cost_plans_host: a leg's rho differs from the radius its coverage flag implies (Edge.cpp:78-80 re-solves it: "
                                      "end the chain before it and route it through ppgpu_cost_edges_*)");
    }
    // device order: most legs first (stable, so equal plans keep the caller's order)
    std::vector<int> order((size_t)n_plans);
    for (int p = 0; p < n_plans; p++) order[(size_t)p] = p;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return offs[a + 1] - offs[a] > offs[b + 1] - offs[b]; });
    const int maxLegs = offs[order[0] + 1] - offs[order[0]];
    for (int p = 0; p < n_plans; p++) { h_costed[p] = 0; h_stop[p] = PPGPU_CHAIN_LEGS; }
    if (maxLegs == 0) return PPGPU_OK;
    std::vector<int> nAt((size_t)maxLegs, 0);             // plans that have a leg at depth d
    std::vector<size_t> at((size_t)maxLegs + 1, 0);       // where depth d starts in the device arrays
    for (int p = 0; p < n_plans; p++)
        for (int d = 0; d < offs[p + 1] - offs[p]; d++) nAt[(size_t)d]++;
    for (int d = 0; d < maxLegs; d++) at[(size_t)d + 1] = at[(size_t)d] + (size_t)nAt[(size_t)d];
    const size_t L = at[(size_t)maxLegs];
    const int n1 = nAt[0];                                // plans with at least one leg
    const int run0 = c->nverts, rib0 = c->nribbons;
    if ((long long)run0 + n1 >= (1 << 24)) return fail(PPGPU_ECAPACITY, "cost_plans_host: open vertices plus plans exceed 2^24-1");
    hipStream_t st = c->stream;
    // ---- stage in: legs, depth-major | start vertex per plan
    const size_t i_s = L * sizeof(ppgpu_wrapper_edge), in_bytes = i_s + (size_t)n1 * sizeof(int);
    // ---- stage out: records | legs costed | stop | child slots (downloaded only when the caller wants them)
    const size_t o_n = L * sizeof(ppgpu_edge_result), o_s = o_n + (size_t)n1 * sizeof(int), o_c = (o_s + (size_t)n1 * sizeof(unsigned) + 127) / 128 * 128,
                 out_bytes = o_c + L * (size_t)stride * 4 * sizeof(double), down_bytes = h_child ? out_bytes : o_c;
    if ((rc = stage_reserve(&c->stage_in, &c->stage_in_cap, in_bytes)) || (rc = stage_reserve(&c->stage_out, &c->stage_out_cap, down_bytes)) ||
        (rc = c->dstage_in.reserve(in_bytes, false, st)) || (rc = c->dstage_out.reserve(out_bytes, false, st)) ||
        (rc = c->verts.reserve((size_t)run0 + n1, true, st)) || (rc = c->ribbons.reserve(((size_t)rib0 + (size_t)n1 * stride) * 4, true, st)) ||
        (rc = c->tgrid.reserve(((size_t)run0 + n1) * c->ng, true, st)))
        return rc;
    char* sin = (char*)c->stage_in;
    ppgpu_wrapper_edge* sw = (ppgpu_wrapper_edge*)sin;
    int* sstart = (int*)(sin + i_s);
    for (int j = 0; j < n1; j++) {
        const int p = order[(size_t)j];
        sstart[j] = h_legs[offs[p]].vertex;
        for (int d = 0; d < offs[p + 1] - offs[p]; d++) {
            ppgpu_wrapper_edge& w = sw[at[(size_t)d] + (size_t)j];
            w = h_legs[offs[p] + d];
            if (d > 0) w.vertex = run0 + j;               // the plan's running vertex
        }
    }
    HIP_TRY(hipMemcpyAsync(c->dstage_in.p, sin, in_bytes, hipMemcpyHostToDevice, st));
    // legs costed = 0, stop = 0 (running), child slots zero beyond each list as on the leg-by-leg route
    HIP_TRY(hipMemsetAsync(c->dstage_out.p + o_n, 0, out_bytes - o_n, st));
    ppgpu_wrapper_edge* d_legs = (ppgpu_wrapper_edge*)c->dstage_in.p;
    ppgpu_edge_result* d_results = (ppgpu_edge_result*)c->dstage_out.p;
    double* d_child = (double*)(c->dstage_out.p + o_c);
    for (int d = 0; d < maxLegs; d++) {
        const int nNow = nAt[(size_t)d], nNext = d + 1 < maxLegs ? nAt[(size_t)d + 1] : 0;
        PPParams p = list_params(c, nNow, nullptr, d_legs + at[(size_t)d], d_results + at[(size_t)d], d_child + at[(size_t)d] * (size_t)stride * 4, stride);
        p.nverts = run0 + n1;                             // the running vertices count as open ones
        c->arc_stops_stale = true;                        // (given curves form no stop classes; the vertices past run0 change under the table all the same)
        if ((rc = launch_cost(c, p))) return rc;
        PPChainArgs a;
        a.results = p.out; a.child = p.child; a.stride = stride;
        a.next = nNext > 0 ? d_legs + at[(size_t)d + 1] : nullptr;
        a.n_now = nNow; a.n_next = nNext; a.depth = d;
        a.start_vertex = (const int*)(c->dstage_in.p + i_s);
        a.verts = c->verts.p; a.run0 = run0;
        a.ribbons = c->ribbons.p; a.rib0 = rib0;
        a.costed = (int*)(c->dstage_out.p + o_n); a.stop = (unsigned*)(c->dstage_out.p + o_s);
        hipLaunchKernelGGL(pp_k_chain_advance, dim3((unsigned)nNow), dim3(64), 0, st, a);
        if (nNext > 0)
            hipLaunchKernelGGL(pp_k_time_grid, dim3((unsigned)nNext), dim3(64), 0, st, c->verts.p + run0, nNext, c->cfg.start_state_time,
                               c->cfg.collision_checking_increment, c->cfg.max_speed, c->ng, c->tgrid.p + (size_t)run0 * c->ng);
        HIP_TRY(hipGetLastError());
    }
    char* sout = (char*)c->stage_out;
    HIP_TRY(hipMemcpyAsync(sout, c->dstage_out.p, down_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const ppgpu_edge_result* sr = (const ppgpu_edge_result*)sout;
    const int* sn = (const int*)(sout + o_n);
    const unsigned* ss = (const unsigned*)(sout + o_s);
    const double* sc = (const double*)(sout + o_c);
    const size_t slot = (size_t)stride * 4;
    for (int j = 0; j < n1; j++) {
        const int q = order[(size_t)j];
        h_costed[q] = sn[j];
        h_stop[q] = ss[j];
        for (int d = 0; d < sn[j] && d < offs[q + 1] - offs[q]; d++) {   // (the slots of legs that were not costed stay as the caller left them)
            const size_t from = at[(size_t)d] + (size_t)j, to = (size_t)(offs[q] + d);
            h_results[to] = sr[from];
            if (h_child) std::memcpy(h_child + to * slot, sc + from * slot, slot * sizeof(double));
        }
    }
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ incumbent
int ppgpu_best_edge(ppgpu_ctx* c, int64_t n, const ppgpu_edge_result* d_results, int32_t goal_only, uint64_t base,
                    uint64_t* d_key2) {
    if (!c) return fail(PPGPU_EINVAL, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (n < 0 || !d_key2 || (n > 0 && !d_results)) return fail(PPGPU_EINVAL, "best_edge: bad arguments");
    int nparts = (int)((n + 255) / 256);
    if (nparts > 1024) nparts = 1024;
    if (nparts < 1) nparts = 1;
    int rc = c->partial.reserve((size_t)nparts * 2, false, c->stream);
    if (rc) return rc;
    hipLaunchKernelGGL(pp_k_best_stage1, dim3(nparts), dim3(256), 0, c->stream, d_results, (long long)n, goal_only,
                       (unsigned long long)base, c->partial.p);
    hipLaunchKernelGGL(pp_k_best_stage2, dim3(1), dim3(256), 0, c->stream, c->partial.p, nparts, (unsigned long long*)d_key2);
    HIP_TRY(hipGetLastError());
    return PPGPU_OK;
}

// Lexicographic min of n (f bits, index) pairs already resident on the device (e.g. the output of an
// all-gather issued by the caller's own communicator).
int ppgpu_key_min(ppgpu_ctx* c, int32_t n, const uint64_t* d_keys, uint64_t* d_key2) {
    if (!c || !d_keys || !d_key2 || n <= 0) return fail(PPGPU_EINVAL, "key_min: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(pp_k_key_min_n, dim3(1), dim3(64), 0, c->stream, (const unsigned long long*)d_keys, n, (unsigned long long*)d_key2);
    HIP_TRY(hipGetLastError());
    return PPGPU_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------ RCCL (incumbent exchange between ranks)
// RCCL is loaded lazily so that single-GPU users (and the CPU-only build check) do not need it.  The NCCL ABI is used through
// dlsym: ncclUniqueId = 128 opaque bytes passed by value, ncclUint64 == 5, ncclSuccess == 0.
#include <dlfcn.h>
namespace {
struct PPNcclId { char internal[PPGPU_COMM_ID_BYTES]; };
struct Rccl {
    int (*get_unique_id)(PPNcclId*) = nullptr;
    int (*comm_init_rank)(void**, int, PPNcclId, int) = nullptr;
    int (*comm_init_all)(void**, int, const int*) = nullptr;
    int (*comm_count)(void*, int*) = nullptr;
    int (*comm_user_rank)(void*, int*) = nullptr;
    int (*comm_destroy)(void*) = nullptr;
    int (*comm_abort)(void*) = nullptr;
    int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*error_string)(int) = nullptr;
    std::string error;
    bool ok = false;
};
// resolved once, published only when complete (contexts may live on several threads)
const Rccl& rccl_table() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { r.error = std::string("cannot load librccl.so: ") + dlerror(); return; }
        r.get_unique_id = (decltype(r.get_unique_id))dlsym(lib, "ncclGetUniqueId");
        r.comm_init_rank = (decltype(r.comm_init_rank))dlsym(lib, "ncclCommInitRank");
        r.comm_init_all = (decltype(r.comm_init_all))dlsym(lib, "ncclCommInitAll");
        r.comm_count = (decltype(r.comm_count))dlsym(lib, "ncclCommCount");
        r.comm_user_rank = (decltype(r.comm_user_rank))dlsym(lib, "ncclCommUserRank");
        r.comm_destroy = (decltype(r.comm_destroy))dlsym(lib, "ncclCommDestroy");
        r.comm_abort = (decltype(r.comm_abort))dlsym(lib, "ncclCommAbort");
        r.all_gather = (decltype(r.all_gather))dlsym(lib, "ncclAllGather");
        r.error_string = (decltype(r.error_string))dlsym(lib, "ncclGetErrorString");
        if (!r.get_unique_id || !r.comm_init_rank || !r.comm_init_all || !r.comm_count || !r.comm_user_rank || !r.comm_destroy || !r.all_gather) {
            r.error = "librccl.so lacks one of ncclGetUniqueId/CommInitRank/CommInitAll/CommCount/CommUserRank/CommDestroy/AllGather";
            return;
        }
        r.ok = true;
    });
    return r;
}
int rccl_fail(const Rccl& r, const char* what, int code) {
    return fail(PPGPU_ERCCL, std::string(what) + " failed: " + (r.error_string ? r.error_string(code) : "") + " (ncclResult " + std::to_string(code) + ")");
}
}  // namespace

extern "C" int ppgpu_comm_unique_id(uint8_t* id128) {
    if (!id128) return fail(PPGPU_EINVAL, "comm_unique_id: null argument");
    const Rccl& r = rccl_table();
    if (!r.ok) return fail(PPGPU_ERCCL, r.error);
    PPNcclId id;
    std::memset(&id, 0, sizeof(id));
    const int rc = r.get_unique_id(&id);
    if (rc != 0) return rccl_fail(r, "ncclGetUniqueId", rc);
    std::memcpy(id128, id.internal, PPGPU_COMM_ID_BYTES);
    return PPGPU_OK;
}

extern "C" int ppgpu_comm_init_rank(ppgpu_ctx* c, int32_t world, int32_t rank, const uint8_t* id128) {
    if (!c || !id128) return fail(PPGPU_EINVAL, "comm_init_rank: null argument");
    if (world <= 0 || rank < 0 || rank >= world) return fail(PPGPU_EINVAL, "comm_init_rank: rank must lie in [0, world)");
    if (c->comm) return fail(PPGPU_ESTATE, "comm_init_rank: the handle already has a communicator (ppgpu_comm_destroy first)");
    const Rccl& r = rccl_table();
    if (!r.ok) return fail(PPGPU_ERCCL, r.error);
    HIP_TRY(hipSetDevice(c->device));
    PPNcclId id;
    std::memcpy(id.internal, id128, PPGPU_COMM_ID_BYTES);
    // the gather buffer first: nothing can fail once the communicator exists
    int rc2 = c->gather.reserve((size_t)world * 2, false, c->stream);
    if (rc2) return rc2;
    void* comm = nullptr;
    const int rc = r.comm_init_rank(&comm, world, id, rank);
    if (rc != 0 || !comm) return rccl_fail(r, "ncclCommInitRank", rc);
    c->comm = comm;
    return PPGPU_OK;
}

extern "C" int ppgpu_comm_init_all(ppgpu_ctx** ctxs, int32_t n) {
    if (!ctxs || n <= 0) return fail(PPGPU_EINVAL, "comm_init_all: bad arguments");
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return fail(PPGPU_EINVAL, "comm_init_all: null context");
        if (ctxs[i]->comm) return fail(PPGPU_ESTATE, "comm_init_all: a handle already has a communicator");
        devs[(size_t)i] = ctxs[i]->device;
        for (int j = 0; j < i; j++)
            if (devs[(size_t)j] == devs[(size_t)i]) return fail(PPGPU_EINVAL, "comm_init_all: RCCL takes one rank per device; two handles share device " + std::to_string(devs[(size_t)i]));
    }
    const Rccl& r = rccl_table();
    if (!r.ok) return fail(PPGPU_ERCCL, r.error);
    // every handle's gather buffer first, so that the handles end up with a communicator each or none at all
    for (int i = 0; i < n; i++) {
        HIP_TRY(hipSetDevice(ctxs[i]->device));
        int rc2 = ctxs[i]->gather.reserve((size_t)n * 2, false, ctxs[i]->stream);
        if (rc2) return rc2;
    }
    std::vector<void*> comms((size_t)n, nullptr);
    const int rc = r.comm_init_all(comms.data(), n, devs.data());
    if (rc != 0) {
        for (void* cm : comms) if (cm) (void)r.comm_destroy(cm);
        return rccl_fail(r, "ncclCommInitAll", rc);
    }
    for (int i = 0; i < n; i++) ctxs[i]->comm = comms[(size_t)i];
    return PPGPU_OK;
}

extern "C" int ppgpu_comm_info(ppgpu_ctx* c, int32_t* world, int32_t* rank) {
    if (!c) return fail(PPGPU_EINVAL, "comm_info: null context");
    if (!c->comm) return fail(PPGPU_ESTATE, "comm_info: the handle has no communicator");
    const Rccl& r = rccl_table();
    if (!r.ok) return fail(PPGPU_ERCCL, r.error);
    int w = 0, k = 0, rc;
    if ((rc = r.comm_count(c->comm, &w)) != 0) return rccl_fail(r, "ncclCommCount", rc);
    if ((rc = r.comm_user_rank(c->comm, &k)) != 0) return rccl_fail(r, "ncclCommUserRank", rc);
    if (world) *world = w;
    if (rank) *rank = k;
    return PPGPU_OK;
}

extern "C" int ppgpu_comm_destroy(ppgpu_ctx* c) {
    if (!c) return fail(PPGPU_EINVAL, "comm_destroy: null context");
    if (!c->comm) return PPGPU_OK;
    const Rccl& r = rccl_table();
    if (!r.ok) return fail(PPGPU_ERCCL, r.error);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    const int rc = r.comm_destroy(c->comm);
    c->comm = nullptr;
    if (rc != 0) return rccl_fail(r, "ncclCommDestroy", rc);
    return PPGPU_OK;
}

// ncclCommAbort: frees the communicator WITHOUT waiting for its outstanding collectives — the way out for the ranks that entered a
// collective a failed rank never joined.  May be called from another host thread than the one stuck in the handle's stream.
extern "C" int ppgpu_comm_abort(ppgpu_ctx* c) {
    if (!c) return fail(PPGPU_EINVAL, "comm_abort: null context");
    void* comm = c->comm;
    if (!comm) return PPGPU_OK;
    const Rccl& r = rccl_table();
    if (!r.ok) return fail(PPGPU_ERCCL, r.error);
    c->comm = nullptr;
    const int rc = r.comm_abort ? r.comm_abort(comm) : r.comm_destroy(comm);
    if (rc != 0) return rccl_fail(r, "ncclCommAbort", rc);
    return PPGPU_OK;
}

// ------------------------------------------------------------------------------ records home on a copy engine
// hipMemcpyAsync from device memory into pinned host memory runs as a blit KERNEL on this stack (__amd_rocclr_copyBuffer in every
// rocprofv3 kernel trace of bench.py's end-to-end loops, with HSA_ENABLE_SDMA=1 and with GPU_BLIT_ENGINE_TYPE=2 alike): 30 MB of
// records take 0.62 ms of wave slots beside fp64-bound kernels.  hsa_amd_memory_async_copy puts the same copy on an SDMA engine.  The
// HSA runtime is the one HIP itself runs on (same soname: the loader hands back the instance already in the process).
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
namespace {
struct HsaApi {
    decltype(&hsa_iterate_agents) iterate_agents = nullptr;
    decltype(&hsa_agent_get_info) agent_get_info = nullptr;
    decltype(&hsa_signal_create) signal_create = nullptr;
    decltype(&hsa_signal_destroy) signal_destroy = nullptr;
    decltype(&hsa_signal_store_relaxed) signal_store_relaxed = nullptr;
    decltype(&hsa_signal_wait_scacquire) signal_wait_scacquire = nullptr;
    decltype(&hsa_amd_memory_async_copy) memory_async_copy = nullptr;
    decltype(&hsa_amd_pointer_info) pointer_info = nullptr;
    std::string error;
    bool ok = false;
};
const HsaApi& hsa_api() {
    static HsaApi a;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = dlopen("libhsa-runtime64.so.1", RTLD_NOW);
        if (!lib) lib = dlopen("libhsa-runtime64.so", RTLD_NOW);
        if (!lib) { a.error = std::string("cannot load libhsa-runtime64.so.1: ") + dlerror(); return; }
        a.iterate_agents = (decltype(a.iterate_agents))dlsym(lib, "hsa_iterate_agents");
        a.agent_get_info = (decltype(a.agent_get_info))dlsym(lib, "hsa_agent_get_info");
        a.signal_create = (decltype(a.signal_create))dlsym(lib, "hsa_signal_create");
        a.signal_destroy = (decltype(a.signal_destroy))dlsym(lib, "hsa_signal_destroy");
        a.signal_store_relaxed = (decltype(a.signal_store_relaxed))dlsym(lib, "hsa_signal_store_relaxed");
        a.signal_wait_scacquire = (decltype(a.signal_wait_scacquire))dlsym(lib, "hsa_signal_wait_scacquire");
        a.memory_async_copy = (decltype(a.memory_async_copy))dlsym(lib, "hsa_amd_memory_async_copy");
        a.pointer_info = (decltype(a.pointer_info))dlsym(lib, "hsa_amd_pointer_info");
        if (!a.iterate_agents || !a.agent_get_info || !a.signal_create || !a.signal_destroy || !a.signal_store_relaxed || !a.signal_wait_scacquire || !a.memory_async_copy || !a.pointer_info) {
            a.error = "libhsa-runtime64 lacks one of the entry points ppgpu_copy_engine_read needs";
            return;
        }
        a.ok = true;
    });
    return a;
}
struct AgentScan { const HsaApi* api; int want_gpu; int seen_gpu; hsa_agent_t gpu, cpu; bool have_gpu, have_cpu; };
hsa_status_t scan_agent(hsa_agent_t agent, void* data) {
    AgentScan* s = (AgentScan*)data;
    hsa_device_type_t type;
    if (s->api->agent_get_info(agent, HSA_AGENT_INFO_DEVICE, &type) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (type == HSA_DEVICE_TYPE_CPU && !s->have_cpu) { s->cpu = agent; s->have_cpu = true; }
    if (type == HSA_DEVICE_TYPE_GPU) {
        if (s->seen_gpu == s->want_gpu) { s->gpu = agent; s->have_gpu = true; }
        s->seen_gpu++;
    }
    return HSA_STATUS_SUCCESS;
}
}  // namespace

static void ppgpu_copy_engine_release(ppgpu_ctx* c) {
    if (!c->hsa_signal) return;
    hsa_signal_t sig; sig.handle = c->hsa_signal;
    (void)hsa_api().signal_destroy(sig);
    c->hsa_signal = 0;
}

extern "C" int ppgpu_copy_engine_wait(ppgpu_ctx* c) {
    if (!c) return fail(PPGPU_EINVAL, "copy_engine_wait: null context");
    if (!c->copy_pending) return PPGPU_OK;
    const HsaApi& a = hsa_api();
    hsa_signal_t sig; sig.handle = c->hsa_signal;
    // (the signal starts at 1; the copy engine takes it to 0, or below on an error)
    const hsa_signal_value_t v = a.signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
    c->copy_pending = false;
    if (v < 0) return fail(PPGPU_EHIP, "copy_engine_wait: the copy engine reported an error");
    return PPGPU_OK;
}

extern "C" int ppgpu_copy_engine_read(ppgpu_ctx* c, void* h_pinned_dst, const void* d_src, uint64_t bytes) {
    if (!c || !h_pinned_dst || !d_src || bytes == 0) return fail(PPGPU_EINVAL, "copy_engine_read: bad arguments");
    const HsaApi& a = hsa_api();
    if (!a.ok) return fail(PPGPU_EHIP, a.error);
    int rc;
    if (c->copy_pending && (rc = ppgpu_copy_engine_wait(c))) return rc;          // one copy in flight per handle
    if (!c->hsa_signal) {
        AgentScan s{&a, c->device, 0, {}, {}, false, false};
        if (a.iterate_agents(scan_agent, &s) != HSA_STATUS_SUCCESS || !s.have_cpu)
            return fail(PPGPU_EHIP, "copy_engine_read: cannot find the HSA agent of the host");
        // the GPU agent is the one that OWNS the source allocation (a HIP device ordinal is not an index into HSA's agent list once
        // HIP_VISIBLE_DEVICES reorders or masks devices)
        hsa_amd_pointer_info_t info;
        std::memset(&info, 0, sizeof(info));
        info.size = sizeof(info);
        if (a.pointer_info(d_src, &info, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS || info.type == HSA_EXT_POINTER_TYPE_UNKNOWN)
            return fail(PPGPU_EHIP, "copy_engine_read: the source is not a device allocation HSA knows");
        hsa_device_type_t owner_type;
        if (a.agent_get_info(info.agentOwner, HSA_AGENT_INFO_DEVICE, &owner_type) != HSA_STATUS_SUCCESS || owner_type != HSA_DEVICE_TYPE_GPU)
            return fail(PPGPU_EHIP, "copy_engine_read: the source allocation is not owned by a GPU agent");
        s.gpu = info.agentOwner; s.have_gpu = true;
        hsa_signal_t sig;
        if (a.signal_create(1, 0, nullptr, &sig) != HSA_STATUS_SUCCESS) return fail(PPGPU_EHIP, "copy_engine_read: hsa_signal_create failed");
        c->hsa_gpu = s.gpu.handle; c->hsa_cpu = s.cpu.handle; c->hsa_signal = sig.handle;
    }
    hsa_signal_t sig; sig.handle = c->hsa_signal;
    hsa_agent_t gpu, cpu; gpu.handle = c->hsa_gpu; cpu.handle = c->hsa_cpu;
    a.signal_store_relaxed(sig, 1);
    const hsa_status_t st = a.memory_async_copy(h_pinned_dst, cpu, d_src, gpu, (size_t)bytes, 0, nullptr, sig);
    if (st != HSA_STATUS_SUCCESS) return fail(PPGPU_EHIP, "copy_engine_read: hsa_amd_memory_async_copy failed (status " + std::to_string((int)st) + "): is the destination pinned host memory?");
    c->copy_pending = true;
    return PPGPU_OK;
}

extern "C" int ppgpu_allreduce_best(ppgpu_ctx* c, void* comm, uint64_t* d_key2) {
    if (!c || !d_key2) return fail(PPGPU_EINVAL, "allreduce_best: null argument");
    if (!comm) comm = c->comm;
    if (!comm) return fail(PPGPU_ESTATE, "allreduce_best: no communicator (pass one, or ppgpu_comm_init_rank / ppgpu_comm_init_all first)");
    HIP_TRY(hipSetDevice(c->device));
    const Rccl& r = rccl_table();
    if (!r.ok) return fail(PPGPU_ERCCL, r.error);
    int world = 0, rc;
    if ((rc = r.comm_count(comm, &world)) != 0 || world <= 0) return rccl_fail(r, "ncclCommCount", rc);
    int rc2 = c->gather.reserve((size_t)world * 2, false, c->stream);
    if (rc2) return rc2;
    // one collective: 16 bytes per rank over xGMI; ncclUint64 == 5 in the NCCL ABI
    if ((rc = r.all_gather(d_key2, c->gather.p, 2, 5, comm, c->stream)) != 0) return rccl_fail(r, "ncclAllGather", rc);
    hipLaunchKernelGGL(pp_k_key_min_n, dim3(1), dim3(64), 0, c->stream, c->gather.p, world, (unsigned long long*)d_key2);
    HIP_TRY(hipGetLastError());
    return PPGPU_OK;
}
