/*
 * ppgpu.h — C ABI of the MI355X (gfx950) implementation of the ASV planner's
 * per-iteration hot path: state sampling -> Dubins edge generation -> per-edge
 * cost evaluation (occupancy grid + dynamic obstacles + ribbon coverage + heuristic)
 * -> incumbent min-reduce.
 *
 * The reference has no FFI layer; its seam is the C++ virtual
 *   Planner::Stats Planner::plan(const RibbonManager&, const State&, PlannerConfig,
 *                                const DubinsPlan&, double timeRemaining)
 *   (/root/reference/path_planner/src/planner/Planner.h:50-51, called from
 *    path_planner/src/executive/executive.cpp:189-190),
 * with the arithmetic living in non-virtual members underneath it.  Each entry
 * point below names the reference function(s) whose work it replaces; the C++
 * host mirror of the reference classes (path_planner_amd/host) is built on
 * nothing but this header, and INTEGRATION.md shows the binding a maintainer
 * of the reference would add.
 *
 * Conventions
 *   - every function returns PPGPU_OK (0) or a negative PPGPU_E* code and
 *     records a message retrievable with ppgpu_last_error(); the C++ host turns
 *     a non-zero code into std::runtime_error so Executive::planLoop's
 *     try/catch (executive.cpp:191-200) behaves as it does today;
 *   - plain pointers and sizes only; `h_` parameters are host memory, `d_`
 *     parameters are device (HBM) memory owned by the caller;
 *   - all floating point is IEEE double, exactly as in the reference
 *     (path_planner_common/include/path_planner_common/State.h:201-202);
 *   - nothing here falls back to the CPU: if no gfx950 device/code object is
 *     available ppgpu_create fails.
 */
#ifndef PATH_PLANNER_AMD_PPGPU_H
#define PATH_PLANNER_AMD_PPGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPGPU_OK          0
#define PPGPU_EINVAL     (-1)  /* bad argument / shape mismatch                      */
#define PPGPU_EHIP       (-2)  /* a HIP runtime call failed (message has the detail) */
#define PPGPU_ENODEV     (-3)  /* no usable gfx950 device                            */
#define PPGPU_ESTATE     (-4)  /* call order violated (e.g. cost before set_config)  */
#define PPGPU_ECAPACITY  (-5)  /* a fixed device-side capacity was exceeded          */
#define PPGPU_ERCCL      (-6)  /* an RCCL call failed                                */

typedef struct ppgpu_ctx ppgpu_ctx;

/* RibbonManager::Heuristic, same order
 * (path_planner/src/planner/utilities/RibbonManager.h:20-26). */
enum {
    PPGPU_H_MAX_DISTANCE = 0,
    PPGPU_H_TSP_POINT_ALL = 1,
    PPGPU_H_TSP_POINT_K = 2,
    PPGPU_H_TSP_DUBINS_ALL = 3,
    PPGPU_H_TSP_DUBINS_K = 4
};

/* DynamicObstaclesManager implementations behind PlannerConfig::obstaclesManager()
 * (path_planner/src/planner/PlannerConfig.h:98-104). */
enum {
    PPGPU_OBST_NONE = 0,    /* base class: collisionExists == 0 (DynamicObstaclesManager.h:23) */
    PPGPU_OBST_BINARY = 1,  /* BinaryDynamicObstaclesManager.cpp:4-22                           */
    PPGPU_OBST_GAUSSIAN = 2 /* GaussianDynamicObstaclesManager.cpp:3-13 (sum of bivariate normal pdfs, floor 1e-5) */
};

/* The scalars of PlannerConfig (PlannerConfig.h:179-207) plus the process-global
 * ribbon half-width (Ribbon.h:16, Ribbon.cpp:4), the two Edge constants
 * (Edge.h:151-152) and the RibbonManager heuristic settings
 * (RibbonManager.h:184-190).  Defaults are the reference's. */
typedef struct ppgpu_config {
    double max_speed;                   /* 2.5  */
    double slow_speed;                  /* 0.5 ; <= 0 means "same as max" (PlannerConfig.h:168-171) */
    double turning_radius;              /* 8    */
    double coverage_turning_radius;     /* 16   */
    double time_horizon;                /* 30   */
    double time_minimum;                /* 5    */
    double collision_checking_increment;/* 0.05 */
    double start_state_time;            /* PlannerConfig::startStateTime() */
    double ribbon_width;                /* 1.5  Ribbon::RibbonWidth (half width) */
    double collision_penalty_factor;    /* 600  Edge::collisionPenaltyFactor()   */
    double time_penalty_factor;         /* 1    Edge::timePenaltyFactor()        */
    double heuristic_turning_radius;    /* RibbonManager::m_TurningRadius (Dubins-TSP heuristics only) */
    int32_t heuristic;                  /* PPGPU_H_* */
    int32_t tsp_k;                      /* RibbonManager::m_K */
    int32_t branching_factor;           /* 9 */
    int32_t reserved;
} ppgpu_config;

/* One open vertex = what Edge::computeTrueCost reads from its start vertex
 * (Edge.cpp:88,98-99; Vertex.h:180-187): State, g, and the vertex's private
 * RibbonManager (list of ribbons + coverageCompletedTime). 64 bytes. */
typedef struct ppgpu_vertex {
    double x, y, heading, speed, time;  /* State (State.h:201-202)                        */
    double g;                           /* Vertex::currentCost()                          */
    double coverage_completed_time;     /* RibbonManager::coverageCompletedTime(), -1 unset */
    int32_t ribbon_offset;              /* first ribbon of this vertex in the ribbon pool */
    int32_t ribbon_count;
} ppgpu_vertex;

/* Bits of ppgpu_edge_result.flags */
#define PPGPU_F_INFEASIBLE   0x01u /* Edge::infeasible()                                          */
#define PPGPU_F_THROWS       0x02u /* the reference would throw out of computeTrueCost here
                                      (DubinsWrapper::sample on an uninitialised / out-of-range
                                      wrapper, Edge.cpp:178 / DubinsWrapper.cpp:29-35)            */
#define PPGPU_F_RIBBON_OVF   0x04u /* child ribbon list exceeded ribbon_stride or 64, or the heuristic's enumeration limit
                                      * (8 ribbons for the brute-force TSP heuristics; 12 for TspPointRobotNoSplitKRibbons
                                      * while its tree has fewer than 2^21 prefixes): h = 0, f = g, never silent */
#define PPGPU_F_RIBBON_LOST  0x40u /* the child's list outgrew the device's 64 ribbons per vertex while the edge was swept: pieces
                                      * were DROPPED, so the record's coverage state is not the reference's (which has no limit) and
                                      * must not be searched on.  Always together with PPGPU_F_RIBBON_OVF.  Without this bit,
                                      * PPGPU_F_RIBBON_OVF on a record whose child count fits ribbon_stride means only that the
                                      * heuristic was not enumerated: the list itself came back whole */
#define PPGPU_F_DUBINS_ERR   0x08u /* dubins_path_sample failed twice (DubinsWrapper.cpp:43-45)    */
#define PPGPU_F_GOAL         0x10u /* SamplingBasedPlanner::goalCondition(child)                   */
#define PPGPU_F_DONE         0x20u /* child->done()                                                */

/* What Vertex::connect + Edge::computeApproxCost + Edge::computeTrueCost leave
 * behind for one edge (Edge.cpp:68-206, Vertex.cpp:49-64,97-104). 128 bytes, so a
 * wavefront writes one record as a single 128-byte transaction. */
typedef struct ppgpu_edge_result {
    uint32_t flags;            /* PPGPU_F_*                                              */
    uint32_t info;             /* bits 0-7 DubinsPathType, bits 8-15 child ribbon count,
                                  bits 16-31 number of sweep steps executed              */
    double true_cost;          /* Edge::trueCost()                                       */
    double collision_penalty;  /* Edge::getSavedCollisionPenalty()                       */
    double approx_cost;        /* Edge::approxCost()                                     */
    double end_x, end_y, end_heading, end_speed, end_time; /* child State (Edge.cpp:177-178) */
    double g, h, f;            /* child currentCost, approxToGo, f                       */
    double coverage_completed_time; /* child RibbonManager::coverageCompletedTime()      */
    double param[3];           /* DubinsPath::param of the edge's curve                  */
} ppgpu_edge_result;

/* Edge descriptor for the list form of ppgpu_cost_edges: which open vertex,
 * which target state, which (radius, speed) configuration
 * (SamplingBasedPlanner.cpp:58-63,69-79,134-148). */
#define PPGPU_EDGE_COVERAGE 0x1u /* use coverage_turning_radius, coverageAllowed = true */
#define PPGPU_EDGE_SLOW     0x2u /* end state's speed = slow_speed instead of max_speed */
static inline uint64_t ppgpu_edge_pack(uint32_t vertex, uint32_t target, uint32_t cfg) {
    return ((uint64_t)(cfg & 0xffu) << 56) | ((uint64_t)(vertex & 0xffffffu) << 32) | (uint64_t)target;
}

/* An edge whose curve already exists: Vertex::connect(start, DubinsWrapper, coverageAllowed)
 * (Vertex.cpp:28-36) — how AStarPlanner::plan re-costs the previous plan (AStarPlanner.cpp:46-59).
 * Fields are DubinsWrapper's (DubinsWrapper.h:118-120) as serialised by NodeBase.h:201-220. */
typedef struct ppgpu_wrapper_edge {
    int32_t vertex;            /* open vertex the edge starts from                        */
    int32_t coverage_allowed;  /* p.getRho() == config.coverageTurningRadius()            */
    double qi[3];              /* DubinsPath::qi (x, y, yaw)                              */
    double param[3];           /* DubinsPath::param                                       */
    double rho;                /* DubinsPath::rho                                         */
    int32_t type;              /* DubinsPathType                                          */
    int32_t reserved;
    double speed;              /* DubinsWrapper::getSpeed()                               */
    double start_time;         /* start time of the curve (m_StartTime); later than the
                                * vertex's first step: that sample throws, the edge is
                                * infeasible with 0 steps (Edge.cpp:126-133)             */
    double end_time;           /* getEndTime(), possibly truncated by updateEndTime()     */
} ppgpu_wrapper_edge;

/* ------------------------------------------------------------------ lifecycle */

/* Process-level handle: device context, stream, persistent buffers.  The reference
 * constructs a new planner every cycle (executive.cpp:85-90); the handle outlives it. */
int ppgpu_create(int device, ppgpu_ctx** out);
int ppgpu_destroy(ppgpu_ctx* ctx);
const char* ppgpu_last_error(void);
/* Launch on a caller-owned hipStream_t (NULL = the handle's own stream). */
int ppgpu_set_stream(ppgpu_ctx* ctx, void* hip_stream);
int ppgpu_synchronize(ppgpu_ctx* ctx);
/* Size the buffers that grow with the sample set — the sample store, the sampler's scratch, the length table and candidate lists
 * of ppgpu_expand_host for batches of up to max_vertices open vertices — for max_samples samples now, so that an anytime planner
 * that doubles its sample set every iteration (AStarPlanner.cpp:101-102) never meets a device allocation inside its time budget.
 * Optional: without it the buffers grow on demand (powers of two) and stay for the life of the handle.  8 million samples and
 * 16 vertices take 2.3 GB of the 288 GB. */
int ppgpu_reserve_samples(ppgpu_ctx* ctx, int64_t max_samples, int32_t max_vertices);
/* How many times the library has grown a device or pinned-host buffer in this process so far, and the wall time those
 * allocations took.  A caller with a time contract (Planner.h:42: plan() returns before timeRemaining) reads it before and after
 * a cycle: a growth inside the budget costs milliseconds and is what ppgpu_reserve_samples is there to avoid.  Either may be NULL. */
int ppgpu_growth_stats(ppgpu_ctx* ctx, uint64_t* count, double* seconds);
/* Measurement aid: with timing on, every costing launch records HIP events on the handle's stream between its kernels;
 * ppgpu_last_timing waits for the last launch and returns, in milliseconds: ms_solve = pp_k_solve_edges; ms_pose = the pose
 * sweep with its chunk-skip planner (pp_k_plan_skips + pp_k_pose_sweep); ms_cover = pp_k_cover_sweep alone; ms_heuristic =
 * everything else of the launch (pp_k_approach_events, pp_k_deferred_list, the heuristic kernels).  The four add up to the
 * launch.  For a launch that ran as several workspace slices each figure is summed over the slices.  On small launches, with
 * the point heuristics and the binary obstacle model, the cover sweep's wavefront computes the edge's heuristic itself.
 * The events cost a few microseconds per launch: leave timing off in production.
 * ppgpu_past_timing reads an earlier launch: back = 0 is the last one, up to 7 launches back (a ring of event sets), so a
 * caller can time several launches in a row without a host wait between them and collect the durations afterwards. */
int ppgpu_enable_timing(ppgpu_ctx* ctx, int32_t on);
int ppgpu_last_timing(ppgpu_ctx* ctx, double* ms_solve, double* ms_pose, double* ms_cover, double* ms_heuristic);
int ppgpu_past_timing(ppgpu_ctx* ctx, int32_t back, double* ms_solve, double* ms_pose, double* ms_cover, double* ms_heuristic);
/* Measurement aid: how many edges of the last costing launch pp_k_cover_sweep visited.  On large launches the approach prepass
 * finishes the edges whose coverage state machine has nothing to do and hands the cover sweep a packed list of the others; on
 * small launches it is every edge.  (Sliced launches: exact with timing on, the last slice's share otherwise.)  Waits for the launch. */
int ppgpu_last_cover_edges(ppgpu_ctx* ctx, int64_t* n_edges);
/* Shared sweeps.  On large launches of solved edges (the dense and the list form, not wrapper edges) the edges whose whole horizon
 * lies on the first arc of their curve fall into classes (open vertex, configuration, direction of that arc) whose members have one
 * and the same sweep: one member of each class is swept and the others take its results, their own DubinsPathType, approx_cost and
 * param[] apart.  The records and child ribbons are the same bytes either way.  PPGPU_SHARE_SWEEPS=0 in the environment of
 * ppgpu_create switches it off.  ppgpu_last_shared_edges: how many edges of the last costing launch took another edge's results
 * (0 with the switch off and on small launches).  Waits for the launch; reads one word per edge back, a measurement aid. */
int ppgpu_last_shared_edges(ppgpu_ctx* ctx, int64_t* n_edges);
/* The sweep list.  A launch with shared sweeps packs the positions of the edges that are swept at all (solved, neither malformed nor
 * co-located, not a class member that takes its head's results) into a list on the device, and the chunk-skip planner, the pose
 * sweep and the approach prepass walk that list instead of every edge (PPGPU_APPROACH_LIST=0: the approach prepass does not).  The records and child ribbons are the same bytes either way.  PPGPU_SWEEP_LIST=0 in
 * the environment of ppgpu_create switches it off.  ppgpu_last_swept_edges: the entries of that list, summed over the slices of the
 * last costing launch; every edge of the launch where it had no list.  With shared tracks (below) the number includes the edges
 * that took their track from a head: it stays "edges - shared - unsolved".  Waits for the launch; a measurement aid. */
int ppgpu_last_swept_edges(ppgpu_ctx* ctx, int64_t* n_edges);
/* Shared tracks.  The first arc of a curve depends on the open vertex, the radius, the speed and the turn direction alone, so all
 * edges of one (open vertex, configuration, direction) sample the same poses while they are on it.  Where that arc crosses a
 * blocked cell of the grid at step kb of the vertex's collision-check time row, every edge of the class that is still on its first
 * arc at that step stops there, with the same track (hits, heading bits, stop) up to it.  A launch with a sweep list walks each
 * class's arc once per set of vertices, grid, keep-out limit and configuration (pp_k_arc_stops, in front of the first such launch
 * after any of them changed), and per class and workspace slice ONE such edge, the head, goes through the chunk-skip planner and the
 * pose sweep; the others, the stop members, get a copy of its track and are costed from there like any swept edge: their end state,
 * g, h and ribbons are their own.  The records and child ribbons are the same bytes either way.  Given curves, the Gaussian obstacle
 * model, launches without a grid or without a sweep list and the traces' own solves form no stop classes.  PPGPU_SHARE_TRACKS=0 in
 * the environment of ppgpu_create switches it off: a launch then builds the lists and runs the kernels it ran before there were stop
 * classes.
 * ppgpu_last_stop_members: how many edges of the last costing launch took their track from a head, summed over its slices (0 with
 * the switch off).  A stop member is not a shared edge (ppgpu_last_shared_edges does not count it) and it is a swept one:
 * ppgpu_last_swept_edges, "edges - shared - unsolved", counts it although the planner and the pose sweep did not walk it.  Waits for
 * the launch; a measurement aid. */
int ppgpu_last_stop_members(ppgpu_ctx* ctx, int64_t* n_edges);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds pp_k_arc_stops took the last time a costing launch queued
 * it (HIP events around the kernel alone).  PPGPU_ESTATE when none was timed since timing was switched on. */
int ppgpu_last_arc_stops_timing(ppgpu_ctx* ctx, double* ms_arc_stops);
/* How the last costing launch was cut: the number of workspace slices it ran as, and the edges of the last one (tests of sliced
 * launches check that they are what they meant to be).  Does not wait. */
int ppgpu_last_slices(ppgpu_ctx* ctx, int64_t* n_slices, int64_t* last_slice_edges);

/* Device memory for callers that have no HIP toolchain of their own (the C++ host library is built with g++ against this header
 * only): buffers for the `d_` parameters below, on the handle's device, and a blocking copy back to the host that first waits
 * for the handle's stream. */
int ppgpu_device_alloc(ppgpu_ctx* ctx, uint64_t bytes, void** d_out);
int ppgpu_device_free(ppgpu_ctx* ctx, void* d_ptr);
int ppgpu_device_read(ppgpu_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);
/* The records' way home while the next batch is being costed (SURVEY.md 8 e: "overlap D2H with the next batch"): an asynchronous
 * device-to-host copy on an SDMA engine (hsa_amd_memory_async_copy) instead of on the CUs — hipMemcpyAsync into pinned memory runs
 * as a blit kernel on this stack and takes wave slots from the fp64-bound costing kernels.  The caller makes sure the source is
 * complete (ppgpu_synchronize) and that h_pinned_dst is pinned host memory (hipHostMalloc, torch pin_memory).  One copy in flight
 * per handle: a second call first waits for the first; ppgpu_copy_engine_wait blocks until the copy has landed. */
int ppgpu_copy_engine_read(ppgpu_ctx* ctx, void* h_pinned_dst, const void* d_src, uint64_t bytes);
int ppgpu_copy_engine_wait(ppgpu_ctx* ctx);

/* ---------------------------------------------------------------- world state */

/* PlannerConfig setters + Ribbon::RibbonWidth + RibbonManager heuristic. */
int ppgpu_set_config(ppgpu_ctx* ctx, const ppgpu_config* cfg);

/* Map::isBlocked source.  rows*cols bytes, row 0 = y in [0,res) (i.e. AFTER the
 * row reversal GridWorldMap's loader applies, GridWorldMap.cpp:25), non-zero =
 * blocked; queries outside [0,cols*res) x [0,rows*res) are blocked
 * (GridWorldMap.cpp:84-93).  rows == 0 selects the base Map: nothing is ever
 * blocked and the extremes are +-DBL_MAX (Map.cpp:4-6, Map.h:34). */
int ppgpu_set_grid(ppgpu_ctx* ctx, const uint8_t* h_cells, int32_t rows, int32_t cols, double resolution);
/* For tests and tools: the clearance map the device built from the grid (rows*cols bytes, cell (r, c) at r*cols + c: the
 * chessboard distance in cells to the nearest cell that is blocked or outside the grid, 0 on a blocked cell, capped at 64),
 * which decides which chunks of steps the pose sweep never samples.  Copied on the handle's stream; the call waits for it.
 * PPGPU_EINVAL without a grid (rows == 0) or when capacity < rows*cols.  No planner path calls this. */
int ppgpu_get_grid_clearance(ppgpu_ctx* ctx, uint8_t* h_out, int64_t capacity);

/* BinaryDynamicObstaclesManager contents: n rows of
 * {x, y, heading, speed, time, width, length} exactly as passed to update()
 * (BinaryDynamicObstaclesManager.cpp:24-35, constructor .h:17-19). */
int ppgpu_set_obstacles(ppgpu_ctx* ctx, int32_t model, int32_t n, const double* h_obstacles7);

/* GaussianDynamicObstaclesManager contents (GaussianDynamicObstaclesManager.h:19-49, .cpp:16-47): n rows of
 * {x, y, heading, speed, time} as passed to update(mmsi, x, y, heading, speed, time), followed — when
 * covariance_given != 0 — by the row-major 2x2 covariance {c00, c01, c10, c11} of the second update() overload
 * (rows of 9 doubles); otherwise rows of 5 doubles and the reference's default covariance [[30,10],[10,30]].
 * collisionExists then is the sum of the obstacles' pdfs at the pose, 0 when below 1e-5, and the edge's collision
 * penalty the sum over steps of that value times collision_penalty_factor (Edge.cpp:150-151).
 * Obstacles whose pdf is below 1e-13 over a whole 64-step chunk are skipped (relative effect < 1e-7). */
int ppgpu_set_gaussian_obstacles(ppgpu_ctx* ctx, int32_t n, const double* h_obstacles, int32_t covariance_given);

/* The open-vertex array: n vertices and the pool of their ribbons
 * (4 doubles each: startX, startY, endX, endY; Ribbon.h:126).  Also rebuilds the
 * per-vertex collision-check time grids (Edge.cpp:114-120,173). */
int ppgpu_set_vertices(ppgpu_ctx* ctx, int32_t n, const ppgpu_vertex* h_vertices,
                       int32_t n_ribbons, const double* h_ribbons4);

/* -------------------------------------------------------------------- sampling */

/* StateGenerator(minX,maxX,minY,maxY,minSpeed,maxSpeed,seed,ribbonManager)
 * (StateGenerator.cpp:5-13,33-38).  bounds6 = {minX,maxX,minY,maxY,minSpeed,maxSpeed};
 * n_ribbons < 0 selects the ribbon-less constructor.  Clears the sample store. */
int ppgpu_sampler_init(ppgpu_ctx* ctx, const double* bounds6, uint64_t seed,
                       int32_t n_ribbons, const double* h_ribbons4);

/* SamplingBasedPlanner::addSamples(generator, n) (SamplingBasedPlanner.cpp:157-164):
 * draw n_attempts states from the generator's stream, keep those whose cell is
 * free, append them (in stream order) to the device sample store.
 * *n_total_out = resulting m_Samples.size(). */
int ppgpu_sampler_add(ppgpu_ctx* ctx, int64_t n_attempts, int64_t* n_total_out);

/* Advance the generator by n_attempts states without storing them (rank r of a sharded
 * batch skips the r * batch attempts that belong to lower ranks; SURVEY.md 8 e).
 * Asynchronous: launches only.  Where the stream resumes depends on the skipped draws (a sample projected onto a ribbon
 * consumes a sixth draw, StateGenerator.cpp:21-28), but the position is kept in device memory and the next
 * ppgpu_sampler_add / ppgpu_sampler_skip starts from it there; an error of the skip is reported by the next ppgpu_sampler_add. */
int ppgpu_sampler_skip(ppgpu_ctx* ctx, int64_t n_attempts);

/* Replace the sample (target-state) store with caller data; x/y/heading arrays of n. */
int ppgpu_set_samples(ppgpu_ctx* ctx, int64_t n, const double* h_x, const double* h_y, const double* h_heading);
/* Explicit target states that are not samples — the nearest ribbon endpoint of the vertex being expanded
 * (SamplingBasedPlanner.cpp:66-79), Brown-path seeds (AStarPlanner.cpp:150-162).  They are stored BEHIND the samples
 * (indices *first_index .. *first_index + n - 1 for edge descriptors), are not seen by ppgpu_dubins_lengths /
 * ppgpu_select_nearest, and are dropped by the next ppgpu_sampler_add / ppgpu_set_samples / ppgpu_set_extra_targets. */
int ppgpu_set_extra_targets(ppgpu_ctx* ctx, int32_t n, const double* h_x, const double* h_y, const double* h_heading,
                            int64_t* first_index);

/* Copy samples [first, first+n) out as States {x,y,heading,speed,time} (5 doubles each). */
int ppgpu_get_samples(ppgpu_ctx* ctx, int64_t first, int64_t n, double* h_states5);
int64_t ppgpu_num_samples(ppgpu_ctx* ctx);

/* ------------------------------------------------------------- edge generation */

/* Edge::computeApproxCost for every (vertex in [v0,v0+nv), sample, radius):
 * the Dubins length DubinsWrapper::length() (Edge.cpp:11-20, DubinsWrapper.cpp:9-22).
 * d_lengths receives nv * n_samples * 2 doubles, index ((v-v0)*n_samples + s)*2 + r,
 * r = 0 turning_radius, r = 1 coverage_turning_radius; -1 for pairs closer than
 * collision_checking_increment (SamplingBasedPlanner.cpp:111). */
int ppgpu_dubins_lengths(ppgpu_ctx* ctx, int32_t v0, int32_t nv, double* d_lengths);

/* The k best samples by Dubins length per (vertex, radius) — the result of the
 * lazy scan in SamplingBasedPlanner::expand (SamplingBasedPlanner.cpp:85-133).
 * h_sample_index / h_length receive nv*2*k entries (index -1 = fewer than k). */
int ppgpu_select_nearest(ppgpu_ctx* ctx, int32_t v0, int32_t nv, int32_t k,
                         int32_t* h_sample_index, double* h_length);

/* The same k samples per (vertex, radius), in the ORDER SamplingBasedPlanner::expand pushes their children: the front-to-back
 * order of the reference's `bestSamples` heap array when its nearest-first scan of the samples ends (std::push_heap / std::pop_heap
 * on approximate cost, SamplingBasedPlanner.cpp:82-133,134-149).  Which child std::pop_heap surfaces first among children of
 * exactly equal f depends on it.  Vertices [0, nv) (v0 must be 0); h_sample_index receives nv*2*k entries (-1 = fewer than k).
 * A list the device cannot replay (k >= 64, more candidates than its scratch holds, two candidates of exactly equal cost inside
 * the heap) keeps ascending length and is counted in *h_fallbacks (may be NULL) and in ppgpu_order_fallbacks(). */
int ppgpu_expand_order(ppgpu_ctx* ctx, int32_t v0, int32_t nv, int32_t k, int32_t* h_sample_index, uint32_t* h_fallbacks);
uint64_t ppgpu_order_fallbacks(ppgpu_ctx* ctx);

/* --------------------------------------------------------------- edge costing */

/* Dense form: every vertex in [v0,v0+nv) x every sample in [s0,s0+ns) x the
 * (radius,speed) configurations enabled in cfg_mask (bit c set = configuration c,
 * c = PPGPU_EDGE_* bits, so 0xF = all four).  Edge e of the launch is
 *   e = ((v-v0)*ns + (s-s0))*popcount(cfg_mask) + rank of c in cfg_mask.
 * Results go to d_results[e]; child ribbon lists (ribbon_stride*4 doubles per edge)
 * to d_child_ribbons, which may be NULL.  Asynchronous on the handle's stream. */
int ppgpu_cost_edges_dense(ppgpu_ctx* ctx, int32_t v0, int32_t nv, int64_t s0, int64_t ns,
                           uint32_t cfg_mask, ppgpu_edge_result* d_results,
                           double* d_child_ribbons, int32_t ribbon_stride);

/* List form: n packed descriptors (ppgpu_edge_pack) in device memory. */
int ppgpu_cost_edges_list(ppgpu_ctx* ctx, int64_t n, const uint64_t* d_edges,
                          ppgpu_edge_result* d_results,
                          double* d_child_ribbons, int32_t ribbon_stride);

/* SamplingBasedPlanner::expand (SamplingBasedPlanner.cpp:52-151) for nv open vertices in ONE round trip: upload the
 * vertices (as ppgpu_set_vertices), find the k samples of smallest Dubins length per vertex and radius (:85-133), build every
 * vertex's edges in the order expand() pushes them —
 *     the vertex's nearest-point-to-cover target (h_nearest, 3 doubles {x, y, heading} per vertex, x = NaN: none; :64-81)
 *       at each speed {max, slow if distinct} and each radius {turning, coverage if distinct},
 *     then, per radius, its k winners in the order of the reference's heap array (ppgpu_expand_order), each at each speed (:134-149)
 * — cost them (Vertex::connect + Edge::computeTrueCost + computeApproxToGo) and return descriptors, records and child ribbons
 * compacted vertex by vertex.  Output arrays hold ppgpu_expand_capacity(nv, k) entries; *n_edges receives the count.
 * Synchronous; replaces the open-vertex array and the explicit targets of the handle. */
int64_t ppgpu_expand_capacity(int32_t nv, int32_t k);
int ppgpu_expand_host(ppgpu_ctx* ctx, int32_t nv, const ppgpu_vertex* h_vertices, int32_t n_ribbons, const double* h_ribbons,
                      const double* h_nearest, int32_t k, int64_t* n_edges, uint64_t* h_edges, ppgpu_edge_result* h_results,
                      double* h_child_ribbons, int32_t ribbon_stride);

/* Vertex::computeApproxToGo (Vertex.cpp:49-64) on its own: h of n poses {x, y, heading}, pose i with its own ribbon list
 * (h_ribbon_counts[i] ribbons, 4 doubles each, concatenated in h_ribbons), with the configured heuristic.  The root of a
 * search has no parent edge; this gives it the same arithmetic as every other vertex.  h_out[i] = distance / max_speed *
 * time_penalty_factor; h_flags[i] (may be NULL) receives PPGPU_F_RIBBON_OVF where the list exceeds the heuristic's limit. */
int ppgpu_heuristic_host(ppgpu_ctx* ctx, int32_t n, const double* h_poses3, const int32_t* h_ribbon_counts, const double* h_ribbons,
                         double* h_out, uint32_t* h_flags);

/* The point-robot TSP heuristics of child lists beyond the enumeration's 8 (12) ribbons, on the device: an exact table over (ribbons
 * done, last ribbon, end entered) gives the enumeration's value bit for bit.  Off by default.  With max_ribbons in
 * 1 .. PPGPU_TSP_TABLE_MAX every costing launch and ppgpu_heuristic_host ends with a pass over the records whose whole list
 * (count <= ribbon_stride) has min_ribbons .. max_ribbons ribbons: h and f are filled in and PPGPU_F_RIBBON_OVF is cleared.
 * min_ribbons = 0 takes only the records the enumeration flagged PPGPU_F_RIBBON_OVF; min_ribbons >= 1 takes every record in the
 * range (tests hold the table to the enumeration that way).  Under PPGPU_H_TSP_POINT_K a list on which the reference's choice of K
 * ribbons depends on an exact tie of sort keys is refused: the record stays as it was (flag, h = 0) and is counted.  The other
 * heuristics are not touched.  max_ribbons = 0 switches the pass off and frees nothing; the workspace (at most 1 GiB) is allocated
 * here, never inside a costing call.  PPGPU_EINVAL: min_ribbons < 0, max_ribbons < 0 or > PPGPU_TSP_TABLE_MAX, min > max > 0. */
#define PPGPU_TSP_TABLE_MAX 16
int ppgpu_set_tsp_table(ppgpu_ctx* ctx, int32_t min_ribbons, int32_t max_ribbons);
/* The same pass for the Dubins-TSP heuristics (PPGPU_H_TSP_DUBINS_ALL / _K), whose enumeration stops at 8 ribbons: a switch of its
 * own, off by default, with the arguments, the range rules and the errors of ppgpu_set_tsp_table.  Each switch serves its own two
 * heuristics and leaves the other two alone.  The table is filled over the Dubins lengths between oriented ribbon ends that the
 * enumeration uses, so it gives the enumeration's bits.  The reference's K variant never limits the ribbons entered:
 * no list is refused, and with tsp_k <= 0 h is DBL_MAX / max_speed * time_penalty_factor as from the enumeration.  The workspace is
 * the one of ppgpu_set_tsp_table, sized for the larger of the two ranges and allocated here or there, never in a costing call; the
 * counters of ppgpu_tsp_table_stats and the time of ppgpu_last_tsp_table_timing are shared by the two switches. */
int ppgpu_set_dubins_tsp_table(ppgpu_ctx* ctx, int32_t min_ribbons, int32_t max_ribbons);
/* Lists the pass answered / refused on this handle so far, under either switch (device counters, one small copy; waits for the handle's stream). */
int ppgpu_tsp_table_stats(ppgpu_ctx* ctx, uint64_t* lists, uint64_t* refused);
/* With ppgpu_enable_timing on: device milliseconds of the last table pass (listing kernel and table kernel, from HIP events; waits
 * for it).  PPGPU_ESTATE when no pass has been timed. */
int ppgpu_last_tsp_table_timing(ppgpu_ctx* ctx, double* ms);

/* Convenience for small batches (the host planner's <= 40 edges per expansion):
 * host descriptors in, host results out, synchronous. */
int ppgpu_cost_edges_host(ppgpu_ctx* ctx, int64_t n, const uint64_t* h_edges,
                          ppgpu_edge_result* h_results,
                          double* h_child_ribbons, int32_t ribbon_stride);

/* Wrapper edges (previous-plan re-costing): host descriptors in, host results out, synchronous.
 * The caller must route a wrapper whose rho differs from the radius its coverage flag implies
 * through ppgpu_cost_edges_* instead (Edge.cpp:78-80 re-solves the curve in that case). */
int ppgpu_cost_wrapper_edges_host(ppgpu_ctx* ctx, int64_t n, const ppgpu_wrapper_edge* h_edges,
                                  ppgpu_edge_result* h_results,
                                  double* h_child_ribbons, int32_t ribbon_stride);

/* ---------------------------------------------------------------- plan chains */

/* Why the chain of a plan ended (h_stop of ppgpu_cost_plans_host): the stop rules of AStarPlanner.cpp:53-57 plus the cases the
 * leg-by-leg host loop throws on. */
#define PPGPU_CHAIN_LEGS        1u /* every leg was costed: the plan ran out of legs                                   */
#define PPGPU_CHAIN_INFEASIBLE  2u /* the last costed leg is PPGPU_F_INFEASIBLE (AStarPlanner.cpp:53-56)                 */
#define PPGPU_CHAIN_GOAL        3u /* the last costed leg's child satisfies goalCondition (AStarPlanner.cpp:57)          */
#define PPGPU_CHAIN_THROWS      4u /* the last costed leg is PPGPU_F_THROWS: the reference throws out of plan() here     */
#define PPGPU_CHAIN_CAPACITY    5u /* PPGPU_F_DUBINS_ERR, PPGPU_F_RIBBON_LOST, or a child list that does not fit ribbon_stride */

/* AStarPlanner::plan's walk over the previous plan (AStarPlanner.cpp:46-59) for n_plans plans in ONE call: plan p is the legs
 * h_legs[h_leg_offsets[p] .. h_leg_offsets[p + 1]); its first leg starts from the open vertex its .vertex names (set with
 * ppgpu_set_vertices; any number of plans may share one; the .vertex of later legs is not read), every later leg from the vertex
 * the leg before produced — Vertex::connect(lastPlanEnd, wrapper, coverageAllowed) + Edge::computeTrueCost (Vertex.cpp:28-36,
 * Edge.cpp:68-206) — end state, g, coverageCompletedTime and child ribbon list, which never leave the device.  The walk of a plan
 * ends after a leg that is infeasible, reaches a goal, throws or exceeds a capacity, or after its last leg: h_legs_costed[p] legs
 * were costed and h_stop[p] says why (PPGPU_CHAIN_*).  PPGPU_F_RIBBON_OVF on a record whose child list fits ribbon_stride does not
 * end it (only h was not enumerated).  Leg k of plan p leaves its record in h_results[h_leg_offsets[p] + k] and its child ribbons
 * in the same slot of h_child_ribbons (ribbon_stride * 4 doubles, may be NULL), exactly the bytes ppgpu_set_vertices +
 * ppgpu_cost_wrapper_edges_host give leg by leg; the slots of legs that were not costed are left untouched.  ribbon_stride is
 * 1 .. 64.  A leg whose rho differs from the radius its coverage flag implies (Edge.cpp:78-80 re-solves it) is refused with
 * PPGPU_EINVAL: the caller ends the chain before it.  Synchronous: one upload, one launch sequence per depth with no host wait
 * between depths, one download, one host wait.  The handle's open vertices are unchanged afterwards. */
int ppgpu_cost_plans_host(ppgpu_ctx* ctx, int32_t n_plans, const int32_t* h_leg_offsets, const ppgpu_wrapper_edge* h_legs,
                          ppgpu_edge_result* h_results, double* h_child_ribbons, int32_t ribbon_stride,
                          int32_t* h_legs_costed, uint32_t* h_stop);

/* ------------------------------------------------------------------ edge traces */

/* What happened ALONG an edge: one record per executed step of the sweep of Edge::computeTrueCost (Edge.cpp:125-175), i.e. per
 * pass of `while (intermediate.time() < endTime)` whose DubinsWrapper::sample succeeded, the blocked one included — as many as
 * bits 16-31 of the edge's ppgpu_edge_result.info say.  The costing launch keeps no per-step state; pp_k_trace_steps rebuilds it
 * from the same solved curve, the same time grid and the same map / obstacle code, without skipping anything. */
#define PPGPU_S_BLOCKED  0x1u  /* Map::isBlocked at this pose (Edge.cpp:144): only ever the last record of an edge */
#define PPGPU_S_STRAIGHT 0x2u  /* lastHeading == intermediate.heading() (Edge.cpp:159): covers even when !coverageAllowed */
typedef struct ppgpu_step_record {          /* 64 bytes */
    double x, y, heading, time;             /* the State handed to isBlocked / collisionExists / cover (Edge.cpp:127) */
    double collision;                       /* collisionExists(intermediate, true) (:150-151); 0 on a blocked step */
    double penalty_before;                  /* collisionPenalty when this step was sampled = the term in gSoFar (:138) */
    uint32_t flags, step;                   /* PPGPU_S_*; the step's index k */
    double reserved;                        /* 0 */
} ppgpu_step_record;

/* Edge::computeTrueCost (Edge.cpp:68-206) step by step for a list of n packed descriptors: first the costing launch of
 * ppgpu_cost_edges_list on the same list (d_results receives exactly its records), then the trace.  d_counts[i] receives the edge's
 * step count (0 for an edge flagged PPGPU_F_THROWS or malformed), d_steps[i * step_stride + k] the record of its step k for
 * k < min(count, step_stride): an edge with more steps than step_stride is cut, not refused, and its count still says how many
 * there were (as with ribbon_stride); records beyond an edge's count are left untouched.  d_steps must be 16-byte aligned.
 * Asynchronous on the handle's stream. */
int ppgpu_trace_edges_list(ppgpu_ctx* ctx, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results,
                           int32_t step_stride, int32_t* d_counts, ppgpu_step_record* d_steps);
/* The same with host descriptors in and host arrays out, synchronous.  h_results may be NULL.  The step records pass through a
 * buffer of the handle that grows like its other buffers (ppgpu_growth_stats counts it); a trace that would exceed the handle's
 * workspace budget runs as consecutive slices of the list, like a costing launch. */
int ppgpu_trace_edges_host(ppgpu_ctx* ctx, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results,
                           int32_t step_stride, int32_t* h_counts, ppgpu_step_record* h_steps);
/* ... for edges whose curve is given (Vertex::connect(start, DubinsWrapper, coverageAllowed), Vertex.cpp:28-36, as
 * ppgpu_cost_wrapper_edges_host costs them): the steps of a plan's segments (AStarPlanner.cpp:46-59 walks them the same way).  A
 * curve that starts after the vertex's first step has no steps (the first sample throws, Edge.cpp:126-133). */
int ppgpu_trace_wrapper_edges_host(ppgpu_ctx* ctx, int64_t n, const ppgpu_wrapper_edge* h_wedges, ppgpu_edge_result* h_results,
                                   int32_t step_stride, int32_t* h_counts, ppgpu_step_record* h_steps);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds pp_k_trace_steps took in the last trace call, summed
 * over its slices (HIP events on the handle's stream around the kernel alone).  Waits for the launch. */
int ppgpu_last_trace_timing(ppgpu_ctx* ctx, double* ms_trace);

/* -------------------------------------------------------------- coverage traces */

/* What every step of an edge did to the ribbons: the coverage state machine of Edge::computeTrueCost (Edge.cpp:153-171) executed
 * literally by pp_k_trace_cover, one record per executed step — record k of an edge belongs to ppgpu_step_record k of the same
 * edge (same step count, same poses) — and one summary per edge that includes the last cover (Edge.cpp:181-191).  The costing
 * launch's cover sweep visits event steps only and takes stretches of them as runs; this walk skips nothing. */
#define PPGPU_C_EVENT   0x1u  /* the else-branch of Edge.cpp:153-158 ran: minDistanceFrom was evaluated (:158)             */
#define PPGPU_C_COVER   0x2u  /* cover() was called at this step (:159-161)                                                */
#define PPGPU_C_CHANGED 0x4u  /* ... and the ribbon list is not, value for value, what it was before the step              */
#define PPGPU_C_DONE    0x8u  /* RibbonManager::done() after the step (:162; RibbonManager.cpp:24-26)                      */
typedef struct ppgpu_cover_record {   /* 32 bytes */
    double to_cover;          /* toCoverDistance after the step's branch (Edge.cpp:153-158).  While the list is empty
                               * minDistanceFrom is 0 (RibbonManager.cpp:143): every step is then an event and this is 0   */
    double remaining;         /* sum of the end-to-end lengths (start to end point) of the ribbons left after the step     */
    uint32_t flags, step;     /* PPGPU_C_*; the step's index k.  A blocked step (Edge.cpp:144-146) breaks before the
                               * coverage branch: its record repeats the state before it, with PPGPU_C_DONE at most        */
    uint32_t ribbons;         /* list length after the step                                                                */
    uint32_t reserved;        /* 0 */
} ppgpu_cover_record;

/* Bits of ppgpu_cover_summary.flags */
#define PPGPU_CS_LAST_COVER   0x01u /* the last cover ran (Edge.cpp:182-184: coverageAllowed, or the heading did not change)  */
#define PPGPU_CS_LAST_CHANGED 0x02u /* ... and changed the list                                                               */
#define PPGPU_CS_DONE         0x04u /* child->done() after it (:185) = PPGPU_F_DONE of the edge's record                      */
#define PPGPU_CS_REFUSED      0x08u /* the list is, or would have grown, beyond the device's 64 ribbons per vertex (the edge's
                                     * record carries PPGPU_F_RIBBON_LOST): count 0, nothing else in the summary is meaningful */
#define PPGPU_CS_THROWS       0x10u /* PPGPU_F_THROWS or a malformed descriptor: the reference throws before the last cover
                                     * (Edge.cpp:178), there is no child; count 0                                             */
typedef struct ppgpu_cover_summary {  /* 32 bytes, per edge */
    int32_t events, changes;          /* steps with PPGPU_C_EVENT / PPGPU_C_CHANGED (the last cover is not a step)            */
    int32_t ribbons_final;            /* list length after the last cover (Edge.cpp:181-191) = bits 8-15 of the record's info */
    uint32_t flags;                   /* PPGPU_CS_*                                                                           */
    double coverage_completed_time;   /* the child's RibbonManager::coverageCompletedTime() (:164-166,187-189), -1 unset      */
    double remaining_final;           /* `remaining` after the last cover                                                     */
} ppgpu_cover_summary;

/* Edge::computeTrueCost's coverage branch (Edge.cpp:153-171,181-191) step by step for a list of n packed descriptors: first the
 * costing launch of ppgpu_cost_edges_list on the same list (d_results receives exactly its records), then the walk.  d_counts[i]
 * receives the edge's step count (what ppgpu_trace_edges_list reports; 0 with PPGPU_CS_REFUSED / PPGPU_CS_THROWS), d_cover[i *
 * step_stride + k] the record of its step k for k < min(count, step_stride): a stride below an edge's count cuts the records,
 * never the count, the summary or the final list; records beyond an edge's count are left untouched.  d_summaries[i] receives the
 * edge's summary; d_child_ribbons (may be NULL) the list after the last cover, ribbon_stride * 4 doubles per edge, its first
 * min(ribbons_final, ribbon_stride) entries written (the costing convention).  d_cover must be 16-byte aligned.  Asynchronous on
 * the handle's stream. */
int ppgpu_trace_cover_list(ppgpu_ctx* ctx, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results,
                           int32_t step_stride, int32_t* d_counts, ppgpu_cover_record* d_cover,
                           ppgpu_cover_summary* d_summaries, double* d_child_ribbons, int32_t ribbon_stride);
/* The same with host descriptors in and host arrays out, synchronous.  h_results and h_child_ribbons may be NULL; entries of
 * h_child_ribbons beyond an edge's final list are zeroed.  The records pass through buffers of the handle that grow like its other
 * buffers (ppgpu_growth_stats counts them); a walk that would exceed the handle's workspace budget runs as consecutive slices of
 * the list, like a costing launch. */
int ppgpu_trace_cover_host(ppgpu_ctx* ctx, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results,
                           int32_t step_stride, int32_t* h_counts, ppgpu_cover_record* h_cover,
                           ppgpu_cover_summary* h_summaries, double* h_child_ribbons, int32_t ribbon_stride);
/* ... for edges whose curve is given (Vertex::connect(start, DubinsWrapper, coverageAllowed), Vertex.cpp:28-36, as
 * ppgpu_trace_wrapper_edges_host traces them).  A curve that starts after the vertex's first step has no steps (Edge.cpp:126-133):
 * its summary is that of the last cover alone, at the vertex's own pose. */
int ppgpu_trace_cover_wrapper_edges_host(ppgpu_ctx* ctx, int64_t n, const ppgpu_wrapper_edge* h_wedges, ppgpu_edge_result* h_results,
                                         int32_t step_stride, int32_t* h_counts, ppgpu_cover_record* h_cover,
                                         ppgpu_cover_summary* h_summaries, double* h_child_ribbons, int32_t ribbon_stride);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds pp_k_trace_cover took in the last coverage-trace call,
 * summed over its slices (HIP events on the handle's stream around the kernel alone).  Waits for the launch. */
int ppgpu_last_cover_trace_timing(ppgpu_ctx* ctx, double* ms_cover_trace);

/* --------------------------------------------------------------- contact traces */

/* Which contact an edge pays for: one record per (edge i, obstacle row j) at contacts[i * n_obst + j], rows in the order of
 * ppgpu_set_obstacles / ppgpu_set_gaussian_obstacles (ppgpu_obstacle_count gives n_obst).  pp_k_trace_contacts walks the executed
 * steps of the edge's sweep — the steps of ppgpu_step_record, same count, same poses and times — and evaluates every contact on its
 * own at every one of them with the arithmetic of collisionExists (Edge.cpp:150-151): the contact's centre projected to the step's
 * time, then the strict box test (BinaryDynamicObstaclesManager.cpp:4-22) or the pdf (GaussianDynamicObstaclesManager.h:31-43).
 *   hit step, binary model     a step that is not blocked (a blocked step breaks before :150) and whose pose the contact's strict box
 *                              holds.  For every edge sum_j hit_steps * collision_penalty_factor is the record's collision_penalty,
 *                              exactly.
 *   hit step, Gaussian model   a COUNTED step — not blocked, and collisionExists, the floored sum over all contacts, is not 0 — at
 *                              which this contact's own pdf is >= 1e-5 (the manager's floor applied to the contact alone).  exposure
 *                              sums the contact's pdf over all counted steps: sum_j exposure * collision_penalty_factor agrees with
 *                              collision_penalty to rounding and to what the costing launch's 1e-13 cull leaves out (this walk
 *                              culls nothing). */
typedef struct ppgpu_contact_record {       /* 64 bytes */
    double cpa_distance;      /* min over EVERY executed step (the blocked one included) of the distance from the pose to the
                               * contact's centre projected to the step's time = sqrt(min d2); -1 without steps */
    double cpa_time;          /* that step's time (the earliest step on equal d2); -1 without steps */
    double first_hit_time, last_hit_time;   /* -1 without a hit step */
    double exposure;          /* binary: (double)hit_steps.  Gaussian: sum of this contact's pdf over the counted steps */
    int32_t cpa_step, hit_steps, first_hit_step, last_hit_step;   /* -1 / 0 / -1 / -1 when empty */
    double peak;              /* Gaussian: max of this contact's pdf over every executed step; binary: 0 */
} ppgpu_contact_record;

/* Rows and model (PPGPU_OBST_*) of the handle's obstacle table: what sizes a contacts array.  Either output may be NULL. */
int ppgpu_obstacle_count(ppgpu_ctx* ctx, int32_t* n, int32_t* model);
/* The per-contact reports of a list of n packed descriptors: first the costing launch of ppgpu_cost_edges_list on the same list
 * (d_results receives exactly its records), then the walk.  d_counts[i] receives the edge's step count (what
 * ppgpu_trace_edges_list reports), d_contacts[i * n_obst + j] the record of edge i and row j; an edge without steps gets the
 * empty record for every row.  With no obstacles set the call still writes results and counts, and touches nothing of d_contacts
 * (which may then be NULL).  d_contacts must be 16-byte aligned.  Asynchronous on the handle's stream. */
int ppgpu_trace_contacts_list(ppgpu_ctx* ctx, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, int32_t* d_counts,
                              ppgpu_contact_record* d_contacts);
/* The same with host descriptors in and host arrays out, synchronous.  h_results may be NULL.  The records pass through a buffer of
 * the handle that grows like its other buffers (ppgpu_growth_stats counts it); a walk that would exceed the handle's workspace
 * budget runs as consecutive slices of the list, like a costing launch. */
int ppgpu_trace_contacts_host(ppgpu_ctx* ctx, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results, int32_t* h_counts,
                              ppgpu_contact_record* h_contacts);
/* ... for edges whose curve is given (as ppgpu_trace_wrapper_edges_host traces them): the contacts of a plan's segments.  A curve
 * that starts after the vertex's first step has no steps (Edge.cpp:126-133): empty records. */
int ppgpu_trace_contacts_wrapper_edges_host(ppgpu_ctx* ctx, int64_t n, const ppgpu_wrapper_edge* h_wedges, ppgpu_edge_result* h_results,
                                            int32_t* h_counts, ppgpu_contact_record* h_contacts);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds pp_k_trace_contacts took in the last contact-trace call,
 * summed over its slices (HIP events on the handle's stream around the kernel alone).  Waits for the launch. */
int ppgpu_last_contact_trace_timing(ppgpu_ctx* ctx, double* ms_contact_trace);

/* --------------------------------------------------------------- chart clearance */

/* How close a pose, an edge or a plan comes to a charted hazard.  The reference asks the static map a yes/no question at every
 * sampled pose (Map::isBlocked: GridWorldMap.cpp:84-93, called at Edge.cpp:144); this is the distance behind that answer.
 * A HAZARD CELL is a cell that is blocked or lies outside the grid (isBlocked is true there).  With g(d) = max(|d| - 1, 0),
 *     gap2((r, c), (r', c')) = g(r - r')^2 + g(c - c')^2      the squared distance, in cells, between the nearest edges of two cells
 *     gap2(A) = min over hazard cells B of gap2(A, B)         0 on a blocked cell and on its eight neighbours
 * Every point of cell A is at least resolution * sqrt(gap2(A)) from every point of every hazard cell (a certified lower bound), and
 * at most resolution * (sqrt(gap2(A)) + sqrt(2)) from some hazard cell.  The device holds min(gap2, PPGPU_DIST_CAP2) as uint16_t,
 * one value per cell at r * cols + c: an exact integer map, built on the first call that needs it after a ppgpu_set_grid
 * (pp_k_dist_cols, pp_k_dist_rows) and kept until the next one.  The clearance of a pose is that of the cell isBlocked puts it
 * in; a pose outside the grid has gap2 0.  clearance = resolution * sqrt((double)gap2), in metres. */
#define PPGPU_DIST_CAP  255     /* cells */
#define PPGPU_DIST_CAP2 65025   /* PPGPU_DIST_CAP squared: a stored value this large means "at least" */
/* For tests and tools: the whole map (rows*cols values).  Copied on the handle's stream; the call waits for it.  PPGPU_EINVAL
 * without a grid (rows == 0) or when capacity < rows*cols. */
int ppgpu_get_grid_distance(ppgpu_ctx* ctx, uint16_t* h_out, int64_t capacity);
/* The certified lower bound at n points {x, y} of h_xy2: h_clearance[i] in metres, h_gap2[i] in cells squared; either output may
 * be NULL.  A point on a blocked cell or outside the grid gives 0.  Without a grid (the base Map, rows == 0) nothing is charted:
 * clearance = DBL_MAX and gap2 = PPGPU_DIST_CAP2.  Synchronous. */
int ppgpu_grid_clearance_at(ppgpu_ctx* ctx, int64_t n, const double* h_xy2, double* h_clearance, uint32_t* h_gap2);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds the two passes of the last build of the map took together
 * (HIP events on the handle's stream around the two kernels).  PPGPU_ESTATE when no build was timed. */
int ppgpu_last_grid_distance_timing(ppgpu_ctx* ctx, double* ms_build);

/* The clearance of an edge: one record per edge, from a walk over the executed steps of its sweep — the steps of
 * ppgpu_step_record, same count, same poses and times — that takes the gap2 of every step's cell. */
#define PPGPU_CL_EMPTY   0x1u  /* no executed step (PPGPU_F_THROWS, malformed, a curve starting after the vertex's first step) */
#define PPGPU_CL_BLOCKED 0x2u  /* the last executed step is the blocked one (Edge.cpp:144-146): clearance 0.  With a keep-out active
                                * (below) "blocked" is blocked in the effective grid, as it is for PPGPU_S_BLOCKED of a step record:
                                * the step's own gap2, and so the clearance, may then be greater than 0 */
#define PPGPU_CL_CAPPED  0x4u  /* min gap2 == PPGPU_DIST_CAP2: clearance is "at least" */
#define PPGPU_CL_NO_MAP  0x8u  /* base Map (rows == 0): clearance DBL_MAX, gap2 = PPGPU_DIST_CAP2, always with CAPPED */
typedef struct ppgpu_clearance_record {   /* 64 bytes */
    double clearance;          /* res * sqrt(min gap2) over EVERY executed step, the blocked one included; -1 when EMPTY */
    double time, x, y;         /* of the step that attains it (the earliest on equal gap2); -1, 0, 0 when EMPTY */
    double first_below_time;   /* time of the first step with gap2 < limit2; -1 without one */
    int32_t step;              /* -1 when EMPTY */
    uint32_t gap2;             /* 0 when EMPTY */
    int32_t below_steps, first_below_step;   /* 0 / -1 */
    uint32_t flags, reserved;  /* PPGPU_CL_*; 0 */
} ppgpu_clearance_record;

/* The calls take a margin in metres.  margin <= 0 (or no grid): no step is counted.  margin > 255 * resolution: PPGPU_EINVAL.
 * Otherwise the host computes limit2 once, the smallest non-negative integer k with resolution * sqrt((double)k) >= margin, and
 * a step is "below" iff its gap2 < limit2: the device compares integers only.
 * The clearance records of a list of n packed descriptors: first the costing launch of ppgpu_cost_edges_list on the same list
 * (d_results receives exactly its records), then the walk.  d_counts[i] receives the edge's step count (what
 * ppgpu_trace_edges_list reports), d_clearance[i] the edge's record; every record is written.  d_clearance must be 16-byte
 * aligned.  Asynchronous on the handle's stream (the first call after a ppgpu_set_grid builds the map on it first). */
int ppgpu_trace_clearance_list(ppgpu_ctx* ctx, int64_t n, const uint64_t* d_edges, ppgpu_edge_result* d_results, int32_t* d_counts,
                               ppgpu_clearance_record* d_clearance, double margin);
/* The same with host descriptors in and host arrays out, synchronous.  h_results may be NULL. */
int ppgpu_trace_clearance_host(ppgpu_ctx* ctx, int64_t n, const uint64_t* h_edges, ppgpu_edge_result* h_results, int32_t* h_counts,
                               ppgpu_clearance_record* h_clearance, double margin);
/* ... for edges whose curve is given (as ppgpu_trace_wrapper_edges_host traces them): the clearance of a plan's segments. */
int ppgpu_trace_clearance_wrapper_edges_host(ppgpu_ctx* ctx, int64_t n, const ppgpu_wrapper_edge* h_wedges, ppgpu_edge_result* h_results,
                                             int32_t* h_counts, ppgpu_clearance_record* h_clearance, double margin);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds pp_k_trace_clearance took in the last clearance-trace
 * call, summed over its slices (HIP events on the handle's stream around the kernel alone).  Waits for the launch. */
int ppgpu_last_clearance_trace_timing(ppgpu_ctx* ctx, double* ms_clearance_trace);

/* The keep-out margin: planning with the distance map, not only reporting on it.
 * limit2 of a margin in metres is the smallest non-negative integer k with resolution * sqrt((double)k) >= margin; margin <= 0
 * gives 0.  ppgpu_keepout_limit2 is the one statement of this rule (no handle, no device): PPGPU_EINVAL for a NaN and for
 * margin > PPGPU_DIST_CAP * resolution.  The trace calls above use it; they go on counting nothing for a margin that is not above 0.
 * The EFFECTIVE GRID at limit2: cell (r, c) is blocked iff gap2(r, c) < limit2, or it is blocked in the grid that was set.  For
 * limit2 >= 1 the first clause contains the second; for limit2 == 0 the effective grid is the grid as set.  Outside the grid stays
 * blocked, and because the outside is a hazard in gap2 the band also runs along the grid's border: this is the hazard set the
 * clearance report measures against.  Every free cell of the effective grid has certified clearance of at least
 * resolution * sqrt(limit2) metres.
 * With a non-zero limit the effective grid (pp_k_keepout_bits) and the chessboard clearance map over it are what every launch
 * reads: the sampler's map filter, all costing routes, all four traces.  The grid as set stays on the device beside it: the
 * distance map, ppgpu_get_grid_distance, ppgpu_grid_clearance_at and the gap2 of the clearance records keep their meaning
 * whatever the limit is.  A handle whose limit was never set does nothing it did not do before. */
int ppgpu_keepout_limit2(double resolution, double margin, uint32_t* limit2);
/* limit2 in cells squared (resolution-free).  limit2 > PPGPU_DIST_CAP2: PPGPU_EINVAL, nothing changed.  The handle keeps the value
 * across ppgpu_set_grid (a grid set under a non-zero limit builds the distance map at once); with the base Map (rows == 0) it is
 * stored and has no effect.  Before or after ppgpu_set_grid: the resulting state is the same.  Synchronous: waits for the stream,
 * then rebuilds the effective grid and its clearance map when the value changes. */
int ppgpu_set_keepout_limit2(ppgpu_ctx* ctx, uint32_t limit2);
int ppgpu_get_keepout_limit2(ppgpu_ctx* ctx, uint32_t* limit2);
/* For tests and tools: the effective grid, one byte 0/1 per cell at r*cols + c.  PPGPU_EINVAL without a grid (rows == 0) or when
 * capacity < rows*cols.  Synchronous. */
int ppgpu_get_grid_blocked(ppgpu_ctx* ctx, uint8_t* h_out, int64_t capacity);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds the last change of the effective grid took:
 * pp_k_keepout_bits (not run on the way back to 0) and the rebuild of the chessboard clearance map.  PPGPU_ESTATE when none was timed. */
int ppgpu_last_keepout_timing(ppgpu_ctx* ctx, double* ms_keepout);

/* ---------------------------------------------------------------- reachable water */

/* Which water a plan can get to at all, and which ribbons lie beyond it.  Everything is exact in integers except where a ribbon's
 * sample points are placed.
 * COMPONENTS.  The grid is the effective grid (what ppgpu_get_grid_blocked returns: the grid as set at limit2 0).  Two free cells are
 * neighbours when they differ by at most 1 in row and in column (8-connectivity); label(r, c) is the smallest row-major index
 * r' * cols + c' over the cells of the component of (r, c); a blocked cell has PPGPU_REACH_NONE.  The labelling is canonical: any
 * correct algorithm writes the same bytes.
 *   Why 8 and not 4: Edge::computeTrueCost samples poses at most collision_checking_increment metres apart (Edge.cpp:114,173) and
 *   declares the edge infeasible at the first pose on a blocked cell (Edge.cpp:144-147).  With increment <= resolution consecutive
 *   poses lie in the same or in 8-neighbouring cells, and two poses either side of the corner between two diagonal hazard cells are
 *   both free: a feasible chain of edges from the start never leaves the 8-connected component of the start's cell, and can leave
 *   nothing smaller.
 * REACH SET of a seed pose: the seed's cell is the one Map::isBlocked puts it in (GridWorldMap.cpp:84-93).  A seed on a blocked cell
 * or outside the grid gives PPGPU_REACH_SEED_BLOCKED, an empty set, and no ribbon is judged.  Otherwise the set is every cell with
 * the seed's label.
 * REACH GAP.  rgap2(A) = min over reachable cells B of gap2(A, B), gap2 as under "chart clearance"; the map holds
 * min(rgap2, PPGPU_DIST_CAP2) as uint16_t.  The outside of the grid is NOT a source here.  Every point of cell A is at least
 * resolution * sqrt(rgap2(A)) from every point of every reachable cell.
 * A RIBBON'S SAMPLES, for {sx, sy, ex, ey} with dx = ex - sx, dy = ey - sy, every product and sum rounded on its own:
 *     len = sqrt(dx*dx + dy*dy),  n = max(1, ceil(len / (0.5 * resolution))),  sample k of 0..n at (sx + dx * (k / n), sy + dy * (k / n))
 * so every point of the ribbon is within resolution / 4 of a sample.  A sample is clamped into [0, cols*res] x [0, rows*res]
 * (projection onto a convex set never increases the distance to a point inside it), its cell is min(size_t(x / res), cols - 1) and
 * likewise for rows.  A sample is OUT iff rgap2(cell) >= lim2 with lim2 = ppgpu_keepout_limit2(resolution, ribbon_width + 0.25 *
 * resolution): an integer comparison.  Ribbon::contains (Ribbon.cpp:39-43) lets a pose cover only what lies within RibbonWidth of it,
 * so no pose in a reachable cell covers any point of the ribbon within resolution / 4 of an OUT sample: that is what a record
 * certifies.  A sample that is not OUT proves nothing: the turning radius may still keep the boat from covering it.
 * Lazy, like the distance map: ppgpu_set_grid and a changed keep-out limit only mark the labels stale, the first call below that
 * needs them builds them (three launches whatever the grid holds), and a seed that moves inside the component of the cached reach
 * set costs one 4-byte look-up.  A handle that never makes these calls allocates and launches nothing for them. */
#define PPGPU_REACH_NONE 0xFFFFFFFFu
#define PPGPU_REACH_TILE 32     /* the labelling's tile edge in cells (tests place their shapes around it) */
/* For tests and tools: the labels, rows*cols values.  PPGPU_EINVAL without a grid (rows == 0), when capacity < rows*cols or when
 * rows*cols >= 2^32 - 1; PPGPU_ECAPACITY if a union-find loop ran into its cap (it cannot).  Synchronous. */
int ppgpu_get_grid_labels(ppgpu_ctx* ctx, uint32_t* h_out, int64_t capacity);
#define PPGPU_REACH_SEED_BLOCKED 0x1u  /* the seed's cell is blocked or outside the grid: nothing is reachable */
#define PPGPU_REACH_NO_MAP       0x2u  /* base Map (rows == 0): nothing is charted, everything is reachable; the counts are 0 */
typedef struct ppgpu_reach_info {       /* 32 bytes */
    uint64_t free_cells, reachable_cells;   /* of the effective grid; with the seed's label (0 for a blocked seed) */
    uint32_t components, seed_label, flags, reserved;   /* PPGPU_REACH_NONE for a blocked seed; PPGPU_REACH_*; 0 */
} ppgpu_reach_info;
/* The seed of the reach set (a plan's start).  Builds the labels if they are stale, and the reach bits and the reach-gap map when
 * the seed's label is not that of the cached set.  out may be NULL.  PPGPU_EINVAL for a NaN.  Synchronous. */
int ppgpu_set_reach_seed(ppgpu_ctx* ctx, double x, double y, ppgpu_reach_info* out);
/* For tests and tools: the reach-gap map of the current seed, rows*cols values (all PPGPU_DIST_CAP2 for a blocked seed).
 * PPGPU_ESTATE without a seed; PPGPU_EINVAL as ppgpu_get_grid_labels.  Synchronous. */
int ppgpu_get_grid_reach_gap(ppgpu_ctx* ctx, uint16_t* h_out, int64_t capacity);
#define PPGPU_RB_ANY_OUT    0x01u  /* some sample is OUT */
#define PPGPU_RB_WHOLE_OUT  0x02u  /* every sample is */
#define PPGPU_RB_START_OUT  0x04u  /* sample 0 is */
#define PPGPU_RB_END_OUT    0x08u  /* the last sample is */
#define PPGPU_RB_DEGENERATE 0x10u  /* len == 0: one sample, pitch 0 */
#define PPGPU_RB_CAPPED     0x20u  /* max_rgap2 == PPGPU_DIST_CAP2: "at least" */
#define PPGPU_RB_NO_SEED    0x40u  /* the seed is blocked: nothing judged, out_samples 0, first_out and last_out -1, the gaps 0 */
#define PPGPU_RB_NO_MAP     0x80u  /* base Map: everything is reachable, nothing judged, as above */
typedef struct ppgpu_ribbon_reach_record {  /* 64 bytes */
    double length, pitch;                   /* len, len / n (0 for a degenerate ribbon) */
    uint32_t samples, out_samples;          /* n + 1 (1 for a degenerate ribbon); how many of them are OUT */
    int32_t first_out, last_out;            /* sample indices, -1 without one */
    uint32_t min_rgap2, max_rgap2, lim2, flags;   /* over the samples' cells, capped as the map is; PPGPU_RB_* */
    double out_length;                      /* pitch * out_samples, capped at length */
    uint64_t reserved;                      /* 0 */
} ppgpu_ribbon_reach_record;
/* One record per ribbon of h_ribbons4 (n rows of {sx, sy, ex, ey}) against the reach set of the current seed.  PPGPU_ESTATE without
 * a seed.  PPGPU_EINVAL for a NaN anywhere, a ribbon with more than 2^22 samples, and ribbon_width + resolution / 4 above 255
 * cells.  Synchronous. */
int ppgpu_ribbon_reach_host(ppgpu_ctx* ctx, int32_t n, const double* h_ribbons4, double ribbon_width, ppgpu_ribbon_reach_record* h_records);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds of the last build of the labels (three kernels), of the
 * last build of a reach set (pp_k_reach_bits and the two passes of its gap map) and of the last ribbon walk; -1 for each that was
 * not timed since ppgpu_enable_timing.  PPGPU_ESTATE with timing off.  Waits for the stream. */
int ppgpu_last_reach_timing(ppgpu_ctx* ctx, double* ms_labels, double* ms_reach_gap, double* ms_ribbons);

/* ---------------------------------------------------------------- distance by water */

/* How far it is by water from a pose (a plan's start) to every cell of the chart and to every ribbon: the planner's heuristics measure
 * straight lines (Vertex::computeApproxToGo), and a breakwater between the start and a survey line makes those arbitrarily optimistic.
 * Everything is exact in integers except where a ribbon's sample points are placed.
 * GRAPH.  The nodes are the free cells of the effective grid (what ppgpu_get_grid_blocked returns: the grid as set at limit2 0); the
 * edges are the 8-neighbour steps the component labels use, a diagonal step allowed whatever the two cells beside it hold (the
 * reasoning under COMPONENTS, "reachable water", applies unchanged).  A row or column step costs PPGPU_WATER_STEP = 12, a diagonal
 * step PPGPU_WATER_DIAG = 17.
 * WATER DISTANCE.  wd(cell) is the cost of the cheapest path from the seed's cell, a uint32_t: 0 on the seed's cell, PPGPU_WATER_NONE
 * on a blocked cell and on a free cell of another component.  The map is canonical: any correct algorithm writes the same bytes.
 * wd(cell) != NONE if and only if label(cell) == label(seed's cell), with the labels of ppgpu_get_grid_labels.
 *   Why 12 and 17: 17 / 12 > sqrt(2), so the polyline through the cell centres of a cheapest path is at most resolution * wd / 12
 *   metres long, and a route of that length or less through free cells therefore exists.  That is what a value certifies: an UPPER
 *   bound on the shortest route through cell centres, at most 0.18 % above its octile length.  It is NOT a lower bound on what a
 *   Dubins vehicle must travel: the turning radius can make the vehicle go farther, and a route between cell centres can be shorter.
 * THE SEED'S CELL is the one Map::isBlocked puts the pose in (GridWorldMap.cpp:84-93), as for the reach seed.  A seed that is blocked
 * or outside the grid gives PPGPU_WATER_SEED_BLOCKED and a map that is all NONE; the base Map (rows == 0) gives PPGPU_WATER_NO_MAP.
 * The water seed is independent of the reach seed.
 * A RIBBON'S SAMPLES are those of the reach report: the same len, n, k / n, clamp and cell rule ("reachable water"), and
 * lim2 = ppgpu_keepout_limit2(resolution, ribbon_width + 0.25 * resolution).
 * APPROACH DISTANCE of a sample in cell A: ad(A) = min of wd(B) over the cells B of the grid with gap2(A, B) < lim2, gap2 as under
 * "chart clearance" (max(|dr| - 1, 0)^2 + max(|dc| - 1, 0)^2); NONE when no such cell has a distance.  It is the distance by water to
 * the nearest cell from which the reach report would let the sample be covered: ad(A) != NONE if and only if the reach report, seeded
 * at the same pose, does not call the sample OUT.  The sample's own cell would not do: a ribbon inside a keep-out band lies on
 * blocked cells and can still be covered from beside them.  lim2 > PPGPU_WATER_MAX_LIM2 (a window of at most 67 x 67 cells) is refused.
 * OVERFLOW.  17 * rows * cols must stay below 2^32 - 1 (no path cost can then reach NONE): PPGPU_EINVAL otherwise.
 * Lazy, like the labels: ppgpu_set_grid and a changed keep-out limit only mark the map stale, the first call below that needs it builds
 * it, and a seed in the cell of the cached map costs no launch.  A handle that never makes these calls allocates and launches
 * nothing for them.  The build relaxes 32 x 32 tiles in rounds, one launch per round (pp_k_water.h); `rounds` says how many had work
 * to do, and may differ between two builds of the same map (the bytes of the map do not). */
#define PPGPU_WATER_NONE 0xFFFFFFFFu
#define PPGPU_WATER_STEP 12
#define PPGPU_WATER_DIAG 17
#define PPGPU_WATER_TILE 32     /* the relaxation's tile edge in cells (tests place their shapes around it) */
#define PPGPU_WATER_MAX_LIM2 1024u
#define PPGPU_WATER_SEED_BLOCKED 0x1u  /* the seed's cell is blocked or outside the grid: the map is all NONE */
#define PPGPU_WATER_NO_MAP       0x2u  /* base Map (rows == 0): nothing is charted; the counts are 0 */
typedef struct ppgpu_water_info {          /* 32 bytes */
    uint64_t wet_cells;                    /* cells with a distance */
    uint32_t max_wd, farthest_cell;        /* the largest distance and the lowest row-major index that attains it (0, NONE when nothing is wet) */
    uint32_t seed_cell, flags;             /* row-major index (NONE for a blocked seed); PPGPU_WATER_* */
    uint32_t rounds, builds;               /* relaxation rounds of the last build; maps this handle has built so far */
} ppgpu_water_info;
/* The seed of the map (a plan's start).  Builds the map when it is stale or the seed's cell is not that of the cached one.  out may
 * be NULL.  PPGPU_EINVAL for a NaN and for 17 * rows * cols >= 2^32 - 1; PPGPU_ECAPACITY if a relaxation loop ran into its cap (it
 * cannot).  Synchronous. */
int ppgpu_set_water_seed(ppgpu_ctx* ctx, double x, double y, ppgpu_water_info* out);
/* For tests and tools: the map of the current seed, rows*cols values.  PPGPU_ESTATE without a seed; PPGPU_EINVAL without a grid
 * (rows == 0) or when capacity < rows*cols.  Synchronous. */
int ppgpu_get_grid_water(ppgpu_ctx* ctx, uint32_t* h_out, int64_t capacity);
/* The map at n points {x, y} of h_xy2 (the cell Map::isBlocked puts each in): h_metres[i] = resolution * wd / 12, +infinity where wd is
 * NONE or the point is outside the grid; h_wd[i] = wd, NONE likewise; either output may be NULL.  The base Map: +infinity and NONE.
 * PPGPU_ESTATE without a seed.  Synchronous. */
int ppgpu_water_distance_at(ppgpu_ctx* ctx, int64_t n, const double* h_xy2, double* h_metres, uint32_t* h_wd);
#define PPGPU_RW_ANY_DRY    0x01u  /* some sample has no approach distance */
#define PPGPU_RW_WHOLE_DRY  0x02u  /* none has */
#define PPGPU_RW_DEGENERATE 0x10u  /* len == 0: one sample, pitch 0 */
#define PPGPU_RW_NO_SEED    0x40u  /* the seed is blocked: nothing judged, wet_samples 0, the sample indices -1, the distances NONE, +infinity metres */
#define PPGPU_RW_NO_MAP     0x80u  /* base Map: nothing judged, as above */
typedef struct ppgpu_ribbon_water_record { /* 64 bytes */
    double length, pitch;                  /* len, len / n (0 for a degenerate ribbon) */
    uint32_t samples, wet_samples;         /* n + 1 (1 for a degenerate ribbon); wet: ad != NONE */
    int32_t nearest_sample, farthest_sample;   /* lowest index attaining min_ad / max_ad over the wet samples; -1 without one */
    uint32_t min_ad, max_ad, start_ad, end_ad; /* NONE where there is none; start/end = sample 0 / the last sample */
    uint32_t lim2, flags;                  /* PPGPU_RW_* */
    double nearest_metres;                 /* resolution * min_ad / 12; +infinity without a wet sample */
} ppgpu_ribbon_water_record;
/* One record per ribbon of h_ribbons4 (n rows of {sx, sy, ex, ey}) against the map of the current seed.  PPGPU_ESTATE without a seed.
 * PPGPU_EINVAL for a NaN anywhere, a ribbon with more than 2^22 samples, ribbon_width + resolution / 4 above 255 cells and
 * lim2 > PPGPU_WATER_MAX_LIM2.  Synchronous. */
int ppgpu_ribbon_water_host(ppgpu_ctx* ctx, int32_t n, const double* h_ribbons4, double ribbon_width, ppgpu_ribbon_water_record* h_records);
/* Measurement aid: with timing on (ppgpu_enable_timing), the milliseconds of the last build of the map (from the fill to the totals:
 * the host's reads of the rounds' active counts between the batches of launches are inside) and of the last ribbon walk; -1 for each
 * that was not timed since ppgpu_enable_timing.  PPGPU_ESTATE with timing off.  Waits for the stream. */
int ppgpu_last_water_timing(ppgpu_ctx* ctx, double* ms_map, double* ms_ribbons);

/* ---------------------------------------------------------------- route by water */

/* Which way the distance by water goes: the cheapest path that the water map of the current seed (above) holds implicitly, made
 * explicit as a step map and walked on the device per query point.  Per route: its length, its turning points, its narrowest place
 * and the direction in which it leaves the seed.  Everything is exact in integers; the only floating point is in the two metres fields.
 * STEP CODES.  Codes 0 .. 7 stand for the offsets (dr, dc) = N(-1,0), S(+1,0), W(0,-1), E(0,+1), NW(-1,-1), NE(-1,+1), SW(+1,-1), SE(+1,+1);
 * the cost is PPGPU_WATER_STEP for codes 0-3 and PPGPU_WATER_DIAG for codes 4-7.  The opposite of a code: N<->S, W<->E, NW<->SE, NE<->SW.
 * STEP MAP, one byte per cell over the water map wd: dir(cell) = PPGPU_ROUTE_NONE where wd == PPGPU_WATER_NONE, PPGPU_ROUTE_SEED on the
 * seed's cell, otherwise the LOWEST code k whose neighbour lies in the grid, has a distance and satisfies
 * wd(neighbour) + cost(k) == wd(cell).  One such neighbour always exists (wd is the fixed point of the relaxation); the lowest code
 * prefers a straight step on a tie.  The map is canonical: any correct algorithm writes the same bytes.
 * APPROACH CELL of a query point with limit lim2: A is the cell Map::isBlocked puts the point in (GridWorldMap.cpp:84-93); a point
 * outside the grid has none.  With lim2 == 0, B = A.  With lim2 >= 1, B is the cell of the grid with gap2(A, B) < lim2 (gap2 as under
 * "chart clearance") that has the smallest wd; on a tie the lowest row-major index wins.  lim2 > PPGPU_WATER_MAX_LIM2 is refused.  For a
 * ribbon's sample, wd(B) is its approach distance ad.
 * ROUTE.  The cells from B to the seed's cell, following dir: wd falls by the step's cost at every step, so the route ends after at most
 * wd(B) / 12 steps.  A TURN is a cell of the route, other than its two ends, whose incoming and outgoing codes differ.  The VERTICES are
 * the seed's cell, the turns and B, listed FROM THE SEED: turns + 2 of them, 1 when B is the seed's cell, 0 without an approach cell.
 * RECORD.  first_dir = code | flags << 8: the code of the first step leaving the seed (the opposite of the walk's last code),
 * PPGPU_ROUTE_SEED when B is the seed's cell, 0xFF for a dry record; the PPGPU_WR_* flags are in bits 8-15.  min_gap2 is the smallest
 * value of the distance map of the occupancy grid AS SET (ppgpu_get_grid_distance, built on first use) over all cells of the route,
 * both ends included; min_gap2_cell the cell that attains it, on a tie the one nearest the seed along the route.  A dry record has
 * metres and narrowest_metres +infinity, min_gap2 and min_gap2_cell NONE, wd and from_cell NONE and all counts 0.
 * VERTICES ARRAY: n * vertex_stride cell indices; slot i * vertex_stride + j holds vertex j of route i, seed first, for
 * j < vertices_written = min(vertices, vertex_stride); the other slots are left as they were.  A truncated route keeps the end near
 * the seed, which is where the vehicle goes first.
 * Lazy and derived: the step map (one byte per cell) is built by the first call below after the water map was built or rebuilt; a
 * moved seed, a new grid and a changed keep-out limit make it stale through the water map.  A handle that never makes these calls
 * allocates and launches nothing for them. */
#define PPGPU_ROUTE_NONE 0xFFu
#define PPGPU_ROUTE_SEED 8u
#define PPGPU_WR_DRY       0x01u  /* no approach cell has a distance */
#define PPGPU_WR_OUTSIDE   0x02u  /* the point is outside the grid (implies PPGPU_WR_DRY) */
#define PPGPU_WR_AT_SEED   0x04u  /* B is the seed's cell */
#define PPGPU_WR_TRUNCATED 0x08u  /* vertices > vertex_stride */
#define PPGPU_WR_NO_SEED   0x40u  /* the seed is blocked: nothing judged, cells NONE, counts 0, +infinity metres */
#define PPGPU_WR_NO_MAP    0x80u  /* base Map: nothing judged, as above */
typedef struct ppgpu_water_route_record {  /* 64 bytes */
    uint32_t point_cell, from_cell;        /* A and B, row-major; PPGPU_WATER_NONE where there is none */
    uint32_t wd, lim2;                     /* wd(B) (NONE without B); the limit as passed */
    uint32_t straight_steps, diagonal_steps;   /* 12 * straight + 17 * diagonal == wd */
    uint32_t turns, vertices;              /* vertices: the total, whatever the stride */
    uint32_t vertices_written, first_dir;  /* min(vertices, vertex_stride); first_dir = code | flags << 8 (above) */
    uint32_t min_gap2, min_gap2_cell;      /* above */
    double metres;                         /* resolution * ((double)straight + (double)diagonal * sqrt(2)) */
    double narrowest_metres;               /* resolution * sqrt((double)min_gap2) */
} ppgpu_water_route_record;
/* For tests and tools: the step map of the current seed, rows*cols bytes.  PPGPU_ESTATE without a seed; PPGPU_EINVAL without a grid
 * (rows == 0) or when capacity < rows*cols.  Synchronous. */
int ppgpu_get_grid_water_dirs(ppgpu_ctx* ctx, uint8_t* h_out, int64_t capacity);
/* One record per point {x, y} of h_xy2 and up to vertex_stride vertices per route into h_vertices (may be NULL with vertex_stride 0).
 * PPGPU_ESTATE without a water seed.  PPGPU_EINVAL for a NaN, n < 0, vertex_stride < 0, vertex_stride > 0 with h_vertices == NULL and
 * lim2 > PPGPU_WATER_MAX_LIM2.  n == 0 is a no-op.  A blocked seed or the base Map gives records with PPGPU_WR_NO_SEED or
 * PPGPU_WR_NO_MAP and no launch.  PPGPU_ECAPACITY if a walk ran into its bound of wd(B) / 12 + 2 rounds (it cannot).  Synchronous. */
int ppgpu_water_routes_host(ppgpu_ctx* ctx, int64_t n, const double* h_xy2, uint32_t lim2, int32_t vertex_stride,
                            ppgpu_water_route_record* h_records, uint32_t* h_vertices);
/* Measurement aid: with timing on, the milliseconds of the last build of the step map and of the last route walk; -1 for each that
 * was not timed since ppgpu_enable_timing.  PPGPU_ESTATE with timing off.  Waits for the stream. */
int ppgpu_last_water_route_timing(ppgpu_ctx* ctx, double* ms_dirs, double* ms_routes);

/* Number of edges a dense launch with these arguments produces. */
int64_t ppgpu_dense_edge_count(int32_t nv, int64_t ns, uint32_t cfg_mask);

/* ---------------------------------------------------------- incumbent selection */

/* Best (smallest f, ties -> smallest edge index) feasible edge of the last costing
 * launch — the batch analogue of the incumbent update AStarPlanner.cpp:109-117.
 * goal_only != 0 restricts to children satisfying goalCondition.
 * d_key2 (device, 2 x uint64) = { bit pattern of f (monotone for f >= 0), edge index },
 * UINT64_MAX/UINT64_MAX when no edge qualifies.  Asynchronous. */
int ppgpu_best_edge(ppgpu_ctx* ctx, int64_t n, const ppgpu_edge_result* d_results,
                    int32_t goal_only, uint64_t edge_index_base, uint64_t* d_key2);

/* Lexicographic min of n keys {f bits, edge index} resident on the device into d_key2 — the
 * combine step after an all-gather issued on the caller's own communicator. Asynchronous. */
int ppgpu_key_min(ppgpu_ctx* ctx, int32_t n, const uint64_t* d_keys, uint64_t* d_key2);

/* The communicator of a sharded iteration (SURVEY.md 8 e: the sample batch is split over the GPUs of a node, every rank
 * costs the edges to its own samples, the incumbents are combined once per iteration).  The reference has no counterpart:
 * its incumbent update is AStarPlanner.cpp:109-117 on one thread.  RCCL is loaded at the first call (dlopen), so a
 * single-GPU user never needs it.
 *   one process per GPU:  rank 0 calls ppgpu_comm_unique_id and hands the 128 bytes to the other ranks by any means (a
 *     file, a TCP store, MPI); every rank then calls ppgpu_comm_init_rank on its own handle (collective: returns when all
 *     world ranks have called it).
 *   one process, several GPUs:  ppgpu_comm_init_all on the n handles (one per device, rank i = ctxs[i]); each handle's
 *     ppgpu_allreduce_best must then be issued from its own host thread (the call blocks until every rank has joined).
 * ppgpu_comm_info reads the size and this handle's rank back from RCCL (ncclCommCount / ncclCommUserRank).
 * The handle owns its communicator; ppgpu_destroy releases it.  ppgpu_comm_init_all either gives every handle a communicator
 * or none (on failure the communicators already made are destroyed again). */
#define PPGPU_COMM_ID_BYTES 128
int ppgpu_comm_unique_id(uint8_t* h_id128);
int ppgpu_comm_init_rank(ppgpu_ctx* ctx, int32_t world, int32_t rank, const uint8_t* h_id128);
int ppgpu_comm_init_all(ppgpu_ctx** ctxs, int32_t n);
int ppgpu_comm_info(ppgpu_ctx* ctx, int32_t* world, int32_t* rank);
int ppgpu_comm_destroy(ppgpu_ctx* ctx);
/* ncclCommAbort on the handle's communicator: gives it up WITHOUT waiting for outstanding collectives, which releases a rank
 * that is waiting in a collective another rank never joined (its own failure came first).  Callable from any host thread. */
int ppgpu_comm_abort(ppgpu_ctx* ctx);

/* Global incumbent across the ranks of one node: lexicographic min of the
 * per-rank keys with one RCCL collective over xGMI (all-gather of 16 bytes per rank, then ppgpu_key_min; RCCL has no
 * MINLOC and 64 bits cannot carry a full-precision f and an index).  rccl_comm is an ncclComm_t created by the caller,
 * or NULL for the handle's own communicator (ppgpu_comm_init_*).  In place on d_key2, asynchronous on the handle's stream. */
int ppgpu_allreduce_best(ppgpu_ctx* ctx, void* rccl_comm, uint64_t* d_key2);

#ifdef __cplusplus
}
#endif

#endif
