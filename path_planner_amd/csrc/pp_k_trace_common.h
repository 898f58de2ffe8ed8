// pp_k_trace_common.h — what the edge traces (pp_k_trace.h, pp_k_cover_trace.h, pp_k_contact_trace.h, pp_k_clearance_trace.h) share: which edge a wave
// has, how many steps it walks, the poses of a 64-step window and how a window's records leave.  Included by pp_kernels.h before them.
#pragma once
// A trace kernel runs AFTER a costing launch over the same edge list, on the same PPEdgeSetup records, one wavefront per edge, and
// does not skip.  They must see the same steps and the same poses as each other and as the costing launch, bit for bit, so
// the step count (pp_trace_head) and the window (pp_trace_window: pp_window_pose, the sweeps' own segment arithmetic, with the
// state it carries from window to window) exist here once.
#define PP_TRACE_WPB 4             // waves (edges) per workgroup
#define PP_TRACE_LDS_STRIDE 65     // 16-byte units between the pieces of the records in LDS (odd: spreads the banks)

// The edge of this wave: el = its position in the slice.  False past the end of the slice.
__device__ __forceinline__ bool pp_trace_entry(const PPParams& p, int& wave, long long& el) {
    el = pp_wave_edge<PP_TRACE_WPB>(wave);
    return el < p.n_edges;
}

struct PPTraceHead {
    long long e, eg;               // slot in the workspace, position in the caller's list
    const PPEdgeSetup* S;
    unsigned rflags, sflags;       // the costed record's flags, the setup record's
    bool throws;                   // the reference throws out of computeTrueCost: no step is reported
    int count;                     // executed steps: bits 16-31 of the record's info, 0 on a throwing edge, never more than the time grid holds
    unsigned vi;
    const double* tg;              // the vertex's row of the time grid
    PPCurveHot hot;
    double chunkTime, chunkSpan;   // what the chunk obstacle functions take: the time and the distance of 64 steps
};
__device__ __forceinline__ PPTraceHead pp_trace_head(const PPParams& p, const long long el) {
    PPTraceHead h;
    h.e = p.ws_base + el;
    h.eg = pp_edge_position(p, p.e_base + el);
    const PPEdgeSetup* S = h.S = p.setup + h.e;
    const ppgpu_edge_result* rec = p.out + h.eg;
    h.rflags = (unsigned)pp_const_i32(&rec->flags)[0];
    const unsigned info = (unsigned)pp_const_i32(&rec->info)[0];
    h.sflags = (unsigned)PP_SI32(sflags);
    h.throws = (h.sflags & (PP_SETUP_MALFORMED | PP_SETUP_COLOCATED)) || PP_SI32(type) < 0 || (h.rflags & PPGPU_F_THROWS);
    h.count = h.throws ? 0 : (int)(info >> 16);   // the costing launch already knows where the loop stopped
    if (h.count > p.ng) h.count = p.ng;           // (a step has a time: never more steps than the grid holds)
    h.vi = (unsigned)PP_SI32(vi);
    h.tg = p.tgrid + (size_t)h.vi * p.ng;
    h.hot = pp_curve_hot(S);
    h.chunkTime = 64.0 * (p.inc_d / p.max_speed);
    h.chunkSpan = h.chunkTime * h.hot.speed;
    return h;
}

// What a walk carries from one window to the next: the segment pp_window_pose is on, and `lastHeading` (Edge.cpp:96).
struct PPTraceWalk {
    int cur;
    PPSeg cs;
    bool dubErr;
    double carryHeading;
};
// srcHeading: the heading of the edge's vertex (a walk without headings never reads it)
__device__ __forceinline__ PPTraceWalk pp_trace_walk_begin(const PPTraceHead& h, const double srcHeading) {
    const PPEdgeSetup* S = h.S;
    return PPTraceWalk{0, pp_seg_load_uniform(&S->seg[0], 0, PP_SF64(p0), PP_SF64(p1), PP_SF64(hi1), PP_SI32(type)), false, srcHeading};
}

// One window, lane = step k.  Lanes past the limit redo lane 0's step and are not valid.
struct PPTraceWindow {
    int k;
    bool valid;
    double t, tFirst;              // the step's time (the reference's repeated `time += timeIncrement`, bit for bit), lane 0's
    double x, y, heading;
    bool blocked, straight;        // Edge.cpp:144; the heading is that of the step before (:159)
};
// The 64 steps from `base` of a walk to `limit` steps.  HEADING = false: heading and straight are not computed (0, false).
template <bool HEADING>
__device__ __forceinline__ PPTraceWindow pp_trace_window(const PPParams& p, const PPTraceHead& h, PPTraceWalk& w, const int base, const int limit) {
    const int lane = pp_lane();
    PPTraceWindow n;
    n.k = base + lane;
    n.valid = n.k < limit;
    n.t = h.tg[n.valid ? n.k : base];
    n.tFirst = pp_readlane(n.t, 0);
    double uth;
    pp_window_pose(h.S, h.hot, w.cur, w.cs, n.t, n.tFirst, n.valid, n.x, n.y, uth, w.dubErr);
    n.heading = 0.0;
    n.straight = false;
    if (HEADING) {
        n.heading = pp_heading_from_yaw(pp_mod2pi(uth));                   // DubinsWrapper.cpp:47
        double prevHeading = __shfl_up(n.heading, 1, PP_WAVE);
        if (lane == 0) prevHeading = w.carryHeading;
        w.carryHeading = pp_readlane(n.heading, PP_WAVE - 1);
        n.straight = prevHeading == n.heading;
    }
    n.blocked = n.valid & pp_is_blocked(p.grid, n.x, n.y);
    return n;
}
// collisionExists at the window's poses and times (Edge.cpp:150-151), binary and Gaussian model
__device__ __forceinline__ int pp_trace_hits(const PPParams& p, const PPTraceHead& h, const PPTraceWindow& n) {
    return pp_obstacle_hits_chunk(p.obst, p.n_obst, n.x, n.y, n.t, n.valid, pp_readlane(n.x, 0), pp_readlane(n.y, 0), n.tFirst, h.chunkSpan, h.chunkTime);
}
__device__ __forceinline__ double pp_trace_density(const PPParams& p, const PPTraceHead& h, const PPTraceWindow& n) {
    return pp_obstacle_density_chunk(reinterpret_cast<const PPGauss*>(p.obst), p.n_obst, n.x, n.y, n.t, n.valid, pp_readlane(n.x, 0), pp_readlane(n.y, 0),
                                     n.tFirst, h.chunkSpan, h.chunkTime);
}

// 64 records of PIECES 16-byte pieces each are contiguous in memory (4 KB or 2 KB).  Lane l has put piece i of its record at
// lds[i * PP_TRACE_LDS_STRIDE + l]; the wave stores them as PIECES fully coalesced 16-byte-per-lane vector stores (a lane storing its
// own 64-byte record would touch 32 lines per instruction, a quarter of each).  out = record 0 of the edge; the records are
// first .. first + 63, and those from n_valid on are not written.
template <int PIECES>
__device__ __forceinline__ void pp_trace_store(const double2* lds, double2* out, const int first, const int n_valid) {
    static_assert(PIECES == 2 || PIECES == 4, "a record is two or four 16-byte pieces");
    const int lane = pp_lane();
    pp_wave_lds_fence();
#pragma unroll
    for (int j = 0; j < PIECES; j++) {
        const int q = j * PP_WAVE + lane;                                  // 16-byte piece q of the 64 records
        const int r = q >> (PIECES / 2);                                   // ... belongs to record first + r
        const double2 v = lds[(q & (PIECES - 1)) * PP_TRACE_LDS_STRIDE + r];
        if (first + r < n_valid) out[(size_t)first * PIECES + q] = v;
    }
    pp_wave_lds_fence();
}
