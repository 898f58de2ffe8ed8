// pp_k_trace.h — pp_k_trace_steps: what happened along an edge, one 64-byte ppgpu_step_record per executed step of the sweep of
// Edge::computeTrueCost (Edge.cpp:125-175).  Included by pp_kernels.h.
#pragma once
// The costing launch answers "what does this edge cost"; its sweeps skip every chunk of steps that provably changes nothing and
// keep no poses.  This kernel runs AFTER a costing launch over the same edge list, on the same PPEdgeSetup records, and does not
// skip: for step k = 0 .. steps - 1 (steps = bits 16-31 of the record's info: the costing launch already knows where the loop
// stopped — a blocked cell, the end time, coverage completed — so there is no coverage state machine and no heuristic here)
//     the pose            pp_window_pose, the sweeps' own segment arithmetic on the same 64-step windows: the same doubles
//     the time            the vertex's row of the time grid (the reference's repeated `time += timeIncrement`, bit for bit)
//     isBlocked           pp_is_blocked at that pose (Edge.cpp:144)
//     collisionExists     pp_obstacle_hits_chunk / pp_obstacle_density_chunk at that pose and time (:150-151); 0 on a blocked step
//     penalty_before      the collision penalty accrued BEFORE the step (the term in gSoFar, :138): an exclusive scan over the wave
//                         plus a carry from chunk to chunk — the only dependence between steps.  Binary model: a scan of the integer
//                         hit counts, times the factor once (how the costing record forms its penalty: the two agree exactly).
// One wavefront per edge, walking its steps 64 at a time.  A wave's 64 records are 4 KB contiguous: the lanes put their records
// into LDS as four 16-byte pieces each and the wave stores the 4 KB as four fully coalesced 16-byte-per-lane vector stores
// (a lane storing its own record would touch 32 lines per instruction, a quarter of each).
#define PP_TRACE_WPB 4
#define PP_TRACE_LDS_STRIDE 65     // 16-byte units between the four pieces of the records in LDS (odd: spreads the banks)
static_assert(sizeof(ppgpu_step_record) == 64, "a step record is 64 bytes: four 16-byte stores");

__device__ __forceinline__ int pp_wave_excl_scan_i(int v, int lane, int& total) {
    int s = v;
#pragma unroll
    for (int o = 1; o < PP_WAVE; o <<= 1) { const int u = __shfl_up(s, o, PP_WAVE); if (lane >= o) s += u; }
    total = pp_readlane_i(s, PP_WAVE - 1);
    return s - v;
}
__device__ __forceinline__ double pp_wave_excl_scan_d(double v, int lane, double& total) {
    double s = v;
#pragma unroll
    for (int o = 1; o < PP_WAVE; o <<= 1) { const double u = __shfl_up(s, o, PP_WAVE); if (lane >= o) s += u; }
    total = pp_readlane(s, PP_WAVE - 1);
    const double before = __shfl_up(s, 1, PP_WAVE);
    return lane == 0 ? 0.0 : before;
}

// el = the edge's position in the slice; lds = this wave's 4 * PP_TRACE_LDS_STRIDE double2
template <bool GAUSSIAN>
__device__ __forceinline__ void pp_trace_edge(const PPParams& p, const long long el, ppgpu_step_record* steps, const long long step_base,
                                              const int stride, int* counts, double2* lds) {
    const int lane = pp_lane();
    const long long e = p.ws_base + el;                                   // slot in the workspace
    const long long eg = pp_edge_position(p, p.e_base + el);              // position in the caller's list
    const PPEdgeSetup* S = p.setup + e;
    const ppgpu_edge_result* rec = p.out + eg;
    const unsigned rflags = (unsigned)pp_const_i32(&rec->flags)[0], info = (unsigned)pp_const_i32(&rec->info)[0];
    const unsigned sflags = (unsigned)PP_SI32(sflags);
    const int dubType = PP_SI32(type);
    int count = (int)(info >> 16);
    if ((sflags & (PP_SETUP_MALFORMED | PP_SETUP_COLOCATED)) || dubType < 0 || (rflags & PPGPU_F_THROWS)) count = 0;
    if (count > p.ng) count = p.ng;                                       // (a step has a time: never more steps than the grid holds)
    if (lane == 0) counts[eg] = count;
    const int nw = count < stride ? count : stride;                       // records written: the ribbon_stride idiom
    if (nw <= 0) return;
    const unsigned vi = (unsigned)PP_SI32(vi);
    const double srcH = pp_sgpr(p.verts[vi].heading);
    const PPCurveHot hot = pp_curve_hot(S);
    const double* tg = p.tgrid + (size_t)vi * p.ng;
    int cur = 0;
    PPSeg cs = pp_seg_load_uniform(&S->seg[0], 0, PP_SF64(p0), PP_SF64(p1), PP_SF64(hi1), PP_SI32(type));
    const double chunkTime = 64.0 * (p.inc_d / p.max_speed);
    const double chunkSpan = chunkTime * hot.speed;
    double carryHeading = srcH;                                           // `lastHeading`, Edge.cpp:96
    int carryHits = 0;
    double carryPen = 0.0;
    bool dubErr = false;
    double2* out = reinterpret_cast<double2*>(steps + (size_t)(eg - step_base) * (size_t)stride);
    for (int base = 0; base < nw; base += PP_WAVE) {
        const int k = base + lane;
        const bool valid = k < nw;
        const double t = tg[valid ? k : base];
        const double tFirst = pp_readlane(t, 0);
        double x, y, uth;
        pp_window_pose(S, hot, cur, cs, t, tFirst, valid, x, y, uth, dubErr);
        const double heading = pp_heading_from_yaw(pp_mod2pi(uth));        // DubinsWrapper.cpp:47
        const bool blk = valid & pp_is_blocked(p.grid, x, y);              // Edge.cpp:144
        double collision = 0.0, before;
        if (!GAUSSIAN) {
            int hits = 0;
            if (p.n_obst > 0)
                hits = pp_obstacle_hits_chunk(p.obst, p.n_obst, x, y, t, valid, pp_readlane(x, 0), pp_readlane(y, 0), tFirst, chunkSpan, chunkTime);
            if (blk) hits = 0;                                             // the loop broke before :150
            int total;
            const int excl = pp_wave_excl_scan_i(hits, lane, total);
            before = (double)(carryHits + excl) * p.cpf;
            carryHits += total;
            collision = (double)hits;
        } else {
            double dens = pp_obstacle_density_chunk(reinterpret_cast<const PPGauss*>(p.obst), p.n_obst, x, y, t, valid, pp_readlane(x, 0),
                                                    pp_readlane(y, 0), tFirst, chunkSpan, chunkTime);
            if (blk) dens = 0.0;
            double total;
            before = carryPen + pp_wave_excl_scan_d(dens * p.cpf, lane, total);
            carryPen += total;
            collision = dens;
        }
        double prevHeading = __shfl_up(heading, 1, PP_WAVE);
        if (lane == 0) prevHeading = carryHeading;
        carryHeading = pp_readlane(heading, PP_WAVE - 1);
        const unsigned sf = (blk ? PPGPU_S_BLOCKED : 0u) | (prevHeading == heading ? PPGPU_S_STRAIGHT : 0u);   // :144, :159
        // the record, as four 16-byte pieces: {x, y} {heading, time} {collision, penalty_before} {flags | step, reserved}
        lds[0 * PP_TRACE_LDS_STRIDE + lane] = make_double2(x, y);
        lds[1 * PP_TRACE_LDS_STRIDE + lane] = make_double2(heading, t);
        lds[2 * PP_TRACE_LDS_STRIDE + lane] = make_double2(collision, before);
        lds[3 * PP_TRACE_LDS_STRIDE + lane] = make_double2(__longlong_as_double((long long)(((unsigned long long)(unsigned)k << 32) | (unsigned long long)sf)), 0.0);
        pp_wave_lds_fence();
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = j * PP_WAVE + lane;                              // 16-byte piece q of the chunk's 4 KB
            const int r = q >> 2;                                          // ... belongs to the record of step base + r
            const double2 v = lds[(q & 3) * PP_TRACE_LDS_STRIDE + r];
            if (base + r < nw) out[(size_t)base * 4 + q] = v;
        }
        pp_wave_lds_fence();
    }
}

// n_edges = slice size; steps[(edge - step_base) * stride + k]; counts[edge]
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_steps(PPParams p, ppgpu_step_record* steps, long long step_base, int stride, int* counts) {
    __shared__ double2 s_rec[PP_TRACE_WPB][4 * PP_TRACE_LDS_STRIDE];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long el = (long long)blockIdx.x * PP_TRACE_WPB + wave;
    if (el >= p.n_edges) return;
    pp_trace_edge<false>(p, el, steps, step_base, stride, counts, s_rec[wave]);
}
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_steps_gaussian(PPParams p, ppgpu_step_record* steps, long long step_base, int stride, int* counts) {
    __shared__ double2 s_rec[PP_TRACE_WPB][4 * PP_TRACE_LDS_STRIDE];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long el = (long long)blockIdx.x * PP_TRACE_WPB + wave;
    if (el >= p.n_edges) return;
    pp_trace_edge<true>(p, el, steps, step_base, stride, counts, s_rec[wave]);
}
