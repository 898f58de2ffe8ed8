// pp_k_trace.h — pp_k_trace_steps: what happened along an edge, one 64-byte ppgpu_step_record per executed step of the sweep of
// Edge::computeTrueCost (Edge.cpp:125-175).  Included by pp_kernels.h.
#pragma once
// The costing launch answers "what does this edge cost"; its sweeps skip every chunk of steps that provably changes nothing and
// keep no poses.  This kernel walks every step on the shared trace core (pp_k_trace_common.h): for step k = 0 .. steps - 1 (steps =
// pp_trace_head's count: the costing launch already knows where the loop stopped — a blocked cell, the end time, coverage completed
// — so there is no coverage state machine and no heuristic here)
//     pose, time, heading, isBlocked, straight      pp_trace_window
//     collisionExists     pp_obstacle_hits_chunk / pp_obstacle_density_chunk at that pose and time (:150-151); 0 on a blocked step
//     penalty_before      the collision penalty accrued BEFORE the step (the term in gSoFar, :138): an exclusive scan over the wave
//                         plus a carry from chunk to chunk — the only dependence between steps.  Binary model: a scan of the integer
//                         hit counts, times the factor once (how the costing record forms its penalty: the two agree exactly).
// A window's 64 records are 4 KB contiguous and leave through pp_trace_store.
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
    const PPTraceHead h = pp_trace_head(p, el);
    if (lane == 0) counts[h.eg] = h.count;
    const int nw = h.count < stride ? h.count : stride;                   // records written: the ribbon_stride idiom
    if (nw <= 0) return;
    PPTraceWalk walk = pp_trace_walk_begin(h, pp_sgpr(p.verts[h.vi].heading));
    int carryHits = 0;
    double carryPen = 0.0;
    double2* out = reinterpret_cast<double2*>(steps + (size_t)(h.eg - step_base) * (size_t)stride);
    for (int base = 0; base < nw; base += PP_WAVE) {
        const PPTraceWindow n = pp_trace_window<true>(p, h, walk, base, nw);
        double collision = 0.0, before;
        if (!GAUSSIAN) {
            int hits = 0;
            if (p.n_obst > 0) hits = pp_trace_hits(p, h, n);
            if (n.blocked) hits = 0;                                       // the loop broke before :150
            int total;
            const int excl = pp_wave_excl_scan_i(hits, lane, total);
            before = (double)(carryHits + excl) * p.cpf;
            carryHits += total;
            collision = (double)hits;
        } else {
            double dens = pp_trace_density(p, h, n);
            if (n.blocked) dens = 0.0;
            double total;
            before = carryPen + pp_wave_excl_scan_d(dens * p.cpf, lane, total);
            carryPen += total;
            collision = dens;
        }
        const unsigned sf = (n.blocked ? PPGPU_S_BLOCKED : 0u) | (n.straight ? PPGPU_S_STRAIGHT : 0u);   // :144, :159
        // the record, as four 16-byte pieces: {x, y} {heading, time} {collision, penalty_before} {flags | step, reserved}
        lds[0 * PP_TRACE_LDS_STRIDE + lane] = make_double2(n.x, n.y);
        lds[1 * PP_TRACE_LDS_STRIDE + lane] = make_double2(n.heading, n.t);
        lds[2 * PP_TRACE_LDS_STRIDE + lane] = make_double2(collision, before);
        lds[3 * PP_TRACE_LDS_STRIDE + lane] = make_double2(__longlong_as_double((long long)(((unsigned long long)(unsigned)n.k << 32) | (unsigned long long)sf)), 0.0);
        pp_trace_store<4>(lds, out, base, nw);
    }
}

// n_edges = slice size; steps[(edge - step_base) * stride + k]; counts[edge]
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_steps(PPParams p, ppgpu_step_record* steps, long long step_base, int stride, int* counts) {
    __shared__ double2 s_rec[PP_TRACE_WPB][4 * PP_TRACE_LDS_STRIDE];
    int wave;
    long long el;
    if (pp_trace_entry(p, wave, el)) pp_trace_edge<false>(p, el, steps, step_base, stride, counts, s_rec[wave]);
}
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_steps_gaussian(PPParams p, ppgpu_step_record* steps, long long step_base, int stride, int* counts) {
    __shared__ double2 s_rec[PP_TRACE_WPB][4 * PP_TRACE_LDS_STRIDE];
    int wave;
    long long el;
    if (pp_trace_entry(p, wave, el)) pp_trace_edge<true>(p, el, steps, step_base, stride, counts, s_rec[wave]);
}
