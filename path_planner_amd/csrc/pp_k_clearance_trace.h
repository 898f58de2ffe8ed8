// pp_k_clearance_trace.h — pp_k_trace_clearance: how close an edge comes to a charted hazard, one 64-byte ppgpu_clearance_record
// per edge: the smallest gap2 (pp_k_distance.h) over the executed steps of the sweep of Edge::computeTrueCost (Edge.cpp:125-175),
// where and when it is attained, and how many steps lie inside a margin.  Included by pp_kernels.h.
#pragma once
// The costing launch asks Map::isBlocked at every sampled pose (Edge.cpp:144); this kernel asks the distance map at the same poses, on
// the shared trace core (pp_k_trace_common.h): the step count is pp_trace_head's and the windows are pp_trace_window's, without
// headings, so the steps and poses are those of the step trace (the same doubles).  Per window, lane = step: the gap2 of the step's
// cell (pp_pose_gap2, every lane of the wave in it) and the lane's smallest key (gap2 << 32) | step so far, with the pose and time
// that go with it; the steps below the margin are counted from a ballot.  One wave min-reduction of the keys at the end: the step
// is in the key, so the earliest step wins on equal gap2 and exactly one lane holds the minimum.  That lane stores the record.
static_assert(sizeof(ppgpu_clearance_record) == 64, "a clearance record is 64 bytes: four 16-byte stores");

__device__ __forceinline__ double pp_pack_i32(unsigned lo, unsigned hi) {
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
}

// el = the edge's position in the slice; limit2: a step is below the margin iff its gap2 < limit2 (0: none is)
__device__ __forceinline__ void pp_clearance_trace_edge(const PPParams& p, const long long el, const uint16_t* dist, const unsigned limit2,
                                                        ppgpu_clearance_record* recs, const long long rec_base, int* counts) {
    const int lane = pp_lane();
    const PPTraceHead h = pp_trace_head(p, el);
    const int count = h.count;
    if (lane == 0) counts[h.eg] = count;
    // the record, as four 16-byte pieces: {clearance, time} {x, y} {first_below_time, step | gap2} {below_steps | first_below_step, flags | reserved}
    double2* out = reinterpret_cast<double2*>(recs + (size_t)(h.eg - rec_base));
    if (count <= 0) {
        if (lane == 0) {
            out[0] = make_double2(-1.0, -1.0);
            out[1] = make_double2(0.0, 0.0);
            out[2] = make_double2(-1.0, pp_pack_i32(0xFFFFFFFFu, 0u));
            out[3] = make_double2(pp_pack_i32(0u, 0xFFFFFFFFu), pp_pack_i32(PPGPU_CL_EMPTY, 0u));
        }
        return;
    }
    const bool nomap = p.grid.rows == 0;                                   // the base Map charts nothing: every step is at the cap
    const double inv_wpr = nomap ? 0.0 : 1.0 / (double)p.grid.wpr;
    unsigned long long best = ~0ull;
    double bx = 0.0, by = 0.0, bt = 0.0;
    int below = 0, firstK = -1;
    double firstT = -1.0;
    bool blockedLast = false;
    PPTraceWalk walk = pp_trace_walk_begin(h, 0.0);
    for (int base = 0; base < count; base += PP_WAVE) {
        const PPTraceWindow n = pp_trace_window<false>(p, h, walk, base, count);
        unsigned g2 = PPGPU_DIST_CAP2;
        if (!nomap) g2 = pp_pose_gap2(p.grid, dist, inv_wpr, n.x, n.y);    // (wave-uniform branch: the ballot inside sees every lane)
        const unsigned long long key = n.valid ? (((unsigned long long)g2 << 32) | (unsigned long long)(unsigned)n.k) : ~0ull;
        if (key < best) { best = key; bx = n.x; by = n.y; bt = n.t; }
        const unsigned long long bl = __ballot(n.valid && g2 < limit2);
        if (bl != 0ull) {
            if (firstK < 0) {
                const int src = __ffsll((unsigned long long)bl) - 1;
                firstK = base + src;
                firstT = pp_readlane(n.t, src);
            }
            below += __popcll(bl);
        }
        blockedLast = blockedLast | (__ballot(n.blocked && n.k == count - 1) != 0ull);   // Edge.cpp:144-146: only ever the last step
    }
    unsigned long long m = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(m, o, PP_WAVE);
        m = u < m ? u : m;
    }
    if (best != m) return;                                                 // count > 0: some lane holds a step, and one lane holds this one
    const unsigned gap2 = (unsigned)(m >> 32);
    const unsigned flags = (blockedLast ? PPGPU_CL_BLOCKED : 0u) | (gap2 == PPGPU_DIST_CAP2 ? PPGPU_CL_CAPPED : 0u) | (nomap ? PPGPU_CL_NO_MAP : 0u);
    const double clearance = nomap ? PP_DBL_MAX : p.grid.res * sqrt((double)gap2);
    out[0] = make_double2(clearance, bt);
    out[1] = make_double2(bx, by);
    out[2] = make_double2(firstT, pp_pack_i32((unsigned)m, gap2));
    out[3] = make_double2(pp_pack_i32((unsigned)below, (unsigned)firstK), pp_pack_i32(flags, 0u));
}

// n_edges = slice size; recs[edge - rec_base]; counts[edge]
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_clearance(PPParams p, const uint16_t* dist, unsigned limit2, ppgpu_clearance_record* recs,
                                                                          long long rec_base, int* counts) {
    int wave;
    long long el;
    if (pp_trace_entry(p, wave, el)) pp_clearance_trace_edge(p, el, dist, limit2, recs, rec_base, counts);
}
