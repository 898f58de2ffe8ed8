// pp_k_cover_trace.h — pp_k_trace_cover: what every step of an edge did to the ribbons, one 32-byte ppgpu_cover_record per executed
// step of the sweep of Edge::computeTrueCost (Edge.cpp:125-175) and one ppgpu_cover_summary per edge (the last cover, :181-191,
// included).  Included by pp_kernels.h.
#pragma once
// The cover sweep (pp_k_cover.h) visits event steps only and takes whole stretches of them as corridor, quiet and long runs; the
// step trace (pp_k_trace.h) has the poses but no coverage state machine.  This kernel is the state machine itself, executed
// literally, on the shared trace core (pp_k_trace_common.h): the step count is pp_trace_head's and the windows are pp_trace_window's,
// so the steps, poses, headings, straight and blocked bits are those of the step trace (the same doubles).  For step
// k = 0 .. steps - 1 it does what the reference does —
//     blocked (Edge.cpp:144-146)                        nothing: the loop broke before the coverage branch
//     toCoverDistance > increment (:153-154)            the literal subtraction, one per step
//     otherwise, an EVENT (:155-171)                    pp_ribbons_event at the step's pose: D = minDistanceFrom, then cover(pose, strict)
//                                                       when the edge covers or the heading did not change (:159); an emptied list
//                                                       sets coverageCompletedTime if it is still -1
// — with no skipping and no runs.  The lanes have a window's 64 poses, straight and blocked bits; the wave then walks the window's steps in a wave-uniform loop (a countdown step is a compare and a subtraction on
// wave-uniform values; an event step broadcasts its pose with a readlane and runs pp_ribbons_event across the lanes, ribbon i in
// lane i), lane j keeping step j's record.  The window's 64 records are 2 KB contiguous and leave through pp_trace_store.  toCoverDistance, lastHeading, the list, its length and coverageCompletedTime
// carry from window to window.  A step_stride below the edge's count cuts the records, not the walk: summary and final list are
// those of the whole edge.
static_assert(sizeof(ppgpu_cover_record) == 32 && sizeof(ppgpu_cover_summary) == 32, "cover records and summaries are two 16-byte pieces");

// sum of the end-to-end lengths of the n ribbons the lanes hold (wave-uniform)
__device__ __forceinline__ double pp_ribbons_total_length(const PPRibbon& r, int n) {
    return pp_sgpr(pp_wave_sum_d(pp_lane() < n ? sqrt(pp_sq_len(r.sx, r.sy, r.ex, r.ey)) : 0.0));
}

// One call of the else-branch of Edge.cpp:153-171 (or of the last cover, :182-184, with doCover = true) at (x, y).  Returns false
// when the list outgrew the wave's 64 ribbons.  changed: the list is not, value for value, what it was.
__device__ __forceinline__ bool pp_cover_trace_event(PPRibbon& rib, int& nrib, double w, double x, double y, bool doCover, double* lds,
                                                     double& D, bool& changed) {
    const PPRibbon old = rib;
    const int oldn = nrib;
    int adv;
    nrib = pp_ribbons_event(rib, nrib, w, x, y, doCover, lds, D, adv);
    D = pp_sgpr(D);
    changed = false;
    if (nrib > PP_WAVE) return false;
    if (doCover && oldn > 0 && adv != -2 && adv != -3)       // (-2 / -3: pp_ribbons_event left the list alone)
        changed = nrib != oldn ||
                  __ballot((pp_lane() < nrib) & ((rib.sx != old.sx) | (rib.sy != old.sy) | (rib.ex != old.ex) | (rib.ey != old.ey))) != 0ull;
    return true;
}

__device__ __forceinline__ void pp_cover_trace_summary(ppgpu_cover_summary* s, int events, int changes, int nrib, unsigned flags, double cct,
                                                       double remaining) {
    if (pp_lane() == 0) {
        s->events = events; s->changes = changes; s->ribbons_final = nrib; s->flags = flags;
        s->coverage_completed_time = cct; s->remaining_final = remaining;
    }
}

// el = the edge's position in the slice; lds_rec = this wave's 2 * PP_TRACE_LDS_STRIDE double2; lds_ev = its 64 x 4 doubles for pp_ribbons_event
__device__ __forceinline__ void pp_cover_trace_edge(const PPParams& p, const long long el, ppgpu_cover_record* recs, const long long rec_base,
                                                    const int stride, int* counts, ppgpu_cover_summary* sums, double* child, const int cstride,
                                                    double2* lds_rec, double* lds_ev) {
    const int lane = pp_lane();
    const PPTraceHead h = pp_trace_head(p, el);
    const PPEdgeSetup* S = h.S;
    const long long eg = h.eg;
    const int count = h.count;
    ppgpu_cover_summary* sum = sums + eg;
    if (h.throws) {
        // the reference throws out of computeTrueCost (Edge.cpp:178 at the latest, before the last cover): there is no child
        if (lane == 0) counts[eg] = 0;
        pp_cover_trace_summary(sum, 0, 0, 0, PPGPU_CS_THROWS, -1.0, 0.0);
        return;
    }
    const ppgpu_vertex* V = p.verts + h.vi;
    const bool cov = ((unsigned)PP_SI32(cbits) & PPGPU_EDGE_COVERAGE) != 0u;    // end()->coverageAllowed()
    double cct = pp_sgpr(V->coverage_completed_time);
    int nrib = __builtin_amdgcn_readfirstlane(V->ribbon_count);
    if (nrib > PP_WAVE || (h.rflags & PPGPU_F_RIBBON_LOST)) {            // a list the device cannot hold: refused before anything is written
        if (lane == 0) counts[eg] = 0;
        pp_cover_trace_summary(sum, 0, 0, 0, PPGPU_CS_REFUSED, -1.0, 0.0);
        return;
    }
    PPRibbon rib = {0, 0, 0, 0};
    if (lane < nrib) {
        const double* rp = p.ribbons + 4 * ((size_t)V->ribbon_offset + lane);
        rib.sx = rp[0]; rib.sy = rp[1]; rib.ex = rp[2]; rib.ey = rp[3];
    }
    const double w = p.ribw, inc_d = p.inc_d;
    double remaining = pp_ribbons_total_length(rib, nrib);
    double toCover = 0.0;                                                 // Edge.cpp:95
    int events = 0, changes = 0;
    // `intermediate` when the loop stops: the vertex's own state on an edge with no steps
    double lastX = pp_sgpr(V->x), lastY = pp_sgpr(V->y);
    bool lastBlocked = false, lastStraight = true;
    const int nw = count < stride ? count : stride;                       // records written: the ribbon_stride idiom
    double2* out = reinterpret_cast<double2*>(recs + (size_t)(eg - rec_base) * (size_t)stride);
    if (count > 0) {
        PPTraceWalk walk = pp_trace_walk_begin(h, pp_sgpr(V->heading));
        for (int base = 0; base < count; base += PP_WAVE) {
            const PPTraceWindow n = pp_trace_window<true>(p, h, walk, base, count);
            const unsigned long long blkMask = __ballot(n.blocked);                                 // Edge.cpp:144
            const unsigned long long strMask = __ballot(n.straight);                                // :159
            const int nsteps = (count - base) < PP_WAVE ? (count - base) : PP_WAVE;
            double myToCover = 0.0, myRemaining = 0.0;
            unsigned myFlags = 0u;
            int myRibbons = 0;
            for (int j = 0; j < nsteps; j++) {
                unsigned f = 0u;
                if (!((blkMask >> j) & 1ull)) {
                    if (toCover > inc_d) {
                        toCover -= inc_d;                                  // :153-154
                    } else {
                        const bool doCover = cov || ((strMask >> j) & 1ull) != 0ull;
                        bool changed;
                        double D;
                        if (!pp_cover_trace_event(rib, nrib, w, pp_readlane(n.x, j), pp_readlane(n.y, j), doCover, lds_ev, D, changed)) {
                            // (only where the literal walk splits a piece the costing launch's runs did not: records of earlier windows stay)
                            if (lane == 0) counts[eg] = 0;
                            pp_cover_trace_summary(sum, 0, 0, 0, PPGPU_CS_REFUSED, -1.0, 0.0);
                            return;
                        }
                        toCover = D;                                       // :158
                        f = PPGPU_C_EVENT | (doCover ? PPGPU_C_COVER : 0u) | (changed ? PPGPU_C_CHANGED : 0u);
                        events++;
                        if (changed) { changes++; remaining = pp_ribbons_total_length(rib, nrib); }
                        if (nrib == 0 && cct == -1) cct = pp_readlane(n.t, j);       // :162-166
                    }
                }
                if (nrib == 0) f |= PPGPU_C_DONE;
                if (lane == j) { myToCover = toCover; myRemaining = remaining; myFlags = f; myRibbons = nrib; }
            }
            lastX = pp_readlane(n.x, nsteps - 1); lastY = pp_readlane(n.y, nsteps - 1);
            lastBlocked = ((blkMask >> (nsteps - 1)) & 1ull) != 0ull;
            lastStraight = ((strMask >> (nsteps - 1)) & 1ull) != 0ull;
            if (base < nw) {
                // the record, as two 16-byte pieces: {to_cover, remaining} {flags | step, ribbons | reserved}
                lds_rec[0 * PP_TRACE_LDS_STRIDE + lane] = make_double2(myToCover, myRemaining);
                lds_rec[1 * PP_TRACE_LDS_STRIDE + lane] =
                    make_double2(__longlong_as_double((long long)(((unsigned long long)(unsigned)n.k << 32) | (unsigned long long)myFlags)),
                                 __longlong_as_double((long long)(unsigned long long)(unsigned)myRibbons));
                pp_trace_store<2>(lds_rec, out, base, nw);
            }
        }
    }
    // cover the last little bit (Edge.cpp:181-191): after a blocked step lastHeading is still the heading of the step before it
    const bool lastCover = cov || !lastBlocked || lastStraight;
    unsigned sf = 0u;
    if (lastCover) {
        bool changed;
        double D;
        if (!pp_cover_trace_event(rib, nrib, w, lastX, lastY, true, lds_ev, D, changed)) {
            if (lane == 0) counts[eg] = 0;
            pp_cover_trace_summary(sum, 0, 0, 0, PPGPU_CS_REFUSED, -1.0, 0.0);
            return;
        }
        sf = PPGPU_CS_LAST_COVER | (changed ? PPGPU_CS_LAST_CHANGED : 0u);
        if (changed) remaining = pp_ribbons_total_length(rib, nrib);
    }
    if (nrib == 0) {
        sf |= PPGPU_CS_DONE;
        // `intermediate.time()` where the loop stopped (:187-189): the blocked step's own time, else one increment past the last step
        if (cct == -1) cct = lastBlocked ? pp_const_f64(h.tg + count - 1)[0] : ((count < p.ng) ? pp_const_f64(h.tg + count)[0] : INFINITY);
    }
    if (lane == 0) counts[eg] = count;
    pp_cover_trace_summary(sum, events, changes, nrib, sf, cct, remaining);
    if (child && lane < nrib && lane < cstride) {
        double* c = child + ((size_t)eg * cstride + lane) * 4;
        c[0] = rib.sx; c[1] = rib.sy; c[2] = rib.ex; c[3] = rib.ey;
    }
}

// n_edges = slice size; recs[(edge - rec_base) * stride + k]; counts[edge], sums[edge], child[edge * cstride + i] (may be NULL)
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_cover(PPParams p, ppgpu_cover_record* recs, long long rec_base, int stride, int* counts,
                                                                     ppgpu_cover_summary* sums, double* child, int cstride) {
    __shared__ double2 s_rec[PP_TRACE_WPB][2 * PP_TRACE_LDS_STRIDE];
    __shared__ double s_ev[PP_TRACE_WPB][PP_WAVE * 4];
    int wave;
    long long el;
    if (pp_trace_entry(p, wave, el)) pp_cover_trace_edge(p, el, recs, rec_base, stride, counts, sums, child, cstride, s_rec[wave], s_ev[wave]);
}
