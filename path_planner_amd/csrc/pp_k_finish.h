// pp_k_finish.h — phase C, the tail of Edge::computeTrueCost (Edge.cpp:177-205): where the step loop stopped, the pose it stopped on and
// the end pose, the last cover, the hit sums, cost / g / flags, the heuristic and the 16-double record.  Three routes reach it: the
// approach lane of a quiet edge (pp_finish_quiet_edge), the lane that takes over an edge from its wave (pp_k_cover_finish) and the wave
// that keeps its edge (the second half of pp_cover_sweep_edge, pp_k_cover.h).  The two lane routes are ONE function, pp_lane_phase_c;
// the wave has its own statements only where 64 lanes work on one edge (poses by pp_window_pose, the last cover by pp_ribbons_event,
// hit sums and record store across the lanes, the stop rule through scalar loads) and shares the done / goal flags and maxDistance
// (pp_device.h).
// Included by pp_kernels.h ahead of pp_k_cover.h.
#pragma once

// ---- pieces shared by the routes (and by the approach loop of pp_k_cover.h)

// Where the loop of Edge.cpp:143-175 stopped: by the `break` at :146 (the blocked step `limit` is reached only if every step before it
// ran — nexec == limit — AND its own time still passes `while (t < endTime)`: endTime may have shrunk at an event before it, :169) or
// by its condition failing (or the first sample threw: stopKind 2, `intermediate` still holds the source pose).  nexec = steps that ran.
struct PPLoopStop {                 // (as initialised: no step ran)
    bool infeasible = false;        // the stop itself makes the edge infeasible
    bool coverFinal = true;         // `lastHeading == intermediate.heading()` where the loop stopped (true unless it broke at a blocked step)
    int lastIdx = -1;               // the step whose pose `intermediate` holds (-1: the source pose)
    int steps = 0, hexec = 0;       // steps for the record, steps whose obstacle hits count
    double tfinal = INFINITY;       // intermediate.time(): only matters when the ribbons run out at the last cover
};
// Lane form, for both lane routes.  The wave states the same rule once more in wave form (pp_cover_sweep_edge, pp_k_cover.h), through
// wave-uniform scalar loads: shared through this function its sweep kernels spill more registers (profiles/cover_finish_ab.txt).
__device__ __forceinline__ PPLoopStop pp_loop_stop(int limit, int stopKind, int nexec, double endTime, const double* tg, int ng, bool cov,
                                                   const unsigned long long* teq) {
    PPLoopStop s;
    // the loop's condition failed after nexec steps (or the first sample threw: `intermediate` still holds the source pose) ...
    if (stopKind == 2 && ng > 0 && tg[0] < endTime) s.infeasible = true;
    s.lastIdx = nexec - 1;
    s.tfinal = (nexec < ng) ? tg[nexec] : INFINITY;
    s.steps = nexec;
    s.hexec = nexec;
    // ... unless it got as far as the blocked step and broke there (:146): `intermediate` is that step's pose, which counts as a step of
    // the record but not for the hits (tfinal and hexec stand: nexec == limit)
    if (stopKind == 1 && nexec == limit && tg[limit] < endTime) {
        s.infeasible = true;
        s.lastIdx = limit;
        s.coverFinal = cov || (((teq[limit >> 6] >> (limit & 63)) & 1ull) != 0ull);
        s.steps = limit + 1;
    }
    return s;
}

// Obstacle hits of the executed steps (Edge.cpp:150-151 summed), lane form: whole chunks from the pose sweep's per-chunk sums, then the
// last partial chunk — a chunk the sweep skipped has no per-step counts (the same boxes at every step), any other step by step.
__device__ __forceinline__ int pp_lane_hit_sum(const PPParams& p, long long e, int hexec) {
    int hitsTotal = 0;
    if (p.n_obst > 0) {
        const unsigned* tch = p.track_chunk_hits + (size_t)e * p.nch;
        const int cfull = hexec >> 6;
        for (int c = 0; c < cfull; c++) hitsTotal += (int)tch[c];
        if ((hexec & 63) != 0 && tch[cfull] != 0u) {
            if (p.track_skip && (p.track_skip[(size_t)e * p.nch + cfull] & PP_SKIP_ALL) != 0) {
                hitsTotal += (hexec & 63) * (int)(tch[cfull] >> 6);
            } else {
                const unsigned short* thits = p.track_hits + (size_t)e * p.ngp;
                for (int i = cfull << 6; i < hexec; i++) hitsTotal += (int)thits[i];
            }
        }
    }
    return hitsTotal;
}

// PPGPU_F_DONE (no ribbon left) and PPGPU_F_GOAL: SamplingBasedPlanner::goalCondition (SamplingBasedPlanner.cpp:42-50)
__device__ __forceinline__ unsigned pp_done_goal_flags(const PPParams& p, int nrib, double endTime, double cct) {
    unsigned f = (nrib == 0) ? PPGPU_F_DONE : 0u;
    const double coverageDoneTime = cct + p.tmin;
    const double nonCoverageDoneTime = p.sst + p.horizon;
    if (endTime >= nonCoverageDoneTime || (nrib == 0 && endTime >= coverageDoneTime)) f |= PPGPU_F_GOAL;
    return f;
}

// The 16 doubles of an edge's record, lane form, into r: the record itself or a stage in LDS.  {flags (low), info (high)} lead; the
// approximate cost and the curve's three segment lengths come from the setup record.
struct PPRecordFields {
    int nrib, steps;
    unsigned flags;
    double trueCost, penalty, endX, endY, endHeading, speed, endTime, g, h, cct;
};
__device__ __forceinline__ void pp_lane_store_record(double* r, const PPEdgeSetupBody* S, const PPRecordFields& f) {
    const unsigned info = (unsigned)(S->type & 0xff) | ((unsigned)(f.nrib & 0xff) << 8) | ((unsigned)(f.steps & 0xffff) << 16);
    r[0] = __hiloint2double((int)info, (int)f.flags);
    r[1] = f.trueCost; r[2] = f.penalty; r[3] = S->approx;
    r[4] = f.endX; r[5] = f.endY; r[6] = f.endHeading; r[7] = f.speed; r[8] = f.endTime;
    r[9] = f.g; r[10] = f.h; r[11] = (f.h == PP_H_DEFERRED) ? f.g : f.g + f.h;
    r[12] = f.cct; r[13] = S->p0; r[14] = S->p1; r[15] = S->p2;
}

// DubinsWrapper::sample (DubinsWrapper.cpp:29-49), lane form: the curve constants a lane samples with, loaded once from its setup
// record, and one pose from them (x, y, un-normalised yaw; err: the arc length fell outside the curve even after the retry).
struct PPLaneCurve : PPCurveHot { double p0, p1, hi1; int word; };
__device__ __forceinline__ PPLaneCurve pp_lane_curve(const PPEdgeSetupBody* S) {
    PPLaneCurve c;
    c.wStart = S->wStart; c.speed = S->speed; c.length = S->length; c.rho = S->rho; c.rho_inv = S->rho_inv; c.qx = S->qx; c.qy = S->qy;
    c.p0 = S->p0; c.p1 = S->p1; c.hi1 = S->hi1; c.word = S->type;
    return c;
}
__device__ __forceinline__ void pp_lane_pose(const PPEdgeSetupBody* S, const PPLaneCurve& c, double t, double& x, double& y, double& uth, bool& err) {
    double dist = (t - c.wStart) * c.speed;                                 // DubinsWrapper.cpp:36
    if (dist < 0 || dist > c.length) dist = dist - 1e-5;                    // EDUBPARAM retry, :39-42
    if (dist < 0 || dist > c.length) { err = true; dist = fmin(fmax(dist, 0.0), c.length); }
    const double tprime = (c.rho_inv != 0.0) ? dist * c.rho_inv : dist / c.rho;
    double ux, uy;
    pp_setup_seg_pose(S, pp_seg_of(tprime, c.p0, c.hi1), tprime, c.p0, c.p1, c.word, ux, uy, uth);
    x = ux * c.rho + c.qx;
    y = uy * c.rho + c.qy;
}

// One ribbon's part of a coverage event at (x, y), lane form: does the ribbon contain the point (RibbonManager::minDistanceFrom then
// returns 0), does it contain it strictly (cover() would split it), and the projection it would be split at.
__device__ __forceinline__ void pp_lane_ribbon_contains(double sx, double sy, double ex, double ey, double x, double y, double w, bool& inside, bool& strict,
                                                        double& px, double& py) {
    const double T = PP_RIBBON_TOL;
    const double dxr = ex - sx, dyr = ey - sy;
    const double sqL = dxr * dxr + dyr * dyr;
    const double dot = (x - sx) * dxr + (y - sy) * dyr;
    px = dxr * dot / sqL + sx;                               // Ribbon::getProjection (Ribbon.cpp:72-78)
    py = dyr * dot / sqL + sy;
    const double a1 = px - sx, a2 = px - ex, b1 = py - sy, b2 = py - ey;
    const bool outx = ((a1 < -T) & (a2 < -T)) | ((a1 > T) & (a2 > T));
    const bool outy = ((b1 < -T) & (b2 < -T)) | ((b1 > T) & (b2 > T));
    const bool cp = !(outx | outy);                          // Ribbon::containsProjection (:90-95)
    const double num = dyr * x - dxr * y + ex * sy - ey * sx;
    const double ld = fabs(num) / sqrt(sqL);                 // Ribbon::distance (Ribbon.h:118-121)
    inside = cp && (ld < w);
    strict = cp && (ld < (w / 2.0));
}

// The ribbon list a lane walks: its own (rp, n: vector loads) and, when every lane of the wave starts from the same vertex (a dense
// launch from one open vertex), the wave's (rpU, nU in scalar registers: scalar loads instead of four vector loads per ribbon).
// pp_with_ribbons hands f the pointer in its address space and the count, so each walk is written once.
struct PPLaneRibbons { const double* rp; int n; const double* rpU; int nU; bool uniform; };
template <class F>
__device__ __forceinline__ auto pp_with_ribbons(const PPLaneRibbons& L, F f) { return L.uniform ? f(pp_const_f64(L.rpU), L.nU) : f(L.rp, L.n); }
// is (x, y) inside the ribbon's bounding box grown by `grow` (pp_ribbons_event's fast path: outside it the ribbon is out of reach)?
__device__ __forceinline__ bool pp_in_grown_box(double sx, double sy, double ex, double ey, double x, double y, double grow) {
    return (x >= fmin(sx, ex) - grow) & (x <= fmax(sx, ex) + grow) & (y >= fmin(sy, ey) - grow) & (y <= fmax(sy, ey) + grow);
}
template <class RP>
__device__ __forceinline__ bool pp_in_any_grown_box(RP r, int n, double x, double y, double grow) {
    bool inBox = false;
    for (int i = 0; i < n; i++) inBox |= pp_in_grown_box(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3], x, y, grow);
    return inBox;
}
template <class RP>
__device__ __forceinline__ void pp_copy_ribbons(double* c, RP r, int n) {
    for (int i = 0; i < 4 * n; i++) c[i] = r[i];
}

// RibbonManager::cover(x, y, strict) over the nrib <= PP_FINISH_MAX ribbons of the child slot c, in list order and in place (Ribbon::split
// / covered, Ribbon.cpp:9-25,39-58; the wave's pp_ribbons_event decides the distance test on squares and falls back to the quotient of
// pp_lane_ribbon_contains when it is close) -> the ribbons left.  Slots the list filled beyond that go back to zero: a wave that
// finishes its own edge never writes them, and callers hand in zeroed buffers.
__device__ __forceinline__ int pp_lane_cover_strict(double* c, int nrib, int stride, double x, double y, double w) {
    double rsx[PP_FINISH_MAX], rsy[PP_FINISH_MAX], rex[PP_FINISH_MAX], rey[PP_FINISH_MAX];
#pragma unroll
    for (int i = 0; i < PP_FINISH_MAX; i++) {
        const bool have = i < nrib;
        rsx[i] = have ? c[4 * i] : 0.0; rsy[i] = have ? c[4 * i + 1] : 0.0; rex[i] = have ? c[4 * i + 2] : 0.0; rey[i] = have ? c[4 * i + 3] : 0.0;
    }
    const double minLength = 2 * w;                                  // Ribbon::minLength (Ribbon.cpp:52-58)
    const double thr = minLength * minLength / (2.0 * 2.0);          // covered(strict): c_StrictModifier^2
    int nout = 0;
#pragma unroll
    for (int i = 0; i < PP_FINISH_MAX; i++) {
        if (i < nrib) {
            const double sx = rsx[i], sy = rsy[i], ex = rex[i], ey = rey[i];
            bool inside, stc;
            double px, py;
            pp_lane_ribbon_contains(sx, sy, ex, ey, x, y, w, inside, stc, px, py);
            const bool keepF = stc && !(pp_sq_len(sx, sy, px, py) < thr);
            const bool keepR = stc ? !(pp_sq_len(px, py, ex, ey) < thr) : !(pp_sq_len(sx, sy, ex, ey) < thr);
            if (keepF) {
                if (nout < stride) { c[4 * nout] = sx; c[4 * nout + 1] = sy; c[4 * nout + 2] = px; c[4 * nout + 3] = py; }
                nout++;
            }
            if (keepR) {
                if (nout < stride) { c[4 * nout] = stc ? px : sx; c[4 * nout + 1] = stc ? py : sy; c[4 * nout + 2] = ex; c[4 * nout + 3] = ey; }
                nout++;
            }
        }
    }
    for (int i = nout; i < nrib; i++) { c[4 * i] = 0.0; c[4 * i + 1] = 0.0; c[4 * i + 2] = 0.0; c[4 * i + 3] = 0.0; }
    return nout;
}

// ---- phase C, lane form: one function for both lane routes
// st = the edge's state when its event loop (Edge.cpp:153-171) is over, cnt = steps k < limit with t_k < st.endTime (each caller's own
// search), rin = the ribbons as the loop left them (st.nrib of them), r = where the record goes.
// QUIET = false, an edge its wave handed over: rin is the edge's child slot, the last cover happens in it.
// QUIET = true, an edge whose events changed nothing: rin is the vertex's list, which becomes the child's — unless the last cover would
// happen within reach of a ribbon or a pose is off the curve: then nothing is written and false says "the wave does this edge".
// Heuristic, by pp_h_route: a list pp_k_heuristic_lanes enumerates is marked PP_H_DEFERRED; MaxDistance is computed here; a wave-form
// enumeration (7 or 8 ribbons) goes on pp_k_heuristic_listed's list.
template <bool QUIET>
__device__ __forceinline__ bool pp_lane_phase_c(const PPParams& p, const PPEdgeSetupBody* S, const PPLaneCurve& cv, const ppgpu_vertex* V, long long e, long long eg,
                                                const PPCoverState& st, int limit, int cnt, const double* tg, const PPLaneRibbons& rin, double* r) {
    const bool cov = (S->cbits & PPGPU_EDGE_COVERAGE) != 0;
    const double endTime = st.endTime;
    double cct = st.cct;
    int nrib = st.nrib, rdt = st.rdt;
    unsigned flags = st.flags;
    // The quiet route never covers, so its nrib stays the vertex's: > 0 and within PP_TSP_MAX and the child slot, by pp_finish_quiet_edge's
    // refusals.  That leaves the quiet instantiation without need_big, RIBBON_OVF and the listed heuristics.
    if (QUIET) __builtin_assume(nrib > 0 && nrib <= PP_TSP_MAX && nrib <= p.stride);
    int nexec = cnt > st.lastEv + 1 ? cnt : st.lastEv + 1;
    nexec = nexec < limit ? nexec : limit;
    const PPLoopStop stop = pp_loop_stop(limit, p.track_summary[e].blocked, nexec, endTime, tg, p.ng, cov, p.track_eq + (size_t)e * p.nch);
    if (stop.infeasible) flags |= PPGPU_F_INFEASIBLE;
    // ---- end state (:177-178) and the pose `intermediate` stopped on
    double ix = V->x, iy = V->y, uth;
    bool ignored = false, perr = false;
    if (stop.lastIdx >= 0) pp_lane_pose(S, cv, tg[stop.lastIdx], ix, iy, uth, ignored);
    double endX, endY;
    pp_lane_pose(S, cv, endTime, endX, endY, uth, perr);
    if (perr) {
        if (QUIET) return false;
        flags |= PPGPU_F_DUBINS_ERR;
    }
    const double endHeading = pp_heading_from_yaw(pp_mod2pi(uth));
    // ---- cover the last little bit (:182-191)
    double* c = p.child + (size_t)eg * p.stride * 4;
    if ((cov || stop.coverFinal) && nrib > 0) {
        if (QUIET) {
            if (pp_with_ribbons(rin, [&](auto rr, int n) { return pp_in_any_grown_box(rr, n, ix, iy, p.ribw + 1e-3); })) return false;
        } else {
            nrib = pp_lane_cover_strict(c, nrib, p.stride, ix, iy, p.ribw);
        }
    }
    if (nrib == 0) {
        if (cct == -1) cct = stop.tfinal;
        rdt = (int)stop.tfinal;
    }
    const double penalty = (double)pp_lane_hit_sum(p, e, stop.hexec) * p.cpf;
    const double netTime = endTime - V->time;                                     // Edge::netTime
    double tc = fmax(netTime - ((nrib == 0) ? (endTime - (double)rdt) : 0), 0);  // :197
    if (V->ribbon_count == 0) tc = 0;                                             // :198 (Edge.cpp:93)
    const double trueCost = tc * p.tpf + penalty;                                 // :199
    const double g = V->g + trueCost;                                             // Vertex::setCurrentCost
    flags |= pp_done_goal_flags(p, nrib, endTime, cct);
    if (nrib > PP_TSP_MAX) atomicOr(&p.words->need_big, 1u);
    if (nrib > p.stride) flags |= PPGPU_F_RIBBON_OVF;
    // ---- h: Vertex::computeApproxToGo, as pp_h_route says.  A lane marks, computes MaxDistance in place, and lists what needs a wave.
    double h = 0;
    const PPHRoute route = pp_h_route(p.heuristic, p.tsp_k, nrib, p.stride, p.fuse_h, p.defer_h);
    if (route == PP_HR_LANES) h = PP_H_DEFERRED;
    if (route == PP_HR_OVERFLOW) flags |= PPGPU_F_RIBBON_OVF;               // (PP_HR_BIG: pp_k_heuristic_big fills it in)
    if (route == PP_HR_MAX_DISTANCE)
        h = pp_h_cost(pp_max_distance(nrib, p.ribw, endX, endY, pp_ribbons_at(rin.rp)), p.max_speed, p.tpf);
    const bool listed = route == PP_HR_WAVE;                                // pp_k_heuristic_listed: a workgroup per such edge
    PPRecordFields f;
    f.nrib = nrib; f.steps = stop.steps; f.flags = flags; f.trueCost = trueCost; f.penalty = penalty;
    f.endX = endX; f.endY = endY; f.endHeading = endHeading; f.speed = cv.speed; f.endTime = endTime; f.g = g; f.h = h; f.cct = cct;
    pp_lane_store_record(r, S, f);
    if (QUIET) pp_with_ribbons(rin, [&](auto rr, int n) { pp_copy_ribbons(c, rr, n); return 0; });
    if (listed) p.hw_list[atomicAdd(&p.words->hw_count, 1u)] = (unsigned)eg;
    return true;
}

// A quiet edge, by its approach lane (pp_k_approach_events): the event loop ran to `limit` and changed nothing, so the state is the
// vertex's and endTime is Edge.cpp:90's.  What this route will not take stays with the edge's wave (-> false, nothing written): a
// track with a sampling error, a list beyond the child slot or the lane heuristics, the Gaussian model, a heuristic that needs a
// wave, a curve that does not contain endTime (DubinsWrapper::containsTime: the reference throws) — and pp_lane_phase_c's two.
__device__ __forceinline__ bool pp_finish_quiet_edge(const PPParams& p, const PPEdgeSetupBody* S, const PPLaneCurve& cv, const ppgpu_vertex* V, long long e, long long eg,
                                                     int limit, int lastEv, const PPLaneRibbons& rin, const double* tg, double* stage) {
    const int nrib = rin.n;                                                  // > 0, no piece short enough to be erased
    if (p.track_summary[e].dub_err) return false;
    // pp_lane_phase_c<true> ASSUMES (__builtin_assume) 0 < nrib <= PP_TSP_MAX and nrib <= p.stride: whoever relaxes this refusal, or lets
    // an empty list reach this function, must relax that assumption with it — otherwise the behaviour is undefined.
    if (nrib > p.stride || nrib > PP_TSP_MAX) return false;
    if (p.n_obst > 0 && p.obst_model == PPGPU_OBST_GAUSSIAN) return false;
    if (pp_h_route(p.heuristic, p.tsp_k, nrib, p.stride, p.fuse_h, p.defer_h) == PP_HR_WAVE) return false;
    const double wEnd = S->wEnd;
    PPCoverState st;
    st.endTime = fmin(p.horizon + 1e-12 + p.sst, wEnd);                      // Edge.cpp:90; no event shortened it
    if (!(cv.wStart <= st.endTime && wEnd >= st.endTime)) return false;
    st.cct = V->coverage_completed_time; st.nrib = nrib; st.lastEv = lastEv; st.rdt = -1;
    st.flags = (V->time >= st.endTime) ? PPGPU_F_INFEASIBLE : 0u;            // :102-110
    return pp_lane_phase_c<true>(p, S, cv, V, e, eg, st, limit, limit, tg, rin, stage);
}

// An edge its wave handed over (PPCoverState; the wave keeps a list longer than PP_FINISH_MAX, the Gaussian model, a curve the
// reference throws on), one LANE per edge: the state and the ribbons are what the wave left, the record goes straight out.
#ifndef PP_FINISH_THREADS
#define PP_FINISH_THREADS 64
#endif
__global__ __launch_bounds__(PP_FINISH_THREADS) void pp_k_cover_finish(PPParams p) {
    const unsigned nlive = (unsigned)pp_const_i32(&p.words->live_count)[0];
    const unsigned li = blockIdx.x * PP_FINISH_THREADS + threadIdx.x;
    if (li >= nlive) return;
    const long long e = p.ws_base + (long long)p.live_list[2 * (size_t)li];
    const long long eg = (long long)p.live_list[2 * (size_t)li + 1];
    const PPCoverState st = p.cover_state[e];
    if (st.nrib < 0) return;                                   // its wave finished it
    const PPEdgeSetupBody* S = p.setup + e;
    const unsigned vi = S->vi;
    const double* tg = p.tgrid + (size_t)vi * p.ng;
    const int limit = p.track_summary[e].limit;
    int cnt = limit;                                           // the time grid is non-decreasing
    if (st.endTime != fmin(p.horizon + 1e-12 + p.sst, S->wEnd)) {         // an event shortened Edge.cpp:90's end time
        int lo = 0, hi = limit;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tg[mid] < st.endTime) lo = mid + 1; else hi = mid;
        }
        cnt = lo;
    }
    const PPLaneRibbons rin = {p.child + (size_t)eg * p.stride * 4, st.nrib, nullptr, 0, false};
    pp_lane_phase_c<false>(p, S, pp_lane_curve(S), p.verts + vi, e, eg, st, limit, cnt, tg, rin, reinterpret_cast<double*>(p.out + eg));
}
