// pp_k_solve.h — phase 0 of an edge: pp_k_solve_edges (Vertex::connect + Edge::computeApproxCost, one lane per edge; one lane per
// curve where a dense launch asks for both speeds of a radius).  Included by pp_kernels.h.
#pragma once
#ifndef PP_CR_SOLVE
#define PP_CR_SOLVE true     // the edges' curves with correctly rounded atan2 / acos / sin / cos (pp_cr.h)
#endif
#ifndef PP_SOLVE_MIN_WAVES
#define PP_SOLVE_MIN_WAVES 1
#endif
// ALL_WORDS: the solver evaluates all six words correctly rounded and pp_curve_init every base heading (pp_k_solve_edges_all_words,
// PPGPU_SOLVE_ALL_WORDS=1, for the tests that compare the two); else only the words that can win, and no sin / cos of the curve's
// bases twice (pp_solve_rank.h, PPSincosMemo): the same records.  Two kernels, so that the test path does not set the registers of
// the production one.
template <bool ALL_WORDS>
__device__ __forceinline__ void pp_solve_edges_body(const PPParams& p) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    pp_launch_reset(p, e);
    if (e >= p.n_edges) return;
    // The two speeds of a radius (configurations c and c ^ PPGPU_EDGE_SLOW) run along the same curve: in the dense enumeration the
    // lane of the slow edge solves it once and writes both records, each where its own lane would have put it; the fast edge's lane
    // leaves.  (Work items are walked configuration-major, so the partner is a whole number of Q = (vertex, sample) pairs away and
    // whole waves leave together.)  A partner that the mask does not hold or that lies in another slice, explicit lists and given
    // curves: one lane per edge, as before.
    long long e2 = -1;                                         // the partner's position in this slice, when this lane writes it too
    if (!p.wedges && !p.edges) {
        const long long Q = p.total_edges / p.per;
        const int r = (int)((p.e_base + e) / Q);               // the edge's configuration is the r-th highest of the mask
        unsigned m = p.cfg_mask;
        for (int i = 0; i < p.per - 1 - r; i++) m &= m - 1;
        const unsigned c = (unsigned)(__ffs((int)m) - 1), c2 = c ^ PPGPU_EDGE_SLOW;
        if ((p.cfg_mask >> c2) & 1u) {
            const int r2 = (int)__popc(p.cfg_mask >> (c2 + 1));
            const long long ep = e + (long long)(r2 - r) * Q;
            if (ep >= 0 && ep < p.n_edges) {
                if (!(c & PPGPU_EDGE_SLOW)) return;
                e2 = ep;
            }
        }
    }
    unsigned vi, target, cbits;
    const long long eg = pp_edge_position(p, p.e_base + e);   // position in the caller's edge list; e = position in this slice
    pp_edge_decode(p, eg, vi, target, cbits);
    PPCurve cv;
    bool valid = false;
    unsigned sflags = 0;
    double srcT = 0, wSpeed = 1, wStart = 0, wEnd = 0;        // (w*: of a given curve)
    double srcHeading = 0;
    PPDubins dub;
    dub.p0 = dub.p1 = dub.p2 = 0; dub.type = -1;
    if (vi >= (unsigned)p.nverts || (!p.wedges && (long long)target >= p.n_samples)) {
        sflags = PP_SETUP_MALFORMED;
        pp_curve_init<false>(cv, 0, 0, 0, 1.0, dub);
    } else {
        const ppgpu_vertex* V = p.verts + vi;
        const double srcX = V->x, srcY = V->y, srcH = V->heading;
        srcT = V->time;
        srcHeading = srcH;
        valid = true;
        double rho = (cbits & PPGPU_EDGE_COVERAGE) ? p.rho_cov : p.rho;             // Edge.cpp:73-76
        if (p.wedges) {
            // the wrapper comes with the edge: DubinsWrapper::fill semantics, start time of ITS curve, possibly truncated end
            const ppgpu_wrapper_edge* W = p.wedges + eg;
            dub.p0 = W->param[0]; dub.p1 = W->param[1]; dub.p2 = W->param[2]; dub.type = W->type;
            if (dub.type < 0 || dub.type > 5) dub.type = -1;
            rho = W->rho; wSpeed = W->speed;
            pp_curve_init<PP_CR_SOLVE, PP_CR_SOLVE && !ALL_WORDS>(cv, W->qi[0], W->qi[1], W->qi[2], rho, dub);
            wStart = W->start_time; wEnd = W->end_time;
        } else {
            const double tgtX = p.sx[target], tgtY = p.sy[target], tgtH = p.sh[target];
            if ((srcX == tgtX) && (srcY == tgtY) && (srcH == tgtH)) sflags |= PP_SETUP_COLOCATED;   // State::isCoLocated
            if constexpr (ALL_WORDS || !PP_CR_SOLVE) {
                pp_dubins_shortest<PP_CR_SOLVE>(srcX, srcY, pp_yaw(srcH), tgtX, tgtY, pp_yaw(tgtH), rho, dub);
                pp_curve_init<PP_CR_SOLVE>(cv, srcX, srcY, pp_yaw(srcH), rho, dub);
            } else {
                pp_dubins_shortest_ranked(srcX, srcY, pp_yaw(srcH), tgtX, tgtY, pp_yaw(tgtH), rho, dub);
                pp_curve_init<PP_CR_SOLVE, true>(cv, srcX, srcY, pp_yaw(srcH), rho, dub);
            }
        }
        // the sweeps take sin/cos of (segment base heading +- arc) with the bounded-argument routine: refuse curves whose
        // angles leave its range (a heading of tens of thousands of radians, or NaN) instead of sampling them wrongly
        {
            const double bound = fabs(cv.qth) + cv.p0 + (cv.t1 == 1 ? 0.0 : cv.p1) + cv.p2;
            if (!(bound < 9.0e4)) dub.type = -1;
        }
    }
    // what depends on the speed, once per record: this lane's own edge, then its fast partner
    for (int k = 0; k < (e2 >= 0 ? 2 : 1); k++) {
        PPEdgeSetup* __restrict__ O = p.setup + p.ws_base + (k ? e2 : e);
        struct { double approx, wStart, wEnd, speed; int type; unsigned vi, cbits, sflags; } S;
        S.vi = vi; S.cbits = k ? (cbits ^ PPGPU_EDGE_SLOW) : cbits; S.sflags = sflags; S.type = -1;
        S.approx = S.wStart = S.wEnd = 0; S.speed = 1;
        if (valid) {
            if (p.wedges) {
                S.speed = wSpeed;
                S.wStart = wStart; S.wEnd = wEnd;
                S.approx = (S.wEnd - srcT) * 1.0;                         // Edge::setEnd(wrapper), Edge.cpp:208-216
            } else {
                S.speed = (S.cbits & PPGPU_EDGE_SLOW) ? p.slow_speed : p.max_speed;
                S.approx = cv.length / S.speed * 1.0;                   // Edge.cpp:17
                S.wStart = srcT;
                S.wEnd = srcT + cv.length / S.speed;                    // DubinsWrapper::setEndTime
            }
            S.type = dub.type;
        }
        pp_curve_segments(cv, O->seg);
        O->qx = cv.qx; O->qy = cv.qy; O->rho = cv.rho; O->rho_inv = cv.rho_inv; O->length = cv.length;
        O->p0 = cv.p0; O->p1 = cv.p1; O->p2 = cv.p2; O->hi1 = cv.p0 + cv.p1;
        O->approx = S.approx; O->wStart = S.wStart; O->wEnd = S.wEnd; O->speed = S.speed;
        O->type = S.type; O->vi = S.vi; O->cbits = S.cbits; O->sflags = S.sflags;
        O->srcH = srcHeading;                                           // the record's spare word: the sweep's first `lastHeading`
        // Which obstacles can come near this edge at all?  Every sampled pose lies within `travel` (arc length) of the curve's first
        // point and an obstacle moves at most |Speed| * duration during the sweep.  pp_k_plan_skips only looks at these, and
        // the pose sweep leaves the obstacles alone on an edge that has none.  Bit j = obstacle j, all ones when there are more than 64.
        unsigned long long omask = 0ull;
        if (p.n_obst > PP_WAVE) omask = ~0ull;
        else if (p.n_obst > 0 && S.type >= 0 && !(S.sflags & PP_SETUP_MALFORMED) && p.ng > 0) {
            const double t0 = p.tgrid[(size_t)vi * p.ng];
            const double endTime = fmin(p.horizon + 1e-12 + p.sst, S.wEnd);
            const double chunkTime = 64.0 * (p.inc_d / p.max_speed);
            const double duration = fmax(endTime - t0, 0.0) + chunkTime;
            const double travel = fmin(cv.length, fmax(endTime - S.wStart, 0.0) * S.speed) + 1e-3;
            for (int j = 0; j < p.n_obst; j++) {
                const PPObst& o = p.obst[j];
                const double dt = t0 - o.Time;
                const double X = o.X + o.Speed * dt * o.cosYaw, Y = o.Y + o.Speed * dt * o.sinYaw;
                const double R = o.reach + travel + fabs(o.Speed) * duration + 1e-3;
                const double dx = cv.qx - X, dy = cv.qy - Y;
                if (!(dx * dx + dy * dy > R * R)) omask |= 1ull << j;
            }
        }
        O->omask = omask;
    }
}
__global__ __launch_bounds__(256, PP_SOLVE_MIN_WAVES) void pp_k_solve_edges(PPParams p) { pp_solve_edges_body<false>(p); }
__global__ __launch_bounds__(256, PP_SOLVE_MIN_WAVES) void pp_k_solve_edges_all_words(PPParams p) { pp_solve_edges_body<true>(p); }
