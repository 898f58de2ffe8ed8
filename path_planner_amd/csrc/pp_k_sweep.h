// pp_k_sweep.h — the collision sweep of Edge::computeTrueCost (Edge.cpp:143-152,172-174): pp_window_pose, the chunk-skip planner
// (pp_k_plan_skips) and pp_k_pose_sweep.  Included by pp_kernels.h.
#pragma once
// ------------------------------------------------------------------------------------------
// Edge costing = four launches over the same edge list (the fourth, pp_k_heuristic, further down), one wavefront-sized piece
// of work each:
//
//   pp_k_solve_edges  (lane per edge,  phase 0: Vertex::connect + Edge::computeApproxCost: Dubins solve, curve constants,
//                      per curve when a dense launch holds both speeds of a radius)
//   pp_k_pose_sweep   (wave per edge)  phase A: 64 consecutive collision-check steps at a time: closed-form pose,
//                                      occupancy lookup, dynamic-obstacle box tests  ->  the edge's "track"
//   pp_k_cover_sweep  (wave per edge)  phase B: the sequential coverage state machine of Edge.cpp:153-171, visited only
//                                      at its event steps (ribbon per lane); phase C: end state, last cover, cost, g,
//                                      one 128-byte record per edge
//
// Fused in one kernel the state machine's registers and the pose pipeline's registers are live together and the loop
// spills; apart, the pose sweep is a spill-free streaming kernel.  What it leaves for the cover sweep (the "track") is small:
// per 64-step chunk a word of heading-unchanged bits and a hit count, per edge where the sweep stopped and why.  The poses
// themselves are not stored: the cover sweep recomputes them (pp_window_pose, the same code) for the few windows it visits.
#ifndef PP_WPB
#define PP_WPB 4   // wavefronts (= edges) per workgroup of the per-edge kernels
#endif
#ifndef PP_MIN_WAVES
#define PP_MIN_WAVES 4   // cover sweep: waves per SIMD the register allocator must leave room for (4 = 128 VGPRs: no spills;
                         // 6 measures 5 % faster but turns 43 spilled registers into 5 GB of scratch traffic per launch)
#endif
#define PP_SF64(field) (pp_const_f64(&S->field)[0])
#define PP_SI32(field) (pp_const_i32(&S->field)[0])

// per-edge result of the pose sweep
struct PPTrackSummary {
    int limit;      // steps [0, limit) can execute: the first blocked step, or the first step at/after the edge's end time
    int blocked;    // 1: step `limit` exists and is blocked (Edge.cpp:144-147); 2: sampling step 0 threw (limit = 0, :126-133)
    int dub_err;    // some sampled arc length fell outside the curve even after the reference's 1e-5 retry
    int pad;        // (round 3 measured a per-edge hit total here: pose sweep +33 us for -10 elsewhere, not taken)
};
static_assert(sizeof(PPTrackSummary) == sizeof(int4), "pp_k_mark_sweeps zeroes the summary of an edge off the sweep list with one 16-byte store");

// What the cover sweep's wave knows when its event loop (Edge.cpp:153-171) is over, for pp_k_cover_finish (one LANE per edge) to go
// on from: the rest of computeTrueCost (Edge.cpp:177-205) is scalar work per edge — where the loop stopped, two poses, the last
// cover, the hit sums, the cost, the record — that a whole wave used to do for one edge at a time (287 of the sweep's 1 047 us at
// config 3).  The ribbons as the loop left them travel in the edge's child-ribbon slot.  nrib < 0: the wave finished the edge itself.
#define PP_FINISH_MAX 8              // ribbons a lane takes over at most (it keeps them in registers; longer lists stay with the wave)
struct PPCoverState {
    double cct, endTime;             // RibbonManager::coverageCompletedTime, the edge's (possibly shortened) end time
    int nrib, lastEv, rdt;           // ribbons left, last event visited, `ribbonsDoneTime` (an int: Edge.cpp:92)
    unsigned flags;                  // PPGPU_F_* collected so far
};
// DubinsWrapper::sample (DubinsWrapper.cpp:29-49) -> dubins_path_sample for the 64 steps of one window, one step per lane:
// x, y and the un-normalised yaw.  Used by BOTH sweeps with the same arithmetic, so the cover sweep sees exactly the poses the
// pose sweep tested (it recomputes them for the few windows that hold coverage events instead of reading them back from HBM).
// The constants of the segment the caller is on (cur / cs) live in scalar registers and are swapped when the window moved on.
struct PPCurveHot { double wStart, speed, length, rho, rho_inv, qx, qy; };
__device__ __forceinline__ PPCurveHot pp_curve_hot(const PPEdgeSetup* S) {
    PPCurveHot h;
    h.wStart = PP_SF64(wStart); h.speed = PP_SF64(speed); h.length = PP_SF64(length); h.rho = PP_SF64(rho); h.rho_inv = PP_SF64(rho_inv);
    h.qx = PP_SF64(qx); h.qy = PP_SF64(qy);
    return h;
}
template <bool TAB = false>
__device__ __forceinline__ void pp_window_pose(const PPEdgeSetup* S, const PPCurveHot& c, int& cur, PPSeg& cs, double t, double tFirst, bool valid,
                                               double& x, double& y, double& uth, bool& dubErr) {
    // lanes past the end of the sweep redo lane 0's step (benign arithmetic, uniform control flow); the caller masks them
    const double tl = valid ? t : tFirst;
    double dist = (tl - c.wStart) * c.speed;                          // DubinsWrapper.cpp:36
    if (__ballot((dist < 0) | (dist > c.length)) != 0ull) {           // rare: the first / last step of a curve
        if (dist < 0 || dist > c.length) dist = dist - 1e-5;          // EDUBPARAM retry, :39-42
        if (dist < 0 || dist > c.length) { dubErr = true; dist = fmin(fmax(dist, 0.0), c.length); }
    }
    // dubins_path_sample(): 64 consecutive arc lengths almost always fall on one segment, which is then advanced with
    // wave-uniform constants
    const double tprime = (c.rho_inv != 0.0) ? dist * c.rho_inv : dist / c.rho;
    double ux, uy;
    bool uniformSeg = __ballot(!((tprime >= cs.lo) & (tprime < cs.hi))) == 0ull;
    if (!uniformSeg) {
        const double hi0 = PP_SF64(p0), hi1 = PP_SF64(hi1);
        const int mine = pp_seg_of(tprime, hi0, hi1);
        const int firstSeg = __builtin_amdgcn_readfirstlane(mine);
        const int lastSeg = __builtin_amdgcn_readlane(mine, 63 - __clzll((long long)__ballot(valid)));
        if (__ballot(mine != firstSeg) != 0ull) {
            // the window straddles a junction: every lane takes its own segment's constants from memory
            pp_setup_seg_pose<TAB>(S, mine, tprime, ux, uy, uth);
        } else {
            uniformSeg = true;
            if (cur != firstSeg) { cur = firstSeg; cs = pp_seg_load_uniform(&S->seg[cur], cur, hi0, PP_SF64(p1), hi1, PP_SI32(type)); }
        }
        if (cur != lastSeg && !uniformSeg) { cur = lastSeg; cs = pp_seg_load_uniform(&S->seg[cur], cur, hi0, PP_SF64(p1), hi1, PP_SI32(type)); }
    }
    if (uniformSeg) pp_curve_seg<TAB>(cs.type, (tprime - cs.o1) - cs.o2, cs.bx, cs.by, cs.bth, cs.sb, cs.cb, ux, uy, uth);
    x = ux * c.rho + c.qx;
    y = uy * c.rho + c.qy;
}

// The cover sweep samples poses only when it loads a window: it re-reads the curve constants there (scalar loads, kept
// inside the loop by laundering the pointer) rather than carrying 33 scalar registers of them through the event loop.
#ifndef PP_COVER_SINCOS_TAB
#define PP_COVER_SINCOS_TAB true    // the cover sweep takes the sine / cosine constants from memory (see pp_sincos_bounded)
#endif
#define PP_WINDOW_POSE(S, t, t0, valid, x, y) do {                                                         \
        const PPEdgeSetup* _S = (S);                                                                       \
        asm volatile("" : "+s"(_S));                                                                       \
        const PPCurveHot _hot = pp_curve_hot(_S);                                                          \
        int _cur = -1;                                                                                     \
        PPSeg _cs = PPSeg{0, 0, 0, 0, 0, INFINITY, -INFINITY, 0, 0, 1};   /* matches nothing: the first use loads a segment */ \
        double _u; bool _e = false;                                                                        \
        pp_window_pose<PP_COVER_SINCOS_TAB>(_S, _hot, _cur, _cs, t, t0, valid, x, y, _u, _e);              \
    } while (0)
// Which 64-step chunks of an edge's sweep can be skipped?  One THREAD per (edge, chunk), in a kernel of its own ahead of the pose
// sweep (inside the sweep the test's registers pushed the per-step loop into spills).  The decision is pp_plan_chunk below, the one
// body of all six planner kernels; its two callers differ in where the ends of the chunk's chord come from and which obstacles it
// is shown (pp_plan_skips_chunk: sampled by the thread, the edge's omask or the whole table; pp_plan_skips_spans: shared between
// neighbouring threads, the obstacles that can come near the chunk's span).  A chunk is skipped when it provably changes nothing the
// sweep records:
//   * all 64 steps exist and lie before the edge's end time, on the curve proper (no retry at the ends);
//   * no pose of the chunk can lie on a blocked cell or off the grid, and every obstacle either holds every pose of the chunk or
//     none (Gaussian model: none comes within its 1e-13 radius): the bounds are stated at pp_plan_chunk;
//   * on edges that may not cover while turning (Edge.cpp:159) the heading-unchanged bits are known without sampling: the step
//     before the chunk and its last step lie on the same segment of the curve — a straight (the heading is the same expression
//     at every step: all bits set) or an arc whose steps are more than 1e-9 rad apart (no two headings equal: all bits clear).
// A skipped chunk's outputs are stored here (its hits; the heading bits); for a chunk that is NOT skipped on such an edge the
// heading of the step before it is stored (`lastHeading`, Edge.cpp:96,174: the sweep needs it when the chunk before was skipped).
// Everything is the arithmetic the sweep itself would do (pp_window_pose's expressions, one lane's worth).
// Can obstacle o hold a pose that lies within `rad` of (x, y), the midpoint of a chunk's chord, at a time within ht of tM?  The
// box test of pp_obstacle_hit with both half-extents grown by the distance pose and obstacle can drift apart (Gaussian model: the
// 1e-13 radius grown likewise).  true = certainly not.
template <bool GAUSSIAN>
__device__ __forceinline__ bool pp_chunk_clear_of(const PPObst& o, double x, double y, double tM, double rad, double ht) {
    const double dt = tM - o.Time;
    const double X = o.X + o.Speed * dt * o.cosYaw, Y = o.Y + o.Speed * dt * o.sinYaw;
    const double slack = rad + fabs(o.Speed) * ht + 1e-3;
    const double dx = x - X, dy = y - Y;
    if (GAUSSIAN) {
        const double R = o.reach + slack;
        return dx * dx + dy * dy > R * R;
    }
    const double rx = dx * o.cosYaw - dy * o.sinYaw, ry = dx * o.sinYaw + dy * o.cosYaw;
    return (fabs(rx) > o.halfL + slack) | (fabs(ry) > o.halfW + slack);
}
#define PP_SKIP_ALL 1     // track_skip bits: the chunk is not sampled at all
#define PP_SKIP_GRID 2    // sampled, but no pose of it can lie on a blocked cell
#define PP_SKIP_OBST 4    // sampled, but no pose of it can lie inside an obstacle
#define PP_SKIP_HITS 8    // with PP_SKIP_ALL: every pose of the chunk lies inside some obstacle box (the chunk's hit count is not zero)
#define PP_PLAN_EDGES_MAX 32          // edges a workgroup of the skip planner stages at most (14 KB of LDS)
// The pose at arc length d of the edge's curve (0 <= d <= length), as the sweep computes it, in two steps: on the unit curve, then
// scaled and placed.
__device__ __forceinline__ void pp_plan_unit_pose(const PPEdgeSetupBody* S, double d, double& ux, double& uy) {
    const double rho = S->rho, rho_inv = S->rho_inv;
    const double tp = (rho_inv != 0.0) ? d * rho_inv : d / rho;
    double uth;
    pp_setup_seg_pose(S, pp_seg_of(tp, S->p0, S->hi1), tp, ux, uy, uth);
}
__device__ __forceinline__ void pp_plan_place(const PPEdgeSetupBody* S, double ux, double uy, double& x, double& y) {
    x = ux * S->rho + S->qx; y = uy * S->rho + S->qy;
}
__device__ __forceinline__ void pp_plan_pose(const PPEdgeSetupBody* S, double d, double& x, double& y) {
    double ux, uy;
    pp_plan_unit_pose(S, d, ux, uy);
    pp_plan_place(S, ux, uy, x, y);
}
// The decision for one (edge, chunk), and its stores.  S: the edge's setup record (in LDS); tg: its time row; tF: the time of the
// chunk's first step (INFINITY: there is none).  ends(dF, dL, xF, yF, xE, yE, tE, dE) gives the chord, from
// the pose F at the first step to the pose E at step 64c + 63 or 64c + 64, with E's time and arc length.  tE and dE arrive as the
// last step's; dF and dL are the arc lengths of the first and the last step.  It is only called for a chunk of 64 steps that all
// lie before the end time on the curve proper.  (Six references and not a struct of them: handed to the lambda, the struct costs
// pp_k_plan_skips six more spilled registers, profiles/plan_skips_shared.txt.)
// each(against, decided) shows against() the obstacles that can matter, while `decided` holds.
//
// The bounds.  The vehicle moves at constant speed on a curve of curvature <= 1/rho and an obstacle at constant velocity, both
// linear in the step time: relative to an obstacle's box the pose at time t is within dev = L^2 / (8 rho) of the point of the
// chord at the same time fraction (a function that vanishes at both ends with second derivative bounded by 1/rho), L = dE - dF
// the arc length the chord spans.  The steps of the chunk are among those the chord spans, the time row rises with the step.
// At config 3 dev is 0.08 .. 0.16 m where a ball around the middle pose needed 3.5 m.
//   grid    two balls around the quarter points of the chord: every chord point is within L/4 of one of them, every pose within dev
//           of the chord, so within L/4 + dev of one of the two.  The clearance map must say every cell that near (+2 cells for
//           the pose's place inside its cell and the rounding of the cell index) is free and inside the grid.
//   box     a box is convex, so both ends inside it shrunk by dev => every pose inside (64 hits per step, known without
//           sampling); both ends beyond one face grown by dev => no pose inside.  In front of that a circle: every pose lies
//           within L/2 + dev of the chord's midpoint, the box within its own reach of its centre, which moves at most |Speed| ht
//           around where it is at the middle step's time, ht = the farthest of tF and tE from it.
//   Gaussian  the same circle with the 1e-13 radius for the reach (no "inside": the density varies).
// Two separate answers come out: no pose of the chunk can be on a blocked cell; no pose can be inside an obstacle.  Both, with
// the heading bits known, skip the chunk; one alone still spares the sweep that half of its per-step work (PP_SKIP_* bits).
template <bool GAUSSIAN, typename Ends, typename Each>
__device__ __forceinline__ void pp_plan_chunk(const PPParams& p, const PPEdgeSetupBody* S, const long long e, const int chunk, const double* tg,
                                              const double endTime, const double tF, Ends ends, Each each) {
    const int k0 = chunk * PP_WAVE;
    unsigned char* skipb = p.track_skip + (size_t)e * p.nch + chunk;
    if (!(tF < endTime)) { *skipb = 0; return; }               // the sweep never reaches this chunk: most threads of a short edge
    // only whole chunks can be skipped, but a chunk cut by the end of the time grid is still sampled, and if the chunk before it is
    // skipped the sweep takes `lastHeading` from here like for any other chunk (tools/fuzz_parity.py seed 17 round 3: an edge of 291
    // steps on a 300-step grid)
    const bool whole = k0 + PP_WAVE - 1 < p.ng;
    const bool cov = (S->cbits & PPGPU_EDGE_COVERAGE) != 0;
    const double wStart = S->wStart, speed = S->speed, length = S->length, rho = S->rho, rho_inv = S->rho_inv;
    const double tM = whole ? tg[k0 + PP_WAVE / 2] : tF, tL = whole ? tg[k0 + PP_WAVE - 1] : tF;
    const double tP = (k0 > 0) ? tg[k0 - 1] : 0.0;
    const double dP = (tP - wStart) * speed, dF = (tF - wStart) * speed, dL = (tL - wStart) * speed;
    const bool okGeom = whole && tL < endTime && (dF >= 0.0) && (dL <= length);   // 64 steps, all before the end time, on the curve proper
    const double hi0 = S->p0, hi1 = S->hi1;
    unsigned long long eqWord = ~0ull;
    double tpP = 0.0;
    int segP = 0;
    bool okHead = true;                                        // the heading-unchanged bits of the chunk are known without sampling
    if (!cov) {
        // the step before the chunk: its heading is what the first step of the chunk is compared with
        tpP = (rho_inv != 0.0) ? dP * rho_inv : dP / rho;
        const double tpL = (rho_inv != 0.0) ? dL * rho_inv : dL / rho;
        segP = pp_seg_of(tpP, hi0, hi1);
        const int segL = pp_seg_of(tpL, hi0, hi1);
        const bool straight = pp_word_seg_type(S->type, segL) == 1;
        eqWord = straight ? ~0ull : 0ull;
        if (k0 > 0) {
            okHead = (dP >= 0.0) && (segP == segL) && (straight || (tpL - tpP) > 65.0 * 1e-9);
        } else {
            // the first chunk: its first step is compared with the source vertex's heading (`lastHeading` starts there, Edge.cpp:96),
            // which is one evaluation of the sweep's own heading expression — no sine or cosine in it
            const double tpF = (rho_inv != 0.0) ? dF * rho_inv : dF / rho;
            const int segF = pp_seg_of(tpF, hi0, hi1);
            okHead = (dF >= 0.0) && (segF == segL) && (straight || (tpL - tpF) > 64.0 * 1e-9);
            const PPSegBase* g = &S->seg[segF];
            const int gtype = pp_word_seg_type(S->type, segF);
            const double tt = (tpF - pp_seg_o1(segF, S->p0)) - pp_seg_o2(segF, S->p1);
            const double uth0 = (gtype == 1) ? (0.0 + g->bth) : ((gtype == 0) ? (tt + g->bth) : (-tt + g->bth));
            const bool same0 = pp_heading_from_yaw(pp_mod2pi(uth0)) == S->srcH;
            eqWord = (eqWord & ~1ull) | (same0 ? 1ull : 0ull);
        }
    }
    bool gridClear = false, obstClear = false;
    int nInside = 0;                                           // obstacles that hold EVERY pose of the chunk (binary model)
    bool decided = false;                                      // every obstacle either holds all poses or none
    if (okGeom) {
        double xF, yF, xE, yE, tE = tL, dE = dL;
        ends(dF, dL, xF, yF, xE, yE, tE, dE);
        const double ht = fmax(tE - tM, tM - tF);
        const double Lc = dE - dF;
        // rho_inv is not zero only where rho is a power of two: there 8 rho and 0.125 rho_inv are exact and the product is the
        // quotient, to the bit, without the division's thirty instructions
        const double dev = ((rho_inv != 0.0) ? Lc * Lc * (0.125 * rho_inv) : Lc * Lc / (8.0 * rho)) * (1.0 + 1e-9) + 1e-3;
        gridClear = true;
        if (p.grid.rows != 0) {
            const int need = (int)((0.25 * Lc + dev) * p.grid.inv_res) + 2;
            for (int h = 0; h < 2; h++) {
                const double f = h ? 0.75 : 0.25;
                const double x = xF + f * (xE - xF), y = yF + f * (yE - yF);
                const double cx = x * p.grid.inv_res, cy = y * p.grid.inv_res;
                const bool inside = (x >= 0.0) & (y >= 0.0) & (cx < (double)p.grid.cols) & (cy < (double)p.grid.rows);
                int clear = 0;
                if (inside) clear = (int)p.grid.clearance[(size_t)(unsigned)cy * p.grid.cols + (unsigned)cx];
                gridClear = gridClear && inside && (need < PP_CLEAR_CAP) && (clear > need);
            }
        }
        decided = true;
        auto against = [&](const PPObst& o) {
            if (GAUSSIAN) {
                if (!pp_chunk_clear_of<true>(o, 0.5 * (xF + xE), 0.5 * (yF + yE), tM, 0.5 * Lc + dev, ht)) decided = false;
                return;
            }
            {
                // most boxes on an edge's list are nowhere near this chunk (this sum is not pp_chunk_clear_of's, to the bit)
                const double dtM = tM - o.Time;
                const double ddx = 0.5 * (xF + xE) - (o.X + o.Speed * dtM * o.cosYaw), ddy = 0.5 * (yF + yE) - (o.Y + o.Speed * dtM * o.sinYaw);
                const double R = o.reach + 0.5 * Lc + dev + fabs(o.Speed) * ht + 1e-3;
                if (ddx * ddx + ddy * ddy > R * R) return;
            }
            const double dtF = tF - o.Time, dtE = tE - o.Time;
            const double txF = xF - (o.X + o.Speed * dtF * o.cosYaw), tyF = yF - (o.Y + o.Speed * dtF * o.sinYaw);
            const double txE = xE - (o.X + o.Speed * dtE * o.cosYaw), tyE = yE - (o.Y + o.Speed * dtE * o.sinYaw);
            const double rxF = txF * o.cosYaw - tyF * o.sinYaw, ryF = txF * o.sinYaw + tyF * o.cosYaw;
            const double rxE = txE * o.cosYaw - tyE * o.sinYaw, ryE = txE * o.sinYaw + tyE * o.cosYaw;
            const bool out = (fmin(rxF, rxE) > o.halfL + dev) | (fmax(rxF, rxE) < -o.halfL - dev) | (fmin(ryF, ryE) > o.halfW + dev) | (fmax(ryF, ryE) < -o.halfW - dev);
            const bool in = (fmax(fabs(rxF), fabs(rxE)) < o.halfL - dev) & (fmax(fabs(ryF), fabs(ryE)) < o.halfW - dev);
            if (in) nInside++;
            else if (!out) decided = false;
        };
        each(against, decided);
        obstClear = decided && nInside == 0;
    }
    const bool ok = okGeom && okHead && gridClear && decided;
    *skipb = ok ? (unsigned char)(PP_SKIP_ALL | (nInside > 0 ? PP_SKIP_HITS : 0)) : (unsigned char)((gridClear ? PP_SKIP_GRID : 0) | (obstClear ? PP_SKIP_OBST : 0));
    if (ok) {
        // (the per-step counts of a skipped chunk are not stored: every step is inside the same nInside boxes, and the one reader
        // that can stop inside a skipped chunk — the cover sweep, when coverage completes there — divides the chunk's sum by 64;
        // round 2 wrote them, 128 bytes per such chunk: half of this kernel's 205 MB of writes)
        p.track_chunk_hits[(size_t)e * p.nch + chunk] = (unsigned)(PP_WAVE * nInside);
        if (!cov) p.track_eq[(size_t)e * p.nch + chunk] = eqWord;
        if (GAUSSIAN) p.track_chunk_pen[(size_t)e * p.nch + chunk] = 0.0;
    } else if (!cov && k0 > 0 && dP >= 0.0 && dP <= length) {
        // not skipped: if the chunk before this one is, the sweep takes `lastHeading` from here
        double ux, uy, uth;
        pp_setup_seg_pose(S, segP, tpP, ux, uy, uth);
        p.track_eq[(size_t)e * p.nch + chunk] = (unsigned long long)__double_as_longlong(pp_heading_from_yaw(pp_mod2pi(uth)));   // (the sweep replaces it by the chunk's bits)
    }
}
// The chunkwise caller: the thread samples both ends of its chunk's own 64 steps and goes through the obstacles that can come near
// the edge at all (pp_k_solve_edges left the list in the setup record), or through the whole table when it holds more than 64.
template <bool GAUSSIAN>
__device__ __forceinline__ void pp_plan_skips_chunk(const PPParams& p, const PPEdgeSetupBody* S, const PPObst* OB, const long long e, const int chunk) {
    const bool sane = !(S->sflags & PP_SETUP_NO_SWEEP) && S->type >= 0;      // (a shared edge: its head is planned)
    const double endTime = fmin(p.horizon + 1e-12 + p.sst, S->wEnd);
    const double* tg = p.tgrid + (size_t)(sane ? S->vi : 0) * p.ng;
    const double tF = (sane && chunk * PP_WAVE < p.ng) ? tg[chunk * PP_WAVE] : INFINITY;
    pp_plan_chunk<GAUSSIAN>(p, S, e, chunk, tg, endTime, tF,
        [&](double dF, double dL, double& xF, double& yF, double& xE, double& yE, double&, double&) {
            // Keep this order, both ends evaluated on the unit curve before either is placed: pp_plan_pose twice costs
            // pp_k_plan_skips_chunkwise six more spilled registers and the Gaussian kernels a wave (profiles/plan_skips_shared.txt)
            double uxF, uyF, uxE, uyE;
            pp_plan_unit_pose(S, dF, uxF, uyF);
            pp_plan_unit_pose(S, dL, uxE, uyE);
            pp_plan_place(S, uxF, uyF, xF, yF);
            pp_plan_place(S, uxE, uyE, xE, yE);
        },
        [&](auto& against, const bool& decided) {
            unsigned long long m = S->omask;
            if (p.n_obst > PP_WAVE) m = 0ull;
            while (decided && m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                against(OB[j]);
            }
            if (p.n_obst > PP_WAVE)
                for (int j = 0; j < p.n_obst && decided; j++) against(OB[j]);
        });
}
// The workgroup's `ne` setup records (contiguous in the workspace from edge el0 on) into s_setup and, OBST_LDS, the obstacle table
// into s_obst; the caller's barrier follows.  A thread reads some 40 fields of its record and ten doubles per obstacle it tests;
// from memory every one of those was a vector load whose lanes hit two or three different lines, ≈ 200 per thread, and the kernel
// ran at the rate the L1 serves such loads, not at the VALU's (round 3).
// LISTED (a compile-time property: the kernels of a launch without a list are the code they were before there was one): the
// workgroup's edges are entries el0 .. el0 + ne - 1 of the sweep list (pp_k_mark_sweeps), read once into s_slot; each record is still
// contiguous.  Otherwise they are those slice positions themselves.
template <bool LISTED>
__device__ __forceinline__ long long pp_plan_count(const PPParams& p) {
    return LISTED ? (long long)(unsigned)pp_const_i32(&p.words->sweep_count)[0] : p.n_edges;
}
template <bool OBST_LDS, bool LISTED>
__device__ __forceinline__ void pp_plan_stage(const PPParams& p, const long long el0, const int ne, double* s_setup, PPObst* s_obst, unsigned* s_slot) {
    const int tid = (int)threadIdx.x;
    if (LISTED) {
        if (tid < ne) s_slot[tid] = p.sweep_list[el0 + tid];
        __syncthreads();
        for (int i = tid; i < ne * PP_SETUP_GLOBAL_WORDS; i += 256) {
            const int ed = i / PP_SETUP_GLOBAL_WORDS, w = i - ed * PP_SETUP_GLOBAL_WORDS;
            const double* src = reinterpret_cast<const double*>(p.setup + p.ws_base + (long long)s_slot[ed]);
            if (w < PP_SETUP_WORDS) s_setup[ed * PP_SETUP_LDS_STRIDE + w] = src[w];
        }
    } else {
        const double* src = reinterpret_cast<const double*>(p.setup + p.ws_base + el0);
        for (int i = tid; i < ne * PP_SETUP_GLOBAL_WORDS; i += 256) {
            const int ed = i / PP_SETUP_GLOBAL_WORDS, w = i - ed * PP_SETUP_GLOBAL_WORDS;
            if (w < PP_SETUP_WORDS) s_setup[ed * PP_SETUP_LDS_STRIDE + w] = src[i];
        }
    }
    if (OBST_LDS) {
        const double* os = reinterpret_cast<const double*>(p.obst);
        double* od = reinterpret_cast<double*>(s_obst);
        for (int i = tid; i < p.n_obst * (int)(sizeof(PPObst) / sizeof(double)); i += 256) od[i] = os[i];
    }
}
// One workgroup per `epw` consecutive entries of the sweep list — or edges of the slice, where the launch has no list; a workgroup
// whose first entry lies past the list's end leaves as a whole — (host: as many as give it 256 (edge, chunk) pairs, at most PP_PLAN_EDGES_MAX), one
// THREAD per (edge, chunk) — measured against one lane per edge walking its chunks (0.29 ms at config 3: 24 dependent iterations
// on 3 700 wavefronts) this mapping took 0.21 ms, most threads of a short edge leaving after two loads.
template <bool GAUSSIAN, bool OBST_LDS, bool LISTED>
__device__ __forceinline__ void pp_plan_skips_thread(const PPParams& p, int epw) {
    __shared__ double s_setup[PP_PLAN_EDGES_MAX * PP_SETUP_LDS_STRIDE];
    __shared__ PPObst s_obst[OBST_LDS ? PP_WAVE : 1];
    __shared__ unsigned s_slot[LISTED ? PP_PLAN_EDGES_MAX : 1];
    const int tid = (int)threadIdx.x;
    const long long el0 = (long long)blockIdx.x * epw, n = pp_plan_count<LISTED>(p);
    if (LISTED && el0 >= n) return;                            // (the whole workgroup, past the end of the list: nothing staged, no barrier met)
    const int ne = (int)((n - el0 < (long long)epw) ? (n - el0) : (long long)epw);
    pp_plan_stage<OBST_LDS, LISTED>(p, el0, ne, s_setup, s_obst, s_slot);
    __syncthreads();
    // (blockIdx.y: further tiles of 256 chunks when one edge alone has more than 256 of them)
    const int t = (int)blockIdx.y * 256 + tid;
    if (t >= ne * p.nch) return;
    const int el = (int)((unsigned)t / (unsigned)p.nch);
    const int chunk = t - el * p.nch;
    const PPEdgeSetupBody* S = reinterpret_cast<const PPEdgeSetupBody*>(&s_setup[el * PP_SETUP_LDS_STRIDE]);
    pp_plan_skips_chunk<GAUSSIAN>(p, S, OBST_LDS ? s_obst : p.obst, p.ws_base + (LISTED ? (long long)s_slot[el] : el0 + el), chunk);
}
#ifndef PP_PLAN_MIN_WAVES
#define PP_PLAN_MIN_WAVES 8   // 62 VGPRs, no spills; 0.28 -> 0.27 ms against the compiler's own choice (6 waves)
#endif
// the obstacle table in LDS (up to 64 obstacles; PPGPU_PLAN_SPANS=0: the tests compare the span planner below with these, and A/B runs
// take both from one library) / read from memory (more)
__global__ __launch_bounds__(256, PP_PLAN_MIN_WAVES) void pp_k_plan_skips_chunkwise(PPParams p, int epw) { pp_plan_skips_thread<false, true, true>(p, epw); }
__global__ __launch_bounds__(256) void pp_k_plan_skips_many(PPParams p, int epw) { pp_plan_skips_thread<false, false, true>(p, epw); }
__global__ __launch_bounds__(256) void pp_k_plan_skips_gaussian_chunkwise(PPParams p, int epw) { pp_plan_skips_thread<true, true, true>(p, epw); }
__global__ __launch_bounds__(256) void pp_k_plan_skips_gaussian_many(PPParams p, int epw) { pp_plan_skips_thread<true, false, true>(p, epw); }
// ... and the same four for a launch without a sweep list (`_direct`: they index the slice)
__global__ __launch_bounds__(256, PP_PLAN_MIN_WAVES) void pp_k_plan_skips_chunkwise_direct(PPParams p, int epw) { pp_plan_skips_thread<false, true, false>(p, epw); }
__global__ __launch_bounds__(256) void pp_k_plan_skips_many_direct(PPParams p, int epw) { pp_plan_skips_thread<false, false, false>(p, epw); }
__global__ __launch_bounds__(256) void pp_k_plan_skips_gaussian_chunkwise_direct(PPParams p, int epw) { pp_plan_skips_thread<true, true, false>(p, epw); }
__global__ __launch_bounds__(256) void pp_k_plan_skips_gaussian_many_direct(PPParams p, int epw) { pp_plan_skips_thread<true, false, false>(p, epw); }

// The span caller (up to 64 obstacles, the table in LDS): the same decisions with two pieces of work taken out of the thread.  The
// workgroup goes through three phases, and every thread stays to the last barrier (what is an early return above is a predicate
// here):
//
//   boundary poses   The chord of chunk c runs from its first step 64c to step 64c + 64, the first step of chunk c + 1, where that
//                    step exists, lies before the edge's end time and on the curve proper, and belongs to a thread of this
//                    workgroup: each thread samples ONE pose, its first step's, leaves it in LDS, and takes the far end from its
//                    neighbour.  Otherwise it samples its own last step 64c + 63 as the chunkwise caller does.  pp_plan_chunk
//                    states every bound for the steps [64c, E] the chord spans, whichever E it is given.
//   span masks       A span is PP_PLAN_SPAN consecutive chunks of an edge, and its PP_PLAN_SPAN threads share out the edge's omask
//                    (obstacle j goes to thread j mod PP_PLAN_SPAN; a short last span deals the residues round) to test each obstacle
//                    ONCE for the whole span.  With A the pose at the span's first step (time tA, arc length dA):
//                      two ends   B = the pose at the next span's first step, from LDS (tB, dB).  Every step the span's chords cover
//                                 lies between the two, so its pose P has |PA| + |PB| <= Ls = dB - dA (arc lengths bound chords) and
//                                 |P - (A+B)/2| = |(P-A) + (P-B)| / 2 <= Ls/2; its time is within (tB - tA)/2 of (tA + tB)/2, and an
//                                 obstacle's centre moves at |Speed|.
//                      one end    no such B (the edge ends in the span, or the tile does): a chord is only used by a chunk whose steps
//                                 all lie before the end time on the curve proper, so every covered step has t <= tE = min(time of
//                                 the step after the span's last, or of the row's last entry; end time) and d <= dE = min((tE - wStart) speed, length), and
//                                 |PA| <= dE - dA; the obstacle's centre is within |Speed| (tE - tA) of where it is at tA.
//                    An obstacle farther from that centre than reach + the pose radius + the obstacle's drift + 1e-3 (the slack of
//                    pp_plan_chunk's bounds; the pose radius carries 1e-9 relative and 1e-3 besides) cannot hold a pose any chord of
//                    the span covers: against() would answer "out" or not run its box test, and leaving the obstacle out answers the
//                    same.  (It can answer "out" where the box test's four faces could not decide: the span planner may skip a chunk
//                    the chunkwise one samples, never the other way round for these obstacles.)  A span whose first pose is not
//                    there keeps the whole omask.
//   chunks           pp_plan_chunk, over the span's mask.
#ifndef PP_PLAN_SPAN
#define PP_PLAN_SPAN 4        // 2 / 4 / 8: profiles/plan_spans_ab.txt
#endif
static_assert(PP_PLAN_SPAN >= 2 && PP_PLAN_SPAN <= 32 && 256 % PP_PLAN_SPAN == 0, "a span may not straddle a 256-chunk tile of a long edge (and 256 threads clear the span words)");
#define PP_PLAN_SPANS_MAX (256 / PP_PLAN_SPAN + PP_PLAN_EDGES_MAX)   // epw ceil(nch / SPAN) <= (epw nch + epw (SPAN - 1)) / SPAN < 256 / SPAN + 32
template <bool GAUSSIAN, bool LISTED>
__device__ __forceinline__ void pp_plan_skips_spans(const PPParams& p, int epw) {
    constexpr int LOG = __builtin_ctz(PP_PLAN_SPAN);
    __shared__ double s_setup[PP_PLAN_EDGES_MAX * PP_SETUP_LDS_STRIDE];
    __shared__ PPObst s_obst[PP_WAVE];
    __shared__ double s_bx[256], s_by[256];                    // the pose at each thread's first step; x = NaN: none
    __shared__ unsigned long long s_span[PP_PLAN_SPANS_MAX];
    __shared__ unsigned s_slot[LISTED ? PP_PLAN_EDGES_MAX : 1];
    const int tid = (int)threadIdx.x;
    const long long el0 = (long long)blockIdx.x * epw, n = pp_plan_count<LISTED>(p);
    if (LISTED && el0 >= n) return;                            // (the whole workgroup, past the end of the list: nothing staged, no barrier met)
    const int ne = (int)((n - el0 < (long long)epw) ? (n - el0) : (long long)epw);
    pp_plan_stage<true, LISTED>(p, el0, ne, s_setup, s_obst, s_slot);
    if (tid < PP_PLAN_SPANS_MAX) s_span[tid] = 0ull;
    __syncthreads();
    // (blockIdx.y: further tiles of 256 chunks when one edge alone has more than 256 of them)
    const int t = (int)blockIdx.y * 256 + tid;
    const bool live = t < ne * p.nch;                          // (the others work on edge 0's chunk 0 and store nothing)
    const int el = live ? (int)((unsigned)t / (unsigned)p.nch) : 0;
    const int chunk = live ? t - el * p.nch : 0;
    const PPEdgeSetupBody* S = reinterpret_cast<const PPEdgeSetupBody*>(&s_setup[el * PP_SETUP_LDS_STRIDE]);
    const int k0 = chunk * PP_WAVE;
    const bool sane = !(S->sflags & PP_SETUP_NO_SWEEP) && S->type >= 0;      // (a shared edge: its head is planned)
    const double endTime = fmin(p.horizon + 1e-12 + p.sst, S->wEnd);
    const double* tg = p.tgrid + (size_t)(sane ? S->vi : 0) * p.ng;
    const double tF = (live && sane && k0 < p.ng) ? tg[k0] : INFINITY;
    const double wStart = S->wStart, speed = S->speed;
    // ---- boundary poses
    {
        const double dF = (tF - wStart) * speed;
        double x = NAN, y = 0.0;
        if (tF < endTime && dF >= 0.0 && dF <= S->length) pp_plan_pose(S, dF, x, y);
        s_bx[tid] = x; s_by[tid] = y;
    }
    __syncthreads();
    // ---- span masks
    const int sp = live ? el * ((p.nch + PP_PLAN_SPAN - 1) >> LOG) + ((chunk - (int)blockIdx.y * 256) >> LOG) : 0;
    {
        const int r = chunk & (PP_PLAN_SPAN - 1), cA = chunk - r, tidA = tid - r;
        const int nT = (p.nch - cA < PP_PLAN_SPAN) ? p.nch - cA : PP_PLAN_SPAN;       // threads of this span
        unsigned long long mine = 0ull;
        for (int q = r; q < PP_PLAN_SPAN; q += nT) mine |= (~0ull / ((1ull << PP_PLAN_SPAN) - 1ull)) << q;   // bits q, q + SPAN, q + 2 SPAN ...
        unsigned long long m = live ? (S->omask & mine) : 0ull;
        unsigned long long keep = m;
        const double xA = s_bx[tidA], yA = s_by[tidA];
        if (m != 0ull && xA == xA) {
            const double tA = tg[cA * PP_WAVE], dA = (tA - wStart) * speed;
            const int cB = cA + PP_PLAN_SPAN, tidB = tidA + PP_PLAN_SPAN;
            const bool inTile = cB < p.nch && tidB < 256;
            const double xB = inTile ? s_bx[tidB] : NAN, yB = inTile ? s_by[tidB] : 0.0;
            double cx, cy, rad, tc, th;
            if (xB == xB) {
                const double tB = tg[cB * PP_WAVE], dB = (tB - wStart) * speed;
                cx = 0.5 * (xA + xB); cy = 0.5 * (yA + yB); rad = 0.5 * (dB - dA); tc = 0.5 * (tA + tB); th = 0.5 * (tB - tA);
            } else {
                const int kE = (cB * PP_WAVE < p.ng) ? cB * PP_WAVE : p.ng - 1;
                const double tE = fmin(tg[kE], endTime), dE = fmin((tE - wStart) * speed, S->length);
                cx = xA; cy = yA; rad = dE - dA; tc = tA; th = tE - tA;
            }
            if (rad >= 0.0 && th >= 0.0) {
                rad = rad * (1.0 + 1e-9) + 1e-3; th = th * (1.0 + 1e-9);
                while (m) {
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const PPObst& o = s_obst[j];
                    const double dt = tc - o.Time;
                    const double ddx = cx - (o.X + o.Speed * dt * o.cosYaw), ddy = cy - (o.Y + o.Speed * dt * o.sinYaw);
                    const double R = o.reach + rad + fabs(o.Speed) * th + 1e-3;
                    if (ddx * ddx + ddy * ddy > R * R) keep &= ~(1ull << j);
                }
            }
        }
        if (keep != 0ull) atomicOr(&s_span[sp], keep);
    }
    __syncthreads();
    // ---- the chunk (no barrier from here on).  The lambdas take what they need from the record again: a value loaded in front of
    // the barriers and captured here stays in a register through the whole decision, and pp_k_plan_skips has none to spare.
    if (!live) return;
    pp_plan_chunk<GAUSSIAN>(p, S, p.ws_base + (LISTED ? (long long)s_slot[el] : el0 + el), chunk, tg, endTime, tF,
        [&](double, double dL, double& xF, double& yF, double& xE, double& yE, double& tE, double& dE) {
            xF = s_bx[tid]; yF = s_by[tid];                    // (0 <= dF <= dL <= length, so this thread left its pose there)
            // the far end E of the chord: the neighbour's first step, or this chunk's last
            xE = NAN; yE = 0.0;
            if (tid + 1 < 256 && chunk + 1 < p.nch) { xE = s_bx[tid + 1]; yE = s_by[tid + 1]; }
            if (xE == xE) {
                tE = tg[chunk * PP_WAVE + PP_WAVE]; dE = (tE - S->wStart) * S->speed;
            } else {
                pp_plan_pose(S, dL, xE, yE);
            }
        },
        [&](auto& against, const bool& decided) {
            unsigned long long m = s_span[sp];                 // the obstacles that can come near this span of the edge
            while (decided && m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                against(s_obst[j]);
            }
        });
}
__global__ __launch_bounds__(256, PP_PLAN_MIN_WAVES) void pp_k_plan_skips(PPParams p, int epw) { pp_plan_skips_spans<false, true>(p, epw); }
__global__ __launch_bounds__(256, PP_PLAN_MIN_WAVES) void pp_k_plan_skips_gaussian(PPParams p, int epw) { pp_plan_skips_spans<true, true>(p, epw); }
__global__ __launch_bounds__(256, PP_PLAN_MIN_WAVES) void pp_k_plan_skips_direct(PPParams p, int epw) { pp_plan_skips_spans<false, false>(p, epw); }
__global__ __launch_bounds__(256, PP_PLAN_MIN_WAVES) void pp_k_plan_skips_gaussian_direct(PPParams p, int epw) { pp_plan_skips_spans<true, false>(p, epw); }

// e = the edge's slot in the workspace.  GAUSSIAN: the dynamic obstacles are GaussianDynamicObstaclesManager's (its own
// instantiation: exp() and the density bookkeeping would otherwise cost the common kernel registers).
//
// The wave is short (some 760 VALU instructions) and spent seven eighths of its life waiting on a chain of dependent loads: record,
// then vertex and time row, then the obstacle row of the lane, then per sampled chunk the times, the grid words, the obstacle rows
// and the branch that ends the edge.  So the loads are issued in as few rounds as the data dependences allow:
//   * at wave start everything whose address follows from the work item alone: the record, the skip bytes, the lane's obstacle row
//     (the source heading travels in the record: pp_k_solve_edges);
//   * the loop steps through the set bits of "not skipped" instead of 64 trips with `continue`, one sampled chunk per trip: its
//     times (and `carry` word) are asked for at the end of the trip before (next_chunk; the first chunk's before the obstacle lanes
//     are set up), then its poses, then its grid words;
//   * the loop is left where the edge ends: the chunk's first step lies at or after the end time, a step is blocked, or the chunk
//     is cut by the end time.
// (Two or three sampled chunks in flight per wave measured slower at config 3: registers the kernel does not have at 6 waves per
// SIMD, and poses a blocked first chunk throws away.  DESIGN.md Appendix B has the figures and the commit that holds that walk.)
template <bool GAUSSIAN>
__device__ __forceinline__ void pp_pose_sweep_edge(const PPParams& p, const long long e) {
    const int lane = pp_lane();
    const PPEdgeSetup* S = p.setup + e;
    PPTrackSummary* sum = p.track_summary + e;
    // ---- the loads that need nothing but the work item, before the first wait
    // Chunks of 64 steps that provably touch neither a blocked cell nor an obstacle are not sampled at all (pp_k_plan_skips decided
    // which, one thread per chunk); the others go through the per-step code below, one step per lane.
    const unsigned char* skipb = p.track_skip ? p.track_skip + (size_t)e * p.nch : nullptr;
    unsigned sbits = (skipb && lane < p.nch) ? (unsigned)skipb[lane] : 0u;     // the skip bytes of the first 64 chunks
    // Up to 64 obstacles: lane i answers for obstacle i's motion during the whole sweep (position at the first step's time, velocity,
    // squared culling radius), so the per-chunk culling below is a dozen instructions and no trip to memory.  The bound is the one
    // pp_obstacle_hits_chunk uses (reach + chunk span + |Speed| * chunk time + slack); it only has to be conservative.
    const bool laneCull = p.n_obst <= PP_WAVE;
    PPObst ol;
    if (laneCull && p.ng > 0 && p.n_obst > 0) {
        // (every lane loads a row, the lanes past the table its last one: no lane masking around the loads)
        const PPObst* o = p.obst + (lane < p.n_obst ? lane : p.n_obst - 1);
        ol.X = o->X; ol.Y = o->Y; ol.cosYaw = o->cosYaw; ol.sinYaw = o->sinYaw; ol.Speed = o->Speed; ol.Time = o->Time; ol.reach = o->reach;
    }
    // the whole record in one round: the fields are asked for together and pinned here, ahead of the test of its flags, or the
    // compiler moves each load down to the branch that first needs it and the wave makes four trips to the record's four lines
    const unsigned sflags = (unsigned)PP_SI32(sflags);
    const int dubType = PP_SI32(type);
    const unsigned vi = (unsigned)PP_SI32(vi);
    const unsigned cbitsW = (unsigned)PP_SI32(cbits);
    const double srcH = PP_SF64(srcH);
    const PPCurveHot hot = pp_curve_hot(S);
    const double wEnd = PP_SF64(wEnd), wStart = hot.wStart, speed = hot.speed;
    const unsigned long long omask = pp_const_u64(&S->omask)[0];
    // the segment of the curve the sweep is on: its constants live in scalar registers, the other two stay in memory
    int cur = 0;
    PPSeg cs = pp_seg_load_uniform(&S->seg[0], 0, PP_SF64(p0), PP_SF64(p1), PP_SF64(hi1), dubType);
    asm volatile("" :: "s"(sflags), "s"(dubType), "s"(vi), "s"(cbitsW), "s"(srcH), "s"(hot.wStart), "s"(hot.speed), "s"(hot.length), "s"(hot.rho),
                 "s"(hot.rho_inv), "s"(hot.qx), "s"(hot.qy), "s"(wEnd), "s"(omask), "s"(cs.bx), "s"(cs.by), "s"(cs.bth), "s"(cs.sb), "s"(cs.cb),
                 "s"(cs.hi));
    const bool cov = (cbitsW & PPGPU_EDGE_COVERAGE) != 0;
    if ((sflags & PP_SETUP_NO_SWEEP) || dubType < 0) {            // (a shared edge: its head is swept)
        if (lane == 0) { sum->limit = 0; sum->blocked = 0; sum->dub_err = 0; sum->pad = 0; }
        return;
    }
    const double endTime = fmin(p.horizon + 1e-12 + p.sst, wEnd);    // Edge.cpp:90 (the cover sweep may end the edge earlier)
    const double* tg = p.tgrid + (size_t)vi * p.ng;
    if (p.wedges && p.ng > 0) {
        // a given curve that starts after the vertex's first step: DubinsWrapper::sample throws at that step, the loop
        // catches it, marks the edge infeasible and stops without counting the step (Edge.cpp:126-133)
        const double t0 = pp_const_f64(tg)[0];
        if (t0 < endTime && t0 < wStart) {
            if (lane == 0) { sum->limit = 0; sum->blocked = 2; sum->dub_err = 0; sum->pad = 0; }
            return;
        }
    }
    unsigned short* thits = p.track_hits + (size_t)e * p.ngp;
    unsigned long long* teq = p.track_eq + (size_t)e * p.nch;
    unsigned* tch = p.track_chunk_hits + (size_t)e * p.nch;
    const bool gaussian = GAUSSIAN;
    // bounds used by the obstacle culling: how far the vehicle / time advance over one 64-step chunk
    const double chunkTime = 64.0 * (p.inc_d / p.max_speed);
    const double chunkSpan = 64.0 * (p.inc_d / p.max_speed) * speed;
    double carryHeading = srcH;                                       // `lastHeading`, Edge.cpp:96
    int anyErr = 0;
    int limit = 0, blocked = 0;
    // Can any obstacle come near this edge at all?  Every sampled pose lies within `travel` (arc length from the start of
    // the curve) of the curve's first point, and an obstacle moves at most |Speed| * duration during the sweep: the same
    // kind of exact bound as the per-chunk culling, applied once — by pp_k_solve_edges, which left the obstacles that pass it in the
    // record's omask (all ones with more than 64 obstacles: then the per-chunk culling alone decides, which is as exact).
    const bool anyObstacle = (p.n_obst > 0 && p.ng > 0) ? (omask != 0ull) : false;
    const double* carry = reinterpret_cast<const double*>(p.track_eq + (size_t)e * p.nch);   // (a chunk's word before the sweep gets to it)
    // the group of 64 chunks the walk is in: which are skipped, which are left to sample (todo), the planner's partial answers
    int g0 = -PP_WAVE;
    unsigned long long skips = 0ull, todo = 0ull, gclear = 0ull, oclear = 0ull;
    bool lastSkipped = false;                                         // the last chunk of the group before was skipped
    // the next chunk to sample: its times and, after a skipped chunk, the planner's `lastHeading`
    int ci;
    double t, carryW;
    bool after;
    auto next_chunk = [&]() {
        while (todo == 0ull) {
            lastSkipped = (g0 >= 0) && ((skips >> 63) & 1ull) != 0ull;
            g0 += PP_WAVE;
            if (g0 > 0) sbits = (skipb && g0 + lane < p.nch) ? (unsigned)skipb[g0 + lane] : 0u;   // (edges of more than 64 chunks; the first group's bytes came with the record)
            skips = __ballot((sbits & PP_SKIP_ALL) != 0u);
            gclear = __ballot((sbits & PP_SKIP_GRID) != 0u);
            oclear = anyObstacle ? __ballot((sbits & PP_SKIP_OBST) != 0u) : ~0ull;   // (no obstacle near the edge: as good as none near any chunk)
            todo = ~skips;                                            // (chunks past the row's end count as sampled: the walk ends at the first of them)
        }
        ci = __ffsll((long long)todo) - 1;                            // (the walk above ended on a group with chunks to sample)
        todo &= todo - 1ull;
        after = ci > 0 ? (((skips >> (ci - 1)) & 1ull) != 0ull) : lastSkipped;
        const int k = (g0 + ci) * PP_WAVE + lane;
        t = (k < p.ng) ? tg[k] : INFINITY;
        carryW = 0.0;
        if (!cov && after && g0 + ci < p.nch) carryW = pp_const_f64(carry + (g0 + ci))[0];
    };
    next_chunk();                                                     // (the first chunk's times travel while the obstacle lanes are set up)
    // The five doubles a lane keeps about its obstacle are read once per sampled chunk, by the culling alone: they wait in LDS, not
    // in ten registers the pose arithmetic in between needs (at 6 waves per SIMD the kernel has 80; kept in registers, one of the
    // five went to scratch and came back from memory in every chunk).  A wave reads only what it wrote itself.
    __shared__ double s_cull[PP_WPB * 5 * PP_WAVE];
    double* cullL = s_cull + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (5 * PP_WAVE) + lane;
    double cullT0 = 0;                                                // (wave-uniform: the row's first time)
    if (anyObstacle && laneCull) {
        const double t0 = pp_const_f64(tg)[0];
        cullT0 = t0;
        double oX0 = 0, oY0 = 0, oVx = 0, oVy = 0, oR2 = -1.0;
        if (lane < p.n_obst) {
            const PPObst& o = ol;
            const double dt = t0 - o.Time;
            oX0 = o.X + o.Speed * dt * o.cosYaw; oY0 = o.Y + o.Speed * dt * o.sinYaw;
            oVx = o.Speed * o.cosYaw; oVy = o.Speed * o.sinYaw;
            const double Rc = o.reach + chunkSpan + fabs(o.Speed) * chunkTime + 2e-3;
            oR2 = Rc * Rc;
        }
        cullL[0 * PP_WAVE] = oX0; cullL[1 * PP_WAVE] = oY0; cullL[2 * PP_WAVE] = oVx; cullL[3 * PP_WAVE] = oVy; cullL[4 * PP_WAVE] = oR2;
        pp_wave_lds_fence();
    }
    for (;;) {
        // ---- its poses; the grid words set off
        const double tFirst = pp_readlane(t, 0);
        const bool live = tFirst < endTime;                           // `while (intermediate.time() < endTime)`
        double x, y, heading;
        bool dubErr = false;
        PPCellRef cell;
        uint32_t word;
        unsigned long long near = 0ull;
        if (live) {
            const bool gridClear = ((gclear >> ci) & 1ull) != 0ull, obstClear = ((oclear >> ci) & 1ull) != 0ull;
            const bool valid = t < endTime;
            double uth;
            pp_window_pose(S, hot, cur, cs, t, tFirst, valid, x, y, uth, dubErr);
            // the heading itself (:47) only matters for "unchanged since the last step" (Edge.cpp:159), which only matters
            // on edges that may not cover while turning
            heading = cov ? 0.0 : pp_heading_from_yaw(pp_mod2pi(uth));
            if (!gridClear && p.grid.rows != 0) {                     // Edge.cpp:144 (pp_k_plan_skips may have ruled it out for the whole chunk)
                cell = pp_blocked_cell(p.grid, x, y);
                word = p.grid.bits[cell.word];
            }
            if (!obstClear && laneCull) {                             // :150-151
                // which obstacles can come near this chunk: lane j answers for obstacle j from its registers
                const double dtc = tFirst - cullT0;
                const double oX0 = cullL[0 * PP_WAVE], oY0 = cullL[1 * PP_WAVE], oVx = cullL[2 * PP_WAVE], oVy = cullL[3 * PP_WAVE], oR2 = cullL[4 * PP_WAVE];
                const double ddx = pp_readlane(x, 0) - (oX0 + oVx * dtc), ddy = pp_readlane(y, 0) - (oY0 + oVy * dtc);
                near = __ballot(!(ddx * ddx + ddy * ddy > oR2));      // oR2 = -1 in lanes without an obstacle
            }
        }
        // ---- resolved with the sequential code.  (Keep this part a block of its own, the two indices ahead of it: its `break`s
        // then leave through one common exit.  Without the braces the compiler lays the loop out differently — 1 690 instructions
        // against 1 655, 44 spilled scalars against 46 — and pp_k_pose_sweep measures 440 us against 422,
        // profiles/pose_queue_cleanup.txt.)
        const int base = (g0 + ci) * PP_WAVE;
        const int k = base + lane;
        {
#ifdef PP_DBG_TRACE
            if (pp_edge_position(p, p.e_base + (e - p.ws_base)) == (long long)(PP_DBG_TRACE) && lane == 0 && base < 400)
                printf("[pose] chunk at %d: sampled after skip %d (eq word %llx)\n", base, (int)after, (unsigned long long)teq[base >> 6]);
#endif
            if (!live) { limit = base; break; }
            // `lastHeading` (Edge.cpp:96,174) of the step before this chunk: the chunks in between were skipped, pp_k_plan_skips left it
            if (!cov && after) carryHeading = carryW;
            const bool obstClear = ((oclear >> ci) & 1ull) != 0ull;
            const bool valid = t < endTime;
            const bool gridTested = !(((gclear >> ci) & 1ull) != 0ull) && p.grid.rows != 0;
            const bool blk = gridTested ? (valid & pp_blocked_test(cell, word)) : false;
            int hits = 0;
            double dens = 0;
            if (obstClear) {
                // pp_k_plan_skips: no obstacle can hold a pose of this chunk
            } else if (laneCull) {
                unsigned long long m = near;
                while (m) {
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (!gaussian) { if (valid) hits += pp_obstacle_hit(pp_obst_load_uniform(p.obst + j), x, y, t); }
                    else dens += pp_obstacle_pdf(reinterpret_cast<const PPGauss*>(p.obst)[j], x, y, t);
                }
                if (gaussian) { if (dens < 1e-5) dens = 0; if (!valid) dens = 0; }   // GaussianDynamicObstaclesManager.cpp:11
            } else {
                if (!gaussian)
                    hits = pp_obstacle_hits_chunk(p.obst, p.n_obst, x, y, t, valid, pp_readlane(x, 0), pp_readlane(y, 0), tFirst, chunkSpan, chunkTime);
                else
                    dens = pp_obstacle_density_chunk(reinterpret_cast<const PPGauss*>(p.obst), p.n_obst, x, y, t, valid, pp_readlane(x, 0),
                                                     pp_readlane(y, 0), tFirst, chunkSpan, chunkTime);
            }
            unsigned long long eqMask = ~0ull;
            if (!cov) {
                double prevHeading = __shfl_up(heading, 1, PP_WAVE);
                if (lane == 0) prevHeading = carryHeading;
                eqMask = __ballot(prevHeading == heading);
#ifdef PP_DBG_TRACE
                if (pp_edge_position(p, p.e_base + (e - p.ws_base)) == (long long)(PP_DBG_TRACE) && lane == 0 && base < 400)
                    printf("[pose] chunk at %d sampled: carry %.17g heading0 %.17g heading1 %.17g eq %llx\n", base, prevHeading, heading, pp_readlane(heading, 1), (unsigned long long)eqMask);
#endif
                carryHeading = pp_readlane(heading, 63);           // (the next chunk's, when that one is adjacent)
            }
            if (__ballot(dubErr) != 0ull) anyErr = 1;

            const unsigned long long bm = __ballot(blk);
            const int fb = bm ? (__ffsll((long long)bm) - 1) : PP_WAVE;
            const int nvalid = __popcll(__ballot(valid));
            const int nlim = fb < nvalid ? fb : nvalid;

            int chunkHits = 0;
            if (__ballot(hits != 0) != 0ull) {
                // per-step counts are only ever read for a chunk whose sum is not zero
                chunkHits = pp_wave_sum_i(lane < nlim ? hits : 0);
                thits[k] = (unsigned short)(hits > 65535 ? 65535 : hits);
            }
            if (gaussian) {
                double chunkPen = 0;
                if (__ballot(dens != 0.0) != 0ull) {
                    chunkPen = pp_wave_sum_d(lane < nlim ? dens * p.cpf : 0.0);
                    p.track_pen[(size_t)e * p.ngp + k] = dens;
                }
                if (lane == 0) p.track_chunk_pen[(size_t)e * p.nch + (base >> 6)] = chunkPen;
            }
            if (lane == 0) {
                tch[base >> 6] = (unsigned)chunkHits;
                if (!cov) teq[base >> 6] = eqMask;                        // only read for edges that may not cover while turning
            }

            if (fb < nvalid) { limit = base + fb; blocked = 1; break; }
            if (nvalid < PP_WAVE) { limit = base + nvalid; break; }
            limit = base + PP_WAVE;
        }
        next_chunk();
    }
    if (lane == 0) { sum->limit = limit; sum->blocked = blocked; sum->dub_err = anyErr; sum->pad = 0; }
}

#ifndef PP_POSE_MIN_WAVES
#define PP_POSE_MIN_WAVES 6
#endif
// n_edges = slice size (ppgpu.hip: launch_cost).  The grid has a wave per edge of the slice either way: the host does not know how
// many of them are on the sweep list.  pp_k_pose_sweep / _gaussian are the kernels of a launch WITH a list: wave i asks for the count
// and the list's entry i together (two scalar loads) and leaves at or past the count.  The `_direct` kernels are those of a launch
// without one: wave i takes edge i, and pp_pose_sweep_edge leaves the edges that are not swept.  Two instantiations and not a branch on
// the pointer: the branch alone changes how the whole sweep is compiled (60 spilled SGPRs against 46, profiles/sweep_list.txt).
__device__ __forceinline__ void pp_pose_sweep_listed(const PPParams& p, bool& mine, long long& idx) {
    const unsigned count = (unsigned)pp_const_i32(&p.words->sweep_count)[0];       // (<= n_edges)
    const unsigned entry = (unsigned)pp_const_i32(p.sweep_list + idx)[0];          // (the list has room for the grid's last workgroup: in bounds whatever the count)
    mine = idx < (long long)count;
    idx = (long long)entry;
}
__global__ __launch_bounds__(PP_WPB * 64, PP_POSE_MIN_WAVES) void pp_k_pose_sweep(PPParams p) {
    int wave;
    long long idx = pp_wave_edge<PP_WPB>(wave);
    bool mine;
    pp_pose_sweep_listed(p, mine, idx);
    if (mine) pp_pose_sweep_edge<false>(p, p.ws_base + idx);
}
__global__ __launch_bounds__(PP_WPB * 64, 4) void pp_k_pose_sweep_gaussian(PPParams p) {
    int wave;
    long long idx = pp_wave_edge<PP_WPB>(wave);
    bool mine;
    pp_pose_sweep_listed(p, mine, idx);
    if (mine) pp_pose_sweep_edge<true>(p, p.ws_base + idx);
}
__global__ __launch_bounds__(PP_WPB * 64, PP_POSE_MIN_WAVES) void pp_k_pose_sweep_direct(PPParams p) {
    int wave;
    const long long idx = pp_wave_edge<PP_WPB>(wave);
    if (idx < p.n_edges) pp_pose_sweep_edge<false>(p, p.ws_base + idx);
}
__global__ __launch_bounds__(PP_WPB * 64, 4) void pp_k_pose_sweep_gaussian_direct(PPParams p) {
    int wave;
    const long long idx = pp_wave_edge<PP_WPB>(wave);
    if (idx < p.n_edges) pp_pose_sweep_edge<true>(p, p.ws_base + idx);
}

// ------------------------------------------------------------------------------------------
// Shared tracks (the rule and its proof: pp_k_solve.h).
//
// pp_k_arc_stops: one wave per class (pp_share_key), 64 steps of the vertex's time row per trip, the pose sweep's own arithmetic on
// the one thing every edge of the class has in common: segment 0.  Its base is {0, 0, qth, s0, c0} with qx, qy, rho and rho_inv as
// pp_curve_init forms them for every edge of the class (pp_curve_base, one piece of code for both), the segment is given the whole
// line (-inf, +inf) and the curve no end (length = +inf), so pp_window_pose stays on it whatever the step.  Only steps with
// t < horizon + 1e-12 + sst count, only the grid stops a sweep.  The entry is the first blocked step, or -1: none before the horizon,
// no grid, or an arc the bounded sine and cosine could not follow (no edge the solver accepts gets that far on its first arc; -1 only
// ever costs a class its sharing).  The loop is bounded by the row's length and no wave waits for another.
// The table changes with the vertices, the grid, the keep-out limit and the configuration: the host queues the kernel in front of
// the first launch that shares tracks after any of them changed, and not otherwise.
__global__ __launch_bounds__(PP_WPB * 64) void pp_k_arc_stops(PPParams p) {
    int wave;
    const long long key = pp_wave_edge<PP_WPB>(wave);
    if (key >= (long long)p.nverts * PP_SHARE_KEYS) return;
    const int lane = pp_lane();
    const unsigned vi = (unsigned)(key / PP_SHARE_KEYS), cbits = ((unsigned)key & (PP_SHARE_KEYS - 1u)) >> 1;
    const int segType = ((unsigned)key & 1u) ? 2 : 0;                    // (pp_share_key: 0 = a left arc, 1 = a right one)
    const ppgpu_vertex* V = p.verts + vi;
    const double rho = (cbits & PPGPU_EDGE_COVERAGE) ? p.rho_cov : p.rho;             // Edge.cpp:73-76
    const double speed = (cbits & PPGPU_EDGE_SLOW) ? p.slow_speed : p.max_speed;
    PPCurve cv;
    PPSincosMemo memo;
    pp_curve_base<PP_CR_SOLVE>(cv, V->x, V->y, pp_yaw(V->heading), rho, memo);
    const PPCurveHot hot = {V->time, speed, INFINITY, cv.rho, cv.rho_inv, cv.qx, cv.qy};
    PPSeg cs = PPSeg{0.0, 0.0, cv.qth, cv.s0, cv.c0, -INFINITY, INFINITY, 0.0, 0.0, segType};
    int cur = 0;
    const double bound = p.horizon + 1e-12 + p.sst;
    const double* tg = p.tgrid + (size_t)vi * p.ng;
    int kb = -1;
    if (p.grid.rows != 0) {
        double tNext = (lane < p.ng) ? tg[lane] : INFINITY;
        for (int k0 = 0; k0 < p.ng; k0 += PP_WAVE) {
            const double t = tNext;
            tNext = (k0 + PP_WAVE + lane < p.ng) ? tg[k0 + PP_WAVE + lane] : INFINITY;   // (the next trip's times travel during this one's poses)
            const double tFirst = pp_readlane(t, 0);
            if (!(tFirst < bound)) break;
            const bool valid = t < bound;
            {
                // (as pp_window_pose is about to form it: a tprime that is no number, or beyond what the solver lets a curve reach, ends the walk)
                const double d = ((valid ? t : tFirst) - hot.wStart) * hot.speed;
                const double tp = (hot.rho_inv != 0.0) ? d * hot.rho_inv : d / hot.rho;
                if (__ballot(!(fabs(cv.qth) + fabs(tp) < 9.0e4)) != 0ull) break;
            }
            double x, y, uth;
            bool dubErr = false;
            pp_window_pose(p.setup, hot, cur, cs, t, tFirst, valid, x, y, uth, dubErr);   // (the record is never looked at: tprime lies in the segment's interval)
            const PPCellRef cell = pp_blocked_cell(p.grid, x, y);
            const uint32_t word = p.grid.bits[cell.word];
            const unsigned long long bm = __ballot(valid & pp_blocked_test(cell, word));
            if (bm != 0ull) { kb = k0 + __ffsll((long long)bm) - 1; break; }
            if (__ballot(valid) != ~0ull) break;
        }
    }
    if (lane == 0) p.arc_stop[key] = kb;
}

// pp_k_track_fanout: after the pose sweep of a slice and before its approach kernel, PP_TF_LANES lanes per stop member (entry j of
// stop_list).  The count is on the device: the grid has at most PP_TF_GRID workgroups, which stride over the members, and the
// workgroups past the count leave at once.  The member goes onto the sweep list, behind the prefix the skip planner and the pose
// sweep have walked (pp_k_approach_events walks both parts as one list), and gets a copy of what those two left its head, as far
// as anyone reads it: the summary (limit = kb, blocked = 1); for the chunks 0 .. kb >> 6 the chunk's hit sum, its skip byte and, on an edge that may
// not cover while turning, its heading bits; and the 128-byte row of per-step hits of each of those chunks that was sampled and
// whose sum is not zero (the only rows a reader looks at: pp_lane_hit_sum).  The readers then find the member's track where they
// find any edge's, with no indirection.
// The kernel also leaves the stop classes' half of the table of heads all-ones for the next slice's solve: pp_k_mark_sweeps was its
// last reader (this kernel goes by stop_of).
#define PP_TF_LANES 16
#define PP_TF_GRID 2048       // workgroups at most: 32 768 members a pass
static_assert(PP_TF_LANES * sizeof(unsigned long long) == PP_WAVE * sizeof(unsigned short), "a row of per-step hits is one 8-byte word per lane");
__global__ __launch_bounds__(256) void pp_k_track_fanout(PPParams p) {
    const unsigned long long n_keys = (unsigned long long)p.nverts * PP_SHARE_KEYS;
    for (unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x; k < n_keys; k += (unsigned long long)gridDim.x * 256u)
        *pp_share_entry(p, pp_stop_key_base(p.nverts) + (unsigned)k) = PP_SHARE_NONE;
    const int sub = (int)(threadIdx.x % PP_TF_LANES);
    const long long count = (long long)(unsigned)pp_const_i32(&p.words->stop_count)[0], swept = (long long)(unsigned)pp_const_i32(&p.words->sweep_count)[0];
    for (long long j = (long long)blockIdx.x * (256 / PP_TF_LANES) + (threadIdx.x / PP_TF_LANES); j < count; j += (long long)gridDim.x * (256 / PP_TF_LANES)) {
        const unsigned slot = p.stop_list[j];
        if (sub == 0) p.sweep_list[swept + j] = slot;                   // (swept + count <= n_edges: within the list)
        const long long e = p.ws_base + (long long)slot;
        const long long h = p.ws_base + (long long)p.stop_of[e - p.ws_base];
        const int4 sum = reinterpret_cast<const int4*>(p.track_summary)[h];
        if (sub == 0) reinterpret_cast<int4*>(p.track_summary)[e] = sum;
        const bool cov = (p.setup[e].cbits & PPGPU_EDGE_COVERAGE) != 0;
        int nchunks = (sum.x >> 6) + 1;                                 // (limit = kb: the chunk of the blocked step is the last one read)
        if (nchunks > p.nch) nchunks = p.nch;
        const size_t rowE = (size_t)e * p.nch, rowH = (size_t)h * p.nch;
        for (int c = sub; c < nchunks; c += PP_TF_LANES) {
            p.track_chunk_hits[rowE + c] = p.track_chunk_hits[rowH + c];
            if (p.track_skip) p.track_skip[rowE + c] = p.track_skip[rowH + c];
            if (!cov) p.track_eq[rowE + c] = p.track_eq[rowH + c];
        }
        if (p.n_obst <= 0) continue;
        for (int c = 0; c < nchunks; c++) {
            const bool skipped = p.track_skip && (p.track_skip[rowH + c] & PP_SKIP_ALL) != 0;
            if (skipped || p.track_chunk_hits[rowH + c] == 0u) continue;
            const unsigned long long* src = reinterpret_cast<const unsigned long long*>(p.track_hits + (size_t)h * p.ngp + (size_t)c * PP_WAVE);
            unsigned long long* dst = reinterpret_cast<unsigned long long*>(p.track_hits + (size_t)e * p.ngp + (size_t)c * PP_WAVE);
            dst[sub] = src[sub];
        }
    }
}
