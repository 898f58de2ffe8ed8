// pp_k_cover.h — the coverage state machine of Edge::computeTrueCost (Edge.cpp:153-171): pp_k_approach_events (lane per edge) walks each
// edge's approach to the ribbons, pp_k_cover_sweep (wave per edge) visits the events that change them.  The rest of the function
// (:177-205, "phase C") is pp_k_finish.h's: the approach lane finishes a quiet edge with it, the wave hands its edge to pp_k_cover_finish or
// finishes it in wave form at the end of pp_cover_sweep_edge (its own stop rule, the shared flags and maxDistance).  Included by pp_kernels.h.
#pragma once
// How many steps pass before the next coverage event: the loop of Edge.cpp:153-154 subtracts the increment from toCoverDistance
// once per step while it is above the increment, so after an event that measured D the next one is m + 1 steps on, m = the
// number of subtractions.  m is guessed as ceil(D / inc - 1) and accepted when the remainder is clearly inside (0, inc); within
// 1e-12 of a boundary the subtraction runs literally.
__device__ __forceinline__ int pp_event_stride(double D, double inc_d, double inv_inc_d, int ng) {
    int m = 0;
    if (D > inc_d) {
        const double qd = D * inv_inc_d;                   // a guess good to an ulp or two; m0 is verified below
        if (qd > (double)(ng + 2)) {
            m = ng + 1;                                    // beyond the grid: never again
        } else {
            const int m0 = (int)ceil(qd - 1.0);
            const double r = fma(-(double)m0, inc_d, D);   // D - m0*inc, one rounding
            const double margin = (double)m0 * D * 5e-16 + 1e-12;
            if (m0 >= 1 && r > margin && r < inc_d - margin) {
                m = m0;                                    // the running subtraction cannot differ
            } else {
                double tc = D;                             // too close to call: do it the long way
                while (tc > inc_d && m <= ng) { tc -= inc_d; m++; }
            }
        }
    }
    return m;
}

// The approach to the ribbons, one LANE per edge.  Until the vehicle first comes within reach of a ribbon (inside some
// ribbon's bounding box grown by the ribbon width: the test of pp_ribbons_event's fast path) a coverage event changes nothing
// and only yields the index of the next one, from the distance to the nearest ribbon endpoint.  That chain is sequential per
// edge but independent across edges; walked by the edge's own wavefront it costs a 64-lane window of poses per event to use one
// pose (2.5 of the 3.85 one-at-a-time events per edge at config 3).  Here 64 edges walk their chains side by side — pose by
// pp_lane_pose (the arithmetic of pp_window_pose), boxes and distance per lane with the expressions of pp_ribbons_event, so every number
// is the one the wavefront would have computed — and each hands over {next event, last event visited} where its chain meets a ribbon,
// runs past the sweep's limit or end time, or passes the point from which the curve stays clear of all ribbons (PPEdgeSetup::tfar).
// The cover sweep starts its state machine there instead of at step 0.
//
// Quiet edges.  When the chain ends without meeting a ribbon (past the sweep's limit, or past PPEdgeSetup::tfar) the cover sweep's
// event loop has nothing to do for this edge, and unless the last cover (Edge.cpp:182-191) happens within reach of a ribbon
// the rest of computeTrueCost is scalar work.  The lane does that too (pp_finish_quiet_edge: pp_lane_phase_c from the vertex's own
// state, the function pp_k_cover_finish runs from a wave's) and marks the edge PP_FAR_DONE; the cover sweep's wave then drops it at
// once.  Nearly half the edges of config 3.
// (PP_FAR_DONE itself: pp_k_common.h, pp_k_mark_sweeps stores it too)
#define PP_FAR_SHARED (-3)      // inside pp_k_approach_events only: a shared edge, stored as PP_FAR_DONE
// PPParams::track_far[e].y = (last event before the hand-over) + 1 in the low 20 bits, and, when the approach lane has already split the
// one ribbon the vehicle entered (round 4): PP_FAR_SPLIT, which piece the corridor run that follows moves (6 bits) and which of its ends
#define PP_FAR_LAST_MASK 0xfffff
#define PP_FAR_SPLIT (1 << 30)
#define PP_FAR_MOVE_END (1 << 29)
#define PP_FAR_PIECE_SHIFT 21
// A quiet edge's record goes to its lane's 16 doubles of LDS (stride PP_REC_STRIDE), and the wave then stores the records of its
// lanes together, 4 records of 128 contiguous bytes per store instruction instead of 64 different lines per field.
#define PP_REC_STRIDE 17
// The approach loop's two walks over the lane's ribbon list (pp_with_ribbons picks the address space).  Is some piece short enough to
// be erased (Ribbon::covered(strict)) wherever the vehicle is?
template <class RP>
__device__ __forceinline__ bool pp_any_tiny_ribbon(RP r, int n, double thr) {
    bool tiny = false;
    for (int i = 0; i < n; i++) tiny |= pp_sq_len(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]) < thr;
    return tiny;
}
// One event at (x, y): which grown boxes hold the point (any, how many, the last such ribbon) and q = the squared distance to the
// nearest ribbon endpoint.
struct PPBoxScan { bool inBox; int boxCount, boxIdx; double q; };
template <class RP>
__device__ __forceinline__ PPBoxScan pp_box_scan(RP r, int n, double x, double y, double grow) {
    PPBoxScan s = {false, 0, 0, PP_DBL_MAX};
    for (int i = 0; i < n; i++) {
        const double sx = r[4 * i], sy = r[4 * i + 1], ex = r[4 * i + 2], ey = r[4 * i + 3];
        const bool in = pp_in_grown_box(sx, sy, ex, ey, x, y, grow);
        s.inBox |= in; s.boxCount += in ? 1 : 0; s.boxIdx = in ? i : s.boxIdx;
        const double qS = (sx - x) * (sx - x) + (sy - y) * (sy - y);
        const double qE = (ex - x) * (ex - x) + (ey - y) * (ey - y);
        s.q = fmin(s.q, fmin(qE, qS));
    }
    return s;
}
// Four waves per SIMD (127 VGPRs): with the 34 KB of LDS below, 4 workgroups per CU, 1 024 resident ones — the 923 of a config-3 launch
// run as ONE round.  At 3 (142 VGPRs, what the compiler takes unbounded) 768 fit, and the last 155 ran as a second round on a
// nearly empty machine (profiles/solve_approach_ab.txt: 113 -> 106 us).  The bound costs 8 spilled VGPRs, 36 B of scratch per lane.
#ifndef PP_APPROACH_MIN_WAVES
#define PP_APPROACH_MIN_WAVES 4
#endif
#ifndef PP_APPROACH_THREADS
#define PP_APPROACH_THREADS 256
#endif
#ifndef PP_LANE_NEAR_MAX
#define PP_LANE_NEAR_MAX 8
#endif
// LISTED: lane i takes entry i of the sweep list (launches with a list, unless PPGPU_APPROACH_LIST=0; pp_k_mark_sweeps then gives the edges off the list their
// track_far entry, and the unsolved ones their place on the live list); otherwise edge i of the slice.
template <bool LISTED>
__device__ __forceinline__ void pp_approach_events_body(const PPParams& p) {
    __shared__ double s_rec[PP_APPROACH_THREADS * PP_REC_STRIDE];      // quiet edges' records, transposed through LDS (34 KB: four workgroups per CU still fit)
    const long long e0 = (long long)blockIdx.x * PP_APPROACH_THREADS;
    long long eIdx = e0 + threadIdx.x;
    bool inRange = eIdx < p.n_edges;
    if (LISTED) {
        // (both parts of the list: the prefix the pose sweep walked, then the stop members, which pp_k_track_fanout gave their head's
        // track and put behind the prefix)
        const long long count = (long long)(unsigned)pp_const_i32(&p.words->sweep_count)[0] + (long long)(unsigned)pp_const_i32(&p.words->stop_count)[0];
        if (e0 >= count) return;                                       // (the whole workgroup: no barrier met)
        inRange = eIdx < count;
        eIdx = inRange ? (long long)p.sweep_list[eIdx] : 0;
    }
    const long long e = eIdx;
    const bool valid = inRange;
    const PPEdgeSetupBody* S = p.setup + p.ws_base + (valid ? e : 0);
    int2 out; out.x = 0; out.y = 0;                 // {first event of the wave, (last event before it) + 1 | PP_FAR_* bits}
    int splitInfo = 0;
#ifdef PP_DBG_PHASES               // tools/cover_phases.py: the lane's cycles before / inside / after its event loop, and its events
    const long long apT0 = (long long)__builtin_readcyclecounter();
    long long apT1 = apT0, apT2 = apT0;
    int apEvents = 0;
#endif
    const unsigned sflags = S->sflags;
    const int dubType = S->type;
    // do all lanes of this wave start from the same open vertex?
    const unsigned viMine = S->vi;
    const unsigned viFirst = (unsigned)__builtin_amdgcn_readfirstlane((int)viMine);
    const bool oneVertex = viFirst < (unsigned)p.nverts && __ballot(valid && viMine != viFirst) == 0ull;
    const double* rpU = p.ribbons + 4 * (size_t)pp_const_i32(&p.verts[oneVertex ? viFirst : 0].ribbon_offset)[0];
    const int nribU = pp_const_i32(&p.verts[oneVertex ? viFirst : 0].ribbon_count)[0];
    if (valid && !(sflags & PP_SETUP_NO_SWEEP) && dubType >= 0) {
        const ppgpu_vertex* V = p.verts + S->vi;
        const int nrib = V->ribbon_count;
        const int limit = p.track_summary[p.ws_base + e].limit;
        if (nrib > 0 && nrib <= PP_WAVE && limit > 0) {
            const double* rp = p.ribbons + 4 * (size_t)V->ribbon_offset;
            const double* tg = p.tgrid + (size_t)S->vi * p.ng;
            const PPLaneCurve cv = pp_lane_curve(S);
            const double endTime0 = fmin(p.horizon + 1e-12 + p.sst, S->wEnd);
            const double w = p.ribw, grow = w + 1e-3, minLength0 = 2 * w;
            // (oneVertex: the list comes through scalar loads instead of twenty vector loads per event)
            const PPLaneRibbons ribs = {rp, nrib, rpU, nribU, oneVertex};
            const bool tiny = pp_with_ribbons(ribs, [&](auto r, int n) { return pp_any_tiny_ribbon(r, n, minLength0 * minLength0 / (2.0 * 2.0)); });
            int k = 0, lastEv = -1;
            bool handOver = tiny;               // the wave has events to visit (or an error to flag)
            // Round 3: an event within reach of ONE ribbon is no longer handed over at once.  The lane takes it exactly (does that
            // ribbon contain the point, strictly or not: the reference's own expressions) and goes on while it changes nothing — the
            // vehicle passes near a ribbon, or travels inside a corridor before it reaches the strict one, or may not cover while it
            // turns: what the wave used to start with (one event and one quiet run, two of a slow edge's nine operations).  At most
            // PP_LANE_NEAR_MAX such events per edge (a crawl along a corridor is the wave's, 64 steps at a time); within reach of
            // two ribbons at once the wave takes over as before.
            int nearBudget = PP_LANE_NEAR_MAX;
            const bool covEdge = (S->cbits & PPGPU_EDGE_COVERAGE) != 0;
            // a piece short enough to be erased makes every event a real one (Ribbon::covered is checked wherever the vehicle is)
#ifdef PP_DBG_PHASES
            apT1 = (long long)__builtin_readcyclecounter();
#endif
            while (!tiny) {
                if (k >= limit) break;
                const double t = tg[k];
                if (!(t < endTime0)) break;
#ifdef PP_DBG_PHASES
                apEvents++;
#endif
                double x, y, uth;
                bool perr = false;
                pp_lane_pose(S, cv, t, x, y, uth, perr);
                if (perr) { handOver = true; break; }                                   // the wavefront's code flags the error
                const PPBoxScan scan = pp_with_ribbons(ribs, [&](auto r, int n) { return pp_box_scan(r, n, x, y, grow); });
                const int boxIdx = scan.boxIdx;
#ifdef PP_DBG_TRACE
                if (pp_edge_position(p, p.e_base + e) == (long long)(PP_DBG_TRACE)) printf("[lane] event %d: inBox %d q %.17g x %.17g y %.17g\n", k, (int)scan.inBox, scan.q, x, y);
#endif
                double D = fmin(PP_DBL_MAX, sqrt(scan.q));
                if (scan.inBox) {
                    if (scan.boxCount == 1 && nearBudget-- > 0) {
                        bool inside, strict;
                        double px, py;
                        const double bsx = rp[4 * boxIdx], bsy = rp[4 * boxIdx + 1], bex = rp[4 * boxIdx + 2], bey = rp[4 * boxIdx + 3];
                        pp_lane_ribbon_contains(bsx, bsy, bex, bey, x, y, w, inside, strict, px, py);
                        // Edge.cpp:159: cover() runs when coverage is allowed on this edge or the heading did not change since the last step
                        const bool coverOn = covEdge || (((p.track_eq[(size_t)(p.ws_base + e) * p.nch + (k >> 6)] >> (k & 63)) & 1ull) != 0ull);
                        if (!(strict && coverOn)) {
                            if (inside) D = 0;                                          // RibbonManager::minDistanceFrom: contained
                            lastEv = k;
                            k = k + pp_event_stride(D, p.inc_d, p.inv_inc_d, p.ng) + 1;
                            continue;
                        }
                        // Round 4: the event that SPLITS the one ribbon in reach is the lane's too, when both halves stay (the vehicle
                        // entered the strict corridor somewhere along the ribbon): RibbonManager::cover over the list in order changes
                        // this ribbon only — nothing else is in reach, nothing is short enough to be erased — into [start, projection]
                        // and [projection, end] (Ribbon::split, Ribbon.cpp:9-17; covered(strict), :23-25).  The new list goes into the
                        // edge's child-ribbon slot and the wave starts one step later, inside the corridor run that nearly always
                        // follows (the half the vehicle travels into, by the direction of travel: the run's own checks decide, a wrong
                        // guess costs it one attempt) — and in long-run mode from its first window.  The wave used to spend a window
                        // and its most expensive kind of event here, then a 64-step run before the first long one.
                        const double thr = minLength0 * minLength0 / (2.0 * 2.0);
                        const bool keepF = !(pp_sq_len(bsx, bsy, px, py) < thr), keepR = !(pp_sq_len(px, py, bex, bey) < thr);
                        if (keepF && keepR && p.lane_split && nrib + 1 <= p.stride && nrib + 1 <= PP_WAVE) {
                            double* c = p.child + (size_t)pp_edge_position(p, p.e_base + e) * p.stride * 4;
                            for (int i = 0; i < boxIdx; i++) { c[4 * i] = rp[4 * i]; c[4 * i + 1] = rp[4 * i + 1]; c[4 * i + 2] = rp[4 * i + 2]; c[4 * i + 3] = rp[4 * i + 3]; }
                            c[4 * boxIdx] = bsx; c[4 * boxIdx + 1] = bsy; c[4 * boxIdx + 2] = px; c[4 * boxIdx + 3] = py;
                            c[4 * boxIdx + 4] = px; c[4 * boxIdx + 5] = py; c[4 * boxIdx + 6] = bex; c[4 * boxIdx + 7] = bey;
                            for (int i = boxIdx + 1; i < nrib; i++) { c[4 * i + 4] = rp[4 * i]; c[4 * i + 5] = rp[4 * i + 1]; c[4 * i + 6] = rp[4 * i + 2]; c[4 * i + 7] = rp[4 * i + 3]; }
                            // which half does the vehicle travel into?  The direction of travel is the pose's yaw.
                            double sn, cs;
                            pp_sincos_bounded(uth, &sn, &cs);
                            const bool towardsEnd = (cs * (bex - bsx) + sn * (bey - bsy)) > 0.0;
                            splitInfo = PP_FAR_SPLIT | (towardsEnd ? 0 : PP_FAR_MOVE_END) | ((towardsEnd ? boxIdx + 1 : boxIdx) << PP_FAR_PIECE_SHIFT);
                            lastEv = k;
                            k = k + 1;
                            handOver = true; break;
                        }
                    }
                    handOver = true; break;                                             // a ribbon changes here (or two are in reach, or the budget is spent): the wavefront takes over
                }
                lastEv = k;
                k = k + pp_event_stride(D, p.inc_d, p.inv_inc_d, p.ng) + 1;
            }
            out.x = k; out.y = (lastEv + 1) | splitInfo;
#ifdef PP_DBG_PHASES
            apT2 = (long long)__builtin_readcyclecounter();
#endif
            if (!handOver && k >= limit && p.quiet_finish &&
                pp_finish_quiet_edge(p, S, cv, V, p.ws_base + e, pp_edge_position(p, p.e_base + e), limit, lastEv, ribs, tg, s_rec + (size_t)threadIdx.x * PP_REC_STRIDE))
                out.x = PP_FAR_DONE;
        }
    }
    // An edge that takes another edge's results (pp_k_share_mark) skipped all of the above: it is marked PP_FAR_DONE without a record and
    // never enters the live list.  (Its flags are read again here: a predicate kept since the top costs the loop above four more spilled registers.)
    asm volatile("" ::: "memory");
    if (valid && (S->sflags & PP_SETUP_SHARED) != 0u) out.x = PP_FAR_SHARED;
    if (valid) p.track_far[p.ws_base + e] = make_int2(max(out.x, PP_FAR_DONE), out.y);
#ifdef PP_DBG_PHASES
    {
        const long long apT3 = (long long)__builtin_readcyclecounter();
        const double wPro = pp_wave_max((double)(apT1 - apT0)), wLoop = pp_wave_max((double)(apT2 - apT1)), wFin = pp_wave_max((double)(apT3 - apT2));
        const double wEv = pp_wave_max((double)apEvents);
        if (valid && out.x == PP_FAR_DONE) {
            double* st = s_rec + (size_t)threadIdx.x * PP_REC_STRIDE;
            st[12] = wPro; st[13] = wLoop * 4294967296.0 + (double)(apT2 - apT1); st[14] = -1.0 - wFin; st[15] = wEv * 1e6 + (double)apEvents;
        }
    }
#endif
    {
        // the records of this wave's quiet edges, from LDS: lanes 16g .. 16g+15 store the 16 doubles of record 4 it + g
        const int lane = threadIdx.x & 63, wbase = (int)threadIdx.x - lane;
        const unsigned long long doneMask = __ballot(valid && out.x == PP_FAR_DONE);
        if (doneMask) {
            pp_wave_lds_fence();
            const long long myEg = valid ? pp_edge_position(p, p.e_base + e) : 0;
            const int g = lane >> 4, slot = lane & 15;
            for (int it = 0; it < 16; it++) {
                const int src = 4 * it + g;
                const long long egs = __shfl(myEg, src, PP_WAVE);
                if ((doneMask >> src) & 1ull) reinterpret_cast<double*>(p.out + egs)[slot] = s_rec[(size_t)(wbase + src) * PP_REC_STRIDE + slot];
            }
        }
    }
    // the edges the cover sweep's waves still have to visit, packed (one atomic per workgroup; the order of the launch — long
    // edges first — survives up to the order in which workgroups get here)
    if (p.live_list) {
        __shared__ unsigned s_cnt[PP_APPROACH_THREADS / 64];
        __shared__ unsigned s_base;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const bool live = valid && out.x >= 0;                                             // (neither PP_FAR_DONE nor PP_FAR_SHARED)
        const unsigned long long m = __ballot(live);
        if (lane == 0) s_cnt[wave] = (unsigned)__popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned tot = 0;
            for (int w = 0; w < PP_APPROACH_THREADS / 64; w++) tot += s_cnt[w];
            s_base = tot ? atomicAdd(&p.words->live_count, tot) : 0u;
        }
        __syncthreads();
        if (live) {
            unsigned at = s_base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; w++) at += s_cnt[w];
            p.live_list[2 * at] = (unsigned)e;                                             // slot in the workspace ...
            p.live_list[2 * at + 1] = (unsigned)pp_edge_position(p, p.e_base + e);         // ... and position in the caller's list (a 64-bit division the wave is spared)
        }
    }
}

__global__ __launch_bounds__(PP_APPROACH_THREADS, PP_APPROACH_MIN_WAVES) void pp_k_approach_events(PPParams p) { pp_approach_events_body<true>(p); }
__global__ __launch_bounds__(PP_APPROACH_THREADS, PP_APPROACH_MIN_WAVES) void pp_k_approach_events_direct(PPParams p) { pp_approach_events_body<false>(p); }

// e = the edge's slot in the workspace, eg = its position in the caller's edge list, lds = 256 doubles private to the wave
#ifndef PP_FUSE_HEUR
#define PP_FUSE_HEUR 1
#endif
template <bool GAUSSIAN>
__device__ __forceinline__ void pp_cover_sweep_edge(const PPParams& p, const long long e, const long long eg, double* lds) {
    const int lane = pp_lane();

    if (p.track_far && pp_const_i32(&p.track_far[e].x)[0] == PP_FAR_DONE) return;   // a quiet edge: pp_k_approach_events finished it
    // ---- phase 0 was done by pp_k_solve_edges: everything here is wave-uniform and arrives through scalar loads
    const PPEdgeSetup* S = p.setup + e;
    unsigned flags = 0;
    ppgpu_edge_result* rec = p.out + eg;
    const unsigned sflags = (unsigned)PP_SI32(sflags);
#if !defined(PP_DBG_COUNTS)
    const bool laneFinish = !GAUSSIAN && p.cover_state != nullptr;
#else
    const bool laneFinish = false;
#endif
    if (laneFinish && lane == 0) p.cover_state[e].nrib = -1;          // until the hand-over below says otherwise: finished here
    if (sflags & PP_SETUP_MALFORMED) {
        // malformed descriptor: fail loudly in the record, touch nothing else
        if (lane == 0) { rec->flags = PPGPU_F_INFEASIBLE | PPGPU_F_THROWS | PPGPU_F_DUBINS_ERR; rec->info = 0; }
        return;
    }
    const unsigned vi = (unsigned)PP_SI32(vi), cbits = (unsigned)PP_SI32(cbits);
    const ppgpu_vertex* V = p.verts + vi;
    const double srcX = pp_sgpr(V->x), srcY = pp_sgpr(V->y), srcT = pp_sgpr(V->time), srcG = pp_sgpr(V->g);
    double cct = pp_sgpr(V->coverage_completed_time);
    int nrib = __builtin_amdgcn_readfirstlane(V->ribbon_count);
    const bool cov = (cbits & PPGPU_EDGE_COVERAGE) != 0;

    // this vertex's ribbons, one per lane (Vertex::connect copies the parent's RibbonManager, Vertex.cpp:24)
    PPRibbon rib = {0, 0, 0, 0};
    if (nrib > PP_WAVE) { nrib = PP_WAVE; flags |= PPGPU_F_RIBBON_OVF | PPGPU_F_RIBBON_LOST; }
    if (lane < nrib) {
        const double* rp = p.ribbons + 4 * ((size_t)V->ribbon_offset + lane);
        rib.sx = rp[0]; rib.sy = rp[1]; rib.ex = rp[2]; rib.ey = rp[3];
    }
    const bool startedDone = (nrib == 0);                             // Edge.cpp:93

    const int dubType = PP_SI32(type);
    const double wEnd = PP_SF64(wEnd), wStart = PP_SF64(wStart), speed = PP_SF64(speed);
    const double endTime0 = fmin(p.horizon + 1e-12 + p.sst, wEnd);    // Edge.cpp:90
    double endTime = endTime0;
    bool infeasible = (srcT >= endTime);                              // :102-110
    bool throwsRef = ((sflags & PP_SETUP_COLOCATED) != 0) || (dubType < 0);
    if (dubType < 0) flags |= PPGPU_F_DUBINS_ERR;

    // ---- the pose sweep's track of this edge
    const PPTrackSummary* sum = p.track_summary + e;
    const int limit = pp_const_i32(&sum->limit)[0];
    const int stopKind = pp_const_i32(&sum->blocked)[0];
    const bool blockedAtLimit = stopKind == 1;
    if (pp_const_i32(&sum->dub_err)[0]) flags |= PPGPU_F_DUBINS_ERR;
    const unsigned long long* teq = p.track_eq + (size_t)e * p.nch;
    const double* tg = p.tgrid + (size_t)vi * p.ng;

#ifdef PP_DBG_COUNTS
    int dbgWindows = 0, dbgCorr = 0, dbgQuiet = 0, dbgGeneric = 0, dbgCorrLen = 0, dbgQuietLen = 0, dbgFar = 0, dbgNoChange = 0, dbgInPlace = 0, dbgRestFar = 0;
#define PP_CNT(x) x
#else
#define PP_CNT(x)
#endif
#ifdef PP_DBG_PHASES               // (with PP_DBG_COUNTS) shader cycles per part of the event loop instead of the counts, tools/cover_phases.py
    long long phWin = 0, phCont = 0, phGen = 0, phRun = 0, phLoop = 0, phT = 0;
#define PP_PH_START() (phT = (long long)__builtin_readcyclecounter())
#define PP_PH_END(acc) (acc += (long long)__builtin_readcyclecounter() - phT)
#else
#define PP_PH_START()
#define PP_PH_END(acc)
#endif
#ifdef PP_DBG_TRACE
#define PP_TRACE(...) do { if (eg == (long long)(PP_DBG_TRACE) && lane == 0) printf(__VA_ARGS__); } while (0)
#else
#define PP_TRACE(...)
#endif
    int rdt = -1;                       // `auto ribbonsDoneTime = -1;` is an int (Edge.cpp:92)
    int nextEvent = 0;                  // toCoverDistance starts at 0: step 0 is an event
    int lastEv = -1;
    int handCont = 0, handPiece = 0, handCount = 0;   // (handCount: entries of the child slot the lane's split list occupies)
    bool handMoveEnd = false;
    if (p.track_far) {                  // the approach was walked by pp_k_approach_events: start where it handed over
        nextEvent = pp_const_i32(&p.track_far[e].x)[0];
        const int fy = pp_const_i32(&p.track_far[e].y)[0];
        lastEv = (fy & PP_FAR_LAST_MASK) - 1;
        if (fy & PP_FAR_SPLIT) {
            // the lane split the ribbon the vehicle entered: the list as it stands is in the edge's child slot, and the wave begins inside
            // the corridor run (long-run mode allowed at once)
            nrib = nrib + 1;
            rib = PPRibbon{0, 0, 0, 0};
            if (lane < nrib) {
                const double* rp = p.child + ((size_t)eg * p.stride + lane) * 4;
                rib.sx = rp[0]; rib.sy = rp[1]; rib.ex = rp[2]; rib.ey = rp[3];
            }
            handCont = 1 | 4; handPiece = (fy >> PP_FAR_PIECE_SHIFT) & 0x3f; handMoveEnd = (fy & PP_FAR_MOVE_END) != 0;
            handCount = nrib;
        }
    }
    const double w = p.ribw;
    const double inc_d = p.inc_d;
    const double runSpan = 64.0 * (p.inc_d / p.max_speed) * speed * (1.0 + 1e-9) + 1e-6;   // how far 64 steps can take the vehicle

    // long runs (pp_corridor_run / pp_quiet_run with ell > 0): one sample every longStride steps — as many steps as make
    // PP_LONG_REACH of travel (a slow edge of config 3: 5 steps of 1 cm; at full speed a step is 5 cm and nothing changes; measured 0.02 .. 0.4 m: the wider the margins, the more attempts fail) — with margins of that travel
#ifndef PP_LONG_REACH
#define PP_LONG_REACH 0.05
#endif
#ifndef PP_LONG_MAX_STRIDE
#define PP_LONG_MAX_STRIDE 16
#endif
#define PP_STEP_LEN() ((p.inc_d / p.max_speed) * speed * (1.0 + 1e-9) + 1e-9)      /* arc length of one step, from above */
    int longStride = 1;
    {
        const double stepLen = PP_STEP_LEN();
        const double sd = PP_LONG_REACH / stepLen;
        longStride = sd >= (double)PP_LONG_MAX_STRIDE ? PP_LONG_MAX_STRIDE : (sd > 1.0 ? (int)sd : 1);
        // the half that vanishes between two samples must be shorter than the minimum length; the curve must not turn much between them
        if (!((double)longStride * stepLen + 1e-6 < 0.5 * w) || !(((double)longStride * stepLen + 1e-6) / PP_SF64(rho) < 0.5)) longStride = 1;
    }

    // ---- phase B: coverage events among steps [0, limit)
    if (!throwsRef) {
#ifdef PP_DBG_PHASES
        const long long phLoop0 = (long long)__builtin_readcyclecounter();
#endif
        bool ended = false;
        int cont = handCont, contPiece = handPiece;   // 1 / 2: the last window ended inside a corridor / quiet run (of piece contPiece); + 4: it was
                                            // one run from end to end (a long run is worth trying)
        bool contMoveEnd = handMoveEnd;
        while (!ended) {
            if (nextEvent >= limit) break;
            // a window of 64 steps of the track starting AT the next event, one step per lane (stretches without events are
            // never loaded)
            const int base = nextEvent;
            // ... or, after a window that was one run from end to end, 64 SAMPLES longStride steps apart (a long run)
            const int stride = ((cont & 4) != 0 && longStride > 1 && base + 2 * longStride < limit) ? longStride : 1;
            PP_TRACE("[wave] window at %d stride %d (limit %d, lastEv %d, nrib %d)\n", base, stride, limit, lastEv, nrib);
            PP_CNT(dbgWindows++);
            PP_PH_START();
            const int k = base + lane * stride;
            const double t = (k < p.ng) ? tg[k] : INFINITY;
            // the poses of the window, recomputed with the pose sweep's own arithmetic (pp_window_pose)
            double2 q;
            {
                PP_WINDOW_POSE(S, t, pp_readlane(t, 0), k < limit, q.x, q.y);
                if (k >= limit) { q.x = 0.0; q.y = 0.0; }
            }
            // Edge.cpp:159: cover only when coverage is allowed on this edge or the heading did not change since the last step
            unsigned long long coverMask = ~0ull, coverAny = ~0ull;
            if (!cov) {
                if (stride == 1) {
                    const int c0 = base >> 6, sh = base & 63;
                    const unsigned long long lo = pp_const_u64(teq + c0)[0];
                    const unsigned long long hi = (sh != 0 && c0 + 1 < p.nch) ? pp_const_u64(teq + c0 + 1)[0] : 0ull;
                    coverMask = sh ? ((lo >> sh) | (hi << (64 - sh))) : lo;
                    coverAny = coverMask;
                } else {
                    // a sample vouches for the steps (previous sample, itself]: cover() enabled at all of them / at any of them
                    const int lo = (lane == 0) ? base : (k - stride + 1);
                    const int cnt = (lane == 0) ? 1 : stride;
                    unsigned long long bits = 0ull;
                    if (k < limit) {
                        const int w0 = lo >> 6, sh = lo & 63;
                        bits = teq[w0] >> sh;
                        if (sh + cnt > 64 && w0 + 1 < p.nch) bits |= teq[w0 + 1] << (64 - sh);
                    }
                    const unsigned long long mask = (1ull << cnt) - 1ull;
                    bits &= mask;
                    coverMask = __ballot(bits == mask);
                    coverAny = __ballot(bits != 0ull);
                }
            }
            const int climit = (stride == 1) ? ((limit - base) < PP_WAVE ? (limit - base) : PP_WAVE) : __popcll(__ballot(k < limit));
            bool runFailed = false, quietFailed = false;
            bool tryQuiet = false;              // a corridor run has just ended inside this window
            PP_PH_END(phWin);
            while (true) {
                const int j = nextEvent - base;
                if (j >= climit) break;
                const double tj = pp_readlane(t, j);
                if (!(tj < endTime)) { ended = true; break; }         // `while (intermediate.time() < endTime)`
                if (j == 0 && (cont & 3) != 0) {
                    // the previous window ended inside a run: this step is an event of the same kind, very likely the whole
                    // window is.  The run's own guarded checks decide; if its first step does not pass, the step goes
                    // through the one-at-a-time code below like any other.
                    int L = 0;
                    double nsx = 0, nsy = 0;
                    const bool stepOk = (lane < climit) & (t < endTime);
                    const int kind = cont & 3;
                    PP_CNT(if (kind == 1) dbgCorr++; else dbgQuiet++);
                    // a long run: margins of the travel between two samples
                    PP_PH_START();
                    const double ell = (stride > 1) ? ((double)stride * PP_STEP_LEN() + 1e-6) : 0.0;
                    const double span = (stride > 1) ? 64.0 * ell : runSpan;
                    if (kind == 1) L = pp_corridor_run(rib, nrib, w, contPiece, contMoveEnd, q.x, q.y, stepOk, coverMask, 0, span, nsx, nsy, ell, ell / PP_SF64(rho));
                    else L = pp_quiet_run(rib, nrib, w, q.x, q.y, stepOk, coverAny, 0, span, ell, ell / PP_SF64(rho));
                    PP_TRACE("[wave]   continued run (kind %d, stride %d) from %d: L %d\n", kind, stride, base, L);
                    PP_PH_END(phCont);
                    if (L > 0) {
                        if (kind == 1 && lane == contPiece) {
                            if (contMoveEnd) { rib.ex = nsx; rib.ey = nsy; } else { rib.sx = nsx; rib.sy = nsy; }
                        }
                        PP_CNT(if (kind == 1) dbgCorrLen += (L - 1) * stride + 1; else dbgQuietLen += (L - 1) * stride + 1);
                        lastEv = base + (L - 1) * stride;
                        nextEvent = lastEv + 1;
                    }
                    if (stride > 1) {
                        // a window of samples is only ever this one attempt: whatever it absorbed, ordinary windows (or, if every
                        // sample held, another long run) go on from there
                        cont = kind | ((L == PP_WAVE) ? 4 : 0);
                        break;
                    }
                    if (L > 0) {
                        cont = (L < climit) ? 0 : (kind | 4);  // ended inside the window: something else happens next / filled it: a long run next
                        tryQuiet = (kind == 1) && (L < climit);
                        continue;
                    }
                    cont = 0;
                }
                const double xj = pp_readlane(q.x, j), yj = pp_readlane(q.y, j);
                double D;                                             // Edge.cpp:158-161
                int adv;
                PP_CNT(dbgGeneric++);
                PP_PH_START();
                nrib = pp_ribbons_event(rib, nrib, w, xj, yj, ((coverMask >> j) & 1ull) != 0ull, lds, D, adv);
                PP_PH_END(phGen);
                PP_CNT(if (adv == -3) dbgFar++; else if (adv == -2) dbgNoChange++; else if (adv >= 0) dbgInPlace++);
                PP_TRACE("[wave]   event %d: adv %d D %.17g nrib %d cover %d x %.17g y %.17g\n", base + j, adv, D, nrib, (int)((coverMask >> j) & 1ull), xj, yj);
                if (nrib > PP_WAVE) { nrib = PP_WAVE; flags |= PPGPU_F_RIBBON_OVF | PPGPU_F_RIBBON_LOST; }

                bool guessed = false;
                if (adv <= -4 && j + 1 < climit && !runFailed && nrib <= PP_WAVE) {
                    // this event split one piece in two (the vehicle has just entered its strict corridor): the next step will move the
                    // inner endpoint of the half the vehicle travels into — guess which from the direction of travel and try the run
                    // at once instead of learning it from one more one-at-a-time event (the run's own checks decide: a wrong guess
                    // gives L = 0 and costs one attempt)
                    const int front = -4 - adv;
                    const double dxp = pp_readlane(rib.ex, front + 1) - pp_readlane(rib.sx, front), dyp = pp_readlane(rib.ey, front + 1) - pp_readlane(rib.sy, front);
                    const bool towardsEnd = ((pp_readlane(q.x, j + 1) - xj) * dxp + (pp_readlane(q.y, j + 1) - yj) * dyp) > 0.0;
                    adv = towardsEnd ? (front + 1) : (front | 0x100);
                    guessed = true;
                }
                if (adv >= 0 && j + 1 < climit && !runFailed) {
                    // this event only moved one piece's endpoint: the following steps very likely do the same
                    double nsx, nsy;
                    const bool moveEnd = (adv & 0x100) != 0;
                    const int piece = adv & 0xff;
                    PP_PH_START();
                    const int L = pp_corridor_run(rib, nrib, w, piece, moveEnd, q.x, q.y, (lane < climit) & (t < endTime), coverMask, j + 1, runSpan, nsx, nsy);
                    PP_PH_END(phRun);
                    PP_CNT(dbgCorr++; dbgCorrLen += L);
                    runFailed = (L == 0) && !guessed;      // do not keep paying for attempts that do not start
                    PP_TRACE("[wave]   corridor run from %d: L %d\n", base + j + 1, L);
                    if (L > 0) {
                        if (lane == piece) {
                            if (moveEnd) { rib.ex = nsx; rib.ey = nsy; } else { rib.sx = nsx; rib.sy = nsy; }
                        }
                        lastEv = base + j + L;
                        nextEvent = base + j + L + 1;      // inside the corridor minDistanceFrom is 0: the next step is an event too
                        if (j + L + 1 >= climit) { cont = 1 | 4; contPiece = piece; contMoveEnd = moveEnd; }   // cut by the window, not by a guard
                        else tryQuiet = true;
                        continue;
                    }
                }
                else if (adv == -2 && D == 0 && nrib > 0 && j + 1 < climit && !quietFailed) {
                    // inside a corridor, nothing changed: the following steps are very likely the same kind of event
                    PP_PH_START();
                    const int L = pp_quiet_run(rib, nrib, w, q.x, q.y, (lane < climit) & (t < endTime), coverMask, j + 1, runSpan);
                    PP_PH_END(phRun);
                    PP_CNT(dbgQuiet++; dbgQuietLen += L);
                    PP_TRACE("[wave]   quiet run from %d: L %d\n", base + j + 1, L);
                    quietFailed = (L == 0);
                    if (L > 0) {
                        lastEv = base + j + L;
                        nextEvent = base + j + L + 1;
                        if (j + L + 1 >= climit) cont = 2 | 4;
                        continue;
                    }
                }
                if (nrib == 0) {                                      // :162-170
                    if (cct == -1) cct = tj;
                    rdt = (int)tj;
                    endTime = fmin(endTime, cct + p.tmin);
                }
                lastEv = base + j;
                // steps until toCoverDistance <= increment again (:153-154): m subtractions
                const int m = pp_event_stride(D, inc_d, p.inv_inc_d, p.ng);
                nextEvent = base + j + m + 1;
            }
        }
#ifdef PP_DBG_PHASES
        phLoop = (long long)__builtin_readcyclecounter() - phLoop0;
#endif
    }

    // ---- the rest is scalar work per edge: pp_k_cover_finish does it with one lane per edge, from what this wave knows now
    if (laneFinish && !throwsRef && (wStart <= endTime && wEnd >= endTime) && nrib <= PP_FINISH_MAX && nrib <= p.stride) {
        if (lane == 0) {
            PPCoverState* st = p.cover_state + e;
            st->cct = cct; st->endTime = endTime; st->lastEv = lastEv; st->rdt = rdt; st->flags = flags | (infeasible ? PPGPU_F_INFEASIBLE : 0u);
            st->nrib = nrib;                                          // (same lane, program order: after the -1 above)
        }
        if (lane < nrib || lane < handCount) {        // (entries of the lane's split list beyond what is left of it: back to zero)
            double* c = p.child + ((size_t)eg * p.stride + lane) * 4;
            c[0] = rib.sx; c[1] = rib.sy; c[2] = rib.ex; c[3] = rib.ey;
        }
        return;
    }
    // ---- where the loop of Edge.cpp:143-175 stopped: pp_loop_stop's rule (pp_k_finish.h), wave form — through wave-uniform scalar loads
    int steps = 0;
    double ix = srcX, iy = srcY;        // `intermediate` position
    double tfinal = (p.ng > 0) ? pp_const_f64(tg)[0] : INFINITY;
    bool coverFinal = true;             // `lastHeading == intermediate.heading()` unless the loop broke at a blocked step
    int hexec = 0;                      // steps whose obstacle hits count
    int lastIdx = -1;                   // the step whose pose `intermediate` holds when the loop stops (-1: the source pose)
    if (!throwsRef) {
        // cnt = steps k < limit with t_k < endTime (the time grid is non-decreasing)
        int cnt = limit;
        if (endTime != endTime0) {
            int lo = 0, hi = limit;
            while (hi > lo) {
                const int span = hi - lo, stride = (span + 63) >> 6;
                const int k = lo + lane * stride;
                const bool lt = (k < hi) && (tg[k] < endTime);
                const int c = __popcll(__ballot(lt));
                if (c == 0) { hi = lo; break; }
                const int nlo = lo + (c - 1) * stride + 1;
                const int nhi = lo + c * stride;
                hi = nhi < hi ? nhi : hi;
                lo = nlo;
            }
            cnt = lo;
        }
        int nexec = cnt > lastEv + 1 ? cnt : lastEv + 1;
        nexec = nexec < limit ? nexec : limit;
        if (blockedAtLimit && nexec == limit && pp_const_f64(tg + limit)[0] < endTime) {   // `break` at :146
            infeasible = true;
            lastIdx = limit;
            coverFinal = cov || (((pp_const_u64(teq + (limit >> 6))[0] >> (limit & 63)) & 1ull) != 0ull);
            tfinal = pp_const_f64(tg + limit)[0];
            steps = limit + 1;
            hexec = limit;
        } else {                                            // loop condition failed, or the first sample threw
            if (stopKind == 2 && pp_const_f64(tg)[0] < endTime) infeasible = true;   // `intermediate` still holds the source pose
            lastIdx = nexec - 1;
            tfinal = (nexec < p.ng) ? pp_const_f64(tg + nexec)[0] : INFINITY;
            steps = nexec;
            hexec = nexec;
        }
    }

    // ---- phase C
    // end()->state().time() = endTime; wrapper.sample(end state)  (Edge.cpp:177-178)
    if (!throwsRef && !(wStart <= endTime && wEnd >= endTime)) throwsRef = true;  // DubinsWrapper::containsTime
    double endX = 0, endY = 0, endHeading = 0;
    int hitsTotal = 0;
    if (!throwsRef) {
        // two samples of the curve in one pass: lane 1 takes the end state's time, every other lane the time of the step
        // `intermediate` stopped on (its position is needed for the last cover below)
        {
            const double tl = (lastIdx >= 0) ? pp_const_f64(tg + lastIdx)[0] : endTime;
            const PPEdgeSetup* S2 = S;
            asm volatile("" : "+s"(S2));
            const PPCurveHot hot = pp_curve_hot(S2);
            int cur = -1;
            PPSeg cs = PPSeg{0, 0, 0, 0, 0, INFINITY, -INFINITY, 0, 0, 1};
            double px, py, puth;
            bool perr = false;
            pp_window_pose<PP_COVER_SINCOS_TAB>(S2, hot, cur, cs, lane == 1 ? endTime : tl, tl, true, px, py, puth, perr);
            if (lastIdx >= 0) { ix = pp_readlane(px, 0); iy = pp_readlane(py, 0); }
            endX = pp_readlane(px, 1);
            endY = pp_readlane(py, 1);
            endHeading = pp_heading_from_yaw(pp_mod2pi(pp_readlane(puth, 1)));
            if ((__ballot(perr) >> 1) & 1ull) flags |= PPGPU_F_DUBINS_ERR;
        }
        // cover the last little bit (:182-191)
        if (cov || coverFinal) {
            double Dunused;
            int advUnused;
            nrib = pp_ribbons_event(rib, nrib, w, ix, iy, true, lds, Dunused, advUnused);
            if (nrib > PP_WAVE) { nrib = PP_WAVE; flags |= PPGPU_F_RIBBON_OVF | PPGPU_F_RIBBON_LOST; }
        }
        if (nrib == 0) {
            if (cct == -1) cct = tfinal;
            rdt = (int)tfinal;
        }
        // obstacle hits of the executed steps (:150-151 summed): whole chunks from the pose sweep's per-chunk sums, the
        // last partial chunk step by step
        const unsigned* tch = p.track_chunk_hits + (size_t)e * p.nch;
        const unsigned short* thits = p.track_hits + (size_t)e * p.ngp;
        const int cfull = hexec >> 6;
        int acc = 0;
        if (p.n_obst > 0) {
            for (int c = lane; c < cfull; c += PP_WAVE) acc += (int)tch[c];
            if ((hexec & 63) != 0 && tch[cfull] != 0u && (cfull << 6) + lane < hexec) {
                // a chunk the pose sweep skipped has no per-step counts: all of its 64 steps are inside the same boxes
                const bool skipped = p.track_skip && (p.track_skip[(size_t)e * p.nch + cfull] & PP_SKIP_ALL) != 0;
                acc += skipped ? (int)(tch[cfull] >> 6) : (int)thits[(cfull << 6) + lane];
            }
            hitsTotal = pp_wave_sum_i(acc);
        }
    }
    double penalty = (double)hitsTotal * p.cpf;                                   // :150-151 summed
    if (GAUSSIAN && !throwsRef && p.n_obst > 0) {
        // Gaussian model: the per-step values are doubles; whole chunks from the pose sweep's sums, the rest step by step
        const double* cpn = p.track_chunk_pen + (size_t)e * p.nch;
        const int cfull = hexec >> 6;
        double acc = 0;
        for (int c = lane; c < cfull; c += PP_WAVE) acc += cpn[c];
        if ((hexec & 63) != 0 && cpn[cfull] != 0.0 && (cfull << 6) + lane < hexec) acc += p.track_pen[(size_t)e * p.ngp + (cfull << 6) + lane] * p.cpf;
        penalty = pp_wave_sum_d(acc);
    }
    const double netTime = endTime - srcT;                                        // Edge::netTime
    double tc = fmax(netTime - ((nrib == 0) ? (endTime - (double)rdt) : 0), 0);  // :197
    if (startedDone) tc = 0;                                                      // :198
    const double trueCost = tc * p.tpf + penalty;                                 // :199
    const double g = srcG + trueCost;                                             // Vertex::setCurrentCost

    // h and f are filled in after the record is stored: by this wave from the ribbons it still holds (PP_FUSE_HEUR, below), or
    // by pp_k_heuristic* from the child ribbons
    const double h = 0;

    if (infeasible) flags |= PPGPU_F_INFEASIBLE;
    if (throwsRef) flags |= PPGPU_F_THROWS | PPGPU_F_INFEASIBLE;
    if (!throwsRef) flags |= pp_done_goal_flags(p, nrib, endTime, cct);

    // ---- one 128-byte record, lanes 0..15 write one 8-byte slot each
    {
        const unsigned info = (unsigned)((dubType < 0 ? 0 : dubType) & 0xff) | ((unsigned)(nrib & 0xff) << 8) |
                              ((unsigned)(steps & 0xffff) << 16);
        double v;
        switch (lane) {
            case 0: v = __hiloint2double((int)info, (int)flags); break;   // {flags (low), info (high)}
            case 1: v = trueCost; break;
            case 2: v = penalty; break;
            case 3: v = PP_SF64(approx); break;
            case 4: v = endX; break;
            case 5: v = endY; break;
            case 6: v = endHeading; break;
            case 7: v = speed; break;
            case 8: v = endTime; break;
            case 9: v = g; break;
            case 10: v = h; break;
            case 11: v = g + h; break;
#if defined(PP_DBG_PHASES)
            case 12: v = (double)phLoop; break;
            case 13: v = (double)phWin * 4294967296.0 + (double)phGen; break;
            case 14: v = (double)phCont; break;
            default: v = (double)phRun; break;
#elif defined(PP_DBG_COUNTS)
            case 12: v = (double)dbgRestFar * 1e9 + (double)dbgFar * 1e6 + (double)dbgNoChange * 1e3 + (double)dbgInPlace; break;
            case 13: v = (double)dbgWindows * 1e6 + (double)dbgGeneric; break;
            case 14: v = (double)dbgCorr * 1e6 + (double)dbgCorrLen; break;
            default: v = (double)dbgQuiet * 1e6 + (double)dbgQuietLen; break;
#else
            case 12: v = cct; break;
            case 13: v = PP_SF64(p0); break;
            case 14: v = PP_SF64(p1); break;
            default: v = PP_SF64(p2); break;
#endif
        }
        if (throwsRef && lane != 0) v = 0;
        if (lane < 16) reinterpret_cast<double*>(rec)[lane] = v;
    }
    if (!throwsRef) {
        if (nrib > PP_TSP_MAX && lane == 0) atomicOr(&p.words->need_big, 1u);
        if (nrib > p.stride && lane == 0) rec->flags = flags | PPGPU_F_RIBBON_OVF;   // after the record store above
        if ((lane < nrib || lane < handCount) && lane < p.stride) {     // (lanes beyond nrib hold zeros: what is left of the lane's split list goes)
            double* c = p.child + ((size_t)eg * p.stride + lane) * 4;
            c[0] = rib.sx; c[1] = rib.sy; c[2] = rib.ex; c[3] = rib.ey;
        }
    }
#if PP_FUSE_HEUR
    // The edge's heuristic, by this wave, from the ribbons in its registers (lane i holds ribbon i).  The Gaussian sweep never fuses (cost_modes)
    // and its LDS row has no room for the tables.  The ONE site that states pp_h_route's conditions in its own words: taken from the function (nrib is
    // a vector value here, and so is its answer) the cover stage took 0.680 -> 0.715 ms, in these words 0.674 -> 0.668 (profiles/heuristic_routes.txt).
    // test_every_route_boundary_against_the_oracle holds the two statements together: the same lists through this wave and through those that ask.
    if constexpr (!GAUSSIAN) {
        const bool deferred = p.defer_h && !throwsRef && nrib <= p.stride && pp_lane_tsp_ok(p.heuristic, p.tsp_k, nrib);
        if (deferred && lane == 0) rec->h = PP_H_DEFERRED;
        if (p.fuse_h && !deferred && !throwsRef && nrib > 0 && nrib <= p.stride) {
            const bool tsp = p.heuristic != PPGPU_H_MAX_DISTANCE;
            bool leaveToBigPass = false;
            const unsigned flags0 = flags;
            double hdist = 0;
            if (tsp && nrib > PP_TSP_MAX) {
                if (pp_tsp_big_ok(p.heuristic, p.tsp_k, nrib)) leaveToBigPass = true;    // pp_k_heuristic_big fills it in
                else flags |= PPGPU_F_RIBBON_OVF;
            } else if (!tsp && nrib > 31) {
                hdist = pp_max_distance(nrib, p.ribw, endX, endY, [&](int i, double& sx, double& sy, double& ex, double& ey) {
                    sx = pp_readlane(rib.sx, i); sy = pp_readlane(rib.sy, i); ex = pp_readlane(rib.ex, i); ey = pp_readlane(rib.ey, i); });
            } else {
                pp_wave_lds_fence();                                   // the event machinery is done with this scratch
                pp_h_stage_points(lds, endX, endY, nrib, [&](int, double& sx, double& sy, double& ex, double& ey) { sx = rib.sx; sy = rib.sy; ex = rib.ex; ey = rib.ey; });
                hdist = tsp ? pp_h_point_from_pts<PP_TSP_MAX>(p.heuristic, p.tsp_k, p.ribw, lds, nrib, 0u, 1u) : pp_h_max_distance(lds, nrib, p.ribw);
                pp_wave_lds_fence();
            }
            if (!leaveToBigPass && lane == 0) { pp_h_store(rec, g, hdist, p.max_speed, p.tpf); if (flags != flags0) rec->flags = flags; }
        }
    }
#endif
}

// The wave that finished an edge's cover sweep goes straight on to the edge's heuristic (point heuristics, binary-obstacle
// sweep; the Dubins heuristics and the 12-ribbon pass keep their own kernels): the child ribbons and the record it needs were
// just written by the same wave, there is no second launch, and the two phases' stalls fall at different times in the four
// waves of a SIMD.  Cover sweep + heuristic 2.26 -> 2.18 ms (against -DPP_FUSE_HEUR=0).
#define PP_COVER_LDS ((PP_FUSE_HEUR) ? (PPTsp<PP_TSP_MAX>::LDS > PP_WAVE * 4 ? PPTsp<PP_TSP_MAX>::LDS : PP_WAVE * 4) : PP_WAVE * 4)
// lds_all = the workgroup's scratch, [PP_WPB][LDS] doubles: a row per wave
template <bool GAUSSIAN, int LDS>
__device__ __forceinline__ void pp_cover_sweep_waves(PPParams p, double (*lds_all)[LDS]) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    PPQueue qs = pp_queue_init();
    const long long n = p.live_list ? (long long)(unsigned)pp_const_i32(&p.words->live_count)[0] : p.n_edges;
    for (long long i = pp_next_edge(p, qs, n); i < n; i = pp_next_edge(p, qs, n)) {
        const long long idx = p.live_list ? (long long)(unsigned)pp_const_i32(p.live_list + 2 * i)[0] : i;
        const long long eg = p.live_list ? (long long)(unsigned)pp_const_i32(p.live_list + 2 * i)[1] : pp_edge_position(p, p.e_base + idx);
        pp_cover_sweep_edge<GAUSSIAN>(p, p.ws_base + idx, eg, lds_all[wave]);
    }
}
__global__ __launch_bounds__(PP_WPB * 64, PP_MIN_WAVES) void pp_k_cover_sweep(PPParams p) {
    __shared__ double lds_all[PP_WPB][PP_COVER_LDS];
    pp_cover_sweep_waves<false>(p, lds_all);
}
__global__ __launch_bounds__(PP_WPB * 64, PP_MIN_WAVES) void pp_k_cover_sweep_gaussian(PPParams p) {
    __shared__ double lds_all[PP_WPB][PP_WAVE * 4];
    pp_cover_sweep_waves<true>(p, lds_all);
}
