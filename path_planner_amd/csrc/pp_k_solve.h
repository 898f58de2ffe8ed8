// pp_k_solve.h — phase 0 of an edge: pp_k_solve_edges (Vertex::connect + Edge::computeApproxCost, one lane per edge; one lane per
// curve where a dense launch asks for both speeds of a radius).  Included by pp_kernels.h.
#pragma once
#ifndef PP_CR_SOLVE
#define PP_CR_SOLVE true     // the edges' curves with correctly rounded atan2 / acos / sin / cos (pp_cr.h)
#endif
#ifndef PP_SOLVE_MIN_WAVES
#define PP_SOLVE_MIN_WAVES 1
#endif
// ------------------------------------------------------------------------------------------
// Shared sweeps.  An edge is swept up to endTime = min(horizon + 1e-12 + sst, wEnd), and every Dubins word begins with an arc.  Where
// the horizon ends while the vehicle is still on that arc, nothing a sweep computes depends on the target: every pose is sampled on
// segment 0, whose base is the vertex's pose, with the constants wStart (the vertex's time), speed, rho and the arc's direction.  All
// such edges of one (vertex, configuration, direction) — a class — have the same track, events, child ribbons, end state, g, h and
// flags, bit for bit; only the type byte, approx_cost and param[] of the record are the edge's own.  So one member of each class, its
// head, is swept, and pp_k_share_fanout hands its results to the others.
//
// The rule (pp_edge_shareable), on the record as the sweeps will read it, with bound = horizon + 1e-12 + sst:
//   * the edge is solved (type >= 0, neither malformed nor co-located);
//   * !(wEnd < bound): endTime is `bound` for every member;
//   * the pose at `bound`, in pp_window_pose's own arithmetic, lies strictly inside segment 0: dist = (bound - wStart) * speed has
//     dist <= length, and tprime = dist * rho_inv (or dist / rho where rho_inv is 0) has tprime < p0.
// Why the one test at `bound` covers every step: each time t a kernel samples (a step of the time row before endTime, endTime itself,
// an end time an event shortened) is <= bound, and t -> (t - wStart) * speed -> tprime is a chain of roundings of non-decreasing
// functions (a subtraction of and products with non-negative constants), so it is non-decreasing in t as computed: dist(t) <=
// dist(bound) <= length, the retry and the clamp of DubinsWrapper::sample can only fire for dist < 0, where they do not look at
// the curve, and tprime(t) <= tprime(bound) < p0 picks segment 0 (pp_seg_of, and the interval (-inf, p0) of pp_seg_load_uniform).
__device__ __forceinline__ bool pp_edge_shareable(const PPParams& p, const PPCurve& cv, int type, unsigned sflags, unsigned cbits,
                                                  double wStart, double wEnd, double speed) {
    if (type < 0 || (sflags & (PP_SETUP_MALFORMED | PP_SETUP_COLOCATED)) || cbits >= 4u) return false;
    const double bound = p.horizon + 1e-12 + p.sst;
    if (wEnd < bound) return false;
    const double dist = (bound - wStart) * speed;
    if (!(dist <= cv.length)) return false;
    const double tprime = (cv.rho_inv != 0.0) ? dist * cv.rho_inv : dist / cv.rho;
    return tprime < cv.p0;
}
// The class of a shareable edge: (vertex, configuration bits, direction of segment 0), an index into PPParams::share_head.
__device__ __forceinline__ unsigned pp_share_key(unsigned vi, unsigned cbits, int type) {
    return vi * PP_SHARE_KEYS + (cbits & 3u) * 2u + (pp_word_seg_type(type, 0) == 0 ? 0u : 1u);
}
// Shared tracks.  The first arc of a class is one curve whatever the target, so the first step kb of the vertex's time row at which
// that arc lies on a blocked cell is a property of the class (pp_k_arc_stops, PPParams::arc_stop).  An edge that is still on the arc
// at step kb stops there: its pose sweep ends with limit = kb and blocked = 1, and everything the sweep leaves up to that step — hits,
// heading bits, skip bytes — is the same for every such edge of the class.  Its RECORD is not: after the break the end state is sampled
// at endTime on the edge's own curve (Edge.cpp:177-203), so g, h and the last cover are the edge's.  So one such edge per class and
// slice, the head, goes through the skip planner and the pose sweep, pp_k_track_fanout copies its track to the others, the members,
// and every kernel after that treats a member as the swept edge it is.
//
// The rule (pp_edge_stopped_on_arc), on the record as the sweeps will read it, with bound = horizon + 1e-12 + sst and
// t_kb = tgrid[kb] of the edge's vertex:
//   * the edge is solved (type >= 0, neither malformed nor co-located), cbits < 4, and pp_edge_shareable does not hold;
//   * its class has a kb;
//   * t_kb < min(bound, wEnd): the edge's own loop reaches step kb;
//   * the pose at t_kb, in pp_window_pose's own arithmetic, lies strictly inside segment 0: dist = (t_kb - wStart) * speed has
//     dist <= length, and tprime = dist * rho_inv (or dist / rho where rho_inv is 0) has tprime < p0.
// Why the one test at t_kb covers every step up to kb: the time row never falls (each entry is the one before plus a positive
// increment, rounded), so a step k <= kb has t_k <= t_kb < endTime — the sweep samples it — and t -> (t - wStart) * speed -> tprime
// is the chain of roundings of non-decreasing functions of the horizon rule above: dist(t_k) <= dist(t_kb) <= length, so the retry and
// the clamp of DubinsWrapper::sample can only fire for dist < 0, where they do not look at the curve, and tprime(t_k) <=
// tprime(t_kb) < p0 picks segment 0.  There the pose is pp_curve_seg on the base {0, 0, qth, s0, c0} with qx, qy, rho, rho_inv,
// wStart and speed: the bits pp_k_arc_stops walked (pp_curve_base forms them for both).  It found no blocked cell before kb and one
// at kb, no obstacle stops a sweep, and a chunk the skip planner spares the grid test provably has no blocked pose: limit = kb.
__device__ __forceinline__ bool pp_edge_stopped_on_arc(const PPParams& p, const PPCurve& cv, int type, unsigned sflags, unsigned vi, unsigned cbits,
                                                       double wStart, double wEnd, double speed) {
    if (type < 0 || (sflags & (PP_SETUP_MALFORMED | PP_SETUP_COLOCATED)) || cbits >= 4u) return false;
    const int kb = p.arc_stop[pp_share_key(vi, cbits, type)];
    if (kb < 0) return false;
    const double t_kb = p.tgrid[(size_t)vi * p.ng + kb];
    if (!(t_kb < fmin(p.horizon + 1e-12 + p.sst, wEnd))) return false;
    const double dist = (t_kb - wStart) * speed;
    if (!(dist <= cv.length)) return false;
    const double tprime = (cv.rho_inv != 0.0) ? dist * cv.rho_inv : dist / cv.rho;
    return tprime < cv.p0;
}
// The head of a class is its member with the lowest position in the caller's list: the minimum of the positions, whatever order
// they arrive in.  It is taken in three stages, each of which passes on only what can still lower the table's entry.
//   1. The wave.  The lanes that hold a position below the entry (a plain look first: in a later slice nearly every lane leaves here)
//      take turns by key; for each key ONE lane goes on.  It is the lowest such lane, and that lane holds the wave's lowest position
//      of the key: work items of one configuration map to list positions in rising order (pp_edge_position), in explicit lists they
//      are the positions.  (One atomic per member would be 70 000 same-address atomics at ~12.5 ns each.)
//   2. The workgroup (PPElectLds, pp_share_elect_wave).  That lane takes the minimum in LDS, in the slot its key maps to.  A slot holds
//      one key, the first that claimed it; a lane that finds another key's claim goes to the table itself, so nothing is lost, and a
//      dense launch, whose workgroup sees the classes of a vertex or two — eight of each kind, the stop classes half the slots away —
//      does not unless its vertex count puts the two kinds on the same slots (nverts * 8 = 32 mod 64): then the loser's atomic goes to
//      the table, one per wave and key, and the result is the same.
//   3. The table (pp_share_elect_flush), after a barrier: one lane per claimed slot looks at the entry and issues the atomicMin where
//      the slot's position is lower.  At most one atomic per workgroup and class, where every working wave of a launch used to issue
//      one per class, all resident at once (so the look saw an empty table), all on the one line a vertex's keys shared.
// No lane waits for another wave's result; every loop is bounded by the lanes of a wave.
#define PP_ELECT_SLOTS 64
struct PPElectLds { unsigned key[PP_ELECT_SLOTS], pos[PP_ELECT_SLOTS]; };
__device__ __forceinline__ void pp_share_elect_wave(const PPParams& p, PPElectLds& lds, bool member, unsigned key, unsigned pos) {
    bool pend = false;
    if (member) pend = pos < __hip_atomic_load(pp_share_entry(p, key), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long m;
    while ((m = __ballot(pend)) != 0ull) {
        const int leader = __ffsll((long long)m) - 1;
        const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)key, leader);
        if (pp_lane() == leader) {
            // (a stop class sits 32 slots from the horizon class of the same vertex, configuration and direction: their keys differ by
            // nverts * 8, which is 0 mod 64 for the 64 open vertices of a dense launch)
            const unsigned slot = (k0 + (k0 >= pp_stop_key_base(p.nverts) ? PP_ELECT_SLOTS / 2u : 0u)) & (PP_ELECT_SLOTS - 1u);
            const unsigned was = atomicCAS(&lds.key[slot], PP_SHARE_NONE, k0);
            if (was == PP_SHARE_NONE || was == k0) atomicMin(&lds.pos[slot], pos);
            else atomicMin(pp_share_entry(p, k0), pos);
        }
        if (key == k0) pend = false;
    }
}
__device__ __forceinline__ void pp_share_elect_flush(const PPParams& p, const PPElectLds& lds) {
    if (threadIdx.x >= PP_ELECT_SLOTS) return;
    const unsigned k = lds.key[threadIdx.x], pos = lds.pos[threadIdx.x];
    if (k == PP_SHARE_NONE) return;
    if (pos < __hip_atomic_load(pp_share_entry(p, k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(pp_share_entry(p, k), pos);
}
// what a lane's records ask of the election: its own edge's (0) and, where it wrote its fast partner's record too, that one's (1)
struct PPElectAsk { bool member0, member1, two; unsigned key0, key1, pos0, pos1; };

// ALL_WORDS: the solver evaluates all six words correctly rounded and pp_curve_init every base heading (pp_k_solve_edges_all_words,
// PPGPU_SOLVE_ALL_WORDS=1, for the tests that compare the two); else only the words that can win, and no sin / cos of the curve's
// bases twice (pp_solve_rank.h, PPSincosMemo): the same records.  Two kernels, so that the test path does not set the registers of
// the production one.
// The records of work item e (a lane that has none to write leaves at once), and what they ask of the election.
template <bool ALL_WORDS>
__device__ __forceinline__ void pp_solve_edge_records(const PPParams& p, long long e, PPElectAsk& ask) {
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
    // (shared sweeps: the rule, once per record.  Two of each by name and not arrays: the loop below is not always unrolled, and an array
    // indexed by k then lives in scratch)
    bool member0 = false, member1 = false;
    unsigned key0 = 0u, key1 = 0u, pos0 = 0u, pos1 = 0u;
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
        if (p.share_head) {
            // (the class of a member, PP_SHARE_NONE for any other edge, PP_SHARE_UNSWEPT for one no kernel sweeps anyway: pp_k_mark_sweeps
            // reads it there, without a look at the record, and puts the edge's head in its place)
            const long long egk = k ? pp_edge_position(p, p.e_base + e2) : eg;
            bool member = pp_edge_shareable(p, cv, S.type, S.sflags, S.cbits, S.wStart, S.wEnd, S.speed);
            const bool unswept = S.type < 0 || (S.sflags & (PP_SETUP_MALFORMED | PP_SETUP_COLOCATED)) != 0u;
            unsigned key = member ? pp_share_key(S.vi, S.cbits, S.type) : PP_SHARE_NONE;
            // (shared tracks: an edge of neither kind of class stays PP_SHARE_NONE; the stop classes have the table's second half)
            if (p.arc_stop && !member && pp_edge_stopped_on_arc(p, cv, S.type, S.sflags, S.vi, S.cbits, S.wStart, S.wEnd, S.speed)) {
                member = true;
                key = pp_stop_key_base(p.nverts) + pp_share_key(S.vi, S.cbits, S.type);
            }
            if (k) { member1 = member; key1 = key; pos1 = (unsigned)egk; } else { member0 = member; key0 = key; pos0 = (unsigned)egk; }
            p.share_of[egk] = unswept ? PP_SHARE_UNSWEPT : key;          // (an unswept edge is no member)
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
    ask.member0 = member0; ask.key0 = key0; ask.pos0 = pos0;
    ask.member1 = member1; ask.key1 = key1; ask.pos1 = pos1;
    ask.two = e2 >= 0;
}
// A workgroup of pp_k_solve_edges: 256 work items.  With shared sweeps every wave reaches both barriers of the election, also the
// waves whose lanes all left pp_solve_edge_records at once (the fast configurations of a dense launch, the lanes past n_edges).
template <bool ALL_WORDS>
__device__ __forceinline__ void pp_solve_edges_body(const PPParams& p) {
    __shared__ PPElectLds lds;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    pp_launch_reset(p, e);
    if (p.share_head) {
        if (threadIdx.x < PP_ELECT_SLOTS) { lds.key[threadIdx.x] = PP_SHARE_NONE; lds.pos[threadIdx.x] = PP_SHARE_NONE; }
        __syncthreads();
    }
    PPElectAsk ask;
    ask.member0 = ask.member1 = ask.two = false;
    ask.key0 = ask.key1 = PP_SHARE_NONE; ask.pos0 = ask.pos1 = 0u;
    pp_solve_edge_records<ALL_WORDS>(p, e, ask);
    if (p.share_head) {
        pp_share_elect_wave(p, lds, ask.member0, ask.key0, ask.pos0);
        if (__ballot(ask.two) != 0ull) pp_share_elect_wave(p, lds, ask.member1, ask.key1, ask.pos1);
        __syncthreads();
        pp_share_elect_flush(p, lds);
    }
}
// After the solve of a slice, one lane per edge; every edge that is in no class leaves after one coalesced 4-byte read.  A member of a
// class that is not its head (the table is final for every class that has a
// member up to this slice: the head is the lowest position, and later slices hold higher ones) is marked PP_SETUP_SHARED, so that
// every per-edge kernel of the launch leaves it at once, and gets a stub record — its own type byte, approx_cost and param[], everything
// else zero (no flags, no ribbons, h = 0) — so that no kernel that builds a list from the records (pp_k_deferred_list,
// pp_k_tsp_table_list, the unfused heuristic kernels) takes what the caller's array held for a deferred or overflowed record.
//
// The sweep list.  The same visit decides which edges of the slice are swept at all — the solved ones that are neither malformed, nor
// co-located, nor (now) shared — and packs their slice positions into p.sweep_list, as pp_k_approach_events packs the live list:
// ballot and popcount per wave, one atomic per workgroup (which also adds to the launch's total), 32-bit entries; the order of the
// workgroups in the list is whatever order they got here in.  The skip planner and the pose sweep walk that list and never see the
// other edges, so those get here what the pose sweep used to leave them: the zeroed summary.  That is all anyone reads of them —
// pp_k_approach_events leaves such an edge before it looks at its track; the cover sweep's wave and pp_k_cover_finish read limit,
// blocked and dub_err, and with limit = 0 no step of it executes: no word of track_eq, no chunk sum, no skip byte is asked for; a
// trace reads the setup records only.  p.sweep_list == NULL: no list (PPGPU_SWEEP_LIST=0), the planner and the sweep walk every edge.
// With a list, 1 024 edges per workgroup (the host picks the size: without a list it stays at 256, which measures 4 us faster where no
// workgroup has anything to add up) and ONE atomic for both counters (they share a 64-bit word: the slice's count in its low half, which the
// add returns, the launch's total in its high half): a line takes an atomic every ~12.5 ns, and 231 of them stay under 3 us where
// two per 256 edges would be 23.  The kernel's stores all come after its last barrier (a barrier waits for the stores before it).
//
// Shared tracks.  A member of a stop class that is not the class's head of this slice is a swept edge whose track comes from that
// head: it is packed into stop_list — stop_count counts the entries (a second 64-bit atomic, only in a workgroup that has some) — which
// pp_k_track_fanout appends to the sweep list behind the prefix that sweep_count bounds, and stop_of holds its head's slice position.  Its
// share_of entry becomes PP_SHARE_NONE like the head's: a stop member is not a shared edge.
#define PP_MARK_THREADS 1024         // with a list
#define PP_MARK_THREADS_PLAIN 256    // without
__global__ __launch_bounds__(PP_MARK_THREADS) void pp_k_mark_sweeps(PPParams p) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = e < p.n_edges;
    const long long eg = valid ? pp_edge_position(p, p.e_base + e) : 0;
    const unsigned key = valid ? p.share_of[eg] : PP_SHARE_UNSWEPT;                  // as pp_k_solve_edges left it
    unsigned head = PP_SHARE_NONE;                                                   // whose results the edge takes: its own
    unsigned trackHead = PP_SHARE_NONE;                                              // whose track it takes (a stop member): its own
    if (key != PP_SHARE_UNSWEPT && key != PP_SHARE_NONE) {
        head = *pp_share_entry(p, key);
        if (head == (unsigned)eg) head = PP_SHARE_NONE;
        // (a stop class: its head is swept like any edge, its members keep their own results; no launch without p.arc_stop has such a key)
        if (key >= pp_stop_key_base(p.nverts)) { trackHead = head; head = PP_SHARE_NONE; }
    }
    const bool stopMember = trackHead != PP_SHARE_NONE;
    const bool swept = key != PP_SHARE_UNSWEPT && head == PP_SHARE_NONE && !stopMember;
    unsigned at = 0u, atStop = 0u;
    if (p.sweep_list) {
        __shared__ unsigned s_cnt[PP_MARK_THREADS / 64], s_cntStop[PP_MARK_THREADS / 64];
        __shared__ unsigned s_base, s_baseStop;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const unsigned long long m = __ballot(swept), ms = __ballot(stopMember);
        if (lane == 0) { s_cnt[wave] = (unsigned)__popcll(m); s_cntStop[wave] = (unsigned)__popcll(ms); }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned tot = 0, totStop = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); w++) { tot += s_cnt[w]; totStop += s_cntStop[w]; }
            // (no carry out of the low half: it is cleared per slice and a slice has fewer than 2^32 edges.  The launch's total counts the
            // stop members too: they are swept edges that took their track from a head)
            s_base = (tot + totStop) ? (unsigned)atomicAdd(pp_sweep_counters(p.words), ((unsigned long long)(tot + totStop) << 32) | tot) : 0u;
            s_baseStop = totStop ? (unsigned)atomicAdd(pp_stop_counters(p.words), ((unsigned long long)totStop << 32) | totStop) : 0u;
        }
        __syncthreads();
        at = s_base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        atStop = s_baseStop + (unsigned)__popcll(ms & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) { at += s_cnt[w]; atStop += s_cntStop[w]; }
    }
    if (!valid) return;
    if (key != PP_SHARE_NONE) p.share_of[eg] = head;
    if (head != PP_SHARE_NONE) {
        PPEdgeSetup* S = p.setup + p.ws_base + e;
        S->sflags |= PP_SETUP_SHARED;
        double* r = reinterpret_cast<double*>(p.out + eg);
        const unsigned info = (unsigned)(S->type & 0xff);
        r[0] = __hiloint2double((int)info, 0);
        r[1] = 0.0; r[2] = 0.0; r[3] = S->approx;
        for (int i = 4; i < 13; i++) r[i] = 0.0;
        r[13] = S->p0; r[14] = S->p1; r[15] = S->p2;
    }
    if (!p.sweep_list) return;
    if (swept) p.sweep_list[at] = (unsigned)e;                 // (a slice position: below 2^32, as the live list's)
    else if (stopMember) {
        // on a list of its own, which pp_k_track_fanout puts behind the prefix once the skip planner and the pose sweep have walked that.
        // That kernel gives the edge its summary and its track, pp_k_approach_events its track_far: nothing of either is written here
        p.stop_list[atStop] = (unsigned)e;
        p.stop_of[e] = (unsigned)pp_edge_slice_position(p, (long long)trackHead);
    } else {
        reinterpret_cast<int4*>(p.track_summary)[p.ws_base + e] = make_int4(0, 0, 0, 0);   // (PPTrackSummary, pp_k_sweep.h: {limit, blocked, dub_err, pad})
        if (p.approach_list) {
            // what pp_k_approach_events would have left: a shared edge is done; an edge without a curve goes to the cover sweep's wave
            // from its step 0 (its record is the wave's to write), so it takes a place on the live list here — a handful per launch
            if (head != PP_SHARE_NONE) {
                p.track_far[p.ws_base + e] = make_int2(PP_FAR_DONE, 0);
            } else {
                p.track_far[p.ws_base + e] = make_int2(0, 0);
                const unsigned li = atomicAdd(&p.words->live_count, 1u);
                p.live_list[2 * (size_t)li] = (unsigned)e;
                p.live_list[2 * (size_t)li + 1] = (unsigned)eg;
            }
        }
    }
}
// Last kernel of the launch, 16 lanes per record (one 128-byte line read, one written): every member takes its head's record but for
// the three fields that are the edge's own (type byte, approx_cost, param[]: the stub holds them) and, copy_child, the head's child slot.
// It also leaves the table of heads as the next launch's solve wants to find it, all-ones: nobody reads the table any more (the
// kernel itself goes by share_of), so the next launch needs no fill in front of its first kernel.  The host fills the table itself
// only when it is new, or when a launch ended before this kernel.
__global__ __launch_bounds__(256) void pp_k_share_fanout(PPParams p, int copy_child) {
    const unsigned long long n_keys = (unsigned long long)p.nverts * PP_SHARE_KEYS;        // (below 2^32: cost_modes)
    for (unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x; k < n_keys; k += (unsigned long long)gridDim.x * 256u)
        *pp_share_entry(p, (unsigned)k) = PP_SHARE_NONE;
    const long long eg = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = (int)(threadIdx.x & 15);
    if (eg >= p.n_edges) return;
    const unsigned h = p.share_of[eg];
    if (h == PP_SHARE_NONE) return;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(p.out + h);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(p.out + eg);
    unsigned long long v = src[sub];
    if (sub == 0) v = (v & ~(0xffull << 32)) | (dst[0] & (0xffull << 32));      // {flags (low word), info (high word): its bits 0-7 are the type}
    if (sub != 3 && sub < 13) dst[sub] = v;
    if (copy_child) {
        const double* cs = p.child + (size_t)h * p.stride * 4;
        double* cd = p.child + (size_t)eg * p.stride * 4;
        for (int i = sub; i < p.stride * 4; i += 16) cd[i] = cs[i];
    }
}
__global__ __launch_bounds__(256, PP_SOLVE_MIN_WAVES) void pp_k_solve_edges(PPParams p) { pp_solve_edges_body<false>(p); }
__global__ __launch_bounds__(256, PP_SOLVE_MIN_WAVES) void pp_k_solve_edges_all_words(PPParams p) { pp_solve_edges_body<true>(p); }
