// pp_k_tsp_table.h — the point-robot TSP heuristics (RibbonManager.cpp:53-94) and the Dubins-TSP heuristics (:97-140) of child lists
// the enumeration declines, by an exact table over (ribbons done, last ribbon, end entered).  Opt-in (ppgpu_set_tsp_table,
// ppgpu_set_dubins_tsp_table).  Included by pp_kernels.h.
#pragma once
// The reference accumulates soFar' = fmax(soFar + len - 2w + dist, 0) from the root to a leaf and takes fmin over the leaves.  Every
// step is a non-decreasing function of soFar (a rounded addition is monotone, and so is fmax), so the minimum over all tours that
// reach "these ribbons done, standing at this endpoint" may be taken BEFORE the next step: the smallest soFar gives the smallest
// soFar', and fmin picks one of its arguments.  The table
//     G[S][2r + e] = min over (r', e') in S \ {r} of fmax(G[S \ {r}][2r' + e'] + len_r - 2w + T[exit(r', e')][entry(r, e)], 0)
// (e = 0: ribbon r entered at its start and left at its end; e = 1 the other way round; layer 1 steps from the query point with
// soFar = 0) therefore ends in min over (r, e) of G[all][2r + e] = the enumeration's value, bit for bit, in O(2^n n^2) steps where
// the enumeration has n! 2^n leaves.  Same expressions (pp_dist, pp_h_T), same left-to-right association as pp_tsp_child.
//
// K variant: from a node only the first min(K, remaining) ribbons of the stable descending sort by KM[point][i] are entered.  That
// set is a function of (remaining set, point) — of the state — unless the K-th and (K+1)-th keys are equal: then the reference's
// choice follows the list order inherited along the path.  A record with such a straddling tie in any reachable state is REFUSED:
// it keeps its flag and h = 0 and the host answers, as before.  Ties inside or outside the chosen set do not matter.  The chosen
// set of every reachable state is written once, next to G (M: 16 bits per state), by the lanes that made the state.
//
// Dubins variants (DUBINS = true, a kernel of its own): the same recursion over T[p][q] = the Dubins length from oriented point p to
// oriented point q (pp_heuristic_edge_dubins: a ribbon's end faces the other end, the query pose carries the child's heading),
// a ribbon's own length from LEN and not from T.  T and LEN are filled by a kernel of their own (pp_k_tsp_table_dubins_T, 256
// threads: the six-word solve needs more registers than a wave of a 1 024-thread workgroup has — built inside the table kernel it
// took all 128 and spilled 83 more) into global memory, one block per listed record, and the table kernel copies its record's in.
// T is not symmetric, and nothing above needs it to be: the step is still fmax(g + LEN[r] - 2w + T[exit][entry], 0), monotone in g.
// The reference's K variant never limits (pp_heuristic_edge), so every remaining ribbon may be entered: no chosen sets, no M, no
// refusal.  A pair on which the solver leaves no word has p0 = p1 = p2 = 0 and pp_dubins_length gives 0: the enumeration feeds that
// 0 into fmin / fmax and so does the table — the same result, no refusal.
#define PP_TSP_TABLE_MAX 16
static_assert(PP_TSP_TABLE_MAX == PPGPU_TSP_TABLE_MAX && PP_TSP_TABLE_MAX <= 16, "the header states the capacity; a state's chosen set is 16 bits");
#define PP_TT_THREADS 1024                       // 16 waves = 32 half-waves; a half-wave takes one subset at a time
#define PP_TT_GRID 1024                          // at most this many workgroups (and slots)
#ifndef PP_TSP_TABLE_BYTES
#define PP_TSP_TABLE_BYTES (1ull << 30)          // workspace budget of the pass: as many slots as fit (at most 1 GiB)
#endif
static_assert(PP_TSP_TABLE_BYTES <= (1ull << 30), "the table pass takes at most 1 GiB of workspace");
#define PP_TT_PTS (2 * PP_TSP_TABLE_MAX + 1)
#define PP_TT_TSTRIDE (PP_TT_PTS * (PP_TT_PTS - 1) + PP_TSP_TABLE_MAX)   // Dubins variants, per listed record: T in the layout of s_T, then LEN
#define PP_TT_TCAP 4096                          // ... for at most this many records of a launch (35 MB); the records beyond stay with the host
#define PP_TT_UNREACHED (-1.0)                   // a state no admissible tour reaches (every real value is >= 0: the clamp)

// A slot sized for lists of up to `cap` ribbons: G (doubles), the subsets in layer order (words), M (16 bits per state)
__host__ __device__ inline size_t pp_tt_states(int cap) { return ((size_t)1 << cap) * (size_t)(2 * cap); }
__host__ __device__ inline size_t pp_tt_slot_bytes(int cap) { return pp_tt_states(cap) * 8 + ((size_t)4 << cap) + ((pp_tt_states(cap) * 2 + 7) & ~(size_t)7); }

struct PPTspTableArgs {
    ppgpu_edge_result* out; const double* child; int stride; long long n_edges;
    int heuristic, tsp_k; double ribw, max_speed, tpf;
    double h_rho;                        // turning radius of the Dubins-TSP heuristics' table
    int min_ribbons, max_ribbons;        // min_ribbons = 0: the records the enumeration flagged
    unsigned* list; unsigned* count;     // the records to take; count[0] how many, count[1] the longest of them
    unsigned list_cap;                   // room in `list` (allocated with the switch): records beyond it stay as they are, for the host
    unsigned long long* stats;           // [0] lists answered, [1] lists refused (cumulative)
    unsigned char* slots; size_t bytes;  // the workspace: cut into slots for the longest list of the launch
    double* T;                           // Dubins variants: PP_TT_TSTRIDE doubles per listed record (list_cap is at most PP_TT_TCAP then)
};

__global__ __launch_bounds__(256) void pp_k_tsp_table_list(PPTspTableArgs q) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= q.n_edges) return;
    const ppgpu_edge_result* rec = q.out + e;
    const unsigned flags = rec->flags;
    const int nrib = (int)((rec->info >> 8) & 0xffu);
    if (flags & (PPGPU_F_THROWS | PPGPU_F_DUBINS_ERR | PPGPU_F_RIBBON_LOST)) return;
    if (nrib < 1 || nrib > q.stride || nrib > q.max_ribbons) return;
    if (q.min_ribbons > 0 ? nrib < q.min_ribbons : !(flags & PPGPU_F_RIBBON_OVF)) return;
    const unsigned at = atomicAdd(q.count, 1u);          // (few records: the order of the list does not matter)
    if (at >= q.list_cap) return;
    q.list[at] = (unsigned)e;
    atomicMax(q.count + 1, (unsigned)nrib);
}

template <bool DUBINS>
__device__ __forceinline__ void pp_tsp_table_run(const PPTspTableArgs& q) {
    constexpr int MAXN = PP_TSP_TABLE_MAX;
    constexpr int KMN = DUBINS ? 1 : PP_TT_PTS * MAXN;                          // the K variant's keys and masks: point-robot only
    __shared__ double s_pts[DUBINS ? 1 : 2 * PP_TT_PTS];
    __shared__ double s_T[PP_TT_PTS * (PP_TT_PTS - 1)];
    __shared__ double s_KM[KMN];
    __shared__ unsigned short s_gt[KMN], s_eq[KMN];                             // ribbons whose key from point p is greater than / equal to ribbon i's
    __shared__ double s_len[DUBINS ? MAXN : 1];                                 // Ribbon::length() of every ribbon
    __shared__ unsigned s_binom[MAXN + 1][MAXN + 1];
    __shared__ unsigned s_first[MAXN + 2];                                      // where layer k starts in the subset list
    __shared__ int s_refuse;
    const unsigned listed = ((volatile unsigned*)q.count)[0];
    const unsigned count = listed < q.list_cap ? listed : q.list_cap;
    if (blockIdx.x >= count) return;
    // Slots sized for the longest list of this launch (<= max_ribbons, for which the workspace holds at least one): shorter lists,
    // more workgroups at work.  The workgroups beyond the last slot leave; the others stride over the list.
    const int cap = (int)((volatile unsigned*)q.count)[1];
    if (cap < 1 || cap > PP_TSP_TABLE_MAX) return;       // (never: the listing kernel takes 1 .. max_ribbons)
    const size_t fit = q.bytes / pp_tt_slot_bytes(cap);
    const unsigned active = fit < (size_t)gridDim.x ? (unsigned)fit : gridDim.x;
    if (blockIdx.x >= active) return;
    const int tid = threadIdx.x;
    const int hw = tid >> 5, hl = tid & 31;              // half-wave and the lane within it
    const int sub = hl & 15, grp = hl >> 4;              // the two groups of sixteen of a half-wave
    unsigned char* slot = q.slots + (size_t)blockIdx.x * pp_tt_slot_bytes(cap);
    double* G = (double*)slot;
    unsigned* order = (unsigned*)(slot + pp_tt_states(cap) * 8);
    unsigned short* M = (unsigned short*)(slot + pp_tt_states(cap) * 8 + ((size_t)4 << cap));
    const bool kvar = !DUBINS && q.heuristic == PPGPU_H_TSP_POINT_K;
    const int K = q.tsp_k;
    const bool nothing = DUBINS ? (q.heuristic == PPGPU_H_TSP_DUBINS_K && K <= 0) : (kvar && K <= 0);
    const double twoW = 2 * q.ribw;
    if (tid < (MAXN + 1) * (MAXN + 1)) {                 // Pascal's triangle, row a column b
        const int a = tid / (MAXN + 1), b = tid - a * (MAXN + 1);
        unsigned long long v = b <= a ? 1ull : 0ull;
        for (int i = 1; i <= b && b <= a; i++) v = v * (unsigned long long)(a - b + i) / (unsigned long long)i;
        s_binom[a][b] = (unsigned)v;
    }
    int listedN = 0;                                     // the subset list in the slot is that of this many ribbons
    for (unsigned li = blockIdx.x; li < count; li += active) {
        const long long e = (long long)q.list[li];
        ppgpu_edge_result* rec = q.out + e;
        const int n = (int)((rec->info >> 8) & 0xffu);   // 1 .. cap (pp_k_tsp_table_list)
        if (nothing) {                                   // the reference's loop body never runs: DBL_MAX (pp_h_tsp_point)
            if (tid == 0) {
                pp_h_store(rec, rec->g, PP_DBL_MAX, q.max_speed, q.tpf);
                rec->flags &= ~PPGPU_F_RIBBON_OVF;
                atomicAdd(q.stats, 1ull);
            }
            continue;
        }
        const int npts = 2 * n + 1, ncol = npts - 1;
        if constexpr (DUBINS) {                          // T and LEN of this record as pp_k_tsp_table_dubins_T left them
            const double* t = q.T + (size_t)li * PP_TT_TSTRIDE;
            if (tid == 0) s_refuse = 0;
            if (tid < n) s_len[tid] = t[PP_TT_PTS * (PP_TT_PTS - 1) + tid];
            for (int idx = tid; idx < npts * ncol; idx += PP_TT_THREADS) {
                const int pp = idx / ncol, at = pp * (PP_TT_PTS - 1) + (idx - pp * ncol);
                s_T[at] = t[at];
            }
            __syncthreads();                             // (the first barrier of a workgroup: Pascal's triangle is whole before s_first is made of it)
        } else {
            if (tid == 0) { s_pts[0] = rec->end_x; s_pts[1] = rec->end_y; s_refuse = 0; }
            if (tid < n) {
                const double* c = q.child + ((size_t)e * q.stride + tid) * 4;
                s_pts[2 * (1 + 2 * tid)] = c[0]; s_pts[2 * (1 + 2 * tid) + 1] = c[1];
                s_pts[2 * (2 + 2 * tid)] = c[2]; s_pts[2 * (2 + 2 * tid) + 1] = c[3];
            }
            __syncthreads();
            for (int idx = tid; idx < npts * ncol; idx += PP_TT_THREADS) {
                const int pp = idx / ncol, qq = 1 + (idx - pp * ncol);
                s_T[pp * (PP_TT_PTS - 1) + (qq - 1)] = pp_dist(s_pts[2 * pp], s_pts[2 * pp + 1], s_pts[2 * qq], s_pts[2 * qq + 1]);
            }
        }
        if (n != listedN) {                              // the subsets of {0 .. n-1}, layer after layer (combinadic rank within a layer)
            if (tid == 0) {
                unsigned at = 0;
                for (int k = 0; k <= n; k++) { s_first[k] = at; at += s_binom[n][k]; }
                s_first[n + 1] = at;
            }
            __syncthreads();
            for (unsigned S = (unsigned)tid; S < (1u << n); S += PP_TT_THREADS) {
                unsigned rank = 0, rest = S;
                int i = 0;
                while (rest) { const int b = __ffs((int)rest) - 1; rest &= rest - 1u; i++; rank += s_binom[b][i]; }
                order[s_first[i] + rank] = S;
            }
            listedN = n;
        }
        __syncthreads();
        if constexpr (!DUBINS) {                         // the K variant's keys and what each ribbon's key is beaten / equalled by (the Dubins variants have neither stage)
            for (int idx = tid; idx < npts * n; idx += PP_TT_THREADS) {
                const int pp = idx / n, ri = idx - pp * n;
                s_KM[pp * MAXN + ri] = fmin(pp_h_T<MAXN>(s_T, pp, 1 + 2 * ri), pp_h_T<MAXN>(s_T, pp, 2 + 2 * ri));
            }
            __syncthreads();
            if (kvar)
                for (int idx = tid; idx < npts * n; idx += PP_TT_THREADS) {
                    const int pp = idx / n, ri = idx - pp * n;
                    const double key = s_KM[pp * MAXN + ri];
                    unsigned gt = 0, eq = 0;
                    for (int j = 0; j < n; j++) {
                        const double kj = s_KM[pp * MAXN + j];
                        gt |= (kj > key ? 1u : 0u) << j;
                        eq |= ((kj == key && j != ri) ? 1u : 0u) << j;
                    }
                    s_gt[pp * MAXN + ri] = (unsigned short)gt; s_eq[pp * MAXN + ri] = (unsigned short)eq;
                }
            __syncthreads();
        }
        const unsigned full = (1u << n) - 1u;
        const int row = 2 * n;                           // states per subset
        // The ribbons that may be entered from a state (remaining set R, point pt): lane `sub` of a group of sixteen answers for
        // ribbon `sub`; the group's sixteen bits of the ballot are the set.  With fewer than K ribbons left all of them are in it.
        auto chosen = [&](unsigned R, int pt, bool reached, bool& tie) -> unsigned {
            bool in = sub < n && ((R >> sub) & 1u);
            tie = false;
            if (kvar && in) {
                const int gt = __popc((unsigned)s_gt[pt * MAXN + sub] & R), ge = gt + __popc((unsigned)s_eq[pt * MAXN + sub] & R);
                tie = reached && gt < K && ge >= K;      // this ribbon's run of equal keys straddles the K-th place
                in = ge < K;
            }
            const unsigned long long b = __ballot(in);
            return (unsigned)(b >> (16 * (pp_lane() >> 4))) & 0xffffu;
        };
        bool tie0 = false;
        const unsigned m0 = DUBINS ? full : chosen(full, 0, true, tie0);
        if (tie0) s_refuse = 1;
        __syncthreads();
        bool refused = s_refuse != 0;
        __syncthreads();                                 // everyone has read the flag before layer 1 may set it
        for (int k = 1; k <= n && !refused; k++) {
            const unsigned first = s_first[k], cnt = s_first[k + 1] - first;
            const unsigned trips = (cnt + 31u) / 32u;    // the same for every half-wave: the ballots and shuffles below are taken by whole waves
            for (unsigned t = 0; t < trips; t++) {
                const unsigned at = t * 32u + (unsigned)hw;
                const bool have = at < cnt;
                const unsigned S = have ? order[first + at] : 0u;
                unsigned rest = S;
                for (int i = 0; i < k; i++) {
                    // r = the i-th ribbon of this half-wave's S: k of them in every subset of the layer, so the trip count is the wave's
                    // (a half-wave past the end of the layer only keeps the other one company)
                    const bool mine = have;
                    const int r = have ? __ffs((int)rest) - 1 : 0;
                    rest &= rest - 1u;
                    const unsigned Sp = S & ~(1u << r);
                    double len;                              // Ribbon::length()
                    if constexpr (DUBINS) len = s_len[r]; else len = pp_h_T<MAXN>(s_T, 1 + 2 * r, 2 + 2 * r);
                    double v0 = PP_DBL_MAX, v1 = PP_DBL_MAX;     // into r's start / end
                    if (k == 1) {
                        if (mine && hl == 0 && ((m0 >> r) & 1u)) {
                            v0 = fmax(0.0 + len - twoW + pp_h_T<MAXN>(s_T, 0, 1 + 2 * r), 0);
                            v1 = fmax(0.0 + len - twoW + pp_h_T<MAXN>(s_T, 0, 2 + 2 * r), 0);
                        }
                    } else if (mine && hl < row && ((Sp >> (hl >> 1)) & 1u)) {
                        // lane hl = state 2r' + e' of the row of S \ {r}: one coalesced read
                        const double g = G[(size_t)Sp * row + hl];
                        const bool ok = g >= 0 && (!kvar || ((M[(size_t)Sp * row + hl] >> r) & 1u));
                        if (ok) {
                            const int ex = (hl & 1) ? 1 + 2 * (hl >> 1) : 2 + 2 * (hl >> 1);     // where (r', e') leaves its ribbon
                            v0 = fmax(g + len - twoW + pp_h_T<MAXN>(s_T, ex, 1 + 2 * r), 0);
                            v1 = fmax(g + len - twoW + pp_h_T<MAXN>(s_T, ex, 2 + 2 * r), 0);
                        }
                    }
                    // the low sixteen lanes gather the minimum into r's start, the high sixteen the one into its end
                    const double other = __shfl_xor(grp ? v0 : v1, 16);
                    double x = fmin(grp ? v1 : v0, other);
#pragma unroll
                    for (int m = 8; m >= 1; m >>= 1) x = fmin(x, __shfl_xor(x, m));
                    const bool reached = mine && x != PP_DBL_MAX;
                    // state (S, 2r + grp) leaves r at its end (grp 0) or start (grp 1); what may be entered from there
                    bool tie = false;
                    unsigned m = 0;
                    if (kvar && k < n) m = chosen(full & ~S, grp ? 1 + 2 * r : 2 + 2 * r, reached, tie);
                    if (tie) s_refuse = 1;
                    if (mine && sub == 0) {
                        G[(size_t)S * row + 2 * r + grp] = reached ? x : PP_TT_UNREACHED;
                        if (kvar) M[(size_t)S * row + 2 * r + grp] = (unsigned short)m;
                    }
                }
            }
            __syncthreads();                             // layer k is whole; layer k + 1 reads nothing else
            refused = s_refuse != 0;
            __syncthreads();                             // ... and everyone has read the flag before layer k + 1 may set it: the
                                                         // whole workgroup leaves the loop at the same layer
        }
        if (tid == 0) {
            if (refused) {
                atomicAdd(q.stats + 1, 1ull);
            } else {
                double hdist = PP_DBL_MAX;
                for (int j = 0; j < row; j++) {
                    const double g = G[(size_t)full * row + j];
                    if (g >= 0) hdist = fmin(hdist, g);
                }
                pp_h_store(rec, rec->g, hdist, q.max_speed, q.tpf);
                rec->flags &= ~PPGPU_F_RIBBON_OVF;
                atomicAdd(q.stats, 1ull);
            }
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(PP_TT_THREADS) void pp_k_tsp_table(PPTspTableArgs q) { pp_tsp_table_run<false>(q); }

// T and LEN of every listed record for the Dubins variants, exactly as pp_heuristic_edge_dubins builds them (the same calls on the
// same values: the same bits).  A workgroup per listed record, striding.
__global__ __launch_bounds__(256) void pp_k_tsp_table_dubins_T(PPTspTableArgs q) {
    __shared__ double s_pts[2 * PP_TT_PTS];
    __shared__ double s_yaw[PP_TT_PTS];
    const unsigned listed = ((volatile unsigned*)q.count)[0];
    const unsigned count = listed < q.list_cap ? listed : q.list_cap;
    if (q.heuristic == PPGPU_H_TSP_DUBINS_K && q.tsp_k <= 0) return;      // the table kernel takes the short way out
    const int tid = threadIdx.x;
    for (unsigned li = blockIdx.x; li < count; li += gridDim.x) {
        const long long e = (long long)q.list[li];
        const ppgpu_edge_result* rec = q.out + e;
        const int n = (int)((rec->info >> 8) & 0xffu);   // 1 .. PP_TSP_TABLE_MAX (pp_k_tsp_table_list)
        double* t = q.T + (size_t)li * PP_TT_TSTRIDE;
        if (tid == 0) { s_pts[0] = rec->end_x; s_pts[1] = rec->end_y; s_yaw[0] = rec->end_heading; }   // the heading where the callee says yaw (Vertex.cpp:51) — kept
        if (tid < n) {
            const double* c = q.child + ((size_t)e * q.stride + tid) * 4;
            const double sx = c[0], sy = c[1], ex = c[2], ey = c[3];
            s_pts[2 * (1 + 2 * tid)] = sx; s_pts[2 * (1 + 2 * tid) + 1] = sy;
            s_pts[2 * (2 + 2 * tid)] = ex; s_pts[2 * (2 + 2 * tid) + 1] = ey;
            s_yaw[1 + 2 * tid] = pp_yaw(pp_heading_to(sx, sy, ex, ey));
            s_yaw[2 + 2 * tid] = pp_yaw(pp_heading_to(ex, ey, sx, sy));
            t[PP_TT_PTS * (PP_TT_PTS - 1) + tid] = sqrt(pp_sq_len(sx, sy, ex, ey));       // Ribbon::length()
        }
        __syncthreads();
        const int npts = 2 * n + 1, ncol = npts - 1;
        for (int idx = tid; idx < npts * ncol; idx += 256) {           // RibbonManager::dubinsDistance for every ordered pair
            const int pp = idx / ncol, qq = 1 + (idx - pp * ncol);
            PPDubins d;
            pp_dubins_shortest(s_pts[2 * pp], s_pts[2 * pp + 1], s_yaw[pp], s_pts[2 * qq], s_pts[2 * qq + 1], s_yaw[qq], q.h_rho, d);
            t[pp * (PP_TT_PTS - 1) + (qq - 1)] = pp_dubins_length(d, q.h_rho);
        }
        __syncthreads();
    }
}
// The Dubins-TSP heuristics: an instantiation of its own (no keys, no chosen sets; T and LEN from pp_k_tsp_table_dubins_T).
__global__ __launch_bounds__(PP_TT_THREADS) void pp_k_tsp_table_dubins(PPTspTableArgs q) { pp_tsp_table_run<true>(q); }
