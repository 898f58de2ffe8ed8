// pp_k_expand.h — SamplingBasedPlanner::expand on the device (SamplingBasedPlanner.cpp:82-149): Dubins lengths to every sample, the k nearest
// per radius in the reference's push order, the edge list of a round trip.  Included by pp_kernels.h.
#pragma once
// ------------------------------------------------------------------------------------------ the pieces the kernels below share
// Both Dubins lengths of a (vertex, sample) pair: Edge::computeApproxCost's length for the k-nearest selection of
// SamplingBasedPlanner::expand (SamplingBasedPlanner.cpp:109-119).  (-1, -1) for a sample not farther than the increment
// (State::distanceTo, :111), unless the caller knows it to be farther (FARTHER); one radius in use (`both` false): l1 = l0, the
// second problem is not solved.
template <bool FARTHER = false>
__device__ __forceinline__ void pp_pair_lengths(const ppgpu_vertex& V, double bx, double by, double bh, double rho, double rho_cov, double inc_d,
                                                bool both, double& l0, double& l1) {
    const double ax = V.x, ay = V.y, ayaw = pp_yaw(V.heading), byaw = pp_yaw(bh);
    l0 = l1 = -1;
    if (FARTHER || sqrt((ax - bx) * (ax - bx) + (ay - by) * (ay - by)) > inc_d) {
        PPDubins d;
        pp_dubins_shortest(ax, ay, ayaw, bx, by, byaw, rho, d);
        l0 = l1 = pp_dubins_length(d, rho);
        if (both) {
            pp_dubins_shortest(ax, ay, ayaw, bx, by, byaw, rho_cov, d);
            l1 = pp_dubins_length(d, rho_cov);
        }
    }
}
// Edge::computeApproxCost (Edge.cpp:17) of a length
__device__ __forceinline__ double pp_approx_cost(double len, double max_speed, double tpf) { return len / max_speed * tpf; }
// The one order of every selection here: (l1, i1) before (l2, i2), by length, equal lengths by index.  i < 0 = no entry, after everything.
__device__ __forceinline__ bool pp_pair_less(double l1, int i1, double l2, int i2) {
    return (i1 >= 0) & ((i2 < 0) | (l1 < l2) | ((l1 == l2) & (i1 < i2)));
}
// the minimum of each half wavefront (32 consecutive lanes), to every lane of the half
__device__ __forceinline__ double pp_half_wave_min(double x) {
    for (int o = 16; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o, PP_WAVE));
    return x;
}
// Rank counting: how many of n pairs come before (x, xi).  An entry's index is I[j], or its position j where I is null ("ties by
// position").  Workgroup form: the pairs are in LDS, every thread reads the same word at a time.
__device__ __forceinline__ int pp_rank_lds(const double* L, const int* I, int n, double x, int xi) {
    int rank = 0;
    for (int j = 0; j < n; j++) rank += pp_pair_less(L[j], I ? I[j] : j, x, xi) ? 1 : 0;
    return rank;
}
// The k-th smallest of those n pairs -> *kthL (its index -> *kthI unless null); both are left as they are when fewer than k entries are
// finite.  256 threads; the caller synchronises before (the pairs, the outputs' initial values) and after.
__device__ __forceinline__ void pp_kth_smallest_lds(const double* L, const int* I, int n, int k, double* kthL, int* kthI) {
    for (int j = (int)threadIdx.x; j < n; j += 256) {
        const double x = L[j];
        const int xi = I ? I[j] : j;
        if (!(x < INFINITY)) continue;
        if (pp_rank_lds(L, I, n, x, xi) == k - 1) { *kthL = x; if (kthI) *kthI = xi; }
    }
}
// Wave form: one value per lane, the first n lanes count, ties by lane; every lane gets the k-th smallest, +inf when fewer than k are finite.
__device__ __forceinline__ double pp_kth_smallest_wave(double x, int n, int k) {
    const int lane = pp_lane();
    int rank = 0;
    for (int i = 0; i < n; i++) rank += pp_pair_less(pp_readlane(x, i), i, x, lane) ? 1 : 0;
    const unsigned long long hit = __ballot((lane < n) & (x < INFINITY) & (rank == k - 1));
    return hit ? pp_readlane(x, __ffsll((long long)hit) - 1) : INFINITY;
}
// The k smallest of n entries in ascending (length, index) order, by successive minima: round j finds the successor of round j - 1's
// winner in that order, so no exclusion list is needed.  `entry(c, l, i)` gives entry c and says whether it counts.  NT = 256: the whole
// workgroup (wl, wi: LDS scratch of one slot per wave, not what `entry` reads); NT = 64: the one wavefront that calls it.  Indices ->
// oi[0, k), lengths -> ol unless null; -1 where the entries run out.
template <int NT, class Entry>
__device__ __forceinline__ void pp_k_smallest(Entry entry, long long n, int k, int* oi, double* ol, double* wl, int* wi) {
    const int t = (int)threadIdx.x & (NT - 1);
    double prevL = -INFINITY;
    int prevI = -1;
    for (int j = 0; j < k; j++) {
        double bl = INFINITY;
        int bi = -1;
        for (long long c = t; c < n; c += NT) {
            double l;
            int i;
            if (!entry(c, l, i)) continue;
            if ((j == 0 || pp_pair_less(prevL, prevI, l, i)) && pp_pair_less(l, i, bl, bi)) { bl = l; bi = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double l2 = __shfl_xor(bl, o, PP_WAVE);
            const int i2 = __shfl_xor(bi, o, PP_WAVE);
            if (pp_pair_less(l2, i2, bl, bi)) { bl = l2; bi = i2; }
        }
        if (NT > PP_WAVE) {
            __syncthreads();
            if (pp_lane() == 0) { wl[threadIdx.x >> 6] = bl; wi[threadIdx.x >> 6] = bi; }
            __syncthreads();
            bl = wl[0]; bi = wi[0];
            for (int w = 1; w < NT / PP_WAVE; w++)
                if (pp_pair_less(wl[w], wi[w], bl, bi)) { bl = wl[w]; bi = wi[w]; }
        }
        if (t == 0) { oi[j] = bi; if (ol) ol[j] = bi >= 0 ? bl : -1.0; }
        prevL = bl; prevI = bi;
        if (bi < 0) {                                                       // fewer than k entries
            for (int jj = j + 1 + t; jj < k; jj += NT) { oi[jj] = -1; if (ol) ol[jj] = -1.0; }
            break;
        }
    }
}
// Append the flagged lanes of a 256-thread workgroup to lists in memory, R flags per thread: slot[j] is where flag j's entry goes (valid
// where take[j]).  ONE_LIST: all R flags go to the list whose length is *count, in flag order; otherwise flag j goes to the list whose
// length is count[j].  One atomic per workgroup and list (a device-scope atomic on one address completes every ~12 ns: per wavefront
// they took longer than everything else in pp_k_expand_candidates); the order of a list is arbitrary.  wcount, wbase: LDS, R * 4 ints each.
template <int R, bool ONE_LIST>
__device__ __forceinline__ void pp_wg_append(const bool (&take)[R], int* count, int* wcount, int* wbase, int (&slot)[R]) {
    const int w = (int)(threadIdx.x >> 6), lane = pp_lane();
    unsigned long long m[R];
#pragma unroll
    for (int j = 0; j < R; j++) {
        m[j] = __ballot(take[j]);
        if (lane == 0) wcount[j * 4 + w] = __popcll(m[j]);
    }
    __syncthreads();
    constexpr int LISTS = ONE_LIST ? 1 : R, PER = (R / LISTS) * 4;         // per-wave counts of one list, consecutive
    if (threadIdx.x < (unsigned)LISTS) {
        const int* wc = wcount + threadIdx.x * PER;
        int* wb = wbase + threadIdx.x * PER;
        int tot = 0;
        for (int i = 0; i < PER; i++) tot += wc[i];
        int base = tot ? atomicAdd(count + threadIdx.x, tot) : 0;
        for (int i = 0; i < PER; i++) { wb[i] = base; base += wc[i]; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < R; j++) slot[j] = wbase[j * 4 + w] + __popcll(m[j] & ((1ull << lane) - 1ull));
}

// ------------------------------------------------------------------------------------------
// Dubins lengths from open vertices to every sample, both radii.  Thread per (vertex, sample); sample loads are coalesced, the vertex
// is a scalar load.
__global__ __launch_bounds__(256) void pp_k_dubins_lengths(const ppgpu_vertex* verts, int v0, const double* sx, const double* sy, const double* sh,
                                                           long long ns, double rho, double rho_cov, double inc_d, double* out) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y;
    if (s >= ns) return;
    double2 o;
    pp_pair_lengths(verts[v0 + v], sx[s], sy[s], sh[s], rho, rho_cov, inc_d, true, o.x, o.y);
    reinterpret_cast<double2*>(out)[(size_t)v * ns + s] = o;
}

// k smallest (length, index) per (vertex, radius), in ascending (length, index) order; one 256-thread workgroup each.
// Two passes over the lengths instead of k: the k-th smallest of the 256 per-thread minima bounds the k-th smallest overall,
// so the second pass keeps the few entries not above that bound and ranks them.  (Fewer than k threads with an entry, or more
// survivors than the list holds - many equal lengths - fall back to k successive minimum scans.)
#define PP_SEL_CAP 1024
__global__ __launch_bounds__(256) void pp_k_select_nearest(const double* lengths, long long ns, int k, int* out_idx, double* out_len) {
    __shared__ double sl[PP_SEL_CAP];
    __shared__ int si[PP_SEL_CAP];
    __shared__ double boundL;
    __shared__ int boundI, count;
    const int vr = blockIdx.x;               // vertex * 2 + radius
    const int v = vr >> 1, r = vr & 1;
    const double* L = lengths + ((size_t)v * ns) * 2 + r;
    int* oi = out_idx + (size_t)vr * k;
    double* ol = out_len + (size_t)vr * k;
    const int tid = (int)threadIdx.x;
    const auto row = [=](long long s, double& l, int& i) { l = L[s * 2]; i = (int)s; return l >= 0; };   // closer than the increment: skipped
    // pass 1: this thread's smallest entry
    double bl = INFINITY;
    int bi = -1;
    for (long long s = tid; s < ns; s += 256) {
        const double l = L[s * 2];
        if (l >= 0 && (bi < 0 || l < bl)) { bl = l; bi = (int)s; }   // ascending s: the first of equal lengths stays
    }
    sl[tid] = bl; si[tid] = bi;
    if (tid == 0) { boundI = -1; boundL = 0; count = 0; }
    __syncthreads();
    if (k <= 256) pp_kth_smallest_lds(sl, si, 256, k, &boundL, &boundI);     // the k-th smallest of the 256 minima
    __syncthreads();
    const double bL = boundL;
    const int bI = boundI;
    __syncthreads();
    if (bI < 0) {                            // fewer than k threads hold an entry (a short sample list)
        pp_k_smallest<256>(row, ns, k, oi, ol, sl, si);
        return;
    }
    // pass 2: the entries not above the bound
    for (long long s = tid; s < ns; s += 256) {
        const double l = L[s * 2];
        if (l >= 0 && !pp_pair_less(bL, bI, l, (int)s)) {
            const int slot = atomicAdd(&count, 1);
            if (slot < PP_SEL_CAP) { sl[slot] = l; si[slot] = (int)s; }
        }
    }
    __syncthreads();
    const int m = count;
    if (m > PP_SEL_CAP) {                    // uniform: the list overflowed
        __syncthreads();
        pp_k_smallest<256>(row, ns, k, oi, ol, sl, si);
        return;
    }
    // rank the survivors (at least k of them: the k minima themselves)
    for (int c = tid; c < m; c += 256) {
        const int rank = pp_rank_lds(sl, si, m, sl[c], si[c]);
        if (rank < k) { oi[rank] = si[c]; ol[rank] = sl[c]; }
    }
}

// ------------------------------------------------------------------------------------------
// The ORDER in which SamplingBasedPlanner::expand pushes the k winners of a radius (SamplingBasedPlanner.cpp:82-149): it visits
// the samples nearest-first by Euclidean distance, keeps a max-heap of the k best by approximate cost (std::push_heap, and
// std::pop_heap once the heap holds k + 1), stops once the heap is full and its worst LENGTH is not above the next distance, and
// then walks the heap ARRAY front to back.  Which vertex std::pop_heap later surfaces among children of exactly equal f depends
// on that order, so it is replayed here: one 256-thread workgroup per (vertex, radius).
//   1. candidates = valid samples (farther than the increment) with distance <= an upper bound of the k-th smallest length:
//      everything the scan can visit before it stops (a winner's distance is at most its length);
//   2. bitonic sort by (distance, sample index) in LDS;
//   3. wave 0 replays the scan with the heap held one slot per lane (parent/child moves are v_readlane and a lane-select, no memory),
//      following libstdc++'s __push_heap / __adjust_heap step for step.  A candidate whose cost is strictly above the heap's
//      root, pushed onto a full heap of pairwise distinct costs and popped again, leaves the array exactly as it was (the hole
//      sinks along the path the push shifted down and every element returns to its slot), so only the candidates at or below
//      the current root — a few dozen of the hundreds to thousands — are taken through the exact steps.
// Equal costs are handled exactly: the heap steps are libstdc++'s, and a candidate above the root is only skipped while no pair of
// equal costs sits where the pop would take another way down than the push came up (pp_ord_safe).  More than PP_ORD_CAP
// candidates (8 192 after the ring filter), k above 63, or such a pair turning up while the ring filter has dropped
// candidates fall back to ascending length and raise *fallbacks (the caller reports it).  (tests/test_gpu_expand_pieces.py: the heap
// steps and pp_ord_safe against libstdc++ on tied costs; tests/test_gpu_expand_ties.py: the pipeline on tied and crowded samples.)
#define PP_ORD_CAP 8192
struct PPOrdHeap { double cost, len; int idx; };
__device__ __forceinline__ void pp_ord_set(PPOrdHeap& h, int slot, double cost, double len, int idx) {   // slot and values are wave-uniform
    const bool mine = pp_lane() == slot;
    h.cost = mine ? cost : h.cost;
    h.len = mine ? len : h.len;
    h.idx = mine ? idx : h.idx;
}
// std::__push_heap(first, holeIndex, topIndex = 0, value, comp = cost <): the value climbs from `hole` past every ancestor whose
// cost is below it, until the first one that is not; the ancestors it passes move one step down the path.  The whole climb is made
// at once, not level by level (a read-lane / compare / move per level made an exact heap step 0.8 us, most of this kernel's time on
// a planner round trip).  Lane a is an ancestor of `hole` iff (hole + 1) >> (level difference) == a + 1;
// ancestors have smaller indices the nearer the root, so "the first ancestor, seen from the hole, that is not below the value" is
// the HIGHEST lane among the ancestors that are not below it, and the ones passed are the ancestors above that lane.
__device__ __forceinline__ void pp_ord_sift_up(PPOrdHeap& h, int hole, double cost, double len, int idx) {
    const int lane = pp_lane();
    const int lh = 31 - __clz(hole + 1), ll = 31 - __clz(lane + 1);
    const bool onPath = (ll <= lh) && (((hole + 1) >> (lh - ll)) == lane + 1);          // the hole and its ancestors
    const bool isAnc = onPath && lane != hole;
    const unsigned long long anc = __ballot(isAnc);
    const unsigned long long stays = __ballot(isAnc && !(h.cost < cost));                // `comp(first + parent, value)` false
    unsigned long long passed = anc;
    if (stays) passed &= ~((2ull << (63 - __clzll((long long)stays))) - 1ull);            // only the ancestors between the hole and the first that stays
    // every lane of the path whose parent is passed takes its parent's entry
    const int par = lane > 0 ? ((lane - 1) >> 1) : 0;
    const double pc = __shfl(h.cost, par, PP_WAVE), pl = __shfl(h.len, par, PP_WAVE);
    const int pi = __shfl(h.idx, par, PP_WAVE);
    const bool recv = onPath && lane > 0 && ((passed >> par) & 1ull) != 0ull;
    h.cost = recv ? pc : h.cost; h.len = recv ? pl : h.len; h.idx = recv ? pi : h.idx;
    const int fin = passed ? (__ffsll((long long)passed) - 1) : hole;                     // the topmost ancestor passed, or the hole itself
    pp_ord_set(h, fin, cost, len, idx);
}
// std::pop_heap on n + 1 elements: the last one is taken out as `value`, the root leaves, std::__adjust_heap(first, 0, n, value):
// the hole sinks from the root to a leaf — at every node to the larger child, the RIGHT one on equal costs, a lone left child when
// n is even — the children on that path move up one step, and the value climbs back from the leaf (__push_heap).  Every node's
// choice is made at once (two shuffles), the path is then a handful of read-lanes.
__device__ __forceinline__ void pp_ord_pop(PPOrdHeap& h, int n) {
    const int lane = pp_lane();
    const double vc = pp_readlane(h.cost, n), vl = pp_readlane(h.len, n);
    const int vi = pp_readlane_i(h.idx, n);
    const int left = 2 * lane + 1, right = 2 * lane + 2;
    const double cl = __shfl(h.cost, left < PP_WAVE ? left : 0, PP_WAVE), cr = __shfl(h.cost, right < PP_WAVE ? right : 0, PP_WAVE);
    int pick = -1;
    if (right < n) pick = (cr < cl) ? left : right;          // `if (comp(first + secondChild, first + (secondChild - 1))) secondChild--`
    else if (left < n) pick = left;                          // `(len & 1) == 0 && secondChild == (len - 2) / 2`
    unsigned long long path = 1ull;
    int bottom = 0;
    for (;;) {
        const int nx = pp_readlane_i(pick, bottom);
        if (nx < 0) break;
        path |= 1ull << nx;
        bottom = nx;
    }
    // every node of the path but the last takes the entry of the child the hole went to
    const int src = pick >= 0 ? pick : 0;
    const double sc = __shfl(h.cost, src, PP_WAVE), sl = __shfl(h.len, src, PP_WAVE);
    const int si = __shfl(h.idx, src, PP_WAVE);
    const bool recv = ((path >> lane) & 1ull) != 0ull && lane != bottom;
    h.cost = recv ? sc : h.cost; h.len = recv ? sl : h.len; h.idx = recv ? si : h.idx;
    pp_ord_sift_up(h, bottom, vc, vl, vi);
}
// Skipping a candidate above the root is only right if pushing and popping it would put every element back (see above).  The
// push shifts the ancestors of slot k down along their path and the pop's hole walks down again choosing the larger child,
// the RIGHT one on equal costs: it retraces the path unless some ancestor whose path child is its left child has a right
// child of EQUAL cost, or k is a right child whose left sibling equals their parent (then the two equal entries trade
// places).  True when no such pair exists in the full heap of k entries as it stands; that changes only when the heap does.
__device__ __forceinline__ bool pp_ord_safe(const PPOrdHeap& h, int k) {
    bool ok = true;
    for (int c = k; c > 0; c = (c - 1) >> 1) {
        const int par = (c - 1) >> 1;
        if (c & 1) { if (c + 1 < k) ok = ok && (pp_readlane(h.cost, c + 1) < pp_readlane(h.cost, par)); }
        else if (c == k) ok = ok && (pp_readlane(h.cost, k - 1) < pp_readlane(h.cost, par));
    }
    return ok;
}

// The pipeline, each step as parallel as its data allows.  Dubins lengths are solved only for the samples that can matter: the k
// winners of a (vertex, radius) are not longer than ANY k lengths one cares to compute, and a sample's Euclidean distance never
// exceeds its Dubins length — so a PROBE of the first PP_PROBE samples (the generator draws uniformly in the box, every prefix is
// spread like the whole) gives a bound Ub, and only the samples within Ub of the vertex — about a seventh of the set at the
// planner's sample counts — get their lengths.  Same winners, same push order: any upper bound of the k-th smallest length serves.
//   pp_k_expand_probe       thread per (vertex, probe sample): its lengths; per radius the minimum of every 32 consecutive probe samples;
//   pp_k_expand_near        thread per (vertex, 8 samples): Ub = the k-th smallest of the vertex's 32 group minima per radius (k different
//                           samples are not longer than it; +inf when fewer than k groups hold a valid sample, or k > 32: then every
//                           valid sample is "near" — the exhaustive path); farther than the increment (SamplingBasedPlanner.cpp:111)
//                           and within the larger of the two bounds -> the vertex's near list;
//   pp_k_near_lengths       thread per (vertex, near slot): its lengths, per 32 slots the smallest of each radius and the slots in use;
//   pp_k_expand_bound       workgroup per (vertex, radius): U = the k-th smallest of those group minima (of runs of groups when there
//                           are more than 512).  At least k samples are not longer than U, so U bounds the k-th smallest length from
//                           above, and it is nearly always equal to it (the k best samples seldom share a group).  Fewer than k near
//                           samples, or fewer than k groups with a valid one: U = +inf (the scan visits everything);
//   pp_k_expand_candidates  thread per (vertex, near slot): the samples the scan can visit — valid, distance <= U — appended to the
//                           (vertex, radius) list {distance, index, length};
//   pp_k_expand_order       workgroup per (vertex, radius): ring filter, sort by (distance, index), replay (above).
#define PP_PROBE 1024
#define PP_PROBE_GROUPS (PP_PROBE / 32)      // minima of 32 probe samples each: the k-th smallest of them bounds the k-th smallest length
#define PP_NEAR_PER 8                        // samples per thread of pp_k_expand_near (a workgroup ranks the probe minima once for 2 048 samples)
#define PP_NEAR_GROUP 32                     // near slots per ranked minimum: a half wavefront (pp_half_wave_min).  (Groups of 256 leave a
                                             // near list of a thousand samples with fewer groups than k: no bound at all.)
#define PP_BOUND_CAP 512                     // values the bound kernel ranks: group minima, merged into runs of consecutive groups when there are more
#define PP_ORD_INNER 1024                    // candidates of the inner ring whose costs set the filter threshold
// What the six kernels work on, filled by the driver (launch_expand_order): open vertices [0, nv), the sample store, the configuration
// and the workspace.  Per (vertex, radius) arrays are indexed vr = vertex * 2 + radius.
// (Laid out so that what a kernel reads sits together: the kernels are short, and every further 64-byte line of the argument block
// is one more scalar-cache miss at their start.)
struct PPExpandArgs {
    const ppgpu_vertex* verts;
    const double *sx, *sy, *sh;
    long long ns;
    double rho, rho_cov, inc_d;
    int k, two_radii;                        // two_radii = 0: radius 1 is not in use (SamplingBasedPlanner.cpp:60-63, 97-100)
    int groups_row, pad_;                    // groups per vertex groupmin / groupcnt are laid out for (only the groups of a vertex's own list are written)
    int *near_idx, *near_count;              // [nv][ns] samples within the vertex's probe bound, order arbitrary; [nv] how many
    double* lengths;                         // [nv][ns] double2 per near SLOT (not per sample)
    double* groupmin; int* groupcnt;         // [nv][groups_row][2] smallest length of a group of near slots per radius; [nv][groups_row] slots in use
    double* probe_min;                       // [nv][2][PP_PROBE_GROUPS]
    double* bound; int* cand_count;          // [nv * 2] U; length of the candidate list
    double* g_key; int* g_val; double* g_len;   // [nv * 2][g_cap] candidate lists: distance, sample, length
    long long g_cap;
    double max_speed, tpf;
    int* out_idx;                            // [nv][2][k] the winners in push order, -1 behind them
    unsigned* fallbacks;                     // lists that kept ascending length
};
// thread per (vertex, probe sample): (PP_PROBE / 256, nv) workgroups
__global__ __launch_bounds__(256) void pp_k_expand_probe(PPExpandArgs a) {
    const int v = blockIdx.y;
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    double l0 = -1, l1 = -1;
    if (s < a.ns) pp_pair_lengths(a.verts[v], a.sx[s], a.sy[s], a.sh[s], a.rho, a.rho_cov, a.inc_d, a.two_radii != 0, l0, l1);
    const double b0 = pp_half_wave_min(l0 >= 0 ? l0 : INFINITY), b1 = pp_half_wave_min(l1 >= 0 ? l1 : INFINITY);
    if ((threadIdx.x & 31) == 0) {
        const int g = (int)(blockIdx.x * 8 + (threadIdx.x >> 5));
        a.probe_min[((size_t)v * 2 + 0) * PP_PROBE_GROUPS + g] = b0;
        a.probe_min[((size_t)v * 2 + 1) * PP_PROBE_GROUPS + g] = b1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.near_count[v] = 0;
}
// the k-th smallest of a (vertex, radius)'s PP_PROBE_GROUPS group minima: +inf when fewer than k are finite.  Every lane gets the value.
__device__ __forceinline__ double pp_probe_bound(const double* probe_min, int v, int r, int k) {
    const int lane = pp_lane();
    return pp_kth_smallest_wave((lane < PP_PROBE_GROUPS) ? probe_min[((size_t)v * 2 + r) * PP_PROBE_GROUPS + lane] : INFINITY, PP_PROBE_GROUPS, k);
}
__global__ __launch_bounds__(256) void pp_k_expand_near(PPExpandArgs a) {
    __shared__ int wcount[PP_NEAR_PER * 4], wbase[PP_NEAR_PER * 4];
    __shared__ double s_Ub;
    const int v = blockIdx.y;
    if (threadIdx.x < PP_WAVE) {
        const double u = (a.k <= PP_PROBE_GROUPS) ? fmax(pp_probe_bound(a.probe_min, v, 0, a.k), pp_probe_bound(a.probe_min, v, 1, a.k)) : INFINITY;
        if (threadIdx.x == 0) s_Ub = u;
    }
    __syncthreads();
    const double Ub = s_Ub;
    const double vx = a.verts[v].x, vy = a.verts[v].y;
    const long long s0 = (long long)blockIdx.x * (256 * PP_NEAR_PER) + threadIdx.x;
    bool take[PP_NEAR_PER];
    int slot[PP_NEAR_PER];
#pragma unroll
    for (int j = 0; j < PP_NEAR_PER; j++) {
        const long long s = s0 + (long long)j * 256;
        take[j] = false;
        if (s < a.ns) {
            const double d = sqrt((vx - a.sx[s]) * (vx - a.sx[s]) + (vy - a.sy[s]) * (vy - a.sy[s]));
            take[j] = (d > a.inc_d) && !(d > Ub * (1.0 + 1e-9));
        }
    }
    pp_wg_append<PP_NEAR_PER, true>(take, a.near_count + v, wcount, wbase, slot);
#pragma unroll
    for (int j = 0; j < PP_NEAR_PER; j++)
        if (take[j]) a.near_idx[(size_t)v * (size_t)a.ns + (size_t)slot[j]] = (int)(s0 + (long long)j * 256);
}
__global__ __launch_bounds__(256) void pp_k_near_lengths(PPExpandArgs a) {
    static_assert(PP_NEAR_GROUP == 32, "pp_half_wave_min is the group minimum");
    const int v = blockIdx.y;
    const int n = a.near_count[v];
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if ((long long)blockIdx.x * 256 >= (long long)n) return;            // (whole workgroups beyond the vertex's list)
    double2 l; l.x = -1; l.y = -1;
    if (slot < n) {
        const int s = a.near_idx[(size_t)v * (size_t)a.ns + (size_t)slot];
        // (every near sample is farther than the increment: pp_k_expand_near took the same distance)
        pp_pair_lengths<true>(a.verts[v], a.sx[s], a.sy[s], a.sh[s], a.rho, a.rho_cov, a.inc_d, a.two_radii != 0, l.x, l.y);
        reinterpret_cast<double2*>(a.lengths)[(size_t)v * (size_t)a.ns + (size_t)slot] = l;
    }
    // the smallest length of every PP_NEAR_GROUP consecutive slots: what pp_k_expand_bound ranks
    const double a0 = pp_half_wave_min(l.x >= 0 ? l.x : INFINITY), a1 = pp_half_wave_min(l.y >= 0 ? l.y : INFINITY);
    if ((threadIdx.x & (PP_NEAR_GROUP - 1)) == 0) {
        const size_t b = ((size_t)v * gridDim.x + blockIdx.x) * (256 / PP_NEAR_GROUP) + (threadIdx.x / PP_NEAR_GROUP);
        a.groupmin[2 * b] = a0;
        a.groupmin[2 * b + 1] = a1;
        const long long left = (long long)n - slot;
        a.groupcnt[b] = (int)(left < PP_NEAR_GROUP ? (left > 0 ? left : 0) : PP_NEAR_GROUP);
    }
}
__global__ __launch_bounds__(256) void pp_k_expand_bound(PPExpandArgs a) {
    __shared__ double vals[PP_BOUND_CAP];
    __shared__ int valid;
    __shared__ double U;
    const int vr = blockIdx.x, v = vr >> 1, r = vr & 1;
    const int tid = (int)threadIdx.x;
    if (tid == 0) { valid = 0; U = INFINITY; a.cand_count[vr] = 0; }
    __syncthreads();
    const int ngrp = (a.near_count[v] + PP_NEAR_GROUP - 1) / PP_NEAR_GROUP;
    const int per = (ngrp + PP_BOUND_CAP - 1) / PP_BOUND_CAP;            // groups per ranked value
    const int nval = per > 0 ? (ngrp + per - 1) / per : 0;
    int c = 0;
    for (int j = tid; j < nval; j += 256) {
        double m = INFINITY;
        for (int b = j * per; b < (j + 1) * per && b < ngrp; b++) {
            m = fmin(m, a.groupmin[2 * ((size_t)v * a.groups_row + b) + r]);
            c += a.groupcnt[(size_t)v * a.groups_row + b];
        }
        vals[j] = m;
    }
    atomicAdd(&valid, c);
    __syncthreads();
    if (valid >= a.k) pp_kth_smallest_lds(vals, nullptr, nval, a.k, &U, nullptr);     // k runs hold a sample not longer than it
    __syncthreads();
    if (tid == 0) a.bound[vr] = U;
}
__global__ __launch_bounds__(256) void pp_k_expand_candidates(PPExpandArgs a) {
    __shared__ int wcount[2 * 4], wbase[2 * 4];
    const int v = blockIdx.y;
    const int n = a.near_count[v];
    if ((long long)blockIdx.x * 256 >= (long long)n) return;            // (whole workgroups beyond the vertex's near list)
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    double len[2] = {-1, -1}, d = 0;
    int s = 0;
    if (slot < n) {
        const double2 L = reinterpret_cast<const double2*>(a.lengths)[(size_t)v * (size_t)a.ns + (size_t)slot];
        len[0] = L.x; len[1] = L.y;
        s = a.near_idx[(size_t)v * (size_t)a.ns + (size_t)slot];
        const double vx = a.verts[v].x, vy = a.verts[v].y;
        d = sqrt((a.sx[s] - vx) * (a.sx[s] - vx) + (a.sy[s] - vy) * (a.sy[s] - vy));       // State::distanceTo of the sample to the source
    }
    bool take[2];
    int at[2];
#pragma unroll
    for (int r = 0; r < 2; r++) take[r] = (r == 0 || a.two_radii) && (len[r] >= 0) && !(d > a.bound[2 * v + r] * (1.0 + 1e-9));
    pp_wg_append<2, false>(take, a.cand_count + 2 * v, wcount, wbase, at);
#pragma unroll
    for (int r = 0; r < 2; r++)
        if (take[r] && at[r] < a.g_cap) {
            const size_t to = (size_t)(2 * v + r) * a.g_cap + at[r];
            a.g_key[to] = d; a.g_val[to] = s; a.g_len[to] = len[r];
        }
}

// ---- the four jobs of pp_k_expand_order, on the LDS arrays the kernel declares
struct PPOrdList { const double* key; const int* val; const double* len; int M; };   // a (vertex, radius)'s candidates: distance, sample, length
// Ring filter.  Most candidates cannot change the heap: a candidate beyond the inner ring (distance > dq = U/4, a sixteenth of the
// disc) whose cost is above the k-th smallest cost INSIDE that ring finds the heap full of k cheaper entries when its turn comes,
// whatever the order inside the ring.  Returns that cost (+inf: keep everything) and the ring's radius in dq.
__device__ __forceinline__ double pp_ord_ring_threshold(const PPOrdList& L, int k, double max_speed, double tpf, double& dq, double* inner,
                                                        int* nInner, double* threshold) {
    const int tid = (int)threadIdx.x;
    int n = 0;
    for (int attempt = 0; attempt < 12; attempt++) {
        for (int i = tid; i < L.M; i += 256)
            if (L.key[i] <= dq) {
                const int slot = atomicAdd(nInner, 1);
                if (slot < PP_ORD_INNER) inner[slot] = pp_approx_cost(L.len[i], max_speed, tpf);
            }
        __syncthreads();
        n = *nInner;
        if (n <= PP_ORD_INNER) break;
        // a crowded ring (tens of thousands of samples under a loose bound): any ring with at least k candidates will do,
        // halving the radius leaves about a quarter of them
        __syncthreads();
        if (tid == 0) *nInner = 0;
        dq *= 0.5;
        __syncthreads();
    }
    if (n >= k && n <= PP_ORD_INNER) pp_kth_smallest_lds(inner, nullptr, n, k, threshold, nullptr);
    __syncthreads();
    return *threshold;
}
// Keep: the ring and the cheaper candidates outside it (a few hundred of thousands) -> cd (distance), ci (position in the list; the
// lengths stay in the list in memory and are fetched by position when the replay gets there).  Returns how many; beyond PP_ORD_CAP
// they were not stored.
__device__ __forceinline__ int pp_ord_keep(const PPOrdList& L, double dq, double T, double max_speed, double tpf, double* cd, int* ci, int* nKept) {
    for (int i = (int)threadIdx.x; i < L.M; i += 256) {
        const double d = L.key[i];
        if (d <= dq || !(pp_approx_cost(L.len[i], max_speed, tpf) > T)) {
            const int slot = atomicAdd(nKept, 1);
            if (slot < PP_ORD_CAP) { cd[slot] = d; ci[slot] = i; }
        }
    }
    __syncthreads();
    return *nKept;
}
// Bitonic sort of the Mk kept candidates by (distance, sample index): list positions are not in sample order, so equal distances
// compare their samples.
__device__ __forceinline__ void pp_ord_sort(const PPOrdList& L, int Mk, double* cd, int* ci) {
    const int tid = (int)threadIdx.x;
    int n2 = 64;
    while (n2 < Mk) n2 <<= 1;
    for (int i = Mk + tid; i < n2; i += 256) { cd[i] = INFINITY; ci[i] = 0x7fffffff; }
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (n2 >> 1); t += 256) {
                const int i = ((t / stride) * stride << 1) + (t % stride), j = i + stride;
                const double ki = cd[i], kj = cd[j];
                const int vi = ci[i], vj = ci[j];
                bool gt = ki > kj;
                if (ki == kj) gt = (vi == 0x7fffffff) ? (vj != 0x7fffffff) : (vj != 0x7fffffff && L.val[vi] > L.val[vj]);
                if (gt == ((i & size) == 0)) { cd[i] = kj; cd[j] = ki; ci[i] = vj; ci[j] = vi; }
            }
        }
    __syncthreads();
}
// The replay, by one wavefront: the heap array -> h, one slot per lane.  unsafeFiltered: the list has to fall back (see below).
struct PPOrdReplay { int hsize, nexact; bool unsafeFiltered; };      // entries in the heap; candidates taken through the exact steps (PP_DBG_ORD)
__device__ __forceinline__ PPOrdReplay pp_ord_replay(const PPOrdList& L, int Mk, int k, double max_speed, double tpf, const double* cd, const int* ci,
                                                     PPOrdHeap& h) {
    const int lane = pp_lane();
    int hsize = 0, nexact = 0;
    bool unsafeFiltered = false, stopped = false;
    bool safe = true, anyEqual = false;                                 // pp_ord_safe of the heap as it stands
    for (int base = 0; base < Mk && !stopped && !unsafeFiltered; base += PP_WAVE) {
        const int c = base + lane;
        const bool have = c < Mk;
        const double d = have ? cd[c] : INFINITY;
        const int pos = have ? ci[c] : 0;                           // position in the candidate list
        const double len = have ? L.len[pos] : INFINITY;
        const int idx = have ? L.val[pos] : -1;
        const double cost = pp_approx_cost(len, max_speed, tpf);
        // the candidates of this chunk that can change the heap: every one while it is not full (or not `safe`), afterwards
        // those at or below the root's cost as it stands at the start of the chunk (the root only ever gets cheaper)
        unsigned long long rest = __ballot(have);
        const unsigned long long low = __ballot(have & (cost <= pp_readlane(h.cost, 0)));
        if (hsize >= k && safe && low == 0ull) {
            // nobody enters the heap; the scan still ends at the first distance the worst kept length does not exceed
            if (__ballot(have & !(pp_readlane(h.len, 0) > d)) != 0ull) stopped = true;
            continue;
        }
        while (true) {
            const unsigned long long cand = (hsize < k || !safe) ? rest : (rest & low);
            if (!cand) break;
            const int j = __ffsll((long long)cand) - 1;
            rest &= ~((2ull << j) - 1ull);                          // j and the candidates before it (no-ops in this state) are done
            const double dj = pp_readlane(d, j), lj = pp_readlane(len, j), cj = pp_readlane(cost, j);
            const int ij = pp_readlane_i(idx, j);
            if (hsize >= k) {
                if (!(pp_readlane(h.len, 0) > dj)) { stopped = true; break; }        // :104-106, else branch :130-132
                if (safe && cj > pp_readlane(h.cost, 0)) continue;                    // the root moved since the chunk began: a no-op
            }
            nexact++;
            // equal costs are what can make the heap unsafe: until one has been pushed onto an equal entry there is nothing to check
            anyEqual = anyEqual || (__ballot((lane < hsize) & (h.cost == cj)) != 0ull);
            pp_ord_sift_up(h, hsize, cj, lj, ij);                                     // push_back + std::push_heap
            hsize++;
            if (hsize > k) { hsize--; pp_ord_pop(h, hsize); }                         // std::pop_heap + pop_back
            if (hsize >= k && anyEqual) {
                safe = pp_ord_safe(h, k);
                // the ring filter dropped candidates on the strength of "a no-op whenever its turn comes": not in this state
                if (!safe && Mk < L.M) { unsafeFiltered = true; break; }
            }
        }
    }
    return PPOrdReplay{hsize, nexact, unsafeFiltered};
}
// Fallback: what a plain selection gives, the k cheapest of the list ascending by (length, sample); only the push order is lost.
__device__ __forceinline__ void pp_ord_fallback(const PPExpandArgs& a, const PPOrdList& L, int vr, double U, double* cd, int* ci, int* nKept, int* out) {
    const int tid = (int)threadIdx.x, v = vr >> 1;
    if (tid == 0) atomicAdd(a.fallbacks, 1u);
    // More candidates within the bound than the list holds (M > g_cap: slots beyond it were dropped in the order the atomics
    // happened to arrive): the truncated list is not a set anyone can name, so the selection runs over the vertex's whole near
    // list instead (every sample within the probe bound, which is not below U: nothing that can win is missing from it)
    const bool fullRow = (long long)L.M > a.g_cap;
    const long long Mc = fullRow ? (long long)a.near_count[v] : (long long)L.M;
    const double* row = a.lengths + (size_t)v * (size_t)a.ns * 2 + (vr & 1);
    const int* rowIdx = a.near_idx + (size_t)v * (size_t)a.ns;
    const auto lenOf = [=](long long c) { return fullRow ? row[2 * c] : L.len[c]; };
    const auto idxOf = [=](long long c) { return fullRow ? rowIdx[c] : L.val[c]; };
    // ONE pass by the whole workgroup, not k (k passes over a late-mission round trip's 2.5 million samples overran the planner's
    // deadline).  U, the k-th smallest group minimum of this row, bounds the k-th smallest length from above, and every sample not
    // longer than U is in the list when the list is whole (its distance is at most its length): the winners are among the entries
    // with length <= U — usually a few dozen — which go to LDS and are selected there.
    __syncthreads();
    if (tid == 0) *nKept = 0;
    __syncthreads();
    for (long long c = tid; c < Mc; c += 256) {
        const double l = lenOf(c);
        if (!(l >= 0) || l > U) continue;
        const int slot = atomicAdd(nKept, 1);
        if (slot < PP_ORD_CAP) { cd[slot] = l; ci[slot] = idxOf(c); }
    }
    __syncthreads();
    const int Ms = *nKept;
    if (Ms <= PP_ORD_CAP) {
        if (tid < PP_WAVE) pp_k_smallest<PP_WAVE>([=](long long c, double& l, int& i) { l = cd[c]; i = ci[c]; return true; }, Ms, a.k, out, nullptr, nullptr, nullptr);
        return;
    }
    // more than PP_ORD_CAP entries within U (thousands of exactly equal lengths): k successive minimum scans of the source, by the
    // whole workgroup (cd / ci as the reduction's scratch)
    pp_k_smallest<256>([=](long long c, double& l, int& i) { l = lenOf(c); i = idxOf(c); return l >= 0; }, Mc, a.k, out, nullptr, cd, ci);
}
__global__ __launch_bounds__(256) void pp_k_expand_order(PPExpandArgs a) {
    __shared__ double cd[PP_ORD_CAP];        // 96 KB of the CU's 160 KB LDS
    __shared__ int ci[PP_ORD_CAP];
    __shared__ double inner[PP_ORD_INNER];
    __shared__ int nInner, nKept, fallbackVerdict;
    __shared__ double threshold;
    const int vr = blockIdx.x, tid = (int)threadIdx.x, k = a.k;
    int* out = a.out_idx + (size_t)vr * k;
    const PPOrdList L = {a.g_key + (size_t)vr * a.g_cap, a.g_val + (size_t)vr * a.g_cap, a.g_len + (size_t)vr * a.g_cap, a.cand_count[vr]};
    if (((vr & 1) && !a.two_radii) || L.M <= 0) {            // radius not in use (:60-63,97-100), or no sample farther than the increment
        for (int j = tid; j < k; j += 256) out[j] = -1;
        return;
    }
    bool fallback = k >= PP_WAVE || (long long)L.M > a.g_cap;     // the heap holds k + 1 entries for a moment, one per lane
    const double U = a.bound[vr];
    if (tid == 0) { nInner = 0; nKept = 0; threshold = INFINITY; }
    __syncthreads();
#ifdef PP_DBG_ORD
    const long long tk0 = wall_clock64();
#endif
    double dq = 0.25 * U;
    const double T = (!fallback && (U < INFINITY) && L.M > 512) ? pp_ord_ring_threshold(L, k, a.max_speed, a.tpf, dq, inner, &nInner, &threshold) : INFINITY;
#ifdef PP_DBG_ORD
    const long long tk1 = wall_clock64();
#endif
    const int Mk = fallback ? 0 : pp_ord_keep(L, dq, T, a.max_speed, a.tpf, cd, ci, &nKept);
#ifdef PP_DBG_ORD
    const long long tk2 = wall_clock64();
#endif
    fallback = fallback || Mk > PP_ORD_CAP;
    if (!fallback) pp_ord_sort(L, Mk, cd, ci);
#ifdef PP_DBG_ORD
    const long long tk3 = wall_clock64();
#endif
    // wave 0 replays; the other waves wait for its verdict: a list that has to fall back is selected by the whole workgroup
    PPOrdHeap h = {INFINITY, INFINITY, -1};
    PPOrdReplay rp = {0, 0, false};
    if (!fallback && tid < PP_WAVE) rp = pp_ord_replay(L, Mk, k, a.max_speed, a.tpf, cd, ci, h);
#ifdef PP_DBG_ORD
    if (pp_lane() == 0 && vr < 4) printf("[ord] vr %d M %d inner %d kept %d exact %d | filter %lld keep %lld sort %lld replay %lld (x10ns)\n", vr, L.M, nInner, Mk, rp.nexact, tk1 - tk0, tk2 - tk1, tk3 - tk2, wall_clock64() - tk3);
#endif
    if (tid == 0) fallbackVerdict = (fallback || rp.unsafeFiltered) ? 1 : 0;
    __syncthreads();
    if (!fallbackVerdict) {
        if (tid < PP_WAVE && tid < k) out[tid] = (tid < rp.hsize) ? h.idx : -1;      // the heap array, front to back
        return;
    }
#ifdef PP_DBG_ORD
    if (tid == 0) printf("[ord] FALLBACK vr %d: k %d M %d cap %lld kept %d unsafeFiltered %d hsize %d | U %g dq %g inner %d threshold %g\n", vr, k, L.M, a.g_cap, Mk, (int)rp.unsafeFiltered, rp.hsize, U, dq, nInner, threshold);
#endif
    pp_ord_fallback(a, L, vr, U, cd, ci, &nKept, out);
}

// ------------------------------------------------------------------------------------------
// The upload block of ppgpu_expand_host, one copy: {vertices | ribbons | explicit target x, y, heading per vertex | has-target
// flags}, as byte offsets.  Everything is 8-byte words except the flags, one byte per vertex at the end.
struct PPExpandBlock {
    size_t verts, ribbons, x, y, heading, flags, bytes;
    __host__ __device__ PPExpandBlock(int nv, int n_ribbons) {
        verts = 0;
        ribbons = verts + (size_t)nv * sizeof(ppgpu_vertex);
        x = ribbons + (size_t)n_ribbons * 4 * sizeof(double);
        y = x + (size_t)nv * sizeof(double);
        heading = y + (size_t)nv * sizeof(double);
        flags = heading + (size_t)nv * sizeof(double);
        bytes = flags + (size_t)nv;
    }
};
// Puts the block's parts where the other kernels expect them (vertex array, ribbon pool, the slots behind the stored samples, flags).
__global__ __launch_bounds__(256) void pp_k_expand_unpack(const unsigned char* blk, int nv, int n_ribbons, ppgpu_vertex* verts, double* ribbons,
                                                        double* ex, double* ey, double* eh, unsigned char* flags, unsigned* zero_word) {
    typedef unsigned long long word;
    const PPExpandBlock B(nv, n_ribbons);
    const size_t words = B.flags / 8;
    if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0u;      // the push-order fallback counter of this round trip
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words + (size_t)nv; i += (size_t)gridDim.x * 256) {
        const size_t at = i * 8;
        if (i >= words) flags[i - words] = blk[B.flags + (i - words)];
        else if (at < B.ribbons) ((word*)verts)[i] = ((const word*)blk)[i];
        else if (at < B.x) ((word*)ribbons)[(at - B.ribbons) / 8] = ((const word*)blk)[i];
        else if (at < B.y) ((word*)ex)[(at - B.x) / 8] = ((const word*)blk)[i];
        else if (at < B.heading) ((word*)ey)[(at - B.y) / 8] = ((const word*)blk)[i];
        else ((word*)eh)[(at - B.heading) / 8] = ((const word*)blk)[i];
    }
}

// ------------------------------------------------------------------------------------------
// The edge list of SamplingBasedPlanner::expand for every open vertex, in its push order (see ppgpu_expand_host): E slots
// per vertex, unused slots hold an all-ones descriptor (vertex index out of range: the costing kernels skip it).
__global__ __launch_bounds__(64) void pp_k_build_expand_edges(int nverts, int k, const int* nearest_idx /* [nv][2][k] */, const unsigned char* has_extra,
                                                             long long first_extra, int two_speeds, int two_radii, int E,
                                                             unsigned long long* edges, const unsigned* fallbacks, unsigned long long* header) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    // (the push-order fallback count of this round trip travels home in the block's header: one download instead of two)
    if (v == 0 && header) header[0] = fallbacks ? (unsigned long long)*fallbacks : 0ull;
    if (v >= nverts) return;
    unsigned long long* out = edges + (size_t)v * E;
    int n = 0;
    const int nsp = two_speeds ? 2 : 1, nrad = two_radii ? 2 : 1;
    // coverageAllowed = (radius == coverageTurningRadius): with one radius that single radius IS the coverage radius
    if (has_extra[v]) {
        for (int si = 0; si < nsp; si++)
            for (int ri = 0; ri < nrad; ri++) {
                const unsigned cov = (two_radii ? ri == 1 : 1) ? PPGPU_EDGE_COVERAGE : 0u;
                out[n++] = ((unsigned long long)(cov | (si == 1 ? PPGPU_EDGE_SLOW : 0u)) << 56) | ((unsigned long long)v << 32) |
                           (unsigned long long)(unsigned)(first_extra + v);
            }
    }
    if (nearest_idx) {
        for (int ri = 0; ri < nrad; ri++) {
            const unsigned cov = (two_radii ? ri == 1 : 1) ? PPGPU_EDGE_COVERAGE : 0u;
            const int slot = (ri == 1) ? 1 : 0;           // slot 1 of the selection is always the coverage radius
            for (int j = 0; j < k; j++) {
                const int s = nearest_idx[((size_t)v * 2 + slot) * k + j];
                if (s < 0) break;
                for (int si = 0; si < nsp; si++)
                    out[n++] = ((unsigned long long)(cov | (si == 1 ? PPGPU_EDGE_SLOW : 0u)) << 56) | ((unsigned long long)v << 32) |
                               (unsigned long long)(unsigned)s;
            }
        }
    }
    for (; n < E; n++) out[n] = ~0ull;
}
