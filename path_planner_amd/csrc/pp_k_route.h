// pp_k_route.h — route by water (ppgpu.h, "route by water"): the step map of the water map (one byte per cell: the code of the step towards
// the seed) and the walk of one route per query point over it, with its record and its vertices.
// Included by pp_kernels.h (after pp_k_water.h: PP_WW_ERROR, PP_WATER_WPB, and pp_k_clearance_trace.h: pp_pack_i32).
#pragma once
// Codes 0 .. 7 = N, S, W, E, NW, NE, SW, SE.  The opposite of a straight code flips its lowest bit; of a diagonal code k it is 11 - k.
__device__ __forceinline__ int pp_route_dr(unsigned k) { return k < 4u ? (k == 0u ? -1 : (k == 1u ? 1 : 0)) : (k < 6u ? -1 : 1); }
__device__ __forceinline__ int pp_route_dc(unsigned k) { return k < 4u ? (k == 2u ? -1 : (k == 3u ? 1 : 0)) : ((k & 1u) ? 1 : -1); }
__device__ __forceinline__ unsigned pp_route_opposite(unsigned k) { return k < 4u ? (k ^ 1u) : 11u - k; }

// One thread per cell: the lowest code whose neighbour is in the grid, has a distance and lies exactly one step's cost nearer the seed.
// Only the seed's cell has distance 0 (every step costs something).  A thread past the last cell stores nothing.
__global__ __launch_bounds__(256) void pp_k_water_dirs(const uint32_t* wd, int rows, int cols, long long ncell, uint8_t* dirs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ncell) return;
    const unsigned v = wd[i];
    unsigned code = PPGPU_ROUTE_NONE;
    if (v == 0u) code = PPGPU_ROUTE_SEED;
    else if (v != PPGPU_WATER_NONE) {
        const int r = (int)(i / cols), c = (int)(i % cols);
#pragma unroll
        for (int k = 7; k >= 0; k--) {                             // (downwards: the lowest code that fits is the last one kept)
            const int nr = r + pp_route_dr((unsigned)k), nc = c + pp_route_dc((unsigned)k);
            if (nr < 0 || nr >= rows || nc < 0 || nc >= cols) continue;
            const unsigned w = wd[(size_t)nr * cols + nc];
            if (w != PPGPU_WATER_NONE && w + (k < 4 ? (unsigned)PPGPU_WATER_STEP : (unsigned)PPGPU_WATER_DIAG) == v) code = (unsigned)k;
        }
    }
    dirs[i] = (uint8_t)code;
}

// What one walk from B to the seed leaves: wave-uniform.
struct PPRouteWalk {
    unsigned straight, diagonal, turns, last_code;                 // last_code: the code of the step that arrived on the seed's cell
    unsigned long long narrow;                                     // (gap2 << 32) | ~(steps from B): the smallest gap2, the cell nearest the seed on a tie
    unsigned narrow_cell;
    bool overrun;
};

// The walk, pos and the code k wave-uniform: lane i looks at the cell i steps ahead along k; the leading lanes whose dir is k are a run
// taken at once; the lane after the run holds the dir of the cell the run arrives on (the cell before it points at it, so it is in
// the grid).  After 64 matches the arrival cell's dir is loaded on its own.  STORE: turn number t of the walk goes to slot
// vertices - 2 - t of `out` when that is below the stride.  At most `bound` rounds; each takes at least one step.
template <bool STORE>
__device__ __forceinline__ PPRouteWalk pp_route_walk(const uint8_t* dirs, const uint16_t* dist, int rows, int cols, unsigned from, unsigned bound, unsigned vertices,
                                                     unsigned stride, uint32_t* out) {
    const int lane = pp_lane();
    PPRouteWalk w;
    w.straight = w.diagonal = w.turns = 0u;
    w.last_code = PPGPU_ROUTE_SEED;
    w.narrow = ~0ull; w.narrow_cell = PPGPU_WATER_NONE;
    w.overrun = false;
    int r = (int)(from / (unsigned)cols), c = (int)(from % (unsigned)cols);
    unsigned k = dirs[from], steps = 0u;
    bool arrived = k == PPGPU_ROUTE_SEED;
    for (unsigned round = 0; !arrived; round++) {
        if (round >= bound || k > 7u) { w.overrun = true; break; }
        const int dr = pp_route_dr(k), dc = pp_route_dc(k);
        const int lr = r + lane * dr, lc = c + lane * dc;
        const bool inside = lr >= 0 && lr < rows && lc >= 0 && lc < cols;
        const size_t at = inside ? (size_t)lr * cols + lc : (size_t)0;
        const unsigned d = inside ? (unsigned)dirs[at] : PPGPU_ROUTE_NONE;
        const unsigned long long match = __ballot(inside && d == k);
        const int run = ~match == 0ull ? 64 : (int)__builtin_ctzll(~match);
        if (run == 0) { w.overrun = true; break; }                 // (lane 0 is pos, whose dir is k)
        if (!STORE) {
            unsigned long long key = ~0ull;
            unsigned cell = PPGPU_WATER_NONE;
            if (lane < run) { key = ((unsigned long long)dist[at] << 32) | (unsigned long long)(~(steps + (unsigned)lane)); cell = (unsigned)at; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long okey = (unsigned long long)__shfl_xor((long long)key, o, PP_WAVE);
                const unsigned ocell = (unsigned)__shfl_xor((int)cell, o, PP_WAVE);
                if (okey < key) { key = okey; cell = ocell; }
            }
            if (key < w.narrow) { w.narrow = key; w.narrow_cell = cell; }
        }
        if (k < 4u) w.straight += (unsigned)run; else w.diagonal += (unsigned)run;
        steps += (unsigned)run;
        r += run * dr; c += run * dc;
        const unsigned here = (unsigned)r * (unsigned)cols + (unsigned)c;
        const unsigned next = run < 64 ? (unsigned)__shfl((int)d, run, PP_WAVE) : (unsigned)dirs[here];
        if (next == PPGPU_ROUTE_SEED) { w.last_code = k; arrived = true; }
        else if (next != k) {                                      // a turn (a code above 7 ends the walk at the top of the next round)
            if (STORE) {
                const unsigned slot = vertices - 2u - w.turns;
                if (lane == 0 && slot < stride) out[slot] = here;
            }
            w.turns++;
            k = next;
        }
    }
    if (!STORE && !w.overrun) {                                    // the seed's cell: the last cell of the route
        const unsigned here = (unsigned)r * (unsigned)cols + (unsigned)c;
        const unsigned long long key = ((unsigned long long)dist[here] << 32) | (unsigned long long)(~steps);
        if (key < w.narrow) { w.narrow = key; w.narrow_cell = here; }
    }
    return w;
}

// One wave per route.  The approach cell: lanes stride over the window |dr|, |dc| <= reach of A (reach from the host, as for
// pp_k_water_ribbons) with the key (wd << 32) | index; the smallest key is the smallest wd at the lowest index.  Then the walk twice: the
// first counts (the vertices are numbered from the seed, and their number is only known at the end), the second stores the turns.  The
// record leaves as four 16-byte pieces, one per lane of lanes 0-3:
// {point_cell | from_cell, wd | lim2} {straight | diagonal, turns | vertices} {written | first_dir, min_gap2 | its cell} {metres, narrowest}.
static_assert(sizeof(ppgpu_water_route_record) == 64, "a water route record is 64 bytes: four 16-byte stores");
__global__ __launch_bounds__(PP_WATER_WPB * 64) void pp_k_water_routes(PPGrid g, const uint32_t* wd, const uint8_t* dirs, const uint16_t* dist, long long n,
                                                                       const double* xy, unsigned seed_cell, unsigned lim2, int reach, unsigned stride,
                                                                       ppgpu_water_route_record* recs, uint32_t* vertices, unsigned long long* words) {
    const int lane = pp_lane();
    const long long route = (long long)blockIdx.x * PP_WATER_WPB + (long long)(threadIdx.x >> 6);
    if (route >= n) return;                                        // (the whole wave)
    const PPCell cell = pp_cell_of(g, xy[2 * route], xy[2 * route + 1]);
    unsigned flags = 0u, a_cell = PPGPU_WATER_NONE, from = PPGPU_WATER_NONE, dist_b = PPGPU_WATER_NONE;
    if (cell.outside) flags = PPGPU_WR_DRY | PPGPU_WR_OUTSIDE;
    else {
        const int r = (int)cell.r, c = (int)cell.c;
        a_cell = (unsigned)r * (unsigned)g.cols + (unsigned)c;
        unsigned long long key = ~0ull;
        if (lim2 == 0u) key = ((unsigned long long)wd[a_cell] << 32) | (unsigned long long)a_cell;
        else {
            const int side = 2 * reach + 1;
            for (int t = lane; t < side * side; t += PP_WAVE) {
                const int rr = r + t / side - reach, cc = c + t % side - reach;
                if (rr < 0 || rr >= g.rows || cc < 0 || cc >= g.cols) continue;
                const unsigned gr = (unsigned)max(abs(rr - r) - 1, 0), gc = (unsigned)max(abs(cc - c) - 1, 0);
                if (gr * gr + gc * gc >= lim2) continue;
                const unsigned at = (unsigned)rr * (unsigned)g.cols + (unsigned)cc;
                const unsigned long long mine = ((unsigned long long)wd[at] << 32) | (unsigned long long)at;
                key = mine < key ? mine : key;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, o, PP_WAVE);
                key = other < key ? other : key;
            }
        }
        dist_b = (unsigned)(key >> 32);
        if (dist_b == PPGPU_WATER_NONE) flags = PPGPU_WR_DRY;
        else from = (unsigned)key;
    }
    unsigned straight = 0u, diagonal = 0u, turns = 0u, count = 0u, written = 0u, code = PPGPU_ROUTE_NONE, gap = PPGPU_WATER_NONE, gap_cell = PPGPU_WATER_NONE;
    double metres = (double)INFINITY, narrowest = (double)INFINITY;
    if (from != PPGPU_WATER_NONE) {
        const unsigned bound = dist_b / (unsigned)PPGPU_WATER_STEP + 2u;
        uint32_t* out = vertices + (size_t)route * stride;         // (not touched with stride 0)
        const PPRouteWalk w = pp_route_walk<false>(dirs, dist, g.rows, g.cols, from, bound, 0u, 0u, out);
        if (w.overrun) { if (lane == 0) atomicMax(words + PP_WW_ERROR, 1ull); }
        else {
            straight = w.straight; diagonal = w.diagonal; turns = w.turns;
            const bool at_seed = dist_b == 0u;
            count = at_seed ? 1u : turns + 2u;
            written = min(count, stride);
            code = at_seed ? PPGPU_ROUTE_SEED : pp_route_opposite(w.last_code);
            gap = (unsigned)(w.narrow >> 32);
            gap_cell = w.narrow_cell;
            if (at_seed) flags |= PPGPU_WR_AT_SEED;
            if (count > stride) flags |= PPGPU_WR_TRUNCATED;
            if (stride > 0u) {                                     // seed first, the turns (second walk), B last
                if (!at_seed && turns > 0u) (void)pp_route_walk<true>(dirs, dist, g.rows, g.cols, from, bound, count, stride, out);
                if (lane == 0) {
                    out[0] = seed_cell;
                    if (count - 1u < stride) out[count - 1u] = from;
                }
            }
            metres = g.res * ((double)straight + (double)diagonal * sqrt(2.0));
            narrowest = g.res * sqrt((double)gap);
        }
    }
    double2 piece = make_double2(pp_pack_i32(a_cell, from), pp_pack_i32(from == PPGPU_WATER_NONE ? PPGPU_WATER_NONE : dist_b, lim2));
    if (lane == 1) piece = make_double2(pp_pack_i32(straight, diagonal), pp_pack_i32(turns, count));
    if (lane == 2) piece = make_double2(pp_pack_i32(written, code | (flags << 8)), pp_pack_i32(gap, gap_cell));
    if (lane == 3) piece = make_double2(metres, narrowest);
    if (lane < 4) reinterpret_cast<double2*>(recs + route)[lane] = piece;
}
