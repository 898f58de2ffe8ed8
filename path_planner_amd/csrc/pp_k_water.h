// pp_k_water.h — distance by water (ppgpu.h, "distance by water"): the cost of the cheapest 8-connected path through the free cells of
// the effective grid from a seed's cell to every cell (a row or column step PPGPU_WATER_STEP, a diagonal step PPGPU_WATER_DIAG) as one
// uint32_t per cell, the totals of that map, the look-up of points in it, and the walk of a ribbon's sample points over it.
// Included by pp_kernels.h (after pp_k_reach.h: pp_reach_free, PP_UF_LOAD, and pp_k_clearance_trace.h: pp_pack_i32).
#pragma once
// The map: single-source shortest paths by chaotic relaxation, one launch per round, and no workgroup waits for another inside one.
//   pp_k_water_round   one 1 024-thread workgroup per tile of PP_WATER_TILE x PP_WATER_TILE cells, thread = cell.  A tile whose dirty flag
//                      of this round is clear leaves at once.  A dirty tile clears its flag, loads its cells and the ring of cells
//                      around them into LDS (a cell outside the grid is NONE; a blocked cell holds NONE in the map already), relaxes
//                      its own cells to a fixed point there, stores those that fell, raises the NEXT round's flag of every
//                      neighbouring tile that touches one of them, and counts itself in the round's word of active tiles.
//   pp_k_water_totals  the cells with a distance, and the largest distance with the lowest row-major index that attains it.
// Why any order gives the same bytes.  A value in the map or in LDS is NONE or the cost of an actual path from the seed, and it is only
// ever replaced by a smaller one.  Only the workgroup of a cell's tile writes it; a neighbour reads it as part of its ring with a
// plain load, which may return the value from before a store of the same launch: an older, larger path cost, never a wrong one.  The
// owner that stored it has raised the reader's flag for the next round, and the kernel boundary between the rounds makes the store
// visible there, so the reader meets the new value then.  A round in which no tile was dirty therefore leaves every tile at its own
// fixed point against the final ring: the map is the fixed point of the relaxation, which is the exact minimum (every path cost is a
// sum of at most rows * cols - 1 steps of 12 or 17: the host has checked that it fits).  How many rounds that takes may differ from
// build to build (a ring read may or may not have seen a store of the same round); the bytes do not.
//   Inside a tile the sweeps are chaotic in the same way: a thread reads its eight neighbours (relaxed workgroup-scope loads: other
// waves store to them in the same sweep) and lowers its own cell; the sweep in which no thread lowered anything read only final
// values.  A cheapest path inside the window has at most 1 023 steps, so that sweep comes within PP_WATER_TILE^2 + 1 sweeps: the cap,
// which raises the sticky error word PP_WW_ERROR (it cannot).
#define PP_WATER_TILE PPGPU_WATER_TILE
#define PP_WATER_SIDE (PP_WATER_TILE + 2)
static_assert(PP_WATER_TILE == 32, "thread = cell: a tile is one 1 024-thread workgroup, a tile row is half a wave");
static_assert(PPGPU_WATER_STEP < PPGPU_WATER_DIAG && PPGPU_WATER_DIAG < 2 * PPGPU_WATER_STEP, "a diagonal step beats two straight ones and no straight one");
// the words the map's kernels leave for the host (one 64-byte block, zeroed before a build)
enum { PP_WW_WET = 0, PP_WW_FARTHEST, PP_WW_ERROR, PP_WW_COUNT = 8 };

#define PP_WATER_ST(p, v, SCOPE) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, SCOPE)
__device__ __forceinline__ unsigned pp_water_step(unsigned from, unsigned cost) { return from == PPGPU_WATER_NONE ? PPGPU_WATER_NONE : from + cost; }

// After the map was filled with NONE and the flags with 0: distance 0 on the seed's cell, and round 0's flag of the seed's tile and of
// the tiles around it (the seed's cell does not fall in round 0, so nobody would raise them for a seed on a tile's border).  One wave.
__global__ __launch_bounds__(64) void pp_k_water_seed(uint32_t* wd, unsigned seed_cell, int cols, int tiles_x, int tiles_y, uint32_t* flags_now) {
    const int lane = (int)threadIdx.x;
    if (lane == 0) wd[seed_cell] = 0u;
    if (lane < 9) {
        const int ty = (int)(seed_cell / (unsigned)cols) / PP_WATER_TILE + lane / 3 - 1, tx = (int)(seed_cell % (unsigned)cols) / PP_WATER_TILE + lane % 3 - 1;
        if (ty >= 0 && ty < tiles_y && tx >= 0 && tx < tiles_x) flags_now[(size_t)ty * tiles_x + tx] = 1u;
    }
}

// grid = (tiles across, tiles down), 1024 threads.  flags_now / flags_next: one word per tile, row-major over the tiles; `active`:
// this round's word.
__global__ __launch_bounds__(PP_WATER_TILE * PP_WATER_TILE) void pp_k_water_round(const uint32_t* bits, int rows, int cols, int wpr, uint32_t* wd,
                                                                                  uint32_t* flags_now, uint32_t* flags_next, unsigned* active,
                                                                                  unsigned long long* words) {
    __shared__ unsigned s_wd[PP_WATER_SIDE * PP_WATER_SIDE];       // [1 + lr][1 + lc]; the ring is rows and columns 0 and 33
    __shared__ unsigned s_touch;                                   // bit (dy + 1) * 3 + (dx + 1): a cell beside the tile at (dy, dx) fell
    const int tx = (int)gridDim.x, tile = (int)blockIdx.y * tx + (int)blockIdx.x;
    if (flags_now[tile] == 0u) return;                             // (the whole workgroup: one word, written by no one in this launch but us)
    const int tid = (int)threadIdx.x, lc = tid & 31, lr = tid >> 5;
    const int r0 = (int)blockIdx.y * PP_WATER_TILE, c0 = (int)blockIdx.x * PP_WATER_TILE;
    const int r = r0 + lr, c = c0 + lc;
    const bool free = pp_reach_free(bits, rows, cols, wpr, r, c);  // (false outside the grid)
    const unsigned was = free ? wd[(size_t)r * cols + c] : PPGPU_WATER_NONE;
    const int me = (1 + lr) * PP_WATER_SIDE + 1 + lc;
    s_wd[me] = was;
    if (tid < 4 * PP_WATER_TILE + 4) {                             // the ring: 34 above, 34 below, 32 to the left, 32 to the right
        int hr, hc;
        if (tid < 2 * PP_WATER_SIDE) { hr = tid < PP_WATER_SIDE ? -1 : PP_WATER_TILE; hc = tid % PP_WATER_SIDE - 1; }
        else { const int k = tid - 2 * PP_WATER_SIDE; hr = k & 31; hc = k < PP_WATER_TILE ? -1 : PP_WATER_TILE; }
        const int gr = r0 + hr, gc = c0 + hc;
        unsigned v = PPGPU_WATER_NONE;
        if (gr >= 0 && gr < rows && gc >= 0 && gc < cols) v = PP_UF_LOAD(wd + (size_t)gr * cols + gc, __HIP_MEMORY_SCOPE_AGENT);
        s_wd[(1 + hr) * PP_WATER_SIDE + 1 + hc] = v;
    }
    if (tid == 0) s_touch = 0u;
    __syncthreads();
    if (tid == 0) flags_now[tile] = 0u;                            // (after the barrier: every wave has read it)
    unsigned mine = was;
    bool overrun = true;
    for (int sweep = 0; sweep < PP_WATER_TILE * PP_WATER_TILE + 1; sweep++) {
        int changed = 0;
        if (free) {
#define PP_WATER_AT(dr, dc) PP_UF_LOAD(s_wd + me + (dr) * PP_WATER_SIDE + (dc), __HIP_MEMORY_SCOPE_WORKGROUP)
            const unsigned straight = min(min(PP_WATER_AT(-1, 0), PP_WATER_AT(1, 0)), min(PP_WATER_AT(0, -1), PP_WATER_AT(0, 1)));
            const unsigned diag = min(min(PP_WATER_AT(-1, -1), PP_WATER_AT(-1, 1)), min(PP_WATER_AT(1, -1), PP_WATER_AT(1, 1)));
#undef PP_WATER_AT
            const unsigned best = min(pp_water_step(straight, PPGPU_WATER_STEP), pp_water_step(diag, PPGPU_WATER_DIAG));
            if (best < mine) {
                mine = best;
                PP_WATER_ST(s_wd + me, best, __HIP_MEMORY_SCOPE_WORKGROUP);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) { overrun = false; break; }
    }
    if (mine < was) {                                              // (free, inside the grid)
        PP_WATER_ST(wd + (size_t)r * cols + c, mine, __HIP_MEMORY_SCOPE_AGENT);
        const int dy = lr == 0 ? -1 : (lr == PP_WATER_TILE - 1 ? 1 : 0), dx = lc == 0 ? -1 : (lc == PP_WATER_TILE - 1 ? 1 : 0);
        unsigned touch = 0u;
        if (dy) touch |= 1u << ((dy + 1) * 3 + 1);
        if (dx) touch |= 1u << (3 + dx + 1);
        if (dy && dx) touch |= 1u << ((dy + 1) * 3 + dx + 1);
        if (touch) atomicOr(&s_touch, touch);
    }
    __syncthreads();
    if (tid < 9 && tid != 4 && ((s_touch >> tid) & 1u)) {
        const int ty = (int)blockIdx.y + tid / 3 - 1, tx2 = (int)blockIdx.x + tid % 3 - 1;
        if (ty >= 0 && ty < (int)gridDim.y && tx2 >= 0 && tx2 < tx) PP_WATER_ST(flags_next + (size_t)ty * tx + tx2, 1u, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) {
        atomicAdd(active, 1u);
        if (overrun) atomicMax(words + PP_WW_ERROR, 1ull);
    }
}

// One thread per cell.  The key of a wet cell is (wd << 32) | ~index: the largest key is the largest distance at the lowest index.
// One ballot per wave for the count, one wave reduction of the keys, one atomic per workgroup and word.
__global__ __launch_bounds__(256) void pp_k_water_totals(const uint32_t* wd, long long ncell, unsigned long long* words) {
    __shared__ unsigned s_count;
    __shared__ unsigned long long s_key[4];
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned v = i < ncell ? wd[i] : PPGPU_WATER_NONE;
    const bool wet = v != PPGPU_WATER_NONE;
    unsigned long long key = wet ? (((unsigned long long)v << 32) | (unsigned long long)(~(unsigned)i)) : 0ull;   // (0: below every wet key)
    const unsigned long long m = __ballot(wet);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, o, PP_WAVE);
        key = other > key ? other : key;
    }
    if (pp_lane() == 0) {
        s_key[threadIdx.x >> 6] = key;
        if (m) atomicAdd(&s_count, (unsigned)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count) {
        unsigned long long k = s_key[0];
        for (int w = 1; w < 4; w++) k = s_key[w] > k ? s_key[w] : k;
        atomicAdd(words + PP_WW_WET, (unsigned long long)s_count);
        atomicMax(words + PP_WW_FARTHEST, k);                      // (a wet cell's key is above 0: its index is below 2^32 - 1)
    }
}

// ppgpu_water_distance_at: n > 0 points {x, y}; the cell is the one Map::isBlocked puts the point in (pp_cell_of: it holds a __ballot,
// so a thread past the end redoes the last point and stores nothing).  Outside the grid: NONE.
__global__ __launch_bounds__(256) void pp_k_water_distance_at(PPGrid g, const uint32_t* wd, long long n, const double* xy, double* metres, unsigned* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long j = i < n ? i : n - 1;
    const PPCell cell = pp_cell_of(g, xy[2 * j], xy[2 * j + 1]);
    unsigned v = PPGPU_WATER_NONE;
    if (!cell.outside) v = wd[(size_t)cell.r * g.cols + cell.c];
    if (i >= n) return;
    if (metres) metres[i] = v == PPGPU_WATER_NONE ? (double)INFINITY : g.res * (double)v / (double)PPGPU_WATER_STEP;
    if (out) out[i] = v;
}

// The ribbon walk: one wave per ribbon, lanes stride over the samples 0 .. n of {sx, sy, ex, ey, len, n} exactly as pp_k_reach_ribbons
// places them.  A sample in cell A takes ad(A) = min of wd(B) over the cells B of the grid with gap2(A, B) < lim2: the lane walks the
// window |dr|, |dc| <= reach itself (reach = the largest d with (d - 1)^2 < lim2, from the host; at most 32).  Neighbouring lanes hold
// neighbouring samples, so their windows are the same cache lines.  The extremes are wave reductions of 64-bit keys that carry the
// sample index: (ad << 32) | k for the smallest (the lowest index wins a tie), (ad << 32) | ~k for the largest (likewise).
// The record leaves as four 16-byte pieces, one per lane of lanes 0-3:
// {length, pitch} {samples | wet_samples, nearest | farthest} {min_ad | max_ad, start_ad | end_ad} {lim2 | flags, nearest_metres}.
#define PP_WATER_WPB 4
static_assert(sizeof(ppgpu_ribbon_water_record) == 64, "a ribbon water record is 64 bytes: four 16-byte stores");
__global__ __launch_bounds__(PP_WATER_WPB * 64) void pp_k_water_ribbons(PPGrid g, const uint32_t* wd, int n_ribbons, const double* ribbons6, unsigned lim2, int reach,
                                                                        ppgpu_ribbon_water_record* recs) {
    const int lane = pp_lane();
    const int rib = (int)blockIdx.x * PP_WATER_WPB + (int)(threadIdx.x >> 6);
    if (rib >= n_ribbons) return;                                  // (the whole wave)
    const double* q = ribbons6 + (size_t)rib * 6;
    const double sx = q[0], sy = q[1], dx = q[2] - q[0], dy = q[3] - q[1], len = q[4], nd = q[5];
    const bool degenerate = len == 0.0;
    const int n = (int)nd, samples = degenerate ? 1 : n + 1;
    const double w = (double)g.cols * g.res, h = (double)g.rows * g.res;
    unsigned wet = 0, start_ad = PPGPU_WATER_NONE, end_ad = PPGPU_WATER_NONE;
    unsigned long long lo = ~0ull, hi = 0ull;                      // (a wet sample's keys lie strictly between)
    for (int base = 0; base < samples; base += PP_WAVE) {
        const bool valid = base + lane < samples;
        const int k = valid ? base + lane : samples - 1;
        const double t = (double)k / nd;
        double x = sx + dx * t, y = sy + dy * t;
        x = x < 0.0 ? 0.0 : (x > w ? w : x);
        y = y < 0.0 ? 0.0 : (y > h ? h : y);
        const PPCell cell = pp_cell_of(g, x, y);
        const int r = (int)min(cell.r, (unsigned)g.rows - 1u), c = (int)min(cell.c, (unsigned)g.cols - 1u);
        unsigned ad = PPGPU_WATER_NONE;
        const int rlo = max(r - reach, 0), rhi = min(r + reach, g.rows - 1), clo = max(c - reach, 0), chi = min(c + reach, g.cols - 1);
        for (int rr = rlo; rr <= rhi; rr++) {
            const unsigned gr = (unsigned)max(abs(rr - r) - 1, 0), gr2 = gr * gr;
            if (gr2 >= lim2) continue;
            const uint32_t* row = wd + (size_t)rr * g.cols;
            for (int cc = clo; cc <= chi; cc++) {
                const unsigned gc = (unsigned)max(abs(cc - c) - 1, 0);
                if (gr2 + gc * gc < lim2) ad = min(ad, row[cc]);
            }
        }
        const bool is_wet = valid && ad != PPGPU_WATER_NONE;
        if (is_wet) {
            const unsigned long long klo = ((unsigned long long)ad << 32) | (unsigned long long)(unsigned)k;
            const unsigned long long khi = (((unsigned long long)ad << 32) | (unsigned long long)(~(unsigned)k));
            lo = klo < lo ? klo : lo;
            hi = khi > hi ? khi : hi;
        }
        wet += (unsigned)__popcll(__ballot(is_wet));
        if (base == 0) start_ad = (unsigned)__shfl((int)ad, 0, PP_WAVE);
        if (base + PP_WAVE >= samples) end_ad = (unsigned)__shfl((int)ad, samples - 1 - base, PP_WAVE);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long olo = (unsigned long long)__shfl_xor((long long)lo, o, PP_WAVE), ohi = (unsigned long long)__shfl_xor((long long)hi, o, PP_WAVE);
        lo = olo < lo ? olo : lo;
        hi = ohi > hi ? ohi : hi;
    }
    unsigned min_ad = PPGPU_WATER_NONE, max_ad = PPGPU_WATER_NONE;
    int nearest = -1, farthest = -1;
    if (wet) {
        min_ad = (unsigned)(lo >> 32); nearest = (int)(unsigned)lo;
        max_ad = (unsigned)(hi >> 32); farthest = (int)(~(unsigned)hi);
    }
    const double pitch = degenerate ? 0.0 : len / nd;
    const double metres = wet ? g.res * (double)min_ad / (double)PPGPU_WATER_STEP : (double)INFINITY;
    const unsigned flags = (wet < (unsigned)samples ? PPGPU_RW_ANY_DRY : 0u) | (wet == 0u ? PPGPU_RW_WHOLE_DRY : 0u) | (degenerate ? PPGPU_RW_DEGENERATE : 0u);
    double2 piece = make_double2(len, pitch);
    if (lane == 1) piece = make_double2(pp_pack_i32((unsigned)samples, wet), pp_pack_i32((unsigned)nearest, (unsigned)farthest));
    if (lane == 2) piece = make_double2(pp_pack_i32(min_ad, max_ad), pp_pack_i32(start_ad, end_ad));
    if (lane == 3) piece = make_double2(pp_pack_i32(lim2, flags), metres);
    if (lane < 4) reinterpret_cast<double2*>(recs + rib)[lane] = piece;
}
