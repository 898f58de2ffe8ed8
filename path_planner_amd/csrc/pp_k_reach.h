// pp_k_reach.h — reachable water (ppgpu.h, "reachable water"): the 8-connected components of the free cells of the effective grid as
// canonical labels (the smallest row-major index of the component), the cells that carry a seed's label as a bit grid, and the
// walk of a ribbon's sample points over the reach-gap map built from those bits (pp_k_distance.h without the outside as a source).
// Included by pp_kernels.h.
#pragma once
// Labelling: three launches whatever the grid holds, and no workgroup waits for another inside one.
//   pp_k_reach_tiles    one workgroup per tile of PP_REACH_TILE x PP_REACH_TILE cells labels its tile in LDS by union-find and writes
//                       label[cell] = the global index of the smallest cell of the cell's component WITHIN the tile.
//   pp_k_reach_merge    one thread per cell of a tile's first row or first column unites it with its free neighbours across the
//                       border, by union-find over `label` itself: the larger root is hung under the smaller with an atomicMin.
//   pp_k_reach_flatten  every free cell walks to its root and stores it, and the free cells and the roots are counted.
// label[x] <= x always, and only an atomicMin (or the flatten's store of an ancestor) ever writes a label that is read in the same
// launch: a walk x -> label[x] -> ... strictly decreases until it meets a cell that is its own label, so it ends within rows * cols
// steps even when a read returns an older parent (parents only decrease: an old parent is still an ancestor).  In pp_uf_union the
// larger of the two roots strictly decreases from one pass to the next (a failed atomicMin hands back a parent below it), so the
// loop ends too.  Both loops carry a cap all the same and raise the sticky error word PP_RW_ERROR when they run into it.
//   Which pairs are united: two free cells next to each other in a row belong to one run; a cell is united with the cell above it
// unless both have a free cell to their left that the same rule unites (one union per pair of touching runs' first contact, and
// the runs carry the rest); with a diagonal neighbour only when the two cells between them are blocked (otherwise one of those
// connects the pair through a row step and a column step).  The tile kernel applies this to neighbours inside the tile, with a
// row run's first cell as every cell's first label; the merge kernel applies it to neighbours in another tile, where "to the
// left" ("above", along a tile's first column) stops at the tile's corner.
#define PP_REACH_TILE PPGPU_REACH_TILE
static_assert(PP_REACH_TILE == 32, "a tile row is one 32-bit word of run arithmetic, a wave's ballot is two tile rows");
// the words the labelling and the reach set leave for the host (one 64-byte block, zeroed before the launches that add to it)
enum { PP_RW_FREE = 0, PP_RW_COMPONENTS, PP_RW_REACHABLE, PP_RW_ERROR, PP_RW_COUNT = 8 };

#define PP_UF_LOAD(p, SCOPE) __hip_atomic_load((p), __ATOMIC_RELAXED, SCOPE)
// the root of x's tree; `cap` walks at most
template <int SCOPE>
__device__ __forceinline__ unsigned pp_uf_find(unsigned* L, unsigned x, unsigned cap, bool& overrun) {
    for (unsigned i = 0; i < cap; i++) {
        const unsigned p = PP_UF_LOAD(L + x, SCOPE);
        if (p >= x) return x;                       // (p == x: a root.  p > x cannot be: the walk ends all the same)
        x = p;
    }
    overrun = true;
    return x;
}
// a and b end in one tree: the larger root is hung under the smaller.  An atomicMin that did not find the root it expected (another
// thread hung it elsewhere meanwhile: `old`) has replaced or kept a parent; either way a ~ old ~ b must still be joined, so the loop
// goes on with old.
template <int SCOPE>
__device__ __forceinline__ void pp_uf_union(unsigned* L, unsigned a, unsigned b, unsigned cap, bool& overrun) {
    for (unsigned i = 0; i < cap; i++) {
        a = pp_uf_find<SCOPE>(L, a, cap, overrun);
        b = pp_uf_find<SCOPE>(L, b, cap, overrun);
        if (a == b || overrun) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
    overrun = true;
}

__device__ __forceinline__ bool pp_reach_free(const uint32_t* bits, int rows, int cols, int wpr, int r, int c) {
    if (r < 0 || r >= rows || c < 0 || c >= cols) return false;
    return !((bits[(size_t)r * wpr + (c >> 5)] >> (c & 31)) & 1u);
}

// grid = (tiles across, tiles down), 1024 threads: thread = cell (lr, lc) of the tile.  A cell of the tile outside the grid is blocked.
__global__ __launch_bounds__(PP_REACH_TILE * PP_REACH_TILE) void pp_k_reach_tiles(const uint32_t* bits, int rows, int cols, int wpr, uint32_t* label,
                                                                                  unsigned long long* words) {
    __shared__ unsigned s_free[PP_REACH_TILE + 2];                 // [1 + lr]: the free cells of tile row lr; rows -1 and 32 are blocked
    __shared__ unsigned s_lab[PP_REACH_TILE * PP_REACH_TILE];
    const int tid = (int)threadIdx.x, lc = tid & 31, lr = tid >> 5;
    const int r = (int)blockIdx.y * PP_REACH_TILE + lr, c = (int)blockIdx.x * PP_REACH_TILE + lc;
    const bool free = pp_reach_free(bits, rows, cols, wpr, r, c);
    const unsigned long long m = __ballot(free);                   // a wave is two tile rows
    if (lc == 0) s_free[1 + lr] = (uint32_t)(m >> ((lr & 1) * 32));
    if (tid == 0) { s_free[0] = 0u; s_free[PP_REACH_TILE + 1] = 0u; }
    // every cell starts as the first cell of its row run: the cells of a run are united without a union
    const unsigned row = (uint32_t)(m >> ((lr & 1) * 32));
    const unsigned blocked_before = ~row & ((1u << lc) - 1u);
    const int start = blocked_before ? 32 - __clz((int)blocked_before) : 0;
    s_lab[tid] = (unsigned)(lr * PP_REACH_TILE + start);
    __syncthreads();
    bool overrun = false;
    if (free) {
        const unsigned above = s_free[lr];                         // row lr - 1
        const bool fN = (above >> lc) & 1u, fW = lc > 0 && ((row >> (lc - 1)) & 1u), fE = lc < 31 && ((row >> (lc + 1)) & 1u);
        const bool fNW = lc > 0 && ((above >> (lc - 1)) & 1u), fNE = lc < 31 && ((above >> (lc + 1)) & 1u);
        const unsigned cap = PP_REACH_TILE * PP_REACH_TILE + 1;
        if (fN) {
            if (!(fW && fNW)) pp_uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, (unsigned)tid, (unsigned)(tid - PP_REACH_TILE), cap, overrun);
        } else {
            if (fNW && !fW) pp_uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, (unsigned)tid, (unsigned)(tid - PP_REACH_TILE - 1), cap, overrun);
            if (fNE && !fE) pp_uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, (unsigned)tid, (unsigned)(tid - PP_REACH_TILE + 1), cap, overrun);
        }
    }
    __syncthreads();
    if (r < rows && c < cols) {
        unsigned out = PPGPU_REACH_NONE;
        if (free) {
            const unsigned root = pp_uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, (unsigned)tid, PP_REACH_TILE * PP_REACH_TILE + 1, overrun);
            // row-major order inside the tile is row-major order in the grid: the tile's smallest cell is the grid's smallest
            out = (unsigned)((size_t)((int)blockIdx.y * PP_REACH_TILE + (int)(root >> 5)) * cols + (size_t)((int)blockIdx.x * PP_REACH_TILE + (int)(root & 31u)));
        }
        label[(size_t)r * cols + c] = out;
    }
    if (overrun) atomicMax(words + PP_RW_ERROR, 1ull);
}

// One thread per cell of the rows k * T (k >= 1: `hcells` of them, row by row) and then of the columns k * T (column by column).
// Every access to `label` is an agent-scope atomic: other workgroups write the same words in this launch.
__global__ __launch_bounds__(256) void pp_k_reach_merge(const uint32_t* bits, int rows, int cols, int wpr, uint32_t* label, long long hcells, long long total,
                                                        unsigned long long* words) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const unsigned cap = (unsigned)((long long)rows * cols) + 1u;          // rows * cols < 2^32 - 1 (checked by the host)
    bool overrun = false;
#define PP_REACH_FREE(rr, cc) pp_reach_free(bits, rows, cols, wpr, (rr), (cc))
#define PP_REACH_UNITE(rr, cc) pp_uf_union<__HIP_MEMORY_SCOPE_AGENT>(label, a, (unsigned)((size_t)(rr) * cols + (cc)), cap, overrun)
    if (i < hcells) {                                                      // first row of a tile: the neighbours in the row above
        const int r = (int)(i / cols + 1) * PP_REACH_TILE, c = (int)(i % cols);
        if (!PP_REACH_FREE(r, c)) return;
        const unsigned a = (unsigned)((size_t)r * cols + c);
        const bool fN = PP_REACH_FREE(r - 1, c), fW = PP_REACH_FREE(r, c - 1), fE = PP_REACH_FREE(r, c + 1);
        const bool fNW = PP_REACH_FREE(r - 1, c - 1), fNE = PP_REACH_FREE(r - 1, c + 1);
        if (fN) {
            if (!((c % PP_REACH_TILE) != 0 && fW && fNW)) PP_REACH_UNITE(r - 1, c);
        } else {
            if (fNW && !fW) PP_REACH_UNITE(r - 1, c - 1);
            if (fNE && !fE) PP_REACH_UNITE(r - 1, c + 1);
        }
    } else {                                                               // first column of a tile: the neighbours in the column to the left
        const long long j = i - hcells;
        const int c = (int)(j / rows + 1) * PP_REACH_TILE, r = (int)(j % rows);
        if (!PP_REACH_FREE(r, c)) return;
        const unsigned a = (unsigned)((size_t)r * cols + c);
        const bool fW = PP_REACH_FREE(r, c - 1), fN = PP_REACH_FREE(r - 1, c), fS = PP_REACH_FREE(r + 1, c);
        const bool fNW = PP_REACH_FREE(r - 1, c - 1), fSW = PP_REACH_FREE(r + 1, c - 1);
        if (fW) {
            if (!((r % PP_REACH_TILE) != 0 && fN && fNW)) PP_REACH_UNITE(r, c - 1);
        } else {
            if (fNW && !fN) PP_REACH_UNITE(r - 1, c - 1);
            if (fSW && !fS) PP_REACH_UNITE(r + 1, c - 1);
        }
    }
#undef PP_REACH_FREE
#undef PP_REACH_UNITE
    if (overrun) atomicMax(words + PP_RW_ERROR, 1ull);
}

// One thread per cell.  A cell's store replaces its parent by its root, an ancestor: a walk of another workgroup through it stays a
// walk towards the same root.  Free cells and roots: one ballot per wave, one atomic per workgroup and counter.
__global__ __launch_bounds__(256) void pp_k_reach_flatten(uint32_t* label, long long ncell, unsigned long long* words) {
    __shared__ unsigned s_count[2];
    if (threadIdx.x < 2) s_count[threadIdx.x] = 0u;
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool free = false, root = false, overrun = false;
    if (i < ncell) {
        const unsigned l = PP_UF_LOAD(label + i, __HIP_MEMORY_SCOPE_AGENT);
        if (l != PPGPU_REACH_NONE) {
            free = true;
            const unsigned top = pp_uf_find<__HIP_MEMORY_SCOPE_AGENT>(label, (unsigned)i, (unsigned)ncell + 1u, overrun);
            root = top == (unsigned)i;
            if (top != l) __hip_atomic_store(label + i, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const unsigned long long mf = __ballot(free), mr = __ballot(root);
    if (pp_lane() == 0) {
        if (mf) atomicAdd(&s_count[0], (unsigned)__popcll(mf));
        if (mr) atomicAdd(&s_count[1], (unsigned)__popcll(mr));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count[0]) atomicAdd(words + PP_RW_FREE, (unsigned long long)s_count[0]);
    if (threadIdx.x == 1 && s_count[1]) atomicAdd(words + PP_RW_COMPONENTS, (unsigned long long)s_count[1]);
    if (overrun) atomicMax(words + PP_RW_ERROR, 1ull);
}

// The cells that carry the seed's label as a bit grid of PPGrid's layout, and their number: pp_k_keepout_bits' shape (one workgroup per
// row and tile of 256 columns, a wave's ballot is the two words of its 64 cells, padding bits zero, no lane leaves before the ballot).
__global__ __launch_bounds__(256) void pp_k_reach_bits(const uint32_t* label, int rows, int cols, int wpr, unsigned seed_label, uint32_t* bits,
                                                       unsigned long long* words) {
    __shared__ unsigned s_count;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    const int r = (int)blockIdx.x, c = (int)blockIdx.y * 256 + (int)threadIdx.x;
    const bool reach = r < rows && c < cols && seed_label != PPGPU_REACH_NONE && label[(size_t)r * cols + c] == seed_label;   // (a blocked seed: no cell)
    const unsigned long long m = __ballot(reach);
    const int w = c >> 5;
    if ((c & 31) == 0 && r < rows && w < wpr) bits[(size_t)r * wpr + w] = (uint32_t)(m >> (c & 32));
    if (pp_lane() == 0 && m) atomicAdd(&s_count, (unsigned)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(words + PP_RW_REACHABLE, (unsigned long long)s_count);
}

// The ribbon walk: one wave per ribbon, lanes stride over the samples 0 .. n of {sx, sy, ex, ey, len, n} (len and n from the host:
// ppgpu.h states the rule).  A sample is clamped into the grid's rectangle and its cell is the one pp_cell_of puts it in, held to
// the last row and column; it is OUT iff the reach gap of that cell is at least lim2.  pp_cell_of holds a __ballot: a lane past the
// last sample redoes the last one and contributes nothing.  The record leaves as four 16-byte pieces, one per lane of lanes 0-3:
// {length, pitch} {samples | out_samples, first_out | last_out} {min_rgap2 | max_rgap2, lim2 | flags} {out_length, reserved}.
#define PP_REACH_WPB 4
static_assert(sizeof(ppgpu_ribbon_reach_record) == 64, "a ribbon reach record is 64 bytes: four 16-byte stores");
__global__ __launch_bounds__(PP_REACH_WPB * 64) void pp_k_reach_ribbons(PPGrid g, const uint16_t* rgap, int n_ribbons, const double* ribbons6, unsigned lim2,
                                                                        ppgpu_ribbon_reach_record* recs) {
    const int lane = pp_lane();
    const int rib = (int)blockIdx.x * PP_REACH_WPB + (int)(threadIdx.x >> 6);
    if (rib >= n_ribbons) return;                                  // (the whole wave)
    const double* q = ribbons6 + (size_t)rib * 6;
    const double sx = q[0], sy = q[1], dx = q[2] - q[0], dy = q[3] - q[1], len = q[4], nd = q[5];
    const bool degenerate = len == 0.0;
    const int n = (int)nd, samples = degenerate ? 1 : n + 1;
    const double w = (double)g.cols * g.res, h = (double)g.rows * g.res;
    unsigned outs = 0, lo = 0xFFFFFFFFu, hi = 0u;
    int first = -1, last = -1;
    for (int base = 0; base < samples; base += PP_WAVE) {
        const bool valid = base + lane < samples;
        const int k = valid ? base + lane : samples - 1;
        const double t = (double)k / nd;
        double x = sx + dx * t, y = sy + dy * t;
        x = x < 0.0 ? 0.0 : (x > w ? w : x);
        y = y < 0.0 ? 0.0 : (y > h ? h : y);
        const PPCell cell = pp_cell_of(g, x, y);
        const unsigned r = min(cell.r, (unsigned)g.rows - 1u), c = min(cell.c, (unsigned)g.cols - 1u);
        const unsigned g2 = rgap[(size_t)r * g.cols + c];
        if (valid) { lo = min(lo, g2); hi = max(hi, g2); }
        const unsigned long long out = __ballot(valid && g2 >= lim2);
        if (out != 0ull) {
            if (first < 0) first = base + __ffsll(out) - 1;
            last = base + 63 - __clzll((long long)out);
            outs += (unsigned)__popcll(out);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o, PP_WAVE));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o, PP_WAVE));
    }
    const double pitch = degenerate ? 0.0 : len / nd;
    const double out_len = fmin(pitch * (double)outs, len);
    const unsigned flags = (outs ? PPGPU_RB_ANY_OUT : 0u) | (outs == (unsigned)samples ? PPGPU_RB_WHOLE_OUT : 0u) | (first == 0 ? PPGPU_RB_START_OUT : 0u) |
                           (last == samples - 1 ? PPGPU_RB_END_OUT : 0u) | (degenerate ? PPGPU_RB_DEGENERATE : 0u) | (hi == PPGPU_DIST_CAP2 ? PPGPU_RB_CAPPED : 0u);
    double2 piece = make_double2(len, pitch);
    if (lane == 1) piece = make_double2(pp_pack_i32((unsigned)samples, outs), pp_pack_i32((unsigned)first, (unsigned)last));
    if (lane == 2) piece = make_double2(pp_pack_i32(lo, hi), pp_pack_i32(lim2, flags));
    if (lane == 3) piece = make_double2(out_len, 0.0);
    if (lane < 4) reinterpret_cast<double2*>(recs + rib)[lane] = piece;
}
