// pp_k_distance.h — the distance map of the occupancy grid: min(gap2, PPGPU_DIST_CAP2) per cell as uint16_t (ppgpu.h, "chart
// clearance": the squared distance in cells between the nearest edges of a cell and of the nearest cell that is blocked or
// outside the grid), and the lookup of a pose in it.  Included by pp_kernels.h.
#pragma once
// Not PPGrid::clearance (pp_k_common.h): that map is a chessboard distance capped at 64, built with every grid to cull chunks.  This
// one is Euclidean, exact in integers, and built only when a clearance call asks for it.  With g(d) = max(|d| - 1, 0) monotone in
// |d|, the minimum of g(dr)^2 + g(dc)^2 over the hazard cells of one column is attained at the column's nearest hazard cell, so
//     v(r, c)    = centre distance in rows from (r, c) to the nearest hazard cell of column c; rows -1 and `rows` are hazards
//     gap2(r, c) = min over dc of g(dc)^2 + g(v(r, c + dc))^2, with v = 0 in the columns outside the grid
// i.e. the plain squared Euclidean distance transform of the hazard set dilated by one cell, in two separable passes.
#define PP_DIST_VCAP (PPGPU_DIST_CAP + 1)   // v is capped here: g(256)^2 is the cap of the map, nothing farther can matter
#define PP_DIST_TILE 32                     // rows per thread of the column pass (their hazard bits fill one register)
static_assert(PPGPU_DIST_CAP * PPGPU_DIST_CAP == PPGPU_DIST_CAP2 && PPGPU_DIST_CAP2 <= 0xFFFF, "the capped map fits uint16_t");
static_assert(PP_DIST_VCAP % 8 == 0, "pp_dist_scan looks at eight rows at a time");

// OUTSIDE_IS_HAZARD: the chart's map, as described above.  Without it the rows and columns outside the grid hold no source: the map of
// the distance to a set of cells alone (the reach gap of pp_k_reach.h), v = PP_DIST_VCAP in the columns outside.
template <bool OUTSIDE_IS_HAZARD>
__device__ __forceinline__ bool pp_dist_hazard(const uint32_t* bits, int rows, int wpr, int r, int c) {
    if (r < 0 || r >= rows) return OUTSIDE_IS_HAZARD;
    return (bits[(size_t)r * wpr + (c >> 5)] >> (c & 31)) & 1u;
}
// min(PP_DIST_VCAP, the smallest d >= 1 with a hazard at row from + dir * d): eight rows' words are on their way before the first
// is looked at (one row at a time the walk is a chain of dependent load latencies)
template <bool OUTSIDE_IS_HAZARD>
__device__ __forceinline__ int pp_dist_scan(const uint32_t* bits, int rows, int wpr, int from, int dir, int c) {
    for (int d0 = 1; d0 <= PP_DIST_VCAP; d0 += 8) {
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) m |= (pp_dist_hazard<OUTSIDE_IS_HAZARD>(bits, rows, wpr, from + dir * (d0 + j), c) ? 1u : 0u) << j;
        if (m) return d0 + __ffs((int)m) - 1;
    }
    return PP_DIST_VCAP;
}

// Column pass.  One thread per column and tile of PP_DIST_TILE rows; adjacent lanes take adjacent columns, so a wave reads one or
// two words of a row and writes 128 contiguous bytes of v per row (lanes striding across rows would touch 64 lines per access).
// The thread finds the nearest hazard above its tile, walks down, finds the nearest below, walks back up.
template <bool OUTSIDE_IS_HAZARD>
__global__ __launch_bounds__(256) void pp_k_dist_cols(const uint32_t* bits, int rows, int cols, int wpr, uint16_t* v) {
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c >= cols) return;
    const int r0 = (int)blockIdx.y * PP_DIST_TILE;
    const int nr = (rows - r0) < PP_DIST_TILE ? (rows - r0) : PP_DIST_TILE;
    unsigned hazard = 0;
    for (int i = 0; i < nr; i++) hazard |= (pp_dist_hazard<OUTSIDE_IS_HAZARD>(bits, rows, wpr, r0 + i, c) ? 1u : 0u) << i;
    uint16_t* col = v + (size_t)r0 * cols + c;
    int d = pp_dist_scan<OUTSIDE_IS_HAZARD>(bits, rows, wpr, r0, -1, c) - 1;                   // what row r0 - 1 would hold
    for (int i = 0; i < nr; i++) {
        d = ((hazard >> i) & 1u) ? 0 : min(d + 1, PP_DIST_VCAP);
        col[(size_t)i * cols] = (uint16_t)d;
    }
    d = pp_dist_scan<OUTSIDE_IS_HAZARD>(bits, rows, wpr, r0 + nr - 1, +1, c) - 1;              // what row r0 + nr would hold
    for (int i = nr - 1; i >= 0; i--) {
        d = ((hazard >> i) & 1u) ? 0 : min(d + 1, PP_DIST_VCAP);
        const int down = col[(size_t)i * cols];
        if (d < down) col[(size_t)i * cols] = (uint16_t)d;
    }
}

// Row pass.  One workgroup per row and tile of 256 columns: the tile's v and the PP_DIST_VCAP columns on either side of it (0 outside
// the grid where the outside is a hazard) are staged in LDS, 1.5 KB whatever the grid's width.  Each thread walks outwards from its own column and leaves once
// g(dc)^2 alone reaches its best: at most PPGPU_DIST_CAP steps, on an empty grid.
template <bool OUTSIDE_IS_HAZARD>
__global__ __launch_bounds__(256) void pp_k_dist_rows(const uint16_t* v, int rows, int cols, uint16_t* dist) {
    __shared__ uint16_t s_v[256 + 2 * PP_DIST_VCAP];
    const int r = (int)blockIdx.x, c0 = (int)blockIdx.y * 256;
    const uint16_t* row = v + (size_t)r * cols;
    for (int j = (int)threadIdx.x; j < 256 + 2 * PP_DIST_VCAP; j += 256) {
        const int cc = c0 - PP_DIST_VCAP + j;
        s_v[j] = (cc >= 0 && cc < cols) ? row[cc] : (uint16_t)(OUTSIDE_IS_HAZARD ? 0 : PP_DIST_VCAP);
    }
    __syncthreads();
    const int c = c0 + (int)threadIdx.x;
    if (c >= cols) return;
    const int i = PP_DIST_VCAP + (int)threadIdx.x;
    const int g0 = max((int)s_v[i] - 1, 0);
    unsigned best = (unsigned)(g0 * g0);                                    // <= PPGPU_DIST_CAP2: v is capped
    for (int dc = 1; dc <= PPGPU_DIST_CAP; dc++) {
        const unsigned gd2 = (unsigned)((dc - 1) * (dc - 1));
        if (gd2 >= best) break;
        const int gv = max(min((int)s_v[i - dc], (int)s_v[i + dc]) - 1, 0);
        best = min(best, gd2 + (unsigned)(gv * gv));
    }
    dist[(size_t)r * cols + c] = (uint16_t)best;
}

// gap2 of the cell pp_blocked_cell puts the pose in (the cell arithmetic of pp_is_blocked, stated once): 0 outside the grid.  All
// lanes of the wave must be here (pp_blocked_cell holds a __ballot).  inv_wpr = 1.0 / g.wpr: the cell's row comes back out of its
// word's index, a multiple of wpr below 2^52, so the product is within 2^-21 of the row and truncates to it.
__device__ __forceinline__ unsigned pp_pose_gap2(const PPGrid& g, const uint16_t* dist, double inv_wpr, double x, double y) {
    const PPCellRef ref = pp_blocked_cell(g, x, y);
    unsigned gap2 = 0;
    if (!ref.outside) {
        const unsigned r = (unsigned)((double)(unsigned long long)(ref.word - (ref.col >> 5)) * inv_wpr + 0.5);
        gap2 = dist[(size_t)r * g.cols + ref.col];
    }
    return gap2;
}

// ppgpu_grid_clearance_at: n > 0 points {x, y}; a thread past the end redoes the last point and stores nothing
__global__ __launch_bounds__(256) void pp_k_grid_clearance_at(PPGrid g, const uint16_t* dist, long long n, const double* xy, double* clearance, unsigned* gap2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long j = i < n ? i : n - 1;
    const unsigned g2 = pp_pose_gap2(g, dist, 1.0 / (double)g.wpr, xy[2 * j], xy[2 * j + 1]);
    if (i >= n) return;
    if (clearance) clearance[i] = g.res * sqrt((double)g2);
    if (gap2) gap2[i] = g2;
}
