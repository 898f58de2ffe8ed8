// pp_k_keepout.h — pp_k_keepout_bits: the effective grid of a keep-out margin (ppgpu.h, "chart clearance"): the distance map
// (pp_k_distance.h) thresholded into the packed bit grid every kernel reads through PPGrid::bits.  Included by pp_kernels.h.
#pragma once
// Cell (r, c) is blocked in the effective grid iff gap2(r, c) < limit2.  The caller passes limit2 >= 1, so a cell blocked in the
// grid as set (gap2 0) stays blocked, and the band along the grid's border comes with the map: the outside is a hazard in gap2.
// One workgroup per row and tile of 256 columns, one thread per cell: a wave reads 128 contiguous bytes of the map, its ballot is
// the two words of its 64 cells, and lanes 0 and 32 store one each.  A lane past `cols` contributes 0 (the padding bits of a row's
// last word stay zero) and a word past `wpr` is not written.  No lane leaves before the ballot.
__global__ __launch_bounds__(256) void pp_k_keepout_bits(const uint16_t* dist, int rows, int cols, int wpr, unsigned limit2, uint32_t* bits) {
    const int r = (int)blockIdx.x, c = (int)blockIdx.y * 256 + (int)threadIdx.x;
    const bool blocked = r < rows && c < cols && (unsigned)dist[(size_t)r * cols + c] < limit2;
    const unsigned long long m = __ballot(blocked);
    const int w = c >> 5;
    if ((c & 31) == 0 && r < rows && w < wpr) bits[(size_t)r * wpr + w] = (uint32_t)(m >> (c & 32));
}
