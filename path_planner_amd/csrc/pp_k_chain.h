// pp_k_chain.h — chained costing of multi-leg plans (ppgpu_cost_plans_host): pp_k_chain_advance turns the record a plan's leg of
// depth d was costed into, into the open vertex its leg of depth d + 1 starts from, without leaving the device — what the host loop
// of AStarPlanner.cpp:46-59 does between two computeTrueCost calls (makeVertex + ribbonsToArray + ppgpu_set_vertices on the host
// route).  Included by pp_kernels.h.
#pragma once

// Everything of one depth, by value.  Plans are numbered in the call's device order (most legs first), so the plans that have a leg
// at depth d are [0, n_now) and those that have one at depth d + 1 are [0, n_next), n_next <= n_now.
struct PPChainArgs {
    const ppgpu_edge_result* results;   // [n_now] the records of depth d
    const double* child; int stride;    // [n_now][stride][4] their child ribbon lists
    ppgpu_wrapper_edge* next;           // [n_next] the legs of depth d + 1 (NULL when n_next == 0)
    int n_now, n_next, depth;
    const int* start_vertex;            // [plan] the open vertex the plan starts from
    ppgpu_vertex* verts; int run0;      // plan j's running vertex is verts[run0 + j] ...
    double* ribbons; int rib0;          // ... and its ribbons start at ribbon rib0 + j * stride of the pool
    int* costed; unsigned* stop;        // [plan] legs costed so far; why the chain ended (0: it has not)
};

// AStarPlanner.cpp:53-57 plus the capacity cases: why a chain ends at this record, 0 when it goes on
__device__ __forceinline__ unsigned pp_chain_stop(unsigned flags, int count, int stride) {
    if (flags & PPGPU_F_THROWS) return PPGPU_CHAIN_THROWS;
    if ((flags & (PPGPU_F_DUBINS_ERR | PPGPU_F_RIBBON_LOST)) || count > stride) return PPGPU_CHAIN_CAPACITY;
    if (flags & PPGPU_F_INFEASIBLE) return PPGPU_CHAIN_INFEASIBLE;
    if (flags & PPGPU_F_GOAL) return PPGPU_CHAIN_GOAL;
    return 0u;                          // (PPGPU_F_RIBBON_OVF alone: the list is whole, only h was not enumerated)
}

// One wavefront per plan: lane 0 writes the scalars, lane i copies ribbon i.  Latency-bound by construction (a few hundred bytes
// per plan); it exists to keep the host out of the loop between depths.
__global__ __launch_bounds__(64) void pp_k_chain_advance(PPChainArgs a) {
    const int j = blockIdx.x;
    if (j >= a.n_now) return;
    const int lane = threadIdx.x;
    unsigned stop = a.stop[j];
    const ppgpu_edge_result* r = a.results + j;
    int count = 0;
    if (stop == 0u) {                   // the leg just costed belongs to the chain
        count = (int)((r->info >> 8) & 0xffu);
        stop = pp_chain_stop(r->flags, count, a.stride);
        if (stop == 0u && j >= a.n_next) stop = PPGPU_CHAIN_LEGS;
        if (lane == 0) {
            a.costed[j] = a.depth + 1;
            if (stop != 0u) a.stop[j] = stop;
        }
    }
    if (j >= a.n_next) return;
    ppgpu_vertex* V = a.verts + a.run0 + j;
    if (stop != 0u) {
        // The chain has ended but the plan still has a slot in the next launch: its leg becomes a curve that starts after the first
        // step of the plan's own start vertex — the 0-step "first sample throws" edge (Edge.cpp:126-133), which costs no sweep.
        if (lane == 0) {
            const int sv = a.start_vertex[j];
            a.next[j].vertex = sv;
            a.next[j].start_time = 1e300;
            ppgpu_vertex v = a.verts[sv];       // (nothing reads the running vertex again; its time-grid row stays defined)
            v.ribbon_offset = a.rib0 + j * a.stride;
            v.ribbon_count = 0;
            *V = v;
        }
        return;
    }
    if (lane == 0) {                    // Vertex(child state, g, child RibbonManager): what makeVertex() uploads for this child
        ppgpu_vertex v;
        v.x = r->end_x; v.y = r->end_y; v.heading = r->end_heading; v.speed = r->end_speed; v.time = r->end_time;
        v.g = r->g;
        v.coverage_completed_time = r->coverage_completed_time;
        v.ribbon_offset = a.rib0 + j * a.stride;
        v.ribbon_count = count;
        *V = v;
    }
    if (lane < count) {                 // count <= stride <= 64 (pp_chain_stop)
        const double* s = a.child + ((size_t)j * a.stride + lane) * 4;
        double* d = a.ribbons + ((size_t)a.rib0 + (size_t)j * a.stride + lane) * 4;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
    }
}
