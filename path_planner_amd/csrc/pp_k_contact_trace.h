// pp_k_contact_trace.h — pp_k_trace_contacts: which contact an edge pays for, one 64-byte ppgpu_contact_record per (edge, obstacle
// row): on how many steps of the sweep of Edge::computeTrueCost (Edge.cpp:125-175) the contact is hit, from when to when, what it
// adds to the penalty, and how close the vehicle comes to it otherwise.  Included by pp_kernels.h.
#pragma once
// The step trace (pp_k_trace.h) gives collisionExists per step, summed over the contacts; this kernel gives the same sweep per
// contact, on the shared trace core (pp_k_trace_common.h): the step count is pp_trace_head's and the windows are pp_trace_window's,
// without headings, so the steps and poses are those of the step trace (the same doubles).  No skipping, no culling.  Per window
//     lane = step          pose, time, isBlocked from pp_trace_window; Gaussian model: the step's own collisionExists
//                          (pp_obstacle_density_chunk, the floored sum the costing launch counts).  {x, y} {time, flags} go to LDS.
//     lane = obstacle row  walks the window's steps from LDS (every lane reads the same address: a broadcast) with the arithmetic of
//                          pp_obstacle_hit / pp_obstacle_pdf and keeps the contact's accumulators in registers: strict `<` on the
//                          squared distance keeps the earliest step on ties, and nothing crosses lanes.
// More than 64 rows: passes of 64, each walking the edge again (the accumulators stay in registers; fleets that large are rare).
// A pass's records are contiguous (4 KB for 64 rows) and leave through pp_trace_store, from the LDS block that held the window's
// steps.  With 16 rows the second phase uses a quarter of the wave; DESIGN.md 4.2 says why that form was kept.
#define PP_KTRACE_VALID   1u       // flags of a step in LDS: the step was executed,
#define PP_KTRACE_BLOCKED 2u       // ... Map::isBlocked at its pose (Edge.cpp:144: the loop broke before collisionExists),
#define PP_KTRACE_COUNTED 4u       // ... it adds to the penalty (:150-151): not blocked and, Gaussian model, a floored sum that is not 0
static_assert(sizeof(ppgpu_contact_record) == 64, "a contact record is 64 bytes: four 16-byte stores");
static_assert(sizeof(PPObst) == sizeof(PPGauss) && offsetof(PPGauss, i00) == offsetof(PPObst, halfL) && offsetof(PPGauss, i10) == offsetof(PPObst, pad),
              "a PPGauss row is read through PPObst's fields");

// el = the edge's position in the slice; lds = this wave's 4 * PP_TRACE_LDS_STRIDE double2 (the window's steps, then the records)
template <bool GAUSSIAN>
__device__ __forceinline__ void pp_contact_trace_edge(const PPParams& p, const long long el, ppgpu_contact_record* recs, const long long rec_base,
                                                      int* counts, double2* lds) {
    const int lane = pp_lane();
    const PPTraceHead h = pp_trace_head(p, el);
    const int count = h.count;
    if (lane == 0) counts[h.eg] = count;
    const int nob = p.n_obst;
    if (nob <= 0) return;
    double2* out = reinterpret_cast<double2*>(recs + (size_t)(h.eg - rec_base) * (size_t)nob);
    for (int b = 0; b < nob; b += PP_WAVE) {
        const int rows = (nob - b) < PP_WAVE ? (nob - b) : PP_WAVE;
        PPObst o = {0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};
        if (lane < rows) o = p.obst[b + lane];
        // a PPGauss row in PPObst's fields (same size, same leading fields): the inverse covariance and the norm
        const double i00 = o.halfL, i01 = o.halfW, i10 = o.pad[0], i11 = o.pad[1], norm = o.pad[2];
        double minD2 = INFINITY, cpaTime = -1.0, firstT = -1.0, lastT = -1.0, exposure = 0.0, peak = 0.0;
        int cpaStep = -1, hitSteps = 0, firstK = -1, lastK = -1;
        PPTraceWalk walk = pp_trace_walk_begin(h, 0.0);
        for (int base = 0; base < count; base += PP_WAVE) {
            const PPTraceWindow n = pp_trace_window<false>(p, h, walk, base, count);
            bool counted = n.valid & !n.blocked;
            if (GAUSSIAN) counted = counted & (pp_trace_density(p, h, n) != 0.0);
            const unsigned sf = (n.valid ? PP_KTRACE_VALID : 0u) | (n.blocked ? PP_KTRACE_BLOCKED : 0u) | (counted ? PP_KTRACE_COUNTED : 0u);
            lds[lane] = make_double2(n.x, n.y);
            lds[PP_TRACE_LDS_STRIDE + lane] = make_double2(n.t, __longlong_as_double((long long)(unsigned long long)sf));
            pp_wave_lds_fence();
            const int nsteps = (count - base) < PP_WAVE ? (count - base) : PP_WAVE;
            for (int s = 0; s < nsteps; s++) {
                const double2 xy = lds[s], tf = lds[PP_TRACE_LDS_STRIDE + s];
                const double st = tf.x;
                const unsigned f = (unsigned)(unsigned long long)__double_as_longlong(tf.y);
                // pp_obstacle_hit / pp_obstacle_pdf, term for term
                const double dt = st - o.Time;
                const double X = o.X + o.Speed * dt * o.cosYaw;
                const double Y = o.Y + o.Speed * dt * o.sinYaw;
                const double tx = xy.x - X, ty = xy.y - Y;
                const double d2 = tx * tx + ty * ty;
                if (cpaStep < 0 || d2 < minD2) { minD2 = d2; cpaStep = base + s; cpaTime = st; }
                bool hit;
                if (!GAUSSIAN) {
                    const double rx = tx * o.cosYaw - ty * o.sinYaw;
                    const double ry = tx * o.sinYaw + ty * o.cosYaw;
                    hit = (f & PP_KTRACE_COUNTED) && fabs(rx) < o.halfL && fabs(ry) < o.halfW;
                } else {
                    const double r0 = tx * i00 + ty * i10, r1 = tx * i01 + ty * i11;
                    const double quadform = r0 * tx + r1 * ty;
                    const double pdf = norm * exp(-0.5 * quadform);
                    if (pdf > peak) peak = pdf;
                    if (f & PP_KTRACE_COUNTED) exposure += pdf;
                    hit = (f & PP_KTRACE_COUNTED) && pdf >= 1e-5;          // the manager's floor (.cpp:11) applied to the contact alone
                }
                if (hit) {
                    if (hitSteps == 0) { firstK = base + s; firstT = st; }
                    lastK = base + s; lastT = st;
                    hitSteps++;
                }
            }
            pp_wave_lds_fence();
        }
        if (!GAUSSIAN) exposure = (double)hitSteps;
        const double cpaDist = cpaStep >= 0 ? sqrt(minD2) : -1.0;
        // the record, as four 16-byte pieces: {cpa_distance, cpa_time} {first, last hit time} {exposure, cpa_step | hit_steps}
        // {first | last hit step, peak}
        lds[0 * PP_TRACE_LDS_STRIDE + lane] = make_double2(cpaDist, cpaTime);
        lds[1 * PP_TRACE_LDS_STRIDE + lane] = make_double2(firstT, lastT);
        lds[2 * PP_TRACE_LDS_STRIDE + lane] =
            make_double2(exposure, __longlong_as_double((long long)(((unsigned long long)(unsigned)hitSteps << 32) | (unsigned long long)(unsigned)cpaStep)));
        lds[3 * PP_TRACE_LDS_STRIDE + lane] =
            make_double2(__longlong_as_double((long long)(((unsigned long long)(unsigned)lastK << 32) | (unsigned long long)(unsigned)firstK)), peak);
        pp_trace_store<4>(lds, out, b, nob);                               // row b + r: of the pass's 64 rows, those the table has
    }
}

// n_edges = slice size; recs[(edge - rec_base) * p.n_obst + row]; counts[edge]
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_contacts(PPParams p, ppgpu_contact_record* recs, long long rec_base, int* counts) {
    __shared__ double2 s_rec[PP_TRACE_WPB][4 * PP_TRACE_LDS_STRIDE];
    int wave;
    long long el;
    if (pp_trace_entry(p, wave, el)) pp_contact_trace_edge<false>(p, el, recs, rec_base, counts, s_rec[wave]);
}
__global__ __launch_bounds__(PP_TRACE_WPB * 64) void pp_k_trace_contacts_gaussian(PPParams p, ppgpu_contact_record* recs, long long rec_base, int* counts) {
    __shared__ double2 s_rec[PP_TRACE_WPB][4 * PP_TRACE_LDS_STRIDE];
    int wave;
    long long el;
    if (pp_trace_entry(p, wave, el)) pp_contact_trace_edge<true>(p, el, recs, rec_base, counts, s_rec[wave]);
}
