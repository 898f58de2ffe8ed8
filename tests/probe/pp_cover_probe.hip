// pp_cover_probe.hip — test-only probes of the coverage state machine's pieces, each alone (tests/cover_probe.py,
// tests/test_gpu_cover_pieces.py): pp_ribbons_event, pp_corridor_run and pp_quiet_run of pp_device.h (with pp_pieces_in_reach and
// pp_any_erasable_piece inside them), pp_event_stride, pp_box_scan and pp_any_tiny_ribbon of pp_k_cover.h, and the lane forms
// pp_lane_ribbon_contains and pp_lane_cover_strict of pp_k_finish.h (pp_in_grown_box inside pp_box_scan).  The kernels here only call
// the header's functions, through the contracts their callers keep: whole 64-lane wavefronts with every lane executing the call, ribbon
// i in lane i and the zero ribbon in lanes >= n, 64 x 4 doubles of LDS per wave for pp_ribbons_event; they re-implement none of them.
// Each entry point takes host arrays, allocates, copies in, launches, synchronises, copies out, frees, and returns the HIP error code.
// Built by __graft_entry__.build() into tests/probe/libpp_cover_probe.so; never linked into libppgpu.so.
#include "pp_kernels.h"
#include <stddef.h>

#define PROBE_BLOCK 256

// ----------------------------------------------------------------------------- kernels
// One wavefront per case: the case's list, then its events one after the other as pp_cover_sweep_edge applies them (a count above 64 is
// reported as returned and clamped to 64 before the next event).  Event g = ev_off[case] + i writes count, D, adv and all 64 lanes.
__global__ __launch_bounds__(PP_WAVE) void probe_k_cover_events(const double* ribs, const int* ns, const double* ws, const long long* ev_off,
                                                                const double* ev, int* out_cnt, double* out_D, int* out_adv, double* out_ribs) {
    __shared__ double lds[PP_WAVE * 4];
    const int cs = blockIdx.x, lane = pp_lane();
    const double* rp = ribs + ((size_t)cs * PP_WAVE + lane) * 4;
    PPRibbon r = {rp[0], rp[1], rp[2], rp[3]};
    int n = ns[cs];
    const double w = ws[cs];
    for (long long g = ev_off[cs]; g < ev_off[cs + 1]; g++) {
        double D;
        int adv;
        const int cnt = pp_ribbons_event(r, n, w, ev[3 * g], ev[3 * g + 1], ev[3 * g + 2] != 0.0, lds, D, adv);
        n = cnt > PP_WAVE ? PP_WAVE : cnt;
        if (lane == 0) { out_cnt[g] = cnt; out_D[g] = D; out_adv[g] = adv; }
        double* o = out_ribs + ((size_t)g * PP_WAVE + lane) * 4;
        o[0] = r.sx; o[1] = r.sy; o[2] = r.ex; o[3] = r.ey;
    }
}

// One wavefront per case: lane i holds ribbon i and pose i.  ints = {n, kind (1 corridor, 2 quiet), adv, moveEnd, first},
// masks = {stepOk, coverMask}, dbls = {w, span, ell, sinDt}; out = {L, newX, newY} (the last two as the run left them: 0 when L == 0
// or for a quiet run).
__global__ __launch_bounds__(PP_WAVE) void probe_k_cover_runs(const double* ribs, const double* poses, const int* ints, const unsigned long long* masks,
                                                              const double* dbls, int* out_L, double* out_xy) {
    const int cs = blockIdx.x, lane = pp_lane();
    const double* rp = ribs + ((size_t)cs * PP_WAVE + lane) * 4;
    const PPRibbon r = {rp[0], rp[1], rp[2], rp[3]};
    const double x = poses[((size_t)cs * PP_WAVE + lane) * 2], y = poses[((size_t)cs * PP_WAVE + lane) * 2 + 1];
    const int n = ints[5 * cs], kind = ints[5 * cs + 1], adv = ints[5 * cs + 2], first = ints[5 * cs + 4];
    const bool moveEnd = ints[5 * cs + 3] != 0;
    const bool stepOk = ((masks[2 * cs] >> lane) & 1ull) != 0ull;
    const unsigned long long coverMask = masks[2 * cs + 1];
    const double w = dbls[4 * cs], span = dbls[4 * cs + 1], ell = dbls[4 * cs + 2], sinDt = dbls[4 * cs + 3];
    double nx = 0.0, ny = 0.0;
    int L;
    if (kind == 1) L = pp_corridor_run(r, n, w, adv, moveEnd, x, y, stepOk, coverMask, first, span, nx, ny, ell, sinDt);
    else L = pp_quiet_run(r, n, w, x, y, stepOk, coverMask, first, span, ell, sinDt);
    if (lane == 0) { out_L[cs] = L; out_xy[2 * cs] = nx; out_xy[2 * cs + 1] = ny; }
}

// One lane per case from here on.
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_lane_contains(const double* rib, const double* x, const double* y, const double* w,
                                                                     unsigned char* inside, unsigned char* strict, double* pxy, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    bool in, st;
    double px, py;
    pp_lane_ribbon_contains(rib[4 * i], rib[4 * i + 1], rib[4 * i + 2], rib[4 * i + 3], x[i], y[i], w[i], in, st, px, py);
    inside[i] = in ? 1 : 0; strict[i] = st ? 1 : 0;
    pxy[2 * i] = px; pxy[2 * i + 1] = py;
}
// slots: one child slot of PP_FINISH_MAX ribbons per case, changed in place
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_lane_cover_strict(double* slots, const int* nrib, const int* stride, const double* x, const double* y,
                                                                         const double* w, int* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_lane_cover_strict(slots + (size_t)i * PP_FINISH_MAX * 4, nrib[i], stride[i], x[i], y[i], w[i]);
}
// lists: case i's ribbons start at off[i]; out_i = {inBox, boxCount, boxIdx, any tiny}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_box_scan(const double* lists, const long long* off, const int* ns, const double* x, const double* y,
                                                                const double* grow, const double* thr, int* out_i, double* out_q, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* r = lists + 4 * off[i];
    const PPBoxScan s = pp_box_scan(r, ns[i], x[i], y[i], grow[i]);
    out_i[4 * i] = s.inBox ? 1 : 0; out_i[4 * i + 1] = s.boxCount; out_i[4 * i + 2] = s.boxIdx;
    out_i[4 * i + 3] = pp_any_tiny_ribbon(r, ns[i], thr[i]) ? 1 : 0;
    out_q[i] = s.q;
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_event_stride(const double* D, const double* inc, const double* inv_inc, const int* ng, int* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_event_stride(D[i], inc[i], inv_inc[i], ng[i]);
}

// ----------------------------------------------------------------------------- host side
namespace {
// device buffers of one call: freed when the call returns, whatever it returns
struct Bufs {
    void* p[16];
    int k = 0;
    hipError_t err = hipSuccess;
    ~Bufs() { for (int i = 0; i < k; i++) (void)hipFree(p[i]); }
    template <class T> T* alloc(size_t count) {
        if (err != hipSuccess) return nullptr;
        void* d = nullptr;
        err = hipMalloc(&d, (count ? count : 1) * sizeof(T));
        if (err != hipSuccess) return nullptr;
        p[k++] = d;
        return (T*)d;
    }
    template <class T> T* in(const T* h, size_t count) {
        T* d = alloc<T>(count);
        if (d && count) err = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
        return err == hipSuccess ? d : nullptr;
    }
    template <class T> void out(T* h, const T* d, size_t count) {
        if (err == hipSuccess && count) err = hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    // after the launch: launch error, then the kernel's own
    void ran() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
};
inline unsigned nblk(long long n) { return (unsigned)((n + PROBE_BLOCK - 1) / PROBE_BLOCK); }
}  // namespace

extern "C" {
// ribs: ncase x 64 x 4 (zero beyond ns[case]); ev_off: ncase + 1 offsets into ev (x, y, doCover per event), increasing from 0;
// outputs per event: count, D, adv, 64 x 4 doubles
int ppc_cover_events(const double* ribs, const int* ns, const double* ws, const long long* ev_off, const double* ev, long long ncase,
                     int* out_cnt, double* out_D, int* out_adv, double* out_ribs) {
    if (ncase <= 0) return ncase < 0 ? (int)hipErrorInvalidValue : 0;
    long long nev = ev_off[ncase];
    if (ev_off[0] != 0 || nev < 0) return (int)hipErrorInvalidValue;
    for (long long i = 0; i < ncase; i++)
        if (ns[i] < 0 || ns[i] > PP_WAVE || ev_off[i + 1] < ev_off[i]) return (int)hipErrorInvalidValue;
    Bufs b;
    const double* dr = b.in(ribs, (size_t)ncase * PP_WAVE * 4);
    const int* dn = b.in(ns, (size_t)ncase);
    const double* dw = b.in(ws, (size_t)ncase);
    const long long* doff = b.in(ev_off, (size_t)ncase + 1);
    const double* dev = b.in(ev, (size_t)nev * 3);
    int* oc = b.alloc<int>((size_t)nev);
    double* oD = b.alloc<double>((size_t)nev);
    int* oa = b.alloc<int>((size_t)nev);
    double* orb = b.alloc<double>((size_t)nev * PP_WAVE * 4);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_cover_events, dim3((unsigned)ncase), dim3(PP_WAVE), 0, 0, dr, dn, dw, doff, dev, oc, oD, oa, orb);
    b.ran();
    b.out(out_cnt, oc, (size_t)nev);
    b.out(out_D, oD, (size_t)nev);
    b.out(out_adv, oa, (size_t)nev);
    b.out(out_ribs, orb, (size_t)nev * PP_WAVE * 4);
    return (int)b.err;
}

// ribs: ncase x 64 x 4, poses: ncase x 64 x 2, ints: ncase x 5, masks: ncase x 2, dbls: ncase x 4 (see probe_k_cover_runs)
int ppc_cover_runs(const double* ribs, const double* poses, const int* ints, const unsigned long long* masks, const double* dbls, long long ncase,
                   int* out_L, double* out_xy) {
    if (ncase <= 0) return ncase < 0 ? (int)hipErrorInvalidValue : 0;
    for (long long i = 0; i < ncase; i++) {
        const int n = ints[5 * i], kind = ints[5 * i + 1], adv = ints[5 * i + 2], first = ints[5 * i + 4];
        if (n < 0 || n > PP_WAVE || (kind != 1 && kind != 2) || first < 0 || first > PP_WAVE) return (int)hipErrorInvalidValue;
        if (kind == 1 && (adv < 0 || adv >= PP_WAVE)) return (int)hipErrorInvalidValue;      // the lane pp_readlane reads the piece from
        if (first == PP_WAVE) return (int)hipErrorInvalidValue;                              // ... and the pose of step `first`
    }
    Bufs b;
    const double* dr = b.in(ribs, (size_t)ncase * PP_WAVE * 4);
    const double* dp = b.in(poses, (size_t)ncase * PP_WAVE * 2);
    const int* di = b.in(ints, (size_t)ncase * 5);
    const unsigned long long* dm = b.in(masks, (size_t)ncase * 2);
    const double* dd = b.in(dbls, (size_t)ncase * 4);
    int* oL = b.alloc<int>((size_t)ncase);
    double* oxy = b.alloc<double>((size_t)ncase * 2);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_cover_runs, dim3((unsigned)ncase), dim3(PP_WAVE), 0, 0, dr, dp, di, dm, dd, oL, oxy);
    b.ran();
    b.out(out_L, oL, (size_t)ncase);
    b.out(out_xy, oxy, (size_t)ncase * 2);
    return (int)b.err;
}

int ppc_lane_contains(const double* rib, const double* x, const double* y, const double* w, unsigned char* inside, unsigned char* strict,
                      double* pxy, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    const double* dr = b.in(rib, (size_t)n * 4);
    const double* dx = b.in(x, (size_t)n);
    const double* dy = b.in(y, (size_t)n);
    const double* dw = b.in(w, (size_t)n);
    unsigned char* oi = b.alloc<unsigned char>((size_t)n);
    unsigned char* os = b.alloc<unsigned char>((size_t)n);
    double* op = b.alloc<double>((size_t)n * 2);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_lane_contains, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dr, dx, dy, dw, oi, os, op, n);
    b.ran();
    b.out(inside, oi, (size_t)n);
    b.out(strict, os, (size_t)n);
    b.out(pxy, op, (size_t)n * 2);
    return (int)b.err;
}

// slots: n x PP_FINISH_MAX x 4 doubles, in and out
int ppc_lane_cover_strict(double* slots, const int* nrib, const int* stride, const double* x, const double* y, const double* w, int* out, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    for (long long i = 0; i < n; i++)
        if (nrib[i] < 0 || nrib[i] > PP_FINISH_MAX || stride[i] < 0 || stride[i] > PP_FINISH_MAX) return (int)hipErrorInvalidValue;
    Bufs b;
    double* ds = b.in(slots, (size_t)n * PP_FINISH_MAX * 4);
    const int* dn = b.in(nrib, (size_t)n);
    const int* dst = b.in(stride, (size_t)n);
    const double* dx = b.in(x, (size_t)n);
    const double* dy = b.in(y, (size_t)n);
    const double* dw = b.in(w, (size_t)n);
    int* o = b.alloc<int>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_lane_cover_strict, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, ds, dn, dst, dx, dy, dw, o, n);
    b.ran();
    b.out(slots, ds, (size_t)n * PP_FINISH_MAX * 4);
    b.out(out, o, (size_t)n);
    return (int)b.err;
}

// lists: nrib_total x 4; off: n + 1 ribbon offsets, increasing from 0; case i scans ribbons off[i] .. off[i + 1] - 1
int ppc_box_scan(const double* lists, const long long* off, const double* x, const double* y, const double* grow, const double* thr,
                 int* out_i, double* out_q, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    if (off[0] != 0) return (int)hipErrorInvalidValue;
    Bufs b;
    int* hn = new int[(size_t)n];
    bool bad = false;
    for (long long i = 0; i < n; i++) { hn[i] = (int)(off[i + 1] - off[i]); bad |= off[i + 1] < off[i]; }
    const double* dl = bad ? nullptr : b.in(lists, (size_t)off[n] * 4);
    const long long* doff = b.in(off, (size_t)n + 1);
    const int* dn = b.in(hn, (size_t)n);
    delete[] hn;
    if (bad) return (int)hipErrorInvalidValue;
    const double* dx = b.in(x, (size_t)n);
    const double* dy = b.in(y, (size_t)n);
    const double* dg = b.in(grow, (size_t)n);
    const double* dt = b.in(thr, (size_t)n);
    int* oi = b.alloc<int>((size_t)n * 4);
    double* oq = b.alloc<double>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_box_scan, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dl, doff, dn, dx, dy, dg, dt, oi, oq, n);
    b.ran();
    b.out(out_i, oi, (size_t)n * 4);
    b.out(out_q, oq, (size_t)n);
    return (int)b.err;
}

// inv_inc = 1.0 / inc, the launch's own expression (ppgpu.hip: p.inv_inc_d = 1.0 / p.inc_d), computed here in the host's double division
int ppc_event_stride(const double* D, const double* inc, const int* ng, int* out, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    double* hinv = new double[(size_t)n];
    for (long long i = 0; i < n; i++) hinv[i] = 1.0 / inc[i];
    const double* dD = b.in(D, (size_t)n);
    const double* di = b.in(inc, (size_t)n);
    const double* dv = b.in(hinv, (size_t)n);
    delete[] hinv;
    const int* dg = b.in(ng, (size_t)n);
    int* o = b.alloc<int>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_event_stride, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dD, di, dv, dg, o, n);
    b.ran();
    b.out(out, o, (size_t)n);
    return (int)b.err;
}
}  // extern "C"
