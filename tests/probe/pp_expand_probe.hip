// pp_expand_probe.hip — test-only probes of the small algorithms of path_planner_amd/csrc/pp_k_expand.h, each alone
// (tests/expand_probe.py, tests/test_gpu_expand_pieces.py): the heap steps of the push-order replay and pp_ord_safe, the rank /
// k-th smallest / k smallest selections, pp_wg_append, pp_half_wave_min, pp_ord_sort, and the kernel pp_k_expand_bound on group
// minima of the test's own.  The kernels here only call the header's
// functions, through the contracts their callers keep (whole wavefronts, 256-thread workgroups, pairs in LDS); they re-implement
// none of them.  Each entry point takes host arrays, allocates, copies in, launches, synchronises, copies out, frees, and returns
// the HIP error code.  Built by __graft_entry__.build() into tests/probe/libpp_expand_probe.so; never linked into libppgpu.so.
#include "pp_kernels.h"
#include <stddef.h>

#define PROBE_LDS_CAP 1024      // pairs a selection probe holds in LDS (pp_k_select_nearest's PP_SEL_CAP)

// ----------------------------------------------------------------------------- kernels
// One wavefront per case, the driver loop of the scan (pp_ord_replay without its skipping): push entry i, pop once the heap holds
// k + 1.  After every operation lanes 0 .. k - 1 write h.idx; once the heap is full, lane 0 writes pp_ord_safe's verdict (else -1).
__global__ __launch_bounds__(PP_WAVE) void probe_k_heap_replay(const double* costs, const long long* ops_off, const long long* idx_off,
                                                               const int* nops, const int* ks, int* out_idx, int* out_safe) {
    const int cs = blockIdx.x, lane = pp_lane(), k = ks[cs];
    const double* c = costs + ops_off[cs];
    int* oi = out_idx + idx_off[cs];
    int* os = out_safe + ops_off[cs];
    PPOrdHeap h = {INFINITY, INFINITY, -1};
    int hsize = 0;
    for (int i = 0; i < nops[cs]; i++) {
        pp_ord_sift_up(h, hsize, c[i], c[i], i);
        hsize++;
        if (hsize > k) { hsize--; pp_ord_pop(h, hsize); }
        if (lane < k) oi[(size_t)i * k + lane] = lane < hsize ? h.idx : -1;
        const bool safe = hsize >= k ? pp_ord_safe(h, k) : false;
        if (lane == 0) os[i] = hsize >= k ? (safe ? 1 : 0) : -1;
    }
}
// One wavefront per case: lane's value x[case][lane], every lane's answer out.
__global__ __launch_bounds__(PP_WAVE) void probe_k_kth_wave(const double* x, const int* n, const int* k, double* out) {
    const size_t at = (size_t)blockIdx.x * PP_WAVE + threadIdx.x;
    out[at] = pp_kth_smallest_wave(x[at], n[blockIdx.x], k[blockIdx.x]);
}
// One 256-thread workgroup per case, the pairs in LDS as the callers hold them; the outputs start from the sentinels.
__global__ __launch_bounds__(256) void probe_k_kth_lds(const double* L, const int* I, const long long* off, const int* n, const int* k,
                                                       double sentL, int sentI, double* outL, int* outI) {
    __shared__ double sl[PROBE_LDS_CAP];
    __shared__ int si[PROBE_LDS_CAP];
    __shared__ double kthL;
    __shared__ int kthI;
    const int cs = blockIdx.x, m = n[cs];
    for (int j = (int)threadIdx.x; j < m; j += 256) { sl[j] = L[off[cs] + j]; si[j] = I ? I[off[cs] + j] : 0; }
    if (threadIdx.x == 0) { kthL = sentL; kthI = sentI; }
    __syncthreads();
    pp_kth_smallest_lds(sl, I ? si : nullptr, m, k[cs], &kthL, &kthI);
    __syncthreads();
    if (threadIdx.x == 0) { outL[cs] = kthL; outI[cs] = kthI; }
}
// One list in LDS, one query (x, xi) per thread.
__global__ __launch_bounds__(256) void probe_k_rank_lds(const double* L, const int* I, int n, const double* x, const int* xi, int nq, int* out) {
    __shared__ double sl[PROBE_LDS_CAP];
    __shared__ int si[PROBE_LDS_CAP];
    for (int j = (int)threadIdx.x; j < n; j += 256) { sl[j] = L[j]; si[j] = I ? I[j] : 0; }
    __syncthreads();
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q < nq) out[q] = pp_rank_lds(sl, I ? si : nullptr, n, x[q], xi[q]);
}
// One workgroup of NT threads per case; entry c of a case = (L, I)[off + c], counted where valid and its length is not negative.
template <int NT>
__global__ __launch_bounds__(NT) void probe_k_k_smallest(const double* L, const int* I, const unsigned char* valid, const long long* off,
                                                         const int* n, const int* k, const long long* ooff, int* oi, double* ol, int with_len) {
    __shared__ double wl[4];
    __shared__ int wi[4];
    const int cs = blockIdx.x;
    const double* l0 = L + off[cs];
    const int* i0 = I + off[cs];
    const unsigned char* v0 = valid + off[cs];
    const auto entry = [=](long long c, double& l, int& i) { l = l0[c]; i = i0[c]; return v0[c] != 0 && l >= 0; };
    pp_k_smallest<NT>(entry, (long long)n[cs], k[cs], oi + ooff[cs], with_len ? ol + ooff[cs] : nullptr, wl, wi);
}
// take: [workgroups][R][256] flags.  Every taken flag writes its id (workgroup * R + flag) * 256 + thread to its slot of its list
// (list 0 with ONE_LIST, list j otherwise; `cap` slots each).  A slot outside [0, cap) is not written: *bad counts them.
template <int R, bool ONE_LIST>
__global__ __launch_bounds__(256) void probe_k_wg_append(const unsigned char* take_in, int* count, int* lists, int cap, int* bad) {
    __shared__ int wcount[R * 4], wbase[R * 4];
    bool take[R];
    int slot[R];
#pragma unroll
    for (int j = 0; j < R; j++) take[j] = take_in[((size_t)blockIdx.x * R + j) * 256 + threadIdx.x] != 0;
    pp_wg_append<R, ONE_LIST>(take, count, wcount, wbase, slot);
#pragma unroll
    for (int j = 0; j < R; j++)
        if (take[j]) {
            if (slot[j] < 0 || slot[j] >= cap) { atomicAdd(bad, 1); continue; }
            lists[(size_t)(ONE_LIST ? 0 : j) * cap + slot[j]] = (int)((blockIdx.x * R + j) * 256 + threadIdx.x);
        }
}
// n is a multiple of the workgroup (the loader pads with +inf)
__global__ __launch_bounds__(256) void probe_k_half_wave_min(const double* x, double* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    out[i] = pp_half_wave_min(x[i]);
}
// cd / ci at PP_ORD_CAP, as pp_k_expand_order declares them; the first n2 (the power of two the sort pads to) come back.
__global__ __launch_bounds__(256) void probe_k_ord_sort(const double* cd_in, const int* ci_in, const int* val, int Mk, int n2, double* cd_out, int* ci_out) {
    __shared__ double cd[PP_ORD_CAP];
    __shared__ int ci[PP_ORD_CAP];
    for (int i = (int)threadIdx.x; i < Mk; i += 256) { cd[i] = cd_in[i]; ci[i] = ci_in[i]; }
    __syncthreads();
    const PPOrdList L = {nullptr, val, nullptr, Mk};
    pp_ord_sort(L, Mk, cd, ci);
    for (int i = (int)threadIdx.x; i < n2; i += 256) { cd_out[i] = cd[i]; ci_out[i] = ci[i]; }
}

// (pp_k_expand_bound is launched as it is: a kernel of its own, whose inputs the host side below lays out.)

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
        if (k >= 16) { err = hipErrorOutOfMemory; return nullptr; }
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
const int BAD = (int)hipErrorInvalidValue;

// offsets of concatenated per-case arrays: off[c] = sum of len(c') for c' < c; false when a length is negative
template <class Len>
bool offsets(int ncase, Len len, long long* off, long long* total) {
    long long t = 0;
    for (int c = 0; c < ncase; c++) {
        const long long l = len(c);
        if (l < 0) return false;
        off[c] = t;
        t += l;
    }
    *total = t;
    return true;
}

template <int R, bool ONE_LIST>
int wg_append(const unsigned char* take, int nwg, int* count, int* lists, int cap, int* bad) {
    constexpr int LISTS = ONE_LIST ? 1 : R;
    if (nwg <= 0 || cap <= 0) return BAD;
    Bufs b;
    const unsigned char* dt = b.in(take, (size_t)nwg * R * 256);
    int* dc = b.in(count, LISTS);
    int* dl = b.in(lists, (size_t)LISTS * cap);
    const int zero = 0;
    int* db = b.in(&zero, 1);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL((probe_k_wg_append<R, ONE_LIST>), dim3(nwg), dim3(256), 0, 0, dt, dc, dl, cap, db);
    b.ran();
    b.out(count, dc, LISTS);
    b.out(lists, dl, (size_t)LISTS * cap);
    b.out(bad, db, 1);
    return (int)b.err;
}
}  // namespace

extern "C" {
// Case c: costs[ops_off[c] .. + nops[c]), 1 <= k[c] < 64.  out_idx[idx_off[c] + i * k[c] + q] = slot q of the heap array after
// operation i (idx_off[c] = sum of nops * k of the cases before); out_safe[ops_off[c] + i] = pp_ord_safe (1 / 0; -1: heap not full).
int ppe_heap_replay(const double* costs, const int* nops, const int* ks, int ncase, int* out_idx, int* out_safe) {
    if (ncase <= 0) return ncase < 0 ? BAD : 0;
    for (int c = 0; c < ncase; c++)
        if (ks[c] < 1 || ks[c] >= PP_WAVE || nops[c] < 0) return BAD;
    long long* ops_off = new long long[2 * (size_t)ncase];
    long long* idx_off = ops_off + ncase;
    long long nop = 0, nidx = 0;
    offsets(ncase, [&](int c) { return (long long)nops[c]; }, ops_off, &nop);
    offsets(ncase, [&](int c) { return (long long)nops[c] * ks[c]; }, idx_off, &nidx);
    int rc;
    {
        Bufs b;
        const double* dc = b.in(costs, (size_t)nop);
        const long long* doo = b.in(ops_off, (size_t)ncase);
        const long long* dio = b.in(idx_off, (size_t)ncase);
        const int* dn = b.in(nops, (size_t)ncase);
        const int* dk = b.in(ks, (size_t)ncase);
        int* di = b.alloc<int>((size_t)nidx);
        int* ds = b.alloc<int>((size_t)nop);
        if (b.err == hipSuccess) {
            hipLaunchKernelGGL(probe_k_heap_replay, dim3(ncase), dim3(PP_WAVE), 0, 0, dc, doo, dio, dn, dk, di, ds);
            b.ran();
            b.out(out_idx, di, (size_t)nidx);
            b.out(out_safe, ds, (size_t)nop);
        }
        rc = (int)b.err;
    }
    delete[] ops_off;
    return rc;
}

// x: [ncase][64] one value per lane; the first n[c] lanes count; out: [ncase][64] what every lane got
int ppe_kth_wave(const double* x, const int* n, const int* k, int ncase, double* out) {
    if (ncase <= 0) return ncase < 0 ? BAD : 0;
    for (int c = 0; c < ncase; c++)
        if (n[c] < 0 || n[c] > PP_WAVE || k[c] < 1) return BAD;
    Bufs b;
    const double* dx = b.in(x, (size_t)ncase * PP_WAVE);
    const int* dn = b.in(n, (size_t)ncase);
    const int* dk = b.in(k, (size_t)ncase);
    double* d = b.alloc<double>((size_t)ncase * PP_WAVE);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_kth_wave, dim3(ncase), dim3(PP_WAVE), 0, 0, dx, dn, dk, d);
    b.ran();
    b.out(out, d, (size_t)ncase * PP_WAVE);
    return (int)b.err;
}

// Case c: the pairs (L, I)[sum of n before c .. + n[c]), n[c] <= 1024; I null: ties by position.  outL / outI [ncase]: the k-th
// smallest, or the sentinels they were pre-set to.
int ppe_kth_lds(const double* L, const int* I, const int* n, const int* k, int ncase, double sentL, int sentI, double* outL, int* outI) {
    if (ncase <= 0) return ncase < 0 ? BAD : 0;
    for (int c = 0; c < ncase; c++)
        if (n[c] < 0 || n[c] > PROBE_LDS_CAP || k[c] < 1) return BAD;
    long long* off = new long long[(size_t)ncase];
    long long tot = 0;
    offsets(ncase, [&](int c) { return (long long)n[c]; }, off, &tot);
    int rc;
    {
        Bufs b;
        const double* dL = b.in(L, (size_t)tot);
        const int* dI = I ? b.in(I, (size_t)tot) : nullptr;
        const long long* doff = b.in(off, (size_t)ncase);
        const int* dn = b.in(n, (size_t)ncase);
        const int* dk = b.in(k, (size_t)ncase);
        double* dl = b.alloc<double>((size_t)ncase);
        int* di = b.alloc<int>((size_t)ncase);
        if (b.err == hipSuccess) {
            hipLaunchKernelGGL(probe_k_kth_lds, dim3(ncase), dim3(256), 0, 0, dL, dI, doff, dn, dk, sentL, sentI, dl, di);
            b.ran();
            b.out(outL, dl, (size_t)ncase);
            b.out(outI, di, (size_t)ncase);
        }
        rc = (int)b.err;
    }
    delete[] off;
    return rc;
}

// one list of n <= 1024 pairs (I null: ties by position), nq queries (x, xi): how many pairs come before each
int ppe_rank_lds(const double* L, const int* I, int n, const double* x, const int* xi, int nq, int* out) {
    if (n < 0 || n > PROBE_LDS_CAP || nq < 0) return BAD;
    if (nq == 0) return 0;
    Bufs b;
    const double* dL = b.in(L, (size_t)n);
    const int* dI = I ? b.in(I, (size_t)n) : nullptr;
    const double* dx = b.in(x, (size_t)nq);
    const int* dxi = b.in(xi, (size_t)nq);
    int* d = b.alloc<int>((size_t)nq);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_rank_lds, dim3((nq + 255) / 256), dim3(256), 0, 0, dL, dI, n, dx, dxi, nq, d);
    b.ran();
    b.out(out, d, (size_t)nq);
    return (int)b.err;
}

// nt = 256 or 64.  Case c: entries (L, I, valid)[sum of n before c .. + n[c]); its k[c] winners -> oi / ol[sum of k before c ..).
// ol null: the form without lengths.  The outputs are copied in first, so what the kernel leaves unwritten shows.
int ppe_k_smallest(int nt, const double* L, const int* I, const unsigned char* valid, const int* n, const int* k, int ncase, int* oi, double* ol) {
    if (ncase <= 0) return ncase < 0 ? BAD : 0;
    if (nt != 256 && nt != PP_WAVE) return BAD;
    for (int c = 0; c < ncase; c++)
        if (n[c] < 0 || k[c] < 0) return BAD;
    long long* off = new long long[2 * (size_t)ncase];
    long long* ooff = off + ncase;
    long long tot = 0, otot = 0;
    offsets(ncase, [&](int c) { return (long long)n[c]; }, off, &tot);
    offsets(ncase, [&](int c) { return (long long)k[c]; }, ooff, &otot);
    int rc;
    {
        Bufs b;
        const double* dL = b.in(L, (size_t)tot);
        const int* dI = b.in(I, (size_t)tot);
        const unsigned char* dv = b.in(valid, (size_t)tot);
        const long long* doff = b.in(off, (size_t)ncase);
        const long long* dooff = b.in(ooff, (size_t)ncase);
        const int* dn = b.in(n, (size_t)ncase);
        const int* dk = b.in(k, (size_t)ncase);
        int* doi = b.in(oi, (size_t)otot);
        double* dol = ol ? b.in(ol, (size_t)otot) : nullptr;
        if (b.err == hipSuccess) {
            if (nt == 256) hipLaunchKernelGGL(probe_k_k_smallest<256>, dim3(ncase), dim3(256), 0, 0, dL, dI, dv, doff, dn, dk, dooff, doi, dol, ol ? 1 : 0);
            else hipLaunchKernelGGL(probe_k_k_smallest<PP_WAVE>, dim3(ncase), dim3(PP_WAVE), 0, 0, dL, dI, dv, doff, dn, dk, dooff, doi, dol, ol ? 1 : 0);
            b.ran();
            b.out(oi, doi, (size_t)otot);
            if (ol) b.out(ol, dol, (size_t)otot);
        }
        rc = (int)b.err;
    }
    delete[] off;
    return rc;
}

// pp_wg_append<8, true>: take [nwg][8][256]; count[1] in / out; list [cap] in / out.  pp_wg_append<2, false>: take [nwg][2][256];
// count[2]; lists [2][cap].  *bad: taken flags whose slot fell outside [0, cap) (not written).
int ppe_wg_append_one_list8(const unsigned char* take, int nwg, int* count, int* list, int cap, int* bad) {
    return wg_append<8, true>(take, nwg, count, list, cap, bad);
}
int ppe_wg_append_two_lists(const unsigned char* take, int nwg, int* count, int* lists, int cap, int* bad) {
    return wg_append<2, false>(take, nwg, count, lists, cap, bad);
}

// n a multiple of 256
int ppe_half_wave_min(const double* x, double* out, long long n) {
    if (n <= 0 || (n % 256) != 0) return n == 0 ? 0 : BAD;
    Bufs b;
    const double* dx = b.in(x, (size_t)n);
    double* d = b.alloc<double>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_half_wave_min, dim3((unsigned)(n / 256)), dim3(256), 0, 0, dx, d);
    b.ran();
    b.out(out, d, (size_t)n);
    return (int)b.err;
}

// pp_k_expand_bound for one vertex: near_count near slots in groups of 32, groupmin[g][2] the smallest length of group g per radius
// (+inf: none), groupcnt[g] its slots in use.  -> bound[2] (U per radius), cand_count[2] (handed in non-zero, the kernel resets them).
int ppe_expand_bound(const double* groupmin, const int* groupcnt, int near_count, int k, double* bound, int* cand_count) {
    if (near_count < 0 || k < 1) return BAD;
    const int ngrp = (near_count + PP_NEAR_GROUP - 1) / PP_NEAR_GROUP;
    Bufs b;
    PPExpandArgs a{};
    a.k = k;
    a.groups_row = ngrp;
    a.near_count = b.in(&near_count, 1);
    a.groupmin = b.in(groupmin, (size_t)ngrp * 2);
    a.groupcnt = b.in(groupcnt, (size_t)ngrp);
    a.bound = b.in(bound, 2);
    a.cand_count = b.in(cand_count, 2);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(pp_k_expand_bound, dim3(2), dim3(256), 0, 0, a);
    b.ran();
    b.out(bound, a.bound, 2);
    b.out(cand_count, a.cand_count, 2);
    return (int)b.err;
}

// Mk kept candidates (distance cd, list position ci < M), val[M] the list's samples; cd_out / ci_out [n2], n2 = the power of two
// (at least 64) the sort pads to.
int ppe_ord_sort(const double* cd, const int* ci, const int* val, int Mk, int M, int n2, double* cd_out, int* ci_out) {
    if (Mk < 0 || Mk > PP_ORD_CAP || M < 0) return BAD;
    int want = 64;
    while (want < Mk) want <<= 1;
    if (n2 != want) return BAD;
    for (int i = 0; i < Mk; i++)
        if (ci[i] < 0 || ci[i] >= M) return BAD;
    Bufs b;
    const double* dcd = b.in(cd, (size_t)Mk);
    const int* dci = b.in(ci, (size_t)Mk);
    const int* dv = b.in(val, (size_t)M);
    double* ocd = b.alloc<double>((size_t)n2);
    int* oci = b.alloc<int>((size_t)n2);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_ord_sort, dim3(1), dim3(256), 0, 0, dcd, dci, dv, Mk, n2, ocd, oci);
    b.ran();
    b.out(cd_out, ocd, (size_t)n2);
    b.out(ci_out, oci, (size_t)n2);
    return (int)b.err;
}
}  // extern "C"
