// pp_device_probe.hip — test-only probes of the small device functions in path_planner_amd/csrc/pp_device.h (tests/device_probe.py,
// tests/test_gpu_device_math.py).  One trivial kernel per primitive, one lane per element, 256-thread blocks; each entry point takes
// host arrays, allocates, copies in, launches, synchronises, copies out, frees, and returns the HIP error code.  Built by
// __graft_entry__.build() into tests/probe/libpp_device_probe.so; never linked into libppgpu.so.
#include "pp_device.h"
#include <stddef.h>

#define PROBE_BLOCK 256

// ----------------------------------------------------------------------------- kernels
template <bool TAB>
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_sincos_bounded(const double* x, double* s, double* c, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    double sn, cs;
    pp_sincos_bounded<TAB>(x[i], &sn, &cs);
    s[i] = sn; c[i] = cs;
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_sincos(const double* x, double* s, double* c, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    double sn, cs;
    pp_sincos(x[i], &sn, &cs);
    s[i] = sn; c[i] = cs;
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_cr_sincos(const double* x, double* s, double* c, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    double sn, cs;
    pp_cr_sincos(x[i], &sn, &cs);
    s[i] = sn; c[i] = cs;
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_cr_atan2(const double* y, const double* x, double* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_cr_atan2(y[i], x[i]);
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_cr_acos(const double* v, double* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_cr_acos(v[i]);
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_mod2pi(const double* t, double* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_mod2pi(t[i]);
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_udiv_small(const unsigned* x, const unsigned* d, unsigned* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_udiv_small(x[i], d[i]);
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_is_blocked(PPGrid g, const double* x, const double* y, unsigned char* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_is_blocked(g, x[i], y[i]) ? 1 : 0;
}
// pp_blocked_cell, the load, pp_blocked_test: what the pose sweep does in three places.  (The host side always allocates at least one
// word, so the word 0 a lane outside the grid reads exists even for an empty grid.)
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_blocked_cell(PPGrid g, const double* x, const double* y, unsigned char* outside,
                                                                    unsigned* row, unsigned* col, unsigned char* blocked, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PPCellRef ref = pp_blocked_cell(g, x[i], y[i]);
    const uint32_t w = g.bits[ref.word];
    outside[i] = ref.outside ? 1 : 0;
    row[i] = g.wpr > 0 ? (unsigned)(ref.word / (size_t)g.wpr) : 0u;
    col[i] = ref.col;
    blocked[i] = pp_blocked_test(ref, w) ? 1 : 0;
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_line_distance_lt(const double* num, const double* sqL, const double* lim,
                                                                        unsigned char* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = pp_line_distance_lt(num[i], sqL[i], lim[i]) ? 1 : 0;
}
__global__ __launch_bounds__(PROBE_BLOCK) void probe_k_obstacle_hit(const PPObst* ob, const double* x, const double* y, const double* t,
                                                                    int* out, long long n) {
    const long long i = (long long)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PPObst o = ob[i];
    out[i] = pp_obstacle_hit(o, x[i], y[i], t[i]);
}

// ----------------------------------------------------------------------------- host side
namespace {
// device buffers of one call: freed when the call returns, whatever it returns
struct Bufs {
    void* p[12];
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

template <class K>
int sincos_like(K kernel, const double* x, double* s, double* c, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    const double* dx = b.in(x, (size_t)n);
    double* ds = b.alloc<double>((size_t)n);
    double* dc = b.alloc<double>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(kernel, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dx, ds, dc, n);
    b.ran();
    b.out(s, ds, (size_t)n);
    b.out(c, dc, (size_t)n);
    return (int)b.err;
}
// the PPGrid of ppgpu_sampler_add / the costing launches, without the clearance map
PPGrid make_grid(Bufs& b, const uint32_t* bits, int rows, int cols, int wpr, double res) {
    const uint32_t* d = b.in(bits, (size_t)rows * (size_t)wpr);
    return PPGrid{d, rows, cols, wpr, res, res > 0 ? 1.0 / res : 0.0, nullptr};
}
}  // namespace

extern "C" {
int ppp_sincos_bounded(const double* x, double* s, double* c, long long n) { return sincos_like(probe_k_sincos_bounded<false>, x, s, c, n); }
int ppp_sincos_bounded_tab(const double* x, double* s, double* c, long long n) { return sincos_like(probe_k_sincos_bounded<true>, x, s, c, n); }
int ppp_sincos(const double* x, double* s, double* c, long long n) { return sincos_like(probe_k_sincos, x, s, c, n); }
int ppp_cr_sincos(const double* x, double* s, double* c, long long n) { return sincos_like(probe_k_cr_sincos, x, s, c, n); }

int ppp_cr_atan2(const double* y, const double* x, double* out, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    const double* dy = b.in(y, (size_t)n);
    const double* dx = b.in(x, (size_t)n);
    double* d = b.alloc<double>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_cr_atan2, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dy, dx, d, n);
    b.ran();
    b.out(out, d, (size_t)n);
    return (int)b.err;
}
static int unary(void (*kernel)(const double*, double*, long long), const double* v, double* out, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    const double* dv = b.in(v, (size_t)n);
    double* d = b.alloc<double>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(kernel, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dv, d, n);
    b.ran();
    b.out(out, d, (size_t)n);
    return (int)b.err;
}
int ppp_cr_acos(const double* v, double* out, long long n) { return unary(probe_k_cr_acos, v, out, n); }
int ppp_mod2pi(const double* t, double* out, long long n) { return unary(probe_k_mod2pi, t, out, n); }

int ppp_udiv_small(const unsigned* x, const unsigned* d, unsigned* out, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    const unsigned* dx = b.in(x, (size_t)n);
    const unsigned* dd = b.in(d, (size_t)n);
    unsigned* o = b.alloc<unsigned>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_udiv_small, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dx, dd, o, n);
    b.ran();
    b.out(out, o, (size_t)n);
    return (int)b.err;
}

// bits: rows x wpr words, bit (c & 31) of word c >> 5 (the layout ppgpu_set_grid uploads); rows == 0: the base Map, bits may be NULL
int ppp_is_blocked(const uint32_t* bits, int rows, int cols, int wpr, double res, const double* x, const double* y,
                   unsigned char* out, long long n) {
    if (n <= 0 || rows < 0 || cols < 0 || wpr < (cols + 31) / 32) return n == 0 ? 0 : (int)hipErrorInvalidValue;
    Bufs b;
    const PPGrid g = make_grid(b, bits, rows, cols, wpr, res);
    const double* dx = b.in(x, (size_t)n);
    const double* dy = b.in(y, (size_t)n);
    unsigned char* o = b.alloc<unsigned char>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_is_blocked, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, g, dx, dy, o, n);
    b.ran();
    b.out(out, o, (size_t)n);
    return (int)b.err;
}
int ppp_blocked_cell(const uint32_t* bits, int rows, int cols, int wpr, double res, const double* x, const double* y,
                     unsigned char* outside, unsigned* row, unsigned* col, unsigned char* blocked, long long n) {
    if (n <= 0 || rows < 0 || cols < 0 || wpr < (cols + 31) / 32) return n == 0 ? 0 : (int)hipErrorInvalidValue;
    Bufs b;
    const PPGrid g = make_grid(b, bits, rows, cols, wpr, res);
    const double* dx = b.in(x, (size_t)n);
    const double* dy = b.in(y, (size_t)n);
    unsigned char* o = b.alloc<unsigned char>((size_t)n);
    unsigned* r = b.alloc<unsigned>((size_t)n);
    unsigned* c = b.alloc<unsigned>((size_t)n);
    unsigned char* bl = b.alloc<unsigned char>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_blocked_cell, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, g, dx, dy, o, r, c, bl, n);
    b.ran();
    b.out(outside, o, (size_t)n);
    b.out(row, r, (size_t)n);
    b.out(col, c, (size_t)n);
    b.out(blocked, bl, (size_t)n);
    return (int)b.err;
}

int ppp_line_distance_lt(const double* num, const double* sqL, const double* lim, unsigned char* out, long long n) {
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    const double* dn = b.in(num, (size_t)n);
    const double* ds = b.in(sqL, (size_t)n);
    const double* dl = b.in(lim, (size_t)n);
    unsigned char* o = b.alloc<unsigned char>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_line_distance_lt, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dn, ds, dl, o, n);
    b.ran();
    b.out(out, o, (size_t)n);
    return (int)b.err;
}

// obst12: n rows of PPObst (12 doubles each: X, Y, cosYaw, sinYaw, Speed, Time, halfL, halfW, reach, pad x 3), row i tested against point i
int ppp_obstacle_hit(const double* obst12, const double* x, const double* y, const double* t, int* out, long long n) {
    static_assert(sizeof(PPObst) == 12 * sizeof(double), "PPObst is 12 doubles");
    if (n <= 0) return n < 0 ? (int)hipErrorInvalidValue : 0;
    Bufs b;
    const PPObst* dob = b.in((const PPObst*)obst12, (size_t)n);
    const double* dx = b.in(x, (size_t)n);
    const double* dy = b.in(y, (size_t)n);
    const double* dt = b.in(t, (size_t)n);
    int* o = b.alloc<int>((size_t)n);
    if (b.err != hipSuccess) return (int)b.err;
    hipLaunchKernelGGL(probe_k_obstacle_hit, dim3(nblk(n)), dim3(PROBE_BLOCK), 0, 0, dob, dx, dy, dt, o, n);
    b.ran();
    b.out(out, o, (size_t)n);
    return (int)b.err;
}
}  // extern "C"
