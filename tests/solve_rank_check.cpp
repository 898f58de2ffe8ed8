// Host check of path_planner_amd/csrc/pp_solve_rank.h (tests/test_solve_rank.py): the ranked Dubins solver — rank the six words on
// the library's atan2 / acos, evaluate only the contenders correctly rounded — against "all six correctly rounded", which is
// pp_dubins_shortest<true> of pp_device.h restated here.  Both must give the same (type, p0, p1, p2), bit for bit.
// The "library" of this check is glibc's atan2 / acos moved by up to PP_RANK_LIB_ULPS ulp (a fixed function of the argument's bits), so
// that the ranking sees errors as large as the header assumes for the device's library.  mod2pi is the reference's
// t - 2 pi floor(t / 2 pi), which is what pp_mod2pi of pp_device.h returns.
// usage: solve_rank_check N   — N random problems after the fixed adversarial list.  Prints one line:
//     cases <n> mismatches <n> multi_contender <n> fallback <n> words_evaluated <n> no_path <n>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../path_planner_amd/csrc/pp_solve_rank.h"

static const double TWO_PI = 6.283185307179586476925286766559;
static uint64_t bits_of(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }
static uint64_t mix(uint64_t z) { z += 0x9e3779b97f4a7c15ull; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
static double move_ulps(double v, uint64_t h) {
    int k = (int)(h % (2 * (int)PP_RANK_LIB_ULPS + 1)) - (int)PP_RANK_LIB_ULPS;
    for (; k > 0; k--) v = nextafter(v, INFINITY);
    for (; k < 0; k++) v = nextafter(v, -INFINITY);
    return v;
}
struct Ops {
    static double mod2pi(double t) { return t - TWO_PI * floor(t / TWO_PI); }
    // exact where the solver relies on the library being exact: zeros, the axes, +-1, non-finite input
    static double atan2(double y, double x) {
        const double t0 = ::atan2(y, x);
        if (x == 0.0 || y == 0.0 || !(fabs(t0) > 1e-300) || !std::isfinite(x) || !std::isfinite(y)) return t0;
        return move_ulps(t0, mix(bits_of(y) ^ mix(bits_of(x))));
    }
    static double acos(double v) {
        const double t0 = ::acos(v);
        if (!(fabs(v) < 1.0) || t0 == 0.0) return t0;
        const double m = move_ulps(t0, mix(bits_of(v)));
        return m > 0.0 ? m : t0;
    }
};
static void cr_sincos(double x, double* s, double* c) { PPdd S, C; pp_cr_sincos_dd(x, &S, &C); *s = S.h + S.l; *c = C.h + C.l; }
static double cr_atan2(double y, double x) {
    const double t0 = Ops::atan2(y, x);
    if (x == 0.0 || y == 0.0 || !(fabs(t0) > 1e-300) || !std::isfinite(x) || !std::isfinite(y)) return t0;
    PPdd s, c; pp_cr_sincos_dd(t0, &s, &c); return pp_cr_atan2_step(y, x, t0, s, c);
}
static double cr_acos(double v) {
    const double t0 = Ops::acos(v);
    if (!(fabs(v) < 1.0) || t0 == 0.0) return t0;
    PPdd s, c; pp_cr_sincos_dd(t0, &s, &c); return pp_cr_acos_step(v, t0, s, c);
}
struct Path { int type; double p0, p1, p2; };

// the words of pp_dubins_shortest<true>, from the normalised problem on
static Path all_six(const PPWordIn& in) {
    const double d = in.d, d_sq = in.d_sq, alpha = in.alpha, beta = in.beta, sa = in.sa, ca = in.ca, sb = in.sb, cb = in.cb, c_ab = in.c_ab;
    double best = INFINITY, t, p, q;
    Path out = {-1, 0, 0, 0};
    {  // LSL
        double tmp0 = d + sa - sb;
        double p_sq = 2 + d_sq - (2 * c_ab) + (2 * d * (sa - sb));
        if (p_sq >= 0) {
            double tmp1 = cr_atan2((cb - ca), tmp0);
            t = Ops::mod2pi(tmp1 - alpha);
            p = sqrt(p_sq);
            q = Ops::mod2pi(beta - tmp1);
            double cost = t + p + q;
            if (cost < best) { best = cost; out = Path{0, t, p, q}; }
        }
    }
    {  // LSR
        double p_sq = -2 + (d_sq) + (2 * c_ab) + (2 * d * (sa + sb));
        if (p_sq >= 0) {
            p = sqrt(p_sq);
            double tmp0 = cr_atan2((-ca - cb), (d + sa + sb)) - cr_atan2(-2.0, p);
            t = Ops::mod2pi(tmp0 - alpha);
            q = Ops::mod2pi(tmp0 - Ops::mod2pi(beta));
            double cost = t + p + q;
            if (cost < best) { best = cost; out = Path{1, t, p, q}; }
        }
    }
    {  // RSL
        double p_sq = -2 + d_sq + (2 * c_ab) - (2 * d * (sa + sb));
        if (p_sq >= 0) {
            p = sqrt(p_sq);
            double tmp0 = cr_atan2((ca + cb), (d - sa - sb)) - cr_atan2(2.0, p);
            t = Ops::mod2pi(alpha - tmp0);
            q = Ops::mod2pi(beta - tmp0);
            double cost = t + p + q;
            if (cost < best) { best = cost; out = Path{2, t, p, q}; }
        }
    }
    {  // RSR
        double tmp0 = d - sa + sb;
        double p_sq = 2 + d_sq - (2 * c_ab) + (2 * d * (sb - sa));
        if (p_sq >= 0) {
            double tmp1 = cr_atan2((ca - cb), tmp0);
            t = Ops::mod2pi(alpha - tmp1);
            p = sqrt(p_sq);
            q = Ops::mod2pi(tmp1 - beta);
            double cost = t + p + q;
            if (cost < best) { best = cost; out = Path{3, t, p, q}; }
        }
    }
    {  // RLR
        double tmp0 = (6. - d_sq + 2 * c_ab + 2 * d * (sa - sb)) / 8.;
        double phi = cr_atan2(ca - cb, d - sa + sb);
        if (fabs(tmp0) <= 1) {
            p = Ops::mod2pi((TWO_PI) - cr_acos(tmp0));
            t = Ops::mod2pi(alpha - phi + Ops::mod2pi(p / 2.));
            q = Ops::mod2pi(alpha - beta - t + Ops::mod2pi(p));
            double cost = t + p + q;
            if (cost < best) { best = cost; out = Path{4, t, p, q}; }
        }
    }
    {  // LRL
        double tmp0 = (6. - d_sq + 2 * c_ab + 2 * d * (sb - sa)) / 8.;
        double phi = cr_atan2(ca - cb, d + sa - sb);
        if (fabs(tmp0) <= 1) {
            p = Ops::mod2pi(TWO_PI - cr_acos(tmp0));
            t = Ops::mod2pi(-alpha - phi + p / 2.);
            q = Ops::mod2pi(Ops::mod2pi(beta) - alpha - t + Ops::mod2pi(p));
            double cost = t + p + q;
            if (cost < best) { best = cost; out = Path{5, t, p, q}; }
        }
    }
    return out;
}
// the preamble of pp_dubins_shortest<true>: two poses and a radius to the normalised problem
static PPWordIn normalise(double q0x, double q0y, double q0t, double q1x, double q1y, double q1t, double rho) {
    PPWordIn in;
    const double dx = q1x - q0x, dy = q1y - q0y;
    const double D = sqrt(dx * dx + dy * dy);
    in.d = D / rho;
    double theta = 0;
    if (in.d > 0) theta = Ops::mod2pi(cr_atan2(dy, dx));
    in.alpha = Ops::mod2pi(q0t - theta);
    in.beta = Ops::mod2pi(q1t - theta);
    in.mbeta = Ops::mod2pi(in.beta);
    double unused;
    cr_sincos(in.alpha, &in.sa, &in.ca);
    cr_sincos(in.beta, &in.sb, &in.cb);
    cr_sincos(in.alpha - in.beta, &unused, &in.c_ab);
    in.d_sq = in.d * in.d;
    return in;
}
// a normalised problem given directly: d and the two angles as they are (no mod2pi), their sin / cos correctly rounded
static PPWordIn direct(double d, double alpha, double beta) {
    PPWordIn in;
    in.d = d; in.d_sq = d * d; in.alpha = alpha; in.beta = beta; in.mbeta = Ops::mod2pi(beta);
    double unused;
    cr_sincos(alpha, &in.sa, &in.ca);
    cr_sincos(beta, &in.sb, &in.cb);
    cr_sincos(alpha - beta, &unused, &in.c_ab);
    return in;
}
// ... and with the sin / cos given too (the exact zeros and ones that no angle's double gives)
static PPWordIn literal(double d, double alpha, double beta, double sa, double ca, double sb, double cb, double c_ab) {
    PPWordIn in = {d, d * d, alpha, beta, Ops::mod2pi(beta), sa, ca, sb, cb, c_ab};
    return in;
}

static uint64_t st = 0x2545f4914f6cdd1dull;
static double rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * (1.0 / 9007199254740992.0); }

static void adversarial(std::vector<PPWordIn>& v) {
    const double PI = 3.14159265358979323846;
    const double hs[] = {0.0, -0.0, PI / 2, -PI / 2, PI, -PI, PI / 4, 3 * PI / 4, 1.0, TWO_PI, 1e-12, -1e-12};
    const double rhos[] = {1.0, 8.0, 10.0, 0.3};
    for (double rho : rhos)
        for (double h0 : hs)
            for (double h1 : hs) {
                // target straight ahead and straight behind, along both axes and a diagonal
                const double ds[] = {0.5, 2.0, 4.0, 10.0, 1000.0};
                for (double L : ds) {
                    v.push_back(normalise(0, 0, h0, L * rho, 0, h1, rho));
                    v.push_back(normalise(0, 0, h0, -L * rho, 0, h1, rho));
                    v.push_back(normalise(3, -2, h0, 3, -2 + L * rho, h1, rho));
                    v.push_back(normalise(3, -2, h0, 3 - L * rho, -2 - L * rho, h1, rho));
                }
                v.push_back(normalise(7, 7, h0, 7, 7, h1, rho));                 // co-located poses
            }
    // mirror images: beta = -alpha (LSL / RSR tie), beta = alpha + pi, alpha = beta; short d so that RLR / LRL are feasible and tie
    for (int i = 0; i <= 64; i++) {
        const double a = TWO_PI * i / 64.0;
        const double ds[] = {0.0, 0.25, 1.0, 2.0, 3.0, 4.0, 4.0000001, 7.5, 300.0};
        for (double d : ds) {
            v.push_back(direct(d, a, Ops::mod2pi(-a)));
            v.push_back(direct(d, a, Ops::mod2pi(TWO_PI - a)));
            v.push_back(direct(d, a, Ops::mod2pi(a + PI)));
            v.push_back(direct(d, a, a));
            v.push_back(normalise(0, 0, a, d, 0, -a, 1.0));
            v.push_back(normalise(0, 0, a, 0, d, PI - a, 1.0));
        }
    }
    // p_sq exactly 0 (LSR at d = 2 between opposite headings, LSL / RSR at d = 0) and |tmp0| exactly 1 (d = 0 and d = 4, equal headings)
    v.push_back(literal(2.0, 0.0, PI, 0.0, 1.0, 0.0, -1.0, -1.0));
    v.push_back(literal(2.0, PI, 0.0, 0.0, -1.0, 0.0, 1.0, -1.0));
    v.push_back(literal(0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0));
    v.push_back(literal(4.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0));
    v.push_back(literal(4.0, 1.0, 1.0, sin(1.0), cos(1.0), sin(1.0), cos(1.0), 1.0));
    v.push_back(literal(0.0, 2.5, 2.5, sin(2.5), cos(2.5), sin(2.5), cos(2.5), 1.0));
    v.push_back(literal(nextafter(4.0, 5.0), 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0));
    v.push_back(literal(nextafter(4.0, 0.0), 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0));
    v.push_back(literal(nextafter(2.0, 0.0), 0.0, PI, 0.0, 1.0, 0.0, -1.0, -1.0));
    // a mod2pi argument within 1e-12 of 0 and of 2 pi: headings a hair off the line to the target, on either side, and off each other
    const double eps[] = {0.0, 1e-12, -1e-12, 3e-13, -3e-13, 1e-15, -1e-15, 1e-9, -1e-9, 5e-7, -5e-7, 2e-6, -2e-6};
    for (double ea : eps)
        for (double eb : eps) {
            const double ds[] = {0.5, 1.0, 3.0, 5.0, 40.0, 5000.0};
            for (double d : ds) {
                v.push_back(normalise(0, 0, ea, d, 0, eb, 1.0));
                v.push_back(normalise(0, 0, PI + ea, d, 0, PI + eb, 1.0));
                v.push_back(normalise(0, 0, ea, d, 0, PI + eb, 1.0));
                v.push_back(normalise(0, 0, PI / 2 + ea, d, 0, -PI / 2 + eb, 1.0));
                v.push_back(direct(d, Ops::mod2pi(ea), Ops::mod2pi(eb)));
                v.push_back(direct(d, Ops::mod2pi(1.0 + ea), Ops::mod2pi(1.0 + eb)));
                v.push_back(direct(d, TWO_PI + ea, eb < 0 ? TWO_PI + eb : eb));        // (2 pi itself is a value mod2pi returns)
            }
        }
    // d at the fallback threshold, and beyond every bound
    const double dd[] = {PP_RANK_MAX_D, nextafter(PP_RANK_MAX_D, 0.0), nextafter(PP_RANK_MAX_D, 1e9), 2 * PP_RANK_MAX_D, 1e9, 1e300, INFINITY, NAN};
    for (double d : dd)
        for (int i = 0; i < 16; i++) {
            v.push_back(direct(d, rnd() * TWO_PI, rnd() * TWO_PI));
            v.push_back(normalise(0, 0, rnd() * 7 - 3.5, d, 0, rnd() * 7 - 3.5, 1.0));
            v.push_back(normalise(0, 0, 0.0, d * 0.5, d * 0.5, 0.0, 0.70710678118654752440));
        }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 1000000;
    std::vector<PPWordIn> cases;
    adversarial(cases);
    const long n_fixed = (long)cases.size();
    long mism = 0, multi = 0, fallback = 0, words = 0, nopath = 0;
    for (long i = 0; i < n_fixed + n; i++) {
        PPWordIn in;
        if (i < n_fixed) in = cases[i];
        else {
            const int kind = (int)(i % 8);
            const double rho = (kind & 1) ? 8.0 : 0.5 + rnd() * 20.0;
            const double span = kind < 4 ? 100.0 : (kind < 6 ? 6.0 * rho : 3000.0);      // mostly CSC; short edges where CCC wins; far targets
            in = normalise(rnd() * span, rnd() * span, (rnd() * 2 - 1) * 3.2, rnd() * span, rnd() * span, (rnd() * 2 - 1) * 3.2, rho);
        }
        const Path ref = all_six(in);
        const unsigned mask = pp_rank_contenders<Ops>(in);
        Path got;
        pp_solve_contenders<Ops>(in, mask, got.p0, got.p1, got.p2, got.type);
        const int nc = __builtin_popcount(mask);
        words += nc;
        if (nc > 1) multi++;
        if (!(in.d <= PP_RANK_MAX_D)) fallback++;
        if (ref.type < 0) nopath++;
        if (got.type != ref.type || bits_of(got.p0) != bits_of(ref.p0) || bits_of(got.p1) != bits_of(ref.p1) || bits_of(got.p2) != bits_of(ref.p2)) {
            if (mism++ < 10)
                std::fprintf(stderr, "case %ld: d %a alpha %a beta %a: all six -> %d %a %a %a, ranked (mask %#x) -> %d %a %a %a\n", i, in.d, in.alpha, in.beta,
                             ref.type, ref.p0, ref.p1, ref.p2, mask, got.type, got.p0, got.p1, got.p2);
        }
    }
    std::printf("cases %ld fixed %ld mismatches %ld multi_contender %ld fallback %ld words_evaluated %ld no_path %ld\n", n_fixed + n, n_fixed, mism, multi, fallback, words, nopath);
    return 0;
}
