// pp_solve_rank.h — the Dubins solver of the planner's edges without the work its result does not need: the six words are RANKED on
// the library's atan2 / acos, and only the words that can still be the reference's choice are evaluated with the correctly rounded
// ones (pp_cr.h).  The result is, bit for bit, that of evaluating all six correctly rounded (pp_dubins_shortest<true>).
//
// Why it is the same.  Let eps bound |library angle - correctly rounded angle|.  A word's cost t + p + q is a continuous function
// of its angles (slope at most 5: the CCC words use acos in p, t and q) except where an argument of a mod2pi crosses a multiple of
// 2 pi, where it jumps by 2 pi.  A word none of whose mod2pi arguments (as ranked) lies within DELTA of such a multiple is CERTAIN: its
// correctly rounded cost is within E of the ranked one.  A certain word whose ranked cost exceeds the smallest certain ranked cost by
// more than DELTA > 2 E has a strictly larger correctly rounded cost than that word, so the reference, which keeps the first
// strictly-smallest cost in enum order, cannot choose it.  Every other feasible word — uncertain, or within DELTA of the certain
// minimum — is a CONTENDER; the contenders are evaluated correctly rounded in enum order with the reference's strict `<`.  The
// feasibility tests (p_sq >= 0, |tmp0| <= 1) use no inverse trig and are the reference's own.
//
// The bounds.  No accuracy of the device library's double atan2 / acos is documented with it, so PP_RANK_LIB_ULPS = 16 ulp is
// assumed: eps <= 16.5 ulp(pi) = 7.4e-15.  E <= 5 eps (3.7e-14) + a dozen roundings of angle-sized values (ulp(32) each, 4.3e-14) +
// the two roundings of t + p + q at the largest admitted d (ulp(2^16 + 32) = 1.5e-11): E < 1.6e-11 at d <= PP_RANK_MAX_D, and
// DELTA = 1e-6 is more than 10^4 times 2 E.  A lane whose d is beyond PP_RANK_MAX_D (or NaN), or whose ranked costs are not all
// finite, evaluates every feasible word correctly rounded, as pp_dubins_shortest<true> does.
//
// No six-way divergence.  Lanes of a wave win with different words, so the correctly rounded evaluation is written once for all
// words: a word is two angle requests (atan2(y, x), acos(v) or none, chosen by selects on the word's index), one shared
// pp_cr_sincos_dd + Newton step per request (pp_cr_angle), and the word's own expressions for t, p, q.  The loop over contenders is
// bounded by a counter; it runs once for almost every wave.
//
// Compiled for the device (pp_device.h) and for the host (tests/solve_rank_check.cpp), like pp_cr.h.  The library trig and the exact
// mod2pi come as the static members atan2 / acos / mod2pi of the template parameter O.
#pragma once
#include "pp_cr.h"
#ifndef PP_CR_MEMBER
#define PP_CR_MEMBER inline          // what PP_CR_FN is to a free function, for a member
#endif
#define PP_RANK_LIB_ULPS 16.0        // assumed error of the library's atan2 / acos (see above)
#define PP_RANK_MAX_D 65536.0        // largest d = distance / rho that is ranked
#define PP_RANK_DELTA 1.0e-6         // margin of a cost, and of a mod2pi argument from a multiple of 2 pi
#define PP_RANK_2PI 6.283185307179586476925286766559
#define PP_RANK_INV_2PI 0.15915494309189533576888376337251

// what all six words share: dubins_shortest_path's normalised problem (mbeta = mod2pi(beta), which LSR and LRL take)
struct PPWordIn { double d, d_sq, alpha, beta, mbeta, sa, ca, sb, cb, c_ab; };
// word w's requests: A = atan2(yA, xA) always; B = atan2(yB, xB) (kindB 1), acos(yB) (kindB 2) or nothing (kindB 0)
struct PPWordReq { bool feasible; int kindB; double yA, xA, yB, xB, aux; };    // aux: p_sq of a CSC word

// The expressions are dubins.c's, operand for operand (a - b is a + (-b) bit for bit, so the two signs of a term share a line).
PP_CR_FN PPWordReq pp_word_requests(int w, const PPWordIn& in) {
    PPWordReq r;
    const double sd = (w == 0 || w == 4) ? (in.sa - in.sb) : (in.sb - in.sa);              // LSL, RLR : RSR, LRL
    const double cross = 2 * in.d * (in.sa + in.sb);
    const double psq_same = 2 + in.d_sq - (2 * in.c_ab) + (2 * in.d * sd);                   // LSL, RSR
    const double psq_cross = -2 + in.d_sq + (2 * in.c_ab) + (w == 1 ? cross : -cross);      // LSR, RSL
    const double tmp0 = (6. - in.d_sq + 2 * in.c_ab + 2 * in.d * sd) / 8.;                   // RLR, LRL
    const double u = (w == 0 || w == 1 || w == 5) ? in.d + in.sa : in.d - in.sa;
    r.xA = (w == 0 || w == 2 || w == 5) ? u - in.sb : u + in.sb;
    r.yA = w == 0 ? (in.cb - in.ca) : w == 1 ? (-in.ca - in.cb) : w == 2 ? (in.ca + in.cb) : (in.ca - in.cb);
    r.aux = (w == 0 || w == 3) ? psq_same : psq_cross;
    r.feasible = w < 4 ? (r.aux >= 0) : (fabs(tmp0) <= 1);
    r.kindB = (w == 1 || w == 2) ? 1 : (w >= 4 ? 2 : 0);
    r.yB = w == 1 ? -2.0 : (w == 2 ? 2.0 : tmp0);
    r.xB = sqrt(r.aux);
    return r;
}
// t, p, q of word w from its two angles; `mod` is the mod2pi to use
template <class M>
PP_CR_FN void pp_word_assemble(int w, const PPWordIn& in, const PPWordReq& r, double A, double B, M& mod, double& t, double& p, double& q) {
    if (w < 4) {
        p = sqrt(r.aux);
        const double base = (w == 1 || w == 2) ? A - B : A;
        const double argT = (w <= 1) ? base - in.alpha : in.alpha - base;
        const double argQ = (w == 0 || w == 2) ? in.beta - base : (w == 1 ? base - in.mbeta : base - in.beta);
        t = mod(argT);
        q = mod(argQ);
    } else {
        p = mod(PP_RANK_2PI - B);
        const double ph = p / 2.;
        const double h = (w == 4) ? mod(ph) : ph;
        const double lead = (w == 4) ? in.alpha - A : -in.alpha - A;
        t = mod(lead + h);
        const double mp = mod(p);
        const double qb = (w == 4) ? in.alpha - in.beta : in.mbeta - in.alpha;
        q = mod(qb - t + mp);
    }
}
// mod2pi as the ranking takes it: the product form, and a note of any argument within DELTA of a multiple of 2 pi (or NaN)
struct PPRankMod {
    bool near;
    PP_CR_MEMBER double operator()(double t) {
        const double qq = t * PP_RANK_INV_2PI, k = floor(qq), fr = qq - k;
        const double g = PP_RANK_DELTA * PP_RANK_INV_2PI;
        near = near | !((fr > g) & (fr < 1.0 - g));
        return t - PP_RANK_2PI * k;
    }
};
template <class O>
struct PPExactMod { PP_CR_MEMBER double operator()(double t) { return O::mod2pi(t); } };

// One request, correctly rounded, from the library's value t0 of it: pp_cr_atan2 / pp_cr_acos (pp_device.h) as one sequence.
// kind 1: atan2(y, x); kind 2: acos(y).  Where those return the library's value (zeros, the axes, +-1, non-finite input) so does this.
PP_CR_FN double pp_cr_angle(int kind, double y, double x, double t0) {
    const bool special = (kind == 1) ? (x == 0.0 || y == 0.0 || !(fabs(t0) > 1e-300) || !(fabs(x) < INFINITY) || !(fabs(y) < INFINITY))
                                     : (!(fabs(y) < 1.0) || t0 == 0.0);
    PPdd s, c;
    pp_cr_sincos_dd(special ? 0.0 : t0, &s, &c);
    const double ra = pp_cr_atan2_step(y, x, t0, s, c), rc = pp_cr_acos_step(y, t0, s, c);
    return special ? t0 : (kind == 1 ? ra : rc);
}

// bit w: word w is a contender
template <class O>
PP_CR_FN unsigned pp_rank_contenders(const PPWordIn& in) {
    unsigned feas = 0, unc = 0;
    bool bad = !(in.d <= PP_RANK_MAX_D);
    double cost[6], cmin = INFINITY;
#pragma unroll
    for (int w = 0; w < 6; w++) {
        const PPWordReq r = pp_word_requests(w, in);
        const double A = O::atan2(r.yA, r.xA);
        const double B = r.kindB == 1 ? O::atan2(r.yB, r.xB) : (r.kindB == 2 ? O::acos(r.yB) : 0.0);
        PPRankMod m;
        m.near = false;
        double t, p, q;
        pp_word_assemble(w, in, r, A, B, m, t, p, q);
        const double c = t + p + q;
        const bool finite = fabs(c) < INFINITY;
        cost[w] = c;
        if (r.feasible) {
            feas |= 1u << w;
            if (!finite) bad = true;
            if (m.near || !finite) unc |= 1u << w;
            else cmin = fmin(cmin, c);
        }
    }
    unsigned mask = unc;
#pragma unroll
    for (int w = 0; w < 6; w++)
        if (((feas & ~unc) >> w) & 1u) { if (cost[w] <= cmin + PP_RANK_DELTA) mask |= 1u << w; }
    return bad ? feas : mask;
}

// the contenders, correctly rounded, in enum order: the first strictly-smallest t + p + q (type -1 and zeros when there is none)
template <class O>
PP_CR_FN void pp_solve_contenders(const PPWordIn& in, unsigned mask, double& p0, double& p1, double& p2, int& type) {
    double best = INFINITY;
    type = -1;
    p0 = p1 = p2 = 0;
    for (int it = 0; it < 6; it++) {
        if (mask == 0u) break;
        const int w = __builtin_ctz(mask);
        mask &= mask - 1u;
        const PPWordReq r = pp_word_requests(w, in);
        const double A = pp_cr_angle(1, r.yA, r.xA, O::atan2(r.yA, r.xA));
        double B = 0.0;
        if (r.kindB != 0) B = pp_cr_angle(r.kindB, r.yB, r.xB, r.kindB == 1 ? O::atan2(r.yB, r.xB) : O::acos(r.yB));
        PPExactMod<O> m;
        double t, p, q;
        pp_word_assemble(w, in, r, A, B, m, t, p, q);
        const double cost = t + p + q;
        if (cost < best) { best = cost; p0 = t; p1 = p; p2 = q; type = w; }
    }
}
