"""The exact subset table of the point-robot TSP heuristics (path_planner_amd/csrc/pp_k_tsp_table.h), restated in numpy and held to
the oracle's literal recursion (RibbonManager.cpp:53-94) bit for bit; the ABI of the switch.  No GPU.

The recursion accumulates soFar' = fmax(soFar + len - 2w + dist, 0) and takes fmin over the leaves.  Each step is non-decreasing
in soFar, so the minimum over every tour that reaches (ribbons done, last ribbon, end entered) can be taken before the next step:
2^n 2n states instead of n! 2^n leaves, the same bits.  Under the K variant the ribbons that may be entered from a state are the
first min(K, remaining) of a stable descending sort; that set belongs to the state unless the K-th and (K+1)-th keys are equal, and
a list with such a tie in a reachable state is refused (`tsp_table` returns refused = True)."""
import re
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = np.finfo(np.float64).max
H_ALL, H_K = 1, 2


def tsp_table(ribbons4, heuristic, K, x, y, w):
    """(distance, refused) of TspPointRobotNoSplitAllRibbons (heuristic 1) / ...KRibbons (2) from (x, y), ribbon width w: the table
    G[S][2r + e], filled layer by layer in popcount(S), every layer as whole arrays."""
    r = np.asarray(ribbons4, dtype=np.float64).reshape(-1, 4)
    n = len(r)
    if n == 0:
        return 0.0, False
    kvar = heuristic == H_K
    if kvar and K <= 0:
        return DBL_MAX, False
    px = np.concatenate([[x], r[:, [0, 2]].ravel()])        # point 0 = query, 1 + 2i / 2 + 2i = start / end of ribbon i
    py = np.concatenate([[y], r[:, [1, 3]].ravel()])
    dx, dy = px[:, None] - px[None, :], py[:, None] - py[None, :]
    T = np.sqrt(dx * dx + dy * dy)
    KM = np.minimum(T[:, 1::2], T[:, 2::2])                 # [point][ribbon]: distance to its nearer endpoint
    length = T[1 + 2 * np.arange(n), 2 + 2 * np.arange(n)]
    twoW = 2 * w
    bits = 1 << np.arange(n)
    exits = np.array([2 + 2 * (j >> 1) if (j & 1) == 0 else 1 + 2 * (j >> 1) for j in range(2 * n)])   # where state j leaves its ribbon

    # per point and ribbon: the ribbons whose key from that point is greater than / equal to this one's, as bit masks
    GT = ((KM[:, None, :] > KM[:, :, None]) * bits[None, None, :]).sum(axis=2)
    EQ = ((KM[:, None, :] == KM[:, :, None]) * bits[None, None, :]).sum(axis=2) - bits[None, :]      # (without itself)
    pop = np.array([bin(s).count("1") for s in range(1 << n)])

    def chosen(R, pt, reached):
        """The ribbons that may be entered from states (remaining set R[m], point pt[m]) as bit masks, and whether a reached one
        has a run of equal keys straddling the K-th place."""
        if not kvar:
            return R.copy(), False
        inR = (R[:, None] & bits[None, :]) != 0
        gt = pop[GT[pt] & R[:, None]]
        ge = gt + pop[EQ[pt] & R[:, None]]
        tie = inR & (gt < K) & (ge >= K) & reached[:, None]
        return ((inR & (ge < K)) * bits[None, :]).sum(axis=1), bool(tie.any())

    full = (1 << n) - 1
    S_all = np.arange(1 << n)
    G = np.full((1 << n, 2 * n), -1.0)
    M = np.zeros((1 << n, 2 * n), dtype=np.int64)
    m0, tie = chosen(np.array([full]), np.array([0]), np.array([True]))
    if tie:
        return 0.0, True
    for k in range(1, n + 1):
        S = S_all[pop == k]
        for ri in range(n):
            Sk = S[(S & bits[ri]) != 0]
            Sp = Sk ^ bits[ri]
            for e in (0, 1):
                entry = 1 + 2 * ri + e
                if k == 1:
                    ok = (m0[0] >> ri) & 1
                    G[Sk, 2 * ri + e] = np.fmax(0.0 + length[ri] - twoW + T[0, entry], 0) if ok else -1.0
                    continue
                g = G[Sp]                                    # [m][2n]: the row of S \ {r}
                valid = (g >= 0) & (((M[Sp] >> ri) & 1) != 0)
                cand = np.fmax(g + length[ri] - twoW + T[exits, entry][None, :], 0)
                best = np.where(valid, cand, np.inf).min(axis=1)
                G[Sk, 2 * ri + e] = np.where(np.isfinite(best), best, -1.0)
        if k < n:                                            # what may be entered from the new states
            for j in range(2 * n):
                Sj = S[(S & bits[j >> 1]) != 0]
                m, tie = chosen(full ^ Sj, np.full(len(Sj), exits[j]), G[Sj, j] >= 0)
                if tie:
                    return 0.0, True
                M[Sj, j] = m
    last = G[full]
    return float(last[last >= 0].min()), False


def random_list(rng, n, w, short=0.3):
    """n ribbons in a 200 m box; a share of them pieces between w and 2.5 w long, so len - 2w goes negative and the clamp works."""
    a = rng.uniform(0, 200, (n, 2))
    ang = rng.uniform(0, 2 * np.pi, n)
    ln = np.where(rng.random(n) < short, rng.uniform(w, 2.5 * w, n), rng.uniform(5, 80, n))
    return np.column_stack([a, a[:, 0] + ln * np.cos(ang), a[:, 1] + ln * np.sin(ang)])


def mirror_pairs(n, x, y):
    """n ribbons in mirror pairs about (x, y) (the odd one on the axis, nearest): every other key from the query point comes twice,
    the largest among them."""
    out = []
    for i in range(n // 2):
        d, s = 6.0 + 4.0 * i, 3.0 + 1.5 * i
        out.append([x + d, y - s, x + d, y + s + 10])
        out.append([x - d, y - s, x - d, y + s + 10])
    if n % 2:
        out.append([x - 4.0, y + 3.0, x + 4.0, y + 3.0])
    return np.array(out)


VARIANTS = [(H_ALL, 0), (H_K, 0), (H_K, 1), (H_K, 2), (H_K, 3)]


def test_table_is_the_literal_recursion_bit_for_bit():
    import oracle as orc
    w = 1.5
    before = orc.O.ppo_get_ribbon_width()
    orc.O.ppo_set_ribbon_width(w)
    try:
        rng = np.random.default_rng(20261018)
        compared = refused_random = n_random = 0
        for case in range(420):
            n = 1 + case % 7
            heuristic, K = VARIANTS[(case // 7) % len(VARIANTS)]
            rib = random_list(rng, n, w)
            if case % 11 == 0 and n >= 2:                      # a shared endpoint: zero distances, equal keys inside a set
                rib[1, :2] = rib[0, 2:]
            x, y = rng.uniform(0, 200, 2)
            got, refused = tsp_table(rib, heuristic, K, x, y, w)
            n_random += 1
            if refused:
                refused_random += 1
                continue
            want = orc.ribbons_heuristic(rib, heuristic, K, x, y)
            assert got == want, (case, n, heuristic, K, got, want)
            compared += 1
        assert refused_random * 10 <= n_random, (refused_random, n_random)
        assert compared >= 350
        # deliberately tied lists: the K variant refuses where the tie straddles the K-th place, the All variant answers
        tied_refused = 0
        for n in (2, 4, 5, 6):
            rib = mirror_pairs(n, 100.0, 100.0)
            got, refused = tsp_table(rib, H_ALL, 0, 100.0, 100.0, w)
            assert not refused and got == orc.ribbons_heuristic(rib, H_ALL, 0, 100.0, 100.0)
            for K in (1, 2, 3):
                got, refused = tsp_table(rib, H_K, K, 100.0, 100.0, w)
                tied_refused += int(refused)
                if not refused:
                    assert got == orc.ribbons_heuristic(rib, H_K, K, 100.0, 100.0), (n, K)
        assert tied_refused >= 4
        # equally spaced parallel lines from a point off the axis: ties only between states, never across a K-th place at the root
        lines = np.array([[10.0, 10.0 + 5 * i, 60.0, 10.0 + 5 * i] for i in range(6)])
        for heuristic, K in VARIANTS:
            got, refused = tsp_table(lines, heuristic, K, 3.0, 1.0, w)
            if not refused:
                assert got == orc.ribbons_heuristic(lines, heuristic, K, 3.0, 1.0), (heuristic, K)
    finally:
        orc.O.ppo_set_ribbon_width(before)


def test_switch_is_declared_exported_and_bound():
    from path_planner_amd import api
    text = open(os.path.join(ROOT, "include", "ppgpu.h")).read()
    assert re.search(r"int\s+ppgpu_set_tsp_table\s*\(\s*ppgpu_ctx\*\s*\w+,\s*int32_t\s+min_ribbons,\s*int32_t\s+max_ribbons\s*\)\s*;", text)
    assert re.search(r"int\s+ppgpu_tsp_table_stats\s*\(\s*ppgpu_ctx\*\s*\w+,\s*uint64_t\*\s*lists,\s*uint64_t\*\s*refused\s*\)\s*;", text)
    for name in ("ppgpu_set_tsp_table", "ppgpu_tsp_table_stats"):
        assert name in api.EXPORTS and hasattr(api.LIB, name)
    assert hasattr(api.Context, "set_tsp_table") and hasattr(api.Context, "tsp_table_stats")
