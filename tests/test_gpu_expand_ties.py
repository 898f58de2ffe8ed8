"""-m gpu: the push-order pipeline (ppgpu_expand_order: probe, near list, bound, candidates, ring filter, sort, replay) on inputs
whose costs and distances tie and whose rings are crowded — what a random world never draws and sixty lines of pp_k_expand.h exist
for.  The reference is the oracle's literal scan with libstdc++'s own heap steps, visiting in the order the device documents for
equal distances: ascending (distance, sample index) (World.expand_order_by_index).  Every comparison is exact.

One radius (coverage_turning_radius = turning_radius) and one vertex per call wherever a list may fall back, so that the fallback
count of a call belongs to one list.  The "precondition" assertions are about the INPUTS, computed from the device's own rows of
lengths and numpy distances: a case that stops reaching its branch fails instead of passing for nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X0, Y0 = 128.0, 128.0                  # the root of config 1; heading 0 looks along +y
ORD_INNER, ORD_RING_MIN, ORD_CAP, BOUND_SLOTS = 1024, 512, 8192, 512 * 32      # PP_ORD_INNER, the ring filter's list size, PP_ORD_CAP, PP_BOUND_CAP x 32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _vertices(poses):
    from path_planner_amd import workloads
    from path_planner_amd.types import VERTEX_DTYPE
    root = workloads.config1().root()
    v = np.zeros(len(poses), dtype=VERTEX_DTYPE)
    for i, (x, y, h) in enumerate(poses):
        v[i] = root[0]
        v[i]["x"], v[i]["y"], v[i]["heading"] = x, y, h
    return v


SIX = [(X0, Y0, 0.0), (X0 + 1.5, Y0 - 0.75, 0.4), (X0 - 2.25, Y0 + 1.0, 5.9), (X0 + 0.5, Y0 + 2.5, 1.1), (X0 - 1.0, Y0 - 2.0, 3.0),
       (X0 + 3.0, Y0 + 0.25, 2.0)]


class OneRadius:
    """Config 1 with one radius, a sample set of the test's own, one vertex per call."""

    def __init__(self, torch, sx, sy, sh):
        from path_planner_amd import api, workloads
        import oracle as orc
        self.torch = torch
        self.w = workloads.config1()
        self.w.cfg.coverage_turning_radius = self.w.cfg.turning_radius
        self.S = [np.ascontiguousarray(a, dtype=np.float64) for a in (sx, sy, sh)]
        self.n = len(self.S[0])
        self.ctx = api.Context(0)
        self.ctx.set_config(self.w.cfg); self.ctx.set_grid(None, 0.0); self.ctx.set_obstacles(None)
        self.ctx.set_vertices(self.w.root(), self.w.ribbons4)
        self.ctx.set_samples(*self.S)
        self.world = orc.World(self.w.cfg, None, 0.0, None)
        self.vertex = None

    def at(self, v1):
        """Make v1 (one vertex) the open vertex; -> (the device's row of lengths, -1 = closer than the increment; numpy distances)."""
        self.vertex = v1
        self.ctx.set_vertices(v1, self.w.ribbons4)
        d_len = self.torch.zeros(self.n * 2, dtype=self.torch.float64, device="cuda:0")
        self.torch.cuda.synchronize()      # the fill ran on torch's stream, the library works on its own
        self.ctx.dubins_lengths(0, 1, d_len.data_ptr()); self.ctx.synchronize()
        L = d_len.cpu().numpy().reshape(self.n, 2)
        assert np.array_equal(L[:, 0], L[:, 1])             # one radius
        dx, dy = self.S[0] - v1["x"][0], self.S[1] - v1["y"][0]
        return L[:, 0].copy(), np.sqrt(dx * dx + dy * dy)    # State::distanceTo, term for term

    def order(self, k):
        idx, fb = self.ctx.expand_order(1, k)
        assert (idx[0, 1] == -1).all()                      # the radius not in use
        return idx[0, 0], fb

    def oracle(self, k):
        v = self.vertex
        src = np.array([v["x"][0], v["y"][0], v["heading"][0], v["speed"][0], v["time"][0]])
        return self.world.expand_order_by_index(src, *self.S, k)[0]


def _kth_length(L, k):
    return np.sort(L[L >= 0])[k - 1]


def _ascending(L, k):
    ok = np.nonzero(L >= 0)[0]
    order = ok[np.lexsort((ok, L[ok]))][:k]
    out = np.full(k, -1, dtype=np.int32)
    out[:len(order)] = order
    return out


def _exact_with_ties(torch, sx, sy, sh, ks, poses):
    """Every (vertex, k): no fallback, the by-index oracle's array.  -> per call (winners, lengths row, distances)."""
    run = OneRadius(torch, sx, sy, sh)
    assert run.n <= ORD_RING_MIN                             # the candidate list cannot reach the ring filter: every tie is replayed
    calls = []
    for pose in poses:
        L, d = run.at(_vertices([pose]))
        for k in ks:
            idx, fb = run.order(k)
            want = run.oracle(k)
            assert fb == 0, (pose, k, fb)
            assert np.array_equal(idx, want), (pose, k, idx.tolist(), want.tolist())
            calls.append((idx[idx >= 0], L, d))
    return calls


def test_duplicates_in_a_short_list(torch_cuda):
    """(a) 300 samples, 8 poses of which appear 2 to 6 times each at scattered indices — four of them close ahead of the vertices (among
    the winners), four anywhere: equal costs meet in the heap, and equal distances are visited in index order."""
    rng = np.random.default_rng(41)
    n = 300
    sx, sy, sh = X0 + rng.uniform(-60, 60, n), Y0 + rng.uniform(-60, 60, n), rng.uniform(0, 2 * np.pi, n)
    slots = rng.permutation(n)
    at = 0
    for j in range(8):
        copies = int(rng.integers(2, 7))
        if j < 4:
            pose = (X0 + rng.uniform(-3, 3), Y0 + rng.uniform(8, 20), rng.uniform(-0.3, 0.3) % (2 * np.pi))
        else:
            pose = (X0 + rng.uniform(-60, 60), Y0 + rng.uniform(-60, 60), rng.uniform(0, 2 * np.pi))
        for s in slots[at:at + copies]:
            sx[s], sy[s], sh[s] = pose
        at += copies
    calls = _exact_with_ties(torch_cuda, sx, sy, sh, (5, 9, 20), SIX)
    # precondition: winners of bit-equal length
    tied = sum(int(len(np.unique(L[win])) < len(win)) for win, L, d in calls)
    print(f"duplicates, short list: {tied} of {len(calls)} calls have winners of bit-equal length")
    assert tied > 0


def test_equal_distances_with_different_costs(torch_cuda):
    """(b) Groups of 4 to 8 samples on one spot with different headings, at scattered indices (list position and sample index
    disagree), and pairs mirrored through the first vertex: equal distances, different costs.  The visit order among them decides
    which get into the heap before it is full and where they end up."""
    rng = np.random.default_rng(42)
    n = 300
    sx = X0 + np.round(rng.uniform(-60, 60, n) * 8) / 8      # multiples of 1/8: every difference below is exact
    sy = Y0 + np.round(rng.uniform(-60, 60, n) * 8) / 8
    sh = rng.uniform(0, 2 * np.pi, n)
    slots = rng.permutation(n)
    at = 0
    for j in range(14):
        size = int(rng.integers(4, 9))
        r, th = rng.uniform(3, 22), rng.uniform(0, 2 * np.pi)
        gx, gy = X0 + round(r * np.sin(th) * 8) / 8, Y0 + round(r * np.cos(th) * 8) / 8
        g = slots[at:at + size]
        sx[g], sy[g] = gx, gy
        at += size
    mirrored = []
    for j in range(20):
        a, b = round(rng.uniform(-20, 20) * 8) / 8, round(rng.uniform(2, 20) * 8) / 8
        p, q = slots[at], slots[at + 1]
        sx[p], sy[p], sx[q], sy[q] = X0 + a, Y0 + b, X0 - a, Y0 - b
        mirrored.append((p, q))
        at += 2
    calls = _exact_with_ties(torch_cuda, sx, sy, sh, (5, 9, 20), SIX)
    d0 = calls[0][2]                                          # distances from the first vertex
    assert sum(int(d0[p] == d0[q]) for p, q in mirrored) == len(mirrored)       # tie bit for bit, by construction of the coordinates
    # precondition: a group of equal distance with members among the winners and members left out
    straddles = mirror_straddles = 0
    for win, L, d in calls:
        inside = np.zeros(n, dtype=bool)
        inside[win] = True
        valid = L >= 0
        for s in win:
            same = valid & (d == d[s])
            straddles += int((same & ~inside).any())
    for win, L, d in calls[:3]:                               # the first vertex's calls: the mirrored pairs tie there
        inside = np.zeros(n, dtype=bool)
        inside[win] = True
        mirror_straddles += sum(int(inside[p] != inside[q]) for p, q in mirrored)
    print(f"equal distances: {straddles} winners share their distance with a sample left out; {mirror_straddles} mirrored pairs split")
    assert straddles > 0


def _behind(rng, n, lo, hi, rho):
    """n poses behind a vertex at (X0, Y0) looking along +y, lo .. hi turning radii away (more of them near lo), looking the way the vertex
    looks: short distances, and curves of two half turns and more."""
    u = rng.random(n)
    d = rho * (lo + (hi - lo) * u * u)
    th = np.pi + rng.uniform(-0.3, 0.3, n)
    return X0 + d * np.sin(th), Y0 + d * np.cos(th), rng.uniform(-0.2, 0.2, n) % (2 * np.pi)


def _spread(rng, n, half):
    return X0 + rng.uniform(-half, half, n), Y0 + rng.uniform(-half, half, n), rng.uniform(0, 2 * np.pi, n)


def _crowded(seed, rings, n_spread, half):
    rng = np.random.default_rng(seed)
    parts = [_behind(rng, n, lo, hi, 8.0) for n, lo, hi in rings] + [_spread(rng, n_spread, half)]
    sx, sy, sh = [np.concatenate([p[i] for p in parts]) for i in range(3)]
    order = rng.permutation(len(sx))
    return sx[order], sy[order], sh[order]


def test_crowded_ring(torch_cuda):
    """(c) 6 000 samples, 5 000 of them 1.5 to 4 turning radii behind the vertex and looking past it, 1 000 spread over a square of
    1.2 km: the first ring of the filter (a quarter of the bound) holds more than PP_ORD_INNER candidates and is halved."""
    k = 20
    sx, sy, sh = _crowded(43, [(5000, 1.5, 4.0)], 1000, 600.0)
    run = OneRadius(torch_cuda, sx, sy, sh)
    assert run.w.cfg.turning_radius == 8.0
    L, d = run.at(_vertices([SIX[0]]))
    assert len(np.unique(d)) == len(d)                       # no duplicates, no ties: only the ring's crowding is on trial
    Lk = _kth_length(L, k)
    inner, cands = int(((L >= 0) & (d <= Lk / 4)).sum()), int(((L >= 0) & (d <= Lk)).sum())
    print(f"crowded ring: L_k {Lk:.3f}, {inner} valid samples within L_k / 4, {cands} within L_k")
    assert inner > ORD_INNER and cands > ORD_RING_MIN        # preconditions (the bound U is at least L_k)
    idx, fb = run.order(k)
    assert fb == 0
    assert np.array_equal(idx, run.oracle(k)), (idx.tolist(), run.oracle(k).tolist())


def test_crowded_ring_of_a_list_longer_than_the_replay_holds(torch_cuda):
    """More candidates than PP_ORD_CAP, so the replay depends on what the ring filter drops: 12 300 samples behind the vertex in three
    bands (300 within 0.3 to 0.6 turning radii, 3 000 within 0.9 to 1.4, 9 000 within 2 to 4).  The first ring (a quarter of the bound,
    about 1.6 radii) holds more than PP_ORD_INNER; halved it holds the 300, whose k-th cost is the threshold.  A filter that fails to
    find a threshold keeps everything, and the list falls back."""
    k = 9
    sx, sy, sh = _crowded(44, [(300, 0.3, 0.6), (3000, 0.9, 1.4), (9000, 2.0, 4.0)], 0, 0.0)
    run = OneRadius(torch_cuda, sx, sy, sh)
    L, d = run.at(_vertices([SIX[0]]))
    Lk = _kth_length(L, k)
    valid = L >= 0
    inner, halved, cands = int((valid & (d <= Lk / 4)).sum()), int((valid & (d <= Lk / 8)).sum()), int((valid & (d <= Lk)).sum())
    print(f"crowded ring, long list: L_k {Lk:.3f}, {inner} within L_k / 4, {halved} within L_k / 8, {cands} within L_k")
    assert inner > ORD_INNER and cands > ORD_CAP and halved >= k
    idx, fb = run.order(k)
    assert fb == 0
    assert np.array_equal(idx, run.oracle(k)), (idx.tolist(), run.oracle(k).tolist())


def test_merged_runs_of_the_bound(torch_cuda):
    """(d) Config 3, 20 000 samples, k = 40: above 32 every valid sample is on the near list, more than PP_BOUND_CAP x 32 slots, so
    pp_k_expand_bound ranks minima of runs of groups.  Root and two children, both radii, against the oracle's scan."""
    from path_planner_amd import workloads
    from path_planner_amd.types import F_INFEASIBLE
    from test_gpu_parity import _children_as_vertices, _dense, _setup
    k = 40
    w = workloads.by_name("cfg3")
    ctx, world, n, cs = _setup(w, 20000)
    gpu, gchild = _dense(torch_cuda, ctx, 1, 512, 0xF)
    feas = np.nonzero((gpu["flags"] & F_INFEASIBLE) == 0)[0]
    verts, pool = _children_as_vertices(w, gpu, gchild, feas[[len(feas) // 3, 2 * len(feas) // 3]])
    assert len(verts) == 3
    for v in range(3):
        far = int((np.sqrt((cs[:, 0] - verts["x"][v]) ** 2 + (cs[:, 1] - verts["y"][v]) ** 2) > w.cfg.collision_checking_increment).sum())
        assert far > BOUND_SLOTS, (v, far)                  # precondition: the near list is longer than the bound kernel ranks one by one
    ctx.set_vertices(verts, pool)
    idx, fb = ctx.expand_order(3, k)
    assert fb == 0
    for v in range(3):
        src = np.array([verts["x"][v], verts["y"][v], verts["heading"][v], verts["speed"][v], verts["time"][v]])
        d = np.sqrt((cs[:, 0] - src[0]) ** 2 + (cs[:, 1] - src[1]) ** 2)
        assert len(np.unique(d)) == len(d)                   # untied: the reference's own visit order is defined
        want = world.expand_order(src, cs[:, 0], cs[:, 1], cs[:, 2], k)
        assert np.array_equal(idx[v], want), (v, idx[v].tolist(), want.tolist())
        assert np.array_equal(want, world.expand_order_by_index(src, cs[:, 0], cs[:, 1], cs[:, 2], k))


# (f) duplicates in a long list
F_SEEDS = list(range(50, 56))
F_K = 9


def _long_list_world(seed):
    """4 000 samples: 3 000 behind the vertices within 0.3 to 4 turning radii (long curves: hundreds of candidates within the k-th
    length), 1 000 spread over a square of 1.2 km.  -> (with duplicates, without): in the first, three of the poses cheapest from the
    first vertex are copied over 2 to 4 far samples each, at scattered indices."""
    import oracle as orc
    from path_planner_amd import workloads
    sx, sy, sh = _crowded(seed, [(3000, 0.3, 4.0)], 1000, 600.0)
    rng = np.random.default_rng(1000 + seed)
    w = workloads.config1()
    w.cfg.coverage_turning_radius = w.cfg.turning_radius
    L = orc.World(w.cfg, None, 0.0, None).dubins_lengths(_vertices([SIX[0]]), 0, 1, sx, sy, sh)[0][:, 0]
    by_length = np.argsort(np.where(L >= 0, L, np.inf))
    far = by_length[2000:]
    dx, dy, dh = sx.copy(), sy.copy(), sh.copy()
    targets = rng.permutation(far)
    at = 0
    for src in rng.choice(by_length[:24], 3, replace=False):
        copies = int(rng.integers(2, 5))
        for s in targets[at:at + copies]:
            dx[s], dy[s], dh[s] = sx[src], sy[src], sh[src]
        at += copies
    return (dx, dy, dh), (sx, sy, sh)


def test_duplicates_in_a_long_list(torch_cuda):
    """(f) The ring filter drops candidates on the strength of "a no-op whenever its turn comes"; equal costs in the heap can make that
    untrue (pp_ord_safe), and the list then falls back.  Per call: no fallback -> the by-index oracle's array, exactly; fallback ->
    ascending (length, sample index) of the device's own lengths, the same bytes on a second call.  The same worlds without the
    duplicates never fall back.  Over the family both kinds occur, and at most half of the calls fall back."""
    poses = [(X0 + a, Y0 + b, h) for a, b, h in [(0, 0, 0.0), (0.4, -0.3, 0.05), (-0.5, 0.2, 6.2), (0.2, 0.6, 0.1), (-0.3, -0.5, 6.25), (0.6, 0.1, 0.15)]]
    exact_tied = fell_back = calls = 0
    for seed in F_SEEDS:
        with_dups, without = _long_list_world(seed)
        for samples, control in ((without, True), (with_dups, False)):
            run = OneRadius(torch_cuda, *samples)
            for pose in poses:
                L, d = run.at(_vertices([pose]))
                Lk = _kth_length(L, F_K)
                assert int(((L >= 0) & (d <= Lk)).sum()) > ORD_RING_MIN      # precondition: the list reaches the ring filter
                idx, fb = run.order(F_K)
                assert fb in (0, 1)
                if control:
                    assert fb == 0, (seed, pose)
                    assert np.array_equal(idx, run.oracle(F_K)), (seed, pose, "control")
                    continue
                calls += 1
                if fb == 0:
                    assert np.array_equal(idx, run.oracle(F_K)), (seed, pose, idx.tolist(), run.oracle(F_K).tolist())
                    exact_tied += int(len(np.unique(L[idx[idx >= 0]])) < (idx >= 0).sum())
                else:
                    fell_back += 1
                    assert np.array_equal(idx, _ascending(L, F_K)), (seed, pose, idx.tolist(), _ascending(L, F_K).tolist())
                    idx2, fb2 = run.order(F_K)
                    assert fb2 == 1 and idx2.tobytes() == idx.tobytes()
    print(f"duplicates, long list: {calls} calls, {fell_back} fell back, {exact_tied} replayed exactly with equal lengths among the winners")
    assert exact_tied > 0 and fell_back > 0
    assert 2 * fell_back <= calls
