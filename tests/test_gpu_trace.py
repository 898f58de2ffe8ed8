"""-m gpu: per-step edge traces (ppgpu_trace_edges_* -> pp_k_trace_steps) against the CPU oracle, step by step.

Every world is built from fixed seeds with the oracle alone (samples, children of the root as further open vertices, which edges
to look at), so what the device is asked is the same on every run.  The device's poses are compared with the oracle's
dubins_path_sample on the record's curve; everything that is a function of a pose (isBlocked, collisionExists) is evaluated by
the oracle AT THE DEVICE'S POSE, so both sides see the same doubles."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * math.pi
FLIP_EPS = 1e-9          # a binary collision answer may differ only where the oracle's own answer flips within this distance
FLIP_CAP = 1e-3          # ... on at most this share of all steps


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class TraceWorld:
    """Oracle world + what to upload: config, grid, obstacles, open vertices with their ribbon pool, targets, an edge list."""

    def __init__(self, cfg, grid, res, obst=None, gauss=None):
        import oracle as orc
        self.cfg, self.grid, self.res, self.obst, self.gauss = cfg, grid, res, obst, gauss
        self.world = orc.World(cfg, grid, res, obst, gauss=gauss)
        self.binary = gauss is None

    def context(self):
        from path_planner_amd import api
        ctx = api.Context(0)
        ctx.set_config(self.cfg)
        ctx.set_grid(self.grid, self.res)
        if self.gauss is not None:
            ctx.set_gaussian_obstacles(self.gauss)
        else:
            ctx.set_obstacles(self.obst)
        ctx.set_vertices(self.verts, self.pool)
        ctx.set_samples(self.sx, self.sy, self.sh)
        return ctx


def _children(w_root, w_rib, res, child, pick):
    from path_planner_amd.types import VERTEX_DTYPE
    v = np.zeros(len(pick) + 1, dtype=VERTEX_DTYPE)
    pool = [np.asarray(w_rib, dtype=np.float64).reshape(-1, 4)]
    v[0] = w_root[0]
    off = len(pool[0])
    for k, e in enumerate(pick):
        r = res[e]
        nr = int((r["info"] >> 8) & 0xFF)
        v[k + 1] = (r["end_x"], r["end_y"], r["end_heading"], r["end_speed"], r["end_time"], r["g"], r["coverage_completed_time"], off, nr)
        pool.append(child[e, :nr])
        off += nr
    return v, np.concatenate(pool)


def _grow(tw, w, n_samples, n_children, seed, n_cand):
    """Samples of workload w, children of its root as further vertices, n_cand random (vertex, target, configuration) candidates
    costed by the oracle: returns (candidate descriptors, their oracle records)."""
    from path_planner_amd.types import F_INFEASIBLE, F_GOAL, edge_pack
    cs = tw.world.add_samples(w.bounds6, w.seed, w.ribbons4, 0, n_samples)
    tw.sx, tw.sy, tw.sh = cs[:, 0].copy(), cs[:, 1].copy(), cs[:, 2].copy()
    n = len(cs)
    e0 = edge_pack(np.zeros(4 * n, dtype=np.uint64), np.repeat(np.arange(n), 4), np.tile(np.arange(4), n))
    r0, c0 = tw.world.cost_edges(w.root(), w.ribbons4, tw.sx, tw.sy, tw.sh, e0, stride=10, threads=8)
    feas = np.nonzero(((r0["flags"] & F_INFEASIBLE) == 0) & ((r0["flags"] & F_GOAL) == 0))[0]
    pick = feas[:: max(1, len(feas) // n_children)][:n_children]
    tw.verts, tw.pool = _children(w.root(), w.ribbons4, r0, c0, pick)
    rng = np.random.default_rng(seed)
    vi, ti, cb = rng.integers(0, len(tw.verts), n_cand), rng.integers(0, n, n_cand), rng.integers(0, 4, n_cand)
    far = np.hypot(tw.verts["x"][vi] - tw.sx[ti], tw.verts["y"][vi] - tw.sy[ti]) > 2 * w.cfg.collision_checking_increment
    cand = edge_pack(vi[far], ti[far], cb[far])
    return cand, tw.world.cost_edges(tw.verts, tw.pool, tw.sx, tw.sy, tw.sh, cand, threads=8)


def _pick(groups, per):
    out = []
    for g in groups:
        g = np.asarray(g)
        out.extend(g[:: max(1, len(g) // per)][:per].tolist())
    return np.array(sorted(set(out)), dtype=np.int64)


def world_binary():
    """Config 3: a 2048^2 grid with blocked cells, 16 moving boxes; root + 30 of its children; edges that end on a blocked cell,
    edges that pass through boxes, and others."""
    from path_planner_amd import workloads
    from path_planner_amd.types import F_INFEASIBLE, F_THROWS
    w = workloads.config3(n_samples=512)
    tw = TraceWorld(w.cfg, w.grid, w.res, w.obst)
    cand, rec = _grow(tw, w, 512, 30, 5, 3000)
    steps = rec["info"] >> 16
    ok = (rec["flags"] & F_THROWS) == 0
    blocked = np.nonzero(ok & ((rec["flags"] & F_INFEASIBLE) != 0) & (steps > 0))[0]
    hit = np.nonzero(ok & (rec["collision_penalty"] > 0))[0]
    rest = np.nonzero(ok & ((rec["flags"] & F_INFEASIBLE) == 0) & (rec["collision_penalty"] == 0))[0]
    assert len(blocked) >= 12 and len(hit) >= 12, (len(blocked), len(hit))
    tw.edges = cand[_pick([blocked, hit, rest], 16)]
    return tw


def world_gaussian(cov):
    """Config 2's grid with 12 Gaussian obstacles, default or custom covariance (as tests/test_gpu_parity.py builds them)."""
    from path_planner_amd import workloads
    from path_planner_amd.types import F_INFEASIBLE
    w = workloads.config2()
    rng = np.random.default_rng(5)
    n_ob = 12
    root = w.root()
    rows = np.zeros((n_ob, 9 if cov == "custom" else 5))
    rows[:, 0] = root["x"][0] + rng.uniform(-70, 70, n_ob)
    rows[:, 1] = root["y"][0] + rng.uniform(-70, 70, n_ob)
    rows[:, 2] = rng.uniform(0, 2 * np.pi, n_ob)
    rows[:, 3] = rng.uniform(0, 3, n_ob)
    rows[:, 4] = root["time"][0] - rng.uniform(0, 5, n_ob)
    if cov == "custom":
        for i in range(n_ob):
            a, b = rng.uniform(4, 60), rng.uniform(4, 60)
            c = rng.uniform(-0.6, 0.6) * np.sqrt(a * b)
            rows[i, 5:] = [a, c, c, b]
    tw = TraceWorld(w.cfg, w.grid, w.res, gauss=rows)
    cand, rec = _grow(tw, w, 512, 12, 6, 1200)
    hit = np.nonzero(rec["collision_penalty"] > 0)[0]
    blocked = np.nonzero(((rec["flags"] & F_INFEASIBLE) != 0) & ((rec["info"] >> 16) > 0))[0]
    rest = np.nonzero(rec["collision_penalty"] == 0)[0]
    assert len(hit) >= 12, len(hit)
    tw.edges = cand[_pick([hit, blocked, rest], 12)]
    return tw


def world_coverage():
    """A small world whose vertex 0 has one short ribbon right ahead — edges along it complete coverage and are cut at
    coverageCompletedTime + timeMinimum (Edge.cpp:169) — and whose vertex 1 is done at the start (no ribbons,
    coverageCompletedTime set: AStarPlanner.cpp:19)."""
    from path_planner_amd import workloads
    from path_planner_amd.types import VERTEX_DTYPE, F_INFEASIBLE, F_DONE, F_THROWS, edge_pack, make_config, H_TSP_POINT_K
    cfg = make_config(start_state_time=3.0, heuristic=H_TSP_POINT_K, tsp_k=2, time_minimum=2.0)
    grid = np.zeros((300, 300), dtype=np.uint8)
    grid[40:60, 100:180] = 1
    grid[200:230, 60:90] = 1
    obst = workloads.obstacles(4, 9, 150.0, time=3.0, keep_free=(75, 75, 25))
    tw = TraceWorld(cfg, grid, 0.5, obst)
    rib = np.array([[75.0, 80.0, 75.0, 86.0]])
    v = np.zeros(2, dtype=VERTEX_DTYPE)
    v[0] = (75.0, 75.0, 0.0, 2.5, 3.0, 0.0, -1.0, 0, 1)
    v[1] = (80.0, 70.0, 0.4, 2.5, 4.0, 1.0, 3.5, 1, 0)
    tw.verts, tw.pool = v, rib
    rng = np.random.default_rng(11)
    n = 200
    tw.sx, tw.sy, tw.sh = rng.uniform(20, 130, n), rng.uniform(20, 130, n), rng.uniform(0, 2 * np.pi, n)
    tw.sx[:8], tw.sy[:8], tw.sh[:8] = 75.0, np.linspace(100.0, 135.0, 8), 0.0      # straight north over the ribbon, far beyond it
    cand = edge_pack(np.repeat(np.arange(2), 4 * n), np.tile(np.repeat(np.arange(n), 4), 2), np.tile(np.arange(4), 2 * n))
    rec = tw.world.cost_edges(tw.verts, tw.pool, tw.sx, tw.sy, tw.sh, cand, threads=8)
    ok = ((rec["flags"] & (F_INFEASIBLE | F_THROWS)) == 0)
    vi = (cand >> np.uint64(32)) & np.uint64(0xFFFFFF)
    curve_end = tw.verts["time"][vi.astype(np.int64)] + rec["approx_cost"]
    # cut by coverage completion: feasible, done, and ended before both the curve's own end and the horizon
    cut = np.nonzero(ok & (vi == 0) & ((rec["flags"] & F_DONE) != 0) & (rec["end_time"] < curve_end - 0.1) &
                     (rec["end_time"] < cfg.start_state_time + cfg.time_horizon - 0.1))[0]
    done = np.nonzero(ok & (vi == 1))[0]
    other = np.nonzero(ok & (vi == 0) & ((rec["flags"] & F_DONE) == 0))[0]
    assert len(cut) >= 4 and len(done) >= 12, (len(cut), len(done))
    tw.cut_edges = cand[cut[:8]]
    tw.edges = np.concatenate([cand[cut[:8]], cand[_pick([done, other], 14)]])
    return tw


WORLDS = {"binary": world_binary, "gaussian_default": lambda: world_gaussian("default"), "gaussian_custom": lambda: world_gaussian("custom"),
          "coverage": world_coverage}


def _angdiff(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b)) % TWO_PI
    return np.minimum(d, TWO_PI - d)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)


def reference_times(cfg, t0, n):
    """Edge.cpp:114-120,173 in Python floats (IEEE doubles, one rounding per operation, as the reference compiles)."""
    dt = cfg.collision_checking_increment / cfg.max_speed
    t = t0 + math.fmod(t0 - cfg.start_state_time, dt)
    out = np.empty(n)
    for k in range(n):
        out[k] = t
        t += dt
    return out


def _edge_curve(tw, desc, rec):
    """(path8, start time, speed, vertex index) of the list-form edge `desc` with record `rec` (DubinsWrapper::set, Edge.cpp:73-80)."""
    import oracle as orc
    vi = int((int(desc) >> 32) & 0xFFFFFF)
    cb = int(int(desc) >> 56)
    cfg = tw.cfg
    rho = cfg.coverage_turning_radius if cb & 1 else cfg.turning_radius
    slow = cfg.slow_speed if cfg.slow_speed > 0 else cfg.max_speed
    speed = slow if cb & 2 else cfg.max_speed
    v = tw.verts[vi]
    p8 = np.array([v["x"], v["y"], orc.yaw(float(v["heading"])), rec["param"][0], rec["param"][1], rec["param"][2], rho, float(rec["info"] & 0xFF)])
    return p8, float(v["time"]), speed, vi


def oracle_pose(p8, start, speed, t):
    """DubinsWrapper::sample (DubinsWrapper.cpp:29-49) on the oracle's dubins_path_sample."""
    import oracle as orc
    length = float(p8[3] + p8[4] + p8[5]) * float(p8[6])
    dist = (t - start) * speed
    if dist < 0 or dist > length:
        dist -= 1e-5
    err, q = orc.dubins_sample(p8, dist)
    assert err == 0, (err, dist, length)
    h = math.pi / 2 - q[2]
    if h < 0:
        h += TWO_PI
    return q[0], q[1], h


def check_trace(tw, descs, res, counts, steps, curves=None, check_poses=True, stats=None):
    """Checks 1 (counts), 2 (times), 3 (poses), 4 (blocked), 5 / 6 (collision), 7 (running penalty), 8 (straight flag)
    for the edges `descs` with records `res`, step counts `counts` and step records `steps[i, :counts[i]]` (untruncated).
    curves[i] = (path8, start, speed, vertex) where the edges are not list-form descriptors."""
    from path_planner_amd.types import F_INFEASIBLE, F_THROWS, F_DUBINS_ERR, S_BLOCKED, S_STRAIGHT
    from parity import REL_TOL
    cfg = tw.cfg
    cpf = cfg.collision_penalty_factor
    stats = stats if stats is not None else {}
    for key in ("steps", "flip_steps", "worst_xy", "worst_heading", "worst_collision", "n_blocked", "n_collision_steps", "n_straight"):
        stats.setdefault(key, 0)
    times_of = {}
    for i in range(len(res)):
        r = res[i]
        n = int(counts[i])
        throws = (r["flags"] & F_THROWS) != 0
        assert n == (0 if throws else int(r["info"] >> 16)), (i, n, r["info"] >> 16)                      # 1
        assert n <= steps.shape[1]
        if n == 0:
            continue
        s = steps[i, :n]
        p8, start, speed, vi = curves[i] if curves is not None else _edge_curve(tw, descs[i], r)
        v = tw.verts[vi]
        assert np.array_equal(s["step"], np.arange(n)) and np.all(s["reserved"] == 0)
        # 2: bit-equal times
        if vi not in times_of or len(times_of[vi]) < n:
            times_of[vi] = reference_times(cfg, float(v["time"]), max(n, 1501))
        assert np.array_equal(s["time"], times_of[vi][:n]), (i, "times")
        # 3: poses against the oracle's sample of the record's curve
        if check_poses:
            for k in range(n):
                ox, oy, oh = oracle_pose(p8, start, speed, float(s["time"][k]))
                dxy = max(_rel(s["x"][k], ox), _rel(s["y"][k], oy))
                dh = float(_angdiff(s["heading"][k], oh))
                stats["worst_xy"] = max(stats["worst_xy"], float(dxy))
                stats["worst_heading"] = max(stats["worst_heading"], dh)
                assert dxy <= REL_TOL and dh <= REL_TOL, (i, k, s[k], ox, oy, oh)
        # 4: blocked = the oracle's isBlocked at the device's pose; only ever on the last record; there iff the edge is infeasible
        blk = (s["flags"] & S_BLOCKED) != 0
        assert np.array_equal(blk, tw.world.is_blocked(s["x"], s["y"]) != 0), (i, "blocked")
        assert not blk[:-1].any()
        if not (r["flags"] & F_DUBINS_ERR):
            assert bool(blk[-1]) == bool(r["flags"] & F_INFEASIBLE), (i, "blocked vs infeasible", r["flags"])
        stats["n_blocked"] += int(blk[-1])
        # 5 / 6: collisionExists at the device's pose and time; 0 on a blocked step
        want = np.array([tw.world.collision_exists(float(s["x"][k]), float(s["y"][k]), float(s["time"][k]), True) for k in range(n)])
        want[blk] = 0.0
        if tw.binary:
            for k in np.nonzero(s["collision"] != want)[0]:
                x, y, t = float(s["x"][k]), float(s["y"][k]), float(s["time"][k])
                near = [tw.world.collision_exists(x + dx, y + dy, t, True) for dx, dy in ((FLIP_EPS, 0), (-FLIP_EPS, 0), (0, FLIP_EPS), (0, -FLIP_EPS))]
                assert any(c != want[k] for c in near), (i, k, s[k], want[k], near)
                stats["flip_steps"] += 1
        else:
            rel = _rel(s["collision"], want)
            stats["worst_collision"] = max(stats["worst_collision"], float(rel.max()))
            assert rel.max() <= REL_TOL, (i, "gaussian collision", rel.max())
        stats["n_collision_steps"] += int(np.count_nonzero(s["collision"]))
        # 7: the running penalty
        assert s["penalty_before"][0] == 0.0
        seq = np.zeros(n)
        acc = 0.0
        for k in range(n):
            seq[k] = acc
            acc += s["collision"][k] * cpf
        if tw.binary:
            assert np.array_equal(s["penalty_before"], seq), (i, "penalty")
            assert s["penalty_before"][-1] + s["collision"][-1] * cpf == r["collision_penalty"], (i, acc, r["collision_penalty"])
        else:
            assert _rel(s["penalty_before"], seq).max() <= REL_TOL
            assert _rel(s["penalty_before"][-1] + s["collision"][-1] * cpf, r["collision_penalty"]) <= REL_TOL
        # 8: the straight flag from the device's own headings
        prev = np.concatenate([[float(v["heading"])], s["heading"][:-1]])
        assert np.array_equal((s["flags"] & S_STRAIGHT) != 0, s["heading"] == prev), (i, "straight")
        assert np.all((s["flags"] & ~np.uint32(S_BLOCKED | S_STRAIGHT)) == 0)
        stats["n_straight"] += int(np.count_nonzero(s["flags"] & S_STRAIGHT))
        stats["steps"] += n
    assert stats["flip_steps"] <= FLIP_CAP * max(stats["steps"], 1), stats
    return stats


STRIDE = 1504     # more than any edge has: a 30 s horizon at 0.02 s per step is 1 501 steps


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_steps_match_the_oracle(torch_cuda, name):
    """Checks 1-8 on a few dozen edges per world, and the records against ppgpu_cost_edges_host byte for byte."""
    from path_planner_amd.types import STEP_DTYPE
    tw = WORLDS[name]()
    ctx = tw.context()
    want = ctx.cost_edges_host(tw.edges)
    sentinel = np.frombuffer(np.full(STEP_DTYPE.itemsize, 0xA5, dtype=np.uint8).tobytes(), dtype=STEP_DTYPE)[0]
    steps = np.full((len(tw.edges), STRIDE), sentinel, dtype=STEP_DTYPE)
    res, counts, steps = ctx.trace_edges(tw.edges, STRIDE, steps)
    assert res.tobytes() == want.tobytes()
    assert np.array_equal(counts, (res["info"] >> 16).astype(np.int32) * ((res["flags"] & 2) == 0))
    stats = check_trace(tw, tw.edges, res, counts, steps)
    print(name, "edges", len(tw.edges), stats)
    for i in range(len(tw.edges)):                                     # nothing written beyond an edge's count
        assert steps[i, counts[i]:].tobytes() == np.full(STRIDE - counts[i], sentinel, dtype=STEP_DTYPE).tobytes()
    assert stats["steps"] > 5000 and stats["n_straight"] > 0
    if name != "coverage":
        assert stats["n_collision_steps"] > 100
    if name == "binary":
        assert stats["n_blocked"] >= 8
    if name == "coverage":
        # the edges cut by coverage completion stop where the record says, well short of their curve and of the horizon
        ncut = len(tw.cut_edges)
        for i in range(ncut):
            end = steps[i, counts[i] - 1]["time"]
            assert end < res["end_time"][i] <= end + 2 * tw.cfg.collision_checking_increment / tw.cfg.max_speed
            assert res["end_time"][i] == res["coverage_completed_time"][i] + tw.cfg.time_minimum
        # the done-at-start vertex: its edges cost their collision penalty only, their steps are all there
        done = ((tw.edges >> np.uint64(32)) & np.uint64(0xFFFFFF)) == 1
        assert done.sum() >= 10 and np.all(counts[done] > 0)
        assert np.all(res["true_cost"][done] == res["collision_penalty"][done])


def test_stride_cuts_records_not_counts(torch_cuda):
    """Check 9: a step_stride below some counts — counts come back whole, records [0, stride) are those of the untruncated run,
    nothing beyond an edge's slot is written."""
    from path_planner_amd.types import STEP_DTYPE
    tw = world_binary()
    ctx = tw.context()
    res, counts, steps = ctx.trace_edges(tw.edges, STRIDE)
    small = 100
    assert np.count_nonzero(counts > small) >= 10 and np.count_nonzero((counts > 0) & (counts < small)) >= 1
    sentinel = np.frombuffer(np.full(STEP_DTYPE.itemsize, 0x5A, dtype=np.uint8).tobytes(), dtype=STEP_DTYPE)[0]
    cut = np.full((len(tw.edges), small), sentinel, dtype=STEP_DTYPE)
    res2, counts2, cut = ctx.trace_edges(tw.edges, small, cut)
    assert res2.tobytes() == res.tobytes() and np.array_equal(counts2, counts)
    for i in range(len(tw.edges)):
        m = min(int(counts[i]), small)
        assert cut[i, :m].tobytes() == steps[i, :m].tobytes()
        assert cut[i, m:].tobytes() == np.full(small - m, sentinel, dtype=STEP_DTYPE).tobytes()


def test_wrapper_form_gives_the_list_form_steps(torch_cuda):
    """Check 10: the same edges handed over as curves (Vertex::connect(start, DubinsWrapper, coverageAllowed)) — qi from the
    vertex, param / type from the list form's records — give the same step records; one that starts after its vertex's first
    step has none (Edge.cpp:126-133)."""
    import oracle as orc
    from path_planner_amd.types import WRAPPER_EDGE_DTYPE, F_INFEASIBLE, F_THROWS
    tw = world_binary()
    ctx = tw.context()
    res, counts, steps = ctx.trace_edges(tw.edges, STRIDE)
    keep = np.nonzero((res["flags"] & F_THROWS) == 0)[0]
    we = np.zeros(len(keep) + 1, dtype=WRAPPER_EDGE_DTYPE)
    curves = []
    for j, i in enumerate(keep):
        p8, start, speed, vi = _edge_curve(tw, tw.edges[i], res[i])
        end = orc.O.ppo_wrapper_fill_end_time(p8.ctypes.data, speed, start)
        we[j] = (vi, 1 if p8[6] == tw.cfg.coverage_turning_radius else 0, p8[0:3], p8[3:6], p8[6], int(p8[7]), 0, speed, start, end)
        curves.append((p8, start, speed, vi))
    late = int(np.argmax(counts[keep]))
    we[-1] = we[late]
    # (the vertex's first step comes less than one interval after its own time, Edge.cpp:116-120: this start lies after it)
    we[-1]["start_time"] += 1.5 * tw.cfg.collision_checking_increment / tw.cfg.max_speed
    wres, wcounts, wsteps = ctx.trace_wrapper_edges(we, STRIDE)
    assert wres.tobytes() == ctx.cost_wrapper_edges_host(we).tobytes()
    assert wcounts[-1] == 0 and (wres["flags"][-1] & F_INFEASIBLE) and (wres["info"][-1] >> 16) == 0
    assert np.array_equal(wcounts[:-1], counts[keep])
    for j, i in enumerate(keep):
        assert wsteps[j, :counts[i]].tobytes() == steps[i, :counts[i]].tobytes(), (j, i)
    # ... and, on wrapper edges of their own kind (entered part-way along, cut short, at a foreign speed), the oracle's steps
    rng = np.random.default_rng(17)
    we2, curves2 = [], []
    for i in range(len(tw.verts)):
        v = tw.verts[i]
        for t in rng.choice(len(tw.sx), size=2, replace=False):
            rho = float(rng.choice([tw.cfg.turning_radius, tw.cfg.coverage_turning_radius]))
            err, p8 = orc.dubins_shortest_path([v["x"], v["y"], orc.yaw(float(v["heading"]))], [tw.sx[t], tw.sy[t], orc.yaw(float(tw.sh[t]))], rho)
            if err != 0 or np.hypot(tw.sx[t] - v["x"], tw.sy[t] - v["y"]) < 1.0:
                continue
            speed = float(rng.choice([tw.cfg.max_speed, 1.7, tw.cfg.slow_speed]))
            dur = float(p8[3] + p8[4] + p8[5]) * rho / speed
            start = max(0.0, float(v["time"]) - float(rng.choice([0.0, 0.25])) * dur)
            end = orc.O.ppo_wrapper_fill_end_time(p8.ctypes.data, speed, start)
            if rng.random() < 0.4:
                end = min(end, start + float(rng.uniform(0.5, 1.0)) * (end - start))
            if not end > float(v["time"]) + 0.1:
                continue
            we2.append((i, 1 if rho == tw.cfg.coverage_turning_radius else 0, p8[0:3], p8[3:6], rho, int(p8[7]), 0, speed, start, end))
            curves2.append((p8.copy(), start, speed, i))
    we2 = np.array(we2, dtype=WRAPPER_EDGE_DTYPE)
    r2, c2, s2 = ctx.trace_wrapper_edges(we2, STRIDE)
    ok = np.nonzero((r2["flags"] & F_THROWS) == 0)[0]
    stats = check_trace(tw, None, r2[ok], c2[ok], s2[ok], curves=[curves2[i] for i in ok])
    print("wrapper edges", len(we2), stats)
    assert stats["steps"] > 5000


@pytest.mark.parametrize("budget", [24 << 10, 400 << 10])
def test_sliced_trace_is_bit_identical(torch_cuda, monkeypatch, budget):
    """A handle with a small workspace budget runs the trace as slices.  24 KB: the costing launch is sliced too (6 edges at a
    time) and the trace solves each slice's curves again, one edge's step records per pass; 400 KB: the costing launch fits, its
    setup records are re-used, the step records come home four edges at a time.  The same bytes as in one piece."""
    tw = world_binary()
    whole = tw.context().trace_edges(tw.edges, STRIDE)
    monkeypatch.setenv("PPGPU_SLICE_BYTES", str(budget))
    cut = tw.context().trace_edges(tw.edges, STRIDE)
    for a, b in zip(whole, cut):
        assert a.tobytes() == b.tobytes()


def test_large_launch_through_the_prepass_route(torch_cuda, monkeypatch):
    """One launch of more than 8 192 edges with the production setting, so that the records the trace starts from came through
    the chunk-skip planner and the approach prepass; list form, device arrays.  Records byte-identical to the costing entry
    point; times, blocked flags, penalties and straight flags on every step; poses and collisions on a strided subset; and the
    subset's steps equal to those a small launch of the same edges gives."""
    from path_planner_amd.types import RESULT_DTYPE, STEP_DTYPE, F_THROWS, F_INFEASIBLE, S_BLOCKED, S_STRAIGHT, edge_pack
    torch = torch_cuda
    monkeypatch.delenv("PPGPU_PREPASS_MIN_EDGES", raising=False)
    tw = world_binary()
    rng = np.random.default_rng(9)
    ne = 9000
    vi, ti, cb = rng.integers(0, len(tw.verts), ne), rng.integers(0, len(tw.sx), ne), rng.integers(0, 4, ne)
    far = np.hypot(tw.verts["x"][vi] - tw.sx[ti], tw.verts["y"][vi] - tw.sy[ti]) > 2 * tw.cfg.collision_checking_increment
    edges = edge_pack(vi[far], ti[far], cb[far])
    ne = len(edges)
    assert ne >= 8192
    ctx = tw.context()
    d_e = torch.from_numpy(edges.view(np.int64)).to("cuda:0")
    d_res = torch.zeros(ne * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_counts = torch.full((ne,), -1, dtype=torch.int32, device="cuda:0")
    d_steps = torch.full((ne * STRIDE * STEP_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()      # the fills ran on torch's stream, the library works on its own
    ctx.trace_edges_list(ne, d_e.data_ptr(), d_res.data_ptr(), STRIDE, d_counts.data_ptr(), d_steps.data_ptr())
    ctx.synchronize()
    res = d_res.cpu().numpy().view(RESULT_DTYPE)
    counts = d_counts.cpu().numpy()
    steps = d_steps.cpu().numpy().view(STEP_DTYPE).reshape(ne, STRIDE)
    del d_steps
    assert res.tobytes() == ctx.cost_edges_host(edges).tobytes()
    assert np.array_equal(counts, np.where((res["flags"] & F_THROWS) != 0, 0, res["info"] >> 16).astype(np.int32))
    # every step: time, blocked, penalty, straight flag, nothing beyond the count
    valid = np.arange(STRIDE)[None, :] < counts[:, None]
    assert np.all(steps.view(np.uint8).reshape(ne, STRIDE, 64)[~valid] == 0xA5)
    evi = ((edges >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64)
    for v in range(len(tw.verts)):
        rows = np.nonzero(evi == v)[0]
        t = reference_times(tw.cfg, float(tw.verts["time"][v]), STRIDE)
        assert np.all((steps["time"][rows] == t[None, :]) | ~valid[rows]), v
    blk = (steps["flags"] & S_BLOCKED) != 0
    ob = tw.world.is_blocked(steps["x"][valid], steps["y"][valid]) != 0
    assert np.array_equal(blk[valid], ob)
    last = np.maximum(counts - 1, 0)
    has = counts > 0
    idx = np.arange(ne)
    assert np.count_nonzero(blk & valid) == np.count_nonzero(blk[idx, last] & has)
    assert np.array_equal(blk[idx, last][has], (res["flags"][has] & F_INFEASIBLE) != 0)
    col = np.where(valid, steps["collision"], 0.0)
    assert np.all(col == np.round(col))
    seq = np.cumsum(col, axis=1) * tw.cfg.collision_penalty_factor       # integers times 600: exact in double
    before = np.concatenate([np.zeros((ne, 1)), seq[:, :-1]], axis=1)
    assert np.all((steps["penalty_before"] == before) | ~valid)
    assert np.array_equal(seq[idx, last][has], res["collision_penalty"][has])
    prev = np.concatenate([tw.verts["heading"][evi][:, None], steps["heading"][:, :-1]], axis=1)
    assert np.all((((steps["flags"] & S_STRAIGHT) != 0) == (steps["heading"] == prev)) | ~valid)
    # poses and collisions on a subset, against the oracle and against a small launch of the same edges
    sub = np.arange(0, ne, ne // 40)
    stats = check_trace(tw, edges[sub], res[sub], counts[sub], steps[sub])
    print("large launch:", ne, "edges,", int(counts.sum()), "steps; subset", stats)
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", "1000000000")
    r3, c3, s3 = tw.context().trace_edges(edges[sub], STRIDE)
    assert np.array_equal(c3, counts[sub])
    for j, i in enumerate(sub):
        assert s3[j, :c3[j]].tobytes() == steps[i, :c3[j]].tobytes()


def test_bad_arguments_are_refused(torch_cuda):
    from path_planner_amd import api
    from path_planner_amd.types import STEP_DTYPE
    tw = world_coverage()
    ctx = tw.context()
    with pytest.raises(api.PpgpuError):
        ctx.trace_edges(tw.edges, 0)
    counts = np.zeros(4, dtype=np.int32)
    steps = np.zeros((4, 8), dtype=STEP_DTYPE)
    rc = api.LIB.ppgpu_trace_edges_host(ctx._h, 4, tw.edges[:4].ctypes.data, None, 8, None, steps.ctypes.data)
    assert rc == -1 and b"trace_edges_host" in api.LIB.ppgpu_last_error()
    rc = api.LIB.ppgpu_trace_edges_host(ctx._h, 4, tw.edges[:4].ctypes.data, None, 8, counts.ctypes.data, steps.ctypes.data)
    assert rc == 0 and counts.max() > 8                                 # h_results may be NULL; counts are whole
    before = ctx.growth_stats()[0]
    ctx.trace_edges(tw.edges, 4 * STRIDE)                               # a larger step buffer than any call before: the handle grows, and says so
    assert ctx.growth_stats()[0] > before
