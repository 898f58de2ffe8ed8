"""-m gpu: shared tracks (pp_k_solve.h, pp_k_arc_stops, pp_k_track_fanout).  All edges of one (vertex, configuration, direction) sample
the same poses while they are on their first arc; where that arc crosses a blocked cell at step kb of the vertex's time row, every edge
of the class that is still on the arc at that step stops there, and one of them per slice is planned and posed for all.  Every test
costs the same edges on a handle with PPGPU_SHARE_TRACKS=0 and on one with the switch on and wants the same bytes in the records and
the child ribbons, the same shared and swept counts, 0 stop members with the switch off, and with it on a count that lies between a
numpy restatement of the rule (pp_edge_stopped_on_arc) on the device's own param[0] and approx_cost with 1e-9 to spare and with 1e-9
of grace: members - 1 of every class and slice.  Every edge the strict restatement admits must have kb + 1 steps and F_INFEASIBLE.
The restatement takes kb from a numpy walk of the class's circle over the grid (_arc_stop); test_rule_boundary holds that walk
against the oracle.  conftest.py forces the prepasses, and so the sharing and the sweep list, onto launches of any size."""
import math

import numpy as np
import pytest

from test_gpu_shared_sweeps import _list, _same_bytes
from test_gpu_solve_heads import _ahead_targets, _arc_target, _root_pose

pytestmark = pytest.mark.gpu

SLOW, COVERAGE = 2, 1
STRIDE = 8
F_INFEASIBLE, F_THROWS = 0x01, 0x02


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---------------------------------------------------------------------------------------- the rule, restated
def _time_row(cfg, t0):
    """A vertex's collision-check times (Edge.cpp:114-120,173: a running sum), as many as ppgpu_set_config gives a row."""
    inc = cfg.collision_checking_increment / cfg.max_speed
    row = np.empty(int(cfg.time_horizon / inc) + 8)
    t = t0 + math.fmod(t0 - cfg.start_state_time, inc)
    for k in range(len(row)):
        row[k] = t
        t += inc
    return row


def _arc_pose(pose, rho, left, d):
    """The point d metres along the left or right circle of radius rho through pose = (x, y, heading)."""
    x0, y0, h0 = pose
    yaw = np.pi / 2 - h0
    phi = np.asarray(d, dtype=np.float64) / rho
    if left:
        return x0 - rho * np.sin(yaw) + rho * np.sin(yaw + phi), y0 + rho * np.cos(yaw) - rho * np.cos(yaw + phi)
    return x0 + rho * np.sin(yaw) - rho * np.sin(yaw - phi), y0 - rho * np.cos(yaw) + rho * np.cos(yaw - phi)


def _class_constants(cfg, c):
    return (cfg.slow_speed if c & SLOW else cfg.max_speed), (cfg.coverage_turning_radius if c & COVERAGE else cfg.turning_radius)


def _arc_stop(cfg, grid, res, vertex, c, left):
    """The first step before the horizon at which the first arc of class (vertex, configuration c, direction) lies on a blocked cell
    or off the grid, -1: none."""
    x0, y0, h0, t0 = vertex
    row = _time_row(cfg, t0)
    speed, rho = _class_constants(cfg, c)
    row = row[row < cfg.time_horizon + 1e-12 + cfg.start_state_time]
    x, y = _arc_pose((x0, y0, h0), rho, left, (row - t0) * speed)
    cx, cy = np.floor(x / res).astype(np.int64), np.floor(y / res).astype(np.int64)
    out = (x < 0) | (y < 0) | (cx >= grid.shape[1]) | (cy >= grid.shape[0])
    blocked = out | (grid[np.clip(cy, 0, grid.shape[0] - 1), np.clip(cx, 0, grid.shape[1] - 1)] != 0)
    hit = np.nonzero(blocked)[0]
    return int(hit[0]) if len(hit) else -1


def _vertex4(verts, i):
    return float(verts["x"][i]), float(verts["y"][i]), float(verts["heading"][i]), float(verts["time"][i])


def _stops(cfg, grid, res, verts):
    """kb of every class: [vertex][configuration * 2 + (0 left, 1 right)]."""
    return np.asarray([[_arc_stop(cfg, grid, res, _vertex4(verts, v), k // 2, k % 2 == 0) for k in range(8)] for v in range(len(verts))])


def _stop_rule(cfg, verts, vi, cfgs, res, stops, margin):
    """pp_edge_stopped_on_arc on the device's own records, every comparison with `margin` to spare: (who passes, class key, kb)."""
    bound = cfg.time_horizon + 1e-12 + cfg.start_state_time
    t0 = np.asarray(verts["time"], dtype=np.float64)[vi]
    speed = np.where((cfgs & SLOW) != 0, cfg.slow_speed, cfg.max_speed)
    rho = np.where((cfgs & COVERAGE) != 0, cfg.coverage_turning_radius, cfg.turning_radius)
    left = np.isin(res["info"] & 0xFF, (0, 1, 5))                  # LSL, LSR, LRL
    cls = cfgs * 2 + np.where(left, 0, 1)
    kb = stops[vi, cls]
    rows = {int(v): _time_row(cfg, float(verts["time"][v])) for v in np.unique(vi)}
    t_kb = np.asarray([rows[int(v)][max(int(k), 0)] for v, k in zip(vi, kb)])
    length, p0 = res["approx_cost"] * speed, res["param"][:, 0]
    solved = (res["flags"] & F_THROWS) == 0
    dist_h = (bound - t0) * speed
    shareable = solved & (t0 + res["approx_cost"] >= bound) & (dist_h <= length) & (dist_h / rho < p0)
    dist = (t_kb - t0) * speed
    # (t_kb < bound without a margin: both are the row's and the configuration's own doubles, the same bits here and on the device —
    # the last step before the horizon lies within 1e-12 of it by construction; the margin is for what the edge's curve contributes)
    ok = solved & ~shareable & (kb >= 0) & (t_kb < bound) & (t_kb < t0 + res["approx_cost"] - margin) & (dist <= length - margin) & (dist / rho < p0 - margin)
    return ok, vi * 8 + cls, kb


def _members(ok, key, slice_of):
    """members - 1 of every (slice, class)."""
    k = key[ok] + (slice_of[ok].astype(np.int64) << 40)
    return int(sum(n - 1 for n in np.unique(k, return_counts=True)[1]))


# ---------------------------------------------------------------------------------------- handles and runs
def _handle(w, tracks, monkeypatch, verts=None, pool=None, gaussian=False, **env):
    from path_planner_amd import api
    for k in ("PPGPU_SLICE_BYTES", "PPGPU_SWEEP_LIST", "PPGPU_SOLVE_ALL_WORDS", "PPGPU_SHARE_SWEEPS", "PPGPU_APPROACH_LIST", "PPGPU_SHARE_TRACKS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not tracks:
        monkeypatch.setenv("PPGPU_SHARE_TRACKS", "0")
    ctx = api.Context(0)                # (the switches are read when the handle is created)
    ctx.set_config(w.cfg)
    ctx.set_grid(w.grid, w.res)
    if gaussian:
        ctx.set_gaussian_obstacles(np.ascontiguousarray(w.obst[:, :5]))
    else:
        ctx.set_obstacles(w.obst)
    ctx.set_vertices(w.root() if verts is None else verts, w.ribbons4 if pool is None else pool)
    return ctx


def _cost(torch, ctx, t, edges, stride=STRIDE):
    """(records, child ribbons), (stop members, shared edges, swept edges) of one launch of `edges` over the targets t."""
    ctx.set_samples(t[:, 0], t[:, 1], t[:, 2])
    out = _list(torch, ctx, edges, stride)
    return out, (ctx.last_stop_members(), ctx.last_shared_edges(), ctx.last_swept_edges())


def _both(torch, w, monkeypatch, t, edges, stride=STRIDE, **kw):
    runs = []
    for tracks in (False, True):
        ctx = _handle(w, tracks, monkeypatch, **kw)
        runs.append(_cost(torch, ctx, t, edges, stride))
        ctx.close()
    return runs


def _check(what, cfg, verts, vi, cfgs, runs, stops, slice_of=None, want_members=True):
    """Off against on: the bytes, the counters, and the members' count and records against the rule.  Returns (strict mask, key, kb)."""
    (off, n_off), (on, n_on) = runs
    assert _same_bytes(on, off), what
    assert n_off[0] == 0 and n_on[1:] == n_off[1:], (what, n_off, n_on)             # shared and swept: what they were
    res = off[0]
    slice_of = np.zeros(len(res), dtype=np.int64) if slice_of is None else slice_of
    ok, key, kb = _stop_rule(cfg, verts, vi, cfgs, res, stops, 1e-9)
    low = _members(ok, key, slice_of)
    high = _members(_stop_rule(cfg, verts, vi, cfgs, res, stops, -1e-9)[0], key, slice_of)
    print(what, "edges", len(res), "members", n_on[0], "rule", low, high, "classes", len(np.unique(key[ok])), "shared", n_on[1], "swept", n_on[2])
    assert low <= n_on[0] <= high, (what, n_on, low, high)
    assert want_members is None or (low > 0) == want_members, (what, low)
    assert np.array_equal(res["info"][ok] >> 16, kb[ok] + 1) and np.all(res["flags"][ok] & F_INFEASIBLE), what
    return ok, key, kb


def _oracle_parity(w, verts, pool, t, edges, got, stride=STRIDE):
    import oracle as orc
    from parity import compare_results
    cpu, cchild = orc.World(w.cfg, w.grid, w.res, w.obst).cost_edges(verts, pool, t[:, 0], t[:, 1], t[:, 2], edges, stride=stride, threads=8)
    rep = compare_results(got[0], cpu, got[1], cchild)
    assert rep["ok"], rep
    return cpu


def _edges_all(nt, configs):
    from path_planner_amd.types import edge_pack
    cfgs = np.tile(np.asarray(configs), nt)
    return edge_pack(np.zeros(len(cfgs), dtype=np.uint64), np.repeat(np.arange(nt), len(configs)), cfgs), cfgs


# ---------------------------------------------------------------------------------------- 1. the rule's boundary, config 3
def test_rule_boundary(torch_cuda, monkeypatch):
    """Config 3's map and root: the common arc of (rho 8, fast, left) is blocked at step 301 = 15.05 m, that of (rho 16, fast, right) at
    step 702 = 35.1 m (the oracle confirms both below, on edges that are still on their first arc there).  Targets whose first arc ends
    one step, two steps and a nanometre before and after those steps."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=64)
    root, verts = _root_pose(w), w.root()
    stops = _stops(w.cfg, w.grid, w.res, verts)
    print("stops of the root's classes", stops[0])
    # (configuration 0, left), (configuration 0, right), (configuration 1, right); the other five classes have none
    assert stops[0, 0] == 301 and stops[0, 1] == 625 and stops[0, 3] == 702 and np.all(stops[0, [2, 4, 5, 6, 7]] == -1)
    step = w.cfg.collision_checking_increment                          # metres per step at full speed
    t = []
    for rho, left, kb in ((w.cfg.turning_radius, True, 301), (w.cfg.coverage_turning_radius, False, 702)):
        t += [_arc_target(root, rho, left, kb * step + d) for d in (-2 * step, -step, -1e-9, 1e-9, step, 2 * step)]
        t += [_arc_target(root, rho, left, kb * step + 3.0 + k) for k in range(3)]       # well past the stop: members whatever the margin
    t = np.asarray(t + list(_ahead_targets(root, 30)))
    edges, cfgs = _edges_all(len(t), (0, 1, 2, 3))
    runs = _both(torch_cuda, w, monkeypatch, t, edges)
    vi = np.zeros(len(cfgs), dtype=np.int64)
    ok, key, kb = _check("rule boundary", w.cfg, verts, vi, cfgs, runs, stops)
    assert {0, 3} <= set(np.unique(key[ok]))
    cpu = _oracle_parity(w, verts, w.ribbons4, t, edges, runs[1][0])
    # the oracle's own step counts on the edges that pass: the stop steps are the reference's, not only the walk's
    assert np.array_equal(cpu["info"][ok] >> 16, kb[ok] + 1) and np.all(cpu["flags"][ok] & F_INFEASIBLE)


# ---------------------------------------------------------------------------------------- hand-made worlds
def _hand_world(horizon=6.0, obst=None):
    """An empty 2 048 x 2 048 grid of 2 cm cells (a step at full speed is 5 cm: every step lies in a cell of its own), the vertex in
    the middle heading north-east, three ribbons, a horizon of 300 steps."""
    from path_planner_amd import workloads
    from path_planner_amd.types import H_TSP_POINT_K, make_config
    cfg = make_config(start_state_time=1.0, time_horizon=horizon, heuristic=H_TSP_POINT_K, tsp_k=2)
    res, n = 0.02, 2048
    c = n * res / 2
    rib = [[c - 6, c + 3 + 2 * i, c + 6, c + 3 + 2 * i] for i in range(3)]
    return workloads.Workload("hand", np.zeros((n, n), dtype=np.uint8), res, obst, rib, [c, c, 0.6, 2.5, 1.0], 64, 7, cfg)


def _block_step(w, vertex, c, left, k):
    """Blocks the cell under step k of the class's arc."""
    speed, rho = _class_constants(w.cfg, c)
    row = _time_row(w.cfg, vertex[3])
    x, y = _arc_pose(vertex[:3], rho, left, (row[k] - vertex[3]) * speed)
    w.grid[int(y / w.res), int(x / w.res)] = 1


def _fan_targets(pose, cfg, arcs):
    """Targets one arc of each length away on the four circles through the pose, one straight ahead (a first arc of length 0), and
    twenty some way ahead."""
    t = [_arc_target(pose, rho, left, a) for rho in (cfg.turning_radius, cfg.coverage_turning_radius) for left in (True, False) for a in arcs]
    yaw = np.pi / 2 - pose[2]
    t.append((pose[0] + 9.0 * np.cos(yaw), pose[1] + 9.0 * np.sin(yaw), pose[2]))
    return np.asarray(t + [tuple(p) for p in _ahead_targets(pose, 20)])


def _last_step(cfg, t0):
    row = _time_row(cfg, t0)
    return int(np.nonzero(row < cfg.time_horizon + 1e-12 + cfg.start_state_time)[0][-1])


@pytest.mark.parametrize("want", [0, 63, 64, 65, "last"])
def test_stops_at_chunk_edges(torch_cuda, monkeypatch, want):
    """2. One blocked cell under step `want` of the left arcs of configurations 0 and 1: the stop on the first step (the vertex stands
    on a blocked cell: every class stops there, and an edge is a member unless its first arc has length 0), on the last step of chunk
    0, the first and second of chunk 1, and the last step before the horizon.  Configuration 0 may not cover while turning (its
    members copy track_eq), configuration 1 may."""
    w = _hand_world()
    verts = w.root()
    vertex = _vertex4(verts, 0)
    k = _last_step(w.cfg, vertex[3]) if want == "last" else want
    for c in (0, 1):
        _block_step(w, vertex, c, True, k)
    stops = _stops(w.cfg, w.grid, w.res, verts)
    print("stops", stops[0])
    assert stops[0, 0] == k and stops[0, 2] == k
    arcs = [0.5, 2.0, 3.1, 3.15, 3.2, 3.25, 3.3, 5.0, 10.0, 14.9, 15.1, 17.0]
    if want == "last":
        # An edge still on its first arc at the horizon is shared by the horizon rule already, so a member here has its first arc end
        # between the last step (15 m) and the horizon, 2.5e-12 m later: three targets inside that window.  The strict restatement
        # (1e-9 to spare) cannot admit them, the one with grace does, and the device may land anywhere in between: the bytes decide.
        arcs += [15.0 + d for d in (0.8e-12, 1.2e-12, 1.6e-12)]
    t = _fan_targets(vertex[:3], w.cfg, arcs)
    edges, cfgs = _edges_all(len(t), (0, 1))
    runs = _both(torch_cuda, w, monkeypatch, t, edges)
    vi = np.zeros(len(cfgs), dtype=np.int64)
    ok, key, _ = _check("stop at step %d" % k, w.cfg, verts, vi, cfgs, runs, stops, want_members=None if want == "last" else True)
    if want == "last":
        grace, gkey, _ = _stop_rule(w.cfg, verts, vi, cfgs, runs[0][0][0], stops, -1e-9)
        assert {0, 2} <= set(np.unique(gkey[grace])) and _members(grace, gkey, vi) >= 2
    else:
        assert {0, 2} <= set(np.unique(key[ok]))
    _oracle_parity(w, verts, w.ribbons4, t, edges, runs[1][0])
    if k == 0:
        res = runs[0][0][0]
        flat = ((res["flags"] & F_THROWS) == 0) & (res["param"][:, 0] == 0.0)
        assert np.any(flat) and not np.any(ok & flat)


def test_hits_before_the_stop(torch_cuda, monkeypatch):
    """3. A box at rest across the common arcs of configurations 0 and 1 around step 60, the blocked cell at step 150: the members
    copy chunk sums that are not zero and the per-step rows of those chunks (the stop lies in a chunk with hits before it)."""
    vertex = _vertex4(_hand_world().root(), 0)
    bx, by = _arc_pose(vertex[:3], 8.0, True, 60 * 0.05)
    obst = np.asarray([[bx, by, 0.3, 0.0, 1.0, 3.0, 5.0], [bx + 60.0, by, 0.0, 0.0, 1.0, 3.0, 5.0]])
    w = _hand_world(obst=obst)
    verts = w.root()
    for c in (0, 1):
        _block_step(w, vertex, c, True, 150)
    stops = _stops(w.cfg, w.grid, w.res, verts)
    assert stops[0, 0] == 150 and stops[0, 2] == 150
    t = _fan_targets(vertex[:3], w.cfg, [2.0, 7.4, 7.6, 8.0, 9.0, 10.0, 12.0, 15.0])
    edges, cfgs = _edges_all(len(t), (0, 1, 2, 3))
    runs = _both(torch_cuda, w, monkeypatch, t, edges)
    ok, key, _ = _check("hits before the stop", w.cfg, verts, np.zeros(len(cfgs), dtype=np.int64), cfgs, runs, stops)
    res = runs[1][0][0]
    print("penalties of the members", np.unique(res["collision_penalty"][ok]))
    assert np.all(res["collision_penalty"][ok & (key == 0)] > 0)
    _oracle_parity(w, verts, w.ribbons4, t, edges, runs[1][0])


def test_short_curves_and_a_clear_circle(torch_cuda, monkeypatch):
    """4. The left arc of configuration 0 is blocked at step 200 (10 m), but every curve that begins with it ends before that step
    (wEnd <= t_kb); the right circle is clear, and the curves that begin with it are long.  No members."""
    w = _hand_world()
    verts = w.root()
    vertex = _vertex4(verts, 0)
    _block_step(w, vertex, 0, True, 200)
    stops = _stops(w.cfg, w.grid, w.res, verts)
    assert stops[0, 0] == 200 and stops[0, 1] == -1
    rho = w.cfg.turning_radius
    t = np.asarray([_arc_target(vertex[:3], rho, True, a) for a in (1.0, 2.0, 3.0, 4.0, 5.0)] + [_arc_target(vertex[:3], rho, False, a) for a in (11.0, 12.0, 13.0, 14.0)])
    edges, cfgs = _edges_all(len(t), (0,))
    runs = _both(torch_cuda, w, monkeypatch, t, edges)
    _check("short curves, clear circle", w.cfg, verts, np.zeros(len(cfgs), dtype=np.int64), cfgs, runs, stops, want_members=False)
    assert runs[1][1][0] == 0
    res = runs[0][0][0]
    left = np.isin(res["info"] & 0xFF, (0, 1, 5))
    row = _time_row(w.cfg, vertex[3])
    assert np.count_nonzero(left & (vertex[3] + res["approx_cost"] <= row[200])) >= 5          # they end before the stop
    assert np.count_nonzero(~left & (res["param"][:, 0] * rho > 10.5)) >= 4                       # long first arcs on the clear circle


# ---------------------------------------------------------------------------------------- 5, 6: config 3's own edges
def test_shuffled_open_vertices(torch_cuda, monkeypatch):
    """5. 64 open vertices x 16 samples x 4 configurations as an explicit list in a shuffled order: one wave holds several vertices
    and classes of both kinds."""
    from path_planner_amd import workloads
    from path_planner_amd.types import edge_pack
    from test_gpu_solve_heads import _open_vertices
    w = workloads.config3(n_samples=1024)
    ns, stride = 16, 12
    runs, keep = [], None
    for tracks in (False, True):
        ctx = _handle(w, tracks, monkeypatch)
        ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
        n = ctx.sampler_add(1024)
        v, pool = _open_vertices(w, ctx, n, stride)
        assert len(v) == 64
        t = ctx.get_samples()[:ns, :3]
        # two targets one long arc away from the last vertex and from the root, on each of the fast circles
        far = [_arc_target((float(v["x"][i]), float(v["y"][i]), float(v["heading"][i])), rho, lr, 20.0 + d)
               for i in (0, 63) for rho in (w.cfg.turning_radius, w.cfg.coverage_turning_radius) for lr in (True, False) for d in (0.0, 1.0)]
        t = np.concatenate([t, np.asarray(far)])
        ctx.set_vertices(v, pool)
        vi, ti, cb = np.meshgrid(np.arange(64), np.arange(len(t)), np.arange(4), indexing="ij")
        order = np.random.default_rng(11).permutation(vi.size)
        vi, cfgs = vi.ravel()[order], cb.ravel()[order]
        edges = edge_pack(vi, ti.ravel()[order], cfgs)
        runs.append(_cost(torch_cuda, ctx, t, edges, stride))
        keep = v, vi, cfgs
        ctx.close()
    v, vi, cfgs = keep
    stops = _stops(w.cfg, w.grid, w.res, v)
    ok, key, _ = _check("64 open vertices, shuffled", w.cfg, v, vi, cfgs, runs, stops)
    assert len(np.unique(key[ok] // 8)) >= 8                     # stop classes of many vertices


def test_three_slices_heads_per_slice(torch_cuda, monkeypatch):
    """6. The sampler's 75 attempts from config 3's root and a few long first arcs, x 4 configurations, cut into three slices: a track lives
    in the slice's workspace, so every slice elects its own heads, and the members' count is members - 1 per class AND slice."""
    from path_planner_amd import workloads
    from test_gpu_sweep_list import _steps_per_row
    w = workloads.config3(n_samples=75)
    root, verts = _root_pose(w), w.root()
    nch = _steps_per_row(w.cfg)[1]
    per_edge = 256 + nch * 64 * 2 + nch * 12 + 16          # workspace bytes of an edge (cost_modes): setup record, track rows, summary
    runs, slices = [], None
    for tracks in (False, True):
        ctx = _handle(w, tracks, monkeypatch)
        ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
        ctx.sampler_add(75)
        t = ctx.get_samples()[:, :3]
        ctx.close()
        far = [_arc_target(root, rho, lr, a) for rho, lr, a in ((8.0, True, 17.0), (16.0, False, 37.0), (8.0, True, 18.0), (16.0, False, 38.0))]
        t = np.concatenate([np.asarray(far[:2]), t, np.asarray(far[2:])])
        edges, cfgs = _edges_all(len(t), (0, 1, 2, 3))
        per = -(-len(edges) // 3)
        ctx = _handle(w, tracks, monkeypatch, PPGPU_SLICE_BYTES=str(per_edge * per + 64))      # (both handles: the same launch shape)
        runs.append(_cost(torch_cuda, ctx, t, edges))
        slices = ctx.last_slices()
        ctx.close()
        print("slices", slices)
        assert slices[0] == 3 and slices[1] == len(edges) - 2 * per, slices
    stops = _stops(w.cfg, w.grid, w.res, verts)
    slice_of = np.arange(len(edges)) // per
    ok, key, _ = _check("three slices", w.cfg, verts, np.zeros(len(cfgs), dtype=np.int64), cfgs, runs, stops, slice_of=slice_of)
    assert max(len(np.unique(slice_of[ok & (key == k)])) for k in np.unique(key[ok])) >= 2       # a class with a head in more than one slice


# ---------------------------------------------------------------------------------------- 7. staleness
def test_table_follows_grid_vertices_and_keepout(torch_cuda, monkeypatch):
    """7. One handle through: a launch; ppgpu_set_grid with the blocked cell moved; ppgpu_set_vertices with the vertex turned; a
    keep-out limit that grows the cell.  After each change the launch must agree with a fresh handle (switch on, and off) on the
    bytes and on the members' count: a table that outlived its inputs would name a stop step that is no longer one."""
    from path_planner_amd.types import VERTEX_DTYPE
    w = _hand_world()
    verts = w.root()
    vertex = _vertex4(verts, 0)
    for c in (0, 1):
        _block_step(w, vertex, c, True, 100)
    grid1 = w.grid.copy()
    grid2 = np.zeros_like(grid1)
    w.grid = grid2
    for c in (0, 1):
        _block_step(w, vertex, c, True, 180)
    turned = np.array(verts, dtype=VERTEX_DTYPE)
    turned["heading"] = verts["heading"] + 0.002           # 1.8 cm sideways at the stop of configuration 0: another cell, or none
    lim2 = 30                                              # cells within sqrt(30) cells of a blocked one: the arcs stop some steps earlier
    t = _fan_targets(vertex[:3], w.cfg, [2.0, 4.0, 5.5, 8.0, 9.5, 12.0, 15.1])
    edges, cfgs = _edges_all(len(t), (0, 1, 2, 3))
    stages = [("first grid", grid1, verts, 0), ("grid moved", grid2, verts, 0), ("vertex turned", grid2, turned, 0), ("keep-out", grid2, turned, lim2)]

    def fresh(tracks, grid, v, lim):
        w.grid = grid
        ctx = _handle(w, tracks, monkeypatch, verts=v)
        if lim:
            ctx.set_keepout_limit2(lim)
        out = _cost(torch_cuda, ctx, t, edges)
        ctx.close()
        return out

    w.grid = grid1
    one = _handle(w, True, monkeypatch)
    counts = []
    for what, grid, v, lim in stages:
        if what == "grid moved":
            one.set_grid(grid, w.res)
        elif what == "vertex turned":
            one.set_vertices(v, w.ribbons4)
        elif what == "keep-out":
            one.set_keepout_limit2(lim)
        got = _cost(torch_cuda, one, t, edges)
        off, on = fresh(False, grid, v, lim), fresh(True, grid, v, lim)
        print(what, "members", got[1][0], "fresh handle", on[1][0])
        assert _same_bytes(got[0], off[0]) and _same_bytes(on[0], off[0]), what
        assert got[1] == on[1] and off[1][0] == 0 and off[1][1:] == on[1][1:], (what, got[1], on[1], off[1])
        if lim == 0:
            w.grid = grid
            _check(what, w.cfg, v, np.zeros(len(cfgs), dtype=np.int64), cfgs, (off, got), _stops(w.cfg, grid, w.res, v), want_members=None)
        counts.append(got[1][0])
    one.close()
    assert counts[0] > 0 and counts[1] > 0 and counts[3] > 0 and len(set(counts[:2])) == 2, counts


# ---------------------------------------------------------------------------------------- 8, 9
def test_switch_off_is_the_parent(torch_cuda, monkeypatch):
    """8. Config 3, 512 attempts, dense 0xF as a list: no members with the switch off, shared and swept edges unchanged, the same
    bytes; with the switch on a tenth of the swept edges are members (the root's three blocked arcs)."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=512)
    ctx = _handle(w, False, monkeypatch)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    ctx.sampler_add(512)
    t = ctx.get_samples()[:, :3]
    ctx.close()
    edges, cfgs = _edges_all(len(t), (0, 1, 2, 3))
    runs = _both(torch_cuda, w, monkeypatch, t, edges)
    verts = w.root()
    _check("switch off", w.cfg, verts, np.zeros(len(cfgs), dtype=np.int64), cfgs, runs, _stops(w.cfg, w.grid, w.res, verts))
    (_, n_off), (_, n_on) = runs
    assert n_off[0] == 0 and n_on[0] >= 0.05 * n_on[2], (n_off, n_on)


def test_gaussian_model_forms_no_stop_classes(torch_cuda, monkeypatch):
    """9. The Gaussian obstacle model: no members, and the same bytes either way."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=256)
    ctx = _handle(w, False, monkeypatch, gaussian=True)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    ctx.sampler_add(256)
    t = ctx.get_samples()[:, :3]
    ctx.close()
    edges, _ = _edges_all(len(t), (0, 1, 2, 3))
    (off, n_off), (on, n_on) = _both(torch_cuda, w, monkeypatch, t, edges, gaussian=True)
    assert _same_bytes(on, off) and n_off == n_on and n_on[0] == 0, (n_off, n_on)
