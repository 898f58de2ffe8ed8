"""-m gpu: how pp_k_solve_edges elects the head of a class of shared sweeps (pp_k_solve.h): the wave's lowest position per class, the
workgroup's in LDS, one atomicMin per workgroup and class on a table with a 128-byte line per class (pp_share_entry), which the last
kernel of a launch leaves all-ones for the next.  The head stays the member with the lowest position in the caller's list, so every
case wants (a) the bytes of the records and the child ribbons of a handle with PPGPU_SHARE_SWEEPS=0 and (b) ppgpu_last_shared_edges
equal to the rule (pp_edge_shareable) applied in Python to that handle's records: members - 1 of every class.  The rule is taken with
1e-9 to spare and with 1e-9 of grace, as test_gpu_shared_sweeps.py's _rule_members does for one vertex; the two counts must agree (no
edge of these lists sits on the rule's boundary) and be the device's.  conftest.py forces the prepasses, and so the sharing, onto
launches of any size.  Each case also asserts, on the rule's own membership, that its list holds the layout it is there for."""
import numpy as np
import pytest

from test_gpu_shared_sweeps import _dense, _list, _same_bytes

pytestmark = pytest.mark.gpu

SLOW, COVERAGE = 2, 1
STRIDE = 8


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _handle(w, share, monkeypatch, verts=None, pool=None, **env):
    from path_planner_amd import api
    for k in ("PPGPU_SLICE_BYTES", "PPGPU_SWEEP_LIST", "PPGPU_SOLVE_ALL_WORDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if share:
        monkeypatch.delenv("PPGPU_SHARE_SWEEPS", raising=False)
    else:
        monkeypatch.setenv("PPGPU_SHARE_SWEEPS", "0")
    ctx = api.Context(0)                # (the switches are read when the handle is created)
    ctx.set_config(w.cfg)
    ctx.set_grid(w.grid, w.res)
    ctx.set_obstacles(w.obst)
    ctx.set_vertices(w.root() if verts is None else verts, w.ribbons4 if pool is None else pool)
    return ctx


def _classes(w, verts, vi, cfgs, res, margin):
    """pp_edge_shareable on the records of edges (vertex vi, configuration cfgs): who is a member, with `margin` to spare in every
    comparison, and the class key (vertex * 8 + configuration * 2 + direction of the first arc) of each edge."""
    bound = w.cfg.time_horizon + 1e-12 + w.cfg.start_state_time
    t0 = np.asarray(verts["time"], dtype=np.float64)[vi]
    speed = np.where((cfgs & SLOW) != 0, w.cfg.slow_speed, w.cfg.max_speed)
    rho = np.where((cfgs & COVERAGE) != 0, w.cfg.coverage_turning_radius, w.cfg.turning_radius)
    length = res["approx_cost"] * speed
    dist = (bound - t0) * speed
    solved = (res["flags"] & 0x02) == 0
    ok = solved & (t0 + res["approx_cost"] >= bound + margin) & (dist <= length - margin) & (dist / rho < res["param"][:, 0] - margin)
    left = np.isin(res["info"] & 0xFF, (0, 1, 5))                  # LSL, LSR, LRL
    return ok, vi * 8 + cfgs * 2 + np.where(left, 0, 1)


def _rule(w, verts, vi, cfgs, res):
    """(edges the rule shares, member mask, class keys); the count must not depend on the margin."""
    counts = []
    for margin in (1e-9, -1e-9):
        ok, key = _classes(w, verts, vi, cfgs, res, margin)
        counts.append(int(sum(max(0, n - 1) for n in np.bincount(key[ok]))))
    assert counts[0] == counts[1], ("an edge of the list sits on the rule's boundary", counts)
    ok, key = _classes(w, verts, vi, cfgs, res, 0.0)
    return counts[0], ok, key


def _arc_target(pose, rho, left, arc):
    """Where a vehicle at pose = (x, y, heading) is after an arc of `arc` metres at radius rho, 2 m straight on and 0.3 rad more of
    the same turn: a target whose curve at that radius begins with that arc (LSL or RSR, well away from the degenerate one-arc case)."""
    x, y, h0 = pose
    yaw = np.pi / 2 - h0
    sgn = 1.0 if left else -1.0
    for phi, straight in ((arc / rho, 2.0), (0.3, 0.0)):
        cx, cy = x - sgn * rho * np.sin(yaw), y + sgn * rho * np.cos(yaw)
        yaw += sgn * phi
        x, y = cx + sgn * rho * np.sin(yaw), cy - sgn * rho * np.cos(yaw)
        x, y = x + straight * np.cos(yaw), y + straight * np.sin(yaw)
    return x, y, (np.pi / 2 - yaw) % (2 * np.pi)


def _ahead_targets(pose, n):
    """n targets some way ahead of the pose, a little to either side, heading as the pose's: a short first arc, so no member of any
    class at slow speed (the horizon ends on the straight)."""
    x0, y0, h0 = pose
    yaw = np.pi / 2 - h0
    k = np.arange(n)
    fwd, side = 40.0 + 0.05 * k, np.where(k % 2 == 0, 2.0, -2.0) + 0.001 * k
    return np.stack([x0 + fwd * np.cos(yaw) - side * np.sin(yaw), y0 + fwd * np.sin(yaw) + side * np.cos(yaw), np.full(n, h0)], axis=1)


def _root_pose(w):
    return float(w.start5[0]), float(w.start5[1]), float(w.start5[2])


def _reach(w):
    return w.cfg.slow_speed * w.cfg.time_horizon


def _check(torch, w, verts, edges_vi, edges_cfg, run, what):
    """run(handle) -> (records, child).  Off and on handles are the caller's; returns the on handle's shared count checked."""
    (off, on) = run
    res_off, res_on, shared = off[0], on[0], on[2]
    want, ok, key = _rule(w, verts, edges_vi, edges_cfg, res_off[0])
    print(what, "edges", len(res_off[0]), "shared", shared, "rule", want, "classes", len(np.unique(key[ok])))
    assert _same_bytes(res_on, res_off), what
    assert want > 0 and shared == want, (what, shared, want)
    return ok, key


def test_dense_launch_one_vertex_257_samples(torch_cuda, monkeypatch):
    """1 vertex x 257 samples x 0xF: work items run configuration-major (3, 2, 1, 0), 257 to a configuration, and the slow lanes
    (items 0 .. 513) write their fast partners' records too.  Class (3, left) has its lowest member, sample 200, in the last wave of
    workgroup 0 and more of them in that wave; class (3, right) has members in every wave of workgroup 0; class (2, right) has its only
    members, samples 255 and 256, in items 512 and 513: the two working lanes of the last workgroup that has any."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=64)
    root = _root_pose(w)
    rc, rt, reach = w.cfg.coverage_turning_radius, w.cfg.turning_radius, _reach(w)
    t = _ahead_targets(root, 257)
    for k, s in enumerate((200, 230, 250)):
        t[s] = _arc_target(root, rc, True, reach + 4.0 + k)
    for k, s in enumerate((10, 70, 130, 199)):
        t[s] = _arc_target(root, rc, False, reach + 4.0 + k)
    for k, s in enumerate((255, 256)):
        t[s] = _arc_target(root, rt, False, reach + 4.0 + k)
    runs = []
    for share in (False, True):
        ctx = _handle(w, share, monkeypatch)
        ctx.set_samples(t[:, 0], t[:, 1], t[:, 2])
        runs.append((_dense(torch_cuda, ctx, 257, STRIDE), None, ctx.last_shared_edges()))
        ctx.close()
    assert runs[0][2] == 0
    cfgs = np.tile(np.arange(4), 257)
    sample = np.repeat(np.arange(257), 4)
    ok, key = _check(torch_cuda, w, w.root(), np.zeros(4 * 257, dtype=np.int64), cfgs, runs, "dense 257")
    members = lambda k: sample[ok & (key == k)]
    assert members(3 * 2 + 0).min() == 200 and len(members(3 * 2 + 0)) >= 3           # item 200: wave 3 of workgroup 0
    assert set((10, 70, 130, 199)) <= set(members(3 * 2 + 1))
    assert sorted(members(2 * 2 + 1)) == [255, 256]                                   # items 257 + 255, 257 + 256


def test_explicit_list_lowest_member_in_the_last_workgroup(torch_cuda, monkeypatch):
    """An explicit list of 1 000 edges of one vertex (one lane per edge, item = position; workgroups of 256), shuffled configurations.
    Class (3, left) lives in the last workgroup only, in three of its waves, so the highest-numbered workgroup holds its lowest
    position; class (3, right) has members in all four waves of workgroup 0 and in workgroups 1 and 2; class (2, left) has two
    members in one wave."""
    from path_planner_amd import workloads
    from path_planner_amd.types import edge_pack
    w = workloads.config3(n_samples=64)
    root = _root_pose(w)
    rc, rt, reach = w.cfg.coverage_turning_radius, w.cfg.turning_radius, _reach(w)
    n_bg = 200
    t = list(_ahead_targets(root, n_bg))
    t += [_arc_target(root, rc, True, reach + 3.0 + k) for k in range(4)]        # targets n_bg .. n_bg + 3: (3, left)
    t += [_arc_target(root, rc, False, reach + 3.0 + k) for k in range(8)]       # n_bg + 4 .. n_bg + 11: (3, right)
    t += [_arc_target(root, rt, True, reach + 3.0 + k) for k in range(2)]        # n_bg + 12, 13: (2, left)
    t = np.asarray(t)
    rng = np.random.default_rng(7)
    n = 1000
    target, cfgs = rng.integers(0, n_bg, n), rng.integers(0, 4, n)
    place = {3 * 2 + 0: [(770, n_bg), (830, n_bg + 1), (835, n_bg + 2), (990, n_bg + 3)],
             3 * 2 + 1: [(5, n_bg + 4), (66, n_bg + 5), (130, n_bg + 6), (131, n_bg + 7), (255, n_bg + 8), (300, n_bg + 9), (600, n_bg + 10), (601, n_bg + 11)],
             2 * 2 + 0: [(400, n_bg + 12), (401, n_bg + 13)]}
    for k, spots in place.items():
        for pos, tg in spots:
            target[pos], cfgs[pos] = tg, k // 2
    edges = edge_pack(np.zeros(n, dtype=np.uint64), target, cfgs)
    runs = []
    for share in (False, True):
        ctx = _handle(w, share, monkeypatch)
        ctx.set_samples(t[:, 0], t[:, 1], t[:, 2])
        runs.append((_list(torch_cuda, ctx, edges, STRIDE), None, ctx.last_shared_edges()))
        ctx.close()
    assert runs[0][2] == 0
    ok, key = _check(torch_cuda, w, w.root(), np.zeros(n, dtype=np.int64), cfgs, runs, "explicit list")
    pos = np.arange(n)
    for k, spots in place.items():
        assert sorted(pos[ok & (key == k)]) == sorted(p for p, _ in spots), k
    assert pos[ok & (key == 6)].min() // 256 == (n - 1) // 256


def _open_vertices(w, ctx, n, stride):
    """The root and 63 of its children (as test_gpu_shared_sweeps.py's check 3 and bench.py's open-vertex run build them)."""
    from path_planner_amd.types import VERTEX_DTYPE, F_INFEASIBLE, F_GOAL, edge_pack
    res, child = ctx.cost_edges_host(edge_pack(np.zeros(4 * n, dtype=np.uint64), np.arange(4 * n) // 4, np.arange(4 * n) % 4), stride=stride)
    ok = np.nonzero(((res["flags"] & (F_INFEASIBLE | F_GOAL)) == 0) & (((res["info"] >> 8) & 0xFF) <= stride))[0][:63]
    v = np.zeros(len(ok) + 1, dtype=VERTEX_DTYPE)
    pool = [np.asarray(w.ribbons4, dtype=np.float64).reshape(-1, 4)]
    v[0] = w.root()[0]
    off = len(pool[0])
    for k, e in enumerate(ok):
        r, nr = res[e], int((res[e]["info"] >> 8) & 0xFF)
        v[k + 1] = (r["end_x"], r["end_y"], r["end_heading"], r["end_speed"], r["end_time"], r["g"], r["coverage_completed_time"], off, nr)
        pool.append(child[e, :nr]); off += nr
    return v, np.concatenate(pool)


def test_64_open_vertices_reach_the_last_entry_of_the_table(torch_cuda, monkeypatch):
    """64 open vertices x 48 targets x 0xF, dense: 512 classes, the table's last entry (vertex 63, class 7 = configuration 3, right)
    among them; four of the targets lie one arc away from vertex 63 and four from vertex 0, on both circles."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=1024)
    stride = 12
    runs, keep = [], None
    for share in (False, True):
        ctx = _handle(w, share, monkeypatch)
        ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
        n = ctx.sampler_add(1024)
        v, pool = _open_vertices(w, ctx, n, stride)
        assert len(v) == 64
        samples = ctx.get_samples()[:40, :3]
        last = (float(v["x"][63]), float(v["y"][63]), float(v["heading"][63]))
        rc, reach = w.cfg.coverage_turning_radius, _reach(w)
        extra = [_arc_target(last, rc, False, reach + 5.0), _arc_target(last, rc, False, reach + 6.0), _arc_target(last, rc, True, reach + 5.0),
                 _arc_target(last, rc, True, reach + 6.0)] + [_arc_target(_root_pose(w), rc, lr, reach + d) for lr in (True, False) for d in (5.0, 6.0)]
        t = np.concatenate([samples, np.asarray(extra)])
        ctx.set_vertices(v, pool)
        ctx.set_samples(t[:, 0], t[:, 1], t[:, 2])
        from test_gpu_parity import _dense as dense
        runs.append((dense(torch_cuda, ctx, 64, len(t), 0xF, stride), None, ctx.last_shared_edges()))
        keep = v, len(t)
        ctx.close()
    assert runs[0][2] == 0
    v, ns = keep
    vi = np.repeat(np.arange(64), ns * 4)
    cfgs = np.tile(np.arange(4), 64 * ns)
    ok, key = _check(torch_cuda, w, v, vi, cfgs, runs, "64 open vertices")
    assert np.count_nonzero(ok & (key == 63 * 8 + 7)) >= 2 and np.count_nonzero(ok & (key == 7)) >= 2
    assert len(np.unique(key[ok] // 8)) == 64            # every vertex has a class with members


def test_three_slices_members_behind_an_earlier_head(torch_cuda, monkeypatch):
    """The sampler's 75 attempts from the root, dense 0xF, cut into three slices (PPGPU_SLICE_BYTES, the setting test_gpu_sweep_list.py
    and test_gpu_shared_sweeps.py use, sized here for a third of the launch): members of the second and third slice find their head,
    elected in an earlier slice, with the plain look."""
    from path_planner_amd import workloads
    from test_gpu_heuristic_routes import dense_edges
    from test_gpu_sweep_list import _steps_per_row
    w = workloads.config3(n_samples=75)
    nch = _steps_per_row(w.cfg)[1]
    per_edge = 256 + nch * 64 * 2 + nch * 12 + 16          # workspace bytes of an edge (cost_modes): setup record, track rows, summary
    runs, slices, n = [], None, 75
    for share in (False, True):
        env = {"PPGPU_SLICE_BYTES": str(per_edge * -(-4 * n // 3) + 64)} if share else {}      # (n: what the off handle's sampler kept)
        ctx = _handle(w, share, monkeypatch, **env)
        ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
        n = ctx.sampler_add(75)
        edges = dense_edges(n, 0xF)
        runs.append((ctx.cost_edges_host(edges, stride=STRIDE), None, ctx.last_shared_edges()))
        slices = ctx.last_slices()
        ctx.close()
    assert runs[0][2] == 0
    print("slices", slices)
    assert slices[0] == 3, slices
    cfgs = np.tile(np.arange(4), n)
    ok, key = _check(torch_cuda, w, w.root(), np.zeros(4 * n, dtype=np.int64), cfgs, runs, "three slices")
    per = -(-len(cfgs) // 3)
    pos = np.arange(len(cfgs))
    behind = sum(int(np.count_nonzero(pos[ok & (key == k)] // per > pos[ok & (key == k)].min() // per)) for k in np.unique(key[ok]))
    assert behind > 0


def test_launches_back_to_back_on_one_handle(torch_cuda, monkeypatch):
    """One handle with sharing on, one with it off, the same launches on both, each compared: (1) three vertices, dense; (2) a smaller
    list of vertex 0 alone whose members all lie BEHIND position 100, where launch 1 left heads at positions of one digit: a head that
    outlived launch 1 would be taken for theirs; (3) 40 vertices, more than ever before, so the table is a new one; (4) a launch of
    given curves, which shares nothing (the only launch of such a handle that does not), then (5) launch 2 again."""
    from path_planner_amd import workloads
    from path_planner_amd.types import VERTEX_DTYPE, edge_pack
    from test_gpu_parity import _dense as dense
    from test_gpu_solve_ranked import _given_curves
    w = workloads.config3(n_samples=64)
    root = _root_pose(w)
    rc, rt, reach = w.cfg.coverage_turning_radius, w.cfg.turning_radius, _reach(w)
    # targets 0 .. 11 one arc away on the four circles through the root (members, so launch 1's heads of vertex 0 come early), then 120 ahead of it
    t = np.concatenate([np.asarray([_arc_target(root, r, lr, reach + 3.0 + k) for r in (rc, rt) for lr in (True, False) for k in range(3)]), _ahead_targets(root, 120)])
    ns = len(t)

    def verts(n):
        v = np.zeros(n, dtype=VERTEX_DTYPE)
        v[:] = w.root()[0]
        v["heading"] = root[2] + 0.05 * np.arange(n)
        return v

    v3, v40 = verts(3), verts(40)
    rng = np.random.default_rng(3)
    n2 = 600
    target2 = np.concatenate([rng.integers(12, ns, 100), rng.integers(0, ns, n2 - 100)])
    cfg2 = np.concatenate([rng.integers(0, 4, 100), rng.choice([0, 1, 3], n2 - 100)])              # (no class of configuration 2)
    edges2 = edge_pack(np.zeros(n2, dtype=np.uint64), target2, cfg2)
    out = []
    for share in (False, True):
        ctx = _handle(w, share, monkeypatch, verts=v3)
        ctx.set_samples(t[:, 0], t[:, 1], t[:, 2])
        steps = [("three vertices", dense(torch_cuda, ctx, 3, ns, 0xF, STRIDE), ctx.last_shared_edges())]
        steps.append(("smaller list", _list(torch_cuda, ctx, edges2, STRIDE), ctx.last_shared_edges()))
        ctx.set_vertices(v40, w.ribbons4)
        steps.append(("forty vertices", dense(torch_cuda, ctx, 40, ns, 0xF, STRIDE), ctx.last_shared_edges()))
        ctx.cost_wrapper_edges_host(_given_curves(w, v40), stride=STRIDE)
        assert ctx.last_shared_edges() == 0
        steps.append(("smaller list again", _list(torch_cuda, ctx, edges2, STRIDE), ctx.last_shared_edges()))
        out.append(steps)
        ctx.close()
    dense_keys = lambda nv: (np.repeat(np.arange(nv), ns * 4), np.tile(np.arange(4), nv * ns))
    lists = {"three vertices": (v3,) + dense_keys(3), "smaller list": (v3, np.zeros(n2, dtype=np.int64), cfg2),
             "forty vertices": (v40,) + dense_keys(40), "smaller list again": (v40, np.zeros(n2, dtype=np.int64), cfg2)}
    for (what, off, n_off), (_, on, n_on) in zip(*out):
        assert n_off == 0
        v, vi, cfgs = lists[what]
        ok, key = _check(torch_cuda, w, v, vi, cfgs, ((off, None, 0), (on, None, n_on)), what)
        if what == "three vertices":
            heads1 = {int(k): int(np.nonzero(ok & (key == k))[0].min()) for k in np.unique(key[ok])}
        if what.startswith("smaller list"):
            # every member of launch 2 lies behind position 100, and launch 1 had heads of the same classes before it
            assert np.nonzero(ok)[0].min() >= 100
            assert sum(heads1.get(int(k), 1 << 30) < 100 for k in np.unique(key[ok])) >= 2
