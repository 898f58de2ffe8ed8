"""-m gpu: pp_k_solve_edges ranks the six Dubins words on the library's atan2 / acos and evaluates only the contenders correctly
rounded (pp_solve_rank.h), and pp_curve_init takes sin / cos of a base heading once (PPSincosMemo).  The records and child lists
of the default handle must be, byte for byte, those of a handle created with PPGPU_SOLVE_ALL_WORDS=1, which evaluates all six
words and every base heading as before: on targets chosen to sit on the solver's decisions (straight ahead and behind, mirror
images, tangent circles, co-located poses, headings a hair off the line to the target, d at the solver's fallback threshold and
beyond it, a distance whose ranked costs are not finite) and on random ones, through the dense
enumeration, an explicit list and given curves, with the prepasses forced on and at the production threshold.
The targets are poses, so "p_sq exactly 0" and "|tmp0| exactly 1" are only approached here: the tangent circles are laid out with
cos / sin of rounded angles and land within a few ulp of those limits, on either side.  The exact zeros and ones are fed to the
selection itself by tests/test_solve_rank.py, on the CPU, with a million random problems.  The fallback, by contrast, is the
device's own comparison and select, and is run here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDE = 8
N_SAMPLES = 512
MAX_D = 65536.0                 # PP_RANK_MAX_D


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def world():
    from path_planner_amd import workloads
    from path_planner_amd.types import VERTEX_DTYPE
    w = workloads.config2()
    root = w.root()
    verts = np.zeros(3, dtype=VERTEX_DTYPE)
    verts[:] = root[0]
    verts["heading"] = [0.0, 1.0, np.pi / 2]        # yaw pi/2, pi/2 - 1 and +0.0
    return w, verts, _targets(w, verts)


def _targets(w, verts):
    """At most N_SAMPLES targets {x, y, heading}: the adversarial list, laid out around vertex 0 for both turning radii, then
    random ones."""
    x0, y0 = float(verts["x"][0]), float(verts["y"][0])
    yaw0 = np.pi / 2 - float(verts["heading"][0])
    out = []

    def add(theta, dist, yaw):
        out.append((x0 + dist * np.cos(theta), y0 + dist * np.sin(theta), np.pi / 2 - yaw))

    for rho in (w.cfg.turning_radius, w.cfg.coverage_turning_radius):
        for L in (0.5, 2.0, 4.0, 10.0):
            for eps in (0.0, 1e-12, -1e-12, 1e-9):
                add(yaw0, L * rho, yaw0 + eps)                     # straight ahead, heading on / a hair off the line
                add(yaw0 + np.pi, L * rho, yaw0 + eps)             # straight behind
                add(yaw0 + eps, L * rho, yaw0)                     # the line itself a hair off the start heading
                add(yaw0, L * rho, yaw0 + np.pi + eps)             # ahead, facing back
            for a in (0.3, 1.0, np.pi / 2, 2.5, np.pi):            # mirror images: alpha = a, beta = -a; and beta = a + pi
                add(yaw0 - a, L * rho, yaw0 - 2 * a)
                add(yaw0 + a, L * rho, yaw0 + 2 * a)
                add(yaw0 - a, L * rho, yaw0 + np.pi)
        for side in (1.0, -1.0):                                   # circles that touch: p_sq and |tmp0| at their limits
            add(yaw0 + side * np.pi / 2, 2.0 * rho, yaw0 + np.pi)
            add(yaw0 + side * np.pi / 2, 4.0 * rho, yaw0)
            add(yaw0 + side * np.pi / 2, 2.0 * rho, yaw0)
    for h in (0.0, 1.0, np.pi / 2, 3.0):                           # co-located with the three vertices (positions equal)
        out.append((x0, y0, h))
    # d = distance / rho at the fallback threshold PP_RANK_MAX_D = 65 536 of pp_solve_rank.h (at it the words are still ranked, beyond
    # it every feasible word is evaluated), a step and a part in 1e9 on both sides of it, far beyond it, and so far that the ranked
    # costs are not finite (1e200 m: the squared distance overflows), for both radii, ahead, behind and to the side
    for rho in (w.cfg.turning_radius, w.cfg.coverage_turning_radius):
        at = MAX_D * rho
        for dist in (at, np.nextafter(at, 0.0), np.nextafter(at, np.inf), at * (1 - 1e-9), at * (1 + 1e-9), 2 * at, 1e3 * at, 1e200):
            add(yaw0, dist, yaw0 + 0.3)
            add(yaw0 + np.pi, dist, yaw0 - 2.0)
            add(yaw0 + np.pi / 2, dist, yaw0 + np.pi)
            out.append((x0 + dist, y0, 1.0))                       # (along an axis: the distance is the coordinate difference)
    assert len(out) < N_SAMPLES - 100
    rng = np.random.default_rng(23)
    while len(out) < N_SAMPLES:
        out.append((x0 + rng.uniform(-60, 60), y0 + rng.uniform(-60, 60), rng.uniform(0, 2 * np.pi)))
    return np.asarray(out, dtype=np.float64)


def _context(world, monkeypatch, all_words):
    from path_planner_amd import api
    w, verts, tg = world
    if all_words:
        monkeypatch.setenv("PPGPU_SOLVE_ALL_WORDS", "1")
    else:
        monkeypatch.delenv("PPGPU_SOLVE_ALL_WORDS", raising=False)
    ctx = api.Context(0)                # (the switch is read when the handle is created)
    ctx.set_config(w.cfg)
    ctx.set_grid(w.grid, w.res)
    ctx.set_obstacles(w.obst)
    ctx.set_vertices(verts, w.ribbons4)
    ctx.set_samples(tg[:, 0], tg[:, 1], tg[:, 2])
    return ctx


def _dense(torch, ctx, nv, ns, mask):
    from path_planner_amd import api
    from path_planner_amd.types import RESULT_DTYPE
    ne = api.Context.dense_edge_count(nv, ns, mask)
    d_res = torch.zeros(ne * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_child = torch.zeros(ne * STRIDE * 4, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()      # the fill ran on torch's stream, the library works on its own
    ctx.cost_edges_dense(0, nv, 0, ns, mask, d_res.data_ptr(), d_child.data_ptr(), STRIDE)
    ctx.synchronize()
    return d_res.cpu().numpy().view(RESULT_DTYPE), d_child.cpu().numpy().reshape(ne, STRIDE, 4)


def _rows_differing(a, b):
    return int(np.count_nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)))


@pytest.mark.parametrize("prepass_min_edges", ["0", None])
def test_ranked_solver_gives_the_records_of_all_six_words(torch_cuda, world, monkeypatch, prepass_min_edges):
    from path_planner_amd.types import edge_pack, F_INFEASIBLE
    if prepass_min_edges is None:
        monkeypatch.delenv("PPGPU_PREPASS_MIN_EDGES", raising=False)      # the production threshold
    else:
        monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", prepass_min_edges)
    w, verts, tg = world
    nv, ns = len(verts), len(tg)
    rng = np.random.default_rng(5)
    pos = rng.permutation(nv * ns * 4)[:2000]
    edges = edge_pack(pos // (4 * ns), (pos // 4) % ns, pos % 4)
    got = {}
    for all_words in (False, True):
        ctx = _context(world, monkeypatch, all_words)
        got[all_words] = [_dense(torch_cuda, ctx, nv, ns, 0xF), _dense(torch_cuda, ctx, nv, ns, 0x5), ctx.cost_edges_host(edges, stride=STRIDE)]
        ctx.close()
    for what, (res, child), (ares, achild) in zip(("dense 0xF", "dense 0x5", "explicit list"), got[False], got[True]):
        assert len(res) == len(ares) > 0
        assert res.tobytes() == ares.tobytes(), "%s: records differ in %d edges" % (what, _rows_differing(res, ares))
        assert child.tobytes() == achild.tobytes(), "%s: child lists differ" % what
    res = got[False][0][0]
    assert np.count_nonzero((res["flags"] & F_INFEASIBLE) == 0) > 200          # real edges, not a world of refusals


def _given_curves(w, verts):
    """Curves handed over as DubinsWrapper fields: every word with p0 = 0, p1 = 0, both, and all three, from start yaws -0.0, +0.0,
    pi/2 and 1 (the memo compares bits: 0.0 + -0.0 is +0.0, another argument), then random ones."""
    from path_planner_amd.types import WRAPPER_EDGE_DTYPE
    x0, y0, t0 = float(verts["x"][0]), float(verts["y"][0]), float(verts["time"][0])
    rows = []
    rng = np.random.default_rng(31)
    for word in range(6):
        for qth in (-0.0, 0.0, np.pi / 2, 1.0):
            for p in ((0.0, 0.7, 0.9), (0.6, 0.0, 0.9), (0.0, 0.0, 1.1), (0.0, 0.0, 0.0), (0.5, 1.5, 0.0), (-0.0, 1.0, 0.5)):
                rows.append((word, qth, p))
    for _ in range(112):
        rows.append((int(rng.integers(0, 6)), float(rng.uniform(-3.2, 6.4)), tuple(rng.uniform(0.0, 3.0, 3))))
    we = np.zeros(len(rows), dtype=WRAPPER_EDGE_DTYPE)
    for k, (word, qth, p) in enumerate(rows):
        rho = w.cfg.turning_radius if k % 2 == 0 else w.cfg.coverage_turning_radius
        speed = w.cfg.max_speed
        we[k]["vertex"] = 0
        we[k]["coverage_allowed"] = k % 2
        we[k]["qi"] = (x0, y0, qth)
        we[k]["param"] = p
        we[k]["rho"] = rho
        we[k]["type"] = word
        we[k]["speed"] = speed
        we[k]["start_time"] = t0
        we[k]["end_time"] = t0 + (p[0] + p[1] + p[2]) * rho / speed
    return we


def test_given_curves_with_repeated_base_headings(torch_cuda, world, monkeypatch):
    w, verts, _ = world
    we = _given_curves(w, verts)
    got = {}
    for all_words in (False, True):
        ctx = _context(world, monkeypatch, all_words)
        got[all_words] = ctx.cost_wrapper_edges_host(we, stride=STRIDE)
        ctx.close()
    (res, child), (ares, achild) = got[False], got[True]
    assert len(res) == len(we)
    assert res.tobytes() == ares.tobytes(), "records differ in %d curves" % int(np.count_nonzero(res != ares))
    assert child.tobytes() == achild.tobytes()
