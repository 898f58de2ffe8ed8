"""-m gpu: the sweep list (pp_k_mark_sweeps, pp_k_solve.h).  A launch with shared sweeps packs the slice positions of the edges that are
swept at all into a list, and the skip planner (all six pp_k_plan_skips* kernels), the pose sweep and the approach kernel walk that list
instead of every edge.  Every test here costs the same edges with the list on and off (PPGPU_SWEEP_LIST, read by ppgpu_create) and wants the same bytes
in the records and the child ribbons, and holds ppgpu_last_swept_edges against edges - shared - unsolved: a number below the launch's
edge count, so that no test passes with the list unused.  conftest.py forces the prepasses, and so the sharing and the list, onto
launches of any size."""
import numpy as np
import pytest

from test_gpu_shared_sweeps import _dense, _list, _oracle, _same_bytes

pytestmark = pytest.mark.gpu

PP_WPB = 4        # waves (= list entries) per workgroup of the pose sweep


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _switch(monkeypatch, listed, **env):
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", "0")
    monkeypatch.delenv("PPGPU_SHARE_SWEEPS", raising=False)
    for k in ("PPGPU_PLAN_SPANS", "PPGPU_SLICE_BYTES", "PPGPU_APPROACH_LIST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if listed:
        monkeypatch.delenv("PPGPU_SWEEP_LIST", raising=False)
    else:
        monkeypatch.setenv("PPGPU_SWEEP_LIST", "0")


def _context(w, n_samples, listed, monkeypatch, gaussian=False, **env):
    """A handle on workload w with its sampler's first n_samples attempts, created with the switch set as `listed` says."""
    from path_planner_amd import api
    _switch(monkeypatch, listed, **env)
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.set_grid(w.grid, w.res)
    if gaussian:
        ctx.set_gaussian_obstacles(np.ascontiguousarray(w.obst[:, :5]))
    else:
        ctx.set_obstacles(w.obst)
    ctx.set_vertices(w.root(), w.ribbons4)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    return ctx, ctx.sampler_add(n_samples)


def _unsolved(records):
    """Edges no kernel sweeps for want of a curve: malformed, co-located, or without a Dubins word.  From the root of these worlds
    nothing else raises PPGPU_F_THROWS (a solved curve from the root contains its end time)."""
    from path_planner_amd.types import F_THROWS
    return int(np.count_nonzero(records["flags"] & F_THROWS))


def _counts(ctx, records, what):
    edges, shared, swept, unsolved = len(records), ctx.last_shared_edges(), ctx.last_swept_edges(), _unsolved(records)
    print(what, "edges", edges, "shared", shared, "unsolved", unsolved, "swept", swept)
    assert swept == edges - shared - unsolved, (what, edges, shared, unsolved, swept)
    return shared, swept


def _steps_per_row(cfg):
    """Entries of a vertex's time row, as ppgpu_set_config computes them, and the 64-step chunks they make."""
    ng = int(cfg.time_horizon / (cfg.collision_checking_increment / cfg.max_speed)) + 8
    return ng, (ng + 63) // 64


@pytest.fixture(scope="module")
def dense_off(torch_cuda):
    """Config 3, 2 048 attempts, dense 0xF with the list off: costed once, read-only, for the tests that want its bytes."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=2048)
    with pytest.MonkeyPatch.context() as mp:
        off, n = _context(w, 2048, False, mp)
        want = _dense(torch_cuda, off, n, 8)
        assert off.last_shared_edges() > 0                      # (sweeps are shared either way: only the walk differs)
        assert off.last_swept_edges() == len(want[0])           # no list: every edge is walked
    for a in want:
        a.setflags(write=False)
    return w, n, want


def test_dense_launch_on_is_off_and_the_oracle(torch_cuda, monkeypatch, dense_off):
    from parity import compare_results
    from test_gpu_heuristic_routes import dense_edges
    w, n, want = dense_off
    on, n_on = _context(w, 2048, True, monkeypatch)
    got = _dense(torch_cuda, on, n_on, 8)
    assert n_on == n and _same_bytes(got, want)
    shared, swept = _counts(on, got[0], "dense")
    assert shared > 0 and swept < len(got[0])
    world, cs = _oracle(w, 2048)
    cpu, cchild = world.cost_edges(w.root(), w.ribbons4, cs[:, 0], cs[:, 1], cs[:, 2], dense_edges(n, 0xF), stride=8, threads=8)
    rep = compare_results(got[0], cpu, got[1], cchild)
    assert rep["ok"], rep


def test_the_same_launch_in_slices(torch_cuda, monkeypatch, dense_off):
    """Three slices, the last one ragged: the per-slice count is cleared with the live list's, the per-launch total is not, and a
    member whose head lies in an earlier slice stays off its own slice's list."""
    w, n, want = dense_off
    ng, nch = _steps_per_row(w.cfg)
    per_edge = 256 + nch * 64 * 2 + nch * (8 + 4) + 16         # about what cost_modes counts; the handle says below how it really cut
    edges = len(want[0])
    per_slice = edges * 2 // 5
    whole, _ = _context(w, 2048, True, monkeypatch)
    got_whole = _dense(torch_cuda, whole, n, 8)
    shared_whole, swept_whole = _counts(whole, got_whole[0], "whole")
    cut, _ = _context(w, 2048, True, monkeypatch, PPGPU_SLICE_BYTES=str(per_slice * per_edge + per_edge // 2))
    got = _dense(torch_cuda, cut, n, 8)
    n_slices, last_slice = cut.last_slices()
    print("slices", n_slices, "edges of the last", last_slice)
    assert whole.last_slices() == (1, edges)
    assert n_slices >= 3 and last_slice < (edges - last_slice) // (n_slices - 1), (n_slices, last_slice)     # a ragged last one
    assert _same_bytes(got, want) and _same_bytes(got_whole, want)
    shared, swept = _counts(cut, got[0], "sliced (%d edges per slice)" % per_slice)
    assert (shared, swept) == (shared_whole, swept_whole)


def _explicit_world(n_targets):
    """Config 3's root, n_targets of its samples, and one more target AT the root: an edge to it is co-located."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=256)
    world, cs = _oracle(w, 256)
    assert len(cs) >= n_targets
    x0, y0, h0 = w.start5[0], w.start5[1], w.start5[2]
    t = np.concatenate([cs[:n_targets, :3], [[x0, y0, h0]]])
    return w, np.ascontiguousarray(t, dtype=np.float64)


def _ragged_list(n_edges, sweepable_at, n_targets):
    """n_edges descriptors: configuration 0 (fast, the tight radius: the horizon never ends on its first arc, so none of them is
    shared) to distinct targets at the positions `sweepable_at`; everywhere else an edge nobody sweeps, by turns one from a vertex
    that does not exist and one to the target at the root."""
    from path_planner_amd.types import edge_pack
    vertex = np.zeros(n_edges, dtype=np.uint64)
    target = np.zeros(n_edges, dtype=np.int64)
    good = np.zeros(n_edges, dtype=bool)
    good[list(sweepable_at)] = True
    target[good] = np.arange(int(good.sum())) % n_targets
    bad = np.nonzero(~good)[0]
    vertex[bad[0::2]] = 5                                       # one open vertex: index 5 is out of range
    target[bad[1::2]] = n_targets                               # the co-located target
    return edge_pack(vertex, target, np.zeros(n_edges, dtype=np.int64)), int(good.sum())


def _ragged_cases():
    ng, nch = 1508, 24                                          # config 3: asserted in the test
    epw = 256 // nch                                            # 10 edges per workgroup of the skip planner
    cases = {
        "none": (100, []),                                      # a count of 0: every workgroup of both kernels leaves
        "one": (100, [57]),
        "first_and_last": (100, [0, 99]),
        "not_a_multiple_of_wpb": (100, list(range(5, 95))),     # 90 = 9 epw, 22 PP_WPB + 2
        "not_a_multiple_of_epw": (100, list(range(3, 95))),     # 92 = 23 PP_WPB, 9 epw + 2
        "all": (100, list(range(100))),
        "single_swept": (1, [0]),
        "single_unswept": (1, []),
    }
    assert 90 % epw == 0 and 90 % PP_WPB != 0 and 92 % PP_WPB == 0 and 92 % epw != 0
    return cases


@pytest.mark.parametrize("case", list(_ragged_cases()))
def test_lists_that_are_ragged_at_their_ends(torch_cuda, monkeypatch, case):
    n_edges, at = _ragged_cases()[case]
    n_targets = 100
    w, t = _explicit_world(n_targets)
    assert _steps_per_row(w.cfg) == (1508, 24)
    edges, n_good = _ragged_list(n_edges, at, n_targets)
    runs = {}
    for listed in (False, True):
        ctx, _ = _context(w, 64, listed, monkeypatch)
        ctx.set_samples(t[:, 0], t[:, 1], t[:, 2])
        runs[listed] = _list(torch_cuda, ctx, edges, 8), ctx
    (off, off_ctx), (on, on_ctx) = runs[False], runs[True]
    assert _same_bytes(on, off)
    assert off_ctx.last_swept_edges() == n_edges
    shared, swept = _counts(on_ctx, on[0], case)
    assert shared == 0 and swept == n_good and _unsolved(on[0]) == n_edges - n_good


def test_long_edges(torch_cuda, monkeypatch):
    """258 chunks per edge: the pose sweep's walk takes further groups of 64 skip bytes on an edge it found through the list, and the
    planner runs one edge per workgroup (epw == 1) with a second blockIdx.y tile of 256 chunks."""
    import sweep_worlds as sw
    from test_gpu_sweep_inputs import _dense as dense_world
    w = sw.long_(16500)
    assert (w.ng + 63) // 64 > 256 and 256 // ((w.ng + 63) // 64) == 0
    runs = {}
    for listed in (False, True):
        _switch(monkeypatch, listed)
        ctx = w.context()
        runs[listed] = dense_world(torch_cuda, ctx, w), ctx
    (off, _), (on, on_ctx) = runs[False], runs[True]
    assert _same_bytes(on, off)
    assert int((on[0]["info"] >> 16).max()) > 256 * 64          # some edge runs past the planner's first tile
    shared, swept = _counts(on_ctx, on[0], "long16500")
    assert shared == 0 or swept < len(on[0])


@pytest.mark.parametrize("what", ["chunkwise", "many", "gaussian", "approach_direct"])
def test_the_other_planner_bodies_and_sweeps(torch_cuda, monkeypatch, what):
    """PPGPU_PLAN_SPANS=0: pp_k_plan_skips_chunkwise.  80 obstacles: pp_k_plan_skips_many, and the pose sweep without its obstacle
    lanes.  The Gaussian model: pp_k_plan_skips_gaussian and pp_k_pose_sweep_gaussian.  PPGPU_APPROACH_LIST=0: the approach kernel
    alone walks the slice on a launch with a list (pp_k_approach_events_direct), and pp_k_mark_sweeps leaves track_far to it."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=512, n_obst=80) if what == "many" else workloads.config3(n_samples=512)
    env = {"chunkwise": {"PPGPU_PLAN_SPANS": "0"}, "approach_direct": {"PPGPU_APPROACH_LIST": "0"}}.get(what, {})
    runs = {}
    for listed in (False, True):
        ctx, n = _context(w, 512, listed, monkeypatch, gaussian=(what == "gaussian"), **env)
        runs[listed] = _dense(torch_cuda, ctx, n, 8), ctx
    (off, _), (on, on_ctx) = runs[False], runs[True]
    assert _same_bytes(on, off)
    shared, swept = _counts(on_ctx, on[0], what)
    assert shared > 0 and swept < len(on[0])
