"""-m gpu: coverage traces (ppgpu_trace_cover_* -> pp_k_trace_cover) against the replay of tests/cover_replay.py, step by step,
and against the costing launch itself.

The replay is fed the DEVICE's poses and straight / blocked bits (ctx.trace_edges on the same list), so both sides of a comparison
see the same doubles; what differs is the executor of the state machine: the oracle's ribbons_min_distance / ribbons_cover on the
CPU, pp_ribbons_event on the device.  The worlds are the three of tests/cover_replay.py, built once and shared."""
import numpy as np
import pytest

import cover_replay as cr
from test_gpu_trace import STRIDE, _edge_curve, _rel, reference_times

pytestmark = pytest.mark.gpu

LIST_TOL = 1e-9          # metres: a final list against the costing launch's (the runs' own decision guard)
RIBBONS = 16             # ribbon_stride of the final lists: more than any list of these worlds


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _sentinel(dtype, byte):
    return np.frombuffer(np.full(dtype.itemsize, byte, dtype=np.uint8).tobytes(), dtype=dtype)[0]


_runs = {}


def device_run(name):
    """(world, step trace, coverage trace with sentinel-filled records) of world `name`: one context, computed once, left unchanged."""
    from path_planner_amd.types import COVER_DTYPE
    if name not in _runs:
        tw = cr.cover_world(name)
        ctx = tw.context()
        trace = ctx.trace_edges(tw.edges, STRIDE)
        cover = np.full((len(tw.edges), STRIDE), _sentinel(COVER_DTYPE, 0xA5), dtype=COVER_DTYPE)
        _runs[name] = (tw, trace, ctx.trace_cover(tw.edges, STRIDE, cover, ribbon_stride=RIBBONS))
    return _runs[name]


def _step_inputs(tw, vi, s, n):
    """What the replay needs of an edge's n device step records s."""
    from path_planner_amd.types import S_BLOCKED, S_STRAIGHT
    times = reference_times(tw.cfg, float(tw.verts["time"][vi]), n + 1)
    assert np.array_equal(s["time"], times[:n])
    return s["x"], s["y"], (s["flags"] & S_STRAIGHT) != 0, (s["flags"] & S_BLOCKED) != 0, times


def check_cover(tw, inputs, steps, counts, cover, ccounts, summ, final, stats):
    """Check 1 for the edges whose replay inputs are inputs[i] = (cov, ribbons, cct, vertex (x, y), vertex index)."""
    from parity import REL_TOL
    from path_planner_amd.types import CS_LAST_COVER, CS_LAST_CHANGED, CS_DONE, CS_REFUSED, CS_THROWS, C_EVENT
    for key in ("edges", "steps", "diverged", "splits", "trims", "erasures", "events", "worst_to_cover", "worst_remaining", "worst_final"):
        stats.setdefault(key, 0)
    for i, (cov, rib0, cct0, vxy, vi) in enumerate(inputs):
        n = int(counts[i])
        assert int(ccounts[i]) == n, (i, ccounts[i], n)
        c = cover[i, :n]
        assert np.array_equal(c["step"], np.arange(n)) and np.all(c["reserved"] == 0)
        assert not (summ["flags"][i] & (CS_REFUSED | CS_THROWS))
        xs, ys, straight, blocked, times = _step_inputs(tw, vi, steps[i, :n], n)
        r = cr.replay_edge(tw.cfg, cov, rib0, cct0, xs, ys, straight, blocked, times, vxy)
        stats["edges"] += 1
        stats["steps"] += n
        for key in ("splits", "trims", "erasures", "events"):
            stats[key] += getattr(r, key)
        print("edge", i, "steps", n, "events", r.events, int(summ["events"][i]), "changes", r.changes, int(summ["changes"][i]),
              "final", len(r.final), int(summ["ribbons_final"][i]))
        rel_tc, rel_rem = _rel(c["to_cover"], r.to_cover), _rel(c["remaining"], r.remaining)
        bad = (c["flags"] != r.flags) | (c["ribbons"] != r.ribbons) | (rel_tc > REL_TOL) | (rel_rem > REL_TOL)
        nf = int(summ["ribbons_final"][i])
        same_end = (int(summ["events"][i]) == r.events and int(summ["changes"][i]) == r.changes and nf == len(r.final) and
                    int(summ["flags"][i]) == r.summary_flags and
                    (nf == 0 or float(_rel(final[i, :nf], r.final).max()) <= REL_TOL) and
                    float(_rel(summ["remaining_final"][i], r.remaining_final)) <= REL_TOL and
                    (summ["coverage_completed_time"][i] == r.cct))
        if bad.any() or not same_end:
            k = int(np.argmax(bad)) if bad.any() else n
            knife = cr.knife_edge(tw.cfg, cov, rib0, cct0, xs, ys, straight, blocked, times, vxy, k)
            print("  edge", i, "leaves the replay at step", k, "of", n, "knife edge:", knife,
                  (c[k], r.to_cover[k], r.remaining[k], r.flags[k], r.ribbons[k]) if k < n else (summ[i], r.summary_flags, r.cct, len(r.final)))
            assert knife, (i, k)
            stats["diverged"] += 1
            continue
        if n:
            stats["worst_to_cover"] = max(stats["worst_to_cover"], float(rel_tc.max()))
            stats["worst_remaining"] = max(stats["worst_remaining"], float(rel_rem.max()))
        if nf:
            stats["worst_final"] = max(stats["worst_final"], float(_rel(final[i, :nf], r.final).max()))
        assert np.all(final[i, nf:] == 0.0)
        assert int(summ["events"][i]) == int(np.count_nonzero(c["flags"] & C_EVENT))
    print(stats)
    assert stats["diverged"] * cr.KNIFE_SHARE <= stats["edges"], stats
    return stats


@pytest.mark.parametrize("name", ["coverage", "cfg2", "cfg3"])
def test_every_step_against_the_replay(torch_cuda, name):
    """Check 1: counts, step indices, flags and list lengths identical on every step; to_cover and remaining within
    parity.REL_TOL; the summary identical, the final list within REL_TOL; nothing written beyond an edge's count; at most 1 edge
    in 20 may leave the replay, and only where the replay's own decision flips within 1e-9 (cover_replay.knife_edge).  The worlds
    hold the cases: splits, trims, erasures to an empty list, edges that leave a turn without covering, the done-at-start vertex,
    a blocked last step, edges longer than 64 steps."""
    from path_planner_amd.types import COVER_DTYPE, C_COVER, C_DONE, C_EVENT, S_BLOCKED
    tw, (res, counts, steps), (cres, ccounts, cover, summ, final) = device_run(name)
    assert cres.tobytes() == res.tobytes()
    stats = check_cover(tw, [cr.edge_inputs(tw, d) for d in tw.edges], steps, counts, cover, ccounts, summ, final, {})
    sentinel = _sentinel(COVER_DTYPE, 0xA5)
    for i in range(len(tw.edges)):                                     # nothing written beyond an edge's count
        assert cover[i, counts[i]:].tobytes() == np.full(STRIDE - counts[i], sentinel, dtype=COVER_DTYPE).tobytes()
    assert np.count_nonzero(counts > 64) >= 10
    valid = np.arange(STRIDE)[None, :] < counts[:, None]
    cfg_bits = (tw.edges >> np.uint64(56)).astype(np.int64)
    # events at which an edge that may not cover in turns (cfg bit 0 clear) indeed did not: it was turning
    turning = valid & ((cfg_bits & 1) == 0)[:, None] & ((cover["flags"] & C_EVENT) != 0) & ((cover["flags"] & C_COVER) == 0)
    print(name, "events without cover on non-coverage edges:", int(np.count_nonzero(turning)))
    assert np.count_nonzero(turning.any(axis=1)) >= 3
    if name == "coverage":
        assert stats["erasures"] >= 8
        done_start = ((tw.edges >> np.uint64(32)) & np.uint64(0xFFFFFF)) == 1     # the done-at-start vertex: done from the first record on
        assert done_start.sum() >= 10
        for i in np.nonzero(done_start)[0]:
            assert counts[i] > 0 and np.all(cover["flags"][i, :counts[i]] & C_DONE) and np.all(cover["ribbons"][i, :counts[i]] == 0)
            assert np.all(cover["to_cover"][i, :counts[i]] == 0.0) and summ["coverage_completed_time"][i] == 3.5
    if name == "cfg2":
        assert stats["splits"] >= 8
    if name == "cfg3":
        assert stats["splits"] >= 20 and stats["trims"] >= 2000
    if name != "coverage":                                              # a blocked last step
        last = steps["flags"][np.arange(len(counts)), np.maximum(counts - 1, 0)]
        assert np.count_nonzero((counts > 0) & ((last & S_BLOCKED) != 0)) >= 5


def check_against_costing(res, want, want_child, counts, summ, final, stats):
    """Check 2 on the edges the reference does not throw on."""
    from path_planner_amd.types import CS_DONE, CS_REFUSED, CS_THROWS, F_DONE, F_RIBBON_LOST, F_THROWS
    assert res.tobytes() == want.tobytes()
    throws = (res["flags"] & F_THROWS) != 0
    assert np.array_equal((summ["flags"] & CS_THROWS) != 0, throws)
    assert np.array_equal((summ["flags"] & CS_REFUSED) != 0, ~throws & ((res["flags"] & F_RIBBON_LOST) != 0))
    ok = (summ["flags"] & (CS_THROWS | CS_REFUSED)) == 0
    assert np.array_equal(counts[ok], (res["info"][ok] >> 16).astype(np.int32)) and np.all(counts[~ok] == 0)
    assert summ["coverage_completed_time"][ok].tobytes() == res["coverage_completed_time"][ok].tobytes()
    nf = ((res["info"] >> 8) & 0xFF).astype(np.int64)
    assert np.array_equal(summ["ribbons_final"][ok], nf[ok])
    assert np.array_equal((summ["flags"][ok] & CS_DONE) != 0, (res["flags"][ok] & F_DONE) != 0)
    worst = 0.0
    for i in np.nonzero(ok)[0]:
        m = min(int(nf[i]), final.shape[1])
        if m:
            worst = max(worst, float(np.abs(final[i, :m] - want_child[i, :m]).max()))
    stats["worst_list_difference_m"] = max(stats.get("worst_list_difference_m", 0.0), worst)
    print("final lists against the costing launch: worst difference", worst, "m over", int(ok.sum()), "edges")
    assert worst <= LIST_TOL, worst


@pytest.mark.parametrize("name", ["coverage", "cfg2", "cfg3"])
def test_against_the_costing_launch(torch_cuda, name):
    """Check 2: coverage_completed_time is the record's, bit for bit; ribbons_final its info bits 8-15; the done bit its
    PPGPU_F_DONE; the final list that of cost_edges_host within 1e-9 m; the records byte-identical."""
    tw, _, (cres, ccounts, cover, summ, final) = device_run(name)
    want, want_child = tw.context().cost_edges_host(tw.edges, stride=RIBBONS)
    check_against_costing(cres, want, want_child, ccounts, summ, final, {})


def test_stride_cuts_records_not_counts(torch_cuda):
    """Check 3: a step_stride of 100 — counts, summaries and final lists are whole, records [0, 100) are those of the uncut run,
    the sentinels beyond an edge's slot are intact."""
    from path_planner_amd.types import COVER_DTYPE
    tw, _, (res, counts, cover, summ, final) = device_run("cfg3")
    small = 100
    assert np.count_nonzero(counts > small) >= 10 and np.count_nonzero((counts > 0) & (counts < small)) >= 1
    sentinel = _sentinel(COVER_DTYPE, 0x5A)
    cut = np.full((len(tw.edges), small), sentinel, dtype=COVER_DTYPE)
    res2, counts2, cut, summ2, final2 = tw.context().trace_cover(tw.edges, small, cut, ribbon_stride=RIBBONS)
    assert res2.tobytes() == res.tobytes() and np.array_equal(counts2, counts)
    assert summ2.tobytes() == summ.tobytes() and final2.tobytes() == final.tobytes()
    for i in range(len(tw.edges)):
        m = min(int(counts[i]), small)
        assert cut[i, :m].tobytes() == cover[i, :m].tobytes()
        assert cut[i, m:].tobytes() == np.full(small - m, sentinel, dtype=COVER_DTYPE).tobytes()


def test_wrapper_form_gives_the_list_form_records(torch_cuda):
    """Check 4: the same edges handed over as curves give byte-identical cover records and summaries; one curve that starts 1.5
    steps late has count 0 and the summary of the last cover alone, at the vertex's own pose."""
    import oracle as orc
    from parity import REL_TOL
    from path_planner_amd.types import WRAPPER_EDGE_DTYPE, CS_LAST_COVER, F_INFEASIBLE
    tw, _, (res, counts, cover, summ, final) = device_run("cfg3")
    we = np.zeros(len(tw.edges) + 1, dtype=WRAPPER_EDGE_DTYPE)
    for i in range(len(tw.edges)):
        p8, start, speed, vi = _edge_curve(tw, tw.edges[i], res[i])
        end = orc.O.ppo_wrapper_fill_end_time(p8.ctypes.data, speed, start)
        we[i] = (vi, 1 if p8[6] == tw.cfg.coverage_turning_radius else 0, p8[0:3], p8[3:6], p8[6], int(p8[7]), 0, speed, start, end)
    late = int(np.argmax(summ["changes"]))
    we[-1] = we[late]
    # (the vertex's first step comes less than one interval after its own time, Edge.cpp:116-120: this start lies after it)
    we[-1]["start_time"] += 1.5 * tw.cfg.collision_checking_increment / tw.cfg.max_speed
    wres, wcounts, wcover, wsumm, wfinal = tw.context().trace_cover_wrapper_edges(we, STRIDE, ribbon_stride=RIBBONS)
    assert np.array_equal(wcounts[:-1], counts)
    assert wsumm[:-1].tobytes() == summ.tobytes() and wfinal[:-1].tobytes() == final.tobytes()
    for i in range(len(tw.edges)):
        assert wcover[i, :counts[i]].tobytes() == cover[i, :counts[i]].tobytes(), i
    assert wcounts[-1] == 0 and (wres["flags"][-1] & F_INFEASIBLE) and (wres["info"][-1] >> 16) == 0
    cov, rib0, cct0, vxy, vi = cr.edge_inputs(tw, tw.edges[late])
    times = reference_times(tw.cfg, float(tw.verts["time"][vi]), 1)
    r = cr.replay_edge(tw.cfg, cov, rib0, cct0, np.zeros(0), np.zeros(0), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool), times, vxy)
    s = wsumm[-1]
    assert (s["events"], s["changes"]) == (0, 0) and (s["flags"] & CS_LAST_COVER) and int(s["flags"]) == r.summary_flags
    assert s["ribbons_final"] == len(r.final) and s["coverage_completed_time"] == r.cct
    assert float(_rel(wfinal[-1, :len(r.final)], r.final).max(initial=0.0)) <= REL_TOL


@pytest.mark.parametrize("budget", [24 << 10, 400 << 10])
def test_sliced_cover_trace_is_bit_identical(torch_cuda, monkeypatch, budget):
    """Check 5: a handle with a small workspace budget runs the walk as slices (24 KB: the costing launch is sliced too and the
    trace solves each slice's curves again; 400 KB: the setup records are re-used, the cover records come home a few edges at a
    time).  The same bytes as in one piece."""
    tw, _, whole = device_run("cfg3")
    monkeypatch.setenv("PPGPU_SLICE_BYTES", str(budget))
    from path_planner_amd.types import COVER_DTYPE
    cover = np.full((len(tw.edges), STRIDE), _sentinel(COVER_DTYPE, 0xA5), dtype=COVER_DTYPE)
    cut = tw.context().trace_cover(tw.edges, STRIDE, cover, ribbon_stride=RIBBONS)
    for a, b in zip(whole, cut):
        assert a.tobytes() == b.tobytes()


def test_large_launch_through_the_prepass_route(torch_cuda, monkeypatch):
    """Check 6: one list of more than 8 192 edges on the cfg3 world with the production setting, device arrays: the records the
    walk starts from came through the chunk-skip planner and the approach prepass.  The whole list passes check 2; a strided subset
    of 40 edges has the cover records, summaries and final lists of a small launch of the same edges, byte for byte."""
    from path_planner_amd.types import RESULT_DTYPE, COVER_DTYPE, COVER_SUMMARY_DTYPE, edge_pack
    torch = torch_cuda
    monkeypatch.delenv("PPGPU_PREPASS_MIN_EDGES", raising=False)
    tw = cr.cover_world("cfg3")
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
    d_cover = torch.full((ne * STRIDE * COVER_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_summ = torch.zeros(ne * COVER_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_final = torch.zeros((ne, RIBBONS, 4), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()      # the fills ran on torch's stream, the library works on its own
    ctx.trace_cover_list(ne, d_e.data_ptr(), d_res.data_ptr(), STRIDE, d_counts.data_ptr(), d_cover.data_ptr(), d_summ.data_ptr(),
                         d_final.data_ptr(), RIBBONS)
    ctx.synchronize()
    res = d_res.cpu().numpy().view(RESULT_DTYPE)
    counts = d_counts.cpu().numpy()
    cover = d_cover.cpu().numpy().view(COVER_DTYPE).reshape(ne, STRIDE)
    summ = d_summ.cpu().numpy().view(COVER_SUMMARY_DTYPE)
    final = d_final.cpu().numpy()
    del d_cover
    want, want_child = ctx.cost_edges_host(edges, stride=RIBBONS)
    check_against_costing(res, want, want_child, counts, summ, final, {})
    valid = np.arange(STRIDE)[None, :] < counts[:, None]
    assert np.all(cover.view(np.uint8).reshape(ne, STRIDE, COVER_DTYPE.itemsize)[~valid] == 0xA5)
    sub = np.arange(0, ne, ne // 40)
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", "1000000000")
    r3, c3, cover3, summ3, final3 = tw.context().trace_cover(edges[sub], STRIDE, ribbon_stride=RIBBONS)
    assert np.array_equal(c3, counts[sub]) and summ3.tobytes() == summ[sub].tobytes() and final3.tobytes() == final[sub].tobytes()
    for j, i in enumerate(sub):
        assert cover3[j, :c3[j]].tobytes() == cover[i, :c3[j]].tobytes()
    print("large launch:", ne, "edges,", int(counts.sum()), "steps,", int(summ["events"].sum()), "events,", int(summ["changes"].sum()), "changes")


def test_bad_arguments_are_refused(torch_cuda):
    """Check 7: stride 0, NULL counts and NULL summaries are refused with the entry point's name; results may be NULL; the
    handle's buffers are counted."""
    from path_planner_amd import api
    from path_planner_amd.types import COVER_DTYPE, COVER_SUMMARY_DTYPE
    tw = cr.cover_world("coverage")
    ctx = tw.context()
    with pytest.raises(api.PpgpuError):
        ctx.trace_cover(tw.edges, 0)
    counts = np.zeros(4, dtype=np.int32)
    cover = np.zeros((4, 8), dtype=COVER_DTYPE)
    summ = np.zeros(4, dtype=COVER_SUMMARY_DTYPE)
    e = tw.edges[:4].copy()
    fn = api.LIB.ppgpu_trace_cover_host
    assert fn(ctx._h, 4, e.ctypes.data, None, 0, counts.ctypes.data, cover.ctypes.data, summ.ctypes.data, None, 0) == -1
    assert b"trace_cover_host" in api.LIB.ppgpu_last_error()
    assert fn(ctx._h, 4, e.ctypes.data, None, 8, None, cover.ctypes.data, summ.ctypes.data, None, 0) == -1
    assert b"trace_cover_host" in api.LIB.ppgpu_last_error()
    assert fn(ctx._h, 4, e.ctypes.data, None, 8, counts.ctypes.data, cover.ctypes.data, None, None, 0) == -1
    assert b"trace_cover_host" in api.LIB.ppgpu_last_error()
    assert fn(ctx._h, 4, e.ctypes.data, None, 8, counts.ctypes.data, cover.ctypes.data, summ.ctypes.data, None, 0) == 0
    assert counts.max() > 8 and summ["events"].min() > 0                # h_results may be NULL; counts are whole
    before = ctx.growth_stats()[0]
    ctx.trace_cover(tw.edges, 4 * STRIDE)                               # a larger record buffer than any call before: the handle grows, and says so
    assert ctx.growth_stats()[0] > before
