"""-m gpu: the host planner's two users of the device's edge traces, through plan_cli on fixed-clock scenarios of
tests/test_gpu_host_planner.py's kind: PlannerConfig::setPlanTrace (the returned plan step by step) and
PlannerConfig::setDeviceTrajectories (the search dump's "Trajectory:" lines from the device's own sweep)."""
import math
import os
import tempfile

import numpy as np
import pytest

from test_gpu_host_planner import _read_search_dump, _run_cli, _scenario, _write_map

pytestmark = pytest.mark.gpu

T0, DT, CALLS, INIT = 1000.0, 1e-3, 24, 256


def _stats(r):
    return {k: v for k, v in r.items() if not k.startswith("wall_ms") and not k.startswith("plan_trace_")}


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1.0)


def _angdiff(a, b):
    d = abs(a - b) % (2 * math.pi)
    return min(d, 2 * math.pi - d)


def _pose(seg, t):
    """The oracle's DubinsWrapper::sample of plan segment {qi[3], param[3], rho, type, speed, start, end} at time t."""
    import oracle as orc
    p8 = np.array(list(seg[:7]) + [float(seg[7])])
    err, q = orc.dubins_sample(p8, (t - seg[9]) * seg[8])
    assert err == 0
    h = math.pi / 2 - q[2]
    return q[0], q[1], h + 2 * math.pi if h < 0 else h


def test_plan_trace_follows_the_returned_plan():
    """cfg plan_trace 1: statistics unchanged; one traced segment per plan segment; step times strictly increasing; every step
    on its segment's curve; segment s+1 picks up where segment s ended; the penalties the steps accrued are the plan's.

    Where segment s+1 picks up: its first step is sampled at the vertex's time moved on to the next multiple of the
    collision-check interval since the start state (Edge.cpp:116-120), up to 0.02 s = 5 cm after the end state of segment s, so
    the two are compared through the curve: segment s+1's curve starts at segment s's end state, the first step lies less than
    one interval later, and its pose is that curve's pose at its time — each within parity.REL_TOL."""
    from path_planner_amd import workloads
    from parity import REL_TOL
    w = workloads.by_name("cfg3")
    inc_t = w.cfg.collision_checking_increment / w.cfg.max_speed
    with tempfile.TemporaryDirectory() as d:
        mp = os.path.join(d, "grid.map")
        _write_map(w.grid, w.res, mp)
        sc = os.path.join(d, "s.txt")
        _scenario(w, sc, mp, T0, DT, CALLS, INIT)
        plain = _run_cli(sc)
        tf = os.path.join(d, "trace.txt")
        with open(sc, "a") as f:
            f.write(f"cfg plan_trace 1\nplan_trace_file {tf}\n")
        traced = _run_cli(sc)
        rows = np.loadtxt(tf, ndmin=2)
    assert "plan_trace_segments" not in plain
    assert _stats(plain) == _stats(traced)
    plan = traced["plan"]
    assert len(plan) >= 2 and traced["plan_trace_segments"] == len(plan) and traced["plan_trace_steps"] == len(rows)
    seg_of = rows[:, 0].astype(int)
    assert sorted(set(seg_of.tolist())) == list(range(len(plan)))
    total_penalty = 0.0
    for s, seg in enumerate(plan):
        r = rows[seg_of == s]
        assert np.array_equal(r[:, 1], np.arange(len(r))) and len(r) > 0
        t = r[:, 5]
        assert np.all(np.diff(t) > 0)
        assert t[-1] < seg[10] <= t[-1] + 2 * inc_t                        # the sweep ran to the segment's end
        for k in range(0, len(r), 7):
            x, y, h = _pose(seg, t[k])
            assert _rel(r[k, 2], x) <= REL_TOL and _rel(r[k, 3], y) <= REL_TOL and _angdiff(r[k, 4], h) <= REL_TOL
        assert r[0, 7] == 0.0 and np.all(np.diff(r[:, 7]) >= 0)
        total_penalty += r[-1, 7] + r[-1, 6] * 600.0
        assert not (r[:, 8].astype(int) & 1).any()                          # a plan never runs over a blocked cell
        if s + 1 < len(plan):
            nxt = plan[s + 1]
            ex, ey, eh = _pose(seg, seg[10])
            sx, sy, sh = _pose(nxt, max(nxt[9], seg[10]))
            assert _rel(ex, sx) <= REL_TOL and _rel(ey, sy) <= REL_TOL and _angdiff(eh, sh) <= REL_TOL
            first = rows[seg_of == s + 1][0]
            assert 0 <= first[5] - seg[10] < inc_t * (1 + 1e-9)
    assert _rel(total_penalty, traced["plan_collision_penalty"]) <= REL_TOL


def _blocks(items):
    out = []
    for it in items:
        if it["tag"] == "trajectory-start":
            out.append([])
        elif it["tag"] == "trajectory":
            out[-1].append(it)
    return out


def test_device_trajectories_write_the_dump_the_host_loop_writes():
    """visualization_file + cfg device_trajectories 1: the same search, a dump that parses the way the viewer reads it, with as
    many "Trajectory:" blocks, as many lines in each and every number within parity.REL_TOL of the host-rebuilt dump of the same
    fixed-clock run.  With both switches spelled out as 0 the dump and the statistics are byte for byte those of a scenario
    that does not mention them."""
    from path_planner_amd import workloads
    from parity import REL_TOL
    w = workloads.by_name("cfg3")
    with tempfile.TemporaryDirectory() as d:
        mp = os.path.join(d, "grid.map")
        _write_map(w.grid, w.res, mp)
        runs = {}
        for name, extra in (("host", ""), ("device", "cfg device_trajectories 1\n"), ("off", "cfg device_trajectories 0\ncfg plan_trace 0\n")):
            sc = os.path.join(d, name + ".txt")
            _scenario(w, sc, mp, T0, DT, CALLS, INIT)
            dump = os.path.join(d, name + ".dump")
            with open(sc, "a") as f:
                f.write(f"visualization_file {dump}\n" + extra)
            res = _run_cli(sc)
            runs[name] = (res, open(dump, "rb").read(), _read_search_dump(dump))
    assert runs["off"][1] == runs["host"][1] and _stats(runs["off"][0]) == _stats(runs["host"][0])
    assert list(runs["off"][0]) == list(runs["host"][0])                  # the same keys in the same order
    assert _stats(runs["device"][0]) == _stats(runs["host"][0])
    hi, di = runs["host"][2][0], runs["device"][2][0]
    assert [i["tag"] for i in hi] == [i["tag"] for i in di] and runs["host"][2][1] == runs["device"][2][1]
    hb, db = _blocks(hi), _blocks(di)
    assert len(hb) == len(db) and len(hb) > 100
    assert [len(b) for b in hb] == [len(b) for b in db]
    worst, lines = 0.0, 0
    for a, b in zip(hi, di):
        for k in ("x", "y", "speed", "time", "f", "g", "h"):
            if k in a:
                worst = max(worst, _rel(a[k], b[k]))
        if "heading" in a:
            worst = max(worst, _angdiff(a["heading"], b["heading"]))
            assert a["ids"] == b["ids"] and a["kind"] == b["kind"]
        lines += a["tag"] == "trajectory"
    print("trajectory blocks", len(hb), "lines", lines, "worst deviation", worst)
    assert lines > 1000 and worst <= REL_TOL
