"""-m gpu: PlannerConfig::setPlanCoverage through plan_cli on the fixed-clock scenario of tests/test_gpu_plan_trace.py: what every
step of the returned plan did to the ribbons (Planner::Stats::Coverage), next to the plan's step trace."""
import math
import os
import tempfile

import numpy as np

import cover_replay as cr
from test_gpu_host_planner import _run_cli, _scenario, _write_map
from test_gpu_plan_trace import CALLS, DT, INIT, T0, _stats
import pytest

pytestmark = pytest.mark.gpu

# `remaining` is recomputed only when the list changed.  A trim or an erasure shortens it; a split replaces one length by those of
# its two halves, whose sum is the same up to the rounding of three square roots of numbers below 1e3 m (a few 1e-13 m).
SPLIT_SLACK = 1e-9


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)


def test_plan_coverage_follows_the_returned_plan():
    """cfg plan_trace 1 + cfg plan_coverage 1: the coverage file has exactly the trace file's (segment, step) pairs and times;
    `remaining` never increases along the plan, segment s + 1 starting from no more than segment s left; every line equals the
    replay of tests/cover_replay.py on the trace file's poses, segment s + 1 from the list the replay of segment s left (the rule
    of tests/test_gpu_cover_trace.py's check 1).  With plan_coverage 0 the JSON line and the plan are what they are without it."""
    from path_planner_amd import workloads
    from parity import REL_TOL
    w = workloads.by_name("cfg3")
    # The vehicle starts ON the second survey line, 1 m from its start point, heading along it (the map is free around this stretch
    # of the line).  Step 0 of the plan's first segment is then a coverage event at the start pose itself (toCoverDistance starts at
    # 0, the time nudge of a start state is 0, the heading is the vertex's own): cover() splits the line there and the 1 m front
    # piece, shorter than the ribbon width, is erased — whatever plan the search returns, it covers at least that metre.
    line = w.ribbons4[1]
    start = [float(line[0]) + 1.0, float(line[1]), math.pi / 2, 2.5, 1.0]
    total = float(np.hypot(w.ribbons4[:, 2] - w.ribbons4[:, 0], w.ribbons4[:, 3] - w.ribbons4[:, 1]).sum())
    with tempfile.TemporaryDirectory() as d:
        mp = os.path.join(d, "grid.map")
        _write_map(w.grid, w.res, mp)
        sc = os.path.join(d, "s.txt")
        _scenario(w, sc, mp, T0, DT, CALLS, INIT, start=start)
        plain = _run_cli(sc)
        off = os.path.join(d, "off.txt")
        with open(off, "w") as f:
            f.write(open(sc).read() + "cfg plan_coverage 0\n")
        unchanged = _run_cli(off)
        tf, cf = os.path.join(d, "trace.txt"), os.path.join(d, "coverage.txt")
        with open(sc, "a") as f:
            f.write(f"cfg plan_trace 1\nplan_trace_file {tf}\ncfg plan_coverage 1\nplan_coverage_file {cf}\n")
        both = _run_cli(sc)
        trace = np.loadtxt(tf, ndmin=2)
        cover = np.loadtxt(cf, ndmin=2)
    assert list(unchanged) == list(plain) and _stats(unchanged) == _stats(plain) and "plan_coverage_steps" not in plain
    strip = lambda r: {k: v for k, v in _stats(r).items() if k != "plan_coverage_steps"}       # noqa: E731
    assert strip(both) == _stats(plain)
    plan = both["plan"]
    assert len(plan) >= 2 and both["plan_coverage_steps"] == len(cover) == len(trace) == both["plan_trace_steps"]
    assert np.array_equal(cover[:, :2], trace[:, :2]) and np.array_equal(cover[:, 2], trace[:, 5])
    remaining = cover[:, 4]
    assert np.all(np.diff(remaining) <= SPLIT_SLACK), float(np.diff(remaining).max())
    assert remaining[0] <= total - 1.0 + SPLIT_SLACK and remaining[-1] <= remaining[0]     # the plan covers something
    seg_of = cover[:, 0].astype(int)
    rib, cct = np.asarray(w.ribbons4, dtype=np.float64).reshape(-1, 4), -1.0
    vxy = (start[0], start[1])
    inc_t = w.cfg.collision_checking_increment / w.cfg.max_speed
    worst = 0.0
    for s, seg in enumerate(plan):
        t, c = trace[seg_of == s], cover[seg_of == s]
        n = len(t)
        flags = t[:, 8].astype(int)
        xs, ys, straight, blocked = t[:, 2], t[:, 3], (flags & 2) != 0, (flags & 1) != 0
        times = np.concatenate([t[:, 5], [t[-1, 5] + inc_t]])
        cov = seg[6] == w.cfg.coverage_turning_radius
        r = cr.replay_edge(w.cfg, cov, rib, cct, xs, ys, straight, blocked, times, vxy)
        rel = np.maximum(_rel(c[:, 3], r.to_cover), _rel(c[:, 4], r.remaining))
        bad = (c[:, 6].astype(np.uint32) != r.flags) | (c[:, 5].astype(np.uint32) != r.ribbons) | (rel > REL_TOL)
        print("segment", s, "steps", n, "events", r.events, "changes", r.changes, "ribbons left", len(r.final), "worst", float(rel.max()))
        if bad.any():
            k = int(np.argmax(bad))
            knife = cr.knife_edge(w.cfg, cov, rib, cct, xs, ys, straight, blocked, times, vxy, k)
            # (a plan has fewer than 20 segments: by check 1's rule none of them may leave the replay, knife edge or not)
            raise AssertionError(("segment", s, "step", k, "knife edge", knife, c[k], r.to_cover[k], r.remaining[k], r.flags[k], r.ribbons[k]))
        worst = max(worst, float(rel.max()))
        if s + 1 < len(plan):
            first = cover[seg_of == s + 1][0]
            assert first[4] <= c[-1, 4] + SPLIT_SLACK
            assert _rel(first[4], r.remaining_final) <= REL_TOL or first[4] <= r.remaining_final
        rib, cct, vxy = r.final, r.cct, (float(xs[-1]), float(ys[-1]))
    print("plan coverage: segments", len(plan), "steps", len(cover), "worst deviation", worst, "remaining", remaining[0], "->", remaining[-1])
