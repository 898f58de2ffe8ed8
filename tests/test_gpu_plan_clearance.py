"""-m gpu: the host planner's clearance reports (PlannerConfig::setPlanClearance -> Planner::Stats::Clearance / PlanClearance,
GpuAStarPlanner::PlanEvaluation::clearance) through plan_cli on a fixed-clock scenario of tests/test_gpu_host_planner.py's kind,
against the recipe of tests/clearance_replay.py run on the poses the same run's plan trace wrote."""
import copy
import os
import tempfile

import numpy as np
import pytest

from test_gpu_host_planner import _run_cli, _scenario, _write_map
from test_gpu_plan_contacts import _steps_of

pytestmark = pytest.mark.gpu

T0, DT, CALLS, INIT = 1000.0, 1e-3, 40, 256
KEYS = ("plan_clearance", "plan_clearance_time", "plan_below_margin_steps")
WIDE_MARGIN = 40.0        # metres: wider than any plan of this world keeps clear (and within 255 cells of 0.2 m)


def _world():
    """Config 2 (10 % of a 1024 x 1024 chart blocked, the middle kept free) with an island of 5 x 5 cells three metres north of
    the first survey line: whatever covers that line passes it."""
    from path_planner_amd import workloads
    w = copy.copy(workloads.by_name("cfg2"))
    w.grid = w.grid.copy()
    c = float(w.start5[0])
    r, col = int((c + 13.0) / w.res), int((c + 5.0) / w.res)
    w.grid[r:r + 5, col:col + 5] = 1
    w.obst = None
    return w


def _run(w, d, name, extra):
    sc = os.path.join(d, name + ".txt")
    _scenario(w, sc, os.path.join(d, "grid.map"), T0, DT, CALLS, INIT)
    with open(sc, "a") as f:
        f.write("".join(line + "\n" for line in extra))
    return _run_cli(sc)


def _stats(r):
    return {k: v for k, v in r.items() if not k.startswith("wall_ms") and not k.startswith("plan_trace_") and k not in KEYS}


def _file_records(rows):
    """plan_clearance_file rows (segment clearance time x y step gap2 below_steps first_below_time flags) as records[segment]."""
    from path_planner_amd.types import CLEARANCE_DTYPE
    out = np.zeros(len(rows), dtype=CLEARANCE_DTYPE)
    assert list(rows[:, 0]) == list(range(len(rows)))
    for f, k in (("clearance", 1), ("time", 2), ("x", 3), ("y", 4), ("step", 5), ("gap2", 6), ("below_steps", 7), ("first_below_time", 8), ("flags", 9)):
        out[f] = rows[:, k]
    out["first_below_step"] = np.where(out["below_steps"] > 0, 0, -1)       # (the file has no such column: merge() only asks whether there is one)
    return out


def _check_run(on, trace, crow, w, gap2, margin):
    """The clearance file of a run equals the recipe on its trace file, segment by segment; the JSON keys are the merge."""
    import clearance_replay as clr
    plan = on["plan"]
    got = _file_records(crow)
    assert len(got) == len(plan) >= 2
    for s in range(len(plan)):
        want = clr.replay(w.grid, w.res, _steps_of(trace[trace[:, 0] == s]), margin, gap2)
        for f in ("time", "x", "y", "step", "gap2", "below_steps", "first_below_time", "flags"):
            assert got[s][f] == want[f], (margin, s, f, got[s][f], want[f])
        assert abs(got[s]["clearance"] - want["clearance"]) <= np.spacing(abs(want["clearance"])), (margin, s)
    merged, seg = clr.merge(got)
    assert (on["plan_clearance"], on["plan_clearance_time"], on["plan_below_margin_steps"]) == (merged["clearance"], merged["time"], merged["below_steps"])
    return got, merged


def test_plan_clearance_equals_the_recipe_on_the_plan_trace():
    """cfg plan_trace 1 + cfg plan_clearance 1.  Three runs of the same binary: the switch off, on with a margin wider than the plan
    keeps, on with half the clearance the plan has: the same plan and statistics, the same keys but the three new ones."""
    import clearance_replay as clr
    w = _world()
    gap2 = clr.gap2_numpy(w.grid)
    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        tf, cf = os.path.join(d, "trace.txt"), os.path.join(d, "clearance.txt")
        off = _run(w, d, "off", ["cfg plan_trace 1", "cfg plan_clearance 0", f"cfg plan_clearance_margin {WIDE_MARGIN}", f"plan_clearance_file {cf}"])
        assert not os.path.exists(cf)
        on = _run(w, d, "on", ["cfg plan_trace 1", f"plan_trace_file {tf}", "cfg plan_clearance 1", f"cfg plan_clearance_margin {WIDE_MARGIN}",
                               f"plan_clearance_file {cf}"])
        trace, crow = np.loadtxt(tf, ndmin=2), np.loadtxt(cf, ndmin=2)
        assert not any(k in off for k in KEYS) and [k for k in on if k not in KEYS] == list(off)
        assert _stats(on) == _stats(off) and on["plan"] == off["plan"]
        assert on["plan_trace_segments"] == off["plan_trace_segments"] and on["plan_trace_steps"] == off["plan_trace_steps"]
        got, merged = _check_run(on, trace, crow, w, gap2, WIDE_MARGIN)
        # a margin wider than the plan's clearance: steps are counted, as many as the recipe counts
        assert 0 < on["plan_clearance"] < WIDE_MARGIN and on["plan_below_margin_steps"] == int(got["below_steps"].sum()) > 0
        small = 0.5 * on["plan_clearance"]
        os.remove(tf); os.remove(cf)
        on2 = _run(w, d, "on2", ["cfg plan_trace 1", f"plan_trace_file {tf}", "cfg plan_clearance 1", f"cfg plan_clearance_margin {small!r}",
                                 f"plan_clearance_file {cf}"])
        trace2, crow2 = np.loadtxt(tf, ndmin=2), np.loadtxt(cf, ndmin=2)
    assert on2["plan"] == on["plan"] and np.array_equal(trace2, trace)
    _check_run(on2, trace2, crow2, w, gap2, small)
    assert on2["plan_below_margin_steps"] == 0 and on2["plan_clearance"] == on["plan_clearance"] and on2["plan_clearance_time"] == on["plan_clearance_time"]
    print("plan clearance:", len(on["plan"]), "segments,", [on[k] for k in KEYS], "per segment", got["clearance"].tolist())


def test_evaluate_reports_the_clearance_of_every_plan():
    """plan_cli evaluate on two prev_begin blocks (the plan a first cycle returned, and its first leg alone) with the switch on: per
    plan the three keys, those of the plan() run for the whole plan and of its first segment for the first leg; with the switch off
    the line is what it was."""
    import clearance_replay as clr
    w = _world()
    row = lambda p: "prev " + " ".join(repr(float(v)) if i != 7 else str(int(v)) for i, v in enumerate(p))
    opts = ["cfg plan_clearance 1", "cfg plan_clearance_margin 2.5"]
    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        cf = os.path.join(d, "clearance.txt")
        first = _run(w, d, "first", opts + [f"plan_clearance_file {cf}"])
        segs = _file_records(np.loadtxt(cf, ndmin=2))
        plan = np.array(first["plan"], dtype=np.float64).reshape(-1, 11)
        assert len(plan) >= 2
        blocks = ["prev_begin"] + [row(p) for p in plan] + ["prev_end", "prev_begin", row(plan[0]), "prev_end", "evaluate"]
        off = _run(w, d, "ev_off", blocks)["evaluations"]
        on = _run(w, d, "ev_on", blocks + opts)["evaluations"]
    assert len(on) == 2 and [{k: v for k, v in e.items() if k not in KEYS} for e in on] == off
    assert not any(k in e for e in off for k in KEYS)
    assert [on[0]["legs_costed"], on[1]["legs_costed"]] == [len(plan), 1]
    assert [on[0][k] for k in KEYS] == [first[k] for k in KEYS]
    m, _ = clr.merge(segs[:1])
    assert [on[1][k] for k in KEYS] == [m["clearance"], m["time"], m["below_steps"]]
    print("evaluate:", [[e[k] for k in KEYS] for e in on])


def test_an_empty_plan_reports_no_clearance():
    """evaluate on a plan that has already ended at the start time: no leg is walked, the keys are -1 / -1 / 0."""
    w = _world()
    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        c = float(w.start5[0])
        past = f"prev {c!r} {c!r} 0.0 1.0 1.0 1.0 8.0 0 2.5 0.0 0.5"       # ends before the start's time
        ev = _run(w, d, "ev_empty", ["prev_begin", past, "prev_end", "evaluate", "cfg plan_clearance 1"])["evaluations"]
    assert len(ev) == 1 and ev[0]["legs_costed"] == 0
    assert [ev[0][k] for k in KEYS] == [-1.0, -1.0, 0]
