"""-m gpu: the host planner with a keep-out margin (PlannerConfig::setKeepoutMargin -> ppgpu_set_keepout_limit2 on every context,
Planner::Stats::Keepout) through plan_cli on fixed-clock scenarios of tests/test_gpu_host_planner.py's kind.  A margin on the map
as set must plan what no margin plans on the inflated map (tests/keepout_worlds.py: effective), which the oracle plans too; the
clearance report of such a plan counts no step below the same margin; a start inside the band relaxes the margin to the clearance
it has; and evaluatePlans finds the leg of an older plan that enters the band.  tests/test_keepout_abi.py shows on the oracle alone
that the world, the margin and the relaxed start are what these tests need."""
import math
import os
import tempfile

import numpy as np
import pytest

import keepout_worlds as kw
from test_gpu_host_planner import _compare, _run_cli, _scenario, _write_map

pytestmark = pytest.mark.gpu

T0, DT = 1000.0, 1e-3
KEYS = ("keepout_margin", "keepout_limit2", "keepout_certified", "keepout_relaxed")
CLEARANCE_KEYS = ("plan_clearance", "plan_clearance_time", "plan_below_margin_steps")
MARGIN = f"cfg keepout_margin {kw.PLAN_MARGIN!r}"


def _maps(d, w, gap2, limits):
    """{limit2: path of the map inflated at it} (0: the map as set)"""
    out = {}
    for k in limits:
        out[k] = os.path.join(d, "grid%d.map" % k)
        _write_map(kw.effective(w.grid, k, gap2), w.res, out[k])
    return out


def _run(w, d, name, map_path, init, calls, extra=(), start=None):
    sc = os.path.join(d, name + ".txt")
    _scenario(w, sc, map_path, T0, DT, calls, init, start=start)
    with open(sc, "a") as f:
        f.write("".join(line + "\n" for line in extra))
    return _run_cli(sc)


def _stats(r):
    return {k: v for k, v in r.items() if not k.startswith("wall_ms") and k not in KEYS and k not in CLEARANCE_KEYS}


def _oracle(w, grid, init, calls, start=None):
    import oracle as orc
    orc.O.ppo_set_ribbon_width(w.cfg.ribbon_width)
    world = orc.World(w.cfg, grid, w.res, w.obst)
    rc, st, plan, _, _ = world.plan(w.ribbons4, w.start5 if start is None else start, calls * DT, T0, DT, initial_samples=init)
    assert rc == 0
    return st, plan


def test_margin_plans_what_the_inflated_map_plans(prepass_route):
    w, init, calls, gap2 = kw.plan_world()
    with tempfile.TemporaryDirectory() as d:
        maps = _maps(d, w, gap2, (0, kw.PLAN_LIMIT2))
        plain = _run(w, d, "plain", maps[0], init, calls)
        margin = _run(w, d, "margin", maps[0], init, calls, [MARGIN])
        inflated = _run(w, d, "inflated", maps[kw.PLAN_LIMIT2], init, calls)
        off = _run(w, d, "off", maps[0], init, calls, ["cfg keepout_margin 0"])
    print("margin:", {k: margin[k] for k in margin if k != "plan"})
    # identical statistics, first-goal iteration and plan, segment by segment
    assert _stats(margin) == _stats(inflated) and margin["plan"] == inflated["plan"]
    assert margin["first_goal_iteration"] == inflated["first_goal_iteration"] >= 0 and len(margin["plan"]) >= 2
    # ... which the oracle plans on the inflated map
    st, plan = _oracle(w, kw.effective(w.grid, kw.PLAN_LIMIT2, gap2), init, calls)
    _compare(margin, st, plan)
    # the keys: only with a margin named, and what Stats::Keepout holds
    assert not any(k in r for r in (plain, inflated, off) for k in KEYS) and [k for k in margin if k not in KEYS] == list(plain)
    assert margin["keepout_margin"] == kw.PLAN_MARGIN and margin["keepout_limit2"] == kw.PLAN_LIMIT2
    assert margin["keepout_certified"] == w.res * math.sqrt(float(kw.PLAN_LIMIT2)) and margin["keepout_relaxed"] is False
    # the margin decided something; with it off the run is the plain one
    assert margin["plan"] != plain["plan"] and _stats(off) == _stats(plain) and off["plan"] == plain["plan"]


def test_clearance_report_counts_no_step_below_the_planned_margin():
    w, init, calls, gap2 = kw.plan_world()
    report = ["cfg plan_clearance 1", f"cfg plan_clearance_margin {kw.PLAN_MARGIN!r}"]
    with tempfile.TemporaryDirectory() as d:
        maps = _maps(d, w, gap2, (0,))
        margin = _run(w, d, "margin", maps[0], init, calls, [MARGIN])
        both = _run(w, d, "both", maps[0], init, calls, [MARGIN] + report)
        plain = _run(w, d, "plain", maps[0], init, calls, report)
    print("clearance of the plan with a margin:", [both[k] for k in CLEARANCE_KEYS], "without:", [plain[k] for k in CLEARANCE_KEYS])
    assert _stats(both) == _stats(margin) and both["plan"] == margin["plan"] and [both[k] for k in KEYS] == [margin[k] for k in KEYS]
    assert both["plan_below_margin_steps"] == 0 and both["plan_clearance"] >= both["keepout_certified"] == kw.PLAN_MARGIN
    # the plan made without the margin comes closer than that: the report would have said so
    assert plain["plan_below_margin_steps"] > 0 and plain["plan_clearance"] < kw.PLAN_MARGIN


def test_a_start_inside_the_band_relaxes_the_margin():
    w, init, calls, gap2 = kw.plan_world()
    start = kw.relaxed_start(w)
    with tempfile.TemporaryDirectory() as d:
        maps = _maps(d, w, gap2, (0, kw.RELAXED_GAP2, kw.PLAN_LIMIT2))
        relaxed = _run(w, d, "relaxed", maps[0], init, calls, [MARGIN], start=start)
        inflated = _run(w, d, "inflated", maps[kw.RELAXED_GAP2], init, calls, start=start)
        hard = _run(w, d, "hard", maps[kw.PLAN_LIMIT2], init, calls, start=start)
        # the next call from the default start, outside the band, in the same world: the whole margin again
        whole = _run(w, d, "whole", maps[0], init, calls, [MARGIN])
    print("relaxed:", {k: relaxed[k] for k in relaxed if k != "plan"})
    assert relaxed["keepout_relaxed"] is True and relaxed["keepout_limit2"] == kw.RELAXED_GAP2 == int(gap2[kw.RELAXED_RC])
    assert relaxed["keepout_margin"] == kw.PLAN_MARGIN and relaxed["keepout_certified"] == w.res * math.sqrt(float(kw.RELAXED_GAP2))
    assert _stats(relaxed) == _stats(inflated) and relaxed["plan"] == inflated["plan"] and len(relaxed["plan"]) >= 1
    assert relaxed["first_goal_iteration"] >= 0
    st, plan = _oracle(w, kw.effective(w.grid, kw.RELAXED_GAP2, gap2), init, calls, start=start)
    _compare(relaxed, st, plan)
    assert len(hard["plan"]) == 0 and hard["first_goal_iteration"] < 0          # what the hard limit would have left the vehicle with
    assert whole["keepout_relaxed"] is False and whole["keepout_limit2"] == kw.PLAN_LIMIT2


def test_evaluate_stops_at_the_leg_that_enters_the_band():
    w, init, calls, gap2 = kw.plan_world()
    row = lambda p: "prev " + " ".join(repr(float(v)) if i != 7 else str(int(v)) for i, v in enumerate(p))
    with tempfile.TemporaryDirectory() as d:
        maps = _maps(d, w, gap2, (0, kw.PLAN_LIMIT2))
        first = _run(w, d, "first", maps[0], init, calls)
        plan = np.array(first["plan"], dtype=np.float64).reshape(-1, 11)
        assert len(plan) >= 2
        blocks = ["prev_begin"] + [row(p) for p in plan] + ["prev_end", "prev_begin", row(plan[0]), "prev_end", "evaluate"]
        plain = _run(w, d, "ev_plain", maps[0], init, calls, blocks)["evaluations"]
        margin = _run(w, d, "ev_margin", maps[0], init, calls, blocks + [MARGIN])["evaluations"]
        inflated = _run(w, d, "ev_inflated", maps[kw.PLAN_LIMIT2], init, calls, blocks)["evaluations"]
    print("evaluate under the margin:", [{k: e[k] for k in ("legs_costed", "stop") + KEYS} for e in margin])
    assert len(margin) == 2 and [{k: v for k, v in e.items() if k not in KEYS} for e in margin] == inflated
    assert not any(k in e for e in plain + inflated for k in KEYS)
    for e in margin:
        assert [e[k] for k in KEYS] == [kw.PLAN_MARGIN, kw.PLAN_LIMIT2, w.res * math.sqrt(float(kw.PLAN_LIMIT2)), False]
    # without the margin the whole plan is feasible; under it the first leg is, and the walk stops at the second, which enters the band
    assert plain[0]["legs_costed"] == len(plan) and all(leg["feasible"] for leg in plain[0]["legs"]) and plain[0]["stop"] != "infeasible"
    assert margin[0]["stop"] == "infeasible" and margin[0]["legs_costed"] == 2
    assert [leg["feasible"] for leg in margin[0]["legs"]] == [True, False]
    assert margin[1]["legs_costed"] == 1 and margin[1]["legs"][0]["feasible"] and margin[1]["stop"] == "ran_out_of_legs"
