"""-m gpu: the host planner's route-by-water report (PlannerConfig::setPlanWaterRoute -> one ppgpu_water_routes_host call on the first
context, Planner::Stats::WaterReport::Routes) through plan_cli, on tests/water_replay.py's detour world: the keys of the JSON line and
the lines of the route file against tests/route_replay.py, and that the report changes nothing else."""
import os
import tempfile

import numpy as np
import pytest

import reach_replay as rr
import route_replay as ro
import water_replay as wr
from test_gpu_plan_reach import _run, _without
from test_gpu_plan_water import KEYS as WATER_KEYS

pytestmark = pytest.mark.gpu

KEYS = ("water_route_metres", "water_route_turns", "water_route_vertices", "water_route_truncated", "water_route_narrowest_metres", "water_route_first_dir")
RTOL = 1e-12
# `water_rounds` says how many relaxation rounds the build of the water map took, which may differ between two builds of one map
# (ppgpu.h, "distance by water"): it is the one key two runs need not share
LOOSE = ("water_rounds",)


def _lines(path):
    """The lines of a plan_water_route_file: ribbon j x y."""
    return [(int(a), int(b), float(x), float(y)) for a, b, x, y in (line.split() for line in open(path).read().splitlines())]


def _check_keys(got, want):
    for k in KEYS:
        if isinstance(want[k], float):
            assert got[k] == pytest.approx(want[k], rel=RTOL, abs=0.0), (k, got[k], want[k])
        else:
            assert got[k] == want[k] and type(got[k]) is type(want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("margin", [0.0, 3.0])
def test_report_through_plan_cli(margin):
    w, init, calls, gap2 = wr.detour_world()
    limit2 = rr.PLAN_MARGINS[margin]
    recs, verts, keys, lines = ro.plan_routes(w, gap2, limit2)
    cfg = [f"cfg keepout_margin {margin!r}"] if margin else []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "route.txt")
        off = _run(w, d, "off", init, calls, cfg + ["cfg plan_water 1", "cfg plan_water_route 0"])
        on = _run(w, d, "on", init, calls, cfg + ["cfg plan_water 1", "cfg plan_water_route 1", "plan_water_route_file " + path])
        alone = _run(w, d, "alone", init, calls, cfg + ["cfg plan_water_route 1"])
        plain = _run(w, d, "plain", init, calls, cfg)
        got = _lines(path)
    print("margin", margin, {k: on[k] for k in KEYS}, "lines", len(got))
    # the report changes nothing: the plan, segment by segment, its cost and every other key
    assert "exception" not in on and on["plan"] == off["plan"] == plain["plan"]
    assert _without(on, KEYS + LOOSE) == _without(off, LOOSE) and [k for k in on if k not in KEYS] == list(off)
    assert on["water_rounds"] >= 1 and off["water_rounds"] >= 1
    # the switch has effect only together with plan_water
    assert _without(alone, ()) == _without(plain, ()) and not any(k in r for r in (off, alone, plain) for k in KEYS)
    assert _without(on, KEYS + WATER_KEYS) == _without(plain, ())
    # the keys and the file against the replay
    _check_keys(on, keys)
    assert [g[:2] for g in got] == [l[:2] for l in lines]
    assert np.allclose([g[2:] for g in got], [l[2:] for l in lines], rtol=RTOL, atol=0.0)
    cols = w.grid.shape[1]
    if margin == 0.0:
        # ribbon 1's route goes round the wall: it crosses row 27 inside the strait, columns 78-82
        cells = [(int(y / w.res), int(x / w.res)) for i, j, x, y in got if i == 1]
        assert cells == [divmod(v, cols) for v in verts[1]] and recs["wd"][1] == 751
        crossing = [c for r, c in ro.expand([r * cols + c for r, c in cells], cols) if r == rr.PLAN_WALL_ROW]
        assert crossing and all(78 <= c <= 82 for c in crossing)
    else:
        # the keys follow the inflated grid: the strait is closed, ribbon 1 has no route, and the routes keep 3 cells off the hazards
        assert not any(i == 1 for i, _, _, _ in got) and ro.flags_of(recs[1]) == ro.WR_DRY
        assert all(r["min_gap2"] >= 9 for r in recs if not ro.flags_of(r) & ro.WR_DRY)
        assert on["water_route_narrowest_metres"] >= 3.0
    assert on["nearest_ribbon_by_water"] == 2 and on["water_route_vertices"] >= 1


def test_evaluate_carries_the_report():
    """PlanEvaluation::water carries the routes of the call: the same for every plan."""
    w, init, calls, gap2 = wr.detour_world()
    _, _, keys, _ = ro.plan_routes(w, gap2, 0)
    row = lambda p: "prev " + " ".join(repr(float(v)) if i != 7 else str(int(v)) for i, v in enumerate(p))
    with tempfile.TemporaryDirectory() as d:
        first = _run(w, d, "first", init, calls)
        plan = np.array(first["plan"], dtype=np.float64).reshape(-1, 11)
        assert len(plan) >= 1
        blocks = ["prev_begin"] + [row(p) for p in plan] + ["prev_end", "prev_begin", row(plan[0]), "prev_end", "evaluate"]
        off = _run(w, d, "ev_off", init, calls, blocks + ["cfg plan_water 1"])["evaluations"]
        on = _run(w, d, "ev_on", init, calls, blocks + ["cfg plan_water 1", "cfg plan_water_route 1"])["evaluations"]
    assert len(on) == 2 and [_without(e, KEYS + LOOSE) for e in on] == [_without(e, LOOSE) for e in off] and not any(k in e for e in off for k in KEYS)
    for e in on:
        _check_keys(e, keys)
