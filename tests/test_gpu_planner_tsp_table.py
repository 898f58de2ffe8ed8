"""-m gpu: PlannerConfig::setDeviceTspTable through plan_cli (`cfg device_tsp_table N`): the heuristic of children whose ribbon list
exceeds the device's enumeration comes from the device's table pass instead of the host's search on the planning thread.  The scenario
is that of test_gpu_host_planner.py::test_children_with_long_ribbon_lists_do_not_abort_the_plan: five parallel ribbons crossed near
their ends in open water, children of up to ten pieces."""
import os
import tempfile

import numpy as np
import pytest

from test_gpu_host_planner import _run_cli, _scenario, _write_map

pytestmark = pytest.mark.gpu

NEW_KEYS = ("table_heuristics", "table_refused")


def _plan(heuristic, table):
    from path_planner_amd import workloads
    w = workloads.by_name("cfg3")
    w.cfg.heuristic = heuristic
    w.grid = np.zeros_like(w.grid)
    w.obst = None
    w.start5 = np.array([float(w.ribbons4[0][0]) + 2.0, float(w.ribbons4[0][1]) - 6.0, 0.0, 2.5, 1.0])
    with tempfile.TemporaryDirectory() as d:
        mp = os.path.join(d, "grid.map")
        _write_map(w.grid, w.res, mp)
        sc = os.path.join(d, "s.txt")
        _scenario(w, sc, mp, 1000.0, 1e-3, 300, 256)
        if table is not None:
            with open(sc, "a") as f:
                f.write(f"cfg device_tsp_table {table}\n")
        host = _run_cli(sc)
    print({k: host[k] for k in host if k != "plan"})
    assert "exception" not in host, host
    return host


def test_point_robot_heuristic_same_plan_without_the_host_search():
    """TspPointRobotNoSplitAllRibbons: at up to ten pieces the host's search is exhaustive and the All variant has no refusals, so the
    table's h is the host's bit for bit — the plan and every statistic but the two counters of who answered (and the wall times) are
    those of the run without the line, whose JSON does not carry the new keys."""
    base = _plan(1, None)
    assert base["host_heuristics"] > 0 and not any(k in base for k in NEW_KEYS)
    on = _plan(1, 16)
    assert on["host_heuristics"] == 0 and on["table_heuristics"] > 0 and on["table_refused"] == 0
    assert on["plan_depth"] >= 1 and len(on["plan"]) >= 1
    for k in base:
        if k in ("host_heuristics", "wall_ms_median", "wall_ms_max"):
            continue
        assert on[k] == base[k], (k, on[k], base[k])
    off = _plan(1, 0)                                       # named but off: the keys are there, nothing was answered by the table
    assert off["table_heuristics"] == 0 and off["table_refused"] == 0 and off["host_heuristics"] == base["host_heuristics"]
    assert off["plan"] == base["plan"]


def test_dubins_heuristic_plans_without_the_host_search():
    """TspDubinsNoSplitAllRibbons: no exception, a plan comes back, every long list was answered on the device.  (The device's Dubins
    lengths come from the device's libm, so h may differ from the host's in its last bits: the plan is not held to the host's here.)"""
    on = _plan(3, 16)
    assert on["plan_depth"] >= 1 and len(on["plan"]) >= 1
    assert on["host_heuristics"] == 0 and on["table_heuristics"] > 0 and on["table_refused"] == 0
