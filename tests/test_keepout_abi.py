"""The keep-out entry points exist at every layer that needs no GPU (declared in include/ppgpu.h, exported by libppgpu.so, bound in
path_planner_amd.api), ppgpu_keepout_limit2, which takes no handle, states the rule of tests/clearance_replay.py's limit2, and the
planning world of tests/test_gpu_keepout_plan.py is what that test needs, shown on the oracle alone."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clearance_replay as clr
import keepout_worlds as kw
from test_contact_trace_abi import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ppgpu_keepout_limit2", "ppgpu_set_keepout_limit2", "ppgpu_get_keepout_limit2", "ppgpu_get_grid_blocked", "ppgpu_last_keepout_timing"]
METHODS = ["set_keepout_limit2", "get_keepout_limit2", "get_grid_blocked", "last_keepout_timing"]
PPGPU_EINVAL = -1


def test_header_declares_the_entry_points_under_chart_clearance():
    txt = _header()
    full = open(os.path.join(ROOT, "include", "ppgpu.h")).read()
    section = full[full.index("chart clearance"):]
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, txt, flags=re.M), name
        assert name in section, name
    assert re.search(r"^int\s+ppgpu_keepout_limit2\s*\(\s*double\s+\w+,\s*double\s+\w+,\s*uint32_t\s*\*", txt, flags=re.M)
    for name in SYMBOLS[1:]:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name


def test_library_exports_and_binding_has_them():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert getattr(api.LIB, name).restype is C.c_int
    for method in METHODS:
        assert callable(getattr(api.Context, method)), method
    assert callable(api.keepout_limit2)


def _limit2(res, margin):
    """(return code, limit2) of the C entry point itself: no handle, no device."""
    from path_planner_amd import api
    out = C.c_uint32(0xA5A5A5A5)
    rc = api.LIB.ppgpu_keepout_limit2(float(res), float(margin), C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("res", [1.0, 0.25, 1.0 / 3.0, 0.3, 0.07, 0.05])
def test_limit2_is_the_rule_of_the_replay(res):
    from path_planner_amd import api
    assert _limit2(res, 0.0) == (0, 0) and _limit2(res, -1.0) == (0, 0) and _limit2(res, -math.inf) == (0, 0)
    assert _limit2(res, 1e-300) == (0, 1) == (0, clr.limit2(res, 1e-300))
    for k in (1, 2, 3, 4, 5, 8, 9, 10, 17, 100, 101, 4096, 65024, 65025):
        m = res * math.sqrt(float(k))
        assert _limit2(res, m) == (0, clr.limit2(res, m)), (res, k)
        assert _limit2(res, m)[1] <= k                                  # a margin of exactly res * sqrt(k): gap2 == k is not below
        if k < clr.DIST_CAP2:
            up = float(np.nextafter(m, np.inf))                         # one ulp above: it is
            assert _limit2(res, up) == (0, clr.limit2(res, up)) and _limit2(res, up)[1] > k, (res, k)
        down = float(np.nextafter(m, -np.inf))
        assert _limit2(res, down) == (0, clr.limit2(res, down)), (res, k)
    assert _limit2(res, clr.DIST_CAP * res) == (0, clr.limit2(res, clr.DIST_CAP * res))
    assert api.keepout_limit2(res, 2.5 * res) == clr.limit2(res, 2.5 * res) == 7
    # refused: above 255 cells, and a NaN
    rc, out = _limit2(res, clr.DIST_CAP * res * (1 + 1e-9))
    assert rc == PPGPU_EINVAL and b"255 cells" in api.LIB.ppgpu_last_error()
    assert _limit2(res, 256 * res)[0] == PPGPU_EINVAL and _limit2(res, math.inf)[0] == PPGPU_EINVAL
    assert _limit2(res, math.nan)[0] == PPGPU_EINVAL
    with pytest.raises(api.PpgpuError):
        api.keepout_limit2(res, math.nan)
    assert api.LIB.ppgpu_keepout_limit2(res, 1.0, None) == PPGPU_EINVAL


def test_effective_grid_definition():
    """limit2 0: the grid as set; limit2 >= 1 contains the blocked cells, their eight neighbours and the border; every free cell of
    the effective grid has gap2 >= limit2; the grids grow with the limit."""
    for make in list(kw.EXTRA_GRIDS.values()):
        g = make()
        g2 = clr.gap2_numpy(g)
        assert np.array_equal(g2, clr.gap2_brute(g))
        assert np.array_equal(kw.effective(g, 0, g2), (g != 0).astype(np.uint8))
        last = kw.effective(g, 0, g2)
        for k in kw.LIMITS[1:]:
            e = kw.effective(g, k, g2)
            assert np.all(e >= last) and np.all(g2[e == 0] >= k) and np.all(e[g2 == 0] == 1)
            last = e
        assert last.all()                                              # nothing of these grids is 255 cells from a hazard
    assert kw.strip300().shape[1] > 256 and kw.strip300().shape[1] % 32 != 0 and kw.block64().shape[1] == 64


# ------------------------------------------------------------------------------------------------------------ the planning world
def _oracle_plan(w, grid, init, calls, start=None):
    import oracle as orc
    orc.O.ppo_set_ribbon_width(w.cfg.ribbon_width)
    world = orc.World(w.cfg, grid, w.res, w.obst)
    rc, st, plan, _, _ = world.plan(w.ribbons4, w.start5 if start is None else start, calls * 1e-3, 1000.0, 1e-3, initial_samples=init)
    assert rc == 0
    return st, plan


def _leg_gap2(w, gap2, seg):
    """The smallest gap2 over poses every 5 cm along a plan segment {qi[3], param[3], rho, type, speed, start, end}."""
    import oracle as orc
    out = clr.DIST_CAP2
    for d in np.arange(0.0, (seg[10] - seg[9]) * seg[8], 0.05):
        e, q = orc.dubins_sample(seg[:8], float(d))
        assert e == 0
        out = min(out, int(clr.step_gap2(gap2, w.res, [q[0]], [q[1]])[0]))
    return out


def test_planning_world_on_the_oracle():
    w, init, calls, gap2 = kw.plan_world()
    assert clr.limit2(w.res, kw.PLAN_MARGIN) == kw.PLAN_LIMIT2
    r0, c0 = int(w.start5[1] / w.res), int(w.start5[0] / w.res)
    assert gap2[r0, c0] >= kw.PLAN_LIMIT2                              # the default start lies outside the band: nothing is relaxed
    st0, plan0 = _oracle_plan(w, w.grid, init, calls)
    inflated = kw.effective(w.grid, kw.PLAN_LIMIT2, gap2)
    st1, plan1 = _oracle_plan(w, inflated, init, calls)
    # the inflated map still reaches a goal within the budget, by another plan than the map as set
    assert st0.first_goal_iteration >= 0 and st1.first_goal_iteration >= 0 and st1.expanded >= 3 and len(plan1) >= 2
    assert plan0.shape != plan1.shape or not np.array_equal(plan0, plan1)
    # the plan made on the map as set keeps clear on its first leg and enters the band on its second: what `evaluate` must find
    assert len(plan0) >= 2 and _leg_gap2(w, gap2, plan0[0]) >= kw.PLAN_LIMIT2 > _leg_gap2(w, gap2, plan0[1])
    # the relaxed start: inside the band, not on a hazard's neighbour
    r, c = kw.RELAXED_RC
    s = kw.relaxed_start(w)
    assert (int(s[1] / w.res), int(s[0] / w.res)) == (r, c) and 0 < gap2[r, c] == kw.RELAXED_GAP2 < kw.PLAN_LIMIT2
    # ... from which the hard limit plans nothing, the relaxed one reaches a goal, by another plan than the map as set
    sth, planh = _oracle_plan(w, inflated, init, calls, start=s)
    assert len(planh) == 0 and sth.first_goal_iteration < 0
    relaxed = kw.effective(w.grid, kw.RELAXED_GAP2, gap2)
    assert not relaxed[r, c]
    str_, planr = _oracle_plan(w, relaxed, init, calls, start=s)
    sts, plans = _oracle_plan(w, w.grid, init, calls, start=s)
    assert str_.first_goal_iteration >= 0 and len(planr) >= 1
    assert planr.shape != plans.shape or not np.array_equal(planr, plans)
