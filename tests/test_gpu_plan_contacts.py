"""-m gpu: the host planner's per-contact reports (PlannerConfig::setPlanContacts -> Planner::Stats::Contacts / PlanContacts,
GpuAStarPlanner::PlanEvaluation::contacts) through plan_cli on fixed-clock scenarios of tests/test_gpu_host_planner.py's kind,
against the recipe of tests/contact_replay.py run on the poses the same run's plan trace wrote."""
import copy
import math
import os
import tempfile

import numpy as np
import pytest

from test_gpu_host_planner import _run_cli, _scenario, _write_map

pytestmark = pytest.mark.gpu

T0, DT, CALLS, INIT = 1000.0, 1e-3, 40, 256
CONTACT_KEYS = ("plan_contacts_hit", "nearest_contact_mmsi", "nearest_contact_cpa")


def _world():
    """Config 2 (no obstacles of its own) with boxes across the survey lines: one the vehicle starts inside (every plan pays for
    it), one moving east along the first line, one parked on the second, one parked 10 km away."""
    from path_planner_amd import workloads
    w = copy.copy(workloads.by_name("cfg2"))
    c = float(w.start5[0])
    w.obst = np.array([
        [c + 1.5, c + 2.0, 0.0, 0.0, 1.0, 10.0, 10.0],
        [c - 10, c + 10, math.pi / 2, 1.0, 1.0, 4.0, 12.0],
        [c + 15, c + 30, 0.3, 0.0, -4.0, 6.0, 6.0],
        [c + 10000.0, c, 0.0, 0.0, 1.0, 6.0, 14.0],
    ], dtype=np.float64)
    return w


def _stats(r):
    return {k: v for k, v in r.items() if not k.startswith("wall_ms") and not k.startswith("plan_trace_") and k not in CONTACT_KEYS}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)


def _steps_of(rows):
    """plan_trace_file rows (segment step x y heading time collision penalty_before flags) of one segment as step records."""
    from path_planner_amd.types import STEP_DTYPE
    s = np.zeros(len(rows), dtype=STEP_DTYPE)
    s["step"], s["x"], s["y"], s["heading"], s["time"] = rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
    s["collision"], s["penalty_before"], s["flags"] = rows[:, 6], rows[:, 7], rows[:, 8]
    return s


def _file_records(rows, n_obst):
    """plan_contacts_file rows (segment mmsi hit_steps first_hit_time last_hit_time cpa_distance cpa_time exposure peak) as
    records[segment, contact]; the MMSIs are 1 .. n_obst in row order."""
    import contact_replay as cr
    nseg = int(rows[:, 0].max()) + 1
    assert len(rows) == nseg * n_obst
    out = np.stack([cr.empty_records(n_obst) for _ in range(nseg)])
    for k, r in enumerate(rows):
        s, j = divmod(k, n_obst)
        assert (int(r[0]), int(r[1])) == (s, j + 1)
        o = out[s, j]
        o["hit_steps"], o["first_hit_time"], o["last_hit_time"], o["cpa_distance"], o["cpa_time"], o["exposure"], o["peak"] = r[2:9]
        o["cpa_step"] = 0 if r[5] >= 0 else -1            # (the file has no step indices: merge() only asks whether there is a CPA)
    return out


def _keys_of(merged):
    """The three JSON keys of a plan's merged records."""
    has = merged["cpa_step"] >= 0
    hit = int(np.count_nonzero(merged["hit_steps"] > 0))
    if not has.any():
        return hit, -1, -1.0
    j = int(np.argmin(np.where(has, merged["cpa_distance"], np.inf)))
    return hit, j + 1, float(merged["cpa_distance"][j])


def _run(w, d, name, extra, gauss=None):
    sc = os.path.join(d, name + ".txt")
    _scenario(w, sc, os.path.join(d, "grid.map"), T0, DT, CALLS, INIT, gauss=gauss)
    with open(sc, "a") as f:
        f.write("".join(line + "\n" for line in extra))
    return _run_cli(sc)


def test_plan_contacts_equal_the_recipe_on_the_plan_trace():
    """cfg plan_trace 1 + cfg plan_contacts 1: the contacts file equals the recipe on the trace file's poses segment by segment; the
    exposures times 600 sum to the segments' collision penalties exactly; the JSON keys are those of the stated merge.  Two
    runs of the same binary, option off and on: the same plan, the same statistics, the same keys but the three new ones."""
    import contact_replay as cr
    from parity import REL_TOL
    w = _world()
    n_obst = len(w.obst)
    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        tf, cf = os.path.join(d, "trace.txt"), os.path.join(d, "contacts.txt")
        off = _run(w, d, "off", ["cfg plan_trace 1", "cfg plan_contacts 0", f"plan_contacts_file {cf}"])
        assert not os.path.exists(cf)
        on = _run(w, d, "on", ["cfg plan_trace 1", f"plan_trace_file {tf}", "cfg plan_contacts 1", f"plan_contacts_file {cf}"])
        trace = np.loadtxt(tf, ndmin=2)
        crow = np.loadtxt(cf, ndmin=2)
    assert not any(k in off for k in CONTACT_KEYS) and [k for k in on if k not in CONTACT_KEYS] == list(off)
    assert _stats(on) == _stats(off) and on["plan"] == off["plan"]
    assert on["plan_trace_segments"] == off["plan_trace_segments"] and on["plan_trace_steps"] == off["plan_trace_steps"]
    plan = on["plan"]
    assert len(plan) >= 2
    got = _file_records(crow, n_obst)
    assert got.shape == (len(plan), n_obst)
    rows = cr.Rows(obst=w.obst)
    penalties = 0.0
    for s in range(len(plan)):
        steps = _steps_of(trace[trace[:, 0] == s])
        want, _, _ = cr.replay(rows, steps)
        for f in ("hit_steps", "first_hit_time", "last_hit_time", "cpa_time", "exposure", "peak"):
            assert np.array_equal(got[s][f], want[f]), (s, f, got[s][f], want[f])
        assert np.all(np.abs(got[s]["cpa_distance"] - want["cpa_distance"]) <= np.spacing(want["cpa_distance"])), s
        seg_penalty = steps["penalty_before"][-1] + steps["collision"][-1] * 600.0
        assert got[s]["exposure"].sum() * 600.0 == seg_penalty, (s, got[s]["exposure"], seg_penalty)
        penalties += seg_penalty
    assert crow[:, 7].sum() * 600.0 == penalties and penalties > 0
    assert _rel(penalties, on["plan_collision_penalty"]) <= REL_TOL
    merged = cr.merge(got)
    assert merged["hit_steps"][0] > 0 and merged["first_hit_time"][0] == trace[0, 5]          # the box over the start, from the first step
    assert merged["hit_steps"][3] == 0 and merged["cpa_distance"][3] > 9000
    assert (on["plan_contacts_hit"], on["nearest_contact_mmsi"], on["nearest_contact_cpa"]) == _keys_of(merged)
    print("plan contacts:", len(plan), "segments,", [on[k] for k in CONTACT_KEYS], "hit steps per contact", merged["hit_steps"].tolist())


def test_gaussian_plan_contacts_match_the_recipe():
    """The same boxes' tracks as Gaussian contacts (default covariance): exposure, peak and closest approach within REL_TOL of the
    recipe on the trace file's poses, the counted steps being those whose trace record has a collision value."""
    import contact_replay as cr
    from parity import REL_TOL
    w = _world()
    gauss = w.obst[:, :5].copy()
    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        tf, cf = os.path.join(d, "trace.txt"), os.path.join(d, "contacts.txt")
        on = _run(w, d, "on", ["cfg plan_trace 1", f"plan_trace_file {tf}", "cfg plan_contacts 1", f"plan_contacts_file {cf}"], gauss=gauss)
        trace = np.loadtxt(tf, ndmin=2)
        crow = np.loadtxt(cf, ndmin=2)
    plan = on["plan"]
    got = _file_records(crow, len(gauss))
    assert got.shape == (len(plan), len(gauss)) and len(plan) >= 1
    rows = cr.Rows(gauss=gauss)
    total = 0.0
    for s in range(len(plan)):
        steps = _steps_of(trace[trace[:, 0] == s])
        want, _, pdf = cr.replay(rows, steps)
        for f in ("exposure", "peak", "cpa_distance"):
            assert _rel(got[s][f], want[f]).max() <= REL_TOL, (s, f, got[s][f], want[f])
        assert np.array_equal(got[s]["cpa_time"], want["cpa_time"])
        counted = steps["collision"] != 0
        at_floor = ((np.abs(pdf - cr.FLOOR) <= REL_TOL * cr.FLOOR) & counted[None, :]).sum(axis=1)
        assert np.all(np.abs(got[s]["hit_steps"] - want["hit_steps"]) <= at_floor), (s, got[s]["hit_steps"], want["hit_steps"])
        total += float(got[s]["exposure"].sum()) * 600.0
    assert total > 0 and _rel(total, on["plan_collision_penalty"]) <= REL_TOL
    assert (on["plan_contacts_hit"], on["nearest_contact_mmsi"]) == _keys_of(cr.merge(got))[:2]
    print("gaussian plan contacts:", len(plan), "segments,", [on[k] for k in CONTACT_KEYS], "penalty", total)


def test_evaluate_reports_the_contacts_of_every_plan():
    """plan_cli evaluate on two prev_begin blocks (the plan a first cycle returned, and its first leg alone) with the option on:
    per plan, the three keys are those of the recipe on ppgpu_trace_wrapper_edges_host of the same legs, each leg traced from
    the vertex the leg before it left; with the option off the line is what it was."""
    import contact_replay as cr
    from path_planner_amd import api
    from path_planner_amd.types import WRAPPER_EDGE_DTYPE, VERTEX_DTYPE
    w = _world()
    row = lambda p: "prev " + " ".join(repr(float(v)) if i != 7 else str(int(v)) for i, v in enumerate(p))
    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        plan = np.array(_run(w, d, "first", [])["plan"], dtype=np.float64).reshape(-1, 11)
        assert len(plan) >= 2
        blocks = ["prev_begin"] + [row(p) for p in plan] + ["prev_end", "prev_begin", row(plan[0]), "prev_end", "evaluate"]
        off = _run(w, d, "ev_off", blocks)["evaluations"]
        on = _run(w, d, "ev_on", blocks + ["cfg plan_contacts 1"])["evaluations"]
    assert len(on) == 2 and [{k: v for k, v in e.items() if k not in CONTACT_KEYS} for e in on] == off
    assert not any(k in e for e in off for k in CONTACT_KEYS)
    # the same legs on a handle of our own: the chain's records and child lists, then every costed leg from its parent vertex
    c = w.cfg
    assert c.start_state_time == float(w.start5[4])                     # (plan_cli sets it to the start's time)
    ctx = api.Context(0)
    ctx.set_config(c); ctx.set_grid(w.grid, w.res); ctx.set_obstacles(w.obst)
    root = w.root()
    ctx.set_vertices(root, w.ribbons4)
    cands = [plan, plan[:1]]
    legs = np.zeros(sum(len(p) for p in cands), dtype=WRAPPER_EDGE_DTYPE)
    offsets = [0]
    for p in cands:
        for seg in p:
            legs[offsets[-1]] = (0, 1 if seg[6] == c.coverage_turning_radius else 0, seg[0:3], seg[3:6], seg[6], int(seg[7]), 0, seg[8], seg[9], seg[10])
            offsets[-1] += 1
        offsets.append(offsets[-1])
    offsets = [0] + offsets[:-1]
    res, child, costed, stop = ctx.cost_plans(offsets, legs, 64)
    rows = cr.Rows(obst=w.obst)
    for i, p in enumerate(cands):
        assert costed[i] == on[i]["legs_costed"] == len(p)
        verts = np.zeros(costed[i], dtype=VERTEX_DTYPE)
        pool = [np.asarray(w.ribbons4, dtype=np.float64).reshape(-1, 4)]
        verts[0] = root[0]
        we = legs[offsets[i]:offsets[i] + costed[i]].copy()
        for j in range(1, costed[i]):
            r = res[offsets[i] + j - 1]
            nr = int((r["info"] >> 8) & 0xFF)
            verts[j] = (r["end_x"], r["end_y"], r["end_heading"], r["end_speed"], r["end_time"], r["g"], r["coverage_completed_time"],
                        sum(len(q) for q in pool), nr)
            pool.append(child[offsets[i] + j - 1, :nr])
            we[j]["vertex"] = j
        ctx.set_vertices(verts, np.concatenate(pool))
        wres, counts, steps = ctx.trace_wrapper_edges(we, 1504)
        assert np.array_equal(counts, res["info"][offsets[i]:offsets[i] + costed[i]] >> 16)
        segs = np.stack([cr.replay(rows, steps[j, :counts[j]])[0] for j in range(costed[i])])
        hit, mmsi, cpa = _keys_of(cr.merge(segs))
        e = on[i]
        assert (e["plan_contacts_hit"], e["nearest_contact_mmsi"]) == (hit, mmsi), (i, e, hit, mmsi, cpa)
        assert abs(e["nearest_contact_cpa"] - cpa) <= np.spacing(cpa), (i, e, cpa)
        assert float(segs["exposure"].sum()) * 600.0 == sum(leg["collision_penalty"] for leg in e["legs"])
    assert on[0]["plan_contacts_hit"] >= 1
    print("evaluate:", [[e[k] for k in CONTACT_KEYS] for e in on])
