"""-m gpu: several of the host planner's plan reports (PlannerConfig::setPlanTrace / setPlanCoverage / setPlanContacts / setPlanClearance)
sharing one plan() or one evaluatePlans() call, through plan_cli on the fixed-clock scenario of the neighbouring tests: every report is
what the same call gives when it is the only one asked for."""
import os
import tempfile

import numpy as np
import pytest

import test_gpu_plan_clearance as pcl
import test_gpu_plan_contacts as pco
from test_gpu_host_planner import _write_map

pytestmark = pytest.mark.gpu

KINDS = {           # switch -> the JSON keys it adds  (the scenario's clock and budget are test_gpu_plan_clearance's T0, DT, CALLS, INIT)
    "plan_trace": ("plan_trace_segments", "plan_trace_steps"),
    "plan_coverage": ("plan_coverage_steps",),
    "plan_contacts": pco.CONTACT_KEYS,
    "plan_clearance": pcl.KEYS,
}
REPORT_KEYS = tuple(k for keys in KINDS.values() for k in keys)


def _world():
    """test_gpu_plan_clearance's world (config 2 with an island three metres north of the first survey line) with vessels.  Config 2
    has no obstacles of its own, so they are the boxes of test_gpu_plan_contacts' world, which is config 2 too."""
    w = pcl._world()
    w.obst = pco._world().obst
    return w


def _search(r):
    """The plan and every search statistic of a plan() line."""
    return {k: v for k, v in r.items() if not k.startswith("wall_ms") and k not in REPORT_KEYS}


def test_four_reports_in_one_plan_are_the_four_reports_alone():
    """One run with all four switches on against four runs with plan_trace and one of the others: every file of the combined run is
    byte-equal to the file of the run that made it alone (the trace file to all four), each report's JSON keys are equal, and so are
    the plan and the search statistics."""
    w = _world()
    margin = [f"cfg plan_clearance_margin {pcl.WIDE_MARGIN}"]

    def run(d, name, kinds):
        files = {k: os.path.join(d, f"{name}_{k}.txt") for k in kinds}
        r = pcl._run(w, d, name, margin + [f"cfg {k} 1" for k in kinds] + [f"{k}_file {p}" for k, p in files.items()])
        return r, {k: open(p, "rb").read() for k, p in files.items()}

    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        both, both_files = run(d, "all", list(KINDS))
        alone = {k: run(d, k, ["plan_trace"] + ([k] if k != "plan_trace" else [])) for k in KINDS}
    print("all four:", {k: both[k] for k in REPORT_KEYS}, "| file bytes", {k: len(v) for k, v in both_files.items()})
    # it exercises something: several segments, a contact with a closest approach, a clearance
    assert len(both["plan"]) >= 2 and both["plan_trace_segments"] == len(both["plan"])
    assert both["nearest_contact_mmsi"] >= 1 and both["nearest_contact_cpa"] >= 0
    assert both["plan_clearance"] >= 0 and both["plan_clearance_time"] >= 0
    for k, (r, files) in alone.items():
        assert files[k] == both_files[k] and len(files[k]) > 0, k
        assert files["plan_trace"] == both_files["plan_trace"], k
        assert [r[j] for j in KINDS[k] + KINDS["plan_trace"]] == [both[j] for j in KINDS[k] + KINDS["plan_trace"]], k
        assert _search(r) == _search(both), k
        assert [j for j in both if j in r] == list(r), k           # (and the keys come in the same order)


def test_both_reports_in_one_evaluation_are_the_two_reports_alone():
    """plan_cli evaluate on three prev_begin blocks (the plan a first cycle returned, its first leg alone, a plan that ended before the
    start time) with plan_contacts and plan_clearance both on: per plan the contact keys of a run with contacts alone and the clearance
    keys of a run with clearance alone; the empty plan has no clearance and no contact hit or approached; the whole plan's keys are
    those plan() reported for it (the closest approach to the last bit: plan() sweeps from the search's vertices, the evaluation
    from the chain's records)."""
    w = _world()
    row = lambda p: "prev " + " ".join(repr(float(v)) if i != 7 else str(int(v)) for i, v in enumerate(p))
    contacts, clearance = ["cfg plan_contacts 1"], ["cfg plan_clearance 1", "cfg plan_clearance_margin 2.5"]
    c = float(w.start5[0])
    past = f"prev {c!r} {c!r} 0.0 1.0 1.0 1.0 8.0 0 2.5 0.0 0.5"       # ends before the start's time
    with tempfile.TemporaryDirectory() as d:
        _write_map(w.grid, w.res, os.path.join(d, "grid.map"))
        first = pcl._run(w, d, "first", contacts + clearance)
        plan = np.array(first["plan"], dtype=np.float64).reshape(-1, 11)
        assert len(plan) >= 2
        blocks = ["prev_begin"] + [row(p) for p in plan] + ["prev_end", "prev_begin", row(plan[0]), "prev_end", "prev_begin", past, "prev_end", "evaluate"]
        both = pcl._run(w, d, "ev_both", blocks + contacts + clearance)["evaluations"]
        only_contacts = pcl._run(w, d, "ev_contacts", blocks + contacts)["evaluations"]
        only_clearance = pcl._run(w, d, "ev_clearance", blocks + clearance)["evaluations"]
    print("evaluate:", [[e[k] for k in pco.CONTACT_KEYS + pcl.KEYS] for e in both], "| plan():", [first[k] for k in pco.CONTACT_KEYS + pcl.KEYS])
    assert len(both) == len(only_contacts) == len(only_clearance) == 3
    assert [e["legs_costed"] for e in both] == [len(plan), 1, 0]
    for e, a, b in zip(both, only_contacts, only_clearance):
        assert {k: v for k, v in e.items() if k not in pcl.KEYS} == a and not any(k in a for k in pcl.KEYS)
        assert {k: v for k, v in e.items() if k not in pco.CONTACT_KEYS} == b and not any(k in b for k in pco.CONTACT_KEYS)
    assert [both[2][k] for k in pcl.KEYS] == [-1.0, -1.0, 0]
    assert [both[2][k] for k in pco.CONTACT_KEYS] == [0, -1, -1.0]
    assert [both[0][k] for k in pcl.KEYS] == [first[k] for k in pcl.KEYS]
    assert [both[0][k] for k in pco.CONTACT_KEYS[:2]] == [first[k] for k in pco.CONTACT_KEYS[:2]]
    assert abs(both[0]["nearest_contact_cpa"] - first["nearest_contact_cpa"]) <= np.spacing(first["nearest_contact_cpa"])
    assert first["plan_contacts_hit"] >= 1 and first["nearest_contact_mmsi"] >= 1 and first["plan_clearance"] >= 0
