"""The worlds of tests/sweep_worlds_spans.py hold their cases, on the oracle alone (no device).  Conditions, not measurements: if a
fleet misses a bar, the fleet changes, not the bar."""
import math

import numpy as np
import pytest

import sweep_worlds_spans as sp
from path_planner_amd.types import F_INFEASIBLE


def _shape(name):
    w, cpu, _ = sp.oracle_records(name)
    feas = (cpu["flags"] & F_INFEASIBLE) == 0
    hits = cpu["collision_penalty"] / w.cfg.collision_penalty_factor
    assert len(cpu) == 1024 and w.cfg.collision_penalty_factor == 600.0
    assert np.array_equal(hits, np.round(hits))                # whole hits: the device tests may demand the same bits
    return w, feas, hits


def test_graze_touches_edges_for_a_fraction_of_a_chunk():
    w, feas, hits = _shape("graze")
    few, fewer, none = int((feas & (hits > 0) & (hits <= 32)).sum()), int((feas & (hits > 0) & (hits <= 8)).sum()), int((feas & (hits == 0)).sum())
    print("graze: feasible", int(feas.sum()), "0 < hits <= 32:", few, "hits <= 8:", fewer, "no hit:", none)
    assert w.obst.shape == (16, 7) and np.all(w.obst[:, 5] == 2.0) and np.all(w.obst[:, 6] == 4.0) and float(w.obst[:, 3].min()) >= 4.0
    assert few >= 300
    assert fewer >= 50
    assert none >= 20


@pytest.mark.parametrize("H", sp.SHORT_HORIZONS)
def test_short_horizon_rows_and_hits(H):
    w, feas, hits = _shape("short%g" % H)
    assert w.cfg.time_horizon == H and w.obst.shape == (6, 7)
    assert (w.ng + 63) // 64 == sp.SHORT_CHUNKS[H]
    hit, few, none = int((feas & (hits > 0)).sum()), int((feas & (hits > 0) & (hits <= 32)).sum()), int((feas & (hits == 0)).sum())
    print("short", H, "ng", w.ng, "feasible hit:", hit, "0 < hits <= 32:", few, "feasible, no hit:", none)
    assert hit >= 150
    assert few >= 100
    assert none >= 100


def test_offpower_worlds_hold_their_case():
    """Radii that are no power of two, so the device takes its d / rho forms; the binary world has edges with hits and edges without."""
    for name in sp.OFFPOWER:
        w = sp.WORLDS[name]()
        for r in (w.cfg.turning_radius, w.cfg.coverage_turning_radius):
            assert math.frexp(r)[0] != 0.5, (name, r)
    assert not sp.WORLDS["gaussian_offpower"]().binary and not set(sp.OFFPOWER) & set(sp.NAMES)
    w, feas, hits = _shape("offpower")
    hit, none = int((feas & (hits > 0)).sum()), int((feas & (hits == 0)).sum())
    print("offpower: feasible", int(feas.sum()), "hit:", hit, "no hit:", none)
    assert w.binary and w.obst.shape == (16, 7)
    assert hit >= 1
    assert none >= 1
