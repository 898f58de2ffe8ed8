"""Directed worlds for the skip planner's span masks (pp_k_plan_skips: one circle test per obstacle and span of chunks in front of the
per-chunk tests), beside tests/sweep_worlds.py and built from its pieces.

  graze        small fast boxes that touch an edge for a fraction of a chunk: the hits a span bound that is slightly too small loses.
  short<H>     time horizons of 3.0, 4.9, 5.1 and 11.6 s on the common map and samples: time rows of 3, 4, 5 and 10 chunks — less than
               a span of four, exactly one, one and a short one, two and a short one — under a fleet that passes through the disc the
               vehicle can reach in that time.
  offpower     turning radii of 10 and 12.5 m, neither a power of two, under the graze fleet and under the Gaussian rows of the fast
               fleet: the planner's forms for a radius without an exact reciprocal (d / rho, L^2 / (8 rho)), which the radii 8 and 16
               of every other world never reach.  Outside NAMES: at such a radius device and oracle poses may differ in the last bit
               at a grazing step, and these worlds are for comparing the two planners.

A plain module: no fixtures, no device.  tests/test_sweep_worlds_spans.py asserts on the oracle alone that every world holds its case;
tests/test_gpu_plan_spans.py costs them on the device."""
import functools
import math

import numpy as np

from path_planner_amd.types import make_config, H_MAX_DISTANCE
from sweep_worlds import _common, SweepWorld, through
import sweep_worlds as sw

SHORT_HORIZONS = (3.0, 4.9, 5.1, 11.6)
SHORT_CHUNKS = {3.0: 3, 4.9: 4, 5.1: 5, 11.6: 10}


def graze():
    return _common("graze", through(16, np.random.default_rng(31), (4.0, 20.0), (-20.0, 10.0), 2.0, 4.0))


def _short_fleet(H):
    """6 boxes of 2 x 4 m whose track passes, at a time inside the horizon, through the disc around the map centre that the vehicle
    (2.5 m/s) can reach in it; each row back-projected along its track to its own stamp, as sweep_worlds.through does."""
    rng = np.random.default_rng(41)
    o = np.zeros((6, 7), dtype=np.float64)
    for i in range(6):
        u, a = rng.uniform(), rng.uniform(0, 2 * math.pi)
        r = 2.0 + 0.9 * 2.5 * H * math.sqrt(u)
        px, py = sw.C + r * math.cos(a), sw.C + r * math.sin(a)
        tp = sw.T0 + rng.uniform(0.2, H - 0.2)
        h, v = rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 4.0)
        ts = sw.T0 + rng.uniform(-10.0, 0.5 * H)
        o[i] = (px - v * (tp - ts) * math.sin(h), py - v * (tp - ts) * math.cos(h), h, v, ts, 2.0, 4.0)
    return o


def short(H):
    base = _common("short%g" % H, _short_fleet(H))
    cfg = make_config(start_state_time=sw.T0, heuristic=H_MAX_DISTANCE, time_horizon=H)
    return SweepWorld(base.name, cfg, base.grid, base.res, base.rib, base._root5(), base.sx, base.sy, base.sh, obst=base.obst)


OFFPOWER_RADII = (10.0, 12.5)


def _offpower(base):
    cfg = make_config(start_state_time=sw.T0, heuristic=H_MAX_DISTANCE, turning_radius=OFFPOWER_RADII[0], coverage_turning_radius=OFFPOWER_RADII[1])
    return SweepWorld(base.name, cfg, base.grid, base.res, base.rib, base._root5(), base.sx, base.sy, base.sh, obst=base.obst, gauss=base.gauss)


def offpower():
    return _offpower(_common("offpower", graze().obst))


def gaussian_offpower():
    return _offpower(_common("gaussian_offpower", gauss=sw.gaussian("fast").gauss))


WORLDS = {"graze": graze}
WORLDS.update({"short%g" % H: functools.partial(short, H) for H in SHORT_HORIZONS})
NAMES = list(WORLDS)                   # the worlds held to the oracle to the bit
OFFPOWER = ["offpower", "gaussian_offpower"]
WORLDS.update({"offpower": offpower, "gaussian_offpower": gaussian_offpower})

_CACHE = {}


def oracle_records(name):
    """(world, records, child ribbons) of a named world, costed by the oracle once per process; the arrays are read-only."""
    if name not in _CACHE:
        w = WORLDS[name]()
        cpu, cchild = w.oracle_cost()
        cpu.setflags(write=False); cchild.setflags(write=False)
        _CACHE[name] = (w, cpu, cchild)
    return _CACHE[name]
