"""Directed worlds for the collision sweep's obstacle filters (pp_k_solve_edges' omask, pp_k_plan_skips' chord test, the pose sweep's
per-chunk culling) and for the cover sweep's hit sums: obstacle fleets and horizons that workloads.obstacles() and tools/fuzz_parity.py
never draw.  Fast and reversing boxes (the |Speed| * time term of every bound), rows stamped after the vertex's first step
(dt = t - o.Time < 0), counts on both sides of 64 (where the lane culling, the LDS table, the `_many` planner kernels and omask = ~0
switch), chunks lying wholly inside several boxes, an edge that ends part-way through such a chunk, and edges of more than 256 chunks.

A plain module: no fixtures, no device.  tests/test_sweep_worlds.py asserts on the oracle alone that every world is what it claims to
be; tests/test_gpu_sweep_inputs.py costs the same worlds on the device.  oracle_records() costs a world once per process and hands
out read-only arrays."""
import functools
import math

import numpy as np

from path_planner_amd import workloads
from path_planner_amd.types import make_config, edge_pack, H_MAX_DISTANCE

C = 51.2          # the middle of the common 512 x 512 map at 0.2 m
T0 = 1.0          # the root's time
HORIZON = 30.0    # make_config's default time horizon
MASK = 0xF
RIBBON_STRIDE = 8


class SweepWorld:
    """One root vertex, explicit samples, every (sample, configuration) edge of mask 0xF in cost_edges_dense's order."""

    def __init__(self, name, cfg, grid, res, ribbons4, root5, sx, sy, sh, obst=None, gauss=None):
        self.name, self.cfg, self.grid, self.res = name, cfg, grid, res
        self.rib = np.asarray(ribbons4, dtype=np.float64).reshape(-1, 4)
        self.verts = workloads.root_vertex(root5[0], root5[1], root5[2], root5[3], root5[4], self.rib)
        self.sx, self.sy, self.sh = [np.ascontiguousarray(a, dtype=np.float64) for a in (sx, sy, sh)]
        self.obst = None if obst is None else np.ascontiguousarray(obst, dtype=np.float64).reshape(-1, 7)
        self.gauss = None if gauss is None else np.ascontiguousarray(gauss, dtype=np.float64).reshape(-1, 5)
        assert self.obst is None or self.gauss is None
        self.ns = len(self.sx)
        self.edges = edge_pack(np.zeros(self.ns * 4, dtype=np.uint64), np.repeat(np.arange(self.ns), 4), np.tile(np.arange(4), self.ns))

    @property
    def binary(self):
        return self.gauss is None

    @property
    def ng(self):
        """Entries of a vertex's time row, as ppgpu_set_config computes them."""
        return int(self.cfg.time_horizon / (self.cfg.collision_checking_increment / self.cfg.max_speed)) + 8

    def without_row(self, j):
        keep = np.arange(len(self.obst)) != j
        return SweepWorld("%s-row%d" % (self.name, j), self.cfg, self.grid, self.res, self.rib, self._root5(), self.sx, self.sy, self.sh,
                          obst=self.obst[keep])

    def _root5(self):
        v = self.verts[0]
        return [float(v["x"]), float(v["y"]), float(v["heading"]), float(v["speed"]), float(v["time"])]

    def context(self):
        """A device handle holding this world (it reads the handle switches from the environment when it is created)."""
        from path_planner_amd import api
        ctx = api.Context(0)
        ctx.set_config(self.cfg); ctx.set_grid(self.grid, self.res)
        if self.gauss is not None:
            ctx.set_gaussian_obstacles(self.gauss)
        else:
            ctx.set_obstacles(self.obst)
        ctx.set_vertices(self.verts, self.rib)
        ctx.set_samples(self.sx, self.sy, self.sh)
        return ctx

    def oracle_cost(self, threads=8):
        import oracle as orc
        world = orc.World(self.cfg, self.grid, self.res, self.obst, gauss=self.gauss)
        return world.cost_edges(self.verts, self.rib, self.sx, self.sy, self.sh, self.edges, stride=RIBBON_STRIDE, threads=threads)


# ------------------------------------------------------------------------------------------------------------ obstacle rows
def through(n, rng, speed, stamp, width, length, sign=1):
    """n rows {x, y, heading, speed, time, width, length} of boxes whose track passes within 25 m of the map centre at a time inside
    the horizon.  Each row is back-projected along its track to its own stamp T0 + stamp (a box moves along its compass heading:
    dx = speed sin(heading), dy = speed cos(heading)).  sign = -1: the heading turned by pi and the speed negated, which is the same
    track and the same box."""
    o = np.zeros((n, 7), dtype=np.float64)
    for i in range(n):
        r, a = 25.0 * math.sqrt(rng.uniform()), rng.uniform(0, 2 * math.pi)
        px, py = C + r * math.cos(a), C + r * math.sin(a)              # where the box is ...
        tp = T0 + rng.uniform(2.0, HORIZON - 2.0)                      # ... at this time
        h, v = rng.uniform(0, 2 * math.pi), rng.uniform(*speed)
        ts = T0 + rng.uniform(*stamp)
        x, y = px - v * (tp - ts) * math.sin(h), py - v * (tp - ts) * math.cos(h)
        o[i] = (x, y, h, v, ts, width, length) if sign > 0 else (x, y, h + math.pi, -v, ts, width, length)
    return o


STACKED = np.asarray([[C, C + 14, .3, .2, T0, 70, 70], [C + 5, C + 10, 2., .3, T0 - 5, 60, 80], [C - 4, C + 16, 4., .1, T0 + 3, 90, 50]],
                     dtype=np.float64)
COUNTS = (1, 63, 64, 65, 128, 129)
FAR = np.asarray([[C + 10000.0, C, 0.0, 0.0, T0, 6.0, 14.0]], dtype=np.float64)      # parked 10 km off the map: it can change no answer


def _fast(sign):
    return through(16, np.random.default_rng(21), (5.0, 20.0), (0.0, 0.0), 10.0, 30.0, sign)


def _stamps():
    return through(16, np.random.default_rng(22), (1.0, 12.0), (-60.0, 20.0), 10.0, 30.0)


def _count_rows():
    return through(129, np.random.default_rng(23), (0.0, 15.0), (-30.0, 10.0), 6.0, 14.0)


# ------------------------------------------------------------------------------------------------------------ the worlds
def _common(name, obst=None, gauss=None):
    cfg = make_config(start_state_time=T0, heuristic=H_MAX_DISTANCE)
    grid = workloads.blob_grid(512, 0.2, 0.04, 5, (C, C), keep_free_radius=8, blob=16)
    rib = [[C - 20, C + 10, C + 20, C + 10], [C - 20, C + 18, C + 20, C + 18], [C + 12, C - 25, C + 12, C + 5]]
    rng = np.random.default_rng(3)
    ext = 512 * 0.2
    sx, sy, sh = rng.uniform(0.1 * ext, 0.9 * ext, 256), rng.uniform(0.1 * ext, 0.9 * ext, 256), rng.uniform(0, 2 * np.pi, 256)
    return SweepWorld(name, cfg, grid, 0.2, rib, [C, C, 0.0, 2.5, T0], sx, sy, sh, obst=obst, gauss=gauss)


def fast():
    return _common("fast", _fast(1))


def reversed_():
    return _common("reversed", _fast(-1))


def stamps():
    return _common("stamps", _stamps())


def stacked():
    return _common("stacked", STACKED)


def count(n):
    return _common("count%d" % n, _count_rows()[:n])


def count64_far():
    return _common("count64+far", np.concatenate([_count_rows()[:64], FAR]))


def done_inside():
    """Coverage completes part-way through a chunk that lies inside both boxes: one ribbon straight ahead of the root, targets
    beyond it, the first two `stacked` boxes over everything; the edge ends time_minimum after the ribbon is done."""
    cfg = make_config(start_state_time=T0, heuristic=H_MAX_DISTANCE)
    grid = np.zeros((512, 512), dtype=np.uint8)
    rng = np.random.default_rng(5)
    sx, sy, sh = rng.uniform(C - 8, C + 8, 128), rng.uniform(C + 16, C + 45, 128), rng.uniform(-0.5, 0.5, 128)
    return SweepWorld("done_inside", cfg, grid, 0.2, [[C, C + 6, C, C + 14]], [C, C, 0.0, 2.5, T0], sx, sy, sh, obst=STACKED[:2])


LONG_STEPS = (16376, 16377, 16500)     # time rows of 16 384 entries (exactly 256 chunks), 16 385 (257: a second planner tile of one chunk), 16 508
LONG_INC = 0.025


def long_(steps):
    """Edges of more than 256 chunks: steps of 0.01 s, a slow edge advances 0.005 m per step and runs `steps` + 1 of them when its
    target is more than that far away.  Half the samples are drawn in the far corner of the map for that."""
    cfg = make_config(start_state_time=T0, heuristic=H_MAX_DISTANCE, collision_checking_increment=LONG_INC,
                      time_horizon=(steps + 0.5) * LONG_INC / 2.5)
    grid = workloads.blob_grid(512, 0.2, 0.03, 5, (10.0, 10.0), 8, 16)
    rib = [[14.0, 30.0, 90.0, 34.0], [30.0, 14.0, 36.0, 92.0]]
    rng = np.random.default_rng(7)
    n = 128
    sx, sy = rng.uniform(8.0, 96.0, n), rng.uniform(8.0, 96.0, n)
    sx[n // 2:], sy[n // 2:] = rng.uniform(70.0, 98.0, n - n // 2), rng.uniform(70.0, 98.0, n - n // 2)
    sh = rng.uniform(0, 2 * np.pi, n)
    obst = workloads.obstacles(8, 3, 512 * 0.2, time=T0)
    return SweepWorld("long%d" % steps, cfg, grid, 0.2, rib, [10.0, 10.0, 0.6, 2.5, T0], sx, sy, sh, obst=obst)


def gaussian(name):
    """The Gaussian counterpart of a binary fleet: the same rows {x, y, heading, speed, time} with the default covariance."""
    w = WORLDS[name]()
    return _common("gaussian_" + name, gauss=w.obst[:, :5])


WORLDS = {"fast": fast, "reversed": reversed_, "stamps": stamps, "stacked": stacked, "count64+far": count64_far, "done_inside": done_inside}
WORLDS.update({"count%d" % n: functools.partial(count, n) for n in COUNTS})
WORLDS.update({"long%d" % s: functools.partial(long_, s) for s in LONG_STEPS})
BINARY = ["fast", "reversed", "stamps", "stacked"] + ["count%d" % n for n in COUNTS] + ["count64+far"]     # the common world's binary fleets
GAUSSIAN = ["fast", "stamps", "count65"]
WORLDS.update({"gaussian_" + g: functools.partial(gaussian, g) for g in GAUSSIAN})

_CACHE = {}


def oracle_records(name):
    """(world, records, child ribbons) of a named world, costed by the oracle once per process; the arrays are read-only."""
    if name not in _CACHE:
        w = WORLDS[name]()
        cpu, cchild = w.oracle_cost()
        cpu.setflags(write=False); cchild.setflags(write=False)
        _CACHE[name] = (w, cpu, cchild)
    return _CACHE[name]
