"""The recipe the device's contact records (ppgpu_trace_contacts_* -> pp_k_trace_contacts) are compared against, and a directed
world of short edges.

A plain module: no fixtures, no device.  Given the obstacle rows as they were uploaded and an edge's step records (the device's own
ppgpu_step_record: x, y, time, collision, flags), replay() restates per contact what collisionExists does (Edge.cpp:150-151;
BinaryDynamicObstaclesManager.cpp:4-22, GaussianDynamicObstaclesManager.h:31-43) in numpy doubles: elementwise + - * and np.sqrt are
exact IEEE operations, one rounding each, which is what the library computes (it is built without contraction).  cosYaw / sinYaw come
from math.cos / math.sin(math.pi / 2 - heading), the host libm ppgpu_set_obstacles uses; numpy's own cos is not bit-equal to it.
tests/test_contact_trace_abi.py pins the binary hit test on the oracle."""
import math

import numpy as np

from path_planner_amd.types import CONTACT_DTYPE, S_BLOCKED

FLOOR = 1e-5      # GaussianDynamicObstaclesManager.cpp:11


class Rows:
    """Obstacle rows with the per-row constants hoisted as ppgpu_set_obstacles / ppgpu_set_gaussian_obstacles hoist them."""

    def __init__(self, obst=None, gauss=None):
        assert (obst is None) != (gauss is None)
        self.gaussian = gauss is not None
        o = np.asarray(gauss if self.gaussian else obst, dtype=np.float64)
        o = o.reshape(-1, o.shape[-1])
        self.n = o.shape[0]
        self.X, self.Y, self.Speed, self.Time = o[:, 0].copy(), o[:, 1].copy(), o[:, 3].copy(), o[:, 4].copy()
        yaw = [math.pi / 2 - float(h) for h in o[:, 2]]
        self.cosYaw = np.array([math.cos(a) for a in yaw], dtype=np.float64)
        self.sinYaw = np.array([math.sin(a) for a in yaw], dtype=np.float64)
        if not self.gaussian:
            assert o.shape[1] == 7
            self.halfW, self.halfL = (o[:, 5] + 2) / 2, (o[:, 6] + 2) / 2         # strict: Width += 2, Length += 2 (.cpp:8-11)
        else:
            assert o.shape[1] in (5, 9)
            c00, c01, c10, c11 = (o[:, 5], o[:, 6], o[:, 7], o[:, 8]) if o.shape[1] == 9 else [np.full(self.n, v) for v in (30.0, 10.0, 10.0, 30.0)]
            det = c00 * c11 - c10 * c01
            invdet = 1.0 / det
            self.i00, self.i10, self.i01, self.i11 = c11 * invdet, -c10 * invdet, -c01 * invdet, c00 * invdet
            self.norm = 1.0 / (2 * math.pi) / np.sqrt(det)

    def offsets(self, x, y, t):
        """(tx, ty)[row, point]: the pose relative to the contact's centre projected to the point's time."""
        x, y, t = [np.asarray(a, dtype=np.float64)[None, :] for a in (x, y, t)]
        c = lambda a: a[:, None]
        dt = t - c(self.Time)
        X = c(self.X) + c(self.Speed) * dt * c(self.cosYaw)
        Y = c(self.Y) + c(self.Speed) * dt * c(self.sinYaw)
        return x - X, y - Y

    def box_hit(self, x, y, t):
        """hit[row, point]: the row's strict box holds the point (pp_obstacle_hit)."""
        tx, ty = self.offsets(x, y, t)
        c = lambda a: a[:, None]
        rx = tx * c(self.cosYaw) - ty * c(self.sinYaw)
        ry = tx * c(self.sinYaw) + ty * c(self.cosYaw)
        return (np.abs(rx) < c(self.halfL)) & (np.abs(ry) < c(self.halfW))

    def pdf(self, x, y, t):
        """pdf[row, point] (pp_obstacle_pdf)."""
        tx, ty = self.offsets(x, y, t)
        c = lambda a: a[:, None]
        r0, r1 = tx * c(self.i00) + ty * c(self.i10), tx * c(self.i01) + ty * c(self.i11)
        quadform = r0 * tx + r1 * ty
        return c(self.norm) * np.exp(-0.5 * quadform)


def empty_records(n):
    r = np.zeros(n, dtype=CONTACT_DTYPE)
    for f in ("cpa_distance", "cpa_time", "first_hit_time", "last_hit_time"):
        r[f] = -1.0
    for f in ("cpa_step", "first_hit_step", "last_hit_step"):
        r[f] = -1
    return r


def replay(rows, steps):
    """The contact records of one edge from its executed steps (a 1-d array of STEP_DTYPE records, cut at the edge's count).
    Returns (records[rows.n], d2min[rows.n], pdf[rows.n, steps] or None)."""
    out = empty_records(rows.n)
    n = len(steps)
    if n == 0 or rows.n == 0:
        return out, np.full(rows.n, np.inf), None
    x, y, t = steps["x"], steps["y"], steps["time"]
    blocked = (steps["flags"] & S_BLOCKED) != 0
    tx, ty = rows.offsets(x, y, t)
    d2 = tx * tx + ty * ty
    k = np.argmin(d2, axis=1)                       # the first of equal minima
    idx = np.arange(rows.n)
    d2min = d2[idx, k]
    out["cpa_distance"], out["cpa_time"], out["cpa_step"] = np.sqrt(d2min), t[k], k
    pdf = None
    if not rows.gaussian:
        hit = rows.box_hit(x, y, t) & ~blocked[None, :]
        out["exposure"] = hit.sum(axis=1).astype(np.float64)
    else:
        counted = (steps["collision"] != 0) & ~blocked
        pdf = rows.pdf(x, y, t)
        hit = (pdf >= FLOOR) & counted[None, :]
        for j in range(rows.n):                     # in step order, one rounding per addition, as a lane adds them
            acc = 0.0
            for v in pdf[j, counted]:
                acc += float(v)
            out["exposure"][j] = acc
        out["peak"] = pdf.max(axis=1)
    out["hit_steps"] = hit.sum(axis=1)
    any_hit = hit.any(axis=1)
    first = np.argmax(hit, axis=1)
    last = n - 1 - np.argmax(hit[:, ::-1], axis=1)
    out["first_hit_step"] = np.where(any_hit, first, -1)
    out["last_hit_step"] = np.where(any_hit, last, -1)
    out["first_hit_time"] = np.where(any_hit, t[first], -1.0)
    out["last_hit_time"] = np.where(any_hit, t[last], -1.0)
    return out, d2min, pdf


def merge(segments):
    """Planner::Stats::PlanContacts from Stats::Contacts: records[segment, contact] merged over the segments — hit_steps and exposure
    summed, first and last hit the earliest and latest, CPA the smallest (the earlier segment on ties), peak the largest.  Steps
    are counted per segment: the merged record keeps the CPA's index within its own segment and no hit step indices (-1)."""
    segments = np.asarray(segments)
    out = empty_records(segments.shape[1])
    for s in segments:
        for j, r in enumerate(s):
            o = out[j]
            o["hit_steps"] += r["hit_steps"]
            o["exposure"] += r["exposure"]
            o["peak"] = max(o["peak"], r["peak"])
            if r["hit_steps"] > 0:
                if o["first_hit_time"] < 0 or r["first_hit_time"] < o["first_hit_time"]:
                    o["first_hit_time"] = r["first_hit_time"]
                o["last_hit_time"] = max(o["last_hit_time"], r["last_hit_time"])
            if r["cpa_step"] >= 0 and (o["cpa_distance"] < 0 or r["cpa_distance"] < o["cpa_distance"]):
                o["cpa_distance"], o["cpa_time"], o["cpa_step"] = r["cpa_distance"], r["cpa_time"], r["cpa_step"]
    return out


# ------------------------------------------------------------------------------------------------------------ the directed world
STEP_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129)
EC = 12.8         # the middle of a 128 x 128 map at 0.2 m
ET0 = 1.0         # the root's time
SIDE = 4.1        # x of the second vertex, whose one edge ends on the blocked cell
BLOCK_STEP = 40   # ... at about this step


class EdgesWorld:
    """Short edges, which the sweep worlds do not have (their shortest edge has 160 steps): a 128 x 128 grid at 0.2 m, the root at
    its centre (heading 0, 2.5 m/s), targets straight ahead at distances that give edges of exactly STEP_COUNTS steps, a second
    vertex whose edge a blocked cell stops within its first window, three boxes (one over the root at the root's time: hit at step 0;
    one first entered on the last step of the 64-step edge; one parked 10 km away: never hit, a huge CPA), and one wrapper-form edge
    whose curve starts after the vertex's first step (no steps)."""

    def __init__(self):
        import oracle as orc
        from path_planner_amd import workloads
        from path_planner_amd.types import make_config, edge_pack, H_MAX_DISTANCE, VERTEX_DTYPE, WRAPPER_EDGE_DTYPE
        self.cfg = make_config(start_state_time=ET0, heuristic=H_MAX_DISTANCE)
        inc = self.cfg.collision_checking_increment
        self.res = 0.2
        self.grid = np.zeros((128, 128), dtype=np.uint8)
        self.pool = np.array([[1.0, 2.0, 1.0, 20.0]])                                   # one ribbon far to the west: no edge finishes coverage
        root = workloads.root_vertex(EC, EC, 0.0, 2.5, ET0, self.pool)
        self.verts = np.zeros(2, dtype=VERTEX_DTYPE)
        self.verts[0] = root[0]
        self.verts[1] = root[0]
        self.verts[1]["x"] = SIDE
        # step k of a straight edge lies k increments ahead of its vertex: an edge of n steps ends between steps n - 1 and n
        self.sy = np.array([EC + inc * (n - 0.5) for n in STEP_COUNTS] + [EC + inc * 100.5], dtype=np.float64)
        self.sx = np.array([EC] * len(STEP_COUNTS) + [SIDE], dtype=np.float64)
        self.sh = np.zeros(len(self.sx))
        row = int((EC + inc * BLOCK_STEP + self.res / 2) / self.res)
        self.grid[row, int(SIDE / self.res)] = 1                                        # the one blocked cell, ahead of the second vertex
        self.blocked_edge = len(STEP_COUNTS)
        self.edges = edge_pack(np.array([0] * len(STEP_COUNTS) + [1], dtype=np.uint64), np.arange(len(self.sx)), np.zeros(len(self.sx), dtype=np.uint64))
        y63 = EC + inc * 63
        self.obst = np.array([
            [EC, EC, math.pi / 2, 5.0, ET0, 0.5, 0.5],                                  # over the root at the root's time, leaving eastwards
            [EC, y63 - inc / 2 + 2.0, 0.0, 0.0, ET0, 2.0, 2.0],                         # its near side lies between steps 62 and 63 of the root's edges
            [EC + 10000.0, EC, 0.0, 0.0, ET0, 6.0, 14.0],                               # parked 10 km away
        ], dtype=np.float64)
        self.gauss = None
        self.binary = True
        self.world = orc.World(self.cfg, self.grid, self.res, self.obst)
        self.records = self.world.cost_edges(self.verts, self.pool, self.sx, self.sy, self.sh, self.edges)
        self.records.setflags(write=False)
        # the 64-step edge again as a curve that starts after the vertex's first step (Edge.cpp:126-133: the first sample throws)
        i = STEP_COUNTS.index(64)
        r = self.records[i]
        dt = inc / self.cfg.max_speed
        p8 = np.array([EC, EC, orc.yaw(0.0), r["param"][0], r["param"][1], r["param"][2], self.cfg.turning_radius, float(r["info"] & 0xFF)])
        self.wedges = np.zeros(2, dtype=WRAPPER_EDGE_DTYPE)
        for j, start in enumerate((ET0, ET0 + 1.5 * dt)):
            end = orc.O.ppo_wrapper_fill_end_time(p8.ctypes.data, self.cfg.max_speed, start)
            self.wedges[j] = (0, 0, p8[0:3], p8[3:6], p8[6], int(p8[7]), 0, self.cfg.max_speed, start, end)

    def context(self):
        from path_planner_amd import api
        ctx = api.Context(0)
        ctx.set_config(self.cfg)
        ctx.set_grid(self.grid, self.res)
        ctx.set_obstacles(self.obst)
        ctx.set_vertices(self.verts, self.pool)
        ctx.set_samples(self.sx, self.sy, self.sh)
        return ctx


_WORLD = []


def edges_world():
    """The directed world, built (and costed by the oracle) once per process."""
    if not _WORLD:
        _WORLD.append(EdgesWorld())
    return _WORLD[0]
