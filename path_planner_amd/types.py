"""ctypes / numpy mirrors of the structs in include/ppgpu.h."""
import ctypes as C

import numpy as np


class PpgpuConfig(C.Structure):
    """struct ppgpu_config (include/ppgpu.h)."""
    _fields_ = [
        ("max_speed", C.c_double), ("slow_speed", C.c_double), ("turning_radius", C.c_double),
        ("coverage_turning_radius", C.c_double), ("time_horizon", C.c_double), ("time_minimum", C.c_double),
        ("collision_checking_increment", C.c_double), ("start_state_time", C.c_double),
        ("ribbon_width", C.c_double), ("collision_penalty_factor", C.c_double),
        ("time_penalty_factor", C.c_double), ("heuristic_turning_radius", C.c_double),
        ("heuristic", C.c_int32), ("tsp_k", C.c_int32), ("branching_factor", C.c_int32), ("reserved", C.c_int32),
    ]


# Reference defaults: PlannerConfig.h:179-189, Ribbon.cpp:4, Edge.h:151-152, executive.cpp:391
CONFIG_DEFAULTS = dict(
    max_speed=2.5, slow_speed=0.5, turning_radius=8.0, coverage_turning_radius=16.0, time_horizon=30.0,
    time_minimum=5.0, collision_checking_increment=0.05, start_state_time=0.0, ribbon_width=1.5,
    collision_penalty_factor=600.0, time_penalty_factor=1.0, heuristic_turning_radius=8.0,
    heuristic=2, tsp_k=2, branching_factor=9, reserved=0,
)

H_MAX_DISTANCE, H_TSP_POINT_ALL, H_TSP_POINT_K, H_TSP_DUBINS_ALL, H_TSP_DUBINS_K = range(5)
OBST_NONE, OBST_BINARY = 0, 1
EDGE_COVERAGE, EDGE_SLOW = 1, 2
F_INFEASIBLE, F_THROWS, F_RIBBON_OVF, F_DUBINS_ERR, F_GOAL, F_DONE = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
F_RIBBON_LOST = 0x40   # the sweep ran out of its 64 ribbons per vertex and dropped pieces (always with F_RIBBON_OVF)
# why a plan's chain ended (ppgpu_cost_plans_host): PPGPU_CHAIN_*
CHAIN_LEGS, CHAIN_INFEASIBLE, CHAIN_GOAL, CHAIN_THROWS, CHAIN_CAPACITY = 1, 2, 3, 4, 5


def make_config(**kw):
    d = dict(CONFIG_DEFAULTS)
    for k, v in kw.items():
        if k not in d:
            raise KeyError(k)
        d[k] = v
    return PpgpuConfig(**d)


# struct ppgpu_vertex, 64 bytes
VERTEX_DTYPE = np.dtype([
    ("x", "<f8"), ("y", "<f8"), ("heading", "<f8"), ("speed", "<f8"), ("time", "<f8"), ("g", "<f8"),
    ("coverage_completed_time", "<f8"), ("ribbon_offset", "<i4"), ("ribbon_count", "<i4"),
])
assert VERTEX_DTYPE.itemsize == 64

# struct ppgpu_edge_result, 128 bytes
RESULT_DTYPE = np.dtype([
    ("flags", "<u4"), ("info", "<u4"), ("true_cost", "<f8"), ("collision_penalty", "<f8"), ("approx_cost", "<f8"),
    ("end_x", "<f8"), ("end_y", "<f8"), ("end_heading", "<f8"), ("end_speed", "<f8"), ("end_time", "<f8"),
    ("g", "<f8"), ("h", "<f8"), ("f", "<f8"), ("coverage_completed_time", "<f8"), ("param", "<f8", (3,)),
])
assert RESULT_DTYPE.itemsize == 128

# struct ppgpu_wrapper_edge, 96 bytes
WRAPPER_EDGE_DTYPE = np.dtype([
    ("vertex", "<i4"), ("coverage_allowed", "<i4"), ("qi", "<f8", (3,)), ("param", "<f8", (3,)), ("rho", "<f8"),
    ("type", "<i4"), ("reserved", "<i4"), ("speed", "<f8"), ("start_time", "<f8"), ("end_time", "<f8"),
])
assert WRAPPER_EDGE_DTYPE.itemsize == 96

# struct ppgpu_step_record, 64 bytes: one executed step of an edge's sweep (ppgpu_trace_*)
S_BLOCKED, S_STRAIGHT = 0x1, 0x2
STEP_DTYPE = np.dtype([
    ("x", "<f8"), ("y", "<f8"), ("heading", "<f8"), ("time", "<f8"), ("collision", "<f8"), ("penalty_before", "<f8"),
    ("flags", "<u4"), ("step", "<u4"), ("reserved", "<f8"),
])
assert STEP_DTYPE.itemsize == 64

# struct ppgpu_cover_record, 32 bytes: what one executed step did to the ribbons (ppgpu_trace_cover_*); record k of an edge belongs
# to its STEP_DTYPE record k
C_EVENT, C_COVER, C_CHANGED, C_DONE = 0x1, 0x2, 0x4, 0x8
COVER_DTYPE = np.dtype([
    ("to_cover", "<f8"), ("remaining", "<f8"), ("flags", "<u4"), ("step", "<u4"), ("ribbons", "<u4"), ("reserved", "<u4"),
])
assert COVER_DTYPE.itemsize == 32

# struct ppgpu_cover_summary, 32 bytes, per edge: the last cover (Edge.cpp:181-191) included
CS_LAST_COVER, CS_LAST_CHANGED, CS_DONE, CS_REFUSED, CS_THROWS = 0x01, 0x02, 0x04, 0x08, 0x10
COVER_SUMMARY_DTYPE = np.dtype([
    ("events", "<i4"), ("changes", "<i4"), ("ribbons_final", "<i4"), ("flags", "<u4"), ("coverage_completed_time", "<f8"),
    ("remaining_final", "<f8"),
])
assert COVER_SUMMARY_DTYPE.itemsize == 32

# struct ppgpu_contact_record, 64 bytes, per (edge, obstacle row): hits, exposure and closest approach (ppgpu_trace_contacts_*)
CONTACT_DTYPE = np.dtype([
    ("cpa_distance", "<f8"), ("cpa_time", "<f8"), ("first_hit_time", "<f8"), ("last_hit_time", "<f8"), ("exposure", "<f8"),
    ("cpa_step", "<i4"), ("hit_steps", "<i4"), ("first_hit_step", "<i4"), ("last_hit_step", "<i4"), ("peak", "<f8"),
])
assert CONTACT_DTYPE.itemsize == 64

# struct ppgpu_clearance_record, 64 bytes, per edge: the closest approach to a charted hazard (ppgpu_trace_clearance_*).  The
# distance map behind it holds min(gap2, DIST_CAP2) per cell, in cells squared (ppgpu_get_grid_distance)
DIST_CAP, DIST_CAP2 = 255, 65025
CL_EMPTY, CL_BLOCKED, CL_CAPPED, CL_NO_MAP = 0x1, 0x2, 0x4, 0x8
CLEARANCE_DTYPE = np.dtype([
    ("clearance", "<f8"), ("time", "<f8"), ("x", "<f8"), ("y", "<f8"), ("first_below_time", "<f8"),
    ("step", "<i4"), ("gap2", "<u4"), ("below_steps", "<i4"), ("first_below_step", "<i4"), ("flags", "<u4"), ("reserved", "<u4"),
])
assert CLEARANCE_DTYPE.itemsize == 64

# reachable water (ppgpu_get_grid_labels, ppgpu_set_reach_seed, ppgpu_ribbon_reach_host): struct ppgpu_reach_info, 32 bytes, and
# struct ppgpu_ribbon_reach_record, 64 bytes, per ribbon.  REACH_TILE is the labelling's tile edge in cells
REACH_NONE, REACH_TILE = 0xFFFFFFFF, 32
REACH_SEED_BLOCKED, REACH_NO_MAP = 0x1, 0x2
REACH_INFO_DTYPE = np.dtype([
    ("free_cells", "<u8"), ("reachable_cells", "<u8"), ("components", "<u4"), ("seed_label", "<u4"), ("flags", "<u4"), ("reserved", "<u4"),
])
assert REACH_INFO_DTYPE.itemsize == 32
RB_ANY_OUT, RB_WHOLE_OUT, RB_START_OUT, RB_END_OUT, RB_DEGENERATE, RB_CAPPED, RB_NO_SEED, RB_NO_MAP = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
RIBBON_REACH_DTYPE = np.dtype([
    ("length", "<f8"), ("pitch", "<f8"), ("samples", "<u4"), ("out_samples", "<u4"), ("first_out", "<i4"), ("last_out", "<i4"),
    ("min_rgap2", "<u4"), ("max_rgap2", "<u4"), ("lim2", "<u4"), ("flags", "<u4"), ("out_length", "<f8"), ("reserved", "<u8"),
])
assert RIBBON_REACH_DTYPE.itemsize == 64

# distance by water (ppgpu_set_water_seed, ppgpu_get_grid_water, ppgpu_water_distance_at, ppgpu_ribbon_water_host): struct
# ppgpu_water_info, 32 bytes, and struct ppgpu_ribbon_water_record, 64 bytes, per ribbon.  WATER_TILE is the relaxation's tile edge
WATER_NONE, WATER_STEP, WATER_DIAG, WATER_TILE, WATER_MAX_LIM2 = 0xFFFFFFFF, 12, 17, 32, 1024
WATER_SEED_BLOCKED, WATER_NO_MAP = 0x1, 0x2
WATER_INFO_DTYPE = np.dtype([
    ("wet_cells", "<u8"), ("max_wd", "<u4"), ("farthest_cell", "<u4"), ("seed_cell", "<u4"), ("flags", "<u4"), ("rounds", "<u4"), ("builds", "<u4"),
])
assert WATER_INFO_DTYPE.itemsize == 32
RW_ANY_DRY, RW_WHOLE_DRY, RW_DEGENERATE, RW_NO_SEED, RW_NO_MAP = 0x01, 0x02, 0x10, 0x40, 0x80
RIBBON_WATER_DTYPE = np.dtype([
    ("length", "<f8"), ("pitch", "<f8"), ("samples", "<u4"), ("wet_samples", "<u4"), ("nearest_sample", "<i4"), ("farthest_sample", "<i4"),
    ("min_ad", "<u4"), ("max_ad", "<u4"), ("start_ad", "<u4"), ("end_ad", "<u4"), ("lim2", "<u4"), ("flags", "<u4"), ("nearest_metres", "<f8"),
])
assert RIBBON_WATER_DTYPE.itemsize == 64

# route by water (ppgpu_get_grid_water_dirs, ppgpu_water_routes_host): the step map's codes 0..7 = N, S, W, E, NW, NE, SW, SE, and
# struct ppgpu_water_route_record, 64 bytes, per query point.  first_dir = code | WR_* << 8
ROUTE_NONE, ROUTE_SEED = 0xFF, 8
WR_DRY, WR_OUTSIDE, WR_AT_SEED, WR_TRUNCATED, WR_NO_SEED, WR_NO_MAP = 0x01, 0x02, 0x04, 0x08, 0x40, 0x80
WATER_ROUTE_DTYPE = np.dtype([
    ("point_cell", "<u4"), ("from_cell", "<u4"), ("wd", "<u4"), ("lim2", "<u4"), ("straight_steps", "<u4"), ("diagonal_steps", "<u4"),
    ("turns", "<u4"), ("vertices", "<u4"), ("vertices_written", "<u4"), ("first_dir", "<u4"), ("min_gap2", "<u4"), ("min_gap2_cell", "<u4"),
    ("metres", "<f8"), ("narrowest_metres", "<f8"),
])
assert WATER_ROUTE_DTYPE.itemsize == 64


def edge_pack(vertex, target, cfg):
    """ppgpu_edge_pack()."""
    vertex = np.asarray(vertex, dtype=np.uint64)
    target = np.asarray(target, dtype=np.uint64)
    cfg = np.asarray(cfg, dtype=np.uint64)
    return ((cfg & np.uint64(0xFF)) << np.uint64(56)) | ((vertex & np.uint64(0xFFFFFF)) << np.uint64(32)) | target
