"""ctypes binding of libppgpu.so (include/ppgpu.h).  Glue for tests/ and bench.py.

Importing this module REQUIRES the in-tree HIP library; there is no fallback.
"""
import ctypes as C
import os

import numpy as np

from .types import PpgpuConfig, RESULT_DTYPE, VERTEX_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPGPU_LIB_OVERRIDE") or os.path.join(_HERE, "csrc", "libppgpu.so")   # override: the A/B tools (tools/ab_libs.sh, tools/records_hash.py, tools/kernel_times.py)


class PpgpuError(RuntimeError):
    pass


def _load():
    # The PyTorch wheel carries its own ROCm runtime; whichever libamdhip64 a process loads first serves every later user.  Loaded
    # after this library's, torch reports "No HIP GPUs are available".  tests/ and bench.py pair the two, so torch goes first
    # whenever it is installed (importing it does not touch the device).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). path_planner_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u32, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
    sig = {
        "ppgpu_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "ppgpu_destroy": (C.c_int, [vp]),
        "ppgpu_last_error": (C.c_char_p, []),
        "ppgpu_set_stream": (C.c_int, [vp, vp]),
        "ppgpu_synchronize": (C.c_int, [vp]),
        "ppgpu_reserve_samples": (C.c_int, [vp, i64, i32]),
        "ppgpu_growth_stats": (C.c_int, [vp, C.POINTER(u64), C.POINTER(dbl)]),
        "ppgpu_device_alloc": (C.c_int, [vp, u64, C.POINTER(vp)]),
        "ppgpu_device_free": (C.c_int, [vp, vp]),
        "ppgpu_device_read": (C.c_int, [vp, vp, vp, u64]),
        "ppgpu_copy_engine_read": (C.c_int, [vp, vp, vp, u64]),
        "ppgpu_copy_engine_wait": (C.c_int, [vp]),
        "ppgpu_heuristic_host": (C.c_int, [vp, i32, vp, vp, vp, vp, vp]),
        "ppgpu_set_tsp_table": (C.c_int, [vp, i32, i32]),
        "ppgpu_set_dubins_tsp_table": (C.c_int, [vp, i32, i32]),
        "ppgpu_tsp_table_stats": (C.c_int, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "ppgpu_last_tsp_table_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_expand_capacity": (C.c_int64, [i32, i32]),
        "ppgpu_expand_host": (C.c_int, [vp, i32, vp, i32, vp, vp, i32, C.POINTER(C.c_int64), vp, vp, vp, i32]),
        "ppgpu_enable_timing": (C.c_int, [vp, i32]),
        "ppgpu_last_timing": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]),
        "ppgpu_past_timing": (C.c_int, [vp, i32, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]),
        "ppgpu_last_cover_edges": (C.c_int, [vp, C.POINTER(i64)]),
        "ppgpu_last_shared_edges": (C.c_int, [vp, C.POINTER(i64)]),
        "ppgpu_last_swept_edges": (C.c_int, [vp, C.POINTER(i64)]),
        "ppgpu_last_stop_members": (C.c_int, [vp, C.POINTER(i64)]),
        "ppgpu_last_arc_stops_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_last_slices": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "ppgpu_set_config": (C.c_int, [vp, C.POINTER(PpgpuConfig)]),
        "ppgpu_set_grid": (C.c_int, [vp, vp, i32, i32, dbl]),
        "ppgpu_get_grid_clearance": (C.c_int, [vp, vp, i64]),
        "ppgpu_set_obstacles": (C.c_int, [vp, i32, i32, vp]),
        "ppgpu_set_gaussian_obstacles": (C.c_int, [vp, i32, vp, i32]),
        "ppgpu_set_vertices": (C.c_int, [vp, i32, vp, i32, vp]),
        "ppgpu_sampler_init": (C.c_int, [vp, vp, u64, i32, vp]),
        "ppgpu_sampler_add": (C.c_int, [vp, i64, C.POINTER(i64)]),
        "ppgpu_sampler_skip": (C.c_int, [vp, i64]),
        "ppgpu_set_samples": (C.c_int, [vp, i64, vp, vp, vp]),
        "ppgpu_set_extra_targets": (C.c_int, [vp, i32, vp, vp, vp, C.POINTER(i64)]),
        "ppgpu_get_samples": (C.c_int, [vp, i64, i64, vp]),
        "ppgpu_num_samples": (i64, [vp]),
        "ppgpu_dubins_lengths": (C.c_int, [vp, i32, i32, vp]),
        "ppgpu_select_nearest": (C.c_int, [vp, i32, i32, i32, vp, vp]),
        "ppgpu_expand_order": (C.c_int, [vp, i32, i32, i32, vp, C.POINTER(u32)]),
        "ppgpu_order_fallbacks": (u64, [vp]),
        "ppgpu_cost_edges_dense": (C.c_int, [vp, i32, i32, i64, i64, u32, vp, vp, i32]),
        "ppgpu_cost_edges_list": (C.c_int, [vp, i64, vp, vp, vp, i32]),
        "ppgpu_cost_edges_host": (C.c_int, [vp, i64, vp, vp, vp, i32]),
        "ppgpu_cost_wrapper_edges_host": (C.c_int, [vp, i64, vp, vp, vp, i32]),
        "ppgpu_cost_plans_host": (C.c_int, [vp, i32, vp, vp, vp, vp, i32, vp, vp]),
        "ppgpu_trace_edges_list": (C.c_int, [vp, i64, vp, vp, i32, vp, vp]),
        "ppgpu_trace_edges_host": (C.c_int, [vp, i64, vp, vp, i32, vp, vp]),
        "ppgpu_trace_wrapper_edges_host": (C.c_int, [vp, i64, vp, vp, i32, vp, vp]),
        "ppgpu_last_trace_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_trace_cover_list": (C.c_int, [vp, i64, vp, vp, i32, vp, vp, vp, vp, i32]),
        "ppgpu_trace_cover_host": (C.c_int, [vp, i64, vp, vp, i32, vp, vp, vp, vp, i32]),
        "ppgpu_trace_cover_wrapper_edges_host": (C.c_int, [vp, i64, vp, vp, i32, vp, vp, vp, vp, i32]),
        "ppgpu_last_cover_trace_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_obstacle_count": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "ppgpu_trace_contacts_list": (C.c_int, [vp, i64, vp, vp, vp, vp]),
        "ppgpu_trace_contacts_host": (C.c_int, [vp, i64, vp, vp, vp, vp]),
        "ppgpu_trace_contacts_wrapper_edges_host": (C.c_int, [vp, i64, vp, vp, vp, vp]),
        "ppgpu_last_contact_trace_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_get_grid_distance": (C.c_int, [vp, vp, i64]),
        "ppgpu_grid_clearance_at": (C.c_int, [vp, i64, vp, vp, vp]),
        "ppgpu_last_grid_distance_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_trace_clearance_list": (C.c_int, [vp, i64, vp, vp, vp, vp, dbl]),
        "ppgpu_trace_clearance_host": (C.c_int, [vp, i64, vp, vp, vp, vp, dbl]),
        "ppgpu_trace_clearance_wrapper_edges_host": (C.c_int, [vp, i64, vp, vp, vp, vp, dbl]),
        "ppgpu_last_clearance_trace_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_keepout_limit2": (C.c_int, [dbl, dbl, C.POINTER(u32)]),
        "ppgpu_set_keepout_limit2": (C.c_int, [vp, u32]),
        "ppgpu_get_keepout_limit2": (C.c_int, [vp, C.POINTER(u32)]),
        "ppgpu_get_grid_blocked": (C.c_int, [vp, vp, i64]),
        "ppgpu_last_keepout_timing": (C.c_int, [vp, C.POINTER(dbl)]),
        "ppgpu_get_grid_labels": (C.c_int, [vp, vp, i64]),
        "ppgpu_set_reach_seed": (C.c_int, [vp, dbl, dbl, vp]),
        "ppgpu_get_grid_reach_gap": (C.c_int, [vp, vp, i64]),
        "ppgpu_ribbon_reach_host": (C.c_int, [vp, i32, vp, dbl, vp]),
        "ppgpu_last_reach_timing": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]),
        "ppgpu_set_water_seed": (C.c_int, [vp, dbl, dbl, vp]),
        "ppgpu_get_grid_water": (C.c_int, [vp, vp, i64]),
        "ppgpu_water_distance_at": (C.c_int, [vp, i64, vp, vp, vp]),
        "ppgpu_ribbon_water_host": (C.c_int, [vp, i32, vp, dbl, vp]),
        "ppgpu_last_water_timing": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(dbl)]),
        "ppgpu_get_grid_water_dirs": (C.c_int, [vp, vp, i64]),
        "ppgpu_water_routes_host": (C.c_int, [vp, i64, vp, u32, i32, vp, vp]),
        "ppgpu_last_water_route_timing": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(dbl)]),
        "ppgpu_dense_edge_count": (i64, [i32, i64, u32]),
        "ppgpu_best_edge": (C.c_int, [vp, i64, vp, i32, u64, vp]),
        "ppgpu_key_min": (C.c_int, [vp, i32, vp, vp]),
        "ppgpu_allreduce_best": (C.c_int, [vp, vp, vp]),
        "ppgpu_comm_unique_id": (C.c_int, [vp]),
        "ppgpu_comm_init_rank": (C.c_int, [vp, i32, i32, vp]),
        "ppgpu_comm_init_all": (C.c_int, [C.POINTER(vp), i32]),
        "ppgpu_comm_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "ppgpu_comm_destroy": (C.c_int, [vp]),
        "ppgpu_comm_abort": (C.c_int, [vp]),
    }
    # measurement aids an older build of the library may lack (tools/ab_libs.sh loads the parent commit's): calling one there raises
    optional = {"ppgpu_last_swept_edges", "ppgpu_last_slices", "ppgpu_last_stop_members", "ppgpu_last_arc_stops_timing"}
    for name, (res, args) in sig.items():
        if name in optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)   # AttributeError here = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    return lib, list(sig)


LIB, EXPORTS = _load()


def keepout_limit2(res, margin):
    """limit2 of a margin in metres at a resolution (ppgpu_keepout_limit2: no handle, no device)."""
    k = C.c_uint32()
    rc = LIB.ppgpu_keepout_limit2(float(res), float(margin), C.byref(k))
    if rc != 0:
        raise PpgpuError(f"ppgpu_keepout_limit2 failed ({rc}): {LIB.ppgpu_last_error().decode()}")
    return k.value


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    return int(a)   # raw device pointer (e.g. torch.Tensor.data_ptr())


class Context:
    """One ppgpu_ctx.  Methods mirror the C entry points one to one."""

    def __init__(self, device=0):
        h = C.c_void_p()
        rc = LIB.ppgpu_create(device, C.byref(h))
        if rc != 0:
            raise PpgpuError(f"ppgpu_create: {LIB.ppgpu_last_error().decode()}")
        self._h = h

    def _ck(self, rc, what):
        if rc != 0:
            raise PpgpuError(f"{what} failed ({rc}): {LIB.ppgpu_last_error().decode()}")

    def close(self):
        if self._h:
            LIB.ppgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        self._ck(LIB.ppgpu_set_stream(self._h, stream_ptr), "ppgpu_set_stream")

    def enable_timing(self, on=True):
        self._ck(LIB.ppgpu_enable_timing(self._h, 1 if on else 0), "ppgpu_enable_timing")

    def last_timing(self):
        """(solve, pose sweep, cover sweep, heuristic) kernel durations in ms of the last costing launch."""
        t = [C.c_double() for _ in range(4)]
        self._ck(LIB.ppgpu_last_timing(self._h, *[C.byref(x) for x in t]), "ppgpu_last_timing")
        return tuple(x.value for x in t)

    def past_timing(self, back):
        """The same for the launch `back` launches ago (0 = the last one, at most 7)."""
        t = [C.c_double() for _ in range(4)]
        self._ck(LIB.ppgpu_past_timing(self._h, back, *[C.byref(x) for x in t]), "ppgpu_past_timing")
        return tuple(x.value for x in t)

    def last_cover_edges(self):
        """Edges of the last costing launch that pp_k_cover_sweep visited (the others were finished by the approach prepass)."""
        n = C.c_int64()
        self._ck(LIB.ppgpu_last_cover_edges(self._h, C.byref(n)), "ppgpu_last_cover_edges")
        return n.value

    def last_shared_edges(self):
        """Edges of the last costing launch that were not swept themselves but took the results of another edge of their class."""
        n = C.c_int64()
        self._ck(LIB.ppgpu_last_shared_edges(self._h, C.byref(n)), "ppgpu_last_shared_edges")
        return n.value

    def last_swept_edges(self):
        """Edges of the last costing launch on its sweep list (the ones the skip planner and the pose sweep walked); every edge of a
        launch without a list."""
        n = C.c_int64()
        self._ck(LIB.ppgpu_last_swept_edges(self._h, C.byref(n)), "ppgpu_last_swept_edges")
        return n.value

    def last_stop_members(self):
        """Edges of the last costing launch that took their track from the head of their stop class (PPGPU_SHARE_TRACKS); they count
        as swept edges, not as shared ones."""
        n = C.c_int64()
        self._ck(LIB.ppgpu_last_stop_members(self._h, C.byref(n)), "ppgpu_last_stop_members")
        return n.value

    def last_arc_stops_timing(self):
        """Milliseconds of the last timed pp_k_arc_stops (enable_timing, then a launch after new vertices, grid, keep-out or config)."""
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_arc_stops_timing(self._h, C.byref(ms)), "ppgpu_last_arc_stops_timing")
        return ms.value

    def last_slices(self):
        """(workspace slices the last costing launch ran as, edges of the last one)."""
        n, last = C.c_int64(), C.c_int64()
        self._ck(LIB.ppgpu_last_slices(self._h, C.byref(n), C.byref(last)), "ppgpu_last_slices")
        return n.value, last.value

    def reserve_samples(self, max_samples, max_vertices=16):
        self._ck(LIB.ppgpu_reserve_samples(self._h, max_samples, max_vertices), "ppgpu_reserve_samples")

    def synchronize(self):
        self._ck(LIB.ppgpu_synchronize(self._h), "ppgpu_synchronize")

    def set_config(self, cfg):
        self.cfg = cfg
        self._ck(LIB.ppgpu_set_config(self._h, C.byref(cfg)), "ppgpu_set_config")

    def set_grid(self, cells, resolution):
        if cells is None:
            self._ck(LIB.ppgpu_set_grid(self._h, None, 0, 0, 0.0), "ppgpu_set_grid")
            return
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        self._ck(LIB.ppgpu_set_grid(self._h, _ptr(cells), cells.shape[0], cells.shape[1], float(resolution)), "ppgpu_set_grid")

    def get_grid_clearance(self, rows, cols):
        """The device's clearance map of the grid last set (rows x cols bytes); for tests and tools."""
        out = np.zeros((rows, cols), dtype=np.uint8)
        self._ck(LIB.ppgpu_get_grid_clearance(self._h, _ptr(out), out.size), "ppgpu_get_grid_clearance")
        return out

    def set_obstacles(self, obst7, model=1):
        if obst7 is None or len(obst7) == 0:
            self._ck(LIB.ppgpu_set_obstacles(self._h, 0, 0, None), "ppgpu_set_obstacles")
            return
        o = np.ascontiguousarray(obst7, dtype=np.float64).reshape(-1, 7)
        self._ck(LIB.ppgpu_set_obstacles(self._h, model, o.shape[0], _ptr(o)), "ppgpu_set_obstacles")

    def set_gaussian_obstacles(self, rows):
        """rows: n x 5 {x, y, heading, speed, time} (default covariance) or n x 9 (+ row-major 2x2 covariance)."""
        o = np.ascontiguousarray(rows, dtype=np.float64)
        if o.size == 0:
            self._ck(LIB.ppgpu_set_gaussian_obstacles(self._h, 0, None, 0), "ppgpu_set_gaussian_obstacles")
            return
        assert o.ndim == 2 and o.shape[1] in (5, 9)
        self._ck(LIB.ppgpu_set_gaussian_obstacles(self._h, o.shape[0], _ptr(o), 1 if o.shape[1] == 9 else 0), "ppgpu_set_gaussian_obstacles")

    def set_vertices(self, vertices, ribbons4):
        v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        r = np.ascontiguousarray(ribbons4, dtype=np.float64).reshape(-1, 4)
        self._ck(LIB.ppgpu_set_vertices(self._h, v.shape[0], _ptr(v), r.shape[0], _ptr(r) if r.shape[0] else None),
                 "ppgpu_set_vertices")

    def sampler_init(self, bounds6, seed, ribbons4=None):
        b = np.ascontiguousarray(bounds6, dtype=np.float64)
        if ribbons4 is None:
            self._ck(LIB.ppgpu_sampler_init(self._h, _ptr(b), int(seed), -1, None), "ppgpu_sampler_init")
        else:
            r = np.ascontiguousarray(ribbons4, dtype=np.float64).reshape(-1, 4)
            self._ck(LIB.ppgpu_sampler_init(self._h, _ptr(b), int(seed), r.shape[0], _ptr(r) if r.shape[0] else None),
                     "ppgpu_sampler_init")

    def sampler_add(self, n_attempts):
        tot = C.c_int64()
        self._ck(LIB.ppgpu_sampler_add(self._h, int(n_attempts), C.byref(tot)), "ppgpu_sampler_add")
        return tot.value

    def copy_engine_read(self, h_pinned_ptr, d_ptr, nbytes):
        self._ck(LIB.ppgpu_copy_engine_read(self._h, int(h_pinned_ptr), int(d_ptr), int(nbytes)), "ppgpu_copy_engine_read")

    def copy_engine_wait(self):
        self._ck(LIB.ppgpu_copy_engine_wait(self._h), "ppgpu_copy_engine_wait")

    def growth_stats(self):
        n, sec = C.c_uint64(), C.c_double()
        self._ck(LIB.ppgpu_growth_stats(self._h, C.byref(n), C.byref(sec)), "ppgpu_growth_stats")
        return int(n.value), float(sec.value)

    def sampler_skip(self, n_attempts):
        self._ck(LIB.ppgpu_sampler_skip(self._h, int(n_attempts)), "ppgpu_sampler_skip")

    def set_samples(self, x, y, heading):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        h = np.ascontiguousarray(heading, dtype=np.float64)
        self._ck(LIB.ppgpu_set_samples(self._h, x.shape[0], _ptr(x), _ptr(y), _ptr(h)), "ppgpu_set_samples")

    def num_samples(self):
        return LIB.ppgpu_num_samples(self._h)

    def get_samples(self, first=0, n=None):
        if n is None:
            n = self.num_samples() - first
        out = np.zeros((n, 5), dtype=np.float64)
        self._ck(LIB.ppgpu_get_samples(self._h, first, n, _ptr(out)), "ppgpu_get_samples")
        return out

    def dubins_lengths(self, v0, nv, d_lengths):
        self._ck(LIB.ppgpu_dubins_lengths(self._h, v0, nv, _ptr(d_lengths)), "ppgpu_dubins_lengths")

    def set_extra_targets(self, x, y, heading):
        """Explicit (non-sample) targets; returns the index of the first one for edge descriptors."""
        x, y, heading = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, heading)]
        first = C.c_int64(0)
        self._ck(LIB.ppgpu_set_extra_targets(self._h, x.shape[0], _ptr(x) if x.shape[0] else None, _ptr(y) if x.shape[0] else None,
                                             _ptr(heading) if x.shape[0] else None, C.byref(first)), "ppgpu_set_extra_targets")
        return int(first.value)

    def select_nearest(self, v0, nv, k):
        idx = np.zeros((nv, 2, k), dtype=np.int32)
        ln = np.zeros((nv, 2, k), dtype=np.float64)
        self._ck(LIB.ppgpu_select_nearest(self._h, v0, nv, k, _ptr(idx), _ptr(ln)), "ppgpu_select_nearest")
        return idx, ln

    def expand_order(self, nv, k):
        """The k winners per (vertex, radius) in the order expand() pushes them (the reference's heap array); (idx, fallbacks)."""
        idx = np.zeros((nv, 2, k), dtype=np.int32)
        fb = C.c_uint32(0)
        self._ck(LIB.ppgpu_expand_order(self._h, 0, nv, k, _ptr(idx), C.byref(fb)), "ppgpu_expand_order")
        return idx, int(fb.value)

    def order_fallbacks(self):
        return int(LIB.ppgpu_order_fallbacks(self._h))

    def cost_edges_dense(self, v0, nv, s0, ns, cfg_mask, d_results, d_child=None, stride=0):
        self._ck(LIB.ppgpu_cost_edges_dense(self._h, v0, nv, s0, ns, cfg_mask, _ptr(d_results), _ptr(d_child), stride),
                 "ppgpu_cost_edges_dense")

    def cost_edges_list(self, n, d_edges, d_results, d_child=None, stride=0):
        self._ck(LIB.ppgpu_cost_edges_list(self._h, n, _ptr(d_edges), _ptr(d_results), _ptr(d_child), stride),
                 "ppgpu_cost_edges_list")

    def heuristic_host(self, poses3, ribbon_lists):
        """h of each pose {x, y, heading} with its own ribbon list (Vertex::computeApproxToGo); returns (h, flags)."""
        ps = np.ascontiguousarray(poses3, dtype=np.float64).reshape(-1, 3)
        counts = np.array([len(r) for r in ribbon_lists], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 4) for r in ribbon_lists]) if counts.sum() else np.zeros((0, 4)))
        out = np.zeros(len(ps), dtype=np.float64)
        fl = np.zeros(len(ps), dtype=np.uint32)
        self._ck(LIB.ppgpu_heuristic_host(self._h, len(ps), _ptr(ps), _ptr(counts), _ptr(flat) if len(flat) else None, _ptr(out), _ptr(fl)), "ppgpu_heuristic_host")
        return out, fl

    def set_tsp_table(self, min_ribbons, max_ribbons):
        """The exact-table pass over child lists of min_ribbons .. max_ribbons (<= 16) ribbons; min_ribbons = 0: the lists the
        enumeration declines; max_ribbons = 0: off (the default)."""
        self._ck(LIB.ppgpu_set_tsp_table(self._h, int(min_ribbons), int(max_ribbons)), "ppgpu_set_tsp_table")

    def set_dubins_tsp_table(self, min_ribbons, max_ribbons):
        """The same pass for the Dubins-TSP heuristics (3, 4): a switch of its own, same arguments, shared workspace and counters."""
        self._ck(LIB.ppgpu_set_dubins_tsp_table(self._h, int(min_ribbons), int(max_ribbons)), "ppgpu_set_dubins_tsp_table")

    def tsp_table_stats(self):
        """(lists the table pass answered, lists it refused for a tie) on this handle so far."""
        lists, refused = C.c_uint64(), C.c_uint64()
        self._ck(LIB.ppgpu_tsp_table_stats(self._h, C.byref(lists), C.byref(refused)), "ppgpu_tsp_table_stats")
        return int(lists.value), int(refused.value)

    def last_tsp_table_timing(self):
        """Device milliseconds of the last table pass (enable_timing first)."""
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_tsp_table_timing(self._h, C.byref(ms)), "ppgpu_last_tsp_table_timing")
        return float(ms.value)

    def expand_host(self, vertices, ribbons4, nearest3, k, stride=0):
        """SamplingBasedPlanner::expand for several vertices in one round trip: (descriptors, records, child ribbons)."""
        v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        r = np.ascontiguousarray(ribbons4, dtype=np.float64).reshape(-1, 4)
        nz = np.ascontiguousarray(nearest3, dtype=np.float64).reshape(-1, 3)
        cap = int(LIB.ppgpu_expand_capacity(v.shape[0], k))
        e = np.zeros(cap, dtype=np.uint64)
        res = np.zeros(cap, dtype=RESULT_DTYPE)
        child = np.zeros((cap, stride, 4), dtype=np.float64) if stride > 0 else None
        n = C.c_int64(0)
        self._ck(LIB.ppgpu_expand_host(self._h, v.shape[0], _ptr(v), r.shape[0], _ptr(r) if r.shape[0] else None, _ptr(nz), k, C.byref(n),
                                       _ptr(e), _ptr(res), _ptr(child), stride), "ppgpu_expand_host")
        m = n.value
        return e[:m], res[:m], (child[:m] if child is not None else None)

    def cost_edges_host(self, edges, stride=0):
        e = np.ascontiguousarray(edges, dtype=np.uint64)
        res = np.zeros(e.shape[0], dtype=RESULT_DTYPE)
        child = np.zeros((e.shape[0], stride, 4), dtype=np.float64) if stride > 0 else None
        self._ck(LIB.ppgpu_cost_edges_host(self._h, e.shape[0], _ptr(e), _ptr(res), _ptr(child), stride), "ppgpu_cost_edges_host")
        return (res, child) if stride > 0 else res

    def cost_wrapper_edges_host(self, wedges, stride=0):
        from .types import WRAPPER_EDGE_DTYPE
        e = np.ascontiguousarray(wedges, dtype=WRAPPER_EDGE_DTYPE)
        res = np.zeros(e.shape[0], dtype=RESULT_DTYPE)
        child = np.zeros((e.shape[0], stride, 4), dtype=np.float64) if stride > 0 else None
        self._ck(LIB.ppgpu_cost_wrapper_edges_host(self._h, e.shape[0], _ptr(e), _ptr(res), _ptr(child), stride), "ppgpu_cost_wrapper_edges_host")
        return (res, child) if stride > 0 else res

    def cost_plans(self, leg_offsets, legs, stride, results=None, child=None, want_child=True):
        """AStarPlanner.cpp:46-59 for many plans in one call (ppgpu_cost_plans_host): plan p is legs[leg_offsets[p]:leg_offsets[p + 1]],
        each leg's .vertex its plan's start vertex.  Returns (records, child ribbons or None, legs_costed, stop codes); `results` /
        `child`: arrays to write into (the slots of legs that were not costed are left as they are), zeroed ones by default."""
        from .types import WRAPPER_EDGE_DTYPE
        off = np.ascontiguousarray(leg_offsets, dtype=np.int32)
        e = np.ascontiguousarray(legs, dtype=WRAPPER_EDGE_DTYPE)
        n_plans = off.shape[0] - 1
        assert n_plans >= 0 and (n_plans == 0 or int(off[-1]) <= e.shape[0])
        if results is None:
            results = np.zeros(e.shape[0], dtype=RESULT_DTYPE)
        if child is None and want_child:
            child = np.zeros((e.shape[0], stride, 4), dtype=np.float64)
        assert results.dtype == RESULT_DTYPE and results.shape == (e.shape[0],) and results.flags["C_CONTIGUOUS"]
        assert child is None or (child.dtype == np.float64 and child.shape == (e.shape[0], stride, 4) and child.flags["C_CONTIGUOUS"])
        costed = np.zeros(n_plans, dtype=np.int32)
        stop = np.zeros(n_plans, dtype=np.uint32)
        self._ck(LIB.ppgpu_cost_plans_host(self._h, n_plans, _ptr(off), _ptr(e) if e.shape[0] else None, _ptr(results) if e.shape[0] else None,
                                           _ptr(child) if child is not None and e.shape[0] else None, stride, _ptr(costed), _ptr(stop)),
                 "ppgpu_cost_plans_host")
        return results, child, costed, stop

    def trace_edges_list(self, n, d_edges, d_results, step_stride, d_counts, d_steps):
        self._ck(LIB.ppgpu_trace_edges_list(self._h, n, _ptr(d_edges), _ptr(d_results), step_stride, _ptr(d_counts), _ptr(d_steps)),
                 "ppgpu_trace_edges_list")

    def _trace_records_host(self, fn, name, e, records, dtype, per_edge, before=(), after=(), none_when_empty=False):
        """The host form `fn` of a trace over the list e: (records as cost_edges_host returns them, step counts, records[n, per_edge]).
        `records`: an array to write into, a zeroed one by default.  before / after: what fn takes ahead of the counts and behind the records."""
        n = e.shape[0]
        res = np.zeros(n, dtype=RESULT_DTYPE)
        counts = np.zeros(n, dtype=np.int32)
        if records is None:
            records = np.zeros((n, per_edge), dtype=dtype)
        assert records.dtype == dtype and records.shape == (n, per_edge) and records.flags["C_CONTIGUOUS"]
        self._ck(fn(self._h, n, _ptr(e), _ptr(res), *before, _ptr(counts), _ptr(records) if records.size or not none_when_empty else None, *after), name)
        return res, counts, records

    def _trace_host(self, fn, name, e, step_stride, steps):
        from .types import STEP_DTYPE
        return self._trace_records_host(fn, name, e, steps, STEP_DTYPE, step_stride, before=(step_stride,))

    def trace_edges(self, edges, step_stride, steps=None):
        """Edge::computeTrueCost step by step: (records as cost_edges_host returns them, step counts, steps[n, step_stride]).
        `steps`: an array to write into (entries beyond an edge's count are left as they are); a zeroed one by default."""
        e = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._trace_host(LIB.ppgpu_trace_edges_host, "ppgpu_trace_edges_host", e, step_stride, steps)

    def trace_wrapper_edges(self, wedges, step_stride, steps=None):
        from .types import WRAPPER_EDGE_DTYPE
        e = np.ascontiguousarray(wedges, dtype=WRAPPER_EDGE_DTYPE)
        return self._trace_host(LIB.ppgpu_trace_wrapper_edges_host, "ppgpu_trace_wrapper_edges_host", e, step_stride, steps)

    def last_trace_timing(self):
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_trace_timing(self._h, C.byref(ms)), "ppgpu_last_trace_timing")
        return ms.value

    def trace_cover_list(self, n, d_edges, d_results, step_stride, d_counts, d_cover, d_summaries, d_child=None, ribbon_stride=0):
        self._ck(LIB.ppgpu_trace_cover_list(self._h, n, _ptr(d_edges), _ptr(d_results), step_stride, _ptr(d_counts), _ptr(d_cover),
                                            _ptr(d_summaries), _ptr(d_child), ribbon_stride), "ppgpu_trace_cover_list")

    def _trace_cover_host(self, fn, name, e, step_stride, cover, ribbon_stride):
        from .types import COVER_DTYPE, COVER_SUMMARY_DTYPE
        n = e.shape[0]
        summaries = np.zeros(n, dtype=COVER_SUMMARY_DTYPE)
        child = np.zeros((n, ribbon_stride, 4), dtype=np.float64) if ribbon_stride > 0 else None
        res, counts, cover = self._trace_records_host(fn, name, e, cover, COVER_DTYPE, step_stride, before=(step_stride,),
                                                      after=(_ptr(summaries), _ptr(child), ribbon_stride))
        return res, counts, cover, summaries, child

    def trace_cover(self, edges, step_stride, cover=None, ribbon_stride=0):
        """The coverage branch of Edge::computeTrueCost step by step: (records as cost_edges_host returns them, step counts,
        cover[n, step_stride], summaries, final lists [n, ribbon_stride, 4] or None).  `cover`: an array to write into (entries
        beyond an edge's count are left as they are); a zeroed one by default."""
        e = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._trace_cover_host(LIB.ppgpu_trace_cover_host, "ppgpu_trace_cover_host", e, step_stride, cover, ribbon_stride)

    def trace_cover_wrapper_edges(self, wedges, step_stride, cover=None, ribbon_stride=0):
        from .types import WRAPPER_EDGE_DTYPE
        e = np.ascontiguousarray(wedges, dtype=WRAPPER_EDGE_DTYPE)
        return self._trace_cover_host(LIB.ppgpu_trace_cover_wrapper_edges_host, "ppgpu_trace_cover_wrapper_edges_host", e, step_stride,
                                      cover, ribbon_stride)

    def last_cover_trace_timing(self):
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_cover_trace_timing(self._h, C.byref(ms)), "ppgpu_last_cover_trace_timing")
        return ms.value

    def obstacle_count(self):
        """(rows, model) of the handle's obstacle table: what sizes a contacts array."""
        n, model = C.c_int32(), C.c_int32()
        self._ck(LIB.ppgpu_obstacle_count(self._h, C.byref(n), C.byref(model)), "ppgpu_obstacle_count")
        return n.value, model.value

    def trace_contacts_list(self, n, d_edges, d_results, d_counts, d_contacts):
        self._ck(LIB.ppgpu_trace_contacts_list(self._h, n, _ptr(d_edges), _ptr(d_results), _ptr(d_counts), _ptr(d_contacts)),
                 "ppgpu_trace_contacts_list")

    def _trace_contacts_host(self, fn, name, e, contacts):
        from .types import CONTACT_DTYPE
        # (without obstacles there is no record to hand over)
        return self._trace_records_host(fn, name, e, contacts, CONTACT_DTYPE, self.obstacle_count()[0], none_when_empty=True)

    def trace_contacts(self, edges, contacts=None):
        """Edge::computeTrueCost contact by contact: (records as cost_edges_host returns them, step counts, contacts[n, n_obst]).
        `contacts`: an array to write into; a zeroed one by default."""
        e = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._trace_contacts_host(LIB.ppgpu_trace_contacts_host, "ppgpu_trace_contacts_host", e, contacts)

    def trace_contacts_wrapper_edges(self, wedges, contacts=None):
        from .types import WRAPPER_EDGE_DTYPE
        e = np.ascontiguousarray(wedges, dtype=WRAPPER_EDGE_DTYPE)
        return self._trace_contacts_host(LIB.ppgpu_trace_contacts_wrapper_edges_host, "ppgpu_trace_contacts_wrapper_edges_host", e, contacts)

    def last_contact_trace_timing(self):
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_contact_trace_timing(self._h, C.byref(ms)), "ppgpu_last_contact_trace_timing")
        return ms.value

    def get_grid_distance(self, rows, cols):
        """The device's distance map of the grid last set: min(gap2, DIST_CAP2) per cell, rows x cols uint16; for tests and tools."""
        out = np.zeros((rows, cols), dtype=np.uint16)
        self._ck(LIB.ppgpu_get_grid_distance(self._h, _ptr(out), out.size), "ppgpu_get_grid_distance")
        return out

    def grid_clearance_at(self, xy):
        """(clearance in metres, gap2 in cells squared) of the cells the points xy[n, 2] lie in: the certified lower bound."""
        p = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        clearance = np.zeros(p.shape[0], dtype=np.float64)
        gap2 = np.zeros(p.shape[0], dtype=np.uint32)
        self._ck(LIB.ppgpu_grid_clearance_at(self._h, p.shape[0], _ptr(p), _ptr(clearance), _ptr(gap2)), "ppgpu_grid_clearance_at")
        return clearance, gap2

    def last_grid_distance_timing(self):
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_grid_distance_timing(self._h, C.byref(ms)), "ppgpu_last_grid_distance_timing")
        return ms.value

    def trace_clearance_list(self, n, d_edges, d_results, d_counts, d_clearance, margin=0.0):
        self._ck(LIB.ppgpu_trace_clearance_list(self._h, n, _ptr(d_edges), _ptr(d_results), _ptr(d_counts), _ptr(d_clearance), float(margin)),
                 "ppgpu_trace_clearance_list")

    def _trace_clearance_host(self, fn, name, e, margin, records):
        from .types import CLEARANCE_DTYPE
        if records is not None:
            records = records.reshape(-1, 1)
        res, counts, records = self._trace_records_host(fn, name, e, records, CLEARANCE_DTYPE, 1, after=(float(margin),))
        return res, counts, records.reshape(-1)

    def trace_clearance(self, edges, margin=0.0, records=None):
        """How close each edge comes to a charted hazard: (records as cost_edges_host returns them, step counts, clearance[n]).
        `records`: an array to write into (every record is written); a zeroed one by default."""
        e = np.ascontiguousarray(edges, dtype=np.uint64)
        return self._trace_clearance_host(LIB.ppgpu_trace_clearance_host, "ppgpu_trace_clearance_host", e, margin, records)

    def trace_clearance_wrapper_edges(self, wedges, margin=0.0, records=None):
        from .types import WRAPPER_EDGE_DTYPE
        e = np.ascontiguousarray(wedges, dtype=WRAPPER_EDGE_DTYPE)
        return self._trace_clearance_host(LIB.ppgpu_trace_clearance_wrapper_edges_host, "ppgpu_trace_clearance_wrapper_edges_host", e, margin, records)

    def last_clearance_trace_timing(self):
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_clearance_trace_timing(self._h, C.byref(ms)), "ppgpu_last_clearance_trace_timing")
        return ms.value

    def set_keepout_limit2(self, limit2):
        """Plan on the effective grid: a cell is blocked iff its gap2 < limit2 (0: the grid as set)."""
        self._ck(LIB.ppgpu_set_keepout_limit2(self._h, int(limit2)), "ppgpu_set_keepout_limit2")

    def get_keepout_limit2(self):
        k = C.c_uint32()
        self._ck(LIB.ppgpu_get_keepout_limit2(self._h, C.byref(k)), "ppgpu_get_keepout_limit2")
        return k.value

    def get_grid_blocked(self, rows, cols):
        """The effective grid the launches read, rows x cols bytes of 0/1; for tests and tools."""
        out = np.zeros((rows, cols), dtype=np.uint8)
        self._ck(LIB.ppgpu_get_grid_blocked(self._h, _ptr(out), out.size), "ppgpu_get_grid_blocked")
        return out

    def last_keepout_timing(self):
        ms = C.c_double()
        self._ck(LIB.ppgpu_last_keepout_timing(self._h, C.byref(ms)), "ppgpu_last_keepout_timing")
        return ms.value

    # ---- reachable water: which cells a plan from a seed can get to, and which ribbons lie beyond them
    def get_grid_labels(self, rows, cols):
        """The canonical 8-connected component labels of the effective grid, rows x cols uint32 (REACH_NONE on a blocked cell):
        the smallest row-major cell index of each component; for tests and tools.  Built on first use."""
        out = np.zeros((rows, cols), dtype=np.uint32)
        self._ck(LIB.ppgpu_get_grid_labels(self._h, _ptr(out), out.size), "ppgpu_get_grid_labels")
        return out

    def set_reach_seed(self, x, y):
        """The pose whose component is the reach set; returns the REACH_INFO_DTYPE block (flags: REACH_SEED_BLOCKED, REACH_NO_MAP)."""
        from .types import REACH_INFO_DTYPE
        info = np.zeros(1, dtype=REACH_INFO_DTYPE)
        self._ck(LIB.ppgpu_set_reach_seed(self._h, float(x), float(y), _ptr(info)), "ppgpu_set_reach_seed")
        return info[0]

    def get_grid_reach_gap(self, rows, cols):
        """min(rgap2, DIST_CAP2) per cell, rows x cols uint16: the squared gap in cells to the nearest cell of the current seed's reach
        set (0 on the set and beside it); for tests and tools."""
        out = np.zeros((rows, cols), dtype=np.uint16)
        self._ck(LIB.ppgpu_get_grid_reach_gap(self._h, _ptr(out), out.size), "ppgpu_get_grid_reach_gap")
        return out

    def ribbon_reach(self, ribbons4, ribbon_width):
        """One RIBBON_REACH_DTYPE record per ribbon {sx, sy, ex, ey}: how much of it no pose in the reach set can cover.  A sample
        that is not OUT proves nothing (the turning radius may still prevent coverage)."""
        from .types import RIBBON_REACH_DTYPE
        rb = np.ascontiguousarray(ribbons4, dtype=np.float64).reshape(-1, 4)
        out = np.zeros(rb.shape[0], dtype=RIBBON_REACH_DTYPE)
        self._ck(LIB.ppgpu_ribbon_reach_host(self._h, rb.shape[0], _ptr(rb), float(ribbon_width), _ptr(out)), "ppgpu_ribbon_reach_host")
        return out

    def last_reach_timing(self):
        """(labels, reach set and gap map, ribbon walk) device milliseconds of the last of each, -1 where none was timed since
        enable_timing."""
        t = [C.c_double() for _ in range(3)]
        self._ck(LIB.ppgpu_last_reach_timing(self._h, *[C.byref(x) for x in t]), "ppgpu_last_reach_timing")
        return tuple(x.value for x in t)

    # ---- distance by water: how far it is through free cells from a seed to every cell, and to every ribbon
    def set_water_seed(self, x, y):
        """The pose the distances are measured from; returns the WATER_INFO_DTYPE block (flags: WATER_SEED_BLOCKED, WATER_NO_MAP).
        Builds the map unless the cached one is that of the seed's cell."""
        from .types import WATER_INFO_DTYPE
        info = np.zeros(1, dtype=WATER_INFO_DTYPE)
        self._ck(LIB.ppgpu_set_water_seed(self._h, float(x), float(y), _ptr(info)), "ppgpu_set_water_seed")
        return info[0]

    def get_grid_water(self, rows, cols):
        """wd per cell, rows x cols uint32: the cost of the cheapest 8-connected path from the seed's cell (12 per row or column
        step, 17 per diagonal step), WATER_NONE on blocked cells and other components; for tests and tools."""
        out = np.zeros((rows, cols), dtype=np.uint32)
        self._ck(LIB.ppgpu_get_grid_water(self._h, _ptr(out), out.size), "ppgpu_get_grid_water")
        return out

    def water_distance_at(self, xy):
        """(metres, wd) of the map at n points {x, y}: resolution * wd / 12 and wd; +inf and WATER_NONE where there is no distance or
        the point is outside the grid."""
        pts = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        metres, wd = np.zeros(pts.shape[0], dtype=np.float64), np.zeros(pts.shape[0], dtype=np.uint32)
        self._ck(LIB.ppgpu_water_distance_at(self._h, pts.shape[0], _ptr(pts), _ptr(metres), _ptr(wd)), "ppgpu_water_distance_at")
        return metres, wd

    def ribbon_water(self, ribbons4, ribbon_width):
        """One RIBBON_WATER_DTYPE record per ribbon {sx, sy, ex, ey}: how far by water the nearest and the farthest of its samples can
        be approached.  An upper bound on a route through cell centres, not a lower bound on what a Dubins vehicle travels."""
        from .types import RIBBON_WATER_DTYPE
        rb = np.ascontiguousarray(ribbons4, dtype=np.float64).reshape(-1, 4)
        out = np.zeros(rb.shape[0], dtype=RIBBON_WATER_DTYPE)
        self._ck(LIB.ppgpu_ribbon_water_host(self._h, rb.shape[0], _ptr(rb), float(ribbon_width), _ptr(out)), "ppgpu_ribbon_water_host")
        return out

    def last_water_timing(self):
        """(map build, ribbon walk) device milliseconds of the last of each, -1 where none was timed since enable_timing."""
        t = [C.c_double() for _ in range(2)]
        self._ck(LIB.ppgpu_last_water_timing(self._h, *[C.byref(x) for x in t]), "ppgpu_last_water_timing")
        return tuple(x.value for x in t)

    # ---- route by water: which way the distance by water goes, per query point
    def get_grid_water_dirs(self, rows, cols):
        """dir per cell, rows x cols uint8: the code of the step towards the seed (0..7 = N, S, W, E, NW, NE, SW, SE; the lowest
        code on a tie), ROUTE_SEED on the seed's cell, ROUTE_NONE where there is no distance; for tests and tools."""
        out = np.zeros((rows, cols), dtype=np.uint8)
        self._ck(LIB.ppgpu_get_grid_water_dirs(self._h, _ptr(out), out.size), "ppgpu_get_grid_water_dirs")
        return out

    def water_routes(self, xy, lim2=0, vertex_stride=0, vertices=None):
        """(records, vertices): one WATER_ROUTE_DTYPE record per point {x, y} and an (n, vertex_stride) uint32 array whose row i holds
        the first vertices_written vertices of route i, the seed's cell first.  `vertices`: an array to write into (its other slots
        are left as they were); a new one, filled with WATER_NONE, otherwise."""
        from .types import WATER_ROUTE_DTYPE, WATER_NONE
        pts = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n, stride = pts.shape[0], int(vertex_stride)
        recs = np.zeros(n, dtype=WATER_ROUTE_DTYPE)
        if vertices is None:
            vertices = np.full((n, max(stride, 0)), WATER_NONE, dtype=np.uint32)
        assert vertices.dtype == np.uint32 and vertices.flags.c_contiguous and vertices.size >= n * max(stride, 0)
        self._ck(LIB.ppgpu_water_routes_host(self._h, n, _ptr(pts), int(lim2), stride, _ptr(recs), _ptr(vertices) if stride > 0 else None),
                 "ppgpu_water_routes_host")
        return recs, vertices

    def last_water_route_timing(self):
        """(step map build, route walk) device milliseconds of the last of each, -1 where none was timed since enable_timing."""
        t = [C.c_double() for _ in range(2)]
        self._ck(LIB.ppgpu_last_water_route_timing(self._h, *[C.byref(x) for x in t]), "ppgpu_last_water_route_timing")
        return tuple(x.value for x in t)

    @staticmethod
    def dense_edge_count(nv, ns, cfg_mask):
        return LIB.ppgpu_dense_edge_count(nv, ns, cfg_mask)

    def best_edge(self, n, d_results, d_key2, goal_only=False, base=0):
        self._ck(LIB.ppgpu_best_edge(self._h, n, _ptr(d_results), 1 if goal_only else 0, base, _ptr(d_key2)), "ppgpu_best_edge")

    def key_min(self, n, d_keys, d_key2):
        self._ck(LIB.ppgpu_key_min(self._h, n, _ptr(d_keys), _ptr(d_key2)), "ppgpu_key_min")

    # ---- the communicator of a sharded iteration (RCCL, loaded by the library at the first call)
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from ncclGetUniqueId: rank 0 makes them, every rank passes them to comm_init_rank."""
        buf = (C.c_uint8 * 128)()
        rc = LIB.ppgpu_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise PpgpuError(f"ppgpu_comm_unique_id failed ({rc}): {LIB.ppgpu_last_error().decode()}")
        return bytes(buf)

    def comm_init_rank(self, world, rank, id128):
        assert len(id128) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(id128)
        self._ck(LIB.ppgpu_comm_init_rank(self._h, world, rank, C.cast(buf, C.c_void_p)), "ppgpu_comm_init_rank")

    def comm_info(self):
        """(ranks, this handle's rank) as RCCL reports them (ncclCommCount, ncclCommUserRank)."""
        w, r = C.c_int32(), C.c_int32()
        self._ck(LIB.ppgpu_comm_info(self._h, C.byref(w), C.byref(r)), "ppgpu_comm_info")
        return w.value, r.value

    def comm_destroy(self):
        self._ck(LIB.ppgpu_comm_destroy(self._h), "ppgpu_comm_destroy")

    def allreduce_best(self, d_key2, comm=None):
        """One collective per iteration: the global incumbent, in place on d_key2 (the handle's own communicator by default)."""
        self._ck(LIB.ppgpu_allreduce_best(self._h, comm, _ptr(d_key2)), "ppgpu_allreduce_best")
