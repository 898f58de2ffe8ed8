"""ppgpu_cost_plans_host exists at every layer that needs no GPU: declared in include/ppgpu.h with its stop codes, exported by
libppgpu.so, bound in path_planner_amd.api as Context.cost_plans, and the numpy mirrors it takes and fills have the header's layout."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {"LEGS": 1, "INFEASIBLE": 2, "GOAL": 3, "THROWS": 4, "CAPACITY": 5}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppgpu.h")).read(), flags=re.S)


def test_header_declares_the_entry_point_and_the_stop_codes():
    txt = _header()
    m = re.search(r"^int\s+ppgpu_cost_plans_host\s*\(([^;]*)\)\s*;", txt, flags=re.M)
    assert m, "ppgpu_cost_plans_host is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9, args
    assert args[0].startswith("ppgpu_ctx") and args[1].startswith("int32_t") and args[2].startswith("const int32_t")
    assert args[3].startswith("const ppgpu_wrapper_edge") and args[4].startswith("ppgpu_edge_result") and args[5].startswith("double")
    assert args[6].startswith("int32_t") and args[7].startswith("int32_t") and args[8].startswith("uint32_t")
    for name, value in CODES.items():
        assert re.search(r"#define\s+PPGPU_CHAIN_%s\s+%du\b" % (name, value), txt), name


def test_library_exports_and_binding_has_it():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    assert hasattr(lib, "ppgpu_cost_plans_host")
    assert "ppgpu_cost_plans_host" in api.EXPORTS
    fn = api.LIB.ppgpu_cost_plans_host
    assert fn.restype is C.c_int and len(fn.argtypes) == 9
    assert callable(api.Context.cost_plans)


def test_stop_codes_and_record_layouts():
    from path_planner_amd import types as T
    assert (T.CHAIN_LEGS, T.CHAIN_INFEASIBLE, T.CHAIN_GOAL, T.CHAIN_THROWS, T.CHAIN_CAPACITY) == (1, 2, 3, 4, 5)
    # what the call takes (96-byte wrapper edges, their .vertex the plan's start vertex) and what it fills (128-byte records)
    w = T.WRAPPER_EDGE_DTYPE
    assert w.itemsize == 96
    assert {n: w.fields[n][1] for n in w.names} == {"vertex": 0, "coverage_allowed": 4, "qi": 8, "param": 32, "rho": 56, "type": 64,
                                                     "reserved": 68, "speed": 72, "start_time": 80, "end_time": 88}
    r = T.RESULT_DTYPE
    assert r.itemsize == 128
    assert [r.fields[n][1] for n in ("flags", "info", "end_x", "end_time", "g", "coverage_completed_time")] == [0, 4, 32, 64, 72, 96]
    # the running vertex the device makes of a record is a ppgpu_vertex
    v = T.VERTEX_DTYPE
    assert v.itemsize == 64 and [v.fields[n][1] for n in ("time", "g", "coverage_completed_time", "ribbon_offset", "ribbon_count")] == [32, 40, 48, 56, 60]
