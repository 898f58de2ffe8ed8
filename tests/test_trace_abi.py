"""The trace entry points exist at every layer that needs no GPU: declared in include/ppgpu.h, exported by libppgpu.so, bound in
path_planner_amd.api, and the step record's numpy mirror has the header's layout."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = ["ppgpu_trace_edges_list", "ppgpu_trace_edges_host", "ppgpu_trace_wrapper_edges_host"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppgpu.h")).read(), flags=re.S)


def test_header_declares_the_trace_entry_points():
    txt = _header()
    for name in TRACE:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name
    assert re.search(r"#define\s+PPGPU_S_BLOCKED\s+0x1u", txt) and re.search(r"#define\s+PPGPU_S_STRAIGHT\s+0x2u", txt)
    assert "typedef struct ppgpu_step_record" in txt


def test_library_exports_and_binding_has_them():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    for name in TRACE:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert getattr(api.LIB, name).restype is C.c_int
    assert callable(api.Context.trace_edges) and callable(api.Context.trace_wrapper_edges) and callable(api.Context.trace_edges_list)


def test_step_record_layout():
    from path_planner_amd.types import STEP_DTYPE, S_BLOCKED, S_STRAIGHT
    assert STEP_DTYPE.itemsize == 64
    off = {n: STEP_DTYPE.fields[n][1] for n in STEP_DTYPE.names}
    assert off == {"x": 0, "y": 8, "heading": 16, "time": 24, "collision": 32, "penalty_before": 40, "flags": 48, "step": 52, "reserved": 56}
    assert (S_BLOCKED, S_STRAIGHT) == (1, 2)
