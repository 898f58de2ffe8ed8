"""The coverage-trace entry points exist at every layer that needs no GPU — declared in include/ppgpu.h with the layout of their
numpy mirrors, exported by libppgpu.so, bound in path_planner_amd.api — and the recipe the GPU tests compare the device against
(tests/cover_replay.py) reproduces the oracle's own edge costing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = ["ppgpu_trace_cover_list", "ppgpu_trace_cover_host", "ppgpu_trace_cover_wrapper_edges_host", "ppgpu_last_cover_trace_timing"]
C_TYPES = {"double": ("<f8", 8), "uint32_t": ("<u4", 4), "int32_t": ("<i4", 4)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppgpu.h")).read(), flags=re.S)


def _struct_layout(txt, name):
    """[(field, numpy type, offset)] of `typedef struct name { ... } name;` (plain scalar fields, natural alignment), and its size."""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S).group(1)
    out, off, align = [], 0, 1
    for ctype, names in re.findall(r"(\w+)\s+([\w\s,]+);", body):
        np_type, size = C_TYPES[ctype]
        align = max(align, size)
        for field in [f.strip() for f in names.split(",")]:
            off = (off + size - 1) // size * size
            out.append((field, np_type, off))
            off += size
    return out, (off + align - 1) // align * align


def test_header_layout_equals_the_numpy_mirrors():
    from path_planner_amd import types as T
    txt = _header()
    for name in COVER:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name
    for struct, dtype in (("ppgpu_cover_record", T.COVER_DTYPE), ("ppgpu_cover_summary", T.COVER_SUMMARY_DTYPE)):
        fields, size = _struct_layout(txt, struct)
        assert size == dtype.itemsize and size % 16 == 0, (struct, size)
        assert [(n, dtype.fields[n][0].str, dtype.fields[n][1]) for n in dtype.names] == fields, struct
    for macro, value in (("PPGPU_C_EVENT", T.C_EVENT), ("PPGPU_C_COVER", T.C_COVER), ("PPGPU_C_CHANGED", T.C_CHANGED), ("PPGPU_C_DONE", T.C_DONE),
                         ("PPGPU_CS_LAST_COVER", T.CS_LAST_COVER), ("PPGPU_CS_LAST_CHANGED", T.CS_LAST_CHANGED), ("PPGPU_CS_DONE", T.CS_DONE),
                         ("PPGPU_CS_REFUSED", T.CS_REFUSED), ("PPGPU_CS_THROWS", T.CS_THROWS)):
        assert int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+)u" % macro, txt).group(1), 16) == value, macro


def test_library_exports_and_binding_has_them():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    for name in COVER:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert getattr(api.LIB, name).restype is C.c_int
    assert callable(api.Context.trace_cover) and callable(api.Context.trace_cover_wrapper_edges) and callable(api.Context.trace_cover_list)
    assert callable(api.Context.last_cover_trace_timing)


@pytest.mark.parametrize("name", ["coverage", "cfg2", "cfg3"])
def test_the_replay_reproduces_the_oracles_edge_costing(name):
    """The recipe pins itself: Edge.cpp:125-191 replayed with the oracle's primitives on the oracle's own poses gives the child
    lists of ppo_cost_edges bit for bit and coverage_completed_time exactly, on every edge of the world — and the worlds hold
    what the GPU tests need them to hold."""
    import cover_replay as cr
    from path_planner_amd.types import CS_DONE, F_DONE, F_THROWS
    tw = cr.cover_world(name)
    rec, child = tw.world.cost_edges(tw.verts, tw.pool, tw.sx, tw.sy, tw.sh, tw.edges, stride=64, threads=8)
    assert not np.any(rec["flags"] & F_THROWS)
    tot = dict(edges=len(tw.edges), steps=0, splits=0, trims=0, erasures=0, done_records=0, knife=0, long=0)
    for i, desc in enumerate(tw.edges):
        cov, rib0, cct0, vxy, vi = cr.edge_inputs(tw, desc)
        xs, ys, straight, blocked, times = cr.oracle_steps(tw, desc, rec[i])
        r = cr.replay_edge(tw.cfg, cov, rib0, cct0, xs, ys, straight, blocked, times, vxy)
        nr = int((rec["info"][i] >> 8) & 0xFF)
        assert len(r.final) == nr and np.array_equal(r.final, child[i, :nr]), (name, i)
        assert r.cct == rec["coverage_completed_time"][i], (name, i, r.cct, rec["coverage_completed_time"][i])
        assert bool(r.summary_flags & CS_DONE) == bool(rec["flags"][i] & F_DONE)
        # the countdown's decisions that lie within 1e-9 of toCover == increment (what a device may legitimately flip)
        before = np.concatenate([[0.0], r.to_cover[:-1]]) if len(xs) else np.zeros(0)
        tot["knife"] += int(np.count_nonzero(np.abs(before - tw.cfg.collision_checking_increment) <= cr.KNIFE_EPS))
        tot["steps"] += len(xs)
        tot["long"] += len(xs) > 64
        for key in ("splits", "trims", "erasures"):
            tot[key] += getattr(r, key)
        tot["done_records"] += bool(rec["flags"][i] & F_DONE)
    print(name, tot)
    assert tot["long"] >= 10
    if name == "coverage":
        assert tot["erasures"] >= 8 and tot["done_records"] >= 20
    if name == "cfg2":
        assert tot["splits"] >= 8
    if name == "cfg3":
        assert tot["splits"] >= 20 and tot["trims"] >= 2000
