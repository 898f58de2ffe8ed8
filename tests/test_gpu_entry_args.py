"""-m gpu: what the costing, trace and plan-chain entry points refuse, with which code and which message — and that a refusal
leaves the handle as it was.

The smallest world there is: the base map (no grid), no obstacles, one open vertex with one ribbon, two explicit targets, lists of
two edges, step_stride 4.  Every refused call is refused on the host before anything is launched, so the device pointers handed
over are never read (they are valid allocations all the same).  The functions are called through api.LIB directly: the codes and
the texts of ppgpu_last_error() are the contract (the C++ host library forwards the texts into exceptions)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, EINVAL, ESTATE, ECAPACITY = 0, -1, -4, -5
STEP_STRIDE = 4
CHILD_STRIDE = 4
FILL = 0xA5

NO_VERTICES = "ppgpu_set_vertices must be called (after ppgpu_set_config)"
NO_TARGETS = "no targets: call ppgpu_sampler_add, ppgpu_set_samples or ppgpu_set_extra_targets"

COST_FORMS = ("cost_edges_list", "cost_edges_host", "cost_wrapper_edges_host")
TRACE_FORMS = ("trace_edges_list", "trace_edges_host", "trace_wrapper_edges_host")
WRAPPER_FORMS = ("cost_wrapper_edges_host", "trace_wrapper_edges_host", "cost_plans_host")
NEED_TARGETS = ("cost_edges_list", "cost_edges_host", "trace_edges_list", "trace_edges_host")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _vertex(**kw):
    from path_planner_amd.types import VERTEX_DTYPE
    v = np.zeros(1, dtype=VERTEX_DTYPE)
    v[0] = (0.0, 0.0, 0.0, 2.5, 0.0, 0.0, -1.0, 0, 1)
    for k, x in kw.items():
        v[k] = x
    return v


RIBBON = np.array([[0.0, 20.0, 0.0, 40.0]])
TARGETS = (np.array([30.0, -20.0]), np.array([40.0, 60.0]), np.array([0.5, 2.0]))


def _filled(n, dtype):
    return np.frombuffer(np.full(n * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).tobytes(), dtype=dtype).copy()


class Rig:
    """One handle and valid arguments for every entry point under test; `upto` = how far the world is set up."""

    def __init__(self, torch, upto="targets"):
        from path_planner_amd import api
        from path_planner_amd.types import RESULT_DTYPE, STEP_DTYPE, WRAPPER_EDGE_DTYPE, edge_pack, make_config
        self.api, self.torch = api, torch
        self.cfg = make_config()
        self.ctx = api.Context(0)
        self.ctx.set_config(self.cfg)
        self.ctx.set_grid(None, 0.0)
        self.ctx.set_obstacles(None)
        if upto in ("vertices", "targets"):
            self.set_vertices()
        if upto == "targets":
            self.set_targets()
        self.edges = edge_pack(np.zeros(2, dtype=np.uint64), np.arange(2), np.array([0, 1]))
        w = np.zeros(2, dtype=WRAPPER_EDGE_DTYPE)
        for i in range(2):   # a plausible curve from the vertex: never costed here, only looked at by the checks
            w[i] = (0, i, (0.0, 0.0, np.pi / 2), (0.5, 1.0, 0.5), self.cfg.coverage_turning_radius if i else self.cfg.turning_radius,
                    0, 0, 2.5, 0.0, 4.0)
        self.wedges = w
        self.offs = np.array([0, 1, 2], dtype=np.int32)
        self.res = _filled(2, RESULT_DTYPE)
        self.child = _filled(2 * CHILD_STRIDE * 4, np.float64)
        self.counts = _filled(2, np.int32)
        self.steps = _filled(2 * STEP_STRIDE, STEP_DTYPE)
        self.costed = _filled(2, np.int32)
        self.stop = _filled(2, np.uint32)
        self.d_edges = torch.from_numpy(self.edges.view(np.int64)).to("cuda:0")
        self.d_res = torch.full((2 * RESULT_DTYPE.itemsize,), FILL, dtype=torch.uint8, device="cuda:0")
        self.d_child = torch.full((2 * CHILD_STRIDE * 4 * 8,), FILL, dtype=torch.uint8, device="cuda:0")
        self.d_counts = torch.full((2 * 4,), FILL, dtype=torch.uint8, device="cuda:0")
        self.d_steps = torch.full((2 * STEP_STRIDE * STEP_DTYPE.itemsize,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()      # the fills ran on torch's stream, the library works on its own

    def set_vertices(self):
        self.ctx.set_vertices(_vertex(), RIBBON)

    def set_targets(self):
        self.ctx.set_samples(*TARGETS)

    def args(self, fn):
        """Valid arguments of ppgpu_<fn> behind the handle, by name and in call order."""
        host = dict(n=2, edges=self.edges, results=self.res)
        dev = dict(n=2, edges=self.d_edges.data_ptr(), results=self.d_res.data_ptr())
        return {
            "cost_edges_list": dict(dev, child=None, stride=0),
            "cost_edges_host": dict(host, child=None, stride=0),
            "cost_wrapper_edges_host": dict(host, edges=self.wedges, child=None, stride=0),
            "trace_edges_list": dict(dev, stride=STEP_STRIDE, counts=self.d_counts.data_ptr(), steps=self.d_steps.data_ptr()),
            "trace_edges_host": dict(host, stride=STEP_STRIDE, counts=self.counts, steps=self.steps),
            "trace_wrapper_edges_host": dict(host, edges=self.wedges, stride=STEP_STRIDE, counts=self.counts, steps=self.steps),
            "cost_plans_host": dict(n=2, offs=self.offs, edges=self.wedges, results=self.res, child=None, stride=CHILD_STRIDE,
                                    costed=self.costed, stop=self.stop),
        }[fn]

    def call(self, fn, **over):
        """(return code, message) of ppgpu_<fn> with the valid arguments, `over` replacing some of them."""
        a = self.args(fn)
        assert set(over) <= set(a), (fn, over)
        a.update(over)
        raw = [x.ctypes.data if isinstance(x, np.ndarray) else x for x in a.values()]
        rc = getattr(self.api.LIB, "ppgpu_" + fn)(self.ctx._h, *raw)
        return rc, self.api.LIB.ppgpu_last_error().decode()

    def host_untouched(self):
        return all(np.all(a.view(np.uint8) == FILL) for a in (self.res, self.child, self.counts, self.steps, self.costed, self.stop))

    def device_untouched(self):
        self.ctx.synchronize()
        return all(bool((t == FILL).all().item()) for t in (self.d_res, self.d_child, self.d_counts, self.d_steps))

    def two_edges(self):
        """The valid call: both edges through ppgpu_cost_edges_host, records and child ribbons as bytes."""
        res, child = self.ctx.cost_edges_host(self.edges, stride=CHILD_STRIDE)
        return res.tobytes() + child.tobytes()


@pytest.fixture(scope="module")
def rig(torch_cuda):
    return Rig(torch_cuda)


@pytest.fixture(scope="module")
def fresh_bytes(torch_cuda):
    """What a handle that never saw a refused call answers."""
    from path_planner_amd.types import F_THROWS
    r = Rig(torch_cuda)
    res, _ = r.ctx.cost_edges_host(r.edges, stride=CHILD_STRIDE)
    assert np.all((res["flags"] & F_THROWS) == 0) and np.all((res["info"] >> 16) > 0)      # two edges that were really swept
    return r.two_edges()


def _wrapper(rig, **fields):
    w = rig.wedges.copy()
    for k, x in fields.items():
        w[k][1] = x
    return w


def _cases():
    """(id, function, replaced arguments as a function of the rig, code, message)."""
    out = []

    def add(fn, what, over, code, msg):
        out.append(pytest.param(fn, over, code, msg, id=f"{fn}-{what}"))

    for fn in COST_FORMS + TRACE_FORMS:
        bad = fn + ": bad arguments"
        add(fn, "negative_n", lambda r: dict(n=-1), EINVAL, bad)
        add(fn, "null_list", lambda r: dict(edges=None), EINVAL, bad)
    for fn in COST_FORMS:
        add(fn, "null_results", lambda r: dict(results=None), EINVAL, fn + ": bad arguments")
        dev = fn.endswith("_list")
        for s in (0, -1):
            add(fn, f"child_stride_{s}", lambda r, s=s, dev=dev: dict(child=r.d_child.data_ptr() if dev else r.child, stride=s), EINVAL,
                fn + ": ribbon_stride must be positive")
    # (the list form has no early return for an empty list: the stride is looked at all the same)
    add("cost_edges_list", "empty_child_stride_0", lambda r: dict(n=0, child=r.d_child.data_ptr(), stride=0), EINVAL,
        "cost_edges_list: ribbon_stride must be positive")
    for fn in TRACE_FORMS:
        add(fn, "null_counts", lambda r: dict(counts=None), EINVAL, fn + ": bad arguments")
        add(fn, "null_steps", lambda r: dict(steps=None), EINVAL, fn + ": bad arguments")
        for s in (0, 65536):
            add(fn, f"step_stride_{s}", lambda r, s=s: dict(stride=s), EINVAL, fn + ": step_stride must be in 1 .. 65535")
        add(fn, "empty_step_stride_0", lambda r: dict(n=0, stride=0), EINVAL, fn + ": step_stride must be in 1 .. 65535")
    add("trace_edges_list", "null_results", lambda r: dict(results=None), EINVAL, "trace_edges_list: null results")
    add("trace_edges_list", "unaligned_steps", lambda r: dict(steps=r.d_steps.data_ptr() + 8), EINVAL,
        "trace_edges_list: d_steps must be 16-byte aligned")
    for fn in WRAPPER_FORMS:
        positive = fn + ": rho and speed must be positive"
        for name, x in (("zero", 0.0), ("negative", -8.0), ("nan", float("nan"))):
            add(fn, f"rho_{name}", lambda r, x=x: dict(edges=_wrapper(r, rho=x)), EINVAL, positive)
            add(fn, f"speed_{name}", lambda r, x=x: dict(edges=_wrapper(r, speed=x)), EINVAL, positive)
        add(fn, "vertex_minus_1", lambda r: dict(edges=_wrapper(r, vertex=-1)), EINVAL, fn + ": vertex out of range")
        add(fn, "vertex_nverts", lambda r: dict(edges=_wrapper(r, vertex=1)), EINVAL, fn + ": vertex out of range")
    fn = "cost_plans_host"
    add(fn, "negative_n", lambda r: dict(n=-1), EINVAL, fn + ": bad arguments")
    for name in ("offs", "costed", "stop"):
        add(fn, f"null_{name}", lambda r, name=name: {name: None}, EINVAL, fn + ": bad arguments")
    for s in (0, 65):
        add(fn, f"ribbon_stride_{s}", lambda r, s=s: dict(stride=s), EINVAL, fn + ": ribbon_stride must be in 1 .. 64")
        add(fn, f"ribbon_stride_{s}_with_child", lambda r, s=s: dict(child=r.child, stride=s), EINVAL, fn + ": ribbon_stride must be in 1 .. 64")
    add(fn, "negative_offset", lambda r: dict(offs=np.array([-1, 1, 2], dtype=np.int32)), EINVAL, fn + ": negative leg offset")
    add(fn, "decreasing_offsets", lambda r: dict(offs=np.array([0, 2, 1], dtype=np.int32)), EINVAL, fn + ": leg offsets must not decrease")
    add(fn, "null_legs", lambda r: dict(edges=None), EINVAL, fn + ": null legs or results")
    add(fn, "null_results", lambda r: dict(results=None), EINVAL, fn + ": null legs or results")
    return out


@pytest.mark.parametrize("fn,over,code,msg", _cases())
def test_refused_with_code_and_message(rig, fresh_bytes, fn, over, code, msg):
    rc, err = rig.call(fn, **over(rig))
    assert rc == code and msg in err, (rc, err)
    assert rig.host_untouched()
    assert rig.two_edges() == fresh_bytes


def test_before_vertices_and_before_targets(torch_cuda, fresh_bytes):
    r = Rig(torch_cuda, upto="config")
    for fn in COST_FORMS + TRACE_FORMS + ("cost_plans_host",):
        rc, err = r.call(fn)
        assert rc == ESTATE and NO_VERTICES in err, (fn, rc, err)
    r.set_targets()                                       # targets alone do not help: vertices are asked for first
    for fn in NEED_TARGETS:
        rc, err = r.call(fn)
        assert rc == ESTATE and NO_VERTICES in err, (fn, rc, err)
    r = Rig(torch_cuda, upto="vertices")
    for fn in NEED_TARGETS:
        rc, err = r.call(fn)
        assert rc == ESTATE and NO_TARGETS in err, (fn, rc, err)
    assert r.host_untouched() and r.device_untouched()
    r.set_targets()
    assert r.two_edges() == fresh_bytes


def test_empty_lists_are_fine_and_write_nothing(rig, fresh_bytes):
    for fn in COST_FORMS + TRACE_FORMS + ("cost_plans_host",):
        rc, err = rig.call(fn, n=0)
        assert rc == OK, (fn, rc, err)
    # the host forms return before they look at the child stride
    for fn in ("cost_edges_host", "cost_wrapper_edges_host"):
        rc, err = rig.call(fn, n=0, child=rig.child, stride=0)
        assert rc == OK, (fn, rc, err)
    # plans without a leg: their counts and stop codes are written, no record is
    rc, err = rig.call("cost_plans_host", offs=np.zeros(3, dtype=np.int32), edges=None, results=None)
    assert rc == OK, (rc, err)
    assert np.array_equal(rig.costed, [0, 0]) and np.array_equal(rig.stop, [1, 1])
    rig.costed.view(np.uint8)[:] = FILL
    rig.stop.view(np.uint8)[:] = FILL
    assert rig.host_untouched() and rig.device_untouched()
    assert rig.two_edges() == fresh_bytes


VERTEX_DEFECTS = {
    # name: (vertex fields, ribbons in the pool, code, message)
    "range_beyond_the_pool": (dict(ribbon_count=2), 1, EINVAL, "ribbon range outside the pool"),
    "range_from_beyond_the_pool": (dict(ribbon_offset=1), 1, EINVAL, "ribbon range outside the pool"),
    "negative_offset": (dict(ribbon_offset=-1), 1, EINVAL, "ribbon range outside the pool"),
    "65_ribbons": (dict(ribbon_count=65), 65, ECAPACITY, "more than 64 ribbons on one vertex"),
    "time_before_start": (dict(time=-1.0), 1, EINVAL, "vertex time before start_state_time"),
}


@pytest.mark.parametrize("name", sorted(VERTEX_DEFECTS))
def test_open_vertices_are_checked_alike(rig, fresh_bytes, name):
    """ppgpu_set_vertices and ppgpu_expand_host refuse the same vertices with the same code, each under its own name."""
    from path_planner_amd.types import RESULT_DTYPE
    fields, n_pool, code, msg = VERTEX_DEFECTS[name]
    LIB = rig.api.LIB
    v = _vertex(**fields)
    pool = np.ascontiguousarray(np.arange(n_pool * 4, dtype=np.float64).reshape(n_pool, 4))
    rc = LIB.ppgpu_set_vertices(rig.ctx._h, 1, v.ctypes.data, n_pool, pool.ctypes.data)
    err = LIB.ppgpu_last_error().decode()
    assert rc == code and err == "vertices: " + msg, (rc, err)
    assert rig.two_edges() == fresh_bytes
    cap = int(LIB.ppgpu_expand_capacity(1, 1))
    n_out = C.c_int64(-7)
    e, res = _filled(cap, np.uint64), _filled(cap, RESULT_DTYPE)
    rc = LIB.ppgpu_expand_host(rig.ctx._h, 1, v.ctypes.data, n_pool, pool.ctypes.data, None, 1, C.byref(n_out), e.ctypes.data, res.ctypes.data, None, 0)
    err = LIB.ppgpu_last_error().decode()
    assert rc == code and err == "expand_host: " + msg, (rc, err)
    assert n_out.value == -7 and np.all(e.view(np.uint8) == FILL) and np.all(res.view(np.uint8) == FILL)
    assert rig.two_edges() == fresh_bytes
