"""-m gpu: per-contact reports (ppgpu_trace_contacts_* -> pp_k_trace_contacts) against the recipe of tests/contact_replay.py run on
the device's OWN step records (ppgpu_trace_edges_host of the same list): both sides see the same poses and times, and the recipe's
+ - * and sqrt are the exact IEEE operations the kernel performs, so every integer and time field must be equal and cpa_distance
equal to 1 ulp.  The worlds are tests/sweep_worlds.py's (512^2 maps, 1 024 edges each, of which a few dozen are traced) and
contact_replay.edges_world() (edges of 1 .. 129 steps)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDE = 1504     # more than any edge has: a 30 s horizon at 0.02 s per step is 1 501 steps
PER_GROUP = 16    # edges per world and kind (hit, blocked, neither)
BINARY = ["stamps", "stacked", "reversed", "count1", "count64", "count65", "count129", "done_inside", "edges_world"]
GAUSSIAN = ["gaussian_stamps", "gaussian_count65"]
INT_FIELDS = ("cpa_step", "hit_steps", "first_hit_step", "last_hit_step")
TIME_FIELDS = ("cpa_time", "first_hit_time", "last_hit_time")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _sentinel(shape):
    from path_planner_amd.types import CONTACT_DTYPE
    return np.full(int(np.prod(shape)) * CONTACT_DTYPE.itemsize, 0xA5, dtype=np.uint8).view(CONTACT_DTYPE).reshape(shape)


def _untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == 0xA5))


def _pick(groups, per):
    out = []
    for g in groups:
        g = np.asarray(g)
        out.extend(g[:: max(1, len(g) // per)][:per].tolist())
    return np.array(sorted(set(out)), dtype=np.int64)


_PICKED = {}


def picked(name):
    """(world, rows, edge list) of a named world: about 48 of a sweep world's edges spread over hit, blocked and neither (chosen
    from the oracle's records, once per process), all of edges_world()."""
    import contact_replay as cr
    import sweep_worlds as sw
    from path_planner_amd.types import F_INFEASIBLE, F_THROWS
    if name not in _PICKED:
        if name == "edges_world":
            w = cr.edges_world()
            edges = w.edges
        else:
            w, rec, _ = sw.oracle_records(name)
            ok = (rec["flags"] & F_THROWS) == 0
            steps = rec["info"] >> 16
            blocked = np.nonzero(ok & ((rec["flags"] & F_INFEASIBLE) != 0) & (steps > 0))[0]
            hit = np.nonzero(ok & (rec["collision_penalty"] > 0))[0]
            rest = np.nonzero(ok & ((rec["flags"] & F_INFEASIBLE) == 0) & (rec["collision_penalty"] == 0))[0]
            assert len(hit) >= PER_GROUP, (name, len(hit))
            assert name == "done_inside" or len(blocked) >= PER_GROUP, (name, len(blocked))     # (done_inside's map is empty)
            edges = w.edges[_pick([hit, blocked, rest], PER_GROUP)]
        rows = cr.Rows(obst=w.obst) if w.gauss is None else cr.Rows(gauss=w.gauss)
        _PICKED[name] = (w, rows, edges)
    return _PICKED[name]


def trace_both(ctx, edges):
    """trace_edges and trace_contacts of the same list, the contacts written into a buffer of 0xA5 bytes; asserts what both models
    share: records byte-equal to the costing entry, equal counts, every record written."""
    n_obst = ctx.obstacle_count()[0]
    want = ctx.cost_edges_host(edges)
    res_t, counts_t, steps = ctx.trace_edges(edges, STRIDE)
    res, counts, contacts = ctx.trace_contacts(edges, _sentinel((len(edges), n_obst)))
    assert res.tobytes() == want.tobytes() and res_t.tobytes() == want.tobytes()
    assert np.array_equal(counts, counts_t)
    assert contacts.shape == (len(edges), n_obst)
    # exactly n * n_obst records are written: no field of any keeps the fill pattern (0xA5A5A5A5 is no step, 0xA5.. no time)
    assert not np.any(contacts["hit_steps"] == np.int32(-1515870811)) and not np.any(contacts["cpa_step"] == np.int32(-1515870811))
    assert np.all(contacts["hit_steps"] >= 0) and np.all(contacts["exposure"] >= 0) and np.all(contacts["peak"] >= 0)
    return res, counts, steps, contacts


def check_empty(c):
    import contact_replay as cr
    assert c.tobytes() == cr.empty_records(len(c)).tobytes()


@pytest.mark.parametrize("name", BINARY)
def test_binary_contacts_equal_the_recipe(torch_cuda, name):
    import contact_replay as cr
    w, rows, edges = picked(name)
    ctx = w.context()
    assert ctx.obstacle_count() == (len(w.obst), 1)
    res, counts, steps, contacts = trace_both(ctx, edges)
    cpf = w.cfg.collision_penalty_factor
    stats = dict(edges=len(edges), steps=int(counts.sum()), hit_records=0, empty_edges=0, worst_cpa_ulp=0.0)
    for i in range(len(edges)):
        s = steps[i, :counts[i]]
        got = contacts[i]
        if counts[i] == 0:
            check_empty(got)
            stats["empty_edges"] += 1
            continue
        want, d2min, _ = cr.replay(rows, s)
        for f in INT_FIELDS + TIME_FIELDS + ("exposure", "peak"):
            assert np.array_equal(got[f], want[f]), (name, i, f, got[f], want[f])
        ulp = np.abs(got["cpa_distance"] - want["cpa_distance"]) / np.spacing(want["cpa_distance"])
        stats["worst_cpa_ulp"] = max(stats["worst_cpa_ulp"], float(ulp.max()))
        assert ulp.max() <= 1.0, (name, i, got["cpa_distance"], want["cpa_distance"])
        assert np.all(got["peak"] == 0) and np.array_equal(got["exposure"], got["hit_steps"].astype(np.float64))
        assert float(got["hit_steps"].sum()) * cpf == res["collision_penalty"][i], (name, i)
        assert got["hit_steps"].sum() == s["collision"].sum(), (name, i)
        stats["hit_records"] += int(np.count_nonzero(got["hit_steps"]))
    print(name, stats)
    assert stats["hit_records"] > 0
    if name == "edges_world":
        assert list(counts[:len(cr.STEP_COUNTS)]) == list(cr.STEP_COUNTS) and 0 < counts[w.blocked_edge] <= 64
        i64 = cr.STEP_COUNTS.index(64)
        assert np.all(contacts["first_hit_step"][:len(cr.STEP_COUNTS), 0] == 0)                    # the box over the root
        assert contacts["hit_steps"][i64, 1] == 1 and contacts["first_hit_step"][i64, 1] == 63     # entered on the last step
        assert contacts["hit_steps"][i64 - 1, 1] == 0
        assert np.all(contacts["hit_steps"][:, 2] == 0) and np.all(contacts["cpa_distance"][:, 2] > 9000)      # parked 10 km away


@pytest.mark.parametrize("name", GAUSSIAN)
def test_gaussian_contacts_match_the_recipe(torch_cuda, name):
    import contact_replay as cr
    from parity import REL_TOL
    w, rows, edges = picked(name)
    ctx = w.context()
    assert ctx.obstacle_count() == (len(w.gauss), 2)
    res, counts, steps, contacts = trace_both(ctx, edges)
    cpf = w.cfg.collision_penalty_factor

    def rel(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)

    stats = dict(edges=len(edges), steps=int(counts.sum()), hit_records=0, floor_steps=0, hit_step_differences=0, worst_exposure=0.0, worst_sum=0.0)
    for i in range(len(edges)):
        s = steps[i, :counts[i]]
        got = contacts[i]
        if counts[i] == 0:
            check_empty(got)
            continue
        want, d2min, pdf = cr.replay(rows, s)
        assert np.array_equal(got["cpa_step"], want["cpa_step"]) and np.array_equal(got["cpa_time"], want["cpa_time"]), (name, i)
        for f in ("exposure", "peak", "cpa_distance"):
            r = rel(got[f], want[f])
            assert r.max() <= REL_TOL, (name, i, f, got[f], want[f])
        stats["worst_exposure"] = max(stats["worst_exposure"], float(rel(got["exposure"], want["exposure"]).max()))
        # hit steps: those of the recipe, except on steps where the contact's pdf is within REL_TOL (relative) of the floor
        counted = (s["collision"] != 0) & ((s["flags"] & 1) == 0)
        at_floor = (np.abs(pdf - cr.FLOOR) <= REL_TOL * cr.FLOOR) & counted[None, :]
        stats["floor_steps"] += int(at_floor.sum())
        diff = np.abs(got["hit_steps"] - want["hit_steps"])
        assert np.all(diff <= at_floor.sum(axis=1)), (name, i, got["hit_steps"], want["hit_steps"])
        stats["hit_step_differences"] += int(diff.sum())
        same = diff == 0
        for f in ("first_hit_step", "last_hit_step", "first_hit_time", "last_hit_time"):
            assert np.array_equal(got[f][same & (at_floor.sum(axis=1) == 0)], want[f][same & (at_floor.sum(axis=1) == 0)]), (name, i, f)
        r = rel(float(got["exposure"].sum()) * cpf, res["collision_penalty"][i])
        stats["worst_sum"] = max(stats["worst_sum"], float(r))
        assert r <= REL_TOL, (name, i, float(got["exposure"].sum()) * cpf, res["collision_penalty"][i])
        stats["hit_records"] += int(np.count_nonzero(got["hit_steps"]))
    print(name, stats, "(floor_steps: counted steps with a contact's pdf within REL_TOL of 1e-5)")
    assert stats["hit_records"] > 0


def test_no_obstacles_leave_the_buffer_untouched(torch_cuda):
    """A world without obstacles: counts and results as usual, not one byte of the contacts written."""
    import contact_replay as cr
    w = cr.edges_world()
    ctx = w.context()
    ctx.set_obstacles(np.zeros((0, 7)))
    assert ctx.obstacle_count() == (0, 0)
    res, counts, contacts = ctx.trace_contacts(w.edges)
    assert contacts.shape == (len(w.edges), 0)
    assert list(counts[:len(cr.STEP_COUNTS)]) == list(cr.STEP_COUNTS)
    assert res.tobytes() == ctx.cost_edges_host(w.edges).tobytes()
    from path_planner_amd import api
    buf = _sentinel((len(w.edges), 3))
    c2 = np.full(len(w.edges), -1, dtype=np.int32)
    rc = api.LIB.ppgpu_trace_contacts_host(ctx._h, len(w.edges), w.edges.ctypes.data, None, c2.ctypes.data, buf.ctypes.data)
    assert rc == 0 and np.array_equal(c2, counts) and _untouched(buf)


def test_wrapper_form_and_edges_without_steps(torch_cuda):
    """The wrapper form gives the list form's records for the same edge; a curve that starts after its vertex's first step has no
    steps and gets the empty record for every contact."""
    import contact_replay as cr
    w = cr.edges_world()
    ctx = w.context()
    i64 = cr.STEP_COUNTS.index(64)
    _, counts, contacts = ctx.trace_contacts(w.edges)
    wres, wcounts, wcontacts = ctx.trace_contacts_wrapper_edges(w.wedges, _sentinel((2, 3)))
    assert wres.tobytes() == ctx.cost_wrapper_edges_host(w.wedges).tobytes()
    assert list(wcounts) == [64, 0]
    assert wcontacts[0].tobytes() == contacts[i64].tobytes()
    check_empty(wcontacts[1])


def test_wrapper_form_gives_the_list_form_records(torch_cuda):
    """... on a sweep world: the picked edges handed over as curves (qi from the vertex, param / type from the list form's records)."""
    import oracle as orc
    from path_planner_amd.types import WRAPPER_EDGE_DTYPE, F_THROWS
    w, rows, edges = picked("stamps")
    ctx = w.context()
    res, counts, contacts = ctx.trace_contacts(edges)
    keep = np.nonzero((res["flags"] & F_THROWS) == 0)[0]
    we = np.zeros(len(keep), dtype=WRAPPER_EDGE_DTYPE)
    v = w.verts[0]
    for j, i in enumerate(keep):
        cb = int(int(edges[i]) >> 56)
        rho = w.cfg.coverage_turning_radius if cb & 1 else w.cfg.turning_radius
        speed = w.cfg.slow_speed if cb & 2 else w.cfg.max_speed
        r = res[i]
        p8 = np.array([v["x"], v["y"], orc.yaw(float(v["heading"])), r["param"][0], r["param"][1], r["param"][2], rho, float(r["info"] & 0xFF)])
        end = orc.O.ppo_wrapper_fill_end_time(p8.ctypes.data, speed, float(v["time"]))
        we[j] = (0, cb & 1, p8[0:3], p8[3:6], rho, int(p8[7]), 0, speed, float(v["time"]), end)
    wres, wcounts, wcontacts = ctx.trace_contacts_wrapper_edges(we)
    assert np.array_equal(wcounts, counts[keep])
    assert wcontacts.tobytes() == contacts[keep].tobytes()


@pytest.mark.parametrize("budget", [24 << 10, 400 << 10])
def test_sliced_contact_trace_is_bit_identical(torch_cuda, monkeypatch, budget):
    """A handle with a small workspace budget runs the costing launch and the walk as slices (24 KB: a few edges at a time, the
    curves solved again per slice; 400 KB: the costing launch fits, the records come home in passes).  The same bytes as in one piece."""
    w, rows, edges = picked("count65")
    whole = w.context().trace_contacts(edges)
    monkeypatch.setenv("PPGPU_SLICE_BYTES", str(budget))
    cut = w.context().trace_contacts(edges, _sentinel((len(edges), 65)))
    for a, b in zip(whole, cut):
        assert a.tobytes() == b.tobytes()


def test_whole_world_through_the_prepass_route(torch_cuda, monkeypatch):
    """All 1 024 edges of count65 in one launch that takes the chunk-skip planner and the approach prepass, list form, device
    arrays: records byte-identical to the costing entry point, the hit sums on every edge, and the contact records equal to those
    of a launch that samples every chunk."""
    import sweep_worlds as sw
    from path_planner_amd.types import RESULT_DTYPE, CONTACT_DTYPE, F_THROWS
    torch = torch_cuda
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", "0")
    w = sw.WORLDS["count65"]()
    ne, nob = len(w.edges), len(w.obst)
    ctx = w.context()
    d_e = torch.from_numpy(w.edges.view(np.int64)).to("cuda:0")
    d_res = torch.zeros(ne * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_counts = torch.full((ne,), -1, dtype=torch.int32, device="cuda:0")
    d_con = torch.full((ne * nob * CONTACT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()      # the fills ran on torch's stream, the library works on its own
    ctx.trace_contacts_list(ne, d_e.data_ptr(), d_res.data_ptr(), d_counts.data_ptr(), d_con.data_ptr())
    ctx.synchronize()
    res = d_res.cpu().numpy().view(RESULT_DTYPE)
    counts = d_counts.cpu().numpy()
    contacts = d_con.cpu().numpy().view(CONTACT_DTYPE).reshape(ne, nob)
    assert res.tobytes() == ctx.cost_edges_host(w.edges).tobytes()
    assert np.array_equal(counts, np.where((res["flags"] & F_THROWS) != 0, 0, res["info"] >> 16).astype(np.int32))
    assert np.array_equal(contacts["hit_steps"].sum(axis=1) * w.cfg.collision_penalty_factor, res["collision_penalty"])
    assert np.all((contacts["cpa_step"] >= 0) == (counts > 0)[:, None]) and np.all(contacts["cpa_step"] < np.maximum(counts, 1)[:, None])
    print("whole world:", ne, "edges,", int(counts.sum()), "steps,", int(np.count_nonzero(contacts["hit_steps"])), "hit records")
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", "1000000000")
    r2, c2, k2 = w.context().trace_contacts(w.edges)
    assert np.array_equal(c2, counts) and k2.tobytes() == contacts.tobytes()


def test_bad_arguments_are_refused(torch_cuda):
    import contact_replay as cr
    from path_planner_amd import api
    w = cr.edges_world()
    ctx = w.context()
    n = len(w.edges)
    counts = np.zeros(n, dtype=np.int32)
    contacts = _sentinel((n, 3))
    e = w.edges
    rc = api.LIB.ppgpu_trace_contacts_host(ctx._h, n, e.ctypes.data, None, counts.ctypes.data, None)            # obstacles set, no records
    assert rc == -1 and b"trace_contacts_host" in api.LIB.ppgpu_last_error()
    rc = api.LIB.ppgpu_trace_contacts_host(ctx._h, n, e.ctypes.data, None, None, contacts.ctypes.data)
    assert rc == -1 and b"trace_contacts_host" in api.LIB.ppgpu_last_error()
    rc = api.LIB.ppgpu_trace_contacts_host(ctx._h, -1, e.ctypes.data, None, counts.ctypes.data, contacts.ctypes.data)
    assert rc == -1
    rc = api.LIB.ppgpu_trace_contacts_wrapper_edges_host(ctx._h, 2, w.wedges.ctypes.data, None, None, contacts.ctypes.data)
    assert rc == -1 and b"trace_contacts_wrapper_edges_host" in api.LIB.ppgpu_last_error()
    rc = api.LIB.ppgpu_trace_contacts_list(ctx._h, -1, None, None, None, None)
    assert rc == -1 and b"trace_contacts_list" in api.LIB.ppgpu_last_error()
    assert _untouched(contacts)
    rc = api.LIB.ppgpu_trace_contacts_host(ctx._h, n, e.ctypes.data, None, counts.ctypes.data, contacts.ctypes.data)
    assert rc == 0 and list(counts[:len(cr.STEP_COUNTS)]) == list(cr.STEP_COUNTS)       # h_results may be NULL
    assert api.LIB.ppgpu_obstacle_count(None, None, None) == -1
    # the host form's records pass through a buffer of the handle, and its growth is counted
    w2, _, edges = picked("count129")
    ctx2 = w2.context()
    before = ctx2.growth_stats()[0]
    ctx2.trace_contacts(edges)
    assert ctx2.growth_stats()[0] > before
