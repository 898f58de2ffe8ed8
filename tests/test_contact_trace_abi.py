"""The contact-trace entry points exist at every layer that needs no GPU — declared in include/ppgpu.h with the layout of their numpy
mirror, exported by libppgpu.so, bound in path_planner_amd.api; DynamicObstaclesManager::deviceIds names the rows of deviceRows —
and the recipe the GPU tests compare the device against (tests/contact_replay.py) pins itself on the oracle."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTACT = ["ppgpu_trace_contacts_list", "ppgpu_trace_contacts_host", "ppgpu_trace_contacts_wrapper_edges_host", "ppgpu_obstacle_count",
           "ppgpu_last_contact_trace_timing"]
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


def test_header_layout_equals_the_numpy_mirror():
    from path_planner_amd.types import CONTACT_DTYPE
    txt = _header()
    for name in CONTACT:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name
    fields, size = _struct_layout(txt, "ppgpu_contact_record")
    assert size == CONTACT_DTYPE.itemsize == 64 and size % 16 == 0
    assert [(n, CONTACT_DTYPE.fields[n][0].str, CONTACT_DTYPE.fields[n][1]) for n in CONTACT_DTYPE.names] == fields
    full = open(os.path.join(ROOT, "include", "ppgpu.h")).read()
    for cite in ("Edge.cpp:150-151", "BinaryDynamicObstaclesManager.cpp:4-22", "GaussianDynamicObstaclesManager.h:31-43"):
        assert cite in full[full.index("contact traces"):], cite


def test_library_exports_and_binding_has_them():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    for name in CONTACT:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert getattr(api.LIB, name).restype is C.c_int
    for method in ("trace_contacts", "trace_contacts_wrapper_edges", "trace_contacts_list", "obstacle_count", "last_contact_trace_timing"):
        assert callable(getattr(api.Context, method)), method


def _ids_and_rows(H, h, width):
    ids = np.zeros(64, dtype=np.uint32)
    n = H.pph_obst_device_ids(h, ids.ctypes.data, 64)
    rows = np.zeros(64 * width)
    m = H.pph_obst_device_rows(h, rows.ctypes.data, rows.size)
    assert m == n * width
    return ids[:n].tolist(), rows[:m].reshape(n, width)


def test_device_ids_name_the_rows_of_device_rows():
    """DynamicObstaclesManager::deviceIds: the MMSIs of deviceRows' rows, in the same order, after update, forget (the last track
    moves into the freed slot) and addIgnore (a muted contact's reports are dropped; what it reported before stays), for both
    managers.  Every contact reports x = its MMSI, so a row names its own contact."""
    import hostlib
    H = hostlib.H
    so = open(hostlib.HOST_SO, "rb").read()
    assert b"BinaryDynamicObstaclesManager9deviceIds" in so and b"GaussianDynamicObstaclesManager9deviceIds" in so
    H.pph_obst_device_ids.restype, H.pph_obst_device_ids.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    H.pph_obst_add_ignore.restype, H.pph_obst_add_ignore.argtypes = None, [C.c_void_p, C.c_uint]
    for gaussian, width in ((0, 7), (1, 9)):
        h = H.pph_obst_create(gaussian)
        assert _ids_and_rows(H, h, width)[0] == []
        report = lambda m, y=0.0: H.pph_obst_update(h, m, float(m), y, 0.3, 1.0, 5.0, 4.0, 9.0)
        for m in (901, 17, 333, 4000000000, 58):
            report(m)
        ids, rows = _ids_and_rows(H, h, width)
        assert ids == [901, 17, 333, 4000000000, 58] and np.array_equal(rows[:, 0], np.array(ids, dtype=np.float64))
        report(333, 7.0)                                     # a second report of a known contact keeps its row
        ids, rows = _ids_and_rows(H, h, width)
        assert ids == [901, 17, 333, 4000000000, 58] and rows[2, 1] == 7.0
        H.pph_obst_forget(h, 17)                             # the last track moves into the freed slot
        ids, rows = _ids_and_rows(H, h, width)
        assert ids == [901, 58, 333, 4000000000] and np.array_equal(rows[:, 0], np.array(ids, dtype=np.float64))
        H.pph_obst_forget(h, 12345)                          # unknown: nothing happens
        H.pph_obst_add_ignore(h, 77)
        report(77)                                           # muted before its first report: never a row
        H.pph_obst_add_ignore(h, 333)
        report(333, 9.0)                                     # muted later: the row stays what it was
        report(5)
        ids, rows = _ids_and_rows(H, h, width)
        assert ids == [901, 58, 333, 4000000000, 5] and np.array_equal(rows[:, 0], np.array(ids, dtype=np.float64)) and rows[2, 1] == 7.0
        H.pph_obst_free(h)


def _probe_points(obst, rows, n, seed):
    """n points (x, y, t): a third within 1e-12 of a box's long or short side at the point's time, a third inside or just around a
    box, a third anywhere on the map."""
    rng = np.random.default_rng(seed)
    x, y, t = np.zeros(n), np.zeros(n), rng.uniform(0.0, 40.0, n)
    for i in range(n):
        j = int(rng.integers(0, rows.n))
        dt = t[i] - rows.Time[j]
        cx = rows.X[j] + rows.Speed[j] * dt * rows.cosYaw[j]
        cy = rows.Y[j] + rows.Speed[j] * dt * rows.sinYaw[j]
        kind = i % 3
        if kind == 0:
            side = float(rng.choice([-1.0, 1.0]))
            eps = float(rng.uniform(-1e-12, 1e-12))
            if rng.random() < 0.5:
                rx, ry = side * (rows.halfL[j] + eps), float(rng.uniform(-1, 1)) * rows.halfW[j]
            else:
                rx, ry = float(rng.uniform(-1, 1)) * rows.halfL[j], side * (rows.halfW[j] + eps)
        elif kind == 1:
            rx, ry = float(rng.uniform(-1.5, 1.5)) * rows.halfL[j], float(rng.uniform(-1.5, 1.5)) * rows.halfW[j]
        else:
            x[i], y[i] = rng.uniform(0, 400), rng.uniform(0, 400)
            continue
        c, s = rows.cosYaw[j], rows.sinYaw[j]                # the box frame is the world frame turned by +yaw: back by -yaw
        x[i], y[i] = cx + rx * c + ry * s, cy - rx * s + ry * c
    return x, y, t


def test_the_recipes_box_test_is_the_oracles():
    """The recipe pins itself: for 40 000 points, a third of them within 1e-12 of a box's side, the recipe's per-contact hit equals
    the oracle's collisionExists of a world holding that row alone, exactly, and the sum over the rows the whole world's answer."""
    import contact_replay as cr
    import oracle as orc
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=16)
    assert len(w.obst) == 16
    rows = cr.Rows(obst=w.obst)
    n = 40000
    x, y, t = _probe_points(w.obst, rows, n, 31)
    hit = rows.box_hit(x, y, t)
    whole = orc.World(w.cfg, obst=w.obst)
    want_sum = np.array([whole.collision_exists(float(x[i]), float(y[i]), float(t[i]), True) for i in range(n)])
    mismatches = int(np.count_nonzero(hit.sum(axis=0) != want_sum))
    for j in range(rows.n):
        alone = orc.World(w.cfg, obst=w.obst[j:j + 1])
        want = np.array([alone.collision_exists(float(x[i]), float(y[i]), float(t[i]), True) for i in range(n)])
        mismatches += int(np.count_nonzero(hit[j] != (want != 0)))
        assert np.all((want == 0) | (want == 1))
    print("probe points", n, "hits", int(hit.sum()), "near a side and hit", int(hit[:, 0::3].sum()), "mismatches", mismatches)
    assert mismatches == 0
    near = hit[:, 0::3].any(axis=0)
    assert hit.sum() > n // 4 and 0.2 < near.mean() < 0.8          # the points at the sides fall on both sides of them


def test_edges_world_holds_what_it_claims():
    """Step counts, the blocked edge, the three boxes' hit patterns and the wrapper edge without steps — on the oracle alone."""
    import contact_replay as cr
    import oracle as orc
    from path_planner_amd.types import F_INFEASIBLE, F_THROWS
    w = cr.edges_world()
    rec = w.records
    nroot = len(cr.STEP_COUNTS)
    assert not np.any(rec["flags"] & F_THROWS)
    assert list(rec["info"][:nroot] >> 16) == list(cr.STEP_COUNTS) and not np.any(rec["flags"][:nroot] & F_INFEASIBLE)
    b = w.blocked_edge
    assert (rec["flags"][b] & F_INFEASIBLE) and 0 < (rec["info"][b] >> 16) <= 64              # stopped within its first window
    free = orc.World(w.cfg, np.zeros_like(w.grid), w.res, w.obst).cost_edges(w.verts, w.pool, w.sx, w.sy, w.sh, w.edges)
    assert (free["info"][b] >> 16) > (rec["info"][b] >> 16) and not (free["flags"][b] & F_INFEASIBLE)    # ... by the one blocked cell
    cpf = w.cfg.collision_penalty_factor
    hits = np.zeros((len(w.edges), 3))
    for j in range(3):
        alone = orc.World(w.cfg, w.grid, w.res, w.obst[j:j + 1]).cost_edges(w.verts, w.pool, w.sx, w.sy, w.sh, w.edges)
        hits[:, j] = alone["collision_penalty"] / cpf
    assert np.array_equal(hits.sum(axis=1) * cpf, rec["collision_penalty"])
    i1, i63, i64 = (cr.STEP_COUNTS.index(n) for n in (1, 63, 64))
    assert hits[i1, 0] == 1 and np.all(hits[:nroot, 0] >= 1)        # over the root at the root's time: the 1-step edge's only step is hit
    assert hits[i63, 1] == 0 and hits[i64, 1] == 1                  # first entered on the last step of the 64-step edge
    assert np.all(hits[i64 + 1:nroot, 1] > 1)
    assert np.all(hits[:, 2] == 0)                                  # parked 10 km away
    assert w.world.collision_exists(cr.EC, cr.EC, cr.ET0, True) == 1
    wrec = w.world.cost_wrapper_edges(w.verts, w.pool, w.wedges)
    assert (wrec["info"][0] >> 16) == 64 and (wrec["info"][1] >> 16) == 0 and (wrec["flags"][1] & F_INFEASIBLE)


def test_merge_is_the_stated_merge():
    import contact_replay as cr
    a, b = cr.empty_records(2), cr.empty_records(2)
    a[0] = (3.0, 10.0, 11.0, 12.0, 2.0, 5, 2, 6, 7, 0.5)
    b[0] = (3.0, 20.0, 21.0, 22.0, 3.0, 1, 3, 2, 4, 0.25)           # an equal CPA later on: the earlier segment's stays
    b[1] = (8.0, 23.0, -1.0, -1.0, 0.0, 4, 0, -1, -1, 0.0)
    m = cr.merge([a, b])
    assert (m["hit_steps"][0], m["exposure"][0], m["first_hit_time"][0], m["last_hit_time"][0]) == (5, 5.0, 11.0, 22.0)
    assert (m["cpa_distance"][0], m["cpa_time"][0], m["peak"][0]) == (3.0, 10.0, 0.5)
    assert (m["hit_steps"][1], m["first_hit_time"][1], m["cpa_distance"][1], m["cpa_time"][1]) == (0, -1.0, 8.0, 23.0)
