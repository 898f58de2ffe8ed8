"""-m gpu: the three edge traces at the edges of their 64-step windows.  The traces share one window walk and one record store
(pp_k_trace_common.h); both can go wrong where a window is full, one step short or one step long, and where a workgroup is not.
contact_replay.edges_world() is directed at that: 9 edges (a partial last workgroup of 4 waves) of exactly 1, 2, 63, 64, 65, 127,
128 and 129 steps, one a blocked cell stops near step 40, a wrapper-form edge with no steps, 3 boxes.
tests/test_trace_windows_inputs.py proves these inputs on the CPU, and picks from test_gpu_trace.world_binary()'s candidates the
shortest edge of three or more windows whose count is 0, 1 and 63 modulo 64."""
import numpy as np
import pytest

import contact_replay as cr
import cover_replay
from test_gpu_trace import check_trace
from test_gpu_cover_trace import check_cover
from test_trace_windows_inputs import residue_world

pytestmark = pytest.mark.gpu

FULL = 160               # more steps than any edge of edges_world() has, and no multiple of 64
STRIDES = (1, 63, 64, 65, 130)
RIBBONS = 16             # ribbon_stride of the final lists: more than any list of these worlds
FILL = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _filled(shape, dtype):
    return np.full(int(np.prod(shape)) * dtype.itemsize, FILL, dtype=np.uint8).view(dtype).reshape(shape)


def _untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def _trace_all(w, edges, stride):
    """(step trace, cover trace, contact trace) of one context, every record array pre-filled with the sentinel."""
    from path_planner_amd.types import STEP_DTYPE, COVER_DTYPE, CONTACT_DTYPE
    ctx = w.context()
    n = len(edges)
    return (ctx.trace_edges(edges, stride, _filled((n, stride), STEP_DTYPE)),
            ctx.trace_cover(edges, stride, _filled((n, stride), COVER_DTYPE), ribbon_stride=RIBBONS),
            ctx.trace_contacts(edges, _filled((n, ctx.obstacle_count()[0]), CONTACT_DTYPE)))


_RUNS = {}


def full_run():
    """The untruncated traces of edges_world(): computed once, left unchanged."""
    if "edges" not in _RUNS:
        _RUNS["edges"] = _trace_all(cr.edges_world(), cr.edges_world().edges, FULL)
    return _RUNS["edges"]


def residue_run():
    if "residue" not in _RUNS:
        tw, want = residue_world()
        _RUNS["residue"] = _trace_all(tw, tw.edges, int(want.max()) + 1)
    return _RUNS["residue"]


def test_counts(torch_cuda):
    """The three traces report the same counts: STEP_COUNTS, and the oracle's for the blocked edge.  Their records of the costing
    launch are the same bytes."""
    w = cr.edges_world()
    (res, counts, _), (cres, ccounts, _, _, _), (kres, kcounts, _) = full_run()
    want = list(cr.STEP_COUNTS) + [int(w.records["info"][w.blocked_edge] >> 16)]
    assert list(counts) == want and list(ccounts) == want and list(kcounts) == want
    assert res.tobytes() == cres.tobytes() == kres.tobytes()


def test_step_trace(torch_cuda):
    """test_gpu_trace's checks 1-8 on every edge, the residue edges included; nothing is written beyond an edge's count."""
    w = cr.edges_world()
    res, counts, steps = full_run()[0]
    stats = check_trace(w, w.edges, res, counts, steps)
    assert stats["steps"] == sum(cr.STEP_COUNTS) + counts[w.blocked_edge] and stats["n_blocked"] == 1 and stats["n_collision_steps"] > 0
    for i in range(len(w.edges)):
        assert _untouched(steps[i, counts[i]:]), i
    tw, want = residue_world()
    res, counts, steps = residue_run()[0]
    assert list(counts) == list(want)
    check_trace(tw, tw.edges, res, counts, steps)
    for i in range(len(tw.edges)):
        assert _untouched(steps[i, counts[i]:]), i


def test_cover_trace(torch_cuda):
    """test_gpu_cover_trace's check 1 on every edge, the residue edges included; nothing is written beyond an edge's count."""
    for w, (trace, cover_run, _) in ((cr.edges_world(), full_run()), (residue_world()[0], residue_run())):
        res, counts, steps = trace
        cres, ccounts, cover, summ, final = cover_run
        stats = check_cover(w, [cover_replay.edge_inputs(w, d) for d in w.edges], steps, counts, cover, ccounts, summ, final, {})
        assert stats["edges"] == len(w.edges) and stats["events"] > 0
        for i in range(len(w.edges)):
            assert _untouched(cover[i, counts[i]:]), i


def test_contact_trace(torch_cuda):
    """The records equal contact_replay.replay on the device's own steps, as test_binary_contacts_equal_the_recipe checks them; a
    guard row behind the last edge's slot keeps its fill."""
    from path_planner_amd import api
    from path_planner_amd.types import CONTACT_DTYPE
    w = cr.edges_world()
    (res, counts, steps), _, (_, _, contacts) = full_run()
    rows = cr.Rows(obst=w.obst)
    assert not _untouched(contacts) and np.all(contacts["hit_steps"] >= 0)
    for i in range(len(w.edges)):
        want, _, _ = cr.replay(rows, steps[i, :counts[i]])
        got = contacts[i]
        for f in ("cpa_step", "hit_steps", "first_hit_step", "last_hit_step", "cpa_time", "first_hit_time", "last_hit_time", "exposure", "peak"):
            assert np.array_equal(got[f], want[f]), (i, f, got[f], want[f])
        assert np.all(np.abs(got["cpa_distance"] - want["cpa_distance"]) <= np.spacing(want["cpa_distance"])), i
        assert float(got["hit_steps"].sum()) * w.cfg.collision_penalty_factor == res["collision_penalty"][i], i
    n = len(w.edges)
    guarded = _filled((n + 1, len(w.obst)), CONTACT_DTYPE)
    kcounts = np.zeros(n, dtype=np.int32)
    assert api.LIB.ppgpu_trace_contacts_host(w.context()._h, n, w.edges.ctypes.data, None, kcounts.ctypes.data, guarded.ctypes.data) == 0
    assert guarded[:n].tobytes() == contacts.tobytes() and _untouched(guarded[n])


@pytest.mark.parametrize("stride", STRIDES)
def test_strides_cut_records_only(torch_cuda, stride):
    """A step_stride at, below and above a window edge: step and cover records [0, min(count, stride)) are those of the untruncated
    run, counts, summaries and final lists are whole, the rest of every slot keeps its fill."""
    w = cr.edges_world()
    (res, counts, steps), (_, _, cover, summ, final), _ = full_run()
    (res2, counts2, steps2), (cres2, ccounts2, cover2, summ2, final2), _ = _trace_all(w, w.edges, stride)
    assert res2.tobytes() == res.tobytes() == cres2.tobytes()
    assert np.array_equal(counts2, counts) and np.array_equal(ccounts2, counts)
    assert summ2.tobytes() == summ.tobytes() and final2.tobytes() == final.tobytes()
    for i in range(len(w.edges)):
        m = min(int(counts[i]), stride)
        assert steps2[i, :m].tobytes() == steps[i, :m].tobytes() and cover2[i, :m].tobytes() == cover[i, :m].tobytes(), i
        assert _untouched(steps2[i, m:]) and _untouched(cover2[i, m:]), i


def test_wrapper_form_edges(torch_cuda):
    """Counts of 64 and 0 through the three wrapper entries; the 64-step curve has the list form's records; the curve without steps
    writes no step or cover record, and the empty record for every contact."""
    from path_planner_amd.types import STEP_DTYPE, COVER_DTYPE, CONTACT_DTYPE
    w = cr.edges_world()
    (_, _, steps), (_, _, cover, _, _), (_, _, contacts) = full_run()
    i64 = cr.STEP_COUNTS.index(64)
    ctx = w.context()
    _, wcounts, wsteps = ctx.trace_wrapper_edges(w.wedges, FULL, _filled((2, FULL), STEP_DTYPE))
    _, ccounts, wcover, wsumm, _ = ctx.trace_cover_wrapper_edges(w.wedges, FULL, _filled((2, FULL), COVER_DTYPE), ribbon_stride=RIBBONS)
    _, kcounts, wcontacts = ctx.trace_contacts_wrapper_edges(w.wedges, _filled((2, len(w.obst)), CONTACT_DTYPE))
    assert list(wcounts) == [64, 0] and list(ccounts) == [64, 0] and list(kcounts) == [64, 0]
    assert wsteps[0, :64].tobytes() == steps[i64, :64].tobytes() and _untouched(wsteps[0, 64:]) and _untouched(wsteps[1])
    assert wcover[0, :64].tobytes() == cover[i64, :64].tobytes() and _untouched(wcover[0, 64:]) and _untouched(wcover[1])
    assert wsumm["events"][1] == 0
    assert wcontacts[0].tobytes() == contacts[i64].tobytes() and wcontacts[1].tobytes() == cr.empty_records(len(w.obst)).tobytes()
