"""The inputs of tests/test_gpu_trace_windows.py, proven on the CPU before they travel: the oracle's records of
contact_replay.edges_world() have exactly the step counts the window-edge tests rely on, and the random candidates of
test_gpu_trace.world_binary() hold edges of three or more windows whose count is 0, 1 and 63 modulo 64."""
import numpy as np

import contact_replay as cr

RESIDUES = (0, 1, 63)    # step count modulo 64: a full last window, one step in the last window, one lane short of a full one


def test_edges_world_has_the_step_counts():
    from path_planner_amd.types import F_INFEASIBLE, F_THROWS
    w = cr.edges_world()
    rec = w.records
    n = len(cr.STEP_COUNTS)
    assert len(w.edges) == n + 1 == 9 and w.blocked_edge == n            # 9 edges: a partial last workgroup of 4 waves
    assert not np.any(rec["flags"] & F_THROWS)
    assert list(rec["info"][:n] >> 16) == list(cr.STEP_COUNTS)
    assert not np.any(rec["flags"][:n] & F_INFEASIBLE)
    assert rec["flags"][n] & F_INFEASIBLE and 0 < (rec["info"][n] >> 16) <= 64 and abs(int(rec["info"][n] >> 16) - cr.BLOCK_STEP) <= 2
    assert len(w.obst) == 3 and len(w.wedges) == 2


_RESIDUE = []


def residue_world():
    """(world, counts): test_gpu_trace.world_binary()'s world and candidates, its edge list the candidate with the fewest steps of
    each class of RESIDUES (oracle-costed, not thrown).  Built once per process."""
    from path_planner_amd import workloads
    from path_planner_amd.types import F_THROWS
    from test_gpu_trace import TraceWorld, _grow
    if not _RESIDUE:
        w = workloads.config3(n_samples=512)
        tw = TraceWorld(w.cfg, w.grid, w.res, w.obst)
        cand, rec = _grow(tw, w, 512, 30, 5, 3000)                        # world_binary()'s own call
        steps = (rec["info"] >> 16).astype(np.int64)
        ok = (rec["flags"] & F_THROWS) == 0
        pick = []
        for r in RESIDUES:
            cls = np.nonzero(ok & (steps > 0) & (steps % 64 == r))[0]
            assert len(cls) > 0, r
            pick.append(int(cls[np.argmin(steps[cls])]))
        tw.edges = cand[pick]
        _RESIDUE.append((tw, steps[pick]))
    return _RESIDUE[0]


def test_every_residue_class_has_an_edge_of_three_windows():
    tw, counts = residue_world()
    assert [int(c) % 64 for c in counts] == list(RESIDUES)
    assert np.all(counts > 128), counts                                   # the carry crosses at least two window boundaries
