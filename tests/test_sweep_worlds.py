"""The worlds of tests/sweep_worlds.py are what they claim to be, on the oracle alone (no device): a device test over a world in
which no edge is hit, no chunk lies inside a box or no edge outruns 256 chunks would prove nothing.  Conditions, not measurements;
if a fleet misses a bar after a seed changes, the fleet changes, not the bar."""
import numpy as np
import pytest

import sweep_worlds as sw
from path_planner_amd.types import F_INFEASIBLE


def _shape(name):
    w, cpu, cchild = sw.oracle_records(name)
    feas = (cpu["flags"] & F_INFEASIBLE) == 0
    return w, cpu, cchild, feas, (cpu["info"] >> 16).astype(np.int64), cpu["collision_penalty"] / w.cfg.collision_penalty_factor


@pytest.mark.parametrize("name", ["fast", "reversed", "stamps"] + ["count%d" % n for n in sw.COUNTS] + ["count64+far"])
def test_fleet_hits_many_feasible_edges(name):
    w, cpu, _, feas, steps, hits = _shape(name)
    print(name, "feasible", int(feas.sum()), "of", len(cpu), "with hits", int((feas & (hits > 0)).sum()), "most hits", float(hits[feas].max()))
    assert len(cpu) == 1024
    assert int(feas.sum()) >= 300
    assert int((feas & (hits > 0)).sum()) >= 200


@pytest.mark.parametrize("name", sw.BINARY + ["done_inside"] + ["long%d" % s for s in sw.LONG_STEPS])
def test_binary_penalties_are_whole_hits(name):
    """penalty = hits x 600: every partial sum is an integer below 2^53, so the device tests may demand the same bits."""
    w, cpu, _, feas, steps, hits = _shape(name)
    assert w.cfg.collision_penalty_factor == 600.0
    assert np.array_equal(hits, np.round(hits)) and float(cpu["collision_penalty"].max()) < 2.0 ** 53


def test_count_fleets_are_prefixes_of_one_fleet():
    rows = sw.count(129).obst
    assert rows.shape == (129, 7)
    for n in sw.COUNTS:
        assert np.array_equal(sw.count(n).obst, rows[:n])
    far = sw.count64_far().obst
    assert far.shape == (65, 7) and np.array_equal(far[:64], rows[:64])
    assert abs(far[64, 0] - sw.C) >= 10000.0 and far[64, 3] == 0.0        # parked 10 km off the map
    assert float(np.abs(rows[:, 3]).max()) > 12.0 and int((rows[:, 4] > sw.T0).sum()) >= 4


def test_fast_and_reversed_are_the_same_tracks():
    wf, cf, _, feasf, _, hf = _shape("fast")
    wr, cr, _, feasr, _, hr = _shape("reversed")
    assert np.all(wf.obst[:, 3] >= 5.0) and float(wf.obst[:, 3].max()) > 15.0 and np.all(wf.obst[:, 4] == sw.T0)
    assert np.array_equal(wr.obst[:, 3], -wf.obst[:, 3]) and np.allclose(wr.obst[:, 2], wf.obst[:, 2] + np.pi)
    assert np.array_equal(wr.obst[:, [0, 1, 4, 5, 6]], wf.obst[:, [0, 1, 4, 5, 6]])
    # false positives must be able to show: feasible edges that no box touches
    assert int((feasf & (hf == 0)).sum()) >= 5 and int((feasr & (hr == 0)).sum()) >= 5
    # the same hit counts edge for edge (cos and sin of a yaw turned by pi are the negatives only up to rounding: an edge that grazes
    # a face may differ)
    assert np.array_equal(cf["flags"], cr["flags"])
    differ = feasf & (hf != hr)
    print("fast / reversed: feasible", int(feasf.sum()), "hit counts differ on", int(differ.sum()))
    assert int(differ.sum()) <= 0.01 * int(feasf.sum())


def test_stamps_has_rows_stamped_after_the_first_step_that_hit():
    w, cpu, _, feas, _, hits = _shape("stamps")
    late = np.nonzero(w.obst[:, 4] > sw.T0)[0]
    assert len(late) >= 4 and int((w.obst[:, 4] < sw.T0).sum()) >= 4
    seen = 0
    for j in late:
        other, _ = w.without_row(int(j)).oracle_cost()
        assert np.array_equal(other["flags"], cpu["flags"])
        changed = int((feas & (other["collision_penalty"] != cpu["collision_penalty"])).sum())
        print("row", int(j), "stamped", float(w.obst[j, 4]), "hits feasible edges:", changed)
        seen += changed > 0
    assert seen >= 1


def test_stacked_puts_steps_inside_several_boxes():
    w, cpu, _, feas, steps, hits = _shape("stacked")
    print("stacked: feasible", int(feas.sum()), "with more hits than steps", int((feas & (hits > steps)).sum()), "most hits", float(hits[feas].max()))
    assert int((feas & (hits > steps)).sum()) >= 1


def test_done_inside_ends_part_way_through_a_chunk_inside_both_boxes():
    w, cpu, _, feas, steps, hits = _shape("done_inside")
    horizon_steps = int(w.cfg.time_horizon / (w.cfg.collision_checking_increment / w.cfg.max_speed))
    nrib = (cpu["info"] >> 8) & 0xFF
    m = feas & (nrib == 0) & (steps < horizon_steps) & (steps % 64 != 0) & (hits == 2 * steps)
    print("done_inside:", int(m.sum()), "edges, steps", np.unique(steps[m]).tolist(), "configurations", np.unique(np.nonzero(m)[0] % 4).tolist())
    assert int(m.sum()) >= 30


@pytest.mark.parametrize("steps", sw.LONG_STEPS)
def test_long_edges_outrun_256_chunks(steps):
    w, cpu, cchild, feas, nsteps, hits = _shape("long%d" % steps)
    assert w.ng == steps + 8                                   # ppgpu_set_config: (int)steps + 8
    assert (w.ng + 63) // 64 == {16376: 256, 16377: 257, 16500: 258}[steps]
    assert int(nsteps.max()) == steps + 1
    full = feas & (nsteps == steps + 1)
    print("long", steps, "feasible", int(feas.sum()), "at the horizon", int(full.sum()), "beyond 8 192 steps", int((nsteps > 8192).sum()),
          "beyond 16 384", int((nsteps > 16384).sum()), "with hits", int((feas & (hits > 0)).sum()))
    # feasible edges that run to the horizon: past 16 384 steps wherever the horizon allows that (the 256-chunk row ends at 16 377)
    assert int(full.sum()) >= 5
    if steps + 1 > 16384:
        assert int((feas & (nsteps > 16384)).sum()) >= 5
    assert int((full & (hits > 0)).sum()) >= 1, "no long edge is hit: the hit sums over hundreds of chunks are not exercised"
