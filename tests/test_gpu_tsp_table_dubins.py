"""-m gpu: the device's exact subset table for the Dubins-TSP heuristics of long child ribbon lists (ppgpu_set_dubins_tsp_table,
path_planner_amd/csrc/pp_k_tsp_table.h) against the enumeration kernel on short lists — bit for bit: the table is filled over the
same Dubins lengths, from the device's own libm — against the numpy table of tests/test_tsp_table_dubins.py (the oracle's solver on
glibc: parity.REL_TOL, the project's bar) and the host's search on long ones, and through a costing launch."""
import numpy as np
import pytest

from parity import ABS_FLOOR, REL_TOL
from test_tsp_table import DBL_MAX, random_list
from test_tsp_table_dubins import H_DALL, H_DK, tsp_table_dubins

pytestmark = pytest.mark.gpu

F_OVF = 0x04


def _ctx(heuristic, K):
    from path_planner_amd import api
    from path_planner_amd.types import make_config
    cfg = make_config(heuristic=heuristic, tsp_k=K)
    ctx = api.Context(0)
    ctx.set_config(cfg)
    return ctx, cfg


def _table_h(cfg, rib, pose):
    """h as the device forms it: distance / max_speed * time_penalty_factor (the pose's heading goes where the callee says yaw)."""
    d = tsp_table_dubins(rib, cfg.heuristic, cfg.tsp_k, pose[0], pose[1], pose[2], cfg.ribbon_width, cfg.heuristic_turning_radius)
    return d / cfg.max_speed * cfg.time_penalty_factor


def _close(a, b):
    return abs(a - b) <= REL_TOL * max(abs(a), abs(b)) + ABS_FLOOR


def _cases(rng, sizes, per_size, w):
    poses, lists = [], []
    for n in sizes:
        for j in range(per_size):
            lists.append(random_list(rng, n, w))
            poses.append([*rng.uniform(0, 200, 2), rng.uniform(0, 2 * np.pi)])
    return np.array(poses), lists


@pytest.mark.parametrize("heuristic,K", [(H_DALL, 0), (H_DK, 2), (H_DK, 0)])
def test_table_is_the_enumeration_on_short_lists(heuristic, K):
    """Every list the enumeration kernel answers, answered again by the table (min_ribbons = 1 takes them all): the same h and flags
    bit for bit, nothing refused.  One list has two ribbons meeting at a point (a Dubins problem between two poses at one place)."""
    ctx, cfg = _ctx(heuristic, K)
    rng = np.random.default_rng(1000 * heuristic + K)
    poses, lists = _cases(rng, range(1, 9), 5, cfg.ribbon_width)
    lists[17][1, :2] = lists[17][0, 2:]                    # (a list of 4)
    h_off, f_off = ctx.heuristic_host(poses, lists)
    assert ctx.tsp_table_stats() == (0, 0)
    assert not np.any(f_off & F_OVF)                       # all within the enumeration's limit
    ctx.set_dubins_tsp_table(1, 16)
    h_on, f_on = ctx.heuristic_host(poses, lists)
    assert ctx.tsp_table_stats() == (len(lists), 0)
    assert h_on.tobytes() == h_off.tobytes() and np.array_equal(f_on, f_off)
    if K == 0 and heuristic == H_DK:
        assert np.all(h_on == DBL_MAX / cfg.max_speed * cfg.time_penalty_factor)
    else:
        for i in (0, 7, 17, 22, 39):                       # ... and the numpy table's value, to the bar
            assert _close(h_on[i], _table_h(cfg, lists[i], poses[i])), (i, h_on[i])
    ctx.close()


@pytest.mark.parametrize("heuristic,K,n", [(H_DALL, 0, 9), (H_DK, 2, 10), (H_DALL, 0, 13), (H_DK, 1, 16)])
def test_long_lists_get_the_exhaustive_value(heuristic, K, n):
    """Beyond the enumeration's 8 ribbons: with the switch off the record says PPGPU_F_RIBBON_OVF and h = 0; with (0, 16) the flag is
    clear and h is the numpy table's — and, at 9 and 10 ribbons where its search is exhaustive, the host's — within parity.REL_TOL
    (the device's Dubins lengths come from the device's libm)."""
    import hostlib
    ctx, cfg = _ctx(heuristic, K)
    rng = np.random.default_rng(77 * n + heuristic)
    poses, lists = _cases(rng, [n], 2, cfg.ribbon_width)
    h_off, f_off = ctx.heuristic_host(poses, lists)
    assert np.all(f_off & F_OVF) and np.all(h_off == 0.0)
    ctx.set_dubins_tsp_table(0, 16)
    h_on, f_on = ctx.heuristic_host(poses, lists)
    assert not np.any(f_on & F_OVF)
    assert ctx.tsp_table_stats() == (2, 0)
    for i in range(2):
        want = _table_h(cfg, lists[i], poses[i])
        print("n", n, "pose", i, "device", h_on[i], "numpy", want, "rel", abs(h_on[i] - want) / want)
        assert _close(h_on[i], want), (i, h_on[i], want)
        if n <= 10:
            hostlib.H.pph_set_ribbon_width(cfg.ribbon_width)
            h_host = hostlib.ribbons_heuristic(lists[i], heuristic, K, *poses[i], cfg.heuristic_turning_radius) / cfg.max_speed * cfg.time_penalty_factor
            assert _close(h_on[i], h_host), (i, h_on[i], h_host)
    ctx.set_dubins_tsp_table(0, 0)                         # off again: as before
    h_again, f_again = ctx.heuristic_host(poses, lists)
    assert np.array_equal(h_again, h_off) and np.array_equal(f_again, f_off)
    ctx.close()


@pytest.mark.parametrize("n", [9, 13])
def test_list_order_does_not_change_a_bit(n):
    """The same long list as given, reversed and randomly permuted, in one launch: identical bytes of h.  Every tour's sum is formed in
    the tour's own order over lengths that belong to pairs of points, so the set of leaves does not depend on the order of the list; a
    wrong combinadic rank or state index would, and would pass a tolerance."""
    ctx, cfg = _ctx(H_DALL, 0)
    rng = np.random.default_rng(5 + n)
    poses, lists = _cases(rng, [n], 1, cfg.ribbon_width)
    rib = lists[0]
    lists = [rib, rib[::-1].copy(), rib[rng.permutation(n)].copy()]
    poses = np.repeat(poses, 3, axis=0)
    ctx.set_dubins_tsp_table(0, 16)
    h, f = ctx.heuristic_host(poses, lists)
    assert not np.any(f & F_OVF) and ctx.tsp_table_stats() == (3, 0)
    assert h[0] > 0 and h[:1].tobytes() == h[1:2].tobytes() == h[2:].tobytes(), h
    assert _close(h[0], _table_h(cfg, rib, poses[0]))
    ctx.close()


def test_more_lists_than_workgroups_and_slots():
    """One launch of 1 100 lists of mixed lengths: more than the grid of 1 024 workgroups, and — the two 14-ribbon lists in the middle
    size the slots — some 220 slots, so every workgroup takes several records one after the other, its slot and its subset list reused
    across lengths.  The short ones against the enumeration, bit for bit; the two long ones against the numpy table."""
    ctx, cfg = _ctx(H_DALL, 0)
    rng = np.random.default_rng(9)
    poses, lists = _cases(rng, [int(v) for v in rng.integers(1, 9, 1098)], 1, cfg.ribbon_width)
    poses = list(poses)
    for at in (400, 700):
        p, l = _cases(rng, [14], 1, cfg.ribbon_width)
        poses.insert(at, p[0]); lists.insert(at, l[0])
    poses = np.array(poses)
    h_off, f_off = ctx.heuristic_host(poses, lists)
    ctx.set_dubins_tsp_table(1, 16)
    h_on, f_on = ctx.heuristic_host(poses, lists)
    assert ctx.tsp_table_stats() == (1100, 0)
    short = np.array([len(l) != 14 for l in lists])
    assert short.sum() == 1098
    assert h_on[short].tobytes() == h_off[short].tobytes() and np.array_equal(f_on[short], f_off[short])
    for i in (400, 700):
        assert (f_off[i] & F_OVF) and h_off[i] == 0.0
        assert not (f_on[i] & F_OVF) and _close(h_on[i], _table_h(cfg, lists[i], poses[i])), (i, h_on[i])
    ctx.close()


def test_through_a_costing_launch():
    """A costed edge whose child has 13-14 pieces, under TspDubinsNoSplitAllRibbons: with the switch on its record carries the h that
    ppgpu_heuristic_host gives for the returned child list and end pose under the same switch, bit for bit, f = g + h and the flag
    clear; the child ribbons and every other byte of the record are those of the switch-off call."""
    from path_planner_amd import api, workloads
    from path_planner_amd.types import edge_pack, F_INFEASIBLE
    from test_gpu_tsp_table import crossing_scene
    w = workloads.config1()
    w.cfg.heuristic, w.cfg.tsp_k = H_DALL, 2
    ribs = crossing_scene()
    root = workloads.root_vertex(110.0, 128.0, 0.0, 2.5, 1.0, ribs)
    e = edge_pack(np.array([0]), np.array([0]), np.array([1]))
    outs = []
    for on in (False, True):
        ctx = api.Context(0)
        ctx.set_config(w.cfg)
        ctx.set_grid(w.grid, w.res)
        ctx.set_obstacles(None)
        ctx.set_vertices(root, ribs)
        ctx.set_samples(np.array([112.0]), np.array([165.0]), np.array([0.05]))
        if on:
            ctx.set_dubins_tsp_table(0, 16)
        outs.append(ctx.cost_edges_host(e, stride=32))
        assert ctx.tsp_table_stats() == ((1, 0) if on else (0, 0))
        if on:
            r1, c1 = outs[1]
            n = int((r1["info"][0] >> 8) & 0xFF)
            h_alone, f_alone = ctx.heuristic_host([[r1["end_x"][0], r1["end_y"][0], r1["end_heading"][0]]], [c1[0, :n]])
            assert ctx.tsp_table_stats() == (2, 0) and not (f_alone[0] & F_OVF)
        ctx.close()
    (r0, c0), (r1, c1) = outs
    assert 13 <= n <= 16 and n == int((r0["info"][0] >> 8) & 0xFF)
    assert (r0["flags"][0] & F_OVF) and r0["h"][0] == 0.0 and not (r0["flags"][0] & F_INFEASIBLE)
    assert c0.tobytes() == c1.tobytes()
    assert r1["h"][0] > 0 and r1["h"].tobytes() == h_alone.tobytes()
    assert r1["f"][0] == r1["g"][0] + r1["h"][0] and r1["flags"][0] == (r0["flags"][0] & ~np.uint32(F_OVF))
    masked0, masked1 = r0.copy(), r1.copy()
    for r in (masked0, masked1):
        r["h"] = 0; r["f"] = 0; r["flags"] = 0
    assert masked0.tobytes() == masked1.tobytes()


def test_limits_and_the_heuristics_out_of_scope():
    from path_planner_amd import api
    rng = np.random.default_rng(4)
    ctx, cfg = _ctx(H_DK, 2)
    for bad in ((0, 17), (5, 4), (-1, 4)):
        with pytest.raises(api.PpgpuError, match=r"\(-1\)"):
            ctx.set_dubins_tsp_table(*bad)
    ctx.set_dubins_tsp_table(0, 16)
    poses, lists = _cases(rng, [17, 13], 1, cfg.ribbon_width)
    h, f = ctx.heuristic_host(poses, lists)
    assert (f[0] & F_OVF) and h[0] == 0.0                  # 17 ribbons: beyond the table too, left to the host
    assert not (f[1] & F_OVF) and _close(h[1], _table_h(cfg, lists[1], poses[1]))
    assert ctx.tsp_table_stats() == (1, 0)
    ctx.close()
    poses, lists = _cases(rng, [3, 10, 13], 2, cfg.ribbon_width)
    for heuristic in (0, 1, 2):                            # MaxDistance and the two point-robot heuristics: the other switch's
        ctx, cfg = _ctx(heuristic, 2)
        off = ctx.heuristic_host(poses, lists)
        ctx.set_dubins_tsp_table(1, 16)
        on = ctx.heuristic_host(poses, lists)
        assert on[0].tobytes() == off[0].tobytes() and np.array_equal(on[1], off[1])
        assert ctx.tsp_table_stats() == (0, 0)
        ctx.close()
