"""-m gpu: the device's exact subset table for the TSP heuristic of long child ribbon lists (ppgpu_set_tsp_table,
path_planner_amd/csrc/pp_k_tsp_table.h) against the enumeration kernels on short lists, against the numpy table of
tests/test_tsp_table.py (itself held to the oracle's literal recursion) on long ones, and through a costing launch."""
import numpy as np
import pytest

from test_tsp_table import DBL_MAX, H_ALL, H_K, mirror_pairs, random_list, tsp_table

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
    """(h, refused) as the device forms it: distance / max_speed * time_penalty_factor."""
    d, refused = tsp_table(rib, cfg.heuristic, cfg.tsp_k, pose[0], pose[1], cfg.ribbon_width)
    return d / cfg.max_speed * cfg.time_penalty_factor, refused


def _cases(rng, sizes, per_size, w, tied_every=0):
    poses, lists = [], []
    for n in sizes:
        for j in range(per_size):
            x, y = rng.uniform(0, 200, 2)
            tied = tied_every and n >= 2 and (len(lists) % tied_every) == tied_every - 1
            lists.append(mirror_pairs(n, x, y) if tied else random_list(rng, n, w))
            poses.append([x, y, rng.uniform(0, 2 * np.pi)])
    return np.array(poses), lists


@pytest.mark.parametrize("heuristic,K,sizes,per_size", [(H_ALL, 0, range(1, 9), 7), (H_K, 1, range(1, 13), 4), (H_K, 2, range(1, 13), 4),
                                                        (H_K, 3, range(1, 11), 4), (H_K, 0, [3], 4)])
def test_table_is_the_enumeration_on_short_lists(heuristic, K, sizes, per_size):
    """Every list the enumeration kernels answer, answered again by the table (min_ribbons = 1 takes them all): the same h and flags
    bit for bit.  A list the table refuses keeps the enumeration's record; there are exactly as many as the numpy rule says."""
    ctx, cfg = _ctx(heuristic, K)
    rng = np.random.default_rng(1000 * heuristic + K)
    poses, lists = _cases(rng, sizes, per_size, cfg.ribbon_width, tied_every=9 if heuristic == H_K and K > 0 else 0)
    h_off, f_off = ctx.heuristic_host(poses, lists)
    assert ctx.tsp_table_stats() == (0, 0)
    assert not np.any(f_off & F_OVF)                       # all within the enumeration's limits
    ctx.set_tsp_table(1, 16)
    h_on, f_on = ctx.heuristic_host(poses, lists)
    want = [_table_h(cfg, rib, p) for rib, p in zip(lists, poses)]
    refused = sum(1 for _, r in want if r)
    assert ctx.tsp_table_stats() == (len(lists) - refused, refused)
    assert h_on.tobytes() == h_off.tobytes() and np.array_equal(f_on, f_off)
    for i, (h, r) in enumerate(want):
        if not r:
            assert h == h_on[i], (i, len(lists[i]), h, h_on[i])
    if heuristic == H_K and K in (1, 3):
        assert refused > 0                                 # the mirror-pair lists: the tie straddles an odd K
    if heuristic == H_K and K == 0:
        assert np.all(h_on == DBL_MAX / cfg.max_speed * cfg.time_penalty_factor)
    ctx.close()


@pytest.mark.parametrize("heuristic,K,n,n_poses,host", [(H_ALL, 0, 9, 4, True), (H_ALL, 0, 10, 4, True), (H_ALL, 0, 13, 3, False), (H_ALL, 0, 16, 2, False),
                                                        (H_K, 2, 13, 3, True), (H_K, 2, 14, 3, False), (H_K, 2, 16, 2, False)])
def test_long_lists_get_the_exhaustive_value(heuristic, K, n, n_poses, host):
    """Beyond the enumeration: with the switch off the record says PPGPU_F_RIBBON_OVF and h = 0; with (0, 16) the flag is clear and h is
    the numpy table's, bit for bit — and, where the host's pruned search finishes within its node budget, the host's."""
    import hostlib
    ctx, cfg = _ctx(heuristic, K)
    rng = np.random.default_rng(77 * n + heuristic)
    poses, lists = _cases(rng, [n], n_poses, cfg.ribbon_width)
    h_off, f_off = ctx.heuristic_host(poses, lists)
    assert np.all(f_off & F_OVF) and np.all(h_off == 0.0)
    ctx.set_tsp_table(0, 16)
    h_on, f_on = ctx.heuristic_host(poses, lists)
    assert not np.any(f_on & F_OVF)
    assert ctx.tsp_table_stats() == (n_poses, 0)
    for i in range(n_poses):
        h, refused = _table_h(cfg, lists[i], poses[i])
        assert not refused and h == h_on[i], (i, h, h_on[i])
    if host:
        hostlib.H.pph_set_ribbon_width(cfg.ribbon_width)
        h_host = hostlib.ribbons_heuristic(lists[0], heuristic, K, poses[0][0], poses[0][1], poses[0][2]) / cfg.max_speed * cfg.time_penalty_factor
        assert h_host == h_on[0], (h_host, h_on[0])
    ctx.set_tsp_table(0, 0)                                # off again: as before
    h_again, f_again = ctx.heuristic_host(poses, lists)
    assert np.array_equal(h_again, h_off) and np.array_equal(f_again, f_off)
    ctx.close()


def test_a_tie_across_the_kth_place_is_refused():
    """13 ribbons in mirror pairs about the query point, K = 1: the two farthest keys are equal, the reference's choice hangs on list
    order, the table refuses — flag and h = 0 stay for the host, the refusal is counted.  The All variant has no such choice."""
    pose = np.array([[100.0, 100.0, 0.3]])
    rib = mirror_pairs(13, 100.0, 100.0)
    ctx, cfg = _ctx(H_K, 1)
    ctx.set_tsp_table(0, 16)
    h, f = ctx.heuristic_host(pose, [rib])
    assert (f[0] & F_OVF) and h[0] == 0.0
    assert ctx.tsp_table_stats() == (0, 1)
    assert _table_h(cfg, rib, pose[0])[1]
    ctx.close()
    ctx, cfg = _ctx(H_ALL, 0)
    ctx.set_tsp_table(0, 16)
    h, f = ctx.heuristic_host(pose, [rib])
    want, refused = _table_h(cfg, rib, pose[0])
    assert not refused and not (f[0] & F_OVF) and h[0] == want
    assert ctx.tsp_table_stats() == (1, 0)
    ctx.close()


def test_limits_and_the_heuristics_out_of_scope():
    from path_planner_amd import api
    rng = np.random.default_rng(4)
    ctx, cfg = _ctx(H_K, 2)
    with pytest.raises(api.PpgpuError, match=r"\(-1\)"):
        ctx.set_tsp_table(0, 17)
    with pytest.raises(api.PpgpuError, match=r"\(-1\)"):
        ctx.set_tsp_table(5, 4)
    with pytest.raises(api.PpgpuError, match=r"\(-1\)"):
        ctx.set_tsp_table(-1, 4)
    ctx.set_tsp_table(0, 16)
    poses, lists = _cases(rng, [17, 13], 1, cfg.ribbon_width)
    h, f = ctx.heuristic_host(poses, lists)
    assert (f[0] & F_OVF) and h[0] == 0.0                  # 17 ribbons: beyond the table too, left to the host
    assert not (f[1] & F_OVF) and h[1] == _table_h(cfg, lists[1], poses[1])[0]
    assert ctx.tsp_table_stats() == (1, 0)
    ctx.set_tsp_table(0, 12)                               # a smaller range: the 13 are out of it
    h, f = ctx.heuristic_host(poses, lists)
    assert np.all(f & F_OVF) and np.all(h == 0.0)
    ctx.close()
    poses, lists = _cases(rng, [3, 10, 13], 2, cfg.ribbon_width)
    for heuristic in (0, 3, 4):                            # MaxDistance and the two Dubins-TSP heuristics: not touched
        ctx, cfg = _ctx(heuristic, 2)
        off = ctx.heuristic_host(poses, lists)
        ctx.set_tsp_table(1, 16)
        on = ctx.heuristic_host(poses, lists)
        assert on[0].tobytes() == off[0].tobytes() and np.array_equal(on[1], off[1])
        assert ctx.tsp_table_stats() == (0, 0)
        ctx.close()

@pytest.mark.parametrize("K", [1, 0])
def test_more_lists_than_workgroups_and_slots(K):
    """One launch of 1 300 lists of mixed lengths: more than the grid of 1 024 workgroups, and — the two 14-ribbon lists size the
    slots — some 220 slots, so every workgroup takes several records one after the other: its slot and its subset list are reused
    across lengths, refused lists (every ninth: mirror pairs, K = 1) sit between answered ones.  Against the enumeration, bit for bit;
    the two long lists against the numpy table.  K = 0: every record takes the short way out (DBL_MAX)."""
    ctx, cfg = _ctx(H_K, K)
    rng = np.random.default_rng(9 + K)
    sizes = [int(v) for v in rng.integers(1, 9, 1298)]
    poses, lists, mirrored = [], [], []
    for i, n in enumerate(sizes):
        p, l = _cases(rng, [n], 1, cfg.ribbon_width)
        mirrored.append(K > 0 and i % 9 == 8 and n >= 2)
        if mirrored[-1]:
            l = [mirror_pairs(n, p[0][0], p[0][1])]
        poses.append(p[0]); lists.append(l[0])
    for at in (400, 900):                                      # the long ones in the middle of the list
        p, l = _cases(rng, [14], 1, cfg.ribbon_width)
        poses.insert(at, p[0]); lists.insert(at, l[0]); mirrored.insert(at, False)
    poses = np.array(poses)
    long_ones = [i for i, l in enumerate(lists) if len(l) == 14]
    # (random coordinates tie nowhere — tests/test_tsp_table.py — so only the mirrored lists are asked; a refusal elsewhere shows in the counts)
    tied = [i for i, l in enumerate(lists) if mirrored[i] and _table_h(cfg, l, poses[i])[1]]
    h_off, f_off = ctx.heuristic_host(poses, lists)
    ctx.set_tsp_table(1, 16)
    h_on, f_on = ctx.heuristic_host(poses, lists)
    assert ctx.tsp_table_stats() == (len(lists) - len(tied), len(tied))
    short = np.array([i not in long_ones for i in range(len(lists))])
    assert h_on[short].tobytes() == h_off[short].tobytes() and np.array_equal(f_on[short], f_off[short])
    assert K == 0 or len(tied) >= 50
    for i in long_ones:
        assert not (f_on[i] & F_OVF) and h_on[i] == _table_h(cfg, lists[i], poses[i])[0]
        assert K == 0 or ((f_off[i] & F_OVF) and h_off[i] == 0.0)
    ctx.close()


def crossing_scene():
    """Seven parallel ribbons crossed near their western ends by one coverage edge going north (the geometry of
    test_gpu_parity.py::test_long_child_ribbon_list_gets_its_heuristic_on_the_host), spacings and ends irregular so that no keys tie.
    (The edge must not end on the line it crossed them on: the two pieces of a split ribbon end symmetrically about the crossing, and
    from a point on that line their keys are equal — the edge of the test below bears a little east.)"""
    dy = np.cumsum([0.0, 3.5, 3.31, 3.74, 3.43, 3.62, 3.27])
    dx0 = np.array([0.0, 0.21, -0.17, 0.33, -0.29, 0.11, -0.07])
    dx1 = np.array([0.0, 1.3, -2.1, 0.7, 2.9, -1.6, 0.4])
    return np.column_stack([108.0 + dx0, 131.0 + dy, 148.0 + dx1, 131.0 + dy])


def test_through_a_costing_launch():
    """A costed edge whose child has 13-14 pieces: with the switch on its record carries the table's h (of the returned child list and
    end pose) and f = g + h with the flag clear; the child ribbons and every other byte of the record are those of the switch-off call."""
    from path_planner_amd import api, workloads
    from path_planner_amd.types import edge_pack, F_INFEASIBLE
    import oracle as orc
    w = workloads.config1()
    w.cfg.heuristic, w.cfg.tsp_k = 2, 2
    ribs = crossing_scene()
    root = workloads.root_vertex(110.0, 128.0, 0.0, 2.5, 1.0, ribs)
    e = edge_pack(np.array([0]), np.array([0]), np.array([1]))
    world = orc.World(w.cfg, w.grid, w.res, None)
    cpu, cchild = world.cost_edges(root, ribs, np.array([112.0]), np.array([165.0]), np.array([0.05]), e, stride=32)
    n_cpu = int((cpu["info"][0] >> 8) & 0xFF)
    assert 13 <= n_cpu <= 16
    outs = []
    for on in (False, True):
        ctx = api.Context(0)
        ctx.set_config(w.cfg)
        ctx.set_grid(w.grid, w.res)
        ctx.set_obstacles(None)
        ctx.set_vertices(root, ribs)
        ctx.set_samples(np.array([112.0]), np.array([165.0]), np.array([0.05]))
        if on:
            ctx.set_tsp_table(0, 16)
        outs.append(ctx.cost_edges_host(e, stride=32))
        assert ctx.tsp_table_stats() == ((1, 0) if on else (0, 0))
        ctx.close()
    (r0, c0), (r1, c1) = outs
    n = int((r0["info"][0] >> 8) & 0xFF)
    assert n == n_cpu and (r0["flags"][0] & F_OVF) and r0["h"][0] == 0.0 and not (r0["flags"][0] & F_INFEASIBLE)
    assert c0.tobytes() == c1.tobytes()
    h, refused = _table_h(w.cfg, c1[0, :n], (r1["end_x"][0], r1["end_y"][0]))
    assert not refused
    assert r1["h"][0] == h and r1["f"][0] == r1["g"][0] + h and r1["flags"][0] == (r0["flags"][0] & ~np.uint32(F_OVF))
    masked0, masked1 = r0.copy(), r1.copy()
    for r in (masked0, masked1):
        r["h"] = 0; r["f"] = 0; r["flags"] = 0
    assert masked0.tobytes() == masked1.tobytes()
