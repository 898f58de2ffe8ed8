"""The oracle's pieces behind the expand-order tests, on the CPU: the scan that visits by (distance, sample index) against the
reference's own visit order where distances are distinct, and the bare heap replay against what a heap of the k smallest must be."""
import numpy as np
import pytest

import oracle as orc


@pytest.mark.parametrize("cfgname,n_samples", [("cfg1", 64), ("cfg2", 300), ("cfg2", 4096)])
def test_by_index_scan_is_the_reference_scan_on_distinct_distances(cfgname, n_samples):
    from path_planner_amd import workloads
    w = workloads.by_name(cfgname)
    world = orc.World(w.cfg, w.grid, w.res, w.obst)
    cs = world.add_samples(w.bounds6, w.seed, w.ribbons4, 0, n_samples)
    root = np.asarray(w.start5, dtype=np.float64)
    # the root and a few child poses: samples themselves, as reached at the end of an edge
    srcs = [root] + [np.array([cs[i, 0], cs[i, 1], cs[i, 2], w.cfg.max_speed, root[4] + 10.0 + i]) for i in (0, len(cs) // 3, len(cs) - 1)]
    compared = 0
    for src in srcs:
        d = np.hypot(cs[:, 0] - src[0], cs[:, 1] - src[1])
        assert len(np.unique(d)) == len(d)                      # untied input: both visit orders are defined and equal
        for k in (5, 9):
            a = world.expand_order(src, cs[:, 0], cs[:, 1], cs[:, 2], k)
            b = world.expand_order_by_index(src, cs[:, 0], cs[:, 1], cs[:, 2], k)
            assert np.array_equal(a, b), (cfgname, src, k, a, b)
            assert (a[0] >= 0).sum() == min(k, int((d > w.cfg.collision_checking_increment).sum()))
            compared += 1
    assert compared == 8


def _alphabet_costs(rng, n, letters):
    return rng.choice(rng.uniform(1.0, 2.0, letters), n) if letters else rng.permutation(n).astype(np.float64)


@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 17, 33, 63])
def test_heap_replay_keeps_a_heap_of_the_k_smallest(k):
    rng = np.random.default_rng(100 + k)
    met_equal = 0
    for letters in (1, 2, 3, 5, 0):
        c = _alphabet_costs(rng, 4 * k + 7, letters)
        arr, eq = orc.heap_replay(c, k)
        met_equal += eq
        assert arr.shape == (len(c), k)
        for i in range(len(c)):
            h = arr[i]
            m = min(i + 1, k)
            assert (h[:m] >= 0).all() and (h[m:] == -1).all() and len(set(h[:m].tolist())) == m and (h[:m] <= i).all()
            hc = c[h[:m]]
            for q in range(1, m):
                assert not (hc[(q - 1) // 2] < hc[q]), (k, letters, i, q)      # a max-heap under cost <
            # the k smallest costs seen so far, as a multiset
            assert np.array_equal(np.sort(hc), np.sort(c[:i + 1])[:m]), (k, letters, i)
        if letters == 0:
            assert eq == 0
    if k >= 3:
        assert met_equal > 0


def test_heap_noop_on_distinct_and_on_tied_heaps():
    # distinct costs: a push above the root and the pop undo each other
    assert orc.heap_noop([5.0, 4.0, 3.0, 2.0, 1.0], 6.0)
    assert orc.heap_noop([5.0, 4.0, 3.0, 2.0, 1.0], 1e300)
    # k = 3: the push moves the root down to slot 1 (a left child); its right sibling, slot 2, equals it: the pop's hole goes right
    assert not orc.heap_noop([5.0, 4.0, 5.0], 6.0)
    assert orc.heap_noop([5.0, 4.0, 4.0], 6.0)
    # k = 2: slot 2 is a right child whose left sibling equals their parent
    assert not orc.heap_noop([4.0, 4.0], 6.0)
