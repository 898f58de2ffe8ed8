"""-m gpu: the small algorithms of path_planner_amd/csrc/pp_k_expand.h, each alone (tests/probe/pp_expand_probe.hip), against plain
references: libstdc++'s own std::push_heap / std::pop_heap for the heap steps of the push-order replay (oracle.heap_replay /
heap_noop), np.lexsort for every selection, set arithmetic for the compaction.  Every comparison is exact.

The inputs are what a random world never produces and the pieces exist for: costs and distances that tie, index arrays that disagree
with list positions, lists around every size at which the code takes another path."""
import numpy as np
import pytest

import expand_probe as ep
import oracle as orc

pytestmark = pytest.mark.gpu

PAD = 0x7fffffff


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    """As in every GPU module: the GPU is there, and torch has met it before a library of ours opens it (in a process where the
    probe came first, torch.cuda.is_available() answers False afterwards)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---------------------------------------------------------------------------------------------- heap steps, pp_ord_safe
HEAP_KS = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 62, 63]
ALPHABETS = [1, 2, 3, 5, 0]            # distinct cost values; 0 = every cost distinct
SEEDS = 3


def _heap_cases():
    cases = []
    for k in HEAP_KS:
        n = 4 * k + 7
        for letters in ALPHABETS:
            for order in ("random", "ascending", "descending"):
                for seed in range(SEEDS):
                    rng = np.random.default_rng([k, letters, seed, len(order)])
                    c = rng.choice(rng.uniform(1.0, 2.0, letters), n) if letters else rng.permutation(n) * 0.25 + 1.0
                    if order == "ascending":
                        c = np.sort(c)
                    elif order == "descending":
                        c = np.sort(c)[::-1].copy()
                    cases.append({"k": k, "letters": letters, "order": order, "seed": seed, "cost": c})
    return cases


@pytest.fixture(scope="module")
def heap_runs():
    """Every case once through the device (one launch) and once through libstdc++."""
    cases = _heap_cases()
    dev = ep.heap_replay([c["cost"] for c in cases], [c["k"] for c in cases])
    for c, (arr, safe) in zip(cases, dev):
        c["dev"], c["safe"] = arr, safe
        c["ref"], c["equal_children"] = orc.heap_replay(c["cost"], c["k"])
    return cases


def test_heap_steps_are_libstdcxx_after_every_operation(heap_runs):
    """pp_ord_sift_up / pp_ord_pop driven as the scan drives them: the heap array equals std::push_heap / std::pop_heap's after every
    single operation, with one, two, three and five distinct costs (ties everywhere) and with none."""
    for c in heap_runs:
        bad = np.nonzero((c["dev"] != c["ref"]).any(axis=1))[0]
        assert bad.size == 0, (f"k {c['k']} alphabet {c['letters']} {c['order']} seed {c['seed']}: the heap array differs after operation "
                               f"{bad[0]} (cost {c['cost'][bad[0]]!r}): device {c['dev'][bad[0]].tolist()} libstdc++ {c['ref'][bad[0]].tolist()}")
    # the references are not the trivial answer: tied cases end in arrays that are not ascending (cost, index) ...
    for k in HEAP_KS:
        if k < 3:
            continue
        differs = 0
        for c in heap_runs:
            if c["k"] == k and c["letters"]:
                final = c["ref"][-1]
                asc = np.sort(final)[np.lexsort((np.sort(final), c["cost"][np.sort(final)]))]
                differs += int(not np.array_equal(final, asc))
        assert differs > 0, k
    # ... and pops did meet two children of equal cost (the RIGHT one is taken)
    met = sum(c["equal_children"] for c in heap_runs if c["letters"])
    assert met > 0
    assert all(c["equal_children"] == 0 for c in heap_runs if not c["letters"])
    print(f"heap replay: {len(heap_runs)} cases, {sum(len(c['cost']) for c in heap_runs)} operations, {met} pops met two equal children")


def test_ord_safe_never_calls_a_heap_safe_that_a_push_and_pop_would_change(heap_runs):
    """pp_ord_safe is the licence to skip a candidate above the root.  One direction is exact: where it says safe, pushing an entry
    strictly above the root (the next double, and 1e300) and popping leaves libstdc++'s array as it was.  It may say unsafe of a heap
    that would survive (the rule is conservative); with distinct costs it never does."""
    n_safe = n_unsafe = n_unsafe_unchanged = 0
    for c in heap_runs:
        k, cost = c["k"], c["cost"]
        assert (c["safe"][:k - 1] == -1).all() and np.isin(c["safe"][k - 1:], (0, 1)).all(), (k, c["safe"])
        for i in range(k - 1, len(cost)):
            hc = cost[c["dev"][i]]
            unchanged = [orc.heap_noop(hc, np.nextafter(hc[0], np.inf)), orc.heap_noop(hc, 1e300)]
            if c["safe"][i] == 1:
                n_safe += 1
                assert all(unchanged), (f"k {k} alphabet {c['letters']} {c['order']} seed {c['seed']} after operation {i}: pp_ord_safe says "
                                        f"safe, a push above the root and a pop change the array; costs in array order {hc.tolist()}")
            else:
                n_unsafe += 1
                n_unsafe_unchanged += int(all(unchanged))
                assert c["letters"], (k, i, "unsafe with pairwise distinct costs")
    print(f"pp_ord_safe: safe {n_safe}, unsafe {n_unsafe}, of which the array would not have changed {n_unsafe_unchanged}")
    assert n_safe > 0 and n_unsafe > 0
    tied_safe = sum(int((c["safe"] == 1).sum()) for c in heap_runs if c["letters"] > 1)
    assert tied_safe > 0                     # both verdicts occur among the tied alphabets themselves


# ---------------------------------------------------------------------------------------------- selections
SEL_N = [0, 1, 63, 64, 65, 255, 256, 257, 600]
SEL_K = [1, 2, 9, 32, 33, 63, 64, 300]


def _sizes(k, cap=None):
    ns = sorted(set(SEL_N + [max(k - 1, 0), k, k + 1]))
    return [n for n in ns if cap is None or n <= cap]


def _tied_values(rng, n, inf_share=0.15):
    """n values from a handful of distinct ones (heavy ties), some of them +inf."""
    x = rng.choice(rng.uniform(1.0, 50.0, max(1, n // 6)), n) if n else np.zeros(0)
    x[rng.random(n) < inf_share] = np.inf
    return x


def _pair_less(l1, i1, l2, i2):
    """The documented order of every selection: by length, equal lengths by index; index < 0 = no entry, after everything."""
    return (i1 >= 0) & ((i2 < 0) | (l1 < l2) | ((l1 == l2) & (i1 < i2)))


@pytest.mark.parametrize("with_index", [True, False], ids=["index_array", "by_position"])
def test_rank_lds_counts_the_pairs_before(with_index):
    rng = np.random.default_rng(21)
    for n in SEL_N + [1024]:
        L = _tied_values(rng, n)
        I = rng.permutation(n).astype(np.int32) if with_index else np.arange(n, dtype=np.int32)
        if with_index and n:
            gone = rng.random(n) < 0.1                       # no entry: index -1 (its length is whatever was there)
            I[gone] = -1
        # queries: every entry of the list itself, and strangers: values of the alphabet with other indices, -1, +inf
        x = np.concatenate([L, rng.choice(L, 40) if n else np.full(40, 3.0), [np.inf, 0.0, 1e9]])
        xi = np.concatenate([I, rng.integers(-1, n + 5, 40), [5, -1, 0]]).astype(np.int32)
        got = ep.rank_lds(L, I if with_index else None, x, xi)
        want = _pair_less(L[None, :], I[None, :], x[:, None], xi[:, None]).sum(axis=1)
        assert np.array_equal(got, want), (n, np.nonzero(got != want)[0][:5])
        if with_index and n >= 63:
            by_pos = _pair_less(L[None, :], np.arange(n)[None, :], x[:, None], xi[:, None]).sum(axis=1)
            assert not np.array_equal(want, by_pos)          # ties by index and ties by position are different answers here


@pytest.mark.parametrize("with_index", [True, False], ids=["index_array", "by_position"])
def test_kth_smallest_lds(with_index):
    """The k-th smallest finite pair -> the outputs; fewer than k finite ones: the outputs stay what they were."""
    rng = np.random.default_rng(22)
    SL, SI = -123.5, -77
    Ls, Is, ks, want = [], [], [], []
    for k in SEL_K:
        for n in _sizes(k, 1024):
            L = _tied_values(rng, n)
            I = rng.permutation(n).astype(np.int32) + 3 if with_index else np.arange(n, dtype=np.int32)
            if with_index:
                I[~np.isfinite(L)] = -1                      # as pp_k_select_nearest fills it: no entry = (+inf, -1)
            fin = np.nonzero(np.isfinite(L))[0]
            order = fin[np.lexsort((I[fin], L[fin]))]
            Ls.append(L); Is.append(I); ks.append(k)
            want.append((L[order[k - 1]], I[order[k - 1]]) if k <= len(order) else (SL, SI))
    gl, gi = ep.kth_lds(Ls, Is if with_index else None, ks, SL, SI)
    kept = 0
    for j, (wl, wi) in enumerate(want):
        assert gl[j] == wl and gi[j] == wi, (ks[j], len(Ls[j]), gl[j], gi[j], wl, wi)
        kept += int(wi == SI)
    assert 0 < kept < len(want)


def test_kth_smallest_wave():
    """One value per lane, the first n lanes count, ties by lane, every lane gets the answer; +inf with fewer than k finite."""
    rng = np.random.default_rng(23)
    xs, ns, ks, want = [], [], [], []
    for k in [k for k in SEL_K if k <= 64]:
        for n in _sizes(k, 64):
            x = np.full(64, 0.5)                             # lanes beyond n hold something smaller than everything: not to be counted
            x[:n] = _tied_values(rng, n)
            fin = np.sort(x[:n][np.isfinite(x[:n])])
            xs.append(x); ns.append(n); ks.append(k)
            want.append(fin[k - 1] if k <= len(fin) else np.inf)
    got = ep.kth_wave(np.array(xs), ns, ks)
    for j, w in enumerate(want):
        assert (got[j] == w).all(), (ks[j], ns[j], got[j], w)
    assert 0 < sum(int(np.isinf(w)) for w in want) < len(want)


@pytest.mark.parametrize("nt", [256, 64])
def test_k_smallest_in_ascending_length_then_index(nt):
    """pp_k_smallest: the k smallest entries in ascending (length, index), -1 / -1.0 where the entries run out — written for every
    slot, by whichever thread owns it.  Entries that do not count: flagged invalid, or of negative length."""
    rng = np.random.default_rng(24 + nt)
    Ls, Is, Vs, ks, want = [], [], [], [], []
    for k in SEL_K:
        for n in _sizes(k):
            L = _tied_values(rng, n)
            V = (rng.random(n) < 0.8).astype(np.uint8)
            L[rng.random(n) < 0.1] = -1.0                    # closer than the increment: not an entry
            I = (rng.permutation(n) * 3 + 1).astype(np.int32)     # positions and indices disagree
            ok = np.nonzero((V != 0) & (L >= 0))[0]
            order = ok[np.lexsort((I[ok], L[ok]))][:k]
            wi, wl = np.full(k, -1, dtype=np.int32), np.full(k, -1.0)
            wi[:len(order)] = I[order]; wl[:len(order)] = L[order]
            Ls.append(L); Is.append(I); Vs.append(V); ks.append(k); want.append((wi, wl))
    # a tail far longer than thread 0's share: k = 300 over 3 entries, and over none
    for n in (3, 0):
        L, I, V = np.array([2.0, 1.0, 2.0])[:n], np.array([9, 4, 7], dtype=np.int32)[:n], np.ones(n, dtype=np.uint8)
        wi, wl = np.full(300, -1, dtype=np.int32), np.full(300, -1.0)
        wi[:n] = [4, 7, 9][:n]; wl[:n] = [1.0, 2.0, 2.0][:n]
        Ls.append(L); Is.append(I); Vs.append(V); ks.append(300); want.append((wi, wl))
    for with_len in (True, False):
        got = ep.k_smallest(nt, Ls, Is, Vs, ks, with_lengths=with_len)
        short = 0
        for j, (wi, wl) in enumerate(want):
            gi, gl = got[j]
            assert np.array_equal(gi, wi), (nt, ks[j], len(Ls[j]), gi[:12], wi[:12])
            if with_len:
                assert gl.tobytes() == wl.tobytes(), (nt, ks[j], len(Ls[j]), gl[:12], wl[:12])
            short += int(wi[-1] < 0)
        assert 0 < short < len(want)


def test_half_wave_min():
    rng = np.random.default_rng(25)
    x = rng.choice(rng.uniform(-5, 5, 40), 64 * 9 + 17)
    x[rng.random(x.size) < 0.2] = np.inf
    x[64:96] = np.inf                                         # a half wave with no finite value at all
    got, padded = ep.half_wave_min(x)
    want = np.repeat(padded.reshape(-1, 32).min(axis=1), 32)[:x.size]
    assert got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- pp_wg_append
@pytest.mark.parametrize("one_list", [True, False], ids=["8_flags_one_list", "2_flags_two_lists"])
@pytest.mark.parametrize("nwg", [1, 5])
@pytest.mark.parametrize("density", [0.0, 1 / 64, 0.5, 1.0])
def test_wg_append_hands_out_every_slot_once(one_list, nwg, density):
    R, lists = (8, 1) if one_list else (2, 2)
    rng = np.random.default_rng([nwg, int(density * 64), R])
    take = (rng.random((nwg, R, 256)) < density).astype(np.uint8)
    if density == 0.5 and nwg == 5:
        take[2] = 0                                           # an all-false workgroup among busy ones
        take[3, :, 64:] = 0                                   # one whose flags all sit in wave 0
    c0 = np.array([37] if one_list else [11, 1000], dtype=np.int32)
    totals = np.array([int(take.sum())] if one_list else [int(take[:, 0].sum()), int(take[:, 1].sum())])
    cap = int((c0 + totals).max()) + 8
    count, out, bad = ep.wg_append(one_list, take, c0, cap)
    assert bad == 0
    assert count.tolist() == (c0 + totals).tolist()           # (density 0: no workgroup adds anything, the counters stay)
    for l in range(lists):
        ids = out[l]
        used = np.nonzero(ids >= 0)[0]
        assert used.tolist() == list(range(c0[l], c0[l] + totals[l])), (l, used[:5], c0[l], totals[l])
        wg, flag, thread = ids[used] // (R * 256), (ids[used] // 256) % R, ids[used] % 256
        # exactly the taken flags of this list, each once
        mine = np.nonzero(take if one_list else take[:, l:l + 1])
        want_ids = (mine[0] * R + (mine[1] if one_list else l)) * 256 + mine[2]
        assert np.array_equal(np.sort(ids[used]), np.sort(want_ids))
        if one_list:
            # one atomic per workgroup: its flags occupy one contiguous range, in flag order
            for g in range(nwg):
                at = used[wg == g]
                if at.size:
                    assert at.max() - at.min() + 1 == at.size, g
                    assert (np.diff(flag[wg == g][np.argsort(at)]) >= 0).all(), g


# ---------------------------------------------------------------------------------------------- pp_ord_sort
@pytest.mark.parametrize("Mk", [0, 1, 2, 63, 64, 65, 1000, 4097, 8192])
def test_ord_sort_by_distance_then_sample(Mk):
    """The kept candidates sorted by (distance, SAMPLE index): equal distances are common, the list's positions are not in sample
    order, and the padding the bitonic network needs never comes before a candidate."""
    rng = np.random.default_rng(300 + Mk)
    M = Mk + Mk // 3 + 5
    val = (rng.permutation(M) * 2 + 1).astype(np.int32)                 # the list's samples, shuffled
    ci = rng.permutation(M)[:Mk].astype(np.int32)                       # kept positions, in arrival order
    cd = rng.choice(rng.uniform(1.0, 90.0, max(1, Mk // 8)), Mk) if Mk else np.zeros(0)
    ocd, oci = ep.ord_sort(cd, ci, val)
    order = np.lexsort((val[ci], cd))
    assert (oci[:Mk] != PAD).all()
    assert ocd[:Mk].tobytes() == cd[order].tobytes() and np.array_equal(oci[:Mk], ci[order]), Mk
    assert np.isinf(ocd[Mk:]).all() and (oci[Mk:] == PAD).all()
    if Mk >= 63:
        by_position = np.lexsort((ci, cd))
        assert not np.array_equal(ci[order], ci[by_position])          # sorting equal distances by list position is another answer


# ---------------------------------------------------------------------------------------------- pp_k_expand_bound
@pytest.mark.parametrize("k", [1, 9, 40])
def test_expand_bound_ranks_runs_of_groups(k):
    """U = the k-th smallest group minimum; with more than PP_BOUND_CAP = 512 groups, of the minima of runs of consecutive groups (as
    many per run as it takes to get down to 512).  Fewer than k near slots, or fewer than k runs with a valid sample: +inf."""
    rng = np.random.default_rng(60 + k)
    infinite = finite = 0
    for near in [0, 1, 31, 32, 33, 32 * k - 1, 32 * k, 512 * 32 - 5, 512 * 32, 512 * 32 + 1, 1024 * 32, 1024 * 32 + 1, 1300 * 32 + 7]:
        for empty_share in (0.0, 0.6, 1.0):
            ngrp = (near + 31) // 32
            gm = rng.choice(rng.uniform(5.0, 90.0, max(1, ngrp // 3)), (ngrp, 2))           # tied minima
            gm[rng.random((ngrp, 2)) < empty_share] = np.inf                                  # groups without a valid sample
            gc = np.full(ngrp, 32, dtype=np.int32)
            if ngrp:
                gc[-1] = near - 32 * (ngrp - 1)
            U, count = ep.expand_bound(gm, gc, near, k)
            assert count.tolist() == [0, 0]
            per = -(-ngrp // 512) if ngrp else 0
            for r in range(2):
                want = np.inf
                if near >= k and ngrp:
                    runs = [gm[j:j + per, r].min() for j in range(0, ngrp, per)]
                    fin = np.sort([x for x in runs if np.isfinite(x)])
                    if len(fin) >= k:
                        want = fin[k - 1]
                assert U[r] == want, (k, near, empty_share, r, U[r], want)
                infinite += int(np.isinf(want)); finite += int(np.isfinite(want))
                if np.isfinite(want) and per > 1:
                    # the bound it stands for: at least k samples are not longer
                    assert (gm[:, r] <= want).sum() >= k
    assert infinite > 0 and finite > 0
