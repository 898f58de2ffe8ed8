"""CPU: the input sets of tests/test_gpu_cover_pieces.py (tests/cover_probe_inputs.py) are deterministic, stay within the 64 lanes, and
hold every class the GPU tests rely on, named from the reference's own replay, so that no GPU test passes vacuously.  Each test prints
its per-class counts (pytest -s shows them)."""
import collections

import numpy as np
import pytest

import cover_probe_inputs as ci
import oracle as orc


@pytest.fixture(scope="module")
def events():
    return list(zip(ci.event_cases(), ci.event_reference()))


@pytest.fixture(scope="module")
def runs():
    return ci.run_cases()


def _of(events, cls):
    return [(c, r) for c, r in events if c["cls"] == cls]


def _show(title, counter):
    print(f"\n{title}:")
    for k in sorted(counter, key=str):
        print(f"  {k}: {counter[k]}")


def _case_bytes(c):
    return c["list"].tobytes() + c["events"].tobytes() + np.float64(c["w"]).tobytes()


def test_event_cases_are_deterministic_and_within_the_lanes(events):
    again = ci.event_cases.__wrapped__()
    assert len(again) == len(events)
    assert all(_case_bytes(a) == _case_bytes(c) for a, (c, _) in zip(again, events))
    total = sum(len(c["events"]) for c, _ in events)
    _show("events per class", collections.Counter({k: sum(len(c["events"]) for c, _ in _of(events, k)) for k in {c["cls"] for c, _ in events}}))
    print(f"  cases {len(events)}, events {total}")
    assert total <= 20000
    for c, recs in events:
        assert len(c["list"]) <= ci.WAVE and c["w"] in ci.WIDTHS
        assert len(c["events"]) <= (ci.WAVE if c["cls"] == "sequence" else 8)
        assert all(len(r["before"]) <= ci.WAVE for r in recs)
        assert np.isfinite(c["events"]).all() and np.isfinite(c["list"]).all()
    assert orc.O.ppo_get_ribbon_width() == ci.DEFAULT_WIDTH


def test_orientation_set(events):
    cnt = collections.Counter()
    names, lengths = set(), set()
    for c, recs in _of(events, "orientation"):
        names.add(c["name"])
        r = c["list"][0]
        lengths.add(round(float(np.hypot(r[2] - r[0], r[3] - r[1])), 3))
        grow = c["w"] + 1e-3
        for kind, (x, y, cov), rec in zip(c["kinds"], c["events"], recs):
            inbox = ci.in_grown_box(rec["before"][0], x, y, grow) if len(rec["before"]) else False
            changed = rec["what"] != ("none",)
            cnt[(c["sub"], kind, "contained" if rec["D"] == 0.0 else "apart", "changed" if changed else "same")] += 1
            if kind == "far":
                assert not inbox and rec["D"] > 900.0 and not changed
            if kind in ("outside", "before", "beyond"):
                assert rec["D"] > 0.0 and not changed
            if kind == "nonstrict" and len(rec["before"]) == 1:
                assert rec["D"] == 0.0 and not changed
            if kind == "inside":
                assert rec["D"] == 0.0 and changed == bool(cov)
    _show("orientation (class, point, minDistanceFrom, list)", cnt)
    assert names == {o[0] for o in ci.ORIENTS} and len(names) == 22
    assert 400.0 in lengths and min(lengths) < 2 * max(ci.WIDTHS) + 0.01
    for ocls in ("axis", "345", "oblique"):
        assert cnt[(ocls, "inside", "contained", "changed")] >= 4 and cnt[(ocls, "far", "apart", "same")] >= 8


def test_knife_edges_show_both_outcomes(events):
    cnt = collections.Counter()
    for c, recs in _of(events, "knife"):
        cnt[(c["sub"][0], c["sub"][1], bool(ci.knife_outcome(c, recs[0])))] += 1
    _show("knife edges (comparison, orientation, outcome)", cnt)
    for comp in ci.KNIFE_HALF:
        for oname, _ in ci.KNIFE_ORIENTS:
            assert cnt[(comp, oname, True)] >= 5 and cnt[(comp, oname, False)] >= 5, (comp, oname)


def test_list_size_set(events):
    cnt = collections.Counter()
    for c, recs in _of(events, "sizes"):
        n, lane = c["sub"]
        assert len(c["list"]) == n
        grow = c["w"] + 1e-3
        far, near, nonstrict, split, move = recs
        decider = c["list"][lane]
        (fx, fy, _), (nx, ny, _) = c["events"][0], c["events"][1]
        # far: outside every grown box (the early-out), the nearest endpoint is the decider's start
        assert not any(ci.in_grown_box(r, fx, fy, grow) for r in c["list"]) and far["what"] == ("none",)
        d_all = np.minimum(np.hypot(c["list"][:, 0] - fx, c["list"][:, 1] - fy), np.hypot(c["list"][:, 2] - fx, c["list"][:, 3] - fy))
        assert int(np.argmin(d_all)) == lane and abs(far["D"] - 500.0) < 1e-6
        # near: inside the decider's box, contained nowhere
        assert ci.in_grown_box(decider, nx, ny, grow) and 0.0 < near["D"] < 0.31 and near["what"] == ("none",)
        assert nonstrict["D"] == 0.0 and nonstrict["what"] == ("none",)
        assert split["what"] == ("split", lane) and len(split["after"]) == n + 1
        if lane + 1 < ci.WAVE:
            assert move["what"] == ("move", lane + 1, False)
        cnt[(n, lane)] += 1
        cnt["past 64"] += len(split["after"]) > ci.WAVE
        cnt["wave reduction decides in lane >= 8"] += n >= 9 and lane >= 8
    _show("list sizes (n, deciding lane)", cnt)
    for n in ci.LIST_SIZES:
        for lane in {0, 7, 8, n - 1}:
            if lane < n:
                assert cnt[(n, lane)] >= 3
    assert cnt["past 64"] >= 6 and cnt["wave reduction decides in lane >= 8"] >= 12


def test_box_boundary_set(events):
    cnt = collections.Counter()
    for c, recs in _of(events, "box"):
        x, y, _ = c["events"][0]
        inbox = ci.in_grown_box(c["box_rib"], x, y, c["grow"])
        cnt[(c["sub"], len(c["list"]), inbox)] += 1
        assert recs[0]["what"] == ("none",) and recs[0]["D"] > 0.0
    _show("grown-box faces ((orientation, face), n, inside)", cnt)
    for oname in ("axis", "oblique"):
        for face in range(4):
            for n in (1, 9):
                assert cnt[((oname, face), n, True)] >= 6 and cnt[((oname, face), n, False)] >= 6


def test_star_and_mixed_sets(events):
    cnt = collections.Counter()
    for c, recs in _of(events, "star"):
        k = c["sub"]
        assert len(recs[0]["after"]) == 2 * k, "every ribbon of the star splits in two"
        cnt[("star", k, len(recs[0]["after"]))] += 1
        assert len(recs[1]["before"]) == min(2 * k, ci.WAVE)
    assert cnt[("star", 33, 66)] >= 3 and cnt[("star", 32, 64)] >= 3
    in_place = {"BU", "CU", "UB", "BCU", "UCB", "BCUUUUUUU", "UUUUUUUUBC"}
    for c, recs in _of(events, "mixed"):
        route = ci.route_of(recs[0])
        cnt[("mixed", c["sub"], route, len(recs[0]["before"]), len(recs[0]["after"]))] += 1
        assert route == ("in-place" if c["sub"] in in_place else "compaction"), c["sub"]
    _show("several pieces at one event", cnt)
    # the in-place condition met, and missed by one piece: the same list with one piece more that splits in two / is erased
    for met, missed in (("BCU", "BCUA"), ("BCU", "ABCU"), ("BCUUUUUUU", "BCUUUUUUUA"), ("UCB", "TBC")):
        assert any(k[1] == met and k[2] == "in-place" for k in cnt) and any(k[1] == missed and k[2] == "compaction" for k in cnt)
    # one move alone (adv >= 0, either end), two moves at once (adv = -1), one split alone (adv <= -4)
    whats = collections.Counter((c["sub"], r[0]["what"][0]) for c, r in _of(events, "mixed"))
    assert whats[("BU", "move")] and whats[("CU", "move")] and whats[("BCU", "other")] and whats[("AU", "split")] and whats[("UA", "split")]


def test_tiny_and_degenerate_set(events):
    cnt = collections.Counter()
    for c, recs in _of(events, "tiny"):
        kind, arg = c["sub"]
        cnt[(kind, arg)] += 1
        if kind == "erase":
            assert len(recs[0]["after"]) == len(c["list"]) - 1 and recs[0]["D"] > 900.0
            assert np.array_equal(recs[0]["after"], np.delete(c["list"], arg, axis=0))
        elif kind == "keep":
            assert all(r["what"] == ("none",) for r in recs)
        elif kind == "zero":
            zero = [i for i, r in enumerate(c["list"]) if r[0] == r[2] and r[1] == r[3]]
            assert len(zero) == 1
            if arg:
                assert len(recs[0]["after"]) == len(c["list"]) - 1, "cover() erases the zero-length ribbon"
            else:
                assert all(r["what"] == ("none",) for r in recs)
        else:
            assert len(c["list"]) == 0 and all(len(r["after"]) == 0 and r["D"] == 0.0 for r in recs)
    _show("tiny and degenerate pieces", cnt)
    for lane in (0, 8):
        assert cnt[("erase", lane)] >= 6 and cnt[("keep", lane)] >= 6
    assert cnt[("erase", 19)] >= 6 and cnt[("zero", True)] >= 12 and cnt[("zero", False)] >= 6 and cnt[("empty", 0)] + cnt[("empty", 1)] >= 6


def test_sequence_set(events):
    cnt = collections.Counter()
    for c, recs in _of(events, "sequence"):
        kind, shape, step = c["sub"]
        assert len(recs) == ci.WAVE
        whats = [r["what"][0] for r in recs]
        for wh in set(whats):
            cnt[(kind, shape, step, wh)] += whats.count(wh)
        steps = np.hypot(*np.diff(c["events"][:, :2], axis=0).T)
        assert np.all(np.abs(steps - step) < 1e-3 * step)
        if kind == "down" and shape == "straight" and c["events"][:, 2].all():
            assert whats[0] == "split" and all(w == "move" for w in whats[1:]), "one split, then the start follows the vehicle"
        if kind == "collinear":
            touched = {r["what"][1] for r in recs if r["what"][0] in ("move", "split")}
            assert len(touched) >= 2, "both collinear pieces are covered in turn"
        if kind == "cross":
            assert max(len(r["after"]) for r in recs) >= 3, "the second ribbon is split too"
    _show("sequences (kind, shape, step, what cover() did)", cnt)
    for kind in ci.SEQ_KINDS:
        for shape in ("straight", "arc"):
            for step in (0.05, 0.01):
                assert sum(v for k, v in cnt.items() if k[:3] == (kind, shape, step) and k[3] != "none") >= 6


# ----------------------------------------------------------------------------- runs
def test_run_cases_are_deterministic(runs):
    again = ci.clean_run_cases()[:40] + ci.long_trap_cases()[:20]
    first = [r for r in runs if r["cls"] == "clean"][:40] + [r for r in runs if r["cls"] == "long-trap"][:20]
    for a, b in zip(again, first):
        assert a["list"].tobytes() == b["list"].tobytes() and a["poses"].tobytes() == b["poses"].tobytes() and a["ref_steps"] == b["ref_steps"]
    for r in runs:
        assert len(r["list"]) <= ci.WAVE and r["poses"].shape == (ci.WAVE, 2) and len(r["steps"]) == 63 * r["s"] + 1
        assert np.array_equal(r["poses"], r["steps"][::r["s"]]), "the samples are steps of the track handed over"
        assert 0 <= r["first"] < ci.WAVE and 0 <= r["adv"] < max(len(r["list"]), 1)
        if r["s"] > 1:
            assert r["ell"] < 0.5 * r["w"] and r["sin_dt"] < 0.5 and r["first"] == 0
    assert orc.O.ppo_get_ribbon_width() == ci.DEFAULT_WIDTH


def test_clean_tracks(runs):
    cnt = collections.Counter()
    for r in [r for r in runs if r["cls"] == "clean"]:
        oname, forward, first, sibling, off = r["sub"]
        assert r["clean"], "every decision of the replay clears its boundary by 1e-6"
        assert r["ref_steps"] == ci.WAVE - first, "the window cuts a clean track, nothing else does"
        assert r["move_end"] == (not forward) and len(r["list"]) == (2 if sibling else 1)
        cnt[(oname, "moveEnd" if r["move_end"] else "moveStart", first, "sibling" if sibling else "alone")] += 1
        cnt[("offset", off)] += 1
    for r in [r for r in runs if r["cls"] == "long-clean"]:
        assert r["clean"] and r["ref_steps"] == 63 * r["s"] + 1
        cnt[("long", r["sub"][0], r["s"])] += 1
    for r in [r for r in runs if r["cls"] == "quiet" and r["sub"][0] in ("between", "off")]:
        assert r["clean"] and r["ref_steps"] == ci.WAVE - r["first"]
        cnt[("quiet", r["sub"][0], r["first"])] += 1
    _show("clean tracks", cnt)
    for oname, _ in ci.RUN_ORIENTS:
        for end in ("moveEnd", "moveStart"):
            for first in ci.FIRSTS:
                for sib in ("sibling", "alone"):
                    assert cnt[(oname, end, first, sib)] >= 5
    assert all(cnt[("offset", off)] >= 48 for off in ci.OFFSETS)
    assert all(cnt[("long", k, s)] >= 6 for k in ("corridor", "quiet") for s in ci.LONG_S)
    assert all(cnt[("quiet", k, f)] >= 6 for k in ("between", "off") for f in ci.FIRSTS)


def test_tracks_that_end_inside_the_window(runs):
    cnt = collections.Counter()
    for r in [r for r in runs if r["cls"] == "ending"]:
        what = r["sub"][0]
        left = ci.WAVE - r["first"]
        if what == "erasable":
            assert r["ref_steps"] == 0
        else:
            assert 10 <= r["ref_steps"] < left - 10, (r["sub"], r["ref_steps"])
        if what == "stepOk":
            assert r["ref_steps"] == 37 - r["first"]
        if what == "coverMask":
            assert r["ref_steps"] == 29 - r["first"]
        cnt[(what, r["ref_steps"])] += 1
    for r in [r for r in runs if r["cls"] == "quiet" and r["sub"][0] not in ("between", "off")]:
        what = r["sub"][0]
        left = ci.WAVE - r["first"]
        if what == "erasable-on":
            assert r["ref_steps"] == 0
        elif what in ("erasable-off", "into-off"):
            assert r["ref_steps"] == left
        else:
            assert 3 <= r["ref_steps"] < left - 10
        cnt[("quiet " + what, r["ref_steps"])] += 1
    _show("tracks that end inside the window (why, reference run length)", cnt)
    for what in ("shallow", "rest", "front", "crossing", "stepOk", "coverMask", "erasable"):
        assert sum(v for k, v in cnt.items() if k[0] == what) >= 36
    for what in ("into", "into-off", "out", "erasable-on", "erasable-off"):
        assert sum(v for k, v in cnt.items() if k[0] == "quiet " + what) >= 36


def test_knife_edge_runs(runs):
    cnt = collections.Counter()
    for r in [r for r in runs if r["cls"] == "knife-run"]:
        what, oname, offset = r["sub"]
        assert r["first"] == 0 and r["ref_steps"] >= ci.KNIFE_STEP
        went_on = r["ref_steps"] > ci.KNIFE_STEP
        assert went_on == (offset <= 0.0), "the bisection put offset 0 on the last step the replay still takes"
        scale = "ulps" if abs(offset) < 5e-12 * max(1.0, abs(r["list"][0, 0]) / 100.0) else "metres"
        cnt[(what, oname, scale, "taken" if went_on else "refused")] += 1
    _show("knife-edge runs (edge, orientation, step size, what the replay does at step 30)", cnt)
    for what in ("strict", "rest"):
        for oname, _ in ci.RUN_ORIENTS:
            for scale in ("ulps", "metres"):
                assert cnt[(what, oname, scale, "taken")] >= 5 and cnt[(what, oname, scale, "refused")] >= 5


def test_long_run_traps(runs):
    """A trap is real when the reference's replay first differs at a step strictly between samples 20 and 21, which a run that looked at
    the samples alone would vouch for."""
    cnt = collections.Counter()
    for r in [r for r in runs if r["cls"] == "long-trap"]:
        what, delta = r["sub"]
        s = r["s"]
        assert r["ref_steps"] < 63 * s + 1 or (s == 5 and delta == 1e-6), "the replay differs somewhere (s = 5 steps over the smallest bulge)"
        real = 20 * s < r["ref_steps"] < 21 * s
        cnt[(what, "between samples" if real else "at a sample or before")] += 1
        cnt[("delta", delta, real)] += 1
    _show("long-run traps", cnt)
    for what in ("strict", "end", "sibling", "quiet-out", "quiet-in"):
        assert cnt[(what, "between samples")] >= 12, what
    for delta in (1e-6, 1e-5, 3e-5):
        assert cnt[("delta", delta, True)] >= 20


def test_event_stride_set():
    D, inc, ng = ci.event_stride_set()
    ref = ci.event_stride_reference(D, inc, ng)
    idx = np.random.RandomState(3).choice(len(D), 400, replace=False)
    assert all(ref[i] == ci.event_stride_reference_scalar(D[i], inc[i], ng[i]) for i in idx)
    cnt = collections.Counter()
    for c in (0.05, 0.1, 0.25, 1.0 / 3.0, 0.0125):
        for g in (8, 1508):
            sel = (inc == c) & (ng == g)
            m = ref[sel]
            assert set(range(0, g + 2)) <= set(m.tolist()), "every stride up to 'never again' occurs"
            assert (D[sel] == 0.0).any() and (D[sel] == c).any() and (D[sel] == np.finfo(np.float64).max).any()
            # around k inc the literal loop gives k - 1 on one side and k on the other: both occur for most k
            k = np.arange(1, g + 4)
            base = k * c
            both = sum(len(set(ref[sel][np.abs(D[sel] - b) <= 8 * np.spacing(b)].tolist())) >= 2 for b in base[:: max(1, g // 50)])
            cnt[(round(c, 4), g, "k with both strides nearby")] = both
            assert both >= 4
    _show("pp_event_stride set", cnt)
    print(f"  elements {len(D)}")
