"""-m gpu: the pieces of the coverage state machine, each alone (tests/probe/pp_cover_probe.hip), against the reference's RibbonManager
as the oracle replays it (tests/cover_probe_inputs.py, held to its classes by tests/test_cover_probe_inputs.py):

  * pp_ribbons_event, byte for byte: count, D, every lane's ribbon and the adv hand-over code, for every event of every case;
  * the lane forms pp_lane_cover_strict, pp_lane_ribbon_contains, pp_box_scan / pp_any_tiny_ribbon, and pp_event_stride against the
    literal subtraction loop;
  * pp_corridor_run and pp_quiet_run: every step a run claims is a step the reference's replay treats that way (no tolerance), the
    moved endpoint is the replay's within the rounding the code documents, and on clean tracks the run is as long as the replay's.

Worst corridor endpoint deviation measured on MI355X: see DESIGN.md, Appendix C."""
import numpy as np
import pytest

import cover_probe as cp
import cover_probe_inputs as ci
import oracle as orc

pytestmark = pytest.mark.gpu

LIST_TOL = 1e-9      # m: the guard tests/test_gpu_cover_trace.py already holds a moved endpoint to


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _describe(case, i, rec):
    return (f"{case['cls']} {case['sub']} w {case['w']} event {i} at ({case['events'][i, 0]!r}, {case['events'][i, 1]!r}) cover {rec['cover']}, "
            f"list of {len(rec['before'])}, the reference: {rec['what']} -> {len(rec['after'])}")


# ----------------------------------------------------------------------------- events
@pytest.fixture(scope="module")
def ev():
    """every event of every case, once on the device, and the reference's records flattened the same way"""
    cases, refs = ci.event_cases(), ci.event_reference()
    off, cnt, D, adv, ribs = cp.cover_events([c["list"] for c in cases], [c["w"] for c in cases], [c["events"] for c in cases])
    recs, owner = [], []
    for ic, rs in enumerate(refs):
        for i, r in enumerate(rs):
            recs.append(r)
            owner.append((ic, i))
    assert len(recs) == int(off[-1]) == len(cnt)
    return {"cases": cases, "cnt": cnt, "D": D, "adv": adv, "ribs": ribs, "recs": recs, "owner": owner}


def _fail_list(ev, bad, what):
    lines = [_describe(ev["cases"][ev["owner"][g][0]], ev["owner"][g][1], ev["recs"][g]) + f"; device: count {ev['cnt'][g]} D {ev['D'][g]!r} adv {ev['adv'][g]}"
             for g in bad[:5]]
    return f"{what} at {len(bad)} of {len(ev['recs'])} events:\n  " + "\n  ".join(lines)


def test_event_count_and_distance_are_the_references(ev):
    want_cnt = np.array([len(r["after"]) for r in ev["recs"]], dtype=np.int32)
    bad = np.nonzero(ev["cnt"] != want_cnt)[0]
    assert bad.size == 0, _fail_list(ev, bad, "returned count differs")
    want_D = np.array([r["D"] for r in ev["recs"]], dtype=np.float64)
    bad = np.nonzero(_u64(ev["D"]) != _u64(want_D))[0]
    assert bad.size == 0, _fail_list(ev, bad, "D differs in its bytes")
    print(f"\n{len(want_cnt)} events; counts up to {want_cnt.max()}, {int((want_cnt > 64).sum())} above 64")


def test_event_lists_are_the_references_bytes(ev):
    want = np.zeros_like(ev["ribs"])
    for g, r in enumerate(ev["recs"]):
        k = min(len(r["after"]), cp.WAVE)
        want[g, :k] = r["after"][:k]
    bad = np.nonzero((_u64(ev["ribs"]) != _u64(want)).any(axis=(1, 2)))[0]
    assert bad.size == 0, _fail_list(ev, bad, "lanes differ from the reference's pieces (or hold something beyond the count)")
    # without cover() the list is the one handed in
    for g, r in enumerate(ev["recs"]):
        if not r["cover"]:
            k = len(r["before"])
            assert ev["ribs"][g, :k].tobytes() == r["before"].tobytes() and not ev["ribs"][g, k:].any()


def test_event_adv_codes_say_what_the_reference_did(ev):
    seen = {"-3": 0, "-2": 0, "move start": 0, "move end": 0, "split": 0, "-1": 0}
    for g, r in enumerate(ev["recs"]):
        a, what, nb = int(ev["adv"][g]), r["what"], len(r["before"])
        case, i = ev["cases"][ev["owner"][g][0]], ev["owner"][g][1]
        msg = _describe(case, i, r) + f"; adv {a}"
        if nb == 0:
            assert a == -1, msg
            continue
        x, y, _ = case["events"][i]
        grow, w = case["w"] + 1e-3, case["w"]
        b = r["before"]
        early = not any(ci.in_grown_box(q, x, y, grow) or ((q[2] - q[0]) * (q[2] - q[0]) + (q[3] - q[1]) * (q[3] - q[1])) < (2 * w) * (2 * w) / 4.0 for q in b)
        assert (a == -3) == early, msg + " (the early-out is taken exactly outside every grown box with no erasable piece)"
        if a in (-3, -2):
            assert what == ("none",), msg
            seen[str(a)] += 1
        elif a >= 0:
            assert what == ("move", a & 0xff, (a & 0x100) != 0), msg
            seen["move end" if a & 0x100 else "move start"] += 1
        elif a <= -4:
            assert what == ("split", -4 - a), msg
            seen["split"] += 1
        else:
            assert a == -1, msg
            seen["-1"] += 1
        # and the other way round: the runs are only ever started by these codes
        if what == ("none",):
            assert a in (-3, -2), msg
        elif what[0] == "move":
            assert a >= 0, msg
        elif what[0] == "split" and nb < cp.WAVE:
            assert a <= -4, msg
    print(f"\nadv codes: {seen}")
    assert all(v > 0 for v in seen.values())


# ----------------------------------------------------------------------------- lane forms
def test_lane_cover_strict_matches_the_wave_form_and_the_reference(ev):
    """every cover() on a list of at most 8 ribbons, with a child slot wide enough and with one narrower than the resulting count"""
    gs = [g for g, r in enumerate(ev["recs"]) if r["cover"] and len(r["before"]) <= cp.FINISH_MAX]
    lists, strides, xs, ys, ws, which = [], [], [], [], [], []
    for g in gs:
        r = ev["recs"][g]
        case, i = ev["cases"][ev["owner"][g][0]], ev["owner"][g][1]
        nb, na = len(r["before"]), len(r["after"])
        for stride in {cp.FINISH_MAX, max(nb, min(na - 1, cp.FINISH_MAX)) if na > nb else cp.FINISH_MAX}:
            lists.append(r["before"]); strides.append(stride); xs.append(case["events"][i, 0]); ys.append(case["events"][i, 1]); ws.append(case["w"])
            which.append(g)
    out, slots = cp.lane_cover_strict(lists, strides, xs, ys, ws)
    narrow = 0
    for j, g in enumerate(which):
        r = ev["recs"][g]
        na, stride = len(r["after"]), strides[j]
        msg = _describe(ev["cases"][ev["owner"][g][0]], ev["owner"][g][1], r) + f"; stride {stride}: returned {out[j]}"
        assert out[j] == na == ev["cnt"][g], msg
        k = min(na, stride)
        assert slots[j, :k].tobytes() == r["after"][:k].tobytes(), msg
        assert not slots[j, k:].any(), msg + " (slots beyond stay zero)"
        kk = min(k, cp.WAVE)
        assert slots[j, :kk].tobytes() == ev["ribs"][g, :kk].tobytes(), msg
        narrow += stride < na
    print(f"\n{len(which)} lane covers, {narrow} with a slot narrower than the count")
    assert len(which) > 5000 and narrow > 50


def test_lane_ribbon_contains_on_the_knife_edges(ev):
    cases = [c for c in ev["cases"] if c["cls"] == "knife"]
    rib = np.array([c["list"][0] for c in cases])
    x, y, w = np.array([c["events"][0, 0] for c in cases]), np.array([c["events"][0, 1] for c in cases]), np.array([c["w"] for c in cases])
    inside, strict, pxy = cp.lane_contains(rib, x, y, w)
    want_in, want_st, want_p = np.zeros(len(cases), dtype=np.uint8), np.zeros(len(cases), dtype=np.uint8), np.zeros((len(cases), 2))
    for i, c in enumerate(cases):
        with ci.ribbon_width(c["w"]):
            r = np.ascontiguousarray(rib[i])
            want_in[i] = orc.O.ppo_ribbon_contains(r.ctypes.data, x[i], y[i], 0)
            want_st[i] = orc.O.ppo_ribbon_contains(r.ctypes.data, x[i], y[i], 1)
            orc.O.ppo_ribbon_projection(r.ctypes.data, x[i], y[i], want_p[i].ctypes.data)
    assert np.array_equal(_u64(pxy), _u64(want_p)), f"projection differs at {np.nonzero((_u64(pxy) != _u64(want_p)).any(axis=1))[0][:5]}"
    bad = np.nonzero((inside != want_in) | (strict != want_st))[0]
    assert bad.size == 0, f"{bad.size} of {len(cases)} knife-edge points: first {cases[bad[0]]['sub']} w {w[bad[0]]} at ({x[bad[0]]!r}, {y[bad[0]]!r})"
    print(f"\n{len(cases)} points: inside {int(want_in.sum())}, strictly {int(want_st.sum())}")
    assert 0 < want_st.sum() < want_in.sum() < len(cases)


def test_box_scan_and_tiny_equal_numpy(ev):
    sel = [c for c in ev["cases"] if c["cls"] in ("box", "tiny", "sizes")]
    lists, xs, ys, grows, thrs = [], [], [], [], []
    for c in sel:
        for x, y, _ in c["events"][:2]:
            lists.append(c["list"]); xs.append(x); ys.append(y); grows.append(c["w"] + 1e-3); thrs.append((2 * c["w"]) * (2 * c["w"]) / (2.0 * 2.0))
    in_box, box_count, box_idx, tiny, q = cp.box_scan(lists, xs, ys, grows, thrs)
    n_in = n_tiny = 0
    for j, (r, x, y, g, t) in enumerate(zip(lists, xs, ys, grows, thrs)):
        inb = np.array([ci.in_grown_box(s, x, y, g) for s in r], dtype=bool)
        assert in_box[j] == inb.any() and box_count[j] == inb.sum(), (j, x, y)
        if inb.any():
            assert box_idx[j] == np.nonzero(inb)[0][-1]
        sq = (r[:, 2] - r[:, 0]) * (r[:, 2] - r[:, 0]) + (r[:, 3] - r[:, 1]) * (r[:, 3] - r[:, 1])
        assert tiny[j] == (sq < t).any()
        if len(r):
            qs = (r[:, 0] - x) * (r[:, 0] - x) + (r[:, 1] - y) * (r[:, 1] - y)
            qe = (r[:, 2] - x) * (r[:, 2] - x) + (r[:, 3] - y) * (r[:, 3] - y)
            assert _u64(q[j:j + 1])[0] == _u64(np.array([np.minimum(qs, qe).min()]))[0]
        n_in += inb.any()
        n_tiny += tiny[j]
    print(f"\n{len(lists)} scans: {n_in} inside a grown box, {n_tiny} with an erasable piece")
    assert 300 < n_in < len(lists) - 300 and n_tiny > 50


def test_event_stride_is_the_literal_loop():
    D, inc, ng = ci.event_stride_set()
    got = cp.event_stride(D, inc, ng)
    want = ci.event_stride_reference(D, inc, ng)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} of {len(D)}: first D {D[bad[0]]!r} inc {inc[bad[0]]!r} ng {ng[bad[0]]}: {got[bad[0]]}, the loop gives {want[bad[0]]}"


# ----------------------------------------------------------------------------- runs
@pytest.fixture(scope="module")
def runs():
    cases = ci.run_cases()
    L, xy = cp.cover_runs([c["list"] for c in cases], [c["poses"] for c in cases], [c["kind"] for c in cases], [c["adv"] for c in cases],
                          [c["move_end"] for c in cases], [c["first"] for c in cases], [c["step_ok"] for c in cases],
                          [c["cover_mask"] for c in cases], [c["w"] for c in cases], [c["span"] for c in cases], [c["ell"] for c in cases],
                          [c["sin_dt"] for c in cases])
    return cases, L, xy


def _run_name(c, L):
    return (f"{c['cls']} {c['sub']} kind {c['kind']} w {c['w']} s {c['s']} first {c['first']} adv {c['adv']} moveEnd {c['move_end']}: L {L} "
            f"claims {ci.claimed_steps(c, L)} steps, the reference's replay goes {c['ref_steps']}")


def test_runs_claim_only_what_the_replay_does(runs):
    """corridor run: every claimed step moves exactly the named endpoint of the named piece in the replay and nothing else; quiet run:
    every claimed step has minDistanceFrom == 0 and leaves the list alone (cover_probe_inputs.make_run counts exactly those steps).

    Before pp_corridor_run added pp_line_num_slack to its strict test, 74 of the 1 440 knife-edge runs — all on the strict edge around
    (1e5, -3e4), step 30 up to 3.0e-9 m outside the reference's own edge — claimed all 64 steps where the replay refuses step 30: the
    run measures the line distance on the piece as it found it, the replay on the piece with the moved start, and ex * sy - ey * sx
    (3e9 there) rounds to about 1e-6, more than a 1e-9 relative guard on w / 2 covers."""
    cases, L, _ = runs
    bad = []
    for c, l in zip(cases, L):
        assert 0 <= l <= cp.WAVE - c["first"], _run_name(c, l)
        if ci.claimed_steps(c, l) > c["ref_steps"]:
            bad.append(_run_name(c, l))
        if c["cls"] == "ending" and c["sub"][0] == "erasable":
            assert l == 0, _run_name(c, l)
    assert not bad, f"{len(bad)} of {len(cases)} runs claim a step the replay treats differently:\n  " + "\n  ".join(bad[:12])


def test_corridor_endpoint_is_the_replays_within_rounding(runs):
    cases, L, xy = runs
    worst, worst_at, n = 0.0, None, 0
    per_centre = {}
    for c, l, p in zip(cases, L, xy):
        k = ci.claimed_steps(c, l)
        if c["kind"] != 1 or k == 0 or k > c["ref_steps"]:
            continue
        dev = float(np.hypot(*(p - c["ref_ends"][k - 1])))
        n += 1
        big = abs(c["list"][0, 0]) > 1e4
        per_centre[big] = max(per_centre.get(big, 0.0), dev)
        if dev > worst:
            worst, worst_at = dev, _run_name(c, l)
    print(f"\nworst corridor endpoint deviation over {n} runs: {worst:.3e} m ({worst_at}); around (100, 100): {per_centre.get(False, 0.0):.3e} m, "
          f"around (1e5, -3e4): {per_centre.get(True, 0.0):.3e} m")
    assert n > 800
    assert worst <= LIST_TOL, worst_at


def test_runs_are_not_vacuous(runs):
    cases, L, _ = runs
    short = {}
    for c, l in zip(cases, L):
        if c["clean"] and c["s"] == 1:
            assert l == c["ref_steps"], _run_name(c, l)
        if c["cls"] == "long-clean":
            assert l == cp.WAVE, _run_name(c, l)
        if c["cls"] == "knife-run" and c["sub"][2] <= -1e-6:
            # 1e-6 m inside the edge is at least 6e-7 of w / 2 or w: hundreds of times the run's 1e-9 guard
            assert l == c["ref_steps"], _run_name(c, l)
        if c["cls"] in ("ending", "quiet", "long-trap", "knife-run"):
            key = (c["cls"], c["sub"][0])
            short.setdefault(key, []).append(c["ref_steps"] - ci.claimed_steps(c, l))
    print("\nsteps the reference's replay goes beyond what the run claimed (min .. max):")
    for key in sorted(short):
        print(f"  {key}: {min(short[key])} .. {max(short[key])}")
