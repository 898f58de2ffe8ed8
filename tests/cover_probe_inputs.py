"""Inputs and references of the cover-piece tests (tests/test_gpu_cover_pieces.py runs them on the device, tests/test_cover_probe_inputs.py
holds the sets themselves to their classes on the CPU).

Every set is deterministic (fixed seeds) and needs only the CPU.  The reference is the oracle's RibbonManager (oracle.ribbons_cover,
oracle.ribbons_min_distance and the single-ribbon calls), pinned to the reference's own objects by tests/test_golden.py; it is replayed
once per process and shared by every test.

Two kinds of cases:
  * EVENT cases: a list of at most 64 ribbons, a width, and up to 64 events (x, y, doCover) applied one after the other, as
    pp_cover_sweep_edge applies pp_ribbons_event (a count above 64 is reported and the list cut to 64 before the next event);
  * RUN cases: a list, 64 poses (one per lane), and the arguments of pp_corridor_run / pp_quiet_run, with ALL the steps of the track
    (for a long run the steps between the samples too) and the reference's replay of them."""
import contextlib
import functools
import math

import numpy as np

import oracle as orc

WAVE = 64
CAP = 128                      # the reference's list may grow past 64: the overflow is a count, never an access
WIDTHS = (0.4, 1.5, 3.0)
CENTRES = ((100.0, 100.0), (1e5, -3e4))
TOL = 1e-5                     # Ribbon::c_Tolerance
DEFAULT_WIDTH = 1.5
CLEAR = 1e-6                   # what a clean track's decisions clear their boundaries by (relative; 1e-6 m for the projection tolerance)


@contextlib.contextmanager
def ribbon_width(w):
    orc.O.ppo_set_ribbon_width(float(w))
    try:
        yield
    finally:
        orc.O.ppo_set_ribbon_width(DEFAULT_WIDTH)


# ----------------------------------------------------------------------------- geometry
def unit(deg):
    return (math.cos(math.radians(deg)), math.sin(math.radians(deg)))


def _seeded_dirs(n, seed):
    rng = np.random.RandomState(seed)
    return [unit(a) for a in rng.uniform(3.0, 357.0, n)]


# name, class, direction.  3-4-5 has exactly representable endpoints for lengths that are multiples of 5.
ORIENTS = ([("0", "axis", (1.0, 0.0)), ("90", "axis", (0.0, 1.0)), ("345", "345", (0.8, 0.6)), ("1", "oblique", unit(1.0)),
            ("89", "oblique", unit(89.0)), ("179", "oblique", unit(179.0))] +
           [("s%d" % i, "oblique", d) for i, d in enumerate(_seeded_dirs(16, 20240))])
KNIFE_ORIENTS = [("axis", (1.0, 0.0)), ("345", (0.8, 0.6)), ("oblique", _seeded_dirs(1, 77)[0])]


def nrm(d):
    return (-d[1], d[0])


def rot(d, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return (c * d[0] - s * d[1], s * d[0] + c * d[1])


def mk(S, d, L):
    return np.array([S[0], S[1], S[0] + L * d[0], S[1] + L * d[1]])


def at(S, d, t, off=0.0):
    n = nrm(d)
    return (S[0] + t * d[0] + off * n[0], S[1] + t * d[1] + off * n[1])


def ulp_vec(p, u):
    """a step of about one ulp of each coordinate of p along u"""
    return (float(np.spacing(abs(p[0]))) * u[0], float(np.spacing(abs(p[1]))) * u[1])


def stepped(p, sv, k):
    return (p[0] + k * sv[0], p[1] + k * sv[1])


def find_flip(f, p, sv, K):
    """k in [-K, K) with f(p + k sv) != f(p + (k + 1) sv): the reference's own knife edge, found by bisection on the reference."""
    lo, hi = -K, K
    flo, fhi = f(stepped(p, sv, lo)), f(stepped(p, sv, hi))
    assert flo != fhi, "the reference takes one decision over the whole range"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(stepped(p, sv, mid)) == flo:
            lo = mid
        else:
            hi = mid
    return lo


# ----------------------------------------------------------------------------- the reference, one event
def classify(before, after):
    """What cover() did: ('none',), ('move', piece, end_moved), ('split', piece) with both halves kept, or ('other',)."""
    nb, na = len(before), len(after)
    if nb == na:
        if before.tobytes() == after.tobytes():
            return ("none",)
        rows = np.nonzero((before.view(np.uint64) != after.view(np.uint64)).any(axis=1))[0]
        if len(rows) == 1:
            i = int(rows[0])
            s = before[i, :2].tobytes() != after[i, :2].tobytes()
            e = before[i, 2:].tobytes() != after[i, 2:].tobytes()
            if s != e:
                return ("move", i, e)
        return ("other",)
    if na == nb + 1:
        for i in range(nb):
            if before[i].tobytes() != after[i].tobytes():
                break
        ok = (before[:i].tobytes() == after[:i].tobytes() and before[i + 1:].tobytes() == after[i + 2:].tobytes() and
              before[i, :2].tobytes() == after[i, :2].tobytes() and before[i, 2:].tobytes() == after[i + 1, 2:].tobytes() and
              after[i, 2:].tobytes() == after[i + 1, :2].tobytes())
        return ("split", i) if ok else ("other",)
    return ("other",)


def ref_event(cur, x, y, do_cover):
    """(D on the list before the cover, the list after it: uncut, up to CAP pieces)"""
    D = orc.ribbons_min_distance(cur, x, y)
    after = orc.ribbons_cover(cur, x, y, True, cap=CAP) if do_cover else cur.copy()
    return D, after


def replay_events(lst, w, events):
    out = []
    cur = np.ascontiguousarray(lst, dtype=np.float64).reshape(-1, 4)
    with ribbon_width(w):
        for x, y, c in np.asarray(events, dtype=np.float64).reshape(-1, 3):
            D, after = ref_event(cur, x, y, c != 0.0)
            out.append({"D": D, "before": cur, "after": after, "what": classify(cur, after), "cover": c != 0.0})
            cur = after[:WAVE]
    return out


# ----------------------------------------------------------------------------- event cases
def _case(cls, sub, lst, w, events, **kw):
    d = {"cls": cls, "sub": sub, "list": np.ascontiguousarray(lst, dtype=np.float64).reshape(-1, 4), "w": float(w),
         "events": np.ascontiguousarray(events, dtype=np.float64).reshape(-1, 3)}
    d.update(kw)
    return d


def _ev(points, cover):
    cover = [cover] * len(points) if np.isscalar(cover) else cover
    return [(p[0], p[1], 1.0 if c else 0.0) for p, c in zip(points, cover)]


def orientation_cases():
    out = []
    for io, (name, ocls, d) in enumerate(ORIENTS):
        for il in range(4):
            for ic, C in enumerate(CENTRES):
                w = WIDTHS[(io + il + ic) % 3]
                L = (2 * w + 1e-3, 5.0, 55.0, 400.0)[il]
                r = mk(C, d, L)
                pts = [at(C, d, -1000.0, 300.0), at(C, d, 0.5 * L, 1.5 * w), at(C, d, -3.0, 0.1 * w), at(C, d, L + 3.0, -0.1 * w),
                       at(C, d, 0.5 * L, 0.7 * w), at(C, d, 0.5 * L, -0.7 * w), at(C, d, 0.5 * L, 0.2 * w)]
                kinds = ["far", "outside", "before", "beyond", "nonstrict", "nonstrict", "inside"]
                out.append(_case("orientation", ocls, [r], w, _ev(pts, False), kinds=kinds, name=name))
                out.append(_case("orientation", ocls, [r], w, _ev(pts, True), kinds=kinds, name=name))
    return out


KNIFE_HALF = {"perp_w": 40, "perp_w2": 40, "proj_start": 8, "proj_end": 8, "keepF": 8, "keepR": 8}


def knife_cases():
    """Single events stepping across each comparison of the reference in ulp-sized steps, centred on the reference's own flip."""
    out = []
    L = 40.0
    for oname, d in KNIFE_ORIENTS:
        for w in WIDTHS:
            for C in CENTRES:
                r = mk(C, d, L)
                lst = r.reshape(1, 4)
                rp = r.ctypes.data
                with ribbon_width(w):
                    def contains(p, strict):
                        return orc.O.ppo_ribbon_contains(rp, p[0], p[1], strict)

                    def count(p):
                        return len(orc.ribbons_cover(lst, p[0], p[1], True, cap=CAP))
                    plans = [
                        ("perp_w", at(C, d, 0.4 * L, w), nrm(d), lambda p: contains(p, 0), 1e-6),
                        ("perp_w2", at(C, d, 0.4 * L, 0.5 * w), nrm(d), lambda p: contains(p, 1), 1e-6),
                        ("proj_start", at(C, d, 0.0, 0.1 * w), d, lambda p: contains(p, 0), 1e-3),
                        ("proj_end", at(C, d, L, 0.1 * w), d, lambda p: contains(p, 0), 1e-3),
                        ("keepF", at(C, d, w, 0.1 * w), d, count, 1e-6),
                        ("keepR", at(C, d, L - w, 0.1 * w), d, count, 1e-6),
                    ]
                    for comp, p0, u, f, rng in plans:
                        sv = ulp_vec(p0, u)
                        K = int(rng / max(abs(sv[0]), abs(sv[1]))) + 64
                        k0 = find_flip(f, p0, sv, K)
                        h = KNIFE_HALF[comp]
                        for k in range(k0 - h + 1, k0 + h + 2):      # the flip lies between k0 and k0 + 1: h + ... on either side
                            p = stepped(p0, sv, k)
                            out.append(_case("knife", (comp, oname), lst, w, _ev([p], True)))
    return out


def knife_outcome(case, rec):
    comp = case["sub"][0]
    if comp in ("perp_w", "proj_start", "proj_end"):
        return rec["D"] == 0.0
    if comp == "perp_w2":
        return rec["what"] != ("none",)
    return len(rec["after"]) == 2


LIST_SIZES = (1, 2, 8, 9, 32, 63, 64)


def _parallel_list(C, d, n, lane, L=30.0, gap=25.0):
    """n parallel ribbons `gap` apart; the one through C sits in `lane`, the others fill the remaining lanes in order of distance"""
    out = np.zeros((n, 4))
    j = 0
    for i in range(n):
        if i == lane:
            out[i] = mk(C, d, L)
        else:
            j += 1
            out[i] = mk(at(C, d, 0.0, gap * j), d, L)
    return out


def list_size_cases():
    out = []
    dirs = _seeded_dirs(4, 31)
    for n in LIST_SIZES:
        for il, lane in enumerate(sorted({0, 7, 8, n - 1})):
            if lane >= n:
                continue
            for iw, w in enumerate(WIDTHS):
                C = CENTRES[(il + iw) % 2]
                d = dirs[(il + iw) % 4]
                d = (abs(d[0]), abs(d[1]))        # first quadrant: the far point below lies outside every grown box
                lst = _parallel_list(C, d, n, lane)
                pts = [at(C, d, -500.0), at(C, d, -0.3), at(C, d, 10.0, 0.7 * w), at(C, d, 10.0, 0.1 * w), at(C, d, 10.05, 0.1 * w)]
                out.append(_case("sizes", (n, lane), lst, w, _ev(pts, True), kinds=["far", "near", "nonstrict", "split", "move"]))
    return out


def grown_box(r, grow):
    """the box of pp_in_grown_box, in its own expressions"""
    return (min(r[0], r[2]) - grow, max(r[0], r[2]) + grow, min(r[1], r[3]) - grow, max(r[1], r[3]) + grow)


def in_grown_box(r, x, y, grow):
    b = grown_box(r, grow)
    return (x >= b[0]) and (x <= b[1]) and (y >= b[2]) and (y <= b[3])


def box_cases():
    out = []
    for oname, d in KNIFE_ORIENTS[::2]:
        for w in WIDTHS:
            for C in CENTRES:
                r = mk(C, d, 30.0)
                grow = w + 1e-3
                b = grown_box(r, grow)
                mx, my = 0.5 * (b[0] + b[1]), 0.5 * (b[2] + b[3])
                for n in (1, 9):
                    lst = r.reshape(1, 4) if n == 1 else _parallel_list(C, d, 9, 8, gap=200.0)
                    for face in range(4):
                        v = b[face]
                        for k in range(-3, 4):
                            vk = v
                            for _ in range(abs(k)):
                                vk = float(np.nextafter(vk, math.inf if k > 0 else -math.inf))
                            p = (vk, my) if face < 2 else (mx, vk)
                            out.append(_case("box", (oname, face), lst, w, _ev([p], True), grow=grow, box_rib=r))
    return out


def star(C, k, L=40.0):
    return np.array([mk(at(C, unit(5.7 + 180.0 * i / k), -0.5 * L), unit(5.7 + 180.0 * i / k), L) for i in range(k)])


STAR_K = (2, 3, 8, 31, 32, 33)


def star_cases():
    out = []
    for k in STAR_K:
        for iw, w in enumerate(WIDTHS):
            for C in CENTRES:
                pts = [C, (C[0] + 0.3 * w, C[1] + 0.2 * w)]
                out.append(_case("star", k, star(C, k), w, _ev(pts, True)))
    return out


def mixed_cases():
    """One event at P at which pieces split keeping both halves (A), keep only the rest (B) or only the front (C), vanish after the
    split (V), are erased from afar (T) or stay untouched (U).  `sub` names the pieces present, in list order."""
    out = []
    combos = ["BU", "CU", "UB", "BCU", "UCB", "BCUA", "ABCU", "BCT", "TBC", "AU", "UA", "BV", "VU", "ABCVTU", "UTVCBA", "BCUUUUUUU", "UUUUUUUUBC",
              "BCUUUUUUUA"]
    for w in WIDTHS:
        for C in CENTRES:
            pieces = {
                "A": mk(at(C, unit(10.0), -15.0), unit(10.0), 30.0),
                "B": mk(at(C, unit(50.0), -0.5 * w), unit(50.0), 30.0),
                "C": mk(at(C, unit(100.0), -30.0 + 0.5 * w), unit(100.0), 30.0),
                "V": mk(at(C, unit(140.0), -0.75 * w), unit(140.0), 1.5 * w),
                "T": mk(at(C, unit(0.0), 300.0, 40.0), unit(33.0), 0.5 * w),
            }
            for combo in combos:
                lst, nu = [], 0
                for ch in combo:
                    if ch == "U":
                        nu += 1
                        lst.append(mk(at(C, unit(20.0), 200.0, 30.0 * nu), unit(70.0), 25.0))
                    else:
                        lst.append(pieces[ch])
                out.append(_case("mixed", combo, lst, w, _ev([C], True)))
    return out


def route_of(rec):
    """in-place: every changed piece changed one endpoint and none vanished; compaction: the count changed"""
    b, a = rec["before"], rec["after"]
    if len(a) != len(b):
        return "compaction"
    if rec["what"] == ("none",):
        return "none"
    for i in range(len(b)):
        s = b[i, :2].tobytes() != a[i, :2].tobytes()
        e = b[i, 2:].tobytes() != a[i, 2:].tobytes()
        if s and e:
            return "other"
    return "in-place"


def tiny_cases():
    out = []
    for w in WIDTHS:
        for ic, C in enumerate(CENTRES):
            far = at(C, (1.0, 0.0), -1000.0, -700.0)
            for n in (3, 9, 20):
                for lane in sorted({0, 8, n - 1}):
                    if lane >= n:
                        continue
                    lst = _parallel_list(C, unit(25.0), n, lane)
                    lst[lane] = mk(C, unit(25.0), 0.5 * w)
                    out.append(_case("tiny", ("erase", lane), lst, w, _ev([far], True)))
                    out.append(_case("tiny", ("keep", lane), lst, w, _ev([far, far], [False, False])))
            # a zero-length ribbon: the reference's projection on it is NaN (0 / 0), every comparison with it is false, so the ribbon
            # "contains" every projection and its line distance (x / 0) decides: never inside.  cover() erases it as covered.
            for lane in (0, 2):
                lst = _parallel_list(C, unit(25.0), 3, 1)
                lst[lane] = (C[0] + 7.0, C[1] - 3.0, C[0] + 7.0, C[1] - 3.0)
                near = (C[0] + 7.0, C[1] - 3.0)
                out.append(_case("tiny", ("zero", True), lst, w, _ev([far, near], True)))
                out.append(_case("tiny", ("zero", True), lst, w, _ev([near], True)))
                out.append(_case("tiny", ("zero", False), lst, w, _ev([far, near, at(C, unit(25.0), 10.0, 0.1 * w)], False)))
            out.append(_case("tiny", ("empty", ic), np.zeros((0, 4)), w, _ev([C, far], [True, False])))
    return out


def straight_track(P0, u, step, j0, j1):
    return np.array([(P0[0] + j * step * u[0], P0[1] + j * step * u[1]) for j in range(j0, j1)])


def arc_track(P0, u, step, rho, j0, j1, left=True):
    """a circle of radius rho through P0 with heading u there, step j at arc length j * step"""
    n = nrm(u) if left else (u[1], -u[0])
    O = (P0[0] + rho * n[0], P0[1] + rho * n[1])
    out = []
    for j in range(j0, j1):
        a = j * step / rho
        out.append((O[0] - rho * n[0] * math.cos(a) + rho * u[0] * math.sin(a), O[1] - rho * n[1] * math.cos(a) + rho * u[1] * math.sin(a)))
    return np.array(out)


SEQ_KINDS = ("enter", "down", "leave", "cross", "collinear")


def sequence_cases():
    out = []
    i = 0
    for kind in SEQ_KINDS:
        for shape in ("straight", "arc"):
            for step in (0.05, 0.01):
                for w in WIDTHS:
                    for C in CENTRES:
                        d = (0.8, 0.6) if (i % 3 == 0) else ((1.0, 0.0) if i % 3 == 1 else _seeded_dirs(3, 5)[i % 3])
                        L = 60.0
                        lst = [mk(C, d, L)]
                        u = d
                        if kind == "enter":
                            u = rot(d, 20.0)
                            P0 = at(C, d, 20.0, -0.5 * w - 32.3 * step * math.sin(math.radians(20.0)))
                        elif kind == "down":
                            P0 = at(C, d, 20.0, 0.1 * w)
                        elif kind == "leave":
                            P0 = at(C, d, L - w - 20.5 * step, -0.15 * w) if (i // 3) % 2 == 0 else at(C, d, L - 32.5 * step, 0.05 * w)
                        elif kind == "cross":
                            X = at(C, d, 20.0 + 32.0 * step)
                            lst.append(mk(at(X, rot(d, 60.0), -12.0), rot(d, 60.0), 30.0))
                            P0 = at(C, d, 20.0, 0.1 * w)
                        else:
                            a = mk(C, d, 30.0)
                            b = np.array([a[2], a[3], a[2] + 30.0 * d[0], a[3] + 30.0 * d[1]])     # starts on the bytes a ends on
                            lst = [a, b]
                            P0 = at(C, d, 30.0 - 32.5 * step, 0.1 * w)
                        trk = straight_track(P0, u, step, 0, WAVE) if shape == "straight" else arc_track(P0, u, step, 8.0, 0, WAVE, left=(i % 2 == 0))
                        cover = [True] * WAVE if i % 2 == 0 else [(j % 7) != 3 for j in range(WAVE)]
                        out.append(_case("sequence", (kind, shape, step), lst, w, _ev(trk, cover)))
                        i += 1
    return out


@functools.lru_cache(maxsize=None)
def event_cases():
    return (orientation_cases() + knife_cases() + list_size_cases() + box_cases() + star_cases() + mixed_cases() + tiny_cases() +
            sequence_cases())


@functools.lru_cache(maxsize=None)
def event_reference():
    """per case, per event: the reference's record (replay_events)"""
    return [replay_events(c["list"], c["w"], c["events"]) for c in event_cases()]


# ----------------------------------------------------------------------------- run cases
def step_span(step):
    return 64.0 * step * (1.0 + 1e-9) + 1e-6      # the caller's runSpan


def decisions_clear(cur, x, y, w):
    """Does every decision quantity of cover() and minDistanceFrom at (x, y) clear its boundary by CLEAR?  Lengths against the strict
    minimum length w, the projection against the piece's extent grown by TOL (by 1e-6 m), the line distance against w and w / 2,
    the halves of a split against w: relative to the boundary's own value."""
    for sx, sy, ex, ey in cur:
        L = math.hypot(ex - sx, ey - sy)
        if abs(L - w) <= CLEAR * w:
            return False
        if L == 0.0:
            continue
        dx, dy = (ex - sx) / L, (ey - sy) / L
        t = (x - sx) * dx + (y - sy) * dy
        ld = abs((x - sx) * dy - (y - sy) * dx)
        # the reference tests the projection per coordinate: outside if beyond TOL in x or in y
        ax, ay = abs(dx), abs(dy)
        edges = [TOL / a for a in (ax, ay) if a > 1e-12]
        reach = min(edges)
        if abs(t + reach) <= 1e-6 or abs(t - L - reach) <= 1e-6:
            return False
        if t < -reach or t > L + reach:
            continue
        if abs(ld - w) <= CLEAR * w or abs(ld - 0.5 * w) <= CLEAR * 0.5 * w:
            return False
        if ld < 0.5 * w and (abs(t - w) <= CLEAR * w or abs(L - t - w) <= CLEAR * w):
            return False
    return True


def make_run(cls, sub, kind, w, ribbons0, track, lead, first=0, s=1, step=0.05, rho=8.0, step_ok=None, cover_mask=None, inject=None,
             adv=None, move_end=None, want_clean=False):
    """track: positions of steps -lead .. 63 * s (index 0 = step -lead).  The reference replays the lead-in and the window's steps
    before `first` with cover on; the list it leaves is the run's.  inject = (position, ribbon): a piece put into that list by hand."""
    full = (1 << WAVE) - 1
    step_ok = full if step_ok is None else step_ok
    cover_mask = full if cover_mask is None else cover_mask
    track = np.asarray(track, dtype=np.float64)
    assert len(track) == lead + 63 * s + 1
    pos = lambda j: track[j + lead]
    cur = np.ascontiguousarray(ribbons0, dtype=np.float64).reshape(-1, 4)
    with ribbon_width(w):
        last = ("none",)
        prev = None
        for j in range(-lead, first):
            x, y = pos(j)
            _, after = ref_event(cur, x, y, kind == 1 or ((cover_mask >> max(j, 0)) & 1) != 0)
            last, cur, prev = classify(cur, after), after[:WAVE], j
        if kind == 1 and adv is None:
            if last[0] == "move":
                adv, move_end = last[1], last[2]
            elif last[0] == "split":
                # the caller's guess after a split: which half the vehicle travels into
                f = last[1]
                dxp, dyp = cur[f + 1, 2] - cur[f, 0], cur[f + 1, 3] - cur[f, 1]
                nxt, here = pos(prev + 1), pos(prev)
                towards_end = ((nxt[0] - here[0]) * dxp + (nxt[1] - here[1]) * dyp) > 0.0
                adv, move_end = (f + 1, False) if towards_end else (f, True)
            else:
                raise AssertionError(f"{cls} {sub}: the lead-in ended on {last}, no piece to run on")
        if inject is not None:
            at_, rib = inject
            cur = np.insert(cur, at_, np.asarray(rib, dtype=np.float64), axis=0)
            if kind == 1 and at_ <= adv:
                adv += 1
        lst = cur.copy()
        # the reference from step `first` on, every step
        good, ends, clean = 0, [], True
        nsteps = 63 * s + 1
        for j in range(first, nsteps):
            lane = j if s == 1 else -(-j // s)          # the sample that vouches for step j
            x, y = pos(j)
            ok = ((step_ok >> lane) & 1) != 0
            cov = ((cover_mask >> lane) & 1) != 0
            clean = clean and want_clean and decisions_clear(cur, x, y, w)
            if not ok:
                break
            D, after = ref_event(cur, x, y, cov)
            what = classify(cur, after)
            if kind == 1:
                if not (cov and what == ("move", adv, move_end)):
                    break
                ends.append(after[adv, 2:].copy() if move_end else after[adv, :2].copy())
            else:
                if not (D == 0.0 and what == ("none",)):
                    break
            cur = after[:WAVE]
            good += 1
    poses = np.array([pos(i * s) for i in range(WAVE)])
    ell = 0.0 if s == 1 else s * step + 1e-6
    return {"cls": cls, "sub": sub, "kind": kind, "w": float(w), "list": lst, "poses": poses, "steps": track[lead:].copy(), "s": s, "first": first,
            "step_ok": step_ok, "cover_mask": cover_mask, "adv": 0 if adv is None else int(adv), "move_end": bool(move_end),
            "span": step_span(step) if s == 1 else 64.0 * ell, "ell": ell, "sin_dt": 0.0 if s == 1 else ell / rho,
            "ref_steps": good, "ref_ends": np.array(ends).reshape(-1, 2), "clean": bool(clean and want_clean)}


def claimed_steps(case, L):
    """how many steps from `first` on a run of L lanes claims"""
    return int(L) if case["s"] == 1 else ((int(L) - 1) * case["s"] + 1 if L > 0 else 0)


RUN_ORIENTS = [("axis", (1.0, 0.0)), ("345", (0.8, 0.6)), ("oblique", _seeded_dirs(2, 99)[1])]
OFFSETS = (0.0, 0.3, -0.3, 0.9, -0.9)      # of w / 2
FIRSTS = (0, 1, 31, 63)
LEAD = 3


def _down(C, d, L, forward, t0, off, step, j0, j1):
    """a straight track parallel to the piece, step 0 at t0 along it, `off` beside it, towards its end or its start"""
    u = d if forward else (-d[0], -d[1])
    return straight_track(at(C, d, t0, off), u, step, j0, j1)


def clean_run_cases():
    out = []
    i = 0
    L = 60.0
    for oname, d in RUN_ORIENTS:
        for w in WIDTHS:
            for off in OFFSETS:
                for forward in (True, False):
                    for first in FIRSTS:
                        for sibling in (True, False):
                            C = CENTRES[i % 2]
                            step = (0.05, 0.01)[(i // 2) % 2]
                            # no sibling: the first split leaves a front shorter than the minimum length, which vanishes at once
                            t_in = 20.0 if sibling else 0.5 * w
                            t0 = t_in + LEAD * step if forward else L - t_in - LEAD * step
                            trk = _down(C, d, L, forward, t0, off * 0.5 * w, step, -LEAD, WAVE)
                            out.append(make_run("clean", (oname, forward, first, sibling, off), 1, w, [mk(C, d, L)], trk, LEAD, first=first, step=step,
                                                want_clean=True))
                            i += 1
    return out


def ending_run_cases():
    out = []
    L = 60.0
    i = 0
    for oname, d in RUN_ORIENTS:
        for w in WIDTHS:
            for first in (0, 5):
                for step in (0.05, 0.01):
                    C = CENTRES[i % 2]
                    i += 1
                    base = [mk(C, d, L)]
                    # leaves the strict corridor at 2 degrees, around step 40
                    a = math.radians(2.0)
                    u = rot(d, 2.0)
                    P0 = at(C, d, 20.0, 0.5 * w - 40.3 * step * math.sin(a))
                    trk = straight_track(P0, u, step, -LEAD, WAVE)
                    out.append(make_run("ending", ("shallow", oname), 1, w, base, trk, LEAD, first=first, step=step))
                    # the remainder drops below the minimum length around step 40 (towards the end) / the front does (towards the start)
                    trk = _down(C, d, L, True, L - w - 40.5 * step, 0.1 * w, step, -LEAD, WAVE)
                    out.append(make_run("ending", ("rest", oname), 1, w, base, trk, LEAD, first=first, step=step))
                    trk = _down(C, d, L, False, w + 40.5 * step, -0.1 * w, step, -LEAD, WAVE)
                    out.append(make_run("ending", ("front", oname), 1, w, base, trk, LEAD, first=first, step=step))
                    # enters a crossing ribbon's strict corridor around step 40
                    for ang in (70.0, 15.0):
                        dq = rot(d, ang)
                        X = at(C, d, 20.0 + 40.3 * step + 0.5 * w / math.sin(math.radians(ang)), 0.1 * w)
                        trk = _down(C, d, L, True, 20.0, 0.1 * w, step, -LEAD, WAVE)
                        out.append(make_run("ending", ("crossing", oname), 1, w, base + [mk(at(X, dq, -12.0), dq, 30.0)], trk, LEAD, first=first, step=step))
                    # one step not executable / one step without cover()
                    trk = _down(C, d, L, True, 20.0, 0.1 * w, step, -LEAD, WAVE)
                    full = (1 << WAVE) - 1
                    out.append(make_run("ending", ("stepOk", oname), 1, w, base, trk, LEAD, first=first, step=step, step_ok=full & ~(1 << 37)))
                    out.append(make_run("ending", ("coverMask", oname), 1, w, base, trk, LEAD, first=first, step=step, cover_mask=full & ~(1 << 29)))
                    # an erasable piece anywhere in the list
                    tiny = mk(at(C, d, 300.0, 500.0), rot(d, 40.0), 0.5 * w)
                    for where in (0, 2):
                        out.append(make_run("ending", ("erasable", oname), 1, w, base, trk, LEAD, first=first, step=step, inject=(where, tiny)))
    return out


def quiet_run_cases():
    out = []
    L = 60.0
    i = 0
    full = (1 << WAVE) - 1
    for oname, d in RUN_ORIENTS:
        for w in WIDTHS:
            for first in FIRSTS:
                C = CENTRES[i % 2]
                step = (0.05, 0.01)[(i // 2) % 2]
                i += 1
                base = [mk(C, d, L), mk(at(C, d, 0.0, 40.0), d, L)]
                for side in (1.0, -1.0):
                    # between w / 2 and w, cover on: nothing splits
                    trk = _down(C, d, L, side > 0, 30.0, side * 0.75 * w, step, 0, WAVE)
                    out.append(make_run("quiet", ("between", oname), 2, w, base, trk, 0, first=first, step=step, want_clean=True))
                    # inside w / 2, cover off: nothing may change
                    trk = _down(C, d, L, side > 0, 30.0, side * 0.1 * w, step, 0, WAVE)
                    out.append(make_run("quiet", ("off", oname), 2, w, base, trk, 0, first=first, step=step, cover_mask=0, want_clean=True))
                # crossing from between into the strict corridor around step 35: ends with cover on, goes on where cover is off
                a = math.radians(3.0)
                P0 = at(C, d, 30.0, 0.5 * w + 35.3 * step * math.sin(a))
                trk = straight_track(P0, rot(d, -3.0), step, 0, WAVE)
                out.append(make_run("quiet", ("into", oname), 2, w, base, trk, 0, first=min(first, 31), step=step))
                out.append(make_run("quiet", ("into-off", oname), 2, w, base, trk, 0, first=min(first, 31), step=step, cover_mask=full & ((1 << 30) - 1)))
                # leaving the ribbon over its edge at w around step 35
                P0 = at(C, d, 30.0, w - 35.3 * step * math.sin(a))
                trk = straight_track(P0, rot(d, 3.0), step, 0, WAVE)
                out.append(make_run("quiet", ("out", oname), 2, w, base, trk, 0, first=min(first, 31), step=step))
                # an erasable piece: with cover on every step would change the list
                tiny = mk(at(C, d, 300.0, 500.0), rot(d, 40.0), 0.5 * w)
                trk = _down(C, d, L, True, 30.0, 0.75 * w, step, 0, WAVE)
                out.append(make_run("quiet", ("erasable-on", oname), 2, w, base, trk, 0, first=first, step=step, inject=(1, tiny)))
                out.append(make_run("quiet", ("erasable-off", oname), 2, w, base, trk, 0, first=first, step=step, inject=(1, tiny), cover_mask=0))
    return out


KNIFE_STEP = 30
KNIFE_ULPS = 12
KNIFE_DELTAS = (1e-11, 1e-10, 1e-9, 3e-9, 1e-8, 3e-8, 1e-7, 1e-6)


def knife_run_cases():
    """Clean corridor tracks whose step 30 alone is moved onto a knife edge of the reference's own decision there, found by bisection on
    the replay (the list as steps 0 .. 29 left it): across the strict corridor's edge along the normal ("strict"), and along the piece
    to where the remainder reaches the minimum length ("rest").  Steps of one ulp of the coordinate over +-12, and +-1e-11 .. 1e-6 m:
    inside the 1e-9 guard of pp_corridor_run the run must stop at step 30 whatever its own arithmetic says; beyond the guard its
    arithmetic (the piece's line as the run found it) and the replay's (the line from the moved start) must agree."""
    out = []
    L, step, k = 60.0, 0.05, KNIFE_STEP
    i = 0
    for oname, d in RUN_ORIENTS:
        for w in WIDTHS:
            for C in CENTRES:
                for what in ("strict", "rest"):
                    side = 1.0 if i % 2 == 0 else -1.0
                    i += 1
                    off = 0.3 * 0.5 * w * side
                    t0 = 20.0 + LEAD * step if what == "strict" else L - w - k * step
                    base_trk = _down(C, d, L, True, t0, off, step, -LEAD, WAVE)
                    cur = mk(C, d, L).reshape(1, 4)
                    with ribbon_width(w):
                        for j in range(-LEAD, k):
                            x, y = base_trk[j + LEAD]
                            _, cur = ref_event(cur, x, y, True)
                        adv = len(cur) - 1
                        before = cur

                        def moves(p):
                            return classify(before, orc.ribbons_cover(before, p[0], p[1], True, cap=CAP)) == ("move", adv, False)
                        if what == "strict":
                            p0, u = at(C, d, t0 + k * step, 0.5 * w * side), (side * nrm(d)[0], side * nrm(d)[1])
                        else:
                            p0, u = at(C, d, L - w, off), d
                        sv = ulp_vec(p0, u)
                        size = math.hypot(sv[0], sv[1])
                        k0 = find_flip(moves, p0, sv, int(1e-5 / size))
                    ks = list(range(k0 - KNIFE_ULPS + 1, k0 + KNIFE_ULPS + 1))
                    for delta in KNIFE_DELTAS:
                        n = max(int(round(delta / size)), KNIFE_ULPS + 1)
                        ks += [k0 - n, k0 + 1 + n]
                    for kk in ks:
                        trk = base_trk.copy()
                        trk[k + LEAD] = stepped(p0, sv, kk)
                        out.append(make_run("knife-run", (what, oname, (kk - k0) * size), 1, w, [mk(C, d, L)], trk, LEAD, step=step))
    return out


LONG_S = (2, 5, 16)
DELTAS = (1e-6, 1e-5, 3e-5, 1e-4)


def long_clean_cases():
    out = []
    L = 60.0
    i = 0
    for oname, d in RUN_ORIENTS:
        for s in LONG_S:
            step = 0.05 / s
            for io, off in enumerate(OFFSETS):
                for forward in ((True, False) if off == 0.0 else ((io + s) % 2 == 0,)):
                    C, w = CENTRES[i % 2], WIDTHS[i % 3]
                    i += 1
                    t0 = 20.0 + LEAD * step if forward else L - 20.0 - LEAD * step
                    trk = _down(C, d, L, forward, t0, off * 0.5 * w, step, -LEAD, 63 * s + 1)
                    out.append(make_run("long-clean", ("corridor", oname, s), 1, w, [mk(C, d, L)], trk, LEAD, s=s, step=step, want_clean=True))
            for side in (1.0, -1.0):
                C, w = CENTRES[i % 2], WIDTHS[i % 3]
                i += 1
                trk = _down(C, d, L, side > 0, 30.0, side * 0.75 * w, step, 0, 63 * s + 1)
                out.append(make_run("long-clean", ("quiet", oname, s), 2, w, [mk(C, d, L)], trk, 0, s=s, step=step, want_clean=True))
    return out


def _bulge_track(C, d, t_apex, dist, rho, s, step, lead, m=20, outward=1.0):
    """An arc of radius rho whose farthest point from the piece's centre line (on the `outward` side) is `dist` away, at t_apex along the
    piece, and lies midway between samples m and m + 1; travel towards the piece's end."""
    n = nrm(d)
    n = (outward * n[0], outward * n[1])
    A = at(C, d, t_apex)
    O = (A[0] + (dist - rho) * n[0], A[1] + (dist - rho) * n[1])
    out = []
    for j in range(-lead, 63 * s + 1):
        a = (j - (m + 0.5) * s) * step / rho
        out.append((O[0] + rho * (n[0] * math.cos(a) + d[0] * math.sin(a)), O[1] + rho * (n[1] * math.cos(a) + d[1] * math.sin(a))))
    return np.array(out)


def long_trap_cases():
    out = []
    i = 0
    L = 60.0
    for oname, d in RUN_ORIENTS[1:]:
        for s in LONG_S:
            step = 0.05 / s
            for rho in (8.0, 10.0):
                for delta in DELTAS:
                    w = WIDTHS[i % 3]
                    C = CENTRES[i % 2]
                    side = 1.0 if i % 4 < 2 else -1.0
                    i += 1
                    base = [mk(C, d, L)]
                    # bulges out of the strict corridor by delta between samples 20 and 21
                    trk = _bulge_track(C, d, 25.0, 0.5 * w + delta, rho, s, step, LEAD, outward=side)
                    out.append(make_run("long-trap", ("strict", delta), 1, w, base, trk, LEAD, s=s, step=step, rho=rho))
                    # the same where the piece ends: the apex lies where the remainder reaches the minimum length
                    trk = _bulge_track(C, d, L - w, 0.5 * w + delta, rho, s, step, LEAD, outward=side)
                    out.append(make_run("long-trap", ("end", delta), 1, w, base, trk, LEAD, s=s, step=step, rho=rho))
                    # well inside the piece's own corridor, bulging INTO a parallel sibling's strict corridor by delta
                    a0 = 0.25 * w
                    sib = mk(at(C, d, 0.0, side * (a0 - delta + 0.5 * w)), d, L)
                    trk = _bulge_track(C, d, 25.0, a0, rho, s, step, LEAD, outward=side)
                    out.append(make_run("long-trap", ("sibling", delta), 1, w, base + [sib], trk, LEAD, s=s, step=step, rho=rho, adv=1, move_end=False))
                    # quiet: between the corridors, bulging out of the ribbon (w) / into the strict corridor (w / 2)
                    trk = _bulge_track(C, d, 25.0, w + delta, rho, s, step, 0, outward=side)
                    out.append(make_run("long-trap", ("quiet-out", delta), 2, w, base, trk, 0, s=s, step=step, rho=rho))
                    trk = _bulge_track(C, d, 25.0, -(0.5 * w - delta), rho, s, step, 0, outward=-side)
                    out.append(make_run("long-trap", ("quiet-in", delta), 2, w, base, trk, 0, s=s, step=step, rho=rho))
    return out


@functools.lru_cache(maxsize=None)
def run_cases():
    return clean_run_cases() + ending_run_cases() + quiet_run_cases() + knife_run_cases() + long_clean_cases() + long_trap_cases()


# ----------------------------------------------------------------------------- pp_event_stride
def event_stride_set():
    """(D, inc, ng): D = k inc +- {0, 1, 2, 4} ulp for k = 1 .. ng + 3, and 0, inc, DBL_MAX"""
    Ds, incs, ngs = [], [], []
    for inc in (0.05, 0.1, 0.25, 1.0 / 3.0, 0.0125):
        for ng in (8, 1508):
            k = np.arange(1, ng + 4, dtype=np.float64)
            base = k * inc
            vals = [base]
            for u in (1, 2, 4):
                up, dn = base.copy(), base.copy()
                for _ in range(u):
                    up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
                vals += [up, dn]
            # the running sum k times inc, where the subtraction loop's own rounding lands
            acc = np.cumsum(np.full(ng + 3, inc))
            v = np.concatenate(vals + [acc, np.array([0.0, inc, np.finfo(np.float64).max])])
            Ds.append(v)
            incs.append(np.full(v.size, inc))
            ngs.append(np.full(v.size, ng, dtype=np.int32))
    return np.concatenate(Ds), np.concatenate(incs), np.concatenate(ngs)


def event_stride_reference(D, inc, ng):
    """the loop of Edge.cpp:153-154, literally: `while tc > inc and m <= ng: tc -= inc; m += 1` for every element at once (one pass of
    the loop body per iteration here, in IEEE doubles as Python's floats are)"""
    tc, m = np.array(D, dtype=np.float64), np.zeros(len(D), dtype=np.int32)
    while True:
        go = (tc > inc) & (m <= ng)
        if not go.any():
            return m
        tc[go] -= inc[go]
        m[go] += 1


def event_stride_reference_scalar(D, inc, ng):
    m, tc = 0, float(D)
    while tc > inc and m <= ng:
        tc -= inc
        m += 1
    return m
