"""ctypes loader of tests/probe/libpp_cover_probe.so: the pieces of the coverage state machine (pp_ribbons_event, pp_corridor_run,
pp_quiet_run, pp_event_stride, pp_box_scan, pp_any_tiny_ribbon, pp_lane_ribbon_contains, pp_lane_cover_strict), each alone, with numpy
in and numpy out.  __graft_entry__.build() compiles the library; PP_COVER_PROBE_LIB points at another build of it (a copy of csrc/ with
one guard changed on purpose, to see that the tests notice)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "probe", "libpp_cover_probe.so")
WAVE = 64
FINISH_MAX = 8      # PP_FINISH_MAX: ribbons of a child slot the lane form covers

_lib = []


def lib_path():
    return os.environ.get("PP_COVER_PROBE_LIB") or DEFAULT_LIB


def lib():
    if not _lib:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run build() (python __graft_entry__.py) first")
        L = C.CDLL(path)
        vp, ll = C.c_void_p, C.c_longlong
        for name, args in [
            ("ppc_cover_events", [vp, vp, vp, vp, vp, ll, vp, vp, vp, vp]),
            ("ppc_cover_runs", [vp, vp, vp, vp, vp, ll, vp, vp]),
            ("ppc_lane_contains", [vp, vp, vp, vp, vp, vp, vp, ll]),
            ("ppc_lane_cover_strict", [vp, vp, vp, vp, vp, vp, vp, ll]),
            ("ppc_box_scan", [vp, vp, vp, vp, vp, vp, vp, vp, ll]),
            ("ppc_event_stride", [vp, vp, vp, vp, ll]),
        ]:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        _lib.append(L)
    return _lib[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP error {rc}")


def pack_lists(lists):
    """lists of k_i x 4 (k_i <= 64) -> (ncase x 64 x 4 with the zero ribbon beyond k_i, the k_i)."""
    ribs = np.zeros((len(lists), WAVE, 4))
    ns = np.zeros(len(lists), dtype=np.int32)
    for i, r in enumerate(lists):
        r = np.asarray(r, dtype=np.float64).reshape(-1, 4)
        assert r.shape[0] <= WAVE, "a list stays within the 64 lanes"
        ribs[i, :r.shape[0]] = r
        ns[i] = r.shape[0]
    return ribs, ns


def cover_events(lists, ws, events):
    """Case i: lists[i] (k x 4, k <= 64), width ws[i], events[i] (m x 3: x, y, doCover) applied one after the other, the count
    clamped to 64 between them.  -> (offsets ncase + 1, count, D, adv, ribbons nev x 64 x 4) with the events of case i at
    offsets[i] .. offsets[i + 1] - 1."""
    ribs, ns = pack_lists(lists)
    ws = _f64(ws)
    assert ws.size == len(lists) == len(events)
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    for i, e in enumerate(events):
        off[i + 1] = off[i] + np.asarray(e).reshape(-1, 3).shape[0]
    nev = int(off[-1])
    ev = np.concatenate([np.asarray(e, dtype=np.float64).reshape(-1, 3) for e in events]) if nev else np.zeros((0, 3))
    ev = np.ascontiguousarray(ev)
    cnt, adv = np.zeros(nev, dtype=np.int32), np.zeros(nev, dtype=np.int32)
    D, out = np.zeros(nev), np.zeros((nev, WAVE, 4))
    if len(lists):
        _ck(lib().ppc_cover_events(_p(ribs), _p(ns), _p(ws), _p(off), _p(ev), len(lists), _p(cnt), _p(D), _p(adv), _p(out)), "ppc_cover_events")
    return off, cnt, D, adv, out


def cover_runs(lists, poses, kind, adv, move_end, first, step_ok, cover_mask, w, span, ell, sin_dt):
    """One run per case: kind 1 = pp_corridor_run, 2 = pp_quiet_run; poses ncase x 64 x 2; step_ok / cover_mask 64-bit masks.
    -> (L, new endpoint ncase x 2)."""
    ribs, ns = pack_lists(lists)
    nc = len(lists)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(nc, WAVE, 2)
    ints = np.ascontiguousarray(np.stack([ns, _i32(kind), _i32(adv), _i32(move_end), _i32(first)], axis=1), dtype=np.int32)
    masks = np.ascontiguousarray(np.stack([np.asarray(step_ok, dtype=np.uint64), np.asarray(cover_mask, dtype=np.uint64)], axis=1))
    dbls = np.ascontiguousarray(np.stack([_f64(w), _f64(span), _f64(ell), _f64(sin_dt)], axis=1))
    L, xy = np.zeros(nc, dtype=np.int32), np.zeros((nc, 2))
    if nc:
        _ck(lib().ppc_cover_runs(_p(ribs), _p(poses), _p(ints), _p(masks), _p(dbls), nc, _p(L), _p(xy)), "ppc_cover_runs")
    return L, xy


def lane_contains(rib4, x, y, w):
    """pp_lane_ribbon_contains of ribbon i at point i -> (inside, strict, projection n x 2)."""
    rib = np.ascontiguousarray(rib4, dtype=np.float64).reshape(-1, 4)
    x, y, w = _f64(x), _f64(y), _f64(w)
    n = x.size
    assert rib.shape[0] == n == y.size == w.size
    inside, strict, pxy = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros((n, 2))
    _ck(lib().ppc_lane_contains(_p(rib), _p(x), _p(y), _p(w), _p(inside), _p(strict), _p(pxy), n), "ppc_lane_contains")
    return inside, strict, pxy


def lane_cover_strict(lists, stride, x, y, w):
    """pp_lane_cover_strict on one zeroed child slot of 8 ribbons per case holding lists[i] (<= 8) -> (returned count, slots n x 8 x 4)."""
    n = len(lists)
    slots = np.zeros((n, FINISH_MAX, 4))
    nrib = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(lists):
        r = np.asarray(r, dtype=np.float64).reshape(-1, 4)
        assert r.shape[0] <= FINISH_MAX
        slots[i, :r.shape[0]] = r
        nrib[i] = r.shape[0]
    stride, x, y, w = _i32(stride), _f64(x), _f64(y), _f64(w)
    out = np.zeros(n, dtype=np.int32)
    if n:
        _ck(lib().ppc_lane_cover_strict(_p(slots), _p(nrib), _p(stride), _p(x), _p(y), _p(w), _p(out), n), "ppc_lane_cover_strict")
    return out, slots


def box_scan(lists, x, y, grow, thr):
    """pp_box_scan and pp_any_tiny_ribbon of lists[i] at point i -> (inBox, boxCount, boxIdx, tiny, q)."""
    n = len(lists)
    off = np.zeros(n + 1, dtype=np.int64)
    for i, r in enumerate(lists):
        off[i + 1] = off[i] + np.asarray(r).reshape(-1, 4).shape[0]
    flat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 4) for r in lists])) if off[-1] else np.zeros((0, 4))
    x, y, grow, thr = _f64(x), _f64(y), _f64(grow), _f64(thr)
    oi, oq = np.zeros((n, 4), dtype=np.int32), np.zeros(n)
    if n:
        _ck(lib().ppc_box_scan(_p(flat), _p(off), _p(x), _p(y), _p(grow), _p(thr), _p(oi), _p(oq), n), "ppc_box_scan")
    return oi[:, 0], oi[:, 1], oi[:, 2], oi[:, 3], oq


def event_stride(D, inc, ng):
    D, inc, ng = _f64(D), _f64(inc), _i32(ng)
    assert D.size == inc.size == ng.size
    out = np.zeros(D.size, dtype=np.int32)
    if D.size:
        _ck(lib().ppc_event_stride(_p(D), _p(inc), _p(ng), _p(out), D.size), "ppc_event_stride")
    return out
