"""ctypes loader of tests/probe/libpp_device_probe.so: the small device functions of path_planner_amd/csrc/pp_device.h, one lane per
element, with numpy in and numpy out.  __graft_entry__.build() compiles the library; PP_DEVICE_PROBE_LIB points at another build of it
(a copy of csrc/ with one primitive changed on purpose, to see that the tests notice)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "probe", "libpp_device_probe.so")

_lib = []


def lib_path():
    return os.environ.get("PP_DEVICE_PROBE_LIB") or DEFAULT_LIB


def lib():
    if not _lib:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run build() (python __graft_entry__.py) first")
        L = C.CDLL(path)
        vp, ll, i32, dbl = C.c_void_p, C.c_longlong, C.c_int, C.c_double
        for name, args in [
            ("ppp_sincos_bounded", [vp, vp, vp, ll]), ("ppp_sincos_bounded_tab", [vp, vp, vp, ll]), ("ppp_sincos", [vp, vp, vp, ll]),
            ("ppp_cr_sincos", [vp, vp, vp, ll]), ("ppp_cr_atan2", [vp, vp, vp, ll]), ("ppp_cr_acos", [vp, vp, ll]),
            ("ppp_mod2pi", [vp, vp, ll]), ("ppp_udiv_small", [vp, vp, vp, ll]),
            ("ppp_is_blocked", [vp, i32, i32, i32, dbl, vp, vp, vp, ll]),
            ("ppp_blocked_cell", [vp, i32, i32, i32, dbl, vp, vp, vp, vp, vp, vp, ll]),
            ("ppp_line_distance_lt", [vp, vp, vp, vp, ll]), ("ppp_obstacle_hit", [vp, vp, vp, vp, vp, ll]),
        ]:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        _lib.append(L)
    return _lib[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP error {rc}")


def _sincos(name, x):
    x = _f64(x)
    s, c = np.empty_like(x), np.empty_like(x)
    _ck(getattr(lib(), name)(_p(x), _p(s), _p(c), x.size), name)
    return s, c


def sincos_bounded(x, tab=False):
    return _sincos("ppp_sincos_bounded_tab" if tab else "ppp_sincos_bounded", x)


def sincos(x):
    return _sincos("ppp_sincos", x)


def cr_sincos(x):
    return _sincos("ppp_cr_sincos", x)


def cr_atan2(y, x):
    y, x = _f64(y), _f64(x)
    assert y.size == x.size
    out = np.empty_like(x)
    _ck(lib().ppp_cr_atan2(_p(y), _p(x), _p(out), x.size), "ppp_cr_atan2")
    return out


def cr_acos(v):
    v = _f64(v)
    out = np.empty_like(v)
    _ck(lib().ppp_cr_acos(_p(v), _p(out), v.size), "ppp_cr_acos")
    return out


def mod2pi(t):
    t = _f64(t)
    out = np.empty_like(t)
    _ck(lib().ppp_mod2pi(_p(t), _p(out), t.size), "ppp_mod2pi")
    return out


def udiv_small(x, d):
    x = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)
    d = np.ascontiguousarray(np.broadcast_to(np.asarray(d, dtype=np.uint32), x.shape))
    out = np.empty_like(x)
    _ck(lib().ppp_udiv_small(_p(x), _p(d), _p(out), x.size), "ppp_udiv_small")
    return out


def pack_grid(cells):
    """rows x cols of 0 / 1 -> (rows x words-per-row uint32, words per row): bit (c & 31) of word c >> 5, as ppgpu_set_grid packs it."""
    cells = np.asarray(cells, dtype=np.uint8)
    rows, cols = cells.shape
    wpr = (cols + 31) // 32
    if rows == 0 or cols == 0:
        return np.zeros((rows, wpr), dtype=np.uint32), wpr
    padded = np.zeros((rows, wpr * 32), dtype=np.uint8)
    padded[:, :cols] = cells != 0
    bits = np.packbits(padded.reshape(rows, wpr, 32), axis=2, bitorder="little").view("<u4").reshape(rows, wpr)
    return np.ascontiguousarray(bits), wpr


def is_blocked(cells, res, x, y):
    bits, wpr = pack_grid(cells)
    x, y = _f64(x), _f64(y)
    assert x.size == y.size
    out = np.empty(x.size, dtype=np.uint8)
    _ck(lib().ppp_is_blocked(_p(bits), cells.shape[0], cells.shape[1], wpr, float(res), _p(x), _p(y), _p(out), x.size), "ppp_is_blocked")
    return out


def blocked_cell(cells, res, x, y):
    """(outside, row, col, pp_blocked_test of the cell's word) per point."""
    bits, wpr = pack_grid(cells)
    x, y = _f64(x), _f64(y)
    assert x.size == y.size
    outside, blocked = np.empty(x.size, dtype=np.uint8), np.empty(x.size, dtype=np.uint8)
    row, col = np.empty(x.size, dtype=np.uint32), np.empty(x.size, dtype=np.uint32)
    _ck(lib().ppp_blocked_cell(_p(bits), cells.shape[0], cells.shape[1], wpr, float(res), _p(x), _p(y), _p(outside), _p(row), _p(col),
                               _p(blocked), x.size), "ppp_blocked_cell")
    return outside, row, col, blocked


def line_distance_lt(num, sqL, lim):
    num, sqL, lim = _f64(num), _f64(sqL), _f64(lim)
    assert num.size == sqL.size == lim.size
    out = np.empty(num.size, dtype=np.uint8)
    _ck(lib().ppp_line_distance_lt(_p(num), _p(sqL), _p(lim), _p(out), num.size), "ppp_line_distance_lt")
    return out


def obstacle_hit(obst12, x, y, t):
    """obst12: n x 12 raw PPObst rows {X, Y, cosYaw, sinYaw, Speed, Time, halfL, halfW, reach, pad x 3}; row i against point i."""
    ob = np.ascontiguousarray(obst12, dtype=np.float64).reshape(-1, 12)
    x, y, t = _f64(x), _f64(y), _f64(t)
    assert ob.shape[0] == x.size == y.size == t.size
    out = np.empty(x.size, dtype=np.int32)
    _ck(lib().ppp_obstacle_hit(_p(ob), _p(x), _p(y), _p(t), _p(out), x.size), "ppp_obstacle_hit")
    return out
