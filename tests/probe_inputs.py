"""Inputs and references of the device-primitive tests (tests/test_gpu_device_math.py runs them on the device, tests/test_device_probe_inputs.py
checks the sets themselves and the host build of pp_cr.h on the CPU).

Every set is deterministic.  Sets for a function with a wave-wide shortcut come with the numpy restatement of the shortcut's GUARD
(never of its result): `orders()` turns it into the two evaluation orders of the ballot-independence check, and `wave_routes()` says which
elements' waves took the guarded route in a given order.

References: mpmath at 240 bits for the transcendentals, as a (nearest double, remainder) pair; numpy float64 for the reference's literal
expressions, where IEEE division, square root and floor are the same operation on both sides."""
import functools
from fractions import Fraction

import numpy as np

WAVE = 64
MP_PREC = 240
TWO_PI = 6.283185307179586476925286766559      # PP_TWO_PI
INV_TWO_PI = 0.15915494309189533576888376337251


# ----------------------------------------------------------------------------- evaluation orders
def pad_off_wave(*arrays):
    """The same arrays, one ordinary element (a copy of the first) longer if their length is a multiple of the wave: the last wave of
    every launch is partial."""
    n = len(arrays[0])
    if n % WAVE != 0:
        return arrays if len(arrays) > 1 else arrays[0]
    out = tuple(np.concatenate([a, a[:1]]) for a in arrays)
    return out if len(out) > 1 else out[0]


def orders(guard):
    """(mixed, separated): two permutations of range(n).  Mixed spreads the guarded elements evenly, so that every wave holds some
    when there are enough of them (wave_routes tells); separated puts every unguarded element first, in whole waves of their own."""
    guard = np.asarray(guard, dtype=bool)
    n = guard.size
    assert n % WAVE != 0, "n must leave a partial last wave"
    b, o = np.nonzero(guard)[0], np.nonzero(~guard)[0]
    key = np.empty(n)
    key[b] = (np.arange(b.size) + 0.5) / max(b.size, 1)
    key[o] = np.arange(o.size) / max(o.size, 1)
    mixed = np.argsort(key, kind="stable")
    separated = np.concatenate([o, b])
    return mixed, separated


def solitary_order(guard, stride):
    """(index, lanes): a launch in which every `stride`-th guarded element sits alone in its wave, at a varying lane, among unguarded
    elements (recycled), so that no other guarded lane decides the wave's route for it.  index[lanes] are those guarded elements."""
    guard = np.asarray(guard, dtype=bool)
    b, o = np.nonzero(guard)[0][::stride], np.nonzero(~guard)[0]
    index = np.resize(o, b.size * WAVE + 17)
    lanes = np.arange(b.size) * WAVE + (np.arange(b.size) * 7) % WAVE
    index[lanes] = b
    return index, lanes


def wave_routes(guard_in_order):
    """Per element: does its wave (64 consecutive elements of this launch order) hold a guarded lane?"""
    g = np.asarray(guard_in_order, dtype=bool)
    n = g.size
    padded = np.zeros(-(-n // WAVE) * WAVE, dtype=bool)
    padded[:n] = g
    return np.repeat(padded.reshape(-1, WAVE).any(axis=1), WAVE)[:n]


def route_counts(guard):
    """(elements whose wave takes the guarded route in the mixed order, elements whose wave does not in the separated order)."""
    guard = np.asarray(guard, dtype=bool)
    mixed, separated = orders(guard)
    return int(wave_routes(guard[mixed]).sum()), int((~wave_routes(guard[separated])).sum())


def neighbours(v, k):
    """v with its k nearest doubles on either side, per element: shape (len(v), 2k + 1) flattened."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    cols = [v]
    lo, hi = v, v
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        cols += [lo, hi]
    return np.stack(cols, axis=1).reshape(-1)


# ----------------------------------------------------------------------------- mpmath references
def _mp():
    import mpmath
    mpmath.mp.prec = MP_PREC
    return mpmath.mp


def nearest_double(v):
    """The mpf v rounded to the nearest double (ties to even), subnormals included: the division of two integers is correctly rounded."""
    sign, man, exp, _ = v._mpf_
    if man == 0:
        return 0.0
    f = float(Fraction(man) * Fraction(2) ** exp) if exp < 0 else float(man * 2 ** exp)
    return -f if sign else f


def _pair(mp, v):
    hi = nearest_double(v)
    return hi, float(v - mp.mpf(hi))


def ref_sincos(x):
    """sin and cos of every double of x: (sin hi, sin lo, cos hi, cos lo); hi is the correctly rounded value, hi + lo the value to ~1e-32."""
    mp = _mp()
    out = np.empty((4, len(x)))
    for i, xi in enumerate(np.asarray(x, dtype=np.float64).tolist()):
        c, s = mp.cos_sin(mp.mpf(xi))
        out[0, i], out[1, i] = _pair(mp, s)
        out[2, i], out[3, i] = _pair(mp, c)
    return out


def ref_atan2(y, x):
    mp = _mp()
    out = np.empty((2, len(x)))
    for i, (yi, xi) in enumerate(zip(np.asarray(y, dtype=np.float64).tolist(), np.asarray(x, dtype=np.float64).tolist())):
        out[0, i], out[1, i] = _pair(mp, mp.atan2(mp.mpf(yi), mp.mpf(xi)))
    return out


def ref_acos(v):
    mp = _mp()
    out = np.empty((2, len(v)))
    for i, vi in enumerate(np.asarray(v, dtype=np.float64).tolist()):
        out[0, i], out[1, i] = _pair(mp, mp.acos(mp.mpf(vi)))
    return out


def ulp_error(got, hi, lo):
    """|got - (hi + lo)| in ulps of the exact value hi + lo (hi its nearest double).  An exact zero admits only zero."""
    got, hi, lo = (np.asarray(a, dtype=np.float64) for a in (got, hi, lo))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.spacing(np.abs(hi))
        m, _ = np.frexp(np.abs(hi))
        # hi a power of two and the exact value just inside the binade below: its ulp is half of spacing(hi)
        u = np.where((m == 0.5) & (np.sign(lo) == -np.sign(hi)) & (np.abs(hi) > 2.3e-308), u / 2, u)
        err = np.abs((got - hi) - lo) / u
    err = np.where(hi == 0.0, np.where(got == 0.0, 0.0, np.inf), err)
    return np.where(np.isnan(got), np.inf, err)


# ----------------------------------------------------------------------------- sine / cosine
def _multiples(ks, num, den):
    """nearest double to k * pi * num / den for every k"""
    mp = _mp()
    unit = mp.pi * num / den
    return np.array([nearest_double(unit * int(k)) for k in ks])


def _signed(ks):
    ks = np.asarray(list(ks), dtype=np.int64)
    return np.concatenate([ks, -ks[ks != 0]])


@functools.lru_cache(maxsize=None)
def sincos_bounded_set():
    """pp_sincos_bounded's arguments, all |x| < 1e5."""
    rng = np.random.default_rng(20240501)
    ks = _signed(list(range(0, 2001)) + list(range(2037, 63662, 37)) + [63661])
    parts = [
        neighbours(_multiples(ks, 1, 2), 1),                                       # k pi/2: the reduction's zeros
        neighbours(_multiples(_signed(range(1, 256, 2)), 1, 4), 1),                # odd k pi/4: where sin and cos swap roles
        neighbours([0.0, -0.0, 5e-324, 1e-300, 1e-8, 0.3, 0.78125, -5e-324, -1e-300, -1e-8, -0.3, -0.78125], 2),
        np.array([99999.99999999999, -99999.99999999999]),
        rng.uniform(-9e4, 9e4, 5000),
        rng.uniform(-7.0, 7.0, 5000),
    ]
    x = pad_off_wave(np.concatenate(parts))
    assert np.all(np.abs(x) < 1e5)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sincos_bounded_ref():
    r = ref_sincos(sincos_bounded_set())
    r.setflags(write=False)
    return r


SINCOS_LIBRARY_LANES = np.array([1e5, 2.5e5, np.inf, -np.inf, np.nan, -1e5, -2.5e5, np.nextafter(1e5, np.inf), 1e6, 3e9])


@functools.lru_cache(maxsize=None)
def sincos_route_set():
    """pp_sincos: the bounded set plus enough lanes at or beyond 1e5 (or not finite) to put one into every wave.  Returns (x, guard)."""
    base = sincos_bounded_set()
    nwaves = -(-base.size // WAVE) + 40
    extra = np.resize(SINCOS_LIBRARY_LANES, 2 * nwaves)
    if (base.size + extra.size) % WAVE == 0:
        extra = np.resize(SINCOS_LIBRARY_LANES, 2 * nwaves + 1)
    x = np.concatenate([base, extra])                    # the bounded set first: element i of it is element i here
    guard = ~(np.abs(x) < 1.0e5)
    x.setflags(write=False)
    return x, guard


CR_CHUNKS = 5


@functools.lru_cache(maxsize=None)
def cr_sincos_set():
    """pp_cr_sincos' arguments, |x| < 1e6: the bounded set, k pi/2 on to 636 619 in steps of 37, and the odd multiples of pi/32 (the ties
    of the reduction by pi/16)."""
    ks = _signed(list(range(63661 + 37, 636620, 37)) + [636619])
    parts = [
        sincos_bounded_set(),
        neighbours(_multiples(ks, 1, 2), 1),
        neighbours(_multiples(_signed(range(1, 1024, 2)), 1, 32), 1),
        neighbours(_multiples(_signed(range(1, 10185917, 203718)), 1, 32), 1),     # ... and some out to 1e6
        np.array([999999.9999999999, -999999.9999999999]),
    ]
    x = pad_off_wave(np.concatenate(parts))
    assert np.all(np.abs(x) < 1e6)
    x.setflags(write=False)
    return x


def cr_sincos_chunk(i):
    """Chunk i of CR_CHUNKS of cr_sincos_set(), interleaved so that every chunk holds every kind of argument; at most 30 000 values."""
    x = cr_sincos_set()[i::CR_CHUNKS]
    assert x.size <= 30000
    return pad_off_wave(x)


@functools.lru_cache(maxsize=None)
def cr_sincos_chunk_ref(i):
    r = ref_sincos(cr_sincos_chunk(i))
    r.setflags(write=False)
    return r


CR_SINCOS_BEYOND = np.array([1e6, -1e6, 1.5e6, 1e7, -3.3e8, 1e12, 1e15, 2.0 ** 60, 1e22, -1e100, 1e300])


# ----------------------------------------------------------------------------- atan2 / acos
def _pairs_with_signs(y, x):
    return [(sy * y, sx * x) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]


@functools.lru_cache(maxsize=None)
def atan2_set():
    """(y, x) for pp_cr_atan2: finite, no zero."""
    rng = np.random.default_rng(20240502)
    n = 6000
    y = rng.uniform(-100, 100, n)
    x = rng.uniform(-100, 100, n)
    i = np.arange(n)
    y[i % 5 == 0] *= 1e-9                                 # cr_trig_check.cpp's distribution
    x[i % 11 == 0] *= 1e-12
    named = [(1e-310, 1.0), (1e-305, 1e5), (3e-300, 1.0), (1e-300, -1.0), (-1e-300, -1.0), (1.0, 1e-300), (1.0, -1e-300), (1e300, 1e-300),
             (5e-324, 5e-324), (1e308, 1e308), (1e-200, 1e-200), (1e200, -1e200)]
    named += _pairs_with_signs(1e-17, 1.0) + _pairs_with_signs(1.0, 1.0) + _pairs_with_signs(3.0, 3.0)
    named += [(b, a) for a, b in named]
    named += [(-a, b) for a, b in named]
    yy = np.concatenate([y, np.array([p[0] for p in named])])
    xx = np.concatenate([x, np.array([p[1] for p in named])])
    yy, xx = pad_off_wave(yy, xx)
    assert np.all(np.isfinite(yy) & np.isfinite(xx) & (yy != 0) & (xx != 0))
    yy.setflags(write=False), xx.setflags(write=False)
    return yy, xx


@functools.lru_cache(maxsize=None)
def atan2_ref():
    r = ref_atan2(*atan2_set())
    r.setflags(write=False)
    return r


def atan2_guard_set():
    """Zeros, axes and infinities: what pp_cr_atan2 hands to the library, which must return numpy.arctan2's bits."""
    v = [0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e300, -1e300, np.inf, -np.inf]
    p = [(a, b) for a in v for b in v if a == 0 or b == 0 or np.isinf(a) or np.isinf(b)]
    y, x = np.array([q[0] for q in p]), np.array([q[1] for q in p])
    return pad_off_wave(y, x)


@functools.lru_cache(maxsize=None)
def acos_set():
    """v for pp_cr_acos, |v| < 1."""
    rng = np.random.default_rng(20240503)
    n = 6000
    v = rng.uniform(-1, 1, n)
    i = np.arange(n)
    near = 1.0 - rng.uniform(0, 1e-9, n)
    v[i % 18 == 0] = near[i % 18 == 0]
    v[i % 18 == 9] = -near[i % 18 == 9]
    b1 = np.nextafter(1.0, 0.0)
    b2 = np.nextafter(b1, 0.0)
    named = [b1, b2, -b1, -b2, 0.0, -0.0, 0.5, -0.5, 5e-324, 1e-17, -1e-17, 2.0 ** -27, 1.0 - 2.0 ** -30, np.sqrt(0.5), np.sqrt(0.75),
             -(2.0 ** -27), -(1.0 - 2.0 ** -30), -np.sqrt(0.5), -np.sqrt(0.75)]
    out = np.concatenate([v, neighbours(named, 1)])
    out = pad_off_wave(out[np.abs(out) < 1.0])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def acos_ref():
    r = ref_acos(acos_set())
    r.setflags(write=False)
    return r


ACOS_GUARDS = np.array([1.0, -1.0, np.nextafter(1.0, 2.0), -np.nextafter(1.0, 2.0), 1.5, -2.0, 1e300, np.inf, -np.inf, np.nan])


# ----------------------------------------------------------------------------- mod2pi
def mod2pi_literal(t):
    """dubins.c's mod2pi: t - 2pi floor(t / 2pi), each operation rounded once."""
    t = np.asarray(t, dtype=np.float64)
    return t - TWO_PI * np.floor(t / TWO_PI)


def mod2pi_guard(t):
    """Does pp_mod2pi's lane ask for the true division?  (The product by 1/2pi is within 1e-9 of an integer.)"""
    t = np.asarray(t, dtype=np.float64)
    q = t * INV_TWO_PI
    fr = q - np.floor(q)
    return ~((fr > 1e-9) & (fr < 1.0 - 1e-9))


@functools.lru_cache(maxsize=None)
def mod2pi_set():
    """Arguments of pp_mod2pi, |t| < 1e5 + a little: the doubles around every kind of k 2pi, and uniform draws.  Returns (t, guard)."""
    rng = np.random.default_rng(20240504)
    ks = np.concatenate([np.arange(-2000, 2001), rng.integers(-15900, 15901, 20000)])
    mp = _mp()
    two_pi = 2 * mp.pi
    exact = np.array([nearest_double(two_pi * int(k)) for k in ks])
    product = ks.astype(np.float64) * TWO_PI
    named = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300])
    t = np.concatenate([neighbours(exact, 3), neighbours(product, 3), named, rng.uniform(-1e5, 1e5, 20000)])
    t = pad_off_wave(t)
    assert np.all(np.abs(t) < 1.0001e5)
    t.setflags(write=False)
    return t, mod2pi_guard(t)


# ----------------------------------------------------------------------------- small division
UDIV_X = 1 << 21


def udiv_divisors():
    """(1..64, 256 drawn from [65, 2^21), the powers of two up to 2^21)."""
    rng = np.random.default_rng(20240505)
    drawn = np.unique(rng.integers(65, UDIV_X, 256))
    while drawn.size < 256:
        drawn = np.unique(np.concatenate([drawn, rng.integers(65, UDIV_X, 256 - drawn.size)]))
    return np.arange(1, 65), drawn, 2 ** np.arange(0, 22)


# ----------------------------------------------------------------------------- grid cells
GRID_RES = [(0.1, Fraction(1, 10)), (0.3, Fraction(3, 10)), (0.5, Fraction(1, 2)), (1.0 / 3.0, Fraction(1, 3)), (0.7, Fraction(7, 10)),
            (1.0, Fraction(1)), (2.0, Fraction(2)), (1e-3, Fraction(1, 1000)), (37.5, Fraction(75, 2))]
GRID_SHAPES = [(1, 1), (7, 33), (33, 7), (300, 300), (3, 2048)]


def checkerboard(rows, cols):
    r, c = np.indices((rows, cols))
    return ((r + c) & 1).astype(np.uint8)


def _u32_sat(v):
    """double -> unsigned as the device converts: truncated, negative and NaN to 0, too large to 2^32 - 1"""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 0.0, np.clip(np.trunc(v), 0.0, 4294967295.0)).astype(np.uint64)


def grid_guard(res, x, y):
    """Does pp_is_blocked's / pp_blocked_cell's lane ask for the true divisions?  (4e-9 either way changes the truncated product.)"""
    inv = 1.0 / res if res > 0 else 0.0
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    cx, cy = x * inv, y * inv
    lo, hi = 1.0 - 4e-9, 1.0 + 4e-9
    return (_u32_sat(cx * lo) != _u32_sat(cx * hi)) | (_u32_sat(cy * lo) != _u32_sat(cy * hi))


def grid_literal(res, rows, cols, x, y):
    """GridWorldMap::isBlocked's own arithmetic: (outside, row, col); row and col are 0 where outside (size_t of such a quotient is
    not defined)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(over="ignore"):
        qx, qy = x / res, y / res
    outside = (x < 0) | (qx >= float(cols)) | (y < 0) | (qy >= float(rows))
    row = np.where(outside, 0, np.where(outside, 0.0, qy)).astype(np.int64)
    col = np.where(outside, 0, np.where(outside, 0.0, qx)).astype(np.int64)
    return outside, row, col


def _axis_boundaries(res, res_exact, ncell):
    k = np.arange(0, ncell + 2)
    inv = 1.0 / res
    exact = np.array([float(res_exact * int(i)) for i in k])
    edge = np.concatenate([k * res, k / inv, exact, [float(ncell) * res]])
    named = np.array([0.0, -0.0, -5e-324, 5e-324, 1e12, 1e300, -1e300, 4294967296.0 * res])
    return np.concatenate([neighbours(edge, 2), named])


def _axis_ordinary(rng, res, ncell, n):
    return (rng.integers(0, ncell, n) + rng.uniform(0.2, 0.8, n)) * res


def grid_points(res, res_exact, rows, cols, seed):
    """(x, y) for one grid: boundary x with ordinary y, ordinary x with boundary y, both boundary, and ordinary pairs."""
    rng = np.random.default_rng(seed)
    bx, by = _axis_boundaries(res, res_exact, cols), _axis_boundaries(res, res_exact, rows)
    both = max(bx.size, by.size)
    n_ord = 1500
    x = np.concatenate([bx, _axis_ordinary(rng, res, cols, by.size), np.resize(bx, both), _axis_ordinary(rng, res, cols, n_ord)])
    y = np.concatenate([_axis_ordinary(rng, res, rows, bx.size), by, rng.permutation(np.resize(by, both)), _axis_ordinary(rng, res, rows, n_ord)])
    return pad_off_wave(x, y)


def grid_cases(res_index):
    """Every (rows, cols, cells, x, y) of one resolution."""
    res, res_exact = GRID_RES[res_index]
    out = []
    for j, (rows, cols) in enumerate(GRID_SHAPES):
        x, y = grid_points(res, res_exact, rows, cols, 20240600 + 16 * res_index + j)
        out.append((rows, cols, checkerboard(rows, cols), x, y))
    return res, out


# ----------------------------------------------------------------------------- line distance
def line_distance_literal(num, sqL, lim):
    """Ribbon::distance(...) < lim, literally"""
    with np.errstate(all="ignore"):
        return (np.abs(num) / np.sqrt(sqL)) < lim


def line_distance_guard(num, sqL, lim):
    """Does pp_line_distance_lt's lane evaluate the literal expression?"""
    with np.errstate(all="ignore"):
        A = num * num
        C = (lim * lim) * sqL
        return ~((A < C * (1.0 - 1e-11)) | (A > C * (1.0 + 1e-11)))


@functools.lru_cache(maxsize=None)
def line_distance_set():
    """(num, sqL, lim)"""
    rng = np.random.default_rng(20240507)
    sqL = np.concatenate([rng.uniform(1e-6, 1e4, 4000), 10.0 ** rng.uniform(-300, 300, 2000)])
    fixed = np.array([0.75, 1.0, 2.0, 1e-5, 0.3])
    lim = np.concatenate([np.resize(fixed, sqL.size), 10.0 ** rng.uniform(-150, 150, sqL.size)])
    sqL = np.concatenate([sqL, sqL])
    with np.errstate(all="ignore"):
        edge = lim * np.sqrt(sqL)
        per = 9 + 6
        num = np.concatenate([neighbours(edge, 4).reshape(-1, 9),
                              np.stack([edge * 0.5, edge * 2.0, edge * (1 - 1e-6), edge * (1 + 1e-6), edge * (1 - 3e-12), edge * (1 + 3e-12)], axis=1)],
                             axis=1)
    num = np.concatenate([num, -num], axis=1).reshape(-1)
    sqL = np.repeat(sqL, 2 * per)
    lim = np.repeat(lim, 2 * per)
    inf, nan = np.inf, np.nan
    deg = np.array([
        # num, sqL, lim
        (0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (-1.0, 0.0, 0.75), (1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 4.0, 1.0), (nan, 1.0, 1.0), (inf, 1.0, 1.0),
        (-inf, 1.0, 1.0), (1.0, nan, 1.0), (1.0, inf, 1.0), (1.0, 1.0, inf), (1.0, 1.0, nan), (1e200, 1e-300, 1.0), (1e200, 1e300, 1e60),
        (1e-200, 1e300, 1e-300), (1e-200, 1e-300, 1e-50), (1e-170, 1e-30, 1e-155), (1e160, 1e300, 1e10), (1e160, 1e300, 1e11),
        (5e-324, 1.0, 5e-324), (5e-324, 1.0, 1e-323), (1e-323, 1.0, 5e-324), (1e154, 1.0, 1e154), (1.4e154, 1.0, 1.3e154), (1.3e154, 1.0, 1.4e154),
        (1e-162, 1.0, 1.1e-162), (1.1e-162, 1.0, 1e-162), (1e-162, 1e-4, 1e-160), (1.01e-162, 1e-4, 1e-160), (0.99e-162, 1e-4, 1e-160),
    ])
    num, sqL, lim = (np.concatenate([a, deg[:, j]]) for j, a in enumerate((num, sqL, lim)))
    num, sqL, lim = pad_off_wave(num, sqL, lim)
    for a in (num, sqL, lim):
        a.setflags(write=False)
    return num, sqL, lim


# ----------------------------------------------------------------------------- dynamic obstacles
def obstacle_hit_literal(ob, x, y, t):
    """BinaryDynamicObstaclesManager::collisionExists(x, y, t, strict) for one obstacle per point, operation by operation, on PPObst rows
    (cos / sin of the yaw and the strict half sizes already taken, as ppgpu_set_obstacles does)."""
    X0, Y0, cosYaw, sinYaw, Speed, Time, halfL, halfW = (ob[:, j] for j in range(8))
    with np.errstate(all="ignore"):
        dt = t - Time
        dx = Speed * dt * cosYaw
        dy = Speed * dt * sinYaw
        X = X0 + dx
        Y = Y0 + dy
        tx = x - X
        ty = y - Y
        rx = tx * cosYaw - ty * sinYaw
        ry = tx * sinYaw + ty * cosYaw
        return ((np.abs(rx) < halfL) & (np.abs(ry) < halfW)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def obstacle_set():
    """(PPObst rows n x 12, x, y, t, expected) — expected is -1 where only the literal restatement says what must come out."""
    rng = np.random.default_rng(20240508)
    rows, xs, ys, ts, exp = [], [], [], [], []

    def add(X, Y, c, s, speed, time, hl, hw, x, y, t, e=-1):
        rows.append([X, Y, c, s, speed, time, hl, hw, np.hypot(hl, hw) * 1.0000001, 0.0, 0.0, 0.0])
        xs.append(x), ys.append(y), ts.append(t), exp.append(e)

    # at rest, axis aligned, centred on the origin: |rx| is the point's own |x|
    for hl, hw in [(6.0, 3.5), (1.5, 1.25), (0.1 + 1.0, 0.3 + 1.0), (26.0, 6.0), (1e-3 + 1, 1.0)]:
        for sgn in (1.0, -1.0):
            for t in (0.0, 17.25):
                below_l, below_w = np.nextafter(hl, 0.0), np.nextafter(hw, 0.0)
                add(0, 0, 1, 0, 0, 3.0, hl, hw, sgn * hl, 0.0, t, 0)                     # exactly the half length: strict, no hit
                add(0, 0, 1, 0, 0, 3.0, hl, hw, sgn * below_l, 0.0, t, 1)
                add(0, 0, 1, 0, 0, 3.0, hl, hw, sgn * np.nextafter(hl, np.inf), 0.0, t, 0)
                add(0, 0, 1, 0, 0, 3.0, hl, hw, 0.0, sgn * hw, t, 0)
                add(0, 0, 1, 0, 0, 3.0, hl, hw, 0.0, sgn * below_w, t, 1)
                add(0, 0, 1, 0, 0, 3.0, hl, hw, 0.0, sgn * np.nextafter(hw, np.inf), t, 0)
                add(0, 0, 1, 0, 0, 3.0, hl, hw, sgn * below_l, -sgn * below_w, t, 1)     # the corner, just inside
                add(0, 0, 1, 0, 0, 3.0, hl, hw, sgn * below_l, sgn * hw, t, 0)
                # the same box away from the origin, at coordinates for which the translation is exact
                add(64.0, -32.0, 1, 0, 0, 3.0, hl, hw, 64.0 + sgn * hl, -32.0, t, 0 if 64.0 + sgn * hl - 64.0 == sgn * hl else -1)
    # moving and rotated: points placed around the box's edges in its own frame, then whatever the arithmetic makes of them
    n = 4000
    yaw = rng.uniform(-np.pi, np.pi, n)
    c, s = np.cos(yaw), np.sin(yaw)
    speed = rng.uniform(-12, 12, n)
    time = rng.uniform(0, 100, n)
    t = time + rng.uniform(-50, 200, n)
    X0, Y0 = rng.uniform(-500, 500, n), rng.uniform(-500, 500, n)
    hl, hw = rng.uniform(1.0, 30.0, n), rng.uniform(1.0, 8.0, n)
    eps = np.resize(np.array([0.0, 1e-16, -1e-16, 1e-15, -1e-15, 1e-12, -1e-12, 1e-3, -1e-3, 0.3, -0.3, -0.9]), n)
    on_l = rng.integers(0, 2, n) == 0
    u = np.where(on_l, hl * (1 + eps), hl * rng.uniform(-1.2, 1.2, n)) * rng.choice([-1.0, 1.0], n)
    v = np.where(on_l, hw * rng.uniform(-1.2, 1.2, n), hw * (1 + eps)) * rng.choice([-1.0, 1.0], n)
    dt = t - time
    cx, cy = X0 + speed * dt * c, Y0 + speed * dt * s
    px, py = cx + (u * c + v * s), cy + (-u * s + v * c)          # inverse of the rotation by +yaw
    for i in range(n):
        add(X0[i], Y0[i], c[i], s[i], speed[i], time[i], hl[i], hw[i], px[i], py[i], t[i])
    # an obstacle a million metres from where it was reported
    add(10.0, 20.0, np.cos(0.3), np.sin(0.3), 1e3, 0.0, 6.0, 3.5, 10.0 + 1e6 * np.cos(0.3), 20.0 + 1e6 * np.sin(0.3), 1e3)
    add(10.0, 20.0, np.cos(0.3), np.sin(0.3), 1e3, 0.0, 6.0, 3.5, 10.0 + 1e6 * np.cos(0.3) + 7.0, 20.0 + 1e6 * np.sin(0.3), 1e3)
    add(10.0, 20.0, np.cos(0.3), np.sin(0.3), 1e3, 0.0, 6.0, 3.5, 10.0, 20.0, 1e3)
    ob = np.array(rows, dtype=np.float64)
    x, y, t_, e = np.array(xs, dtype=np.float64), np.array(ys, dtype=np.float64), np.array(ts, dtype=np.float64), np.array(exp, dtype=np.int32)
    ob, x, y, t_, e = pad_off_wave(ob, x, y, t_, e)
    return ob, x, y, t_, e
