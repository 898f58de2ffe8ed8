"""-m gpu: the small device functions of path_planner_amd/csrc/pp_device.h and pp_cr.h, each alone (tests/probe/pp_device_probe.hip),
against a plain high-precision reference: mpmath for sin / cos / atan2 / acos, numpy float64 for the reference's literal expressions,
the oracle's World.is_blocked for grid cells.  The inputs (tests/probe_inputs.py) sit on the boundaries the shortcuts exist for — cell
edges, multiples of 2pi and pi/2, a ribbon's knife edge — which a random world almost never produces.

Every probe runs in two launch orders (guarded lanes in every wave / unguarded lanes in waves of their own): the shortcuts are chosen
per wave by __ballot, so an element's bytes must not depend on its neighbours."""
import numpy as np
import pytest

import device_probe as dp
import probe_inputs as pi

pytestmark = pytest.mark.gpu


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = a.dtype.itemsize
    return np.nonzero((a.view(np.uint8).reshape(-1, w) != b.view(np.uint8).reshape(-1, w)).any(axis=1))[0]


def both_orders(fn, arrays, guard=None, what="", solitary=0):
    """fn(*arrays) evaluated in the mixed and in the separated order of `guard` (a fixed pseudo-random labelling for a function without
    a shortcut); asserts that every element gives the same bytes in both, returns the results in the arrays' own order.
    solitary = s: a third launch in which every s-th guarded element is the only guarded lane of its wave — in the other two orders a
    lane that only just asks for the guarded route shares its wave with lanes that ask for it anyway."""
    arrays = [np.asarray(a) for a in arrays]
    n = len(arrays[0])
    if guard is None:
        guard = np.random.default_rng(7).integers(0, 4, n) == 0
    mixed, separated = pi.orders(guard)
    outs = []
    for order in (mixed, separated):
        r = fn(*[a[order] for a in arrays])
        r = r if isinstance(r, tuple) else (r,)
        back = []
        for v in r:
            o = np.empty_like(v)
            o[order] = v
            back.append(o)
        outs.append(back)
    for j, (a, b) in enumerate(zip(*outs)):
        bad = _differing(a, b)
        assert bad.size == 0, (f"{what}: output {j} of {bad.size} elements depends on the launch order, first at index {bad[0]}: "
                               f"inputs {[x[bad[0]] for x in arrays]} mixed {a[bad[0]]!r} separated {b[bad[0]]!r}")
    if solitary:
        index, lanes = pi.solitary_order(guard, solitary)
        r = fn(*[a[index] for a in arrays])
        for j, v in enumerate(r if isinstance(r, tuple) else (r,)):
            bad = _differing(v[lanes], outs[0][j][index[lanes]])
            assert bad.size == 0, (f"{what}: output {j} of {bad.size} guarded elements changes when the element is alone in its wave, first "
                                   f"{[x[index[lanes[bad[0]]]] for x in arrays]}: {v[lanes[bad[0]]]!r} / {outs[0][j][index[lanes[bad[0]]]]!r}")
    return outs[0] if len(outs[0]) > 1 else outs[0][0]


def _routes_hold(guard, what):
    """at least 1 000 elements whose wave takes the guarded route, and 1 000 whose wave does not: no test passes vacuously"""
    guarded, unguarded = pi.route_counts(guard)
    print(f"{what}: {guarded} elements on the guarded route (mixed order), {unguarded} on the fast route (separated order)")
    assert guarded >= 1000 and unguarded >= 1000, (what, guarded, unguarded)


def _worst(err, x, what):
    i = int(np.argmax(err))
    line = f"{what}: worst error {err[i]:.4f} ulp at x = {x[i]!r} ({float(x[i]).hex()})"
    print(line)
    return line


# ----------------------------------------------------------------------------- pp_sincos_bounded / pp_sincos
@pytest.fixture(scope="module")
def bounded():
    """pp_sincos_bounded<false> on its set, both orders: (x, sin, cos)"""
    x = pi.sincos_bounded_set()
    s, c = both_orders(lambda v: dp.sincos_bounded(v), [x], what="pp_sincos_bounded<false>")
    return x, s, c


def test_sincos_bounded_is_within_one_ulp(bounded):
    """The header's promise: error below 1 ulp of the exact value, for sin and for cos (CPU restatement: 0.81 / 0.82 ulp)."""
    x, s, c = bounded
    ref = pi.sincos_bounded_ref()
    es, ec = pi.ulp_error(s, ref[0], ref[1]), pi.ulp_error(c, ref[2], ref[3])
    _worst(es, x, "pp_sincos_bounded sin")
    _worst(ec, x, "pp_sincos_bounded cos")
    assert es.max() < 1.0 and ec.max() < 1.0


def test_sincos_bounded_table_instantiation_gives_the_same_bytes(bounded):
    x, s, c = bounded
    st, ct = both_orders(lambda v: dp.sincos_bounded(v, tab=True), [x], what="pp_sincos_bounded<true>")
    assert _same_bytes(st, s) and _same_bytes(ct, c), (_differing(st, s)[:5], _differing(ct, c)[:5])


def test_sincos_routes(bounded):
    """pp_sincos: a wave whose every |x| < 1e5 runs pp_sincos_bounded; one lane at 1e5 or beyond (or not finite) sends the whole wave to
    the library, which only has to be sane (1e-12 absolute: a wrong quadrant, not an ulp)."""
    xb, sb, cb = bounded
    x, guard = pi.sincos_route_set()
    _routes_hold(guard, "pp_sincos")
    mixed, separated = pi.orders(guard)
    assert pi.wave_routes(guard[mixed]).all(), "the mixed order must put a library lane into every wave"
    # separated: waves of bounded arguments only -> the bytes of pp_sincos_bounded<false>
    s_sep, c_sep = dp.sincos(x[separated])
    fast = ~pi.wave_routes(guard[separated])
    idx = separated[fast]
    assert np.all(idx < xb.size) and fast.sum() >= xb.size - pi.WAVE
    assert _same_bytes(s_sep[fast], sb[idx]) and _same_bytes(c_sep[fast], cb[idx])
    # mixed: every wave on the library's route
    s_mix, c_mix = dp.sincos(x[mixed])
    s_lib, c_lib = np.empty_like(s_mix), np.empty_like(c_mix)
    s_lib[mixed], c_lib[mixed] = s_mix, c_mix
    ref = pi.sincos_bounded_ref()
    n = xb.size
    assert np.abs((s_lib[:n] - ref[0]) - ref[1]).max() <= 1e-12 and np.abs((c_lib[:n] - ref[2]) - ref[3]).max() <= 1e-12
    fin = np.isfinite(x) & guard
    far = np.unique(x[fin])
    rf = pi.ref_sincos(far)
    pos = np.searchsorted(far, x[fin])
    assert np.abs(s_lib[fin] - rf[0][pos]).max() <= 1e-12 and np.abs(c_lib[fin] - rf[2][pos]).max() <= 1e-12
    assert np.isnan(s_lib[~np.isfinite(x)]).all() and np.isnan(c_lib[~np.isfinite(x)]).all()
    changed = int(((s_lib[:n] != sb) | (c_lib[:n] != cb)).sum())
    print(f"pp_sincos: {changed} of {n} bounded arguments change bits between pp_sincos_bounded and the library route")


# ----------------------------------------------------------------------------- pp_cr_*
@pytest.mark.parametrize("chunk", range(pi.CR_CHUNKS))
def test_cr_sincos_is_correctly_rounded(chunk):
    x = pi.cr_sincos_chunk(chunk)
    s, c = both_orders(dp.cr_sincos, [x], what="pp_cr_sincos")
    ref = pi.cr_sincos_chunk_ref(chunk)
    bad_s, bad_c = np.nonzero(s != ref[0])[0], np.nonzero(c != ref[2])[0]
    print(f"pp_cr_sincos chunk {chunk}: {x.size} arguments, not correctly rounded: sin {bad_s.size}, cos {bad_c.size}")
    assert bad_s.size == 0, [(float(x[i]).hex(), s[i], ref[0][i]) for i in bad_s[:5]]
    assert bad_c.size == 0, [(float(x[i]).hex(), c[i], ref[2][i]) for i in bad_c[:5]]


def test_cr_sincos_beyond_its_range_is_sane():
    x = pi.pad_off_wave(np.resize(pi.CR_SINCOS_BEYOND, 129))
    s, c = both_orders(dp.cr_sincos, [x], what="pp_cr_sincos (library route)")
    ref = pi.ref_sincos(pi.CR_SINCOS_BEYOND)
    k = np.arange(x.size) % pi.CR_SINCOS_BEYOND.size
    assert np.abs(s - ref[0][k]).max() <= 1e-12 and np.abs(c - ref[2][k]).max() <= 1e-12
    xs = np.array([np.inf, -np.inf, np.nan])
    s, c = dp.cr_sincos(xs)
    assert np.isnan(s).all() and np.isnan(c).all()


def test_cr_atan2_is_correctly_rounded():
    y, x = pi.atan2_set()
    t = both_orders(dp.cr_atan2, [y, x], what="pp_cr_atan2")
    ref = pi.atan2_ref()
    bad = np.nonzero(t != ref[0])[0]
    print(f"pp_cr_atan2: {x.size} arguments, not correctly rounded: {bad.size}")
    assert bad.size == 0, [(float(y[i]).hex(), float(x[i]).hex(), t[i], ref[0][i]) for i in bad[:5]]


def test_cr_atan2_guards_are_numpys_bits():
    y, x = pi.atan2_guard_set()
    t = both_orders(dp.cr_atan2, [y, x], what="pp_cr_atan2 (guards)")
    exp = np.arctan2(y, x)
    bad = _differing(t, exp)
    assert bad.size == 0, [(y[i], x[i], t[i], exp[i]) for i in bad[:8]]


def test_cr_acos_is_correctly_rounded():
    v = pi.acos_set()
    t = both_orders(dp.cr_acos, [v], what="pp_cr_acos")
    ref = pi.acos_ref()
    bad = np.nonzero(t != ref[0])[0]
    print(f"pp_cr_acos: {v.size} arguments, not correctly rounded: {bad.size}")
    assert bad.size == 0, [(float(v[i]).hex(), t[i], ref[0][i]) for i in bad[:5]]


def test_cr_acos_guards():
    v = pi.pad_off_wave(np.resize(pi.ACOS_GUARDS, 130))
    t = both_orders(dp.cr_acos, [v], what="pp_cr_acos (guards)")
    assert np.all(t[v == 1.0] == 0.0) and not np.signbit(t[v == 1.0]).any()
    assert _same_bytes(t[v == -1.0], np.full((v == -1.0).sum(), np.pi))
    out = ~(np.abs(v) <= 1.0)
    assert out.sum() >= 80 and np.isnan(t[out]).all()


# ----------------------------------------------------------------------------- pp_mod2pi
def test_mod2pi_is_the_literal_expression():
    t, guard = pi.mod2pi_set()
    _routes_hold(guard, "pp_mod2pi")
    assert pi.wave_routes(guard[pi.orders(guard)[0]]).all()
    got = both_orders(dp.mod2pi, [t], guard, what="pp_mod2pi", solitary=16)
    exp = pi.mod2pi_literal(t)
    bad = _differing(got, exp)
    assert bad.size == 0, (bad.size, [(float(t[i]).hex(), got[i], exp[i]) for i in bad[:5]])


# ----------------------------------------------------------------------------- pp_udiv_small
def _udiv_all_x(divisors):
    x = np.arange(pi.UDIV_X, dtype=np.uint32)
    # x = k d - 1, k d, k d + 1 for every k are all among 0 .. 2^21 - 1; the launch also carries a partial last wave
    xs = np.concatenate([x, x[:37]])
    for d in divisors:
        got = dp.udiv_small(xs, np.uint32(d))
        exp = xs // np.uint32(d)
        if not np.array_equal(got, exp):
            i = int(np.nonzero(got != exp)[0][0])
            raise AssertionError(f"pp_udiv_small({xs[i]}, {d}) = {got[i]}, x // d = {exp[i]}; {(got != exp).sum()} wrong for this d")


def test_udiv_small_divisors_to_64():
    _udiv_all_x(pi.udiv_divisors()[0])


def test_udiv_small_drawn_divisors_first_half():
    _udiv_all_x(pi.udiv_divisors()[1][:128])


def test_udiv_small_drawn_divisors_second_half():
    _udiv_all_x(pi.udiv_divisors()[1][128:])


def test_udiv_small_powers_of_two_and_order():
    _udiv_all_x(pi.udiv_divisors()[2])
    rng = np.random.default_rng(11)
    x = rng.integers(0, pi.UDIV_X, 100001).astype(np.uint32)
    d = rng.integers(1, pi.UDIV_X, 100001).astype(np.uint32)
    got = both_orders(dp.udiv_small, [x, d], what="pp_udiv_small")
    assert np.array_equal(got, x // d)


# ----------------------------------------------------------------------------- grid cells
@pytest.mark.parametrize("res_index", range(len(pi.GRID_RES)))
def test_grid_cells_match_the_oracle_and_the_literal_expression(res_index):
    """Checkerboard grids: a cell off by one in either axis flips the answer.  pp_is_blocked and pp_blocked_cell + pp_blocked_test
    against the oracle's isBlocked; pp_blocked_cell's (outside, row, col) against the reference's own arithmetic in numpy."""
    import oracle as orc
    res, cases = pi.grid_cases(res_index)
    guarded = unguarded = 0
    for rows, cols, cells, x, y in cases:
        guard = pi.grid_guard(res, x, y)
        g, u = pi.route_counts(guard)
        guarded, unguarded = guarded + g, unguarded + u
        what = f"res {res} grid {rows} x {cols}"
        exp = orc.World(orc.PpgpuConfig(), cells, res).is_blocked(x, y)
        got = both_orders(lambda a, b: dp.is_blocked(cells, res, a, b), [x, y], guard, what="pp_is_blocked " + what, solitary=8)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (what, bad.size, [(float(x[i]).hex(), float(y[i]).hex(), got[i], exp[i]) for i in bad[:5]])
        outside, row, col, blocked = both_orders(lambda a, b: dp.blocked_cell(cells, res, a, b), [x, y], guard, what="pp_blocked_cell " + what, solitary=8)
        bad = np.nonzero(blocked != exp)[0]
        assert bad.size == 0, (what, bad.size, [(float(x[i]).hex(), float(y[i]).hex(), blocked[i], exp[i]) for i in bad[:5]])
        e_out, e_row, e_col = pi.grid_literal(res, rows, cols, x, y)
        assert np.array_equal(outside != 0, e_out), (what, np.nonzero((outside != 0) != e_out)[0][:5])
        inside = ~e_out
        assert np.array_equal(row[inside], e_row[inside]) and np.array_equal(col[inside], e_col[inside]), what
        assert np.all(row[e_out] == 0)                               # a lane outside the grid reads word 0
    print(f"grid res {res}: {guarded} elements on the guarded route, {unguarded} on the fast route")
    assert guarded >= 1000 and unguarded >= 1000


def test_empty_grid_blocks_nothing():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-10, 10, 190), [0.0, -0.0, -1.0, 1e300, -1e300]])
    y = rng.permutation(x)
    cells = np.zeros((0, 0), dtype=np.uint8)
    for res in (0.0, 1.0):
        assert not both_orders(lambda a, b: dp.is_blocked(cells, res, a, b), [x, y], what="pp_is_blocked (no grid)").any()


# ----------------------------------------------------------------------------- pp_line_distance_lt
def test_line_distance_lt_is_the_literal_expression():
    num, sqL, lim = pi.line_distance_set()
    guard = pi.line_distance_guard(num, sqL, lim)
    print(f"pp_line_distance_lt: {guard.sum()} of {guard.size} elements inside the margin")
    assert guard.sum() >= 1000 and (~guard).sum() >= 1000
    got = both_orders(dp.line_distance_lt, [num, sqL, lim], guard, what="pp_line_distance_lt")
    exp = pi.line_distance_literal(num, sqL, lim)
    bad = np.nonzero((got != 0) != exp)[0]
    assert bad.size == 0, (bad.size, [(float(num[i]).hex(), float(sqL[i]).hex(), float(lim[i]).hex(), got[i], exp[i]) for i in bad[:5]])


# ----------------------------------------------------------------------------- pp_obstacle_hit
def test_obstacle_hit_is_the_literal_expression():
    ob, x, y, t, expected = pi.obstacle_set()
    got = both_orders(dp.obstacle_hit, [ob, x, y, t], what="pp_obstacle_hit")
    exp = pi.obstacle_hit_literal(ob, x, y, t)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (bad.size, [(ob[i].tolist(), x[i], y[i], t[i], got[i], exp[i]) for i in bad[:3]])
    known = expected >= 0
    assert known.sum() >= 150 and np.array_equal(got[known], expected[known])
    assert 200 < got.sum() < got.size - 200                          # both answers occur
