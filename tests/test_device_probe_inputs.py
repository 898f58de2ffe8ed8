"""CPU: the input sets of tests/test_gpu_device_math.py (tests/probe_inputs.py) are deterministic and reach both routes of every shortcut;
the host build of pp_cr.h is correctly rounded on the very sets the device is asked about (so a failure there points at the device);
the mpmath references agree with numpy where numpy is exact; and the per-lane restatement of each guarded shortcut in numpy gives the
literal expression's answer on its set."""
import os
import subprocess

import numpy as np
import pytest

import probe_inputs as pi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the sets
def _bytes(v):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (v if isinstance(v, tuple) else (v,)))


@pytest.mark.parametrize("make", [pi.sincos_bounded_set, pi.sincos_route_set, pi.cr_sincos_set, pi.atan2_set, pi.acos_set, pi.mod2pi_set,
                                  pi.line_distance_set, pi.obstacle_set], ids=lambda f: f.__name__)
def test_sets_are_deterministic_and_leave_a_partial_wave(make):
    a, b = make.__wrapped__(), make.__wrapped__()
    assert _bytes(a) == _bytes(b)
    first = a[0] if isinstance(a, tuple) else a
    assert len(first) % pi.WAVE != 0 and len(first) > 2 * pi.WAVE


def test_grid_sets_are_deterministic():
    (_, a), (_, b) = pi.grid_cases(3), pi.grid_cases(3)
    for (r0, c0, g0, x0, y0), (r1, c1, g1, x1, y1) in zip(a, b):
        assert (r0, c0) == (r1, c1) and _bytes((g0, x0, y0)) == _bytes((g1, x1, y1)) and x0.size % pi.WAVE != 0
        assert not np.isnan(x0).any() and not np.isnan(y0).any()      # the reference's size_t(NaN) is undefined


def test_orders_are_permutations_that_separate_and_mix():
    guard = np.zeros(64 * 50 + 17, dtype=bool)
    guard[::9] = True
    mixed, separated = pi.orders(guard)
    n = guard.size
    assert np.array_equal(np.sort(mixed), np.arange(n)) and np.array_equal(np.sort(separated), np.arange(n))
    assert pi.wave_routes(guard[mixed]).all()
    fast = ~pi.wave_routes(guard[separated])
    assert fast.sum() >= (~guard).sum() - pi.WAVE and not guard[separated][fast].any()


def test_every_shortcut_set_reaches_both_routes():
    counts = {"pp_sincos": pi.route_counts(pi.sincos_route_set()[1]), "pp_mod2pi": pi.route_counts(pi.mod2pi_set()[1])}
    for i in range(len(pi.GRID_RES)):
        res, cases = pi.grid_cases(i)
        per = [pi.route_counts(pi.grid_guard(res, x, y)) for _, _, _, x, y in cases]
        counts[f"grid res {res}"] = (sum(p[0] for p in per), sum(p[1] for p in per))
    num, sqL, lim = pi.line_distance_set()
    g = pi.line_distance_guard(num, sqL, lim)
    counts["pp_line_distance_lt (per lane)"] = (int(g.sum()), int((~g).sum()))
    print(counts)
    for what, (guarded, unguarded) in counts.items():
        assert guarded >= 1000 and unguarded >= 1000, (what, guarded, unguarded)
    for guard in (pi.sincos_route_set()[1], pi.mod2pi_set()[1]):
        assert pi.wave_routes(guard[pi.orders(guard)[0]]).all()


def test_solitary_order_leaves_one_guarded_lane_per_wave():
    t, guard = pi.mod2pi_set()
    index, lanes = pi.solitary_order(guard, 16)
    g = guard[index]
    assert index.size % pi.WAVE != 0 and g[lanes].all() and g.sum() == lanes.size >= 20000
    assert (g[: lanes.size * pi.WAVE].reshape(-1, pi.WAVE).sum(axis=1) == 1).all()
    # ... among them lanes that only just ask for the division, and for which it matters
    q = t[index[lanes]] * pi.INV_TWO_PI
    matters = (np.floor(q) != np.floor(t[index[lanes]] / pi.TWO_PI)) & (q != np.floor(q))
    assert matters.sum() >= 100


# ----------------------------------------------------------------------------- the shortcuts, restated lane by lane
def test_mod2pi_shortcut_restated_gives_the_literal_expression():
    t, guard = pi.mod2pi_set()
    fast = t - pi.TWO_PI * np.floor(t * pi.INV_TWO_PI)
    exp = pi.mod2pi_literal(t)
    assert np.array_equal(np.where(guard, exp, fast).view(np.uint64), exp.view(np.uint64))
    assert guard.sum() > 300000                                        # the set is made of boundaries


def test_grid_shortcut_restated_gives_the_literal_cell():
    for i in range(len(pi.GRID_RES)):
        res, cases = pi.grid_cases(i)
        inv = 1.0 / res
        for rows, cols, cells, x, y in cases:
            guard = pi.grid_guard(res, x, y)
            cxl, cyl = pi._u32_sat(x * inv * (1.0 - 4e-9)), pi._u32_sat(y * inv * (1.0 - 4e-9))
            f_out = (x < 0) | (cxl >= cols) | (y < 0) | (cyl >= rows)
            e_out, e_row, e_col = pi.grid_literal(res, rows, cols, x, y)
            ok = guard | ((f_out == e_out) & (e_out | ((cyl == e_row) & (cxl == e_col))))
            assert ok.all(), (res, rows, cols, x[~ok][:4], y[~ok][:4])


def test_line_distance_shortcut_restated_gives_the_literal_expression():
    num, sqL, lim = pi.line_distance_set()
    with np.errstate(all="ignore"):
        A, C = num * num, (lim * lim) * sqL
        fast = np.where(A < C * (1.0 - 1e-11), True, False)
    guard = pi.line_distance_guard(num, sqL, lim)
    exp = pi.line_distance_literal(num, sqL, lim)
    bad = np.nonzero(~guard & (fast != exp))[0]
    assert bad.size == 0, [(num[i], sqL[i], lim[i]) for i in bad[:5]]


def test_obstacle_set_knows_its_edges():
    ob, x, y, t, expected = pi.obstacle_set()
    exp = pi.obstacle_hit_literal(ob, x, y, t)
    known = expected >= 0
    assert known.sum() >= 150 and np.array_equal(exp[known], expected[known])
    assert 200 < exp.sum() < exp.size - 200


# ----------------------------------------------------------------------------- references
def test_references_agree_with_numpy_where_numpy_is_exact():
    r = pi.ref_sincos(np.array([0.0, -0.0, 5e-324, 1e-300, -1e-300, 1e-8]))
    assert r[0].tolist() == [0.0, 0.0, 5e-324, 1e-300, -1e-300, 1e-8] and r[2].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, float(np.cos(1e-8))]
    y = np.array([1.0, -1.0, 1.0, -1.0, 5e-324, 1e308, 1e-310, 1e-305, 1e-200, 1e200, 1e-17])
    x = np.array([1.0, 1.0, -1.0, -1.0, 5e-324, 1e308, 1.0, 1e5, 1e-200, -1e200, 1.0])
    a = pi.ref_atan2(y, x)[0]
    exact = np.array([np.pi / 4, -np.pi / 4, 3 * np.pi / 4, -3 * np.pi / 4, np.pi / 4, np.pi / 4, 1e-310, 1e-310, np.pi / 4, 3 * np.pi / 4, 1e-17])
    assert a.tolist() == exact.tolist() and a.tolist() == np.arctan2(y, x).tolist()
    v = np.array([0.0, -0.0, 5e-324, 1e-17])
    assert pi.ref_acos(v)[0].tolist() == [np.pi / 2] * 4 == np.arccos(v).tolist()
    assert pi.nearest_double(pi._mp().mpf(2) ** -1074 * 1.5) == 1e-323 and pi.nearest_double(pi._mp().mpf(2) ** -1075) == 0.0   # ties to even


def test_ulp_error_measures_ulps():
    x = np.array([0.5, 1.0, 3.0, 1e-5, 100.0])
    r = pi.ref_sincos(x)
    assert pi.ulp_error(r[0], r[0], r[1]).max() <= 0.5
    e = pi.ulp_error(np.nextafter(r[0], np.inf), r[0], r[1])
    assert np.all((e >= 0.5) & (e <= 1.5))
    assert pi.ulp_error([1e-300], [0.0], [0.0])[0] == np.inf and pi.ulp_error([-0.0], [0.0], [0.0])[0] == 0.0
    assert pi.ulp_error([np.nan], [1.0], [0.0])[0] == np.inf


# ----------------------------------------------------------------------------- host pp_cr.h on the device's sets
@pytest.fixture(scope="module")
def cr_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cr") / "cr_trig_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cr_trig_check.cpp"), "-o", exe, "-lm"])

    def run(lines, per_line):
        out = subprocess.run([exe, "--stdin"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == per_line * len(lines)
        return np.array([float.fromhex(w) for w in out]).reshape(len(lines), per_line)
    return run


@pytest.mark.parametrize("chunk", range(pi.CR_CHUNKS))
def test_host_cr_sincos_is_correctly_rounded_on_the_device_set(cr_check, chunk):
    x = pi.cr_sincos_chunk(chunk)
    got = cr_check([f"s {v.hex()}" for v in x.tolist()], 2)
    ref = pi.cr_sincos_chunk_ref(chunk)
    assert np.array_equal(got[:, 0], ref[0]) and np.array_equal(got[:, 1], ref[2])


def test_host_cr_atan2_is_correctly_rounded_on_the_device_set(cr_check):
    y, x = pi.atan2_set()
    got = cr_check([f"t {a.hex()} {b.hex()}" for a, b in zip(y.tolist(), x.tolist())], 1)
    assert np.array_equal(got[:, 0], pi.atan2_ref()[0])


def test_host_cr_acos_is_correctly_rounded_on_the_device_set(cr_check):
    v = pi.acos_set()
    got = cr_check([f"a {a.hex()}" for a in v.tolist()], 1)
    assert np.array_equal(got[:, 0], pi.acos_ref()[0])
