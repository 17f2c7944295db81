"""The host's real-space table (build_realspace_table behind pse_host_realspace_table) and the oracle's radial functions against the
mpmath closed forms of tests/realspace_ref.py, at every xi the parameter rule admits in practice -- 0.05 .. 20 -- and on the CPU.

What the device reads is this table; what every other test compares the device with is this oracle.  Neither was ever held to anything
outside xi = 0.273 .. 0.8.  Two findings live here:
  * small xi: the Gauss-Legendre panels of the wave-part quadrature were sized by the oscillation alone.  At xi = 0.05 all of
    H(k) = (1 + k^2/4xi^2) exp(-k^2/4xi^2) fell into one panel; the table was off by 6.6e-10 and the oracle, which shares the rule for
    r < 0.25, by 5.1e-10 with the same sign.  Both now bound the panel by 4 xi as well (pse_params.cpp wave_fg, pse_oracle.c).
  * large xi: degree 9 on eighths cannot follow a function of scale 1 / xi.  format_eps, computed from the closed forms alone, is the
    price: below 2e-13 up to XI_TABLE = 4, 4.9e-13 at xi = 6, 2.1e-10 at 10, 2e-8 at 20.  The table reaches exactly that.
"""
import math

import numpy as np
import pytest

import realspace_ref as ref

XIS = (0.05, 0.08, 0.1, 0.2, 0.273, 0.5, 0.8, 1.0, 2.0, 3.0, 4.0, 6.0, 10.0, 20.0)
ERRORS = (1e-3, 1e-6)
CONTRACT = ref.CONTRACT   # |f - f_ref|, |g - g_ref| < 2e-13 of the device's table, as the GPU tests assert it (xi <= XI_TABLE)
CAP = 16                  # intervals looked at per case: 128 mpmath samples each
U = 2.0 ** -53


def rcut_of(xi, error):
    """The rule's cutoff sqrt(-ln error) / xi -- or 3 where that is below 2.5, so that the intervals either side of r = 2 are in."""
    rc = math.sqrt(-math.log(error)) / xi
    return rc if rc >= 2.5 else 3.0


def intervals_of(rcut):
    """At most CAP intervals of the table of rcut (realspace_ref.probe_intervals: the first three, those around r = 2, the last three
    and the rest spread)."""
    return ref.probe_intervals(rcut, CAP)


def points_of(k):
    """k/8 exactly, the double just below (k + 1)/8 and 16 points inside (interval 0 starts at 1e-6: r > 0)."""
    lo, hi = k / 8.0, (k + 1) / 8.0
    inner = lo + (np.arange(16) + 0.37) / 16.0 * 0.125
    return np.concatenate([[lo if k > 0 else 1e-6], inner, [np.nextafter(hi, 0.0)]])


def table_eval(coef, r):
    """eval_fg's operations restated (pse_amd/csrc/pse_device.h): s = 8 r, k = (int) s, t = 2 (s - k) - 1, Horner from the top, and
    the analytic branch f0, g0 minus the result.  Returns f_w, g_w, f, g, k."""
    r = np.asarray(r, float)
    s = r * 8.0
    k = s.astype(np.int64)
    t = 2.0 * (s - k) - 1.0
    c = coef[k]
    fw, gw = c[:, 0, 9].copy(), c[:, 1, 9].copy()
    for q in range(8, -1, -1):
        fw = fw * t + c[:, 0, q]
        gw = gw * t + c[:, 1, q]
    far = r > 2.0
    with np.errstate(divide="ignore"):
        ir = 1.0 / r
    f0 = np.where(far, 0.75 * ir + 0.5 * ir ** 3, 1.0 - 0.28125 * r)
    g0 = np.where(far, 1.5 * ir - ir ** 3, 1.0 - 0.1875 * r)
    return fw, gw, f0 - fw, g0 - gw, k


@pytest.fixture(scope="module")
def engine_mod():
    from pse_amd import build
    build.build_lib()
    import pse_amd
    return pse_amd


_CASES = {}


def case(xi, error):
    """Points, intervals and reference of one (xi, error), computed once: r, k, the mpmath f_w, g_w, f, g rounded to double."""
    key = (xi, error)
    if key not in _CASES:
        rcut = rcut_of(xi, error)
        ks = intervals_of(rcut)
        r = np.concatenate([points_of(k) for k in ks])
        fw, gw = ref.fg_wave(r, xi)
        f, g = ref.fg_real(r, xi)
        _CASES[key] = dict(rcut=rcut, ks=ks, r=r, k=np.repeat(ks, 18), fw=fw, gw=gw, f=f, g=g)
    return _CASES[key]


def test_the_entry_point_sizes_and_refuses(engine_mod):
    import ctypes
    from pse_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int(-1)
    assert lib.pse_host_realspace_table(0.5, 5.0, 0, None, ctypes.byref(n)) != 0 and n.value == 41
    assert b"null coef" in lib.pse_last_error()
    buf = np.zeros(41 * 20 + 1)
    buf[-1] = 123.0
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.pse_host_realspace_table(0.5, 5.0, 41 * 20 - 1, buf.ctypes.data_as(dp), ctypes.byref(n)) != 0 and b"cap" in lib.pse_last_error()
    assert not buf[:-1].any()
    assert lib.pse_host_realspace_table(0.5, 5.0, 41 * 20, buf.ctypes.data_as(dp), ctypes.byref(n)) == 0 and buf[-1] == 123.0 and buf[:-1].all()
    for xi, rcut in ((0.0, 5.0), (-1.0, 5.0), (float("nan"), 5.0), (0.5, 0.0), (0.5, float("nan")), (0.5, 2e5)):
        assert lib.pse_host_realspace_table(xi, rcut, 41 * 20, buf.ctypes.data_as(dp), ctypes.byref(n)) != 0
    assert lib.pse_host_realspace_table(0.5, 5.0, 0, None, None) != 0
    t = engine_mod.host_realspace_table(0.5, 5.0)
    assert t.shape == (41, 2, 10) and np.array_equal(t.ravel(), buf[:-1])
    assert engine_mod.host_realspace_table(0.5, 4.875).shape == (40, 2, 10)      # ceil(8 rcut) + 1: rcut on an interval's edge


@pytest.mark.parametrize("error", ERRORS)
@pytest.mark.parametrize("xi", XIS)
def test_host_table_is_within_the_format_of_the_closed_forms(engine_mod, xi, error):
    """The wave parts read from the host's table lie within the format's own error of the mpmath closed forms, interval by interval
    (interval_eps of the point's interval: at most format_eps), and f = f0 - f_w, g = g0 - g_w within that plus the rounding of the
    analytic branch: f0, g0 are three or four operations on values below 1.5 (4 u |f0|) and the subtraction rounds once (u |f|)."""
    c = case(xi, error)
    coef = engine_mod.host_realspace_table(xi, c["rcut"])
    assert len(coef) == ref.n_intervals(c["rcut"])
    fw, gw, f, g, k = table_eval(coef, c["r"])
    assert np.array_equal(k, c["k"])
    eps = np.array([ref.interval_eps(xi, int(q)) for q in c["k"]])
    whole = ref.format_eps(xi, c["rcut"], intervals=c["ks"])
    assert eps.max() == whole
    dfw, dgw = np.abs(fw - c["fw"]), np.abs(gw - c["gw"])
    i = int(np.argmax(np.maximum(dfw / eps[:, 0], dgw / eps[:, 1])))
    print(f"xi = {xi}, rcut = {c['rcut']:.3f} ({len(c['ks'])} of {len(coef)} intervals): table - closed form {max(dfw.max(), dgw.max()):.2e}, "
          f"format_eps {whole:.2e}; nearest to its interval's bound at r = {c['r'][i]:.6g}: {max(dfw[i] / eps[i, 0], dgw[i] / eps[i, 1]):.2f} of it")
    # (the reference was rounded to double: u |value| on top)
    assert np.all(dfw <= eps[:, 0] + U * np.abs(c["fw"])) and np.all(dgw <= eps[:, 1] + U * np.abs(c["gw"]))
    f0, g0 = f + fw, g + gw
    assert np.all(np.abs(f - c["f"]) <= eps[:, 0] + U * (4 * np.abs(f0) + 2 * np.abs(c["f"])))
    assert np.all(np.abs(g - c["g"]) <= eps[:, 1] + U * (4 * np.abs(g0) + 2 * np.abs(c["g"])))


def test_format_eps_decides_xi_table():
    """The contract of the GPU tests, |f - f_ref|, |g - g_ref| < 2e-13, is the format's own error up to a limit in xi and no further:
    XI_TABLE is the largest listed xi with format_eps < 2e-13 for it and every smaller one, from the closed forms alone.  The worst
    intervals are the first ones (the wave parts vary fastest at small r), which every case holds."""
    eps = {xi: max(ref.format_eps(xi, rcut_of(xi, e), intervals=intervals_of(rcut_of(xi, e))) for e in ERRORS) for xi in XIS}
    print("format_eps: " + ", ".join(f"xi = {xi:g}: {v:.2e}" for xi, v in eps.items()))
    ok = [xi for xi in XIS if all(eps[x] < CONTRACT for x in XIS if x <= xi)]
    # what the scan finds is what realspace_ref.XI_TABLE says -- and with it record_bound.table, the header comment of
    # pse_eval_realspace, README.md and DESIGN.md
    assert max(ok) == ref.XI_TABLE == 4.0
    assert all(eps[xi] >= CONTRACT for xi in XIS if xi > ref.XI_TABLE)
    # the margin of the contract at the limit, and what lies beyond it (DESIGN.md carries this table)
    assert eps[4.0] < 1e-13 and 4e-13 < eps[6.0] < 6e-13 and 1e-10 < eps[10.0] < 3e-10 and 1e-8 < eps[20.0] < 4e-8
    assert all(eps[xi] < 4e-15 for xi in XIS if xi <= 2.0)


@pytest.mark.parametrize("xi,rcut", [(0.5, 5.2565), (1.0, 3.0), (4.0, 3.0), (10.0, 3.0)])
def test_the_probed_intervals_hold_the_worst_one(xi, rcut):
    """format_eps over every interval of a table, as it is defined, equals format_eps over the intervals the capped tests look at: the
    worst interval is one of the first three (the rounding term follows sum |c_q|, largest at small r; the interpolation term follows
    the tenth derivative, largest at small r too)."""
    every = ref.format_eps(xi, rcut)
    assert every == ref.format_eps(xi, rcut, intervals=intervals_of(rcut)) == ref.format_eps(xi, rcut, intervals=(0, 1, 2))
    print(f"xi = {xi}, rcut = {rcut}: format_eps over all {ref.n_intervals(rcut)} intervals = {every:.3e}")


@pytest.mark.parametrize("xi", [0.05, 0.5, 4.0, 10.0])
def test_the_gpu_bound_passes_the_right_table_and_catches_a_wrong_one(engine_mod, xi):
    """A rehearsal of tests/test_gpu_realspace.py on the CPU: the restated evaluation of the host's table lies within the bound that
    file derives for the device (format_eps plus the rounding around the table), and a table read wrongly does not -- the intervals
    shifted by one, or the 20 doubles of an interval read with the stride 21 of the padded LDS copy.  (The device is never given a
    wrong table: what a wrong index would do is shown here.)"""
    from test_gpu_realspace import fg_bound
    c = case(xi, 1e-3)
    coef = engine_mod.host_realspace_table(xi, c["rcut"])
    eps = ref.format_eps(xi, c["rcut"], intervals=c["ks"])
    df, dg = fg_bound(c["r"], c["f"], c["g"], eps)
    flat = np.concatenate([coef.ravel(), np.zeros(len(coef))])
    wrong = {"shifted by one": np.roll(coef, 1, axis=0),
             "stride 21": np.stack([flat[21 * k:21 * k + 20] for k in range(len(coef))]).reshape(len(coef), 2, 10)}
    _, _, f, g, _ = table_eval(coef, c["r"])
    assert np.all(np.abs(f - c["f"]) <= df) and np.all(np.abs(g - c["g"]) <= dg)
    for name, t in wrong.items():
        _, _, f, g, _ = table_eval(t, c["r"])
        bad = (np.abs(f - c["f"]) > df) | (np.abs(g - c["g"]) > dg)
        far = np.maximum(np.abs(f - c["f"]) / df, np.abs(g - c["g"]) / dg)
        print(f"xi = {xi}, table {name}: {int(bad.sum())} of {len(bad)} points outside the bound, the nearest miss {far[bad].min():.3g} times it")
        assert bad.sum() >= len(bad) - 36, name      # (stride 21 reads intervals 0 and 1 almost right: their 36 points may pass)


def test_table_error_accounts_for_the_fp64_floor_at_xi_10(engine_mod, oracle):
    """The fp64 Lanczos operator meets the un-rounded M_real^{1/2} psi of the geometry "f: xi = 10" to 2.4e-9 only
    (tests/test_gpu_lanczos_fp64.py, measured on an MI355X), with nothing rounded in the operator.  Here, on the CPU: the dense
    M_real of that geometry from the closed forms, and again with f, g read from the host's table by the restated evaluation.  The
    tables' error alone (1.9e-10 at these r) moves M^{1/2} psi by 2.43e-9 relative: the floor is the table's format, and it lies
    inside what record_bound.table allows for it."""
    import record_bound as rb
    g = {x["name"]: x for x in rb.geometries()}["f: xi = 10 (overlapping pairs)"]
    pos, box, xi, rcut = g["pos"], g["box"], g["xi"], g["rcut"]
    n = len(pos)
    i, j, r, d = rb.pairs(pos, box, rcut)
    _, _, ft, gt, _ = table_eval(engine_mod.host_realspace_table(xi, rcut), r)
    fr, gr = ref.fg_real(r, xi)

    def dense(f, gg):
        M = np.eye(3 * n) * float(ref.self_mobility_mp(xi))
        for a, b, rr, dd, ff, g2 in zip(i, j, r, d, f, gg):
            B = ff * np.eye(3) + (g2 - ff) * np.outer(dd, dd) / rr ** 2
            M[3 * a:3 * a + 3, 3 * b:3 * b + 3] += B
            M[3 * b:3 * b + 3, 3 * a:3 * a + 3] += B
        return M
    M0, Mt = dense(fr, gr), dense(ft, gt)
    assert np.abs(M0 - rb.dense_mreal(oracle, pos, box, xi, rcut, rounded=False)).max() < 4 * U      # the oracle's dense matrix is this one
    psi = np.random.default_rng(n).normal(size=(n, 3))                                               # the psi of the GPU test
    want, lam = rb.sqrt_apply(M0, psi)
    got, _ = rb.sqrt_apply(Mt, psi)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    dM = np.linalg.norm(Mt - M0, 2)
    allowed = rb.sqrt_bound(rb.table(xi, rcut), lam) * np.linalg.norm(psi) / np.linalg.norm(want)
    print(f"f: xi = 10: |table - closed form| = {max(np.abs(ft - fr).max(), np.abs(gt - gr).max()):.2e}, ||dM|| = {dM:.2e}, lambda_min = {lam:.3e}: "
          f"M^1/2 psi moves by {rel:.3e} relative (the device's floor: 2.4e-9); record_bound.table allows {allowed:.3e}")
    assert dM <= rb.table(xi, rcut)                  # one partner per row: ||dM|| <= |df| + |d(g - f)| of a pair
    assert 1e-9 < rel <= allowed


# The oracle against the closed forms, in units of u = 2^-53 (absolute: |f|, |g| <= 1).  Its radial functions are long double inside
# and rounded to double once, so the floor is u / 2.  Largest value seen over every xi, error and point of this file (after the fix of
# the quadrature's panels and of the small-xi switch of the closed form): fg_real 1.0 u, fg_wave 1.0 u, fg_wave quad 1.0 u.
# Asserted: twice that, the margin being for points between the samples.
ORACLE_SEEN_U = {"fg_real": 1.0, "fg_wave": 1.0, "fg_wave_quad": 1.0}


def oracle_switch(xi):
    """Below this r the oracle's closed form hands over to its quadrature (oracle/pse_oracle.c fg_wave_l)."""
    return max(0.25, 0.025 / xi ** (4.0 / 3.0))


@pytest.mark.parametrize("xi", XIS)
def test_oracle_radial_functions_match_the_closed_forms(oracle, xi):
    """fg_real and both wave routes (the closed form with its small-r switch, and the quadrature alone at every r) against mpmath, at
    the points of the table test and either side of the switch: r = 0.25 and the oracle's switch for this xi, with the doubles next
    to them."""
    sw = oracle_switch(xi)
    edge = [0.2, np.nextafter(0.25, 0.0), 0.25, np.nextafter(0.25, 1.0), 0.3]
    if sw > 0.25:
        edge += [0.99 * sw, np.nextafter(sw, 0.0), sw, np.nextafter(sw, 9.0), 1.01 * sw]
    er = np.array(edge)
    efw, egw = ref.fg_wave(er, xi)
    ef, eg = ref.fg_real(er, xi)
    seen = dict.fromkeys(ORACLE_SEEN_U, 0.0)
    for error in ERRORS:
        c = case(xi, error)
        r = np.concatenate([c["r"], er])
        want = dict(fg_real=(np.concatenate([c["f"], ef]), np.concatenate([c["g"], eg])),
                    fg_wave=(np.concatenate([c["fw"], efw]), np.concatenate([c["gw"], egw])))
        want["fg_wave_quad"] = want["fg_wave"]
        route = lambda quad: tuple(np.array([oracle.fg_wave(float(x), xi, quad=quad) for x in r]).T)      # (the port takes one r)
        got = dict(fg_real=oracle.fg_real(r, xi), fg_wave=route(False), fg_wave_quad=route(True))
        for name in seen:
            seen[name] = max(seen[name], max(np.abs(got[name][0] - want[name][0]).max(), np.abs(got[name][1] - want[name][1]).max()) / U)
    print(f"xi = {xi}: oracle - closed form, in units of 2^-53: " + ", ".join(f"{n} {v:.3g}" for n, v in seen.items()))
    for name, v in seen.items():
        assert v <= 2.0 * ORACLE_SEEN_U[name], (name, v)
