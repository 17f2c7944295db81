"""tests/realspace_ref.py held to what it does not contain: the reference's own closed forms in 50 digits (the pin fixture), the
defining Fourier integral by mpmath.quad, the continuity of f and g where the RPY branch switches, and their decay at the cutoff."""
import json
import math
import os

import mpmath
import numpy as np
import pytest

import realspace_ref as ref

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_arithmetic.json")))


def test_reference_matches_the_pin_rows():
    """Imrr_exact / rr_exact are the reference's expression text (PSEv1/Stokes.cc:348-406, three branches) in 50-digit arithmetic,
    stored as doubles: the mpmath closed forms rounded to double may differ from them by one rounding of each side, 2^-53 |value| each
    (|f|, |g| <= 1) -- r = 1e-3 .. 9.6 and r = 2 exactly."""
    rows = FIX["realspace"]["rows"]
    assert len(rows) > 100 and any(q["r"] == 2.0 for q in rows) and min(q["r"] for q in rows) <= 1e-3
    worst = 0.0
    for q in rows:
        f, g = ref.fg_real_mp(q["r"], q["xi"])
        worst = max(worst, abs(float(f) - q["Imrr_exact"]), abs(float(g) - q["rr_exact"]))
    print(f"closed forms against {len(rows)} pin rows: {worst:.2e}")
    assert worst <= 2.0 ** -52


@pytest.mark.parametrize("r,xi", [(0.1, 0.05), (1.53, 0.05), (0.249, 0.05), (30.0, 0.05), (3.0, 0.273), (2.0, 1.0), (0.125, 10.0)])
def test_wave_part_is_the_fourier_integral(r, xi):
    """mpmath.quad of the defining integral (30 digits, panels bounded by the oscillation and by the Gaussian) against the closed
    second-difference forms: independent of them, small xi included.  1e-24: quad's own estimate is below 1e-27 on these panels."""
    fq, gq = ref.fg_wave_fourier(r, xi, dps=30)
    fc, gc = ref.fg_wave_mp(r, xi)
    print(f"r = {r}, xi = {xi}: |df| = {float(abs(fq - fc)):.1e}, |dg| = {float(abs(gq - gc)):.1e}")
    assert abs(fq - fc) < 1e-24 and abs(gq - gc) < 1e-24


@pytest.mark.parametrize("xi", [0.05, 0.273, 0.5, 1.0, 4.0, 10.0])
def test_f_and_g_are_continuous_at_the_touching_distance(xi):
    """The RPY branches meet at r = 2 (both give f = 7/16, g = 5/8) and the wave parts are smooth: f(2 (1 + d)) - f(2 (1 - d)) is
    4 d |f'(2)| + O(d^2).  |f'|, |g'| <= 9/32 + |f_w'|, and differentiating under the Fourier integral (the bracket's derivative is
    below 1 in modulus, sinc^2(k) k <= min(k, 1/k)) gives |f_w'|, |g_w'| <= (3/pi) (1/2 + Int_1^inf H / k dk) < 2 + ln(1 + 2 xi)
    < 3 + 3 xi: with d = 2^-40 the jump allowed is 4 d (3 + 3 xi)."""
    d = 2.0 ** -40
    jump = 4 * d * (3 + 3 * xi)
    lo, hi, at = ref.fg_real_mp(2.0 * (1 - d), xi), ref.fg_real_mp(2.0 * (1 + d), xi), ref.fg_real_mp(2.0, xi)
    fw, gw = ref.fg_wave_mp(2.0, xi)
    assert abs(at[0] + fw - mpmath.mpf(7) / 16) < 1e-45 and abs(at[1] + gw - mpmath.mpf(5) / 8) < 1e-45
    for a, b, c in zip(lo, hi, at):
        assert abs(a - b) < jump and min(a, b) - jump < c < max(a, b) + jump


@pytest.mark.parametrize("xi", [0.05, 0.1, 0.273, 0.5])
@pytest.mark.parametrize("error", [1e-3, 1e-6])
def test_f_and_g_decay_at_the_rate_of_the_error_parameter(xi, error):
    """rcut = sqrt(-ln error) / xi makes exp(-xi^2 rcut^2) = error.  f and g are the two-sphere average of a kernel that falls like
    exp(-xi^2 s^2) times a polynomial of degree four in xi s, over distances s in [r - 2, r + 2]: an envelope is
    K exp(-xi^2 (r - 2)^2) with K = 3 xi (1 + xi r)^4.  exp(-xi^2 (r - 2)^2) = error^(m^2) exp(4 xi^2 r) at r = m rcut, so for the small
    xi of this test (4 xi^2 r = 4 m xi sqrt(-ln error) <= 11) the functions fall with error^(m^2) as the cutoff rule assumes; at m = 2
    they are below the envelope of m = 1 by more than error^2."""
    rc = math.sqrt(-math.log(error)) / xi
    env = lambda r: 3 * xi * (1 + xi * r) ** 4 * math.exp(-xi * xi * (r - 2) ** 2)
    vals = []
    for m in (1.0, 1.25, 1.5, 2.0):
        f, g = ref.fg_real_mp(m * rc, xi)
        vals.append(max(abs(f), abs(g)))
        assert vals[-1] < env(m * rc), (m, float(vals[-1]), env(m * rc))
    assert vals[0] > vals[1] > vals[2] > vals[3]
    assert vals[3] < env(rc) * error ** 2
    print(f"xi = {xi}, error = {error:g}: max(|f|, |g|) / error at rcut = {float(vals[0]) / error:.3g}")


def test_format_eps_is_a_maximum_over_intervals_and_grows_with_xi():
    """format_eps takes the worst interval; the format's cost grows with xi (the functions vary on the scale 1 / xi, the intervals do
    not shrink), and a subset of intervals can only give less."""
    ks = (0, 1, 15, 16, 24)
    e = [ref.format_eps(xi, 3.0, intervals=ks) for xi in (0.5, 2.0, 6.0, 10.0)]
    assert e[0] < e[1] < e[2] < e[3]
    assert ref.format_eps(2.0, 3.0, intervals=(15, 16)) <= e[1]
    assert e[1] == max(max(ref.interval_eps(2.0, k)) for k in ks)
    assert ref.n_intervals(3.0) == 25 and ref.n_intervals(3.01) == 26
    # the rounding part alone: C_ROUND 2^-53 sum |c_q| with sum |c_q| >= |f_w| ~ 1 at small r and large xi is the floor
    assert e[0] > ref.C_ROUND * 2.0 ** -53 * 0.5
