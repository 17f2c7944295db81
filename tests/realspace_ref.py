"""The real-space pair functions f(r), g(r) of M_real = f (I - rr) + g rr in mpmath, from the closed forms alone, and the error that the
FORMAT of the device's table costs -- a reference that depends on nothing it checks (no quadrature, no host builder, no device).

The closed forms (derivation: the comment above W0 in oracle/pse_oracle.c; restated here, not called):
  the smooth part of the Hasimoto-split biharmonic kernel is B_w(s) = s erf(xi s) + exp(-xi^2 s^2) / (xi sqrt(pi)); W0'' = s B_w(s),
  W1 = W0', W2 = W0''; with the second differences D_i = W_i(r + 2) - 2 W_i(r) + W_i(r - 2) (two spheres of radius a = 1)
      f_w = 3 / (16 r) (D2 - D1 / r + D0 / r^2),      g_w = 3 / (8 r^2) (D1 - D0 / r)
  are the free-space wave parts, and f = f_RPY - f_w, g = g_RPY - g_w with the RPY branch at r = 2:
      r > 2: f_RPY = 3/(4r) + 1/(2r^3), g_RPY = 3/(2r) - 1/r^3;      r <= 2: f_RPY = 1 - 9r/32, g_RPY = 1 - 3r/16.
The differences cancel like 1 / (xi^4 r^3) at small r: the working precision is DPS = 50 digits plus the digits that cancellation
costs at the (r, xi) asked for, so the forms hold for every r > 0 and need no small-r switch.

The table's format (pse_amd/csrc/pse_host.h, eval_fg in pse_device.h): on every interval [k/8, (k+1)/8) the wave parts are ten double
coefficients of a polynomial in t = 2 (8r - k) - 1, evaluated by a ten-term Horner in double.  format_eps bounds what that costs.
"""
import functools
import math

import mpmath
from mpmath import mp, mpf

DPS = 50
PER_UNIT = 8       # RS_PER_UNIT
NCOEF = 10         # RS_NCOEF
N_SAMPLE = 128     # an interval's interpolant is held to the reference at t = cos(pi i / N_SAMPLE), i = 0 .. N_SAMPLE: both ends and 127 inside
SAMPLING = 1.0 / math.cos(NCOEF * math.pi / (2 * N_SAMPLE))   # what the largest sample may miss of the true maximum (interval_eps)
C_ROUND = 24.0     # see interval_eps
CONTRACT = 2e-13   # |f - f_ref|, |g - g_ref| of the device's table as the GPU tests have always asserted it ...
XI_TABLE = 4.0     # ... which the format can keep up to this xi: the largest listed one with format_eps < CONTRACT, as
#                    tests/test_realspace_table_cpu.py finds it from the closed forms (6.6e-14 at 4, 4.9e-13 at 6, 2.1e-10 at 10)


def _dps(r, xi):
    """Digits: DPS after the cancellation eps / (xi^4 r^3) of the second differences (and of f_RPY - f_w where f is tiny)."""
    lost = -math.log10(min(1.0, float(xi) ** 4 * float(r) ** 3))
    return DPS + 10 + int(math.ceil(lost))


def _W(s, xi):
    """W0, W1, W2 at s (odd in s; one erf and one exp)."""
    x2 = xi * xi
    e = mpmath.erf(xi * s)
    g = mpmath.exp(-x2 * s * s) / mpmath.sqrt(mpmath.pi)
    s2 = s * s
    w0 = e * (s2 * s2 / 12 - 1 / (16 * x2 * x2)) + g * (s2 * s / (12 * xi) - s / (24 * x2 * xi))
    w1 = s2 * s / 3 * e + g * (2 * x2 * s2 - 1) / (6 * x2 * xi)
    w2 = s2 * e + s * g / xi
    return w0, w1, w2


def _wave(r, xi):
    a, b, c = _W(r + 2, xi), _W(r, xi), _W(r - 2, xi)
    d0, d1, d2 = (a[i] - 2 * b[i] + c[i] for i in range(3))
    return 3 / (16 * r) * (d2 - d1 / r + d0 / (r * r)), 3 / (8 * r * r) * (d1 - d0 / r)


def _rpy(r):
    if r > 2:
        r3 = r * r * r
        return mpf(3) / (4 * r) + 1 / (2 * r3), mpf(3) / (2 * r) - 1 / r3
    return 1 - 9 * r / 32, 1 - 3 * r / 16


def fg_wave_mp(r, xi):
    """(f_w, g_w) as mpf; r, xi taken as the exact values of the doubles (or mpf) given."""
    with mp.workdps(_dps(r, xi)):
        fw, gw = _wave(mpf(r), mpf(xi))
        return +fw, +gw


def fg_real_mp(r, xi):
    """(f, g) as mpf."""
    with mp.workdps(_dps(r, xi)):
        r_, xi_ = mpf(r), mpf(xi)
        fw, gw = _wave(r_, xi_)
        f0, g0 = _rpy(r_)
        return f0 - fw, g0 - gw


def fg_wave(r, xi):
    """(f_w, g_w) rounded to double, for a sequence of r."""
    import numpy as np
    out = np.array([[float(v) for v in fg_wave_mp(float(x), xi)] for x in np.ravel(r)]).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def fg_real(r, xi):
    """(f, g) rounded to double, for a sequence of r."""
    import numpy as np
    out = np.array([[float(v) for v in fg_real_mp(float(x), xi)] for x in np.ravel(r)]).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def fg_wave_fourier(r, xi, dps=30):
    """(f_w, g_w) from the defining Fourier integral by mpmath.quad -- independent of the closed forms:
         f_w = (3/pi) Int_0^inf H(k) sinc^2(k) [j0(kr) - j1(kr)/(kr)] dk,   g_w = (3/pi) Int_0^inf H(k) sinc^2(k) 2 j1(kr)/(kr) dk,
       H(k) = (1 + k^2/4xi^2) exp(-k^2/4xi^2).  Panels of at most half a period of the fastest factor and a quarter of the Gaussian's
       width, out to where H < 1e-40."""
    with mp.workdps(dps):
        r, xi = mpf(r), mpf(xi)
        kmax = 2 * xi * mpmath.sqrt(100)
        dk = min(mpmath.pi / (r + 2), xi / 2)
        n = int(mpmath.ceil(kmax / dk))
        pts = [kmax * i / n for i in range(n + 1)]

        def j0(x): return mpmath.sinc(x)

        def j1ox(x):
            if abs(x) < mpf(10) ** (-dps // 6):
                return mpf(1) / 3 - x * x / 30 + x ** 4 / 840 - x ** 6 / 45360
            return (mpmath.sin(x) / x - mpmath.cos(x)) / (x * x)

        def H(k):
            q = k * k / (4 * xi * xi)
            return (1 + q) * mpmath.exp(-q) * mpmath.sinc(k) ** 2

        f = mpmath.quad(lambda k: H(k) * (j0(k * r) - j1ox(k * r)), pts)
        g = mpmath.quad(lambda k: H(k) * 2 * j1ox(k * r), pts)
        return 3 / mpmath.pi * f, 3 / mpmath.pi * g


# ---- the table's format -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cheb_to_monomial():
    C = [[0] * NCOEF for _ in range(NCOEF)]
    C[0][0] = 1
    C[1][1] = 1
    for q in range(2, NCOEF):
        for p in range(NCOEF):
            C[q][p] = (2 * C[q - 1][p - 1] if p > 0 else 0) - C[q - 2][p]
    return C


@functools.lru_cache(maxsize=None)
def interval_eps(xi, k):
    """The format's error on the interval [k/8, (k+1)/8): (eps_f, eps_g) as floats.

    Interpolation: the degree-9 interpolants of the reference f_w, g_w at the ten Chebyshev nodes of the first kind, written in powers of
    t as the table holds them (exact coefficients c_q, in mpmath); their largest distance from the reference over the N_SAMPLE + 1
    points t = cos(pi i / N_SAMPLE), both ends among them, times SAMPLING: the error of an interpolant at Chebyshev nodes is a smooth
    factor times T_10(t) = cos(10 theta), t = cos(theta); between two samples theta moves by pi / N_SAMPLE, so an extremum of cos(10
    theta) lies within 10 pi / (2 N_SAMPLE) in phase of a sample, which then sees at least cos(10 pi / (2 N_SAMPLE)) = 0.9925 of it.

    Rounding: C_ROUND 2^-53 sum |c_q| with C_ROUND = 24, from the operations of eval_fg (u = 2^-53, |t| <= 1):
      * each stored coefficient is c_q (1 + d), |d| <= u:                                      u sum |c_q|;
      * Horner in nine steps, each one fma (one rounding) or a product and a sum (two): the classical bound gamma_18 sum |c_q| |t|^q
        with gamma_18 = 18 u / (1 - 18 u):                                                       18 (1 + 2^-48) u sum |c_q|;
      * t itself: 8 r, the integer part and s - k are exact, 2 (s - k) - 1 rounds once where s - k < 1/4, by at most u / 2; the
        polynomial moves by |p'| u / 2 <= (u / 2) sum q |c_q| <= 4.5 u sum |c_q|.
      1 + 18 + 4.5 = 23.5, rounded up."""
    xi = float(xi)
    n = NCOEF
    lo = mpf(k) / PER_UNIT
    # the digits of the smallest r looked at bound the cancellation for the whole interval (interval 0: r = 2^-24, see below)
    rmin = float(lo) if k > 0 else 2.0 ** -24
    dps = _dps(rmin, xi)
    with mp.workdps(dps):
        xim = mpf(xi)
        tn, cosq, ts = _nodes(dps)
        vals = [_wave(lo + (t + 1) / (2 * PER_UNIT), xim) for t in tn]
        C = _cheb_to_monomial()
        polys = []
        for which in (0, 1):
            cheb = [sum(vals[m][which] * cosq[q][m] for m in range(n)) * (1 if q == 0 else 2) / n for q in range(n)]
            polys.append([sum(cheb[q] * C[q][p] for q in range(p, n)) for p in range(n)])
        worst = [mpf(0), mpf(0)]
        for i, t in enumerate(ts):
            if k == 0 and i == len(ts) - 1:
                t = mpf(-1) + mpf(2) ** -20      # r = 0 itself is not a point of the table (r > 0): r = 2^-24 stands for its lower end
            ref = _wave(lo + (t + 1) / (2 * PER_UNIT), xim)
            for which in (0, 1):
                p = polys[which][n - 1]
                for q in range(n - 2, -1, -1):
                    p = p * t + polys[which][q]
                worst[which] = max(worst[which], abs(p - ref[which]))
        return tuple(float(SAMPLING * worst[which] + C_ROUND * mpf(2) ** -53 * sum(abs(c) for c in polys[which])) for which in (0, 1))


@functools.lru_cache(maxsize=None)
def _nodes(dps):
    """At `dps` digits: the ten Chebyshev nodes, cos(q theta_m) at them, and the N_SAMPLE + 1 sample points cos(pi i / N_SAMPLE)."""
    n = NCOEF
    with mp.workdps(dps):
        th = [mpmath.pi * (m + mpf(1) / 2) / n for m in range(n)]
        return ([mpmath.cos(a) for a in th], [[mpmath.cos(q * a) for a in th] for q in range(n)],
                [mpmath.cos(mpmath.pi * i / N_SAMPLE) for i in range(N_SAMPLE + 1)])


def n_intervals(rcut):
    """Intervals of the table of a cutoff: 0 .. ceil(8 rcut) (build_realspace_table)."""
    return int(math.ceil(rcut * PER_UNIT)) + 1


def probe_intervals(rcut, cap=16):
    """At most `cap` intervals of the table of rcut, for the tests that cannot afford every one (128 mpmath samples each): the first
    three (small r, where the wave parts vary fastest and the format is at its worst), 15, 16, 17 (either side of r = 2, where the
    analytic branch switches), the last three (the one that holds rcut and the one beyond it, which the table carries), the rest
    spread evenly.  tests/test_realspace_table_cpu.py shows on dense scans that the largest interval_eps is among them."""
    n = n_intervals(rcut)
    must = sorted(set(k for k in (0, 1, 2, 15, 16, 17, n - 3, n - 2, n - 1) if 0 <= k < n))
    room = max(cap - len(must), 0)
    spread = [int(round(3 + (n - 7) * i / max(room - 1, 1))) for i in range(room)] if n > 8 else []
    return sorted(set(must) | set(k for k in spread if 0 <= k < n))


def self_mobility_mp(xi):
    """The self term of M_real (PSEv1/Stokes.cc:319), a = 1: (1 + 4 sqrt(pi) xi erfc(2 xi) - exp(-4 xi^2)) / (4 sqrt(pi) xi)."""
    with mp.workdps(DPS + 10 + int(math.ceil(-math.log10(min(1.0, float(xi)))))):
        x, sp = mpf(xi), mpmath.sqrt(mpmath.pi)
        return (1 + 4 * sp * x * mpmath.erfc(2 * x) - mpmath.exp(-4 * x * x)) / (4 * sp * x)


def format_eps(xi, rcut, intervals=None):
    """The error that the table's format alone costs f_w or g_w (hence f or g) anywhere in (0, rcut]: the largest interval_eps over
    every interval up to ceil(8 rcut) -- or over `intervals`, a subset of them (the CPU tests cap the count per case)."""
    ks = range(n_intervals(rcut)) if intervals is None else intervals
    return max(max(interval_eps(float(xi), int(k))) for k in ks)
