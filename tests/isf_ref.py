"""Reference of the intermediate scattering functions (pse_isf_sample, pse_isf_correlate; include/pse_amd.h).

self_part(): in np.longdouble (eps 1.08e-19 where the C long double is the x87 format) from the float64 positions: the fractional
coordinates s = ((x - xy y)/Lx, y/Ly, z/Lz) now and at the origin, t = m.(s_now - s_org), t -= rint(t), cos and sin of 2 pi t, summed
per type and rounded to float64 once.  coll_part(): Re(rho_a(now) conj rho_b(origin)) of two density arrays, plain float64.

dyadic_case() and self_exact(): inputs whose every fractional coordinate is a multiple of 1/4 in [-1/2, 1/2) in a box where s is
computed without rounding, so that s, ds = s_now - s_org and m.ds are exact, every phasor is one of 1, -i, -1, i, and every sum is
an integer below 2^53: no sum can round in any order.  self_exact asserts all of that and counts the four values.

THE BOUND tol(), per component of self, per mode, for n_a particles of the type (eps = 2^-53; s_max >= 1/2 bounds |s| now and at
the origin).  The kernel's order of operations (k_isf_self, pse_amd/csrc/pse_scatter.hip), per particle:
  1. s_x = fma(-xy, y, x) / Lx: two roundings, |error| <= 2 eps s_max; s_y, s_z: one rounding, eps s_max.  Now and at the origin.
  2. ds_c = s_c(now) - s_c(origin): one rounding, <= eps |ds_c| <= 2 eps s_max.  Together |error of ds_x| <= 6 eps s_max, of ds_y and
     ds_z <= 4 eps s_max.  Every mode of a segment m0 + t d uses this same ds, and its phase is linear in the mode, so the errors of
     the seed (m0) and of the t steps (d) add up to exactly m.error(ds): 2 pi 6 eps s_max sum|m_i| = 37.7 eps s_max sum|m_i| in the
     phase, whatever m0 and d are.
  3. f_c = fma(m_c, ds_c, -rint(m_c ds_c)): the product loses its integer part exactly, one rounding of a value <= 1/2: eps / 2 each;
     (f_x + f_y) + f_z: eps / 2 and eps; t -= rint(t) and the factor -2: exact.  3 eps in t, 2 pi 3 eps = 18.9 eps in the phase.
  4. sincospi: 2 ulp = 2 eps.  Seed and step each: 20.9 eps per component.
  5. the recurrence: t <= 7 complex multiplications, each <= 2 eps per component, and the error of the step enters t times:
     20.9 (1 + 7) + 7 x 2 = 181 eps.
  6. the sums: one lane adds a span in particle order, the spans are added by lanes and a butterfly: every addition rounds a partial
     sum of at most n_a, eps n_a / 2, once per term.
Worst case per term: 181 eps + eps n_a / 2 + 37.7 eps s_max sum|m_i| = 2.0e-14 + 5.6e-17 n_a + 4.2e-15 s_max sum|m_i|.  With the factor
two that structure_factor_ref.tol takes:   tol = n_a (4e-14 + 1.2e-16 n_a + 8.4e-15 s_max sum|m_i|).

self_float64(): the kernel's order restated in plain float64 -- the plan's segments (plan() restates structure_factor_plan), the
exactly reduced products (an error-free product in place of the fused operation), the recurrence, the spans of 256 in particle order,
the lanes and the butterfly --, with NumPy's sin and cos behind the quadrant reduction of a sincospi.  The CPU tests hold it to half the bound."""
import numpy as np

import structure_factor_ref as sr
from structure_factor_ref import LD, need_extended_precision  # noqa: F401  (the tests take them from here)

DYADIC_BOXES = {"cube16": (16.0, 16.0, 16.0, 0.0), "tilt16": (16.0, 8.0, 32.0, 0.5)}
SPAN = 256          # isf_span at the sizes of the tests
RUN, SHORT = 8, 2   # SF_RUN, SF_SHORT


def _types(n, types):
    return np.zeros(n, dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)


def self_part(now, org, box, modes, types=None, ntypes=1):
    """self[a, q] = sum_{j of type a} exp(-2 pi i m_q.(s_j(now) - s_j(org))), complex128 rounded once from extended precision."""
    ds = sr.fractional(now, box, LD) - sr.fractional(org, box, LD)
    m = np.asarray(modes, dtype=np.int64).reshape(-1, 3).astype(LD)
    two_pi = LD(8) * np.arctan(LD(1))
    types = _types(len(ds), types)
    out = np.zeros((ntypes, m.shape[0]), dtype=np.complex128)
    for q0 in range(0, m.shape[0], 512):
        t = ds @ m[q0:q0 + 512].T
        t = t - np.rint(t)
        c, sn = np.cos(two_pi * t), np.sin(two_pi * t)
        for a in range(ntypes):
            sel = types == a
            out[a, q0:q0 + 512] = c[sel].sum(axis=0).astype(np.float64) - 1j * sn[sel].sum(axis=0).astype(np.float64)
    return out


def coll_part(rho_now, rho_org):
    """coll[a, b, q] = Re(rho_now[a, q] conj rho_org[b, q]) = re re + im im, float64."""
    return rho_now.real[:, None, :] * rho_org.real[None, :, :] + rho_now.imag[:, None, :] * rho_org.imag[None, :, :]


def s_max(box, *configurations):
    return max(sr.s_max(p, box) for p in configurations)


def tol(modes, n, smax=0.5):
    """The bound per component of self, per mode, for n particles of the type (module docstring)."""
    m = np.abs(np.asarray(modes, dtype=np.int64).reshape(-1, 3)).sum(axis=1)
    return n * (4e-14 + 1.2e-16 * n + 8.4e-15 * smax * m)


def worst_ratio(got, want, modes, counts, smax=0.5):
    """max over types and modes of the larger component error over tol(m, n_a); a type without particles must be exactly zero."""
    worst = 0.0
    for a, n in enumerate(counts):
        if n == 0:
            assert np.all(got[a] == 0.0)
            continue
        err = np.maximum(np.abs(got[a].real - want[a].real), np.abs(got[a].imag - want[a].imag))
        worst = max(worst, float((err / tol(modes, int(n), smax)).max()))
    return worst


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------

def dyadic_case(name, n, seed=0):
    """(now, org): two sets of n positions in DYADIC_BOXES[name] whose fractional coordinates are multiples of 1/4 in [-1/2, 1/2)."""
    box = DYADIC_BOXES[name]
    rng = np.random.default_rng(seed)
    return tuple(sr.from_fractional(rng.integers(-2, 2, size=(n, 3)) / 4.0, box) for _ in range(2))


def _quarters(pos, box):
    """4 s as integers; asserts that s, as the device computes it in float64, is an exact multiple of 1/4."""
    Lx, Ly, Lz, xy = box
    s64 = np.stack([(pos[:, 0] - xy * pos[:, 1]) / Lx, pos[:, 1] / Ly, pos[:, 2] / Lz], axis=1)
    sld = sr.fractional(pos, box, LD)
    assert np.array_equal(s64.astype(LD), sld), "s is not exact in float64"
    q = np.rint(4.0 * s64)
    assert np.array_equal(q / 4.0, s64), "s is not a multiple of 1/4"
    assert np.abs(pos).max() < 2.0 ** 20
    return q.astype(np.int64)


def self_exact(now, org, box, modes, types=None, ntypes=1):
    """The self part of a dyadic case in integers: complex128 (ntypes, nk) with integer components.  Every phasor is (-i)^j, j = m.(4 ds)
    mod 4; s and ds are asserted exact, the products and the sums are integers far below 2^53."""
    dq = _quarters(now, box) - _quarters(org, box)                    # 4 ds, exact integers
    m = np.asarray(modes, dtype=np.int64).reshape(-1, 3)
    j = (dq @ m.T) % 4                                                 # exp(-2 pi i j / 4) = (-i)^j
    assert np.abs(dq).max() * np.abs(m).max() * 3 < 2 ** 50
    re = (j == 0).astype(np.int64) - (j == 2)
    im = (j == 3).astype(np.int64) - (j == 1)
    types = _types(len(dq), types)
    out = np.zeros((ntypes, m.shape[0]), dtype=np.complex128)
    for a in range(ntypes):
        out[a] = re[types == a].sum(axis=0) + 1j * im[types == a].sum(axis=0)
    return out


def rho_exact(pos, box, modes, types=None, ntypes=1):
    """rho of a dyadic configuration in integers."""
    q = _quarters(pos, box)
    m = np.asarray(modes, dtype=np.int64).reshape(-1, 3)
    j = (q @ m.T) % 4
    re = (j == 0).astype(np.int64) - (j == 2)
    im = (j == 3).astype(np.int64) - (j == 1)
    types = _types(len(q), types)
    out = np.zeros((ntypes, m.shape[0]), dtype=np.complex128)
    for a in range(ntypes):
        out[a] = re[types == a].sum(axis=0) + 1j * im[types == a].sum(axis=0)
    return out


# ---- the kernel's order in float64 ---------------------------------------------------------------------------------------------------

def plan(modes):
    """structure_factor_plan restated: (distinct modes in the canonical order, inverse (the place of every listed mode among them),
    segments [(first, len, d)]): greedy arithmetic progressions of at most RUN modes, cut in front of (0, 0, 0)."""
    m = np.asarray(modes, dtype=np.int64).reshape(-1, 3)
    distinct, inverse = np.unique(m, axis=0, return_inverse=True)      # (lexicographic: mx, then my, then mz)
    nu, segs, q = len(distinct), [], 0
    zero = lambda u: not distinct[u].any()                             # noqa: E731
    while q < nu:
        d, ln = np.zeros(3, dtype=np.int64), 1
        if q + 1 < nu and not zero(q + 1):
            d, ln = distinct[q + 1] - distinct[q], 2
            while ln < RUN and q + ln < nu and not zero(q + ln) and np.array_equal(distinct[q + ln] - distinct[q + ln - 1], d):
                ln += 1
        segs.append((q, ln, d))
        q += ln
    return distinct, np.asarray(inverse).reshape(-1), segs


def _reduced(m, ds):
    """fma(m, ds, -rint(m ds)) for an integer m (|m| <= 4096) and float64 ds, by an error-free product: ds = hi + lo with 26 bits in
    hi, so that m hi and m lo are exact."""
    m = float(m)
    p = m * ds
    c = 134217729.0 * ds                                               # Veltkamp split, 2^27 + 1
    hi = c - (c - ds)
    lo = ds - hi
    err = (m * hi - p) + m * lo                                        # exact: m ds = p + err
    return (p - np.rint(p)) + err                                      # (p - rint(p) is exact; one rounding, as the fused operation)


def _sincospi(x):
    """(sin(pi x), cos(pi x)) as a sincospi computes them: x = k / 2 + r exactly with |r| <= 1/4, sin and cos of pi r, turned by the
    quadrant k -- exact at every multiple of 1/2."""
    k = np.rint(2.0 * x)
    r = x - 0.5 * k                                                     # exact
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    q = k.astype(np.int64) % 4
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def _phase(m, ds):
    t = (_reduced(m[0], ds[:, 0]) + _reduced(m[1], ds[:, 1])) + _reduced(m[2], ds[:, 2])
    t = t - np.rint(t)
    sn, cs = _sincospi(-2.0 * t)                                        # exp(-2 pi i t)
    return cs, sn


def _ordered_sum(pos, val):
    """The sum of val (the members of one type, at the positions `pos` of the group) in the kernel's order: spans of SPAN positions,
    each in ascending order; lane l of 64 adds the spans l, l + 64, ... in ascending order; then the xor butterfly."""
    lanes = np.zeros(64)
    span = pos // SPAN
    for r in np.unique(span):
        lanes[r % 64] += np.cumsum(val[span == r])[-1]                 # (cumsum adds one after the other)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    return lanes[0]


def self_float64(now, org, box, modes, types=None, ntypes=1):
    """The self part in plain float64, in the kernel's order (module docstring).  complex128 (ntypes, nk)."""
    ds = sr.fractional(now, box, np.float64) - sr.fractional(org, box, np.float64)
    distinct, inverse, segs = plan(modes)
    types = _types(len(ds), types)
    where = np.arange(len(ds))
    val = np.zeros((ntypes, len(distinct)), dtype=np.complex128)
    for first, ln, d in segs:
        cr, ci = _phase(distinct[first], ds)
        wr, wi = _phase(d, ds)
        for t in range(ln):
            for a in range(ntypes):
                sel = types == a
                val[a, first + t] = _ordered_sum(where[sel], cr[sel]) + 1j * _ordered_sum(where[sel], ci[sel])
            cr, ci = cr * wr - ci * wi, cr * wi + ci * wr
    return val[:, inverse]


# ---- the inputs that the CPU and the GPU tests share ---------------------------------------------------------------------------------

NMAX = 513                                       # two spans of 256 and one particle
ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)
GROUP = np.arange(1, NMAX, 2)


def mode_sets():
    """One mode; (0, 0, 0) alone; the half space |m_i| <= 3; a line of 201 modes per axis; 127, 128 and 129 scattered modes (their
    sorted neighbours pair up: 64 segments of two fill a wave at 128); the eight corners at +-4096; a list with duplicates."""
    s = sr.mode_sets()
    out = {k: s[k] for k in ("one", "zero", "half3", "corners", "xline", "yline", "zline")}
    for nk in (127, 128, 129):
        out[f"scattered{nk}"] = sr.scattered(nk, 64, seed=9)
    out["duplicates"] = np.array([[3, -2, 5], [-3, 2, -5], [3, -2, 5], [0, 0, 0], [3, -2, 5], [0, 0, 0], [4, -2, 5], [5, -2, 5]])
    return out


def configuration(name, n=NMAX):
    """(now, org): the first n of two sets of 513 seeded points of the box sr.BOXES[name]."""
    box = sr.BOXES[name]
    return sr.points(NMAX, box, seed=11)[:n].copy(), sr.points(NMAX, box, seed=12)[:n].copy()


def types_of(n, ntypes, empty=None, seed=21):
    """Seeded types below ntypes; `empty`: a type that no particle gets (the draws are of ntypes - 1 types, shifted past it)."""
    if ntypes == 1:
        return None
    if empty is None:
        return np.random.default_rng(seed).integers(0, ntypes, n)
    t = np.random.default_rng(seed).integers(0, ntypes - 1, n)
    return np.where(t >= empty, t + 1, t)


def general_cases():
    """[(id, box name, n, mode-set key, ntypes, empty type or None, grouped)]: what the GPU tests hold to the bound."""
    out = []
    for name in ("cubic", "tilted", "negative"):
        out += [(f"{name}-rows{n}", name, n, "half3", 2, None, False) for n in ROWS]
        out += [(f"{name}-{key}", name, NMAX, key, 1, None, False) for key in sorted(mode_sets())]
        out += [(f"{name}-group", name, NMAX, "half3", 3, None, True)]
    out += [(f"tilted-types{nt}", "tilted", NMAX, "zline", nt, None if nt == 1 else 1, False) for nt in (1, 2, 3, 8)]
    return out


def case_inputs(case):
    """(box, now, org, modes, types, ntypes, members or None) of a general case; positions and types are in the caller's order."""
    _, name, n, key, ntypes, empty, grouped = case
    now, org = configuration(name, n)
    members = GROUP if grouped else None
    return sr.BOXES[name], now, org, mode_sets()[key], types_of(n, ntypes, empty), ntypes, members


def case_reference(case, fn=None):
    """fn (default: self_part) on the members of a general case, and the number of members of every type."""
    box, now, org, modes, types, ntypes, members = case_inputs(case)
    if members is not None:
        now, org, types = now[members], org[members], None if types is None else types[members]
    counts = np.bincount(_types(len(now), types), minlength=ntypes)
    return (fn or self_part)(now, org, box, modes, types, ntypes), counts
