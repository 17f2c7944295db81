"""The device's real-space pair functions f(r), g(r) against the mpmath closed forms of tests/realspace_ref.py, xi from 0.05 to 10:
through pse_eval_realspace on every interval of the table, as each near-field kernel computes them (isolated pairs through
pse_mobility(parts = 1): the build pass, the kept-list pass, the packed cell pass, the table in LDS and in global memory), and as
M_real^{1/2} sees them (the pair list of the fp64 Lanczos operator).

ONE bound, derived from the code (eval_fg in pse_amd/csrc/pse_device.h), nothing in it measured on the device; u = 2^-53:
  * the table:  format_eps(xi) of tests/realspace_ref.py -- the interpolation error of degree 9 on eighths plus the rounding of ten
    coefficients and a ten-step Horner, from the closed forms alone;
  * the r that is looked up:  r' = r2 rsqrt(r2) with r2 = dx^2 + dy^2 + dz^2 (two fma and a product: 2 u relative, u in r), rsqrt
    (1 ulp: 2 u) and the product (u): |r' - r| <= RHO r, RHO = 2^-51.  f moves by RHO r |f'|, and r |f'| <= 3 P0f + 2.1,
    r |g'| <= 3 P0g + 1: P0 is the sum of the moduli of the terms of the analytic branch (powers r^-1, r^-3, or 1 and r), and under the
    Fourier integral of the wave part r d/dr turns the bracket j0(x) - j1(x)/x into -x j1(x) + j2(x), at most 1.4 in modulus (2 j1/x
    into -2 j2, at most 0.62), times (3/pi) Int H sinc^2 <= 3/2.  An r' that lands in the interval next to r's evaluates that
    interval's polynomial a distance <= 16 RHO r beyond its end, where it is as good as at the end to 1e-12 of itself;
  * the analytic branch:  ir = rsqrt(r2) carries 3 u, ir^2 6 u, ir^3 10 u, the products with the constants and the sum 2 u more:
    |df0| <= 12 u P0f, |dg0| <= 12 u P0g (r <= 2: one product and one difference of values <= 1.6, far inside that);
  * the subtraction f0 - fw:  u |f|;  (g0 - gw):  u |g|.
  So  df = format_eps + 12 u P0f + u |f| + RHO (3 P0f + 2.1),   dg = format_eps + 12 u P0g + u |g| + RHO (3 P0g + 1).
  * pse_eval_realspace returns g = f + h r^2 with h = ((g0 - gw) - f) ir^2:  the difference (u), ir^2 (6 u), two products and the sum:
    dg += 10 u |g - f| + u |g|.
  * a near-field kernel returns the row f F + h (d.F) d:  |du| <= (df + d(g - f)) |F| + 16 u (|f| + |g - f|) |F| with
    d(g - f) <= dg + df + u |g - f|  (h as above, the dot product three terms, three more products and the sum);
  * a self row is self F: the self term is one double (select_params, long double inside: u), the product rounds (u), and the
    reference row is rounded to double (u / 2 per component):  3 u |self| |F|.
"""
import functools
import math

import mpmath
import numpy as np
import pytest

from conftest import to4
import realspace_ref as ref
import record_bound as rb

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RHO = 2.0 ** -51
Q = 2.0 ** -40          # every coordinate is a multiple of Q, every box length an integer, xy Ly an integer: differences of positions
#                         and image shifts are exact in double, so the separation a kernel sees is the planted one to the last bit
ERROR = 1e-3
SKIN = 0.4              # r_buff of the kept neighbour list (the handle's default where the table fits the LDS)
GRID_SIZES = (8, 10, 12, 16, 20, 24, 30, 32, 36, 40, 48, 50, 54, 60, 64, 72, 80, 90, 96, 100, 108, 120, 128, 144, 150, 160)


def q(x):
    return np.round(np.asarray(x, float) / Q) * Q


def rule_rcut(xi):
    return math.sqrt(-math.log(ERROR)) / xi


@functools.lru_cache(maxsize=None)
def eps_of(xi, rcut):
    """format_eps over the probed intervals of this table (the first three hold the worst one: tests/test_realspace_table_cpu.py)."""
    return ref.format_eps(xi, rcut, intervals=ref.probe_intervals(rcut))


def p0(r):
    far = r > 2.0
    return (np.where(far, 0.75 / r + 0.5 / r ** 3, 1.0 + 0.28125 * r), np.where(far, 1.5 / r + 1.0 / r ** 3, 1.0 + 0.1875 * r))


def fg_bound(r, f, g, eps):
    """(df, dg) of the module docstring for f0 - fw and g0 - gw."""
    p0f, p0g = p0(r)
    return (eps + 12 * U * p0f + U * np.abs(f) + RHO * (3 * p0f + 2.1), eps + 12 * U * p0g + U * np.abs(g) + RHO * (3 * p0g + 1.0))


def small_grid(box, xi):
    """The smallest far-field grid the parameter check admits for this box (P = 2, no strain): the near field does not read it."""
    import pse_amd
    lmax = max(box[:3])
    for n in GRID_SIZES:
        grid = tuple(min(s for s in GRID_SIZES if s >= n * L / lmax) for L in box[:3])
        try:
            pse_amd.host_select_params(box, xi, ERROR, 0.0, grid=grid, P=2)
        except pse_amd.PSEError:
            continue
        return grid
    raise AssertionError(("no grid", box, xi))


def new_engine(n, box, xi, rcut=0.0, **kw):
    import pse_amd
    return pse_amd.Engine(n, box, xi=xi, error=ERROR, max_strain=0.0, grid=small_grid(box, xi), P=2, rcut=rcut, **kw)


# -- 1. pse_eval_realspace on every interval ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xi,rcut_override", [(0.05, 0.0), (0.1, 0.0), (0.273, 0.0), (0.5, 0.0), (1.0, 0.0), (2.0, 0.0), (4.0, 0.0),
                                              (10.0, 0.0), (0.273, 10.0), (0.5, 10.0)])
def test_eval_realspace_on_every_interval(xi, rcut_override):
    """Both ends of every interval the table holds and 8 points inside; r = 2 and the doubles either side; r = 1e-6; rcut (1 - 1e-9);
    the largest r the entry accepts and the first it refuses (the entry keeps 2^-50 away from the table's end: the kernel looks up
    r' = r2 rsqrt(r2), which may exceed r by RHO r, and the interval behind the last one does not exist)."""
    import pse_amd
    rcut = rcut_override or rule_rcut(xi)
    L = float(max(16, 2 * math.ceil(rcut) + 2))
    eng = new_engine(8, (L, L, L, 0.0), xi, rcut=rcut_override)
    assert abs(eng.info()["rcut"] - rcut) <= 1e-15 * rcut
    n = ref.n_intervals(rcut)
    pts = []
    for k in range(n):
        lo, hi = k / 8.0, (k + 1) / 8.0
        pts += [lo if k else 2.0 ** -30] + list(lo + (np.arange(8) + 0.41) / 64.0) + [np.nextafter(hi, 0.0)]
    r_max = n / 8.0
    while not r_max * 8.0 * (1.0 + 2.0 ** -50) < n:          # the entry's own test, on the same doubles
        r_max = np.nextafter(r_max, 0.0)
    assert n / 8.0 - r_max < 16 * 2.0 ** -50 * n / 8.0
    edge = [np.nextafter(2.0, 0.0), 2.0, np.nextafter(2.0, 3.0), 1e-6, rcut * (1 - 1e-9), r_max]
    r = np.array([x for x in pts if x <= r_max] + [x for x in edge if x <= r_max])
    assert len(r) >= 10 * n - 1
    f, g = eng.eval_realspace(r)
    with pytest.raises(pse_amd.PSEError, match="table range"):
        eng.eval_realspace(np.array([1.0, np.nextafter(r_max, 9e9)]) if n > 8 else np.array([np.nextafter(r_max, 9e9)]))
    eng.close()
    fr, gr = ref.fg_real(r, xi)
    eps = eps_of(xi, rcut)
    df, dg = fg_bound(r, fr, gr, eps)
    dg = dg + 10 * U * np.abs(gr - fr) + U * np.abs(gr)
    ef, eg = np.abs(f - fr), np.abs(g - gr)
    i = int(np.argmax(np.maximum(ef / df, eg / dg)))
    print(f"eval_realspace xi = {xi}, rcut = {rcut:.4f}, {n} intervals, {len(r)} points: max |f - f_ref| = {ef.max():.3e}, max |g - g_ref| = "
          f"{eg.max():.3e}; format_eps = {eps:.3e}, bound at the worst point (r = {r[i]:.17g}) {df[i]:.3e} / {dg[i]:.3e}, "
          f"error there {ef[i]:.3e} / {eg[i]:.3e}", flush=True)
    # MI355X, largest |f - f_ref| / |g - g_ref| (format_eps): xi = 0.05 .. 1: <= 1.4e-16 / 1.7e-16 (2.2e-16 .. 2.3e-15); 2: 1.8e-16 /
    # 1.2e-16 (2.6e-15); 4: 6.30e-14 / 1.0e-14 (6.60e-14); 10: 2.004e-10 / 3.0e-11 (2.073e-10) -- at large xi the error IS the format's
    assert np.all(ef <= df), (xi, r[np.argmax(ef / df)], (ef / df).max())
    assert np.all(eg <= dg), (xi, r[np.argmax(eg / dg)], (eg / dg).max())
    if xi <= ref.XI_TABLE:       # and with it the contract the older tests assert (tests/test_realspace_table_cpu.py: XI_TABLE)
        assert ef.max() < ref.CONTRACT and eg.max() < ref.CONTRACT


# -- 2. f, g as the near-field kernels compute them: isolated pairs -------------------------------------------------------------------
def separations(rcut, rmin=0.0, cap=50):
    """Target separations: both ends (the upper one Q below the edge) and the middle of the intervals up to rcut -- all of them, or
    `cap` of them: the first three, those either side of r = 2, the last three, the rest spread --, r = 2 and its neighbours, and
    rcut (1 -+ 1e-9).  Returns (r, inside): the pair just outside the cutoff must contribute exactly nothing."""
    n = int(math.ceil(8 * rcut))
    ks = range(n) if n <= cap else ref.probe_intervals(rcut - 0.125, cap)
    out = []
    for k in ks:
        out += [k / 8.0 if k else 2.0 ** -10, (k + 0.5) / 8.0, (k + 1) / 8.0 - Q]
        if n <= 8:                                       # a table of a handful of intervals (xi >= 4): the quarter points too
            out += [(k + 0.25) / 8.0, (k + 0.75) / 8.0]
    out += [2.0 - Q, 2.0, 2.0 + Q, math.floor(rcut * (1 - 1e-9) / Q) * Q]
    r = np.array(sorted(set(x for x in out if rmin <= x < rcut * (1 - 1e-9) + Q)))
    r = np.concatenate([r, [math.ceil(rcut * (1 + 1e-9) / Q) * Q]])
    return r, np.arange(len(r)) < len(r) - 1


def directions(r, rng):
    """Separation vectors on the grid Q: along x, y, z (the length is r exactly) and in general position, in turn."""
    d = np.zeros((len(r), 3))
    for m, x in enumerate(r):
        if m % 4 < 3:
            d[m, m % 4] = x * (-1) ** (m // 4)
        else:
            v = rng.normal(size=3)
            d[m] = q(x * v / np.linalg.norm(v))
    return d


def exact_r2(d):
    return [sum(mpmath.mpf(float(c)) ** 2 for c in row) for row in d]


@functools.lru_cache(maxsize=None)
def planted(xi, rmin=0.0, cap=50, spacing_for_skin=SKIN):
    """Isolated pairs on a simple-cubic lattice in a tilted box (xy = 0.25).  Site spacing a > 3 rcut + 2 skin + 1: particle i sits on
    the site, its partner j at site + d, |d| <= rcut (1 + 1e-9), and every particle may move by 0.05, so particles of different pairs
    stay further apart than a - 2 rcut - 0.2 > rcut + 2 skin.  The first layer of sites lies on the -y face of the box and the last
    column 0.25 inside its +x face: pairs there whose d points outward have the partner wrapped, and the kernels form r2 from an image
    shift (on the -y face d is turned outward where it has a y component: the sign of d changes neither r nor the block).
    F_i = 0, F_j random: u_i = [f (I - dd) + g dd] F_j, u_j = self F_j."""
    from oracle import pse_port
    rng = np.random.default_rng(int(1000 * xi) + 7)
    rcut = rule_rcut(xi)
    r, inside = separations(rcut, rmin, cap)
    d = directions(r, rng)
    npairs = len(r)
    a = 4.0 * math.ceil((3 * rcut + 2 * spacing_for_skin + 1.0 + 1e-9) / 4.0)
    nx = int(math.ceil(npairs ** (1 / 3)))
    ny = int(math.ceil(math.sqrt(npairs / nx)))
    nz = int(math.ceil(npairs / (nx * ny)))
    box = (nx * a, ny * a, nz * a, 0.25)
    idx = np.array([(i, j, k) for k in range(nz) for j in range(ny) for i in range(nx)][:npairs], float)
    d = np.where(((idx[:, 1] == 0) & (d[:, 1] > 0))[:, None], -d, d)   # on the -y face every d with a y component points outward
    sites = idx * a - 0.5 * np.array(box[:3])                       # first layers ON the -x, -y, -z faces
    sites[:, 0] += a - 0.25                                         # ... x: the last column 0.25 inside the +x face
    sites[:, 2] += 0.5 * a
    sites[:, 0] += box[3] * sites[:, 1]
    unwrapped = np.concatenate([sites, sites + d])
    assert np.array_equal(unwrapped, q(unwrapped))
    pos = pse_port.wrap(unwrapped, np.zeros(unwrapped.shape, dtype=np.int64), box)[0]
    got = pse_port.min_image(pos[npairs:] - pos[:npairs], box)
    assert np.array_equal(got, d), "the wrapped separations are not the planted ones to the last bit"
    wrapped = np.any(np.abs(pos[npairs:] - pos[:npairs] - d) > 1.0, axis=1)
    assert wrapped.sum() >= min(3, npairs // 8), wrapped.sum()
    force = np.zeros((2 * npairs, 3))
    force[npairs:] = rng.normal(size=(npairs, 3))
    # every pair translated rigidly by its own vector, |.| < 0.05: the separations stay what they are, to the last bit
    shift = q(rng.uniform(-0.028, 0.028, size=(npairs, 3)))
    moved = pse_port.wrap(unwrapped + np.concatenate([shift, shift]), np.zeros(unwrapped.shape, dtype=np.int64), box)[0]
    assert np.array_equal(pse_port.min_image(moved[npairs:] - moved[:npairs], box), d)
    # the reference rows, in mpmath from the exact separations
    r2 = exact_r2(d)
    u = np.zeros((2 * npairs, 3))
    fg = np.zeros((npairs, 2))
    self_m = ref.self_mobility_mp(xi)
    for m in range(npairs):
        F = [mpmath.mpf(float(c)) for c in force[npairs + m]]
        if inside[m]:
            rr = mpmath.sqrt(r2[m])
            f, g = ref.fg_real_mp(rr, xi)
            dm = [mpmath.mpf(float(c)) for c in d[m]]
            dF = sum(x * y for x, y in zip(dm, F)) / r2[m]
            u[m] = [float(f * F[c] + (g - f) * dF * dm[c]) for c in range(3)]
            fg[m] = float(f), float(g)
        u[npairs + m] = [float(self_m * c) for c in F]
    rr = np.array([float(mpmath.sqrt(x)) for x in r2])
    eps = eps_of(xi, rcut)
    df, dg = fg_bound(rr, fg[:, 0], fg[:, 1], eps)
    gmf = np.abs(fg[:, 1] - fg[:, 0])
    fn = np.linalg.norm(force[npairs:], axis=1)
    bound = np.zeros(2 * npairs)
    bound[:npairs] = np.where(inside, ((2 * df + dg + U * gmf) + 16 * U * (np.abs(fg[:, 0]) + gmf)) * fn, 0.0)
    bound[npairs:] = 3 * U * abs(float(self_m)) * fn
    out = dict(xi=xi, rcut=rcut, box=box, n=2 * npairs, npairs=npairs, pos=pos, moved=moved, force=force, d=d, r=rr, inside=inside,
               wrapped=wrapped, u=u, fg=fg, bound=bound, eps=eps, self=float(self_m), dfg=(df, dg))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_rows(c, u, what):
    """Every row within its bound; the pair outside the cutoff contributes exactly nothing; the two projections f and g printed."""
    n = c["npairs"]
    err = np.linalg.norm(u - c["u"], axis=1)
    assert np.all(u[:n][~c["inside"]] == 0.0), (what, u[:n][~c["inside"]])
    F = c["force"][n:]
    dh = c["d"] / c["r"][:, None]
    g_dev = (u[:n] * dh).sum(1) / (F * dh).sum(1)                   # u_i . d = g (F_j . d)
    ins = c["inside"]
    share = np.where(c["bound"] > 0, err / np.where(c["bound"] > 0, c["bound"], 1.0), 0.0)
    worst, worst_self = int(np.argmax(share[:n])), n + int(np.argmax(share[n:]))
    print(f"isolated pairs xi = {c['xi']}, {what}: {n} pairs ({int(c['wrapped'].sum())} through an image), max |u - u_ref| = {err[:n].max():.3e}, "
          f"nearest to its bound the pair at r = {c['r'][worst]:.17g}: {err[worst]:.3e} of {c['bound'][worst]:.3e}; self rows {err[n:].max():.3e}, "
          f"nearest {err[worst_self]:.3e} of {c['bound'][worst_self]:.3e}; max |g - g_ref| from u.d = "
          f"{np.abs(g_dev - c['fg'][:, 1])[ins & (np.abs((F * dh).sum(1)) > 0.3)].max():.3e}; format_eps = {c['eps']:.3e}", flush=True)
    # MI355X, largest |u - u_ref| of a pair row, and the bound of the row nearest to its bound: xi = 0.5: 5.2e-15 (5.0e-15 of 3.6e-14),
    # 1: 1.2e-15 (of 2.1e-14), 0.2 (global memory): 1.3e-14 (6.6e-15 of 1.4e-14), 4: 1.2e-13 (of 4.5e-13), 10: 1.5e-10 (7.0e-11 of
    # 4.0e-10); the three routes agree to 2e-16; self rows <= 0.62 of 3 u |self| |F|
    assert np.all(err <= c["bound"]), (what, int(np.argmax(share)), c["r"][int(np.argmax(share)) % n], share.max())


@pytest.mark.parametrize("xi", [0.5, 1.0])
def test_isolated_pairs_on_every_pass(xi):
    """Table in LDS: the build pass of a new handle (it writes the kept list), the kept-list pass after every particle has moved by
    less than 0.05, and the packed cell pass with the skin set to 0 -- the routes of tests/test_gpu_cell_grids.py."""
    c = planted(xi)
    eng = new_engine(c["n"], c["box"], xi)
    assert eng.neighbor_stats()[0] == SKIN
    _, b0, r0 = eng.neighbor_stats()
    u = eng.mobility(to4(c["pos"]), to4(c["force"]), parts=1).cpu().numpy()[:, :3]
    _, b1, r1 = eng.neighbor_stats()
    assert (b1, r1) == (b0 + 1, r0)
    check_rows(c, u, "(a) build pass + kept list")
    u = eng.mobility(to4(c["moved"]), to4(c["force"]), parts=1).cpu().numpy()[:, :3]
    _, b2, r2 = eng.neighbor_stats()
    assert (b2, r2) == (b1, r1 + 1), ("the kept list was not reused", b1, r1, b2, r2)
    check_rows(c, u, "(b) kept list")
    eng.set_neighbor_skin(0.0)
    u = eng.mobility(to4(c["pos"]), to4(c["force"]), parts=1).cpu().numpy()[:, :3]
    assert eng.neighbor_stats()[2] == r2
    check_rows(c, u, "(c) skin 0, packed records")
    eng.close()


@pytest.mark.parametrize("xi", [0.2, 4.0, 10.0])
def test_isolated_pairs_one_pass(xi):
    """xi = 0.2: rcut = 13.1, the table does not fit the LDS and the one pass reads it from global memory (no kept list).  xi = 4 and
    10: the whole table is a handful of intervals, every pair overlaps."""
    c = planted(xi, spacing_for_skin=0.0 if xi == 0.2 else SKIN)
    eng = new_engine(c["n"], c["box"], xi)
    assert eng.neighbor_stats()[0] == (0.0 if xi == 0.2 else SKIN)
    u = eng.mobility(to4(c["pos"]), to4(c["force"]), parts=1).cpu().numpy()[:, :3]
    check_rows(c, u, "table in global memory" if xi == 0.2 else "build pass + kept list")
    eng.close()


def test_isolated_pairs_at_small_xi_two_particles_at_a_time():
    """xi = 0.05: rcut = 52.6, a lattice of pairs would need a box of thousands; one engine of two particles in a box of 112, the
    positions rewritten in place, three dozen separations -- the ends of the first intervals, of those either side of r = 2 and of the
    last ones, r = 2, the cutoff from both sides -- along the axes, in general position, and through the tilted y face."""
    import torch
    from oracle import pse_port
    xi = 0.05
    rcut = rule_rcut(xi)
    box = (112.0, 112.0, 112.0, 0.25)
    rng = np.random.default_rng(5)
    r, inside = separations(rcut, cap=10)
    keep = np.concatenate([np.arange(0, len(r) - 1, max(1, (len(r) - 1) // 34)), [len(r) - 3, len(r) - 2, len(r) - 1]])
    r, inside = r[np.unique(keep)], inside[np.unique(keep)]
    d = directions(r, rng)
    eng = new_engine(2, box, xi)
    assert eng.neighbor_stats()[0] == 0.0                                   # the table is read from global memory
    eps = eps_of(xi, rcut)
    self_m = ref.self_mobility_mp(xi)
    dpos, dF = to4(np.zeros((2, 3))), to4(np.zeros((2, 3)))
    worst = (0.0, 0.0, 0.0, 0.0)
    for m in range(len(r)):
        site = q(np.array([rng.uniform(-50, 50), -56.0 if m % 3 == 0 else rng.uniform(-50, 50), rng.uniform(-50, 50)]))
        site[0] += 0.25 * site[1]
        pos = pse_port.wrap(np.stack([site, site + d[m]]), np.zeros((2, 3), dtype=np.int64), box)[0]
        assert np.array_equal(pse_port.min_image(pos[1:] - pos[:1], box)[0], d[m])
        F = np.stack([np.zeros(3), rng.normal(size=3)])
        dpos[:, :3] = torch.tensor(pos, dtype=torch.float64, device="cuda")
        dF[:, :3] = torch.tensor(F, dtype=torch.float64, device="cuda")
        u = eng.mobility(dpos, dF, parts=1).cpu().numpy()[:, :3]
        Fm = [mpmath.mpf(float(x)) for x in F[1]]
        assert np.linalg.norm(u[1] - [float(self_m * x) for x in Fm]) <= 3 * U * float(self_m) * np.linalg.norm(F[1])
        if not inside[m]:
            assert np.all(u[0] == 0.0), (r[m], u[0])
            continue
        r2 = exact_r2(d[m:m + 1])[0]
        f, g = ref.fg_real_mp(mpmath.sqrt(r2), xi)
        dm = [mpmath.mpf(float(x)) for x in d[m]]
        dFm = sum(x * y for x, y in zip(dm, Fm)) / r2
        want = np.array([float(f * Fm[k] + (g - f) * dFm * dm[k]) for k in range(3)])
        f, g, rr = float(f), float(g), np.array(float(mpmath.sqrt(r2)))
        df, dg = fg_bound(rr, f, g, eps)
        bound = ((2 * df + dg + U * abs(g - f)) + 16 * U * (abs(f) + abs(g - f))) * np.linalg.norm(F[1])
        err = np.linalg.norm(u[0] - want)
        if err / bound > worst[0]:
            worst = (err / bound, float(rr), err, float(bound))
        assert err <= bound, (float(rr), d[m], err, bound)                   # MI355X: at most 0.27 of it (2.0e-15 of 7.5e-15, r = 2.125)
    print(f"isolated pairs xi = 0.05, two particles at a time: {len(r)} separations, worst at r = {worst[1]:.17g}: |u - u_ref| = {worst[2]:.3e} "
          f"of bound {worst[3]:.3e}; format_eps = {eps:.3e}", flush=True)
    eng.close()


# -- 3. M_real^{1/2} reads the same table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xi,rmin", [(0.5, 1.0), (4.0, 0.25)])
def test_sqrt_mreal_of_isolated_pairs(xi, rmin):
    """The fp64 Lanczos operator on isolated pairs, tol = 1e-12.  M_real is then block diagonal, one 6 x 6 block [[s I, B], [B, s I]]
    per pair with B = f (I - dd) + g dd and s the self term; its square root is [[A, C], [C, A]] with, along d (lambda = g) and across it
    (lambda = f), a = (sqrt(s + lambda) + sqrt(s - lambda)) / 2 and c = (sqrt(s + lambda) - sqrt(s - lambda)) / 2 -- mpmath again.
    Separations from rmin up, so that the blocks stay well conditioned (s - f -> 0 as r -> 0) and the iteration converges inside the
    basis cap.  Bound: the Lanczos tolerance times |psi|, plus the table term through the square root (record_bound.sqrt_bound): each
    row has one partner, so ||dM||_2 <= max over pairs of df + d(g - f), the bound of the module docstring."""
    c = planted(xi, rmin=rmin)
    n, npairs = c["n"], c["npairs"]
    tol = 1e-12
    psi = np.random.default_rng(11).normal(size=(n, 3))
    s = ref.self_mobility_mp(xi)
    want = np.zeros((n, 3))
    lam_min, lam_max = mpmath.mpf(s), mpmath.mpf(s)
    r2 = exact_r2(c["d"])
    for m in range(npairs):
        pi_, pj = ([mpmath.mpf(float(x)) for x in psi[k]] for k in (m, npairs + m))
        if not c["inside"][m]:
            rs = mpmath.sqrt(s)
            want[m], want[npairs + m] = [float(rs * x) for x in pi_], [float(rs * x) for x in pj]
            continue
        f, g = ref.fg_real_mp(mpmath.sqrt(r2[m]), xi)
        dm = [mpmath.mpf(float(x)) for x in c["d"][m]]
        lam_min, lam_max = min(lam_min, s - abs(f), s - abs(g)), max(lam_max, s + abs(f), s + abs(g))
        coef = {}
        for name, lam in (("perp", f), ("par", g)):
            hi, lo = mpmath.sqrt(s + lam), mpmath.sqrt(s - lam)
            coef[name] = ((hi + lo) / 2, (hi - lo) / 2)

        def apply(x, which):
            xd = sum(p * t for p, t in zip(x, dm)) / r2[m]
            return [coef["perp"][which] * (x[k] - xd * dm[k]) + coef["par"][which] * xd * dm[k] for k in range(3)]
        want[m] = [float(a + b) for a, b in zip(apply(pi_, 0), apply(pj, 1))]
        want[npairs + m] = [float(a + b) for a, b in zip(apply(pj, 0), apply(pi_, 1))]
    assert lam_min > 0 and lam_max / lam_min < 50, (float(lam_min), float(lam_max))   # the case is the well-conditioned one it is meant to be
    df, dg = c["dfg"]
    gmf = np.abs(c["fg"][:, 1] - c["fg"][:, 0])
    dM = float(np.where(c["inside"], 2 * df + dg + U * gmf + 16 * U * (np.abs(c["fg"][:, 0]) + gmf), 0.0).max())
    bound = (tol + rb.sqrt_bound(dM, float(lam_min))) * np.linalg.norm(psi)
    eng = new_engine(n, c["box"], xi, lanczos_operator="fp64")
    out, m = eng.sqrt_mreal(to4(c["pos"]), to4(psi), tol=tol)
    step = eng.info()["lanczos_stepnorm"]
    eng.close()
    err = np.linalg.norm(out.cpu().numpy()[:, :3] - want)
    print(f"sqrt_mreal fp64 on isolated pairs xi = {xi}: {npairs} pairs, r >= {rmin}, condition {float(lam_max / lam_min):.1f}, m = {m}, "
          f"step norm {step:.2e}; |out - M^1/2 psi| = {err:.3e}, bound {bound:.3e} (tol |psi| = {tol * np.linalg.norm(psi):.3e}, table term "
          f"{rb.sqrt_bound(dM, float(lam_min)) * np.linalg.norm(psi):.3e})", flush=True)
    assert m < 100 and step <= tol, (m, step)
    assert err <= bound, (xi, err, bound)        # MI355X: xi = 0.5: 1.5e-12 of 2.5e-11 (m = 19); xi = 4: 1.7e-13 of 1.6e-11 (m = 11)
