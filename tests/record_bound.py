"""A bound on what the 16-byte pair records of the per-step pair list do to the near-field operator, from the un-rounded f, g alone.

The Lanczos iteration of M_real^{1/2} psi applies every pair's term f v + h (d.v) d (h = (g - f) / r^2) from a record that holds it as
four rounded numbers (pse_amd/csrc/pse_kernels.hip, pair_coef / nb_pack): fr = f as a signed 26-bit integer in units of 2^-24, and
s = d sqrt|h| (the root taken in single precision) as three signed 22-bit mantissas under the exponent e of its largest component
(value = m 2^(e - 21), e clamped to [-100, 100]), the sign of h in a bit; the term is then fr v + sgn(h) (s.v) s.  Nothing below reads
that rounding restated (oracle/pse_oracle.c pair_term, rounded=True): only the un-rounded f, g (oracle fg_real) and the record format.
The tests use it two ways: on the CPU it must bound the restatement (tests/test_record_bound.py), on the GPU it bounds how far the
device's M_real^{1/2} psi may be from the true one (tests/test_gpu_lanczos_truth.py and the truth assertions beside the restatement
ones).

Error of one pair term in operator norm, T = f I + sgn(h) s s^T against T_r = fr I + sgn(h) s_r s_r^T (u = 2^-24):
  * fr: f 2^24 is exact in double, rint is off by <= 1/2, so |fr - f| <= 2^-25 -- as long as |f| < 2 (the 26-bit field saturates at
    +-(2 - 2^-24) silently; tests/test_record_bound.py holds |f| < 2 over every admitted xi and r).
  * the root: sqrtf((float)|h|) = sqrt|h| (1 + d1) with |d1| <= u/2 (the conversion, halved by the root) + u (sqrtf) + u^2, and the
    three products d_p sqrt|h| in double add 2^-53: |d1| <= 1.501 u.  (Valid for |h| >= 2^-126, a normal float: pair_eps checks it.)
  * the mantissas: with m the largest |component| and 2^(e-1) <= m < 2^e, each component is off by at most half a unit 2^(e - 21),
    i.e. <= m 2^-21 -- or a whole unit where the largest one rounds up to 2^21 and is clamped to 2^21 - 1, which needs m > 2^e (1 - 2^-22):
    again <= m 2^-21 (1 + 2^-21).  Over three components |s_r - s| <= |s| k with k = 1.501 u + sqrt(3) 2^-21 (1 + 2^-21)(1 + 1.501 u)
    = 0.9599 2^-20.
  * |s_r s_r^T - s s^T| <= |s_r - s| (|s_r| + |s|) <= |s|^2 k (2 + k), and |s|^2 = |h| r^2 = |g - f|:  <= 1.9198 2^-20 |g - f|.
    The sign bit is h's own: it adds nothing.
  So eps_ij <= 2^-25 + c |g - f| 2^-20 with c = 2.  An exponent below -100 is clamped: the units are then 2^-121 and the component
  error 2^-122 absolute, but such an s has |s| < 2^-100 and |s s^T| < 2^-199; the absolute 2^-198 added below covers it.

Error of the whole operator: dM = M_r - M is symmetric (both directions of a pair round alike, the self term is exact), so
||dM||_2 <= max_i sum_j ||dM_ij||_2 (block Gershgorin / Schur test) <= max_i sum_j eps_ij.

Error of the square root: for symmetric positive definite A, B, ||A^{1/2} - B^{1/2}|| <= ||A - B|| / (sqrt(lmin A) + sqrt(lmin B)), and
lmin(M_r) >= lmin(M) - ||dM|| (Weyl), so ||M_r^{1/2} psi - M^{1/2} psi|| <= ||dM|| / (sqrt(lmin) + sqrt(lmin - ||dM||)) ||psi||.

The vector rows (single GPU): the pair-list mat-vec gathers each neighbour's vector row from a 16-byte mirror, three 40-bit mantissas
under one exponent (pse_amd/csrc/pse_device.h vq_pack): |v_r - v|_row <= sqrt(3) 2^-39 |v|_row.  That perturbs each product by at most
sqrt(3) 2^-39 max_i sum_j ||T_ij|| ||v|| -- not a fixed operator, but of the size of one: ~2e-12 of the row sum, four orders below the
records.  `vector_rows=True` adds it to ||dM||; it never decides a test.
"""
import math

import numpy as np

U = 2.0 ** -24
C_S = 2.0                    # the c of eps_ij (derivation above: 1.9198 rounded up)
EPS_F = 2.0 ** -25           # rounding of fr
EPS_ABS = 2.0 ** -198        # an exponent clamped at -100
VEC_ROWS = math.sqrt(3.0) * 2.0 ** -39


def table(xi, rcut):
    """What the device's table adds to a pair term, |df| + |d(g - f)| <= 3 max(|df|, |dg|).  Up to xi = XI_TABLE the table is held to
    the closed forms at 2e-13 each (tests/test_realspace_table_cpu.py: the format allows it): 6e-13.  Beyond, degree 9 on eighths
    cannot follow a function of scale 1 / xi and the table is as good as its format: 3 format_eps(xi, rcut), from the mpmath closed
    forms alone (tests/realspace_ref.py) -- 6.2e-10 at xi = 10, still below the 2^-25 of the records."""
    import realspace_ref
    if xi <= realspace_ref.XI_TABLE:
        return 6e-13
    return 3.0 * realspace_ref.format_eps(xi, rcut)


def pair_eps(f, g, r=None):
    """Operator-norm error of one pair term read from its record (the bound derived above)."""
    f = np.asarray(f, float); g = np.asarray(g, float)
    if np.any(np.abs(f) >= 2.0 - U):
        raise ValueError("|f| >= 2: the 26-bit fr field saturates, the bound does not hold")
    if r is not None:
        h = np.abs(g - f) / np.asarray(r, float) ** 2
        if np.any((h > 0.0) & (h < 2.0 ** -126)):
            raise ValueError("|h| below the smallest normal float: the relative error of sqrtf does not hold")
    return EPS_F + C_S * np.abs(g - f) * 2.0 ** -20 + EPS_ABS


def pairs(pos, box, rcut):
    """Minimum-image pairs i < j with r < rcut: (i, j, r, d) -- the pairs of the near-field sum (rcut <= half the box)."""
    from oracle import pse_port
    pos = np.asarray(pos, float)
    i, j = np.triu_indices(len(pos), 1)
    d = pse_port.min_image(pos[i] - pos[j], box)
    r = np.linalg.norm(d, axis=1)
    keep = r < rcut
    return i[keep], j[keep], r[keep], d[keep]


def operator_bound(pos, box, xi, rcut, extra_pair=0.0, vector_rows=False):
    """Bound on ||M_r - M||_2 (block Gershgorin over eps_ij + extra_pair per pair), from the un-rounded f, g."""
    from oracle import pse_port
    n = len(pos)
    i, j, r, _ = pairs(pos, box, rcut)
    f, g = pse_port.fg_real(r, xi) if len(r) else (np.zeros(0), np.zeros(0))
    e = pair_eps(f, g, r) + extra_pair
    row = np.zeros(n)
    np.add.at(row, i, e); np.add.at(row, j, e)
    b = float(row.max()) if n else 0.0
    if vector_rows:
        t = np.abs(f) + np.abs(g - f)
        rs = np.full(n, abs(pse_port.self_mobility(xi)))
        np.add.at(rs, i, t); np.add.at(rs, j, t)
        b += VEC_ROWS * float(rs.max())
    return b


def dense_mreal(oracle, pos, box, xi, rcut, rounded):
    """The 3N x 3N near-field matrix, column by column through the oracle (N <= 200)."""
    n = len(pos)
    eye = np.eye(3 * n)
    M = np.stack([oracle.mobility_real(pos, eye[c].reshape(n, 3), box, xi, rcut, rounded=rounded).ravel() for c in range(3 * n)], 1)
    return M


def sqrt_apply(M, psi):
    """M^{1/2} psi for symmetric positive definite M (eigendecomposition in double)."""
    lam, V = np.linalg.eigh(0.5 * (M + M.T))
    return (V @ (np.sqrt(np.maximum(lam, 0.0)) * (V.T @ np.ravel(psi)))).reshape(np.shape(psi)), float(lam.min())


def sqrt_bound(dM, lam_min):
    """Bound on ||M_r^{1/2} - M^{1/2}||_2 for ||M_r - M||_2 <= dM."""
    if not dM < lam_min:
        raise ValueError("the perturbation bound reaches the smallest eigenvalue")
    return dM / (math.sqrt(lam_min) + math.sqrt(lam_min - dM))


def truth(oracle, pos, box, xi, rcut, psi, extra_pair=0.0, vector_rows=False):
    """The un-rounded reference and its bound: dict ref = M^{1/2} psi (dense M, no rounding), lam_min, dM (bound on ||M_r - M||),
    abs (bound on ||M_r^{1/2} psi - M^{1/2} psi||) and rel = abs / ||ref||."""
    M = dense_mreal(oracle, pos, box, xi, rcut, rounded=False)
    ref, lam = sqrt_apply(M, psi)
    dM = operator_bound(pos, box, xi, rcut, extra_pair=extra_pair, vector_rows=vector_rows)
    a = sqrt_bound(dM, lam) * np.linalg.norm(psi)
    return dict(M=M, ref=ref, lam_min=lam, dM=dM, abs=a, rel=a / np.linalg.norm(ref))


def _pair_sites(rng, k, box, spacing):
    """k sites in the box, at least `spacing` apart (minimum image): one pair is placed at each, so pairs do not see each other."""
    from oracle import pse_port
    out = []
    while len(out) < k:
        p = (rng.uniform(-0.5, 0.5, 3)) * np.array(box[:3])
        p[0] += box[3] * p[1]
        if all(np.linalg.norm(pse_port.min_image(p - q, box)) > spacing for q in out):
            out.append(p)
    return np.array(out)


def _with_partners(sites, seps, box):
    from oracle import pse_port
    pos = np.concatenate([sites, sites + np.asarray(seps)])
    return pse_port.wrap(pos, np.zeros(pos.shape, dtype=np.int64), box)[0]


def _spheres(rng, n, box, dmin=2.0):
    """n positions at least dmin apart (minimum image; rejection sampling): a suspension without overlaps."""
    from oracle import pse_port
    out = np.zeros((0, 3))
    while len(out) < n:
        p = rng.uniform(-0.5, 0.5, 3) * np.array(box[:3])
        p[0] += box[3] * p[1]
        if len(out) == 0 or np.linalg.norm(pse_port.min_image(out - p, box), axis=1).min() >= dmin:
            out = np.concatenate([out, p[None]])
    return out


def geometries():
    """The placements where the packing of the records goes wrong, N <= 200 (dense matrices on the CPU); dicts of name, pos, box, xi,
    error, rcut = sqrt(-ln error) / xi.  Shared by tests/test_record_bound.py (against the restatement) and
    tests/test_gpu_lanczos_truth.py (the device against the un-rounded operator)."""
    rng = np.random.default_rng(2024)
    out = []

    def add(name, pos, box, xi, error):
        out.append(dict(name=name, pos=np.ascontiguousarray(pos, float), box=tuple(float(b) for b in box), xi=float(xi),
                        error=float(error), rcut=math.sqrt(-math.log(error)) / xi))

    rc = math.sqrt(-math.log(1e-3)) / 0.5
    box = (48.0, 48.0, 48.0, 0.0)
    # (a) pairs along one axis: two components of s exactly 0 (separations 0.5 .. 2 .. rcut along x, y and z)
    seps = []
    for k, r in enumerate(np.concatenate([np.linspace(0.5, 2.0, 7), np.linspace(2.2, rc * 0.99, 14)])):
        d = np.zeros(3); d[k % 3] = r * (-1) ** k
        seps.append(d)
    add("a: along one axis", _with_partners(_pair_sites(rng, len(seps), box, 2 * rc + 1), seps, box), box, 0.5, 1e-3)
    # (b) one component 1e-9 .. 1e-4 of the others: the shared exponent flushes or truncates it
    seps = []
    for k, tiny in enumerate(np.repeat([1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4], 4)):
        u = rng.normal(size=3); u[k % 3] = tiny * np.abs(u).max() * (-1) ** k
        seps.append((1.0 + 0.17 * k) * u / np.linalg.norm(u))
    add("b: one component tiny", _with_partners(_pair_sites(rng, len(seps), box, 2 * rc + 1), seps, box), box, 0.5, 1e-3)
    # (c) overlapping pairs (small g - f), r = 1e-3 .. 2, and the touching distance; the touching pairs alone
    rs = np.concatenate([np.geomspace(1e-3, 2.0, 20), [2.0, 2.0]])
    seps = [r * u / np.linalg.norm(u) for r, u in zip(rs, rng.normal(size=(len(rs), 3)))]
    add("c: overlapping, r = 1e-3 .. 2", _with_partners(_pair_sites(rng, len(seps), box, 2 * rc + 1), seps, box), box, 0.5, 1e-3)
    rs = np.concatenate([np.linspace(0.5, 2.0, 12), [2.0] * 8])
    seps = [r * u / np.linalg.norm(u) for r, u in zip(rs, rng.normal(size=(len(rs), 3)))]
    add("c: overlapping, r = 0.5 .. 2, touching", _with_partners(_pair_sites(rng, len(seps), box, 2 * rc + 1), seps, box), box, 0.5, 1e-3)
    # (d) just inside rcut, where f and h are tiny
    seps = [rc * (1 - 1e-9) * u / np.linalg.norm(u) for u in rng.normal(size=(20, 3))]
    add("d: rcut (1 - 1e-9)", _with_partners(_pair_sites(rng, len(seps), box, 2 * rc + 1), seps, box), box, 0.5, 1e-3)
    # (e) pairs reached only through the tilted image (across the y faces of boxes with xy = +-0.5), in a non-cubic box, + a suspension
    for xy in (0.5, -0.5):
        box = (36.0, 30.0, 42.0, xy)
        sites = _pair_sites(rng, 12, box, 2 * rc + 1)
        sites[:, 1] = 0.5 * box[1] - rng.uniform(0.05, 1.5, len(sites))           # near the +y face: the partner lies across it
        sites[:, 0] = rng.uniform(-0.5, 0.5, len(sites)) * box[0] + xy * sites[:, 1]
        seps = [np.array([rng.uniform(-1, 1), 1.0, rng.uniform(-1, 1)]) * rng.uniform(1.6, 3.0) for _ in range(len(sites))]
        seps = [s * min(1.0, 0.99 * rc / np.linalg.norm(s)) for s in seps]
        add(f"e: tilted image xy = {xy:+.1f}", _with_partners(sites, seps, box), box, 0.5, 1e-3)
    box = (15.0, 12.0, 13.0, 0.5)
    add("e: suspension, box 15 x 12 x 13, xy = +0.5", _spheres(rng, 60, box), box, 0.5, 1e-3)
    # (f) xi across 0.2 .. 2 (and 10): at large xi f is small next to the self term, the fixed-point fr loses relative accuracy
    for xi, n, L, dmin in ((0.2, 40, 30.0, 2.0), (0.5, 60, 14.0, 2.0), (1.0, 40, 10.0, 2.0), (2.0, 50, 7.0, 1.2)):
        box = (L, L, L, 0.0)
        add(f"f: xi = {xi}", _spheres(rng, n, box, dmin), box, xi, 1e-3)
    box = (6.0, 6.0, 6.0, 0.0)
    rs = np.linspace(0.05, 0.25, 16)
    seps = [r * u / np.linalg.norm(u) for r, u in zip(rs, rng.normal(size=(len(rs), 3)))]
    add("f: xi = 10 (overlapping pairs)", _with_partners(_spheres(rng, len(rs), box, 1.0), seps, box), box, 10.0, 1e-3)
    # (g) h = (g - f) / r^2 < 0 inside the cutoff: xi = 2, error = 1e-6 (1.54 < r < rcut = 1.86), pairs placed there + a suspension
    box = (20.0, 20.0, 20.0, 0.0)
    seps = [r * u / np.linalg.norm(u) for r, u in zip(np.linspace(1.0, 1.858, 24), rng.normal(size=(24, 3)))]
    add("g: h < 0 (xi = 2, error = 1e-6)", _with_partners(_pair_sites(rng, len(seps), box, 4.0), seps, box), box, 2.0, 1e-6)
    box = (8.0, 8.0, 8.0, 0.0)
    add("g: suspension (xi = 2, error = 1e-6)", _spheres(rng, 50, box, 1.6), box, 2.0, 1e-6)
    return out
