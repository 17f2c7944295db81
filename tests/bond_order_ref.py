"""O(N^2) NumPy reference of the bond-orientational order (pse_bond_order_compute), shared by tests/test_bond_order_cpu.py (which
validates it) and tests/test_gpu_bond_order.py (which compares the device to it).

Over the ordered pairs (i, j) with minimum-image separation d = r_j - r_i (oracle.pse_port.min_image), r = |d| > 0, that `excl` keeps:
j is a NEIGHBOUR of i when r < rnb[p], p = p(type_i, type_j) as in cluster_ref; rnb[p] = 0 switches p off.  With the semi-normalised
harmonics C_lm = sqrt(4 pi/(2l + 1)) Y_lm from scipy.special.sph_harm_y (Condon-Shortley phase), m = 0..l:
  c_lm(i) = mean_j C_lm(d_ij/r)  (0 without neighbours),   q_l = sqrt(|c_l0|^2 + 2 sum_{m>0} |c_lm|^2),
  cbar_lm(i) = (c_lm(i) + sum_{j in nb(i)} c_lm(j))/(nb(i) + 1),   qbar_l its norm,
  s_ij = Re sum_{m=-l..l} c_lm(i) conj c_lm(j)/(q_l(i) q_l(j)) for the solid degree (0 where a q is 0), n_conn(i) = #{j: s_ij > threshold},
  stats[a] = (members of type a, those with n_conn >= min_conn).

The integers (nnb, n_conn, stats) of two correct implementations can differ only for a pair at the edge of rnb or a bond at the edge of
the threshold: the clearance report says how far the input stays from both, and every test asserts CLEAR before it compares.

The second half restates, in plain float64 NumPy, the arithmetic the device kernel uses for one term C_lm(d) (kernel_terms), and derives
the bound on its error from the order of the operations (term_bound, bound): that bound is the tolerance of the GPU tests.
Not a test module: nothing here is collected."""
import functools

import numpy as np

import exclusion_ref
from cluster_ref import pair_types, rlink_array

CLEAR = 1e-9
U = 2.0 ** -53            # unit roundoff of float64
DEGREES = (2, 4, 6, 8, 10, 12)


# ---- the reference ------------------------------------------------------------------------------------------------------------------

def harmonics(d, l):
    """C_lm(d/|d|), m = 0..l, for separation vectors d (n, 3): (n, l + 1) complex."""
    from scipy.special import sph_harm_y
    d = np.asarray(d, dtype=float).reshape(-1, 3)
    theta = np.arctan2(np.hypot(d[:, 0], d[:, 1]), d[:, 2])     # (well conditioned at the poles, where arccos(z/r) is not)
    phi = np.arctan2(d[:, 1], d[:, 0])
    m = np.arange(l + 1)
    return np.sqrt(4.0 * np.pi / (2 * l + 1)) * sph_harm_y(l, m[None, :], theta[:, None], phi[:, None])


def norm(c):
    """sqrt(|c_0|^2 + 2 sum_{m>0} |c_m|^2) along the last axis."""
    a = np.abs(c) ** 2
    return np.sqrt(a[..., 0] + 2.0 * a[..., 1:].sum(axis=-1))


def shell_q(vectors, l):
    """q_l of one particle whose neighbours sit at `vectors`."""
    return float(norm(harmonics(vectors, l).mean(axis=0)))


def neighbours(pos, box, types, ntypes, rnb, port, excl=None, ids=None):
    """((i, j, d) of the ordered neighbour pairs, d = r_j - r_i; the least |r - rnb[p]| over all pairs of a pair type that is on; the
    least r of a neighbour pair)."""
    pos = np.asarray(pos, dtype=float)
    n = len(pos)
    types = np.zeros(n, dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    rn = rlink_array(rnb, ntypes)
    i, j = np.nonzero(~np.eye(n, dtype=bool))
    d = port.min_image(pos[j] - pos[i], box)
    r = np.sqrt((d * d).sum(axis=1))
    keep = exclusion_ref.kept_mask(i, j, excl, ids) & (r > 0.0)
    i, j, d, r = i[keep], j[keep], d[keep], r[keep]
    cut = rn[pair_types(types, i, j, ntypes)] if len(i) else np.zeros(0)
    on = cut > 0.0
    clear = float(np.abs(r[on] - cut[on]).min()) if on.any() else np.inf
    m = r < cut
    return (i[m], j[m], d[m]), clear, (float(r[m].min()) if m.any() else np.inf)


def bond_order(pos, box, types, ntypes, rnb, degrees, port, excl=None, ids=None, solid=None):
    """The whole reference in one call.  solid = (degree, threshold, min_conn) or None.  Returns a dict: nnb (n,), c {l: (n, l + 1)
    complex}, q and qbar (n, nl), s {(i, j): s_ij} and nconn (n,) with a solid pass (else None), stats (ntypes, 2), clear = (distance
    clearance, threshold clearance), rmin (the shortest bond), nbmax."""
    n = len(pos)
    ty = np.zeros(n, dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    (i, j, d), clear_r, rmin = neighbours(pos, box, types, ntypes, rnb, port, excl, ids)
    nnb = np.bincount(i, minlength=n).astype(np.int64)
    out = dict(nnb=nnb, c={}, q=np.zeros((n, len(degrees))), qbar=np.zeros((n, len(degrees))), s=None, nconn=None, rmin=rmin,
               nbmax=int(nnb.max()) if n else 0)
    for col, l in enumerate(degrees):
        c = np.zeros((n, l + 1), dtype=complex)
        if len(i):
            np.add.at(c, i, harmonics(d, l))
        c[nnb > 0] /= nnb[nnb > 0, None]
        cbar = c.copy()
        if len(i):
            np.add.at(cbar, i, c[j])
        cbar /= (nnb + 1)[:, None]
        out["c"][l], out["q"][:, col], out["qbar"][:, col] = c, norm(c), norm(cbar)
    stats = np.zeros((ntypes, 2), dtype=np.int64)
    stats[:, 0] = np.bincount(ty, minlength=ntypes)
    clear_s = np.inf
    if solid is not None:
        l, threshold, min_conn = solid
        c, q = out["c"][l], out["q"][:, list(degrees).index(l)]
        dot = (c[i, 0] * np.conj(c[j, 0])).real + 2.0 * (c[i, 1:] * np.conj(c[j, 1:])).real.sum(axis=1)
        den = q[i] * q[j]
        s = np.where(den > 0.0, dot / np.where(den > 0.0, den, 1.0), 0.0)
        out["s"] = {(int(a), int(b)): float(v) for a, b, v in zip(i, j, s)}
        out["nconn"] = np.bincount(i[s > threshold], minlength=n).astype(np.int64)
        stats[:, 1] = np.bincount(ty[out["nconn"] >= min_conn], minlength=ntypes)
        clear_s = float(np.abs(s - threshold).min()) if len(s) else np.inf
    out["stats"], out["clear"] = stats, (clear_r, clear_s)
    return out


def assert_clear(clear):
    assert min(clear) >= CLEAR, ("a pair within 1e-9 of its neighbour distance or a bond within 1e-9 of the threshold: change the input", clear)


def histogram(values, types, ntypes, nbins, lo, hi):
    """counts (ntypes, nbins) of the binning formula of pse_bond_order_histogram applied to `values` (n,), in its order of operations."""
    values, types = np.asarray(values, dtype=np.float64), np.asarray(types, dtype=np.int64)
    counts = np.zeros((ntypes, nbins), dtype=np.int64)
    m = (values >= lo) & (values < hi)
    b = np.minimum(((values[m] - lo) * float(nbins) / (hi - lo)).astype(np.int64), nbins - 1)
    np.add.at(counts, (types[m], b), 1)
    return counts


# ---- the kernel's arithmetic, restated ------------------------------------------------------------------------------------------------

def coef_a(l, m):
    return (2 * l - 1) / np.sqrt(float((l - m) * (l + m)))


def coef_b(l, m):
    return np.sqrt(float((l - 1 - m) * (l - 1 + m)) / float((l - m) * (l + m)))


def start(m):
    """T_m^m = (-1)^m sqrt((2m - 1)!!/(2m)!!), formed as the kernel's constant is."""
    p = 1.0
    for k in range(1, m + 1):
        p *= (2 * k - 1) / (2 * k)
    return -np.sqrt(p) if m & 1 else np.sqrt(p)


def legendre_row(z, L):
    """T_L^m(z), m = 0..L, by the upward recurrence in l: (len(z), L + 1)."""
    z = np.asarray(z, dtype=np.float64)
    out = np.empty(z.shape + (L + 1,))
    for m in range(L + 1):
        p2 = np.full(z.shape, start(m))
        if m == L:
            out[..., m] = p2
            continue
        p1 = (coef_a(m + 1, m) * z) * p2
        for l in range(m + 2, L + 1):
            p1, p2 = (coef_a(l, m) * z) * p1 - coef_b(l, m) * p2, p1
        out[..., m] = p1
    return out


def kernel_terms(d, L):
    """C_Lm(d/|d|), m = 0..L, as the device forms one term: r^2, one square root and one division, T_L^m(z) by the recurrence and
    (x + i y)^m by repeated multiplication -- float64 throughout (NumPy does not fuse; the device's fused operations round less)."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    ir = 1.0 / np.sqrt(r2)
    x, y, z = d[:, 0] * ir, d[:, 1] * ir, d[:, 2] * ir
    t = legendre_row(z, L)
    out = np.empty((len(d), L + 1), dtype=complex)
    wx, wy = np.ones(len(d)), np.zeros(len(d))
    for m in range(L + 1):
        out[:, m] = t[:, m] * wx + 1j * (t[:, m] * wy)
        wx, wy = wx * x - wy * y, wx * y + wy * x
    return out


# ---- the bound, from the order of the operations ---------------------------------------------------------------------------------------
# One term C_Lm = T_L^m(z) w^m, w = x + i y, |w| = s = sin(theta).  In units of u = 2^-53, with p_l the exact T_l^m:
#   start      T_m^m: m quotients, m products, a square root within an ulp            e_m     = (m + 2) |p_m|
#   first step (a z) p: a within 2 ulp (root, quotient), two products                 e_{m+1} = |a z| e_m + 4 |a z p_m|
#   step       fma(a z, p1, -(b p2)): a and b within 2 ulp, a z, b p2, the fma        e_l     = |a z| e_{l-1} + b e_{l-2} + 4 (|a z p_{l-1}| + |b p_{l-2}|)
#   power      w^m from m - 1 complex products of two products and a sum each         f_m     = 3 m s^m
#   the term   |delta C_Lm| <= s^m e_L + |p_L| f_m
# term_units(L) is the largest value of that over m and a grid of z.  The direction itself carries the normalisation -- r^2 from three
# products and two sums, a root, a quotient, a product: 6 u per component -- and whatever the two implementations differ by in the
# separation vector (dpos: an absolute error over the shortest bond); a polynomial of degree L bounded by 1 on the sphere moves by at
# most (L + 1)^2 per unit of that (Markov).  A sum of nb terms of modulus <= 1 adds (nb - 1) u nb/nb, the division by nb two roundings.

@functools.lru_cache(maxsize=None)
def term_units(L):
    z = np.concatenate([np.linspace(-1.0, 1.0, 4001), [0.999999, -0.999999]])
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    worst = 0.0
    for m in range(L + 1):
        p2 = np.full(z.shape, abs(start(m)))
        e2 = (m + 2) * p2
        if m == L:
            p1, e1 = p2, e2
        else:
            az = np.abs(coef_a(m + 1, m) * z)
            sg2 = np.full(z.shape, start(m))
            sg1 = (coef_a(m + 1, m) * z) * sg2
            p1, e1 = np.abs(sg1), az * e2 + 4.0 * az * p2
            for l in range(m + 2, L + 1):
                a, b = coef_a(l, m), coef_b(l, m)
                az = np.abs(a * z)
                e1, e2 = az * e1 + b * e2 + 4.0 * (az * np.abs(sg1) + b * np.abs(sg2)), e1
                sg1, sg2 = (a * z) * sg1 - b * sg2, sg1
            p1 = np.abs(sg1)
        worst = max(worst, float((s ** m * (e1 + 3.0 * m * p1)).max()))
    return worst


def term_bound(L, dpos=0.0):
    """|delta C_Lm| of one term, per real component; dpos: the absolute error of the separation vector over the shortest bond."""
    return term_units(L) * U + (L + 1) ** 2 * (6.0 * U + dpos)


def bound(L, nbmax, dpos=0.0, averaged=False):
    """The tolerance of q_L (averaged: of qbar_L): the norm of 2L + 1 complex errors of c_lm, each sqrt(2) times the per-component error
    term_bound + (nb + 2) u of the mean (one more sum of nb + 1 rows and a division for cbar), plus the L + 4 roundings of the norm."""
    c = term_bound(L, dpos) + (nbmax + 2) * U
    if averaged:
        c += (nbmax + 3) * U
    return np.sqrt(2.0 * (2 * L + 1)) * c + (L + 4) * U


def c_bound(L, nbmax, dpos=0.0):
    """The tolerance of one complex c_lm."""
    return np.sqrt(2.0) * (term_bound(L, dpos) + (nbmax + 2) * U)


def separation_error(box, rmin):
    """dpos of two float64 minimum images of one pair: each rounds a handful of times at the scale of the box, 4 u L apiece."""
    return 8.0 * U * max(box[:3]) / rmin


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

SHELLS = {
    "sc": np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=float),
    "fcc": np.array([[a, b, 0] for a in (1, -1) for b in (1, -1)] + [[a, 0, b] for a in (1, -1) for b in (1, -1)]
                    + [[0, a, b] for a in (1, -1) for b in (1, -1)], dtype=float),
    "bcc8": np.array([[a, b, c] for a in (1, -1) for b in (1, -1) for c in (1, -1)], dtype=float),
}
SHELLS["bcc14"] = np.concatenate([SHELLS["bcc8"], 2.0 * SHELLS["sc"]])
_h, _c = np.sqrt(3.0) / 2.0, np.sqrt(2.0 / 3.0)     # hcp, ideal c/a: six in the plane, three above and three below, the same triangle
SHELLS["hcp"] = np.array([[1, 0, 0], [-1, 0, 0], [0.5, _h, 0], [-0.5, _h, 0], [0.5, -_h, 0], [-0.5, -_h, 0]]
                         + [[0.5, _h / 3, s * _c] for s in (1, -1)] + [[-0.5, _h / 3, s * _c] for s in (1, -1)]
                         + [[0.0, -2 * _h / 3, s * _c] for s in (1, -1)])


def sc_lattice(k, a):
    """k^3 sites of a simple cubic lattice of spacing a, centred on the origin: fills a periodic box of side k a."""
    g = np.arange(k)
    idx = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return (idx + 0.5) * a - 0.5 * k * a


def fcc_lattice(k, a):
    """4 k^3 sites of an fcc lattice of cubic cell a, centred: fills a periodic box of side k a."""
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    g = np.arange(k)
    idx = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    return ((idx + basis[None]).reshape(-1, 3) + 0.25) * a - 0.5 * k * a
