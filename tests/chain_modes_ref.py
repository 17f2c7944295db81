"""Reference for the chain normal modes (pse_chain_modes_compute, pse_chain_modes_correlate, analyze.RouseModes) in exact arithmetic:
the layout and the unfolding are those of conformation_ref.py and chain_stats_ref.py -- plain Python, rational, independent of the
library's --, every float64 weight is taken as the rational it is, X, the static sums and the correlations are exact integer sums over a
common power-of-two denominator, and a result is rounded to float64 once, at the end.  Also: the test that a set of dyadic inputs is
summed without any rounding in ANY order, a float64 restatement of the kernels' documented order (chunks of 16, the per-tile and
per-block orders, the lanes and the xor butterfly, every fma emulated exactly), and the error bound of the kernels."""
import functools
import math
from fractions import Fraction

import numpy as np

import conformation_cases as cc
from chain_stats_ref import exact_offsets, ranks_of
from conformation_ref import layout, tiles_of

EPS = cc.EPS
CHUNK = 16      # ranks of one chunk of the projection
BLOCK = 256     # linear molecules of one wave of the correlation pass
COLS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def gamma(n):
    return n * EPS / (1.0 - n * EPS)


def fma(a, b, c):
    """The correctly rounded a b + c of three float64 (float() of a Fraction rounds to nearest, ties to even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chains(n, bonds):
    """(mols, linear): the layout of conformation_ref and, for every LINEAR molecule in ascending molecule number, a dict with mol,
    size and order: the breadth-first positions of its members in rank order (rank 0: the end with the lower caller index)."""
    mols, _ = layout(n, bonds)
    ranks = ranks_of(n, bonds, mols)
    lin = [dict(mol=k, size=len(rk), order=np.argsort(rk)) for k, (mo, rk) in enumerate(zip(mols, ranks)) if mo["ends"] is not None]
    return mols, lin


@functools.lru_cache(maxsize=None)
def rouse_weights(m, K):
    """The weights that pse_host_rouse_weights documents, from mpmath at 40 digits, rounded once: the comparison of the CPU test."""
    import mpmath
    mpmath.mp.dps = 40
    w = np.zeros((K, m))
    w[0, 0], w[0, m - 1] = -1.0, 1.0
    for p in range(1, K):
        for q in range(m):
            if (p * (2 * q + 1)) % (2 * m) != m:                                # (an odd multiple of pi / 2: exactly 0)
                w[p, q] = float(mpmath.cos(mpmath.pi * p * (2 * q + 1) / (2 * m)) / m)
    return w


def dyadic_weights(m, K, rng):
    """K rows of multiples of 1/2 in [-1, 1]; row 0 the end-to-end functional."""
    w = rng.integers(-2, 3, (K, m)) / 2.0
    w[0] = 0.0
    w[0, 0], w[0, m - 1] = -1.0, 1.0
    return w


def _ints(w):
    """A float64 array as Python integers over a common power-of-two denominator: (object array, denominator)."""
    fr = [Fraction(float(x)) for x in np.asarray(w).ravel()]
    den = max(f.denominator for f in fr)
    return np.array([int(f * den) for f in fr], dtype=object).reshape(np.shape(w)), den


def _headroom(terms):
    """sum |t| / g for integer terms t whose greatest common divisor is g: below 2^53, every partial sum in every order is a multiple
    of g of fewer than 53 bits, so float64 adds (and fused multiply-adds) round nothing."""
    terms = [abs(int(t)) for t in terms if t != 0]
    if not terms:
        return 0
    return sum(terms) // math.gcd(*terms)


def reference(pos, box, bonds, tables, mol_types=None, ntypes=1, dyadic=False):
    """Everything pse_chain_modes_compute writes in one call from zeroed outputs, rounded once: modes (nlin, K, 3), sums (ntypes, K, 6)
    -- `sample` is the same --; and beside them X (the exact modes as integers, (nlin, K, 3) objects) over `den`, lin_mol, lin_size,
    lin_type, nlin_type, absx = sum_q |w_q| |u_q| and wsum = sum_q |w_q| (floats, for the bound), umax and size per linear molecule.
    `tables`: {m: (K, m) float64 weights}.  dyadic=True ASSERTS that no sum of the call can round in any order (_headroom)."""
    pos = np.asarray(pos, dtype=np.float64)
    mols, lin = chains(pos.shape[0], bonds)
    us, scale = exact_offsets(pos, box, mols)
    K = next(iter(tables.values())).shape[0]
    wi = {m: _ints(w) for m, w in tables.items()}
    wden = max(d for _, d in wi.values())
    den = scale * wden
    nlin = len(lin)
    X = np.zeros((nlin, K, 3), dtype=object)
    absx, wsum, umax = np.zeros((nlin, K, 3)), np.zeros((nlin, K)), np.zeros(nlin)
    head = 0
    for j, ch in enumerate(lin):
        m = ch["size"]
        assert tables[m].shape == (K, m)
        w, d = wi[m]
        u = us[ch["mol"]][ch["order"]]                      # (m, 3) integers over `scale`, in rank order
        up = wden // d
        for k in range(K):
            for c in range(3):
                terms = [int(w[k, q]) * int(u[q, c]) * up for q in range(m)]
                X[j, k, c] = sum(terms)
                absx[j, k, c] = float(Fraction(sum(abs(t) for t in terms), den))
                head = max(head, _headroom(terms)) if dyadic else 0
            wsum[j, k] = float(np.abs(tables[m][k]).sum())
        umax[j] = max(abs(int(v)) for v in u.ravel()) / scale
    lin_type = np.array([0 if mol_types is None else int(mol_types[ch["mol"]]) for ch in lin])
    exact = np.zeros((ntypes, K, 6), dtype=object)
    for a in range(ntypes):
        for k in range(K):
            for c, (i, b) in enumerate(COLS):
                terms = [int(X[j, k, i]) * int(X[j, k, b]) for j in range(nlin) if lin_type[j] == a]
                exact[a, k, c] = sum(terms)
                head = max(head, _headroom(terms)) if dyadic else 0
    if dyadic:
        assert head < 2 ** 53, f"the inputs are not summed exactly in every order: a sum needs {head.bit_length()} bits"
    rnd = np.vectorize(lambda v, d: float(Fraction(int(v), d)), otypes=[np.float64])
    return dict(modes=rnd(X, den), sums=rnd(exact, den * den), X=X, den=den, lin_mol=np.array([ch["mol"] for ch in lin]),
                lin_size=np.array([ch["size"] for ch in lin]), lin_type=lin_type, nlin_type=np.bincount(lin_type, minlength=ntypes),
                absx=absx, wsum=wsum, umax=umax, mols=mols, headroom=head, K=K)


def correlate(now, then, ntypes, dyadic=False):
    """(ntypes, K, 3, 3): [a, k, alpha, beta] = the exact sum over the linear molecules of type a of X_alpha(now) X_beta(then), rounded
    once; `now`, `then`: two reference() results of one topology."""
    nlin, K = now["X"].shape[:2]
    out = np.zeros((ntypes, K, 3, 3))
    den = now["den"] * then["den"]
    head = 0
    for a in range(ntypes):
        js = [j for j in range(nlin) if now["lin_type"][j] == a]
        for k in range(K):
            for al in range(3):
                for be in range(3):
                    terms = [int(now["X"][j, k, al]) * int(then["X"][j, k, be]) for j in js]
                    out[a, k, al, be] = float(Fraction(sum(terms), den))
                    head = max(head, _headroom(terms)) if dyadic else 0
    if dyadic:
        assert head < 2 ** 53, f"the correlation is not summed exactly in every order: a sum needs {head.bit_length()} bits"
    return out


# ---- the kernels' order of operations, restated in float64 ---------------------------------------------------------------------------
def unfold_float(pos, box, mols):
    """Per molecule the offsets u (m, 3) in breadth-first order as conformation_ref.kernel_order unfolds them: the device's minimum
    image and the pointer jumping of the molecule's tile."""
    Lx, Ly, Lz, xy = (float(v) for v in box)
    first, rounds = tiles_of(mols)
    out = []
    for k, mo in enumerate(mols):
        mem, par = np.array(mo["members"]), np.array(mo["parent"])
        d = pos[mem, :3] - pos[mem[par], :3]
        ny = np.rint(d[:, 1] * (1.0 / Ly)); d[:, 1] -= ny * Ly; d[:, 0] -= ny * xy * Ly
        d[:, 0] -= np.rint(d[:, 0] * (1.0 / Lx)) * Lx
        d[:, 2] -= np.rint(d[:, 2] * (1.0 / Lz)) * Lz
        d[0] = 0.0
        u, anc = d.copy(), par.copy()
        tile = max(t for t in range(len(rounds)) if first[t] <= k)
        for _ in range(rounds[tile]):
            u, anc = u + u[anc], anc[anc]
        out.append(u)
    return out


def project(w, u):
    """X (K, 3) of one chain in the documented order: chunks of 16 ranks, within a chunk ascending q with one fma each from +0.0, then
    the chunks in ascending order from +0.0."""
    K, m = w.shape
    X = np.zeros((K, 3))
    for k in range(K):
        for c in range(3):
            x = 0.0
            for q0 in range(0, m, CHUNK):
                acc = 0.0
                for q in range(q0, min(q0 + CHUNK, m)):
                    acc = fma(float(w[k, q]), float(u[q, c]), acc)
                x += acc
            X[k, c] = x
    return X


def _lanes(part):
    """The finishing order of k_mol_finish over the rows of part (nrows, ncol): lane l of 64 adds the rows l, l + 64, ... in ascending
    order, then the xor butterfly."""
    lanes = np.zeros((64,) + part.shape[1:])
    for t in range(part.shape[0]):
        lanes[t % 64] += part[t]
    o = 32
    while o > 0:
        lanes = lanes + lanes[np.arange(64) ^ o]
        o //= 2
    return lanes[0]


def kernel_order(pos, box, bonds, tables, mol_types=None, ntypes=1):
    """(modes (nlin, K, 3), sums (ntypes, K, 6)) as the kernels compute them, in float64 with their order of operations."""
    pos = np.asarray(pos, dtype=np.float64)
    mols, lin = chains(pos.shape[0], bonds)
    us = unfold_float(pos, box, mols)
    K = next(iter(tables.values())).shape[0]
    modes = np.array([project(tables[ch["size"]], us[ch["mol"]][ch["order"]]) for ch in lin])
    first, _ = tiles_of(mols)
    part = np.zeros((len(first) - 1, ntypes, K, 6))
    for j, ch in enumerate(lin):
        t = max(t for t in range(len(first) - 1) if first[t] <= ch["mol"])
        a = 0 if mol_types is None else int(mol_types[ch["mol"]])
        for k in range(K):
            for c, (i, b) in enumerate(COLS):
                part[t, a, k, c] = fma(modes[j, k, i], modes[j, k, b], part[t, a, k, c])
    return modes, _lanes(part)


def kernel_correlate(now, then, lin_type, ntypes):
    """(ntypes, K, 3, 3) from two float64 mode arrays (nlin, K, 3) in the order of k_modes_corr and its finishing kernel: blocks of 256
    molecules, lane l takes j0 + l, + 64, + 128, + 192 with one fma each from +0.0, the xor butterfly, then the blocks lane by lane."""
    nlin, K = now.shape[:2]
    nblk = -(-nlin // BLOCK)
    part = np.zeros((nblk, ntypes, K, 3, 3))
    for b in range(nblk):
        lanes = np.zeros((64, ntypes, K, 3, 3))
        for i in range(BLOCK // 64):
            for l in range(64):
                j = b * BLOCK + i * 64 + l
                if j >= nlin:
                    continue
                a = int(lin_type[j])
                for k in range(K):
                    for al in range(3):
                        for be in range(3):
                            lanes[l, a, k, al, be] = fma(now[j, k, al], then[j, k, be], lanes[l, a, k, al, be])
        o = 32
        while o > 0:
            lanes = lanes + lanes[np.arange(64) ^ o]
            o //= 2
        part[b] = lanes[0]
    return _lanes(part)


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------
def bounds(ref, box):
    """tX (nlin, K, 3): the absolute error bound of the kernel's X against the once-rounded exact value.  With du = 16 m EPS S the
    bound of conformation_cases.bounds on a component of an unfolded offset (S = max(U, Lmax)), the computed offsets are u + delta,
    |delta| <= du.  The projection runs every term through at most min(m, 16) fused multiply-adds of its chunk and at most
    ceil(m / 16) additions of chunks, together at most m + 2 roundings, so (Higham, Accuracy and Stability, 3.1)
      |X_hat - sum w (u + delta)| <= gamma_{m+2} sum |w| (|u| + du),   |sum w delta| <= du sum |w|,
    and the reference's own rounding adds EPS |X|:   tX = gamma_{m+2} (absx + du wsum) + du wsum + EPS |X|."""
    Lmax = max(box[:3])
    S = np.maximum(ref["umax"], Lmax)
    m = ref["lin_size"].astype(np.float64)
    du = (16.0 * m * EPS * S)[:, None, None]
    g = (gamma(ref["lin_size"] + 2.0))[:, None, None]
    ws = ref["wsum"][:, :, None]
    return g * (ref["absx"] * (1.0 + 2.0 ** -40) + du * ws) + du * ws + EPS * np.abs(ref["modes"])


def product_bound(xa, ta, xb, tb):
    """|xa_hat xb_hat - xa xb| for |xa_hat - xa| <= ta, |xb_hat - xb| <= tb: the product rule."""
    return np.abs(xa) * tb + np.abs(xb) * ta + ta * tb


def sums_bound(ref, tX, ntypes, ntiles):
    """(ntypes, K, 6): the bound of the static sums.  Every term X_a X_b carries product_bound; the additions -- at most 512 fused
    multiply-adds within a tile, ceil(ntiles / 64) additions in a lane of the finishing kernel and 6 levels of its butterfly, and the
    one addition to `sums` -- add gamma_n of the sum of the terms' sizes, n = 519 + ceil(ntiles / 64); the reference's rounding EPS |sum|."""
    X = ref["modes"]
    n = 519 + -(-ntiles // 64)
    out = np.zeros((ntypes,) + X.shape[1:2] + (6,))
    for a in range(ntypes):
        sel = ref["lin_type"] == a
        for c, (i, b) in enumerate(COLS):
            pb = product_bound(X[sel, :, i], tX[sel, :, i], X[sel, :, b], tX[sel, :, b])
            size = (np.abs(X[sel, :, i]) + tX[sel, :, i]) * (np.abs(X[sel, :, b]) + tX[sel, :, b])
            out[a, :, c] = pb.sum(axis=0) + gamma(n) * size.sum(axis=0) + EPS * np.abs(ref["sums"][a, :, c])
    return out


def correlate_bound(now, t_now, then, t_then, ntypes, exact):
    """(ntypes, K, 3, 3): the bound of one correlation against `exact` (correlate()).  Every term carries product_bound; the additions
    -- 4 fused multiply-adds in a lane, 6 levels of the butterfly, ceil(nblocks / 64) additions and 6 levels in the finishing kernel,
    and the one addition to corr -- add gamma_n of the sum of the terms' sizes, n = 17 + ceil(nblocks / 64)."""
    X, Y = now["modes"], then["modes"]
    nblk = -(-X.shape[0] // BLOCK)
    n = 17 + -(-nblk // 64)
    out = np.zeros((ntypes, X.shape[1], 3, 3))
    for a in range(ntypes):
        sel = now["lin_type"] == a
        for al in range(3):
            for be in range(3):
                pb = product_bound(X[sel, :, al], t_now[sel, :, al], Y[sel, :, be], t_then[sel, :, be])
                size = (np.abs(X[sel, :, al]) + t_now[sel, :, al]) * (np.abs(Y[sel, :, be]) + t_then[sel, :, be])
                out[a, :, al, be] = pb.sum(axis=0) + gamma(n) * size.sum(axis=0) + EPS * np.abs(exact[a, :, al, be])
    return out


# ---- the cases that the GPU tests run and the CPU tests check first ---------------------------------------------------------------------
DYADIC_NAMES = ("shuffled chain", "1024 chain", "513 dimers", "2 64 256 1024", "four 64")   # the cases of cc.DYADIC with a linear molecule


def tables_for(n, bonds, K, make):
    """{m: make(m, K)} for the distinct sizes of the linear molecules."""
    _, lin = chains(n, bonds)
    return {m: make(m, K) for m in sorted({ch["size"] for ch in lin})}


def dyadic(name, K=5):
    box, n, bonds, pos, types, ntypes = cc.DYADIC[name]
    rng = np.random.default_rng(41)
    tables = tables_for(n, bonds, K, lambda m, k: dyadic_weights(m, k, rng))
    return box, n, bonds, pos, types, ntypes, tables


def padded_rouse(m, K):
    """Rouse weights for a chain that may be shorter than K: min(K, m) rows of rouse_weights and zero rows above, so that the tables
    of one object share one K."""
    w = np.zeros((K, m))
    w[:min(K, m)] = rouse_weights(m, min(K, m))
    return w


def edge(k, K=9):
    """The general-position cases of conformation_cases.EDGES -- sizes 2, 3, 63, 64, 65, 255, 257 and 1023, a star, rings and a comb, a
    tile of exactly 1024, 1, 2 and 8 types with empty ones -- with (padded) Rouse weights."""
    lengths, xy, ntypes, seed = cc.EDGES[k]
    box, n, bonds, pos, types = cc.edge_case(lengths, xy, ntypes, seed)
    return box, n, bonds, pos, types, ntypes, tables_for(n, bonds, K, padded_rouse)


def general(name):
    """The general-position cases beyond EDGES: "1024 and dimers" -- a 1024-bead chain, a tile of 512 dimers, then two sizes (20 and 7)
    and a ring in one tile, two types, K = 9; "K=32" and "K=1" -- chains of 40, 33 and 40 and a star, one type."""
    rng = np.random.default_rng(97)
    if name == "1024 and dimers":
        shapes, K, ntypes = [("chain", 1024)] + [("chain", 2)] * 512 + [("chain", 20), ("chain", 7), ("ring", 5), ("chain", 20)], 9, 2
    else:
        shapes, K, ntypes = [("chain", 40), ("chain", 33), ("chain", 40), ("star", 5)], {"K=32": 32, "K=1": 1}[name], 1
    n, bonds, sizes, kinds = cc.build(shapes, gaps=(1,))
    box = (16.0, 32.0, 16.0, 0.5)
    pos = cc.place(n, bonds, box, rng, 3.0)
    mols, _ = layout(n, bonds)
    for k, kind in enumerate(kinds):
        if kind == "ring":
            cc.ring_place(pos, mols[k]["members"][0], sizes[k], 1.5, rng)
    types = None if ntypes == 1 else np.arange(len(shapes)) % 2
    return box, n, bonds, cc.wrap(pos, box), types, ntypes, tables_for(n, bonds, K, padded_rouse)


GENERAL_NAMES = ("1024 and dimers", "K=32", "K=1")
