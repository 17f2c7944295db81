"""Reference for the chain statistics (pse_molecule_pairs_compute, analyze.ChainStatistics).  The layout and the minimum image are
conformation_ref's; the offsets u are exact rationals -- every float64 input is a dyadic rational, so all u of a case share a power of
two as denominator and are held as Python integers over it.  D(s), C(s) and `terms` are exact integers, rounded to float64 once.  The
inverse distances of H are taken to 128 bits behind the binary point (38 digits) by integer square roots and summed exactly as
integers; mpmath at 40 digits confirms the method in test_chain_stats_cpu.py.  A pair with r2 == 0 adds nothing.  Also: the rank of
every member, found from the bonds themselves; a NumPy float64 restatement of the kernel's order of operations; and the error bounds."""
import functools
import math
from fractions import Fraction

import numpy as np

import conformation_cases as cc
from conformation_ref import layout, min_image, tiles_of, _tree

EPS = cc.EPS
FBITS = 128   # bits behind the binary point of an inverse distance


def ranks_of(n, bonds, mols=None):
    """rank (list per molecule, by breadth-first position): along the chain from the end with the lower caller index for a linear
    molecule -- walked over the bonds, not over the spanning tree --, the breadth-first position otherwise."""
    if mols is None:
        mols, _ = layout(n, bonds)
    nb = {}
    for i, j in np.asarray(bonds).tolist():
        nb.setdefault(i, []).append(j); nb.setdefault(j, []).append(i)
    out = []
    for mo in mols:
        mem = mo["members"]
        if mo["ends"] is None:
            out.append(list(range(len(mem))))
            continue
        where = {i: p for p, i in enumerate(mem)}
        rank, prev, at = [0] * len(mem), None, mem[mo["ends"][0]]
        for r in range(len(mem)):
            rank[where[at]] = r
            nxt = [j for j in nb[at] if j != prev]
            prev, at = at, (nxt[0] if nxt else None)
        assert at is None and sorted(rank) == list(range(len(mem)))
        out.append(rank)
    return out


def exact_offsets(pos, box, mols):
    """Per molecule the exact offsets u of its members in breadth-first order, as integers over the common denominator `scale` (a
    power of two): (list of (m, 3) object arrays, scale)."""
    fbox = tuple(Fraction(float(v)) for v in box)
    P = {}
    us, scale = [], 1
    for mo in mols:
        mem = mo["members"]
        for i in mem:
            P[i] = [Fraction(float(v)) for v in pos[i, :3]]
        u = [[Fraction(0)] * 3]
        for p in range(1, len(mem)):
            d, _ = min_image([P[mem[p]][c] - P[mem[mo["parent"][p]]][c] for c in range(3)], fbox)
            u.append([u[mo["parent"][p]][c] + d[c] for c in range(3)])
        scale = max([scale] + [x[c].denominator for x in u for c in range(3)])
        us.append(u)
    assert scale & (scale - 1) == 0
    return [np.array([[int(x[c] * scale) for c in range(3)] for x in u], dtype=object) for u in us], scale


def inverse_root(r2, lg):
    """floor-accurate 2^FBITS / sqrt(r2 / 4^lg) for the positive integer r2: an integer, relative error below 2^-120."""
    q = math.isqrt(r2 << 256)                       # sqrt(r2) 2^128
    return (1 << (FBITS + 128 + lg)) // q


def reference(pos, box, bonds, mol_types=None, ntypes=1, ns=1):
    """Everything pse_molecule_pairs_compute writes in one call from zeroed outputs: inv_rh (nmol,), curves (ntypes, ns, 2), sums
    (ntypes, 2) -- `sample` is the same --, each rounded to float64 once; terms (ntypes, ns, 2) int64; and what the tests need beside
    them: inexact (how many entries of curves were rounded at all), hsum (nmol,): the sum of 1/r over the pairs, s3 (nmol,): the sum
    of 1/r^3, rmin: the smallest non-zero distance of two members of one molecule, nzero: the pairs at distance 0, npairs (nmol,),
    size, linear, umax (nmol,), mols, ranks."""
    pos = np.asarray(pos, dtype=np.float64)
    mols, _ = layout(pos.shape[0], bonds)
    ranks = ranks_of(pos.shape[0], bonds, mols)
    U, scale = exact_offsets(pos, box, mols)
    lg = scale.bit_length() - 1
    sc2 = scale * scale
    nmol = len(mols)
    curves = [[[0, 0] for _ in range(ns)] for _ in range(ntypes)]
    terms = np.zeros((ntypes, ns, 2), dtype=np.int64)
    inv = [Fraction(0)] * nmol
    hsum, s3, umax = np.zeros(nmol), np.zeros(nmol), np.zeros(nmol)
    rmin2, nzero = None, 0
    for k, mo in enumerate(mols):
        m = len(mo["members"])
        a = 0 if mol_types is None else int(mol_types[k])
        u = np.empty((m, 3), dtype=object)
        u[np.array(ranks[k])] = U[k]
        umax[k] = max(abs(int(x)) for x in U[k].ravel()) / scale
        b = u[1:] - u[:-1]
        H, r2all = 0, []
        for s in range(1, m):
            d = u[s:] - u[:-s]
            r2 = (d * d).sum(axis=1).tolist()
            H += sum(inverse_root(x, lg) for x in r2 if x)
            r2all += r2
            if mo["ends"] is not None and s < ns:
                curves[a][s][0] += sum(r2)
                if s < m - 1:
                    curves[a][s][1] += int((b[:-s] * b[s:]).sum())
        if mo["ends"] is not None:
            curves[a][0][1] += int((b * b).sum())
            for s in range(min(ns, m)):
                terms[a, s, 0] += m - s
                terms[a, s, 1] += m - 1 - s
        nz = [x for x in r2all if x]
        nzero += len(r2all) - len(nz)
        if nz:
            rmin2 = min(nz) if rmin2 is None else min(rmin2, min(nz))
        r2f = np.array([x / sc2 for x in nz], dtype=np.float64)
        s3[k] = (r2f ** -1.5).sum()
        inv[k] = Fraction(2 * H, (1 << FBITS) * m * m)
        hsum[k] = float(Fraction(H, 1 << FBITS))
    inexact = 0
    out_curves = np.zeros((ntypes, ns, 2))
    for a in range(ntypes):
        for s in range(ns):
            for c in range(2):
                x = Fraction(curves[a][s][c], sc2)
                out_curves[a, s, c] = float(x)
                inexact += Fraction(out_curves[a, s, c]) != x
    t = np.zeros(nmol, dtype=int) if mol_types is None else np.asarray(mol_types)
    sums = np.array([[float(sum((v for v, ta in zip(inv, t) if ta == a), Fraction(0))),
                      float(sum((v * v for v, ta in zip(inv, t) if ta == a), Fraction(0)))] for a in range(ntypes)])
    size = np.array([len(mo["members"]) for mo in mols])
    return dict(inv_rh=np.array([float(v) for v in inv]), curves=out_curves, sums=sums, terms=terms, inexact=inexact, hsum=hsum, s3=s3,
                rmin=math.sqrt(rmin2 / sc2), nzero=nzero, npairs=size * (size - 1) // 2, size=size,
                linear=np.array([mo["ends"] is not None for mo in mols]), umax=umax, mols=mols, ranks=ranks)


# ---- the kernel's order of operations, restated in NumPy float64 -------------------------------------------------------------------
def kernel_order(pos, box, bonds, mol_types=None, ntypes=1, ns=1):
    """(inv_rh (nmol,), curves (ntypes, ns, 2), sums (ntypes, 2)) as the kernels compute them, in float64 with their order of
    operations: the unfolding of the conformation pass (minimum image, pointer jumping); per (molecule, s) the terms in ascending c,
    one after another; the sum of H(s) by the halving tree over the ranks; per (tile, type, s) and for the sums of a (tile, type)
    the molecules in ascending number, one after another; the tiles lane by lane of 64, then the xor butterfly.  Fused multiply-adds
    are not restated: r2 and b.b' may differ in their last bit."""
    pos = np.asarray(pos, dtype=np.float64)
    Lx, Ly, Lz, xy = (float(v) for v in box)
    mols, _ = layout(pos.shape[0], bonds)
    ranks = ranks_of(pos.shape[0], bonds, mols)
    first, rounds = tiles_of(mols)
    nmol, ntile = len(mols), len(rounds)
    inv = np.zeros(nmol)
    D, C = np.zeros((nmol, ns)), np.zeros((nmol, ns))
    for k, mo in enumerate(mols):
        mem, par, m = np.array(mo["members"]), np.array(mo["parent"]), len(mo["members"])
        d = pos[mem, :3] - pos[mem[par], :3]
        ny = np.rint(d[:, 1] * (1.0 / Ly)); d[:, 1] -= ny * Ly; d[:, 0] -= ny * xy * Ly
        d[:, 0] -= np.rint(d[:, 0] * (1.0 / Lx)) * Lx
        d[:, 2] -= np.rint(d[:, 2] * (1.0 / Lz)) * Lz
        d[0] = 0.0
        u, anc = d.copy(), par.copy()
        tile = max(t for t in range(ntile) if first[t] <= k)
        for _ in range(rounds[tile]):
            u, anc = u + u[anc], anc[anc]
        x = np.empty_like(u)
        x[np.array(ranks[k])] = u                              # rank order
        b = x[1:] - x[:-1]
        H, Dk, Ck = np.zeros(m), np.zeros(m), np.zeros(m)
        for c in range(m):                                     # the lane of separation s = 0 .. m - 1 - c takes its term c
            e = x[c:] - x[c]
            r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            with np.errstate(divide="ignore"):
                H[:m - c] += np.where(r2 != 0.0, 1.0 / np.sqrt(r2), 0.0)
            Dk[:m - c] += r2
            if c < m - 1:
                bb = b[c:] * b[c]
                Ck[:m - 1 - c] += (bb[:, 0] + bb[:, 1]) + bb[:, 2]
        inv[k] = 2.0 * _tree(H[:, None], m)[0] / (float(m) * float(m))
        if mo["ends"] is not None:
            w = min(m, ns)
            D[k, :w], C[k, :w] = Dk[:w], Ck[:w]
    t = np.zeros(nmol, dtype=int) if mol_types is None else np.asarray(mol_types)
    linear = np.array([mo["ends"] is not None for mo in mols])

    def across(part):                                          # part (ntiles, ncol)
        lanes = np.zeros((64, part.shape[1]))
        for q in range(part.shape[0]):
            lanes[q % 64] += part[q]
        w = 32
        while w > 0:
            lanes = lanes + lanes[np.arange(64) ^ w]
            w //= 2
        return lanes[0]
    curves, sums = np.zeros((ntypes, ns, 2)), np.zeros((ntypes, 2))
    for a in range(ntypes):
        pc, ps = np.zeros((ntile, ns * 2)), np.zeros((ntile, 2))
        for q in range(ntile):
            for k in range(first[q], first[q + 1]):
                if t[k] != a:
                    continue
                ps[q, 0] += inv[k]
                ps[q, 1] += inv[k] * inv[k]
                if linear[k]:
                    pc[q, 0::2] += D[k]
                    pc[q, 1::2] += C[k]
        curves[a] = across(pc).reshape(ns, 2)
        sums[a] = across(ps)
    return inv, curves, sums


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------
def dyadic_bounds(ref, mol_types, ntypes):
    """On dyadic inputs every r2 is exact, so a term 1.0 / sqrt(r2) carries two correctly rounded operations, a sum of P = m (m - 1) / 2
    positive terms at most P - 1 additions in any order, then the division by m^2, and one to spare: |inv_rh - exact| <= (P + 4) EPS
    inv_rh.  A type's sums: the bounds of its N molecules, v^2 with 2 (P + 4) EPS + 2 EPS relative (the product's rounding and the
    second order), and N + 8 additions of positive terms (in the tile, a lane's tiles, six butterfly levels), each EPS of the sum.
    Returns (inv_rh (nmol,), sums (ntypes, 2)), absolute."""
    v = ref["inv_rh"]
    rel = (ref["npairs"] + 4.0) * EPS
    t = np.zeros(len(v), dtype=int) if mol_types is None else np.asarray(mol_types)
    sums = np.zeros((ntypes, 2))
    for a in range(ntypes):
        k = t == a
        n = k.sum() + 8.0
        sums[a, 0] = (rel[k] * v[k]).sum() + n * EPS * v[k].sum()
        sums[a, 1] = ((2.0 * rel[k] + 2.0 * EPS) * v[k] ** 2).sum() + n * EPS * (v[k] ** 2).sum()
    return rel * v, sums


def bounds(ref, box, mol_types, ntypes, ns):
    """Absolute error bounds of the kernel's float64 outputs in general position against the once-rounded reference, extending
    conformation_cases.bounds (S = max(U, Lmax), du <= 16 m EPS S per component):
      d = u_{c+s} - u_c and b_c: 2 du + EPS 2 S <= 34 m EPS S = tR, |d| <= 2 S per component;
      r2 and b . b': three products 2 (2 S) tR + EPS 4 S^2 each and two additions on values <= 12 S^2: <= 4 tG = 1024 m EPS S^2 = t2;
      D(s), C(s) of one molecule, n terms one after another on partial sums <= 12 n S^2:  n t2 + n^2 12 EPS S^2 <= n (1024 m + 12 n) EPS S^2;
      a type's curve: its molecules' bounds and N + 8 additions (N molecules of the type), each EPS of the sum of 12 n S^2;
      1 / sqrt(r2): with x = t2 / r^2 <= 1/2 (asserted through rmin) the relative error of r2^(-1/2) is <= x, plus 3 EPS for the square
        root, the division and the second order: per term (1 / r) (t2 / r^2 + 3 EPS), r the reference's exact distance;
      inv_rh: (2 / m^2) [t2 sum 1/r^3 + (3 + m + 10) EPS sum 1/r] -- at most m additions along a lane and 10 levels of the tree, on
        positive terms -- and 2 EPS inv_rh for the division and the reference's rounding;
      sums: as dyadic_bounds, from these.
    Returns (inv_rh (nmol,), curves (ntypes, ns, 2), sums (ntypes, 2), x: the largest t2 / r^2)."""
    S = np.maximum(ref["umax"], max(box[:3]))
    m = ref["size"].astype(np.float64)
    t2 = 1024.0 * m * EPS * S * S
    v = ref["inv_rh"]
    dv = 2.0 / (m * m) * (t2 * ref["s3"] + (m + 13.0) * EPS * ref["hsum"]) + 2.0 * EPS * v
    t = np.zeros(len(v), dtype=int) if mol_types is None else np.asarray(mol_types)
    curves, sums = np.zeros((ntypes, ns, 2)), np.zeros((ntypes, 2))
    for a in range(ntypes):
        k = t == a
        n = k.sum() + 8.0
        sums[a, 0] = dv[k].sum() + n * EPS * v[k].sum()
        sums[a, 1] = (2.0 * v[k] * dv[k] + dv[k] ** 2 + 2.0 * EPS * v[k] ** 2).sum() + n * EPS * (v[k] ** 2).sum()
        kl = k & ref["linear"]
        nl = kl.sum() + 8.0
        for s in range(ns):
            for c in range(2):
                cnt = np.maximum(m[kl] - s - c, 0.0)
                curves[a, s, c] = (cnt * (1024.0 * m[kl] + 12.0 * cnt) * EPS * S[kl] ** 2).sum() + nl * EPS * (12.0 * cnt * S[kl] ** 2).sum()
    return dv, curves, sums, float((t2 / ref["rmin"] ** 2).max())


# ---- the cases, each computed once -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dyadic(name, ns=None):
    box, n, bonds, pos, types, ntypes = cc.DYADIC[name]
    ns = ns or 1024
    return box, n, bonds, pos, types, ntypes, ns, reference(pos, box, bonds, types, ntypes, ns)


@functools.lru_cache(maxsize=None)
def edge(k, ns=1024):
    lengths, xy, ntypes, seed = cc.EDGES[k]
    box, n, bonds, pos, types = cc.edge_case(lengths, xy, ntypes, seed)
    return box, n, bonds, pos, types, ntypes, ns, reference(pos, box, bonds, types, ntypes, ns)
