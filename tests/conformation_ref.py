"""Reference for the chain conformations (pse_molecules_compute, analyze.Conformations) in exact rational arithmetic: every float64
input is taken as the fractions.Fraction it is, the integer of every minimum image is decided from the exact rationals, every sum and
product is exact, and a result is rounded to float64 once, at the end.  The layout -- components, breadth-first order, ends -- is found
here in plain Python, independently of the library's.  Also: the margins by which a set of inputs stays clear of a half box and of
the bin edges, and a NumPy float64 restatement of the kernel's order of operations."""
import math
from fractions import Fraction

import numpy as np

COLS = 14
TILE = 1024


def layout(n, bonds):
    """The molecules of the bond list: a list, in the order of their smallest member, of dicts with members (caller indices in
    breadth-first order from the smallest member, neighbours in ascending order), parent (breadth-first position of the parent, the
    root its own), depth, ends ((lo, hi) positions, lower caller index first, or None) and nring; and mol_of (n,)."""
    nb = [set() for _ in range(n)]
    nbonds = 0
    for i, j in np.asarray(bonds).tolist():
        assert i != j and 0 <= i < n and 0 <= j < n and j not in nb[i]
        nb[i].add(j); nb[j].add(i)
        nbonds += 1
    mol_of = [-1] * n
    mols = []
    for root in range(n):
        if mol_of[root] >= 0 or not nb[root]:
            continue
        members, parent, depth, where = [root], [0], [0], {root: 0}
        mol_of[root] = len(mols)
        q = 0
        while q < len(members):
            for j in sorted(nb[members[q]]):
                if j not in where:
                    where[j] = len(members)
                    mol_of[j] = len(mols)
                    members.append(j); parent.append(q); depth.append(depth[q] + 1)
            q += 1
        degree = [len(nb[i]) for i in members]
        nring = sum(degree) // 2 - (len(members) - 1)
        ones = [p for p, d in enumerate(degree) if d == 1]
        linear = nring == 0 and len(ones) == 2 and all(d in (1, 2) for d in degree)
        ends = tuple(sorted(ones, key=lambda p: members[p])) if linear else None
        mols.append(dict(members=members, parent=parent, depth=depth, ends=ends, nring=nring))
    return mols, np.array(mol_of)


def tiles_of(mols):
    """The tiles of the greedy packing: (first molecule of every tile and the end, rounds per tile)."""
    first, rounds, fill, deep = [0], [], 0, 0
    for k, mo in enumerate(mols):
        m = len(mo["members"])
        assert m <= TILE
        if fill + m > TILE:
            first.append(k); rounds.append(math.ceil(math.log2(deep + 1))); fill, deep = 0, 0
        fill += m
        deep = max(deep, max(mo["depth"]))
    first.append(len(mols)); rounds.append(math.ceil(math.log2(deep + 1)))
    return first, rounds


def _nearest(q):
    """The integer nearest to the Fraction q (ties do not occur in inputs held clear of a half box)."""
    return math.floor(q + Fraction(1, 2))


def min_image(d, box):
    """The minimum image of the exact displacement d = [dx, dy, dz] in the box (Lx, Ly, Lz, xy) of Fractions, in the order of the
    device's: y with the tilt taken off x, then x, then z.  Returns (image, margin): the smallest distance of a rounded quotient from
    a half-integer, i.e. from a half box in units of the box length."""
    Lx, Ly, Lz, xy = box
    dx, dy, dz = d
    qy = dy / Ly; ny = _nearest(qy)
    dy -= ny * Ly; dx -= ny * xy * Ly
    qx = dx / Lx; nx = _nearest(qx)
    dx -= nx * Lx
    qz = dz / Lz; nz = _nearest(qz)
    dz -= nz * Lz
    margin = min(abs(abs(q - n) - Fraction(1, 2)) for q, n in ((qx, nx), (qy, ny), (qz, nz)))
    return [dx, dy, dz], float(margin)


def _bin(q, nbins, vmax):
    """(bin of sqrt(q), relative distance of sqrt(q) from the nearest bin edge) for the exact q >= 0: bin b holds b vmax / nbins <=
    sqrt(q) < (b + 1) vmax / nbins, decided on the squares; values at or above vmax fall in bin nbins."""
    w = Fraction(vmax) / nbins
    b = int(math.sqrt(float(q)) / float(w))
    while (b * w) ** 2 > q:
        b -= 1
    while ((b + 1) * w) ** 2 <= q:
        b += 1
    v = math.sqrt(float(q))
    edge = min(abs(v - float(b * w)), abs(float((b + 1) * w) - v))
    return min(b, nbins), (edge / v if v > 0 else 1.0)


def reference(pos, box, bonds, mol_types=None, ntypes=1, nbins=0, rg_max=None, ree_max=None):
    """Everything pse_molecules_compute writes in one call from zeroed outputs, rounded once: rows (nmol, 14), unfolded (n, 4) with NaN
    rows for non-members, sums (ntypes, 14) -- `sample` is the same --, hist (2, ntypes, nbins + 1); and what the tests need beside
    them: image_margin, bin_margin (the smallest over the call), umax (nmol,): max |u_i| per molecule in the infinity norm, size
    (nmol,), linear (nmol,), mols, and inexact, inexact4: how many of the float64 results were rounded at all -- 0: the case is exact --, the fourth moments of sums
    (columns 6 and 13) counted apart from everything else."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    fbox = tuple(Fraction(float(v)) for v in box)
    mols, mol_of = layout(n, bonds)
    nmol = len(mols)
    rows = np.full((nmol, COLS), np.nan)
    unfolded = np.full((n, 4), np.nan)
    exact_sums = [[Fraction(0)] * COLS for _ in range(ntypes)]
    hist = np.zeros((2, ntypes, nbins + 1), dtype=np.int64)
    image_margin, bin_margin = 0.5, 1.0
    umax = np.zeros(nmol)
    P = [[Fraction(float(v)) for v in pos[i, :3]] for i in range(n)]
    inexact = [0, 0]

    def fl(x, fourth=False):   # the one rounding; counts the results that needed it
        f = float(x)
        inexact[1 if fourth else 0] += Fraction(f) != x
        return f
    order = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    for k, mo in enumerate(mols):
        mem, m = mo["members"], len(mo["members"])
        a = 0 if mol_types is None else int(mol_types[k])
        u = [[Fraction(0)] * 3]
        for p in range(1, m):
            d, mg = min_image([P[mem[p]][c] - P[mem[mo["parent"][p]]][c] for c in range(3)], fbox)
            image_margin = min(image_margin, mg)
            u.append([u[mo["parent"][p]][c] + d[c] for c in range(3)])
        root = P[mem[0]]
        su = [sum(x[c] for x in u) for c in range(3)]
        for p in range(m):
            unfolded[mem[p]] = [fl(root[c] + u[p][c]) for c in range(3)] + [float(k)]
        umax[k] = max(abs(float(x[c])) for x in u for c in range(3))
        v = [[x[c] - su[c] / m for c in range(3)] for x in u]
        G = [sum(x[i] * x[j] for x in v) / m for i, j in order]
        rg2 = G[0] + G[1] + G[2]
        rows[k, :3] = [fl(root[c] + su[c] / m) for c in range(3)]
        rows[k, 3:9] = [fl(g) for g in G]
        rows[k, 9] = fl(rg2)
        for c in range(6):
            exact_sums[a][c] += G[c]
        exact_sums[a][6] += rg2 * rg2
        if nbins:
            b, mg = _bin(rg2, nbins, rg_max)
            hist[0, a, b] += 1
            bin_margin = min(bin_margin, mg)
        if mo["ends"] is not None:
            lo, hi = mo["ends"]
            R = [u[hi][c] - u[lo][c] for c in range(3)]
            R2 = R[0] * R[0] + R[1] * R[1] + R[2] * R[2]
            rows[k, 10:13] = [fl(x) for x in R]
            rows[k, 13] = fl(R2)
            for c, (i, j) in enumerate(order):
                exact_sums[a][7 + c] += R[i] * R[j]
            exact_sums[a][13] += R2 * R2
            if nbins:
                b, mg = _bin(R2, nbins, ree_max)
                hist[1, a, b] += 1
                bin_margin = min(bin_margin, mg)
    sums = np.array([[fl(x, c in (6, 13)) for c, x in enumerate(row)] for row in exact_sums])
    return dict(rows=rows, unfolded=unfolded, sums=sums, hist=hist, image_margin=image_margin, bin_margin=bin_margin, umax=umax, inexact=inexact[0], inexact4=inexact[1],
                size=np.array([len(mo["members"]) for mo in mols]), linear=np.array([mo["ends"] is not None for mo in mols]), mols=mols,
                mol_of=mol_of)


# ---- the kernel's order of operations, restated in NumPy float64 -------------------------------------------------------------------
def _tree(x, m):
    """The halving tree of the kernel over the positions 0 .. m - 1 of the rows of x (m, ncol): position p adds position p + s for s =
    the powers of two below m, descending, where p + s < m."""
    x = x.copy()
    s = 1
    while s < m:
        s *= 2
    s //= 2
    while s > 0:
        k = min(s, m - s)
        if k > 0:
            x[:k] += x[s:s + k]
        s //= 2
    return x[0]


def kernel_order(pos, box, bonds, mol_types=None, ntypes=1):
    """rows (nmol, 14) and sums (ntypes, 14) as the kernels compute them, in float64 with their order of operations: the minimum image
    of the device, pointer jumping for the tree sums, the halving trees over the members and over the molecules of a tile, the tiles
    in order (lane by lane of 64, then the xor butterfly).  Fused multiply-adds are not restated: |R|^2 may differ in its last bit."""
    pos = np.asarray(pos, dtype=np.float64)
    Lx, Ly, Lz, xy = (float(v) for v in box)
    mols, _ = layout(pos.shape[0], bonds)
    first, rounds = tiles_of(mols)
    rows = np.full((len(mols), COLS), np.nan)
    terms = np.zeros((len(mols), COLS))
    for k, mo in enumerate(mols):
        mem, par, m = np.array(mo["members"]), np.array(mo["parent"]), len(mo["members"])
        d = pos[mem, :3] - pos[mem[par], :3]
        ny = np.rint(d[:, 1] * (1.0 / Ly)); d[:, 1] -= ny * Ly; d[:, 0] -= ny * xy * Ly
        d[:, 0] -= np.rint(d[:, 0] * (1.0 / Lx)) * Lx
        d[:, 2] -= np.rint(d[:, 2] * (1.0 / Lz)) * Lz
        d[0] = 0.0
        u, anc = d.copy(), par.copy()
        tile = max(t for t in range(len(rounds)) if first[t] <= k)
        for _ in range(rounds[tile]):
            u, anc = u + u[anc], anc[anc]
        mean = _tree(u, m) / float(m)
        v = u - mean
        G = _tree(np.stack([v[:, 0] * v[:, 0], v[:, 1] * v[:, 1], v[:, 2] * v[:, 2], v[:, 0] * v[:, 1], v[:, 0] * v[:, 2],
                            v[:, 1] * v[:, 2]], 1), m) / float(m)
        rg2 = (G[0] + G[1]) + G[2]
        rows[k, :3] = pos[mem[0], :3] + mean
        rows[k, 3:9], rows[k, 9] = G, rg2
        terms[k, :6], terms[k, 6] = G, rg2 * rg2
        if mo["ends"] is not None:
            R = u[mo["ends"][1]] - u[mo["ends"][0]]
            R2 = (R[0] * R[0] + R[1] * R[1]) + R[2] * R[2]
            rows[k, 10:13], rows[k, 13] = R, R2
            terms[k, 7:13] = [R[0] * R[0], R[1] * R[1], R[2] * R[2], R[0] * R[1], R[0] * R[2], R[1] * R[2]]
            terms[k, 13] = R2 * R2
    sums = np.zeros((ntypes, COLS))
    for a in range(ntypes):
        part = []
        for t in range(len(rounds)):
            x = terms[first[t]:first[t + 1]].copy()
            if mol_types is not None:
                x[np.asarray(mol_types)[first[t]:first[t + 1]] != a] = 0.0
            part.append(_tree(x, x.shape[0]))
        part = np.array(part)
        lanes = np.zeros((64, COLS))
        for t in range(part.shape[0]):
            lanes[t % 64] += part[t]
        w = 32
        while w > 0:   # the xor butterfly: every lane ends with the same sum
            lanes = lanes + lanes[np.arange(64) ^ w]
            w //= 2
        sums[a] = lanes[0]
    return rows, sums
