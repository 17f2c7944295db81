"""The inputs that tests/test_gpu_conformations.py runs on the device and tests/test_conformations_cpu.py checks on the CPU: molecule
shapes as bond lists, dyadic and general-position coordinates, the re-imaging by lattice vectors, and the error bound of the kernel."""
import numpy as np

EPS = 2.0 ** -53   # the rounding unit of float64


# ---- topologies: (n, bonds) with the molecules in the order of their smallest member ---------------------------------------------------
def chain(first, m):
    i = np.arange(first, first + m - 1)
    return np.stack([i, i + 1], 1)


def ring(first, m):
    return np.concatenate([chain(first, m), [[first + m - 1, first]]])


def star(first, m):
    """A hub (the first index) with m - 1 arms of one bead."""
    return np.stack([np.full(m - 1, first), np.arange(first + 1, first + m)], 1)


def comb(first, backbone, tooth):
    """A backbone chain with a side chain of `tooth` beads on every second backbone bead."""
    out, nxt = [chain(first, backbone)], first + backbone
    for b in range(0, backbone, 2):
        out.append(np.array([[first + b, nxt]]))
        out.append(chain(nxt, tooth))
        nxt += tooth
    return np.concatenate([o for o in out if len(o)]), nxt - first


def build(shapes, gaps=()):
    """(n, bonds, sizes, kinds) of the molecules `shapes` = [(kind, m), ...] laid one after another, with `gaps[k]` unbonded particles in
    front of molecule k."""
    bonds, at, sizes = [], 0, []
    for k, (kind, m) in enumerate(shapes):
        at += gaps[k] if k < len(gaps) else 0
        if kind == "comb":
            b, m = comb(at, m, 3)
        else:
            b = {"chain": chain, "ring": ring, "star": star}[kind](at, m)
        bonds.append(b); sizes.append(m); at += m
    return at, np.concatenate(bonds), sizes, [k for k, _ in shapes]


def relabel(n, bonds, rng):
    """The same molecules under a random relabelling of the particles that keeps every molecule's smallest member where it is (and with
    it the numbering of the molecules): (bonds in the new labels, new_of_old)."""
    from conformation_ref import layout
    mols, _ = layout(n, bonds)
    new_of_old = np.arange(n)
    for mo in mols:
        rest = np.array(sorted(mo["members"])[1:])
        new_of_old[rest] = rng.permutation(rest)
    return new_of_old[np.asarray(bonds)], new_of_old


# ---- coordinates -------------------------------------------------------------------------------------------------------------------------
def wrap(pos, box):
    """pos wrapped into the box (Lx, Ly, Lz, xy), in the order of the device's minimum image; exact on dyadic data."""
    Lx, Ly, Lz, xy = box
    pos = pos.copy()
    n = np.floor(pos[:, 2] / Lz + 0.5); pos[:, 2] -= n * Lz
    n = np.floor(pos[:, 1] / Ly + 0.5); pos[:, 1] -= n * Ly; pos[:, 0] -= n * (xy * Ly)
    n = np.floor((pos[:, 0] - xy * pos[:, 1]) / Lx + 0.5); pos[:, 0] -= n * Lx
    return pos


def reimage(pos, box, rng, reach=3):
    """Every bead moved by its own random lattice vector."""
    Lx, Ly, Lz, xy = box
    k = rng.integers(-reach, reach + 1, (pos.shape[0], 3)).astype(np.float64)
    out = pos.copy()
    out[:, 0] += k[:, 0] * Lx + k[:, 1] * (xy * Ly)
    out[:, 1] += k[:, 1] * Ly
    out[:, 2] += k[:, 2] * Lz
    return out


def place(n, bonds, box, rng, step, grid=None):
    """Coordinates for the molecules of `bonds`: every tree edge of the reference layout a random vector -- grid=None: a random
    direction of a length in [0.5, step]; grid=g: a non-zero vector of multiples of g with components in [-step, step] -- from a random
    root, unbonded particles anywhere, all wrapped into the box.  A ring bond that closes a cycle is as long as the walk makes it: the
    callers keep rings planar and small (ring_place)."""
    from conformation_ref import layout
    mols, _ = layout(n, bonds)
    L = np.array(box[:3])
    pos = (rng.uniform(size=(n, 3)) - 0.5) * L
    if grid is not None:
        pos = np.round(pos / grid) * grid
    for mo in mols:
        mem, par = mo["members"], mo["parent"]
        for p in range(1, len(mem)):
            if grid is None:
                d = rng.normal(size=3)
                d *= rng.uniform(0.5, step) / np.linalg.norm(d)
            else:
                d = np.zeros(3)
                while not d.any():
                    d = rng.integers(-int(step / grid), int(step / grid) + 1, 3) * grid
            pos[mem[p]] = pos[mem[par[p]]] + d
    return pos


def ring_place(pos, first, m, radius, rng, grid=None):
    """The m beads first .. first + m - 1 on a tilted circle around the position of `first`, with a little noise."""
    t = 2.0 * np.pi * np.arange(m) / m
    e1, e2 = np.array([1.0, 0.0, 0.25]), np.array([0.0, 1.0, -0.5])
    p = pos[first] + radius * ((np.cos(t) - 1.0)[:, None] * e1 + np.sin(t)[:, None] * e2) + rng.uniform(-0.05, 0.05, (m, 3))
    p[0] = pos[first]
    pos[first:first + m] = p if grid is None else np.round(p / grid) * grid


# ---- the dyadic cases: every quantity exact --------------------------------------------------------------------------------------------
# Coordinates are multiples of a grid g >= 2^-8 (so multiples of 2^-8), box lengths 16 and 32, xy Ly a multiple of 4, sizes powers of
# two: u is a multiple of g, the mean of g / m, v^2 of (g / m)^2 and G of g^2 / m^3; with |v| < 2^7 a sum of m squares stays below
# 2^(14 + log2 m), so G needs 14 + 4 log2 m - 2 log2 g <= 53 bits: g = 1 for m = 1024 (bond length 1), 2^-8 up to m = 64.  Partial
# sums are bounded by the sums of the absolute values, which fit the same way.  The fourth moments (Rg^2)^2 and (R^2)^2 are products
# of exact values rounded once by the kernel and once by the reference; the SUM of several rounded ones is not the rounded exact sum,
# so a type that holds more than one molecule must have exact fourth moments: reference()["inexact"] == 0 is asserted for those
# cases, and for the others that every type holds one molecule.

def dyadic_cases():
    rng = np.random.default_rng(7)
    out = {}
    # a 64-bead chain in shuffled caller order among unbonded particles, g = 2^-8
    n, bonds, _, _ = build([("chain", 64)], gaps=(5,))
    n += 3
    box = (16.0, 16.0, 16.0, 0.25)
    pos = place(n, bonds, box, rng, 2.0, grid=2.0 ** -8)
    b2, new_of_old = relabel(n, bonds, rng)
    p2 = np.empty_like(pos); p2[new_of_old] = pos
    out["shuffled chain"] = (box, n, b2, wrap(p2, box), None, 1)
    # 1024 beads of bond length 1 in a box of 16: the walk winds round the box many times
    n, bonds, _, _ = build([("chain", 1024)])
    box = (16.0, 16.0, 16.0, -0.5)
    steps = np.eye(3)[rng.integers(0, 3, 1023)] * rng.choice([-1.0, 1.0], 1023)[:, None]
    steps[::3] = [1.0, 0.0, 0.0]                                               # a drift along x: some forty box lengths
    pos = np.concatenate([[[0.5, -3.25, 7.0]], [0.5, -3.25, 7.0] + np.cumsum(steps, 0)])
    out["1024 chain"] = (box, n, bonds, wrap(pos, box), None, 1)
    # a star of 256 around one hub, g = 2^-4; non-cubic box
    n, bonds, _, _ = build([("star", 256)], gaps=(1,))
    box = (16.0, 32.0, 16.0, 0.5)
    out["star 256"] = (box, n, bonds, wrap(place(n, bonds, box, rng, 3.0, grid=2.0 ** -4), box), None, 1)
    # a ring of 64, g = 2^-6
    n, bonds, _, _ = build([("ring", 64)])
    box = (16.0, 32.0, 16.0, 0.0)
    pos = np.zeros((n, 3)); pos[0] = [7.5, -15.0, 3.0]
    ring_place(pos, 0, 64, 5.0, rng, grid=2.0 ** -6)
    out["ring 64"] = (box, n, bonds, wrap(pos, box), None, 1)
    # 513 dimers: two tiles, two types; g = 2^-4 keeps the sums of 513 fourth moments exact
    n, bonds, _, _ = build([("chain", 2)] * 513)
    box = (16.0, 16.0, 16.0, 0.5)
    out["513 dimers"] = (box, n, bonds, wrap(place(n, bonds, box, rng, 3.0, grid=2.0 ** -4), box), np.arange(513) % 2, 2)
    # sizes 2, 64, 256 and 1024 together, a type each (1024: a tile of its own), unit steps
    n, bonds, _, _ = build([("chain", 2), ("chain", 64), ("chain", 256), ("chain", 1024)], gaps=(0, 2, 0, 1))
    box = (16.0, 32.0, 16.0, -0.5)
    out["2 64 256 1024"] = (box, n, bonds, wrap(place(n, bonds, box, rng, 1.0, grid=1.0), box), np.arange(4), 4)
    # four compact 64-mers of two types on the integer lattice: exact fourth moments, summed over a type
    n, bonds, _, _ = build([("chain", 64)] * 4)
    box = (16.0, 16.0, 16.0, 0.25)
    out["four 64"] = (box, n, bonds, wrap(place(n, bonds, box, rng, 1.0, grid=1.0), box), np.array([0, 1, 1, 0]), 2)
    return out


DYADIC = dyadic_cases()
HIST = dict(nbins=32, rg_max=23.9, ree_max=63.7)   # (edges that no dyadic value sits on)



# ---- general positions at the wave and tile edges --------------------------------------------------------------------------------------

EDGE_SHAPES = ([("chain", 257), ("chain", 255), ("star", 65), ("ring", 63), ("chain", 64)] + [("chain", 64)] * 5   # a tile of exactly 1024
               + [("chain", 1023), ("chain", 3), ("comb", 10), ("chain", 65), ("ring", 3), ("chain", 63), ("chain", 2)])   # 3 does not fit


def edge_case(lengths, xy, ntypes, seed):
    from conformation_ref import layout
    rng = np.random.default_rng(seed)
    n, bonds, sizes, kinds = build(EDGE_SHAPES, gaps=(2, 0, 1, 0, 0, 3))
    box = lengths + (xy,)
    pos = place(n, bonds, box, rng, 3.0)
    mols, _ = layout(n, bonds)
    for k, kind in enumerate(kinds):
        if kind == "ring":
            ring_place(pos, mols[k]["members"][0], sizes[k], 0.4 * sizes[k] ** 0.5 + 0.5, rng)
    if ntypes == 1:
        types = None
    elif ntypes == 2:
        types = np.array([1 if kind in ("star", "ring", "comb") else 0 for kind in kinds])   # type 1 has no linear molecule
    else:
        types = np.array([7 if kind != "chain" else k % 5 for k, kind in enumerate(kinds)])   # 5 and 6 are empty, 7 has no linear one
    return box, n, bonds, wrap(pos, box), types


EDGES = [((16.0, 16.0, 16.0), 0.5, 1, 11), ((16.0, 32.0, 16.0), -0.5, 2, 12), ((16.0, 32.0, 16.0), 0.5, 8, 13),
         ((16.0, 16.0, 16.0), -0.5, 8, 14)]
EDGE_HIST = dict(nbins=50, rg_max=20.0, ree_max=90.0)



# ---- the bound ---------------------------------------------------------------------------------------------------------------------------
def bounds(ref, box):
    """Absolute error bounds of the kernel's float64 outputs against the once-rounded exact values, from the order of its operations,
    with S = max(U, Lmax), U the largest |u_i| of the molecule and m its size.  Every count below is of roundings of relative size
    EPS = 2^-53 (ties to even), products with |x| <= S included:
      an edge: the subtraction of two positions of size <= 1.5 L (EPS 1.5 L, twice with the tilt), n xy Ly in two roundings (2 EPS L),
        the three subtractions of n L (each exact or EPS L): <= 6 EPS S;
      u_i: at most m edges and at most 10 additions of partial sums <= U:                      du  <= (6 m + 10) EPS S  <= 16 m EPS S;
      the mean: du, 10 levels of the tree and the division:                                     dmean <= du + 11 EPS S;
      v = u - mean: dv <= du + dmean + EPS S                                                          <= 44 m EPS S,   |v| <= 2 S;
      a product v_a v_b: 2 (2 S) dv + EPS 4 S^2                                                        <= (176 m + 4) EPS S^2;
      G_ab: the mean of m such products, 10 levels of the tree and the division on values <= 4 S^2:   <= (176 m + 52) EPS S^2
                                                                                                       <= 256 m EPS S^2 = tG;
      Rg^2: three of them and two additions on values <= 12 S^2:                                      <= 3 tG + 24 EPS S^2 <= 4 tG;
      R = u_hi - u_lo: 2 du + EPS 2 S <= 34 m EPS S = tR;  R_a R_b: 2 (2 S) tR + EPS 4 S^2 <= 140 m EPS S^2 <= tG;  R^2 <= 4 tG;
      c = r_root + mean: dmean + EPS (1.5 L + S) <= 32 m EPS S;  unfolded: du + EPS (1.5 L + S) <= 32 m EPS S;
      (Rg^2)^2 and (R^2)^2 on values q <= 12 S^2: 2 q 4 tG + EPS q^2 <= 96 S^2 tG + 144 EPS S^4 <= 128 S^2 tG.
    A type's sum adds the bounds of its molecules and, for the order of the additions (at most 10 + 1 + 6 + 1 levels), 18 EPS times the
    sum of the bounds on the terms' sizes.  Returns (rows (nmol, 14), unfolded per molecule (nmol,), per-molecule bounds of the 14 terms
    (nmol, 14), sizes of the 14 terms (nmol, 14))."""
    Lmax = max(box[:3])
    S = np.maximum(ref["umax"], Lmax)
    m = ref["size"].astype(np.float64)
    tG = 256.0 * m * EPS * S * S
    rows = np.zeros((len(m), 14))
    rows[:, 0:3] = (32.0 * m * EPS * S)[:, None]
    rows[:, 3:9] = tG[:, None]
    rows[:, 9] = 4.0 * tG
    rows[:, 10:13] = (34.0 * m * EPS * S)[:, None]
    rows[:, 13] = 4.0 * tG
    terms = np.zeros((len(m), 14))
    terms[:, 0:6] = tG[:, None]; terms[:, 7:13] = tG[:, None]
    terms[:, 6] = terms[:, 13] = 128.0 * S * S * tG
    size = np.zeros((len(m), 14))
    size[:, 0:6] = size[:, 7:13] = (4.0 * S * S)[:, None]
    size[:, 6] = size[:, 13] = (12.0 * S * S) ** 2
    return rows, 32.0 * m * EPS * S, terms, size


def sums_bound(ref, box, mol_types, ntypes):
    _, _, terms, size = bounds(ref, box)
    t = np.zeros(len(terms), dtype=int) if mol_types is None else np.asarray(mol_types)
    out = np.zeros((ntypes, 14))
    for a in range(ntypes):
        out[a] = terms[t == a].sum(axis=0) + 18.0 * EPS * size[t == a].sum(axis=0)
    return out
