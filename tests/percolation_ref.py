"""O(N^2) reference of the cluster analysis with percolation (pse_clusters_span), shared by tests/test_percolation_cpu.py (which
validates it) and tests/test_gpu_percolation.py (which compares the device to it).

Links come from cluster_ref (minimum image of oracle.pse_port, its 1e-9 clearance); their SHIFTS from NumPy with the arithmetic of
the device's min_image: for d = r_i - r_j, n2 = rint(d_y iLy), n1 = rint((d_x - n2 xy Ly) iLx), n3 = rint(d_z iLz).  A breadth-first
UNFOLDING in Python integers starts at the smallest caller index of every component (c = 0 there) and sets c_j = c_i + n_ij along
the links it walks; every link that contradicts it, m = c_j - c_i - n_ij != 0, ORs the axes of its non-zero components into the
component's flags (the links off the breadth-first tree are its fundamental cycles).  image = c where the component has no flag,
zeros otherwise.  Geometry of a component without a flag, 0 its label member: D_i = (r_i - r_0) + c_i (a1, a2, a3) in fp64 in the
order include/pse_amd.h writes down, q = rint(D 2^20) as Python integers, sum q and sum q^2 exact; Rg^2 once as a Fraction and once
by the fixed fp64 expression of the header, restated here in Python floats (IEEE fp64, no contraction).

Besides the clearance of the links there is a second one: q_margin, the least distance of any D 2^20 from a half-integer.  The device
may contract a product and a sum of D into one fma, which moves D by an ulp (1e-15 of a box length, 1e-9 in units of 2^-20): with
q_margin >= Q_CLEAR = 1e-6 no q can differ.  Every test asserts both before it compares anything.
Not a test module: nothing here is collected."""
from collections import deque
from fractions import Fraction

import numpy as np

import cluster_ref as cr

Q_SCALE = 2.0 ** 20
Q_CLEAR = 1e-6
RG2_ULPS = 8.0      # |rg2 - exact| <= 8 2^-53 2^-40 sum q^2 / s: the roundings of the fixed expression (pse_cluster_word.h counts 7)


def lattice(box):
    Lx, Ly, Lz, xy = (float(b) for b in box)
    return np.array([[Lx, 0.0, 0.0], [xy * Ly, Ly, 0.0], [0.0, 0.0, Lz]])


def shifts(pos, box, i, j):
    """(len(i), 3) int64: the integers min_image takes from r_i - r_j, and how far the nearest of the three rint arguments is from a tie."""
    Lx, Ly, Lz, xy = (float(b) for b in box)
    d = np.asarray(pos, dtype=float)[i] - np.asarray(pos, dtype=float)[j]
    ty = d[:, 1] * (1.0 / Ly)
    n2 = np.rint(ty)
    tx = (d[:, 0] - n2 * xy * Ly) * (1.0 / Lx)
    n1 = np.rint(tx)
    tz = d[:, 2] * (1.0 / Lz)
    n3 = np.rint(tz)
    t = np.stack([tx, ty, tz], axis=1)
    tie = float((0.5 - np.abs(t - np.rint(t))).min()) if len(i) else np.inf
    return np.stack([n1, n2, n3], axis=1).astype(np.int64), tie


def unfold(n, i, j, shift, ids=None):
    """(comp, c, flags): comp[k] the row of the smallest caller index of k's component, c (n, 3) Python-int unfolding from there,
    flags per row (of its component)."""
    ids = list(range(n)) if ids is None else [int(v) for v in ids]
    adj = [[] for _ in range(n)]
    for a, b, s in zip(np.asarray(i).tolist(), np.asarray(j).tolist(), np.asarray(shift).tolist()):
        adj[a].append((b, tuple(s)))                       # c_b = c_a + s
        adj[b].append((a, tuple(-v for v in s)))
    comp, c = [-1] * n, [None] * n
    for start in sorted(range(n), key=lambda k: ids[k]):
        if comp[start] >= 0:
            continue
        comp[start], c[start] = start, (0, 0, 0)
        todo = deque([start])
        while todo:
            a = todo.popleft()
            for b, s in adj[a]:
                if comp[b] < 0:
                    comp[b], c[b] = start, tuple(u + v for u, v in zip(c[a], s))
                    todo.append(b)
    flag_of = {}
    for a in range(n):
        for b, s in adj[a]:
            m = [c[b][k] - c[a][k] - s[k] for k in range(3)]
            bits = sum(1 << k for k in range(3) if m[k] != 0)
            flag_of[comp[a]] = flag_of.get(comp[a], 0) | bits
    flags = np.array([flag_of.get(comp[k], 0) for k in range(n)], dtype=np.int64)
    return np.array(comp, dtype=np.int64), c, flags


def rg2_fixed(sq, lo, hi, s):
    """The ONE fp64 expression of pse_cluster_word.h on the integer sums, in Python floats."""
    n = float(s)
    x, y, z = float(sq[0]), float(sq[1]), float(sq[2])
    S2 = float(hi) * 4294967296.0 + float(lo)
    m2 = (x * x + y * y) + z * z
    M = m2 / (n * n)
    return (S2 / n - M) * 2.0 ** -40


def span(pos, box, types, ntypes, rlink, port, excl=None, ids=None, nhist=None, exempt=()):
    """The whole reference in one call: a dict with label, size, stats, hist (cluster_ref), span, image (n, 3), rg2 (exact, rounded
    once), rg2_fixed, rg2_bound, pstats (8), clear (links), q_margin, tie."""
    pos = np.asarray(pos, dtype=float)
    n = len(pos)
    (i, j), clear = cr.links(pos, box, types, ntypes, rlink, port, excl, ids, exempt)
    label, size, stats, hist = cr.outputs(cr.components(n, i, j), ids, nhist)
    shift, tie = shifts(pos, box, i, j)
    comp, c, flags = unfold(n, i, j, shift, ids)
    caller = np.arange(n) if ids is None else np.asarray(ids, dtype=np.int64)
    assert np.array_equal(caller[comp], label)
    image = np.array([[0, 0, 0] if flags[k] else list(c[k]) for k in range(n)], dtype=np.int64).reshape(n, 3)
    Lx, Ly, Lz, xy = (float(b) for b in box)
    r0 = pos[comp]
    im = image.astype(float)
    D = np.empty((n, 3))
    D[:, 0] = ((pos[:, 0] - r0[:, 0]) + im[:, 0] * Lx) + im[:, 1] * (xy * Ly)
    D[:, 1] = (pos[:, 1] - r0[:, 1]) + im[:, 1] * Ly
    D[:, 2] = (pos[:, 2] - r0[:, 2]) + im[:, 2] * Lz
    t = D * Q_SCALE
    free = flags == 0
    q_margin = float(np.abs(np.abs(t[free] - np.floor(t[free])) - 0.5).min()) if free.any() else np.inf
    q = np.rint(t).astype(np.int64).tolist()
    sums = {}
    for k in range(n):
        if free[k]:
            e = sums.setdefault(int(comp[k]), [0, 0, 0, 0, 0, 0])       # sum q (3), lo, hi, members
            for a in range(3):
                e[a] += q[k][a]
                e[3] += (q[k][a] * q[k][a]) & 0xffffffff
                e[4] += (q[k][a] * q[k][a]) >> 32
            e[5] += 1
    rg2, fixed, bound = np.full(n, -1.0), np.full(n, -1.0), np.zeros(n)
    for root, (sx, sy, sz, lo, hi, s) in sums.items():
        S2 = (hi << 32) + lo
        exact = (Fraction(S2, s) - Fraction(sx * sx + sy * sy + sz * sz, s * s)) / (1 << 40)
        assert exact >= 0
        m = comp == root
        rg2[m], fixed[m] = float(exact), rg2_fixed((sx, sy, sz), lo, hi, s)
        bound[m] = RG2_ULPS * 2.0 ** -53 * 2.0 ** -40 * (S2 / s)
    roots = np.nonzero(comp == np.arange(n))[0]
    f, s = flags[roots], size[roots]
    fin = s[f == 0]
    pstats = np.array([(f != 0).sum(), s[f != 0].sum(), ((f & 1) != 0).sum(), ((f & 2) != 0).sum(), ((f & 4) != 0).sum(), (f == 7).sum(),
                       fin.max() if len(fin) else 0, (fin.astype(np.int64) ** 2).sum()], dtype=np.int64)
    return dict(label=label, size=size, stats=stats, hist=hist, span=flags, image=image, rg2=rg2, rg2_fixed=fixed, rg2_bound=bound,
                pstats=pstats, clear=clear, q_margin=q_margin, tie=tie, comp=comp, links=(i, j), shifts=shift)


def assert_clear(ref):
    cr.assert_clear(ref["clear"])
    assert ref["q_margin"] >= Q_CLEAR, ("a D 2^20 within 1e-6 of a half-integer: change the input", ref["q_margin"])
    assert ref["tie"] >= 1e-9, ("a link within 1e-9 of a tie of rint", ref["tie"])


def unfolded(pos, image, box):
    return np.asarray(pos, dtype=float)[:, :3] + np.asarray(image, dtype=float) @ lattice(box)


# ---- the planted inputs of the two test modules -------------------------------------------------------------------------------------
# Each returns positions inside the primary cell of its box; the tests fix the link distance.

def wrap(pos, box):
    """The positions folded into the primary cell -L/2 <= s < L/2 of the lattice coordinates."""
    A = lattice(box)
    s = np.asarray(pos, dtype=float) @ np.linalg.inv(A)
    return (s - np.floor(s + 0.5)) @ A


def rod(box, direction, start, spacing=1.75):
    """Equally spaced particles along the lattice vector sum_k direction[k] a_k, from `start` once round: ceil(|v| / spacing) of them
    (eight at 1.75 along an axis of the 14^3 box), so that the last is one spacing short of the first's image."""
    v = np.asarray(direction, dtype=float) @ lattice(box)
    m = int(np.ceil(np.linalg.norm(v) / spacing - 1e-12))
    return wrap(np.asarray(start, dtype=float) + np.arange(m)[:, None] * v / m, box)


def double_helix(box, R=1.5, M=20):
    """M points on a helix round x that advances TWO box lengths in one turn: the points k and k + M/2 share x (mod Lx) on opposite
    sides of the axis, 2 R apart, so after one box length the walk is NOT back; it closes after two.  Winding (2, 0, 0)."""
    k = np.arange(M)
    th = 2.0 * np.pi * k / M
    x = -0.5 * box[0] + 0.35 + 2.0 * box[0] * k / M
    return wrap(np.stack([x, R * np.cos(th), R * np.sin(th)], axis=1), box)


def six_turn_helix(box, closed, R=2.5, M=60):
    """One turn of a helix round x over SIX box lengths: six passes through the box, 60 degrees and a chord R apart.  closed: all M
    points, the last links to the first through the face (winding 6); open: the last two are left out."""
    k = np.arange(M if closed else M - 2)
    th = 2.0 * np.pi * k / M
    x = -0.5 * box[0] + 0.35 + 6.0 * box[0] * k / M
    return wrap(np.stack([x, R * np.cos(th), R * np.sin(th)], axis=1), box)


def c_shape(box):
    """Ten beads at unit spacing: out through the +x face, up, and back in through it."""
    x0 = 0.5 * box[0] - 1.7
    pts = [(x0 + k, 0.0, 0.0) for k in range(4)] + [(x0 + 3, float(k), 0.0) for k in (1, 2)] + [(x0 + 3 - k, 3.0, 0.0) for k in range(4)]
    return wrap(np.array(pts), box)


# ---- the inputs of tests/test_gpu_percolation.py, listed once so that tests/test_percolation_cpu.py can hold every one to the margins ----
import math  # noqa: E402

from pair_table_ref import random_points  # noqa: E402

CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
GRID_TILTED = (14.0, 11.0, 17.0, 0.25)           # xy Ly = 2.75: every lattice vector a multiple of 2^-10
NMAX = 513
SEED = 14                                         # picked by tests/test_percolation_cpu.py (the random regimes, the margins)
RCUT = math.sqrt(-math.log(1e-3)) / 0.5           # the engine's cutoff at xi = 0.5, error = 1e-3
NS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
RLINKS = (1.0, 1.5, 1.8, 2.2, 3.0, RCUT)
UP, DOWN = 1.75 * (1.0 + 1e-6), 1.75 * (1.0 - 1e-6)
START = (0.3, -1.1, 2.2)


def random_regimes(box):
    """(n, rlink, positions): the first n of the 513 seeded points of the box at every link distance."""
    pts = random_points(NMAX, box, seed=SEED)
    for n in NS:
        for rlink in RLINKS:
            yield n, rlink, pts[:n]


def grid_points(n, box, seed=5):
    """n points of the box whose coordinates are multiples of 2^-10."""
    rng = np.random.default_rng(seed)
    L = np.array(box[:3])
    return wrap(rng.integers(0, (L * 1024).astype(np.int64), size=(n, 3)) / 1024.0, box)   # (the lattice vectors are such multiples too)


def two_rods_and_a_cloud(box):
    cloud = random_points(120, box, seed=SEED + 1)
    return np.concatenate([rod(box, (1, 0, 0), (0.2, -4.9, -5.1)), rod(box, (0, 0, 1), (3.1, 3.3, 0.4)), cloud])


def closed_chain():
    """The 512-bead boustrophedon chain of the cluster tests, and the same with one more bead that closes its first row through the x face."""
    from test_gpu_clusters import serpentine
    chain = serpentine(512, 0.9)
    bridge = np.array([[chain[14, 0] + 0.7, chain[0, 1], chain[0, 2]]])
    assert abs(chain[14, 0] + 1.4 - 14.0 - chain[0, 0]) < 1e-12
    return chain, np.concatenate([chain, bridge])


def planted():
    """name -> (positions, box, keywords of span(): rlink, and types / ntypes / excl where the case has them)."""
    from test_gpu_clusters import lattice as shuffled_lattice
    out = {}
    for bname, box in (("cubic", CUBIC), ("tilted", TILTED)):
        for k, direction in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            out[f"rod_a{k + 1}_{bname}"] = (rod(box, direction, START), box, dict(rlink=UP))
        out[f"double_helix_{bname}"] = (double_helix(box), box, dict(rlink=UP))
        out[f"open_helix_{bname}"] = (six_turn_helix(box, False), box, dict(rlink=UP))
        out[f"closed_helix_{bname}"] = (six_turn_helix(box, True), box, dict(rlink=UP))
        out[f"c_shape_{bname}"] = (c_shape(box), box, dict(rlink=1.2))
        out[f"two_rods_and_a_cloud_{bname}"] = (two_rods_and_a_cloud(box), box, dict(rlink=UP))
    for k in range(3):
        out[f"rod_a{k + 1}_short"] = (out[f"rod_a{k + 1}_cubic"][0], CUBIC, dict(rlink=DOWN))
    out["rod_110"] = (rod(CUBIC, (1, 1, 0), START), CUBIC, dict(rlink=UP))
    out["rod_111"] = (rod(CUBIC, (1, 1, 1), START), CUBIC, dict(rlink=UP))
    out["lattice"] = (shuffled_lattice()[0], CUBIC, dict(rlink=UP))
    chain, closed = closed_chain()
    out["chain"] = (chain, CUBIC, dict(rlink=1.0))
    out["chain_closed"] = (closed, CUBIC, dict(rlink=1.0))
    for name, order in (("reversed", np.arange(NMAX)[::-1]), ("shuffled", np.random.default_rng(9).permutation(NMAX))):
        out[f"chain_closed_{name}"] = (closed[order], CUBIC, dict(rlink=1.0))
    x = rod(CUBIC, (1, 0, 0), START)
    out["rod_excluded_pair"] = (x, CUBIC, dict(rlink=UP, excl=np.array([[0, 1]])))
    out["rod_pair_type_off"] = (x, CUBIC, dict(rlink={(0, 0): UP, (1, 1): UP}, types=np.array([0, 0, 0, 0, 1, 1, 1, 1]), ntypes=2))
    out["rod_pair_type_on"] = (x, CUBIC, dict(rlink=UP, types=np.array([0, 0, 0, 0, 1, 1, 1, 1]), ntypes=2))
    for bname, box in (("cubic", CUBIC), ("grid_tilted", GRID_TILTED)):
        out[f"grid_{bname}"] = (grid_points(450, box), box, dict(rlink=1.5))
        out[f"grid_rod_{bname}"] = (np.concatenate([grid_points(100, box, seed=6), rod(box, (1, 0, 0), (-7.0, 5.0, 6.0))]), box, dict(rlink=UP))
    return out


def gpu_inputs():
    """(name, positions, box, keywords) of every input the GPU tests compare on."""
    for bname, box in (("cubic", CUBIC), ("tilted", TILTED)):
        for n, rlink, pos in random_regimes(box):
            yield f"random_{bname}_{n}_{rlink:.2f}", pos, box, dict(rlink=rlink)
    for name, (pos, box, kw) in planted().items():
        yield name, pos, box, kw
    pos = two_rods_and_a_cloud(CUBIC)                                      # the group of the switches: every particle but the rod's fourth
    yield "group", np.delete(pos, 3, axis=0), CUBIC, dict(rlink=UP)
