"""NumPy reference of the dihedral forces and their observables (pse_dihedral_forces), shared by tests/test_dihedral_reference.py
(which validates it) and tests/test_gpu_dihedrals.py (which compares the device to it), and generators of dihedral topologies whose
bond angles are PRESCRIBED or asserted, so that every dihedral of a test is where the bound of the GPU tests can hold.

Per dihedral (i, j, k, l) of type t: d1 = r_i - r_j, d2 = r_k - r_j, d3 = r_k - r_l (oracle.pse_port.min_image), m = d1 x d2,
nn = d2 x d3, b = |d2|, phi = arctan2(b d1.nn, m.nn) in (-pi, pi] (IUPAC: cis 0, trans pi) and
  harmonic (kind 0)  params (k, d, mult, phi0): V = k/2 (1 + d cos(mult phi - phi0)),  g = dV/dphi = -k d mult/2 sin(mult phi - phi0)
  OPLS     (kind 1)  params (k1, k2, k3, k4):   V = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2phi) + k3 (1 + cos 3phi) + k4 (1 - cos 4phi)]
  F_i = -g b/|m|^2 m,  F_l = g b/|nn|^2 nn,  s = d1.d2/b^2,  t = d3.d2/b^2,  F_j = -F_i + s F_i - t F_l,  F_k = -F_l - s F_i + t F_l
A dihedral with |m|^2 == 0 or |nn|^2 == 0 does nothing.  U = sum V, W_ab = sum (d1_a F_i,b + d2_a F_k,b + (d2 - d3)_a F_l,b),
ndihedrals = the number of dihedrals that acted.  The dihedrals are put into a canonical order ((l, k, j, i) for (i, j, k, l) where
l < i, sorted by (i, j, k, l, type)) before anything is summed, so the result is exactly independent of the order of the list and of
the direction a quadruple is written in.

Why both bond angles have sin >= SIN_MIN on the inputs: F_i = -g b m/|m|^2 has the size g / (r1 sin(theta_ijk)), and a rounding error
eps of the positions' differences turns m by eps / sin(theta_ijk), which moves phi -- and with it g -- by as much: two correct
evaluations (NumPy's with arctan2, the device's without) can differ by k mult^2 eps / sin^2 relative to k mult / (r sin).  With
sin >= 0.05 that stays some 1e-13 of the largest force; nearer the straight angle it does not.
Not a test module: nothing here is collected."""
import numpy as np

import angle_ref as ar
import bond_ref as br

NAMES = ("U", "Wxx", "Wxy", "Wxz", "Wyy", "Wyz", "Wzz", "ndihedrals")
HARMONIC, OPLS = 0, 1
SIN_MIN = 0.05


def canonical(quads, types):
    """(i, j, k, l, t) with i < l, sorted by (i, j, k, l, t)."""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    t = np.zeros(len(q), dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    q = np.where((q[:, 3] < q[:, 0])[:, None], q[:, ::-1], q)
    o = np.lexsort((t, q[:, 3], q[:, 2], q[:, 1], q[:, 0]))
    return q[o, 0], q[o, 1], q[o, 2], q[o, 3], t[o]


def energy_and_slope(phi, kind, par):
    """V(phi) and dV/dphi per dihedral: kind (n,), par (n, 4)."""
    p0, p1, p2, p3 = par.T
    x = p2 * phi - p3
    Vh, gh = 0.5 * p0 * (1.0 + p1 * np.cos(x)), -0.5 * p0 * p1 * p2 * np.sin(x)
    Vo = 0.5 * (p0 * (1.0 + np.cos(phi)) + p1 * (1.0 - np.cos(2.0 * phi)) + p2 * (1.0 + np.cos(3.0 * phi)) + p3 * (1.0 - np.cos(4.0 * phi)))
    go = 0.5 * (-p0 * np.sin(phi) + 2.0 * p1 * np.sin(2.0 * phi) - 3.0 * p2 * np.sin(3.0 * phi) + 4.0 * p3 * np.sin(4.0 * phi))
    harm = kind == HARMONIC
    return np.where(harm, Vh, Vo), np.where(harm, gh, go)


def dihedral_terms(pos, box, quads, types, kinds, params, port):
    """dict of per-dihedral arrays in canonical order: i, j, k, l, d1, d2, d3, phi, V, Fi, Fj, Fk, Fl, acts; V and the forces are
    zero (and phi is 0) where the dihedral does not act."""
    pos = np.asarray(pos, dtype=float)
    i, j, k, l, t = canonical(quads, types)
    kind, par = np.asarray(kinds, dtype=np.int64)[t], np.asarray(params, dtype=float).reshape(-1, 4)[t]
    d1 = port.min_image(pos[i] - pos[j], box)
    d2 = port.min_image(pos[k] - pos[j], box)
    d3 = port.min_image(pos[k] - pos[l], box)
    m, nn = np.cross(d1, d2), np.cross(d2, d3)
    m2, n2 = (m * m).sum(axis=1), (nn * nn).sum(axis=1)
    acts = (m2 > 0.0) & (n2 > 0.0)
    b2 = (d2 * d2).sum(axis=1)
    b = np.sqrt(b2)
    phi = np.where(acts, np.arctan2(b * (d1 * nn).sum(axis=1), (m * nn).sum(axis=1)), 0.0)
    V, g = energy_and_slope(phi, kind, par)
    sm2, sn2, sb2 = np.where(acts, m2, 1.0), np.where(acts, n2, 1.0), np.where(acts, b2, 1.0)
    Fi = (-g * b / sm2)[:, None] * m
    Fl = (g * b / sn2)[:, None] * nn
    s, tt = ((d1 * d2).sum(axis=1) / sb2)[:, None], ((d3 * d2).sum(axis=1) / sb2)[:, None]
    Fj = -Fi + s * Fi - tt * Fl
    Fk = -Fl - s * Fi + tt * Fl
    a = acts[:, None]
    return dict(i=i, j=j, k=k, l=l, d1=d1, d2=d2, d3=d3, phi=phi, V=np.where(acts, V, 0.0), Fi=np.where(a, Fi, 0.0), Fj=np.where(a, Fj, 0.0),
                Fk=np.where(a, Fk, 0.0), Fl=np.where(a, Fl, 0.0), acts=acts)


def virial_tensor(q):
    """The full 3 x 3 W_ab = sum (d1_a F_i,b + d2_a F_k,b + (d2 - d3)_a F_l,b): nothing is symmetrised."""
    return (np.einsum("na,nb->ab", q["d1"], q["Fi"]) + np.einsum("na,nb->ab", q["d2"], q["Fk"])
            + np.einsum("na,nb->ab", q["d2"] - q["d3"], q["Fl"]))


def dihedral_observables(pos, box, quads, types, kinds, params, port):
    """(obs[8], F[n, 3]): U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, ndihedrals; the forces of the same dihedral sum."""
    q = dihedral_terms(pos, box, quads, types, kinds, params, port)
    W = virial_tensor(q)
    obs = np.array([q["V"].sum(), W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2], float(q["acts"].sum())])
    F = np.zeros((len(pos), 3))
    for who, f in (("i", "Fi"), ("j", "Fj"), ("k", "Fk"), ("l", "Fl")):
        np.add.at(F, q[who], q[f])
    return obs, F


def sines(pos, box, quads, port):
    """sin of the two bond angles (at j and at k) of every dihedral of a list whose three arms all have a length, from the cross
    products (for the assertion that a test's dihedrals are where the bound needs them)."""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    pos = np.asarray(pos, dtype=float)
    d1 = port.min_image(pos[q[:, 0]] - pos[q[:, 1]], box)
    d2 = port.min_image(pos[q[:, 2]] - pos[q[:, 1]], box)
    d3 = port.min_image(pos[q[:, 2]] - pos[q[:, 3]], box)
    r1, r2, r3 = (np.linalg.norm(d, axis=1) for d in (d1, d2, d3))
    ok = (r1 > 0.0) & (r2 > 0.0) & (r3 > 0.0)
    sj = np.linalg.norm(np.cross(d1, d2), axis=1)[ok] / (r1 * r2)[ok]
    sk = np.linalg.norm(np.cross(d2, d3), axis=1)[ok] / (r2 * r3)[ok]
    return np.concatenate([sj, sk])


def arm_lengths(pos, box, quads, port):
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    pos = np.asarray(pos, dtype=float)
    return np.concatenate([np.linalg.norm(port.min_image(pos[q[:, a]] - pos[q[:, a + 1]], box), axis=1) for a in range(3)])


# ---- generators ----------------------------------------------------------------------------------------------------------------
BOXES = br.BOXES
N_MAX = 513
N_TOPOLOGY = 300
ROW_COUNTS = (4, 63, 64, 65, 255, 256, 257, 513)
TOPOLOGIES = ("chains", "ring", "star", "duplicates", "two_types", "faces")
PARAMS = {HARMONIC: (30.0, -1.0, 3.0, 0.7), OPLS: (15.0, -8.0, 12.0, 5.0)}
ARM_RANGE = ar.ARM_RANGE        # the arms of the chains; the graph's lie in GRAPH_ARM_RANGE
GRAPH_ARM_RANGE = (0.05, 3.0)


def bent_chains(nchains, beads, box, seed, port, first=0):
    """The chains of angle_ref.bent_chains -- arm lengths uniform in ARM_RANGE, every bond angle uniform in angle_ref.THETA_RANGE
    (sin >= 0.239) about a random azimuth, so the dihedral angles are uniform -- with one dihedral per four consecutive beads."""
    pos, _ = ar.bent_chains(nchains, beads, box, seed, port, first)
    b = np.concatenate([first + ch * beads + np.arange(beads - 3) for ch in range(nchains)])
    return pos, np.stack([b, b + 1, b + 2, b + 3], axis=1)


def _case(pos, quads, types, kinds, params=None, degenerate=0):
    kinds = list(kinds)
    out = dict(pos=pos, quads=np.asarray(quads, dtype=np.int64), types=None if types is None else np.asarray(types, dtype=np.int64),
               kinds=kinds, params=[PARAMS[q] for q in kinds] if params is None else [tuple(p) for p in params], degenerate=degenerate)
    for a in (out["pos"], out["quads"]) + (() if types is None else (out["types"],)):
        a.setflags(write=False)
    return out


def chain_case(n, box, kind, port):
    """One chain of n beads: n - 3 dihedrals."""
    pos, quads = bent_chains(1, n, box, 500 + n, port)
    return _case(pos, quads, None, [kind])


def _cone(rng, axis, theta):
    """A unit vector at the angle theta to `axis`, at a random azimuth."""
    v = np.cross(axis, br._directions(rng, 1)[0]); v /= np.linalg.norm(v)
    return np.cos(theta) * axis + np.sin(theta) * v


def topology_case(name, box, kind, port):
    """The topologies of the GPU tests at N_TOPOLOGY particles, each with particles in no dihedral; `kind` is the potential of the
    single-type ones."""
    n = N_TOPOLOGY
    if name == "chains":            # eight chains of 30 and 60 particles in no dihedral
        pos, quads = bent_chains(8, 30, box, 61, port)
        return _case(br._pad(pos, n, box, 62), quads, None, [kind])
    if name == "ring":              # 100 beads, zigzag about a regular polygon: every dihedral, the closing ones included
        pos, _ = br.ring(100, box, 1.0, 0.5, 63, port)
        b = np.arange(100)
        return _case(br._pad(pos, n, box, 64), np.stack([b, (b + 1) % 100, (b + 2) % 100, (b + 3) % 100], axis=1), None, [kind])
    if name == "star":              # one central bond 0-1 shared by 40 dihedrals between 6 arms at 0 and 7 at 1: two long rows
        rng = np.random.default_rng(65)
        hub = rng.uniform(-1.0, 1.0, 3)
        u = br._directions(rng, 1)[0]
        pj, pk = hub, hub + rng.uniform(*ARM_RANGE) * u
        ai = [pj + rng.uniform(*ARM_RANGE) * _cone(rng, u, rng.uniform(*ar.THETA_RANGE)) for _ in range(6)]
        al = [pk + rng.uniform(*ARM_RANGE) * _cone(rng, -u, rng.uniform(*ar.THETA_RANGE)) for _ in range(7)]
        pos = br._wrap(np.vstack([pj, pk] + ai + al), box, port)
        a, c = np.divmod(rng.permutation(42)[:40], 7)
        quads = np.stack([2 + a, np.zeros(40, dtype=np.int64), np.ones(40, dtype=np.int64), 8 + c], axis=1)
        return _case(br._pad(pos, n, box, 66), quads, None, [kind])
    if name == "duplicates":        # every third dihedral of a chain twice (the copy reversed), one of them three times
        pos, quads = bent_chains(1, 100, box, 67, port)
        quads = np.vstack([quads, quads[::3, ::-1], quads[3:4]])
        return _case(br._pad(pos, n, box, 68), quads, None, [kind])
    if name == "two_types":         # a harmonic and an OPLS type alternating along four chains
        pos, quads = bent_chains(4, 50, box, 69, port)
        types = np.arange(len(quads)) % 2
        return _case(br._pad(pos, n, box, 70), quads, types, [kind, OPLS if kind == HARMONIC else HARMONIC])
    if name == "faces":             # j next to the x, y and z faces and the xy edge, i, k and l beyond: a y crossing shifts x by xy Ly
        Lx, Ly, Lz, xy = box
        v = np.array([[0.5 * Lx - 0.2, 0.3, -1.0], [1.0 + xy * (0.5 * Ly - 0.2), 0.5 * Ly - 0.2, 2.0], [-2.0, -1.0, 0.5 * Lz - 0.2],
                      [0.5 * Lx - 0.1 + xy * (0.5 * Ly - 0.1), 0.5 * Ly - 0.1, 0.0]])
        u1 = np.array([[0.8, 0.36, 0.48], [0.36, 0.8, -0.48], [0.48, -0.36, 0.8], [0.6, 0.64, 0.48]])
        u2 = np.array([[0.8, -0.48, -0.36], [-0.48, 0.8, 0.36], [-0.36, 0.48, 0.8], [0.64, 0.6, -0.48]])
        u3 = np.array([[0.6, 0.0, 0.8], [0.0, 0.6, 0.8], [0.8, 0.0, 0.6], [0.48, 0.64, 0.6]])
        u1 /= np.linalg.norm(u1, axis=1)[:, None]; u2 /= np.linalg.norm(u2, axis=1)[:, None]
        pi_, pk = v + 1.1 * u1, v + 1.4 * u2
        pos = br._wrap(np.vstack([v, pi_, pk, pk + 1.2 * u3]), box, port)     # i, k, l lie beyond the face and are stored wrapped
        assert min(np.abs(pos[4 * a:4 * a + 4] - pos[:4]).max(axis=1).min() for a in (1, 2, 3)) > 5.0
        q = np.arange(4)
        return _case(br._pad(pos, n, box, 72), np.stack([4 + q, q, 8 + q, 12 + q], axis=1), None, [kind])
    raise KeyError(name)


GRAPH_SEED = 1000   # a seed whose quadruples all have sin >= SIN_MIN and arms in GRAPH_ARM_RANGE, in both boxes


def graph_case(box, kind, port, seed=None):
    """150 random quadruples (repeats possible) among 60 points of a ball of diameter 3 and 240 particles in no dihedral: rows of
    every length, every role, in no order.  The bond angles are whatever the points give: the seed is one for which all have
    sin >= SIN_MIN (tests/test_dihedral_reference.py asserts it)."""
    rng = np.random.default_rng(GRAPH_SEED if seed is None else seed)
    m = 60
    pos = br._directions(rng, m) * (1.5 * rng.uniform(size=m) ** (1.0 / 3.0))[:, None] + rng.uniform(-1.0, 1.0, 3)
    quads = np.array([rng.permutation(m)[:4] for _ in range(150)])
    return _case(br._pad(br._wrap(pos, box, port), N_TOPOLOGY, box, 74), quads, None, [kind])


def multiplicity_case(box, port):
    """Twelve harmonic types -- every multiplicity 1..6 with d = -1 and d = +1, each with a phi0 of its own -- and one OPLS type in turn
    along four chains."""
    pos, quads = bent_chains(4, 50, box, 75, port)
    params = [(30.0, d, float(mult), 0.3 * mult - 1.0) for mult in range(1, 7) for d in (-1.0, 1.0)] + [PARAMS[OPLS]]
    return _case(br._pad(pos, N_TOPOLOGY, box, 76), quads, np.arange(len(quads)) % 13, [HARMONIC] * 12 + [OPLS], params=params)


def degenerate_case(box, port):
    """Exactly collinear triples along x at coordinates and arm lengths (1 and 2) for which the differences are exact in binary, so
    that the cross product is exactly zero: (0, 1, 2, 3) has i, j, k collinear, (4, 5, 6, 7) has j, k, l collinear, (8, 9, 10, 11)
    all four; each carries both types.  A generic dihedral (12, 13, 14, 15) keeps the forces of the case away from zero.  Six
    degenerate dihedrals."""
    ex, ey, ez = np.eye(3)
    v, w, g, h = np.array([0.5, 0.25, -1.0]), np.array([-2.5, 1.5, 3.0]), np.array([2.0, -3.0, 0.5]), np.array([-1.0, -2.0, 1.5])
    pos = np.array([v - ex, v, v + 2.0 * ex, v + 2.0 * ex + ey,
                    w + ez, w, w + ex, w + 3.0 * ex,
                    g, g + ex, g + 3.0 * ex, g + 4.0 * ex,
                    h + [0.2, 0.9, 0.1], h, h + [1.0, 0.1, -0.2], h + [1.3, -0.4, 0.8]])
    quads = [[0, 1, 2, 3]] * 2 + [[4, 5, 6, 7]] * 2 + [[8, 9, 10, 11]] * 2 + [[12, 13, 14, 15]] * 2
    types = [0, 1] * 4
    return _case(br._pad(pos, N_TOPOLOGY, box, 77), quads, types, [HARMONIC, OPLS], degenerate=6)


def all_cases(port):
    """(label, box, case) of every fixed input of the GPU tests."""
    for box in BOXES:
        for kind in (HARMONIC, OPLS):
            for n in ROW_COUNTS:
                yield f"chain{n}", box, chain_case(n, box, kind, port)
            for name in TOPOLOGIES:
                yield name, box, topology_case(name, box, kind, port)
            yield "graph", box, graph_case(box, kind, port)
        yield "multiplicity", box, multiplicity_case(box, port)
        yield "degenerate", box, degenerate_case(box, port)
