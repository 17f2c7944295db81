"""NumPy reference of the angle forces and their observables (pse_angle_forces), shared by tests/test_angle_reference.py (which
validates it) and tests/test_gpu_angles.py (which compares the device to it), and generators of angle topologies whose angles are
PRESCRIBED or asserted, so that every angle of a test is where the bound of the GPU tests can hold.

Per angle (i, j, k) of type t, j the vertex: d1 = r_i - r_j, d2 = r_k - r_j (oracle.pse_port.min_image), r1 = |d1|, r2 = |d2|,
c = d1.d2 / (r1 r2) clamped to [-1, 1] and
  harmonic (kind 0)  V = k/2 (theta - theta0)^2, theta = acos(c),  g = k (theta - theta0) / max(sqrt(1 - c^2), 1e-3)
  cosinesq (kind 1)  V = k/2 (c - cos theta0)^2,                   g = -k (c - cos theta0)
  F_i = g (d2/(r1 r2) - c d1/r1^2),  F_k = g (d1/(r1 r2) - c d2/r2^2),  F_j = -(F_i + F_k)
An angle with r1 == 0 or r2 == 0 does nothing.  U = sum V, W_ab = sum (d1_a F_i,b + d2_a F_k,b), nangles = the number of angles
that acted.  The angles are put into a canonical order (lower end first, sorted by (i, j, k, type)) before anything is summed, so
the result is exactly independent of the order of the list and of the order of an angle's ends.

Why sin(theta) >= SIN_MIN on the inputs: theta = acos(c) has the derivative -1/sin(theta), and the force carries another 1/sin(theta),
so a rounding error eps of c becomes k eps / sin^2(theta) in g; two correct acos implementations (NumPy's and the device's) can then
differ by that much.  With sin(theta) >= 0.05 that is 400 k eps ~ 3e-12 for k = 30, inside 1e-11; nearer the straight angle it is not.
Not a test module: nothing here is collected."""
import numpy as np

import bond_ref as br

NAMES = ("U", "Wxx", "Wxy", "Wxz", "Wyy", "Wyz", "Wzz", "nangles")
HARMONIC, COSINESQ = 0, 1
S_FLOOR = 1e-3
SIN_MIN = 0.05


def canonical(triples, types):
    """(i, j, k, t) with i < k, sorted by (i, j, k, t)."""
    tr = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    t = np.zeros(len(tr), dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    i, j, k = np.minimum(tr[:, 0], tr[:, 2]), tr[:, 1], np.maximum(tr[:, 0], tr[:, 2])
    o = np.lexsort((t, k, j, i))
    return i[o], j[o], k[o], t[o]


def angle_terms(pos, box, triples, types, kinds, k, theta0, port):
    """dict of per-angle arrays in canonical order: i, j, k, d1, d2, c (the clamped cosine), V, Fi, Fk, acts; V, Fi, Fk are zero
    where the angle does not act."""
    pos = np.asarray(pos, dtype=float)
    i, j, kk_, t = canonical(triples, types)
    kind, K, th0 = np.asarray(kinds, dtype=np.int64)[t], np.asarray(k, dtype=float)[t], np.asarray(theta0, dtype=float)[t]
    d1 = port.min_image(pos[i] - pos[j], box)
    d2 = port.min_image(pos[kk_] - pos[j], box)
    r1sq, r2sq = (d1 * d1).sum(axis=1), (d2 * d2).sum(axis=1)
    acts = (r1sq > 0.0) & (r2sq > 0.0)
    a1, a2 = np.where(acts, r1sq, 1.0), np.where(acts, r2sq, 1.0)
    ir12 = 1.0 / (np.sqrt(a1) * np.sqrt(a2))
    c = np.clip((d1 * d2).sum(axis=1) * ir12, -1.0, 1.0)
    harm = kind == HARMONIC
    dth = np.arccos(c) - th0
    dc = c - np.cos(th0)
    g = np.where(harm, K * dth / np.maximum(np.sqrt(1.0 - c * c), S_FLOOR), -K * dc)
    V = np.where(harm, 0.5 * K * dth * dth, 0.5 * K * dc * dc)
    Fi = g[:, None] * (d2 * ir12[:, None] - (c / a1)[:, None] * d1)
    Fk = g[:, None] * (d1 * ir12[:, None] - (c / a2)[:, None] * d2)
    m = acts[:, None]
    return dict(i=i, j=j, k=kk_, d1=d1, d2=d2, c=c, V=np.where(acts, V, 0.0), Fi=np.where(m, Fi, 0.0), Fk=np.where(m, Fk, 0.0), acts=acts)


def virial_tensor(terms):
    """The full 3 x 3 W_ab = sum (d1_a F_i,b + d2_a F_k,b): nothing is symmetrised."""
    return np.einsum("na,nb->ab", terms["d1"], terms["Fi"]) + np.einsum("na,nb->ab", terms["d2"], terms["Fk"])


def angle_observables(pos, box, triples, types, kinds, k, theta0, port):
    """(obs[8], F[n, 3]): U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, nangles; the forces of the same angle sum."""
    q = angle_terms(pos, box, triples, types, kinds, k, theta0, port)
    obs = np.zeros(8)
    obs[0] = q["V"].sum()
    for n, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        obs[1 + n] = (q["d1"][:, a] * q["Fi"][:, b] + q["d2"][:, a] * q["Fk"][:, b]).sum()
    obs[7] = float(q["acts"].sum())
    F = np.zeros((len(pos), 3))
    np.add.at(F, q["i"], q["Fi"])
    np.add.at(F, q["k"], q["Fk"])
    np.add.at(F, q["j"], -(q["Fi"] + q["Fk"]))
    return obs, F


def sines(pos, box, triples, port):
    """sin(theta) of every angle of a list whose arms both have a length (for the assertion that a test's angles are where the bound
    needs them): from the cross product, which is accurate near the straight angle where sqrt(1 - c^2) is not."""
    tr = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    pos = np.asarray(pos, dtype=float)
    d1 = port.min_image(pos[tr[:, 0]] - pos[tr[:, 1]], box)
    d2 = port.min_image(pos[tr[:, 2]] - pos[tr[:, 1]], box)
    r = np.linalg.norm(d1, axis=1) * np.linalg.norm(d2, axis=1)
    return np.linalg.norm(np.cross(d1, d2), axis=1)[r > 0.0] / r[r > 0.0]


def arm_lengths(pos, box, triples, port):
    tr = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    pos = np.asarray(pos, dtype=float)
    d1 = port.min_image(pos[tr[:, 0]] - pos[tr[:, 1]], box)
    d2 = port.min_image(pos[tr[:, 2]] - pos[tr[:, 1]], box)
    return np.concatenate([np.linalg.norm(d1, axis=1), np.linalg.norm(d2, axis=1)])


# ---- generators ----------------------------------------------------------------------------------------------------------------
BOXES = br.BOXES
N_MAX = 513
N_TOPOLOGY = 300
ROW_COUNTS = (3, 63, 64, 65, 255, 256, 257, 513)
TOPOLOGIES = ("chains", "ring", "star", "duplicates", "two_types", "faces")
K_H, TH0_H = 30.0, 2.2      # harmonic
K_C, TH0_C = 30.0, 2.6      # cosine-squared
PARAMS = {HARMONIC: (K_H, TH0_H), COSINESQ: (K_C, TH0_C)}
THETA_RANGE = (0.35, 2.9)   # the prescribed vertex angles of the chains: sin >= 0.239
ARM_RANGE = (0.6, 1.6)


def bent_chains(nchains, beads, box, seed, port, first=0):
    """nchains chains of `beads` beads from uniform random starts, wrapped into the tilted box: bond lengths uniform in ARM_RANGE,
    and the angle at every inner bead uniform in THETA_RANGE about a random azimuth -- prescribed, so that no angle comes near 0 or
    pi.  Returns (pos, triples): the particles first .. first + nchains * beads - 1 in chain order, one angle per inner bead."""
    rng = np.random.default_rng(seed)
    Lx, Ly, Lz, _ = box
    pos, triples = [], []
    for ch in range(nchains):
        start = (rng.uniform(size=3) - 0.5) * np.array([Lx, Ly, Lz])
        u = br._directions(rng, 1)[0]
        walk = [start]
        for s in range(beads - 1):
            if s > 0:
                theta = rng.uniform(*THETA_RANGE)              # the angle at bead s between -u (back) and the new direction
                v = np.cross(u, br._directions(rng, 1)[0]); v /= np.linalg.norm(v)
                u = -np.cos(theta) * u + np.sin(theta) * v
                u /= np.linalg.norm(u)
            walk.append(walk[-1] + rng.uniform(*ARM_RANGE) * u)
        pos.append(np.array(walk))
        b = first + ch * beads + np.arange(1, beads - 1)
        triples.append(np.stack([b - 1, b, b + 1], axis=1))
    return br._wrap(np.vstack(pos), box, port), np.vstack(triples)


def _case(pos, triples, types, kinds, theta0=None, collinear=0):
    kinds = list(kinds)
    out = dict(pos=pos, triples=np.asarray(triples, dtype=np.int64), types=None if types is None else np.asarray(types, dtype=np.int64),
               kinds=kinds, k=[PARAMS[q][0] for q in kinds], theta0=[PARAMS[q][1] for q in kinds] if theta0 is None else list(theta0),
               collinear=collinear)
    for a in (out["pos"], out["triples"]) + (() if types is None else (out["types"],)):
        a.setflags(write=False)
    return out


def chain_case(n, box, kind, port):
    """One chain of n beads: n - 2 angles."""
    pos, triples = bent_chains(1, n, box, 300 + n, port)
    return _case(pos, triples, None, [kind])


def topology_case(name, box, kind, port):
    """The topologies of the GPU tests at N_TOPOLOGY particles, each with particles in no angle; `kind` is the potential of the
    single-type ones."""
    n = N_TOPOLOGY
    if name == "chains":            # eight chains of 30 and 60 particles in no angle
        pos, triples = bent_chains(8, 30, box, 31, port)
        return _case(br._pad(pos, n, box, 32), triples, None, [kind])
    if name == "ring":              # 100 beads, zigzag about a regular polygon: every angle, the closing ones included, the same
        pos, pairs = br.ring(100, box, 1.0, 0.5, 33, port)
        b = np.arange(100)
        return _case(br._pad(pos, n, box, 34), np.stack([(b - 1) % 100, b, (b + 1) % 100], axis=1), None, [kind])
    if name == "star":              # a hub that is the vertex of 40 angles between its 12 arms: one long row
        rng = np.random.default_rng(35)
        pos, pairs = br.star(12, box, rng.uniform(*ARM_RANGE, 12), 36, port)
        a, b = np.triu_indices(12, 1)
        pick = rng.permutation(len(a))[:40]
        return _case(br._pad(pos, n, box, 37), np.stack([1 + a[pick], np.zeros(40, dtype=np.int64), 1 + b[pick]], axis=1), None, [kind])
    if name == "duplicates":        # every third angle of a chain twice (the copy with swapped ends), one of them three times
        pos, triples = bent_chains(1, 100, box, 38, port)
        triples = np.vstack([triples, triples[::3, ::-1], triples[3:4]])
        return _case(br._pad(pos, n, box, 39), triples, None, [kind])
    if name == "two_types":         # harmonic and cosine-squared angles alternating along four chains, different theta0
        pos, triples = bent_chains(4, 50, box, 40, port)
        types = np.arange(len(triples)) % 2
        return _case(br._pad(pos, n, box, 41), triples, types, [kind, COSINESQ if kind == HARMONIC else HARMONIC])
    if name == "faces":             # vertices next to the x, y and z faces and the xy edge, both ends beyond: a y crossing shifts x by xy Ly
        Lx, Ly, Lz, xy = box
        v = np.array([[0.5 * Lx - 0.2, 0.3, -1.0], [1.0 + xy * (0.5 * Ly - 0.2), 0.5 * Ly - 0.2, 2.0], [-2.0, -1.0, 0.5 * Lz - 0.2],
                      [0.5 * Lx - 0.1 + xy * (0.5 * Ly - 0.1), 0.5 * Ly - 0.1, 0.0]])
        u1 = np.array([[0.8, 0.36, 0.48], [0.36, 0.8, -0.48], [0.48, -0.36, 0.8], [0.6, 0.64, 0.48]])
        u2 = np.array([[0.8, -0.48, -0.36], [-0.48, 0.8, 0.36], [-0.36, 0.48, 0.8], [0.64, 0.6, -0.48]])
        u1 /= np.linalg.norm(u1, axis=1)[:, None]; u2 /= np.linalg.norm(u2, axis=1)[:, None]
        pos = br._wrap(np.vstack([v, v + 1.1 * u1, v + 1.4 * u2]), box, port)    # the ends lie beyond the face and are stored wrapped
        assert np.abs(pos[4:8] - pos[:4]).max(axis=1).min() > 5.0 and np.abs(pos[8:] - pos[:4]).max(axis=1).min() > 5.0
        q = np.arange(4)
        return _case(br._pad(pos, n, box, 42), np.stack([4 + q, q, 8 + q], axis=1), None, [kind])
    raise KeyError(name)


def graph_case(box, kind, port):
    """150 random triples (repeats possible) among 60 points of a ball of diameter 3 and 240 particles in no angle: rows of every
    length, every role, in no order.  The angles are whatever the points give: the seed is one for which all have sin >= SIN_MIN
    (tests/test_angle_reference.py asserts it)."""
    rng = np.random.default_rng(53)
    m = 60
    pos = br._directions(rng, m) * (1.5 * rng.uniform(size=m) ** (1.0 / 3.0))[:, None] + rng.uniform(-1.0, 1.0, 3)
    i = rng.integers(0, m, 150)
    j = (i + rng.integers(1, m, 150)) % m
    k = rng.integers(0, m, 150)
    clash = (k == i) | (k == j)
    while clash.any():
        k[clash] = rng.integers(0, m, int(clash.sum()))
        clash = (k == i) | (k == j)
    return _case(br._pad(br._wrap(pos, box, port), N_TOPOLOGY, box, 44), np.stack([i, j, k], axis=1), None, [kind])


def collinear_case(box, port):
    """Exactly straight and exactly folded triples along x, at coordinates and arm lengths (1 and 2) for which d1, d2, r1 r2 and c
    are exact in binary: c is exactly -1 or +1 and the bracket of the force exactly zero, whatever multiplies it.  The straight
    triple (0, 1, 2) carries a harmonic angle with theta0 = pi and cosine-squared ones with theta0 = pi and 2.6; the folded one
    (3, 4, 5) all four types; a generic angle (6, 7, 8) keeps the forces of the case away from zero.  Three + four collinear angles."""
    v = np.array([0.5, 0.25, -1.0])
    w = np.array([-2.5, 1.5, 3.0])
    g = np.array([2.0, -3.0, 0.5])
    ex = np.array([1.0, 0.0, 0.0])
    pos = np.array([v - ex, v, v + 2.0 * ex, w + ex, w, w + 2.0 * ex, g + [0.9, 0.2, 0.1], g, g + [-0.3, 1.0, 0.4]])
    triples = [[0, 1, 2]] * 3 + [[3, 4, 5]] * 4 + [[6, 7, 8]]
    types = [0, 1, 2, 0, 1, 2, 3, 3]
    c = _case(br._pad(pos, N_TOPOLOGY, box, 45), triples, types, [HARMONIC, COSINESQ, COSINESQ, HARMONIC],
              theta0=[np.pi, np.pi, 2.6, 2.0], collinear=7)
    return c


def all_cases(port):
    """(label, box, case) of every fixed input of the GPU tests."""
    for box in BOXES:
        for kind in (HARMONIC, COSINESQ):
            for n in ROW_COUNTS:
                yield f"chain{n}", box, chain_case(n, box, kind, port)
            for name in TOPOLOGIES:
                yield name, box, topology_case(name, box, kind, port)
            yield "graph", box, graph_case(box, kind, port)
        yield "collinear", box, collinear_case(box, port)
