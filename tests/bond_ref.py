"""NumPy reference of the bonded forces and their observables (pse_bond_forces), shared by tests/test_bond_reference.py (which
validates it) and tests/test_gpu_bonds.py (which compares the device to it), and generators of bond topologies whose bond lengths
are PRESCRIBED, so that every FENE bond of a test is where the test wants it.

Per bond (i, j) of type t with d = r_i - r_j (oracle.pse_port.min_image) and r = |d|, the force on i from j is c d:
  harmonic (kind 0)  V = k/2 (r - r0)^2,                     c = -k (r - r0)/r
  FENE     (kind 1)  V = -k/2 r0^2 ln(1 - (r/r0)^2), r < r0,  c = -k / (1 - (r/r0)^2)
A bond with r == 0 does nothing; a FENE bond with r >= r0 does nothing and is counted as overstretched.
U = sum V, W_ab = sum c d_a d_b, nbonds = the number of bonds that acted.  The bonds are put into a canonical order (lower endpoint
first, sorted by endpoints and type) before anything is summed, so the result is exactly independent of the order of the list and
of the order of a bond's endpoints.  Not a test module: nothing here is collected."""
import numpy as np

NAMES = ("U", "Wxx", "Wxy", "Wxz", "Wyy", "Wyz", "Wzz", "nbonds")
HARMONIC, FENE = 0, 1
# FENE magnifies rounding by 1 / (1 - (r/r0)^2): every acting FENE bond of the tests has (r/r0)^2 <= X2_MAX, every overstretched
# one r/r0 >= OVER_MIN
X2_MAX, OVER_MIN = 0.9, 1.05


def canonical(pairs, types):
    """(i, j, t) with i < j, sorted by (i, j, t)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    t = np.zeros(len(pairs), dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    i, j = pairs.min(axis=1), pairs.max(axis=1)
    o = np.lexsort((t, j, i))
    return i[o], j[o], t[o]


def bond_terms(pos, box, pairs, types, kinds, k, r0, port):
    """(i, j, d, r, c, V, acts, over) per bond in canonical order; c and V are zero where the bond does not act."""
    pos = np.asarray(pos, dtype=float)
    i, j, t = canonical(pairs, types)
    kind, kk, rr0 = np.asarray(kinds, dtype=np.int64)[t], np.asarray(k, dtype=float)[t], np.asarray(r0, dtype=float)[t]
    d = port.min_image(pos[i] - pos[j], box)
    r = np.sqrt((d * d).sum(axis=1))
    fene = kind == FENE
    over = fene & (r >= rr0) & (r > 0.0)
    acts = (r > 0.0) & ~over
    rs = np.where(acts, r, 1.0)
    x = np.where(acts & fene, (rs / np.where(fene, rr0, 1.0)) ** 2, 0.0)
    c = np.where(fene, -kk / (1.0 - x), -kk * (rs - rr0) / rs)
    V = np.where(fene, -0.5 * kk * rr0 * rr0 * np.log1p(-x), 0.5 * kk * (rs - rr0) ** 2)
    return i, j, d, r, np.where(acts, c, 0.0), np.where(acts, V, 0.0), acts, over


def bond_observables(pos, box, pairs, types, kinds, k, r0, port):
    """(obs[8], F[n, 3], overstretched): U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, nbonds; the forces of the same bond sum; the number of
    FENE bonds at r >= r0."""
    i, j, d, r, c, V, acts, over = bond_terms(pos, box, pairs, types, kinds, k, r0, port)
    obs = np.zeros(8)
    obs[0] = V.sum()
    for q, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        obs[1 + q] = (c * d[:, a] * d[:, b]).sum()
    obs[7] = float(acts.sum())
    F = np.zeros((len(pos), 3))
    np.add.at(F, i, c[:, None] * d)
    np.add.at(F, j, -c[:, None] * d)
    return obs, F, int(over.sum())


def fene_ratios(pos, box, pairs, types, kinds, r0, port):
    """r / r0 of the FENE bonds of a list (for the assertion that a test's bonds are where the bound needs them)."""
    i, j, t = canonical(pairs, types)
    d = port.min_image(np.asarray(pos, dtype=float)[i] - np.asarray(pos, dtype=float)[j], box)
    r = np.sqrt((d * d).sum(axis=1))
    m = np.asarray(kinds)[t] == FENE
    return r[m] / np.asarray(r0, dtype=float)[t][m]


def assert_fene_in_range(pos, box, pairs, types, kinds, r0, port, n_over=0):
    """Every FENE bond has (r/r0)^2 <= X2_MAX, except exactly n_over with r/r0 >= OVER_MIN."""
    q = fene_ratios(pos, box, pairs, types, kinds, r0, port)
    over = q >= OVER_MIN
    assert int(over.sum()) == n_over, (int(over.sum()), n_over)
    assert np.all(q[~over] ** 2 <= X2_MAX), q[~over].max()


# ---- generators: positions with prescribed bond lengths ---------------------------------------------------------------------------
def _wrap(pos, box, port):
    return port.wrap(pos, np.zeros(pos.shape, dtype=np.int64), box)[0]


def _directions(rng, m):
    u = rng.normal(size=(m, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def lengths(rng, m, lo, hi):
    """m bond lengths uniform in [lo, hi]."""
    return rng.uniform(lo, hi, m)


def chains(nchains, beads, box, step, seed, port, first=0):
    """nchains random walks of `beads` beads each from uniform random starts, wrapped into the tilted box; step[c * (beads - 1) + s] is
    the length of bond s of chain c.  Returns (pos, pairs): the particles first .. first + nchains * beads - 1 in chain order."""
    rng = np.random.default_rng(seed)
    step = np.asarray(step, dtype=float).reshape(nchains, beads - 1)
    Lx, Ly, Lz, _ = box
    pos, pairs = [], []
    for c in range(nchains):
        start = (rng.uniform(size=3) - 0.5) * np.array([Lx, Ly, Lz])
        walk = np.vstack([np.zeros(3), np.cumsum(_directions(rng, beads - 1) * step[c][:, None], axis=0)]) + start
        pos.append(walk)
        b = first + c * beads + np.arange(beads - 1)
        pairs.append(np.stack([b, b + 1], axis=1))
    return _wrap(np.vstack(pos), box, port), np.vstack(pairs)


def ring(n, box, side, zig, seed, port):
    """A closed ring of n (even) beads: a regular polygon of side `side` in a random plane whose beads are displaced alternately
    by +-zig/2 along the normal, so that EVERY bond, the closing one included, has length sqrt(side^2 + zig^2)."""
    assert n % 2 == 0 and n >= 4
    rng = np.random.default_rng(seed)
    R = side / (2.0 * np.sin(np.pi / n))
    e1 = _directions(rng, 1)[0]
    e2 = np.cross(e1, _directions(rng, 1)[0]); e2 /= np.linalg.norm(e2)
    e3 = np.cross(e1, e2)
    a = 2.0 * np.pi * np.arange(n) / n
    pos = R * (np.cos(a)[:, None] * e1 + np.sin(a)[:, None] * e2) + 0.5 * zig * ((-1.0) ** np.arange(n))[:, None] * e3
    b = np.arange(n)
    return _wrap(pos + rng.uniform(-1.0, 1.0, 3), box, port), np.stack([b, (b + 1) % n], axis=1)


def star(arms, box, arm_length, seed, port):
    """A hub (particle 0) bonded to `arms` particles at the distances arm_length[a] in random directions."""
    rng = np.random.default_rng(seed)
    hub = rng.uniform(-1.0, 1.0, 3)
    pos = np.vstack([hub, hub + _directions(rng, arms) * np.asarray(arm_length, dtype=float)[:, None]])
    return _wrap(pos, box, port), np.stack([np.zeros(arms, dtype=np.int64), 1 + np.arange(arms)], axis=1)


def random_graph(n, nbonds, box, diameter, seed, port):
    """n points uniform in a ball of the given diameter (so that no two are farther apart than that, and none coincide) and nbonds
    random pairs i != j among them; a pair may be drawn more than once."""
    rng = np.random.default_rng(seed)
    pos = _directions(rng, n) * (0.5 * diameter * rng.uniform(size=n) ** (1.0 / 3.0))[:, None] + rng.uniform(-1.0, 1.0, 3)
    i = rng.integers(0, n, nbonds)
    j = (i + rng.integers(1, n, nbonds)) % n
    return _wrap(pos, box, port), np.stack([i, j], axis=1)


# ---- the inputs of the GPU tests (tests/test_gpu_bonds.py); tests/test_bond_reference.py asserts the FENE ranges on the same ----
BOXES = ((14.0, 14.0, 14.0, 0.0), (14.0, 11.0, 17.0, 0.3))
N_MAX = 513
N_TOPOLOGY = 300
ROW_COUNTS = (2, 63, 64, 65, 255, 256, 257, 513)
TOPOLOGIES = ("chains", "ring", "star", "duplicates", "two_types", "faces")
K_H, R0_H = 30.0, 1.2      # harmonic: lengths in [0.6, 1.9], either side of r0
K_F, R0_F = 30.0, 1.5      # FENE: lengths in [0.3, 0.94] r0, (r/r0)^2 <= 0.8836
PARAMS = {HARMONIC: (K_H, R0_H), FENE: (K_F, R0_F)}


def length_range(kind):
    return (0.6, 1.9) if kind == HARMONIC else (0.3 * R0_F, 0.94 * R0_F)


def _case(pos, pairs, types, kinds, n_over=0):
    kinds = list(kinds)
    out = dict(pos=pos, pairs=np.asarray(pairs, dtype=np.int64), types=None if types is None else np.asarray(types, dtype=np.int64),
               kinds=kinds, k=[PARAMS[q][0] for q in kinds], r0=[PARAMS[q][1] for q in kinds], n_over=n_over)
    for a in (out["pos"], out["pairs"]) + (() if types is None else (out["types"],)):
        a.setflags(write=False)
    return out


def _pad(pos, n, box, seed):
    """pos followed by uniform random (unbonded) points, n rows in all."""
    Lx, Ly, Lz, xy = box
    f = np.random.default_rng(seed).uniform(0.0, 1.0, (n - len(pos), 3)) - 0.5
    extra = np.stack([f[:, 0] * Lx + xy * f[:, 1] * Ly, f[:, 1] * Ly, f[:, 2] * Lz], axis=1)
    return np.vstack([pos, extra])


def chain_case(n, box, kind, port, n_over=0):
    """One chain of n beads; n_over > 0 (FENE): that many bonds, spread over the chain, at r/r0 in [1.05, 1.2]."""
    rng = np.random.default_rng(100 + n)
    step = lengths(rng, n - 1, *length_range(kind))
    if n_over:
        where = np.linspace(0, n - 2, n_over + 2).astype(int)[1:-1]
        step[where] = R0_F * rng.uniform(OVER_MIN, 1.2, n_over)
    pos, pairs = chains(1, n, box, step, 200 + n, port)
    return _case(pos, pairs, None, [kind], n_over)


def topology_case(name, box, kind, port):
    """The topologies of the GPU tests at N_TOPOLOGY particles; `kind` is the potential of the single-type ones."""
    n = N_TOPOLOGY
    rng = np.random.default_rng(7)
    lo, hi = length_range(kind)
    if name == "chains":            # eight chains of 30 and 60 unbonded particles
        pos, pairs = chains(8, 30, box, lengths(rng, 8 * 29, lo, hi), 11, port)
        return _case(_pad(pos, n, box, 12), pairs, None, [kind])
    if name == "ring":
        side = 0.5 * (lo + hi)
        pos, pairs = ring(200, box, side, 0.3 * side, 13, port)
        return _case(_pad(pos, n, box, 14), pairs, None, [kind])
    if name == "star":              # a hub with 40 bonds: one long row
        pos, pairs = star(40, box, lengths(rng, 40, lo, hi), 15, port)
        return _case(_pad(pos, n, box, 16), pairs, None, [kind])
    if name == "duplicates":        # every third bond of a chain twice, one of them three times, copies with swapped endpoints
        pos, pairs = chains(1, 100, box, lengths(rng, 99, lo, hi), 17, port)
        pairs = np.vstack([pairs, pairs[::3, ::-1], pairs[3:4]])
        return _case(_pad(pos, n, box, 18), pairs, None, [kind])
    if name == "two_types":         # harmonic and FENE bonds alternating along four chains (`kind` is the type of the even bonds)
        types = np.tile(np.arange(4 * 49) % 2, 1)
        kinds = [kind, FENE if kind == HARMONIC else HARMONIC]
        step = np.array([rng.uniform(*length_range(kinds[t])) for t in types])
        pos, pairs = chains(4, 50, box, step, 19, port)
        return _case(_pad(pos, n, box, 20), pairs, types, kinds)
    if name == "faces":             # bonds through the x, y and z faces and through the xy edge: a y crossing shifts x by xy Ly
        Lx, Ly, Lz, xy = box
        r = 0.5 * (lo + hi)
        a = np.array([[0.5 * Lx - 0.2, 0.3, -1.0], [1.0 + xy * (0.5 * Ly - 0.2), 0.5 * Ly - 0.2, 2.0], [-2.0, -1.0, 0.5 * Lz - 0.2],
                      [0.5 * Lx - 0.1 + xy * (0.5 * Ly - 0.1), 0.5 * Ly - 0.1, 0.0]])
        u = np.array([[0.8, 0.36, 0.48], [0.36, 0.8, -0.48], [0.48, -0.36, 0.8], [0.6, 0.64, 0.48]])
        u /= np.linalg.norm(u, axis=1)[:, None]
        pos = _wrap(np.vstack([a, a + r * u]), box, port)       # partner q + 4 lies beyond the face and is stored wrapped
        assert np.abs(pos[4:] - pos[:4]).max(axis=1).min() > 5.0   # no stored separation is the bond: each needs an image
        return _case(_pad(pos, n, box, 22), np.stack([np.arange(4), 4 + np.arange(4)], axis=1), None, [kind])
    raise KeyError(name)


def overstretch_case(box, port):
    """A FENE chain of 120 beads with exactly three bonds at r/r0 >= 1.05."""
    return chain_case(120, box, FENE, port, n_over=3)


def graph_case(box, kind, port):
    """400 random bonds (repeats included) among 120 points of a ball whose diameter is the longest length allowed for `kind`, and
    180 unbonded particles: rows of every length, in no order."""
    pos, pairs = random_graph(120, 400, box, length_range(kind)[1], 23, port)
    return _case(_pad(pos, N_TOPOLOGY, box, 24), pairs, None, [kind])


def all_cases(port):
    """(label, box, case) of every fixed input of the GPU tests."""
    for box in BOXES:
        for kind in (HARMONIC, FENE):
            for n in ROW_COUNTS:
                yield f"chain{n}", box, chain_case(n, box, kind, port)
            for name in TOPOLOGIES:
                yield name, box, topology_case(name, box, kind, port)
            yield "graph", box, graph_case(box, kind, port)
        yield "overstretch", box, overstretch_case(box, port)
