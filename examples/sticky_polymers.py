"""Sticky bead-spring polymers, with and without pair exclusions: 100 chains of 20 beads at phi = 0.05 -- harmonic bonds of rest length
R0_BOND (forces.Bonds), a cosine-squared bending term (forces.Angles) and a Morse pair potential with its well at R_WELL, just
outside contact, between all beads (forces.TablePair) -- with hydrodynamic interactions and Brownian motion, no shear; 300 steps,
run twice from the same start.

The rest length of the bonds lies INSIDE the Morse core (R0_BOND < R_WELL), as in any force field whose bonded parameters were fitted
with the bonded pairs excluded from the pair potential -- HOOMD's default, nlist.reset_exclusions(['bond']).  In the first run the
table acts on every pair: bonded neighbours feel bond and core at once, the bonds are pushed out towards R_WELL and the bending term
works against the 1-3 attraction.  In the second run forces.Exclusions.from_topology(bonds=..., angles=...) takes the 1-2 and 1-3 pairs out
of the table (pse_pair_table_excl): the mean bond length sits at R0_BOND again, up to thermal motion.  Prints for both runs, per
block of 100 steps, the mean bond length, the mean radius of gyration, the pair energy and the number of pairs the table acted on.
`--chains C --beads B` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from semiflexible_polymers import _min_image, radius_of_gyration   # noqa: E402

K_BOND, R0_BOND = 100.0, 1.6            # harmonic bonds, in kT / a^2 and bead radii a
K_BEND, THETA0 = 5.0, math.pi           # cosine-squared: V = k/2 (cos theta + 1)^2
D_WELL, ALPHA, R_WELL = 2.0, 2.0, 2.2   # Morse D ((1 - e^{-alpha (r - R_WELL)})^2 - 1): a well of 2 kT just outside contact (r = 2)
R_MIN, R_MAX, WIDTH = 0.5, 4.5, 1024    # the table's range and nodes
BEND_RANGE = (0.3, 1.2)                 # the turn from bond to bond of the starting walks: no bead starts on its second neighbour


def build_topology(nchains, beads, box, bond_length, seed):
    """nchains random walks of `beads` beads with steps of length bond_length from uniform random starts, wrapped into the (Lx, Ly,
    Lz, xy) box: each step turns by an angle uniform in BEND_RANGE about a random azimuth from the one before.  Returns (pos[nchains
    * beads, 3], pairs[nchains * (beads - 1), 2], triples[nchains * (beads - 2), 3], quads[nchains * (beads - 3), 4]); chain c is the
    beads c * beads ... c * beads + beads - 1, bonded in that order, one angle at every inner bead, one dihedral per four in a row."""
    rng = np.random.default_rng(seed)
    Lx, Ly, Lz, xy = box
    unit = lambda v: v / np.linalg.norm(v, axis=-1)[..., None]
    u = unit(rng.normal(size=(nchains, 3)))
    steps = [u]
    for s in range(beads - 2):
        bend = rng.uniform(*BEND_RANGE, size=(nchains, 1))
        v = unit(np.cross(u, rng.normal(size=(nchains, 3))))
        u = unit(np.cos(bend) * u + np.sin(bend) * v)
        steps.append(u)
    start = (rng.uniform(size=(nchains, 1, 3)) - 0.5) * np.array([Lx, Ly, Lz])
    walk = np.cumsum(bond_length * np.stack(steps, axis=1), axis=1)
    pos = np.concatenate([start, start + walk], axis=1).reshape(-1, 3)
    n = np.floor(pos[:, 2] / Lz + 0.5); pos[:, 2] -= n * Lz
    n = np.floor(pos[:, 1] / Ly + 0.5); pos[:, 1] -= n * Ly; pos[:, 0] -= n * xy * Ly
    n = np.floor((pos[:, 0] - xy * pos[:, 1]) / Lx + 0.5); pos[:, 0] -= n * Lx
    idx = lambda m: (np.arange(nchains)[:, None] * beads + np.arange(beads - m)[None, :]).reshape(-1)
    b1, b2, b3 = idx(1), idx(2), idx(3)
    return pos, np.stack([b1, b1 + 1], axis=1), np.stack([b2, b2 + 1, b2 + 2], axis=1), np.stack([b3, b3 + 1, b3 + 2, b3 + 3], axis=1)


def mean_bond_length(pos, box, pairs):
    """Mean over the bonds of |r_i - r_j| by the minimum image."""
    return float(np.linalg.norm(_min_image(pos[pairs[:, 0]] - pos[pairs[:, 1]], box), axis=1).mean())


def morse(r):
    e = math.exp(-ALPHA * (r - R_WELL))
    return D_WELL * ((1.0 - e) ** 2 - 1.0)


def morse_force(r):
    e = math.exp(-ALPHA * (r - R_WELL))
    return -2.0 * D_WELL * ALPHA * (1.0 - e) * e


def run(pos, pairs, triples, box, nchains, beads, exclude):
    import torch
    from pse_amd import integrate, forces
    from pse_amd.system import System
    s = System(pos, box, dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3)
    excl = forces.Exclusions.from_topology(pse, bonds=pairs, angles=triples) if exclude else None
    pair = forces.TablePair.from_functions(pse, morse, morse_force, R_MIN, R_MAX, WIDTH, virial=True, exclusions=excl)
    forces.Bonds(pse, pairs, kind="harmonic", k=K_BOND, r0=R0_BOND)
    forces.Angles(pse, triples, kind="cosinesq", k=K_BEND, theta0=THETA0)
    print("with exclusions (1-2 and 1-3 pairs: %d)" % excl.npairs_listed if exclude else "without exclusions")
    torch.cuda.synchronize()
    t0 = time.time()
    lengths = []
    for blk in range(3):
        s.run(100)
        ok = bool(torch.isfinite(s.pos).all())
        p = s.pos[:, :3].cpu().numpy()
        lengths.append(mean_bond_length(p, s.box, pairs))
        print('  ', blk, 'finite', ok, '<bond> %.4f (r0 %.2f)' % (lengths[-1], R0_BOND), '<Rg> %.4f' % radius_of_gyration(p, s.box, nchains, beads),
              'U_pair %.6g' % pair.energy, 'npairs %d' % pair.npairs)
        assert ok
    torch.cuda.synchronize()
    print('   300 steps in %.2f s' % (time.time() - t0))
    return lengths[-1]


def main(argv):
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, phi = opt("--chains", 100), opt("--beads", 20), 0.05
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    pos, pairs, triples, _ = build_topology(nchains, beads, box, R0_BOND, seed=5)
    plain = run(pos, pairs, triples, box, nchains, beads, exclude=False)
    excl = run(pos, pairs, triples, box, nchains, beads, exclude=True)
    print('mean bond length after 300 steps: %.4f without exclusions, %.4f with (r0 = %.2f)' % (plain, excl, R0_BOND))


if __name__ == "__main__":
    main(sys.argv[1:])
