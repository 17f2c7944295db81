"""Chain statistics with and without bending stiffness: the 200 chains of 20 beads of semiflexible_polymers.py, once with its
cosine-squared bending term and once freely jointed, at rest (no shear), measured by one analyze.ChainStatistics(period=10) and one
analyze.Conformations(period=10) -- every ten steps one pass each on the device; nothing is copied to the host until the run is over.
Prints for both runs the internal-distance curve <R^2(s)>/s at a few separations s (flat for an ideal chain, rising towards s b l_p
for a stiff one), the bond length, the persistence length l_p read from the bond-vector correlation, Kirkwood's hydrodynamic radius
Rh = 1 / <1/Rh> and Rg/Rh (Rg from the Conformations).  `--chains C --beads B --steps S` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from semiflexible_polymers import build_topology, K_BEND, THETA0


def run(nchains, beads, steps, with_angles):
    import torch
    from pse_amd import analyze, integrate, forces
    from pse_amd.system import System
    phi = 0.1
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    k_fene, r0 = 30.0 / 4.0, 3.0
    pos, pairs, triples = build_topology(nchains, beads, box, 2.0, seed=5)
    s = System(pos, box, dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3)
    kc = 200.0   # core: k/2 (2 - r)^2 for r < 2
    forces.TablePair.from_functions(pse, lambda r: 0.5 * kc * (2.0 - r) ** 2, lambda r: kc * (2.0 - r), 0.0, 2.0, 256)
    bonds = forces.Bonds(pse, pairs, kind="fene", k=k_fene, r0=r0)
    if with_angles:
        forces.Angles(pse, triples, kind="cosinesq", k=K_BEND, theta0=THETA0)
    stats = analyze.ChainStatistics(pse, bonds, period=10)
    conf = analyze.Conformations(pse, bonds, period=10)
    torch.cuda.synchronize()
    t0 = time.time()
    s.run(steps)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert bool(torch.isfinite(s.pos).all()) and bonds.overstretched == 0
    sep, r2 = stats.internal_distances()
    _, c = stats.bond_correlation()
    b, lp, rh, rg = stats.bond_length(), stats.persistence_length(smax=3), stats.rh(), math.sqrt(conf.rg2())
    print('with the bending term' if with_angles else 'freely jointed', '--', stats.nmol, 'chains of', beads, 'beads,', stats.samples, 'samples')
    print('   <R^2(s)>/s at s =', ', '.join('%d: %.3f' % (q, r2[q] / q) for q in (1, 2, 4, 8, beads - 1) if q < beads))
    print('   c(s) at s = 1, 2, 3: %.4f %.4f %.4f   bond length %.4f   l_p %.3f   (l_p / b %.2f)' % (c[1], c[2], c[3], b, lp, lp / b))
    print('   Rh %.4f   Rg %.4f   Rg/Rh %.4f   per-molecule 1/Rh now: %.4f .. %.4f' % ((rh, rg, rg / rh) + tuple(np.sort(stats.per_molecule())[[0, -1]])))
    print('   %d steps in %.2f s, %.3f ms per step' % (steps, dt, 1e3 * dt / steps))
    assert np.isfinite(r2[:beads]).all() and np.isfinite([lp, rh, rg]).all()
    return lp, rg / rh


def main(argv):
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, steps = opt("--chains", 200), opt("--beads", 20), opt("--steps", 2000)
    stiff = run(nchains, beads, steps, True)
    free = run(nchains, beads, steps, False)
    print('l_p with / without the bending term: %.3f / %.3f' % (stiff[0], free[0]))


if __name__ == "__main__":
    main(sys.argv[1:])
