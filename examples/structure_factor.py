"""The structure of the diblock-copolymer melt of block_copolymers.py in reciprocal space: analyze.StructureFactor sums the densities
rho_A(k), rho_B(k) of the two blocks on the reciprocal lattice of the box (pse_structure_factor_accumulate) every PERIOD steps -- a
direct, exact sum over all modes with |k| <= K_MAX, nothing read back until a number is printed -- the other half of what
pair_correlations.py measures with g(r): g(r) ends at the real-space cutoff (5.26), S(k) begins at 2 pi / L, where the microphase
peak of a block copolymer lives.  The system, its potentials and its bonds are those of pair_correlations.py.

Prints, every 250 steps, the shell-averaged S_AA, S_AB and S_BB over the samples of that block, and the k of the largest S_AA: as the
A blocks find each other, S_AA grows a peak at the k of the domain spacing and S_AB turns negative there.
`--chains C --beads B --steps S` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sticky_polymers import build_topology   # noqa: E402
from block_copolymers import (morse, morse_force, core, K_BOND, R0_BOND, R_MIN, R_MAX, R_WELL, WIDTH, DT, BLOCK)   # noqa: E402

K_MAX, NSHELLS = 2.0, 16   # every mode of the half space up to |k| = 2 (a bead's diameter is 2: the contact peak lies beyond, near 3.5)
PERIOD = 10                # steps between samples


def main(argv):
    import torch
    from pse_amd import analyze, integrate, forces
    from pse_amd.system import System
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, steps, phi = opt("--chains", 100), opt("--beads", 20), opt("--steps", 2000), 0.08
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    pos, pairs, _, _ = build_topology(nchains, beads, box, R0_BOND, seed=5)
    names = ["A", "B"]
    types = np.tile(np.where(np.arange(beads) < beads // 2, "A", "B"), nchains)
    s = System(pos, box, dt=DT)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3)
    excl = forces.Exclusions.from_topology(pse, bonds=pairs)
    forces.TypedTablePair.from_functions(pse, types, {("A", "A"): (morse, morse_force, R_MIN, R_MAX, WIDTH),
                                                      ("A", "B"): (core, morse_force, R_MIN, R_WELL, WIDTH),
                                                      ("B", "B"): (core, morse_force, R_MIN, R_WELL, WIDTH)},
                                         exclusions=excl, type_names=names)
    forces.Bonds(pse, pairs, kind="harmonic", k=K_BOND, r0=R0_BOND)
    modes = analyze.modes_within(box, K_MAX)
    sf = analyze.StructureFactor(pse, modes, types=types, type_names=names, period=PERIOD)
    print("%d chains of %d beads, L = %.2f; %d modes with |k| <= %.1f (2 pi / L = %.3f), %d shells, a sample every %d steps"
          % (nchains, beads, L, sf.nk, K_MAX, 2 * math.pi / L, NSHELLS, PERIOD))
    torch.cuda.synchronize()
    t0 = time.time()
    for blk in range(steps // BLOCK):
        sf.reset()
        s.run(BLOCK)
        assert bool(torch.isfinite(s.pos).all())
        k, saa, cnt = sf.shell_average(NSHELLS, K_MAX, "A", "A")                                   # (the first read waits for the device)
        sab, sbb = sf.shell_average(NSHELLS, K_MAX, "A", "B")[1], sf.shell_average(NSHELLS, K_MAX, "B", "B")[1]
        top = int(np.nanargmax(saa))
        print('  step', (blk + 1) * BLOCK, 'samples', sf.samples, 'largest S_AA %.3f at k = %.3f (S_AB %.3f, S_BB %.3f there)'
              % (saa[top], k[top], sab[top], sbb[top]))
    torch.cuda.synchronize()
    print('%d steps in %.2f s' % (steps // BLOCK * BLOCK, time.time() - t0))
    print('   k     modes  S_AA    S_AB    S_BB   of the last block')
    for row in zip(k, cnt, saa, sab, sbb):
        if row[1]:
            print('  %.3f  %5d  %6.3f  %6.3f  %6.3f' % row)


if __name__ == "__main__":
    main(sys.argv[1:])
