"""The structure of the diblock-copolymer melt of block_copolymers.py, measured with ONE analyzer: analyze.RDF samples the
pair-distance histogram of the integrator's cell list (pse_pair_hist_accumulate) every PERIOD steps -- one cell walk per sample, no
force provider, nothing read back until a number is printed -- and from the same counters come the partial radial distribution
functions g_AA, g_AB, g_BB and the coordination numbers.  The system, its potentials and its bonds are those of block_copolymers.py
(imported); the bonded pairs are excluded from the counts as they are from the pair potentials.

Prints, every 250 steps, g at contact (the bin that ends at R_CONTACT) for the three pairs of types and the A-A and B-B
coordination at R_CONTACT -- the contacts per bead that block_copolymers.py counts with two zero-table providers on every step --
over the samples of that block.  The A blocks find each other: g_AA at contact and the A-A coordination grow; the B blocks stay
where the excluded volume leaves them.  `--chains C --beads B --steps S` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sticky_polymers import build_topology   # noqa: E402
from block_copolymers import (morse, morse_force, core, K_BOND, R0_BOND, R_MIN, R_MAX, R_WELL, WIDTH, R_CONTACT, DT, BLOCK)   # noqa: E402

NBINS, R_HIST = 50, 5.0    # bins of 0.1 up to 5 (the engine's cutoff is 5.26): R_CONTACT = 2.6 is the upper edge of bin 25
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
    rdf = analyze.RDF(pse, NBINS, R_HIST, types=types, type_names=names, exclusions=excl, period=PERIOD)
    contact = int(round(R_CONTACT / (R_HIST / NBINS))) - 1          # the bin whose upper edge is R_CONTACT
    print("%d chains of %d beads, L = %.2f, %d excluded pairs; %d bins of %.2f, a sample every %d steps"
          % (nchains, beads, L, excl.npairs_listed, NBINS, R_HIST / NBINS, PERIOD))
    torch.cuda.synchronize()
    t0 = time.time()
    first = last = None
    for blk in range(steps // BLOCK):
        rdf.reset()
        s.run(BLOCK)
        assert bool(torch.isfinite(s.pos).all())
        g = {key: rdf.g(*key)[contact] for key in (("A", "A"), ("A", "B"), ("B", "B"))}          # (the first read waits for the device)
        last = {a: rdf.coordination(a, a, R_CONTACT) for a in names}
        first = first or last
        print('  step', (blk + 1) * BLOCK, 'samples', rdf.samples, 'g at contact: AA %.3f AB %.3f BB %.3f' % (g["A", "A"], g["A", "B"], g["B", "B"]),
              'A-A contacts per A bead %.3f' % last["A"], 'B-B contacts per B bead %.3f' % last["B"])
    torch.cuda.synchronize()
    print('%d steps in %.2f s' % (steps // BLOCK * BLOCK, time.time() - t0))
    print('contacts per bead, first block -> last: A-A %.3f -> %.3f, B-B %.3f -> %.3f' % (first["A"], last["A"], first["B"], last["B"]))
    r, gaa = rdf.r, rdf.g("A", "A")
    print('g_AA(r) of the last block:', ' '.join('%.1f:%.2f' % (x, y) for x, y in zip(r[15::5], gaa[15::5])))


if __name__ == "__main__":
    main(sys.argv[1:])
