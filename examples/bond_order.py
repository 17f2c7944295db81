"""Melting of an fcc crystal at rest: unit-radius beads with a soft repulsion (forces.HarmonicRepulsion) start on the sites of an fcc
lattice of cubic cell A = 3.4 -- nearest neighbours at A/sqrt(2) = 2.40, volume fraction 0.43, below the freezing density of hard
spheres -- and ONE analyzer says how ordered every neighbourhood still is: analyze.BondOrder computes the Steinhardt q_4 and q_6, the
neighbour-averaged q-bar_6 and the solid-like bonds of every bead every PERIOD steps on the device (pse_bond_order_compute: two passes
over the cell list the step uses anyway; nothing is read back until a number is printed).

Neighbours are the beads closer than RNB = 2.9: between the first fcc shell (2.40, twelve beads) and the second (A = 3.40, six more),
so that the perfect crystal has exactly its twelve nearest neighbours and thermal motion of a few tenths moves nobody across the edge.
A bond is solid-like when the q_6 vectors of its two ends have a normalised product above 0.7, a bead when it has at least 7 of them.

Prints, every 100 steps, the mean q_6, the mean q-bar_6, the mean number of neighbours and the solid-like fraction of the last sample.
At step 0 they sit at the fcc values (q_6 = 0.5745 = q-bar_6, 12 neighbours, all solid-like; q_4 = 0.1909) and decay as Brownian motion
disorders the shells.  `--cells K --steps S` change the run (4 K^3 beads)."""
import numpy as np, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

A = 3.4                       # cubic cell of the fcc lattice
RNB = 2.9                     # between A / sqrt(2) = 2.40 and A = 3.40
SOLID = (6, 0.7, 7)           # degree, threshold on s_ij, connections of a solid-like bead
PERIOD, BLOCK = 10, 100


def fcc(cells, a):
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    g = np.arange(cells)
    idx = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    return ((idx + basis[None]).reshape(-1, 3) + 0.25) * a - 0.5 * cells * a


def main(argv):
    import torch
    from pse_amd import analyze, integrate, forces
    from pse_amd.system import System
    opt = lambda name, default, kind=int: kind(argv[argv.index(name) + 1]) if name in argv else default
    cells, steps = opt("--cells", 8), opt("--steps", 500)
    L = cells * A
    s = System(fcc(cells, A), (L, L, L, 0.0), dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3)
    forces.HarmonicRepulsion(pse, k=200.0, sigma=2.0)
    order = analyze.BondOrder(pse, RNB, degrees=(4, 6), solid=SOLID, period=PERIOD, capacity=BLOCK // PERIOD)
    print("%d beads on an fcc lattice, L = %.2f; neighbours below %.2f, a sample every %d steps" % (s.n, L, RNB, PERIOD))

    def report():
        last = order.table()[-1]                        # timestep, members, solid-like (the first read waits for the device)
        print("  step %4d  <q6> %.4f  <qbar6> %.4f  <q4> %.4f  neighbours %.2f  solid-like fraction %.3f"
              % (last[0], order.q(6).mean(), order.qbar(6).mean(), order.q(4).mean(), order.neighbors().mean(), last[2] / last[1]))

    torch.cuda.synchronize()
    t0 = time.time()
    s.run(1)                                            # the sample of step 0: the perfect crystal
    report()
    for blk in range(steps // BLOCK):
        s.run(BLOCK)                                    # steps 1 + 100 blk .. 100 (blk + 1): the last sample is that of step 100 (blk + 1)
        assert bool(torch.isfinite(s.pos).all())
        report()
    torch.cuda.synchronize()
    print("%d steps in %.2f s; mean q6 over all %d samples (from the histogram) %.3f, solid-like fraction over the last block %.3f"
          % (steps // BLOCK * BLOCK + 1, time.time() - t0, order.samples, order.mean(6), order.solid_fraction()))


if __name__ == "__main__":
    main(sys.argv[1:])
