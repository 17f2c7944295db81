"""Gelation of the attractive suspension at rest: the spheres of attractive_suspension.py -- a Morse well of 3 kT outside a harmonic
core, both tabulated by forces.TablePair.from_functions -- without shear, and ONE analyzer that says which of them hang together:
analyze.Clusters labels the connected components of the links r < R_WELL, the end of the well, every PERIOD steps on the device
(pse_clusters_label: a union-find over the cell list the step uses anyway; nothing is read back until a number is printed).

Prints, every 100 steps, the number of clusters, the fraction of the system in the largest one and the weight-average cluster size of
that block's samples: the clusters merge and the weight-average size grows.  The default volume fraction is 0.05, not the 0.2 of
attractive_suspension.py: a random start at 0.2 has 6.5 partners within R_WELL of every sphere, far above the 2.7 at which overlapping
spheres percolate, and is one cluster from the first step on (`--phi 0.2` shows that); at 0.05 there are 1.6.
`--n N --phi PHI --steps S` change the run."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

K_CORE = 200.0                                  # core: k/2 (2 - r)^2 for r < 2 (contact of unit spheres)
D, ALPHA, R0, R_WELL = 3.0, 4.0, 2.1, 3.2       # Morse well of depth D at R0, range 1/ALPHA, from contact to R_WELL, shifted to end at V = 0
PERIOD, BLOCK = 10, 100


def main(argv):
    import torch
    from pse_amd import analyze, integrate, forces
    from pse_amd.system import System
    opt = lambda name, default, kind=int: kind(argv[argv.index(name) + 1]) if name in argv else default
    n, phi, steps = opt("--n", 8000), opt("--phi", 0.05, float), opt("--steps", 500)
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    pos = np.random.default_rng(5).uniform(-L / 2, L / 2, size=(n, 3))
    s = System(pos, (L, L, L, 0.0), dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3)
    forces.TablePair.from_functions(pse, lambda r: 0.5 * K_CORE * (2.0 - r) ** 2, lambda r: K_CORE * (2.0 - r), 0.0, 2.0, 256)
    e = lambda r: math.exp(-ALPHA * (r - R0))
    Vm = lambda r: D * ((1.0 - e(r)) ** 2 - 1.0)
    forces.TablePair.from_functions(pse, lambda r: Vm(r) - Vm(R_WELL), lambda r: -2.0 * D * ALPHA * (1.0 - e(r)) * e(r), 2.0, R_WELL, 1024)
    clusters = analyze.Clusters(pse, R_WELL, period=PERIOD, capacity=BLOCK // PERIOD)   # the ring holds one block of samples
    print("%d spheres at phi = %.2f, L = %.2f; linked below %.2f, a sample every %d steps" % (n, phi, L, R_WELL, PERIOD))
    torch.cuda.synchronize()
    t0 = time.time()
    for blk in range(steps // BLOCK):
        s.run(BLOCK)
        assert bool(torch.isfinite(s.pos).all())
        last = clusters.table()[-1]                     # (the first read waits for the device)
        print("  step %d  clusters %d  largest fraction %.4f  weight-average size %.1f  (number-average %.2f over %d samples)"
              % ((blk + 1) * BLOCK, last[1], clusters.largest_fraction(), clusters.weight_average(), clusters.number_average(),
                 len(clusters.table())))
    torch.cuda.synchronize()
    print("%d steps in %.2f s; give-up word of the labelling: %d" % (steps // BLOCK * BLOCK, time.time() - t0, clusters.status()))
    ns = clusters.size_distribution()
    print("n(s) per sample, s = 1 .. 8:", " ".join("%.1f" % v for v in ns[:8]), " clusters of 100 or more: %.2f" % ns[99:].sum())


if __name__ == "__main__":
    main(sys.argv[1:])
