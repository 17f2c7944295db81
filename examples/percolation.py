"""The gel point of the attractive suspension at rest: the run of gelation.py -- a Morse well of 3 kT outside a harmonic core, no shear --
with analyze.Clusters(percolation=True): beside the labels, every sample says which clusters are connected to their own periodic
image and along which lattice axes, makes every other cluster whole across the boundaries and takes its radius of gyration, all on
the device (pse_clusters_span: the union-find of pse_clusters_label with an integer image offset beside every parent pointer; nothing
is read back until a number is printed).

Prints, every 100 steps, the number of clusters, whether and along which axes one spans in the last sample, the share of that block's
samples with a spanning cluster, the weight-average size of the clusters that span nothing and the fractal dimension d_f -- the
least-squares slope of log s on log Rg over the finite clusters of the last sample with SMIN members or more (n/a, or noise, while
there are only a few of them).  At the default volume fraction of 0.12 a random start has 3.9 partners within R_WELL of every sphere,
above the 2.7 at which overlapping spheres percolate: one cluster spans all three axes from the first sample on, and the run shows the
finite clusters beside it; `--phi 0.05` starts below the threshold, as gelation.py does.
`--n N --phi PHI --steps S` change the run."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

K_CORE = 200.0                                  # core: k/2 (2 - r)^2 for r < 2 (contact of unit spheres)
D, ALPHA, R0, R_WELL = 3.0, 4.0, 2.1, 3.2       # Morse well of depth D at R0, range 1/ALPHA, from contact to R_WELL, shifted to end at V = 0
PERIOD, BLOCK, SMIN = 10, 100, 5


def main(argv):
    import torch
    from pse_amd import analyze, integrate, forces
    from pse_amd.system import System
    opt = lambda name, default, kind=int: kind(argv[argv.index(name) + 1]) if name in argv else default
    n, phi, steps = opt("--n", 8000), opt("--phi", 0.12, float), opt("--steps", 500)
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    pos = np.random.default_rng(5).uniform(-L / 2, L / 2, size=(n, 3))
    s = System(pos, (L, L, L, 0.0), dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3)
    forces.TablePair.from_functions(pse, lambda r: 0.5 * K_CORE * (2.0 - r) ** 2, lambda r: K_CORE * (2.0 - r), 0.0, 2.0, 256)
    e = lambda r: math.exp(-ALPHA * (r - R0))
    Vm = lambda r: D * ((1.0 - e(r)) ** 2 - 1.0)
    forces.TablePair.from_functions(pse, lambda r: Vm(r) - Vm(R_WELL), lambda r: -2.0 * D * ALPHA * (1.0 - e(r)) * e(r), 2.0, R_WELL, 1024)
    clusters = analyze.Clusters(pse, R_WELL, period=PERIOD, capacity=BLOCK // PERIOD, percolation=True)   # the rings hold one block of samples
    print("%d spheres at phi = %.2f, L = %.2f; linked below %.2f, a sample every %d steps" % (n, phi, L, R_WELL, PERIOD))
    torch.cuda.synchronize()
    t0 = time.time()
    for blk in range(steps // BLOCK):
        s.run(BLOCK)
        assert bool(torch.isfinite(s.pos).all())
        last, perc = clusters.table()[-1], clusters.percolation_table()[-1]          # (the first read waits for the device)
        axes = "".join(a for a, k in zip("xyz", (3, 4, 5)) if perc[k]) or "-"
        table = clusters.cluster_table()
        try:
            df = "%.2f" % analyze.fractal_dimension_of(table["size"], table["rg2"], smin=SMIN)
        except ValueError:
            df = "n/a"                                                                # fewer than two finite clusters of SMIN members
        print("  step %d  clusters %d  spanning %d along %s (%d members)  P(span) %.2f  finite weight-average size %.1f  d_f %s"
              % ((blk + 1) * BLOCK, last[1], perc[1], axes, perc[2], clusters.percolation_probability(), clusters.finite_weight_average(), df))
    torch.cuda.synchronize()
    print("%d steps in %.2f s; give-up word of the labelling: %d" % (steps // BLOCK * BLOCK, time.time() - t0, clusters.status()))
    U, lab = clusters.unfolded(), clusters.labels()
    table = clusters.cluster_table()
    finite = table[table["span"] == 0]
    if len(finite):
        big = finite[np.argmax(finite["size"])]
        m = U[lab == big["label"]]
        print("largest finite cluster: %d members, Rg %.2f on the device, %.2f from its unfolded positions on the host"
              % (big["size"], math.sqrt(big["rg2"]), math.sqrt(((m - m.mean(axis=0)) ** 2).sum() / len(m))))


if __name__ == "__main__":
    main(sys.argv[1:])
