"""Chain conformations under shear: the 200 FENE chains of 20 beads of polymer_solution.py under the same oscillatory Lees-Edwards
shear, measured by one analyze.Conformations(period=10) -- every ten steps one pass on the device (pse_molecules_compute) unfolds
every chain along its own bonds, whatever image its beads are in and however often the box has flipped, and reduces the gyration
tensor and the end-to-end vector; nothing is copied to the host until a block is printed.  Per block of 100 steps: <Rg^2>,
<R^2>/<Rg^2> (6 for an ideal chain), the coil stretching G_xx/G_yy and the orientation angle chi of the mean gyration tensor against
the flow direction, all from series().  Once, at the end: the mean Rg by the host formula of semiflexible_polymers.py beside the
same number from per_molecule(); they agree.  `--chains C --beads B` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from polymer_solution import build_chains
from semiflexible_polymers import radius_of_gyration


def main(argv):
    import torch
    from pse_amd import analyze, integrate, shear_function, variant, forces
    from pse_amd.system import System
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, phi = opt("--chains", 200), opt("--beads", 20), 0.1
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    k_fene, r0 = 30.0 / 4.0, 3.0
    pos, pairs = build_chains(nchains, beads, box, 2.0, seed=5)
    s = System(pos, box, dt=1e-3)
    ff = shear_function.sine(dt=1e-3, shear_rate=1.0, shear_freq=1.0)
    s.box_tilt_variant = variant.shear_variant(ff, 2000, max_strain=0.5)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3, function_form=ff)
    kc = 200.0   # core: k/2 (2 - r)^2 for r < 2
    forces.TablePair.from_functions(pse, lambda r: 0.5 * kc * (2.0 - r) ** 2, lambda r: kc * (2.0 - r), 0.0, 2.0, 256)
    bonds = forces.Bonds(pse, pairs, kind="fene", k=k_fene, r0=r0)
    conf = analyze.Conformations(pse, bonds, period=10, capacity=10, nbins=40, rg_max=10.0, ree_max=30.0)   # one block of samples
    print(conf.nmol, 'molecules of', sorted(set(conf.sizes().tolist())), 'beads,', int(conf.nlinear[0]), 'linear')
    torch.cuda.synchronize()
    t0 = time.time()
    for blk in range(5):
        s.run(100)
        tab = conf.series()                                 # (10, 1 + 14): timestep, then the sums over the chains of one sample
        G = analyze.tensor_of(tab[:, 1:7].mean(axis=0) / conf.nmol)
        rg2, ree2 = np.trace(G), tab[:, 8:11].sum(axis=1).mean() / conf.nlinear[0]
        lam, b, c, kappa2 = analyze.shape_of(G)
        print(blk, 'steps', int(tab[0, 0]), '-', int(tab[-1, 0]), 'xy %.4f' % s.box[3], ' <Rg^2> %.4f  <R^2>/<Rg^2> %.3f  Gxx/Gyy %.4f  chi %.4f rad'
              '  kappa^2 of <G> %.4f' % (rg2, ree2 / rg2, G[0, 0] / G[1, 1], analyze.orientation_angle(G), kappa2))
        assert np.isfinite(tab).all() and bonds.overstretched == 0
    torch.cuda.synchronize()
    dt = time.time() - t0
    rows = conf.per_molecule()
    rg_host = radius_of_gyration(s.pos[:, :3].cpu().numpy(), s.box, nchains, beads)
    rg_dev = float(np.sqrt(rows[:, 9]).mean())
    counts, edges = conf.histogram("rg")
    print('<Rg> host formula %.12f  per_molecule() %.12f  (difference %.1e);  most frequent Rg in [%.2f, %.2f)'
          % (rg_host, rg_dev, abs(rg_host - rg_dev), edges[counts[:-1].argmax()], edges[counts[:-1].argmax() + 1]))
    assert abs(rg_host - rg_dev) <= 1e-11 * rg_host
    print('500 steps in %.2f s, %.3f ms per step' % (dt, 2.0 * dt))


if __name__ == "__main__":
    main(sys.argv[1:])
