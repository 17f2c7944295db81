"""A polymer solution under shear: 200 bead-spring chains of 20 beads (FENE bonds, forces.Bonds / pse_bond_forces) at phi = 0.1 with
a harmonic core repulsion between all beads (forces.TablePair), hydrodynamic interactions and Brownian motion, under oscillatory
Lees-Edwards shear; 500 steps.  Prints per block of 100 steps the mean radius of gyration of the chains, the bond energy and the
polymer (bond) contribution to sigma_xy -- sampled every 10 steps by the bond pass itself into a device log (forces.StressLog) that is
read once per block -- and the number of FENE bonds found beyond their maximum extension, which must stay 0.
`--no-bonds` runs the same system without the bond provider (for the cost of the bond call), `--chains C --beads B` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_chains(nchains, beads, box, bond_length, seed):
    """nchains freely jointed chains of `beads` beads with bonds of length bond_length from uniform random starts, wrapped into the
    (Lx, Ly, Lz, xy) box: (pos[nchains * beads, 3], pairs[nchains * (beads - 1), 2]); chain c is the beads c * beads ...
    c * beads + beads - 1, bonded in that order."""
    rng = np.random.default_rng(seed)
    Lx, Ly, Lz, xy = box
    u = rng.normal(size=(nchains, beads - 1, 3))
    u *= bond_length / np.linalg.norm(u, axis=2)[:, :, None]
    start = (rng.uniform(size=(nchains, 1, 3)) - 0.5) * np.array([Lx, Ly, Lz])
    pos = np.concatenate([start, start + np.cumsum(u, axis=1)], axis=1).reshape(-1, 3)
    n = np.floor(pos[:, 2] / Lz + 0.5); pos[:, 2] -= n * Lz
    n = np.floor(pos[:, 1] / Ly + 0.5); pos[:, 1] -= n * Ly; pos[:, 0] -= n * xy * Ly
    n = np.floor((pos[:, 0] - xy * pos[:, 1]) / Lx + 0.5); pos[:, 0] -= n * Lx
    first = (np.arange(nchains)[:, None] * beads + np.arange(beads - 1)[None, :]).reshape(-1)
    return pos, np.stack([first, first + 1], axis=1)


def radius_of_gyration(pos, box, nchains, beads):
    """Mean over the chains of Rg, each chain unfolded along its bonds by the minimum image (bonds are far shorter than half the box)."""
    Lx, Ly, Lz, xy = box
    p = pos.reshape(nchains, beads, 3)
    d = p[:, 1:] - p[:, :-1]
    n = np.rint(d[..., 2] / Lz); d[..., 2] -= n * Lz
    n = np.rint(d[..., 1] / Ly); d[..., 1] -= n * Ly; d[..., 0] -= n * xy * Ly
    n = np.rint(d[..., 0] / Lx); d[..., 0] -= n * Lx
    chain = np.concatenate([np.zeros((nchains, 1, 3)), np.cumsum(d, axis=1)], axis=1)
    chain -= chain.mean(axis=1, keepdims=True)
    return float(np.sqrt((chain ** 2).sum(axis=2).mean(axis=1)).mean())


def main(argv):
    import torch
    from pse_amd import integrate, shear_function, variant, forces
    from pse_amd.system import System
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, phi = opt("--chains", 200), opt("--beads", 20), 0.1
    with_bonds = "--no-bonds" not in argv
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    # Kremer-Grest chains in units of the bead radius a = 1 (sigma = 2): r0 = 1.5 sigma, k = 30 kT / sigma^2; bonds start at contact
    k_fene, r0 = 30.0 / 4.0, 3.0
    pos, pairs = build_chains(nchains, beads, box, 2.0, seed=5)
    s = System(pos, box, dt=1e-3)
    ff = shear_function.sine(dt=1e-3, shear_rate=1.0, shear_freq=1.0)
    s.box_tilt_variant = variant.shear_variant(ff, 2000, max_strain=0.5)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3, function_form=ff)
    kc = 200.0   # core: k/2 (2 - r)^2 for r < 2
    forces.TablePair.from_functions(pse, lambda r: 0.5 * kc * (2.0 - r) ** 2, lambda r: kc * (2.0 - r), 0.0, 2.0, 256)
    if with_bonds:
        bonds = forces.Bonds(pse, pairs, kind="fene", k=k_fene, r0=r0, virial=True)
        log = forces.StressLog(bonds, period=10, capacity=10)   # one block of samples; the ring then starts over
    torch.cuda.synchronize()
    t0 = time.time()
    for blk in range(5):
        s.run(100)
        ok = bool(torch.isfinite(s.pos).all())
        rg = radius_of_gyration(s.pos[:, :3].cpu().numpy(), s.box, nchains, beads)
        print(blk, 'finite', ok, 'xy', round(s.box[3], 4), 'm', pse.cpp_method.lanczosIterations(), '<Rg> %.4f' % rg)
        assert ok
        if with_bonds:
            tab = log.table()   # columns: forces.StressLog.COLUMNS
            over = bonds.overstretched
            print('   ', len(tab), 'samples, steps', int(tab[0, 0]), '-', int(tab[-1, 0]), ' <U_bond> %.6g  <sigma_xy bond> %.6g  sigma_xy(last) %.6g at xy %.4f'
                  '  bonds(last) %d of %d  overstretched %d' % (tab[:, 2].mean(), tab[:, 4].mean(), tab[-1, 4], tab[-1, 1], int(tab[-1, 9]), len(pairs), over))
            assert over == 0 and np.isfinite(tab).all()
    torch.cuda.synchronize()
    dt = time.time() - t0
    print('500 steps in %.2f s, %.3f ms per step, %s' % (dt, 2.0 * dt, 'with bonds' if with_bonds else 'without bonds'))


if __name__ == "__main__":
    main(sys.argv[1:])
