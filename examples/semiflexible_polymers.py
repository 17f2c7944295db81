"""Semiflexible polymers under shear: 200 bead-spring chains of 20 beads at phi = 0.1 -- FENE bonds (forces.Bonds / pse_bond_forces),
a cosine-squared bending term at every inner bead (forces.Angles / pse_angle_forces: V = k/2 (cos theta + 1)^2, straight at rest) and a
harmonic core repulsion between all beads (forces.TablePair) -- with hydrodynamic interactions and Brownian motion, under
oscillatory Lees-Edwards shear; 500 steps.  Prints per block of 100 steps the mean cosine of the bond angle (-1: rods), the mean
radius of gyration of the chains, and the bending and the bond energy with their contributions to sigma_xy -- sampled every 10 steps by
the two passes themselves into device logs (forces.StressLog) that are read once per block.
`--no-angles` runs the same chains freely jointed (for the effect and the cost of the bending term), `--chains C --beads B` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

K_BEND, THETA0 = 20.0, math.pi     # in kT: a persistence length of the order of ten bonds
BEND_RANGE = (0.14, 0.74)          # the bends (pi - theta) of the starting configuration: gently curved, never exactly straight


def build_topology(nchains, beads, box, bond_length, seed):
    """nchains gently curved chains of `beads` beads with bonds of length bond_length from uniform random starts, wrapped into the
    (Lx, Ly, Lz, xy) box: each bond turns by an angle uniform in BEND_RANGE about a random azimuth from the one before.  Returns
    (pos[nchains * beads, 3], pairs[nchains * (beads - 1), 2], triples[nchains * (beads - 2), 3]); chain c is the beads c * beads ...
    c * beads + beads - 1, bonded in that order, with one angle (b - 1, b, b + 1) at every inner bead b."""
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
    first = (np.arange(nchains)[:, None] * beads + np.arange(beads - 1)[None, :]).reshape(-1)
    mid = (np.arange(nchains)[:, None] * beads + np.arange(1, beads - 1)[None, :]).reshape(-1)
    return pos, np.stack([first, first + 1], axis=1), np.stack([mid - 1, mid, mid + 1], axis=1)


def _min_image(d, box):
    Lx, Ly, Lz, xy = box
    n = np.rint(d[..., 2] / Lz); d[..., 2] -= n * Lz
    n = np.rint(d[..., 1] / Ly); d[..., 1] -= n * Ly; d[..., 0] -= n * xy * Ly
    n = np.rint(d[..., 0] / Lx); d[..., 0] -= n * Lx
    return d


def mean_bond_angle_cosine(pos, box, triples):
    """Mean over the angles of cos(theta) at the vertex, arms by the minimum image: -1 for straight chains, 0 for freely jointed ones."""
    d1 = _min_image(pos[triples[:, 0]] - pos[triples[:, 1]], box)
    d2 = _min_image(pos[triples[:, 2]] - pos[triples[:, 1]], box)
    return float(((d1 * d2).sum(axis=1) / (np.linalg.norm(d1, axis=1) * np.linalg.norm(d2, axis=1))).mean())


def radius_of_gyration(pos, box, nchains, beads):
    """Mean over the chains of Rg, each chain unfolded along its bonds by the minimum image (bonds are far shorter than half the box)."""
    p = pos.reshape(nchains, beads, 3)
    d = _min_image(p[:, 1:] - p[:, :-1], box)
    chain = np.concatenate([np.zeros((nchains, 1, 3)), np.cumsum(d, axis=1)], axis=1)
    chain -= chain.mean(axis=1, keepdims=True)
    return float(np.sqrt((chain ** 2).sum(axis=2).mean(axis=1)).mean())


def main(argv):
    import torch
    from pse_amd import integrate, shear_function, variant, forces
    from pse_amd.system import System
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, phi = opt("--chains", 200), opt("--beads", 20), 0.1
    with_angles = "--no-angles" not in argv
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    # Kremer-Grest bonds in units of the bead radius a = 1 (sigma = 2): r0 = 1.5 sigma, k = 30 kT / sigma^2; bonds start at contact
    k_fene, r0 = 30.0 / 4.0, 3.0
    pos, pairs, triples = build_topology(nchains, beads, box, 2.0, seed=5)
    s = System(pos, box, dt=1e-3)
    ff = shear_function.sine(dt=1e-3, shear_rate=1.0, shear_freq=1.0)
    s.box_tilt_variant = variant.shear_variant(ff, 2000, max_strain=0.5)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3, function_form=ff)
    kc = 200.0   # core: k/2 (2 - r)^2 for r < 2
    forces.TablePair.from_functions(pse, lambda r: 0.5 * kc * (2.0 - r) ** 2, lambda r: kc * (2.0 - r), 0.0, 2.0, 256)
    bonds = forces.Bonds(pse, pairs, kind="fene", k=k_fene, r0=r0, virial=True)
    logs = {"bond": forces.StressLog(bonds, period=10, capacity=10)}   # one block of samples; the ring then starts over
    if with_angles:
        angles = forces.Angles(pse, triples, kind="cosinesq", k=K_BEND, theta0=THETA0, virial=True)
        logs["bend"] = forces.StressLog(angles, period=10, capacity=10)
    torch.cuda.synchronize()
    t0 = time.time()
    for blk in range(5):
        s.run(100)
        ok = bool(torch.isfinite(s.pos).all())
        p = s.pos[:, :3].cpu().numpy()
        print(blk, 'finite', ok, 'xy', round(s.box[3], 4), 'm', pse.cpp_method.lanczosIterations(),
              '<cos theta> %.4f' % mean_bond_angle_cosine(p, s.box, triples), '<Rg> %.4f' % radius_of_gyration(p, s.box, nchains, beads))
        assert ok
        for name, log in logs.items():
            tab = log.table()   # columns: forces.StressLog.COLUMNS
            print('   ', name, len(tab), 'samples, steps', int(tab[0, 0]), '-', int(tab[-1, 0]), ' <U> %.6g  <sigma_xy> %.6g  sigma_xy(last) %.6g at xy %.4f'
                  '  acted(last) %d' % (tab[:, 2].mean(), tab[:, 4].mean(), tab[-1, 4], tab[-1, 1], int(tab[-1, 9])))
            assert np.isfinite(tab).all()
        assert bonds.overstretched == 0
    torch.cuda.synchronize()
    dt = time.time() - t0
    print('500 steps in %.2f s, %.3f ms per step, %s' % (dt, 2.0 * dt, 'with angles' if with_angles else 'without angles'))


if __name__ == "__main__":
    main(sys.argv[1:])
