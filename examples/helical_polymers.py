"""Helical polymers under shear: 200 bead-spring chains of 20 beads at phi = 0.1 -- the FENE bonds and the core repulsion of
semiflexible_polymers.py, a cosine-squared bending term that holds every bond angle near THETA0 (forces.Angles) and a harmonic
dihedral with a non-zero phase, V = k/2 (1 - cos(phi - PHI0)), that gives every four consecutive beads the torsion PHI0
(forces.Dihedrals / pse_dihedral_forces; phi is the IUPAC dihedral angle: cis 0, trans pi) -- with hydrodynamic interactions and
Brownian motion, under oscillatory Lees-Edwards shear; 500 steps.  The chains start as helices with a little disorder.  Prints per
block of 100 steps the mean of cos(phi - PHI0) over the dihedrals (1: perfect helices, 0: no torsional order), the mean radius of
gyration, and the bond, bending and torsion energies with their contributions to sigma_xy -- sampled every 10 steps by the three
passes themselves into device logs (forces.StressLog) that are read once per block.
`--no-dihedrals` runs the same chains without the torsion term, `--chains C --beads B` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from semiflexible_polymers import _min_image, radius_of_gyration   # noqa: E402

K_BEND, THETA0 = 40.0, 1.9         # cosine-squared: V = k/2 (cos theta - cos THETA0)^2, in kT
K_TORSION, PHI0 = 10.0, 1.0        # harmonic dihedral, d = -1, mult = 1: V = k/2 (1 - cos(phi - PHI0)), minimum at phi = PHI0
JITTER = 0.15                      # the starting bond angles and dihedrals are uniform within +-JITTER of THETA0 and PHI0


def build_topology(nchains, beads, box, bond_length, seed):
    """nchains helices of `beads` beads with bonds of length bond_length from uniform random starts and directions, wrapped into the
    (Lx, Ly, Lz, xy) box: every bond angle within JITTER of THETA0 and every dihedral within JITTER of PHI0.  Returns (pos[nchains *
    beads, 3], pairs[nchains * (beads - 1), 2], triples[nchains * (beads - 2), 3], quads[nchains * (beads - 3), 4]); chain c is the
    beads c * beads ... c * beads + beads - 1, bonded in that order, one angle at every inner bead, one dihedral per four in a row."""
    rng = np.random.default_rng(seed)
    Lx, Ly, Lz, xy = box
    unit = lambda v: v / np.linalg.norm(v, axis=-1)[..., None]
    p = np.zeros((nchains, beads, 3))
    p[:, 0] = (rng.uniform(size=(nchains, 3)) - 0.5) * np.array([Lx, Ly, Lz])
    u = unit(rng.normal(size=(nchains, 3)))
    p[:, 1] = p[:, 0] + bond_length * u
    v = unit(np.cross(u, rng.normal(size=(nchains, 3))))
    th = THETA0 + rng.uniform(-JITTER, JITTER, size=(nchains, 1))
    p[:, 2] = p[:, 1] + bond_length * (-np.cos(th) * u + np.sin(th) * v)
    for s in range(3, beads):       # bead s from the three before it: bond length, bond angle at s - 1, dihedral (s - 3, s - 2, s - 1, s)
        a, b, c = p[:, s - 3], p[:, s - 2], p[:, s - 1]
        th = THETA0 + rng.uniform(-JITTER, JITTER, size=(nchains, 1))
        ph = PHI0 + rng.uniform(-JITTER, JITTER, size=(nchains, 1))
        bc = unit(c - b)
        nrm = unit(np.cross(b - a, bc))
        p[:, s] = c + bond_length * (-np.cos(th) * bc + np.sin(th) * np.cos(ph) * np.cross(nrm, bc) + np.sin(th) * np.sin(ph) * nrm)
    pos = p.reshape(-1, 3)
    n = np.floor(pos[:, 2] / Lz + 0.5); pos[:, 2] -= n * Lz
    n = np.floor(pos[:, 1] / Ly + 0.5); pos[:, 1] -= n * Ly; pos[:, 0] -= n * xy * Ly
    n = np.floor((pos[:, 0] - xy * pos[:, 1]) / Lx + 0.5); pos[:, 0] -= n * Lx
    idx = lambda m: (np.arange(nchains)[:, None] * beads + np.arange(beads - m)[None, :]).reshape(-1)
    b1, b2, b3 = idx(1), idx(2), idx(3)
    return pos, np.stack([b1, b1 + 1], axis=1), np.stack([b2, b2 + 1, b2 + 2], axis=1), np.stack([b3, b3 + 1, b3 + 2, b3 + 3], axis=1)


def dihedral_angles(pos, box, quads):
    """phi of every quadruple (i, j, k, l), arms by the minimum image: atan2(|d2| d1.(d2 x d3), (d1 x d2).(d2 x d3)) with
    d1 = r_i - r_j, d2 = r_k - r_j, d3 = r_k - r_l (the convention of pse_dihedral_forces)."""
    d1 = _min_image(pos[quads[:, 0]] - pos[quads[:, 1]], box)
    d2 = _min_image(pos[quads[:, 2]] - pos[quads[:, 1]], box)
    d3 = _min_image(pos[quads[:, 2]] - pos[quads[:, 3]], box)
    m, nn = np.cross(d1, d2), np.cross(d2, d3)
    return np.arctan2(np.linalg.norm(d2, axis=1) * (d1 * nn).sum(axis=1), (m * nn).sum(axis=1))


def mean_dihedral_cosine(pos, box, quads):
    """Mean over the dihedrals of cos(phi - PHI0): 1 for perfect helices of the preferred torsion, 0 without torsional order."""
    return float(np.cos(dihedral_angles(pos, box, quads) - PHI0).mean())


def main(argv):
    import torch
    from pse_amd import integrate, shear_function, variant, forces
    from pse_amd.system import System
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, phi = opt("--chains", 200), opt("--beads", 20), 0.1
    with_dihedrals = "--no-dihedrals" not in argv
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    k_fene, r0 = 30.0 / 4.0, 3.0   # Kremer-Grest bonds in units of the bead radius, as in semiflexible_polymers.py
    pos, pairs, triples, quads = build_topology(nchains, beads, box, 2.0, seed=5)
    s = System(pos, box, dt=1e-3)
    ff = shear_function.sine(dt=1e-3, shear_rate=1.0, shear_freq=1.0)
    s.box_tilt_variant = variant.shear_variant(ff, 2000, max_strain=0.5)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3, function_form=ff)
    kc = 200.0   # core: k/2 (2 - r)^2 for r < 2
    forces.TablePair.from_functions(pse, lambda r: 0.5 * kc * (2.0 - r) ** 2, lambda r: kc * (2.0 - r), 0.0, 2.0, 256)
    bonds = forces.Bonds(pse, pairs, kind="fene", k=k_fene, r0=r0, virial=True)
    angles = forces.Angles(pse, triples, kind="cosinesq", k=K_BEND, theta0=THETA0, virial=True)
    logs = {"bond": forces.StressLog(bonds, period=10, capacity=10), "bend": forces.StressLog(angles, period=10, capacity=10)}
    if with_dihedrals:
        dihedrals = forces.Dihedrals(pse, quads, kind="harmonic", params=(K_TORSION, -1.0, 1.0, PHI0), virial=True)
        logs["torsion"] = forces.StressLog(dihedrals, period=10, capacity=10)
    torch.cuda.synchronize()
    t0 = time.time()
    for blk in range(5):
        s.run(100)
        ok = bool(torch.isfinite(s.pos).all())
        p = s.pos[:, :3].cpu().numpy()
        print(blk, 'finite', ok, 'xy', round(s.box[3], 4), 'm', pse.cpp_method.lanczosIterations(),
              '<cos(phi - phi0)> %.4f' % mean_dihedral_cosine(p, s.box, quads), '<Rg> %.4f' % radius_of_gyration(p, s.box, nchains, beads))
        assert ok
        for name, log in logs.items():
            tab = log.table()   # columns: forces.StressLog.COLUMNS
            print('   ', name, len(tab), 'samples, steps', int(tab[0, 0]), '-', int(tab[-1, 0]), ' <U> %.6g  <sigma_xy> %.6g  sigma_xy(last) %.6g at xy %.4f'
                  '  acted(last) %d' % (tab[:, 2].mean(), tab[:, 4].mean(), tab[-1, 4], tab[-1, 1], int(tab[-1, 9])))
            assert np.isfinite(tab).all()
        assert bonds.overstretched == 0
    torch.cuda.synchronize()
    dt = time.time() - t0
    print('500 steps in %.2f s, %.3f ms per step, %s' % (dt, 2.0 * dt, 'with dihedrals' if with_dihedrals else 'without dihedrals'))


if __name__ == "__main__":
    main(sys.argv[1:])
