"""Amphiphilic A-B diblock copolymers: 100 chains of 20 beads at phi = 0.08, the first half of every chain of type A, the second of
type B -- equal beads that differ only in how they interact.  Harmonic bonds (forces.Bonds) with the bonded pairs excluded from the
pair potentials (forces.Exclusions.from_topology, HOOMD's default), and ONE typed pair provider (forces.TypedTablePair,
pse_pair_table_typed) with a table per pair of types: A-A a Morse well just outside contact, A-B and B-B the repulsive core of the
same Morse alone, cut and shifted at its minimum -- the solvophobic block attracts itself, the corona only keeps its distance.  With
hydrodynamic interactions and Brownian motion, no shear.

Prints, every 250 steps, the A-A and the B-B contacts per bead: pairs of that pair of types, not bonded, closer than R_CONTACT.  Each
is the `npairs` of a TypedTablePair(virial=True) of its own whose one table is zero on [0, R_CONTACT) with every other pair type
off: it adds no force and counts exactly those pairs.  The A blocks find each other and their number grows; the B blocks stay
where the excluded volume leaves them.  A plain TablePair cannot express this: it would attract every bead to every other.
`--chains C --beads B --steps S` change the size."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sticky_polymers import build_topology, mean_bond_length   # noqa: E402

K_BOND, R0_BOND = 100.0, 2.0            # harmonic bonds, in kT / a^2 and bead radii a
D_WELL, ALPHA, R_WELL = 4.0, 2.0, 2.2   # Morse D ((1 - e^{-alpha (r - R_WELL)})^2 - 1): a well of 4 kT just outside contact (r = 2)
R_MIN, R_MAX, WIDTH = 0.5, 4.5, 1024    # the range and the nodes of the A-A table; the cores end at R_WELL
R_CONTACT = 2.6                         # two beads closer than this are in contact
DT, BLOCK = 2e-3, 250


def morse(r):
    e = math.exp(-ALPHA * (r - R_WELL))
    return D_WELL * ((1.0 - e) ** 2 - 1.0)


def morse_force(r):
    e = math.exp(-ALPHA * (r - R_WELL))
    return -2.0 * D_WELL * ALPHA * (1.0 - e) * e


def core(r):
    """The repulsive branch of the Morse potential, shifted to end at zero where its force does."""
    return morse(r) + D_WELL


def main(argv):
    import torch
    from pse_amd import integrate, forces
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
    zero = (np.zeros((2, 2)), 0.0, R_CONTACT)
    count = {key: forces.TypedTablePair(pse, types, {key: zero}, virial=True, exclusions=excl, type_names=names)
             for key in (("A", "A"), ("B", "B"))}
    per_type = {name: int((types == name).sum()) for name in names}
    print("%d chains of %d beads (%d A, %d B), L = %.2f, %d excluded pairs" % (nchains, beads, per_type["A"], per_type["B"], L, excl.npairs_listed))
    torch.cuda.synchronize()
    t0 = time.time()
    first = last = None
    for blk in range(steps // BLOCK):
        s.run(BLOCK)
        ok = bool(torch.isfinite(s.pos).all())
        p = s.pos[:, :3].cpu().numpy()
        # a contact has two ends: 2 npairs / beads of the type
        last = {key[0]: 2.0 * c.npairs / per_type[key[0]] for key, c in count.items()}
        first = first or last
        print('  step', (blk + 1) * BLOCK, 'finite', ok, '<bond> %.4f' % mean_bond_length(p, s.box, pairs),
              'A-A contacts per A bead %.3f' % last["A"], 'B-B contacts per B bead %.3f' % last["B"])
        assert ok
    torch.cuda.synchronize()
    print('%d steps in %.2f s' % (steps // BLOCK * BLOCK, time.time() - t0))
    print('contacts per bead, first block -> last: A-A %.3f -> %.3f, B-B %.3f -> %.3f' % (first["A"], last["A"], first["B"], last["B"]))


if __name__ == "__main__":
    main(sys.argv[1:])
