"""CPU tests of the NumPy reference the bonded forces are compared with on the GPU (tests/bond_ref.py): its forces are the gradient
of its energy, its virial has the physical sign (dU/d(strain) = -Wxy under an affine shear of box and positions), harmonic bonds on
the overlapping pairs reproduce the pair reference of the harmonic repulsion, the result does not depend on how the list is written,
and every fixed input of the GPU tests has its FENE bonds where the bound of those tests needs them."""
import numpy as np
import pytest

import bond_ref as br
from pair_virial_ref import pair_observables, pair_terms, random_points

BOX = br.BOXES[1]


def mixed_case(oracle):
    return br.topology_case("two_types", BOX, br.HARMONIC, oracle)


def energy(pos, box, c, oracle):
    return br.bond_observables(pos, box, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)[0][0]


@pytest.mark.parametrize("kind", [br.HARMONIC, br.FENE])
@pytest.mark.parametrize("name", ["chains", "star", "faces", "graph"])
def test_forces_are_minus_the_gradient_of_the_energy(oracle, kind, name):
    """Central differences at h = 1e-5 on every coordinate of 12 bonded particles.  The truncation is h^2/6 |V'''| per bond: with
    (r/r0)^2 <= 0.9 the FENE third derivative is below ~1e4 k, so ~2e-7 k; asserted at 1e-5 max(1, max |F|)."""
    c = br.graph_case(BOX, kind, oracle) if name == "graph" else br.topology_case(name, BOX, kind, oracle)
    pos = c["pos"]
    obs, F, over = br.bond_observables(pos, BOX, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)
    assert over == 0 and obs[7] == len(c["pairs"]) and np.abs(F).max() > 1.0
    assert np.abs(F.sum(axis=0)).max() <= 1e-11 * np.abs(F).max()            # Newton's third law
    h = 1e-5
    bonded = np.unique(c["pairs"])
    for p in bonded[:: max(1, len(bonded) // 12)]:
        for a in range(3):
            up, dn = pos.copy(), pos.copy()
            up[p, a] += h; dn[p, a] -= h
            g = (energy(up, BOX, c, oracle) - energy(dn, BOX, c, oracle)) / (2.0 * h)
            assert abs(g + F[p, a]) <= 1e-5 * max(1.0, np.abs(F).max()), (p, a, g, F[p, a])


@pytest.mark.parametrize("kind", [br.HARMONIC, br.FENE])
def test_sign_convention_by_affine_strain(oracle, kind):
    """(U(+delta) - U(-delta)) / (2 delta) = -Wxy for the strain x -> x + delta y, xy -> xy + delta, as for the pair reference
    (tests/test_pair_virial_reference.py): off by O(delta^2) times the third strain derivative; asserted at 1e-6 max(1, sum |c dx dy|)."""
    delta = 1e-4
    c = br.topology_case("chains", BOX, kind, oracle)
    pos = c["pos"]
    obs, _, _ = br.bond_observables(pos, BOX, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)
    i, j, d, r, cc, V, acts, over = br.bond_terms(pos, BOX, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)
    scale = np.abs(cc * d[:, 0] * d[:, 1]).sum()
    assert abs(obs[2]) > 1e-3 * scale

    def u(e):
        p = pos.copy()
        p[:, 0] += e * p[:, 1]
        return energy(p, BOX[:3] + (BOX[3] + e,), c, oracle)

    slope = (u(delta) - u(-delta)) / (2.0 * delta)
    err = abs(slope + obs[2])
    print(f"dU/dstrain = {slope:.12g}, -Wxy = {-obs[2]:.12g}, |difference| = {err:.3e}, scale {scale:.6g}")
    assert err <= 1e-6 * max(1.0, scale), (slope, -obs[2], err, scale)


@pytest.mark.parametrize("xy", [0.0, 0.3])
def test_harmonic_bonds_on_the_overlapping_pairs_are_the_harmonic_repulsion(oracle, xy):
    """Bonds with r0 = sigma on exactly the pairs pair_terms finds: V = k/2 (r - sigma)^2 and c = -k (r - sigma)/r are the
    repulsion's terms, so U, W, the count and the forces agree to rounding."""
    k, sigma = 40.0, 2.0
    box = (14.0, 11.0, 17.0, xy)
    pos = random_points(300, box, seed=11)
    i, j, d, c, r = pair_terms(pos, box, k, sigma, oracle)
    assert len(i) > 20
    ref, Fref = pair_observables(pos, box, k, sigma, oracle)
    obs, F, over = br.bond_observables(pos, box, np.stack([i, j], axis=1), None, [br.HARMONIC], [k], [sigma], oracle)
    assert over == 0 and obs[7] == ref[7]
    assert np.abs(obs - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    assert np.abs(F - Fref).max() <= 1e-13 * max(1.0, np.abs(Fref).max())


def test_list_order_and_endpoint_order_change_nothing(oracle):
    c = mixed_case(oracle)
    ref = br.bond_observables(c["pos"], BOX, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)
    rng = np.random.default_rng(1)
    o = rng.permutation(len(c["pairs"]))
    pairs = c["pairs"][o].copy()
    flip = rng.uniform(size=len(pairs)) < 0.5
    pairs[flip] = pairs[flip, ::-1]
    got = br.bond_observables(c["pos"], BOX, pairs, c["types"][o], c["kinds"], c["k"], c["r0"], oracle)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]


def test_overstretched_and_coincident_bonds_are_left_out(oracle):
    c = br.overstretch_case(BOX, oracle)
    obs, F, over = br.bond_observables(c["pos"], BOX, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)
    assert over == 3 and obs[7] == len(c["pairs"]) - 3 and np.isfinite(obs).all() and np.isfinite(F).all()
    q = br.fene_ratios(c["pos"], BOX, c["pairs"], None, c["kinds"], c["r0"], oracle)
    keep = q < 1.0                  # (a chain's list is in canonical order already: q is in list order)
    part = br.bond_observables(c["pos"], BOX, c["pairs"][keep], None, c["kinds"], c["k"], c["r0"], oracle)
    # (zeros in a NumPy sum move the blocks of its pairwise summation: equal to rounding, not bit for bit)
    assert np.abs(part[0] - obs).max() <= 1e-13 * np.abs(obs).max() and np.array_equal(part[1], F) and part[2] == 0
    # r == 0: nothing, not counted, not overstretched
    pos = np.zeros((2, 3))
    for kind in (br.HARMONIC, br.FENE):
        o, f, n = br.bond_observables(pos, BOX, [[0, 1]], None, [kind], [30.0], [1.5], oracle)
        assert not o.any() and not f.any() and n == 0


def test_fene_bonds_of_every_gpu_input_are_inside_the_range_of_the_bound(oracle):
    """(r/r0)^2 <= 0.9 for every acting FENE bond, r/r0 >= 1.05 for the overstretched ones and exactly as many of those as the case
    says: the generators prescribe the bond lengths, this is the check that they did."""
    seen = 0
    for label, box, c in br.all_cases(oracle):
        br.assert_fene_in_range(c["pos"], box, c["pairs"], c["types"], c["kinds"], c["r0"], oracle, c["n_over"])
        obs, F, over = br.bond_observables(c["pos"], box, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)
        assert over == c["n_over"] and obs[7] == len(c["pairs"]) - over, label
        # every bond is far shorter than half the smallest perpendicular width (5.5): the minimum image is the bond
        r = br.bond_terms(c["pos"], box, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], oracle)[3]
        assert 0.0 < r.min() and r.max() < 2.0, (label, r.min(), r.max())
        seen += 1
    assert seen == 2 * (2 * (len(br.ROW_COUNTS) + len(br.TOPOLOGIES) + 1) + 1)


def test_prescribed_lengths_are_what_the_generators_deliver(oracle):
    rng = np.random.default_rng(3)
    step = br.lengths(rng, 3 * 19, 0.5, 1.4)
    pos, pairs = br.chains(3, 20, BOX, step, 5, oracle)
    d = oracle.min_image(pos[pairs[:, 0]] - pos[pairs[:, 1]], BOX)
    assert np.abs(np.linalg.norm(d, axis=1) - step).max() < 1e-13
    pos, pairs = br.ring(50, BOX, 1.0, 0.4, 5, oracle)
    d = oracle.min_image(pos[pairs[:, 0]] - pos[pairs[:, 1]], BOX)
    assert len(pairs) == 50 and np.abs(np.linalg.norm(d, axis=1) - np.sqrt(1.16)).max() < 1e-12
    arm = br.lengths(rng, 40, 0.5, 1.4)
    pos, pairs = br.star(40, BOX, arm, 5, oracle)
    d = oracle.min_image(pos[pairs[:, 0]] - pos[pairs[:, 1]], BOX)
    assert np.all(pairs[:, 0] == 0) and np.abs(np.linalg.norm(d, axis=1) - arm).max() < 1e-13
    pos, pairs = br.random_graph(60, 200, BOX, 1.4, 5, oracle)
    d = oracle.min_image(pos[pairs[:, 0]] - pos[pairs[:, 1]], BOX)
    r = np.linalg.norm(d, axis=1)
    assert np.all(pairs[:, 0] != pairs[:, 1]) and 0.0 < r.min() and r.max() <= 1.4
