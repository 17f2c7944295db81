"""CPU tests of the NumPy reference the angle forces are compared with on the GPU (tests/angle_ref.py), on EVERY fixed input of
tests/test_gpu_angles.py: its forces are minus the gradient of its energy, its virial has the physical sign (dU/d(strain) = -Wxy under
an affine shear of box and positions), is symmetric and traceless, the forces of every angle add up to zero, the result does not
depend on how the list is written, and every angle of those inputs has sin(theta) >= 0.05 -- the condition under which two acos
implementations can agree to the bound of the GPU tests -- except the exactly collinear triples of the collinear case."""
import numpy as np
import pytest

import angle_ref as ar

BOX = ar.BOXES[1]


@pytest.fixture(scope="module")
def cases(oracle):
    return list(ar.all_cases(oracle))


def observables(pos, box, c, oracle):
    return ar.angle_observables(pos, box, c["triples"], c["types"], c["kinds"], c["k"], c["theta0"], oracle)


def terms(c, box, oracle):
    return ar.angle_terms(c["pos"], box, c["triples"], c["types"], c["kinds"], c["k"], c["theta0"], oracle)


def test_the_inputs_are_all_there(cases):
    assert len(cases) == 2 * (2 * (len(ar.ROW_COUNTS) + len(ar.TOPOLOGIES) + 1) + 1)
    for label, box, c in cases:
        assert len(c["pos"]) <= ar.N_MAX and c["triples"].max() < len(c["pos"])
        if label.startswith("chain") and label != "chains":
            assert len(c["triples"]) == len(c["pos"]) - 2
        else:
            assert len(c["pos"]) == ar.N_TOPOLOGY and len(np.setdiff1d(np.arange(ar.N_TOPOLOGY), np.unique(c["triples"]))) > 0


def test_every_angle_of_every_gpu_input_is_away_from_the_straight_and_the_folded_angle(oracle, cases):
    """sin(theta) >= 0.05 for every angle, asserted on the reference's own geometry; the collinear case has exactly its seven
    collinear angles (sin == 0) and nothing in between.  Every arm is far shorter than half the smallest perpendicular width (5.5)."""
    lowest = 1.0
    for label, box, c in cases:
        s = ar.sines(c["pos"], box, c["triples"], oracle)
        assert len(s) == len(c["triples"]), label
        flat = s == 0.0
        assert int(flat.sum()) == c["collinear"], (label, int(flat.sum()))
        assert np.all(s[~flat] >= ar.SIN_MIN), (label, s[~flat].min())
        lowest = min(lowest, s[~flat].min())
        r = ar.arm_lengths(c["pos"], box, c["triples"], oracle)
        assert 0.3 < r.min() and r.max() < 3.0, (label, r.min(), r.max())
    print("smallest sin(theta) of all inputs:", lowest)


def test_forces_are_minus_the_gradient_of_the_energy(oracle, cases):
    """Central differences at h = 1e-5 on every coordinate of eight particles of every input.  The truncation is h^2/6 times the third
    derivative of V along the coordinate, at most ~ k / (r^3 sin^2(theta)) ~ 30 / (0.2 * 0.0025) = 6e4: 1e-6; the rounding of the
    energy difference is ~ 1e-16 U / h ~ 1e-8.  Asserted at 1e-5 max(1, max |F|).  The particles of the exactly collinear triples
    are left out: there the harmonic energy has a cusp and the capped force is not its gradient."""
    h = 1e-5
    worst = 0.0
    for label, box, c in cases:
        pos = c["pos"]
        obs, F = observables(pos, box, c, oracle)
        assert obs[7] == len(c["triples"]) and np.abs(F).max() > 0.1, label
        members = np.unique(c["triples"])
        if c["collinear"]:
            members = members[members >= 6]
        for p in members[:: max(1, len(members) // 8)]:
            for a in range(3):
                up, dn = pos.copy(), pos.copy()
                up[p, a] += h; dn[p, a] -= h
                g = (observables(up, box, c, oracle)[0][0] - observables(dn, box, c, oracle)[0][0]) / (2.0 * h)
                err = abs(g + F[p, a]) / max(1.0, np.abs(F).max())
                worst = max(worst, err)
                assert err <= 1e-5, (label, p, a, g, F[p, a])
    print("largest |dU/dx + F| / max(1, max |F|):", worst)


def test_sign_convention_by_affine_strain(oracle, cases):
    """(U(+delta) - U(-delta)) / (2 delta) = -Wxy for the strain x -> x + delta y, xy -> xy + delta, as for the pair and bond
    references: off by O(delta^2) times the third strain derivative; asserted at 1e-6 max(1, sum |d1x Fiy| + |d2x Fky|)."""
    delta = 1e-4
    seen = 0
    for label, box, c in cases:
        if c["collinear"]:
            continue
        pos = c["pos"]
        obs, _ = observables(pos, box, c, oracle)
        q = terms(c, box, oracle)
        scale = (np.abs(q["d1"][:, 0] * q["Fi"][:, 1]) + np.abs(q["d2"][:, 0] * q["Fk"][:, 1])).sum()

        def u(e):
            p = pos.copy()
            p[:, 0] += e * p[:, 1]
            return observables(p, box[:3] + (box[3] + e,), c, oracle)[0][0]

        slope = (u(delta) - u(-delta)) / (2.0 * delta)
        err = abs(slope + obs[2])
        assert err <= 1e-6 * max(1.0, scale), (label, slope, -obs[2], err, scale)
        seen += abs(obs[2]) > 1e-3 * scale
    assert seen > len(cases) // 2          # ... and Wxy is not small against its terms in most of them


def test_virial_is_symmetric_and_traceless_and_forces_add_up_to_zero(oracle, cases):
    """Angle potentials depend on directions only: scaling everything changes nothing, so trace W = -dU/d(ln scale) = 0; W is
    symmetric because the energy is invariant under rotation; the three forces of an angle cancel.  All three hold per angle up
    to the rounding of sums of a few terms: asserted at 1e-13 times the sum of the absolute values of the terms."""
    for label, box, c in cases:
        q = terms(c, box, oracle)
        W = ar.virial_tensor(q)
        scale = np.abs(q["d1"][:, :, None] * q["Fi"][:, None, :]).sum() + np.abs(q["d2"][:, :, None] * q["Fk"][:, None, :]).sum()
        obs, F = observables(c["pos"], box, c, oracle)
        assert np.abs(W - W.T).max() <= 1e-13 * scale, (label, W)
        assert abs(np.trace(W)) <= 1e-13 * scale, (label, np.trace(W), scale)
        assert abs(obs[1] + obs[4] + obs[6]) <= 1e-13 * scale and np.abs(obs[1:7] - W[np.triu_indices(3)]).max() <= 1e-13 * scale
        fs = np.abs(q["Fi"]).sum() + np.abs(q["Fk"]).sum()
        assert np.abs(F.sum(axis=0)).max() <= 1e-13 * fs, (label, F.sum(axis=0))
        assert np.isfinite(obs).all() and np.isfinite(F).all()


def test_list_order_and_end_order_change_nothing(oracle):
    c = ar.topology_case("two_types", BOX, ar.HARMONIC, oracle)
    ref = observables(c["pos"], BOX, c, oracle)
    rng = np.random.default_rng(1)
    o = rng.permutation(len(c["triples"]))
    triples = c["triples"][o].copy()
    flip = rng.uniform(size=len(triples)) < 0.5
    triples[flip] = triples[flip, ::-1]
    got = ar.angle_observables(c["pos"], BOX, triples, c["types"][o], c["kinds"], c["k"], c["theta0"], oracle)
    assert flip.any() and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_the_two_potentials_at_hand_computed_values(oracle):
    """A right angle with arms 1 and 2 along x and y: c = 0, theta = pi/2.  harmonic, k = 3, theta0 = 2: V = 1.5 (pi/2 - 2)^2,
    g = 3 (pi/2 - 2); cosinesq, k = 3, theta0 = 2: V = 1.5 cos^2(2), g = 3 cos(2).  With c = 0 the forces are F_i = g d2 / (r1 r2) =
    (0, g, 0) and F_k = g d1 / (r1 r2) = (g/2, 0, 0): perpendicular to the own arm, g over its length."""
    pos = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    for kind, g, V in ((ar.HARMONIC, 3.0 * (np.pi / 2 - 2.0), 1.5 * (np.pi / 2 - 2.0) ** 2), (ar.COSINESQ, 3.0 * np.cos(2.0), 1.5 * np.cos(2.0) ** 2)):
        obs, F = ar.angle_observables(pos, BOX, [[0, 1, 2]], None, [kind], [3.0], [2.0], oracle)
        Fi, Fk = np.array([0.0, g / 1.0, 0.0]), np.array([g / 2.0, 0.0, 0.0])
        assert abs(obs[0] - V) <= 1e-15 and obs[7] == 1.0
        assert np.abs(F - np.array([Fi, -(Fi + Fk), Fk])).max() <= 1e-15
        # W_xy = d1_x F_i,y + d2_x F_k,y = g, W_yx = d2_y F_k,x = g; the diagonal is zero
        assert abs(obs[2] - g) <= 1e-15 and abs(obs[1]) + abs(obs[4]) + abs(obs[6]) <= 1e-15


def test_coincident_members_and_collinear_triples(oracle):
    """r1 == 0 or r2 == 0 (also through a periodic image): nothing, not counted.  The collinear triples give exactly c = -1 / +1,
    zero force and the energies k/2 (theta - theta0)^2 and k/2 (c - cos theta0)^2."""
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.5, 2.5, 3.5], [1.0 + BOX[0], 2.0, 3.0], [0.5, 2.0, 3.0]])
    for kind in (ar.HARMONIC, ar.COSINESQ):
        obs, F = ar.angle_observables(pos, BOX, [[0, 1, 2], [2, 3, 1], [2, 1, 4]], None, [kind], [30.0], [2.0], oracle)
        one, F1 = ar.angle_observables(pos, BOX, [[2, 1, 4]], None, [kind], [30.0], [2.0], oracle)
        assert obs[7] == 1.0 and np.array_equal(obs, one) and np.array_equal(F, F1) and np.abs(F).max() > 0.1
    c = ar.collinear_case(BOX, oracle)
    q = terms(c, BOX, oracle)
    flat = np.isin(q["j"], (1, 4))
    assert flat.sum() == 7 and np.array_equal(np.sort(q["c"][flat]), [-1.0] * 3 + [1.0] * 4)
    assert not q["Fi"][flat].any() and not q["Fk"][flat].any() and q["acts"].all()
    K = ar.K_C
    expect = sorted([0.0, 0.0, 0.5 * K * (-1.0 - np.cos(2.6)) ** 2,                                # straight: harmonic pi, cosinesq pi, cosinesq 2.6
                     0.5 * K * np.pi ** 2, 0.5 * K * 4.0, 0.5 * K * (1.0 - np.cos(2.6)) ** 2, 0.5 * K * 4.0])   # folded: the four types
    assert np.allclose(sorted(q["V"][flat]), expect, rtol=1e-15, atol=1e-15)
