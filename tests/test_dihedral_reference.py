"""CPU tests of the NumPy reference the dihedral forces are compared with on the GPU (tests/dihedral_ref.py), on EVERY fixed input
of tests/test_gpu_dihedrals.py: its forces are minus the gradient of its energy (both kinds, every multiplicity, both d, several
phi0), the sign convention is the IUPAC one at hand-computed geometries, its virial has the physical sign (dU/d(strain) = -Wxy
under an affine shear of box and positions), is symmetric and traceless, the forces of every dihedral add up to zero, the result
does not depend on how the list is written, and both bond angles of every dihedral of those inputs have sin >= 0.05 -- except the
exactly collinear triples of the degenerate case."""
import numpy as np
import pytest

import dihedral_ref as dr

BOX = dr.BOXES[1]


@pytest.fixture(scope="module")
def cases(oracle):
    return list(dr.all_cases(oracle))


def observables(pos, box, c, oracle):
    return dr.dihedral_observables(pos, box, c["quads"], c["types"], c["kinds"], c["params"], oracle)


def terms(c, box, oracle):
    return dr.dihedral_terms(c["pos"], box, c["quads"], c["types"], c["kinds"], c["params"], oracle)


def test_the_inputs_are_all_there(cases):
    assert len(cases) == 2 * (2 * (len(dr.ROW_COUNTS) + len(dr.TOPOLOGIES) + 1) + 2)
    for label, box, c in cases:
        assert len(c["pos"]) <= dr.N_MAX and c["quads"].max() < len(c["pos"])
        assert all(len(set(q)) == 4 for q in c["quads"].tolist()), label
        if label.startswith("chain") and label != "chains":
            assert len(c["quads"]) == len(c["pos"]) - 3
        else:
            assert len(c["pos"]) == dr.N_TOPOLOGY and len(np.setdiff1d(np.arange(dr.N_TOPOLOGY), np.unique(c["quads"]))) > 0
    assert dr.ROW_COUNTS == (4, 63, 64, 65, 255, 256, 257, 513)


def test_both_bond_angles_of_every_dihedral_of_every_gpu_input_are_away_from_straight_and_folded(oracle, cases):
    """sin >= 0.05 for the bond angles at j and at k of every dihedral, asserted on the reference's own geometry; the degenerate case
    has exactly its collinear triples (sin == 0) and nothing in between.  The arms of the prescribed geometries lie in the angle
    generators' range [0.6, 1.6] (the ring's zigzag: sqrt(1.25)), those of the random graph in [0.05, 3]: every arm is far shorter
    than half the smallest perpendicular width (5.5)."""
    lowest = 1.0
    for label, box, c in cases:
        s = dr.sines(c["pos"], box, c["quads"], oracle)
        assert len(s) == 2 * len(c["quads"]), label
        flat = s == 0.0
        assert (flat.sum() > 0) == (c["degenerate"] > 0), (label, int(flat.sum()))
        assert np.all(s[~flat] >= dr.SIN_MIN), (label, s[~flat].min())
        lowest = min(lowest, s[~flat].min())
        r = dr.arm_lengths(c["pos"], box, c["quads"], oracle)
        lo, hi = dr.GRAPH_ARM_RANGE if label == "graph" else (0.6, 3.0) if label == "degenerate" else dr.ARM_RANGE
        assert lo <= r.min() and r.max() <= hi, (label, r.min(), r.max())
        q = terms(c, box, oracle)
        assert int((~q["acts"]).sum()) == c["degenerate"], label
    print("smallest sin of a bond angle of all inputs:", lowest)


def test_forces_are_minus_the_gradient_of_the_energy(oracle, cases):
    """Central differences at h = 1e-5 on every coordinate of eight particles of every input.  The truncation is h^2/6 times the third
    derivative of V along the coordinate, at most ~ k mult^3 / (r sin)^3 ~ 30 * 216 / (0.03)^3 in the worst corner but 1e-10 times
    that; the rounding of the energy difference is ~ 1e-16 U / h ~ 1e-8.  Asserted at 1e-5 max(1, max |F|).  The particles of the
    degenerate dihedrals are left out: there phi is not defined."""
    h = 1e-5
    worst = 0.0
    for label, box, c in cases:
        pos = c["pos"]
        obs, F = observables(pos, box, c, oracle)
        assert obs[7] == len(c["quads"]) - c["degenerate"] and np.abs(F).max() > 0.1, label
        members = np.unique(c["quads"])
        if c["degenerate"]:
            members = members[members >= 12]
        for p in members[:: max(1, len(members) // 8)]:
            for a in range(3):
                up, dn = pos.copy(), pos.copy()
                up[p, a] += h; dn[p, a] -= h
                g = (observables(up, box, c, oracle)[0][0] - observables(dn, box, c, oracle)[0][0]) / (2.0 * h)
                err = abs(g + F[p, a]) / max(1.0, np.abs(F).max())
                worst = max(worst, err)
                assert err <= 1e-5, (label, p, a, g, F[p, a])
    print("largest |dU/dx + F| / max(1, max |F|):", worst)


PARAM_SETS = [(dr.HARMONIC, (7.0, d, float(mult), phi0)) for mult in range(1, 7) for d in (-1.0, 1.0) for phi0 in (0.0, 0.9, -2.5)] \
    + [(dr.OPLS, (3.0, -2.0, 5.0, 1.5)), (dr.OPLS, (0.0, 0.0, 0.0, 4.0)), (dr.OPLS, (1.0, 0.0, 0.0, 0.0)), (dr.OPLS, (0.0, 0.0, -2.0, 0.0))]


def test_gradient_on_random_quadruples_for_every_multiplicity_sign_and_phase(oracle):
    """200 random quadruples with bond-angle sines >= 0.2, h = 1e-6, each with the next of the 40 parameter sets (both kinds, every
    multiplicity 1..6, both d, three phi0, four OPLS sets): all twelve force components against central differences of V, at 1e-6
    of the largest force (the noise of the difference quotient is some 1e-9); the four forces add up to zero, W is symmetric and
    traceless, and the same geometry written (l, k, j, i) has the same phi and the mirrored forces.  If a sign of the written
    forces ever disagrees with the gradient, the gradient is right."""
    rng = np.random.default_rng(11)
    h, worst, done = 1e-6, 0.0, 0
    big = (1000.0, 1000.0, 1000.0, 0.0)
    one = [[0, 1, 2, 3]]
    while done < 200:
        pos = rng.normal(size=(4, 3))
        if dr.sines(pos, big, one, oracle).min() < 0.2:
            continue
        kind, params = PARAM_SETS[done % len(PARAM_SETS)]
        done += 1
        f = lambda p: dr.dihedral_observables(p, big, one, None, [kind], [params], oracle)   # noqa: E731
        obs, F = f(pos)
        scale = max(1.0, np.abs(F).max())
        for p in range(4):
            for a in range(3):
                up, dn = pos.copy(), pos.copy()
                up[p, a] += h; dn[p, a] -= h
                g = (f(up)[0][0] - f(dn)[0][0]) / (2.0 * h)
                worst = max(worst, abs(g + F[p, a]) / scale)
        assert np.abs(F.sum(axis=0)).max() <= 1e-13 * max(1.0, np.abs(F).sum())
        t1 = dr.dihedral_terms(pos, big, one, None, [kind], [params], oracle)
        t2 = dr.dihedral_terms(pos[::-1], big, one, None, [kind], [params], oracle)   # the same geometry written l, k, j, i
        W = dr.virial_tensor(t1)
        assert np.abs(W - W.T).max() <= 1e-12 * scale and abs(np.trace(W)) <= 1e-12 * scale
        assert abs(t1["phi"][0] - t2["phi"][0]) <= 1e-13
        assert np.abs(t1["Fi"] - t2["Fl"]).max() <= 1e-12 * scale and np.abs(t1["Fj"] - t2["Fk"]).max() <= 1e-12 * scale
    print("largest |dV/dx + F| / max(1, max |F|):", worst)
    assert worst <= 1e-6


def test_sign_convention_at_hand_computed_geometries(oracle):
    """cis -> 0, trans -> pi, and i = (0,1,0), j = 0, k = (1,0,0), l = (1,0,1) -> +pi/2 (IUPAC); V there for both kinds."""
    big = (1000.0, 1000.0, 1000.0, 0.0)
    j, k = np.zeros(3), np.array([1.0, 0.0, 0.0])
    geo = {"cis": (np.array([[0.0, 1.0, 0.0], j, k, [1.0, 1.0, 0.0]]), 0.0), "trans": (np.array([[0.0, 1.0, 0.0], j, k, [1.0, -1.0, 0.0]]), np.pi),
           "quarter": (np.array([[0.0, 1.0, 0.0], j, k, [1.0, 0.0, 1.0]]), 0.5 * np.pi),
           "minus quarter": (np.array([[0.0, 1.0, 0.0], j, k, [1.0, 0.0, -1.0]]), -0.5 * np.pi)}
    kh, d, mult, phi0 = 3.0, -1.0, 2.0, 0.4
    k1, k2, k3, k4 = 1.0, 2.0, 3.0, 4.0
    for name, (pos, phi) in geo.items():
        q = dr.dihedral_terms(pos, big, [[0, 1, 2, 3]], None, [dr.HARMONIC], [(kh, d, mult, phi0)], oracle)
        assert abs(q["phi"][0] - phi) <= 1e-15, (name, q["phi"][0])
        assert abs(q["V"][0] - 0.5 * kh * (1.0 + d * np.cos(mult * phi - phi0))) <= 1e-14, name
        q = dr.dihedral_terms(pos, big, [[0, 1, 2, 3]], None, [dr.OPLS], [(k1, k2, k3, k4)], oracle)
        V = 0.5 * (k1 * (1 + np.cos(phi)) + k2 * (1 - np.cos(2 * phi)) + k3 * (1 + np.cos(3 * phi)) + k4 * (1 - np.cos(4 * phi)))
        assert abs(q["V"][0] - V) <= 1e-14, name
    # the numbers themselves: OPLS at cis = k1 + k3, at trans = 0, at +-pi/2 = (k1 + 2 k2 + k3) / 2
    for name, V in (("cis", k1 + k3), ("trans", 0.0), ("quarter", 0.5 * (k1 + 2 * k2 + k3)), ("minus quarter", 0.5 * (k1 + 2 * k2 + k3))):
        obs, _ = dr.dihedral_observables(geo[name][0], big, [[0, 1, 2, 3]], None, [dr.OPLS], [(k1, k2, k3, k4)], oracle)
        assert abs(obs[0] - V) <= 1e-14 and obs[7] == 1.0, name
    # at +pi/2, harmonic k = 2, mult = 1, d = 1, phi0 = 0: V = k/2 = 1, g = -k/2 = -1; m = d1 x d2 = (0, 0, -1), nn = d2 x d3 = (0, 1, 0):
    # F_i = -g m = (0, 0, -1), F_l = g nn = (0, -1, 0), which turns l away from i's side, towards phi = pi, the minimum of 1 + cos phi
    obs, F = dr.dihedral_observables(geo["quarter"][0], big, [[0, 1, 2, 3]], None, [dr.HARMONIC], [(2.0, 1.0, 1.0, 0.0)], oracle)
    assert abs(obs[0] - 1.0) <= 1e-15 and np.abs(F[3] - [0.0, -1.0, 0.0]).max() <= 1e-15 and np.abs(F[0] - [0.0, 0.0, -1.0]).max() <= 1e-15


def test_sign_convention_by_affine_strain(oracle, cases):
    """(U(+delta) - U(-delta)) / (2 delta) = -Wxy for the strain x -> x + delta y, xy -> xy + delta, as for the pair, bond and angle
    references: off by O(delta^2) times the third strain derivative; asserted at 1e-6 max(1, sum of |terms of Wxy|)."""
    delta = 1e-4
    seen = 0
    for label, box, c in cases:
        if c["degenerate"]:
            continue
        pos = c["pos"]
        obs, _ = observables(pos, box, c, oracle)
        q = terms(c, box, oracle)
        scale = (np.abs(q["d1"][:, 0] * q["Fi"][:, 1]) + np.abs(q["d2"][:, 0] * q["Fk"][:, 1]) + np.abs((q["d2"] - q["d3"])[:, 0] * q["Fl"][:, 1])).sum()

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
    """A dihedral angle depends on directions only: scaling everything changes nothing, so trace W = 0; W is symmetric because the
    energy is invariant under rotation; the four forces of a dihedral cancel.  All three hold per dihedral up to the rounding of
    sums of a few terms: asserted at 1e-13 times the sum of the absolute values of the terms."""
    for label, box, c in cases:
        q = terms(c, box, oracle)
        W = dr.virial_tensor(q)
        scale = sum(np.abs(q[d][:, :, None] * q[f][:, None, :]).sum() for d, f in (("d1", "Fi"), ("d2", "Fk"), ("d2", "Fl"), ("d3", "Fl")))
        obs, F = observables(c["pos"], box, c, oracle)
        assert np.abs(W - W.T).max() <= 1e-13 * scale, (label, W)
        assert abs(np.trace(W)) <= 1e-13 * scale, (label, np.trace(W), scale)
        assert abs(obs[1] + obs[4] + obs[6]) <= 1e-13 * scale and np.abs(obs[1:7] - W[np.triu_indices(3)]).max() <= 1e-13 * scale
        fs = sum(np.abs(q[f]).sum() for f in ("Fi", "Fj", "Fk", "Fl"))
        assert np.abs(q["Fi"] + q["Fj"] + q["Fk"] + q["Fl"]).max() <= 1e-13 * np.abs(q["Fi"]).max() * 40.0
        assert np.abs(F.sum(axis=0)).max() <= 1e-13 * fs, (label, F.sum(axis=0))
        assert np.isfinite(obs).all() and np.isfinite(F).all()


def test_list_order_and_quadruple_reversal_change_nothing(oracle):
    c = dr.topology_case("two_types", BOX, dr.HARMONIC, oracle)
    ref = observables(c["pos"], BOX, c, oracle)
    rng = np.random.default_rng(1)
    o = rng.permutation(len(c["quads"]))
    quads = c["quads"][o].copy()
    flip = rng.uniform(size=len(quads)) < 0.5
    quads[flip] = quads[flip, ::-1]
    got = dr.dihedral_observables(c["pos"], BOX, quads, c["types"][o], c["kinds"], c["params"], oracle)
    assert flip.any() and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_coincident_members_and_collinear_triples(oracle):
    """A zero-length arm (also through a periodic image) or three consecutive collinear particles: nothing, not counted; the proper
    dihedral beside them acts as if it were alone."""
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.5, 2.5, 3.5], [1.0 + BOX[0], 2.0, 3.0], [0.5, 2.0, 3.9], [2.0, 1.0, 3.0]])
    quads = [[0, 1, 2, 4], [4, 2, 3, 1], [5, 1, 3, 2], [5, 2, 1, 4]]         # i at j; l an image of k; k an image of j; a proper one
    for kind in (dr.HARMONIC, dr.OPLS):
        obs, F = dr.dihedral_observables(pos, BOX, quads, None, [kind], [dr.PARAMS[kind]], oracle)
        one, F1 = dr.dihedral_observables(pos, BOX, quads[3:], None, [kind], [dr.PARAMS[kind]], oracle)
        q = dr.dihedral_terms(pos, BOX, quads, None, [kind], [dr.PARAMS[kind]], oracle)
        assert obs[7] == 1.0 and np.array_equal(obs, one) and np.array_equal(F, F1) and np.abs(F).max() > 0.1, (kind, obs[7], q["acts"])
    c = dr.degenerate_case(BOX, oracle)
    q = terms(c, BOX, oracle)
    assert int((~q["acts"]).sum()) == 6 and np.all(q["i"][~q["acts"]] < 12) and q["acts"][q["i"] >= 12].all()
    for f in ("Fi", "Fj", "Fk", "Fl", "V"):
        assert not q[f][~q["acts"]].any()
    obs, F = observables(c["pos"], BOX, c, oracle)
    assert obs[7] == 2.0 and not F[:12].any() and np.abs(F[12:16]).min(axis=0).max() > 0.1
