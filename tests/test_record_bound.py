"""The bound of tests/record_bound.py -- derived from the un-rounded f, g and the format of the 16-byte pair records alone -- against the
oracle's restatement of the rounding (oracle/pse_oracle.c pair_term, rounded=True): the restatement is not the reference here, it is
what the bound has to cover.  Random and adversarial geometries: pairs along an axis (two components of s exactly 0), one component
1e-9 .. 1e-4 of the others (the shared exponent flushes it), overlapping and touching pairs, pairs just inside rcut, images through the
tilted box, xi from 0.2 to the large end, and pairs with h = (g - f) / r^2 < 0."""
import math

import numpy as np
import pytest

from conftest import make_suspension
import record_bound as rb

RCUT3 = math.sqrt(-math.log(1e-3))


def _pair_block(oracle, d, xi, rcut, rounded):
    """3x3 off-diagonal block of a two-particle near-field matrix with separation d (a box large enough for the minimum image)."""
    L = 4.0 * rcut + 8.0
    pos = np.array([[0.0, 0.0, 0.0], -np.asarray(d, float)])
    out = np.zeros((3, 3))
    for c in range(3):
        F = np.zeros((2, 3)); F[1, c] = 1.0
        out[:, c] = oracle.mobility_real(pos, F, (L, L, L, 0.0), xi, rcut, rounded=rounded)[0]
    return out


def _adversarial_separations(rng, xi, rcut):
    ds = []
    for r in np.concatenate([np.geomspace(1e-3, 2.0, 12), [2.0], np.linspace(2.0, rcut, 8)[1:-1], [rcut * (1 - 1e-9)]]):
        ax = rng.integers(3)
        d = np.zeros(3); d[ax] = r * rng.choice([-1, 1])                                           # (a) along one axis
        ds.append(d)
        for tiny in (1e-9, 1e-7, 1e-6, 1e-5, 1e-4):                                                 # (b) one component tiny
            u = rng.normal(size=3); u[rng.integers(3)] = tiny * rng.choice([-1, 1]) * np.abs(u).max()
            ds.append(r * u / np.linalg.norm(u))
        u = rng.normal(size=3)
        ds.append(r * u / np.linalg.norm(u))                                                        # random direction
    return ds


@pytest.mark.parametrize("xi,err", [(0.2, 1e-3), (0.5, 1e-3), (1.0, 1e-3), (2.0, 1e-3), (2.0, 1e-6), (5.0, 1e-6)])
def test_pair_bound_covers_the_restated_records(oracle, xi, err):
    """One pair at a time: ||T_rounded - T||_2 <= eps_ij = 2^-25 + 2 |g - f| 2^-20, and the bound is not vacuous (the largest
    error reaches a fair share of it)."""
    rng = np.random.default_rng(int(xi * 100) + int(-math.log10(err)))
    rcut = math.sqrt(-math.log(err)) / xi
    worst = 0.0
    for d in _adversarial_separations(rng, xi, rcut):
        r = float(np.linalg.norm(d))
        f, g = oracle.fg_real(r, xi)
        eps = float(rb.pair_eps(f, g, [r])[0])
        T = _pair_block(oracle, d, xi, rcut, rounded=False)
        Tr = _pair_block(oracle, d, xi, rcut, rounded=True)
        e = np.linalg.norm(Tr - T, 2)
        assert e <= eps, (xi, err, d, e, eps)
        worst = max(worst, e / eps)
    assert worst > 0.1, worst


def test_h_changes_sign_inside_the_cutoff(oracle):
    """xi = 2, error = 1e-6: g - f < 0 for 1.54 < r < rcut = 1.86 -- the sign bit of the records is exercised (the geometry of
    tests/test_gpu_lanczos_truth.py case (g))."""
    xi, rcut = 2.0, math.sqrt(-math.log(1e-6)) / 2.0
    r = np.linspace(1.0, rcut * (1 - 1e-9), 200)
    f, g = oracle.fg_real(r, xi)
    assert (g - f < 0).any() and (g - f > 0).any()
    neg = r[g - f < 0]
    for ri in np.concatenate([neg[::20], [neg[np.argmin((g - f)[g - f < 0])]]]):
        d = np.array([ri * 0.6, -ri * 0.8, 0.0])
        T = _pair_block(oracle, d, xi, rcut, rounded=False)
        Tr = _pair_block(oracle, d, xi, rcut, rounded=True)
        fi, gi = oracle.fg_real(ri, xi)
        assert np.linalg.norm(Tr - T, 2) <= rb.pair_eps(fi, gi, [ri])[0]
    # a record that dropped the sign would be off by 2 |g - f| there: far outside the bound
    assert 2 * abs(gi[0] - fi[0]) > 100 * rb.pair_eps(fi, gi, [ri])[0]


@pytest.mark.parametrize("name", [g["name"] for g in rb.geometries()])
def test_operator_and_sqrt_bounds_cover_the_restated_records(oracle, name):
    """||M_r - M||_2 <= max_i sum_j eps_ij, and ||M_r^{1/2} psi - M^{1/2} psi|| <= ||dM|| / (sqrt(lmin) + sqrt(lmin - ||dM||)) ||psi||,
    with M_r the restatement's rounded operator and M the un-rounded one."""
    geo = {g["name"]: g for g in rb.geometries()}[name]
    pos, box, xi, rcut = geo["pos"], geo["box"], geo["xi"], geo["rcut"]
    Lx, Ly, Lz, xy = box
    assert rcut <= 0.5 * min(Lx / math.hypot(1.0, xy), Ly, Lz), name     # the minimum image is the only image inside rcut
    i, j, r, _ = rb.pairs(pos, box, rcut)
    assert len(r) > 0, name
    M = rb.dense_mreal(oracle, pos, box, xi, rcut, rounded=False)
    Mr = rb.dense_mreal(oracle, pos, box, xi, rcut, rounded=True)
    assert np.array_equal(Mr, Mr.T)
    dM = rb.operator_bound(pos, box, xi, rcut)
    e = np.linalg.norm(Mr - M, 2)
    assert e <= dM, (name, e, dM)
    psi = np.random.default_rng(len(pos)).normal(size=pos.shape)
    ref, lam = rb.sqrt_apply(M, psi)
    got, _ = rb.sqrt_apply(Mr, psi)
    bound = rb.sqrt_bound(dM, lam) * np.linalg.norm(psi)
    assert np.linalg.norm(got - ref) <= bound, (name, np.linalg.norm(got - ref), bound)
    # the truth() helper the GPU tests use gives the same reference and bound
    t = rb.truth(oracle, pos, box, xi, rcut, psi)
    assert np.array_equal(t["ref"], ref) and t["abs"] == bound


def test_vector_row_term_is_negligible(oracle):
    """The vector-row term is negligible next to the records (it may be added, it decides nothing)."""
    pos, _, box = make_suspension(60, L=14.0, seed=1)
    rcut = RCUT3 / 0.5
    a = rb.operator_bound(pos, box, 0.5, rcut)
    b = rb.operator_bound(pos, box, 0.5, rcut, vector_rows=True)
    assert 0.0 < b - a < 1e-4 * a


def test_f_stays_inside_the_fixed_point_range(oracle):
    """fr is a signed 26-bit integer in units of 2^-24: |f| < 2 or it saturates silently, in the device and the restatement alike.
    f(r) of the real-space part is largest at r = 0, where it equals the self term (< 1 for every xi); checked over r in [0, rcut]
    and xi from 1e-3 (f -> RPY's 1 - 9 r / 32) to 30 (beyond the grids of the rule for any box that holds 2 rcut), at four errors."""
    for err in (1e-3, 1e-6, 1e-9, 1e-12):
        s = math.sqrt(-math.log(err))
        for xi in np.geomspace(1e-3, 30.0, 25):
            rcut = s / xi
            r = np.concatenate([[1e-12], np.geomspace(1e-6, 2.0, 60), np.linspace(2.0, rcut, 120)]) if rcut > 2 else \
                np.concatenate([[1e-12], np.geomspace(1e-6, rcut, 120)])
            f, _ = oracle.fg_real(r, xi)
            assert np.all(np.isfinite(f)) and np.abs(f).max() < 1.0 + 1e-12, (err, xi, np.abs(f).max())
            assert abs(oracle.self_mobility(xi)) < 1.0


# Where the bound on ||M_r^{1/2} psi - M^{1/2} psi|| / ||M^{1/2} psi|| is above 1e-6 (values computed here; the device's measured error
# at the same placements is in tests/test_gpu_lanczos_truth.py).  Two causes: a nearly singular M (two particles 1e-3 apart: lmin =
# 1.9e-4, and the square root amplifies by 1 / (2 sqrt lmin)), and rows with tens of neighbours, where the row sum of 2^-25 per pair
# (fr, the fixed point of f) adds up -- the worst case of every rounding aligned, which Gershgorin cannot rule out.
ABOVE_FLOOR = {
    "c: overlapping, r = 1e-3 .. 2": 1.28e-5,
    "e: tilted image xy = +0.5": 2.70e-6,
    "e: suspension, box 15 x 12 x 13, xy = +0.5": 2.95e-6,
    "f: xi = 0.2": 1.58e-6,
    "f: xi = 0.5": 2.65e-6,
    "f: xi = 1.0": 1.12e-6,
    "f: xi = 10 (overlapping pairs)": 1.76e-6,     # (1.73e-6 with the table at 6e-13; at xi = 10 it is 3 format_eps = 6.2e-10)
}


@pytest.mark.parametrize("name", [pytest.param(g["name"], marks=pytest.mark.xfail(
    strict=True, reason=f"the record bound is {ABOVE_FLOOR[g['name']]:.3g} relative here (> 1e-6)")) if g["name"] in ABOVE_FLOOR
    else g["name"] for g in rb.geometries()])
def test_record_bound_floor(oracle, name):
    """The bound the GPU truth tests hold the device to is <= 1e-6 of |M^{1/2} psi| (psi of the GPU test)."""
    assert _relative_bound(oracle, name) <= 1e-6, name


def _relative_bound(oracle, name):
    g = {x["name"]: x for x in rb.geometries()}[name]
    psi = np.random.default_rng(len(g["pos"])).normal(size=g["pos"].shape)
    return rb.truth(oracle, g["pos"], g["box"], g["xi"], g["rcut"], psi, extra_pair=rb.table(g["xi"], g["rcut"]), vector_rows=True)["rel"]


@pytest.mark.parametrize("name", list(ABOVE_FLOOR))
def test_record_bound_above_the_floor_is_what_is_recorded(oracle, name):
    """The values ABOVE_FLOOR records (and the xfails above state) are pinned here, outside any xfail: a bound that drifted would
    fail this test instead of hiding behind the expected failure."""
    assert _relative_bound(oracle, name) == pytest.approx(ABOVE_FLOOR[name], rel=0.01), name
