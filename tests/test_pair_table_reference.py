"""CPU tests of the O(N^2) reference the tabulated pair potential is compared with on the GPU (tests/pair_table_ref.py): a linear
table is reproduced to round-off at every width, the harmonic table gives the forces and the virial of the harmonic reference
(tests/pair_virial_ref.py) and its energy within the linear-interpolation bound, the pair sum is antisymmetric and the virial symmetric,
and pairs below rmin contribute nothing."""
import numpy as np
import pytest

import pair_virial_ref
from pair_table_ref import harmonic_table, interpolate, pair_observables, pair_terms, random_points, sample

N = 600
BOX = (12.0, 12.0, 12.0, 0.0)
RMAX = 2.0
K = 40.0


def points():
    return random_points(N, BOX, seed=11)


@pytest.mark.parametrize("width", [2, 3, 1025, 2048])
@pytest.mark.parametrize("rmin", [0.0, 0.7])
def test_linear_table_is_reproduced_to_roundoff(oracle, width, rmin):
    a, b, c, e = 1.5, -0.8, 3.0, -1.25                      # V = a + b r, F = c + e r: the interpolant of a linear function is itself
    table = sample(lambda r: a + b * r, lambda r: c + e * r, rmin, RMAX, width)
    assert table.shape == (width, 2)
    i, j, d, r, V, F = pair_terms(points(), BOX, table, rmin, RMAX, oracle)
    assert len(r) > 1000 and r.min() >= rmin and r.max() < RMAX
    Vx, Fx = a + b * r, c + e * r
    errV, errF = np.abs(V - Vx).max(), np.abs(F - Fx).max()
    print(f"width {width}, rmin {rmin}: {len(r)} pairs, max |V - exact| = {errV:.3e}, max |F - exact| = {errF:.3e}")
    assert errV <= 1e-13 * np.abs(Vx).max() and errF <= 1e-13 * np.abs(Fx).max()
    # the ends of the table: the first node, and the clamp of the index just below rmax
    ends = np.array([rmin, np.nextafter(RMAX, 0.0)])
    Ve, Fe = interpolate(table, rmin, RMAX, ends)
    assert np.abs(Ve - (a + b * ends)).max() <= 1e-13 * np.abs(Vx).max() and np.abs(Fe - (c + e * ends)).max() <= 1e-13 * np.abs(Fx).max()


@pytest.mark.parametrize("width", [2, 3, 1025, 2048])
def test_harmonic_table_against_the_harmonic_reference(oracle, width):
    pos = points()
    table = harmonic_table(K, RMAX, width)
    obs, F = pair_observables(pos, BOX, table, 0.0, RMAX, oracle)
    ref, Fref = pair_virial_ref.pair_observables(pos, BOX, K, RMAX, oracle)
    assert obs[7] == ref[7] > 1000
    # F(r) = k (rmax - r) is linear: forces and virial are those of the closed form
    assert np.abs(F - Fref).max() <= 1e-12 * np.abs(Fref).max()
    assert np.abs(obs[1:7] - ref[1:7]).max() <= 1e-12 * np.abs(ref[1:7]).max()
    # V is a parabola of curvature k: the chord lies above it by at most k dr^2 / 8, per pair
    dr = RMAX / (width - 1)
    bound = ref[7] * K * dr * dr / 8.0
    print(f"width {width}: U_table - U_exact = {obs[0] - ref[0]:.6e}, bound {bound:.6e}")
    assert abs(obs[0] - ref[0]) <= bound
    assert obs[0] >= ref[0] * (1.0 - 1e-14)                 # (the chord of a convex function is never below it)


@pytest.mark.parametrize("xy", [0.0, 0.3])
def test_pair_sum_is_antisymmetric_and_virial_symmetric(oracle, xy):
    box = (14.0, 11.0, 17.0, xy)
    pos = random_points(N, box, seed=5)
    table = sample(lambda r: np.cos(2.0 * r), lambda r: 2.0 * np.sin(2.0 * r), 0.3, RMAX, 37)     # changes sign inside the range
    obs, F = pair_observables(pos, box, table, 0.3, RMAX, oracle)
    i, j, d, r, V, Fr = pair_terms(pos, box, table, 0.3, RMAX, oracle)
    assert obs[7] == len(r) > 300 and (Fr > 0).any() and (Fr < 0).any()
    scale = np.abs(Fr).sum()
    assert np.abs(F.sum(axis=0)).max() <= 1e-13 * scale
    W = np.einsum("pa,pb->ab", d, (Fr / r)[:, None] * d)    # sum d_a F_b with F = F(r) d / r, all nine components
    assert np.abs(W - W.T).max() <= 1e-13 * np.abs(W).max()
    six = np.array([W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2]])
    assert np.abs(six - obs[1:7]).max() <= 1e-12 * np.abs(six).max()
    assert abs(V.sum() - obs[0]) <= 1e-12 * np.abs(V).sum()


def test_pairs_below_rmin_contribute_nothing(oracle):
    """Against the full N x N matrix of separations (not the list of pairs i < j the reference walks): only rmin <= r < rmax acts,
    and the check could tell -- the same sum with the pairs below rmin let in is far outside the tolerance."""
    rmin = 0.7
    a, b, c, e = 1.5, -0.8, 3.0, -1.25
    pos = points()
    table = sample(lambda r: a + b * r, lambda r: c + e * r, rmin, RMAX, 64)
    obs, F = pair_observables(pos, BOX, table, rmin, RMAX, oracle)
    d = oracle.min_image((pos[:, None, :] - pos[None, :, :]).reshape(-1, 3), BOX).reshape(N, N, 3)
    r = np.sqrt((d * d).sum(axis=2))
    np.fill_diagonal(r, 1e30)
    below, inside = r < rmin, (r >= rmin) & (r < RMAX)
    assert below.sum() // 2 >= 1, "the configuration must have pairs below rmin"
    print(f"{below.sum() // 2} pairs below rmin, {inside.sum() // 2} inside")
    assert obs[7] == inside.sum() // 2 == (r < RMAX).sum() // 2 - below.sum() // 2

    def forces(mask):
        c_ij = np.where(mask, (c + e * r) / r, 0.0)
        return (c_ij[:, :, None] * d).sum(axis=1)

    Fin = forces(inside)
    tol = 1e-12 * np.abs(Fin).max()
    assert np.abs(F - Fin).max() <= tol
    assert np.abs(forces(inside | below) - F).max() > 1e6 * tol
    assert abs(obs[0] - 0.5 * np.where(inside, a + b * r, 0.0).sum()) <= 1e-12 * abs(obs[0])
