"""CPU tests of the O(N^2) reference the pair observables are compared with on the GPU (tests/pair_virial_ref.py): its pair sum gives
the forces of oracle.pair_repulsion, and its sign convention is the physical one -- under an affine shear strain of box and
positions together dU/d(strain) = -Wxy, so that sigma_xy = -Wxy / V is the stress."""
import numpy as np
import pytest

from pair_virial_ref import pair_observables, pair_terms, random_points

K, SIGMA = 40.0, 2.0
BOX = (14.0, 11.0, 17.0)


@pytest.mark.parametrize("xy", [0.0, 0.3, -0.5])
def test_reference_force_sum_matches_the_port(oracle, xy):
    box = BOX + (xy,)
    pos = random_points(300, box, seed=11)
    obs, F = pair_observables(pos, box, K, SIGMA, oracle)
    ref = oracle.pair_repulsion(pos, box, K, SIGMA)
    assert obs[7] > 20 and obs[0] > 0.0
    assert np.abs(F - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max()), np.abs(F - ref).max()
    assert np.abs(F.sum(axis=0)).max() <= 1e-12 * np.abs(ref).max()          # Newton's third law: the pair sum is antisymmetric
    # the trace of the virial of a central force: sum c r^2 = sum k (sigma - r) r
    i, j, d, c, r = pair_terms(pos, box, K, SIGMA, oracle)
    assert abs(obs[1] + obs[4] + obs[6] - (K * (SIGMA - r) * r).sum()) <= 1e-12 * obs[0]


def test_reference_sign_convention_by_affine_strain(oracle):
    """(U(+delta) - U(-delta)) / (2 delta) = -Wxy for the strain x -> x + delta y, xy -> xy + delta.  The potential is C^1 with
    curvature bounded by k, so the central difference is off by O(delta^2) sum |terms| (pairs that cross r = sigma inside +-delta
    add the same order): ~1e-8 sum |c d_x d_y| at delta = 1e-4; asserted at 1e-6 max(1, sum |c d_x d_y|)."""
    delta = 1e-4
    box = BOX + (0.3,)
    pos = random_points(300, box, seed=11)
    obs, _ = pair_observables(pos, box, K, SIGMA, oracle)
    i, j, d, c, r = pair_terms(pos, box, K, SIGMA, oracle)
    scale = np.abs(c * d[:, 0] * d[:, 1]).sum()
    assert abs(obs[2]) > 1e-3 * scale            # a Wxy that the check can see

    def energy(e):
        p = pos.copy()
        p[:, 0] += e * p[:, 1]
        return pair_observables(p, BOX + (0.3 + e,), K, SIGMA, oracle)[0][0]

    slope = (energy(delta) - energy(-delta)) / (2.0 * delta)
    err = abs(slope + obs[2])
    print(f"dU/dstrain = {slope:.12g}, -Wxy = {-obs[2]:.12g}, |difference| = {err:.3e}, sum|c dx dy| = {scale:.6g}, ratio = {err / max(1.0, scale):.3e}")
    assert err <= 1e-6 * max(1.0, scale), (slope, -obs[2], err, scale)
