"""CPU tests of tests/farfield_ref.py: the planted inputs are what they claim to be, and the extended-precision reference agrees with
the float64 restatement of the reference algorithm (oracle.pse_port.spread / gather) node by node and particle by particle.

Bound: 1e-13 of the sum of the absolute terms.  Both sides evaluate the same formula; the float64 side rounds s = f N (2^-53 N
relative to a grid unit, a relative change of the outermost weights of 2 expfac r h 1e-14 ~ 1e-13 at P = 14), exp (1 ulp) and
each product; measured 4.6e-14 (spread) and 7.1e-15 (gather) over these cases."""
import numpy as np
import pytest

import farfield_ref as fr

# (P, grid, xy, sparse): from the smallest support on the smallest grid to the largest, both signs of the tilt, odd and even P
CASES = [(4, fr.matrix_grid(4), -0.5, False), (5, fr.matrix_grid(5), 0.3, True), (7, fr.matrix_grid(7), 0.0, False),
         (8, fr.matrix_grid(8), 0.4, True), (13, fr.matrix_grid(13), -0.3, False), (14, (28, 28, 28), 0.5, False)]
IDS = [f"P{c[0]}-{'x'.join(map(str, c[1]))}-xy{c[2]}{'-sparse' if c[3] else ''}" for c in CASES]


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request, oracle):
    P, grid, xy, sparse = request.param
    pos, force, box, parts = fr.make_case(P, grid, xy, seed=100 + P, sparse=sparse)
    box2, p = fr.case_params(oracle, P, grid, xy)
    assert box2 == box
    return dict(P=P, grid=grid, xy=xy, sparse=sparse, pos=pos, force=force, box=box, parts=parts, p=p)


def test_size_and_forces(case):
    n = len(case["pos"])
    assert 500 <= n <= 1500, n
    assert 280 <= len(case["parts"]["planted"]) <= 600
    assert (len(case["parts"]["filler"]) == 0) == case["sparse"]
    f = case["force"]
    assert (f > 0).any(axis=0).all() and (f < 0).any(axis=0).all()


def test_clearance(case):
    """No coordinate within 1e-8 grid units of a node (odd P: or a half-node), yet the planted ones within 1.1e-7 of one."""
    c = fr.clearance(case["pos"], case["box"], case["grid"], case["P"])
    assert c.min() >= fr.CLEAR, float(c.min())
    s = fr.scaled(case["pos"][case["parts"]["planted"]], case["box"], case["grid"])
    near = np.abs(2 * s - np.rint(2 * s)).min(axis=1) / 2          # distance to the nearest node or half-node
    assert near.max() <= 1.1 * fr.PLANT and near.min() >= 0.9 * fr.PLANT, (float(near.min()), float(near.max()))


def test_planted_on_both_sides_of_every_target(case):
    s = fr.scaled(case["pos"][case["parts"]["planted"]], case["box"], case["grid"])
    for a in range(3):
        n = case["grid"][a]
        for t in (0.0, 0.5, 8.0, 8.5, n - 0.5):       # the face (0 = n), the first half-node, a bin boundary, the last half-node
            d = s[:, a] - t
            d -= n * np.rint(d / n)
            hit = np.abs(np.abs(d) - fr.PLANT) < 0.1 * fr.PLANT
            assert (hit & (d > 0)).any() and (hit & (d < 0)).any(), (a, t)


def test_faces_are_straddled_on_every_axis(case):
    """Supports that start below a face and end above it, on every axis (the wrap of the tile kernels and the wrapped region of the
    gather)."""
    st = fr.support_starts(fr.scaled(case["pos"], case["box"], case["grid"]), case["P"])
    for a in range(3):
        o = np.mod(st[:, a], case["grid"][a])
        assert (o + case["P"] - 1 >= case["grid"][a]).sum() >= 10, a


def test_clump_fills_one_bin_next_to_empty_ones(case):
    b = fr.origin_bins(case["pos"], case["box"], case["grid"], case["P"])
    cb = fr.clump_bin(case["grid"])
    in_clump = (b == np.array(cb)[None, :]).all(axis=1)
    assert in_clump.sum() >= 300 and set(np.flatnonzero(in_clump)) == set(case["parts"]["clump"])
    for nb in fr.clump_neighbours(case["grid"]):
        assert nb != cb and not (b == np.array(nb)[None, :]).all(axis=1).any(), nb


def test_reference_matches_float64_port(case, oracle):
    pos, force, box, p = case["pos"], case["force"], case["box"], case["p"]
    ref, mag = fr.spread_ref(pos, force, box, p)
    port = np.asarray(oracle.spread(pos, force, box, p))
    untouched = mag == 0
    assert (port[untouched] == 0.0).all() and (ref[untouched] == 0).all()
    if case["sparse"]:
        assert untouched.mean() > 0.25, untouched.mean()      # most of what lies between the three bars and the clump
    r_spread = fr.worst_ratio(port, ref, mag, 1e-13)
    grid_values = np.random.default_rng(7).normal(size=ref.shape)
    u, umag = fr.gather_ref(grid_values, pos, box, p)
    r_gather = fr.worst_ratio(oracle.gather(grid_values, pos, box, p), u, umag, 1e-13)
    print(f"float64 port against the extended reference, in units of 1e-13 sum|terms|: spread {r_spread:.3f}, gather {r_gather:.3f}")
    assert r_spread <= 1.0 and r_gather <= 1.0, (r_spread, r_gather)
    assert (umag > 0).all()


def test_exact_node_is_the_trap():
    """Why nothing is planted ON a node: clearance reports 0 there (the tests' assertion would fail), 1e-7 away it is 1e-7."""
    grid, box = (16, 16, 16), (12.0, 12.0, 12.0, 0.0)
    on = fr._to_pos(np.array([[3.0, 5.25, 7.5]]), box, grid)
    assert fr.clearance(on, box, grid, 4)[0] == 0 and fr.clearance(on, box, grid, 5)[0] == 0
    off = fr._to_pos(np.array([[3.0 + fr.PLANT, 5.25, 7.5 - fr.PLANT]]), box, grid)
    assert abs(float(fr.clearance(off, box, grid, 5)[0]) - fr.PLANT) < 1e-12
