"""CPU checks of the configurations of tests/cell_grid_cases.py: whatever tests/test_gpu_cell_grids.py relies on being in a case is
shown to be there with the references alone -- the class of every axis of both cell grids, the planted pairs on their side of their
cutoffs, a reference pair for every wrap combination of the cell walk and across every z block boundary, non-zero reference
results.  A planted structure that went missing fails here, not on the GPU."""
import itertools

import numpy as np
import pytest

import cell_grid_cases as cg
import pair_table_ref
import pair_virial_ref

EXPECTED = {   # name: (cells with the kept list, cells without)
    "blocked_padded": ((6, 4, 13, 6), (6, 4, 14, 6)),
    "blocked_exact": ((6, 4, 12, 6), (6, 4, 12, 6)),
    "blocked_tilt_pos": ((6, 4, 13, 6), (6, 4, 14, 6)),
    "blocked_tilt_neg": ((6, 4, 13, 6), (6, 4, 14, 6)),
    "one_cell_x": ((1, 5, 13, 6), (1, 5, 14, 6)),
    "three_cubed": ((3, 3, 3, 3), (3, 3, 3, 3)),
    "global_table": ((3, 3, 12, 6), (3, 3, 12, 6)),
}
MORSE = dict(D=5.0, alpha=2.0, r0=1.5)      # as tests/test_gpu_pair_table.py


@pytest.fixture(scope="module")
def port():
    from oracle import pse_port
    return pse_port


@pytest.fixture(scope="module", params=cg.NAMES)
def case(request, port):
    return cg.build(request.param, port)


def test_the_geometries_are_the_seven(port):
    assert set(cg.NAMES) == set(EXPECTED)
    counts = [cg.build(name, port)["n"] for name in cg.NAMES]
    assert max(counts) <= 2000
    assert any(n % 64 == 1 for n in counts) and any(n % 256 == 0 for n in counts)


def test_cell_classes(case):
    wide, narrow = case["cells_wide"], case["cells_narrow"]
    assert (wide, narrow) == EXPECTED[case["name"]]
    for a in range(3):
        assert cg.cell_class(wide[a]) == cg.cell_class(narrow[a]), (case["name"], "xyz"[a], wide, narrow)
    if case["name"] == "global_table":
        assert case["skin"] == 0.0 and not cg.table_in_lds(case["rcut"]) and wide == narrow
    else:
        assert case["skin"] == cg.SKIN and cg.table_in_lds(case["rcut"])
    # the cutoff fits the minimum image, and the cells are no narrower than what they serve
    w = cg.widths(case["box"])
    assert case["rcut"] + case["skin"] <= 0.5 * min(w)
    for grid, r in ((wide, case["rcut"] + case["skin"]), (narrow, case["rcut"])):
        assert all(grid[a] == 1 or w[a] / grid[a] >= r for a in range(3))


def test_positions_are_inside_the_box(case, port):
    pos, box = case["pos"], case["box"]
    f = cg.fractional(pos, box)
    assert f.min() >= -0.5 and f.max() < 0.5
    wrapped, image = port.wrap(pos, np.zeros((case["n"], 3), dtype=np.int64), box)
    assert np.array_equal(wrapped, pos) and not image.any()
    assert pos.shape == case["force"].shape == case["psi"].shape == (case["n"], 3)
    assert not any(a.flags.writeable for a in (pos, case["force"], case["psi"]))


def test_cutoff_conditions(case, port):
    assert cg.cutoff_problems(case, port) == []
    planted = case["planted"]
    if min(case["cells_wide"][:3]) == 1:
        assert not planted and not case["crossers"]
        return
    names = ("rcut", "rmax", "sigma", "rmin") if case["pair"] else ("rcut",)
    pos, box = case["pos"], case["box"]
    for cname in names:
        rows = [p for p in planted if p[2] == cname]
        inside = [p for p in rows if p[3]]
        assert len(inside) == len(rows) - len(inside) == (cg.N_SITES if cname == "rcut" else cg.pair_sites(case["n"]))
        # half of the kept pairs go through a face of the box: the shifted coordinate of the scan is the largest there is
        through = 0
        for i, j, _, _, straddle in inside:
            d = pos[i] - pos[j]
            crossed = not np.allclose(port.min_image(d, box), d, rtol=0.0, atol=1e-9)
            assert crossed == straddle or cname != "rcut"
            through += crossed
        if cname == "rcut":
            assert through == cg.N_SITES // 2
    # the sites carry the largest coordinates: within 0.02 of a face, every axis and both signs among them
    f = cg.fractional(pos[sorted({p[0] for p in planted})], box)
    near = np.abs(np.abs(f) - 0.5) <= 0.02
    assert near.any(axis=1).all()
    for a in range(3):
        assert (near[:, a] & (f[:, a] > 0)).any() and (near[:, a] & (f[:, a] < 0)).any()
    for i, j, label in case["crossers"]:
        d = port.min_image(pos[i] - pos[j], box)
        assert abs(np.linalg.norm(d) - 2.05) < 1e-12, label
    assert len([c for c in case["crossers"] if c[2][0] == "w"]) == 13


def test_every_wrap_combination_and_block_boundary_has_a_pair(case, port):
    pos, box, rcut = case["pos"], case["box"], case["rcut"]
    i, j, _, r = cg.pair_distances(pos, box, port)
    for grid, reach in {(case["cells_wide"], rcut + case["skin"]), (case["cells_narrow"], rcut)}:
        c = cg.cell_coords(pos, box, grid)
        m = r < reach
        o, w = cg.walk_codes(c[i[m]], c[j[m]], grid)
        assert (o != 2).all(), (case["name"], grid, "a pair within reach lies in no neighbour cell")
        m = r < rcut
        o, w = cg.walk_codes(c[i[m]], c[j[m]], grid)
        _, w_back = cg.walk_codes(c[j[m]], c[i[m]], grid)
        assert np.array_equal(w_back, -w)
        seen = {tuple(t) for t in w} | {tuple(t) for t in w_back}
        want = set(itertools.product(*[(-1, 0, 1) if grid[a] > 1 else (0,) for a in range(3)]))
        assert seen == want, (case["name"], grid, sorted(want - seen))
        cz_i, cz_j = c[i[m], 2], c[j[m], 2]
        for lo, hi in cg.block_boundaries(grid):
            across = ((cz_i == lo) & (cz_j == hi)) | ((cz_i == hi) & (cz_j == lo))
            assert across.sum() >= 1, (case["name"], grid, lo, hi)
        # a tilted box at the limit: pairs through the y face whose x cells differ as well
        if abs(box[3]) == 0.5:
            assert ((w[:, 1] != 0) & (o[:, 0] != 0)).any()
    for a, b, label in case["crossers"]:
        for grid in {case["cells_wide"], case["cells_narrow"]}:
            c = cg.cell_coords(pos[[a, b]], box, grid)
            o, w = cg.walk_codes(c[0], c[1], grid)
            if label[0] == "cz":
                lo, hi, nz = label[1:]
                assert grid[2] != nz or (c[0, 2], c[1, 2]) == (lo, hi), label
            else:
                assert tuple(w) == label[1:], (label, grid, c)        # the walk of a finds b in the image the label names


def test_the_scan_needs_its_slack(case):
    """The single-precision scan of the cell pass, restated (cg.scan_r2): with the radius the launch gives it, it keeps every planted
    pair that lies inside rcut; with the slack for the rounding of the coordinates taken out of that radius, it would drop some of
    them wherever the box is long enough for the rounding to show -- an M_real F without those pairs misses the bound of
    tests/test_gpu_cell_grids.py by eight orders.  So these inputs tell whether the slack is there."""
    inside = [(i, j) for i, j, cname, ins, _ in case["planted"] if cname == "rcut" and ins]
    if not inside:
        return
    pos, box, rcut = case["pos"], case["box"], case["rcut"]
    a, b = (np.array(t) for t in zip(*inside))
    for grid in {case["cells_wide"], case["cells_narrow"]}:
        seen = np.maximum(cg.scan_r2(pos[a], pos[b], box, grid), cg.scan_r2(pos[b], pos[a], box, grid))
        kept, bare = cg.prefilter(box, rcut), cg.prefilter(box, rcut, slack=False)
        excess = seen.max() / bare - 1.0
        print(f"{case['name']} {grid}: largest single-precision r^2 of a pair inside rcut: {seen.max() / rcut ** 2 - 1.0:+.3e} of rcut^2; "
              f"radius^2 of the scan {kept / rcut ** 2 - 1.0:+.3e}, without the slack {bare / rcut ** 2 - 1.0:+.3e}")
        assert (seen < kept * (1.0 - 1e-6)).all()
        if box[2] >= 68.0:
            # beyond the bare radius by more than the two ulps of a float that the order of the device's sum could move it
            assert (seen > bare * (1.0 + 2.4e-7)).sum() >= 3, (case["name"], grid, excess)


def test_every_row_fits_the_kept_list(case, port):
    """A row beyond the capacity marks the kept list as overflowed: it is built again at every call and the pass that reads it never
    runs.  Counted within rcut + skin + 0.2: the GPU test moves every particle by less than 0.1 before the call that reuses the list."""
    if case["skin"] == 0.0:
        return
    i, j, _, r = cg.pair_distances(case["pos"], case["box"], port)
    m = r < case["rcut"] + case["skin"] + 0.2
    count = np.bincount(i[m], minlength=case["n"]) + np.bincount(j[m], minlength=case["n"])
    cap = cg.kept_list_capacity(case["n"], case["box"], case["rcut"], case["skin"])
    print(f"{case['name']}: at most {count.max()} neighbours within rcut + skin + 0.2, capacity {cap}")
    assert count.max() <= cap, (case["name"], int(count.max()), cap)


def test_reference_results_are_not_trivial(case, port):
    pos, box, rcut = case["pos"], case["box"], case["rcut"]
    u = port.mobility_real(pos, case["force"], box, case["xi"], rcut)
    self_only = port.self_mobility(case["xi"]) * case["force"]
    assert np.isfinite(u).all() and np.abs(u - self_only).max() > 1e-3 * np.abs(u).max()
    ur = port.mobility_real(pos, case["force"], box, case["xi"], rcut, rounded=True)
    assert 0.0 < np.abs(ur - u).max() < 1e-5 * np.abs(u).max()          # the rounded operator is another one, and close
    if not case["pair"]:
        return
    obs, F = pair_virial_ref.pair_observables(pos, box, 40.0, cg.SIGMA, port)
    assert obs[7] > 20 and obs.all() and np.abs(F).max() > 1.0
    for rmin, rmax, width in ((cg.RMIN, cg.RMAX, 1000), (0.0, rcut, 1000)):
        table = pair_table_ref.morse_table(rmin=rmin, rmax=rmax, width=width, **MORSE)
        assert (table[:, 1] > 0).any() and (table[:, 1] < 0).any()            # a sign error in F or W cannot cancel
        obs, F = pair_table_ref.pair_observables(pos, box, table, rmin, rmax, port)
        assert obs[7] > 20 and obs.all() and np.abs(F).max() > 1.0
        i, j, _, r = cg.pair_distances(pos, box, port)
        assert obs[7] == ((r >= rmin) & (r < rmax) & (r > 0)).sum()
