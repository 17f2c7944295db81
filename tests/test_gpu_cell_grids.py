"""The cell-list passes on grids of many cells against the direct sums: the near-field kernels (k_mreal_cells in its instantiations,
k_mreal_verlet, k_mreal_list) and the pair-force kernels (k_pair_repulsion, k_pair_table) on the configurations of
tests/cell_grid_cases.py -- z blocks of six cells with a padded or a full last block, the box tilted to the limit the cells are sized
for, one cell along x, three cells along every axis, the f, g table read from global memory -- each with pairs planted through every
face, edge and corner of the box, across every z block boundary, and 1e-9 (relative) inside and outside every cutoff.
tests/test_cell_grid_cases_cpu.py shows on the CPU that the planted structures are there.

Bounds: the project's own, from the tests named at each assertion.  The figures in the comments are the largest seen on an MI355X."""
import functools

import numpy as np
import pytest

from conftest import to4
import cell_grid_cases as cg
import pair_table_ref
import pair_virial_ref
from test_gpu_pair_table import MORSE, check_forces, check_obs, dev

pytestmark = pytest.mark.gpu

NAMES = cg.NAMES
PAIR_NAMES = tuple(n for n in NAMES if cg.SPECS[n][1] == 0.5)
K = 40.0
SEED = 77


def port():
    from oracle import pse_port
    pse_port.lib()
    return pse_port


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def case(name):
    return cg.build(name, port())


def new_engine(name, **kw):
    import pse_amd
    c = case(name)
    eng = pse_amd.Engine(c["n"], c["box"], xi=c["xi"], error=c["error"], max_strain=c["max_strain"], seed=SEED, **kw)
    info = eng.info()
    assert abs(info["rcut"] - c["rcut"]) <= 1e-15 * c["rcut"]
    assert grid_of(eng) == c["cells_wide"][:3]                 # a new handle sizes its cells for the list it keeps
    assert eng.neighbor_stats()[0] == c["skin"]
    return eng


@functools.lru_cache(maxsize=None)
def engine(name):
    """The engine the pair passes and the Brownian calls of a case share."""
    return new_engine(name)


def grid_of(eng):
    i = eng.info()
    return (i["ncell_x"], i["ncell_y"], i["ncell_z"])


def use_grid(eng, c, which):
    """Cells as wide as rcut + skin ("wide": the handle keeps a neighbour list) or as rcut ("narrow": it does not)."""
    eng.set_neighbor_skin(c["skin"] if which == "wide" else 0.0)


def where(c, row):
    return {"row": int(row), "cell (wide)": tuple(int(t) for t in cg.cell_coords(c["pos"][[row]], c["box"], c["cells_wide"])[0]),
            "cell (narrow)": tuple(int(t) for t in cg.cell_coords(c["pos"][[row]], c["box"], c["cells_narrow"])[0])}


def check_mreal(c, u, ref, what):
    """Norm-relative < 1e-12 (tests/test_gpu_parity.py test_mreal_matches_oracle), and no row further from its reference
    than 1e-12 of the largest row."""
    err = np.linalg.norm(u - ref, axis=1)
    worst = int(err.argmax())
    scale = np.linalg.norm(ref, axis=1).max()
    print(f"{c['name']} {what}: rel {rel(u, ref):.3e}, worst row {err[worst] / scale:.3e} of the largest row, {where(c, worst)}", flush=True)
    assert rel(u, ref) < 1e-12, (c["name"], what, rel(u, ref))                         # MI355X: <= 1.5e-15 (all passes, all seven cases)
    assert err[worst] < 1e-12 * scale, (c["name"], what, err[worst] / scale, where(c, worst))   # MI355X: <= 7.7e-15


@pytest.mark.parametrize("name", NAMES)
def test_mreal_on_every_pass(name):
    """M_real F three ways: the cell pass of a new handle, which also writes the kept neighbour list; the pass that reads that list,
    after every particle has moved by less than 0.1; the cell pass on packed records once the skin is off (cells as wide as rcut).
    global_table keeps no list (its table does not fit the LDS): its one pass reads f, g from global memory."""
    c = case(name)
    oracle = port()
    eng = new_engine(name)
    pos, force, box = c["pos"], c["force"], c["box"]
    if name == "global_table":
        # table before walk: f, g at the bound of test_realspace_functions_match_closed_form
        r = np.concatenate([np.random.default_rng(1).uniform(1e-3, c["rcut"], 2000), [2.0, 1.999999, 2.000001, 0.125, c["rcut"] * (1 - 1e-9)]])
        f, g = eng.eval_realspace(r)
        fo, go = oracle.fg_real(r, c["xi"])
        print(f"global_table: max |f - f_ref| = {np.abs(f - fo).max():.3e}, max |g - g_ref| = {np.abs(g - go).max():.3e}", flush=True)
        # 2e-13: the table's contract for xi <= XI_TABLE = 4 (tests/test_realspace_table_cpu.py: the format allows it there, no further)
        assert np.abs(f - fo).max() < 2e-13 and np.abs(g - go).max() < 2e-13                     # MI355X: 1.2e-16, 1.7e-16
    ref = oracle.mobility_real(pos, force, box, c["xi"], c["rcut"], rounded=False)
    _, b0, r0 = eng.neighbor_stats()
    u = eng.mobility(to4(pos), to4(force), parts=1).cpu().numpy()[:, :3]
    _, b1, r1 = eng.neighbor_stats()
    assert (b1, r1) == (b0 + 1, r0)
    check_mreal(c, u, ref, "(a) cell pass" + (" + kept list" if c["skin"] else ", table in global memory"))
    if c["skin"] == 0.0:
        assert grid_of(eng) == c["cells_narrow"][:3]
        eng.close()
        return
    assert grid_of(eng) == c["cells_wide"][:3]
    step = np.random.default_rng(3).uniform(-0.05, 0.05, size=pos.shape)                     # |step| <= 0.087
    moved = oracle.wrap(pos + step, np.zeros(pos.shape, dtype=np.int64), box)[0]
    ref_moved = oracle.mobility_real(moved, force, box, c["xi"], c["rcut"], rounded=False)
    u = eng.mobility(to4(moved), to4(force), parts=1).cpu().numpy()[:, :3]
    _, b2, r2 = eng.neighbor_stats()
    assert (b2, r2) == (b1, r1 + 1), ("the kept list was not reused", b1, r1, b2, r2)
    check_mreal(c, u, ref_moved, "(b) kept list")
    eng.set_neighbor_skin(0.0)
    u = eng.mobility(to4(pos), to4(force), parts=1).cpu().numpy()[:, :3]
    assert grid_of(eng) == c["cells_narrow"][:3]
    assert eng.neighbor_stats()[2] == r2
    check_mreal(c, u, ref, "(c) skin 0, packed records")
    eng.close()


@functools.lru_cache(maxsize=None)
def sqrt_reference(name, rounded):
    c = case(name)
    oracle = port()
    mv = lambda v: oracle.mobility_real(c["pos"], np.ascontiguousarray(v), c["box"], c["xi"], c["rcut"], rounded=rounded)   # noqa: E731
    out, m = oracle.lanczos_sqrt(mv, c["psi"], 2, 1e-3)
    out.setflags(write=False)
    return out, m


@pytest.mark.parametrize("operator", ["records16", "fp64"])
@pytest.mark.parametrize("name", NAMES)
def test_sqrt_mreal(name, operator):
    """M_real^{1/2} psi at tol = 1e-3: the default operator against the Lanczos iteration over the rounded sums, the fp64 operator
    against the un-rounded ones (the bounds of tests/test_gpu_lanczos_fp64.py): the same m, relative < 1e-9.  A new handle builds the
    pair list in the cell pass that writes the kept list; the second call builds it from the kept list; the third, skin off, in the
    plain cell pass; every one feeds the pair-list mat-vecs."""
    c = case(name)
    ref, mref = sqrt_reference(name, operator == "records16")
    eng = new_engine(name, lanczos_operator=operator)
    dpos, dpsi = to4(c["pos"]), to4(c["psi"])
    for what in ("new handle", "same inputs again", "skin 0"):
        if what == "skin 0":
            eng.set_neighbor_skin(0.0)
        _, _, r0 = eng.neighbor_stats()
        out, m = eng.sqrt_mreal(dpos, dpsi, tol=1e-3)
        _, _, r1 = eng.neighbor_stats()
        assert r1 - r0 == (1 if what == "same inputs again" and c["skin"] else 0), (what, r0, r1)
        err = rel(out.cpu().numpy()[:, :3], ref)
        print(f"{name} sqrt_mreal {operator}, {what}: m {m} / {mref}, rel {err:.3e}", flush=True)
        assert m == mref, (name, operator, what, m, mref)
        assert err < 1e-9, (name, operator, what, err)                                   # MI355X: records16 <= 5.4e-14, fp64 <= 1.4e-15
    assert grid_of(eng) == c["cells_narrow"][:3]
    eng.close()


@pytest.mark.parametrize("name", ["blocked_padded", "blocked_tilt_neg", "one_cell_x"])
def test_brownian_velocity(name):
    """The whole Brownian velocity against the port with the rounded pair coefficients (tests/test_gpu_random_configs.py): the same
    m, relative < 1e-9.  The near-field pass builds the pair list and carries M psi along; the mat-vecs read the list.  With the skin
    (the pass also writes the kept list) and without (packed records)."""
    c = case(name)
    oracle = port()
    eng = engine(name)
    p = oracle.select_params(c["box"], c["xi"], c["error"], c["max_strain"])
    i = eng.info()
    assert (i["Nx"], i["Ny"], i["Nz"]) == p["grid"] and i["P"] == p["P"]
    kT, dt, ts = 0.7, 2e-3, 11
    ref, mref = oracle.brownian_velocity(c["pos"], c["force"], c["box"], p, kT, dt, SEED, ts, pair_rounded=True)
    for which in ("wide", "narrow"):
        use_grid(eng, c, which)
        eng.pair_repulsion(to4(c["pos"]), to4(np.zeros((c["n"], 3))), K, cg.SIGMA)          # a walk of the caller: the next call sorts and builds anew
        vel, m = eng.brownian_velocity(to4(c["pos"]), to4(c["force"]), kT, dt, ts)
        assert grid_of(eng) == c["cells_" + which][:3]
        err = rel(vel.cpu().numpy()[:, :3], ref)
        print(f"{name} brownian_velocity, {which} cells: m {m} / {mref}, rel {err:.3e}", flush=True)
        assert m == mref, (name, which, m, mref)
        assert err < 1e-9, (name, which, err)                                            # MI355X: <= 2.4e-14
    use_grid(eng, c, "wide")


# -- the pair passes ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_of(name, kind):
    rmin, rmax = (cg.RMIN, cg.RMAX) if kind == "morse" else (0.0, case(name)["rcut"])
    table = pair_table_ref.morse_table(rmin=rmin, rmax=rmax, width=1000, **MORSE)
    table.setflags(write=False)
    return table, rmin, rmax


@functools.lru_cache(maxsize=None)
def pair_reference(name, kind, group=False):
    """(obs, F) of the O(N^2) reference: kind "morse" (the table on [0.7, 3)), "rcut" (the table over the whole range of the cell
    list) or "repulsion"; group: among members(name) only."""
    c = case(name)
    pos = c["pos"][members(name)] if group else c["pos"]
    if kind == "repulsion":
        obs, F = pair_virial_ref.pair_observables(pos, c["box"], K, cg.SIGMA, port())
    else:
        table, rmin, rmax = table_of(name, kind)
        obs, F = pair_table_ref.pair_observables(pos, c["box"], table, rmin, rmax, port())
    for a in (obs, F):
        a.setflags(write=False)
    return obs, F


@functools.lru_cache(maxsize=None)
def members(name):
    n = case(name)["n"]
    m = np.sort(np.random.default_rng(5).choice(n, size=(2 * n) // 3, replace=False)).astype(np.int32)
    m.setflags(write=False)
    return m


def run_pair(eng, kind, name, dpos, force, **kw):
    if kind == "repulsion":
        if kw.pop("observables", True) is False:
            kw.pop("out", None)
            eng.pair_repulsion(dpos, force, K, cg.SIGMA, **kw)
            return None
        return eng.pair_repulsion_virial(dpos, force, K, cg.SIGMA, **kw)
    table, rmin, rmax = table_of(name, kind)
    return eng.pair_table(dpos, force, dev(table), rmin, rmax, **kw)


@pytest.mark.parametrize("which", ["wide", "narrow"])
@pytest.mark.parametrize("kind", ["repulsion", "morse", "rcut"])
@pytest.mark.parametrize("name", PAIR_NAMES)
def test_pair_passes(name, kind, which):
    """pair_repulsion_virial (k = 40, sigma = 2) and pair_table (Morse, width 1000, on [0.7, 3) and on [0, rcut)) in every call form,
    on the cells of a handle that keeps its neighbour list and of one that does not: forces and the eight sums within
    1e-11 max(1, max |ref|), npairs exactly (check_obs, check_forces of tests/test_gpu_pair_table.py)."""
    c = case(name)
    eng = engine(name)
    use_grid(eng, c, which)
    n = c["n"]
    ref, F = pair_reference(name, kind)
    assert ref[7] > 20
    dpos = to4(c["pos"])
    tag = f"{name} {kind} {which}"
    base = np.random.default_rng(5).normal(size=(n, 3))
    # forces and observables, stored
    f = to4(base, 7.0)
    out = run_pair(eng, kind, name, dpos, f, accumulate=False)
    assert grid_of(eng) == c["cells_" + which][:3]
    check_obs(out.cpu().numpy(), ref, tag + " both")                                    # MI355X: <= 5.0e-4 of the bound (all cases, tables, forms)
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, tag + " both")                                            # MI355X: <= 3.2e-3 of the bound
    assert np.all(g[:, 3] == 7.0)
    # observables only
    check_obs(run_pair(eng, kind, name, dpos, None).cpu().numpy(), ref, tag + " force=None")
    # forces only
    f = to4(base, 7.0)
    assert run_pair(eng, kind, name, dpos, f, accumulate=False, observables=False) is None
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, tag + " forces only")
    assert np.all(g[:, 3] == 7.0)
    # added to what the array holds
    f = to4(base, 7.0)
    check_obs(run_pair(eng, kind, name, dpos, f, accumulate=True).cpu().numpy(), ref, tag + " accumulate")
    g = f.cpu().numpy()
    check_forces(g[:, :3] - base, F, tag + " accumulate")
    assert np.all(g[:, 3] == 7.0)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], c["pos"])
    use_grid(eng, c, "wide")


@pytest.mark.parametrize("kind", ["repulsion", "morse", "rcut"])
def test_pair_passes_on_a_group(kind):
    """Two thirds of the particles of the box tilted to +0.5: the members interact among themselves, the rows of the others stay."""
    import torch
    name = "blocked_tilt_pos"
    c = case(name)
    eng = engine(name)
    use_grid(eng, c, "wide")
    mem = members(name)
    ref, F = pair_reference(name, kind, True)
    assert ref[7] > 20
    sentinel = np.random.default_rng(9).normal(size=(c["n"], 3))
    f = to4(sentinel, 7.0)
    group = torch.tensor(mem, dtype=torch.int32, device="cuda")
    out = run_pair(eng, kind, name, to4(c["pos"]), f, group=group, accumulate=False).cpu().numpy()
    check_obs(out, ref, f"{name} {kind} group")
    g = f.cpu().numpy()
    check_forces(g[mem, :3], F, f"{name} {kind} group")
    others = np.setdiff1d(np.arange(c["n"]), mem)
    assert np.array_equal(g[others, :3], sentinel[others]) and np.all(g[:, 3] == 7.0)


@pytest.mark.parametrize("kind", ["repulsion", "morse"])
def test_two_calls_give_the_same_bits(kind):
    """Equal inputs, equal bits: the sums have a fixed order (no floating-point atomics, a stable cell sort), on the blocked order too."""
    name = "blocked_padded"
    c = case(name)
    eng = engine(name)
    use_grid(eng, c, "wide")
    dpos = to4(c["pos"])
    fa, fb = to4(np.zeros((c["n"], 3))), to4(np.zeros((c["n"], 3)))
    a = run_pair(eng, kind, name, dpos, fa, accumulate=False).cpu().numpy()
    eng.mobility(to4(case(name)["pos"][::-1].copy()), to4(c["force"]), parts=1)             # another entry point in between: the next call sorts again
    b = run_pair(eng, kind, name, dpos, fb, accumulate=False).cpu().numpy()
    assert a[7] > 20 and np.array_equal(a, b) and np.array_equal(fa.cpu().numpy(), fb.cpu().numpy())
