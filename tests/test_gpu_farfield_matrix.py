"""The far-field kernels one by one: every instantiation the host can select -- support P = 4 ... 14, with and without shear, the spread
by blocks of 8 x 8 x TZ nodes (TZ = 8 with one or four waves, TZ = 16) and the gather by bins (one or two bins along z), the generic
kernels below the threshold of the block kernels and (the gather) on grids with an odd Nz -- on the smallest grid at which it exists,
with planted inputs (tests/farfield_ref.py), against the extended-precision reference node by node and particle by particle.

What is asserted, per case:
  path    Engine.far_path() -- the host functions that decide the launches -- names the instantiation the case was written for;
  spread  |g - ref| <= TOL sum|terms| at every node of every component, and exactly 0.0 at nodes outside every support, after a call with
          OTHER particles has filled the grids (the block kernels write every node once; there is no zeroing pass);
  gather  Engine.debug_gather on a seeded normal grid: |u - ref| <= TOL sum|terms| per particle and component; on grids that are 1 at one
          node of a planted particle's support (corner, edge, centre) and at one node outside it (P = 4, 7, 8, 13): h^3 w within TOL for
          the particles that reach the node, exactly 0.0 for the others;
  chain   mobility(parts=2) against the float64 restatement of the whole wave part at the suite's 1e-10;
  order   the same particles in another order: the gather is bit-equal (a particle's sum runs over its own support in a fixed order);
          the spread is NOT bit-equal by construction -- the order of the particles inside a bin is the order in which wavefronts of the
          binning pass reach an atomic counter, and ties of the cell sort go by the caller's index -- so it is held to the same bound
          against the reference.
TOL = 1e-12 is the project's figure for the spread (tests/test_gpu_parity.py), applied to every node's own sum of absolute terms and
not to the largest node of the grid: ~20 times what the float64 restatement needs against the same reference
(tests/test_farfield_ref_cpu.py), which leaves room for the Gaussian recurrence of the block kernels (up to 13 multiplications per
axis where the restatement calls exp once)."""
import time

import numpy as np
import pytest

from conftest import to4
import farfield_ref as fr

pytestmark = pytest.mark.gpu
TOL = 1e-12
T0 = []         # when the first test of this module began
SWITCHES = ("PSE_SPREAD_TZ", "PSE_SPREAD_NW", "PSE_GATHER_BZ")
IMPULSE_P = (4, 7, 8, 13)


def _variants(P):
    """(TZ, NW, BZ) of the engines of support P: every spread variant and every gather variant that exists for it at least once."""
    if P <= 7:
        return [(8, 1, 1), (8, 4, 2), (16, 1, 2)]
    if P == 8:
        return [(8, 1, 1), (8, 4, 1), (16, 1, 1)]
    return [(8, 1, 1), (16, 1, 1)]


# (P, grid, xy, (TZ, NW, BZ) forced or None, expected far_path tuple)
CASES = []
for _P in range(4, 15):
    for _xy in (0.0, fr.matrix_xy(_P)):
        for _v in _variants(_P):
            CASES.append((_P, fr.matrix_grid(_P), _xy, _v, (1, _v[0], _v[1], 1, _v[2], int(_xy != 0.0))))
# one node short of the threshold of the block kernels (2 max(8, P) per axis): both kernels generic
CASES.append((5, (36, 15, 40), 0.3, None, (0, 0, 0, 0, 0, 0)))
CASES.append((13, (36, 25, 40), 0.0, None, (0, 0, 0, 0, 0, 0)))
# odd Nz: the spread by blocks (scalar stores of the z rows), the gather generic; the switches left to the rules (60 blocks: four waves)
CASES.append((6, (16, 36, 45), 0.3, None, (1, 8, 4, 0, 0, 1)))
CASES.append((9, (18, 36, 45), 0.0, (16, 1, 1), (1, 16, 1, 0, 0, 0)))


def _id(c):
    P, grid, xy, v, _ = c
    return f"P{P}-{'x'.join(map(str, grid))}-xy{xy}-" + ("auto" if v is None else f"TZ{v[0]}NW{v[1]}BZ{v[2]}")


def expected_instantiations():
    """The list the suite must reach, written down from the dispatch rules' domain and not from CASES: (kernel, P, SHEAR, ...)."""
    out = set()
    for P in range(4, 15):
        for sh in (0, 1):
            out.add(("spread_tiles", P, sh, 8, 1))
            out.add(("spread_tiles", P, sh, 16, 1))
            if P <= 8:
                out.add(("spread_tiles", P, sh, 8, 4))
            out.add(("gather_bins", P, sh, 1))
            if P <= 7:
                out.add(("gather_bins", P, sh, 2))
    out.add(("spread_atomic",))
    out.add(("gather",))
    return out


def instantiations_of(P, path):
    sf, tz, nw, gf, bz, sh = path
    return {("spread_tiles", P, sh, tz, nw) if sf else ("spread_atomic",), ("gather_bins", P, sh, bz) if gf else ("gather",)}


def families_of(path):
    sf, tz, nw, gf, bz, _ = path
    return (f"k_spread_tiles TZ{tz}/NW{nw}" if sf else "k_spread_atomic"), (f"k_gather_bins BZ{bz}" if gf else "k_gather")


SEEN = {}        # case id -> far_path tuple
WORST = {}       # kernel family -> worst error / (TOL sum|terms|)
_REFS = {}       # (P, grid, xy) -> inputs and references, computed once and shared by the variants


def _worst(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _engine(monkeypatch, n_max, P, grid, xy, forced):
    import pse_amd
    for name, value in zip(SWITCHES, forced or (None, None, None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))       # read per handle, in pse_create
    box = (grid[0] * fr.H, grid[1] * fr.H, grid[2] * fr.H, float(xy))
    return pse_amd.Engine(n_max, box, **fr.engine_kwargs(P, grid))


def _reference(oracle, P, grid, xy):
    key = (P, grid, xy)
    if key in _REFS:
        return _REFS[key]
    sparse = (P + int(xy != 0.0)) % 2 == 0             # every second configuration has no filler: nodes outside every support
    pos, force, box, parts = fr.make_case(P, grid, xy, seed=1000 + 10 * P + int(xy != 0.0), n_fill=600 if P <= 8 else 300,
                                         sparse=sparse)
    _, p = fr.case_params(oracle, P, grid, xy)
    clear = fr.clearance(pos, box, grid, P)
    assert clear.min() >= fr.CLEAR, float(clear.min())
    r = dict(pos=pos, force=force, box=box, parts=parts, p=p, sparse=sparse)
    r["spread"], r["spread_mag"] = fr.spread_ref(pos, force, box, p)
    assert (r["spread_mag"] == 0).any() or not sparse
    rng = np.random.default_rng(77 + P)
    r["grid_values"] = rng.normal(size=(3,) + tuple(grid))
    r["gather"], r["gather_mag"] = fr.gather_ref(r["grid_values"], pos, box, p)
    r["wave"] = oracle.mobility_wave(pos, force, box, p)
    # the particles that fill the grids before the spread under test: everywhere, and large
    r["other_pos"] = fr._to_pos(rng.uniform(0.0, 1.0, (400, 3)) * np.asarray(grid, dtype=float)[None, :], box, grid)
    r["other_force"] = 1e3 * rng.normal(size=(400, 3))
    r["perm"] = rng.permutation(len(pos))
    r["impulses"] = []
    if P in IMPULSE_P:
        j = int(parts["planted"][0])
        nodes, w = fr.support_of(pos[j], box, p)
        before = [(int(nodes[a][0]) - 1) % grid[a] for a in range(3)]          # the node in front of the support on every axis
        picks = {"corner": (0, 0, 0), "edge": (0, P - 1, P // 2), "centre": (P // 2, (P - 1) // 2, P // 2), "outside": None}
        for name, t in picks.items():
            node = before if t is None else [int(nodes[a][t[a]]) for a in range(3)]
            g = np.zeros((3,) + tuple(grid))
            g[:, node[0], node[1], node[2]] = 1.0
            u, mag = fr.gather_ref(g, pos, box, p)
            h3 = fr.LD(p["h"][0]) * fr.LD(p["h"][1]) * fr.LD(p["h"][2])
            if t is None:
                assert (mag[j] == 0).all()
            else:
                assert (u[j] == h3 * w[t]).all() and (mag[j] > 0).all()
            assert (mag == 0).any()                                           # some particle does not reach the node
            r["impulses"].append((name, g, u, mag))
    _REFS[key] = r
    return r


def _check_spread(g, r, family, what):
    ref, mag = r["spread"], r["spread_mag"]
    assert g.shape == ref.shape
    untouched = mag == 0
    assert (g[untouched] == 0.0).all(), f"{what}: {int((g[untouched] != 0.0).sum())} nodes outside every support are not 0.0"
    ratio = fr.worst_ratio(g, ref, mag, TOL)
    _worst(family, ratio)
    print(f"  {what}: worst |g - ref| / (TOL sum|terms|) = {ratio:.4f}  ({family}; {int(untouched.sum())} nodes outside every support)")
    assert ratio <= 1.0, (what, ratio)


def _check_gather(u, ref, mag, family, what):
    untouched = mag == 0
    assert (u[untouched] == 0.0).all(), f"{what}: particles that do not reach a nonzero node got a velocity"
    ratio = fr.worst_ratio(u, ref, mag, TOL)
    _worst(family, ratio)
    print(f"  {what}: worst |u - ref| / (TOL sum|terms|) = {ratio:.4f}  ({family})")
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_far_field_case(torch_cuda, oracle, monkeypatch, case):
    P, grid, xy, forced, want = case
    T0.append(time.time())
    r = _reference(oracle, P, grid, xy)
    pos, force, p = r["pos"], r["force"], r["p"]
    n = len(pos)
    eng = _engine(monkeypatch, n, P, grid, xy, forced)
    try:
        info = eng.info()
        assert (info["Nx"], info["Ny"], info["Nz"]) == tuple(grid) and info["P"] == P and abs(info["eta"] - p["eta"]) < 1e-14
        path = tuple(eng.far_path(n)[k] for k in eng.FAR_PATH_FIELDS)
        SEEN[_id(case)] = (P, path)
        assert path == want, (path, want)
        fam_s, fam_g = families_of(path)
        pos4, f4 = to4(pos), to4(force)
        # spread: after other particles have been spread into the same grids
        eng.debug_spread(to4(r["other_pos"]), to4(r["other_force"]))
        g = eng.debug_spread(pos4, f4)
        _check_spread(g, r, fam_s, "spread")
        # gather: a random grid, then grids with a single nonzero node
        u = eng.debug_gather(pos4, r["grid_values"]).cpu().numpy()[:, :3]
        _check_gather(u, r["gather"], r["gather_mag"], fam_g, "gather, random grid")
        for name, gi, ui, magi in r["impulses"]:
            _check_gather(eng.debug_gather(pos4, gi).cpu().numpy()[:, :3], ui, magi, fam_g, f"gather, impulse at a {name} node")
        # chain
        uw = eng.mobility(pos4, f4, parts=2).cpu().numpy()[:, :3]
        e = np.linalg.norm(uw - r["wave"]) / np.linalg.norm(r["wave"])
        print(f"  chain: rel {e:.2e}")
        assert e < 1e-10, e
        # order
        perm = r["perm"]
        pp4, pf4 = to4(pos[perm]), to4(force[perm])
        _check_spread(eng.debug_spread(pp4, pf4), r, fam_s, "spread, permuted order")
        u2 = eng.debug_gather(pp4, r["grid_values"]).cpu().numpy()[:, :3]
        assert (u2 == u[perm]).all(), "the gather depends on the order of the particles"
    finally:
        eng.close()


# all particles in one bin: fewer than, exactly and one more than the 64 candidates of a chunk of the spread (and one, two passes of the
# gather: 40 particles per pass for P <= 7, 32 above)
SMALL = [(5, fr.matrix_xy(5), (8, 4, 2)), (5, 0.0, (16, 1, 1)), (8, 0.0, (8, 1, 1)), (8, fr.matrix_xy(8), (8, 4, 1))]


@pytest.mark.parametrize("P,xy,forced", SMALL, ids=[f"P{c[0]}-xy{c[1]}-TZ{c[2][0]}NW{c[2][1]}BZ{c[2][2]}" for c in SMALL])
def test_few_particles_in_one_bin(torch_cuda, oracle, monkeypatch, P, xy, forced):
    grid = fr.matrix_grid(P)
    _, p = fr.case_params(oracle, P, grid, xy)
    eng = _engine(monkeypatch, 65, P, grid, xy, forced)
    grid_values = np.random.default_rng(5).normal(size=(3,) + tuple(grid))
    try:
        for n in (1, 2, 63, 64, 65):
            pos, force, box = fr.one_bin_case(P, grid, xy, n, seed=n)
            assert len(pos) == n and fr.clearance(pos, box, grid, P).min() >= fr.CLEAR
            assert len(set(map(tuple, fr.origin_bins(pos, box, grid, P)))) == 1
            path = tuple(eng.far_path(n)[k] for k in eng.FAR_PATH_FIELDS)
            assert path == (1, forced[0], forced[1], 1, forced[2], int(xy != 0.0)), path
            fam_s, fam_g = families_of(path)
            r = {}
            r["spread"], r["spread_mag"] = fr.spread_ref(pos, force, box, p)
            eng.debug_spread(to4(-pos), to4(1e3 * force[::-1].copy()))          # (other particles first)
            _check_spread(eng.debug_spread(to4(pos), to4(force)), r, fam_s, f"spread, N = {n}")
            u, mag = fr.gather_ref(grid_values, pos, box, p)
            _check_gather(eng.debug_gather(to4(pos), grid_values).cpu().numpy()[:, :3], u, mag, fam_g, f"gather, N = {n}")
            uw = eng.mobility(to4(pos), to4(force), parts=2).cpu().numpy()[:, :3]
            ref = oracle.mobility_wave(pos, force, box, p)
            assert np.linalg.norm(uw - ref) / np.linalg.norm(ref) < 1e-10
    finally:
        eng.close()


def test_every_instantiation_was_reached(torch_cuda, monkeypatch):
    """The union of the paths the cases ran on is the whole list: a change of a dispatch threshold cannot drop an instantiation from
    the suite without this test (and the case written for it) failing.  A case that was not run in this session (a -k selection) is
    asked for its path here: creating its engine is enough."""
    reached = set()
    for c in CASES:
        P, grid, xy, forced, _ = c
        if _id(c) not in SEEN:
            eng = _engine(monkeypatch, 1500, P, grid, xy, forced)
            SEEN[_id(c)] = (P, tuple(eng.far_path(1500)[k] for k in eng.FAR_PATH_FIELDS))
            eng.close()
        reached |= instantiations_of(*SEEN[_id(c)])
    want = expected_instantiations()
    assert reached == want, {"missing": sorted(want - reached), "unexpected": sorted(reached - want)}
    lines = [f"{len(reached)} instantiations reached: " + ", ".join(sorted(" ".join(map(str, t)) for t in reached))]
    lines += [f"worst error / (TOL sum|terms|), TOL = {TOL:g}: {fam}: {ratio:.4f}" for fam, ratio in sorted(WORST.items())]
    lines.append(f"seconds since the first case of this module began: {time.time() - T0[0] if T0 else 0.0:.1f}")
    print("\n".join(lines))
