"""CPU tests of the chain conformations that need no device: the layout of pse_host_molecule_rows against the plain-Python layout of
tests/conformation_ref.py and scipy's connected_components, with every refusal; the exact rational reference against closed forms, the
NumPy formula of the examples and its own invariances; the margins of the inputs that tests/test_gpu_conformations.py runs, and a
float64 restatement of the kernel's order of operations against the bound it is held to there; the NumPy helpers; the argument checks
of the Python layers; and every refusal of the pse_molecules_* entry points through the device stand-in of the sanitizer build
(pse_amd/csrc/asan_stub.cpp, which runs the real validators and the real layout), built here without a sanitizer."""
import ctypes
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import conformation_cases as cc
import conformation_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NONE = 0xffffffff


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def lib():
    from pse_amd import build, _lib
    build.build_lib()
    return _lib.load()


def host_rows(lib, n, bonds, drop=()):
    """pse_host_molecule_rows as a dict of arrays cut to their used lengths, or (rc, message) after a refusal.  drop: outputs passed as NULL."""
    b = np.ascontiguousarray(bonds, dtype=np.uint32)
    h = max(n // 2, 1)
    a = dict(mol_of=np.full(n, -7, np.int32), members=np.zeros(n, np.uint32), parent=np.zeros(n, np.uint32), depth=np.zeros(n, np.uint32),
             mol_off=np.zeros(h + 1, np.uint32), ends=np.zeros(2 * h, np.uint32), nring=np.zeros(h, np.uint32),
             tile_mol=np.zeros(h + 1, np.uint32), tile_rounds=np.zeros(h, np.uint32), counts=np.zeros(3, np.uint32))
    rc = lib.pse_host_molecule_rows(n, b.shape[0], vp(b) if "pairs" not in drop else None, *[None if k in drop else vp(v) for k, v in a.items()])
    if rc:
        return rc, lib.pse_last_error().decode()
    nmol, nmem, ntiles = (int(v) for v in a["counts"])
    cut = dict(members=nmem, parent=nmem, depth=nmem, mol_off=nmol + 1, ends=2 * nmol, nring=nmol, tile_mol=ntiles + 1, tile_rounds=ntiles)
    return {k: (v[:cut[k]] if k in cut else v) for k, v in a.items()}


def layout_cases():
    rng = np.random.default_rng(5)
    out = {}
    out["chains"] = cc.build([("chain", 20)] * 7 + [("chain", 2), ("chain", 3)])[:2]
    out["star"] = cc.build([("star", 9)])[:2]
    out["ring"] = cc.build([("ring", 12), ("ring", 3)])[:2]
    out["comb"] = cc.build([("comb", 7), ("chain", 4)])[:2]
    n, bonds = cc.build([("chain", 33)], gaps=(2,))[:2]
    perm = rng.permutation(n)
    out["shuffled chain"] = (n, perm[bonds][rng.permutation(len(bonds))][:, ::-1])
    out["unbonded"] = cc.build([("chain", 5), ("star", 4), ("chain", 2)], gaps=(3, 2, 4))[:2]
    out["unbonded"] = (out["unbonded"][0] + 5, out["unbonded"][1])
    out["513 dimers"] = cc.build([("chain", 2)] * 513)[:2]
    out["1024-mer"] = cc.build([("chain", 1024)])[:2]
    out["edge shapes"] = cc.build(cc.EDGE_SHAPES, gaps=(2, 0, 1, 0, 0, 3))[:2]
    return out


LAYOUTS = layout_cases()


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_host_layout_against_the_reference_and_scipy(lib, name):
    """Numbering, breadth-first order, parents earlier than children, depths, ends, nring, tile packing and round counts."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from pse_amd import analyze
    n, bonds = LAYOUTS[name]
    got = host_rows(lib, n, bonds)
    mols, mol_of = cr.layout(n, bonds)
    assert np.array_equal(got["mol_of"], mol_of) and int(got["counts"][0]) == len(mols)
    # scipy: the same partition, numbered by the smallest member
    _, label = connected_components(coo_matrix((np.ones(len(bonds)), (bonds[:, 0], bonds[:, 1])), shape=(n, n)), directed=False)
    size = np.bincount(label)
    roots = sorted(int(np.nonzero(label == c)[0][0]) for c in range(len(size)) if size[c] >= 2)
    assert len(roots) == len(mols)
    for k, root in enumerate(roots):
        assert np.array_equal(np.nonzero(label == label[root])[0], np.nonzero(got["mol_of"] == k)[0])
    assert np.all(got["mol_of"][size[label] == 1] == -1)
    m_of, nmol = analyze.molecules_of(n, bonds)
    assert nmol == len(mols) and np.array_equal(m_of, mol_of)
    # per molecule
    bondset = {tuple(sorted(b)) for b in np.asarray(bonds).tolist()}
    for k, mo in enumerate(mols):
        o, e = int(got["mol_off"][k]), int(got["mol_off"][k + 1])
        mem, par, dep = got["members"][o:e], got["parent"][o:e], got["depth"][o:e]
        assert np.array_equal(mem, mo["members"]) and np.array_equal(par, mo["parent"]) and np.array_equal(dep, mo["depth"])
        assert mem[0] == mem.min() == roots[k] and par[0] == 0 and dep[0] == 0
        assert np.all(par[1:] < np.arange(1, e - o)) and np.all(dep[1:] == dep[par[1:]] + 1)
        assert all(tuple(sorted((int(mem[p]), int(mem[par[p]])))) in bondset for p in range(1, e - o))
        assert np.all(np.diff(dep) >= 0)                                        # breadth first
        assert int(got["nring"][k]) == mo["nring"] == sum(1 for b in bondset if got["mol_of"][b[0]] == k) - (e - o - 1)
        ends = tuple(int(v) for v in got["ends"][2 * k:2 * k + 2])
        assert ends == (mo["ends"] if mo["ends"] is not None else (NONE, NONE))
        if mo["ends"] is not None:
            assert mem[ends[0]] < mem[ends[1]]
    # tiles
    first, rounds = cr.tiles_of(mols)
    assert got["tile_mol"].tolist() == first and got["tile_rounds"].tolist() == rounds and int(got["counts"][2]) == len(rounds)
    for t in range(len(rounds)):
        fill = int(got["mol_off"][first[t + 1]] - got["mol_off"][first[t]])
        assert 2 <= fill <= cr.TILE
        if t + 1 < len(rounds):                                                 # the next molecule did not fit
            assert fill + int(got["mol_off"][first[t + 1] + 1] - got["mol_off"][first[t + 1]]) > cr.TILE
        deepest = int(got["depth"][got["mol_off"][first[t]]:got["mol_off"][first[t + 1]]].max())
        assert 2 ** rounds[t] >= deepest + 1 > 2 ** (rounds[t] - 1)
    assert int(got["counts"][1]) == int((mol_of >= 0).sum())


def test_layout_shapes_by_hand(lib):
    assert host_rows(lib, *LAYOUTS["513 dimers"])["tile_mol"].tolist() == [0, 512, 513]
    one = host_rows(lib, *LAYOUTS["1024-mer"])
    assert one["tile_mol"].tolist() == [0, 1] and one["tile_rounds"].tolist() == [10] and one["ends"].tolist() == [0, 1023]
    star = host_rows(lib, *LAYOUTS["star"])
    assert star["ends"].tolist() == [NONE, NONE] and star["nring"].tolist() == [0] and star["tile_rounds"].tolist() == [1]
    ring = host_rows(lib, *LAYOUTS["ring"])
    assert ring["nring"].tolist() == [1, 1] and ring["ends"].tolist() == [NONE] * 4 and ring["depth"][:12].max() == 6
    dimer = host_rows(lib, 2, [[1, 0]])
    assert dimer["ends"].tolist() == [0, 1] and dimer["members"].tolist() == [0, 1] and dimer["tile_rounds"].tolist() == [1]
    edge = host_rows(lib, *LAYOUTS["edge shapes"])
    assert edge["tile_mol"].tolist() == [0, 10, 11, 17] and int(edge["mol_off"][10]) == 1024


def test_layout_refusals(lib):
    n, bonds = LAYOUTS["chains"]
    for word, args in ((f"bond 1 = (1, {n}) has an endpoint >= n = {n}", (n, [[0, 1], [1, n], [2, 2]])), ("bond 0 = (4294967295, 1)", (n, [[-1 % 2 ** 32, 1]])),
                       ("bond 1 joins particle 3 to itself", (n, [[0, 1], [3, 3], [0, 1]])),
                       ("the bond (1, 2) is listed twice", (n, [[1, 2], [3, 4], [2, 1]])),
                       ("the bond (1, 2) is listed twice", (n, [[1, 2], [1, 2]])),
                       ("1025 members", cc.build([("chain", 3), ("chain", 1025)])[:2]),
                       ("n = 0", (0, [[0, 1]])), ("no molecule", (n, np.zeros((0, 2))))):
        rc, msg = host_rows(lib, args[0], np.array(args[1], dtype=np.int64))
        assert rc == INVALID and word in msg and "pse_host_molecule_rows" in msg, (word, msg)
    for drop in ("pairs", "mol_of", "members", "parent", "depth", "mol_off", "ends", "nring", "tile_mol", "tile_rounds", "counts"):
        rc, msg = host_rows(lib, n, bonds, drop=(drop,))
        assert rc == INVALID and "null array" in msg, drop
    assert isinstance(host_rows(lib, *cc.build([("chain", 1024), ("chain", 1024)])[:2]), dict)   # the largest molecule is allowed


# ---- the reference against closed forms ------------------------------------------------------------------------------------------------

BIG = (4096.0, 4096.0, 4096.0, 0.0)


@pytest.mark.parametrize("m,b", [(2, 1.5), (3, 1.0), (17, 0.75), (64, 2.0)])
def test_reference_on_a_straight_rod(m, b):
    """m beads at spacing b along a dyadic direction d: Rg^2 = b^2 (m^2 - 1) / 12 |d|^2 exactly, G = Rg^2 d d^T / |d|^2 (rank one)."""
    d = np.array([1.0, -2.0, 0.5])
    pos = np.array([3.0, -1.0, 2.0]) + b * np.arange(m)[:, None] * d
    ref = cr.reference(pos, BIG, cc.chain(0, m))
    rg2 = Fraction(b) ** 2 * (m * m - 1) / 12 * Fraction(21, 4)
    assert ref["rows"][0, 9] == float(rg2)
    G = np.array([[ref["rows"][0, 3], ref["rows"][0, 6], ref["rows"][0, 7]], [ref["rows"][0, 6], ref["rows"][0, 4], ref["rows"][0, 8]],
                  [ref["rows"][0, 7], ref["rows"][0, 8], ref["rows"][0, 5]]])
    assert np.allclose(G, float(rg2) * np.outer(d, d) / 5.25, rtol=1e-15, atol=0)
    assert np.array_equal(ref["rows"][0, 10:13], b * (m - 1) * d) and ref["rows"][0, 13] == (b * (m - 1)) ** 2 * 5.25
    assert np.array_equal(ref["rows"][0, :3], pos.mean(axis=0))
    assert ref["sums"][0, 6] == float(rg2 * rg2) and ref["sums"][0, 13] == float(Fraction(ref["rows"][0, 13]) ** 2)


@pytest.mark.parametrize("m", [3, 4, 12, 63])
def test_reference_on_a_regular_ring(m):
    """A regular m-gon of circumradius r in the xy plane: G_xx = G_yy = r^2 / 2, Rg^2 = r^2, no ends."""
    r = 3.0
    t = 2.0 * np.pi * np.arange(m) / m
    pos = np.stack([r * np.cos(t), r * np.sin(t), np.full(m, 0.5)], 1)
    ref = cr.reference(pos, BIG, cc.ring(0, m))
    assert np.allclose(ref["rows"][0, 3:10], [4.5, 4.5, 0.0, 0.0, 0.0, 0.0, 9.0], rtol=0, atol=1e-14)
    assert np.isnan(ref["rows"][0, 10:]).all() and not ref["sums"][0, 7:].any() and ref["mols"][0]["nring"] == 1
    assert np.allclose(ref["rows"][0, :3], [0.0, 0.0, 0.5], atol=1e-15)


def test_reference_on_the_dimer_across_the_box():
    """Two beads whose bond crosses three faces of a tilted box: R is the minimum image, G = R R^T / 4, c the midpoint NOT re-wrapped."""
    box = (16.0, 32.0, 16.0, 0.5)
    pos = np.array([[7.5, 15.0, -7.0], [8.5 - 16.0 - 16.0, 16.5 - 32.0, -8.5 + 16.0]])   # the image (-1, -1, +1) of the bead at pos[0] + (1, 1.5, -1.5)
    ref = cr.reference(pos, box, [[0, 1]])
    R = np.array([1.0, 1.5, -1.5])
    assert np.array_equal(ref["rows"][0, 10:13], R) and ref["rows"][0, 13] == R @ R
    assert np.array_equal(ref["rows"][0, 3:9], np.array([R[0] ** 2, R[1] ** 2, R[2] ** 2, R[0] * R[1], R[0] * R[2], R[1] * R[2]]) / 4)
    assert np.array_equal(ref["rows"][0, :3], pos[0] + R / 2) and np.array_equal(ref["unfolded"][1, :3], pos[0] + R)


def test_reference_against_the_numpy_formula_of_the_examples():
    """The radius of gyration of examples/semiflexible_polymers.py, restated: equal contiguous chains unfolded along their bonds."""
    def radius_of_gyration(pos, box, nchains, beads):
        Lx, Ly, Lz, xy = box
        p = pos.reshape(nchains, beads, 3)
        d = p[:, 1:] - p[:, :-1]
        n = np.rint(d[..., 2] / Lz); d[..., 2] -= n * Lz
        n = np.rint(d[..., 1] / Ly); d[..., 1] -= n * Ly; d[..., 0] -= n * xy * Ly
        n = np.rint(d[..., 0] / Lx); d[..., 0] -= n * Lx
        chain = np.concatenate([np.zeros((nchains, 1, 3)), np.cumsum(d, axis=1)], axis=1)
        chain -= chain.mean(axis=1, keepdims=True)
        return np.sqrt((chain ** 2).sum(axis=2).mean(axis=1))

    rng = np.random.default_rng(2)
    nchains, beads, box = 12, 20, (24.0, 20.0, 28.0, 0.3)
    n, bonds = cc.build([("chain", beads)] * nchains)[:2]
    pos = cc.wrap(cc.place(n, bonds, box, rng, 2.5), box)
    ref = cr.reference(pos, box, bonds)
    assert np.allclose(np.sqrt(ref["rows"][:, 9]), radius_of_gyration(pos, box, nchains, beads), rtol=1e-13, atol=0)


# ---- the reference's invariances --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["shuffled chain", "star 256", "ring 64", "513 dimers", "four 64"])
def test_reference_is_invariant_under_reimaging_and_relabelling(name):
    """Dyadic inputs, so that the moved coordinates are exact: every output but c and the unfolded positions is EQUAL after every bead
    has moved by its own lattice vector of the tilted box, and those two move by the root's; a relabelling that keeps the roots permutes
    the unfolded rows and changes nothing else."""
    box, n, bonds, pos, types, ntypes = cc.DYADIC[name]
    rng = np.random.default_rng(9)
    ref = cr.reference(pos, box, bonds, types, ntypes, **cc.HIST)
    moved = cc.reimage(pos, box, rng)
    again = cr.reference(moved, box, bonds, types, ntypes, **cc.HIST)
    assert np.array_equal(again["rows"][:, 3:], ref["rows"][:, 3:], equal_nan=True) and np.array_equal(again["sums"], ref["sums"])
    assert np.array_equal(again["hist"], ref["hist"])
    shift = (moved - pos)[[mo["members"][0] for mo in ref["mols"]]]
    assert np.array_equal(again["rows"][:, :3], ref["rows"][:, :3] + shift)
    b2, new_of_old = cc.relabel(n, bonds, rng)
    p2 = np.empty_like(pos); p2[new_of_old] = pos
    perm = cr.reference(p2, box, b2, types, ntypes, **cc.HIST)
    assert np.array_equal(perm["rows"], ref["rows"], equal_nan=True) and np.array_equal(perm["sums"], ref["sums"])
    assert np.array_equal(perm["unfolded"][new_of_old], ref["unfolded"], equal_nan=True)


def test_reference_eigenvalues_are_invariant_under_rotation():
    from pse_amd import analyze
    rng = np.random.default_rng(4)
    n, bonds = cc.build([("chain", 40), ("star", 9), ("ring", 11)])[:2]
    pos = cc.place(n, bonds, BIG, rng, 2.0)
    cc.ring_place(pos, 49, 11, 2.0, rng)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    a, b = cr.reference(pos, BIG, bonds), cr.reference(pos @ q.T, BIG, bonds)
    la, lb = analyze.shape_of(analyze.tensor_of(a["rows"][:, 3:9]))[0], analyze.shape_of(analyze.tensor_of(b["rows"][:, 3:9]))[0]
    assert np.allclose(la, lb, rtol=1e-12, atol=1e-12) and np.allclose(a["rows"][:, 9], b["rows"][:, 9], rtol=1e-13)
    assert np.allclose(a["rows"][0, 13], b["rows"][0, 13], rtol=1e-13)
    assert np.allclose(analyze.tensor_of(b["rows"][:, 3:9]), q @ analyze.tensor_of(a["rows"][:, 3:9]) @ q.T, atol=1e-11)


# ---- the inputs of the GPU tests, and the kernel's order of operations --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge(k):
    lengths, xy, ntypes, seed = cc.EDGES[k]
    box, n, bonds, pos, types = cc.edge_case(lengths, xy, ntypes, seed)
    return box, n, bonds, pos, types, ntypes, cr.reference(pos, box, bonds, types, ntypes, **cc.EDGE_HIST)


@pytest.mark.parametrize("k", range(len(cc.EDGES)))
def test_general_cases_keep_their_margins_and_the_kernel_order_keeps_the_bound(k):
    """Every minimum-image decision at least 1e-6 L from a half box, every histogrammed value at least 1e-9 relative from a bin edge; the
    cases hold the sizes, shapes and types they are meant to; and the kernel's operations in their order, in NumPy float64, stay within
    the bound that the device is held to."""
    box, n, bonds, pos, types, ntypes, ref = edge(k)
    assert ref["image_margin"] > 1e-6 and ref["bin_margin"] > 1e-9
    assert {2, 3, 63, 64, 65, 255, 257, 1023} <= set(ref["size"].tolist()) and n <= 4400
    assert not ref["linear"].all() and max(mo["nring"] for mo in ref["mols"]) == 1
    assert abs(box[3]) == 0.5
    t = np.zeros(len(ref["size"]), dtype=int) if types is None else types
    if ntypes > 1:
        assert (np.bincount(t[ref["linear"]], minlength=ntypes) == 0).any()
    if ntypes == 8:
        assert (np.bincount(t, minlength=ntypes) == 0).any()
    rows, sums = cr.kernel_order(pos, box, bonds, types, ntypes)
    rows_tol, _, _, _ = cc.bounds(ref, box)
    err = np.abs(rows - ref["rows"])
    assert np.array_equal(np.isnan(rows), np.isnan(ref["rows"])) and np.all(err[~np.isnan(err)] <= rows_tol[~np.isnan(err)])
    assert np.nanmax(err / rows_tol) > 1e-7                                     # ... and the bound is not vacuous by many orders
    assert np.all(np.abs(sums - ref["sums"]) <= cc.sums_bound(ref, box, types, ntypes))


@pytest.mark.parametrize("name", sorted(cc.DYADIC))
def test_dyadic_cases_are_exact_and_the_kernel_order_gives_their_bits(name):
    box, n, bonds, pos, types, ntypes = cc.DYADIC[name]
    ref = cr.reference(pos, box, bonds, types, ntypes, **cc.HIST)
    assert ref["inexact"] == 0 and ref["image_margin"] > 1e-6 and ref["bin_margin"] > 1e-9
    if ref["inexact4"]:
        assert len(ref["mols"]) == 1 or np.bincount(types, minlength=ntypes).max() == 1
    assert np.all(pos * 256.0 == np.rint(pos * 256.0)) and set(ref["size"].tolist()) <= {2, 64, 256, 1024}
    rows, sums = cr.kernel_order(pos, box, bonds, types, ntypes)
    assert np.array_equal(rows, ref["rows"], equal_nan=True) and np.array_equal(sums, ref["sums"])


# ---- the NumPy helpers -------------------------------------------------------------------------------------------------------------------

def test_shape_of_and_orientation_angle_on_known_tensors():
    from pse_amd import analyze
    lam, b, c, k2 = analyze.shape_of(np.diag([2.0, 2.0, 2.0]))
    assert lam.tolist() == [2.0, 2.0, 2.0] and b == 0.0 and c == 0.0 and k2 == 0.0
    lam, b, c, k2 = analyze.shape_of(np.diag([0.0, 5.0, 0.0]))               # a rod
    assert np.allclose(lam, [0.0, 0.0, 5.0]) and np.isclose(b, 5.0) and np.isclose(c, 0.0) and np.isclose(k2, 1.0)
    lam, b, c, k2 = analyze.shape_of(np.diag([3.0, 1.0, 2.0]))
    assert np.allclose(lam, [1.0, 2.0, 3.0]) and np.isclose(b, 1.5) and np.isclose(c, 1.0) and np.isclose(k2, (2.25 + 0.75) / 36.0)
    assert np.isclose(k2, 1.0 - 3.0 * (2.0 + 6.0 + 3.0) / 36.0)                # the other textbook form
    lam, b, c, k2 = analyze.shape_of(np.stack([np.diag([1.0, 1.0, 4.0]), np.diag([4.0, 4.0, 1.0])]))   # prolate, oblate; batched
    assert lam.shape == (2, 3) and np.allclose(b, [3.0, 1.5]) and np.allclose(c, [0.0, 3.0])
    for chi in (0.0, 0.3, np.pi / 4, 1.2, -0.7, np.pi / 2):
        d = np.array([np.cos(chi), np.sin(chi), 0.0])
        G = 3.0 * np.outer(d, d) + 0.5 * np.eye(3)
        assert np.isclose(analyze.orientation_angle(G), chi)
    assert analyze.orientation_angle(np.zeros((4, 3, 3))).shape == (4,)
    assert np.array_equal(analyze.tensor_of([1, 2, 3, 4, 5, 6]), [[1, 4, 5], [4, 2, 6], [5, 6, 3]])


# ---- what the Python layers check before the device is touched -------------------------------------------------------------------------

class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


def esc(word):
    return word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")


def test_python_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    bonds = cc.build([("chain", 4), ("chain", 3), ("star", 4)], gaps=(1,))[1]
    nine = cc.build([("chain", k) for k in range(2, 11)])[1]
    for word, kw in [("non-empty integer (nbonds, 2)", dict(bonds=[[0, 1, 2]])), ("non-empty integer (nbonds, 2)", dict(bonds=np.zeros((0, 2), int))),
                     ("non-empty integer (nbonds, 2)", dict(bonds=[[0.5, 1.0]])), ("non-empty integer (nbonds, 2)", dict(bonds=[[0, -1]])),
                     ("no molecule", dict(bonds=[[2, 2]])),
                     ("period", dict(bonds=bonds, period=0)), ("capacity", dict(bonds=bonds, capacity=0)),
                     ("type_names", dict(bonds=bonds, type_names=["A", "A"])), ("one type", dict(bonds=bonds, type_names=["A", "B"])),
                     ("3 molecules", dict(bonds=bonds, molecule_types=[0, 1])), ("3 molecules", dict(bonds=bonds, molecule_types=[0, 1, 0, 1])),
                     ("non-negative", dict(bonds=bonds, molecule_types=[0, -1, 0])), ("outside [1, 8]", dict(bonds=bonds, molecule_types=[0, 8, 0])),
                     ("unknown type name 'C'", dict(bonds=bonds, molecule_types=["A", "C", "A"], type_names=["A", "B"])),
                     ("names need", dict(bonds=bonds, molecule_types=["A", "B", "A"])),
                     ('"size"', dict(bonds=bonds, molecule_types="length")), ("9 distinct molecule sizes", dict(bonds=nine, molecule_types="size")),
                     ("2 sizes", dict(bonds=bonds, molecule_types="size", type_names=["a", "b", "c"])),
                     ("nbins = -1", dict(bonds=bonds, nbins=-1)), ("nbins = 4097", dict(bonds=bonds, nbins=4097)),
                     ("needs rg_max and ree_max", dict(bonds=bonds, nbins=4, rg_max=2.0)),
                     ("positive", dict(bonds=bonds, nbins=4, rg_max=0.0, ree_max=1.0)),
                     ("not finite", dict(bonds=bonds, nbins=4, rg_max=1.0, ree_max=float("inf")))]:
        with pytest.raises(ValueError, match=esc(word)):
            analyze.Conformations(_NoDevice(), **kw)
    out = analyze._conformation_arguments(bonds, "size", ["three", "four"], 5, 8, 2.0, 6.0, 16)
    pairs, types, ntypes, names, period, nbins, rg_max, ree_max, capacity, sizes, values = out
    assert pairs.dtype == np.uint32 and types.tolist() == [1, 0, 1] and types.dtype == np.uint32 and ntypes == 2 and names == ["three", "four"]
    assert (period, nbins, rg_max, ree_max, capacity) == (5, 8, 2.0, 6.0, 16) and sizes.tolist() == [4, 3, 4] and values.tolist() == [3, 4]
    out = analyze._conformation_arguments(bonds, ["B", "A", "B"], ["A", "B", "C"], 1, 0, None, None, 4)
    assert out[1].tolist() == [1, 0, 1] and out[2] == 3 and out[5:8] == (0, 0.0, 0.0) and out[10] is None
    for word, args in (("non-empty integer", ([[0, 1, 2]],)), ("outside [0, n = 3)", ([[0, 3]],)), ("outside [0, n = 3)", ([[0, -1]],))):
        with pytest.raises(ValueError, match=esc(word)):
            analyze.molecules_of(3, *args)
    m_of, nmol = analyze.molecules_of(7, [[5, 6], [3, 1], [1, 2]])
    assert nmol == 2 and m_of.tolist() == [-1, 0, 0, 0, -1, 1, 1]
    for word, args in (("ntypes = 9", (bonds, None, 9)), ("type 2 >= ntypes = 2", (bonds, [0, 2, 0], 2)),
                       ("3 molecules", (bonds, [0, 1], 2)), ("nbins = 5000", (bonds, None, 1, 5000))):
        with pytest.raises(ValueError, match=esc(word)):
            engine.MoleculeTopology(_NoDeviceEngine(), *args)


class _NoDeviceEngine(_NoDevice):
    n_max = 64


# ---- the entry points on the device stand-in --------------------------------------------------------------------------------------------

NAMES = ("pse_molecules_create", "pse_molecules_destroy", "pse_molecules_count", "pse_molecules_compute")


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """The host side of the library over the device stand-in of the sanitizer build, here without a sanitizer: its pse_create runs
    the real parameter rule and its pse_molecules_* entry points the real validators and the real layout."""
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_last_error") + NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


def stub_handle(stub, n_max, L=20.0, **kw):
    from pse_amd._lib import pse_params
    p = pse_params()
    p.n_max, p.Lx, p.Ly, p.Lz, p.xy = n_max, L, L, L, 0.0
    p.xi, p.error, p.max_strain, p.seed = 0.5, 1e-3, 0.5, 1
    p.Nx = p.Ny = p.Nz = 0
    p.P, p.rcut, p.device, p.n_slabs, p.slab_rank = 0, 0.0, -1, 1, 0
    for k, v in kw.items():
        setattr(p, k, v)
    h = ctypes.c_void_p()
    assert stub.pse_create(ctypes.byref(p), ctypes.byref(h)) == 0, stub.pse_last_error()
    return h


def test_refusals_of_the_entry_points_in_the_stated_order(stub):
    n = 12
    h = stub_handle(stub, n)
    pairs = np.array([[0, 1], [1, 2], [4, 5], [7, 8], [8, 9], [9, 7]], dtype=np.uint32)          # a trimer, a dimer, a triangle
    good = dict(n=n, nbonds=len(pairs), pairs=pairs, types=np.array([0, 1, 1], dtype=np.uint32), ntypes=2, nbins=8, rg_max=3.0, ree_max=9.0)

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_molecules_create(hh, a["n"], a["nbonds"], vp(a["pairs"]), vp(a["types"]), a["ntypes"], a["nbins"], a["rg_max"], a["ree_max"],
                                       ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_molecules_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    def bonds(*rows):
        return np.array(rows, dtype=np.uint32)

    # every refusal with a LATER fault planted next to it: the earlier one is what is reported
    refused("null out", with_out=False, hh=None)
    refused("null handle", hh=None, n=0)
    refused("n = 0", n=0, nbonds=0)
    refused("n = 13", n=13, nbonds=0)
    refused("nbonds = 0", nbonds=0, pairs=None)
    refused("null pairs_host", pairs=None, ntypes=0)
    refused("bond 1 = (1, 12) has an endpoint >= n = 12", pairs=bonds((0, 1), (1, 12), (3, 3)), nbonds=3, ntypes=0)
    refused("bond 0 joins particle 3 to itself", pairs=bonds((3, 3), (1, 12)), nbonds=2, ntypes=0)
    refused("the bond (1, 2) is listed twice", pairs=bonds((1, 2), (4, 5), (2, 1)), nbonds=3, ntypes=0)
    refused("ntypes = 0", ntypes=0, types=np.array([0, 2, 1], dtype=np.uint32))
    refused("ntypes = 9", ntypes=9, nbins=-1)
    refused("molecule 1 has type 2 >= ntypes = 2", types=np.array([0, 2, 1], dtype=np.uint32), nbins=-1)
    refused("nbins = -1", nbins=-1, rg_max=0.0)
    refused("nbins = 4097", nbins=4097, rg_max=0.0)
    refused("rg_max = 0", rg_max=0.0, ree_max=-1.0)
    refused("rg_max = nan", rg_max=float("nan"))
    refused("rg_max = inf", rg_max=float("inf"))
    refused("ree_max = -1", ree_max=-1.0)
    refused("ree_max = inf", ree_max=float("inf"))
    big = stub_handle(stub, 1100)
    refused("1025 members", hh=big, n=1100, pairs=np.ascontiguousarray(cc.chain(3, 1025), dtype=np.uint32), nbonds=1024, types=None, ntypes=0)
    rc, m = create()
    assert rc == 0 and m.value, stub.pse_last_error()
    rc, m0 = create(nbins=0, rg_max=float("nan"), ree_max=-1.0, types=None, ntypes=1)     # without bins the maxima are not looked at
    assert rc == 0 and m0.value, stub.pse_last_error()
    # pse_molecules_count: the real layout behind the stand-in
    nmol, nlin, nty = ctypes.c_uint(77), np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
    assert stub.pse_molecules_count(m, ctypes.byref(nmol), vp(nlin), vp(nty)) == 0
    assert nmol.value == 3 and nlin.tolist() == [1, 1] and nty.tolist() == [1, 2]
    assert stub.pse_molecules_count(m, None, None, vp(nty)) == 0 and stub.pse_molecules_count(m0, ctypes.byref(nmol), None, None) == 0
    for word, args in (("null molecule object", (None, ctypes.byref(nmol), vp(nlin), vp(nty))), ("all null", (m, None, None, None))):
        assert stub.pse_molecules_count(*args) == INVALID
        assert word in stub.pse_last_error().decode() and "pse_molecules_count" in stub.pse_last_error().decode()
    # pse_molecules_compute: the arrays are device pointers, which the stand-in never follows
    buf = np.zeros(64)
    at = lambda off=0: ctypes.c_void_p(buf.ctypes.data + off)   # noqa: E731
    assert buf.ctypes.data % 16 == 0

    def compute(word, mm=m, pos=at(), rows=at(), unfolded=at(), sums=at(), sample=at(), hist=at()):
        rc = stub.pse_molecules_compute(mm, pos, rows, unfolded, sums, sample, hist)
        msg = stub.pse_last_error().decode()
        assert (word is None and rc == 0) or (rc == INVALID and word in msg and "pse_molecules_compute" in msg), (word, rc, msg)

    compute("null molecule object", mm=None, pos=None)
    compute("null pos", pos=None, rows=None, unfolded=None, sums=None, sample=None, hist=None)
    compute("all null", rows=None, unfolded=None, sums=None, sample=None, hist=None)
    compute("rows =", rows=at(4), unfolded=at(8))
    compute("16-byte", unfolded=at(8), sums=at(4))
    compute("sums =", sums=at(4), sample=at(4))
    compute("sample =", sample=at(4), hist=at(4))
    compute("hist =", hist=at(4))
    compute("hist =", mm=m0, hist=at(4))
    compute("nbins = 0", mm=m0)
    compute(None, mm=m0, hist=None)
    compute(None)
    for name in ("rows", "unfolded", "sums", "sample", "hist"):                # each output alone
        compute(None, **{k: (at() if k == name else None) for k in ("rows", "unfolded", "sums", "sample", "hist")})
    assert not buf.any()
    assert stub.pse_molecules_destroy(m0) == 0 and stub.pse_molecules_destroy(None) == 0
    for hh in (h, big):                                                        # m is still alive: it goes with its handle
        assert stub.pse_destroy(hh) == 0
