"""The chain statistics without a GPU: the exact reference of tests/chain_stats_ref.py against closed forms, mpmath and its own
invariances; pse_host_chain_order and `terms` against the reference; the float64 restatement of the kernel's order against the exact
reference within the bounds that the device is held to; the conditions of the GPU inputs; the NumPy helper; the argument checks of the
Python layers; and every refusal of the pse_molecule_pairs_* entry points through the device stand-in of the sanitizer build
(pse_amd/csrc/asan_stub.cpp, which runs the real validators and the real layout), built here without a sanitizer."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import conformation_cases as cc
import conformation_ref as cr
import chain_stats_ref as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
BOX = (64.0, 64.0, 64.0, 0.0)


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def lib():
    from pse_amd import build, _lib
    build.build_lib()
    return _lib.load()


# ---- the reference against closed forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,b", [(2, 0.5), (9, 0.75), (40, 1.25)])
def test_reference_on_a_straight_rod(m, b):
    """D(s) = (m - s) (s b)^2, C(s) = (m - 1 - s) b^2, 1/Rh = (2 / m^2) sum_s (m - s) / (s b); the rod lies across the box's faces."""
    n, bonds, _, _ = cc.build([("chain", m)])
    pos = cc.wrap(np.array([30.0, -31.0, 5.0]) + np.arange(m)[:, None] * np.array([b, 0.0, 0.0]), BOX)
    ref = cs.reference(pos, BOX, bonds, None, 1, m + 2)
    s = np.arange(m + 2)
    assert np.array_equal(ref["curves"][0, :, 0], np.maximum(m - s, 0) * (s * b) ** 2)
    assert np.array_equal(ref["curves"][0, :, 1], np.maximum(m - 1 - s, 0) * b * b)
    assert np.array_equal(ref["terms"][0, :, 0], np.maximum(m - s, 0)) and np.array_equal(ref["terms"][0, :, 1], np.maximum(m - 1 - s, 0))
    want = 2 * sum(Fraction(m - k, k) for k in range(1, m)) / (Fraction(b) * m * m)
    assert ref["inv_rh"][0] == float(want) and ref["sums"][0, 0] == float(want) and ref["sums"][0, 1] == float(want * want)
    assert ref["inexact"] == 0 and ref["nzero"] == 0 and ref["rmin"] == b


@pytest.mark.parametrize("m", [3, 12, 64])
def test_reference_on_a_regular_ring(m):
    """1/Rh of a regular m-gon of radius R: (1 / (m R)) sum_{k=1}^{m-1} 1 / (2 sin(pi k / m)); a ring has no curves."""
    import mpmath
    mpmath.mp.dps = 40
    n, bonds, _, _ = cc.build([("ring", m)])
    R = 3.0
    t = 2.0 * np.pi * np.arange(m) / m
    pos = np.stack([R * np.cos(t), R * np.sin(t), np.zeros(m)], 1)
    ref = cs.reference(pos, BOX, bonds, None, 1, 4)
    want = float(sum(1 / (2 * mpmath.sin(mpmath.pi * k / m)) for k in range(1, m)) / (m * R))
    assert abs(ref["inv_rh"][0] - want) <= 1e-14 * want                       # (the vertices are rounded to float64)
    assert not ref["curves"].any() and not ref["terms"].any() and not ref["linear"][0]


def test_reference_on_the_dimer_and_on_coincident_beads():
    """The dimer: 1/Rh = 1 / (2 r).  A pair at distance 0 adds nothing: a trimer whose ends coincide has 1/Rh = (2 / 9) (2 / r)."""
    pos = np.array([[31.5, 0.0, 0.0], [-31.25, 0.25, 0.0]])                   # across the box: r^2 = 1.25^2 + 0.25^2
    ref = cs.reference(pos, BOX, [[0, 1]], None, 1, 2)
    r2 = Fraction(25, 16) + Fraction(1, 16)
    assert abs(ref["inv_rh"][0] - 0.5 / float(r2) ** 0.5) <= 2 * cc.EPS and ref["curves"][0].tolist() == [[0.0, float(r2)], [float(r2), 0.0]]
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 4.0, 3.0], [1.0, 2.0, 3.0]])
    ref = cs.reference(pos, BOX, [[0, 1], [1, 2]], None, 1, 3)
    assert ref["nzero"] == 1 and ref["inv_rh"][0] == float(Fraction(2, 9)) and ref["curves"][0].tolist() == [[0.0, 8.0], [8.0, -4.0], [0.0, 0.0]]


def test_inverse_distances_against_mpmath():
    """The integer square roots of the reference against mpmath at 40 digits on the smallest general case."""
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.default_rng(2)
    n, bonds, _, _ = cc.build([("chain", 12), ("star", 7)])
    pos = cc.wrap(cc.place(n, bonds, (16.0, 16.0, 16.0, 0.5), rng, 3.0), (16.0, 16.0, 16.0, 0.5))
    box = (16.0, 16.0, 16.0, 0.5)
    ref = cs.reference(pos, box, bonds, None, 1, 12)
    mols, _ = cr.layout(n, bonds)
    U, scale = cs.exact_offsets(pos, box, mols)
    for k, u in enumerate(U):
        m = len(u)
        h = sum(1 / mpmath.sqrt(mpmath.mpf(int(((u[i] - u[j]) ** 2).sum())) / (scale * scale)) for i in range(m) for j in range(i))
        assert abs(mpmath.mpf(float(ref["inv_rh"][k])) - 2 * h / (m * m)) <= mpmath.mpf(2) ** -53 * 2 * h / (m * m)
        assert abs(ref["hsum"][k] - float(h)) <= 1e-15 * float(h)


@pytest.mark.parametrize("name", ["shuffled chain", "four 64", "star 256"])
def test_reference_is_invariant_under_relabelling_lattice_shifts_and_reversal(name):
    box, n, bonds, pos, types, ntypes = cc.DYADIC[name]
    ns = 64
    ref = cs.reference(pos, box, bonds, types, ntypes, ns)
    rng = np.random.default_rng(9)
    moved = cs.reference(cc.reimage(pos, box, rng), box, bonds, types, ntypes, ns)
    b2, new_of_old = cc.relabel(n, bonds, rng)
    p2 = np.empty_like(pos); p2[new_of_old] = pos
    relabelled = cs.reference(p2, box, b2, types, ntypes, ns)
    flipped = cs.reference(pos[::-1].copy(), box, (n - 1 - np.asarray(bonds)), None if types is None else types[::-1], ntypes, ns)   # the chain reversed, the molecules too
    for other in (moved, relabelled, flipped):
        assert np.array_equal(other["curves"], ref["curves"]) and np.array_equal(other["sums"], ref["sums"])
        assert np.array_equal(np.sort(other["inv_rh"]), np.sort(ref["inv_rh"])) and np.array_equal(other["terms"], ref["terms"])
    assert np.array_equal(moved["inv_rh"], ref["inv_rh"]) and np.array_equal(relabelled["inv_rh"], ref["inv_rh"])


# ---- the host layout: chain rank, terms ---------------------------------------------------------------------------------------------

def rank_cases():
    rng = np.random.default_rng(5)
    out = {}
    for name, shapes, gaps in (("chains", [("chain", 20)] * 3 + [("chain", 2), ("chain", 3)], ()), ("stars", [("star", 9), ("star", 3)], (1,)),
                               ("rings", [("ring", 12), ("ring", 3)], ()), ("comb", [("comb", 7), ("chain", 4)], ()),
                               ("edge shapes", cc.EDGE_SHAPES, (2, 0, 1, 0, 0, 3))):
        n, bonds = cc.build(shapes, gaps=gaps)[:2]
        out[name] = (n, bonds)
        perm = rng.permutation(n)
        out[name + " shuffled"] = (n, perm[bonds][rng.permutation(len(bonds))][:, ::-1])
    return out


RANKS = rank_cases()


@pytest.mark.parametrize("name", sorted(RANKS))
def test_host_chain_order_against_the_reference(lib, name):
    """rank[slot] of pse_host_chain_order on the arrays of pse_host_molecule_rows: the reference's own rank, found by walking the
    bonds; a linear molecule counts from the end with the lower caller index and consecutive ranks are bonded."""
    n, bonds = RANKS[name]
    b = np.ascontiguousarray(bonds, dtype=np.uint32)
    h = max(n // 2, 1)
    a = dict(mol_of=np.zeros(n, np.int32), members=np.zeros(n, np.uint32), parent=np.zeros(n, np.uint32), depth=np.zeros(n, np.uint32),
             mol_off=np.zeros(h + 1, np.uint32), ends=np.zeros(2 * h, np.uint32), nring=np.zeros(h, np.uint32),
             tile_mol=np.zeros(h + 1, np.uint32), tile_rounds=np.zeros(h, np.uint32), counts=np.zeros(3, np.uint32))
    assert lib.pse_host_molecule_rows(n, b.shape[0], vp(b), *[vp(v) for v in a.values()]) == 0
    nmol, nmem = int(a["counts"][0]), int(a["counts"][1])
    rank = np.full(nmem + 1, 77, np.uint32)
    assert lib.pse_host_chain_order(nmol, vp(a["parent"]), vp(a["mol_off"]), vp(a["ends"]), vp(rank)) == 0
    assert rank[nmem] == 77
    mols, _ = cr.layout(n, bonds)
    want = cs.ranks_of(n, bonds, mols)
    bondset = {tuple(sorted(x)) for x in np.asarray(bonds).tolist()}
    for k, mo in enumerate(mols):
        o, e = int(a["mol_off"][k]), int(a["mol_off"][k + 1])
        assert rank[o:e].tolist() == want[k]
        if mo["ends"] is not None:
            along = np.empty(e - o, dtype=int); along[rank[o:e]] = a["members"][o:e]
            assert along[0] < along[-1] and all(tuple(sorted((int(along[q]), int(along[q + 1])))) in bondset for q in range(e - o - 1))
        else:
            assert rank[o:e].tolist() == list(range(e - o))
    for drop in range(4):
        args = [vp(a["parent"]), vp(a["mol_off"]), vp(a["ends"]), vp(rank)]
        args[drop] = None
        assert lib.pse_host_chain_order(nmol, *args) == INVALID and "null array" in lib.pse_last_error().decode()


# ---- the kernel's order within the bounds; the conditions of the GPU inputs --------------------------------------------------------

@pytest.mark.parametrize("k", range(len(cc.EDGES)))
def test_general_cases_keep_their_distances_and_the_kernel_order_keeps_the_bound(k):
    """Every EDGES case has its smallest intramolecular distance >= 0.05 (measured: 0.064 to 0.129) and no coincident pair, so that
    the relative error of r2 stays below 1/2 as the bound of 1/r assumes; terms equals a brute-force count; and the kernel's
    operations in their order, in NumPy float64, stay within the bounds that the device is held to."""
    box, n, bonds, pos, types, ntypes, ns, ref = cs.edge(k)
    assert ref["rmin"] >= 0.05 and ref["nzero"] == 0
    assert {2, 3, 63, 64, 65, 255, 257, 1023} <= set(ref["size"].tolist()) and ns == 1024
    t = np.zeros(len(ref["size"]), dtype=int) if types is None else types
    brute = np.zeros((ntypes, ns, 2), dtype=np.int64)
    for a, m in zip(t[ref["linear"]], ref["size"][ref["linear"]]):
        for s in range(ns):
            brute[a, s, 0] += sum(1 for c in range(m) if c + s < m)
            brute[a, s, 1] += sum(1 for c in range(m - 1) if c + s < m - 1)
    assert np.array_equal(ref["terms"], brute)
    inv, curves, sums = cs.kernel_order(pos, box, bonds, types, ntypes, ns)
    tol, ctol, stol, x = cs.bounds(ref, box, types, ntypes, ns)
    assert x <= 0.5
    err = np.abs(inv - ref["inv_rh"])
    assert np.all(err <= tol) and (err / tol).max() > 1e-9                     # ... and the bound is not vacuous by many orders
    assert np.all(np.abs(curves - ref["curves"]) <= ctol) and np.all(np.abs(sums - ref["sums"]) <= stol)


@pytest.mark.parametrize("name", sorted(cc.DYADIC))
def test_dyadic_cases_are_exact_and_the_kernel_order_keeps_their_bound(name):
    """The reference rounds no entry of the curves, the restated order gives their bits, and 1/Rh within (P + 4) 2^-53; the cases
    "1024 chain", "2 64 256 1024" and "four 64" contain coincident pairs (253, 229 and 33): the zero rule is exercised."""
    box, n, bonds, pos, types, ntypes, ns, ref = cs.dyadic(name)
    assert ref["inexact"] == 0
    want = {"1024 chain": 253, "2 64 256 1024": 229, "four 64": 33}
    assert ref["nzero"] == want.get(name, 0)
    inv, curves, sums = cs.kernel_order(pos, box, bonds, types, ntypes, ns)
    assert np.array_equal(curves, ref["curves"])
    tol, stol = cs.dyadic_bounds(ref, types, ntypes)
    assert np.all(np.abs(inv - ref["inv_rh"]) <= tol) and np.all(np.abs(sums - ref["sums"]) <= stol)


# ---- the NumPy helper and the Python layers --------------------------------------------------------------------------------------------

def test_persistence_length_of_on_a_synthetic_exponential():
    from pse_amd import analyze
    s = np.arange(12)
    b, lp = 0.97, 4.5
    c = np.exp(-s * b / lp)
    for smax in (1, 3, 11, 40):
        assert np.isclose(analyze.persistence_length_of(s, c, b, smax), lp, rtol=1e-12)
    c2 = c.copy(); c2[4] = -0.01                                               # the fit stops before the first c(s) <= 0
    assert np.isclose(analyze.persistence_length_of(s, c2, b, 11), lp, rtol=1e-12)
    c2[1] = 0.0
    assert np.isnan(analyze.persistence_length_of(s, c2, b, 11))
    c3 = c.copy(); c3[5] = np.nan
    assert np.isclose(analyze.persistence_length_of(s, c3, b, 11), lp, rtol=1e-12)
    assert analyze.persistence_length_of(s, np.ones(12), b, 3) == float("inf")
    with pytest.raises(ValueError, match="smax"):
        analyze.persistence_length_of(s, c, b, 0)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


class _NoDeviceEngine(_NoDevice):
    n_max = 64


def test_python_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    bonds = cc.build([("chain", 4), ("chain", 3), ("star", 4)], gaps=(1,))[1]
    for word, kw in [("non-empty integer (nbonds, 2)", dict(bonds=[[0, 1, 2]])), ("no molecule", dict(bonds=[[2, 2]])),
                     ("period", dict(bonds=bonds, period=0)), ("capacity", dict(bonds=bonds, capacity=0)),
                     ("3 molecules", dict(bonds=bonds, molecule_types=[0, 1])), ("one type", dict(bonds=bonds, type_names=["A", "B"])),
                     ("smax = 0", dict(bonds=bonds, smax=0)), ("smax = 1025", dict(bonds=bonds, smax=1025))]:
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
            analyze.ChainStatistics(_NoDevice(), **kw)
    for word, args in (("ntypes = 9", (bonds, None, 9)), ("type 2 >= ntypes = 2", (bonds, [0, 2, 0], 2)), ("3 molecules", (bonds, [0, 1], 2)),
                       ("ns = 0", (bonds, None, 1, 0)), ("ns = 1025", (bonds, None, 1, 1025))):
        with pytest.raises(ValueError, match=word):
            engine.MoleculePairs(_NoDeviceEngine(), *args)


# ---- the entry points on the device stand-in --------------------------------------------------------------------------------------------

NAMES = ("pse_molecule_pairs_create", "pse_molecule_pairs_destroy", "pse_molecule_pairs_counts", "pse_molecule_pairs_compute")


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
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


def stub_handle(stub, n_max, L=20.0):
    from pse_amd._lib import pse_params
    p = pse_params()
    p.n_max, p.Lx, p.Ly, p.Lz, p.xy = n_max, L, L, L, 0.0
    p.xi, p.error, p.max_strain, p.seed = 0.5, 1e-3, 0.5, 1
    p.Nx = p.Ny = p.Nz = 0
    p.P, p.rcut, p.device, p.n_slabs, p.slab_rank = 0, 0.0, -1, 1, 0
    h = ctypes.c_void_p()
    assert stub.pse_create(ctypes.byref(p), ctypes.byref(h)) == 0, stub.pse_last_error()
    return h


def test_refusals_of_the_entry_points_in_the_stated_order(stub):
    n = 12
    h = stub_handle(stub, n)
    pairs = np.array([[0, 1], [1, 2], [4, 5], [7, 8], [8, 9], [9, 7]], dtype=np.uint32)          # a trimer, a dimer, a triangle
    good = dict(n=n, nbonds=len(pairs), pairs=pairs, types=np.array([0, 1, 1], dtype=np.uint32), ntypes=2, ns=4)

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_molecule_pairs_create(hh, a["n"], a["nbonds"], vp(a["pairs"]), vp(a["types"]), a["ntypes"], a["ns"],
                                            ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_molecule_pairs_create" in msg, (word, msg)
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
    refused("ntypes = 9", ntypes=9, ns=0)
    refused("molecule 1 has type 2 >= ntypes = 2", types=np.array([0, 2, 1], dtype=np.uint32), ns=0)
    refused("ns = 0", ns=0)
    refused("ns = -3", ns=-3)
    refused("ns = 1025", ns=1025)
    big = stub_handle(stub, 1100)
    refused("1025 members", hh=big, n=1100, pairs=np.ascontiguousarray(cc.chain(3, 1025), dtype=np.uint32), nbonds=1024, types=None, ntypes=0)
    rc, m = create()
    assert rc == 0 and m.value, stub.pse_last_error()
    rc, m1 = create(ns=1024, types=None, ntypes=1)
    assert rc == 0 and m1.value, stub.pse_last_error()
    # pse_molecule_pairs_counts: the real layout behind the stand-in
    nmol, nty, terms = ctypes.c_uint(77), np.full(2, 77, np.uint32), np.full((2, 4, 2), 77, np.uint64)
    assert stub.pse_molecule_pairs_counts(m, ctypes.byref(nmol), vp(nty), vp(terms)) == 0
    assert nmol.value == 3 and nty.tolist() == [1, 2]
    assert terms.tolist() == [[[3, 2], [2, 1], [1, 0], [0, 0]], [[2, 1], [1, 0], [0, 0], [0, 0]]]   # the trimer; the dimer (the triangle is not linear)
    assert stub.pse_molecule_pairs_counts(m, None, None, vp(terms)) == 0 and stub.pse_molecule_pairs_counts(m1, ctypes.byref(nmol), None, None) == 0
    for word, args in (("null molecule-pair object", (None, ctypes.byref(nmol), vp(nty), vp(terms))), ("all null", (m, None, None, None))):
        assert stub.pse_molecule_pairs_counts(*args) == INVALID
        assert word in stub.pse_last_error().decode() and "pse_molecule_pairs_counts" in stub.pse_last_error().decode()
    # pse_molecule_pairs_compute: the arrays are device pointers, which the stand-in never follows
    buf = np.zeros(64)
    at = lambda off=0: ctypes.c_void_p(buf.ctypes.data + off)   # noqa: E731
    assert buf.ctypes.data % 8 == 0

    def compute(word, mm=m, pos=at(), inv_rh=at(), curves=at(), sums=at(), sample=at()):
        rc = stub.pse_molecule_pairs_compute(mm, pos, inv_rh, curves, sums, sample)
        msg = stub.pse_last_error().decode()
        assert (word is None and rc == 0) or (rc == INVALID and word in msg and "pse_molecule_pairs_compute" in msg), (word, rc, msg)

    compute("null molecule-pair object", mm=None, pos=None)
    compute("null pos", pos=None, inv_rh=None, curves=None, sums=None, sample=None)
    compute("all null", inv_rh=None, curves=None, sums=None, sample=None)
    compute("inv_rh =", inv_rh=at(4), curves=at(4))
    compute("curves =", curves=at(4), sums=at(4))
    compute("sums =", sums=at(4), sample=at(4))
    compute("sample =", sample=at(4))
    compute(None)
    for name in ("inv_rh", "curves", "sums", "sample"):                        # each output alone
        compute(None, **{k: (at() if k == name else None) for k in ("inv_rh", "curves", "sums", "sample")})
    assert not buf.any()
    assert stub.pse_molecule_pairs_destroy(m1) == 0 and stub.pse_molecule_pairs_destroy(None) == 0
    for hh in (h, big):                                                        # m is still alive: it goes with its handle
        assert stub.pse_destroy(hh) == 0
