"""CPU tests of the pair-distance histogram that need no device: the O(N^2) reference the GPU tests compare to
(tests/pair_hist_ref.py) against the already validated typed reference (tests/pair_typed_ref.py), against itself at twice the bins
and on a simple-cubic lattice whose shells are known; g and the coordination number of pse_amd.analyze on counts whose answer is
known; the refusals of pse_pair_hist_create and pse_pair_hist_accumulate through the device stand-in of the sanitizer build
(pse_amd/csrc/asan_stub.cpp, which runs the real validators), built here without a sanitizer; and the argument checks of
analyze.RDF that come before the device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pair_hist_ref as hr
import pair_typed_ref as tr
from pair_table_ref import random_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
CAP = 8192
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
RCUT = 5.2565                                   # just below sqrt(-ln 1e-3) / 0.5 = 5.25652...
RANGES = ((0.0, 3.0), (0.7, 3.0), (0.0, RCUT), (1.0, 5.0))


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# ---- the reference ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("n", [300, 513])
def test_inputs_are_clear_of_every_edge(n, box, oracle):
    """The condition on the inputs of the GPU tests: no pair within 1e-9 of a bin edge, of rmin or of rmax, for every range and every
    number of bins they use."""
    pos = random_points(n, box, seed=11)
    i, j, r = hr.pair_distances(pos, box, oracle)
    worst = np.inf
    for rmin, rmax in RANGES:
        for nbins in (1, 2, 7, 64, 227, 1365, 2730, 8192):
            clear = hr.clearance(i, j, r, nbins, rmin, rmax)
            worst = min(worst, *clear)
            hr.assert_clear(clear)
    print(f"n = {n}: smallest clearance {worst:.3e}")


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("rng", [(0.0, 3.0), (0.7, 3.0)], ids=["rmin0", "rmin0.7"])
def test_row_sums_are_the_pair_counts_of_the_typed_reference(box, rng, oracle):
    """The sum over the bins of pair type p is the number of pairs of that type in [rmin, rmax): what pair_typed_ref.pairs_in_range
    counts with a zero table on that range for every pair type."""
    n, ntypes = 300, 3
    rmin, rmax = rng
    pos = random_points(n, box, seed=11)
    types = np.random.default_rng(21).integers(0, ntypes, n)
    counts, clear = hr.histogram(pos, box, types, ntypes, 64, rmin, rmax, oracle)
    hr.assert_clear(clear)
    zero = {(a, b): (np.zeros((2, 2)), rmin, rmax) for a in range(ntypes) for b in range(a, ntypes)}
    want = tr.pairs_in_range(pos, box, types, ntypes, zero, oracle)
    assert counts.sum(axis=1).tolist() == [want[p] for p in range(6)] and counts.sum() > 1000
    # one type: the plain count; no types: the same
    one, _ = hr.histogram(pos, box, None, 1, 64, rmin, rmax, oracle)
    assert np.array_equal(one[0], counts.sum(axis=0))
    # exclusions drop exactly the listed pairs that are in range
    i, j, r = hr.pair_distances(pos, box, oracle)
    inr = np.nonzero((r >= rmin) & (r < rmax))[0][:50]
    excl = np.stack([j[inr], i[inr]], axis=1)                                # (either order)
    less, _ = hr.histogram(pos, box, types, ntypes, 64, rmin, rmax, oracle, excl=excl)
    assert counts.sum() - less.sum() == 50 and (less <= counts).all()


@pytest.mark.parametrize("k", [1, 7, 64, 1365])
def test_folding_a_histogram_of_twice_the_bins(k, oracle):
    pos = random_points(300, TILTED, seed=11)
    types = np.random.default_rng(21).integers(0, 2, 300)
    fine, c2 = hr.histogram(pos, TILTED, types, 2, 2 * k, 0.7, 3.0, oracle)
    coarse, c1 = hr.histogram(pos, TILTED, types, 2, k, 0.7, 3.0, oracle)
    hr.assert_clear(c1), hr.assert_clear(c2)
    assert np.array_equal(fine.reshape(3, k, 2).sum(axis=2), coarse) and coarse.sum() > 500


def sc_lattice(m, a=2.0):
    g = (np.arange(m) + 0.5) * a - 0.5 * m * a
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3), (m * a, m * a, m * a, 0.0)


def test_simple_cubic_lattice_shells(oracle):
    """Spacing 2: 6, 12, 8 and 6 neighbours at 2, 2 sqrt 2, 2 sqrt 3 and 4 -- 3 N, 6 N, 4 N and 3 N pairs -- and nothing in between."""
    pos, box = sc_lattice(6)
    n = len(pos)
    nbins, rmin, rmax = 40, 0.05, 4.05                                      # bins of 0.1 with the shells inside: bins 19, 27, 34 and 39
    counts, clear = hr.histogram(pos, box, None, 1, nbins, rmin, rmax, oracle)
    assert min(clear) > 0.04, clear
    want = np.zeros(nbins, dtype=np.int64)
    want[[19, 27, 34, 39]] = 3 * n, 6 * n, 4 * n, 3 * n
    assert np.array_equal(counts[0], want)
    # a range that ends inside the third shell's gap holds the first three alone
    counts, _ = hr.histogram(pos, box, None, 1, 7, 0.0, 3.5, oracle)
    assert counts[0].tolist() == [0, 0, 0, 0, 3 * n, 6 * n, 4 * n]


def test_coordination_on_the_lattice(oracle):
    from pse_amd import analyze
    pos, box = sc_lattice(6)
    n = len(pos)
    counts, _ = hr.histogram(pos, box, None, 1, 40, 0.0, 4.0, oracle)
    edges = analyze.bin_edges(40, 0.0, 4.0)
    for r, want in ((2.5, 6.0), (3.0, 18.0), (3.5, 26.0), (4.0, 26.0), (0.0, 0.0), (2.0, 0.0)):
        assert analyze.coordination_of_counts(counts, 1, [n], 0, 0, edges, r) == want
        assert hr.coordination(pos, box, np.zeros(n, dtype=int), 0, 0, r, oracle) == want
    assert analyze.coordination_of_counts(3 * counts, 3, [n], 0, 0, edges, 3.0) == 18.0      # per sample
    with pytest.raises(ValueError, match="not a bin edge"):
        analyze.coordination_of_counts(counts, 1, [n], 0, 0, edges, 2.55)
    with pytest.raises(ValueError, match="no samples"):
        analyze.coordination_of_counts(counts, 0, [n], 0, 0, edges, 2.5)
    # two types, alternating along x: a's b partners and b's a partners from the same row; a-a from its own
    types = (np.arange(n) // 36) % 2
    c2, _ = hr.histogram(pos, box, types, 2, 40, 0.0, 4.0, oracle)
    na = [int((types == 0).sum()), int((types == 1).sum())]
    for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for r in (2.5, 3.0, 3.5):
            assert analyze.coordination_of_counts(c2, 1, na, a, b, edges, r) == hr.coordination(pos, box, types, a, b, r, oracle)
    assert analyze.coordination_of_counts(c2, 1, na, 0, 1, edges, 2.5) == 2.0 and analyze.coordination_of_counts(c2, 1, na, 0, 0, edges, 2.5) == 4.0


def test_g_of_the_ideal_gas_expectation_is_one():
    from pse_amd import analyze
    type_counts, nbins, rmin, rmax, samples = [100, 37, 1], 50, 0.7, 5.0, 4
    volume = 14.0 * 11.0 * 17.0
    edges = analyze.bin_edges(nbins, rmin, rmax)
    assert edges[0] == rmin and abs(edges[-1] - rmax) < 1e-15 and len(edges) == nbins + 1
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    P = analyze.pair_counts(type_counts)
    assert P.tolist() == [4950.0, 3700.0, 100.0, 666.0, 37.0, 0.0]          # AA, AB, AC, BB, BC, CC: one C particle has no C-C pair
    ideal = samples * P[:, None] * shell[None, :] / volume
    g = analyze.g_of_counts(ideal, samples, type_counts, edges, volume)
    assert np.abs(g[:5] - 1.0).max() < 1e-14 and not g[5].any()
    assert np.abs(g - hr.g_of_counts(ideal, samples, type_counts, nbins, rmin, rmax, volume)).max() < 1e-14
    assert np.abs(analyze.g_of_counts(2.5 * ideal, samples, type_counts, edges, volume)[:5] - 2.5).max() < 1e-13
    with pytest.raises(ValueError, match="no samples"):
        analyze.g_of_counts(ideal, 0, type_counts, edges, volume)


# ---- pse_pair_hist_create and pse_pair_hist_accumulate on the device stand-in ------------------------------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """The host side of the library over the device stand-in of the sanitizer build, here without a sanitizer: its pse_create runs
    the real parameter rule and its histogram entry points the real validators."""
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_get_info", "pse_last_error", "pse_pair_hist_create", "pse_pair_hist_destroy",
                 "pse_pair_hist_accumulate", "pse_exclusions_create"):
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


def test_create_and_accumulate_refusals_on_the_stand_in(stub):
    from pse_amd import _lib
    n = 6
    h = stub_handle(stub, n)
    info = _lib.pse_info()
    assert stub.pse_get_info(h, ctypes.byref(info)) == 0
    rcut = info.as_dict()["rcut"]
    assert RCUT < rcut < RCUT + 1e-4
    good = dict(n=n, types=np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32), ntypes=2, nbins=64, rmin=0.5, rmax=rcut)

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_pair_hist_create(hh, a["n"], vp(a["types"]), a["ntypes"], a["nbins"], a["rmin"], a["rmax"],
                                       ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_pair_hist_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    refused("null out", with_out=False)
    refused("null handle", hh=None)
    refused("n = 0", n=0)
    refused("n = 7", n=7)
    refused("n = 7", n=7, types=None)
    refused("ntypes = 0", ntypes=0)
    refused("ntypes = 9", ntypes=9)
    refused("type 2", types=np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32))
    refused("type 1", ntypes=1, nbins=CAP)
    refused("nbins = 0", nbins=0)
    refused("nbins = -4", nbins=-4)
    refused("8193", ntypes=1, types=None, nbins=CAP + 1)
    refused("8193 counters", nbins=2731)                                        # 3 x 2731
    refused("8208 counters", ntypes=8, nbins=228)                               # 36 x 228
    refused("finite", rmin=np.nan)
    refused("finite", rmax=np.inf)
    refused("negative", rmin=-0.5)
    refused("must exceed", rmax=0.5)
    refused("must exceed", rmin=2.0, rmax=1.0)
    refused("rcut", rmax=rcut * (1.0 + 1e-12))
    refused("hydrodynamic cutoff", rmax=rcut * (1.0 + 1e-12))
    slab = stub_handle(stub, n, L=40.0, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    refused("slab rank", hh=slab, rmax=3.0)
    # the caps themselves, rmax = rcut, no types
    made = []
    for kw in (dict(), dict(nbins=2730), dict(ntypes=1, types=None, nbins=CAP), dict(ntypes=3, nbins=1365), dict(ntypes=8, nbins=227),
               dict(types=None, nbins=1, rmin=0.0)):
        rc, g = create(**kw)
        assert rc == 0 and g.value, (kw, stub.pse_last_error())
        made.append(g)
    g = made[0]

    # the call.  Any non-null, 8-byte aligned address will do for the arrays: the stand-in reads none of them
    other = stub_handle(stub, n)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex, ex_other = ctypes.c_void_p(), ctypes.c_void_p()
    assert stub.pse_exclusions_create(h, n, 1, vp(pairs), ctypes.byref(ex)) == 0
    assert stub.pse_exclusions_create(other, n, 1, vp(pairs), ctypes.byref(ex_other)) == 0
    buf = np.zeros(8)
    X = vp(buf)

    def call(word, gg=g, pos=X, N=n, counts=X, e=None):
        rc = stub.pse_pair_hist_accumulate(gg, pos, None, N, counts, e)
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg and "pse_pair_hist_accumulate" in msg), (word, rc, msg)

    call("null histogram", gg=None)
    call("N = 0", N=0)
    call("N = 7", N=n + 1)
    call("null pos", pos=None)
    call("null counts", counts=None)
    call("8-byte aligned", counts=ctypes.c_void_p(buf.ctypes.data + 4))
    call("another handle", e=ex_other)
    call(None, e=ex)
    call(None)
    call(None, N=1)
    for g in made[1:]:
        assert stub.pse_pair_hist_destroy(g) == 0
    assert stub.pse_pair_hist_destroy(None) == 0
    for hh in (h, other, slab):                                                # the object still alive goes with its handle
        assert stub.pse_destroy(hh) == 0


# ---- analyze.RDF and engine.PairHistogram: what is checked before the device is touched ---------------------------------------------

class _NoDevice:
    """Stands where the integrator (or the engine) belongs: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


def test_rdf_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    types = [0, 1, 1, 0]
    named = ["A", "B", "B", "A"]
    cases = [
        ("at least one bin", dict(nbins=0, rmax=3.0)),
        ("rmin < rmax", dict(nbins=8, rmax=3.0, rmin=3.0)),
        ("rmin < rmax", dict(nbins=8, rmax=3.0, rmin=-0.1)),
        ("rmin < rmax", dict(nbins=8, rmax=float("inf"))),
        ("rmin < rmax", dict(nbins=8, rmax=float("nan"))),
        ("more than 8192", dict(nbins=8193, rmax=3.0)),
        ("more than 8192", dict(nbins=2731, rmax=3.0, types=types)),
        ("outside [1, 8]", dict(nbins=8, rmax=3.0, types=[0, 8])),
        ("non-negative", dict(nbins=8, rmax=3.0, types=[0, -1])),
        ("non-negative", dict(nbins=8, rmax=3.0, types=[])),
        ("non-negative", dict(nbins=8, rmax=3.0, types=[0.5, 1.0])),
        ("type_names", dict(nbins=8, rmax=3.0, types=named)),                                       # names without the list
        ("unknown type name 'C'", dict(nbins=8, rmax=3.0, types=["A", "C"], type_names=["A", "B"])),
        ("distinct strings", dict(nbins=8, rmax=3.0, types=named, type_names=["A", "A"])),
        ("distinct strings", dict(nbins=8, rmax=3.0, types=types, type_names=[0, 1])),
        ("one type", dict(nbins=8, rmax=3.0, type_names=["A", "B"])),
        ("period", dict(nbins=8, rmax=3.0, period=0)),
    ]
    for word, kw in cases:
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            analyze.RDF(_NoDevice(), **kw)
    # what goes to pse_pair_hist_create: names by their position in type_names, which may know more types than the particles show
    ty, ntypes, nbins, rmin, rmax, names, period = analyze._rdf_arguments(64, 3.0, 0.7, named, ["A", "B", "C"], 250)
    assert ty.tolist() == [0, 1, 1, 0] and ty.dtype == np.uint32 and (ntypes, nbins, rmin, rmax, names, period) == (3, 64, 0.7, 3.0, ["A", "B", "C"], 250)
    ty, ntypes, *_ = analyze._rdf_arguments(64, 3.0, 0.0, None, None, 1)
    assert ty is None and ntypes == 1
    ty, ntypes, *_ = analyze._rdf_arguments(64, 3.0, 0.0, np.array([2, 0, 0]), None, 1)
    assert ty.tolist() == [2, 0, 0] and ntypes == 3
    # the device object of the engine checks the same before it asks the engine for anything
    for word, args in (("outside [1, 8]", (None, 9, 8, 0.0, 3.0)), ("type 2 >= ntypes = 2", ([0, 2], 2, 8, 0.0, 3.0)),
                       ("more than 8192", (None, 8, 228, 0.0, 3.0)), ("at least one bin", (None, 1, 0, 0.0, 3.0))):
        with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
            engine.PairHistogram(_NoDevice(), *args)
    with pytest.raises(ValueError, match="not a bin edge"):
        analyze.edge_index(analyze.bin_edges(10, 0.0, 5.0), 2.6)
    assert analyze.edge_index(analyze.bin_edges(50, 0.0, 5.0), 2.6) == 26
