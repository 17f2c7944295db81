"""CPU tests of the bond-orientational order that need no device: the O(N^2) reference the GPU tests compare to
(tests/bond_order_ref.py) on the ideal shells, on periodic perfect lattices and under rotations and permutations; its harmonics
(scipy) and the kernel's recurrence, restated in float64 NumPy, against mpmath.spherharm at 40 digits, with the bound derived from the
order of the operations; the pure functions of analyze.BondOrder against brute force; the refusals of the three entry points, in the
documented order, through the device stand-in of the sanitizer build (pse_amd/csrc/asan_stub.cpp, which runs the real validators),
built here without a sanitizer; and the argument checks of analyze.BondOrder that come before the device is touched."""
import ctypes
import functools
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

import bond_order_ref as br
from test_pair_hist_cpu import stub_handle, _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
RCUT = 5.2565                                   # just below sqrt(-ln 1e-3) / 0.5 = 5.25652...


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def esc(word):
    return word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")


# ---- the reference ---------------------------------------------------------------------------------------------------------------

TABLE = {   # shell: {l: q_l} to six decimals, and the closed forms that are known
    "sc": ({4: 0.763763, 6: 0.353553}, {4: math.sqrt(7 / 12), 6: math.sqrt(1 / 8)}),
    "fcc": ({4: 0.190941, 6: 0.574524, 8: 0.403915, 12: 0.600083}, {4: math.sqrt(7 / 192), 6: math.sqrt(169 / 512)}),
    "hcp": ({4: 0.097222, 6: 0.484762}, {4: 7 / 72}),
    "bcc8": ({4: 0.509175, 6: 0.628539}, {4: math.sqrt(7 / 27), 6: math.sqrt(32 / 81)}),
    "bcc14": ({4: 0.036370, 6: 0.510688}, {}),
}


def shell_q_exact(shell, l):
    """q_l of an ideal shell from mpmath.spherharm at 40 digits, the unit vectors formed at that precision (hcp: the irrational
    coordinates themselves, not their float64 values)."""
    mpmath.mp.dps = 40
    mp = mpmath.mpf
    if shell == "hcp":
        h, c = mpmath.sqrt(3) / 2, mpmath.sqrt(mp(2) / 3)
        half = mp(1) / 2
        vectors = ([(mp(1), mp(0), mp(0)), (mp(-1), mp(0), mp(0)), (half, h, mp(0)), (-half, h, mp(0)), (half, -h, mp(0)), (-half, -h, mp(0))]
                   + [(sx * half, h / 3, sz * c) for sx in (1, -1) for sz in (1, -1)] + [(mp(0), -2 * h / 3, sz * c) for sz in (1, -1)])
    else:
        vectors = [tuple(mp(float(v)) for v in d) for d in br.SHELLS[shell]]
    total = mp(0)
    for m in range(l + 1):
        acc = mpmath.mpc(0)
        for x, y, z in vectors:
            acc += mpmath.spherharm(l, m, mpmath.acos(z / mpmath.sqrt(x * x + y * y + z * z)), mpmath.atan2(y, x))
        total += (1 if m == 0 else 2) * abs(acc / len(vectors)) ** 2
    return float(mpmath.sqrt(4 * mpmath.pi / (2 * l + 1) * total))


@pytest.mark.parametrize("shell", sorted(TABLE))
def test_ideal_shells(shell):
    vectors = br.SHELLS[shell]
    assert len(vectors) == {"sc": 6, "fcc": 12, "hcp": 12, "bcc8": 8, "bcc14": 14}[shell]
    r = np.sqrt((vectors ** 2).sum(axis=1))
    assert np.allclose(r[: 8 if shell == "bcc14" else None], r[0], rtol=0, atol=1e-15)
    decimals, closed = TABLE[shell]
    assert abs(br.shell_q(vectors, 2)) < 1e-12                                                   # q_2 vanishes on all of them
    for l, v in decimals.items():
        assert abs(br.shell_q(vectors, l) - v) < 5.1e-7, (shell, l)
    for l, v in closed.items():
        assert abs(br.shell_q(vectors, l) - v) < 1e-12, (shell, l)
    for l in decimals:                                                                           # every entry of the table at 40 digits
        exact = shell_q_exact(shell, l)
        assert abs(exact - decimals[l]) < 5.1e-7 and abs(br.shell_q(vectors, l) - exact) < 1e-12, (shell, l, exact)
    for l in br.DEGREES:                                                                         # the restated recurrence gives the same shells
        mine = float(br.norm(br.kernel_terms(vectors, l).mean(axis=0)))
        assert abs(mine - br.shell_q(vectors, l)) < br.bound(l, len(vectors))


def test_one_neighbour_has_q_one_and_none_has_zero(oracle):
    box = (10.0, 10.0, 10.0, 0.0)
    pos = np.array([[0.0, 0.0, 0.0], [0.3, -1.1, 0.7], [4.0, 4.0, -4.0]])
    ref = br.bond_order(pos, box, None, 1, 2.0, (2, 4, 6, 8, 10, 12)[:4], oracle, solid=(4, 0.5, 1))
    assert ref["nnb"].tolist() == [1, 1, 0] and ref["nbmax"] == 1
    assert np.allclose(ref["q"][:2], 1.0, rtol=0, atol=1e-13) and not ref["q"][2].any() and not ref["qbar"][2].any()
    assert np.allclose(ref["qbar"][:2], 1.0, rtol=0, atol=1e-13)                                  # even l: C_lm(-d) = C_lm(d)
    assert ref["nconn"].tolist() == [1, 1, 0] and ref["stats"].tolist() == [[3, 2]]
    assert abs(ref["s"][(0, 1)] - 1.0) < 1e-13 and abs(ref["rmin"] - math.sqrt(0.09 + 1.21 + 0.49)) < 1e-15


@pytest.mark.parametrize("lattice", ["sc", "fcc"])
def test_periodic_perfect_lattice(lattice, oracle):
    """On a periodic perfect lattice every particle sees the same shell: q-bar_l = q_l, and s_ij = 1 for every bond."""
    if lattice == "sc":
        pos, box, rnb, nb = br.sc_lattice(4, 2.0), (8.0, 8.0, 8.0, 0.0), 2.5, 6
    else:
        pos, box, rnb, nb = br.fcc_lattice(3, 4.0), (12.0, 12.0, 12.0, 0.0), 3.4, 12              # first shell 2.83, second 4
    ref = br.bond_order(pos, box, None, 1, rnb, (4, 6), oracle, solid=(6, 0.7, nb))
    assert (ref["nnb"] == nb).all() and ref["clear"][0] > 0.3
    closed = TABLE[lattice][1]
    for col, l in enumerate((4, 6)):
        assert np.abs(ref["q"][:, col] - closed[l]).max() < 1e-12 and np.abs(ref["qbar"][:, col] - ref["q"][:, col]).max() < 1e-12
    assert max(abs(v - 1.0) for v in ref["s"].values()) < 1e-12 and len(ref["s"]) == nb * len(pos)
    assert (ref["nconn"] == nb).all() and ref["stats"].tolist() == [[len(pos), len(pos)]]


def test_rotation_and_permutation_invariance(oracle):
    rng = np.random.default_rng(4)
    box = (40.0, 40.0, 40.0, 0.0)
    pos = rng.uniform(-4.0, 4.0, size=(120, 3))                                                  # a cluster clear of the boundary
    types = rng.integers(0, 2, 120)
    rnb, degrees, solid = [2.6, 2.2, 3.0], (4, 6, 12), (6, 0.3, 3)
    a = br.bond_order(pos, box, types, 2, rnb, degrees, oracle, solid=solid)
    br.assert_clear(a["clear"])
    assert a["nbmax"] > 8 and 0 < a["stats"][:, 1].sum() < 120
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    b = br.bond_order(pos @ rot.T, box, types, 2, rnb, degrees, oracle, solid=solid)
    assert np.array_equal(a["nnb"], b["nnb"]) and np.array_equal(a["nconn"], b["nconn"]) and np.array_equal(a["stats"], b["stats"])
    assert np.abs(a["q"] - b["q"]).max() < 1e-12 and np.abs(a["qbar"] - b["qbar"]).max() < 1e-12
    perm = rng.permutation(120)
    c = br.bond_order(pos[perm], box, types[perm], 2, rnb, degrees, oracle, solid=solid)
    assert np.array_equal(c["nnb"], a["nnb"][perm]) and np.array_equal(c["nconn"], a["nconn"][perm]) and np.array_equal(a["stats"], c["stats"])
    assert np.abs(c["q"] - a["q"][perm]).max() < 1e-13 and np.abs(c["qbar"] - a["qbar"][perm]).max() < 1e-13
    relabel = br.bond_order(pos, box, 1 - types, 2, rnb[::-1], degrees, oracle, solid=solid)       # A <-> B with their distances
    assert np.array_equal(relabel["stats"], a["stats"][::-1]) and np.array_equal(relabel["nnb"], a["nnb"])


def test_exclusions_groups_and_switches(oracle):
    rng = np.random.default_rng(6)
    box = (14.0, 11.0, 17.0, 0.3)
    pos = rng.uniform(-0.5, 0.5, size=(80, 3)) * np.array(box[:3])
    types = rng.integers(0, 2, 80)
    full = br.bond_order(pos, box, types, 2, 3.0, (4,), oracle)
    (i, j, _), _, _ = br.neighbours(pos, box, types, 2, 3.0, oracle)
    assert np.array_equal(np.bincount(i, minlength=80), np.bincount(j, minlength=80))              # the relation is symmetric
    off = br.bond_order(pos, box, types, 2, {(0, 0): 3.0, (1, 1): 3.0}, (4,), oracle)              # A-B off: exactly those neighbours go
    cross = np.bincount(i[types[i] != types[j]], minlength=80)
    assert np.array_equal(off["nnb"], full["nnb"] - cross) and cross.sum() > 0
    excl = np.stack([i[:10], j[:10]], axis=1)
    cut = br.bond_order(pos, box, types, 2, 3.0, (4,), oracle, excl=excl)
    assert cut["nnb"].sum() < full["nnb"].sum() and cut["nnb"].sum() >= full["nnb"].sum() - 20
    members = np.arange(0, 80, 3)
    sub = br.bond_order(pos[members], box, types[members], 2, 3.0, (4,), oracle, excl=excl, ids=members)
    assert sub["stats"][:, 0].sum() == len(members)


# ---- the harmonics and the kernel's recurrence against 40 digits ------------------------------------------------------------------------

def directions():
    rng = np.random.default_rng(12)
    d = rng.normal(size=(150, 3)) * rng.uniform(0.5, 3.0, size=(150, 1))
    axes = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 2.5], [1e-9, 0, -1.0], [0, 1e-160, 1.0]], dtype=float)
    return np.concatenate([d, axes])


@functools.lru_cache(maxsize=None)
def exact(L):
    """C_Lm of the float64 separation vectors of directions(), their unit vectors formed at 40 digits: (n, L + 1) complex."""
    mpmath.mp.dps = 40
    out = []
    for d in directions():
        x, y, z = (mpmath.mpf(float(v)) for v in d)
        theta, phi = mpmath.acos(z / mpmath.sqrt(x * x + y * y + z * z)), mpmath.atan2(y, x)
        f = mpmath.sqrt(4 * mpmath.pi / (2 * L + 1))
        out.append([complex(f * mpmath.spherharm(L, m, theta, phi)) for m in range(L + 1)])
    return np.array(out)


@pytest.mark.parametrize("L", br.DEGREES)
def test_reference_harmonics_against_mpmath(L):
    err = np.abs(br.harmonics(directions(), L) - exact(L)).max()
    print(f"l = {L}: scipy against 40 digits {err:.3e}")
    assert err < 2e-14 * (L + 1)
    assert np.abs(np.abs(exact(L)[-9:-7, 0]) - 1.0).max() < 1e-15 and np.abs(exact(L)[-9:-7, 1:]).max() < 1e-30      # the poles: C_l0 = 1 alone


@pytest.mark.parametrize("L", br.DEGREES)
def test_kernel_recurrence_against_mpmath(L):
    """The arithmetic of k_bond_order_c for one term, restated in float64 NumPy (bond_order_ref.kernel_terms), against 40 digits on 150
    random separation vectors of length 0.5 to 3, the six axes and three near-pole vectors.  Largest error of a component seen,
    l = 2, 4, 6, 8, 10, 12: 5.6e-16, 1.4e-15, 3.0e-15, 4.9e-15, 6.4e-15, 7.7e-15 (scipy's own: 5.6e-16 to 2.7e-15); the derived per-component bound term_bound(l) is
    8.0e-15, 2.8e-14, 8.9e-14, 3.4e-13, 1.6e-12, 8.2e-12 (its recurrence part is a majorant that grows with |a_lm z| <= sqrt(2l - 1)
    per step, the measured error does not).  The bound must hold with at least four times room; it is the tolerance of the GPU tests."""
    diff = br.kernel_terms(directions(), L) - exact(L)
    err = max(np.abs(diff.real).max(), np.abs(diff.imag).max())
    print(f"l = {L}: recurrence against 40 digits {err:.3e}, bound {br.term_bound(L):.3e} ({br.term_units(L):.1f} u from the recurrence)")
    assert 4.0 * err <= br.term_bound(L)
    assert br.bound(L, 20) >= br.term_bound(L) and br.bound(L, 20, averaged=True) > br.bound(L, 20) > br.bound(L, 10)
    assert br.bound(L, 20, dpos=1e-14) > br.bound(L, 20)
    assert br.bound(12, 40) < 1e-9                                                                # still a test of fp64 arithmetic


def test_recurrence_constants_and_start_values():
    from math import factorial
    for m in range(13):
        dfact = math.prod(range(2 * m - 1, 0, -2)) if m else 1
        assert abs(br.start(m) - (-1) ** m * dfact / math.sqrt(factorial(2 * m))) < 4e-16
    z = np.array([-1.0, -0.3, 0.0, 0.5, 1.0])
    for L in br.DEGREES:                                                                         # m = 0: the Legendre polynomial itself
        assert np.abs(br.legendre_row(z, L)[:, 0] - np.polynomial.legendre.Legendre.basis(L)(z)).max() < 1e-14


# ---- the pure functions of analyze.BondOrder ---------------------------------------------------------------------------------------------

def test_analyzer_functions_against_brute_force():
    from pse_amd import analyze
    rng = np.random.default_rng(5)
    values = rng.uniform(0.0, 1.0, 4000)
    counts = br.histogram(values, np.zeros(4000, dtype=int), 1, 100, 0.0, 1.0)[0]
    assert counts.sum() == 4000 and np.array_equal(counts, np.histogram(values, bins=100, range=(0.0, 1.0))[0])
    assert abs(analyze.histogram_mean(counts, 0.0, 1.0) - values.mean()) <= 0.5 / 100
    centres = (np.arange(100) + 0.5) / 100
    assert abs(analyze.histogram_mean(counts, 0.0, 1.0) - (counts * centres).sum() / 4000) < 1e-15
    hi = analyze.BOND_ORDER_HI                                                                   # the analyzer's own bins
    assert hi == 1.0 + 2.0 ** -26 and abs(analyze.histogram_mean(br.histogram(values, np.zeros(4000, dtype=int), 1, 100, 0.0, hi)[0])
                                          - (counts * centres).sum() / 4000 * hi) < 1e-15
    assert analyze.histogram_mean([0, 0, 4, 0], 0.0, 2.0) == 1.25
    rows = rng.integers(0, 50, size=(7, 3, 2))
    rows[..., 0] += 50
    assert abs(analyze.solid_fraction_of(rows) - rows[..., 1].sum() / rows[..., 0].sum()) < 1e-15
    for a in range(3):
        assert abs(analyze.solid_fraction_of(rows, a) - sum(r[a, 1] for r in rows) / sum(r[a, 0] for r in rows)) < 1e-15
    assert analyze.solid_fraction_of([[[4, 1]]]) == 0.25
    for f, arg in ((analyze.histogram_mean, (np.zeros(8),)), (analyze.solid_fraction_of, (np.zeros((0, 1, 2)),))):
        with pytest.raises(ValueError, match="no samples"):
            f(*arg)
    # the planted edges of the binning contract
    planted = np.array([0.0, np.nextafter(1.0, 0.0), 1.0, np.nan, -1e-300, 0.5])
    got = br.histogram(planted, np.array([0, 1, 0, 0, 1, 1]), 2, 4, 0.0, 1.0)
    assert got.tolist() == [[1, 0, 0, 0], [0, 0, 1, 1]]


def test_the_analyzers_bins_keep_a_particle_with_one_neighbour():
    """One neighbour: q_l = 1 up to rounding, and the kernel's arithmetic puts it AT OR ABOVE 1 about as often as below.  Bins that end
    at 1 would drop those particles (pse_bond_order_histogram counts lo <= v < hi); the analyzer's end at BOND_ORDER_HI, which is above
    1 + the error bound of every degree, so all of them land in the last bin."""
    from pse_amd import analyze
    d = np.random.default_rng(3).normal(size=(20000, 3))
    for L in br.DEGREES:
        q = br.norm(br.kernel_terms(d, L))
        above = int((q >= 1.0).sum())
        print(f"l = {L}: {above} of 20000 single-neighbour q at or above 1, largest excess {q.max() - 1.0:.2e}")
        assert 2000 < above < 18000 and q.max() - 1.0 <= br.bound(L, 1) < analyze.BOND_ORDER_HI - 1.0
        ends_at_one = br.histogram(q, np.zeros(20000, dtype=int), 1, 100, 0.0, 1.0)
        kept = br.histogram(q, np.zeros(20000, dtype=int), 1, 100, 0.0, analyze.BOND_ORDER_HI)
        assert ends_at_one.sum() == 20000 - above and kept.sum() == 20000 == kept[0, 99]
    assert max(br.bound(L, 60, br.separation_error((20.0, 20.0, 20.0), 0.01), averaged=True) for L in br.DEGREES) < analyze.BOND_ORDER_HI - 1.0


def test_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    ty, nt, rnb, deg = engine._bond_order_arguments([0, 2, 1], 3, {(2, 0): 1.5, (1, 1): 2.5}, (6, 4))
    assert nt == 3 and deg.tolist() == [6, 4] and deg.dtype == np.int32 and rnb.tolist() == br.rlink_array({(2, 0): 1.5, (1, 1): 2.5}, 3).tolist()
    assert engine._bond_order_arguments(None, 1, 3.0, [12])[2].tolist() == [3.0]
    for word, args in (("outside [1, 8]", (None, 9, 1.0, (4,))), ("type 2 >= ntypes = 2", ([0, 2], 2, 1.0, (4,))), ("3 entries", ([0, 1], 2, [1.0, 2.0], (4,))),
                       ("rnb must be finite", (None, 1, float("nan"), (4,))), ("not negative", (None, 1, -1.0, (4,))),
                       ("every pair type is off: rnb", (None, 1, 0.0, (4,))), ("rnb key", ([0, 1], 2, {(0, 2): 1.0}, (4,))),
                       ("1 to 4 integers", (None, 1, 1.0, ())), ("1 to 4 integers", (None, 1, 1.0, (2, 4, 6, 8, 10))),
                       ("1 to 4 integers", (None, 1, 1.0, (4.0,))), ("degree 5", (None, 1, 1.0, (5,))), ("degree 14", (None, 1, 1.0, (4, 14))),
                       ("degree 0", (None, 1, 1.0, (0,))), ("twice", (None, 1, 1.0, (4, 6, 4)))):
        with pytest.raises(ValueError, match=esc(word)):
            engine.BondOrderShells(_NoDevice(), *args)
    named = ["A", "B", "B", "A"]
    for word, kw in (("every pair type is off", dict(rnb=0.0)), ("period", dict(rnb=1.0, period=0)), ("nbins", dict(rnb=1.0, nbins=0)),
                     ("nbins", dict(rnb=1.0, nbins=8193)), ("capacity", dict(rnb=1.0, capacity=0)), ("type_names", dict(rnb=1.0, types=named)),
                     ("unknown type name 'C'", dict(rnb={("A", "C"): 1.0}, types=named, type_names=["A", "B"])),
                     ("twice", dict(rnb={("A", "B"): 1.0, ("B", "A"): 2.0}, types=named, type_names=["A", "B"])),
                     ("a pair", dict(rnb={"A": 1.0}, types=named, type_names=["A", "B"])), ("finite", dict(rnb=float("nan"))),
                     ("degree 3", dict(rnb=1.0, degrees=(3,))), ("solid must be", dict(rnb=1.0, solid=(6, 0.7))),
                     ("not among the degrees", dict(rnb=1.0, solid=(8, 0.7, 7))), ("threshold", dict(rnb=1.0, solid=(6, 1.5, 7))),
                     ("threshold", dict(rnb=1.0, solid=(6, float("nan"), 7))), ("min_conn", dict(rnb=1.0, solid=(6, 0.7, -1)))):
        with pytest.raises(ValueError, match=esc(word)):
            analyze.BondOrder(_NoDevice(), **kw)
    got = analyze._bond_order_analyzer_arguments({("B", "A"): 1.5}, (6, 4), named, ["A", "B"], 3, (6, 0.7, 7), 50, 16)
    assert got[0].tolist() == [0, 1, 1, 0] and got[1] == 2 and got[2].tolist() == [0.0, 1.5, 0.0] and got[3].tolist() == [6, 4]
    assert got[4:] == (["A", "B"], 3, (6, 0.7, 7), 50, 16)


# ---- the three entry points on the device stand-in ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """The host side of the library over the device stand-in of the sanitizer build, here without a sanitizer, as
    tests/test_clusters_cpu.py builds it."""
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_get_info", "pse_last_error", "pse_bond_order_create", "pse_bond_order_destroy",
                 "pse_bond_order_compute", "pse_bond_order_histogram", "pse_exclusions_create"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


def test_refusals_of_the_three_entry_points_on_the_stand_in(stub):
    from pse_amd import _lib
    n = 6
    h = stub_handle(stub, n)
    info = _lib.pse_info()
    assert stub.pse_get_info(h, ctypes.byref(info)) == 0
    rcut = info.as_dict()["rcut"]
    assert RCUT < rcut < RCUT + 1e-4
    ints = lambda *v: np.array(v, dtype=np.int32)   # noqa: E731
    good = dict(n=n, types=np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32), ntypes=2, rnb=np.array([1.5, 0.0, rcut]), nl=2, degrees=ints(4, 6))

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_bond_order_create(hh, a["n"], vp(a["types"]), a["ntypes"], vp(a["rnb"]), a["nl"], vp(a["degrees"]),
                                        ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_bond_order_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    refused("null out", with_out=False)
    refused("null handle", hh=None)
    refused("n = 0", n=0)
    refused("n = 7", n=7)
    refused("ntypes = 0", ntypes=0)
    refused("ntypes = 9", ntypes=9)
    refused("null rnb_host", rnb=None)
    refused("not finite", rnb=np.array([1.5, np.nan, 1.0]))
    refused("not finite", rnb=np.array([np.inf, 0.0, 1.0]))
    refused("negative", rnb=np.array([1.5, 0.0, -1.0]))
    refused("pair type 2 has rnb", rnb=np.array([1.5, 0.0, rcut * (1.0 + 1e-12)]))
    refused("hydrodynamic cutoff", rnb=np.array([6.0, 0.0, 0.0]))
    refused("every pair type is off", rnb=np.zeros(3))
    refused("type 2", types=np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32))
    refused("nl = 0", nl=0)
    refused("nl = 5", nl=5, degrees=ints(2, 4, 6, 8, 10))
    refused("null degrees_host", degrees=None)
    refused("degree 1 = 5", degrees=ints(4, 5))
    refused("degree 0 = 14", degrees=ints(14, 4))
    refused("degree 0 = 0", degrees=ints(0, 4))
    refused("degree 1 = -2", degrees=ints(4, -2))
    refused("listed twice", degrees=ints(6, 6))
    # the order: the shared arguments first, in the order of pse_clusters_create, then the degrees
    refused("n = 7", n=7, ntypes=9, rnb=None, nl=0)
    refused("ntypes = 9", ntypes=9, rnb=None, nl=0)
    refused("null rnb_host", rnb=None, nl=0)
    refused("every pair type is off", rnb=np.zeros(3), types=np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32), nl=0)
    refused("type 2", types=np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32), nl=0)
    refused("nl = 0", nl=0, degrees=None)
    refused("null degrees_host", degrees=None, nl=3)
    refused("degree 1 = 5", nl=3, degrees=ints(4, 5, 4))
    made = []
    for kw in (dict(), dict(types=None, ntypes=1, rnb=np.array([rcut])), dict(ntypes=8, rnb=np.full(36, 1.0)),
               dict(nl=4, degrees=ints(12, 2, 8, 10)), dict(nl=1, degrees=ints(6, 6))):
        rc, b = create(**kw)
        assert rc == 0 and b.value, (kw, stub.pse_last_error())
        made.append(b)
    b = made[0]

    # compute.  Any non-null, 8-byte aligned address will do for the arrays: the stand-in reads none of them
    other = stub_handle(stub, n)
    slab = stub_handle(stub, n, L=40.0, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    rc, bslab = create(hh=slab)
    assert rc == 0, stub.pse_last_error()
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex, ex_other = ctypes.c_void_p(), ctypes.c_void_p()
    assert stub.pse_exclusions_create(h, n, 1, vp(pairs), ctypes.byref(ex)) == 0
    assert stub.pse_exclusions_create(other, n, 1, vp(pairs), ctypes.byref(ex_other)) == 0
    buf = np.zeros(8)
    X, odd = vp(buf), ctypes.c_void_p(buf.ctypes.data + 4)
    outputs = ("nnb", "q", "qbar", "nconn", "stats")
    none = {k: None for k in outputs}

    def compute(word, bb=b, pos=X, N=n, nnb=X, q=X, qbar=X, sd=1, thr=0.7, mc=7, nconn=X, stats=X, e=None):
        rc = stub.pse_bond_order_compute(bb, pos, None, N, nnb, q, qbar, sd, thr, mc, nconn, stats, e)
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg and "pse_bond_order_compute" in msg), (word, rc, msg)

    compute("null bond-order object", bb=None)
    compute("N = 0", N=0)
    compute("N = 7", N=n + 1)
    compute("null pos", pos=None)
    compute("all null", **none)
    compute("solid_degree = 2", sd=2)
    compute("solid_degree = -2", sd=-2)
    compute("threshold = nan", thr=float("nan"))
    compute("threshold = inf", thr=float("inf"))
    compute("threshold = 1.5", thr=1.5)
    compute("threshold = -1.01", thr=-1.01)
    compute("stats is not 8-byte aligned", stats=odd)
    compute("another handle", e=ex_other)
    compute("slab rank", bb=bslab)
    # the order
    compute("N = 7", N=n + 1, pos=None, **none)
    compute("null pos", pos=None, sd=5, **none)
    compute("all null", sd=5, thr=9.0, **none)
    compute("solid_degree = 5", sd=5, thr=9.0, stats=odd)
    compute("threshold = 9", thr=9.0, stats=odd, e=ex_other)
    compute("stats is not 8-byte aligned", stats=odd, e=ex_other)
    compute("another handle", bb=bslab, e=ex)                                   # the exclusions before the slab rank
    compute("null pos", bb=bslab, pos=None)
    compute(None, e=ex)
    compute(None)
    compute(None, N=1)
    compute(None, sd=-1, thr=float("nan"))                                     # the threshold means nothing without a solid pass
    compute(None, sd=0, thr=-1.0, mc=0)
    compute(None, sd=1, thr=1.0)
    for only in outputs:                                                       # each output alone will do
        compute(None, **{k: None for k in outputs if k != only})

    def hist(word, bb=b, values=X, column=1, N=n, nbins=100, lo=0.0, hi=1.0, counts=X):
        rc = stub.pse_bond_order_histogram(bb, values, column, None, N, nbins, lo, hi, counts)
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg and "pse_bond_order_histogram" in msg), (word, rc, msg)

    hist("null bond-order object", bb=None)
    hist("N = 0", N=0)
    hist("N = 7", N=n + 1)
    hist("null values", values=None)
    hist("column = 2", column=2)
    hist("column = -1", column=-1)
    hist("nbins = 0", nbins=0)
    hist("2 types x 4097 bins", nbins=4097)
    hist("must be finite", lo=float("nan"))
    hist("must be finite", hi=float("inf"))
    hist("must exceed", lo=1.0, hi=1.0)
    hist("must exceed", lo=1.0, hi=0.5)
    hist("null counts", counts=None)
    hist("counts is not 8-byte aligned", counts=odd)
    hist("N = 7", N=n + 1, values=None, column=9)                               # the order
    hist("null values", values=None, column=9, nbins=0)
    hist("column = 9", column=9, nbins=0)
    hist("nbins = 0", nbins=0, lo=float("nan"))
    hist("bins", nbins=4097, lo=float("nan"))
    hist("must be finite", lo=float("nan"), counts=None)
    hist("must exceed", hi=0.0, counts=None)
    hist(None)
    hist(None, nbins=4096)
    hist(None, bb=made[1], column=0, nbins=8192)
    hist(None, bb=bslab)                                                       # it reads no cell list: a slab rank will do
    hist(None, lo=-2.0, hi=-1.0, column=0, N=1)
    for b in made[1:]:
        assert stub.pse_bond_order_destroy(b) == 0
    assert stub.pse_bond_order_destroy(None) == 0
    for hh in (h, other, slab):                                                # the objects still alive go with their handles
        assert stub.pse_destroy(hh) == 0
