"""The chain normal modes without a GPU: the exact reference of tests/chain_modes_ref.py against closed forms, mpmath and its own
invariances; pse_host_rouse_weights against mpmath, its exact symmetries, zeros and refusals; the float64 restatement of the kernels'
order against the exact reference within the bounds that the device is held to, on the cases of the GPU tests; the NumPy helper
relaxation_time_of; the schedule; the argument checks of the Python layers; and every refusal of the pse_chain_modes_* entry points
through the device stand-in of the sanitizer build (pse_amd/csrc/asan_stub.cpp, which runs the real validators and the real layout),
built here without a sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import conformation_cases as cc
import chain_modes_ref as cm

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


def host_weights(lib, m, K):
    out = np.full((K, m), np.nan)
    assert lib.pse_host_rouse_weights(m, K, vp(out)) == 0, lib.pse_last_error()
    return out


# ---- the reference against closed forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,b", [(2, 0.5), (9, 0.75), (40, 1.25)])
def test_reference_on_a_straight_rod(m, b):
    """A rod r_q = r_0 + q b e along (1, 2, -2) / 3 across the box's faces: u_q = q b e, so X_p = b e (1/m) sum_q q cos(pi p (2 q + 1) /
    (2 m)) -- for p >= 1, with t = pi p / (2 m), the closed form -b cos t / (2 m sin^2 t) for odd p and 0 for even p (half the derivative
    of sum_q sin((2 q + 1) t) = sin^2(m t) / sin t) --, against mpmath at 40 digits."""
    import mpmath
    mpmath.mp.dps = 40
    n, bonds, _, _ = cc.build([("chain", m)])
    e = np.array([1.0, 2.0, -2.0]) / 3.0
    pos = cc.wrap(np.array([30.0, -31.0, 5.0]) + np.arange(m)[:, None] * b * e, BOX)
    K = min(m, 6)
    ref = cm.reference(pos, BOX, bonds, {m: cm.rouse_weights(m, K)})
    assert ref["modes"].shape == (1, K, 3)
    scale = np.abs(b * e) * m
    placed = 2 * m * cc.EPS * 64.0              # the beads are rounded where they lie (|r| < 32): every u_q is off by up to this
    assert np.all(np.abs(ref["modes"][0, 0] - (m - 1) * b * e) <= placed + 8 * cc.EPS * scale)      # R
    for p in range(1, K):
        t = mpmath.pi * p / (2 * m)
        want = mpmath.mpf(0) if p % 2 == 0 else -mpmath.mpf(b) * mpmath.cos(t) / (2 * m * mpmath.sin(t) ** 2)
        # (the weights are rounded cosines: m terms of relative error EPS, and the positions are the rounded rod)
        assert np.all(np.abs(ref["modes"][0, p] - float(want) * e) <= placed + 8 * m * cc.EPS * scale), p


def test_reference_on_the_dimer():
    """m = 2 across the box: R = u_1, X_1 = (cos(pi / 4) u_0 + cos(3 pi / 4) u_1) / 2 = -u_1 / (2 sqrt 2)."""
    pos = np.array([[31.5, 0.0, 0.0], [-31.25, 0.25, 0.0]])                   # u_1 = (1.25, 0.25, 0)
    ref = cm.reference(pos, BOX, [[0, 1]], {2: cm.rouse_weights(2, 2)})
    assert np.array_equal(ref["modes"][0, 0], [1.25, 0.25, 0.0])
    assert np.allclose(ref["modes"][0, 1], -np.array([1.25, 0.25, 0.0]) / (2.0 * np.sqrt(2.0)), rtol=4 * cc.EPS, atol=0.0)
    assert np.array_equal(ref["lin_mol"], [0]) and np.array_equal(ref["lin_size"], [2])


def test_reference_is_invariant_under_translation_relabelling_and_reversal():
    """A common translation moves X_{p >= 1} by (sum_q w_q) t only -- the rounding of the weights' sum --, and not at all here, where
    the offsets are bond sums; a permutation of the caller indices that keeps the lower end changes nothing; reversing the chain gives
    (-1)^p X_p and -R; and the static sums equal the lag-0 correlation of a buffer with itself."""
    rng = np.random.default_rng(5)
    m, K = 24, 8
    n, bonds, _, _ = cc.build([("chain", m), ("ring", 5), ("chain", m)])
    box = (16.0, 16.0, 16.0, 0.25)
    pos = cc.place(n, bonds, box, rng, 2.5)
    tables = {m: cm.rouse_weights(m, K)}
    ref = cm.reference(cc.wrap(pos, box), box, bonds, tables)
    assert list(ref["lin_mol"]) == [0, 2] and list(ref["nlin_type"]) == [2]
    shifted = cm.reference(cc.wrap(pos + np.array([3.1, -7.7, 0.3]), box), box, bonds, tables)
    tol = 64 * m * cc.EPS * 16.0 * np.abs(tables[m]).sum(axis=1)[None, :, None]      # (the positions themselves are re-rounded)
    assert np.all(np.abs(shifted["modes"] - ref["modes"]) <= tol)
    assert np.all(np.abs(tables[m][1:].sum(axis=1)) <= m * cc.EPS)                    # sum_q w_{p,q} = 0 up to rounding
    b2, new_of_old = cc.relabel(n, bonds, rng)
    p2 = np.empty_like(pos); p2[new_of_old] = pos
    again = cm.reference(cc.wrap(p2, box), box, b2, tables)
    lower_kept = [min(new_of_old[0], new_of_old[m - 1]) == new_of_old[0], min(new_of_old[m + 5], new_of_old[n - 1]) == new_of_old[m + 5]]
    sign = np.array([1.0 if kept else -1.0 for kept in lower_kept])[:, None, None]
    flip = np.where(sign > 0, 1.0, np.array([-1.0] + [(-1.0) ** p for p in range(1, K)])[None, :, None])
    assert np.array_equal(again["modes"], ref["modes"] * flip)
    rev = np.arange(n); rev[:m] = rev[:m][::-1]                                     # the first chain reversed in the caller's order
    p3 = np.empty_like(pos); p3[rev] = pos
    back = cm.reference(cc.wrap(p3, box), box, rev[np.asarray(bonds)], tables)
    parity = np.array([-1.0] + [(-1.0) ** p for p in range(1, K)])[:, None]
    # (reversed, the offsets are counted from the other end: X'_p = (-1)^p X_p - u_{m-1} sum_q w_{p,q}, the sum zero up to rounding)
    slack = 2.5 * m * np.abs(tables[m].sum(axis=1))[:, None] + 4 * cc.EPS * np.abs(ref["modes"][0])
    assert np.array_equal(back["modes"][0, 0], -ref["modes"][0, 0]) and np.all(np.abs(back["modes"][0] - ref["modes"][0] * parity) <= slack)
    assert np.array_equal(back["modes"][1], ref["modes"][1])
    own = cm.correlate(ref, ref, 1)
    for c, (i, b) in enumerate(cm.COLS):
        assert np.array_equal(own[:, :, i, b], ref["sums"][:, :, c]) and np.array_equal(own[:, :, b, i], ref["sums"][:, :, c])


# ---- pse_host_rouse_weights -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [2, 3, 20, 63, 64, 257, 1024])
def test_host_rouse_weights_against_mpmath(lib, m):
    """Within 1 ulp of cos(pi p (2 q + 1) / (2 m)) / m from mpmath; row 0 is (-1, 0, ..., 0, +1); w_{p,m-1-q} = (-1)^p w_{p,q} bit for
    bit; an odd multiple of pi / 2 gives exactly +0.0."""
    K = min(m, 32)
    w, want = host_weights(lib, m, K), cm.rouse_weights(m, K)
    assert np.array_equal(w[0], want[0])
    assert np.all(np.abs(w - want) <= np.spacing(np.abs(want)))
    for p in range(1, K):
        assert np.array_equal(w[p, ::-1], (-1.0) ** p * w[p]), p               # (equal magnitudes bit for bit; a zero is +0.0, below)
        zero = (p * (2 * np.arange(m) + 1)) % (2 * m) == m
        assert np.array_equal(w[p][zero].view(np.uint64), np.zeros(int(zero.sum()), dtype=np.uint64)) and not np.any(w[p][~zero] == 0.0)
    if m == 20:
        assert np.any((np.outer(np.arange(1, K), 2 * np.arange(m) + 1) % (2 * m)) == m)   # (the zeros are met: p = 4, q = 2)


def test_host_rouse_weights_refusals(lib):
    out = np.full((40, 40), 7.0)
    for word, args in (("null out", (8, 3, None)), ("m = 1", (1, 1, vp(out))), ("m = 0", (0, 1, vp(out))), ("nmodes = 0", (8, 0, vp(out))),
                       ("nmodes = 33", (40, 33, vp(out))), ("nmodes = -2", (8, -2, vp(out))), ("nmodes - 1 = 8", (8, 9, vp(out)))):
        assert lib.pse_host_rouse_weights(*args) == INVALID
        msg = lib.pse_last_error().decode()
        assert word in msg and "pse_host_rouse_weights" in msg, (word, msg)
    assert np.all(out == 7.0)                                                    # nothing is written after a refusal
    assert lib.pse_host_rouse_weights(8, 8, vp(out)) == 0                         # nmodes - 1 = 7 < m


# ---- the kernels' order against the exact reference -------------------------------------------------------------------------------------

def _within(name, box, n, bonds, pos, types, ntypes, tables):
    ref = cm.reference(pos, box, bonds, tables, types, ntypes)
    modes, sums = cm.kernel_order(pos, box, bonds, tables, types, ntypes)
    tX = cm.bounds(ref, box)
    ntiles = len(cm.tiles_of(ref["mols"])[0]) - 1
    ts = cm.sums_bound(ref, tX, ntypes, ntiles)
    ex, es = np.abs(modes - ref["modes"]), np.abs(sums - ref["sums"])
    print(name, "modes: largest error / bound", (ex / np.maximum(tX, 1e-300)).max(), "sums:", (es / np.maximum(ts, 1e-300)).max())
    assert np.all(ex <= tX) and np.all(es <= ts)
    # the correlation of the call with the positions moved a little: the same chains, other X
    pos2 = cc.wrap(pos + np.random.default_rng(1).uniform(-0.05, 0.05, pos.shape), box)
    ref2 = cm.reference(pos2, box, bonds, tables, types, ntypes)
    modes2, _ = cm.kernel_order(pos2, box, bonds, tables, types, ntypes)
    exact = cm.correlate(ref, ref2, ntypes)
    tc = cm.correlate_bound(ref, tX, ref2, cm.bounds(ref2, box), ntypes, exact)
    ec = np.abs(cm.kernel_correlate(modes, modes2, ref["lin_type"], ntypes) - exact)
    print(name, "corr: largest error / bound", (ec / np.maximum(tc, 1e-300)).max())
    assert np.all(ec <= tc)
    return ref


@pytest.mark.parametrize("k", range(len(cc.EDGES)))
def test_the_kernel_order_keeps_the_bound_at_the_wave_and_tile_edges(k):
    """The cases of the GPU test: the float64 restatement of the documented order stays within the bound of the exact value, so the
    margin of the GPU test is known before a GPU sees it."""
    box, n, bonds, pos, types, ntypes, tables = cm.edge(k)
    ref = _within(f"edge {k}", box, n, bonds, pos, types, ntypes, tables)
    assert sorted(set(ref["lin_size"].tolist())) == [2, 3, 63, 64, 65, 255, 257, 1023]
    kinds = cc.build(cc.EDGE_SHAPES, gaps=(2, 0, 1, 0, 0, 3))[3]
    assert len(ref["lin_mol"]) == kinds.count("chain") and len(ref["mols"]) == len(kinds)   # rings, the star and the comb are skipped


@pytest.mark.parametrize("name", cm.GENERAL_NAMES)
def test_the_kernel_order_keeps_the_bound_on_the_other_general_cases(name):
    box, n, bonds, pos, types, ntypes, tables = cm.general(name)
    ref = _within(name, box, n, bonds, pos, types, ntypes, tables)
    assert ref["K"] == {"1024 and dimers": 9, "K=32": 32, "K=1": 1}[name]


@pytest.mark.parametrize("name", cm.DYADIC_NAMES)
def test_dyadic_cases_are_exact_in_every_order(name):
    """The reference asserts that no sum can round; the restated order then gives its bits, static sums and self-correlation."""
    box, n, bonds, pos, types, ntypes, tables = cm.dyadic(name)
    ref = cm.reference(pos, box, bonds, tables, types, ntypes, dyadic=True)
    assert 0 < ref["headroom"] < 2 ** 53
    assert all(np.all(np.abs(2.0 * w) == np.round(np.abs(2.0 * w))) and np.abs(w).max() <= 1.0 for w in tables.values())
    modes, sums = cm.kernel_order(pos, box, bonds, tables, types, ntypes)
    assert np.array_equal(modes, ref["modes"]) and np.array_equal(sums, ref["sums"])
    if len(ref["lin_mol"]) <= 1024 and ref["lin_size"].max() <= 64:
        own = cm.correlate(ref, ref, ntypes, dyadic=True)
        assert np.array_equal(cm.kernel_correlate(modes, modes, ref["lin_type"], ntypes), own)


# ---- the NumPy helpers and the Python layers --------------------------------------------------------------------------------------------

def test_relaxation_time_of_on_exponentials():
    from pse_amd import analyze
    t = np.arange(0.0, 40.0, 2.0)
    for tau in (0.7, 3.0, 5.5, 17.25):
        assert np.isclose(analyze.relaxation_time_of(t, np.exp(-t / tau)), tau, rtol=1e-12), tau
    assert np.isnan(analyze.relaxation_time_of(t, np.exp(-t / 100.0)))              # never falls to 1/e within the lags
    assert np.isnan(analyze.relaxation_time_of(t, np.ones(t.shape[0])))
    c = np.exp(-t / 3.0); c[2:] = -0.25                                             # a crossing into negative values: linear in c
    assert np.isclose(analyze.relaxation_time_of(t, c), 2.0 + 2.0 * (c[1] - np.exp(-1.0)) / (c[1] + 0.25), rtol=1e-12)
    c = np.exp(-t / 3.0); c[1] = np.nan                                             # a lag without origins is stepped over
    assert np.isnan(analyze.relaxation_time_of(t[:2], c[:2]))
    with pytest.raises(ValueError, match="one length"):
        analyze.relaxation_time_of(t, np.ones(3))


def test_the_schedule_serves_the_analyzer_through_its_public_methods():
    """What RouseModes relies on: a slot is overwritten only after its origin met its last lag, and counts follow."""
    from pse_amd import analyze
    sch = analyze.MSDSchedule(5, 2)
    assert sch.norigins == 3
    stored, met = {}, []
    for s in range(9):
        def accumulate(slots, rows, s=s):
            for slot, row in zip(slots, rows):
                assert s - stored[slot] == row + 1                               # the row is the lag - 1 of the slot's origin
                met.append((stored[slot], row + 1))
        sch.sample(accumulate, lambda slot, s=s: stored.__setitem__(slot, s))
    assert len(set(met)) == len(met) and sorted(met) == sorted((o, l) for o in range(0, 9, 2) for l in range(1, 6) if o + l <= 8)
    assert sch.samples == 9 and sch.counts == [4, 4, 3, 3, 2]


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


class _NoDeviceEngine(_NoDevice):
    n_max = 64


def test_python_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    bonds = cc.build([("chain", 6), ("chain", 4), ("star", 4)], gaps=(1,))[1]
    for word, kw in [("non-empty integer (nbonds, 2)", dict(bonds=[[0, 1, 2]])), ("no molecule", dict(bonds=[[2, 2]])),
                     ("period", dict(bonds=bonds, period=0)), ("3 molecules", dict(bonds=bonds, molecule_types=[0, 1])),
                     ("one type", dict(bonds=bonds, type_names=["A", "B"])), ("nmodes = 0", dict(bonds=bonds, nmodes=0)),
                     ("nmodes = 32", dict(bonds=bonds, nmodes=32)),
                     ("nmodes = 4 needs chains of more than 4 members, the smallest linear molecule has 4", dict(bonds=bonds, nmodes=4)),
                     ("no linear molecule", dict(bonds=cc.star(0, 5))), ("nlags and origin_every", dict(bonds=bonds, nmodes=3, nlags=0)),
                     ("more than 64", dict(bonds=bonds, nmodes=3, nlags=130, origin_every=2))]:
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
            analyze.RouseModes(_NoDevice(), **kw)
    w6, w4 = np.zeros((3, 6)), np.zeros((3, 4))
    for word, args in (("ntypes = 9", (bonds, [4, 6], [w4, w6], None, 9)), ("3 molecules", (bonds, [4, 6], [w4, w6], [0, 1], 2)),
                       ("ascending", (bonds, [6, 4], [w6, w4])), ("2 tables", (bonds, [4], [w4, w6])),
                       ("the shape (3, 6)", (bonds, [4, 6], [w6, w6])), ("K in [1, 32]", (bonds, [4, 6], [np.zeros((33, 4)), np.zeros((33, 6))])),
                       ("not finite", (bonds, [4, 6], [w4, np.full((3, 6), np.inf)])), ("norigins = 65", (bonds, [4, 6], [w4, w6], None, 1, 65)),
                       ("norigins = -1", (bonds, [4, 6], [w4, w6], None, 1, -1))):
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            engine.ChainModes(_NoDeviceEngine(), *args)
    mol_of, nmol, sizes, linear = analyze.linear_molecules_of(16, bonds)
    assert nmol == 3 and sizes.tolist() == [6, 4, 4] and linear.tolist() == [True, True, False]


# ---- the entry points on the device stand-in --------------------------------------------------------------------------------------------

NAMES = ("pse_chain_modes_create", "pse_chain_modes_destroy", "pse_chain_modes_counts", "pse_chain_modes_compute", "pse_chain_modes_store",
         "pse_chain_modes_correlate")


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
    n = 14
    h = stub_handle(stub, n)
    # a trimer, a dimer, a triangle and a 4-chain: linear sizes 2, 3 and 4
    pairs = np.array([[0, 1], [1, 2], [4, 5], [7, 8], [8, 9], [9, 7], [10, 11], [11, 12], [12, 13]], dtype=np.uint32)
    K = 2
    good = dict(n=n, nbonds=len(pairs), pairs=pairs, types=np.array([0, 1, 1, 0], dtype=np.uint32), ntypes=2, nmodes=K, nsizes=3,
                sizes=np.array([2, 3, 4], dtype=np.uint32), weights=np.arange(K * 9, dtype=np.float64), norigins=3)

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_chain_modes_create(hh, a["n"], a["nbonds"], vp(a["pairs"]), vp(a["types"]), a["ntypes"], a["nmodes"], a["nsizes"],
                                         vp(a["sizes"]), vp(a["weights"]), a["norigins"], ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_chain_modes_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    def bonds(*rows):
        return np.array(rows, dtype=np.uint32)

    def sizes(*v):
        return np.array(v, dtype=np.uint32)

    bad_w = good["weights"].copy(); bad_w[2 * K + 1 * 3 + 2] = np.nan             # size 3, row 1, rank 2
    # every refusal with a LATER fault planted next to it: the earlier one is what is reported
    refused("null out", with_out=False, hh=None)
    refused("null handle", hh=None, n=0)
    refused("n = 0", n=0, nbonds=0)
    refused("n = 15", n=15, nbonds=0)
    refused("nbonds = 0", nbonds=0, pairs=None)
    refused("null pairs_host", pairs=None, ntypes=0)
    refused("bond 1 = (1, 14) has an endpoint >= n = 14", pairs=bonds((0, 1), (1, 14), (3, 3)), nbonds=3, ntypes=0)
    refused("the bond (1, 2) is listed twice", pairs=bonds((1, 2), (4, 5), (2, 1)), nbonds=3, ntypes=0)
    refused("ntypes = 0", ntypes=0, nmodes=0)
    refused("ntypes = 9", ntypes=9, nmodes=0)
    refused("molecule 1 has type 2 >= ntypes = 2", types=np.array([0, 2, 1, 0], dtype=np.uint32), nmodes=0)
    refused("nmodes = 0", nmodes=0, norigins=-1)
    refused("nmodes = 33", nmodes=33, norigins=65)
    refused("norigins = -1", norigins=-1, pairs=bonds((7, 8), (8, 9), (9, 7)), nbonds=3, types=None, ntypes=1)
    refused("norigins = 65", norigins=65, nsizes=0)
    refused("none of the 1 molecules is linear", pairs=bonds((7, 8), (8, 9), (9, 7)), nbonds=3, types=None, ntypes=1, nsizes=0)
    refused("nsizes = 0", nsizes=0, sizes=None)
    refused("null sizes_host", sizes=None, weights=None)
    refused("null weights_host", weights=None, sizes=sizes(2, 3, 5))
    refused("sizes_host[2] = 5 is not", sizes=sizes(2, 3, 5), weights=bad_w)
    refused("sizes_host[0] = 3 is not", sizes=sizes(3, 2, 4), weights=bad_w)           # not ascending
    refused("4 is missing", sizes=sizes(2, 3), nsizes=2, weights=bad_w)
    refused("sizes_host[3] = 6 is not", sizes=sizes(2, 3, 4, 6), nsizes=4, weights=np.zeros(K * 15))
    refused("size 3, row 1, rank 2 is nan", weights=bad_w)
    inf_w = good["weights"].copy(); inf_w[0] = np.inf
    refused("size 2, row 0, rank 0 is inf", weights=inf_w)
    rc, m = create()
    assert rc == 0 and m.value, stub.pse_last_error()
    rc, m0 = create(norigins=0, types=None, ntypes=1)
    assert rc == 0 and m0.value, stub.pse_last_error()
    # pse_chain_modes_counts: the real layout behind the stand-in
    nmol, nlin, nty = ctypes.c_uint(77), ctypes.c_uint(77), np.full(2, 77, np.uint32)
    lin_mol, lin_size = np.full(3, 77, np.uint32), np.full(3, 77, np.uint32)
    assert stub.pse_chain_modes_counts(m, ctypes.byref(nmol), ctypes.byref(nlin), vp(nty), vp(lin_mol), vp(lin_size)) == 0
    assert nmol.value == 4 and nlin.value == 3 and nty.tolist() == [2, 1] and lin_mol.tolist() == [0, 1, 3] and lin_size.tolist() == [3, 2, 4]
    assert stub.pse_chain_modes_counts(m0, None, ctypes.byref(nlin), None, None, None) == 0 and nlin.value == 3
    for word, args in (("null chain-modes object", (None, ctypes.byref(nmol), None, None, None, None)), ("all null", (m, None, None, None, None, None))):
        assert stub.pse_chain_modes_counts(*args) == INVALID
        assert word in stub.pse_last_error().decode() and "pse_chain_modes_counts" in stub.pse_last_error().decode()
    # the device calls: the arrays are device pointers, which the stand-in never follows
    buf = np.zeros(64)
    at = lambda off=0: ctypes.c_void_p(buf.ctypes.data + off)   # noqa: E731
    assert buf.ctypes.data % 8 == 0
    i32 = lambda *v: np.array(v, dtype=np.int32)   # noqa: E731
    slots, rows = i32(0, 1), i32(0, 1)
    s03, s13, s10, s02, s00, r05, r11 = i32(0, 3), i32(1, 3), i32(1, 0), i32(0, 2), i32(0, 0), i32(0, 5), i32(1, 1)   # (kept alive)

    def check(fn, who, cases):
        for word, args in cases:
            assert getattr(stub, fn)(*args) == INVALID, (word, args)
            msg = stub.pse_last_error().decode()
            assert word in msg and who in msg, (word, msg)

    # before any compute: store and correlate refuse
    check("pse_chain_modes_store", "pse_chain_modes_store",
          (("null chain-modes object", (None, 0)), ("norigins = 0", (m0, 9)), ("slot = 3 outside", (m, 3)), ("slot = -1 outside", (m, -1)),
           ("no pse_chain_modes_compute since create", (m, 0))))
    check("pse_chain_modes_correlate", "pse_chain_modes_correlate",
          (("null chain-modes object", (None, 0, None, None, 0, None)), ("norigins = 0", (m0, 0, None, None, 0, None)),
           ("no pse_chain_modes_compute since create", (m, 0, None, None, 0, None))))
    check("pse_chain_modes_compute", "pse_chain_modes_compute",
          (("null chain-modes object", (None, None, at(4), None, None)), ("null pos", (m, None, at(4), None, None)),
           ("modes =", (m, at(), at(4), at(4), None)), ("sums =", (m, at(), at(), at(4), at(4))), ("sample =", (m, at(), None, None, at(4)))))
    assert stub.pse_chain_modes_compute(m, at(), None, None, None) == 0, stub.pse_last_error()      # all three NULL is legal
    assert stub.pse_chain_modes_compute(m0, at(), at(), at(), at()) == 0, stub.pse_last_error()
    assert stub.pse_chain_modes_store(m, 0) == 0 and stub.pse_chain_modes_store(m, 2) == 0, stub.pse_last_error()
    check("pse_chain_modes_correlate", "pse_chain_modes_correlate",
          (("norigins = 0", (m0, 1, vp(slots), vp(rows), 2, at())), ("npairs = 0", (m, 0, None, None, 0, None)),
           ("npairs = 65", (m, 65, None, None, 0, None)), ("null slots_host", (m, 2, None, None, 0, None)),
           ("null rows_host", (m, 2, vp(slots), None, 0, None)), ("nrows = 0", (m, 2, vp(s03), vp(rows), 0, None)),
           ("pair 1 names the slot 3 outside", (m, 2, vp(s13), vp(rows), 1, None)),
           ("pair 0 names the slot 1, which was never stored", (m, 2, vp(s10), vp(r05), 2, None)),
           ("pair 1 names the row 5 outside", (m, 2, vp(s02), vp(r05), 2, None)),
           ("pairs 0 and 1 both name the row 1", (m, 2, vp(s02), vp(r11), 2, None)),
           ("null corr", (m, 2, vp(s00), vp(rows), 2, None)),
           ("corr =", (m, 2, vp(s02), vp(rows), 2, at(4)))))
    assert stub.pse_chain_modes_correlate(m, 2, vp(s00), vp(rows), 2, at()) == 0, stub.pse_last_error()
    assert not buf.any()                                                             # nothing was written through any pointer
    assert stub.pse_chain_modes_destroy(m0) == 0 and stub.pse_chain_modes_destroy(None) == 0
    assert stub.pse_destroy(h) == 0                                                  # m is still alive: it goes with its handle
