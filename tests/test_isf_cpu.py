"""The intermediate scattering functions without a GPU: the reference of tests/isf_ref.py against closed forms and its own
invariances; the float64 restatement of the kernel's order within half the bound on every case of the GPU tests; the dyadic cases
exact in shuffled orders; MSDSchedule.drop_origins against a brute-force list; the argument checks of the Python layers; and every
refusal of the pse_isf_* entry points in the stated order through the device stand-in of the sanitizer build
(pse_amd/csrc/asan_stub.cpp, which runs the real validators), built here without a sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import isf_ref as ir
import structure_factor_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SETS = ir.mode_sets()


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture
def extended():
    ir.need_extended_precision()


def lattice(n, box):
    """n points of a simple lattice that fits the box exactly: g^3 >= n sites at fractional coordinates (i, j, k) / g - 1/2."""
    g = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    i = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    return sr.from_fractional(i / g - 0.5, box), g


# ---- the reference against closed forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cubic", "tilted", "negative"])
def test_reference_on_a_rigidly_translated_lattice(name, extended):
    """Every particle moved by the same vector: self = N exp(-2 pi i m.ds), whatever the positions are."""
    box = sr.BOXES[name]
    org, _ = lattice(216, box)
    ds = np.array([[0.013, -0.27, 0.4]])
    now = org + sr.from_fractional(ds, box)
    modes = SETS["half3"]
    got = ir.self_part(now, org, box, modes)[0]
    want = 216 * np.exp(-2j * np.pi * (modes @ ds[0]))
    assert np.abs(got - want).max() <= 216 * 2e-14


def test_reference_lattice_mode_has_the_modulus_n(extended):
    """rho at a reciprocal vector of the lattice (a multiple of g in every index) is N in modulus; off the lattice it vanishes."""
    box = sr.TILTED
    pos, g = lattice(216, box)
    assert g == 6
    on, off = np.array([[6, 0, 0], [0, -12, 6], [6, 6, 6], [0, 0, 0]]), np.array([[1, 0, 0], [0, 2, 0], [3, 3, 1]])
    assert np.abs(np.abs(sr.rho(pos, box, on)[0]) - 216).max() <= 1e-10
    assert np.abs(sr.rho(pos, box, off)[0]).max() <= 1e-10
    # ... and the collective part of a rigid translation: rho(now) conj rho(org) = N^2 exp(-2 pi i m.ds) on the lattice modes
    ds = np.array([[0.05, 0.11, -0.3]])
    now = pos + sr.from_fractional(ds, box)
    coll = ir.coll_part(sr.rho(now, box, on), sr.rho(pos, box, on))[0, 0]
    assert np.abs(coll - 216 ** 2 * np.cos(2 * np.pi * (on @ ds[0]))).max() <= 1e-7


def test_reference_invariances(extended):
    """Lattice-vector moves of every particle, now and at the origin independently, and a relabelling of the particles."""
    box = sr.NEGATIVE
    now, org = ir.configuration("negative", 200)
    types = ir.types_of(200, 3)
    modes = SETS["half3"]
    base = ir.self_part(now, org, box, modes, types, 3)
    rng = np.random.default_rng(3)
    shift = lambda: rng.integers(-3, 4, size=(200, 3)).astype(np.float64) @ sr.lattice_vectors(box)   # noqa: E731
    moved_now, moved_org = now + shift(), org + shift()
    smax = ir.s_max(box, moved_now, moved_org)
    got = ir.self_part(moved_now, moved_org, box, modes, types, 3)
    counts = np.bincount(types, minlength=3)
    assert ir.worst_ratio(got, base, modes, counts, smax) <= 0.5      # (the float64 positions themselves moved by roundings)
    order = rng.permutation(200)
    again = ir.self_part(now[order], org[order], box, modes, types[order], 3)
    assert np.abs(again - base).max() <= 1e-12
    # self against itself is N_a, and the conjugate when now and origin change places
    assert np.array_equal(ir.self_part(now, now, box, modes, types, 3), counts[:, None] * np.ones(len(modes)))
    assert np.abs(ir.self_part(org, now, box, modes, types, 3) - base.conj()).max() <= 1e-12


# ---- the kernel's order in float64 ---------------------------------------------------------------------------------------------------

def test_plan_restates_the_segments():
    distinct, inverse, segs = ir.plan(SETS["duplicates"])
    assert len(distinct) == 5 and np.array_equal(distinct[inverse], SETS["duplicates"])
    # (-3, 2, -5) | (0, 0, 0), (3, -2, 5) | (4, -2, 5), (5, -2, 5): (0, 0, 0) is always a seed, and a run ends where the step changes
    assert [(f, ln) for f, ln, _ in segs] == [(0, 1), (1, 2), (3, 2)] and segs[1][2].tolist() == [3, -2, 5] and segs[2][2].tolist() == [1, 0, 0]
    distinct, _, segs = ir.plan(SETS["zline"])
    assert len(distinct) == 201 and [ln for _, ln, _ in segs] == [8] * 25 + [1] and all(d.tolist() == [0, 0, 1] for _, _, d in segs[:25])
    assert sum(ln for _, ln, _ in ir.plan(SETS["scattered128"])[2]) == len(np.unique(SETS["scattered128"], axis=0))


def test_the_reduced_product_is_the_fused_operation():
    """fma(m, ds, -rint(m ds)) against the exact value in extended precision, rounded once."""
    rng = np.random.default_rng(5)
    ds = rng.uniform(-1.0, 1.0, 4000)
    for m in (1, -3, 4096, -4095, 1237):
        exact = ir.LD(m) * ds.astype(ir.LD)                            # 13 + 53 bits: not exact in 64, so compare to an ulp
        want = (exact - np.rint(exact)).astype(np.float64)
        got = ir._reduced(m, ds)
        assert np.abs(got - want).max() <= 2.0 ** -53 and np.abs(got).max() <= 0.5 + 2.0 ** -50


@pytest.mark.parametrize("case", ir.general_cases(), ids=lambda c: c[0])
def test_the_kernel_order_keeps_half_the_bound(case, extended):
    want, counts = ir.case_reference(case)
    got, _ = ir.case_reference(case, ir.self_float64)
    ratio = ir.worst_ratio(got, want, ir.case_inputs(case)[3], counts)
    print(f"{case[0]}: float64 restatement, worst error / tol = {ratio:.4f}")
    assert ratio <= 0.5


@pytest.mark.parametrize("name", sorted(ir.DYADIC_BOXES))
def test_dyadic_cases_are_exact_in_every_order(name):
    """s, ds and m.ds are exact (the reference asserts it), every phasor is one of 1, -i, -1, i: the float64 restatement of the
    kernel's order equals the integer reference bit for bit, in the given and in shuffled particle orders, and after every particle
    has moved by its own lattice vector."""
    box = ir.DYADIC_BOXES[name]
    now, org = ir.dyadic_case(name, 300)
    types = ir.types_of(300, 3)
    rng = np.random.default_rng(7)
    for key in ("half3", "zline", "corners", "duplicates"):
        modes = SETS[key]
        want = ir.self_exact(now, org, box, modes, types, 3)
        # (the extended-precision reference is not exact here: its 2 pi is rounded, cos(pi / 2) is 3e-20 there)
        assert np.abs(want).max() > 20 and np.abs(want - ir.self_part(now, org, box, modes, types, 3)).max() <= 300 * 1e-18
        for _ in range(3):
            order = rng.permutation(300)
            assert np.array_equal(ir.self_float64(now[order], org[order], box, modes, types[order], 3), want)
        moved = now + rng.integers(-3, 4, size=(300, 3)).astype(np.float64) @ sr.lattice_vectors(box)
        assert np.array_equal(ir.self_exact(moved, org, box, modes, types, 3), want)
        assert np.array_equal(ir.self_float64(moved, org, box, modes, types, 3), want)
        r = ir.rho_exact(now, box, modes, types, 3)
        assert np.abs(r - sr.rho(now, box, modes, types, 3)).max() <= 300 * 1e-18


# ---- the schedule --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nlags,every", [(5, 1), (5, 2), (7, 3), (4, 4), (1, 1)])
def test_drop_origins_against_a_brute_force_list(nlags, every):
    """Origins are the samples that are multiples of origin_every; a drop before sample d forgets every origin < d.  Brute force:
    sample s meets origin o when o < s <= o + nlags and no drop lies in (o, s]."""
    from pse_amd import analyze
    drops = {6, 7, 13, 20}
    sch = analyze.MSDSchedule(nlags, every)
    plain = analyze.MSDSchedule(nlags, every)
    stored, met, met_plain = {}, [], []
    for s in range(30):
        if s in drops:
            sch.drop_origins()
            assert sch.live == {}

        def accumulate(slots, rows, s=s, out=met):
            for slot, row in zip(slots, rows):
                assert s - stored[slot] == row + 1                    # the slot still holds the origin that the row belongs to
                out.append((stored[slot], s))
        sch.sample(accumulate, lambda slot, s=s: stored.__setitem__(slot, s))
        plain.sample(lambda slots, rows, s=s: met_plain.extend((s - r - 1, s) for r in rows), lambda slot: None)
    want = [(o, s) for s in range(30) for o in range(0, s, every) if s - o <= nlags and not any(o < d <= s for d in drops)]
    assert sorted(met) == sorted(want) and len(set(met)) == len(met)
    counts = [sum(1 for o, s in want if s - o == lag) for lag in range(1, nlags + 1)]
    assert sch.counts == counts and sch.samples == 30
    # without a drop the schedule is what it was
    assert sorted(met_plain) == sorted((o, s) for s in range(30) for o in range(0, s, every) if s - o <= nlags)
    sch.reset()
    assert sch.pairs(nlags) == plain.pairs(nlags) and sch.samples == 0


# ---- the Python layers ---------------------------------------------------------------------------------------------------------------

class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


class _NoDeviceEngine(_NoDevice):
    n_max = 64


def test_python_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    modes = SETS["half3"]
    for word, kw in [("non-empty integer (nk, 3)", dict(modes=[[1, 2]], nlags=4)), ("beyond +-4096", dict(modes=[[0, 4097, 0]], nlags=4)),
                     ("more than 4096", dict(modes=np.zeros((4097, 3), dtype=int), nlags=4)),
                     ("nlags and origin_every", dict(modes=modes, nlags=0)), ("nlags and origin_every", dict(modes=modes, nlags=4, origin_every=0)),
                     ("more than 64", dict(modes=modes, nlags=130, origin_every=2)), ("period", dict(modes=modes, nlags=4, period=0)),
                     ("one type", dict(modes=modes, nlags=4, type_names=["A", "B"])),
                     ("unknown type name", dict(modes=modes, nlags=4, types=["A", "C"], type_names=["A", "B"])),
                     ("both off", dict(modes=modes, nlags=4, self_part=False, collective=False))]:
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)").replace("+", r"\+")):
            analyze.IntermediateScattering(_NoDevice(), **kw)
    for word, args in (("ntypes = 9", (None, 9, modes, 4)), ("norigins = 0", (None, 1, modes, 0)), ("norigins = 65", (None, 1, modes, 65)),
                       ("more than 4096", (None, 1, np.zeros((4097, 3), dtype=int), 4)), ("non-empty integer", (None, 1, np.zeros((0, 3), dtype=int), 4)),
                       ("type", (np.array([0, 2]), 2, modes, 4))):
        with pytest.raises(ValueError, match=word):
            engine.ScatteringOrigins(_NoDeviceEngine(), *args)


# ---- the entry points on the device stand-in ------------------------------------------------------------------------------------------

NAMES = ("pse_isf_create", "pse_isf_destroy", "pse_isf_sample", "pse_isf_store", "pse_isf_correlate")


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
    modes = np.ascontiguousarray(SETS["half3"][:20], dtype=np.int32)
    good = dict(n=n, types=np.array([0, 1] * 7, dtype=np.uint32), ntypes=2, nk=len(modes), modes=modes, norigins=3)

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_isf_create(hh, a["n"], vp(a["types"]), a["ntypes"], a["nk"], vp(a["modes"]), a["norigins"],
                                 ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_isf_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    far = modes.copy(); far[7, 1] = -4097
    bad = good["types"].copy(); bad[5] = 2
    big = np.zeros((4097, 3), dtype=np.int32)
    # every refusal with a LATER fault planted next to it: the earlier one is what is reported
    refused("null out", with_out=False, hh=None)
    refused("null handle", hh=None, n=0)
    refused("n = 0", n=0, ntypes=0)
    refused("n = 15", n=15, ntypes=0)
    refused("ntypes = 0", ntypes=0, nk=0)
    refused("ntypes = 9", ntypes=9, nk=0)
    refused("nk = 0", nk=0, modes=None)
    refused("nk = 4097 outside [1, 4096]", nk=4097, modes=None)
    refused("null modes_host", modes=None, types=bad)
    refused("mode 7 has the index my = -4097", modes=far, types=bad)
    refused("type 2", types=bad, norigins=0)
    refused("norigins = 0", norigins=0)
    refused("norigins = 65", norigins=65)
    refused("norigins = -1", norigins=-1)
    rc, f = create(modes=big[:4096], nk=4096, types=None, ntypes=1)                # the cap itself is allowed
    assert rc == 0 and f.value, stub.pse_last_error()
    assert stub.pse_isf_destroy(f) == 0
    rc, f = create()
    assert rc == 0 and f.value, stub.pse_last_error()
    # the device calls: the arrays are device pointers, which the stand-in never follows
    buf = np.zeros(64)
    at = lambda off=0: ctypes.c_void_p(buf.ctypes.data + off)   # noqa: E731
    assert buf.ctypes.data % 8 == 0
    i32 = lambda *v: np.array(v, dtype=np.int32)   # noqa: E731
    slots, rows = i32(0, 1), i32(0, 1)
    s03, s13, s10, s02, s00, s20, r05, r11 = i32(0, 3), i32(1, 3), i32(1, 0), i32(0, 2), i32(0, 0), i32(2, 0), i32(0, 5), i32(1, 1)

    def check(fn, cases):
        for word, args in cases:
            assert getattr(stub, fn)(*args) == INVALID, (word, args)
            msg = stub.pse_last_error().decode()
            assert word in msg and fn in msg, (word, msg)

    # before any sample: store and correlate refuse
    check("pse_isf_store", (("null scattering object", (None, 9)), ("slot = 3 outside", (f, 3)), ("slot = -1 outside", (f, -1)),
                            ("no pse_isf_sample since create", (f, 0))))
    check("pse_isf_correlate", (("null scattering object", (None, 0, None, None, 0, None, None)),
                                ("no pse_isf_sample since create", (f, 0, None, None, 0, None, None))))
    check("pse_isf_sample", (("null scattering object", (None, None, None, 0, at(4), None)), ("N = 0 outside", (f, None, None, 0, at(4), None)),
                             ("N = 15 outside", (f, None, None, 15, at(4), None)), ("null pos", (f, None, None, n, at(4), None)),
                             ("rho =", (f, at(), None, n, at(4), at(4))), ("static_sums =", (f, at(), None, n, at(), at(4)))))
    assert stub.pse_isf_sample(f, at(), None, n, None, None) == 0, stub.pse_last_error()          # both NULL is legal
    assert stub.pse_isf_store(f, 0) == 0, stub.pse_last_error()
    assert stub.pse_isf_sample(f, at(), None, n - 1, at(), at()) == 0, stub.pse_last_error()      # another N
    assert stub.pse_isf_store(f, 2) == 0, stub.pse_last_error()
    assert stub.pse_isf_sample(f, at(), None, n, None, at()) == 0, stub.pse_last_error()          # slot 0 has this N, slot 2 has not
    check("pse_isf_correlate",
          (("npairs = 0", (f, 0, None, None, 0, None, None)), ("npairs = 65", (f, 65, None, None, 0, None, None)),
           ("null slots_host", (f, 2, None, None, 0, None, None)), ("null rows_host", (f, 2, vp(slots), None, 0, None, None)),
           ("nrows = 0", (f, 2, vp(s03), vp(rows), 0, None, None)),
           ("pair 1 names the slot 3 outside", (f, 2, vp(s13), vp(rows), 1, None, None)),
           ("pair 0 names the slot 1, which was never stored", (f, 2, vp(s10), vp(r05), 2, None, None)),
           ("pair 0 names the slot 2, stored with N = 13: the current sample has N = 14", (f, 2, vp(s20), vp(r05), 2, None, None)),
           ("pair 1 names the slot 2, stored with N = 13", (f, 2, vp(s02), vp(r05), 2, None, None)),
           ("pair 1 names the row 5 outside", (f, 2, vp(s00), vp(r05), 2, None, None)),
           ("pairs 0 and 1 both name the row 1", (f, 2, vp(s00), vp(r11), 2, None, None)),
           ("self and coll are both null", (f, 2, vp(s00), vp(rows), 2, None, None)),
           ("self =", (f, 2, vp(s00), vp(rows), 2, at(4), at(4))),
           ("coll =", (f, 2, vp(s00), vp(rows), 2, at(), at(4)))))
    assert stub.pse_isf_correlate(f, 2, vp(s00), vp(rows), 2, at(), None) == 0, stub.pse_last_error()   # one slot for two rows
    assert stub.pse_isf_correlate(f, 1, vp(s00), vp(rows), 2, None, at()) == 0, stub.pse_last_error()
    assert not buf.any()                                                             # nothing was written through any pointer
    assert stub.pse_isf_destroy(f) == 0 and stub.pse_isf_destroy(None) == 0
    rc, f = create()                                                                 # still alive below: it goes with its handle
    assert rc == 0
    assert stub.pse_destroy(h) == 0
