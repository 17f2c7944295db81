"""CPU tests of the typed pair tables that need no device: the O(N^2) reference the GPU tests compare to (tests/pair_typed_ref.py)
against a decomposition into runs of the already validated plain reference (tests/pair_table_ref.py); pse_host_typed_table_layout
through ctypes against its NumPy restatement, with every refusal; the refusals of pse_typed_table_create and pse_pair_table_typed
through the device stand-in of the sanitizer build (pse_amd/csrc/asan_stub.cpp, which runs the real validators), built here
without a sanitizer; and the argument checks of forces.TypedTablePair that come before the device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pair_table_ref
import pair_typed_ref as tr
from pair_table_ref import harmonic_table, morse_table, random_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
CAP = 3584
CUBIC = (14.0, 14.0, 14.0, 0.0)                 # the boxes of tests/test_gpu_pair_table.py
TILTED = (14.0, 11.0, 17.0, 0.3)
MORSE = dict(D=5.0, alpha=2.0, r0=1.5)
A, B, C = 0, 1, 2


def three_type_tables():
    """Five of the six pair types of three particle types on, each with a range of its own; B-B is off."""
    return {(A, A): (morse_table(rmin=0.7, rmax=3.0, width=1000, **MORSE), 0.7, 3.0),
            (B, A): (harmonic_table(40.0, 2.0, 1024), 0.0, 2.0),
            (A, C): (morse_table(rmin=1.0, rmax=2.8, width=300, **MORSE), 1.0, 2.8),
            (C, B): (harmonic_table(25.0, 2.0, 257, rmin=0.5), 0.5, 2.0),
            (C, C): (morse_table(rmin=0.7, rmax=2.5, width=500, **MORSE), 0.7, 2.5)}


# ---- the reference of the GPU tests, by decomposition -----------------------------------------------------------------------------

@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
def test_reference_is_the_sum_of_plain_passes_over_the_pair_types(box, oracle):
    """For a == b the typed sums hold the plain pass over the particles of type a with the table aa; for a < b the plain pass with
    the table ab over the particles of both types less what it finds within either type."""
    n, ntypes = 200, 3
    pos = random_points(n, box, seed=11)
    types = np.random.default_rng(21).integers(0, ntypes, n)
    tables = three_type_tables()
    obs, F = tr.typed_observables(pos, box, types, ntypes, tables, oracle)
    counts = tr.pairs_in_range(pos, box, types, ntypes, tables, oracle)
    assert len(counts) == 5 and tr.pair_index(B, B, ntypes) not in counts
    assert min(counts.values()) >= 20, counts                                  # every pair type that is on has work
    below = tr.pairs_below_rmin(pos, box, types, ntypes, tables, oracle)
    assert max(below.values()) >= 1, below                                     # ... and some pair lies under an rmin
    want, wantF = np.zeros(8), np.zeros((n, 3))

    def plain(rows, key):
        table, rmin, rmax = tables[key]
        o, f = pair_table_ref.pair_observables(pos[rows], box, table, rmin, rmax, oracle)
        full = np.zeros((n, 3))
        full[rows] = f
        return o, full

    for key in tables:
        a, b = min(key), max(key)
        ra, rb = np.nonzero(types == a)[0], np.nonzero(types == b)[0]
        if a == b:
            o, f = plain(ra, key)
        else:
            both = np.sort(np.concatenate([ra, rb]))
            (o, f), (oa, fa), (ob, fb) = plain(both, key), plain(ra, key), plain(rb, key)
            o, f = o - oa - ob, f - fa - fb
        assert o[7] == counts[tr.pair_index(a, b, ntypes)]
        want += o
        wantF += f
    assert obs[7] == want[7] == sum(counts.values())
    assert np.abs(obs - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(F - wantF).max() <= 1e-12 * max(1.0, np.abs(wantF).max())
    assert np.abs(F).max() > 1.0 and np.abs(F.sum(axis=0)).max() <= 1e-10 * np.abs(F).max()
    # the B-B pairs in the range of any table do exist: switched on they would count
    on = dict(tables)
    on[(B, B)] = tables[(A, A)]
    assert tr.typed_observables(pos, box, types, ntypes, on, oracle)[0][7] > obs[7]


def test_reference_with_one_type_is_the_plain_reference(oracle):
    pos = random_points(200, TILTED, seed=11)
    table, rmin, rmax = three_type_tables()[(A, A)]
    obs, F = tr.typed_observables(pos, TILTED, np.zeros(200, dtype=int), 1, {(0, 0): (table, rmin, rmax)}, oracle)
    o, f = pair_table_ref.pair_observables(pos, TILTED, table, rmin, rmax, oracle)
    assert np.array_equal(obs, o) and np.array_equal(F, f)


# ---- pse_host_typed_table_layout ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pse_amd import build, _lib
    build.build_lib()
    return _lib.load()


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def layout(lib, ntypes, width, rmin, rmax):
    npt = max(1, ntypes * (ntypes + 1) // 2)
    width, rmin, rmax = np.asarray(width, dtype=np.int32), np.asarray(rmin, dtype=np.float64), np.asarray(rmax, dtype=np.float64)
    base, scale, rmax2, total = np.full(npt, -7, dtype=np.int32), np.full(npt, -7.0), np.full(npt, -7.0), ctypes.c_int(-7)
    rc = lib.pse_host_typed_table_layout(ntypes, vp(width), vp(rmin), vp(rmax), vp(base), vp(scale), vp(rmax2), ctypes.byref(total))
    return rc, base, scale, rmax2, total.value


@pytest.mark.parametrize("ntypes", range(1, 9))
def test_pair_type_index_walks_the_upper_triangle(ntypes):
    from pse_amd.engine import pair_type_index
    npt = ntypes * (ntypes + 1) // 2
    seen = [tr.pair_index(a, b, ntypes) for a in range(ntypes) for b in range(a, ntypes)]
    assert seen == list(range(npt))                                            # a bijection, row by row
    for a in range(ntypes):
        for b in range(ntypes):
            assert tr.pair_index(a, b, ntypes) == tr.pair_index(b, a, ntypes) == pair_type_index(a, b, ntypes) == pair_type_index(b, a, ntypes)


@pytest.mark.parametrize("ntypes", [1, 2, 3, 8])
def test_layout_matches_the_numpy_restatement(lib, ntypes):
    rng = np.random.default_rng(ntypes)
    npt = ntypes * (ntypes + 1) // 2
    width = rng.integers(2, CAP // npt, npt).astype(np.int32)
    width[rng.uniform(size=npt) < 0.3] = 0
    width[0] = 2                                                               # the smallest table; and not all off
    rmin = rng.uniform(0.0, 1.0, npt)
    rmax = rmin + rng.uniform(0.1, 3.0, npt)
    rmin[width == 0], rmax[width == 0] = np.nan, -1.0                          # an off pair type's range is not looked at
    rc, base, scale, rmax2, total = layout(lib, ntypes, width, rmin, rmax)
    assert rc == 0, lib.pse_last_error()
    rbase, rscale, rrmax2, rtotal = tr.layout_numpy(width, rmin, rmax)
    assert np.array_equal(base, rbase) and total == rtotal == int(width.sum())
    assert np.array_equal(base, np.concatenate([[0], np.cumsum(width)[:-1]]))    # off pair types take no room
    on = width > 0
    assert np.array_equal(scale[on], (width[on] - 1).astype(np.float64) / (rmax[on] - rmin[on]))     # bit for bit
    assert np.array_equal(rmax2[on], rmax[on] * rmax[on])
    assert np.array_equal(scale, rscale) and np.array_equal(rmax2, rrmax2)
    assert not scale[~on].any() and not rmax2[~on].any()


def test_layout_cap_and_refusals(lib):
    ok = lambda *a: layout(lib, *a)                                           # noqa: E731
    rc, base, _, _, total = ok(2, [2048, 1536, 0], [0.0] * 3, [1.0] * 3)
    assert rc == 0 and total == CAP and base.tolist() == [0, 2048, 3584]
    rc, base, scale, rmax2, total = ok(2, [2048, 1536, 2], [0.0] * 3, [1.0] * 3)
    assert rc == INVALID and "3586" in lib.pse_last_error().decode()
    rc, base, scale, rmax2, total = ok(2, [2048, 1537, 0], [0.0] * 3, [1.0] * 3)
    assert rc == INVALID and "3585" in lib.pse_last_error().decode() and str(CAP) in lib.pse_last_error().decode()
    assert total == -7 and np.all(base == -7) and np.all(scale == -7.0) and np.all(rmax2 == -7.0)      # a refused call writes nothing

    def bad(word, ntypes=2, width=(10, 0, 10), rmin=(0.0, 0.0, 0.5), rmax=(1.0, 0.0, 2.0)):
        rc = ok(ntypes, list(width), list(rmin), list(rmax))[0]
        msg = lib.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_host_typed_table_layout" in msg, (word, msg)

    bad("ntypes = 0", ntypes=0)
    bad("ntypes = 9", ntypes=9)
    bad("width 1", width=(10, 1, 10))
    bad("width -3", width=(10, -3, 10))
    bad("width 2049", width=(10, 0, 2049))
    bad("all widths are zero", width=(0, 0, 0))
    bad("finite", rmin=(np.nan, 0.0, 0.5))
    bad("finite", rmax=(1.0, 0.0, np.inf))
    bad("negative", rmin=(0.0, 0.0, -0.5))
    bad("must exceed", rmax=(1.0, 0.0, 0.5))
    bad("must exceed", rmin=(1.0, 0.0, 0.5))
    w, lo, hi = np.array([4], dtype=np.int32), np.zeros(1), np.ones(1)
    o_i, o_d, t = np.zeros(1, dtype=np.int32), np.zeros(1), ctypes.c_int(0)
    for args in ((None, vp(lo), vp(hi), vp(o_i), vp(o_d), vp(o_d), ctypes.byref(t)), (vp(w), None, vp(hi), vp(o_i), vp(o_d), vp(o_d), ctypes.byref(t)),
                 (vp(w), vp(lo), None, vp(o_i), vp(o_d), vp(o_d), ctypes.byref(t)), (vp(w), vp(lo), vp(hi), None, vp(o_d), vp(o_d), ctypes.byref(t)),
                 (vp(w), vp(lo), vp(hi), vp(o_i), None, vp(o_d), ctypes.byref(t)), (vp(w), vp(lo), vp(hi), vp(o_i), vp(o_d), None, ctypes.byref(t)),
                 (vp(w), vp(lo), vp(hi), vp(o_i), vp(o_d), vp(o_d), None)):
        assert lib.pse_host_typed_table_layout(1, *args) == INVALID and "null" in lib.pse_last_error().decode()


# ---- pse_typed_table_create and pse_pair_table_typed on the device stand-in ----------------------------------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """The host side of the library over the device stand-in of the sanitizer build, here without a sanitizer: its pse_create runs
    the real parameter rule and its typed-table entry points the real validators and the real layout function."""
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_get_info", "pse_last_error", "pse_typed_table_create", "pse_typed_table_destroy",
                 "pse_pair_table_typed", "pse_exclusions_create"):
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


def test_create_and_call_refusals_on_the_stand_in(stub):
    from pse_amd import _lib
    n = 6
    h = stub_handle(stub, n)
    info = _lib.pse_info()
    assert stub.pse_get_info(h, ctypes.byref(info)) == 0
    rcut = info.as_dict()["rcut"]
    good = dict(n=n, types=np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32), ntypes=2, width=np.array([3, 0, 2], dtype=np.int32),
                rmin=np.array([0.5, 0.0, 0.0]), rmax=np.array([2.0, 0.0, rcut]), tables=np.arange(10, dtype=np.float64))

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_typed_table_create(hh, a["n"], vp(a["types"]), a["ntypes"], vp(a["width"]), vp(a["rmin"]), vp(a["rmax"]), vp(a["tables"]),
                                         ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_typed_table_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    refused("null out", with_out=False)
    refused("null handle", hh=None)
    for name in ("types", "width", "rmin", "rmax", "tables"):
        refused("null", **{name: None})
    refused("n = 0", n=0)
    refused("n = 7", n=7)
    refused("ntypes = 0", ntypes=0)
    refused("ntypes = 9", ntypes=9)
    refused("type 2", types=np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32))
    refused("width 1", width=np.array([3, 1, 2], dtype=np.int32))
    refused("width -1", width=np.array([3, -1, 2], dtype=np.int32))
    refused("width 2049", width=np.array([3, 0, 2049], dtype=np.int32), tables=np.zeros(2 * 2052))
    refused("all widths are zero", width=np.zeros(3, dtype=np.int32))
    refused("3585", width=np.array([2048, 1537, 0], dtype=np.int32), rmax=np.array([2.0, 1.0, 0.0]), tables=np.zeros(2 * 3585))
    refused("finite", rmin=np.array([np.nan, 0.0, 0.0]))
    refused("finite", rmax=np.array([2.0, 0.0, np.inf]))
    refused("negative", rmin=np.array([-0.5, 0.0, 0.0]))
    refused("must exceed", rmax=np.array([0.5, 0.0, rcut]))
    refused("rcut", rmax=np.array([2.0, 0.0, rcut * (1.0 + 1e-12)]))
    bad = good["tables"].copy()
    bad[7] = np.inf
    refused("table entry 3 (F)", tables=bad)
    # the off pair type's range is not looked at; the cap itself and rmax = rcut are accepted
    rc, t = create(rmin=np.array([0.5, np.nan, 0.0]), rmax=np.array([2.0, -1.0, rcut]))
    assert rc == 0 and t.value, stub.pse_last_error()
    rc, tcap = create(width=np.array([2048, 1536, 0], dtype=np.int32), rmax=np.array([2.0, 1.0, 0.0]), tables=np.zeros(2 * CAP))
    assert rc == 0 and tcap.value, stub.pse_last_error()
    assert stub.pse_typed_table_destroy(tcap) == 0

    # the call: the order of the header.  Any non-null address will do for the arrays: the stand-in reads none of them
    other = stub_handle(stub, n)
    slab = stub_handle(stub, n, L=40.0, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex, ex_other = ctypes.c_void_p(), ctypes.c_void_p()
    assert stub.pse_exclusions_create(h, n, 1, vp(pairs), ctypes.byref(ex)) == 0
    assert stub.pse_exclusions_create(other, n, 1, vp(pairs), ctypes.byref(ex_other)) == 0
    rc, tslab = create(hh=slab)
    assert rc == 0, stub.pse_last_error()
    buf = np.zeros(8)
    X = vp(buf)

    def call(word, tt=t, pos=X, force=X, N=n, out8=X, e=None):
        rc = stub.pse_pair_table_typed(tt, pos, force, None, N, 0, out8, e)
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg), (word, rc, msg)

    call("null typed table", tt=None)
    call("null pos", pos=None)
    call("both null", force=None, out8=None)
    call("N = 0", N=0)
    call("N = 7", N=n + 1)
    call("slab rank", tt=tslab)
    call(None, tt=tslab, out8=None)                                            # forces only are allowed there
    call("another handle", e=ex_other)
    call(None, e=ex)
    call(None)
    call(None, force=None)
    call(None, out8=None)
    assert stub.pse_typed_table_destroy(t) == 0
    for hh in (h, other, slab):                                                # the objects still alive go with their handles
        assert stub.pse_destroy(hh) == 0


# ---- forces.TypedTablePair: what is checked before the device is touched ------------------------------------------------------------

class _NoDevice:
    """Stands where the integrator belongs: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


def test_provider_argument_checks_come_before_the_device():
    from pse_amd import forces
    t = harmonic_table(40.0, 2.0, 16)
    ok = (t, 0.0, 2.0)
    types = [0, 1, 1, 0]
    named = ["A", "B", "B", "A"]
    cases = [
        ("both", dict(types=types, tables={(0, 1): ok, (1, 0): ok})),                                  # one pair in both orders
        ("both", dict(types=named, tables={("A", "B"): ok, ("B", "A"): ok}, type_names=["A", "B"])),
        ("twice", dict(types=named, tables={("A", "B"): ok, (0, 1): ok}, type_names=["A", "B"])),
        ("unknown type name 'C'", dict(types=named, tables={("A", "C"): ok}, type_names=["A", "B"])),
        ("unknown type name 'C'", dict(types=["A", "C"], tables={("A", "A"): ok}, type_names=["A", "B"])),
        ("type_names", dict(types=named, tables={("A", "A"): ok})),                                    # names without the list
        ("(width, 2)", dict(types=types, tables={(0, 1): (np.zeros((5, 3)), 0.0, 2.0)})),
        ("(width, 2)", dict(types=types, tables={(0, 1): (np.zeros((1, 2)), 0.0, 2.0)})),
        ("(width, 2)", dict(types=types, tables={(0, 1): (np.zeros((2049, 2)), 0.0, 2.0)})),
        ("finite", dict(types=types, tables={(0, 1): (np.full((4, 2), np.nan), 0.0, 2.0)})),
        ("rmin < rmax", dict(types=types, tables={(0, 1): (t, 2.0, 1.0)})),
        ("(table, rmin, rmax)", dict(types=types, tables={(0, 1): (t, 0.0)})),
        ("non-empty dict", dict(types=types, tables={})),
        ("pair (a, b)", dict(types=types, tables={0: ok})),
        ("outside [1, 8]", dict(types=[0, 8], tables={(0, 0): ok})),
        ("non-negative", dict(types=[0, -1], tables={(0, 0): ok})),
    ]
    for word, kw in cases:
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            forces.TypedTablePair(_NoDevice(), **kw)
    with pytest.raises(ValueError, match="V, F, rmin, rmax, width"):
        forces.TypedTablePair.from_functions(_NoDevice(), types, {(0, 1): (abs, abs, 0.0, 2.0)})
    with pytest.raises(ValueError, match="at least 2"):
        forces.TypedTablePair.from_functions(_NoDevice(), types, {(0, 1): (abs, abs, 0.0, 2.0, 1)})
    # the arrays that go to pse_typed_table_create: names by their position in type_names, the tables in the order of p(a, b)
    ty, ntypes, width, rmin, rmax, entries = forces._typed_arguments(named, {("B", "A"): ok, ("B", "B"): (t[:5], 0.5, 1.0)}, ["A", "B"])
    assert ty.tolist() == [0, 1, 1, 0] and ty.dtype == np.uint32 and ntypes == 2
    assert width.tolist() == [0, 16, 5] and rmin.tolist() == [0.0, 0.0, 0.5] and rmax.tolist() == [0.0, 2.0, 1.0]
    assert np.array_equal(entries, np.concatenate([t, t[:5]]))
    rw, rlo, rhi, rent = tr.arrays({(1, 0): ok, (1, 1): (t[:5], 0.5, 1.0)}, 2)
    assert np.array_equal(width, rw) and np.array_equal(rmin, rlo) and np.array_equal(rmax, rhi) and np.array_equal(entries, rent)
