"""CPU tests of the static structure factor that need no device: the extended-precision reference the GPU tests compare to
(tests/structure_factor_ref.py) on a lattice whose densities are known and against its own symmetries; the bound of the GPU tests
against a plain-float64 restatement on the GPU tests' inputs; the NumPy helpers of pse_amd.analyze; the refusals of
pse_structure_factor_create and pse_structure_factor_accumulate through the device stand-in of the sanitizer build
(pse_amd/csrc/asan_stub.cpp, which runs the real validators), built here without a sanitizer; and the argument checks of
analyze.StructureFactor that come before the device is touched."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import structure_factor_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(autouse=True)
def _extended():
    sr.need_extended_precision()


# ---- the reference ---------------------------------------------------------------------------------------------------------------

def fractional_lattice(c, box):
    g = np.arange(c) / c - 0.5
    s = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return sr.from_fractional(s, box)


@pytest.mark.parametrize("box", [sr.CUBIC, sr.TILTED], ids=["cubic", "tilted"])
def test_simple_cubic_lattice_has_its_bragg_peaks_and_nothing_else(box):
    """c^3 sites at the fractional coordinates i/c: |rho(m)| = N where every m_i is a multiple of c, 0 elsewhere."""
    c = 4
    pos = fractional_lattice(c, box)
    n = c ** 3
    g = np.arange(-2 * c, 2 * c + 1)
    modes = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    r = np.abs(sr.rho(pos, box, modes)[0])
    bragg = (modes % c == 0).all(axis=1)
    assert bragg.sum() == 125
    print(f"lattice: |rho| - N at the peaks <= {np.abs(r[bragg] - n).max():.2e}, |rho| elsewhere <= {r[~bragg].max():.2e}")
    assert np.abs(r[bragg] - n).max() <= 1e-9 and r[~bragg].max() <= 1e-9


@pytest.mark.parametrize("name", sorted(sr.BOXES))
def test_reference_symmetries(name):
    box = sr.BOXES[name]
    n, ntypes = 257, 3
    pos = sr.points(n, box)
    types = np.random.default_rng(21).integers(0, ntypes, n)
    modes = np.concatenate([sr.half_space(2), sr.line(2, -20, 20), [[0, 0, 0]]])
    r = sr.rho(pos, box, modes, types, ntypes)
    one = sr.rho(pos, box, modes)
    # rho(0) = N_a, exactly
    assert np.array_equal(r[:, -1], np.bincount(types, minlength=ntypes).astype(complex)) and one[0, -1] == n
    # the types add up to the one-type density; rho(-m) is the conjugate
    assert np.abs(r.sum(axis=0) - one[0]).max() <= 1e-13 * n
    assert np.abs(sr.rho(pos, box, -modes, types, ntypes) - r.conj()).max() == 0.0
    # random lattice vectors, the tilted one included, added to every particle: unchanged to within the bound at the larger |s|
    shift = np.random.default_rng(31).integers(-3, 4, size=(n, 3)).astype(np.float64) @ sr.lattice_vectors(box)
    moved = pos + shift
    smax = sr.s_max(moved, box)
    assert 2.5 < smax < 3.6
    ratio = sr.worst_ratio(sr.rho(moved, box, modes, types, ntypes), r, modes, n, smax)
    print(f"{name}: shifted by lattice vectors to |s| <= {smax:.2f}: worst error / tol = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", sorted(sr.BOXES))
def test_the_bound_leaves_room_for_plain_float64(name):
    """A plain-float64 restatement stays inside tol(m) against the reference on the inputs of the GPU tests (every mode set with
    sum |m_i| <= 192; the corners at +-4096 are what the exact reduction of the kernel is for: float64 m.s has lost 13 bits there)."""
    box = sr.BOXES[name]
    n = 513
    pos = sr.points(n, box)
    worst, margin = 0.0, 0.0
    for key, modes in sr.mode_sets().items():
        if key == "corners":
            continue
        assert np.abs(modes).sum(axis=1).max() <= 192
        want, got = sr.rho(pos, box, modes), sr.rho_float64(pos, box, modes)
        worst = max(worst, sr.worst_ratio(got, want, modes, n))
        margin = max(margin, float(np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)).max()) / n)
    print(f"{name}: float64 against long double, n = {n}: worst error {margin:.2e} N, worst error / tol = {worst:.3f}")
    assert worst <= 1.0


# ---- the helpers of pse_amd.analyze ------------------------------------------------------------------------------------------------

def test_k_vectors_are_the_phase_of_the_definition():
    from pse_amd import analyze
    for box in sr.BOXES.values():
        pos = sr.points(40, box, seed=3)
        modes = sr.half_space(2)
        k = analyze.k_vectors(modes, box)
        s = sr.fractional(pos, box, np.float64)
        assert np.abs(pos @ k.T - 2.0 * math.pi * (s @ modes.T.astype(float))).max() < 1e-12
    Lx, Ly, Lz, xy = sr.TILTED
    assert np.allclose(analyze.k_vectors([[1, 2, 3]], sr.TILTED)[0], 2 * math.pi * np.array([1 / Lx, 2 / Ly - xy / Lx, 3 / Lz]), rtol=1e-15)
    assert np.array_equal(analyze.k_vectors([[1, 2, 3]], sr.CUBIC[:3]), analyze.k_vectors([[1, 2, 3]], sr.CUBIC))
    a = analyze.axis_modes(256)
    assert a.shape == (768, 3) and a.dtype == np.int32 and (np.count_nonzero(a, axis=1) == 1).all() and a.min() == 0 and a.max() == 256
    assert len({tuple(m) for m in a}) == 768
    with pytest.raises(ValueError, match="positive"):
        analyze.axis_modes(0)


def test_modes_within_against_brute_force():
    from pse_amd import analyze
    box, kmax = (14.0, 11.0, 17.0, 0.3), 2.3
    m = analyze.modes_within(box, kmax)
    g = np.arange(-8, 9)
    every = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    kn = np.linalg.norm(2 * math.pi * every / np.array(box[:3]), axis=1)         # (tilt 0)
    inside = every[(kn <= kmax) & (kn > 0)]
    assert len(inside) == 2 * len(m) and len(m) > 100 and np.abs(inside).max() < 8
    got = {tuple(v) for v in m}
    assert len(got) == len(m)
    for v in inside:                                                            # one of every pair +-m, none missing
        assert (tuple(v) in got) != (tuple(-v) in got)
    for v in m:                                                                 # first non-zero component positive
        assert v[np.nonzero(v)[0][0]] > 0
    assert m.dtype == np.int32 and m.tolist() == sorted(m.tolist())
    assert len(analyze.modes_within((14.0, 14.0, 14.0), 2 * math.pi / 14.0 * 1.0000001)) == 3
    assert len(analyze.modes_within((40.0, 40.0, 40.0), 2 * math.pi / 40.0 * 24.8)) <= 32768
    with pytest.raises(ValueError, match="more than 32768"):
        analyze.modes_within((40.0, 40.0, 40.0), 2 * math.pi / 40.0 * 25.2)
    with pytest.raises(ValueError, match="more than 32768"):
        analyze.modes_within((347.0, 347.0, 347.0), 3.5)
    with pytest.raises(ValueError, match="kmax > 0"):
        analyze.modes_within(box, 0.0)


def test_normalisations_and_shell_average_on_the_lattice():
    """Two interleaved types on the fractional lattice: at a Bragg peak of the whole lattice rho_A = rho_B = N/2 (types by layer of z,
    peaks with mz a multiple of c), so S_AA = S_BB = S_AB = N/2 and the total S = N; away from every peak all are 0."""
    from pse_amd import analyze
    c, box = 4, sr.CUBIC
    pos = fractional_lattice(c, box)
    n = c ** 3
    types = np.arange(n) % 2                                                      # z is the fastest index: A and B alternate along z
    modes = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 8], [1, 0, 0], [0, 2, 1], [0, 0, 2], [3, 3, 3]])
    r = sr.rho(pos, box, modes, types, 2)
    sums = 3.0 * sr.products(r)                                                   # three equal samples
    counts = [n // 2, n // 2]
    want = np.array([1, 1, 1, 0, 0, 0, 0]) * (n / 2.0)
    for a, b in ((0, 0), (0, 1), (1, 1), (1, 0)):
        got = analyze.S_of_sums(sums, 3, counts, a, b)
        special = got[5]                                                          # (0, 0, 2): the sublattices' own peak, rho_A = -rho_B = N/2
        assert np.abs(np.delete(got, 5) - np.delete(want, 5)).max() < 1e-9
        assert abs(special - (n / 2.0 if a == b else -n / 2.0)) < 1e-9
    total = analyze.S_of_sums(sums, 3, counts)
    assert np.abs(total - np.array([1, 1, 1, 0, 0, 0, 0]) * float(n)).max() < 1e-9
    assert np.allclose(total, (np.abs(r.sum(axis=0)) ** 2) / n, atol=1e-9)
    with pytest.raises(ValueError, match="no samples"):
        analyze.S_of_sums(sums, 0, counts)
    with pytest.raises(ValueError, match="both types or neither"):
        analyze.S_of_sums(sums, 1, counts, 0, None)
    with pytest.raises(ValueError, match="no particle of type 1"):
        analyze.S_of_sums(sums, 1, [n, 0], 0, 1)
    # shells: |k| in units of 2 pi / 14 is 0, 4, sqrt 80, 1, sqrt 5, 2, sqrt 27
    k = analyze.k_vectors(modes, box)
    unit = 2 * math.pi / 14.0
    centres, mean, cnt = analyze.shell_average_of(k, total, 9, kmax=9 * unit)
    assert np.allclose(centres, (np.arange(9) + 0.5) * unit, rtol=1e-14) and cnt.tolist() == [1, 1, 2, 0, 1, 1, 0, 0, 1]
    assert np.allclose(mean[[0, 1, 2, 4, 5, 8]], [n, 0, 0, n, 0, n], atol=1e-9) and np.isnan(mean[[3, 6, 7]]).all()
    centres, mean, cnt = analyze.shell_average_of(k, total, 2)                    # kmax = the largest |k| = sqrt 80: the edge mode is kept
    assert cnt.tolist() == [5, 2] and abs(mean[0] - 2 * n / 5.0) < 1e-9 and abs(mean[1] - n / 2.0) < 1e-9
    centres, mean, cnt = analyze.shell_average_of(k, total, 2, kmax=3 * unit)     # modes beyond kmax are left out
    assert cnt.tolist() == [2, 2]
    with pytest.raises(ValueError, match="nbins"):
        analyze.shell_average_of(k, total, 0)


# ---- pse_structure_factor_create and pse_structure_factor_accumulate on the device stand-in -----------------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """The host side of the library over the device stand-in of the sanitizer build, here without a sanitizer: its pse_create runs
    the real parameter rule and its structure-factor entry points the real validators and the real mode plan."""
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_last_error", "pse_structure_factor_create", "pse_structure_factor_destroy",
                 "pse_structure_factor_accumulate"):
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
    n = 6
    h = stub_handle(stub, n)
    good = dict(n=n, types=np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32), ntypes=2, nk=3,
                modes=np.array([[1, 0, 0], [0, -4096, 4096], [0, 0, 0]], dtype=np.int32))

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_structure_factor_create(hh, a["n"], vp(a["types"]), a["ntypes"], a["nk"], vp(a["modes"]),
                                              ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_structure_factor_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    bad_type = np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32)
    big = np.zeros((32769, 3), dtype=np.int32)
    refused("null out", with_out=False)
    refused("null out", with_out=False, hh=None)
    refused("null handle", hh=None, n=0)
    refused("n = 0", n=0, ntypes=0)
    refused("n = 7", n=7, ntypes=9)
    refused("n = 7", n=7, types=None)
    refused("ntypes = 0", ntypes=0, nk=0)
    refused("ntypes = 9", ntypes=9, modes=None)
    refused("nk = 0", nk=0, modes=None)
    refused("nk = 32769", nk=32769, modes=big, types=bad_type)
    refused("null modes", modes=None, types=bad_type)
    refused("mx = 4097", modes=np.array([[1, 0, 0], [4097, 0, 0], [0, 0, 0]], dtype=np.int32), types=bad_type)
    refused("my = -4097", modes=np.array([[1, 0, 0], [0, -4097, 5000], [0, 0, 0]], dtype=np.int32))
    refused("mz = 5000", modes=np.array([[1, 0, 0], [0, 0, 5000], [0, 0, 0]], dtype=np.int32))
    refused("mode 2", modes=np.array([[1, 0, 0], [0, 0, 0], [0, 0, -4097]], dtype=np.int32))
    refused("type 2", types=bad_type)
    refused("type 1", ntypes=1)
    # the caps themselves, no types, duplicates and a mode with its negative, a slab rank
    slab = stub_handle(stub, n, L=40.0, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    made = []
    for kw in (dict(), dict(nk=32768, modes=big), dict(types=None, ntypes=1), dict(ntypes=8), dict(hh=slab), dict(n=1),
               dict(modes=np.array([[1, 2, 3], [-1, -2, -3], [1, 2, 3]], dtype=np.int32))):
        rc, f = create(**kw)
        assert rc == 0 and f.value, (kw, stub.pse_last_error())
        made.append(f)
    f = made[0]

    # the call.  Any non-null, 8-byte aligned address will do for the arrays: the stand-in reads none of them
    buf = np.zeros(8)
    X, odd = vp(buf), ctypes.c_void_p(buf.ctypes.data + 4)

    def call(word, ff=f, pos=X, N=n, rho=X, sums=X):
        rc = stub.pse_structure_factor_accumulate(ff, pos, None, N, rho, sums)
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg and "pse_structure_factor_accumulate" in msg), (word, rc, msg)

    call("null structure-factor object", ff=None, N=0)
    call("N = 0", N=0, pos=None)
    call("N = 7", N=n + 1, pos=None)
    call("null pos", pos=None, rho=None, sums=None)
    call("both null", rho=None, sums=None)
    call("rho", rho=odd, sums=odd)
    call("8-byte aligned", rho=odd)
    call("sums", sums=odd)
    call("8-byte aligned", rho=None, sums=odd)
    call(None)
    call(None, rho=None)
    call(None, sums=None)
    call(None, N=1)
    for g in made[1:4]:
        assert stub.pse_structure_factor_destroy(g) == 0
    assert stub.pse_structure_factor_destroy(None) == 0
    for hh in (h, slab):                                                       # the objects still alive go with their handle
        assert stub.pse_destroy(hh) == 0


# ---- analyze.StructureFactor and engine.StructureFactorModes: what is checked before the device is touched --------------------------

class _NoDevice:
    """Stands where the integrator (or the engine) belongs: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


def test_analyzer_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    ok = [[1, 0, 0], [0, 1, 0]]
    named = ["A", "B", "B", "A"]
    cases = [
        ("(nk, 3)", dict(modes=[])),
        ("(nk, 3)", dict(modes=[1, 2, 3])),
        ("(nk, 3)", dict(modes=[[1, 2]])),
        ("(nk, 3)", dict(modes=[[0.5, 1.0, 2.0]])),
        ("more than 32768", dict(modes=np.zeros((32769, 3), dtype=int))),
        ("4097 beyond", dict(modes=[[0, -4097, 0]])),
        ("outside [1, 8]", dict(modes=ok, types=[0, 8])),
        ("non-negative", dict(modes=ok, types=[0, -1])),
        ("non-negative", dict(modes=ok, types=[])),
        ("type_names", dict(modes=ok, types=named)),                                       # names without the list
        ("unknown type name 'C'", dict(modes=ok, types=["A", "C"], type_names=["A", "B"])),
        ("distinct strings", dict(modes=ok, types=named, type_names=["A", "A"])),
        ("one type", dict(modes=ok, type_names=["A", "B"])),
        ("period", dict(modes=ok, period=0)),
    ]
    for word, kw in cases:
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            analyze.StructureFactor(_NoDevice(), **kw)
    ty, ntypes, modes, names, period = analyze._structure_factor_analyzer_arguments(ok, named, ["A", "B", "C"], 250)
    assert ty.tolist() == [0, 1, 1, 0] and ty.dtype == np.uint32 and (ntypes, names, period) == (3, ["A", "B", "C"], 250)
    assert modes.dtype == np.int32 and modes.flags.c_contiguous and modes.tolist() == ok
    ty, ntypes, *_ = analyze._structure_factor_analyzer_arguments(ok, None, None, 1)
    assert ty is None and ntypes == 1
    for word, args in (("outside [1, 8]", (None, 9, ok)), ("type 2 >= ntypes = 2", ([0, 2], 2, ok)), ("(nk, 3)", (None, 1, [[1, 2]])),
                       ("4100 beyond", (None, 1, [[4100, 0, 0]]))):
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            engine.StructureFactorModes(_NoDevice(), *args)
