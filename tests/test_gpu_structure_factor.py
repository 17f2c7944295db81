"""GPU tests of the static structure factor (pse_structure_factor_create, pse_structure_factor_accumulate) and of
analyze.StructureFactor on top of it: rho against the extended-precision reference of tests/structure_factor_ref.py (validated on
the CPU by tests/test_structure_factor_cpu.py), per component within tol(m) = N (2e-14 + 4e-15 s_max sum|m_i|), over the chunk and
tile edges of the two kernels, the mode sets from one mode to the corners at +-4096, the numbers of types, a group, lattice shifts, a
changed box, the accumulation into sums, bit-reproducibility, the state of the handle, the error returns of the raw C-ABI, the
lifetime of the device object, and the analyzer through System.run.

The kernel stages SF_CHUNK = 256 particles at a time and gives a workgroup 64 segments of at most SF_RUN = 8 modes: 512 modes of a
line, 128 of a scattered list (whose sorted neighbours pair up)."""
import ctypes
import functools
import gc

import numpy as np
import pytest

from conftest import to4
import structure_factor_ref as sr
from test_gpu_provider_lifetime import _Unraisable

pytestmark = pytest.mark.gpu

NMAX = 513                                       # two chunks of 256 and one particle
CHUNK, TILE_LINE, TILE_SCATTERED = 256, 512, 128
INVALID = -1
BOXES = pytest.mark.parametrize("name", ["cubic", "tilted", "negative"])
SETS = sr.mode_sets()


@pytest.fixture(autouse=True)
def _extended():
    sr.need_extended_precision()


@functools.lru_cache(maxsize=None)
def engine(name):
    import pse_amd
    return pse_amd.Engine(NMAX, sr.BOXES[name], xi=0.5, error=1e-3)


@functools.lru_cache(maxsize=None)
def points(name, n=NMAX):
    """The first n of the 513 seeded points of the box."""
    pos = sr.points(NMAX, sr.BOXES[name])[:n].copy()
    pos.setflags(write=False)
    return pos


def types_of(n, ntypes, seed=21):
    return np.random.default_rng(seed).integers(0, ntypes, n)


@functools.lru_cache(maxsize=None)
def reference(name, key, n=NMAX, ntypes=1):
    """The reference rho of the first n points of the box for the mode set `key`, computed once and shared."""
    r = sr.rho(points(name, n), sr.BOXES[name], SETS[key], None if ntypes == 1 else types_of(n, ntypes), ntypes)
    r.setflags(write=False)
    return r


def device(eng, pos, modes, types=None, ntypes=1, group=None, n=None, rho=True, sums=None):
    """One accumulate call on a new object, read back: rho (ntypes, nk) complex, or None."""
    import torch
    sf = eng.structure_factor(types, ntypes, modes, n)
    assert (sf.nk, sf.ntypes, sf.npt) == (len(modes), ntypes, ntypes * (ntypes + 1) // 2)
    out = torch.full((ntypes, len(modes), 2), np.nan, dtype=torch.float64, device="cuda") if rho else None
    g = None if group is None else torch.tensor(np.asarray(group), dtype=torch.int32, device="cuda")
    assert eng.structure_factor_accumulate(to4(pos), sf, rho=out, sums=sums, group=g) == (out, sums)
    got = None
    if rho:
        got = out.cpu().numpy()
        got = got[..., 0] + 1j * got[..., 1]
    sf.close()
    with pytest.raises(ValueError, match="closed"):
        eng.structure_factor_accumulate(to4(pos), sf, rho=out, sums=sums, group=g)
    return got


def assert_within(got, want, modes, n, smax=0.5, what=""):
    ratio = sr.worst_ratio(got, want, modes, n, smax)
    print(f"{what}: n = {n}, {len(modes)} modes: worst error / tol = {ratio:.4f}")
    assert got.shape == want.shape and np.isfinite(got.view(np.float64)).all() and ratio <= 1.0, (what, ratio)


# -- rows, modes, types ----------------------------------------------------------------------------------------------------------------

@BOXES
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_row_counts(n, name):
    """One particle, two, a wave and a chunk less one, full, plus one; two chunks less one, two chunks, two chunks plus one."""
    pos, types = points(name, n), types_of(n, 2)
    got = device(engine(name), pos, SETS["half3"], types, 2)
    assert_within(got, reference(name, "half3", n, 2), SETS["half3"], n, what=f"{name} rows")


@BOXES
@pytest.mark.parametrize("key", sorted(SETS))
def test_mode_sets(key, name):
    """One mode; (0, 0, 0) alone, which gives N exactly; the half space |m_i| <= 3; the eight corners at +-4096; lines of 201 modes
    along z, x and y at (5, -7) -- runs far longer than a segment; 4096 scattered modes."""
    modes = SETS[key]
    got = device(engine(name), points(name), modes)
    assert_within(got, reference(name, key), modes, NMAX, what=f"{name} {key}")
    if key == "zero":
        assert got[0, 0] == NMAX


@pytest.mark.parametrize("nk", [TILE_LINE - 1, TILE_LINE, TILE_LINE + 1, TILE_SCATTERED - 1, TILE_SCATTERED, TILE_SCATTERED + 1])
def test_tile_edges(nk):
    """A workgroup's 64 segments: a line of 511, 512 and 513 modes (full segments), and 127, 128 and 129 scattered ones (pairs)."""
    name = "tilted"
    modes = sr.line(2, 0, nk - 1, at=(1, -2)) if nk >= TILE_LINE - 1 else sr.scattered(nk, 64, seed=9)
    pos = points(name, 257)
    got = device(engine(name), pos, modes)
    assert_within(got, sr.rho(pos, sr.BOXES[name], modes), modes, 257, what=f"tile {nk}")


@BOXES
@pytest.mark.parametrize("ntypes", [1, 2, 3, 8])
def test_types(ntypes, name):
    got = device(engine(name), points(name), SETS["zline"], None if ntypes == 1 else types_of(NMAX, ntypes), ntypes)
    assert_within(got, reference(name, "zline", NMAX, ntypes), SETS["zline"], NMAX, what=f"{name} {ntypes} types")


def test_no_types_an_unused_type_and_a_short_type_array():
    import torch
    name = "tilted"
    eng, pos, modes = engine(name), points(name), SETS["half3"]
    # types_host = NULL is one type, bit for bit
    one = device(eng, pos, modes, np.zeros(NMAX, dtype=int), 1)
    assert np.array_equal(device(eng, pos, modes), one)
    # a declared type without particles: rho exactly 0, its rows of sums untouched
    types = types_of(NMAX, 2) * 2                                              # types 0 and 2 of three
    pre = np.random.default_rng(4).uniform(-1e6, 1e6, size=(6, len(modes)))
    sums = torch.tensor(pre, device="cuda")
    got = device(eng, pos, modes, types, 3, sums=sums)
    assert np.all(got[1] == 0.0) and np.abs(got[0]).min() > 0.0
    want = sr.rho(pos, sr.BOXES[name], modes, types, 3)
    assert_within(got, want, modes, NMAX, what="unused type")
    after = sums.cpu().numpy()
    for p in (1, 3, 4):                                                        # AB, BB, BC
        assert np.array_equal(after[p], pre[p])
    assert not np.array_equal(after[0], pre[0]) and not np.array_equal(after[2], pre[2]) and not np.array_equal(after[5], pre[5])
    # a type array shorter than the rows: the particles past it act as type 0
    short = types_of(300, 2)
    full = np.concatenate([short, np.zeros(NMAX - 300, dtype=int)])
    got = device(eng, pos, modes, short, 2, n=300)
    assert np.array_equal(got, device(eng, pos, modes, full, 2))
    assert_within(got, sr.rho(pos, sr.BOXES[name], modes, full, 2), modes, NMAX, what="short types")


@BOXES
def test_group_of_every_other_particle(name):
    """The types are those of the caller's indices, not of the positions in the group."""
    pos, types, modes = points(name), types_of(NMAX, 3), SETS["half3"]
    members = np.arange(1, NMAX, 2)
    got = device(engine(name), pos, modes, types, 3, group=members)
    assert_within(got, sr.rho(pos[members], sr.BOXES[name], modes, types[members], 3), modes, len(members), what=f"{name} group")


@BOXES
def test_lattice_shifts(name):
    """Every particle moved by its own lattice vector, the tilted one included, out to |s| = 3.5: the same rho, within the bound at
    that s_max."""
    box = sr.BOXES[name]
    shift = np.random.default_rng(31).integers(-3, 4, size=(NMAX, 3)).astype(np.float64) @ sr.lattice_vectors(box)
    moved = points(name) + shift
    smax = sr.s_max(moved, box)
    assert 3.0 < smax < 3.6
    for key in ("half3", "corners", "zline"):
        got = device(engine(name), moved, SETS[key])
        assert_within(got, reference(name, key), SETS[key], NMAX, smax, what=f"{name} shifted {key}")


def test_the_box_of_the_call_not_of_the_creation():
    import pse_amd
    import torch
    eng = pse_amd.Engine(NMAX, sr.CUBIC, xi=0.5, error=1e-3)
    pos, modes = points("cubic"), SETS["half3"]
    sf = eng.structure_factor(None, 1, modes)
    rho = torch.empty((1, len(modes), 2), dtype=torch.float64, device="cuda")
    for xy in (0.0, 0.25, -0.4):
        box = sr.CUBIC[:3] + (xy,)
        eng.set_box(*box)
        eng.structure_factor_accumulate(to4(pos), sf, rho=rho)
        got = rho.cpu().numpy()
        assert_within(got[..., 0] + 1j * got[..., 1], sr.rho(pos, box, modes), modes, NMAX, what=f"xy = {xy}")
    eng.close()


# -- sums ----------------------------------------------------------------------------------------------------------------------------

def test_sums_are_added_to_and_either_output_may_be_absent():
    import torch
    name, ntypes = "tilted", 3
    eng, pos, types, modes = engine(name), to4(points(name)), types_of(NMAX, ntypes), SETS["half3"]
    nk = len(modes)
    sf = eng.structure_factor(types, ntypes, modes)
    pre = np.random.default_rng(4).uniform(-1e6, 1e6, size=(6, nk))
    sums, rho = torch.tensor(pre, device="cuda"), torch.empty((ntypes, nk, 2), dtype=torch.float64, device="cuda")
    eng.structure_factor_accumulate(pos, sf, rho=rho, sums=sums)
    r = rho.cpu().numpy()
    r = r[..., 0] + 1j * r[..., 1]
    prod, mag = sr.products(r), sr.products(np.abs(r).astype(complex))         # Re(rho_a conj rho_b) and |rho_a| |rho_b|
    once = sums.cpu().numpy()
    slack = 4.0 * 2.0 ** -53 * (mag + np.abs(pre))
    print(f"sums: worst error / slack = {(np.abs(once - (pre + prod)) / slack).max():.3f}")
    assert (np.abs(once - (pre + prod)) <= slack).all() and np.abs(prod).max() > 100.0
    # again: added twice; rho = NULL
    eng.structure_factor_accumulate(pos, sf, sums=sums)
    twice = sums.cpu().numpy()
    assert (np.abs(twice - (once + prod)) <= 4.0 * 2.0 ** -53 * (mag + np.abs(once))).all()
    # sums = NULL: rho alone, the same bits, sums untouched
    again = torch.zeros_like(rho)
    eng.structure_factor_accumulate(pos, sf, rho=again)
    assert torch.equal(again, rho) and np.array_equal(sums.cpu().numpy(), twice)
    # the Python layer's own checks
    for kw, word in ((dict(), "both None"), (dict(rho=rho[:2]), "rho must be"), (dict(sums=sums.float()), "sums must be"),
                     (dict(rho=rho.cpu()), "rho must be"), (dict(sums=sums[:, :-1]), "sums must be")):
        with pytest.raises(ValueError, match=word):
            eng.structure_factor_accumulate(pos, sf, **kw)
    sf.close()


# -- reproducibility -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["half3", "zline", "scattered"])
def test_equal_inputs_equal_bits_and_the_order_of_the_list_does_not_matter(key):
    name = "negative"
    eng, pos, types, modes = engine(name), points(name), types_of(NMAX, 2), SETS[key]
    first = device(eng, pos, modes, types, 2)
    assert np.array_equal(first, device(eng, pos, modes, types, 2))
    # a permuted mode list: the same bits, permuted -- the value of a mode is a function of the mode SET
    perm = np.random.default_rng(8).permutation(len(modes))
    assert np.array_equal(device(eng, pos, modes[perm], types, 2), first[:, perm])
    # a permuted particle order: another order of the sums, the same rho within the bound
    order = np.random.default_rng(9).permutation(NMAX)
    got = device(eng, pos[order], modes, types[order], 2)
    assert_within(got, reference(name, key, NMAX, 2), modes, NMAX, what=f"permuted particles {key}")


def test_duplicates_and_a_mode_with_its_negative():
    name = "tilted"
    modes = np.array([[3, -2, 5], [-3, 2, -5], [3, -2, 5], [0, 0, 0], [3, -2, 5], [0, 0, 0]])
    got = device(engine(name), points(name), modes)
    assert got[0, 0] == got[0, 2] == got[0, 4] and got[0, 3] == got[0, 5] == NMAX
    assert_within(got, sr.rho(points(name), sr.BOXES[name], modes), modes, NMAX, what="duplicates")


# -- the state of the handle -----------------------------------------------------------------------------------------------------------

def test_the_handle_is_left_as_it_was():
    """No sort, no neighbour list: a mobility call in between changes nothing, the counters of the kept list and info() are what they
    were before the pass, and the second mobility call reuses the kept list exactly as it does without the pass in between."""
    import pse_amd
    import torch
    name = "tilted"
    modes = SETS["half3"]
    force = to4(np.random.default_rng(2).normal(size=(NMAX, 3)))
    counts, vels = [], []
    for with_pass in (False, True):
        eng = pse_amd.Engine(NMAX, sr.BOXES[name], xi=0.5, error=1e-3)
        pos = to4(points(name))
        if with_pass:
            sf = eng.structure_factor(None, 1, modes)
            rho = [torch.empty((1, len(modes), 2), dtype=torch.float64, device="cuda") for _ in range(3)]
            eng.structure_factor_accumulate(pos, sf, rho=rho[0])               # on a handle that has never sorted
        v1 = eng.mobility(pos, force).clone()
        before, info = eng.neighbor_stats(), eng.info()
        if with_pass:
            eng.structure_factor_accumulate(pos, sf, rho=rho[1])
            assert eng.neighbor_stats() == before and eng.info() == info
        v2 = eng.mobility(pos, force)
        counts.append((before, eng.neighbor_stats()))
        vels.append(v2.cpu().numpy())
        assert (v1 - v2).abs().max().item() <= 1e-10
        if with_pass:
            eng.structure_factor_accumulate(pos, sf, rho=rho[2])
            assert torch.equal(rho[0], rho[1]) and torch.equal(rho[1], rho[2])
            got = rho[2].cpu().numpy()
            assert_within(got[..., 0] + 1j * got[..., 1], reference(name, "half3"), modes, NMAX, what="between the mobility calls")
        eng.close()
    print("(r_buff, builds, reuses) after the first and the second mobility call, without / with the pass:", counts)
    assert counts[0] == counts[1] and np.abs(vels[0] - vels[1]).max() <= 1e-10
    with pytest.raises(ValueError, match="went with the engine"):
        eng.structure_factor_accumulate(pos, sf, rho=rho[0])


def test_a_span_of_several_chunks():
    """n_max x ntypes x nk beyond 2^24 partial sums: a row of the workspace covers two chunks, staged one after the other."""
    import pse_amd
    name = "cubic"
    eng = pse_amd.Engine(600000, sr.BOXES[name], xi=0.5, error=1e-3)
    got = device(eng, points(name), SETS["scattered"], types_of(NMAX, 2), 2)
    assert_within(got, reference(name, "scattered", NMAX, 2), SETS["scattered"], NMAX, what="span of two chunks")
    eng.close()


# -- the raw C-ABI ---------------------------------------------------------------------------------------------------------------------

def test_misuse_is_reported_before_any_launch():
    """Raw C-ABI, as a C host would call it: a rejected call leaves both outputs untouched, and the handle works afterwards; the pass
    works on a slab rank's handle."""
    import torch
    from pse_amd import _lib
    from pse_amd._lib import pse_params
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731

    def create(L, n_max, **kw):
        p = pse_params()
        p.n_max, p.Lx, p.Ly, p.Lz, p.xy = n_max, L, L, L, 0.0
        p.xi, p.error, p.max_strain, p.seed = 0.5, 1e-3, 0.5, 1
        p.Nx = p.Ny = p.Nz = 0
        p.P, p.rcut, p.device, p.n_slabs, p.slab_rank = 0, 0.0, -1, 1, 0
        for k, v in kw.items():
            setattr(p, k, v)
        out = ctypes.c_void_p()
        return lib.pse_create(ctypes.byref(p), ctypes.byref(out)), out

    n = 300
    box = sr.CUBIC
    pos = points("cubic", n)
    types = types_of(n, 2).astype(np.uint32)
    modes = np.ascontiguousarray(SETS["half3"], dtype=np.int32)
    nk = len(modes)
    rc, h = create(box[0], n)
    assert rc == 0, msg()
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()

    def sf_on(hh, expect=0, word=None, ty=types, ntypes=2, mm=modes, k=nk, nn=n):
        f = ctypes.c_void_p(777)
        assert lib.pse_structure_factor_create(hh, nn, None if ty is None else vp(ty), ntypes, k, None if mm is None else vp(mm),
                                               ctypes.byref(f)) == expect, msg()
        assert expect == 0 or (word in msg() and "pse_structure_factor_create" in msg() and not f.value), (word, msg())
        return f

    f = sf_on(h)
    bad = types.copy()
    bad[5] = 2
    far = modes.copy()
    far[7, 1] = -4097
    sf_on(h, INVALID, "n_max", nn=n + 1)
    sf_on(h, INVALID, "ntypes = 9", ntypes=9)
    sf_on(h, INVALID, "nk = 0", k=0)
    sf_on(h, INVALID, "nk = 32769", k=32769)
    sf_on(h, INVALID, "null modes", mm=None)
    sf_on(h, INVALID, "my = -4097", mm=far)
    sf_on(h, INVALID, "type 2", ty=bad)
    sf_on(None, INVALID, "null handle")
    assert lib.pse_structure_factor_create(h, n, vp(types), 2, nk, vp(modes), None) == INVALID and "null out" in msg()
    dpos = to4(pos)
    rho = torch.full((2, nk, 2), -5.0, dtype=torch.float64, device="cuda")
    sums = torch.full((3, nk), -7.0, dtype=torch.float64, device="cuda")
    call = lib.pse_structure_factor_accumulate

    def refused(word, ff=f, p=P(dpos), nn=n, r=P(rho), s=P(sums)):
        assert call(ff, p, None, nn, r, s) == INVALID, word
        assert word in msg() and "pse_structure_factor_accumulate" in msg(), (word, msg())

    refused("null structure-factor object", ff=None)
    refused("n_max", nn=0)
    refused("n_max", nn=n + 1)
    refused("null pos", p=None)
    refused("both null", r=None, s=None)
    refused("rho", r=ctypes.c_void_p(rho.data_ptr() + 4))
    refused("sums", s=ctypes.c_void_p(sums.data_ptr() + 4))
    torch.cuda.synchronize()
    assert np.all(rho.cpu().numpy() == -5.0) and np.all(sums.cpu().numpy() == -7.0)    # nothing was launched, nothing was written
    assert call(f, P(dpos), None, n, P(rho), P(sums)) == 0, msg()
    want = sr.rho(pos, box, modes, types, 2)
    got = rho.cpu().numpy()
    got = got[..., 0] + 1j * got[..., 1]
    assert_within(got, want, modes, n, what="after the refusals")
    assert np.abs(sums.cpu().numpy() + 7.0 - sr.products(got)).max() <= 1e-9
    # a slab rank's handle: positions are replicated there, the sums are complete (its box is 40^3)
    fs = sf_on(hs)
    assert call(fs, P(dpos), None, n, P(rho), None) == 0, msg()
    got = rho.cpu().numpy()
    assert_within(got[..., 0] + 1j * got[..., 1], sr.rho(pos, (40.0, 40.0, 40.0, 0.0), modes, types, 2), modes, n, what="slab rank")
    assert lib.pse_structure_factor_destroy(f) == 0
    assert lib.pse_structure_factor_destroy(None) == 0
    f = sf_on(h)                                                                       # still alive below: it goes with its handle
    for hh in (h, hs):
        assert lib.pse_destroy(hh) == 0


# -- analyze.StructureFactor -----------------------------------------------------------------------------------------------------------

@pytest.fixture
def restored_context():
    """A System registers itself as the current simulation context: put back what was there."""
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


def system(pos, box, members=None):
    from pse_amd import integrate
    from pse_amd.system import Group, System
    s = System(pos, box, dt=1e-3)
    group = s.all() if members is None else Group(s, members)
    return s, integrate.PSEv1(group=group, T=0.0, seed=3, xi=0.5, error=1e-3)


def test_analyzer_through_system_run(restored_context):
    """period and samples, reset(), S(a, b), S() and shell_average() against NumPy on the reference's sums over the positions of every
    sampled step; the particles move under a harmonic repulsion, so the samples differ."""
    from pse_amd import analyze, forces, shear_function, variant
    box = sr.CUBIC
    pos = points("cubic")
    n = len(pos)
    s, pse = system(pos, box)
    forces.HarmonicRepulsion(pse, k=40.0)
    names = ["A", "B"]
    types = types_of(n, 2)
    modes = analyze.modes_within(box, 2.0)
    nk = len(modes)
    sf = analyze.StructureFactor(pse, modes, types=[names[t] for t in types], type_names=names, period=2)
    assert s.analyzers == [sf] and sf.samples == 0 and not sf.sums.any() and (sf.nk, sf.npt, sf.ntypes) == (nk, 3, 2) and nk > 150
    with pytest.raises(ValueError, match="no samples"):
        sf.S()
    with pytest.raises(ValueError, match="no samples"):
        sf.k
    want = np.zeros((3, nk))
    snaps = []
    for t in range(5):                                                                 # samples at steps 0, 2 and 4
        if t % 2 == 0:
            snaps.append(s.pos.cpu().numpy()[:, :3].copy())
            want += sr.products(sr.rho(snaps[-1], box, modes, types, 2))
        s.run(1)
    assert sf.samples == 3 and np.abs(snaps[0] - snaps[2]).max() > 1e-6 and sf.boxes == [box] * 3
    got = sf.sums
    # (the products of two densities within tol of the reference's: |rho| <= n, three samples)
    bound = 3 * 2.0 * n * sr.tol(modes, n)[None, :]
    assert got.shape == (3, nk) and got.dtype == np.float64 and (np.abs(got - want) <= bound).all()
    counts = np.bincount(types, minlength=2)
    close = lambda x, y: np.abs(x - y).max() <= 1e-12 * np.abs(y).max()                 # noqa: E731
    assert close(sf.S("A", "A"), got[0] / (3 * counts[0])) and close(sf.S("B", "A"), got[1] / (3 * np.sqrt(counts[0] * counts[1])))
    assert np.array_equal(sf.S(1, 0), sf.S("A", "B")) and close(sf.S(1, 1), got[2] / (3 * counts[1]))
    total = (got[0] + got[2] + 2 * got[1]) / (3 * n)
    assert close(sf.S(), total) and total.min() > 0.0
    k = sf.k
    assert k.shape == (nk, 3) and np.array_equal(k, analyze.k_vectors(modes, box)) and np.linalg.norm(k, axis=1).max() <= 2.0
    centres, mean, cnt = sf.shell_average(8)
    kn = np.linalg.norm(k, axis=1)
    w = kn.max() / 8
    idx = np.minimum((kn / w).astype(int), 7)
    ref = np.array([total[idx == b].mean() if (idx == b).any() else np.nan for b in range(8)])
    ok = ~np.isnan(ref)
    assert cnt.sum() == nk and np.array_equal(np.isnan(mean), ~ok) and close(mean[ok], ref[ok]) and close(centres, (np.arange(8) + 0.5) * w)
    assert close(sf.shell_average(8, a="A", b="B")[1][ok], np.array([sf.S("A", "B")[idx == b].mean() for b in range(8) if ok[b]]))
    with pytest.raises(ValueError, match="unknown type name"):
        sf.S("A", "C")
    with pytest.raises(ValueError, match="both types or neither"):
        sf.S("A")
    # density(): one fresh call on the current positions, nothing accumulated
    now = s.pos.cpu().numpy()[:, :3].copy()
    d = sf.density()
    assert d.shape == (2, nk) and d.dtype == np.complex128 and sf.samples == 3 and np.array_equal(sf.sums, got)
    assert_within(d, sr.rho(now, box, modes, types, 2), modes, n, what="density()")
    sf.reset()
    assert sf.samples == 0 and not sf.sums.any() and sf.boxes == []
    s.run(1)                                                                           # step 5: not a sample
    assert sf.samples == 0 and not sf.sums.any()
    snap = s.pos.cpu().numpy()[:, :3].copy()
    s.run(1)                                                                           # step 6
    one = sr.products(sr.rho(snap, box, modes, types, 2))
    assert sf.samples == 1 and (np.abs(sf.sums - one) <= bound / 3).all()
    with pytest.raises(ValueError, match="entries"):
        analyze.StructureFactor(pse, modes, types=types[:-1])
    assert s.analyzers == [sf]
    # a tilting box: the sums are per integer mode, there is no one k
    s.box_tilt_variant = variant.shear_variant(shear_function.steady(dt=s.dt, shear_rate=2.0), 2000, max_strain=0.5)
    s.run(3)                                                                           # steps 7 (no sample), 8 (sample), 9
    assert sf.samples == 2 and sf.boxes[0] == box and sf.boxes[1] != box and sf.boxes[1][:3] == box[:3]
    with pytest.raises(ValueError, match="boxes of the samples differ"):
        sf.k
    with pytest.raises(ValueError, match="boxes of the samples differ"):
        sf.shell_average(8)
    assert sf.S().shape == (nk,)                                                       # per integer mode it is still readable


def test_analyzer_on_a_group(restored_context):
    from pse_amd import analyze
    box = sr.TILTED
    pos, types = points("tilted"), types_of(NMAX, 2)
    members = np.arange(0, NMAX - 50)
    s, pse = system(pos, box, members)
    modes = SETS["half3"]
    sf = analyze.StructureFactor(pse, modes, types=types)
    s.run(1)
    r = sr.rho(pos[members], box, modes, types[members], 2)
    counts = np.bincount(types[members], minlength=2)
    want = sr.products(r)[1] / np.sqrt(counts[0] * counts[1])
    assert np.abs(sf.S(0, 1) - want).max() <= 2.0 * len(members) * sr.tol(modes, len(members)).max() / np.sqrt(counts[0] * counts[1])


def test_analyzer_dies_with_the_engine_that_set_params_replaces(restored_context):
    """The device object does not outlive its handle: after setParams() the analyzer says so, nothing is freed twice, and a new one
    on the new handle sums what the old one summed (tests/test_gpu_provider_lifetime.py)."""
    from pse_amd import analyze
    box = sr.CUBIC
    pos = points("cubic", 300)
    s, pse = system(pos, box)
    types = types_of(300, 2)
    modes = SETS["half3"]
    old = analyze.StructureFactor(pse, modes, types=types)
    s.run(1)
    kept = old.sums
    assert np.abs(kept).max() > 100.0 and pse.engine.serial == 1
    pse.cpp_method.setParams()                                     # a new handle; pse_destroy freed the device object
    assert pse.engine.serial == 2
    with pytest.raises(ValueError, match="setParams"):
        old.analyze(0)
    with pytest.raises(ValueError, match="setParams"):
        old.density()
    assert np.array_equal(old.sums, kept) and old.samples == 1     # the sums are a tensor of the analyzer's own: still readable
    del s.analyzers[:]
    with _Unraisable() as quiet:
        del old
        gc.collect()
    assert quiet.seen == []
    new = analyze.StructureFactor(pse, modes, types=types)
    snap = s.pos.cpu().numpy()[:, :3].copy()
    new.analyze(0)
    assert new.samples == 1 and (np.abs(new.sums - sr.products(sr.rho(snap, box, modes, types, 2))) <= 2.0 * 300 * sr.tol(modes, 300)[None, :]).all()
    s.analyzers.remove(new)
    with _Unraisable() as quiet:                                   # a collected analyzer frees its object, the handle lives on
        del new
        gc.collect()
    assert quiet.seen == [] and s.analyzers == []
