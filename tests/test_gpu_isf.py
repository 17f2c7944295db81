"""GPU tests of the intermediate scattering functions (pse_isf_create, pse_isf_sample, pse_isf_store, pse_isf_correlate) and of
analyze.IntermediateScattering on top of them.  References, bounds and inputs are those of tests/isf_ref.py, validated on the CPU by
tests/test_isf_cpu.py.

1. Exact: on the dyadic inputs (every fractional coordinate a multiple of 1/4 in a box where s is computed without rounding) self and
   coll equal the integer reference bit for bit, also after every particle has moved by its own lattice vector -- sincospi is exact
   at multiples of 1/2, and then nothing rounds.  The lists of pairs (1, 2, 63, 64 pairs, a slot for several rows, a slot
   overwritten, rows that no pair names) are tested on these inputs: every value is exact.
2. General positions: self within tol = n_a (4e-14 + 1.2e-16 n_a + 8.4e-15 s_max sum|m_i|) of the extended-precision reference; rho and
   static_sums bit-equal to pse_structure_factor_accumulate; coll within 4 x 2^-53 (|re re| + |im im|) of the product of the device's
   own rho bits.  Rows 1 .. 513 (a span is 256 particles), three boxes, the mode sets from one mode to the corners at +-4096 (a wave
   is 64 segments: 128 scattered modes), 1, 2, 3 and 8 types with an empty one, a group, a span of 512.
3. Queue-only: equal bits on repetition, a permuted list, a captured graph; the raw C-ABI: refusals write nothing, a slab rank works.
4. The analyzer through System.run with prescribed velocities: a uniform drift, a shear that flips, affine motion."""
import ctypes
import functools
import gc

import numpy as np
import pytest

from conftest import to4
import isf_ref as ir
import structure_factor_ref as sr
from test_gpu_msd import PrescribedMotion, restored_context  # noqa: F401
from test_gpu_provider_lifetime import _Unraisable

pytestmark = pytest.mark.gpu

NMAX = ir.NMAX
INVALID = -1
SETS = ir.mode_sets()
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def engine(name):
    import pse_amd
    if name in ir.DYADIC_BOXES:
        return pse_amd.Engine(NMAX, ir.DYADIC_BOXES[name], xi=1.0, error=1e-3)
    return pse_amd.Engine(NMAX, sr.BOXES[name], xi=0.5, error=1e-3)


def dev_group(members):
    import torch
    return None if members is None else torch.tensor(np.asarray(members), dtype=torch.int32, device="cuda")


def cplx(t):
    r = t.cpu().numpy()
    return r[..., 0] + 1j * r[..., 1]


class Run:
    """An object on `eng` with the origins `orgs` sampled and stored in slots 0, 1, ... and `now` in the current buffer; rho_now and
    rho_org[k] are what pse_isf_sample wrote (complex, (ntypes, nk))."""

    def __init__(self, eng, now, orgs, modes, types=None, ntypes=1, members=None, norigins=None, static=None):
        import torch
        self.eng, self.ntypes, self.nk = eng, ntypes, len(modes)
        self.isf = eng.isf_origins(types, ntypes, modes, norigins or len(orgs))
        assert (self.isf.nk, self.isf.ntypes, self.isf.norigins) == (len(modes), ntypes, norigins or len(orgs))
        self.group = dev_group(members)
        rho = torch.full((ntypes, self.nk, 2), np.nan, dtype=torch.float64, device="cuda")
        self.rho_org = []
        for k, org in enumerate(orgs):
            eng.isf_sample(to4(org), self.isf, rho=rho, group=self.group)
            eng.isf_store(self.isf, k)
            self.rho_org.append(cplx(rho))
        self.pos = to4(now)
        eng.isf_sample(self.pos, self.isf, rho=rho, static_sums=static, group=self.group)
        self.rho_now = cplx(rho)

    def correlate(self, slots=(0,), rows=(0,), nrows=1, self_part=True, coll=True, fill=0.0):
        import torch
        s = torch.full((nrows, self.ntypes, self.nk, 2), fill, dtype=torch.float64, device="cuda") if self_part else None
        c = torch.full((nrows, self.ntypes, self.ntypes, self.nk), fill, dtype=torch.float64, device="cuda") if coll else None
        assert self.eng.isf_correlate(self.isf, list(slots), list(rows), s, c) == (s, c)
        return (cplx(s) if self_part else None), (c.cpu().numpy() if coll else None)

    def close(self):
        self.isf.close()


def assert_coll(coll, rho_now, rho_org, what=""):
    """coll (ntypes, ntypes, nk) against the product of the device's own rho bits: a fused or unfused product and one addition."""
    a, b = rho_now[:, None, :], rho_org[None, :, :]
    want = a.real * b.real + a.imag * b.imag
    slack = 4.0 * U * (np.abs(a.real * b.real) + np.abs(a.imag * b.imag))
    worst = float((np.abs(coll - want) / np.where(slack > 0.0, slack, 1.0)).max())
    print(f"{what}: coll, worst error / slack = {worst:.3f}")
    assert (np.abs(coll - want) <= slack).all(), what


# -- 1. exact ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ir.DYADIC_BOXES))
def test_dyadic_inputs_are_exact_also_after_lattice_moves(name):
    box = ir.DYADIC_BOXES[name]
    now, org = ir.dyadic_case(name, NMAX)
    types = ir.types_of(NMAX, 3)
    moved = now + np.random.default_rng(7).integers(-3, 4, size=(NMAX, 3)).astype(np.float64) @ sr.lattice_vectors(box)
    for key in ("half3", "zline", "corners", "duplicates", "scattered128", "zero"):
        modes = SETS[key]
        want = ir.self_exact(now, org, box, modes, types, 3)
        r_now, r_org = ir.rho_exact(now, box, modes, types, 3), ir.rho_exact(org, box, modes, types, 3)
        for frame in (now, moved):
            run = Run(engine(name), frame, [org], modes, types, 3)
            got, coll = run.correlate()
            assert np.array_equal(run.rho_now, r_now) and np.array_equal(run.rho_org[0], r_org), key
            assert np.array_equal(got[0], want), key
            assert np.array_equal(coll[0], ir.coll_part(r_now, r_org)), key
            run.close()
        if key == "zero":
            counts = np.bincount(types, minlength=3)
            assert np.array_equal(want[:, 0], counts) and np.array_equal(coll[0, :, :, 0], np.outer(counts, counts))


@pytest.mark.parametrize("key", ["zline", "scattered129", "one"])
@pytest.mark.parametrize("npairs", [1, 2, 63, 64])
def test_lists_of_pairs(npairs, key):
    """npairs pairs over four slots -- every slot is listed for several rows --, the rows a permutation of a longer list: the rows
    that no pair names keep their NaN, the others hold the exact sums of their slot.  26 long segments, 65 short ones and a single
    segment per pair: a wave of 64 items holds 3, 1 and 64 pairs."""
    name = "tilt16"
    box, modes = ir.DYADIC_BOXES[name], SETS[key]
    n, nslots, nrows = 300, 4, npairs + 3
    now = ir.dyadic_case(name, n, seed=1)[0]
    orgs = [ir.dyadic_case(name, n, seed=10 + k)[1] for k in range(nslots)]
    types = ir.types_of(n, 2)
    run = Run(engine(name), now, orgs, modes, types, 2)
    rng = np.random.default_rng(npairs)
    slots, rows = rng.integers(0, nslots, npairs), rng.permutation(nrows)[:npairs]
    got, coll = run.correlate(slots, rows, nrows, fill=np.nan)
    named = np.zeros(nrows, dtype=bool)
    named[rows] = True
    assert np.isnan(got[~named].real).all() and np.isnan(got[~named].imag).all() and np.isnan(coll[~named]).all()
    want = [ir.self_exact(now, org, box, modes, types, 2) for org in orgs]
    r_now = ir.rho_exact(now, box, modes, types, 2)
    # (NaN + x is NaN: the named rows were filled with NaN as well, so correlate again into zeros)
    got, coll = run.correlate(slots, rows, nrows)
    for sl, row in zip(slots, rows):
        assert np.array_equal(got[row], want[sl]), (sl, row)
        assert np.array_equal(coll[row], ir.coll_part(r_now, ir.rho_exact(orgs[sl], box, modes, types, 2))), (sl, row)
    assert not got[~named].any() and not coll[~named].any()
    run.close()


def test_a_slot_overwritten_either_output_alone_and_two_calls_accumulate():
    import torch
    name = "cube16"
    box, modes = ir.DYADIC_BOXES[name], SETS["half3"]
    now, org = ir.dyadic_case(name, 257)
    other = ir.dyadic_case(name, 257, seed=5)[1]
    eng = engine(name)
    run = Run(eng, now, [org, org], modes)
    want, want_other = ir.self_exact(now, org, box, modes), ir.self_exact(now, other, box, modes)
    assert not np.array_equal(want, want_other)
    # slot 1 overwritten: sample the other origin, store it, sample `now` again
    eng.isf_sample(to4(other), run.isf)
    eng.isf_store(run.isf, 1)
    eng.isf_sample(run.pos, run.isf)
    got, coll = run.correlate((0, 1), (1, 0), 2)
    assert np.array_equal(got[1], want) and np.array_equal(got[0], want_other)
    # self alone and coll alone: the same bits
    s_only, none = run.correlate((0, 1), (1, 0), 2, coll=False)
    none2, c_only = run.correlate((0, 1), (1, 0), 2, self_part=False)
    assert none is None and none2 is None and np.array_equal(s_only, got) and np.array_equal(c_only, coll)
    # two calls accumulate, onto what was there
    s = torch.full((2, 1, len(modes), 2), 5.0, dtype=torch.float64, device="cuda")
    c = torch.full((2, 1, 1, len(modes)), -3.0, dtype=torch.float64, device="cuda")
    for _ in range(2):
        eng.isf_correlate(run.isf, [0, 1], [1, 0], s, c)
    assert np.array_equal(cplx(s), (5.0 + 5.0j) + 2 * got) and np.array_equal(c.cpu().numpy(), -3.0 + 2 * coll)
    # the Python layer's own checks
    for args, word in ((([0], [0], None, None), "both None"), (([0], [0], s[:, :, :-1], None), "self_sums must be"),
                       (([0], [0], s, c[:1]), "coll must be"), (([0], [2], s, c), "row outside"), (([2], [0], s, c), "slot outside"),
                       (([0, 1], [1, 1], s, c), "row twice")):
        with pytest.raises(ValueError, match=word):
            eng.isf_correlate(run.isf, *args)
    with pytest.raises(ValueError, match="slot = 2"):
        eng.isf_store(run.isf, 2)
    fresh = eng.isf_origins(None, 1, modes, 2)
    with pytest.raises(ValueError, match="no isf_sample yet"):
        eng.isf_store(fresh, 0)
    eng.isf_sample(run.pos, fresh)
    with pytest.raises(ValueError, match="never stored"):
        eng.isf_correlate(fresh, [0], [0], s, c)
    eng.isf_store(fresh, 0)
    eng.isf_sample(run.pos[:200], fresh)
    with pytest.raises(ValueError, match="stored with N = 257: the current sample has N = 200"):
        eng.isf_correlate(fresh, [0], [0], s, c)
    fresh.close()
    run.close()
    with pytest.raises(ValueError, match="closed"):
        eng.isf_sample(run.pos, run.isf)
    with pytest.raises(ValueError, match="closed"):
        eng.isf_correlate(run.isf, [0], [0], s, c)


# -- 2. general positions --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference(case):
    """The extended-precision reference of a general case, computed once."""
    want, counts = ir.case_reference(case)
    want.setflags(write=False)
    return want, counts


@pytest.mark.parametrize("case", ir.general_cases(), ids=lambda c: c[0])
def test_general_positions(case):
    """self within the bound of the reference; rho and static_sums the bits of pse_structure_factor_accumulate; coll within four
    roundings of the product of the device's own rho."""
    import torch
    ir.need_extended_precision()
    box, now, org, modes, types, ntypes, members = ir.case_inputs(case)
    eng = engine(case[1])
    npt = ntypes * (ntypes + 1) // 2
    pre = np.random.default_rng(4).uniform(-1e3, 1e3, size=(npt, len(modes)))
    static = torch.tensor(pre, device="cuda")
    run = Run(eng, now, [org], modes, types, ntypes, members, static=static)
    got, coll = run.correlate()
    want, counts = reference(case)
    ratio = ir.worst_ratio(got[0], want, modes, counts)
    print(f"{case[0]}: self, worst error / tol = {ratio:.4f}")
    assert np.isfinite(got.view(np.float64)).all() and ratio <= 1.0
    # the structure-factor pass on the same inputs: the same bits in rho and in what was added to the sums
    sf = eng.structure_factor(types, ntypes, modes)
    rho = torch.empty((ntypes, len(modes), 2), dtype=torch.float64, device="cuda")
    sums = torch.tensor(pre, device="cuda")
    eng.structure_factor_accumulate(run.pos, sf, rho=rho, sums=sums, group=run.group)
    assert np.array_equal(cplx(rho), run.rho_now) and torch.equal(sums, static)
    sf.close()
    assert_coll(coll[0], run.rho_now, run.rho_org[0], case[0])
    if case[3] == "zero":
        assert np.array_equal(got[0][:, 0], counts) and np.array_equal(coll[0][:, :, 0], np.outer(counts, counts))
    run.close()


def test_lattice_shifts_between_origin_and_now():
    """Every particle moved by its own lattice vector, the tilted one included, out to |s| = 3.5: the same self, within the bound at
    that s_max; no images and no unwrapping are needed."""
    ir.need_extended_precision()
    name = "tilted"
    case = (f"{name}-shift", name, NMAX, "corners", 1, None, False)
    box, now, org, modes, _, _, _ = ir.case_inputs(case)
    moved = now + np.random.default_rng(31).integers(-3, 4, size=(NMAX, 3)).astype(np.float64) @ sr.lattice_vectors(box)
    smax = ir.s_max(box, moved, org)
    assert 3.0 < smax < 3.6
    for key in ("corners", "zline"):
        modes = SETS[key]
        run = Run(engine(name), moved, [org], modes)
        got, _ = run.correlate(coll=False)
        want, counts = reference((f"{name}-{key}", name, NMAX, key, 1, None, False))
        ratio = ir.worst_ratio(got[0], want, modes, counts, smax)
        print(f"shifted {key}: worst error / tol = {ratio:.4f}")
        assert ratio <= 1.0
        run.close()


def test_a_span_of_512():
    """n_max x ntypes x nk x 64 pairs beyond 2^24 partial sums: a row of the workspace covers 512 particles."""
    import pse_amd
    ir.need_extended_precision()
    name = "cubic"
    case = (f"{name}-scattered128", name, NMAX, "scattered128", 1, None, False)
    box, now, org, modes, _, _, _ = ir.case_inputs(case)
    eng = pse_amd.Engine(600000, box, xi=0.5, error=1e-3)
    run = Run(eng, now, [org], modes)
    got, coll = run.correlate()
    want, counts = reference(case)
    assert ir.worst_ratio(got[0], want, modes, counts) <= 1.0
    assert_coll(coll[0], run.rho_now, run.rho_org[0], "span of 512")
    run.close()
    eng.close()


# -- 3. queue-only ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["half3", "zline", "scattered129"])
def test_equal_inputs_equal_bits_and_the_order_of_the_list_does_not_matter(key):
    name = "negative"
    box, now, org, modes, types, ntypes, _ = ir.case_inputs((key, name, NMAX, key, 2, None, False))
    eng = engine(name)
    run = Run(eng, now, [org, now], modes, types, ntypes)
    first = run.correlate((0, 1), (0, 1), 2)
    again = run.correlate((0, 1), (0, 1), 2)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    # against itself: N_a, and the static products
    counts = np.bincount(types, minlength=2)
    assert np.array_equal(first[0][1], counts[:, None] * np.ones(len(modes)))
    run.close()
    # a permuted mode list: the same bits, permuted -- the value of a mode is a function of the mode SET
    perm = np.random.default_rng(8).permutation(len(modes))
    run = Run(eng, now, [org, now], modes[perm], types, ntypes)
    got = run.correlate((0, 1), (0, 1), 2)
    assert np.array_equal(got[0], first[0][..., perm]) and np.array_equal(got[1], first[1][..., perm])
    run.close()


def test_duplicates_have_the_same_bits_in_every_place():
    name = "tilted"
    box, now, org, modes, _, _, _ = ir.case_inputs(("dup", name, NMAX, "duplicates", 1, None, False))
    run = Run(engine(name), now, [org], modes)
    got, coll = run.correlate()
    for x in (got[0, 0], coll[0, 0, 0]):
        assert x[0] == x[2] == x[4] and x[3] == x[5]
    assert got[0, 0, 3] == NMAX and coll[0, 0, 0, 3] == NMAX * NMAX
    run.close()


def test_sample_correlate_and_store_captured_into_a_graph_replay_the_eager_bits():
    import pse_amd
    import torch
    name = "tilted"
    box, now, org, modes, types, ntypes, _ = ir.case_inputs(("graph", name, NMAX, "half3", 2, None, False))
    eng = pse_amd.Engine(NMAX, box, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    isf = eng.isf_origins(types, ntypes, modes, 2)
    nk = len(modes)
    pos = to4(org)
    s = torch.zeros((2, ntypes, nk, 2), dtype=torch.float64, device="cuda")
    c = torch.zeros((2, ntypes, ntypes, nk), dtype=torch.float64, device="cuda")
    static = torch.zeros((3, nk), dtype=torch.float64, device="cuda")

    def start():
        for t in (s, c, static):
            t.zero_()
        pos.copy_(to4(org))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            eng.isf_sample(pos, isf)
            eng.isf_store(isf, 0)
            eng.isf_store(isf, 1)
        st.synchronize()

    def sample():
        eng.isf_sample(pos, isf, static_sums=static)
        eng.isf_correlate(isf, [1, 0], [0, 1], s, c)
        eng.isf_store(isf, 1)

    frames = [now, 0.5 * (now + org)]
    start()
    eager = []
    for p in frames:
        pos.copy_(to4(p))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            sample()
        st.synchronize()
        eager.append([t.cpu().numpy().copy() for t in (s, c, static)])
    assert np.abs(eager[1][0] - 2 * eager[0][0]).max() > 0.0
    start()
    pos.copy_(to4(frames[0]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        sample()
    torch.cuda.synchronize()
    assert not s.cpu().numpy().any() and not static.cpu().numpy().any(), "a capture runs nothing"
    for k, p in enumerate(frames):
        pos.copy_(to4(p))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for t, want in zip((s, c, static), eager[k]):
            assert np.array_equal(t.cpu().numpy(), want), k
    isf.close()
    eng.close()


def test_refusals_write_nothing_and_a_slab_rank_works():
    """Raw C-ABI, as a C host would call it: a refused call leaves the outputs untouched, and the object works afterwards; the passes
    work on a slab rank's handle (positions are replicated there)."""
    import torch
    from pse_amd import _lib
    from pse_amd._lib import pse_params
    ir.need_extended_precision()
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731
    ints = lambda *v: np.array(v, dtype=np.int32)          # noqa: E731

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

    n, ntypes = 300, 2
    now, org = ir.configuration("cubic", n)
    types = ir.types_of(n, ntypes).astype(np.uint32)
    modes = np.ascontiguousarray(SETS["half3"], dtype=np.int32)
    nk = len(modes)
    rc, h = create(sr.CUBIC[0], n)
    assert rc == 0, msg()
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    f = ctypes.c_void_p(777)
    for word, kw in (("n = 301", dict(nn=n + 1)), ("nk = 4097", dict(k=4097)), ("norigins = 65", dict(no=65)), ("norigins = 0", dict(no=0))):
        a = dict(dict(nn=n, k=nk, no=2), **kw)
        assert lib.pse_isf_create(h, a["nn"], vp(types), ntypes, a["k"], vp(modes), a["no"], ctypes.byref(f)) == INVALID
        assert word in msg() and "pse_isf_create" in msg() and not f.value, (word, msg())
    assert lib.pse_isf_create(h, n, vp(types), ntypes, nk, vp(modes), 2, ctypes.byref(f)) == 0 and f.value, msg()
    dnow, dorg = to4(now), to4(org)
    rho = torch.full((ntypes, nk, 2), -5.0, dtype=torch.float64, device="cuda")
    s = torch.full((3, ntypes, nk, 2), -7.0, dtype=torch.float64, device="cuda")
    c = torch.full((3, ntypes, ntypes, nk), -9.0, dtype=torch.float64, device="cuda")

    def refused(fn, word, *args):
        assert getattr(lib, fn)(*args) == INVALID, (fn, word)
        assert word in msg() and fn in msg(), (word, msg())

    def corr(word, sl, ro, npairs=None, se=P(s), co=P(c), ff=f):
        """pse_isf_correlate with the lists sl, ro (kept alive through the call); word None: it must succeed."""
        sl, ro = ints(*sl), ints(*ro)
        rc = lib.pse_isf_correlate(ff, len(sl) if npairs is None else npairs, vp(sl), vp(ro), 3, se, co)
        assert (word is None and rc == 0) or (rc == INVALID and word in msg() and "pse_isf_correlate" in msg()), (word, rc, msg())

    refused("pse_isf_store", "no pse_isf_sample since create", f, 0)
    corr("no pse_isf_sample since create", (0,), (0,))
    refused("pse_isf_sample", "N = 0", f, P(dorg), None, 0, P(rho), None)
    refused("pse_isf_sample", "N = 301", f, P(dorg), None, n + 1, P(rho), None)
    refused("pse_isf_sample", "null pos", f, None, None, n, P(rho), None)
    refused("pse_isf_sample", "rho =", f, P(dorg), None, n, ctypes.c_void_p(rho.data_ptr() + 4), None)
    assert lib.pse_isf_sample(f, P(dorg), None, n, None, None) == 0, msg()
    corr("slot 0, which was never stored", (0,), (0,))
    refused("pse_isf_store", "slot = 2 outside", f, 2)
    assert lib.pse_isf_store(f, 0) == 0, msg()
    assert lib.pse_isf_sample(f, P(dnow), None, n - 1, None, None) == 0, msg()
    corr("stored with N = 300: the current sample has N = 299", (0,), (0,))
    assert lib.pse_isf_sample(f, P(dnow), None, n, None, None) == 0, msg()
    corr("npairs = 65", (0,), (0,), npairs=65)
    corr("names the slot 1, which was never stored", (0, 1), (0, 1))
    corr("names the row 3 outside", (0, 0), (0, 3))
    corr("both name the row 2", (0, 0), (2, 2))
    corr("both null", (0,), (0,), se=None, co=None)
    corr("coll =", (0,), (0,), co=ctypes.c_void_p(c.data_ptr() + 4))
    torch.cuda.synchronize()
    assert np.all(rho.cpu().numpy() == -5.0) and np.all(s.cpu().numpy() == -7.0) and np.all(c.cpu().numpy() == -9.0)
    corr(None, (0, 0), (2, 0))
    got = cplx(s) + (7.0 + 7.0j)
    want = ir.self_part(now, org, sr.CUBIC, modes, types, ntypes)
    counts = np.bincount(types, minlength=ntypes)
    assert np.array_equal(got[0], got[2]) and not got[1].any() and ir.worst_ratio(got[0], want, modes, counts) <= 1.0
    assert np.all(c.cpu().numpy()[1] == -9.0) and np.abs(c.cpu().numpy()[0] + 9.0).max() > 10.0
    # a slab rank's handle: its box is 40^3
    fs = ctypes.c_void_p()
    assert lib.pse_isf_create(hs, n, vp(types), ntypes, nk, vp(modes), 1, ctypes.byref(fs)) == 0, msg()
    assert lib.pse_isf_sample(fs, P(dorg), None, n, None, None) == 0 and lib.pse_isf_store(fs, 0) == 0, msg()
    assert lib.pse_isf_sample(fs, P(dnow), None, n, P(rho), None) == 0, msg()
    s.zero_()
    corr(None, (0,), (1,), co=None, ff=fs)
    box40 = (40.0, 40.0, 40.0, 0.0)
    assert ir.worst_ratio(cplx(s)[1], ir.self_part(now, org, box40, modes, types, ntypes), modes, counts) <= 1.0
    assert sr.worst_ratio(cplx(rho), sr.rho(now, box40, modes, types, ntypes), modes, n) <= 1.0
    assert lib.pse_isf_destroy(fs) == 0 and lib.pse_isf_destroy(None) == 0
    for hh in (h, hs):                                                                 # f is still alive: it goes with its handle
        assert lib.pse_destroy(hh) == 0


# -- 4. analyze.IntermediateScattering --------------------------------------------------------------------------------------------------

class Recorder:
    """An analyzer that notes the flips of the box at every sample."""

    def __init__(self, system):
        self.system, self.flips = system, []
        system.analyzers.append(self)

    def analyze(self, timestep):
        self.flips.append(self.system.tilt_flips)


def prescribed(vel, rate, steps, nlags, every, modes, **kw):
    from pse_amd import analyze, shear_function, variant
    from pse_amd.system import System
    dt = 2.0 ** -6
    s = System.create_lattice_sc(4.0, 3, dt=dt)                                # 27 particles at -4, 0, 4 in a box of 12: dyadic
    mover = PrescribedMotion(s, np.broadcast_to(np.asarray(vel, dtype=np.float64), (s.n, 3)).copy(), rate)
    if rate:
        s.box_tilt_variant = variant.shear_variant(shear_function.steady(dt=dt, shear_rate=rate), 100000, max_strain=0.5)
    rec = Recorder(s)
    isf = analyze.IntermediateScattering(mover, modes, nlags, origin_every=every, **kw)
    s.run(steps)
    return s, isf, rec, mover


def test_a_uniform_drift_through_system_run(restored_context):
    """Every particle moves with v = (8, -24, 16): Fs(m, lag) = cos(2 pi m.v lag dt / L) whatever the wraps through the faces, and the
    collective part of the rigidly moving lattice is S(m) times the same cosine; counts, lags, S and f."""
    ir.need_extended_precision()
    modes = SETS["half3"]
    v, nlags, every, steps, L, dt = np.array([8.0, -24.0, 16.0]), 6, 2, 20, 12.0, 2.0 ** -6
    types = np.arange(27) % 3
    s, isf, rec, mover = prescribed(v, 0.0, steps, nlags, every, modes, types=types, period=1)
    assert np.abs(s.image.cpu().numpy()).max() >= 1                                    # particles went through the faces
    assert isf.samples == steps and np.array_equal(isf.lags, np.arange(1, nlags + 1))
    want_counts = [sum(1 for o in range(0, steps, every) for t in range(steps) if t - o == lag) for lag in range(1, nlags + 1)]
    assert isf.counts.tolist() == want_counts and len(isf.boxes) == steps
    lag = np.arange(1, nlags + 1).astype(ir.LD)[:, None]
    phase = (modes.astype(ir.LD) @ (v.astype(ir.LD) * ir.LD(dt) / ir.LD(L)))[None, :] * lag
    want = np.cos(ir.LD(8) * np.arctan(ir.LD(1)) * phase).astype(np.float64)
    for a in (None, 0, 1, 2):
        n = 27 if a is None else 9
        got = isf.Fs(a)
        ratio = float((np.abs(got - want) / (ir.tol(modes, n, 0.5)[None, :] / n)).max())
        print(f"drift, type {a}: worst error of Fs / bound = {ratio:.4f}")
        assert got.shape == (nlags, len(modes)) and ratio <= 1.0
    # the lattice moves rigidly: F(m, lag) = S(m) cos(...), S = 27 on the lattice's own modes and 0 elsewhere
    S = isf.S()
    on = (np.abs(modes) % 3 == 0).all(axis=1)
    assert np.abs(S[on] - 27.0).max() <= 1e-9 and np.abs(S[~on]).max() <= 1e-9
    assert np.abs(isf.F() - S[None, :] * want).max() <= 1e-9
    assert np.abs(isf.f()[:, on] - want[:, on]).max() <= 1e-10
    assert np.abs(isf.F(0, 1) - isf.collective_sums[:, 0, 1] / (np.array(want_counts)[:, None] * 9.0)).max() <= 1e-12
    assert isf.k.shape == (len(modes), 3) and isf.self_sums.shape == (nlags, 3, len(modes)) and isf.static_sums.shape == (6, len(modes))
    centres, mean, cnt = isf.shell_average(isf.Fs(), 4)
    assert mean.shape == (nlags, 4) and cnt.sum() == len(modes)
    tau = isf.relaxation_times("self")
    assert tau.shape == (len(modes),) and np.nanmin(tau) > 0.0
    with pytest.raises(ValueError, match="which must be"):
        isf.relaxation_times("both")
    with pytest.raises(ValueError, match="both types or neither"):
        isf.F(0)
    isf.reset()
    assert isf.samples == 0 and not isf.self_sums.any() and not isf.collective_sums.any() and isf.boxes == [] and not isf.counts.any()
    mover.engine.close()


def test_a_shear_that_flips_never_pairs_samples_across_the_flip(restored_context):
    """Particles at rest in a box sheared at rate 2: the motion is purely affine.  The tilt grows by 1/32 per step and flips at step
    16: no count pairs a sample after the flip with an origin before it, and between the flips Fs is exactly 1."""
    modes = SETS["half3"]
    nlags, every, steps = 6, 2, 40
    s, isf, rec, mover = prescribed((0.0, 0.0, 0.0), 2.0, steps, nlags, every, modes, collective=False)
    assert s.tilt_flips == 1 and rec.flips[0] == 0 and rec.flips[-1] == 1
    flip = rec.flips.index(1)                                                          # the first sample in the new labelling
    want = [sum(1 for o in range(0, steps, every) for t in range(steps) if t - o == lag and not (o < flip <= t)) for lag in range(1, nlags + 1)]
    plain = [sum(1 for o in range(0, steps, every) for t in range(steps) if t - o == lag) for lag in range(1, nlags + 1)]
    assert isf.counts.tolist() == want and want != plain and 8 < flip < 24
    assert np.array_equal(isf.Fs(), np.ones((nlags, len(modes))))                       # exactly: affine motion leaves s where it was
    with pytest.raises(ValueError, match="boxes of the samples differ"):
        isf.k
    with pytest.raises(ValueError, match="collective=False"):
        isf.collective_sums
    # the same run with a drift across the flow on top: the advected modes see the drift alone, through the flip
    v = np.array([0.0, 0.0, 16.0])
    s2, isf2, rec2, mover2 = prescribed(v, 2.0, steps, nlags, every, modes, collective=False)
    lag = np.arange(1, nlags + 1)[:, None]
    want2 = np.cos(2.0 * np.pi * (modes[:, 2] * 16.0 * 2.0 ** -6 / 12.0)[None, :] * lag)
    assert isf2.counts.tolist() == want and np.abs(isf2.Fs() - want2).max() <= 1e-12
    for m in (mover, mover2):
        m.engine.close()


def test_analyzer_dies_with_its_engine_and_frees_its_object(restored_context):
    from pse_amd import analyze
    modes = SETS["half3"]
    s, isf, rec, mover = prescribed((8.0, 0.0, 0.0), 0.0, 3, 4, 1, modes)
    kept = isf.self_sums
    assert np.abs(kept).max() > 1.0 and s.analyzers == [rec, isf]
    with pytest.raises(ValueError, match="entries"):
        analyze.IntermediateScattering(mover, modes, 4, types=np.zeros(5, dtype=int))
    assert s.analyzers == [rec, isf]
    mover.engine.close()                                           # pse_destroy frees the device object
    with pytest.raises(ValueError, match="went with the engine"):
        isf.analyze(0)
    assert np.array_equal(isf.self_sums, kept)                     # the sums are tensors of the analyzer's own: still readable
    del s.analyzers[:]
    with _Unraisable() as quiet:
        del isf
        gc.collect()
    assert quiet.seen == []
