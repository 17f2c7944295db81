"""pse_molecules_compute and analyze.Conformations on the device against the exact rational reference of tests/conformation_ref.py:
bit for bit on dyadic inputs whose every quantity is exact in float64, within the bound derived from the kernel's order of operations
(tests/conformation_cases.py: bounds) on general positions at the wave and tile edges, every output alone, the analyzer through
System.run under a shear that flips, a captured graph and a slab rank's handle."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
import conformation_cases as cc
import conformation_ref as cr

pytestmark = pytest.mark.gpu

NMAX = 4400
INVALID = -1


@functools.lru_cache(maxsize=None)
def engine(lengths):
    import pse_amd
    return pse_amd.Engine(NMAX, lengths + (0.0,), xi=0.5, error=1e-3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    """Equal bit for bit, any NaN standing for any NaN (the reference's NaN is not the device's)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(np.where(nan, 0.0, got)), bits(np.where(nan, 0.0, want))))


def compute(box, n, bonds, pos, mol_types=None, ntypes=1, nbins=0, rg_max=None, ree_max=None, calls=1, only=None):
    """One molecule object on the engine of the box's lengths, `calls` computes from zeroed outputs (unfolded: from -3).  Returns the
    outputs as NumPy arrays; only=name: that output alone, the others None."""
    import torch
    eng = engine(tuple(box[:3]))
    eng.set_box(*box)
    mol = eng.molecule_topology(bonds, mol_types, ntypes, nbins, rg_max, ree_max, n=n)
    dev = "cuda"
    out = dict(rows=torch.zeros((mol.nmol, 14), dtype=torch.float64, device=dev),
               unfolded=torch.full((n, 4), -3.0, dtype=torch.float64, device=dev),
               sums=torch.zeros((ntypes, 14), dtype=torch.float64, device=dev),
               sample=torch.zeros((ntypes, 14), dtype=torch.float64, device=dev),
               hist=torch.zeros((2, ntypes, nbins + 1), dtype=torch.int64, device=dev) if nbins else None)
    if only is not None:
        out = {k: (v if k == only else None) for k, v in out.items()}
    p = to4(pos)
    for _ in range(calls):
        eng.molecules_compute(p, mol, **out)
    torch.cuda.synchronize()
    res = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    res["nmol"], res["nlinear"], res["nmol_type"] = mol.nmol, mol.nlinear, mol.nmol_type
    mol.close()
    eng.set_box(*(tuple(box[:3]) + (0.0,)))
    return res


# -- 1. dyadic inputs: every quantity exact, every output bit for bit (conformation_cases.dyadic_cases says why they are) ----------

DYADIC, HIST = cc.DYADIC, cc.HIST


@functools.lru_cache(maxsize=None)
def dyadic_reference(name):
    box, n, bonds, pos, types, ntypes = DYADIC[name]
    return cr.reference(pos, box, bonds, types, ntypes, **HIST)


@pytest.mark.parametrize("name", sorted(DYADIC))
def test_dyadic_inputs_bit_for_bit(name):
    """rows, unfolded, sample, sums and hist equal the reference bit for bit; two calls give equal bits, and sums after two calls is
    twice sample, exactly; re-imaging every bead by its own lattice vector changes nothing but c and the unfolded positions, which move
    by the root's lattice vector."""
    box, n, bonds, pos, types, ntypes = DYADIC[name]
    ref = dyadic_reference(name)
    assert ref["image_margin"] > 1e-6 and ref["bin_margin"] > 1e-9
    assert ref["inexact"] == 0
    if ref["inexact4"]:                                                        # rounded fourth moments: then one molecule per type
        assert len(ref["mols"]) == 1 or np.bincount(types, minlength=ntypes).max() == 1
    got = compute(box, n, bonds, pos, types, ntypes, **HIST)
    members = ref["mol_of"] >= 0
    assert same_bits(got["rows"], ref["rows"])
    assert same_bits(got["unfolded"][members], ref["unfolded"][members]) and np.all(got["unfolded"][~members] == -3.0)
    assert same_bits(got["sample"], ref["sums"]) and same_bits(got["sums"], ref["sums"])
    assert np.array_equal(got["hist"], ref["hist"])
    assert got["nmol"] == len(ref["mols"])
    t = np.zeros(got["nmol"], dtype=int) if types is None else types
    assert np.array_equal(got["nmol_type"], np.bincount(t, minlength=ntypes))
    assert np.array_equal(got["nlinear"], np.bincount(t[ref["linear"]], minlength=ntypes))
    twice = compute(box, n, bonds, pos, types, ntypes, **HIST, calls=2)
    assert same_bits(twice["rows"], got["rows"]) and same_bits(twice["sample"], got["sample"]) and same_bits(twice["unfolded"], got["unfolded"])
    assert same_bits(twice["sums"], 2.0 * got["sample"]) and np.array_equal(twice["hist"], 2 * got["hist"])
    moved = cc.reimage(pos, box, np.random.default_rng(3))
    again = compute(box, n, bonds, moved, types, ntypes, **HIST)
    assert same_bits(again["rows"][:, 3:], got["rows"][:, 3:]) and same_bits(again["sums"], got["sums"])
    assert np.array_equal(again["hist"], got["hist"])
    shift = (moved - pos)[[mo["members"][0] for mo in ref["mols"]]]
    assert same_bits(again["rows"][:, :3], got["rows"][:, :3] + shift)
    assert same_bits(again["unfolded"][members, :3], got["unfolded"][members, :3] + shift[ref["mol_of"][members]])


# -- 2. general positions at the wave and tile edges --------------------------------------------------------------------------------------

EDGES, EDGE_HIST, edge_case = cc.EDGES, cc.EDGE_HIST, cc.edge_case


@functools.lru_cache(maxsize=None)
def edge_reference(k):
    lengths, xy, ntypes, seed = EDGES[k]
    box, n, bonds, pos, types = edge_case(lengths, xy, ntypes, seed)
    return cr.reference(pos, box, bonds, types, ntypes, **EDGE_HIST)


@pytest.mark.parametrize("k", range(len(EDGES)))
def test_sizes_at_the_wave_and_tile_edges_within_the_bound(k):
    """Sizes 2, 3, 63, 64, 65, 255, 257 and 1023, a star, rings and a comb, mixed in one tile, a tile filled to exactly 1024 and a
    molecule pushed to the next, 1, 2 and 8 types with empty types and a type without a linear molecule, both boxes at the tilt limit:
    every float64 output within the bound of conformation_cases.bounds of the once-rounded exact value, the integers equal.  The
    inputs are held clear of every half box (1e-6 L) and of every bin edge (1e-9 relative): tests/test_conformations_cpu.py checks the
    same cases' margins and that a float64 restatement of the kernel's order of operations keeps the bound."""
    lengths, xy, ntypes, seed = EDGES[k]
    box, n, bonds, pos, types = edge_case(lengths, xy, ntypes, seed)
    ref = edge_reference(k)
    assert ref["image_margin"] > 1e-6 and ref["bin_margin"] > 1e-9
    got = compute(box, n, bonds, pos, types, ntypes, **EDGE_HIST)
    rows_tol, unf_tol, _, _ = cc.bounds(ref, box)
    err = np.abs(got["rows"] - ref["rows"])
    print("rows: largest error / bound", np.nanmax(err / rows_tol))
    assert np.array_equal(np.isnan(got["rows"]), np.isnan(ref["rows"]))
    assert np.all(np.isnan(got["rows"][~ref["linear"], 10:])) and not np.isnan(got["rows"][:, :10]).any()
    assert np.all(err[~np.isnan(err)] <= rows_tol[~np.isnan(err)])
    members = ref["mol_of"] >= 0
    uerr = np.abs(got["unfolded"][members, :3] - ref["unfolded"][members, :3]).max(axis=1)
    assert np.all(uerr <= unf_tol[ref["mol_of"][members]])
    assert np.array_equal(got["unfolded"][members, 3], ref["mol_of"][members].astype(float))
    assert np.all(got["unfolded"][~members] == -3.0)
    stol = cc.sums_bound(ref, box, types, ntypes)
    serr = np.abs(got["sums"] - ref["sums"])
    print("sums: largest error / bound", (serr / np.maximum(stol, 1e-300)).max())
    assert np.all(serr <= stol) and same_bits(got["sample"], got["sums"])
    t = np.zeros(got["nmol"], dtype=int) if types is None else types
    empty = np.bincount(t, minlength=ntypes) == 0
    assert same_bits(got["sums"][empty], np.zeros((int(empty.sum()), 14)))                 # exactly +0.0
    nolinear = np.bincount(t[ref["linear"]], minlength=ntypes) == 0
    assert same_bits(got["sums"][nolinear, 7:], np.zeros((int(nolinear.sum()), 7)))
    assert np.array_equal(got["hist"], ref["hist"])
    assert np.array_equal(got["nmol_type"], np.bincount(t, minlength=ntypes))
    assert np.array_equal(got["nlinear"], np.bincount(t[ref["linear"]], minlength=ntypes))


# -- 3. every output alone, nbins == 0 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("only", ["rows", "unfolded", "sums", "sample", "hist"])
def test_every_output_alone_gives_the_bits_of_the_full_call(only):
    lengths, xy, ntypes, seed = EDGES[1]
    box, n, bonds, pos, types = edge_case(lengths, xy, ntypes, seed)
    full = compute(box, n, bonds, pos, types, ntypes, **EDGE_HIST)
    alone = compute(box, n, bonds, pos, types, ntypes, **EDGE_HIST, only=only)
    assert all(alone[k] is None for k in ("rows", "unfolded", "sums", "sample", "hist") if k != only)
    if only == "hist":
        assert np.array_equal(alone["hist"], full["hist"])
    else:
        assert same_bits(alone[only], full[only])


def test_without_bins_there_is_no_histogram():
    import torch
    box, n, bonds, pos, types, ntypes = DYADIC["four 64"]
    got = compute(box, n, bonds, pos, types, ntypes)
    assert got["hist"] is None and same_bits(got["sums"], dyadic_reference("four 64")["sums"])
    eng = engine(tuple(box[:3]))
    mol = eng.molecule_topology(bonds, types, ntypes, n=n)
    with pytest.raises(ValueError, match="nbins = 0"):
        eng.molecules_compute(to4(pos), mol, hist=torch.zeros((2, ntypes, 1), dtype=torch.int64, device="cuda"))
    mol.close()


# -- 4. analyze.Conformations on a System -------------------------------------------------------------------------------------------------

@pytest.fixture
def restored_context():
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


class Snapshots:
    def __init__(self, system):
        self.system, self.frames = system, []
        system.analyzers.append(self)

    def analyze(self, timestep):
        s = self.system
        self.frames.append((int(timestep), s.pos.cpu().numpy()[:, :3].copy(), tuple(s.box)))


def chains_system(dt):
    from pse_amd.system import System
    rng = np.random.default_rng(21)
    shapes = [("chain", 8)] * 3 + [("chain", 5)] * 2 + [("star", 6)]
    n, bonds, sizes, kinds = cc.build(shapes, gaps=(0, 1))
    n += 1
    box = (16.0, 16.0, 16.0, 0.0)
    pos = cc.wrap(cc.place(n, bonds, box, rng, 2.5), box)
    return System(pos, box, dt=dt), n, bonds, sizes


def test_analyzer_through_system_run_under_a_shear_that_flips(restored_context):
    """analyze.Conformations made from a forces.Bonds, molecule_types="size" with names, a period, a ring shorter than the run, reset():
    every row of series() equals the exact reference at the positions and the box of its step within the bound -- through the
    Lees-Edwards flip at step 16 --, and per_molecule() and unfolded() the reference at the final positions."""
    from pse_amd import analyze, forces, integrate, shear_function, variant
    dt, rate = 2.0 ** -6, 2.0                                                  # the tilt grows by 1/32 per step: the flip at step 16
    s, n, bonds, sizes = chains_system(dt)
    fn = shear_function.steady(dt=dt, shear_rate=rate)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3, function_form=fn)
    s.box_tilt_variant = variant.shear_variant(fn, 100000, max_strain=0.5)
    fb = forces.Bonds(pse, bonds, kind="harmonic", k=20.0, r0=2.0)
    conf = analyze.Conformations(pse, fb, molecule_types="size", type_names=["five", "six", "eight"], period=3, capacity=4, nbins=16,
                                 rg_max=8.0, ree_max=24.0)
    assert conf.ntypes == 3 and list(conf.size_values) == [5, 6, 8] and conf.nmol == 6
    assert np.array_equal(conf.sizes(), sizes) and list(conf.nmol_type) == [2, 1, 3] and list(conf.nlinear) == [2, 0, 3]
    snaps = Snapshots(s)
    s.run(24)
    assert s.tilt_flips >= 1
    sampled = [f for f in snaps.frames if f[0] % 3 == 0]
    assert conf.samples == len(sampled) == 8
    ser = conf.series()
    assert ser.shape == (4, 1 + 3 * 14) and [int(t) for t in ser[:, 0]] == [f[0] for f in sampled[-4:]]
    types = np.searchsorted(conf.size_values, sizes)
    total = np.zeros((3, 14))
    for r, (step, pos, box) in enumerate(sampled):
        ref = cr.reference(pos, box, bonds, types, 3)
        assert ref["image_margin"] > 1e-6
        total += ref["sums"]
        if r >= 4:
            err = np.abs(ser[r - 4, 1:].reshape(3, 14) - ref["sums"])
            assert np.all(err <= cc.sums_bound(ref, box, types, 3)), (step, err.max())
    serr = np.abs(conf.sums() - total)
    assert np.all(serr <= 8 * cc.sums_bound(ref, box, types, 3) + 8 * cc.EPS * np.abs(total))
    assert abs(conf.rg2("eight") - total[2, :3].sum() / (8 * 3)) <= 1e-12 * conf.rg2("eight")
    assert abs(conf.ree2("five") - total[0, 7:10].sum() / (8 * 2)) <= 1e-12 * conf.ree2("five")
    assert np.isnan(conf.ree2("six")) and conf.gyration_tensor().shape == (3, 3)
    assert np.allclose(np.trace(conf.gyration_tensor()), total[:, :3].sum() / (8 * 6), rtol=1e-12)
    counts, edges = conf.histogram("rg")
    assert counts.sum() == 8 * 6 and edges.shape == (17,) and conf.histogram("ree", "six")[0].sum() == 0
    pos, box = s.pos.cpu().numpy()[:, :3].copy(), tuple(s.box)               # after the last step, in the box of that step
    ref = cr.reference(pos, box, bonds, types, 3)
    assert ref["image_margin"] > 1e-6
    rows = conf.per_molecule()
    rows_tol, unf_tol, _, _ = cc.bounds(ref, box)
    err = np.abs(rows - ref["rows"])
    assert np.array_equal(np.isnan(rows), np.isnan(ref["rows"])) and np.all(err[~np.isnan(err)] <= rows_tol[~np.isnan(err)])
    unf = conf.unfolded()
    members = ref["mol_of"] >= 0
    assert np.all(np.abs(unf[members, :3] - ref["unfolded"][members, :3]).max(axis=1) <= unf_tol[ref["mol_of"][members]])
    assert np.all(unf[~members, 3] == -1.0) and np.isnan(unf[~members, :3]).all()
    assert conf.samples == 8                                                   # the readers took no sample
    conf.reset()
    assert conf.samples == 0 and not conf.sums().any() and conf.series().shape == (0, 43) and conf.histogram("rg")[0].sum() == 0
    with pytest.raises(ValueError, match="no samples"):
        conf.rg2()
    s.run(3)
    assert conf.samples == 1 and int(conf.series()[0, 0]) == 24


# -- 5. queue-only: a captured graph ------------------------------------------------------------------------------------------------------

def test_a_captured_graph_replayed_on_moved_positions_gives_the_eager_bits():
    import torch
    import pse_amd
    lengths, xy, ntypes, seed = EDGES[2]
    box, n, bonds, pos, types = edge_case(lengths, xy, ntypes, seed)
    frames = [pos, cc.wrap(pos + 0.125, box)]
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    mol = eng.molecule_topology(bonds, types, ntypes, 20, 20.0, 90.0, n=n)
    p = to4(pos)
    out = dict(rows=torch.zeros((mol.nmol, 14), dtype=torch.float64, device="cuda"), unfolded=torch.zeros((n, 4), dtype=torch.float64, device="cuda"),
               sums=torch.zeros((ntypes, 14), dtype=torch.float64, device="cuda"), sample=torch.zeros((ntypes, 14), dtype=torch.float64, device="cuda"),
               hist=torch.zeros((2, ntypes, 21), dtype=torch.int64, device="cuda"))
    eager = []
    for f in frames:
        p.copy_(to4(f))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            eng.molecules_compute(p, mol, **out)
        st.synchronize()
        eager.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    assert np.abs(eager[1]["rows"][:, :3] - eager[0]["rows"][:, :3]).max() > 0.0
    for v in out.values():
        v.zero_()
    p.copy_(to4(frames[0]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        eng.molecules_compute(p, mol, **out)
    torch.cuda.synchronize()
    assert not out["sums"].cpu().numpy().any() and not out["hist"].cpu().numpy().any(), "a capture runs nothing"
    for k, f in enumerate(frames):
        p.copy_(to4(f))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for name in ("rows", "unfolded", "sums", "sample"):
            assert same_bits(out[name].cpu().numpy(), eager[k][name]), (k, name)
        assert np.array_equal(out["hist"].cpu().numpy(), eager[k]["hist"])
    mol.close()
    eng.close()


# -- 6. the raw C-ABI: refusals write nothing, a slab rank's handle -----------------------------------------------------------------------

def test_refusals_write_nothing_and_a_slab_rank_works():
    import torch
    from pse_amd import _lib
    from pse_amd._lib import pse_params
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
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

    box, n, bonds, pos, types, ntypes = DYADIC["four 64"]
    ref = dyadic_reference("four 64")
    pairs, ty = np.ascontiguousarray(bonds, dtype=np.uint32), np.ascontiguousarray(types, dtype=np.uint32)
    rc, h = create(16.0, n)
    assert rc == 0, msg()
    assert lib.pse_set_box(h, *box) == 0, msg()
    m = ctypes.c_void_p(777)
    assert lib.pse_molecules_create(h, n + 1, len(pairs), vp(pairs), vp(ty), ntypes, 32, 23.9, 63.7, ctypes.byref(m)) == INVALID
    assert f"n = {n + 1}" in msg() and not m.value
    assert lib.pse_molecules_create(h, n, len(pairs), vp(pairs), vp(ty), ntypes, 32, 23.9, 63.7, ctypes.byref(m)) == 0 and m.value, msg()
    p = to4(pos)
    rows = torch.full((4, 14), -7.0, dtype=torch.float64, device="cuda")
    sums = torch.full((ntypes, 14), -7.0, dtype=torch.float64, device="cuda")
    hist = torch.full((2, ntypes, 33), 5, dtype=torch.int64, device="cuda")
    unf = torch.full((n, 4), -7.0, dtype=torch.float64, device="cuda")
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)   # noqa: E731
    for word, args in (("null molecule object", (None, P(p), P(rows), None, None, None, None)),
                       ("null pos", (m, None, P(rows), None, None, None, None)),
                       ("all null", (m, P(p), None, None, None, None, None)),
                       ("rows =", (m, P(p), off(rows, 4), None, None, None, None)),
                       ("16-byte", (m, P(p), P(rows), off(unf, 8), None, None, None)),
                       ("sums =", (m, P(p), P(rows), None, off(sums, 4), None, None)),
                       ("sample =", (m, P(p), P(rows), None, None, off(sums, 4), None)),
                       ("hist =", (m, P(p), P(rows), None, None, None, off(hist, 4)))):
        assert lib.pse_molecules_compute(*args) == INVALID and word in msg() and "pse_molecules_compute" in msg(), (word, msg())
    torch.cuda.synchronize()
    assert np.all(rows.cpu().numpy() == -7.0) and np.all(sums.cpu().numpy() == -7.0) and np.all(hist.cpu().numpy() == 5)
    assert np.all(unf.cpu().numpy() == -7.0)
    assert lib.pse_molecules_compute(m, P(p), P(rows), P(unf), P(sums), None, P(hist)) == 0, msg()
    torch.cuda.synchronize()
    assert same_bits(rows.cpu().numpy(), ref["rows"]) and same_bits(sums.cpu().numpy(), ref["sums"] - 7.0)
    assert np.array_equal(hist.cpu().numpy(), ref["hist"] + 5)
    # a slab rank's handle: positions are replicated there, the result is complete (its box is 32^3, where the same chains are exact too)
    rc, hs = create(32.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    ms = ctypes.c_void_p()
    assert lib.pse_molecules_create(hs, n, len(pairs), vp(pairs), vp(ty), ntypes, 0, 0.0, 0.0, ctypes.byref(ms)) == 0, msg()
    box_s = (32.0, 32.0, 32.0, 0.0)
    pos_s = cc.wrap(ref["unfolded"][:, :3], box_s)                              # the same chains, unfolded and wrapped into the larger box
    want = cr.reference(pos_s, box_s, bonds, types, ntypes)
    assert want["inexact"] == 0 and want["inexact4"] == 0 and want["image_margin"] > 1e-6
    rows.zero_(); sums.zero_()
    assert lib.pse_molecules_compute(ms, P(to4(pos_s)), P(rows), None, P(sums), None, P(hist)) == INVALID and "nbins = 0" in msg()
    assert lib.pse_molecules_compute(ms, P(to4(pos_s)), P(rows), None, P(sums), None, None) == 0, msg()
    torch.cuda.synchronize()
    assert same_bits(rows.cpu().numpy(), want["rows"]) and same_bits(sums.cpu().numpy(), want["sums"])
    assert lib.pse_molecules_destroy(ms) == 0 and lib.pse_molecules_destroy(None) == 0
    for hh in (h, hs):                                                                    # m is still alive: it goes with its handle
        assert lib.pse_destroy(hh) == 0
