"""pse_molecule_pairs_compute and analyze.ChainStatistics on the device against the exact reference of tests/chain_stats_ref.py: the
curves bit for bit and 1/Rh within (P + 4) 2^-53 on the dyadic cases of conformation_cases.py, within the bound derived from the order
of operations on general positions at the wave and tile edges; ns = 1, ns below the largest molecule and ns = 1024; every output
alone; two calls; beads moved by lattice vectors; a captured graph; a slab rank's handle; the analyzer through System.run under a
shear that flips; refusals that write nothing."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
import conformation_cases as cc
import chain_stats_ref as cs

pytestmark = pytest.mark.gpu

NMAX = 4400
INVALID = -1
NAMES = ("inv_rh", "curves", "sums", "sample")


@functools.lru_cache(maxsize=None)
def engine(lengths):
    import pse_amd
    return pse_amd.Engine(NMAX, lengths + (0.0,), xi=0.5, error=1e-3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    return bool(np.array_equal(bits(got), bits(want)))


def compute(box, n, bonds, pos, mol_types=None, ntypes=1, ns=1, calls=1, only=None):
    """One pair object on the engine of the box's lengths, `calls` computes from zeroed outputs.  Returns the outputs as NumPy arrays;
    only=name: that output alone, the others None."""
    import torch
    eng = engine(tuple(box[:3]))
    eng.set_box(*box)
    mp = eng.molecule_pairs(bonds, mol_types, ntypes, ns, n=n)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    out = dict(inv_rh=z(mp.nmol), curves=z(ntypes, ns, 2), sums=z(ntypes, 2), sample=z(ntypes, 2))
    if only is not None:
        out = {k: (v if k == only else None) for k, v in out.items()}
    p = to4(pos)
    for _ in range(calls):
        eng.molecule_pairs_compute(p, mp, **out)
    torch.cuda.synchronize()
    res = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    res["nmol"], res["nmol_type"], res["terms"] = mp.nmol, mp.nmol_type, mp.terms
    mp.close()
    eng.set_box(*(tuple(box[:3]) + (0.0,)))
    return res


# -- 1. dyadic inputs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cc.DYADIC))
def test_dyadic_inputs(name):
    """curves bit for bit against the exact reference, which rounded nothing; inv_rh within (P + 4) 2^-53 relative, sums and sample
    within the bound that follows; terms and the counts equal; two calls double curves and sums and leave sample and inv_rh; beads
    moved by their own lattice vectors give equal bits."""
    box, n, bonds, pos, types, ntypes, ns, ref = cs.dyadic(name)
    assert ref["inexact"] == 0
    got = compute(box, n, bonds, pos, types, ntypes, ns)
    assert same_bits(got["curves"], ref["curves"])
    tol, stol = cs.dyadic_bounds(ref, types, ntypes)
    err = np.abs(got["inv_rh"] - ref["inv_rh"])
    print("inv_rh: largest error / bound", (err / tol).max())
    assert np.all(err <= tol)
    serr = np.abs(got["sums"] - ref["sums"])
    print("sums: largest error / bound", (serr / np.maximum(stol, 1e-300)).max())
    assert np.all(serr <= stol) and same_bits(got["sample"], got["sums"])
    assert np.array_equal(got["terms"], ref["terms"]) and got["nmol"] == len(ref["mols"])
    t = np.zeros(got["nmol"], dtype=int) if types is None else types
    assert np.array_equal(got["nmol_type"], np.bincount(t, minlength=ntypes))
    twice = compute(box, n, bonds, pos, types, ntypes, ns, calls=2)
    assert same_bits(twice["curves"], 2.0 * got["curves"]) and same_bits(twice["sums"], 2.0 * got["sums"])
    assert same_bits(twice["sample"], got["sample"]) and same_bits(twice["inv_rh"], got["inv_rh"])
    moved = cc.reimage(pos, box, np.random.default_rng(3))
    again = compute(box, n, bonds, moved, types, ntypes, ns)
    assert all(same_bits(again[k], got[k]) for k in NAMES)


# -- 2. general positions at the wave and tile edges --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(cc.EDGES)))
def test_sizes_at_the_wave_and_tile_edges_within_the_bound(k):
    """Sizes 2, 3, 63, 64, 65, 255, 257 and 1023, a star, rings and a comb, a tile of exactly 1024, 1, 2 and 8 types with empty types
    and types without a linear molecule: every output within chain_stats_ref.bounds of the once-rounded exact value; a type
    without (linear) molecules holds exactly +0.0.  tests/test_chain_stats_cpu.py checks the same cases' smallest distances and that a
    float64 restatement of the kernel's order keeps the bound."""
    box, n, bonds, pos, types, ntypes, ns, ref = cs.edge(k)
    got = compute(box, n, bonds, pos, types, ntypes, ns)
    tol, ctol, stol, x = cs.bounds(ref, box, types, ntypes, ns)
    assert x <= 0.5 and ref["nzero"] == 0
    err = np.abs(got["inv_rh"] - ref["inv_rh"])
    print("inv_rh: largest error / bound", (err / tol).max())
    assert np.all(err <= tol)
    cerr = np.abs(got["curves"] - ref["curves"])
    print("curves: largest error / bound", (cerr / np.maximum(ctol, 1e-300)).max())
    assert np.all(cerr <= ctol)
    serr = np.abs(got["sums"] - ref["sums"])
    print("sums: largest error / bound", (serr / np.maximum(stol, 1e-300)).max())
    assert np.all(serr <= stol) and same_bits(got["sample"], got["sums"])
    assert np.array_equal(got["terms"], ref["terms"])
    t = np.zeros(got["nmol"], dtype=int) if types is None else types
    empty = np.bincount(t, minlength=ntypes) == 0
    assert same_bits(got["sums"][empty], np.zeros((int(empty.sum()), 2)))
    nolinear = np.bincount(t[ref["linear"]], minlength=ntypes) == 0
    assert same_bits(got["curves"][nolinear], np.zeros((int(nolinear.sum()), ns, 2)))
    assert same_bits(got["curves"][:, 0, 0], np.zeros(ntypes))                 # D(0) = +0.0
    if ns > 1:
        assert same_bits(got["curves"][:, 0, 1], got["curves"][:, 1, 0])      # C(0) has the bits of D(1)


# -- 3. the number of separations; every output alone -----------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [1, 100])
def test_fewer_separations_give_the_leading_rows_of_the_full_curves(ns):
    """ns = 1 and ns smaller than the largest molecule (ns = 1024 is the case of every test above): the curves are the first ns rows
    of the full ones bit for bit, the other outputs do not change, terms likewise."""
    box, n, bonds, pos, types, ntypes, full_ns, ref = cs.edge(1)
    assert full_ns == 1024 and ns < ref["size"].max()
    full = compute(box, n, bonds, pos, types, ntypes, full_ns)
    got = compute(box, n, bonds, pos, types, ntypes, ns)
    assert same_bits(got["curves"], full["curves"][:, :ns]) and np.array_equal(got["terms"], ref["terms"][:, :ns])
    assert all(same_bits(got[k], full[k]) for k in ("inv_rh", "sums", "sample"))
    box, n, bonds, pos, types, ntypes, _, dref = cs.dyadic("2 64 256 1024")
    want = cs.reference(pos, box, bonds, types, ntypes, ns) if ns == 1 else None
    got = compute(box, n, bonds, pos, types, ntypes, ns)
    assert same_bits(got["curves"], dref["curves"][:, :ns])
    if want is not None:
        assert same_bits(got["curves"], want["curves"]) and np.array_equal(got["terms"], want["terms"])


@pytest.mark.parametrize("only", NAMES)
def test_every_output_alone_gives_the_bits_of_the_full_call(only):
    box, n, bonds, pos, types, ntypes, ns, _ = cs.edge(2)
    full = compute(box, n, bonds, pos, types, ntypes, ns)
    alone = compute(box, n, bonds, pos, types, ntypes, ns, only=only)
    assert all(alone[k] is None for k in NAMES if k != only)
    assert same_bits(alone[only], full[only])


# -- 4. analyze.ChainStatistics on a System -----------------------------------------------------------------------------------------------

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


def test_analyzer_through_system_run_under_a_shear_that_flips(restored_context):
    """analyze.ChainStatistics made from a forces.Bonds, molecule_types="size" with names, a period, a ring shorter than the run,
    reset(): every row of series() and the accumulated curves and sums equal the exact reference at the positions and the box of
    the sampled steps within the bound -- through the Lees-Edwards flip at step 16 --, the readers what follows from them."""
    from pse_amd import analyze, forces, integrate, shear_function, variant
    from pse_amd.system import System
    rng = np.random.default_rng(21)
    shapes = [("chain", 8)] * 3 + [("chain", 5)] * 2 + [("star", 6)]
    n, bonds, sizes, kinds = cc.build(shapes, gaps=(0, 1))
    n += 1
    box0 = (16.0, 16.0, 16.0, 0.0)
    dt, rate = 2.0 ** -6, 2.0                                                  # the tilt grows by 1/32 per step: the flip at step 16
    s = System(cc.wrap(cc.place(n, bonds, box0, rng, 2.5), box0), box0, dt=dt)
    fn = shear_function.steady(dt=dt, shear_rate=rate)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3, function_form=fn)
    s.box_tilt_variant = variant.shear_variant(fn, 100000, max_strain=0.5)
    fb = forces.Bonds(pse, bonds, kind="harmonic", k=20.0, r0=2.0)
    st = analyze.ChainStatistics(pse, fb, molecule_types="size", type_names=["five", "six", "eight"], period=3, capacity=4)
    assert st.ntypes == 3 and st.smax == 8 and st.nmol == 6 and list(st.nmol_type) == [2, 1, 3] and np.array_equal(st.sizes(), sizes)
    snaps = Snapshots(s)
    s.run(24)
    assert s.tilt_flips >= 1
    sampled = [f for f in snaps.frames if f[0] % 3 == 0]
    assert st.samples == len(sampled) == 8
    ser = st.series()
    assert ser.shape == (4, 1 + 3 * 2) and [int(t) for t in ser[:, 0]] == [f[0] for f in sampled[-4:]]
    types = np.searchsorted(st.size_values, sizes)
    total_c, total_s, tol_c, tol_s = np.zeros((3, 8, 2)), np.zeros((3, 2)), np.zeros((3, 8, 2)), np.zeros((3, 2))
    for r, (step, pos, box) in enumerate(sampled):
        ref = cs.reference(pos, box, bonds, types, 3, 8)
        _, ctol, stol, x = cs.bounds(ref, box, types, 3, 8)
        assert x <= 0.5
        total_c += ref["curves"]; total_s += ref["sums"]; tol_c += ctol; tol_s += stol
        if r >= 4:
            assert np.all(np.abs(ser[r - 4, 1:].reshape(3, 2) - ref["sums"]) <= stol), step
    assert np.array_equal(st.terms, ref["terms"])
    assert np.all(np.abs(st.curves() - total_c) <= tol_c + 8 * cc.EPS * np.abs(total_c))
    assert np.all(np.abs(st.sums() - total_s) <= tol_s + 8 * cc.EPS * np.abs(total_s))
    sep, r2 = st.internal_distances("eight")
    assert sep.tolist() == list(range(8)) and r2[0] == 0.0
    assert np.allclose(r2, total_c[2, :, 0] / (8 * ref["terms"][2, :, 0]), rtol=1e-12)
    sep, r2 = st.internal_distances("five")
    assert np.isnan(r2[5:]).all() and not np.isnan(r2[:5]).any()
    assert np.isnan(st.internal_distances("six")[1]).all() and np.isnan(st.bond_length("six")) and np.isnan(st.persistence_length("six"))
    c = st.bond_correlation()[1]
    assert c[0] == 1.0 and np.allclose(c[:7], total_c[:, :7, 1].sum(0) / ref["terms"][:, :7, 1].sum(0) / (total_c[:, 0, 1].sum() / ref["terms"][:, 0, 1].sum()))
    b = st.bond_length("eight")
    assert np.isclose(b, np.sqrt(total_c[2, 0, 1] / (8 * 21)), rtol=1e-12) and np.isclose(b * b, st.internal_distances("eight")[1][1], rtol=1e-12)
    assert np.isclose(st.persistence_length("eight", 3), analyze.persistence_length_of(*st.bond_correlation("eight"), b, 3), equal_nan=True)
    assert np.isclose(st.inv_rh("six"), total_s[1, 0] / 8, rtol=1e-12) and np.isclose(st.rh(), 8 * 6 / total_s[:, 0].sum(), rtol=1e-12)
    pos, box = s.pos.cpu().numpy()[:, :3].copy(), tuple(s.box)
    ref = cs.reference(pos, box, bonds, types, 3, 8)
    assert np.all(np.abs(st.per_molecule() - ref["inv_rh"]) <= cs.bounds(ref, box, types, 3, 8)[0])
    assert st.samples == 8                                                     # the readers took no sample
    st.reset()
    assert st.samples == 0 and not st.sums().any() and not st.curves().any() and st.series().shape == (0, 7)
    with pytest.raises(ValueError, match="no samples"):
        st.rh()
    s.run(3)
    assert st.samples == 1 and int(st.series()[0, 0]) == 24


# -- 5. queue-only: a captured graph ------------------------------------------------------------------------------------------------------

def test_a_captured_graph_replayed_on_moved_positions_gives_the_eager_bits():
    import torch
    import pse_amd
    box, n, bonds, pos, types, ntypes, ns, _ = cs.edge(2)
    ns = 300
    frames = [pos, cc.wrap(pos + 0.125, box)]
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    mp = eng.molecule_pairs(bonds, types, ntypes, ns, n=n)
    p = to4(pos)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    out = dict(inv_rh=z(mp.nmol), curves=z(ntypes, ns, 2), sums=z(ntypes, 2), sample=z(ntypes, 2))
    eager = []
    for f in frames:
        p.copy_(to4(f))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            eng.molecule_pairs_compute(p, mp, **out)
        st.synchronize()
        eager.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    assert np.abs(eager[1]["inv_rh"] - eager[0]["inv_rh"]).max() > 0.0
    for v in out.values():
        v.zero_()
    p.copy_(to4(frames[0]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        eng.molecule_pairs_compute(p, mp, **out)
    torch.cuda.synchronize()
    assert not out["sums"].cpu().numpy().any() and not out["curves"].cpu().numpy().any(), "a capture runs nothing"
    for k, f in enumerate(frames):
        p.copy_(to4(f))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for name in NAMES:
            assert same_bits(out[name].cpu().numpy(), eager[k][name]), (k, name)
    mp.close()
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

    box, n, bonds, pos, types, ntypes, _, _ = cs.dyadic("four 64")
    ns = 64
    ref = cs.reference(pos, box, bonds, types, ntypes, ns)
    pairs, ty = np.ascontiguousarray(bonds, dtype=np.uint32), np.ascontiguousarray(types, dtype=np.uint32)
    rc, h = create(16.0, n)
    assert rc == 0, msg()
    assert lib.pse_set_box(h, *box) == 0, msg()
    m = ctypes.c_void_p(777)
    assert lib.pse_molecule_pairs_create(h, n, len(pairs), vp(pairs), vp(ty), ntypes, 1025, ctypes.byref(m)) == INVALID
    assert "ns = 1025" in msg() and not m.value
    assert lib.pse_molecule_pairs_create(h, n + 1, len(pairs), vp(pairs), vp(ty), ntypes, 0, ctypes.byref(m)) == INVALID
    assert f"n = {n + 1}" in msg() and not m.value
    assert lib.pse_molecule_pairs_create(h, n, len(pairs), vp(pairs), vp(ty), ntypes, ns, ctypes.byref(m)) == 0 and m.value, msg()
    p = to4(pos)
    inv = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    curves = torch.full((ntypes, ns, 2), -7.0, dtype=torch.float64, device="cuda")
    sums = torch.full((ntypes, 2), -7.0, dtype=torch.float64, device="cuda")
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)   # noqa: E731
    for word, args in (("null molecule-pair object", (None, P(p), P(inv), None, None, None)),
                       ("null pos", (m, None, P(inv), None, None, None)),
                       ("all null", (m, P(p), None, None, None, None)),
                       ("inv_rh =", (m, P(p), off(inv, 4), off(curves, 4), None, None)),
                       ("curves =", (m, P(p), P(inv), off(curves, 4), off(sums, 4), None)),
                       ("sums =", (m, P(p), P(inv), P(curves), off(sums, 4), off(sums, 4))),
                       ("sample =", (m, P(p), P(inv), P(curves), None, off(sums, 4)))):
        assert lib.pse_molecule_pairs_compute(*args) == INVALID and word in msg() and "pse_molecule_pairs_compute" in msg(), (word, msg())
    torch.cuda.synchronize()
    assert np.all(inv.cpu().numpy() == -7.0) and np.all(curves.cpu().numpy() == -7.0) and np.all(sums.cpu().numpy() == -7.0)
    assert lib.pse_molecule_pairs_compute(m, P(p), P(inv), P(curves), None, P(sums)) == 0, msg()
    torch.cuda.synchronize()
    tol, stol = cs.dyadic_bounds(ref, types, ntypes)
    assert same_bits(curves.cpu().numpy(), ref["curves"] - 7.0) and np.all(np.abs(inv.cpu().numpy() - ref["inv_rh"]) <= tol)
    assert np.all(np.abs(sums.cpu().numpy() - ref["sums"]) <= stol)
    first = {"inv": inv.cpu().numpy().copy(), "sums": sums.cpu().numpy().copy()}
    # a slab rank's handle: positions are replicated there, the result is complete.  The same chains, unfolded and wrapped into a box
    # of 32^3: the offsets are the same numbers, so every output has the bits of the first handle's.
    import conformation_ref as cr
    rc, hs = create(32.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    ms = ctypes.c_void_p()
    assert lib.pse_molecule_pairs_create(hs, n, len(pairs), vp(pairs), vp(ty), ntypes, ns, ctypes.byref(ms)) == 0, msg()
    box_s = (32.0, 32.0, 32.0, 0.0)
    pos_s = cc.wrap(cr.reference(pos, box, bonds, types, ntypes)["unfolded"][:, :3], box_s)
    inv.zero_(); curves.zero_(); sums.zero_()
    assert lib.pse_molecule_pairs_compute(ms, P(to4(pos_s)), P(inv), P(curves), P(sums), None) == 0, msg()
    torch.cuda.synchronize()
    assert same_bits(curves.cpu().numpy(), ref["curves"]) and same_bits(inv.cpu().numpy(), first["inv"]) and same_bits(sums.cpu().numpy(), first["sums"])
    nmol, nty = ctypes.c_uint(0), np.zeros(ntypes, np.uint32)
    terms = np.zeros((ntypes, ns, 2), np.uint64)
    assert lib.pse_molecule_pairs_counts(ms, ctypes.byref(nmol), vp(nty), vp(terms)) == 0
    assert nmol.value == 4 and nty.tolist() == [2, 2] and np.array_equal(terms.astype(np.int64), ref["terms"])
    assert lib.pse_molecule_pairs_destroy(ms) == 0 and lib.pse_molecule_pairs_destroy(None) == 0
    for hh in (h, hs):                                                                    # m is still alive: it goes with its handle
        assert lib.pse_destroy(hh) == 0
