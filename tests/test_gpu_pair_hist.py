"""GPU tests of the pair-distance histogram (pse_pair_hist_create, pse_pair_hist_accumulate) and of analyze.RDF on top of it: the counts
against the O(N^2) reference of tests/pair_hist_ref.py (validated on the CPU by tests/test_pair_hist_cpu.py) over the wave / workgroup
edges, the numbers of types and bins up to the cap of 8192 counters, rmin = 0 and > 0, rmax = rcut, accumulation, particle order and
type labels, a group, exclusions on chains, the many-cell grids of tests/cell_grid_cases.py, the zero-table trick of
forces.TypedTablePair, the error returns of the raw C-ABI, the lifetime of the device object, and RDF through System.run.

There is no tolerance: the counts are integers and must EQUAL the reference.  What could make two correct implementations differ is a
pair whose r rounds to the other side of a bin edge, of rmin or of rmax; every input is therefore first held to the clearance
condition of pair_hist_ref (1e-9; the device's r differs from NumPy's by ~1e-16 relative)."""
import ctypes
import functools
import gc

import numpy as np
import pytest

from conftest import to4
import cell_grid_cases as cg
import pair_hist_ref as hr
from pair_table_ref import random_points
from test_gpu_pair_typed import chains
from test_gpu_provider_lifetime import _Unraisable

pytestmark = pytest.mark.gpu

NMAX = 513
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
BOXES = pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
INVALID = -1
CAPS = {1: 8192, 2: 2730, 3: 1365, 8: 227}       # the most bins for that many types: npt x nbins <= 8192
R_CONTACT = 2.6


def port():
    from oracle import pse_port
    pse_port.lib()
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(NMAX, box, xi=0.5, error=1e-3)


def rcut(box):
    return engine(box).info()["rcut"]


@functools.lru_cache(maxsize=None)
def points(box, n=NMAX):
    """The first n of the 513 seeded points of the box: every smaller input is a subset of the largest, and so are its pairs."""
    pos = random_points(NMAX, box, seed=11)[:n].copy()
    pos.setflags(write=False)
    return pos


def types_of(n, ntypes, seed=21):
    return np.random.default_rng(seed).integers(0, ntypes, n)


def reference(pos, box, types, ntypes, nbins, rmin, rmax, **kw):
    """The reference counts of an input that is clear of every edge."""
    counts, clear = hr.histogram(pos, box, types, ntypes, nbins, rmin, rmax, port(), **kw)
    hr.assert_clear(clear)
    return counts


def zeros(ntypes, nbins):
    import torch
    return torch.zeros((ntypes * (ntypes + 1) // 2, nbins), dtype=torch.int64, device="cuda")


def device(eng, pos, types, ntypes, nbins, rmin, rmax, counts=None, group=None, exclusions=None, n=None):
    """One accumulate call on a new object into `counts` (default: zeros), read back."""
    import torch
    hist = eng.pair_histogram(types, ntypes, nbins, rmin, rmax, n)
    counts = zeros(ntypes, nbins) if counts is None else counts
    g = None if group is None else torch.tensor(np.asarray(group), dtype=torch.int32, device="cuda")
    assert eng.pair_hist_accumulate(to4(pos), hist, counts, group=g, exclusions=exclusions) is counts
    out = counts.cpu().numpy()
    hist.close()
    return out


# -- rows, types, bins -----------------------------------------------------------------------------------------------------------------

@BOXES
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300, 513])
def test_row_counts(n, box):
    """One lane, one pair, a wave and a workgroup less one, full, plus one; two workgroups and a third with one lane."""
    eng = engine(box)
    pos, types = points(box, n), types_of(n, 2)
    rmax = rcut(box)
    want = reference(pos, box, types, 2, 64, 0.0, rmax)
    got = device(eng, pos, types, 2, 64, 0.0, rmax)
    print(f"n = {n}: {want.sum()} pairs below {rmax:.4f}")
    assert want.sum() > (20 if n >= 63 else -1) and got.dtype == np.int64
    assert np.array_equal(got, want)


@BOXES
@pytest.mark.parametrize("ntypes", [1, 2, 3, 8])
@pytest.mark.parametrize("nbins", [1, 2, 7, 64, "cap"])
def test_types_and_bins(nbins, ntypes, box):
    """Every number of types with few bins (many lanes on one counter, one copy of the counters per wave), 64, and the most that fit
    (8192 counters, one copy); the ranges from zero, from rmin > 0, and up to rcut."""
    eng = engine(box)
    nbins = CAPS[ntypes] if nbins == "cap" else nbins
    pos, types = points(box, 300), types_of(300, ntypes)
    assert len(set(types.tolist())) == ntypes
    for rmin, rmax in ((0.0, 3.0), (0.7, 3.0), (1.0, 5.0), (0.0, rcut(box))):
        want = reference(pos, box, types, ntypes, nbins, rmin, rmax)
        got = device(eng, pos, types, ntypes, nbins, rmin, rmax)
        assert want.sum() > 1000 and (nbins > 64 or want.sum(axis=1).min() > 0)
        assert np.array_equal(got, want), (ntypes, nbins, rmin, rmax, int(np.abs(got - want).sum()))


@BOXES
def test_a_pair_type_without_pairs_and_no_types_at_all(box):
    eng = engine(box)
    pos = points(box, 300)
    rmax = rcut(box)
    types = types_of(300, 2)                                     # three types declared, the third unused: three empty rows
    want = reference(pos, box, types, 3, 64, 0.0, rmax)
    assert not want[[2, 4, 5]].any() and want[[0, 1, 3]].sum(axis=1).min() > 1000
    assert np.array_equal(device(eng, pos, types, 3, 64, 0.0, rmax), want)
    one = reference(pos, box, None, 1, 64, 0.0, rmax)
    assert np.array_equal(one[0], want.sum(axis=0))
    assert np.array_equal(device(eng, pos, None, 1, 64, 0.0, rmax), one)                                  # types_host = NULL
    assert np.array_equal(device(eng, pos, np.zeros(300, dtype=int), 1, 64, 0.0, rmax), one)              # ... is ntypes = 1
    # a type array shorter than the rows: the particles past it act as type 0
    short = types.copy()
    short[200:] = 0
    assert np.array_equal(device(eng, pos, types[:200], 2, 64, 0.0, rmax), reference(pos, box, short, 2, 64, 0.0, rmax))


# -- accumulation ----------------------------------------------------------------------------------------------------------------------

def test_counts_are_added_to():
    import torch
    box = TILTED
    eng = engine(box)
    pos, other = points(box, 300), points(box)[213:]
    types = types_of(300, 2)
    args = (2, 64, 0.7, 3.0)
    a, b = reference(pos, box, types, *args), reference(other, box, types, *args)
    assert a.sum() > 1000 and b.sum() > 1000 and not np.array_equal(a, b)
    hist = eng.pair_histogram(types, *args)
    pre = np.random.default_rng(3).integers(0, 2 ** 40, size=a.shape)                # beyond 32 bits: the counters are 64-bit words
    counts = torch.tensor(pre, dtype=torch.int64, device="cuda")
    eng.pair_hist_accumulate(to4(pos), hist, counts)
    assert np.array_equal(counts.cpu().numpy(), pre + a)                               # what was there is kept
    eng.pair_hist_accumulate(to4(pos), hist, counts)
    assert np.array_equal(counts.cpu().numpy(), pre + 2 * a)                           # the same configuration again: doubled
    eng.pair_hist_accumulate(to4(other), hist, counts)
    assert np.array_equal(counts.cpu().numpy(), pre + 2 * a + b)                       # another configuration: added
    first, second = zeros(2, 64), zeros(2, 64)
    eng.pair_hist_accumulate(to4(pos), hist, first)
    eng.mobility(to4(other), to4(np.ones((300, 3))), parts=1)                          # another entry point in between: the next call sorts again
    eng.pair_hist_accumulate(to4(pos), hist, second)
    assert np.array_equal(first.cpu().numpy(), second.cpu().numpy()) and np.array_equal(first.cpu().numpy(), a)
    with pytest.raises(ValueError, match="int64"):
        eng.pair_hist_accumulate(to4(pos), hist, torch.zeros((3, 64), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        eng.pair_hist_accumulate(to4(pos), hist, zeros(2, 32))
    hist.close()
    with pytest.raises(ValueError, match="closed"):
        eng.pair_hist_accumulate(to4(pos), hist, first)


# -- order and labels --------------------------------------------------------------------------------------------------------------------

@BOXES
def test_particle_order_and_type_labels(box):
    eng = engine(box)
    pos, types = points(box, 300), types_of(300, 3)
    args = (64, 0.7, 3.0)
    want = reference(pos, box, types, 3, *args)
    perm = np.random.default_rng(8).permutation(300)
    assert np.array_equal(device(eng, pos[perm], types[perm], 3, *args), want)         # the order of the particles does not matter
    relabel = np.array([2, 0, 1])                                                      # A -> C, B -> A, C -> B
    got = device(eng, pos, relabel[types], 3, *args)
    for a in range(3):
        for b in range(a, 3):
            assert np.array_equal(got[hr.pair_index(relabel[a], relabel[b], 3)], want[hr.pair_index(a, b, 3)]), (a, b)
    assert len({hr.pair_index(relabel[a], relabel[b], 3) for a in range(3) for b in range(a, 3)}) == 6


# -- a group -----------------------------------------------------------------------------------------------------------------------------

@BOXES
def test_group_of_every_other_particle(box):
    eng = engine(box)
    pos, types = points(box), types_of(NMAX, 2)
    members = np.arange(0, NMAX, 2)
    rmax = rcut(box)
    want = reference(pos[members], box, types[members], 2, 64, 0.0, rmax)
    assert 1000 < want.sum() < reference(pos, box, types, 2, 64, 0.0, rmax).sum() // 3
    assert np.array_equal(device(eng, pos, types, 2, 64, 0.0, rmax, group=members), want)             # types are caller indices


# -- exclusions --------------------------------------------------------------------------------------------------------------------------

@BOXES
def test_exclusions_on_chains(box):
    from pse_amd.forces import exclusion_pairs
    eng = engine(box)
    pos, types, bonds, angles = chains(box)
    n = len(pos)
    excl = exclusion_pairs(bonds, angles)
    args = (2, 64, 0.0, 3.0)
    everything = reference(pos, box, types, *args)
    want = reference(pos, box, types, *args, excl=excl)
    bonded = reference(pos, box, types, *args, excl=bonds)
    assert everything.sum() - bonded.sum() == len(bonds)                               # every bond (0.95 long) is in range: all absent
    assert bonded[1].sum() == everything[1].sum() - len(bonds)                         # ... and all of them are A-B pairs
    assert everything.sum() - want.sum() > len(bonds) + 100
    ex = eng.exclusions(excl)
    assert np.array_equal(device(eng, pos, types, *args, exclusions=ex), want)
    exb = eng.exclusions(bonds)
    assert np.array_equal(device(eng, pos, types, *args, exclusions=exb), bonded)
    assert np.array_equal(device(eng, pos, types, *args), everything)
    # an object with nothing in range leaves the counts as they are
    i, j, r = hr.pair_distances(pos, box, port())
    far = np.stack([i, j], axis=1)[r > 3.5][:400]
    exf = eng.exclusions(far)
    assert np.array_equal(device(eng, pos, types, *args, exclusions=exf), everything)
    # a group: exclusions and types are caller indices
    members = np.sort(np.random.default_rng(6).choice(n, 200, replace=False))
    wantg = reference(pos[members], box, types[members], *args, excl=excl, ids=members)
    assert wantg.sum() < reference(pos[members], box, types[members], *args).sum()
    assert np.array_equal(device(eng, pos, types, *args, exclusions=ex, group=members), wantg)
    for e in (ex, exb, exf):
        e.close()


# -- many-cell grids ---------------------------------------------------------------------------------------------------------------------

GRID_NAMES = ("blocked_padded", "blocked_tilt_neg", "one_cell_x", "three_cubed")


@pytest.mark.parametrize("name", GRID_NAMES)
def test_many_cell_grids(name):
    """rmax = rcut, 64 bins: the pairs through faces, edges, corners and block boundaries are counted, the pair 1e-9 inside the cutoff
    lands in the last bin (through the clamp if its t rounds to 64), the pair 1e-9 outside is not counted."""
    import pse_amd
    c = cg.build(name, port())
    pos, box, n, nbins = c["pos"], c["box"], c["n"], 64
    types = types_of(n, 2)
    at_rcut = [(i, j) for i, j, cname, _, _ in c["planted"] if cname == "rcut"]
    eng = pse_amd.Engine(n, box, xi=c["xi"], error=c["error"], max_strain=c["max_strain"], seed=77)
    rmax = eng.info()["rcut"]
    assert abs(rmax - c["rcut"]) <= 1e-15 * c["rcut"]
    want, clear = hr.histogram(pos, box, types, 2, nbins, 0.0, rmax, port(), exempt=at_rcut)
    hr.assert_clear(clear)                                      # the planted pairs are exempt from the rmax clearance, and only from that
    # on the host, before the device is asked: the planted pairs are where they were planted
    i, j, r = hr.pair_distances(pos, box, port())
    r_of = dict(zip(zip(i.tolist(), j.tolist()), r.tolist()))
    inside = [r_of[(min(a, b), max(a, b))] for a, b, cname, ins, _ in c["planted"] if cname == "rcut" and ins]
    outside = [r_of[(min(a, b), max(a, b))] for a, b, cname, ins, _ in c["planted"] if cname == "rcut" and not ins]
    assert len(inside) == len(outside) == (0 if name == "one_cell_x" else cg.N_SITES)
    assert all(x < rmax and hr.bin_of(np.array([x]), nbins, 0.0, rmax)[0] == nbins - 1 for x in inside) and all(x >= rmax for x in outside)
    assert all(r_of[(min(a, b), max(a, b))] < 2.1 for a, b, _ in c["crossers"]) and (len(c["crossers"]) >= 13 or name == "one_cell_x")
    assert want[:, -1].sum() >= len(inside) and want.sum() > 3000
    hist = eng.pair_histogram(types, 2, nbins, 0.0, rmax)
    dpos = to4(pos)
    for which in ("wide", "narrow"):
        eng.set_neighbor_skin(c["skin"] if which == "wide" else 0.0)
        counts = zeros(2, nbins)
        eng.pair_hist_accumulate(dpos, hist, counts)
        info = eng.info()
        assert (info["ncell_x"], info["ncell_y"], info["ncell_z"]) == c["cells_" + which][:3]
        got = counts.cpu().numpy()
        assert np.array_equal(got, want), (name, which, int(np.abs(got - want).sum()), np.argwhere(got != want)[:5].tolist())
    hist.close()
    eng.close()


# -- the raw C-ABI -----------------------------------------------------------------------------------------------------------------------

def test_misuse_is_reported_before_any_launch():
    """Raw C-ABI, as a C host would call it: a rejected call leaves the counts untouched, and the handle works afterwards."""
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

    n, nbins = 300, 16
    box = CUBIC
    pos = points(box, n)
    types = types_of(n, 2).astype(np.uint32)
    rc, h = create(box[0], n)
    assert rc == 0, msg()
    rc, h2 = create(box[0], n)
    assert rc == 0, msg()
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()

    def hist_on(hh, expect=0, word=None, ty=types, ntypes=2, nb=nbins, rmin=0.0, rmax=3.0, nn=n):
        g = ctypes.c_void_p(777)
        assert lib.pse_pair_hist_create(hh, nn, None if ty is None else vp(ty), ntypes, nb, rmin, rmax, ctypes.byref(g)) == expect, msg()
        assert expect == 0 or (word in msg() and "pse_pair_hist_create" in msg() and not g.value), (word, msg())
        return g

    g = hist_on(h)
    big = types.copy()
    big[5] = 2
    hist_on(h, INVALID, "type 2", ty=big)
    hist_on(h, INVALID, "ntypes = 9", ntypes=9)
    hist_on(h, INVALID, "nbins = 0", nb=0)
    hist_on(h, INVALID, "8193 counters", nb=2731)
    hist_on(h, INVALID, "must exceed", rmin=3.0)
    hist_on(h, INVALID, "rcut", rmax=5.3)
    hist_on(h, INVALID, "n_max", nn=n + 1)
    hist_on(hs, INVALID, "slab rank")
    hist_on(None, INVALID, "null handle")
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex2 = ctypes.c_void_p()
    assert lib.pse_exclusions_create(h2, n, 1, vp(pairs), ctypes.byref(ex2)) == 0, msg()
    dpos = to4(pos)
    counts = torch.full((3, nbins), -5, dtype=torch.int64, device="cuda")
    call = lib.pse_pair_hist_accumulate

    def refused(word, gg=g, p=P(dpos), nn=n, c=P(counts), e=None):
        assert call(gg, p, None, nn, c, e) == INVALID, word
        assert word in msg() and "pse_pair_hist_accumulate" in msg(), (word, msg())

    refused("null histogram", gg=None)
    refused("n_max", nn=0)
    refused("n_max", nn=n + 1)
    refused("null pos", p=None)
    refused("null counts", c=None)
    refused("8-byte aligned", c=ctypes.c_void_p(counts.data_ptr() + 4))
    refused("another handle", e=ex2)
    torch.cuda.synchronize()
    assert np.all(counts.cpu().numpy() == -5)                                          # nothing was launched, nothing was written
    assert call(g, P(dpos), None, n, P(counts), None) == 0, msg()
    want = reference(pos, box, types, 2, nbins, 0.0, 3.0)
    assert want.sum() > 1000 and np.array_equal(counts.cpu().numpy(), want - 5)
    assert lib.pse_pair_hist_destroy(g) == 0
    assert lib.pse_pair_hist_destroy(None) == 0
    g = hist_on(h)                                                                     # still alive below: it goes with its handle
    for hh in (h, h2, hs):
        assert lib.pse_destroy(hh) == 0


# -- analyze.RDF -------------------------------------------------------------------------------------------------------------------------

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


def test_rdf_through_system_run(restored_context):
    """period and samples, reset(), g() and coordination() against the reference on the positions of every sampled step; the
    particles move under a harmonic repulsion, so the samples differ."""
    from pse_amd import analyze, forces
    box = CUBIC
    pos = points(box)
    n = len(pos)
    s, pse = system(pos, box)
    forces.HarmonicRepulsion(pse, k=40.0)
    names = ["A", "B"]
    types = types_of(n, 2)
    nbins, rmin, rmax = 50, 0.0, 5.0                                                   # bins of 0.1: R_CONTACT = 2.6 is the edge of bin 26
    rdf = analyze.RDF(pse, nbins, rmax, rmin, types=[names[t] for t in types], type_names=names, period=2)
    assert s.analyzers == [rdf] and rdf.samples == 0 and not rdf.counts.any()
    with pytest.raises(ValueError, match="no samples"):
        rdf.g()
    want = np.zeros((3, nbins), dtype=np.int64)
    snaps = []
    for t in range(5):                                                                 # samples at steps 0, 2 and 4
        if t % 2 == 0:
            snaps.append(s.pos.cpu().numpy()[:, :3].copy())
            want += reference(snaps[-1], box, types, 2, nbins, rmin, rmax)
        s.run(1)
    assert rdf.samples == 3 and np.abs(snaps[0] - snaps[2]).max() > 1e-6
    got = rdf.counts
    assert got.shape == (3, nbins) and got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(rdf.counts_of("B", "A"), want[1]) and np.array_equal(rdf.counts_of(1, 1), want[2])
    assert np.array_equal(rdf.edges, analyze.bin_edges(nbins, rmin, rmax)) and np.allclose(rdf.r, rmin + (np.arange(nbins) + 0.5) * 0.1, atol=1e-14)
    # g: equal to the reference's g of its own counts (the scatter of either about 1 is that of the counts: 1 / sqrt(count))
    type_counts = np.bincount(types, minlength=2)
    gref = hr.g_of_counts(want, 3, type_counts, nbins, rmin, rmax, box[0] * box[1] * box[2])
    g = rdf.g()
    assert g.shape == (3, nbins) and np.abs(g - gref).max() <= 1e-12 * gref.max()
    assert np.array_equal(rdf.g("A", "B"), g[1]) and np.array_equal(rdf.g(1, 0), g[1])
    # coordination: the reference, pair by pair, averaged over the samples
    for a, b in (("A", "A"), ("A", "B"), ("B", "A"), ("B", "B")):
        ref = np.mean([hr.coordination(p, box, types, names.index(a), names.index(b), R_CONTACT, port()) for p in snaps])
        assert abs(rdf.coordination(a, b, R_CONTACT) - ref) <= 1e-12 * max(1.0, ref) and ref > 0.1, (a, b)
    with pytest.raises(ValueError, match="not a bin edge"):
        rdf.coordination("A", "A", 2.65)
    with pytest.raises(ValueError, match="unknown type name"):
        rdf.counts_of("A", "C")
    rdf.reset()
    assert rdf.samples == 0 and not rdf.counts.any()
    s.run(1)                                                                           # step 5: not a sample
    assert rdf.samples == 0 and not rdf.counts.any()
    snap = s.pos.cpu().numpy()[:, :3].copy()
    s.run(1)                                                                           # step 6
    assert rdf.samples == 1 and np.array_equal(rdf.counts, reference(snap, box, types, 2, nbins, rmin, rmax))
    with pytest.raises(ValueError, match="entries"):
        analyze.RDF(pse, nbins, rmax, types=types[:-1])
    with pytest.raises(RuntimeError, match="rcut"):
        analyze.RDF(pse, nbins, 5.3)
    assert s.analyzers == [rdf]


def test_contacts_equal_the_zero_table_trick(restored_context):
    """The A-A and B-B contacts below R_CONTACT that examples/block_copolymers.py counts with two zero-table TypedTablePair providers
    are the sums of the RDF's bins below that edge, exactly; on a group, with the bonded pairs excluded from both."""
    from pse_amd import analyze, forces
    box = TILTED[:3] + (0.0,)
    pos, types, bonds, _ = chains(box)
    members = np.arange(0, len(pos) - 50)
    s, pse = system(pos, box, members)
    i, j, r = hr.pair_distances(pos[members], box, port())
    hr.assert_clear(hr.clearance(i, j, r, 50, 0.0, 5.0))
    excl = forces.Exclusions(pse, bonds)
    zero = np.zeros((2, 2))
    aa = forces.TypedTablePair(pse, types, {(0, 0): (zero, 0.0, R_CONTACT)}, virial=True, exclusions=excl)
    bb = forces.TypedTablePair(pse, types, {(1, 1): (zero, 0.0, R_CONTACT)}, virial=True, exclusions=excl)
    rdf = analyze.RDF(pse, 50, 5.0, types=types, exclusions=excl)
    s.run(1)
    k = analyze.edge_index(rdf.edges, R_CONTACT)
    assert k == 26 and aa.npairs > 100 and bb.npairs > 100
    assert rdf.counts_of(0, 0)[:k].sum() == aa.npairs and rdf.counts_of(1, 1)[:k].sum() == bb.npairs
    na = np.bincount(types[members], minlength=2)
    assert rdf.coordination(0, 0, R_CONTACT) == 2.0 * aa.npairs / na[0] and rdf.coordination(1, 1, R_CONTACT) == 2.0 * bb.npairs / na[1]
    want = reference(pos[members], box, types[members], 2, 50, 0.0, 5.0, excl=bonds, ids=members)
    assert np.array_equal(rdf.counts, want)


def test_rdf_dies_with_the_engine_that_set_params_replaces(restored_context):
    """The device object does not outlive its handle: after setParams() the analyzer says so, nothing is freed twice, and a new one
    on the new handle counts what the old one counted (tests/test_gpu_provider_lifetime.py)."""
    from pse_amd import analyze
    box = CUBIC
    pos = points(box, 300)
    s, pse = system(pos, box)
    types = types_of(300, 2)
    old = analyze.RDF(pse, 32, 3.0, types=types)
    s.run(1)
    kept = old.counts
    assert kept.sum() > 1000 and pse.engine.serial == 1
    pse.cpp_method.setParams()                                     # a new handle; pse_destroy freed the device object
    assert pse.engine.serial == 2
    with pytest.raises(ValueError, match="setParams"):
        old.analyze(0)
    assert np.array_equal(old.counts, kept) and old.samples == 1   # the counts are a tensor of the analyzer's own: still readable
    del s.analyzers[:]
    with _Unraisable() as quiet:
        del old
        gc.collect()
    assert quiet.seen == []
    new = analyze.RDF(pse, 32, 3.0, types=types)
    new.analyze(0)
    assert np.array_equal(new.counts, kept)
    s.analyzers.remove(new)
    with _Unraisable() as quiet:                                   # a collected analyzer frees its object, the handle lives on
        del new
        gc.collect()
    assert quiet.seen == [] and s.analyzers == []
