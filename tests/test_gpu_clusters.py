"""GPU tests of the cluster analysis (pse_clusters_create, pse_clusters_label, pse_clusters_status) and of analyze.Clusters on top of
it: labels, sizes, stats and the size counts against the O(N^2) reference of tests/cluster_ref.py (validated on the CPU by
tests/test_clusters_cpu.py) over the wave / workgroup edges and the regimes from many small clusters to one; a lattice on which every
particle hooks into the same tree; a chain in three caller orders; the numbers of types and the pair-type switches; every output alone
and together; a group; particle order and type labels; exclusions on chains; the many-cell grids of tests/cell_grid_cases.py; the error
returns of the raw C-ABI; the lifetime of the device object; a captured graph; and Clusters through System.run.

There is no tolerance: every output is an integer and must EQUAL the reference.  What could make two correct implementations differ
is a pair whose r rounds to the other side of its link distance; every input is therefore first held to the clearance condition of
cluster_ref (1e-9; the device's r^2 differs from NumPy's r by ~1e-16 relative).  status() is 0 after every case."""
import ctypes
import functools
import gc

import numpy as np
import pytest

from conftest import to4
import cell_grid_cases as cg
import cluster_ref as cr
from pair_table_ref import random_points
from test_gpu_pair_typed import chains
from test_gpu_provider_lifetime import _Unraisable

pytestmark = pytest.mark.gpu

NMAX = 513
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
BOXES = pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
INVALID = -1
SENTINEL = -7


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
    """The first n of the 513 seeded points of the box."""
    pos = random_points(NMAX, box, seed=11)[:n].copy()
    pos.setflags(write=False)
    return pos


def types_of(n, ntypes, seed=21):
    return np.random.default_rng(seed).integers(0, ntypes, n)


def reference(pos, box, types, ntypes, rlink, **kw):
    """(label, size, stats, hist) of an input that is clear of every link distance."""
    label, size, stats, hist, clear = cr.clusters(pos, box, types, ntypes, rlink, port(), **kw)
    cr.assert_clear(clear)
    return label, size, stats, hist


def device(eng, pos, types, ntypes, rlink, group=None, exclusions=None, n=None, nhist=None, dtype=None, links=None):
    """One labelling on a new object (or on `links`), read back: (label, size, stats, hist) as int64 arrays; label and size by
    caller index, SENTINEL where the call did not write.  status() must be 0."""
    import torch
    dtype = dtype or torch.int32
    own = links is None
    links = eng.clusters(types, ntypes, rlink, n) if own else links
    rows = len(pos)
    label = torch.full((rows,), SENTINEL, dtype=dtype, device="cuda")
    size = torch.full((rows,), SENTINEL, dtype=dtype, device="cuda")
    stats = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    members = rows if group is None else len(group)
    hist = torch.zeros(members if nhist is None else nhist, dtype=torch.int64, device="cuda")
    g = None if group is None else torch.tensor(np.asarray(group), dtype=torch.int32, device="cuda")
    out = eng.cluster_label(to4(pos), links, label=label, size=size, stats=stats, hist=hist, group=g, exclusions=exclusions)
    assert out[0] is label and out[1] is size and out[2] is stats and out[3] is hist
    got = tuple(t.cpu().numpy().astype(np.int64) for t in out)
    assert links.status() == 0
    if own:
        links.close()
    return got


def assert_equal(got, want, what=""):
    for name, g, w in zip(("label", "size", "stats", "hist"), got, want):
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:5].ravel().tolist())


# -- rows and regimes ------------------------------------------------------------------------------------------------------------------

@BOXES
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300, 513])
def test_rows_and_regimes(n, box):
    """One lane, one pair, a wave and a workgroup less one, full, plus one; two workgroups and a third with one lane -- each from many
    small clusters (rlink = 1) through the threshold (1.5, 1.8) to one cluster (3, rcut)."""
    eng = engine(box)
    pos = points(box, n)
    for rlink in (1.0, 1.5, 1.8, 3.0, rcut(box)):
        want = reference(pos, box, None, 1, rlink)
        label, size, stats, hist = want
        print(f"n = {n}, rlink = {rlink:.4f}: {stats[0]} clusters, largest {stats[1]}, {hist[0]} singletons")
        if n == NMAX and rlink == 1.0:
            assert hist[0] > 200
        if n == NMAX and rlink == 1.5:
            assert stats[1] > 100 and hist[0] > 20
        if n == NMAX and rlink >= 3.0:
            assert stats.tolist() == [1, 513, 513 * 513, 513]
        assert_equal(device(eng, pos, None, 1, rlink), want, (n, rlink))


# -- contention and depth ----------------------------------------------------------------------------------------------------------------

def lattice(seed=3):
    """8^3 sites at spacing 1.75 in the 14^3 box, in a shuffled caller order: (pos, ix) with ix the x plane of every particle."""
    k = np.arange(8)
    idx = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    order = np.random.default_rng(seed).permutation(512)
    idx = idx[order]
    return (idx + 0.5) * 1.75 - 7.0, idx[:, 0]


def test_lattice_every_particle_hooks_into_one_tree():
    eng = engine(CUBIC)
    pos, _ = lattice()
    want = reference(pos, CUBIC, None, 1, 1.75 * (1.0 + 1e-6))
    assert want[2].tolist() == [1, 512, 512 * 512, 512] and not want[0].any()              # one cluster through all six faces
    (i, j), _ = cr.links(pos, CUBIC, None, 1, 1.75 * (1.0 + 1e-6), port())
    assert len(i) == 3 * 512                                                                 # six links per particle
    assert_equal(device(eng, pos, None, 1, 1.75 * (1.0 + 1e-6)), want)
    want = reference(pos, CUBIC, None, 1, 1.75 * (1.0 - 1e-6))
    assert want[2].tolist() == [512, 1, 512, 512] and np.array_equal(want[0], np.arange(512))
    assert_equal(device(eng, pos, None, 1, 1.75 * (1.0 - 1e-6)), want)


def test_lattice_with_two_planes_of_another_type():
    eng = engine(CUBIC)
    pos, ix = lattice()
    types = np.isin(ix, (2, 5)).astype(np.int64)                                             # the x planes 2 and 5 are B
    r = 1.75 * (1.0 + 1e-6)
    want = reference(pos, CUBIC, types, 2, {(0, 0): r})                                      # A-B and B-B off
    assert want[2][0] == 2 + 128 and want[3][0] == 128 and sorted(np.unique(want[1]).tolist()) == [1, 128, 256]
    slab = want[0][ix == 6][0]
    assert (want[0][np.isin(ix, (6, 7, 0, 1))] == slab).all()                                # merged across the periodic face
    assert_equal(device(eng, pos, types, 2, {(0, 0): r}), want)
    want = reference(pos, CUBIC, types, 2, {(0, 1): r})                                      # only A-B on
    assert want[2].tolist() == [256, 3, 128 * 9 + 128, 512] and want[3][:3].tolist() == [128, 0, 128]
    assert (want[1][np.isin(ix, (1, 2, 3, 4, 5, 6))] == 3).all() and (want[1][np.isin(ix, (0, 7))] == 1).all()
    assert_equal(device(eng, pos, types, 2, {(0, 1): r}), want)


def serpentine(nbeads, step):
    """A chain that fills the box plane by plane, row by row: consecutive beads `step` apart, everything else at least sqrt(2) step."""
    pts = []
    y, dy, x, dx = 0, 1, 0, 1
    for z in range(0, 13, 2):
        for row in range(7):
            for _ in range(15):
                pts.append((x, y, z))
                x += dx
            x -= dx
            dx = -dx
            if row < 6:
                pts.append((x, y + dy, z))
                y += 2 * dy
        dy = -dy
        pts.append((x, y, z + 1))
    assert len(pts) >= nbeads
    return np.array(pts[:nbeads], dtype=float) * step - 6.5


def test_chain_in_three_caller_orders():
    eng = engine(CUBIC)
    rlink = 1.0
    pos = serpentine(NMAX, 0.9 * rlink)
    (i, j), clear = cr.links(pos, CUBIC, None, 1, rlink, port())
    assert len(i) == NMAX - 1 and np.array_equal(j - i, np.ones(NMAX - 1, dtype=int)) and clear > 0.09      # a chain and nothing else
    base = device(eng, pos, None, 1, rlink)
    assert base[2].tolist() == [1, NMAX, NMAX * NMAX, NMAX] and not base[0].any()
    for order in (np.arange(NMAX)[::-1], np.random.default_rng(9).permutation(NMAX)):
        want = reference(pos[order], CUBIC, None, 1, rlink)
        got = device(eng, pos[order], None, 1, rlink)
        assert_equal(got, want)
        assert_equal(got, base)                                                              # equal labels, whatever the order
    half = reference(pos, CUBIC, None, 1, 0.89 * rlink)
    assert half[2][0] == NMAX
    assert_equal(device(eng, pos, None, 1, 0.89 * rlink), half)


# -- types and pair-type switches --------------------------------------------------------------------------------------------------------

@BOXES
@pytest.mark.parametrize("ntypes", [1, 2, 3, 8])
def test_types_and_pair_type_switches(ntypes, box):
    eng = engine(box)
    pos, types = points(box, 300), types_of(300, ntypes)
    assert len(set(types.tolist())) == ntypes
    npt = ntypes * (ntypes + 1) // 2
    ty = None if ntypes == 1 else types
    pairs = [(a, b) for a in range(ntypes) for b in range(a, ntypes)]
    for a, b in pairs:                                                                         # one pair type on at a time, all 36 at eight types
        want = reference(pos, box, ty, ntypes, {(b, a): 2.2})
        assert 1 < want[2][0] < 300
        assert_equal(device(eng, pos, ty, ntypes, {(b, a): 2.2}), want, (a, b))
    rlink = 1.0 + 1.5 * np.random.default_rng(31).uniform(size=npt)                            # another distance for every pair type
    want = reference(pos, box, ty, ntypes, rlink)
    assert (ntypes == 1 or want[2][0] > 1) and want[2][0] < 300 and want[2][1] > 5
    assert_equal(device(eng, pos, ty, ntypes, rlink), want)
    assert_equal(device(eng, pos, ty, ntypes, 1.5), reference(pos, box, ty, ntypes, 1.5))


@BOXES
def test_no_types_short_types_and_an_unused_type(box):
    eng = engine(box)
    pos, types = points(box, 300), types_of(300, 2)
    one = reference(pos, box, None, 1, 1.5)
    assert_equal(device(eng, pos, None, 1, 1.5), one)                                          # types_host = NULL
    assert_equal(device(eng, pos, np.zeros(300, dtype=int), 1, 1.5), one)                      # ... is ntypes = 1
    rl = {(0, 0): 1.5, (0, 1): 1.2, (1, 1): 2.0, (2, 2): 3.0, (0, 2): 3.0}                     # a third type declared, never used
    assert_equal(device(eng, pos, types, 3, rl), reference(pos, box, types, 3, rl))
    assert_equal(device(eng, pos, types, 3, rl), reference(pos, box, types, 2, {k: v for k, v in rl.items() if 2 not in k}))
    short = types.copy()
    short[200:] = 0                                                                            # the particles past the types act as type 0
    assert_equal(device(eng, pos, types[:200], 2, [1.5, 1.2, 2.0]), reference(pos, box, short, 2, [1.5, 1.2, 2.0]))


# -- outputs -----------------------------------------------------------------------------------------------------------------------------

def test_outputs_alone_together_and_accumulated():
    import torch
    box = TILTED
    eng = engine(box)
    pos, other = points(box, 300), points(box)[213:]
    a, b = reference(pos, box, None, 1, 1.5), reference(other, box, None, 1, 1.5)
    assert not np.array_equal(a[3], b[3]) and a[2][0] > 20
    links = eng.clusters(None, 1, 1.5)
    dpos = to4(pos)
    new = lambda n, dt=torch.int32: torch.full((n,), SENTINEL, dtype=dt, device="cuda")   # noqa: E731
    # each alone
    label, size, stats, hist = new(300), new(300), new(4, torch.int64), torch.zeros(300, dtype=torch.int64, device="cuda")
    eng.cluster_label(dpos, links, label=label)
    eng.cluster_label(dpos, links, size=size)
    eng.cluster_label(dpos, links, stats=stats)
    eng.cluster_label(dpos, links, hist=hist)
    assert_equal([t.cpu().numpy() for t in (label, size, stats, hist)], a, "alone")
    # int64 labels and sizes
    assert_equal(device(eng, pos, None, 1, 1.5, dtype=torch.int64, links=links), a, "int64")
    # hist accumulates, stats is overwritten
    pre = np.random.default_rng(3).integers(0, 2 ** 40, size=300)
    hist = torch.tensor(pre, dtype=torch.int64, device="cuda")
    eng.cluster_label(dpos, links, stats=stats, hist=hist)
    eng.cluster_label(dpos, links, stats=stats, hist=hist)
    assert np.array_equal(hist.cpu().numpy(), pre + 2 * a[3]) and np.array_equal(stats.cpu().numpy(), a[2])
    eng.cluster_label(to4(other), links, stats=stats, hist=hist)
    assert np.array_equal(hist.cpu().numpy(), pre + 2 * a[3] + b[3]) and np.array_equal(stats.cpu().numpy(), b[2])
    # the overflow bin
    for nhist in (1, 5, 300):
        want = reference(pos, box, None, 1, 1.5, nhist=nhist)
        assert want[3].sum() == a[2][0] and (nhist == 300 or want[3][-1] > 0)
        assert_equal(device(eng, pos, None, 1, 1.5, nhist=nhist, links=links), want, nhist)
    big = reference(pos, box, None, 1, 3.0, nhist=70)                                          # a cluster beyond the bins summed in LDS
    assert big[3][-1] == 1 and big[2][1] == 300
    assert_equal(device(eng, pos, None, 1, 3.0, nhist=70), big)
    assert_equal(device(eng, pos, None, 1, 3.0), reference(pos, box, None, 1, 3.0))
    # two calls in a row: equal bits
    assert_equal(device(eng, pos, None, 1, 1.5, links=links), device(eng, pos, None, 1, 1.5, links=links))
    with pytest.raises(ValueError, match="all None"):
        eng.cluster_label(dpos, links)
    with pytest.raises(ValueError, match="label must be"):
        eng.cluster_label(dpos, links, label=new(299))
    with pytest.raises(ValueError, match="stats must be"):
        eng.cluster_label(dpos, links, stats=new(4))
    with pytest.raises(ValueError, match="hist must be"):
        eng.cluster_label(dpos, links, hist=new(8))
    links.close()
    with pytest.raises(ValueError, match="closed"):
        eng.cluster_label(dpos, links, label=label)


@BOXES
def test_group_of_every_other_particle(box):
    eng = engine(box)
    pos, types = points(box), types_of(NMAX, 2)
    members = np.arange(0, NMAX, 2)
    rl = [2.2, 1.8, 2.5]
    label, size, stats, hist = reference(pos[members], box, types[members], 2, rl, ids=members)
    assert 1 < stats[0] < len(members) and stats[3] == len(members)
    got = device(eng, pos, types, 2, rl, group=members)                                        # types and labels are caller indices
    assert np.array_equal(got[0][members], label) and np.array_equal(got[1][members], size)
    assert (got[0][1::2] == SENTINEL).all() and (got[1][1::2] == SENTINEL).all()               # entries outside the group are left alone
    assert np.array_equal(got[2], stats) and np.array_equal(got[3], hist)


# -- invariance --------------------------------------------------------------------------------------------------------------------------

@BOXES
def test_particle_order_and_type_labels(box):
    eng = engine(box)
    pos, types = points(box, 300), types_of(300, 3)
    rl = {(0, 0): 1.5, (0, 1): 2.0, (1, 1): 1.2, (1, 2): 2.4, (2, 2): 1.8}
    want = reference(pos, box, types, 3, rl)
    assert 1 < want[2][0] < 300
    assert_equal(device(eng, pos, types, 3, rl), want)
    perm = np.random.default_rng(8).permutation(300)
    got = device(eng, pos[perm], types[perm], 3, rl)
    assert_equal(got, reference(pos[perm], box, types[perm], 3, rl))
    inv = np.empty(300, dtype=np.int64); inv[perm] = np.arange(300)
    assert np.array_equal(got[1], want[1][perm]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    # the same partition: particles share a label after the permutation exactly when they did before, and the label is the least new index
    assert np.array_equal(got[0], np.array([inv[np.nonzero(want[0] == want[0][p])[0]].min() for p in perm]))
    relabel = np.array([2, 0, 1])                                                              # A -> C, B -> A, C -> B, with their rlink
    swapped = {(int(relabel[a]), int(relabel[b])): r for (a, b), r in rl.items()}
    assert_equal(device(eng, pos, relabel[types], 3, swapped), want)


# -- exclusions --------------------------------------------------------------------------------------------------------------------------

@BOXES
def test_exclusions_on_chains(box):
    eng = engine(box)
    pos, types, bonds, _ = chains(box)
    n, rlink = len(pos), 0.97                                                                  # bonds are 0.95 long
    (i, j), clear = cr.links(pos, box, None, 1, rlink, port())
    cr.assert_clear(clear)
    linked = set(zip(i.tolist(), j.tolist()))
    assert all(tuple(b) in linked for b in bonds.tolist())                                     # every bond is a link ...
    # (... but not the only ones: the chains are random walks that cross, beads that are not bonded come as close as 0.035, so no
    # link distance reaches the bonded neighbours alone; what holds is stated on the reference and the device must equal it)
    without = reference(pos, box, None, 1, rlink)
    assert all(len(set(without[0][c:c + 10].tolist())) == 1 for c in range(0, n, 10)) and without[2][0] <= 30    # the chains, some joined
    alone = reference(pos, box, None, 1, rlink, excl=bonds)
    (ie, je), _ = cr.links(pos, box, None, 1, rlink, port(), excl=bonds)
    assert len(ie) == len(i) - len(bonds) and alone[2][0] > 5 * without[2][0] and alone[3][0] > 100               # mostly singletons
    ex = eng.exclusions(bonds)
    assert_equal(device(eng, pos, None, 1, rlink), without)
    assert_equal(device(eng, pos, None, 1, rlink, exclusions=ex), alone)
    # a longer reach, typed, on a group: exclusions and types are caller indices
    rl = [1.6, 1.3, 1.9]
    members = np.sort(np.random.default_rng(6).choice(n, 200, replace=False))
    label, size, stats, hist = reference(pos[members], box, types[members], 2, rl, excl=bonds, ids=members)
    free = reference(pos[members], box, types[members], 2, rl, ids=members)
    assert stats[0] > free[2][0]
    got = device(eng, pos, types, 2, rl, group=members, exclusions=ex)
    assert np.array_equal(got[0][members], label) and np.array_equal(got[1][members], size)
    assert np.array_equal(got[2], stats) and np.array_equal(got[3], hist)
    assert_equal(device(eng, pos, types, 2, rl, exclusions=ex), reference(pos, box, types, 2, rl, excl=bonds))
    ex.close()


# -- many-cell grids ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cg.NAMES)
def test_many_cell_grids(name):
    """rlink = rcut for all pairs: the partners planted 1e-9 inside the cutoff share their site's label, those 1e-9 outside are settled
    by the reference (another path may join them), the pairs through every face, edge, corner and block boundary are joined."""
    import pse_amd
    c = cg.build(name, port())
    pos, box, n = c["pos"], c["box"], c["n"]
    eng = pse_amd.Engine(n, box, xi=c["xi"], error=c["error"], max_strain=c["max_strain"], seed=77)
    rlink = eng.info()["rcut"]
    assert abs(rlink - c["rcut"]) <= 1e-15 * c["rcut"]
    want = reference(pos, box, None, 1, rlink, nhist=64)
    label = want[0]
    inside = [(i, j) for i, j, cname, ins, _ in c["planted"] if cname == "rcut" and ins]
    assert len(inside) == (0 if name == "one_cell_x" else cg.N_SITES)
    assert all(label[i] == label[j] for i, j in inside) and all(label[i] == label[j] for i, j, _ in c["crossers"])
    assert len(c["crossers"]) >= 13 or name == "one_cell_x"
    links = eng.clusters(None, 1, rlink)
    for which in ("wide", "narrow"):
        eng.set_neighbor_skin(c["skin"] if which == "wide" else 0.0)
        got = device(eng, pos, None, 1, rlink, nhist=64, links=links)
        info = eng.info()
        assert (info["ncell_x"], info["ncell_y"], info["ncell_z"]) == c["cells_" + which][:3]
        assert_equal(got, want, (name, which))
    # a shorter reach, where the system is not one cluster
    short = reference(pos, box, None, 1, 0.3 * rlink, nhist=64)
    assert short[2][0] > 10
    assert_equal(device(eng, pos, None, 1, 0.3 * rlink, nhist=64), short, (name, "short"))
    links.close()
    eng.close()


# -- the raw C-ABI -----------------------------------------------------------------------------------------------------------------------

def test_misuse_is_reported_before_any_launch():
    """Raw C-ABI, as a C host would call it: a rejected call leaves the outputs untouched, and the handle works afterwards."""
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
    box = CUBIC
    pos = points(box, n)
    types = types_of(n, 2).astype(np.uint32)
    rl = np.array([1.5, 1.2, 2.0])
    rc, h = create(box[0], n)
    assert rc == 0, msg()
    rc, h2 = create(box[0], n)
    assert rc == 0, msg()
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()

    def links_on(hh, expect=0, word=None, ty=types, ntypes=2, r=rl, nn=n):
        g = ctypes.c_void_p(777)
        assert lib.pse_clusters_create(hh, nn, None if ty is None else vp(ty), ntypes, None if r is None else vp(r), ctypes.byref(g)) == expect, msg()
        assert expect == 0 or (word in msg() and "pse_clusters_create" in msg() and not g.value), (word, msg())
        return g

    g = links_on(h)
    big = types.copy()
    big[5] = 2
    links_on(h, INVALID, "type 2", ty=big)
    links_on(h, INVALID, "ntypes = 9", ntypes=9)
    links_on(h, INVALID, "null rlink_host", r=None)
    links_on(h, INVALID, "not finite", r=np.array([1.5, np.nan, 1.0]))
    links_on(h, INVALID, "negative", r=np.array([1.5, -1.0, 1.0]))
    links_on(h, INVALID, "rcut", r=np.array([1.5, 5.3, 1.0]))
    links_on(h, INVALID, "every pair type is off", r=np.zeros(3))
    links_on(h, INVALID, "n_max", nn=n + 1)
    links_on(None, INVALID, "null handle")
    gs = links_on(hs)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex2 = ctypes.c_void_p()
    assert lib.pse_exclusions_create(h2, n, 1, vp(pairs), ctypes.byref(ex2)) == 0, msg()
    dpos = to4(pos)
    label = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    size = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    stats = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    hist = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    call = lib.pse_clusters_label

    def refused(word, gg=g, p=P(dpos), nn=n, lab=P(label), sz=P(size), st=P(stats), hi=P(hist), nh=n, e=None):
        assert call(gg, p, None, nn, lab, sz, st, hi, nh, e) == INVALID, word
        assert word in msg() and "pse_clusters_label" in msg(), (word, msg())

    refused("null cluster object", gg=None)
    refused("n_max", nn=0)
    refused("n_max", nn=n + 1)
    refused("null pos", p=None)
    refused("all null", lab=None, sz=None, st=None, hi=None)
    refused("stats is not 8-byte aligned", st=ctypes.c_void_p(stats.data_ptr() + 4))
    refused("hist is not 8-byte aligned", hi=ctypes.c_void_p(hist.data_ptr() + 4))
    refused("nhist = 0", nh=0)
    refused("another handle", e=ex2)
    refused("slab rank", gg=gs)
    torch.cuda.synchronize()
    for t in (label, size, stats, hist):
        assert np.all(t.cpu().numpy() == SENTINEL)                                             # nothing was launched, nothing was written
    word = ctypes.c_uint(99)
    assert lib.pse_clusters_status(None, ctypes.byref(word)) == INVALID and "null cluster object" in msg()
    assert lib.pse_clusters_status(g, None) == INVALID and "null status" in msg()
    hist.zero_()
    assert call(g, P(dpos), None, n, P(label), P(size), P(stats), P(hist), n, None) == 0, msg()
    assert lib.pse_clusters_status(g, ctypes.byref(word)) == 0 and word.value == 0
    want = reference(pos, box, types, 2, rl)
    assert 1 < want[2][0] < n
    assert_equal([t.cpu().numpy() for t in (label, size, stats, hist)], want)
    assert lib.pse_clusters_destroy(g) == 0
    assert lib.pse_clusters_destroy(None) == 0
    g = links_on(h)                                                                            # still alive below: it goes with its handle
    for hh in (h, h2, hs):
        assert lib.pse_destroy(hh) == 0


# -- a captured graph --------------------------------------------------------------------------------------------------------------------

def test_captured_graph_replayed_twice():
    import pse_amd
    import torch
    box = TILTED
    frames = [points(box, 300), points(box)[213:]]
    wants = [reference(p, box, None, 1, 1.5) for p in frames]
    assert not np.array_equal(wants[0][0], wants[1][0])
    eng = pse_amd.Engine(300, box, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    links = eng.clusters(None, 1, 1.5)
    pos = to4(frames[0])
    label = torch.full((300,), SENTINEL, dtype=torch.int32, device="cuda")
    size = torch.full((300,), SENTINEL, dtype=torch.int32, device="cuda")
    stats = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    hist = torch.zeros(300, dtype=torch.int64, device="cuda")
    sample = lambda: eng.cluster_label(pos, links, label=label, size=size, stats=stats, hist=hist)   # noqa: E731
    with torch.cuda.stream(st):
        sample()                                                                               # warm-up outside the capture
    st.synchronize()
    assert_equal([t.cpu().numpy() for t in (label, size, stats, hist)], wants[0], "eager")
    hist.zero_(); label.fill_(SENTINEL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        sample()
    torch.cuda.synchronize()
    assert not hist.cpu().numpy().any() and (label.cpu().numpy() == SENTINEL).all(), "a capture runs nothing"
    total = np.zeros(300, dtype=np.int64)
    for k, p in enumerate(frames):
        pos.copy_(to4(p))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        total += wants[k][3]
        got = [t.cpu().numpy() for t in (label, size, stats, hist)]
        assert_equal(got[:3], wants[k][:3], ("replay", k))
        assert np.array_equal(got[3], total)
    assert links.status() == 0
    links.close()
    eng.close()


# -- analyze.Clusters --------------------------------------------------------------------------------------------------------------------

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


def test_clusters_through_system_run(restored_context):
    """period, the ring and its rows, labels(), sizes(), members(), the size distribution and the averages against the reference on
    the positions of every sampled step; the particles move in a Morse well outside a harmonic core, so the samples differ."""
    import math
    from pse_amd import analyze, forces
    box = CUBIC
    pos = points(box)
    n = len(pos)
    s, pse = system(pos, box)
    forces.TablePair.from_functions(pse, lambda r: 100.0 * (2.0 - r) ** 2, lambda r: 200.0 * (2.0 - r), 0.0, 2.0, 256)
    D, alpha, r0, r1 = 30.0, 4.0, 2.1, 3.2
    e = lambda r: math.exp(-alpha * (r - r0))               # noqa: E731
    forces.TablePair.from_functions(pse, lambda r: D * ((1.0 - e(r)) ** 2 - 1.0), lambda r: -2.0 * D * alpha * (1.0 - e(r)) * e(r), 2.0, r1, 512)
    names = ["A", "B"]
    types = types_of(n, 2)
    rl = {("A", "A"): 1.8, ("B", "A"): 1.5}                                                    # B-B never links; 86 clusters at step 0
    coded = {(0, 0): 1.8, (0, 1): 1.5}
    cl = analyze.Clusters(pse, rl, types=[names[t] for t in types], type_names=names, period=2, nhist=6, capacity=2)
    assert s.analyzers == [cl] and cl.samples == 0
    for reader in (cl.labels, cl.sizes, cl.size_distribution, cl.number_average):
        with pytest.raises(ValueError, match="no samples"):
            reader()
    refs, steps, snaps = [], [], []
    for t in range(5):                                                                         # samples at steps 0, 2 and 4
        if t % 2 == 0:
            snap = s.pos.cpu().numpy()[:, :3].copy()
            snaps.append(snap)
            refs.append(reference(snap, box, types, 2, coded, nhist=6))
            steps.append(t)
        s.run(1)
    assert cl.samples == 3 and cl.status() == 0 and np.abs(snaps[0] - snaps[2]).max() > 1e-6
    table = cl.table()                                                                         # a ring of two rows: steps 2 and 4
    assert table.dtype == np.int64 and table.tolist() == [[steps[k]] + refs[k][2].tolist() for k in (1, 2)]
    assert np.array_equal(cl.labels(), refs[2][0]) and np.array_equal(cl.sizes(), refs[2][1])
    ns = cl.size_distribution()
    assert np.array_equal(ns * 3, refs[0][3] + refs[1][3] + refs[2][3])
    assert abs(ns.sum() - np.mean([r[2][0] for r in refs])) < 1e-12                            # sums to the mean number of clusters
    kept = np.array([refs[k][2] for k in (1, 2)], dtype=float)
    assert cl.number_average() == kept[:, 3].sum() / kept[:, 0].sum() and cl.weight_average() == kept[:, 2].sum() / kept[:, 3].sum()
    assert cl.largest_fraction() == (kept[:, 1] / kept[:, 3]).mean() and cl.weight_average() > cl.number_average() > 1.0
    big = int(refs[2][0][np.argmax(refs[2][1])])
    assert np.array_equal(cl.members(big), np.nonzero(refs[2][0] == big)[0]) and len(cl.members(big)) == refs[2][2][1]
    cl.reset()
    assert cl.samples == 0 and len(cl.table()) == 0
    s.run(1)                                                                                   # step 5: not a sample
    assert cl.samples == 0
    snap = s.pos.cpu().numpy()[:, :3].copy()
    s.run(1)                                                                                   # step 6
    want = reference(snap, box, types, 2, coded, nhist=6)
    assert cl.samples == 1 and cl.table().tolist() == [[6] + want[2].tolist()] and np.array_equal(cl.size_distribution(), want[3])
    with pytest.raises(ValueError, match="entries"):
        analyze.Clusters(pse, 2.0, types=types[:-1])
    with pytest.raises(RuntimeError, match="rcut"):
        analyze.Clusters(pse, 5.3)
    assert s.analyzers == [cl]


def test_clusters_on_a_group_with_exclusions(restored_context):
    from pse_amd import analyze, forces
    box = TILTED[:3] + (0.0,)
    pos, types, bonds, _ = chains(box)
    members = np.arange(0, len(pos) - 50)
    s, pse = system(pos, box, members)
    excl = forces.Exclusions(pse, bonds)
    cl = analyze.Clusters(pse, 1.6, types=types, exclusions=excl)
    s.run(1)
    label, size, stats, hist = reference(pos[members], box, types[members], 2, 1.6, excl=bonds, ids=members, nhist=len(pos))
    assert 1 < stats[0] < len(members)
    assert np.array_equal(cl.labels()[members], label) and np.array_equal(cl.sizes()[members], size)
    assert (cl.labels()[len(members):] == -1).all() and not cl.sizes()[len(members):].any()
    assert cl.table().tolist() == [[0] + stats.tolist()] and np.array_equal(cl.size_distribution(), hist)


def test_clusters_die_with_the_engine_that_set_params_replaces(restored_context):
    """The device object does not outlive its handle: after setParams() the analyzer says so, nothing is freed twice, and a new one
    on the new handle finds what the old one found (tests/test_gpu_provider_lifetime.py)."""
    from pse_amd import analyze
    box = CUBIC
    pos = points(box, 300)
    s, pse = system(pos, box)
    old = analyze.Clusters(pse, 1.5)
    s.run(1)
    kept = old.labels()
    assert np.array_equal(kept, reference(pos, box, None, 1, 1.5)[0]) and pse.engine.serial == 1
    pse.cpp_method.setParams()                                     # a new handle; pse_destroy freed the device object
    assert pse.engine.serial == 2
    with pytest.raises(ValueError, match="setParams"):
        old.analyze(0)
    with pytest.raises(ValueError, match="setParams"):
        old.status()
    assert np.array_equal(old.labels(), kept) and old.samples == 1  # the outputs are tensors of the analyzer's own: still readable
    del s.analyzers[:]
    with _Unraisable() as quiet:
        del old
        gc.collect()
    assert quiet.seen == []
    new = analyze.Clusters(pse, 1.5)
    new.analyze(0)
    assert np.array_equal(new.labels(), kept) and new.status() == 0
    s.analyzers.remove(new)
    with _Unraisable() as quiet:                                   # a collected analyzer frees its object, the handle lives on
        del new
        gc.collect()
    assert quiet.seen == [] and s.analyzers == []
