"""GPU tests of the bond-orientational order (pse_bond_order_create, pse_bond_order_compute, pse_bond_order_histogram) and of
analyze.BondOrder on top of it, against the O(N^2) reference of tests/bond_order_ref.py (validated on the CPU by
tests/test_bond_order_cpu.py): random inputs over the wave / workgroup edges in both boxes and every degree; perfect lattices, also in a
box tilted by a lattice vector; pairs along the axes; solid-like bonds on a half-disordered crystal; the numbers of types and the
pair-type switches; a group, exclusions, particle order and repeated calls; every output alone; the many-cell grids of
tests/cell_grid_cases.py; the histogram; the error returns of the raw C-ABI and the lifetime of the object; a captured graph; and
BondOrder through System.run, on the crystal and on a dilute system whose single-neighbour particles have q = 1 up to rounding.

The integer outputs (nnb, nconn, stats) must EQUAL the reference: every input is first held to its clearance condition (1e-9 from
every neighbour distance and from the threshold).  q and qbar must lie within bond_order_ref.bound: the bound derived from the order
of the kernel's operations (test_bond_order_cpu.test_kernel_recurrence_against_mpmath holds it against 40 digits), evaluated for the
largest number of neighbours and the shortest bond of the input."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
import bond_order_ref as br
import cell_grid_cases as cg
from pair_table_ref import random_points
from test_gpu_pair_typed import chains

pytestmark = pytest.mark.gpu

NMAX = 513
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
FCC_BOX = (12.0, 12.0, 12.0, 0.0)
BOXES = pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
INVALID = -1
SENTINEL = -7
FCC_RNB = 3.4                       # between the first (2 sqrt 2 = 2.83) and the second (4) shell of the fcc lattice of cubic cell 4


def port():
    from oracle import pse_port
    pse_port.lib()
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box, nmax=NMAX):
    import pse_amd
    return pse_amd.Engine(nmax, box, xi=0.5, error=1e-3)


@functools.lru_cache(maxsize=None)
def points(box, n=NMAX):
    """The first n of the 513 seeded points of the box."""
    pos = random_points(NMAX, box, seed=11)[:n].copy()
    pos.setflags(write=False)
    return pos


def types_of(n, ntypes, seed=21):
    return np.random.default_rng(seed).integers(0, ntypes, n)


def reference(pos, box, types, ntypes, rnb, degrees, **kw):
    ref = br.bond_order(pos, box, types, ntypes, rnb, degrees, port(), **kw)
    br.assert_clear(ref["clear"])
    return ref


def device(eng, pos, types, ntypes, rnb, degrees, solid=None, group=None, exclusions=None, n=None, shells=None, only=None):
    """One compute on a new object (or on `shells`), read back: a dict of nnb, nconn (int64), q, qbar (float64) by caller index and
    stats, SENTINEL where the call did not write.  `only`: the names of the outputs to pass (default: all)."""
    import torch
    own = shells is None
    shells = eng.bond_order_shells(types, ntypes, rnb, degrees, n) if own else shells
    rows, nl = len(pos), len(degrees)
    out = dict(nnb=torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda"),
               q=torch.full((rows, nl), float(SENTINEL), dtype=torch.float64, device="cuda"),
               qbar=torch.full((rows, nl), float(SENTINEL), dtype=torch.float64, device="cuda"),
               nconn=torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda"),
               stats=torch.full((ntypes, 2), SENTINEL, dtype=torch.int64, device="cuda"))
    g = None if group is None else torch.tensor(np.asarray(group), dtype=torch.int32, device="cuda")
    passed = {k: (v if only is None or k in only else None) for k, v in out.items()}
    eng.bond_order(to4(pos), shells, solid=solid, group=g, exclusions=exclusions, **passed)
    got = {k: v.cpu().numpy().astype(np.int64 if v.dtype != torch.float64 else np.float64) for k, v in out.items()}
    if own:
        shells.close()
    return got


def assert_matches(got, ref, box, degrees, what="", rows=None, solid=True):
    """nnb (and with a solid pass nconn, stats) equal, q and qbar within the derived bound; rows: the caller indices of the reference's rows."""
    rows = np.arange(len(ref["nnb"])) if rows is None else np.asarray(rows)
    assert np.array_equal(got["nnb"][rows], ref["nnb"]), (what, "nnb", int((got["nnb"][rows] != ref["nnb"]).sum()))
    dpos = br.separation_error(box, ref["rmin"]) if np.isfinite(ref["rmin"]) else 0.0
    for col, l in enumerate(degrees):
        for name, avg in (("q", False), ("qbar", True)):
            err = np.abs(got[name][rows, col] - ref[name][:, col]).max()
            tol = br.bound(l, ref["nbmax"], dpos, averaged=avg)
            print(f"{what} {name}_{l}: error {err:.3e}, bound {tol:.3e} (nb <= {ref['nbmax']}, shortest bond {ref['rmin']:.3f})")
            assert err <= tol, (what, name, l, err, tol)
    assert not np.isnan(got["q"]).any() and not np.isnan(got["qbar"]).any()
    assert np.array_equal(got["stats"][:, 0], ref["stats"][:, 0]), (what, "members")
    if solid and ref["nconn"] is not None:
        assert np.array_equal(got["nconn"][rows], ref["nconn"]), (what, "nconn", int((got["nconn"][rows] != ref["nconn"]).sum()))
        assert np.array_equal(got["stats"], ref["stats"]), (what, "stats")


# -- random inputs -------------------------------------------------------------------------------------------------------------------

@BOXES
@pytest.mark.parametrize("degrees", [(4, 6), (2, 8, 10, 12)], ids=["l4-6", "l2-8-10-12"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_random_inputs(n, degrees, box):
    """One lane, one pair, a wave and a workgroup less one, full, plus one; two workgroups and a third with one lane; about 20
    neighbours per particle at the full size."""
    pos = points(box, n)
    solid = (degrees[-1], 0.2, 3)
    ref = reference(pos, box, None, 1, 3.0, degrees, solid=solid)
    if n == NMAX:
        assert 15 < ref["nnb"].mean() < 25 and 0 < ref["stats"][0, 1] < n
    got = device(engine(box), pos, None, 1, 3.0, degrees, solid=solid)
    assert_matches(got, ref, box, degrees, f"n = {n}")
    if n == 1:
        assert got["nnb"].tolist() == [0] and not got["q"].any() and not got["qbar"].any() and got["nconn"].tolist() == [0]
        assert got["stats"].tolist() == [[1, 0]]


@BOXES
def test_planted_isolated_particle(box):
    pos = points(box, 64).copy()
    grid = np.stack(np.meshgrid(*[np.linspace(-0.45, 0.45, 10) * L for L in box[:3]], indexing="ij"), axis=-1).reshape(-1, 3)
    d = port().min_image(grid[:, None, :] - pos[None, 1:, :], box)
    far = np.sqrt((d * d).sum(axis=2)).min(axis=1)
    assert far.max() > 3.3
    pos[0] = grid[np.argmax(far)]
    ref = reference(pos, box, None, 1, 3.0, (4, 6), solid=(6, 0.5, 1))
    assert ref["nnb"][0] == 0 and ref["nnb"][1:].max() > 0
    got = device(engine(box), pos, None, 1, 3.0, (4, 6), solid=(6, 0.5, 1))
    assert_matches(got, ref, box, (4, 6))
    assert got["nnb"][0] == 0 and not got["q"][0].any() and not got["qbar"][0].any() and got["nconn"][0] == 0


# -- lattices ------------------------------------------------------------------------------------------------------------------------

CLOSED = {"sc": {4: np.sqrt(7 / 12), 6: np.sqrt(1 / 8)}, "fcc": {4: np.sqrt(7 / 192), 6: np.sqrt(169 / 512)}}


@pytest.mark.parametrize("lattice,tilt", [("sc", 0.0), ("sc", 1.0 / 7.0), ("fcc", 0.0), ("fcc", 1.0 / 3.0)],
                         ids=["sc", "sc-tilted", "fcc", "fcc-tilted"])
def test_lattice_on_the_device(lattice, tilt):
    """Every particle sees the ideal shell, through every face of the box: the closed forms, q-bar = q, every bond solid-like.  The
    tilted boxes shift the y image by one lattice vector ((2, 14, 0) and (4, 12, 0)): the same crystal."""
    if lattice == "sc":
        pos, box, rnb, nb = br.sc_lattice(7, 2.0), (14.0, 14.0, 14.0, tilt), 2.5, 6
    else:
        pos, box, rnb, nb = br.fcc_lattice(3, 4.0), FCC_BOX[:3] + (tilt,), FCC_RNB, 12
    assert len(pos) == (343 if lattice == "sc" else 108)
    pos = cg.wrap(pos, box)
    for min_conn in (1, nb):
        ref = reference(pos, box, None, 1, rnb, (4, 6), solid=(6, 0.7, min_conn))
        assert (ref["nnb"] == nb).all() and ref["stats"].tolist() == [[len(pos), len(pos)]]
        got = device(engine(box, len(pos)), pos, None, 1, rnb, (4, 6), solid=(6, 0.7, min_conn))
        assert_matches(got, ref, box, (4, 6), lattice)
        assert (got["nconn"] == nb).all() and got["stats"].tolist() == [[len(pos), len(pos)]]
        dpos = br.separation_error(box, ref["rmin"])
        for col, l in enumerate((4, 6)):
            assert np.abs(got["q"][:, col] - CLOSED[lattice][l]).max() <= br.bound(l, nb, dpos) + 1e-12     # (1e-12: the reference's own, CPU-tested)
            assert np.abs(got["qbar"][:, col] - got["q"][:, col]).max() <= br.bound(l, nb, dpos, averaged=True) + br.bound(l, nb, dpos)


def test_pairs_along_the_axes():
    """A pair along +-z, +-x and +-y exactly: one neighbour each, q_l = 1 for every degree, nothing singular at the poles."""
    centres = np.array([[-5.0, -5.0, -5.0], [0.0, -5.0, -5.0], [5.0, -5.0, -5.0], [-5.0, 2.0, 2.0], [0.0, 2.0, 2.0], [5.0, 2.0, 2.0]])
    steps = 1.5 * np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=float)
    pos = np.concatenate([centres, centres + steps])
    for degrees in ((2, 4, 6), (8, 10, 12)):
        ref = reference(pos, CUBIC, None, 1, 2.0, degrees, solid=(degrees[0], 0.9, 1))
        assert (ref["nnb"] == 1).all() and np.abs(ref["q"] - 1.0).max() < 1e-13
        got = device(engine(CUBIC), pos, None, 1, 2.0, degrees, solid=(degrees[0], 0.9, 1))
        assert_matches(got, ref, CUBIC, degrees, "axes")
        assert (got["nconn"] == 1).all() and got["stats"].tolist() == [[12, 12]]
        for col, l in enumerate(degrees):
            assert np.abs(got["q"][:, col] - 1.0).max() <= br.bound(l, 1, br.separation_error(CUBIC, 1.5))


# -- solid-like bonds ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def half_crystal(amplitude=0.3, seed=2):
    """The fcc block with the half x > 0 displaced by a seeded jitter of the given amplitude."""
    pos = br.fcc_lattice(3, 4.0)
    rng = np.random.default_rng(seed)
    jitter = rng.uniform(-amplitude, amplitude, size=pos.shape)
    pos = pos + jitter * (pos[:, :1] > 0.0)
    pos.setflags(write=False)
    return pos


@pytest.mark.parametrize("min_conn", [1, 7])
@pytest.mark.parametrize("threshold", [0.5, 0.7])
@pytest.mark.parametrize("amplitude", [0.3, 0.8])
def test_solid_bonds_on_a_half_crystal(amplitude, threshold, min_conn):
    """At amplitude 0.3 the shaken half stays solid-like (s_ij > 0.88 everywhere, 11 or 12 connections); at 0.8 it melts: every
    number of connections from 0 to 12 occurs and about half of the particles are solid-like."""
    pos, box = half_crystal(amplitude), FCC_BOX
    ref = reference(pos, box, None, 1, FCC_RNB, (4, 6), solid=(6, threshold, min_conn))
    print(f"amplitude {amplitude}, threshold {threshold}, min_conn {min_conn}: solid-like {ref['stats'][0, 1]} of 108, clearance {ref['clear']}")
    if amplitude == 0.3:
        assert ref["stats"].tolist() == [[108, 108]] and set(ref["nconn"].tolist()) == {11, 12}
    else:
        assert len(set(ref["nconn"].tolist())) > 10 and (min_conn == 1 or 50 < ref["stats"][0, 1] < 70)
    got = device(engine(box, 108), pos, None, 1, FCC_RNB, (4, 6), solid=(6, threshold, min_conn))
    assert_matches(got, ref, box, (4, 6), "half crystal")


def test_no_solid_pass_leaves_nconn_alone():
    pos, box = half_crystal(), FCC_BOX
    ref = reference(pos, box, None, 1, FCC_RNB, (4, 6))
    got = device(engine(box, 108), pos, None, 1, FCC_RNB, (4, 6), solid=None)
    assert_matches(got, ref, box, (4, 6), "no solid pass")
    assert (got["nconn"] == SENTINEL).all() and got["stats"].tolist() == [[108, 0]]
    got = device(engine(box, 108), pos, None, 1, FCC_RNB, (4, 6), solid=None, only=("stats",))  # the members alone
    assert got["stats"].tolist() == [[108, 0]] and (got["nnb"] == SENTINEL).all()


# -- types and switches --------------------------------------------------------------------------------------------------------------

@BOXES
@pytest.mark.parametrize("ntypes", [1, 2, 3, 8])
def test_types_and_pair_type_switches(ntypes, box):
    eng = engine(box)
    pos, types = points(box, 300), types_of(300, ntypes)
    assert len(set(types.tolist())) == ntypes
    npt = ntypes * (ntypes + 1) // 2
    ty = None if ntypes == 1 else types
    degrees, solid = (6,), (6, 0.3, 2)
    full = reference(pos, box, ty, ntypes, 3.0, degrees, solid=solid)
    assert_matches(device(eng, pos, ty, ntypes, 3.0, degrees, solid=solid), full, box, degrees, "all on")
    if ntypes > 1:                                                                               # one pair type off: exactly those neighbours go
        rnb = np.full(npt, 3.0)
        rnb[1] = 0.0                                                                             # p(0, 1)
        ref = reference(pos, box, ty, ntypes, rnb, degrees, solid=solid)
        (i, j, _), _, _ = br.neighbours(pos, box, ty, ntypes, 3.0, port())
        gone = np.bincount(i[np.minimum(types[i], types[j]) + np.maximum(types[i], types[j]) * 8 == 8], minlength=300)
        assert np.array_equal(ref["nnb"], full["nnb"] - gone) and gone.sum() > 0
        got = device(eng, pos, ty, ntypes, rnb, degrees, solid=solid)
        assert_matches(got, ref, box, degrees, "A-B off")
        assert np.array_equal(got["nnb"], full["nnb"] - gone)
    rnb = 2.0 + 1.5 * np.random.default_rng(31).uniform(size=npt)                                 # another distance for every pair type
    ref = reference(pos, box, ty, ntypes, rnb, degrees, solid=solid)
    assert_matches(device(eng, pos, ty, ntypes, rnb, degrees, solid=solid), ref, box, degrees, "per pair type")
    if ntypes == 3:                                                                              # a relabelling permutes the stats rows
        relabel = np.array([2, 0, 1])
        swapped = {(int(relabel[a]), int(relabel[b])): rnb[a * 3 - a * (a - 1) // 2 + (b - a)] for a in range(3) for b in range(a, 3)}
        got = device(eng, pos, relabel[types], 3, swapped, degrees, solid=solid)
        assert np.array_equal(got["stats"][relabel], ref["stats"]) and np.array_equal(got["nnb"], ref["nnb"]) and np.array_equal(got["nconn"], ref["nconn"])


# -- group, exclusions, order --------------------------------------------------------------------------------------------------------

@BOXES
def test_group_of_every_third_particle(box):
    pos, types = points(box), types_of(NMAX, 2)
    members = np.arange(0, NMAX, 3)
    degrees, solid, rnb = (4, 6), (6, 0.3, 2), [4.0, 3.5, 4.5]
    ref = reference(pos[members], box, types[members], 2, rnb, degrees, solid=solid, ids=members)
    assert ref["nnb"].mean() > 8
    got = device(engine(box), pos, types, 2, rnb, degrees, solid=solid, group=members)            # types are caller indices
    assert_matches(got, ref, box, degrees, "group", rows=members)
    outside = np.setdiff1d(np.arange(NMAX), members)
    for name in ("nnb", "q", "qbar", "nconn"):
        assert (got[name][outside] == SENTINEL).all(), name                                      # rows outside the group keep the sentinel


@BOXES
def test_exclusions_on_chains(box):
    eng = engine(box)
    pos, types, bonds, _ = chains(box)
    degrees, solid = (4, 6), (6, 0.3, 2)
    free = reference(pos, box, types, 2, 2.5, degrees, solid=solid)
    ref = reference(pos, box, types, 2, 2.5, degrees, solid=solid, excl=bonds)
    assert ref["nnb"].sum() == free["nnb"].sum() - 2 * len(bonds)                                # every bond (0.95 long) was a neighbour pair
    ex = eng.exclusions(bonds)
    assert_matches(device(eng, pos, types, 2, 2.5, degrees, solid=solid), free, box, degrees, "free")
    assert_matches(device(eng, pos, types, 2, 2.5, degrees, solid=solid, exclusions=ex), ref, box, degrees, "excluded")
    members = np.sort(np.random.default_rng(6).choice(len(pos), 200, replace=False))
    sub = reference(pos[members], box, types[members], 2, 2.5, degrees, solid=solid, excl=bonds, ids=members)
    got = device(eng, pos, types, 2, 2.5, degrees, solid=solid, group=members, exclusions=ex)
    assert_matches(got, sub, box, degrees, "excluded group", rows=members)
    ex.close()


@BOXES
def test_particle_order_and_equal_bits(box):
    eng = engine(box)
    pos, types = points(box, 300), types_of(300, 2)
    degrees, solid, rnb = (4, 6, 12), (6, 0.3, 3), [3.0, 2.6, 3.2]
    ref = reference(pos, box, types, 2, rnb, degrees, solid=solid)
    shells = eng.bond_order_shells(types, 2, rnb, degrees)
    a = device(eng, pos, types, 2, rnb, degrees, solid=solid, shells=shells)
    b = device(eng, pos, types, 2, rnb, degrees, solid=solid, shells=shells)
    assert_matches(a, ref, box, degrees, "order")
    for name in a:
        assert np.array_equal(a[name], b[name]), name                                            # the same call twice: equal bits
    shells.close()
    perm = np.random.default_rng(8).permutation(300)
    c = device(eng, pos[perm], types[perm], 2, rnb, degrees, solid=solid)
    assert np.array_equal(c["nnb"], a["nnb"][perm]) and np.array_equal(c["nconn"], a["nconn"][perm]) and np.array_equal(c["stats"], a["stats"])
    assert_matches(c, reference(pos[perm], box, types[perm], 2, rnb, degrees, solid=solid), box, degrees, "permuted")
    dpos = br.separation_error(box, ref["rmin"])
    for col, l in enumerate(degrees):
        assert np.abs(c["q"][:, col] - a["q"][perm, col]).max() <= 2.0 * br.bound(l, ref["nbmax"], dpos)


# -- outputs -------------------------------------------------------------------------------------------------------------------------

def test_every_output_alone_and_together():
    import torch
    box = TILTED
    eng = engine(box)
    pos = points(box, 300)
    degrees, solid = (4, 6), (6, 0.3, 3)
    ref = reference(pos, box, None, 1, 3.0, degrees, solid=solid)
    shells = eng.bond_order_shells(None, 1, 3.0, degrees)
    together = device(eng, pos, None, 1, 3.0, degrees, solid=solid, shells=shells)
    assert_matches(together, ref, box, degrees, "together")
    for only in ("nnb", "q", "qbar", "nconn", "stats"):
        got = device(eng, pos, None, 1, 3.0, degrees, solid=solid, shells=shells, only=(only,))
        assert np.array_equal(got[only], together[only]), only                                   # equal bits, alone or together
        for other in got:
            assert other == only or (got[other] == SENTINEL).all(), (only, other)
    dpos = to4(pos)
    with pytest.raises(ValueError, match="all None"):
        eng.bond_order(dpos, shells)
    with pytest.raises(ValueError, match="nnb must be"):
        eng.bond_order(dpos, shells, nnb=torch.zeros(299, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="q must be"):
        eng.bond_order(dpos, shells, q=torch.zeros((300, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="stats must be"):
        eng.bond_order(dpos, shells, stats=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="degree 8"):
        eng.bond_order(dpos, shells, nnb=torch.zeros(300, dtype=torch.int32, device="cuda"), solid=(8, 0.5, 1))
    shells.close()
    with pytest.raises(ValueError, match="closed"):
        eng.bond_order(dpos, shells, nnb=torch.zeros(300, dtype=torch.int32, device="cuda"))


# -- many-cell grids -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cg.NAMES)
def test_many_cell_grids(name):
    """rnb = rcut: the neighbour set through every face, edge, corner and block boundary; nnb must be exact."""
    import pse_amd
    c = cg.build(name, port())
    pos, box, n = c["pos"], c["box"], c["n"]
    eng = pse_amd.Engine(n, box, xi=c["xi"], error=c["error"], max_strain=c["max_strain"], seed=77)
    rnb = eng.info()["rcut"]
    assert abs(rnb - c["rcut"]) <= 1e-15 * c["rcut"]
    degrees, solid = (4, 6), (6, 0.3, 3)
    ref = reference(pos, box, None, 1, rnb, degrees, solid=solid)
    short = reference(pos, box, None, 1, 0.3 * rnb, degrees, solid=solid)
    shells = eng.bond_order_shells(None, 1, rnb, degrees)
    for which in ("wide", "narrow"):
        eng.set_neighbor_skin(c["skin"] if which == "wide" else 0.0)
        got = device(eng, pos, None, 1, rnb, degrees, solid=solid, shells=shells)
        info = eng.info()
        assert (info["ncell_x"], info["ncell_y"], info["ncell_z"]) == c["cells_" + which][:3]
        assert_matches(got, ref, box, degrees, (name, which))
    assert_matches(device(eng, pos, None, 1, 0.3 * rnb, degrees, solid=solid), short, box, degrees, (name, "short"))
    shells.close()
    eng.close()


# -- the histogram -------------------------------------------------------------------------------------------------------------------

def test_histogram_of_the_devices_own_q():
    import torch
    box = CUBIC
    eng = engine(box)
    pos, types = points(box), types_of(NMAX, 3)
    degrees = (4, 6)
    shells = eng.bond_order_shells(types, 3, 3.0, degrees)
    q = torch.zeros((NMAX, 2), dtype=torch.float64, device="cuda")
    eng.bond_order(to4(pos), shells, q=q)
    host = q.cpu().numpy()
    for l, col, nbins, lo, hi in ((4, 0, 100, 0.0, 1.0), (6, 1, 37, 0.1, 0.45), (6, 1, 1, 0.0, 1.0), (4, 0, 2730, 0.0, 0.5)):
        counts = torch.zeros((3, nbins), dtype=torch.int64, device="cuda")
        want = br.histogram(host[:, col], types, 3, nbins, lo, hi)
        assert want.sum() > 100
        assert eng.bond_order_histogram(q, shells, l, counts, lo, hi) is counts
        assert np.array_equal(counts.cpu().numpy(), want), (l, nbins)
        eng.bond_order_histogram(q, shells, l, counts, lo, hi)
        assert np.array_equal(counts.cpu().numpy(), 2 * want), (l, nbins, "accumulated")
    members = np.arange(0, NMAX, 3)
    counts = torch.zeros((3, 50), dtype=torch.int64, device="cuda")
    eng.bond_order_histogram(q, shells, 6, counts, group=torch.tensor(members, dtype=torch.int32, device="cuda"))
    assert np.array_equal(counts.cpu().numpy(), br.histogram(host[members, 1], types[members], 3, 50, 0.0, 1.0))
    # planted values: lo is counted, just below hi lands in the last bin, hi and NaN are not counted
    planted = np.array([0.0, np.nextafter(1.0, 0.0), 1.0, np.nan, -1e-300, 0.5, np.inf, 0.25])
    vals = torch.zeros((NMAX, 2), dtype=torch.float64, device="cuda")
    vals[:, 0] = 2.0
    vals[:8, 0] = torch.tensor(planted, dtype=torch.float64)
    counts = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    eng.bond_order_histogram(vals, shells, 4, counts)
    want = br.histogram(planted, types[:8], 3, 4, 0.0, 1.0)
    assert want.sum() == 4 and want[:, 0].sum() == 1 and want[:, 3].sum() == 1
    assert np.array_equal(counts.cpu().numpy(), want)
    with pytest.raises(ValueError, match="counts must be"):
        eng.bond_order_histogram(q, shells, 4, torch.zeros((2, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="more than 8192"):
        eng.bond_order_histogram(q, shells, 4, torch.zeros((3, 2731), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="must exceed"):
        eng.bond_order_histogram(q, shells, 4, counts, 1.0, 1.0)
    shells.close()


# -- the raw C-ABI -------------------------------------------------------------------------------------------------------------------

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

    n, box = 300, CUBIC
    pos = points(box, n)
    types = types_of(n, 2).astype(np.uint32)
    rnb, deg = np.array([3.0, 2.6, 3.2]), np.array([4, 6], dtype=np.int32)
    rc, h = create(box[0], n)
    assert rc == 0, msg()
    rc, h2 = create(box[0], n)
    assert rc == 0, msg()
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()

    def shells_on(hh, expect=0, word=None, ty=types, ntypes=2, r=rnb, nn=n, nl=2, d=deg):
        b = ctypes.c_void_p(777)
        rc = lib.pse_bond_order_create(hh, nn, None if ty is None else vp(ty), ntypes, None if r is None else vp(r), nl,
                                       None if d is None else vp(d), ctypes.byref(b))
        assert rc == expect, msg()
        assert expect == 0 or (word in msg() and "pse_bond_order_create" in msg() and not b.value), (word, msg())
        return b

    b = shells_on(h)
    shells_on(h, INVALID, "ntypes = 9", ntypes=9)
    shells_on(h, INVALID, "null rnb_host", r=None)
    shells_on(h, INVALID, "rcut", r=np.array([1.5, 5.3, 1.0]))
    shells_on(h, INVALID, "every pair type is off", r=np.zeros(3))
    shells_on(h, INVALID, "n_max", nn=n + 1)
    shells_on(h, INVALID, "nl = 5", nl=5)
    shells_on(h, INVALID, "null degrees_host", d=None)
    shells_on(h, INVALID, "degree 1 = 7", d=np.array([4, 7], dtype=np.int32))
    shells_on(h, INVALID, "listed twice", d=np.array([4, 4], dtype=np.int32))
    shells_on(None, INVALID, "null handle")
    bs = shells_on(hs)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex2 = ctypes.c_void_p()
    assert lib.pse_exclusions_create(h2, n, 1, vp(pairs), ctypes.byref(ex2)) == 0, msg()
    dpos = to4(pos)
    nnb = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    nconn = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    q = torch.full((n, 2), float(SENTINEL), dtype=torch.float64, device="cuda")
    qbar = torch.full((n, 2), float(SENTINEL), dtype=torch.float64, device="cuda")
    stats = torch.full((2, 2), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((2, 10), SENTINEL, dtype=torch.int64, device="cuda")
    call = lib.pse_bond_order_compute

    def refused(word, bb=b, p=P(dpos), nn=n, a=P(nnb), qq=P(q), qb=P(qbar), sd=1, thr=0.3, nc=P(nconn), st=P(stats), e=None):
        assert call(bb, p, None, nn, a, qq, qb, sd, thr, 3, nc, st, e) == INVALID, word
        assert word in msg() and "pse_bond_order_compute" in msg(), (word, msg())

    refused("null bond-order object", bb=None)
    refused("n_max", nn=0)
    refused("n_max", nn=n + 1)
    refused("null pos", p=None)
    refused("all null", a=None, qq=None, qb=None, nc=None, st=None)
    refused("solid_degree = 2", sd=2)
    refused("threshold = 2", thr=2.0)
    refused("stats is not 8-byte aligned", st=ctypes.c_void_p(stats.data_ptr() + 4))
    refused("another handle", e=ex2)
    refused("slab rank", bb=bs)
    hcall = lib.pse_bond_order_histogram

    def hrefused(word, bb=b, v=P(q), col=1, nn=n, nbins=10, lo=0.0, hi=1.0, c=P(counts)):
        assert hcall(bb, v, col, None, nn, nbins, lo, hi, c) == INVALID, word
        assert word in msg() and "pse_bond_order_histogram" in msg(), (word, msg())

    hrefused("null bond-order object", bb=None)
    hrefused("null values", v=None)
    hrefused("column = 2", col=2)
    hrefused("nbins = 0", nbins=0)
    hrefused("4097 bins", nbins=4097)
    hrefused("must exceed", hi=0.0)
    hrefused("null counts", c=None)
    hrefused("counts is not 8-byte aligned", c=ctypes.c_void_p(counts.data_ptr() + 4))
    torch.cuda.synchronize()
    for t in (nnb, nconn, q, qbar, stats, counts):
        assert np.all(t.cpu().numpy() == SENTINEL)                                             # nothing was launched, nothing was written
    assert call(b, P(dpos), None, n, P(nnb), P(q), P(qbar), 1, 0.3, 3, P(nconn), P(stats), None) == 0, msg()
    ref = reference(pos, box, types, 2, rnb, (4, 6), solid=(6, 0.3, 3))
    got = {k: t.cpu().numpy() for k, t in (("nnb", nnb), ("q", q), ("qbar", qbar), ("nconn", nconn), ("stats", stats))}
    assert_matches(got, ref, box, (4, 6), "raw")
    counts.zero_()
    assert hcall(b, P(q), 1, None, n, 10, 0.0, 1.0, P(counts)) == 0, msg()
    assert np.array_equal(counts.cpu().numpy(), br.histogram(got["q"][:, 1], types, 2, 10, 0.0, 1.0))
    assert lib.pse_bond_order_destroy(b) == 0
    assert lib.pse_bond_order_destroy(None) == 0
    b = shells_on(h)                                                                           # still alive below: it goes with its handle
    for hh in (h, h2, hs):
        assert lib.pse_destroy(hh) == 0


# -- a captured graph ----------------------------------------------------------------------------------------------------------------

def test_captured_graph_replayed_twice():
    import pse_amd
    import torch
    box = TILTED
    frames = [points(box, 300), points(box)[213:]]
    degrees, solid = (4, 6), (6, 0.3, 3)
    eng = pse_amd.Engine(300, box, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    shells = eng.bond_order_shells(None, 1, 3.0, degrees)
    pos = to4(frames[0])
    nnb = torch.full((300,), SENTINEL, dtype=torch.int32, device="cuda")
    nconn = torch.full((300,), SENTINEL, dtype=torch.int32, device="cuda")
    q = torch.zeros((300, 2), dtype=torch.float64, device="cuda")
    qbar = torch.zeros((300, 2), dtype=torch.float64, device="cuda")
    stats = torch.full((1, 2), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.zeros((1, 100), dtype=torch.int64, device="cuda")
    outs = (nnb, nconn, q, qbar, stats)

    def sample():
        eng.bond_order(pos, shells, nnb=nnb, q=q, qbar=qbar, solid=solid, nconn=nconn, stats=stats)
        eng.bond_order_histogram(q, shells, 6, counts)

    eager = []
    for p in frames:                                                                           # the eager calls, also the warm-up
        pos.copy_(to4(p))
        counts.zero_()
        with torch.cuda.stream(st):
            sample()
        st.synchronize()
        eager.append([t.cpu().numpy().copy() for t in outs + (counts,)])
    assert not np.array_equal(eager[0][0], eager[1][0])
    ref = reference(frames[0], box, None, 1, 3.0, degrees, solid=solid)
    assert np.array_equal(eager[0][0], ref["nnb"]) and np.array_equal(eager[0][1], ref["nconn"])
    for t in outs:
        t.fill_(SENTINEL)
    counts.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        sample()
    torch.cuda.synchronize()
    assert not counts.cpu().numpy().any() and (nnb.cpu().numpy() == SENTINEL).all(), "a capture runs nothing"
    total = np.zeros((1, 100), dtype=np.int64)
    for k, p in enumerate(frames):
        pos.copy_(to4(p))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        total += eager[k][5]
        for t, want in zip(outs, eager[k][:5]):
            assert np.array_equal(t.cpu().numpy(), want), ("replay", k)                        # the eager call's bits
        assert np.array_equal(counts.cpu().numpy(), total)
    shells.close()
    eng.close()


# -- analyze.BondOrder ---------------------------------------------------------------------------------------------------------------

@pytest.fixture
def restored_context():
    """A System registers itself as the current simulation context: put back what was there."""
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


def test_bond_order_through_system_run(restored_context):
    """The fcc crystal at rest (T = 0, no forces: zero velocities) over three samples: the histogram mass is 3 N in the fcc bins, the
    table has three rows, all solid-like, and reset() clears it."""
    from pse_amd import analyze, integrate
    from pse_amd.system import System
    pos = br.fcc_lattice(3, 4.0)
    n = len(pos)
    s = System(pos, FCC_BOX, dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3)
    bo = analyze.BondOrder(pse, FCC_RNB, degrees=(4, 6), solid=(6, 0.7, 7), nbins=100, capacity=8)
    assert s.analyzers == [bo] and bo.samples == 0
    for reader in (lambda: bo.q(6), bo.neighbors, bo.solid_like, lambda: bo.histogram(6), bo.solid_fraction):
        with pytest.raises(ValueError, match="no samples"):
            reader()
    s.run(3)
    assert bo.samples == 3
    tol = br.bound(6, 12, br.separation_error(FCC_BOX, 2.8)) + 1e-12
    assert np.abs(bo.q(6) - CLOSED["fcc"][6]).max() <= tol and np.abs(bo.qbar(6) - CLOSED["fcc"][6]).max() <= 2 * tol
    assert np.abs(bo.q(4) - CLOSED["fcc"][4]).max() <= tol
    assert (bo.neighbors() == 12).all() and (bo.connections() == 12).all() and bo.solid_like().all()
    for averaged in (False, True):
        h6, h4 = bo.histogram(6, averaged=averaged), bo.histogram(4, averaged=averaged)
        assert h6.sum() == 3 * n and h6[57] == 3 * n and h4[19] == 3 * n                         # q_6 = 0.5745, q_4 = 0.1909
        assert abs(bo.mean(6, averaged=averaged) - 0.575 * analyze.BOND_ORDER_HI) < 1e-12            # the centre of bin 57 of the analyzer's bins
    assert bo.table().tolist() == [[t, n, n] for t in range(3)] and bo.solid_fraction() == 1.0
    with pytest.raises(ValueError, match="degree 8"):
        bo.q(8)
    bo.reset()
    assert bo.samples == 0 and len(bo.table()) == 0
    with pytest.raises(ValueError, match="no samples"):
        bo.histogram(6)
    s.run(1)
    assert bo.samples == 1 and bo.table().tolist() == [[3, n, n]] and bo.histogram(6).sum() == n
    plain = analyze.BondOrder(pse, FCC_RNB, degrees=(6,), period=2)
    s.run(2)                                                                                   # steps 4 and 5: one sample of the second
    assert plain.samples == 1 and plain.table().tolist() == [[4, n, 0]]
    with pytest.raises(ValueError, match="no solid-bond pass"):
        plain.solid_like()
    with pytest.raises(RuntimeError, match="rcut"):
        analyze.BondOrder(pse, 5.3)


def test_analyzer_counts_every_member_of_a_dilute_system(restored_context):
    """Where particles have ONE neighbour q_l = q-bar_l = 1 up to rounding, at or above 1 as often as below: the histogram mass must
    still be samples x members.  Twelve isolated pairs (six along the axes), 64 random points of which many have no or one
    neighbour, and a group that leaves some out; three samples at rest."""
    from pse_amd import analyze, integrate
    from pse_amd.system import Group, System
    box = (40.0, 40.0, 40.0, 0.0)
    rng = np.random.default_rng(17)
    centres = np.stack(np.meshgrid(*[np.array([-15.0, -5.0, 5.0])] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:12]
    steps = 1.5 * np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=float)
    u = rng.normal(size=(6, 3))
    steps = np.concatenate([steps, 1.5 * u / np.linalg.norm(u, axis=1)[:, None]])
    cloud = rng.uniform(8.0, 19.0, size=(64, 3))                                                # dilute, away from the pairs
    pos = np.concatenate([centres, centres + steps, cloud])
    n = len(pos)
    types = rng.integers(0, 2, n)
    members = np.setdiff1d(np.arange(n), [3, 30, 50])                                           # (pair 3 loses a partner: no neighbour left)
    degrees = (4, 6, 12)
    ref = reference(pos[members], box, types[members], 2, 2.5, degrees, ids=members)
    ones = int((ref["nnb"] == 1).sum())
    assert ones >= 22 and (ref["nnb"] == 0).sum() >= 5 and (ref["nnb"] > 1).sum() >= 5
    s = System(pos, box, dt=1e-3)
    pse = integrate.PSEv1(group=Group(s, members), T=0.0, seed=3, xi=0.5, error=1e-3)
    bo = analyze.BondOrder(pse, 2.5, degrees=degrees, types=types, nbins=50)
    s.run(3)
    assert bo.samples == 3 and np.array_equal(bo.neighbors()[members], ref["nnb"])
    per_type = np.bincount(types[members], minlength=2)
    for l in degrees:
        col = degrees.index(l)
        q = bo.q(l)[members]
        print(f"l = {l}: {int((q[ref['nnb'] == 1] >= 1.0).sum())} of {ones} single-neighbour q at or above 1")
        assert np.abs(q[ref["nnb"] == 1] - 1.0).max() <= br.bound(l, 1, br.separation_error(box, ref["rmin"]))
        for averaged in (False, True):
            values = (bo.qbar(l) if averaged else bo.q(l))[members]
            for a in (0, 1):
                h = bo.histogram(l, a, averaged)
                assert h.sum() == 3 * per_type[a], (l, a, averaged, int(h.sum()))               # nobody is dropped
                want = br.histogram(values[types[members] == a], np.zeros(per_type[a], dtype=int), 1, 50, 0.0, analyze.BOND_ORDER_HI)[0]
                assert np.array_equal(h, 3 * want), (l, a, averaged)
            assert bo.histogram(l, None, averaged).sum() == 3 * len(members)
            assert averaged or bo.histogram(l)[49] >= 3 * ones              # q = 1, whichever way it rounds, is in the last bin (q-bar = 1
                                                                            # only where the one neighbour has no other)
            assert abs(bo.mean(l, None, averaged) - values.mean()) <= 0.5 * analyze.BOND_ORDER_HI / 50
        assert np.abs(bo.q(l)[members] - ref["q"][:, col]).max() <= br.bound(l, ref["nbmax"], br.separation_error(box, ref["rmin"]))
    assert bo.table().tolist() == [[t, per_type[0], 0, per_type[1], 0] for t in range(3)]
