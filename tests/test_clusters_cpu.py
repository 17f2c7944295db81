"""CPU tests of the cluster analysis that need no device: the O(N^2) reference the GPU tests compare to (tests/cluster_ref.py)
against scipy's connected_components on the seeded inputs of the GPU tests, against hand-built cases and against the invariants of a
labelling; the pure functions of analyze.Clusters against brute force; the three forms of `rlink`; the refusals of the four entry
points through the device stand-in of the sanitizer build (pse_amd/csrc/asan_stub.cpp, which runs the real validators), built here
without a sanitizer; and the argument checks of analyze.Clusters that come before the device is touched."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as cr
from pair_table_ref import random_points
from test_pair_hist_cpu import stub_handle, _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
RCUT = 5.2565                                   # just below sqrt(-ln 1e-3) / 0.5 = 5.25652...
RCUT_EXACT = math.sqrt(-math.log(1e-3)) / 0.5   # the engine's cutoff at xi = 0.5, error = 1e-3
# rlink: (clusters, largest, singletons) at n = 513, cubic / tilted
REGIMES = {1.0: ((320, 7, 211), (321, 7, 214)), 1.5: ((76, 209, 33), (61, 381, 34)), 1.8: ((10, 501, 6), (7, 506, 5)),
           3.0: ((1, 513, 0), (1, 513, 0)), RCUT_EXACT: ((1, 513, 0), (1, 513, 0))}


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def union_find(n, i, j):
    """Ten lines that owe nothing to cluster_ref: the component of every row as the smallest row in it."""
    lab = np.arange(n)
    changed = True
    while changed:
        changed = False
        for a, b in zip(i.tolist(), j.tolist()):
            m = min(lab[a], lab[b])
            if lab[a] != m or lab[b] != m:
                lab[a] = lab[b] = m
                changed = True
    return lab


# ---- the reference ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("rlink", sorted(REGIMES))
def test_regimes_of_the_seeded_points(rlink, box, oracle):
    """The regimes the GPU tests rely on: many small clusters, the threshold, one giant cluster with a few singletons, one cluster.
    The smallest clearance of these inputs is 1.76e-5 (rlink = rcut in the tilted box; 6.0e-5 and more below rcut)."""
    pos = random_points(513, box, seed=11)
    label, size, stats, hist, clear = cr.clusters(pos, box, None, 1, rlink, oracle)
    print(f"rlink = {rlink}: clearance {clear:.3e}, stats {stats.tolist()}, singletons {hist[0]}")
    cr.assert_clear(clear)
    assert clear >= 1.7e-5
    assert (int(stats[0]), int(stats[1]), int(hist[0])) == REGIMES[rlink][box is TILTED]
    assert stats[3] == 513 and hist.sum() == stats[0] and (hist * np.arange(1, 514)).sum() == 513
    (i, j), _ = cr.links(pos, box, None, 1, rlink, oracle)
    assert np.array_equal(label, union_find(513, i, j))


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 300, 513])
def test_reference_agrees_with_scipy(n, box, oracle):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    pos = random_points(513, box, seed=11)[:n]
    types = np.random.default_rng(21).integers(0, 2, n)
    for ntypes, ty, rlink in ((1, None, 1.0), (1, None, 1.5), (1, None, 1.8), (2, types, {(0, 0): 1.8, (0, 1): 1.2}), (2, types, {(1, 0): 2.0})):
        (i, j), clear = cr.links(pos, box, ty, ntypes, rlink, oracle)
        cr.assert_clear(clear)
        label, size, stats, hist = cr.outputs(cr.components(n, i, j))
        graph = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n))
        ncomp, comp = connected_components(graph, directed=False)
        assert ncomp == stats[0]
        least = np.full(ncomp, n)
        np.minimum.at(least, comp, np.arange(n))
        assert np.array_equal(label, least[comp]) and np.array_equal(size, np.bincount(comp)[comp])
        assert np.array_equal(label, union_find(n, i, j))


def test_hand_built_cases(oracle):
    box = (10.0, 10.0, 10.0, 0.0)
    # a dimer and a loner
    pos = np.array([[0.0, 0.0, 0.0], [1.2, 0.0, 0.0], [4.0, 4.0, 4.0]])
    label, size, stats, hist, clear = cr.clusters(pos, box, None, 1, 1.5, oracle)
    assert label.tolist() == [0, 0, 2] and size.tolist() == [2, 2, 1] and stats.tolist() == [2, 2, 5, 3] and hist.tolist() == [1, 1, 0]
    assert abs(clear - 0.3) < 1e-12
    label, size, stats, hist, _ = cr.clusters(pos, box, None, 1, 1.1, oracle)
    assert label.tolist() == [0, 1, 2] and stats.tolist() == [3, 1, 3, 3] and hist.tolist() == [3, 0, 0]
    # a chain through the periodic face in x: 4.0, 4.9, -4.2 (= 5.8), -3.3, and a loner; fed in an order that is not the chain's
    pos = np.array([[-3.3, 0.0, 0.0], [0.0, 3.0, 0.0], [4.9, 0.0, 0.0], [4.0, 0.0, 0.0], [-4.2, 0.0, 0.0]])
    label, size, stats, hist, _ = cr.clusters(pos, box, None, 1, 1.0, oracle)
    assert label.tolist() == [0, 1, 0, 0, 0] and size.tolist() == [4, 1, 4, 4, 4] and stats.tolist() == [2, 4, 17, 5]
    # caller indices: the label is the smallest id, not the smallest row
    label, *_ = cr.clusters(pos, box, None, 1, 1.0, oracle, ids=[9, 3, 7, 8, 4])
    assert label.tolist() == [4, 3, 4, 4, 4]
    # two triangles joined by one particle between them; without it (rows 0-5) they are two clusters
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.8, 0.0]])
    pos = np.concatenate([tri, tri + [2.6, 0.0, 0.0], [[1.8, 0.0, 0.0]]])
    label, size, stats, _, _ = cr.clusters(pos[:6], box, None, 1, 1.1, oracle)
    assert label.tolist() == [0, 0, 0, 3, 3, 3] and stats.tolist() == [2, 3, 18, 6]
    label, size, stats, hist, _ = cr.clusters(pos, box, None, 1, 1.1, oracle, nhist=5)
    assert label.tolist() == [0] * 7 and size.tolist() == [7] * 7 and stats.tolist() == [1, 7, 49, 7] and hist.tolist() == [0, 0, 0, 0, 1]
    # types: with only the A-B links on, the bridge (type B) and the two corners it reaches, rows 1 and 3 at 0.8, are one cluster
    # and nothing else is linked; with only A-A on, the bridge is alone
    types = np.array([0, 0, 0, 0, 0, 0, 1])
    label, *_ = cr.clusters(pos, box, types, 2, {(0, 1): 1.1}, oracle)
    assert label.tolist() == [0, 1, 2, 1, 4, 5, 1]
    label, *_ = cr.clusters(pos, box, types, 2, {(0, 0): 1.1}, oracle)
    assert label.tolist() == [0, 0, 0, 3, 3, 3, 6]
    # an excluded pair is no link
    label, *_ = cr.clusters(pos[:3], box, None, 1, 1.1, oracle, excl=np.array([[0, 1], [0, 2], [1, 2]]))
    assert label.tolist() == [0, 1, 2]


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
def test_label_and_size_invariants(box, oracle):
    pos = random_points(513, box, seed=11)
    types = np.random.default_rng(21).integers(0, 3, 513)
    for rlink in (1.0, 1.5, [1.5, 0.0, 1.2, 1.8, 0.0, 2.0]):
        label, size, stats, hist, clear = cr.clusters(pos, box, types, 3, rlink, oracle, nhist=5)
        cr.assert_clear(clear)
        assert np.array_equal(label[label], label) and (label <= np.arange(513)).all()
        assert np.array_equal(size, np.bincount(label)[label])
        roots = np.unique(label)
        assert size[roots].sum() == 513 == stats[3] and len(roots) == stats[0] and size.max() == stats[1] and (size[roots] ** 2).sum() == stats[2]
        assert hist.tolist() == [int((size[roots] == s).sum()) for s in (1, 2, 3, 4)] + [int((size[roots] >= 5).sum())]
    # a permuted order: the same partition, labels the permuted minima
    perm = np.random.default_rng(8).permutation(513)
    a = cr.clusters(pos, box, types, 3, 1.5, oracle)[0]
    b = cr.clusters(pos[perm], box, types[perm], 3, 1.5, oracle, ids=perm)[0]
    assert np.array_equal(b, a[perm])


# ---- the pure functions of analyze.Clusters ----------------------------------------------------------------------------------------

def test_analyzer_functions_against_brute_force():
    from pse_amd import analyze
    rng = np.random.default_rng(5)
    samples = [rng.integers(1, 9, size=rng.integers(3, 12)) for _ in range(6)]          # the cluster sizes of six samples
    nhist = 6
    hist = np.zeros(nhist, dtype=np.int64)
    rows = []
    for s in samples:
        for v in s:
            hist[min(v, nhist) - 1] += 1
        rows.append([len(s), s.max(), (s ** 2).sum(), s.sum()])
    ns = analyze.size_distribution_of(hist, len(samples))
    want = [np.mean([(np.minimum(s, nhist) == k).sum() for s in samples]) for k in range(1, nhist + 1)]
    assert np.allclose(ns, want, rtol=0, atol=1e-15) and abs(ns.sum() - np.mean([len(s) for s in samples])) < 1e-14
    num, wgt, frac = analyze.averages_of(rows)
    allsizes = np.concatenate(samples).astype(float)
    assert abs(num - allsizes.mean()) < 1e-14 and abs(wgt - (allsizes ** 2).sum() / allsizes.sum()) < 1e-14
    assert abs(frac - np.mean([s.max() / s.sum() for s in samples])) < 1e-15 and wgt >= num
    assert analyze.averages_of([[4, 1, 4, 4]]) == (1.0, 1.0, 0.25) and analyze.averages_of([[1, 4, 16, 4]]) == (4.0, 4.0, 1.0)
    for f, arg in ((analyze.size_distribution_of, (hist, 0)), (analyze.averages_of, (np.zeros((0, 4)),))):
        with pytest.raises(ValueError, match="no samples"):
            f(*arg)


def test_the_three_forms_of_rlink():
    from pse_amd import engine
    from pse_amd.engine import pair_type_index
    ty, nt, rl = engine._cluster_arguments(None, 1, 1.5)
    assert ty is None and nt == 1 and rl.tolist() == [1.5] and rl.dtype == np.float64
    _, _, rl = engine._cluster_arguments([0, 2, 1], 3, 2.0)
    assert rl.tolist() == [2.0] * 6
    _, _, rl = engine._cluster_arguments([0, 2, 1], 3, {(2, 0): 1.5, (1, 1): 2.5})       # either key order; a missing pair is off
    want = np.zeros(6)
    want[pair_type_index(0, 2, 3)], want[pair_type_index(1, 1, 3)] = 1.5, 2.5
    assert rl.tolist() == want.tolist() and rl.tolist() == cr.rlink_array({(2, 0): 1.5, (1, 1): 2.5}, 3).tolist()
    ty, _, rl = engine._cluster_arguments(np.array([0, 1]), 2, [1.0, 0.0, 2.0])
    assert rl.tolist() == [1.0, 0.0, 2.0] and ty.dtype == np.uint32
    for word, args in (("outside [1, 8]", (None, 9, 1.0)), ("type 2 >= ntypes = 2", ([0, 2], 2, 1.0)), ("3 entries", ([0, 1], 2, [1.0, 2.0])),
                       ("finite", (None, 1, float("nan"))), ("finite", (None, 1, float("inf"))), ("not negative", (None, 1, -1.0)),
                       ("every pair type is off", (None, 1, 0.0)), ("every pair type is off", ([0, 1], 2, {})),
                       ("twice", ([0, 1], 2, {(0, 1): 1.0, (1, 0): 1.0})), ("rlink key", ([0, 1], 2, {(0, 2): 1.0})),
                       ("rlink key", ([0, 1], 2, {0: 1.0})), ("non-negative", ([0, -1], 2, 1.0))):
        with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
            engine.ClusterLinks(_NoDevice(), *args)


def test_cluster_analyzer_argument_checks_come_before_the_device():
    from pse_amd import analyze
    named = ["A", "B", "B", "A"]
    for word, kw in (("every pair type is off", dict(rlink=0.0)), ("period", dict(rlink=1.0, period=0)), ("nhist", dict(rlink=1.0, nhist=0)),
                     ("capacity", dict(rlink=1.0, capacity=0)), ("type_names", dict(rlink=1.0, types=named)),
                     ("unknown type name 'C'", dict(rlink={("A", "C"): 1.0}, types=named, type_names=["A", "B"])),
                     ("twice", dict(rlink={("A", "B"): 1.0, ("B", "A"): 2.0}, types=named, type_names=["A", "B"])),
                     ("a pair", dict(rlink={"A": 1.0}, types=named, type_names=["A", "B"])), ("finite", dict(rlink=float("nan")))):
        with pytest.raises(ValueError, match=word):
            analyze.Clusters(_NoDevice(), **kw)
    ty, nt, rl, names, period, nhist, cap = analyze._cluster_analyzer_arguments({("B", "A"): 1.5}, named, ["A", "B"], 3, None, 16)
    assert ty.tolist() == [0, 1, 1, 0] and nt == 2 and rl.tolist() == [0.0, 1.5, 0.0] and (names, period, nhist, cap) == (["A", "B"], 3, None, 16)


# ---- the four entry points on the device stand-in ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """The host side of the library over the device stand-in of the sanitizer build, here without a sanitizer, as
    tests/test_pair_hist_cpu.py builds it."""
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_get_info", "pse_last_error", "pse_clusters_create", "pse_clusters_destroy",
                 "pse_clusters_label", "pse_clusters_status", "pse_exclusions_create"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


def test_refusals_of_the_four_entry_points_on_the_stand_in(stub):
    from pse_amd import _lib
    n = 6
    h = stub_handle(stub, n)
    info = _lib.pse_info()
    assert stub.pse_get_info(h, ctypes.byref(info)) == 0
    rcut = info.as_dict()["rcut"]
    assert RCUT < rcut < RCUT + 1e-4
    good = dict(n=n, types=np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32), ntypes=2, rlink=np.array([1.5, 0.0, rcut]))

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_clusters_create(hh, a["n"], vp(a["types"]), a["ntypes"], vp(a["rlink"]), ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_clusters_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    refused("null out", with_out=False)
    refused("null handle", hh=None)
    refused("n = 0", n=0)
    refused("n = 7", n=7)
    refused("n = 7", n=7, types=None)
    refused("ntypes = 0", ntypes=0)
    refused("ntypes = 9", ntypes=9)
    refused("null rlink_host", rlink=None)
    refused("not finite", rlink=np.array([1.5, np.nan, 1.0]))
    refused("not finite", rlink=np.array([np.inf, 0.0, 1.0]))
    refused("negative", rlink=np.array([1.5, 0.0, -1.0]))
    refused("pair type 2 has rlink", rlink=np.array([1.5, 0.0, rcut * (1.0 + 1e-12)]))
    refused("hydrodynamic cutoff", rlink=np.array([6.0, 0.0, 0.0]))
    refused("every pair type is off", rlink=np.zeros(3))
    refused("type 2", types=np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32))
    refused("type 1", ntypes=1, rlink=np.array([1.0]))
    made = []
    for kw in (dict(), dict(types=None, ntypes=1, rlink=np.array([rcut])), dict(ntypes=8, rlink=np.full(36, 1.0)),
               dict(rlink=np.array([0.0, 1e-300, 0.0]))):
        rc, g = create(**kw)
        assert rc == 0 and g.value, (kw, stub.pse_last_error())
        made.append(g)
    g = made[0]

    # the call.  Any non-null, 8-byte aligned address will do for the arrays: the stand-in reads none of them
    other = stub_handle(stub, n)
    slab = stub_handle(stub, n, L=40.0, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    rc, gslab = create(hh=slab)
    assert rc == 0, stub.pse_last_error()
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex, ex_other = ctypes.c_void_p(), ctypes.c_void_p()
    assert stub.pse_exclusions_create(h, n, 1, vp(pairs), ctypes.byref(ex)) == 0
    assert stub.pse_exclusions_create(other, n, 1, vp(pairs), ctypes.byref(ex_other)) == 0
    buf = np.zeros(8)
    X, odd = vp(buf), ctypes.c_void_p(buf.ctypes.data + 4)

    def call(word, gg=g, pos=X, N=n, label=X, size=X, stats=X, hist=X, nhist=4, e=None):
        rc = stub.pse_clusters_label(gg, pos, None, N, label, size, stats, hist, nhist, e)
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg and "pse_clusters_label" in msg), (word, rc, msg)

    call("null cluster object", gg=None)
    call("N = 0", N=0)
    call("N = 7", N=n + 1)
    call("null pos", pos=None)
    call("all null", label=None, size=None, stats=None, hist=None)
    call("stats is not 8-byte aligned", stats=odd)
    call("hist is not 8-byte aligned", hist=odd)
    call("nhist = 0", nhist=0)
    call("another handle", e=ex_other)
    call("slab rank", gg=gslab)
    call("null pos", gg=gslab, pos=None)                                       # the order: pos before the slab rank
    call("N = 7", N=n + 1, pos=None, label=None, size=None, stats=None, hist=None)
    call(None, e=ex)
    call(None)
    call(None, N=1)
    call(None, hist=None, nhist=0)                                             # nhist means nothing without hist
    for only in ("label", "size", "stats", "hist"):                            # each output alone will do
        call(None, **{k: None for k in ("label", "size", "stats", "hist") if k != only})
    word = ctypes.c_uint(77)
    assert stub.pse_clusters_status(g, ctypes.byref(word)) == 0 and word.value == 0
    assert stub.pse_clusters_status(None, ctypes.byref(word)) == INVALID and "null cluster object" in stub.pse_last_error().decode()
    assert stub.pse_clusters_status(g, None) == INVALID and "null status" in stub.pse_last_error().decode()
    for g in made[1:]:
        assert stub.pse_clusters_destroy(g) == 0
    assert stub.pse_clusters_destroy(None) == 0
    for hh in (h, other, slab):                                                # the objects still alive go with their handles
        assert stub.pse_destroy(hh) == 0
