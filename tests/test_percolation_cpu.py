"""CPU tests of the cluster analysis with percolation that need no device: the reference the GPU tests compare to
(tests/percolation_ref.py) against closed forms, against its own invariances (caller order, rigid translation through the walls) and
against the sequential union-find with offsets restated here; the margins of every input of tests/test_gpu_percolation.py and the
regime its random inputs must contain (the seed is picked HERE); pack and unpack of the 64-bit word; the refusals of pse_clusters_span
on the device stand-in of the sanitizer build, built here without a sanitizer; and the NumPy helpers and argument checks of the
Python layer."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as cr
import percolation_ref as pr
from pse_amd.analyze import unfold_clusters          # the product's unfolding: every shape below is made whole by it
from pair_table_ref import random_points
from test_pair_hist_cpu import stub_handle, _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
BOXES = pytest.mark.parametrize("box", [pr.CUBIC, pr.TILTED], ids=["cubic", "tilted"])
UP, DOWN = 1.75 * (1.0 + 1e-6), 1.75 * (1.0 - 1e-6)
START = (0.3, -1.1, 2.2)


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------

@BOXES
def test_rods_through_each_lattice_axis(box, oracle):
    for k, direction in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        pos = pr.rod(box, direction, START)
        ref = pr.span(pos, box, None, 1, UP, oracle)
        cr.assert_clear(ref["clear"])
        n = len(pos)
        assert (ref["span"] == 1 << k).all() and ref["stats"].tolist() == [1, n, n * n, n], (k, ref["span"])
        assert not ref["image"].any() and (ref["rg2"] == -1.0).all() and np.array_equal(unfold_clusters(pos, ref["image"], box), pos)
        assert ref["pstats"].tolist() == [1, n] + [int(a == k) for a in range(3)] + [0, 0, 0]
    pos = pr.rod(pr.CUBIC, (1, 0, 0), START)
    assert len(pos) == 8
    ref = pr.span(pos, pr.CUBIC, None, 1, DOWN, oracle)                            # 1e-6 short: eight singletons, nothing spans
    assert not ref["span"].any() and ref["stats"].tolist() == [8, 1, 8, 8] and not ref["rg2"].any()
    assert ref["pstats"].tolist() == [0, 0, 0, 0, 0, 0, 1, 8]


def test_diagonal_rods_helices_and_the_c_shape(oracle):
    box = pr.CUBIC
    assert (pr.span(pr.rod(box, (1, 1, 0), START), box, None, 1, UP, oracle)["span"] == 3).all()
    assert (pr.span(pr.rod(box, (1, 1, 1), START), box, None, 1, UP, oracle)["span"] == 7).all()
    ref = pr.span(pr.double_helix(box), box, None, 1, UP, oracle)
    assert (ref["span"] == 1).all() and ref["stats"][0] == 1
    i, j = ref["links"]
    assert len(i) == 20 and abs(ref["shifts"][:, 0]).sum() == 2                    # one ring of 20 links, two of them through the face
    ref = pr.span(pr.six_turn_helix(box, False), box, None, 1, UP, oracle)
    assert not ref["span"].any() and ref["stats"][0] == 1 and sorted(set(ref["image"][:, 0].tolist())) == [0, 1, 2, 3, 4, 5]
    assert not ref["image"][:, 1:].any()
    U = unfold_clusters(pr.six_turn_helix(box, False), ref["image"], box)
    assert np.allclose(np.diff(U[:, 0]), 6.0 * 14.0 / 60, rtol=0, atol=1e-12)       # made whole: x advances evenly over six boxes
    assert (pr.span(pr.six_turn_helix(box, True), box, None, 1, UP, oracle)["span"] == 1).all()
    ref = pr.span(pr.c_shape(box), box, None, 1, 1.2, oracle)
    assert not ref["span"].any() and ref["image"][:, 0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0] and not ref["image"][:, 1:].any()
    U = unfold_clusters(pr.c_shape(box), ref["image"], box)
    rg2 = ((U - U.mean(axis=0)) ** 2).sum() / 10
    assert abs(ref["rg2"][0] - rg2) < 1e-5 and abs(ref["rg2"][0] - ref["rg2_fixed"][0]) <= ref["rg2_bound"][0]   # (q resolves 2^-20)


# ---- caller order and translation ---------------------------------------------------------------------------------------------------

def shapes(pos, ref, box):
    """Per cluster that spans nothing, keyed by its sorted member set: the unfolded members about their mean."""
    U = unfold_clusters(pos, ref["image"], box)
    assert np.abs(U - pr.unfolded(pos, ref["image"], box)).max() < 1e-12
    out = {}
    for root in np.unique(ref["comp"]):
        m = np.nonzero(ref["comp"] == root)[0]
        if not ref["span"][root]:
            out[tuple(m.tolist())] = U[m] - U[m].mean(axis=0)
    return out


@BOXES
def test_caller_order_and_translation_through_the_walls(box, oracle):
    pos = np.concatenate([random_points(257, box, seed=pr.SEED), pr.rod(box, (0, 0, 1), (6.1, 4.9, 0.0), spacing=1.2)])
    n = len(pos)
    base = pr.span(pos, box, None, 1, 1.5, oracle)
    pr.assert_clear(base)
    assert base["pstats"][0] >= 1 and base["pstats"][6] >= 5
    want = shapes(pos, base, box)
    rng = np.random.default_rng(4)
    for trial in range(4):
        perm = rng.permutation(n)
        shift = rng.uniform(-30.0, 30.0, size=3) if trial else np.zeros(3)
        moved = pr.wrap(pos[perm] + shift, box)
        ref = pr.span(moved, box, None, 1, 1.5, oracle)
        assert ref["clear"] >= 1e-10
        assert np.array_equal(ref["span"], base["span"][perm]) and np.array_equal(ref["size"], base["size"][perm])
        assert np.array_equal(ref["pstats"], base["pstats"])
        got = shapes(moved, ref, box)
        back = {tuple(sorted(perm[list(k)].tolist())): (k, v) for k, v in got.items()}
        assert set(back) == set(want)
        for members, (k, v) in back.items():
            order = np.argsort(perm[list(k)])
            assert np.abs(v[order] - want[members]).max() < 1e-9, (trial, members[:3])
        # caller indices: the images are relative to the member with the smallest CALLER index, whatever its row
        ids = rng.permutation(n) + 7
        by_id = pr.span(moved, box, None, 1, 1.5, oracle, ids=ids)
        assert np.array_equal(by_id["span"], ref["span"])
        first = np.array([np.nonzero(by_id["comp"] == c)[0][np.argmin(ids[by_id["comp"] == c])] for c in by_id["comp"]])
        assert np.array_equal(first, by_id["comp"]) and not by_id["image"][np.unique(first)].any()


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------

def test_margins_of_the_gpu_inputs(oracle):
    """Both clearances and the distance from a tie of rint on every seeded and planted input of tests/test_gpu_percolation.py."""
    worst = [np.inf, np.inf, np.inf]
    count = 0
    for name, pos, box, kw in pr.gpu_inputs():
        ref = pr.span(pos, box, kw.get("types"), kw.get("ntypes", 1), kw["rlink"], oracle, excl=kw.get("excl"))
        pr.assert_clear(ref)
        worst = [min(w, ref[k]) for w, k in zip(worst, ("clear", "q_margin", "tie"))]
        count += 1
    print(f"{count} inputs: link clearance {worst[0]:.3e}, q margin {worst[1]:.3e}, tie {worst[2]:.3e}")
    assert count > 120


def test_random_regimes_hold_a_spanning_and_a_finite_cluster_together(oracle):
    """The seed of the random inputs is picked so that, in BOTH boxes, some sample has a spanning cluster and beside it a cluster of ten
    or more that spans nothing; and the regimes run from nothing spanning to everything in one cluster that spans all three axes."""
    for box in (pr.CUBIC, pr.TILTED):
        both, none_span, all_span = 0, 0, 0
        for n, rlink, pos in pr.random_regimes(box):
            ps = pr.span(pos, box, None, 1, rlink, oracle)["pstats"]
            both += ps[0] >= 1 and ps[6] >= 10
            none_span += n == 513 and ps[0] == 0
            all_span += n == 513 and ps[5] == 1 and ps[1] == 513
        assert both >= 1 and none_span >= 1 and all_span >= 1, (box, both, none_span, all_span)


# ---- the sequential algorithm -----------------------------------------------------------------------------------------------------------

def sequential(n, links, shifts, rng):
    """The union-find with offsets of pse_percolation.hip, one link at a time: word[x] = (parent, c_x - c_parent), parent <= x, the
    larger root under the smaller, path halving at random.  Returns (root, c - c_root, flags at the roots)."""
    parent = list(range(n))
    off = [(0, 0, 0)] * n
    flag = [0] * n
    add = lambda a, b: tuple(u + v for u, v in zip(a, b))      # noqa: E731
    sub = lambda a, b: tuple(u - v for u, v in zip(a, b))      # noqa: E731

    def find(x):
        s = (0, 0, 0)
        while parent[x] != x:
            p = parent[x]
            o = off[x]
            if rng.random() < 0.5 and parent[p] != p:          # halve: (grandparent, o_x + o_parent) as one word
                o = add(o, off[p])
                parent[x], off[x] = parent[p], o
                p = parent[p]
            s = add(s, o)
            x = p
        return x, s

    for (i, j), nij in zip(links, shifts):
        A, a = find(i)
        B, b = find(j)
        if A == B:
            m = sub(sub(b, a), nij)
            flag[A] |= sum(1 << k for k in range(3) if m[k])
        elif A > B:
            parent[A], off[A] = B, sub(sub(b, nij), a)
        else:
            parent[B], off[B] = A, sub(add(a, nij), b)
    root, c = [0] * n, [None] * n
    for x in range(n):
        root[x], c[x] = find(x)
    for x in range(n):
        if root[x] != x:
            flag[root[x]] |= flag[x]
    return root, c, flag


@BOXES
def test_sequential_union_find_with_offsets_against_the_reference(box, oracle):
    rng = np.random.default_rng(17)
    inputs = [(random_points(200, box, seed=s), rl) for s, rl in ((1, 1.5), (2, 1.8), (3, 2.2), (4, 3.0))]
    inputs += [(pr.six_turn_helix(box, False), UP), (pr.double_helix(box), UP), (pr.c_shape(box), 1.2)]
    spanning = finite = 0
    for pos, rlink in inputs:
        ref = pr.span(pos, box, None, 1, rlink, oracle)
        n = len(pos)
        links = list(zip(*[a.tolist() for a in ref["links"]]))
        for trial in range(3):
            order = rng.permutation(len(links))
            flip = rng.random(len(links)) < 0.5                                     # either end first: the shift changes sign
            ls = [(links[k][1], links[k][0]) if flip[k] else links[k] for k in order]
            ss = [tuple((-ref["shifts"][k] if flip[k] else ref["shifts"][k]).tolist()) for k in order]
            root, c, flag = sequential(n, ls, ss, rng)
            assert np.array_equal(np.array(root), cr.components(n, *ref["links"]))  # rows are caller indices here: root = label
            assert np.array_equal(np.array([flag[r] for r in root]), ref["span"])
            for x in range(n):
                if not ref["span"][x]:                                              # c_x - c_root, root the label member
                    assert c[x] == tuple(ref["image"][x].tolist()), (x, c[x], ref["image"][x])
        spanning += int(ref["pstats"][0])
        finite += int((ref["image"] != 0).any())
    assert spanning >= 3 and finite >= 3


# ---- pack and unpack ------------------------------------------------------------------------------------------------------------------

def test_word_pack_and_unpack():
    import pse_amd
    assert pse_amd.host_cluster_word(5, (0, 0, 0)) == 5                              # a root is the number of its row
    top = 2 ** 28 - 1
    for parent in (0, 1, 12345, top):
        for c in ((0, 0, 0), (1, -1, 0), (-1, 1, 1), (2047, -2047, 2047), (-2047, 2047, -2047), (7, -300, 2047)):
            w = pse_amd.host_cluster_word(parent, c)
            assert 0 <= w < 2 ** 64 and w & (2 ** 28 - 1) == parent
            assert pse_amd.host_cluster_word_parts(w) == (parent, c)
            assert [(w >> s) & 0xfff for s in (28, 40, 52)] == [v & 0xfff for v in c]   # 12-bit two's complement, a1 lowest
    for parent, c, word in ((2 ** 28, (0, 0, 0), "parent"), (0, (2048, 0, 0), "offset"), (0, (0, -2048, 0), "offset"), (0, (0, 0, 2048), "offset"),
                            (top, (0, 0, -2048), "offset")):
        with pytest.raises(pse_amd.PSEError, match=word):
            pse_amd.host_cluster_word(parent, c)
    with pytest.raises(ValueError):
        pse_amd.host_cluster_word(0, (0, 0))
    with pytest.raises(ValueError):
        pse_amd.host_cluster_word_parts(2 ** 64)
    assert pse_amd.host_cluster_word_parts(2 ** 64 - 1) == (top, (-1, -1, -1))


# ---- pse_clusters_span on the device stand-in ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_last_error", "pse_clusters_create", "pse_clusters_destroy", "pse_clusters_span",
                 "pse_clusters_status", "pse_exclusions_create", "pse_host_cluster_word", "pse_host_cluster_word_parts"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


def test_refusals_of_span_on_the_stand_in_in_order(stub):
    n = 6
    h, other = stub_handle(stub, n), stub_handle(stub, n)
    slab = stub_handle(stub, n, L=40.0, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    rl = np.array([1.5])

    def links(hh):
        g = ctypes.c_void_p()
        assert stub.pse_clusters_create(hh, n, None, 1, vp(rl), ctypes.byref(g)) == 0, stub.pse_last_error()
        return g

    g, gslab = links(h), links(slab)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex, ex_other = ctypes.c_void_p(), ctypes.c_void_p()
    assert stub.pse_exclusions_create(h, n, 1, vp(pairs), ctypes.byref(ex)) == 0
    assert stub.pse_exclusions_create(other, n, 1, vp(pairs), ctypes.byref(ex_other)) == 0
    buf = np.zeros(8)
    X, odd = vp(buf), ctypes.c_void_p(buf.ctypes.data + 4)
    outs = ("label", "size", "stats", "hist", "span", "image", "rg2", "pstats")

    def call(word, gg=g, pos=X, N=n, nhist=4, e=None, **kw):
        a = dict({k: X for k in outs}, **kw)
        rc = stub.pse_clusters_span(gg, pos, None, N, a["label"], a["size"], a["stats"], a["hist"], nhist, a["span"], a["image"], a["rg2"],
                                    a["pstats"], e)
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg and "pse_clusters_span" in msg), (word, rc, msg)

    none = {k: None for k in outs}
    call("null cluster object", gg=None)
    call("N = 0", N=0)
    call("N = 7", N=n + 1)
    call("null pos", pos=None)
    call("all null", **none)
    call("stats is not 8-byte aligned", stats=odd)
    call("hist is not 8-byte aligned", hist=odd)
    call("nhist = 0", nhist=0)
    call("another handle", e=ex_other)
    call("slab rank", gg=gslab)
    call("rg2 is not 8-byte aligned", rg2=odd)
    call("pstats is not 8-byte aligned", pstats=odd)
    # the order: each refusal wins over every later one
    call("N = 7", N=n + 1, pos=None, **none)
    call("null pos", pos=None, **none)
    call("all null", **dict(none, stats=None), nhist=0, e=ex_other)
    call("stats is not", stats=odd, hist=odd, nhist=0, rg2=odd)
    call("hist is not", hist=odd, nhist=0, e=ex_other)
    call("nhist = 0", nhist=0, e=ex_other, rg2=odd)
    call("another handle", e=ex_other, rg2=odd, pstats=odd)
    call("slab rank", gg=gslab, rg2=odd, pstats=odd)
    call("rg2 is not", rg2=odd, pstats=odd)
    call(None, e=ex)
    call(None)
    call(None, hist=None, nhist=0)
    call(None, span=ctypes.c_void_p(buf.ctypes.data + 4), image=ctypes.c_void_p(buf.ctypes.data + 4))   # 4-byte words
    for only in outs:                                                                # each output alone will do
        call(None, **{k: None for k in outs if k != only})
    # the word helpers of the same library
    w, parent, c = ctypes.c_ulonglong(0), ctypes.c_uint(0), np.zeros(3, dtype=np.int32)
    assert stub.pse_host_cluster_word(9, vp(np.array([1, -2, 3], dtype=np.int32)), ctypes.byref(w)) == 0
    assert stub.pse_host_cluster_word_parts(w.value, ctypes.byref(parent), vp(c)) == 0 and (parent.value, c.tolist()) == (9, [1, -2, 3])
    assert stub.pse_host_cluster_word(9, None, ctypes.byref(w)) == INVALID and "null c" in stub.pse_last_error().decode()
    assert stub.pse_host_cluster_word(9, vp(c), None) == INVALID and "null word" in stub.pse_last_error().decode()
    assert stub.pse_host_cluster_word_parts(w.value, None, vp(c)) == INVALID and "null parent" in stub.pse_last_error().decode()
    for hh in (h, other, slab):
        assert stub.pse_destroy(hh) == 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------

def test_numpy_helpers_and_argument_checks_without_a_device():
    from pse_amd import analyze
    box = pr.TILTED
    pos = np.array([[1.0, 2.0, 3.0, 0.0], [-1.0, 0.5, 0.0, 0.0]])
    images = np.array([[1, -2, 3], [0, 0, 0]])
    U = analyze.unfold_clusters(pos, images, box)
    assert np.allclose(U, pr.unfolded(pos[:, :3], images, box), rtol=0, atol=1e-12) and U.shape == (2, 3)
    assert np.array_equal(analyze.unfold_clusters(pos[:, :3], images, box[:3]), pos[:, :3] + images * np.array(box[:3]))
    with pytest.raises(ValueError, match="images"):
        analyze.unfold_clusters(pos, images[:1], box)
    # s = 3 Rg^1.8 exactly
    rg = np.array([1.0, 2.0, 3.5, 6.0, 10.0])
    sizes = 3.0 * rg ** 1.8
    assert abs(analyze.fractal_dimension_of(sizes, rg ** 2, smin=1) - 1.8) < 1e-12
    mixed_s, mixed_r = np.concatenate([sizes, [1.0, 500.0, 2.0]]), np.concatenate([rg ** 2, [0.0, -1.0, 9.0]])
    assert abs(analyze.fractal_dimension_of(mixed_s, mixed_r, smin=3) - 1.8) < 1e-12     # a singleton, a spanning and a small cluster drop out
    with pytest.raises(ValueError, match="no slope"):
        analyze.fractal_dimension_of([10, 12], [4.0, -1.0], smin=5)
    with pytest.raises(ValueError, match="one entry per cluster"):
        analyze.fractal_dimension_of([10, 12], [4.0])
    prow = np.array([[1, 40, 1, 0, 0, 0, 6, 100], [0, 0, 0, 0, 0, 0, 9, 300], [2, 70, 1, 1, 0, 0, 3, 50]])
    srow = np.array([[5, 40, 0, 100], [9, 9, 300, 100], [6, 50, 0, 100]])
    assert analyze.percolation_averages_of((prow, srow)) == (2.0 / 3.0, 450.0 / 190.0)
    assert [analyze.percolation_averages_of((prow, srow), k)[0] for k in (0, 1, 2)] == [2.0 / 3.0, 1.0 / 3.0, 0.0]
    assert math.isnan(analyze.percolation_averages_of(([[1, 10, 1, 1, 1, 1, 0, 0]], [[1, 10, 100, 10]]))[1])
    with pytest.raises(ValueError, match="no samples"):
        analyze.percolation_averages_of((np.zeros((0, 8)), np.zeros((0, 4))))
    with pytest.raises(ValueError, match="axis"):
        analyze.percolation_averages_of((prow, srow), 3)
    for word, kw in (("every pair type is off", dict(rlink=0.0)), ("capacity", dict(rlink=1.0, capacity=0))):
        with pytest.raises(ValueError, match=word):                                  # percolation=True adds no check of its own and skips none
            analyze.Clusters(_NoDevice(), percolation=True, **kw)
    assert analyze.Clusters.PERCOLATION_COLUMNS[0] == "timestep" and len(analyze.Clusters.PERCOLATION_COLUMNS) == 9
