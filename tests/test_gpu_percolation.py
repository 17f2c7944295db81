"""GPU tests of the cluster analysis with percolation (pse_clusters_span) and of analyze.Clusters(percolation=True) on top of it,
against the reference of tests/percolation_ref.py (validated on the CPU by tests/test_percolation_cpu.py, which also holds every input
used here to the margins): N <= 513, seconds in all.

label, size, stats and hist must EQUAL both the reference and what pse_clusters_label writes on the same object; span, image and pstats
must EQUAL the reference.  rg2 is held to 8 2^-53 2^-40 sum q^2 / s of the exact rational value (the roundings of the fixed fp64
expression; every q equals the reference's by the q margin), and on the inputs whose coordinates and lattice vectors are multiples of
2^-10 -- every D exact -- it must equal, bit for bit, that fixed expression evaluated on the exact integer sums in Python floats (the
rounded exact value itself differs from ANY fp64 evaluation of a difference of two quotients in the last bits).
status() is 0 after every case."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
import percolation_ref as pr
from test_gpu_clusters import restored_context, system  # noqa: F401  (the fixture and the frozen-system helper of the cluster tests)

pytestmark = pytest.mark.gpu

NMAX = pr.NMAX
CUBIC, TILTED = pr.CUBIC, pr.TILTED
BOXES = pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
INVALID = -1
SENTINEL = -7
OUTS = ("label", "size", "stats", "hist", "span", "image", "rg2", "pstats")
PLANTED = pr.planted()
# the flags every planted input must show (the reference is held to this before the device is)
EXPECT = {"rod_a1": {1}, "rod_a2": {2}, "rod_a3": {4}, "rod_110": {3}, "rod_111": {7}, "double_helix": {1}, "open_helix": {0}, "closed_helix": {1},
          "c_shape": {0}, "two_rods_and_a_cloud": {0, 1, 4}, "lattice": {7}, "chain": {0}, "chain_closed": {1}, "rod_excluded_pair": {0},
          "rod_pair_type_off": {0}, "rod_pair_type_on": {1}, "grid_rod": {0, 1}}


def port():
    from oracle import pse_port
    pse_port.lib()
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(NMAX, box, xi=0.5, error=1e-3)


def reference(pos, box, rlink, types=None, ntypes=1, excl=None, **kw):
    ref = pr.span(pos, box, types, ntypes, rlink, port(), excl=excl, **kw)
    pr.assert_clear(ref)
    return ref


def buffers(rows, members=None, nhist=None):
    import torch
    new = lambda shape, dt: torch.full(shape, SENTINEL, dtype=dt, device="cuda")   # noqa: E731
    return dict(label=new((rows,), torch.int32), size=new((rows,), torch.int32), stats=new((4,), torch.int64),
                hist=torch.zeros((rows if members is None else members) if nhist is None else nhist, dtype=torch.int64, device="cuda"),
                span=new((rows,), torch.int32), image=new((rows, 3), torch.int32), rg2=new((rows,), torch.float64), pstats=new((8,), torch.int64))


def host(bufs):
    return {k: (v.cpu().numpy() if k == "rg2" else v.cpu().numpy().astype(np.int64)) for k, v in bufs.items() if v is not None}


def device(eng, pos, rlink, types=None, ntypes=1, group=None, exclusions=None, links=None):
    """One pse_clusters_label and one pse_clusters_span on one object, read back: (the four outputs of the first, the eight of the
    second), by caller index, SENTINEL where a call did not write.  status() must be 0."""
    import torch
    own = links is None
    links = eng.clusters(types, ntypes, rlink) if own else links
    g = None if group is None else torch.tensor(np.asarray(group), dtype=torch.int32, device="cuda")
    members = None if group is None else len(group)
    first, second = buffers(len(pos), members), buffers(len(pos), members)
    dpos = to4(pos)
    eng.cluster_label(dpos, links, label=first["label"], size=first["size"], stats=first["stats"], hist=first["hist"], group=g, exclusions=exclusions)
    out = eng.cluster_span(dpos, links, group=g, exclusions=exclusions, **second)
    assert all(o is second[k] for o, k in zip(out, OUTS))
    got = host({k: first[k] for k in OUTS[:4]}), host(second)
    assert links.status() == 0
    if own:
        links.close()
    return got


def assert_matches(got, ref, what="", rows=None, bitwise=False):
    """`got` of device() against the reference; rows: the caller indices the reference's rows stand for (a group)."""
    plain, full = got
    rows = np.arange(len(ref["label"])) if rows is None else np.asarray(rows)
    for name in ("label", "size", "stats", "hist", "span", "image", "pstats"):
        g, w = full[name], ref[name]
        g = g[rows] if name in ("label", "size", "span", "image") else g
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:5].ravel().tolist())
    for name in ("label", "size", "stats", "hist"):
        assert np.array_equal(plain[name], full[name]), (what, name, "differs from pse_clusters_label")
    rg2 = full["rg2"][rows]
    err = np.abs(rg2 - ref["rg2"])
    worst = int(np.argmax(err - ref["rg2_bound"]))
    print(f"{what}: rg2 max error {err.max():.3e} (bound there {ref['rg2_bound'][int(np.argmax(err))]:.3e}), "
          f"{int((rg2 == ref['rg2_fixed']).sum())} of {len(rg2)} bit-equal to the fixed expression")
    assert (err <= ref["rg2_bound"]).all(), (what, "rg2", worst, rg2[worst], ref["rg2"][worst], ref["rg2_bound"][worst])
    assert np.array_equal(rg2 == -1.0, ref["span"] != 0) and np.array_equal(rg2 == 0.0, (ref["size"] == 1) | (ref["rg2"] == 0.0))
    if bitwise:
        assert np.array_equal(rg2.view(np.int64), ref["rg2_fixed"].view(np.int64)), (what, "rg2 bits")


# -- random regimes ----------------------------------------------------------------------------------------------------------------------

@BOXES
@pytest.mark.parametrize("n", pr.NS)
def test_random_regimes(n, box):
    eng = engine(box)
    for m, rlink, pos in pr.random_regimes(box):
        if m != n:
            continue
        ref = reference(pos, box, rlink)
        print(f"n = {n}, rlink = {rlink:.4f}: stats {ref['stats'].tolist()}, pstats {ref['pstats'].tolist()}")
        assert_matches(device(eng, pos, rlink), ref, (n, rlink))


# -- planted cases, contention and depth, switches ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted(name):
    pos, box, kw = PLANTED[name]
    ref = reference(pos, box, **kw)
    flags = set(ref["span"].tolist())
    key = [k for k in EXPECT if name == k or name.startswith(k + "_")]
    if name.endswith("_short"):
        assert flags == {0} and ref["stats"][0] == len(pos)                                      # 1e-6 short of the spacing: singletons
    elif key:
        assert flags == EXPECT[max(key, key=len)], (name, flags)
    if name in ("lattice", "chain", "chain_closed"):
        assert ref["stats"][0] == 1                                                              # every row in one tree
    if name == "open_helix_cubic":
        assert sorted(set(ref["image"][:, 0].tolist())) == [0, 1, 2, 3, 4, 5]
    if name.startswith(("c_shape", "rod_excluded_pair")):
        assert ref["image"].any() and ref["stats"][0] == 1
    eng = engine(box)
    ex = None if kw.get("excl") is None else eng.exclusions(kw["excl"])
    got = device(eng, pos, kw["rlink"], kw.get("types"), kw.get("ntypes", 1), exclusions=ex)
    assert_matches(got, ref, name, bitwise=name.startswith("grid"))
    if ex is not None:
        assert_matches(device(eng, pos, kw["rlink"]), reference(pos, box, kw["rlink"]), name + " without the exclusion")
        assert set(reference(pos, box, kw["rlink"])["span"].tolist()) == {1}                     # ... the rod holds, and spans
        ex.close()


def test_chain_in_three_caller_orders_spans_alike():
    eng = engine(CUBIC)
    base = device(eng, PLANTED["chain_closed"][0], 1.0)[1]
    for name in ("chain_closed_reversed", "chain_closed_shuffled"):
        got = device(eng, PLANTED[name][0], 1.0)[1]
        for k in ("label", "size", "span", "stats", "pstats", "rg2"):
            assert np.array_equal(got[k], base[k]), (name, k)


@BOXES
def test_group(box):
    """Every particle but the fourth of the x rod: the rod is open, only the z rod spans; entries outside the group are left alone."""
    eng = engine(box)
    pos = pr.two_rods_and_a_cloud(box)
    members = np.delete(np.arange(len(pos)), 3)
    ref = reference(pos[members], box, pr.UP, ids=members)
    assert set(ref["span"].tolist()) == {0, 4}
    got = device(eng, pos, pr.UP, group=members)
    assert_matches(got, ref, "group", rows=members)
    for k in ("label", "size", "span", "rg2"):
        assert got[1][k][3] == SENTINEL
    assert (got[1]["image"][3] == SENTINEL).all()
    whole = reference(pos, box, pr.UP)
    assert set(whole["span"].tolist()) == {0, 1, 4}
    assert_matches(device(eng, pos, pr.UP), whole, "whole")


# -- interface ---------------------------------------------------------------------------------------------------------------------------

def test_outputs_alone_repeats_and_after_a_label():
    import torch
    box = TILTED
    eng = engine(box)
    pts = pr.random_regimes(box)
    pos = [p for n, rl, p in pts if n == 513 and rl == 1.5][0]
    other = pos[::-1][:300].copy()
    a, b = reference(pos, box, 1.5), reference(other, box, 1.5)
    assert a["pstats"][0] >= 1 and a["pstats"][6] >= 10 and not np.array_equal(a["pstats"], b["pstats"])
    links = eng.clusters(None, 1, 1.5)
    dpos = to4(pos)
    alone = buffers(len(pos))
    for k in OUTS:                                                                               # every output alone
        eng.cluster_span(dpos, links, **{k: alone[k]})
    got = host(alone)
    assert_matches(({k: got[k] for k in OUTS[:4]}, got), a, "alone")
    first = device(eng, pos, 1.5, links=links)                                                   # a label, then a span, on the one object
    assert_matches(first, a, "first")
    second = device(eng, other, 1.5, links=links)                                                # two calls on one object, another input
    assert_matches(second, b, "second")
    again = device(eng, pos, 1.5, links=links)                                                   # equal bits on a repeat, rg2 included
    for k in OUTS:
        assert np.array_equal(again[1][k].view(np.int64), first[1][k].view(np.int64)), k
    # hist accumulates, stats and pstats are overwritten
    bufs = buffers(len(pos))
    eng.cluster_span(dpos, links, stats=bufs["stats"], hist=bufs["hist"], pstats=bufs["pstats"])
    eng.cluster_span(dpos, links, stats=bufs["stats"], hist=bufs["hist"], pstats=bufs["pstats"])
    assert np.array_equal(bufs["hist"].cpu().numpy(), 2 * a["hist"]) and np.array_equal(bufs["pstats"].cpu().numpy(), a["pstats"])
    assert links.status() == 0
    new = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device="cuda")            # noqa: E731
    with pytest.raises(ValueError, match="all None"):
        eng.cluster_span(dpos, links)
    for word, kw in (("span must be", dict(span=new(512))), ("image must be", dict(image=new((513, 2)))), ("rg2 must be", dict(rg2=new(513))),
                     ("pstats must be", dict(pstats=new(8))), ("label must be", dict(label=new(512))), ("stats must be", dict(stats=new(4)))):
        with pytest.raises(ValueError, match=word):
            eng.cluster_span(dpos, links, **kw)
    links.close()
    with pytest.raises(ValueError, match="closed"):
        eng.cluster_span(dpos, links, span=alone["span"])


def test_misuse_is_reported_before_any_launch():
    """Raw C-ABI: a rejected call leaves the outputs untouched, and the object works afterwards."""
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
        assert lib.pse_create(ctypes.byref(p), ctypes.byref(out)) == 0, msg()
        return out

    pos, box, kw = PLANTED["two_rods_and_a_cloud_cubic"]
    n = len(pos)
    h, h2, hs = create(box[0], n), create(box[0], n), create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    rl = np.array([kw["rlink"]])

    def links_on(hh):
        g = ctypes.c_void_p()
        assert lib.pse_clusters_create(hh, n, None, 1, vp(rl), ctypes.byref(g)) == 0, msg()
        return g

    g, gs = links_on(h), links_on(hs)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex2 = ctypes.c_void_p()
    assert lib.pse_exclusions_create(h2, n, 1, vp(pairs), ctypes.byref(ex2)) == 0, msg()
    dpos = to4(pos)
    bufs = buffers(n)
    bufs["hist"].fill_(SENTINEL)
    call = lib.pse_clusters_span

    def refused(word, gg=g, p=P(dpos), nn=n, nh=n, e=None, **kw):
        a = dict({k: P(bufs[k]) for k in OUTS}, **kw)
        assert call(gg, p, None, nn, a["label"], a["size"], a["stats"], a["hist"], nh, a["span"], a["image"], a["rg2"], a["pstats"], e) == INVALID, word
        assert word in msg() and "pse_clusters_span" in msg(), (word, msg())

    odd = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 4)   # noqa: E731
    refused("null cluster object", gg=None)
    refused("n_max", nn=0)
    refused("n_max", nn=n + 1)
    refused("null pos", p=None)
    refused("all null", **{k: None for k in OUTS})
    refused("stats is not 8-byte aligned", stats=odd("stats"))
    refused("hist is not 8-byte aligned", hist=odd("hist"))
    refused("nhist = 0", nh=0)
    refused("another handle", e=ex2)
    refused("slab rank", gg=gs)
    refused("rg2 is not 8-byte aligned", rg2=odd("rg2"))
    refused("pstats is not 8-byte aligned", pstats=odd("pstats"))
    torch.cuda.synchronize()
    for t in bufs.values():
        assert np.all(t.cpu().numpy() == SENTINEL)                                               # nothing was launched, nothing was written
    bufs["hist"].zero_()
    a = {k: P(bufs[k]) for k in OUTS}
    assert call(g, P(dpos), None, n, a["label"], a["size"], a["stats"], a["hist"], n, a["span"], a["image"], a["rg2"], a["pstats"], None) == 0, msg()
    word = ctypes.c_uint(99)
    assert lib.pse_clusters_status(g, ctypes.byref(word)) == 0 and word.value == 0
    got = host(bufs)
    assert_matches(({k: got[k] for k in OUTS[:4]}, got), reference(pos, box, kw["rlink"]), "raw")
    assert lib.pse_clusters_destroy(g) == 0
    for hh in (h, h2, hs):
        assert lib.pse_destroy(hh) == 0


def test_captured_graph_replayed_twice():
    import pse_amd
    import torch
    box = TILTED
    full = [p for n, rl, p in pr.random_regimes(box) if n == 513 and rl == 1.5][0]
    frames = [full[:300], full[213:]]
    wants = [reference(p, box, 1.8) for p in frames]
    assert wants[0]["pstats"][0] == wants[1]["pstats"][0] == 1 and set(wants[0]["span"].tolist()) != set(wants[1]["span"].tolist())
    eng = pse_amd.Engine(300, box, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    links = eng.clusters(None, 1, 1.8)
    pos = to4(frames[0])
    bufs = buffers(300)
    sample = lambda: eng.cluster_span(pos, links, **bufs)   # noqa: E731
    with torch.cuda.stream(st):
        sample()                                                                               # warm-up outside the capture: places the scratch
    st.synchronize()
    got = host(bufs)
    assert_matches(({k: got[k] for k in OUTS[:4]}, got), wants[0], "eager")
    bufs["hist"].zero_(); bufs["span"].fill_(SENTINEL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        sample()
    torch.cuda.synchronize()
    assert not bufs["hist"].cpu().numpy().any() and (bufs["span"].cpu().numpy() == SENTINEL).all(), "a capture runs nothing"
    total = np.zeros(300, dtype=np.int64)
    for k, p in enumerate(frames):
        pos.copy_(to4(p))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        total += wants[k]["hist"]
        got = host(bufs)
        assert np.array_equal(got["hist"], total)
        got["hist"] = wants[k]["hist"]
        assert_matches(({k2: got[k2] for k2 in OUTS[:4]}, got), wants[k], ("replay", k))
    assert links.status() == 0
    links.close()
    eng.close()


# -- analyze.Clusters --------------------------------------------------------------------------------------------------------------------

def test_percolating_clusters_through_system_run(restored_context):
    """A frozen configuration (kT = 0, no forces): every sample is the same, so every reader is the reference; the ring after more
    samples than its capacity; and Clusters() without the keyword has exactly the table it has without this feature."""
    from pse_amd import analyze
    box = CUBIC
    pos = [p for n, rl, p in pr.random_regimes(box) if n == 513 and rl == 1.5][0]
    ref = reference(pos, box, 1.5, nhist=6)
    assert ref["pstats"][0] >= 1 and ref["pstats"][6] >= 10
    s, pse = system(pos, box)
    cl = analyze.Clusters(pse, 1.5, period=2, nhist=6, capacity=2, percolation=True)
    plain = analyze.Clusters(pse, 1.5, period=2, nhist=6, capacity=2)
    assert s.analyzers == [cl, plain] and cl.percolation and not plain.percolation
    for reader in (cl.spanning, cl.images, cl.rg2, cl.unfolded, cl.cluster_table, cl.percolation_probability):
        with pytest.raises(ValueError, match="no samples"):
            reader()
    s.run(5)                                                                                     # samples at steps 0, 2 and 4
    assert np.abs(s.pos.cpu().numpy()[:, :3] - pos).max() == 0.0                                 # frozen
    assert cl.samples == 3 and cl.status() == 0 and plain.status() == 0
    # without the keyword: the table, labels and sizes of today, and no reader of the new ones
    assert analyze.Clusters.COLUMNS == ("timestep", "clusters", "largest", "sum_s2", "N")
    assert plain.table().dtype == np.int64 and plain.table().tolist() == [[t] + ref["stats"].tolist() for t in (2, 4)]
    assert np.array_equal(plain.labels(), ref["label"]) and np.array_equal(plain.sizes(), ref["size"])
    assert np.array_equal(plain.size_distribution() * 3, 3 * ref["hist"])
    for reader in (plain.spanning, plain.images, plain.rg2, plain.unfolded, plain.cluster_table, plain.percolation_table):
        with pytest.raises(ValueError, match="percolation=True"):
            reader()
    # with it: the same four, and the new readers
    assert cl.table().tolist() == plain.table().tolist() and np.array_equal(cl.labels(), ref["label"]) and np.array_equal(cl.sizes(), ref["size"])
    assert np.array_equal(cl.size_distribution(), plain.size_distribution())
    assert np.array_equal(cl.spanning(), ref["span"]) and np.array_equal(cl.images(), ref["image"])
    assert (np.abs(cl.rg2() - ref["rg2"]) <= ref["rg2_bound"]).all()
    assert cl.percolation_table().tolist() == [[t] + ref["pstats"].tolist() for t in (2, 4)]     # a ring of two rows
    U = cl.unfolded()
    assert np.array_equal(U, analyze.unfold_clusters(pos, ref["image"], box)) and np.abs(U - pr.unfolded(pos, ref["image"], box)).max() < 1e-12
    i, j = ref["links"]
    finite = ref["span"][i] == 0
    d = U[i[finite]] - U[j[finite]]
    assert finite.sum() > 50 and (np.sqrt((d * d).sum(axis=1)) < 1.5).all()                      # made whole: every link is short
    table = cl.cluster_table()
    roots = np.unique(ref["label"])
    assert np.array_equal(table["label"], roots) and np.array_equal(table["size"], ref["size"][roots])
    assert np.array_equal(table["span"], ref["span"][roots]) and np.array_equal(table["rg2"], cl.rg2()[roots])
    assert cl.percolation_probability() == 1.0
    assert [cl.percolation_probability(k) for k in range(3)] == [float(ref["pstats"][2 + k] > 0) for k in range(3)]
    ps, st = ref["pstats"], ref["stats"]
    assert cl.finite_weight_average() == float(2 * ps[7]) / float(2 * (st[3] - ps[1]))
    big = table[(table["span"] == 0) & (table["size"] >= 3)]
    df = analyze.fractal_dimension_of(big["size"], big["rg2"], smin=3)
    assert 0.5 < df < 3.5, df
    cl.reset()
    assert cl.samples == 0 and len(cl.percolation_table()) == 0 and len(cl.table()) == 0
    s.run(1)                                                                                     # step 5: not a sample
    assert cl.samples == 0
    s.run(1)                                                                                     # step 6
    assert cl.samples == 1 and cl.percolation_table().tolist() == [[6] + ref["pstats"].tolist()]
