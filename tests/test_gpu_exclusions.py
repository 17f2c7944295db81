"""GPU tests of the pair exclusions (pse_exclusions_create, pse_pair_table_excl, pse_pair_repulsion_excl): forces, energy, virial and
pair count against the O(N^2) reference of tests/exclusion_ref.py (validated on the CPU by tests/test_exclusion_rows_cpu.py) with
exclusions planted among the pairs that act -- random points rarely put a given index pair in range -- a long row (a hub), the wave
and workgroup edges, a group (exclusions are caller indices), an object shorter than the arrays, bit-identity with the plain entry
points and under the order of the list, every call form, asynchronous submission, the error returns, and the providers on top
(forces.Exclusions.from_topology, forces.TablePair beside forces.Bonds with a forces.StressLog, the topology builder of
examples/sticky_polymers.py).

Bound: the project's own for these passes (tests/test_gpu_pair_table.py), 1e-11 max(1, max |ref|), the eight observables together and
the forces together; npairs must match exactly.  Boxes, table and sizes are those of tests/test_gpu_pair_table.py."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import to4
import exclusion_ref as xr
import pair_table_ref
import pair_virial_ref
from pair_table_ref import morse_table, random_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAX = 513
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
N = 300
K, SIGMA = 40.0, 2.0
INVALID = -1
MORSE = dict(D=5.0, alpha=2.0, r0=1.5)
RMIN, RMAX = 0.7, 3.0
KINDS = ("table", "repulsion")


def port():
    from oracle import pse_port
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(NMAX, box, xi=0.5, error=1e-3)


@functools.lru_cache(maxsize=None)
def w1000():
    t = morse_table(rmin=RMIN, rmax=RMAX, width=1000, **MORSE)
    t.setflags(write=False)
    return t


def dev(a):
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")


def acting(kind, pos, box):
    """(i, j) of the pairs of rows of pos that the plain pass acts on."""
    if kind == "table":
        return pair_table_ref.pair_terms(pos, box, w1000(), RMIN, RMAX, port())[:2]
    return pair_virial_ref.pair_terms(pos, box, K, SIGMA, port())[:2]


def reference(kind, pos, box, excl, ids=None):
    """(obs[8], F, number of in-range pairs excluded)"""
    if kind == "table":
        return xr.table_observables(pos, box, w1000(), RMIN, RMAX, port(), excl, ids)
    return xr.repulsion_observables(pos, box, K, SIGMA, port(), excl, ids)


def device(kind, eng, dpos, f, ex, group=None, accumulate=False, out=None):
    """The fused call of `kind` with exclusion object ex (None: the plain entry point): returns the eight doubles (device)."""
    if kind == "table":
        return eng.pair_table(dpos, f, dev(w1000()), RMIN, RMAX, group=group, accumulate=accumulate, out=out, exclusions=ex)
    return eng.pair_repulsion_virial(dpos, f, K, SIGMA, group=group, accumulate=accumulate, out=out, exclusions=ex)


def far_pairs(n, count, seed, *acting_lists):
    """`count` random index pairs below n that are in none of the acting (i, j) lists: out of range, they must change nothing."""
    rng = np.random.default_rng(seed)
    near = set()
    for i, j in acting_lists:
        near |= set(zip(i.tolist(), j.tolist()))
    out = []
    while len(out) < count:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and (min(a, b), max(a, b)) not in near:
            out.append((a, b))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def planted(kind, box, n=N, seed=11):
    """(pos, excl, obs, F, nex, hub): a seeded half of the acting pairs, 200 out-of-range pairs, and a hub -- the particle with the
    most in-range neighbours, excluded from all of them and from 250 others: a long row.  Computed once, shared, never written to."""
    pos = random_points(n, box, seed)
    i, j = acting(kind, pos, box)
    rng = np.random.default_rng(21)
    half = rng.uniform(size=len(i)) < 0.5
    hub = int(np.argmax(np.bincount(np.concatenate([i, j]), minlength=n)))
    nbrs = np.concatenate([j[i == hub], i[j == hub]])
    others = rng.permutation(np.delete(np.arange(n), hub))[:250]
    excl = np.concatenate([np.stack([j[half], i[half]], axis=1), far_pairs(n, 200, 31, (i, j)),
                           np.stack([np.full(len(nbrs), hub), nbrs], axis=1), np.stack([others, np.full(250, hub)], axis=1)])
    excl = excl[rng.permutation(len(excl))]
    obs, F, nex = reference(kind, pos, box, excl)
    for a in (pos, excl, obs, F):
        a.setflags(write=False)
    return pos, excl, obs, F, nex, hub


def check_obs(got, ref, what=""):
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"{what}: max |obs - ref| = {err:.3e} (bound {tol:.3e}), npairs {got[7]:.0f} / {ref[7]:.0f}, U {ref[0]:.6g}")
    assert got[7] == ref[7], (what, got[7], ref[7])
    assert err <= tol, (what, got, ref)


def check_forces(got, ref, what=""):
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"{what}: max |F - ref| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("kind", KINDS)
def test_planted_exclusions(kind, box):
    eng = engine(box)
    pos, excl, ref, F, nex, hub = planted(kind, box)
    i, j = acting(kind, pos, box)
    assert nex >= 20 and ref[7] >= 20 and ref[7] + nex == len(i)                     # neither path is vacuous
    plain, Fplain, _ = reference(kind, pos, box, None)
    assert np.abs(plain - ref).max() > 1.0 and np.abs(Fplain[hub]).max() > 0.1       # the exclusions matter, also at the hub
    ex = eng.exclusions(excl, n=N)
    off, _ = xr.rows_numpy(N, excl)
    assert np.diff(off).max() == off[hub + 1] - off[hub] > 250                       # the long row
    f = to4(np.random.default_rng(5).normal(size=(N, 3)), 7.0)
    out = device(kind, eng, to4(pos), f, ex).cpu().numpy()
    check_obs(out, ref, f"{kind}: half of {len(i)} pairs, 200 far pairs and a hub of {off[hub + 1] - off[hub]}")
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, kind)
    assert np.all(g[:, 3] == 7.0)
    assert np.all(g[hub, :3] == 0.0) and not F[hub].any()                            # nothing acts on the hub: exactly zero
    ex.close()


@pytest.mark.parametrize("n", [2, 65, 257, 513])
def test_row_counts(n):
    """Two particles whose only pair is excluded; one lane of the second wave; one lane of the second workgroup; three workgroup
    rows for the finishing kernel."""
    box = TILTED
    eng = engine(box)
    pos = random_points(n, box, seed=100 + n)
    if n == 2:
        pos[1] = pos[0] + np.array([0.9, -0.7, 0.4])                                 # in range of both passes
    for kind in KINDS:
        i, j = acting(kind, pos, box)
        if n == 2:
            assert len(i) == 1
            excl = np.array([[1, 0]])
        else:
            excl = np.stack([i[::2], j[::2]], axis=1)
        ref, F, nex = reference(kind, pos, box, excl)
        assert nex == len(excl) >= 1
        if n == 2:
            assert not ref.any() and not F.any()
        else:
            assert ref[7] >= 1
        ex = eng.exclusions(excl, n=n)
        f = to4(np.ones((n, 3)), 3.0)
        out = device(kind, eng, to4(pos), f, ex).cpu().numpy()
        check_obs(out, ref, f"{kind} n={n}")
        g = f.cpu().numpy()
        check_forces(g[:, :3], F, f"{kind} n={n}")
        assert np.all(g[:, 3] == 3.0)
        if n == 2:
            assert not out.any() and not g[:, :3].any()                              # eight zeros, zero forces
        ex.close()


@pytest.mark.parametrize("kind", KINDS)
def test_group_exclusions_are_caller_indices(kind):
    """Every other particle is in the group.  The exclusions name particles by their index in the caller's arrays -- the values of
    `group` -- not by their position in the group and not by their row of the engine's sorted order: the reference is taken over the
    members with the same index pairs."""
    import torch
    box = TILTED
    eng = engine(box)
    pos = random_points(N, box, seed=11)
    members = np.arange(0, N, 2)
    i, j = acting(kind, pos[members], box)                                           # rows of the group ...
    half = np.random.default_rng(8).uniform(size=len(i)) < 0.5
    excl = np.stack([members[i[half]], members[j[half]]], axis=1)                    # ... named by their caller indices
    # pairs of NON-members in range of each other, and pairs that would hit if a position in the group were taken for an index
    io, jo = acting(kind, pos, box)
    odd = (io % 2 == 1) & (jo % 2 == 1)
    excl = np.concatenate([excl, np.stack([io[odd], jo[odd]], axis=1)])
    ref, F, nex = reference(kind, pos[members], box, excl, ids=members)
    wrong = reference(kind, pos[members], box, excl)[0]                              # positions in the group read as indices
    assert nex == int(half.sum()) >= 5 and ref[7] >= 5 and wrong[7] != ref[7]
    ex = eng.exclusions(excl, n=N)
    sentinel = np.random.default_rng(9).normal(size=(N, 3))
    f = to4(sentinel, 7.0)
    group = torch.tensor(members, dtype=torch.int32, device="cuda")
    out = device(kind, eng, to4(pos), f, ex, group=group).cpu().numpy()
    check_obs(out, ref, f"{kind}: group of every other particle")
    g = f.cpu().numpy()
    check_forces(g[members, :3], F, f"{kind}: group")
    assert np.array_equal(g[1::2, :3], sentinel[1::2]) and np.all(g[:, 3] == 7.0)    # non-members untouched
    ex.close()


@pytest.mark.parametrize("kind", KINDS)
def test_object_shorter_than_the_arrays(kind):
    """An object created with n = 100 on 300 particles: the particles 100 .. 299 have no exclusions, and no row is read for them."""
    box = CUBIC
    eng = engine(box)
    pos = random_points(N, box, seed=11)
    i, j = acting(kind, pos, box)
    low = (i < 100) & (j < 100)
    excl = np.stack([i[low], j[low]], axis=1)
    ref, F, nex = reference(kind, pos, box, excl)
    assert nex == int(low.sum()) >= 5 and ref[7] == len(i) - nex
    ex = eng.exclusions(excl, n=100)
    assert ex.n == 100
    f = to4(np.zeros((N, 3)), 7.0)
    out = device(kind, eng, to4(pos), f, ex).cpu().numpy()
    check_obs(out, ref, f"{kind}: ex->n = 100 < N = {N}")
    check_forces(f.cpu().numpy()[:, :3], F, kind)
    with pytest.raises(Exception, match="n = 100"):                                  # an index the object has no row for
        eng.exclusions([[0, 100]], n=100)
    ex.close()


def test_bit_identity_with_the_plain_passes_and_under_list_order():
    box = TILTED
    eng = engine(box)
    pos = random_points(N, box, seed=11)
    dpos, dtab = to4(pos), dev(w1000())
    far = far_pairs(N, 200, 41, acting("table", pos, box), acting("repulsion", pos, box))
    ex = eng.exclusions(far, n=N)
    zero = lambda: to4(np.zeros((N, 3)), 7.0)                                        # noqa: E731
    # the same summation order: with nothing in range excluded, every bit is the plain entry point's
    for kind in KINDS:
        fa, fb = zero(), zero()
        a = device(kind, eng, dpos, fa, None).cpu().numpy()
        b = device(kind, eng, dpos, fb, ex).cpu().numpy()
        assert a[7] > 20 and np.array_equal(a, b) and np.array_equal(fa.cpu().numpy(), fb.cpu().numpy()), kind
    fa, fb = zero(), zero()                                                          # forces only
    eng.pair_table(dpos, fa, dtab, RMIN, RMAX, accumulate=False, observables=False)
    eng.pair_table(dpos, fb, dtab, RMIN, RMAX, accumulate=False, observables=False, exclusions=ex)
    assert np.array_equal(fa.cpu().numpy(), fb.cpu().numpy()) and fa[:, :3].abs().max().item() > 0.1
    fa, fb = zero(), zero()
    eng.pair_repulsion(dpos, fa, K, SIGMA, accumulate=False)
    eng.pair_repulsion(dpos, fb, K, SIGMA, accumulate=False, exclusions=ex)
    assert np.array_equal(fa.cpu().numpy(), fb.cpu().numpy()) and fa[:, :3].abs().max().item() > 0.1
    ex.close()
    # a function of the pair set: permuted, flipped, with duplicates; and a repeated call
    for kind in KINDS:
        _, excl, ref, F, _, _ = planted(kind, box)
        rng = np.random.default_rng(3)
        other = np.concatenate([excl, excl[rng.integers(0, len(excl), 100)]])
        other = other[rng.permutation(len(other))]
        flip = rng.uniform(size=len(other)) < 0.5
        other[flip] = other[flip, ::-1]
        e1, e2 = eng.exclusions(excl, n=N), eng.exclusions(other, n=N)
        f1, f2, f3 = zero(), zero(), zero()
        a = device(kind, eng, dpos, f1, e1).cpu().numpy()
        b = device(kind, eng, dpos, f2, e2).cpu().numpy()
        c = device(kind, eng, dpos, f3, e1).cpu().numpy()
        check_obs(a, ref, f"{kind}: set")
        assert np.array_equal(a, b) and np.array_equal(f1.cpu().numpy(), f2.cpu().numpy()), kind
        assert np.array_equal(a, c) and np.array_equal(f1.cpu().numpy(), f3.cpu().numpy()), kind
        e1.close(); e2.close()


def test_call_forms():
    import torch
    box = TILTED
    eng = engine(box)
    dtab = dev(w1000())
    base = np.random.default_rng(5).normal(size=(N, 3))
    for kind in KINDS:
        pos, excl, ref, F, _, _ = planted(kind, box)
        dpos = to4(pos)
        ex = eng.exclusions(excl, n=N)
        # accumulate = 0: overwritten, w kept; accumulate = 1: added
        f0, f1 = to4(base, 7.0), to4(base, 7.0)
        check_obs(device(kind, eng, dpos, f0, ex, accumulate=False).cpu().numpy(), ref, f"{kind} accumulate=0")
        check_obs(device(kind, eng, dpos, f1, ex, accumulate=True).cpu().numpy(), ref, f"{kind} accumulate=1")
        g0, g1 = f0.cpu().numpy(), f1.cpu().numpy()
        check_forces(g0[:, :3], F, f"{kind} accumulate=0")
        check_forces(g1[:, :3] - base, F, f"{kind} accumulate=1")
        assert np.all(g0[:, 3] == 7.0) and np.all(g1[:, 3] == 7.0)
        # force = None: the same eight numbers
        c = device(kind, eng, dpos, None, ex).cpu().numpy()
        check_obs(c, ref, f"{kind} force=None")
        # out8 = NULL: forces only
        for acc, want in ((False, F), (True, F + base)):
            f2 = to4(base, 7.0)
            if kind == "table":
                out = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
                assert eng.pair_table(dpos, f2, dtab, RMIN, RMAX, accumulate=acc, out=out, observables=False, exclusions=ex) is None
                assert np.isnan(out.cpu().numpy()).all()
            else:
                assert eng.pair_repulsion(dpos, f2, K, SIGMA, accumulate=acc, exclusions=ex) is f2
            g2 = f2.cpu().numpy()
            check_forces(g2[:, :3], want, f"{kind} out8=NULL accumulate={acc}")
            assert np.all(g2[:, 3] == 7.0)
        # a row of a log: only that row is written
        log = torch.full((6, 8), float("nan"), dtype=torch.float64, device="cuda")
        ret = device(kind, eng, dpos, None, ex, out=log[3])
        assert ret.data_ptr() == log[3].data_ptr()
        host = log.cpu().numpy()
        assert np.array_equal(host[3], c) and np.isnan(np.delete(host, 3, axis=0)).all()
        assert np.array_equal(dpos.cpu().numpy()[:, :3], pos)
        ex.close()
        with pytest.raises(ValueError, match="closed"):
            device(kind, eng, dpos, None, ex)
    # an object of another engine is refused before the call
    other = engine(CUBIC).exclusions([[0, 1]], n=N)
    with pytest.raises(ValueError, match="another engine"):
        eng.pair_table(dpos, None, dtab, RMIN, RMAX, exclusions=other)
    other.close()
    for bad in ([[0, 0]], [[0, NMAX]], np.zeros((0, 2), dtype=np.int64), [[0, 1, 2]], [[0.5, 1.0]], [[-1, 2]]):
        with pytest.raises(Exception):
            eng.exclusions(bad)


def test_async_submission_gives_the_same_numbers():
    import torch
    import pse_amd
    box = TILTED
    eng = pse_amd.Engine(N, box, xi=0.5, error=1e-3)
    for kind in KINDS:
        pos, excl, ref, F, _, _ = planted(kind, box)
        dpos = to4(pos)
        ex = eng.exclusions(excl)
        fs = to4(np.zeros((N, 3)))
        sync = device(kind, eng, dpos, fs, ex).cpu().numpy()
        eng.set_async(True)
        for _ in range(2):                                                # twice: the second call finds the first one's state in place
            fa = to4(np.zeros((N, 3)))
            out = device(kind, eng, dpos, fa, ex)
            torch.cuda.synchronize()
            out = out.cpu().numpy()
            check_obs(out, ref, f"{kind} async")
            assert np.abs(out - sync).max() <= 1e-11 * max(1.0, np.abs(ref).max())
            check_forces(fa.cpu().numpy()[:, :3], F, f"{kind} async")
        eng.set_async(False)
        ex.close()
    eng.close()


def test_misuse_is_reported_before_any_launch():
    """Raw C-ABI, as a C host would call it (the style of tests/test_gpu_errors.py)."""
    import torch
    from pse_amd import _lib
    from pse_amd._lib import pse_params
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    H = lambda a: ctypes.c_void_p(a.ctypes.data)           # noqa: E731

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

    n = 64
    box = (20.0, 20.0, 20.0, 0.0)
    pos = random_points(n, box, seed=1)
    pos[1] = pos[0] + np.array([0.6, 0.5, -0.4])
    pos[2] = pos[0] + np.array([-0.5, 0.7, 0.3])
    table = pair_table_ref.harmonic_table(1.0, 2.0, 16)
    dpos, dF, dtab = to4(pos), to4(np.zeros((n, 3)), 5.0), dev(table)
    out8 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    rc, h = create(20.0, n)
    assert rc == 0, msg()
    rc, h2 = create(20.0, n)
    assert rc == 0, msg()
    info = _lib.pse_info()
    assert lib.pse_get_info(h, ctypes.byref(info)) == 0
    rc_h = info.as_dict()["rcut"]

    # pse_exclusions_create
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex, ex2 = ctypes.c_void_p(), ctypes.c_void_p()

    def no_object(word, hh=h, nn=n, npairs=1, p=pairs, o=ex):
        rc = lib.pse_exclusions_create(hh, nn, npairs, None if p is None else H(p), None if o is None else ctypes.byref(o))
        assert rc == INVALID and word in msg() and "pse_exclusions_create" in msg(), (word, msg())
        assert o is None or not o.value

    no_object("null out", o=None)
    no_object("null handle", hh=None)
    no_object("null pairs", p=None)
    no_object("n = 0", nn=0)
    no_object("n_max", nn=n + 1)
    no_object("npairs = 0", npairs=0)
    no_object("npairs = 1073741825", npairs=(1 << 30) + 1)
    no_object("(0, 64)", p=np.array([[0, 64]], dtype=np.uint32))
    no_object("particle 7", p=np.array([[7, 7]], dtype=np.uint32))
    assert lib.pse_exclusions_create(h, n, 1, H(pairs), ctypes.byref(ex)) == 0 and ex.value, msg()
    assert lib.pse_exclusions_create(h2, n, 1, H(pairs), ctypes.byref(ex2)) == 0 and ex2.value, msg()

    table_call, rep_call = lib.pse_pair_table_excl, lib.pse_pair_repulsion_excl

    def table_refused(word, hh=h, rmax=2.0, o=P(out8), e=ex):
        assert table_call(hh, P(dpos), P(dF), None, n, P(dtab), 16, 0.0, rmax, 0, o, e) == INVALID, word
        assert word in msg(), (word, msg())

    def rep_refused(word, hh=h, f=P(dF), sigma=2.0, o=P(out8), e=ex):
        assert rep_call(hh, P(dpos), f, None, n, 1.0, sigma, 0, o, e) == INVALID, word
        assert word in msg(), (word, msg())

    table_refused("null exclusion", e=None)
    table_refused("another handle", e=ex2)
    table_refused("null handle", hh=None)
    table_refused("rcut", rmax=rc_h * (1.0 + 1e-12))                      # the refusals of pse_pair_table come first ...
    table_refused("rcut", rmax=rc_h * (1.0 + 1e-12), e=None)
    rep_refused("null exclusion", e=None)
    rep_refused("null exclusion", e=None, o=None)
    rep_refused("another handle", e=ex2)
    rep_refused("null handle", hh=None)
    rep_refused("repulsion range", sigma=rc_h * (1.0 + 1e-12))            # ... and those of the repulsion
    rep_refused("null array", f=None, o=None)                             # out8 = NULL is pse_pair_repulsion: it needs a force array
    # a slab rank orders only its own cells: observables are refused there, with or without exclusions
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    exs = ctypes.c_void_p()
    assert lib.pse_exclusions_create(hs, n, 1, H(pairs), ctypes.byref(exs)) == 0, msg()
    table_refused("slab rank", hh=hs, e=exs)
    rep_refused("slab rank", hh=hs, e=exs)
    assert lib.pse_destroy(hs) == 0                                       # (frees exs with it)
    # nothing was launched, nothing was written; and the handle works afterwards
    torch.cuda.synchronize()
    assert np.all(out8.cpu().numpy() == -1.0) and np.array_equal(dF.cpu().numpy(), to4(np.zeros((n, 3)), 5.0).cpu().numpy())
    ref, F, nex = xr.table_observables(pos, box, table, 0.0, 2.0, port(), pairs)
    assert nex == 1 and ref[7] >= 1
    assert table_call(h, P(dpos), P(dF), None, n, P(dtab), 16, 0.0, 2.0, 0, P(out8), ex) == 0, msg()
    check_obs(out8.cpu().numpy(), ref, "table after the refused calls")
    check_forces(dF.cpu().numpy()[:, :3], F, "table after the refused calls")
    ref, F, nex = xr.repulsion_observables(pos, box, 1.0, 2.0, port(), pairs)
    assert rep_call(h, P(dpos), P(dF), None, n, 1.0, 2.0, 0, P(out8), ex) == 0, msg()
    check_obs(out8.cpu().numpy(), ref, "repulsion after the refused calls")
    check_forces(dF.cpu().numpy()[:, :3], F, "repulsion after the refused calls")
    assert rep_call(h, P(dpos), P(dF), None, n, 1.0, 2.0, 0, None, ex) == 0, msg()          # forces only
    check_forces(dF.cpu().numpy()[:, :3], F, "repulsion, out8 = NULL")
    assert lib.pse_exclusions_destroy(None) == 0 and lib.pse_exclusions_destroy(ex) == 0
    assert lib.pse_destroy(h) == 0
    assert lib.pse_destroy(h2) == 0                                       # ex2 is still alive: the handle frees it


def _example():
    spec = importlib.util.spec_from_file_location("sticky_polymers", os.path.join(ROOT, "examples", "sticky_polymers.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


@pytest.fixture
def restored_context():
    """A System registers itself as the current simulation context, and a shear function made later takes its zero from that
    context's time step: put back what was there, so that the two steps run here are not some later test's time origin."""
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


def test_chains_with_bonds_a_table_and_a_stress_log(restored_context):
    """12 chains of 20 beads from the example's build_topology in the tilted box: forces.Exclusions.from_topology(bonds, angles,
    dihedrals), forces.TablePair(virial=True, exclusions=...) beside forces.Bonds through two integrator steps with a StressLog at
    period 1: every row of the log is what a direct Engine.pair_table(..., exclusions=...) gives on the positions of that step, and
    the reference; the table acts on fewer pairs than without exclusions by exactly the in-range excluded ones."""
    import torch
    from pse_amd import forces, integrate
    from pse_amd.system import System
    box = TILTED
    nchains, beads = 12, 20
    n = nchains * beads
    pos, pairs, triples, quads = _example().build_topology(nchains, beads, box, 2.0, seed=5)
    assert pos.shape == (n, 3) and pairs.shape == (nchains * (beads - 1), 2) and triples.shape == (nchains * (beads - 2), 3)
    assert quads.shape == (nchains * (beads - 3), 4)
    assert np.all(pairs[:, 1] == pairs[:, 0] + 1) and not np.any(pairs[:, 1] % beads == 0)          # no bond from chain to chain
    assert np.all(np.diff(triples, axis=1) == 1) and not np.any(triples[:, 1:] % beads == 0)
    assert np.all(np.diff(quads, axis=1) == 1) and not np.any(quads[:, 1:] % beads == 0)
    d = port().min_image(pos[pairs[:, 0]] - pos[pairs[:, 1]], box)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 2.0).max() < 1e-12                                 # steps of 2.0
    excl = forces.exclusion_pairs(pairs, triples, quads)
    assert len(excl) == nchains * (3 * beads - 6)
    vol = box[0] * box[1] * box[2]
    s = System(pos, box, dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3)           # no noise: the forces alone move the beads
    table = np.array(w1000())
    ref, F, nex = xr.table_observables(pos, box, table, RMIN, RMAX, port(), excl)
    assert nex >= len(pairs) > 0 and ref[7] > 0                                       # every bond is in range of the table
    plain = forces.TablePair(pse, table, RMIN, RMAX, virial=True)
    plain.compute(0)
    npairs_plain = plain.npairs
    s.forces.remove(plain)
    with pytest.raises(ValueError):
        forces.Exclusions.from_topology(pse)
    with pytest.raises(ValueError, match="same integrator"):
        forces.TablePair(pse, table, RMIN, RMAX, exclusions=excl)                     # the pairs are not the object
    assert s.forces == []
    xo = forces.Exclusions.from_topology(pse, bonds=pairs, angles=triples, dihedrals=quads)
    tp = forces.TablePair(pse, table, RMIN, RMAX, virial=True, exclusions=xo)
    s.net_force.zero_()
    tp.compute(0)
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "TablePair with exclusions")
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    W = np.array([[ref[1], ref[2], ref[3]], [ref[2], ref[4], ref[5]], [ref[3], ref[5], ref[6]]])
    assert abs(tp.energy - ref[0]) <= tol and tp.npairs == ref[7]
    assert np.abs(tp.virial - W).max() <= tol and np.abs(tp.stress() + W / vol).max() <= tol / vol
    assert npairs_plain - tp.npairs == nex > 0
    # the repulsion takes the same object
    rep = forces.HarmonicRepulsion(pse, k=K, sigma=2.5, virial=True, exclusions=xo)
    s.net_force.zero_()
    rep.compute(0)
    r8, rF, rnex = xr.repulsion_observables(pos, box, K, 2.5, port(), excl)
    assert rnex >= len(pairs)
    check_obs(rep._observables(), r8, "HarmonicRepulsion(virial=True) with exclusions")
    check_forces(s.net_force.cpu().numpy()[:, :3], rF, "HarmonicRepulsion with exclusions")
    s.forces.remove(rep)
    rep0 = forces.HarmonicRepulsion(pse, k=K, sigma=2.5, exclusions=xo)               # virial=False: forces only
    s.net_force.zero_()
    rep0.compute(0)
    check_forces(s.net_force.cpu().numpy()[:, :3], rF, "HarmonicRepulsion(virial=False) with exclusions")
    s.forces.remove(rep0)
    forces.Bonds(pse, pairs, kind="harmonic", k=50.0, r0=1.8)
    log = forces.StressLog(tp, period=1, capacity=4)
    eng = engine(box)
    ex = eng.exclusions(excl, n=n)
    direct = []
    for t in range(2):
        snap = s.pos.clone()
        direct.append(eng.pair_table(snap, None, tp.table, RMIN, RMAX, exclusions=ex).cpu().numpy())
        check_obs(direct[-1], xr.table_observables(snap.cpu().numpy()[:, :3], box, table, RMIN, RMAX, port(), excl)[0], f"step {t}")
        s.run(1)
    tab = log.table()
    assert tab.shape == (2, 10) and list(tab[:, 0]) == [0.0, 1.0]
    assert not np.array_equal(direct[0], direct[1])                       # the beads did move
    for row, d8 in zip(tab, direct):
        t8 = 1e-11 * max(1.0, np.abs(d8).max())
        assert abs(row[2] - d8[0]) <= t8 and row[9] == d8[7] > 0
        assert np.abs(row[3:9] + d8[1:7] / vol).max() <= t8 / vol
    assert torch.isfinite(s.pos).all()
    ex.close()
