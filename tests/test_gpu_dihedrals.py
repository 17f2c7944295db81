"""GPU tests of the dihedral forces (pse_dihedrals_create / pse_dihedral_forces): harmonic and OPLS dihedrals against the NumPy
reference of tests/dihedral_ref.py (validated on the CPU by tests/test_dihedral_reference.py, which also asserts that both bond
angles of every dihedral of the inputs used here have sin >= 0.05, the exactly collinear triples of the degenerate case apart),
bit-exact invariance under the order of the list and the direction of a quadruple, the call forms, the degenerate geometries, the
error returns, and the host UI on top (Engine.dihedrals, forces.Dihedrals with forces.Bonds, forces.Angles and a StressLog, the
topology builder of examples/helical_polymers.py).  The reference takes phi from arctan2; the device takes no atan2.

Bound: the project's own for these passes (tests/test_gpu_pair_virial.py), 1e-11 max(1, max |ref|), the eight observables together
and the forces together; the count of dihedrals must match exactly."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

import angle_ref as ar
import bond_ref as br
import dihedral_ref as dr
from conftest import to4
from pair_virial_ref import random_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBIC, TILTED = dr.BOXES
BOX_IDS = ["cubic", "tilted"]
KIND_IDS = ["harmonic", "opls"]
KIND_NAMES = {dr.HARMONIC: "harmonic", dr.OPLS: "opls"}
INVALID = -1


def port():
    from oracle import pse_port
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(dr.N_MAX, box, xi=0.5, error=1e-3)


def check_obs(got, ref, what=""):
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"{what}: max |obs - ref| = {err:.3e} (bound {tol:.3e}), ndihedrals {got[7]:.0f} / {ref[7]:.0f}, U {ref[0]:.6g}, "
          f"trace W {got[1] + got[4] + got[6]:.3e}")
    assert got[7] == ref[7], (what, got[7], ref[7])
    assert err <= tol, (what, got, ref)


def check_forces(got, F, what=""):
    tol = 1e-11 * max(1.0, np.abs(F).max())
    err = np.abs(got - F).max()
    print(f"{what}: max |F - ref| = {err:.3e} (bound {tol:.3e}), max |F| {np.abs(F).max():.6g}")
    assert err <= tol, (what, err, tol)


def reference(c, box, pos=None):
    return dr.dihedral_observables(c["pos"] if pos is None else pos, box, c["quads"], c["types"], c["kinds"], c["params"], port())


def dihedral_list(eng, c, quads=None, types="case"):
    return eng.dihedrals(c["quads"] if quads is None else quads, c["types"] if isinstance(types, str) else types, kinds=c["kinds"],
                         params=c["params"], n=len(c["pos"]))


def run_case(c, box, what):
    """accumulate = 0 on a preset force array: observables, forces, kept w."""
    n = len(c["pos"])
    ref, F = reference(c, box)
    assert ref[7] == len(c["quads"]) - c["degenerate"]
    dl = dihedral_list(engine(box), c)
    f = to4(np.random.default_rng(5).normal(size=(n, 3)), 3.0)
    out = dl.forces(to4(c["pos"]), f, accumulate=False).cpu().numpy()
    check_obs(out, ref, what)
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, what)
    assert np.all(g[:, 3] == 3.0)
    dl.close()
    return out, g


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
@pytest.mark.parametrize("kind", [dr.HARMONIC, dr.OPLS], ids=KIND_IDS)
@pytest.mark.parametrize("n", dr.ROW_COUNTS)
def test_row_counts(n, kind, box):
    """One chain of n beads, n - 3 dihedrals: the smallest list, a partial last wave, a full one, one lane of the next; the same for
    the 256-thread workgroup (257: a second workgroup of one thread; 513 = n_max: a third)."""
    run_case(dr.chain_case(n, box, kind, port()), box, f"chain n={n} kind={kind}")


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
@pytest.mark.parametrize("kind", [dr.HARMONIC, dr.OPLS], ids=KIND_IDS)
@pytest.mark.parametrize("name", dr.TOPOLOGIES + ("graph",))
def test_topologies(name, kind, box):
    c = dr.graph_case(box, kind, port()) if name == "graph" else dr.topology_case(name, box, kind, port())
    assert len(c["pos"]) == dr.N_TOPOLOGY
    out, g = run_case(c, box, f"{name} kind={kind}")
    free = np.setdiff1d(np.arange(dr.N_TOPOLOGY), np.unique(c["quads"]))
    assert len(free) > 0 and not g[free, :3].any()                    # accumulate = 0 zeroes the rows of particles in no dihedral
    if name == "star":                                                # the central bond 0-1 is j-k of all 40: two rows of 40 entries
        assert np.all(c["quads"][:, 1] == 0) and np.all(c["quads"][:, 2] == 1) and len(c["quads"]) == 40
    if name == "duplicates":                                          # every copy acts: more dihedrals than distinct quadruples
        canon = np.where((c["quads"][:, 3] < c["quads"][:, 0])[:, None], c["quads"][:, ::-1], c["quads"])
        assert out[7] == len(c["quads"]) > len(np.unique(canon, axis=0))
    if name == "two_types":
        assert sorted(c["kinds"]) == [dr.HARMONIC, dr.OPLS] and set(c["types"]) == {0, 1}


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
def test_every_multiplicity_both_signs_and_a_phase_each(box):
    """Thirteen types in one list: harmonic with mult = 1..6, d = -1 and +1 and a phi0 of its own each, and one OPLS type: the
    rotation recurrence of the device against cos and sin of mult arctan2(...) - phi0."""
    c = dr.multiplicity_case(box, port())
    assert len(c["kinds"]) == 13 and set(c["types"]) == set(range(13))
    run_case(c, box, "multiplicities")


def test_call_forms():
    """accumulate 0 and 1, force = NULL, out8 = NULL; the row of a particle in no dihedral keeps its preset value bit for bit under
    accumulate = 1 and becomes zero under accumulate = 0; w survives in both."""
    import torch
    box = TILTED
    c = dr.topology_case("chains", box, dr.HARMONIC, port())
    n = len(c["pos"])
    ref, F = reference(c, box)
    dl = dihedral_list(engine(box), c)
    dpos = to4(c["pos"])
    base = np.random.default_rng(6).normal(size=(n, 3))
    free = np.setdiff1d(np.arange(n), np.unique(c["quads"]))
    assert len(free) == 60
    # accumulate = 1
    f1 = to4(base, 7.0)
    out1 = dl.forces(dpos, f1, accumulate=True)
    assert out1.shape == (8,) and out1.is_cuda and out1.dtype == torch.float64
    check_obs(out1.cpu().numpy(), ref, "accumulate=1")
    g1 = f1.cpu().numpy()
    check_forces(g1[:, :3], F + base, "accumulate=1")
    assert np.array_equal(g1[free, :3], to4(base).cpu().numpy()[free, :3]) and np.all(g1[:, 3] == 7.0)
    # accumulate = 0
    f0 = to4(base, 7.0)
    out0 = dl.forces(dpos, f0, accumulate=False).cpu().numpy()
    g0 = f0.cpu().numpy()
    check_forces(g0[:, :3], F, "accumulate=0")
    assert not g0[free, :3].any() and np.all(g0[:, 3] == 7.0)
    assert np.array_equal(out0, out1.cpu().numpy())
    # force = NULL: observables only
    outn = dl.forces(dpos, None).cpu().numpy()
    assert np.array_equal(outn, out0)
    # out8 = NULL: forces only, a given `out` is left alone
    keep = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    f2 = to4(base, 7.0)
    assert dl.forces(dpos, f2, accumulate=False, out=keep, observables=False) is None
    assert np.array_equal(f2.cpu().numpy(), g0) and np.all(keep.cpu().numpy() == -1.0)
    # both NULL is refused
    import pse_amd
    with pytest.raises(pse_amd.PSEError, match="both null"):
        dl.forces(dpos, None, observables=False)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], c["pos"])
    dl.close()


@pytest.mark.parametrize("name", ["two_types", "duplicates", "graph", "star"])
def test_order_invariance_bit_for_bit(name):
    """A permuted list with reversed quadruples gives bit-identical forces and out8; so do two calls on equal inputs."""
    box = TILTED
    c = dr.graph_case(box, dr.HARMONIC, port()) if name == "graph" else dr.topology_case(name, box, dr.HARMONIC, port())
    n = len(c["pos"])
    eng = engine(box)
    dpos = to4(c["pos"])

    def run(dl):
        f = to4(np.zeros((n, 3)))
        o = dl.forces(dpos, f, accumulate=False).cpu().numpy()
        return o, f.cpu().numpy()

    a = dihedral_list(eng, c)
    o1, f1 = run(a)
    o2, f2 = run(a)
    assert np.array_equal(o1, o2) and np.array_equal(f1, f2)
    rng = np.random.default_rng(4)
    for trial in range(2):
        o = rng.permutation(len(c["quads"]))
        quads = c["quads"][o].copy()
        flip = rng.uniform(size=len(quads)) < 0.5
        quads[flip] = quads[flip, ::-1]
        assert flip.any() and not np.array_equal(quads, c["quads"])
        b = dihedral_list(eng, c, quads, None if c["types"] is None else c["types"][o])
        o3, f3 = run(b)
        assert np.array_equal(o1, o3) and np.array_equal(f1, f3)
        b.close()
    a.close()


@pytest.mark.parametrize("kind", ["harmonic", "opls"])
def test_coincident_members_do_nothing(kind):
    """A zero-length arm -- i at j, and l and k at images of k and j -- makes |m|^2 or |nn|^2 zero: nothing happens and nothing is
    counted; the one proper dihedral of the list acts."""
    box = TILTED
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.5, 2.5, 3.5], [1.0 + box[0], 2.0, 3.0], [0.5, 2.0, 3.9], [2.0, 1.0, 3.0]])
    quads = [[0, 1, 2, 4], [4, 2, 3, 1], [5, 1, 3, 2], [5, 2, 1, 4]]
    code = {"harmonic": dr.HARMONIC, "opls": dr.OPLS}[kind]
    dl = engine(box).dihedrals(quads, kinds=[kind], params=[dr.PARAMS[code]], n=6)
    ref, F = dr.dihedral_observables(pos, box, quads, None, [code], [dr.PARAMS[code]], port())
    assert ref[7] == 1 and not F[[0, 3]].any() and np.abs(F[[1, 2, 4, 5]]).max(axis=1).min() > 0.5
    f = to4(np.ones((6, 3)))
    out = dl.forces(to4(pos), f, accumulate=False).cpu().numpy()
    check_obs(out, ref, f"zero arm, {kind}")
    g = f.cpu().numpy()[:, :3]
    check_forces(g, F, f"zero arm, {kind}")
    assert not g[[0, 3]].any() and np.isfinite(out).all()
    dl.close()


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
def test_exactly_collinear_triples(box):
    """i, j, k collinear, j, k, l collinear, all four collinear, each with both kinds: the cross product is exactly zero, the result
    finite, nothing counted; the generic dihedral beside them acts."""
    c = dr.degenerate_case(box, port())
    assert c["degenerate"] == 6
    out, g = run_case(c, box, "degenerate")
    assert np.isfinite(out).all() and np.isfinite(g).all()
    assert out[7] == 2.0 and not g[:12, :3].any() and np.abs(g[12:16, :3]).max() > 0.1


def test_neighbour_list_is_untouched():
    """Dihedral calls between two mobility calls on the same positions: the second mobility call reuses the kept list exactly as it
    does without them, and the dihedral calls themselves neither build nor reuse."""
    import pse_amd
    box = TILTED
    c = dr.topology_case("chains", box, dr.HARMONIC, port())
    n = len(c["pos"])
    force = to4(np.random.default_rng(1).normal(size=(n, 3)))

    def stats(eng):
        b, r = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        assert eng._lib.pse_neighbor_stats(eng._h, None, ctypes.byref(b), ctypes.byref(r)) == 0
        return b.value, r.value

    counts = []
    for with_dihedrals in (False, True):
        eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3)
        dpos = to4(c["pos"])
        eng.mobility(dpos, force)
        before = stats(eng)
        if with_dihedrals:
            dl = dihedral_list(eng, c)
            f = to4(np.zeros((n, 3)))
            dl.forces(dpos, f, accumulate=False)
            dl.forces(dpos, f, accumulate=True, observables=False)
            assert stats(eng) == before
            check_forces(f.cpu().numpy()[:, :3], 2.0 * reference(c, box)[1], "between the mobility calls")
        eng.mobility(dpos, force)
        counts.append((before, stats(eng)))
        if with_dihedrals:
            dl.close()
        eng.close()
    print("(builds, reuses) after the first and the second mobility call, without / with dihedral calls:", counts)
    assert counts[0] == counts[1], counts
    assert sum(counts[1][1]) > sum(counts[1][0]) >= 1                      # the mobility calls do go through the list


def test_asynchronous_submission_into_a_log_row():
    """Four calls on four configurations, each into its own row of a (4, 8) tensor, read once at the end."""
    import torch
    box = TILTED
    eng = engine(box)
    cases = [dr.topology_case(name, box, dr.OPLS, port()) for name in ("chains", "ring", "star", "two_types")]
    lists = [dihedral_list(eng, c) for c in cases]
    dpos = [to4(c["pos"]) for c in cases]
    fs = [to4(np.zeros((dr.N_TOPOLOGY, 3))) for _ in cases]
    log = torch.full((4, 8), -1.0, dtype=torch.float64, device="cuda")
    for q in range(4):
        assert lists[q].forces(dpos[q], fs[q], accumulate=False, out=log[q]).data_ptr() == log[q].data_ptr()
    rows = log.cpu().numpy()                                              # the one read
    for q, c in enumerate(cases):
        ref, F = reference(c, box)
        check_obs(rows[q], ref, f"log row {q}")
        check_forces(fs[q].cpu().numpy()[:, :3], F, f"log row {q}")
    for dl in lists:
        dl.close()


def test_a_slab_rank_handle_takes_dihedral_calls():
    """The pass does not use the cell list, so a slab rank's handle (which orders only its own cells) gives the complete sums."""
    import pse_amd
    box = (40.0, 40.0, 40.0, 0.0)
    c = dr.topology_case("chains", box, dr.HARMONIC, port())
    eng = pse_amd.Engine(dr.N_TOPOLOGY, box, xi=0.5, error=1e-3, grid=(48, 48, 48), n_slabs=2, slab_rank=0)
    dl = dihedral_list(eng, c)
    f = to4(np.zeros((dr.N_TOPOLOGY, 3)))
    out = dl.forces(to4(c["pos"]), f, accumulate=False).cpu().numpy()
    ref, F = reference(c, box)
    assert np.all(dr.sines(c["pos"], box, c["quads"], port()) >= dr.SIN_MIN)      # (this box is not among the inputs validated on the CPU)
    check_obs(out, ref, "slab rank")
    check_forces(f.cpu().numpy()[:, :3], F, "slab rank")
    dl.close()
    eng.close()


def test_misuse_is_reported():
    """Raw C-ABI, as a C host would call it: every error return of pse_dihedrals_create and pse_dihedral_forces, with a message
    naming the value; the object then works after all the refusals."""
    import torch
    from pse_amd import _lib
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    eng = engine(CUBIC)
    h, n = eng._h, 64
    A = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)                # noqa: E731
    good_quads = u32([[0, 1, 2, 3], [1, 2, 3, 4], [5, 9, 7, 8]])
    good_params = np.array([[30.0, -1.0, 3.0, 0.7], [15.0, -8.0, 12.0, 5.0]])
    good = dict(h=h, n=n, nd=3, quads=good_quads, types=u32([0, 1, 0]), nt=2, kind=np.array([0, 1], dtype=np.int32), params=good_params)
    nan, inf = float("nan"), float("inf")

    def create(out="new", **kw):
        a = dict(good, **kw)
        b = ctypes.c_void_p(0xdead) if out == "new" else out
        par = None if a["params"] is None else np.ascontiguousarray(a["params"], dtype=np.float64)
        rc = lib.pse_dihedrals_create(a["h"], a["n"], a["nd"], A(a["quads"]), A(a["types"]), a["nt"], A(a["kind"]), A(par),
                                      None if b is None else ctypes.byref(b))
        return rc, b

    def refused(word, **kw):
        rc, b = create(**kw)
        assert rc == INVALID, (word, rc)
        assert msg() and word in msg(), (word, msg())
        assert b is None or not b.value                   # *out is null after a refusal

    def with_param(t, q, v):
        p = good_params.copy()
        p[t, q] = v
        return p

    refused("null handle", h=None)
    refused("null quads_host", quads=None)
    refused("null out", out=None)
    refused("null parameter array", kind=None)
    refused("null parameter array", params=None)
    refused("n = 0", n=0)
    refused(f"n = {dr.N_MAX + 1}", n=dr.N_MAX + 1)
    refused("ndihedrals = 0", nd=0)
    refused("ndihedrals = 268435457", nd=(1 << 28) + 1)
    for q in ([64, 9, 7, 8], [5, 64, 7, 8], [5, 9, 64, 8], [5, 9, 7, 64]):
        refused("(%d, %d, %d, %d) has an index >= n = 64" % tuple(q), quads=u32([[0, 1, 2, 3], [1, 2, 3, 4], q]))
    for q in ([7, 7, 3, 4], [7, 3, 7, 4], [7, 3, 4, 7], [3, 7, 7, 4], [3, 7, 4, 7], [3, 4, 7, 7]):
        refused("(%d, %d, %d, %d) has two equal members" % tuple(q), quads=u32([[0, 1, 2, 3], q, [5, 9, 7, 8]]))
    refused("ntypes = 0", nt=0)
    refused("ntypes = 65", nt=65)
    refused("ntypes = -1", nt=-1)
    refused("type 2", types=u32([0, 2, 0]))
    refused("type 1", types=u32([0, 1, 0]), nt=1)
    refused("kind 2", kind=np.array([0, 2], dtype=np.int32))
    refused("kind -1", kind=np.array([-1, 1], dtype=np.int32))
    for t in range(2):
        for q in range(4):
            refused("finite", params=with_param(t, q, nan))
            refused("finite", params=with_param(t, q, inf))
    refused("d = 0.5", params=with_param(0, 1, 0.5))
    refused("d = 0", params=with_param(0, 1, 0.0))
    refused("d = -2", params=with_param(0, 1, -2.0))
    refused("mult = 0", params=with_param(0, 2, 0.0))
    refused("mult = 7", params=with_param(0, 2, 7.0))
    refused("mult = 2.5", params=with_param(0, 2, 2.5))
    refused("mult = -1", params=with_param(0, 2, -1.0))
    # a negative k, any phi0, mult = 6, d = +1, OPLS constants of any sign and types = NULL are legal
    rc, b = create(types=None, params=np.array([[-1.0, 1.0, 6.0, -9.0], [0.0, -1.0, 0.5, 7.0]]))
    assert rc == 0 and b.value, msg()
    assert lib.pse_dihedrals_destroy(b) == 0
    rc, b = create(types=None)                                          # ... and the object works after all the refusals
    assert rc == 0 and b.value, msg()
    pos = random_points(n, CUBIC, seed=2) * 0.1                       # a cluster: every arm is short
    assert np.all(dr.sines(pos, CUBIC, good_quads, port()) >= dr.SIN_MIN)
    dpos, dF = to4(pos), to4(np.zeros((n, 3)), 5.0)
    out8 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    call = lib.pse_dihedral_forces
    for word, args in (("null dihedral object", (None, P(dpos), P(dF), 0, P(out8))), ("null pos", (b, None, P(dF), 0, P(out8))),
                       ("both null", (b, P(dpos), None, 0, None))):
        assert call(*args) == INVALID and word in msg(), (word, msg())
    torch.cuda.synchronize()
    assert np.all(out8.cpu().numpy() == -1.0) and np.array_equal(dF.cpu().numpy(), to4(np.zeros((n, 3)), 5.0).cpu().numpy())
    assert call(b, P(dpos), P(dF), 0, P(out8)) == 0, msg()
    ref, F = dr.dihedral_observables(pos, CUBIC, good_quads, None, [0, 1], good_params, port())
    check_obs(out8.cpu().numpy(), ref, "after the refused calls")
    check_forces(dF.cpu().numpy()[:, :3], F, "after the refused calls")
    assert lib.pse_dihedrals_destroy(b) == 0 and lib.pse_dihedrals_destroy(None) == 0


def test_engine_wrapper_checks_its_arguments_and_lifetime():
    import pse_amd
    eng = pse_amd.Engine(64, CUBIC, xi=0.5, error=1e-3)
    for bad in ([], [[0, 1, 2]], [[0, 1, 2, 3, 4]], [[0.5, 1.0, 2.0, 3.0]], [[-1, 2, 3, 4]]):
        with pytest.raises(ValueError):
            eng.dihedrals(bad)
    with pytest.raises(ValueError):
        eng.dihedrals([[0, 1, 2, 3]], types=[0, 1])
    with pytest.raises(ValueError):
        eng.dihedrals([[0, 1, 2, 3]], kinds=["cosine"])
    with pytest.raises(ValueError):
        eng.dihedrals([[0, 1, 2, 3]], kinds=["harmonic", "opls"], params=[(1.0, 1.0, 1.0, 0.0)])
    with pytest.raises(ValueError):
        eng.dihedrals([[0, 1, 2, 3]], kinds=["harmonic"], params=[(1.0, 1.0, 1.0)])
    with pytest.raises(pse_amd.PSEError, match="n_max"):
        eng.dihedrals([[0, 1, 2, 3]], n=65)
    with pytest.raises(pse_amd.PSEError, match="mult"):
        eng.dihedrals([[0, 1, 2, 3]], params=[(1.0, 1.0, 7.0, 0.0)])
    dl = eng.dihedrals([[0, 1, 2, 3], [1, 2, 3, 4]], kinds="opls", params=(1.0, 2.0, 3.0, 4.0))   # one type: a scalar kind and one 4-tuple; n defaults to n_max
    assert dl.n == 64 and dl.ndihedrals == 2
    with pytest.raises(ValueError):
        dl.forces(to4(np.zeros((10, 3))), None)                            # fewer rows than the topology has particles
    keep = eng.dihedrals([[3, 4, 5, 6]])                                    # the defaults: harmonic, k = 1, d = 1, mult = 1, phi0 = 0
    dl.close(); dl.close()                                                  # closing twice is harmless
    with pytest.raises(ValueError, match="closed"):
        dl.forces(to4(np.zeros((64, 3))), None)
    eng.close()                                                             # frees `keep`'s device object with the handle ...
    keep.close()                                                            # ... which the wrapper knows


def _sheared_system(pos, box, dt):
    from pse_amd import integrate, shear_function, variant
    from pse_amd.system import System
    s = System(pos, box, dt=dt)
    ff = shear_function.steady(dt=dt, shear_rate=2.0)
    s.box_tilt_variant = variant.shear_variant(ff, 2000, max_strain=0.5)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3, function_form=ff)
    return s, pse


class _Snapshots:
    """Analyzer: positions and box of the sample steps (analyzers run before the forces of the same step)."""

    def __init__(self, system, period):
        self.system, self.period, self.saved = system, period, {}

    def analyze(self, timestep):
        if timestep % self.period == 0:
            self.saved[timestep] = (self.system.pos.clone(), self.system.box)


@pytest.fixture
def restored_context():
    """A System registers itself as the current simulation context, and a shear function made later takes its zero from that
    context's time step: put back what was there, so that the 20 steps run here are not some later test's time origin."""
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


def test_dihedrals_provider_with_bonds_and_angles_in_a_sheared_run_with_a_stress_log(restored_context):
    """forces.Dihedrals (a harmonic and an OPLS type) beside forces.Bonds and forces.Angles through 20 steps of a sheared System.run
    with a StressLog at period 5: each sampled row is the reference on the positions an analyzer saved on that step, in the box of
    that step."""
    import torch
    from pse_amd import forces
    box = TILTED[:3] + (0.0,)
    c = dr.topology_case("two_types", box, dr.HARMONIC, port())
    kinds = [KIND_NAMES[q] for q in c["kinds"]]
    pairs = np.unique(np.sort(np.vstack([c["quads"][:, :2], c["quads"][:, 1:3], c["quads"][:, 2:]]), axis=1), axis=0)   # the bonds along the four chains
    triples = np.unique(np.vstack([c["quads"][:, :3], c["quads"][:, 1:]]), axis=0)                                     # ... and their angles
    assert len(pairs) == 4 * 49 and len(triples) == 4 * 48
    s, pse = _sheared_system(c["pos"], box, dt=1e-3)
    vol = box[0] * box[1] * box[2]
    plain = forces.Dihedrals(pse, c["quads"], kind=kinds, params=c["params"], types=c["types"])
    ref, F = reference(c, box)
    plain.compute(0)                                                       # virial=False: forces only
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "Dihedrals, virial=False")
    assert plain.kind == tuple(kinds) and plain.params == tuple(tuple(float(v) for v in p) for p in c["params"])
    with pytest.raises(RuntimeError, match="Dihedrals"):
        plain.energy
    with pytest.raises(ValueError, match="Dihedrals"):
        forces.StressLog(plain, 1, 4)
    s.forces.remove(plain)
    for bad in (dict(kind="cosine"), dict(kind=["harmonic", "opls"], params=[(1.0, 1.0, 1.0, 0.0)] * 3), dict(types=[0]),
                dict(params=(1.0, 1.0, 1.0)), dict(params=1.0)):
        with pytest.raises(ValueError):
            forces.Dihedrals(pse, c["quads"], **bad)
    with pytest.raises(ValueError):
        forces.Dihedrals(pse, np.zeros((0, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        forces.Dihedrals(pse, c["quads"][:, :3])
    with pytest.raises(ValueError):                                        # an index that would wrap to a valid one as uint32
        forces.Dihedrals(pse, [[0, 1, 2, 2 ** 32 + 3]])
    with pytest.raises(ValueError):
        forces.Dihedrals(pse, c["quads"], kind=kinds, params=c["params"], types=c["types"] + 2 ** 32)
    assert s.forces == []
    one = forces.Dihedrals(pse, c["quads"], kind="opls", params=dr.PARAMS[dr.OPLS])      # a scalar kind and one 4-tuple: one type
    assert one.kind == ("opls",) and one.params == (dr.PARAMS[dr.OPLS],)
    s.forces.remove(one)
    bonds = forces.Bonds(pse, pairs, kind="harmonic", k=br.K_H, r0=1.1, virial=True)
    angles = forces.Angles(pse, triples, kind="cosinesq", k=ar.K_C, theta0=ar.TH0_C, virial=True)
    dihedrals = forces.Dihedrals(pse, c["quads"], kind=kinds, params=c["params"], types=c["types"], virial=True)
    s.net_force.zero_()
    dihedrals.compute(0)
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    W = np.array([[ref[1], ref[2], ref[3]], [ref[2], ref[4], ref[5]], [ref[3], ref[5], ref[6]]])
    assert abs(dihedrals.energy - ref[0]) <= tol and dihedrals.ndihedrals == dihedrals.npairs == ref[7] == len(c["quads"])
    assert np.abs(dihedrals.virial - W).max() <= tol and np.abs(dihedrals.stress() + W / vol).max() <= tol / vol
    assert abs(np.trace(dihedrals.virial)) <= tol
    log = forces.StressLog(dihedrals, period=5, capacity=8)
    alog = forces.StressLog(angles, period=5, capacity=8)
    blog = forces.StressLog(bonds, period=5, capacity=8)
    snap = _Snapshots(s, 5)
    s.analyzers.append(snap)
    s.run(20)
    tab, atab, btab = log.table(), alog.table(), blog.table()
    assert tab.shape == (4, 10) and list(tab[:, 0]) == [0.0, 5.0, 10.0, 15.0] and sorted(snap.saved) == [0, 5, 10, 15]
    assert tab[0, 1] == 0.0 and np.all(np.diff(tab[:, 1]) > 0.0)           # the box tilt of the sample steps: sheared
    moved = 0.0
    for row, arow, brow in zip(tab, atab, btab):
        p, b = snap.saved[int(row[0])]
        p = p.cpu().numpy()[:, :3]
        assert b[3] == row[1]
        assert np.all(dr.sines(p, b, c["quads"], port()) >= dr.SIN_MIN)                         # still where the bound holds
        r8, _ = reference(c, b, p)
        t8 = 1e-11 * max(1.0, np.abs(r8).max())
        print(f"step {int(row[0])}: xy {row[1]:.4f}, U {row[2]:.6g} / {r8[0]:.6g}, sigma_xy {row[4]:.6g} / {-r8[2] / vol:.6g}")
        assert row[9] == r8[7] == len(c["quads"])
        assert abs(row[2] - r8[0]) <= t8 and np.abs(row[3:9] + r8[1:7] / vol).max() <= t8 / vol
        a8, _ = ar.angle_observables(p, b, triples, None, [ar.COSINESQ], [ar.K_C], [ar.TH0_C], port())      # the angles beside them ...
        ta = 1e-11 * max(1.0, np.abs(a8).max())
        assert arow[9] == a8[7] == len(triples) and abs(arow[2] - a8[0]) <= ta and np.abs(arow[3:9] + a8[1:7] / vol).max() <= ta / vol
        b8, _, over = br.bond_observables(p, b, pairs, None, [br.HARMONIC], [br.K_H], [1.1], port())        # ... and the bonds
        tb = 1e-11 * max(1.0, np.abs(b8).max())
        assert over == 0 and brow[9] == b8[7] == len(pairs) and abs(brow[2] - b8[0]) <= tb and np.abs(brow[3:9] + b8[1:7] / vol).max() <= tb / vol
        moved = max(moved, np.abs(p - c["pos"]).max())
    assert moved > 1e-3 and torch.isfinite(s.pos).all()


def test_topology_builder_of_the_helical_example():
    """examples/helical_polymers.py build_topology at 12 chains of 20: chain-ordered beads, one bond per neighbouring pair, one angle
    per inner bead and one dihedral per four beads in a row, none from chain to chain; every dihedral within the example's jitter of
    its PHI0 in the convention of the reference -- so the sign the example prescribes is the sign the device uses -- and its mean
    dihedral cosine against the one computed here; the device takes the topology as it is, with the example's parameters."""
    spec = importlib.util.spec_from_file_location("helical_polymers", os.path.join(ROOT, "examples", "helical_polymers.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    box = TILTED
    nchains, beads, b = 12, 20, 2.0
    pos, pairs, triples, quads = ex.build_topology(nchains, beads, box, b, seed=5)
    assert pos.shape == (nchains * beads, 3) and pairs.shape == (nchains * (beads - 1), 2) and triples.shape == (nchains * (beads - 2), 3)
    assert quads.shape == (nchains * (beads - 3), 4)
    assert np.all(pairs[:, 1] == pairs[:, 0] + 1) and not np.any(pairs[:, 1] % beads == 0)          # no bond from chain to chain
    assert np.all(np.diff(triples, axis=1) == 1) and not np.any(triples[:, 1:] % beads == 0)        # no angle from chain to chain
    assert np.all(np.diff(quads, axis=1) == 1) and not np.any(quads[:, 1:] % beads == 0)            # no dihedral from chain to chain
    assert np.array_equal(port().wrap(pos, np.zeros(pos.shape, dtype=np.int64), box)[0], pos)         # inside the tilted cell
    assert np.abs(dr.arm_lengths(pos, box, quads, port()) - b).max() < 1e-12
    params = (ex.K_TORSION, -1.0, 1.0, ex.PHI0)
    q = dr.dihedral_terms(pos, box, quads, None, [dr.HARMONIC], [params], port())
    assert np.abs(q["phi"] - ex.PHI0).max() <= ex.JITTER + 1e-12 and np.ptp(q["phi"]) > ex.JITTER
    assert abs(ex.mean_dihedral_cosine(pos, box, quads) - np.cos(q["phi"] - ex.PHI0).mean()) < 1e-12
    th = np.arcsin(ar.sines(pos, box, triples, port()))                                               # THETA0 = 1.9 > pi/2: theta = pi - asin
    assert np.abs(np.pi - th - ex.THETA0).max() <= ex.JITTER + 1e-9
    assert np.all(dr.sines(pos, box, quads, port()) >= dr.SIN_MIN)
    # ... and on the device, with the example's harmonic dihedral (phi0 != 0)
    dl = engine(box).dihedrals(quads, kinds="harmonic", params=params, n=len(pos))
    f = to4(np.zeros((len(pos), 3)))
    out = dl.forces(to4(pos), f, accumulate=False).cpu().numpy()
    ref, F = dr.dihedral_observables(pos, box, quads, None, [dr.HARMONIC], [params], port())
    check_obs(out, ref, "example topology")
    check_forces(f.cpu().numpy()[:, :3], F, "example topology")
    assert out[7] == len(quads) and 0.0 < ref[0] < 0.5 * ex.K_TORSION * (1.0 - np.cos(ex.JITTER)) * len(quads)
    dl.close()
