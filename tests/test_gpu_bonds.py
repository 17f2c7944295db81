"""GPU tests of the bonded forces (pse_bonds_create / pse_bond_forces / pse_bonds_overstretched): harmonic and FENE bonds against
the NumPy reference of tests/bond_ref.py (validated on the CPU by tests/test_bond_reference.py, which also asserts that the FENE
bonds of the inputs used here have (r/r0)^2 <= 0.9, or r/r0 >= 1.05 where they are meant to be overstretched), against the existing
harmonic repulsion, bit-exact invariance under the order of the list, the call forms, the error returns, and the host UI on top
(Engine.bonds, forces.Bonds with a StressLog, the topology builder of examples/polymer_solution.py).

Bound: the project's own for these passes (tests/test_gpu_pair_virial.py), 1e-11 max(1, max |ref|), the eight observables together
and the forces together; nbonds and the overstretched count must match exactly."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

import bond_ref as br
from conftest import to4
from pair_virial_ref import pair_observables, pair_terms, random_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBIC, TILTED = br.BOXES
BOX_IDS = ["cubic", "tilted"]
KIND_IDS = ["harmonic", "fene"]
INVALID = -1


def port():
    from oracle import pse_port
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(br.N_MAX, box, xi=0.5, error=1e-3)


def check_obs(got, ref, what=""):
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"{what}: max |obs - ref| = {err:.3e} (bound {tol:.3e}), nbonds {got[7]:.0f} / {ref[7]:.0f}, U {ref[0]:.6g}")
    assert got[7] == ref[7], (what, got[7], ref[7])
    assert err <= tol, (what, got, ref)


def check_forces(got, F, what=""):
    tol = 1e-11 * max(1.0, np.abs(F).max())
    err = np.abs(got - F).max()
    print(f"{what}: max |F - ref| = {err:.3e} (bound {tol:.3e}), max |F| {np.abs(F).max():.6g}")
    assert err <= tol, (what, err, tol)


def reference(c, box):
    return br.bond_observables(c["pos"], box, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], port())


def bond_list(eng, c, pairs=None, types="case"):
    return eng.bonds(c["pairs"] if pairs is None else pairs, c["types"] if isinstance(types, str) else types, kinds=c["kinds"], k=c["k"],
                     r0=c["r0"], n=len(c["pos"]))


def run_case(c, box, what):
    """accumulate = 0 on a preset force array: observables, forces, kept w, overstretched count."""
    n = len(c["pos"])
    ref, F, over = reference(c, box)
    assert ref[7] == len(c["pairs"]) - c["n_over"] and over == c["n_over"]
    bl = bond_list(engine(box), c)
    f = to4(np.random.default_rng(5).normal(size=(n, 3)), 3.0)
    out = bl.forces(to4(c["pos"]), f, accumulate=False).cpu().numpy()
    check_obs(out, ref, what)
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, what)
    assert np.all(g[:, 3] == 3.0)
    assert bl.overstretched == over
    bl.close()
    return out, g


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
@pytest.mark.parametrize("kind", [br.HARMONIC, br.FENE], ids=KIND_IDS)
@pytest.mark.parametrize("n", br.ROW_COUNTS)
def test_row_counts(n, kind, box):
    """One chain of n beads: a partial last wave, a full one, one lane of the next; the same for the 256-thread workgroup (257: a
    second workgroup of one thread; 513 = n_max: a third)."""
    run_case(br.chain_case(n, box, kind, port()), box, f"chain n={n} kind={kind}")


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
@pytest.mark.parametrize("kind", [br.HARMONIC, br.FENE], ids=KIND_IDS)
@pytest.mark.parametrize("name", br.TOPOLOGIES + ("graph",))
def test_topologies(name, kind, box):
    c = br.graph_case(box, kind, port()) if name == "graph" else br.topology_case(name, box, kind, port())
    assert len(c["pos"]) == br.N_TOPOLOGY
    out, g = run_case(c, box, f"{name} kind={kind}")
    unbonded = np.setdiff1d(np.arange(br.N_TOPOLOGY), np.unique(c["pairs"]))
    assert len(unbonded) > 0 and not g[unbonded, :3].any()            # accumulate = 0 zeroes the rows without bonds
    if name == "star":
        assert np.bincount(c["pairs"].ravel())[0] == 40
    if name == "duplicates":                                          # every copy acts: more bonds than distinct pairs
        assert out[7] == len(c["pairs"]) > len(np.unique(np.sort(c["pairs"], axis=1), axis=0))
    if name == "two_types":
        assert sorted(c["kinds"]) == [br.HARMONIC, br.FENE] and set(c["types"]) == {0, 1}


def test_call_forms():
    """accumulate 0 and 1, force = NULL, out8 = NULL; an unbonded row keeps its preset value bit for bit under accumulate = 1 and
    becomes zero under accumulate = 0; w survives in both."""
    import torch
    box = TILTED
    c = br.topology_case("chains", box, br.FENE, port())
    n = len(c["pos"])
    ref, F, _ = reference(c, box)
    bl = bond_list(engine(box), c)
    dpos = to4(c["pos"])
    base = np.random.default_rng(6).normal(size=(n, 3))
    unbonded = np.setdiff1d(np.arange(n), np.unique(c["pairs"]))
    assert len(unbonded) == 60
    # accumulate = 1
    f1 = to4(base, 7.0)
    out1 = bl.forces(dpos, f1, accumulate=True)
    assert out1.shape == (8,) and out1.is_cuda and out1.dtype == torch.float64
    check_obs(out1.cpu().numpy(), ref, "accumulate=1")
    g1 = f1.cpu().numpy()
    check_forces(g1[:, :3], F + base, "accumulate=1")
    assert np.array_equal(g1[unbonded, :3], to4(base).cpu().numpy()[unbonded, :3]) and np.all(g1[:, 3] == 7.0)
    # accumulate = 0
    f0 = to4(base, 7.0)
    out0 = bl.forces(dpos, f0, accumulate=False).cpu().numpy()
    g0 = f0.cpu().numpy()
    check_forces(g0[:, :3], F, "accumulate=0")
    assert not g0[unbonded, :3].any() and np.all(g0[:, 3] == 7.0)
    assert np.array_equal(out0, out1.cpu().numpy())
    # force = NULL: observables only
    outn = bl.forces(dpos, None).cpu().numpy()
    assert np.array_equal(outn, out0)
    # out8 = NULL: forces only, a given `out` is left alone
    keep = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    f2 = to4(base, 7.0)
    assert bl.forces(dpos, f2, accumulate=False, out=keep, observables=False) is None
    assert np.array_equal(f2.cpu().numpy(), g0) and np.all(keep.cpu().numpy() == -1.0)
    # both NULL is refused
    import pse_amd
    with pytest.raises(pse_amd.PSEError, match="both null"):
        bl.forces(dpos, None, observables=False)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], c["pos"])
    bl.close()


@pytest.mark.parametrize("box", [TILTED[:3] + (0.0,), TILTED], ids=["straight", "tilted"])
def test_harmonic_bonds_agree_with_the_repulsion_pass(box):
    """Harmonic bonds with r0 = sigma on the pairs with r < sigma of a random configuration are the harmonic repulsion: forces and
    the eight doubles against pse_pair_repulsion_virial on the same engine."""
    k, sigma, n = 40.0, 2.0, 300
    pos = random_points(n, box, seed=11)
    i, j, d, c, r = pair_terms(pos, box, k, sigma, port())
    assert len(i) > 20
    eng = engine(box)
    dpos = to4(pos)
    fr, fb = to4(np.zeros((n, 3))), to4(np.zeros((n, 3)))
    rep = eng.pair_repulsion_virial(dpos, fr, k, sigma, accumulate=False).cpu().numpy()
    bl = eng.bonds(np.stack([i, j], axis=1), kinds=["harmonic"], k=[k], r0=[sigma], n=n)
    got = bl.forces(dpos, fb, accumulate=False).cpu().numpy()
    ref, F = pair_observables(pos, box, k, sigma, port())
    check_obs(got, rep, "bonds against pse_pair_repulsion_virial")
    check_obs(got, ref, "bonds against the pair reference")
    check_forces(fb.cpu().numpy()[:, :3], fr.cpu().numpy()[:, :3], "bonds against pse_pair_repulsion_virial")
    check_forces(fb.cpu().numpy()[:, :3], F, "bonds against the pair reference")
    assert bl.overstretched == 0
    bl.close()


@pytest.mark.parametrize("name", ["two_types", "duplicates", "graph"])
def test_order_invariance_bit_for_bit(name):
    """A permuted list with swapped endpoints gives bit-identical forces and out8; so do two calls on equal inputs."""
    box = TILTED
    c = br.graph_case(box, br.FENE, port()) if name == "graph" else br.topology_case(name, box, br.FENE, port())
    n = len(c["pos"])
    eng = engine(box)
    dpos = to4(c["pos"])

    def run(bl):
        f = to4(np.zeros((n, 3)))
        o = bl.forces(dpos, f, accumulate=False).cpu().numpy()
        return o, f.cpu().numpy()

    a = bond_list(eng, c)
    o1, f1 = run(a)
    o2, f2 = run(a)
    assert np.array_equal(o1, o2) and np.array_equal(f1, f2)
    rng = np.random.default_rng(4)
    for trial in range(2):
        o = rng.permutation(len(c["pairs"]))
        pairs = c["pairs"][o].copy()
        flip = rng.uniform(size=len(pairs)) < 0.5
        pairs[flip] = pairs[flip, ::-1]
        assert flip.any() and not np.array_equal(pairs, c["pairs"])
        b = bond_list(eng, c, pairs, None if c["types"] is None else c["types"][o])
        o3, f3 = run(b)
        assert np.array_equal(o1, o3) and np.array_equal(f1, f3)
        b.close()
    a.close()


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
def test_fene_overstretch_is_left_out_and_counted(box):
    c = br.overstretch_case(box, port())
    n = len(c["pos"])
    ref, F, over = reference(c, box)
    assert over == 3 and ref[7] == len(c["pairs"]) - 3
    bl = bond_list(engine(box), c)
    dpos = to4(c["pos"])
    f = to4(np.zeros((n, 3)))
    out = bl.forces(dpos, f, accumulate=False).cpu().numpy()
    check_obs(out, ref, "overstretched chain")
    check_forces(f.cpu().numpy()[:, :3], F, "overstretched chain")
    assert np.isfinite(out).all() and np.isfinite(f.cpu().numpy()).all()
    assert bl.overstretched == 3
    bl.forces(dpos, f, accumulate=False, observables=False)          # the forces-only kernel counts too
    assert bl.overstretched == 6
    # another object on the same handle has its own counter
    other = bond_list(engine(box), br.chain_case(63, box, br.FENE, port()))
    assert other.overstretched == 0
    other.close()
    bl.close()


def test_coincident_endpoints_do_nothing():
    box = TILTED
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.5, 2.5, 3.5], [1.0 + box[0], 2.0, 3.0]])   # 3 is an image of 0: r == 0 too
    pairs = [[0, 1], [1, 2], [3, 1]]
    for kind in ("harmonic", "fene"):
        bl = engine(box).bonds(pairs, kinds=[kind], k=[30.0], r0=[1.5], n=4)
        ref, F, over = br.bond_observables(pos, box, pairs, None, [{"harmonic": br.HARMONIC, "fene": br.FENE}[kind]], [30.0], [1.5], port())
        assert ref[7] == 1 and over == 0
        f = to4(np.zeros((4, 3)))
        out = bl.forces(to4(pos), f, accumulate=False).cpu().numpy()
        check_obs(out, ref, f"r == 0, {kind}")
        check_forces(f.cpu().numpy()[:, :3], F, f"r == 0, {kind}")
        assert bl.overstretched == 0
        bl.close()


def test_neighbour_list_is_untouched():
    """Bond calls between two mobility calls on the same positions: the second mobility call reuses the kept list exactly as it does
    without them, and the bond calls themselves neither build nor reuse."""
    import pse_amd
    box = TILTED
    c = br.topology_case("chains", box, br.HARMONIC, port())
    n = len(c["pos"])
    force = to4(np.random.default_rng(1).normal(size=(n, 3)))

    def stats(eng):
        b, r = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        assert eng._lib.pse_neighbor_stats(eng._h, None, ctypes.byref(b), ctypes.byref(r)) == 0
        return b.value, r.value

    counts = []
    for with_bonds in (False, True):
        eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3)
        dpos = to4(c["pos"])
        eng.mobility(dpos, force)
        before = stats(eng)
        if with_bonds:
            bl = bond_list(eng, c)
            f = to4(np.zeros((n, 3)))
            bl.forces(dpos, f, accumulate=False)
            bl.forces(dpos, f, accumulate=True, observables=False)
            assert stats(eng) == before
            check_forces(f.cpu().numpy()[:, :3], 2.0 * reference(c, box)[1], "between the mobility calls")
        eng.mobility(dpos, force)
        counts.append((before, stats(eng)))
        if with_bonds:
            bl.close()
        eng.close()
    print("(builds, reuses) after the first and the second mobility call, without / with bond calls:", counts)
    assert counts[0] == counts[1], counts
    assert sum(counts[1][1]) > sum(counts[1][0]) >= 1                      # the mobility calls do go through the list


def test_asynchronous_submission_into_a_log_row():
    """Four calls on four configurations, each into its own row of a (4, 8) tensor, read once at the end."""
    import torch
    box = TILTED
    eng = engine(box)
    cases = [br.topology_case(name, box, br.FENE, port()) for name in ("chains", "ring", "star", "two_types")]
    lists = [bond_list(eng, c) for c in cases]
    dpos = [to4(c["pos"]) for c in cases]
    fs = [to4(np.zeros((br.N_TOPOLOGY, 3))) for _ in cases]
    log = torch.full((4, 8), -1.0, dtype=torch.float64, device="cuda")
    for q in range(4):
        assert lists[q].forces(dpos[q], fs[q], accumulate=False, out=log[q]).data_ptr() == log[q].data_ptr()
    rows = log.cpu().numpy()                                              # the one read
    for q, c in enumerate(cases):
        ref, F, _ = reference(c, box)
        check_obs(rows[q], ref, f"log row {q}")
        check_forces(fs[q].cpu().numpy()[:, :3], F, f"log row {q}")
    for bl in lists:
        bl.close()


def test_a_slab_rank_handle_takes_bond_calls():
    """The pass does not use the cell list, so a slab rank's handle (which orders only its own cells) gives the complete sums."""
    import pse_amd
    box = (40.0, 40.0, 40.0, 0.0)
    c = br.topology_case("chains", box, br.FENE, port())
    eng = pse_amd.Engine(br.N_TOPOLOGY, box, xi=0.5, error=1e-3, grid=(48, 48, 48), n_slabs=2, slab_rank=0)
    bl = bond_list(eng, c)
    f = to4(np.zeros((br.N_TOPOLOGY, 3)))
    out = bl.forces(to4(c["pos"]), f, accumulate=False).cpu().numpy()
    ref, F, _ = reference(c, box)
    check_obs(out, ref, "slab rank")
    check_forces(f.cpu().numpy()[:, :3], F, "slab rank")
    bl.close()
    eng.close()


def test_misuse_is_reported():
    """Raw C-ABI, as a C host would call it: every error return of pse_bonds_create, with a message naming the value."""
    import torch
    from pse_amd import _lib
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    eng = engine(CUBIC)
    h, n = eng._h, 64
    A = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)                # noqa: E731
    good_pairs = u32([[0, 1], [1, 2], [5, 9]])
    good = dict(h=h, n=n, nb=3, pairs=good_pairs, types=u32([0, 1, 0]), nt=2, kind=np.array([0, 1], dtype=np.int32),
                k=np.array([30.0, 20.0]), r0=np.array([1.0, 1.5]))
    nan, inf = float("nan"), float("inf")

    def create(out="new", **kw):
        a = dict(good, **kw)
        b = ctypes.c_void_p(0xdead) if out == "new" else out
        rc = lib.pse_bonds_create(a["h"], a["n"], a["nb"], A(a["pairs"]), A(a["types"]), a["nt"], A(a["kind"]), A(a["k"]), A(a["r0"]),
                                  None if b is None else ctypes.byref(b))
        return rc, b

    def refused(word, **kw):
        rc, b = create(**kw)
        assert rc == INVALID, (word, rc)
        assert msg() and word in msg(), (word, msg())
        assert b is None or not b.value                   # *out is null after a refusal

    refused("null handle", h=None)
    refused("null pairs_host", pairs=None)
    refused("null out", out=None)
    refused("null parameter array", kind=None)
    refused("null parameter array", k=None)
    refused("null parameter array", r0=None)
    refused("n = 0", n=0)
    refused(f"n = {br.N_MAX + 1}", n=br.N_MAX + 1)
    refused("nbonds = 0", nb=0)
    refused("nbonds = 1073741825", nb=(1 << 30) + 1)
    refused("(5, 64)", pairs=u32([[0, 1], [1, 2], [5, 64]]))
    refused("(64, 1)", pairs=u32([[0, 1], [64, 1], [5, 9]]))
    refused("particle 7 to itself", pairs=u32([[0, 1], [7, 7], [5, 9]]))
    refused("ntypes = 0", nt=0)
    refused("ntypes = 65", nt=65)
    refused("ntypes = -1", nt=-1)
    refused("type 2", types=u32([0, 2, 0]))
    refused("type 1", types=u32([0, 1, 0]), nt=1)
    refused("kind 2", kind=np.array([0, 2], dtype=np.int32))
    refused("kind -1", kind=np.array([-1, 1], dtype=np.int32))
    refused("finite", k=np.array([nan, 20.0]))
    refused("finite", k=np.array([30.0, inf]))
    refused("finite", r0=np.array([nan, 1.5]))
    refused("finite", r0=np.array([1.0, inf]))
    refused("r0 = -0.5", r0=np.array([-0.5, 1.5]))
    refused("FENE type 1", r0=np.array([1.0, 0.0]))
    # a harmonic r0 = 0 and types = NULL are legal; the object works after all the refusals
    rc, b = create(types=None, r0=np.array([0.0, 1.5]))
    assert rc == 0 and b.value, msg()
    pos = random_points(n, CUBIC, seed=2) * 0.1                       # a cluster: every bond is short
    dpos, dF = to4(pos), to4(np.zeros((n, 3)), 5.0)
    out8 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    call = lib.pse_bond_forces
    for word, args in (("null bond object", (None, P(dpos), P(dF), 0, P(out8))), ("null pos", (b, None, P(dF), 0, P(out8))),
                       ("both null", (b, P(dpos), None, 0, None))):
        assert call(*args) == INVALID and word in msg(), (word, msg())
    cnt = ctypes.c_ulonglong(99)
    assert lib.pse_bonds_overstretched(None, ctypes.byref(cnt)) == INVALID and "null" in msg()
    assert lib.pse_bonds_overstretched(b, None) == INVALID and "null" in msg()
    torch.cuda.synchronize()
    assert np.all(out8.cpu().numpy() == -1.0) and np.array_equal(dF.cpu().numpy(), to4(np.zeros((n, 3)), 5.0).cpu().numpy())
    assert call(b, P(dpos), P(dF), 0, P(out8)) == 0, msg()
    ref, F, over = br.bond_observables(pos, CUBIC, good_pairs, None, [0, 1], [30.0, 20.0], [0.0, 1.5], port())
    check_obs(out8.cpu().numpy(), ref, "after the refused calls")
    check_forces(dF.cpu().numpy()[:, :3], F, "after the refused calls")
    assert lib.pse_bonds_overstretched(b, ctypes.byref(cnt)) == 0 and cnt.value == 0
    assert lib.pse_bonds_destroy(b) == 0 and lib.pse_bonds_destroy(None) == 0


def test_engine_wrapper_checks_its_arguments_and_lifetime():
    import pse_amd
    eng = pse_amd.Engine(64, CUBIC, xi=0.5, error=1e-3)
    for bad in ([], [[0, 1, 2]], [[0.5, 1.0]], [[-1, 2]]):
        with pytest.raises(ValueError):
            eng.bonds(bad)
    with pytest.raises(ValueError):
        eng.bonds([[0, 1]], types=[0, 1])
    with pytest.raises(ValueError):
        eng.bonds([[0, 1]], kinds=["morse"])
    with pytest.raises(ValueError):
        eng.bonds([[0, 1]], kinds=["harmonic", "fene"], k=[1.0], r0=[1.0, 1.0])
    with pytest.raises(pse_amd.PSEError, match="n_max"):
        eng.bonds([[0, 1]], n=65)
    bl = eng.bonds([[0, 1], [1, 2]], kinds="fene", k=30.0, r0=1.5)         # scalars for a single type; n defaults to n_max
    assert bl.n == 64 and bl.nbonds == 2
    with pytest.raises(ValueError):
        bl.forces(to4(np.zeros((10, 3))), None)                            # fewer rows than the topology has particles
    keep = eng.bonds([[3, 4]])
    bl.close(); bl.close()                                                  # closing twice is harmless
    with pytest.raises(ValueError, match="closed"):
        bl.forces(to4(np.zeros((64, 3))), None)
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


def test_bonds_provider_in_a_sheared_run_with_a_stress_log(restored_context):
    """forces.Bonds (a harmonic and a FENE type) through 20 steps of a sheared System.run with a StressLog at period 5: each sampled
    row is the reference on the positions an analyzer saved on that step, in the box of that step."""
    import torch
    from pse_amd import forces
    box = TILTED[:3] + (0.0,)
    c = br.topology_case("two_types", box, br.HARMONIC, port())
    kinds = ["harmonic" if q == br.HARMONIC else "fene" for q in c["kinds"]]
    s, pse = _sheared_system(c["pos"], box, dt=1e-3)
    vol = box[0] * box[1] * box[2]
    plain = forces.Bonds(pse, c["pairs"], kind=kinds, k=c["k"], r0=c["r0"], types=c["types"])
    ref, F, _ = reference(c, box)
    plain.compute(0)                                                       # virial=False: forces only
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "Bonds, virial=False")
    with pytest.raises(RuntimeError, match="Bonds"):
        plain.energy
    with pytest.raises(ValueError, match="Bonds"):
        forces.StressLog(plain, 1, 4)
    s.forces.remove(plain)
    for bad in (dict(kind="morse"), dict(kind=["harmonic", "fene"], k=[1.0, 2.0, 3.0]), dict(types=[0])):
        with pytest.raises(ValueError):
            forces.Bonds(pse, c["pairs"], **bad)
    with pytest.raises(ValueError):
        forces.Bonds(pse, np.zeros((0, 2), dtype=np.int64))
    assert s.forces == []
    bonds = forces.Bonds(pse, c["pairs"], kind=kinds, k=c["k"], r0=c["r0"], types=c["types"], virial=True)
    s.net_force.zero_()
    bonds.compute(0)
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    W = np.array([[ref[1], ref[2], ref[3]], [ref[2], ref[4], ref[5]], [ref[3], ref[5], ref[6]]])
    assert abs(bonds.energy - ref[0]) <= tol and bonds.nbonds == bonds.npairs == ref[7] and bonds.overstretched == 0
    assert np.abs(bonds.virial - W).max() <= tol and np.abs(bonds.stress() + W / vol).max() <= tol / vol
    log = forces.StressLog(bonds, period=5, capacity=8)
    snap = _Snapshots(s, 5)
    s.analyzers.append(snap)
    s.run(20)
    tab = log.table()
    assert tab.shape == (4, 10) and list(tab[:, 0]) == [0.0, 5.0, 10.0, 15.0] and sorted(snap.saved) == [0, 5, 10, 15]
    assert tab[0, 1] == 0.0 and np.all(np.diff(tab[:, 1]) > 0.0)           # the box tilt of the sample steps: sheared
    moved = 0.0
    for row in tab:
        p, b = snap.saved[int(row[0])]
        p = p.cpu().numpy()[:, :3]
        assert b[3] == row[1]
        br.assert_fene_in_range(p, b, c["pairs"], c["types"], c["kinds"], c["r0"], port())      # still where the bound holds
        r8, _, over = br.bond_observables(p, b, c["pairs"], c["types"], c["kinds"], c["k"], c["r0"], port())
        t8 = 1e-11 * max(1.0, np.abs(r8).max())
        print(f"step {int(row[0])}: xy {row[1]:.4f}, U {row[2]:.6g} / {r8[0]:.6g}, sigma_xy {row[4]:.6g} / {-r8[2] / vol:.6g}")
        assert over == 0 and row[9] == r8[7] == len(c["pairs"])
        assert abs(row[2] - r8[0]) <= t8 and np.abs(row[3:9] + r8[1:7] / vol).max() <= t8 / vol
        moved = max(moved, np.abs(p - c["pos"]).max())
    assert moved > 1e-3 and bonds.overstretched == 0 and torch.isfinite(s.pos).all()


def test_topology_builder_of_the_polymer_example():
    """examples/polymer_solution.py build_chains at small size: chain-ordered beads, bonds of the prescribed length through the
    periodic faces, and its radius of gyration unfolds the chains; the device takes the topology as it is."""
    spec = importlib.util.spec_from_file_location("polymer_solution", os.path.join(ROOT, "examples", "polymer_solution.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    box = TILTED
    nchains, beads, b = 12, 20, 2.0
    pos, pairs = ex.build_chains(nchains, beads, box, b, seed=5)
    assert pos.shape == (nchains * beads, 3) and pairs.shape == (nchains * (beads - 1), 2)
    assert np.all(pairs[:, 1] == pairs[:, 0] + 1) and not np.any(pairs[:, 1] % beads == 0)          # no bond from chain to chain
    assert np.array_equal(port().wrap(pos, np.zeros(pos.shape, dtype=np.int64), box)[0], pos)         # inside the tilted cell
    d = port().min_image(pos[pairs[:, 0]] - pos[pairs[:, 1]], box)
    assert np.abs(np.linalg.norm(d, axis=1) - b).max() < 1e-12
    assert np.abs(pos[pairs[:, 0]] - pos[pairs[:, 1]]).max() > 5.0                                    # some bonds do cross a face
    # Rg of the unfolded chains, against the chains unfolded here
    rg = []
    for ch in range(nchains):
        q = np.vstack([np.zeros(3), np.cumsum(-d[ch * (beads - 1):(ch + 1) * (beads - 1)], axis=0)])
        rg.append(np.sqrt(((q - q.mean(axis=0)) ** 2).sum(axis=1).mean()))
    assert abs(ex.radius_of_gyration(pos, box, nchains, beads) - np.mean(rg)) < 1e-12
    # ... and on the device, with the example's FENE parameters
    k, r0 = 7.5, 3.0
    bl = engine(box).bonds(pairs, kinds="fene", k=k, r0=r0, n=len(pos))
    f = to4(np.zeros((len(pos), 3)))
    out = bl.forces(to4(pos), f, accumulate=False).cpu().numpy()
    ref, F, over = br.bond_observables(pos, box, pairs, None, [br.FENE], [k], [r0], port())
    br.assert_fene_in_range(pos, box, pairs, None, [br.FENE], [r0], port())
    check_obs(out, ref, "example topology")
    check_forces(f.cpu().numpy()[:, :3], F, "example topology")
    assert over == 0 and bl.overstretched == 0 and out[7] == len(pairs)
    bl.close()
