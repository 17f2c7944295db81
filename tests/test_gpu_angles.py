"""GPU tests of the angle forces (pse_angles_create / pse_angle_forces): harmonic and cosine-squared angles against the NumPy
reference of tests/angle_ref.py (validated on the CPU by tests/test_angle_reference.py, which also asserts that every angle of the
inputs used here has sin(theta) >= 0.05, the exactly collinear triples of the collinear case apart), bit-exact invariance under the
order of the list and of an angle's ends, the call forms, the degenerate geometries, the error returns, and the host UI on top
(Engine.angles, forces.Angles with forces.Bonds and a StressLog, the topology builder of examples/semiflexible_polymers.py).

Bound: the project's own for these passes (tests/test_gpu_pair_virial.py), 1e-11 max(1, max |ref|), the eight observables together
and the forces together; the count of angles must match exactly."""
import ctypes
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

import angle_ref as ar
import bond_ref as br
from conftest import to4
from pair_virial_ref import random_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBIC, TILTED = ar.BOXES
BOX_IDS = ["cubic", "tilted"]
KIND_IDS = ["harmonic", "cosinesq"]
KIND_NAMES = {ar.HARMONIC: "harmonic", ar.COSINESQ: "cosinesq"}
INVALID = -1


def port():
    from oracle import pse_port
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(ar.N_MAX, box, xi=0.5, error=1e-3)


def check_obs(got, ref, what=""):
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"{what}: max |obs - ref| = {err:.3e} (bound {tol:.3e}), nangles {got[7]:.0f} / {ref[7]:.0f}, U {ref[0]:.6g}, "
          f"trace W {got[1] + got[4] + got[6]:.3e}")
    assert got[7] == ref[7], (what, got[7], ref[7])
    assert err <= tol, (what, got, ref)


def check_forces(got, F, what=""):
    tol = 1e-11 * max(1.0, np.abs(F).max())
    err = np.abs(got - F).max()
    print(f"{what}: max |F - ref| = {err:.3e} (bound {tol:.3e}), max |F| {np.abs(F).max():.6g}")
    assert err <= tol, (what, err, tol)


def reference(c, box, pos=None):
    return ar.angle_observables(c["pos"] if pos is None else pos, box, c["triples"], c["types"], c["kinds"], c["k"], c["theta0"], port())


def angle_list(eng, c, triples=None, types="case"):
    return eng.angles(c["triples"] if triples is None else triples, c["types"] if isinstance(types, str) else types, kinds=c["kinds"],
                      k=c["k"], theta0=c["theta0"], n=len(c["pos"]))


def run_case(c, box, what):
    """accumulate = 0 on a preset force array: observables, forces, kept w."""
    n = len(c["pos"])
    ref, F = reference(c, box)
    assert ref[7] == len(c["triples"])
    al = angle_list(engine(box), c)
    f = to4(np.random.default_rng(5).normal(size=(n, 3)), 3.0)
    out = al.forces(to4(c["pos"]), f, accumulate=False).cpu().numpy()
    check_obs(out, ref, what)
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, what)
    assert np.all(g[:, 3] == 3.0)
    al.close()
    return out, g


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
@pytest.mark.parametrize("kind", [ar.HARMONIC, ar.COSINESQ], ids=KIND_IDS)
@pytest.mark.parametrize("n", ar.ROW_COUNTS)
def test_row_counts(n, kind, box):
    """One chain of n beads, n - 2 angles: the smallest list, a partial last wave, a full one, one lane of the next; the same for the
    256-thread workgroup (257: a second workgroup of one thread; 513 = n_max: a third)."""
    run_case(ar.chain_case(n, box, kind, port()), box, f"chain n={n} kind={kind}")


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
@pytest.mark.parametrize("kind", [ar.HARMONIC, ar.COSINESQ], ids=KIND_IDS)
@pytest.mark.parametrize("name", ar.TOPOLOGIES + ("graph",))
def test_topologies(name, kind, box):
    c = ar.graph_case(box, kind, port()) if name == "graph" else ar.topology_case(name, box, kind, port())
    assert len(c["pos"]) == ar.N_TOPOLOGY
    out, g = run_case(c, box, f"{name} kind={kind}")
    free = np.setdiff1d(np.arange(ar.N_TOPOLOGY), np.unique(c["triples"]))
    assert len(free) > 0 and not g[free, :3].any()                    # accumulate = 0 zeroes the rows of particles in no angle
    if name == "star":
        assert np.bincount(c["triples"][:, 1])[0] == 40               # the hub is the vertex of all 40
    if name == "duplicates":                                          # every copy acts: more angles than distinct triples
        canon = np.stack([c["triples"][:, [0, 2]].min(axis=1), c["triples"][:, 1], c["triples"][:, [0, 2]].max(axis=1)], axis=1)
        assert out[7] == len(c["triples"]) > len(np.unique(canon, axis=0))
    if name == "two_types":
        assert sorted(c["kinds"]) == [ar.HARMONIC, ar.COSINESQ] and set(c["types"]) == {0, 1} and c["theta0"][0] != c["theta0"][1]


def test_call_forms():
    """accumulate 0 and 1, force = NULL, out8 = NULL; the row of a particle in no angle keeps its preset value bit for bit under
    accumulate = 1 and becomes zero under accumulate = 0; w survives in both."""
    import torch
    box = TILTED
    c = ar.topology_case("chains", box, ar.HARMONIC, port())
    n = len(c["pos"])
    ref, F = reference(c, box)
    al = angle_list(engine(box), c)
    dpos = to4(c["pos"])
    base = np.random.default_rng(6).normal(size=(n, 3))
    free = np.setdiff1d(np.arange(n), np.unique(c["triples"]))
    assert len(free) == 60
    # accumulate = 1
    f1 = to4(base, 7.0)
    out1 = al.forces(dpos, f1, accumulate=True)
    assert out1.shape == (8,) and out1.is_cuda and out1.dtype == torch.float64
    check_obs(out1.cpu().numpy(), ref, "accumulate=1")
    g1 = f1.cpu().numpy()
    check_forces(g1[:, :3], F + base, "accumulate=1")
    assert np.array_equal(g1[free, :3], to4(base).cpu().numpy()[free, :3]) and np.all(g1[:, 3] == 7.0)
    # accumulate = 0
    f0 = to4(base, 7.0)
    out0 = al.forces(dpos, f0, accumulate=False).cpu().numpy()
    g0 = f0.cpu().numpy()
    check_forces(g0[:, :3], F, "accumulate=0")
    assert not g0[free, :3].any() and np.all(g0[:, 3] == 7.0)
    assert np.array_equal(out0, out1.cpu().numpy())
    # force = NULL: observables only
    outn = al.forces(dpos, None).cpu().numpy()
    assert np.array_equal(outn, out0)
    # out8 = NULL: forces only, a given `out` is left alone
    keep = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    f2 = to4(base, 7.0)
    assert al.forces(dpos, f2, accumulate=False, out=keep, observables=False) is None
    assert np.array_equal(f2.cpu().numpy(), g0) and np.all(keep.cpu().numpy() == -1.0)
    # both NULL is refused
    import pse_amd
    with pytest.raises(pse_amd.PSEError, match="both null"):
        al.forces(dpos, None, observables=False)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], c["pos"])
    al.close()


@pytest.mark.parametrize("name", ["two_types", "duplicates", "graph", "star"])
def test_order_invariance_bit_for_bit(name):
    """A permuted list with swapped ends gives bit-identical forces and out8; so do two calls on equal inputs."""
    box = TILTED
    c = ar.graph_case(box, ar.HARMONIC, port()) if name == "graph" else ar.topology_case(name, box, ar.HARMONIC, port())
    n = len(c["pos"])
    eng = engine(box)
    dpos = to4(c["pos"])

    def run(al):
        f = to4(np.zeros((n, 3)))
        o = al.forces(dpos, f, accumulate=False).cpu().numpy()
        return o, f.cpu().numpy()

    a = angle_list(eng, c)
    o1, f1 = run(a)
    o2, f2 = run(a)
    assert np.array_equal(o1, o2) and np.array_equal(f1, f2)
    rng = np.random.default_rng(4)
    for trial in range(2):
        o = rng.permutation(len(c["triples"]))
        triples = c["triples"][o].copy()
        flip = rng.uniform(size=len(triples)) < 0.5
        triples[flip] = triples[flip, ::-1]
        assert flip.any() and not np.array_equal(triples, c["triples"])
        b = angle_list(eng, c, triples, None if c["types"] is None else c["types"][o])
        o3, f3 = run(b)
        assert np.array_equal(o1, o3) and np.array_equal(f1, f3)
        b.close()
    a.close()


@pytest.mark.parametrize("kind", ["harmonic", "cosinesq"])
def test_coincident_members_do_nothing(kind):
    """r1 == 0 (i at j), and r2 == 0 through a periodic image (3 is an image of 1): nothing happens and nothing is counted; the one
    proper angle of the list acts."""
    box = TILTED
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.5, 2.5, 3.5], [1.0 + box[0], 2.0, 3.0], [0.5, 2.0, 3.0]])
    triples = [[0, 1, 2], [2, 3, 1], [2, 1, 4]]
    code = {"harmonic": ar.HARMONIC, "cosinesq": ar.COSINESQ}[kind]
    al = engine(box).angles(triples, kinds=[kind], k=[30.0], theta0=[2.0], n=5)
    ref, F = ar.angle_observables(pos, box, triples, None, [code], [30.0], [2.0], port())
    assert ref[7] == 1 and not F[[0, 3]].any() and np.abs(F[[1, 2, 4]]).max(axis=1).min() > 1.0
    f = to4(np.ones((5, 3)))
    out = al.forces(to4(pos), f, accumulate=False).cpu().numpy()
    check_obs(out, ref, f"r == 0, {kind}")
    g = f.cpu().numpy()[:, :3]
    check_forces(g, F, f"r == 0, {kind}")
    assert not g[[0, 3]].any() and np.isfinite(out).all()
    al.close()


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=BOX_IDS)
def test_exactly_straight_and_exactly_folded_triples(box):
    """c = -1 exactly with theta0 = pi (harmonic) and with the cosine-squared kind, c = +1 exactly with every type: finite, and --
    the bracket of the force is exactly zero there, whatever the capped 1/sin multiplies it by -- within the bound of the reference."""
    c = ar.collinear_case(box, port())
    assert c["collinear"] == 7
    out, g = run_case(c, box, "collinear")
    assert np.isfinite(out).all() and np.isfinite(g).all()
    assert not g[:6, :3].any() and np.abs(g[6:9, :3]).max() > 0.1           # the collinear triples feel nothing, the generic one acts
    assert out[0] > 0.5 * ar.K_H * math.pi ** 2                              # the folded harmonic angle at theta0 = pi is in U


def test_neighbour_list_is_untouched():
    """Angle calls between two mobility calls on the same positions: the second mobility call reuses the kept list exactly as it
    does without them, and the angle calls themselves neither build nor reuse."""
    import pse_amd
    box = TILTED
    c = ar.topology_case("chains", box, ar.HARMONIC, port())
    n = len(c["pos"])
    force = to4(np.random.default_rng(1).normal(size=(n, 3)))

    def stats(eng):
        b, r = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        assert eng._lib.pse_neighbor_stats(eng._h, None, ctypes.byref(b), ctypes.byref(r)) == 0
        return b.value, r.value

    counts = []
    for with_angles in (False, True):
        eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3)
        dpos = to4(c["pos"])
        eng.mobility(dpos, force)
        before = stats(eng)
        if with_angles:
            al = angle_list(eng, c)
            f = to4(np.zeros((n, 3)))
            al.forces(dpos, f, accumulate=False)
            al.forces(dpos, f, accumulate=True, observables=False)
            assert stats(eng) == before
            check_forces(f.cpu().numpy()[:, :3], 2.0 * reference(c, box)[1], "between the mobility calls")
        eng.mobility(dpos, force)
        counts.append((before, stats(eng)))
        if with_angles:
            al.close()
        eng.close()
    print("(builds, reuses) after the first and the second mobility call, without / with angle calls:", counts)
    assert counts[0] == counts[1], counts
    assert sum(counts[1][1]) > sum(counts[1][0]) >= 1                      # the mobility calls do go through the list


def test_asynchronous_submission_into_a_log_row():
    """Four calls on four configurations, each into its own row of a (4, 8) tensor, read once at the end."""
    import torch
    box = TILTED
    eng = engine(box)
    cases = [ar.topology_case(name, box, ar.COSINESQ, port()) for name in ("chains", "ring", "star", "two_types")]
    lists = [angle_list(eng, c) for c in cases]
    dpos = [to4(c["pos"]) for c in cases]
    fs = [to4(np.zeros((ar.N_TOPOLOGY, 3))) for _ in cases]
    log = torch.full((4, 8), -1.0, dtype=torch.float64, device="cuda")
    for q in range(4):
        assert lists[q].forces(dpos[q], fs[q], accumulate=False, out=log[q]).data_ptr() == log[q].data_ptr()
    rows = log.cpu().numpy()                                              # the one read
    for q, c in enumerate(cases):
        ref, F = reference(c, box)
        check_obs(rows[q], ref, f"log row {q}")
        check_forces(fs[q].cpu().numpy()[:, :3], F, f"log row {q}")
    for al in lists:
        al.close()


def test_a_slab_rank_handle_takes_angle_calls():
    """The pass does not use the cell list, so a slab rank's handle (which orders only its own cells) gives the complete sums."""
    import pse_amd
    box = (40.0, 40.0, 40.0, 0.0)
    c = ar.topology_case("chains", box, ar.HARMONIC, port())
    eng = pse_amd.Engine(ar.N_TOPOLOGY, box, xi=0.5, error=1e-3, grid=(48, 48, 48), n_slabs=2, slab_rank=0)
    al = angle_list(eng, c)
    f = to4(np.zeros((ar.N_TOPOLOGY, 3)))
    out = al.forces(to4(c["pos"]), f, accumulate=False).cpu().numpy()
    ref, F = reference(c, box)
    assert np.all(ar.sines(c["pos"], box, c["triples"], port()) >= ar.SIN_MIN)      # (this box is not among the inputs validated on the CPU)
    check_obs(out, ref, "slab rank")
    check_forces(f.cpu().numpy()[:, :3], F, "slab rank")
    al.close()
    eng.close()


def test_misuse_is_reported():
    """Raw C-ABI, as a C host would call it: every error return of pse_angles_create and pse_angle_forces, with a message naming the
    value; the object then works after all the refusals."""
    import torch
    from pse_amd import _lib
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    eng = engine(CUBIC)
    h, n = eng._h, 64
    A = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)                # noqa: E731
    good_triples = u32([[0, 1, 2], [1, 2, 3], [5, 9, 7]])
    good = dict(h=h, n=n, na=3, triples=good_triples, types=u32([0, 1, 0]), nt=2, kind=np.array([0, 1], dtype=np.int32),
                k=np.array([30.0, 20.0]), theta0=np.array([2.0, 2.5]))
    nan, inf = float("nan"), float("inf")

    def create(out="new", **kw):
        a = dict(good, **kw)
        b = ctypes.c_void_p(0xdead) if out == "new" else out
        rc = lib.pse_angles_create(a["h"], a["n"], a["na"], A(a["triples"]), A(a["types"]), a["nt"], A(a["kind"]), A(a["k"]), A(a["theta0"]),
                                   None if b is None else ctypes.byref(b))
        return rc, b

    def refused(word, **kw):
        rc, b = create(**kw)
        assert rc == INVALID, (word, rc)
        assert msg() and word in msg(), (word, msg())
        assert b is None or not b.value                   # *out is null after a refusal

    refused("null handle", h=None)
    refused("null triples_host", triples=None)
    refused("null out", out=None)
    refused("null parameter array", kind=None)
    refused("null parameter array", k=None)
    refused("null parameter array", theta0=None)
    refused("n = 0", n=0)
    refused(f"n = {ar.N_MAX + 1}", n=ar.N_MAX + 1)
    refused("nangles = 0", na=0)
    refused("nangles = 268435457", na=(1 << 28) + 1)
    refused("(5, 9, 64)", triples=u32([[0, 1, 2], [1, 2, 3], [5, 9, 64]]))
    refused("(1, 64, 3)", triples=u32([[0, 1, 2], [1, 64, 3], [5, 9, 7]]))
    refused("(64, 1, 2)", triples=u32([[64, 1, 2], [1, 2, 3], [5, 9, 7]]))
    refused("(7, 7, 3) has two equal members", triples=u32([[0, 1, 2], [7, 7, 3], [5, 9, 7]]))
    refused("(1, 7, 7) has two equal members", triples=u32([[0, 1, 2], [1, 7, 7], [5, 9, 7]]))
    refused("(5, 9, 5) has two equal members", triples=u32([[0, 1, 2], [1, 2, 3], [5, 9, 5]]))
    refused("ntypes = 0", nt=0)
    refused("ntypes = 65", nt=65)
    refused("ntypes = -1", nt=-1)
    refused("type 2", types=u32([0, 2, 0]))
    refused("type 1", types=u32([0, 1, 0]), nt=1)
    refused("kind 2", kind=np.array([0, 2], dtype=np.int32))
    refused("kind -1", kind=np.array([-1, 1], dtype=np.int32))
    refused("finite", k=np.array([nan, 20.0]))
    refused("finite", k=np.array([30.0, inf]))
    refused("finite", theta0=np.array([nan, 2.5]))
    refused("finite", theta0=np.array([2.0, inf]))
    refused("theta0 = -0.5", theta0=np.array([-0.5, 2.5]))
    refused("theta0 = 3.2", theta0=np.array([2.0, 3.2]))
    # theta0 = 0 and pi, a negative k and types = NULL are legal; the object works after all the refusals
    rc, b = create(types=None, theta0=np.array([math.pi, 0.0]), k=np.array([-1.0, 20.0]))
    assert rc == 0 and b.value, msg()
    assert lib.pse_angles_destroy(b) == 0
    rc, b = create(types=None)
    assert rc == 0 and b.value, msg()
    pos = random_points(n, CUBIC, seed=2) * 0.1                       # a cluster: every arm is short
    assert np.all(ar.sines(pos, CUBIC, good_triples, port()) >= ar.SIN_MIN)
    dpos, dF = to4(pos), to4(np.zeros((n, 3)), 5.0)
    out8 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    call = lib.pse_angle_forces
    for word, args in (("null angle object", (None, P(dpos), P(dF), 0, P(out8))), ("null pos", (b, None, P(dF), 0, P(out8))),
                       ("both null", (b, P(dpos), None, 0, None))):
        assert call(*args) == INVALID and word in msg(), (word, msg())
    torch.cuda.synchronize()
    assert np.all(out8.cpu().numpy() == -1.0) and np.array_equal(dF.cpu().numpy(), to4(np.zeros((n, 3)), 5.0).cpu().numpy())
    assert call(b, P(dpos), P(dF), 0, P(out8)) == 0, msg()
    ref, F = ar.angle_observables(pos, CUBIC, good_triples, None, [0, 1], [30.0, 20.0], [2.0, 2.5], port())
    check_obs(out8.cpu().numpy(), ref, "after the refused calls")
    check_forces(dF.cpu().numpy()[:, :3], F, "after the refused calls")
    assert lib.pse_angles_destroy(b) == 0 and lib.pse_angles_destroy(None) == 0


def test_engine_wrapper_checks_its_arguments_and_lifetime():
    import pse_amd
    eng = pse_amd.Engine(64, CUBIC, xi=0.5, error=1e-3)
    for bad in ([], [[0, 1]], [[0, 1, 2, 3]], [[0.5, 1.0, 2.0]], [[-1, 2, 3]]):
        with pytest.raises(ValueError):
            eng.angles(bad)
    with pytest.raises(ValueError):
        eng.angles([[0, 1, 2]], types=[0, 1])
    with pytest.raises(ValueError):
        eng.angles([[0, 1, 2]], kinds=["cosine"])
    with pytest.raises(ValueError):
        eng.angles([[0, 1, 2]], kinds=["harmonic", "cosinesq"], k=[1.0], theta0=[1.0, 1.0])
    with pytest.raises(pse_amd.PSEError, match="n_max"):
        eng.angles([[0, 1, 2]], n=65)
    with pytest.raises(pse_amd.PSEError, match="theta0"):
        eng.angles([[0, 1, 2]], theta0=4.0)
    al = eng.angles([[0, 1, 2], [1, 2, 3]], kinds="cosinesq", k=30.0, theta0=2.5)   # scalars for a single type; n defaults to n_max
    assert al.n == 64 and al.nangles == 2
    with pytest.raises(ValueError):
        al.forces(to4(np.zeros((10, 3))), None)                            # fewer rows than the topology has particles
    keep = eng.angles([[3, 4, 5]])                                          # the defaults: harmonic, k = 1, theta0 = pi
    al.close(); al.close()                                                  # closing twice is harmless
    with pytest.raises(ValueError, match="closed"):
        al.forces(to4(np.zeros((64, 3))), None)
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


def test_angles_provider_with_bonds_in_a_sheared_run_with_a_stress_log(restored_context):
    """forces.Angles (a harmonic and a cosine-squared type) beside forces.Bonds through 20 steps of a sheared System.run with a
    StressLog at period 5: each sampled row is the reference on the positions an analyzer saved on that step, in the box of that step."""
    import torch
    from pse_amd import forces
    box = TILTED[:3] + (0.0,)
    c = ar.topology_case("two_types", box, ar.HARMONIC, port())
    kinds = [KIND_NAMES[q] for q in c["kinds"]]
    pairs = np.vstack([c["triples"][:, :2], c["triples"][:, 1:]])
    pairs = np.unique(np.sort(pairs, axis=1), axis=0)                      # the bonds along the four chains
    s, pse = _sheared_system(c["pos"], box, dt=1e-3)
    vol = box[0] * box[1] * box[2]
    plain = forces.Angles(pse, c["triples"], kind=kinds, k=c["k"], theta0=c["theta0"], types=c["types"])
    ref, F = reference(c, box)
    plain.compute(0)                                                       # virial=False: forces only
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "Angles, virial=False")
    with pytest.raises(RuntimeError, match="Angles"):
        plain.energy
    with pytest.raises(ValueError, match="Angles"):
        forces.StressLog(plain, 1, 4)
    s.forces.remove(plain)
    for bad in (dict(kind="cosine"), dict(kind=["harmonic", "cosinesq"], k=[1.0, 2.0, 3.0]), dict(types=[0])):
        with pytest.raises(ValueError):
            forces.Angles(pse, c["triples"], **bad)
    with pytest.raises(ValueError):
        forces.Angles(pse, np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        forces.Angles(pse, c["triples"][:, :2])
    with pytest.raises(ValueError):                                        # an index that would wrap to a valid one as uint32
        forces.Angles(pse, [[0, 1, 2 ** 32 + 2]])
    with pytest.raises(ValueError):
        forces.Angles(pse, c["triples"], kind=kinds, k=c["k"], theta0=c["theta0"], types=c["types"] + 2 ** 32)
    assert s.forces == []
    bonds = forces.Bonds(pse, pairs, kind="harmonic", k=br.K_H, r0=1.1, virial=True)
    angles = forces.Angles(pse, c["triples"], kind=kinds, k=c["k"], theta0=c["theta0"], types=c["types"], virial=True)
    s.net_force.zero_()
    angles.compute(0)
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    W = np.array([[ref[1], ref[2], ref[3]], [ref[2], ref[4], ref[5]], [ref[3], ref[5], ref[6]]])
    assert abs(angles.energy - ref[0]) <= tol and angles.nangles == angles.npairs == ref[7] == len(c["triples"])
    assert np.abs(angles.virial - W).max() <= tol and np.abs(angles.stress() + W / vol).max() <= tol / vol
    assert abs(np.trace(angles.virial)) <= tol
    log = forces.StressLog(angles, period=5, capacity=8)
    blog = forces.StressLog(bonds, period=5, capacity=8)
    snap = _Snapshots(s, 5)
    s.analyzers.append(snap)
    s.run(20)
    tab, btab = log.table(), blog.table()
    assert tab.shape == (4, 10) and list(tab[:, 0]) == [0.0, 5.0, 10.0, 15.0] and sorted(snap.saved) == [0, 5, 10, 15]
    assert tab[0, 1] == 0.0 and np.all(np.diff(tab[:, 1]) > 0.0)           # the box tilt of the sample steps: sheared
    moved = 0.0
    for row, brow in zip(tab, btab):
        p, b = snap.saved[int(row[0])]
        p = p.cpu().numpy()[:, :3]
        assert b[3] == row[1]
        assert np.all(ar.sines(p, b, c["triples"], port()) >= ar.SIN_MIN)                       # still where the bound holds
        r8, _ = reference(c, b, p)
        t8 = 1e-11 * max(1.0, np.abs(r8).max())
        print(f"step {int(row[0])}: xy {row[1]:.4f}, U {row[2]:.6g} / {r8[0]:.6g}, sigma_xy {row[4]:.6g} / {-r8[2] / vol:.6g}")
        assert row[9] == r8[7] == len(c["triples"])
        assert abs(row[2] - r8[0]) <= t8 and np.abs(row[3:9] + r8[1:7] / vol).max() <= t8 / vol
        b8, _, over = br.bond_observables(p, b, pairs, None, [br.HARMONIC], [br.K_H], [1.1], port())   # the bonds beside them, too
        tb = 1e-11 * max(1.0, np.abs(b8).max())
        assert over == 0 and brow[9] == b8[7] == len(pairs) and abs(brow[2] - b8[0]) <= tb and np.abs(brow[3:9] + b8[1:7] / vol).max() <= tb / vol
        moved = max(moved, np.abs(p - c["pos"]).max())
    assert moved > 1e-3 and torch.isfinite(s.pos).all()


def test_topology_builder_of_the_semiflexible_example():
    """examples/semiflexible_polymers.py build_topology at small size: chain-ordered beads, one bond per neighbouring pair and one
    angle per inner bead, none from chain to chain; its mean bond-angle cosine against the one computed here; the device takes
    the topology as it is, with the example's parameters."""
    spec = importlib.util.spec_from_file_location("semiflexible_polymers", os.path.join(ROOT, "examples", "semiflexible_polymers.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    box = TILTED
    nchains, beads, b = 12, 20, 2.0
    pos, pairs, triples = ex.build_topology(nchains, beads, box, b, seed=5)
    assert pos.shape == (nchains * beads, 3) and pairs.shape == (nchains * (beads - 1), 2) and triples.shape == (nchains * (beads - 2), 3)
    assert np.all(pairs[:, 1] == pairs[:, 0] + 1) and not np.any(pairs[:, 1] % beads == 0)          # no bond from chain to chain
    assert np.all(triples[:, 0] + 1 == triples[:, 1]) and np.all(triples[:, 1] + 1 == triples[:, 2])
    assert not np.any(triples[:, 1] % beads == 0) and not np.any(triples[:, 2] % beads == 0)           # no angle from chain to chain
    assert np.array_equal(port().wrap(pos, np.zeros(pos.shape, dtype=np.int64), box)[0], pos)         # inside the tilted cell
    d1 = port().min_image(pos[triples[:, 0]] - pos[triples[:, 1]], box)
    d2 = port().min_image(pos[triples[:, 2]] - pos[triples[:, 1]], box)
    assert np.abs(np.linalg.norm(d1, axis=1) - b).max() < 1e-12 and np.abs(np.linalg.norm(d2, axis=1) - b).max() < 1e-12
    cosines = (d1 * d2).sum(axis=1) / (b * b)
    assert abs(ex.mean_bond_angle_cosine(pos, box, triples) - cosines.mean()) < 1e-12
    assert np.all(ar.sines(pos, box, triples, port()) >= ar.SIN_MIN)
    # ... and on the device, with the example's cosine-squared parameters
    al = engine(box).angles(triples, kinds="cosinesq", k=ex.K_BEND, theta0=ex.THETA0, n=len(pos))
    f = to4(np.zeros((len(pos), 3)))
    out = al.forces(to4(pos), f, accumulate=False).cpu().numpy()
    ref, F = ar.angle_observables(pos, box, triples, None, [ar.COSINESQ], [ex.K_BEND], [ex.THETA0], port())
    check_obs(out, ref, "example topology")
    check_forces(f.cpu().numpy()[:, :3], F, "example topology")
    assert out[7] == len(triples)
    al.close()
