"""GPU tests of what the force providers (pse_amd.forces) owe to the engine they are made on (integrate.PSEv1.engine, the ctypes
binding on the handle of the C++ Stokes object): a provider dies with the handle that setParams() replaces and says so, a collected
provider frees its device object and leaves the others alone, and an empty group is treated as the C++ layer treated it.  The same
two promises for the analysis objects of an Engine (exclusions, histogram, structure factor, displacement origins, cluster links).

64 particles, four chains of 16 beads (tests/bond_ref.py chains) in the cubic box of the provider tests.  Everything compared here is
the output of the same kernels on the same arguments, so equal means bit for bit: np.array_equal."""
import gc
import sys

import numpy as np
import pytest

import bond_ref as br
from pair_table_ref import morse_table

pytestmark = pytest.mark.gpu

BOX = (14.0, 14.0, 14.0, 0.0)
NCHAINS, BEADS = 4, 16
RMIN, RMAX = 0.7, 3.0


@pytest.fixture(scope="module")
def case():
    """Positions and topology, made once and never written to."""
    from oracle import pse_port
    pos, pairs = br.chains(NCHAINS, BEADS, BOX, np.full(NCHAINS * (BEADS - 1), 1.6), 5, pse_port)
    first = np.arange(NCHAINS * BEADS).reshape(NCHAINS, BEADS)
    triples = np.stack([first[:, :-2], first[:, 1:-1], first[:, 2:]], axis=-1).reshape(-1, 3)
    quads = np.stack([first[:, :-3], first[:, 1:-2], first[:, 2:-1], first[:, 3:]], axis=-1).reshape(-1, 4)
    table = morse_table(rmin=RMIN, rmax=RMAX, width=64, D=5.0, alpha=2.0, r0=1.5)
    out = dict(pos=pos, pairs=pairs, triples=triples, quads=quads, table=table, types=np.arange(NCHAINS * BEADS) % 2)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture
def restored_context():
    """A System registers itself as the current simulation context: put back what was there."""
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


def system(case, members=None):
    from pse_amd import integrate
    from pse_amd.system import Group, System
    s = System(case["pos"], BOX, dt=1e-3)
    group = s.all() if members is None else Group(s, members)
    return s, integrate.PSEv1(group=group, T=0.0, seed=3, xi=0.5, error=1e-3)


def bonded(pse, c):
    from pse_amd import forces
    return [forces.Bonds(pse, c["pairs"], kind="fene", k=30.0, r0=2.5), forces.Angles(pse, c["triples"], kind="harmonic", k=5.0, theta0=2.0),
            forces.Dihedrals(pse, c["quads"], kind="opls", params=(1.0, 2.0, 3.0, 4.0))]


def pair(pse, c):
    from pse_amd import forces
    excl = forces.Exclusions.from_topology(pse, bonds=c["pairs"], angles=c["triples"])
    t = np.array(c["table"])
    return [forces.TablePair(pse, t, RMIN, RMAX, exclusions=excl),
            forces.TypedTablePair(pse, c["types"], {(0, 0): (t, RMIN, RMAX), (0, 1): (0.5 * t, RMIN, 2.5)}, virial=True)]


def net_force(s, timestep=0):
    """What the providers of `s` leave in net_force, as System.run fills it."""
    s.net_force.zero_()
    for f in s.forces:
        f.compute(timestep)
    return s.net_force.cpu().numpy().copy()


class _Unraisable:
    """Collects what a __del__ raised instead of letting the interpreter print it."""

    def __enter__(self):
        self.seen, self._hook = [], sys.unraisablehook
        sys.unraisablehook = self.seen.append
        return self

    def __exit__(self, *exc):
        sys.unraisablehook = self._hook


def test_providers_die_with_the_engine_that_set_params_replaces(case, restored_context):
    s, pse = system(case)
    old = bonded(pse, case) + pair(pse, case)
    kept = net_force(s)
    assert np.abs(kept[:, :3]).max() > 0.0 and pse.engine.serial == 1
    pse.cpp_method.setParams()                                     # a new handle; pse_destroy freed the five device objects
    assert pse.engine.serial == 2
    for p in old:
        with pytest.raises(ValueError, match="setParams"):
            p.compute(0)
    with pytest.raises(ValueError, match="setParams"):
        old[0].overstretched
    del s.forces[:]
    with _Unraisable() as quiet:                                   # nothing is freed twice, nothing complains
        del old, p
        gc.collect()
    assert quiet.seen == []
    bonded(pse, case), pair(pse, case)
    assert len(s.forces) == 5 and np.array_equal(net_force(s), kept)


def test_empty_group(case, restored_context):
    """A HarmonicRepulsion without virial does nothing on an empty group; every pass that would have to write observables or that
    the C-ABI refuses at N = 0 raises, as through the C++ layer before."""
    from pse_amd import forces
    s, pse = system(case, members=[])
    assert len(pse.group) == 0
    excl = forces.Exclusions(pse, case["pairs"])
    s.net_force[:, :3] = 7.0
    before = s.net_force.cpu().numpy().copy()
    forces.HarmonicRepulsion(pse, k=40.0)
    forces.HarmonicRepulsion(pse, k=40.0, exclusions=excl)
    for f in s.forces:
        f.compute(0)
    assert np.array_equal(s.net_force.cpu().numpy(), before)
    refused = [forces.HarmonicRepulsion(pse, k=40.0, virial=True), forces.HarmonicRepulsion(pse, k=40.0, virial=True, exclusions=excl)] + pair(pse, case)
    for f in refused:
        with pytest.raises(RuntimeError):
            f.compute(0)
    assert np.array_equal(s.net_force.cpu().numpy(), before)


def test_a_collected_provider_frees_its_object_and_leaves_the_rest(case, restored_context):
    s, pse = system(case)
    bonded(pse, case)
    kept = net_force(s)                                            # the run that never had the pair providers
    extra = pair(pse, case)
    assert not np.array_equal(net_force(s), kept)
    for p in extra:
        s.forces.remove(p)
    with _Unraisable() as quiet:
        del extra, p
        gc.collect()                                               # pse_typed_table_destroy and pse_exclusions_destroy run here
    assert quiet.seen == [] and len(s.forces) == 3
    assert np.array_equal(net_force(s), kept)
    s.run(2)                                                       # ... and the integrator steps with what is left
    moved = s.pos.cpu().numpy()[:, :3]
    assert np.isfinite(moved).all() and np.abs(moved - case["pos"]).max() > 0.0


# -- the analysis objects of an Engine ----------------------------------------------------------------------------------------------

ANALYSIS = ("exclusions", "histogram", "structure_factor", "origins", "links")   # in the order they are made


def make(eng, case, name):
    from pse_amd import analyze
    types = np.array(case["types"])
    return {"exclusions": lambda: eng.exclusions(np.array(case["pairs"])),
            "histogram": lambda: eng.pair_histogram(types, 2, 8, 0.0, RMAX),
            "structure_factor": lambda: eng.structure_factor(types, 2, analyze.axis_modes(2)),
            "origins": lambda: eng.msd_origins(types, 2, 2),
            "links": lambda: eng.clusters(types, 2, 1.8)}[name]()


def run_pass(eng, case, objs, name):
    """The pass of objs[name] into fresh output tensors, read back: a tuple of arrays.  The exclusions act in a repulsion pass of their
    own (and in the histogram's, where both are alive)."""
    import torch
    n = NCHAINS * BEADS

    def to4(a):
        o = np.zeros((n, 4)); o[:, :3] = a
        return torch.tensor(o, dtype=torch.float64, device="cuda")

    pos, obj = to4(case["pos"]), objs[name]
    if name == "exclusions":
        out = (eng.pair_repulsion(pos, torch.zeros_like(pos), 40.0, sigma=2.5, exclusions=obj),)
    elif name == "histogram":
        out = (eng.pair_hist_accumulate(pos, obj, torch.zeros((3, 8), dtype=torch.int64, device="cuda"), exclusions=objs.get("exclusions")),)
    elif name == "structure_factor":
        out = eng.structure_factor_accumulate(pos, obj, rho=torch.zeros((2, 6, 2), dtype=torch.float64, device="cuda"),
                                              sums=torch.zeros((3, 6), dtype=torch.float64, device="cuda"))
    elif name == "origins":
        image = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
        shift = 0.125 * ((np.arange(3 * n).reshape(n, 3) % 5) - 2.0)
        eng.msd_store(pos, image, obj, 0, 0.0)
        eng.msd_store(to4(case["pos"] + shift), image, obj, 1, 0.0)
        out = (eng.msd_accumulate(to4(case["pos"] - shift), image, obj, 0.0, [0, 1], [1, 0], torch.zeros((2, 2, 10), dtype=torch.float64, device="cuda")),
               eng.msd_displacement(pos, image, obj, 1, 0.0))
    else:
        out = eng.cluster_label(pos, obj, label=torch.zeros(n, dtype=torch.int32, device="cuda"), size=torch.zeros(n, dtype=torch.int32, device="cuda"),
                                stats=torch.zeros(4, dtype=torch.int64, device="cuda"), hist=torch.zeros(n, dtype=torch.int64, device="cuda"))
        assert obj.status() == 0
    return tuple(t.cpu().numpy() for t in out)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_collected_analysis_object_frees_its_arrays_and_leaves_the_rest(case):
    import pse_amd
    eng = pse_amd.Engine(NCHAINS * BEADS, BOX, xi=0.5, error=1e-3, seed=3)
    objs = {name: make(eng, case, name) for name in ANALYSIS}
    first = {name: run_pass(eng, case, objs, name) for name in ANALYSIS}
    assert first["exclusions"][0].any() and first["histogram"][0].sum() > 0 and np.abs(first["structure_factor"][0]).max() > 0.0
    assert first["origins"][0].any() and first["links"][2][0] < NCHAINS * BEADS               # something was linked
    dropped = (ANALYSIS[1], ANALYSIS[-1])
    with _Unraisable() as quiet:
        for name in dropped:
            del objs[name]
        gc.collect()                                               # pse_pair_hist_destroy and pse_clusters_destroy run here
    assert quiet.seen == []
    for name in objs:
        assert same(run_pass(eng, case, objs, name), first[name]), name
    for name in dropped:
        objs[name] = make(eng, case, name)
        assert same(run_pass(eng, case, objs, name), first[name]), name
    eng.close()


def test_the_analysis_objects_go_with_the_engine(case):
    import pse_amd
    eng = pse_amd.Engine(NCHAINS * BEADS, BOX, xi=0.5, error=1e-3, seed=3)
    objs = {name: make(eng, case, name) for name in ANALYSIS}
    eng.close()                                                    # pse_destroy freed the five device objects
    for name in ANALYSIS:
        with pytest.raises(ValueError, match="went with the engine"):
            run_pass(eng, case, {name: objs[name]}, name)
    with pytest.raises(ValueError, match="went with the engine"):
        objs["links"].status()
    with _Unraisable() as quiet:                                   # nothing is freed twice, nothing complains
        del objs
        gc.collect()
    assert quiet.seen == []
