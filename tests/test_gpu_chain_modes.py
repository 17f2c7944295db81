"""pse_chain_modes_compute, _store and _correlate and analyze.RouseModes on the device against the exact reference of
tests/chain_modes_ref.py: bit for bit on dyadic inputs (positions of conformation_cases.py, weights that are multiples of 1/2), where
the reference asserts that no sum can round in any order; within the bound derived from the order of operations on general positions
with Rouse weights at the wave, chunk and tile edges; the correlation pass at the block edges with one and 64 pairs; every output alone
and none; two calls; equal bits; a captured graph; a slab rank's handle; the analyzer through System.run under a shear that flips.
tests/test_chain_modes_cpu.py checks the same cases' margins with a float64 restatement of the kernels' order."""
import functools

import numpy as np
import pytest

from conftest import to4
import conformation_cases as cc
import chain_modes_ref as cm

pytestmark = pytest.mark.gpu

NMAX = 4400
NAMES = ("out", "sums", "sample")


@functools.lru_cache(maxsize=None)
def engine(lengths):
    import pse_amd
    return pse_amd.Engine(NMAX, lengths + (0.0,), xi=0.5, error=1e-3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    return bool(np.array_equal(bits(got), bits(want)))


class Modes:
    """One chain-modes object on the engine of the box's lengths, and the passes on it with NumPy in and out."""

    def __init__(self, box, n, bonds, tables, types=None, ntypes=1, norigins=0, eng=None):
        self.eng, self.box, self.ntypes = eng or engine(tuple(box[:3])), box, ntypes
        self.eng.set_box(*box)
        sizes = sorted(tables)
        self.obj = self.eng.chain_modes(bonds, sizes, [tables[m] for m in sizes], types, ntypes, norigins, n=n)
        self.K = self.obj.K

    def z(self, *shape, fill=0.0):
        import torch
        return torch.full(shape, fill, dtype=torch.float64, device="cuda")

    def compute(self, pos, calls=1, only=None, nothing=False):
        """`calls` computes from zeroed outputs: {out, sums, sample} as NumPy arrays; only=name: that output alone; nothing: none."""
        import torch
        o = self.obj
        out = dict(out=self.z(o.nlin, o.K, 3), sums=self.z(o.ntypes, o.K, 6), sample=self.z(o.ntypes, o.K, 6))
        if only is not None or nothing:
            out = {k: (v if k == only else None) for k, v in out.items()}
        p = to4(pos)
        for _ in range(calls):
            self.eng.chain_modes_compute(p, o, **out)
        torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}

    def correlate(self, slots, rows, corr):
        self.eng.chain_modes_correlate(self.obj, slots, rows, corr)

    def close(self):
        self.obj.close()
        self.eng.set_box(*(tuple(self.box[:3]) + (0.0,)))


# -- 1. dyadic inputs: bit for bit ---------------------------------------------------------------------------------------------------------

SECOND = {"shuffled chain": (2.0, 2.0 ** -8), "513 dimers": (3.0, 2.0 ** -4), "four 64": (1.0, 1.0)}   # (step, grid) of a second frame


@pytest.mark.parametrize("name", cm.DYADIC_NAMES)
def test_dyadic_inputs_bit_for_bit(name):
    """modes, sums and sample equal the exact reference, which asserted that nothing can round; the counts; two calls double sums and
    leave sample and modes; every bead moved by its own lattice vector gives equal bits; and, for the cases of chains of at most 64
    beads, the correlation with a stored second frame, twice."""
    box, n, bonds, pos, types, ntypes, tables = cm.dyadic(name)
    ref = cm.reference(pos, box, bonds, tables, types, ntypes, dyadic=True)
    md = Modes(box, n, bonds, tables, types, ntypes, norigins=2)
    got = md.compute(pos)
    assert same_bits(got["out"], ref["modes"]) and same_bits(got["sums"], ref["sums"]) and same_bits(got["sample"], ref["sums"])
    o = md.obj
    assert o.nmol == len(ref["mols"]) and o.nlin == len(ref["lin_mol"]) and np.array_equal(o.nlin_type, ref["nlin_type"])
    assert np.array_equal(o.lin_mol, ref["lin_mol"]) and np.array_equal(o.lin_size, ref["lin_size"])
    twice = md.compute(pos, calls=2)
    assert same_bits(twice["sums"], 2.0 * got["sums"]) and same_bits(twice["sample"], got["sample"]) and same_bits(twice["out"], got["out"])
    moved = cc.reimage(pos, box, np.random.default_rng(3))
    again = md.compute(moved)
    assert all(same_bits(again[k], got[k]) for k in NAMES)
    if name in SECOND:
        step, grid = SECOND[name]
        pos2 = cc.wrap(cc.place(n, bonds, box, np.random.default_rng(19), step, grid=grid), box)
        ref2 = cm.reference(pos2, box, bonds, tables, types, ntypes, dyadic=True)
        want = cm.correlate(ref2, ref, ntypes, dyadic=True)                       # now: the second frame; then: the first
        md.compute(pos)
        md.eng.chain_modes_store(o, 1)
        assert same_bits(md.compute(pos2)["out"], ref2["modes"])
        corr = md.z(3, ntypes, md.K, 3, 3)
        md.correlate([1], [2], corr)
        assert same_bits(corr.cpu().numpy()[2], want) and not corr.cpu().numpy()[:2].any()
        md.correlate([1], [2], corr)
        assert same_bits(corr.cpu().numpy()[2], 2.0 * want)
        assert np.any(want != np.swapaxes(want, -1, -2))                            # (the nine entries are not symmetric)
    md.close()


def test_three_caller_orders_of_one_chain():
    """One 64-bead chain on dyadic positions under the identity, the reversed and a random labelling: each equals its own reference."""
    rng = np.random.default_rng(23)
    n, bonds, _, _ = cc.build([("chain", 64)])
    box = (16.0, 16.0, 16.0, 0.25)
    pos = cc.place(n, bonds, box, rng, 2.0, grid=2.0 ** -8)
    tables = {64: cm.dyadic_weights(64, 6, rng)}
    seen = []
    for new_of_old in (np.arange(n), np.arange(n)[::-1].copy(), rng.permutation(n)):
        b2 = new_of_old[np.asarray(bonds)]
        p2 = np.empty_like(pos); p2[new_of_old] = pos
        p2 = cc.wrap(p2, box)
        ref = cm.reference(p2, box, b2, tables, dyadic=True)
        md = Modes(box, n, b2, tables)
        got = md.compute(p2)
        md.close()
        assert same_bits(got["out"], ref["modes"]) and same_bits(got["sums"], ref["sums"])
        seen.append(got["out"][0, 0])
    assert np.array_equal(seen[1], -seen[0])                                        # reversed: R changes its sign


# -- 2. general positions and Rouse weights: within the derived bound ----------------------------------------------------------------------

def _general(label, box, n, bonds, pos, types, ntypes, tables):
    ref = cm.reference(pos, box, bonds, tables, types, ntypes)
    md = Modes(box, n, bonds, tables, types, ntypes)
    got = md.compute(pos)
    o = md.obj
    assert o.nlin == len(ref["lin_mol"]) and np.array_equal(o.lin_mol, ref["lin_mol"]) and np.array_equal(o.lin_size, ref["lin_size"])
    assert np.array_equal(o.nlin_type, ref["nlin_type"]) and o.nmol == len(ref["mols"])
    md.close()
    tX = cm.bounds(ref, box)
    ts = cm.sums_bound(ref, tX, ntypes, len(cm.tiles_of(ref["mols"])[0]) - 1)
    ex, es = np.abs(got["out"] - ref["modes"]), np.abs(got["sums"] - ref["sums"])
    print(label, "modes: largest error / bound", (ex / np.maximum(tX, 1e-300)).max(), "sums:", (es / np.maximum(ts, 1e-300)).max())
    assert np.all(ex <= tX) and np.all(es <= ts) and same_bits(got["sample"], got["sums"])
    empty = ref["nlin_type"] == 0
    assert same_bits(got["sums"][empty], np.zeros((int(empty.sum()), md.K, 6)))     # a type without linear molecules: exactly +0.0
    return ref, got


@pytest.mark.parametrize("k", range(len(cc.EDGES)))
def test_sizes_at_the_wave_and_tile_edges_within_the_bound(k):
    """Sizes 2, 3, 63, 64, 65, 255, 257 and 1023, a tile filled to exactly 1024, a star, rings and a comb that are skipped, 1, 2 and 8
    types with empty ones, K = 9 with (padded) Rouse weights."""
    box, n, bonds, pos, types, ntypes, tables = cm.edge(k)
    ref, _ = _general(f"edge {k}", box, n, bonds, pos, types, ntypes, tables)
    assert sorted(set(ref["lin_size"].tolist())) == [2, 3, 63, 64, 65, 255, 257, 1023] and len(ref["lin_mol"]) < len(ref["mols"])


@pytest.mark.parametrize("name", cm.GENERAL_NAMES)
def test_a_1024_chain_a_tile_of_dimers_two_sizes_in_a_tile_and_the_extreme_K(name):
    box, n, bonds, pos, types, ntypes, tables = cm.general(name)
    ref, _ = _general(name, box, n, bonds, pos, types, ntypes, tables)
    if name == "1024 and dimers":
        assert ref["lin_size"].tolist() == [1024] + [2] * 512 + [20, 7, 20]
    else:
        assert ref["K"] in (1, 32)


# -- 3. the correlation pass at the block edges --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nlin", [1, 63, 64, 65, 255, 256, 257])
def test_correlate_at_the_block_edges_with_one_and_64_pairs(nlin):
    """nlin trimers of two types in general position, four frames: one pair; 64 pairs that name two slots for 32 rows each; a slot
    overwritten and used again; the row that no pair names keeps its bits.  Every entry within the bound of the exact correlation."""
    rng = np.random.default_rng(100 + nlin)
    n, bonds, _, _ = cc.build([("chain", 3)] * nlin)
    box = (16.0, 16.0, 16.0, 0.25)
    types, ntypes = (np.arange(nlin) % 2, 2) if nlin > 1 else (None, 1)
    tables = {3: cm.rouse_weights(3, 3)}
    base = cc.place(n, bonds, box, rng, 2.5)
    frames = [cc.wrap(base + rng.uniform(-0.2, 0.2, base.shape), box) for _ in range(4)]
    refs = [cm.reference(f, box, bonds, tables, types, ntypes) for f in frames]
    tol = [cm.bounds(r, box) for r in refs]

    def check(got, now, then, calls=1):
        exact = cm.correlate(refs[now], refs[then], ntypes)
        t = calls * cm.correlate_bound(refs[now], tol[now], refs[then], tol[then], ntypes, exact) + 2 * cc.EPS * np.abs(calls * exact)
        err = np.abs(got - calls * exact)
        assert np.all(err <= t), (now, then, (err / np.maximum(t, 1e-300)).max())
        return (err / np.maximum(t, 1e-300)).max()

    md = Modes(box, n, bonds, tables, types, ntypes, norigins=3)
    e, o = md.eng, md.obj
    md.compute(frames[0]); e.chain_modes_store(o, 0)
    md.compute(frames[1]); e.chain_modes_store(o, 2)
    md.compute(frames[2])
    corr = md.z(66, ntypes, md.K, 3, 3)
    corr[65] = -7.0
    md.correlate([0], [0], corr)                                                    # one pair
    slots = [0, 2] * 32
    md.correlate(slots, list(range(1, 65)), corr)                                   # 64 pairs, a slot listed for many rows
    c = corr.cpu().numpy()
    worst = check(c[0], 2, 0)
    for row in range(1, 65):
        assert same_bits(c[row], c[1 if slots[row - 1] == 0 else 2])                # equal inputs give equal bits
    assert same_bits(c[1], c[0])
    worst = max(worst, check(c[2], 2, 1))
    assert np.all(c[65] == -7.0)                                                    # a row that no pair names is untouched
    e.chain_modes_store(o, 0)                                                       # the slot overwritten (frame 2) and used again
    md.compute(frames[3])
    corr[65] = 0.0
    md.correlate([0, 2], [65, 0], corr)
    c2 = corr.cpu().numpy()
    worst = max(worst, check(c2[65], 3, 2))
    assert np.all(np.abs(c2[0] - c[0] - cm.correlate(refs[3], refs[1], ntypes)) <= 2 * cm.correlate_bound(refs[3], tol[3], refs[1], tol[1], ntypes, c2[0]))
    assert same_bits(c2[1:65], c[1:65])
    print("corr: largest error / bound", worst)
    md.close()


# -- 4. the outputs ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("only", NAMES)
def test_every_output_alone_gives_the_bits_of_the_full_call(only):
    box, n, bonds, pos, types, ntypes, tables = cm.edge(2)
    md = Modes(box, n, bonds, tables, types, ntypes)
    full = md.compute(pos)
    alone = md.compute(pos, only=only)
    md.close()
    assert all(alone[k] is None for k in NAMES if k != only) and same_bits(alone[only], full[only])


def test_no_output_at_all_is_followed_by_a_correct_correlate_and_equal_calls_give_equal_bits():
    """compute with modes, sums and sample all NULL still fills the current buffer: the correlation that follows is the exact one
    (dyadic inputs).  The same calls a second time, on a second object, give identical bits (general positions)."""
    box, n, bonds, pos, types, ntypes, tables = cm.dyadic("four 64")
    pos2 = cc.wrap(cc.place(n, bonds, box, np.random.default_rng(19), 1.0, grid=1.0), box)
    ref, ref2 = (cm.reference(p, box, bonds, tables, types, ntypes, dyadic=True) for p in (pos, pos2))
    md = Modes(box, n, bonds, tables, types, ntypes, norigins=1)
    assert all(v is None for v in md.compute(pos, nothing=True).values())
    md.eng.chain_modes_store(md.obj, 0)
    md.compute(pos2, nothing=True)
    corr = md.z(1, ntypes, md.K, 3, 3)
    md.correlate([0], [0], corr)
    assert same_bits(corr.cpu().numpy()[0], cm.correlate(ref2, ref, ntypes, dyadic=True))
    md.close()
    box, n, bonds, pos, types, ntypes, tables = cm.edge(3)
    pos2 = cc.wrap(pos + 0.125, box)
    runs = []
    for _ in range(2):
        md = Modes(box, n, bonds, tables, types, ntypes, norigins=2)
        first = md.compute(pos)
        md.eng.chain_modes_store(md.obj, 1)
        second = md.compute(pos2)
        corr = md.z(2, ntypes, md.K, 3, 3)
        md.correlate([1, 1], [1, 0], corr)
        runs.append([first[k] for k in NAMES] + [second[k] for k in NAMES] + [corr.cpu().numpy()])
        md.close()
    assert all(same_bits(a, b) for a, b in zip(*runs)) and runs[0][-1].any() and same_bits(runs[0][-1][0], runs[0][-1][1])


# -- 5. queue-only: a captured graph -------------------------------------------------------------------------------------------------------

def test_compute_correlate_and_store_captured_into_a_graph_replay_the_eager_bits():
    import torch
    import pse_amd
    box, n, bonds, pos, types, ntypes, tables = cm.edge(2)
    frames = [pos, cc.wrap(pos + 0.125, box), cc.wrap(pos - 0.0625, box)]
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    md = Modes(box, n, bonds, tables, types, ntypes, norigins=2, eng=eng)
    o = md.obj
    p = to4(pos)
    out = dict(out=md.z(o.nlin, o.K, 3), sums=md.z(ntypes, o.K, 6), sample=md.z(ntypes, o.K, 6))
    corr = md.z(2, ntypes, o.K, 3, 3)
    everything = dict(out, corr=corr)

    def sample():                                                                    # one stream, no parallel branches
        eng.chain_modes_compute(p, o, **out)
        eng.chain_modes_correlate(o, [1], [0], corr)
        eng.chain_modes_store(o, 1)

    def start():
        p.copy_(to4(frames[0]))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            eng.chain_modes_compute(p, o)
            eng.chain_modes_store(o, 1)
        st.synchronize()
        for v in everything.values():
            v.zero_()
        torch.cuda.synchronize()

    start()
    eager = []
    for f in frames[1:]:
        p.copy_(to4(f))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            sample()
        st.synchronize()
        eager.append({k: v.cpu().numpy().copy() for k, v in everything.items()})
    assert np.abs(eager[1]["corr"] - 2.0 * eager[0]["corr"]).max() > 0.0 and not eager[0]["corr"][1].any()
    start()
    p.copy_(to4(frames[1]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        sample()
    torch.cuda.synchronize()
    assert not corr.cpu().numpy().any() and not out["sums"].cpu().numpy().any(), "a capture runs nothing"
    for k, f in enumerate(frames[1:]):
        p.copy_(to4(f))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for name, v in everything.items():
            assert same_bits(v.cpu().numpy(), eager[k][name]), (k, name)
    o.close()
    eng.close()


# -- 6. a slab rank's handle ---------------------------------------------------------------------------------------------------------------

def test_a_slab_rank_gives_the_bits_of_the_reference():
    """Positions are replicated on a slab rank, so the passes are complete there: the dyadic chains of "four 64", unfolded and wrapped
    into a box of 32^3 on the handle of rank 0 of 2 -- the offsets are the same numbers -- give the reference's bits, correlation included."""
    import pse_amd
    import conformation_ref as cr
    box, n, bonds, pos, types, ntypes, tables = cm.dyadic("four 64")
    pos2 = cc.wrap(cc.place(n, bonds, box, np.random.default_rng(19), 1.0, grid=1.0), box)
    ref, ref2 = (cm.reference(p, box, bonds, tables, types, ntypes, dyadic=True) for p in (pos, pos2))
    box_s = (32.0, 32.0, 32.0, 0.0)
    eng = pse_amd.Engine(n, box_s, xi=0.5, error=1e-3, grid=(48, 48, 48), n_slabs=2, slab_rank=0)
    md = Modes(box_s, n, bonds, tables, types, ntypes, norigins=1, eng=eng)
    wide = [cc.wrap(cr.reference(p, box, bonds, types, ntypes)["unfolded"][:, :3], box_s) for p in (pos, pos2)]
    got = md.compute(wide[0])
    assert same_bits(got["out"], ref["modes"]) and same_bits(got["sums"], ref["sums"])
    eng.chain_modes_store(md.obj, 0)
    md.compute(wide[1])
    corr = md.z(1, ntypes, md.K, 3, 3)
    md.correlate([0], [0], corr)
    assert same_bits(corr.cpu().numpy()[0], cm.correlate(ref2, ref, ntypes, dyadic=True))
    md.obj.close()
    eng.close()


# -- 7. analyze.RouseModes on a System -----------------------------------------------------------------------------------------------------

@pytest.fixture
def restored_context():
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


class Snapshots:
    def __init__(self, system):
        self.system, self.frames = system, []
        system.analyzers.append(self)

    def analyze(self, timestep):
        s = self.system
        self.frames.append((int(timestep), s.pos.cpu().numpy()[:, :3].copy(), tuple(s.box)))


class PrescribedMotion:
    """An integrator for System.run that moves the particles with fixed velocities (Engine.integrate with a shear rate) on an engine
    of its own: what an analyzer needs of an integrator (system, group, engine) and System of one (update, set_box)."""

    def __init__(self, system, vel, rate):
        import pse_amd
        from pse_amd.system import Group
        self.system, self.group, self.rate = system, Group(system), rate
        self.engine = pse_amd.Engine(system.n, system.box, xi=0.5, error=1e-3)
        system.vel[:, :3] = to4(vel)[:, :3]
        system.integrators.append(self)

    def set_box(self, box):
        self.engine.set_box(*box)

    def update(self, timestep):
        s = self.system
        self.engine.integrate(s.pos, s.vel, s.accel, s.image, s.net_force, s.dt, shear_rate=self.rate)


def test_analyzer_through_system_run_under_a_shear_that_flips(restored_context):
    """analyze.RouseModes on chains that move with prescribed velocities -- every chain drifts through the faces of the box, its beads
    drift apart slowly -- under a steady shear whose box flips at step 16: amplitudes and correlation_tensor within the bound of the
    exact reference evaluated on the recorded positions of every sampled step; counts equal a brute-force count; the normalised
    autocorrelation is 1 at lag 0; the readers take no sample; reset() clears everything."""
    import pse_amd
    from pse_amd import analyze, shear_function, variant
    from pse_amd.system import System
    rng = np.random.default_rng(77)
    shapes = [("chain", 8)] * 3 + [("chain", 5)] * 2 + [("star", 6), ("ring", 4)]
    n, bonds, sizes, kinds = cc.build(shapes, gaps=(0, 1))
    n += 1
    box0 = (16.0, 16.0, 16.0, 0.0)
    dt, rate = 2.0 ** -6, 2.0                                                  # the tilt grows by 1/32 per step: the flip at step 16
    pos0 = cc.place(n, bonds, box0, rng, 1.5, grid=2.0 ** -6)
    cc.ring_place(pos0, n - 5, 4, 1.0, rng, grid=2.0 ** -6)                    # (the ring: the last four bonded particles)
    s = System(cc.wrap(pos0, box0), box0, dt=dt)
    mol_of = analyze.molecules_of(n, bonds)[0]
    drift = rng.integers(-24, 25, (7, 3)).astype(np.float64)                   # per molecule: up to 11 length units in the run, through the faces
    vel = np.where(mol_of[:, None] >= 0, drift[np.maximum(mol_of, 0)], 0.0) + rng.integers(-4, 5, (n, 3)) / 4.0
    mover = PrescribedMotion(s, vel, rate)
    s.box_tilt_variant = variant.shear_variant(shear_function.steady(dt=dt, shear_rate=rate), 100000, max_strain=0.5)
    nmodes, nlags, every, period = 3, 4, 2, 3
    rm = analyze.RouseModes(mover, bonds, nmodes=nmodes, nlags=nlags, origin_every=every, molecule_types="size",
                            type_names=["four", "five", "six", "eight"], period=period)
    K = nmodes + 1
    assert rm.K == K and rm.ntypes == 4 and rm.nlin == 5 and rm.nmol == 7 and list(rm.nlin_type) == [0, 2, 0, 3]
    assert list(rm.linear_sizes) == [5, 8] and list(rm.lin_size) == [8, 8, 8, 5, 5] and np.array_equal(rm.lags, period * np.arange(1, nlags + 1))
    snaps = Snapshots(s)
    s.run(30)
    assert s.tilt_flips >= 1
    sampled = [f for f in snaps.frames if f[0] % period == 0]
    assert rm.samples == len(sampled) == 10
    types = np.searchsorted(rm.size_values, sizes)
    tables = {int(m): pse_amd.host_rouse_weights(int(m), K) for m in rm.linear_sizes}
    refs = [cm.reference(p, b, bonds, tables, types, 4) for _, p, b in sampled]
    tols = [cm.bounds(r, b) for r, (_, _, b) in zip(refs, sampled)]
    # the static amplitudes: the sum over the samples of the exact sums
    total = sum(r["sums"] for r in refs)
    ttol = sum(cm.sums_bound(r, t, 4, 1) for r, t in zip(refs, tols)) + 16 * cc.EPS * np.abs(total)
    got = rm._sums.cpu().numpy()
    assert np.all(np.abs(got - total) <= ttol)
    amp = rm.amplitudes("eight")
    assert amp.shape == (K,) and np.allclose(amp, total[3, :, :3].sum(axis=1) / (10 * 3), rtol=1e-12)
    assert np.allclose(rm.amplitudes(), total[:, :, :3].sum(axis=(0, 2)) / (10 * 5), rtol=1e-12)
    assert np.isnan(rm.amplitudes("six")).all() and np.isnan(rm.amplitude_tensor("four")).all() and rm.amplitude_tensor().shape == (K, 3, 3)
    # the correlations: brute force over every pair (origin sample, later sample) that the schedule admits
    want, wtol, counts = np.zeros((nlags, 4, K, 3, 3)), np.zeros((nlags, 4, K, 3, 3)), np.zeros(nlags, dtype=np.int64)
    for i in range(0, 10, every):
        for lag in range(1, nlags + 1):
            if i + lag < 10:
                exact = cm.correlate(refs[i + lag], refs[i], 4)
                want[lag - 1] += exact
                wtol[lag - 1] += cm.correlate_bound(refs[i + lag], tols[i + lag], refs[i], tols[i], 4, exact)
                counts[lag - 1] += 1
    assert np.array_equal(rm.counts, counts) and counts.min() >= 3
    corr = rm._corr.cpu().numpy()
    err = np.abs(corr - want)
    print("corr: largest error / bound", (err / np.maximum(wtol + 16 * cc.EPS * np.abs(want), 1e-300)).max())
    assert np.all(err <= wtol + 16 * cc.EPS * np.abs(want))
    ct = rm.correlation_tensor("eight")
    assert ct.shape == (nlags, K, 3, 3) and np.allclose(ct, want[:, 3] / (counts[:, None, None, None] * 3), rtol=1e-9, atol=1e-12)
    assert np.any(np.abs(ct[..., 0, 1] - ct[..., 1, 0]) > 1e-6)                   # under shear xy and yx differ
    ac = rm.autocorrelation()
    assert ac.shape == (nlags + 1, K) and np.all(ac[0] == 1.0)
    assert np.allclose(ac[1:], np.trace(want.sum(axis=1), axis1=-2, axis2=-1) / (counts[:, None] * 5) / rm.amplitudes()[None, :], rtol=1e-9)
    assert np.isnan(rm.autocorrelation("four")).all() and rm.relaxation_times().shape == (K,)
    # per_molecule(): the current positions; row 0 is R, whose weights are -1 and +1: exact on these dyadic positions
    pos, box = s.pos.cpu().numpy()[:, :3].copy(), tuple(s.box)
    ref = cm.reference(pos, box, bonds, tables, types, 4)
    pm = rm.per_molecule()
    assert pm.shape == (5, K, 3) and np.all(np.abs(pm - ref["modes"]) <= cm.bounds(ref, box)) and same_bits(pm[:, 0], ref["modes"][:, 0])
    assert rm.samples == 10                                                         # the readers took no sample
    rm.reset()
    assert rm.samples == 0 and not rm._sums.cpu().numpy().any() and not rm._corr.cpu().numpy().any() and not rm.counts.any()
    with pytest.raises(ValueError, match="no samples"):
        rm.amplitudes()
    s.run(3)
    assert rm.samples == 1 and not rm.counts.any() and np.isnan(rm.correlation_tensor()).all()
    mover.engine.close()
