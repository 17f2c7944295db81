"""GPU tests of the typed pair tables (pse_typed_table_create, pse_pair_table_typed): forces, energy, virial and pair count against the
O(N^2) reference of tests/pair_typed_ref.py (validated on the CPU by tests/test_pair_typed_cpu.py) over the wave / workgroup edges,
the numbers of types, the table widths and ranges, every call form, a group, the bit-identities (labels swapped, calls repeated, an
exclusion object that excludes nothing in range), the plain pass on the same table, exclusions on chains, the many-cell grids of
tests/cell_grid_cases.py, the error returns of the raw C-ABI, and the provider on top (forces.TypedTablePair, forces.StressLog).

Bound: the plain table pass's own (tests/test_gpu_pair_table.py), 1e-11 max(1, max |ref|) per quantity -- the eight observables
together, the forces together; npairs must match exactly.  check_obs and check_forces are restated here."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
import cell_grid_cases as cg
import pair_table_ref
import pair_typed_ref as tr
from pair_table_ref import harmonic_table, morse_table, random_points

pytestmark = pytest.mark.gpu

NMAX = 513
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
N = 300
K = 40.0
INVALID = -1
CAP = 3584
MORSE = dict(D=5.0, alpha=2.0, r0=1.5)          # F > 0 inside r0 = 1.5, F < 0 outside
A, B, C = 0, 1, 2


def port():
    from oracle import pse_port
    pse_port.lib()
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(NMAX, box, xi=0.5, error=1e-3)


def rcut(box):
    return engine(box).info()["rcut"]


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


def morse(rmin, rmax, width, r0=1.5):
    return morse_table(D=5.0, alpha=2.0, r0=r0, rmin=rmin, rmax=rmax, width=width), rmin, rmax


W2 = (np.array([[3.0, 5.0], [-1.0, -2.0]]), 0.0, 2.0)        # the index clamp is the only path; V and F change sign along the one interval


@functools.lru_cache(maxsize=None)
def tables_case(name, box):
    """(ntypes, {(a, b): (table, rmin, rmax)}) by name.  Every table has F of both signs."""
    if name == "nt1":
        return 1, {(0, 0): morse(0.7, 3.0, 1000)}
    if name == "nt2":           # what the row counts and most other tests use: three ranges, rmin > 0 twice
        return 2, {(A, A): morse(0.7, 3.0, 1000), (B, A): morse(0.0, 2.0, 512, r0=1.2), (B, B): morse(1.0, 2.8, 300)}
    if name == "nt2_w2":        # width 2 next to width 1000, and one pair type off
        return 2, {(A, A): W2, (A, B): morse(0.7, 3.0, 1000)}
    if name == "nt3":           # five of six pair types on, B-B off, in either order of the keys
        return 3, {(A, A): morse(0.7, 3.0, 1000), (B, A): morse(0.0, 2.0, 1024, r0=1.2), (A, C): morse(1.0, 2.8, 300),
                   (C, B): morse(0.5, 2.0, 257, r0=1.0), (C, C): morse(0.7, 2.5, 500)}
    if name == "nt8":           # 36 pair types, every third one off, widths and ranges all different
        t = {}
        for a in range(8):
            for b in range(a, 8):
                p = tr.pair_index(a, b, 8)
                if p % 3 != 2:
                    t[(a, b) if p % 2 else (b, a)] = morse(0.2 * (p % 5), 2.2 + 0.05 * p, 40 + 3 * p, r0=1.1 + 0.01 * p)
        return 8, t
    if name == "cap":           # the widths sum to the cap exactly: 56 KB of LDS
        return 2, {(A, A): morse(0.7, 3.0, 2048), (A, B): morse(0.0, 2.5, 1024), (B, B): morse(0.5, 2.0, 512, r0=1.2)}
    if name == "rcut":          # one pair type over the whole range of the cell list, another far inside it: the common prefilter
        rc = rcut(box)          # lets every A-B pair below rcut through, the pair type's own test must stop it at 1.5
        return 2, {(A, A): morse(0.0, rc, 1000), (A, B): morse(0.5, 1.5, 200, r0=1.0), (B, B): morse(0.7, 3.0, 500)}
    raise KeyError(name)


def types_of(n, ntypes, seed=21):
    return np.random.default_rng(seed).integers(0, ntypes, n)


@functools.lru_cache(maxsize=None)
def case(name, box, n=N, seed=11):
    """(pos, types, ntypes, tables, obs, F): computed once, shared, never written to."""
    ntypes, tables = tables_case(name, box)
    pos, types = random_points(n, box, seed), types_of(n, ntypes)
    obs, F = tr.typed_observables(pos, box, types, ntypes, tables, port())
    for a in (pos, types, obs, F):
        a.setflags(write=False)
    return pos, types, ntypes, tables, obs, F


def typed(eng, types, tables, n=None):
    return eng.typed_table(types, tables, n)


def run(eng, pos, types, tables, w=3.0, **kw):
    """One stored call on a new object: (out8 as NumPy, force rows as NumPy)."""
    f = to4(np.zeros((len(pos), 3)), w)
    tt = typed(eng, types, tables)
    out = eng.pair_table_typed(to4(pos), f, tt, accumulate=False, **kw)
    out, g = out.cpu().numpy(), f.cpu().numpy()
    tt.close()
    return out, g


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_row_counts(n, box):
    """A partial last wave, a full one, one lane of the next; the same for the 256-thread workgroup; 513: three workgroup rows; 1: no
    pair at all.  n = 2: the pair placed by hand, once as A-B, and once as A-A with A-A off: exactly zeros."""
    ntypes, tables = tables_case("nt2", box)
    pos = random_points(n, box, seed=100 + n)
    types = types_of(n, ntypes, seed=n)
    if n == 2:
        pos[1] = pos[0] + np.array([0.9, -0.7, 0.4])
        types = np.array([A, B])
    ref, F = tr.typed_observables(pos, box, types, ntypes, tables, port())
    if n == 1:
        assert not ref.any()
    else:
        assert ref[7] >= 1 and (n < 63 or ref[7] >= 10)
    if n >= 63:
        assert set(types.tolist()) == {A, B}
    out, g = run(engine(box), pos, types, tables)
    check_obs(out, ref, f"n={n}")
    check_forces(g[:, :3], F, f"n={n}")
    assert np.all(g[:, 3] == 3.0)
    if n == 2:
        off = {k: v for k, v in tables.items() if k != (A, A)}
        out, g = run(engine(box), pos, np.array([A, A]), off)
        assert not out.any() and not g[:, :3].any() and np.all(g[:, 3] == 3.0)          # A-A is off: nothing, exactly
        out, g = run(engine(box), pos, np.array([A, A]), tables)
        assert out[7] == 1.0 and g[:, :3].any()                                       # ... and it is the type that does it


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("name", ["nt1", "nt2", "nt2_w2", "nt3", "nt8", "cap", "rcut"])
def test_tables(name, box):
    import torch
    pos, types, ntypes, tables, ref, F = case(name, box)
    counts = tr.pairs_in_range(pos, box, types, ntypes, tables, port())
    assert ref[7] > 20 and min(counts.values()) >= 1, counts
    if name != "nt8":
        assert min(counts.values()) >= 20, counts
    assert any(v >= 1 for v in tr.pairs_below_rmin(pos, box, types, ntypes, tables, port()).values())
    for t, _, _ in tables.values():
        assert (t[:, 1] > 0).any() and (t[:, 1] < 0).any()                    # a sign error in F or W cannot cancel
    total = sum(len(t) for t, _, _ in tables.values())
    if name == "cap":
        assert total == CAP
    if name == "rcut":          # A-B pairs between the pair type's rmax and the common prefilter's do exist
        wide = dict(tables)
        wide[(A, B)] = morse(0.5, 3.0, 200, r0=1.0)
        assert tr.pairs_in_range(pos, box, types, ntypes, wide, port())[tr.pair_index(A, B, 2)] > counts[tr.pair_index(A, B, 2)] + 20
    if name in ("nt2_w2", "nt3", "nt8"):
        assert len(tables) < ntypes * (ntypes + 1) // 2                        # a pair type is off
    eng = engine(box)
    f = to4(np.zeros((N, 3)), 7.0)
    tt = typed(eng, types, tables)
    assert tt.ntypes == ntypes and tt.count == total
    out = eng.pair_table_typed(to4(pos), f, tt, accumulate=False)
    assert out.shape == (8,) and out.is_cuda and out.dtype == torch.float64
    check_obs(out.cpu().numpy(), ref, f"{name} ntypes={ntypes} entries={total}")
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, name)
    assert np.all(g[:, 3] == 7.0)
    tt.close()


def test_call_forms():
    import torch
    import pse_amd
    box = TILTED
    eng = engine(box)
    pos, types, ntypes, tables, ref, F = case("nt3", box)
    dpos, tt = to4(pos), typed(eng, types, tables)
    base = np.random.default_rng(5).normal(size=(N, 3))
    # accumulate = 0: overwritten, w kept; accumulate = 1: added
    f0 = to4(base, 7.0)
    check_obs(eng.pair_table_typed(dpos, f0, tt, accumulate=False).cpu().numpy(), ref, "accumulate=0")
    g0 = f0.cpu().numpy()
    check_forces(g0[:, :3], F, "accumulate=0")
    f1 = to4(base, 7.0)
    check_obs(eng.pair_table_typed(dpos, f1, tt, accumulate=True).cpu().numpy(), ref, "accumulate=1")
    g1 = f1.cpu().numpy()
    check_forces(g1[:, :3] - base, F, "accumulate=1")
    assert np.all(g0[:, 3] == 7.0) and np.all(g1[:, 3] == 7.0)
    # force = None: the same eight numbers
    c = eng.pair_table_typed(dpos, None, tt).cpu().numpy()
    check_obs(c, ref, "force=None")
    # observables = False: the same forces, `out` is not touched, nothing is returned
    out = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    for acc, want in ((False, F), (True, F + base)):
        f2 = to4(base, 7.0)
        assert eng.pair_table_typed(dpos, f2, tt, accumulate=acc, out=out, observables=False) is None
        g2 = f2.cpu().numpy()
        check_forces(g2[:, :3], want, f"observables=False accumulate={acc}")
        assert np.all(g2[:, 3] == 7.0)
    assert np.isnan(out.cpu().numpy()).all()
    # a row of a log: only that row is written
    log = torch.full((6, 8), float("nan"), dtype=torch.float64, device="cuda")
    ret = eng.pair_table_typed(dpos, None, tt, out=log[3])
    assert ret.data_ptr() == log[3].data_ptr()
    host = log.cpu().numpy()
    assert np.array_equal(host[3], c) and np.isnan(np.delete(host, 3, axis=0)).all()
    # neither forces nor observables: refused by the C-ABI
    with pytest.raises(Exception, match="both null"):
        eng.pair_table_typed(dpos, None, tt, observables=False)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], pos)
    # the owner object: another engine, closed
    other = pse_amd.Engine(N, box, xi=0.5, error=1e-3)
    with pytest.raises(ValueError, match="another engine"):
        other.pair_table_typed(dpos, None, tt)
    other.close()
    tt.close()
    tt.close()
    with pytest.raises(ValueError, match="closed"):
        eng.pair_table_typed(dpos, None, tt)
    # the tables dictionary: both orders of one pair
    with pytest.raises(ValueError, match="both"):
        eng.typed_table(types, {(A, B): tables[(A, A)], (B, A): tables[(A, A)]})
    # a type the C-ABI refuses, by name
    with pytest.raises(pse_amd.PSEError, match="rcut"):
        eng.typed_table(types, {(A, A): morse(0.0, 7.0, 10)})


def test_group_counts_only_its_members_and_a_short_type_array():
    import torch
    box = TILTED
    eng = engine(box)
    pos, types, ntypes, tables, _, _ = case("nt3", box)
    members = np.arange(0, N, 2)
    ref, F = tr.typed_observables(pos[members], box, types[members], ntypes, tables, port())
    assert ref[7] > 5
    sentinel = np.random.default_rng(9).normal(size=(N, 3))
    f = to4(sentinel, 7.0)
    group = torch.tensor(members, dtype=torch.int32, device="cuda")
    tt = typed(eng, types, tables)
    out = eng.pair_table_typed(to4(pos), f, tt, group=group, accumulate=False).cpu().numpy()
    check_obs(out, ref, "group of every other particle")
    g = f.cpu().numpy()
    check_forces(g[members, :3], F, "group")
    assert np.array_equal(g[1::2, :3], sentinel[1::2]) and np.all(g[:, 3] == 7.0)       # non-members untouched
    tt.close()
    # types for the first 100 particles only: the others act as type 0
    short = typed(eng, types, tables, n=100)
    assert short.n == 100
    as0 = np.where(np.arange(N) < 100, types, 0)
    ref, F = tr.typed_observables(pos, box, as0, ntypes, tables, port())
    f = to4(np.zeros((N, 3)), 7.0)
    out = eng.pair_table_typed(to4(pos), f, short, accumulate=False).cpu().numpy()
    check_obs(out, ref, "types for 100 of 300")
    check_forces(f.cpu().numpy()[:, :3], F, "types for 100 of 300")
    assert not np.array_equal(ref, case("nt3", box)[4])
    short.close()


def test_bit_identities():
    """Labels swapped together with their tables; the same call twice; again after another entry point; an exclusion object with
    nothing in range against none: the same bits every time."""
    box = TILTED
    eng = engine(box)
    pos, types, ntypes, tables, ref, F = case("nt3", box)
    dpos = to4(pos)
    tt = typed(eng, types, tables)
    fa, fb, fc, fd, fe = (to4(np.zeros((N, 3))) for _ in range(5))
    a = eng.pair_table_typed(dpos, fa, tt, accumulate=False).cpu().numpy()
    b = eng.pair_table_typed(dpos, fb, tt, accumulate=False).cpu().numpy()
    check_obs(a, ref, "first call")
    assert np.array_equal(a, b) and np.array_equal(fa.cpu().numpy(), fb.cpu().numpy())
    other = random_points(N, box, seed=77)
    eng.mobility(to4(other), to4(np.random.default_rng(1).normal(size=(N, 3))))
    c = eng.pair_table_typed(dpos, fc, tt, accumulate=False).cpu().numpy()
    assert np.array_equal(a, c) and np.array_equal(fa.cpu().numpy(), fc.cpu().numpy())
    # A <-> C: the tables lie elsewhere in the stage, every pair finds the same numbers
    swap = {A: C, B: B, C: A}
    relabelled = {(swap[k[0]], swap[k[1]]): v for k, v in tables.items()}
    assert not np.array_equal(tr.arrays(relabelled, ntypes)[0], tr.arrays(tables, ntypes)[0])          # (the widths by pair type: another layout)
    ts = typed(eng, np.array([swap[t] for t in types.tolist()]), relabelled)
    d = eng.pair_table_typed(dpos, fd, ts, accumulate=False).cpu().numpy()
    assert np.array_equal(a, d) and np.array_equal(fa.cpu().numpy(), fd.cpu().numpy())
    # exclusions none of which is in range of its pair type's table
    i, j = tr.typed_terms(pos, box, types, ntypes, tables, port())[:2]
    acting = set(zip(i.tolist(), j.tolist()))
    rng = np.random.default_rng(3)
    far = [p for p in np.sort(rng.integers(0, N, (400, 2)), axis=1).tolist() if p[0] != p[1] and tuple(p) not in acting]
    assert len(far) > 300
    ex = eng.exclusions(np.array(far))
    e = eng.pair_table_typed(dpos, fe, tt, accumulate=False, exclusions=ex).cpu().numpy()
    assert np.array_equal(a, e) and np.array_equal(fa.cpu().numpy(), fe.cpu().numpy())
    for o in (ex, ts, tt):
        o.close()


@pytest.mark.parametrize("ntypes", [1, 3])
def test_agrees_with_the_plain_pass_on_one_table(ntypes):
    import torch
    box = TILTED
    eng = engine(box)
    pos = random_points(N, box, seed=11)
    table, rmin, rmax = morse(0.7, 3.0, 1000 if ntypes == 1 else 500)          # (six copies of the table share the stage)
    types = types_of(N, ntypes)
    assert len(set(types.tolist())) == ntypes
    tables = {(a, b): (table, rmin, rmax) for a in range(ntypes) for b in range(a, ntypes)}
    ref, F = pair_table_ref.pair_observables(pos, box, table, rmin, rmax, port())
    fp, ft = to4(np.zeros((N, 3))), to4(np.zeros((N, 3)))
    plain = eng.pair_table(to4(pos), fp, torch.tensor(table, dtype=torch.float64, device="cuda"), rmin, rmax, accumulate=False).cpu().numpy()
    tt = typed(eng, types, tables)
    got = eng.pair_table_typed(to4(pos), ft, tt, accumulate=False).cpu().numpy()
    check_obs(got, ref, f"typed, ntypes={ntypes}, against the plain reference")
    check_obs(got, plain, f"typed, ntypes={ntypes}, against pse_pair_table")
    assert got[7] == plain[7] > 20
    check_forces(ft.cpu().numpy()[:, :3], fp.cpu().numpy()[:, :3], "typed against pse_pair_table")
    tt.close()


def chains(box, nchains=30, beads=10, seed=4):
    """Chains of `beads` beads a step of 0.95 apart, types alternating along each: (pos, types, bonds, angles)."""
    rng = np.random.default_rng(seed)
    start = random_points(nchains, box, seed)
    pos, bonds, angles = [], [], []
    for c in range(nchains):
        p = start[c]
        for q in range(beads):
            i = c * beads + q
            pos.append(p)
            if q + 1 < beads:
                bonds.append([i, i + 1])
            if q + 2 < beads:
                angles.append([i, i + 1, i + 2])
            u = rng.normal(size=3)
            p = p + 0.95 * u / np.linalg.norm(u)
    types = np.tile(np.arange(beads) % 2, nchains)
    return cg.wrap(np.array(pos), box), types, np.array(bonds), np.array(angles)


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
def test_exclusions_on_chains_of_alternating_types(box):
    from pse_amd.forces import exclusion_pairs
    eng = engine(box)
    ntypes, tables = tables_case("nt2", box)
    pos, types, bonds, angles = chains(box)
    excl = exclusion_pairs(bonds, angles)                                     # 1-2 pairs are A-B, 1-3 pairs A-A and B-B
    i, j, _, _, _, _, p = tr.typed_terms(pos, box, types, ntypes, tables, port())
    gone = ~tr.exclusion_ref.kept_mask(i, j, excl)
    for q in range(3):
        assert (gone & (p == q)).sum() >= 5, (q, int((gone & (p == q)).sum()))          # excluded pairs in range, of every pair type
    ref, F = tr.typed_observables(pos, box, types, ntypes, tables, port(), excl)
    everything = tr.typed_observables(pos, box, types, ntypes, tables, port())[0]
    assert ref[7] == everything[7] - gone.sum() and ref[7] > 20
    tt, ex = typed(eng, types, tables), eng.exclusions(excl)
    f = to4(np.zeros((N, 3)), 7.0)
    out = eng.pair_table_typed(to4(pos), f, tt, accumulate=False, exclusions=ex).cpu().numpy()
    check_obs(out, ref, "chains with exclusions")
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, "chains with exclusions")
    assert np.all(g[:, 3] == 7.0)
    check_obs(eng.pair_table_typed(to4(pos), None, tt).cpu().numpy(), everything, "chains, nothing excluded")
    # a group: exclusions and types are caller indices
    import torch
    members = np.sort(np.random.default_rng(6).choice(N, 200, replace=False))
    ref, F = tr.typed_observables(pos[members], box, types[members], ntypes, tables, port(), excl, ids=members)
    f = to4(np.zeros((N, 3)), 7.0)
    out = eng.pair_table_typed(to4(pos), f, tt, group=torch.tensor(members, dtype=torch.int32, device="cuda"), accumulate=False,
                               exclusions=ex).cpu().numpy()
    check_obs(out, ref, "chains with exclusions, group")
    check_forces(f.cpu().numpy()[members, :3], F, "chains with exclusions, group")
    ex.close()
    tt.close()


# -- many-cell grids -------------------------------------------------------------------------------------------------------------------

GRID_NAMES = ("blocked_padded", "blocked_tilt_neg", "one_cell_x")
CUTOFF_TYPE = {"rmax": (A, A), "rmin": (A, A), "rcut": (A, B), "sigma": (B, B)}      # the pair type whose range ends at that cutoff


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """(case, types, tables, obs, F): the configuration unchanged; the first seeded type assignment with, for every cutoff the case
    plants pairs around, a planted pair inside and one outside that have exactly the pair type whose range ends there."""
    c = cg.build(name, port())
    tables = {(A, A): morse(cg.RMIN, cg.RMAX, 1000), (A, B): morse(0.0, c["rcut"], 1000),
              (B, B): (harmonic_table(K, cg.SIGMA, 1024), 0.0, cg.SIGMA)}
    for seed in range(100):
        types = types_of(c["n"], 2, seed)
        have = {(cname, inside) for i, j, cname, inside, _ in c["planted"]
                if cname in CUTOFF_TYPE and tuple(sorted((types[i], types[j]))) == CUTOFF_TYPE[cname]}
        if have == {(cname, inside) for _, _, cname, inside, _ in c["planted"] if cname in CUTOFF_TYPE}:
            break
    obs, F = tr.typed_observables(c["pos"], c["box"], types, 2, tables, port())
    for a in (types, obs, F):
        a.setflags(write=False)
    return c, types, tables, obs, F


@pytest.mark.parametrize("name", GRID_NAMES)
def test_many_cell_grids(name):
    import pse_amd
    c, types, tables, ref, F = grid_case(name)
    # on the host, before the device is asked: the planted pairs that test each range are there, on the side they were planted on
    pos, box = c["pos"], c["box"]
    i, j, _, _, _, _, _ = tr.typed_terms(pos, box, types, 2, tables, port())
    acting = set(zip(i.tolist(), j.tolist()))
    seen = set()
    for a, b, cname, inside, _ in c["planted"]:
        if cname in CUTOFF_TYPE and tuple(sorted((types[a], types[b]))) == CUTOFF_TYPE[cname]:
            key = (min(a, b), max(a, b))
            assert (key in acting) == (inside if cname != "rmin" else not inside), (cname, inside, key)
            seen.add((cname, inside))
    # (one_cell_x has one cell along x: cell_grid_cases plants its cutoff pairs only where every axis has several cells)
    assert len(seen) == (0 if name == "one_cell_x" else 8), seen
    assert seen == {(cname, inside) for _, _, cname, inside, _ in c["planted"] if cname in CUTOFF_TYPE}
    counts = tr.pairs_in_range(pos, box, types, 2, tables, port())
    assert min(counts.values()) > 20, counts
    eng = pse_amd.Engine(c["n"], box, xi=c["xi"], error=c["error"], max_strain=c["max_strain"], seed=77)
    assert abs(eng.info()["rcut"] - c["rcut"]) <= 1e-15 * c["rcut"]
    tt = typed(eng, types, tables)
    dpos = to4(pos)
    for which in ("wide", "narrow"):
        eng.set_neighbor_skin(c["skin"] if which == "wide" else 0.0)
        f = to4(np.zeros((c["n"], 3)), 7.0)
        out = eng.pair_table_typed(dpos, f, tt, accumulate=False).cpu().numpy()
        info = eng.info()
        assert (info["ncell_x"], info["ncell_y"], info["ncell_z"]) == c["cells_" + which][:3]
        check_obs(out, ref, f"{name} {which}")
        g = f.cpu().numpy()
        check_forces(g[:, :3], F, f"{name} {which}")
        assert np.all(g[:, 3] == 7.0)
    tt.close()
    eng.close()


# -- the raw C-ABI ---------------------------------------------------------------------------------------------------------------------

def test_misuse_is_reported_before_any_launch():
    """Raw C-ABI, as a C host would call it (the style of tests/test_gpu_pair_table.py)."""
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

    n = 64
    box = (20.0, 20.0, 20.0, 0.0)
    pos = random_points(n, box, seed=1)
    pos[1] = pos[0] + np.array([0.6, 0.5, -0.4])
    types = (np.arange(n) % 2).astype(np.uint32)
    tables = {(A, A): morse(0.7, 3.0, 100), (A, B): morse(0.0, 2.0, 16, r0=1.0)}
    width, rmin, rmax, entries = tr.arrays(tables, 2)
    dpos, dF = to4(pos), to4(np.zeros((n, 3)), 5.0)
    out8 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")

    def table_on(h, expect=0):
        t = ctypes.c_void_p(777)
        rc = lib.pse_typed_table_create(h, n, vp(types), 2, vp(width), vp(rmin), vp(rmax), vp(entries), ctypes.byref(t))
        assert rc == expect, msg()
        return t

    rc, h = create(20.0, n)
    assert rc == 0, msg()
    rc, h2 = create(20.0, n)
    assert rc == 0, msg()
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    t, ts = table_on(h), table_on(hs)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    ex2 = ctypes.c_void_p()
    assert lib.pse_exclusions_create(h2, n, 1, vp(pairs), ctypes.byref(ex2)) == 0, msg()
    # a refusal at creation leaves *out null
    bad = ctypes.c_void_p(777)
    big = types.copy()
    big[5] = 2
    assert lib.pse_typed_table_create(h, n, vp(big), 2, vp(width), vp(rmin), vp(rmax), vp(entries), ctypes.byref(bad)) == INVALID
    assert "type 2" in msg() and not bad.value
    call = lib.pse_pair_table_typed

    def refused(word, tt=t, p=P(dpos), f=P(dF), nn=n, o=P(out8), e=None):
        assert call(tt, p, f, None, nn, 0, o, e) == INVALID, word
        assert word in msg(), (word, msg())

    refused("null typed table", tt=None)
    refused("null pos", p=None)
    refused("both null", f=None, o=None)
    refused("n_max", nn=0)
    refused("n_max", nn=n + 1)
    refused("slab rank", tt=ts)
    refused("another handle", e=ex2)
    # nothing was launched, nothing was written; and the handle works afterwards
    torch.cuda.synchronize()
    assert np.all(out8.cpu().numpy() == -1.0) and np.array_equal(dF.cpu().numpy(), to4(np.zeros((n, 3)), 5.0).cpu().numpy())
    assert call(t, P(dpos), P(dF), None, n, 0, P(out8), None) == 0, msg()
    ref, F = tr.typed_observables(pos, box, types, 2, tables, port())
    assert ref[7] >= 1
    check_obs(out8.cpu().numpy(), ref, "after the refused calls")
    check_forces(dF.cpu().numpy()[:, :3], F, "after the refused calls")
    assert lib.pse_typed_table_destroy(t) == 0
    assert lib.pse_typed_table_destroy(None) == 0
    for hh in (h, h2, hs):                                                     # ts and ex2 are still alive: they go with their handles
        assert lib.pse_destroy(hh) == 0


# -- the provider ------------------------------------------------------------------------------------------------------------------------

def test_typed_provider_with_a_stress_log():
    """forces.TypedTablePair(virial=True) through two integrator steps with a StressLog at period 1: every row of the log is what a
    direct Engine.pair_table_typed call gives on the positions of that step; from_functions samples what morse_table samples."""
    import torch
    from pse_amd import forces, integrate
    from pse_amd.system import System
    box = TILTED[:3] + (0.0,)
    pos = random_points(N, box, seed=11)
    vol = box[0] * box[1] * box[2]
    s = System(pos, box, dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3)      # no shear, no noise: the forces alone move the particles
    D, al = MORSE["D"], MORSE["alpha"]

    def V(re):
        return lambda r: D * ((1.0 - np.exp(-al * (r - re))) ** 2 - 1.0)

    def Fr(re):
        return lambda r: -2.0 * D * al * (1.0 - np.exp(-al * (r - re))) * np.exp(-al * (r - re))

    names = ["A", "B"]
    types = types_of(N, 2)
    named = [names[t] for t in types]
    functions = {("A", "A"): (V(1.5), Fr(1.5), 0.7, 3.0, 500), ("B", "A"): (V(1.2), Fr(1.2), 0.0, 2.0, 300)}       # B-B is off
    tables = {(A, A): morse(0.7, 3.0, 500), (A, B): morse(0.0, 2.0, 300, r0=1.2)}
    plain = forces.TypedTablePair.from_functions(pse, named, functions, type_names=names)
    assert plain.ntypes == 2 and plain.table(1, 1) is None
    for key, (t, _, _) in tables.items():
        got = plain.table(*key)
        assert got.shape == t.shape and np.abs(got - t).max() <= 1e-12
    ref, F = tr.typed_observables(pos, box, types, 2, tables, port())
    assert ref[7] > 20
    plain.compute(0)                                                      # virial=False: forces only
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "TypedTablePair, virial=False")
    with pytest.raises(RuntimeError, match="TypedTablePair"):
        plain.energy
    with pytest.raises(ValueError, match="TypedTablePair"):
        forces.StressLog(plain, 1, 4)
    s.forces.remove(plain)
    with pytest.raises(ValueError, match="entries"):
        forces.TypedTablePair(pse, types[:-1], tables)
    assert s.forces == []
    tp = forces.TypedTablePair(pse, types, {k: (torch.tensor(t), lo, hi) for k, (t, lo, hi) in tables.items()}, virial=True)
    s.net_force.zero_()
    tp.compute(0)
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "TypedTablePair, virial=True")
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    W = np.array([[ref[1], ref[2], ref[3]], [ref[2], ref[4], ref[5]], [ref[3], ref[5], ref[6]]])
    assert abs(tp.energy - ref[0]) <= tol and tp.npairs == ref[7]
    assert np.abs(tp.virial - W).max() <= tol and np.abs(tp.stress() + W / vol).max() <= tol / vol
    log = forces.StressLog(tp, period=1, capacity=4)
    direct = []
    eng = engine(box)
    tt = typed(eng, types, tables)
    for t in range(2):
        snap = s.pos.clone()
        direct.append(eng.pair_table_typed(snap, None, tt).cpu().numpy())
        check_obs(direct[-1], tr.typed_observables(snap.cpu().numpy()[:, :3], box, types, 2, tables, port())[0], f"step {t}")
        s.run(1)
    tab = log.table()
    assert tab.shape == (2, 10) and list(tab[:, 0]) == [0.0, 1.0]
    assert not np.array_equal(direct[0], direct[1])                       # the particles did move
    for row, d8 in zip(tab, direct):
        t8 = 1e-11 * max(1.0, np.abs(d8).max())
        assert abs(row[2] - d8[0]) <= t8 and row[9] == d8[7] > 0
        assert np.abs(row[3:9] + d8[1:7] / vol).max() <= t8 / vol
    assert torch.isfinite(s.pos).all()
    tt.close()
