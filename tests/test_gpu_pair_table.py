"""GPU tests of the tabulated pair potential (pse_pair_table): forces, energy, virial and pair count against the O(N^2) reference of
tests/pair_table_ref.py (validated on the CPU by tests/test_pair_table_reference.py) over the wave / workgroup edges, the table
widths and ranges, every call form, the harmonic table against pse_pair_repulsion_virial, reproducibility, asynchronous submission,
the error returns, and the providers on top (forces.TablePair, forces.HarmonicRepulsion, forces.StressLog).

Bound: the repulsion's own (tests/test_gpu_pair_virial.py), 1e-11 max(1, max |ref|) per quantity -- the eight observables together,
the forces together; npairs must match exactly.  The device forms t as (r - rmin) * [(width - 1)/(rmax - rmin)], the reference as
(r - rmin)(width - 1)/(rmax - rmin): two ulps of t <= 2047, i.e. 5e-13 of a node spacing in V and F, far inside the bound."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
from pair_table_ref import harmonic_table, morse_table, pair_observables, random_points
import pair_virial_ref

pytestmark = pytest.mark.gpu

NMAX = 513
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
N = 300
K = 40.0
INVALID = -1
MORSE = dict(D=5.0, alpha=2.0, r0=1.5)          # F > 0 inside r0 = 1.5, F < 0 outside


def port():
    from oracle import pse_port
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(box):
    import pse_amd
    return pse_amd.Engine(NMAX, box, xi=0.5, error=1e-3)


def rcut(box):
    return engine(box).info()["rcut"]


@functools.lru_cache(maxsize=None)
def table_case(name, box):
    """(table, rmin, rmax) by name; rmax 'rcut' is the engine's own cutoff."""
    if name == "w2":            # the index clamp is the only path; V and F change sign along the one interval
        return np.array([[3.0, 5.0], [-1.0, -2.0]]), 0.0, 2.0
    if name == "w3":
        return np.array([[3.0, 5.0], [-2.0, 1.0], [0.5, -2.0]]), 0.0, 2.0
    if name == "w1000":
        return morse_table(rmin=0.7, rmax=3.0, width=1000, **MORSE), 0.7, 3.0
    if name == "w2048":         # fills the 32 KB LDS stage
        return morse_table(rmin=0.7, rmax=3.0, width=2048, **MORSE), 0.7, 3.0
    if name == "w2048_rmin0":
        return morse_table(rmin=0.0, rmax=2.5, width=2048, **MORSE), 0.0, 2.5
    if name == "rcut":          # the whole range the cell list serves
        rc = rcut(box)
        return morse_table(rmin=0.0, rmax=rc, width=1000, **MORSE), 0.0, rc
    if name == "rcut_rmin":
        rc = rcut(box)
        return morse_table(rmin=0.7, rmax=rc, width=257, **MORSE), 0.7, rc
    if name == "harmonic":
        return harmonic_table(K, 2.0, 1024), 0.0, 2.0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, box, n=N, seed=11):
    """(pos, table, rmin, rmax, obs, F): computed once, shared, never written to."""
    table, rmin, rmax = table_case(name, box)
    pos = random_points(n, box, seed)
    obs, F = pair_observables(pos, box, table, rmin, rmax, port())
    for a in (pos, table, obs, F):
        a.setflags(write=False)
    return pos, table, rmin, rmax, obs, F


def dev(table):
    import torch
    return torch.tensor(np.asarray(table), dtype=torch.float64, device="cuda")


def pairs_below(pos, box, rmin):
    i, j = np.triu_indices(len(pos), 1)
    d = port().min_image(pos[i] - pos[j], box)
    r = np.sqrt((d * d).sum(axis=1))
    return int(((r < rmin) & (r > 0)).sum())


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
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_row_counts(n, box):
    """A partial last wave, a full one, one lane of the next; the same for the 256-thread workgroup; 513: three workgroup rows for
    the finishing kernel instead of two; 1: no pair at all, the eight numbers are zeros."""
    table, rmin, rmax = table_case("w1000", box)
    pos = random_points(n, box, seed=100 + n)
    if n == 2:
        pos[1] = pos[0] + np.array([0.9, -0.7, 0.4])       # two random points would not meet
    ref, F = pair_observables(pos, box, table, rmin, rmax, port())
    if n == 1:
        assert not ref.any()
    else:
        assert ref[7] >= 1 and (n < 63 or ref[7] >= 10)
    f = to4(np.zeros((n, 3)), 3.0)
    out = engine(box).pair_table(to4(pos), f, dev(table), rmin, rmax, accumulate=False).cpu().numpy()
    check_obs(out, ref, f"n={n}")
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, f"n={n}")
    assert np.all(g[:, 3] == 3.0)


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
@pytest.mark.parametrize("name", ["w2", "w3", "w1000", "w2048", "w2048_rmin0", "rcut", "rcut_rmin"])
def test_tables(name, box):
    import torch
    pos, table, rmin, rmax, ref, F = case(name, box)
    assert ref[7] > 20
    if rmin > 0:
        assert pairs_below(pos, box, rmin) >= 1
    assert (table[:, 1] > 0).any() and (table[:, 1] < 0).any()            # a sign error in F or W cannot cancel
    f = to4(np.zeros((N, 3)), 7.0)
    out = engine(box).pair_table(to4(pos), f, dev(table), rmin, rmax, accumulate=False)
    assert out.shape == (8,) and out.is_cuda and out.dtype == torch.float64
    check_obs(out.cpu().numpy(), ref, f"{name} width={len(table)} [{rmin}, {rmax:.4f})")
    g = f.cpu().numpy()
    check_forces(g[:, :3], F, name)
    assert np.all(g[:, 3] == 7.0)


def test_call_forms():
    import torch
    box = TILTED
    eng = engine(box)
    pos, table, rmin, rmax, ref, F = case("w1000", box)
    dpos, dtab = to4(pos), dev(table)
    base = np.random.default_rng(5).normal(size=(N, 3))
    # accumulate = 0: overwritten, w kept; accumulate = 1: added
    f0 = to4(base, 7.0)
    check_obs(eng.pair_table(dpos, f0, dtab, rmin, rmax, accumulate=False).cpu().numpy(), ref, "accumulate=0")
    g0 = f0.cpu().numpy()
    check_forces(g0[:, :3], F, "accumulate=0")
    f1 = to4(base, 7.0)
    check_obs(eng.pair_table(dpos, f1, dtab, rmin, rmax, accumulate=True).cpu().numpy(), ref, "accumulate=1")
    g1 = f1.cpu().numpy()
    check_forces(g1[:, :3] - base, F, "accumulate=1")
    assert np.all(g0[:, 3] == 7.0) and np.all(g1[:, 3] == 7.0)
    # force = None: the same eight numbers
    c = eng.pair_table(dpos, None, dtab, rmin, rmax).cpu().numpy()
    check_obs(c, ref, "force=None")
    # observables = False: the same forces, `out` is not touched, nothing is returned
    out = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    for acc, want in ((False, F), (True, F + base)):
        f2 = to4(base, 7.0)
        assert eng.pair_table(dpos, f2, dtab, rmin, rmax, accumulate=acc, out=out, observables=False) is None
        g2 = f2.cpu().numpy()
        check_forces(g2[:, :3], want, f"observables=False accumulate={acc}")
        assert np.all(g2[:, 3] == 7.0)
    assert np.isnan(out.cpu().numpy()).all()
    # a row of a log: only that row is written
    log = torch.full((6, 8), float("nan"), dtype=torch.float64, device="cuda")
    ret = eng.pair_table(dpos, None, dtab, rmin, rmax, out=log[3])
    assert ret.data_ptr() == log[3].data_ptr()
    host = log.cpu().numpy()
    assert np.array_equal(host[3], c) and np.isnan(np.delete(host, 3, axis=0)).all()
    # neither forces nor observables: refused by the C-ABI
    with pytest.raises(Exception, match="both null"):
        eng.pair_table(dpos, None, dtab, rmin, rmax, observables=False)
    # the table must be what the header says
    for bad in (dtab[:, :1], dtab.to(torch.float32), dtab.cpu(), dtab.t()):
        with pytest.raises(ValueError):
            eng.pair_table(dpos, None, bad, rmin, rmax)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], pos) and np.array_equal(dtab.cpu().numpy(), table)


def test_group_counts_only_its_members():
    import torch
    box = TILTED
    pos, table, rmin, rmax, _, _ = case("w1000", box)
    members = np.arange(0, N, 2)
    ref, F = pair_observables(pos[members], box, table, rmin, rmax, port())
    assert ref[7] > 5
    sentinel = np.random.default_rng(9).normal(size=(N, 3))
    f = to4(sentinel, 7.0)
    group = torch.tensor(members, dtype=torch.int32, device="cuda")
    out = engine(box).pair_table(to4(pos), f, dev(table), rmin, rmax, group=group, accumulate=False).cpu().numpy()
    check_obs(out, ref, "group of every other particle")
    g = f.cpu().numpy()
    check_forces(g[members, :3], F, "group")
    assert np.array_equal(g[1::2, :3], sentinel[1::2]) and np.all(g[:, 3] == 7.0)       # non-members untouched


@pytest.mark.parametrize("box", [CUBIC, TILTED], ids=["cubic", "tilted"])
def test_harmonic_table_agrees_with_the_repulsion(box):
    eng = engine(box)
    pos, table, rmin, rmax, ref, F = case("harmonic", box)
    dpos = to4(pos)
    ft, fr = to4(np.zeros((N, 3))), to4(np.zeros((N, 3)))
    tab = eng.pair_table(dpos, ft, dev(table), rmin, rmax, accumulate=False).cpu().numpy()
    rep = eng.pair_repulsion_virial(dpos, fr, K, 2.0, accumulate=False).cpu().numpy()
    check_obs(tab, ref, "harmonic table")
    assert tab[7] == rep[7] > 20
    tol = 1e-11 * max(1.0, np.abs(rep).max())
    assert np.abs(tab[1:7] - rep[1:7]).max() <= tol                       # F is linear in r: the table is exact for W ...
    check_forces(ft.cpu().numpy()[:, :3], fr.cpu().numpy()[:, :3], "table against repulsion")      # ... and for the forces
    dr = 2.0 / (len(table) - 1)
    print(f"U_table - U = {tab[0] - rep[0]:.3e}, bound {rep[7] * K * dr * dr / 8.0:.3e}")
    assert abs(tab[0] - rep[0]) <= rep[7] * K * dr * dr / 8.0             # the chord of the parabola, per pair


def test_repeatable_and_independent_of_other_calls():
    box = TILTED
    eng = engine(box)
    pos, table, rmin, rmax, ref, F = case("w2048", box)
    dpos, dtab = to4(pos), dev(table)
    fa, fb, fc = (to4(np.zeros((N, 3))) for _ in range(3))
    a = eng.pair_table(dpos, fa, dtab, rmin, rmax, accumulate=False).cpu().numpy()
    b = eng.pair_table(dpos, fb, dtab, rmin, rmax, accumulate=False).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(fa.cpu().numpy(), fb.cpu().numpy())       # bit for bit: no atomics, stable sort
    # another entry point in between: `prepare` state is shared, the next call sorts again
    other = random_points(N, box, seed=77)
    eng.mobility(to4(other), to4(np.random.default_rng(1).normal(size=(N, 3))))
    c = eng.pair_table(dpos, fc, dtab, rmin, rmax, accumulate=False).cpu().numpy()
    check_obs(c, ref, "after pse_mobility")
    check_forces(fc.cpu().numpy()[:, :3], F, "after pse_mobility")
    assert np.array_equal(a, c) and np.array_equal(fa.cpu().numpy(), fc.cpu().numpy())


def test_async_submission_gives_the_same_numbers():
    import torch
    import pse_amd
    box = TILTED
    pos, table, rmin, rmax, ref, F = case("w1000", box)
    eng = pse_amd.Engine(N, box, xi=0.5, error=1e-3)
    dpos, dtab = to4(pos), dev(table)
    fs = to4(np.zeros((N, 3)))
    sync = eng.pair_table(dpos, fs, dtab, rmin, rmax, accumulate=False).cpu().numpy()
    eng.set_async(True)
    for _ in range(2):                                                # twice: the second call finds the first one's state in place
        fa = to4(np.zeros((N, 3)))
        out = eng.pair_table(dpos, fa, dtab, rmin, rmax, accumulate=False)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        check_obs(out, ref, "async")
        assert np.abs(out - sync).max() <= 1e-11 * max(1.0, np.abs(ref).max())
        check_forces(fa.cpu().numpy()[:, :3], F, "async")
    eng.set_async(False)
    eng.close()


def test_misuse_is_reported_before_any_launch():
    """Raw C-ABI, as a C host would call it (the style of tests/test_gpu_errors.py)."""
    import torch
    from pse_amd import _lib
    from pse_amd._lib import pse_params
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731

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
    table = harmonic_table(1.0, 2.0, 16)
    dpos, dF, dtab = to4(pos), to4(np.zeros((n, 3)), 5.0), dev(np.concatenate([table, table]))     # (room to step 8 bytes into it)
    out8 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    rc, h = create(20.0, n)
    assert rc == 0, msg()
    info = _lib.pse_info()
    assert lib.pse_get_info(h, ctypes.byref(info)) == 0
    rc_h = info.as_dict()["rcut"]
    call = lib.pse_pair_table
    nan, inf = float("nan"), float("inf")

    def refused(word, hh=h, p=P(dpos), f=P(dF), nn=n, t=P(dtab), w=16, rmin=0.0, rmax=2.0, o=P(out8)):
        assert call(hh, p, f, None, nn, t, w, rmin, rmax, 0, o) == INVALID, word
        assert word in msg(), (word, msg())

    refused("null handle", hh=None)
    refused("null pos", p=None)
    refused("null table", t=None)
    refused("both null", f=None, o=None)
    refused("n_max", nn=0)
    refused("n_max", nn=n + 1)
    refused("width", w=1)
    refused("width", w=0)
    refused("width", w=2049)
    refused("negative", rmin=-0.1)
    refused("must exceed", rmin=2.0, rmax=2.0)
    refused("must exceed", rmin=1.5, rmax=1.0)
    refused("rcut", rmax=rc_h * (1.0 + 1e-12))
    refused("finite", rmin=nan)
    refused("finite", rmax=nan)
    refused("finite", rmax=inf)
    refused("16-byte", t=ctypes.c_void_p(dtab.data_ptr() + 8))
    # a slab rank orders only its own cells: observables are refused there
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    refused("slab rank", hh=hs)
    assert lib.pse_destroy(hs) == 0
    # nothing was launched, nothing was written; and the handle works afterwards
    torch.cuda.synchronize()
    assert np.all(out8.cpu().numpy() == -1.0) and np.array_equal(dF.cpu().numpy(), to4(np.zeros((n, 3)), 5.0).cpu().numpy())
    assert call(h, P(dpos), P(dF), None, n, P(dtab), 16, 0.0, 2.0, 0, P(out8)) == 0, msg()
    ref, F = pair_observables(pos, box, table, 0.0, 2.0, port())
    assert ref[7] >= 1
    check_obs(out8.cpu().numpy(), ref, "after the refused calls")
    check_forces(dF.cpu().numpy()[:, :3], F, "after the refused calls")
    # rmax = rcut itself is accepted
    assert call(h, P(dpos), P(dF), None, n, P(dtab), 16, 0.0, rc_h, 0, P(out8)) == 0, msg()
    assert lib.pse_destroy(h) == 0


def _system(pos, box, dt=1e-3):
    from pse_amd import integrate
    from pse_amd.system import System
    s = System(pos, box, dt=dt)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3)      # no shear, no noise: the forces alone move the particles
    return s, pse


def test_table_provider_with_a_stress_log():
    """forces.TablePair(virial=True) through two integrator steps with a StressLog at period 1: every row of the log is what a direct
    Engine.pair_table call gives on the positions of that step."""
    import torch
    from pse_amd import forces
    box = TILTED[:3] + (0.0,)
    pos = random_points(N, box, seed=11)
    vol = box[0] * box[1] * box[2]
    s, pse = _system(pos, box)
    r0, r1 = 0.7, 3.0
    D, al, re = MORSE["D"], MORSE["alpha"], MORSE["r0"]
    V = lambda r: D * ((1.0 - np.exp(-al * (r - re))) ** 2 - 1.0)                             # noqa: E731
    Fr = lambda r: -2.0 * D * al * (1.0 - np.exp(-al * (r - re))) * np.exp(-al * (r - re))    # noqa: E731
    plain = forces.TablePair.from_functions(pse, V, Fr, r0, r1, 500)
    table = plain.table.cpu().numpy()
    assert table.shape == (500, 2) and np.abs(table - morse_table(rmin=r0, rmax=r1, width=500, **MORSE)).max() <= 1e-12
    ref, F = pair_observables(pos, box, table, r0, r1, port())
    plain.compute(0)                                                      # virial=False: forces only
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "TablePair, virial=False")
    with pytest.raises(RuntimeError, match="TablePair"):
        plain.energy
    with pytest.raises(ValueError, match="TablePair"):
        forces.StressLog(plain, 1, 4)
    s.forces.remove(plain)
    for bad in (np.zeros((1, 2)), np.zeros((2049, 2)), np.zeros((5, 3)), np.full((4, 2), np.nan)):
        with pytest.raises(ValueError):
            forces.TablePair(pse, bad, r0, r1)
    with pytest.raises(ValueError):
        forces.TablePair(pse, table, 2.0, 1.0)
    assert s.forces == []
    tp = forces.TablePair(pse, torch.tensor(table), r0, r1, virial=True)          # a torch array will do as well
    s.net_force.zero_()
    tp.compute(0)
    check_forces(s.net_force.cpu().numpy()[:, :3], F, "TablePair, virial=True")
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    W = np.array([[ref[1], ref[2], ref[3]], [ref[2], ref[4], ref[5]], [ref[3], ref[5], ref[6]]])
    assert abs(tp.energy - ref[0]) <= tol and tp.npairs == ref[7]
    assert np.abs(tp.virial - W).max() <= tol and np.abs(tp.stress() + W / vol).max() <= tol / vol
    log = forces.StressLog(tp, period=1, capacity=4)
    direct = []
    eng = engine(box)
    for t in range(2):
        snap = s.pos.clone()
        direct.append(eng.pair_table(snap, None, tp.table, r0, r1).cpu().numpy())
        check_obs(direct[-1], pair_observables(snap.cpu().numpy()[:, :3], box, table, r0, r1, port())[0], f"step {t}")
        s.run(1)
    tab = log.table()
    assert tab.shape == (2, 10) and list(tab[:, 0]) == [0.0, 1.0]
    assert not np.array_equal(direct[0], direct[1])                       # the particles did move
    for row, d8 in zip(tab, direct):
        t8 = 1e-11 * max(1.0, np.abs(d8).max())
        assert abs(row[2] - d8[0]) <= t8 and row[9] == d8[7] > 0
        assert np.abs(row[3:9] + d8[1:7] / vol).max() <= t8 / vol
    assert torch.isfinite(s.pos).all()


def test_harmonic_provider_still_logs():
    """The providers now share a base class: HarmonicRepulsion with a StressLog as before, and next to a TablePair."""
    from pse_amd import forces
    box = TILTED[:3] + (0.0,)
    pos = random_points(N, box, seed=11)
    vol = box[0] * box[1] * box[2]
    s, pse = _system(pos, box)
    plain = forces.HarmonicRepulsion(pse, k=K, sigma=2.0)
    with pytest.raises(RuntimeError, match="HarmonicRepulsion"):
        plain.energy
    with pytest.raises(ValueError, match="StressLog needs a HarmonicRepulsion"):
        forces.StressLog(plain, 1, 4)
    s.forces.remove(plain)
    rep = forces.HarmonicRepulsion(pse, k=K, sigma=2.0, virial=True)
    tp = forces.TablePair(pse, harmonic_table(K, 2.0, 1024), 0.0, 2.0, virial=True)
    rlog, tlog = forces.StressLog(rep, 1, 4), forces.StressLog(tp, 1, 4)
    ref, F = pair_virial_ref.pair_observables(pos, box, K, 2.0, port())
    s.run(1)
    check_forces(s.net_force.cpu().numpy()[:, :3], 2.0 * F, "both providers add their forces")
    rt, tt = rlog.table(), tlog.table()
    assert rt.shape == tt.shape == (1, 10)
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    assert abs(rt[0, 2] - ref[0]) <= tol and rt[0, 9] == tt[0, 9] == ref[7]
    assert np.abs(rt[0, 3:9] + ref[1:7] / vol).max() <= tol / vol and np.abs(tt[0, 3:9] + ref[1:7] / vol).max() <= tol / vol
    assert abs(rep.energy - ref[0]) <= tol and isinstance(rep.energy, float)
    assert abs(tp.energy - ref[0]) <= ref[7] * K * (2.0 / 1023) ** 2 / 8.0
