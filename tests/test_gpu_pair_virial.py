"""GPU tests of the fused force + observables pass of the harmonic repulsion (pse_pair_repulsion_virial): energy, virial and pair
count against the O(N^2) reference of tests/pair_virial_ref.py (validated on the CPU by tests/test_pair_virial_reference.py), the
forces against pse_pair_repulsion, reproducibility, the error returns, and the host UI on top (HarmonicRepulsion(virial=True),
StressLog).

Bound: the project's own for this provider, 1e-11 max(1, max |ref|) over the eight numbers (a few hundred fp64 terms put the true
error near 1e-13); npairs must match exactly."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
from pair_virial_ref import pair_observables, random_points

pytestmark = pytest.mark.gpu

K, SIGMA = 40.0, 2.0
BOX = (14.0, 11.0, 17.0)
N = 300
INVALID = -1


def port():
    from oracle import pse_port
    return pse_port


@functools.lru_cache(maxsize=None)
def engine(xy):
    import pse_amd
    return pse_amd.Engine(N, BOX + (xy,), xi=0.5, error=1e-3)


@functools.lru_cache(maxsize=None)
def uniform_case(xy, sigma):
    """(pos, obs, F) of the N uniform random points in the cell of tilt xy: computed once, shared, never written to."""
    pos = random_points(N, BOX + (xy,), seed=11)
    obs, F = pair_observables(pos, BOX + (xy,), K, sigma, port())
    for a in (pos, obs, F):
        a.setflags(write=False)
    return pos, obs, F


def walk_points(n, box, seed=3):
    """n points of a random walk with steps of length 1.5 < sigma, wrapped into the cell: consecutive points always overlap, however
    few they are, and the walk crosses the periodic faces."""
    rng = np.random.default_rng(seed)
    step = rng.normal(size=(n, 3))
    step *= 1.5 / np.linalg.norm(step, axis=1)[:, None]
    pos = np.cumsum(step, axis=0)
    return port().wrap(pos, np.zeros((n, 3), dtype=np.int64), box)[0]


def check_obs(got, ref, what=""):
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"{what}: max |obs - ref| = {err:.3e} (bound {tol:.3e}), npairs {got[7]:.0f} / {ref[7]:.0f}, U {ref[0]:.6g}")
    assert got[7] == ref[7], (what, got[7], ref[7])
    assert err <= tol, (what, got, ref)


def force_tol(F):
    return 1e-11 * max(1.0, np.abs(F).max())


@pytest.mark.parametrize("xy", [0.0, 0.3, -0.5])
@pytest.mark.parametrize("sigma", [SIGMA, "rcut"])
def test_observables_and_forces_match_reference(xy, sigma):
    import torch
    eng = engine(xy)
    sig = eng.info()["rcut"] if sigma == "rcut" else sigma
    pos, ref, F = uniform_case(xy, sig)
    assert ref[7] > 20
    dpos = to4(pos)
    base = np.random.default_rng(5).normal(size=(N, 3))
    # accumulate = 0: overwritten, w kept
    f0 = to4(base, 7.0)
    out = eng.pair_repulsion_virial(dpos, f0, K, sig, accumulate=False)
    assert out.shape == (8,) and out.is_cuda and out.dtype == torch.float64
    check_obs(out.cpu().numpy(), ref, f"xy={xy} sigma={sig:.4f}")
    g0 = f0.cpu().numpy()
    assert np.abs(g0[:, :3] - F).max() <= force_tol(F) and np.all(g0[:, 3] == 7.0)
    # accumulate = 1: added
    f1 = to4(base, 7.0)
    out1 = eng.pair_repulsion_virial(dpos, f1, K, sig, accumulate=True)
    check_obs(out1.cpu().numpy(), ref, "accumulate")
    g1 = f1.cpu().numpy()
    assert np.abs(g1[:, :3] - (F + base)).max() <= force_tol(F) and np.all(g1[:, 3] == 7.0)
    # ... and both agree with the plain call on the same engine
    for acc, fused in ((False, g0), (True, g1)):
        p = eng.pair_repulsion(dpos, to4(base, 7.0), K, sig, accumulate=acc).cpu().numpy()
        assert np.abs(p[:, :3] - fused[:, :3]).max() <= force_tol(F) and np.all(p[:, 3] == 7.0)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], pos)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_wave_and_workgroup_edges(n):
    """A partial last wave, a full one, one lane of the next; the same for the 256-thread workgroup (257: a second workgroup of one
    thread)."""
    xy = 0.3
    box = BOX + (xy,)
    pos = walk_points(n, box)
    ref, F = pair_observables(pos, box, K, SIGMA, port())
    if n >= 2:
        assert ref[7] >= n - 1 > 0
    else:
        assert not ref.any()
    f = to4(np.zeros((n, 3)), 3.0)
    out = engine(xy).pair_repulsion_virial(to4(pos), f, K, SIGMA, accumulate=False).cpu().numpy()
    check_obs(out, ref, f"n={n}")
    g = f.cpu().numpy()
    assert np.abs(g[:, :3] - F).max() <= force_tol(F) and np.all(g[:, 3] == 3.0)


def test_pair_across_the_sheared_boundary():
    """Two particles whose minimum image goes through the y face of the tilted cell (a y image shifts x by xy Ly), against the pair
    worked out by hand."""
    xy = 0.3
    Lx, Ly, Lz = BOX
    d = np.array([-0.5, -0.9, -0.3])                     # r_1 - r_2 of the true neighbours
    p1 = np.array([3.0, 0.5 * Ly - 0.4, 0.2])
    p2 = p1 - d                                          # beyond the +y face ...
    p2 = p2 - np.array([xy * Ly, Ly, 0.0])               # ... so it is stored one y image down, x shifted by xy Ly
    assert abs(p2[1]) < 0.5 * Ly and abs(p2[0] - xy * p2[1]) < 0.5 * Lx
    r = np.sqrt((d * d).sum())
    c = K * (SIGMA - r) / r
    ref = np.array([0.5 * K * (SIGMA - r) ** 2, c * d[0] * d[0], c * d[0] * d[1], c * d[0] * d[2], c * d[1] * d[1], c * d[1] * d[2],
                    c * d[2] * d[2], 1.0])
    f = to4(np.zeros((2, 3)))
    out = engine(xy).pair_repulsion_virial(to4(np.stack([p1, p2])), f, K, SIGMA, accumulate=False).cpu().numpy()
    check_obs(out, ref, "pair across the sheared face")
    g = f.cpu().numpy()[:, :3]
    assert np.abs(g[0] - c * d).max() <= force_tol(c * d) and np.abs(g[1] + c * d).max() <= force_tol(c * d)


def test_group_counts_only_its_members():
    import torch
    xy = 0.3
    pos, _, _ = uniform_case(xy, SIGMA)
    members = np.arange(0, N, 2)
    ref, F = pair_observables(pos[members], BOX + (xy,), K, SIGMA, port())
    assert ref[7] > 5
    sentinel = np.random.default_rng(9).normal(size=(N, 3))
    f = to4(sentinel, 7.0)
    group = torch.tensor(members, dtype=torch.int32, device="cuda")
    out = engine(xy).pair_repulsion_virial(to4(pos), f, K, SIGMA, group=group, accumulate=False).cpu().numpy()
    check_obs(out, ref, "group of every other particle")
    g = f.cpu().numpy()
    assert np.abs(g[members, :3] - F).max() <= force_tol(F)
    assert np.array_equal(g[1::2, :3], sentinel[1::2]) and np.all(g[:, 3] == 7.0)       # non-members untouched


def test_force_none_reproducibility_and_row_isolation():
    import torch
    xy = -0.5
    eng = engine(xy)
    pos, ref, _ = uniform_case(xy, SIGMA)
    dpos = to4(pos)
    a = eng.pair_repulsion_virial(dpos, to4(np.zeros((N, 3))), K, SIGMA).cpu().numpy()
    b = eng.pair_repulsion_virial(dpos, to4(np.zeros((N, 3))), K, SIGMA).cpu().numpy()
    assert np.array_equal(a, b)                                       # bit-reproducible: no atomics, stable sort
    # observables only: the same eight numbers, the positions as they were
    c = eng.pair_repulsion_virial(dpos, None, K, SIGMA).cpu().numpy()
    check_obs(c, ref, "force=None")
    assert np.array_equal(c, a)
    assert np.array_equal(dpos.cpu().numpy()[:, :3], pos)
    # a row of a log: only that row is written
    log = torch.full((6, 8), float("nan"), dtype=torch.float64, device="cuda")
    ret = eng.pair_repulsion_virial(dpos, None, K, SIGMA, out=log[3])
    assert ret.data_ptr() == log[3].data_ptr()
    host = log.cpu().numpy()
    assert np.array_equal(host[3], a) and np.isnan(np.delete(host, 3, axis=0)).all()


def test_async_submission_gives_the_same_numbers():
    import pse_amd
    xy = 0.3
    pos, ref, F = uniform_case(xy, SIGMA)
    eng = pse_amd.Engine(N, BOX + (xy,), xi=0.5, error=1e-3)
    dpos = to4(pos)
    fs = to4(np.zeros((N, 3)))
    sync = eng.pair_repulsion_virial(dpos, fs, K, SIGMA, accumulate=False).cpu().numpy()
    eng.set_async(True)
    for _ in range(2):                                                # twice: the second call finds the first one's state in place
        fa = to4(np.zeros((N, 3)))
        out = eng.pair_repulsion_virial(dpos, fa, K, SIGMA, accumulate=False).cpu().numpy()
        check_obs(out, ref, "async")
        assert np.abs(out - sync).max() <= 1e-11 * max(1.0, np.abs(ref).max())
        assert np.abs(fa.cpu().numpy()[:, :3] - F).max() <= force_tol(F)
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
    pos = random_points(n, (20.0, 20.0, 20.0, 0.0), seed=1)
    dpos, dF = to4(pos), to4(np.zeros((n, 3)), 5.0)
    out8 = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    rc, h = create(20.0, n)
    assert rc == 0, msg()
    call = lib.pse_pair_repulsion_virial
    assert call(None, P(dpos), P(dF), None, n, 1.0, 2.0, 0, P(out8)) == INVALID and "null handle" in msg()
    assert call(h, P(dpos), P(dF), None, n, 1.0, 2.0, 0, None) == INVALID and "out8" in msg()
    assert call(h, None, P(dF), None, n, 1.0, 2.0, 0, P(out8)) == INVALID and "null array" in msg()
    assert call(h, P(dpos), P(dF), None, 0, 1.0, 2.0, 0, P(out8)) == INVALID and "n_max" in msg()
    assert call(h, P(dpos), P(dF), None, n + 1, 1.0, 2.0, 0, P(out8)) == INVALID and "n_max" in msg()
    assert call(h, P(dpos), P(dF), None, n, 1.0, 50.0, 0, P(out8)) == INVALID and "repulsion range" in msg()
    assert call(h, P(dpos), P(dF), None, n, 1.0, 0.0, 0, P(out8)) == INVALID and "repulsion range" in msg()
    # a slab rank: its sort orders only its own cells
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    assert call(hs, P(dpos), P(dF), None, n, 1.0, 2.0, 0, P(out8)) == INVALID and "slab rank" in msg()
    assert lib.pse_destroy(hs) == 0
    # nothing was launched, nothing was written; and the handle works afterwards
    torch.cuda.synchronize()
    assert np.all(out8.cpu().numpy() == -1.0) and np.array_equal(dF.cpu().numpy()[:, :3], np.zeros((n, 3)))
    assert call(h, P(dpos), P(dF), None, n, 1.0, 2.0, 0, P(out8)) == 0, msg()
    ref, _ = pair_observables(pos, (20.0, 20.0, 20.0, 0.0), 1.0, 2.0, port())
    check_obs(out8.cpu().numpy(), ref, "after the refused calls")
    assert lib.pse_destroy(h) == 0


def test_host_ui_energy_stress_and_log():
    import torch
    from pse_amd import forces, integrate, shear_function, variant
    from pse_amd.system import System
    box = BOX + (0.0,)
    pos, ref, F = uniform_case(0.0, SIGMA)
    vol = BOX[0] * BOX[1] * BOX[2]
    dt = 1e-2
    s = System(pos, box, dt=dt)
    sf = shear_function.sine(dt=dt, shear_rate=2.0, shear_freq=5.0)
    s.box_tilt_variant = variant.shear_variant(sf, 100, max_strain=0.5)
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3, function_form=sf)
    plain = forces.HarmonicRepulsion(pse, k=K, sigma=SIGMA)
    plain.compute(0)
    f_plain = s.net_force.cpu().numpy().copy()
    assert np.abs(f_plain[:, :3] - F).max() <= force_tol(F)            # virial=False: today's path, today's forces
    with pytest.raises(RuntimeError):
        plain.energy
    with pytest.raises(ValueError):
        forces.StressLog(plain, 2, 8)
    s.forces.remove(plain)
    rep = forces.HarmonicRepulsion(pse, k=K, sigma=SIGMA, virial=True)
    s.net_force.zero_()
    rep.compute(0)
    assert np.abs(s.net_force.cpu().numpy() - f_plain).max() <= force_tol(F)
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    W = np.array([[ref[1], ref[2], ref[3]], [ref[2], ref[4], ref[5]], [ref[3], ref[5], ref[6]]])
    assert abs(rep.energy - ref[0]) <= tol and rep.npairs == ref[7]
    assert np.abs(rep.virial - W).max() <= tol and np.array_equal(rep.virial, rep.virial.T)
    assert np.abs(rep.stress() + W / vol).max() <= tol / vol
    # a log over 6 steps at period 2: rows at steps 0, 2, 4 with the tilt of those steps, each against the reference on the positions
    # and the box of its step (the run is stepped one by one here only to take those positions; the log itself never waits)
    log = forces.StressLog(rep, period=2, capacity=8)
    osf = port().SinShear(2.0, 5.0, 0, dt)
    refs, tilts = [], []
    for t in range(6):
        if t % 2 == 0:
            tilts.append(port().variant_value(osf, t, 100, -0.5, 0.5))
            refs.append(pair_observables(s.pos.cpu().numpy()[:, :3], BOX + (tilts[-1],), K, SIGMA, port())[0])
        s.run(1)
    tab = log.table()
    assert tab.shape == (3, 10) and list(tab[:, 0]) == [0.0, 2.0, 4.0]
    assert len(set(tilts)) == 3                                       # the tilt did change between the samples
    assert np.abs(refs[0] - ref).max() <= tol                         # the first sample is the state above
    for row, r8, xy in zip(tab, refs, tilts):
        assert abs(row[1] - xy) < 1e-15
        t8 = 1e-11 * max(1.0, np.abs(r8).max())
        assert abs(row[2] - r8[0]) <= t8 and row[9] == r8[7] > 0
        assert np.abs(row[3:9] + r8[1:7] / vol).max() <= t8 / vol
    # the ring keeps the newest rows
    ring = forces.StressLog(rep, period=2, capacity=2)
    s.run(6)
    assert list(ring.table()[:, 0]) == [8.0, 10.0]
    assert isinstance(rep.energy, float) and torch.isfinite(s.pos).all()
