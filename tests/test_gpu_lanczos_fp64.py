"""The fp64 Lanczos operator (pse_set_lanczos_operator(h, PSE_LANCZOS_FP64)): the near field inside the Lanczos iteration of
M_real^{1/2} psi applied exactly in double -- so the device meets the TRUE operator (the oracle's un-rounded sums, rounded=False /
pair_rounded=False) at the tightness the 16-byte records reach only against their own restatement, every driver applies it, and the
default mode is left as it was."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import make_suspension, to4
import record_bound as rb

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
M_MAX = 100   # the device's Lanczos basis cap (pse_capi.hip M_MAX)
GEOS = {g["name"]: g for g in rb.geometries()}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _child(code, env_extra):
    """Run `code` in a fresh Python process (environment switches are read once, in pse_create) -> its last output line."""
    env = dict(os.environ, **env_extra)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout.strip().splitlines()[-1]


# -- 1. the truth where the records fail ------------------------------------------------------------------------------------------
# Measured on an MI355X (relative error against M^{1/2} psi of the dense un-rounded operator; the records measured 2.7e-7 at c and 7.0e-7
# at f, tests/test_gpu_lanczos_truth.py): 4e-12 at a, m = 20, tol 1e-10; c (r = 1e-3 .. 2: condition 3.6e3, m = 95 without
# reorthogonalisation) 1.0e-8; f (xi = 10) 2.4e-9 at m = 13.  That last floor is the table's: at xi = 10 degree 9 on eighths follows f, g
# to 2.1e-10 only (format_eps, tests/realspace_ref.py; record_bound.table(10, rcut) = 6.2e-10), and the dense un-rounded M_real of that
# geometry with f, g read from the host's table instead of the closed forms moves M^{1/2} psi by 2.43e-9 relative
# (tests/test_realspace_table_cpu.py test_table_error_accounts_for_the_fp64_floor_at_xi_10) -- the operator's arithmetic adds nothing
# that can be seen.  FLOOR holds every geometry an order below what the records reach.
FLOOR = 2e-8


@pytest.mark.parametrize("name", list(GEOS))
def test_sqrt_mreal_meets_the_unrounded_operator(torch_cuda, oracle, name):
    import pse_amd
    g = GEOS[name]
    pos, box, xi = g["pos"], g["box"], g["xi"]
    n = len(pos)
    psi = np.random.default_rng(n).normal(size=(n, 3))
    eng = pse_amd.Engine(n, box, xi=xi, error=g["error"], lanczos_operator="fp64")
    assert eng.lanczos_operator == "fp64"
    ref, _ = rb.sqrt_apply(rb.dense_mreal(oracle, pos, box, xi, g["rcut"], rounded=False), psi)
    for tol in (1e-10, 1e-9, 1e-8):
        out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=tol)
        if m < M_MAX and eng.info()["lanczos_stepnorm"] <= tol:
            break
    else:
        pytest.fail(f"{name}: no convergence at tol = 1e-8 (m = {m})")
    err = rel(out.cpu().numpy()[:, :3], ref)
    print(f"fp64 {name}: m = {m}, tol = {tol:g}, |device - M^1/2 psi| / |M^1/2 psi| = {err:.3e}", flush=True)
    assert err <= tol + FLOOR, (name, m, tol, err)
    eng.close()


# -- 2. the oracle's un-rounded algorithm, m for m ----------------------------------------------------------------------------------
def test_dense_sqrt_mreal_matches_the_unrounded_oracle(torch_cuda, oracle):
    import pse_amd
    n = 60
    pos, _, box = make_suspension(n, L=16.0)
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3, lanczos_operator="fp64")
    rcut = eng.info()["rcut"]
    psi = np.random.default_rng(5).normal(size=(n, 3))
    mv = lambda v: oracle.mobility_real(pos, np.ascontiguousarray(v), box, 0.5, rcut, rounded=False)   # noqa: E731
    for tol in (1e-3, 1e-8):
        out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=tol)
        up, mp = oracle.lanczos_sqrt(mv, psi, 2, tol)
        print(f"fp64 dense n = 60, tol {tol:g}: m {m} / {mp}, rel {rel(out.cpu().numpy()[:, :3], up):.2e}", flush=True)
        assert m == mp, (tol, m, mp)
        assert rel(out.cpu().numpy()[:, :3], up) < 1e-9, tol


def _cluster(oracle, n_ball, radius, seed, n=400, L=30.0, centre=None):
    rng = np.random.default_rng(seed)
    box = (L, L, L, 0.0)
    ball = rng.normal(size=(n_ball, 3))
    ball *= (radius * rng.uniform(size=(n_ball, 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    c = np.array([L / 2 - 1.0, 0.0, -L / 2 + 0.5]) if centre is None else np.asarray(centre, float)
    pos = np.concatenate([ball + c, rng.uniform(-L / 2, L / 2, size=(n - n_ball, 3))])
    return oracle.wrap(pos, np.zeros((n, 3), dtype=np.int64), box)[0], box, rng


def test_overflow_rows_match_the_unrounded_oracle(torch_cuda, oracle):
    """Rows far beyond the list capacity: every mat-vec walks the cells for them, with the exact pair term."""
    import pse_amd
    pos, box, rng = _cluster(oracle, 300, 4.0, 17)
    n = len(pos)
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3, lanczos_operator="fp64")
    rcut = eng.info()["rcut"]
    assert ((np.linalg.norm(pos[:, None] - pos[None], axis=2) < rcut).sum(1) - 1).max() > 100
    psi = rng.normal(size=(n, 3))
    out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=1e-3)
    up, mp = oracle.lanczos_sqrt(lambda v: oracle.mobility_real(pos, np.ascontiguousarray(v), box, 0.5, rcut, rounded=False), psi, 2, 1e-3)
    print(f"fp64 overflow rows: m {m} / {mp}, rel {rel(out.cpu().numpy()[:, :3], up):.2e}", flush=True)
    assert m == mp and rel(out.cpu().numpy()[:, :3], up) < 1e-9, (m, mp, rel(out.cpu().numpy()[:, :3], up))


def test_overflow_rows_on_the_kept_neighbour_list(torch_cuda, oracle):
    """A cluster whose rows overflow the per-step pair list but fit the neighbour list kept across calls: after a move within the
    skin the call reuses the kept list, and the mat-vecs take those rows from it (the kept-list branch of k_mreal_list)."""
    import pse_amd
    pos, box, rng = _cluster(oracle, 36, 2.4, 29, centre=(0.0, 0.0, 0.0))
    n = len(pos)
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3, lanczos_operator="fp64")
    eng.set_neighbor_skin(0.4)
    rcut = eng.info()["rcut"]
    d = pos[:, None] - pos[None]
    d -= box[0] * np.rint(d / box[0])
    cnt = (np.linalg.norm(d, axis=2) < rcut).sum(1) - 1
    nbar = n / (box[0] ** 3) * 4.18879020478639 * rcut ** 3
    cap = (max(16, min(int(np.ceil(1.5 * nbar + 16.0)), 256)) + 3) & ~3      # the pair-list capacity (pse_create)
    assert cnt.max() > cap, (cnt.max(), cap)
    psi = rng.normal(size=(n, 3))
    eng.sqrt_mreal(to4(pos), to4(psi), tol=1e-3)                              # builds both lists
    moved = oracle.wrap(pos + rng.uniform(-0.05, 0.05, size=pos.shape), np.zeros((n, 3), dtype=np.int64), box)[0]
    _, b0, r0 = eng.neighbor_stats()
    out, m = eng.sqrt_mreal(to4(moved), to4(psi), tol=1e-3)
    _, b1, r1 = eng.neighbor_stats()
    assert r1 == r0 + 1 and b1 == b0, (b0, r0, b1, r1)                         # the kept list was used
    up, mp = oracle.lanczos_sqrt(lambda v: oracle.mobility_real(moved, np.ascontiguousarray(v), box, 0.5, rcut, rounded=False), psi, 2, 1e-3)
    print(f"fp64 kept list: m {m} / {mp}, rel {rel(out.cpu().numpy()[:, :3], up):.2e}", flush=True)
    assert m == mp and rel(out.cpu().numpy()[:, :3], up) < 1e-9, (m, mp, rel(out.cpu().numpy()[:, :3], up))


@pytest.mark.parametrize("xy", [0.0, 0.3])
def test_brownian_velocity_matches_the_unrounded_oracle(torch_cuda, oracle, xy):
    import pse_amd
    n = 1000
    pos, force, box = make_suspension(n, phi=0.1, xy=xy)
    seed, ts, kT, dt = 424242, 11, 1.0, 1e-3
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3, seed=seed, lanczos_operator="fp64")
    p = oracle.select_params(box, 0.5, 1e-3, 0.5)
    vel, m = eng.brownian_velocity(to4(pos), to4(force), kT, dt, ts)
    tru, mt = oracle.brownian_velocity(pos, force, box, p, kT, dt, seed, ts, pair_rounded=False)
    print(f"fp64 brownian_velocity xy = {xy}: m {m} / {mt}, rel {rel(vel.cpu().numpy()[:, :3], tru):.2e}", flush=True)
    assert m == mt and rel(vel.cpu().numpy()[:, :3], tru) < 1e-9, (m, mt, rel(vel.cpu().numpy()[:, :3], tru))


def test_step_matches_the_unrounded_oracle(torch_cuda, oracle):
    import pse_amd
    torch = torch_cuda
    n = 1000
    pos, force, box = make_suspension(n, phi=0.1, xy=0.25)
    seed, ts, kT, dt, rate = 99, 3, 1.0, 2e-2, 0.7
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3, seed=seed, lanczos_operator="fp64")
    p = oracle.select_params(box, 0.5, 1e-3, 0.5)
    dpos = to4(pos, w=1.0); dvel = to4(np.zeros((n, 3)), w=2.0); dF = to4(force, w=0.5)
    accel = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    image = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    ms = eng.step(dpos, dvel, accel, image, dF, kT, dt, ts, shear_rate=rate)
    ut, mt = oracle.brownian_velocity(pos, force, box, p, kT, dt, seed, ts, pair_rounded=False)
    assert ms == mt and rel(dvel.cpu().numpy()[:, :3], ut) < 1e-9, (ms, mt, rel(dvel.cpu().numpy()[:, :3], ut))
    newpos, newimg = oracle.integrate(pos, np.zeros((n, 3), dtype=np.int64), ut, box, dt, rate)
    assert np.abs(dpos.cpu().numpy()[:, :3] - newpos).max() < 1e-9
    assert np.array_equal(image.cpu().numpy(), newimg)


# -- 3. the mode in every driver ----------------------------------------------------------------------------------------------------
def test_queue_only_and_captured_calls_match_the_host_checked_call(torch_cuda):
    import pse_amd
    torch = torch_cuda
    n = 6000
    pos, force, box = make_suspension(n, phi=0.15, xy=0.1)
    kw = dict(xi=0.5, error=1e-6, seed=11, lanczos_operator="fp64")
    ref = pse_amd.Engine(n, box, **kw)
    eng = pse_amd.Engine(n, box, **kw)
    eng.set_async(True)
    dpos, dF = to4(pos), to4(force)
    u_ref, m = ref.brownian_velocity(dpos, dF, 1.0, 1e-3, 5, lanczos_m=2)
    u_ref = u_ref.cpu().numpy()[:, :3]
    vel, _ = eng.brownian_velocity(dpos, dF, 1.0, 1e-3, 5, lanczos_m=m)
    torch.cuda.synchronize()
    i = eng.info()
    assert i["lanczos_status"] == 0 and i["lanczos_m"] == m, (i["lanczos_m"], m)
    assert rel(vel.cpu().numpy()[:, :3], u_ref) < 1e-12
    # captured once, replayed once
    s = torch.cuda.Stream()
    eng.set_stream(s.cuda_stream)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.set_timestep_offset(word)
    out = to4(np.zeros((n, 3)))
    with torch.cuda.stream(s):
        eng.brownian_velocity(dpos, dF, 1.0, 1e-3, 5, vel=out, lanczos_m=m)   # warm-up outside the capture
    s.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        eng.brownian_velocity(dpos, dF, 1.0, 1e-3, 5, vel=out, lanczos_m=m)
    g.replay()
    torch.cuda.synchronize()
    i = eng.info()
    assert i["lanczos_status"] == 0 and i["lanczos_m"] == m
    assert rel(out.cpu().numpy()[:, :3], u_ref) < 1e-12


def test_replicated_team_matches_single_gpu(torch_cuda):
    """An in-process team of three (the two-step driver) against the single GPU, both in fp64 mode."""
    import pse_amd
    from pse_amd.sharded import LoopbackSimulation
    n = 3000
    pos, force, box = make_suspension(n, phi=0.1, xy=0.15)
    kw = dict(xi=0.5, error=1e-3, seed=3, grid=(48, 48, 48), lanczos_operator="fp64")
    ref = pse_amd.Engine(n, box, **kw)
    v_ref, m_ref = ref.brownian_velocity(to4(pos), to4(force), 1.0, 1e-3, 9)
    sim = LoopbackSimulation(n, box, 3, **kw)
    assert sim.team.lanczos_operator == "fp64"
    sim.load(pos, force)
    vels, m = sim.brownian_velocity(1.0, 1e-3, 9)
    assert m == m_ref
    for r in range(3):
        assert rel(vels[r].cpu().numpy()[:, :3], v_ref.cpu().numpy()[:, :3]) < 1e-12, r


_SSTEP_CHILD = """
import numpy as np
import pse_amd
from pse_amd.sharded import LoopbackSimulation
from conftest import make_suspension, to4
n = 3000
pos, force, box = make_suspension(n, phi=0.1, xy=0.15)
kw = dict(xi=0.5, error=1e-3, seed=3, grid=(48, 48, 48), lanczos_operator="fp64")
ref = pse_amd.Engine(n, box, **kw)
v_ref, m_ref = ref.brownian_velocity(to4(pos), to4(force), 1.0, 1e-3, 9)
sim = LoopbackSimulation(n, box, 2, **kw)
sim.load(pos, force)
vels, m = sim.brownian_velocity(1.0, 1e-3, 9)
i = sim.engines[0].info()
v = v_ref.cpu().numpy()[:, :3]
err = max(np.linalg.norm(x.cpu().numpy()[:, :3] - v) / np.linalg.norm(v) for x in vels)
print(m, m_ref, i["lanczos_exchanges"], i["lanczos_matvecs"], repr(float(err)))
"""


def test_one_step_team_driver_matches_single_gpu(torch_cuda):
    """PSE_TEAM_SSTEP=0 (read in pse_create): a team of two with one Lanczos iteration per exchange, in a child process."""
    m, m_ref, exch, matvecs, err = _child(_SSTEP_CHILD, {"PSE_TEAM_SSTEP": "0"}).split()
    assert m == m_ref and exch == matvecs, (m, m_ref, exch, matvecs)
    assert float(err) < 1e-12, err


def test_owned_particle_team_matches_single_gpu(torch_cuda):
    import math
    import pse_amd
    from pse_amd.sharded import LocalLoopbackSimulation
    n, grid = 24_000, 64
    pos, force, box = make_suspension(n, phi=0.1)
    xi = math.pi * grid / (2.0 * box[0] * math.sqrt(-math.log(1e-3)))
    kw = dict(xi=xi, error=1e-3, seed=5, grid=(grid,) * 3, lanczos_operator="fp64")
    sim = LocalLoopbackSimulation(n, box, 2, **kw)
    sim.load(pos, force)
    ref = pse_amd.Engine(n, box, **kw)
    vel = to4(np.zeros((n, 3)), 1.0)
    _, mr = ref.brownian_velocity(to4(pos), to4(force), 1.0, 1e-3, 7, vel=vel, lanczos_m=2)
    sim.step(1.0, 1e-3, 7, integrate=False, lanczos_m=mr)
    p, u, im, owner = sim.gather()
    assert all(e.info()["lanczos_status"] == 0 and e.info()["lanczos_m"] == mr for e in sim.engines)
    assert rel(u, vel.cpu().numpy()[:, :3]) < 1e-9, rel(u, vel.cpu().numpy()[:, :3])


# -- 4. the default untouched --------------------------------------------------------------------------------------------------------
def test_default_mode_is_bit_identical_after_a_round_trip(torch_cuda):
    import pse_amd
    n = 3000
    pos, force, box = make_suspension(n, phi=0.1, xy=0.2)
    eng = pse_amd.Engine(n, box, xi=0.5, error=1e-3, seed=8)
    v = ctypes.c_int(-1)
    assert eng._lib.pse_get_lanczos_operator(eng._h, ctypes.byref(v)) == 0 and v.value == 0
    assert eng.lanczos_operator == "records16"
    b0 = eng.info()["device_bytes"]
    dpos, dF = to4(pos), to4(force)
    psi = to4(np.random.default_rng(2).normal(size=(n, 3)))

    def calls():
        u, m = eng.brownian_velocity(dpos, dF, 1.0, 1e-3, 4)
        s, ms = eng.sqrt_mreal(dpos, psi, tol=1e-6)
        return u.clone(), m, s.clone(), ms
    calls()                                                                       # (the first call builds the kept list, the others reuse it)
    u0, m0, s0, ms0 = calls()
    eng.set_lanczos_operator("fp64")
    assert eng.lanczos_operator == "fp64" and eng.info()["device_bytes"] > b0      # the fp64 plane counts
    u1, _, s1, _ = calls()
    assert rel(u1.cpu().numpy(), u0.cpu().numpy()) < 1e-6                          # the same velocity, up to the records' rounding
    assert not torch_cuda.equal(s1, s0)                                           # ... and another operator
    eng.set_lanczos_operator("records16")
    u2, m2, s2, ms2 = calls()
    # the near-field half is bit for bit what it was; the whole velocity differs from one default call to the next by the far field's
    # order of summation alone (2.8e-14 of velocities of order 50 on an MI355X, with or without a round trip)
    assert ms2 == ms0 and torch_cuda.equal(s2, s0)
    assert m2 == m0 and (u2 - u0).abs().max().item() <= 1e-12 * u0.abs().max().item()
    # bad values on a live handle
    assert eng._lib.pse_set_lanczos_operator(eng._h, 2) == -1
    assert eng._lib.pse_set_lanczos_operator(eng._h, -1) == -1
    assert eng._lib.pse_get_lanczos_operator(eng._h, None) == -1
    assert eng.lanczos_operator == "records16"
    with pytest.raises(ValueError):
        eng.set_lanczos_operator("fp32")


def test_environment_default_selects_fp64():
    code = ("import pse_amd\n"
            "e = pse_amd.Engine(500, (20.0, 20.0, 20.0, 0.0), xi=0.5, error=1e-3)\n"
            "print(e.lanczos_operator)\n")
    assert _child(code, {"PSE_LANCZOS_OP": "fp64"}) == "fp64"


def test_team_refuses_members_with_different_operators(torch_cuda):
    import pse_amd
    from pse_amd import PSEError
    from pse_amd.sharded import LoopbackSimulation
    n = 2000
    pos, force, box = make_suspension(n, phi=0.1)
    sim = LoopbackSimulation(n, box, 2, xi=0.5, error=1e-3, seed=1, grid=(48, 48, 48))
    sim.load(pos, force)
    sim.engines[1].set_lanczos_operator("fp64")
    with pytest.raises(PSEError, match="error -1:.*different Lanczos operators"):
        sim.brownian_velocity(1.0, 1e-3, 1)
    with pytest.raises(PSEError, match="different Lanczos operators"):
        sim.team.lanczos_operator
    sim.team.set_lanczos_operator("fp64")
    vels, m = sim.brownian_velocity(1.0, 1e-3, 1)
    assert m >= 1
