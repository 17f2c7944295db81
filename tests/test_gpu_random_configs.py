"""Parity on configurations nobody picked by hand: seeded random boxes (three different edge lengths, any tilt the reference
allows), particle counts around the wave and block sizes (1, 2, 63, 64, 65, ...), grids from the reference's rule and explicit ones
with odd / non-2-3-5 sizes (which take the rocFFT x pass instead of the fused one), several accuracies.  Every case holds the
three parts of the path to the oracle: near field <= 1e-12 (C direct sum over minimum images), far field <= 1e-10 and the
Brownian velocity <= 1e-9 with the same Lanczos count (NumPy restatement of the reference algorithm)."""
import math

import numpy as np
import pytest

from conftest import to4

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def config(seed):
    rng = np.random.default_rng(1000 + seed)
    err = [1e-3, 1e-4, 1e-6][seed % 3]
    xi = rng.uniform(0.45, 0.7)
    rcut = math.sqrt(-math.log(err)) / xi
    lo = 2.3 * rcut                                                  # the minimum image needs rcut < half the narrowest width
    Lx, Ly, Lz = (float(rng.uniform(lo, lo + 14.0)) for _ in range(3))
    xy = float(rng.uniform(-0.5, 0.5)) if seed % 4 else 0.0
    n = [1, 2, 63, 64, 65, 127, 129, 300, 777, 1500, 2049, 2500][seed % 12]
    grid = None
    if seed % 3 == 1:                                                # explicit grid: odd and prime sizes included
        pick = rng.choice([22, 27, 31, 33, 36, 40, 45, 49, 50], 3)
        grid = tuple(int(g) for g in pick)
    box = (Lx, Ly, Lz, xy)
    f = rng.uniform(-0.5, 0.5, (n, 3))
    pos = np.empty((n, 3))
    pos[:, 1] = f[:, 1] * Ly
    pos[:, 2] = f[:, 2] * Lz
    pos[:, 0] = f[:, 0] * Lx + xy * pos[:, 1]
    if n > 2:                                                        # a particle on a face and two nearly touching across a face
        pos[0] = (-0.5 * Lx + xy * pos[0, 1], pos[0, 1], pos[0, 2])
        pos[1] = (pos[2, 0] + Lx - 2.05, pos[2, 1], pos[2, 2]) if pos[2, 0] < 0 else (pos[2, 0] - Lx + 2.05, pos[2, 1], pos[2, 2])
        fx = (pos[1, 0] - xy * pos[1, 1]) / Lx
        pos[1, 0] -= round(fx) * Lx                                  # back into the box
    force = rng.normal(size=(n, 3))
    return dict(box=box, xi=xi, err=err, grid=grid, pos=pos, force=force, n=n, seed=int(rng.integers(1, 2 ** 31)))


def config_fast(seed):
    """Grids wide enough for the binned spread / gather kernels at every support size 4..14 (the rule's P for these accuracies
    and strains), xi taken from the grid as SURVEY.md 8(d) prescribes, a few thousand particles (many bins, several passes per bin)."""
    rng = np.random.default_rng(5000 + seed)
    err = [1e-3, 1e-4, 1e-5, 1e-6, 1e-7][seed % 5]
    max_strain = [0.5, 0.0][(seed // 5) % 2]
    s = math.sqrt(-math.log(err))
    grid = tuple(int(g) for g in rng.choice([32, 36, 40, 45, 48, 50, 54, 60, 64], 3))
    if seed % 7 == 3:
        grid = (grid[0], grid[1], grid[2] | 1)                       # odd Nz: the gather leaves the binned path
    h = rng.uniform(0.6, 0.9, 3)
    Lx, Ly, Lz = (float(grid[a] * h[a]) for a in range(3))
    xi = float(0.9 * min(math.pi / (2.0 * h[a] * s) for a in range(3)))
    xy = float(rng.uniform(-0.5, 0.5)) if seed % 3 else 0.0
    n = int(rng.integers(200, 2500))                                 # the O(N^2) oracle times the Lanczos count bounds the size
    f = rng.uniform(-0.5, 0.5, (n, 3))
    pos = np.empty((n, 3))
    pos[:, 1] = f[:, 1] * Ly
    pos[:, 2] = f[:, 2] * Lz
    pos[:, 0] = f[:, 0] * Lx + xy * pos[:, 1]
    return dict(box=(Lx, Ly, Lz, xy), xi=xi, err=err, grid=grid, pos=pos, force=rng.normal(size=(n, 3)), n=n,
                seed=int(rng.integers(1, 2 ** 31)), max_strain=max_strain)


@pytest.mark.parametrize("seed", list(range(12)) + list(range(100, 130)))
def test_random_configuration(oracle, seed):
    import torch
    import pse_amd
    assert torch.cuda.is_available()
    c = config(seed) if seed < 100 else config_fast(seed - 100)
    ms = c.get("max_strain", 0.5)
    p = oracle.select_params(c["box"], c["xi"], c["err"], ms, grid=c["grid"])
    if p["eta"] >= 1.0:
        pytest.skip("the drawn grid is too coarse for this xi (eta >= 1: the engine refuses it, as the rule demands)")
    if p["rcut"] > 0.5 * min(c["box"][:3]) / 1.05:
        pytest.skip("cutoff beyond half the box")
    eng = pse_amd.Engine(max(c["n"], 8), c["box"], xi=c["xi"], error=c["err"], max_strain=ms, grid=c["grid"] or (0, 0, 0), seed=c["seed"])
    i = eng.info()
    assert (i["Nx"], i["Ny"], i["Nz"]) == p["grid"] and i["P"] == p["P"] and abs(i["eta"] - p["eta"]) < 1e-13
    pos, force = c["pos"], c["force"]
    ur = eng.mobility(to4(pos), to4(force), parts=1).cpu().numpy()[:, :3]
    ref_r = oracle.mobility_real(pos, force, c["box"], c["xi"], i["rcut"], rounded=False)
    assert rel(ur, ref_r) < 1e-12, ("near field", seed, rel(ur, ref_r))
    uw = eng.mobility(to4(pos), to4(force), parts=2).cpu().numpy()[:, :3]
    ref_w = oracle.mobility_wave(pos, force, c["box"], p)
    assert rel(uw, ref_w) < 1e-10, ("far field", seed, rel(uw, ref_w))
    u = eng.mobility(to4(pos), to4(force)).cpu().numpy()[:, :3]
    assert rel(u, ref_r + ref_w) < 1e-10
    vel, m = eng.brownian_velocity(to4(pos), to4(force), 0.7, 2e-3, 5 + seed)
    ref, mref = oracle.brownian_velocity(pos, force, c["box"], p, 0.7, 2e-3, c["seed"], 5 + seed, pair_rounded=True)
    assert m == mref, (seed, m, mref)
    assert rel(vel.cpu().numpy()[:, :3], ref) < 1e-9, ("Brownian", seed, rel(vel.cpu().numpy()[:, :3], ref))
    # the truth: the un-rounded algorithm (beyond the dense matrix: a fixed 1e-6 relative, m within one)
    tru, mt = oracle.brownian_velocity(pos, force, c["box"], p, 0.7, 2e-3, c["seed"], 5 + seed, pair_rounded=False)
    # (MI355X, all 42 configurations: at most 4.7e-7, m equal in every one)
    print(f"truth random {seed} Brownian: rel {rel(vel.cpu().numpy()[:, :3], tru):.2e}, m {m} / {mt}", flush=True)
    assert abs(m - mt) <= 1 and rel(vel.cpu().numpy()[:, :3], tru) < 1e-6, ("Brownian truth", seed, m, mt, rel(vel.cpu().numpy()[:, :3], tru))
    if seed % 3 == 0 and c["n"] >= 64:
        # a particle GROUP (d_group_members / group_size of the reference): the listed particles interact among themselves only, the
        # others keep what they had; and the stand-alone near-field square root on the same group
        n = c["n"]
        members = np.sort(np.random.default_rng(seed).choice(n, size=(2 * n) // 3, replace=False)).astype(np.int32)
        g = torch.tensor(members, dtype=torch.int32, device="cuda")
        vel = to4(np.full((n, 3), -3.0), w=1.25)
        eng.mobility(to4(pos), to4(force), vel=vel, group=g)
        v = vel.cpu().numpy()
        sub_ref = oracle.mobility_real(pos[members], force[members], c["box"], c["xi"], i["rcut"], rounded=False) + oracle.mobility_wave(pos[members], force[members], c["box"], p)
        assert rel(v[members, :3], sub_ref) < 1e-10, ("group", seed)
        others = np.setdiff1d(np.arange(n), members)
        assert np.all(v[others, :3] == -3.0) and np.all(v[:, 3] == 1.25)
        psi = np.random.default_rng(seed + 1).normal(size=(n, 3))
        out, ms = eng.sqrt_mreal(to4(pos), to4(psi), tol=1e-4, group=g)
        mv = lambda x: oracle.mobility_real(pos[members], np.ascontiguousarray(x), c["box"], c["xi"], i["rcut"], rounded=True)   # noqa: E731
        up, mp = oracle.lanczos_sqrt(mv, psi[members], 2, 1e-4)
        assert ms == mp and rel(out.cpu().numpy()[members, :3], up) < 1e-9, ("sqrt on a group", seed, ms, mp)
        mvt = lambda x: oracle.mobility_real(pos[members], np.ascontiguousarray(x), c["box"], c["xi"], i["rcut"], rounded=False)   # noqa: E731
        ut, mt = oracle.lanczos_sqrt(mvt, psi[members], 2, 1e-4)
        # (MI355X, 13 configurations: at most 4.9e-7, m equal)
        print(f"truth random {seed} sqrt on a group: rel {rel(out.cpu().numpy()[members, :3], ut):.2e}, m {ms} / {mt}", flush=True)
        assert abs(ms - mt) <= 1 and rel(out.cpu().numpy()[members, :3], ut) < 1e-6, ("sqrt on a group, truth", seed, ms, mt)
    if seed % 2 == 0 and c["n"] >= 8:
        # the force provider on the same cell grid (soft repulsion, O(N^2) port) and one full sheared step: Euler update and the
        # triclinic wrap in a box with three different edges (PSEv1/Stokes.cu:156-190)
        n = c["n"]
        fr = eng.pair_repulsion(to4(pos), to4(np.zeros((n, 3))), 25.0, 2.0, accumulate=False).cpu().numpy()[:, :3]
        fr_ref = oracle.pair_repulsion(pos, c["box"], 25.0, 2.0)
        assert np.abs(fr - fr_ref).max() < 1e-11 * max(1.0, np.abs(fr_ref).max()), ("repulsion", seed)
        dt, rate, ts = 0.05, 0.6, 40 + seed
        dpos, dvel = to4(pos, w=3.0), to4(np.zeros((n, 3)), w=2.0)           # velocity.w carries the mass (HOOMD)
        accel = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        image = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
        eng.step(dpos, dvel, accel, image, to4(force, w=0.5), 0.7, dt, ts, shear_rate=rate)
        u, _ = oracle.brownian_velocity(pos, force, c["box"], p, 0.7, dt, c["seed"], ts, pair_rounded=True)
        newpos, newimg = oracle.integrate(pos, np.zeros((n, 3), dtype=np.int64), u, c["box"], dt, rate)
        got = dpos.cpu().numpy()
        same = np.all(image.cpu().numpy() == newimg, axis=1)          # a particle that lands within rounding of a face may wrap either way
        assert same.sum() >= n - 1, ("images", seed, n - same.sum())
        assert np.abs(got[same, :3] - newpos[same]).max() < 1e-8, ("step", seed, np.abs(got[same, :3] - newpos[same]).max())
        assert np.all(got[:, 3] == 3.0) and np.abs(accel.cpu().numpy() - force / 2.0).max() < 1e-15
        # the truth: the velocity the device's step wrote against the un-rounded algorithm (a fixed 1e-6 relative)
        ut, _ = oracle.brownian_velocity(pos, force, c["box"], p, 0.7, dt, c["seed"], ts, pair_rounded=False)
        # (MI355X, 20 configurations: at most 2.4e-7)
        print(f"truth random {seed} step velocity: rel {rel(dvel.cpu().numpy()[:, :3], ut):.2e}", flush=True)
        assert rel(dvel.cpu().numpy()[:, :3], ut) < 1e-6, ("step truth", seed, rel(dvel.cpu().numpy()[:, :3], ut))
    eng.close()
