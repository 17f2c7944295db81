"""CPU tests of tests/wave_grid_ref.py: the grid-to-grid check of the wave-space stage discriminates, and the reference alone meets the
conditions tests/test_gpu_wave_grid.py rests on.

  (a) the float64 pipeline lies within the device's bound of the long-double one (it IS e_ref: the assertion is that the bound is
      FACTOR x a number of the expected size, 1e-16 ... 2e-15, and that both pipelines run in the precision they claim);
  (b) every planted defect fails the bound: a band of high modes zeroed (per axis), a sign flip from one mode up, ONE mode off by
      1e-3, the partner term of the Nyquist symmetrisation dropped, the flip of the noise's conjugate partner dropped on the kz = 0
      plane, one stale pad value mixed into the last live mode of one row;
  (c) the mode-band, sign-flip and single-mode plants change the EXISTING style of check -- gathered velocities of a Gaussian-spread
      force field through the physical operator at (32, 36, 360), the check of tests/test_gpu_parity.py with its bound of 1e-10 --
      by less than 1e-10: why the grid-to-grid test exists;
  (d) the coverage condition holds for every grid of the GPU matrix, the engine accepts every case's parameters, and the matrix
      names every kernel family and plan."""
import ctypes

import numpy as np
import pytest

from conftest import make_suspension
import wave_grid_ref as wg

LD = wg.LD
# even / odd / mixed, all with a tilt
GRIDS = [((16, 18, 20), 0.3), ((15, 9, 25), -0.2), ((12, 15, 16), 0.1)]
IDS = ["x".join(map(str, g)) for g, _ in GRIDS]


@pytest.fixture(scope="module", params=GRIDS, ids=IDS)
def case(request, oracle):
    grid, xy = request.param
    box, p = wg.case_params(grid, xy)
    x = wg.white(grid)
    r = dict(grid=grid, box=box, p=p, x=x)
    r["ref"] = wg.wave_grid(x, box, p, eta=1.0, dtype=LD)
    r["yard"] = wg.wave_grid(x, box, p, eta=1.0)
    r["noise"] = wg.noise_spectrum(box, p, eta=1.0)
    r["nref"] = wg.wave_grid(None, box, p, eta=1.0, noise=r["noise"], dtype=LD)
    r["nyard"] = wg.wave_grid(None, box, p, eta=1.0, noise=r["noise"])
    return r


def test_float64_pipeline_is_the_yardstick(case):
    assert case["ref"].dtype == LD and case["yard"].dtype == np.float64
    for what, yard, ref in (("white", case["yard"], case["ref"]), ("noise", case["nyard"], case["nref"])):
        er, em, _ = wg.compare(yard, ref)
        print(f"{what}: e_ref real {er:.2e}, per mode {em:.2e}")
        assert 1e-17 < er < 2e-15 and 1e-18 < em < 2e-15, (what, er, em)
        ok, text, _ = wg.within(yard, ref, yard)
        assert ok, text


def _band(axis, lo, hi):
    def f(fh):
        fh = fh.copy()
        sl = [slice(None)] * 4
        sl[1 + axis] = slice(lo, hi)
        fh[tuple(sl)] = 0
        return fh
    return f


def _sign(axis, k0):
    def f(fh):
        fh = fh.copy()
        sl = [slice(None)] * 4
        sl[1 + axis] = slice(k0, None)
        fh[tuple(sl)] *= -1
        return fh
    return f


def _single(node, rel=1e-3):
    def f(fh):
        fh = fh.copy()
        fh[node] *= 1.0 + rel
        return fh
    return f


def _mode_plants(grid):
    nx, ny, nz = grid
    nzh = nz // 2 + 1
    return {"band x": _band(0, nx // 2 - 1, nx // 2 + 2), "band y": _band(1, ny // 2 - 1, ny // 2 + 2), "band z": _band(2, nzh - 3, nzh),
            "sign flip from kz = 3 up": _sign(2, 3), "sign flip from i = 5 up": _sign(0, 5),
            "one mode off by 1e-3": _single((2, nx - 2, ny // 2, nzh - 2))}


def _own_only(oracle):
    """wave_scale without the partner term of the symmetrisation: s(k) (I - kk) v(k) with the node's own folded wave vector."""
    def scale(fh, box, q):
        kx, ky, kz, k2, w, sinc = oracle.kvectors(box, q)
        return oracle._project(kx, ky, kz, k2, fh) * (w * sinc * sinc)
    return scale


def test_every_plant_fails_the_bound(case, oracle):
    x, box, p, grid = case["x"], case["box"], case["p"], case["grid"]
    ok, _, _ = wg.within(case["yard"], case["ref"], case["yard"])
    assert ok
    for name, pre in _mode_plants(grid).items():
        ok, text, _ = wg.within(wg.wave_grid(x, box, p, eta=1.0, pre=pre), case["ref"], case["yard"])
        print(f"{name}: {text}")
        assert not ok, name
    # the partner term matters where an index is a Nyquist index: a grid with an even axis
    bad = wg.wave_grid(x, box, p, eta=1.0, scale=_own_only(oracle))
    ok, text, _ = wg.within(bad, case["ref"], case["yard"])
    print(f"partner term dropped: {text}")
    assert ok == all(n % 2 for n in grid), text          # (an all-odd grid has no Nyquist index: the two operators are the same)
    # one stale value of the pad (of the size of a live mode) into the last live mode of ONE row, at 1e-3
    def pad(uh):
        uh = uh.copy()
        uh[0, 3, 2, -1] += 1e-3 * uh[0, 3, 2, -2]
        return uh
    ok, text, _ = wg.within(wg.wave_grid(x, box, p, eta=1.0, post=pad), case["ref"], case["yard"])
    print(f"pad value mixed in: {text}")
    assert not ok
    # the noise: the conjugate partner on the kz = 0 plane without its flip.  The operator is a real matrix per mode, so psi -> conj psi
    # conjugates the mode's output.
    nx, ny, nz = grid
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    flipped = ((nx - i) % nx * ny + (ny - j) % ny) < (i * ny + j)
    def noflip(uh):
        uh = uh.copy()
        uh[:, :, :, 0] = np.where(flipped[None], np.conj(uh[:, :, :, 0]), uh[:, :, :, 0])
        return uh
    ok, text, _ = wg.within(wg.wave_grid(None, box, p, eta=1.0, noise=case["noise"], post=noflip), case["nref"], case["nyard"])
    print(f"noise partner not flipped: {text}")
    assert not ok
    ok, text, _ = wg.within(case["nyard"], case["nref"], case["nyard"])
    assert ok, text


def test_physical_operator_hides_the_mode_plants(oracle):
    """The existing style of check at (32, 36, 360), L = 24, n = 1200 (tests/test_gpu_parity.py): its bound is 1e-10."""
    grid, xy, n = (32, 36, 360), 0.1, 1200
    pos, force, box = make_suspension(n, L=24.0, xy=xy)
    p = oracle.select_params(box, 0.5, 1e-3, 0.5, grid=grid, P=4)
    fh = np.fft.rfftn(oracle.spread(pos, force, box, p), axes=wg.AXES)

    def velocities(fh):
        return oracle.gather(np.fft.irfftn(oracle.wave_scale(fh, box, p), s=grid, axes=wg.AXES, norm="forward"), pos, box, p)
    good = velocities(fh)
    plants = {"kz modes 40..180 zeroed": _band(2, 40, 181), "sign of every kz mode >= 25 flipped": _sign(2, 25),
              "one mode off by 1e-3": _single((1, 9, 20, 120))}
    x = wg.white(grid)
    ref = wg.wave_grid(x, box, p, eta=1.0, dtype=LD)
    yard = wg.wave_grid(x, box, p, eta=1.0)
    for name, pre in plants.items():
        change = np.linalg.norm(velocities(pre(fh)) - good) / np.linalg.norm(good)
        ok, text, _ = wg.within(wg.wave_grid(x, box, p, eta=1.0, pre=pre), ref, yard)
        print(f"{name}: end-to-end check moves by {change:.1e}; grid to grid at eta = 1: {text}")
        assert change < 1e-10, (name, change)
        assert not ok, name
    m16, m10 = wg.masked(box, p, 1e-16), wg.masked(box, p, 1e-10)
    print(f"modes with weight < 1e-16 of the largest: {100 * m16:.1f} %, < 1e-10: {100 * m10:.1f} %")
    assert m16 > 0.85 and m10 > 0.9


@pytest.mark.parametrize("c", wg.CASES, ids=[wg.case_id(c) for c in wg.CASES])
def test_case_meets_the_coverage_condition(oracle, c):
    from pse_amd import _lib
    grid, xy, path = c
    assert np.prod(grid) <= 2e6
    box, p = wg.case_params(grid, xy)
    assert p["eta"] < 1.0
    op, nz = wg.coverage(box, p)
    print(f"{wg.case_id(c)}: operator weight >= 1e-9 of the largest at {100 * op:.2f} % of the modes, noise weight >= 1e-6 at {100 * nz:.2f} %")
    assert op >= 0.99 and nz >= 0.999, (op, nz)
    # the engine's own rule takes the parameters (pse_create runs the same function first)
    q = _lib.pse_params()
    q.n_max, q.Lx, q.Ly, q.Lz, q.xy = 8, box[0], box[1], box[2], box[3]
    q.xi, q.error, q.max_strain, q.seed = wg.XI, wg.ERROR, wg.MAX_STRAIN, wg.SEED
    q.Nx, q.Ny, q.Nz = grid
    q.P, q.rcut, q.device, q.n_slabs, q.slab_rank = 4, 0.0, -1, 1, 0
    info = _lib.pse_info()
    lib = _lib.load()
    assert lib.pse_host_select_params(ctypes.byref(q), ctypes.byref(info)) == 0, lib.pse_last_error().decode()
    assert (info.Nx, info.Ny, info.Nz, info.P) == tuple(grid) + (4,) and abs(info.eta - p["eta"]) < 1e-14


def test_every_kernel_family_is_in_the_matrix():
    """The list of the kernels and plans of the wave-space stage, written down from the launchers' domain and not from CASES."""
    fam = wg.families()
    want = {("x", wg.X_LDS, 2, n) for n in (16, 32, 64, 128)} | {("x", wg.X_LDS, 8, 16)}
    want |= {("x", wg.X_REGS, 8, 256), ("x", wg.X_REGS, 4, 360), ("x", wg.X_REGS, 4, 512)}
    want |= {("x", wg.X_CT, 4, 180)} | {("x", wg.X_CT, 2, n) for n in (270, 375, 500)}
    want |= {("x", wg.X_RT, 4, n) for n in (18, 20, 24, 45, 50, 60, 90, 120)} | {("x", wg.X_RT, 2, 225), ("x", wg.X_RT, 2, 240)}
    want |= {("x", wg.X_ROC, 0, 12), ("x", wg.X_ROC, 0, 600)}
    want |= {("y", wg.Y_RT, 4, n) for n in (18, 20, 24, 45, 50, 60, 90, 120)} | {("y", wg.Y_CT, 4, n) for n in (360, 270, 375, 500)}
    want |= {("y", wg.Y_REGS, 8, 256), ("y", wg.Y_REGS, 4, 512), ("y", wg.ROC, 0, 16), ("y", wg.ROC, 0, 128), ("y", wg.ROC, 0, 512)}
    want |= {("z", wg.Z_ROWS, 256), ("z", wg.Z_ROWS, 512)} | {("z", wg.Z_G, n) for n in (360, 270, 180, 240, 300, 320, 384, 400, 450, 480, 500)}
    want |= {("z", wg.ROC, 15), ("z", wg.ROC, 16)}
    assert want <= fam, sorted(want - fam)
    # radix coverage of the runtime plans: 9, 8, 5, 4, 3, 2 each lead or follow in some plan
    for axis in (0, 1):
        sizes = {c[0][axis] for c in wg.CASES if c[2]["xy"[axis]] in (wg.X_RT, wg.Y_RT)}
        radices = set()
        for n in sizes:
            for r in (9, 8, 5, 4, 3, 2):
                while n % r == 0:
                    radices.add(r); n //= r
        assert radices == {9, 8, 5, 4, 3, 2}, (axis, radices)
    assert len(wg.SWITCH_CASES) == len(wg.SWITCH_GRIDS)
