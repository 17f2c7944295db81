"""The wave-space stage of a step on its own, grid to grid, at every mode: forward transforms (z, y, x), the k-space operator (+ noise),
inverse transforms -- Engine.debug_wave_grid, the code a step runs -- against the long-double reference of tests/wave_grid_ref.py,
for every transform kernel and plan the host can select (wave_grid_ref.CASES; Engine.fft_path() must name the one the case is for).

The end-to-end checks (tests/test_gpu_parity.py) send a Gaussian-spread field through the physical operator, whose
exp(-(1 - eta) k^2 / 4 xi^2) leaves ~90 % of the modes of these grids below 1e-16 of the largest: a transform that is wrong there passes
them (tests/test_wave_grid_ref_cpu.py keeps the demonstration).  Here the operator runs at eta = 1, where the factor is algebraic.

Per case, all with the device grids poisoned (NaN in every double of both allocations, pad columns included) before the input goes in:
  white     standard-normal input at eta = 1;
  delta     a unit value at (Nx - 1, 1, Nz - 2) of component 1 (flat spectrum, known phases: a permuted output order shows);
  physical  the white input through the engine's own xi, eta;
  noise     no input, the k-space noise at eta = 1 and at the engine's own eta;
  twice     the white case again after the others: bit-identical (no state in the spectra or the pad).
Bound: FACTOR = 32 times e_ref, the error of the float64 NumPy pipeline against the long-double one for that very case, in real space
(max |out - ref| / max |ref|) and per mode (the same of the half spectra).  32 covers the other radix decompositions (up to nine
stages), the few-ulp rsqrt / sin / exp of the operator and rocFFT where it serves an axis; one mode wrong by 1e-3 sits at 1e+7 x e_ref.
Measured on the MI355X: e_ref 4e-17 ... 1e-15 over the cases, the device at most 14.8 x e_ref (the delta input at 60 x 20 x 16, where e_ref
of the nearly exact float64 transform of a single node is smallest), 8.8 x for the other inputs; per kernel family in docs/HISTORY.md."""
import os

import numpy as np
import pytest

import wave_grid_ref as wg

pytestmark = pytest.mark.gpu
LD = wg.LD
FFT_SWITCHES = ("PSE_OWN_Y", "PSE_OWN_Y_POW2", "PSE_OWN_Z", "PSE_XMIX", "PSE_NO_XFUSE", "PSE_XFFT_SMALL_KB", "PSE_YFFT_KB")
WORST = {}       # (axis kernel, ...) -> worst error / e_ref seen


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _check(what, out, ref, yard, path):
    ok, text, ratio = wg.within(out, ref, yard)
    for key in (("x", path["x"], path["x_kb"]), ("y", path["y"], path["y_kb"]), ("z", path["z"]), ("case", what.split(",")[0])):
        WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"  {what}: {text}")
    assert ok, f"{what}: {text}  [{path}]"


def _run_case(case, expect_path):
    import pse_amd
    grid, xy, _ = case
    box, p = wg.case_params(grid, xy)
    eng = pse_amd.Engine(8, box, xi=wg.XI, error=wg.ERROR, seed=wg.SEED, grid=grid, P=4)
    try:
        info = eng.info()
        assert (info["Nx"], info["Ny"], info["Nz"], info["P"]) == tuple(grid) + (4,) and abs(info["eta"] - p["eta"]) < 1e-14
        path = eng.fft_path()
        print(f"  {wg.case_id(case)}: {path}")
        expect_path(path, case)
        x, d = wg.white(grid), wg.delta(grid)
        # white, eta = 1                      (MI355X: at most 7.8 x e_ref over the matrix -- at 60 x 20 x 16; real <= 1.3e-15, per mode <= 1.1e-15)
        ref, yard = wg.wave_grid(x, box, p, eta=1.0, dtype=LD), wg.wave_grid(x, box, p, eta=1.0)
        first = eng.debug_wave_grid(x, eta=1.0)
        _check("white", first, ref, yard, path)
        # delta                               (MI355X: at most 14.8 x e_ref -- 60 x 20 x 16, per mode; real <= 7.5e-16, per mode <= 2.3e-15)
        out = eng.debug_wave_grid(d, eta=1.0)
        _check("delta", out, wg.wave_grid(d, box, p, eta=1.0, dtype=LD), wg.wave_grid(d, box, p, eta=1.0), path)
        # the engine's own operator           (MI355X: at most 8.5 x e_ref -- 16 x 18 x 15; real <= 1.1e-15, per mode <= 1.1e-15)
        out = eng.debug_wave_grid(x)
        _check("physical", out, wg.wave_grid(x, box, p, dtype=LD), wg.wave_grid(x, box, p), path)
        # the noise, without input            (MI355X: at most 6.9 x e_ref at eta = 1, 8.8 at the engine's eta -- 16 x 18 x 15; real <= 2.5e-15, per mode <= 6.3e-16)
        for eta in (1.0, None):
            nk = wg.noise_spectrum(box, p, eta=eta)
            out = eng.debug_wave_grid(None, eta=eta or 0.0, noise=True, kT=wg.KT, dt=wg.DT, timestep=wg.TIMESTEP)
            _check(f"noise, eta = {eta or p['eta']:.3g}", out, wg.wave_grid(None, box, p, eta=eta, noise=nk, dtype=LD),
                   wg.wave_grid(None, box, p, eta=eta, noise=nk), path)
        again = eng.debug_wave_grid(x, eta=1.0)
        # twice                               (MI355X: bit-identical in all cases)
        assert np.array_equal(again, first), "the white case differs after other inputs: state left in the spectra or the pad"
    finally:
        eng.close()


def _default_path(path, case):
    assert path == case[2], (path, case[2])


@pytest.mark.parametrize("case", wg.CASES, ids=[wg.case_id(c) for c in wg.CASES])
def test_wave_grid(torch_cuda, oracle, monkeypatch, case):
    for name in FFT_SWITCHES:                       # (read per handle, in pse_create)
        monkeypatch.delenv(name, raising=False)
    _run_case(case, _default_path)


def _path_under_switches(path, case):
    """tests/test_gpu_switches.py runs the switch sizes with one switch set: the path is the default one except for what that switch
    selects (the rules of make_plans, xfft_choice and yfft_choice, restated)."""
    grid, _, want = case
    env = os.environ
    exp = dict(want)
    if env.get("PSE_NO_XFUSE"):                                                   # ... and the own y and z passes need the fused x pass
        exp.update(xfuse=0, own_y=0, own_z=0, x=wg.X_ROC, x_kb=0, y=wg.ROC, y_kb=0, z=wg.ROC)
    if env.get("PSE_OWN_Y") == "0" or (env.get("PSE_OWN_Y_POW2") == "0" and want["y"] == wg.Y_REGS):
        exp.update(own_y=0, own_z=0, y=wg.ROC, y_kb=0, z=wg.ROC)                  # (the own z pass runs under an own y pass only)
    if env.get("PSE_OWN_Z") == "0":
        exp.update(own_z=0, z=wg.ROC)
    if env.get("PSE_XMIX") == "1" and grid[0] & (grid[0] - 1):                    # runtime plans: four columns up to 200 points, two above
        exp.update(x=wg.X_RT, x_kb=4 if grid[0] <= 200 else 2)
    if env.get("PSE_XFFT_SMALL_KB") == "8" and want["x"] == wg.X_LDS:
        exp.update(x_kb=8)
    if env.get("PSE_YFFT_KB") in ("2", "8") and want["y"] in (wg.Y_CT, wg.Y_RT):
        exp.update(y=wg.Y_RT, y_kb=int(env["PSE_YFFT_KB"]))
    assert path == exp, (path, exp)


@pytest.mark.parametrize("case", wg.SWITCH_CASES, ids=[wg.case_id(c) for c in wg.SWITCH_CASES])
def test_wave_grid_at_the_switch_sizes(torch_cuda, oracle, case):
    _run_case(case, _path_under_switches)


def test_worst_errors_per_kernel(torch_cuda):
    """Not an assertion of its own: the figures docs/HISTORY.md records, per kernel family, in units of e_ref."""
    for key, ratio in sorted(WORST.items()):
        print(f"worst error / e_ref: {' '.join(map(str, key))}: {ratio:.1f}")
    assert all(r <= wg.FACTOR for r in WORST.values())
