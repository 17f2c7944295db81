"""Reference of the wave-space stage from grid to grid (host only, NumPy): what Engine.debug_wave_grid computes,

    out = irfftn( wave_scale(rfftn(x)) [+ noise_k], norm="forward" )

with oracle/pse_port.py's wave_scale and noise_k on a copy of the parameters that carries the xi / eta overrides.  With
dtype = np.longdouble the transforms and the products run in the 80-bit format (numpy.fft keeps long double): that is the reference.
With np.float64 it is the yardstick: the difference of the two, e_ref, is the error a correct float64 implementation of the same
operation makes, and the bound of the device tests is a multiple of it (tests/test_gpu_wave_grid.py).

Why eta = 1: the physical operator carries exp(-(1 - eta) k^2 / 4 xi^2), which on the oversampled grids that select the engine's own
transform kernels damps ~90 % of the modes below 1e-16 of the largest -- a transform that is wrong there changes nothing anyone
compares.  At eta = 1 the factor is 6 pi (1 + q) / k^2 sinc^2 / Ng: algebraic, every mode but the zeros of sin|k| carries weight
(coverage() measures it)."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import pse_port

LD = np.longdouble
AXES = (1, 2, 3)
XI, ERROR, MAX_STRAIN = 0.5, 1e-3, 0.5
FACTOR = 32          # the device may lie FACTOR x e_ref from the long-double reference
SEED, TIMESTEP, KT, DT = 31, 4, 1.0, 1e-3      # of the noise cases


# ------------------------------------------------------------------------------------------ boxes and parameters
def axis_length(n, long_x=False):
    """Box length for n nodes: h = 0.77 on a short axis (never shorter than 12.3 = 2 rcut + a margin); a long axis keeps L = 24.3, and
    a long x axis -- the spacing the spreading Gaussian is sized by -- is stretched beyond 256 nodes so that hx stays at 24.3 / 256.
    The lengths are not multiples of 1 / 2: |k| = 2 pi |(i / Lx, j / Ly, k / Lz)| then misses the zeros n pi of sin |k|, which a box of
    L = 12 or 24 hits exactly at 0.3 % of its modes (coverage())."""
    if n <= 64:
        return max(12.3, 0.77 * n)
    return 24.3 * max(1.0, n / 256.0) if long_x else 24.3


def case_box(grid, xy):
    return (axis_length(grid[0], True), axis_length(grid[1]), axis_length(grid[2]), float(xy))


def case_params(grid, xy, P=4):
    box = case_box(grid, xy)
    return box, pse_port.select_params(box, XI, ERROR, MAX_STRAIN, grid=tuple(grid), P=P)


def _with(p, xi=None, eta=None):
    q = dict(p)
    if xi:
        q["xi"] = float(xi)
    if eta:
        q["eta"] = float(eta)
    return q


# ------------------------------------------------------------------------------------------ inputs
def white(grid, seed=7):
    """Standard-normal grids, a stream of its own per component."""
    return np.stack([np.random.default_rng([seed, c]).standard_normal(tuple(grid)) for c in range(3)])


def delta(grid, comp=1, node=None):
    """A unit value in one component at an off-origin node: a flat spectrum with known phases."""
    node = (grid[0] - 1, 1, grid[2] - 2) if node is None else node
    x = np.zeros((3,) + tuple(grid))
    x[(comp,) + tuple(node)] = 1.0
    return x


# ------------------------------------------------------------------------------------------ the pipeline
def _per_component(fn, x):
    """The three components side by side (the long-double transforms are the cost of a reference; they release the interpreter)."""
    with ThreadPoolExecutor(max_workers=3) as pool:
        return np.stack(list(pool.map(fn, x)))


def rfft3(x, dtype=np.float64):
    return _per_component(lambda a: np.fft.rfftn(np.asarray(a, dtype=dtype)), x)


def irfft3(uh, grid):
    return _per_component(lambda a: np.fft.irfftn(a, s=tuple(grid), axes=(0, 1, 2), norm="forward"), uh)   # unnormalised: 1 / Ng lives in w


def noise_spectrum(box, p, xi=None, eta=None, seed=SEED, timestep=TIMESTEP, kT=KT, dt=DT):
    return pse_port.noise_k(box, _with(p, xi, eta), kT, dt, seed, timestep)


def wave_grid(x, box, p, xi=None, eta=None, noise=None, dtype=np.float64, pre=None, scale=None, post=None):
    """x: (3, Nx, Ny, Nz) or None (zeros); noise: None or a half spectrum (noise_spectrum) added after the operator.
    pre / scale / post: where tests/test_wave_grid_ref_cpu.py plants defects -- pre(fh) after the forward transforms, scale in place of
    pse_port.wave_scale, post(uh) before the inverse transforms."""
    q = _with(p, xi, eta)
    grid = p["grid"]
    ctype = np.result_type(dtype, np.complex64)
    if x is None:
        uh = np.zeros((3, grid[0], grid[1], grid[2] // 2 + 1), dtype=ctype)
    else:
        fh = rfft3(x, dtype)
        if pre is not None:
            fh = pre(fh)
        uh = (scale or pse_port.wave_scale)(fh, box, q)
    if noise is not None:
        uh = uh + noise
    if post is not None:
        uh = post(uh)
    out = irfft3(uh.astype(ctype, copy=False), grid)
    assert out.dtype == dtype, out.dtype
    return out


# ------------------------------------------------------------------------------------------ comparison
def compare(out, ref):
    """(real-space error, per-mode error, worst mode (component, i, j, k)): max |out - ref| over the largest |ref|, and the same of
    the half spectra.  The difference is formed in the reference's precision; its transform needs no more than float64 (it is
    relative to the difference), the reference's own spectrum is taken in float64 for its largest mode only."""
    out = np.asarray(out)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    if not np.isfinite(out).all():
        bad = np.argwhere(~np.isfinite(out))
        return math.inf, math.inf, tuple(int(v) for v in bad[0]) + (len(bad),)
    d = (out.astype(ref.dtype) - ref)
    e_real = float(np.abs(d).max() / np.abs(ref).max())
    dm = np.abs(np.fft.rfftn(d.astype(np.float64), axes=AXES))
    top = np.abs(np.fft.rfftn(ref.astype(np.float64), axes=AXES)).max()
    worst = np.unravel_index(int(np.argmax(dm)), dm.shape)
    return e_real, float(dm.max() / top), tuple(int(v) for v in worst)


def within(out, ref, yard):
    """Is `out` within FACTOR x e_ref of ref, in real space and per mode?  yard: the float64 pipeline's output for the same case.
    Returns (ok, text, ratio): the text names the figures and the worst mode, ratio is the larger of the two errors in units of e_ref."""
    er, em, _ = compare(yard, ref)
    dr, dm, worst = compare(out, ref)
    text = (f"real {dr:.2e} (e_ref {er:.2e}, x{dr / er:.1f}), per mode {dm:.2e} (e_ref {em:.2e}, x{dm / em:.1f}), "
            f"worst mode (component, i, j, k) = {worst}")
    return dr <= FACTOR * er and dm <= FACTOR * em, text, max(dr / er, dm / em)


# ------------------------------------------------------------------------------------------ coverage
def coverage(box, p, xi=None):
    """At eta = 1: the share of the half-spectrum modes whose operator weight w sinc^2 is >= 1e-9 of the largest, and whose noise
    weight sqrt(w) sinc is >= 1e-6 of the largest."""
    _, _, _, _, w, sinc = pse_port.kvectors(box, _with(p, xi, 1.0))
    op = np.abs(w * sinc * sinc)
    nz = np.abs(np.sqrt(w) * sinc)
    return float((op >= 1e-9 * op.max()).mean()), float((nz >= 1e-6 * nz.max()).mean())


def masked(box, p, level):
    """The share of the modes whose weight under the PHYSICAL operator (the handle's own eta) is below `level` of the largest."""
    _, _, _, _, w, sinc = pse_port.kvectors(box, p)
    op = np.abs(w * sinc * sinc)
    return float((op < level * op.max()).mean())


# ------------------------------------------------------------------------------------------ the GPU matrix
# (grid, xy, what Engine.fft_path() must report).  The named axis has the size its kernel requires, the others are as small as the
# selection allows; P = 4 everywhere.  own_y needs the fused x pass and a Ny that is not a power of two (or 256 / 512), own_z needs
# own_y: tests/test_gpu_wave_grid.py asserts the path, so a change of a dispatch rule cannot silently move a case to another kernel.
X_LDS, X_REGS, X_CT, X_RT, X_ROC = "k_xfft_scale", "k_xfft_scale_cols", "k_xfft_scale_mixed/ct", "k_xfft_scale_mixed/rt", "rocfft+k_scale"
Y_CT, Y_RT, Y_REGS, ROC = "k_fft_cols/ct", "k_fft_cols/rt", "k_yfft_regs", "rocfft"
Z_ROWS, Z_G = "k_zfft_rows", "k_zfft_rows_g"


def _c(grid, xy, x, x_kb, y, y_kb, z):
    return (tuple(grid), xy, dict(xfuse=int(x != X_ROC), own_y=int(y != ROC), own_z=int(z != ROC), x=x, x_kb=x_kb, y=y, y_kb=y_kb, z=z))


CASES = [
    # x: the LDS pass, two columns per workgroup; Nzh = 8 and 16 are multiples of the column count, 11 and 23 are not
    _c((16, 18, 15), 0.1, X_LDS, 2, Y_RT, 4, ROC), _c((32, 16, 20), 0.0, X_LDS, 2, ROC, 0, ROC),
    _c((64, 20, 45), -0.2, X_LDS, 2, Y_RT, 4, ROC), _c((128, 16, 30), 0.1, X_LDS, 2, ROC, 0, ROC),
    # ... eight columns: rows x ceil(Nzh / 8) >= 1024 (Nzh = 65: not a multiple; 16: a multiple)
    _c((16, 128, 128), 0.2, X_LDS, 8, ROC, 0, ROC), _c((16, 512, 30), 0.0, X_LDS, 8, ROC, 0, ROC),
    # x: the register passes
    _c((256, 16, 18), 0.2, X_REGS, 8, ROC, 0, ROC), _c((360, 18, 16), 0.1, X_REGS, 4, Y_RT, 4, ROC), _c((512, 16, 16), -0.1, X_REGS, 4, ROC, 0, ROC),
    # x: mixed radix, compile-time plans
    _c((180, 16, 16), 0.0, X_CT, 4, ROC, 0, ROC), _c((270, 16, 20), -0.1, X_CT, 2, ROC, 0, ROC),
    _c((375, 20, 16), 0.3, X_CT, 2, Y_RT, 4, ROC), _c((500, 16, 18), 0.2, X_CT, 2, ROC, 0, ROC),
    # x: runtime plans, four columns (18 = 9 2, 20 = 5 4, 24 = 8 3, 45 = 9 5, 50 = 5 5 2, 60 = 5 4 3, 90 = 9 5 2, 120 = 8 5 3) and two
    _c((18, 16, 16), 0.1, X_RT, 4, ROC, 0, ROC), _c((20, 18, 16), 0.0, X_RT, 4, Y_RT, 4, ROC), _c((24, 16, 18), -0.3, X_RT, 4, ROC, 0, ROC),
    _c((45, 16, 16), 0.2, X_RT, 4, ROC, 0, ROC), _c((50, 16, 20), 0.0, X_RT, 4, ROC, 0, ROC), _c((60, 20, 16), 0.1, X_RT, 4, Y_RT, 4, ROC),
    _c((90, 16, 16), -0.2, X_RT, 4, ROC, 0, ROC), _c((120, 18, 16), 0.0, X_RT, 4, Y_RT, 4, ROC),
    _c((225, 16, 16), 0.1, X_RT, 2, ROC, 0, ROC), _c((240, 16, 18), -0.1, X_RT, 2, ROC, 0, ROC),
    # x not fused (Nx outside 16..512): rocFFT's 3-D plan + k_scale with its Nyquist branches (even sizes, with and without tilt) and without (odd)
    _c((12, 16, 16), 0.3, X_ROC, 0, ROC, 0, ROC), _c((12, 15, 18), 0.0, X_ROC, 0, ROC, 0, ROC), _c((600, 16, 16), 0.1, X_ROC, 0, ROC, 0, ROC),
    # y: k_fft_cols, runtime plans over every radix
    _c((16, 24, 16), 0.2, X_LDS, 2, Y_RT, 4, ROC), _c((16, 45, 18), -0.1, X_LDS, 2, Y_RT, 4, ROC), _c((16, 50, 16), 0.0, X_LDS, 2, Y_RT, 4, ROC),
    _c((16, 60, 15), 0.3, X_LDS, 2, Y_RT, 4, ROC), _c((16, 90, 16), 0.1, X_LDS, 2, Y_RT, 4, ROC), _c((16, 120, 16), -0.2, X_LDS, 2, Y_RT, 4, ROC),
    # y: compile-time plans
    _c((16, 360, 16), 0.1, X_LDS, 2, Y_CT, 4, ROC), _c((16, 270, 18), 0.0, X_LDS, 2, Y_CT, 4, ROC),
    _c((18, 375, 16), -0.3, X_RT, 4, Y_CT, 4, ROC), _c((16, 500, 16), 0.2, X_LDS, 2, Y_CT, 4, ROC),
    # y: the register pass at 256 with rocFFT's z pass and with the own one, at 512 with Nz = 180
    _c((16, 256, 16), 0.2, X_LDS, 2, Y_REGS, 8, ROC), _c((16, 256, 180), 0.0, X_LDS, 8, Y_REGS, 8, Z_G), _c((16, 512, 180), 0.1, X_LDS, 8, Y_REGS, 4, Z_G),
    # z: k_zfft_rows
    _c((16, 18, 256), 0.1, X_LDS, 2, Y_RT, 4, Z_ROWS), _c((16, 18, 512), -0.2, X_LDS, 2, Y_RT, 4, Z_ROWS),
    # z: k_zfft_rows_g at its eleven sizes
    _c((16, 18, 360), 0.1, X_LDS, 2, Y_RT, 4, Z_G), _c((18, 20, 270), 0.0, X_RT, 4, Y_RT, 4, Z_G), _c((16, 18, 180), -0.2, X_LDS, 2, Y_RT, 4, Z_G),
    _c((20, 18, 240), 0.0, X_RT, 4, Y_RT, 4, Z_G), _c((16, 20, 300), 0.15, X_LDS, 2, Y_RT, 4, Z_G), _c((16, 18, 320), 0.0, X_LDS, 2, Y_RT, 4, Z_G),
    _c((16, 18, 384), 0.3, X_LDS, 2, Y_RT, 4, Z_G), _c((18, 18, 400), 0.1, X_RT, 4, Y_RT, 4, Z_G), _c((16, 18, 450), 0.0, X_LDS, 2, Y_RT, 4, Z_G),
    _c((16, 20, 480), -0.1, X_LDS, 2, Y_RT, 4, Z_G), _c((16, 18, 500), 0.2, X_LDS, 2, Y_RT, 4, Z_G),
]
# the sizes at which the developer switches of the transforms select other kernels (tests/test_gpu_switches.py)
SWITCH_GRIDS = [(32, 16, 20), (16, 18, 15), (180, 16, 16), (360, 18, 16), (256, 16, 18), (16, 360, 16), (16, 45, 18), (16, 256, 16),
                (16, 18, 256), (16, 18, 360)]
SWITCH_CASES = [c for c in CASES if c[0] in SWITCH_GRIDS]


def case_id(c):
    return "x".join(map(str, c[0])) + f"-xy{c[1]}"


def families(cases=CASES):
    """Every (axis, kernel, columns) the cases name: what test_every_kernel_family_is_in_the_matrix holds against the list of the issue."""
    out = set()
    for grid, _, path in cases:
        out.add(("x", path["x"], path["x_kb"], grid[0]))
        out.add(("y", path["y"], path["y_kb"], grid[1]))
        out.add(("z", path["z"], grid[2]))
    return out
