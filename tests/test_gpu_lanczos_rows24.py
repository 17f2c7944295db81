"""The Lanczos vectors of the single-GPU pair-list path in 24-byte rows (pse_handle.rows24; pse_device.h row24_load / row24_store): the
basis V[j >= 1] and the results of the pair-list mat-vecs hold (x, y, z) without the padding word of a double4.  The arithmetic is what
it was -- the same operations in the same order on the same numbers, the same rows per workgroup in every partial sum -- so an engine
created with PSE_ROWS24=0 (double4 rows, as before) and one created with the default must return the SAME BYTES: torch.equal on the
outputs, equal m, equal mat-vec counts.  Both engines live in one process and get the same positions, psi and seed.

What a 24-byte row can get wrong and a 32-byte row cannot is addressing: the sizes are a lone row, a partial wave on either side of
a wave boundary, one update workgroup exactly and more than one, and (4097) rows that straddle 128-byte lines at every phase.  phi
and xi as in tests/test_gpu_lanczos_update_sums.py, so that a pair list exists at these sizes.  pse_info has no field that names the
pair list or the layout; what shows both is device_bytes -- the packed engine is smaller by a quarter of the basis exactly when
the layout is in use, which needs the list -- and every case asserts it.

The far field is not bit-reproducible from run to run, so the Brownian velocity is compared through brownian_velocity_part(parts=1):
the near field plus the Lanczos noise at zero force, which is the whole of what the layout touches."""
import contextlib
import os

import numpy as np
import pytest

from conftest import make_suspension, to4

pytestmark = pytest.mark.gpu

ERR = 1e-3
TOL = 1e-6          # sqrt_mreal: m = 17 .. 19 beyond 1000 particles, so starting counts 1 and 2 run further batches
SEED = 7
KT, DT, TS = 1.0, 1e-3, 3
M_MAX = 100         # pse_host.h: the basis holds M_MAX + 1 vectors of n_max rows
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@contextlib.contextmanager
def environment(**kw):
    """Developer switches are read in pse_create: set (or, None, unset) for the engines created inside."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def case(n, seed=0):
    """tests/test_gpu_lanczos_update_sums.py case(): a box of 16 at xi = 0.5 up to 300 particles, phi = 0.3 at xi = 1 beyond."""
    pos, _, box = make_suspension(n, L=16.0, seed=12345 + seed) if n <= 300 else make_suspension(n, phi=0.3, seed=12345 + seed)
    psi = np.random.default_rng(1000 + n + seed).normal(size=(n, 3))
    return pos, box, psi, (0.5 if n <= 300 else 1.0)


def engines(n, box, xi, **env):
    """(double4 rows, default) -- two engines that differ in PSE_ROWS24 alone."""
    import pse_amd
    with environment(PSE_ROWS24="0", **env):
        plain = pse_amd.Engine(n, box, xi=xi, error=ERR, seed=SEED)
    with environment(PSE_ROWS24=None, **env):
        packed = pse_amd.Engine(n, box, xi=xi, error=ERR, seed=SEED)
    return plain, packed


def basis_quarter(n):
    """Bytes the basis shrinks by: (M_MAX + 1) n rows of 32 bytes against as many of 24, allocated in whole double4."""
    rows = (M_MAX + 1) * n
    return 32 * (rows - (3 * rows + 3) // 4)


def assert_packed(plain, packed, n):
    """The default engine runs on the packed layout (so it has a pair list): smaller by the basis' quarter, nothing else differs."""
    a, b = plain.info()["device_bytes"], packed.info()["device_bytes"]
    assert a - b == basis_quarter(n), (n, a, b, a - b, basis_quarter(n))


def same(torch, a, b, what):
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


@pytest.mark.parametrize("n", SIZES)
def test_sqrt_mreal_same_bytes(torch_cuda, n):
    """Host-checked: iteration 0 is a pair-list mat-vec on psi (no M psi rode along with a build pass); from the starting counts 1 and 2
    a batch ends on a scalars-only iteration whose vector part follows, then further batches; at m and m + 3 one batch decides."""
    torch = torch_cuda
    pos, box, psi, xi = case(n)
    plain, packed = engines(n, box, xi)
    assert_packed(plain, packed, n)
    dpos, dpsi = to4(pos), to4(psi)
    _, m_conv = plain.sqrt_mreal(dpos, dpsi, tol=TOL)
    for m_in in (1, 2, m_conv, m_conv + 3):
        a, ma = plain.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        ia = plain.info()
        b, mb = packed.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        ib = packed.info()
        print(f"rows24 sqrt n = {n} start {m_in}: m {ma} / {mb}, matvecs {ia['lanczos_matvecs']} / {ib['lanczos_matvecs']}", flush=True)
        assert ma == mb and ia["lanczos_matvecs"] == ib["lanczos_matvecs"], (n, m_in, ma, mb, ia["lanczos_matvecs"], ib["lanczos_matvecs"])
        assert bool(torch.isfinite(b).all()) and (n == 1 or float(b.abs().max()) > 0.0)
        same(torch, a, b, (n, m_in))
    plain.close(); packed.close()


@pytest.mark.parametrize("n", SIZES)
def test_brownian_velocity_same_bytes(torch_cuda, n):
    """The Brownian call: M psi of iteration 0 comes from the build pass in double4 rows (w_s), every later mat-vec writes packed rows.
    Host-checked once; then queue-only with the gated extras from starting counts below, at and above the converged one -- there
    k_basis_combine takes m and its coefficients from the device-side decision."""
    torch = torch_cuda
    pos, box, _, xi = case(n)
    plain, packed = engines(n, box, xi)
    assert_packed(plain, packed, n)
    dpos, zero = to4(pos), to4(np.zeros((n, 3)))
    a, ma = plain.brownian_velocity_part(dpos, zero, KT, DT, TS, 1)
    ia = plain.info()
    b, mb = packed.brownian_velocity_part(dpos, zero, KT, DT, TS, 1)
    ib = packed.info()
    print(f"rows24 brownian n = {n}: m {ma} / {mb}, matvecs {ia['lanczos_matvecs']} / {ib['lanczos_matvecs']}", flush=True)
    assert ma == mb and ia["lanczos_matvecs"] == ib["lanczos_matvecs"], (n, ma, mb)
    assert float(b.abs().max()) > 0.0
    same(torch, a, b, (n, "host-checked"))
    plain.set_async(True); packed.set_async(True)
    for m_in in (max(1, ma - 2), ma, ma + 2):
        out = []
        for eng in (plain, packed):
            v, _ = eng.brownian_velocity_part(dpos, zero, KT, DT, TS, 1, lanczos_m=m_in)
            torch.cuda.synchronize()
            i = eng.info()
            out.append((v, i["lanczos_m"], i["lanczos_matvecs"], i["lanczos_status"]))
        (a, ma_q, va, sa), (b, mb_q, vb, sb) = out
        print(f"rows24 brownian queued n = {n} start {m_in}: m {ma_q} / {mb_q}, matvecs {va} / {vb}, status {sa} / {sb}", flush=True)
        assert sa == 0 and sb == 0, (n, m_in, sa, sb)
        assert ma_q == mb_q and va == vb, (n, m_in, ma_q, mb_q, va, vb)
        assert m_in != ma or ma_q == ma, (n, ma_q, ma)      # from the converged count the device decides what the host decided
        assert float(b.abs().max()) > 0.0
        same(torch, a, b, (n, "queued", m_in))
    plain.close(); packed.close()


def test_rows_that_overflow_the_pair_list(torch_cuda, oracle):
    """A dense cluster (tests/test_gpu_lanczos_update_sums.py): rows beyond the list capacity walk the cells INSIDE the mat-vec and gather
    their neighbours' rows from the vector itself -- scattered 24-byte rows."""
    torch = torch_cuda
    n, L = 400, 30.0
    rng = np.random.default_rng(17)
    box = (L, L, L, 0.0)
    ball = rng.normal(size=(300, 3))
    ball *= (4.0 * rng.uniform(size=(300, 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    pos = np.concatenate([ball + np.array([L / 2 - 1.0, 0.0, -L / 2 + 0.5]), rng.uniform(-L / 2, L / 2, size=(n - 300, 3))])
    pos = oracle.wrap(pos, np.zeros((n, 3), dtype=np.int64), box)[0]
    psi = rng.normal(size=(n, 3))
    plain, packed = engines(n, box, 0.5)
    assert_packed(plain, packed, n)
    rcut = plain.info()["rcut"]
    d = pos[:, None] - pos[None]
    d -= L * np.rint(d / L)
    cap = (max(16, min(int(np.ceil(1.5 * n / L ** 3 * 4.18879020478639 * rcut ** 3 + 16.0)), 256)) + 3) & ~3   # the pair-list capacity (pse_create)
    assert ((np.linalg.norm(d, axis=2) < rcut).sum(1) - 1).max() > cap
    dpos, dpsi = to4(pos), to4(psi)
    for m_in in (2, 9):
        a, ma = plain.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        b, mb = packed.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        print(f"rows24 overflow rows start {m_in}: m {ma} / {mb}", flush=True)
        assert ma == mb and plain.info()["lanczos_matvecs"] == packed.info()["lanczos_matvecs"]
        same(torch, a, b, ("overflow", m_in))
    zero = to4(np.zeros((n, 3)))
    a, ma = plain.brownian_velocity_part(dpos, zero, KT, DT, TS, 1)
    b, mb = packed.brownian_velocity_part(dpos, zero, KT, DT, TS, 1)
    assert ma == mb
    same(torch, a, b, "overflow, brownian")
    plain.close(); packed.close()


def test_fp64_operator_at_create_keeps_double4(torch_cuda):
    """PSE_LANCZOS_OP=fp64 at create: the fp64 mat-vec gathers its neighbours' rows from the basis as doubles, so the handle keeps the
    double4 layout whatever PSE_ROWS24 says -- the same device_bytes -- and matches itself across the switch."""
    torch = torch_cuda
    n = 257
    pos, box, psi, xi = case(n)
    plain, packed = engines(n, box, xi, PSE_LANCZOS_OP="fp64")
    assert plain.lanczos_operator == packed.lanczos_operator == "fp64"
    assert plain.info()["device_bytes"] == packed.info()["device_bytes"]
    dpos, dpsi = to4(pos), to4(psi)
    for m_in in (2, 12):
        a, ma = plain.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        b, mb = packed.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        assert ma == mb and plain.info()["lanczos_matvecs"] == packed.info()["lanczos_matvecs"]
        same(torch, a, b, ("fp64 at create", m_in))
    plain.close(); packed.close()


@pytest.mark.parametrize("n", [65, 4097])
def test_fp64_operator_selected_later_reads_the_packed_basis(torch_cuda, n):
    """pse_set_lanczos_operator on a handle that was created with the records operator: the layout was decided at create, so the fp64
    mat-vec gathers from 24-byte rows -- told so per launch -- and returns what it returns from double4 rows; back to the records
    operator likewise."""
    torch = torch_cuda
    pos, box, psi, xi = case(n)
    plain, packed = engines(n, box, xi)
    assert_packed(plain, packed, n)
    dpos, dpsi = to4(pos), to4(psi)
    for op in ("fp64", "records16"):
        plain.set_lanczos_operator(op); packed.set_lanczos_operator(op)
        a, ma = plain.sqrt_mreal(dpos, dpsi, tol=TOL)
        b, mb = packed.sqrt_mreal(dpos, dpsi, tol=TOL)
        print(f"rows24 operator {op} n = {n}: m {ma} / {mb}", flush=True)
        assert ma == mb and plain.info()["lanczos_matvecs"] == packed.info()["lanczos_matvecs"]
        same(torch, a, b, (n, op))
    plain.close(); packed.close()
