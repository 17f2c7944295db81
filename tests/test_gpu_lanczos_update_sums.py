"""The one-step Lanczos iteration of a single GPU without a second read of x_{j-1} (pse_vectors.h, launch_lz_update's next_sums;
pse_kernels.h LzFuse.upd): from iteration 1 on the pair-list mat-vec sums x_j.M x_j alone, k_lz_update leaves one pair of partial sums
of x_{j+1}.x_{j+1} and x_{j+1}.x_j per workgroup, and the reduction launch behind the next mat-vec adds them.  What can go wrong is
bookkeeping -- how many partials there are, a scalars-only iteration whose vector part (and with it the sums) follows later, a
launch that met the closed gate of a queue-only call -- so the cases are row counts around the update's workgroup size, starting
counts around the converged one, the queue-only form called repeatedly and a captured call.  Reference: the oracle's Lanczos on its
restatement of the rounded pair-list operator, at the tolerance tests/test_gpu_parity.py and tests/test_reference_lanczos.py hold a
single evaluation from identical positions to: equal m, 1e-9."""
import numpy as np
import pytest

from conftest import make_suspension, to4

pytestmark = pytest.mark.gpu

ERR = 1e-3
TOL = 1e-6        # of the iteration: m = 17 .. 19 at the sizes beyond 1000 particles (printed)
REL = 1e-9        # tests/test_gpu_parity.py test_lanczos_sqrt_matches_dense, a single evaluation from identical positions


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def case(n, seed=0):
    """Positions, box, psi and xi of a row count.  Up to 300 particles: a box of 16 at xi = 0.5 (rcut = 5.26 fits, forty neighbours
    at n = 256).  Beyond: phi = 0.3 at xi = 1 (rcut = 2.63, five neighbours) -- the oracle's mat-vec tests every pair of a block and its
    halo, and its cost goes with rcut^3."""
    pos, _, box = make_suspension(n, L=16.0, seed=12345 + seed) if n <= 300 else make_suspension(n, phi=0.3, seed=12345 + seed)
    psi = np.random.default_rng(1000 + n + seed).normal(size=(n, 3))
    return pos, box, psi, (0.5 if n <= 300 else 1.0)


class Operator:
    """The oracle's near-field mat-vec (all pairs: O(n^2)); beyond 10^3 particles in blocks of the box with their halo of width rcut:
    every row sees all of its neighbours.  About 150 particles per block, blocks no narrower than 2 rcut: fewer pairs tested, and
    not so many calls that their overhead takes over."""

    def __init__(self, oracle, pos, box, xi, rcut, rounded=True):
        self.oracle, self.pos, self.box, self.xi, self.rcut, self.rounded = oracle, pos, box, xi, rcut, rounded
        self.parts = None
        n, L = len(pos), box[0]
        if n > 1000:
            assert box[3] == 0.0 and box[0] == box[1] == box[2]
            blocks = max(1, min(int(L / (2.0 * rcut)), int(round((n / 150.0) ** (1.0 / 3.0)))))
            x = pos + 0.5 * L                                   # [0, L)
            w = L / blocks
            own_of = np.minimum((x / w).astype(int), blocks - 1)
            self.parts = []
            for b in np.ndindex(blocks, blocks, blocks):
                own = np.flatnonzero(np.all(own_of == np.array(b), axis=1))
                t = np.abs(x - (np.array(b) + 0.5) * w)
                t = np.maximum(np.minimum(t, L - t) - 0.5 * w, 0.0)   # distance to the block, per axis, minimum image
                near = np.flatnonzero((t * t).sum(1) < (rcut * 1.0001) ** 2)
                halo = np.setdiff1d(near, own)
                self.parts.append((own, np.concatenate([own, halo])))
            assert sum(len(o) for o, _ in self.parts) == n

    def __call__(self, v):
        v = np.ascontiguousarray(v)
        if self.parts is None:
            return self.oracle.mobility_real(self.pos, v, self.box, self.xi, self.rcut, rounded=self.rounded)
        out = np.empty_like(v)
        for own, sel in self.parts:
            out[own] = self.oracle.mobility_real(self.pos[sel], v[sel], self.box, self.xi, self.rcut, rounded=self.rounded)[:len(own)]
        return out


_REFS = {}


def reference(oracle, key, pos, box, psi, xi, rcut, m_in=2, tol=TOL, rounded=True):
    """(M^{1/2} psi, m) of the oracle, computed once per case and shared."""
    k = (key, m_in, tol, rounded)
    if k not in _REFS:
        _REFS[k] = oracle.lanczos_sqrt(Operator(oracle, pos, box, xi, rcut, rounded), psi, m_in, tol)
    return _REFS[k]


def engine(n, box, xi, **kw):
    import pse_amd
    return pse_amd.Engine(n, box, xi=xi, error=ERR, **kw)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 20000])
def test_row_counts_around_the_update_workgroup(torch_cuda, oracle, n):
    """The update leaves one pair of partials per workgroup of 256 rows: one workgroup, exactly one, two of which the second holds one
    row; 17 and 79 partials, both fewer than the slots."""
    pos, box, psi, xi = case(n)
    eng = engine(n, box, xi)
    out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=TOL)
    up, mp = reference(oracle, n, pos, box, psi, xi, eng.info()["rcut"])
    e = rel(out.cpu().numpy()[:, :3], up)
    print(f"update-sums n = {n}: m {m} / {mp}, rel {e:.2e}", flush=True)
    assert m == mp, (n, m, mp)
    assert e < REL, (n, e)
    eng.close()


N_COUNTS = 4097


def test_starting_counts_run_a_deferred_vector_part(torch_cuda, oracle):
    """From a starting count below the converged one the host-checked driver ends its first batch with a scalars-only iteration, then
    queues that iteration's vector part -- the launch that leaves two sums of the next one -- and a further batch."""
    pos, box, psi, xi = case(N_COUNTS)
    eng = engine(N_COUNTS, box, xi)
    rcut = eng.info()["rcut"]
    _, m_conv = reference(oracle, N_COUNTS, pos, box, psi, xi, rcut)
    assert m_conv >= 12, m_conv
    for m_in in (1, 2, m_conv, m_conv + 3):
        out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=TOL, lanczos_m=m_in)
        up, mp = reference(oracle, N_COUNTS, pos, box, psi, xi, rcut, m_in=m_in)
        e = rel(out.cpu().numpy()[:, :3], up)
        print(f"update-sums start {m_in}: m {m} / {mp}, matvecs {eng.info()['lanczos_matvecs']}, rel {e:.2e}", flush=True)
        assert m == mp and e < REL, (m_in, m, mp, e)
        if m_in < m_conv:
            assert eng.info()["lanczos_matvecs"] > max(m_in, 2)   # a further batch ran
    eng.close()


def test_rows_that_overflow_the_pair_list_take_part(torch_cuda, oracle):
    """A dense cluster: rows beyond the list capacity (count -1) walk the cells inside the mat-vec, which sums x.M x over them like
    over the others."""
    n, L = 400, 30.0
    rng = np.random.default_rng(17)
    box = (L, L, L, 0.0)
    ball = rng.normal(size=(300, 3))
    ball *= (4.0 * rng.uniform(size=(300, 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    pos = np.concatenate([ball + np.array([L / 2 - 1.0, 0.0, -L / 2 + 0.5]), rng.uniform(-L / 2, L / 2, size=(n - 300, 3))])
    pos = oracle.wrap(pos, np.zeros((n, 3), dtype=np.int64), box)[0]
    psi = rng.normal(size=(n, 3))
    xi = 0.5
    eng = engine(n, box, xi)
    rcut = eng.info()["rcut"]
    d = pos[:, None] - pos[None]
    d -= L * np.rint(d / L)
    cap = (max(16, min(int(np.ceil(1.5 * n / L ** 3 * 4.18879020478639 * rcut ** 3 + 16.0)), 256)) + 3) & ~3   # the pair-list capacity (pse_create)
    assert ((np.linalg.norm(d, axis=2) < rcut).sum(1) - 1).max() > cap
    out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=TOL)
    up, mp = reference(oracle, "cluster", pos, box, psi, xi, rcut)
    e = rel(out.cpu().numpy()[:, :3], up)
    print(f"update-sums overflow rows: m {m} / {mp}, rel {e:.2e}", flush=True)
    assert m == mp and e < REL, (m, mp, e)
    eng.close()


def test_queue_only_calls_in_a_row(torch_cuda, oracle):
    """The queue-only form with its gated extras, five calls in a row on one engine from starting counts below, at and above the
    converged one: the launches behind the closed gate write no sums, and what they leave undone does not reach the next call.
    Same m as the host-checked form, status 0."""
    torch = torch_cuda
    pos, box, psi, xi = case(N_COUNTS)
    eng, ref = engine(N_COUNTS, box, xi), engine(N_COUNTS, box, xi)
    eng.set_async(True)
    rcut = eng.info()["rcut"]
    _, m_conv = reference(oracle, N_COUNTS, pos, box, psi, xi, rcut)
    dpos, dpsi = to4(pos), to4(psi)
    for m_in in (m_conv - 2, m_conv, m_conv + 2, m_conv - 1, m_conv):
        out, _ = eng.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        torch.cuda.synchronize()
        i = eng.info()
        _, m_host = ref.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_in)
        up, mp = reference(oracle, N_COUNTS, pos, box, psi, xi, rcut, m_in=m_in)
        e = rel(out.cpu().numpy()[:, :3], up)
        print(f"update-sums queued start {m_in}: m {i['lanczos_m']} / host {m_host} / oracle {mp}, status {i['lanczos_status']}, rel {e:.2e}", flush=True)
        assert i["lanczos_status"] == 0 and i["lanczos_m"] == m_host == mp, (m_in, i["lanczos_m"], m_host, mp, i["lanczos_status"])
        assert e < REL, (m_in, e)
    eng.close(); ref.close()


def test_a_captured_call_replays_on_a_second_configuration(torch_cuda, oracle):
    """One queue-only call captured into a graph: nothing between the launches is host work, so the replay on other positions and
    another psi iterates on its own."""
    torch = torch_cuda
    n = 8257
    pos, box, psi, xi = case(n)
    eng = engine(n, box, xi)
    eng.set_async(True)
    s = torch.cuda.Stream()
    eng.set_stream(s.cuda_stream)
    rcut = eng.info()["rcut"]
    _, m_conv = reference(oracle, n, pos, box, psi, xi, rcut)
    dpos, dpsi = to4(pos), to4(psi)
    with torch.cuda.stream(s):                                 # warm-up outside the capture
        eng.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_conv)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        out, _ = eng.sqrt_mreal(dpos, dpsi, tol=TOL, lanczos_m=m_conv)
    for trial in range(2):
        p, _, q, _ = case(n, seed=trial)
        dpos.copy_(to4(p)); dpsi.copy_(to4(q))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        i = eng.info()
        up, mp = reference(oracle, (n, trial), p, box, q, xi, rcut, m_in=m_conv)
        e = rel(out.cpu().numpy()[:, :3], up)
        print(f"update-sums replay {trial}: m {i['lanczos_m']} / {mp}, status {i['lanczos_status']}, rel {e:.2e}", flush=True)
        assert i["lanczos_status"] == 0 and i["lanczos_m"] == mp, (trial, i["lanczos_m"], mp, i["lanczos_status"])
        assert e < REL, (trial, e)
    eng.close()


def test_fp64_operator(torch_cuda, oracle):
    """The fp64 operator has its own instantiation of the mat-vec that sums x.M x alone: the un-rounded oracle, m for m."""
    n = 4097
    pos, box, psi, xi = case(n)
    eng = engine(n, box, xi, lanczos_operator="fp64")
    assert eng.lanczos_operator == "fp64"
    out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=TOL)
    up, mp = reference(oracle, n, pos, box, psi, xi, eng.info()["rcut"], rounded=False)
    e = rel(out.cpu().numpy()[:, :3], up)
    print(f"update-sums fp64 n = {n}: m {m} / {mp}, rel {e:.2e}", flush=True)
    assert m == mp and e < REL, (m, mp, e)
    eng.close()
