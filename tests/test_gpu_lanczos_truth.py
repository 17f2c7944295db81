"""The device's M_real^{1/2} psi against the TRUE near-field operator: the dense un-rounded M_real (oracle, rounded=False) and its
square root by eigendecomposition, not the restatement of the 16-byte pair records.  The difference may be what the records' rounding
allows (tests/record_bound.py: a bound from the un-rounded f, g and the record format alone) plus the Lanczos tolerance -- at the
placements where a packing goes wrong: pairs along one axis, one component 1e-9 .. 1e-4 of the others, overlapping and touching pairs,
pairs just inside rcut, images through the tilted box, xi from 0.2 to 10, and h = (g - f) / r^2 < 0 (record_bound.geometries).
Whether the bound itself stays below 1e-6 is a property of the geometry, not of the device: tests/test_record_bound.py states it."""
import numpy as np
import pytest

from conftest import to4
import record_bound as rb

pytestmark = pytest.mark.gpu

GEOS = {g["name"]: g for g in rb.geometries()}
M_MAX = 100   # the device's Lanczos basis cap (pse_capi.hip M_MAX)
# Measured on an MI355X (relative error of the device against M^{1/2} psi of the un-rounded operator | the bound + tol it is held to):
#   a 3.1e-8 | 5.8e-7   b 3.4e-8 | 4.4e-7   c (r = 1e-3 .. 2, tol 1e-9, m = 95) 2.7e-7 | 1.3e-5   c (touching) 4.1e-8 | 5.7e-7
#   d 3.1e-8 | 4.9e-8   e (+0.5) 8.2e-8 | 2.7e-6   e (-0.5) 3.9e-8 | 5.2e-7   e (suspension) 1.2e-7 | 2.9e-6
#   f: xi = 0.2 6.0e-8 | 1.6e-6   0.5 1.0e-7 | 2.7e-6   1.0 8.7e-8 | 1.1e-6   2.0 7.2e-8 | 7.3e-7   10 7.0e-7 | 1.7e-6
#   g (pairs) 1.4e-7 | 4.5e-7   g (suspension) 1.5e-7 | 9.0e-7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.mark.parametrize("name", list(GEOS))
def test_sqrt_mreal_against_the_unrounded_operator(torch_cuda, oracle, name):
    import pse_amd
    g = GEOS[name]
    pos, box, xi = g["pos"], g["box"], g["xi"]
    n = len(pos)
    psi = np.random.default_rng(n).normal(size=(n, 3))
    eng = pse_amd.Engine(n, box, xi=xi, error=g["error"])
    assert abs(eng.info()["rcut"] - g["rcut"]) < 1e-12
    t = rb.truth(oracle, pos, box, xi, g["rcut"], psi, extra_pair=rb.table(xi, g["rcut"]), vector_rows=True)
    # tol = 1e-10 where the iteration converges within the basis cap; otherwise the smallest tolerance that does, added to the bound
    for tol in (1e-10, 1e-9, 1e-8):
        out, m = eng.sqrt_mreal(to4(pos), to4(psi), tol=tol)
        if m < M_MAX and eng.info()["lanczos_stepnorm"] <= tol:
            break
    else:
        pytest.fail(f"{name}: no convergence at tol = 1e-8 (m = {m})")
    err = np.linalg.norm(out.cpu().numpy()[:, :3] - t["ref"]) / np.linalg.norm(t["ref"])
    print(f"{name}: m = {m}, tol = {tol:g}, |device - M^1/2 psi| / |M^1/2 psi| = {err:.3e}, bound {t['rel']:.3e} + tol")
    assert err <= t["rel"] + tol, (name, m, tol, err, t["rel"])
    eng.close()
