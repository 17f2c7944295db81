"""The references of the Lanczos decision tests (tests/lanczos_decision_ref.py, tests/golden/lanczos_decision.json.gz) and the host twin of
the device-side solver, on the CPU:

- the float64 solvers -- numpy.linalg.eigh and the product's tridiag_eigen (pse_host_lanczos_sqrt_e1), which backs every host-checked
  Brownian call -- against the 40-digit t = T^{1/2} e_1 on every fixture entry: Krylov tridiagonals that have lost orthogonality
  (Ritz values in pairs), Wilkinson matrices, a graded one, one with a negative eigenvalue, sizes up to 98;
- the fixture is what the committed generator computes (small sizes recomputed here), the closed form of TOEP is right;
- every decision case of tests/test_gpu_lanczos_decision.py is decided by the reference alone: the reference walk ends where the case
  intends, the tolerance is 1 % away from every reference step norm, and the largest step-norm error a device within its bound can
  have is a thousandth of that margin."""
import math

import numpy as np
import pytest

import lanczos_decision_ref as R

STORED = [f for f in R.FAMILY_SIZES if f != "TOEP"]


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.mark.parametrize("fam", list(R.FAMILY_SIZES))
def test_float64_solvers_are_within_32_yardsticks_of_the_multiprecision_square_root(fx, fam):
    """numpy.linalg.eigh now and pse_host_lanczos_sqrt_e1 within 32 e' of t_ref, e' = max(e_numpy as stored, u |t_ref|_2): the host
    solver is measured against the independent LAPACK result, not against itself."""
    import pse_amd
    worst = {"numpy": (0.0, 0), "host": (0.0, 0)}
    for m in R.FAMILY_SIZES[fam]:
        a, b = fx.coeffs(fam, m)
        t_ref = fx.t_ref(fam, m)
        e1 = max(fx.info(fam, m)["e_numpy"], R.U * R.norm2(t_ref))
        for name, t in (("numpy", R.t_numpy(a, b, m)), ("host", pse_amd.host_lanczos_sqrt_e1(a, b))):
            ratio = R.max_abs_err(t, t_ref) / e1
            worst[name] = max(worst[name], (ratio, m))
    print(f"{fam}: worst error in units of e': numpy {worst['numpy'][0]:.2f} at m = {worst['numpy'][1]}, "
          f"host {worst['host'][0]:.2f} at m = {worst['host'][1]}")
    assert worst["numpy"][0] <= R.FACTOR and worst["host"][0] <= R.FACTOR, worst


def test_the_families_have_the_properties_they_are_there_for(fx):
    i = fx.info("K3", 98)
    assert i["gap_min"] < 1e-12 and i["lam_min"] > 0            # orthogonality lost: Ritz values in pairs
    assert fx.info("WILK", 98)["gap_min"] < 1e-14
    assert fx.info("GRAD", 98)["lam_min"] < 1e-11
    for m in R.FAMILY_SIZES["NEG"]:
        assert fx.info("NEG", m)["lam_min"] < -0.1                # the clamp max(lambda, 0) acts


@pytest.mark.parametrize("fam", STORED)
def test_fixture_is_what_the_committed_generator_computes(fx, fam):
    """Small sizes recomputed with mpmath now: the stored coefficients bit for bit, the stored t to 1e-30."""
    import mpmath as mp
    small = [m for m in R.FAMILY_SIZES[fam] if m <= 12]
    sizes = small if len(small) <= 3 else [small[2], small[6], small[11]]
    assert sizes
    for m in sizes:
        a, b = R.family(fam, m)
        fa, fb = fx.coeffs(fam, m)
        assert np.array_equal(a, fa) and np.array_equal(b[1:], fb[1:]), (fam, m)
        t, lam = R.t_ref_mp(a, b, m)
        with mp.workdps(R.DPS):
            assert max(abs(x - y) for x, y in zip(t, fx.t_ref(fam, m))) < mp.mpf("1e-30"), (fam, m)
        assert float(lam[0]) == fx.info(fam, m)["lam_min"]


@pytest.mark.parametrize("m", [7, 33])
def test_toeplitz_closed_form_matches_eigsy(m):
    import mpmath as mp
    a, b = R.family("TOEP", m)
    t, _ = R.t_ref_mp(a, b, m)
    with mp.workdps(R.DPS):
        assert max(abs(x - y) for x, y in zip(t, R.toeplitz_t_ref(m))) < mp.mpf("1e-35")


def test_the_reference_walk_on_two_by_two_matrices_by_hand():
    """T_1 = (a0), T_2 = [[a0, b1], [b1, a1]] with the square root of a 2 x 2 matrix in closed form: (T + sqrt(det) I) / sqrt(tr + 2 sqrt(det))."""
    a0, a1, b1 = 2.0, 3.0, 0.5
    s = math.sqrt(a0 * a1 - b1 * b1)
    t2 = [(a0 + s) / math.sqrt(a0 + a1 + 2 * s), b1 / math.sqrt(a0 + a1 + 2 * s)]
    t_of = {1: [math.sqrt(a0)], 2: t2}.__getitem__
    alpha, beta = np.array([a0, a1]), np.array([0.0, b1, 0.7])
    step = math.sqrt(((t2[0] - math.sqrt(a0)) ** 2 + t2[1] ** 2) / a0)
    mirror = dict(m=0.0, stepnorm=0.0, status=0.0, seq=0.0, open=2.0)
    for tol, status, want_open in ((step * 1.5, 0, 2.0), (step / 1.5, 1, 3.0)):
        st, mr = R.walk(dict(m_lo=1, m_hi=2, done_iters=2, first=1, last=1, tol=tol, seq=9.0), alpha, beta, 4.0, None, mirror, t_of)
        assert (st["done"], st["m_final"], st["status"], st["checked"]) == (1, 2, status, 1 if status == 0 else 2)
        assert abs(float(st["stepnorm"]) - step) < 1e-15
        assert abs(float(st["coef"][0]) - t2[0] / 4.0) < 1e-15 and abs(float(st["coef"][1]) - t2[1] / b1) < 1e-15
        assert mr == dict(m=2.0, stepnorm=st["stepnorm"], status=float(status), seq=9.0, open=want_open)
    st2, mr2 = R.walk(dict(m_lo=2, m_hi=2, done_iters=2, first=0, last=1, tol=0.0), alpha, beta, 4.0, st, mr, t_of)
    assert st2 is st and mr2 is mr                                  # done: a later decision leaves everything as it is


def case_ids():
    return [c["name"] for c in R.fixture().cases]


@pytest.mark.parametrize("name", case_ids())
def test_decision_cases_are_decided_by_the_reference_alone(fx, name):
    case = next(c for c in fx.cases if c["name"] == name)
    fam = case["family"]
    ref = fx.case_reference(case)
    got = [[st["done"], st["m_final"], st["status"]] for st, _ in ref]
    assert got == case["intent"], (name, got)
    sizes = list(case["fail"]) + ([case["pass"]] if case["pass"] else [])
    if not sizes:
        return
    tols = {d["tol"] for d in case["decisions"]}
    assert len(tols) == 1
    tol = tols.pop()
    margin = math.inf
    for m in case["fail"]:
        s = fx.stepnorm_ref(fam, m)
        assert s >= 1.01 * tol, (name, m, s, tol)
        margin = min(margin, s - tol)
    if case["pass"]:
        s = fx.stepnorm_ref(fam, case["pass"])
        assert s <= tol / 1.01, (name, case["pass"], s, tol)
        margin = min(margin, tol - s)
    a, _ = fx.coeffs(fam, 1)
    bound = max(R.stepnorm_bound(m, max(fx.e_ref(fam, m), fx.e_ref(fam, m - 1)), a[0]) for m in sizes)
    print(f"{name}: tol {tol:.4e} margin {margin:.3e} bound on the device's step-norm error {bound:.3e}")
    assert bound <= 1e-3 * margin, (name, bound, margin)
