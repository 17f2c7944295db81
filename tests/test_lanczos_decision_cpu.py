"""The references of the Lanczos decision tests (tests/lanczos_decision_ref.py, tests/golden/lanczos_decision.json.gz) and the host twin of
the device-side solver, on the CPU:

- the float64 solvers -- numpy.linalg.eigh and the product's tridiag_eigen (pse_host_lanczos_sqrt_e1), which backs every host-checked
  Brownian call -- against the 40-digit t = T^{1/2} e_1 on every fixture entry: Krylov tridiagonals that have lost orthogonality
  (Ritz values in pairs), Wilkinson matrices, a graded one, one with a negative eigenvalue, sizes up to 98;
- the fixture is what the committed generator computes (small sizes recomputed here), the closed form of TOEP is right;
- every decision case of tests/test_gpu_lanczos_decision.py is decided by the reference alone: the reference walk ends where the case
  intends, the tolerance is 1 % away from every reference step norm, and the largest step-norm error a device within its bound can
  have is a thousandth of that margin;
- the host twin of the device-side decision (lz_decide_host through pse_host_lz_decide), which ends the iteration of every host-checked
  Brownian call, against the reference walk after every decision: the 30 cases the device is held to, by the same checker
  (R.run_case), and four sequences as the host drivers issue them (R.host_decisions), whose later batches check three to six sizes."""
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


def two_by_two():
    """T_1 = (a0), T_2 = [[a0, b1], [b1, a1]] with the square root of a 2 x 2 matrix in closed form: (T + sqrt(det) I) / sqrt(tr + 2 sqrt(det))."""
    a0, a1, b1 = 2.0, 3.0, 0.5
    s = math.sqrt(a0 * a1 - b1 * b1)
    t2 = [(a0 + s) / math.sqrt(a0 + a1 + 2 * s), b1 / math.sqrt(a0 + a1 + 2 * s)]
    step = math.sqrt(((t2[0] - math.sqrt(a0)) ** 2 + t2[1] ** 2) / a0)
    return a0, b1, t2, step, np.array([a0, a1]), np.array([0.0, b1, 0.7])


def test_the_reference_walk_on_two_by_two_matrices_by_hand():
    a0, b1, t2, step, alpha, beta = two_by_two()
    t_of = {1: [math.sqrt(a0)], 2: t2}.__getitem__
    mirror = dict(m=0.0, stepnorm=0.0, status=0.0, seq=0.0, open=2.0)
    for tol, status, want_open in ((step * 1.5, 0, 2.0), (step / 1.5, 1, 3.0)):
        st, mr = R.walk(dict(m_lo=1, m_hi=2, done_iters=2, first=1, last=1, tol=tol, seq=9.0), alpha, beta, 4.0, None, mirror, t_of)
        assert (st["done"], st["m_final"], st["status"], st["checked"]) == (1, 2, status, 1 if status == 0 else 2)
        assert abs(float(st["stepnorm"]) - step) < 1e-15
        assert abs(float(st["coef"][0]) - t2[0] / 4.0) < 1e-15 and abs(float(st["coef"][1]) - t2[1] / b1) < 1e-15
        assert mr == dict(m=2.0, stepnorm=st["stepnorm"], status=float(status), seq=9.0, open=want_open)
    st2, mr2 = R.walk(dict(m_lo=2, m_hi=2, done_iters=2, first=0, last=1, tol=0.0), alpha, beta, 4.0, st, mr, t_of)
    assert st2 is st and mr2 is mr                                  # done: a later decision leaves everything as it is


def test_the_host_decision_on_two_by_two_matrices_by_hand():
    """The same by the host twin.  Its t are float64 results of tridiag_eigen: each entry within FACTOR u |t|_2 of the closed form
    (the yardstick of every other test here); the step norm within R.stepnorm_bound of that error."""
    import pse_amd
    a0, b1, t2, step, alpha, beta = two_by_two()
    e = R.U * math.hypot(*t2)
    scal = np.full(R.LZ_NSCAL, np.nan)
    scal[R.LZ_ALPHA:R.LZ_ALPHA + 2], scal[R.LZ_BETA + 1:R.LZ_BETA + 3], scal[R.LZ_NORM] = alpha, beta[1:], 4.0
    for tol, status, want_open in ((step * 1.5, 0, 2.0), (step / 1.5, 1, 3.0)):
        first = dict(m_lo=1, m_hi=2, done_iters=2, first=1, last=1, tol=tol, seq=9.0, m_max=100)
        o, o2 = pse_amd.host_lz_decide(scal, [first, dict(first, m_lo=2, first=0, tol=0.0)], 2.0)
        assert (o["done"], o["m_final"], o["status"], o["checked"]) == (1, 2, status, 1 if status == 0 else 2)
        assert abs(o["stepnorm"] - step) <= R.stepnorm_bound(2, e, a0)
        assert abs(o["coef"][0] - t2[0] / 4.0) <= R.FACTOR * e / 4.0 and abs(o["coef"][1] - t2[1] / b1) <= R.FACTOR * e / b1
        assert np.isnan(o["coef"][2:]).all() and np.isnan(o["t_prev"][o["checked"]:]).all()
        assert o["mirror"] == dict(m=2.0, stepnorm=o["stepnorm"], status=float(status), seq=9.0, open=want_open)
        assert R.bits(o2) == R.bits(o)                              # done: a later decision leaves everything as it is


def test_the_host_decision_refuses_what_would_index_outside_its_arrays():
    """The twin indexes alpha[m - 1], beta[m], beta[pending_beta] and t_prev[] by these fields; pse_host_lz_decide refuses, before
    any decision is taken, whatever lies outside 1 <= m_lo <= m_hi <= done_iters <= 100, wherever in the sequence it stands.  What
    only the device refuses is taken: any number of sizes, and sizes above 98."""
    import pse_amd
    good = dict(m_lo=5, m_hi=6, done_iters=6, first=1, last=1, tol=0.0, m_max=100, seq=1.0)
    scal = np.zeros(R.LZ_NSCAL)
    scal[:100] = 1.0; scal[R.LZ_BETA + 1:R.LZ_BETA + 101] = 0.1; scal[R.LZ_NORM] = 1.0
    assert pse_amd.host_lz_decide(scal, [good])[0]["m_final"] == 6
    assert pse_amd.host_lz_decide(scal, [dict(good, m_lo=1)])[0]["m_final"] == 6
    assert pse_amd.host_lz_decide(scal, [dict(good, m_lo=99, m_hi=100, done_iters=100)])[0]["m_final"] == 100
    assert pse_amd.host_lz_decide(scal, [good] + [dict(good, first=0)] * 39)[-1]["m_final"] == 6
    bad = [dict(good, m_lo=0), dict(good, m_lo=-3), dict(good, m_lo=7), dict(good, m_hi=0, m_lo=0), dict(good, m_hi=-3, m_lo=-3),
           dict(good, done_iters=5), dict(good, m_hi=101, m_lo=101, done_iters=101), dict(good, done_iters=101),
           dict(good, m_hi=1 << 20, m_lo=1 << 20, done_iters=1 << 20), dict(good, pending_beta=7), dict(good, pending_beta=-1),
           dict(good, m_max=101), dict(good, first=0)]
    for d in bad:
        with pytest.raises(pse_amd.PSEError, match="pse_host_lz_decide"):
            pse_amd.host_lz_decide(scal, [d])
        with pytest.raises(pse_amd.PSEError, match="pse_host_lz_decide"):
            pse_amd.host_lz_decide(scal, [good, dict(d, first=0)] if d.get("first", 1) else [d, good])
    with pytest.raises(pse_amd.PSEError, match="m_lo = 7 outside"):
        pse_amd.host_lz_decide(scal, [dict(good, m_lo=7)])
    with pytest.raises(pse_amd.PSEError):
        pse_amd.host_lz_decide(scal, [])
    with pytest.raises(pse_amd.PSEError):
        pse_amd.host_lz_decide(scal, [good] + [dict(good, first=0)] * 40)
    with pytest.raises(ValueError):
        pse_amd.host_lz_decide(scal[:300], [good])


def case_ids():
    return [c["name"] for c in R.fixture().cases]


def decided_by_the_reference_alone(fx, case):
    name, fam = case["name"], case["family"]
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


@pytest.mark.parametrize("name", case_ids())
def test_decision_cases_are_decided_by_the_reference_alone(fx, name):
    decided_by_the_reference_alone(fx, next(c for c in fx.cases if c["name"] == name))


@pytest.mark.parametrize("name", case_ids())
def test_host_walk_follows_the_reference_after_every_decision(fx, name):
    """The 30 cases of the device, through the host twin: pending-beta breakdown, breakdown inside a batch, NaN alpha, infinite last
    beta, dead norm, the end on m_max -- none of which an end-to-end Brownian call produces."""
    import pse_amd
    R.run_case(fx, next(c for c in fx.cases if c["name"] == name), pse_amd.host_lz_decide)


def host_driver_cases():
    """Sequences as lanczos and lanczos_team issue them, on K3 (a reference t at every size): the later batches check 3 - 6 sizes in
    one decision, which no case of the device can.  fail / pass: the sizes whose step norm the walk compares with tol, as in the
    fixture.  K3 step norms: m = 12, 13, 14 -> 2.651e-3, 2.581e-3, 1.974e-3; m = 22, 23 -> 4.774e-4, 4.119e-4."""
    def case(name, m_in, batches, two_step, tol, end, fail, ok, m_max=100):
        dec = R.host_decisions(m_in, batches, two_step, tol, m_max=m_max)
        return dict(name=name, family="K3", norm=float(1.5).hex(), patches=[], open0=0.0, decisions=dec,
                    intent=[[0, 0, 0]] * (batches - 1) + [[1, end, 0]], fail=list(fail), **{"pass": ok})
    return [case("host_one_step_m2_ends_inside_a_batch_of_three", 2, 7, False, 2.257e-3, 14, range(2, 14), 14),
            case("host_two_step_m2_ends_inside_a_batch_of_three", 2, 7, True, 2.257e-3, 14, range(2, 14), 14),
            case("host_one_step_m20_ends_inside_a_batch_of_five", 20, 2, False, 4.434e-4, 23, range(20, 23), 23),
            case("host_one_step_m24_ends_on_m_max_30", 24, 2, False, 0.0, 30, range(24, 31), 0, m_max=30)]


@pytest.mark.parametrize("case", host_driver_cases(), ids=lambda c: c["name"])
def test_host_walk_on_the_batches_the_host_drivers_issue(fx, case):
    import pse_amd
    sizes = [(d["m_lo"], d["m_hi"]) for d in case["decisions"]]
    if case["name"].endswith("of_three"):
        assert sizes == [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 15)]
        assert [d.get("pending_beta", 0) for d in case["decisions"]] == ([0] * 7 if "two_step" in case["name"] else [0, 2, 4, 6, 8, 10, 12])
    elif case["name"].endswith("of_five"):
        assert sizes == [(19, 20), (21, 25)] and case["decisions"][1]["pending_beta"] == 20
    else:
        assert sizes == [(23, 24), (25, 30)]
    decided_by_the_reference_alone(fx, case)
    out = R.run_case(fx, case, pse_amd.host_lz_decide)
    assert out[-1]["m_final"] == case["intent"][-1][1] and out[-1]["status"] == 0
