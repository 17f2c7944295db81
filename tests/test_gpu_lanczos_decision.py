"""The device-side Lanczos decision (k_lz_decide, lz_sqrt_e1 in pse_vectors.hip) by itself, on given coefficients, at every size it
supports (pse_debug_lz_decide): the square root t = T^{1/2} e_1 of one wavefront against 40-digit references on Krylov, Toeplitz,
Wilkinson, graded and indefinite tridiagonals (tests/lanczos_decision_ref.py, tests/golden/lanczos_decision.json.gz), and the walk --
the sequences of decisions lanczos_queued and lanczos_local issue -- against the reference walk after every launch, by the checker
that tests/test_lanczos_decision_cpu.py holds the host drivers' twin to (R.run_case).

Above m = 64 entries 64 .. of d and e live in a second register, every lane owns two eigenvector rows, and from the pair (55, 56) on
the dynamic LDS passes 48 KB: none of that ran in the suite before (its largest device-side decision was at m = 20).

Yardstick: e_ref = max(error of numpy.linalg.eigh, error of the host twin, u |t|_2) per (family, size); the device may be 32 e_ref
off (tests/test_lanczos_decision_cpu.py shows that the tolerances of the walk cases leave 1000 times that)."""
import numpy as np
import pytest

import lanczos_decision_ref as R
from conftest import make_suspension, to4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def sqrt_single(fx, fam, m, poison=True):
    """One decision that ends at size m with status 1 (tol = 0, last): t_prev is the kernel's t."""
    import pse_amd
    a, b = fx.coeffs(fam, m)
    dec = [dict(m_lo=m, m_hi=m, done_iters=m, first=1, last=1, tol=0.0, m_max=100, seq=1.0)]
    o, = pse_amd.debug_lz_decide(R.scal_image(a, b, 1.0, dec, poison=poison), dec)
    assert (o["done"], o["m_final"], o["checked"], o["status"]) == (1, m, m, 1), (fam, m, o["done"], o["m_final"], o["checked"], o["status"])
    assert np.isnan(o["t_prev"][m:]).all() and np.isnan(o["coef"][m:]).all()
    return o


@pytest.mark.parametrize("fam", list(R.FAMILY_SIZES))
def test_square_root_of_one_wavefront_against_40_digits(fx, fam):
    worst = {False: (0.0, 0), True: (0.0, 0)}
    for m in R.FAMILY_SIZES[fam]:
        o = sqrt_single(fx, fam, m)
        t_ref, e = fx.t_ref(fam, m), fx.e_ref(fam, m)
        ratio = R.max_abs_err(o["t_prev"][:m], t_ref) / e
        worst[m > 64] = max(worst[m > 64], (ratio, m))
        _, b = fx.coeffs(fam, m)
        back = o["coef"][:m] * np.concatenate([[1.0], b[1:m]])       # the coefficients are t / norm, then / beta_q
        assert R.max_abs_err(back, t_ref) <= R.FACTOR * e, (fam, m)
    print(f"{fam}: worst |t - t_ref| in units of e_ref: {worst[False][0]:.2f} at m = {worst[False][1]} (m <= 64), "
          f"{worst[True][0]:.2f} at m = {worst[True][1]} (m > 64)")
    assert max(worst[False][0], worst[True][0]) <= R.FACTOR, worst


def test_square_roots_of_both_wavefronts_at_every_pair_of_sizes(fx):
    """K3, the pair (m - 1, m) for m = 2 .. 98: wavefront 1 solves size m behind the LDS offset m_lo^2.  Call 1 (tol = 0) leaves size
    m in t_prev; call 2 (m_max = m) ends at m with status 0 and the coefficients of wavefront 1's t."""
    import pse_amd
    a, b = fx.coeffs("K3", R.M_SUPPORTED)
    worst = {False: (0.0, 0), True: (0.0, 0)}
    for m in range(2, R.M_SUPPORTED + 1):
        d1 = dict(m_lo=m - 1, m_hi=m, done_iters=m, first=1, last=0, tol=0.0, m_max=100, seq=1.0)
        d2 = dict(d1, m_max=m)
        scal = R.scal_image(a, b, 1.0, [d1])
        (o1,), (o2,) = pse_amd.debug_lz_decide(scal, [d1]), pse_amd.debug_lz_decide(scal, [d2])
        assert (o1["done"], o1["checked"]) == (0, m) and (o2["done"], o2["m_final"], o2["status"], o2["checked"]) == (1, m, 0, m - 1), m
        t_ref, e = fx.t_ref("K3", m), fx.e_ref("K3", m)
        assert np.array_equal(o2["t_prev"][:m - 1], sqrt_single(fx, "K3", m - 1)["t_prev"][:m - 1]), m      # wavefront 0: as when alone
        back = o2["coef"][:m] * np.concatenate([[1.0], b[1:m]])
        for t in (o1["t_prev"][:m], back):
            ratio = R.max_abs_err(t, t_ref) / e
            worst[m > 64] = max(worst[m > 64], (ratio, m))
        s_ref = fx.stepnorm_ref("K3", m)
        bound = R.stepnorm_bound(m, max(e, fx.e_ref("K3", m - 1)), a[0])
        assert abs(o1["stepnorm"] - s_ref) <= bound and abs(o2["stepnorm"] - s_ref) <= bound, (m, o1["stepnorm"], s_ref, bound)
    print(f"K3 pairs: worst |t - t_ref| in units of e_ref: {worst[False][0]:.2f} at m = {worst[False][1]} (m <= 64), "
          f"{worst[True][0]:.2f} at m = {worst[True][1]} (m > 64)")
    assert max(worst[False][0], worst[True][0]) <= R.FACTOR, worst


@pytest.mark.parametrize("m", [1, 2, 7, 64, 65, 98])
def test_entries_the_decision_has_no_right_to_read_do_not_matter(fx, m):
    """alpha[q >= done_iters], beta[q > done_iters], beta[done_iters] without have_last_beta, beta[0] and every other slot: NaN in all
    the other tests; here against the full coefficient arrays in a zeroed image."""
    assert R.bits(sqrt_single(fx, "K3", m, poison=True)) == R.bits(sqrt_single(fx, "K3", m, poison=False))


def run_case(fx, case, open0=None):
    import pse_amd
    return R.run_case(fx, case, pse_amd.debug_lz_decide, open0)


def case_ids():
    return [c["name"] for c in R.fixture().cases]


@pytest.mark.parametrize("name", case_ids())
def test_walk_follows_the_reference_after_every_launch(fx, name):
    run_case(fx, next(c for c in fx.cases if c["name"] == name))


def test_open_calls_are_counted_from_the_value_the_mirror_holds(fx):
    """Status 2 (a NaN alpha inside the first size) twice: the second sequence starts from the count the first one left."""
    case = next(c for c in fx.cases if c["name"] == "nan_alpha_first_size")
    out = run_case(fx, case)
    assert out[-1]["mirror"]["open"] == case["open0"] + 1 and out[-1]["status"] == 2 and out[-1]["m_final"] == 1
    out2 = run_case(fx, case, open0=out[-1]["mirror"]["open"])
    assert out2[-1]["mirror"]["open"] == case["open0"] + 2


def test_dead_norm_reads_no_coefficient(fx):
    for name in ("norm_zero", "norm_nan"):
        o, = run_case(fx, next(c for c in fx.cases if c["name"] == name))
        assert (o["done"], o["m_final"], o["status"], o["checked"], o["stepnorm"]) == (1, 0, 0, 0, 1.0)
        assert np.isnan(o["coef"]).all() and o["mirror"]["m"] == 0.0


def test_supported_sizes_and_refusals():
    """1 .. 98 fit (97^2 + 98^2 doubles <= 150 KB); the entry point refuses, before any launch, whatever the kernel was not sized for."""
    import pse_amd
    sup = [m for m in range(-1, 130) if pse_amd.debug_lz_decide_supported(m)]
    assert sup == list(range(1, 99))
    good = dict(m_lo=5, m_hi=6, done_iters=6, first=1, last=1, tol=0.0, m_max=100, seq=1.0)
    scal = np.zeros(R.LZ_NSCAL)
    scal[:6] = 1.0; scal[R.LZ_BETA + 1:R.LZ_BETA + 6] = 0.1; scal[R.LZ_NORM] = 1.0
    assert pse_amd.debug_lz_decide(scal, [good])[0]["m_final"] == 6
    bad = [dict(good, m_hi=99, m_lo=98, done_iters=99), dict(good, m_hi=100, m_lo=100, done_iters=100), dict(good, m_hi=0, m_lo=0),
           dict(good, m_hi=1 << 20, m_lo=1 << 20, done_iters=1 << 20), dict(good, m_hi=-3, m_lo=-3),
           dict(good, m_lo=4), dict(good, m_lo=7), dict(good, m_lo=0, m_hi=1), dict(good, done_iters=5), dict(good, done_iters=101),
           dict(good, m_max=101), dict(good, first=0), dict(good, pending_beta=7), dict(good, pending_beta=-1)]
    for d in bad:
        with pytest.raises(pse_amd.PSEError):
            pse_amd.debug_lz_decide(scal, [d])
        with pytest.raises(pse_amd.PSEError):                        # ... wherever in the sequence it stands
            pse_amd.debug_lz_decide(scal, [good, dict(d, first=0)] if d.get("first", 1) else [d, good])
    with pytest.raises(pse_amd.PSEError):
        pse_amd.debug_lz_decide(scal, [])
    with pytest.raises(pse_amd.PSEError):
        pse_amd.debug_lz_decide(scal, [good] + [dict(good, first=0)] * 40)
    with pytest.raises(ValueError):
        pse_amd.debug_lz_decide(scal[:300], [good])


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_queue_only_brownian_calls_from_starting_counts_of_64_to_98():
    """End to end above the sizes the rest of the suite reaches (tests/test_gpu_async.py: 6 - 8): the queue-only call takes the
    device-side decision at the pairs (63, 64) .. (97, 98) -- same m, same velocities as the host-checked driver from the same
    starting count.  Counts whose extras would pass 98 take the host-driven path: 97 with the default two extras (99 mat-vecs
    would tell), 100 always."""
    import torch
    import pse_amd
    n = 3000
    pos, force, box = make_suspension(n, phi=0.15)
    kw = dict(xi=0.5, error=1e-3, seed=11)
    ref = pse_amd.Engine(n, box, **kw)
    eng = pse_amd.Engine(n, box, **kw)
    eng.set_async(True)
    dpos, dF = to4(pos), to4(force)
    for m_in, extra, on_device in ((64, None, True), (65, None, True), (66, None, True), (96, None, True), (98, 0, True),
                                   (97, None, False), (100, None, False)):
        eng.set_lanczos_extra(-1 if extra is None else extra)
        vel, _ = eng.brownian_velocity(dpos, dF, 1.0, 1e-3, 5, lanczos_m=m_in)
        torch.cuda.synchronize()
        i = eng.info()
        u2, m2 = ref.brownian_velocity(dpos, dF, 1.0, 1e-3, 5, lanczos_m=m_in)
        assert i["lanczos_status"] == 0 and i["lanczos_m"] == m2, (m_in, i["lanczos_m"], m2, i["lanczos_status"])
        err = rel(vel.cpu().numpy()[:, :3], u2.cpu().numpy()[:, :3])
        print(f"m_in = {m_in}: m = {m2}, |u - u_host| / |u_host| = {err:.2e}, mat-vecs {i['lanczos_matvecs']}")
        assert err < 1e-12, (m_in, err)
        if on_device:
            assert pse_amd.debug_lz_decide_supported(m_in + (2 if extra is None else extra))
            assert i["lanczos_matvecs"] == m_in + (2 if extra is None else extra), (m_in, i["lanczos_matvecs"])   # the gated extras were queued
        else:                                                        # the fallback: the host walked, nothing beyond m_in was queued
            assert not pse_amd.debug_lz_decide_supported(min(100, m_in + 2))
            assert i["lanczos_matvecs"] == m_in, (m_in, i["lanczos_matvecs"])
    assert i["lanczos_open_calls"] == 0
