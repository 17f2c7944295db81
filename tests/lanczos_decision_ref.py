"""Reference of the Lanczos decision (k_lz_decide / lz_sqrt_e1 in pse_vectors.hip, tridiag_eigen / lanczos_sqrt_e1 in pse_params.cpp):
the families of tridiagonals the tests use, t = T^{1/2} e_1 in multiprecision, and the convergence walk of the drivers as a plain
function.  tests/golden/make_lanczos_decision_fixture.py computes the multiprecision results ONCE with the functions of this module and
stores them in tests/golden/lanczos_decision.json.gz; the tests read them back through Fixture.

Conventions (pse_vectors.h): the tridiagonal of size m is T(alpha[0..m), beta[1..m)); beta[0] is unused; beta[m] = |x_m| is the
coefficient that arrives one iteration later.  A family gives alpha[0..m) and beta[0..m]."""
import functools
import gzip
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_PATH = os.path.join(HERE, "golden", "lanczos_decision.json.gz")

U = 2.0 ** -53
DPS = 40                     # digits of the stored references (the generator checks them against 50 digits)
FACTOR = 32.0                # what this project allows over a float64 yardstick (tests/wave_grid_ref.py)
M_SUPPORTED = 98             # largest size of the device-side decision: 97^2 + 98^2 doubles fit 150 KB of LDS, 98^2 + 99^2 do not
LZ_ALPHA, LZ_BETA, LZ_NORM, LZ_NSCAL = 0, 128, 256, 400
MIRROR_FIELDS = ("m", "stepnorm", "status", "seq", "open")
BREAKDOWN = 1e-8             # PSEv1/Brownian.cu:503
# the lane and register boundary at entry 64, the first pair of sizes above 48 KB of LDS (55, 56), the largest supported pair
B_SIZES = (1, 2, 3, 55, 56, 63, 64, 65, 66, 97, 98)
ALL_SIZES = tuple(range(1, M_SUPPORTED + 1))
FAMILY_SIZES = {"K3": ALL_SIZES, "K6": B_SIZES, "TOEP": ALL_SIZES, "WILK": B_SIZES, "GRAD": B_SIZES, "NEG": (5, 65, 98)}
SHARED = ("K3", "K6")        # one alpha / beta pair for all sizes


# ---- the families ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _krylov(lo):
    """float64 Lanczos without reorthogonalisation on diag(geomspace(lo, 1, 400)), 98 iterations.  Sums by math.fsum (correctly rounded),
    so the coefficients do not depend on how a BLAS orders a dot product."""
    D = np.geomspace(lo, 1.0, 400)
    v = np.random.default_rng(1).standard_normal(400)
    v = v / math.sqrt(math.fsum(v * v))
    vp = np.zeros(400)
    alpha, beta = np.zeros(M_SUPPORTED), np.zeros(M_SUPPORTED + 1)
    for j in range(M_SUPPORTED):
        w = D * v
        alpha[j] = math.fsum(v * w)
        w = w - alpha[j] * v - beta[j] * vp
        beta[j + 1] = math.sqrt(math.fsum(w * w))
        vp, v = v, w / beta[j + 1]
    return alpha, beta


def family(name, m):
    """alpha[0..m), beta[0..m] (beta[0] = 0) of the family at size m."""
    if name in ("K3", "K6"):
        a, b = _krylov(1e-3 if name == "K3" else 1e-6)
        return a[:m].copy(), b[:m + 1].copy()
    if name == "TOEP":
        alpha, beta = np.full(m, 2.0), np.ones(m + 1)
    elif name == "WILK":     # Wilkinson's W+_m shifted to positive: eigenvalues in pairs that agree to many digits
        alpha, beta = np.abs(np.arange(m) - (m - 1) / 2.0) + 1.5, np.ones(m + 1)
    elif name == "GRAD":
        g = 10.0 ** (-12.0 * np.arange(m + 1) / m)
        alpha, beta = g[:m].copy(), np.zeros(m + 1)
        beta[1:] = 0.1 * np.sqrt(g[:-1] * g[1:])
    elif name == "NEG":      # one clearly negative eigenvalue: the clamp max(lambda, 0) acts
        rng = np.random.default_rng(1000 + m)
        alpha, beta = rng.uniform(0.5, 1.5, m), np.zeros(m + 1)
        beta[1:] = rng.uniform(0.01, 0.3, m)
        alpha[3] = -0.5
    else:
        raise KeyError(name)
    beta[0] = 0.0
    return alpha, beta


# ---- t = T^{1/2} e_1 ---------------------------------------------------------------------------------------------------------------
def t_ref_mp(alpha, beta, m, dps=DPS):
    """Z sqrt(max(Lambda, 0)) Z^T e_1 from mpmath.eigsy at `dps` digits -> (t as mpf, sorted eigenvalues as mpf)."""
    import mpmath as mp
    with mp.workdps(dps):
        A = mp.zeros(m, m)
        for i in range(m):
            A[i, i] = mp.mpf(float(alpha[i]))
            if i + 1 < m:
                A[i, i + 1] = A[i + 1, i] = mp.mpf(float(beta[i + 1]))
        E, Q = mp.eigsy(A)
        w = [mp.sqrt(max(E[j], mp.mpf(0))) * Q[0, j] for j in range(m)]
        t = [mp.fsum(Q[i, j] * w[j] for j in range(m)) for i in range(m)]
        return t, sorted(E[j] for j in range(m))


@functools.lru_cache(maxsize=None)
def toeplitz_t_ref(m, dps=DPS):
    """TOEP in closed form: lambda_k = 2 + 2 cos(k pi / (m + 1)), z_ik = sqrt(2 / (m + 1)) sin(i k pi / (m + 1)), i, k = 1 .. m."""
    import mpmath as mp
    with mp.workdps(dps):
        h = mp.pi / (m + 1)
        s = [mp.sin(j * h) for j in range((m + 1) * 2)]            # sin(i k h) = s[(i k) mod (2 m + 2)]
        w = [mp.sqrt(2 + 2 * mp.cos(k * h)) * s[k] for k in range(1, m + 1)]
        return tuple(mp.fsum(s[(i * k) % (2 * m + 2)] * w[k - 1] for k in range(1, m + 1)) * 2 / (m + 1) for i in range(1, m + 1))


def t_numpy(alpha, beta, m):
    """float64: numpy.linalg.eigh (LAPACK) on the dense matrix."""
    T = np.diag(np.asarray(alpha[:m], dtype=np.float64))
    for i in range(m - 1):
        T[i, i + 1] = T[i + 1, i] = beta[i + 1]
    w, Z = np.linalg.eigh(T)
    return Z @ (np.sqrt(np.maximum(w, 0.0)) * Z[0])


def max_abs_err(t, t_ref):
    """max_i |t_i - t_ref_i| in multiprecision, as a float."""
    import mpmath as mp
    with mp.workdps(DPS):
        return float(max(abs(mp.mpf(float(a)) - b) for a, b in zip(t, t_ref)))


def norm2(t_ref):
    import mpmath as mp
    with mp.workdps(DPS):
        return float(mp.sqrt(mp.fsum(x * x for x in t_ref)))


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
DECISION_DEFAULTS = dict(m_lo=0, m_hi=0, done_iters=0, have_last_beta=0, pending_beta=0, first=0, last=0, normalised=0, m_max=100,
                         tol=0.0, seq=1.0)


def walk(dec, alpha, beta, norm, state, mirror, t_of):
    """One decision, as the reference's while loop prescribes it (PSEv1/Brownian.cu:503, 606-724) under the contract LzDecide ->
    LzState of pse_host.h, which the device's k_lz_decide and the host drivers' lz_decide_host both implement, with t_of(m) in place
    of an eigen-solver: t_of returns T_m^{1/2} e_1 as a sequence of m numbers, or None where no solver can succeed (a non-finite
    entry inside T_m).

    state: None before the first decision, else what the previous call returned; mirror: dict of MIRROR_FIELDS.  Returns the new
    (state, mirror); state = dict(done, m_final, status, checked, stepnorm, t_prev, coef): t_prev the vector of size `checked`, coef
    the m_final coefficients of the final combination (t divided by the norm, then by beta_q or -- normalised basis -- by 1), None
    while the iteration is open or where the walk ends before any size was solved."""
    import mpmath as mp
    d = dict(DECISION_DEFAULTS, **dec)
    if not d["first"]:
        if state is None:
            raise ValueError("the first decision of a call must reset the state")
        if state["done"]:
            return state, mirror
    checked, stepnorm, t_prev = (0, 1.0, None) if d["first"] else (state["checked"], state["stepnorm"], state["t_prev"])
    m_final, status, t_fin = 0, 0, None
    pend = d["pending_beta"]
    with mp.workdps(DPS):
        if not (norm > 0.0) or not math.isfinite(norm):          # psi == 0: the result is zero
            m_final = -1
        elif pend > 0 and beta[pend] < BREAKDOWN:                # |x_m| of the vector the previous batch ended on
            m_final, stepnorm, t_fin = pend, 0.0, t_prev
        else:
            for m in range(d["m_lo"], d["m_hi"] + 1):
                have_beta = m < d["done_iters"] or d["have_last_beta"]
                t = t_of(m)
                if not math.isfinite(alpha[m - 1]) or (have_beta and not math.isfinite(beta[m])) or t is None:
                    m_final, status, t_fin = max(checked, 1), 2, (t_prev if checked else None)
                    break
                if m < d["done_iters"] and beta[m] < BREAKDOWN:  # invariant subspace
                    m_final, stepnorm, t_fin = m, 0.0, t
                    break
                if checked == m - 1 and checked > 0:
                    s2 = mp.mpf(t[m - 1]) ** 2 + mp.fsum((mp.mpf(t[q]) - mp.mpf(t_prev[q])) ** 2 for q in range(m - 1))
                    stepnorm = mp.sqrt(s2 / mp.mpf(float(alpha[0])))
                    if stepnorm <= d["tol"] or m >= d["m_max"]:
                        m_final, t_fin = m, t
                        break
                if d["have_last_beta"] and m == d["done_iters"] and beta[m] < BREAKDOWN:
                    m_final, stepnorm, t_fin = m, 0.0, t
                    break
                t_prev, checked = t, m
            if not m_final and (d["last"] or d["done_iters"] >= d["m_max"]):   # nothing more is queued: end with what there is
                m_final, t_fin, status = checked, t_prev, (0 if d["done_iters"] >= d["m_max"] else 1)
        new = dict(done=0, m_final=0, status=0, checked=checked, stepnorm=stepnorm, t_prev=t_prev, coef=None)
        if not d["first"]:
            new.update(m_final=state["m_final"], status=state["status"], coef=state["coef"])
        if m_final:
            m = max(m_final, 0)
            coef = None
            if t_fin is not None:
                coef = [mp.mpf(t_fin[q]) / (mp.mpf(norm) if q == 0 else (1 if d["normalised"] else mp.mpf(float(beta[q])))) for q in range(m)]
            new.update(done=1, m_final=m, status=status, coef=coef)
            mirror = dict(mirror, m=float(m), stepnorm=stepnorm, status=float(status), seq=float(d["seq"]))
            if status != 0:
                mirror["open"] = mirror["open"] + 1.0
    return new, mirror


def coef_divisor(d, beta, norm, q):
    return abs(norm) if q == 0 else (1.0 if d.get("normalised", 0) else abs(float(beta[q])))


def stepnorm_bound(m, e_ref, alpha0):
    """|stepnorm_device - stepnorm_ref| <= (|dt_m| + |dt_{m-1}|) / sqrt(alpha_0), each vector within FACTOR e_ref per entry."""
    return (math.sqrt(m) + math.sqrt(m - 1)) * FACTOR * e_ref / math.sqrt(alpha0)


# ---- the sequences of decisions the four drivers issue (pse_capi.hip) --------------------------------------------------------------------
def queued_decisions(m_in, extra, tol, m_max=100, seq=1.0):
    """lanczos_queued: the pair (m_in - 1, m_in), then `extra` gated single sizes, each with the beta that arrived pending."""
    target = max(m_in, 2)
    out = [dict(m_lo=max(m_in - 1, 1), m_hi=target, done_iters=target, first=1, last=int(extra == 0), m_max=m_max, tol=tol, seq=seq)]
    done = target
    for x in range(extra):
        out.append(dict(m_lo=done + 1, m_hi=done + 1, done_iters=done + 1, pending_beta=done, first=0, last=int(x == extra - 1),
                        m_max=m_max, tol=tol, seq=seq))
        done += 1
    return out


def local_decisions(m_in, extra_blocks, tol, m_max=100, seq=1.0):
    """lanczos_local (owned-particle teams, two iterations per exchange): normalised basis, beta[done_iters] exists."""
    target = max(m_in, 2)
    out = [dict(m_lo=max(m_in - 1, 1), m_hi=target, done_iters=target, have_last_beta=1, first=1, last=int(extra_blocks == 0),
                normalised=1, m_max=m_max, tol=tol, seq=seq)]
    done = target
    for x in range(extra_blocks):
        out.append(dict(m_lo=done + 1, m_hi=done + 2, done_iters=done + 2, have_last_beta=1, first=0, last=int(x == extra_blocks - 1),
                        normalised=1, m_max=m_max, tol=tol, seq=seq))
        done += 2
    return out


def host_decisions(m_in, batches, two_step, tol, m_max=100, seq=1.0):
    """lanczos (one iteration per exchange) and lanczos_team (two_step), host-checked: batches up to max(m_in, 2), then up to
    done + max(2, done / 4), not beyond m_max; each decision checks every size not yet checked, from m_in - 1 on.  The one-step driver
    gets beta[done] with its next batch (pending_beta); the two-step driver has it, and a normalised basis."""
    out, done, target = [], 0, max(m_in, 2)
    for k in range(batches):
        d = dict(m_lo=max(done + 1, m_in - 1, 1), m_hi=target, done_iters=target, first=int(k == 0), last=0, m_max=m_max, tol=tol, seq=seq)
        d.update(dict(have_last_beta=1, normalised=1) if two_step else dict(pending_beta=done))
        out.append(d)
        done, target = target, min(m_max, target + max(2, target // 4))
    return out


def scal_image(alpha, beta, norm, decisions, patches=(), poison=True):
    """The device scalars of a sequence of decisions.  poison: every entry no decision of the sequence has a right to read is NaN --
    alpha[q >= done_iters], beta[0], beta[q > done_iters], beta[done_iters] unless have_last_beta, and all the other slots.
    patches: (array name, index, value) written last."""
    done = max(d["done_iters"] for d in decisions)
    last_beta = any(d.get("have_last_beta", 0) for d in decisions if d["done_iters"] == done)
    s = np.full(LZ_NSCAL, np.nan if poison else 0.0)
    n_a = min(done, len(alpha)) if poison else len(alpha)
    n_b = min(done + (1 if last_beta else 0), len(beta)) if poison else len(beta)
    s[LZ_ALPHA:LZ_ALPHA + n_a] = alpha[:n_a]
    s[LZ_BETA + 1:LZ_BETA + n_b] = beta[1:n_b]
    s[LZ_NORM] = norm
    for name, idx, val in patches:
        s[(LZ_ALPHA if name == "alpha" else LZ_BETA) + idx] = val
    return s


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------
def _unhex(xs):
    return np.array([float.fromhex(x) for x in xs])


class Fixture:
    def __init__(self, path=FIXTURE_PATH):
        with gzip.open(path, "rt") as f:
            self.raw = json.load(f)
        assert self.raw["dps"] == DPS
        self.cases = self.raw["cases"]
        for c in self.cases:
            c["decisions"] = [dict(d, tol=float.fromhex(d["tol"])) for d in c["decisions"]]

    def coeffs(self, fam, m):
        """alpha[0..m), beta[0..m] as stored (float.hex: bit for bit what the references were computed from)."""
        f = self.raw["families"][fam]
        src = f if fam in SHARED else f["sizes"][str(m)]
        return _unhex(src["alpha"])[:m], _unhex(src["beta"])[:m + 1]

    def info(self, fam, m):
        """lam_min, gap_min, lam_max_abs, lam_min_pos, e_numpy of an entry (floats)."""
        e = self.raw["families"][fam]["sizes"][str(m)]
        return {k: float.fromhex(e[k]) for k in ("lam_min", "gap_min", "lam_max_abs", "lam_min_pos", "e_numpy")}

    @functools.lru_cache(maxsize=None)
    def t_ref(self, fam, m):
        import mpmath as mp
        if fam == "TOEP":
            return toeplitz_t_ref(m)
        with mp.workdps(DPS):
            return tuple(mp.mpf(x) for x in self.raw["families"][fam]["sizes"][str(m)]["t"])

    @functools.lru_cache(maxsize=None)
    def e_host(self, fam, m):
        import pse_amd
        a, b = self.coeffs(fam, m)
        return max_abs_err(pse_amd.host_lanczos_sqrt_e1(a, b), self.t_ref(fam, m))

    def e_ref(self, fam, m):
        """The yardstick: the larger of the two float64 solvers' own errors, and no less than one rounding of |t|."""
        return max(self.info(fam, m)["e_numpy"], self.e_host(fam, m), U * norm2(self.t_ref(fam, m)))

    def backward_bound(self, fam, m):
        """8 m u |T|_2 / (2 sqrt(lambda_min+)): a backward-stable eigen-solve through the Frechet derivative of the square root."""
        i = self.info(fam, m)
        return 8.0 * m * U * i["lam_max_abs"] / (2.0 * math.sqrt(i["lam_min_pos"]))

    # -- decision cases --
    def case_inputs(self, case):
        """(alpha, beta, norm, patches, scal image, t_of) of a decision case; alpha / beta with the patches applied."""
        fam = case["family"]
        a0, b0 = self.coeffs(fam, M_SUPPORTED)
        norm = float.fromhex(case["norm"])
        patches = [(n, i, float.fromhex(v)) for n, i, v in case["patches"]]
        scal = scal_image(a0, b0, norm, case["decisions"], patches)
        alpha, beta = scal[LZ_ALPHA:LZ_ALPHA + 104].copy(), scal[LZ_BETA:LZ_BETA + 104].copy()

        def t_of(m):
            inside = np.concatenate([alpha[:m], beta[1:m]])
            if not np.all(np.isfinite(inside)):
                return None
            assert np.array_equal(alpha[:m], a0[:m]) and np.array_equal(beta[1:m], b0[1:m]), "the walk needs t of a patched tridiagonal"
            return self.t_ref(fam, m)
        return alpha, beta, norm, patches, scal, t_of

    def case_reference(self, case):
        """The reference walk over the decisions of a case: one (state, mirror) per launch."""
        alpha, beta, norm, _, _, t_of = self.case_inputs(case)
        state, mirror = None, dict(m=0.0, stepnorm=0.0, status=0.0, seq=0.0, open=float(case["open0"]))
        out = []
        for d in case["decisions"]:
            state, mirror = walk(d, alpha, beta, norm, state, mirror, t_of)
            out.append((state, mirror))
        return out

    @functools.lru_cache(maxsize=None)
    def stepnorm_ref(self, fam, m):
        """The step norm of size m against size m - 1, as a float."""
        import mpmath as mp
        a, _ = self.coeffs(fam, m)
        with mp.workdps(DPS):
            t, tp = self.t_ref(fam, m), self.t_ref(fam, m - 1)
            return float(mp.sqrt((t[m - 1] ** 2 + mp.fsum((t[q] - tp[q]) ** 2 for q in range(m - 1))) / mp.mpf(float(a[0]))))


@functools.lru_cache(maxsize=None)
def fixture():
    return Fixture()


# ---- the checker: an implementation of the contract against the reference walk, after every decision ---------------------------------
def bits(o):
    """Everything a launch leaves, as bytes: for 'this launch changed nothing'."""
    return (o["done"], o["m_final"], o["checked"], o["status"], np.float64(o["stepnorm"]).tobytes(), o["t_prev"].tobytes(),
            o["coef"].tobytes(), tuple(np.float64(o["mirror"][k]).tobytes() for k in MIRROR_FIELDS))


def run_case(fx, case, decide, open0=None):
    """decide: pse_amd.debug_lz_decide (the device) or pse_amd.host_lz_decide (the host drivers' twin)."""
    alpha, beta, norm, _, scal, _ = fx.case_inputs(case)
    open0 = case["open0"] if open0 is None else open0
    ref = fx.case_reference(dict(case, open0=open0))
    out = decide(scal, case["decisions"], open0)
    fam, a0 = case["family"], fx.coeffs(case["family"], 1)[0][0]
    for k, (d, o, (r, rm)) in enumerate(zip(case["decisions"], out, ref)):
        where = (case["name"], k)
        assert (o["done"], o["m_final"], o["status"], o["checked"]) == (r["done"], r["m_final"], r["status"], r["checked"]), where
        if k > 0 and ref[k - 1][0]["done"]:
            assert bits(o) == bits(out[k - 1]), where               # after done: a further decision leaves state and mirror as they are
        e_step = max([fx.e_ref(fam, m) for m in range(max(d["m_lo"] - 1, 1), d["m_hi"] + 1)])
        bound = stepnorm_bound(d["m_hi"], e_step, a0)
        assert abs(o["stepnorm"] - float(r["stepnorm"])) <= bound, where + (o["stepnorm"], float(r["stepnorm"]), bound)
        if r["checked"] and np.isfinite(norm) and norm > 0:
            c = r["checked"]
            assert max_abs_err(o["t_prev"][:c], r["t_prev"]) <= FACTOR * fx.e_ref(fam, c), where
            assert np.isnan(o["t_prev"][c:]).all(), where
        m = r["m_final"]
        if r["done"] and r["coef"] is not None:
            e = fx.e_ref(fam, m)
            for q in range(m):
                assert abs(o["coef"][q] - float(r["coef"][q])) <= FACTOR * e / coef_divisor(d, beta, norm, q), where + (q,)
        if r["done"]:
            assert np.isnan(o["coef"][m:]).all(), where              # nothing beyond m_final was written
        for f in ("m", "status", "seq", "open"):
            assert o["mirror"][f] == float(rm[f]), where + (f, o["mirror"][f], float(rm[f]))
        assert abs(o["mirror"]["stepnorm"] - float(rm["stepnorm"])) <= bound, where
        if r["done"]:
            assert o["mirror"]["stepnorm"] == o["stepnorm"], where
    return out
