"""Writes tests/golden/lanczos_decision.json.gz: the multiprecision references of tests/lanczos_decision_ref.py, computed once.

    python tests/golden/make_lanczos_decision_fixture.py [--jobs N] [--out PATH]

For every (family, size) of lanczos_decision_ref.FAMILY_SIZES: t = T^{1/2} e_1 from mpmath.eigsy at 40 digits (TOEP: closed form, not
stored), the smallest eigenvalue, the smallest gap, |T|_2, the smallest positive eigenvalue and the error of float64 numpy.linalg.eigh.
K3 at m = 98 is solved at 50 digits as well and must agree to 1e-25.  Then the decision cases of tests/test_gpu_lanczos_decision.py:
their sizes are SEARCHED on the reference step norms of K3 so that every tolerance keeps a margin to the step norms on either side.
About 12 CPU-minutes (mpmath.eigsy: 0.8 s at m = 33, 19 s at m = 98), spread over --jobs processes; the output does not depend on N."""
import argparse
import gzip
import json
import math
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lanczos_decision_ref as R   # noqa: E402

SEP = 1.06        # smallest ratio of a step norm that must fail to the one that must pass: tol at the geometric mean is > 1.01 from both
NORM = 2.5        # |psi| of the walk cases (the square-root tests use 1)


def hexes(xs):
    return [float(x).hex() for x in xs]


def entry(task):
    import mpmath as mp
    fam, m = task
    t0 = time.time()
    alpha, beta = R.family(fam, m)
    with mp.workdps(R.DPS):
        if fam == "TOEP":
            t = R.toeplitz_t_ref(m)
            lam = sorted(2 + 2 * mp.cos(k * mp.pi / (m + 1)) for k in range(1, m + 1))
        else:
            t, lam = R.t_ref_mp(alpha, beta, m)
        if (fam, m) == ("K3", R.M_SUPPORTED):
            t50, _ = R.t_ref_mp(alpha, beta, m, dps=50)
            with mp.workdps(50):
                d = float(max(abs(a - b) for a, b in zip(t, t50)))
            assert d <= 1e-25, f"K3 at m = {m}: 40 and 50 digits differ by {d:.2e}: raise DPS for every case"
        if fam == "NEG":
            assert lam[0] < -0.1, (fam, m, float(lam[0]))
        e = dict(lam_min=float(lam[0]).hex(),
                 gap_min=float(min([lam[k + 1] - lam[k] for k in range(m - 1)] or [mp.inf])).hex(),
                 lam_max_abs=float(max(abs(lam[0]), abs(lam[-1]))).hex(),
                 lam_min_pos=float(min(x for x in lam if x > 0)).hex(),
                 e_numpy=R.max_abs_err(R.t_numpy(alpha, beta, m), t).hex())
        if fam != "TOEP":
            e["t"] = [mp.nstr(x, R.DPS) for x in t]
        if fam not in R.SHARED:
            e["alpha"], e["beta"] = hexes(alpha), hexes(beta)
    return fam, m, e, time.time() - t0


def step_norms(fam, sizes):
    """Reference step norm of size m against m - 1, as floats, for m = 2 .. 98."""
    import mpmath as mp
    alpha, _ = R.family(fam, R.M_SUPPORTED)
    out = {}
    with mp.workdps(R.DPS):
        ts = {m: [mp.mpf(x) for x in sizes[str(m)]["t"]] for m in R.ALL_SIZES}
        for m in range(2, R.M_SUPPORTED + 1):
            t, tp = ts[m], ts[m - 1]
            out[m] = float(mp.sqrt((t[m - 1] ** 2 + mp.fsum((t[q] - tp[q]) ** 2 for q in range(m - 1))) / mp.mpf(float(alpha[0]))))
    return out


def build_cases(s):
    """The sequences of decisions of the GPU tests on K3.  s[m]: reference step norms.  `fail`: sizes whose step norm must exceed the
    tolerance, `pass`: the size whose step norm must pass (None: none does); intent: [done, m_final, status] after every launch."""
    cases = []

    def sep(fail, pas):
        return min(s[f] for f in fail) / s[pas] >= SEP

    def near(target, ok, lo=3, hi=95):
        for k in range(60):
            for m in (target + k, target - k):
                if lo <= m <= hi and ok(m):
                    return m
        raise RuntimeError(f"no size near {target} keeps the margin")

    def tol_for(fail, pas):
        if fail and pas:
            return math.sqrt(min(s[f] for f in fail) * s[pas])
        return SEP * s[pas] if pas else min(s[f] for f in fail) / SEP

    def add(name, decisions, fail, pas, intent, norm=NORM, patches=(), open0=0.0):
        assert len(intent) == len(decisions) and not any(c["name"] == name for c in cases), name
        cases.append(dict(name=name, family="K3", norm=float(norm).hex(), open0=open0,
                          patches=[[n, i, float(v).hex()] for n, i, v in patches],
                          decisions=[dict(d, tol=float(d["tol"]).hex()) for d in decisions], fail=list(fail), **{"pass": pas}, intent=intent))

    open_ = [0, 0, 0]
    for m in (6, 33, 64, 65, 66, 96):      # converged at the first pair; the two gated extras then leave at once
        add(f"first_pair_{m}", R.queued_decisions(m, 2, tol_for([], m)), [], m, [[1, m, 0]] * 3)
    for tgt in (20, 64):                   # converged in the first gated extra
        m = near(tgt, lambda m: sep([m], m + 1))
        add(f"extra1_{m}", R.queued_decisions(m, 2, tol_for([m], m + 1)), [m], m + 1, [open_, [1, m + 1, 0], [1, m + 1, 0]])
    for tgt in (30, 63):                   # ... in the second
        m = near(tgt, lambda m: sep([m, m + 1], m + 2))
        add(f"extra2_{m}", R.queued_decisions(m, 2, tol_for([m, m + 1], m + 2)), [m, m + 1], m + 2, [open_, open_, [1, m + 2, 0]])
    for m in (12, 65):                     # the queue ran out: status 1, the result of the last size checked
        add(f"ran_out_{m}", R.queued_decisions(m, 1, tol_for([m, m + 1], None)), [m, m + 1], None, [open_, [1, m + 1, 1]])
    for m in (40, 66):                     # breakdown beta_m < 1e-8 inside (m < done_iters)
        add(f"breakdown_inside_{m}", R.queued_decisions(m, 2, 1e-3), [], None, [[1, m - 1, 0]] * 3, patches=[("beta", m - 1, 1e-9)])
    for m in (10, 64):                     # ... through pending_beta: the result is the previous size's
        add(f"breakdown_pending_{m}", R.queued_decisions(m, 2, tol_for([m], None)), [m], None, [open_, [1, m, 0], [1, m, 0]],
            patches=[("beta", m, 1e-9)])
    for m in (17, 65):                     # ... at m = done_iters, which only the team form can see (have_last_beta)
        add(f"breakdown_last_beta_{m}", R.local_decisions(m, 1, tol_for([m], None)), [m], None, [[1, m, 0]] * 2, patches=[("beta", m, 1e-9)])
    m = near(64, lambda m: sep([m], m + 1))   # the team form: normalised basis, pairs of sizes
    add(f"team_first_of_block_{m}", R.local_decisions(m, 1, tol_for([m], m + 1)), [m], m + 1, [open_, [1, m + 1, 0]])
    for tgt in (31, 96):
        m = near(tgt, lambda m: sep([m, m + 1], m + 2), hi=96)
        add(f"team_second_of_block_{m}", R.local_decisions(m, 1, tol_for([m, m + 1], m + 2)), [m, m + 1], m + 2, [open_, [1, m + 2, 0]])
    for m in (8, 66):                      # m_max reached with the step norm above the tolerance: status 0
        add(f"m_max_{m}", [dict(m_lo=m - 1, m_hi=m, done_iters=m, first=1, last=0, m_max=m, tol=tol_for([m], None), seq=1.0)], [m], None,
            [[1, m, 0]])
    add("nan_alpha_first_size", R.queued_decisions(6, 2, 1e-3), [], None, [[1, 1, 2]] * 3, patches=[("alpha", 2, math.nan)], open0=3.0)
    m = 64                                 # a NaN alpha arrives with the first extra: the result is the size checked before
    add(f"nan_alpha_extra_{m}", R.queued_decisions(m, 2, tol_for([m], None)), [m], None, [open_, [1, m, 2], [1, m, 2]],
        patches=[("alpha", m, math.nan)], open0=1.0)
    for m in (9, 65):                      # an infinite beta_m that have_last_beta brings into play
        add(f"inf_last_beta_{m}", [dict(m_lo=m - 1, m_hi=m, done_iters=m, have_last_beta=1, first=1, last=1, normalised=1, m_max=100,
                                        tol=1e-3, seq=1.0)], [], None, [[1, m - 1, 2]], patches=[("beta", m, math.inf)])
    dead = [("alpha", q, math.nan) for q in range(6)] + [("beta", q, math.nan) for q in range(1, 6)]
    add("norm_zero", R.queued_decisions(6, 0, 1e-3), [], None, [[1, 0, 0]], norm=0.0, patches=dead)
    add("norm_nan", R.queued_decisions(6, 0, 1e-3), [], None, [[1, 0, 0]], norm=math.nan, patches=dead)
    # To the largest size through single-size extras from 96.  By the step norm where K3 allows it; its step norms are not monotone
    # there (96: 1.97e-7, 97: 2.09e-7, 98: 2.06e-7 -- no tolerance fails 96 and 97 and passes 98), so the walk then ends at 98 because
    # that is m_max, with every step norm above the tolerance: status 0 all the same.
    if sep([96, 97], 98):
        add("to_98_from_96", R.queued_decisions(96, 2, tol_for([96, 97], 98)), [96, 97], 98, [open_, open_, [1, 98, 0]])
    else:
        add("to_98_from_96_by_m_max", R.queued_decisions(96, 2, tol_for([96, 97, 98], None), m_max=98), [96, 97, 98], None,
            [open_, open_, [1, 98, 0]])
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=R.FIXTURE_PATH)
    args = ap.parse_args()
    tasks = sorted(((fam, m) for fam in R.FAMILY_SIZES for m in R.FAMILY_SIZES[fam]), key=lambda x: -x[1])   # the long ones first
    fams = {fam: dict(sizes={}) for fam in R.FAMILY_SIZES}
    t0 = time.time()
    with multiprocessing.Pool(args.jobs) as pool:
        for fam, m, e, dt in pool.imap_unordered(entry, tasks):
            fams[fam]["sizes"][str(m)] = e
            print(f"{fam:5s} m = {m:2d}  lam_min {float.fromhex(e['lam_min']):10.3e}  gap {float.fromhex(e['gap_min']):9.2e}  "
                  f"e_numpy {float.fromhex(e['e_numpy']):9.2e}  {dt:5.1f} s", flush=True)
    for fam in R.FAMILY_SIZES:   # a fixed order, whichever process finished first
        fams[fam]["sizes"] = {str(m): fams[fam]["sizes"][str(m)] for m in R.FAMILY_SIZES[fam]}
    for fam in R.SHARED:
        a, b = R.family(fam, R.M_SUPPORTED)
        fams[fam]["alpha"], fams[fam]["beta"] = hexes(a), hexes(b)
    s = step_norms("K3", fams["K3"]["sizes"])
    print("K3 step norms: " + " ".join(f"{m}:{s[m]:.3e}" for m in sorted(s)), flush=True)
    cases = build_cases(s)
    for c in cases:
        print(f"case {c['name']}: fail {c['fail']} pass {c['pass']} tol {[float.fromhex(d['tol']) for d in c['decisions']][0]:.4e}", flush=True)
    doc = dict(dps=R.DPS, families=fams, step_norms_K3={str(m): s[m].hex() for m in sorted(s)}, cases=cases)
    data = json.dumps(doc, sort_keys=True, separators=(",", ":")).encode()
    with open(args.out, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:   # (no name, no time: the same bytes every run)
        g.write(data)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(cases)} cases, {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    main()
