"""How the chains of a polymer solution relax: the FENE chains of polymer_solution.py (200 chains of 10 beads at phi = 0.1, a harmonic
core between all beads, hydrodynamic interactions and Brownian motion) at rest, measured by one analyze.RouseModes -- every sample one
projection of every chain onto its normal modes X_p and the end-to-end vector R, one correlation with the live time origins and one
store, all on the device; nothing is copied to the host until the run is over.  Prints p, the amplitude <X_p^2> and the relaxation
time tau_p (the first crossing of 1/e of <X_p(t).X_p(0)> / <X_p^2>) for p = 1 .. 4, the tau of R, and the exponent of a log-log fit
of tau_p against p -- beside it, as text, what the Zimm model (hydrodynamic interactions: tau_p ~ p^(-3 nu)) and the Rouse model
(none: tau_p ~ p^(-(1 + 2 nu))) predict for an ideal (nu = 1/2) and a swollen (nu = 0.588) chain.  A chain of ten beads is short and
the run (60000 steps, a few times the longest relaxation time of some 20000 steps) is short: the fit shows where the chains stand, it
proves neither model.  `--chains C --beads B --steps S` change the size; a mode that does not fall to 1/e within the lags prints nan
and is left out of the fit."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from polymer_solution import build_chains


def main(argv):
    import torch
    from pse_amd import analyze, integrate, forces
    from pse_amd.system import System
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    nchains, beads, steps, phi = opt("--chains", 200), opt("--beads", 10), opt("--steps", 60000), 0.1
    n = nchains * beads
    L = (4 * math.pi * n / (3 * phi)) ** (1 / 3)
    box = (L, L, L, 0.0)
    k_fene, r0 = 30.0 / 4.0, 3.0
    pos, pairs = build_chains(nchains, beads, box, 2.0, seed=5)
    s = System(pos, box, dt=1e-3)
    pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3)
    kc = 200.0   # core: k/2 (2 - r)^2 for r < 2
    forces.TablePair.from_functions(pse, lambda r: 0.5 * kc * (2.0 - r) ** 2, lambda r: kc * (2.0 - r), 0.0, 2.0, 256)
    bonds = forces.Bonds(pse, pairs, kind="fene", k=k_fene, r0=r0)
    nmodes = min(4, beads - 1)
    period = max(1, steps // 150)                     # some 150 samples; lags up to 64 samples, a new origin every second sample
    modes = analyze.RouseModes(pse, bonds, nmodes=nmodes, nlags=64, origin_every=2, period=period)
    torch.cuda.synchronize()
    t0 = time.time()
    s.run(steps)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert bool(torch.isfinite(s.pos).all()) and bonds.overstretched == 0
    amp, tau, c = modes.amplitudes(), modes.relaxation_times() * s.dt, modes.autocorrelation()
    print(modes.nlin, 'chains of', beads, 'beads,', modes.samples, 'samples every', period, 'steps, lags up to', int(modes.lags[-1]), 'steps')
    print('   <R^2> %.4f   tau_R %.4g   (C_R at the last lag %.3f)' % (amp[0], tau[0], c[-1, 0]))
    for p in range(1, nmodes + 1):
        print('   p %d   <X_p^2> %.5f   tau_p %.4g   (C_p at the last lag %.3f)' % (p, amp[p], tau[p], c[-1, p]))
    ok = np.isfinite(tau[1:])
    if ok.sum() >= 2:
        slope = np.polyfit(np.log(np.arange(1, nmodes + 1)[ok]), np.log(tau[1:][ok]), 1)[0]
        print('   tau_p ~ p^%.2f over p = %s' % (slope, ', '.join(str(p) for p in np.arange(1, nmodes + 1)[ok])))
    else:
        print('   fewer than two modes fell to 1/e within the lags: run longer (--steps)')
    print('   Zimm: p^-1.50 (nu = 1/2), p^-1.76 (nu = 0.588);  Rouse: p^-2.00 (nu = 1/2), p^-2.18 (nu = 0.588)')
    print('   %d steps in %.2f s, %.3f ms per step' % (steps, dt, 1e3 * dt / steps))
    assert np.isfinite(amp).all() and np.all(amp > 0.0) and np.all(c[0] == 1.0)


if __name__ == "__main__":
    main(sys.argv[1:])
