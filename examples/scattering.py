"""Dynamic scattering from a suspension at rest: 8 000 soft-repulsive Brownian spheres at phi = 0.1, 2 500 steps.  After 1 500 steps
(three times a^2 / D0) for the structure of the random start to relax, analyze.IntermediateScattering samples every fifth step: it
keeps eight time origins of fractional coordinates and densities on the device and correlates every sample with all of them, on
every mode of the box with |k| a <= 1.  Read at the end, per shell of |k|: the self part F_s(k, t) and the normalised collective part
f(k, t) = F / S at a few lags; the short-time self-diffusion D_s(k)/D0 = -ln F_s / (<k^2> D0 t) at the first lag; and the hydrodynamic
function H(k) = S(k) D_c(k) / D0 from the initial slope of ln f, D_c(k) = -ln f / (<k^2> t).  D0 = kT: the mobility is in units of
1/(6 pi eta a).  Without hydrodynamic interactions H(k) is identically 1.  D_s/D0 comes out as the self-mobility of the periodic
Rotne-Prager-Yamakawa tensor, about 1 - 2.837 a/L, in every shell; the collective part of 200 samples of one run is noisy where a
shell holds few modes: an indication, not a measurement."""
import numpy as np, math, sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pse_amd import analyze, forces, integrate
from pse_amd.system import System
rng = np.random.default_rng(5)
n, phi, dt, kT = 8000, 0.1, 2e-3, 1.0
L = (4*math.pi*n/(3*phi))**(1/3)
box = (L, L, L, 0.0)
s = System(rng.uniform(-L/2, L/2, size=(n, 3)), box, dt=dt)
pse = integrate.PSEv1(group=s.all(), T=kT, seed=11, xi=0.5, error=1e-3)
forces.HarmonicRepulsion(pse, k=200.0, sigma=2.0)
s.run(1500)                                  # let the structure of the random start relax
modes = analyze.modes_within(box, 1.0)
isf = analyze.IntermediateScattering(pse, modes, nlags=8, origin_every=1, period=5)
s.run(1000)
t = isf.lags * dt
nbins = 6
k, Fs, cnt = isf.shell_average(isf.Fs(), nbins)
_, f, _ = isf.shell_average(isf.f(), nbins)
_, S, _ = isf.shell_average(isf.S(), nbins)
_, k2, _ = isf.shell_average((isf.k**2).sum(axis=1), nbins)
print('%d modes, %d samples, origins per lag %d .. %d' % (len(modes), isf.samples, isf.counts.min(), isf.counts.max()))
print('   |k|a  modes    S(k)   ' + '  '.join('Fs(t=%.2f)' % t[j] for j in (0, 3, 7)) + '   ' + '  '.join(' f(t=%.2f)' % t[j] for j in (0, 3, 7))
      + '   Ds/D0     H(k)')
for b in range(nbins):
    if cnt[b] == 0:
        continue
    Ds = -math.log(Fs[0, b]) / (k2[b] * kT * t[0])
    H = S[b] * -math.log(f[0, b]) / (k2[b] * kT * t[0])
    print('%7.3f  %5d  %7.4f   ' % (k[b], cnt[b], S[b]) + '  '.join('%10.6f' % Fs[j, b] for j in (0, 3, 7)) + '   '
          + '  '.join('%10.6f' % f[j, b] for j in (0, 3, 7)) + '  %7.4f  %7.4f' % (Ds, H))
