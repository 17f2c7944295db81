"""Self-diffusion under shear: 20 000 soft-repulsive Brownian spheres at phi = 0.1 in a steady Lees-Edwards shear that flips the box
once on the way, 700 steps.  analyze.MSD keeps ten time origins of unwrapped positions on the device and sums the displacement
moments of every fifth step against all of them; read at the end: the mean-squared displacement across the flow, msd_yy + msd_zz --
the two components that carry no affine advection -- against the lag, and its slope over 4 dt in units of D0 = kT (the mobility is in
units of 1/(6 pi eta a)): the self-diffusion coefficient D/D0.  (msd(), the trace, and alpha2() contain the advection dx = rate y t
under shear: they are for quiescent runs.)"""
import numpy as np, math, sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pse_amd import analyze, forces, integrate, shear_function, variant
from pse_amd.system import System
rng = np.random.default_rng(5)
n, phi, dt, kT, rate = 20000, 0.1, 1e-3, 1.0, 1.0
L = (4*math.pi*n/(3*phi))**(1/3)
s = System(rng.uniform(-L/2, L/2, size=(n, 3)), (L, L, L, 0.0), dt=dt)
ff = shear_function.steady(dt=dt, shear_rate=rate)
s.box_tilt_variant = variant.shear_variant(ff, 100000, max_strain=0.5)
pse = integrate.PSEv1(group=s.all(), T=kT, seed=11, xi=0.5, error=1e-3, function_form=ff)
forces.HarmonicRepulsion(pse, k=200.0, sigma=2.0)
s.run(100)                                   # let the overlaps of the random start relax
msd = analyze.MSD(pse, nlags=40, origin_every=4, period=5)
s.run(600)
t = msd.lags * dt
tensor = msd.msd_tensor()
across = tensor[:, 1, 1] + tensor[:, 2, 2]
print('strain %.3f  flips %d  samples %d  origins per lag %d .. %d' % (s.strain, s.tilt_flips, msd.samples, msd.counts.min(), msd.counts.max()))
print(' lag/steps   t        msd_yy+msd_zz   D/D0 (slope / 4 dt)')
for k in range(0, msd.nlags, 4):
    slope = (across[k] - (across[k-1] if k else 0.0)) / (t[k] - (t[k-1] if k else 0.0))
    print('%8d  %7.4f  %14.6g  %10.4f' % (msd.lags[k], t[k], across[k], slope / (4*kT)))
print('D/D0 over the whole window: %.4f' % (across[-1] / (4*kT*t[-1])))
