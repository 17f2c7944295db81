"""An attractive suspension under shear: 8 000 spheres at phi = 0.2 with a Morse attraction outside contact and a harmonic core
repulsion inside it, both given as Python functions and tabulated by forces.TablePair.from_functions (pse_pair_table: one kernel for
any short-range central potential), under oscillatory Lees-Edwards shear with Brownian motion; 500 steps.  Prints per block of 100
steps a health line and the rheology of the block: the potential energy U and the particle stress sigma_xy of the two potentials
together, sampled every 10 steps by the force passes themselves into device logs (forces.StressLog) that are read once per block."""
import numpy as np, math, sys, time, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from pse_amd import integrate, shear_function, variant, forces
from pse_amd.system import System
rng = np.random.default_rng(5)
n, phi = 8000, 0.2
L = (4*math.pi*n/(3*phi))**(1/3)
pos = rng.uniform(-L/2, L/2, size=(n,3))
s = System(pos, (L,L,L,0.0), dt=1e-3)
ff = shear_function.sine(dt=1e-3, shear_rate=1.0, shear_freq=1.0)
s.box_tilt_variant = variant.shear_variant(ff, 2000, max_strain=0.5)
pse = integrate.PSEv1(group=s.all(), T=1.0, seed=11, xi=0.5, error=1e-3, function_form=ff)
# core: k/2 (2 - r)^2 for r < 2 (contact of unit spheres); F = -dV/dr > 0 pushes apart
k = 200.0
core = forces.TablePair.from_functions(pse, lambda r: 0.5*k*(2.0-r)**2, lambda r: k*(2.0-r), 0.0, 2.0, 256, virial=True)
# attraction: Morse well of depth D = 3 kT at r0 = 2.1, range 1/alpha = 0.25, from contact to 3.2, shifted to end at V = 0
D, alpha, r0, r1 = 3.0, 4.0, 2.1, 3.2
e = lambda r: math.exp(-alpha*(r-r0))
Vm = lambda r: D*((1.0-e(r))**2 - 1.0)
well = forces.TablePair.from_functions(pse, lambda r: Vm(r) - Vm(r1), lambda r: -2.0*D*alpha*(1.0-e(r))*e(r), 2.0, r1, 1024, virial=True)
logs = [forces.StressLog(p, period=10, capacity=10) for p in (core, well)]   # one block of samples each; the rings then start over
t0=time.time()
for blk in range(5):
    s.run(100)
    p = s.pos
    ok = bool(torch.isfinite(p).all())
    print(blk, 'finite', ok, 'xy', round(s.box[3],4), 'm', pse.cpp_method.lanczosIterations(), 'maxF', float(s.net_force[:,:3].abs().max()))
    tc, tw = (g.table() for g in logs)   # columns: forces.StressLog.COLUMNS
    U, sxy = tc[:,2] + tw[:,2], tc[:,4] + tw[:,4]
    assert np.isfinite(U).all() and np.isfinite(sxy).all()
    print('   ', len(tc), 'samples, steps', int(tc[0,0]), '-', int(tc[-1,0]), ' <U> %.6g (core %.6g, well %.6g)  <sigma_xy> %.6g  sigma_xy(last) %.6g at xy %.4f  pairs(last) core %d well %d'
          % (U.mean(), tc[:,2].mean(), tw[:,2].mean(), sxy.mean(), sxy[-1], tc[-1,1], int(tc[-1,9]), int(tw[-1,9])))
torch.cuda.synchronize(); print('500 steps in %.2f s' % (time.time()-t0))
