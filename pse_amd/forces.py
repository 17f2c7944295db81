"""Force providers: what fills `net_force` before the integrator consumes it (HOOMD's force computes in the reference,
PSEv1/Stokes.cc:447; its example script has none).  SURVEY.md 8 f4: the step either side of the hot path, kept minimal."""


class HarmonicRepulsion:
    """F_i = sum_j k (sigma - r)(r_i - r_j)/r for minimum-image pairs with r < sigma (sigma = 2a: contact of unit spheres).
    Evaluated on the integrator's own cell list; sigma must not exceed the hydrodynamic real-space cutoff.

    virial=True: compute() makes the fused call (pse_pair_repulsion_virial) instead -- the same forces, plus the potential energy
    and the virial of the same pass in eight device doubles.  `energy`, `virial` and `stress()` copy them to the host when they are
    read (that waits for the stream); a StressLog samples them without any wait."""

    def __init__(self, integrator, k, sigma=2.0, virial=False):
        self.integrator, self.k, self.sigma = integrator, float(k), float(sigma)
        self._fused = bool(virial)
        self._own = None     # where a fused call writes when no log takes the sample
        self._obs = None     # the eight device doubles of the most recent fused call: U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs
        self.log = None      # a StressLog registers itself here
        integrator.system.forces.append(self)

    def compute(self, timestep):
        s, g = self.integrator.system, self.integrator.group
        m = g.members
        if not self._fused:
            self.integrator.cpp_method.pairRepulsion(s.pos.data_ptr(), s.net_force.data_ptr(), 0 if m is None else m.data_ptr(),
                                                     len(g), self.k, self.sigma, True)
            return
        out = self.log.row(timestep) if self.log is not None else None
        if out is None:
            if self._own is None:
                import torch
                self._own = torch.zeros(8, dtype=torch.float64, device=s.pos.device)
            out = self._own
        self.integrator.cpp_method.pairRepulsionVirial(s.pos.data_ptr(), s.net_force.data_ptr(), 0 if m is None else m.data_ptr(),
                                                       len(g), self.k, self.sigma, True, out.data_ptr())
        self._obs = out

    def _observables(self):
        if self._obs is None:
            raise RuntimeError("no observables yet: HarmonicRepulsion(..., virial=True) and one compute() first")
        return self._obs.cpu().numpy()

    @property
    def energy(self):
        """U = sum over pairs of k/2 (sigma - r)^2 at the most recent compute()."""
        return float(self._observables()[0])

    @property
    def npairs(self):
        return int(self._observables()[7])

    @property
    def virial(self):
        """W_ab = sum_{i<j} (r_i - r_j)_a F_ij,b (F_ij: force on i from j) at the most recent compute(): 3 x 3, symmetric."""
        return _sym3(self._observables()[1:7])

    def stress(self):
        """Particle stress -W / V, V = Lx Ly Lz of the system's current box."""
        Lx, Ly, Lz, _ = self.integrator.system.box
        return -self.virial / (Lx * Ly * Lz)


def _sym3(w):
    import numpy as np
    xx, xy, xz, yy, yz, zz = (float(v) for v in w)
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


class StressLog:
    """Energy and stress of a HarmonicRepulsion(..., virial=True) every `period` steps, in a device ring of `capacity` rows: on a
    sample step the provider's fused call writes its eight doubles straight into the next row, the step number, the box tilt and the
    volume are noted on the host, and nothing waits for the device until table() is read.  Once full, the oldest rows are replaced."""

    COLUMNS = ("timestep", "xy", "U", "sxx", "sxy", "sxz", "syy", "syz", "szz", "npairs")

    def __init__(self, provider, period, capacity):
        import torch
        if not getattr(provider, "_fused", False):
            raise ValueError("StressLog needs a HarmonicRepulsion(..., virial=True)")
        if int(period) < 1 or int(capacity) < 1:
            raise ValueError("period and capacity must be positive")
        self.provider, self.period, self.capacity = provider, int(period), int(capacity)
        self.rows = torch.zeros((self.capacity, 8), dtype=torch.float64, device=provider.integrator.system.pos.device)
        self._host = [None] * self.capacity    # (timestep, xy, volume) of each row
        self.count = 0                         # samples taken so far
        provider.log = self

    def row(self, timestep):
        """The row the provider's call of this step writes, or None when the step is not a sample."""
        if timestep % self.period:
            return None
        Lx, Ly, Lz, xy = self.provider.integrator.system.box
        q = self.count % self.capacity
        self._host[q] = (int(timestep), float(xy), Lx * Ly * Lz)
        self.count += 1
        return self.rows[q]

    def table(self):
        """(samples, 10) NumPy array, oldest first: timestep, xy, U, sigma_xx, xy, xz, yy, yz, zz, npairs (one copy from the device)."""
        import numpy as np
        n = min(self.count, self.capacity)
        dev = self.rows.cpu().numpy()
        out = np.zeros((n, len(self.COLUMNS)))
        for r in range(n):
            q = (self.count - n + r) % self.capacity
            t, xy, vol = self._host[q]
            out[r, 0], out[r, 1], out[r, 2] = t, xy, dev[q, 0]
            out[r, 3:9] = -dev[q, 1:7] / vol
            out[r, 9] = dev[q, 7]
        return out


class ConstantForce:
    """The same force on every particle of the group (gravity / sedimentation); its mean is what the k = 0 mode drops."""

    def __init__(self, system, fx=0.0, fy=0.0, fz=0.0):
        import torch
        self.system = system
        self.f = torch.tensor([fx, fy, fz, 0.0], dtype=torch.float64, device="cuda")
        system.forces.append(self)

    def compute(self, timestep):
        self.system.net_force += self.f
