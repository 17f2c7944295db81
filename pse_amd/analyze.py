"""Structure analyzers: what is measured from the positions during a run, next to the path.  RDF samples the pair-distance histogram
of the integrator's engine (pse_pair_hist_accumulate: one walk of the cell list the step uses anyway) into a device tensor and turns
the counts into the radial distribution functions g_ab(r) and coordination numbers when they are read.  StructureFactor is the other
half of how structure is reported: the densities rho_a(k) on the reciprocal lattice of the (tilted) box, summed directly and exactly
on the device (pse_structure_factor_accumulate), and their products S_ab(k) -- at any k the box admits, far below 2 pi / rcut, and
resolved in direction."""
import math

from .engine import (SF_MAX_MODES, PairHistogram, StructureFactorModes, _pair_hist_arguments, _structure_factor_arguments,
                     pair_type_index)
from .forces import _excl_list


def _rdf_arguments(nbins, rmax, rmin, types, type_names, period):
    """What RDF checks before it touches the device: `types` as integers -- a name is its position in `type_names` --, the number of
    types, the bins and the period.  Returns (types uint32 or None, ntypes, nbins, rmin, rmax, names or None, period)."""
    names = None if type_names is None else list(type_names)
    if names is not None and (not names or len(set(names)) != len(names) or not all(isinstance(v, str) for v in names)):
        raise ValueError("type_names must be distinct strings")
    if int(period) < 1:
        raise ValueError("period must be positive")
    if types is None:
        if names is not None and len(names) != 1:
            raise ValueError("type_names without types: there is one type")
        ntypes = 1
    else:
        import numpy as np
        types = np.asarray(_type_codes(types.tolist() if hasattr(types, "tolist") else list(types), names))
        if types.ndim != 1 or types.shape[0] == 0 or not np.issubdtype(types.dtype, np.integer) or types.min() < 0:
            raise ValueError("types must be a non-empty 1-D sequence of non-negative integers or names, one per particle")
        ntypes = max(int(types.max()) + 1, len(names or ()))
    return _pair_hist_arguments(types, ntypes, nbins, rmin, rmax) + (names, int(period))


def _typed_arguments(types, type_names, period):
    """The part of _rdf_arguments that knows no bins: (types as an integer array or None, ntypes, names or None, period)."""
    types, ntypes, _, _, _, names, period = _rdf_arguments(1, 1.0, 0.0, types, type_names, period)
    return types, ntypes, names, period


def _type_codes(values, names):
    """`values` with every name replaced by its position in `names`."""
    out = []
    for v in values:
        if isinstance(v, str):
            if names is None:
                raise ValueError(f"type name {v!r}: names need a type_names= list")
            if v not in names:
                raise ValueError(f"unknown type name {v!r}: type_names is {names}")
            v = names.index(v)
        out.append(v)
    return out


def bin_edges(nbins, rmin, rmax):
    """The nbins + 1 edges of the uniform bins: bin b covers [edges[b], edges[b + 1])."""
    import numpy as np
    return rmin + np.arange(nbins + 1) * ((rmax - rmin) / nbins)


def pair_counts(type_counts):
    """P[p] = the number of unordered particle pairs of pair type p for N_a particles of type a: N_a (N_a - 1)/2 and N_a N_b."""
    import numpy as np
    nt = len(type_counts)
    P = np.zeros(nt * (nt + 1) // 2)
    for a in range(nt):
        for b in range(a, nt):
            na, nb = float(type_counts[a]), float(type_counts[b])
            P[pair_type_index(a, b, nt)] = 0.5 * na * (na - 1.0) if a == b else na * nb
    return P


def g_of_counts(counts, samples, type_counts, edges, volume):
    """g[p, b] = counts / (samples P_p V_shell(b) / V): the counts over what an ideal gas of the same composition gives.  A pair type
    without pairs (P_p = 0) gives zeros.  NumPy only."""
    import numpy as np
    counts, edges = np.asarray(counts, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    if samples < 1:
        raise ValueError("no samples yet")
    shell = 4.0 * math.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    ideal = samples * pair_counts(type_counts)[:, None] * shell[None, :] / volume
    return np.divide(counts, ideal, out=np.zeros_like(counts), where=ideal > 0.0)


def edge_index(edges, r):
    """k with edges[k] == r to 1e-12 relative; ValueError if r is not a bin edge."""
    import numpy as np
    edges = np.asarray(edges, dtype=np.float64)
    k = int(np.abs(edges - r).argmin())
    if not abs(edges[k] - r) <= 1e-12 * max(1.0, abs(r)):
        raise ValueError(f"r = {r} is not a bin edge: the nearest one is {edges[k]:.12g}")
    return k


def coordination_of_counts(counts, samples, type_counts, a, b, edges, r):
    """The mean number of b partners of an a particle within r: the a-b pairs below r per sample, over N_a; twice that for a == b
    (a pair gives each of its two members a partner).  r must be a bin edge (to 1e-12 relative)."""
    import numpy as np
    k = edge_index(edges, r)
    if samples < 1:
        raise ValueError("no samples yet")
    if type_counts[a] == 0:
        raise ValueError(f"there is no particle of type {a}")
    nt = len(type_counts)
    pairs = float(np.asarray(counts)[pair_type_index(a, b, nt), :k].sum()) / samples
    return (2.0 if a == b else 1.0) * pairs / float(type_counts[a])


class RDF:
    """Radial distribution functions of a run: every `period` steps the distances of all pairs of the integrator's group below `rmax`
    are binned on the device (pse_pair_hist_accumulate), one row of `nbins` uniform bins on [rmin, rmax) per pair of types, into an
    int64 CUDA tensor of this object.  Sampling only queues work; the readers below are the only places that wait for the device.
    rmax may not exceed the hydrodynamic real-space cutoff (5.26 at xi = 0.5, error = 1e-3: the first and second shell of unit-radius
    beads).  `types`: one per particle of the system, integers or names with a `type_names=` list, whose order numbers them; None: one
    type.  At most 8 types and 8192 counters (pair types x bins).  exclusions: a forces.Exclusions whose pairs are not counted.

    counts -- (npt, nbins) int64;  edges, r -- bin edges and centres;  counts_of(a, b);  g(a, b) or g() for all pair types;
    coordination(a, b, r);  samples;  reset()."""

    def __init__(self, integrator, nbins, rmax, rmin=0.0, types=None, type_names=None, exclusions=None, period=1):
        import numpy as np
        import torch
        types, self.ntypes, self.nbins, self.rmin, self.rmax, self.type_names, self.period = _rdf_arguments(
            nbins, rmax, rmin, types, type_names, period)   # (raises before the device is touched)
        system = integrator.system
        if types is not None and types.shape[0] != system.n:
            raise ValueError(f"types has {types.shape[0]} entries, the system {system.n} particles")
        self.integrator, self.system = integrator, system
        self.types = np.zeros(system.n, dtype=np.uint32) if types is None else types
        self._excl = _excl_list(integrator, exclusions)
        self._hist = PairHistogram(integrator.engine, types, self.ntypes, self.nbins, self.rmin, self.rmax, system.n)
        self.npt = self._hist.npt
        self._counts = torch.zeros((self.npt, self.nbins), dtype=torch.int64, device=system.pos.device)
        self.samples = 0
        self._volume = 0.0      # the sum of the box volumes of the samples
        system.analyzers.append(self)

    def analyze(self, timestep):
        if timestep % self.period:
            return
        s = self.system
        self.integrator.engine.pair_hist_accumulate(s.pos, self._hist, self._counts, group=self.integrator.group.members,
                                                    exclusions=self._excl)
        self.samples += 1
        self._volume += s.box[0] * s.box[1] * s.box[2]

    def reset(self):
        self._counts.zero_()
        self.samples, self._volume = 0, 0.0

    def _code(self, v):
        v = _type_codes([v], self.type_names)[0]
        if not 0 <= int(v) < self.ntypes:
            raise ValueError(f"type {v} outside [0, {self.ntypes})")
        return int(v)

    def _type_counts(self):
        """N_a among the members of the integrator's group."""
        import numpy as np
        m = self.integrator.group.members
        t = self.types if m is None else self.types[m.cpu().numpy()]
        return np.bincount(t, minlength=self.ntypes)

    @property
    def counts(self):
        return self._counts.cpu().numpy()

    @property
    def edges(self):
        return bin_edges(self.nbins, self.rmin, self.rmax)

    @property
    def r(self):
        e = self.edges
        return 0.5 * (e[:-1] + e[1:])

    def counts_of(self, a, b):
        return self.counts[pair_type_index(self._code(a), self._code(b), self.ntypes)]

    def g(self, a=None, b=None):
        """g_ab at the bin centres, (nbins,); without arguments all pair types, (npt, nbins).  V is the mean volume of the samples."""
        if (a is None) != (b is None):
            raise ValueError("g() takes both types or neither")
        if self.samples < 1:
            raise ValueError("no samples yet")
        g = g_of_counts(self.counts, self.samples, self._type_counts(), self.edges, self._volume / self.samples)
        return g if a is None else g[pair_type_index(self._code(a), self._code(b), self.ntypes)]

    def coordination(self, a, b, r):
        """The mean number of `b` partners of an `a` particle within r; r must be a bin edge (ValueError otherwise)."""
        a, b = self._code(a), self._code(b)   # (and the bin edge: checked before the device is read)
        edges = self.edges
        edge_index(edges, r)
        return coordination_of_counts(self.counts, self.samples, self._type_counts(), a, b, edges, r)


def k_vectors(modes, box):
    """The wave vectors (nk, 3) of the integer modes (mx, my, mz) in the box (Lx, Ly, Lz[, xy]): k = 2 pi (mx/Lx, my/Ly - xy mx/Lx,
    mz/Lz), so that k.r = 2 pi m.s with s the fractional coordinates ((x - xy y)/Lx, y/Ly, z/Lz)."""
    import numpy as np
    m = np.asarray(modes, dtype=np.float64).reshape(-1, 3)
    Lx, Ly, Lz = float(box[0]), float(box[1]), float(box[2])
    xy = float(box[3]) if len(box) > 3 else 0.0
    return 2.0 * math.pi * np.stack([m[:, 0] / Lx, m[:, 1] / Ly - xy * m[:, 0] / Lx, m[:, 2] / Lz], axis=1)


def axis_modes(mmax):
    """The 3 mmax modes (m, 0, 0), (0, m, 0), (0, 0, m), m = 1..mmax: three lines through the origin, int32 (3 mmax, 3)."""
    import numpy as np
    if int(mmax) < 1:
        raise ValueError("mmax must be positive")
    out = np.zeros((3, int(mmax), 3), dtype=np.int32)
    for c in range(3):
        out[c, :, c] = np.arange(1, int(mmax) + 1)
    return out.reshape(-1, 3)


def modes_within(box, kmax):
    """Every mode with 0 < |k| <= kmax of the box at tilt 0, one of each pair +-m: the half space whose first non-zero component is
    positive, int32 (nk, 3) in ascending (mx, my, mz).  ValueError above 32768 modes (the limit of one object)."""
    import numpy as np
    L = np.array([float(box[0]), float(box[1]), float(box[2])])
    if not (kmax > 0.0 and np.all(L > 0.0)):
        raise ValueError("need kmax > 0 and positive box lengths")
    top = np.floor(kmax * L / (2.0 * math.pi) * (1.0 + 1e-12)).astype(np.int64)
    if 0.5 * np.prod(2.0 * top + 1.0) > 64.0 * SF_MAX_MODES:   # (the bounding block alone is far beyond the limit)
        raise ValueError(f"kmax = {kmax} admits more than {SF_MAX_MODES} modes in this box")
    gx, gy, gz = np.meshgrid(np.arange(0, top[0] + 1), np.arange(-top[1], top[1] + 1), np.arange(-top[2], top[2] + 1), indexing="ij")
    m = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    half = (m[:, 0] > 0) | ((m[:, 0] == 0) & ((m[:, 1] > 0) | ((m[:, 1] == 0) & (m[:, 2] > 0))))
    m = m[half]
    m = m[np.linalg.norm(k_vectors(m, tuple(L)), axis=1) <= kmax]
    if m.shape[0] > SF_MAX_MODES:
        raise ValueError(f"kmax = {kmax} admits {m.shape[0]} modes in this box, more than {SF_MAX_MODES}")
    return np.ascontiguousarray(m, dtype=np.int32)


def S_of_sums(sums, samples, type_counts, a=None, b=None):
    """The structure factors of accumulated sums[p, q] = sum over the samples of Re(rho_a conj rho_b): with both types
    S_ab = sums[p(a, b)] / (samples sqrt(N_a N_b)); with neither the total S = (sum_a sums[p(a, a)] + 2 sum_{a<b} sums[p(a, b)]) /
    (samples N), N the sum of type_counts.  NumPy only."""
    import numpy as np
    sums = np.asarray(sums, dtype=np.float64)
    nt = len(type_counts)
    if (a is None) != (b is None):
        raise ValueError("S() takes both types or neither")
    if samples < 1:
        raise ValueError("no samples yet")
    if a is not None:
        if type_counts[a] == 0 or type_counts[b] == 0:
            raise ValueError(f"there is no particle of type {a if type_counts[a] == 0 else b}")
        return sums[pair_type_index(a, b, nt)] / (samples * math.sqrt(float(type_counts[a]) * float(type_counts[b])))
    total = np.zeros(sums.shape[1])
    for i in range(nt):
        for j in range(i, nt):
            total += (1.0 if i == j else 2.0) * sums[pair_type_index(i, j, nt)]
    return total / (samples * float(np.sum(type_counts)))


def shell_average_of(k, values, nbins, kmax=None):
    """The mean of values[q] over nbins uniform bins of |k_q| on [0, kmax] (default: the largest |k|; modes beyond kmax are left out):
    (bin centres, means, counts), nan where a bin holds no mode."""
    import numpy as np
    kn, values = np.linalg.norm(np.asarray(k, dtype=np.float64), axis=1), np.asarray(values, dtype=np.float64)
    if int(nbins) < 1:
        raise ValueError("nbins must be positive")
    kmax = float(kn.max()) if kmax is None else float(kmax)
    if not kmax > 0.0:
        raise ValueError("kmax must be positive")
    w = kmax / int(nbins)
    idx = np.minimum((kn / w).astype(np.int64), int(nbins) - 1)
    keep = kn <= kmax
    cnt = np.bincount(idx[keep], minlength=int(nbins))
    tot = np.bincount(idx[keep], weights=values[keep], minlength=int(nbins))
    return (np.arange(int(nbins)) + 0.5) * w, np.divide(tot, cnt, out=np.full(int(nbins), np.nan), where=cnt > 0), cnt


def _structure_factor_analyzer_arguments(modes, types, type_names, period):
    """What StructureFactor checks before it touches the device.  Returns (types uint32 or None, ntypes, modes int32 (nk, 3), names or
    None, period)."""
    types, ntypes, names, period = _typed_arguments(types, type_names, period)
    types, ntypes, modes = _structure_factor_arguments(types, ntypes, modes)
    return types, ntypes, modes, names, period


class StructureFactor:
    """Static structure factors of a run: every `period` steps the densities rho_a(m) = sum_{j of type a} exp(-2 pi i m.s_j) of the
    integrator's group are summed on the device (pse_structure_factor_accumulate) for the integer modes `modes` (nk, 3) of the
    reciprocal lattice of the box AS IT IS at that step, and Re(rho_a conj rho_b) is added to a float64 CUDA tensor of this object,
    one row per pair of types.  Sampling only queues work; the readers below are the only places that wait for the device.
    `types`, `type_names`: as for RDF; at most 8 types, 32768 modes, |m_i| <= 4096.  The box of every sample is recorded (`boxes`).
    Under shear the box tilts from step to step: the sums are kept per INTEGER mode, whose wave vector k = 2 pi (mx/Lx, my/Ly -
    xy mx/Lx, mz/Lz) moves with the tilt.  `k` and `shell_average` therefore raise ValueError when the samples' boxes differ: sample
    at a period over which the tilt repeats (a Lees-Edwards box returns to itself once per unit of strain), or read `sums` per mode.

    sums -- (npt, nk) float64;  samples;  reset();  S(a, b) = sums / (samples sqrt(N_a N_b)), S() the total (sum_a |rho_a|^2 +
    2 sum_{a<b} Re rho_a rho_b*) / (samples N);  k -- (nk, 3);  shell_average(nbins, kmax=None[, a, b]) -- the mean of S over bins
    of |k|: (centres, means, counts);  density() -- (ntypes, nk) complex, the rho of one fresh call on the current positions."""

    def __init__(self, integrator, modes, types=None, type_names=None, period=1):
        import numpy as np
        import torch
        types, self.ntypes, self.modes, self.type_names, self.period = _structure_factor_analyzer_arguments(
            modes, types, type_names, period)   # (raises before the device is touched)
        system = integrator.system
        if types is not None and types.shape[0] != system.n:
            raise ValueError(f"types has {types.shape[0]} entries, the system {system.n} particles")
        self.integrator, self.system = integrator, system
        self.types = np.zeros(system.n, dtype=np.uint32) if types is None else types
        self._sf = StructureFactorModes(integrator.engine, types, self.ntypes, self.modes, system.n)
        self.npt, self.nk = self._sf.npt, self._sf.nk
        self._sums = torch.zeros((self.npt, self.nk), dtype=torch.float64, device=system.pos.device)
        self.samples, self.boxes = 0, []
        system.analyzers.append(self)

    def analyze(self, timestep):
        if timestep % self.period:
            return
        s = self.system
        self.integrator.engine.structure_factor_accumulate(s.pos, self._sf, sums=self._sums, group=self.integrator.group.members)
        self.samples += 1
        self.boxes.append(tuple(s.box))

    def reset(self):
        self._sums.zero_()
        self.samples, self.boxes = 0, []

    _code = RDF._code
    _type_counts = RDF._type_counts

    @property
    def sums(self):
        return self._sums.cpu().numpy()

    def density(self):
        import torch
        s = self.system
        rho = torch.empty((self.ntypes, self.nk, 2), dtype=torch.float64, device=s.pos.device)
        self.integrator.engine.structure_factor_accumulate(s.pos, self._sf, rho=rho, group=self.integrator.group.members)
        r = rho.cpu().numpy()
        return r[..., 0] + 1j * r[..., 1]

    def S(self, a=None, b=None):
        """S_ab per mode, (nk,); without arguments the total S."""
        if (a is None) != (b is None):
            raise ValueError("S() takes both types or neither")
        if self.samples < 1:
            raise ValueError("no samples yet")
        if a is not None:
            a, b = self._code(a), self._code(b)
        return S_of_sums(self.sums, self.samples, self._type_counts(), a, b)

    def _box(self):
        if not self.boxes:
            raise ValueError("no samples yet")
        if any(bx != self.boxes[0] for bx in self.boxes):
            raise ValueError("the boxes of the samples differ (a tilting box): the sums are per integer mode, there is no one k; sample "
                             "at a period over which the tilt repeats")
        return self.boxes[0]

    @property
    def k(self):
        return k_vectors(self.modes, self._box())

    def shell_average(self, nbins, kmax=None, a=None, b=None):
        k = self.k   # (the differing-box check comes first)
        return shell_average_of(k, self.S(a, b), nbins, kmax)
