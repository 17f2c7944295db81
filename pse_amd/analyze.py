"""Structure analyzers: what is measured from the positions during a run, next to the path.  RDF samples the pair-distance histogram
of the integrator's engine (pse_pair_hist_accumulate: one walk of the cell list the step uses anyway) into a device tensor and turns
the counts into the radial distribution functions g_ab(r) and coordination numbers when they are read.  StructureFactor is the other
half of how structure is reported: the densities rho_a(k) on the reciprocal lattice of the (tilted) box, summed directly and exactly
on the device (pse_structure_factor_accumulate), and their products S_ab(k) -- at any k the box admits, far below 2 pi / rcut, and
resolved in direction.  MSD is the dynamic counterpart: the engine keeps up to 64 time origins of unwrapped positions
(pse_msd_store) and one streaming pass per sample sums the first, second and fourth moments of the displacement per type and per
origin (pse_msd_accumulate): the drift, the mean-squared displacement tensor and the non-Gaussian parameter over many time origins.
Clusters says which particles hang together: the connected components of a distance criterion, labelled on the device by a union-find
over the sorted rows (pse_clusters_label), with the number of clusters, the largest one and the size distribution n(s) per sample.
BondOrder says whether a neighbourhood is ordered: the Steinhardt q_l, the neighbour-averaged q-bar_l and the solid-like bonds of
every particle (pse_bond_order_compute: spherical harmonics up to degree 12 summed over the neighbours on the cell list), with their
per-type distributions and the solid-like fraction per sample.
Conformations measures the molecules that a bond topology defines: every molecule unfolded along its own bonds in the box of the
step, its gyration tensor, Rg^2 and end-to-end vector reduced on the device (pse_molecules_compute: pointer jumping and fixed-order
trees in LDS, one workgroup per tile of molecules), per-type sums, a ring of per-sample sums and the histograms of Rg and |R|.
RouseModes is their dynamic counterpart: the normal modes X_p and the end-to-end vector of every linear chain in the same unfolded
coordinates (pse_chain_modes_compute), kept for up to 64 time origins on the device (pse_chain_modes_store) and correlated with them
per type and mode (pse_chain_modes_correlate): amplitudes, <X_p(t) X_p(0)> and the relaxation times tau_p.
IntermediateScattering is the dynamic counterpart of StructureFactor: the self part F_s(k, t) and the collective part F(k, t) of the
density correlations over up to 64 time origins (pse_isf_sample, pse_isf_store, pse_isf_correlate), on the integer modes of the box."""
import contextlib
import math

from .engine import (BOND_ORDER_MAX_COUNTERS, MSD_MAX_ORIGINS, MSD_MOMENTS, SF_MAX_MODES, BondOrderShells, ClusterLinks, DisplacementOrigins,
                     PairHistogram, ScatteringOrigins, StructureFactorModes, _bond_order_arguments, _cluster_arguments, _isf_arguments,
                     _msd_arguments, _ntypes_argument, _pair_hist_arguments, _structure_factor_arguments, _types_argument, pair_type_index)
from .forces import _excl_list


def _typed_arguments(types, type_names, period):
    """What every analyzer checks first, before it touches the device: `types` as integers -- a name is its position in `type_names`
    --, the number of types and the period.  Returns (types uint32 or None, ntypes, names or None, period)."""
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
    ntypes = _ntypes_argument(ntypes)
    return _types_argument(types, ntypes), ntypes, names, int(period)


def _rdf_arguments(nbins, rmax, rmin, types, type_names, period):
    """_typed_arguments and the bins of RDF.  Returns (types uint32 or None, ntypes, nbins, rmin, rmax, names or None, period)."""
    types, ntypes, names, period = _typed_arguments(types, type_names, period)
    return _pair_hist_arguments(types, ntypes, nbins, rmin, rmax) + (names, period)


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


def _pair_dict_codes(r, names, word):
    """A dict {(a, b): r} over pairs of types, whose keys may name their types by `names`, with integer keys (a <= b); anything but a
    dict comes back as it is.  `word`: what the messages call the distances."""
    if not isinstance(r, dict):
        return r
    coded = {}
    for key, v in r.items():
        if not (isinstance(key, tuple) and len(key) == 2):
            raise ValueError(f"{word} key {key!r}: need a pair (a, b) of types")
        coded.setdefault(tuple(sorted(_type_codes(list(key), names))), []).append(v)
    if any(len(v) > 1 for v in coded.values()):
        raise ValueError(f"{word} names a pair of types twice")
    return {k: v[0] for k, v in coded.items()}


class _TypedAnalyzer:
    """What the analyzers share: one type per particle of the system (`types`, `ntypes`, `type_names`), a `period`, a count of
    `samples`, and their place in system.analyzers."""

    @contextlib.contextmanager
    def _attach(self, integrator, types):
        """Around the rest of __init__: refuses `types` of another length than the system first, and registers the analyzer with
        the system last -- only when the block, which makes the device object, has not raised.  Yields the system."""
        import numpy as np
        system = integrator.system
        if types is not None and types.shape[0] != system.n:
            raise ValueError(f"types has {types.shape[0]} entries, the system {system.n} particles")
        self.integrator, self.system = integrator, system
        self.types = np.zeros(system.n, dtype=np.uint32) if types is None else types
        yield system
        system.analyzers.append(self)

    def _due(self, timestep):
        return timestep % self.period == 0

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

    def _sampled(self):
        if self.samples < 1:
            raise ValueError("no samples yet")


class _SampleRing:
    """The ring of per-sample rows that Clusters and BondOrder keep: `_rows`, a device tensor of `capacity` rows that the sample
    writes its slot of, and the timestep of every slot on the host.  Once full, the oldest rows are replaced."""

    def _ring_reset(self):
        self._steps = [None] * self.capacity
        self.samples = 0

    def _slot(self):
        """Where this sample's row goes."""
        return self.samples % self.capacity

    def _record(self, slot, timestep):
        self._steps[slot] = int(timestep)
        self.samples += 1

    def table(self):
        """(samples kept, 1 + the words of a row) int64, oldest first: the timestep, then the sample's row (one copy from the device)."""
        import numpy as np
        n = min(self.samples, self.capacity)
        dev = self._rows.cpu().numpy().reshape(self.capacity, -1)
        out = np.zeros((n, 1 + dev.shape[1]), dtype=np.int64)
        for r in range(n):
            q = (self.samples - n + r) % self.capacity
            out[r, 0], out[r, 1:] = self._steps[q], dev[q]
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


class RDF(_TypedAnalyzer):
    """Radial distribution functions of a run: every `period` steps the distances of all pairs of the integrator's group below `rmax`
    are binned on the device (pse_pair_hist_accumulate), one row of `nbins` uniform bins on [rmin, rmax) per pair of types, into an
    int64 CUDA tensor of this object.  Sampling only queues work; the readers below are the only places that wait for the device.
    rmax may not exceed the hydrodynamic real-space cutoff (5.26 at xi = 0.5, error = 1e-3: the first and second shell of unit-radius
    beads).  `types`: one per particle of the system, integers or names with a `type_names=` list, whose order numbers them; None: one
    type.  At most 8 types and 8192 counters (pair types x bins).  exclusions: a forces.Exclusions whose pairs are not counted.

    counts -- (npt, nbins) int64;  edges, r -- bin edges and centres;  counts_of(a, b);  g(a, b) or g() for all pair types;
    coordination(a, b, r);  samples;  reset()."""

    def __init__(self, integrator, nbins, rmax, rmin=0.0, types=None, type_names=None, exclusions=None, period=1):
        import torch
        types, self.ntypes, self.nbins, self.rmin, self.rmax, self.type_names, self.period = _rdf_arguments(
            nbins, rmax, rmin, types, type_names, period)   # (raises before the device is touched)
        with self._attach(integrator, types) as system:
            self._excl = _excl_list(integrator, exclusions)
            self._hist = PairHistogram(integrator.engine, types, self.ntypes, self.nbins, self.rmin, self.rmax, system.n)
            self.npt = self._hist.npt
            self._counts = torch.zeros((self.npt, self.nbins), dtype=torch.int64, device=system.pos.device)
            self.samples = 0
            self._volume = 0.0      # the sum of the box volumes of the samples

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        s = self.system
        self.integrator.engine.pair_hist_accumulate(s.pos, self._hist, self._counts, group=self.integrator.group.members,
                                                    exclusions=self._excl)
        self.samples += 1
        self._volume += s.box[0] * s.box[1] * s.box[2]

    def reset(self):
        self._counts.zero_()
        self.samples, self._volume = 0, 0.0

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
        self._sampled()
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


class StructureFactor(_TypedAnalyzer):
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
        import torch
        types, self.ntypes, self.modes, self.type_names, self.period = _structure_factor_analyzer_arguments(
            modes, types, type_names, period)   # (raises before the device is touched)
        with self._attach(integrator, types) as system:
            self._sf = StructureFactorModes(integrator.engine, types, self.ntypes, self.modes, system.n)
            self.npt, self.nk = self._sf.npt, self._sf.nk
            self._sums = torch.zeros((self.npt, self.nk), dtype=torch.float64, device=system.pos.device)
            self.samples, self.boxes = 0, []

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        s = self.system
        self.integrator.engine.structure_factor_accumulate(s.pos, self._sf, sums=self._sums, group=self.integrator.group.members)
        self.samples += 1
        self.boxes.append(tuple(s.box))

    def reset(self):
        self._sums.zero_()
        self.samples, self.boxes = 0, []

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
        self._sampled()
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


def unwrap(pos, image, box, strain):
    """The unwrapped positions (N, 3) of wrapped positions `pos` (N, >= 3) with images `image` (N, 3) in the box (Lx, Ly, Lz[, xy]):
    x + ix Lx + iy strain Ly, y + iy Ly, z + iz Lz.  `strain` is the ACCUMULATED tilt -- the box's xy plus the lattice vectors that
    Lees-Edwards flips have taken off it so far (System.strain) -- and stands where xy would: with the current xy the result jumps by
    iy Lx at every flip; with the strain it is the same point before and after a flip, through every re-wrap behind a changed tilt,
    every x and z wrap and every y wrap before the first flip.  LIMIT: a y image gained AFTER a flip shifts x_u by flips Ly (the
    step's wrap takes xy Ly, the current tilt, off x; the formula adds strain Ly): x_u of a sheared run is right only while no
    particle gains a y image after a flip; y_u and z_u are always right.
    NumPy only; the device restates it (pse_msd_store), with the same order of operations up to the fused roundings."""
    import numpy as np
    pos, image = np.asarray(pos, dtype=np.float64), np.asarray(image)
    Lx, Ly, Lz = float(box[0]), float(box[1]), float(box[2])
    sLy = float(strain) * Ly
    out = np.empty((pos.shape[0], 3))
    out[:, 0] = image[:, 1] * sLy + (image[:, 0] * Lx + pos[:, 0])
    out[:, 1] = image[:, 1] * Ly + pos[:, 1]
    out[:, 2] = image[:, 2] * Lz + pos[:, 2]
    return out


class MSDSchedule:
    """Which origins an MSD sample is taken against and where the next origin goes; integers only.  Sample s = 0, 1, ... (1) is
    accumulated against every origin j = 0, 1, ... with 1 <= s - j origin_every <= nlags, into row lag - 1, and then (2), if s is a
    multiple of origin_every, is stored as origin s / origin_every in slot (s / origin_every) % norigins, norigins =
    ceil(nlags / origin_every): a slot is overwritten only after its origin's lag nlags has been taken.  `counts[lag - 1]`: the origins
    that lag has been taken against so far; `live[slot]`: the sample stored in that slot since the last reset().  drop_origins():
    the origins stored so far are no longer paired with later samples (their slots leave `live`); sums and counts stay."""

    def __init__(self, nlags, origin_every=1):
        self.nlags, self.origin_every = int(nlags), int(origin_every)
        if self.nlags < 1 or self.origin_every < 1:
            raise ValueError("nlags and origin_every must be positive")
        self.norigins = -(-self.nlags // self.origin_every)
        if self.norigins > MSD_MAX_ORIGINS:
            raise ValueError(f"nlags / origin_every = {self.nlags} / {self.origin_every} needs {self.norigins} origins, more than "
                             f"{MSD_MAX_ORIGINS}")
        self.reset()

    def reset(self):
        self.samples, self.counts, self.live, self._first = 0, [0] * self.nlags, {}, 0

    def drop_origins(self):
        """Every origin older than the next sample is no longer paired: the next sample, if it is an origin, is the oldest one."""
        self._first = -(-self.samples // self.origin_every)  # the smallest j with j oe >= samples
        self.live = {}

    def pairs(self, s=None):
        """[(slot, row)] of sample s (default: the next one), oldest origin first."""
        s = self.samples if s is None else int(s)
        oe = self.origin_every
        first = max(self._first, -(-(s - self.nlags) // oe))   # the smallest j with s - j oe <= nlags that was not dropped
        last = (s - 1) // oe if s >= 1 else -1               # the largest j with s - j oe >= 1
        return [(j % self.norigins, s - j * oe - 1) for j in range(first, last + 1)]

    def sample(self, accumulate, store):
        """One sample: accumulate(slots, rows) if there is a live origin, then store(slot) if this sample is an origin."""
        s, pairs = self.samples, self.pairs()
        if pairs:
            accumulate([p[0] for p in pairs], [p[1] for p in pairs])
            for _, row in pairs:
                self.counts[row] += 1
        if s % self.origin_every == 0:
            store((s // self.origin_every) % self.norigins)
            self.live[(s // self.origin_every) % self.norigins] = s
        self.samples = s + 1

    def slot_of_lag(self, lag):
        """The slot of the origin that was `lag` samples old at the last sample; ValueError if there is none."""
        s = self.samples - 1
        j, rem = divmod(s - int(lag), self.origin_every)
        if s < 0 or not 1 <= int(lag) <= self.nlags or rem or j < 0:
            raise ValueError(f"no live origin {lag} samples before the last sample")
        return j % self.norigins


def _msd_analyzer_arguments(nlags, origin_every, types, type_names, period):
    """What MSD checks before it touches the device.  Returns (schedule, types uint32 or None, ntypes, names or None, period)."""
    schedule = MSDSchedule(nlags, origin_every)
    types, ntypes, names, period = _typed_arguments(types, type_names, period)
    types, ntypes, _ = _msd_arguments(types, ntypes, schedule.norigins)
    return schedule, types, ntypes, names, period


def moments_of_sums(sums, counts, type_counts, a=None):
    """The mean moments per lag of accumulated sums (nlags, ntypes, 10): sums[:, a] / (counts N_a), or with a = None those of all types
    together, sum_a sums[:, a] / (counts N); nan where a lag has no origin yet or the type no particle.  NumPy only."""
    import numpy as np
    sums, counts = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    tot, n = (sums.sum(axis=1), float(np.sum(type_counts))) if a is None else (sums[:, a], float(type_counts[a]))
    den = counts * n
    return np.divide(tot, den[:, None], out=np.full(tot.shape, np.nan), where=den[:, None] > 0.0)


class MSD(_TypedAnalyzer):
    """Displacement moments of a run over many time origins: every `period` steps (a sample) the displacements d of the integrator's
    group since each live origin are reduced on the device (pse_msd_accumulate) to ten sums per particle type and lag -- dx dy dz,
    dx^2 dy^2 dz^2 dxdy dxdz dydz, |d|^4 -- in a float64 CUDA tensor of this object, and every `origin_every` samples the unwrapped
    positions become a new origin (pse_msd_store).  Lags run from 1 to `nlags` samples; ceil(nlags / origin_every) <= 64 origins are
    kept.  Sampling only queues work; the readers below are the only places that wait for the device.  `types`, `type_names`: as for
    RDF; at most 8 types.  Positions are unwrapped with the system's accumulated strain (System.strain, analyze.unwrap): a flip of
    the box does not move them.

    Under shear the displacement contains the affine advection dx = rate * integral of y_u dt: the xx, xy and xz entries of the
    tensor, the x component of the mean displacement and the trace contain it; yy, zz and yz do not (read msd_tensor()[:, 1, 1] +
    msd_tensor()[:, 2, 2] for the diffusion across the flow).  LIMIT (analyze.unwrap): once the box has flipped, every y image a
    particle gains shifts its unwrapped x by flips * Ly, so everything that contains x -- xx, xy, xz, the trace msd(), alpha2(), the x
    of mean_displacement() and of displacement() -- is wrong from then on; yy, zz, yz and the y, z drift stay right.  msd() and
    alpha2() warn (RuntimeWarning) when a sample was taken in a flipped box.

    lags -- in steps;  counts -- origins per lag;  sums -- (nlags, ntypes, 10);  mean_displacement(a) -- (nlags, 3);  msd(a) -- the
    trace, (nlags,);  msd_tensor(a) -- (nlags, 3, 3);  alpha2(a) = 3 <d^4> / (5 <d^2>^2) - 1;  displacement(slot=, lag=) -- (N, 4) per
    particle against the CURRENT positions: d and |d|^2;  reset().  a = None: all types together."""

    def __init__(self, integrator, nlags, origin_every=1, types=None, type_names=None, period=1):
        import torch
        self._schedule, types, self.ntypes, self.type_names, self.period = _msd_analyzer_arguments(
            nlags, origin_every, types, type_names, period)   # (raises before the device is touched)
        with self._attach(integrator, types) as system:
            self.nlags, self.origin_every, self.norigins = self._schedule.nlags, self._schedule.origin_every, self._schedule.norigins
            self._origins = DisplacementOrigins(integrator.engine, types, self.ntypes, self.norigins, system.n)
            self._sums = torch.zeros((self.nlags, self.ntypes, MSD_MOMENTS), dtype=torch.float64, device=system.pos.device)
            self.flipped = False      # a sample was taken with tilt_flips != 0: the moments that contain x are not to be trusted

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        s, e, g = self.system, self.integrator.engine, self.integrator.group.members
        self.flipped = self.flipped or s.tilt_flips != 0
        self._schedule.sample(lambda slots, rows: e.msd_accumulate(s.pos, s.image, self._origins, s.strain, slots, rows, self._sums, group=g),
                              lambda slot: e.msd_store(s.pos, s.image, self._origins, slot, s.strain, group=g))

    def reset(self):
        """Forget the sums, the counts and the origins."""
        self._sums.zero_()
        self._schedule.reset()
        self.flipped = False

    def _warn_x(self, what):
        if self.flipped:
            import warnings
            warnings.warn(f"{what} contains the unwrapped x, which is shifted by flips * Ly for every y image gained after a "
                          "Lees-Edwards flip (analyze.unwrap): samples were taken in a flipped box; use the yy, zz, yz entries of "
                          "msd_tensor()", RuntimeWarning, stacklevel=3)

    @property
    def samples(self):
        return self._schedule.samples

    @property
    def lags(self):
        import numpy as np
        return np.arange(1, self.nlags + 1) * self.period

    @property
    def counts(self):
        import numpy as np
        return np.array(self._schedule.counts, dtype=np.int64)

    @property
    def sums(self):
        return self._sums.cpu().numpy()

    def _moments(self, a):
        return moments_of_sums(self.sums, self.counts, self._type_counts(), None if a is None else self._code(a))

    def mean_displacement(self, a=None):
        return self._moments(a)[:, 0:3]

    def msd_tensor(self, a=None):
        import numpy as np
        m = self._moments(a)
        t = np.empty((self.nlags, 3, 3))
        for (i, j), c in {(0, 0): 3, (1, 1): 4, (2, 2): 5, (0, 1): 6, (0, 2): 7, (1, 2): 8}.items():
            t[:, i, j] = t[:, j, i] = m[:, c]
        return t

    def msd(self, a=None):
        self._warn_x("msd()")
        m = self._moments(a)
        return m[:, 3] + m[:, 4] + m[:, 5]

    def alpha2(self, a=None):
        import numpy as np
        self._warn_x("alpha2()")
        m = self._moments(a)
        d2 = m[:, 3] + m[:, 4] + m[:, 5]
        return np.divide(3.0 * m[:, 9], 5.0 * d2 * d2, out=np.full(self.nlags, np.nan), where=d2 > 0.0) - 1.0

    def displacement(self, slot=None, lag=None):
        """(N, 4): d and |d|^2 of every particle of the group from the origin in `slot` -- or the one that was `lag` samples old at the
        last sample -- to the current positions; rows outside the group are zero.  A slot that holds no origin stored since the
        last reset() is refused.  (x: see LIMIT above.)"""
        if (slot is None) == (lag is None):
            raise ValueError("displacement() takes a slot or a lag")
        slot = self._schedule.slot_of_lag(lag) if slot is None else int(slot)
        if slot not in self._schedule.live:
            raise ValueError(f"slot {slot} holds no origin stored since the last reset()")
        s = self.system
        return self.integrator.engine.msd_displacement(s.pos, s.image, self._origins, slot, s.strain,
                                                       group=self.integrator.group.members).cpu().numpy()


def size_distribution_of(hist, samples):
    """n(s), s = 1 .. len(hist): the mean number of clusters of s members per sample, from the accumulated counts; the last entry
    holds every cluster of len(hist) members or more.  NumPy only."""
    import numpy as np
    if samples < 1:
        raise ValueError("no samples yet")
    return np.asarray(hist, dtype=np.float64) / float(samples)


def averages_of(rows):
    """From the per-sample rows (clusters, largest, sum of s^2, N), one per sample: the number-average size sum N / sum clusters,
    the weight-average size sum s^2 / sum N -- the size of the cluster a randomly chosen particle is in -- and the mean over the
    samples of largest / N.  Returns (number_average, weight_average, largest_fraction).  NumPy only."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    if rows.shape[0] < 1:
        raise ValueError("no samples yet")
    return (float(rows[:, 3].sum() / rows[:, 0].sum()), float(rows[:, 2].sum() / rows[:, 3].sum()), float((rows[:, 1] / rows[:, 3]).mean()))


def unfold_clusters(pos, images, box):
    """pos + images (a1, a2, a3) for the box (Lx, Ly, Lz[, xy]): every cluster that spans nothing made whole around its label member
    (the `image` of Engine.cluster_span, Clusters.images()).  pos (n, 3) or (n, 4); returns (n, 3).  NumPy only."""
    import numpy as np
    pos, images = np.asarray(pos, dtype=np.float64), np.asarray(images)
    if pos.ndim != 2 or pos.shape[1] not in (3, 4) or images.shape != (pos.shape[0], 3):
        raise ValueError("pos must be (n, 3) or (n, 4) and images (n, 3)")
    Lx, Ly, Lz = (float(b) for b in box[:3])
    xy = float(box[3]) if len(box) > 3 else 0.0
    im = images.astype(np.float64)
    out = pos[:, :3].copy()
    out[:, 0] += im[:, 0] * Lx + im[:, 1] * (xy * Ly)
    out[:, 1] += im[:, 1] * Ly
    out[:, 2] += im[:, 2] * Lz
    return out


def fractal_dimension_of(sizes, rg2, smin=5):
    """d_f from s ~ Rg^d_f: the least-squares slope of log s on log Rg over the clusters with s >= smin and Rg^2 > 0 (one entry per
    cluster; spanning clusters, rg2 = -1, and singletons drop out).  At least two distinct radii are needed.  NumPy only."""
    import numpy as np
    sizes, rg2 = np.asarray(sizes, dtype=np.float64).ravel(), np.asarray(rg2, dtype=np.float64).ravel()
    if sizes.shape != rg2.shape:
        raise ValueError("sizes and rg2 must have one entry per cluster each")
    keep = (sizes >= smin) & (rg2 > 0.0)
    x, y = 0.5 * np.log(rg2[keep]), np.log(sizes[keep])
    if len(x) < 2 or np.ptp(x) == 0.0:
        raise ValueError(f"fewer than two clusters of {smin} or more members with distinct radii: no slope")
    x0, y0 = x - x.mean(), y - y.mean()
    return float((x0 * y0).sum() / (x0 * x0).sum())


def percolation_averages_of(rows, axis=None):
    """From the per-sample rows of eight words (Engine.cluster_span's pstats) and the rows of four (stats), one per sample:
    (the share of samples with a cluster spanning `axis` -- 0, 1, 2; None: any --, the weight-average size of the clusters that span
    nothing, sum s^2 / sum s over them; nan where every particle is in a spanning cluster).  NumPy only."""
    import numpy as np
    p, st = rows
    p, st = np.asarray(p, dtype=np.float64).reshape(-1, 8), np.asarray(st, dtype=np.float64).reshape(-1, 4)
    if p.shape[0] < 1 or p.shape[0] != st.shape[0]:
        raise ValueError("no samples yet")
    if axis is not None and int(axis) not in (0, 1, 2):
        raise ValueError("axis must be None, 0, 1 or 2")
    col = p[:, 0] if axis is None else p[:, 2 + int(axis)]
    free = (st[:, 3] - p[:, 1]).sum()
    return float((col > 0).mean()), float(p[:, 7].sum() / free) if free > 0 else float("nan")


def _cluster_analyzer_arguments(rlink, types, type_names, period, nhist, capacity):
    """What Clusters checks before it touches the device.  A dict `rlink` may name its types by `type_names`.  Returns (types uint32
    or None, ntypes, rlink (npt,), names or None, period, nhist or None, capacity)."""
    types, ntypes, names, period = _typed_arguments(types, type_names, period)
    types, ntypes, rlink = _cluster_arguments(types, ntypes, _pair_dict_codes(rlink, names, "rlink"))
    if nhist is not None and int(nhist) < 1:
        raise ValueError("nhist must be positive")
    if int(capacity) < 1:
        raise ValueError("capacity must be positive")
    return types, ntypes, rlink, names, period, None if nhist is None else int(nhist), int(capacity)


class Clusters(_TypedAnalyzer, _SampleRing):
    """Which particles hang together: every `period` steps the members of the integrator's group are labelled by the connected
    component of the links 0 < r < rlink (pse_clusters_label; a union-find on the device over the cell list the step uses anyway).
    `rlink`: a scalar, a dict {(a, b): r} over pairs of types (names with `type_names=`; a missing pair never links) or one entry per
    pair of types; none may exceed the hydrodynamic real-space cutoff.  `types`, `type_names`, `exclusions`: as for RDF.
    Each sample writes its row (clusters, largest, sum of s^2, N) into a device ring of `capacity` rows -- once full, the oldest rows
    are replaced -- and adds its clusters to the size counts, `nhist` words (default: the number of particles; the last holds every
    larger cluster).  Sampling only queues work; the readers are the only places that wait for the device.
    `percolation=True`: every sample also finds which clusters are connected to their own periodic image and along which lattice
    axes, makes every other cluster whole across the boundaries and takes its radius of gyration (pse_clusters_span; the definitions
    are in include/pse_amd.h), and keeps a second device ring of eight words per sample.  The default leaves every call, row and
    column as without it.  Not measured: the centre of mass and the gyration tensor per cluster (unfolded() gives the host what it needs).

    labels(), sizes() -- the last sample, by particle index (-1 / 0 outside the group);  table() -- (samples kept, 5): step, clusters,
    largest, sum s^2, N;  size_distribution() -- mean n(s) per sample;  number_average(), weight_average(), largest_fraction() -- over
    the samples kept;  members(label);  samples;  reset().
    With percolation: spanning() -- (n,) bits 0, 1, 2 per particle;  images() -- (n, 3);  unfolded() -- the sampled positions plus
    images (a1, a2, a3);  rg2() -- (n,), -1 in a spanning cluster;  cluster_table() -- one row per cluster
    of the last sample: label, size, span, Rg^2;  percolation_table() -- (samples kept, 9): step and PERCOLATION_COLUMNS;
    percolation_probability(axis=None) -- the share of kept samples with a spanning cluster;  finite_weight_average() -- sum s^2 /
    sum s over the clusters that span nothing."""

    COLUMNS = ("timestep", "clusters", "largest", "sum_s2", "N")
    PERCOLATION_COLUMNS = ("timestep", "spanning", "spanning_members", "span_a1", "span_a2", "span_a3", "span_all", "largest_finite",
                           "sum_s2_finite")

    def __init__(self, integrator, rlink, types=None, type_names=None, exclusions=None, period=1, nhist=None, capacity=1024,
                 percolation=False):
        import torch
        self.percolation = bool(percolation)
        types, self.ntypes, self.rlink, self.type_names, self.period, nhist, self.capacity = _cluster_analyzer_arguments(
            rlink, types, type_names, period, nhist, capacity)   # (raises before the device is touched)
        with self._attach(integrator, types) as system:
            self.nhist = system.n if nhist is None else nhist
            self._excl = _excl_list(integrator, exclusions)
            self._links = ClusterLinks(integrator.engine, types, self.ntypes, self.rlink, system.n)
            dev = system.pos.device
            self._label = torch.full((system.n,), -1, dtype=torch.int32, device=dev)
            self._size = torch.zeros(system.n, dtype=torch.int32, device=dev)
            self._rows = torch.zeros((self.capacity, 4), dtype=torch.int64, device=dev)
            self._hist = torch.zeros(self.nhist, dtype=torch.int64, device=dev)
            if self.percolation:
                self._span = torch.zeros(system.n, dtype=torch.int32, device=dev)
                self._image = torch.zeros((system.n, 3), dtype=torch.int32, device=dev)
                self._rg2 = torch.zeros(system.n, dtype=torch.float64, device=dev)
                self._prows = torch.zeros((self.capacity, 8), dtype=torch.int64, device=dev)
                self._pos_at = torch.zeros_like(system.pos)
            self._ring_reset()

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        q = self._slot()
        if self.percolation:
            self.integrator.engine.cluster_span(self.system.pos, self._links, label=self._label, size=self._size, stats=self._rows[q],
                                                hist=self._hist, span=self._span, image=self._image, rg2=self._rg2, pstats=self._prows[q],
                                                group=self.integrator.group.members, exclusions=self._excl)
            self._pos_at.copy_(self.system.pos)   # (queued behind the pass: the step that follows moves the particles)
        else:
            self.integrator.engine.cluster_label(self.system.pos, self._links, label=self._label, size=self._size, stats=self._rows[q],
                                                 hist=self._hist, group=self.integrator.group.members, exclusions=self._excl)
        self._record(q, timestep)

    def reset(self):
        self._rows.zero_(); self._hist.zero_()
        self._label.fill_(-1); self._size.zero_()
        if self.percolation:
            self._span.zero_(); self._image.zero_(); self._rg2.zero_(); self._prows.zero_()
        self._ring_reset()

    def _percolating(self):
        if not self.percolation:
            raise ValueError("this analyzer was made without percolation=True")
        self._sampled()

    def spanning(self):
        """(n,) int64: bits 0, 1, 2 are set when the particle's cluster in the last sample spans a1, a2, a3; 0 outside the group."""
        self._percolating()
        return self._span.cpu().numpy().astype("int64")

    def images(self):
        """(n, 3) int64: the lattice vector that makes the particle's cluster whole around its label member; zeros in a spanning cluster."""
        self._percolating()
        return self._image.cpu().numpy().astype("int64")

    def unfolded(self):
        """(n, 3): the positions of the last sample plus images() (a1, a2, a3) in the current box: every cluster that spans nothing
        in one piece.  The analyzer keeps a device copy of the sampled positions, since the step that follows a sample moves the
        particles; valid until the box changes."""
        self._percolating()
        return unfold_clusters(self._pos_at.cpu().numpy(), self.images(), self.system.box)

    def rg2(self):
        """(n,) float64: Rg^2 of the particle's cluster in the last sample; 0 for a singleton and outside the group, -1 in a spanning one."""
        self._percolating()
        return self._rg2.cpu().numpy()

    def cluster_table(self):
        """One row per cluster of the last sample, by ascending label: a structured array with the fields label, size, span, rg2."""
        import numpy as np
        label, size, span, rg2 = self.labels(), self.sizes(), self.spanning(), self.rg2()
        roots = np.nonzero(label == np.arange(len(label)))[0]
        out = np.zeros(len(roots), dtype=[("label", np.int64), ("size", np.int64), ("span", np.int64), ("rg2", np.float64)])
        out["label"], out["size"], out["span"], out["rg2"] = roots, size[roots], span[roots], rg2[roots]
        return out

    def percolation_table(self):
        """(samples kept, 9) int64, oldest first: PERCOLATION_COLUMNS."""
        import numpy as np
        if not self.percolation:
            raise ValueError("this analyzer was made without percolation=True")
        n = min(self.samples, self.capacity)
        dev = self._prows.cpu().numpy()
        out = np.zeros((n, 9), dtype=np.int64)
        for r in range(n):
            q = (self.samples - n + r) % self.capacity
            out[r, 0], out[r, 1:] = self._steps[q], dev[q]
        return out

    def percolation_probability(self, axis=None):
        """The share of the kept samples in which some cluster spans `axis` (0, 1, 2; None: any axis)."""
        return percolation_averages_of((self.percolation_table()[:, 1:], self.table()[:, 1:]), axis)[0]

    def finite_weight_average(self):
        """sum s^2 / sum s over the clusters that span nothing, over the kept samples: the weight-average size short of the gel."""
        return percolation_averages_of((self.percolation_table()[:, 1:], self.table()[:, 1:]))[1]

    def status(self):
        """The give-up word of the device object (0: every sample was labelled completely; see include/pse_amd.h)."""
        return self._links.status()

    def labels(self):
        """(n,) int64: the smallest particle index of every particle's cluster in the last sample; -1 outside the group."""
        self._sampled()
        return self._label.cpu().numpy().astype("int64")

    def sizes(self):
        """(n,) int64: the number of members of every particle's cluster in the last sample; 0 outside the group."""
        self._sampled()
        return self._size.cpu().numpy().astype("int64")

    def members(self, label):
        """The particle indices of the cluster whose label is `label` (the smallest index among them), ascending."""
        import numpy as np
        return np.nonzero(self.labels() == int(label))[0]

    def size_distribution(self):
        """n(s) for s = 1 .. nhist: the mean number of clusters of s members per sample since the last reset(); its sum is the mean
        number of clusters.  The last entry counts every cluster of nhist members or more."""
        return size_distribution_of(self._hist.cpu().numpy(), self.samples)

    def number_average(self):
        return averages_of(self.table()[:, 1:])[0]

    def weight_average(self):
        return averages_of(self.table()[:, 1:])[1]

    def largest_fraction(self):
        return averages_of(self.table()[:, 1:])[2]


# The upper edge of the bins of q_l and q-bar_l in BondOrder.  pse_bond_order_histogram counts lo <= v < hi, and both are at most 1
# exactly but 1 up to rounding for a particle with one neighbour -- above it as often as below, by less than 1e-9 (the error bound of
# DESIGN.md): with hi = 1 those particles would be dropped.  The bins are therefore [b, b + 1) BOND_ORDER_HI / nbins.
BOND_ORDER_HI = 1.0 + 2.0 ** -26


def histogram_mean(counts, lo=0.0, hi=BOND_ORDER_HI):
    """The mean of the binned values from their counts: sum_b counts[b] centre_b / sum_b counts[b], centre_b the middle of bin b of
    the uniform bins on [lo, hi) (default: the bins of BondOrder) -- exact to half a bin width.  NumPy only."""
    import numpy as np
    counts = np.asarray(counts, dtype=np.float64).ravel()
    if counts.sum() <= 0:
        raise ValueError("no samples yet")
    edges = bin_edges(len(counts), lo, hi)
    return float((counts * 0.5 * (edges[:-1] + edges[1:])).sum() / counts.sum())


def solid_fraction_of(rows, a=None):
    """From the per-sample rows (members, solid-like) per type, shape (samples, ntypes, 2): the solid-like members of type `a` (None:
    of all types) over all samples divided by the members.  NumPy only."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(-1, rows.shape[-2] if rows.ndim >= 2 else 1, 2)
    if rows.shape[0] < 1:
        raise ValueError("no samples yet")
    sel = rows if a is None else rows[:, int(a):int(a) + 1]
    if sel[..., 0].sum() <= 0:
        raise ValueError("no members of that type")
    return float(sel[..., 1].sum() / sel[..., 0].sum())


def _bond_order_analyzer_arguments(rnb, degrees, types, type_names, period, solid, nbins, capacity):
    """What BondOrder checks before it touches the device.  A dict `rnb` may name its types by `type_names`.  Returns (types uint32 or
    None, ntypes, rnb (npt,), degrees int32, names or None, period, solid or None, nbins, capacity)."""
    types, ntypes, names, period = _typed_arguments(types, type_names, period)
    types, ntypes, rnb, degrees = _bond_order_arguments(types, ntypes, _pair_dict_codes(rnb, names, "rnb"), degrees)
    if solid is not None:
        if not (isinstance(solid, (tuple, list)) and len(solid) == 3):
            raise ValueError("solid must be None or (degree, threshold, min_conn)")
        degree, threshold, min_conn = int(solid[0]), float(solid[1]), int(solid[2])
        if degree not in degrees.tolist():
            raise ValueError(f"solid names the degree {degree}, which is not among the degrees {tuple(degrees.tolist())}")
        if not (math.isfinite(threshold) and -1.0 <= threshold <= 1.0):
            raise ValueError(f"solid threshold = {threshold} outside [-1, 1]")
        if min_conn < 0:
            raise ValueError("solid min_conn must not be negative")
        solid = (degree, threshold, min_conn)
    if int(nbins) < 1 or ntypes * int(nbins) > BOND_ORDER_MAX_COUNTERS:
        raise ValueError(f"nbins = {nbins}: need at least one bin and at most {BOND_ORDER_MAX_COUNTERS} counters over the {ntypes} types")
    if int(capacity) < 1:
        raise ValueError("capacity must be positive")
    return types, ntypes, rnb, degrees, names, period, solid, int(nbins), int(capacity)


class BondOrder(_TypedAnalyzer, _SampleRing):
    """Whether the neighbourhoods are ordered: every `period` steps the Steinhardt bond-orientational order parameters q_l of the
    members of the integrator's group, their neighbour-averaged form q-bar_l (Lechner and Dellago) and, with `solid=(degree, threshold,
    min_conn)`, e.g. (6, 0.7, 7), the solid-like bonds of ten Wolde, Ruiz-Montero and Frenkel (pse_bond_order_compute: two passes over
    the cell list the step uses anyway).  Neighbours are the particles within `rnb`: a scalar, a dict {(a, b): r} over pairs of types
    (names with `type_names=`; a missing pair is never a neighbour) or one entry per pair of types, none beyond the hydrodynamic
    real-space cutoff.  `degrees`: 1 to 4 distinct even l from 2 to 12.  `types`, `type_names`, `exclusions`: as for RDF.
    Each sample adds q_l and q-bar_l of every degree to per-type histograms of `nbins` uniform bins on [0, BOND_ORDER_HI) on the device --
    the upper edge 1 + 2^-26, so that a q of 1 with its rounding (one neighbour) lands in the last bin: every member is counted -- and writes its
    row (members, solid-like per type) into a device ring of `capacity` rows -- once full, the oldest rows are replaced.  Sampling
    only queues work; the readers are the only places that wait for the device.
    solid_like() is a boolean mask by particle index: Group(system, numpy.nonzero(mask)[0]) of it is the group an analyze.Clusters on
    a second integrator view would label to find the largest crystalline nucleus (the coupling itself is left to the caller).

    q(l), qbar(l), neighbors(), connections(), solid_like() -- the last sample, by particle index (0 outside the group);
    histogram(l, a=None, averaged=False) -- the accumulated counts;  mean(l, a=None, averaged=False) -- from them;  table() --
    (samples kept, 1 + 2 ntypes): timestep, then members and solid-like per type;  solid_fraction(a=None);  samples;  reset()."""

    def __init__(self, integrator, rnb, degrees=(4, 6), types=None, type_names=None, exclusions=None, period=1, solid=None, nbins=100,
                 capacity=1024):
        import torch
        types, self.ntypes, self.rnb, self.degrees, self.type_names, self.period, self.solid, self.nbins, self.capacity = \
            _bond_order_analyzer_arguments(rnb, degrees, types, type_names, period, solid, nbins, capacity)   # (raises before the device is touched)
        with self._attach(integrator, types) as system:
            self.nl = int(self.degrees.shape[0])
            self._excl = _excl_list(integrator, exclusions)
            self._shells = BondOrderShells(integrator.engine, types, self.ntypes, self.rnb, self.degrees, system.n)
            dev = system.pos.device
            self._nnb = torch.zeros(system.n, dtype=torch.int32, device=dev)
            self._nconn = torch.zeros(system.n, dtype=torch.int32, device=dev)
            self._q = torch.zeros((system.n, self.nl), dtype=torch.float64, device=dev)
            self._qbar = torch.zeros((system.n, self.nl), dtype=torch.float64, device=dev)
            self._rows = torch.zeros((self.capacity, self.ntypes, 2), dtype=torch.int64, device=dev)
            self._hist = torch.zeros((2, self.nl, self.ntypes, self.nbins), dtype=torch.int64, device=dev)   # [q | q-bar][degree][type][bin]
            self._ring_reset()

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        eng, members = self.integrator.engine, self.integrator.group.members
        r = self._slot()
        eng.bond_order(self.system.pos, self._shells, nnb=self._nnb, q=self._q, qbar=self._qbar, solid=self.solid,
                       nconn=None if self.solid is None else self._nconn, stats=self._rows[r], group=members, exclusions=self._excl)
        for which, values in enumerate((self._q, self._qbar)):
            for d, l in enumerate(self.degrees.tolist()):
                eng.bond_order_histogram(values, self._shells, l, self._hist[which, d], 0.0, BOND_ORDER_HI, group=members)
        self._record(r, timestep)

    def reset(self):
        for t in (self._rows, self._hist, self._nnb, self._nconn, self._q, self._qbar):
            t.zero_()
        self._ring_reset()

    def q(self, l):
        """(n,) float64: q_l of every particle in the last sample; 0 outside the group."""
        self._sampled()
        return self._q[:, self._shells.column(l)].cpu().numpy()

    def qbar(self, l):
        """(n,) float64: the neighbour-averaged q-bar_l of every particle in the last sample; 0 outside the group."""
        self._sampled()
        return self._qbar[:, self._shells.column(l)].cpu().numpy()

    def neighbors(self):
        """(n,) int64: the number of neighbours of every particle in the last sample; 0 outside the group."""
        self._sampled()
        return self._nnb.cpu().numpy().astype("int64")

    def _solid(self):
        self._sampled()
        if self.solid is None:
            raise ValueError("this BondOrder has no solid-bond pass: give solid=(degree, threshold, min_conn)")

    def connections(self):
        """(n,) int64: the number of solid-like bonds of every particle in the last sample; 0 outside the group."""
        self._solid()
        return self._nconn.cpu().numpy().astype("int64")

    def solid_like(self):
        """(n,) bool: the group members with at least min_conn solid-like bonds in the last sample -- the particles to hand, as a
        Group, to an analyze.Clusters that is to find the crystalline nuclei."""
        import numpy as np
        conn = self.connections()
        members = self.integrator.group.members   # (None: every particle)
        if members is None:
            return conn >= self.solid[2]
        mask = np.zeros(self.system.n, dtype=bool)
        members = members.cpu().numpy().astype("int64")
        mask[members] = conn[members] >= self.solid[2]
        return mask

    def histogram(self, l, a=None, averaged=False):
        """(nbins,) int64: the counts of q_l (averaged=True: of q-bar_l) in the bins on [0, BOND_ORDER_HI) over all samples since the last reset(), of type `a`
        (an index or a name; None: of all types)."""
        self._sampled()
        h = self._hist[1 if averaged else 0, self._shells.column(l)].cpu().numpy()
        return h.sum(axis=0) if a is None else h[_type_codes([a], self.type_names)[0]]

    def mean(self, l, a=None, averaged=False):
        """The mean of q_l (averaged=True: of q-bar_l) over all samples, from the histogram: exact to half a bin width."""
        return histogram_mean(self.histogram(l, a, averaged))

    def solid_fraction(self, a=None):
        """The solid-like members of type `a` (None: all) over the samples kept, divided by the members."""
        self._solid()
        return solid_fraction_of(self.table()[:, 1:].reshape(-1, self.ntypes, 2), None if a is None else _type_codes([a], self.type_names)[0])


def molecules_of(n, bonds):
    """The molecules of a bond list by the rule of pse_host_molecule_rows, NumPy only: (mol_of, nmol).  The molecules are the connected
    components of the (nbonds, 2) index pairs `bonds` among n particles with at least two members, numbered in the order of their
    smallest member; mol_of (n,) int64 holds the molecule of every particle, -1 for a particle without a bond.  For building one type
    per molecule (Conformations(molecule_types=...)).  A bond (i, i) makes no molecule here; the library refuses it."""
    import numpy as np
    n = int(n)
    b = np.asarray(bonds)
    if b.ndim != 2 or b.shape[1] != 2 or b.shape[0] == 0 or not np.issubdtype(b.dtype, np.integer):
        raise ValueError("bonds must be a non-empty integer (nbonds, 2) array of particle indices")
    if n < 1 or b.min() < 0 or b.max() >= n:
        raise ValueError(f"bonds holds an index outside [0, n = {n})")
    i, j = b[:, 0].astype(np.int64), b[:, 1].astype(np.int64)
    label = np.arange(n, dtype=np.int64)
    while True:   # the smallest label of a component spreads along the bonds, and every label jumps to its own label's label
        new = label.copy()
        np.minimum.at(new, i, label[j])
        np.minimum.at(new, j, label[i])
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    bonded = np.zeros(n, dtype=bool)
    bonded[i[i != j]] = True
    bonded[j[i != j]] = True
    roots = np.unique(label[bonded])
    mol_of = np.where(bonded, np.searchsorted(roots, label), -1)
    return mol_of, int(roots.shape[0])


def tensor_of(cols):
    """(..., 6) columns xx, yy, zz, xy, xz, yz as symmetric (..., 3, 3) tensors."""
    import numpy as np
    c = np.asarray(cols, dtype=np.float64)
    return np.stack([np.stack([c[..., 0], c[..., 3], c[..., 4]], -1), np.stack([c[..., 3], c[..., 1], c[..., 5]], -1),
                     np.stack([c[..., 4], c[..., 5], c[..., 2]], -1)], -2)


def shape_of(G):
    """The shape descriptors of gyration tensors G (..., 3, 3): (eigenvalues (..., 3) in ascending order l1 <= l2 <= l3, asphericity
    b = l3 - (l1 + l2)/2, acylindricity c = l2 - l1, relative shape anisotropy kappa^2 = (b^2 + 3/4 c^2) / (l1 + l2 + l3)^2: 0 for a
    sphere, 1 for a rod)."""
    import numpy as np
    lam = np.linalg.eigvalsh(np.asarray(G, dtype=np.float64))
    b = lam[..., 2] - 0.5 * (lam[..., 0] + lam[..., 1])
    c = lam[..., 1] - lam[..., 0]
    return lam, b, c, (b * b + 0.75 * c * c) / lam.sum(axis=-1) ** 2


def orientation_angle(G):
    """The orientation angle chi of tensors G (..., 3, 3) in the flow-gradient plane: tan 2 chi = 2 G_xy / (G_xx - G_yy), chi in
    (-pi/2, pi/2], the angle of the major axis of the xy block against the flow direction x."""
    import numpy as np
    G = np.asarray(G, dtype=np.float64)
    return 0.5 * np.arctan2(2.0 * G[..., 0, 1], G[..., 0, 0] - G[..., 1, 1])


MOL_MAX_TYPES = 8   # molecule types of one Conformations


def _conformation_arguments(bonds, molecule_types, type_names, period, nbins, rg_max, ree_max, capacity):
    """What Conformations checks before it touches the device, from the (nbonds, 2) pairs `bonds` (the molecules and their numbers do
    not depend on how many particles there are beyond the largest index).  Returns (pairs
    uint32, molecule types uint32 (nmol,) or None, ntypes, names or None, period, nbins, rg_max, ree_max, capacity, sizes (nmol,),
    size_values: the molecule size of every type with molecule_types="size", else None)."""
    import numpy as np
    from .engine import _molecule_arguments
    names = None if type_names is None else list(type_names)
    if names is not None and (not names or len(set(names)) != len(names) or not all(isinstance(v, str) for v in names)):
        raise ValueError("type_names must be distinct strings")
    if int(period) < 1:
        raise ValueError("period must be positive")
    if int(capacity) < 1:
        raise ValueError("capacity must be positive")
    b = np.asarray(bonds)
    if b.ndim != 2 or b.shape[1:] != (2,) or b.shape[0] == 0 or not np.issubdtype(b.dtype, np.integer) or b.min() < 0:
        raise ValueError("bonds must be a forces.Bonds or a non-empty integer (nbonds, 2) array of particle indices")
    mol_of, nmol = molecules_of(int(b.max()) + 1, b)
    if nmol == 0:
        raise ValueError("bonds makes no molecule")
    sizes = np.bincount(mol_of[mol_of >= 0], minlength=nmol)
    size_values = None
    if molecule_types is None:
        if names is not None and len(names) != 1:
            raise ValueError("type_names without molecule_types: there is one type")
        types, ntypes = None, 1
    elif isinstance(molecule_types, str):
        if molecule_types != "size":
            raise ValueError('molecule_types must be None, "size" or one code or name per molecule')
        size_values = np.unique(sizes)
        if size_values.shape[0] > MOL_MAX_TYPES:
            raise ValueError(f"molecule_types=\"size\": {size_values.shape[0]} distinct molecule sizes, more than {MOL_MAX_TYPES} types")
        types, ntypes = np.searchsorted(size_values, sizes), int(size_values.shape[0])
        if names is not None and len(names) != ntypes:
            raise ValueError(f"type_names has {len(names)} entries, the molecules {ntypes} sizes")
    else:
        types = np.asarray(_type_codes(molecule_types.tolist() if hasattr(molecule_types, "tolist") else list(molecule_types), names))
        if types.ndim != 1 or not np.issubdtype(types.dtype, np.integer) or (types.shape[0] and types.min() < 0):
            raise ValueError("molecule_types must be a 1-D sequence of non-negative integers or names, one per molecule")
        if types.shape[0] != nmol:
            raise ValueError(f"molecule_types has {types.shape[0]} entries, the bonds make {nmol} molecules")
        ntypes = max(int(types.max()) + 1, len(names or ()))
    ntypes = _ntypes_argument(ntypes)
    pairs, types, ntypes, nbins, rg_max, ree_max = _molecule_arguments(bonds, types, ntypes, nbins, rg_max, ree_max)
    return pairs, types, ntypes, names, int(period), nbins, rg_max, ree_max, int(capacity), sizes, size_values


class Conformations(_TypedAnalyzer, _SampleRing):
    """The conformation of the molecules that a bond topology defines: every `period` steps one pass (pse_molecules_compute) unfolds
    every molecule along its own bonds by the minimum image in the box of that step -- right through any number of Lees-Edwards
    flips, while every bond is shorter than half the smallest box length -- and reduces its gyration tensor G, Rg^2 and, for a linear
    molecule, its end-to-end vector R.  `bonds`: a forces.Bonds, whose pairs are reused, or an (nbonds, 2) array of particle indices;
    the molecules are its connected components (molecules_of).  `molecule_types`: None (one type), one code or name (`type_names=`) per
    molecule, or "size": the distinct molecule sizes in ascending order are the types (at most 8).  Each sample adds its per-type sums
    to the accumulated `sums`, writes them alone into a device ring of `capacity` rows -- once full, the oldest rows are replaced --
    and, with nbins > 0, counts Rg on [0, rg_max) and |R| on [0, ree_max).  Sampling only queues work; the readers are the only places
    that wait for the device.  Every particle has mass 1.  Not measured: molecules of more than 1024 members.
    Internal distances, the persistence length and the hydrodynamic radius are ChainStatistics', the time correlations of R and of
    the normal modes are RouseModes'.

    nmol, nlinear, nmol_type, sizes();  gyration_tensor(a), rg2(a), rg4(a), ree_tensor(a), ree2(a), ree4(a) -- means over the molecules
    (R: the linear ones) of type `a` (None: all) and over the samples since reset();  series() -- (samples kept, 1 + ntypes 14): the
    timestep and every type's sums of that sample (COLUMNS);  per_molecule() -- (nmol, 14) at the current positions (ROW_COLUMNS);
    unfolded();  histogram(which, a);  samples;  reset()."""

    COLUMNS = ("Gxx", "Gyy", "Gzz", "Gxy", "Gxz", "Gyz", "Rg4", "RxRx", "RyRy", "RzRz", "RxRy", "RxRz", "RyRz", "R4")
    ROW_COLUMNS = ("cx", "cy", "cz", "Gxx", "Gyy", "Gzz", "Gxy", "Gxz", "Gyz", "Rg2", "Rx", "Ry", "Rz", "R2")

    def __init__(self, integrator, bonds, molecule_types=None, type_names=None, period=1, nbins=0, rg_max=None, ree_max=None, capacity=1024):
        import torch
        from .engine import MOL_COLS, MoleculeTopology
        lst = getattr(bonds, "_list", None)
        pairs = lst.index if lst is not None and hasattr(lst, "index") else bonds
        (pairs, types, self.ntypes, self.type_names, self.period, self.nbins, self.rg_max, self.ree_max, self.capacity, self._sizes,
         self.size_values) = _conformation_arguments(pairs, molecule_types, type_names, period, nbins, rg_max, ree_max, capacity)
        with self._attach(integrator, None) as system:          # (the line above raises before the integrator is touched)
            if int(pairs.max()) >= system.n:
                raise ValueError(f"bonds holds the index {int(pairs.max())}, the system has {system.n} particles")
            self.molecule_types = types
            self._mol = MoleculeTopology(integrator.engine, pairs, types, self.ntypes, self.nbins, self.rg_max, self.ree_max, system.n)
            self.nmol, self.nlinear, self.nmol_type = self._mol.nmol, self._mol.nlinear, self._mol.nmol_type
            dev = system.pos.device
            self._sums = torch.zeros((self.ntypes, MOL_COLS), dtype=torch.float64, device=dev)
            self._rows = torch.zeros((self.capacity, self.ntypes, MOL_COLS), dtype=torch.float64, device=dev)
            self._hist = torch.zeros((2, self.ntypes, self.nbins + 1), dtype=torch.int64, device=dev) if self.nbins else None
            self._ring_reset()

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        q = self._slot()
        self.integrator.engine.molecules_compute(self.system.pos, self._mol, sums=self._sums, sample=self._rows[q], hist=self._hist)
        self._record(q, timestep)

    def reset(self):
        self._sums.zero_(); self._rows.zero_()
        if self._hist is not None:
            self._hist.zero_()
        self._ring_reset()

    def sizes(self):
        """(nmol,) int64: the number of members of every molecule."""
        return self._sizes.astype("int64")

    def sums(self):
        """(ntypes, 14) float64: the accumulated sums (COLUMNS) since the last reset()."""
        return self._sums.cpu().numpy()

    def _mean(self, a, cols, counts):
        import numpy as np
        self._sampled()
        s = self.sums()
        if a is None:
            return s[:, cols].sum(axis=0) / (self.samples * counts.sum())
        a = self._code(a)
        return s[a, cols] / (self.samples * counts[a]) if counts[a] else np.full(len(range(*cols.indices(14))), np.nan)

    def gyration_tensor(self, a=None):
        """(3, 3): the mean gyration tensor of the molecules of type `a` (None: of all)."""
        return tensor_of(self._mean(a, slice(0, 6), self.nmol_type))

    def rg2(self, a=None):
        """<Rg^2>, the trace of gyration_tensor(a)."""
        return float(self._mean(a, slice(0, 3), self.nmol_type).sum())

    def rg4(self, a=None):
        """<(Rg^2)^2>."""
        return float(self._mean(a, slice(6, 7), self.nmol_type)[0])

    def ree_tensor(self, a=None):
        """(3, 3): <R_a R_b> over the linear molecules of type `a` (None: of all)."""
        return tensor_of(self._mean(a, slice(7, 13), self.nlinear))

    def ree2(self, a=None):
        """<R^2> over the linear molecules."""
        return float(self._mean(a, slice(7, 10), self.nlinear).sum())

    def ree4(self, a=None):
        """<(R^2)^2> over the linear molecules."""
        return float(self._mean(a, slice(13, 14), self.nlinear)[0])

    def series(self):
        """(samples kept, 1 + ntypes 14) float64, oldest first: the timestep, then for every type the 14 sums (COLUMNS) of that sample
        alone (one copy from the device).  Divide by nmol_type (columns 0-6) or nlinear (7-13) for means."""
        import numpy as np
        n = min(self.samples, self.capacity)
        dev = self._rows.cpu().numpy().reshape(self.capacity, -1)
        out = np.zeros((n, 1 + dev.shape[1]))
        for r in range(n):
            q = (self.samples - n + r) % self.capacity
            out[r, 0], out[r, 1:] = self._steps[q], dev[q]
        return out

    table = series   # (the ring's rows are doubles here: the integer table of _SampleRing would truncate them)

    def per_molecule(self):
        """(nmol, 14) float64: the row of every molecule (ROW_COLUMNS) at the system's current positions; the four R columns are NaN for
        a molecule that is not linear.  One pass and one copy; no sample is taken."""
        import torch
        from .engine import MOL_COLS
        rows = torch.empty((self.nmol, MOL_COLS), dtype=torch.float64, device=self.system.pos.device)
        self.integrator.engine.molecules_compute(self.system.pos, self._mol, rows=rows)
        return rows.cpu().numpy()

    def unfolded(self):
        """(n, 4) float64: every member's unfolded position r_root + u at the system's current positions and the number of its
        molecule; (NaN, NaN, NaN, -1) for a particle in no molecule."""
        import torch
        out = torch.full((self.system.n, 4), float("nan"), dtype=torch.float64, device=self.system.pos.device)
        out[:, 3] = -1.0
        self.integrator.engine.molecules_compute(self.system.pos, self._mol, unfolded=out)
        return out.cpu().numpy()

    def histogram(self, which, a=None):
        """(counts (nbins + 1,), edges (nbins + 1,)): the accumulated counts of `which` = "rg" (Rg of every molecule) or "ree" (|R| of
        the linear ones) for the type `a` (None: all types); counts[b] belongs to [edges[b], edges[b + 1]), the last entry counts the
        values at or above the maximum."""
        import numpy as np
        if which not in ("rg", "ree"):
            raise ValueError('which must be "rg" or "ree"')
        if self._hist is None:
            raise ValueError("this analyzer was made with nbins = 0: it has no histogram")
        h = self._hist.cpu().numpy()[0 if which == "rg" else 1]
        counts = h.sum(axis=0) if a is None else h[self._code(a)]
        return counts, np.arange(self.nbins + 1) * ((self.rg_max if which == "rg" else self.ree_max) / self.nbins)


def persistence_length_of(s, c, b, smax=1):
    """The persistence length l_p of a bond correlation c(s) ~ exp(-s b / l_p) with the bond length b: -b / k, k the least-squares slope
    through the origin of ln c(s) over s = 1 .. smax, k = sum s ln c(s) / sum s^2, stopping before the first c(s) <= 0 (or NaN).  NaN
    where no separation is left, inf for k == 0."""
    import numpy as np
    s, c = np.asarray(s, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if int(smax) < 1:
        raise ValueError("smax must be positive")
    keep = (s >= 1) & (s <= int(smax))
    s, c = s[keep], c[keep]
    order = np.argsort(s)
    s, c = s[order], c[order]
    bad = np.nonzero(~(c > 0.0))[0]
    if bad.shape[0]:
        s, c = s[:bad[0]], c[:bad[0]]
    if s.shape[0] == 0:
        return float("nan")
    k = float((s * np.log(c)).sum() / (s * s).sum())
    return -float(b) / k if k != 0.0 else float("inf")


class ChainStatistics(_TypedAnalyzer, _SampleRing):
    """The pair statistics of the molecules that a bond topology defines: every `period` steps one pass (pse_molecule_pairs_compute)
    unfolds every molecule as Conformations does and sums over the pairs of its members: 1/Rh = (1/m^2) sum over i != j of 1/r_ij
    (Kirkwood's hydrodynamic radius) for every molecule and, for the linear ones, along the chain, the internal distances
    D(s) = sum_c |r_{c+s} - r_c|^2 and the bond correlations C(s) = sum_c b_c . b_{c+s} for the separations s = 0 .. smax - 1
    (`smax`: default the largest molecule size).  `bonds`, `molecule_types`, `type_names`, `period`, `capacity` as for Conformations.
    The curves and the per-type sums of 1/Rh and (1/Rh)^2 accumulate on the device, every sample's sums alone go into a device ring
    of `capacity` rows.  Sampling only queues work; the readers are the only places that wait for the device.  Every particle has
    mass 1; a pair at distance 0 adds nothing to 1/Rh.

    nmol, nmol_type, terms (ntypes, smax, 2): the summands behind every entry of the curves in one sample;  internal_distances(a) --
    (s, <R^2(s)>);  bond_correlation(a) -- (s, <b.b>_s / <b^2>);  bond_length(a) -- <b^2>^(1/2);  persistence_length(a, smax);
    inv_rh(a) -- <1/Rh>;  rh(a) -- 1 / <1/Rh>;  per_molecule() -- (nmol,) 1/Rh at the current positions;  series() -- (samples kept,
    1 + ntypes 2): the timestep and every type's sums of 1/Rh and (1/Rh)^2 of that sample;  samples;  reset().  `a`: a type (None: all);
    NaN for a type without (linear) molecules."""

    COLUMNS = ("inv_rh", "inv_rh2")

    def __init__(self, integrator, bonds, molecule_types=None, type_names=None, period=1, smax=None, capacity=1024):
        import torch
        from .engine import MOLPAIR_COLS, MOLPAIR_SUMS, MOL_TILE, MoleculePairs
        lst = getattr(bonds, "_list", None)
        pairs = lst.index if lst is not None and hasattr(lst, "index") else bonds
        (pairs, types, self.ntypes, self.type_names, self.period, _, _, _, self.capacity, self._sizes,
         self.size_values) = _conformation_arguments(pairs, molecule_types, type_names, period, 0, None, None, capacity)
        self.smax = int(self._sizes.max()) if smax is None else int(smax)
        if not 1 <= self.smax <= MOL_TILE:
            raise ValueError(f"smax = {self.smax} outside [1, {MOL_TILE}]")
        with self._attach(integrator, None) as system:          # (the lines above raise before the integrator is touched)
            if int(pairs.max()) >= system.n:
                raise ValueError(f"bonds holds the index {int(pairs.max())}, the system has {system.n} particles")
            self.molecule_types = types
            self._pairs = MoleculePairs(integrator.engine, pairs, types, self.ntypes, self.smax, system.n)
            self.nmol, self.nmol_type, self.terms = self._pairs.nmol, self._pairs.nmol_type, self._pairs.terms
            dev = system.pos.device
            self._curves = torch.zeros((self.ntypes, self.smax, MOLPAIR_COLS), dtype=torch.float64, device=dev)
            self._sums = torch.zeros((self.ntypes, MOLPAIR_SUMS), dtype=torch.float64, device=dev)
            self._rows = torch.zeros((self.capacity, self.ntypes, MOLPAIR_SUMS), dtype=torch.float64, device=dev)
            self._ring_reset()

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        q = self._slot()
        self.integrator.engine.molecule_pairs_compute(self.system.pos, self._pairs, curves=self._curves, sums=self._sums, sample=self._rows[q])
        self._record(q, timestep)

    def reset(self):
        self._curves.zero_(); self._sums.zero_(); self._rows.zero_()
        self._ring_reset()

    def sizes(self):
        """(nmol,) int64: the number of members of every molecule."""
        return self._sizes.astype("int64")

    def curves(self):
        """(ntypes, smax, 2) float64: the accumulated sums of D(s) and C(s) since the last reset()."""
        return self._curves.cpu().numpy()

    def sums(self):
        """(ntypes, 2) float64: the accumulated sums of 1/Rh and (1/Rh)^2 since the last reset()."""
        return self._sums.cpu().numpy()

    def _curve(self, a, col):
        """The mean of column `col` of the curves per summand, (smax,): NaN where there is no summand."""
        import numpy as np
        self._sampled()
        c, t = self.curves()[:, :, col], self.terms[:, :, col].astype(np.float64)
        if a is None:
            c, t = c.sum(axis=0), t.sum(axis=0)
        else:
            a = self._code(a)
            c, t = c[a], t[a]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(t > 0, c / (self.samples * t), np.nan)

    def internal_distances(self, a=None):
        """(s (smax,), <R^2(s)> (smax,)): the mean squared distance of two members s bonds apart along the chain, over the linear
        molecules of type `a` (None: of all) and the samples; NaN where no molecule is that long."""
        import numpy as np
        return np.arange(self.smax), self._curve(a, 0)

    def bond_correlation(self, a=None):
        """(s (smax,), c(s) (smax,)): <b_c . b_{c+s}> / <b^2>, c(0) = 1."""
        import numpy as np
        c = self._curve(a, 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.arange(self.smax), c / c[0]

    def bond_length(self, a=None):
        """<b^2>^(1/2) over the bonds of the linear molecules."""
        return float(self._curve(a, 1)[0] ** 0.5)

    def persistence_length(self, a=None, smax=1):
        """persistence_length_of(bond_correlation(a), bond_length(a), smax): -b / k with k the slope of ln c(s) over s = 1 .. smax."""
        s, c = self.bond_correlation(a)
        return persistence_length_of(s, c, self.bond_length(a), smax)

    def inv_rh(self, a=None):
        """<1/Rh> over the molecules of type `a` (None: of all) and the samples."""
        self._sampled()
        s, n = self.sums()[:, 0], self.nmol_type
        if a is None:
            return float(s.sum() / (self.samples * n.sum()))
        a = self._code(a)
        return float(s[a] / (self.samples * n[a])) if n[a] else float("nan")

    def rh(self, a=None):
        """1 / <1/Rh>: the hydrodynamic radius."""
        return 1.0 / self.inv_rh(a)

    def series(self):
        """(samples kept, 1 + ntypes 2) float64, oldest first: the timestep, then for every type the sums of 1/Rh and (1/Rh)^2 over its
        molecules in that sample alone (one copy from the device).  Divide by nmol_type for means."""
        import numpy as np
        n = min(self.samples, self.capacity)
        dev = self._rows.cpu().numpy().reshape(self.capacity, -1)
        out = np.zeros((n, 1 + dev.shape[1]))
        for r in range(n):
            q = (self.samples - n + r) % self.capacity
            out[r, 0], out[r, 1:] = self._steps[q], dev[q]
        return out

    table = series   # (the ring's rows are doubles here: the integer table of _SampleRing would truncate them)

    def per_molecule(self):
        """(nmol,) float64: 1/Rh of every molecule at the system's current positions.  One pass and one copy; no sample is taken."""
        import torch
        out = torch.empty((self.nmol,), dtype=torch.float64, device=self.system.pos.device)
        self.integrator.engine.molecule_pairs_compute(self.system.pos, self._pairs, inv_rh=out)
        return out.cpu().numpy()


def linear_molecules_of(n, bonds):
    """molecules_of and, per molecule, its size and whether it is LINEAR by the rule of pse_host_molecule_rows -- a tree with exactly
    two members of degree 1 and all others of degree 2 (a dimer is): (mol_of, nmol, sizes (nmol,), linear (nmol,) bool).  NumPy only;
    every bond is taken to be listed once (the library refuses a bond listed twice)."""
    import numpy as np
    mol_of, nmol = molecules_of(n, bonds)
    b = np.asarray(bonds).astype(np.int64)
    b = b[b[:, 0] != b[:, 1]]
    deg = np.bincount(b.ravel(), minlength=int(n))
    member = mol_of >= 0
    sizes = np.bincount(mol_of[member], minlength=nmol)
    nb = np.bincount(mol_of[b[:, 0]], minlength=nmol)
    ones = np.bincount(mol_of[member], weights=(deg[member] == 1), minlength=nmol)
    twos = np.bincount(mol_of[member], weights=(deg[member] == 2), minlength=nmol)
    return mol_of, nmol, sizes, (nb == sizes - 1) & (ones == 2) & (twos == sizes - 2)


def relaxation_time_of(lags, c):
    """The time at which a normalised correlation c(t), given at the ascending times `lags`, first falls to 1/e: between the first
    two consecutive points with c[i - 1] > 1/e >= c[i], interpolated linearly in ln c (linearly in c where c[i] <= 0), which is exact
    for exp(-t / tau).  NaN if the curve never crosses.  NumPy only."""
    import numpy as np
    t, c = np.asarray(lags, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if t.ndim != 1 or c.shape != t.shape:
        raise ValueError("lags and c must be 1-D sequences of one length")
    level = math.exp(-1.0)
    for i in range(1, t.shape[0]):
        if c[i - 1] > level >= c[i]:
            if c[i] > 0.0:
                f = (math.log(c[i - 1]) + 1.0) / (math.log(c[i - 1]) - math.log(c[i]))
            else:
                f = (c[i - 1] - level) / (c[i - 1] - c[i])
            return float(t[i - 1] + (t[i] - t[i - 1]) * f)
    return float("nan")


ROUSE_MAX_MODES = 31   # nmodes of one RouseModes: with the end-to-end row, PSE_CHAIN_MODES_MAX functionals


def _rouse_arguments(bonds, nmodes, nlags, origin_every, molecule_types, type_names, period):
    """What RouseModes checks before it touches the device.  Returns (schedule, pairs uint32, molecule types uint32 (nmol,) or None,
    ntypes, names or None, period, K = nmodes + 1, the distinct sizes of the linear molecules, size_values)."""
    import numpy as np
    schedule = MSDSchedule(nlags, origin_every)
    nmodes = int(nmodes)
    if not 1 <= nmodes <= ROUSE_MAX_MODES:
        raise ValueError(f"nmodes = {nmodes} outside [1, {ROUSE_MAX_MODES}]")
    pairs, types, ntypes, names, period, _, _, _, _, _, size_values = _conformation_arguments(bonds, molecule_types, type_names, period, 0,
                                                                                           None, None, 1)
    _, _, sizes, linear = linear_molecules_of(int(pairs.max()) + 1, pairs)
    if not linear.any():
        raise ValueError("bonds makes no linear molecule: there is no chain to project")
    lin_sizes = np.unique(sizes[linear])
    if nmodes >= int(lin_sizes[0]):
        raise ValueError(f"nmodes = {nmodes} needs chains of more than {nmodes} members, the smallest linear molecule has {int(lin_sizes[0])}")
    return schedule, pairs, types, ntypes, names, period, nmodes + 1, lin_sizes, size_values


class RouseModes(_TypedAnalyzer):
    """The normal modes of the linear molecules that a bond topology defines, and their time correlations: every `period` steps (a
    sample) one pass (pse_chain_modes_compute) unfolds every molecule as Conformations does and projects every linear one onto K =
    nmodes + 1 weight rows -- row 0 the end-to-end vector R, rows p = 1 .. nmodes the Rouse modes X_p = (1/m) sum_q cos(pi p (2 q + 1) /
    (2 m)) u_q (pse_host_rouse_weights, one table per distinct size) --, adds the static second moments per molecule type, correlates
    the sample with every live origin (pse_chain_modes_correlate: all nine <X_alpha(t) X_beta(0)>) and, every `origin_every` samples,
    stores it as a new origin (pse_chain_modes_store).  Lags run from 1 to `nlags` samples by MSDSchedule; ceil(nlags / origin_every)
    <= 64 origins are kept on the device.  `bonds`, `molecule_types` (None, one code or name per molecule, or "size") and `type_names`
    as for Conformations; nmodes < the size of the smallest linear molecule.  Rings, stars and other non-linear molecules are
    skipped.  Sampling only queues work; the readers below are the only places that wait for the device.

    X is built from bond vectors alone, so it is continuous through Lees-Edwards flips wherever Conformations is.  Under shear the
    chain is deformed affinely with the flow: the xx, xy and xz entries of the tensors contain that deformation, and nothing is
    subtracted; <X_x(t) X_y(0)> and <X_y(t) X_x(0)> differ, which is why correlation_tensor keeps all nine entries.  Not measured:
    the centre-of-mass mode p = 0 and chain diffusion (MSD of the beads is analyze.MSD), mass weighting, multi-tau lag schemes.

    lags -- in steps;  counts -- origins per lag;  nlin, nlin_type;  amplitude_tensor(a) -- (K, 3, 3) <X_k X_k^T>;  amplitudes(a) --
    (K,) <X_k . X_k>, entry 0 = <R^2>;  correlation_tensor(a) -- (nlags, K, 3, 3), [alpha, beta] = <X_alpha(t) X_beta(0)>;
    autocorrelation(a) -- (nlags + 1, K): the trace over the static amplitude, lag 0 = 1;  relaxation_times(a) -- (K,) by
    relaxation_time_of;  per_molecule() -- (nlin, K, 3) at the current positions;  reset().  a = None: all types together; NaN for a
    type without linear molecules."""

    def __init__(self, integrator, bonds, nmodes=8, nlags=64, origin_every=1, molecule_types=None, type_names=None, period=1):
        import numpy as np
        import torch
        from .engine import CHAIN_MODES_STATIC, ChainModes, host_rouse_weights
        lst = getattr(bonds, "_list", None)
        pairs = lst.index if lst is not None and hasattr(lst, "index") else bonds
        (self._schedule, pairs, types, self.ntypes, self.type_names, self.period, self.K, self.linear_sizes,
         self.size_values) = _rouse_arguments(pairs, nmodes, nlags, origin_every, molecule_types, type_names, period)
        self.nmodes = self.K - 1
        with self._attach(integrator, None) as system:          # (the lines above raise before the integrator is touched)
            if int(pairs.max()) >= system.n:
                raise ValueError(f"bonds holds the index {int(pairs.max())}, the system has {system.n} particles")
            self.molecule_types = types
            self.nlags, self.origin_every, self.norigins = self._schedule.nlags, self._schedule.origin_every, self._schedule.norigins
            weights = [host_rouse_weights(int(m), self.K) for m in self.linear_sizes]
            self._modes = ChainModes(integrator.engine, pairs, self.linear_sizes, weights, types, self.ntypes, self.norigins, system.n)
            self.nmol, self.nlin, self.nlin_type = self._modes.nmol, self._modes.nlin, self._modes.nlin_type
            self.lin_mol, self.lin_size = self._modes.lin_mol, self._modes.lin_size
            dev = system.pos.device
            self._sums = torch.zeros((self.ntypes, self.K, CHAIN_MODES_STATIC), dtype=torch.float64, device=dev)
            self._corr = torch.zeros((self.nlags, self.ntypes, self.K, 3, 3), dtype=torch.float64, device=dev)

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        e, m = self.integrator.engine, self._modes
        e.chain_modes_compute(self.system.pos, m, sums=self._sums)
        self._schedule.sample(lambda slots, rows: e.chain_modes_correlate(m, slots, rows, self._corr),
                              lambda slot: e.chain_modes_store(m, slot))

    def reset(self):
        """Forget the sums, the correlations, the counts and the origins."""
        self._sums.zero_(); self._corr.zero_()
        self._schedule.reset()

    @property
    def samples(self):
        return self._schedule.samples

    @property
    def lags(self):
        import numpy as np
        return np.arange(1, self.nlags + 1) * self.period

    @property
    def counts(self):
        import numpy as np
        return np.array(self._schedule.counts, dtype=np.int64)

    def _of_type(self, x, a, axis):
        """(the sum over the types or the entry of type `a` along `axis`, the number of linear molecules behind it)"""
        if a is None:
            return x.sum(axis=axis), int(self.nlin_type.sum())
        a = self._code(a)
        return x.take(a, axis=axis), int(self.nlin_type[a])

    def amplitude_tensor(self, a=None):
        """(K, 3, 3): <X_k X_k^T> over the linear molecules of type `a` (None: of all) and the samples since reset()."""
        import numpy as np
        self._sampled()
        s, n = self._of_type(self._sums.cpu().numpy(), a, 0)
        return tensor_of(s / (self.samples * n)) if n else np.full((self.K, 3, 3), np.nan)

    def amplitudes(self, a=None):
        """(K,): <X_k . X_k>, the traces of amplitude_tensor(a); entry 0 is <R^2>."""
        import numpy as np
        return np.trace(self.amplitude_tensor(a), axis1=-2, axis2=-1)

    def correlation_tensor(self, a=None):
        """(nlags, K, 3, 3): [lag - 1, k, alpha, beta] = <X_alpha(t + lag) X_beta(t)> of functional k over the linear molecules of type
        `a` (None: of all) and the origins of that lag; NaN where a lag has no origin yet."""
        import numpy as np
        c, n = self._of_type(self._corr.cpu().numpy(), a, 1)
        den = (self.counts * n).astype(np.float64)[:, None, None, None]
        return np.divide(c, den, out=np.full(c.shape, np.nan), where=den > 0.0)

    def autocorrelation(self, a=None):
        """(nlags + 1, K): <X_k(t + lag) . X_k(t)> / <X_k . X_k> for lag = 0 .. nlags samples; row 0 is 1."""
        import numpy as np
        amp = self.amplitudes(a)
        tr = np.trace(self.correlation_tensor(a), axis1=-2, axis2=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.concatenate([np.where(np.isnan(amp), np.nan, 1.0)[None, :], tr / amp[None, :]], axis=0)

    def relaxation_times(self, a=None):
        """(K,): relaxation_time_of every column of autocorrelation(a), in steps; entry 0 is the relaxation time of R."""
        import numpy as np
        c = self.autocorrelation(a)
        t = np.concatenate([[0], self.lags])
        return np.array([relaxation_time_of(t, c[:, k]) for k in range(self.K)])

    def per_molecule(self):
        """(nlin, K, 3) float64: X_k of every linear molecule (lin_mol, lin_size) at the system's current positions.  One pass and one
        copy; no sample is taken."""
        import torch
        out = torch.empty((self.nlin, self.K, 3), dtype=torch.float64, device=self.system.pos.device)
        self.integrator.engine.chain_modes_compute(self.system.pos, self._modes, out=out)
        return out.cpu().numpy()


def _isf_analyzer_arguments(modes, nlags, origin_every, types, type_names, period, self_part, collective):
    """What IntermediateScattering checks before it touches the device.  Returns (schedule, types uint32 or None, ntypes, modes int32
    (nk, 3), names or None, period)."""
    schedule = MSDSchedule(nlags, origin_every)
    types, ntypes, names, period = _typed_arguments(types, type_names, period)
    types, ntypes, modes, _ = _isf_arguments(types, ntypes, modes, schedule.norigins)
    if not (self_part or collective):
        raise ValueError("self_part and collective are both off: nothing to measure")
    return schedule, types, ntypes, modes, names, period


class IntermediateScattering(_TypedAnalyzer):
    """Intermediate scattering functions of a run over many time origins: every `period` steps (a sample) the fractional coordinates
    of the integrator's group and its densities rho_a(m) on the integer modes `modes` (nk, 3) go into a buffer on the device
    (pse_isf_sample, which also adds the static Re(rho_a conj rho_b) exactly as StructureFactor does), the sample is correlated with
    every live origin (pse_isf_correlate) and, every `origin_every` samples, stored as a new origin (pse_isf_store).  Lags run from 1
    to `nlags` samples by MSDSchedule; ceil(nlags / origin_every) <= 64 origins are kept.  `types`, `type_names`: as for RDF; at most 8
    types, 4096 modes, |m_i| <= 4096.  Sampling only queues work; the readers below are the only places that wait for the device.

    Self part: F_s(m, t) = <exp(-2 pi i m.(s_j(t) - s_j(0)))> over the particles of a type, s the fractional coordinates: no images and
    no unwrapping are needed, a particle that wrapped around the box gives the same value.  Collective part: F_ab(m, t) =
    <rho_a(m, t) conj rho_b(m, 0)> / sqrt(N_a N_b), a the type NOW and b the type AT THE ORIGIN; both orders are kept, they differ
    under shear.  In a tilting box an integer mode is the ADVECTED wave vector k(t) = 2 pi (mx/Lx, my/Ly - xy(t) mx/Lx, mz/Lz), the
    usual choice under shear: purely affine motion leaves F_s = 1.  A Lees-Edwards flip relabels the integer modes (s_x changes by a
    multiple of s_y), so when system.tilt_flips differs from its value at the previous sample the live origins are dropped
    (MSDSchedule.drop_origins; sums and counts stay): lags that span a flip are never sampled, and with a flip every T samples the
    lags >= T stay empty (NaN).  `k` and `shell_average` raise ValueError when the samples' boxes differ, as StructureFactor's do.

    samples;  lags -- in steps;  counts -- origins per lag;  self_sums -- (nlags, ntypes, nk) complex;  collective_sums -- (nlags,
    ntypes, ntypes, nk);  static_sums -- (npt, nk);  boxes;  Fs(a) -- (nlags, nk) = Re self / (counts N_a);  F(a, b) = coll / (counts
    sqrt(N_a N_b)), F() the total sum_ab coll / (counts N);  S(a, b), S() -- the static structure factor of the samples;  f(a, b) =
    F / S;  k -- (nk, 3);  shell_average(values, nbins, kmax=None) -- the mean of values (nk,) or (rows, nk) over bins of |k|:
    (centres, means, counts);  relaxation_times(which="self" | "collective", a=None) -- (nk,), in steps, by relaxation_time_of;
    reset().  a = None: all types together; NaN where a lag has no origin yet or a type no particle."""

    def __init__(self, integrator, modes, nlags, origin_every=1, types=None, type_names=None, period=1, self_part=True, collective=True):
        import torch
        self._schedule, types, self.ntypes, self.modes, self.type_names, self.period = _isf_analyzer_arguments(
            modes, nlags, origin_every, types, type_names, period, self_part, collective)   # (raises before the device is touched)
        with self._attach(integrator, types) as system:
            self.nlags, self.origin_every, self.norigins = self._schedule.nlags, self._schedule.origin_every, self._schedule.norigins
            self._isf = ScatteringOrigins(integrator.engine, types, self.ntypes, self.modes, self.norigins, system.n)
            self.npt, self.nk = self._isf.npt, self._isf.nk
            dev = system.pos.device
            self._self = torch.zeros((self.nlags, self.ntypes, self.nk, 2), dtype=torch.float64, device=dev) if self_part else None
            self._coll = torch.zeros((self.nlags, self.ntypes, self.ntypes, self.nk), dtype=torch.float64, device=dev) if collective else None
            self._static = torch.zeros((self.npt, self.nk), dtype=torch.float64, device=dev)
            self.boxes, self._flips = [], None

    def analyze(self, timestep):
        if not self._due(timestep):
            return
        s, e, f = self.system, self.integrator.engine, self._isf
        if self._flips is not None and s.tilt_flips != self._flips:
            self._schedule.drop_origins()   # (the stored origins are in the old labelling of the modes)
        self._flips = s.tilt_flips
        e.isf_sample(s.pos, f, static_sums=self._static, group=self.integrator.group.members)
        self._schedule.sample(lambda slots, rows: e.isf_correlate(f, slots, rows, self._self, self._coll), lambda slot: e.isf_store(f, slot))
        self.boxes.append(tuple(s.box))

    def reset(self):
        """Forget the sums, the counts, the boxes and the origins."""
        for t in (self._self, self._coll, self._static):
            if t is not None:
                t.zero_()
        self._schedule.reset()
        self.boxes, self._flips = [], None

    @property
    def samples(self):
        return self._schedule.samples

    @property
    def lags(self):
        import numpy as np
        return np.arange(1, self.nlags + 1) * self.period

    @property
    def counts(self):
        import numpy as np
        return np.array(self._schedule.counts, dtype=np.int64)

    @property
    def self_sums(self):
        if self._self is None:
            raise ValueError("this analyzer was made with self_part=False")
        r = self._self.cpu().numpy()
        return r[..., 0] + 1j * r[..., 1]

    @property
    def collective_sums(self):
        if self._coll is None:
            raise ValueError("this analyzer was made with collective=False")
        return self._coll.cpu().numpy()

    @property
    def static_sums(self):
        return self._static.cpu().numpy()

    def _per_lag(self, tot, n):
        import numpy as np
        den = self.counts.astype(np.float64)[:, None] * n
        return np.divide(tot, den, out=np.full(tot.shape, np.nan), where=den > 0.0)

    def Fs(self, a=None):
        """(nlags, nk): the self part of type `a` (None: of all particles)."""
        import numpy as np
        r, nc = self.self_sums.real, self._type_counts()
        return self._per_lag(r.sum(axis=1), float(np.sum(nc))) if a is None else self._per_lag(r[:, self._code(a)], float(nc[self._code(a)]))

    def F(self, a=None, b=None):
        """(nlags, nk): F_ab, a the type now and b the type at the origin; without arguments the total."""
        import numpy as np
        if (a is None) != (b is None):
            raise ValueError("F() takes both types or neither")
        c, nc = self.collective_sums, self._type_counts()
        if a is None:
            return self._per_lag(c.sum(axis=(1, 2)), float(np.sum(nc)))
        a, b = self._code(a), self._code(b)
        return self._per_lag(c[:, a, b], math.sqrt(float(nc[a]) * float(nc[b])))

    def S(self, a=None, b=None):
        """S_ab per mode, (nk,), of the samples taken; without arguments the total S."""
        if (a is None) != (b is None):
            raise ValueError("S() takes both types or neither")
        self._sampled()
        if a is not None:
            a, b = self._code(a), self._code(b)
        return S_of_sums(self.static_sums, self.samples, self._type_counts(), a, b)

    def f(self, a=None, b=None):
        """(nlags, nk): F / S, the normalised collective part; NaN or inf at a mode where S vanishes."""
        import numpy as np
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.F(a, b) / self.S(a, b)[None, :]

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

    def shell_average(self, values, nbins, kmax=None):
        """The mean of `values` -- (nk,), or (rows, nk) row by row -- over nbins bins of |k|: (centres, means, counts)."""
        import numpy as np
        k, values = self.k, np.asarray(values, dtype=np.float64)   # (the differing-box check comes first)
        if values.ndim == 1:
            return shell_average_of(k, values, nbins, kmax)
        if values.ndim != 2 or values.shape[1] != self.nk:
            raise ValueError(f"values must be ({self.nk},) or (rows, {self.nk})")
        out = [shell_average_of(k, row, nbins, kmax) for row in values]
        return out[0][0], np.stack([o[1] for o in out]), out[0][2]

    def relaxation_times(self, which="self", a=None):
        """(nk,): the time, in steps, at which F_s(m, t) (which="self") or f(m, t) = F / S of type `a` with itself (which="collective";
        a = None: the totals) first falls to 1/e, by relaxation_time_of with the value 1 at lag 0; NaN where it never does."""
        import numpy as np
        if which not in ("self", "collective"):
            raise ValueError('which must be "self" or "collective"')
        c = self.Fs(a) if which == "self" else self.f(a, a)
        t = np.concatenate([[0], self.lags])
        return np.array([relaxation_time_of(t, np.concatenate([[1.0], c[:, q]])) for q in range(self.nk)])
