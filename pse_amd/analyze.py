"""Structure analyzers: what is measured from the positions during a run, next to the path.  RDF samples the pair-distance histogram
of the integrator's engine (pse_pair_hist_accumulate: one walk of the cell list the step uses anyway) into a device tensor and turns
the counts into the radial distribution functions g_ab(r) and coordination numbers when they are read."""
import math

from .engine import PairHistogram, _pair_hist_arguments, pair_type_index
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
