"""Force providers: what fills `net_force` before the integrator consumes it (HOOMD's force computes in the reference,
PSEv1/Stokes.cc:447; its example script has none).  SURVEY.md 8 f4: the step either side of the hot path, kept minimal."""
import math

from .engine import (ANGLE_KINDS, BOND_KINDS, DIHEDRAL_KINDS, AngleList, BondList, DihedralList, ExclusionList, TypedTable, _per_type,
                     _topology_arrays, _type_params, _typed_tables, _typed_types)


class _ObsProvider:
    """What the pair, bond, angle and dihedral providers share: the eight device doubles of the most recent fused call -- U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz,
    npairs -- where that call writes them (a row of a StressLog on a sample step, a buffer of the provider's own otherwise), and the
    host-side readers.  A subclass sets NAME (what its messages call it) and makes the call in compute(): one force pass of the
    integrator's engine (integrate.PSEv1.engine, engine._ForcePasses), added to net_force."""

    NAME = "pair provider"

    def __init__(self, integrator, virial):
        self.integrator = integrator
        self._fused = bool(virial)
        self._own = None     # where a fused call writes when no log takes the sample
        self._obs = None     # the eight device doubles of the most recent fused call: U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs
        self.log = None      # a StressLog registers itself here
        integrator.system.forces.append(self)

    def _pass(self, timestep):
        """The keywords every pass takes: the forces are added, and the eight doubles go where _fused_out says."""
        return dict(accumulate=True, out=self._fused_out(timestep), observables=self._fused)

    def _fused_out(self, timestep):
        """The eight doubles the call of this step writes, recorded as the most recent ones; None without virial=True."""
        if not self._fused:
            return None
        out = self.log.row(timestep) if self.log is not None else None
        if out is None:
            if self._own is None:
                import torch
                self._own = torch.zeros(8, dtype=torch.float64, device=self.integrator.system.pos.device)
            out = self._own
        self._obs = out
        return out

    def _observables(self):
        if self._obs is None:
            raise RuntimeError(f"no observables yet: {self.NAME}(..., virial=True) and one compute() first")
        return self._obs.cpu().numpy()

    @property
    def energy(self):
        """U = the sum of the pair energies (HarmonicRepulsion: k/2 (sigma - r)^2) at the most recent compute()."""
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


def exclusion_pairs(bonds=None, angles=None, dihedrals=None):
    """HOOMD's exclusion sets (nlist.reset_exclusions(['bond', 'angle', 'dihedral'])) of the index arrays that are given: both
    members of a bond (nb, 2), the two ends of an angle (na, 3: columns 0 and 2), the two ends of a dihedral (nd, 4: columns 0 and
    3).  Returns their union as an (npairs, 2) int64 array of (smaller, larger) index pairs, each once, in ascending order.  Needs no
    device; ValueError if nothing was passed."""
    import numpy as np
    parts = []
    for name, a, cols, ends in (("bonds", bonds, 2, (0, 1)), ("angles", angles, 3, (0, 2)), ("dihedrals", dihedrals, 4, (0, 3))):
        if a is None:
            continue
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] != cols or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must be an integer (count, {cols}) array of particle indices")
        parts.append(a[:, ends].astype(np.int64))
    if not parts:
        raise ValueError("from_topology needs at least one of bonds, angles, dihedrals")
    p = np.concatenate(parts, axis=0)
    return np.unique(np.stack([p.min(axis=1), p.max(axis=1)], axis=1), axis=0)


class Exclusions:
    """Pairs that the pair providers skip (pse_exclusions_create; HOOMD's nlist.reset_exclusions): `pairs` is an (npairs, 2) integer
    array of particle indices into the system's arrays; order and duplicates do not matter.  Pass the object as `exclusions=` to
    TablePair or HarmonicRepulsion: the excluded pairs then add nothing to the forces, the energy, the virial or npairs.  In HOOMD
    bonded pairs are excluded by default; here nothing is excluded unless asked for.  The set is copied to the device once, here."""

    def __init__(self, integrator, pairs):
        pairs, _ = _topology_arrays(pairs, None, 2, "pairs", "pair")
        self.integrator, self.npairs_listed = integrator, pairs.shape[0]
        self.list = ExclusionList(integrator.engine, pairs, integrator.system.n)

    @classmethod
    def from_topology(cls, integrator, bonds=None, angles=None, dihedrals=None):
        """The exclusions HOOMD derives from a topology (exclusion_pairs): the union of what is passed."""
        return cls(integrator, exclusion_pairs(bonds, angles, dihedrals))


def _excl_list(integrator, exclusions):
    """The ExclusionList of an Exclusions object for a provider of `integrator`, or None."""
    if exclusions is None:
        return None
    if not isinstance(exclusions, Exclusions) or exclusions.integrator is not integrator:
        raise ValueError("exclusions must be a forces.Exclusions made on the same integrator")
    return exclusions.list


class HarmonicRepulsion(_ObsProvider):
    """F_i = sum_j k (sigma - r)(r_i - r_j)/r for minimum-image pairs with r < sigma (sigma = 2a: contact of unit spheres).
    Evaluated on the integrator's own cell list; sigma must not exceed the hydrodynamic real-space cutoff.

    virial=True: compute() makes the fused call (pse_pair_repulsion_virial) instead -- the same forces, plus the potential energy
    and the virial of the same pass in eight device doubles.  `energy`, `virial` and `stress()` copy them to the host when they are
    read (that waits for the stream); a StressLog samples them without any wait.

    exclusions: an Exclusions object whose pairs do not repel (pse_pair_repulsion_excl); None: every pair in range acts."""

    NAME = "HarmonicRepulsion"

    def __init__(self, integrator, k, sigma=2.0, virial=False, exclusions=None):
        self.k, self.sigma = float(k), float(sigma)
        self._excl = _excl_list(integrator, exclusions)
        super().__init__(integrator, virial)

    def compute(self, timestep):
        s, g, eng = self.integrator.system, self.integrator.group, self.integrator.engine
        if not self._fused:
            if len(g):   # (with virial=True an empty group is refused by the C-ABI: no device code here could write zeros to the eight doubles)
                eng.pair_repulsion(s.pos, s.net_force, self.k, self.sigma, group=g.members, accumulate=True, exclusions=self._excl)
            return
        eng.pair_repulsion_virial(s.pos, s.net_force, self.k, self.sigma, group=g.members, accumulate=True, out=self._fused_out(timestep),
                                  exclusions=self._excl)


class TablePair(_ObsProvider):
    """A tabulated central pair potential (pse_pair_table; HOOMD's pair.table for the one particle type here): `table` is a NumPy or
    torch (width, 2) array, 2 <= width <= 2048, of V and F -- the pair energy and the magnitude of the radial force, positive for a
    repulsion -- at the nodes r_k = rmin + k (rmax - rmin)/(width - 1); both are linear between the nodes.  Pairs with
    rmin <= r < rmax act, the rest contribute nothing; rmax must not exceed the hydrodynamic real-space cutoff.  The table is copied
    to the device once, here.

    virial=True: the same call also writes the potential energy, the virial and the pair count: `energy`, `virial`, `stress()`,
    `npairs` and StressLog as for HarmonicRepulsion.

    exclusions: an Exclusions object whose pairs the table does not act on (pse_pair_table_excl) -- what HOOMD does by default for
    bonded pairs; None: every pair in range acts."""

    NAME = "TablePair"

    def __init__(self, integrator, table, rmin, rmax, virial=False, exclusions=None):
        import torch
        t = torch.as_tensor(table).detach().to(dtype=torch.float64)
        if t.dim() != 2 or t.shape[1] != 2 or not 2 <= t.shape[0] <= 2048:
            raise ValueError("table must have shape (width, 2) with 2 <= width <= 2048: V and F at the nodes")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("table has non-finite entries")
        self.rmin, self.rmax = float(rmin), float(rmax)
        if not 0.0 <= self.rmin < self.rmax < float("inf"):
            raise ValueError("need 0 <= rmin < rmax, both finite")
        self.table = t.to(integrator.system.pos.device).contiguous().clone()
        self._excl = _excl_list(integrator, exclusions)
        super().__init__(integrator, virial)

    @classmethod
    def from_functions(cls, integrator, V, F, rmin, rmax, width, virial=False, exclusions=None):
        """Sample the callables V(r) and F(r) = -dV/dr (one float in, one float out) at the `width` nodes."""
        import numpy as np
        width, rmin, rmax = int(width), float(rmin), float(rmax)
        if width < 2:
            raise ValueError("width must be at least 2")
        r = rmin + np.arange(width) * ((rmax - rmin) / (width - 1))
        return cls(integrator, np.array([[float(V(x)), float(F(x))] for x in r]), rmin, rmax, virial=virial, exclusions=exclusions)

    def compute(self, timestep):
        s = self.integrator.system
        self.integrator.engine.pair_table(s.pos, s.net_force, self.table, self.rmin, self.rmax, group=self.integrator.group.members,
                                          exclusions=self._excl, **self._pass(timestep))


def _typed_arguments(types, tables, type_names):
    """What TypedTablePair checks before it touches the device: `types` and the keys of `tables` as integers -- a name is its
    position in `type_names` --, then the arrays of pse_typed_table_create (engine._typed_tables).  Returns (types uint32, ntypes,
    widths, rmin, rmax, entries)."""
    if not isinstance(tables, dict) or not tables:
        raise ValueError("tables must be a non-empty dict {(a, b): (table, rmin, rmax)}")
    names = None if type_names is None else list(type_names)
    if names is not None and (len(set(names)) != len(names) or not all(isinstance(v, str) for v in names)):
        raise ValueError("type_names must be distinct strings")

    def code(v):
        if not isinstance(v, str):
            return v
        if names is None:
            raise ValueError(f"type name {v!r}: names need a type_names= list")
        if v not in names:
            raise ValueError(f"unknown type name {v!r}: type_names is {names}")
        return names.index(v)

    types = [code(v) for v in (types.tolist() if hasattr(types, "tolist") else list(types))]
    coded = {}
    for key, value in tables.items():
        k = tuple(code(v) for v in key) if isinstance(key, tuple) else key
        if k in coded:
            raise ValueError(f"tables names the pair {key!r} twice, by name and by number")
        coded[k] = value
    types, ntypes = _typed_types(types, coded)
    return (types, max(ntypes, len(names or ()))) + _typed_tables(coded, max(ntypes, len(names or ())))


class TypedTablePair(_ObsProvider):
    """One tabulated pair potential per pair of particle types (pse_pair_table_typed; HOOMD's pair.table with pair_coeff.set('A', 'B',
    ...)): `types` gives every particle of the system its type -- integers, or names with a `type_names=` list, whose order numbers
    them --, `tables` is a dict {(a, b): (table, rmin, rmax)} with `table`, `rmin` and `rmax` as for TablePair.  A key may name its two
    types in either order (both orders of one pair are a ValueError); a pair of types without a key does not interact.  At most 8
    types, and at most 3584 table entries over all pairs of types.  Types and tables are copied to the device once, here.

    virial=True: `energy`, `virial`, `stress()`, `npairs` and StressLog as for TablePair -- with all pair types but one off, `npairs`
    counts the contacts of that pair of types.  exclusions: as for TablePair."""

    NAME = "TypedTablePair"

    def __init__(self, integrator, types, tables, virial=False, exclusions=None, type_names=None):
        types, self.ntypes, width, rmin, rmax, entries = _typed_arguments(types, tables, type_names)   # (raises before the device is touched)
        n = integrator.system.n
        if types.shape[0] != n:
            raise ValueError(f"types has {types.shape[0]} entries, the system {n} particles")
        self.types, self.widths, self.rmin, self.rmax, self.tables = types, width, rmin, rmax, entries
        self._excl = _excl_list(integrator, exclusions)
        self._typed = TypedTable.from_arrays(integrator.engine, types, self.ntypes, width, rmin, rmax, entries)
        super().__init__(integrator, virial)

    @classmethod
    def from_functions(cls, integrator, types, functions, virial=False, exclusions=None, type_names=None):
        """`functions`: {(a, b): (V, F, rmin, rmax, width)} -- the callables V(r) and F(r) = -dV/dr (one float in, one float out) of
        each pair of types, sampled at `width` nodes as TablePair.from_functions samples them."""
        import numpy as np
        if not isinstance(functions, dict) or not functions:
            raise ValueError("functions must be a non-empty dict {(a, b): (V, F, rmin, rmax, width)}")
        tables = {}
        for key, value in functions.items():
            if not (isinstance(value, (tuple, list)) and len(value) == 5):
                raise ValueError(f"functions[{key!r}] must be (V, F, rmin, rmax, width)")
            V, F, rmin, rmax, width = value[0], value[1], float(value[2]), float(value[3]), int(value[4])
            if width < 2:
                raise ValueError("width must be at least 2")
            r = rmin + np.arange(width) * ((rmax - rmin) / (width - 1))
            tables[key] = (np.array([[float(V(x)), float(F(x))] for x in r]), rmin, rmax)
        return cls(integrator, types, tables, virial=virial, exclusions=exclusions, type_names=type_names)

    def table(self, a, b):
        """The (width, 2) table of the pair of types (a, b), integers, as it was copied to the device; None if the pair is off."""
        from .engine import pair_type_index
        p = pair_type_index(int(a), int(b), self.ntypes)
        first = int(self.widths[:p].sum())
        return self.tables[first:first + int(self.widths[p])] if self.widths[p] else None

    def compute(self, timestep):
        s = self.integrator.system
        self.integrator.engine.pair_table_typed(s.pos, s.net_force, self._typed, group=self.integrator.group.members, exclusions=self._excl,
                                                **self._pass(timestep))


class _TopologyProvider(_ObsProvider):
    """What Bonds, Angles and Dihedrals share: the provider holds a BondList, AngleList or DihedralList of the integrator's engine."""

    def _create(self, integrator, List, index, types, kind, k, x):
        """The checks, all before the integrator is touched, and the list: `kind`, `k` and `x` are scalars -- a scalar serves every
        type -- or sequences of one length; with List.WIDTH = w parameters per type `k` is one w-tuple or a sequence of them and `x`
        is None.  Returns the three per-type tuples as the provider shows them (the third None with a width)."""
        xname, what, width = List.X, List.WHAT, List.WIDTH
        if width is not None:
            import numpy as np
            if np.ndim(k) not in (1, 2) or np.shape(k)[-1] != width:
                raise ValueError(f"{xname} must be one {width}-tuple or a sequence of them (one per {what} type)")
            k = [tuple(k)] if np.ndim(k) == 1 else [tuple(v) for v in k]
            x = [None] * len(k)
        kind, k, x = _per_type(kind), _per_type(k), _per_type(x)
        nt = max(len(kind), len(k), len(x))
        kind, k, x = (v * nt if len(v) == 1 else v for v in (kind, k, x))
        if not len(kind) == len(k) == len(x) == nt:
            raise ValueError(f"kind, k and {xname} must be scalars or sequences of one length (one entry per {what} type)")
        for v in kind:
            if v not in List.KINDS:
                raise ValueError(f"{what} kind must be one of {sorted(List.KINDS)}, not {v!r}")
        _, k_a, x_a = _type_params(kind, k, x, xname, List.KINDS, what, width)
        index, types = _topology_arrays(index, types, List.COLS, List.INDEX, what)
        self._list = List(integrator.engine, index, types, kind, k_a, x_a, integrator.system.n)
        return tuple(kind), tuple(map(tuple, k_a.tolist())) if width else tuple(k_a.tolist()), None if x_a is None else tuple(x_a.tolist())

    def compute(self, timestep):
        s = self.integrator.system
        self._list.forces(s.pos, s.net_force, **self._pass(timestep))


class Bonds(_TopologyProvider):
    """Harmonic and FENE bonds (pse_bond_forces; HOOMD's bond.harmonic and bond.fene): `pairs` is an (nbonds, 2) integer array of
    particle indices into the system's arrays.  kind = "harmonic": V = k/2 (r - r0)^2; "fene": V = -k/2 r0^2 ln(1 - (r/r0)^2), r < r0.
    `kind`, `k` and `r0` are scalars (one bond type) or sequences with one entry per type, and `types` then gives each bond's type
    (None: all type 0).  The topology is copied to the device once, here.  Duplicate bonds act once each.  A bond must stay shorter
    than half the smallest perpendicular box width: the minimum image is the nearest one only there.  A FENE bond found at r >= r0
    contributes nothing and is counted in `overstretched` (HOOMD aborts there).

    virial=True: the same call also writes the bond energy, the virial and the number of bonds that acted: `energy`, `virial`,
    `stress()`, `nbonds` and StressLog as for HarmonicRepulsion."""

    NAME = "Bonds"
    KINDS = BOND_KINDS

    def __init__(self, integrator, pairs, kind="harmonic", k=1.0, r0=1.0, types=None, virial=False):
        self.kind, self.k, self.r0 = self._create(integrator, BondList, pairs, types, kind, k, r0)
        super().__init__(integrator, virial)

    @property
    def nbonds(self):
        """The number of bonds that acted at the most recent compute() (the count the pair providers call npairs)."""
        return self.npairs

    @property
    def overstretched(self):
        """FENE bonds found at r >= r0 by all compute() calls so far (waits for the stream)."""
        return self._list.overstretched


class Angles(_TopologyProvider):
    """Harmonic and cosine-squared angles (pse_angle_forces; HOOMD's angle.harmonic and angle.cosinesq): `triples` is an (nangles, 3)
    integer array of particle indices into the system's arrays, (end, vertex, end).  With theta the angle at the vertex between the
    two arms, kind = "harmonic": V = k/2 (theta - theta0)^2; "cosinesq": V = k/2 (cos theta - cos theta0)^2.  `kind`, `k` and `theta0`
    (radians, in [0, pi]) are scalars (one angle type) or sequences with one entry per type, and `types` then gives each angle's type
    (None: all type 0).  The topology is copied to the device once, here.  Duplicate angles act once each.  An arm must stay shorter
    than half the smallest perpendicular box width: the minimum image is the nearest one only there.  Within sin(theta) < 1e-3 of the
    straight or the folded angle the harmonic force is capped (HOOMD's rule) and no longer exactly the gradient of the energy.

    virial=True: the same call also writes the angle energy, the virial (traceless) and the number of angles that acted: `energy`,
    `virial`, `stress()`, `nangles` and StressLog as for HarmonicRepulsion."""

    NAME = "Angles"
    KINDS = ANGLE_KINDS

    def __init__(self, integrator, triples, kind="harmonic", k=1.0, theta0=math.pi, types=None, virial=False):
        self.kind, self.k, self.theta0 = self._create(integrator, AngleList, triples, types, kind, k, theta0)
        super().__init__(integrator, virial)

    @property
    def nangles(self):
        """The number of angles that acted at the most recent compute() (the count the pair providers call npairs)."""
        return self.npairs


class Dihedrals(_TopologyProvider):
    """Harmonic and OPLS dihedrals (pse_dihedral_forces; HOOMD's dihedral.harmonic and dihedral.opls): `quads` is an (ndihedrals, 4)
    integer array of particle indices (i, j, k, l) into the system's arrays.  phi is the IUPAC dihedral angle of the three arms
    i-j, j-k, k-l: the planar cis arrangement is 0, trans is pi (this convention whatever sign a given HOOMD version uses).
    kind = "harmonic": params (k, d, mult, phi0), V = k/2 (1 + d cos(mult phi - phi0)), d = -1 or +1, mult an integer in 1..6;
    "opls": params (k1, k2, k3, k4), V = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2phi) + k3 (1 + cos 3phi) + k4 (1 - cos 4phi)].  `kind` is
    a scalar or a sequence with one entry per type, `params` one 4-tuple or one per type, and `types` then gives each dihedral's type
    (None: all type 0).  The topology is copied to the device once, here.  Duplicate dihedrals act once each.  An arm must stay
    shorter than half the smallest perpendicular box width: the minimum image is the nearest one only there.  A dihedral with three
    consecutive collinear particles has no angle and does nothing.

    virial=True: the same call also writes the dihedral energy, the virial (traceless) and the number of dihedrals that acted:
    `energy`, `virial`, `stress()`, `ndihedrals` and StressLog as for HarmonicRepulsion."""

    NAME = "Dihedrals"
    KINDS = DIHEDRAL_KINDS

    def __init__(self, integrator, quads, kind="harmonic", params=(1.0, 1.0, 1.0, 0.0), types=None, virial=False):
        self.kind, self.params, _ = self._create(integrator, DihedralList, quads, types, kind, params, None)
        super().__init__(integrator, virial)

    @property
    def ndihedrals(self):
        """The number of dihedrals that acted at the most recent compute() (the count the pair providers call npairs)."""
        return self.npairs


def _sym3(w):
    import numpy as np
    xx, xy, xz, yy, yz, zz = (float(v) for v in w)
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


class StressLog:
    """Energy and stress of a HarmonicRepulsion, TablePair, Bonds, Angles or Dihedrals(..., virial=True) every `period` steps, in a device ring of `capacity` rows: on a
    sample step the provider's fused call writes its eight doubles straight into the next row, the step number, the box tilt and the
    volume are noted on the host, and nothing waits for the device until table() is read.  Once full, the oldest rows are replaced."""

    COLUMNS = ("timestep", "xy", "U", "sxx", "sxy", "sxz", "syy", "syz", "szz", "npairs")

    def __init__(self, provider, period, capacity):
        import torch
        if not getattr(provider, "_fused", False):
            raise ValueError(f"StressLog needs a {getattr(provider, 'NAME', HarmonicRepulsion.NAME)}(..., virial=True)")
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
