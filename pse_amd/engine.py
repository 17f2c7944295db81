"""Thin Python owner of a pse_handle: torch tensors in, torch tensors out, everything through the C-ABI.

Arrays follow HOOMD's layout with Scalar = double: pos/vel/force are (N,4) float64 CUDA tensors
(x,y,z,type|mass|energy), accel (N,3) float64, image (N,3) int32, group_members (N,) int32/uint32.
"""
import ctypes
import math

from . import _lib
from ._lib import pse_info, pse_params


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _is_cuda(t, *dtypes):
    """Is `t` a contiguous CUDA tensor of one of `dtypes`?  Every caller adds its own shape clause and its own message."""
    import torch
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and t.is_contiguous()


def _chk4(t, name, n=None):
    import torch
    if not (_is_cuda(t, torch.float64) and t.dim() == 2 and t.shape[1] == 4):
        raise ValueError(f"{name} must be a contiguous (N,4) float64 CUDA tensor")
    if n is not None and t.shape[0] < n:
        raise ValueError(f"{name} has fewer than {n} rows")


def _chk_group(g, name="group"):
    import torch
    if g is None:
        return
    if not (_is_cuda(g, torch.int32, torch.uint32) and g.dim() == 1):
        raise ValueError(f"{name} must be a contiguous 1-D int32/uint32 CUDA tensor (the C-ABI reads unsigned int indices)")


def _chk_arr(t, name, cols, dtype, n):
    if not (_is_cuda(t, dtype) and t.dim() == 2 and t.shape[1] == cols and t.shape[0] >= n):
        raise ValueError(f"{name} must be a contiguous (N>={n},{cols}) {dtype} CUDA tensor")


# the near-field operator of the Lanczos iteration (pse_set_lanczos_operator): name -> enum pse_lanczos_operator
LANCZOS_OPERATORS = {"records16": 0, "fp64": 1}


def _lanczos_operator_code(name):
    if name not in LANCZOS_OPERATORS:
        raise ValueError(f"lanczos_operator must be one of {sorted(LANCZOS_OPERATORS)}, not {name!r}")
    return LANCZOS_OPERATORS[name]


def host_select_params(box, xi=0.5, error=1e-3, max_strain=0.5, grid=(0, 0, 0), P=0, rcut=0.0):
    """Parameter rule of Stokes::setParams (PSEv1/Stokes.cc:129-236,319), host only."""
    lib = _lib.load()
    p = pse_params(n_max=1, Lx=box[0], Ly=box[1], Lz=box[2], xy=box[3] if len(box) > 3 else 0.0, xi=xi, error=error,
                   max_strain=max_strain, seed=0, Nx=grid[0], Ny=grid[1], Nz=grid[2], P=P, rcut=rcut, device=-1,
                   n_slabs=1, slab_rank=0)
    info = pse_info()
    _lib.check(lib.pse_host_select_params(ctypes.byref(p), ctypes.byref(info)))
    return info.as_dict()


def host_realspace_table(xi, rcut):
    """The real-space table of (xi, rcut) as the device holds it, host only: array (n_intervals, 2, 10) -- per interval of width 1/8
    the coefficients of f_w and of g_w in powers of t = 2 (8 r - k) - 1, lowest first."""
    import numpy as np
    lib = _lib.load()
    n = ctypes.c_int(0)
    lib.pse_host_realspace_table(xi, rcut, 0, None, ctypes.byref(n))   # sizes the array (and reports a bad xi or rcut below)
    coef = np.zeros(max(n.value, 0) * 20)
    _lib.check(lib.pse_host_realspace_table(xi, rcut, len(coef), coef.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(n)))
    return coef.reshape(n.value, 2, 10)


def host_lanczos_sqrt_e1(alpha, beta):
    """t = T^{1/2} e_1 (host); alpha[0..m), beta[0..m] with beta[0] unused."""
    import numpy as np
    lib = _lib.load()
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    b = np.ascontiguousarray(beta, dtype=np.float64)
    t = np.zeros(len(a))
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(lib.pse_host_lanczos_sqrt_e1(len(a), a.ctypes.data_as(dp), b.ctypes.data_as(dp), t.ctypes.data_as(dp)))
    return t


LZ_DECISION_FIELDS = ("m_lo", "m_hi", "done_iters", "have_last_beta", "pending_beta", "first", "last", "normalised", "m_max", "tol", "seq")
LZ_MIRROR_FIELDS = ("m", "stepnorm", "status", "seq", "open")


def debug_lz_decide_supported(m_hi):
    """Whether the device-side Lanczos decision can check the sizes m_hi - 1 and m_hi (pse_debug_lz_decide_supported)."""
    return bool(_lib.load().pse_debug_lz_decide_supported(int(m_hi)))


def debug_lz_decide(scal, decisions, open0=0.0):
    """The device-side Lanczos decision on given coefficients (pse_debug_lz_decide; current device, no engine).  scal: the image of
    the device scalars (400 doubles: alpha at 0, beta at 128, the norm at 256); decisions: dicts of LZ_DECISION_FIELDS (missing
    ones 0) in the order a driver issues them; open0: the host mirror's count of open calls before the first.  Returns one dict per
    launch: done, m_final, checked, status, stepnorm, t_prev[104], coef[104] and mirror (dict of LZ_MIRROR_FIELDS)."""
    return _lz_decide("pse_debug_lz_decide", scal, decisions, open0)


def host_lz_decide(scal, decisions, open0=0.0):
    """The Lanczos decision of the host-checked drivers on given coefficients (pse_host_lz_decide; no device): arguments and result
    as debug_lz_decide; a decision may check any number of sizes."""
    return _lz_decide("pse_host_lz_decide", scal, decisions, open0)


def _lz_decide(entry, scal, decisions, open0):
    import numpy as np
    lib = _lib.load()
    s = np.ascontiguousarray(scal, dtype=np.float64)
    if s.shape != (_lib.PSE_DEBUG_LZ_NSCAL,):
        raise ValueError(f"scal must hold {_lib.PSE_DEBUG_LZ_NSCAL} doubles")
    n = len(decisions)
    dec = (_lib.pse_debug_lz_decision * max(n, 1))()
    for k, d in enumerate(decisions):
        unknown = set(d) - set(LZ_DECISION_FIELDS)
        if unknown:
            raise ValueError(f"decision {k}: unknown fields {sorted(unknown)}")
        for name in LZ_DECISION_FIELDS:
            setattr(dec[k], name, (float if name in ("tol", "seq") else int)(d.get(name, 0)))
    out = (_lib.pse_debug_lz_outcome * max(n, 1))()
    _lib.check(getattr(lib, entry)(s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n, dec, float(open0), out))
    return [dict(done=o.done, m_final=o.m_final, checked=o.checked, status=o.status, stepnorm=o.stepnorm,
                 t_prev=np.array(o.t_prev), coef=np.array(o.coef), mirror=dict(zip(LZ_MIRROR_FIELDS, o.mirror))) for o in out[:n]]


def _chk_out8(out, pos):
    """Where a pass writes its eight observables: `out`, checked, or a new tensor next to `pos` when out is None."""
    import torch
    if out is None:
        return torch.empty(8, dtype=torch.float64, device=pos.device)
    if not (_is_cuda(out, torch.float64) and out.dim() == 1 and out.shape[0] == 8):
        raise ValueError("out must be a contiguous 8-element float64 CUDA tensor (a row of a larger one will do)")
    return out


# the potentials of pse_bonds_create, pse_angles_create and pse_dihedrals_create: name -> PSE_BOND_*, PSE_ANGLE_*, PSE_DIHEDRAL_*
BOND_KINDS = {"harmonic": 0, "fene": 1}
ANGLE_KINDS = {"harmonic": 0, "cosinesq": 1}
DIHEDRAL_KINDS = {"harmonic": 0, "opls": 1}


def _per_type(v):
    """A scalar or a sequence as a list (strings are scalars)."""
    import numpy as np
    if isinstance(v, str) or np.ndim(v) == 0:
        return [v]
    return list(v)


def _topology_arrays(index, types, cols, name, what):
    """The (count, cols) index array `name` of a list of `what`s ("bond" | "angle" | "dihedral") and its optional type array, checked, as
    contiguous uint32 arrays."""
    import numpy as np
    index = np.asarray(index)
    if index.ndim != 2 or index.shape[1] != cols or index.shape[0] == 0 or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"{name} must be a non-empty integer (n{what}s, {cols}) array of particle indices")
    if index.min() < 0 or index.max() >= 2 ** 32:
        raise ValueError(f"{name} holds an index outside [0, 2^32)")
    if types is not None:
        types = np.asarray(types)
        if types.shape != (index.shape[0],) or not np.issubdtype(types.dtype, np.integer) or types.min() < 0 or types.max() >= 2 ** 32:
            raise ValueError(f"types must be an integer array in [0, 2^32) with one entry per {what}")
        types = np.ascontiguousarray(types, dtype=np.uint32)
    return np.ascontiguousarray(index, dtype=np.uint32), types


def _type_params(kinds, k, x, xname, table, what, width=None):
    """The per-type parameters of a list of `what`s as (int32 kind codes, float64 k, float64 `xname`) arrays: scalars or sequences
    with one entry per type each, a kind being a name of `table` or its code.  width = w: a type has w parameters and not two: `k`
    holds them, one w-tuple or one per type, `x` is not used, and the result is (kind codes, (ntypes, w) float64 array, None)."""
    import numpy as np
    if width is not None:
        kinds, p = _per_type(kinds), np.array(k, dtype=np.float64)
        p = p[None] if p.ndim == 1 else p
        if p.ndim != 2 or p.shape[1] != width or len(kinds) != p.shape[0] or not kinds:
            raise ValueError(f"kinds and {xname} must have one entry and one {width}-tuple per {what} type")
        k, x = np.ascontiguousarray(p), None
    else:
        kinds, k, x = _per_type(kinds), _per_type(k), _per_type(x)
        if not (len(kinds) == len(k) == len(x)) or not kinds:
            raise ValueError(f"kinds, k and {xname} must have one entry per {what} type each")
    for v in kinds:
        if isinstance(v, str) and v not in table:
            raise ValueError(f"{what} kind must be one of {sorted(table)}, not {v!r}")
    return (np.array([table[v] if isinstance(v, str) else int(v) for v in kinds], dtype=np.int32), np.array(k, dtype=np.float64),
            None if x is None else np.array(x, dtype=np.float64))


class _DeviceObject:
    """What the owners of a device object share.  The object belongs to one handle, which frees it when it goes: the owner holds a
    reference to its engine (an Engine, or the StokesEngine of an integrator) and the engine's serial at creation, and a changed
    serial -- Engine.close(), or a setParams() of the integrator, which makes a new handle -- says that the object went with its
    handle.  A subclass names the library function that frees the object (DESTROY)."""

    def _create(self, engine, create, *args):
        """create(handle, *args, &object) on the handle of `engine`."""
        self.engine, self._lib, self._obj = engine, engine._lib, ctypes.c_void_p()
        _lib.check(getattr(self._lib, create)(engine._h, *args, ctypes.byref(self._obj)))
        self._serial = engine.serial

    def _handle(self, engine=None):
        """The device object, for a pass of `engine` (None: of its own engine)."""
        if self._obj is None or not self._obj.value:
            raise ValueError(f"this {type(self).__name__} is closed")
        if engine is not None and engine is not self.engine:
            raise ValueError(f"this {type(self).__name__} belongs to another engine")
        if self.engine.serial != self._serial:
            raise ValueError(f"this {type(self).__name__} went with the engine it was made on (setParams makes a new engine, close() ends "
                             "one): make it again")
        return self._obj

    def close(self):
        o, self._obj = getattr(self, "_obj", None), None
        if o is not None and o.value and self.engine.serial == self._serial:   # (otherwise the handle freed it already)
            getattr(self._lib, self.DESTROY)(o)

    __del__ = close


def _rows(engine, n):
    """How many rows of the caller-order arrays an object covers: `n`, or the engine's n_max."""
    n = int(engine.n_max if n is None else n)
    if not 0 <= n < 2 ** 32:
        raise ValueError("n outside [0, 2^32)")
    return n


def _vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class _TopologyList(_DeviceObject):
    """What BondList, AngleList and DihedralList share: the owner of a device topology among the rows of the caller-order arrays.
    A subclass names its entries (WHAT), its index array (INDEX, COLS columns), its second parameter (X) -- or, with WIDTH
    parameters per type, the one array of them -- its kind table and its three library functions."""

    WIDTH = None

    def __init__(self, engine, index, types, kinds, k, x, n):
        index, types = _topology_arrays(index, types, self.COLS, self.INDEX, self.WHAT)
        kind_a, k_a, x_a = _type_params(kinds, k, x, self.X, self.KINDS, self.WHAT, self.WIDTH)
        self.n, self.count = _rows(engine, n), index.shape[0]
        self.index = index   # (the host copy: analyze.Conformations finds the molecules of a forces.Bonds from it)
        par = (_vp(k_a),) if x_a is None else (_vp(k_a), _vp(x_a))
        self._create(engine, self.CREATE, self.n, self.count, _vp(index), _vp(types), len(kind_a), _vp(kind_a), *par)

    def forces(self, pos, force, accumulate=True, out=None, observables=True):
        """The forces of the list on the first n rows of `pos` (pse_bond_forces, pse_angle_forces, pse_dihedral_forces), added to `force` (or stored:
        accumulate=False, which zeroes the rows of particles in no entry), or force=None: observables only.  observables=True: returns
        the 8-element float64 CUDA tensor U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, count, written to `out` when one is given (e.g. a row of a
        log tensor); observables=False: forces only, the reduction is not run and None is returned.  Queue-only: nothing is read back."""
        obj = self._handle()
        _chk4(pos, "pos", self.n)
        if force is not None:
            _chk4(force, "force", self.n)
        out = _chk_out8(out, pos) if observables else None
        _lib.check(getattr(self._lib, self.FORCES)(obj, _ptr(pos), _ptr(force), 1 if accumulate else 0, _ptr(out)))
        return out


class BondList(_TopologyList):
    """Owner of a pse_bonds object: a fixed set of harmonic / FENE bonds."""

    WHAT, INDEX, COLS, X, KINDS = "bond", "pairs", 2, "r0", BOND_KINDS
    CREATE, FORCES, DESTROY = "pse_bonds_create", "pse_bond_forces", "pse_bonds_destroy"
    nbonds = property(lambda self: self.count)

    @property
    def overstretched(self):
        """FENE bonds found at r >= r0 by all calls since creation (pse_bonds_overstretched: waits for the stream)."""
        v = ctypes.c_ulonglong(0)
        _lib.check(self._lib.pse_bonds_overstretched(self._handle(), ctypes.byref(v)))
        return int(v.value)


class AngleList(_TopologyList):
    """Owner of a pse_angles object: a fixed set of harmonic / cosine-squared angles (end, vertex, end)."""

    WHAT, INDEX, COLS, X, KINDS = "angle", "triples", 3, "theta0", ANGLE_KINDS
    CREATE, FORCES, DESTROY = "pse_angles_create", "pse_angle_forces", "pse_angles_destroy"
    nangles = property(lambda self: self.count)


class DihedralList(_TopologyList):
    """Owner of a pse_dihedrals object: a fixed set of harmonic / OPLS dihedrals (i, j, k, l)."""

    WHAT, INDEX, COLS, X, KINDS, WIDTH = "dihedral", "quads", 4, "params", DIHEDRAL_KINDS, 4
    CREATE, FORCES, DESTROY = "pse_dihedrals_create", "pse_dihedral_forces", "pse_dihedrals_destroy"
    ndihedrals = property(lambda self: self.count)


class ExclusionList(_DeviceObject):
    """Owner of a pse_exclusions object: a set of particle pairs that the pair passes skip (HOOMD's nlist.reset_exclusions).  `pairs`
    is an (npairs, 2) integer array of caller-order particle indices below `n` (default: n_max); a pair listed twice or in either
    order is one exclusion.  Pass it as `exclusions=` to Engine.pair_table, pair_repulsion or pair_repulsion_virial."""

    DESTROY = "pse_exclusions_destroy"

    def __init__(self, engine, pairs, n=None):
        pairs, _ = _topology_arrays(pairs, None, 2, "pairs", "pair")
        self.n, self.count = _rows(engine, n), pairs.shape[0]
        self._create(engine, "pse_exclusions_create", self.n, self.count, _vp(pairs))


PAIR_TYPED_MAX_TYPES = 8   # pse_typed_table_create: particle types, and with them at most 36 pair types


def pair_type_index(a, b, ntypes):
    """The index of the pair of types (a, b), either order, among the ntypes (ntypes + 1)/2 pair types (include/pse_amd.h): the
    upper triangle row by row."""
    a, b = (a, b) if a <= b else (b, a)
    return a * ntypes - a * (a - 1) // 2 + (b - a)


def _ntypes_argument(ntypes):
    """The number of particle types of a typed object, checked."""
    if not 1 <= ntypes <= PAIR_TYPED_MAX_TYPES:
        raise ValueError(f"ntypes = {ntypes} outside [1, {PAIR_TYPED_MAX_TYPES}]")
    return ntypes


def _types_argument(types, ntypes=None):
    """The type array of a typed object, checked: None (one type) stays None, anything else must be a non-empty 1-D array of
    integers in [0, ntypes) -- ntypes=None: of non-negative integers -- and comes back as a contiguous uint32 array."""
    import numpy as np
    if types is None:
        return None
    types = np.asarray(types)
    if types.ndim != 1 or types.shape[0] == 0 or not np.issubdtype(types.dtype, np.integer) or types.min() < 0:
        raise ValueError("types must be a non-empty 1-D array of non-negative integers, one per particle")
    if ntypes is not None and types.max() >= ntypes:
        raise ValueError(f"types holds the type {int(types.max())} >= ntypes = {ntypes}")
    return np.ascontiguousarray(types, dtype=np.uint32)


class _TypedObject(_DeviceObject):
    """What the owners of an object with one type per particle share: `ntypes`, the number of pair types `npt`, and the rule for the
    rows `n` that the object covers -- `n` of the `types` (default: all of them), or without types `n` rows of the engine's arrays
    (default: n_max).  Every such object is made by create(handle, n, types, ntypes, *args, &object)."""

    def _create(self, engine, create, types, ntypes, n, *args):
        self.ntypes, self.npt = ntypes, ntypes * (ntypes + 1) // 2
        if types is None:
            self.n = _rows(engine, n)
        else:
            self.n = int(types.shape[0] if n is None else n)
            if not 0 <= self.n <= types.shape[0]:
                raise ValueError("n outside [0, len(types)]")
        super()._create(engine, create, self.n, _vp(types), ntypes, *args)


def _typed_tables(tables, ntypes):
    """The `tables` dictionary {(a, b): (table, rmin, rmax)} of a typed pair table as the arrays of pse_typed_table_create: (widths
    int32 (npt,), rmin float64 (npt,), rmax float64 (npt,), entries float64 (sum of widths, 2)).  A key may name its types in either
    order; both orders of one pair are a ValueError; a pair that is missing is off (width 0).  Needs no device."""
    import numpy as np
    if not isinstance(tables, dict) or not tables:
        raise ValueError("tables must be a non-empty dict {(a, b): (table, rmin, rmax)}")
    _ntypes_argument(ntypes)
    npt = ntypes * (ntypes + 1) // 2
    width, rmin, rmax, parts = np.zeros(npt, dtype=np.int32), np.zeros(npt), np.zeros(npt), [None] * npt
    for key, value in tables.items():
        if not (isinstance(key, tuple) and len(key) == 2 and all(isinstance(t, (int, np.integer)) for t in key)):
            raise ValueError(f"tables key {key!r} is not a pair (a, b) of integer types")
        a, b = int(key[0]), int(key[1])
        if not (0 <= a < ntypes and 0 <= b < ntypes):
            raise ValueError(f"tables key {key!r} names a type outside [0, {ntypes})")
        p = pair_type_index(a, b, ntypes)
        if parts[p] is not None:
            raise ValueError(f"tables holds both ({a}, {b}) and ({b}, {a}): one pair of types, one table")
        if not (isinstance(value, (tuple, list)) and len(value) == 3):
            raise ValueError(f"tables[{key!r}] must be (table, rmin, rmax)")
        t = value[0].detach().cpu().numpy() if hasattr(value[0], "detach") else value[0]
        t = np.array(t, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != 2 or not 2 <= t.shape[0] <= 2048:
            raise ValueError(f"tables[{key!r}]: the table must be (width, 2) with 2 <= width <= 2048: V and F at the nodes")
        if not np.isfinite(t).all():
            raise ValueError(f"tables[{key!r}]: table entries must be finite")
        lo, hi = float(value[1]), float(value[2])
        if not 0.0 <= lo < hi < float("inf"):
            raise ValueError(f"tables[{key!r}]: need 0 <= rmin < rmax, both finite")
        width[p], rmin[p], rmax[p], parts[p] = t.shape[0], lo, hi, t
    return width, rmin, rmax, np.ascontiguousarray(np.concatenate([t for t in parts if t is not None], axis=0))


def _typed_types(types, tables):
    """(uint32 types, ntypes): the type array of a typed pair table, checked; ntypes is one more than the largest type in `types`
    or in a key of `tables`."""
    import numpy as np
    types = _types_argument(np.asarray(types))   # (None is no type array here: it fails the check as the 0-D array it becomes)
    keys = [int(t) for key in tables for t in key] if isinstance(tables, dict) and all(isinstance(k, tuple) for k in tables) else []
    return types, max([int(types.max())] + keys) + 1


class TypedTable(_TypedObject):
    """Owner of a pse_typed_table object: one type per particle and one tabulated potential per pair of types (HOOMD's pair.table with
    a pair_coeff per type pair).  `types`: (n,) integers, the type of caller-order particle t; a particle past them acts as type 0.
    `tables`: {(a, b): (table, rmin, rmax)} with `table` a (width, 2) array of V and F at the nodes as for Engine.pair_table; either
    order of a key, a missing pair is off.  Pass it as `typed` to Engine.pair_table_typed."""

    DESTROY = "pse_typed_table_destroy"

    def __init__(self, engine, types, tables, n=None):
        types, ntypes = _typed_types(types, tables)
        self._create_from(engine, types, ntypes, *_typed_tables(tables, ntypes), n)

    @classmethod
    def from_arrays(cls, engine, types, ntypes, width, rmin, rmax, entries):
        """The object of arrays that are checked already: what _typed_types and _typed_tables return (forces.TypedTablePair, which
        numbers its types by name and may know more types than the particles show)."""
        self = cls.__new__(cls)
        self._create_from(engine, types, ntypes, width, rmin, rmax, entries, None)
        return self

    def _create_from(self, engine, types, ntypes, width, rmin, rmax, entries, n):
        self.count = int(width.sum())
        self._create(engine, "pse_typed_table_create", types, ntypes, n, _vp(width), _vp(rmin), _vp(rmax), _vp(entries))


PAIR_HIST_MAX_COUNTERS = 8192   # pse_pair_hist_create: pair types x bins


def _pair_hist_arguments(types, ntypes, nbins, rmin, rmax):
    """The arguments of a pair histogram, checked before the device is touched: (types uint32 (n,) or None, ntypes, nbins, rmin,
    rmax).  `types`: None (one type) or a 1-D array of integers in [0, ntypes)."""
    import numpy as np
    ntypes, nbins, rmin, rmax = int(ntypes), int(nbins), float(rmin), float(rmax)
    _ntypes_argument(ntypes)
    if nbins < 1:
        raise ValueError(f"nbins = {nbins}: need at least one bin")
    npt = ntypes * (ntypes + 1) // 2
    if npt * nbins > PAIR_HIST_MAX_COUNTERS:
        raise ValueError(f"{npt} pair types x {nbins} bins = {npt * nbins} counters, more than {PAIR_HIST_MAX_COUNTERS}")
    if not 0.0 <= rmin < rmax < float("inf"):
        raise ValueError("need 0 <= rmin < rmax, both finite")
    return _types_argument(types, ntypes), ntypes, nbins, rmin, rmax


class PairHistogram(_TypedObject):
    """Owner of a pse_pair_hist object: one type per particle and nbins uniform bins on [rmin, rmax) for every pair of types.
    `types`: (n,) integers below ntypes, the type of caller-order particle t, or None: one type; a particle past them acts as type 0.
    Pass it as `hist` to Engine.pair_hist_accumulate."""

    DESTROY = "pse_pair_hist_destroy"

    def __init__(self, engine, types, ntypes, nbins, rmin, rmax, n=None):
        types, ntypes, self.nbins, self.rmin, self.rmax = _pair_hist_arguments(types, ntypes, nbins, rmin, rmax)
        self._create(engine, "pse_pair_hist_create", types, ntypes, n, self.nbins, self.rmin, self.rmax)


SF_MAX_INDEX = 4096    # pse_structure_factor_create: |mx|, |my|, |mz|
SF_MAX_MODES = 32768   # ... and the number of modes


def _structure_factor_arguments(types, ntypes, modes):
    """The arguments of a structure-factor object, checked before the device is touched: (types uint32 (n,) or None, ntypes, modes
    int32 (nk, 3)).  `types`: None (one type) or a 1-D array of integers in [0, ntypes); `modes`: integer triples within
    +-SF_MAX_INDEX, at most SF_MAX_MODES of them."""
    import numpy as np
    ntypes = int(ntypes)
    _ntypes_argument(ntypes)
    modes = np.asarray(modes)
    if modes.ndim != 2 or modes.shape[1] != 3 or modes.shape[0] == 0 or not np.issubdtype(modes.dtype, np.integer):
        raise ValueError("modes must be a non-empty integer (nk, 3) array of reciprocal-lattice indices (mx, my, mz)")
    if modes.shape[0] > SF_MAX_MODES:
        raise ValueError(f"{modes.shape[0]} modes, more than {SF_MAX_MODES}")
    if np.abs(modes).max() > SF_MAX_INDEX:
        raise ValueError(f"modes holds the index {int(np.abs(modes).max())} beyond +-{SF_MAX_INDEX}")
    return _types_argument(types, ntypes), ntypes, np.ascontiguousarray(modes, dtype=np.int32)


class StructureFactorModes(_TypedObject):
    """Owner of a pse_structure_factor object: one type per particle and a list of integer modes (mx, my, mz) of the box's reciprocal
    lattice.  `types`: (n,) integers below ntypes, the type of caller-order particle t, or None: one type; a particle past them acts
    as type 0.  Pass it as `sf` to Engine.structure_factor_accumulate."""

    DESTROY = "pse_structure_factor_destroy"

    def __init__(self, engine, types, ntypes, modes, n=None):
        types, ntypes, self.modes = _structure_factor_arguments(types, ntypes, modes)
        self.nk = int(self.modes.shape[0])
        self._create(engine, "pse_structure_factor_create", types, ntypes, n, self.nk, _vp(self.modes))


MSD_MAX_ORIGINS = 64   # pse_msd_create: slots of one object, and pairs (slot, row) of one pse_msd_accumulate
MSD_MOMENTS = 10       # dx dy dz, dx^2 dy^2 dz^2 dxdy dxdz dydz, |d|^4


def _msd_arguments(types, ntypes, norigins):
    """The arguments of a displacement object, checked before the device is touched: (types uint32 (n,) or None, ntypes, norigins)."""
    norigins = int(norigins)
    if not 1 <= norigins <= MSD_MAX_ORIGINS:
        raise ValueError(f"norigins = {norigins} outside [1, {MSD_MAX_ORIGINS}]")
    ntypes = _ntypes_argument(int(ntypes))
    return _types_argument(types, ntypes), ntypes, norigins


def _msd_pairs(slots, rows, norigins, nrows):
    """The (slot, row) lists of one pse_msd_accumulate as two int32 arrays, checked before the device is touched."""
    import numpy as np
    slots, rows = np.asarray(slots), np.asarray(rows)
    if slots.ndim != 1 or rows.shape != slots.shape:
        raise ValueError("slots and rows must be 1-D integer sequences of one length")
    if not 1 <= slots.shape[0] <= MSD_MAX_ORIGINS:
        raise ValueError(f"{slots.shape[0]} pairs outside [1, {MSD_MAX_ORIGINS}]")
    if not np.issubdtype(slots.dtype, np.integer) or not np.issubdtype(rows.dtype, np.integer):
        raise ValueError("slots and rows must be 1-D integer sequences of one length")
    if slots.min() < 0 or slots.max() >= norigins:
        raise ValueError(f"slots holds a slot outside [0, {norigins})")
    if rows.min() < 0 or rows.max() >= nrows:
        raise ValueError(f"rows holds a row outside [0, {nrows})")
    if len(set(rows.tolist())) != rows.shape[0]:
        raise ValueError("rows names a row twice")
    return np.ascontiguousarray(slots, dtype=np.int32), np.ascontiguousarray(rows, dtype=np.int32)


def _finite(x, name):
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"{name} = {x} is not finite")
    return x


class DisplacementOrigins(_TypedObject):
    """Owner of a pse_msd object: one type per particle and `norigins` slots of unwrapped positions on the device.  `types`: (n,)
    integers below ntypes, the type of caller-order particle t, or None: one type; a particle past them acts as type 0.  Pass it as
    `origins` to Engine.msd_store, msd_accumulate and msd_displacement."""

    DESTROY = "pse_msd_destroy"

    def __init__(self, engine, types, ntypes, norigins, n=None):
        types, ntypes, self.norigins = _msd_arguments(types, ntypes, norigins)
        self._create(engine, "pse_msd_create", types, ntypes, n, self.norigins)


ISF_MAX_ORIGINS = 64   # pse_isf_create: slots of one object, and pairs (slot, row) of one pse_isf_correlate
ISF_MAX_MODES = 4096   # ... and the number of modes


def _isf_arguments(types, ntypes, modes, norigins):
    """The arguments of a scattering object, checked before the device is touched: (types uint32 (n,) or None, ntypes, modes int32
    (nk, 3), norigins): those of a structure-factor object with at most ISF_MAX_MODES modes, and 1 <= norigins <= ISF_MAX_ORIGINS."""
    types, ntypes, modes = _structure_factor_arguments(types, ntypes, modes)
    if modes.shape[0] > ISF_MAX_MODES:
        raise ValueError(f"{modes.shape[0]} modes, more than {ISF_MAX_MODES}")
    norigins = int(norigins)
    if not 1 <= norigins <= ISF_MAX_ORIGINS:
        raise ValueError(f"norigins = {norigins} outside [1, {ISF_MAX_ORIGINS}]")
    return types, ntypes, modes, norigins


class ScatteringOrigins(_TypedObject):
    """Owner of a pse_isf object: one type per particle, a list of integer modes (mx, my, mz) of the box's reciprocal lattice, a
    current buffer and `norigins` origin slots of fractional coordinates and densities on the device.  `types`, `modes`: as for
    StructureFactorModes, at most 4096 modes.  Pass it as `isf` to Engine.isf_sample, isf_store and isf_correlate.  sample_n: N of the
    sample in the current buffer (0: none yet); slot_n[s]: N of the sample stored in slot s (0: never stored)."""

    DESTROY = "pse_isf_destroy"

    def __init__(self, engine, types, ntypes, modes, norigins, n=None):
        types, ntypes, self.modes, self.norigins = _isf_arguments(types, ntypes, modes, norigins)
        self.nk = int(self.modes.shape[0])
        self._create(engine, "pse_isf_create", types, ntypes, n, self.nk, _vp(self.modes), self.norigins)
        self.sample_n, self.slot_n = 0, [0] * self.norigins


MOL_TILE = 1024       # PSE_MOL_TILE: members of the largest molecule
MOL_COLS = 14         # PSE_MOL_COLS: columns of a molecule's row and of a type's sums
MOL_MAX_BINS = 4096   # pse_molecules_create: bins of each histogram


def _molecule_arguments(pairs, mol_types, ntypes, nbins, rg_max, ree_max):
    """The arguments of a MoleculeTopology, checked before the device is touched: (pairs uint32 (nbonds, 2), molecule types uint32
    (nmol,) or None, ntypes, nbins, rg_max, ree_max).  Whether there is one type per molecule is the library's to say: it finds the
    molecules."""
    import numpy as np
    pairs, _ = _topology_arrays(pairs, None, 2, "bonds", "bond")
    ntypes = _ntypes_argument(int(ntypes))
    if mol_types is not None:
        mol_types = np.asarray(mol_types)
        if mol_types.ndim != 1 or mol_types.shape[0] == 0 or not np.issubdtype(mol_types.dtype, np.integer) or mol_types.min() < 0:
            raise ValueError("molecule_types must be a non-empty 1-D array of non-negative integers, one per molecule")
        if mol_types.max() >= ntypes:
            raise ValueError(f"molecule_types holds the type {int(mol_types.max())} >= ntypes = {ntypes}")
        mol_types = np.ascontiguousarray(mol_types, dtype=np.uint32)
    nbins = int(nbins)
    if not 0 <= nbins <= MOL_MAX_BINS:
        raise ValueError(f"nbins = {nbins} outside [0, {MOL_MAX_BINS}]")
    if nbins > 0:
        if rg_max is None or ree_max is None:
            raise ValueError("nbins > 0 needs rg_max and ree_max")
        rg_max, ree_max = _finite(rg_max, "rg_max"), _finite(ree_max, "ree_max")
        if not (rg_max > 0.0 and ree_max > 0.0):
            raise ValueError("rg_max and ree_max must be positive")
    else:
        rg_max = ree_max = 0.0
    return pairs, mol_types, ntypes, nbins, rg_max, ree_max


class MoleculeTopology(_DeviceObject):
    """Owner of a pse_molecules object: the molecules of a bond topology -- the connected components of `pairs`, an (nbonds, 2) array
    of caller-order particle indices below `n` (default: n_max) -- with one type per molecule (`mol_types`: (nmol,) integers below
    ntypes in the order of the molecule numbers, or None: one type) and `nbins` bins for the histograms of Rg on [0, rg_max) and of
    |R| on [0, ree_max) (0: none).  Pass it as `molecules` to Engine.molecules_compute.  nmol, nlinear and nmol_type (per type) are
    read once at creation (host words: no device wait)."""

    DESTROY = "pse_molecules_destroy"

    def __init__(self, engine, pairs, mol_types=None, ntypes=1, nbins=0, rg_max=None, ree_max=None, n=None):
        import numpy as np
        pairs, mol_types, self.ntypes, self.nbins, self.rg_max, self.ree_max = _molecule_arguments(pairs, mol_types, ntypes, nbins, rg_max,
                                                                                                 ree_max)
        self.n = _rows(engine, n)
        if mol_types is not None:   # (the library reads nmol entries: the count has to be right before it does)
            from .analyze import molecules_of
            nmol = molecules_of(self.n, pairs)[1]
            if mol_types.shape[0] != nmol:
                raise ValueError(f"molecule_types has {mol_types.shape[0]} entries, the bonds make {nmol} molecules")
        self._create(engine, "pse_molecules_create", self.n, pairs.shape[0], _vp(pairs), _vp(mol_types), self.ntypes, self.nbins,
                     self.rg_max, self.ree_max)
        nmol, nlinear, nmol_type = ctypes.c_uint(0), np.zeros(self.ntypes, dtype=np.uint32), np.zeros(self.ntypes, dtype=np.uint32)
        _lib.check(self._lib.pse_molecules_count(self._obj, ctypes.byref(nmol), _vp(nlinear), _vp(nmol_type)))
        self.nmol, self.nlinear, self.nmol_type = int(nmol.value), nlinear.astype(np.int64), nmol_type.astype(np.int64)


MOLPAIR_COLS = 2      # PSE_MOLPAIR_COLS: per separation D, C
MOLPAIR_SUMS = 2      # PSE_MOLPAIR_SUMS: per type the sum of 1/Rh and of (1/Rh)^2


class MoleculePairs(_DeviceObject):
    """Owner of a pse_molecule_pairs object: the molecules of a bond topology as for a MoleculeTopology (`pairs`, `mol_types`, `ntypes`,
    `n`), the chain rank of every member and `ns`, the number of separations of the curves (1 .. 1024).  Pass it as `pairs` to
    Engine.molecule_pairs_compute.  nmol, nmol_type (per type) and terms (ntypes, ns, 2) -- the number of summands behind every entry
    of the curves -- are read once at creation (host words: no device wait)."""

    DESTROY = "pse_molecule_pairs_destroy"

    def __init__(self, engine, pairs, mol_types=None, ntypes=1, ns=1, n=None):
        import numpy as np
        pairs, mol_types, self.ntypes, _, _, _ = _molecule_arguments(pairs, mol_types, ntypes, 0, None, None)
        self.ns = int(ns)
        if not 1 <= self.ns <= MOL_TILE:
            raise ValueError(f"ns = {self.ns} outside [1, {MOL_TILE}]")
        self.n = _rows(engine, n)
        if mol_types is not None:   # (the library reads nmol entries: the count has to be right before it does)
            from .analyze import molecules_of
            nmol = molecules_of(self.n, pairs)[1]
            if mol_types.shape[0] != nmol:
                raise ValueError(f"molecule_types has {mol_types.shape[0]} entries, the bonds make {nmol} molecules")
        self._create(engine, "pse_molecule_pairs_create", self.n, pairs.shape[0], _vp(pairs), _vp(mol_types), self.ntypes, self.ns)
        nmol, nmol_type = ctypes.c_uint(0), np.zeros(self.ntypes, dtype=np.uint32)
        terms = np.zeros((self.ntypes, self.ns, MOLPAIR_COLS), dtype=np.uint64)
        _lib.check(self._lib.pse_molecule_pairs_counts(self._obj, ctypes.byref(nmol), _vp(nmol_type), _vp(terms)))
        self.nmol, self.nmol_type, self.terms = int(nmol.value), nmol_type.astype(np.int64), terms.astype(np.int64)


CHAIN_MODES_MAX = 32      # PSE_CHAIN_MODES_MAX: functionals of one ChainModes
CHAIN_MODES_STATIC = 6    # PSE_CHAIN_MODES_STATIC: xx, yy, zz, xy, xz, yz
CHAIN_MODES_CORR = 9      # PSE_CHAIN_MODES_CORR: 3 alpha + beta, alpha of now, beta of the origin


def host_cluster_word(parent, c):
    """The 64-bit word of the union-find with image offsets (pse_host_cluster_word; host only): the parent row, below 2^28, and the
    offset c (three integers in [-2047, 2047]) packed as the device packs them."""
    import numpy as np
    parent, c = int(parent), [int(v) for v in c]
    if not 0 <= parent < 2 ** 32 or len(c) != 3 or any(not -2 ** 31 <= v < 2 ** 31 for v in c):
        raise ValueError("parent no C unsigned, or c not three C ints")
    word = ctypes.c_ulonglong(0)
    _lib.check(_lib.load().pse_host_cluster_word(parent, _vp(np.array(c, dtype=np.int32)), ctypes.byref(word)))
    return int(word.value)


def host_cluster_word_parts(word):
    """(parent, (c1, c2, c3)) of a word of host_cluster_word (pse_host_cluster_word_parts; host only)."""
    import numpy as np
    word = int(word)
    if not 0 <= word < 2 ** 64:
        raise ValueError("word no unsigned 64-bit integer")
    parent, c = ctypes.c_uint(0), np.zeros(3, dtype=np.int32)
    _lib.check(_lib.load().pse_host_cluster_word_parts(word, ctypes.byref(parent), _vp(c)))
    return int(parent.value), tuple(int(v) for v in c)


def host_rouse_weights(m, nmodes):
    """The (nmodes, m) weights of pse_host_rouse_weights for a chain of m members (host only): row 0 the end-to-end functional
    (-1, 0, ..., 0, +1), rows p >= 1 the Rouse modes cos(pi p (2 q + 1) / (2 m)) / m with the argument reduced in integers."""
    import numpy as np
    m, nmodes = int(m), int(nmodes)
    if not 0 <= m <= 2 ** 24 or not -2 ** 31 <= nmodes < 2 ** 31:
        raise ValueError("m outside [0, 2^24] or nmodes no C int")
    out = np.zeros((min(max(nmodes, 1), CHAIN_MODES_MAX), max(m, 1)))   # (the library refuses what would not fit before it writes)
    _lib.check(_lib.load().pse_host_rouse_weights(m, nmodes, _vp(out)))
    return out


def _chain_modes_arguments(sizes, weights, norigins):
    """The tables of a ChainModes, checked before the device is touched: (sizes uint32 (nsizes,), weights float64 flat, K, norigins).
    `sizes`: the distinct sizes of the linear molecules, ascending; `weights`: one (K, m) array per size, finite."""
    import numpy as np
    sizes = np.asarray(sizes)
    if sizes.ndim != 1 or sizes.shape[0] == 0 or not np.issubdtype(sizes.dtype, np.integer) or sizes.min() < 2 or np.any(np.diff(sizes) <= 0):
        raise ValueError("sizes must be a non-empty ascending 1-D sequence of distinct molecule sizes >= 2")
    tables = [np.asarray(w, dtype=np.float64) for w in weights]
    if len(tables) != sizes.shape[0]:
        raise ValueError(f"weights has {len(tables)} tables, sizes {sizes.shape[0]} entries")
    K = tables[0].shape[0] if tables[0].ndim == 2 else 0
    if not 1 <= K <= CHAIN_MODES_MAX:
        raise ValueError(f"a weight table must be (K, m) with K in [1, {CHAIN_MODES_MAX}]")
    for m, w in zip(sizes.tolist(), tables):
        if w.shape != (K, m):
            raise ValueError(f"the weight table of size {m} has the shape {w.shape}, not {(K, m)}")
        if not np.isfinite(w).all():
            raise ValueError(f"the weight table of size {m} holds a value that is not finite")
    norigins = int(norigins)
    if not 0 <= norigins <= MSD_MAX_ORIGINS:
        raise ValueError(f"norigins = {norigins} outside [0, {MSD_MAX_ORIGINS}]")
    flat = np.ascontiguousarray(np.concatenate([w.ravel() for w in tables]))
    return np.ascontiguousarray(sizes, dtype=np.uint32), flat, K, norigins


class ChainModes(_DeviceObject):
    """Owner of a pse_chain_modes object: the molecules of a bond topology as for a MoleculeTopology (`pairs`, `mol_types`, `ntypes`,
    `n`), K weight rows per distinct size of the LINEAR molecules (`sizes` ascending, `weights` one (K, m) array per size) and
    `norigins` <= 64 origin slots (0: static only).  Pass it as `modes` to Engine.chain_modes_compute, chain_modes_store and
    chain_modes_correlate.  nmol, nlin, nlin_type (per type), lin_mol and lin_size (per linear molecule, in the order of the device
    arrays) are read once at creation (host words: no device wait)."""

    DESTROY = "pse_chain_modes_destroy"

    def __init__(self, engine, pairs, sizes, weights, mol_types=None, ntypes=1, norigins=0, n=None):
        import numpy as np
        pairs, mol_types, self.ntypes, _, _, _ = _molecule_arguments(pairs, mol_types, ntypes, 0, None, None)
        sizes, flat, self.K, self.norigins = _chain_modes_arguments(sizes, weights, norigins)
        self.n = _rows(engine, n)
        if mol_types is not None:   # (the library reads nmol entries: the count has to be right before it does)
            from .analyze import molecules_of
            nmol = molecules_of(self.n, pairs)[1]
            if mol_types.shape[0] != nmol:
                raise ValueError(f"molecule_types has {mol_types.shape[0]} entries, the bonds make {nmol} molecules")
        self._create(engine, "pse_chain_modes_create", self.n, pairs.shape[0], _vp(pairs), _vp(mol_types), self.ntypes, self.K,
                     int(sizes.shape[0]), _vp(sizes), _vp(flat), self.norigins)
        c_nmol, c_nlin, nlin_type = ctypes.c_uint(0), ctypes.c_uint(0), np.zeros(self.ntypes, dtype=np.uint32)
        _lib.check(self._lib.pse_chain_modes_counts(self._obj, ctypes.byref(c_nmol), ctypes.byref(c_nlin), _vp(nlin_type), None, None))
        self.nmol, self.nlin, self.nlin_type = int(c_nmol.value), int(c_nlin.value), nlin_type.astype(np.int64)
        lin_mol, lin_size = np.zeros(self.nlin, dtype=np.uint32), np.zeros(self.nlin, dtype=np.uint32)
        _lib.check(self._lib.pse_chain_modes_counts(self._obj, None, None, None, _vp(lin_mol), _vp(lin_size)))
        self.lin_mol, self.lin_size = lin_mol.astype(np.int64), lin_size.astype(np.int64)
        self.computed = False     # chain_modes_compute has been queued
        self.stored = set()       # the slots that hold a buffer


def _cluster_arguments(types, ntypes, rlink, name="rlink"):
    """The arguments of a ClusterLinks, checked before the device is touched: (types uint32 (n,) or None, ntypes, rlink float64 (npt,)).
    `rlink`: a scalar (every pair type), a dict {(a, b): r} in either key order with a missing pair off, or npt entries in the
    order of pair_type_index; 0 switches a pair type off, at least one must be on.  `name`: what the messages call the distances."""
    import numpy as np
    ntypes = int(ntypes)
    _ntypes_argument(ntypes)
    npt = ntypes * (ntypes + 1) // 2
    if isinstance(rlink, dict):
        out = np.zeros(npt)
        seen = set()
        for key, r in rlink.items():
            if not (isinstance(key, tuple) and len(key) == 2 and all(isinstance(v, (int, np.integer)) and 0 <= v < ntypes for v in key)):
                raise ValueError(f"{name} key {key!r}: need a pair (a, b) of types in [0, {ntypes})")
            p = pair_type_index(int(key[0]), int(key[1]), ntypes)
            if p in seen:
                raise ValueError(f"{name} names the pair of types {tuple(sorted(key))} twice")
            seen.add(p)
            out[p] = float(r)
    elif np.ndim(rlink) == 0:
        out = np.full(npt, float(rlink))
    else:
        out = np.array(rlink, dtype=np.float64)
        if out.shape != (npt,):
            raise ValueError(f"{name} must be a scalar, a dict or {npt} entries, one per pair of types")
    if not np.isfinite(out).all() or (out < 0.0).any():
        raise ValueError(f"{name} must be finite and not negative (0 switches a pair type off)")
    if not (out > 0.0).any():
        raise ValueError(f"every pair type is off: {name} needs a positive entry")
    return _types_argument(types, ntypes), ntypes, np.ascontiguousarray(out)


class ClusterLinks(_TypedObject):
    """Owner of a pse_clusters object: one type per particle and one link distance per pair of types (see _cluster_arguments for
    `rlink`).  `types`: (n,) integers below ntypes, the type of caller-order particle t, or None: one type; a particle past them acts
    as type 0.  Pass it as `links` to Engine.cluster_label."""

    DESTROY = "pse_clusters_destroy"

    def __init__(self, engine, types, ntypes, rlink, n=None):
        types, ntypes, self.rlink = _cluster_arguments(types, ntypes, rlink)
        self._create(engine, "pse_clusters_create", types, ntypes, n, _vp(self.rlink))

    def status(self):
        """The object's sticky give-up word (pse_clusters_status: waits for the stream).  0: every labelling so far was complete."""
        word = ctypes.c_uint(0)
        _lib.check(self._lib.pse_clusters_status(self._handle(), ctypes.byref(word)))
        return int(word.value)


BOND_ORDER_MAX_DEGREES = 4               # pse_bond_order_create: degrees of one object
BOND_ORDER_DEGREES = (2, 4, 6, 8, 10, 12)  # ... and what they may be
BOND_ORDER_MAX_COUNTERS = 8192           # pse_bond_order_histogram: types x bins


def _bond_order_arguments(types, ntypes, rnb, degrees):
    """The arguments of a BondOrderShells, checked before the device is touched: (types uint32 (n,) or None, ntypes, rnb float64
    (npt,), degrees int32 (nl,)).  `rnb`: the three forms of _cluster_arguments' rlink; `degrees`: 1 to 4 distinct even integers from
    2 to 12."""
    import numpy as np
    types, ntypes, rnb = _cluster_arguments(types, ntypes, rnb, "rnb")
    deg = np.asarray(degrees)
    if deg.ndim != 1 or not 1 <= deg.shape[0] <= BOND_ORDER_MAX_DEGREES or not np.issubdtype(deg.dtype, np.integer):
        raise ValueError(f"degrees must be 1 to {BOND_ORDER_MAX_DEGREES} integers")
    for l in deg.tolist():
        if l not in BOND_ORDER_DEGREES:
            raise ValueError(f"degree {l} is not one of the even degrees {BOND_ORDER_DEGREES}")
    if len(set(deg.tolist())) != deg.shape[0]:
        raise ValueError("degrees names a degree twice")
    return types, ntypes, rnb, np.ascontiguousarray(deg, dtype=np.int32)


class BondOrderShells(_TypedObject):
    """Owner of a pse_bond_order object: one type per particle, one neighbour distance per pair of types and the degrees l of the
    Steinhardt parameters (see _bond_order_arguments).  `types`: (n,) integers below ntypes, the type of caller-order particle t, or
    None: one type; a particle past them acts as type 0.  Pass it as `shells` to Engine.bond_order and Engine.bond_order_histogram."""

    DESTROY = "pse_bond_order_destroy"

    def __init__(self, engine, types, ntypes, rnb, degrees=(4, 6), n=None):
        types, ntypes, self.rnb, self.degrees = _bond_order_arguments(types, ntypes, rnb, degrees)
        self.nl = int(self.degrees.shape[0])
        self._create(engine, "pse_bond_order_create", types, ntypes, n, _vp(self.rnb), self.nl, _vp(self.degrees))

    def column(self, l):
        """The column of degree `l` in q and qbar."""
        cols = self.degrees.tolist()
        if int(l) not in cols:
            raise ValueError(f"degree {l} is not among the degrees {tuple(cols)} of this object")
        return cols.index(int(l))


class _ForcePasses:
    """The force providers of the C-ABI on one handle, for whoever holds one: an Engine, which owns its handle, and the
    StokesEngine of an integrator, whose handle the C++ Stokes object owns.  Needs `_lib`, `_h` (the handle; raises where there is
    none), `n_max`, and `serial`: a number that changes when the handle goes, by which the objects made here know (_DeviceObject)."""

    def pair_repulsion(self, pos, force, k, sigma=2.0, group=None, accumulate=True, exclusions=None):
        """Soft repulsion k (sigma - r) r_hat for r < sigma added to (or stored in) `force`.  exclusions: an
        ExclusionList (Engine.exclusions) whose pairs contribute nothing (pse_pair_repulsion_excl); None: every pair in range acts."""
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk4(force, "force"); _chk_group(group)
        if exclusions is not None:
            _lib.check(self._lib.pse_pair_repulsion_excl(self._h, _ptr(pos), _ptr(force), _ptr(group), n, float(k), float(sigma),
                                                         1 if accumulate else 0, None, exclusions._handle(self)))
            return force
        _lib.check(self._lib.pse_pair_repulsion(self._h, _ptr(pos), _ptr(force), _ptr(group), n, float(k), float(sigma),
                                                1 if accumulate else 0))
        return force

    def pair_repulsion_virial(self, pos, force, k, sigma=2.0, group=None, accumulate=True, out=None, exclusions=None):
        """pair_repulsion plus the pair observables of the same pass (pse_pair_repulsion_virial): returns the 8-element float64 CUDA
        tensor U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs (W_ab = sum_{i<j} d_a F_b, stress = -W / V; see include/pse_amd.h).  `force`
        may be None (observables only).  `out`: where to write them -- e.g. a row of a (samples, 8) log tensor; nothing is read
        back, the tensor is filled when the stream gets there.  exclusions: as for pair_repulsion; the excluded pairs are in none of
        the eight numbers."""
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        if force is not None:
            _chk4(force, "force")
        out = _chk_out8(out, pos)
        if exclusions is not None:
            _lib.check(self._lib.pse_pair_repulsion_excl(self._h, _ptr(pos), _ptr(force), _ptr(group), n, float(k), float(sigma),
                                                         1 if accumulate else 0, _ptr(out), exclusions._handle(self)))
            return out
        _lib.check(self._lib.pse_pair_repulsion_virial(self._h, _ptr(pos), _ptr(force), _ptr(group), n, float(k), float(sigma),
                                                       1 if accumulate else 0, _ptr(out)))
        return out

    def pair_table(self, pos, force, table, rmin, rmax, group=None, accumulate=True, out=None, observables=True, exclusions=None):
        """A tabulated central pair potential on the engine's cell list (pse_pair_table; see include/pse_amd.h).  `table`: contiguous
        (width, 2) float64 CUDA tensor, V and F (magnitude of the radial force, positive for a repulsion) at the nodes
        rmin + k (rmax - rmin)/(width - 1), linear in between; pairs with rmin <= r < rmax act.  `force` is incremented (or stored,
        accumulate=False), or None: observables only.  observables=True: returns the 8-element float64 CUDA tensor U, Wxx, Wxy, Wxz,
        Wyy, Wyz, Wzz, npairs, written to `out` when one is given (e.g. a row of a log tensor).  observables=False: forces only, the
        reduction is not run, `out` is left alone and None is returned.  Nothing is read back; the stream reads `table`, so keep it
        alive and unchanged until the stream has passed the call.  exclusions: an ExclusionList (Engine.exclusions) whose pairs
        contribute nothing to the forces or the eight numbers (pse_pair_table_excl); None: every pair in range acts."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        if force is not None:
            _chk4(force, "force")
        if not (_is_cuda(table, torch.float64) and table.dim() == 2 and table.shape[1] == 2):
            raise ValueError("table must be a contiguous (width, 2) float64 CUDA tensor: V and F at the nodes")
        out = _chk_out8(out, pos) if observables else None
        if exclusions is not None:
            _lib.check(self._lib.pse_pair_table_excl(self._h, _ptr(pos), _ptr(force), _ptr(group), n, _ptr(table), int(table.shape[0]),
                                                     float(rmin), float(rmax), 1 if accumulate else 0, _ptr(out), exclusions._handle(self)))
            return out
        _lib.check(self._lib.pse_pair_table(self._h, _ptr(pos), _ptr(force), _ptr(group), n, _ptr(table), int(table.shape[0]),
                                            float(rmin), float(rmax), 1 if accumulate else 0, _ptr(out)))
        return out

    def typed_table(self, types, tables, n=None):
        """A typed pair table on the device (pse_typed_table_create; see include/pse_amd.h): `types` (n,) the type of every
        caller-order particle, `tables` {(a, b): (table, rmin, rmax)} one tabulated potential per pair of types, either order of a
        key, a missing pair off; `n`: how many of `types` to use (default: all).  Returns a TypedTable: the `typed` of
        pair_table_typed."""
        return TypedTable(self, types, tables, n)

    def pair_table_typed(self, pos, force, typed, group=None, accumulate=True, out=None, observables=True, exclusions=None):
        """Engine.pair_table with, for every pair, the table and the range of its pair of types (pse_pair_table_typed).  `typed`: a
        TypedTable (Engine.typed_table).  `force`, `group`, `accumulate`, `out`, `observables` and what is returned as for
        pair_table; exclusions: an ExclusionList whose pairs contribute nothing, None: every pair in range acts."""
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        if force is not None:
            _chk4(force, "force")
        out = _chk_out8(out, pos) if observables else None
        _lib.check(self._lib.pse_pair_table_typed(typed._handle(self), _ptr(pos), _ptr(force), _ptr(group), n, 1 if accumulate else 0,
                                                  _ptr(out), None if exclusions is None else exclusions._handle(self)))
        return out

    def pair_histogram(self, types, ntypes, nbins, rmin, rmax, n=None):
        """A pair-distance histogram on the device (pse_pair_hist_create; see include/pse_amd.h): `types` (n,) the type of every
        caller-order particle, below `ntypes` <= 8, or None: one type; `nbins` uniform bins on [rmin, rmax), rmax <= rcut, for each of
        the ntypes (ntypes + 1)/2 pair types, at most 8192 counters in all; `n`: how many of `types` to use (default: all; without
        types: n_max).  Returns a PairHistogram: the `hist` of pair_hist_accumulate."""
        return PairHistogram(self, types, ntypes, nbins, rmin, rmax, n)

    def pair_hist_accumulate(self, pos, hist, counts, group=None, exclusions=None):
        """One sample of the pair distances (pse_pair_hist_accumulate): every unordered pair with rmin <= r < rmax, r > 0 adds 1 to
        counts[p, b], p = pair_type_index of its types, b its bin.  `counts`: a contiguous (npt, nbins) int64 CUDA tensor, ADDED to --
        zero it once, accumulate as many samples as you like.  exclusions: an ExclusionList whose pairs are not counted.  Queue-only:
        nothing is read back; integers only, so the counts are exact and do not depend on the order of the particles.  Returns counts."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        if not (_is_cuda(counts, torch.int64) and tuple(counts.shape) == (hist.npt, hist.nbins)):
            raise ValueError(f"counts must be a contiguous ({hist.npt}, {hist.nbins}) int64 CUDA tensor")
        _lib.check(self._lib.pse_pair_hist_accumulate(hist._handle(self), _ptr(pos), _ptr(group), n, _ptr(counts),
                                                      None if exclusions is None else exclusions._handle(self)))
        return counts

    def structure_factor(self, types, ntypes, modes, n=None):
        """A static structure factor on the device (pse_structure_factor_create; see include/pse_amd.h): `types` (n,) the type of
        every caller-order particle, below `ntypes` <= 8, or None: one type; `modes` (nk, 3) integers (mx, my, mz) within +-4096, at
        most 32768, of the reciprocal lattice of whatever box the engine has when a sample is taken; `n`: how many of `types` to use
        (default: all; without types: n_max).  Returns a StructureFactorModes with nk, ntypes, npt and close(): the `sf` of
        structure_factor_accumulate."""
        return StructureFactorModes(self, types, ntypes, modes, n)

    def structure_factor_accumulate(self, pos, sf, rho=None, sums=None, group=None):
        """One sample of the densities rho_a(m) = sum_{j of type a} exp(-2 pi i m.s_j) in the engine's current box
        (pse_structure_factor_accumulate).  `rho`: a contiguous (ntypes, nk, 2) float64 CUDA tensor, (re, im), OVERWRITTEN; `sums`: a
        contiguous (npt, nk) float64 CUDA tensor, ADDED to: sums[p, q] += Re(rho_a conj rho_b), p = pair_type_index(a, b) -- zero it
        once, accumulate as many samples as you like.  Either may be None, not both.  Queue-only: nothing is read back, the sort and
        the neighbour list are not touched; no atomics, equal inputs give equal bits.  Returns (rho, sums)."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        for t, name, shape in ((rho, "rho", (sf.ntypes, sf.nk, 2)), (sums, "sums", (sf.npt, sf.nk))):
            if t is not None and not (_is_cuda(t, torch.float64) and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {shape} float64 CUDA tensor")
        if rho is None and sums is None:
            raise ValueError("rho and sums are both None: nothing to compute")
        _lib.check(self._lib.pse_structure_factor_accumulate(sf._handle(self), _ptr(pos), _ptr(group), n, _ptr(rho), _ptr(sums)))
        return rho, sums

    def msd_origins(self, types, ntypes, norigins, n=None):
        """Displacement origins on the device (pse_msd_create; see include/pse_amd.h): `types` (n,) the type of every caller-order
        particle, below `ntypes` <= 8, or None: one type; `norigins` <= 64 slots of n_max unwrapped positions, zeroed; `n`: how many of
        `types` to use (default: all; without types: n_max).  Returns a DisplacementOrigins with ntypes, norigins and close()."""
        return DisplacementOrigins(self, types, ntypes, norigins, n)

    @staticmethod
    def _msd_common(pos, image, group):
        import torch
        _chk4(pos, "pos"); _chk_group(group)
        _chk_arr(image, "image", 3, torch.int32, pos.shape[0])
        return pos.shape[0] if group is None else group.shape[0]

    def msd_store(self, pos, image, origins, slot, strain, group=None):
        """The unwrapped positions x + ix Lx + iy strain Ly, y + iy Ly, z + iz Lz of the group into slot `slot` of `origins`
        (pse_msd_store), in the engine's current box lengths.  `strain`: the accumulated tilt (System.strain), NOT the box's xy.
        With it the unwrapped x survives a flip, but a y image gained AFTER a flip shifts it by flips Ly (include/pse_amd.h, LIMIT):
        the moments with x are right for a sheared run only while no particle gains a y image after a flip; y and z always are.
        Queue-only."""
        n = self._msd_common(pos, image, group)
        slot = int(slot)
        if not 0 <= slot < origins.norigins:
            raise ValueError(f"slot = {slot} outside [0, {origins.norigins})")
        _lib.check(self._lib.pse_msd_store(origins._handle(self), slot, _ptr(pos), _ptr(image), _ptr(group), n, _finite(strain, "strain")))

    def msd_accumulate(self, pos, image, origins, strain, slots, rows, sums, group=None):
        """One sample of the displacement moments (pse_msd_accumulate): for every pair (slots[q], rows[q]) and every type a,
        sums[rows[q], a, :] += the ten moments dx dy dz, dx^2 dy^2 dz^2 dxdy dxdz dydz, |d|^4 of d = r_u(now) - r_u(slot) summed over
        the group members of type a.  `sums`: a contiguous (nrows, ntypes, 10) float64 CUDA tensor, ADDED to; at most 64 pairs, every
        slot stored before, no row twice; the group must be the one the slots were stored with.  Queue-only: nothing is read back,
        no atomics, equal inputs give equal bits.  Returns sums."""
        import torch
        n = self._msd_common(pos, image, group)
        if not (_is_cuda(sums, torch.float64) and sums.dim() == 3 and sums.shape[0] >= 1
                and tuple(sums.shape[1:]) == (origins.ntypes, MSD_MOMENTS)):
            raise ValueError(f"sums must be a contiguous (nrows, {origins.ntypes}, {MSD_MOMENTS}) float64 CUDA tensor")
        slots, rows = _msd_pairs(slots, rows, origins.norigins, int(sums.shape[0]))
        _lib.check(self._lib.pse_msd_accumulate(origins._handle(self), _ptr(pos), _ptr(image), _ptr(group), n, _finite(strain, "strain"),
                                                int(slots.shape[0]), _vp(slots), _vp(rows), int(sums.shape[0]), _ptr(sums)))
        return sums

    def msd_displacement(self, pos, image, origins, slot, strain, out=None, group=None):
        """The displacement of every group member against slot `slot` (pse_msd_displacement): out[t] = (dx, dy, dz, |d|^2), a
        contiguous (N, 4) float64 CUDA tensor in the caller's order (default: a new one of zeros); rows outside the group are not
        touched.  Queue-only.  Returns out."""
        import torch
        n = self._msd_common(pos, image, group)
        slot = int(slot)
        if not 0 <= slot < origins.norigins:
            raise ValueError(f"slot = {slot} outside [0, {origins.norigins})")
        if out is None:
            out = torch.zeros_like(pos)
        _chk4(out, "out", pos.shape[0])
        _lib.check(self._lib.pse_msd_displacement(origins._handle(self), slot, _ptr(pos), _ptr(image), _ptr(group), n,
                                                  _finite(strain, "strain"), _ptr(out)))
        return out

    def isf_origins(self, types, ntypes, modes, norigins, n=None):
        """Scattering origins on the device (pse_isf_create; see include/pse_amd.h): `types` (n,) the type of every caller-order
        particle, below `ntypes` <= 8, or None: one type; `modes` (nk, 3) integers (mx, my, mz) within +-4096, at most 4096, of the
        reciprocal lattice of whatever box the engine has when a sample is taken; `norigins` <= 64 slots; `n`: how many of `types` to
        use (default: all; without types: n_max).  Returns a ScatteringOrigins with nk, ntypes, npt, norigins and close()."""
        return ScatteringOrigins(self, types, ntypes, modes, norigins, n)

    def isf_sample(self, pos, isf, rho=None, static_sums=None, group=None):
        """One sample into the current buffer of `isf` (pse_isf_sample): the fractional coordinates of the group in the engine's
        current box and the densities rho_a(m), by the pass of structure_factor_accumulate -- `rho` (a contiguous (ntypes, nk, 2)
        float64 CUDA tensor, WRITTEN) and `static_sums` ((npt, nk), ADDED to) get its bits; either may be None, and both.  Every
        sample of one object must use the same group.  Queue-only.  Returns (rho, static_sums)."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        for t, name, shape in ((rho, "rho", (isf.ntypes, isf.nk, 2)), (static_sums, "static_sums", (isf.npt, isf.nk))):
            if t is not None and not (_is_cuda(t, torch.float64) and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {shape} float64 CUDA tensor")
        _lib.check(self._lib.pse_isf_sample(isf._handle(self), _ptr(pos), _ptr(group), n, _ptr(rho), _ptr(static_sums)))
        isf.sample_n, isf._group = int(n), group   # (the device object remembers the group's pointer: the tensor must live as long)
        return rho, static_sums

    def isf_store(self, isf, slot):
        """The current buffer of `isf` into its origin slot `slot` (pse_isf_store).  Queue-only."""
        slot = int(slot)
        if not 0 <= slot < isf.norigins:
            raise ValueError(f"slot = {slot} outside [0, {isf.norigins})")
        if not isf.sample_n:
            raise ValueError("no isf_sample yet: the current buffer holds nothing")
        _lib.check(self._lib.pse_isf_store(isf._handle(self), slot))
        isf.slot_n[slot] = isf.sample_n

    def isf_correlate(self, isf, slots, rows, self_sums=None, coll=None):
        """The current buffer of `isf` against stored origins (pse_isf_correlate): for every pair (slots[q], rows[q]), types a, b and
        mode m, self_sums[rows[q], a, m] += (re, im) of the sum over the group members of type a of exp(-2 pi i m.(s(now) - s(slot)))
        and coll[rows[q], a, b, m] += Re(rho_a(m; now) conj rho_b(m; slot)).  `self_sums`: a contiguous (nrows, ntypes, nk, 2)
        float64 CUDA tensor, `coll`: (nrows, ntypes, ntypes, nk), both ADDED to, either may be None, not both; at most 64 pairs,
        every slot stored before with the N of the current sample, no row twice.  Queue-only: nothing is read back, no atomics, equal
        inputs give equal bits.  Returns (self_sums, coll)."""
        import torch
        if self_sums is None and coll is None:
            raise ValueError("self_sums and coll are both None: nothing to compute")
        first = self_sums if self_sums is not None else coll
        nrows = int(first.shape[0]) if _is_cuda(first, torch.float64) and first.dim() >= 1 else 0
        for t, name, tail in ((self_sums, "self_sums", (isf.ntypes, isf.nk, 2)), (coll, "coll", (isf.ntypes, isf.ntypes, isf.nk))):
            if t is not None and not (_is_cuda(t, torch.float64) and nrows >= 1 and tuple(t.shape) == (nrows,) + tail):
                raise ValueError(f"{name} must be a contiguous {('nrows',) + tail} float64 CUDA tensor, nrows the same for both")
        if not isf.sample_n:
            raise ValueError("no isf_sample yet: the current buffer holds nothing")
        slots, rows = _msd_pairs(slots, rows, isf.norigins, nrows)
        for q, sl in enumerate(slots.tolist()):
            if isf.slot_n[sl] != isf.sample_n:
                raise ValueError(f"pair {q} names the slot {sl}, " + ("which was never stored" if not isf.slot_n[sl] else
                                 f"stored with N = {isf.slot_n[sl]}: the current sample has N = {isf.sample_n}"))
        _lib.check(self._lib.pse_isf_correlate(isf._handle(self), int(slots.shape[0]), _vp(slots), _vp(rows), nrows, _ptr(self_sums),
                                               _ptr(coll)))
        return self_sums, coll

    def clusters(self, types, ntypes, rlink, n=None):
        """The link criterion of a cluster analysis on the device (pse_clusters_create; see include/pse_amd.h): `types` (n,) the type
        of every caller-order particle, below `ntypes` <= 8, or None: one type; `rlink`: a scalar, a dict {(a, b): r} (a missing pair
        is off) or npt entries, each 0 (off) or in (0, rcut]; `n`: how many of `types` to use (default: all; without types: n_max).
        Returns a ClusterLinks: the `links` of cluster_label."""
        return ClusterLinks(self, types, ntypes, rlink, n)

    def cluster_label(self, pos, links, label=None, size=None, stats=None, hist=None, group=None, exclusions=None):
        """The connected components of the links among the group members (pse_clusters_label): two particles are linked when
        0 < r < rlink of their pair of types and the pair is not in `exclusions`.  All outputs are CUDA tensors, any may be None, not all:
        `label`, `size`: contiguous 1-D int32 or int64 tensors of at least pos.shape[0] entries, by caller index -- the smallest
        caller index of the particle's cluster and its number of members; entries outside the group are left alone;
        `stats`: contiguous (4,) int64, OVERWRITTEN with the number of clusters, the largest size, the sum of s^2 and N;
        `hist`: contiguous 1-D int64, ADDED to: a cluster of size s adds 1 to hist[min(s, len(hist)) - 1].
        Queue-only: nothing is read back (an int64 label or size goes through an int32 copy on the device); integers only, so the
        result does not depend on the order of the particles.  Returns (label, size, stats, hist)."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        for t, name in ((label, "label"), (size, "size")):
            if t is not None and not (_is_cuda(t, torch.int32, torch.int64) and t.dim() == 1 and t.shape[0] >= pos.shape[0]):
                raise ValueError(f"{name} must be a contiguous 1-D int32 or int64 CUDA tensor of at least {pos.shape[0]} entries")
        if stats is not None and not (_is_cuda(stats, torch.int64) and tuple(stats.shape) == (4,)):
            raise ValueError("stats must be a contiguous (4,) int64 CUDA tensor")
        if hist is not None and not (_is_cuda(hist, torch.int64) and hist.dim() == 1 and hist.shape[0] >= 1):
            raise ValueError("hist must be a contiguous 1-D int64 CUDA tensor of at least one entry")
        if label is None and size is None and stats is None and hist is None:
            raise ValueError("label, size, stats and hist are all None: nothing to compute")
        obj = links._handle(self)
        ex = None if exclusions is None else exclusions._handle(self)
        narrow = [None if t is None or t.dtype == torch.int32 else t.to(torch.int32) for t in (label, size)]   # (keeps the entries outside the group)
        l32, s32 = [t if w is None else w for t, w in zip((label, size), narrow)]
        _lib.check(self._lib.pse_clusters_label(obj, _ptr(pos), _ptr(group), n, _ptr(l32), _ptr(s32), _ptr(stats), _ptr(hist),
                                                0 if hist is None else int(hist.shape[0]), ex))
        for t, w in zip((label, size), narrow):
            if w is not None:
                t.copy_(w)
        return label, size, stats, hist

    def cluster_span(self, pos, links, label=None, size=None, stats=None, hist=None, span=None, image=None, rg2=None, pstats=None,
                     group=None, exclusions=None):
        """cluster_label with percolation (pse_clusters_span; the definitions are in include/pse_amd.h): `label`, `size`, `stats`,
        `hist` as there, bit for bit, and
        `span`: contiguous 1-D int32 of at least pos.shape[0] entries, by caller index -- bits 0, 1, 2 set when the particle's cluster
        is connected to its own periodic image along the lattice axis a1, a2, a3;
        `image`: contiguous (>= pos.shape[0], 3) int32 -- the lattice vector that, added to the particle, makes its cluster whole
        around the cluster's label member; zeros in a spanning cluster;
        `rg2`: contiguous 1-D float64 of at least pos.shape[0] entries -- the squared radius of gyration of the particle's cluster, 0
        for a singleton, -1 for a spanning cluster;
        `pstats`: contiguous (8,) int64, OVERWRITTEN: spanning clusters, their members, clusters spanning a1, a2, a3, all three, the
        largest size and the sum of s^2 among the clusters that span nothing.
        All may be None, not all.  Queue-only, integers only behind the fixed-point conversion: equal inputs give equal bits.
        Returns (label, size, stats, hist, span, image, rg2, pstats)."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        rows = pos.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        for t, name in ((label, "label"), (size, "size")):
            if t is not None and not (_is_cuda(t, torch.int32, torch.int64) and t.dim() == 1 and t.shape[0] >= rows):
                raise ValueError(f"{name} must be a contiguous 1-D int32 or int64 CUDA tensor of at least {rows} entries")
        if stats is not None and not (_is_cuda(stats, torch.int64) and tuple(stats.shape) == (4,)):
            raise ValueError("stats must be a contiguous (4,) int64 CUDA tensor")
        if hist is not None and not (_is_cuda(hist, torch.int64) and hist.dim() == 1 and hist.shape[0] >= 1):
            raise ValueError("hist must be a contiguous 1-D int64 CUDA tensor of at least one entry")
        if span is not None and not (_is_cuda(span, torch.int32) and span.dim() == 1 and span.shape[0] >= rows):
            raise ValueError(f"span must be a contiguous 1-D int32 CUDA tensor of at least {rows} entries")
        if image is not None and not (_is_cuda(image, torch.int32) and image.dim() == 2 and image.shape[1] == 3 and image.shape[0] >= rows):
            raise ValueError(f"image must be a contiguous (>= {rows}, 3) int32 CUDA tensor")
        if rg2 is not None and not (_is_cuda(rg2, torch.float64) and rg2.dim() == 1 and rg2.shape[0] >= rows):
            raise ValueError(f"rg2 must be a contiguous 1-D float64 CUDA tensor of at least {rows} entries")
        if pstats is not None and not (_is_cuda(pstats, torch.int64) and tuple(pstats.shape) == (8,)):
            raise ValueError("pstats must be a contiguous (8,) int64 CUDA tensor")
        if all(t is None for t in (label, size, stats, hist, span, image, rg2, pstats)):
            raise ValueError("label, size, stats, hist, span, image, rg2 and pstats are all None: nothing to compute")
        obj = links._handle(self)
        ex = None if exclusions is None else exclusions._handle(self)
        narrow = [None if t is None or t.dtype == torch.int32 else t.to(torch.int32) for t in (label, size)]   # (keeps the entries outside the group)
        l32, s32 = [t if w is None else w for t, w in zip((label, size), narrow)]
        _lib.check(self._lib.pse_clusters_span(obj, _ptr(pos), _ptr(group), n, _ptr(l32), _ptr(s32), _ptr(stats), _ptr(hist),
                                               0 if hist is None else int(hist.shape[0]), _ptr(span), _ptr(image), _ptr(rg2), _ptr(pstats), ex))
        for t, w in zip((label, size), narrow):
            if w is not None:
                t.copy_(w)
        return label, size, stats, hist, span, image, rg2, pstats

    def bond_order_shells(self, types, ntypes, rnb, degrees=(4, 6), n=None):
        """The neighbour criterion and the degrees of a bond-order analysis on the device (pse_bond_order_create; see
        include/pse_amd.h): `types` (n,) the type of every caller-order particle, below `ntypes` <= 8, or None: one type; `rnb`: a
        scalar, a dict {(a, b): r} (a missing pair is off) or npt entries, each 0 (off) or in (0, rcut]; `degrees`: 1 to 4 distinct
        even l from 2 to 12; `n`: how many of `types` to use (default: all; without types: n_max).  Returns a BondOrderShells: the
        `shells` of bond_order."""
        return BondOrderShells(self, types, ntypes, rnb, degrees, n)

    def bond_order(self, pos, shells, nnb=None, q=None, qbar=None, solid=None, nconn=None, stats=None, group=None, exclusions=None):
        """The Steinhardt bond-orientational order of the group members (pse_bond_order_compute): two particles are neighbours when
        0 < r < rnb of their pair of types and the pair is not in `exclusions`.  All outputs are CUDA tensors, any may be None, not all:
        `nnb`, `nconn`: contiguous 1-D int32 tensors of at least pos.shape[0] entries, by caller index -- the number of neighbours
        and the number of them connected by a solid-like bond; `q`, `qbar`: contiguous (>= pos.shape[0], nl) float64 -- q_l and the
        neighbour-averaged q-bar_l, one column per degree of `shells`; entries outside the group are left alone;
        `stats`: contiguous (ntypes, 2) int64, OVERWRITTEN with the members and the solid-like members of every type.
        `solid`: None (no solid-bond pass: nconn is not written, the solid counts are 0) or (degree, threshold, min_conn): a bond is
        solid-like when the normalised product s_ij of the two c_lm vectors of `degree` exceeds `threshold`, a particle with at least
        `min_conn` of them.  Queue-only: nothing is read back, no floating-point atomics: equal inputs give equal bits.
        Returns (nnb, q, qbar, nconn, stats)."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        for t, name in ((nnb, "nnb"), (nconn, "nconn")):
            if t is not None and not (_is_cuda(t, torch.int32) and t.dim() == 1 and t.shape[0] >= pos.shape[0]):
                raise ValueError(f"{name} must be a contiguous 1-D int32 CUDA tensor of at least {pos.shape[0]} entries")
        for t, name in ((q, "q"), (qbar, "qbar")):
            if t is not None and not (_is_cuda(t, torch.float64) and t.dim() == 2 and t.shape[0] >= pos.shape[0]
                                      and t.shape[1] == shells.nl):
                raise ValueError(f"{name} must be a contiguous (N >= {pos.shape[0]}, {shells.nl}) float64 CUDA tensor")
        if stats is not None and not (_is_cuda(stats, torch.int64) and tuple(stats.shape) == (shells.ntypes, 2)):
            raise ValueError(f"stats must be a contiguous ({shells.ntypes}, 2) int64 CUDA tensor")
        if nnb is None and q is None and qbar is None and nconn is None and stats is None:
            raise ValueError("nnb, q, qbar, nconn and stats are all None: nothing to compute")
        column, threshold, min_conn = -1, 0.0, 0
        if solid is not None:
            degree, threshold, min_conn = solid
            column, threshold, min_conn = shells.column(degree), _finite(threshold, "threshold"), int(min_conn)
            if not -1.0 <= threshold <= 1.0:
                raise ValueError(f"threshold = {threshold} outside [-1, 1]")
            if not 0 <= min_conn < 2 ** 32:
                raise ValueError(f"min_conn = {min_conn} outside [0, 2^32)")
        _lib.check(self._lib.pse_bond_order_compute(shells._handle(self), _ptr(pos), _ptr(group), n, _ptr(nnb), _ptr(q), _ptr(qbar), column,
                                                    threshold, min_conn, _ptr(nconn), _ptr(stats),
                                                    None if exclusions is None else exclusions._handle(self)))
        return nnb, q, qbar, nconn, stats

    def bond_order_histogram(self, values, shells, l, counts, lo=0.0, hi=1.0, group=None, n=None):
        """One sample of the per-type distribution of a bond-order parameter (pse_bond_order_histogram): the group member t of type a
        with lo <= v < hi, v = values[t, column of degree l], adds 1 to counts[a, b], b = min(int((v - lo) nbins / (hi - lo)),
        nbins - 1).  `values`: a contiguous (N, nl) float64 CUDA tensor by caller index, q or qbar of bond_order; `counts`: a
        contiguous (ntypes, nbins) int64 CUDA tensor, ADDED to; `n`: the number of group members without a group (default: the rows
        of values).  Queue-only; integers only.  Returns counts."""
        import torch
        if not (_is_cuda(values, torch.float64) and values.dim() == 2 and values.shape[1] == shells.nl):
            raise ValueError(f"values must be a contiguous (N, {shells.nl}) float64 CUDA tensor")
        _chk_group(group)
        if not (_is_cuda(counts, torch.int64) and counts.dim() == 2 and counts.shape[0] == shells.ntypes and counts.shape[1] >= 1):
            raise ValueError(f"counts must be a contiguous ({shells.ntypes}, nbins) int64 CUDA tensor")
        if shells.ntypes * int(counts.shape[1]) > BOND_ORDER_MAX_COUNTERS:
            raise ValueError(f"{shells.ntypes} types x {int(counts.shape[1])} bins, more than {BOND_ORDER_MAX_COUNTERS} counters")
        lo, hi = _finite(lo, "lo"), _finite(hi, "hi")
        if not hi > lo:
            raise ValueError(f"hi = {hi} must exceed lo = {lo}")
        members = (values.shape[0] if n is None else int(n)) if group is None else group.shape[0]
        if group is None and members > values.shape[0]:
            raise ValueError("n exceeds the rows of values")
        _lib.check(self._lib.pse_bond_order_histogram(shells._handle(self), _ptr(values), shells.column(l), _ptr(group), members,
                                                      int(counts.shape[1]), lo, hi, _ptr(counts)))
        return counts

    def molecule_topology(self, pairs, mol_types=None, ntypes=1, nbins=0, rg_max=None, ree_max=None, n=None):
        """The molecules of a bond topology on the device (pse_molecules_create; see include/pse_amd.h and MoleculeTopology).
        Returns a MoleculeTopology: the `molecules` of molecules_compute."""
        return MoleculeTopology(self, pairs, mol_types, ntypes, nbins, rg_max, ree_max, n)

    def molecules_compute(self, pos, molecules, rows=None, unfolded=None, sums=None, sample=None, hist=None):
        """The conformation of every molecule at `pos` in the engine's current box (pse_molecules_compute): each molecule is unfolded
        along its own bonds by the minimum image, which is right through any number of Lees-Edwards flips while every bond is shorter
        than half the smallest box length.  All outputs are contiguous CUDA tensors, any may be None, not all:
        `rows` (nmol, 14) float64, WRITTEN: c(3), G_xx, G_yy, G_zz, G_xy, G_xz, G_yz, Rg^2, R(3), R^2 (R: NaN without two ends);
        `unfolded` (N, 4) float64 by caller index, members WRITTEN with (r_root + u, molecule number), other rows left alone;
        `sums` (ntypes, 14) float64, ADDED to, and `sample` (ntypes, 14) float64, WRITTEN with this call's sums alone: the sums over
        the molecules of a type of G_ab (6), (Rg^2)^2, R_a R_b (6), (R^2)^2, the last seven over the linear molecules;
        `hist` (2, ntypes, nbins + 1) int64, ADDED to: Rg and |R|, the last counter for values at or above the maximum.
        Queue-only: nothing is read back, no floating-point atomics: equal inputs give equal bits.  Returns the five."""
        import torch
        _chk4(pos, "pos", molecules.n)
        shapes = ((rows, "rows", (molecules.nmol, MOL_COLS), torch.float64), (sums, "sums", (molecules.ntypes, MOL_COLS), torch.float64),
                  (sample, "sample", (molecules.ntypes, MOL_COLS), torch.float64),
                  (hist, "hist", (2, molecules.ntypes, molecules.nbins + 1), torch.int64))
        for t, name, shape, dtype in shapes:
            if t is not None and not (_is_cuda(t, dtype) and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {shape} {dtype} CUDA tensor")
        if unfolded is not None:
            _chk4(unfolded, "unfolded", molecules.n)
        if hist is not None and molecules.nbins == 0:
            raise ValueError("hist given, but the molecules were made with nbins = 0")
        if rows is None and unfolded is None and sums is None and sample is None and hist is None:
            raise ValueError("rows, unfolded, sums, sample and hist are all None: nothing to compute")
        _lib.check(self._lib.pse_molecules_compute(molecules._handle(self), _ptr(pos), _ptr(rows), _ptr(unfolded), _ptr(sums), _ptr(sample),
                                                   _ptr(hist)))
        return rows, unfolded, sums, sample, hist

    def molecule_pairs(self, pairs, mol_types=None, ntypes=1, ns=1, n=None):
        """The molecules of a bond topology with their chain ranks on the device (pse_molecule_pairs_create; see include/pse_amd.h
        and MoleculePairs).  Returns a MoleculePairs: the `pairs` of molecule_pairs_compute."""
        return MoleculePairs(self, pairs, mol_types, ntypes, ns, n)

    def molecule_pairs_compute(self, pos, pairs, inv_rh=None, curves=None, sums=None, sample=None):
        """The pair sums of every molecule at `pos` in the engine's current box (pse_molecule_pairs_compute), on the offsets that
        molecules_compute unfolds.  All outputs are contiguous float64 CUDA tensors, any may be None, not all:
        `inv_rh` (nmol,), WRITTEN: 1/Rh = (1/m^2) sum over i != j of 1/r_ij (a pair at distance 0 adds nothing);
        `curves` (ntypes, ns, 2), ADDED to: per type and separation s the sums over the linear molecules of D(s) = sum |u_{c+s} - u_c|^2
        and C(s) = sum b_c . b_{c+s};
        `sums` (ntypes, 2), ADDED to, and `sample` (ntypes, 2), WRITTEN with this call's sums alone: the sum of 1/Rh and of (1/Rh)^2.
        Queue-only: nothing is read back, no floating-point atomics: equal inputs give equal bits.  Returns the four."""
        import torch
        _chk4(pos, "pos", pairs.n)
        shapes = ((inv_rh, "inv_rh", (pairs.nmol,)), (curves, "curves", (pairs.ntypes, pairs.ns, MOLPAIR_COLS)),
                  (sums, "sums", (pairs.ntypes, MOLPAIR_SUMS)), (sample, "sample", (pairs.ntypes, MOLPAIR_SUMS)))
        for t, name, shape in shapes:
            if t is not None and not (_is_cuda(t, torch.float64) and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {shape} {torch.float64} CUDA tensor")
        if inv_rh is None and curves is None and sums is None and sample is None:
            raise ValueError("inv_rh, curves, sums and sample are all None: nothing to compute")
        _lib.check(self._lib.pse_molecule_pairs_compute(pairs._handle(self), _ptr(pos), _ptr(inv_rh), _ptr(curves), _ptr(sums), _ptr(sample)))
        return inv_rh, curves, sums, sample

    def chain_modes(self, pairs, sizes, weights, mol_types=None, ntypes=1, norigins=0, n=None):
        """The linear molecules of a bond topology with K weight rows per size and `norigins` origin slots on the device
        (pse_chain_modes_create; see include/pse_amd.h and ChainModes).  Returns a ChainModes: the `modes` of chain_modes_compute,
        chain_modes_store and chain_modes_correlate."""
        return ChainModes(self, pairs, sizes, weights, mol_types, ntypes, norigins, n)

    def chain_modes_compute(self, pos, modes, out=None, sums=None, sample=None):
        """X_k = sum_q w_{k,q} u_q of every linear molecule at `pos` in the engine's current box (pse_chain_modes_compute), on the
        offsets that molecules_compute unfolds, into the object's current buffer.  All outputs are contiguous float64 CUDA tensors,
        any may be None, and all of them: `out` (nlin, K, 3), WRITTEN; `sums` (ntypes, K, 6), ADDED to, and `sample` (ntypes, K, 6),
        WRITTEN with this call's sums alone: per type and k the sums over the linear molecules of X_x^2, X_y^2, X_z^2, X_x X_y,
        X_x X_z, X_y X_z.  Queue-only: nothing is read back, no floating-point atomics: equal inputs give equal bits.  Returns the three."""
        import torch
        _chk4(pos, "pos", modes.n)
        shapes = ((out, "out", (modes.nlin, modes.K, 3)), (sums, "sums", (modes.ntypes, modes.K, CHAIN_MODES_STATIC)),
                  (sample, "sample", (modes.ntypes, modes.K, CHAIN_MODES_STATIC)))
        for t, name, shape in shapes:
            if t is not None and not (_is_cuda(t, torch.float64) and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {shape} {torch.float64} CUDA tensor")
        _lib.check(self._lib.pse_chain_modes_compute(modes._handle(self), _ptr(pos), _ptr(out), _ptr(sums), _ptr(sample)))
        modes.computed = True
        return out, sums, sample

    def chain_modes_store(self, modes, slot):
        """The current buffer of `modes` into its origin slot `slot` (pse_chain_modes_store).  Queue-only."""
        slot = int(slot)
        if not 0 <= slot < modes.norigins:
            raise ValueError(f"slot = {slot} outside [0, {modes.norigins})")
        if not modes.computed:
            raise ValueError("no chain_modes_compute yet: the current buffer holds nothing")
        _lib.check(self._lib.pse_chain_modes_store(modes._handle(self), slot))
        modes.stored.add(slot)

    def chain_modes_correlate(self, modes, slots, rows, corr):
        """One sample of the time correlations (pse_chain_modes_correlate): for every pair (slots[q], rows[q]), type a and k,
        corr[rows[q], a, k, alpha, beta] += the sum over the linear molecules of type a of X_alpha(current buffer) X_beta(slot).
        `corr`: a contiguous (nrows, ntypes, K, 3, 3) float64 CUDA tensor, ADDED to; at most 64 pairs, every slot stored before, no
        row twice.  Queue-only: nothing is read back, no atomics, equal inputs give equal bits.  Returns corr."""
        import torch
        if not (_is_cuda(corr, torch.float64) and corr.dim() == 5 and corr.shape[0] >= 1
                and tuple(corr.shape[1:]) == (modes.ntypes, modes.K, 3, 3)):
            raise ValueError(f"corr must be a contiguous (nrows, {modes.ntypes}, {modes.K}, 3, 3) float64 CUDA tensor")
        if modes.norigins == 0:
            raise ValueError("these modes were made with norigins = 0: there is no origin to correlate with")
        if not modes.computed:
            raise ValueError("no chain_modes_compute yet: the current buffer holds nothing")
        slots, rows = _msd_pairs(slots, rows, modes.norigins, int(corr.shape[0]))
        missing = sorted(set(slots.tolist()) - modes.stored)
        if missing:
            raise ValueError(f"slot {missing[0]} was never stored")
        _lib.check(self._lib.pse_chain_modes_correlate(modes._handle(self), int(slots.shape[0]), _vp(slots), _vp(rows), int(corr.shape[0]),
                                                       _ptr(corr)))
        return corr

    def exclusions(self, pairs, n=None):
        """A set of excluded pairs on the device (pse_exclusions_create; HOOMD's nlist.reset_exclusions): `pairs` (npairs, 2)
        caller-order particle indices below `n` (default: n_max).  Returns an ExclusionList: the `exclusions=` of the pair passes."""
        return ExclusionList(self, pairs, n)

    def bonds(self, pairs, types=None, kinds=(0,), k=(1.0,), r0=(1.0,), n=None):
        """A bond topology on the device (pse_bonds_create; see include/pse_amd.h): `pairs` (nbonds, 2) particle indices into arrays of
        `n` rows (default: n_max), `types` (nbonds,) indices into the per-type sequences `kinds` ("harmonic" | "fene" or
        BOND_KINDS codes), `k`, `r0`, or None: all type 0.  Returns a BondList."""
        return BondList(self, pairs, types, kinds, k, r0, n)

    def angles(self, triples, types=None, kinds=(0,), k=(1.0,), theta0=(math.pi,), n=None):
        """An angle topology on the device (pse_angles_create; see include/pse_amd.h): `triples` (nangles, 3) particle indices (end,
        vertex, end) into arrays of `n` rows (default: n_max), `types` (nangles,) indices into the per-type sequences `kinds`
        ("harmonic" | "cosinesq" or ANGLE_KINDS codes), `k`, `theta0` (radians, in [0, pi]), or None: all type 0.  Returns an AngleList."""
        return AngleList(self, triples, types, kinds, k, theta0, n)

    def dihedrals(self, quads, types=None, kinds=(0,), params=((1.0, 1.0, 1.0, 0.0),), n=None):
        """A dihedral topology on the device (pse_dihedrals_create; see include/pse_amd.h): `quads` (ndihedrals, 4) particle indices
        (i, j, k, l) into arrays of `n` rows (default: n_max), `types` (ndihedrals,) indices into the per-type sequences `kinds`
        ("harmonic" | "opls" or DIHEDRAL_KINDS codes) and `params` (one 4-tuple per type: harmonic (k, d, mult, phi0), OPLS
        (k1, k2, k3, k4)), or None: all type 0.  phi is the IUPAC dihedral angle: cis 0, trans pi.  Returns a DihedralList."""
        return DihedralList(self, quads, types, kinds, params, None, n)


class StokesEngine(_ForcePasses):
    """The force passes on the engine of an integrator (integrate.PSEv1.engine): `cpp_method` is the C++ Stokes object, which owns
    the handle and replaces it in setParams().  Holds a reference to it, so that it outlives every object made here, and never
    destroys the handle."""

    def __init__(self, cpp_method, n_max):
        self.cpp_method, self.n_max, self._lib = cpp_method, int(n_max), _lib.load()

    @property
    def _h(self):
        h = self.cpp_method.handle()
        if not h:
            raise RuntimeError("Stokes::setParams() has not been called")
        return ctypes.c_void_p(h)

    @property
    def serial(self):
        return self.cpp_method.engineSerial()


class Engine(_ForcePasses):
    """One PSE engine instance == one `Stokes` object's device state (PSEv1/Stokes.h:128-150)."""

    serial = 0   # (_ForcePasses) close() is the one change
    n_max = property(lambda self: self.params.n_max)

    def __init__(self, n_max, box, xi=0.5, error=1e-3, max_strain=0.5, seed=0, grid=(0, 0, 0), P=0, rcut=0.0,
                 device=-1, n_slabs=1, slab_rank=0, local_rows=0, lanczos_operator=None):
        """lanczos_operator: "records16" (the 16-byte pair records, single-precision accurate) or "fp64" (the exact operator: tight
        tolerances of the Lanczos noise mean what they say); None keeps the handle's default (PSE_LANCZOS_OP in the environment)."""
        op = None if lanczos_operator is None else _lanczos_operator_code(lanczos_operator)
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        box = tuple(float(b) for b in box) + ((0.0,) if len(box) == 3 else ())
        self.params = pse_params(n_max=int(n_max), Lx=box[0], Ly=box[1], Lz=box[2], xy=box[3], xi=xi, error=error,
                                 max_strain=max_strain, seed=int(seed) & 0xFFFFFFFF, Nx=grid[0], Ny=grid[1],
                                 Nz=grid[2], P=P, rcut=rcut, device=device, n_slabs=n_slabs, slab_rank=slab_rank,
                                 local_rows=int(local_rows))
        _lib.check(self._lib.pse_create(ctypes.byref(self.params), ctypes.byref(self._h)))
        self.box = box
        if op is not None:
            _lib.check(self._lib.pse_set_lanczos_operator(self._h, op))

    def set_lanczos_operator(self, name):
        """The near-field operator of the Lanczos iteration from now on (pse_set_lanczos_operator): "records16" or "fp64".  A graph
        captured before the switch keeps its mode."""
        _lib.check(self._lib.pse_set_lanczos_operator(self._h, _lanczos_operator_code(name)))

    @property
    def lanczos_operator(self):
        """"records16" or "fp64" (pse_get_lanczos_operator)."""
        v = ctypes.c_int(-1)
        _lib.check(self._lib.pse_get_lanczos_operator(self._h, ctypes.byref(v)))
        return {c: n for n, c in LANCZOS_OPERATORS.items()}[v.value]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.pse_destroy(self._h)
            self._h = ctypes.c_void_p()
            self.serial = 1

    __del__ = close

    def info(self):
        out = pse_info()
        _lib.check(self._lib.pse_get_info(self._h, ctypes.byref(out)))
        return out.as_dict()

    def local_layout(self):
        """Row capacities of an owned-particle handle (local_rows=1): dict rows_own (capacity of the caller's arrays), rows_ghost,
        records (per neighbour message), layers (cell layers along x), layers_per_rank."""
        v = [ctypes.c_int() for _ in range(5)]
        _lib.check(self._lib.pse_local_layout(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("rows_own", "rows_ghost", "records", "layers", "layers_per_rank"), [x.value for x in v]))

    def set_box(self, Lx, Ly, Lz, xy):
        _lib.check(self._lib.pse_set_box(self._h, Lx, Ly, Lz, xy))
        self.box = (Lx, Ly, Lz, xy)

    def set_timing(self, on=True):
        _lib.check(self._lib.pse_set_timing(self._h, 1 if on else 0))

    def set_async(self, on=True):
        """Deterministic evaluations only queue work (no read-back, capturable into a hipGraph); reuse or rebuild of the kept
        neighbour list is decided on the device."""
        _lib.check(self._lib.pse_set_async(self._h, 1 if on else 0))

    def set_timestep_offset(self, word):
        """word: a 1-element int32/uint32 CUDA tensor (or None): Brownian calls draw their noise at timestep + word[0], read on the
        device -- what lets a captured step replay with fresh noise.  The tensor must outlive the registration."""
        self._ts_word = word
        _lib.check(self._lib.pse_set_timestep_offset(self._h, _ptr(word)))

    def debug_last_gate(self):
        """0: the last asynchronous evaluation reused the kept list, != 0: it rebuilt, -1: it did not take the two-chain path."""
        g = ctypes.c_int(-2)
        _lib.check(self._lib.pse_debug_last_gate(self._h, ctypes.byref(g)))
        return g.value

    def set_neighbor_skin(self, r_buff):
        """r_buff of the neighbour list kept across calls (HOOMD's nlist r_buff, PSEv1/integrate.py:60); 0 rebuilds every call."""
        _lib.check(self._lib.pse_set_neighbor_skin(self._h, float(r_buff)))

    def neighbor_stats(self):
        """(r_buff, builds, reuses) of the kept neighbour list."""
        r, b, u = ctypes.c_double(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
        _lib.check(self._lib.pse_neighbor_stats(self._h, ctypes.byref(r), ctypes.byref(b), ctypes.byref(u)))
        return r.value, b.value, u.value

    def set_stream(self, stream_ptr):
        _lib.check(self._lib.pse_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    # -- hot path -------------------------------------------------------------------------------------------
    def mobility(self, pos, force, vel=None, group=None, parts=3):
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk4(force, "force"); _chk_group(group)
        if vel is None:
            vel = torch.zeros_like(pos)
        _chk4(vel, "vel")
        _lib.check(self._lib.pse_mobility(self._h, _ptr(pos), _ptr(force), _ptr(vel), _ptr(group), n, parts))
        return vel

    def brownian_velocity(self, pos, force, kT, dt, timestep, vel=None, group=None, lanczos_m=2):
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk4(force, "force"); _chk_group(group)
        if vel is None:
            vel = torch.zeros_like(pos)
        _chk4(vel, "vel")
        m = ctypes.c_int(int(lanczos_m))
        _lib.check(self._lib.pse_brownian_velocity(self._h, _ptr(pos), _ptr(force), _ptr(vel), _ptr(group), n,
                                                   float(kT), float(dt), int(timestep), ctypes.byref(m)))
        return vel, m.value

    def brownian_velocity_part(self, pos, force, kT, dt, timestep, parts, vel=None, group=None, lanczos_m=2):
        """One half of brownian_velocity (pse_brownian_velocity_part): parts = 1 real space + Lanczos noise, 2 wave space + k-space noise."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk4(force, "force"); _chk_group(group)
        if vel is None:
            vel = torch.zeros_like(pos)
        _chk4(vel, "vel")
        m = ctypes.c_int(int(lanczos_m))
        _lib.check(self._lib.pse_brownian_velocity_part(self._h, _ptr(pos), _ptr(force), _ptr(vel), _ptr(group), n, float(kT), float(dt),
                                                        int(timestep), int(parts), ctypes.byref(m)))
        return vel, m.value

    def integrate(self, pos, vel, accel, image, force, dt, shear_rate=0.0, group=None):
        """The Euler update + wrap alone (pse_integrate) for velocities the caller has put together."""
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk4(vel, "vel"); _chk4(force, "force"); _chk_group(group)
        _chk_arr(accel, "accel", 3, torch.float64, pos.shape[0]); _chk_arr(image, "image", 3, torch.int32, pos.shape[0])
        _lib.check(self._lib.pse_integrate(self._h, _ptr(pos), _ptr(vel), _ptr(accel), _ptr(image), _ptr(force), _ptr(group), n, float(dt),
                                           float(shear_rate)))

    def step(self, pos, vel, accel, image, force, kT, dt, timestep, shear_rate=0.0, group=None, lanczos_m=2):
        n = pos.shape[0] if group is None else group.shape[0]
        import torch
        _chk4(pos, "pos"); _chk4(vel, "vel"); _chk4(force, "force"); _chk_group(group)
        _chk_arr(accel, "accel", 3, torch.float64, pos.shape[0]); _chk_arr(image, "image", 3, torch.int32, pos.shape[0])
        m = ctypes.c_int(int(lanczos_m))
        _lib.check(self._lib.pse_step(self._h, _ptr(pos), _ptr(vel), _ptr(accel), _ptr(image), _ptr(force),
                                      _ptr(group), n, float(kT), float(dt), int(timestep), float(shear_rate),
                                      ctypes.byref(m)))
        return m.value

    def sqrt_mreal(self, pos, psi, tol=1e-3, group=None, lanczos_m=2):
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk4(psi, "psi"); _chk_group(group)
        out = torch.zeros_like(psi)
        m = ctypes.c_int(int(lanczos_m))
        _lib.check(self._lib.pse_sqrt_mreal(self._h, _ptr(pos), _ptr(psi), _ptr(out), _ptr(group), n, float(tol),
                                            ctypes.byref(m)))
        return out, m.value

    def random_psi(self, n, timestep, group=None):
        import torch
        rows = n if group is None else int(group.max().item()) + 1
        psi = torch.zeros((rows, 4), dtype=torch.float64, device="cuda")
        _lib.check(self._lib.pse_random_psi(self._h, _ptr(psi), _ptr(group), n, int(timestep)))
        return psi

    # -- introspection ---------------------------------------------------------------------------------------
    def eval_realspace(self, r):
        import numpy as np
        r = np.ascontiguousarray(r, dtype=np.float64)
        f = np.zeros_like(r); g = np.zeros_like(r)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(self._lib.pse_eval_realspace(self._h, r.ctypes.data_as(dp), len(r), f.ctypes.data_as(dp),
                                                g.ctypes.data_as(dp)))
        return f, g

    def debug_spread(self, pos, force, group=None):
        """The three force grids right after the spread (3, Nx, Ny, Nz), host array."""
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk4(force, "force"); _chk_group(group)
        _lib.check(self._lib.pse_debug_spread(self._h, _ptr(pos), _ptr(force), _ptr(group), n))
        return self.debug_grid()

    def debug_gather(self, pos, grid, group=None):
        """The gather alone: (N, 4) velocities (caller order) that the three host grids `grid` (3, Nx, Ny, Nz) give at the particles."""
        import numpy as np
        import torch
        n = pos.shape[0] if group is None else group.shape[0]
        _chk4(pos, "pos"); _chk_group(group)
        i = self.info()
        grid = np.ascontiguousarray(grid, dtype=np.float64)
        if grid.shape != (3, i["Nx"] // max(1, self.params.n_slabs), i["Ny"], i["Nz"]):
            raise ValueError(f"grid must have the shape of debug_grid(), not {grid.shape}")
        vel = torch.zeros_like(pos)
        _lib.check(self._lib.pse_debug_gather(self._h, _ptr(pos), grid.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _ptr(group), n,
                                              _ptr(vel)))
        return vel

    FAR_PATH_FIELDS = ("spread_fast", "TZ", "NW", "gather_fast", "BZ", "shear")

    def far_path(self, n):
        """Which far-field kernels a call with n particles launches (pse_debug_far_path): dict of FAR_PATH_FIELDS."""
        out = (ctypes.c_int * 6)()
        _lib.check(self._lib.pse_debug_far_path(self._h, int(n), out))
        return dict(zip(self.FAR_PATH_FIELDS, out))

    FFT_PATH_FIELDS = ("xfuse", "own_y", "own_z", "x", "x_kb", "y", "y_kb", "z")
    FFT_X_KERNELS = ("rocfft+k_scale", "k_xfft_scale", "k_xfft_scale_cols", "k_xfft_scale_mixed/ct", "k_xfft_scale_mixed/rt")
    FFT_Y_KERNELS = ("rocfft", "k_fft_cols/ct", "k_fft_cols/rt", "k_yfft_regs")
    FFT_Z_KERNELS = ("rocfft", "k_zfft_rows", "k_zfft_rows_g")

    def fft_path(self):
        """Which transform kernels this engine runs (pse_debug_fft_path): dict of FFT_PATH_FIELDS, the kernels by name (FFT_*_KERNELS),
        x_kb / y_kb the kz columns per workgroup (0 where rocFFT serves the axis)."""
        out = (ctypes.c_int * 8)()
        _lib.check(self._lib.pse_debug_fft_path(self._h, out))
        d = dict(zip(self.FFT_PATH_FIELDS, out))
        d["x"] = self.FFT_X_KERNELS[d["x"]]; d["y"] = self.FFT_Y_KERNELS[d["y"]]; d["z"] = self.FFT_Z_KERNELS[d["z"]]
        return d

    def debug_wave_grid(self, grid=None, xi=0.0, eta=0.0, noise=False, kT=0.0, dt=1.0, timestep=0, poison=True):
        """The wave-space stage alone, grid to grid (pse_debug_wave_grid): the host grids `grid` (3, Nx, Ny, Nz; None: zeros) through the
        forward transforms, the k-space operator (xi, eta > 0 replace the engine's own; + the k-space noise if `noise`) and the inverse
        transforms, as a step runs them; returns the (3, Nx, Ny, Nz) host array.  poison: both device grids are filled with NaN first."""
        import numpy as np
        i = self.info()
        shape = (3, i["Nx"] // max(1, self.params.n_slabs), i["Ny"], i["Nz"])
        dp = ctypes.POINTER(ctypes.c_double)
        src = None
        if grid is not None:
            grid = np.ascontiguousarray(grid, dtype=np.float64)
            if grid.shape != shape:
                raise ValueError(f"grid must have the shape of debug_grid(), not {grid.shape}")
            src = grid.ctypes.data_as(dp)
        out = np.zeros(shape)
        _lib.check(self._lib.pse_debug_wave_grid(self._h, src, float(xi), float(eta), int(bool(noise)), float(kT), float(dt), int(timestep),
                                                 int(bool(poison)), out.ctypes.data_as(dp)))
        return out

    def debug_kvector(self, ijk):
        """(n, 5): kx, ky, kz, w sinc^2, sqrt(w) sinc of the grid nodes ijk (n, 3) as the k-space kernels evaluate them."""
        import numpy as np
        ijk = np.ascontiguousarray(ijk, dtype=np.int32)
        out = np.zeros((len(ijk), 5))
        _lib.check(self._lib.pse_debug_kvector(self._h, len(ijk), ijk.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def set_lanczos_extra(self, extra):
        """Gated iterations a queue-only Brownian call queues beyond its starting count (pse_set_lanczos_extra; -1: the default, 0: none --
        for a time-stepping loop whose steps end at their starting count: pse_amd.sharded.LanczosCount)."""
        _lib.check(self._lib.pse_set_lanczos_extra(self._h, int(extra)))

    def matvec_ms(self, reps=20):
        """Milliseconds per launch of the pair-list mat-vec of a Lanczos iteration, `reps` launches back to back between one pair of
        events (pse_debug_matvec_ms): right after a Brownian call of a single-GPU engine."""
        ms = ctypes.c_float(0)
        _lib.check(self._lib.pse_debug_matvec_ms(self._h, int(reps), ctypes.byref(ms)))
        return ms.value

    def grid_placement(self):
        """What pse_create's grid-placement planner did: {"tried": pairs timed (0: off or not applicable), "ms_first", "ms_kept": the
        x pass + inverse y + z passes on the first pair allocated and on the one kept}."""
        n, a, b = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_float(0)
        _lib.check(self._lib.pse_debug_grid_placement(self._h, ctypes.byref(n), ctypes.byref(a), ctypes.byref(b)))
        return {"tried": n.value, "ms_first": a.value, "ms_kept": b.value}

    def debug_grid(self):
        import numpy as np
        i = self.info()
        out = np.zeros((3, i["Nx"] // max(1, self.params.n_slabs), i["Ny"], i["Nz"]))
        _lib.check(self._lib.pse_debug_copy_grid(self._h, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out


class Team:
    """A pse_team: the local slab ranks bound to a transport (RCCL across processes, or in-process loopback)."""

    def __init__(self, engines, unique_id=None, transport=None):
        """transport: an object with exchange(xfers) and allreduce_sum(array) (see pse_amd.sharded.TorchTransport): the
        host-staged third transport of include/pse_amd.h, one member per process."""
        self._lib = _lib.load()
        self.engines = list(engines)
        self._t = ctypes.c_void_p()
        if transport is not None:
            self._transport = transport              # the callbacks must outlive the team
            self._cb = _lib.pse_transport(None, _lib.EXCHANGE_FN(self._exchange), _lib.ALLREDUCE_FN(self._allreduce))
            _lib.check(self._lib.pse_team_create_transport(self.engines[0]._h, ctypes.byref(self._cb), ctypes.byref(self._t)))
            return
        arr = (ctypes.c_void_p * len(self.engines))(*[e._h for e in self.engines])
        idbuf = ctypes.create_string_buffer(bytes(unique_id), 128) if unique_id is not None else None
        _lib.check(self._lib.pse_team_create(arr, len(self.engines), idbuf, ctypes.byref(self._t)))

    def _exchange(self, _user, n, xfers):
        import numpy as np
        try:
            ops = []
            for q in range(n):
                x = xfers[q]
                send = np.ctypeslib.as_array(x.send, shape=(x.send_count,)) if x.send_count else None
                recv = np.ctypeslib.as_array(x.recv, shape=(x.recv_count,)) if x.recv_count else None
                ops.append((send, x.send_to, recv, x.recv_from))
            self._transport.exchange(ops)
            return 0
        except Exception as e:   # noqa: BLE001  (an exception must not unwind through the C caller)
            print("pse_amd transport: exchange failed:", repr(e))
            return 1

    def _allreduce(self, _user, buf, n):
        import numpy as np
        try:
            self._transport.allreduce_sum(np.ctypeslib.as_array(buf, shape=(n,)))
            return 0
        except Exception as e:   # noqa: BLE001
            print("pse_amd transport: all-reduce failed:", repr(e))
            return 1

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().pse_team_unique_id(buf))
        return buf.raw

    def debug_solo(self, slab_rank):
        """Developer switch: queue the work of one member only (see include/pse_amd.h); -1 switches it off."""
        _lib.check(self._lib.pse_team_debug_solo(self._t, int(slab_rank)))

    def close(self):
        if getattr(self, "_t", None) is not None and self._t.value:
            self._lib.pse_team_destroy(self._t)
            self._t = ctypes.c_void_p()

    __del__ = close

    @staticmethod
    def _ptrs(tensors):
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    @staticmethod
    def _chk(group, *lists):
        _chk_group(group)
        for name, ts in lists:
            for t in ts:
                _chk4(t, name)

    def mobility(self, pos, force, vel, group=None, parts=3):
        n = pos[0].shape[0] if group is None else group.shape[0]
        self._chk(group, ("pos", pos), ("force", force), ("vel", vel))
        _lib.check(self._lib.pse_team_mobility(self._t, self._ptrs(pos), self._ptrs(force), self._ptrs(vel), _ptr(group),
                                               n, parts))
        return vel

    def brownian_velocity(self, pos, force, vel, kT, dt, timestep, group=None, lanczos_m=2):
        n = pos[0].shape[0] if group is None else group.shape[0]
        self._chk(group, ("pos", pos), ("force", force), ("vel", vel))
        m = ctypes.c_int(int(lanczos_m))
        _lib.check(self._lib.pse_team_brownian_velocity(self._t, self._ptrs(pos), self._ptrs(force), self._ptrs(vel),
                                                        _ptr(group), n, float(kT), float(dt), int(timestep),
                                                        ctypes.byref(m)))
        return vel, m.value

    def step_local(self, pos, vel, accel, image, force, tag, n_local, kT, dt, timestep, shear_rate=0.0, integrate=True, lanczos_m=2):
        """Owned-particle step (pse_team_step_local): per member, rows [0, n_local[0]) of the arrays are the particles the rank owns;
        tag (int32, global indices) and n_local (1-element int32) are CUDA tensors, rewritten with the arrays.  Queue-only."""
        import torch
        for t in list(pos) + list(vel) + list(force):
            _chk4(t, "pos/vel/force")
        self._check_local_arrays(pos, vel, force, accel, image, tag)
        for a_, im_, tg, nl, p_ in zip(accel, image, tag, n_local, pos):
            _chk_arr(a_, "accel", 3, torch.float64, p_.shape[0]); _chk_arr(im_, "image", 3, torch.int32, p_.shape[0])
            if not (tg.is_cuda and tg.dtype == torch.int32 and tg.is_contiguous() and tg.shape[0] >= p_.shape[0]):
                raise ValueError("tag must be a contiguous int32 CUDA tensor with a row per particle slot")
            if not (nl.is_cuda and nl.dtype == torch.int32 and nl.numel() == 1):
                raise ValueError("n_local must be a 1-element int32 CUDA tensor")
        m = ctypes.c_int(int(lanczos_m))
        _lib.check(self._lib.pse_team_step_local(self._t, self._ptrs(pos), self._ptrs(vel), self._ptrs(accel), self._ptrs(image),
                                                 self._ptrs(force), self._ptrs(tag), self._ptrs(n_local), float(kT), float(dt),
                                                 int(timestep), float(shear_rate), 1 if integrate else 0, ctypes.byref(m)))
        return m.value

    DIAG_KINDS = {0: "migrate_ghosts", 1: "lanczos", 2: "all_to_all", 3: "halo", 4: "all_gather", 5: "ghost_rows"}

    def set_diag(self, on=True):
        """Bracket every exchange of the team's calls with events (pse_team_set_diag)."""
        _lib.check(self._lib.pse_team_set_diag(self._t, 1 if on else 0))

    def diag(self):
        """The exchanges of the last call (waits for it): dict with exchanges_per_step, exchange_us {kind: [device us, ...]},
        exchange_host_us, exchange_bytes, lanes_ms, critical_path_ms."""
        d = _lib.pse_team_diag()
        _lib.check(self._lib.pse_team_get_diag(self._t, ctypes.byref(d)))
        out = {"exchanges_per_step": d.n_exchanges, "exchange_us": {}, "exchange_host_us": {}, "exchange_bytes": {},
               "lanes_ms": {"main": d.main_lane_ms, "side": d.side_lane_ms}, "critical_path_ms": d.critical_path_ms}
        for q in range(d.n_exchanges):
            k = self.DIAG_KINDS.get(d.kind[q], str(d.kind[q]))
            out["exchange_us"].setdefault(k, []).append(round(d.device_us[q], 2))
            out["exchange_host_us"].setdefault(k, []).append(round(d.host_us[q], 2))
            out["exchange_bytes"].setdefault(k, []).append(int(d.bytes[q]))
        return out

    def redistribute_local(self, pos, vel, accel, image, force, tag, n_local):
        """After set_box has taken every member's tilt through a Lees-Edwards flip: every particle to the rank that owns it under the
        new box (pse_team_redistribute_local; arrays as for step_local, force rewritten too).  Waits for the streams twice."""
        self._check_local_arrays(pos, vel, force, accel, image, tag)
        _lib.check(self._lib.pse_team_redistribute_local(self._t, self._ptrs(pos), self._ptrs(vel), self._ptrs(accel), self._ptrs(image),
                                                         self._ptrs(force), self._ptrs(tag), self._ptrs(n_local)))

    def _check_local_arrays(self, pos, vel, force, accel, image, tag):
        if getattr(self, "_rows_own", None) is None:     # a step writes up to rows_own rows back (particles migrate in): the arrays must hold them
            self._rows_own = [e.local_layout()["rows_own"] for e in self.engines]
        for k, ts in enumerate(zip(pos, vel, force, accel, image, tag)):
            if any(t.shape[0] < self._rows_own[k] for t in ts):
                raise ValueError(f"member {k}: pos / vel / force / accel / image / tag need {self._rows_own[k]} rows (rows_own of pse_local_layout), "
                                 f"not the current particle count")

    def set_lanczos_operator(self, name):
        """The Lanczos operator ("records16" or "fp64") on every member of this process (the team calls refuse members whose modes
        differ; the ranks of a process team each set it)."""
        code = _lanczos_operator_code(name)
        for e in self.engines:
            _lib.check(self._lib.pse_set_lanczos_operator(e._h, code))

    @property
    def lanczos_operator(self):
        """The members' operator; raises if they differ."""
        ops = {e.lanczos_operator for e in self.engines}
        if len(ops) != 1:
            raise _lib.PSEError(f"team members use different Lanczos operators: {sorted(ops)}")
        return ops.pop()

    def set_lanczos_extra(self, extra):
        """Iterations an owned-particle step queues beyond its starting count (pse_team_set_lanczos_extra; -1: the default, gated
        on the device-side decision; 0: none -- for loops whose steps keep ending at their starting count).  Same on every rank."""
        _lib.check(self._lib.pse_team_set_lanczos_extra(self._t, int(extra)))

    def local_status(self):
        """Synchronises; raises if a member's step failed on the device (capacity exceeded, a particle moved too far)."""
        flags = (ctypes.c_int * len(self.engines))()
        _lib.check(self._lib.pse_team_local_status(self._t, flags))
        return list(flags)

    def step(self, pos, vel, accel, image, force, kT, dt, timestep, shear_rate=0.0, group=None, lanczos_m=2):
        n = pos[0].shape[0] if group is None else group.shape[0]
        import torch
        self._chk(group, ("pos", pos), ("vel", vel), ("force", force))
        for a_, im_ in zip(accel, image):
            _chk_arr(a_, "accel", 3, torch.float64, n); _chk_arr(im_, "image", 3, torch.int32, n)
        m = ctypes.c_int(int(lanczos_m))
        _lib.check(self._lib.pse_team_step(self._t, self._ptrs(pos), self._ptrs(vel), self._ptrs(accel),
                                           self._ptrs(image), self._ptrs(force), _ptr(group), n, float(kT), float(dt),
                                           int(timestep), float(shear_rate), ctypes.byref(m)))
        return m.value
