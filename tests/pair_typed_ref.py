"""O(N^2) NumPy reference of the typed pair tables (pse_pair_table_typed), shared by tests/test_pair_typed_cpu.py (which validates it
by decomposition into runs of the plain reference) and tests/test_gpu_pair_typed.py (which compares the device to it), and the NumPy
restatement of pse_host_typed_table_layout.

Every particle has a type below ntypes; the pair of types a <= b has the index p(a, b) = a ntypes - a (a - 1)/2 + (b - a).  `tables`
is {(a, b): (table, rmin, rmax)}, either order of a key; a pair type without a key is off.  Each pair i < j looks up p(type_i, type_j)
and applies that pair type's table on that pair type's range with pair_table_ref.interpolate; the sums are those of
pair_table_ref.pair_observables.  With `excl` (caller indices; `ids`: the caller index of every row, as in exclusion_ref) the listed
pairs are dropped.  Not a test module: nothing here is collected."""
import numpy as np

import exclusion_ref
import pair_table_ref


def pair_index(a, b, ntypes):
    a, b = (a, b) if a <= b else (b, a)
    return a * ntypes - a * (a - 1) // 2 + (b - a)


def by_pair_type(tables, ntypes):
    """{p: (table, rmin, rmax)}; both orders of one pair are an error."""
    out = {}
    for (a, b), v in tables.items():
        p = pair_index(a, b, ntypes)
        assert p not in out, (a, b)
        out[p] = v
    return out


def typed_terms(pos, box, types, ntypes, tables, port):
    """(i, j, d, r, V, F, p) of the pairs i < j that lie in the range of their pair type, in the order of np.triu_indices."""
    pos, types = np.asarray(pos, dtype=float), np.asarray(types, dtype=np.int64)
    i, j = np.triu_indices(len(pos), 1)
    d = port.min_image(pos[i] - pos[j], box)
    r = np.sqrt((d * d).sum(axis=1))
    lo, hi = np.minimum(types[i], types[j]), np.maximum(types[i], types[j])
    p = lo * ntypes - lo * (lo - 1) // 2 + (hi - lo)
    V, F, act = np.zeros(len(r)), np.zeros(len(r)), np.zeros(len(r), dtype=bool)
    for q, (table, rmin, rmax) in by_pair_type(tables, ntypes).items():
        m = (p == q) & (r >= rmin) & (r < rmax) & (r > 0.0)
        V[m], F[m] = pair_table_ref.interpolate(table, rmin, rmax, r[m])
        act |= m
    return i[act], j[act], d[act], r[act], V[act], F[act], p[act]


def typed_observables(pos, box, types, ntypes, tables, port, excl=None, ids=None):
    """(obs[8], F[n, 3]) = U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs and the forces; `types` are the types of the rows of pos."""
    i, j, d, r, V, Fr, _ = typed_terms(pos, box, types, ntypes, tables, port)
    m = exclusion_ref.kept_mask(i, j, excl, ids)
    return exclusion_ref.sum_terms(len(pos), i[m], j[m], d[m], (Fr / r)[m], V[m])


def pairs_in_range(pos, box, types, ntypes, tables, port):
    """{p: number of acting pairs} of the pair types that are on."""
    p = typed_terms(pos, box, types, ntypes, tables, port)[6]
    return {q: int((p == q).sum()) for q in by_pair_type(tables, ntypes)}


def pairs_below_rmin(pos, box, types, ntypes, tables, port):
    """{p: number of pairs of that pair type with 0 < r < rmin}."""
    shifted = {k: (np.zeros((2, 2)), 0.0, rmin) for k, (_, rmin, _) in tables.items() if rmin > 0.0}
    if not shifted:
        return {}
    p = typed_terms(pos, box, types, ntypes, shifted, port)[6]
    return {q: int((p == q).sum()) for q in by_pair_type(shifted, ntypes)}


def arrays(tables, ntypes):
    """(width int32, rmin, rmax, entries (sum of widths, 2)) as pse_typed_table_create takes them."""
    npt = ntypes * (ntypes + 1) // 2
    width, rmin, rmax, parts = np.zeros(npt, dtype=np.int32), np.zeros(npt), np.zeros(npt), []
    for q, (table, lo, hi) in sorted(by_pair_type(tables, ntypes).items()):
        width[q], rmin[q], rmax[q] = len(table), lo, hi
        parts.append(np.asarray(table, dtype=float))
    return width, rmin, rmax, np.ascontiguousarray(np.concatenate(parts, axis=0))


def layout_numpy(width, rmin, rmax):
    """(base, scale, rmax2, total) of pse_host_typed_table_layout: offsets = the running sum of the widths; an off pair type has
    scale = rmax2 = 0."""
    width = np.asarray(width, dtype=np.int64)
    on = width > 0
    base = np.concatenate([[0], np.cumsum(width)[:-1]]).astype(np.int32)
    scale, rmax2 = np.zeros(len(width)), np.zeros(len(width))
    scale[on] = (width[on] - 1).astype(np.float64) / (np.asarray(rmax)[on] - np.asarray(rmin)[on])
    rmax2[on] = np.asarray(rmax)[on] * np.asarray(rmax)[on]
    return base, scale, rmax2, int(width.sum())
