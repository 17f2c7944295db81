"""O(N^2) NumPy reference of the pair passes with exclusions (pse_pair_table_excl, pse_pair_repulsion_excl), shared by
tests/test_exclusion_rows_cpu.py (which validates it) and tests/test_gpu_exclusions.py (which compares the device to it), and the
NumPy restatement of the rows pse_host_exclusion_rows builds.

The pair terms are those of pair_table_ref.pair_terms and pair_virial_ref.pair_terms; a pair whose (min, max) particle index is in
the exclusion set is dropped; what is left is summed exactly as pair_table_ref.pair_observables sums, so an exclusion set that
removes nothing reproduces it bit for bit.  Exclusions are CALLER indices: with `ids` the rows of `pos` are the particles ids[0],
ids[1], ... of the caller's arrays (a group), and a pair of rows (a, b) is excluded when (ids[a], ids[b]) is in the set.
Not a test module: nothing here is collected."""
import numpy as np

import pair_table_ref
import pair_virial_ref


def pair_keys(pairs):
    """The distinct unordered pairs of an (npairs, 2) index list as sorted int64 keys min * 2^32 + max."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.unique(p.min(axis=1) * (1 << 32) + p.max(axis=1))


def kept_mask(i, j, excl, ids=None):
    """True for the row pairs (i, j) that are not in the exclusion list `excl` (caller indices; None or empty: all kept)."""
    if excl is None or len(excl) == 0:
        return np.ones(len(i), dtype=bool)
    if ids is not None:
        ids = np.asarray(ids, dtype=np.int64)
        i, j = ids[i], ids[j]
    k = np.minimum(i, j).astype(np.int64) * (1 << 32) + np.maximum(i, j)
    return ~np.isin(k, pair_keys(excl))


def sum_terms(n, i, j, d, c, u):
    """obs[8] and F[n, 3] of the pairs (i, j) with separation d, force c d on i and energy u: the sums of pair_observables."""
    obs = np.zeros(8)
    obs[0] = u.sum()
    for q, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        obs[1 + q] = (c * d[:, a] * d[:, b]).sum()
    obs[7] = float(len(c))
    F = np.zeros((n, 3))
    np.add.at(F, i, c[:, None] * d)
    np.add.at(F, j, -c[:, None] * d)
    return obs, F


def table_terms(pos, box, table, rmin, rmax, port, excl, ids=None):
    """((i, j, d, c, V) of the acting pairs, kept mask): the terms of pair_table_ref.pair_terms and which of them survive `excl`."""
    i, j, d, r, V, Fr = pair_table_ref.pair_terms(pos, box, table, rmin, rmax, port)
    return (i, j, d, Fr / r, V), kept_mask(i, j, excl, ids)


def table_observables(pos, box, table, rmin, rmax, port, excl, ids=None, keep=True):
    """(obs[8], F[n, 3], number of in-range pairs that `excl` removes).  keep=False: the sums over the EXCLUDED pairs instead."""
    (i, j, d, c, V), m = table_terms(pos, box, table, rmin, rmax, port, excl, ids)
    nex = int((~m).sum())
    if not keep:
        m = ~m
    return sum_terms(len(pos), i[m], j[m], d[m], c[m], V[m]) + (nex,)


def repulsion_terms(pos, box, k, sigma, port, excl, ids=None):
    i, j, d, c, r = pair_virial_ref.pair_terms(pos, box, k, sigma, port)
    return (i, j, d, c, 0.5 * k * (sigma - r) ** 2), kept_mask(i, j, excl, ids)


def repulsion_observables(pos, box, k, sigma, port, excl, ids=None, keep=True):
    """The same for the harmonic repulsion k/2 (sigma - r)^2."""
    (i, j, d, c, U), m = repulsion_terms(pos, box, k, sigma, port, excl, ids)
    nex = int((~m).sum())
    if not keep:
        m = ~m
    return sum_terms(len(pos), i[m], j[m], d[m], c[m], U[m]) + (nex,)


def rows_numpy(n, pairs):
    """(row_off[n + 1], entries) of pse_host_exclusion_rows: the distinct pairs in both directions, row i = the partners of i ascending."""
    key = pair_keys(pairs)
    lo, hi = key >> 32, key & 0xFFFFFFFF
    owner, partner = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    o = np.lexsort((partner, owner))
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))])
    return off, partner[o]
