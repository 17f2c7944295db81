"""O(N^2) NumPy reference of the pair-distance histogram (pse_pair_hist_accumulate), shared by tests/test_pair_hist_cpu.py (which
validates it) and tests/test_gpu_pair_hist.py (which compares the device to it, exactly: the counts are integers).

Over the unordered pairs i < j with minimum-image separation d = r_i - r_j (oracle.pse_port.min_image), r = |d|, rmin <= r < rmax and
r > 0: counts[p, b] += 1 with p = p(type_i, type_j) = a ntypes - a (a - 1)/2 + (b - a), a <= b, and
b = min(floor((r - rmin) nbins/(rmax - rmin)), nbins - 1).  With `excl` (caller indices; `ids`: the caller index of every row, as in
exclusion_ref) the listed pairs are dropped.

Two correct implementations can differ only where r rounds to the other side of a bin edge or of rmin / rmax: clearance() returns how
far the input stays from that, and every test asserts CLEAR on its input before it compares anything.
Not a test module: nothing here is collected."""
import numpy as np

import exclusion_ref
from pair_typed_ref import pair_index  # noqa: F401  (the tests take the pair-type index from here)

CLEAR = 1e-9     # the least distance of t = (r - rmin) scale from an integer, and of r from rmin and rmax, over the pairs in range


def pair_distances(pos, box, port, excl=None, ids=None):
    """(i, j, r) of the pairs i < j of the rows of pos that `excl` keeps, r > 0."""
    pos = np.asarray(pos, dtype=float)
    i, j = np.triu_indices(len(pos), 1)
    d = port.min_image(pos[i] - pos[j], box)
    r = np.sqrt((d * d).sum(axis=1))
    m = exclusion_ref.kept_mask(i, j, excl, ids) & (r > 0.0)
    return i[m], j[m], r[m]


def bin_of(r, nbins, rmin, rmax):
    scale = nbins / (rmax - rmin)
    return np.minimum(((r - rmin) * scale).astype(np.int64), nbins - 1)


def histogram(pos, box, types, ntypes, nbins, rmin, rmax, port, excl=None, ids=None, exempt=()):
    """(counts (npt, nbins) int64, (edge, rmin, rmax clearance)).  types: the types of the rows of pos, or None: one type.  exempt:
    row pairs (i, j) left out of the rmax clearance (pairs planted at rmax on purpose) -- and of that one only."""
    n = len(pos)
    types = np.zeros(n, dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    i, j, r = pair_distances(pos, box, port, excl, ids)
    npt = ntypes * (ntypes + 1) // 2
    m = (r >= rmin) & (r < rmax)
    lo, hi = np.minimum(types[i], types[j])[m], np.maximum(types[i], types[j])[m]
    p = lo * ntypes - lo * (lo - 1) // 2 + (hi - lo)
    counts = np.zeros((npt, nbins), dtype=np.int64)
    np.add.at(counts, (p, bin_of(r[m], nbins, rmin, rmax)), 1)
    return counts, clearance(i, j, r, nbins, rmin, rmax, exempt)


def clearance(i, j, r, nbins, rmin, rmax, exempt=()):
    """(min |t - rint(t)| over the pairs in range, min |r - rmin|, min |r - rmax|) over all pairs; inf where there is no pair.  A
    pair exactly on rmin = 0 cannot exist (r > 0), so rmin = 0 is measured like any other value."""
    scale = nbins / (rmax - rmin)
    m = (r >= rmin) & (r < rmax)
    t = (r[m] - rmin) * scale
    edge = float(np.abs(t - np.rint(t)).min()) if len(t) else np.inf
    keep = np.ones(len(r), dtype=bool)
    if len(exempt):
        key = np.minimum(i, j).astype(np.int64) * (1 << 32) + np.maximum(i, j)
        keep = ~np.isin(key, exclusion_ref.pair_keys(np.asarray(exempt)))
    lo = float(np.abs(r - rmin).min()) if len(r) else np.inf
    hi = float(np.abs(r[keep] - rmax).min()) if keep.any() else np.inf
    return edge, lo, hi


def assert_clear(clear):
    assert min(clear) >= CLEAR, ("a pair within 1e-9 of a bin edge, rmin or rmax: change the seed of the input", clear)


def g_of_counts(counts, samples, type_counts, nbins, rmin, rmax, volume):
    """g[p, b] = counts / (samples P_p V_shell / V), written out on its own."""
    nt = len(type_counts)
    edges = rmin + np.arange(nbins + 1) * ((rmax - rmin) / nbins)
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    g = np.zeros(np.shape(counts))
    for a in range(nt):
        for b in range(a, nt):
            P = type_counts[a] * (type_counts[a] - 1) / 2 if a == b else type_counts[a] * type_counts[b]
            if P:
                g[pair_index(a, b, nt)] = np.asarray(counts)[pair_index(a, b, nt)] / (samples * P * shell / volume)
    return g


def coordination(pos, box, types, a, b, r, port):
    """The mean number of b partners within r of an a particle, counted pair by pair."""
    types = np.asarray(types)
    i, j, d = pair_distances(pos, box, port)
    m = d < r
    ti, tj = types[i][m], types[j][m]
    partners = ((ti == a) & (tj == b)).sum() + ((ti == b) & (tj == a)).sum()
    return partners / float((types == a).sum())
