"""O(N^2) NumPy reference of the cluster analysis (pse_clusters_label), shared by tests/test_clusters_cpu.py (which validates it) and
tests/test_gpu_clusters.py (which compares the device to it, exactly: every output is an integer).

Over the unordered pairs i < j of pair_hist_ref.pair_distances (minimum image of oracle.pse_port, r > 0, the pairs of `excl` dropped):
a pair is a LINK when r < rlink[p], p = p(type_i, type_j) = a ntypes - a (a - 1)/2 + (b - a), a <= b; rlink[p] = 0 switches p off.
A cluster is a connected component of the links.  label = the smallest CALLER index (`ids`; default: the row) of the cluster, size
its number of members, stats = (clusters, largest, sum of s^2, N), hist[min(s, nhist) - 1] += 1 per cluster.

The device compares r^2 with rlink^2, NumPy r with rlink: they can differ only for a pair at the edge.  clearance() returns how far
the input stays from that, and every test asserts CLEAR on its input before it compares anything.
Not a test module: nothing here is collected."""
import numpy as np

import pair_hist_ref
from pair_typed_ref import pair_index

CLEAR = 1e-9


def rlink_array(rlink, ntypes):
    """npt link distances from a scalar, a dict {(a, b): r} (either key order, a missing pair off) or npt entries."""
    npt = ntypes * (ntypes + 1) // 2
    if isinstance(rlink, dict):
        out = np.zeros(npt)
        for (a, b), r in rlink.items():
            out[pair_index(min(a, b), max(a, b), ntypes)] = r
        return out
    if np.ndim(rlink) == 0:
        return np.full(npt, float(rlink))
    out = np.asarray(rlink, dtype=float)
    assert out.shape == (npt,)
    return out


def pair_types(types, i, j, ntypes):
    lo, hi = np.minimum(types[i], types[j]), np.maximum(types[i], types[j])
    return lo * ntypes - lo * (lo - 1) // 2 + (hi - lo)


def links(pos, box, types, ntypes, rlink, port, excl=None, ids=None, exempt=()):
    """((i, j) of the linked rows, clearance).  types: the types of the rows of pos, or None: one type.  exempt: row pairs left out of
    the clearance (pairs planted at the edge on purpose)."""
    n = len(pos)
    types = np.zeros(n, dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    rl = rlink_array(rlink, ntypes)
    i, j, r = pair_hist_ref.pair_distances(pos, box, port, excl, ids)
    cut = rl[pair_types(types, i, j, ntypes)]
    m = r < cut
    return (i[m], j[m]), clearance(i, j, r, cut, exempt)


def clearance(i, j, r, cut, exempt=()):
    """The least |r - rlink[p]| over all pairs of a pair type that is on; inf where there is none."""
    keep = cut > 0.0
    if len(exempt):
        ex = {(min(a, b), max(a, b)) for a, b in exempt}
        keep &= np.array([(a, b) not in ex for a, b in zip(i.tolist(), j.tolist())], dtype=bool) if len(i) else keep
    return float(np.abs(r[keep] - cut[keep]).min()) if keep.any() else np.inf


def assert_clear(clear):
    assert clear >= CLEAR, ("a pair within 1e-9 of its link distance: change the seed of the input", clear)


def components(n, i, j):
    """root[k] = the smallest row of k's component: a union-find with the smaller root on top (the ten lines the scipy test stands
    beside)."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(k) for k in range(n)], dtype=np.int64)


def outputs(root, ids=None, nhist=None):
    """(label, size, stats, hist) of the components `root` of the rows: label and size per ROW (label = the smallest caller index
    ids[...] of the row's component), stats = (clusters, largest, sum s^2, N), hist of nhist (default: N) words."""
    n = len(root)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    nhist = n if nhist is None else nhist
    _, comp = np.unique(root, return_inverse=True)
    least = np.full(comp.max() + 1, np.iinfo(np.int64).max)
    np.minimum.at(least, comp, ids)
    sizes = np.bincount(comp)
    stats = np.array([len(sizes), sizes.max(), (sizes.astype(np.int64) ** 2).sum(), n], dtype=np.int64)
    hist = np.bincount(np.minimum(sizes, nhist) - 1, minlength=nhist).astype(np.int64)
    return least[comp], sizes[comp].astype(np.int64), stats, hist


def clusters(pos, box, types, ntypes, rlink, port, excl=None, ids=None, nhist=None, exempt=()):
    """(label, size, stats, hist, clearance) of an input: the whole reference in one call."""
    (i, j), clear = links(pos, box, types, ntypes, rlink, port, excl, ids, exempt)
    return outputs(components(len(pos), i, j), ids, nhist) + (clear,)
