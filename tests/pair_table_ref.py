"""O(N^2) NumPy reference of the tabulated pair potential (pse_pair_table), shared by tests/test_pair_table_reference.py (which
validates it) and tests/test_gpu_pair_table.py (which compares the device to it).

table[k] = (V_k, F_k) at the nodes r_k = rmin + k dr, dr = (rmax - rmin)/(width - 1); F is the magnitude of the radial force, positive
for a repulsion.  Over the unordered pairs i < j with minimum-image separation d = r_i - r_j (oracle.pse_port.min_image) and
rmin <= r < rmax, r > 0:
    t = (r - rmin)(width - 1)/(rmax - rmin),  k = min(floor(t), width - 2),  w = t - k,
    V(r) = V_k + w (V_k+1 - V_k),  F(r) = F_k + w (F_k+1 - F_k),
U = sum V(r),  W_ab = sum c d_a d_b with c = F(r)/r (c d is the force on i from j),  npairs = the number of such pairs.
Not a test module: nothing here is collected."""
import numpy as np

from pair_virial_ref import random_points  # noqa: F401  (the tests take their configurations from here)


def interpolate(table, rmin, rmax, r):
    """V(r), F(r) of the rule above for an array r with rmin <= r < rmax."""
    table = np.asarray(table, dtype=float)
    width = len(table)
    t = (r - rmin) * (width - 1) / (rmax - rmin)
    k = np.minimum(np.floor(t).astype(np.int64), width - 2)
    w = t - k
    lo, hi = table[k], table[k + 1]
    return lo[:, 0] + w * (hi[:, 0] - lo[:, 0]), lo[:, 1] + w * (hi[:, 1] - lo[:, 1])


def pair_terms(pos, box, table, rmin, rmax, port):
    """(i, j, d, r, V, F) of the pairs i < j with rmin <= r < rmax and r > 0."""
    pos = np.asarray(pos, dtype=float)
    i, j = np.triu_indices(len(pos), 1)
    d = port.min_image(pos[i] - pos[j], box)
    r = np.sqrt((d * d).sum(axis=1))
    m = (r >= rmin) & (r < rmax) & (r > 0.0)
    i, j, d, r = i[m], j[m], d[m], r[m]
    V, F = interpolate(table, rmin, rmax, r)
    return i, j, d, r, V, F


def pair_observables(pos, box, table, rmin, rmax, port):
    """obs[8] = U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs and the per-particle forces F[n, 3] of the same pair sum."""
    i, j, d, r, V, Fr = pair_terms(pos, box, table, rmin, rmax, port)
    c = Fr / r
    obs = np.zeros(8)
    obs[0] = V.sum()
    for q, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        obs[1 + q] = (c * d[:, a] * d[:, b]).sum()
    obs[7] = float(len(r))
    F = np.zeros((len(pos), 3))
    np.add.at(F, i, c[:, None] * d)
    np.add.at(F, j, -c[:, None] * d)
    return obs, F


def nodes(rmin, rmax, width):
    return rmin + np.arange(width) * ((rmax - rmin) / (width - 1))


def sample(V, F, rmin, rmax, width):
    """(width, 2) table of two vectorised functions at the nodes."""
    r = nodes(rmin, rmax, width)
    return np.stack([V(r), F(r)], axis=1)


def harmonic_table(k, sigma, width, rmin=0.0):
    """The harmonic repulsion k/2 (sigma - r)^2 as a table on [rmin, sigma]."""
    return sample(lambda r: 0.5 * k * (sigma - r) ** 2, lambda r: k * (sigma - r), rmin, sigma, width)


def morse_table(D, alpha, r0, rmin, rmax, width):
    """Morse D ((1 - e^{-alpha (r - r0)})^2 - 1): repulsive inside r0, attractive outside -- F changes sign at r0."""
    def V(r):
        e = np.exp(-alpha * (r - r0))
        return D * ((1.0 - e) ** 2 - 1.0)

    def F(r):
        e = np.exp(-alpha * (r - r0))
        return -2.0 * D * alpha * (1.0 - e) * e
    return sample(V, F, rmin, rmax, width)
