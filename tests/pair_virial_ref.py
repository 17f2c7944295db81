"""O(N^2) NumPy reference of the pair observables of the harmonic repulsion (pse_pair_repulsion_virial), shared by
tests/test_pair_virial_reference.py (which validates it) and tests/test_gpu_pair_virial.py (which compares the device to it).

Over the unordered pairs i < j with minimum-image separation d = r_i - r_j (oracle.pse_port.min_image: z, then y, then x) and
0 < r < sigma:  U = sum k/2 (sigma - r)^2,  W_ab = sum c d_a d_b with c = k (sigma - r)/r  (c d is the force on i from j),
npairs = the number of such pairs.  Not a test module: nothing here is collected."""
import numpy as np

NAMES = ("U", "Wxx", "Wxy", "Wxz", "Wyy", "Wyz", "Wzz", "npairs")


def pair_terms(pos, box, k, sigma, port):
    """(i, j, d, c, r) of the pairs i < j with 0 < r < sigma."""
    pos = np.asarray(pos, dtype=float)
    i, j = np.triu_indices(len(pos), 1)
    d = port.min_image(pos[i] - pos[j], box)
    r = np.sqrt((d * d).sum(axis=1))
    m = (r < sigma) & (r > 0.0)
    i, j, d, r = i[m], j[m], d[m], r[m]
    return i, j, d, k * (sigma - r) / r, r


def pair_observables(pos, box, k, sigma, port):
    """obs[8] = U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs and the per-particle forces F[n, 3] of the same pair sum."""
    i, j, d, c, r = pair_terms(pos, box, k, sigma, port)
    obs = np.zeros(8)
    obs[0] = (0.5 * k * (sigma - r) ** 2).sum()
    for q, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        obs[1 + q] = (c * d[:, a] * d[:, b]).sum()
    obs[7] = float(len(r))
    F = np.zeros((len(pos), 3))
    np.add.at(F, i, c[:, None] * d)
    np.add.at(F, j, -c[:, None] * d)
    return obs, F


def random_points(n, box, seed):
    """n uniform random points in the primary cell of the xy-tilted box (centred on the origin)."""
    Lx, Ly, Lz, xy = box
    f = np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)) - 0.5
    pos = np.empty((n, 3))
    pos[:, 1] = f[:, 1] * Ly
    pos[:, 2] = f[:, 2] * Lz
    pos[:, 0] = f[:, 0] * Lx + xy * pos[:, 1]
    return pos
