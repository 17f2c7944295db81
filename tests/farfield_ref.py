"""Reference and inputs of the far-field tests (tests/test_farfield_ref_cpu.py, tests/test_gpu_farfield_matrix.py).

The reference is the spread (PSEv1/Mobility.cu:114-252) and the gather (PSEv1/Mobility.cu:325-477) in extended precision
(np.longdouble): the support start by the rule of support_start (pse_farbin.h; PSEv1/Mobility.cu:212-214), every weight as
prefac * exp(-expfac * r^2) directly -- no recurrence, no separable tables -- and, next to every sum, the sum of the absolute values
of its terms: the scale a kernel's rounding error is measured against node by node (a maximum norm over the grid hides the outer
layers of a support, whose weights are 1e-16 of the central one).

The inputs are planted: coordinates 1e-7 grid units either side of nodes and half-nodes on every axis (the faces included), a clump
whose support origins fill ONE 8^3 bin next to empty bins, and a uniform filler.  NOTHING sits exactly on a node or half-node: there
the support origin depends on the last bit of ((x - xy y) / Lx + 0.5) Nx, and two correct implementations take different supports
(3.7e-4 of the largest node value apart).  `clearance` measures the distance; the tests assert it.
"""
import numpy as np

LD = np.longdouble
BIN = 8                      # nodes per far-field bin and axis (pse_farbin.h)
H = 0.75                     # grid spacing of every case
PLANT = 1e-7                 # distance of a planted coordinate from its node / half-node, grid units
CLEAR = 1e-8                 # every coordinate is at least this far from a support-origin switch, grid units
# error -> the support size the parameter rule itself would choose (PSEv1/Stokes.cc:225-229 at max_strain 0.5): the Gaussian of every
# case is as wide against its support as in production
ERROR_OF_P = {4: 1e-2, 5: 3e-3, 6: 1e-3, 7: 3e-4, 8: 1e-4, 9: 4e-5, 10: 2e-5, 11: 1e-5, 12: 3e-6, 13: 1e-6, 14: 3e-7}


def matrix_grid(P):
    """The smallest grid at which every far-field path of support P exists: one axis at the threshold of the block kernels,
    2 max(8, P) (x for even P, y for odd P), one axis that is no multiple of 8 (a partial last bin and tile), Nz = 40 (even, five bins:
    a single last bin for the two-bin gather, a partial last tile for the 16-node spread block)."""
    m = 2 * max(8, P)
    return (m, 36, 40) if P % 2 == 0 else (36, m, 40)


def matrix_xy(P):
    """The tilt of the sheared cases of support P: +-0.3 ... +-0.5."""
    return (-0.5, 0.3, -0.4, 0.5, -0.3, 0.4)[P % 6]


def case_params(oracle, P, grid, xy):
    """(box, p): a box of grid * H with tilt xy and the parameter set of oracle.select_params with explicit grid and P."""
    box = (grid[0] * H, grid[1] * H, grid[2] * H, float(xy))
    return box, oracle.select_params(box, 0.5, ERROR_OF_P[P], 0.5, grid=grid, P=P, rcut=2.5)


def engine_kwargs(P, grid):
    return dict(xi=0.5, error=ERROR_OF_P[P], max_strain=0.5, grid=tuple(grid), P=P, rcut=2.5)


# ------------------------------------------------------------------------------------------ geometry, extended precision
def scaled(pos, box, grid):
    """s = f N per axis (n, 3), f the fractional coordinate in [0, 1), in extended precision from the float64 positions."""
    Lx, Ly, Lz, xy = (LD(b) for b in box)
    pos = np.asarray(pos, dtype=LD)
    f = np.empty_like(pos)
    f[:, 0] = (pos[:, 0] - xy * pos[:, 1]) / Lx + LD(0.5)
    f[:, 1] = pos[:, 1] / Ly + LD(0.5)
    f[:, 2] = pos[:, 2] / Lz + LD(0.5)
    f -= np.floor(f)
    return f * np.asarray(grid, dtype=LD)[None, :]


def clearance(pos, box, grid, P):
    """Smallest distance (grid units, over particles and axes) of s to a value at which the support origin changes: the integers, and
    for odd P the half-integers as well."""
    s = scaled(pos, box, grid)
    d = np.abs(s - np.rint(s))
    if P % 2:
        d = np.minimum(d, np.abs(d - LD(0.5)))
    return d.min(axis=1)


def support_starts(s, P):
    """First node of the support per axis, unwrapped (support_start: i0 - P/2 + 1, one less for odd P in the lower half of a cell)."""
    i0 = np.floor(s)
    start = i0 - (P // 2) + 1 - (P % 2) * ((s - i0) < LD(0.5))
    return start.astype(np.int64)


def origin_bins(pos, box, grid, P):
    """(n, 3) bin of the wrapped support origin per axis."""
    st = support_starts(scaled(pos, box, grid), P)
    return np.mod(st, np.asarray(grid)[None, :]) // BIN


def _weights(pos, box, p):
    """w (n, P, P, P) extended precision, lin (n, P, P, P) node index."""
    grid, P = p["grid"], p["P"]
    xy = LD(box[3])
    hx, hy, hz = (LD(v) for v in p["h"])
    xi, eta = LD(p["xi"]), LD(p["eta"])
    expfac = 2 * xi * xi / eta                                                 # Brownian.cu:829
    prefac = (2 * xi * xi / LD(np.pi) / eta) ** LD(1.5)                       # Brownian.cu:828
    s = scaled(pos, box, grid)
    st = support_starts(s, P)
    t = st[:, :, None] + np.arange(P)[None, None, :]                          # (n, 3, P) node per axis, unwrapped
    d = t.astype(LD) - s[:, :, None]
    ey = hy * d[:, 1]
    ex = hx * d[:, 0][:, :, None] + xy * ey[:, None, :]                       # (n, P, P): Mobility.cu:223-230
    ez = hz * d[:, 2]
    r2 = (ex * ex + (ey * ey)[:, None, :])[:, :, :, None] + (ez * ez)[:, None, None, :]
    w = prefac * np.exp(-expfac * r2)
    idx = [np.mod(t[:, a], grid[a]) for a in range(3)]
    lin = (idx[0][:, :, None, None] * grid[1] + idx[1][:, None, :, None]) * grid[2] + idx[2][:, None, None, :]
    return w, lin


def _chunks(n, P):
    step = max(1, 400000 // P ** 3)
    return [slice(a, min(n, a + step)) for a in range(0, n, step)]


def spread_ref(pos, force, box, p):
    """(sum, sum of |terms|): two (3, Nx, Ny, Nz) extended-precision arrays; a node no support reaches has |terms| == 0."""
    ng = int(np.prod(p["grid"]))
    out = np.zeros((3, ng), dtype=LD)
    mag = np.zeros((3, ng), dtype=LD)
    force = np.asarray(force, dtype=LD)
    for sl in _chunks(len(pos), p["P"]):
        w, lin = _weights(pos[sl], box, p)
        order = np.argsort(lin, axis=None, kind="stable")
        ls = lin.ravel()[order]
        first = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
        nodes = ls[first]
        for c in range(3):
            term = (w * force[sl, c][:, None, None, None]).ravel()[order]
            out[c, nodes] += np.add.reduceat(term, first)
            mag[c, nodes] += np.add.reduceat(np.abs(term), first)
    shape = (3,) + tuple(p["grid"])
    return out.reshape(shape), mag.reshape(shape)


def gather_ref(grid_values, pos, box, p):
    """(u, sum of |terms|): two (n, 3) extended-precision arrays, u = h^3 sum_nodes w u_grid (Brownian.cu:872)."""
    h3 = LD(p["h"][0]) * LD(p["h"][1]) * LD(p["h"][2])
    g = np.asarray(grid_values, dtype=LD).reshape(3, -1)
    u = np.empty((len(pos), 3), dtype=LD)
    mag = np.empty((len(pos), 3), dtype=LD)
    for sl in _chunks(len(pos), p["P"]):
        w, lin = _weights(pos[sl], box, p)
        for c in range(3):
            term = h3 * w * g[c][lin]
            u[sl, c] = term.sum(axis=(1, 2, 3))
            mag[sl, c] = np.abs(term).sum(axis=(1, 2, 3))
    return u, mag


def support_of(pos1, box, p):
    """One particle: (nodes (3, P) wrapped node per axis, w (P, P, P) its weights in extended precision)."""
    grid, P = p["grid"], p["P"]
    st = support_starts(scaled(pos1[None, :], box, grid), P)[0]
    nodes = np.stack([np.mod(st[a] + np.arange(P), grid[a]) for a in range(3)])
    w, _ = _weights(pos1[None, :], box, p)
    return nodes, w[0]


# ------------------------------------------------------------------------------------------ planted inputs
def _to_pos(s, box, grid):
    """float64 positions of scaled coordinates s (n, 3) (any real: wrapped into [0, N))."""
    Lx, Ly, Lz, xy = box
    f = np.mod(s, np.asarray(grid, dtype=float)[None, :]) / np.asarray(grid, dtype=float)[None, :]
    pos = np.empty_like(f)
    pos[:, 1] = (f[:, 1] - 0.5) * Ly
    pos[:, 2] = (f[:, 2] - 0.5) * Lz
    pos[:, 0] = (f[:, 0] - 0.5) * Lx + xy * pos[:, 1]
    return pos


def plant_targets(n):
    """Nodes of an axis with n nodes that coordinates are planted at (and, + 0.5, the half-nodes): both faces (0 and n are the faces
    f = -0.5 and +0.5), the first and last nodes, the bin and tile boundaries and their neighbours, the middle."""
    t = {0, 1, 7, 8, 9, 15, 16, n // 2, n - 9, n - 8, n - 7, n - 1, n}
    last_bin = BIN * ((n - 1) // BIN)              # first node of the (possibly partial) last bin
    t |= {last_bin - 1, last_bin, last_bin + 1}
    return sorted(x for x in t if 0 <= x <= n)


def clump_bin(grid):
    """The bin the clump fills: the last one along x and y (a partial one where the axis is no multiple of 8; the supports wrap
    round both faces), the second along z."""
    return ((grid[0] - 1) // BIN, (grid[1] - 1) // BIN, 1)


def clump_neighbours(grid):
    """The bins next to the clump's along z and y, kept empty: z neighbours are neighbours in the record order too (they share the
    two-bin workgroup of the gather and the z run of the spread)."""
    bx, by, bz = clump_bin(grid)
    nb = [(g + BIN - 1) // BIN for g in grid]
    return [(bx, by, (bz - 1) % nb[2]), (bx, by, (bz + 1) % nb[2]), (bx, (by - 1) % nb[1], bz), (bx, (by + 1) % nb[1], bz)]


def _clump_scaled(rng, P, grid, n):
    """n scaled coordinates whose support origin floor(s - 0.5 (P odd)) - P/2 + 1 lies in clump_bin(grid)."""
    cb = clump_bin(grid)
    lo = np.array([BIN * cb[a] + P // 2 - 1 + 0.5 * (P % 2) for a in range(3)])
    width = np.array([min(BIN, grid[a] - BIN * cb[a]) for a in range(3)], dtype=float)
    return lo[None, :] + rng.uniform(0.0, 1.0, (n, 3)) * width[None, :]


def make_case(P, grid, xy, seed, n_fill=600, n_clump=320, sparse=False):
    """(pos (n, 3), force (n, 3), box, parts): parts = dict of index arrays "planted", "clump", "filler".

    planted: for every axis, every target of plant_targets (and eight seeded nodes more) and its half-node, both signs: that coordinate
             at target +- PLANT, the other two uniform (sparse: inside a window three nodes wide) -- and every fifth with all three
             coordinates planted (corners of cells);
    clump:   n_clump particles whose support origins lie in clump_bin(grid);
    filler:  n_fill uniform particles (none if sparse).
    Particles other than the clump's whose origin falls into the clump's bin or one of clump_neighbours are dropped; coordinates
    closer than CLEAR to an origin switch are redrawn.  Forces: N(0, 1) per component, both signs."""
    rng = np.random.default_rng(seed)
    grid = tuple(grid)
    box = (grid[0] * H, grid[1] * H, grid[2] * H, float(xy))
    gN = np.asarray(grid, dtype=float)

    targets = [sorted(set(plant_targets(grid[a])) | set(int(v) for v in rng.integers(0, grid[a], 8))) for a in range(3)]

    def other(a):
        # sparse: the free coordinates stay in a window three nodes wide, so that the supports form three bars and most of the grid is
        # outside every support
        # (along z the window lies in the last bin, away from the clump's bins)
        w0 = grid[a] // 3 if a < 2 else BIN * ((grid[a] - 1) // BIN)
        return w0 + rng.uniform(0.0, 3.0) if sparse else rng.uniform(0.0, 1.0) * grid[a]

    def planted_value(a):
        t = targets[a][:4] if sparse else targets[a]
        return t[rng.integers(len(t))] + 0.5 * rng.integers(2) + PLANT * (1 - 2 * rng.integers(2))

    keep_out = set([clump_bin(grid)] + clump_neighbours(grid))

    def outside(s):
        b = origin_bins(_to_pos(s, box, grid), box, grid, P)
        return np.array([tuple(r) not in keep_out for r in b], dtype=bool)

    def sweep():
        rows = []
        for a in range(3):
            for t in targets[a]:
                for half in (0.0, 0.5):
                    for sign in (-1.0, 1.0):
                        for _ in range(20):          # (the free coordinates are redrawn while the origin falls into a bin kept empty)
                            s = np.array([other(b) for b in range(3)])
                            if len(rows) % 5 == 4:
                                s = np.array([planted_value(b) for b in range(3)])
                            s[a] = t + half + sign * PLANT
                            if outside(s[None, :])[0]:
                                rows.append(s)
                                break
        return np.array(rows)
    s_clump = _clump_scaled(rng, P, grid, n_clump)
    s_fill = rng.uniform(0.0, 1.0, (0 if sparse else n_fill, 3)) * gN[None, :]

    def redraw(s, fresh):
        for _ in range(100):
            bad = clearance(_to_pos(s, box, grid), box, grid, P) < 2 * CLEAR
            if not bad.any():
                return s
            s[bad] = fresh(int(bad.sum()))
        raise RuntimeError("could not clear the origin switches")
    s_clump = redraw(s_clump, lambda k: _clump_scaled(rng, P, grid, k))
    s_fill = redraw(s_fill, lambda k: rng.uniform(0.0, 1.0, (k, 3)) * gN[None, :])

    s_plant = np.empty((0, 3))
    while len(s_plant) < 280:                                # every target, both signs, on every axis: as many sweeps as it takes
        s_plant = np.concatenate([s_plant, sweep()])
    s_fill = s_fill[outside(s_fill)] if len(s_fill) else s_fill
    s_all = np.concatenate([s_plant, s_clump, s_fill])
    order = rng.permutation(len(s_all))                      # the groups are interleaved in the caller's order
    kind = np.concatenate([np.zeros(len(s_plant), int), np.ones(len(s_clump), int), np.full(len(s_fill), 2)])[order]
    pos = _to_pos(s_all[order], box, grid)
    force = rng.normal(size=pos.shape)
    parts = {name: np.flatnonzero(kind == k) for k, name in enumerate(("planted", "clump", "filler"))}
    return pos, force, box, parts


def one_bin_case(P, grid, xy, n, seed):
    """n particles whose support origins all lie in clump_bin(grid) (the small-N cases: one chunk of the spread, one pass of the gather,
    and one more)."""
    rng = np.random.default_rng(seed)
    grid = tuple(grid)
    box = (grid[0] * H, grid[1] * H, grid[2] * H, float(xy))
    while True:
        pos = _to_pos(_clump_scaled(rng, P, grid, n), box, grid)
        if clearance(pos, box, grid, P).min() >= 2 * CLEAR:
            return pos, rng.normal(size=pos.shape), box


def worst_ratio(got, ref, mag, tol):
    """max over entries of |got - ref| / (tol mag) where mag > 0 (0.0 if there is no such entry)."""
    got = np.asarray(got, dtype=LD)
    live = mag > 0
    if not live.any():
        return 0.0
    return float((np.abs(got - ref)[live] / (LD(tol) * mag[live])).max())
