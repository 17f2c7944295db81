"""Seeded configurations on cell grids of many cells, shared by tests/test_cell_grid_cases_cpu.py (which checks that every structure
planted here is really there) and tests/test_gpu_cell_grids.py (which holds the device's cell-list passes to the O(N^2) references on
them).  NumPy only; `port` is oracle.pse_port, handed in as in pair_table_ref.py.  Not a test module: nothing here is collected.

The cell rule of the engine (pse_engine.hip cells_for), restated: perpendicular widths w = (Lx / sqrt(1 + g^2), Ly, Lz) with
g = max(|xy|, max_strain); n = floor(w / r) cells per axis, fewer than three count as one; the cells are stored in blocks of bz = 6
along z once nz >= 12, else bz = nz.  A handle uses r = rcut + skin while it keeps a neighbour list across calls and r = rcut while
it does not; skin = 0.4 unless the f, g table is too large for its LDS copy (then 0: one grid).  Every box below is chosen so that
each axis falls into the same class under both radii (cell_class).

What is planted into the uniform random positions of every case whose grid has more than one cell along every axis:
  * crossers: pairs 2.05 apart whose minimum image goes through every face, edge and corner of the box -- one pair per wrap code
    of the cell walk and its mirror image; in a tilted box a y image shifts x by xy Ly -- and pairs that straddle every boundary
    between two z blocks of either grid;
  * cutoff pairs: 40 sites next to a face, alternately with a partner across that face and inside it, one partner at
    r = rcut (1 - 1e-9) and one at rcut (1 + 1e-9) each, and the same at rmax, sigma and rmin of the pair passes (pair_sites).
    The single-precision scan of the cell pass must keep the first, the fp64 test must drop the second.  The partners through the z
    face (the longest edge) are picked for the largest r^2 that scan would see (scan_r2): without the slack of its radius for the
    rounding of the coordinates (prefilter) it would drop them -- the CPU test shows that for every case with Lz >= 68.
    (Each site lies within 0.02 of a face in ONE fractional coordinate -- the axes in turn, both signs -- and anywhere in the other
    two.  With all three at +-0.5 the forty sites are one periodic cluster at the corner of the box, with their partners ~170
    neighbours per row: the rows overflow the kept neighbour list, which is then never reused, and the pass that reads it could not
    be tested on these cases.  kept_list_capacity() restates that capacity; the CPU test holds every row of every case below it.)
build() asserts with port.min_image that every planted r lies on its side of its cutoff by 5e-10 .. 2e-9 relative and that no other
pair of the case comes within 1e-7 relative of any cutoff the case uses; the seeds are the first for which that holds and every
row fits the kept list with eight entries to spare."""
import functools
import itertools
import math

import numpy as np

SKIN = 0.4
BZ = 6
RMIN, RMAX, SIGMA = 0.7, 3.0, 2.0           # the pair passes: Morse table on [0.7, 3), harmonic repulsion below 2
EPS = 1e-9                                  # relative distance of a planted pair from its cutoff
CLEAR = 1e-7                                # no other pair comes this close (relative)
N_SITES = 40

#         name               box (Lx, Ly, Lz, xy)            xi    n     seed
SPECS = {
    "blocked_padded":   ((40.0, 23.0, 75.0, 0.0),    0.5,  1665, 1),    # n = 64 * 26 + 1: the last wave has one lane
    "blocked_exact":    ((40.0, 23.0, 68.1, 0.0),    0.5,  1536, 1),    # n = 256 * 6: every workgroup is full
    "blocked_tilt_pos": ((40.0, 23.0, 75.0, 0.5),    0.5,  1647, 1),
    "blocked_tilt_neg": ((40.0, 23.0, 75.0, -0.5),   0.5,  1647, 2),
    "one_cell_x":       ((17.0, 30.0, 75.0, 0.3),    0.5,  913,  1),
    "three_cubed":      ((19.5, 17.5, 17.5, 0.2),    0.5,  285,  1),    # phi = 0.2
    "global_table":     ((40.0, 36.0, 135.0, 0.0),   0.24, 1500, 1),
}
NAMES = tuple(SPECS)
ERROR, MAX_STRAIN = 1e-3, 0.5


def cutoff(xi, error=ERROR):
    return math.sqrt(-math.log(error)) / xi


def table_in_lds(rcut):
    """pse_kernels.hip mreal_table_in_lds: intervals of 1/8, 20 coefficients each, padded to 21 doubles, at most 14 KB."""
    return (math.ceil(rcut * 8) + 1) * 21 * 8 <= 14 * 1024


def widths(box, max_strain=MAX_STRAIN):
    g = max(abs(box[3]), max_strain)
    return (box[0] / math.sqrt(1.0 + g * g), box[1], box[2])


def skin_of(box, rcut, max_strain=MAX_STRAIN):
    if not table_in_lds(rcut) or rcut + SKIN > 0.5 * min(widths(box, max_strain)):
        return 0.0
    return SKIN


def cells(box, r, max_strain=MAX_STRAIN):
    """(nx, ny, nz, bz) of cells at least r wide."""
    n = [int(math.floor(w / r)) for w in widths(box, max_strain)]
    n = [1 if c < 3 else c for c in n]
    return (n[0], n[1], n[2], BZ if n[2] >= 2 * BZ else n[2])


def pair_sites(n):
    """How many of the sites also carry partners at rmax, sigma and rmin: every second one -- with six more close partners at all
    forty, rows next to them no longer fit the kept neighbour list (kept_list_capacity) -- and ten in three_cubed (285 particles)."""
    return N_SITES // 2 if n >= 1000 else 10


def kept_list_capacity(n, box, rcut, skin):
    """Entries per row of the neighbour list kept across calls (pse_engine.hip pse_create): twice the mean count within rcut + skin at the
    density of n particles, + 32, at most 512, rounded up to whole groups of four."""
    nbar = n / (box[0] * box[1] * box[2]) * 4.18879020478639 * (rcut + skin) ** 3
    return (max(16, min(int(math.ceil(2.0 * nbar + 32.0)), 512)) + 3) & ~3


def cell_class(n):
    if n == 1:
        return "1"
    if n == 3:
        return "3"
    if n < 12:
        return "4-11"
    return "12+, multiple of 6" if n % BZ == 0 else "12+, last block padded"


def block_boundaries(grid):
    """The pairs (cz, cz') of z cells next to one another across the end of a block, the wrap nz - 1 | 0 included."""
    nz, bz = grid[2], grid[3]
    if nz == 1:
        return []
    out = [(k - 1, k) for k in range(bz, nz, bz)]
    return out + [(nz - 1, 0)]


def fractional(pos, box):
    """f in [-0.5, 0.5) for positions inside the box."""
    Lx, Ly, Lz, xy = box
    return np.stack([(pos[:, 0] - xy * pos[:, 1]) / Lx, pos[:, 1] / Ly, pos[:, 2] / Lz], axis=1)


def from_fractional(f, box):
    Lx, Ly, Lz, xy = box
    f = np.atleast_2d(f)
    y = f[:, 1] * Ly
    return np.stack([f[:, 0] * Lx + xy * y, y, f[:, 2] * Lz], axis=1)


def wrap(pos, box):
    """Into the box centred on the origin: z, then y (a y image shifts x by xy Ly), then x."""
    Lx, Ly, Lz, xy = box
    pos = np.array(pos, dtype=float, copy=True)
    n = np.floor(pos[:, 2] / Lz + 0.5); pos[:, 2] -= n * Lz
    n = np.floor(pos[:, 1] / Ly + 0.5); pos[:, 1] -= n * Ly; pos[:, 0] -= n * xy * Ly
    n = np.floor((pos[:, 0] - xy * pos[:, 1]) / Lx + 0.5); pos[:, 0] -= n * Lx
    return pos


def cell_coords(pos, box, grid):
    f = fractional(pos, box) + 0.5
    f -= np.floor(f)
    n = np.array(grid[:3])
    return np.minimum((f * n).astype(np.int64), n - 1)


def walk_codes(ci, cj, grid):
    """How the cell walk of a particle in cell ci reaches cell cj: per axis the offset o in {-1, 0, 1} and the wrap w in {-1, 0, 1} of
    the neighbour cell ci + o (arrays (m, 3) each); o = 2 marks a cell that is no neighbour."""
    n = np.array(grid[:3])
    d = np.mod(cj - ci, n)
    o = np.where(d == 0, 0, np.where(d == 1, 1, np.where(d == n - 1, -1, 2)))
    a = ci + o
    w = np.where(a < 0, -1, np.where(a >= n, 1, 0))
    return o, np.where(o == 2, 0, w)


def pair_distances(pos, box, port):
    """(i, j, d, r) of all pairs i < j, minimum image."""
    i, j = np.triu_indices(len(pos), 1)
    d = port.min_image(pos[i] - pos[j], box)
    return i, j, d, np.sqrt((d * d).sum(axis=1))


def scan_r2(a, b, box, grid):
    """r^2 as the single-precision scan of the cell pass (k_mreal_cells) sees the particles b from the particles a (arrays (m, 3)) on
    the cell grid `grid`: a's coordinates minus the image shift of b's cell, rounded to float; b's coordinates rounded to float;
    differences, squares and sum in float."""
    f32 = np.float32
    Lx, Ly, Lz, xy = box
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    _, w = walk_codes(cell_coords(a, box, grid), cell_coords(b, box, grid), grid)
    shift = np.stack([w[:, 0] * Lx + w[:, 1] * xy * Ly, w[:, 1] * Ly, w[:, 2] * Lz], axis=1)
    d = (a - shift).astype(f32) - b.astype(f32)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float64)


def prefilter(box, r, slack=True):
    """The squared radius of that scan (pse_kernels.hip launch_mreal, rcut2_pre) for the radius r; slack=False: without the term for
    the rounding of the coordinates."""
    cmax = 1.5 * (box[0] + abs(box[3]) * box[1] + box[1] + box[2])
    rpre = r + (16.0 * cmax * 5.97e-8 if slack else 0.0)
    return float(np.float32(rpre * rpre * (1.0 + 1e-6)))


def _adverse_pair(rng, site, r, box, grid):
    """`site` moved along z by up to 0.01 and a partner at distance r through the z face next to it, nearly along z: of 4000 such
    pairs the one with the largest r^2 in the eyes of the single-precision scan (z is the longest edge: its coordinates round the most)."""
    sites = np.tile(site, (4000, 1))
    sites[:, 2] += rng.uniform(-0.01, 0.01, 4000)
    u = rng.normal(size=(4000, 3)) * np.array([0.2, 0.2, 0.0])
    u[:, 2] = 1.0 if site[2] > 0 else -1.0
    u /= np.linalg.norm(u, axis=1)[:, None]
    cand = wrap(sites + r * u, box)
    k = int(np.maximum(scan_r2(sites, cand, box, grid), scan_r2(cand, sites, box, grid)).argmax())
    return sites[k], sites[k] + r * u[k]


def _unit(rng):
    u = rng.normal(size=3)
    return u / np.linalg.norm(u)


def _leaves_box(p, box):
    f = fractional(p[None], box)[0]
    return bool(np.any(f < -0.5) or np.any(f >= 0.5))


def _partner(rng, site, r, box, straddle):
    """site + r u for a random direction u, through a face of the box (straddle) or not."""
    for _ in range(400):
        p = site + r * _unit(rng)
        if _leaves_box(p, box) == straddle:
            return p
    return p


def make(name, seed, port):
    """(case, cutoff_problems(case)) of the geometry `name` drawn with `seed`."""
    box, xi, n, _ = SPECS[name]
    Lx, Ly, Lz, xy = box
    rcut = cutoff(xi)
    skin = skin_of(box, rcut)
    wide, narrow = cells(box, rcut + skin), cells(box, rcut)
    pair = xi == 0.5                                         # the pair passes run on these
    cutoffs = {"rcut": rcut}
    if skin > 0.0:
        cutoffs["rcut+skin"] = rcut + skin
    if pair:
        cutoffs.update(rmax=RMAX, sigma=SIGMA, rmin=RMIN)
    rng = np.random.default_rng(seed)
    planted, crossers, rows = [], [], []                   # planted: (i, j, cutoff name, inside, straddle); crossers: (i, j, label)

    def add(p):
        rows.append(np.asarray(p, dtype=float))
        return len(rows) - 1

    if min(wide[:3]) > 1:
        L = (Lx, Ly, Lz)
        for w in itertools.product((-1, 0, 1), repeat=3):    # through every face, edge and corner: one pair per wrap code and its mirror
            if w <= (0, 0, 0):
                continue
            f = rng.uniform(-0.4, 0.4, 3)
            for a in range(3):
                if w[a]:
                    f[a] = w[a] * (0.5 - 0.3 / L[a])
            A = from_fractional(f, box)[0]
            B = A + 2.05 * np.array(w) / math.sqrt(sum(t * t for t in w))
            crossers.append((add(A), add(B), ("w",) + w))
        for g in {wide, narrow}:                             # across the ends of the z blocks inside the box
            for lo, hi in block_boundaries(g)[:-1]:
                f = rng.uniform(-0.5, 0.5, 3)
                A = from_fractional(f, box)[0]
                A[2] = -0.5 * Lz + hi * Lz / g[2] - 1.0
                B = A + np.array([0.0, 0.0, 2.05])
                crossers.append((add(A), add(B), ("cz", lo, hi, g[2])))
        for k in range(N_SITES):
            a, sign = k % 3, 1.0 if (k // 3) % 2 else -1.0
            f = rng.uniform(-0.5, 0.5, 3)
            f[a] = sign * (0.5 - 0.02 * rng.uniform(0.05, 1.0))
            site = from_fractional(f, box)[0]
            straddle = k % 2 == 0
            adverse = None
            if a == 2 and straddle:
                site, adverse = _adverse_pair(rng, site, rcut * (1.0 - EPS), box, narrow)
            s = add(site)
            for cname in (("rcut", "rmax", "sigma", "rmin") if pair and k < pair_sites(n) else ("rcut",)):
                rc = cutoffs[cname]
                inner = adverse if cname == "rcut" and adverse is not None else _partner(rng, site, rc * (1.0 - EPS), box, straddle)
                planted.append((s, add(inner), cname, True, straddle))
                planted.append((s, add(_partner(rng, site, rc * (1.0 + EPS), box, not straddle)), cname, False, not straddle))
    n_planted = len(rows)
    assert n_planted < n
    pos = np.concatenate([from_fractional(rng.uniform(-0.5, 0.5, (n - n_planted, 3)), box), np.array(rows).reshape(-1, 3)])
    planted = [(i + n - n_planted, j + n - n_planted, c, ins, st) for i, j, c, ins, st in planted]
    crossers = [(i + n - n_planted, j + n - n_planted, lab) for i, j, lab in crossers]
    order = rng.permutation(n)                               # the planted particles anywhere among the rows
    inv = np.empty(n, dtype=np.int64); inv[order] = np.arange(n)
    pos = wrap(pos[order], box)
    planted = [(int(inv[i]), int(inv[j]), c, ins, st) for i, j, c, ins, st in planted]
    crossers = [(int(inv[i]), int(inv[j]), lab) for i, j, lab in crossers]
    force = rng.normal(size=(n, 3))
    psi = rng.normal(size=(n, 3))
    case = dict(name=name, box=box, xi=xi, error=ERROR, max_strain=MAX_STRAIN, pos=pos, force=force, psi=psi, n=n, seed=seed, rcut=rcut,
                skin=skin, cells_wide=wide, cells_narrow=narrow, cutoffs=cutoffs, planted=tuple(planted), crossers=tuple(crossers), pair=pair)
    for a in (pos, force, psi):
        a.setflags(write=False)
    return case, cutoff_problems(case, port)


def cutoff_problems(case, port):
    """The conditions on the inputs, as a list of what is wrong: every planted pair on its side of its cutoff by 5e-10 .. 2e-9
    relative (by the reference's own minimum image), and no other pair within 1e-7 relative of any cutoff of the case."""
    pos, box = case["pos"], case["box"]
    i, j, _, r = pair_distances(pos, box, port)
    n = case["n"]
    key = {(min(a, b), max(a, b)): (c, ins) for a, b, c, ins, _ in case["planted"]}
    out = []
    seen = set()
    for cname, rc in case["cutoffs"].items():
        for q in np.nonzero(np.abs(r / rc - 1.0) < CLEAR)[0]:
            k = (int(i[q]), int(j[q]))
            if k not in key or key[k][0] != cname:
                out.append(("stray pair at a cutoff", cname, k, float(r[q] / rc - 1.0)))
                continue
            m = r[q] / rc - 1.0
            inside = key[k][1]
            if not (5e-10 <= (-m if inside else m) <= 2e-9):
                out.append(("planted pair off its margin", cname, k, float(m)))
            seen.add(k)
    for k in key:
        if k not in seen:
            out.append(("planted pair not at its cutoff", key[k][0], k))
    assert len(r) == n * (n - 1) // 2
    return out


def build(name, port):
    """The case `name`: dict(name, box, xi, error, max_strain, pos, force, psi, n, seed, rcut, skin, cells_wide, cells_narrow (each
    (nx, ny, nz, bz)), cutoffs {name: radius}, planted ((i, j, cutoff name, inside, straddles a face), ...),
    crossers ((i, j, ("w", wx, wy, wz) | ("cz", lo, hi, nz)), ...), pair (the pair passes run on it)).  Built once; the arrays are read-only."""
    return _build(name, port)


@functools.lru_cache(maxsize=None)
def _build(name, port):
    case, problems = make(name, SPECS[name][3], port)
    assert not problems, (name, case["seed"], problems[:5])
    return case
