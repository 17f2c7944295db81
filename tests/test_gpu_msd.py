"""GPU tests of the displacement moments (pse_msd_create, pse_msd_store, pse_msd_accumulate, pse_msd_displacement) and of analyze.MSD
on top of them, against the references of tests/msd_ref.py (validated on the CPU by tests/test_msd_cpu.py).

1. Exact cases.  Dyadic inputs -- coordinates, box lengths and strain Ly multiples of 2^-4, every displacement component below 32,
   N <= 4096 (asserted here, on the CPU) -- make every product and every sum exact in fp64, whatever the order: `sums` must equal the
   integer reference bit for bit.  N around the wave (64) and the workgroup (256), one to 64 pairs, one to eight types, a type without
   members, no types, a group, n < n_max, N = n_max with more pairs than the object has slots, a slab rank.
2. General position.  Random doubles against the extended-precision reference, within the bound of `bound()` below.
3. A trajectory through wraps and a Lees-Edwards flip at the engine level, exact against the recurrence of the unwrapped trajectory.
4. analyze.MSD through System.run under a steady shear that flips: with hydrodynamics against the run's own samples, and with
   prescribed velocities against the same run without the shear -- yy, zz, yz equal bit for bit.
5. Store + accumulate captured into a graph replay the eager bits.
6. Refusals on the device leave `sums` untouched.

The bound of 2, from the kernels' order of operations, with u = 2^-53: x_u = fma(iy, sLy, fma(ix, Lx, x)) has two roundings, y_u and
z_u one, each of at most u R, R the largest magnitude of an unwrapped coordinate or of the intermediate x + ix Lx on either side; the
subtraction adds u |d| <= u R (D <= R is asserted): one displacement component carries at most e = 5 u R.  A moment of order q of
one particle is then off by at most c_q e (D + e)^(q - 1), D the largest |d|: c_1 = 1, c_2 = 2 (|d_a d_b| moves by (|d_a| + |d_b|) e
+ e^2), c_4 = 7 (r^2 moves by 2 sqrt(3) D e + 3 e^2, its square by twice r^2 times that: 4 sqrt(3) < 7).  Forming the moment rounds
f_q times relative to its size: f_1 = 0, f_2 = 1 (one product), f_4 = 7 (three products, two sums -- 3 u on r^2 --, twice that and
one for the square).  The sums: three additions over the four particles of a lane, six levels of the tree over the wave (nine in
all, with nblk = ceil(N / 256) rows of the workspace, one per wave), then in k_msd_finish a strip
of ceil(nblk / nstrip) rows in four interleaved partial sums (at most ceil(k / 4) + 3 additions and two to join them), nstrip
additions over the strips and one into `sums`: s = 9 + ceil(k / 4) + 5 + nstrip + 1 + f_q with nstrip = 1024 / (10 ntypes), k =
ceil(nblk / nstrip), nblk = ceil(N / 256).  Per type a and moment c:  bound = N_a (c_q e (D + e)^(q - 1) + g D^q), g = s u /
(1 - s u), which has the higher orders of u in it.  The test asserts that s stays below the cap of a sequential sum, N_a + q + 2.
Worst error seen: 0.26 % of the bound (docs/HISTORY.md)."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import to4
import msd_ref as mr

pytestmark = pytest.mark.gpu

NMAX = 5000
BOX = (16.0, 12.0, 20.0, 0.0)          # dyadic lengths; 12 >= twice the real-space cutoff
INVALID = -1
U = 2.0 ** -53
ORDER = np.array([1, 1, 1, 2, 2, 2, 2, 2, 2, 4])
CQ = {1: 1.0, 2: 2.0, 4: 7.0}
FQ = {1: 0, 2: 1, 4: 7}


@functools.lru_cache(maxsize=None)
def engine():
    import pse_amd
    return pse_amd.Engine(NMAX, BOX, xi=0.5, error=1e-3)


def dev_image(image):
    import torch
    return torch.tensor(np.ascontiguousarray(image, dtype=np.int32), device="cuda")


def dev_group(members):
    import torch
    return None if members is None else torch.tensor(np.asarray(members), dtype=torch.int32, device="cuda")


def lattice_shift(image, lengths, sLy):
    im = np.asarray(image, dtype=np.float64)
    return np.stack([im[:, 0] * lengths[0] + im[:, 1] * sLy, im[:, 1] * lengths[1], im[:, 2] * lengths[2]], axis=1)


STRAINS = (0.0, 0.3125, -0.4375, 1.75, -2.25)     # times Ly = 12: 0, 3.75, -5.25, 21, -27 -- multiples of 2^-4


def dyadic_case(n, nslots, seed, lengths=BOX[:3]):
    """now = (pos, image, strain) and nslots origins (pos_k, image_k, strain_k), all dyadic, with displacements below 21 per component:
    images of both signs in all three axes, an origin's images within one of the current ones, its strain any of STRAINS."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(-128, 128, (n, 3)) / 16.0
    image = rng.integers(-3, 4, (n, 3))
    strain = STRAINS[seed % len(STRAINS)]
    ru = pos + lattice_shift(image, lengths, strain * lengths[1])
    slots = []
    for k in range(nslots):
        d = rng.integers(-20 * 16, 20 * 16 + 1, (n, 3)) / 16.0
        if k == 0:
            d[: n // 2] = 0.0                                   # particles that did not move
        image_k = image - rng.integers(-1, 2, (n, 3))
        strain_k = STRAINS[(seed + 1 + k) % len(STRAINS)]
        pos_k = (ru - d) - lattice_shift(image_k, lengths, strain_k * lengths[1])
        slots.append((pos_k, image_k, strain_k))
    return (pos, image, strain), slots


def exact_reference(now, slots, lengths, types, ntypes, members=None):
    """[(ntypes, 10)] per slot, exact; asserts the conditions under which fp64 is exact in any order."""
    pos, image, strain = now
    n = pos.shape[0] if members is None else len(members)
    assert n <= 4096
    now_u = mr.unwrap_exact(pos, image, lengths, strain * lengths[1])        # (asserts the multiples of 2^-4)
    out = []
    for pos_k, image_k, strain_k in slots:
        out.append(mr.moments_exact(now_u, mr.unwrap_exact(pos_k, image_k, lengths, strain_k * lengths[1]), types, ntypes, members))
    return out                                                                # (moments_exact asserts |d| < 32)


def store_all(eng, origins, slots, group=None, order=None):
    for k in (range(len(slots)) if order is None else order):
        pos_k, image_k, strain_k = slots[k]
        eng.msd_store(to4(pos_k), dev_image(image_k), origins, k, strain_k, group=group)


def planted(shape):
    import torch
    v = ((np.arange(int(np.prod(shape))) % 7) - 3.0) * 0.25
    return torch.tensor(v.reshape(shape), dtype=torch.float64, device="cuda"), v.reshape(shape)


def types_for(n, ntypes, seed, kind):
    """kind 'none': no types; 'gap': a type without members; 'all'."""
    if kind == "none":
        return None
    t = np.random.default_rng(seed).integers(0, ntypes, n)
    if kind == "gap" and ntypes > 1:
        t[t == ntypes // 2] = 0
    return t


# -- 1. exact cases ------------------------------------------------------------------------------------------------------------------

EXACT = [(1, 1, 1, "all"), (63, 3, 2, "gap"), (64, 8, 7, "all"), (65, 1, 64, "none"), (255, 3, 7, "all"), (256, 8, 2, "gap"),
         (257, 3, 64, "gap"), (1000, 8, 64, "gap"), (4096, 3, 7, "all"), (4096, 1, 64, "none"), (4096, 8, 1, "all")]


@pytest.mark.parametrize("n,ntypes,npairs,kind", EXACT)
def test_exact_sums_on_dyadic_inputs(n, ntypes, npairs, kind):
    eng = engine()
    seed = n + 10 * ntypes + npairs
    now, slots = dyadic_case(n, npairs, seed)
    types = types_for(n, ntypes, seed, kind)
    want = exact_reference(now, slots, BOX[:3], types, ntypes)
    assert n < NMAX and (kind != "gap" or ntypes == 1 or not np.any(types == ntypes // 2))
    origins = eng.msd_origins(types, ntypes, npairs, n=None if types is not None else n)
    store_all(eng, origins, slots, order=list(reversed(range(npairs))))
    nrows = npairs + 3
    rows = np.random.default_rng(seed).permutation(nrows)[:npairs]            # permuted against the slots, three rows untouched
    sums, before = planted((nrows, ntypes, 10))
    pos, image, strain = now
    assert eng.msd_accumulate(to4(pos), dev_image(image), origins, strain, list(range(npairs)), rows.tolist(), sums) is sums
    expect = before.copy()
    for k in range(npairs):
        expect[rows[k]] += want[k]
    got = sums.cpu().numpy()
    assert np.array_equal(got, expect), np.argwhere(got != expect)[:5]
    if kind == "gap" and ntypes > 1:                                          # a type without members adds exactly +0.0
        assert np.array_equal(got[:, ntypes // 2], before[:, ntypes // 2])
    # a second sample into the same tensor, other pairs: ADDED again
    eng.msd_accumulate(to4(pos), dev_image(image), origins, strain, [npairs - 1], [int(rows[0])], sums)
    expect[rows[0]] += want[npairs - 1]
    assert np.array_equal(sums.cpu().numpy(), expect)
    origins.close()
    with pytest.raises(ValueError, match="closed"):
        eng.msd_accumulate(to4(pos), dev_image(image), origins, strain, [0], [0], sums)


def test_more_pairs_than_slots_at_n_max():
    """A call may list a slot for several rows, so npairs is not bounded by norigins: the workspace of the partial sums is sized for
    64 pairs whatever the object holds.  N = n_max = 4096 (every row of the workspace is in use), two slots, 64 pairs."""
    import pse_amd
    n, ntypes = 4096, 3
    eng = pse_amd.Engine(n, BOX, xi=0.5, error=1e-3)
    now, slots = dyadic_case(n, 2, 91)
    types = types_for(n, ntypes, 92, "all")
    want = exact_reference(now, slots, BOX[:3], types, ntypes)
    pos, image, strain = now
    for norigins in (1, 2):
        origins = eng.msd_origins(types, ntypes, norigins)
        store_all(eng, origins, slots[:norigins])
        which = [q % norigins for q in range(64)]
        sums, before = planted((64, ntypes, 10))
        eng.msd_accumulate(to4(pos), dev_image(image), origins, strain, which, list(reversed(range(64))), sums)
        got = sums.cpu().numpy()
        for q in range(64):
            assert np.array_equal(got[63 - q], before[63 - q] + want[which[q]]), (norigins, q)
        origins.close()
    eng.close()


def test_exact_on_a_group_whose_complement_is_nan_and_displacement_rows():
    import torch
    eng = engine()
    n, ntypes, nslots = 1000, 3, 2
    now, slots = dyadic_case(n, nslots, 77)
    types = types_for(n, ntypes, 77, "all")
    members = np.sort(np.random.default_rng(78).permutation(n)[:600])
    outside = np.setdiff1d(np.arange(n), members)
    want = exact_reference(now, slots, BOX[:3], types, ntypes, members)
    origins = eng.msd_origins(types, ntypes, nslots)
    group = dev_group(members)
    nan_pos = np.full((n, 3), np.nan)
    for k in range(nslots):                                                    # NaN in every row of the planes, then the members' rows
        eng.msd_store(to4(nan_pos), dev_image(slots[k][1]), origins, k, 0.0)
    holed = [(np.where(np.isin(np.arange(n), members)[:, None], p, np.nan), im, st) for p, im, st in slots]
    store_all(eng, origins, holed, group=group)
    pos, image, strain = now
    pos_holed = pos.copy()
    pos_holed[outside] = np.nan
    sums, before = planted((2, ntypes, 10))
    eng.msd_accumulate(to4(pos_holed), dev_image(image), origins, strain, [0, 1], [1, 0], sums, group=group)
    got = sums.cpu().numpy()
    assert np.array_equal(got[1], before[1] + want[0]) and np.array_equal(got[0], before[0] + want[1])
    # a permuted group gives the same bits on exact data
    perm = np.random.default_rng(79).permutation(members)
    sums2, _ = planted((2, ntypes, 10))
    eng.msd_accumulate(to4(pos_holed), dev_image(image), origins, strain, [0, 1], [1, 0], sums2, group=dev_group(perm))
    assert np.array_equal(sums2.cpu().numpy(), got)
    # the displacement rows: exact, and the rows outside the group keep what was there
    now_u = mr.unwrap_exact(pos, image, BOX[:3], strain * BOX[1])
    for k in range(nslots):
        d = (now_u - mr.unwrap_exact(slots[k][0], slots[k][1], BOX[:3], slots[k][2] * BOX[1])) / 16.0
        out = torch.full((n, 4), -5.0, dtype=torch.float64, device="cuda")
        assert eng.msd_displacement(to4(pos_holed), dev_image(image), origins, k, strain, out=out, group=group) is out
        o = out.cpu().numpy()
        assert np.array_equal(o[members, :3], d[members]) and np.array_equal(o[members, 3], (d[members] ** 2).sum(axis=1))
        assert np.all(o[outside] == -5.0)
    full = eng.msd_displacement(to4(pos), dev_image(image), origins, 0, strain, group=group).cpu().numpy()
    assert not np.any(full[outside]) and full.shape == (n, 4)
    origins.close()


# -- 2. general position --------------------------------------------------------------------------------------------------------------

def bound(n, counts, R, D):
    """(ntypes, 10): the bound of the module docstring."""
    ntypes = len(counts)
    assert D <= R
    e = 5.0 * U * R
    nblk, nstrip = -(-n // 256), 1024 // (10 * ntypes)
    k = -(-nblk // nstrip)
    out = np.zeros((ntypes, 10))
    for c, q in enumerate(ORDER):
        s = 9 + -(-k // 4) + 5 + nstrip + 1 + FQ[q]
        for a, na in enumerate(counts):
            assert na == 0 or s <= na + q + 2, "the bound may not exceed that of a sequential sum"
            out[a, c] = na * (CQ[q] * e * (D + e) ** (q - 1) + s * U / (1.0 - s * U) * D ** q)
    return out


def general_case(n, nslots, seed):
    rng = np.random.default_rng(seed)
    L = np.array(BOX[:3])
    strain = 1.3
    pos = rng.uniform(-0.5, 0.5, (n, 3)) * L
    image = rng.integers(-3, 4, (n, 3))
    slots = []
    for k in range(nslots):
        strain_k = strain - 0.17 * (k + 1)
        image_k = image - rng.integers(-1, 2, (n, 3))
        d = rng.normal(size=(n, 3)) * (0.5 + k)
        pos_k = pos + lattice_shift(image, L, strain * L[1]) - d - lattice_shift(image_k, L, strain_k * L[1])
        slots.append((pos_k, image_k, strain_k))
    return (pos, image, strain), slots


def extended_reference(now, slots, types, ntypes):
    """([(ntypes, 10) longdouble], counts, R, D) of the double inputs the device sees (sLy = strain Ly formed in double)."""
    L = BOX[:3]
    pos, image, strain = now
    now_u = mr.unwrap_ld(pos, image, L, strain * L[1])
    R = float(max(np.abs(now_u).max(), np.abs(pos[:, 0] + image[:, 0] * L[0]).max()))
    D, out, counts = 0.0, [], None
    for pos_k, image_k, strain_k in slots:
        u_k = mr.unwrap_ld(pos_k, image_k, L, strain_k * L[1])
        R = max(R, float(np.abs(u_k).max()), float(np.abs(pos_k[:, 0] + image_k[:, 0] * L[0]).max()))
        D = max(D, float(np.sqrt(((now_u - u_k) ** 2).sum(axis=1).max())))
        m, counts = mr.moments_ld(now_u, u_k, types, ntypes)
        out.append(m)
    return out, counts, R, D


@pytest.mark.parametrize("n", [1000, 4096])
def test_general_position_within_the_bound_reproducible_and_under_a_permutation(n):
    mr.need_extended_precision()
    eng = engine()
    ntypes, nslots = 3, 5
    now, slots = general_case(n, nslots, 5 + n)
    types = types_for(n, ntypes, 6 + n, "all")
    want, counts, R, D = extended_reference(now, slots, types, ntypes)
    tol = bound(n, counts, R, D)

    def run(order):
        import torch
        p = lambda a: np.ascontiguousarray(a[order])                          # noqa: E731
        origins = eng.msd_origins(types[order], ntypes, nslots)
        store_all(eng, origins, [(p(pk), p(ik), sk) for pk, ik, sk in slots])
        out = []
        for _ in range(2):
            sums = torch.zeros((nslots, ntypes, 10), dtype=torch.float64, device="cuda")
            eng.msd_accumulate(to4(p(now[0])), dev_image(p(now[1])), origins, now[2], list(range(nslots)), list(range(nslots)), sums)
            out.append(sums.cpu().numpy())
        origins.close()
        assert np.array_equal(out[0], out[1]), "equal inputs, equal bits"
        return out[0]

    worst = 0.0
    for what, order in (("caller order", np.arange(n)), ("permuted", np.random.default_rng(9).permutation(n))):
        got = run(order)
        ratio = max(float((np.abs(got[k].astype(np.longdouble) - want[k]) / tol).max()) for k in range(nslots))
        print(f"N = {n}, {what}: R = {R:.3g}, D = {D:.3g}, worst error / bound = {ratio:.4f}")
        worst = max(worst, ratio)
    assert np.all(np.isfinite(got)) and worst <= 1.0, worst


# -- 3. a trajectory through wraps and a flip, at the engine level -----------------------------------------------------------------------

def test_displacement_follows_the_unwrapped_trajectory_through_wraps_and_a_flip():
    """Engine.integrate with a shear rate, alternating with set_box and the re-wrap of System._set_tilt, on the dyadic schedule that
    tests/test_msd_cpu.py checks on the CPU first (every y image gained before the flip: see the limit recorded there): the
    displacement against slot 0 equals the recurrence x_u += (v_x + rate y_u) dt, y_u += v_y dt, z_u += v_z dt EXACTLY after every
    step, and so do the summed moments."""
    import torch
    import pse_amd
    from pse_amd import analyze
    n, steps, L, dt, rate = 64, 12, mr.SHEAR_L, mr.SHEAR_DT, mr.SHEAR_RATE
    pos0, vel = mr.shear_case(n, 11)
    types = np.arange(n) % 3
    eng = pse_amd.Engine(n, (L, L, L, 0.0), xi=0.5, error=1e-3)
    pos, dvel, image = to4(pos0), to4(vel, 1.0), torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    accel, force = torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    origins = eng.msd_origins(types, 3, 2)
    eng.msd_store(pos, image, origins, 0, 0.0)
    xy, flips, seen_flip, dropped = 0.0, 0, False, 0
    for step, (mpos, mimage, mbox, mflips, ru, _) in enumerate(mr.shear_trajectory(pos0, vel, steps)):
        xy, flips = mr.next_tilt(xy, flips)
        eng.set_box(L, L, L, xy)
        f = torch.floor((pos[:, 0] - xy * pos[:, 1]) / L + 0.5)                # System._set_tilt
        pos[:, 0] -= f * L
        image[:, 0] += f.to(torch.int32)
        eng.integrate(pos, dvel, accel, image, force, dt, shear_rate=rate)
        assert (xy, flips) == (mbox[3], mflips)
        hp, hi = pos.cpu().numpy()[:, :3], image.cpu().numpy()
        assert np.array_equal(hp, mpos) and np.array_equal(hi, mimage), "the host model of the step is the step"
        want = ru - pos0
        got = eng.msd_displacement(pos, image, origins, 0, xy + flips).cpu().numpy()
        assert np.array_equal(got[:, :3], want) and np.array_equal(got[:, 3], (want ** 2).sum(axis=1)), step
        sums = torch.zeros((1, 3, 10), dtype=torch.float64, device="cuda")
        eng.msd_accumulate(pos, image, origins, xy + flips, [0], [0], sums)
        tab = mr.moment_table(want)                                            # (dyadic, 64 terms: float64 is exact here)
        assert np.array_equal(sums.cpu().numpy()[0], np.stack([tab[types == a].sum(axis=0) for a in range(3)])), step
        if flips:                                                              # the case can fail: without the flip count, off by iy Lx
            seen_flip = True
            stale = eng.msd_displacement(pos, image, origins, 0, xy).cpu().numpy()
            assert np.array_equal(stale[:, 0] - want[:, 0], -hi[:, 1] * L)
            dropped = max(dropped, int(np.count_nonzero(hi[:, 1])))
            assert np.array_equal(analyze.unwrap(hp, hi, mbox, xy + flips), ru)
    assert seen_flip and dropped >= 10 and np.count_nonzero(hi[:, 0]) >= 5
    eng.close()


# -- 4. analyze.MSD on a System --------------------------------------------------------------------------------------------------------

@pytest.fixture
def restored_context():
    """A System registers itself as the current simulation context: put back what was there."""
    from pse_amd import context
    saved = context.current
    yield
    context.current = saved


class UniformForce:
    def __init__(self, system, fy):
        self.system, self.fy = system, fy
        system.forces.append(self)

    def compute(self, timestep):
        self.system.net_force[:, 1] += self.fy


class ByHand:
    """The schedule of analyze.MSD driven through the engine calls, with a list of origins instead of the scheduler's arithmetic."""

    def __init__(self, pse, nlags, every, types, ntypes):
        import torch
        self.pse, self.nlags, self.every, self.s = pse, nlags, every, 0
        self.norigins = -(-nlags // every)
        self.origins = pse.engine.msd_origins(types, ntypes, self.norigins)
        self.sums = torch.zeros((nlags, ntypes, 10), dtype=torch.float64, device="cuda")
        self.counts, self.live, self.snaps = np.zeros(nlags, dtype=np.int64), [], []
        pse.system.analyzers.append(self)

    def analyze(self, timestep):
        s, e = self.pse.system, self.pse.engine
        live = [(born, slot) for born, slot in self.live if 1 <= self.s - born <= self.nlags]
        if live:
            e.msd_accumulate(s.pos, s.image, self.origins, s.strain, [slot for _, slot in live], [self.s - born - 1 for born, _ in live],
                             self.sums)
            for born, _ in live:
                self.counts[self.s - born - 1] += 1
        if self.s % self.every == 0:
            slot = (self.s // self.every) % self.norigins
            self.live = [v for v in self.live if v[1] != slot] + [(self.s, slot)]
            e.msd_store(s.pos, s.image, self.origins, slot, s.strain)
        self.snaps.append((s.pos.cpu().numpy()[:, :3].copy(), s.image.cpu().numpy().copy(), s.box, s.strain))
        self.s += 1


def sheared_run(shear, steps, nlags=6, every=2):
    from pse_amd import analyze, integrate, shear_function, variant
    from pse_amd.system import System
    dt, rate = 2.0 ** -6, 2.0                                                  # the tilt grows by 1/32 per step: the flip at step 16
    s = System.create_lattice_sc(4.0, 3, dt=dt)
    fn = shear_function.steady(dt=dt, shear_rate=rate) if shear else None
    pse = integrate.PSEv1(group=s.all(), T=0.0, seed=3, xi=0.5, error=1e-3, function_form=fn)
    if shear:
        s.box_tilt_variant = variant.shear_variant(fn, 100000, max_strain=0.5)
    UniformForce(s, 2000.0)
    types = np.arange(s.n) % 3
    msd = analyze.MSD(pse, nlags, origin_every=every, types=[["A", "B", "C"][t] for t in types], type_names=["A", "B", "C"])
    hand = ByHand(pse, nlags, every, types, 3)
    s.run(steps)
    return s, msd, hand, types


def test_analyzer_through_system_run_under_a_shear_that_flips(restored_context):
    """counts, lags and sums of analyze.MSD against the same schedule driven by hand through the engine calls (equal bits), tilt_flips,
    and the yy, zz and yz moments against an extended-precision evaluation of y + iy Ly, z + iz Lz from the positions and images of
    every sample -- no strain, no tilt and no x enter those.

    yy, zz, yz are NOT equal between this run and the same run without the shear, and cannot be with
    hydrodynamics: the velocity that the uniform force gives the lattice is a lattice sum over the periodic images, and the images of
    a tilted box sit elsewhere -- the particles of the sheared run really move differently in y.  This test prints the relative
    difference of the yy moments of the two runs (the figure is in docs/HISTORY.md) and asserts that yy, zz, yz carry nothing of the
    shear, the strain or the unwrapping of x against the host evaluation, within the bound of the general-position test; the
    comparison of the two RUNS is asserted where it can hold, with prescribed velocities
    (test_yy_zz_yz_do_not_depend_on_the_shear_when_the_motion_is_prescribed).  The variant's tilt, rate t dt, and the integrator's advection, rate y dt per step, agree step for step:
    both are multiples of 2^-5 here, and tests/test_msd_cpu.py checks that tilt + flips is the plain sum of the increments."""
    mr.need_extended_precision()
    steps, nlags, every = 24, 6, 2
    s, msd, hand, types = sheared_run(True, steps)
    assert s.tilt_flips == 1 and s.box[3] < 0.0 and s.strain == (steps - 1) * 2.0 * 2.0 ** -6
    image = s.image.cpu().numpy()
    assert np.count_nonzero(image[:, 1]) >= 9, "the force was to carry particles through the y face"
    assert np.array_equal(msd.lags, np.arange(1, nlags + 1)) and msd.samples == steps
    assert np.array_equal(msd.counts, hand.counts) and msd.counts.tolist() == [sum(1 for t in range(steps) for o in range(0, t, every)
                                                                                   if t - o == lag) for lag in range(1, nlags + 1)]
    got = msd.sums
    assert np.array_equal(got, hand.sums.cpu().numpy()) and got.shape == (nlags, 3, 10)
    # yy, zz, yz from the samples' own y_u, z_u
    want = np.zeros((nlags, 3, 10), dtype=np.longdouble)
    tol = np.zeros((nlags, 3, 10))
    counts3 = np.bincount(types, minlength=3)
    unwrapped = [mr.unwrap_ld(p, im, box[:3], strain * box[1]) for p, im, box, strain in hand.snaps]
    for t in range(steps):
        for o in range(0, t, every):
            if 1 <= t - o <= nlags:
                m, _ = mr.moments_ld(unwrapped[t], unwrapped[o], types, 3)
                want[t - o - 1] += m
                R = float(max(np.abs(unwrapped[t]).max(), np.abs(unwrapped[o]).max()))
                D = float(np.sqrt(((unwrapped[t] - unwrapped[o]) ** 2).sum(axis=1).max()))
                tol[t - o - 1] += bound_small(s.n, counts3, R, D) + U * np.abs(np.asarray(want[t - o - 1], dtype=np.float64))
    for c in (1, 2, 4, 5, 8):                                                  # dy, dz, dy^2, dz^2, dy dz
        assert np.all(np.abs(got[..., c].astype(np.longdouble) - want[..., c]) <= tol[..., c]), c
    assert np.all(got[..., 4] > 0.0)
    # the readers
    n_a = counts3.astype(np.float64)
    den = msd.counts[:, None] * n_a[None, :]
    assert np.allclose(msd.msd_tensor("B")[:, 1, 1], got[:, 1, 4] / den[:, 1], rtol=1e-15, atol=0.0)
    with pytest.warns(RuntimeWarning, match="flipped box"):                   # the trace contains x: see analyze.unwrap, LIMIT
        trace = msd.msd()
    assert msd.flipped and np.allclose(trace, got[:, :, 3:6].sum(axis=(1, 2)) / (msd.counts * s.n), rtol=1e-14, atol=0.0)
    assert np.allclose(msd.mean_displacement(0)[:, 1], got[:, 0, 1] / den[:, 0], rtol=1e-15, atol=0.0)
    t9 = msd.msd_tensor()
    assert t9.shape == (nlags, 3, 3) and np.array_equal(t9, t9.transpose(0, 2, 1))
    with pytest.warns(RuntimeWarning, match="flipped box"):
        a2 = msd.alpha2()
    d2 = got[:, :, 3:6].sum(axis=(1, 2)) / (msd.counts * s.n)
    assert np.allclose(a2, 3.0 * got[:, :, 9].sum(axis=1) / (msd.counts * s.n) / (5.0 * d2 * d2) - 1.0, rtol=1e-12, atol=1e-12)
    disp = msd.displacement(lag=1)                                            # the origin of sample 22, one before the last sample
    now = mr.unwrap_ld(s.pos.cpu().numpy()[:, :3], image, s.box[:3], s.strain * s.box[1])
    assert np.abs(disp[:, 1:3].astype(np.longdouble) - (now - unwrapped[steps - 2])[:, 1:3]).max() <= 8 * U * float(np.abs(now).max())
    assert np.array_equal(disp, msd.displacement(slot=msd._schedule.slot_of_lag(1))) and msd._schedule.slot_of_lag(1) == 11 % 3
    with pytest.raises(ValueError, match="a slot or a lag"):
        msd.displacement()
    with pytest.raises(ValueError, match="no live origin"):
        msd.displacement(lag=2)                                                # sample 21 was no origin
    # the same run without the shear: printed, not asserted (see above)
    import warnings
    s0, msd0, _, _ = sheared_run(False, steps)
    assert s0.tilt_flips == 0 and s0.strain == 0.0 and not msd0.flipped
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                         # no flip, no warning
        assert np.all(msd0.msd() > 0.0)
    yy, yy0 = msd.msd_tensor()[:, 1, 1], msd0.msd_tensor()[:, 1, 1]
    print(f"yy moment with and without the shear, relative difference per lag: {np.abs(yy - yy0) / yy0}")
    msd.reset()
    assert msd.samples == 0 and not msd.sums.any() and not msd.counts.any() and not msd.flipped
    for slot in range(msd.norigins):                                           # the slots still hold the old origins: not live
        with pytest.raises(ValueError, match="since the last reset"):
            msd.displacement(slot=slot)


class PrescribedMotion:
    """An integrator for System.run that moves the particles with fixed velocities: Engine.integrate (pse_integrate) with a shear
    rate, on an engine of its own -- what analyze.MSD needs of an integrator (system, group, engine) and System of one (update,
    set_box).  No hydrodynamics: y and z move the same way whatever the box does."""

    def __init__(self, system, vel, rate):
        import pse_amd
        from pse_amd.system import Group
        self.system, self.group, self.rate = system, Group(system), rate
        self.engine = pse_amd.Engine(system.n, system.box, xi=0.5, error=1e-3)
        system.vel[:, :3] = to4(vel)[:, :3]
        system.integrators.append(self)

    def set_box(self, box):
        self.engine.set_box(*box)

    def update(self, timestep):
        s = self.system
        self.engine.integrate(s.pos, s.vel, s.accel, s.image, s.net_force, s.dt, shear_rate=self.rate)


def prescribed_run(shear, steps, nlags, every):
    from pse_amd import analyze, shear_function, variant
    from pse_amd.system import System
    dt, rate = 2.0 ** -6, 2.0                                                  # the tilt grows by 1/32 per step: the flip at step 16
    s = System.create_lattice_sc(4.0, 3, dt=dt)                                # 27 particles at -4, 0, 4 in a box of 12: dyadic
    rng = np.random.default_rng(41)
    vel = rng.integers(-8, 9, (s.n, 3)).astype(np.float64)
    vel[:, 1] = np.where(np.arange(s.n) % 2 == 0, 16.0, -24.0)                 # a quarter and 3/8 per step through the y faces
    mover = PrescribedMotion(s, vel, rate if shear else 0.0)
    if shear:
        s.box_tilt_variant = variant.shear_variant(shear_function.steady(dt=dt, shear_rate=rate), 100000, max_strain=0.5)
    types = np.arange(s.n) % 3
    msd = analyze.MSD(mover, nlags, origin_every=every, types=types)
    s.run(steps)
    return s, msd, mover


def test_yy_zz_yz_do_not_depend_on_the_shear_when_the_motion_is_prescribed(restored_context):
    """analyze.MSD on a System whose particles move with prescribed velocities (no hydrodynamics, dyadic data), once under a steady
    shear whose box flips at step 16 and once without: the y images change in both, before and after the flip, and the moments
    without x -- dy, dz, dy^2, dz^2, dy dz -- of the two runs are EQUAL BIT FOR BIT, as are counts and lags; the moments with x
    differ (the advection, and after the flip the limit of analyze.unwrap)."""
    steps, nlags, every = 40, 6, 2
    s1, m1, e1 = prescribed_run(True, steps, nlags, every)
    s0, m0, e0 = prescribed_run(False, steps, nlags, every)
    assert s1.tilt_flips == 1 and s0.tilt_flips == 0 and s1.strain == (steps - 1) / 32.0 and m1.flipped and not m0.flipped
    i1, i0 = s1.image.cpu().numpy(), s0.image.cpu().numpy()
    assert np.array_equal(i1[:, 1:], i0[:, 1:]) and np.abs(i0[:, 1]).min() >= 1 and np.abs(i0[:, 1]).max() >= 2   # before and after step 16
    assert np.array_equal(s1.pos.cpu().numpy()[:, 1:3], s0.pos.cpu().numpy()[:, 1:3])
    g1, g0 = m1.sums, m0.sums
    free = [1, 2, 4, 5, 8]                                                     # dy, dz, dy^2, dz^2, dy dz
    assert np.array_equal(g1[..., free], g0[..., free]) and np.all(g0[..., 4] > 0.0) and np.any(g0[..., 8] != 0.0)
    assert not np.array_equal(g1[..., 3], g0[..., 3])                          # dx^2 does contain the shear
    assert np.array_equal(m1.counts, m0.counts) and np.array_equal(m1.lags, m0.lags) and m1.counts.min() >= 15
    t1, t0 = m1.msd_tensor(), m0.msd_tensor()
    for i, j in ((1, 1), (2, 2), (1, 2)):
        assert np.array_equal(t1[:, i, j], t0[:, i, j])
    assert np.array_equal(m1.mean_displacement()[:, 1:], m0.mean_displacement()[:, 1:])
    # the unsheared run is plain kinematics: dy = v_y lag dt for every particle
    vy2 = np.where(np.arange(s0.n) % 2 == 0, 16.0, -24.0) ** 2
    types = np.arange(s0.n) % 3
    for a in range(3):
        want = vy2[types == a].sum() * (np.arange(1, nlags + 1) * 2.0 ** -6) ** 2 * m0.counts
        assert np.array_equal(g0[:, a, 4], want)
    for e in (e1, e0):
        e.engine.close()


def bound_small(n, counts, R, D):
    """bound() without the cap of the sequential sum, which a few dozen particles per type cannot meet: with one wave there is one row
    of the workspace and the other strips of k_msd_finish add exact zeros, so the depth that counts is 3 + 6 + 2 + 1 + 1."""
    e = 5.0 * U * max(R, D)
    out = np.zeros((len(counts), 10))
    for c, q in enumerate(ORDER):
        for a, na in enumerate(counts):
            out[a, c] = na * (CQ[q] * e * (D + e) ** (q - 1) + (13 + FQ[q]) * U * D ** q)
    return out


# -- 5. queue-only ------------------------------------------------------------------------------------------------------------------

def test_store_and_accumulate_captured_into_a_graph_replay_the_eager_bits():
    import torch
    import pse_amd
    n, ntypes = 1000, 3
    now, slots = general_case(n, 2, 31)
    types = types_for(n, ntypes, 32, "all")
    eng = pse_amd.Engine(n, BOX, xi=0.5, error=1e-3)
    eng.set_async(True)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    origins = eng.msd_origins(types, ntypes, 2)
    pos, image = to4(slots[0][0]), dev_image(slots[0][1])
    sums = torch.zeros((3, ntypes, 10), dtype=torch.float64, device="cuda")

    def sample():
        eng.msd_accumulate(pos, image, origins, 0.8, [1, 0], [0, 2], sums)
        eng.msd_store(pos, image, origins, 0, 0.8)

    with torch.cuda.stream(st):
        eng.msd_store(pos, image, origins, 0, slots[0][2])                     # eager: two origins, then two samples
        eng.msd_store(to4(slots[1][0]), dev_image(slots[1][1]), origins, 1, slots[1][2])
    st.synchronize()
    frames = [(now[0], now[1]), (slots[1][0] + 0.25, slots[1][1])]
    eager = []
    for p, im in frames:
        pos.copy_(to4(p)); image.copy_(dev_image(im))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            sample()
        st.synchronize()
        eager.append(sums.cpu().numpy().copy())
    assert np.abs(eager[1] - eager[0]).max() > 0.0 and not np.any(eager[0][1])
    # the same two samples from a captured graph, from the same start
    with torch.cuda.stream(st):
        eng.msd_store(to4(slots[0][0]), dev_image(slots[0][1]), origins, 0, slots[0][2])
    st.synchronize()
    sums.zero_()
    pos.copy_(to4(frames[0][0])); image.copy_(dev_image(frames[0][1]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
        sample()
    torch.cuda.synchronize()
    assert not sums.cpu().numpy().any(), "a capture runs nothing"
    for k, (p, im) in enumerate(frames):
        pos.copy_(to4(p)); image.copy_(dev_image(im))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(sums.cpu().numpy(), eager[k]), k
    origins.close()
    eng.close()


# -- 6. refusals on the device ---------------------------------------------------------------------------------------------------------

def test_refusals_leave_sums_untouched_and_a_slab_rank_works():
    """Raw C-ABI, as a C host would call it: a refused call writes nothing, and the object works afterwards; the passes work on a slab
    rank's handle (exact case)."""
    import torch
    from pse_amd import _lib
    from pse_amd._lib import pse_params
    lib = _lib.load()
    msg = lambda: lib.pse_last_error().decode()          # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731
    ints = lambda *v: np.array(v, dtype=np.int32)          # noqa: E731

    def create(L, n_max, **kw):
        p = pse_params()
        p.n_max, p.Lx, p.Ly, p.Lz, p.xy = n_max, L, L, L, 0.0
        p.xi, p.error, p.max_strain, p.seed = 0.5, 1e-3, 0.5, 1
        p.Nx = p.Ny = p.Nz = 0
        p.P, p.rcut, p.device, p.n_slabs, p.slab_rank = 0, 0.0, -1, 1, 0
        for k, v in kw.items():
            setattr(p, k, v)
        out = ctypes.c_void_p()
        return lib.pse_create(ctypes.byref(p), ctypes.byref(out)), out

    n, ntypes, L = 257, 2, 16.0
    lengths = (L, L, L)
    now, slots = dyadic_case(n, 2, 3, lengths)                                 # (strain Ly multiples of 2^-4 at Ly = 16 and 40 too)
    types = types_for(n, ntypes, 4, "all").astype(np.uint32)
    rc, h = create(L, n)
    assert rc == 0, msg()
    m = ctypes.c_void_p(777)
    assert lib.pse_msd_create(h, n + 1, vp(types), ntypes, 4, ctypes.byref(m)) == INVALID and "n = 258" in msg() and not m.value
    assert lib.pse_msd_create(h, n, vp(types), ntypes, 65, ctypes.byref(m)) == INVALID and "norigins = 65" in msg() and not m.value
    assert lib.pse_msd_create(h, n, vp(types), ntypes, 4, ctypes.byref(m)) == 0 and m.value, msg()
    pos, image = to4(now[0]), dev_image(now[1])
    sums = torch.full((3, ntypes, 10), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((n, 4), -5.0, dtype=torch.float64, device="cuda")

    def store(k):
        assert lib.pse_msd_store(m, k, P(to4(slots[k][0])), P(dev_image(slots[k][1])), None, n, slots[k][2]) == 0, msg()

    def acc(word, pos_=P(pos), image_=P(image), nn=n, strain=now[2], npairs=2, sl=ints(0, 1), ro=ints(2, 0), nrows=3, su=P(sums)):
        rc = lib.pse_msd_accumulate(m, pos_, image_, None, nn, strain, npairs, None if sl is None else vp(sl), None if ro is None else vp(ro),
                                    nrows, su)
        assert (word is None and rc == 0) or (rc == INVALID and word in msg() and "pse_msd_accumulate" in msg()), (word, rc, msg())

    acc("slot 0, which was never stored")
    store(0)
    acc("slot 1, which was never stored")
    assert lib.pse_msd_displacement(m, 1, P(pos), P(image), None, n, 0.0, P(out)) == INVALID and "never stored" in msg()
    store(1)
    acc("N = 0", nn=0)
    acc("N = 258", nn=n + 1)
    acc("null pos", pos_=None)
    acc("null image", image_=None)
    acc("strain = nan", strain=float("nan"))
    acc("npairs = 0", npairs=0)
    acc("npairs = 65", npairs=65)
    acc("null slots_host", sl=None)
    acc("null rows_host", ro=None)
    acc("nrows = 0", nrows=0)
    acc("slot 4 outside", sl=ints(0, 4))
    acc("slot 2, which was never stored", sl=ints(0, 2))
    acc("row 3 outside", ro=ints(3, 0))
    acc("both name the row 2", ro=ints(2, 2))
    acc("null sums", su=None)
    acc("8-byte aligned", su=ctypes.c_void_p(sums.data_ptr() + 4))
    assert lib.pse_msd_accumulate(None, P(pos), P(image), None, n, 0.0, 2, vp(ints(0, 1)), vp(ints(2, 0)), 3, P(sums)) == INVALID
    for bad in (dict(slot=4), dict(nn=0), dict(strain=float("inf")), dict(o=None), dict(o=ctypes.c_void_p(out.data_ptr() + 4))):
        a = dict(dict(slot=0, nn=n, strain=0.0, o=P(out)), **bad)
        assert lib.pse_msd_displacement(m, a["slot"], P(pos), P(image), None, a["nn"], a["strain"], a["o"]) == INVALID, bad
        assert lib.pse_msd_store(m, a["slot"], P(pos), P(image), None, a["nn"], a["strain"]) == (INVALID if "o" not in bad else 0)
    torch.cuda.synchronize()
    assert np.all(sums.cpu().numpy() == -7.0) and np.all(out.cpu().numpy() == -5.0)       # nothing was launched, nothing was written
    store(0)                                                                              # (the two stores above that passed wrote slot 0)
    acc(None)
    want = exact_reference(now, slots, lengths, types, ntypes)
    got = sums.cpu().numpy()
    assert np.array_equal(got[2], want[0] - 7.0) and np.array_equal(got[0], want[1] - 7.0) and np.all(got[1] == -7.0)
    # a slab rank's handle: positions are replicated there, the sums are complete (its box is 40^3)
    rc, hs = create(40.0, n, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    assert rc == 0, msg()
    ms = ctypes.c_void_p()
    assert lib.pse_msd_create(hs, n, vp(types), ntypes, 2, ctypes.byref(ms)) == 0, msg()
    now_s, slots_s = dyadic_case(n, 2, 5, (40.0, 40.0, 40.0))
    for k in range(2):
        assert lib.pse_msd_store(ms, k, P(to4(slots_s[k][0])), P(dev_image(slots_s[k][1])), None, n, slots_s[k][2]) == 0, msg()
    sums.zero_()
    assert lib.pse_msd_accumulate(ms, P(to4(now_s[0])), P(dev_image(now_s[1])), None, n, now_s[2], 2, vp(ints(0, 1)), vp(ints(2, 0)), 3, P(sums)) == 0, msg()
    want = exact_reference(now_s, slots_s, (40.0, 40.0, 40.0), types, ntypes)
    got = sums.cpu().numpy()
    assert np.array_equal(got[2], want[0]) and np.array_equal(got[0], want[1]) and not got[1].any()
    assert lib.pse_msd_destroy(ms) == 0 and lib.pse_msd_destroy(None) == 0
    for hh in (h, hs):                                                                    # m is still alive: it goes with its handle
        assert lib.pse_destroy(hh) == 0
