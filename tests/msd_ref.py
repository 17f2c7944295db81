"""The reference of the displacement-moment tests: the unwrapped position x + ix Lx + iy sLy, y + iy Ly, z + iz Lz (sLy = strain Ly,
formed in double as the library forms it) and the ten moments of a displacement summed per type -- dx dy dz, dx^2 dy^2 dz^2 dxdy
dxdz dydz, (dx^2 + dy^2 + dz^2)^2 -- in two forms.  EXACT: for dyadic inputs, multiples of 2^-4, everything is an integer in units of
2^-4 (positions), 2^-8 (second moments) and 2^-16 (the fourth); the element-wise products are int64, whose range the conditions of
`dyadic_units` keep far away, and every sum is a sum of Python integers.  EXTENDED: numpy.longdouble on the double inputs.  Plus a host
model of the integration step's wrap and of the re-wrap behind a changed tilt, for the trajectory tests.  NumPy only."""
import numpy as np

UNIT = 16            # 1 / 2^-4
MOMENTS = 10
SCALE = np.array([UNIT] * 3 + [UNIT ** 2] * 6 + [UNIT ** 4], dtype=object)   # units per moment


def need_extended_precision():
    import pytest
    if np.finfo(np.longdouble).eps > 2.0 ** -60:
        pytest.skip("numpy.longdouble is not an extended type on this platform")


def dyadic_units(x):
    """x (float64 array or scalar) in units of 2^-4 as int64; asserts that every value is such a multiple and below 2^31 units."""
    u = np.asarray(x, dtype=np.float64) * UNIT
    assert np.all(np.isfinite(u)) and np.all(u == np.rint(u)), "not a multiple of 2^-4"
    assert np.all(np.abs(u) < 2.0 ** 31)
    return u.astype(np.int64)


def unwrap_exact(pos, image, lengths, sLy):
    """r_u in units of 2^-4, int64 (N, 3): every input must be a multiple of 2^-4 (asserted) and every product below 2^62."""
    p, L, s = dyadic_units(np.asarray(pos)[:, :3]), dyadic_units(lengths), int(dyadic_units(sLy))
    im = np.asarray(image).astype(np.int64)
    assert np.abs(im).max(initial=0) < 2 ** 20
    return np.stack([p[:, 0] + im[:, 0] * int(L[0]) + im[:, 1] * s, p[:, 1] + im[:, 1] * int(L[1]), p[:, 2] + im[:, 2] * int(L[2])], axis=1)


def unwrap_ld(pos, image, lengths, sLy):
    """r_u in numpy.longdouble from the double inputs, (N, 3)."""
    ld = np.longdouble
    p, im = np.asarray(pos, dtype=np.float64)[:, :3].astype(ld), np.asarray(image).astype(ld)
    Lx, Ly, Lz, s = ld(np.float64(lengths[0])), ld(np.float64(lengths[1])), ld(np.float64(lengths[2])), ld(np.float64(sLy))
    return np.stack([p[:, 0] + im[:, 0] * Lx + im[:, 1] * s, p[:, 1] + im[:, 1] * Ly, p[:, 2] + im[:, 2] * Lz], axis=1)


def moment_table(d):
    """The ten moments of every row of d (M, 3), in d's own arithmetic (int64 or longdouble), (M, 10)."""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    r2 = dx * dx + dy * dy + dz * dz
    return np.stack([dx, dy, dz, dx * dx, dy * dy, dz * dz, dx * dy, dx * dz, dy * dz, r2 * r2], axis=1)


def member_types(types, members, n):
    """The type of every member (caller-order indices), with the library's rule: no types, or an index past them, is type 0."""
    members = np.arange(n) if members is None else np.asarray(members, dtype=np.int64)
    if types is None:
        return members, np.zeros(members.shape[0], dtype=np.int64)
    types = np.asarray(types, dtype=np.int64)
    return members, np.where(members < types.shape[0], types[np.minimum(members, types.shape[0] - 1)], 0)


def moments_exact(now_u, slot_u, types, ntypes, members=None):
    """(ntypes, 10) float64, EXACT: the sums over the members of every type of the moments of now_u - slot_u (int64, units of 2^-4),
    added as Python integers and divided by the moment's power of two; asserts |d| < 32 per component and that every result is
    representable (below 2^53 units)."""
    members, ty = member_types(types, members, now_u.shape[0])
    d = now_u[members] - slot_u[members]
    assert np.abs(d).max(initial=0) < 32 * UNIT, "a displacement component of 32 or more"
    assert members.shape[0] <= 4096
    tab = moment_table(d).astype(object)
    out = np.zeros((ntypes, MOMENTS))
    for a in range(ntypes):
        tot = tab[ty == a].sum(axis=0) if np.any(ty == a) else np.zeros(MOMENTS, dtype=object)
        for c in range(MOMENTS):
            assert abs(int(tot[c])) < 2 ** 53
            out[a, c] = int(tot[c]) / int(SCALE[c])     # (an integer below 2^53 over a power of two: exact)
    return out


def moments_ld(now, slot, types, ntypes, members=None):
    """(ntypes, 10) longdouble: the same sums in extended precision, and the per-type counts N_a."""
    members, ty = member_types(types, members, now.shape[0])
    tab = moment_table(now[members] - slot[members])
    out = np.zeros((ntypes, MOMENTS), dtype=np.longdouble)
    for a in range(ntypes):
        out[a] = tab[ty == a].sum(axis=0, dtype=np.longdouble)
    return out, np.bincount(ty, minlength=ntypes)


# ---- host models of the step's wrap, of the re-wrap behind a changed tilt, and of the unwrapped trajectory --------------------------

def integrate_model(pos, image, vel, box, dt, rate):
    """What pse_integrate does to (pos (N, 3), image (N, 3)) with velocities vel in the box (Lx, Ly, Lz, xy): the Euler step with the
    shear term, then the triclinic wrap z, y (a y image shifts x by xy Ly), x.  In place; plain float64, the same operations in the
    same order as the kernel (exact on dyadic data)."""
    Lx, Ly, Lz, xy = box
    pos[:, 0] += (vel[:, 0] + rate * pos[:, 1]) * dt
    pos[:, 1] += vel[:, 1] * dt
    pos[:, 2] += vel[:, 2] * dt
    n = np.floor(pos[:, 2] * (1.0 / Lz) + 0.5)
    pos[:, 2] -= n * Lz; image[:, 2] += n.astype(image.dtype)
    n = np.floor(pos[:, 1] * (1.0 / Ly) + 0.5)
    pos[:, 1] -= n * Ly; pos[:, 0] -= n * xy * Ly; image[:, 1] += n.astype(image.dtype)
    n = np.floor((pos[:, 0] - xy * pos[:, 1]) * (1.0 / Lx) + 0.5)
    pos[:, 0] -= n * Lx; image[:, 0] += n.astype(image.dtype)


def set_tilt_model(pos, image, box, xy):
    """What System._set_tilt does: the new box, and x re-wrapped into its primary cell with image.x adjusted.  In place; returns the
    new box."""
    Lx, Ly, Lz, _ = box
    f = np.floor((pos[:, 0] - xy * pos[:, 1]) / Lx + 0.5)
    pos[:, 0] -= f * Lx
    image[:, 0] += f.astype(image.dtype)
    return (Lx, Ly, Lz, float(xy))


def unwrapped_step(ru, vel, dt, rate):
    """The recurrence of the unwrapped trajectory: x_u += (v_x + rate y_u) dt, y_u += v_y dt, z_u += v_z dt.  In place."""
    ru[:, 0] += (vel[:, 0] + rate * ru[:, 1]) * dt
    ru[:, 1] += vel[:, 1] * dt
    ru[:, 2] += vel[:, 2] * dt


SHEAR_L, SHEAR_DT, SHEAR_RATE = 16.0, 2.0 ** -4, 2.0      # the tilt grows by 1/8 per step: beyond +0.5, the flip, at the fifth step


def shear_case(n, seed, late=False):
    """Dyadic start of the trajectory tests in the cubic box SHEAR_L: positions (n, 3) -- x and z multiples of 2^-4, y of 1/2 -- and
    integer velocities, so that every coordinate stays a multiple of 2^-4.  A third of the particles moves up and a third down through
    the y faces at one unit per step; late = False: from within 3.5 of the face, so that every y image is gained in the first four
    steps, BEFORE the flip; late = True: from anywhere."""
    rng = np.random.default_rng(seed)
    h = SHEAR_L / 2
    pos = rng.integers(-h * 16, h * 16, (n, 3)) / 16.0
    pos[:, 1] = rng.integers(-h * 2, h * 2, n) / 2.0
    vel = rng.integers(-16, 17, (n, 3)).astype(np.float64)
    kind = np.arange(n) % 3
    vel[:, 1] = np.where(kind == 0, 0.0, np.where(kind == 1, 16.0, -16.0))
    if not late:
        near = rng.integers(1, 8, n) / 2.0                     # 0.5 .. 3.5 from the face
        pos[:, 1] = np.where(kind == 0, pos[:, 1], np.where(kind == 1, h - near, -h + near - 0.5))
    return pos, vel


def next_tilt(xy, flips, dt=SHEAR_DT, rate=SHEAR_RATE):
    """The tilt of the next step of a steady shear and the flips so far: advanced by rate dt, and beyond +0.5 flipped by -1."""
    new = xy + rate * dt
    return (new - 1.0, flips + 1) if new > 0.5 else (new, flips)


def shear_trajectory(pos, vel, steps, dt=SHEAR_DT, rate=SHEAR_RATE, L=SHEAR_L):
    """The host model of a sheared run from (pos, vel) -- per step: the tilt advanced (next_tilt) and x re-wrapped as System._set_tilt
    does, then one integration step -- next to the recurrence of the unwrapped trajectory.  Yields, after every step, (pos, image, box,
    flips, r_u of the recurrence, the y images gained in this step); the arrays are the model's own, reused from step to step."""
    pos, image, ru, box, flips = pos.copy(), np.zeros(pos.shape, dtype=np.int64), pos.copy(), (L, L, L, 0.0), 0
    for _ in range(steps):
        xy, flips = next_tilt(box[3], flips, dt, rate)
        box = set_tilt_model(pos, image, box, xy)
        iy = image[:, 1].copy()
        unwrapped_step(ru, vel, dt, rate)
        integrate_model(pos, image, vel, box, dt, rate)
        yield pos, image, box, flips, ru, image[:, 1] - iy
