"""Reference of the static structure factor (pse_structure_factor_accumulate; include/pse_amd.h), in extended precision: the fractional
coordinates s = ((x - xy y)/Lx, y/Ly, z/Lz) of the float64 positions, t = m.s, t -= rint(t), cos and sin of 2 pi t, all in
np.longdouble (eps 1.08e-19 where the C long double is the x87 format), summed per type and rounded to float64 once.  Also the inputs
the CPU and the GPU tests share, the bound they compare against, and a plain-float64 restatement whose distance from the reference
the CPU tests measure against that bound."""
import numpy as np
import pytest

LD = np.longdouble
CUBIC = (14.0, 14.0, 14.0, 0.0)
TILTED = (14.0, 11.0, 17.0, 0.3)
NEGATIVE = (14.0, 11.0, 17.0, -0.5)
BOXES = {"cubic": CUBIC, "tilted": TILTED, "negative": NEGATIVE}
MAX_INDEX = 4096


def need_extended_precision():
    """The reference is only one if long double is wider than double: eps 1.08e-19 (x87).  Skips, loudly, where it is not."""
    eps = float(np.finfo(LD).eps)
    if not eps < 1.1e-19:
        pytest.skip(f"np.longdouble has eps = {eps:.3e} here, not 1.08e-19: NO EXTENDED PRECISION, the structure-factor reference is "
                    "not one on this machine")


def points(n, box, seed=11):
    """n seeded points inside the primary cell: fractional coordinates uniform in [-1/2, 1/2)."""
    s = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(n, 3))
    return from_fractional(s, box)


def from_fractional(s, box):
    Lx, Ly, Lz, xy = box
    y = s[:, 1] * Ly
    return np.stack([s[:, 0] * Lx + xy * y, y, s[:, 2] * Lz], axis=1)


def lattice_vectors(box):
    Lx, Ly, Lz, xy = box
    return np.array([[Lx, 0.0, 0.0], [xy * Ly, Ly, 0.0], [0.0, 0.0, Lz]])


def fractional(pos, box, dtype=LD):
    Lx, Ly, Lz, xy = (dtype(v) for v in box)
    p = np.asarray(pos, dtype=np.float64).astype(dtype)
    return np.stack([(p[:, 0] - xy * p[:, 1]) / Lx, p[:, 1] / Ly, p[:, 2] / Lz], axis=1)


def _rho(pos, box, modes, types, ntypes, dtype):
    s = fractional(pos, box, dtype)
    m = np.asarray(modes, dtype=np.int64).reshape(-1, 3).astype(dtype)
    two_pi = dtype(8) * np.arctan(dtype(1))
    types = np.zeros(len(s), dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    out = np.zeros((ntypes, m.shape[0]), dtype=np.complex128)
    for q0 in range(0, m.shape[0], 512):                                     # (blocks of modes: the table of phases stays small)
        t = s @ m[q0:q0 + 512].T
        t = t - np.rint(t)
        c, sn = np.cos(two_pi * t), np.sin(two_pi * t)
        for a in range(ntypes):
            sel = types == a
            out[a, q0:q0 + 512] = c[sel].sum(axis=0).astype(np.float64) - 1j * sn[sel].sum(axis=0).astype(np.float64)
    return out


def rho(pos, box, modes, types=None, ntypes=1):
    """rho[a, q] = sum_{j of type a} exp(-2 pi i m_q.s_j), complex128 rounded once from extended precision."""
    return _rho(pos, box, modes, types, ntypes, LD)


def rho_float64(pos, box, modes, types=None, ntypes=1):
    """The same statement in plain float64: what the bound must leave room for."""
    return _rho(pos, box, modes, types, ntypes, np.float64)


def pair_index(a, b, ntypes):
    a, b = (a, b) if a <= b else (b, a)
    return a * ntypes - a * (a - 1) // 2 + (b - a)


def products(r):
    """prod[p(a, b), q] = Re(rho_a conj rho_b), a <= b, from rho (ntypes, nk) complex."""
    nt = r.shape[0]
    out = np.zeros((nt * (nt + 1) // 2, r.shape[1]))
    for a in range(nt):
        for b in range(a, nt):
            out[pair_index(a, b, nt)] = r[a].real * r[b].real + r[a].imag * r[b].imag
    return out


def s_max(pos, box):
    return max(0.5, float(np.abs(fractional(pos, box, np.float64)).max()))


def tol(modes, n, smax=0.5):
    """The bound per component of rho, per mode: n (2e-14 + 4e-15 s_max (|mx| + |my| + |mz|)) -- three roundings in s times 2 pi |m|,
    two ulps of sincos, 64 recurrence steps, about twice the worst case."""
    m = np.abs(np.asarray(modes, dtype=np.int64).reshape(-1, 3)).sum(axis=1)
    return n * (2e-14 + 4e-15 * smax * m)


def worst_ratio(got, want, modes, n, smax=0.5):
    """max over modes and types of the larger component error over tol(m)."""
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    return float((err / tol(modes, n, smax)[None, :]).max())


# ---- the mode sets of the GPU tests -------------------------------------------------------------------------------------------------

def half_space(mmax):
    g = np.arange(-mmax, mmax + 1)
    m = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    keep = (m[:, 0] > 0) | ((m[:, 0] == 0) & ((m[:, 1] > 0) | ((m[:, 1] == 0) & (m[:, 2] > 0))))
    return m[keep]


def line(axis, lo=-100, hi=100, at=(5, -7)):
    """The modes lo..hi along `axis` with the other two indices `at`."""
    m = np.zeros((hi - lo + 1, 3), dtype=np.int64)
    m[:, [c for c in range(3) if c != axis]] = at
    m[:, axis] = np.arange(lo, hi + 1)
    return m


def scattered(nk, mmax, seed=5):
    return np.random.default_rng(seed).integers(-mmax, mmax + 1, size=(nk, 3))


def mode_sets():
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * MAX_INDEX
    return {"one": np.array([[3, -2, 5]]), "zero": np.array([[0, 0, 0]]), "half3": half_space(3), "corners": corners,
            "zline": line(2), "xline": line(0), "yline": line(1), "scattered": scattered(4096, 64)}
