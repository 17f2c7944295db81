"""CPU tests of the displacement moments that need no device: the reference the GPU tests compare to (tests/msd_ref.py) against its own
ties -- lattice invariance of the unwrapped position, continuity through a Lees-Edwards flip with the accumulated strain where the
position + image . box formula with the current tilt jumps, and where the strain formula itself still jumps (a y image gained AFTER a
flip), the integer path against the extended one --; the scheduler of analyze.MSD against a brute-force count; the flip count of
System._set_tilt; every refusal of the five pse_msd_* entry points through the device stand-in of the sanitizer build
(pse_amd/csrc/asan_stub.cpp, which runs the real validators), built here without a sanitizer; and the argument checks of the Python
layers that come before the device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import msd_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def dyadic_case(seed, n=200, L=(8.0, 16.0, 4.0), xy=0.3125):
    """Wrapped dyadic positions inside the tilted cell, images of both signs in all three axes."""
    rng = np.random.default_rng(seed)
    y = rng.integers(-L[1] * 8, L[1] * 8, n) / 16.0
    z = rng.integers(-L[2] * 8, L[2] * 8, n) / 16.0
    x = np.rint(xy * y * 16.0) / 16.0 + rng.integers(-L[0] * 8, L[0] * 8, n) / 16.0
    return np.stack([x, y, z], axis=1), rng.integers(-3, 4, (n, 3))


# ---- the reference's own ties ------------------------------------------------------------------------------------------------------

def test_unwrap_is_invariant_under_every_lattice_vector_of_the_current_box():
    from pse_amd import analyze
    L, xy = (8.0, 16.0, 4.0), 0.3125
    pos, image = dyadic_case(1, L=L, xy=xy)
    base = analyze.unwrap(pos, image, L + (xy,), xy)
    rng = np.random.default_rng(2)
    for _ in range(20):
        k = rng.integers(-4, 5, (pos.shape[0], 3))
        # the particle moved by k_x a1 + k_y a2 + k_z a3, a2 = (xy Ly, Ly, 0), and its image by -k
        moved = pos + np.stack([k[:, 0] * L[0] + k[:, 1] * xy * L[1], k[:, 1] * L[1], k[:, 2] * L[2]], axis=1)
        assert np.array_equal(analyze.unwrap(moved, image - k, L + (xy,), xy), base)      # (dyadic: exact)
    assert np.array_equal(base, mr.unwrap_exact(pos, image, L, xy * L[1]) / 16.0)
    assert analyze.unwrap(np.zeros((1, 4)), np.zeros((1, 3), dtype=int), L, 0.0).shape == (1, 3)


def synthetic_flip(pos, image, box, flips):
    """xy -> xy - 1, one more flip, and the re-wrap of x that System._set_tilt does."""
    pos, image = pos.copy(), image.copy()
    box = mr.set_tilt_model(pos, image, box, box[3] - 1.0)
    return pos, image, box, flips + 1


def test_unwrap_with_the_strain_is_continuous_through_a_flip_and_the_current_tilt_is_not():
    from pse_amd import analyze
    L = (8.0, 8.0, 4.0)
    box, flips = L + (0.5,), 0
    pos, image = dyadic_case(3, L=L, xy=0.5)
    before = analyze.unwrap(pos, image, box, box[3] + flips)
    p2, i2, box2, flips2 = synthetic_flip(pos, image, box, flips)
    assert box2[3] == -0.5 and flips2 == 1 and np.any(i2[:, 0] != image[:, 0])             # the re-wrap did move particles
    assert np.array_equal(analyze.unwrap(p2, i2, box2, box2[3] + flips2), before)          # with the strain: the same point
    # position + image . box with the CURRENT tilt, the formula dump.load used to document: off by image.y Lx, at every flip
    stale = analyze.unwrap(p2, i2, box2, box2[3])
    assert np.array_equal(stale[:, 0] - before[:, 0], -image[:, 1] * L[0]) and np.any(image[:, 1] != 0)
    assert np.array_equal(stale[:, 1:], before[:, 1:])


def test_strain_follows_the_trajectory_while_no_y_image_changes_after_a_flip_and_jumps_by_ly_when_one_does():
    """The limit of the definition, on record: x_u = x + ix Lx + iy strain Ly attributes strain Ly to EVERY y image, the step's wrap
    takes xy Ly (the current tilt) off x when one is gained, so a y image gained after `flips` flips shifts x_u by flips Ly.  Through
    the wraps before the first flip, through every x and z wrap and through the flips themselves it is exact.  (1) is the schedule
    of the device test of the trajectory (tests/test_gpu_msd.py)."""
    from pse_amd import analyze
    # (1) every y image is gained before the flip: exact through x, y, z wraps and the flip; without the flip count, off by iy Lx
    pos, vel = mr.shear_case(64, 11)
    for step, (p, image, box, flips, ru, gained) in enumerate(mr.shear_trajectory(pos, vel, 12)):
        assert flips == (step >= 4) and (flips == 0 or not np.any(gained))
        assert np.array_equal(analyze.unwrap(p, image, box, box[3] + flips), ru)
        stale = analyze.unwrap(p, image, box, box[3]) - ru
        assert np.array_equal(stale[:, 0], -flips * image[:, 1] * box[0]) and not np.any(stale[:, 1:])
    assert flips == 1 and np.count_nonzero(image[:, 1] > 0) >= 5 and np.count_nonzero(image[:, 1] < 0) >= 5
    assert np.count_nonzero(image[:, 0]) >= 5 and np.count_nonzero(image[:, 2]) >= 3
    # (2) y images gained after a flip: off by flips Ly each time, and only in x
    pos, vel = mr.shear_case(64, 12, late=True)
    off = np.zeros(64)
    for p, image, box, flips, ru, gained in mr.shear_trajectory(pos, vel, 24):
        off += gained * flips * box[1]
        d = analyze.unwrap(p, image, box, box[3] + flips) - ru
        assert np.array_equal(d[:, 0], off) and not np.any(d[:, 1:])
    assert flips == 3 and np.count_nonzero(off) >= 5


def test_integer_and_extended_paths_agree_on_dyadic_data():
    L, sLy = (8.0, 4.0, 16.0), -1.3125 * 4.0
    pos, image = dyadic_case(7, n=500, L=L)
    pos2, image2 = dyadic_case(8, n=500, L=L)
    image2 = np.clip(image2, image - 1, image + 1)                    # |d| stays below 32
    types = np.random.default_rng(9).integers(0, 3, 500)
    members = np.random.default_rng(10).permutation(500)[:300]
    extended = np.finfo(np.longdouble).eps <= 2.0 ** -60              # (only the comparison needs an extended long double)
    for mem in (None, members):
        exact = mr.moments_exact(mr.unwrap_exact(pos2, image2, L, sLy), mr.unwrap_exact(pos, image, L, sLy), types, 4, mem)
        assert not np.any(exact[3]) and np.all(exact[:3, 3:6] > 0)
        if extended:
            ext, counts = mr.moments_ld(mr.unwrap_ld(pos2, image2, L, sLy), mr.unwrap_ld(pos, image, L, sLy), types, 4, mem)
            assert np.array_equal(exact.astype(np.longdouble), ext) and counts[3] == 0
            assert counts.sum() == (500 if mem is None else 300)
    # types past the end and no types at all act as type 0
    a = mr.moments_exact(mr.unwrap_exact(pos2, image2, L, sLy), mr.unwrap_exact(pos, image, L, sLy), None, 1)
    b = mr.moments_exact(mr.unwrap_exact(pos2, image2, L, sLy), mr.unwrap_exact(pos, image, L, sLy), types[:100] * 0 + 0, 1)
    assert np.array_equal(a, b)
    with pytest.raises(AssertionError):
        mr.dyadic_units(np.array([0.03125]))


# ---- the scheduler ------------------------------------------------------------------------------------------------------------------

class Recorder:
    """A fake engine: records what an MSD sample asks of it."""

    def __init__(self):
        self.calls, self.slot_origin, self.t = [], {}, 0

    def accumulate(self, slots, rows):
        self.calls.append(("acc", self.t, list(slots), list(rows)))

    def store(self, slot):
        self.calls.append(("store", self.t, slot))


@pytest.mark.parametrize("nlags,every", [(1, 1), (5, 1), (5, 2), (7, 3), (64, 1), (640, 10)])
def test_schedule_takes_every_lag_of_every_origin_once_before_its_slot_is_reused(nlags, every):
    from pse_amd import analyze
    sch, rec = analyze.MSDSchedule(nlags, every), Recorder()
    assert sch.norigins == -(-nlags // every) <= 64
    nsamples = 3 * nlags + 2 * every + 5
    for t in range(nsamples):
        rec.t = t
        sch.sample(rec.accumulate, rec.store)
    in_slot, taken, brute = {}, {}, [0] * nlags          # slot -> the sample that was stored there; (origin sample) -> lags taken
    for call in rec.calls:
        if call[0] == "acc":
            _, t, slots, rows = call
            assert 1 <= len(slots) == len(rows) <= 64 and len(set(rows)) == len(rows) and len(set(slots)) == len(slots)
            for slot, row in zip(slots, rows):
                origin = in_slot[slot]                                                      # (KeyError: a slot never stored)
                assert t - origin == row + 1, "the row is the lag - 1 of what is in the slot"
                assert row + 1 not in taken[origin]
                taken[origin].add(row + 1)
        else:
            _, t, slot = call
            assert t % every == 0 and slot == (t // every) % sch.norigins
            if slot in in_slot:                                                             # reused: every lag was taken
                assert taken[in_slot[slot]] == set(range(1, nlags + 1))
            in_slot[slot] = t
            taken[t] = set()
    # accumulate comes before store in a sample, and the counts are those of a brute-force enumeration
    order = [(c[1], c[0]) for c in rec.calls]
    assert order == sorted(order, key=lambda v: (v[0], v[1] != "acc"))
    for t in range(nsamples):
        for origin in range(0, t, every):
            if 1 <= t - origin <= nlags:
                brute[t - origin - 1] += 1
    assert sch.counts == brute and sum(brute) == sum(len(v) for v in taken.values()) and sch.samples == nsamples
    sch.reset()
    assert sch.samples == 0 and not any(sch.counts) and sch.pairs() == []


def test_schedule_refuses_more_than_64_origins_before_the_device():
    from pse_amd import analyze
    for nlags, every in ((65, 1), (641, 10), (129, 2)):
        with pytest.raises(ValueError, match="more than 64"):
            analyze.MSDSchedule(nlags, every)
        with pytest.raises(ValueError, match="more than 64"):
            analyze.MSD(_NoDevice(), nlags, every)
    for nlags, every in ((0, 1), (3, 0)):
        with pytest.raises(ValueError, match="positive"):
            analyze.MSDSchedule(nlags, every)
    sch = analyze.MSDSchedule(4, 2)
    with pytest.raises(ValueError, match="no live origin"):
        sch.slot_of_lag(1)
    for _ in range(4):
        sch.sample(lambda *a: None, lambda *a: None)
    assert sch.slot_of_lag(1) == 1 and sch.slot_of_lag(3) == 0            # sample 3: origins 0 (slot 0) and 2 (slot 1)
    assert sch.live == {0: 0, 1: 2}                                       # what each slot holds: the sample stored there
    sch.sample(lambda *a: None, lambda *a: None)                          # sample 4 is an origin: slot 0 is overwritten
    assert sch.live == {0: 4, 1: 2}
    sch.reset()
    assert sch.live == {} and sch.samples == 0                            # after a reset no slot holds an origin of this series
    sch.sample(lambda *a: None, lambda *a: None)
    assert sch.live == {0: 0}
    with pytest.raises(ValueError, match="no live origin"):
        sch.slot_of_lag(2)


def test_moments_of_sums():
    from pse_amd import analyze
    sums = np.zeros((2, 2, 10))
    sums[0, 0], sums[0, 1], sums[1, 1] = 6.0, 4.0, 8.0
    m = analyze.moments_of_sums(sums, [2, 0], [3, 1])
    assert np.array_equal(m[0], np.full(10, 10.0 / 8.0)) and np.all(np.isnan(m[1]))
    assert np.array_equal(analyze.moments_of_sums(sums, [2, 4], [3, 1], 1), np.stack([np.full(10, 2.0), np.full(10, 2.0)]))
    assert np.all(np.isnan(analyze.moments_of_sums(sums, [2, 4], [3, 0], 1)))


# ---- System.tilt_flips ------------------------------------------------------------------------------------------------------------

def test_flip_count_of_a_tilt_change():
    """A System needs a device for its arrays, so the arithmetic of _set_tilt is a pure helper."""
    from pse_amd import system
    assert system.flips_between(0.5, -0.5) == 1 and system.flips_between(-0.5, 0.5) == -1
    assert system.flips_between(0.4375, -0.5) == 1 and system.flips_between(0.49, -0.49) == 1
    for old, new in ((0.0, 0.0625), (0.4375, 0.5), (-0.5, -0.4375), (0.25, -0.125), (0.0, 0.0)):
        assert system.flips_between(old, new) == 0
    xy, flips, strain = 0.0, 0, 0.0
    for _ in range(100):                                   # a steady shear: the strain is the tilt without the flips
        new = xy + 0.0625
        new = new - 1.0 if new > 0.5 else new
        flips += system.flips_between(xy, new)
        xy, strain = new, strain + 0.0625
        assert xy + flips == strain
    assert flips == 6
    assert isinstance(system.flips_between(0.5, -0.5), int)


# ---- the five entry points on the device stand-in -------------------------------------------------------------------------------------

MSD_NAMES = ("pse_msd_create", "pse_msd_destroy", "pse_msd_store", "pse_msd_accumulate", "pse_msd_displacement")


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """The host side of the library over the device stand-in of the sanitizer build, here without a sanitizer: its pse_create runs
    the real parameter rule and its pse_msd_* entry points the real validators."""
    from pse_amd import _lib
    csrc = os.path.join(ROOT, "pse_amd", "csrc")
    out = str(tmp_path_factory.mktemp("stub") / "libpse_stub.so")
    subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(csrc, "pse_params.cpp"), os.path.join(csrc, "pse_host_api.cpp"), os.path.join(csrc, "asan_stub.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    for name in ("pse_create", "pse_destroy", "pse_last_error") + MSD_NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


def stub_handle(stub, n_max, L=20.0, **kw):
    from pse_amd._lib import pse_params
    p = pse_params()
    p.n_max, p.Lx, p.Ly, p.Lz, p.xy = n_max, L, L, L, 0.0
    p.xi, p.error, p.max_strain, p.seed = 0.5, 1e-3, 0.5, 1
    p.Nx = p.Ny = p.Nz = 0
    p.P, p.rcut, p.device, p.n_slabs, p.slab_rank = 0, 0.0, -1, 1, 0
    for k, v in kw.items():
        setattr(p, k, v)
    h = ctypes.c_void_p()
    assert stub.pse_create(ctypes.byref(p), ctypes.byref(h)) == 0, stub.pse_last_error()
    return h


def ints(*v):
    return np.array(v, dtype=np.int32)


def test_refusals_of_the_five_entry_points_in_the_stated_order(stub):
    n = 6
    h = stub_handle(stub, n)
    good = dict(n=n, types=np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32), ntypes=2, norigins=4)

    def create(hh=h, with_out=True, **kw):
        a = dict(good, **kw)
        out = ctypes.c_void_p(12345)
        rc = stub.pse_msd_create(hh, a["n"], vp(a["types"]), a["ntypes"], a["norigins"], ctypes.byref(out) if with_out else None)
        return rc, out

    def refused(word, **kw):
        rc, out = create(**kw)
        msg = stub.pse_last_error().decode()
        assert rc == INVALID and word in msg and "pse_msd_create" in msg, (word, msg)
        assert not out.value or not kw.get("with_out", True)                   # *out is null after a refusal

    bad_type = np.array([0, 1, 1, 2, 1, 0], dtype=np.uint32)
    # every refusal with a LATER fault planted next to it: the earlier one is what is reported
    refused("null out", with_out=False, hh=None)
    refused("null handle", hh=None, n=0)
    refused("n = 0", n=0, ntypes=0)
    refused("n = 7", n=7, ntypes=9, types=None)
    refused("ntypes = 0", ntypes=0, norigins=0)
    refused("ntypes = 9", ntypes=9, norigins=65)
    refused("norigins = 0", norigins=0, types=bad_type)
    refused("norigins = 65", norigins=65, types=bad_type)
    refused("norigins = -1", norigins=-1)
    refused("type 2", types=bad_type)
    refused("particle 1 has type 1", ntypes=1)
    slab = stub_handle(stub, n, L=40.0, n_slabs=2, slab_rank=0, Nx=48, Ny=48, Nz=48)
    made = []
    for kw in (dict(), dict(norigins=64, ntypes=8), dict(types=None, ntypes=1, norigins=1), dict(hh=slab), dict(n=1)):
        rc, m = create(**kw)
        assert rc == 0 and m.value, (kw, stub.pse_last_error())
        made.append(m)
    m = made[0]

    # Any non-null, 8-byte aligned address will do for the device arrays: the stand-in reads none of them
    buf = np.zeros(8)
    X, odd = vp(buf), ctypes.c_void_p(buf.ctypes.data + 4)
    nan, inf = float("nan"), float("inf")

    def check(who, rc, word):
        msg = stub.pse_last_error().decode()
        assert (rc == 0 and word is None) or (rc == INVALID and word in msg and who in msg), (who, word, rc, msg)

    def store(word, mm=m, slot=0, pos=X, image=X, N=n, strain=0.25):
        check("pse_msd_store", stub.pse_msd_store(mm, slot, pos, image, None, N, strain), word)

    def disp(word, mm=m, slot=0, pos=X, image=X, N=n, strain=0.25, out=X):
        check("pse_msd_displacement", stub.pse_msd_displacement(mm, slot, pos, image, None, N, strain, out), word)

    def acc(word, mm=m, pos=X, image=X, N=n, strain=0.25, npairs=2, slots=ints(0, 2), rows=ints(1, 0), nrows=3, sums=X):
        check("pse_msd_accumulate", stub.pse_msd_accumulate(mm, pos, image, None, N, strain, npairs, vp(slots), vp(rows), nrows, sums), word)

    # nothing is stored yet: displacement and accumulate refuse every slot, after everything that comes before
    disp("slot 0 was never stored", out=None)
    acc("slot 0, which was never stored", rows=ints(5, 5), sums=None)
    for f in (store, disp):
        f("null displacement object", mm=None, slot=-1)
        f("slot = -1", slot=-1, N=0)
        f("slot = 4", slot=4, N=0)
        f("N = 0", N=0, pos=None)
        f("N = 7", N=n + 1, pos=None)
        f("null pos", pos=None, image=None)
        f("null image", image=None, strain=nan)
        f("strain = nan", strain=nan)
        f("strain = inf", strain=inf)
        f("strain = -inf", strain=-inf)
    store(None)
    store(None, slot=2, strain=-7.5, N=1)
    disp("strain = nan", strain=nan, slot=1, out=None)         # behind the shared checks:
    disp("slot 1 was never stored", slot=1, out=None)
    disp("null out", out=None)
    disp("8-byte aligned", out=odd)
    disp(None)
    disp(None, slot=2)

    acc("null displacement object", mm=None, N=0)
    acc("N = 0", N=0, pos=None)
    acc("N = 7", N=n + 1, pos=None)
    acc("null pos", pos=None, image=None)
    acc("null image", image=None, strain=inf)
    acc("strain = inf", strain=inf, npairs=0)
    acc("npairs = 0", npairs=0, slots=None)
    acc("npairs = 65", npairs=65, slots=None)
    acc("null slots_host", slots=None, rows=None)
    acc("null rows_host", rows=None, nrows=0)
    acc("nrows = 0", nrows=0, slots=ints(0, 4))
    acc("slot 4 outside", slots=ints(0, 4), rows=ints(7, 7))
    acc("slot -1 outside", slots=ints(-1, 1))
    acc("slot 1, which was never stored", slots=ints(0, 1), rows=ints(3, 0))
    acc("slot 3, which was never stored", slots=ints(3, 9), npairs=1, rows=ints(3, 0))
    acc("row 3 outside", rows=ints(3, 3))
    acc("row -1 outside", rows=ints(0, -1), sums=None)
    acc("both name the row 1", rows=ints(1, 1), sums=None)
    acc("null sums", sums=None)
    acc("8-byte aligned", sums=odd)
    acc(None)
    acc(None, npairs=1, slots=ints(2), rows=ints(2))
    acc(None, slots=ints(2, 0), rows=ints(0, 2), N=1)
    acc(None, slots=ints(0, 0), rows=ints(0, 1))               # one slot into two rows is allowed
    # 64 pairs on an object of 64 origins
    big = made[1]
    for s in range(64):
        store(None, mm=big, slot=s)
    acc(None, mm=big, npairs=64, slots=ints(*range(64)), rows=ints(*reversed(range(64))), nrows=64)
    acc("both name the row 5", mm=big, npairs=64, slots=ints(*range(64)), rows=ints(*([5] + list(range(1, 63)) + [5])), nrows=64)
    for g in made[1:3]:
        assert stub.pse_msd_destroy(g) == 0
    assert stub.pse_msd_destroy(None) == 0
    for hh in (h, slab):                                                       # the objects still alive go with their handle
        assert stub.pse_destroy(hh) == 0


# ---- what the Python layers check before the device is touched -------------------------------------------------------------------

class _NoDevice:
    """Stands where the integrator (or the engine) belongs: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the integrator was used ({name}) before the arguments were checked")


def esc(word):
    return word.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")


def test_python_argument_checks_come_before_the_device():
    from pse_amd import analyze, engine
    named = ["A", "B", "B", "A"]
    for word, kw in [("more than 64", dict(nlags=65)), ("more than 64", dict(nlags=130, origin_every=2)), ("positive", dict(nlags=0)),
                     ("positive", dict(nlags=4, origin_every=0)), ("outside [1, 8]", dict(nlags=4, types=[0, 8])),
                     ("non-negative", dict(nlags=4, types=[0, -1])), ("type_names", dict(nlags=4, types=named)),
                     ("unknown type name 'C'", dict(nlags=4, types=["A", "C"], type_names=["A", "B"])),
                     ("one type", dict(nlags=4, type_names=["A", "B"])), ("period", dict(nlags=4, period=0))]:
        with pytest.raises(ValueError, match=esc(word)):
            analyze.MSD(_NoDevice(), **kw)
    sch, ty, ntypes, names, period = analyze._msd_analyzer_arguments(640, 10, named, ["A", "B", "C"], 25)
    assert (sch.nlags, sch.origin_every, sch.norigins) == (640, 10, 64) and ty.tolist() == [0, 1, 1, 0] and ty.dtype == np.uint32
    assert (ntypes, names, period) == (3, ["A", "B", "C"], 25)
    for word, args in (("norigins = 0", (None, 1, 0)), ("norigins = 65", (None, 1, 65)), ("outside [1, 8]", (None, 9, 4)),
                       ("type 2 >= ntypes = 2", ([0, 2], 2, 4))):
        with pytest.raises(ValueError, match=esc(word)):
            engine.DisplacementOrigins(_NoDevice(), *args)
    for word, args in (("one length", ([0, 1], [0], 4, 4)), ("one length", ([[0]], [[0]], 4, 4)), ("one length", ([0.5], [0], 4, 4)),
                       ("0 pairs", ([], [], 4, 4)), ("65 pairs", (list(range(65)), list(range(65)), 80, 80)),
                       ("slot outside [0, 4)", ([0, 4], [0, 1], 4, 4)), ("slot outside", ([-1], [0], 4, 4)),
                       ("row outside [0, 3)", ([0, 1], [0, 3], 4, 3)), ("row twice", ([0, 1], [2, 2], 4, 4))):
        with pytest.raises(ValueError, match=esc(word)):
            engine._msd_pairs(*args)
    s, r = engine._msd_pairs([3, 0], (1, 0), 4, 2)
    assert s.dtype == r.dtype == np.int32 and s.tolist() == [3, 0] and r.tolist() == [1, 0]
    with pytest.raises(ValueError, match="not finite"):
        engine._finite(float("nan"), "strain")
    with pytest.raises(ValueError, match="not finite"):
        engine._finite(float("-inf"), "strain")
    assert engine._finite(2, "strain") == 2.0
