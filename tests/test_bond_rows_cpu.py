"""CPU tests of pse_host_bond_rows, the host builder of the per-particle rows a bond object stores, through ctypes against a NumPy
restatement: offsets, both directions, rows sorted by (partner, type), duplicates kept, empty rows, and output that depends on the
bond set only -- not on the order of the list or of a bond's endpoints."""
import ctypes

import numpy as np
import pytest

INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from pse_amd import build, _lib
    build.build_lib()
    return _lib.load()


def rows(lib, n, pairs, types=None):
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    nb = len(pairs)
    t = None if types is None else np.ascontiguousarray(types, dtype=np.uint32)
    off = np.full(n + 1, -7, dtype=np.int32)
    ent = np.full((2 * nb, 2), 0xFFFFFFFF, dtype=np.uint32)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rc = lib.pse_host_bond_rows(n, nb, vp(pairs), vp(t), vp(off), vp(ent))
    assert rc == 0, lib.pse_last_error()
    return off, ent


def rows_numpy(n, pairs, types=None):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    t = np.zeros(len(pairs), dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    owner = np.concatenate([pairs[:, 0], pairs[:, 1]])
    partner = np.concatenate([pairs[:, 1], pairs[:, 0]])
    tt = np.concatenate([t, t])
    o = np.lexsort((tt, partner, owner))
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))])
    return off, np.stack([partner[o], tt[o]], axis=1)


def random_list(n, nb, ntypes, seed):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, n, nb)
    j = (i + rng.integers(1, n, nb)) % n
    return np.stack([i, j], axis=1), rng.integers(0, ntypes, nb)


@pytest.mark.parametrize("n,nb,ntypes", [(2, 1, 1), (5, 3, 2), (64, 200, 3), (257, 256, 1), (1000, 5000, 64)])
def test_rows_match_the_numpy_restatement(lib, n, nb, ntypes):
    pairs, types = random_list(n, nb, ntypes, seed=n + nb)
    off, ent = rows(lib, n, pairs, types)
    roff, rent = rows_numpy(n, pairs, types)
    assert np.array_equal(off, roff) and off[0] == 0 and off[-1] == 2 * nb
    assert np.array_equal(ent, rent)
    # types == NULL: all type 0
    off0, ent0 = rows(lib, n, pairs)
    assert np.array_equal(off0, roff) and np.array_equal(ent0, rows_numpy(n, pairs)[1]) and not ent0[:, 1].any()


def test_both_directions_sorted_rows_duplicates_and_empty_rows(lib):
    # particle 3 is unbonded, the bond (1, 4) is listed three times (once swapped, once with another type), particle 5 is last
    pairs = [[4, 1], [0, 1], [1, 4], [5, 0], [1, 4], [2, 1]]
    types = [1, 0, 0, 2, 1, 0]
    off, ent = rows(lib, 6, pairs, types)
    assert off.tolist() == [0, 2, 7, 8, 8, 11, 12]
    row = lambda i: [tuple(e) for e in ent[off[i]:off[i + 1]].tolist()]
    assert row(0) == [(1, 0), (5, 2)]
    assert row(1) == [(0, 0), (2, 0), (4, 0), (4, 1), (4, 1)]          # sorted by partner, then type; duplicates kept
    assert row(2) == [(1, 0)]
    assert row(3) == []                                                # unbonded: an empty row
    assert row(4) == [(1, 0), (1, 1), (1, 1)]
    assert row(5) == [(0, 2)]
    # both directions: (j, t) in row i as often as (i, t) in row j
    for i in range(6):
        for j, t in row(i):
            assert row(j).count((i, t)) == row(i).count((j, t))


def test_output_depends_on_the_bond_set_only(lib):
    n = 300
    pairs, types = random_list(n, 900, 4, seed=9)
    pairs[100:120] = pairs[:20]; types[100:120] = types[:20]           # some duplicates
    ref = rows(lib, n, pairs, types)
    rng = np.random.default_rng(2)
    for trial in range(3):
        o = rng.permutation(len(pairs))
        p = pairs[o].copy()
        flip = rng.uniform(size=len(p)) < 0.5
        p[flip] = p[flip, ::-1]
        got = rows(lib, n, p, types[o])
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_invalid_arguments(lib):
    good = np.array([[0, 1]], dtype=np.uint32)
    off, ent = np.zeros(4, dtype=np.int32), np.zeros((2, 2), dtype=np.uint32)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def bad(n, nb, pairs, off_, ent_, word):
        assert lib.pse_host_bond_rows(n, nb, vp(pairs), None, vp(off_), vp(ent_)) == INVALID
        msg = lib.pse_last_error().decode()
        assert word in msg, msg

    bad(3, 1, None, off, ent, "null")
    bad(3, 1, good, None, ent, "null")
    bad(3, 1, good, off, None, "null")
    bad(0, 1, good, off, ent, "n = 0")
    bad(3, 0, good, off, ent, "nbonds = 0")
    bad(3, (1 << 30) + 1, good, off, ent, "nbonds = 1073741825")
    bad(3, 1, np.array([[0, 3]], dtype=np.uint32), off, ent, "(0, 3)")
    bad(3, 1, np.array([[2, 2]], dtype=np.uint32), off, ent, "particle 2")
