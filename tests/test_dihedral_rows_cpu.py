"""CPU tests of pse_host_dihedral_rows, the host builder of the per-particle rows a dihedral object stores, through ctypes against a
NumPy restatement: offsets, every dihedral in the rows of all four of its particles, stored as (l, k, j, i) where l < i, rows
sorted by (i, j, k, l, type), the types in the parallel section behind the quadruples, duplicates kept, empty rows, output that
depends on the dihedral set only -- not on the order of the list or on the direction a quadruple is written in -- and every refusal
with its message."""
import ctypes

import numpy as np
import pytest

INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from pse_amd import build, _lib
    build.build_lib()
    return _lib.load()


def rows(lib, n, quads, types=None):
    """(off, ent): ent (4 nd, 5) = the quadruple of the first section and the type of the second, side by side."""
    quads = np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1, 4)
    nd = len(quads)
    t = None if types is None else np.ascontiguousarray(types, dtype=np.uint32)
    off = np.full(n + 1, -7, dtype=np.int32)
    buf = np.full(20 * nd + 4, 0xFFFFFFFF, dtype=np.uint32)          # four words behind the end: they must stay as they are
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rc = lib.pse_host_dihedral_rows(n, nd, vp(quads), vp(t), vp(off), vp(buf))
    assert rc == 0, lib.pse_last_error()
    assert np.all(buf[20 * nd:] == 0xFFFFFFFF)
    return off, np.concatenate([buf[:16 * nd].reshape(-1, 4), buf[16 * nd:20 * nd, None]], axis=1)


def canon(quads, types=None):
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    t = np.zeros(len(q), dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    q = np.where((q[:, 3] < q[:, 0])[:, None], q[:, ::-1], q)
    return np.concatenate([q, t[:, None]], axis=1)


def rows_numpy(n, quads, types=None):
    c = canon(quads, types)
    owner = np.concatenate([c[:, 0], c[:, 1], c[:, 2], c[:, 3]])
    ent = np.concatenate([c, c, c, c])
    o = np.lexsort((ent[:, 4], ent[:, 3], ent[:, 2], ent[:, 1], ent[:, 0], owner))
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))])
    return off, ent[o]


def random_list(n, nd, ntypes, seed):
    rng = np.random.default_rng(seed)
    q = np.array([rng.choice(n, 4, replace=False) for _ in range(nd)])
    return q, rng.integers(0, ntypes, nd)


@pytest.mark.parametrize("n,nd,ntypes", [(4, 1, 1), (6, 5, 2), (64, 200, 3), (257, 255, 1), (1000, 3000, 64)])
def test_rows_match_the_numpy_restatement(lib, n, nd, ntypes):
    quads, types = random_list(n, nd, ntypes, seed=n + nd)
    off, ent = rows(lib, n, quads, types)
    roff, rent = rows_numpy(n, quads, types)
    assert np.array_equal(off, roff) and off[0] == 0 and off[-1] == 4 * nd
    assert np.array_equal(ent, rent)
    assert np.all(ent[:, 0] < ent[:, 3])                                  # the smaller end first
    # types == NULL: all type 0
    off0, ent0 = rows(lib, n, quads)
    assert np.array_equal(off0, roff) and np.array_equal(ent0, rows_numpy(n, quads)[1]) and not ent0[:, 4].any()


def test_every_dihedral_is_in_exactly_four_rows(lib):
    """... those of its four particles, once per listing, and the row's owner is one of the entry's members: its role."""
    n = 120
    quads, types = random_list(n, 500, 3, seed=4)
    quads[50:60] = quads[:10]; types[50:60] = types[:10]                   # some duplicates
    off, ent = rows(lib, n, quads, types)
    owner = np.repeat(np.arange(n), np.diff(off))
    assert np.all((ent[:, :4] == owner[:, None]).sum(axis=1) == 1)
    listed, times = np.unique(canon(quads, types), axis=0, return_counts=True)
    stored, stimes = np.unique(ent.astype(np.int64), axis=0, return_counts=True)
    assert np.array_equal(listed, stored) and np.array_equal(stimes, 4 * times) and times.max() >= 2
    for q, m in zip(listed, times):                                        # ... and in the row of each member, m times
        for p in q[:4]:
            row = ent[off[p]:off[p + 1]].astype(np.int64)
            assert int((row == q).all(axis=1).sum()) == m


def test_roles_orientation_sorted_rows_duplicates_and_empty_rows(lib):
    # particle 3 is in no dihedral; 4-1-0-2 is listed three times (once reversed, once with another type); 5-0-2-1 is stored reversed
    quads = [[4, 1, 0, 2], [0, 2, 1, 5], [2, 0, 1, 4], [5, 0, 2, 1], [4, 1, 0, 2]]
    types = [1, 0, 0, 2, 1]
    off, ent = rows(lib, 6, quads, types)
    assert off.tolist() == [0, 5, 10, 15, 15, 18, 20]
    row = lambda p: [tuple(e) for e in ent[off[p]:off[p + 1]].tolist()]
    every = [(0, 2, 1, 5, 0), (1, 2, 0, 5, 2), (2, 0, 1, 4, 0), (2, 0, 1, 4, 1), (2, 0, 1, 4, 1)]   # sorted by (i, j, k, l, type); duplicates kept
    assert row(0) == every and row(1) == every and row(2) == every       # an end of one, inner members of the others
    assert row(3) == []
    assert row(4) == every[2:]
    assert row(5) == every[:2]
    # (1, 2, 0, 5) is not (5, 0, 2, 1) with sorted members: the orientation is a reversal, the inner pair goes with it
    assert (5, 0, 2, 1, 2) not in every and (1, 0, 2, 5, 2) not in every


def test_output_depends_on_the_dihedral_set_only(lib):
    n = 300
    quads, types = random_list(n, 900, 4, seed=9)
    quads[100:120] = quads[:20]; types[100:120] = types[:20]               # some duplicates
    ref = rows(lib, n, quads, types)
    rng = np.random.default_rng(2)
    for trial in range(3):
        o = rng.permutation(len(quads))
        t = quads[o].copy()
        flip = rng.uniform(size=len(t)) < 0.5
        t[flip] = t[flip, ::-1]
        got = rows(lib, n, t, types[o])
        assert flip.any() and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_invalid_arguments(lib):
    good = np.array([[0, 1, 2, 3]], dtype=np.uint32)
    off, ent = np.zeros(6, dtype=np.int32), np.zeros(20, dtype=np.uint32)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def bad(n, nd, quads, off_, ent_, word):
        assert lib.pse_host_dihedral_rows(n, nd, vp(quads), None, vp(off_), vp(ent_)) == INVALID
        msg = lib.pse_last_error().decode()
        assert word in msg, msg

    bad(5, 1, None, off, ent, "null")
    bad(5, 1, good, None, ent, "null")
    bad(5, 1, good, off, None, "null")
    bad(0, 1, good, off, ent, "n = 0")
    bad(5, 0, good, off, ent, "ndihedrals = 0")
    bad(5, (1 << 28) + 1, good, off, ent, "ndihedrals = 268435457")
    u = lambda v: np.array([v], dtype=np.uint32)
    for q in ([5, 0, 1, 2], [0, 5, 1, 2], [0, 1, 5, 2], [0, 1, 2, 5]):
        bad(5, 1, u(q), off, ent, "(%d, %d, %d, %d) has an index >= n = 5" % tuple(q))
    for q in ([2, 2, 1, 0], [2, 1, 2, 0], [2, 1, 0, 2], [1, 2, 2, 0], [1, 2, 0, 2], [0, 1, 2, 2]):
        bad(5, 1, u(q), off, ent, "(%d, %d, %d, %d) has two equal members" % tuple(q))
    assert lib.pse_host_dihedral_rows(5, 1, vp(good), None, vp(off), vp(ent)) == 0          # ... and works after the refusals
    assert off.tolist() == [0, 1, 2, 3, 4, 4] and ent.tolist() == [0, 1, 2, 3] * 4 + [0] * 4
