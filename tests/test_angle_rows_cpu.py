"""CPU tests of pse_host_angle_rows, the host builder of the per-particle rows an angle object stores, through ctypes against a NumPy
restatement: offsets, every angle in the rows of all three of its particles, ends canonicalised to i < k, rows sorted by
(i, j, k, type), duplicates kept, empty rows, output that depends on the angle set only -- not on the order of the list or of an
angle's ends -- and every refusal with its message."""
import ctypes

import numpy as np
import pytest

INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from pse_amd import build, _lib
    build.build_lib()
    return _lib.load()


def rows(lib, n, triples, types=None):
    triples = np.ascontiguousarray(triples, dtype=np.uint32).reshape(-1, 3)
    na = len(triples)
    t = None if types is None else np.ascontiguousarray(types, dtype=np.uint32)
    off = np.full(n + 1, -7, dtype=np.int32)
    ent = np.full((3 * na, 4), 0xFFFFFFFF, dtype=np.uint32)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rc = lib.pse_host_angle_rows(n, na, vp(triples), vp(t), vp(off), vp(ent))
    assert rc == 0, lib.pse_last_error()
    return off, ent


def rows_numpy(n, triples, types=None):
    tr = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    t = np.zeros(len(tr), dtype=np.int64) if types is None else np.asarray(types, dtype=np.int64)
    canon = np.stack([np.minimum(tr[:, 0], tr[:, 2]), tr[:, 1], np.maximum(tr[:, 0], tr[:, 2]), t], axis=1)
    owner = np.concatenate([canon[:, 0], canon[:, 1], canon[:, 2]])
    ent = np.concatenate([canon, canon, canon])
    o = np.lexsort((ent[:, 3], ent[:, 2], ent[:, 1], ent[:, 0], owner))
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))])
    return off, ent[o]


def random_list(n, na, ntypes, seed):
    rng = np.random.default_rng(seed)
    tr = np.array([rng.choice(n, 3, replace=False) for _ in range(na)])
    return tr, rng.integers(0, ntypes, na)


@pytest.mark.parametrize("n,na,ntypes", [(3, 1, 1), (5, 4, 2), (64, 200, 3), (257, 255, 1), (1000, 3000, 64)])
def test_rows_match_the_numpy_restatement(lib, n, na, ntypes):
    triples, types = random_list(n, na, ntypes, seed=n + na)
    off, ent = rows(lib, n, triples, types)
    roff, rent = rows_numpy(n, triples, types)
    assert np.array_equal(off, roff) and off[0] == 0 and off[-1] == 3 * na
    assert np.array_equal(ent, rent)
    assert np.all(ent[:, 0] < ent[:, 2])                                  # ends canonicalised
    # types == NULL: all type 0
    off0, ent0 = rows(lib, n, triples)
    assert np.array_equal(off0, roff) and np.array_equal(ent0, rows_numpy(n, triples)[1]) and not ent0[:, 3].any()


def test_every_angle_is_in_exactly_three_rows(lib):
    """... those of its three particles, once per listing, and the row's owner is one of the entry's members: its role."""
    n = 120
    triples, types = random_list(n, 500, 3, seed=4)
    triples[50:60] = triples[:10]; types[50:60] = types[:10]               # some duplicates
    off, ent = rows(lib, n, triples, types)
    owner = np.repeat(np.arange(n), np.diff(off))
    assert np.all((ent[:, 0] == owner).astype(int) + (ent[:, 1] == owner) + (ent[:, 2] == owner) == 1)
    canon = np.stack([np.minimum(triples[:, 0], triples[:, 2]), triples[:, 1],
                      np.maximum(triples[:, 0], triples[:, 2]), types], axis=1)
    listed, times = np.unique(canon, axis=0, return_counts=True)
    stored, stimes = np.unique(ent.astype(np.int64), axis=0, return_counts=True)
    assert np.array_equal(listed, stored) and np.array_equal(stimes, 3 * times) and times.max() >= 2
    for q, m in zip(listed, times):                                        # ... and in the row of each member, m times
        for p in q[:3]:
            row = ent[off[p]:off[p + 1]].astype(np.int64)
            assert int((row == q).all(axis=1).sum()) == m


def test_roles_sorted_rows_duplicates_and_empty_rows(lib):
    # particle 3 is in no angle; the angle 4-1-0 is listed three times (once with the ends swapped, once with another type)
    triples = [[4, 1, 0], [0, 2, 1], [0, 1, 4], [5, 0, 2], [4, 1, 0]]
    types = [1, 0, 0, 2, 1]
    off, ent = rows(lib, 6, triples, types)
    assert off.tolist() == [0, 5, 9, 11, 11, 14, 15]
    row = lambda p: [tuple(e) for e in ent[off[p]:off[p + 1]].tolist()]
    assert row(0) == [(0, 1, 4, 0), (0, 1, 4, 1), (0, 1, 4, 1), (0, 2, 1, 0), (2, 0, 5, 2)]    # an end, an end, the vertex
    assert row(1) == [(0, 1, 4, 0), (0, 1, 4, 1), (0, 1, 4, 1), (0, 2, 1, 0)]                 # sorted by (i, j, k, type); duplicates kept
    assert row(2) == [(0, 2, 1, 0), (2, 0, 5, 2)]
    assert row(3) == []
    assert row(4) == [(0, 1, 4, 0), (0, 1, 4, 1), (0, 1, 4, 1)]
    assert row(5) == [(2, 0, 5, 2)]


def test_output_depends_on_the_angle_set_only(lib):
    n = 300
    triples, types = random_list(n, 900, 4, seed=9)
    triples[100:120] = triples[:20]; types[100:120] = types[:20]           # some duplicates
    ref = rows(lib, n, triples, types)
    rng = np.random.default_rng(2)
    for trial in range(3):
        o = rng.permutation(len(triples))
        t = triples[o].copy()
        flip = rng.uniform(size=len(t)) < 0.5
        t[flip] = t[flip, ::-1]
        got = rows(lib, n, t, types[o])
        assert flip.any() and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_invalid_arguments(lib):
    good = np.array([[0, 1, 2]], dtype=np.uint32)
    off, ent = np.zeros(5, dtype=np.int32), np.zeros((3, 4), dtype=np.uint32)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def bad(n, na, triples, off_, ent_, word):
        assert lib.pse_host_angle_rows(n, na, vp(triples), None, vp(off_), vp(ent_)) == INVALID
        msg = lib.pse_last_error().decode()
        assert word in msg, msg

    bad(4, 1, None, off, ent, "null")
    bad(4, 1, good, None, ent, "null")
    bad(4, 1, good, off, None, "null")
    bad(0, 1, good, off, ent, "n = 0")
    bad(4, 0, good, off, ent, "nangles = 0")
    bad(4, (1 << 28) + 1, good, off, ent, "nangles = 268435457")
    u = lambda v: np.array([v], dtype=np.uint32)
    bad(4, 1, u([0, 1, 4]), off, ent, "(0, 1, 4)")
    bad(4, 1, u([0, 4, 1]), off, ent, "(0, 4, 1)")
    bad(4, 1, u([4, 0, 1]), off, ent, "(4, 0, 1)")
    bad(4, 1, u([2, 2, 1]), off, ent, "(2, 2, 1) has two equal members")
    bad(4, 1, u([1, 2, 2]), off, ent, "(1, 2, 2) has two equal members")
    bad(4, 1, u([3, 2, 3]), off, ent, "(3, 2, 3) has two equal members")
    assert lib.pse_host_angle_rows(4, 1, vp(good), None, vp(off), vp(ent)) == 0          # ... and works after the refusals
    assert off.tolist() == [0, 1, 2, 3, 3] and ent.tolist() == [[0, 1, 2, 0]] * 3
