"""CPU tests of the pair exclusions that need no device: pse_host_exclusion_rows, the host builder of the per-particle rows an
exclusion object stores, through ctypes against the NumPy restatement of tests/exclusion_ref.py (offsets, both directions, rows
sorted, duplicates collapsed, empty rows, output that depends on the pair SET only, every refusal); the O(N^2) reference the GPU
tests compare to (tests/exclusion_ref.py) against the references of the plain passes; and the set construction of
forces.Exclusions.from_topology (forces.exclusion_pairs) on a toy of three short chains."""
import ctypes

import numpy as np
import pytest

import exclusion_ref as xr
import pair_table_ref
import pair_virial_ref

INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from pse_amd import build, _lib
    build.build_lib()
    return _lib.load()


def rows(lib, n, pairs):
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    npairs = len(pairs)
    off = np.full(n + 1, -7, dtype=np.int32)
    ent = np.full(2 * npairs, 0xFFFFFFFF, dtype=np.uint32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731
    rc = lib.pse_host_exclusion_rows(n, npairs, vp(pairs), vp(off), vp(ent))
    assert rc == 0, lib.pse_last_error()
    assert np.all(ent[off[-1]:] == 0xFFFFFFFF)             # nothing is written behind the entries kept
    return off, ent[:off[-1]]


def random_list(n, npairs, seed):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, n, npairs)
    j = (i + rng.integers(1, n, npairs)) % n
    return np.stack([i, j], axis=1)


@pytest.mark.parametrize("n,npairs", [(2, 1), (5, 3), (64, 200), (257, 256), (1000, 5000)])
def test_rows_match_the_numpy_restatement(lib, n, npairs):
    pairs = random_list(n, npairs, seed=n + npairs)
    off, ent = rows(lib, n, pairs)
    roff, rent = xr.rows_numpy(n, pairs)
    distinct = len({(min(a, b), max(a, b)) for a, b in pairs.tolist()})
    assert np.array_equal(off, roff) and off[0] == 0 and off[-1] == 2 * distinct <= 2 * npairs
    assert np.array_equal(ent, rent)
    if (n, npairs) in ((64, 200), (1000, 5000)):
        assert distinct < npairs                           # the random list does hold duplicates
    for i in range(n):                                     # sorted, no duplicates, never i itself
        row = ent[off[i]:off[i + 1]].astype(np.int64)
        assert np.all(np.diff(row) > 0) and i not in row


def test_a_set_both_directions_an_empty_row_and_the_last_particle(lib):
    # the pair (1, 4) is listed three times, one of them swapped: one entry in each of the two rows; particle 3 is in no pair;
    # particle 5 is the last one
    pairs = [[4, 1], [0, 1], [1, 4], [5, 0], [1, 4], [2, 1]]
    off, ent = rows(lib, 6, pairs)
    assert off.tolist() == [0, 2, 5, 6, 6, 7, 8]
    row = lambda i: ent[off[i]:off[i + 1]].tolist()         # noqa: E731
    assert row(0) == [1, 5]
    assert row(1) == [0, 2, 4]
    assert row(2) == [1]
    assert row(3) == []
    assert row(4) == [1]
    assert row(5) == [0]
    for i in range(6):
        for j in row(i):
            assert row(j).count(i) == 1


def test_output_depends_on_the_pair_set_only(lib):
    n = 300
    pairs = random_list(n, 900, seed=9)
    ref = rows(lib, n, pairs)
    rng = np.random.default_rng(2)
    for trial in range(3):
        p = np.concatenate([pairs, pairs[rng.integers(0, len(pairs), 50)]])      # some pairs once more
        p = p[rng.permutation(len(p))]
        flip = rng.uniform(size=len(p)) < 0.5
        p[flip] = p[flip, ::-1]
        got = rows(lib, n, p)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_invalid_arguments(lib):
    good = np.array([[0, 1]], dtype=np.uint32)
    off, ent = np.zeros(4, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)      # noqa: E731

    def bad(n, npairs, pairs, off_, ent_, word):
        assert lib.pse_host_exclusion_rows(n, npairs, vp(pairs), vp(off_), vp(ent_)) == INVALID
        msg = lib.pse_last_error().decode()
        assert word in msg and "pse_host_exclusion_rows" in msg, msg

    bad(3, 1, None, off, ent, "null")
    bad(3, 1, good, None, ent, "null")
    bad(3, 1, good, off, None, "null")
    bad(0, 1, good, off, ent, "n = 0")
    bad(3, 0, good, off, ent, "npairs = 0")
    bad(3, (1 << 30) + 1, good, off, ent, "npairs = 1073741825")
    bad(3, 1, np.array([[0, 3]], dtype=np.uint32), off, ent, "(0, 3)")
    bad(3, 1, np.array([[3, 0]], dtype=np.uint32), off, ent, "(3, 0)")
    bad(3, 1, np.array([[2, 2]], dtype=np.uint32), off, ent, "particle 2")
    assert not off.any() and not ent.any()                 # a refused call writes nothing


# ---- the reference of the GPU tests ---------------------------------------------------------------------------------------------

BOX = (14.0, 11.0, 17.0, 0.3)
MORSE = dict(D=5.0, alpha=2.0, r0=1.5)


def _table_case(oracle):
    pos = pair_virial_ref.random_points(200, BOX, seed=11)
    table = pair_table_ref.morse_table(rmin=0.7, rmax=3.0, width=1000, **MORSE)
    return pos, table, 0.7, 3.0


def test_reference_without_effective_exclusions_is_the_plain_reference(oracle):
    pos, table, rmin, rmax = _table_case(oracle)
    obs, F = pair_table_ref.pair_observables(pos, BOX, table, rmin, rmax, oracle)
    assert obs[7] > 20
    i, j = pair_table_ref.pair_terms(pos, BOX, table, rmin, rmax, oracle)[:2]
    acting = set(zip(i.tolist(), j.tolist()))
    far = [p for p in random_list(200, 400, seed=3).tolist() if (min(p), max(p)) not in acting]
    assert len(far) > 300
    for excl in (None, np.zeros((0, 2), dtype=np.int64), np.array(far)):
        o, f, nex = xr.table_observables(pos, BOX, table, rmin, rmax, oracle, excl)
        assert nex == 0 and np.array_equal(o, obs) and np.array_equal(f, F)
    robs, rF = pair_virial_ref.pair_observables(pos, BOX, 40.0, 2.0, oracle)
    ri, rj = pair_virial_ref.pair_terms(pos, BOX, 40.0, 2.0, oracle)[:2]
    racting = set(zip(ri.tolist(), rj.tolist()))
    rfar = np.array([p for p in far if (min(p), max(p)) not in racting])
    assert robs[7] > 5
    for excl in (None, rfar):
        o, f, nex = xr.repulsion_observables(pos, BOX, 40.0, 2.0, oracle, excl)
        assert nex == 0 and np.array_equal(o, robs) and np.array_equal(f, rF)


def test_reference_excluded_plus_kept_is_everything(oracle):
    pos, table, rmin, rmax = _table_case(oracle)
    obs, F = pair_table_ref.pair_observables(pos, BOX, table, rmin, rmax, oracle)
    i, j = pair_table_ref.pair_terms(pos, BOX, table, rmin, rmax, oracle)[:2]
    pick = np.random.default_rng(4).uniform(size=len(i)) < 0.5
    excl = np.stack([j[pick], i[pick]], axis=1)            # (larger, smaller): the order of a pair's members does not matter
    kept, Fk, nex = xr.table_observables(pos, BOX, table, rmin, rmax, oracle, excl)
    gone, Fg, nex2 = xr.table_observables(pos, BOX, table, rmin, rmax, oracle, excl, keep=False)
    assert nex == nex2 == int(pick.sum()) and 20 < nex < len(i) - 20
    assert kept[7] + gone[7] == obs[7] and kept[7] == len(i) - nex
    tol = 1e-12 * max(1.0, np.abs(obs).max())
    assert np.abs(kept + gone - obs).max() <= tol and np.abs(Fk + Fg - F).max() <= 1e-12 * max(1.0, np.abs(F).max())
    assert np.abs(gone[:7]).max() > 1.0                    # the excluded half is not negligible
    # a group: the rows of pos are the caller's particles ids[...]; the same index pairs are excluded
    ids = np.arange(0, 400, 2)
    kept2, Fk2, nex3 = xr.table_observables(pos, BOX, table, rmin, rmax, oracle, 2 * excl, ids=ids)
    assert nex3 == nex and np.array_equal(kept2, kept) and np.array_equal(Fk2, Fk)
    # ... and read as row indices where caller indices belong, other pairs would go
    assert not np.array_equal(xr.table_observables(pos, BOX, table, rmin, rmax, oracle, excl, ids=ids)[0], kept)
    # the repulsion
    ri, rj = pair_virial_ref.pair_terms(pos, BOX, 40.0, 2.0, oracle)[:2]
    rex = np.stack([ri[::2], rj[::2]], axis=1)
    robs, rF = pair_virial_ref.pair_observables(pos, BOX, 40.0, 2.0, oracle)
    a, Fa, na = xr.repulsion_observables(pos, BOX, 40.0, 2.0, oracle, rex)
    b, Fb, _ = xr.repulsion_observables(pos, BOX, 40.0, 2.0, oracle, rex, keep=False)
    assert na == len(rex) > 2 and a[7] + b[7] == robs[7]
    assert np.abs(a + b - robs).max() <= 1e-12 * max(1.0, np.abs(robs).max()) and np.abs(Fa + Fb - rF).max() <= 1e-12 * max(1.0, np.abs(rF).max())


# ---- forces.exclusion_pairs: the sets of Exclusions.from_topology ------------------------------------------------------------------

def _toy():
    """Three chains of 5, 4 and 3 beads, numbered consecutively: bonds, angles and dihedrals along each."""
    bonds, angles, dihedrals, first = [], [], [], 0
    for beads in (5, 4, 3):
        b = np.arange(first, first + beads)
        bonds += [[b[q], b[q + 1]] for q in range(beads - 1)]
        angles += [[b[q], b[q + 1], b[q + 2]] for q in range(beads - 2)]
        dihedrals += [[b[q], b[q + 1], b[q + 2], b[q + 3]] for q in range(beads - 3)]
        first += beads
    return np.array(bonds), np.array(angles), np.array(dihedrals)


def test_from_topology_sets_on_three_chains():
    from pse_amd.forces import exclusion_pairs
    bonds, angles, dihedrals = _toy()
    as_set = lambda a: {tuple(p) for p in a.tolist()}      # noqa: E731
    b12 = {(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 8), (9, 10), (10, 11)}
    b13 = {(0, 2), (1, 3), (2, 4), (5, 7), (6, 8), (9, 11)}
    b14 = {(0, 3), (1, 4), (5, 8)}
    got = exclusion_pairs(bonds=bonds)
    assert got.shape == (9, 2) and got.dtype == np.int64 and as_set(got) == b12
    assert as_set(exclusion_pairs(angles=angles)) == b13                   # the two ENDS of an angle, not its vertex
    assert as_set(exclusion_pairs(dihedrals=dihedrals)) == b14
    assert as_set(exclusion_pairs(bonds, angles)) == b12 | b13
    allp = exclusion_pairs(bonds, angles, dihedrals)
    assert as_set(allp) == b12 | b13 | b14 and len(allp) == 18
    # a union without duplicates, whatever the order and the direction: reversed entries, and every bond once more as an "angle end"
    dup = exclusion_pairs(bonds[::-1, ::-1], np.concatenate([angles, np.stack([bonds[:, 1], bonds[:, 0], bonds[:, 0]], axis=1)]), dihedrals[:, ::-1])
    assert np.array_equal(dup, allp)
    assert np.all(allp[:, 0] < allp[:, 1]) and np.array_equal(allp, np.unique(allp, axis=0))
    with pytest.raises(ValueError, match="at least one"):
        exclusion_pairs()
    for bad in (dict(bonds=angles), dict(angles=bonds), dict(dihedrals=angles), dict(bonds=bonds.astype(float))):
        with pytest.raises(ValueError):
            exclusion_pairs(**bad)
