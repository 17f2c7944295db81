"""CPU tests of the two checkers that every typed device object shares (engine._ntypes_argument, engine._types_argument), which need
no device: what they accept and return, every refusal by its text, and that each of the five _*_arguments functions built on them
reports a bad `ntypes` before a bad `types`."""
import re

import numpy as np
import pytest

from pse_amd import engine

NOT_TYPES = "types must be a non-empty 1-D array of non-negative integers, one per particle"


def test_no_types_stay_none():
    assert engine._types_argument(None, 3) is None
    assert engine._types_argument(None) is None


@pytest.mark.parametrize("types", [[0, 2, 1, 2], np.array([0, 2, 1, 2], dtype=np.int64), np.array([[0, 2], [1, 2]], dtype=np.uint8)[:, 1]],
                         ids=["list", "int64", "strided-uint8"])
def test_types_come_back_as_contiguous_uint32(types):
    out = engine._types_argument(types, 3)
    assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"] and out.ndim == 1
    assert out.tolist() == np.asarray(types).tolist()
    assert engine._types_argument(types).tolist() == out.tolist()   # (ntypes=None: any non-negative integers)


@pytest.mark.parametrize("types", [np.zeros(0, dtype=np.int64), [], np.zeros((2, 2), dtype=np.int64), np.array([0.0, 1.0]), [0, -1, 1]],
                         ids=["empty-array", "empty-list", "2-D", "float", "negative"])
def test_what_is_no_type_array_is_refused(types):
    for ntypes in (3, None):
        with pytest.raises(ValueError, match=re.escape(NOT_TYPES)):
            engine._types_argument(types, ntypes)


def test_a_type_equal_to_ntypes_is_refused():
    with pytest.raises(ValueError, match=re.escape("types holds the type 3 >= ntypes = 3")):
        engine._types_argument([0, 3, 1], 3)
    assert engine._types_argument([0, 2, 1], 3).tolist() == [0, 2, 1]
    assert engine._types_argument([0, 3, 1]).tolist() == [0, 3, 1]   # (ntypes=None: no upper limit)


def test_ntypes_within_one_and_eight():
    for ntypes in (1, 8):
        assert engine._ntypes_argument(ntypes) == ntypes
    for ntypes in (0, 9):
        with pytest.raises(ValueError, match=re.escape(f"ntypes = {ntypes} outside [1, 8]")):
            engine._ntypes_argument(ntypes)


ARGUMENTS = {"pair_hist": lambda types, ntypes: engine._pair_hist_arguments(types, ntypes, 10, 0.0, 3.0),
             "structure_factor": lambda types, ntypes: engine._structure_factor_arguments(types, ntypes, [[1, 0, 0]]),
             "msd": lambda types, ntypes: engine._msd_arguments(types, ntypes, 4),
             "cluster": lambda types, ntypes: engine._cluster_arguments(types, ntypes, 2.5),
             "bond_order": lambda types, ntypes: engine._bond_order_arguments(types, ntypes, 2.5, (4, 6))}


@pytest.mark.parametrize("name", sorted(ARGUMENTS))
@pytest.mark.parametrize("ntypes", [0, 9])
def test_bad_ntypes_is_reported_before_bad_types(name, ntypes):
    for bad in ([0, -1], np.array([0.5]), [0, 12]):
        with pytest.raises(ValueError, match=re.escape(f"ntypes = {ntypes} outside [1, 8]")):
            ARGUMENTS[name](bad, ntypes)


@pytest.mark.parametrize("name", sorted(ARGUMENTS))
def test_types_are_checked_by_every_arguments_function(name):
    with pytest.raises(ValueError, match=re.escape(NOT_TYPES)):
        ARGUMENTS[name]([0, -1], 2)
    with pytest.raises(ValueError, match=re.escape("types holds the type 2 >= ntypes = 2")):
        ARGUMENTS[name]([0, 2], 2)
    types, ntypes = ARGUMENTS[name](np.array([0, 1, 1], dtype=np.int64), 2)[:2]
    assert types.dtype == np.uint32 and types.tolist() == [0, 1, 1] and ntypes == 2
    assert ARGUMENTS[name](None, 2)[0] is None
