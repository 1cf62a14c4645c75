"""What BitSliceIndexBase.parallelTransposeWithCount (BBSI/:551-597) computes, on the CPU oracle: the reference's
sequence composed from BSI.from_columns per batch and add_reference over the batches (tests/_bsi_transpose.py)
against plain numpy at set level and against the per-key type rule."""
import numpy as np
import pytest

import _bsi
import _oracle as O
from _bsi import BSI
from _bsi_add import values_of
from _bsi_transpose import (FULL_KEY, full_case, full_keys, index_of, random_index, transpose_counts,
                            transpose_reference)


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


def _check_set_level(r, want_vals, want_counts):
    """the result against (distinct values, counts): columns, values, depth and extremes"""
    cols, counts = values_of(r)
    assert cols.tolist() == want_vals.tolist() and counts.tolist() == want_counts.tolist()
    top = int(want_counts.max()) if want_counts.size else 0
    assert r.bit_count() == top.bit_length()
    assert (r.min, r.max) == ((int(want_counts.min()), top) if want_counts.size else (0, 0))


def _check_typed_by_cardinality(r, ebm_too=True):
    """every container an array up to 4096 values and a bitmap above, none empty: bitmapOf's bytes"""
    for b in r.ba + ([r.ebm] if ebm_too else []):
        assert b == O.from_values(O.to_values(b))


def test_known_answer():
    """BufferBSITest.testTransposeWithCount (:381-407)"""
    x = np.arange(1, 100)
    o = BSI.from_columns(x, np.where(x <= 30, 1, np.where(x <= 60, 2, 3)))
    r = transpose_reference(o, None, 2)
    assert values_of(r)[0].tolist() == [1, 2, 3] and values_of(r)[1].tolist() == [30, 30, 39]
    assert (r.bit_count(), r.min, r.max) == (6, 30, 39)
    _check_typed_by_cardinality(r)


@pytest.mark.parametrize("number", [1, 2, 3, 4, 5, 6])
def test_full_key_cases(number):
    cols, vals, parallelism, size, run = full_case(number)
    o = index_of(cols, vals)
    r = transpose_reference(o, None, parallelism)
    assert full_keys(o, None, parallelism) == {FULL_KEY: run}
    assert _kinds(r.ebm) == ((0, 0, 1) if run else (0, 1, 0)), number
    assert O.to_values(r.ebm).tolist() == ((FULL_KEY << 16) + np.arange(65536)).tolist()
    _check_set_level(r, *transpose_counts(cols, vals, None))
    _check_typed_by_cardinality(r, ebm_too=False)


@pytest.mark.parametrize("parallelism,kinds", [(1, (0, 1, 0)), (2, (0, 0, 1)), (16, (0, 1, 0))])
def test_value_equals_column(parallelism, kinds):
    """65,536 columns whose value is the column: one batch, two batches of 32,768, sixteen of 4,096"""
    c = np.arange(65536)
    o = index_of(c, c)
    r = transpose_reference(o, None, parallelism)
    assert _kinds(r.ebm) == kinds and full_keys(o, None, parallelism) == {0: kinds[2] == 1}
    assert (r.bit_count(), r.min, r.max) == (1, 1, 1) and r.ba[0] == O.from_values(c)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_indexes(seed):
    """17-bit and 32-slice values, with and without a foundSet that holds columns and keys ebM lacks"""
    for wide in (False, True):
        cols, vals, found_cols = random_index(seed, wide=wide)
        o = index_of(cols, vals, 32 if wide else None)
        found = O.from_values(found_cols)
        for parallelism in (1, 2, 7, 30):
            for f, fc in ((None, None), (found, found_cols)):
                r = transpose_reference(o, f, parallelism)
                u, n = transpose_counts(cols, vals, fc)
                assert u.size > 50 and n.max() > 3 and full_keys(o, f, parallelism) == {}
                _check_set_level(r, u, n)
                _check_typed_by_cardinality(r)
        if wide:
            assert int(O.to_values(r.ebm)[-1]) == 0xFFFFFFFF and int(O.to_values(r.ebm)[0]) == 0


def test_empty_results():
    o = index_of([5, 70000], [3, 4])
    for r in (transpose_reference(o, _bsi.EMPTY, 1), transpose_reference(o, O.from_values([6, 1 << 20]), 3),
              transpose_reference(index_of([], []), None, 2)):
        assert r.ebm == _bsi.EMPTY and r.ba == [] and (r.min, r.max) == (0, 0)
    with pytest.raises(ZeroDivisionError):
        transpose_reference(o, None, 0)
