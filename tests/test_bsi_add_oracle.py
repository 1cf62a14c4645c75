"""RoaringBitmapSliceIndex.add (BSI/:66-95) on the CPU oracle: the reference's own known answers
(bsi/src/test/java/org/roaringbitmap/bsi/RBBsiTest.java testAdd / testAddAndEvaluate, BufferBSITest.java:99-135)
and the three facts the fused device kernel rests on: the slices of a run-free sum have the
types their final cardinalities give, the existence bitmap follows Container.ior, and a 32nd slice makes the
reported extrema wrap as Java ints do."""
import numpy as np
import pytest

import _oracle as O
from _bsi import BSI, EMPTY
from _bsi_add import add_reference, sum_values, values_of


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


def test_known_answer_add():
    """testAdd: columns 1..99 with value x plus columns 1..119 with value x"""
    a = BSI.from_columns(np.arange(1, 100), np.arange(1, 100))
    b = BSI.from_columns(np.arange(1, 120), np.arange(1, 120))
    r = add_reference(a, b)
    cols, vals = values_of(r)
    assert cols.tolist() == list(range(1, 120))
    assert vals.tolist() == [2 * x if x < 100 else x for x in range(1, 120)]
    assert (r.min, r.max, r.bit_count()) == (2, 198, 8)


def test_known_answer_add_and_evaluate():
    """testAddAndEvaluate: value x at column x plus value x at column 120 - x"""
    a = BSI.from_columns(np.arange(1, 100), np.arange(1, 100))
    x = np.arange(1, 120)
    b = BSI.from_columns(120 - x, x)
    r = add_reference(a, b)
    assert O.to_values(r.compare("EQ", 120)).tolist() == list(range(1, 100))
    assert O.to_values(r.compare("RANGE", 1, 20)).tolist() == list(range(100, 120))


def _random_pair(seed):
    rng = np.random.default_rng(seed)
    keys = [0, 2, 3, 65535]
    out = []
    for bits, sizes in ((10, (3000, 5000, 60000, 4097)), (12, (5000, 3000, 60000, 4096))):
        cols = np.concatenate([(k << 16) + rng.choice(65536, n, replace=False) for k, n in zip(keys, sizes)])
        out.append((cols.astype(np.int64), rng.integers(0, 1 << bits, size=cols.size)))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_run_free_sums_have_cardinality_canonical_slices(seed):
    """every slice of the composed reference result is byte-equal to bitmapOf of the arithmetic sum's bit"""
    (ca, va), (cb, vb) = _random_pair(seed)
    r = add_reference(BSI.from_columns(ca, va), BSI.from_columns(cb, vb))
    cols, vals = sum_values(ca, va, cb, vb)
    assert r.bit_count() == int(vals.max()).bit_length() and r.steps > r.bit_count()
    for i, s in enumerate(r.ba):
        assert s == O.from_values(cols[(vals >> i) & 1 == 1]), i
    assert (r.min, r.max) == (int(vals.min()), int(vals.max()))


def _one_key(lows, key=7):
    return BSI.from_columns((key << 16) + np.asarray(lows, dtype=np.int64), np.ones(len(lows), dtype=np.int64))


@pytest.mark.parametrize("name,a_lows,b_lows,kinds", [
    ("bitmap_or_bitmap_full_is_run", np.arange(65536), np.arange(65536), (0, 0, 1)),
    ("bitmap_with_array_full_stays_bitmap", np.arange(4000, 65536), np.arange(4000), (0, 1, 0)),
    ("array_with_bitmap_full_is_run", np.arange(4000), np.arange(4000, 65536), (0, 0, 1)),
])
def test_existence_bitmap_follows_ior(name, a_lows, b_lows, kinds):
    a, b = _one_key(a_lows), _one_key(b_lows)
    r = add_reference(a, b)
    assert O.stats(r.ebm)["card"] == 65536 and _kinds(r.ebm) == kinds, name
    assert _kinds(a.ebm)[2] == 0 and _kinds(b.ebm)[2] == 0  # run-free operands


def test_full_slices_cancel_and_carry():
    """65,536 columns of value 1 on both sides: slice 0 vanishes, slice 1 is a full bitmap container"""
    r = add_reference(_one_key(np.arange(65536)), _one_key(np.arange(65536)))
    assert r.ba[0] == EMPTY and _kinds(r.ba[1]) == (0, 1, 0) and O.stats(r.ba[1])["card"] == 65536
    assert (r.min, r.max) == (2, 2)


def test_thirty_second_slice_wraps_the_extrema():
    a = BSI.from_columns([5, 70000], [2**31 - 1, 3])
    b = BSI.from_columns([5], [1])
    r = add_reference(a, b)
    # the descents are unsigned (column 70000 holds the smallest value); valueAt's 1 << 31 wraps the largest
    assert r.bit_count() == 32 and r.max == -2**31 and r.min == 3
    cols, vals = values_of(r)
    assert cols.tolist() == [5, 70000] and vals.tolist() == [2**31, 3]


def test_empty_other_returns_this():
    a = BSI.from_columns([1, 2], [3, 4])
    r = add_reference(a, BSI.from_columns([], []))
    assert (r.ebm, r.ba, r.min, r.max) == (a.ebm, a.ba, 3, 4)
    r = add_reference(BSI.from_columns([], []), a)
    assert (r.ebm, r.ba, r.min, r.max) == (a.ebm, a.ba, 3, 4)
