"""BitSliceIndexBase.parallelIn (BBSI/:611-639) on the CPU oracle: the reference's own known answer
(bsi/src/test/java/org/roaringbitmap/bsi/BufferBSITest.java testIN), the container-type facts the fused device
kernel rests on, and the composed reference (tests/_bsi_in.py in_reference) against the per-key
rule those facts give and against a plain numpy answer."""
import numpy as np
import pytest

import _oracle as O
from _bsi import BSI, EMPTY
from _bsi_in import batch_size, in_reference, in_set

FULL = np.arange(65536, dtype=np.int64)


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


def _ones(cols):
    cols = np.asarray(cols, dtype=np.int64)
    return BSI.from_columns(cols, np.ones(cols.size, dtype=np.int64))


def test_known_answer_in():
    """testIN: columns 1..99 with value = column, values 1..20, parallelism 2"""
    x = np.arange(1, 100)
    r = in_reference(BSI.from_columns(x, x), None, range(1, 21), 2)
    assert O.to_values(r).tolist() == list(range(1, 21))
    assert r == O.from_values(np.arange(1, 21))


def test_batch_size_is_java_int_arithmetic():
    assert [batch_size(c, p) for c, p in ((99, 2), (3, 7), (0, 5), (1 << 20, 1), (1 << 20, 16), (1 << 20, 17))] == \
        [49, 7, 5, 65536, 65536, 61680]


def test_type_facts_of_add_and_lazy_or():
    """what batchIn's add() builds and what MutableRoaringBitmap.or(rbs) makes of it"""
    full = O.from_values(FULL)
    assert _kinds(full) == (0, 1, 0)  # bitmapOf(0..65535): a bitmap container, never a run
    split = O.wide("or", [O.from_values(FULL[:30000]), O.from_values(FULL[30000:])])
    assert _kinds(split) == (0, 0, 1) and O.stats(split)["card"] == 65536  # repairAfterLazy: RunContainer.full()
    assert O.wide("or", [full]) == full  # a single batch: the container add() built
    other = O.from_values((5 << 16) + FULL[:10])
    both = O.wide("or", [full, other])
    assert _kinds(both) == (1, 1, 0) and O.stats(both)["card"] == 65546  # a key of one batch alone is kept
    p = np.random.default_rng(1).permutation(65536)
    a4096 = O.wide("or", [O.from_values(p[:2000]), O.from_values(p[2000:4096])])
    assert _kinds(a4096) == (1, 0, 0) and a4096 == O.from_values(p[:4096])
    b4097 = O.wide("or", [O.from_values(p[:2000]), O.from_values(p[2000:4097])])
    assert _kinds(b4097) == (0, 1, 0) and b4097 == O.from_values(p[:4097])
    assert O.wide("or", [EMPTY, EMPTY]) == EMPTY
    assert in_reference(_ones([]), None, [1], 3) == EMPTY  # no batch at all


def _rule(result_cols, fixed_cols, parallelism):
    """(arrays, bitmaps, runs) by the per-key rule: cardinality alone, but a full container is a run
    container unless batchSize == 65536 and the key's first column has a rank that is a multiple of it"""
    size = batch_size(len(fixed_cols), parallelism)
    fixed_cols = np.sort(np.asarray(fixed_cols, dtype=np.int64))
    keys, cards = np.unique(np.asarray(result_cols, dtype=np.int64) >> 16, return_counts=True)
    out = [0, 0, 0]
    for k, c in zip(keys, cards):
        if c <= 4096:
            out[0] += 1
        elif c < 65536:
            out[1] += 1
        else:
            r = int(np.searchsorted(fixed_cols, k << 16))
            out[1 if size == 65536 and r % 65536 == 0 else 2] += 1
    return tuple(out)


@pytest.mark.parametrize("name,cols,found,parallelism,kinds", [
    ("aligned", np.concatenate([(1 << 16) + FULL, (2 << 16) + FULL]), None, 1, (0, 2, 0)),
    ("misaligned", np.concatenate([[5], (1 << 16) + FULL, (2 << 16) + FULL]), None, 1, (1, 0, 2)),
    ("second_key_aligned_again", np.concatenate([FULL[:30000], (1 << 16) + FULL, (2 << 16) + FULL[:35536],
                                                 (3 << 16) + FULL]), None, 1, (0, 3, 1)),
    ("small_batches", (1 << 16) + FULL, None, 2, (0, 0, 1)),
    ("parallelism_above_cardinality", (1 << 16) + FULL, None, 100000, (0, 1, 0)),  # min(100000, 65536)
    ("found_shifts_the_ranks", (1 << 16) + FULL, np.concatenate([[3, 9], (1 << 16) + FULL]), 1, (0, 0, 1)),
    ("found_pads_to_alignment", (1 << 16) + FULL, np.concatenate([FULL, (1 << 16) + FULL]), 1, (0, 1, 0)),
    ("found_cuts_the_key", (1 << 16) + FULL, (1 << 16) + FULL[:65535], 1, (0, 1, 0)),
])
def test_in_reference_obeys_the_per_key_rule(name, cols, found, parallelism, kinds):
    x = _ones(cols)
    fixed = cols if found is None else found
    r = in_reference(x, None if found is None else O.from_values(found), [1], parallelism)
    want = in_set(cols, np.ones(len(cols)), found, [1])
    assert O.to_values(r).tolist() == want.tolist(), name
    assert _kinds(r) == kinds == _rule(want, fixed, parallelism), name


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_in_reference_equals_plain_numpy(seed):
    rng = np.random.default_rng(seed)
    sizes = rng.permutation([3000, 5000, 60000, 4097, 65536])
    cols = np.concatenate([(k << 16) + rng.choice(65536, n, replace=False) for k, n in zip((0, 2, 3, 9, 65535), sizes)])
    vals = rng.integers(0, 40, size=cols.size)
    found = np.unique(np.concatenate([rng.choice(cols, cols.size // 2, replace=False),
                                      rng.integers(0, 1 << 32, size=2000)]))
    values = rng.integers(-3, 45, size=12).tolist()
    x = BSI.from_columns(cols, vals)
    for f, p in ((None, 1), (None, 3), (found, 2), (found, 70000)):
        r = in_reference(x, None if f is None else O.from_values(f), values, p)
        want = in_set(cols, vals, f, values)
        assert O.to_values(r).tolist() == want.tolist() and want.size > 100
        assert _kinds(r) == _rule(want, cols if f is None else f, p)
