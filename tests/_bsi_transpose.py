"""CPU ORACLE of the buffer package's BitSliceIndexBase.parallelTransposeWithCount (test infrastructure only).

transpose_reference composes the reference's literal sequence (bsi/src/main/java/org/roaringbitmap/bsi/buffer/
BitSliceIndexBase.java, BBSI/ below) from the container-exact oracle (tests/_oracle.py):
  parallelTransposeWithCount BBSI/:569-597  fixed = foundSet or ebM
  parallelExec               BBSI/:99-136   consecutive batches of min(max(card / parallelism, parallelism), 65536)
  transposeWithCount         BBSI/:551-567  per batch a fresh MutableBitSliceIndex, setValue(value, count so far + 1)
                                            for every column that exists in ebM: BSI.from_columns over the batch's
                                            distinct values and their counts (incremental add / remove keep a
                                            container's type tied to its cardinality)
  the sum of the batches     MutableBitSliceIndex.add, buffer/MutableBitSliceIndex.java:201-219, in order into an
                                            empty index: add_reference (ebM.or in place, addDigit's and / xor chain,
                                            the minValue() / maxValue() descents)
transpose_counts is the same answer at set level in plain numpy, independent of any bitmap code, and
full_key_is_run the per-key rule for the one container whose type depends on the batches.
"""
import numpy as np

import _oracle as O
from _bsi import BSI, EMPTY
from _bsi_add import add_reference, values_of
from _bsi_in import batch_size


def batch_values(bsi, found, parallelism):
    """-> per batch of parallelExec the values (uint32 patterns) of its columns that exist in ebM"""
    if parallelism < 1:
        raise ZeroDivisionError("parallelism")
    fixed = O.to_values(bsi.ebm if found is None else found)
    cols, vals = values_of(bsi)
    if not fixed.size or not cols.size:
        return []
    size = batch_size(fixed.size, parallelism)
    out = []
    for i in range(0, fixed.size, size):
        batch = fixed[i:i + size]
        at = np.searchsorted(cols, batch)
        at[at == cols.size] = 0
        out.append(vals[at][cols[at] == batch].astype(np.uint32))
    return out


def transpose_reference(bsi, found, parallelism):
    """bsi.parallelTransposeWithCount(found, parallelism, pool) -> the result as a BSI; found: bytes or None"""
    acc = BSI(EMPTY, [], 0, 0)
    for v in batch_values(bsi, found, parallelism):
        if not v.size:  # an empty batch index: add returns at once
            continue
        u, n = np.unique(v, return_counts=True)
        acc = add_reference(acc, BSI.from_columns(u.astype(np.int64), n.astype(np.int64)))
    return BSI(acc.ebm, acc.ba, acc.min, acc.max)


def transpose_counts(cols, vals, found_cols):
    """-> (the distinct 32-bit value patterns among cols, and among found_cols unless None, ascending, uint32;
    how many columns hold each, int64)"""
    cols = np.asarray(cols, dtype=np.int64)
    v32 = np.asarray(vals, dtype=np.int64).astype(np.uint32)
    if found_cols is not None:
        v32 = v32[np.isin(cols, np.asarray(found_cols, dtype=np.int64))]
    u, n = np.unique(v32, return_counts=True)
    return u.astype(np.uint32), n.astype(np.int64)


def full_key_is_run(batches_low):
    """The per-key rule for a full result key (all 65,536 values under one high half present).  batches_low: per
    batch that contributes a value to the key, in order, the low halves of its values.  With d_t distinct values in
    batch t and U_t in the union after t batches, the container is RunContainer.full() iff some t >= 2 has
    U_t == 65536 and d_t > 4096 (Container.ior: a full union with a bitmap on the other side); else a bitmap."""
    seen = np.zeros(65536, dtype=bool)
    run = False
    for t, low in enumerate(batches_low, start=1):
        d = np.unique(np.asarray(low, dtype=np.int64) & 0xFFFF)
        seen[d] = True
        if t >= 2 and seen.all() and d.size > 4096:
            run = True
    assert seen.all(), "not a full key"
    return run


def full_keys(bsi, found, parallelism):
    """-> {result key: True for a run container, False for a bitmap} for every full result key, by the rule"""
    per = batch_values(bsi, found, parallelism)
    allv = np.unique(np.concatenate(per)) if per else np.zeros(0, dtype=np.uint32)
    keys, n = np.unique(allv >> 16, return_counts=True)
    out = {}
    for k in keys[n == 65536].tolist():
        lows = [v[(v >> 16) == k] & 0xFFFF for v in per]
        out[k] = full_key_is_run([x for x in lows if x.size])
    return out


# ---- shared cases (built once per process, left unchanged) --------------------------------------------------------

def index_of(cols, vals, nbits=None):
    """an oracle index with hand-made slices (bitmapOf-typed); nbits: the slice count, by default the bit length of
    the largest value (one empty slice for all-zero values).  Takes values up to 2^32 - 1 (32 slices)."""
    cols = np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.int64)
    if nbits is None:
        nbits = max(1, int(vals.max()).bit_length()) if vals.size else 0
    ba = [O.from_values(cols[(vals >> i) & 1 == 1]) for i in range(nbits)]
    return BSI(O.from_values(cols), ba, int(vals.min()) if vals.size else 0, int(vals.max()) if vals.size else 0)


FULL_KEY = 3  # the result key the full-key cases fill: values FULL_KEY << 16 | low


def full_case(number):
    """The six hand-made full-key cases -> (columns, values, parallelism, batchSize, is a run container).  The
    columns are 0..n-1, so batch t holds columns [t batchSize, (t + 1) batchSize); a batch is given by the new low
    halves it brings and padded to batchSize with repeats of its first."""
    def pad(lows, size):
        lows = np.asarray(lows, dtype=np.int64)
        return np.concatenate([lows, np.full(size - lows.size, lows[0], dtype=np.int64)])

    a = np.arange
    three = [a(0, 20000), a(20000, 40000), a(40000, 60000)]
    five = three + [pad(a(60000, 63000), 20000), pad(a(63000, 65536), 20000)]
    if number == 1:  # the union becomes full at batch 4, a bitmap batch (5,536 distinct values)
        batches, size, run = three + [pad(a(60000, 65536), 20000)], 20000, True
    elif number == 2:  # full at batch 5, an array batch (2,536 distinct), nothing after
        batches, size, run = five, 20000, False
    elif number == 3:  # ... followed by a batch of 5,000 distinct values
        batches, size, run = five + [pad(a(100, 5100), 20000)], 20000, True
    elif number == 4:  # ... followed by a batch of exactly 4,096
        batches, size, run = five + [pad(a(100, 4196), 20000)], 20000, False
    elif number == 5:  # a full first batch of 65,536, then 100 values
        batches, size, run = [a(65536), a(500, 600)], 65536, False
    elif number == 6:  # a full first batch of 65,536, then 5,000 values
        batches, size, run = [a(65536), a(500, 5500)], 65536, True
    else:
        raise ValueError(number)
    low = np.concatenate(batches)
    parallelism = 1 if size == 65536 else low.size // size
    assert batch_size(low.size, parallelism) == size
    return a(low.size), (FULL_KEY << 16) | low, parallelism, size, run


def random_index(seed, n=6000, wide=False):
    """n columns over five keys (0 and 65535 among them) with skewed values from a pool of 400 (so counts above 1),
    17-bit by default, 32-bit patterns with `wide`; and foundSet columns that hold columns and keys ebM lacks
    -> (columns, values, foundSet columns)"""
    rng = np.random.default_rng(seed)
    keys = np.array([0, 7, 8, 300, 65535], dtype=np.int64)
    cols = np.unique((rng.choice(keys, n) << 16) | rng.integers(0, 65536, n))
    pool = rng.integers(0, 1 << 32 if wide else 1 << 17, 400)
    if wide:
        pool[:3] = [0xFFFFFFFF, 0x80000000, 0]
    vals = pool[np.minimum(rng.geometric(0.02, cols.size) - 1, pool.size - 1)]
    found = np.unique(np.concatenate([cols[::3], cols[(cols >> 16) == 8], rng.integers(0, 1 << 32, 500),
                                      (7 << 16) + rng.integers(0, 65536, 300)]))
    return cols, vals, found
