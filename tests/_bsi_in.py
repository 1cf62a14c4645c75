"""CPU ORACLE of the buffer package's BitSliceIndexBase.parallelIn (test infrastructure only).

in_reference composes the reference's literal sequence (bsi/src/main/java/org/roaringbitmap/bsi/buffer/
BitSliceIndexBase.java, BBSI/ below) from the container-exact oracle (tests/_oracle.py):
  parallelIn   BBSI/:611-625   fixed = foundSet or ebM
  parallelExec BBSI/:99-136    consecutive batches of min(max(card / parallelism, parallelism), 65536) columns
  batchIn      BBSI/:628-639   one MutableRoaringBitmap per batch, add(cID) for every column that exists in ebM
                               and whose value is in the set: bitmapOf's types, O.from_values
  parallelMR   BBSI/:148-164   MutableRoaringBitmap.or(rbs) = BufferFastAggregation.naive_or: naivelazyor per
                               batch, then repairAfterLazy, which is the heap naive_or's steps: O.wide("or")
in_set is the same answer at set level in plain numpy, independent of any bitmap code.
"""
import numpy as np

import _oracle as O
from _bsi import EMPTY
from _bsi_add import values_of


def _patterns(values):
    """an IN list as 32-bit patterns (getValue assembles a Java int: membership is equality of those)"""
    return np.unique(np.asarray(list(values), dtype=np.int64).astype(np.uint32))


def batch_size(card, parallelism):
    """parallelExec's batchSize (BBSI/:104), Java int division"""
    return min(max(card // parallelism, parallelism), 65536)


def in_reference(bsi, found, values, parallelism):
    """bsi.parallelIn(parallelism, found, values, pool) -> the result's bytes; found: bytes or None"""
    if parallelism < 1:
        raise ZeroDivisionError("parallelism")
    fixed = O.to_values(bsi.ebm if found is None else found)
    cols, vals = values_of(bsi)
    want = _patterns(values)
    size = batch_size(fixed.size, parallelism)
    parts = []
    for i in range(0, fixed.size, size):
        batch = fixed[i:i + size]
        at = np.searchsorted(cols, batch)
        at[at == cols.size] = 0
        exists = cols[at] == batch if cols.size else np.zeros(batch.size, dtype=bool)
        hit = exists & np.isin(vals[at].astype(np.uint32), want) if cols.size else exists
        parts.append(O.from_values(batch[hit]))
    return O.wide("or", parts) if parts else EMPTY


def in_set(cols, vals, found_cols, values):
    """the columns (ascending, uint32) among cols, and among found_cols unless None, whose value is listed"""
    cols = np.asarray(cols, dtype=np.int64)
    v32 = np.asarray(vals, dtype=np.int64).astype(np.uint32)
    keep = np.isin(v32, _patterns(values))
    if found_cols is not None:
        keep &= np.isin(cols, np.asarray(found_cols, dtype=np.int64))
    return np.sort(cols[keep]).astype(np.uint32)
