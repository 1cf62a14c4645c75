"""CPU ORACLE of RoaringBitmapSliceIndex.add (test infrastructure only).

add_reference composes the reference's literal sequence (bsi/src/main/java/org/roaringbitmap/bsi/
RoaringBitmapSliceIndex.java:66-95, BSI/ below) from the container-exact oracle's pairwise ops
(tests/_oracle.py): this.ebM.or(other.ebM) in place is "ior", addDigit's RoaringBitmap.and is "and", and
bA[i].xor(x) in place is "xor" (the in-place xor's container types are the static one's).
minValue() / maxValue() are the descents of BSI/:97-138 with valueAt's Java int.  sum_values is the same
sum in plain numpy, independent of any bitmap code.
"""
import numpy as np

import _oracle as O
from _bsi import BSI, EMPTY


def _empty(buf):
    return O.stats(buf)["card"] == 0


def _i32(x):
    return int(np.int64(x).astype(np.int32))


def extreme(ebm, ba, largest):
    """BSI/:97-111 minValue() / :113-127 maxValue(), with valueAt (:129-138)"""
    if _empty(ebm):
        return 0
    ids = ebm
    for i in range(len(ba) - 1, -1, -1):
        tmp = O.pairwise("and" if largest else "andnot", ids, ba[i])
        if not _empty(tmp):
            ids = tmp
    col = int(O.to_values(ids)[0])  # first()
    v = 0
    for i, b in enumerate(ba):
        if O.pairwise_card("and", b, O.from_values([col])) == 1:
            v |= 1 << i
    return _i32(v)


def add_reference(a: BSI, b: BSI):
    """a.add(b) -> the result as a new BSI (its .steps: the addDigit calls made).  a and b stay as they are
    (bitmaps are immutable bytes, so a added to itself adds a snapshot: every value doubles)."""
    if b is None or _empty(b.ebm):  # BSI/:67-69
        r = BSI(a.ebm, a.ba, a.min, a.max, a.run_optimized)
        r.steps = 0
        return r
    ebm = O.pairwise("ior", a.ebm, b.ebm)
    ba = list(a.ba) + [EMPTY] * max(0, b.bit_count() - a.bit_count())  # grow: new slices are empty
    steps = 0
    for i, x in enumerate(b.ba):
        carry, k = x, i
        while True:  # addDigit(carry, k), BSI/:85-95
            nxt = O.pairwise("and", ba[k], carry)
            ba[k] = O.pairwise("xor", ba[k], carry)
            steps += 1
            if _empty(nxt):
                break
            if k + 1 >= len(ba):
                ba.append(EMPTY)
            carry, k = nxt, k + 1
    r = BSI(ebm, ba, extreme(ebm, ba, False), extreme(ebm, ba, True), a.run_optimized)
    r.steps = steps
    return r


def sum_values(cols_a, vals_a, cols_b, vals_b):
    """-> (columns ascending, uint32; their summed values, int64): the columns of either index, a missing
    side counting as 0"""
    cols_a, cols_b = np.asarray(cols_a, dtype=np.int64), np.asarray(cols_b, dtype=np.int64)
    cols = np.union1d(cols_a, cols_b)
    out = np.zeros(cols.size, dtype=np.int64)
    np.add.at(out, np.searchsorted(cols, cols_a), np.asarray(vals_a, dtype=np.int64))
    np.add.at(out, np.searchsorted(cols, cols_b), np.asarray(vals_b, dtype=np.int64))
    return cols.astype(np.uint32), out


def values_of(x: BSI):
    """-> (columns of ebM ascending, their values as unsigned slices): reads the index back on the host"""
    cols = O.to_values(x.ebm)
    v = np.zeros(cols.size, dtype=np.int64)
    for i, b in enumerate(x.ba):
        v |= np.isin(cols, O.to_values(b)).astype(np.int64) << i
    return cols, v
