"""CPU ORACLE of RoaringBitmapSliceIndex.setValues(List<Pair>) (test infrastructure only).

bsi/src/main/java/org/roaringbitmap/bsi/RoaringBitmapSliceIndex.java (BSI/ below): setValues :349-357 is
ensureCapacityInternal(min, max of the list) :315-326 and then, per pair in order, setValueInternal :304-313 --
bA[i].add(column) where bit i of the value is set, bA[i].remove(column) otherwise, for i < bitCount(), and
ebM.add(column).  setValue :299-302 is the list of one pair.  Two independent forms:

set_reference  a plain dict replay of the pairs in order; the final sets are typed by cardinality
               (O.from_values): ArrayContainer.add turns into a bitmap above 4,096 values, BitmapContainer.remove
               into an array at 4,096, BitmapContainer.add returns this, an emptied container is removed, so a
               run-free container's type is its final cardinality's, a full one a bitmap container.  An ebM with
               full run containers keeps them (RunContainer.add returns this for a value inside a run): the
               operand's bytes when no column is new, else or(old ebM, bitmapOf(new columns)) for new columns
               in other keys.
set_composed   slice' = or(andnot(slice, B), S_i) and ebM' = or(ebM, B) from the container-exact pairwise
               oracle on run-free input, B = bitmapOf(the columns), S_i = bitmapOf(the columns whose last value has
               bit i).  The static or returns RunContainer.full() for a full result, which the add sequence
               never does: removeRunCompression puts the bitmap container back.
"""
import numpy as np

import _oracle as O
from _bsi import BSI, EMPTY


def bitlen(x):
    return len(bin(int(x))) - 2  # Integer.toBinaryString(x).length(); 1 for 0


def capacity(ebm_empty, depth, mn, mx, bmin, bmax):
    """ensureCapacityInternal(bmin, bmax) -> (depth', min', max'), BSI/:315-326 with grow :328-347"""
    if ebm_empty:
        return max(depth, bitlen(bmax)), bmin, bmax
    if mn > bmin:
        return depth, bmin, mx  # the else-if: max and the depth stay even when bmax exceeds max
    if mx < bmax:
        return max(depth, bitlen(bmax)), mn, bmax
    return depth, mn, mx


def _pairs(cols, vals):
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals, dtype=np.int64).reshape(-1)
    if cols.size != vals.size or cols.size == 0:
        raise ValueError("setValues needs n >= 1 pairs")
    if vals.min() < 0 or vals.max() >= 1 << 31:
        raise ValueError("Values should be non-negative Java ints")
    return cols, vals


def _has_run(buf):
    return O.stats(buf)["run"] > 0


def set_reference(a: BSI, cols, vals) -> BSI:
    """a.setValues(pairs) -> the result as a new BSI; a stays as it is"""
    cols, vals = _pairs(cols, vals)
    assert not any(_has_run(s) for s in a.ba), "a slice holds a run container"
    old = O.to_values(a.ebm).astype(np.int64)
    depth, mn, mx = capacity(old.size == 0, a.bit_count(), a.min, a.max, int(vals.min()), int(vals.max()))
    last = {}
    for c, v in zip(cols.tolist(), vals.tolist()):  # the replay: a later pair overwrites
        last[c] = v
    touched = np.fromiter(last.keys(), dtype=np.int64, count=len(last))
    win = np.fromiter(last.values(), dtype=np.int64, count=len(last))
    ba = []
    for i in range(depth):
        kept = np.setdiff1d(O.to_values(a.ba[i]).astype(np.int64), touched) if i < a.bit_count() else touched[:0]
        ba.append(O.from_values(np.concatenate([kept, touched[(win >> i) & 1 == 1]])))
    new = np.setdiff1d(touched, old)
    if not _has_run(a.ebm):
        ebm = O.from_values(np.concatenate([old, new]))
    elif new.size == 0:
        ebm = a.ebm
    else:
        ebm = O.pairwise("or", a.ebm, O.from_values(new))
    return BSI(ebm, ba, mn, mx, a.run_optimized)


def set_composed(a: BSI, cols, vals) -> BSI:
    cols, vals = _pairs(cols, vals)
    assert not any(_has_run(s) for s in [a.ebm] + a.ba), "the composed form takes run-free input"
    depth, mn, mx = capacity(O.stats(a.ebm)["card"] == 0, a.bit_count(), a.min, a.max, int(vals.min()),
                             int(vals.max()))
    u, first = np.unique(cols[::-1], return_index=True)
    win = vals[::-1][first]
    b = O.from_values(u)

    def no_run(buf):
        return O.remove_run_compression(buf) if _has_run(buf) else buf

    ba = []
    for i in range(depth):
        s = a.ba[i] if i < a.bit_count() else EMPTY
        ba.append(no_run(O.pairwise("or", O.pairwise("andnot", s, b), O.from_values(u[(win >> i) & 1 == 1]))))
    return BSI(no_run(O.pairwise("or", a.ebm, b)), ba, mn, mx, a.run_optimized)


def replay_values(a_cols, a_vals, cols, vals, depth):
    """(columns ascending, values) after the call, in plain numpy over the pairs alone: values masked to depth"""
    d = dict(zip(np.asarray(a_cols).tolist(), np.asarray(a_vals).tolist()))
    for c, v in zip(np.asarray(cols).tolist(), np.asarray(vals).tolist()):
        d[c] = v & ((1 << depth) - 1)
    c = np.array(sorted(d), dtype=np.int64)
    return c, np.array([d[x] for x in c.tolist()], dtype=np.int64)
