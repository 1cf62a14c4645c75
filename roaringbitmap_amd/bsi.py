"""Host-side mirror of the bit-sliced indexes' query path.

Mirrors bsi/src/main/java/org/roaringbitmap/bsi/RoaringBitmapSliceIndex.java (BSI/):
compare(Operation, startOrValue, end, foundSet) (BSI/:482-513) and
sum(foundSet) (BSI/:581-592), and the buffer package's ImmutableBitSliceIndex /
MutableBitSliceIndex (bsi/src/main/java/org/roaringbitmap/bsi/buffer/BitSliceIndexBase.java,
BBSI/): compare (BBSI/:422-453), rangeEQ / rangeNEQ / rangeLT / rangeLE / rangeGT / rangeGE /
range (BBSI/:351-408) and sum (BBSI/:521-532).  Every query runs on the MI355X
(csrc/bsi.hip) and the results are the reference's bytes, container types included.
Construction (setValue) is host-side by default; from_columns(..., gpu=True) builds the slices on the
device (csrc/bsibuild.hip), and getValues / toPairList read values back in bulk (csrc/bsival.hip with
gpu=True).  add(otherBsi) (BSI/:66-95) sums two indexes in one fused device pass (csrc/bsiadd.hip) when
neither holds a run container, and replays the reference's and / xor chain with the pairwise device ops
otherwise.  setValue / setValues (BSI/:299-357) write pairs into an existing index, repeated columns included:
numpy on the host by default, one device call (csrc/bsiset.hip) with gpu=True.  The buffer index's parallelIn
(BBSI/:611-639), WHERE value IN (...), is one fused pass too (csrc/bsiin.hip), and its parallelTransposeWithCount (BBSI/:551-597), GROUP BY value / COUNT(*), one device
call (csrc/bsitr.hip).
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import OPERATIONS  # noqa: F401  (the operation names, importable from here as before)
from ._lib import IllegalArgumentException, as_u32, call_bytes, check, lib, take
from .roaring import RoaringBitmap, run_optimize_many


def _index_call(f, *args, ebm_cls=RoaringBitmap):
    """f(*args, outs, out3): a one-shot call that makes an index -> (ebM, slices, minValue, maxValue) from the
    1 + nbits buffers it wrote and out3 = {nbits, minValue, maxValue}"""
    outs = (_lib.rbg_buffer * 34)()  # ebM and at most 33 slices (rbg_bsi_add's; the others write at most 33)
    out3 = (ctypes.c_int32 * 3)()
    check(f(*args, outs, out3))
    return (ebm_cls(take(outs[0])), [RoaringBitmap(take(outs[1 + k])) for k in range(int(out3[0]))],
            int(out3[1]), int(out3[2]))


class RoaringBitmapSliceIndex:
    """ebM (existence bitmap), bA (slices, bit 0 first), minValue, maxValue (BSI/:16-38)."""

    def __init__(self, ebm=None, slices=(), min_value=0, max_value=0):
        self.ebM = ebm if ebm is not None else RoaringBitmap()
        self.bA = list(slices)
        self.minValue = int(min_value)
        self.maxValue = int(max_value)
        self.runOptimized = False

    @classmethod
    def from_columns(cls, columns, values, run_optimize=False, gpu=False):
        """setValue(c, v) for each pair, in order (BSI/:320-347); runOptimize() if asked (BSI/:141-150).
        gpu=True: the same object from the one-shot device build (rbg_bsi_from_columns, csrc/bsibuild.hip),
        which takes the pairs in any order but refuses a repeated column (setValue would overwrite)."""
        columns = np.asarray(columns, dtype=np.int64)
        values = np.asarray(values, dtype=np.int64)
        if columns.shape != values.shape:
            raise IllegalArgumentException("columns and values differ in length")
        if (values < 0).any():
            raise IllegalArgumentException("Values should be non-negative")
        if gpu:
            if values.size and int(values.max()) >= 1 << 31:
                raise IllegalArgumentException("Values should be below 2^31")
            c, v = _lib.pair_arrays(columns, values)
            obj = cls(*_index_call(lib().rbg_bsi_from_columns, c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                   v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), c.size,
                                   int(bool(run_optimize))))
            obj.runOptimized = bool(run_optimize)
            return obj
        mn = mx = 0
        if values.size:  # ensureCapacityInternal: first value sets both, then min or else max
            mn = mx = int(values[0])
            for v in values[1:]:
                v = int(v)
                if mn > v:
                    mn = v
                elif mx < v:
                    mx = v
        nbits = (len(bin(mx)) - 2) if values.size else 0
        ebm = RoaringBitmap.from_values(columns, run_optimize)
        ba = [RoaringBitmap.from_values(columns[(values >> i) & 1 == 1], run_optimize) for i in range(nbits)]
        obj = cls(ebm, ba, mn, mx)
        obj.runOptimized = bool(run_optimize)
        return obj

    def setValue(self, columnId, value):
        """BSI/:299-302 setValue(columnId, value), in place: setValues of the one pair."""
        self.setValues([columnId], [value])

    def setValues(self, columns, values, gpu=False):
        """BSI/:349-357 setValues(List<Pair>) as two arrays, in place: ensureCapacityInternal (:315-326) over the
        pairs' min and max, then per pair in order bA[i].add / remove(column) by bit i of the value and
        ebM.add(column) (:304-313) -- a column given many times keeps its last value, and minValue / maxValue
        / bitCount() are the reference's fields (the else-if of :320-325 included), not the true extremes.  A
        negative value or no pair raises IllegalArgumentException.  runOptimized stays as it was.
        Host default, no device: numpy over toArray() of the slices and from_values, so every container has
        the type its cardinality gives -- for a run-free index, or one whose only run containers are in an
        ebM that the pairs leave unchanged; otherwise IllegalArgumentException (try gpu=True).
        gpu=True: the one-shot device pass (rbg_bsi_set_values, csrc/bsiset.hip), which also takes an ebM
        with full run containers and new columns; it refuses a run container in a slice and one in ebM that
        is not full."""
        c, v = _lib.pair_arrays(columns, values)  # an empty list passes its range check
        if v.size == 0:
            raise IllegalArgumentException("setValues: no pair given")
        if len(self.bA) > 32:
            raise IllegalArgumentException("setValues: an index holds at most 32 slices")
        ebm_cls = type(self.ebM)
        if gpu:
            self.ebM, self.bA, self.minValue, self.maxValue = _index_call(
                lib().rbg_bsi_set_values, *self._operands()[0], self.minValue, self.maxValue,
                c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                c.size, ebm_cls=ebm_cls)
            return
        if any(b.container_stats()[2] > 0 for b in self.bA):
            raise IllegalArgumentException("setValues: a slice holds a run container")
        rev = c[::-1]
        cols, first = np.unique(rev, return_index=True)  # the last pair of every column
        win = v[::-1][first]
        old = self.ebM.toArray()
        ebm_same = bool(np.isin(cols, old).all())
        if not ebm_same and self.ebM.container_stats()[2] > 0:
            raise IllegalArgumentException("setValues: ebM holds a run container and the pairs add a column; "
                                           "the host form cannot type it, try gpu=True")
        bmin, bmax, depth = int(v.min()), int(v.max()), len(self.bA)
        if old.size == 0:  # ensureCapacityInternal
            self.minValue, self.maxValue = bmin, bmax
            depth = max(depth, len(bin(bmax)) - 2)
        elif self.minValue > bmin:
            self.minValue = bmin
        elif self.maxValue < bmax:
            self.maxValue = bmax
            depth = max(depth, len(bin(bmax)) - 2)
        ba = []
        for i in range(depth):
            kept = np.setdiff1d(self.bA[i].toArray(), cols) if i < len(self.bA) else cols[:0]
            ba.append(RoaringBitmap.from_values(np.concatenate([kept, cols[(win >> i) & 1 == 1]])))
        self.bA = ba
        if not ebm_same:
            self.ebM = ebm_cls.from_values(np.union1d(old, cols))

    def merge(self, otherBsi):
        """BSI/:379-405 ("designed for distributed computing"; the two indexes hold disjoint
        columns): slice-wise RoaringBitmap.or, runOptimize when either side was run-optimized
        (one device pass over all slices), the existence bitmaps united in place (x1.or(x2),
        Container.ior types) and min / max widened.  The buffer MutableBitSliceIndex.merge is the
        same steps over MutableRoaringBitmap (bsi/.../buffer/MutableBitSliceIndex.java:270-298)."""
        if otherBsi is None or otherBsi.ebM.isEmpty():
            return
        if RoaringBitmap.intersects(self.ebM, otherBsi.ebM):
            raise IllegalArgumentException("merge can be used only in bsiA  bsiB  is null")
        depth = max(self.bitCount(), otherBsi.bitCount())
        new = []
        for i in range(depth):
            cur = self.bA[i] if i < len(self.bA) else RoaringBitmap()
            other = otherBsi.bA[i] if i < len(otherBsi.bA) else RoaringBitmap()
            new.append(RoaringBitmap.or_(cur, other))
        if self.runOptimized or otherBsi.runOptimized:
            run_optimize_many(new)
        self.bA = new
        self.ebM.or_(otherBsi.ebM)  # in place
        self.runOptimized = self.runOptimized or otherBsi.runOptimized
        self.maxValue = max(self.maxValue, otherBsi.maxValue)
        self.minValue = min(self.minValue, otherBsi.minValue)

    def _has_run(self):
        """a run container anywhere in the index, from the serialized headers"""
        return any(b.container_stats()[2] > 0 for b in [self.ebM] + self.bA)

    def add(self, otherBsi):
        """BSI/:66-95, in place: ebM.or(other.ebM), grow, addDigit(other.bA[i], i) for every slice of the other
        index (carry = and(bA[i], x); bA[i].xor(x); the carry goes on to slice i + 1, growing the index by a
        slice when it leaves the top), then minValue() / maxValue() (:97-138).  None or an empty other index
        returns at once.  When neither index holds a run container the whole sum is one fused device pass
        (rbg_bsi_add, csrc/bsiadd.hip), the reference's bytes; otherwise, or with RBG_BSI_ADD_COMPOSED=1 in
        the environment (read at every call), the reference's sequence is replayed with the pairwise device
        ops (_add_composed).  runOptimized stays as it was.  A sum that needs a 33rd slice raises
        IllegalArgumentException on the fused path."""
        if otherBsi is None or otherBsi.ebM.isEmpty():
            return
        if os.environ.get("RBG_BSI_ADD_COMPOSED") == "1" or self._has_run() or otherBsi._has_run():
            self._add_composed(otherBsi)
            return
        if len(self.bA) > 32 or len(otherBsi.bA) > 32:
            raise IllegalArgumentException("add: an index holds at most 32 slices")
        self.ebM, self.bA, self.minValue, self.maxValue = _index_call(
            lib().rbg_bsi_add, *self._operands()[0], self.minValue, self.maxValue, *otherBsi._operands()[0],
            ebm_cls=type(self.ebM))

    def _add_composed(self, otherBsi):
        """The reference's literal sequence (BSI/:71-95) over the device's pairwise ops: the in-place or of the
        existence bitmaps, and per addDigit one static and, one in-place xor and the isEmpty() of the carry.
        (other is self: the reference would read slices it has already changed; a snapshot is added instead,
        which doubles the values as the fused path does.)"""
        other_ba = [b.clone() for b in otherBsi.bA]
        self.ebM.or_(otherBsi.ebM)
        while len(self.bA) < len(other_ba):  # grow(otherBsi.bitCount())
            self.bA.append(RoaringBitmap())
        for i, x in enumerate(other_ba):
            carry, k = x, i
            while True:  # addDigit(carry, k)
                nxt = RoaringBitmap.and_(self.bA[k], carry)
                self.bA[k].xor(carry)
                if nxt.isEmpty():
                    break
                if k + 1 >= len(self.bA):
                    self.bA.append(RoaringBitmap())  # grow(bitCount() + 1)
                carry, k = nxt, k + 1
        self.minValue, self.maxValue = self._extreme(False), self._extreme(True)

    def _extreme(self, largest):
        """minValue() / maxValue() (BSI/:97-138): the descent over the slices, then valueAt(first()) as a
        Java int"""
        if self.ebM.isEmpty():
            return 0
        ids = self.ebM
        for b in reversed(self.bA):
            tmp = RoaringBitmap.and_(ids, b) if largest else RoaringBitmap.andNot(ids, b)
            if not tmp.isEmpty():
                ids = tmp
        col = ids.first()
        v = 0
        for i, b in enumerate(self.bA):
            if b.contains(col):
                v |= 1 << i
        return int(np.int64(v).astype(np.int32))

    def getValue(self, columnId):
        """BSI/:181-196 getValue(columnId) -> (value, exists): ebM.contains, then one contains per slice
        (RoaringBitmap.contains on the serialized bitmaps, on the host)"""
        if not self.ebM.contains(columnId):
            return 0, False
        v = 0
        for i, b in enumerate(self.bA):
            if b.contains(columnId):
                v |= 1 << i
        return v, True

    def valueExist(self, columnId):
        """BBSI/:82 valueExist(columnId): ebM.contains(columnId)"""
        return self.ebM.contains(columnId)

    def getValues(self, columns, gpu=False):
        """getValue for many columns at once, the loop body of the buffer package's batchIn /
        transposeWithCount (BBSI/:551-639): an int64 array in query order, -1 where ebM lacks the column
        (getValue's exists == false).  The columns need not be sorted or distinct.  Host default: numpy
        membership tests against toArray() of ebM and of every slice; gpu=True: one batched lookup on the
        device (rbg_bsi_get_values, csrc/bsival.hip)."""
        q = as_u32(columns)
        if gpu:
            out = np.empty(q.size, dtype=np.int64)
            if q.size:
                check(lib().rbg_bsi_get_values(*self._operands()[0],
                                               q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), q.size,
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            return out
        v = np.zeros(q.size, dtype=np.int64)
        for i, b in enumerate(self.bA):
            v |= np.isin(q, b.toArray()).astype(np.int64) << i
        return np.where(np.isin(q, self.ebM.toArray()), v, -1)

    def toPairList(self, foundSet=None, gpu=False):
        """BBSI/:534-549 toPairList() / toPairList(foundSet) -> (columns, values): the columns of ebM, or of
        and(ebM, foundSet), ascending and unsigned (uint32), and their values (int64) from the batched
        lookup.  Host default: numpy over toArray() and getValues; gpu=True: the intersection, the expansion
        and the lookup run on the device."""
        if foundSet is None:
            cols = self.ebM.toArray(gpu=gpu)
        elif gpu:
            cols = RoaringBitmap.and_(self.ebM, foundSet).toArray(gpu=True)
        else:
            cols = np.intersect1d(self.ebM.toArray(), foundSet.toArray())
        return cols, self.getValues(cols, gpu=gpu)

    def runOptimize(self):
        """BSI/:141-150: runOptimize of ebM and of every slice (one device pass over all of them)."""
        run_optimize_many([self.ebM] + self.bA)
        self.runOptimized = True

    def bitCount(self):
        return len(self.bA)

    def getExistenceBitmap(self):
        return self.ebM

    def getLongCardinality(self):
        return self.ebM.getLongCardinality()

    def _operands(self, foundSet=None):
        """The argument blocks of the one-shot calls: (ebM, its length, the slices, their lengths, their count)
        and (foundSet or null, its length)."""
        arr, lens = _lib.buf_array([b.serialize() for b in self.bA])
        e = self.ebM.serialize()
        f = foundSet.serialize() if foundSet is not None else None
        return (e, len(e), arr, lens, len(self.bA)), (f, len(f) if f else 0)

    _COMPARE = "rbg_bsi_compare"  # the class's compare circuit

    def _compare(self, op, start, end, foundSet):
        index, found = self._operands(foundSet)
        return RoaringBitmap(call_bytes(getattr(lib(), self._COMPARE), op, int(start), int(end), *index,
                                        self.minValue, self.maxValue, *found))

    def compare(self, operation, startOrValue, end=0, foundSet=None):
        """BSI/:482-513 -> RoaringBitmap; the buffer package's index: BBSI/:422-453 -> ImmutableRoaringBitmap (as
        RoaringBitmap bytes)"""
        return self._compare(_lib.bsi_op(operation), startOrValue, end, foundSet)

    def sum(self, foundSet):
        """BSI/:581-592 -> (sum, count) as Java longs"""
        index, found = self._operands(foundSet)
        out = (ctypes.c_int64 * 2)()
        check(lib().rbg_bsi_sum(*index, *found, out))
        return int(out[0]), int(out[1])


class BitSliceIndexBase(RoaringBitmapSliceIndex):
    """The buffer package's index (BBSI/): the same fields, its own compare circuit
    (owenGreatEqual for GE and RANGE's lower bound, rangeEQ from and(ebM, foundSet), rangeNEQ
    against ebM) and ImmutableRoaringBitmap's result types (csrc/bsi.hip, k_bsi_buf)."""

    RANGE_NEQ_DIRECT = 7  # RBG_BSI_RANGE_NEQ_DIRECT
    _COMPARE = "rbg_bsi_compare_buffer"

    def add(self, otherBsi):
        """MutableBitSliceIndex.add (bsi/.../buffer/MutableBitSliceIndex.java:121-130, 201-262): for indexes
        without a run container the heap index's bytes (the mappeable containers' or / and / xor type rules
        are the heap's there), through the same fused pass.  With a run container it is refused:
        MappeableRunContainer's and keeps merged runs, and the buffer package's in-place xor over run
        containers is not established here."""
        if otherBsi is None or otherBsi.ebM.isEmpty():
            return
        if self._has_run() or otherBsi._has_run():
            raise IllegalArgumentException("add: a buffer index with a run container is not supported "
                                           "(the buffer package's in-place xor over run containers)")
        RoaringBitmapSliceIndex.add(self, otherBsi)

    def parallelIn(self, parallelism, foundSet, values, pool=None):
        """BBSI/:611-639 parallelIn(parallelism, foundSet, values, pool) -> ImmutableRoaringBitmap (as
        RoaringBitmap bytes): the columns of ebM, within foundSet unless it is None, whose value is in
        values (any iterable of ints), in one fused device pass (rbg_bsi_in, csrc/bsiin.hip).  pool is accepted
        and ignored: the device pass has no use for an executor, and the result does not depend on it;
        parallelism still decides parallelExec's batch size and with it whether a full container is a bitmap
        or a run container."""
        if int(parallelism) < 1:
            raise IllegalArgumentException("parallelIn: parallelism must be positive")
        if len(self.bA) > 32:
            raise IllegalArgumentException("parallelIn: an index holds at most 32 slices")
        v = _lib.in_list(values)
        index, found = self._operands(foundSet)
        return RoaringBitmap(call_bytes(lib().rbg_bsi_in, *index, *found,
                                        v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v.size, int(parallelism)))

    def parallelTransposeWithCount(self, foundSet, parallelism, pool=None):
        """BBSI/:551-597 parallelTransposeWithCount(foundSet, parallelism, pool) -> a new index of the same
        class: GROUP BY value / COUNT(*).  Its column ids are the distinct values of the columns of ebM, within
        foundSet unless it is None, and its values are how many columns held each; bitCount() is the bit
        length of the largest count, minValue / maxValue the smallest and largest count.  One device call
        (rbg_bsi_transpose, csrc/bsitr.hip).  pool is accepted and ignored, as in parallelIn; parallelism
        decides parallelExec's batch size and with it whether a full container of the result's ebM is a
        bitmap or a run container."""
        if int(parallelism) < 1:
            raise IllegalArgumentException("parallelTransposeWithCount: parallelism must be positive")
        if len(self.bA) > 32:
            raise IllegalArgumentException("parallelTransposeWithCount: an index holds at most 32 slices")
        index, found = self._operands(foundSet)
        return type(self)(*_index_call(lib().rbg_bsi_transpose, *index, *found, int(parallelism)))

    def rangeEQ(self, foundSet, predicate):  # BBSI/:351-375 (== compare(EQ))
        return self._compare(0, predicate, 0, foundSet)

    def rangeNEQ(self, foundSet, predicate):  # BBSI/:384-387
        return self._compare(self.RANGE_NEQ_DIRECT, predicate, 0, foundSet)

    def rangeLT(self, foundSet, predicate):  # BBSI/:389-391
        return self.compare("LT", predicate, 0, foundSet)

    def rangeLE(self, foundSet, predicate):  # BBSI/:393-395
        return self.compare("LE", predicate, 0, foundSet)

    def rangeGT(self, foundSet, predicate):  # BBSI/:397-399
        return self.compare("GT", predicate, 0, foundSet)

    def rangeGE(self, foundSet, predicate):  # BBSI/:401-403
        return self.compare("GE", predicate, 0, foundSet)

    def range(self, foundSet, start, end):  # BBSI/:405-408
        return self.compare("RANGE", start, end, foundSet)

    def sum(self, foundSet):
        """BBSI/:521-532 (the heap index's sum, BSI/:581-592); None or empty -> (0, 0)"""
        if foundSet is None or foundSet.isEmpty():
            return 0, 0
        return RoaringBitmapSliceIndex.sum(self, foundSet)


ImmutableBitSliceIndex = BitSliceIndexBase
MutableBitSliceIndex = BitSliceIndexBase
