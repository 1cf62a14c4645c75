"""RangeBitmap (RB/RangeBitmap.java): a range-encoded index over one unsigned 64-bit value per row.

The Appender is host code in numpy and writes the reference's stream byte for byte (Appender.serialize,
:1483-1504; append, :1543-1588): slice i of a block of 65,536 rows holds the rows whose value has bit i
CLEAR, slices 0-4 are run containers iff 2 + 4 r < 8192 and bitmaps of any cardinality otherwise
(BitmapContainer.runOptimize), slices 5 and up follow RunContainer.toEfficientContainer, and a bitmap
record's size field is the cardinality as a Java char (65,536 stored as 0).

The queries run on the device, one wave per block (rbg_rangebitmap_query / rbg_rangebitmap_count, the
one-shot forms: the index is mapped for the call), as RoaringBitmap.and_ does; Engine.rangebitmap_load /
rangebitmap_query / rangebitmap_count keep an index resident.  Values and thresholds are compared as
unsigned 64-bit numbers: a negative Python int is taken as its 64-bit pattern, as a Java long is.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import IllegalArgumentException, call_bytes, check, lib
from .roaring import RoaringBitmap

_M64 = (1 << 64) - 1
COOKIE = 0xF00D
BITMAP, RUN, ARRAY = 0, 1, 2  # :26-28


def _u64(x) -> int:
    return int(x) & _M64


def _record(present: np.ndarray, run_first: bool) -> bytes:
    """One container record of a slice: present is the block's 65,536 rows as booleans, at least one set.
    run_first: the slice is a BitmapContainer (slices 0-4), typed by BitmapContainer.runOptimize; else a
    RunContainer, typed by toEfficientContainer (RB/RunContainer.java:2326-2335)."""
    card = int(np.count_nonzero(present))
    edge = np.diff(present.astype(np.int8), prepend=np.int8(0), append=np.int8(0))
    starts = np.flatnonzero(edge == 1)
    nruns = int(starts.size)
    if run_first:
        kind = RUN if 2 + 4 * nruns < 8192 else BITMAP
    elif 2 + 4 * nruns <= min(8192, 2 + 2 * card):
        kind = RUN
    else:
        kind = ARRAY if card <= 4096 else BITMAP
    if kind == RUN:
        ends = np.flatnonzero(edge == -1)  # one past each run
        pairs = np.empty(2 * nruns, dtype="<u2")
        pairs[0::2] = starts
        pairs[1::2] = ends - starts - 1
        return bytes([RUN]) + int(nruns).to_bytes(2, "little") + pairs.tobytes()
    if kind == BITMAP:
        words = np.packbits(present, bitorder="little").tobytes()
        return bytes([BITMAP]) + (card & 0xFFFF).to_bytes(2, "little") + words
    return bytes([ARRAY]) + card.to_bytes(2, "little") + np.flatnonzero(present).astype("<u2").tobytes()


class Appender:
    """RangeBitmap.Appender (:1378-1631)."""

    def __init__(self, maxValue):
        bits = max(_u64(maxValue) | 1, 1).bit_length()  # rangeMask / bytesPerMask of maxValue | 1 (:1622-1630)
        self._nslices = bits
        self._range_mask = _M64 >> (64 - bits)
        self._bytes_per_mask = (bits + 7) >> 3
        self._pending = []  # values (uint64 arrays) of the rows since the last append()
        self._pending_rid = 0  # the row id of the first of them
        self.clear()

    def clear(self):
        """clear() (:1443-1451)"""
        self._masks = bytearray()
        self._containers = bytearray()
        self._pending = []
        self._rid = 0
        self._pending_rid = 0
        self._key = 0
        self._dirty = False

    def add(self, value):
        """add(long) (:1511-1533): the value of the next row; IllegalArgumentException("... too large")
        for a value outside the mask."""
        v = _u64(value)
        if v & self._range_mask != v:
            raise IllegalArgumentException(f"{int(value)} too large")
        self._take(np.array([v], dtype=np.uint64))

    def add_many(self, values):
        """add(long) for every element of a numpy array (uint64, or int64 taken as its bit pattern), in
        order; a value outside the mask raises after the values before it were added, as a loop would."""
        v = np.asarray(values)
        if v.dtype.kind == "i":
            v = v.astype(np.int64).view(np.uint64)
        v = np.ascontiguousarray(v.astype(np.uint64, copy=False)).reshape(-1)
        bad = np.flatnonzero((v & np.uint64(self._range_mask)) != v)
        if bad.size:
            self._take(v[:bad[0]])
            raise IllegalArgumentException(f"{int(v[bad[0]])} too large")
        self._take(v)

    def _take(self, v):
        while v.size:
            room = ((self._key + 1) << 16) - self._rid  # append() follows the row that makes rid >>> 16 > key
            if room <= 0:  # rid is an int in the reference and wraps; no index has 2^32 rows
                raise IllegalArgumentException("too many rows")
            part, v = v[:room], v[room:]
            self._pending.append(part)
            self._rid += int(part.size)
            self._dirty = True
            if self._rid >> 16 > self._key:
                self._append()

    def _append(self):
        """append() (:1543-1588): the mask and the non-empty slices of the rows since the last one"""
        vals = np.concatenate(self._pending) if self._pending else np.zeros(0, dtype=np.uint64)
        pos = (self._pending_rid + np.arange(vals.size, dtype=np.int64)) & 0xFFFF  # (char) rid
        clear = ~vals & np.uint64(self._range_mask)
        mask = int(np.bitwise_or.reduce(clear)) if vals.size else 0
        self._masks += mask.to_bytes(8, "little")[:self._bytes_per_mask]
        for i in range(self._nslices):
            if not (mask >> i) & 1:
                continue
            present = np.zeros(65536, dtype=bool)
            present[pos[(clear >> np.uint64(i)) & np.uint64(1) != 0]] = True
            self._containers += _record(present, i < 5)
        self._pending = []
        self._pending_rid = self._rid
        self._key += 1
        self._dirty = False

    def _flush(self) -> bool:
        if self._dirty:
            self._append()
            return True
        return False

    def serializedSizeInBytes(self) -> int:
        """serializedSizeInBytes() (:1458-1472); flushes the rows of an unfinished block"""
        self._flush()
        return 10 + self._key * self._bytes_per_mask + len(self._containers)

    def serialize(self) -> bytes:
        """serialize(ByteBuffer) (:1483-1504) -> the stream.  The reference throws IllegalStateException when
        rows were added since serializedSizeInBytes(); here the size is a property of the bytes returned,
        so the flush happens in this call."""
        self._flush()
        head = (COOKIE.to_bytes(2, "little") + bytes([2, self._nslices]) + (self._key & 0xFFFF).to_bytes(2, "little")
                + (self._rid & 0xFFFFFFFF).to_bytes(4, "little"))
        return head + bytes(self._masks) + bytes(self._containers)

    def build(self):
        """build() (:1415-1438) -> RangeBitmap"""
        return RangeBitmap.map(self.serialize())


class RangeBitmap:
    """A mapped range-encoded index (RB/RangeBitmap.java).  The thresholds are unsigned 64-bit numbers."""

    def __init__(self, buffer: bytes):
        self._buf = bytes(buffer)
        info = (ctypes.c_uint64 * 6)()
        check(lib().rbg_rangebitmap_validate(self._buf, len(self._buf), info))
        self.sliceCount, self.maxKey, self.maxRid, self.mask = int(info[0]), int(info[1]), int(info[2]), int(info[3])
        self._buf = self._buf[:int(info[5])]

    @staticmethod
    def appender(maxValue) -> Appender:
        """appender(long maxValue) (:52-56)"""
        return Appender(maxValue)

    @classmethod
    def from_values(cls, values, maxValue=None, gpu=False):
        """appender(maxValue), add for every value of a numpy array (uint64, or int64 taken as its bit pattern)
        in order, build -> RangeBitmap.  maxValue=None: the largest value given.  The host default runs the
        Appender; gpu=True builds and serializes on the device (rbg_rangebitmap_build), the same bytes.  A value
        outside the mask raises IllegalArgumentException."""
        v = np.asarray(values)
        if v.dtype.kind == "i":
            v = v.astype(np.int64).view(np.uint64)
        v = np.ascontiguousarray(v.astype(np.uint64, copy=False)).reshape(-1)
        if not gpu:
            app = Appender(int(v.max()) if maxValue is None and v.size else (maxValue or 0))
            app.add_many(v)
            return app.build()
        return cls(call_bytes(lib().rbg_rangebitmap_build, ctypes.c_void_p(v.ctypes.data) if v.size else None, v.size,
                              0 if maxValue is None else _u64(maxValue), int(maxValue is None)))

    @classmethod
    def map(cls, buffer):
        """map(ByteBuffer) (:65-85): validated on the host (InvalidRoaringFormat / TruncatedInput)"""
        return cls(buffer)

    def serialize(self) -> bytes:
        return self._buf

    def _ctx(self, context):
        if context is None:
            return None, 0
        b = context.serialize() if isinstance(context, RoaringBitmap) else bytes(context)
        return b, len(b)

    def _query(self, op, a, b=0, context=None) -> RoaringBitmap:
        cb, cl = self._ctx(context)
        return RoaringBitmap(call_bytes(lib().rbg_rangebitmap_query, self._buf, len(self._buf),
                                        _lib.RANGEBITMAP_OP[op], _u64(a), _u64(b), cb, cl))

    def _count(self, op, a, b=0, context=None) -> int:
        cb, cl = self._ctx(context)
        out = ctypes.c_int64()
        check(lib().rbg_rangebitmap_count(self._buf, len(self._buf), _lib.RANGEBITMAP_OP[op], _u64(a), _u64(b), cb, cl,
                                          ctypes.byref(out)))
        return out.value

    def between(self, min, max) -> RoaringBitmap:  # noqa: A002 (the reference's names)
        """between(min, max) (:111-119), both inclusive; there is no form with a context"""
        return self._query("between", min, max)

    def betweenCardinality(self, min, max, context=None) -> int:  # noqa: A002
        """betweenCardinality(min, max[, context]) (:128-154)"""
        return self._count("between", min, max, context)

    def lte(self, threshold, context=None) -> RoaringBitmap:
        """lte(threshold[, context]) (:162-176)"""
        return self._query("lte", threshold, 0, context)

    def lteCardinality(self, threshold, context=None) -> int:
        """lteCardinality (:184-198)"""
        return self._count("lte", threshold, 0, context)

    def lt(self, threshold, context=None) -> RoaringBitmap:
        """lt (:206-220)"""
        return self._query("lt", threshold, 0, context)

    def ltCardinality(self, threshold, context=None) -> int:
        """ltCardinality (:228-242)"""
        return self._count("lt", threshold, 0, context)

    def gt(self, threshold, context=None) -> RoaringBitmap:
        """gt (:250-264)"""
        return self._query("gt", threshold, 0, context)

    def gtCardinality(self, threshold, context=None) -> int:
        """gtCardinality (:272-286)"""
        return self._count("gt", threshold, 0, context)

    def gte(self, threshold, context=None) -> RoaringBitmap:
        """gte (:294-308)"""
        return self._query("gte", threshold, 0, context)

    def gteCardinality(self, threshold, context=None) -> int:
        """gteCardinality (:316-330)"""
        return self._count("gte", threshold, 0, context)

    def eq(self, value, context=None) -> RoaringBitmap:
        """eq (:338-351)"""
        return self._query("eq", value, 0, context)

    def eqCardinality(self, value, context=None) -> int:
        """eqCardinality (:359-373)"""
        return self._count("eq", value, 0, context)

    def neq(self, value, context=None) -> RoaringBitmap:
        """neq (:381-394)"""
        return self._query("neq", value, 0, context)

    def neqCardinality(self, value, context=None) -> int:
        """neqCardinality (:402-416)"""
        return self._count("neq", value, 0, context)
