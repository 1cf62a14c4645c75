"""Oracle of the range-encoded index, RB/RangeBitmap.java restated in Python / numpy.  Test-only.
RB/ = RoaringBitmap/src/main/java/org/roaringbitmap/.

Three parts, each following the reference's own control flow, not the package's:
  Appender   add one value at a time (:1511-1533), append (:1543-1588), serialize (:1483-1504)
  read       map (:65-85) and the record walk of skipContainer (:886-894)
  Replay     SingleEvaluation (:418-901) and DoubleEvaluation (:903-1281) with their `empty` / `full` flags
             (Bits, :1283-1357) carried from block to block as the reference carries them, the stream walked
             record by record; every result container typed by the reference's chain
             new BitmapContainer(bits, -1)[.iand(context)].repairAfterLazy().runOptimize()
"""
import struct

import numpy as np

import _fmt
import _oracle as O

M64 = (1 << 64) - 1
COOKIE = 0xF00D
BITMAP, RUN, ARRAY = 0, 1, 2  # :26-28
A, B, R = _fmt.A, _fmt.B, _fmt.R


def nlz(x):
    """Long.numberOfLeadingZeros"""
    return 64 - (x & M64).bit_length()


def runs_of_sorted(vals):
    """[(start, length - 1)] of ascending distinct ints"""
    out = []
    for v in vals:
        if out and out[-1][0] + out[-1][1] + 1 == v:
            out[-1][1] += 1
        else:
            out.append([v, 0])
    return out


# ---------------------------------------------------------------------------------------------------------
# Appender
# ---------------------------------------------------------------------------------------------------------
class Appender:
    def __init__(self, max_value):
        lz = nlz(max_value | 1)  # rangeMask, bytesPerMask (:1622-1630)
        self.range_mask = M64 >> lz
        self.bytes_per_mask = (64 - lz + 7) >> 3
        self.slices = [set() for _ in range(bin(self.range_mask).count("1"))]  # containerForSlice (:1608-1613)
        self.mask_buffer = bytearray()
        self.containers = bytearray()
        self.mask = 0
        self.rid = 0
        self.key = 0
        self.dirty = False

    def add(self, value):
        value &= M64
        if value & self.range_mask != value:
            raise ValueError(f"{value} too large")
        bits = ~value & self.range_mask
        self.mask |= bits
        while bits:
            index = (bits & -bits).bit_length() - 1  # numberOfTrailingZeros
            bits &= bits - 1
            self.slices[index].add(self.rid & 0xFFFF)  # (char) rid
        self.rid += 1
        self.dirty = True
        if self.rid >> 16 > self.key:
            self.append()

    def append(self):
        self.mask_buffer += self.mask.to_bytes(8, "little")[:self.bytes_per_mask]  # putLong, bufferPos += bytesPerMask
        for i, container in enumerate(self.slices):
            if not container:
                continue
            vals = sorted(container)
            card, runs = len(vals), runs_of_sorted(vals)
            if i < 5:  # a BitmapContainer: BitmapContainer.runOptimize (RB/BitmapContainer.java:1218-1237)
                kind = RUN if 8192 > 2 + 4 * len(runs) else BITMAP
            elif 2 + 4 * len(runs) <= min(8192, 2 + 2 * card):  # a RunContainer: toEfficientContainer (:2326-2335)
                kind = RUN
            else:
                kind = ARRAY if card <= 4096 else BITMAP
            self.containers.append(kind)
            if kind == RUN:  # RunContainer.writeArray: the run count, then the pairs
                self.containers += struct.pack("<H", len(runs))
                for s, l in runs:
                    self.containers += struct.pack("<HH", s, l)
            elif kind == BITMAP:
                self.containers += struct.pack("<H", card & 0xFFFF)  # (char) container.getCardinality()
                words = [0] * 1024
                for v in vals:
                    words[v >> 6] |= 1 << (v & 63)
                self.containers += struct.pack("<1024Q", *words)
            else:
                self.containers += struct.pack("<H", card) + struct.pack(f"<{card}H", *vals)
            container.clear()
        self.mask = 0
        self.key += 1
        self.dirty = False

    def flush(self):
        if self.dirty:
            self.append()

    def serialized_size(self):  # serializedSizeInBytes (:1458-1472)
        self.flush()
        return 10 + self.key * self.bytes_per_mask + len(self.containers)

    def serialize(self):
        self.flush()
        return (struct.pack("<HBBHI", COOKIE, 2, len(self.slices), self.key & 0xFFFF, self.rid & 0xFFFFFFFF)
                + bytes(self.mask_buffer) + bytes(self.containers))


def build(values, max_value=None):
    """the stream of the values, one row each"""
    values = [int(v) & M64 for v in values]
    app = Appender(max(values, default=0) if max_value is None else max_value)
    for v in values:
        app.add(v)
    return app.serialize()


# ---------------------------------------------------------------------------------------------------------
# reader
# ---------------------------------------------------------------------------------------------------------
class Index:
    """map (:65-85): the header, and the records as a flat list in stream order, each (type, size, rows)
    with rows a bool[65536]; position p of the evaluations is an index into that list."""

    def __init__(self, buf):
        cookie, base, self.slice_count, self.max_key, self.max = struct.unpack_from("<HBBHI", buf, 0)
        assert cookie == COOKIE and base == 2
        self.mask = M64 >> (64 - self.slice_count)
        self.bytes_per_mask = (self.slice_count + 7) >> 3
        pos = 10
        self.masks = []
        for _ in range(self.max_key):  # getContainerMask (:1359-1373) reads 1 / 2 / 4 / 8 bytes and masks them
            self.masks.append(int.from_bytes(buf[pos:pos + self.bytes_per_mask], "little") & self.mask)
            pos += self.bytes_per_mask
        self.records = []
        for m in self.masks:
            for _ in range(bin(m).count("1")):
                typ, size = struct.unpack_from("<BH", buf, pos)
                pos += 3
                rows = np.zeros(65536, dtype=bool)
                if typ == BITMAP:
                    rows = np.unpackbits(np.frombuffer(buf, dtype=np.uint8, count=8192, offset=pos),
                                         bitorder="little").astype(bool)
                    pos += 8192
                elif typ == RUN:
                    pr = np.frombuffer(buf, dtype="<u2", count=2 * size, offset=pos).astype(np.int64)
                    for s, l in zip(pr[0::2], pr[1::2]):
                        rows[s:s + l + 1] = True
                    pos += 4 * size
                else:
                    assert typ == ARRAY
                    rows[np.frombuffer(buf, dtype="<u2", count=size, offset=pos)] = True
                    pos += 2 * size
                self.records.append((typ, size, rows))
        self.consumed = pos

    def values(self):
        """the indexed values, one per row (slice i holds the rows whose bit i is clear)"""
        out = np.zeros(self.max, dtype=np.uint64)
        p = 0
        for k, m in enumerate(self.masks):
            n = min(self.max - 65536 * k, 65536)
            v = np.full(n, self.mask, dtype=np.uint64)
            for i in range(self.slice_count):
                if (m >> i) & 1:
                    v[self.records[p][2][:n]] &= np.uint64(~(1 << i) & M64)
                    p += 1
            out[65536 * k:65536 * k + n] = v
        return out


# ---------------------------------------------------------------------------------------------------------
# the typing chain
# ---------------------------------------------------------------------------------------------------------
def run_optimize(kind, rows):
    """Container.runOptimize of an array (RB/ArrayContainer.java:1085-1099), a bitmap
    (RB/BitmapContainer.java:1218-1237) or RunContainer.full() (toEfficientContainer keeps it)"""
    if kind == R:
        return R
    c = int(np.count_nonzero(rows))
    r = int(np.count_nonzero(rows[1:] & ~rows[:-1])) + int(rows[0])
    if kind == A:
        return R if 2 * c > 2 + 4 * r else A
    return R if 8192 > 2 + 4 * r else B


def type_container(bits, context=None):
    """new BitmapContainer(bits, -1)[.iand(context)].repairAfterLazy().runOptimize() -> (kind, rows) or None for
    an empty result, which is not appended (:443-446, :480-487).  context: (kind, rows) of the context's
    container; a lazy bitmap (cardinality -1) stays one through iand of an array, a bitmap or a run
    container (RB/BitmapContainer.java:523-598), so its kind never matters."""
    rows = bits.copy()
    if context is not None:
        rows &= context[1]
    c = int(np.count_nonzero(rows))  # repairAfterLazy (RB/BitmapContainer.java:1205-1215)
    kind = A if c <= 4096 else (R if c == 65536 else B)
    kind = run_optimize(kind, rows)
    return None if c == 0 else (kind, rows)


def to_bytes(result):
    """[(key, (kind, rows))] -> serialized bitmap"""
    return _fmt.encode([(k, kind, np.flatnonzero(rows)) for k, (kind, rows) in result])


def context_of(buf):
    """a serialized bitmap as {key: (kind, rows)}, keys ascending"""
    out = {}
    for key, kind, _card, vals, _nr in _fmt.decode(buf):
        rows = np.zeros(65536, dtype=bool)
        rows[vals] = True
        out[key] = (kind, rows)
    return out


def rows_of(result):
    return np.concatenate([65536 * k + np.flatnonzero(rows) for k, (_, rows) in result] or
                          [np.zeros(0, dtype=np.int64)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------
# SingleEvaluation
# ---------------------------------------------------------------------------------------------------------
class SingleEvaluation:
    def __init__(self, idx):
        self.idx = idx
        self.bits = np.zeros(65536, dtype=bool)
        self.position = 0
        self.empty = True

    # -- the walk
    def skip_container(self):
        self.position += 1

    def skip_containers(self, mask):
        self.position += bin(mask).count("1")

    def next_rows(self):
        rows = self.idx.records[self.position][2]
        self.position += 1
        return rows

    # -- :671-734
    def evaluate_range(self, remaining, threshold, cm):
        idx = self.idx
        skip = 64 - nlz(~(threshold | cm) & idx.mask)
        sl = 0
        if skip > 0:
            while sl < skip:
                if (cm >> sl) & 1:
                    self.skip_container()
                sl += 1
            if not self.empty:
                self.bits[:] = False
                self.empty = True
        else:
            if threshold & 1:
                if remaining >= 0x10000:
                    self.bits[:] = True
                else:
                    self.bits[:remaining] = True
                    if not self.empty:
                        self.bits[remaining:] = False
                if cm & 1:
                    self.skip_container()
                self.empty = False
            else:
                if not self.empty:
                    self.bits[:] = False
                    self.empty = True
                if cm & 1:
                    self.bits |= self.next_rows()
                    self.empty = False
            sl += 1
        while sl < idx.slice_count:
            if (cm >> sl) & 1:
                if (threshold >> sl) & 1:
                    self.bits |= self.next_rows()
                    self.empty = False
                elif self.empty:
                    self.skip_container()
                else:
                    self.bits &= self.next_rows()
            sl += 1

    # -- :736-770
    def evaluate_point(self, limit, value, cm):
        self.bits[:limit] = True
        self.bits[limit:] = False
        self.empty = False
        for sl in range(self.idx.slice_count):
            if (value >> sl) & 1:
                if (cm >> sl) & 1:
                    if self.empty:
                        self.skip_container()
                    else:
                        self.bits &= ~self.next_rows()
            else:
                if (cm >> sl) & 1:
                    if self.empty:
                        self.skip_container()
                    else:
                        self.bits &= self.next_rows()
                elif not self.empty:
                    self.bits[:limit] = False
                    self.empty = True

    def _above(self, t):
        return nlz(t) < nlz(self.idx.mask)

    # -- computePoint :426-495 / computeRange :551-618; point: negate, range: not upper
    def compute(self, point, t, flag, context=None):
        """-> ("range", max) | ("clone",) | ("typed", [(key, (kind, rows))])"""
        idx = self.idx
        flip = flag if point else not flag  # negate / !upper
        if context is not None and not context:
            return ("typed", [])
        if self._above(t):
            if flag:  # negate (:428, :460) / upper (:553, :584)
                return ("clone",) if context is not None else ("range", idx.max)
            return ("typed", [])
        out = []
        remaining = idx.max
        if context is None:
            key = 0
            while remaining > 0:
                cm = idx.masks[key]
                limit = min(remaining, 0x10000)
                if point:
                    self.evaluate_point(limit, t, cm)
                else:
                    self.evaluate_range(remaining, t, cm)
                if flip:
                    self.bits[:limit] ^= True
                    self.empty = False
                if not self.empty:
                    c = type_container(self.bits)
                    if c:
                        out.append((key, c))
                key += 1
                remaining -= 0x10000
            return ("typed", out)
        keys = sorted(context)
        cpos = 0
        prefix = 0
        while prefix <= keys[-1] and remaining > 0:
            cm = idx.masks[prefix]
            if prefix < keys[cpos]:
                self.skip_containers(cm)
            else:
                limit = min(remaining, 0x10000)
                if point:
                    self.evaluate_point(limit, t, cm)
                else:
                    self.evaluate_range(remaining, t, cm)
                if flip:
                    self.bits[:limit] ^= True
                    self.empty = False
                if not self.empty:
                    c = type_container(self.bits, context[keys[cpos]])
                    if c:
                        out.append((prefix, c))
                cpos += 1
            remaining -= 0x10000
            prefix += 1
        return ("typed", out)

    # -- countPoint :497-549 / countRange :620-669
    def count(self, point, t, flag, context=None, context_card=0):
        idx = self.idx
        if context is not None and not context:
            return 0
        if self._above(t):
            if flag:
                return context_card if context is not None else idx.max
            return 0
        count = 0
        remaining = idx.max
        if context is None:
            key = 0
            while remaining > 0:
                cm = idx.masks[key]
                limit = min(remaining, 0x10000)
                if point:
                    self.evaluate_point(limit, t, cm)
                    card = int(np.count_nonzero(self.bits[:limit]))
                    count += limit - card if flag else card
                else:
                    self.evaluate_range(remaining, t, cm)
                    card = int(np.count_nonzero(self.bits[:limit]))
                    count += card if flag else limit - card
                key += 1
                remaining -= 0x10000
            return count
        keys = sorted(context)
        cpos = 0
        prefix = 0
        while prefix <= keys[-1] and remaining > 0:
            limit = min(remaining, 0x10000)
            cm = idx.masks[prefix]
            if prefix < keys[cpos]:
                self.skip_containers(cm)
            else:
                crow = context[keys[cpos]][1]
                if point:
                    self.evaluate_point(limit, t, cm)
                    if flag:
                        self.bits[:limit] ^= True
                        self.empty = False
                    count += int(np.count_nonzero(crow & self.bits))  # container.andCardinality(bits)
                else:
                    self.evaluate_range(remaining, t, cm)
                    if flag:
                        count += int(np.count_nonzero(crow & self.bits))
                    else:  # container.andNot(bits).getCardinality() (:659-661): rows past max inside the key count
                        count += int(np.count_nonzero(crow & ~self.bits))
                cpos += 1
            remaining -= 0x10000
            prefix += 1
        return count


# ---------------------------------------------------------------------------------------------------------
# DoubleEvaluation
# ---------------------------------------------------------------------------------------------------------
class Bits:  # :1283-1357
    def __init__(self):
        self.bits = np.zeros(65536, dtype=bool)
        self.empty = True
        self.full = False

    def clear(self):
        if not self.empty:
            self.bits[:] = False
            self.empty, self.full = True, False

    def fill(self):
        if not self.full:
            self.bits[:] = True
            self.full, self.empty = True, False

    def reset(self, boundary):
        if not self.full:
            self.bits[:boundary] = True
        if not self.empty:
            self.bits[boundary:] = False
        self.empty = False
        self.full = False

    def flip(self, lo, hi):
        self.bits[lo:hi] ^= True
        if not self.full:
            if self.empty:
                self.full, self.empty = True, False
        else:
            self.empty, self.full = True, False

    def or_(self, rec):
        if is_full(rec):
            self.fill()
        elif not self.full:
            self.bits |= rec[2]
            self.empty = False

    def and_(self, rec):
        if not self.empty and not is_full(rec):
            self.bits &= rec[2]
            self.full = False


def is_full(rec):
    """MappeableContainer.isFull of a record as the evaluation constructs it: a bitmap from its size field (the
    cardinality as a char: a full one reads 0 and is not seen as full), an array never, a run container when
    it is the one run (0, 65535)"""
    typ, size, rows = rec
    if typ == RUN:
        return size == 1 and bool(rows.all())
    if typ == BITMAP:
        return size == 65536
    return False


class DoubleEvaluation:
    def __init__(self, idx):
        self.idx = idx
        self.low = Bits()
        self.high = Bits()
        self.position = 0

    def setup_first_slice(self, threshold, bits, remaining, copy):  # :1063-1076
        if threshold & 1:
            if remaining >= 0x10000:
                bits.fill()
            else:
                bits.reset(remaining)
        else:
            bits.clear()
            if copy:
                bits.or_(self.idx.records[self.position])  # orNextIntoBits(bits) leaves the position

    def evaluate(self, cm, remaining, lower, upper):  # :1016-1061
        mask = self.idx.mask
        skip_low = 64 - nlz(~(lower | cm) & mask)
        if skip_low == 64:
            lower = 0
        elif skip_low > 0:
            lower &= -(1 << skip_low) & M64
        skip_high = 64 - nlz(~(upper | cm) & mask)
        if skip_high == 64:
            upper = 0
        elif skip_high > 0:
            upper &= -(1 << skip_high) & M64
        self.setup_first_slice(upper, self.high, remaining, skip_high == 0)
        self.setup_first_slice(lower, self.low, remaining, skip_low == 0)
        if cm & 1:
            self.position += 1
        cm >>= 1
        upper >>= 1
        lower >>= 1
        while cm:
            if cm & 1:
                rec = self.idx.records[self.position]
                self.position += 1
                (self.low.or_ if lower & 1 else self.low.and_)(rec)
                (self.high.or_ if upper & 1 else self.high.and_)(rec)
            cm >>= 1
            upper >>= 1
            lower >>= 1
        self.low.flip(0, min(remaining, 0x10000))

    def _merged(self):
        """the bits compute / count go on with, or None (an empty side), or "full" """
        low, high = self.low, self.high
        if low.empty or high.empty:
            return None
        if low.full and high.full:
            return "full"
        if low.full:
            return high.bits
        if high.full:
            return low.bits
        low.bits &= high.bits  # compute ANDs into low, count into high: the same bits either way
        high.bits[:] = low.bits
        return low.bits

    def compute(self, lower, upper):  # :911-945
        idx = self.idx
        out = []
        remaining = idx.max
        key = 0
        while remaining > 0:
            self.evaluate(idx.masks[key], remaining, lower, upper)
            m = self._merged()
            if isinstance(m, str):
                out.append((key, (R, np.ones(65536, dtype=bool))))  # RunContainer.full()
            elif m is not None:
                c = type_container(m)
                if c:
                    out.append((key, c))
            key += 1
            remaining -= 0x10000
        return out

    def count(self, lower, upper, context=None):  # :947-1014
        idx = self.idx
        count = 0
        remaining = idx.max
        if context is None:
            key = 0
            while remaining > 0:
                self.evaluate(idx.masks[key], remaining, lower, upper)
                limit = min(remaining, 0x10000)
                m = self._merged()
                if isinstance(m, str):
                    count += limit
                elif m is not None:
                    count += int(np.count_nonzero(m[:limit]))
                key += 1
                remaining -= 0x10000
            return count
        keys = sorted(context)  # an empty context throws in the reference (keys[size - 1]); callers give 0
        cpos = 0
        prefix = 0
        while prefix <= keys[-1] and remaining > 0:
            cm = idx.masks[prefix]
            if prefix < keys[cpos]:
                self.position += bin(cm).count("1")
            else:
                self.evaluate(cm, remaining, lower, upper)
                crow = context[keys[cpos]][1]
                m = self._merged()
                if isinstance(m, str):
                    count += int(np.count_nonzero(crow))
                elif m is not None:
                    count += int(np.count_nonzero(crow & m))
                # contextPos is NOT advanced here (:990-1009, unlike :489, :543, :612, :663): every visited key
                # from the context's first one on is intersected with the context's FIRST container
            remaining -= 0x10000
            prefix += 1
        return count


# ---------------------------------------------------------------------------------------------------------
# the public forms (:111-416)
# ---------------------------------------------------------------------------------------------------------
def _finish(idx, res, context_buf):
    if res[0] == "range":
        return O.bitmap_of_range(0, res[1])  # RoaringBitmap.bitmapOfRange(0, max)
    if res[0] == "clone":
        return context_buf  # context.clone()
    return to_bytes(res[1])


def query_typed(idx, op, a, b=0, context_buf=None):
    """the serialized result of op, every container typed by the replayed chain"""
    ctx = None if context_buf is None else context_of(context_buf)
    a &= M64
    b &= M64
    above = lambda t: nlz(t) < nlz(idx.mask)  # noqa: E731
    if op == "between":
        assert ctx is None, "between(min, max, context) does not exist"
        if a == 0 or above(a):
            op, a = "lte", b
        elif above(b):
            op = "gte"
        else:
            return to_bytes(DoubleEvaluation(idx).compute(a - 1, b))
    if op == "lt":
        if a == 0:
            return to_bytes([])
        op, a = "lte", a - 1
    if op == "gte":
        if a == 0:
            return context_buf if ctx is not None else O.bitmap_of_range(0, idx.max)
        op, a = "gt", a - 1
    ev = SingleEvaluation(idx)
    point, flag = {"lte": (False, True), "gt": (False, False), "eq": (True, False), "neq": (True, True)}[op]
    return _finish(idx, ev.compute(point, a, flag, ctx), context_buf)


def query_count(idx, op, a, b=0, context_buf=None):
    ctx = None if context_buf is None else context_of(context_buf)
    ccard = 0 if ctx is None else sum(int(np.count_nonzero(r)) for _, r in ctx.values())
    a &= M64
    b &= M64
    above = lambda t: nlz(t) < nlz(idx.mask)  # noqa: E731
    if op == "between":
        if a == 0 or above(a):
            op, a = "lte", b
        elif above(b):
            op = "gte"
        else:
            if ctx is not None and not ctx:
                return 0
            return DoubleEvaluation(idx).count(a - 1, b, ctx)
    if op == "lt":
        if a == 0:
            return 0
        op, a = "lte", a - 1
    if op == "gte":
        if a == 0:
            return ccard if ctx is not None else idx.max
        op, a = "gt", a - 1
    point, flag = {"lte": (False, True), "gt": (False, False), "eq": (True, False), "neq": (True, True)}[op]
    return SingleEvaluation(idx).count(point, a, flag, ctx, ccard)


def brute_rows(values, max_rid, op, a, b=0, context_rows=None):
    """the rows a query selects, straight from the values (unsigned compare)"""
    v = np.asarray(values, dtype=np.uint64)
    a, b = np.uint64(a & M64), np.uint64(b & M64)
    sel = {"lte": lambda: v <= a, "lt": lambda: v < a, "gt": lambda: v > a, "gte": lambda: v >= a,
           "eq": lambda: v == a, "neq": lambda: v != a, "between": lambda: (v >= a) & (v <= b)}[op]()
    rows = np.flatnonzero(sel).astype(np.int64)
    if context_rows is not None:
        rows = np.intersect1d(rows, np.asarray(context_rows, dtype=np.int64))
    return rows


# ---------------------------------------------------------------------------------------------------------
# the fast model: what the replay comes to, computed from the values (test_rangebitmap_oracle.py holds it to
# the replay; the GPU tests use it, so that no test replays 64 slices block by block on the host)
# ---------------------------------------------------------------------------------------------------------
def plan(mask, op, a, b=0):
    """-> ("empty",) | ("all",) | (op', a', b') with op' in lte / gt / eq / neq / between: the derived forms
    (:111-119, :206-220, :294-308) and the thresholds above the mask (:427-429, :552-554)"""
    a &= M64
    b &= M64
    above = lambda t: nlz(t) < nlz(mask)  # noqa: E731
    if op == "between":
        if a == 0 or above(a):
            op, a = "lte", b
        elif above(b):
            op = "gte"
        else:
            return ("between", a, b)
    if op == "lt":
        if a == 0:
            return ("empty",)
        op, a = "lte", a - 1
    if op == "gte":
        if a == 0:
            return ("all",)
        op, a = "gt", a - 1
    if above(a):
        return ("all",) if op in ("lte", "neq") else ("empty",)
    return (op, a, 0)


def model_bytes(values, mask, op, a, b=0, context_buf=None):
    """the serialized result: a shortcut's own bytes, else O.from_values(rows, True)"""
    n = len(values)
    crows = None if context_buf is None else O.to_values(context_buf).astype(np.int64)
    p = plan(mask, op, a, b)
    if p == ("empty",) or (crows is not None and crows.size == 0):
        return O.from_values([], False)
    if p == ("all",):
        return context_buf if crows is not None else O.bitmap_of_range(0, n)
    return O.from_values(brute_rows(values, n, p[0], p[1], p[2], crows), True)


def model_count(values, mask, op, a, b=0, context_buf=None):
    n = len(values)
    crows = None if context_buf is None else O.to_values(context_buf).astype(np.int64)
    p = plan(mask, op, a, b)
    if p == ("empty",) or (crows is not None and crows.size == 0):
        return 0
    if p == ("all",):
        return int(crows.size) if crows is not None else n
    if crows is None or p[0] in ("lte", "eq", "neq"):
        return int(brute_rows(values, n, p[0], p[1], p[2], crows).size)
    n_blocks = (n + 0xFFFF) >> 16
    if p[0] == "gt":  # |context \ lte| over the visited keys (:659-661)
        visited = crows[(crows >> 16) < n_blocks]
        return int(visited.size - brute_rows(values, n, "lte", p[1], 0, crows).size)
    # between: every key from the context's first to its last against the context's FIRST container (:984-1012)
    k0, k1 = int(crows[0] >> 16), int(crows[-1] >> 16)
    first = crows[(crows >> 16) == k0] & 0xFFFF
    rows = brute_rows(values, n, "between", p[1], p[2])
    count = 0
    for k in range(k0, min(k1, n_blocks - 1) + 1):
        count += int(np.intersect1d(rows[(rows >> 16) == k] & 0xFFFF, first).size)
    return count
