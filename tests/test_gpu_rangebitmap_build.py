"""A range-encoded index built on the MI355X from a value tensor, and a resident one written back out
(rbg_ctx_rangebitmap_build[_device], rbg_ctx_rangebitmap_serialize, rbg_rangebitmap_build; RB/RangeBitmap.java:
Appender, :1378-1631).  Acceptance: rangebitmap_serialize(rangebitmap_build(values, max)) is byte for byte the
package Appender's stream (which test_rangebitmap_oracle.py pins to the oracle's), rangebitmap_info is that of the
loaded stream, and a built index answers every query as _rangebitmap.py's model does."""
import ctypes
import struct

import numpy as np
import pytest

import _oracle as O
import _rangebitmap as RBO

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
OPS1 = ("lte", "lt", "gt", "gte", "eq", "neq")
ROWS = (0, 1, 63, 64, 65, 65535, 65536, 65537, 3 * 65536 + 100)  # group edges, block edges, the cut last block
SLICES = (1, 5, 6, 8, 9, 33, 64)  # smallest; the 5 / 6 typing switch; masks of 1 -> 2 and 4 -> 5 bytes; widest


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dev(gpu):
    import torch
    return torch.device("cuda", 0)


def stream_of(values, max_value):
    import roaringbitmap_amd as rb
    app = rb.RangeBitmap.appender(max_value)
    app.add_many(np.asarray(values))
    return app.serialize()


def layout(n, slices, seed):
    """test_gpu_rangebitmap.py's recipe: n values under `slices` bits that make, where n and slices allow it:
    random (bitmap) low slices, array slices (few rows with a high bit clear), run slices (long stretches), a
    block with no container at all (block 1), a bitmap record of 3,000 scattered rows in slices 0-4 (block 2),
    a block whose mask lacks most slices and is cut (block 3)."""
    rng = np.random.default_rng(seed)
    mask = (1 << slices) - 1
    v = np.full(n, mask, dtype=np.uint64)
    lo = min(n, 65536)
    r = rng.integers(0, 1 << 63, lo, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, lo, dtype=np.uint64)
    keep_high = rng.random(lo) < 0.97  # the bits above 8 clear in 3 % of the rows: arrays in the high slices
    r = np.where(keep_high, r | np.uint64(mask & ~0xFF), r)
    v[:lo] = r & np.uint64(mask)
    v[30000:min(n, 40000)] = ((1 << (slices - 1)) | 5) & mask  # one value over 10,000 rows: runs
    if n > 65536:
        v[65536:min(n, 2 * 65536)] = mask  # no container
    if n > 2 * 65536:
        v[2 * 65536:2 * 65536 + 30000] = 0x1F & mask  # slices 5 and up: one long run
        # slices 0-4: 3,000 isolated rows and nothing else, a bitmap record of 3,000 values
        v[2 * 65536 + 30000 + 2 * rng.choice(17000, 3000, replace=False)] = np.uint64(mask & ~0x1F)
    if n > 3 * 65536:
        v[3 * 65536:] = rng.integers(0, 4, n - 3 * 65536, dtype=np.uint64) & np.uint64(mask)  # mask lacks the high slices
    return v


def thresholds(values, slices):
    mask = (1 << slices) - 1
    stored = int(values[len(values) // 3]) if len(values) else 5 & mask
    t = [0, 1, stored, max(stored - 1, 0), min(stored + 1, M64), mask, M64]
    if slices < 64:
        t.append(mask + 1)
    return sorted(set(t)), stored


def records_by_slice(buf):
    """[(block, slice, type, size)] of a stream"""
    idx = RBO.Index(buf)
    out, p = [], 0
    for k, m in enumerate(idx.masks):
        for i in range(idx.slice_count):
            if (m >> i) & 1:
                out.append((k, i, idx.records[p][0], idx.records[p][1]))
                p += 1
    return out


def check_build(eng, values, max_value, want=None):
    """build == Appender, byte for byte, and the info of the loaded stream; -> the stream"""
    want = stream_of(values, max_value) if want is None else want
    h = eng.rangebitmap_build(values, max_value)
    got = eng.rangebitmap_serialize(h)
    info = eng.rangebitmap_info(h)
    eng.rangebitmap_release(h)
    assert got == want, (len(values), max_value, len(got), len(want))
    loaded = eng.rangebitmap_load(want)
    assert info == eng.rangebitmap_info(loaded)
    eng.rangebitmap_release(loaded)
    return want


@pytest.mark.parametrize("slices", SLICES)
def test_row_counts_by_slice_count(eng, slices):
    for n in ROWS:
        check_build(eng, layout(n, slices, 1000 * slices + n % 997), (1 << slices) - 1)


@pytest.mark.parametrize("slices", [9, 33])
def test_mixed_values_make_every_record_type(eng, slices):
    """the recipe at the largest row count, seed 7: every (slice class, type) combination, an empty block and a
    block whose mask lacks most slices -- asserted from the expected stream, so that a recipe change cannot
    hollow the test out"""
    values = layout(ROWS[-1], slices, 7)
    want = check_build(eng, values, (1 << slices) - 1)
    recs = records_by_slice(want)
    seen = {("low" if i < 5 else "high", t) for _, i, t, _ in recs}
    assert seen == {("low", RBO.RUN), ("low", RBO.BITMAP), ("high", RBO.ARRAY), ("high", RBO.BITMAP), ("high", RBO.RUN)}
    assert any(i < 5 and t == RBO.BITMAP and s == 3000 for _, i, t, s in recs)  # a bitmap of at most 4,096 values
    idx = RBO.Index(want)
    assert idx.masks[1] == 0 and bin(idx.masks[3]).count("1") >= slices - 2 and bin(idx.masks[0]).count("1") == slices
    assert {i for k, i, _, _ in recs if k == 3} >= set(range(2, slices))  # values 0..3: every slice above 1 is full


def test_type_boundaries(eng):
    """one block, 6 slices; the record lists are the Appender's: 2,047 isolated rows in slice 0 are a run of
    2,047 and 2,048 in slice 1 a bitmap (2 + 4 r < 8192); in slice 5, 100 runs of length 2 are a run (the
    2 + 4 r == 2 + 2 c tie), 4,096 isolated rows an array and 4,097 a bitmap"""
    for high_rows, record in ((np.concatenate([4 * np.arange(100), 4 * np.arange(100) + 1]), (RBO.RUN, 100)),
                              (2 * np.arange(4096), (RBO.ARRAY, 4096)),
                              (2 * np.arange(4097), (RBO.BITMAP, 4097))):
        v = np.full(65536, 63, dtype=np.uint64)
        v[2 * np.arange(2047)] &= np.uint64(~1 & 63)
        v[3 * np.arange(2048)] &= np.uint64(~2 & 63)
        v[high_rows] &= np.uint64(~32 & 63)
        want = check_build(eng, v, 63)
        assert [(i, t, s) for _, i, t, s in records_by_slice(want)] == \
            [(0, RBO.RUN, 2047), (1, RBO.BITMAP, 2048), (5,) + record]


def test_extreme_and_full_cases(eng):
    full = check_build(eng, np.zeros(65536 + 10, dtype=np.uint64), 63)  # every slice full: one run each
    assert [(t, s) for _, _, t, s in records_by_slice(full)] == [(RBO.RUN, 1)] * 12
    top = check_build(eng, np.full(70000, 1000, dtype=np.uint64), 1000)  # values equal to maxValue
    assert RBO.Index(top).slice_count == 10 and RBO.Index(top).masks == [23, 23]  # ~1000 & 1023
    none = check_build(eng, np.full(70000, 1023, dtype=np.uint64), 1023)  # equal to the mask: no record at all
    assert records_by_slice(none) == [] and len(none) == 10 + 2 * 2
    zero = check_build(eng, np.zeros(100, dtype=np.uint64), 0)  # maxValue 0: one slice
    assert RBO.Index(zero).slice_count == 1
    wide = check_build(eng, np.array([0, 1 << 63, M64], dtype=np.uint64), M64)
    assert RBO.Index(wide).slice_count == 64
    neg = np.array([-1, -(1 << 63), 5, -12345, 0], dtype=np.int64)  # int64 as its bit pattern
    check_build(eng, neg, M64, stream_of(neg.view(np.uint64), M64))
    check_build(eng, neg, -1, stream_of(neg.view(np.uint64), M64))  # a negative maxValue is its pattern too


def test_max_value_from_the_data(eng):
    rng = np.random.default_rng(5)
    for v in (rng.integers(0, 1 << 27, 70000, dtype=np.uint64), np.array([-3, 7], dtype=np.int64),
              np.zeros(5, dtype=np.uint64), np.zeros(0, dtype=np.uint64)):
        u = v.view(np.uint64) if v.dtype == np.int64 else v
        check_build(eng, v, None, stream_of(u, int(u.max()) if u.size else 0))


def test_forced_passes_give_the_same_bytes(eng, monkeypatch):
    """RBG_RB_BUILD_WS: one block per pass, a budget below one block (still one block), two blocks and a bit
    (passes of 2 + 2), and the default again"""
    slices = 9
    values = layout(ROWS[-1], slices, 7)
    want = check_build(eng, values, 511)
    for budget in (8192 * slices, 1, 2 * 8192 * slices + 100):
        monkeypatch.setenv("RBG_RB_BUILD_WS", str(budget))
        check_build(eng, values, 511, want)
    monkeypatch.delenv("RBG_RB_BUILD_WS")
    check_build(eng, values, 511, want)


class Built:
    """an index built on the engine, with the model's view of it"""

    def __init__(self, eng, values, slices):
        self.eng, self.values = eng, np.asarray(values, dtype=np.uint64)
        self.h = eng.rangebitmap_build(self.values, (1 << slices) - 1)
        info = eng.rangebitmap_info(self.h)
        self.mask = info["mask"]
        assert info["rows"] == len(self.values) and self.mask == (1 << slices) - 1

    def check(self, op, a, b=0, ctx=None, ctx_buf=None, bitmap=True):
        if bitmap:
            out = self.eng.rangebitmap_query(self.h, op, a, b, ctx)
            got = self.eng.batch_fetch(out).serialize()
            self.eng.release(out)
            assert got == RBO.model_bytes(self.values, self.mask, op, a, b, ctx_buf), (op, a, b)
        got = self.eng.rangebitmap_count(self.h, op, a, b, ctx)
        assert got == RBO.model_count(self.values, self.mask, op, a, b, ctx_buf), (op, a, b, "count")


@pytest.mark.parametrize("slices", [9, 33])
def test_queries_over_a_built_index(eng, slices):
    """every op and its cardinality at the thresholds, with and without one context; the handle released and a
    new one built in its place"""
    values = layout(ROWS[-1], slices, 7)
    r = Built(eng, values, slices)
    ts, stored = thresholds(values, slices)
    top = (1 << slices) - 1
    rng = np.random.default_rng(3)
    cbuf = O.from_values(np.concatenate([rng.choice(65536, 3000, replace=False), 65536 + np.arange(500, 42000),
                                         2 * 65536 + rng.choice(65536, 30000, replace=False),
                                         3 * 65536 + np.arange(50, 300)]), True)
    cid = eng.load_pair(cbuf)[0]
    for ctx, buf in ((None, None), (cid, cbuf)):
        for op in OPS1:
            for t in ts:
                r.check(op, t, 0, ctx, buf)
        for a, b in ((0, stored), (stored, stored), (1, top), (stored, M64), (min(stored + 1, M64), stored), (2, 3)):
            r.check("between", a, b, ctx, buf, bitmap=ctx is None)
    eng.release(cid)
    eng.rangebitmap_release(r.h)
    other = layout(65537, 6, 3)
    r2 = Built(eng, other, 6)
    assert r2.h == r.h  # takes the freed handle
    r2.check("between", 3, 40)
    r2.check("neq", int(other[3]))
    eng.rangebitmap_release(r2.h)


def test_close_with_an_index_alive(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    h = e.rangebitmap_build(layout(65537, 9, 2), 511)
    assert e.rangebitmap_count(h, "gte", 0) == 65537
    e.close()


def _first_free(eng):
    """the lowest free batch slot and index handle: a leaked one would take it"""
    b = eng.from_values([1])
    eng.release(b)
    h = eng.rangebitmap_build(np.zeros(1, dtype=np.uint64), 1)
    eng.rangebitmap_release(h)
    return b, h


def test_a_value_outside_the_mask_builds_nothing(eng):
    import roaringbitmap_amd as rb
    from roaringbitmap_amd import _lib as L
    v = layout(2 * 65536, 9, 4)
    good = stream_of(v, 511)
    free = _first_free(eng)
    evictions = L.lib().rbg_pool_evictions()
    bad = v.copy()
    bad[-1] = 512  # one above the mask, in the last row of the second block
    with pytest.raises(rb.IllegalArgumentException, match="512 too large"):
        eng.rangebitmap_build(bad, 511)
    with pytest.raises(rb.IllegalArgumentException, match="too large"):
        eng.rangebitmap_build(np.array([M64], dtype=np.uint64), (1 << 63) - 1)
    assert _first_free(eng) == free and L.lib().rbg_pool_evictions() == evictions
    check_build(eng, v, 511, good)  # the engine works as before
    check_build(eng, bad, None, stream_of(bad, 512))  # and the same values fit their own maximum
    with pytest.raises(ValueError):
        eng.rangebitmap_build(np.zeros(4, dtype=np.float64))
    with pytest.raises(rb.IllegalArgumentException, match="no such index"):
        eng.rangebitmap_serialize(12345)
    assert _first_free(eng) == free


def test_torch_tensors_are_read_in_place(eng, dev):
    import torch
    values = layout(65537 + 64, 33, 9)
    want = stream_of(values, (1 << 33) - 1)
    t = torch.from_numpy(values.view(np.int64)).to(dev)
    strided = torch.stack([t, t + 1], dim=1)[:, 0]
    assert not strided.is_contiguous() and t.is_contiguous()
    for x in (t, strided, t.reshape(-1, 3)):  # flat, a strided view (made contiguous), two dimensions
        h = eng.rangebitmap_build(x, (1 << 33) - 1)
        assert eng.rangebitmap_serialize(h) == want
        eng.rangebitmap_release(h)
    h = eng.rangebitmap_build(t[:0], 7)
    assert eng.rangebitmap_info(h)["rows"] == 0 and eng.rangebitmap_serialize(h) == stream_of([], 7)
    eng.rangebitmap_release(h)
    with pytest.raises(ValueError):
        eng.rangebitmap_build(t.to(torch.int32))
    with pytest.raises(ValueError):
        eng.rangebitmap_build(t.cpu())


def test_round_trips(eng):
    """a loaded index of records the Appender cannot write serializes to its own bytes (trailing bytes are not
    part of it); the one-shot forms agree with the host default"""
    import roaringbitmap_amd as rb
    from roaringbitmap_amd import _lib as L
    full = b"\x00" + struct.pack("<H", 0) + b"\xff" * 8192
    few_rows = np.array([1, 64, 4097, 40000, 65535])
    few = b"\x00" + struct.pack("<H", 5) + np.packbits(np.isin(np.arange(65536), few_rows), bitorder="little").tobytes()
    arr_rows = np.arange(7, 30000, 11)
    arr = b"\x02" + struct.pack("<H", arr_rows.size) + arr_rows.astype("<u2").tobytes()
    head = struct.pack("<HBBHI", 0xF00D, 2, 3, 3, 2 * 65536 + 40)
    buf = head + bytes([0b111, 0b011, 0b100]) + arr + full + few + b"\x02\x00\x00" + full + b"\x01\x00\x00"
    assert RBO.Index(buf).consumed == len(buf)
    for given in (buf, buf + b"trailing"):
        h = eng.rangebitmap_load(given)
        assert eng.rangebitmap_serialize(h) == buf
        eng.rangebitmap_release(h)
    values = layout(65537, 9, 4)
    host = rb.RangeBitmap.from_values(values, 511)
    assert host.serialize() == stream_of(values, 511)
    assert rb.RangeBitmap.from_values(values, 511, gpu=True).serialize() == host.serialize()
    assert rb.RangeBitmap.from_values(values, gpu=True).serialize() == rb.RangeBitmap.from_values(values).serialize()
    got = L.call_bytes(L.lib().rbg_rangebitmap_build, ctypes.c_void_p(values.ctypes.data), values.size, 511, 0)
    assert got == host.serialize()
    with pytest.raises(rb.IllegalArgumentException, match="too large"):
        rb.RangeBitmap.from_values(values, 255, gpu=True)
    assert rb.RangeBitmap.from_values(values, gpu=True).lteCardinality(5) == int(np.count_nonzero(values <= 5))
