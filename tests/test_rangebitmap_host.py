"""The range-encoded index (RB/RangeBitmap.java) without a device: the symbols of its entry points, the
refusals they decide from their arguments before any device use, and the host parser's error codes on bad
and cut streams (rangebitmap_format.cpp through rbg_rangebitmap_validate)."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L

import _rangebitmap as RBO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x_rangebitmap.h")
SYMBOLS = ["rbg_rangebitmap_validate", "rbg_ctx_rangebitmap_load", "rbg_ctx_rangebitmap_release",
           "rbg_ctx_rangebitmap_info", "rbg_ctx_rangebitmap_query", "rbg_ctx_rangebitmap_count", "rbg_rangebitmap_query",
           "rbg_rangebitmap_count"]
OK, INVALID, TRUNCATED, ILLEGAL = L.RBG_OK, L.RBG_ERR_INVALID_FORMAT, L.RBG_ERR_TRUNCATED, L.RBG_ERR_ILLEGAL_ARGUMENT


def test_symbols_exported_declared_and_typed():
    lib = ctypes.CDLL(L.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    main = open(os.path.join(ROOT, "include", "roaring_mi355x.h")).read()
    assert '#include "roaring_mi355x_rangebitmap.h"' in main
    assert sorted(set(re.findall(r"\b(rbg_\w+)\s*\(", src))) == sorted(SYMBOLS)
    assert sorted(L.RANGEBITMAP_SIGNATURES) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(L.lib(), name).argtypes is not None, name
    # the ops in the header's order, and every entry citing its Java lines
    for name, code in L.RANGEBITMAP_OP.items():
        assert re.search(rf"RBG_RB_{name.upper()} = {code}\b", src), name
    text = open(HEADER).read()
    for name in SYMBOLS[4:]:
        before = text[:text.index(f"int {name}(")]
        assert re.search(r":\d+-\d+", before[before.rindex("/*"):]), name
    from roaringbitmap_amd import _build
    assert {"rangebitmap.hip", "rangebitmap_format.cpp", "engine_rangebitmap.cpp"} <= set(_build.SOURCES)
    for f in ("rangebitmap_load", "rangebitmap_release", "rangebitmap_query", "rangebitmap_count"):
        assert callable(getattr(rb.Engine, f))
    for f in ("map", "appender", "lte", "lt", "gt", "gte", "eq", "neq", "between", "lteCardinality", "ltCardinality",
              "gtCardinality", "gteCardinality", "eqCardinality", "neqCardinality", "betweenCardinality"):
        assert callable(getattr(rb.RangeBitmap, f)), f


def _err():
    return L.lib().rbg_last_error().decode()


def test_refusals_come_before_any_device_use():
    """an unknown op and between(min, max, context) in the bitmap-returning form are RBG_ERR_ILLEGAL_ARGUMENT
    with their own text, decided before the handle or the stream is looked at"""
    lib = L.lib()
    stream = RBO.build([1, 2, 3], 3)
    ctx = rb.RoaringBitmap.bitmapOf(1).serialize()
    out = ctypes.c_int32(-7)
    cnt = ctypes.c_int64(-7)
    b = L.rbg_buffer()
    for op in (-1, 7, 100):
        assert lib.rbg_ctx_rangebitmap_query(None, 0, op, 1, 2, -1, 0, ctypes.byref(out)) == ILLEGAL and "unknown op" in _err()
        assert lib.rbg_ctx_rangebitmap_count(None, 0, op, 1, 2, -1, 0, ctypes.byref(cnt)) == ILLEGAL and "unknown op" in _err()
        assert lib.rbg_rangebitmap_query(stream, len(stream), op, 1, 2, None, 0, ctypes.byref(b)) == ILLEGAL
        assert "unknown op" in _err()
        assert lib.rbg_rangebitmap_count(stream, len(stream), op, 1, 2, None, 0, ctypes.byref(cnt)) == ILLEGAL
    between = L.RANGEBITMAP_OP["between"]
    assert lib.rbg_ctx_rangebitmap_query(None, 0, between, 1, 2, 0, 0, ctypes.byref(out)) == ILLEGAL
    assert "between(min, max, context) does not exist" in _err()
    assert lib.rbg_rangebitmap_query(stream, len(stream), between, 1, 2, ctx, len(ctx), ctypes.byref(b)) == ILLEGAL
    assert "between(min, max, context) does not exist" in _err()
    # good arguments, no handle / no output
    assert lib.rbg_ctx_rangebitmap_query(None, 0, 0, 1, 0, -1, 0, ctypes.byref(out)) == ILLEGAL
    assert lib.rbg_ctx_rangebitmap_count(None, 0, between, 1, 2, 0, 0, ctypes.byref(cnt)) == ILLEGAL  # the null handle
    assert lib.rbg_ctx_rangebitmap_load(None, stream, len(stream), ctypes.byref(out)) == ILLEGAL
    assert lib.rbg_ctx_rangebitmap_release(None, 0) == ILLEGAL
    assert lib.rbg_rangebitmap_query(stream, len(stream), 0, 1, 0, None, 0, None) == ILLEGAL
    assert lib.rbg_rangebitmap_count(stream, len(stream), 0, 1, 0, None, 0, None) == ILLEGAL
    assert out.value == -7 and cnt.value == -7 and not b.data
    r = rb.RangeBitmap.map(stream)
    with pytest.raises(rb.IllegalArgumentException, match="does not exist"):
        r._query("between", 1, 2, rb.RoaringBitmap.bitmapOf(1))
    with pytest.raises(TypeError):
        r.between(1, 2, rb.RoaringBitmap.bitmapOf(1))  # the reference has no such method


def validate(buf):
    info = (ctypes.c_uint64 * 6)()
    st = L.lib().rbg_rangebitmap_validate(bytes(buf), len(buf), info)
    return st, [int(x) for x in info]


def small_stream():
    """two blocks; array, bitmap and run records; masks that lack slices"""
    rng = np.random.default_rng(3)
    v = np.where(rng.random(65536 + 50) < 0.03, rng.integers(0, 1 << 9, 65536 + 50), 511)
    v[:3000] &= 0x1F0
    v[10000:20000:2] &= 0x1FE  # slice 0: thousands of runs, a bitmap record
    return RBO.build(v, 511)


def test_a_valid_stream_and_its_facts():
    buf = small_stream()
    idx = RBO.Index(buf)
    assert {t for t, _, _ in idx.records} == {RBO.BITMAP, RBO.RUN, RBO.ARRAY}
    st, info = validate(buf)
    assert st == OK and info[:4] == [9, 2, 65536 + 50, 511] and info[5] == len(buf) == idx.consumed
    assert validate(buf + b"trailing")[0] == OK  # map() reads what the header announces, nothing after it
    r = rb.RangeBitmap.map(buf + b"xx")
    assert (r.sliceCount, r.maxKey, r.maxRid, r.mask) == (9, 2, 65536 + 50, 511) and r.serialize() == buf
    assert validate(RBO.Appender(77).serialize()) == (OK, [7, 0, 0, 127, 0, 10])
    for slices in (1, 8, 9, 24, 25, 33, 64):  # the mask widths
        buf = RBO.build([0, (1 << slices) - 1, 1], (1 << slices) - 1)
        st, info = validate(buf)
        assert st == OK and info[0] == slices and info[5] == len(buf), slices


def test_parser_error_codes():
    buf = bytearray(small_stream())
    for pos, val, what in [(0, 0x0E, "cookie"), (1, 0xF1, "cookie"), (2, 1, "base"), (2, 3, "base"), (3, 0, "slice count"),
                           (3, 65, "slice count"), (3, 255, "slice count")]:
        bad = bytearray(buf)
        bad[pos] = val
        assert validate(bad)[0] == INVALID, what
        with pytest.raises(rb.InvalidRoaringFormat):
            rb.RangeBitmap.map(bytes(bad))
    bad = bytearray(buf)
    first_record = 10 + 2 * 2
    assert bad[first_record] in (0, 1, 2)
    for typ in (3, 0x7F, 0xFF):
        bad[first_record] = typ
        assert validate(bad)[0] == INVALID and "Unknown type" in _err()
    # maxKey against ceil(maxRid / 65536)
    for max_key, max_rid in ((1, 65536 + 50), (3, 65536 + 50), (2, 65536), (2, 2 * 65536 + 1), (0, 1)):
        bad = bytearray(buf)
        bad[4:10] = struct.pack("<HI", max_key, max_rid)
        assert validate(bad)[0] == INVALID, (max_key, max_rid)
    # an empty index must have no block
    assert validate(struct.pack("<HBBHI", 0xF00D, 2, 5, 0, 0))[0] == OK
    assert validate(struct.pack("<HBBHI", 0xF00D, 2, 5, 1, 0))[0] == INVALID
    # the wrapped cardinality of a full bitmap record and a bitmap record of few values are both legal
    full = struct.pack("<HBBHI", 0xF00D, 2, 1, 1, 65536) + b"\x01" + b"\x00" + struct.pack("<H", 0) + b"\xff" * 8192
    assert validate(full) == (OK, [1, 1, 65536, 1, 8192, len(full)])
    few = struct.pack("<HBBHI", 0xF00D, 2, 1, 1, 65536) + b"\x01" + b"\x00" + struct.pack("<H", 2) + b"\x03" + b"\x00" * 8191
    assert validate(few)[0] == OK


def test_every_truncation_of_a_small_stream():
    """a stream cut anywhere ends inside the header, the masks or a record: RBG_ERR_TRUNCATED at every length
    below the whole, whatever lies at the cut"""
    values = np.concatenate([np.arange(300) % 32, np.full(65536 - 300, 31), [0, 31, 7]])
    buf = RBO.build(values, 31)
    idx = RBO.Index(buf)
    assert len(buf) < 9000 and idx.max_key == 2 and len(idx.records) >= 6
    assert validate(buf)[0] == OK
    for n in range(len(buf)):
        assert validate(buf[:n])[0] == TRUNCATED, n
    with pytest.raises(rb.TruncatedInput):
        rb.RangeBitmap.map(buf[:-1])
    # the one-shot forms judge the stream before they look for a device
    cnt = ctypes.c_int64()
    assert L.lib().rbg_rangebitmap_count(buf[:40], 40, 0, 1, 0, None, 0, ctypes.byref(cnt)) == TRUNCATED
    bad = b"\x00" + buf[1:]
    assert L.lib().rbg_rangebitmap_count(bad, len(bad), 0, 1, 0, None, 0, ctypes.byref(cnt)) == INVALID
