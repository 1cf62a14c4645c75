"""Building a range-encoded index from values and writing a resident one back out (RB/RangeBitmap.java:
Appender, :1378-1631), without a device: the symbols of include/roaring_mi355x_rangebitmap_build.h, the
refusals decided from the arguments alone, and the host format layer's rb_emit held to its parser through
rbg_rangebitmap_reserialize (parse, re-lay, emit), which must return exactly the bytes the parser consumed."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x_rangebitmap_build.h")
SYMBOLS = ["rbg_ctx_rangebitmap_build", "rbg_ctx_rangebitmap_build_device", "rbg_ctx_rangebitmap_serialize",
           "rbg_rangebitmap_build", "rbg_rangebitmap_reserialize"]
OK, INVALID, TRUNCATED, ILLEGAL = L.RBG_OK, L.RBG_ERR_INVALID_FORMAT, L.RBG_ERR_TRUNCATED, L.RBG_ERR_ILLEGAL_ARGUMENT
M64 = (1 << 64) - 1


def test_symbols_exported_declared_and_typed():
    lib = ctypes.CDLL(L.LIB_PATH)
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    main = open(os.path.join(ROOT, "include", "roaring_mi355x.h")).read()
    assert '#include "roaring_mi355x_rangebitmap_build.h"' in main
    assert sorted(set(re.findall(r"\b(rbg_\w+)\s*\(", src))) == sorted(SYMBOLS)
    assert list(L.RANGEBITMAP_BUILD_SIGNATURES) == SYMBOLS  # the header's order
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(L.lib(), name).argtypes is not None, name
        before = text[:text.index(f"int {name}(")]
        assert re.search(r":\d+-\d+", before[before.rindex("/*"):]), name  # every entry cites its Java lines
    ci, vp, u64, i32, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_size_t
    P, buf = ctypes.POINTER, ctypes.POINTER(L.rbg_buffer)
    want = {"rbg_ctx_rangebitmap_build": [vp, vp, u64, u64, ci, P(i32)],
            "rbg_ctx_rangebitmap_build_device": [vp, vp, u64, u64, ci, P(i32)],
            "rbg_ctx_rangebitmap_serialize": [vp, i32, buf],
            "rbg_rangebitmap_build": [vp, u64, u64, ci, buf],
            "rbg_rangebitmap_reserialize": [ctypes.c_char_p, sz, buf]}
    for name, args in want.items():
        f = getattr(L.lib(), name)
        assert f.restype is ci and list(f.argtypes) == args, name
    for decl in ("const uint64_t* values, uint64_t n, uint64_t max_value, int max_from_data, int32_t* index",
                 "const uint64_t* values_dev, uint64_t n, uint64_t max_value,", "int32_t index, rbg_buffer* out",
                 "const uint64_t* values, uint64_t n, uint64_t max_value, int max_from_data, rbg_buffer* out",
                 "const uint8_t* buf, size_t len, rbg_buffer* out"):
        assert decl in re.sub(r"\s+", " ", src), decl
    from roaringbitmap_amd import _build
    assert {"rangebitmap_build.hip", "rangebitmap_format.cpp", "engine_rangebitmap.cpp"} <= set(_build.SOURCES)
    for f in ("rangebitmap_build", "rangebitmap_serialize"):
        assert callable(getattr(rb.Engine, f))
    assert callable(rb.RangeBitmap.from_values)


def _err():
    return L.lib().rbg_last_error().decode()


def test_refusals_come_before_any_device_use():
    """a null output, a null pointer with rows and more rows than 65,535 blocks hold are
    RBG_ERR_ILLEGAL_ARGUMENT with their own text before the handle is looked at"""
    lib = L.lib()
    v = np.arange(4, dtype=np.uint64)
    p = ctypes.c_void_p(v.ctypes.data)
    out = ctypes.c_int32(-7)
    b = L.rbg_buffer()
    too_many = 65535 * 65536 + 1
    for f in (lib.rbg_ctx_rangebitmap_build, lib.rbg_ctx_rangebitmap_build_device):
        assert f(None, p, 4, 3, 0, None) == ILLEGAL and "no output" in _err()
        assert f(None, None, 4, 3, 0, ctypes.byref(out)) == ILLEGAL and "no input" in _err()
        assert f(None, p, too_many, 3, 0, ctypes.byref(out)) == ILLEGAL and "65,535 blocks" in _err()
        assert f(None, p, 4, 3, 0, ctypes.byref(out)) == ILLEGAL  # the null handle
        assert f(None, None, 0, 3, 1, ctypes.byref(out)) == ILLEGAL  # no rows are fine; the null handle is not
    odd = ctypes.c_void_p(v.ctypes.data + 4)
    assert lib.rbg_ctx_rangebitmap_build_device(None, odd, 2, 3, 0, ctypes.byref(out)) == ILLEGAL
    assert "8-byte aligned" in _err()
    assert lib.rbg_rangebitmap_build(p, 4, 3, 0, None) == ILLEGAL and "no output" in _err()
    assert lib.rbg_rangebitmap_build(None, 4, 3, 0, ctypes.byref(b)) == ILLEGAL and "no input" in _err()
    assert lib.rbg_rangebitmap_build(p, too_many, 3, 0, ctypes.byref(b)) == ILLEGAL and "65,535 blocks" in _err()
    assert lib.rbg_ctx_rangebitmap_serialize(None, 0, None) == ILLEGAL
    assert lib.rbg_ctx_rangebitmap_serialize(None, 0, ctypes.byref(b)) == ILLEGAL  # the null handle
    assert lib.rbg_rangebitmap_reserialize(None, 8, ctypes.byref(b)) == ILLEGAL
    assert lib.rbg_rangebitmap_reserialize(b"\x0d\xf0", 2, None) == ILLEGAL
    assert out.value == -7 and not b.data


def _stream(values, max_value):
    app = rb.RangeBitmap.appender(max_value)  # byte-equal to the oracle's (test_rangebitmap_oracle.py)
    app.add_many(np.asarray(values, dtype=np.uint64))
    return app.serialize()


def _hand_written():
    """records the Appender cannot write but the format allows: a bitmap record of a full block (size field
    0), a bitmap of 5 values, an array in slice 0, an empty array and an empty run record"""
    full = b"\x00" + struct.pack("<H", 0) + b"\xff" * 8192
    few_rows = np.array([1, 64, 4097, 40000, 65535])
    few = b"\x00" + struct.pack("<H", 5) + np.packbits(np.isin(np.arange(65536), few_rows), bitorder="little").tobytes()
    arr_rows = np.arange(7, 30000, 11)
    arr = b"\x02" + struct.pack("<H", arr_rows.size) + arr_rows.astype("<u2").tobytes()
    n = 2 * 65536 + 40
    head = struct.pack("<HBBHI", 0xF00D, 2, 3, 3, n)
    # block 0: an array in slice 0, the full bitmap, the few; block 1: an empty array, full; block 2: an empty run
    return (head + bytes([0b111, 0b011, 0b100]) + arr + full + few + b"\x02\x00\x00" + full + b"\x01\x00\x00")


def _streams():
    rng = np.random.default_rng(11)
    n3 = 2 * 65536 + 70
    mixed = np.where(rng.random(n3) < 0.03, rng.integers(0, 1 << 9, n3), 511)
    mixed[10000:20000:2] &= 0x1FE  # array, bitmap and run records, three blocks
    return {"empty": rb.RangeBitmap.appender(1000).serialize(),
            "one_row": _stream([5], 7),
            "wide": _stream([0, M64, 1 << 63, 12345], M64),
            "five_byte_mask": _stream(rng.integers(0, 1 << 33, 200), (1 << 33) - 1),
            "mixed": _stream(mixed, 511),
            "hand_written": _hand_written(),
            "trailing_bytes": _stream([3, 1, 2, 0], 3) + b"\x01\x02\x03 anything"}


STREAMS = _streams()


def _reserialize(buf):
    return L.call_bytes(L.lib().rbg_rangebitmap_reserialize, buf, len(buf))


@pytest.mark.parametrize("name", list(STREAMS))
def test_reserialize_returns_what_the_parser_consumed(name):
    buf = STREAMS[name]
    info = (ctypes.c_uint64 * 6)()
    assert L.lib().rbg_rangebitmap_validate(buf, len(buf), info) == OK
    consumed = int(info[5])
    assert consumed == len(buf) or name == "trailing_bytes"
    assert _reserialize(buf) == buf[:consumed]


def test_the_streams_cover_what_they_claim():
    import _rangebitmap as RBO
    kinds = {t for t, _, _ in RBO.Index(STREAMS["mixed"]).records}
    assert kinds == {RBO.BITMAP, RBO.RUN, RBO.ARRAY} and RBO.Index(STREAMS["mixed"]).max_key == 3
    assert RBO.Index(STREAMS["wide"]).slice_count == 64 and RBO.Index(STREAMS["five_byte_mask"]).bytes_per_mask == 5
    assert RBO.Index(STREAMS["empty"]).max_key == 0 and RBO.Index(STREAMS["one_row"]).max == 1
    hw = RBO.Index(STREAMS["hand_written"])
    assert [(t, s) for t, s, _ in hw.records][:2] == [(RBO.ARRAY, 2727), (RBO.BITMAP, 0)] and hw.consumed == len(
        STREAMS["hand_written"])


def test_reserialize_reports_the_parsers_errors():
    lib = L.lib()
    b = L.rbg_buffer()
    good = STREAMS["mixed"]
    bad_cookie = b"\x0e\xf0" + good[2:]
    assert lib.rbg_rangebitmap_reserialize(bad_cookie, len(bad_cookie), ctypes.byref(b)) == INVALID
    assert "invalid cookie" in _err()
    for cut in (0, 1, 5, 9, 11, 20, len(good) // 2, len(good) - 1):
        assert lib.rbg_rangebitmap_reserialize(good, cut, ctypes.byref(b)) == TRUNCATED, cut
    bad_type = bytearray(STREAMS["one_row"])
    bad_type[11] = 3
    assert lib.rbg_rangebitmap_reserialize(bytes(bad_type), len(bad_type), ctypes.byref(b)) == INVALID
    assert not b.data


def test_from_values_on_the_host_is_the_appender():
    rng = np.random.default_rng(3)
    v = rng.integers(0, 1 << 20, 70000, dtype=np.uint64)
    assert rb.RangeBitmap.from_values(v).serialize() == _stream(v, int(v.max()))
    assert rb.RangeBitmap.from_values(v, (1 << 30) - 1).serialize() == _stream(v, (1 << 30) - 1)
    neg = np.array([-1, -2, 5], dtype=np.int64)
    assert rb.RangeBitmap.from_values(neg).serialize() == _stream(neg.view(np.uint64), M64)
    assert rb.RangeBitmap.from_values(np.zeros(0, dtype=np.uint64)).serialize() == rb.RangeBitmap.appender(0).serialize()
    with pytest.raises(rb.IllegalArgumentException, match="too large"):
        rb.RangeBitmap.from_values([1, 2, 9], 7)
