"""Batches of values added to or removed from a bitmap, without a device: the symbols of
include/roaring_mi355x_mutate.h, the refusals decided from the arguments alone, and the host form
(rbg_mutate_values_host, the default of RoaringBitmap.add_many / remove_many / addN / checkedAdd /
checkedRemove) against the model of tests/_mutate.py on the device tests' case list, byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L

import _mutate as M
from _fmt import A, R, decode, encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x_mutate.h")
SYMBOLS = ["rbg_ctx_mutate_values", "rbg_ctx_mutate_values_device", "rbg_mutate_values", "rbg_mutate_values_host"]
OK, ILLEGAL = L.RBG_OK, L.RBG_ERR_ILLEGAL_ARGUMENT
U32P = ctypes.POINTER(ctypes.c_uint32)


def test_symbols_exported_declared_and_typed():
    lib = ctypes.CDLL(L.LIB_PATH)
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    main = open(os.path.join(ROOT, "include", "roaring_mi355x.h")).read()
    assert '#include "roaring_mi355x_mutate.h"' in main
    assert sorted(set(re.findall(r"\b(rbg_\w+)\s*\(", src))) == sorted(SYMBOLS)
    assert list(L.MUTATE_SIGNATURES) == SYMBOLS  # the header's order
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        before = text[:text.index(f"int {name}(")]
        assert re.search(r":\d+-\d+", before[before.rindex("/*"):]), name  # every entry cites its Java lines
    ci, vp, u64, i32, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_size_t
    P, buf, u8p = ctypes.POINTER, ctypes.POINTER(L.rbg_buffer), ctypes.c_char_p
    want = {"rbg_ctx_mutate_values": [vp, i32, ci, U32P, sz, P(i32), P(u64)],
            "rbg_ctx_mutate_values_device": [vp, i32, ci, vp, sz, P(i32), P(u64)],
            "rbg_mutate_values": [u8p, sz, ci, U32P, sz, buf, P(u64)],
            "rbg_mutate_values_host": [u8p, sz, ci, U32P, sz, buf, P(u64)]}
    for name, args in want.items():
        f = getattr(L.lib(), name)
        assert f.restype is ci and list(f.argtypes) == args, name
    flat = re.sub(r"\s+", " ", src)
    for decl in ("rbg_ctx* ctx, int32_t batch, int op, const uint32_t* values, size_t n, int32_t* out_batch, "
                 "uint64_t* changed",
                 "rbg_ctx* ctx, int32_t batch, int op, const void* values_dev, size_t n, int32_t* out_batch, "
                 "uint64_t* changed",
                 "const uint8_t* buf, size_t len, int op, const uint32_t* values, size_t n, rbg_buffer* out, "
                 "uint64_t* changed"):
        assert decl in flat, decl
    m = re.search(r"RBG_MUT_ADD\s*=\s*(\d+),\s*RBG_MUT_REMOVE\s*=\s*(\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (L.RBG_MUT_ADD, L.RBG_MUT_REMOVE) == (0, 1)
    from roaringbitmap_amd import _build
    assert {"mutate.hip", "engine_mutate.cpp", "mutate_host.cpp"} <= set(_build.SOURCES)
    for f in ("mutate_values", "add_values", "remove_values"):
        assert callable(getattr(rb.Engine, f))
    for f in ("add_many", "remove_many", "addN", "checkedAdd", "checkedRemove"):
        assert callable(getattr(rb.RoaringBitmap, f))


def test_refusals_need_no_device():
    """op outside {0, 1}, a null output, null values with n > 0 and a null handle are RBG_ERR_ILLEGAL_ARGUMENT
    from the arguments alone, in all four entry points, and leave no buffer"""
    lib = L.lib()
    x = M.mixed_operand()
    v = np.arange(4, dtype=np.uint32)
    p = v.ctypes.data_as(U32P)
    out, ch, b = ctypes.c_int32(-7), ctypes.c_uint64(99), L.rbg_buffer()
    for f in (lib.rbg_mutate_values, lib.rbg_mutate_values_host):
        for op in (2, -1, 7):
            assert f(x, len(x), op, p, 4, ctypes.byref(b), ctypes.byref(ch)) == ILLEGAL
        assert f(x, len(x), 0, p, 4, None, ctypes.byref(ch)) == ILLEGAL
        assert f(x, len(x), 0, p, 4, ctypes.byref(b), None) == ILLEGAL
        assert f(x, len(x), 1, None, 4, ctypes.byref(b), ctypes.byref(ch)) == ILLEGAL
        assert f(None, 8, 1, p, 4, ctypes.byref(b), ctypes.byref(ch)) == ILLEGAL
        assert not b.data and b.len == 0 and ch.value == 99
    for f, vals in ((lib.rbg_ctx_mutate_values, p), (lib.rbg_ctx_mutate_values_device, ctypes.c_void_p(v.ctypes.data))):
        assert f(None, 0, 0, vals, 4, ctypes.byref(out), ctypes.byref(ch)) == ILLEGAL  # a null handle
        assert out.value == -7 and ch.value == 99


def test_malformed_bitmaps_give_the_parsers_status():
    lib = L.lib()
    x = M.mixed_operand()
    v = np.arange(4, dtype=np.uint32)
    b, ch = L.rbg_buffer(), ctypes.c_uint64()
    f = lib.rbg_mutate_values_host
    assert f(x[:-1], len(x) - 1, 0, v.ctypes.data_as(U32P), 4, ctypes.byref(b), ctypes.byref(ch)) == L.RBG_ERR_TRUNCATED
    assert f(b"\x01\x02\x03\x04" + x[4:], len(x), 0, v.ctypes.data_as(U32P), 4, ctypes.byref(b),
             ctypes.byref(ch)) == L.RBG_ERR_INVALID_FORMAT
    assert not b.data


def _host(x, v, remove):
    v = L.as_u32(v)
    ch = ctypes.c_uint64()
    got = L.call_bytes(lambda *a: L.lib().rbg_mutate_values_host(*a, ctypes.byref(ch)), x, len(x), int(remove),
                       v.ctypes.data_as(U32P), v.size)
    return got, ch.value


@pytest.mark.parametrize("name", M.case_names())
def test_host_form_and_python_methods_match_the_model(name):
    x, v, remove = M.cases()[name]
    want = M.expected(name)
    assert _host(x, v, remove) == want
    y = rb.RoaringBitmap(x)
    assert (y.remove_many if remove else y.add_many)(v) == want[1]
    assert y.serialize() == want[0] and y.getLongCardinality() == sum(len(c[3]) for c in decode(want[0]))


def test_nine_keys_in_five_orders():
    rng = np.random.default_rng(4)
    x, v = M.nine_keys_batch()
    for remove in (False, True):
        want = M.mutate_reference(x, v, remove)
        for order in (v, np.sort(v), np.sort(v)[::-1], rng.permutation(v), rng.permutation(np.concatenate([v, v[:999]]))):
            assert _host(x, order, remove) == want


def test_single_value_and_vararg_methods():
    x = rb.RoaringBitmap(encode([(0, R, np.arange(5, 9))]))
    assert x.checkedAdd(9) is True and x.checkedAdd(9) is False and x.checkedAdd(-1) is True
    assert x.checkedRemove(6) is True and x.checkedRemove(6) is False and x.checkedRemove(1 << 20) is False
    want = M.mutate_reference(encode([(0, R, np.arange(5, 9))]), [9, 0xFFFFFFFF], False)[0]
    assert x.serialize() == M.mutate_reference(want, [6], True)[0]
    assert [c[1] for c in decode(x.serialize())] == [R, A]
    y = rb.RoaringBitmap()
    assert y.add(3, 1, 70000, 3) is None  # add(int... dat); two ints stay the range form add(rangeStart, rangeEnd)
    assert y.toArray().tolist() == [1, 3, 70000]
    assert y.remove(3) is None and y.remove(3) is None and y.remove(12345) is None  # remove(int), :2637-2648
    assert y.toArray().tolist() == [1, 70000]
    assert y.remove(np.int64(70000)) is None and y.toArray().tolist() == [1]
    z = rb.RoaringBitmap(encode([(0, R, np.arange(5, 9))]))
    z.remove(6)  # a run container stays one: [5, 5], [7, 8]
    assert z.serialize() == M.mutate_reference(encode([(0, R, np.arange(5, 9))]), [6], True)[0]
    assert [c[1] for c in decode(z.serialize())] == [R]
    z.remove(5), z.remove(7), z.remove(8)
    assert z.serialize() == encode([])  # the emptied container is dropped
    with pytest.raises(NotImplementedError):
        y.add(9)  # pinned by tests/test_host.py: the single-value add stays refused (checkedAdd / add_many take it)
    with pytest.raises(NotImplementedError):
        rb.MutableRoaringBitmap(y.serialize()).remove(5)  # the plain RoaringBitmap's alone
    for cls in (rb.ImmutableRoaringBitmap, rb.MutableRoaringBitmap):  # the plain RoaringBitmap's alone
        assert cls.add_many is None and cls.checkedAdd is None


def test_addn_argument_checks():
    """addN's three argument errors (RB/RoaringBitmap.java:498-508) and its n == 0 return"""
    x = rb.RoaringBitmap.bitmapOf(1, 2)
    before = x.serialize()
    dat = [10, 11, 12, 13]
    with pytest.raises(L.IllegalArgumentException, match="Negative values do not make sense."):
        x.addN(dat, 0, -1)
    with pytest.raises(L.IllegalArgumentException, match="Negative values do not make sense."):
        x.addN(dat, -1, 2)
    with pytest.raises(L.IllegalArgumentException, match="Data source is too small."):
        x.addN(dat, 2, 3)
    x.addN(dat, 99, 0)  # n == 0 returns before the bounds are looked at
    assert x.serialize() == before
    x.addN(dat, 1, 2)
    assert x.toArray().tolist() == [1, 2, 11, 12]
