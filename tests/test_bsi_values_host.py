"""The BSI values-in / values-out entry points (rbg_bsi_from_columns, rbg_bsi_get_values,
rbg_ctx_bsi_from_columns[_device], rbg_ctx_bsi_get_values[_device], rbg_ctx_bsi_to_pairs[_device]) without a
device: the symbols, the argument checks that come before any device use, and the host forms of getValues /
valueExist / toPairList (BBSI/:82, :534-549, the loop body of :551-639) against the oracle's getValue."""
import ctypes
import os
import re

import numpy as np
import pytest

from roaringbitmap_amd import _lib as L

import _oracle as O
from _bsi import BSI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x.h")
SYMBOLS = ["rbg_bsi_from_columns", "rbg_bsi_get_values", "rbg_ctx_bsi_from_columns", "rbg_ctx_bsi_from_columns_device",
           "rbg_ctx_bsi_get_values", "rbg_ctx_bsi_get_values_device", "rbg_ctx_bsi_to_pairs",
           "rbg_ctx_bsi_to_pairs_device"]


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(L.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in L.EXPORTED


def test_argument_checks_come_before_any_device_use():
    """ILLEGAL_ARGUMENT (-3), not DEVICE (-4): without a GPU the first device call fails, so a status of -3
    shows the check came first; with one the same status is required"""
    lib = L.lib()
    bad = L.RBG_ERR_ILLEGAL_ARGUMENT
    c = np.arange(4, dtype=np.uint32)
    v = np.arange(4, dtype=np.int32)
    cp, vp = c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    outs = (L.rbg_buffer * 33)()
    out3 = (ctypes.c_int32 * 3)(-7, -7, -7)
    assert lib.rbg_bsi_from_columns(None, vp, 4, 0, outs, out3) == bad  # null columns, n > 0
    assert lib.rbg_bsi_from_columns(cp, None, 4, 0, outs, out3) == bad  # null values, n > 0
    assert lib.rbg_bsi_from_columns(cp, vp, 4, 0, None, out3) == bad
    assert lib.rbg_bsi_from_columns(cp, vp, 4, 0, outs, None) == bad
    ebm = O.from_values(c)
    arr, lens = L.buf_array([ebm])
    res = np.full(4, -7, dtype=np.int64)
    rp = res.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert lib.rbg_bsi_get_values(ebm, len(ebm), arr, lens, -1, cp, 4, rp) == bad  # negative nbits
    assert lib.rbg_bsi_get_values(ebm, len(ebm), arr, lens, 33, cp, 4, rp) == bad  # more slices than an int has bits
    assert lib.rbg_bsi_get_values(ebm, len(ebm), arr, lens, 1, None, 4, rp) == bad  # null columns, n > 0
    assert lib.rbg_bsi_get_values(ebm, len(ebm), arr, lens, 1, cp, 4, None) == bad
    assert lib.rbg_bsi_get_values(None, 0, arr, lens, 1, cp, 4, rp) == bad
    assert lib.rbg_bsi_get_values(ebm, len(ebm), None, None, 1, cp, 4, rp) == bad
    batch = ctypes.c_int32(-7)
    assert lib.rbg_ctx_bsi_from_columns(None, cp, vp, 4, 0, ctypes.byref(batch), out3) == bad
    assert lib.rbg_ctx_bsi_from_columns_device(None, None, None, 4, 0, ctypes.byref(batch), out3) == bad
    assert lib.rbg_ctx_bsi_get_values(None, 0, -1, 0, cp, 4, rp) == bad
    assert lib.rbg_ctx_bsi_get_values_device(None, 0, -1, 0, None, 4, None) == bad
    assert lib.rbg_ctx_bsi_to_pairs(None, 0, -1, 0, 0, 0, None, None, None) == bad
    assert lib.rbg_ctx_bsi_to_pairs_device(None, 0, -1, 0, 0, 0, None, None, None) == bad
    assert batch.value == -7 and list(out3) == [-7, -7, -7] and (res == -7).all() and not outs[0].data


def test_length_mismatch_is_refused_at_the_python_layer():
    import roaringbitmap_amd as rb
    with pytest.raises(L.IllegalArgumentException):
        rb.RoaringBitmapSliceIndex.from_columns([1, 2, 3], [1, 2])
    with pytest.raises(L.IllegalArgumentException):
        rb.RoaringBitmapSliceIndex.from_columns([1, 2, 3], [1, 2], gpu=True)
    with pytest.raises(L.IllegalArgumentException):  # a negative value, likewise before any device use
        rb.RoaringBitmapSliceIndex.from_columns([1, 2], [1, -2], gpu=True)


def _three_keys():
    """keys 0, 5 and 65535; key 5 holds even values only (slice 0 has no container there)"""
    rng = np.random.default_rng(31)
    cols = np.concatenate([rng.choice(65536, 300, replace=False), (5 << 16) + rng.choice(65536, 5000, replace=False),
                           (65535 << 16) + np.array([0, 1, 65535])]).astype(np.int64)
    vals = rng.integers(0, 1 << 20, size=cols.size)
    vals[(cols >> 16) == 5] &= ~1
    vals[0] = 0
    return cols, vals


def test_host_read_outs_against_the_oracle():
    """getValues, valueExist and toPairList without gpu=True reach no device"""
    import roaringbitmap_amd as rb
    cols, vals = _three_keys()
    perm = np.random.default_rng(1).permutation(cols.size)
    x = rb.RoaringBitmapSliceIndex.from_columns(cols[perm], vals[perm])
    want = BSI.from_columns(cols[perm], vals[perm])
    assert x.ebM.serialize() == want.ebm and [b.serialize() for b in x.bA] == want.ba
    absent = np.array([70000, (5 << 16) + 1, 6 << 16, 0xFFFFFFFE, (65535 << 16) + 2])
    absent = absent[~np.isin(absent, cols)]
    q = np.concatenate([cols[:40], absent, cols[-3:], cols[:5], absent])
    exp = np.array([want.get_value(int(c))[0] if want.get_value(int(c))[1] else -1 for c in q])
    got = x.getValues(q)
    assert got.dtype == np.int64 and (got == exp).all()
    assert (exp[:40] == vals[:40]).all() and (exp[40:40 + absent.size] == -1).all()
    for c in list(cols[:5]) + list(absent):
        assert x.valueExist(int(c)) == want.get_value(int(c))[1] == x.getValue(int(c))[1]
    pc, pv = x.toPairList()
    order = np.argsort(cols)
    assert pc.dtype == np.uint32 and (pc == cols[order]).all() and (pv == vals[order]).all()
    found = rb.RoaringBitmap.from_values(np.concatenate([cols[::3], absent]))
    fc, fv = x.toPairList(found)
    keep = np.sort(cols[::3])
    assert (fc == keep).all() and (fv == vals[order][np.searchsorted(cols[order], keep)]).all()
    empty = rb.RoaringBitmapSliceIndex.from_columns([], [])
    assert empty.getValues([1, 2]).tolist() == [-1, -1] and empty.toPairList()[0].size == 0
    assert callable(rb.Engine.bsi_from_columns) and callable(rb.Engine.bsi_get_values) and callable(rb.Engine.bsi_to_pairs)
