"""The entry points of the fused BSI IN query (rbg_bsi_in, rbg_ctx_bsi_in; BitSliceIndexBase.parallelIn,
BBSI/:611-639) without a device: the symbols with their argument types, the argument checks that come before
any device use, and the Python side's own checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from roaringbitmap_amd import _lib as L

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x.h")
SYMBOLS = ["rbg_bsi_in", "rbg_ctx_bsi_in"]


def _names(src, name):
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src).group(1)
    return [w.split()[-1].lstrip("*") for w in decl.split(",")]


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(L.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in L.EXPORTED
    i32, ci, vp, sz = ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    i32p = ctypes.POINTER(i32)
    assert L.lib().rbg_ctx_bsi_in.argtypes == [vp, i32, ci, ci, i32p, sz, ci, i32p]
    index = [ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), ci]
    assert L.lib().rbg_bsi_in.argtypes == index + [ctypes.c_char_p, sz, i32p, sz, ci, ctypes.POINTER(L.rbg_buffer)]
    assert _names(src, "rbg_ctx_bsi_in") == ["ctx", "batch", "nbits", "has_found", "values", "n_values", "parallelism",
                                             "out_batch"]
    assert _names(src, "rbg_bsi_in") == ["ebm", "ebm_len", "slices", "slice_lens", "nbits", "found", "found_len",
                                         "values", "n_values", "parallelism", "out"]


def test_argument_checks_come_before_any_device_use():
    """ILLEGAL_ARGUMENT (-3), not DEVICE (-4): without a GPU the first device call fails, so a status of -3
    shows the check came first; with one the same status is required"""
    lib = L.lib()
    bad = L.RBG_ERR_ILLEGAL_ARGUMENT
    ebm = O.from_values(np.arange(4, dtype=np.uint32))
    arr, lens = L.buf_array([ebm])
    vals = (ctypes.c_int32 * 2)(1, 2)
    out = L.rbg_buffer()
    index = (ebm, len(ebm), arr, lens, 1)
    assert lib.rbg_bsi_in(*index, None, 0, vals, 2, 1, None) == bad  # no output
    assert lib.rbg_bsi_in(*index, None, 0, vals, 2, 0, ctypes.byref(out)) == bad  # the reference divides by it
    assert lib.rbg_bsi_in(*index, None, 0, vals, 2, -4, ctypes.byref(out)) == bad
    assert lib.rbg_bsi_in(*index, None, 0, None, 2, 1, ctypes.byref(out)) == bad  # a null list of two values
    assert lib.rbg_bsi_in(ebm, len(ebm), arr, lens, 33, None, 0, vals, 2, 1, ctypes.byref(out)) == bad
    assert lib.rbg_bsi_in(ebm, len(ebm), arr, lens, -1, None, 0, vals, 2, 1, ctypes.byref(out)) == bad
    assert lib.rbg_bsi_in(None, 0, arr, lens, 1, None, 0, vals, 2, 1, ctypes.byref(out)) == bad  # null ebM
    assert lib.rbg_bsi_in(ebm, len(ebm), None, None, 1, None, 0, vals, 2, 1, ctypes.byref(out)) == bad  # null slices
    batch = ctypes.c_int32(-7)
    assert lib.rbg_ctx_bsi_in(None, 0, 1, 0, vals, 2, 1, ctypes.byref(batch)) == bad
    assert batch.value == -7 and not out.data


def test_python_side_checks_reach_no_device():
    import roaringbitmap_amd as rb
    x = rb.MutableBitSliceIndex.from_columns([1, 70000, 3], [5, 6, 7])
    for p in (0, -1):
        with pytest.raises(rb.IllegalArgumentException, match="parallelism"):
            x.parallelIn(p, None, [5])
    for values in ([1 << 32], [-(1 << 31) - 1], np.array([0, 1 << 40])):
        with pytest.raises(rb.IllegalArgumentException, match="32 bits"):
            x.parallelIn(1, None, values)
    wide = rb.MutableBitSliceIndex(x.ebM, [x.ebM] * 33)
    with pytest.raises(rb.IllegalArgumentException, match="32 slices"):
        wide.parallelIn(1, None, [5])
    assert callable(rb.Engine.bsi_in)
    assert not hasattr(rb.RoaringBitmapSliceIndex, "parallelIn")  # the heap index has no such method
    assert rb.ImmutableBitSliceIndex.parallelIn is rb.MutableBitSliceIndex.parallelIn
