"""The entry points of the BSI histogram (rbg_bsi_transpose, rbg_ctx_bsi_transpose;
BitSliceIndexBase.parallelTransposeWithCount, BBSI/:551-597) without a device: the symbols with their argument
types, the argument checks that come before any device use, and the Python side's own checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from roaringbitmap_amd import _lib as L

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x.h")
SYMBOLS = ["rbg_bsi_transpose", "rbg_ctx_bsi_transpose"]


def _names(src, name):
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src).group(1)
    return [w.split()[-1].lstrip("*") for w in decl.split(",")]


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(L.LIB_PATH)
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in L.EXPORTED
    assert text.count("BitSliceIndexBase.java:551-597") >= 2  # both comments cite the Java lines
    i32, ci, vp, sz = ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    i32p = ctypes.POINTER(i32)
    assert L.lib().rbg_ctx_bsi_transpose.argtypes == [vp, i32, ci, ci, ci, i32p, i32p]
    index = [ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), ci]
    assert L.lib().rbg_bsi_transpose.argtypes == index + [ctypes.c_char_p, sz, ci, vp, i32p]
    assert _names(src, "rbg_ctx_bsi_transpose") == ["ctx", "batch", "nbits", "has_found", "parallelism", "out_batch",
                                                    "out3"]
    assert _names(src, "rbg_bsi_transpose") == ["ebm", "ebm_len", "slices", "slice_lens", "nbits", "found", "found_len",
                                                "parallelism", "outs", "out3"]


def test_kernel_source_is_built():
    from roaringbitmap_amd import _build
    assert "bsitr.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "roaringbitmap_amd", "csrc", "bsitr.hip"))


def test_argument_checks_come_before_any_device_use():
    """ILLEGAL_ARGUMENT (-3), not DEVICE (-4): without a GPU the first device call fails, so a status of -3
    shows the check came first; with one the same status is required"""
    lib = L.lib()
    bad = L.RBG_ERR_ILLEGAL_ARGUMENT
    ebm = O.from_values(np.arange(4, dtype=np.uint32))
    arr, lens = L.buf_array([ebm])
    outs = (L.rbg_buffer * 33)()
    out3 = (ctypes.c_int32 * 3)(-7, -7, -7)
    index = (ebm, len(ebm), arr, lens, 1)
    assert lib.rbg_bsi_transpose(*index, None, 0, 1, None, out3) == bad  # no outputs
    assert lib.rbg_bsi_transpose(*index, None, 0, 1, outs, None) == bad
    assert lib.rbg_bsi_transpose(*index, None, 0, 0, outs, out3) == bad  # the reference divides by it
    assert lib.rbg_bsi_transpose(*index, None, 0, -4, outs, out3) == bad
    assert lib.rbg_bsi_transpose(ebm, len(ebm), arr, lens, 33, None, 0, 1, outs, out3) == bad
    assert lib.rbg_bsi_transpose(ebm, len(ebm), arr, lens, -1, None, 0, 1, outs, out3) == bad
    assert lib.rbg_bsi_transpose(None, 0, arr, lens, 1, None, 0, 1, outs, out3) == bad  # null ebM
    assert lib.rbg_bsi_transpose(ebm, len(ebm), None, None, 1, None, 0, 1, outs, out3) == bad  # null slices
    batch = ctypes.c_int32(-7)
    assert lib.rbg_ctx_bsi_transpose(None, 0, 1, 0, 1, ctypes.byref(batch), out3) == bad
    assert batch.value == -7 and list(out3) == [-7, -7, -7] and not outs[0].data


def test_python_side_checks_reach_no_device():
    import roaringbitmap_amd as rb
    x = rb.MutableBitSliceIndex.from_columns([1, 70000, 3], [5, 6, 7])
    for p in (0, -1):
        with pytest.raises(rb.IllegalArgumentException, match="parallelism"):
            x.parallelTransposeWithCount(None, p)
    wide = rb.MutableBitSliceIndex(x.ebM, [x.ebM] * 33)
    with pytest.raises(rb.IllegalArgumentException, match="32 slices"):
        wide.parallelTransposeWithCount(None, 1, pool=object())
    assert callable(rb.Engine.bsi_transpose)
    assert not hasattr(rb.RoaringBitmapSliceIndex, "parallelTransposeWithCount")  # as in the reference
    assert rb.ImmutableBitSliceIndex.parallelTransposeWithCount is rb.MutableBitSliceIndex.parallelTransposeWithCount
