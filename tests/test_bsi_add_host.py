"""The entry points of the fused BSI add (rbg_bsi_add, rbg_ctx_bsi_add; RoaringBitmapSliceIndex.add, BSI/:66-95)
without a device: the symbols with their argument types, the argument checks that come before any device
use, and the Python classes' early returns."""
import ctypes
import os
import re

import numpy as np

from roaringbitmap_amd import _lib as L

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x.h")
SYMBOLS = ["rbg_bsi_add", "rbg_ctx_bsi_add"]


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(L.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in L.EXPORTED
    i32, ci, vp, sz = ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    i32p = ctypes.POINTER(i32)
    assert L.lib().rbg_ctx_bsi_add.argtypes == [vp, i32, ci, i32, ci, i32, i32, i32p, i32p]
    side = [ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), ci]
    assert L.lib().rbg_bsi_add.argtypes == side + [i32, i32] + side + [vp, i32p]
    decl = re.search(r"int\s+rbg_ctx_bsi_add\s*\(([^)]*)\)", src).group(1)
    assert [w.split()[-1].lstrip("*") for w in decl.split(",")] == [
        "ctx", "batch_a", "nbits_a", "batch_b", "nbits_b", "min_a", "max_a", "out_batch", "out3"]


def test_argument_checks_come_before_any_device_use():
    """ILLEGAL_ARGUMENT (-3), not DEVICE (-4): without a GPU the first device call fails, so a status of -3
    shows the check came first; with one the same status is required"""
    lib = L.lib()
    bad = L.RBG_ERR_ILLEGAL_ARGUMENT
    ebm = O.from_values(np.arange(4, dtype=np.uint32))
    arr, lens = L.buf_array([ebm])
    outs = (L.rbg_buffer * 34)()
    out3 = (ctypes.c_int32 * 3)(-7, -7, -7)
    ok = (ebm, len(ebm), arr, lens, 1)
    assert lib.rbg_bsi_add(*ok, 0, 0, *ok, None, out3) == bad
    assert lib.rbg_bsi_add(*ok, 0, 0, *ok, outs, None) == bad
    assert lib.rbg_bsi_add(None, 0, arr, lens, 1, 0, 0, *ok, outs, out3) == bad  # null ebM
    assert lib.rbg_bsi_add(*ok, 0, 0, ebm, len(ebm), None, None, 1, outs, out3) == bad  # null slices, nb > 0
    assert lib.rbg_bsi_add(ebm, len(ebm), arr, lens, -1, 0, 0, *ok, outs, out3) == bad  # negative slice count
    assert lib.rbg_bsi_add(*ok, 0, 0, ebm, len(ebm), arr, lens, 33, outs, out3) == bad  # more slices than an int has bits
    batch = ctypes.c_int32(-7)
    assert lib.rbg_ctx_bsi_add(None, 0, 1, 0, 1, 0, 0, ctypes.byref(batch), out3) == bad
    assert batch.value == -7 and list(out3) == [-7, -7, -7] and not outs[0].data


def test_python_early_returns_reach_no_device():
    """None and an empty other index return at once (BSI/:67-69), for both classes"""
    import roaringbitmap_amd as rb
    for cls in (rb.RoaringBitmapSliceIndex, rb.MutableBitSliceIndex):
        x = cls.from_columns([1, 70000, 3], [5, 6, 7])
        before = (x.ebM.serialize(), [b.serialize() for b in x.bA], x.minValue, x.maxValue)
        x.add(None)
        x.add(cls())
        x.add(cls.from_columns([], []))
        assert (x.ebM.serialize(), [b.serialize() for b in x.bA], x.minValue, x.maxValue) == before
    assert callable(rb.Engine.bsi_add)
