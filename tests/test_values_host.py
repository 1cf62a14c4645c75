"""The values-in / values-out entry points (rbg_build_values, rbg_expand_values, rbg_ctx_from_values[_device],
rbg_ctx_to_values[_device]) without a device: the symbols, the argument checks that come before any device
use, and the host paths that stay the default."""
import ctypes
import os
import re

import numpy as np

from roaringbitmap_amd import _lib as L

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x.h")
SYMBOLS = ["rbg_build_values", "rbg_expand_values", "rbg_ctx_from_values", "rbg_ctx_from_values_device",
           "rbg_ctx_to_values", "rbg_ctx_to_values_device"]


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
    b = L.rbg_buffer()
    v = np.arange(4, dtype=np.uint32)
    vp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert lib.rbg_build_values(None, 4, 0, ctypes.byref(b)) == L.RBG_ERR_ILLEGAL_ARGUMENT  # null values, n > 0
    assert lib.rbg_build_values(vp, 4, 0, None) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert lib.rbg_expand_values(None, 8, ctypes.byref(b)) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert lib.rbg_expand_values(O.from_values(v), 24, None) == L.RBG_ERR_ILLEGAL_ARGUMENT
    out = ctypes.c_int32(-7)
    assert lib.rbg_ctx_from_values(None, vp, 4, 0, ctypes.byref(out)) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert lib.rbg_ctx_from_values_device(None, None, 4, 0, ctypes.byref(out)) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert lib.rbg_ctx_to_values(None, 0, 0, 0, 4, vp, None) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert lib.rbg_ctx_to_values_device(None, 0, 0, 0, 4, 0, None, None) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert out.value == -7 and not b.data


def test_host_paths_stay_the_default():
    """from_values() / toArray() without gpu=True reach no device"""
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(5)
    v = rng.integers(0, 1 << 32, size=20000)
    for ro in (False, True):
        x = rb.RoaringBitmap.from_values(v, ro)
        assert x.serialize() == O.from_values(v.astype(np.uint32), ro)
        assert (x.toArray() == np.unique(v).astype(np.uint32)).all() and x.toArray().dtype == np.uint32
    assert callable(rb.Engine.from_values) and callable(rb.Engine.to_values)
