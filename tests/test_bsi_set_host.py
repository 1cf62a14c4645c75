"""The entry points of setValues on a bit-sliced index (rbg_bsi_set_values, rbg_ctx_bsi_set_values[_device];
RoaringBitmapSliceIndex.setValues, BSI/:349-357) without a device: the symbols with their argument types, the
refusals that come before any device use, and the Python classes' host setValue / setValues against the
oracle's replay (tests/_bsi_set.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from roaringbitmap_amd import _lib as L

import _oracle as O
from _bsi import BSI
from _bsi_set import set_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x.h")
SYMBOLS = ["rbg_bsi_set_values", "rbg_ctx_bsi_set_values", "rbg_ctx_bsi_set_values_device"]


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(L.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in L.EXPORTED
    i32, ci, vp, sz = ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    i32p, u32p = ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint32)
    assert L.lib().rbg_ctx_bsi_set_values.argtypes == [vp, i32, ci, i32, i32, u32p, i32p, sz, i32p, i32p]
    assert L.lib().rbg_ctx_bsi_set_values_device.argtypes == [vp, i32, ci, i32, i32, vp, vp, sz, i32p, i32p]
    index = [ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz), ci]
    assert L.lib().rbg_bsi_set_values.argtypes == index + [i32, i32, u32p, i32p, sz, vp, i32p]
    for name, tail in (("rbg_ctx_bsi_set_values", ["columns", "values"]),
                       ("rbg_ctx_bsi_set_values_device", ["columns_dev", "values_dev"])):
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert [w.split()[-1].lstrip("*") for w in decl.split(",")] == [
            "ctx", "batch", "nbits", "min_value", "max_value"] + tail + ["n", "out_batch", "out3"]


def test_argument_checks_come_before_any_device_use():
    """ILLEGAL_ARGUMENT (-3), not DEVICE (-4): without a GPU the first device call fails, so a status of -3
    shows the check came first; with one the same status is required"""
    lib = L.lib()
    bad = L.RBG_ERR_ILLEGAL_ARGUMENT
    ebm = O.from_values(np.arange(4, dtype=np.uint32))
    arr, lens = L.buf_array([ebm])
    outs = (L.rbg_buffer * 33)()
    out3 = (ctypes.c_int32 * 3)(-7, -7, -7)
    c = (ctypes.c_uint32 * 2)(1, 2)
    v = (ctypes.c_int32 * 2)(3, 4)
    ok = (ebm, len(ebm), arr, lens, 1, 0, 1)
    assert lib.rbg_bsi_set_values(*ok, c, v, 2, None, out3) == bad
    assert lib.rbg_bsi_set_values(*ok, c, v, 2, outs, None) == bad
    assert lib.rbg_bsi_set_values(*ok, None, v, 2, outs, out3) == bad  # null columns, n > 0
    assert lib.rbg_bsi_set_values(*ok, c, None, 2, outs, out3) == bad
    assert lib.rbg_bsi_set_values(None, 0, arr, lens, 1, 0, 1, c, v, 2, outs, out3) == bad  # null ebM
    assert lib.rbg_bsi_set_values(ebm, len(ebm), None, None, 1, 0, 1, c, v, 2, outs, out3) == bad  # null slices
    assert lib.rbg_bsi_set_values(ebm, len(ebm), arr, lens, -1, 0, 1, c, v, 2, outs, out3) == bad
    assert lib.rbg_bsi_set_values(ebm, len(ebm), arr, lens, 33, 0, 1, c, v, 2, outs, out3) == bad  # nbits > 32
    batch = ctypes.c_int32(-7)
    assert lib.rbg_ctx_bsi_set_values(None, 0, 1, 0, 1, c, v, 2, ctypes.byref(batch), out3) == bad
    assert lib.rbg_ctx_bsi_set_values_device(None, 0, 1, 0, 1, None, None, 2, ctypes.byref(batch), out3) == bad
    assert batch.value == -7 and list(out3) == [-7, -7, -7] and not outs[0].data


def _rb_index(cls, o):
    import roaringbitmap_amd as rb
    x = cls(rb.RoaringBitmap(o.ebm), [rb.RoaringBitmap(s) for s in o.ba], o.min, o.max)
    x.runOptimized = o.run_optimized
    return x


def _rb_bytes(x):
    return [x.ebM.serialize()] + [s.serialize() for s in x.bA], x.bitCount(), x.minValue, x.maxValue


def _want(o):
    return [o.ebm] + o.ba, o.bit_count(), o.min, o.max


def _index(cols, vals):
    return BSI.from_columns(np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.int64))


@pytest.mark.parametrize("gpu_flag", [False, True])
def test_python_refusals_reach_no_device(gpu_flag):
    import roaringbitmap_amd as rb
    for cls in (rb.RoaringBitmapSliceIndex, rb.MutableBitSliceIndex):
        x = cls.from_columns([1, 70000, 3], [5, 6, 7])
        before = _rb_bytes(x)
        with pytest.raises(rb.IllegalArgumentException, match="non-negative"):
            x.setValues([1, 2], [3, -1], gpu=gpu_flag)
        with pytest.raises(rb.IllegalArgumentException, match="no pair"):
            x.setValues([], [], gpu=gpu_flag)
        with pytest.raises(rb.IllegalArgumentException, match="differ in length"):
            x.setValues([1, 2], [3], gpu=gpu_flag)
        assert _rb_bytes(x) == before
    assert callable(rb.Engine.bsi_set_values)


def test_host_set_values_against_the_replay():
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(31)
    cols = np.concatenate([(k << 16) + rng.choice(65536, s, replace=False)
                           for k, s in ((0, 4096), (2, 4097), (9, 30000), (65535, 40))])
    a = _index(cols, rng.integers(1, 1 << 10, cols.size))
    upd = rng.choice(cols, 2000, replace=False)
    bc = np.concatenate([upd, (1 << 16) + np.arange(70), [5 << 16, 0xFFFFFFFF], upd[:200], [int(cols[0])] * 3])
    for cls in (rb.RoaringBitmapSliceIndex, rb.MutableBitSliceIndex):
        for hi in (1 << 10, 1 << 13):  # neither / min, then growth
            bv = rng.integers(0, hi, bc.size)
            x = _rb_index(cls, a)
            x.setValues(bc, bv)
            assert _rb_bytes(x) == _want(set_reference(a, bc, bv)), (cls.__name__, hi)
            assert x.runOptimized is False
    e = rb.RoaringBitmapSliceIndex()
    e.setValue(7, 300)  # into the empty index: min = max = 300, nine slices
    assert _rb_bytes(e) == _want(set_reference(_index([], []), [7], [300])) and e.getValue(7) == (300, True)
    e.setValues([7, 0xFFFFFFFF], [0, 513])  # both exceeded: min alone, the high bits dropped
    want = set_reference(set_reference(_index([], []), [7], [300]), [7, 0xFFFFFFFF], [0, 513])
    assert _rb_bytes(e) == _want(want) and (e.bitCount(), e.minValue, e.maxValue) == (9, 0, 300)
    assert e.getValue(7) == (0, True) and e.getValue(0xFFFFFFFF) == (513 & 511, True)


def test_host_form_and_run_containers():
    import roaringbitmap_amd as rb
    cols = np.concatenate([np.arange(65536), (5 << 16) + np.arange(0, 100, 2)])
    a = BSI.from_columns(cols, cols & 255)
    a.ebm = O.run_optimize(a.ebm)
    x = _rb_index(rb.RoaringBitmapSliceIndex, a)
    x.setValues([7, 9, 7], [1, 2, 200])  # the pairs leave ebM unchanged: its bytes stay
    assert _rb_bytes(x) == _want(set_reference(a, [7, 9, 7], [1, 2, 200]))
    with pytest.raises(rb.IllegalArgumentException, match="gpu=True"):
        x.setValues([(9 << 16) + 1], [3])
    ro = BSI.from_columns(np.arange(1000), np.arange(1000) // 100, True)
    assert any(O.stats(s)["run"] for s in ro.ba)
    y = _rb_index(rb.RoaringBitmapSliceIndex, ro)
    with pytest.raises(rb.IllegalArgumentException, match="slice holds a run container"):
        y.setValues([5], [1])
    assert _rb_bytes(y) == _want(ro)
