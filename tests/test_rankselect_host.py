"""Point-query entry points (rbg_point_query, rbg_ctx_point_query, rbg_ctx_point_query_device) without a
device: the symbols, the op codes, and the argument checks that come before any device use."""
import ctypes
import os
import re

import numpy as np

from roaringbitmap_amd import _lib as L

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x.h")
SYMBOLS = ["rbg_point_query", "rbg_ctx_point_query", "rbg_ctx_point_query_device"]


def _header():
    src = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(L.LIB_PATH)
    src = _header()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in L.EXPORTED


def test_op_codes_match_header():
    src = _header()
    names = {"rank": "RBG_PQ_RANK", "select": "RBG_PQ_SELECT", "contains": "RBG_PQ_CONTAINS", "next": "RBG_PQ_NEXT",
             "prev": "RBG_PQ_PREV"}
    assert set(names) == set(L.PQ_OP)
    for k, c in names.items():
        m = re.search(r"\b" + c + r"\s*=\s*(\d+)", src)
        assert m and int(m.group(1)) == L.PQ_OP[k], k
    assert [L.PQ_OP[k] for k in ("rank", "select", "contains", "next", "prev")] == [0, 1, 2, 3, 4]


def _call(op, buf, q, n, out):
    qp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if q is not None else None
    op_ = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if out is not None else None
    return L.lib().rbg_point_query(op, buf, len(buf), qp, n, op_)


def test_argument_checks_come_before_any_device_use():
    """ILLEGAL_ARGUMENT (-3), not DEVICE (-4): on a machine without a GPU the first device call fails, so
    a status of -3 shows the check came first; on one with a GPU the same status is required"""
    buf = O.from_values(np.arange(10, dtype=np.uint32))
    q = np.array([1, 2, 3], dtype=np.uint32)
    out = np.full(3, 77, dtype=np.int64)
    assert _call(L.PQ_OP["rank"], buf, q, 3, None) == L.RBG_ERR_ILLEGAL_ARGUMENT  # null out
    assert _call(L.PQ_OP["rank"], buf, None, 3, out) == L.RBG_ERR_ILLEGAL_ARGUMENT  # null queries
    assert _call(99, buf, q, 3, out) == L.RBG_ERR_ILLEGAL_ARGUMENT  # unknown op
    assert _call(5, buf, q, 3, out) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert _call(16, buf, q, 3, out) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert _call(-1, buf, q, 3, out) == L.RBG_ERR_ILLEGAL_ARGUMENT
    # n == 0: RBG_OK and nothing touched, null pointers included
    assert _call(L.PQ_OP["select"], buf, None, 0, None) == L.RBG_OK
    assert _call(L.PQ_OP["select"], buf, q, 0, out) == L.RBG_OK
    assert (out == 77).all()
    # the session entry points check their arguments the same way (a null context needs no device)
    lib = L.lib()
    assert lib.rbg_ctx_point_query(None, 0, 0, 0, None, 0, None) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert lib.rbg_ctx_point_query_device(None, 0, 0, 0, None, 0, None) == L.RBG_ERR_ILLEGAL_ARGUMENT


def test_python_surface():
    import roaringbitmap_amd as rb
    assert issubclass(rb.NoSuchElementException, rb.RoaringError) and issubclass(rb.NoSuchElementException, LookupError)
    for cls in (rb.RoaringBitmap, rb.ImmutableRoaringBitmap, rb.MutableRoaringBitmap):
        for m in ("rank", "rankLong", "select", "nextValue", "previousValue", "first", "last", "rangeCardinality",
                  "rank_many", "select_many", "contains_many", "next_values", "previous_values"):
            assert callable(getattr(cls, m)), (cls, m)
    assert callable(rb.Engine.point_query)
    x = rb.RoaringBitmap(O.from_values(np.arange(10, dtype=np.uint32)))
    # host checks of rangeCardinality: no device is reached
    assert x.rangeCardinality(100, 100) == 0 and x.rangeCardinality(9, 3) == 0
    for st, en in ((-1, 10), (0, (1 << 32) + 1)):
        try:
            x.rangeCardinality(st, en)
        except ValueError:
            continue
        raise AssertionError((st, en))
