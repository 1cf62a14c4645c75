"""ctypes binding of libroaring_mi355x.so (include/roaring_mi355x.h).

The library is built in-tree (roaringbitmap_amd/_build.py).  There is no CPU
fallback: if the shared object is missing this module raises at import time,
and every compute call returns RBG_ERR_DEVICE when no gfx950 device is present.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RBG_LIB") or os.path.join(HERE, "lib", "libroaring_mi355x.so")

RBG_OK = 0
RBG_ERR_INVALID_FORMAT = -1
RBG_ERR_TRUNCATED = -2
RBG_ERR_ILLEGAL_ARGUMENT = -3
RBG_ERR_DEVICE = -4
RBG_ERR_OUT_OF_MEMORY = -5

OP = {"and": 0, "or": 1, "xor": 2, "andnot": 3, "ior": 4,  # ior: x1.or(x2) in place (Container.ior types)
      "and_buffer": 5, "andnot_buffer": 6}  # the buffer package's and / andNot (ImmutableRoaringBitmap)
CARD_OP = {"and": 0, "or": 1, "xor": 2, "andnot": 3, "intersects": 4, "contains": 5}
WIDE_OP = {"and": 0, "or": 1, "xor": 2, "and_iter": 3, "naive_and": 4, "workshy_and": 5, "parallel_or": 6,
           "parallel_xor": 7, "buffer_or_mutable": 8, "horizontal_or": 9, "horizontal_xor": 10,
           "priorityqueue_or": 11, "priorityqueue_xor": 12, "buffer_and": 13, "buffer_naive_and": 14,
           "buffer_and_iter": 15}
WIDE_CARD_OP = {"and": 0, "or": 1}
RANGE_OP = {"and": 0, "or": 1, "xor": 2, "andnot": 3,
            "and_buffer": 4, "or_buffer": 5, "xor_buffer": 6, "andnot_buffer": 7}  # ImmutableRoaringBitmap's
RBG_ORNOT_INPLACE, RBG_ORNOT_BUFFER = 1, 2
RMUT_OP = {"add": 0, "remove": 1, "flip": 2, "add_inplace": 3}  # rbg_range_mut (| RBG_RMUT_BUFFER: MutableRoaringBitmap's)
RBG_RMUT_BUFFER = 4
PQ_OP = {"rank": 0, "select": 1, "contains": 2, "next": 3, "prev": 4}  # rbg_point_query (RBG_PQ_*)
OPERATIONS = ("EQ", "NEQ", "LE", "LT", "GE", "GT", "RANGE")  # BitmapSliceIndex.Operation order (rbg_bsi_compare)


def bsi_op(op):
    """the code of a BSI compare operation given by name (OPERATIONS) or as the code itself"""
    return OPERATIONS.index(op) if isinstance(op, str) else int(op)


class rbg_buffer(ctypes.Structure):
    _fields_ = [("data", ctypes.POINTER(ctypes.c_uint8)), ("len", ctypes.c_size_t)]


# the header's C types, named once: int, int32_t, int64_t, uint64_t, size_t; void*, const uint8_t*, rbg_buffer*;
# const uint8_t* const*, size_t* and the pointers to the fixed-width integers
P = ctypes.POINTER
ci, i32, i64, u64, sz = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
vp, u8p, buf = ctypes.c_void_p, ctypes.c_char_p, P(rbg_buffer)
strs, szp, u32p, i32p, i64p, u64p = P(ctypes.c_char_p), P(sz), P(ctypes.c_uint32), P(i32), P(i64), P(u64)


# Every entry point of include/roaring_mi355x.h, in the header's order: name -> (restype, argtypes).  lib()
# applies it.  An entry point without argtypes would take a Python int as a C int, silently.
_BSI_COMPARE = [ci, i32, i32, u8p, sz, strs, szp, sz, i32, i32, u8p, sz, buf]
SIGNATURES = {
    "rbg_range_op": (ci, [ci, strs, szp, sz, i64, i64, buf]),
    "rbg_ornot": (ci, [u8p, sz, u8p, sz, i64, ci, buf]),
    "rbg_range_mut": (ci, [ci, u8p, sz, i64, i64, buf]),
    "rbg_add_offset": (ci, [u8p, sz, i64, buf]),
    "rbg_remove_run_compression": (ci, [u8p, sz, buf]),
    "rbg_limit": (ci, [u8p, sz, i32, buf]),
    "rbg_point_query": (ci, [ci, u8p, sz, u32p, sz, i64p]),
    "rbg_build_values": (ci, [u32p, sz, ci, buf]),
    "rbg_expand_values": (ci, [u8p, sz, buf]),
    "rbg_bitmap_of_range": (ci, [i64, i64, buf]),
    "rbg_select_range": (ci, [u8p, sz, i64, i64, ci, buf]),
    "rbg_pairwise": (ci, [ci, u8p, sz, u8p, sz, buf]),
    "rbg_pairwise_inplace": (ci, [ci, u8p, sz, u8p, sz, ci, buf]),
    "rbg_pairwise_card": (ci, [ci, u8p, sz, u8p, sz, i32p]),
    "rbg_wide": (ci, [ci, strs, szp, i32p, sz, buf]),
    "rbg_wide_card": (ci, [ci, strs, szp, sz, i32p]),
    "rbg_batch_and_card": (ci, [sz, strs, szp, strs, szp, i32p]),
    "rbg_bsi_compare": (ci, _BSI_COMPARE),
    "rbg_bsi_compare_buffer": (ci, _BSI_COMPARE),
    "rbg_bsi_sum": (ci, [u8p, sz, strs, szp, sz, u8p, sz, i64p]),
    "rbg_bsi_from_columns": (ci, [u32p, i32p, sz, ci, vp, i32p]),
    "rbg_bsi_get_values": (ci, [u8p, sz, strs, szp, ci, u32p, sz, i64p]),
    "rbg_bsi_add": (ci, [u8p, sz, strs, szp, ci, i32, i32, u8p, sz, strs, szp, ci, vp, i32p]),
    "rbg_bsi_set_values": (ci, [u8p, sz, strs, szp, ci, i32, i32, u32p, i32p, sz, vp, i32p]),
    "rbg_bsi_in": (ci, [u8p, sz, strs, szp, ci, u8p, sz, i32p, sz, ci, buf]),
    "rbg_bsi_transpose": (ci, [u8p, sz, strs, szp, ci, u8p, sz, ci, vp, i32p]),
    "rbg_free": (None, [buf]),
    "rbg_set_devices": (ci, [u64]),
    "rbg_last_error": (u8p, []),
    "rbg_version": (ci, []),
    "rbg_trim": (None, []),
    "rbg_pool_evictions": (u64, []),
    "rbg_from_values": (ci, [u32p, sz, ci, buf]),
    "rbg_run_optimize": (ci, [u8p, sz, buf]),
    "rbg_to_values": (ci, [u8p, sz, buf]),
    "rbg_inspect": (ci, [u8p, sz, szp, i64p, i64p]),
    "rbg_ctx_create": (ci, [ci, P(vp)]),
    "rbg_ctx_destroy": (None, [vp]),
    "rbg_ctx_stream": (vp, [vp]),
    "rbg_ctx_sync": (ci, [vp]),
    "rbg_ctx_profile": (ci, [vp, ci]),
    "rbg_ctx_profile_compute": (ci, [vp, ci]),
    "rbg_ctx_profile_read": (ci, [vp, P(ctypes.c_double), P(ci)]),
    "rbg_ctx_profile_bytes": (ci, [vp, i64p]),
    "rbg_ctx_load_separate": (ci, [vp, strs, szp, sz, i32p]),
    "rbg_ctx_load": (ci, [vp, strs, szp, sz, i32p]),
    "rbg_ctx_load_packed": (ci, [vp, strs, szp, sz, i32p]),
    "rbg_ctx_synth": (ci, [vp, ci, u64, sz, ci, ci, i32p]),
    "rbg_ctx_release": (ci, [vp, i32]),
    "rbg_ctx_select_range": (ci, [vp, i32, i64, i64, i32p]),
    "rbg_ctx_run_optimize": (ci, [vp, i32, i32p, P(ctypes.c_uint8)]),
    "rbg_run_optimize_many": (ci, [vp, szp, sz, vp, P(ctypes.c_uint8)]),
    "rbg_ctx_batch_minmax": (ci, [vp, i32, i32p]),
    "rbg_ctx_batch_stats": (ci, [vp, i32, i64p]),
    "rbg_ctx_batch_fetch": (ci, [vp, i32, sz, buf]),
    "rbg_ctx_batch_fetch_range": (ci, [vp, i32, sz, sz, vp]),
    "rbg_ctx_pairwise": (ci, [vp, ci, i32, sz, i32, sz]),
    "rbg_ctx_pairwise_serialized": (ci, [vp, ci, i32, sz, i32, sz]),
    "rbg_ctx_pairwise_range": (ci, [vp, ci, i32, sz, i32, sz, ci, ci]),
    "rbg_ctx_ornot": (ci, [vp, i32, sz, i32, sz, i64, ci]),
    "rbg_ctx_range_mut": (ci, [vp, ci, i32, sz, i64, i64]),
    "rbg_ctx_add_offset": (ci, [vp, i32, sz, i64]),
    "rbg_ctx_pairwise_card": (ci, [vp, ci, i32, sz, i32, sz]),
    "rbg_ctx_wide": (ci, [vp, ci, i32, ci, ci, i32p]),
    "rbg_ctx_wide_card": (ci, [vp, ci, i32, ci, ci]),
    "rbg_ctx_wide_start": (ci, [vp, ci, i32, ci, ci, i32p, i32]),
    "rbg_ctx_pair_bytes": (ci, [vp, i32, i64p]),
    "rbg_ctx_bsi": (ci, [vp, i32, ci, ci, ci, i32, i32, i32, i32, ci]),
    "rbg_ctx_bsi_sums": (ci, [vp, i64p]),
    "rbg_ctx_bsi_buffer": (ci, [vp, i32, ci, ci, ci, i32, i32, i32, i32]),
    "rbg_ctx_bsi_sums_device": (ci, [vp, vp]),
    "rbg_ctx_bsi_sums_target": (ci, [vp, vp]),
    "rbg_ctx_point_query": (ci, [vp, ci, i32, sz, u32p, sz, i64p]),
    "rbg_ctx_point_query_device": (ci, [vp, ci, i32, sz, vp, sz, vp]),
    "rbg_ctx_from_values": (ci, [vp, u32p, sz, ci, i32p]),
    "rbg_ctx_from_values_device": (ci, [vp, vp, sz, ci, i32p]),
    "rbg_ctx_to_values": (ci, [vp, i32, sz, u64, u64, u32p, u64p]),
    "rbg_ctx_to_values_device": (ci, [vp, i32, sz, u64, u64, ci, vp, u64p]),
    "rbg_ctx_bsi_from_columns": (ci, [vp, u32p, i32p, sz, ci, i32p, i32p]),
    "rbg_ctx_bsi_from_columns_device": (ci, [vp, vp, vp, sz, ci, i32p, i32p]),
    "rbg_ctx_bsi_add": (ci, [vp, i32, ci, i32, ci, i32, i32, i32p, i32p]),
    "rbg_ctx_bsi_set_values": (ci, [vp, i32, ci, i32, i32, u32p, i32p, sz, i32p, i32p]),
    "rbg_ctx_bsi_set_values_device": (ci, [vp, i32, ci, i32, i32, vp, vp, sz, i32p, i32p]),
    "rbg_ctx_bsi_in": (ci, [vp, i32, ci, ci, i32p, sz, ci, i32p]),
    "rbg_ctx_bsi_transpose": (ci, [vp, i32, ci, ci, ci, i32p, i32p]),
    "rbg_ctx_bsi_get_values": (ci, [vp, i32, ci, ci, u32p, sz, i64p]),
    "rbg_ctx_bsi_get_values_device": (ci, [vp, i32, ci, ci, vp, sz, vp]),
    "rbg_ctx_bsi_to_pairs": (ci, [vp, i32, ci, ci, ci, ci, vp, vp, u64p]),
    "rbg_ctx_bsi_to_pairs_device": (ci, [vp, i32, ci, ci, ci, ci, vp, vp, u64p]),
    "rbg_ctx_batch_counts": (ci, [vp, i32, u32p, sz]),
    "rbg_synth_key_bytes": (ci, [ci, u64, sz, u64p]),
    "rbg_ctx_batch_and_card": (ci, [vp, i32]),
    "rbg_ctx_card": (ci, [vp, i32p]),
    "rbg_ctx_cards": (ci, [vp, i32p, sz]),
    "rbg_ctx_result_stats": (ci, [vp, i64p]),
    "rbg_ctx_serialize": (ci, [vp]),
    "rbg_ctx_fetch": (ci, [vp, buf]),
    "rbg_ctx_fetch_shard": (ci, [vp, i64, ci, i64, i64, buf, buf, buf]),
    "rbg_ctx_fetch_shard_device": (ci, [vp, i64, ci, i64, vp, vp, vp, vp]),
    "rbg_ctx_result_layout_device": (ci, [vp, vp]),
    "rbg_ctx_fetch_shard_device_dyn": (ci, [vp, vp, ci, ci, vp, vp]),
}
EXPORTED = list(SIGNATURES)  # the names alone

# Every entry point of include/roaring_mi355x_bitset.h (BitSetUtil: dense bitsets and masks), which
# roaring_mi355x.h includes, in that file's order.  lib() applies it with the table above.
RBG_BITS_PACKED, RBG_BITS_BYTES = 0, 1
BITSET_SIGNATURES = {
    "rbg_ctx_from_bitset": (ci, [vp, vp, u64, ci, ci, i32p]),
    "rbg_ctx_from_bitset_device": (ci, [vp, vp, u64, ci, ci, i32p]),
    "rbg_ctx_to_bitset": (ci, [vp, i32, sz, u64, u64, ci, vp]),
    "rbg_ctx_to_bitset_device": (ci, [vp, i32, sz, u64, u64, ci, vp]),
    "rbg_bitset_build": (ci, [vp, u64, ci, ci, buf]),
    "rbg_bitset_expand": (ci, [u8p, sz, buf]),
}

# Every entry point of include/roaring_mi355x_rangebitmap.h (RangeBitmap: the range-encoded index), which
# roaring_mi355x.h includes, in that file's order.
RANGEBITMAP_OP = {"lte": 0, "lt": 1, "gt": 2, "gte": 3, "eq": 4, "neq": 5, "between": 6}  # RBG_RB_*
RANGEBITMAP_SIGNATURES = {
    "rbg_rangebitmap_validate": (ci, [u8p, sz, u64p]),
    "rbg_ctx_rangebitmap_load": (ci, [vp, u8p, sz, i32p]),
    "rbg_ctx_rangebitmap_release": (ci, [vp, i32]),
    "rbg_ctx_rangebitmap_info": (ci, [vp, i32, u64p]),
    "rbg_ctx_rangebitmap_query": (ci, [vp, i32, ci, u64, u64, i32, sz, i32p]),
    "rbg_ctx_rangebitmap_count": (ci, [vp, i32, ci, u64, u64, i32, sz, i64p]),
    "rbg_rangebitmap_query": (ci, [u8p, sz, ci, u64, u64, u8p, sz, buf]),
    "rbg_rangebitmap_count": (ci, [u8p, sz, ci, u64, u64, u8p, sz, i64p]),
}

# Every entry point of include/roaring_mi355x_rangebitmap_build.h (RangeBitmap.Appender on the device, and a
# resident index back to the reference's stream), which roaring_mi355x.h includes, in that file's order.
RANGEBITMAP_BUILD_SIGNATURES = {
    "rbg_ctx_rangebitmap_build": (ci, [vp, vp, u64, u64, ci, i32p]),
    "rbg_ctx_rangebitmap_build_device": (ci, [vp, vp, u64, u64, ci, i32p]),
    "rbg_ctx_rangebitmap_serialize": (ci, [vp, i32, buf]),
    "rbg_rangebitmap_build": (ci, [vp, u64, u64, ci, buf]),
    "rbg_rangebitmap_reserialize": (ci, [u8p, sz, buf]),
}

# Every entry point of include/roaring_mi355x_mutate.h (batches of values added to or removed from a bitmap),
# which roaring_mi355x.h includes, in that file's order.
RBG_MUT_ADD, RBG_MUT_REMOVE = 0, 1
MUTATE_SIGNATURES = {
    "rbg_ctx_mutate_values": (ci, [vp, i32, ci, u32p, sz, i32p, u64p]),
    "rbg_ctx_mutate_values_device": (ci, [vp, i32, ci, vp, sz, i32p, u64p]),
    "rbg_mutate_values": (ci, [u8p, sz, ci, u32p, sz, buf, u64p]),
    "rbg_mutate_values_host": (ci, [u8p, sz, ci, u32p, sz, buf, u64p]),
}

_lib = None


def lib():
    """Load the engine library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the engine has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in {**SIGNATURES, **BITSET_SIGNATURES, **RANGEBITMAP_SIGNATURES,
                                          **RANGEBITMAP_BUILD_SIGNATURES, **MUTATE_SIGNATURES}.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


class RoaringError(Exception):
    pass


class InvalidRoaringFormat(RoaringError, OSError):
    """RB/InvalidRoaringFormat.java surfaced as IOException (RB/RoaringBitmap.java:1779-1811)."""


class TruncatedInput(RoaringError, OSError):
    """EOFException / BufferUnderflowException on a truncated buffer."""


class IllegalArgumentException(RoaringError, ValueError):
    pass


class ArrayIndexOutOfBoundsException(RoaringError, IndexError):
    """java.lang.ArrayIndexOutOfBoundsException, where the reference's own control flow throws it on
    caller-supplied input (FastAggregation.workAndMemoryShyAnd with a dirty buffer, RB/FastAggregation.java:541-548)"""


class NoSuchElementException(RoaringError, LookupError):
    """java.util.NoSuchElementException: first() / last() of an empty bitmap (RB/RoaringArray.java:971-1027)"""


class DeviceError(RoaringError, RuntimeError):
    pass


def check(status):
    if status >= 0:
        return status
    msg = lib().rbg_last_error().decode(errors="replace")
    cls = {RBG_ERR_INVALID_FORMAT: InvalidRoaringFormat, RBG_ERR_TRUNCATED: TruncatedInput,
           RBG_ERR_ILLEGAL_ARGUMENT: IllegalArgumentException}.get(status, DeviceError)
    raise cls(f"status {status}: {msg}")


def take(b: rbg_buffer) -> bytes:
    if b.len >= 1 << 31:  # string_at takes its size as a C int
        out = bytes((ctypes.c_ubyte * b.len).from_address(ctypes.addressof(b.data.contents)))
    else:
        out = ctypes.string_at(b.data, b.len) if b.len else b""
    lib().rbg_free(ctypes.byref(b))
    return out


def buf_array(bufs):
    n = len(bufs)
    arr = (ctypes.c_char_p * max(n, 1))(*bufs)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in bufs])
    return arr, lens


def call_bytes(f, *args) -> bytes:
    """f(*args, &buffer) -> the bytes the library left in the buffer, which is freed"""
    b = rbg_buffer()
    check(f(*args, ctypes.byref(b)))
    return take(b)


def ids_array(ids):
    """the identity ids of a wide op's inputs as int32[], or a null pointer"""
    return None if ids is None else (ctypes.c_int32 * len(ids))(*ids)


def is_torch(x) -> bool:
    """a torch tensor or dtype, told without importing torch"""
    return type(x).__module__.split(".")[0] == "torch"


def as_u32(values) -> np.ndarray:
    """values (Java ints or their unsigned patterns) as a flat contiguous uint32 array: the low 32 bits"""
    return np.ascontiguousarray(np.asarray(values, dtype=np.int64).astype(np.uint32)).reshape(-1)


def in_list(values) -> np.ndarray:
    """the value list of an IN query as contiguous int32: Java ints, or their unsigned bit patterns"""
    if isinstance(values, np.ndarray) and values.dtype in (np.int32, np.uint32):
        return np.ascontiguousarray(values.reshape(-1)).view(np.int32)
    v = np.asarray(values if isinstance(values, np.ndarray) else list(values), dtype=np.int64).reshape(-1)
    if v.size and (v.min() < -(1 << 31) or v.max() >= 1 << 32):
        raise IllegalArgumentException("the values of an IN list must fit 32 bits")
    return np.ascontiguousarray(v.astype(np.uint32).view(np.int32))


def pair_arrays(columns, values):
    """(column, value) pairs as flat contiguous arrays of one length, uint32 columns and int32 values (Java's
    non-negative ints): the host front of the calls that write pairs into a bit-sliced index"""
    c = np.asarray(columns, dtype=np.int64).reshape(-1)
    v = np.asarray(values, dtype=np.int64).reshape(-1)
    if c.size != v.size:
        raise IllegalArgumentException("columns and values differ in length")
    if v.size and (v.min() < 0 or v.max() >= 1 << 31):
        raise IllegalArgumentException("Values should be non-negative and below 2^31")
    return np.ascontiguousarray(c.astype(np.uint32)), np.ascontiguousarray(v.astype(np.int32))
