"""BitSetUtil (RB/BitSetUtil.java) without a device: the symbols of the dense-bitset entry points, the refusals
they decide from their arguments before any device use, and the host forms of bitmapOf / toLongArray /
toByteArray / equals.  The oracle of a build is the host builder over the set bit positions; the shapes are
those of the reference's TestBitSetUtil, regenerated here from seeds."""
import ctypes
import os
import re

import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "roaring_mi355x_bitset.h")
SYMBOLS = ["rbg_ctx_from_bitset", "rbg_ctx_from_bitset_device", "rbg_ctx_to_bitset", "rbg_ctx_to_bitset_device",
           "rbg_bitset_build", "rbg_bitset_expand"]
BU = rb.BitSetUtil


def test_symbols_exported_declared_and_typed():
    lib = ctypes.CDLL(L.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    main = open(os.path.join(ROOT, "include", "roaring_mi355x.h")).read()
    assert '#include "roaring_mi355x_bitset.h"' in main
    assert sorted(set(re.findall(r"\b(rbg_\w+)\s*\(", src))) == sorted(SYMBOLS)
    assert sorted(L.BITSET_SIGNATURES) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(L.lib(), name).argtypes is not None, name
    assert (L.RBG_BITS_PACKED, L.RBG_BITS_BYTES) == (0, 1) and BU.BLOCK_LENGTH == 1024
    assert re.search(r"RBG_BITS_PACKED = 0, RBG_BITS_BYTES = 1", src)
    from roaringbitmap_amd import _build
    assert "bitset.hip" in _build.SOURCES
    for f in ("from_words", "from_mask", "to_words", "to_mask"):
        assert callable(getattr(rb.Engine, f))


def _err():
    return L.lib().rbg_last_error().decode()


def test_refusals_come_before_any_device_use():
    """every refusal is RBG_ERR_ILLEGAL_ARGUMENT with its own text, and it comes before the handle is even
    looked at: a null handle with good arguments is refused too, but with no such text"""
    lib = L.lib()
    bad = L.RBG_ERR_ILLEGAL_ARGUMENT
    words = np.arange(4, dtype=np.uint64)
    p = ctypes.c_void_p(words.ctypes.data)
    out = ctypes.c_int32(-7)
    b = L.rbg_buffer()
    for f in (lib.rbg_ctx_from_bitset, lib.rbg_ctx_from_bitset_device):
        assert f(None, p, 32, 2, 0, ctypes.byref(out)) == bad and "unknown layout" in _err()
        assert f(None, p, 32, -1, 0, ctypes.byref(out)) == bad and "unknown layout" in _err()
        assert f(None, p, (1 << 29) + 1, L.RBG_BITS_PACKED, 0, ctypes.byref(out)) == bad and "2^32 bits" in _err()
        assert f(None, p, (1 << 32) + 1, L.RBG_BITS_BYTES, 0, ctypes.byref(out)) == bad and "2^32 bits" in _err()
        assert f(None, None, 8, L.RBG_BITS_PACKED, 0, ctypes.byref(out)) == bad and "no input" in _err()
        assert f(None, p, 32, L.RBG_BITS_PACKED, 0, ctypes.byref(out)) == bad  # the null handle
    odd = ctypes.c_void_p(words.ctypes.data + 4)
    assert lib.rbg_ctx_from_bitset_device(None, odd, 8, L.RBG_BITS_PACKED, 0, ctypes.byref(out)) == bad
    assert "8-byte aligned" in _err()
    assert lib.rbg_bitset_build(p, 32, 7, 0, ctypes.byref(b)) == bad and "unknown layout" in _err()
    assert lib.rbg_bitset_build(p, (1 << 29) + 8, L.RBG_BITS_PACKED, 0, ctypes.byref(b)) == bad and "2^32 bits" in _err()
    assert lib.rbg_bitset_build(p, 32, L.RBG_BITS_PACKED, 0, None) == bad
    for f in (lib.rbg_ctx_to_bitset, lib.rbg_ctx_to_bitset_device):
        assert f(None, 0, 0, 0, 64, 5, p) == bad and "unknown layout" in _err()
        assert f(None, 0, 0, 1, 64, L.RBG_BITS_PACKED, p) == bad and "multiple of 64" in _err()
        assert f(None, 0, 0, 64, 1 << 32, L.RBG_BITS_PACKED, p) == bad and "past 2^32" in _err()
        assert f(None, 0, 0, (1 << 32) - 5, 6, L.RBG_BITS_BYTES, p) == bad and "past 2^32" in _err()
        assert f(None, 0, 0, 1 << 63, 1 << 63, L.RBG_BITS_BYTES, p) == bad and "past 2^32" in _err()
        assert f(None, 0, 0, 5, 64, L.RBG_BITS_BYTES, p) == bad  # the null handle
    assert lib.rbg_bitset_expand(None, 8, ctypes.byref(b)) == bad
    assert lib.rbg_bitset_expand(O.from_values(np.arange(3, dtype=np.uint32)), 22, None) == bad
    assert out.value == -7 and not b.data
    with pytest.raises(rb.IllegalArgumentException, match="2\\^32 bits"):
        BU.bitmapOf(np.zeros((1 << 29) + 1, dtype=np.uint8))


def _shapes():
    """name -> bits (uint8 0 / 1, a whole number of words), after TestBitSetUtil's cases"""
    rng = np.random.default_rng(20261021)
    out = {}
    out["empty"] = np.zeros(0, dtype=np.uint8)
    one = np.zeros(64, dtype=np.uint8)
    one[1] = 1
    out["one_bit"] = one
    far = np.zeros(10_000_000 + 64 - 10_000_000 % 64, dtype=np.uint8)
    far[[1, 10_000_000]] = 1
    out["bits_1_and_10M"] = far
    out["full_block"] = np.ones(1 << 16, dtype=np.uint8)
    gaps = np.zeros(9 << 16, dtype=np.uint8)  # blocks 0, 3 and 8 hold bits, the others none
    for k, n in ((0, 5), (3, 4096), (8, 30000)):
        gaps[(k << 16) + rng.choice(1 << 16, n, replace=False)] = 1
    out["gap_blocks"] = gaps
    out["random_blocks"] = (rng.random(5 << 16) < np.repeat([0.001, 0.05, 0.0626, 0.5, 0.99], 1 << 16)).astype(np.uint8)
    out["flip_flap"] = np.repeat(np.arange(10) % 2 == 0, 1 << 16).astype(np.uint8)  # full, empty, full, ...
    out["short_last_block"] = (rng.random((1 << 16) + 64 * 37) < 0.3).astype(np.uint8)
    return out


SHAPES = _shapes()


def _words(bits):
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


@pytest.mark.parametrize("ro", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_bitmap_of_words_is_the_host_builder(name, ro):
    bits = SHAPES[name]
    want = O.from_values(np.flatnonzero(bits).astype(np.uint32), ro)
    w = _words(bits)
    assert BU.bitmapOf(w, run_optimize=ro).serialize() == want
    assert BU.bitmapOf(w.view(np.int64), fastRank=True, run_optimize=ro).serialize() == want
    assert BU.bitmapOf(w.tobytes(), run_optimize=ro).serialize() == want


def test_full_block_types():
    bits = SHAPES["full_block"]
    assert BU.bitmapOf(_words(bits)).container_stats() == (0, 1, 0)
    assert BU.bitmapOf(_words(bits), run_optimize=True).container_stats() == (0, 0, 1)


@pytest.mark.parametrize("ro", [False, True])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9])
def test_bitmap_of_bytes_with_a_tail(n, ro):
    """little-endian bytes; a tail of 1..7 bytes is a last word"""
    b = np.random.default_rng(n).integers(1, 256, size=n, dtype=np.uint8)
    pos = np.flatnonzero(np.unpackbits(b, bitorder="little")).astype(np.uint32)
    assert n == 0 or pos.size
    want = O.from_values(pos, ro)
    assert BU.bitmapOf(b.tobytes(), run_optimize=ro).serialize() == want
    assert BU.bitmapOf(b, run_optimize=ro).serialize() == want
    padded = np.concatenate([b, np.zeros(-n % 8, dtype=np.uint8)]).view("<u8")
    assert BU.bitmapOf(padded, run_optimize=ro).serialize() == want


LENGTHS = {0: 2, 1: 2, 63: 2, 64: 2, 65: 2, 127: 2, 128: 3, 65535: 1024, 65536: 1025, (1 << 31) - 1: 1 << 25}


@pytest.mark.parametrize("last", list(LENGTHS))
def test_to_long_array_length(last):
    """wordsInUse (:76-79): last / 64 + 1 for last >= 64 and 2 for every last in 0..63, not tidied"""
    assert BU.wordsInUse(last) == LENGTHS[last]
    if last < 1 << 20:  # the largest case through the length helper alone: 256 MiB are not allocated
        w = BU.toLongArray(rb.RoaringBitmap.from_values([last]))
        assert w.dtype == np.uint64 and w.size == LENGTHS[last]
        assert int(w[last >> 6]) == 1 << (last & 63) and int(np.count_nonzero(w)) == 1


def test_to_long_array_of_nothing_and_of_negative_bits():
    assert BU.toLongArray(rb.RoaringBitmap()).shape == (0,) and BU.toByteArray(rb.RoaringBitmap()) == b""
    for v in ([1 << 31], [5, 0xFFFFFFFF]):
        with pytest.raises(rb.IllegalArgumentException, match="bitmap has negative bits set"):
            BU.toLongArray(rb.RoaringBitmap.from_values(v))
    with pytest.raises(rb.IllegalArgumentException, match="bitmap has negative bits set"):
        BU.wordsInUse(1 << 31)


def test_to_byte_array_is_eight_times_too_long():
    x = rb.RoaringBitmap.from_values([3, 64, 200, 70000])
    w = BU.toLongArray(x)
    b = BU.toByteArray(x)
    assert isinstance(b, bytes) and len(b) == 64 * w.size
    assert b[:8 * w.size] == w.astype("<u8").tobytes() and not any(b[8 * w.size:])


@pytest.mark.parametrize("name", list(SHAPES))
def test_round_trip_and_equals(name):
    bits = SHAPES[name]
    w = _words(bits)
    x = BU.bitmapOf(w)
    back = BU.toLongArray(x)
    pos = np.flatnonzero(bits)
    if pos.size == 0:
        assert back.size == 0
    else:
        assert back.size == LENGTHS.get(int(pos[-1]), max(int(pos[-1]), 64) // 64 + 1)
        n = min(back.size, w.size)
        assert (back[:n] == w[:n]).all() and not back[n:].any() and not w[n:].any()
    assert BU.equals(w, x) and BU.equals(w.tobytes(), x)
    assert BU.bitmapOf(back).serialize() == x.serialize()
    if pos.size:
        other = w.copy()
        other[int(pos[0]) >> 6] ^= np.uint64(1) << np.uint64(int(pos[0]) & 63)  # one bit fewer
        assert not BU.equals(other, x)
        moved = other.copy()
        free = int(np.flatnonzero(bits == 0)[0]) if (bits == 0).any() else None
        if free is not None:  # as many bits, one elsewhere
            moved[free >> 6] |= np.uint64(1) << np.uint64(free & 63)
            assert not BU.equals(moved, x)
