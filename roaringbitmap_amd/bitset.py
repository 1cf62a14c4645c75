"""BitSetUtil (RB/BitSetUtil.java:29-306): dense bitsets to Roaring bitmaps and back.

java.util.BitSet has no counterpart here: a dense bitset is its toLongArray() content, little-endian 64-bit
words as a numpy uint64 / int64 array, or the bytes of such words (a ByteBuffer).  bitsetOf /
bitsetOfWithoutCopy are therefore toLongArray.  The host forms (the default; no device needed) are numpy
over the host builder and toArray(); gpu=True runs the one-shot device forms (rbg_bitset_build /
rbg_bitset_expand) and gives the same bytes and words, as RoaringBitmap.from_values(..., gpu=True) does.
Engine.from_words / from_mask / to_words / to_mask are the resident forms.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import IllegalArgumentException, call_bytes, lib
from .roaring import RoaringBitmap

_MAX_BYTES = 1 << 29  # 2^32 bits: the reference's key arithmetic (from * Long.SIZE, :169) is Java int


def _as_bytes(words_or_bytes) -> np.ndarray:
    """long[] words (numpy uint64 / int64, or a sequence of ints taken as 64-bit patterns) or little-endian
    bytes (bytes-like, numpy uint8) as a flat uint8 array"""
    x = words_or_bytes
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(x, dtype=np.uint8)
    if not isinstance(x, np.ndarray):
        x = np.array([int(w) & 0xFFFFFFFFFFFFFFFF for w in x], dtype=np.uint64)
    if x.dtype == np.uint8:
        return np.ascontiguousarray(x).reshape(-1)
    if x.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)):
        raise ValueError("BitSetUtil: words are uint64 / int64, bytes are uint8")
    return np.ascontiguousarray(x).reshape(-1).astype("<u8", copy=False).view(np.uint8)


def _positions(b: np.ndarray) -> np.ndarray:
    """the set bit positions of little-endian bytes, ascending, a block of 2^16 bits at a time"""
    parts = []
    for off in range(0, b.size, 8192):
        p = np.flatnonzero(np.unpackbits(b[off:off + 8192], bitorder="little"))
        if p.size:
            parts.append(p.astype(np.uint64) + np.uint64(8 * off))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


class BitSetUtil:
    BLOCK_LENGTH = 1024  # words per container (:29-32)

    @staticmethod
    def bitmapOf(words_or_bytes, fastRank=False, run_optimize=False, gpu=False) -> RoaringBitmap:
        """bitmapOf(long[] words) (:160-174; containerOf, :270-283) and bitmapOf(ByteBuffer bb, fastRank)
        (:185-259): block b = words [1024 b, 1024 b + 1024), zero padded, is key b unless it is all zero, an
        array container up to 4,096 bits and a bitmap container above; bytes are little-endian and a tail
        of 1..7 bytes is a last word (:238-251).  Never a run container, unless run_optimize asks for the
        runOptimize() that usually follows (RB/RoaringBitmap.java:2764-2774).  fastRank (a
        FastRankRoaringBitmap in the reference) is accepted and ignored: the rank directory is built on
        demand.  More than 2^32 bits: IllegalArgumentException.  gpu=True: built on the device
        (rbg_bitset_build), the same bytes."""
        b = _as_bytes(words_or_bytes)
        if b.size > _MAX_BYTES:
            raise IllegalArgumentException("bitset: more than 2^32 bits")
        if gpu:
            return RoaringBitmap(call_bytes(lib().rbg_bitset_build, ctypes.c_void_p(b.ctypes.data) if b.size else None,
                                            b.size, _lib.RBG_BITS_PACKED, int(bool(run_optimize))))
        return RoaringBitmap.from_values(_positions(b), run_optimize)

    @staticmethod
    def wordsInUse(last) -> int:
        """the length of toLongArray for a bitmap whose last value is `last` (:76-79): last / 64 + 1 words for
        last >= 64, and 2 for every last in 0..63 (a trailing zero word included, as the reference has it)"""
        last = int(last)
        if last >= 1 << 31 or last < 0:  # last() < 0 (:72-75)
            raise IllegalArgumentException("bitmap has negative bits set")
        last_bit = max(last, 64)
        return (last_bit - last_bit % 64) // 64 + 1

    @staticmethod
    def toLongArray(bitmap, gpu=False) -> np.ndarray:
        """toLongArray(bitmap) (:67-108) -> numpy uint64: no word for an empty bitmap, else wordsInUse(last)
        words, absent keys zero; a value of at least 2^31 raises IllegalArgumentException("bitmap has negative
        bits set") (:72-75).  gpu=True: expanded on the device (rbg_bitset_expand), the same words."""
        if gpu:
            raw = call_bytes(lib().rbg_bitset_expand, bitmap.serialize(), len(bitmap.serialize()))
            return np.frombuffer(raw, dtype="<u8").astype(np.uint64)
        v = bitmap.toArray()
        if v.size == 0:
            return np.zeros(0, dtype=np.uint64)
        words = np.zeros(BitSetUtil.wordsInUse(v[-1]), dtype=np.uint64)
        w = (v >> 6).astype(np.int64)
        bit = np.uint64(1) << (v & 63).astype(np.uint64)
        uw, start = np.unique(w, return_index=True)  # v ascends: every word's bits are adjacent
        words[uw] = np.bitwise_or.reduceat(bit, start)
        return words

    @staticmethod
    def toByteArray(bitmap, gpu=False) -> bytes:
        """toByteArray(bitmap) (:54-60), as the reference has it: it allocates words.length * Long.SIZE bytes
        (:56; 64 per word, not 8) and writes the words little-endian at the front, so the result is eight
        times the data's length and zero behind it."""
        words = BitSetUtil.toLongArray(bitmap, gpu=gpu)
        out = np.zeros(64 * words.size, dtype=np.uint8)
        out[:8 * words.size] = words.astype("<u8", copy=False).view(np.uint8)
        return out.tobytes()

    @staticmethod
    def equals(words, bitmap) -> bool:
        """equals(BitSet, RoaringBitmap) (:294-306): set equality, the cardinalities first and then the
        set bits, on the host"""
        b = _as_bytes(words)
        if int(np.unpackbits(b).sum(dtype=np.int64)) != bitmap.getLongCardinality():
            return False
        return bool(np.array_equal(_positions(b), bitmap.toArray().astype(np.uint64)))
