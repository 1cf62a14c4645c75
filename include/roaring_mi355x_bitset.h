/*
 * roaring_mi355x_bitset.h — dense bitsets and masks to resident bitmaps and back: the C ABI of
 * BitSetUtil (RB/BitSetUtil.java:29-306).  Part of roaring_mi355x.h, which includes it; kept in a file of
 * its own as the third interchange form next to serialized bytes and value lists.
 *
 * A dense bitset crosses the boundary in one of two layouts:
 *   RBG_BITS_PACKED  little-endian 64-bit words, given as n BYTES of any length: a tail of 1..7 bytes is a
 *                    last word (bitmapOf(ByteBuffer), :238-251).  In device memory the pointer must be 8-byte
 *                    aligned (a tensor view t[1:] is); nothing at or past byte n is read.
 *   RBG_BITS_BYTES   a mask of n ELEMENTS, one byte each, nonzero = set (torch.bool, or x > 0 as uint8).
 * The key arithmetic of the reference (from * Long.SIZE, :169) is Java int, defined up to 2^32 bits: more
 * than 2^32 bits (2^29 packed bytes, 2^32 mask elements) is refused.  Bit positions at or above 2^31 work.
 *
 * Every refusal below is RBG_ERR_ILLEGAL_ARGUMENT with a text in rbg_last_error, decided from the arguments
 * before any device work, and makes no batch.
 */
#ifndef ROARING_MI355X_BITSET_H
#define ROARING_MI355X_BITSET_H

#include "roaring_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RBG_BITS_PACKED = 0, RBG_BITS_BYTES = 1 };

/* BitSetUtil.bitmapOf(long[] words) (:160-174, containerOf :270-283) and bitmapOf(ByteBuffer, fastRank)
 * (:185-259), with run_optimize followed by runOptimize() (RB/RoaringBitmap.java:2764-2774), built on the
 * GPU from host memory (staged through the context's pinned buffer): block b = words [1024 b, 1024 b + 1024),
 * zero padded; an all-zero block gives no container, another gives key b, an array up to 4,096 bits, else a
 * bitmap.  *batch: a new one-bitmap batch, field for field the one rbg_ctx_from_values makes of the bit
 * positions, so every call that takes a resident bitmap takes it.  n == 0: a live empty batch.
 * Refused: an unknown layout, more than 2^32 bits, a null pointer with n > 0. */
int rbg_ctx_from_bitset(rbg_ctx* ctx, const void* bits, uint64_t n, int layout, int run_optimize, int32_t* batch);
/* The same from device memory, read in place: no copy of packed words, one pass packing a mask into pooled
 * words.  The input is read by several kernels and must not change until the call returns (the call reads the
 * container count and the batch totals back, so it returns after the last read).  Also refused: a packed
 * pointer that is not 8-byte aligned. */
int rbg_ctx_from_bitset_device(rbg_ctx* ctx, const void* bits_dev, uint64_t n, int layout, int run_optimize,
                               int32_t* batch);

/* BitSetUtil.toLongArray(bitmap) (:67-108) over a window: the bit positions [first, first + n) of bitmap i of
 * a batch into out (host memory), absent keys and everything past the last value being zeros.
 *   RBG_BITS_PACKED  first % 64 == 0; out: ceil(n / 64) words, bits at or past n in the last word zero
 *   RBG_BITS_BYTES   any first; out: n bytes of 0 / 1
 * The window's size is the caller's: toLongArray's own length (wordsInUse, :76-79) is rbg_bitset_expand's.
 * Every word / byte of the window is written exactly once and nothing outside it.  The batch must be a
 * one-bitmap key-major slot-aligned batch, as the pairwise ops and rbg_ctx_to_values require.
 * Refused: an unknown layout, first % 64 != 0 (packed), first + n > 2^32, such a batch not given. */
int rbg_ctx_to_bitset(rbg_ctx* ctx, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout, void* out);
/* The same into device memory (packed: 8-byte aligned), enqueued on the context stream with no host
 * synchronisation: nothing is read back. */
int rbg_ctx_to_bitset_device(rbg_ctx* ctx, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout,
                             void* out_dev);

/* One-shot BitSetUtil.bitmapOf (:160-174 / :185-259) [+ runOptimize] on the GPU: upload, build, fetch the
 * serialized bitmap, release.  Same bytes as rbg_from_values of the bit positions.  Without a usable
 * device: RBG_ERR_DEVICE; the refusals of rbg_ctx_from_bitset come first. */
int rbg_bitset_build(const void* bits, uint64_t n, int layout, int run_optimize, rbg_buffer* out);
/* One-shot BitSetUtil.toLongArray(bitmap) (:67-108) on the GPU: load, expand, release.  out: the words,
 * little-endian, out->len = 8 * wordsInUse: 0 for an empty bitmap, else last / 64 + 1 words for last >= 64
 * and 2 words for every last in 0..63 (:76-79, a trailing zero word included, as the reference has it).
 * A last value of at least 2^31 (last() < 0, :72-75): RBG_ERR_ILLEGAL_ARGUMENT, "bitmap has negative bits
 * set". */
int rbg_bitset_expand(const uint8_t* buf, size_t len, rbg_buffer* out);

#ifdef __cplusplus
}
#endif
#endif /* ROARING_MI355X_BITSET_H */
