/*
 * roaring_mi355x_rangebitmap_build.h — the range-encoded index built on the GPU and written back out: the C ABI
 * of RangeBitmap.Appender (RB/RangeBitmap.java:1378-1631; RB/ = RoaringBitmap/src/main/java/org/roaringbitmap/).
 * Part of roaring_mi355x.h, which includes it after roaring_mi355x_rangebitmap.h (map and the queries).
 *
 * An index is built in place on the device from one unsigned 64-bit value per row, registered as the handle a
 * load of the Appender's stream gives, queried and released by the calls of roaring_mi355x_rangebitmap.h, and a
 * resident index, loaded or built, is written back as the reference's stream (Appender.serialize, :1483-1504).
 *
 * Refusals are RBG_ERR_ILLEGAL_ARGUMENT and leave no handle behind.  Decided from the arguments before any
 * device work: a null output, a null pointer with n > 0, n > 65535 * 65536 (more blocks than the header's u16
 * maxKey states).  Decided on the device: a value outside the mask.
 */
#ifndef ROARING_MI355X_RANGEBITMAP_BUILD_H
#define ROARING_MI355X_RANGEBITMAP_BUILD_H

#include "roaring_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* RangeBitmap.appender(max_value) (:52-56), add(values[r]) (:1511-1533) for r = 0 .. n - 1 and build()
 * (:1415-1438), on the GPU from host memory (staged through the context's pinned buffer): *index is the handle
 * rbg_ctx_rangebitmap_load gives for the Appender's stream of the same values, with the same info, answering
 * every query with the same bytes.  The slice count, the mask and the bytes per mask come from max_value | 1
 * (:1622-1630); max_from_data != 0: max_value is not read, the largest value given takes its place (0 for
 * n == 0).  Block k is rows [65536 k, 65536 (k + 1)); slice i of it holds the rows whose value has bit i clear;
 * slices 0-4 are typed by BitmapContainer.runOptimize (a run container iff 2 + 4 runs < 8192, else a bitmap
 * container of any cardinality), slices 5 and up by RunContainer.toEfficientContainer (append, :1543-1588).
 * n == 0: a valid index of no blocks.
 * A value outside the mask: "<the largest value> too large".  The reference's add throws at the first such row
 * with the rows before it added (:1513-1515); this batch form refuses the whole call and adds nothing. */
int rbg_ctx_rangebitmap_build(rbg_ctx* ctx, const uint64_t* values, uint64_t n, uint64_t max_value, int max_from_data,
                              int32_t* index);
/* The same (:1511-1588) from device memory (8-byte aligned), read in place.  The values are read by several
 * kernels and must not change until the call returns (the call reads the largest value and the arena's size
 * back, so it returns after the last read); work that produces them on another stream must be ordered before
 * the context's stream, as for rbg_ctx_from_bitset_device. */
int rbg_ctx_rangebitmap_build_device(rbg_ctx* ctx, const uint64_t* values_dev, uint64_t n, uint64_t max_value,
                                     int max_from_data, int32_t* index);
/* Appender.serialize (:1483-1504) of a resident index, loaded or built: the header, maxKey masks of
 * (sliceCount + 7) >> 3 bytes, then [type][u16 size][payload] per container, a bitmap's size being its
 * cardinality as a Java char (65,536 written as 0, :1565).  For a loaded index: the bytes of the loaded stream
 * that map consumed; for a built one: the Appender's bytes.  The stream is written on the host from the index's
 * directory, masks and containers. */
int rbg_ctx_rangebitmap_serialize(rbg_ctx* ctx, int32_t index, rbg_buffer* out);

/* One-shot appender(max_value) / add / serialize (:52-56, :1511-1533, :1483-1504) on the GPU: open, build,
 * serialize, release.  out: the Appender's stream.  Without a usable device: RBG_ERR_DEVICE; the refusals that
 * need no device come first. */
int rbg_rangebitmap_build(const uint64_t* values, uint64_t n, uint64_t max_value, int max_from_data, rbg_buffer* out);
/* Host only, no device: map (:65-85) a stream, lay its containers out as a load does and write them back as
 * rbg_ctx_rangebitmap_serialize does (:1483-1504).  out: the bytes of buf that map consumed; the format errors
 * are rbg_rangebitmap_validate's. */
int rbg_rangebitmap_reserialize(const uint8_t* buf, size_t len, rbg_buffer* out);

#ifdef __cplusplus
}
#endif
#endif /* ROARING_MI355X_RANGEBITMAP_BUILD_H */
