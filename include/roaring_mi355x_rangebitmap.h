/*
 * roaring_mi355x_rangebitmap.h — the range-encoded index: the C ABI of RangeBitmap
 * (RB/RangeBitmap.java; RB/ = RoaringBitmap/src/main/java/org/roaringbitmap/).  Part of roaring_mi355x.h,
 * which includes it.
 *
 * A RangeBitmap indexes one unsigned 64-bit value per row, rows 0 .. maxRid - 1, as up to 64 range-encoded
 * bit slices in its own serialized format (Appender.serialize, :1483-1504).  A serialized index is mapped
 * once (map, :65-85), kept resident, and every query form is answered on the GPU, one wave per block of
 * 65,536 rows, with the reference's bytes.  Values and thresholds are compared as UNSIGNED 64-bit numbers.
 *
 * Refusals are RBG_ERR_ILLEGAL_ARGUMENT, decided from the arguments before any device work: an unknown op, a
 * null output, and RBG_RB_BETWEEN with a context in a bitmap-returning call (the reference has no
 * between(min, max, context); only betweenCardinality takes one).
 */
#ifndef ROARING_MI355X_RANGEBITMAP_H
#define ROARING_MI355X_RANGEBITMAP_H

#include "roaring_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* op(a, b): b is read by RBG_RB_BETWEEN alone (a = min, b = max, both inclusive) */
enum {
  RBG_RB_LTE = 0,     /* lte :162-176, lteCardinality :184-198 */
  RBG_RB_LT = 1,      /* lt :206-220, ltCardinality :228-242: a == 0 is empty, else lte(a - 1) */
  RBG_RB_GT = 2,      /* gt :250-264, gtCardinality :272-286 */
  RBG_RB_GTE = 3,     /* gte :294-308, gteCardinality :316-330: a == 0 is every row / the context, else gt(a - 1) */
  RBG_RB_EQ = 4,      /* eq :338-351, eqCardinality :359-373 */
  RBG_RB_NEQ = 5,     /* neq :381-394, neqCardinality :402-416 */
  RBG_RB_BETWEEN = 6  /* between :111-119, betweenCardinality :128-154 */
};

/* RangeBitmap.map (:65-85) judged on the host alone, no device: RBG_OK, or RBG_ERR_INVALID_FORMAT (cookie,
 * base, a slice count outside 1..64, a container type byte, maxKey != ceil(maxRid / 65536)), or
 * RBG_ERR_TRUNCATED (the stream ends inside the header, the masks or a container record).  info (may be null):
 * {sliceCount, maxKey, maxRid, mask, container payload bytes, bytes consumed}. */
int rbg_rangebitmap_validate(const uint8_t* buf, size_t len, uint64_t* info);

/* RangeBitmap.map (:65-85): a serialized index from host memory, validated as above, its containers laid
 * out in device memory with a directory per (block, slice).  *index: a handle of this context (not a batch:
 * a slice may be a bitmap container of any cardinality, which no serialized bitmap can hold). */
int rbg_ctx_rangebitmap_load(rbg_ctx* ctx, const uint8_t* buf, size_t len, int32_t* index);
/* its device memory back; the handle is dead afterwards */
int rbg_ctx_rangebitmap_release(rbg_ctx* ctx, int32_t index);
/* info as rbg_rangebitmap_validate gives it (the last entry: 0) */
int rbg_ctx_rangebitmap_info(rbg_ctx* ctx, int32_t index, uint64_t* info);

/* lte / lt / gt / gte / eq / neq (:162-394) and between (:111-119), with context_batch >= 0 intersected with
 * bitmap context_i of that batch (a one-bitmap key-major batch, as the pairwise ops require; it is not
 * modified); context_batch < 0: no context.  *out_batch: a new one-bitmap batch that every call taking a
 * resident bitmap takes.  Per key the result is typed as the reference types it,
 * new BitmapContainer(bits, -1)[.iand(context container)].repairAfterLazy().runOptimize() (:443, :480-483), which
 * is runOptimize of an array or bitmap by cardinality; the shortcut results keep their own types: a threshold
 * above the index's mask gives RoaringBitmap.bitmapOfRange(0, maxRid) (run containers), a clone of the context
 * (its own containers, not run-optimised) or the empty bitmap (:427-429, :459-461, :552-554, :583-585).  The
 * two bitmapOfRange / clone shortcuts replace the context's pending result. */
int rbg_ctx_rangebitmap_query(rbg_ctx* ctx, int32_t index, int op, uint64_t a, uint64_t b, int32_t context_batch,
                              size_t context_i, int32_t* out_batch);
/* the *Cardinality forms (:128-154, :184-198, :228-242, :272-286, :316-330, :359-373, :402-416): the same
 * arguments, the count reduced on the device into one word; no container is written.  With a context
 * gtCardinality / gteCardinality count |context \ lte| per visited key as the reference does (countRange,
 * :659-661), which counts context rows at or past maxRid inside the last block.  betweenCardinality with a
 * context, where neither end leaves the mask, is DoubleEvaluation.count (:977-1014) as the reference has it: it
 * never advances its context position, so every block from the context's first key to its last is intersected
 * with the context's FIRST container.  An empty context gives 0 (that method throws on one). */
int rbg_ctx_rangebitmap_count(rbg_ctx* ctx, int32_t index, int op, uint64_t a, uint64_t b, int32_t context_batch,
                              size_t context_i, int64_t* out);

/* One-shot forms of the queries (:111-119, :162-394) and of their cardinalities (:128-154, :184-416): map the
 * serialized index, load the serialized context (context == NULL: none), query, fetch the serialized result /
 * the count, release.  Without a usable device: RBG_ERR_DEVICE; the refusals
 * and the index's format errors come first. */
int rbg_rangebitmap_query(const uint8_t* index, size_t index_len, int op, uint64_t a, uint64_t b,
                          const uint8_t* context, size_t context_len, rbg_buffer* out);
int rbg_rangebitmap_count(const uint8_t* index, size_t index_len, int op, uint64_t a, uint64_t b,
                          const uint8_t* context, size_t context_len, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ROARING_MI355X_RANGEBITMAP_H */
