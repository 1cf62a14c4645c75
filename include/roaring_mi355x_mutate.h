/*
 * roaring_mi355x_mutate.h — batches of values added to or removed from a bitmap: the C ABI of the point
 * mutations RoaringBitmap.add(int...) / addN / add(int) / remove(int) / checkedAdd / checkedRemove
 * (RB/RoaringBitmap.java:483, 498-570, 1162, 2637-2648, 1610, 1646).  Part of roaring_mi355x.h, which
 * includes it.
 *
 * One call is a batch of adds alone (op RBG_MUT_ADD) or of removes alone (op RBG_MUT_REMOVE): the result then
 * does not depend on the order of the values or on duplicates.  Per key the reference's container types hold,
 * byte for byte:
 *   - an array or bitmap container ends as the type its final cardinality gives, an array up to 4,096 values
 *     (RB/ArrayContainer.java:143-171, RB/BitmapContainer.java:1184-1202); 65,536 values stay a bitmap;
 *   - a run container stays a run container, whatever its run count (RunContainer.add / remove return this,
 *     RB/RunContainer.java:248-302, 2038-2070): 1 to 32,768 runs;
 *   - a new key is a fresh array container; a remove under an absent key does nothing;
 *   - an emptied container is dropped (RB/RoaringBitmap.java:2645-2647);
 *   - a key no value touches keeps its container, bytes and type.
 * *changed = the values actually added or removed, duplicates counted once: the sum of checkedAdd /
 * checkedRemove over the batch.  n == 0 leaves the bitmap as it is (addN, :498-570).
 *
 * Every refusal below is RBG_ERR_ILLEGAL_ARGUMENT with a text in rbg_last_error, decided before any device
 * work, and makes no batch: op not RBG_MUT_ADD or RBG_MUT_REMOVE; a null out_batch / out / changed; a null
 * values with n > 0; a batch that is packed, holds more than one bitmap or is bitmap-major.
 */
#ifndef ROARING_MI355X_MUTATE_H
#define ROARING_MI355X_MUTATE_H

#include "roaring_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RBG_MUT_ADD = 0, RBG_MUT_REMOVE = 1 };

/* x.add(values) (RB/RoaringBitmap.java:483; addN :498-570) or, value by value, x.remove(v) (:2637-2648) on a
 * resident bitmap, the single-bitmap key-major unpacked batch `batch`, as a new batch of the same shape:
 * *out_batch is what rbg_ctx_load of the reference's bitmap after the calls gives, usable wherever a loaded
 * bitmap is.  The operand stays as it is.  Only the keys the values touch are expanded (8 KiB each); every other
 * container is copied as it stands.  values is host memory, staged through the context's pinned buffer.
 * Synchronous (the key counts and the batch totals are read back). */
int rbg_ctx_mutate_values(rbg_ctx* ctx, int32_t batch, int op, const uint32_t* values, size_t n,
                          int32_t* out_batch, uint64_t* changed);
/* The same (add(int...) :483, addN :498-570; remove(int) :2637-2648) with values_dev (n uint32) in device
 * memory, read by kernels enqueued on the context stream: work that produces it on another stream must be
 * ordered before the call, and the buffer must not change until the call returns (it is read twice). */
int rbg_ctx_mutate_values_device(rbg_ctx* ctx, int32_t batch, int op, const void* values_dev, size_t n,
                                 int32_t* out_batch, uint64_t* changed);
/* The same in one call on the device over a serialized bitmap (addN :498-570, remove(int) :2637-2648; checkedAdd
 * :1610 / checkedRemove :1646 give *changed): *out = the serialized result, released with rbg_free. */
int rbg_mutate_values(const uint8_t* buf, size_t len, int op, const uint32_t* values, size_t n,
                      rbg_buffer* out, uint64_t* changed);
/* The same on the host, with no device: the rule above (addN :498-570, remove(int) :2637-2648) applied to the
 * serialized bytes.  A malformed or truncated bitmap gives rbg_inspect's status. */
int rbg_mutate_values_host(const uint8_t* buf, size_t len, int op, const uint32_t* values, size_t n,
                           rbg_buffer* out, uint64_t* changed);

#ifdef __cplusplus
}
#endif

#endif /* ROARING_MI355X_MUTATE_H */
