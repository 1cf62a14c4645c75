// The exported C ABI of include/roaring_mi355x.h (engine.hpp: the host units), but the BSI entry points
// (engine_bsi.cpp), those of the range-encoded index (engine_rangebitmap.cpp), rbg_synth_key_bytes
// (engine_synth.cpp) and the accessors of the core's process-wide state (engine.cpp): argument checks, the one-shot fronts and the session calls over the units' ctx_* functions.
#include <algorithm>

#include "engine.hpp"
#include "format.hpp"

namespace rbg {

// the serialized empty bitmap (no run cookie, 0 containers)
static const uint8_t kEmpty[8] = {0x3A, 0x30, 0, 0, 0, 0, 0, 0};
static int emit_empty(rbg_buffer* out) { return emit_bytes(kEmpty, sizeof(kEmpty), out); }

static int ctx_batch_fetch(Ctx* c, int32_t batch, size_t i, rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_batch_fetch_range(c, batch, i, i + 1, out);
}

static bool point_op_ok(int op) { return op >= RBG_PQ_RANK && op <= RBG_PQ_PREV; }

// The one-shot front of an op over one serialized bitmap: the calling thread's context, the upload,
// op(c, id) on the bitmap's batch, the fetch of its result.  The entry point's argument checks come first.
template <class Op>
static int one_shot_unary(const uint8_t* a, size_t a_len, rbg_buffer* out, Op&& op) {
  OneShot os;
  CHK(os.open());
  int32_t id;
  CHK(os.load_separate(&a, &a_len, 1, &id));
  CHK(op(os.c, id));
  return ctx_fetch(os.c, out);
}

// the same over two: one upload for both operands, op(c, ida, idb)
template <class Op>
static int one_shot_binary(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, rbg_buffer* out, Op&& op) {
  OneShot os;
  CHK(os.open());
  const uint8_t* bufs[2] = {a, b};
  const size_t lens[2] = {a_len, b_len};
  int32_t ids[2];
  CHK(os.load_separate(bufs, lens, 2, ids));
  CHK(op(os.c, ids[0], ids[1]));
  return ctx_fetch(os.c, out);
}

}  // namespace rbg

using namespace rbg;

// entry of a session call: a null handle is an illegal argument; else the context, entered
// counts false: the entry of a pairwise op or a serialization, which may go to set 1's stream (Ctx::seq)
int rbg::session(rbg_ctx* ctx, Ctx** c, bool counts) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  *c = &ctx->c;
  return enter(*c, counts);
}

extern "C" {

int rbg_version(void) { return 1; }

int rbg_pairwise(int op, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, rbg_buffer* out) {
  if (!out || op < 0 || op > RBG_ANDNOT_BUFFER) return RBG_ERR_ILLEGAL_ARGUMENT;
  return one_shot_binary(a, a_len, b, b_len, out, [&](Ctx* c, int32_t ia, int32_t ib) {
    return ctx_pairwise(c, op, ia, 0, ib, 0, false);
  });
}

int rbg_pairwise_inplace(int op, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, int same_object,
                         rbg_buffer* out) {
  if (!out || op < 0 || op > 3) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (same_object) {
    // x1.and(x1) / x1.or(x1) return at once (x1 unchanged); x1.xor(x1) / x1.andNot(x1) clear it
    // (RB/RoaringBitmap.java:1271, 2482, 3297-3300, 1347-1350)
    if (op == RBG_XOR || op == RBG_ANDNOT) return emit_empty(out);
    // x1 unchanged: validated on the host like any input, then its own bytes back (no device call)
    HostBitmap hb;
    std::string err;
    const int st = parse(a, a_len, &hb, &err);
    if (st) {
      set_err(err);
      return st;
    }
    uint8_t* p = out_alloc(hb.consumed);
    if (!p) return RBG_ERR_OUT_OF_MEMORY;
    std::memcpy(p, a, hb.consumed);
    out->data = p;
    out->len = hb.consumed;
    return RBG_OK;
  }
  // x1.and / xor / andNot(x2) in place type like the static ops (Container.iand / ixor / iandNot
  // end in the same container types); x1.or(x2) is Container.ior's
  return rbg_pairwise(op == RBG_OR ? RBG_OR_INPLACE : op, a, a_len, b, b_len, out);
}

int rbg_ornot(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, int64_t range_end, int flags,
              rbg_buffer* out) {
  if (!out || flags < 0 || flags > 3) return RBG_ERR_ILLEGAL_ARGUMENT;
  return one_shot_binary(a, a_len, b, b_len, out, [&](Ctx* c, int32_t ia, int32_t ib) {
    return ctx_ornot(c, ia, 0, ib, 0, range_end, flags);
  });
}

int rbg_ctx_ornot(rbg_ctx* ctx, int32_t a, size_t ia, int32_t b, size_t ib, int64_t range_end, int flags) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (flags < 0 || flags > 3) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_ornot(c, a, ia, b, ib, range_end, flags);
}

int rbg_range_mut(int op, const uint8_t* a, size_t a_len, int64_t range_start, int64_t range_end, rbg_buffer* out) {
  if (!out || op < 0 || op > (RBG_RMUT_ADD_INPLACE | RBG_RMUT_BUFFER))
    return RBG_ERR_ILLEGAL_ARGUMENT;
  return one_shot_unary(a, a_len, out, [&](Ctx* c, int32_t id) {
    return ctx_range_mut(c, op & 3, id, 0, range_start, range_end, (op & RBG_RMUT_BUFFER) != 0);
  });
}

int rbg_ctx_range_mut(rbg_ctx* ctx, int op, int32_t batch, size_t i, int64_t range_start, int64_t range_end) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (op < 0 || op > (RBG_RMUT_ADD_INPLACE | RBG_RMUT_BUFFER)) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_range_mut(c, op & 3, batch, i, range_start, range_end, (op & RBG_RMUT_BUFFER) != 0);
}

int rbg_add_offset(const uint8_t* a, size_t a_len, int64_t offset, rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  return one_shot_unary(a, a_len, out, [&](Ctx* c, int32_t id) { return ctx_add_offset(c, id, 0, offset); });
}

/* ---- point queries (rankdir.hip) ---- */

int rbg_ctx_point_query(rbg_ctx* ctx, int op, int32_t batch, size_t i, const uint32_t* q, size_t n, int64_t* out) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!point_op_ok(op)) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (n == 0) return RBG_OK;
  if (!q || !out) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_point_host(c, op, batch, i, q, n, out);
}

int rbg_ctx_point_query_device(rbg_ctx* ctx, int op, int32_t batch, size_t i, const void* q_dev, size_t n,
                               void* out_dev) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!point_op_ok(op)) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (n == 0) return RBG_OK;
  if (!q_dev || !out_dev) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_point(c, op, batch, i, reinterpret_cast<const uint32_t*>(q_dev), n,
                   reinterpret_cast<long long*>(out_dev));
}

int rbg_point_query(int op, const uint8_t* buf, size_t len, const uint32_t* q, size_t n, int64_t* out) {
  if (!point_op_ok(op)) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (n == 0) return RBG_OK;
  if (!buf || !q || !out) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(os.load_separate(&buf, &len, 1, &id));
  return ctx_point_host(c, op, id, 0, q, n, out);
}

int rbg_ctx_from_values(rbg_ctx* ctx, const uint32_t* values, size_t n, int run_optimize, int32_t* batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!batch || (n && !values)) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_from_values_host(c, values, n, run_optimize != 0, batch);
}

int rbg_ctx_from_values_device(rbg_ctx* ctx, const void* values_dev, size_t n, int run_optimize, int32_t* batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!batch || (n && !values_dev)) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_from_values(c, reinterpret_cast<const uint32_t*>(values_dev), n, run_optimize != 0, batch);
}

int rbg_ctx_to_values(rbg_ctx* ctx, int32_t batch, size_t i, uint64_t first, uint64_t count, uint32_t* out,
                      uint64_t* n_out) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_to_values_host(c, batch, i, first, count, out, n_out);
}

int rbg_ctx_to_values_device(rbg_ctx* ctx, int32_t batch, size_t i, uint64_t first, uint64_t count, int out64,
                             void* out_dev, uint64_t* n_out) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_to_values(c, batch, i, first, count, out64 != 0, out_dev, n_out);
}

int rbg_build_values(const uint32_t* values, size_t n, int run_optimize, rbg_buffer* out) {
  if (!out || (n && !values)) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(ctx_from_values_host(c, values, n, run_optimize != 0, &id));
  os.adopt(id);
  return ctx_batch_fetch(c, id, 0, out);
}

int rbg_expand_values(const uint8_t* buf, size_t len, rbg_buffer* out) {
  if (!out || (!buf && len)) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(os.load_separate(&buf, &len, 1, &id));
  const uint64_t card = (uint64_t)c->batches[id]->long_card;
  uint8_t* p = (uint8_t*)std::malloc(card * 4 + 4);
  if (!p) return RBG_ERR_OUT_OF_MEMORY;
  uint64_t got = 0;
  const int st = ctx_to_values_host(c, id, 0, 0, card, reinterpret_cast<uint32_t*>(p), &got);
  if (st != RBG_OK) {
    std::free(p);
    return st;
  }
  out->data = p;
  out->len = (size_t)got * 4;
  return RBG_OK;
}

/* ---- dense bitsets (bitset.hip): BitSetUtil.  The argument checks come before the session is entered, so a
 * refusal needs no device. ---- */

int rbg_ctx_from_bitset(rbg_ctx* ctx, const void* bits, uint64_t n, int layout, int run_optimize, int32_t* batch) {
  CHK(check_bitset_build(bits, n, layout, false));
  Ctx* c;
  CHK(session(ctx, &c));
  if (!batch) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_from_bitset_host(c, bits, n, layout, run_optimize != 0, batch);
}

int rbg_ctx_from_bitset_device(rbg_ctx* ctx, const void* bits_dev, uint64_t n, int layout, int run_optimize,
                               int32_t* batch) {
  CHK(check_bitset_build(bits_dev, n, layout, true));
  Ctx* c;
  CHK(session(ctx, &c));
  if (!batch) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_from_bitset(c, bits_dev, n, layout, run_optimize != 0, batch);
}

int rbg_ctx_to_bitset(rbg_ctx* ctx, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout, void* out) {
  CHK(check_bitset_window(first, n, layout));
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_to_bitset_host(c, batch, i, first, n, layout, out);
}

int rbg_ctx_to_bitset_device(rbg_ctx* ctx, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout,
                             void* out_dev) {
  CHK(check_bitset_window(first, n, layout));
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_to_bitset(c, batch, i, first, n, layout, out_dev);
}

int rbg_bitset_build(const void* bits, uint64_t n, int layout, int run_optimize, rbg_buffer* out) {
  CHK(check_bitset_build(bits, n, layout, false));
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(ctx_from_bitset_host(c, bits, n, layout, run_optimize != 0, &id));
  os.adopt(id);
  return ctx_batch_fetch(c, id, 0, out);
}

// toLongArray's length (RB/BitSetUtil.java:76-79): lastBit = max(last, 64), rounded down to a multiple of 64
static uint64_t words_in_use(uint64_t last) { return std::max<uint64_t>(last, 64) / 64 + 1; }

int rbg_bitset_expand(const uint8_t* buf, size_t len, rbg_buffer* out) {
  if (!out || (!buf && len)) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(os.load_separate(&buf, &len, 1, &id));
  if (c->batches[id]->long_card == 0) return emit_bytes(nullptr, 0, out);  // new long[0] (:68-70)
  const uint32_t q = 0xFFFFFFFFu;
  int64_t last = -1;
  CHK(ctx_point_host(c, PT_PREV, id, 0, &q, 1, &last));  // bitmap.last()
  if (last >= (int64_t)1 << 31) {
    set_err("bitmap has negative bits set");  // :72-75
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const uint64_t nw = words_in_use((uint64_t)last);
  uint8_t* p = (uint8_t*)std::malloc(8 * nw);
  if (!p) return RBG_ERR_OUT_OF_MEMORY;
  const int st = ctx_to_bitset_host(c, id, 0, 0, 64 * nw, RBG_BITS_PACKED, p);
  if (st != RBG_OK) {
    std::free(p);
    return st;
  }
  out->data = p;
  out->len = (size_t)(8 * nw);
  return RBG_OK;
}

// x.limit(maxcardinality) (RB/RoaringBitmap.java:2457-2476).  The cut is planned from the serialized
// header's cardinalities on the host (the reference's own loop walks getCardinality per container);
// ctx_limit cuts on the device.
int rbg_limit(const uint8_t* a, size_t a_len, int32_t maxcard, rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  HostBitmap hb;
  std::string err;
  const int pst = parse(a, a_len, &hb, &err);
  if (pst) {
    set_err(err);
    return pst;
  }
  int cut_key = 65536, leftover = 0;
  int64_t cur = 0;
  for (size_t i = 0; cur < maxcard && i < hb.ctrs.size(); i++) {
    const int64_t cc = hb.ctrs[i].card;
    if (cc + cur <= maxcard) {
      cur += cc;
    } else {
      cut_key = hb.ctrs[i].key;
      leftover = (int)(maxcard - cur);
      break;
    }
  }
  if (leftover == 0) {  // the containers that fit whole: those before the first that does not
    cut_key = 0;
    for (size_t i = 0, acc = 0; i < hb.ctrs.size() && (int64_t)(acc + hb.ctrs[i].card) <= (int64_t)maxcard; i++) {
      acc += hb.ctrs[i].card;
      cut_key = hb.ctrs[i].key + 1;
    }
  }
  return one_shot_unary(a, a_len, out, [&](Ctx* c, int32_t id) { return ctx_limit(c, id, 0, cut_key, leftover); });
}

// RoaringBitmap.bitmapOfRange(min, max) (RB/RoaringBitmap.java:588-615): k_rmut<RMUT_RANGE> over an empty
// bitmap (every container written as a run container)
int rbg_bitmap_of_range(int64_t min, int64_t max, rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  return one_shot_unary(kEmpty, sizeof(kEmpty), out, [&](Ctx* c, int32_t id) {
    return ctx_range_mut(c, RMUT_RANGE, id, 0, min, max, false);
  });
}

int rbg_remove_run_compression(const uint8_t* a, size_t a_len, rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  return one_shot_unary(a, a_len, out, [&](Ctx* c, int32_t id) { return ctx_remove_run_compression(c, id, 0); });
}

int rbg_ctx_add_offset(rbg_ctx* ctx, int32_t batch, size_t i, int64_t offset) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_add_offset(c, batch, i, offset);
}

int rbg_pairwise_card(int op, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, int32_t* out) {
  if (!out || op < 0 || op > RBG_CONTAINS) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t ia, ib;
  CHK(os.load(&a, &a_len, 1, &ia));
  CHK(os.load(&b, &b_len, 1, &ib));
  CHK(ctx_pairwise(c, OP_AND, ia, 0, ib, 0, true));
  ResultInfo ri;
  CHK(ctx_info(c, &ri));
  const uint32_t ac = ri.card32;
  const uint32_t ca = (uint32_t)(uint64_t)c->batches[ia]->long_card;  // RoaringBitmap.getCardinality (int)
  const uint32_t cb = (uint32_t)(uint64_t)c->batches[ib]->long_card;
  switch (op) {
    case RBG_CARD_AND: *out = (int32_t)ac; break;
    case RBG_CARD_OR: *out = (int32_t)(ca + cb - ac); break;         // RB/RoaringBitmap.java:916-920
    case RBG_CARD_XOR: *out = (int32_t)(ca + cb - 2u * ac); break;   // :931-933
    case RBG_CARD_ANDNOT: *out = (int32_t)(ca - ac); break;          // :944-985 (both branches, mod 2^32)
    case RBG_CONTAINS:  // b is a subset of a (:2781-2802): every value of b in a AND b, counted in 64 bits
      *out = ri.long_card == c->batches[ib]->long_card ? 1 : 0;
      break;
    default: *out = ri.any ? 1 : 0; break;                           // intersects :698-720
  }
  return RBG_OK;
}

int rbg_wide(int op, const uint8_t* const* bufs, const size_t* lens, const int32_t* ids, size_t n, rbg_buffer* out) {
  if (!out || op < 0 || op > RBG_WIDE_BUFFER_AND_ITER) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(os.load(bufs, lens, n, &id, wide_reads_packed(op, n)));
  CHK(ctx_wide(c, op, id, 0, 65536, ids, false, nullptr, nullptr));
  return ctx_fetch(c, out);
}

int rbg_range_op(int op, const uint8_t* const* bufs, const size_t* lens, size_t n, int64_t range_start,
                 int64_t range_end, rbg_buffer* out) {
  if (!out || op < RBG_RANGE_AND || op > RBG_RANGE_BUFFER_ANDNOT ||
      ((op == RBG_RANGE_ANDNOT || op == RBG_RANGE_BUFFER_ANDNOT) && n != 2))
    return RBG_ERR_ILLEGAL_ARGUMENT;
  const bool buf = op >= RBG_RANGE_BUFFER_AND;
  const int base = buf ? op - RBG_RANGE_BUFFER_AND : op;
  if (buf && base == RBG_RANGE_AND && n == 0) {
    // BufferFastAggregation.and(long[], Iterator) with no input: an empty bitmap (:81-88)
    CHK(check_range(range_start, range_end));
    return emit_empty(out);
  }
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  CHK(check_range(range_start, range_end));  // rangeSanityCheck before the selections (RB/RoaringBitmap.java:204-213)
  if (base == RBG_RANGE_ANDNOT) {  // andNot(x1, x2, start, end): both operands selected, then andNot
    int32_t ids[2], sel[2];
    CHK(os.load_separate(bufs, lens, 2, ids));
    for (int i = 0; i < 2; i++) {
      CHK(ctx_select_range(c, ids[i], range_start, range_end, &sel[i], buf));
      os.adopt(sel[i]);
    }
    // the buffer package's andNot keeps R \ R's merged run container (ImmutableRoaringBitmap.andNot)
    CHK(ctx_pairwise(c, buf ? RBG_ANDNOT_BUFFER : OP_ANDNOT, sel[0], 0, sel[1], 0, false));
    return ctx_fetch(c, out);
  }
  int32_t id, sel;
  CHK(os.load(bufs, lens, n, &id));
  CHK(ctx_select_range(c, id, range_start, range_end, &sel, buf));
  os.adopt(sel);
  // heap: and -> FastAggregation.and(Iterator) = naive_and(Iterator); or / xor -> naive_or / naive_xor.
  // buffer: and -> BufferFastAggregation.and(Iterator) = workShyAnd for any count (no input: empty);
  // or / xor -> naive_or / naive_xor, typed like the heap's
  const int wop = base == RBG_RANGE_AND ? (buf ? RBG_WIDE_WORKSHY_AND : RBG_WIDE_AND_ITER)
                  : base == RBG_RANGE_OR ? RBG_WIDE_OR
                                         : RBG_WIDE_XOR;
  CHK(ctx_wide(c, wop, sel, 0, 65536, nullptr, false, nullptr, nullptr));
  return ctx_fetch(c, out);
}

int rbg_select_range(const uint8_t* a, size_t a_len, int64_t range_start, int64_t range_end, int buffer,
                     rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id, sel;
  CHK(os.load_separate(&a, &a_len, 1, &id));
  CHK(ctx_select_range(c, id, range_start, range_end, &sel, buffer != 0));
  os.adopt(sel);
  return ctx_batch_fetch(c, sel, 0, out);
}

int rbg_ctx_select_range(rbg_ctx* ctx, int32_t batch, int64_t range_start, int64_t range_end, int32_t* out_batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_batch) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_select_range(c, batch, range_start, range_end, out_batch);
}

int rbg_wide_card(int op, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* out) {
  if (!out || op < 0 || op > 1) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(os.load(bufs, lens, n, &id));
  int hc = 0;
  bool hv = false;
  CHK(ctx_wide(c, op, id, 0, 65536, nullptr, true, &hc, &hv));
  if (hv) {
    *out = hc;
    return RBG_OK;
  }
  ResultInfo ri;
  CHK(ctx_info(c, &ri));
  *out = (int32_t)ri.card32;
  return RBG_OK;
}

int rbg_batch_and_card(size_t n_pairs, const uint8_t* const* a_bufs, const size_t* a_lens,
                       const uint8_t* const* b_bufs, const size_t* b_lens, int32_t* out) {
  if (n_pairs && (!a_bufs || !a_lens || !b_bufs || !b_lens || !out)) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (n_pairs == 0) return RBG_OK;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  std::vector<const uint8_t*> bufs(2 * n_pairs);
  std::vector<size_t> lens(2 * n_pairs);
  for (size_t i = 0; i < n_pairs; i++) {
    bufs[2 * i] = a_bufs[i];
    lens[2 * i] = a_lens[i];
    bufs[2 * i + 1] = b_bufs[i];
    lens[2 * i + 1] = b_lens[i];
  }
  int32_t id;  // bitmap-major: the pairs stay adjacent
  CHK(os.load(bufs.data(), lens.data(), 2 * n_pairs, &id, false, false));
  CHK(ctx_batch_card(c, id));
  HIPCHK(hipMemcpyAsync(out, c->cards.p, 4 * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return RBG_OK;
}

// ---- host-side format utilities ----

int rbg_from_values(const uint32_t* values, size_t n, int run_optimize, rbg_buffer* out) {
  if (!out || (n && !values)) return RBG_ERR_ILLEGAL_ARGUMENT;
  return emit_host(build_from_values(values, n, run_optimize != 0), out);
}

// RoaringBitmap.runOptimize() (RB/RoaringBitmap.java:2764-2774): the device pass
// (runopt.hip) over a one-bitmap batch, like rbg_run_optimize_many.
int rbg_run_optimize(const uint8_t* buf, size_t len, rbg_buffer* out) {
  if (!out || (!buf && len)) return RBG_ERR_ILLEGAL_ARGUMENT;
  uint8_t answer = 0;
  return rbg_run_optimize_many(&buf, &len, 1, out, &answer);
}

int rbg_to_values(const uint8_t* buf, size_t len, rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  std::vector<uint32_t> v;
  std::string err;
  int st = values_of_serialized(buf, len, &v, &err);
  if (st) {
    set_err(err);
    return st;
  }
  return emit_bytes(reinterpret_cast<const uint8_t*>(v.data()), v.size() * 4, out);
}

int rbg_inspect(const uint8_t* buf, size_t len, size_t* consumed, int64_t* cardinality, int64_t* stats3) {
  HostBitmap hb;
  std::string err;
  int st = parse(buf, len, &hb, &err);
  if (st) {
    set_err(err);
    return st;
  }
  if (consumed) *consumed = hb.consumed;
  if (cardinality) *cardinality = hb.card;
  if (stats3) {
    stats3[0] = stats3[1] = stats3[2] = 0;
    for (const HostCtr& c : hb.ctrs) stats3[c.kind]++;
  }
  return RBG_OK;
}

// ---- session API ----
int rbg_ctx_create(int device, rbg_ctx** out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  std::unique_ptr<rbg_ctx> c(new rbg_ctx());
  CHK(ctx_init(&c->c, device));
  *out = c.release();
  return RBG_OK;
}
void rbg_ctx_destroy(rbg_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->c.device);
  delete ctx;
}
void* rbg_ctx_stream(rbg_ctx* ctx) { return ctx ? (void*)ctx->c.stream : nullptr; }
int rbg_ctx_profile(rbg_ctx* ctx, int max_ops) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_profile(c, max_ops, false);
}
int rbg_ctx_profile_compute(rbg_ctx* ctx, int max_ops) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_profile(c, max_ops, true);
}
int rbg_ctx_profile_bytes(rbg_ctx* ctx, int64_t* bytes) {
  if (!ctx || !bytes) {
    set_err("profile_bytes: null argument");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  Ctx* c;
  CHK(session(ctx, &c));
  CHK(sync_streams(c));
  unsigned long long v = 0;
  if (c->rd_ctr.p) HIPCHK(hipMemcpy(&v, c->rd_ctr.p, 8, hipMemcpyDeviceToHost));
  *bytes = (int64_t)v;
  return RBG_OK;
}
int rbg_ctx_profile_read(rbg_ctx* ctx, double* ms3, int* n_ops) {
  Ctx* c;
  CHK(session(ctx, &c));
  CHK(sync_streams(c));
  ms3[0] = ms3[1] = ms3[2] = 0.0;
  for (size_t i = 0; i < c->prof_n; i++) {
    for (int ph = 0; ph < 3; ph++) {
      if (c->prof_compute_only && ph != 1) continue;  // only the compute launch was bracketed
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[4 * i + ph], c->prof_ev[4 * i + ph + 1]));
      ms3[ph] += ms;
    }
  }
  *n_ops = (int)c->prof_n;
  c->prof_n = 0;
  return RBG_OK;
}
int rbg_ctx_sync(rbg_ctx* ctx) {
  Ctx* c;
  CHK(session(ctx, &c));
  return sync_streams(c);
}
int rbg_ctx_load_separate(rbg_ctx* ctx, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* ids) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!ids) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_load_separate(c, bufs, lens, n, ids);
}
int rbg_ctx_load(rbg_ctx* ctx, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_load(c, bufs, lens, n, batch);
}
int rbg_ctx_load_packed(rbg_ctx* ctx, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!batch) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_load(c, bufs, lens, n, batch, true);
}
int rbg_ctx_release(rbg_ctx* ctx, int32_t batch) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  Ctx& c = ctx->c;
  Batch* b;
  CHK(find_batch(&c, batch, &b));  // no statistics read-back for a batch that goes
  CHK(enter(&c));
  // A materialised result references pass-through containers inside its operand
  // batches (ORec::src) until it is serialized: serialize it before an operand goes.
  if (c.r().last == 1 && !c.r().serialized &&
      std::find(c.r().pending_src.begin(), c.r().pending_src.end(), batch) != c.r().pending_src.end())
    CHK(ctx_serialize(&c, true));  // on the context's stream: in front of whatever reuses the buffers
  // No host sync: the buffers go to this context's pool, and whatever reuses them is enqueued on
  // the context's stream after every launch that reads them -- an op or a serialization on set 1's
  // stream may be one, so the context's stream waits for that stream first (join_all); a pooled buffer
  // that is freed goes through hipFree, which waits for the device.
  CHK(join_all(&c));
  for (DevBuf* d : {&b->keys, &b->desc, &b->bm, &b->key_off, &b->bm_off, &b->payload, &b->ro_stats,
                    &b->bsi_tasks, &b->bsi_nt, &b->bsi_table, &b->rd_cum, &b->rd_off, &b->rd_aux})
    pool_put(&c, *d);
  c.batches[batch].reset();
  return RBG_OK;
}
int rbg_ctx_batch_stats(rbg_ctx* ctx, int32_t batch, int64_t* st) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  Batch* b;
  CHK(get_batch(&ctx->c, batch, &b));
  st[0] = (int64_t)b->n_bm;
  st[1] = (int64_t)b->n_ctr;
  st[2] = b->n_kind[0];
  st[3] = b->n_kind[1];
  st[4] = b->n_kind[2];
  st[5] = 0;  // payload bytes (serialized form)
  st[6] = b->long_card;
  st[7] = b->ser_bytes;
  if (b->n_ctr) {
    CHK(enter(&ctx->c));
    hipStream_t s = ctx->c.stream;
    HIPCHK(hipMemsetAsync(ctx->c.scalar.p, 0, 8, s));
    launch_batch_bytes(s, b->desc.as<CDesc>(), b->n_ctr, b->payload.as<uint8_t>(),
                       ctx->c.scalar.as<unsigned long long>());
    unsigned long long pay = 0;
    HIPCHK(hipMemcpyAsync(&pay, ctx->c.scalar.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    st[5] = (int64_t)pay;
  }
  return RBG_OK;
}
int rbg_ctx_batch_fetch(rbg_ctx* ctx, int32_t batch, size_t i, rbg_buffer* out) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_batch_fetch(c, batch, i, out);
}
int rbg_ctx_batch_fetch_range(rbg_ctx* ctx, int32_t batch, size_t first, size_t count, rbg_buffer* outs) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_batch_fetch_range(c, batch, first, first + count, outs);
}
int rbg_ctx_pairwise(rbg_ctx* ctx, int op, int32_t a, size_t ia, int32_t b, size_t ib) {
  Ctx* c;
  CHK(session(ctx, &c, false));
  return ctx_pairwise(c, op, a, ia, b, ib, false);
}
int rbg_ctx_pairwise_serialized(rbg_ctx* ctx, int op, int32_t a, size_t ia, int32_t b, size_t ib) {
  Ctx* c;
  CHK(session(ctx, &c, false));
  if (op < 0 || op > 3) return RBG_ERR_ILLEGAL_ARGUMENT;
  CHK(ctx_pairwise(c, op, a, ia, b, ib, false));
  return ctx_serialize(c);
}
int rbg_ctx_pairwise_range(rbg_ctx* ctx, int op, int32_t a, size_t ia, int32_t b, size_t ib, int key_lo, int key_hi) {
  Ctx* c;
  CHK(session(ctx, &c, false));
  if (key_lo > key_hi) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_pairwise(c, op, a, ia, b, ib, false, key_lo, key_hi);
}
int rbg_ctx_pairwise_card(rbg_ctx* ctx, int op, int32_t a, size_t ia, int32_t b, size_t ib) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (op != RBG_CARD_AND) {
    set_err("the session API computes andCardinality; derive the others from the input cardinalities");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return ctx_pairwise(c, OP_AND, a, ia, b, ib, true);
}
int rbg_ctx_wide(rbg_ctx* ctx, int op, int32_t batch, int key_lo, int key_hi, const int32_t* ids) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_wide(c, op, batch, key_lo, key_hi, ids, false, nullptr, nullptr);
}
int rbg_ctx_wide_start(rbg_ctx* ctx, int op, int32_t batch, int key_lo, int key_hi, const int32_t* ids,
                       int32_t start_bm) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_wide(c, op, batch, key_lo, key_hi, ids, false, nullptr, nullptr, start_bm);
}
int rbg_ctx_batch_counts(rbg_ctx* ctx, int32_t batch, uint32_t* out, size_t n) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  Batch* b;
  CHK(get_batch(&ctx->c, batch, &b));
  if (!out || n != b->n_bm) return RBG_ERR_ILLEGAL_ARGUMENT;
  for (size_t i = 0; i < n; i++) out[i] = b->h_bm_nctr[i];
  return RBG_OK;
}
int rbg_ctx_pair_bytes(rbg_ctx* ctx, int32_t batch, int64_t* out2) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  Batch* b;
  CHK(get_batch(&ctx->c, batch, &b));
  if (!out2 || b->key_major || b->n_bm % 2) {
    set_err("needs a bitmap-major batch of pairs");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(enter(&ctx->c));
  HIPCHK(hipStreamSynchronize(ctx->c.stream));
  std::vector<CDesc> d(b->n_ctr);
  if (b->n_ctr) HIPCHK(hipMemcpy(d.data(), b->desc.p, sizeof(CDesc) * b->n_ctr, hipMemcpyDeviceToHost));
  auto pay = [](const CDesc& x) -> int64_t { return x.kind == KA ? 2 * (int64_t)x.card : x.kind == KB ? 8192 : 0; };
  int64_t matched = 0, all = 0;
  for (size_t p = 0; p < b->n_bm / 2; p++) {
    uint32_t i = b->h_bm_off[2 * p], ie = b->h_bm_off[2 * p + 1], j = ie, je = b->h_bm_off[2 * p + 2];
    all += 4 * (int64_t)(je - i);
    while (i < ie && j < je) {
      if (d[i].key == d[j].key) {
        matched += pay(d[i++]) + pay(d[j++]);
      } else if (d[i].key < d[j].key) {
        i++;
      } else {
        j++;
      }
    }
  }
  out2[0] = matched + all;  // matched payload + descriptors
  int64_t tot = 0;
  for (const CDesc& x : d) tot += pay(x) + 4;
  out2[1] = tot;  // every payload + descriptors
  return RBG_OK;
}
int rbg_ctx_wide_card(rbg_ctx* ctx, int op, int32_t batch, int key_lo, int key_hi) {
  Ctx* c;
  CHK(session(ctx, &c));
  int hc;
  bool hv;
  CHK(ctx_wide(c, op, batch, key_lo, key_hi, nullptr, true, &hc, &hv));
  if (hv) {
    ResultInfo ri = {};
    ri.card32 = (uint32_t)hc;
    ri.long_card = hc;
    HIPCHK(hipMemcpyAsync(c->r().info.p, &ri, sizeof(ri), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return RBG_OK;
}
int rbg_ctx_batch_and_card(rbg_ctx* ctx, int32_t batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_batch_card(c, batch);
}
int rbg_ctx_card(rbg_ctx* ctx, int32_t* out) {
  Ctx* c;
  CHK(session(ctx, &c));
  ResultInfo ri;
  CHK(ctx_info(c, &ri));
  *out = (int32_t)ri.card32;
  return RBG_OK;
}
int rbg_ctx_cards(rbg_ctx* ctx, int32_t* out, size_t n) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (n > c->n_cards) return RBG_ERR_ILLEGAL_ARGUMENT;
  HIPCHK(hipMemcpyAsync(out, c->cards.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return RBG_OK;
}
int rbg_ctx_result_stats(rbg_ctx* ctx, int64_t* st) {
  Ctx* c;
  CHK(session(ctx, &c));
  ResultInfo ri;
  CHK(ctx_info(c, &ri));
  st[0] = ri.n_out;
  st[1] = (int64_t)ri.payload;
  st[2] = ri.has_run;
  st[3] = ri.long_card;
  return RBG_OK;
}
int rbg_ctx_serialize(rbg_ctx* ctx) {
  Ctx* c;
  CHK(session(ctx, &c, false));
  return ctx_serialize(c);
}
int rbg_ctx_fetch(rbg_ctx* ctx, rbg_buffer* out) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_fetch(c, out);
}
int rbg_ctx_result_layout_device(rbg_ctx* ctx, void* dst3) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!dst3) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (c->r().last != 1) {
    set_err("no materialised result pending");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(join_result(c));
  if (c->r().place_pending) {  // the placement writes the layout too (one launch fewer per sharded step)
    OutCtx o = c->r().pending;
    o.layout_out = reinterpret_cast<int64_t*>(dst3);
    launch_place(c->stream, c->r().ntasks.as<uint32_t>(), o, c->r().info.as<ResultInfo>());
    c->r().place_pending = false;
  } else {
    launch_layout_out(c->stream, c->r().info.as<ResultInfo>(), reinterpret_cast<int64_t*>(dst3));
  }
  HIPCHK(hipGetLastError());
  return RBG_OK;
}
int rbg_ctx_fetch_shard_device_dyn(rbg_ctx* ctx, const void* layout, int rank, int world, void* out, void* runb) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!layout || !out || world < 1 || world > 1024 || rank < 0 || rank >= world)
    return RBG_ERR_ILLEGAL_ARGUMENT;
  if (c->r().last != 1) {
    set_err("no materialised result pending");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(join_result(c));
  CHK(ensure_placed(c));
  // an already serialized result's pass-through records may point into released operands: copy its
  // payload region instead (like rbg_ctx_fetch_shard_device); not expected on the sharded path
  if (c->r().serialized) {
    set_err("fetch_shard_device_dyn: the result was already serialized; fetch it before releasing operands "
            "or use rbg_ctx_fetch_shard_device");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  launch_serialize_shard_dyn(c->stream, grid_for((c->r().pending_ub + 255) / 256, 256), c->r().ntasks.as<uint32_t>(), c->r().pending,
                             reinterpret_cast<const int64_t*>(layout), rank, world, (uint8_t*)out, (uint8_t*)runb, true);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}
int rbg_ctx_fetch_shard_device(rbg_ctx* ctx, int64_t total_containers, int has_run, int64_t payload_base,
                               void* desc_dst, void* offsets_dst, void* runflag_dst, void* payload_dst) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_fetch_shard_device(c, total_containers, has_run, payload_base, desc_dst, offsets_dst, runflag_dst,
                                payload_dst);
}

int rbg_ctx_fetch_shard(rbg_ctx* ctx, int64_t total_containers, int has_run, int64_t first_container,
                        int64_t payload_base, rbg_buffer* out_desc, rbg_buffer* out_offsets, rbg_buffer* out_payload) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_desc || !out_offsets || !out_payload) return RBG_ERR_ILLEGAL_ARGUMENT;
  (void)first_container;  // the shard's own buffers start at its first container
  ResultInfo ri;
  CHK(ctx_info(c, &ri));
  const size_t n = ri.n_out;
  const bool offsets = !has_run || total_containers >= 4;
  DevBuf d;
  CHK(d.ensure(9 * n + ri.payload + 64));
  uint8_t* base = d.as<uint8_t>();
  CHK(ctx_fetch_shard_device(c, total_containers, has_run, payload_base, base, base + 4 * n, base + 8 * n,
                             base + 9 * n));
  std::vector<uint8_t> h(9 * n + ri.payload);
  if (!h.empty()) HIPCHK(hipMemcpyAsync(h.data(), base, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  CHK(emit_bytes(h.data(), 4 * n, out_desc));
  CHK(emit_bytes(h.data() + 4 * n, offsets ? 4 * n : 0, out_offsets));
  return emit_bytes(h.data() + 9 * n, ri.payload, out_payload);
}

int rbg_run_optimize_many(const uint8_t* const* bufs, const size_t* lens, size_t n, rbg_buffer* outs,
                          uint8_t* answers) {
  if (n && !outs) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t in = -1, opt = -1;
  CHK(os.load(bufs, lens, n, &in));
  CHK(ctx_run_optimize(c, in, &opt, answers));
  os.adopt(opt);
  for (size_t i = 0; i < n; i++) {
    outs[i] = rbg_buffer{};
    const int st = ctx_batch_fetch(c, opt, i, &outs[i]);
    if (st) {
      for (size_t j = 0; j < i; j++) rbg_free(&outs[j]);
      return st;
    }
  }
  return RBG_OK;
}

int rbg_ctx_run_optimize(rbg_ctx* ctx, int32_t batch, int32_t* out_batch, uint8_t* answers) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_batch) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_run_optimize(c, batch, out_batch, answers);
}

int rbg_ctx_batch_minmax(rbg_ctx* ctx, int32_t batch, int32_t* out2) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  Batch* b;
  CHK(get_batch(&ctx->c, batch, &b));
  if (!out2) return RBG_ERR_ILLEGAL_ARGUMENT;
  out2[0] = b->bsi_min;
  out2[1] = b->bsi_max;
  return RBG_OK;
}

int rbg_ctx_synth(rbg_ctx* ctx, int kind, uint64_t seed, size_t n, int key_lo, int key_hi, int32_t* batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (kind == 4) return synth_c5(c, seed, n, key_lo, key_hi, batch);
  if (kind == 1 || kind == 2) return synth_c3(c, kind, seed, n, key_lo, key_hi, batch);
  if (kind == 3) return synth_c4(c, seed, n, batch);
  if (kind == 0 || (kind >= 16 && kind <= 18)) return synth_c2(c, kind, seed, batch);
  set_err("synthetic kind not available");
  return RBG_ERR_ILLEGAL_ARGUMENT;
}

}  // extern "C"
