// The range-encoded index (RB/RangeBitmap.java) on the host side of the engine: the load of a serialized
// index (rangebitmap_format.cpp walks it once), the build of one from a value tensor (rangebitmap_build.hip), its
// way back to a stream (rangebitmap_format.cpp: rb_emit), the dispatch of a query to a shortcut or to k_rb_query
// (rangebitmap.hip), the result batch, and the entry points of include/roaring_mi355x_rangebitmap.h.
#include <algorithm>
#include <cstdlib>

#include "engine.hpp"
#include "rangebitmap_format.hpp"

namespace rbg {

static bool rb_op_ok(int op) { return op >= RBG_RB_LTE && op <= RBG_RB_BETWEEN; }

// the refusals of a query, decided from the arguments alone
int check_rb_query(int op, bool has_ctx, bool count) {
  if (!rb_op_ok(op)) {
    set_err("range bitmap: unknown op (RBG_RB_LTE .. RBG_RB_BETWEEN)");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (op == RBG_RB_BETWEEN && has_ctx && !count) {
    set_err("range bitmap: between(min, max, context) does not exist; betweenCardinality takes a context");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

static int parse_index(const uint8_t* buf, size_t len, RbIndex* idx) {
  std::string err;
  const int st = rb_parse(buf, len, idx, &err);
  if (st) set_err(err);
  return st;
}

static int find_index(Ctx* c, int32_t index, RangeIndex** out) {
  if (index < 0 || (size_t)index >= c->range_indexes.size() || !c->range_indexes[index]) {
    set_err("range bitmap: no such index");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  *out = c->range_indexes[index].get();
  return RBG_OK;
}

// a new index under the lowest free handle
static int32_t register_index(Ctx* c, std::unique_ptr<RangeIndex> R) {
  size_t id = 0;
  while (id < c->range_indexes.size() && c->range_indexes[id]) id++;
  if (id == c->range_indexes.size()) c->range_indexes.emplace_back();
  c->range_indexes[id] = std::move(R);
  return (int32_t)id;
}

static int nlz(uint64_t x) { return x ? __builtin_clzll(x) : 64; }

// RangeBitmap.map (:65-85): the directory and the re-laid containers go up in three copies
int ctx_rb_load(Ctx* c, const uint8_t* buf, size_t len, int32_t* out_index) {
  RbIndex idx;
  CHK(parse_index(buf, len, &idx));
  auto R = std::make_unique<RangeIndex>();
  R->nslices = idx.nslices;
  R->n_blocks = idx.n_blocks;
  R->max_rid = idx.max_rid;
  R->mask = idx.mask;
  R->payload_bytes = idx.payload_bytes;
  R->arena_bytes = idx.arena_bytes;
  if (idx.n_blocks) {
    std::vector<CDesc> dir(idx.dir.size());
    for (size_t j = 0; j < dir.size(); j++) {
      const RbEntry& e = idx.dir[j];
      dir[j] = CDesc{e.slot, e.card, (uint16_t)(j / idx.nslices), e.kind, 0};
    }
    std::vector<uint8_t> arena(idx.arena_bytes);
    rb_relay(buf, idx, arena.data());
    CHK(pool_take(c, R->dir, sizeof(CDesc) * dir.size() + 16));
    CHK(pool_take(c, R->masks, 8 * idx.masks.size() + 16));
    CHK(pool_take(c, R->arena, idx.arena_bytes + kSlack));
    CHK(upload_words(c, R->dir.p, dir.data(), sizeof(CDesc) * dir.size() / 4));
    CHK(upload_words(c, R->masks.p, idx.masks.data(), 2 * idx.masks.size()));
    CHK(upload_words(c, R->arena.p, arena.data(), idx.arena_bytes / 4));
  }
  *out_index = register_index(c, std::move(R));
  return RBG_OK;
}

// Workspace bytes of one pass of the build (rangebitmap_build.hip).  RBG_RB_BUILD_WS=<bytes> overrides the
// default, read at every call (tests force several passes at small shapes); a pass always holds at least one
// whole block's cells.
constexpr size_t kRbbBudget = 1ull << 30;  // a released workspace of this size still goes to the pool
static size_t rbb_budget() {
  const char* e = std::getenv("RBG_RB_BUILD_WS");
  const unsigned long long v = e ? std::strtoull(e, nullptr, 10) : 0;
  return (size_t)std::min<unsigned long long>(v ? v : kRbbBudget, 4ull << 30);
}

constexpr uint64_t kRbMaxRows = 65535ull * 65536;  // the header's u16 maxKey states at most 65,535 blocks

// the refusals of a build, decided from the arguments alone
int check_rb_build(const void* values, uint64_t n, const void* out) {
  if (!out) {
    set_err("range bitmap build: no output");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (n && !values) {
    set_err("range bitmap build: no input");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (n > kRbMaxRows) {
    set_err("range bitmap build: more than 65,535 blocks of 65,536 rows");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// RangeBitmap.appender(max_value) (:52-56), add (:1511-1533) for every one of the n values in device memory, in
// order, and build (:1415-1438), as the resident index that ctx_rb_load of the Appender's stream makes: the same
// directory, masks and slots, at other offsets only (rangebitmap_build.hip).  max_from_data: max_value is the
// largest value given.  A value outside the mask refuses the whole call (the reference throws at that row, with
// the rows before it added).  Two read-backs: the largest value, then the arena's size with the payload bytes.
// One pass: transpose, plan, scan, write from the same workspace.  Several: every pass is transposed and
// planned (sizes alone), the scan places every container, and each pass is transposed again before it is
// written -- the arena is allocated once at its exact size, as the BSI builders' payload is.
// The values are read by every transpose: they must not change until the call returns.
int ctx_rb_build(Ctx* c, const uint64_t* dev_values, uint64_t n, uint64_t max_value, bool max_from_data,
                 int32_t* out_index) {
  CHK(check_rb_build(dev_values, n, out_index));
  hipStream_t s = c->stream;
  CHK(c->scalar.ensure(64));
  unsigned long long* sc = c->scalar.as<unsigned long long>();  // [0] largest value, [1] payload bytes, [2] arena
  unsigned long long h[3] = {0, 0, 0};
  if (n) {
    HIPCHK(hipMemsetAsync(sc, 0, 64, s));
    launch_rbb_max(s, dev_values, n, sc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, sc, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (max_from_data) max_value = h[0];
  const int nslices = 64 - nlz(max_value | 1);  // rangeMask / bytesPerMask of maxValue | 1 (:1622-1630)
  const uint64_t mask = ~0ull >> (64 - nslices);
  if (h[0] & ~mask) {
    set_err(std::to_string(h[0]) + " too large");  // add's message (:1513-1515), for the largest such value
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  auto R = std::make_unique<RangeIndex>();
  R->nslices = (uint32_t)nslices;
  R->n_blocks = (uint32_t)((n + 0xFFFF) >> 16);
  R->max_rid = n;
  R->mask = mask;
  const size_t K = R->n_blocks, cells = K * (size_t)nslices;
  if (K) {
    CHK(c->rbb_info.ensure(kRbbInfoBytes * cells + 16));
    CHK(c->rbb_size.ensure(8 * (cells + 1)));
    CHK(c->rbb_part.ensure(8 * (scan_parts(cells) + 1)));
    uint64_t* size = c->rbb_size.as<uint64_t>();
    const size_t block_bytes = 8192 * (size_t)nslices;
    const size_t P = std::min(K, std::max<size_t>(1, rbb_budget() / block_bytes));  // blocks per pass
    DevBuf ws;  // back to the pool after the last write (freed on an error)
    CHK(pool_take(c, ws, block_bytes * P));
    auto transpose = [&](size_t k_lo, size_t k_hi) {
      launch_rbb_transpose(s, dev_values, n, mask, (uint32_t)k_lo, (uint32_t)k_hi, nslices, ws.as<uint8_t>());
    };
    for (size_t k_lo = 0; k_lo < K; k_lo += P) {
      const size_t k_hi = std::min(K, k_lo + P);
      transpose(k_lo, k_hi);
      launch_rbb_plan(s, ws.as<uint8_t>(), (uint32_t)k_lo, (uint32_t)k_hi, nslices, c->rbb_info.p, size, sc + 1);
    }
    launch_exclusive_scan(s, size, size, cells, c->rbb_part.as<uint64_t>(), reinterpret_cast<uint64_t*>(sc + 2));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h + 1, sc + 1, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    dbg(s, "rangebitmap_build: transpose + plan");
    R->payload_bytes = h[1];
    R->arena_bytes = h[2];
    CHK(pool_take(c, R->dir, sizeof(CDesc) * cells + 16));
    CHK(pool_take(c, R->masks, 8 * K + 16));
    CHK(pool_take(c, R->arena, R->arena_bytes + kSlack));
    for (size_t k_lo = 0; k_lo < K; k_lo += P) {
      const size_t k_hi = std::min(K, k_lo + P);
      if (P < K) transpose(k_lo, k_hi);  // several passes: the workspace held another pass since the plan
      launch_rbb_write(s, ws.as<uint8_t>(), (uint32_t)k_lo, (uint32_t)k_hi, nslices, c->rbb_info.p, size,
                       R->dir.as<CDesc>(), R->masks.as<uint64_t>(), R->arena.as<uint8_t>());
    }
    HIPCHK(hipGetLastError());
    pool_put(c, ws);  // whatever takes it next is enqueued on this stream, after the write kernels
    HIPCHK(hipStreamSynchronize(s));
    dbg(s, "rangebitmap_build: write");
  }
  *out_index = register_index(c, std::move(R));
  return RBG_OK;
}

// the same from host memory: the values go to the device through the context's pinned buffer
int ctx_rb_build_host(Ctx* c, const uint64_t* values, uint64_t n, uint64_t max_value, bool max_from_data,
                      int32_t* out_index) {
  CHK(check_rb_build(values, n, out_index));
  DevBuf in;
  CHK(pool_take(c, in, 8 * n + 16));
  CHK(upload_words(c, in.p, values, 2 * n));
  const int st = ctx_rb_build(c, in.as<uint64_t>(), n, max_value, max_from_data, out_index);
  pool_put(c, in);
  return st;
}

// Appender.serialize (:1483-1504) of a resident index, loaded or built: the directory, the masks and the arena
// come to the host and rangebitmap_format.cpp's rb_emit writes the stream
int ctx_rb_serialize(Ctx* c, int32_t index, rbg_buffer* out) {
  RangeIndex* R;
  CHK(find_index(c, index, &R));
  hipStream_t s = c->stream;
  RbIndex idx;
  idx.nslices = R->nslices;
  idx.n_blocks = R->n_blocks;
  idx.max_rid = R->max_rid;
  idx.mask = R->mask;
  idx.masks.resize(R->n_blocks);
  idx.dir.resize((size_t)R->n_blocks * R->nslices);
  std::vector<CDesc> dir(idx.dir.size());
  std::vector<uint8_t> arena(R->arena_bytes);
  if (R->n_blocks) {
    HIPCHK(hipMemcpyAsync(dir.data(), R->dir.p, sizeof(CDesc) * dir.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(idx.masks.data(), R->masks.p, 8 * idx.masks.size(), hipMemcpyDeviceToHost, s));
    if (R->arena_bytes) HIPCHK(hipMemcpyAsync(arena.data(), R->arena.p, R->arena_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  for (size_t j = 0; j < dir.size(); j++) {
    idx.dir[j].kind = dir[j].kind;
    idx.dir[j].card = dir[j].card;
    idx.dir[j].slot = dir[j].slot;
  }
  std::vector<uint8_t> bytes;
  std::string err;
  const int st = rb_emit(idx, arena.data(), arena.size(), &bytes, &err);
  if (st) {
    set_err(err);
    return st;
  }
  return emit_host(bytes, out);
}

int ctx_rb_release(Ctx* c, int32_t index) {
  RangeIndex* R;
  CHK(find_index(c, index, &R));
  // to the context's pool, like a batch's buffers: whatever takes them next is enqueued behind every query
  for (DevBuf* d : {&R->dir, &R->masks, &R->arena}) pool_put(c, *d);
  c->range_indexes[index].reset();
  return RBG_OK;
}

int ctx_rb_info(Ctx* c, int32_t index, uint64_t* info) {
  RangeIndex* R;
  CHK(find_index(c, index, &R));
  const uint64_t v[6] = {R->nslices, R->n_blocks, R->max_rid, R->mask, R->payload_bytes, 0};
  std::copy(v, v + 6, info);
  return RBG_OK;
}

// What a query comes to, from the arguments and the index's mask alone (:111-119, :206-220, :294-308 and the
// first lines of computePoint / computeRange, :427-429, :552-554)
enum RbOutcome : int { RB_EMPTY = 0, RB_ALL = 1, RB_KERNEL = 2 };
struct RbPlan {
  int outcome;
  int mode;  // RbMode
  uint64_t t0, t1;
};
static RbPlan rb_plan(uint64_t mask, int op, uint64_t a, uint64_t b) {
  auto above = [&](uint64_t t) { return nlz(t) < nlz(mask); };  // Long.numberOfLeadingZeros(t) < ...(mask)
  if (op == RBG_RB_BETWEEN) {
    if (a == 0 || above(a)) {
      op = RBG_RB_LTE;
      a = b;
    } else if (above(b)) {
      op = RBG_RB_GTE;
    } else {
      return {RB_KERNEL, RBM_BETWEEN, a - 1, b};
    }
  }
  switch (op) {
    case RBG_RB_LT:
      if (a == 0) return {RB_EMPTY, 0, 0, 0};
      a--;
      [[fallthrough]];
    case RBG_RB_LTE: return above(a) ? RbPlan{RB_ALL, 0, 0, 0} : RbPlan{RB_KERNEL, RBM_LTE, a, 0};
    case RBG_RB_GTE:
      if (a == 0) return {RB_ALL, 0, 0, 0};
      a--;
      [[fallthrough]];
    case RBG_RB_GT: return above(a) ? RbPlan{RB_EMPTY, 0, 0, 0} : RbPlan{RB_KERNEL, RBM_GT, a, 0};
    case RBG_RB_EQ: return above(a) ? RbPlan{RB_EMPTY, 0, 0, 0} : RbPlan{RB_KERNEL, RBM_EQ, a, 0};
    default: return above(a) ? RbPlan{RB_ALL, 0, 0, 0} : RbPlan{RB_KERNEL, RBM_NEQ, a, 0};
  }
}

// serialized bytes as a new one-bitmap batch; the bytes are released
static int batch_of_bytes(Ctx* c, rbg_buffer* bytes, int32_t* out_batch) {
  const uint8_t* p = bytes->data;
  const int st = ctx_load_separate(c, &p, &bytes->len, 1, out_batch);
  rbg_free(bytes);
  return st;
}

// One query.  out_batch: the bitmap form; else out_count.
static int rb_run(Ctx* c, int32_t index, int op, uint64_t a, uint64_t b, int32_t ctx_batch, size_t ctx_i,
                  int32_t* out_batch, int64_t* out_count) {
  const bool has_ctx = ctx_batch >= 0, count = out_batch == nullptr;
  CHK(check_rb_query(op, has_ctx, count));
  RangeIndex* R;
  CHK(find_index(c, index, &R));
  Operand o{};
  if (has_ctx) CHK(resolve(c, ctx_batch, ctx_i, &o));
  RbPlan pl = rb_plan(R->mask, op, a, b);
  // an empty context first (:456-458, :580-582); then the shortcuts; then an index without rows (no block to visit)
  if ((has_ctx && o.b->long_card == 0) || (pl.outcome == RB_KERNEL && R->n_blocks == 0)) pl.outcome = RB_EMPTY;
  if (pl.outcome == RB_EMPTY) {
    if (count) *out_count = 0;
    return count ? RBG_OK : ctx_empty_bitmap(c, out_batch);
  }
  if (pl.outcome == RB_ALL) {
    if (count) {
      *out_count = has_ctx ? o.b->long_card : (int64_t)R->max_rid;  // context.getLongCardinality() / max
      return RBG_OK;
    }
    rbg_buffer bytes{nullptr, 0};
    if (has_ctx) {  // context.clone(): the context's own containers
      CHK(ctx_batch_fetch_range(c, ctx_batch, ctx_i, ctx_i + 1, &bytes));
      return batch_of_bytes(c, &bytes, out_batch);
    }
    // RoaringBitmap.bitmapOfRange(0, max): the range mutation over an empty bitmap, run containers throughout
    int32_t e;
    CHK(ctx_empty_bitmap(c, &e));
    BatchGuard g{c, {e}};
    CHK(ctx_range_mut(c, RMUT_RANGE, e, 0, 0, (int64_t)R->max_rid, false));
    CHK(ctx_fetch(c, &bytes));
    return batch_of_bytes(c, &bytes, out_batch);
  }
  hipStream_t s = c->stream;
  RbArgs ka{};
  ka.dir = R->dir.as<CDesc>();
  ka.masks = R->masks.as<uint64_t>();
  ka.arena = R->arena.as<uint8_t>();
  ka.n_blocks = R->n_blocks;
  ka.nslices = R->nslices;
  ka.max_rid = R->max_rid;
  ka.mask = R->mask;
  ka.t0 = pl.t0;
  ka.t1 = pl.t1;
  ka.has_ctx = has_ctx ? 1 : 0;
  if (has_ctx) ka.ctx = o;
  if (count) {
    // gtCardinality with a context counts context \ lte (:659-661), not context & flipped rows
    if (has_ctx && pl.mode == RBM_GT) {
      pl.mode = RBM_LTE;
      ka.ctx_minus = 1;
    }
    ka.ctx_first = has_ctx && pl.mode == RBM_BETWEEN;  // DoubleEvaluation.count(lower, upper, context), :977-1014
    CHK(c->scalar.ensure(64));
    ka.count = c->scalar.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(ka.count, 0, 8, s));
    launch_rb_query(s, pl.mode, ka);
    HIPCHK(hipGetLastError());
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, ka.count, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *out_count = (int64_t)h;
    return RBG_OK;
  }
  // the blocks' bits into a workspace of 8 KiB each, which the dense-bitset builder types and writes
  DevBuf ws;
  const uint64_t nbytes = 8192ull * R->n_blocks;
  CHK(pool_take(c, ws, nbytes + 16));
  ka.out = ws.as<uint8_t>();
  launch_rb_query(s, pl.mode, ka);
  HIPCHK(hipGetLastError());
  const int st = ctx_from_bitset(c, ws.p, nbytes, RBG_BITS_PACKED, true, out_batch);
  pool_put(c, ws);
  return st;
}

int ctx_rb_query(Ctx* c, int32_t index, int op, uint64_t a, uint64_t b, int32_t ctx_batch, size_t ctx_i,
                 int32_t* out_batch) {
  return rb_run(c, index, op, a, b, ctx_batch, ctx_i, out_batch, nullptr);
}
int ctx_rb_count(Ctx* c, int32_t index, int op, uint64_t a, uint64_t b, int32_t ctx_batch, size_t ctx_i, int64_t* out) {
  return rb_run(c, index, op, a, b, ctx_batch, ctx_i, nullptr, out);
}

// the one-shot scope: the index and the context of one call, both gone on return
struct RbOneShot : OneShot {
  int32_t index = -1, ctx_batch = -1;
  ~RbOneShot() {
    if (index >= 0) (void)ctx_rb_release(c, index);
  }
  int load_all(const uint8_t* buf, size_t len, const uint8_t* context, size_t context_len) {
    RbIndex probe;
    CHK(parse_index(buf, len, &probe));  // the format errors need no device
    CHK(open());
    CHK(ctx_rb_load(c, buf, len, &index));
    if (context) CHK(load_separate(&context, &context_len, 1, &ctx_batch));
    return RBG_OK;
  }
};

}  // namespace rbg

using namespace rbg;

extern "C" {

int rbg_rangebitmap_validate(const uint8_t* buf, size_t len, uint64_t* info) {
  if (!buf && len) return RBG_ERR_ILLEGAL_ARGUMENT;
  RbIndex idx;
  CHK(parse_index(buf, len, &idx));
  if (info) {
    const uint64_t v[6] = {idx.nslices, idx.n_blocks, idx.max_rid, idx.mask, idx.payload_bytes, idx.stream_bytes};
    std::copy(v, v + 6, info);
  }
  return RBG_OK;
}

int rbg_ctx_rangebitmap_load(rbg_ctx* ctx, const uint8_t* buf, size_t len, int32_t* index) {
  if (!ctx || !index || (!buf && len)) return RBG_ERR_ILLEGAL_ARGUMENT;
  RbIndex probe;
  CHK(parse_index(buf, len, &probe));  // the format errors need no device
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_rb_load(c, buf, len, index);
}

int rbg_ctx_rangebitmap_build(rbg_ctx* ctx, const uint64_t* values, uint64_t n, uint64_t max_value, int max_from_data,
                              int32_t* index) {
  CHK(check_rb_build(values, n, index));  // the refusals need no device
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_rb_build_host(c, values, n, max_value, max_from_data != 0, index);
}

int rbg_ctx_rangebitmap_build_device(rbg_ctx* ctx, const uint64_t* values_dev, uint64_t n, uint64_t max_value,
                                     int max_from_data, int32_t* index) {
  CHK(check_rb_build(values_dev, n, index));
  if (reinterpret_cast<uintptr_t>(values_dev) & 7) {
    set_err("range bitmap build: the values must be 8-byte aligned");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_rb_build(c, values_dev, n, max_value, max_from_data != 0, index);
}

int rbg_ctx_rangebitmap_serialize(rbg_ctx* ctx, int32_t index, rbg_buffer* out) {
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_rb_serialize(c, index, out);
}

int rbg_rangebitmap_build(const uint64_t* values, uint64_t n, uint64_t max_value, int max_from_data, rbg_buffer* out) {
  CHK(check_rb_build(values, n, out));
  RbOneShot os;
  CHK(os.open());
  CHK(ctx_rb_build_host(os.c, values, n, max_value, max_from_data != 0, &os.index));
  return ctx_rb_serialize(os.c, os.index, out);
}

int rbg_rangebitmap_reserialize(const uint8_t* buf, size_t len, rbg_buffer* out) {
  if (!out || (!buf && len)) return RBG_ERR_ILLEGAL_ARGUMENT;
  RbIndex idx;
  CHK(parse_index(buf, len, &idx));
  std::vector<uint8_t> arena(idx.arena_bytes), bytes;
  rb_relay(buf, idx, arena.data());
  std::string err;
  const int st = rb_emit(idx, arena.data(), arena.size(), &bytes, &err);
  if (st) {
    set_err(err);
    return st;
  }
  return emit_host(bytes, out);
}

int rbg_ctx_rangebitmap_release(rbg_ctx* ctx, int32_t index) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_rb_release(c, index);
}

int rbg_ctx_rangebitmap_info(rbg_ctx* ctx, int32_t index, uint64_t* info) {
  if (!ctx || !info) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_rb_info(&ctx->c, index, info);
}

int rbg_ctx_rangebitmap_query(rbg_ctx* ctx, int32_t index, int op, uint64_t a, uint64_t b, int32_t context_batch,
                              size_t context_i, int32_t* out_batch) {
  CHK(check_rb_query(op, context_batch >= 0, false));
  if (!out_batch) return RBG_ERR_ILLEGAL_ARGUMENT;
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_rb_query(c, index, op, a, b, context_batch, context_i, out_batch);
}

int rbg_ctx_rangebitmap_count(rbg_ctx* ctx, int32_t index, int op, uint64_t a, uint64_t b, int32_t context_batch,
                              size_t context_i, int64_t* out) {
  CHK(check_rb_query(op, context_batch >= 0, true));
  if (!out) return RBG_ERR_ILLEGAL_ARGUMENT;
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_rb_count(c, index, op, a, b, context_batch, context_i, out);
}

int rbg_rangebitmap_query(const uint8_t* index, size_t index_len, int op, uint64_t a, uint64_t b,
                          const uint8_t* context, size_t context_len, rbg_buffer* out) {
  CHK(check_rb_query(op, context != nullptr, false));
  if (!out || (!index && index_len)) return RBG_ERR_ILLEGAL_ARGUMENT;
  RbOneShot os;
  CHK(os.load_all(index, index_len, context, context_len));
  int32_t res;
  CHK(ctx_rb_query(os.c, os.index, op, a, b, os.ctx_batch, 0, &res));
  os.adopt(res);
  return ctx_batch_fetch_range(os.c, res, 0, 1, out);
}

int rbg_rangebitmap_count(const uint8_t* index, size_t index_len, int op, uint64_t a, uint64_t b,
                          const uint8_t* context, size_t context_len, int64_t* out) {
  CHK(check_rb_query(op, context != nullptr, true));
  if (!out || (!index && index_len)) return RBG_ERR_ILLEGAL_ARGUMENT;
  RbOneShot os;
  CHK(os.load_all(index, index_len, context, context_len));
  return ctx_rb_count(os.c, os.index, op, a, b, os.ctx_batch, 0, out);
}

}  // extern "C"
