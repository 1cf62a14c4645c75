// Batches of values added to or removed from a resident bitmap (mutate.hip) and their entry points
// (include/roaring_mi355x_mutate.h); the host form is mutate_host.cpp.
#include <algorithm>

#include "engine.hpp"
#include "format.hpp"

namespace rbg {

// the refusals decided from the arguments alone
static int check_mutate_args(int op, const void* values, size_t n, const void* out, const void* changed) {
  if (op != RBG_MUT_ADD && op != RBG_MUT_REMOVE) {
    set_err("mutate_values: op must be RBG_MUT_ADD or RBG_MUT_REMOVE");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (!out || !changed) {
    set_err("mutate_values: null output");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (n && !values) {
    set_err("mutate_values: no values");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// the refusals of the operand, from the batch's host fields: no device work before them
static int check_mutate_batch(Ctx* c, int32_t batch) {
  Batch* b;
  CHK(find_batch(c, batch, &b));
  if (b->n_bm != 1 || !b->key_major || b->packed) {
    set_err("mutate_values: the operand must be a single-bitmap key-major batch with slot-aligned payloads");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// n values in device memory (u32, any order, duplicates allowed) added to (op 0) or removed from (op 1) bitmap
// 0 of a batch check_mutate_batch accepts, as a new one-bitmap key-major batch; *changed: the values actually
// added or removed.  Two read-backs: the key counts (to size the workspace of 8 KiB cells, one per touched
// key) and the totals with the placement (payload size, kinds, cardinality).  The values are read by two
// kernels: they must not change until the call returns.
static int ctx_mutate_values(Ctx* c, int32_t batch, int op, const uint32_t* v_dev, size_t n, int32_t* out_id,
                             uint64_t* changed) {
  Operand A;
  CHK(resolve(c, batch, 0, &A));
  hipStream_t s = c->stream;
  const size_t Ca = A.b->n_ctr;
  const BmView av{A.key_off, A.desc, A.payload, (int)Ca};
  // the two key scans: [0] over the values' keys, [1] over k_mut_flags' flags
  CHK(c->mut_flag.ensure(kMaxKeys));
  CHK(c->mut_keys.ensure(2 * 2 * kMaxKeys));
  CHK(c->mut_off.ensure(2 * 4 * (kMaxKeys + 4)));
  CHK(c->mut_sc.ensure(128));
  uint16_t* keys2[2] = {c->mut_keys.as<uint16_t>(), c->mut_keys.as<uint16_t>() + kMaxKeys};
  uint32_t* off2[2] = {c->mut_off.as<uint32_t>(), c->mut_off.as<uint32_t>() + (kMaxKeys + 4)};
  // [0] touched keys, [1] keys of the second scan, [2..8] the plan's totals, [9] the placement's total
  unsigned long long* sc = c->mut_sc.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(c->flag.p, 0, kMaxKeys, s));
  HIPCHK(hipMemsetAsync(sc, 0, 128, s));
  launch_bld_keys(s, v_dev, n, c->flag.as<uint8_t>(), keys2[0], off2[0], sc);
  launch_mut_flags(s, c->flag.as<uint8_t>(), A.key_off, Ca != 0, op, c->mut_flag.as<uint8_t>());
  launch_bld_keys(s, nullptr, 0, c->mut_flag.as<uint8_t>(), keys2[1], off2[1], sc + 1);
  HIPCHK(hipGetLastError());
  unsigned long long h[16] = {};
  HIPCHK(hipMemcpyAsync(h, sc, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  dbg(s, "mutate_values: keys");
  // add: a cell per touched key, candidates = touched or present; remove: a cell per touched and present key,
  // candidates = the operand's own keys
  const bool add = op == RBG_MUT_ADD;
  const size_t n_cells = (size_t)h[add ? 0 : 1];
  const uint16_t* cell_keys = keys2[add ? 0 : 1];
  const uint32_t* cell_off = off2[add ? 0 : 1];
  const size_t n_cand = add ? (size_t)h[1] : Ca;
  const uint16_t* cand_keys = add ? keys2[1] : A.b->keys.as<uint16_t>();

  const int32_t id = new_batch(c);
  Batch& b = *c->batches[id];
  BatchGuard guard{c, {id}};  // an error below frees the half-built batch
  DevBuf ws;  // the cells; back to the pool at the end (freed on an error)
  if (n_cells) {
    CHK(pool_take(c, ws, 8192 * n_cells));
    CHK(c->mut_run.ensure(n_cells + 16));
    CHK(c->mut_card.ensure(4 * n_cells + 16));
    launch_mut_expand(s, av, cell_keys, (uint32_t)n_cells, ws.as<uint8_t>(), c->mut_run.as<uint8_t>(),
                      c->mut_card.as<uint32_t>());
    launch_mut_apply(s, v_dev, n, op, cell_off, ws.as<uint32_t>());
  }
  if (n_cand) {
    CHK(c->mut_info.ensure(kMutInfoBytes * n_cand));
    CHK(c->mut_size.ensure(8 * n_cand + 16));
    CHK(c->mut_part.ensure(8 * (scan_parts(n_cand) + 1)));
    launch_mut_plan(s, av, cand_keys, n_cand, cell_off, ws.as<uint8_t>(), c->mut_run.as<uint8_t>(),
                    c->mut_card.as<uint32_t>(), c->mut_info.p, c->mut_size.as<uint64_t>(), sc + 2);
    launch_exclusive_scan(s, c->mut_size.as<uint64_t>(), c->mut_size.as<uint64_t>(), n_cand, c->mut_part.as<uint64_t>(),
                          reinterpret_cast<uint64_t*>(sc + 9));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, sc, 80, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    dbg(s, "mutate_values: expand + apply + plan");
  }
  const size_t C = (size_t)(h[9] >> kMutCountShift);
  b.payload_bytes = (size_t)(h[9] & ((1ull << kMutCountShift) - 1));
  CHK(pool_take(c, b.keys, 2 * C + 16));
  CHK(pool_take(c, b.key_off, 4 * (kMaxKeys + 1)));
  CHK(pool_take(c, b.bm_off, 4 * 2));
  CHK(pool_take(c, b.desc, sizeof(CDesc) * C + 16));
  CHK(pool_take(c, b.bm, 4 * C + 16));
  CHK(pool_take(c, b.payload, b.payload_bytes + 64));
  if (n_cand)
    launch_mut_write(s, av, cand_keys, n_cand, (uint32_t)C, cell_off, ws.as<uint8_t>(), c->mut_info.p,
                     c->mut_size.as<uint64_t>(), b.desc.as<CDesc>(), b.keys.as<uint16_t>(), b.bm.as<uint32_t>(),
                     b.bm_off.as<uint32_t>(), b.payload.as<uint8_t>());
  else
    HIPCHK(hipMemsetAsync(b.bm_off.p, 0, 8, s));
  launch_dec_key_off(s, b.keys.as<uint16_t>(), C, b.key_off.as<uint32_t>());
  HIPCHK(hipGetLastError());
  dbg(s, "mutate_values: write");
  pool_put(c, ws);  // whatever takes it next is enqueued on this stream, after the write kernel
  b.n_bm = 1;
  b.n_ctr = C;
  b.key_major = true;
  b.gapped = false;
  for (int k = 0; k < 3; k++) b.n_kind[k] = (int64_t)h[2 + k];
  const bool has_run = h[4] != 0;
  b.ser_bytes = (int64_t)(header_size(C, has_run) + h[5]);
  b.long_card = (int64_t)h[6];
  b.max_ser = (size_t)h[8];  // run containers above kStagedMax: copied from the operand or grown by the call
  b.h_bm_off = {0, (uint32_t)C};
  b.h_bm_nctr = {(uint32_t)C};
  b.h_bm_card = {b.long_card};
  b.h_has_run = {(uint8_t)has_run};
  b.live = true;
  guard.ids.clear();
  *out_id = id;
  *changed = (uint64_t)h[7];
  return RBG_OK;
}

// the same from host memory
static int ctx_mutate_values_host(Ctx* c, int32_t batch, int op, const uint32_t* v, size_t n, int32_t* out_id,
                                  uint64_t* changed) {
  DevBuf in;
  CHK(pool_take(c, in, 4 * n + 16));
  CHK(upload_words(c, in.p, v, n));  // 64 MiB chunks through the pinned buffer
  const int st = ctx_mutate_values(c, batch, op, in.as<uint32_t>(), n, out_id, changed);
  pool_put(c, in);
  return st;
}

}  // namespace rbg

using namespace rbg;

extern "C" {

int rbg_ctx_mutate_values(rbg_ctx* ctx, int32_t batch, int op, const uint32_t* values, size_t n, int32_t* out_batch,
                          uint64_t* changed) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  CHK(check_mutate_args(op, values, n, out_batch, changed));
  CHK(check_mutate_batch(&ctx->c, batch));
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_mutate_values_host(c, batch, op, values, n, out_batch, changed);
}

int rbg_ctx_mutate_values_device(rbg_ctx* ctx, int32_t batch, int op, const void* values_dev, size_t n,
                                 int32_t* out_batch, uint64_t* changed) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  CHK(check_mutate_args(op, values_dev, n, out_batch, changed));
  CHK(check_mutate_batch(&ctx->c, batch));
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_mutate_values(c, batch, op, reinterpret_cast<const uint32_t*>(values_dev), n, out_batch, changed);
}

int rbg_mutate_values(const uint8_t* buf, size_t len, int op, const uint32_t* values, size_t n, rbg_buffer* out,
                      uint64_t* changed) {
  CHK(check_mutate_args(op, values, n, out, changed));
  if (!buf && len) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id, res;
  CHK(os.load_separate(&buf, &len, 1, &id));
  CHK(ctx_mutate_values_host(c, id, op, values, n, &res, changed));
  os.adopt(res);
  return ctx_batch_fetch_range(c, res, 0, 1, out);
}

}  // extern "C"
