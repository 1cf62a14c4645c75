// The bit-sliced-index (BSI) host code of the MI355X Roaring engine: the batch builders and read-outs
// (from pairs, add, setValues, values back, IN-list, transpose), the compare and sum pipelines of both
// packages, and their exported entry points.  What it needs from the core (engine.cpp) and the loads
// (engine_load.cpp) is declared in engine.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"
#include "format.hpp"

namespace rbg {

// the seeds of a {min, max} pair that kernels lower and raise with atomics: signed values, unsigned values
static const int32_t kMinMaxSeedI32[2] = {INT32_MAX, INT32_MIN};
static const uint32_t kMinMaxSeedU32[2] = {0xFFFFFFFFu, 0u};

// Workspace bytes of one pass of the BSI build (bsibuild.hip).  RBG_BSI_BUILD_WS=<bytes> overrides the
// default, read at every call (tests force several passes at small shapes); a pass always holds at least
// one key's m bitmaps and stays below 2^31 words.
constexpr size_t kBsibBudget = 1ull << 30;  // a released workspace of this size still goes to the pool (kPoolMaxBuf)
static size_t bsib_budget() {
  const char* e = std::getenv("RBG_BSI_BUILD_WS");
  const unsigned long long v = e ? std::strtoull(e, nullptr, 10) : 0;
  return (size_t)std::min<unsigned long long>(v ? v : kBsibBudget, 4ull << 30);
}

// A planned workspace (bsibuild.hip's cells): K present keys x m cells of 8 KiB, walked P whole keys per pass
// under bsib_budget().  begin sizes the scratch and takes the workspace, sweep fills and plans every pass and
// scans the sizes, emit writes the batch.  One pass: fill, plan, scan, write from the same workspace.  Several:
// the sweep plans every pass (sizes alone), the scan places every container, and emit fills each pass again
// before it writes -- the payload is allocated once at its exact size.
// fill(k_lo, k_hi, first) enqueues whatever leaves the cells of keys [k_lo, k_hi) at the front of ws; first: the
// call comes from the first sweep (a caller's once-only statistics), not from a later sweep or from emit.
struct BsibPlan {
  Ctx* c;
  size_t K = 0;
  int m = 0;
  size_t key_bytes = 0;  // of ws per key: the m cells, then whatever the caller keeps after a pass's cells
  size_t P = 0;          // keys per pass
  DevBuf ws;             // back to the pool at the end of emit (freed on an error)
  std::vector<unsigned long long> hp;  // the plan's per-input totals: 4 per cell column, then the three kind counts
  uint64_t total = 0;                  // the scan's total: containers << kBsibCountShift | payload bytes
  bool run_opt = false;                // the plan types as runOptimize() does
  bool ebm_run = false;                // the plan reads bsia_run: per key, column 0 is a full run container

  size_t cells() const { return K * (size_t)m; }
  size_t per_bytes() const { return 8 * (4 * (size_t)m + 4); }

  int begin(Ctx* ctx, size_t n_keys, int n_cols, size_t extra_key_bytes, bool run_optimize, bool reads_ebm_run) {
    c = ctx, K = n_keys, m = n_cols, run_opt = run_optimize, ebm_run = reads_ebm_run;
    key_bytes = 8192 * (size_t)m + extra_key_bytes;
    CHK(c->bsib_info.ensure(kBsibInfoBytes * cells() + 16));
    CHK(c->bsib_size.ensure(8 * (cells() + 1)));
    CHK(c->bsib_part.ensure(8 * (scan_parts(cells()) + 1)));
    CHK(c->bsib_per.ensure(per_bytes()));
    if (ebm_run) CHK(c->bsia_run.ensure(K + 16));
    HIPCHK(hipMemsetAsync(c->bsib_per.p, 0, per_bytes(), c->stream));
    hp.assign(4 * (size_t)m + 4, 0);
    P = std::min(K, std::max<size_t>(1, bsib_budget() / key_bytes));
    if (K) CHK(pool_take(c, ws, key_bytes * P));  // bsi_add of two empty indexes has no key
    return RBG_OK;
  }

  // Every pass filled (a later sweep: only when there are several, the one pass is still in ws) and planned,
  // the sizes scanned, hp and total read back.  more(): the caller's own device-to-host copies, enqueued in
  // front of the one synchronise.
  template <class Fill, class More>
  int sweep(bool first, Fill&& fill, More&& more) {
    hipStream_t s = c->stream;
    uint64_t* size = c->bsib_size.as<uint64_t>();
    unsigned long long* per = c->bsib_per.as<unsigned long long>();
    if (!first) HIPCHK(hipMemsetAsync(per, 0, per_bytes(), s));
    for (size_t k_lo = 0; k_lo < K; k_lo += P) {
      const size_t k_hi = std::min(K, k_lo + P);
      if (first || P < K) CHK(fill(k_lo, k_hi, first));
      launch_bsib_plan(s, ws.as<uint8_t>(), (uint32_t)k_lo, (uint32_t)k_hi, m, run_opt ? 1 : 0, c->bsib_info.p, size, per,
                       per + 4 * m, ebm_run ? c->bsia_run.as<uint8_t>() : nullptr);
    }
    launch_exclusive_scan(s, size, size, cells(), c->bsib_part.as<uint64_t>(), size + cells());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hp.data(), per, 8 * hp.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&total, size + cells(), 8, hipMemcpyDeviceToHost, s));
    CHK(more());
    HIPCHK(hipStreamSynchronize(s));
    return RBG_OK;
  }
  template <class Fill>
  int sweep(bool first, Fill&& fill) {
    return sweep(first, fill, [] { return RBG_OK; });
  }

  // The batch: the first n_bm cell columns are its bitmaps (any further column holds no container).
  template <class Fill>
  int emit(int n_bm, Fill&& fill, const char* what, int32_t* out_id) {
    hipStream_t s = c->stream;
    uint64_t* size = c->bsib_size.as<uint64_t>();
    const size_t C = (size_t)(total >> kBsibCountShift);
    const int32_t id = new_batch(c);
    Batch& b = *c->batches[id];
    BatchGuard guard{c, {id}};  // dropped unless the build completes
    b.payload_bytes = (size_t)(total & ((1ull << kBsibCountShift) - 1));
    CHK(pool_take(c, b.keys, 2 * C + 16));
    CHK(pool_take(c, b.desc, sizeof(CDesc) * C + 16));
    CHK(pool_take(c, b.bm, 4 * C + 16));
    CHK(pool_take(c, b.key_off, 4 * (kMaxKeys + 1)));
    CHK(pool_take(c, b.bm_off, 4 * ((size_t)n_bm + 1)));
    CHK(pool_take(c, b.payload, b.payload_bytes + 64));
    for (size_t k_lo = 0; k_lo < K; k_lo += P) {
      const size_t k_hi = std::min(K, k_lo + P);
      if (P < K) CHK(fill(k_lo, k_hi, false));  // several passes: the workspace held another pass since the plan
      launch_bsib_write(s, ws.as<uint8_t>(), (uint32_t)k_lo, (uint32_t)k_hi, m, c->bsib_info.p, size,
                        c->bsib_pkeys.as<uint16_t>(), b.desc.as<CDesc>(), b.keys.as<uint16_t>(), b.bm.as<uint32_t>(),
                        b.payload.as<uint8_t>());
    }
    launch_bsib_key_off(s, c->bsib_pkoff.as<uint32_t>(), size, m, b.key_off.as<uint32_t>());
    HIPCHK(hipGetLastError());
    pool_put(c, ws);  // whatever takes it next is enqueued on this stream, after the write kernels
    b.n_bm = (size_t)n_bm;
    b.n_ctr = C;
    b.key_major = true;
    for (int k = 0; k < 3; k++) b.n_kind[k] = (int64_t)hp[4 * m + k];
    b.max_ser = 0;  // no container above kStagedMax serialized bytes
    b.h_bm_off.assign(n_bm + 1, 0);
    b.h_bm_nctr.resize(n_bm);
    b.h_bm_card.resize(n_bm);
    b.h_has_run.resize(n_bm);
    for (int i = 0; i < n_bm; i++) {
      b.h_bm_nctr[i] = (uint32_t)hp[4 * i];
      b.h_bm_off[i + 1] = b.h_bm_off[i] + b.h_bm_nctr[i];
      b.h_bm_card[i] = (int64_t)hp[4 * i + 1];
      b.h_has_run[i] = hp[4 * i + 3] != 0;
      b.long_card += b.h_bm_card[i];
      b.ser_bytes += (int64_t)(header_size(b.h_bm_nctr[i], b.h_has_run[i] != 0) + hp[4 * i + 2]);
    }
    HIPCHK(hipMemcpyAsync(b.bm_off.p, b.h_bm_off.data(), 4 * ((size_t)n_bm + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    dbg(s, what);
    guard.ids.clear();
    b.live = true;
    *out_id = id;
    return RBG_OK;
  }
};

// The present keys of a builder's result, the first of its two read-backs.  begin: bsib_pkeys / bsib_pkoff sized,
// the key flags and the 64 scalar bytes zeroed, scalar[1] seeded as a {min, max} pair (kMinMaxSeedI32 / U32); the
// caller then enqueues its own key and min / max kernels.  end: their error, then K = scalar[0] read back,
// synchronising -- with mn / mx the values' signed {min, max} too, a negative one refused; both null: K alone.
static int bsi_keys_begin(Ctx* c, const void* seed) {
  unsigned long long* sc = c->scalar.as<unsigned long long>();
  CHK(c->bsib_pkeys.ensure(2 * kMaxKeys + 16));
  CHK(c->bsib_pkoff.ensure(4 * (kMaxKeys + 1)));
  HIPCHK(hipMemsetAsync(c->flag.p, 0, kMaxKeys, c->stream));
  HIPCHK(hipMemsetAsync(sc, 0, 64, c->stream));
  HIPCHK(hipMemcpyAsync(sc + 1, seed, 8, hipMemcpyHostToDevice, c->stream));
  return RBG_OK;
}
static int bsi_keys_end(Ctx* c, size_t* K, int32_t* mn, int32_t* mx) {
  HIPCHK(hipGetLastError());
  unsigned long long h[2] = {};
  HIPCHK(hipMemcpyAsync(h, c->scalar.p, mn ? 16 : 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *K = (size_t)h[0];
  if (!mn) return RBG_OK;
  *mn = (int32_t)(uint32_t)h[1], *mx = (int32_t)(uint32_t)(h[1] >> 32);
  if (*mn < 0) {
    set_err("Values should be non-negative");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// Integer.toBinaryString(max).length(): the slices a largest value of max needs
static int bsi_bit_length(int32_t max) { return max ? 32 - __builtin_clz((uint32_t)max) : 1; }

// pairs from host memory: the two arrays go to the device through the context's pinned buffer, then
// call(columns, values) runs on the device copies
template <class Call>
static int bsi_with_pairs(Ctx* c, const uint32_t* col, const int32_t* val, size_t n, Call&& call) {
  DevBuf dc, dv;
  CHK(pool_take(c, dc, 4 * n + 16));
  CHK(pool_take(c, dv, 4 * n + 16));
  CHK(upload_words(c, dc.p, col, n));
  CHK(upload_words(c, dv.p, val, n));
  const int st = call(dc.as<uint32_t>(), dv.as<int32_t>());
  pool_put(c, dc);
  pool_put(c, dv);
  return st;
}

// An index as the operand of add and setValues (op: the name in the messages): a key-major, unpacked batch
// [ebM, bA[0..nbits-1]]
static int bsi_index_operand(Ctx* c, const char* op, int32_t id, int nbits, Batch** B, BsiAddSide* side) {
  CHK(get_batch(c, id, B));
  const Batch* b = *B;
  if (nbits < 0 || nbits > 32) {
    set_err(std::string(op) + ": an index holds at most 32 slices");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (!b->key_major || b->packed || b->n_bm != (size_t)(1 + nbits)) {
    set_err(std::string(op) + ": batch must be key-major, unpacked and hold ebM and nbits slices");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  *side = BsiAddSide{b->key_off.as<uint32_t>(), b->desc.as<CDesc>(), b->bm.as<uint32_t>(), b->payload.as<uint8_t>(), nbits};
  return RBG_OK;
}

// A bit-sliced index from n (column, value) pairs in device memory (u32 columns, all distinct; i32 values,
// none negative; any order) as a new key-major batch [ebM, bA[0..nbits-1]]: setValue for every pair
// (BSI/:299-347: ensureCapacityInternal's min / max and bit count, then ebM.add and one add per set bit),
// with run_opt followed by runOptimize() (BSI/:141-150) -- the batch ctx_load of the host builder's
// bitmaps gives (bsibuild.hip).  out3 = {nbits, minValue, maxValue}.  Two read-backs: the key count with
// min / max (a negative value is refused here), then the per-input totals (a repeated column shows as
// cardinality(ebM) != n and is refused before anything is allocated for the batch).
// The K x (nbits + 1) bitmaps are a BsibPlan whose fill is the scatter.  The pairs are read by every scatter:
// they must not change until the call returns.
static int ctx_bsi_from_columns(Ctx* c, const uint32_t* col_dev, const int32_t* val_dev, size_t n, bool run_opt,
                                int32_t* out_id, int32_t* out3) {
  hipStream_t s = c->stream;
  out3[0] = out3[1] = out3[2] = 0;
  if (n == 0) return ctx_empty_bitmap(c, out_id);  // ebM, no slice
  if (n > (1ull << 32)) {
    set_err("bsi_from_columns: more pairs than columns");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  unsigned long long* sc = c->scalar.as<unsigned long long>();  // [0] K, [1] {min, max} as two i32
  CHK(bsi_keys_begin(c, kMinMaxSeedI32));
  launch_bld_keys(s, col_dev, n, c->flag.as<uint8_t>(), c->bsib_pkeys.as<uint16_t>(), c->bsib_pkoff.as<uint32_t>(), sc);
  launch_bsib_minmax(s, val_dev, n, reinterpret_cast<int*>(sc + 1));
  size_t K;
  int32_t mn, mx;
  CHK(bsi_keys_end(c, &K, &mn, &mx));
  const int nbits = bsi_bit_length(mx);
  const int m = nbits + 1;
  dbg(s, "bsi_from_columns: keys + min / max");
  BsibPlan plan;
  CHK(plan.begin(c, K, m, 0, run_opt, false));
  auto scatter = [&](size_t k_lo, size_t k_hi, bool) -> int {
    HIPCHK(hipMemsetAsync(plan.ws.p, 0, 8192 * (size_t)m * (k_hi - k_lo), s));
    launch_bsib_scatter(s, col_dev, val_dev, n, c->bsib_pkoff.as<uint32_t>(), (uint32_t)k_lo, (uint32_t)k_hi, m,
                        plan.ws.as<uint32_t>());
    return RBG_OK;
  };
  CHK(plan.sweep(true, scatter));
  dbg(s, "bsi_from_columns: scatter + plan");
  if (plan.hp[1] != n) {  // setValue overwrites: a column given twice would need the pairs' order
    set_err("bsi_from_columns: a column is given more than once");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(plan.emit(m, scatter, "bsi_from_columns: write", out_id));
  out3[0] = nbits;
  out3[1] = mn;
  out3[2] = mx;
  return RBG_OK;
}

// the same from host memory: the pairs go to the device through the context's pinned buffer
static int ctx_bsi_from_columns_host(Ctx* c, const uint32_t* col, const int32_t* val, size_t n, bool run_opt,
                                     int32_t* out_id, int32_t* out3) {
  return bsi_with_pairs(c, col, val, n, [&](const uint32_t* dc, const int32_t* dv) {
    return ctx_bsi_from_columns(c, dc, dv, n, run_opt, out_id, out3);
  });
}

// An operand of the fused add: an index operand that is run-free as well
static int bsi_add_operand(Ctx* c, int32_t id, int nbits, Batch** B, BsiAddSide* side) {
  CHK(bsi_index_operand(c, "bsi_add", id, nbits, B, side));
  if ((*B)->n_kind[DK_R] != 0) {
    set_err("bsi_add: an operand holds a run container; the composed route (and / xor per slice) handles it");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// RoaringBitmapSliceIndex.add (BSI/:66-95; MutableBitSliceIndex.add, buffer/MutableBitSliceIndex.java:121-130,
// 201-262) of two resident run-free indexes as a new key-major batch [ebM', bA'[0..n'-1]]: what ctx_load of
// the reference's result bitmaps gives (bsiadd.hip; both operands untouched, batch_a == batch_b doubles).
// out3 = {n', minValue, maxValue}, min / max from the descent of BSI/:97-138 as Java ints.  An empty ebM of
// b (:67-69): a copy of a with {nbits_a, min_a, max_a}.  Two read-backs: the key count, then the per-input
// totals with min / max -- the carry out of the top input slice decides whether the result has one more
// slice, and out of slice 31 it is refused before a batch exists.  The K x (2 + max(na, nb)) bitmaps are a
// BsibPlan whose fill is the add, followed in the sweep by the min / max descent.
static int ctx_bsi_add(Ctx* c, int32_t batch_a, int nbits_a, int32_t batch_b, int nbits_b, int32_t min_a, int32_t max_a,
                       int32_t* out_id, int32_t* out3) {
  hipStream_t s = c->stream;
  Batch *A, *B;
  BsiAddSide sa, sb;
  CHK(bsi_add_operand(c, batch_a, nbits_a, &A, &sa));
  CHK(bsi_add_operand(c, batch_b, nbits_b, &B, &sb));
  const bool b_empty = B->h_bm_card.empty() || B->h_bm_card[0] == 0;
  if (b_empty) sb = BsiAddSide{nullptr, nullptr, nullptr, nullptr, 0};
  const int top = b_empty ? nbits_a : std::max(nbits_a, nbits_b);
  const int m = top + 2;
  unsigned long long* sc = c->scalar.as<unsigned long long>();  // [0] K, [1] {min, max} as two u32
  CHK(bsi_keys_begin(c, kMinMaxSeedU32));
  launch_bsia_keys(s, A->keys.as<uint16_t>(), A->n_ctr, B->keys.as<uint16_t>(), b_empty ? 0 : B->n_ctr,
                   c->flag.as<uint8_t>());
  launch_bld_keys(s, nullptr, 0, c->flag.as<uint8_t>(), c->bsib_pkeys.as<uint16_t>(), c->bsib_pkoff.as<uint32_t>(), sc);
  size_t K;
  CHK(bsi_keys_end(c, &K, nullptr, nullptr));  // min / max come with the second read-back
  dbg(s, "bsi_add: keys");
  BsibPlan plan;
  CHK(plan.begin(c, K, m, 0, false, true));
  auto fill = [&](size_t k_lo, size_t k_hi, bool first) -> int {  // every cell of the pass is written: no memset
    launch_bsi_add(s, sa, sb, c->bsib_pkeys.as<uint16_t>(), (uint32_t)k_lo, (uint32_t)k_hi, m, plan.ws.as<uint8_t>(),
                   c->bsia_run.as<uint8_t>());
    if (first && !b_empty)
      launch_bsia_minmax(s, plan.ws.as<uint8_t>(), (uint32_t)(k_hi - k_lo), m, reinterpret_cast<uint32_t*>(sc + 1));
    return RBG_OK;
  };
  uint32_t mm[2] = {0, 0};
  auto read_mm = [&]() -> int {
    HIPCHK(hipMemcpyAsync(mm, sc + 1, 8, hipMemcpyDeviceToHost, s));
    return RBG_OK;
  };
  CHK(plan.sweep(true, fill, read_mm));
  dbg(s, "bsi_add: add + plan");
  const bool grown = plan.hp[4 * (size_t)(m - 1) + 1] != 0;  // a carry left the top input slice
  if (grown && top == 32) {
    set_err("bsi_add: the sum needs more than 32 slices");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const int nbits = top + (grown ? 1 : 0);
  CHK(plan.emit(1 + nbits, fill, "bsi_add: write", out_id));
  out3[0] = nbits;
  if (b_empty) {  // the reference returns before it recomputes them
    out3[1] = min_a;
    out3[2] = max_a;
  } else {  // an empty ebM' (b's ebM holds a column: cannot be) would leave {~0u, 0}; minValue() gives 0 then
    out3[1] = mm[0] <= mm[1] ? (int32_t)mm[0] : 0;
    out3[2] = mm[0] <= mm[1] ? (int32_t)mm[1] : 0;
  }
  return RBG_OK;
}

// RoaringBitmapSliceIndex.setValues(List<Pair>) (BSI/:349-357; setValue, :299-313, is n == 1; the buffer
// package's MutableBitSliceIndex.setValues, buffer/MutableBitSliceIndex.java:146-195) of n >= 1 pairs in device
// memory (u32 columns, repeated at will; i32 values, none negative; the pair with the highest index decides a
// column) on a resident index, the key-major batch [ebM, bA[0..nbits-1]] with the caller's min / max, as a new
// batch [ebM', bA'[0..d'-1]]: what ctx_load of the reference's bitmaps after the call gives (bsiset.hip; the
// operand untouched).  out3 = {d', minValue, maxValue} by ensureCapacityInternal (BSI/:315-326) over the
// batch's own extremes -- its else-if included: a batch below min and above max lowers min alone, and the
// high bits of its values are dropped.  Two read-backs: the key count with min / max (a negative value is
// refused here), then the plan's totals with the run-container refusal (a slice may hold none, ebM only full
// ones, which stay run containers).  The K x (1 + d') bitmaps are a BsibPlan whose fill expands the operand
// and applies the pairs, with the last-pair table of 256 KiB as a key's extra bytes.  The pairs are read by
// every pass: they must not change until the call returns.
static int ctx_bsi_set_values(Ctx* c, int32_t batch, int nbits, int32_t min_v, int32_t max_v, const uint32_t* col_dev,
                              const int32_t* val_dev, size_t n, int32_t* out_id, int32_t* out3) {
  hipStream_t s = c->stream;
  Batch* A;
  BsiAddSide sa;
  CHK(bsi_index_operand(c, "bsi_set_values", batch, nbits, &A, &sa));
  if (n == 0 || n > 0xFFFFFFFFull) {  // values.stream().max().getAsInt() throws on an empty list
    set_err(n ? "bsi_set_values: more pairs than a 32-bit pair index holds" : "bsi_set_values: no pair given");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const bool was_empty = A->h_bm_card.empty() || A->h_bm_card[0] == 0;
  unsigned long long* sc = c->scalar.as<unsigned long long>();  // [0] K, [1] {min, max} as two i32, [2] refused
  CHK(bsi_keys_begin(c, kMinMaxSeedI32));
  launch_bsia_keys(s, A->keys.as<uint16_t>(), A->n_ctr, nullptr, 0, c->flag.as<uint8_t>());
  launch_bld_keys(s, col_dev, n, c->flag.as<uint8_t>(), c->bsib_pkeys.as<uint16_t>(), c->bsib_pkoff.as<uint32_t>(), sc);
  launch_bsib_minmax(s, val_dev, n, reinterpret_cast<int*>(sc + 1));
  size_t K;
  int32_t mn, mx;
  CHK(bsi_keys_end(c, &K, &mn, &mx));
  dbg(s, "bsi_set_values: keys + min / max");
  const int need = bsi_bit_length(mx);
  int d = nbits;
  if (was_empty) {  // ensureCapacityInternal
    min_v = mn;
    max_v = mx;
    d = std::max(d, need);
  } else if (min_v > mn) {
    min_v = mn;
  } else if (max_v < mx) {
    max_v = mx;
    d = std::max(d, need);
  }
  const int m = 1 + d;
  constexpr size_t kTab = 4 * 65536;  // a key's last-pair table: after the cells of a pass
  BsibPlan plan;
  CHK(plan.begin(c, K, m, kTab, false, true));
  uint32_t* tab = reinterpret_cast<uint32_t*>(plan.ws.as<uint8_t>() + 8192 * (size_t)m * plan.P);
  auto fill = [&](size_t k_lo, size_t k_hi, bool) -> int {  // every cell of the pass is written: no memset
    launch_bsis_expand(s, sa, c->bsib_pkeys.as<uint16_t>(), (uint32_t)k_lo, (uint32_t)k_hi, m, plan.ws.as<uint8_t>(),
                       c->bsia_run.as<uint8_t>(), reinterpret_cast<uint32_t*>(sc + 2));
    HIPCHK(hipMemsetAsync(tab, 0, kTab * (k_hi - k_lo), s));
    launch_bsis_last(s, col_dev, n, c->bsib_pkoff.as<uint32_t>(), (uint32_t)k_lo, (uint32_t)k_hi, tab);
    launch_bsis_apply(s, col_dev, val_dev, n, c->bsib_pkoff.as<uint32_t>(), (uint32_t)k_lo, (uint32_t)k_hi, m, tab,
                      plan.ws.as<uint32_t>());
    return RBG_OK;
  };
  uint32_t bad = 0;
  auto read_bad = [&]() -> int {
    HIPCHK(hipMemcpyAsync(&bad, sc + 2, 4, hipMemcpyDeviceToHost, s));
    return RBG_OK;
  };
  CHK(plan.sweep(true, fill, read_bad));
  dbg(s, "bsi_set_values: expand + apply + plan");
  if (bad) {
    set_err("bsi_set_values: a slice holds a run container, or ebM one that is not full");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(plan.emit(m, fill, "bsi_set_values: write", out_id));
  out3[0] = d;
  out3[1] = min_v;
  out3[2] = max_v;
  return RBG_OK;
}

// the same from host memory: the pairs go to the device through the context's pinned buffer
static int ctx_bsi_set_values_host(Ctx* c, int32_t batch, int nbits, int32_t min_v, int32_t max_v, const uint32_t* col,
                                   const int32_t* val, size_t n, int32_t* out_id, int32_t* out3) {
  return bsi_with_pairs(c, col, val, n, [&](const uint32_t* dc, const int32_t* dv) {
    return ctx_bsi_set_values(c, batch, nbits, min_v, max_v, dc, dv, n, out_id, out3);
  });
}

// A batch as the operand of the BSI read-outs (bsival.hip): key-major [ebM, nbits slices, foundSet?]
static int bsi_val_operand(Ctx* c, int32_t id, int nbits, int has_found, Batch** B, BsiValArgs* a) {
  CHK(get_batch(c, id, B));
  const Batch* b = *B;
  if (!b->key_major || b->packed || nbits < 0 || nbits + 2 > kBsiMaxInputs ||
      b->n_bm != (size_t)(1 + nbits + (has_found ? 1 : 0))) {
    set_err("bsi values: batch must hold ebM, nbits slices and the optional foundSet");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  *a = BsiValArgs{b->key_off.as<uint32_t>(), b->desc.as<CDesc>(), b->bm.as<uint32_t>(), b->payload.as<uint8_t>(), nbits};
  return RBG_OK;
}

// getValue (BSI/:181-196) of n columns (device memory, u32, any order, repeats allowed) into out (device
// memory, i64; -1: ebM lacks the column), in query order, enqueued on the context stream
static int ctx_bsi_get_values(Ctx* c, int32_t batch, int nbits, int has_found, const uint32_t* q_dev, size_t n,
                              long long* out_dev) {
  Batch* B;
  BsiValArgs a;
  CHK(bsi_val_operand(c, batch, nbits, has_found, &B, &a));
  launch_bsi_get_values(c->stream, a, q_dev, n, out_dev);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// the same from host memory: staged through the context's pinned buffer, results in out on return
static int ctx_bsi_get_values_host(Ctx* c, int32_t batch, int nbits, int has_found, const uint32_t* q, size_t n,
                                   int64_t* out) {
  CHK(pinned_ensure(c, 12 * n + 64));
  CHK(c->pt_q.ensure(4 * n));
  CHK(c->pt_out.ensure(8 * n));
  uint8_t* pin = reinterpret_cast<uint8_t*>(c->pinned);
  hipStream_t s = c->stream;
  HIPCHK(hipStreamSynchronize(s));  // nothing enqueued earlier still reads the staging buffer
  std::memcpy(pin + 8 * n, q, 4 * n);
  HIPCHK(hipMemcpyAsync(c->pt_q.p, pin + 8 * n, 4 * n, hipMemcpyHostToDevice, s));
  CHK(ctx_bsi_get_values(c, batch, nbits, has_found, c->pt_q.as<uint32_t>(), n, c->pt_out.as<long long>()));
  HIPCHK(hipMemcpyAsync(pin, c->pt_out.p, 8 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(out, pin, 8 * n);
  return RBG_OK;
}

// toPairList() (BBSI/:534-549): every column of ebM, ascending and unsigned, into cols_dev (u32, or i64
// with cols64) with its value in vals_dev (i32, or i64 with vals64), enqueued on the context stream.
// *n_out: the pairs, known here from ebM's cardinality; no buffers with n_out: the size alone.
static int ctx_bsi_to_pairs(Ctx* c, int32_t batch, int nbits, int has_found, bool cols64, bool vals64, void* cols_dev,
                            void* vals_dev, uint64_t* n_out) {
  Batch* B;
  BsiValArgs a;
  CHK(bsi_val_operand(c, batch, nbits, has_found, &B, &a));
  const uint64_t total = B->h_bm_card.empty() ? 0 : (uint64_t)B->h_bm_card[0];
  if (n_out) *n_out = total;
  if (!total || (!cols_dev && !vals_dev && n_out)) return RBG_OK;
  if (!cols_dev || !vals_dev) {
    set_err("bsi_to_pairs: no output buffer");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(c->bsiv_cards.ensure(8 * (kMaxKeys + 1)));
  CHK(c->bsiv_part.ensure(8 * (scan_parts(kMaxKeys) + 1)));
  uint64_t* cards = c->bsiv_cards.as<uint64_t>();
  launch_bsi_pair_cards(c->stream, a, cards);
  launch_exclusive_scan(c->stream, cards, cards, kMaxKeys, c->bsiv_part.as<uint64_t>(), cards + kMaxKeys);
  launch_bsi_pairs(c->stream, a, cards, cols64, vals64, cols_dev, vals_dev);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// the same into host memory: both arrays on the device first, then one copy each
static int ctx_bsi_to_pairs_host(Ctx* c, int32_t batch, int nbits, int has_found, bool cols64, bool vals64, void* cols,
                                 void* vals, uint64_t* n_out) {
  uint64_t total = 0;
  CHK(ctx_bsi_to_pairs(c, batch, nbits, has_found, cols64, vals64, nullptr, nullptr, &total));  // operand check, size
  if (n_out) *n_out = total;
  if (!total || (!cols && !vals && n_out)) return RBG_OK;
  if (!cols || !vals) {
    set_err("bsi_to_pairs: no output buffer");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const size_t cb = (cols64 ? 8 : 4) * (size_t)total, vb = (vals64 ? 8 : 4) * (size_t)total;
  DevBuf dc, dv;
  CHK(pool_take(c, dc, cb));
  CHK(pool_take(c, dv, vb));
  CHK(ctx_bsi_to_pairs(c, batch, nbits, has_found, cols64, vals64, dc.p, dv.p, nullptr));
  HIPCHK(hipMemcpyAsync(cols, dc.p, cb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(vals, dv.p, vb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  pool_put(c, dc);
  pool_put(c, dv);
  return RBG_OK;
}

// The shared front of the queries that walk ebM & fixed (fixed = the foundSet or ebM) in parallelExec's batches
// (BBSI/:99-136): ctx_bsi_in and ctx_bsi_transpose.
struct BsiFixed {
  Batch* B;
  BsiValArgs a;
  int64_t card;        // fixed.getCardinality(), an int
  int64_t ebm_card;
  int64_t batch_size;  // min(max(card / parallelism, parallelism), 65536) (Java int arithmetic)
  bool empty;          // fixed or ebM holds no column: the result is one empty bitmap
};

// the argument checks (op: the name in the messages) and the host's numbers
static int bsi_fixed_operand(Ctx* c, const char* op, int32_t batch, int nbits, int has_found, int parallelism,
                             BsiFixed* f) {
  if (parallelism < 1) {
    set_err(std::string(op) + ": parallelism must be positive");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (nbits < 0 || nbits > 32) {
    set_err(std::string(op) + ": an index holds at most 32 slices");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(bsi_val_operand(c, batch, nbits, has_found, &f->B, &f->a));
  const std::vector<int64_t>& cards = f->B->h_bm_card;
  const size_t fx = has_found ? (size_t)nbits + 1 : 0;
  f->card = cards.size() > fx ? cards[fx] : 0;
  if (f->card > INT32_MAX) {
    set_err(std::string(op) + ": the foundSet (or ebM) holds more than 2^31 - 1 columns");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  f->ebm_card = cards.empty() ? 0 : cards[0];
  f->empty = f->card == 0 || f->ebm_card == 0;
  f->batch_size = std::min<int64_t>(std::max<int64_t>(f->card / parallelism, parallelism), 65536);
  return RBG_OK;
}

// The candidate keys (those ebM and fixed share) into ckeys / ckoff with their count in scalar[0], which the
// caller has zeroed, and into bsiv_cards the exclusive scan of the keys' cardinalities in fixed: the rank in
// fixed of a key's first column.
static int bsi_fixed_keys(Ctx* c, const BsiFixed& f, int has_found, DevBuf& ckeys, DevBuf& ckoff) {
  CHK(ckeys.ensure(2 * kMaxKeys + 16));
  CHK(ckoff.ensure(4 * (kMaxKeys + 1)));
  CHK(c->bsiv_cards.ensure(8 * (kMaxKeys + 1)));
  CHK(c->bsiv_part.ensure(8 * (scan_parts(kMaxKeys) + 1)));
  uint64_t* rank = c->bsiv_cards.as<uint64_t>();
  launch_bsiin_keys(c->stream, f.a, has_found, c->flag.as<uint8_t>(), rank);
  launch_bld_keys(c->stream, nullptr, 0, c->flag.as<uint8_t>(), ckeys.as<uint16_t>(), ckoff.as<uint32_t>(),
                  c->scalar.as<unsigned long long>());
  launch_exclusive_scan(c->stream, rank, rank, kMaxKeys, c->bsiv_part.as<uint64_t>(), rank + kMaxKeys);
  return RBG_OK;
}

constexpr size_t kBsiInHostSort = 1024;  // ctx_bsi_in: longer value lists are sorted on the device

// BitSliceIndexBase.parallelIn(parallelism, foundSet, values, pool) (BBSI/:611-639) over the resident index
// [ebM, bA[0..nbits-1], foundSet?] as a new one-bitmap key-major batch: what ctx_load of the reference's
// result gives (bsiin.hip).  The set is {c in ebM & fixed : value(c) in values}, fixed = the foundSet or ebM;
// parallelism enters through parallelExec's batchSize (BBSI/:99-136) alone, which decides whether a full
// container is a bitmap or RunContainer.full().  values: n_values host ints in any order,
// repeats allowed; the device gets a sorted distinct copy.  An empty fixed, ebM or list: one empty bitmap.  Two
// read-backs: the candidate key count, then the plan's totals.  The K x 8 KiB workspace is a BsibPlan of
// one cell per key whose fill is the membership kernel.
static int ctx_bsi_in(Ctx* c, int32_t batch, int nbits, int has_found, const int32_t* values, size_t n_values,
                      int parallelism, int32_t* out_id) {
  hipStream_t s = c->stream;
  if (n_values > (size_t)INT32_MAX) {
    set_err("bsi_in: more than 2^31 - 1 values in the list");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  BsiFixed f;
  CHK(bsi_fixed_operand(c, "bsi_in", batch, nbits, has_found, parallelism, &f));
  if (f.empty || n_values == 0) return ctx_empty_bitmap(c, out_id);
  unsigned long long* sc = c->scalar.as<unsigned long long>();  // [0] K, [1] the distinct list entries
  // the list as 32-bit patterns (membership is their equality), ascending and distinct, in device memory: a
  // short one is sorted here, a long one on the device
  DevBuf dl;  // back to the pool at the end (freed on an error)
  size_t n_list = 0;
  CHK(pool_take(c, dl, 4 * n_values + 16));
  if (n_values <= kBsiInHostSort) {
    std::vector<uint32_t> list(n_values);
    std::memcpy(list.data(), values, 4 * n_values);
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    n_list = list.size();
    CHK(upload_words(c, dl.p, list.data(), n_list));
    HIPCHK(hipMemsetAsync(sc, 0, 64, s));
  } else {
    DevBuf scratch, temp;
    const size_t tb = bsiin_sort_temp_bytes(n_values);
    CHK(pool_take(c, scratch, 4 * n_values + 16));
    CHK(pool_take(c, temp, tb));
    CHK(upload_words(c, dl.p, values, n_values));
    HIPCHK(hipMemsetAsync(sc, 0, 64, s));
    HIPCHK((hipError_t)launch_bsiin_sort_unique(s, temp.p, tb, dl.as<uint32_t>(), scratch.as<uint32_t>(), sc + 1,
                                                n_values));
    pool_put(c, scratch);  // whatever takes them next is enqueued on this stream, after the sort
    pool_put(c, temp);
  }
  CHK(bsi_fixed_keys(c, f, has_found, c->bsib_pkeys, c->bsib_pkoff));
  HIPCHK(hipGetLastError());
  unsigned long long h[2] = {};
  HIPCHK(hipMemcpyAsync(h, sc, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (n_values > kBsiInHostSort) n_list = (size_t)h[1];
  const size_t K = (size_t)h[0];
  dbg(s, "bsi_in: keys");
  if (K == 0) {  // ebM and the foundSet share no key
    pool_put(c, dl);
    return ctx_empty_bitmap(c, out_id);
  }
  BsibPlan plan;
  CHK(plan.begin(c, K, 1, 0, false, true));
  auto fill = [&](size_t k_lo, size_t k_hi, bool) -> int {  // every cell of the pass is written: no memset
    launch_bsi_in(s, f.a, has_found, dl.as<uint32_t>(), (uint32_t)n_list, c->bsib_pkeys.as<uint16_t>(), (uint32_t)k_lo,
                  (uint32_t)k_hi, c->bsiv_cards.as<uint64_t>(), f.batch_size == 65536, plan.ws.as<uint8_t>(),
                  c->bsia_run.as<uint8_t>());
    return RBG_OK;
  };
  CHK(plan.sweep(true, fill));
  dbg(s, "bsi_in: in + plan");
  const int st = plan.emit(1, fill, "bsi_in: write", out_id);  // synchronises
  pool_put(c, dl);
  return st;
}

// The full result keys of a transpose that are RunContainer.full(): per key, over the batches
// of parallelExec that contribute a value to it in order, d_t distinct values in batch t and U_t in the union
// after it; a run container iff some t >= 2 has U_t == 65536 and d_t > 4096 (Container.ior's full union with
// a bitmap on the other side).  rank[] / val[]: (rank in fixed, value) of every column whose value lies in a
// full key, in any order; slot[value >> 16]: the key's index, or -1.
static void bsit_full_runs(const std::vector<uint32_t>& rank, const std::vector<uint32_t>& val, size_t n,
                           const std::vector<int32_t>& slot, uint64_t batch_size, std::vector<uint8_t>& run) {
  std::vector<std::vector<uint64_t>> per(run.size());  // batch << 16 | low half of the value
  for (size_t i = 0; i < n; i++) {
    const int32_t ki = slot[val[i] >> 16];
    if (ki >= 0) per[(size_t)ki].push_back(((uint64_t)rank[i] / batch_size) << 16 | (val[i] & 0xFFFFu));
  }
  std::vector<uint8_t> seen(65536);
  for (size_t ki = 0; ki < per.size(); ki++) {
    std::vector<uint64_t>& v = per[ki];
    if (v.empty()) continue;
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    std::fill(seen.begin(), seen.end(), 0);
    size_t uni = 0, t = 0;
    for (size_t i = 0; i < v.size();) {
      size_t j = i;
      while (j < v.size() && (v[j] >> 16) == (v[i] >> 16)) {
        if (!seen[v[j] & 0xFFFFu]) seen[v[j] & 0xFFFFu] = 1, uni++;
        j++;
      }
      t++;
      if (t >= 2 && uni == 65536 && j - i > 4096) run[ki] = 1;
      i = j;
    }
  }
}

// ctx_bsi_transpose: below this many columns per result key (an upper bound: min(card(ebM), card(fixed)) / K')
// the sort route runs.  Measured at 32 (the count tables lose 17 x) and at 16,384 (they win); not tuned between.
constexpr uint64_t kBsitSparse = 256;

// BitSliceIndexBase.parallelTransposeWithCount(foundSet, parallelism, pool) (BBSI/:551-597) over the resident
// index [ebM, bA[0..nbits-1], foundSet?] as a new key-major batch [ebM', bA'[0..nbits'-1]]: what ctx_load of
// the reference's result gives (bsitr.hip).  The result's columns are the distinct 32-bit values of the
// columns in ebM & fixed (fixed = the foundSet or ebM), its values their counts; out3 = {nbits', min, max}.
// parallelism enters through parallelExec's batchSize (BBSI/:99-136) alone, which decides whether a full
// result key is a bitmap or RunContainer.full().  No column of fixed in ebM: one empty bitmap,
// {0, 0, 0}.  Read-backs: the result key count, then the plan's totals with min / max and the number of full
// keys.  Per result key the workspace holds m = 1 + bitlen(min(card(ebM), card(fixed))) cells of 8 KiB (no
// count exceeds that many bits) and a count table of 256 KiB: a BsibPlan with the table as a key's extra bytes,
// whose fill counts and writes the cells.  Only when a key is full, batchSize > 4096 and fixed spans two batches: the
// values of the full keys are set in one bitmap per (full key, batch), a workgroup per full key applies the
// rule over its batches (above the byte budget: the (rank, value) pairs go to the host instead), and the plan
// runs again.
static int ctx_bsi_transpose(Ctx* c, int32_t batch, int nbits, int has_found, int parallelism, int32_t* out_id,
                             int32_t* out3) {
  hipStream_t s = c->stream;
  out3[0] = out3[1] = out3[2] = 0;
  BsiFixed f;
  CHK(bsi_fixed_operand(c, "bsi_transpose", batch, nbits, has_found, parallelism, &f));
  if (f.empty) return ctx_empty_bitmap(c, out_id);
  const BsiValArgs a = f.a;
  const int64_t card = f.card, ebm_card = f.ebm_card, batch_size = f.batch_size;
  const uint32_t grid = f.B->h_bm_nctr[0];  // the keys of ebM: every candidate key is one of them
  CHK(c->bsit_rflag.ensure(kMaxKeys));
  CHK(c->bsib_pkeys.ensure(2 * kMaxKeys + 16));
  CHK(c->bsib_pkoff.ensure(4 * (kMaxKeys + 1)));
  // [0] candidate keys, [1] K' result keys, [2] {min, max} as two u32, [3] full result keys, [4] pairs
  unsigned long long* sc = c->scalar.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(sc, 0, 64, s));
  HIPCHK(hipMemcpyAsync(sc + 2, kMinMaxSeedU32, 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(c->bsit_rflag.p, 0, kMaxKeys, s));
  CHK(bsi_fixed_keys(c, f, has_found, c->bsit_ckeys, c->bsit_ckoff));
  uint64_t* rank = c->bsiv_cards.as<uint64_t>();
  BsiTrSweep sw{};
  sw.rflag = c->bsit_rflag.as<uint8_t>();
  launch_bsitr_sweep(s, 0, a, has_found, c->bsit_ckeys.as<uint16_t>(), sc, grid, sw);
  launch_bld_keys(s, nullptr, 0, c->bsit_rflag.as<uint8_t>(), c->bsib_pkeys.as<uint16_t>(), c->bsib_pkoff.as<uint32_t>(),
                  sc + 1);
  HIPCHK(hipGetLastError());
  unsigned long long h[2] = {};
  HIPCHK(hipMemcpyAsync(h, sc, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  dbg(s, "bsi_transpose: keys");
  const size_t K = (size_t)h[1];  // result keys
  if (K == 0) return ctx_empty_bitmap(c, out_id);  // no column of fixed is in ebM
  const uint64_t most = (uint64_t)std::min<int64_t>(card, ebm_card);  // no count is larger
  // Sparse shapes (fewer than kBsitSparse columns per result key): a count table of 256 KiB per key would be
  // zeroed and read for a handful of counts, so the values are sorted and run-length encoded instead and the
  // (value, count) pairs go through the build, whose containers are typed by cardinality.  That is the
  // reference's answer whenever no run container can appear (batchSize <= 4096 or a single batch); a call
  // that could produce one keeps the count tables.  RBG_BSI_TR_ROUTE=count|sort (read at every call) forces
  // a route where it is exact.
  const bool no_run = batch_size <= 4096 || card <= batch_size;
  bool sparse = most < kBsitSparse * (uint64_t)K;
  if (const char* e = std::getenv("RBG_BSI_TR_ROUTE")) sparse = e[0] == 's' ? true : e[0] == 'c' ? false : sparse;
  if (sparse && no_run) {
    DevBuf dv, ds, du, dn, temp;
    const size_t tb = bsitr_sort_temp_bytes(most);
    CHK(pool_take(c, dv, 4 * most + 16));
    CHK(pool_take(c, ds, 4 * most + 16));
    CHK(pool_take(c, du, 4 * most + 16));
    CHK(pool_take(c, dn, 4 * most + 16));
    CHK(pool_take(c, temp, tb));
    BsiTrSweep p{};
    p.n_pairs = sc + 4;
    p.out_val = dv.as<uint32_t>();
    p.cap = most;
    launch_bsitr_sweep(s, 3, a, has_found, c->bsit_ckeys.as<uint16_t>(), sc, grid, p);
    HIPCHK(hipGetLastError());
    unsigned long long n = 0, runs = 0;
    HIPCHK(hipMemcpyAsync(&n, sc + 4, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    n = std::min<unsigned long long>(n, most);
    HIPCHK((hipError_t)launch_bsitr_sort_rle(s, temp.p, tb, dv.as<uint32_t>(), ds.as<uint32_t>(), du.as<uint32_t>(),
                                             dn.as<int32_t>(), sc + 5, n));
    HIPCHK(hipMemcpyAsync(&runs, sc + 5, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    dbg(s, "bsi_transpose: sort + run lengths");
    const int st = ctx_bsi_from_columns(c, du.as<uint32_t>(), dn.as<int32_t>(), (size_t)runs, false, out_id, out3);
    pool_put(c, dv);  // whatever takes them next is enqueued on this stream, after the build
    pool_put(c, ds);
    pool_put(c, du);
    pool_put(c, dn);
    pool_put(c, temp);
    return st;
  }
  const int m = 1 + (64 - __builtin_clzll(most));
  constexpr size_t kTab = 4 * 65536;  // a result key's count table: after the cells of a pass
  BsibPlan plan;
  CHK(plan.begin(c, K, m, kTab, false, true));
  CHK(c->bsit_kcard.ensure(4 * K + 16));
  CHK(c->bsit_full.ensure(K + 16));
  HIPCHK(hipMemsetAsync(c->bsia_run.p, 0, K, s));
  HIPCHK(hipMemsetAsync(c->bsit_kcard.p, 0, 4 * K, s));
  HIPCHK(hipMemsetAsync(c->bsit_full.p, 0, K, s));
  uint32_t* tab = reinterpret_cast<uint32_t*>(plan.ws.as<uint8_t>() + 8192 * (size_t)m * plan.P);
  sw.rkoff = c->bsib_pkoff.as<uint32_t>();
  sw.tab = tab;
  auto fill = [&](size_t k_lo, size_t k_hi, bool stats) -> int {  // every cell of the pass is written
    HIPCHK(hipMemsetAsync(tab, 0, kTab * (k_hi - k_lo), s));
    BsiTrSweep p = sw;
    p.k_lo = (uint32_t)k_lo;
    p.k_hi = (uint32_t)k_hi;
    launch_bsitr_sweep(s, 1, a, has_found, c->bsit_ckeys.as<uint16_t>(), sc, grid, p);
    launch_bsitr_cells(s, tab, (uint32_t)k_lo, (uint32_t)k_hi, m, plan.ws.as<uint8_t>(), stats,
                       reinterpret_cast<uint32_t*>(sc + 2), c->bsit_kcard.as<uint32_t>(), c->bsit_full.as<uint8_t>(),
                       sc + 3);
    return RBG_OK;
  };
  unsigned long long h3[2] = {};  // {min, max}, full keys: the first sweep's statistics
  auto read_h3 = [&]() -> int {
    HIPCHK(hipMemcpyAsync(h3, sc + 2, 16, hipMemcpyDeviceToHost, s));
    return RBG_OK;
  };
  CHK(plan.sweep(true, fill, read_h3));
  dbg(s, "bsi_transpose: count + plan");
  if (h3[1] && batch_size > 4096 && card > batch_size) {  // a full key fed by several batches of bitmap size
    const size_t n_full = (size_t)h3[1];
    const size_t n_batches = (size_t)((card + batch_size - 1) / batch_size);
    std::vector<uint8_t> isfull(K);
    HIPCHK(hipMemcpyAsync(isfull.data(), c->bsit_full.p, K, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_full * n_batches * 8192 <= bsib_budget()) {
      // on the device: a bitmap per (full key, batch), then a workgroup per full key over its batches
      std::vector<uint32_t> tbl(K + n_full, 0xFFFFFFFFu);  // fidx[K], then fki[n_full]
      size_t f = 0;
      for (size_t ki = 0; ki < K && f < n_full; ki++)
        if (isfull[ki]) tbl[ki] = (uint32_t)f, tbl[K + f++] = (uint32_t)ki;
      DevBuf dt, bits;
      CHK(pool_take(c, dt, 4 * tbl.size() + 16));
      CHK(pool_take(c, bits, n_full * n_batches * 8192));
      CHK(upload_words(c, dt.p, tbl.data(), tbl.size()));
      HIPCHK(hipMemsetAsync(bits.p, 0, n_full * n_batches * 8192, s));
      BsiTrSweep p = sw;
      p.rank = rank;
      p.fidx = dt.as<uint32_t>();
      p.bits = bits.as<uint32_t>();
      p.n_batches = (uint32_t)n_batches;
      p.batch_size = (uint32_t)batch_size;
      launch_bsitr_sweep(s, 4, a, has_found, c->bsit_ckeys.as<uint16_t>(), sc, grid, p);
      launch_bsitr_full_runs(s, bits.as<uint32_t>(), (uint32_t)f, (uint32_t)n_batches, dt.as<uint32_t>() + K,
                             c->bsia_run.as<uint8_t>());
      HIPCHK(hipGetLastError());
      pool_put(c, dt);  // whatever takes them next is enqueued on this stream, after the kernels
      pool_put(c, bits);
      CHK(plan.sweep(false, fill));  // a flagged key is a run container of one run: sizes and kinds again
      dbg(s, "bsi_transpose: full keys");
    } else {
      // the bitmaps exceed the budget: the (rank, value) pairs of the full keys go to the host
      const size_t cap = (size_t)most;
      DevBuf dr, dv;
      CHK(pool_take(c, dr, 4 * cap + 16));
      CHK(pool_take(c, dv, 4 * cap + 16));
      BsiTrSweep p = sw;
      p.isfull = c->bsit_full.as<uint8_t>();
      p.rank = rank;
      p.n_pairs = sc + 4;
      p.out_rank = dr.as<uint32_t>();
      p.out_val = dv.as<uint32_t>();
      p.cap = cap;
      launch_bsitr_sweep(s, 2, a, has_found, c->bsit_ckeys.as<uint16_t>(), sc, grid, p);
      HIPCHK(hipGetLastError());
      unsigned long long np = 0;
      std::vector<uint16_t> rkeys(K);
      std::vector<uint8_t> run(K, 0);
      HIPCHK(hipMemcpyAsync(&np, sc + 4, 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(rkeys.data(), c->bsib_pkeys.p, 2 * K, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      const size_t n = (size_t)std::min<unsigned long long>(np, cap);
      std::vector<uint32_t> hr(n), hv(n);
      if (n) {
        HIPCHK(hipMemcpyAsync(hr.data(), dr.p, 4 * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hv.data(), dv.p, 4 * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
      }
      pool_put(c, dr);
      pool_put(c, dv);
      std::vector<int32_t> slot(65536, -1);
      for (size_t ki = 0; ki < K; ki++)
        if (isfull[ki]) slot[rkeys[ki]] = (int32_t)ki;
      bsit_full_runs(hr, hv, n, slot, (uint64_t)batch_size, run);
      if (std::find(run.begin(), run.end(), (uint8_t)1) != run.end()) {
        CHK(pinned_ensure(c, K));
        std::memcpy(c->pinned, run.data(), K);
        HIPCHK(hipMemcpyAsync(c->bsia_run.p, c->pinned, K, hipMemcpyHostToDevice, s));
        CHK(plan.sweep(false, fill));  // the flagged keys are a run container of one run: sizes and kinds again
        dbg(s, "bsi_transpose: full keys (host)");
      }
    }
  }
  const uint32_t mn = (uint32_t)h3[0], mx = (uint32_t)(h3[0] >> 32);
  const int nb = mx ? 32 - __builtin_clz(mx) : 0;
  CHK(plan.emit(1 + nb, fill, "bsi_transpose: write", out_id));
  out3[0] = nb;
  out3[1] = (int32_t)mn;
  out3[2] = (int32_t)mx;
  return RBG_OK;
}

// compareUsingMinMax (BSI/:515-579): 0 = run the circuit, 1 = all, 2 = empty
static int bsi_minmax(int op, int32_t s, int32_t e, int32_t lo, int32_t hi) {
  switch (op) {
    case BSI_LT: return s > hi ? 1 : s <= lo ? 2 : 0;
    case BSI_LE: return s >= hi ? 1 : s < lo ? 2 : 0;
    case BSI_GT: return s < lo ? 1 : s >= hi ? 2 : 0;
    case BSI_GE: return s <= lo ? 1 : s > hi ? 2 : 0;
    case BSI_EQ:
      if (lo == hi && lo == s) return 1;
      return (s < lo || s > hi) ? 2 : 0;
    case BSI_NEQ:
      if (lo == hi) return lo == s ? 2 : 1;
      return 0;
    case BSI_RANGE:
      if (s <= lo && e >= hi) return 1;
      return (s > hi || e < lo) ? 2 : 0;
    default: return 0;
  }
}

// RoaringBitmapSliceIndex.compare (BSI/:482-513) and / or sum (BSI/:581-592) over a
// key-major batch [ebM, bA[0..nbits-1], foundSet?]; the result is materialised like a
// wide op's, the sums land in c->bsi_sums.
static int ctx_bsi(Ctx* c, int32_t id, int op, int nbits, int has_found, int32_t start, int32_t end,
                   int32_t min_value, int32_t max_value, int want_sum) {
  Batch* B;
  CHK(get_batch(c, id, &B));
  if (!B->key_major || B->packed || nbits < 0 || nbits + 2 > kBsiMaxInputs || B->n_bm != (size_t)(1 + nbits + (has_found ? 1 : 0)) ||
      op < 0 || op > BSI_SUM_ONLY || (op == BSI_SUM_ONLY && !has_found)) {
    set_err("bsi: batch must hold ebM, nbits slices and the optional foundSet; bad op");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  hipStream_t s = c->stream;
  CHK(c->bsi_sums.ensure(8 * kBsiSumAll));  // zeroed by the plan kernel
  c->bsi_nbits = nbits;
  int mode = op;
  if (op != BSI_SUM_ONLY) {
    const int mm = bsi_minmax(op, start, end, min_value, max_value);
    if (mm == 1) mode = BSI_ALL;
    if (mm == 2) mode = -1;  // empty result
  }
  const size_t ub = std::min<size_t>(kMaxKeys, std::max<size_t>(B->n_ctr, 1));
  OutCtx oc;
  CHK(prepare_output(c, ub, kStagedMax * ub + B->max_ser, &oc, op == BSI_SUM_ONLY));
  c->r().pending_src = {id};
  const uint32_t need = mode == -1 ? 0xFFFFFFFFu : (op == BSI_SUM_ONLY ? (uint32_t)(nbits + 1) : 0u);
  BsiScratch sc{};
  if (mode >= 0 && mode <= BSI_RANGE) {
    CHK(c->bsi_defer.ensure(4 * (ub + 1)));
    CHK(c->bsi_cnts.ensure((size_t)4 * 128 * 4 * ub));  // count rows (< 128) x 4 units
    CHK(c->bsi_kin.ensure((size_t)16 * 34 * ub));
    CHK(c->bsi_table.ensure((size_t)16 * 34 * ub));
    sc = BsiScratch{c->bsi_defer.as<uint32_t>(), c->bsi_cnts.as<int>(), c->bsi_kin.p, ub, c->bsi_table.p};
    if (!c->bsi_claims.p) {  // zeroed once here, then by k_bsi_types after every query that claims
      CHK(c->bsi_claims.ensure(4 * kBsiClaimWords));
      HIPCHK(hipMemsetAsync(c->bsi_claims.p, 0, 4 * kBsiClaimWords, s));
    }
    sc.claims = c->bsi_claims.as<unsigned int>();
  }
  WideArgs wa{};
  wa.desc = B->desc.as<CDesc>();
  wa.bm = B->bm.as<uint32_t>();
  wa.payload = B->payload.as<uint8_t>();
  c->mark(0);
  Task* tasks = c->r().tasks.as<Task>();
  uint32_t* nt = c->r().ntasks.as<uint32_t>();
  if (sc.defer && bsi_reg_path(mode, nbits)) {
    // The task list (keys where ebM has a container) and the input table depend on the batch
    // only: planned once per batch, kept with it (RoaringBitmapSliceIndex queries on one index,
    // BSI/:482-513, re-walk the same keys every time).
    if (!B->bsi_cached) {
      CHK(B->bsi_tasks.ensure(sizeof(Task) * kMaxKeys));
      CHK(B->bsi_nt.ensure(64));
      CHK(B->bsi_table.ensure((size_t)16 * 34 * ub));
      launch_plan_bsi(s, B->key_off.as<uint32_t>(), B->bm.as<uint32_t>(), need, c->by_key.as<Task>(),
                      c->flag.as<uint8_t>(), c->wg_count.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr);
      launch_compact(s, c->flag.as<uint8_t>(), c->by_key.as<Task>(), c->wg_count.as<uint32_t>(),
                     B->bsi_tasks.as<Task>(), B->bsi_nt.as<uint32_t>());
      launch_bsi_table(s, B->bsi_tasks.as<Task>(), B->bsi_nt.as<uint32_t>(), wa, B->bsi_table.p, ub);
      B->bsi_cached = true;
    }
    tasks = B->bsi_tasks.as<Task>();
    nt = B->bsi_nt.as<uint32_t>();
    sc.table = B->bsi_table.p;
    sc.table_ready = true;
    sc.zlb = c->zlb;
    sc.ztile = c->ztile;
    sc.zsums = c->bsi_sums.as<unsigned long long>();
    sc.nt_src = nt;
    sc.nt_dst = c->r().ntasks.as<uint32_t>();
  } else {
    launch_plan_bsi(s, B->key_off.as<uint32_t>(), B->bm.as<uint32_t>(), need, c->by_key.as<Task>(),
                    c->flag.as<uint8_t>(), c->wg_count.as<uint32_t>(), c->zlb, c->ztile,
                    c->bsi_sums.as<unsigned long long>(), sc.defer);
    launch_compact(s, c->flag.as<uint8_t>(), c->by_key.as<Task>(), c->wg_count.as<uint32_t>(), tasks, nt);
  }
  c->mark(1);
  BsiArgs p{mode < 0 ? BSI_EQ : mode, nbits, has_found, (uint32_t)start, (uint32_t)end};
  launch_bsi(s, grid_for(ub, 65536), tasks, nt, wa, p, oc, want_sum ? c->bsi_sums.as<unsigned long long>() : nullptr,
             sc.defer ? &sc : nullptr, want_sum ? c->bsi_sums_dst : nullptr);
  c->mark(2);
  if (op == BSI_SUM_ONLY) {
    c->r().last = 0;
  } else {
    defer_place(c);
  }
  c->mark(3);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// ---------------------------------------------------------------------------
// Buffer-package BSI: BitSliceIndexBase.compare (bsi/src/main/java/org/roaringbitmap/bsi/buffer/
// BitSliceIndexBase.java, BBSI/ below), bsi.hip's k_bsi_buf
// ---------------------------------------------------------------------------

// horizontal_or's chain order for owenGreatEqual (BBSI/:266, RB/buffer/BufferFastAggregation.java:187-235):
// the queue holds one container pointer per orInput bitmap (in orInputs order, top down,
// BBSI/:247-264); each walks the keys where its orInput has a container, ordered by key, then
// larger cardinality first (RB/buffer/MutableRoaringArray.java:476-481), ties in the heap's
// order.  The poll order of a key's pointers is that key's chain: ord[t * kOwenOrder] = n,
// then the n orInput indices.
static int owen_order(Ctx* c, int M, uint32_t nt) {
  hipStream_t s = c->stream;
  std::vector<uint32_t> keys(nt);
  std::vector<int32_t> tb((size_t)nt * 32 * 4);  // TB: kind, card, src, pad
  if (nt) {
    HIPCHK(hipMemcpyAsync(keys.data(), c->owen_keys.p, 4 * (size_t)nt, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(tb.data(), c->owen_tb.p, 16 * 32 * (size_t)nt, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  std::vector<std::vector<uint32_t>> lists(M);  // tasks (ascending keys) where orInput j has a container
  for (uint32_t t = 0; t < nt; t++)
    for (int j = 0; j < M; j++)
      if (tb[((size_t)t * 32 + j) * 4 + 1] > 0) lists[j].push_back(t);
  std::vector<uint8_t> ord((size_t)std::max<uint32_t>(nt, 1) * kOwenOrder, 0);
  auto ptr = [&](uint32_t j, uint32_t i) {
    const uint32_t t = lists[j][i];
    return HPtr{j, i, keys[t], (uint32_t)tb[((size_t)t * 32 + j) * 4 + 1], t};
  };
  auto push = [&](const HPtr& x) {
    uint8_t* o = ord.data() + (size_t)x.pos * kOwenOrder;
    o[1 + o[0]++] = (uint8_t)x.bm;
  };
  JHeap pq;
  for (int j = 0; j < M; j++)
    if (!lists[j].empty()) pq.add(ptr((uint32_t)j, 0));
  auto advance_add = [&](const HPtr& x) {
    if (x.i + 1 < lists[x.bm].size()) pq.add(ptr(x.bm, x.i + 1));
  };
  while (!pq.q.empty()) {
    const HPtr x1 = pq.poll();
    push(x1);
    if (pq.q.empty() || pq.q[0].key != x1.key) {
      advance_add(x1);
      continue;
    }
    const HPtr x2 = pq.poll();
    push(x2);
    while (!pq.q.empty() && pq.q[0].key == x1.key) {
      const HPtr x = pq.poll();
      push(x);
      if (x.i + 1 < lists[x.bm].size()) pq.add(ptr(x.bm, x.i + 1));
      else if (pq.q.empty()) break;
    }
    advance_add(x1);
    advance_add(x2);
  }
  CHK(c->owen_ord.ensure(ord.size()));
  HIPCHK(hipMemcpyAsync(c->owen_ord.p, ord.data(), ord.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));  // `ord` is a stack vector
  return RBG_OK;
}

// op: RBG_BSI_* (compare) or RBG_BSI_RANGE_NEQ_DIRECT; the batch is [ebM, bA[0..nbits-1], foundSet?].
// Synchronous: the big-run arena is checked after the op (with_big_runs).
static int ctx_bsi_buffer(Ctx* c, int32_t id, int op, int nbits, int has_found, int32_t start, int32_t end,
                          int32_t min_value, int32_t max_value) {
  Batch* B;
  CHK(get_batch(c, id, &B));
  if (!B->key_major || B->packed || nbits < 0 || nbits + 2 > kBsiMaxInputs ||
      B->n_bm != (size_t)(1 + nbits + (has_found ? 1 : 0)) || op < 0 || op > RBG_BSI_RANGE_NEQ_DIRECT) {
    set_err("bsi: batch must hold ebM, nbits slices and the optional foundSet; bad op");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  hipStream_t s = c->stream;
  // compareUsingMinMax (BBSI/:455-519, as the heap one) and the op's own dispatch (BBSI/:422-453)
  int mode, nb_eff = nbits, found_eff = has_found;
  if (op == RBG_BSI_RANGE_NEQ_DIRECT || op == BSI_NEQ) {
    const int mm = op == BSI_NEQ ? bsi_minmax(BSI_NEQ, start, end, min_value, max_value) : 0;
    if (mm) {
      mode = mm == 1 ? BSI_ALL : -1;
    } else {  // andNot(ebM, rangeEQ(foundSet, value)); rangeEQ checks compareUsingMinMax(EQ) itself
      const int em = bsi_minmax(BSI_EQ, start, 0, min_value, max_value);
      mode = BSI_NEQ;
      if (em == 2) {  // andNot(ebM, empty): ebM's clone
        mode = BSI_ALL;
        found_eff = 0;
      } else if (em == 1) {  // andNot(ebM, ebM.clone() or and(ebM, foundSet)): the chain without slices
        nb_eff = 0;
      }
    }
  } else {
    const int mm = bsi_minmax(op, start, end, min_value, max_value);
    mode = mm == 1 ? BSI_ALL : mm == 2 ? -1 : op;
  }
  // owenGreatEqual (BBSI/:245-264): beGtrThan = start - 1, leastSignifZero =
  // Long.numberOfTrailingZeros(~beGtrThan) (64 when start - 1 == -1: no orInput at all)
  uint32_t zeros = 0, ones = 0;
  if (mode == BSI_GE || mode == BSI_RANGE) {
    const int32_t b = (int32_t)((uint32_t)start - 1u);
    const uint32_t nbx = ~(uint32_t)b;
    const int lsz = nbx == 0 ? 64 : __builtin_ctz(nbx);
    for (int w = nbits - 1; w >= lsz; w--) {
      if ((((uint32_t)b >> w) & 1u) == 0) zeros |= 1u << w;
      else ones |= 1u << w;
    }
  }
  const int M = __builtin_popcount(zeros);
  const size_t ub = std::min<size_t>(kMaxKeys, std::max<size_t>(B->n_ctr, 1));
  return with_big_runs(c, true, "bsi", [&](const BigRuns& big) -> int {
    OutCtx oc;
    CHK(prepare_output(c, ub, kStagedMax * ub + B->max_ser + big.cap, &oc, false));
    c->r().pending_src = {id};
    const uint32_t need = mode == -1 ? 0xFFFFFFFFu : 0xFFFFFFFEu;  // every key of any input
    c->mark(0);
    launch_plan_bsi(s, B->key_off.as<uint32_t>(), B->bm.as<uint32_t>(), need, c->by_key.as<Task>(),
                    c->flag.as<uint8_t>(), c->wg_count.as<uint32_t>(), c->zlb, c->ztile, nullptr, nullptr);
    launch_compact(s, c->flag.as<uint8_t>(), c->by_key.as<Task>(), c->wg_count.as<uint32_t>(), c->r().tasks.as<Task>(),
                   c->r().ntasks.as<uint32_t>());
    c->mark(1);
    WideArgs wa{};
    wa.desc = B->desc.as<CDesc>();
    wa.bm = B->bm.as<uint32_t>();
    wa.payload = B->payload.as<uint8_t>();
    BsiArgs p{};
    p.op = mode < 0 ? BSI_EQ : mode;
    p.nbits = nb_eff;
    p.has_found = found_eff;
    p.pred0 = (uint32_t)start;
    p.pred1 = (uint32_t)end;
    p.buffer = 1;
    p.found_input = nbits + 1;
    p.owen_zeros = zeros;
    p.owen_ones = ones;
    p.big = big;
    const int grid = grid_for(ub, 65536);
    if (mode >= 0 && M >= 3) {  // the chain order needs horizontal_or's queue: every orInput's type first
      CHK(c->owen_tb.ensure((size_t)16 * 32 * ub));
      CHK(c->owen_keys.ensure(4 * ub));
      p.owen_tb = c->owen_tb.p;
      p.task_keys = c->owen_keys.as<uint32_t>();
      launch_bsi_owen_pre(s, grid, c->r().tasks.as<Task>(), c->r().ntasks.as<uint32_t>(), wa, p);
      HIPCHK(hipGetLastError());
      uint32_t nt = 0;
      HIPCHK(hipMemcpyAsync(&nt, c->r().ntasks.p, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      CHK(owen_order(c, M, nt));
      p.owen_order = c->owen_ord.as<uint8_t>();
    }
    if (mode >= 0) launch_bsi_buf(s, grid, c->r().tasks.as<Task>(), c->r().ntasks.as<uint32_t>(), wa, p, oc);
    return op_end(c);
  });
}

// (sum, count) of the last BSI call: k_bsi_sum_final's Java longs, read back
static int ctx_bsi_sums(Ctx* c, int64_t* out2) {
  if (!c->bsi_sums.p) {
    out2[0] = out2[1] = 0;
    return RBG_OK;
  }
  HIPCHK(hipMemcpyAsync(out2, c->bsi_sums.as<uint64_t>() + kBsiSumOut, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return RBG_OK;
}

// the batch [ebM, slices, foundSet?] of a one-shot BSI call
static int bsi_load(OneShot& os, const uint8_t* ebm, size_t ebm_len, const uint8_t* const* slices, const size_t* lens,
                    size_t nbits, const uint8_t* found, size_t found_len, int32_t* id) {
  if (!ebm || (nbits && (!slices || !lens)) || nbits + 2 > (size_t)kBsiMaxInputs) return RBG_ERR_ILLEGAL_ARGUMENT;
  std::vector<const uint8_t*> bufs{ebm};
  std::vector<size_t> ls{ebm_len};
  for (size_t i = 0; i < nbits; i++) {
    bufs.push_back(slices[i]);
    ls.push_back(lens[i]);
  }
  if (found) {
    bufs.push_back(found);
    ls.push_back(found_len);
  }
  return os.load(bufs.data(), ls.data(), bufs.size(), id);
}

// the tail of a one-shot builder: the batch it made joins the call's scope, its first n bitmaps are the answer
static int oneshot_fetch(OneShot& os, int32_t id, size_t n, rbg_buffer* outs) {
  os.adopt(id);
  return ctx_batch_fetch_range(os.c, id, 0, n, outs);
}

}  // namespace rbg

using namespace rbg;

extern "C" {

int rbg_ctx_bsi(rbg_ctx* ctx, int32_t batch, int op, int nbits, int has_found, int32_t start, int32_t end,
                int32_t min_value, int32_t max_value, int want_sum) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_bsi(c, batch, op, nbits, has_found, start, end, min_value, max_value, want_sum);
}
int rbg_ctx_bsi_sums(rbg_ctx* ctx, int64_t* out2) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out2) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_sums(c, out2);
}
int rbg_ctx_bsi_sums_target(rbg_ctx* ctx, void* dst2) {
  if (!ctx) return RBG_ERR_ILLEGAL_ARGUMENT;
  ctx->c.bsi_sums_dst = dst2;
  return RBG_OK;
}
int rbg_ctx_bsi_sums_device(rbg_ctx* ctx, void* dst2) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!dst2 || !c->bsi_sums.p) return RBG_ERR_ILLEGAL_ARGUMENT;
  launch_bsi_sums_out(c->stream, c->bsi_sums.as<unsigned long long>(), dst2);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}
int rbg_bsi_compare(int op, int32_t start, int32_t end, const uint8_t* ebm, size_t ebm_len,
                    const uint8_t* const* slices, const size_t* slice_lens, size_t nbits, int32_t min_value,
                    int32_t max_value, const uint8_t* found, size_t found_len, rbg_buffer* out) {
  if (!out || op < 0 || op > BSI_RANGE) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(bsi_load(os, ebm, ebm_len, slices, slice_lens, nbits, found, found_len, &id));
  CHK(ctx_bsi(c, id, op, (int)nbits, found ? 1 : 0, start, end, min_value, max_value, 0));
  return ctx_fetch(c, out);
}
int rbg_bsi_compare_buffer(int op, int32_t start, int32_t end, const uint8_t* ebm, size_t ebm_len,
                           const uint8_t* const* slices, const size_t* slice_lens, size_t nbits, int32_t min_value,
                           int32_t max_value, const uint8_t* found, size_t found_len, rbg_buffer* out) {
  if (!out || op < 0 || op > RBG_BSI_RANGE_NEQ_DIRECT) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(bsi_load(os, ebm, ebm_len, slices, slice_lens, nbits, found, found_len, &id));
  CHK(ctx_bsi_buffer(c, id, op, (int)nbits, found ? 1 : 0, start, end, min_value, max_value));
  return ctx_fetch(c, out);
}
int rbg_ctx_bsi_buffer(rbg_ctx* ctx, int32_t batch, int op, int nbits, int has_found, int32_t start, int32_t end,
                       int32_t min_value, int32_t max_value) {
  Ctx* c;
  CHK(session(ctx, &c));
  return ctx_bsi_buffer(c, batch, op, nbits, has_found, start, end, min_value, max_value);
}
int rbg_bsi_sum(const uint8_t* ebm, size_t ebm_len, const uint8_t* const* slices, const size_t* slice_lens,
                size_t nbits, const uint8_t* found, size_t found_len, int64_t* out2) {
  if (!out2) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (!found) {  // BSI/:582: null foundSet -> (0, 0)
    out2[0] = out2[1] = 0;
    return RBG_OK;
  }
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(bsi_load(os, ebm, ebm_len, slices, slice_lens, nbits, found, found_len, &id));
  CHK(ctx_bsi(c, id, BSI_SUM_ONLY, (int)nbits, 1, 0, 0, 0, 0, 1));
  return ctx_bsi_sums(c, out2);
}

/* ---- a BSI from (column, value) pairs (bsibuild.hip) and its values back (bsival.hip) ---- */

int rbg_ctx_bsi_from_columns(rbg_ctx* ctx, const uint32_t* columns, const int32_t* values, size_t n, int run_optimize,
                             int32_t* batch, int32_t* out3) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!batch || !out3 || (n && (!columns || !values))) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_from_columns_host(c, columns, values, n, run_optimize != 0, batch, out3);
}

int rbg_ctx_bsi_from_columns_device(rbg_ctx* ctx, const void* columns_dev, const void* values_dev, size_t n,
                                    int run_optimize, int32_t* batch, int32_t* out3) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!batch || !out3 || (n && (!columns_dev || !values_dev))) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_from_columns(c, reinterpret_cast<const uint32_t*>(columns_dev),
                              reinterpret_cast<const int32_t*>(values_dev), n, run_optimize != 0, batch, out3);
}

int rbg_ctx_bsi_get_values(rbg_ctx* ctx, int32_t batch, int nbits, int has_found, const uint32_t* columns, size_t n,
                           int64_t* out) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (nbits < 0 || (n && (!columns || !out))) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (n == 0) return RBG_OK;
  return ctx_bsi_get_values_host(c, batch, nbits, has_found, columns, n, out);
}

int rbg_ctx_bsi_get_values_device(rbg_ctx* ctx, int32_t batch, int nbits, int has_found, const void* columns_dev,
                                  size_t n, void* out_dev) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (nbits < 0 || (n && (!columns_dev || !out_dev))) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (n == 0) return RBG_OK;
  return ctx_bsi_get_values(c, batch, nbits, has_found, reinterpret_cast<const uint32_t*>(columns_dev), n,
                            reinterpret_cast<long long*>(out_dev));
}

int rbg_ctx_bsi_to_pairs(rbg_ctx* ctx, int32_t batch, int nbits, int has_found, int columns64, int values64,
                         void* columns_out, void* values_out, uint64_t* n_out) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (nbits < 0) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_to_pairs_host(c, batch, nbits, has_found, columns64 != 0, values64 != 0, columns_out, values_out,
                               n_out);
}

int rbg_ctx_bsi_to_pairs_device(rbg_ctx* ctx, int32_t batch, int nbits, int has_found, int columns64, int values64,
                                void* columns_dev, void* values_dev, uint64_t* n_out) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (nbits < 0) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_to_pairs(c, batch, nbits, has_found, columns64 != 0, values64 != 0, columns_dev, values_dev, n_out);
}

int rbg_bsi_from_columns(const uint32_t* columns, const int32_t* values, size_t n, int run_optimize, rbg_buffer* outs,
                         int32_t* out3) {
  if (!outs || !out3 || (n && (!columns || !values))) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(ctx_bsi_from_columns_host(c, columns, values, n, run_optimize != 0, &id, out3));
  return oneshot_fetch(os, id, 1 + (size_t)out3[0], outs);
}

int rbg_ctx_bsi_add(rbg_ctx* ctx, int32_t batch_a, int nbits_a, int32_t batch_b, int nbits_b, int32_t min_a,
                    int32_t max_a, int32_t* out_batch, int32_t* out3) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_batch || !out3) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_add(c, batch_a, nbits_a, batch_b, nbits_b, min_a, max_a, out_batch, out3);
}

int rbg_bsi_add(const uint8_t* ebm_a, size_t ebm_a_len, const uint8_t* const* slices_a, const size_t* lens_a, int na,
                int32_t min_a, int32_t max_a, const uint8_t* ebm_b, size_t ebm_b_len, const uint8_t* const* slices_b,
                const size_t* lens_b, int nb, rbg_buffer* outs, int32_t* out3) {
  if (!outs || !out3 || na < 0 || nb < 0 || na > 32 || nb > 32) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (!ebm_a || !ebm_b || (na && (!slices_a || !lens_a)) || (nb && (!slices_b || !lens_b))) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t ia, ib, id;
  CHK(bsi_load(os, ebm_a, ebm_a_len, slices_a, lens_a, (size_t)na, nullptr, 0, &ia));
  CHK(bsi_load(os, ebm_b, ebm_b_len, slices_b, lens_b, (size_t)nb, nullptr, 0, &ib));
  CHK(ctx_bsi_add(c, ia, na, ib, nb, min_a, max_a, &id, out3));
  return oneshot_fetch(os, id, 1 + (size_t)out3[0], outs);
}

/* ---- RoaringBitmapSliceIndex.setValues (BSI/:349-357; bsiset.hip) ---- */

int rbg_ctx_bsi_set_values(rbg_ctx* ctx, int32_t batch, int nbits, int32_t min_value, int32_t max_value,
                           const uint32_t* columns, const int32_t* values, size_t n, int32_t* out_batch, int32_t* out3) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_batch || !out3 || (n && (!columns || !values))) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_set_values_host(c, batch, nbits, min_value, max_value, columns, values, n, out_batch, out3);
}

int rbg_ctx_bsi_set_values_device(rbg_ctx* ctx, int32_t batch, int nbits, int32_t min_value, int32_t max_value,
                                  const void* columns_dev, const void* values_dev, size_t n, int32_t* out_batch,
                                  int32_t* out3) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_batch || !out3 || (n && (!columns_dev || !values_dev))) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_set_values(c, batch, nbits, min_value, max_value, reinterpret_cast<const uint32_t*>(columns_dev),
                            reinterpret_cast<const int32_t*>(values_dev), n, out_batch, out3);
}

int rbg_bsi_set_values(const uint8_t* ebm, size_t ebm_len, const uint8_t* const* slices, const size_t* slice_lens,
                       int nbits, int32_t min_value, int32_t max_value, const uint32_t* columns, const int32_t* values,
                       size_t n, rbg_buffer* outs, int32_t* out3) {
  if (!outs || !out3 || nbits < 0 || nbits > 32 || (n && (!columns || !values))) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (!ebm || (nbits && (!slices || !slice_lens))) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t ia, id;
  CHK(bsi_load(os, ebm, ebm_len, slices, slice_lens, (size_t)nbits, nullptr, 0, &ia));
  CHK(ctx_bsi_set_values_host(c, ia, nbits, min_value, max_value, columns, values, n, &id, out3));
  return oneshot_fetch(os, id, 1 + (size_t)out3[0], outs);
}

/* ---- BitSliceIndexBase.parallelIn (BBSI/:611-639; bsiin.hip) ---- */

int rbg_ctx_bsi_in(rbg_ctx* ctx, int32_t batch, int nbits, int has_found, const int32_t* values, size_t n_values,
                   int parallelism, int32_t* out_batch) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_batch || (n_values && !values)) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_in(c, batch, nbits, has_found != 0, values, n_values, parallelism, out_batch);
}

int rbg_bsi_in(const uint8_t* ebm, size_t ebm_len, const uint8_t* const* slices, const size_t* slice_lens, int nbits,
               const uint8_t* found, size_t found_len, const int32_t* values, size_t n_values, int parallelism,
               rbg_buffer* out) {
  if (!out || nbits < 0 || nbits > 32 || parallelism < 1 || (n_values && !values)) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (!ebm || (nbits && (!slices || !slice_lens))) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id, res;
  CHK(bsi_load(os, ebm, ebm_len, slices, slice_lens, (size_t)nbits, found, found_len, &id));
  CHK(ctx_bsi_in(c, id, nbits, found ? 1 : 0, values, n_values, parallelism, &res));
  return oneshot_fetch(os, res, 1, out);
}

/* ---- BitSliceIndexBase.parallelTransposeWithCount (BBSI/:551-597; bsitr.hip) ---- */

int rbg_ctx_bsi_transpose(rbg_ctx* ctx, int32_t batch, int nbits, int has_found, int parallelism, int32_t* out_batch,
                          int32_t* out3) {
  Ctx* c;
  CHK(session(ctx, &c));
  if (!out_batch || !out3) return RBG_ERR_ILLEGAL_ARGUMENT;
  return ctx_bsi_transpose(c, batch, nbits, has_found != 0, parallelism, out_batch, out3);
}

int rbg_bsi_transpose(const uint8_t* ebm, size_t ebm_len, const uint8_t* const* slices, const size_t* slice_lens,
                      int nbits, const uint8_t* found, size_t found_len, int parallelism, rbg_buffer* outs,
                      int32_t* out3) {
  if (!outs || !out3 || nbits < 0 || nbits > 32 || parallelism < 1) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (!ebm || (nbits && (!slices || !slice_lens))) return RBG_ERR_ILLEGAL_ARGUMENT;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id, res;
  CHK(bsi_load(os, ebm, ebm_len, slices, slice_lens, (size_t)nbits, found, found_len, &id));
  CHK(ctx_bsi_transpose(c, id, nbits, found ? 1 : 0, parallelism, &res, out3));
  return oneshot_fetch(os, res, 1 + (size_t)out3[0], outs);
}

int rbg_bsi_get_values(const uint8_t* ebm, size_t ebm_len, const uint8_t* const* slices, const size_t* slice_lens,
                       int nbits, const uint32_t* columns, size_t n, int64_t* out) {
  if (nbits < 0 || (n && (!columns || !out))) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (!ebm || (nbits && (!slices || !slice_lens)) || nbits + 2 > kBsiMaxInputs) return RBG_ERR_ILLEGAL_ARGUMENT;
  if (n == 0) return RBG_OK;
  OneShot os;
  CHK(os.open());
  Ctx* c = os.c;
  int32_t id;
  CHK(bsi_load(os, ebm, ebm_len, slices, slice_lens, (size_t)nbits, nullptr, 0, &id));
  return ctx_bsi_get_values_host(c, id, nbits, 0, columns, n, out);
}

}  // extern "C"
