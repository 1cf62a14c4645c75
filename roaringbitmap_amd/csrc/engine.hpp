// The one internal interface of the engine's host translation units: the macros, constants and types they
// share, and every function that one unit defines and another calls, grouped by the defining unit.
//   engine.cpp        the core: contexts and pools, batches, result output and fetch, pairwise and single-bitmap ops
//   engine_load.cpp   upload of serialized bitmaps and their decode on the device
//   engine_wide.cpp   the aggregations (FastAggregation's dispatch, the horizontal and priority-queue forms)
//   engine_bsi.cpp    every bit-sliced-index pipeline and its entry points
//   engine_rangebitmap.cpp  the range-encoded index: load, build from values, serialize, queries, counts
//   engine_mutate.cpp  batches of values added to or removed from a resident bitmap, and their entry points
//   engine_synth.cpp  the bench workload synthesizers
//   engine_api.cpp    the exported C ABI
// What is declared here is defined once; what no other unit calls stays static in its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/roaring_mi355x.h"
#include "kernels.hpp"

namespace rbg {

void set_err(const std::string& s);  // the calling thread's rbg_last_error text

#define HIPCHK(x)                                                            \
  do {                                                                       \
    hipError_t e_ = (x);                                                     \
    if (e_ != hipSuccess) {                                                  \
      set_err(std::string(#x) + " failed: " + hipGetErrorString(e_));        \
      return e_ == hipErrorOutOfMemory ? RBG_ERR_OUT_OF_MEMORY : RBG_ERR_DEVICE; \
    }                                                                        \
  } while (0)

#define CHK(x)              \
  do {                      \
    int st_ = (x);          \
    if (st_ != RBG_OK) return st_; \
  } while (0)

constexpr size_t kSlack = 256;  // every device buffer carries read slack (group_copy)
constexpr int kMaxKeys = 65536;
constexpr size_t kLbHeader = 256;  // look-back state: error @64, result card @96
// The largest serialized container a kernel stages in its scratch slot (a bitmap, 8192 B, or a run
// container of 2048 runs; kSlotBytes, device.hpp, is this rounded up).  Every op's payload bound counts
// on it: each result container is staged (<= kStagedMax B) or a clone of one input container.
constexpr size_t kStagedMax = 8194;
// tile statuses (kMaxTiles, device.hpp) follow the 65536 task statuses, tile cardinalities them

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      if (p) (void)hipFree(p);
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int ensure(size_t bytes);  // defined after Ctx: an out-of-memory allocation empties the contexts' pools
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

struct Batch {
  bool live = false;
  bool key_major = false;  // containers sorted by (key, input); else by (input, key)
  bool gapped = false;     // slots not back to back (runOptimize result: a hole after a shrunk container)
  bool packed = false;     // array payloads packed at 2 B granularity (C3 uniform synthetic
                           // batches): wide ops and fetches only
  size_t n_bm = 0, n_ctr = 0;
  DevBuf keys, desc, bm, key_off, bm_off, payload;
  size_t payload_bytes = 0;
  std::vector<uint32_t> h_bm_off;   // bitmap-major container ranges (n_bm + 1), or counts prefix
  std::vector<uint32_t> h_bm_nctr;  // containers per input bitmap
  std::vector<int64_t> h_bm_card;   // long cardinality per input bitmap
  int64_t n_kind[3] = {0, 0, 0};
  int64_t ser_bytes = 0;
  int64_t long_card = 0;
  size_t max_ser = 0;  // Σ serialized payload of containers larger than kStagedMax (long run inputs)
  int32_t bsi_min = 0, bsi_max = 0;  // synthetic C5: min / max of the indexed values
  bool pair_cap_known = false;        // batched andCardinality: item capacity computed
  // made by runOptimize: kinds / payload bytes / run flags still in ro_stats (device: 5 u64 totals,
  // plan partial counts, run flags: ro_flags_off) until ensure_stats derives them
  bool stats_pending = false;
  DevBuf ro_stats;
  size_t ro_groups = 0;  // plan workgroups whose partial counts ro_stats holds
  std::vector<uint8_t> h_has_run;
  // BSI compare over this batch (ebM = input 0): the task list (keys of ebM) and the per-key input
  // table, planned by the first query and kept (ctx_bsi)
  bool bsi_cached = false;
  DevBuf bsi_tasks, bsi_nt, bsi_table;
  // rank directory of a single-bitmap key-major batch (rankdir.hip): built on the device by the first
  // point query and kept (ctx_rankdir)
  bool rd_ready = false;
  DevBuf rd_cum, rd_off, rd_aux;
  uint64_t pair_items_cap = 0;
  // host copy of the container table for fetches (batches are immutable once loaded):
  // h_desc in container order, h_pos[h_pos_off[i] .. h_pos_off[i+1]) = bitmap i's containers
  bool h_index = false;
  bool h_chain_identity = false;  // horizontal_order found the batch order to be the chain order
  std::vector<CDesc> h_desc;
  std::vector<uint32_t> h_pos, h_pos_off;
};

// A resident range-encoded index (engine_rangebitmap.cpp; RB/RangeBitmap.java): not a batch, because its slices
// are not bitmaps of the portable format (a bitmap container of any cardinality, rangebitmap_format.hpp)
struct RangeIndex {
  uint32_t nslices = 0, n_blocks = 0;
  uint64_t max_rid = 0, mask = 0;
  uint64_t payload_bytes = 0;  // container payload bytes of the stream
  uint64_t arena_bytes = 0;    // the slots' bytes (the arena carries kSlack behind them)
  DevBuf dir, masks, arena;    // n_blocks x nslices CDesc, n_blocks u64, the containers' slots
};

struct DecBufs {  // scratch of the device decode (decode.hip), reused across loads
  DevBuf meta, head, nctr, base, nch, chbase, chmap, flag, err, card, cons, part, q, qkey, sort, skey, iota, perm,
      size, cpart;
};

// Everything prepare_output hands out to a materialising op and everything that describes the result until
// it is consumed, with the stream its kernels run on and the plan state of a pairwise op.  A context holds
// two: a pairwise op that finds the current set's serialization enqueued and not consumed takes the other
// set, on the other stream, so a stream of independent ops runs as two in-order lanes with no event between
// them.  Set 0 runs on the context's own stream.
struct ResultSet {
  hipStream_t stream = nullptr;
  DevBuf tasks;     // the op's task list: Task (wide) or PTask (pairwise) records
  DevBuf wg_epoch;  // pairwise plan: per-workgroup task counts tagged with the op epoch
  uint32_t epoch = 0;
  // look-back state: ticket @0, error word @64, result card @96, the task statuses @kLbHeader, then the tile
  // statuses, tile cardinalities and the pairwise tile sums
  DevBuf lb;
  DevBuf recs, scratch, result, kind_by_out, info, ntasks, task_card;
  size_t result_cap = 0;
  OutCtx pending{};         // output state of the set's materialising op
  std::vector<int32_t> pending_src;  // batches the pending result's pass-through records point into
  size_t pending_ub = 0;
  bool serialized = false;  // pending result already in the portable layout
  bool place_pending = false;  // the op's k_place not launched yet (serialization then places too)
  // the pending result's records were summed per tile by its compute kernel (OutCtx::tile_agg): its
  // serialization places and copies in one launch (k_serialize_agg) instead of k_place + k_serialize
  bool agg_ok = false;
  ResultInfo last_ri{};   // the pending result's facts, once ctx_info has read them (fetch_shard_device)
  bool ri_valid = false;
  int last = 0;  // 0 none, 1 serialized result, 2 cardinality, 3 batch cardinalities
  bool ready = false;  // the stream, the events and the fixed-size buffers exist (rs_alloc)
  bool in_flight = false;  // the result's serialization is enqueued on the set's stream and nothing consumed it yet
  // set 1 only.  touched: its stream was given work the context's stream has not waited for (join_set records
  // `done` behind it and makes the context's stream wait).  synced_seq: the value of Ctx::seq up to which its
  // stream has waited for the context's stream (lane_sync records `main_done` there)
  bool touched = false;
  uint64_t synced_seq = 0;
  hipEvent_t done = nullptr, main_done = nullptr;
};

struct Ctx {
  int device = 0;
  DecBufs dec;
  DevBuf pc_cnt, pc_part, pc_items, pc_large;  // batched andCardinality scratch
  hipStream_t stream = nullptr;  // the context's stream (the one callers see): everything but set 1's pairwise
                                 // ops and their serializations, and everything that reads a result
  ResultSet rs[2];               // rs[1] (with its stream) is made by the first op that finds rs[0] in flight
  int cur = 0;                   // the set of the last op: what serialize / fetch / statistics mean
  ResultSet& r() { return rs[cur]; }
  // counts the calls that may have given the context's stream work set 1's stream has to run behind: every
  // entry but a pairwise op's or a serialization's own, and every op that runs on the context's stream.
  // (Not an event recorded on every lane-1 op instead: the context's stream is also lane 0, so that wait
  // would put op N behind serialization N - 1 and undo the lanes.)  A new entry point counts unless it only
  // calls ctx_pairwise / ctx_serialize; whatever gives the context's stream work inside an uncounted entry
  // bumps seq itself (main_set, ctx_serialize(on_main)).
  uint64_t seq = 1;
  std::vector<std::unique_ptr<Batch>> batches;
  std::vector<std::unique_ptr<RangeIndex>> range_indexes;  // by index id; a released one is null
  uint64_t* zlb = nullptr;    // look-back state the next plan kernel zeroes (null: none)
  uint64_t* ztile = nullptr;
  DevBuf bsi_defer, bsi_cnts, bsi_kin, bsi_table;  // scratch of the register-resident BSI kernels
  DevBuf bsi_claims;  // k_bsi_reg's unit-pool counters (zero between queries)
  DevBuf bsi_sums;  // kBsiMaxInputs + 1 u64: per-slice |bA[x] & found|, found count
  void* bsi_sums_dst = nullptr;  // rbg_ctx_bsi_sums_target: (sum, count) also written here by every sum
  // buffer-package BSI: owenGreatEqual's orInput types / task keys / chain order, and the arena of
  // result run containers above 2047 runs (BigRuns; big_ctl = {bytes used, overflow})
  DevBuf owen_tb, owen_keys, owen_ord, big, big_ctl;
  DevBuf ones;  // 8192 bytes of 0xFF: the full bitmap container of an in-place OR (k_ior_fix)
  DevBuf ornot_plan;  // OrNotPlan of the last orNot
  DevBuf rd_part;         // scan scratch of the rank directory build
  DevBuf pt_q, pt_out;    // point queries from host memory: the queries and results on the device
  DevBuf bld_info, bld_size, bld_part;  // construction from values (build.hip): the plan's table, slot sizes, scan
  DevBuf tv_out;                        // expansion to host memory: one window of values on the device
  // a BSI batch from (column, value) pairs (bsibuild.hip): the present keys and their CSR, the plan's cell
  // table, the cells' size words (scanned in place) and scan scratch, the per-input totals
  DevBuf bsib_pkeys, bsib_pkoff, bsib_info, bsib_size, bsib_part, bsib_per;
  DevBuf rbb_info, rbb_size, rbb_part;  // a range-encoded index from values (rangebitmap_build.hip): the plan's cell
                                        // table, the cells' slot sizes (scanned in place), scan scratch
  // values added to or removed from a resident bitmap (mutate.hip): the second key scan's flags, both scans' keys
  // and CSRs, the counters, per cell was_run and the old cardinality, the plan's table, the size words (scanned
  // in place) and scan scratch
  DevBuf mut_flag, mut_keys, mut_off, mut_sc, mut_run, mut_card, mut_info, mut_size, mut_part;
  DevBuf bsia_run;  // the sum of two indexes (bsiadd.hip): per present key, ebM' is a full run container
  // parallelTransposeWithCount (bsitr.hip): the candidate input keys and their CSR, the result-key flags, per
  // result key its distinct values and whether it is full
  DevBuf bsit_ckeys, bsit_ckoff, bsit_rflag, bsit_kcard, bsit_full;
  DevBuf bsiv_cards, bsiv_part;  // toPairList (bsival.hip): ebM's cardinality per key (scanned in place)
  DevBuf gather_items, gather_out;  // batch fetch: slot gather list and download buffer
  DevBuf order;                     // horizontal_*: chain order of every key segment
  DevBuf ro_info, ro_size, ro_part;  // range selection scratch (kept: no allocation per call)
  DevBuf rs_card, rs_keep, rs_bm;
  // device buffers of released batches kept for the next batch of a similar size (hipMalloc /
  // hipFree of a 0.36 GB payload cost more than runOptimize's kernels); bounded by kPoolMax
  std::vector<DevBuf> pool;
  size_t pool_bytes = 0;
  std::mutex pool_mu;  // the pool may be emptied by another thread's out-of-memory allocation
  int bsi_nbits = 0;
  DevBuf by_key, flag, wg_count, cards, skip, raw, scalar;
  size_t n_cards = 0;
  void* pinned = nullptr;
  size_t pinned_cap = 0;
  // HIP-event phase timing: 4 events per op (start, after plan+compact, after
  // compute, after finalize+emit); read back without per-op host syncs.
  std::vector<hipEvent_t> prof_ev;
  size_t prof_cap = 0, prof_n = 0;
  DevBuf rd_ctr;  // while profiling: bytes the early-exit workShyAnd kernels read (rbg_ctx_profile_bytes)
  void prof_free() {
    for (hipEvent_t e : prof_ev) (void)hipEventDestroy(e);
    prof_ev.clear();
    prof_cap = prof_n = 0;
  }
  bool prof_compute_only = false;  // events around the compute launch only (rbg_ctx_profile_compute)
  void mark(int phase) {
    if (prof_compute_only && (phase == 0 || phase == 3)) {
      if (phase == 3 && prof_n < prof_cap) prof_n++;  // the op's record is complete
      return;
    }
    if (prof_n < prof_cap) (void)hipEventRecord(prof_ev[4 * prof_n + phase], r().stream);  // the op's stream
    if (phase == 3 && prof_n < prof_cap) prof_n++;
  }
  ~Ctx();
};

// drops the listed batches on scope exit
struct BatchGuard {
  Ctx* c;
  std::vector<int32_t> ids;
  ~BatchGuard() {
    for (int32_t id : ids)
      if (id >= 0 && (size_t)id < c->batches.size()) c->batches[id].reset();
  }
};

static inline uint64_t round16(uint64_t x) { return (x + 15) & ~15ULL; }

// engine.cpp, contexts, pools and batches.
void dbg(hipStream_t s, const char* what);
int ctx_init(Ctx* c, int device);
int enter(Ctx* c, bool counts = true);
int tl_ctx(Ctx** out);
int find_batch(Ctx* c, int32_t id, Batch** out);
int get_batch(Ctx* c, int32_t id, Batch** out);
int32_t new_batch(Ctx* c);
int batch_host_index(Ctx* c, Batch* b);
void pool_put(Ctx* c, DevBuf& b);
int pool_take(Ctx* c, DevBuf& dst, size_t bytes);
size_t pool_clear(Ctx* c);
int pinned_ensure(Ctx* c, size_t bytes);
int upload_words(Ctx* c, void* dst, const void* src, size_t n);
int ctx_profile(Ctx* c, int max_ops, bool compute_only);
// engine.cpp, the output of an op: its bracket, placement, serialization, the result's facts and bytes.
// lanes: the op may take the other set and its stream (the pairwise ops alone; OutCtx and the plan state are
// then the set's own and its kernels go to c->r().stream)
int prepare_output(Ctx* c, size_t max_tasks, size_t max_payload, OutCtx* oc, bool card_only, bool lanes = false);
void defer_place(Ctx* c);
int ensure_placed(Ctx* c);
int grid_for(size_t tasks, size_t cap = 4096);
int op_end(Ctx* c);
// on_main: the caller consumes the result at once (a fetch) or needs the context stream's own order (an
// operand's release): the serialization is enqueued on the context's stream, behind a join
int ctx_serialize(Ctx* c, bool on_main = false);
// The context's stream waits for what the current set's stream holds (join_result) or both sets' (join_all):
// before anything reads or changes a result, before an operand's buffers go to the pool, and before an op
// that runs on the context's stream (main_set: join_all, then set 0 is the current one).  Nothing on set
// 1's stream since the last join: no call into the runtime.
int join_result(Ctx* c);
int join_all(Ctx* c);
int main_set(Ctx* c);
int sync_streams(Ctx* c);  // the host waits for both streams
int ctx_info(Ctx* c, ResultInfo* ri);
uint8_t* out_alloc(size_t n);
int ctx_fetch(Ctx* c, rbg_buffer* out);
int ctx_batch_fetch_range(Ctx* c, int32_t batch, size_t i0, size_t i1, rbg_buffer* outs);
int ctx_fetch_shard_device(Ctx* c, int64_t total_containers, int has_run, int64_t payload_base, void* desc_dst,
                           void* offsets_dst, void* runflag_dst, void* payload_dst);
// engine.cpp, the ops.
// One operand of a per-key op: bitmap i of a single-bitmap key-major slot-aligned batch, and that batch
struct Operand : BmView {
  Batch* b;
};
int resolve(Ctx* c, int32_t id, size_t i, Operand* op);
int ctx_empty_bitmap(Ctx* c, int32_t* out_id);
int ctx_point(Ctx* c, int op, int32_t batch, size_t i, const uint32_t* q_dev, size_t n, long long* out_dev);
int ctx_point_host(Ctx* c, int op, int32_t batch, size_t i, const uint32_t* q, size_t n, int64_t* out);
int ctx_to_values(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t count, bool out64, void* out_dev,
                  uint64_t* n_out);
int ctx_to_values_host(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t count, uint32_t* out,
                       uint64_t* n_out);
int ctx_from_values(Ctx* c, const uint32_t* v_dev, size_t n, bool run_opt, int32_t* out_id);
int ctx_from_values_host(Ctx* c, const uint32_t* v, size_t n, bool run_opt, int32_t* out_id);
int check_bitset_build(const void* bits, uint64_t n, int layout, bool device);
int check_bitset_window(uint64_t first, uint64_t n, int layout);
int ctx_from_bitset(Ctx* c, const void* bits_dev, uint64_t n, int layout, bool run_opt, int32_t* out_id);
int ctx_from_bitset_host(Ctx* c, const void* bits, uint64_t n, int layout, bool run_opt, int32_t* out_id);
int ctx_to_bitset(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout, void* out_dev);
int ctx_to_bitset_host(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout, void* out);
int ctx_pairwise(Ctx* c, int op, int32_t ia, size_t ma, int32_t ib, size_t mb, bool card_only, int key_lo = 0,
                 int key_hi = kMaxKeys, bool lanes = true);
int ctx_ornot(Ctx* c, int32_t ia, size_t ma, int32_t ib, size_t mb, int64_t range_end, int flags);
int check_range(int64_t start, int64_t end);
int ctx_range_mut(Ctx* c, int op, int32_t ia, size_t ma, int64_t start, int64_t end, bool buf);
int ctx_remove_run_compression(Ctx* c, int32_t ia, size_t ma);
int ctx_limit(Ctx* c, int32_t ia, size_t ma, int cut_key, int leftover);
int ctx_add_offset(Ctx* c, int32_t ia, size_t ma, int64_t offset);
int ctx_batch_card(Ctx* c, int32_t id);
int ctx_run_optimize(Ctx* c, int32_t id, int32_t* out_id, uint8_t* answers);
int ctx_select_range(Ctx* c, int32_t id, int64_t start, int64_t end, int32_t* out_id, bool buf = false);
// engine_load.cpp.
int ctx_load_impl(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n, bool key_major, int32_t* out_id,
                  bool pack_arrays = false);
int ctx_load(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* out_id,
             bool pack_arrays = false);
int ctx_load_separate(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* ids);
// engine_wide.cpp.  host_card_out / host_card_valid: a cardinality the host knows without a launch; null unless
// card_only.
bool wide_reads_packed(int op, size_t n);
int ctx_wide(Ctx* c, int op, int32_t id, int key_lo, int key_hi, const int32_t* ids, bool card_only,
             int* host_card_out, bool* host_card_valid, int32_t start_override = -1);
// engine_rangebitmap.cpp: the range-encoded index (RB/RangeBitmap.java).  ctx_batch < 0: no context.
int check_rb_query(int op, bool has_ctx, bool count);
int ctx_rb_load(Ctx* c, const uint8_t* buf, size_t len, int32_t* out_index);
int check_rb_build(const void* values, uint64_t n, const void* out);
int ctx_rb_build(Ctx* c, const uint64_t* dev_values, uint64_t n, uint64_t max_value, bool max_from_data, int32_t* index);
int ctx_rb_build_host(Ctx* c, const uint64_t* values, uint64_t n, uint64_t max_value, bool max_from_data,
                      int32_t* index);
int ctx_rb_serialize(Ctx* c, int32_t index, rbg_buffer* out);
int ctx_rb_release(Ctx* c, int32_t index);
int ctx_rb_info(Ctx* c, int32_t index, uint64_t* info);
int ctx_rb_query(Ctx* c, int32_t index, int op, uint64_t a, uint64_t b, int32_t ctx_batch, size_t ctx_i,
                 int32_t* out_batch);
int ctx_rb_count(Ctx* c, int32_t index, int op, uint64_t a, uint64_t b, int32_t ctx_batch, size_t ctx_i, int64_t* out);
// engine_synth.cpp.
int synth_c2(Ctx* c, int kind, uint64_t seed, int32_t* out_id);
int synth_c3(Ctx* c, int kind, uint64_t seed, size_t n, int key_lo, int key_hi, int32_t* out_id);
int synth_c4(Ctx* c, uint64_t seed, size_t n_pairs, int32_t* out_id);
int synth_c5(Ctx* c, uint64_t seed, size_t rows, int key_lo, int key_hi, int32_t* out_id);

// a malloc'd copy of n bytes as a result buffer (rbg_free releases it); static like with_big_runs below: the
// core's batch fetch and the entry points each inline it
static int emit_bytes(const uint8_t* src, size_t n, rbg_buffer* out) {
  uint8_t* p = (uint8_t*)std::malloc(n ? n : 1);
  if (!p) return RBG_ERR_OUT_OF_MEMORY;
  if (n) std::memcpy(p, src, n);
  out->data = p;
  out->len = n;
  return RBG_OK;
}
static int emit_host(const std::vector<uint8_t>& v, rbg_buffer* out) { return emit_bytes(v.data(), v.size(), out); }

// An op whose kernel may keep run containers above 2047 runs reserves them in the context's big-run
// arena (Ctx::big; big_ctl = {bytes reserved, overflow flag}).  pass(BigRuns) enqueues one complete
// attempt, its prepare_output included (the payload bound counts big.cap).  The arena is checked after
// the pass (a synchronisation); a pass that overflowed counted every reservation, so the arena is grown
// to that size and the pass run once more.  use_arena false: the pass runs once with no arena, nothing
// is read back.
template <class Pass>
static int with_big_runs(Ctx* c, bool use_arena, const char* what, Pass&& pass) {
  if (!use_arena) return pass(BigRuns{nullptr, nullptr, 0});
  CHK(main_set(c));  // a serialization in flight may read records in the arena this op rewrites
  if (!c->big_ctl.p) CHK(c->big_ctl.ensure(16));
  if (!c->big.p) CHK(c->big.ensure(16ull << 20));
  for (int attempt = 0;; attempt++) {
    HIPCHK(hipMemsetAsync(c->big_ctl.p, 0, 16, c->stream));
    CHK(pass(BigRuns{c->big.as<uint8_t>(), c->big_ctl.as<unsigned long long>(), c->big.cap}));
    unsigned long long used[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(used, c->big_ctl.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!used[1]) return RBG_OK;
    if (attempt) {
      set_err(std::string(what) + ": the run-container arena overflowed twice");
      return RBG_ERR_DEVICE;
    }
    CHK(c->big.ensure(used[0] + (used[0] >> 3) + 4096));
  }
}

// The replay of java.util.PriorityQueue over container pointers: horizontal_order (engine_wide.cpp) and owen_order
// (engine_bsi.cpp).
namespace {
struct HPtr {
  uint32_t bm, i, key, card, pos;
};
static int hcmp(const HPtr& x, const HPtr& y) {  // ContainerPointer.compareTo
  if (x.key != y.key) return (int)x.key - (int)y.key;
  return (int)y.card - (int)x.card;
}
struct JHeap {  // java.util.PriorityQueue siftUp / siftDown (OpenJDK)
  std::vector<HPtr> q;
  void add(const HPtr& x) {
    size_t k = q.size();
    q.push_back(x);
    while (k > 0) {
      const size_t p = (k - 1) >> 1;
      if (hcmp(x, q[p]) >= 0) break;
      q[k] = q[p];
      k = p;
    }
    q[k] = x;
  }
  HPtr poll() {
    const HPtr r = q[0];
    const HPtr x = q.back();
    q.pop_back();
    const size_t n = q.size();
    if (n) {
      size_t k = 0;
      const size_t half = n >> 1;
      while (k < half) {
        size_t ch = 2 * k + 1;
        if (ch + 1 < n && hcmp(q[ch], q[ch + 1]) > 0) ch++;
        if (hcmp(x, q[ch]) <= 0) break;
        q[k] = q[ch];
        k = ch;
      }
      q[k] = x;
    }
    return r;
  }
};
}  // namespace

// Scope of a one-shot call: the calling thread's context and the batches the call made, dropped on
// exit.  load / load_separate register their batches before they return, adopt those an op made.
struct OneShot {
  Ctx* c = nullptr;
  BatchGuard g{nullptr, {}};
  int open() {
    CHK(tl_ctx(&c));
    g.c = c;
    return RBG_OK;
  }
  void adopt(int32_t id) { g.ids.push_back(id); }
  int load(const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* id, bool pack_arrays = false,
           bool key_major = true) {
    CHK(ctx_load_impl(c, bufs, lens, n, key_major, id, pack_arrays));
    adopt(*id);
    return RBG_OK;
  }
  int load_separate(const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* ids) {
    CHK(ctx_load_separate(c, bufs, lens, n, ids));
    g.ids.insert(g.ids.end(), ids, ids + n);
    return RBG_OK;
  }
};

}  // namespace rbg

// (hidden: a std:: template the compiler instantiates over the handle, unique_ptr<rbg_ctx>'s destructor, stays
// out of the library's dynamic symbols, whichever unit it lands in)
struct __attribute__((visibility("hidden"))) rbg_ctx {
  rbg::Ctx c;
};

namespace rbg {
// engine_api.cpp.  Entry of a session call: a null handle is an illegal argument; else the context, entered
int session(rbg_ctx* ctx, Ctx** c, bool counts = true);
}  // namespace rbg
