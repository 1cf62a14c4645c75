// Host side of the MI355X Roaring engine, the core unit: device contexts and their buffer pools, batch
// bookkeeping and statistics, result output (prepare_output, placement, serialization, fetch and its buffer
// cache), the rank directory, point queries and to / from values, the pairwise ops and the single-bitmap ops
// (orNot, range mutations, limit, addOffset, runOptimize, range selection), batched andCardinality, profiling and
// the thread-local one-shot context.  The other host units, all behind engine.hpp:
//   engine_load.cpp   upload of serialized bitmaps and their decode on the device (decode.hip)
//   engine_wide.cpp   the aggregations: FastAggregation's dispatch, the horizontal and priority-queue forms
//   engine_bsi.cpp    every bit-sliced-index pipeline and its entry points
//   engine_synth.cpp  the bench workload synthesizers (C2 .. C5)
//   engine_api.cpp    the exported C ABI of include/roaring_mi355x.h
// Process-wide state (the error text, the context list, the device mask, the output-buffer cache) lives here
// alone; the five entry points that are nothing but accessors of it are at the end of this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <chrono>
#include <unordered_map>
#include <vector>

#include <sys/mman.h>

#include "engine.hpp"
#include "format.hpp"

namespace rbg {

static thread_local std::string g_err;
void set_err(const std::string& s) { g_err = s; }

// RBG_DEBUG_SYNC=1: synchronise and report after every pipeline stage (debugging aid)
static bool debug_sync() {
  static int v = -1;
  if (v < 0) {
    const char* e = std::getenv("RBG_DEBUG_SYNC");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}
void dbg(hipStream_t s, const char* what) {
  if (!debug_sync()) return;
  static auto last = std::chrono::steady_clock::now();
  hipError_t e = hipStreamSynchronize(s);
  const auto now = std::chrono::steady_clock::now();
  std::fprintf(stderr, "[rbg] %s done: %s (+%.3f ms)\n", what, hipGetErrorString(e),
               std::chrono::duration<double, std::milli>(now - last).count());
  last = now;
  std::fflush(stderr);
}

// runOptimize's device statistics (Batch::ro_stats): from byte 64 the k_runopt workgroups' partial
// counts (4 u64 each), from ro_flags_off(groups) the per-bitmap run flags, computed only when the host
// asks (ensure_stats).
static size_t ro_flags_off(size_t groups) { return (64 + 32 * groups + 255) & ~(size_t)255; }

// every live context, for release_pools_on
static std::mutex g_ctx_mu;
static std::vector<Ctx*> g_ctxs;

Ctx::~Ctx() {
  {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), this), g_ctxs.end());
  }
  prof_free();
  if (rs[1].stream) {  // both streams drained before anything they use goes
    (void)hipStreamSynchronize(rs[1].stream);
    if (stream) (void)hipStreamSynchronize(stream);
  }
  if (pinned) (void)hipHostFree(pinned);
  batches.clear();
  if (rs[1].done) (void)hipEventDestroy(rs[1].done);
  if (rs[1].main_done) (void)hipEventDestroy(rs[1].main_done);
  if (rs[1].stream) (void)hipStreamDestroy(rs[1].stream);
  if (stream) (void)hipStreamDestroy(stream);
}

size_t pool_clear(Ctx* c) {
  std::lock_guard<std::mutex> g(c->pool_mu);
  const size_t n = c->pool.size();
  c->pool.clear();
  c->pool_bytes = 0;
  return n;
}

// the context the calling thread works on (set by tl_ctx / enter), for release_pools_on's first stage
static thread_local Ctx* t_cur_ctx = nullptr;
static std::atomic<uint64_t> g_pool_evictions{0};

static size_t release_pools_on(int device, int stage) {
  std::lock_guard<std::mutex> g(g_ctx_mu);
  size_t n = 0;
  const bool own = t_cur_ctx && std::find(g_ctxs.begin(), g_ctxs.end(), t_cur_ctx) != g_ctxs.end();
  if (stage == 0) {
    if (own && t_cur_ctx->device == device) n = pool_clear(t_cur_ctx);
  } else {
    for (Ctx* c : g_ctxs)
      if (c->device == device && !(own && c == t_cur_ctx)) n += pool_clear(c);
  }
  g_pool_evictions += n;
  return n;
}

// On an out-of-memory hipMalloc, the device buffers kept for reuse (Ctx::pool) are freed and the
// allocation retried: first the pool of the context the calling thread works on, then, if that was
// not enough, those of every other context on the device (release_pools_on).  Every pooled buffer
// freed this way is counted (rbg_pool_evictions), so memory pressure shows.
int DevBuf::ensure(size_t bytes) {
  if (cap >= bytes && p) return RBG_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  hipError_t e = hipMalloc(&p, bytes + kSlack);
  if (e == hipErrorOutOfMemory) {
    int dev = 0;
    (void)hipGetLastError();
    for (int stage = 0; stage < 2 && e == hipErrorOutOfMemory; stage++) {
      if (hipGetDevice(&dev) != hipSuccess) break;
      if (release_pools_on(dev, stage) > 0) {
        e = hipMalloc(&p, bytes + kSlack);
        if (e == hipErrorOutOfMemory) (void)hipGetLastError();
      }
    }
  }
  if (e != hipSuccess) {
    p = nullptr;
    set_err(std::string("hipMalloc(") + std::to_string(bytes) + ") failed: " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RBG_ERR_OUT_OF_MEMORY : RBG_ERR_DEVICE;
  }
  cap = bytes;
  return RBG_OK;
}

// entry of a session call: the context's device, and the context out-of-memory retries empty first
int enter(Ctx* c, bool counts) {
  t_cur_ctx = c;
  if (counts) c->seq++;  // (see Ctx::seq)
  HIPCHK(hipSetDevice(c->device));
  return RBG_OK;
}

static int rs_alloc(Ctx* c, ResultSet& r);

int ctx_init(Ctx* c, int device) {
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) {
    set_err("no HIP device " + std::to_string(device));
    return RBG_ERR_DEVICE;
  }
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_err(std::string("engine is built for gfx950, device is ") + prop.gcnArchName);
    return RBG_ERR_DEVICE;
  }
  c->device = device;
  {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    g_ctxs.push_back(c);
  }
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  CHK(c->by_key.ensure(sizeof(PTask) * kMaxKeys));  // Task (wide) or PTask (pairwise) records
  CHK(c->flag.ensure(kMaxKeys));
  CHK(c->wg_count.ensure(4 * 256));
  CHK(c->scalar.ensure(64));
  return rs_alloc(c, c->rs[0]);
}

// ---------------------------------------------------------------------------
// the two result sets and their streams
// ---------------------------------------------------------------------------
// One op after the other on one stream leaves HBM idle at every launch boundary and through the compute
// kernel's tail, and the serialization cannot start before the last task is placed.  A stream of independent
// pairwise ops is therefore run as two in-order lanes: op N with its serialization on set N % 2's stream,
// with that set's own records, buffers and plan state, so each lane's launch gaps and tails are filled by
// the other lane's kernels.  Within a lane the stream's order is all the ordering there is; between the
// lanes there is no event in the steady state.  Events order the rest: the context's stream waits for set
// 1's stream before anything consumes a result, frees an operand or runs an op of another kind (join_set),
// and set 1's stream waits for the context's stream after any call that may have given it work (lane_sync).
// The host waits for nothing.
static int join_set(Ctx* c, ResultSet& r) {
  r.in_flight = false;  // consumed, or overwritten by what follows
  if (r.stream == c->stream || !r.touched) return RBG_OK;
  HIPCHK(hipEventRecord(r.done, r.stream));
  HIPCHK(hipStreamWaitEvent(c->stream, r.done, 0));
  r.touched = false;
  return RBG_OK;
}
int join_result(Ctx* c) { return join_set(c, c->r()); }
int join_all(Ctx* c) {
  CHK(join_set(c, c->rs[0]));
  return join_set(c, c->rs[1]);
}
// an op that runs on the context's stream: behind both lanes, into set 0
int main_set(Ctx* c) {
  CHK(join_all(c));
  c->cur = 0;
  c->seq++;
  return RBG_OK;
}
// before the current set's stream is given work: it has run behind everything the context's stream held
// when the last counted call returned (a load, a consumer that placed or read this set, an op of another kind)
static int lane_sync(Ctx* c) {
  ResultSet& r = c->r();
  if (r.stream == c->stream) return RBG_OK;
  if (r.synced_seq != c->seq) {
    HIPCHK(hipEventRecord(r.main_done, c->stream));
    HIPCHK(hipStreamWaitEvent(r.stream, r.main_done, 0));
    r.synced_seq = c->seq;
  }
  r.touched = true;
  return RBG_OK;
}
// the host waits for both streams; nothing is in flight afterwards, so the next op runs on the context's stream
int sync_streams(Ctx* c) {
  if (c->rs[1].stream) HIPCHK(hipStreamSynchronize(c->rs[1].stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (ResultSet& r : c->rs) r.in_flight = r.touched = false;
  return RBG_OK;
}
// a set's stream, events and the buffers whose size no op changes (result and scratch are sized by
// prepare_output); set 0 runs on the context's stream
static int rs_alloc(Ctx* c, ResultSet& r) {
  if (r.ready) return RBG_OK;
  if (&r == &c->rs[0]) {
    r.stream = c->stream;
  } else {
    if (!r.stream) HIPCHK(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
    if (!r.done) HIPCHK(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
    if (!r.main_done) HIPCHK(hipEventCreateWithFlags(&r.main_done, hipEventDisableTiming));
  }
  // (+ 32768 records past the largest task list: sized for the removed key-order pairwise form's
  // wave-major layout; kept so no op's buffer shrinks)
  CHK(r.tasks.ensure(sizeof(PTask) * (kMaxKeys + 32768)));
  CHK(r.ntasks.ensure(64));
  CHK(r.wg_epoch.ensure(8 * 256));
  HIPCHK(hipMemsetAsync(r.wg_epoch.p, 0, 8 * 256, r.stream));  // in front of the stream's first plan kernel
  CHK(r.lb.ensure(kLbHeader + 8 * (kMaxKeys + 2 * kMaxTiles + kMaxAggTiles)));  // + the pairwise tile aggregates
  CHK(r.recs.ensure(sizeof(ORec) * kMaxKeys));
  CHK(r.kind_by_out.ensure(kMaxKeys));
  CHK(r.info.ensure(sizeof(ResultInfo)));
  CHK(r.task_card.ensure(4 * kMaxKeys));
  r.ready = true;
  return RBG_OK;
}

int pinned_ensure(Ctx* c, size_t bytes) {
  if (c->pinned_cap >= bytes) return RBG_OK;
  if (c->pinned) (void)hipHostFree(c->pinned);
  c->pinned = nullptr;
  c->pinned_cap = 0;
  HIPCHK(hipHostMalloc(&c->pinned, bytes, hipHostMallocDefault));
  c->pinned_cap = bytes;
  return RBG_OK;
}

// epoch of the next pairwise plan (never 0, the value the tags start from)
static uint32_t next_epoch(Ctx* c) {
  if (++c->r().epoch == 0) ++c->r().epoch;
  return c->r().epoch;
}
// Where the plan kernel of the op being enqueued writes (after prepare_output, which decides what it
// zeroes); one new epoch per plan that compacts its tasks (k_plan_balanced does not: compacts = false)
static PlanOut plan_out(Ctx* c, bool compacts = true) {
  return PlanOut{c->r().wg_epoch.as<uint64_t>(), compacts ? next_epoch(c) : 0, c->r().tasks.as<PTask>(),
                 c->r().ntasks.as<uint32_t>(), c->zlb, c->ztile};
}

int find_batch(Ctx* c, int32_t id, Batch** out) {
  if (id < 0 || (size_t)id >= c->batches.size() || !c->batches[id] || !c->batches[id]->live) {
    set_err("invalid batch id " + std::to_string(id));
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  *out = c->batches[id].get();
  return RBG_OK;
}

// A batch made by runOptimize on the device has its statistics (container kinds, payload bytes, the
// per-bitmap run flags) in device memory until something on the host needs them: read them then.
static int ensure_stats(Ctx* c, Batch* b) {
  if (!b->stats_pending) return RBG_OK;
  const size_t n = b->n_bm, g = b->ro_groups, foff = ro_flags_off(g);
  uint32_t* flags = reinterpret_cast<uint32_t*>(b->ro_stats.as<uint8_t>() + foff);
  if (n) {
    HIPCHK(hipMemsetAsync(flags, 0, 4 * n, c->stream));
    launch_runopt_flags(c->stream, b->desc.as<CDesc>(), b->bm.as<uint32_t>(), b->n_ctr, flags);
  }
  std::vector<unsigned long long> hs(8 + 4 * g);
  std::vector<uint32_t> hf(n);
  HIPCHK(hipMemcpyAsync(hs.data(), b->ro_stats.p, 8 * hs.size(), hipMemcpyDeviceToHost, c->stream));
  if (n) HIPCHK(hipMemcpyAsync(hf.data(), flags, 4 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  b->stats_pending = false;
  unsigned long long h[4] = {0, 0, 0, 0};
  for (size_t w = 0; w < g; w++)
    for (int k = 0; k < 4; k++) h[k] += hs[8 + 4 * w + k];
  for (int k = 0; k < 3; k++) b->n_kind[k] = (int64_t)h[k];
  int64_t ser = (int64_t)h[3];
  b->h_has_run.assign(n, 0);
  for (size_t i = 0; i < n; i++) {
    const size_t nc = b->h_bm_nctr.empty() ? 0 : b->h_bm_nctr[i];
    ser += (int64_t)header_size(nc, hf[i] != 0);
    b->h_has_run[i] = hf[i] != 0;
  }
  if (b->ser_bytes) b->ser_bytes = ser;  // batches built on the device carry no serialized size
  return RBG_OK;
}

int get_batch(Ctx* c, int32_t id, Batch** out) {
  CHK(find_batch(c, id, out));
  return ensure_stats(c, *out);
}

int32_t new_batch(Ctx* c) {
  for (size_t i = 0; i < c->batches.size(); i++)
    if (!c->batches[i]) {
      c->batches[i].reset(new Batch());
      return (int32_t)i;
    }
  c->batches.emplace_back(new Batch());
  return (int32_t)(c->batches.size() - 1);
}

constexpr size_t kPoolMax = 2ull << 30;    // bytes of released buffers a context keeps
constexpr size_t kPoolMaxBuf = 1ull << 30;  // larger buffers are freed at once

// a released batch buffer into the context's pool (reused only by later work on the same stream)
void pool_put(Ctx* c, DevBuf& b) {
  if (!b.p) return;
  std::lock_guard<std::mutex> g(c->pool_mu);
  if (b.cap > kPoolMaxBuf) {
    b = DevBuf();
    return;
  }
  while (!c->pool.empty() && c->pool_bytes + b.cap > kPoolMax) {  // oldest first
    c->pool_bytes -= c->pool.front().cap;
    c->pool.erase(c->pool.begin());
  }
  c->pool_bytes += b.cap;
  c->pool.push_back(std::move(b));
}

// dst sized for `bytes`: the smallest pooled buffer that holds it (at most twice as large),
// else a fresh allocation
int pool_take(Ctx* c, DevBuf& dst, size_t bytes) {
  if (dst.p && dst.cap >= bytes) return RBG_OK;
  std::unique_lock<std::mutex> lk(c->pool_mu);
  size_t best = c->pool.size();
  for (size_t i = 0; i < c->pool.size(); i++) {
    const size_t cap = c->pool[i].cap;
    if (cap >= bytes && cap <= 2 * bytes + (1u << 20) && (best == c->pool.size() || cap < c->pool[best].cap))
      best = i;
  }
  if (best == c->pool.size()) {
    lk.unlock();  // ensure may empty the pools (out of memory)
    return dst.ensure(bytes);
  }
  c->pool_bytes -= c->pool[best].cap;
  dst = std::move(c->pool[best]);
  c->pool.erase(c->pool.begin() + (std::ptrdiff_t)best);
  return RBG_OK;
}

// ---------------------------------------------------------------------------
// op pipelines
// ---------------------------------------------------------------------------
// Result buffer: [header reserve P0][payload region].  The header (whose size
// depends on the final container count and run flag) is written right in front
// of the payload, so the serialized bitmap starts at P0 - header.
static uint64_t header_reserve(size_t max_tasks) {
  return round16(8 + (max_tasks + 7) / 8 + 8 * (uint64_t)max_tasks + 16);
}

int grid_for(size_t tasks, size_t cap) {
  size_t g = std::min(tasks, cap);
  return (int)std::max<size_t>(g, 1);
}

// Output state of a materialising op: per-task records + scratch slots (the
// device-resident result), and the portable-format buffer the serialization
// writes into on fetch.  Card-only ops need no output state.
// lanes (a materialising pairwise op): if the current set's serialization is enqueued and nothing consumed
// it, the op takes the other set (made by the first op that does) and runs on that set's stream, behind the
// serialization of two ops ago and beside the last one.  Every other op runs on the context's stream,
// behind both lanes, into set 0.
int prepare_output(Ctx* c, size_t max_tasks, size_t max_payload, OutCtx* oc, bool card_only, bool lanes) {
  if (!lanes || card_only) {
    CHK(main_set(c));
  } else {
    if (c->r().in_flight) {
      ResultSet& o = c->rs[c->cur ^ 1];
      CHK(rs_alloc(c, o));
      c->cur ^= 1;
      o.in_flight = false;  // its own stream orders this op behind that serialization
      o.last = 0;
    } else if (c->cur != 0) {
      // nothing to run beside (the last result was consumed, or the host has waited): back to the context's
      // stream, so that whatever a caller puts on that stream brackets and follows the op as it always did
      CHK(main_set(c));
    }
    CHK(lane_sync(c));
  }
  uint8_t* lb = c->r().lb.as<uint8_t>();  // look-back state: ticket @0, error word @64, statuses @256
  *oc = OutCtx{};
  oc->err = reinterpret_cast<uint32_t*>(lb + 64);
  oc->status = reinterpret_cast<uint64_t*>(lb + kLbHeader);
  oc->tile_status = reinterpret_cast<uint64_t*>(lb + kLbHeader + 8 * kMaxKeys);
  oc->tile_card = reinterpret_cast<uint64_t*>(lb + kLbHeader + 8 * (kMaxKeys + kMaxTiles));
  oc->recs = c->r().recs.as<ORec>();
  c->r().serialized = false;
  c->r().place_pending = false;
  c->r().agg_ok = false;
  c->r().ri_valid = false;
  c->r().pending_ub = 0;
  c->zlb = c->ztile = nullptr;
  c->r().pending_src.clear();
  if (card_only) {
    c->zlb = reinterpret_cast<uint64_t*>(lb);  // the error word must not carry over from an earlier op
    return RBG_OK;
  }
  const uint64_t P0 = header_reserve(max_tasks);
  CHK(c->r().result.ensure(P0 + max_payload + 64));
  c->r().result_cap = P0 + max_payload;
  CHK(c->r().scratch.ensure((size_t)kSlotBytes * std::max<size_t>(max_tasks, 1) + 64));
  // the look-back header and tile statuses are zeroed by the op's plan kernel
  c->zlb = reinterpret_cast<uint64_t*>(lb);
  c->ztile = reinterpret_cast<uint64_t*>(lb + kLbHeader + 8 * kMaxKeys);
  oc->out = c->r().result.as<uint8_t>();
  oc->payload_base = P0;
  oc->scratch = c->r().scratch.as<uint8_t>();
  oc->kind_by_out = c->r().kind_by_out.as<uint8_t>();
  c->r().pending = *oc;
  c->r().pending_ub = max_tasks;
  return RBG_OK;
}

// Placement of a materialising op's result (k_place) is deferred until something needs it
// (serialization, result statistics, a key-shard fetch): an op whose caller only wants the
// result to exist on the device (a BSI query followed by its sum) does not pay for it.
void defer_place(Ctx* c) {
  c->r().place_pending = true;
  c->r().last = 1;
}
static int place_on(Ctx* c, hipStream_t s) {
  if (!c->r().place_pending) return RBG_OK;
  launch_place(s, c->r().ntasks.as<uint32_t>(), c->r().pending, c->r().info.as<ResultInfo>());
  HIPCHK(hipGetLastError());
  c->r().place_pending = false;
  return RBG_OK;
}
int ensure_placed(Ctx* c) { return place_on(c, c->stream); }

// Portable serialization of the pending result (RB/RoaringArray.java:896-940),
// on the device, once per result.
// Its kernels go to the set's own stream, where the op's kernels are (on_main: to the context's stream, joined
// first); in_flight from here until something consumes the result.
int ctx_serialize(Ctx* c, bool on_main) {
  ResultSet& r = c->r();
  if (r.last != 1) {
    set_err("no materialised result pending");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (r.serialized) return RBG_OK;
  hipStream_t s = r.stream;
  if (on_main) {
    CHK(join_result(c));
    c->seq++;  // the set's stream runs behind this before it goes on
    s = c->stream;
  } else {
    CHK(lane_sync(c));  // (a consumer may have placed the result on the context's stream)
  }
  if (r.place_pending && r.agg_ok && !r.pending.spec && r.pending_ub <= (size_t)kMaxAggTiles * kAggTile) {
    // placement from the compute kernel's tile sums and the serialization in one launch
    launch_serialize_agg(s, r.ntasks.as<uint32_t>(), r.pending, r.info.as<ResultInfo>(), r.pending_ub);
    r.place_pending = false;
  } else {
    CHK(place_on(c, s));
    if (r.pending.spec) launch_spec_fix(s, r.ntasks.as<uint32_t>(), r.pending);
    launch_serialize(s, r.ntasks.as<uint32_t>(), r.pending);
  }
  HIPCHK(hipGetLastError());
  r.serialized = true;
  r.in_flight = !on_main;
  return RBG_OK;
}

// Bitmap i of a batch as the operand of a per-key op: what the kernels see of it (BmView: key CSR, container
// table, payload, container count) and the batch (statistics read).  The range must be contiguous: a
// one-bitmap key-major batch.
int resolve(Ctx* c, int32_t id, size_t i, Operand* op) {
  Batch* b;
  CHK(get_batch(c, id, &b));
  if (i >= b->n_bm) {
    set_err("bitmap index out of range");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (b->n_bm != 1 || !b->key_major || b->packed) {
    set_err("pairwise operands must be single-bitmap key-major batches with slot-aligned payloads");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  *op = Operand{{b->key_off.as<uint32_t>(), b->desc.as<CDesc>(), b->payload.as<uint8_t>(), (int)b->n_ctr}, b};
  return RBG_OK;
}

// Bracket of an op that is one compute launch: op_begin after prepare_output (the batches the result's
// pass-through records point into, the first two phase marks), op_end after the launch (the placement
// deferred, the last two marks, the launch's error).
static void op_begin(Ctx* c, std::initializer_list<int32_t> src) {
  c->r().pending_src = src;
  c->mark(0);
  c->mark(1);
}
int op_end(Ctx* c) {
  c->mark(2);
  defer_place(c);
  c->mark(3);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// The rank directory of a batch resolve() accepts (rankdir.hip): the container prefix cum, and per bitmap
// / run container a u16 directory in an aux arena.  Sizes in one pass, two device scans, then the fill;
// the host reads back the arena's size alone (8 bytes, once per batch) to allocate it exactly.
// A build that fails part way leaves rd_ready false and whatever buffers it took on the batch: the next
// query takes them again (pool_take keeps a buffer that is large enough), release pools them.
static int ctx_rankdir(Ctx* c, Batch* b) {
  if (b->rd_ready) return RBG_OK;
  const size_t n = b->n_ctr;
  hipStream_t s = c->stream;
  CHK(pool_take(c, b->rd_cum, 8 * (n + 1)));
  CHK(pool_take(c, b->rd_off, 8 * (n + 1)));
  CHK(c->rd_part.ensure(8 * (scan_parts(std::max<uint64_t>(n, 1)) + 1)));
  uint64_t* cum = b->rd_cum.as<uint64_t>();
  uint64_t* off = b->rd_off.as<uint64_t>();
  launch_rd_sizes(s, b->desc.as<CDesc>(), b->payload.as<uint8_t>(), n, cum, off);
  launch_exclusive_scan(s, cum, cum, n, c->rd_part.as<uint64_t>(), cum + n);
  launch_exclusive_scan(s, off, off, n, c->rd_part.as<uint64_t>(), off + n);
  HIPCHK(hipGetLastError());
  uint64_t aux_bytes = 0;
  HIPCHK(hipMemcpyAsync(&aux_bytes, off + n, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  CHK(pool_take(c, b->rd_aux, aux_bytes + 16));
  launch_rd_fill(s, b->desc.as<CDesc>(), b->payload.as<uint8_t>(), n, off, b->rd_aux.as<uint8_t>());
  HIPCHK(hipGetLastError());
  b->rd_ready = true;
  return RBG_OK;
}

// n point queries (device memory, u32) against bitmap i of a batch into out (device memory, i64), in
// query order, enqueued on the context stream
int ctx_point(Ctx* c, int op, int32_t batch, size_t i, const uint32_t* q_dev, size_t n, long long* out_dev) {
  Operand o;
  CHK(resolve(c, batch, i, &o));
  Batch* B = o.b;
  CHK(ctx_rankdir(c, B));
  const PointArgs pa{B->key_off.as<uint32_t>(), o.desc, B->payload.as<uint8_t>(), B->rd_cum.as<uint64_t>(),
                     B->rd_off.as<uint64_t>(), B->rd_aux.as<uint8_t>(), (uint32_t)o.n};
  launch_point(c->stream, op, pa, q_dev, n, out_dev);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// the same from host memory: staged through the context's pinned buffer, results in out on return
int ctx_point_host(Ctx* c, int op, int32_t batch, size_t i, const uint32_t* q, size_t n, int64_t* out) {
  CHK(pinned_ensure(c, 12 * n + 64));
  CHK(c->pt_q.ensure(4 * n));
  CHK(c->pt_out.ensure(8 * n));
  uint8_t* pin = reinterpret_cast<uint8_t*>(c->pinned);
  hipStream_t s = c->stream;
  HIPCHK(hipStreamSynchronize(s));  // nothing enqueued earlier still reads the staging buffer
  std::memcpy(pin + 8 * n, q, 4 * n);
  HIPCHK(hipMemcpyAsync(c->pt_q.p, pin + 8 * n, 4 * n, hipMemcpyHostToDevice, s));
  CHK(ctx_point(c, op, batch, i, c->pt_q.as<uint32_t>(), n, c->pt_out.as<long long>()));
  HIPCHK(hipMemcpyAsync(pin, c->pt_out.p, 8 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(out, pin, 8 * n);
  return RBG_OK;
}

// The values of ranks [first, first + count) of bitmap i of a batch, clipped to the cardinality
// (RoaringBitmap.toArray, RB/RoaringBitmap.java:3224; BatchIterator.nextBatch), into out_dev (u32, or
// i64 with out64), enqueued on the context stream (expand.hip).  *n_out: the values written, known here
// from the batch's cardinality.
int ctx_to_values(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t count, bool out64, void* out_dev,
                  uint64_t* n_out) {
  Operand o;
  CHK(resolve(c, batch, i, &o));
  Batch* B = o.b;
  const uint64_t card = (uint64_t)B->long_card;
  const uint64_t cnt = first < card ? std::min<uint64_t>(count, card - first) : 0;
  if (n_out) *n_out = cnt;
  if (!cnt || (!out_dev && n_out)) return RBG_OK;  // no buffer: the caller asks for the window's size
  if (!out_dev) {
    set_err("to_values: no output buffer");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(ctx_rankdir(c, B));
  const PointArgs pa{B->key_off.as<uint32_t>(), o.desc, B->payload.as<uint8_t>(), B->rd_cum.as<uint64_t>(),
                     B->rd_off.as<uint64_t>(), B->rd_aux.as<uint8_t>(), (uint32_t)o.n};
  launch_to_values(c->stream, pa, first, cnt, out64, out_dev);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// the same into host memory (u32), one window of at most kToValuesWindow values on the device at a time
constexpr uint64_t kToValuesWindow = 64ull << 20;
int ctx_to_values_host(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t count, uint32_t* out,
                       uint64_t* n_out) {
  uint64_t total = 0;
  CHK(ctx_to_values(c, batch, i, first, count, false, nullptr, &total));  // the operand check and the size
  if (n_out) *n_out = total;
  if (!total || (!out && n_out)) return RBG_OK;
  if (!out) {
    set_err("to_values: no output buffer");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(c->tv_out.ensure(4 * std::min<uint64_t>(total, kToValuesWindow)));
  for (uint64_t done = 0; done < total; done += kToValuesWindow) {
    const uint64_t w = std::min<uint64_t>(kToValuesWindow, total - done);
    uint64_t got = 0;
    CHK(ctx_to_values(c, batch, i, first + done, w, false, c->tv_out.p, &got));
    HIPCHK(hipMemcpyAsync(out + done, c->tv_out.p, 4 * w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return RBG_OK;
}

// A bitmap from n values in device memory (u32, any order, duplicates allowed) as a new one-bitmap
// key-major batch: RoaringBitmap.add(int...) / addN / bitmapOf (RB/RoaringBitmap.java:483-570), with
// run_opt followed by runOptimize() (:2764-2774) -- the batch ctx_load of build_from_values' bytes gives
// (build.hip).  Two read-backs: the container count (to size the workspace of 8 KiB bitmaps) and the
// totals (payload size, kinds, cardinality).  The values are read by two kernels: they must not change
// until the call returns.
// The source is either those values or (bits != null) a dense bitset's own words, which then stand where the
// scattered workspace stands (bitset.hip): at most 2^29 bytes, read by three kernels.
static int build_batch(Ctx* c, const uint32_t* v_dev, size_t n, const uint8_t* bits, uint64_t nbytes, bool run_opt,
                       int32_t* out_id) {
  hipStream_t s = c->stream;
  if (bits) n = (size_t)((nbytes + 8191) / 8192);  // the bound of the key count
  const int32_t id = new_batch(c);
  Batch& b = *c->batches[id];
  struct Drop {  // an error below frees the half-built batch
    Ctx* c;
    int32_t id;
    bool keep = false;
    ~Drop() {
      if (!keep) c->batches[id].reset();
    }
  } drop{c, id};
  DevBuf ws;  // C zeroed bitmaps; back to the pool at the end (freed on an error)
  CHK(pool_take(c, b.keys, 2 * std::min<size_t>(n, kMaxKeys) + 16));
  CHK(pool_take(c, b.key_off, 4 * (kMaxKeys + 1)));
  CHK(pool_take(c, b.bm_off, 4 * 2));
  unsigned long long* sc = c->scalar.as<unsigned long long>();  // [0] C, [1..3] kinds, [4] serialized payload
                                                                // bytes, [5] cardinality, [6] slot bytes
  HIPCHK(hipMemsetAsync(c->flag.p, 0, kMaxKeys, s));
  HIPCHK(hipMemsetAsync(sc, 0, 64, s));
  if (bits) launch_bits_flags(s, bits, nbytes, c->flag.as<uint8_t>(), b.keys.as<uint16_t>(), b.key_off.as<uint32_t>(), sc);
  else launch_bld_keys(s, v_dev, n, c->flag.as<uint8_t>(), b.keys.as<uint16_t>(), b.key_off.as<uint32_t>(), sc);
  HIPCHK(hipGetLastError());
  unsigned long long h[8] = {};
  HIPCHK(hipMemcpyAsync(h, sc, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const size_t C = (size_t)h[0];
  dbg(s, "from_values: keys");
  if (C) {
    if (!bits) {
      CHK(pool_take(c, ws, 8192 * C));
      HIPCHK(hipMemsetAsync(ws.p, 0, 8192 * C, s));
      launch_bld_scatter(s, v_dev, n, b.key_off.as<uint32_t>(), ws.as<uint32_t>());
    }
    CHK(c->bld_info.ensure(kBldInfoBytes * C));
    CHK(c->bld_size.ensure(8 * C + 16));
    CHK(c->bld_part.ensure(8 * (scan_parts(C) + 1)));
    if (bits)
      launch_bits_plan(s, bits, nbytes, b.keys.as<uint16_t>(), C, run_opt ? 1 : 0, c->bld_info.p,
                       c->bld_size.as<uint64_t>(), sc + 1);
    else
      launch_bld_plan(s, ws.as<uint8_t>(), C, run_opt ? 1 : 0, c->bld_info.p, c->bld_size.as<uint64_t>(), sc + 1);
    launch_exclusive_scan(s, c->bld_size.as<uint64_t>(), c->bld_size.as<uint64_t>(), C, c->bld_part.as<uint64_t>(),
                          reinterpret_cast<uint64_t*>(sc + 6));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, sc, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    dbg(s, "from_values: scatter + plan");
  }
  b.payload_bytes = (size_t)h[6];
  CHK(pool_take(c, b.desc, sizeof(CDesc) * C + 16));
  CHK(pool_take(c, b.bm, 4 * C + 16));
  CHK(pool_take(c, b.payload, b.payload_bytes + 64));
  if (C && bits)
    launch_bits_write(s, bits, nbytes, b.keys.as<uint16_t>(), C, c->bld_info.p, c->bld_size.as<uint64_t>(),
                      b.desc.as<CDesc>(), b.bm.as<uint32_t>(), b.bm_off.as<uint32_t>(), b.payload.as<uint8_t>());
  else if (C)
    launch_bld_write(s, ws.as<uint8_t>(), C, c->bld_info.p, c->bld_size.as<uint64_t>(), b.keys.as<uint16_t>(),
                     b.desc.as<CDesc>(), b.bm.as<uint32_t>(), b.bm_off.as<uint32_t>(), b.payload.as<uint8_t>());
  else
    HIPCHK(hipMemsetAsync(b.bm_off.p, 0, 8, s));
  HIPCHK(hipGetLastError());
  dbg(s, "from_values: write");
  pool_put(c, ws);  // whatever takes it next is enqueued on this stream, after the write kernel
  b.n_bm = 1;
  b.n_ctr = C;
  b.key_major = true;
  for (int k = 0; k < 3; k++) b.n_kind[k] = (int64_t)h[1 + k];
  const bool has_run = h[3] != 0;
  b.ser_bytes = (int64_t)(header_size(C, has_run) + h[4]);
  b.long_card = (int64_t)h[5];
  b.max_ser = 0;  // no container above kStagedMax serialized bytes
  b.h_bm_off = {0, (uint32_t)C};
  b.h_bm_nctr = {(uint32_t)C};
  b.h_bm_card = {b.long_card};
  b.h_has_run = {(uint8_t)has_run};
  b.live = true;
  drop.keep = true;
  *out_id = id;
  return RBG_OK;
}

int ctx_from_values(Ctx* c, const uint32_t* v_dev, size_t n, bool run_opt, int32_t* out_id) {
  return build_batch(c, v_dev, n, nullptr, 0, run_opt, out_id);
}

// one empty bitmap as a new batch: the result of a query that no column can satisfy
int ctx_empty_bitmap(Ctx* c, int32_t* out_id) { return ctx_from_values(c, nullptr, 0, false, out_id); }

// n bytes from host memory into dst (device), through the context's pinned buffer, a chunk at a time
static int upload_bytes(Ctx* c, void* dst, const void* src, size_t n) {
  constexpr size_t kChunk = 64u << 20;  // bytes per staged copy
  if (!n) return RBG_OK;
  CHK(pinned_ensure(c, std::min(n, kChunk)));
  HIPCHK(hipStreamSynchronize(c->stream));  // nothing enqueued earlier still reads the staging buffer
  for (size_t off = 0; off < n; off += kChunk) {
    const size_t m = std::min(kChunk, n - off);
    std::memcpy(c->pinned, reinterpret_cast<const uint8_t*>(src) + off, m);
    HIPCHK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(dst) + off, c->pinned, m, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return RBG_OK;
}
// n 32-bit words
int upload_words(Ctx* c, void* dst, const void* src, size_t n) { return upload_bytes(c, dst, src, 4 * n); }

// ctx_from_values from host memory
int ctx_from_values_host(Ctx* c, const uint32_t* v, size_t n, bool run_opt, int32_t* out_id) {
  DevBuf in;
  CHK(pool_take(c, in, 4 * n + 16));
  CHK(upload_words(c, in.p, v, n));
  const int st = ctx_from_values(c, in.as<uint32_t>(), n, run_opt, out_id);
  pool_put(c, in);
  return st;
}

// ---- dense bitsets (bitset.hip): BitSetUtil, RB/BitSetUtil.java ----
// The key arithmetic of bitmapOf (from * Long.SIZE, :169) is Java int: a bitset has at most 2^32 bits.
constexpr uint64_t kBitsetMaxBits = 1ull << 32;

// the refusals of a build, decided from the arguments alone; device: bits is read in place by the kernels
int check_bitset_build(const void* bits, uint64_t n, int layout, bool device) {
  if (layout != RBG_BITS_PACKED && layout != RBG_BITS_BYTES) {
    set_err("bitset: unknown layout (RBG_BITS_PACKED or RBG_BITS_BYTES)");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (n && !bits) {
    set_err("bitset: no input");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (n > (layout == RBG_BITS_PACKED ? kBitsetMaxBits / 8 : kBitsetMaxBits)) {
    set_err("bitset: more than 2^32 bits");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (device && layout == RBG_BITS_PACKED && (reinterpret_cast<uintptr_t>(bits) & 7)) {
    set_err("bitset: packed words must be 8-byte aligned");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// the refusals of an expansion's window [first, first + n) of bit positions
int check_bitset_window(uint64_t first, uint64_t n, int layout) {
  if (layout != RBG_BITS_PACKED && layout != RBG_BITS_BYTES) {
    set_err("bitset: unknown layout (RBG_BITS_PACKED or RBG_BITS_BYTES)");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (layout == RBG_BITS_PACKED && (first & 63)) {
    set_err("bitset: a packed window starts at a multiple of 64");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (first > kBitsetMaxBits || n > kBitsetMaxBits - first) {
    set_err("bitset: the window reaches past 2^32");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// BitSetUtil.bitmapOf(long[]) (:160-174, containerOf :270-283) / bitmapOf(ByteBuffer) (:185-259) [+ runOptimize]
// of a dense bitset in device memory, as the batch ctx_from_values of its bit positions makes.  layout
// RBG_BITS_PACKED: n bytes of little-endian 64-bit words, the last possibly cut short; RBG_BITS_BYTES: n mask
// elements, first packed into a pooled buffer of words.  Arguments as check_bitset_build passes them.  The
// input is read by up to four kernels: it must not change until the call returns.
int ctx_from_bitset(Ctx* c, const void* bits_dev, uint64_t n, int layout, bool run_opt, int32_t* out_id) {
  if (!n) return build_batch(c, nullptr, 0, nullptr, 0, run_opt, out_id);
  if (layout == RBG_BITS_PACKED)
    return build_batch(c, nullptr, 0, reinterpret_cast<const uint8_t*>(bits_dev), n, run_opt, out_id);
  const uint64_t nbytes = 8 * ((n + 63) / 64);
  DevBuf words;
  CHK(pool_take(c, words, nbytes + 16));
  launch_bits_pack(c->stream, reinterpret_cast<const uint8_t*>(bits_dev), n, words.as<uint64_t>());
  HIPCHK(hipGetLastError());
  const int st = build_batch(c, nullptr, 0, words.as<uint8_t>(), nbytes, run_opt, out_id);
  pool_put(c, words);
  return st;
}

// the same from host memory
int ctx_from_bitset_host(Ctx* c, const void* bits, uint64_t n, int layout, bool run_opt, int32_t* out_id) {
  DevBuf in;
  CHK(pool_take(c, in, n + 16));
  CHK(upload_bytes(c, in.p, bits, n));
  const int st = ctx_from_bitset(c, in.p, n, layout, run_opt, out_id);
  pool_put(c, in);
  return st;
}

// BitSetUtil.toLongArray (:67-108) over the window [first, first + n) of bit positions of bitmap i of a batch,
// into out_dev: packed words or mask bytes (launch_bits_expand), enqueued on the context stream; nothing is
// read back.  Arguments as check_bitset_window passes them.
int ctx_to_bitset(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout, void* out_dev) {
  Operand o;
  CHK(resolve(c, batch, i, &o));
  if (!n) return RBG_OK;
  if (!out_dev || (layout == RBG_BITS_PACKED && (reinterpret_cast<uintptr_t>(out_dev) & 7))) {
    set_err("bitset: no output buffer, or packed words not 8-byte aligned");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  launch_bits_expand(c->stream, o.key_off, o.desc, o.payload, first, n, layout == RBG_BITS_BYTES, out_dev);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// the same into host memory, one window of at most 256 MiB on the device at a time
int ctx_to_bitset_host(Ctx* c, int32_t batch, size_t i, uint64_t first, uint64_t n, int layout, void* out) {
  CHK(ctx_to_bitset(c, batch, i, first, 0, layout, nullptr));  // the operand check
  if (!n) return RBG_OK;
  if (!out) {
    set_err("bitset: no output buffer");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const bool mask = layout == RBG_BITS_BYTES;
  const uint64_t window = mask ? 1ull << 28 : 1ull << 31;  // bit positions per pass; a multiple of 64
  auto bytes_of = [&](uint64_t bits) { return mask ? bits : 8 * ((bits + 63) / 64); };
  CHK(c->tv_out.ensure(bytes_of(std::min(n, window))));
  for (uint64_t done = 0; done < n; done += window) {
    const uint64_t w = std::min(window, n - done);
    CHK(ctx_to_bitset(c, batch, i, first + done, w, layout, c->tv_out.p));
    HIPCHK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(out) + bytes_of(done), c->tv_out.p, bytes_of(w),
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return RBG_OK;
}

// ImmutableRoaringBitmap.and / andNot and MutableRoaringBitmap's static and / andNot
// (RB/buffer/ImmutableRoaringBitmap.java:299-325, 441-471; RB/buffer/MutableRoaringBitmap.java:235-301):
// the pairwise plan, then k_pair_buf (the buffer package's container types).  A run result above
// 2047 runs goes to the big-run arena (with_big_runs).
static int ctx_pairwise_buffer(Ctx* c, int op, int32_t ia, size_t ma, int32_t ib, size_t mb, int key_lo, int key_hi) {
  key_lo = std::max(0, key_lo);
  key_hi = std::min(kMaxKeys, key_hi);
  Operand A, B;
  CHK(resolve(c, ia, ma, &A));
  CHK(resolve(c, ib, mb, &B));
  hipStream_t s = c->stream;
  const size_t ub = std::max<size_t>(1, op == OP_AND ? (size_t)std::min(A.n, B.n) : (size_t)A.n);
  return with_big_runs(c, true, "buffer and / andNot", [&](const BigRuns& big) -> int {
    OutCtx oc;
    CHK(prepare_output(c, ub, A.b->payload_bytes + B.b->payload_bytes + kStagedMax * ub + big.cap, &oc, false));
    c->r().pending_src = {ia, ib};
    c->mark(0);
    const PlanOut po = plan_out(c);
    launch_plan_pairwise(s, op, key_lo, key_hi, A, B, po, oc.err);
    c->mark(1);
    launch_pair_buf(s, op, grid_for(ub, 65536), po.tasks, po.n_tasks, A.payload, B.payload, oc, big);
    return op_end(c);
  });
}

// RoaringBitmap.orNot(x1, x2, rangeEnd) (static, RB/RoaringBitmap.java:1521-1603) and x1.orNot(x2,
// rangeEnd) (in place, :1431-1506), ornot.hip.  rangeSanityCheck(0, rangeEnd) (:204-213).  The
// reference's maxSize is negative only for rangeEnd == 0 (maxKey = -1) with x1 empty and x2's first
// container full (new char[-1] throws): only that case reads the plan back before returning.
int ctx_ornot(Ctx* c, int32_t ia, size_t ma, int32_t ib, size_t mb, int64_t range_end, int flags) {
  if (range_end < 0 || range_end > (int64_t)0x100000000ll) {
    set_err("rangeEnd should be in [0, 0xffffffff + 1]");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  Operand A, B;
  CHK(resolve(c, ia, ma, &A));
  CHK(resolve(c, ib, mb, &B));
  const int max_key = range_end == 0 ? -1 : (int)((range_end - 1) >> 16);
  const int last_run = (range_end & 0xFFFF) == 0 ? 0x10000 : (int)(range_end & 0xFFFF);
  hipStream_t s = c->stream;
  const size_t ub = std::max<size_t>(1, std::min<size_t>(kMaxKeys, (size_t)(max_key + 1) + (size_t)A.n));
  if (!c->ornot_plan.p) CHK(c->ornot_plan.ensure(sizeof(OrNotPlan)));
  OutCtx oc;
  CHK(prepare_output(c, ub, A.b->payload_bytes + B.b->payload_bytes + kStagedMax * ub, &oc, false));
  op_begin(c, {ia, ib});
  launch_ornot(s, A, B, max_key, last_run, flags, c->ornot_plan.as<OrNotPlan>(), plan_out(c), oc,
               grid_for(ub, 65536));
  CHK(op_end(c));
  if (max_key < 0 && A.n == 0 && B.n > 0) {
    OrNotPlan pl;
    HIPCHK(hipMemcpyAsync(&pl, c->ornot_plan.p, sizeof(pl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (pl.neg) {
      c->r().last = 0;
      set_err("orNot: negative maxSize (the reference throws NegativeArraySizeException)");
      return RBG_ERR_ILLEGAL_ARGUMENT;
    }
  }
  return RBG_OK;
}

// rangeSanityCheck (RB/RoaringBitmap.java:204-213)
int check_range(int64_t start, int64_t end) {
  if (start < 0 || start > 0xFFFFFFFFll || end < 0 || end > 0x100000000ll) {
    set_err("rangeStart=" + std::to_string(start) + " should be in [0, 0xffffffff], rangeEnd=" + std::to_string(end) +
            " in [0, 0xffffffff + 1]");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  return RBG_OK;
}

// One k_rmut launch over operand A (batch ia) into at most ub result containers (rangemut.hip): the
// range mutations, removeRunCompression and limit.  A run result above 2047 runs goes to the big-run
// arena (with_big_runs).  The kernel reaches the arena only for the first and the last key of a range and
// for limit's cut key (the keys between are cloned, emptied or replaced by the full run): at most two
// containers of at most 131,074 B in one call, which the arena's initial 16 MiB always holds, so the
// runner's second pass is never taken from here.
static int run_rmut(Ctx* c, int32_t ia, const Operand& A, RmutArgs ra, bool buf, size_t ub, bool use_arena,
                    const char* what) {
  return with_big_runs(c, use_arena, what, [&](const BigRuns& big) -> int {
    OutCtx oc;
    CHK(prepare_output(c, ub, A.b->payload_bytes + kStagedMax * ub + big.cap, &oc, false));
    op_begin(c, {ia});
    launch_rmut(c->stream, A, ra, buf, plan_out(c), oc, big, grid_for(ub, 65536));
    return op_end(c);
  });
}

// static add / remove / flip(rb, rangeStart, rangeEnd) (RB/RoaringBitmap.java:298-345, 995-1040, 626-668;
// buf: MutableRoaringBitmap's, RB/buffer/MutableRoaringBitmap.java:152-205, 649-700, 455-505), rangemut.hip.
// rangeSanityCheck (:204-213); rangeEnd <= rangeStart gives a clone.
int ctx_range_mut(Ctx* c, int op, int32_t ia, size_t ma, int64_t start, int64_t end, bool buf) {
  if (op < RMUT_ADD || (op > RMUT_ADD_INPLACE && op != RMUT_RANGE)) return RBG_ERR_ILLEGAL_ARGUMENT;
  CHK(check_range(start, end));
  Operand A;
  CHK(resolve(c, ia, ma, &A));
  RmutArgs ra{op, 1, 0, 0, 0};  // end <= start: no key in the range, every container cloned
  if (end > start) {  // (char) casts: Util.highbits / lowbits
    ra.hbs = (int)((uint64_t)start >> 16 & 0xFFFF);
    ra.lbs = (int)(start & 0xFFFF);
    ra.hbl = (int)((uint64_t)(end - 1) >> 16 & 0xFFFF);
    ra.lbl = (int)((end - 1) & 0xFFFF);
  }
  const size_t in_range = end > start ? (size_t)(ra.hbl - ra.hbs + 1) : 0;
  const size_t ub = std::max<size_t>(1, std::min<size_t>(kMaxKeys, (size_t)A.n + in_range));
  return run_rmut(c, ia, A, ra, buf, ub, true, "range add / remove");
}

// x.removeRunCompression() (RB/RoaringBitmap.java:2738-2749; the buffer package's alike): every run
// container through toBitmapOrArrayContainer (RB/RunContainer.java:2300-2323), the rest cloned; rangemut.hip.
// RunContainer.toBitmapOrArrayContainer never makes a run container: no big-run arena (RMUT_DERUN's kernel
// has no path to it)
int ctx_remove_run_compression(Ctx* c, int32_t ia, size_t ma) {
  Operand A;
  CHK(resolve(c, ia, ma, &A));
  return run_rmut(c, ia, A, RmutArgs{RMUT_DERUN, 1, 0, 0, 0}, false, std::max<size_t>(1, (size_t)A.n), false,
                  "removeRunCompression");
}

// The device half of x.limit(maxcardinality) (RB/RoaringBitmap.java:2457-2476; the cut is planned on the
// host, rbg_limit): keys before cut_key cloned, its container cut to the leftover by k_rmut<RMUT_LIMIT>,
// the rest dropped.
int ctx_limit(Ctx* c, int32_t ia, size_t ma, int cut_key, int leftover) {
  Operand A;
  CHK(resolve(c, ia, ma, &A));
  return run_rmut(c, ia, A, RmutArgs{RMUT_LIMIT, cut_key, leftover, 0, 0}, false, std::max<size_t>(1, (size_t)A.n),
                  true, "limit");
}

// RoaringBitmap.addOffset(x, offset) (RB/RoaringBitmap.java:230-288; MutableRoaringBitmap.addOffset,
// RB/buffer/MutableRoaringBitmap.java:84-142, the same bytes), addoffset.hip.  The container offset is
// the floor of offset / 65536 (:233-234); outside [-65536, 65535] the result is empty (:235-237).
int ctx_add_offset(Ctx* c, int32_t ia, size_t ma, int64_t offset) {
  Operand A;
  CHK(resolve(c, ia, ma, &A));
  const int64_t co = offset < 0 ? (offset - 65535) / 65536 : offset / 65536;
  AoffArgs aa{0, 0, 1};
  if (co >= -65536 && co < 65536) aa = AoffArgs{(int)co, (int)(offset - co * 65536), 0};
  // each input container gives at most two output containers, each staged (<= kStagedMax) or a clone
  const size_t ub = std::max<size_t>(1, std::min<size_t>(kMaxKeys, 2 * (size_t)A.n));
  OutCtx oc;
  CHK(prepare_output(c, ub, A.b->payload_bytes + kStagedMax * ub, &oc, false));
  op_begin(c, {ia});
  launch_aoff(c->stream, A, aa, plan_out(c), oc, grid_for(ub, 65536));
  return op_end(c);
}

// op RBG_OR_INPLACE: x1.or(x2) in place (RB/RoaringBitmap.java:2481-2523), the OR with Container.ior's
// types (k_ior_fix)
int ctx_pairwise(Ctx* c, int op, int32_t ia, size_t ma, int32_t ib, size_t mb, bool card_only, int key_lo,
                 int key_hi, bool lanes) {
  if (op == RBG_AND_BUFFER || op == RBG_ANDNOT_BUFFER) {
    if (card_only) return RBG_ERR_ILLEGAL_ARGUMENT;
    return ctx_pairwise_buffer(c, op == RBG_AND_BUFFER ? OP_AND : OP_ANDNOT, ia, ma, ib, mb, key_lo, key_hi);
  }
  if (op == RBG_OR_INPLACE && !card_only) {
    CHK(ctx_pairwise(c, OP_OR, ia, ma, ib, mb, false, key_lo, key_hi, false));  // on the context's stream, like the fix-up
    if (!c->ones.p) {
      CHK(c->ones.ensure(8192));
      HIPCHK(hipMemsetAsync(c->ones.p, 0xFF, 8192, c->stream));
    }
    Operand A, B;
    CHK(resolve(c, ia, ma, &A));
    CHK(resolve(c, ib, mb, &B));
    CHK(join_result(c));
    launch_ior_fix(c->stream, c->r().ntasks.as<uint32_t>(), c->r().recs.as<ORec>(), A, B, c->ones.as<uint8_t>());
    HIPCHK(hipGetLastError());
    c->r().agg_ok = false;  // k_ior_fix changed records after the compute kernel summed them
    return RBG_OK;
  }
  if (op < 0 || op > 3) return RBG_ERR_ILLEGAL_ARGUMENT;
  key_lo = std::max(0, key_lo);
  key_hi = std::min(kMaxKeys, key_hi);
  Operand A, B;
  CHK(resolve(c, ia, ma, &A));
  CHK(resolve(c, ib, mb, &B));
  const int plan_op = card_only ? OP_AND : op;
  size_t ub;
  switch (plan_op) {
    case OP_AND: ub = std::min(A.n, B.n); break;
    case OP_ANDNOT: ub = A.n; break;
    default: ub = std::min<size_t>((size_t)A.n + B.n, kMaxKeys); break;
  }
  // Dense key ranges (the op's task bound covers at least half of the range) take every key of the
  // range as a task (one record and scratch slot per key, key key_lo + t at position t).  Sparse ones
  // are planned and compacted first, so the kernel sees only keys with work.
  const size_t nkeys = key_hi > key_lo ? (size_t)(key_hi - key_lo) : 0;
  const bool dense = nkeys > 0 && 2 * ub >= nkeys;
  OutCtx oc;
  CHK(prepare_output(c, dense ? std::max(ub, nkeys) : ub, A.b->payload_bytes + B.b->payload_bytes + kStagedMax * ub,
                     &oc, card_only, lanes));
  hipStream_t s = c->r().stream;  // the set's own
  c->r().pending_src = {ia, ib};
  c->mark(0);
  const PwDirect pd{key_lo};
  const PlanOut po = plan_out(c, !dense);
  if (dense) {
    // tasks binned by estimated cost so every wave draws the same mix (k_plan_balanced)
    // ... run by one 16-wave workgroup per CU that claims the CU's tasks through LDS (k_pair_cu)
    launch_plan_balanced(s, plan_op, card_only ? 1 : 0, key_lo, (uint32_t)nkeys, A, B, po, oc,
                         c->r().task_card.as<uint32_t>());
  } else {
    launch_plan_pairwise(s, plan_op, key_lo, key_hi, A, B, po, oc.err);
    dbg(s, "plan");
  }
  c->mark(1);
  // the compute kernel sums its kept results per tile for the serialization (k_serialize_agg): either
  // plan kernel has zeroed the sums first
  if (!card_only) {
    oc.tile_agg = reinterpret_cast<unsigned long long*>(oc.tile_status + 2 * kMaxTiles);
    c->r().pending.tile_agg = oc.tile_agg;
    c->r().agg_ok = true;
  }
  // 4 waves (tasks) per workgroup, clamped to the resident grid
  const int grid = grid_for(((dense ? nkeys : ub) + 3) / 4, 16384);
  launch_pairwise(s, op, card_only ? 1 : 0, grid, po.tasks, po.n_tasks, A.payload, B.payload, oc,
                  c->r().task_card.as<uint32_t>(), dense ? &pd : nullptr);
  dbg(s, "pairwise");
  c->mark(2);
  if (card_only) {
    launch_reduce_card(s, c->r().task_card.as<uint32_t>(), c->r().ntasks.as<uint32_t>(), c->r().info.as<ResultInfo>(), oc.err);
    c->r().last = 2;
  } else {
    defer_place(c);
  }
  c->mark(3);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}


// Host index of a batch's containers, built once per batch: the container table and,
// per input bitmap, its container positions (in key order).
int batch_host_index(Ctx* c, Batch* b) {
  if (b->h_index) return RBG_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  b->h_desc.resize(b->n_ctr);
  if (b->n_ctr) HIPCHK(hipMemcpy(b->h_desc.data(), b->desc.p, sizeof(CDesc) * b->n_ctr, hipMemcpyDeviceToHost));
  b->h_pos_off.assign(b->n_bm + 1, 0);
  b->h_pos.resize(b->n_ctr);
  if ((b->n_bm == 1 || !b->key_major) && b->h_bm_off.size() == b->n_bm + 1) {
    for (size_t i = 0; i <= b->n_bm; i++) b->h_pos_off[i] = b->h_bm_off[i];
    for (size_t p = 0; p < b->n_ctr; p++) b->h_pos[p] = (uint32_t)p;
  } else {  // key-major: counting sort of the positions by input bitmap (stable, so key order)
    std::vector<uint32_t> bm(b->n_ctr);
    if (b->n_ctr) HIPCHK(hipMemcpy(bm.data(), b->bm.p, 4 * b->n_ctr, hipMemcpyDeviceToHost));
    for (uint32_t x : bm) b->h_pos_off[x + 1]++;
    for (size_t i = 0; i < b->n_bm; i++) b->h_pos_off[i + 1] += b->h_pos_off[i];
    std::vector<uint32_t> fill(b->h_pos_off.begin(), b->h_pos_off.end() - 1);
    for (size_t p = 0; p < b->n_ctr; p++) b->h_pos[fill[bm[p]]++] = (uint32_t)p;
  }
  b->h_index = true;
  return RBG_OK;
}

int ctx_info(Ctx* c, ResultInfo* ri) {
  CHK(join_result(c));
  if (c->r().last == 1) CHK(ensure_placed(c));
  HIPCHK(hipMemcpyAsync(ri, c->r().info.p, sizeof(ResultInfo), hipMemcpyDeviceToHost, c->stream));
  uint64_t card = 0;
  uint32_t err = 0;
  if (c->r().last == 1)  // materialised result: k_place / the pairwise placer accumulated its cardinality
    HIPCHK(hipMemcpyAsync(&card, c->r().lb.as<uint8_t>() + 64 + 8 * kCardWord, 8, hipMemcpyDeviceToHost, c->stream));
  if (c->r().last == 1 || c->r().last == 2)  // spin timeouts of any kernel of the op
    HIPCHK(hipMemcpyAsync(&err, c->r().lb.as<uint8_t>() + 64, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->r().last == 1) {
    ri->long_card = (int64_t)card;
    ri->card32 = (uint32_t)card;
  }
  ri->err |= err;
  if ((c->r().last == 1 || c->r().last == 2) && ri->err) {
    set_err("a look-back spin of the op's plan or placement timed out: the result is invalid");
    return RBG_ERR_DEVICE;
  }
  if (c->r().last == 1) {
    c->r().last_ri = *ri;
    c->r().ri_valid = true;
  }
  return RBG_OK;
}

// Device -> host copy of a large result into caller (pageable) memory: 32 MiB groups DMA'd into
// the context's pinned staging, each copied out by worker threads as soon as its event fires, so
// the DMA of the next groups overlaps the host copies (the mirror of stage_upload).
static int download_staged(Ctx* c, const uint8_t* dev, uint64_t bytes, uint8_t* dst) {
  constexpr uint64_t kGroup = 32ull << 20;
  hipStream_t s = c->stream;
  if (bytes <= kGroup) {
    HIPCHK(hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RBG_OK;
  }
  CHK(pinned_ensure(c, bytes + 64));
  uint8_t* pin = reinterpret_cast<uint8_t*>(c->pinned);
  const uint32_t groups = (uint32_t)((bytes + kGroup - 1) / kGroup);
  std::vector<hipEvent_t> ev(groups);
  for (auto& e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  int st = RBG_OK;
  for (uint32_t g = 0; g < groups; g++) {
    const uint64_t lo = (uint64_t)g * kGroup, hi = std::min<uint64_t>(bytes, lo + kGroup);
    if (hipMemcpyAsync(pin + lo, dev + lo, hi - lo, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipEventRecord(ev[g], s) != hipSuccess) {
      set_err("device-to-host copy of the result failed");
      st = RBG_ERR_DEVICE;
      break;
    }
  }
  if (st == RBG_OK) {
    std::atomic<uint32_t> next{0};
    std::atomic<int> bad{0};
    const int nthr = (int)std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 0; t < nthr; t++)
      th.emplace_back([&]() {
        for (uint32_t g; (g = next.fetch_add(1)) < groups;) {
          if (hipEventSynchronize(ev[g]) != hipSuccess) {
            bad.store(1);
            continue;
          }
          const uint64_t lo = (uint64_t)g * kGroup, hi = std::min<uint64_t>(bytes, lo + kGroup);
          std::memcpy(dst + lo, pin + lo, hi - lo);
        }
      });
    for (auto& x : th) x.join();
    if (bad.load()) {
      set_err("device-to-host copy of the result failed");
      st = RBG_ERR_DEVICE;
    }
  }
  (void)hipStreamSynchronize(s);
  for (auto& e : ev) (void)hipEventDestroy(e);
  return st;
}

// Large result buffers (a serialized C2 AND result is 0.25 GB): 2 MiB-aligned with transparent
// huge pages, so first touch faults once per 2 MiB instead of once per 4 KiB, and rbg_free keeps up
// to two of them for the next large result (a fresh buffer's pages are faulted and zeroed by the
// kernel on first touch: tens of ms for 0.25 GB, more than its PCIe download).
static std::mutex g_out_mu;
static std::unordered_map<void*, size_t> g_out_live;        // large buffers handed out -> capacity
static std::vector<std::pair<void*, size_t>> g_out_cache;   // freed ones kept for reuse
// The cache holds at most two buffers and 1 GiB; rbg_trim releases it.
constexpr size_t kOutLarge = 8ull << 20, kOutCacheMax = 2, kOutCacheBytes = 1ull << 30, kOutAlign = 2ull << 20;
static size_t out_cache_bytes() {
  size_t b = 0;
  for (const auto& e : g_out_cache) b += e.second;
  return b;
}
uint8_t* out_alloc(size_t n) {
  if (n < kOutLarge) return (uint8_t*)std::malloc(n ? n : 1);
  std::lock_guard<std::mutex> g(g_out_mu);
  for (size_t i = 0; i < g_out_cache.size(); i++) {
    const auto e = g_out_cache[i];
    if (e.second >= n && e.second <= 2 * n + kOutAlign) {
      g_out_cache.erase(g_out_cache.begin() + (std::ptrdiff_t)i);
      g_out_live[e.first] = e.second;
      return (uint8_t*)e.first;
    }
  }
  const size_t cap = (n + kOutAlign - 1) & ~(kOutAlign - 1);
  void* p = nullptr;
  if (posix_memalign(&p, kOutAlign, cap) != 0) return nullptr;
  (void)madvise(p, cap, MADV_HUGEPAGE);
  g_out_live[p] = cap;
  return (uint8_t*)p;
}

int ctx_fetch(Ctx* c, rbg_buffer* out) {
  if (c->r().last != 1) {
    set_err("no serialized result pending");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  CHK(ctx_serialize(c, true));  // consumed at once: on the context's stream (a no-op if already serialized)
  ResultInfo ri;
  CHK(ctx_info(c, &ri));  // joins the set's stream
  uint8_t* p = out_alloc(ri.total);
  if (!p) return RBG_ERR_OUT_OF_MEMORY;
  out->data = p;
  out->len = ri.total;
  const int st = download_staged(c, c->r().result.as<uint8_t>() + ri.start, ri.total, p);
  if (st != RBG_OK) {
    rbg_free(out);
    return st;
  }
  return RBG_OK;
}

// Download bitmaps [i0, i1) of a batch as portable serialized bytes: their slots are
// gathered on the device into one buffer (one D2H copy), the headers built here.
int ctx_batch_fetch_range(Ctx* c, int32_t batch, size_t i0, size_t i1, rbg_buffer* outs) {
  Batch* b;
  CHK(get_batch(c, batch, &b));
  if (i0 > i1 || i1 > b->n_bm || (i1 > i0 && !outs)) return RBG_ERR_ILLEGAL_ARGUMENT;
  CHK(batch_host_index(c, b));
  const std::vector<CDesc>& D = b->h_desc;
  // slots are consecutive in container order: a slot ends where the next one starts
  auto slot_end = [&](uint32_t p) -> uint64_t { return p + 1 < b->n_ctr ? D[p + 1].slot : b->payload_bytes; };
  std::vector<GatherItem> items;
  uint64_t tot = 0;
  for (size_t i = i0; i < i1; i++)
    for (uint32_t k = b->h_pos_off[i]; k < b->h_pos_off[i + 1]; k++) {
      const uint32_t p = b->h_pos[k];
      const uint64_t len = slot_end(p) - D[p].slot;
      items.push_back(GatherItem{D[p].slot, tot, len});
      tot = round16(tot + len);
    }
  std::vector<uint8_t> pay(tot + 16);
  if (!items.empty()) {
    CHK(c->gather_items.ensure(sizeof(GatherItem) * items.size()));
    CHK(c->gather_out.ensure(tot + 16));
    HIPCHK(hipMemcpyAsync(c->gather_items.p, items.data(), sizeof(GatherItem) * items.size(), hipMemcpyHostToDevice,
                          c->stream));
    launch_gather(c->stream, c->gather_items.as<GatherItem>(), items.size(), b->payload.as<uint8_t>(),
                  c->gather_out.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pay.data(), c->gather_out.p, tot, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  size_t it = 0;
  for (size_t i = i0; i < i1; i++) {
    const uint32_t k0 = b->h_pos_off[i], n = b->h_pos_off[i + 1] - k0;
    bool has_run = false;
    std::vector<uint32_t> lens(n);
    for (uint32_t k = 0; k < n; k++) {
      const CDesc& d = D[b->h_pos[k0 + k]];
      has_run |= d.kind == KR;
      if (d.kind == KA) lens[k] = 2 * d.card;
      else if (d.kind == KB) lens[k] = 8192;
      else {
        const uint8_t* q = pay.data() + items[it + k].dst + 2;
        lens[k] = 2 + 4 * (uint32_t)(q[0] | (q[1] << 8));
      }
    }
    std::vector<uint8_t> o;
    auto put16 = [&](uint32_t v) { o.push_back((uint8_t)v); o.push_back((uint8_t)(v >> 8)); };
    auto put32 = [&](uint32_t v) { for (int j = 0; j < 4; j++) o.push_back((uint8_t)(v >> (8 * j))); };
    if (has_run) {
      put32(12347u | (uint32_t)((n - 1) << 16));
      std::vector<uint8_t> fl((n + 7) / 8, 0);
      for (uint32_t k = 0; k < n; k++)
        if (D[b->h_pos[k0 + k]].kind == KR) fl[k / 8] |= (uint8_t)(1u << (k % 8));
      o.insert(o.end(), fl.begin(), fl.end());
    } else {
      put32(12346u);
      put32(n);
    }
    for (uint32_t k = 0; k < n; k++) {
      const CDesc& d = D[b->h_pos[k0 + k]];
      put16(d.key);
      put16(d.card - 1);
    }
    if (!has_run || n >= 4) {
      uint32_t start = (uint32_t)header_size(n, has_run);
      for (uint32_t k = 0; k < n; k++) {
        put32(start);
        start += lens[k];
      }
    }
    for (uint32_t k = 0; k < n; k++) {
      const uint8_t* q = pay.data() + items[it + k].dst + (D[b->h_pos[k0 + k]].kind == KR ? 2 : 0);
      o.insert(o.end(), q, q + lens[k]);
    }
    it += n;
    const int st = emit_host(o, &outs[i - i0]);
    if (st != RBG_OK) {
      for (size_t j = i0; j < i; j++) rbg_free(&outs[j - i0]);
      return st;
    }
  }
  return RBG_OK;
}

int ctx_batch_card(Ctx* c, int32_t id) {
  Batch* B;
  CHK(get_batch(c, id, &B));
  if (B->packed) {
    set_err("batched andCardinality needs slot-aligned payloads");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (B->n_bm % 2 != 0) {
    set_err("batched andCardinality needs an even number of bitmaps");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const size_t np = B->n_bm / 2;
  CHK(main_set(c));  // takes no set of its own: set 0's `last` changes
  CHK(c->cards.ensure(4 * std::max<size_t>(np, 1)));
  if (B->key_major && B->n_bm > 1) {
    // pairs need bitmap-major ranges: permuted view of a key-major batch is not supported
    set_err("batched andCardinality needs a bitmap-major batch");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  c->mark(0);
  c->mark(1);
  if (!B->pair_cap_known) {
    B->pair_items_cap = batch_pair_items_cap(B->h_bm_nctr.data(), np);
    B->pair_cap_known = true;
  }
  CHK(c->pc_cnt.ensure(8 * ((np + 255) / 256) + std::max<size_t>(np, 1) + 16));  // workgroup totals + a count byte per pair
  CHK(c->pc_part.ensure(8 * (scan_parts(std::max<size_t>(np, 1)) + 1)));
  CHK(c->pc_items.ensure(sizeof(PairItem) * std::max<uint64_t>(B->pair_items_cap, 1)));
  CHK(c->pc_large.ensure(4 * std::max<size_t>(np, 1)));
  CHK(c->scalar.ensure(64));
  launch_batch_and_card(c->stream, np, B->bm_off.as<uint32_t>(), B->keys.as<uint16_t>(), B->desc.as<CDesc>(),
                        B->payload.as<uint8_t>(), c->cards.as<int32_t>(), c->pc_cnt.as<uint64_t>(),
                        c->pc_part.as<uint64_t>(), c->scalar.as<uint64_t>() + 7, c->pc_items.as<PairItem>(),
                        c->pc_large.as<uint32_t>());
  c->mark(2);
  c->mark(3);
  HIPCHK(hipGetLastError());
  c->n_cards = np;
  c->r().last = 3;
  return RBG_OK;
}

// Key-shard placement of the pending result inside a global portable bitmap of
// total_containers containers, enqueued on the context stream.
int ctx_fetch_shard_device(Ctx* c, int64_t total_containers, int has_run, int64_t payload_base, void* desc_dst,
                           void* offsets_dst, void* runflag_dst, void* payload_dst) {
  if (c->r().last != 1) {
    set_err("no materialised result pending");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (total_containers < 0 || total_containers > kMaxKeys || payload_base < 0 || !desc_dst || !payload_dst) {
    set_err("fetch_shard: bad layout or null destination");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const bool offsets = !has_run || total_containers >= 4;  // RB/RoaringArray.java:927-933
  if (offsets && !offsets_dst) {
    set_err("fetch_shard: the global bitmap has an offset table; offsets_dst is required");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  // the result's facts: read by the result_stats call that sized the global layout (which also
  // reported a timed-out spin as RBG_ERR_DEVICE), so the fetch stays asynchronous; without one,
  // ctx_info synchronises here
  ResultInfo ri;
  CHK(join_result(c));
  if (c->r().ri_valid) {
    ri = c->r().last_ri;
    CHK(ensure_placed(c));
  } else {
    CHK(ctx_info(c, &ri));
  }
  const uint64_t off0 = header_size((size_t)total_containers, has_run != 0) + (uint64_t)payload_base;
  if (off0 > 0xFFFFFFFFull) {
    set_err("fetch_shard: payload offsets exceed 32 bits");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  uint8_t* emit_dst = (uint8_t*)payload_dst;
  if (c->r().serialized) {
    // already serialized (possibly because an operand batch was released since): copy the
    // payload region rather than re-reading the operands' pass-through containers
    if (ri.payload)
      HIPCHK(hipMemcpyAsync(payload_dst, c->r().result.as<uint8_t>() + c->r().pending.payload_base, ri.payload,
                            hipMemcpyDeviceToDevice, c->stream));
    emit_dst = nullptr;
  }
  launch_serialize_shard(c->stream, grid_for((c->r().pending_ub + 255) / 256, 256), c->r().ntasks.as<uint32_t>(), c->r().pending,
                         emit_dst, off0, (uint8_t*)desc_dst, offsets ? (uint8_t*)offsets_dst : nullptr,
                         has_run ? (uint8_t*)runflag_dst : nullptr);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// RoaringBitmap.runOptimize (RB/RoaringBitmap.java:2764-2774) over every bitmap of a
// batch, into a new batch: plan (new kind + slot size per container), scan of the
// slot sizes, write.  answers[i] = 1 iff bitmap i holds a run container afterwards.

int ctx_run_optimize(Ctx* c, int32_t id, int32_t* out_id, uint8_t* answers) {
  Batch* a;
  CHK(get_batch(c, id, &a));
  if (a->packed) {
    set_err("runOptimize needs slot-aligned payloads (not a packed synthetic batch)");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  hipStream_t s = c->stream;
  const size_t C = a->n_ctr, n = a->n_bm;
  // one kernel: every container is written at its own slot offset (a conversion never makes a slot
  // larger), so the new batch has the input's payload size and layout and nothing waits on the host
  const int32_t bid = new_batch(c);
  Batch& b = *c->batches[bid];
  struct Drop {  // an error below frees the half-built batch
    Ctx* c;
    int32_t id;
    bool keep = false;
    ~Drop() {
      if (!keep) c->batches[id].reset();
    }
  } drop{c, bid};
  CHK(pool_take(c, b.desc, sizeof(CDesc) * C + 16));
  CHK(pool_take(c, b.payload, a->payload_bytes + 64));
  b.ro_groups = runopt_groups(C);
  CHK(pool_take(c, b.ro_stats, ro_flags_off(b.ro_groups) + 4 * n + 16));
  CHK(pool_take(c, b.keys, a->keys.cap));
  CHK(pool_take(c, b.bm, a->bm.cap));
  CHK(pool_take(c, b.key_off, a->key_off.cap));
  CHK(pool_take(c, b.bm_off, a->bm_off.cap));
  const RoCopy cp{a->keys.as<uint16_t>(), b.keys.as<uint16_t>(), a->bm.as<uint32_t>(), b.bm.as<uint32_t>(),
                  a->key_off.as<uint32_t>(), b.key_off.as<uint32_t>(), a->key_off.cap / 4,
                  a->bm_off.as<uint32_t>(), b.bm_off.as<uint32_t>(), a->bm_off.cap / 4};
  if (C)
    launch_runopt(s, a->desc.as<CDesc>(), a->payload.as<uint8_t>(), C, b.desc.as<CDesc>(), b.payload.as<uint8_t>(), cp,
                  b.ro_stats.as<unsigned long long>() + 8);
  HIPCHK(hipGetLastError());
  // no host read-back here: the new batch's statistics stay on the device until needed (ensure_stats)
  b.n_bm = n;
  b.n_ctr = C;
  b.key_major = a->key_major;
  b.h_bm_off = a->h_bm_off;
  b.h_bm_nctr = a->h_bm_nctr;
  b.h_bm_card = a->h_bm_card;
  b.long_card = a->long_card;
  b.bsi_min = a->bsi_min;
  b.bsi_max = a->bsi_max;
  b.payload_bytes = a->payload_bytes;  // the input's layout (holes after shrunk containers)
  b.gapped = a->gapped || a->n_kind[DK_R] > 0;  // only R -> A can leave an all-array batch with holes
  b.max_ser = 0;  // runOptimize leaves no container above kStagedMax serialized bytes
  b.ser_bytes = a->ser_bytes ? 1 : 0;  // nonzero: computed by ensure_stats
  b.stats_pending = true;
  b.live = true;
  drop.keep = true;
  *out_id = bid;
  if (answers) {  // runOptimize's boolean per bitmap: the statistics now
    CHK(ensure_stats(c, &b));
    for (size_t i = 0; i < n; i++) answers[i] = b.h_has_run[i];
  }
  return RBG_OK;
}

// selectRangeWithoutCopy (RB/RoaringBitmap.java:3160-3214) of every bitmap of a key-major batch into a
// new batch, on the device (runopt.hip: k_rsel_plan, two scans, k_rsel_write, the key CSR); one host
// read-back for the new batch's container counts.  rangeSanityCheck (:204-213) first.
// x.selectRange(rangeStart, rangeEnd) (RB/RoaringBitmap.java:3095-3147; buffer RB/buffer/ImmutableRoaringBitmap.java
// :701-757): no rangeSanityCheck (the range aggregations, which do check, call check_range first); the high and
// low bits are the reference's char casts of rangeStart and rangeEnd - 1 (Util.highbits / lowbits, RB/Util.java
// :436-438,481-483), so selectRange(x, Long.MAX_VALUE) keeps [start, 0xFFFFFFFF).  Divergences, raised as
// IllegalArgumentException: a negative bound (the reference's assert) and casts that put the last key below the
// first (the reference would append keys out of order).
int ctx_select_range(Ctx* c, int32_t id, int64_t start, int64_t end, int32_t* out_id, bool buf) {
  if (start < 0 || end < 0) {
    set_err("selectRange: rangeStart and rangeEnd must not be negative");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (end > start && ((uint64_t)start >> 16 & 0xFFFF) > ((uint64_t)(end - 1) >> 16 & 0xFFFF)) {
    set_err("selectRange: the range's key casts are out of order (the reference would build an unsorted bitmap)");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  Batch* a;
  CHK(get_batch(c, id, &a));
  if (!a->key_major || a->packed) {
    set_err("range selection needs a key-major batch with slot-aligned payloads");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  hipStream_t s = c->stream;
  const size_t C = a->n_ctr, n = a->n_bm;
  RselArgs ra{1, 0, 0, 0, buf ? 1 : 0};  // end <= start: no key is kept
  if (end > start) {  // (char) casts: Util.highbits / lowbits
    ra.hbs = (int)((uint64_t)start >> 16 & 0xFFFF);
    ra.lbs = (int)(start & 0xFFFF);
    ra.hbl = (int)((uint64_t)(end - 1) >> 16 & 0xFFFF);
    ra.lbl = (int)((end - 1) & 0xFFFF);
  }
  CHK(c->ro_info.ensure(4 * C + 16));
  CHK(c->ro_size.ensure(8 * C + 16));
  CHK(c->ro_part.ensure(8 * (scan_parts(std::max<size_t>(C, 1)) + 1)));
  CHK(c->rs_card.ensure(4 * C + 16));
  CHK(c->rs_keep.ensure(8 * C + 16));
  CHK(c->rs_bm.ensure(16 * n + 64 + 16));  // per bitmap: kept containers, cardinality; then the totals
  const int32_t bid = new_batch(c);
  Batch& b = *c->batches[bid];
  BatchGuard guard{c, {bid}};  // dropped unless the selection completes
  CHK(pool_take(c, b.desc, sizeof(CDesc) * C + 16));
  CHK(pool_take(c, b.payload, a->payload_bytes + 64));
  CHK(b.keys.ensure(2 * C + 16));
  CHK(b.bm.ensure(4 * C + 16));
  CHK(b.key_off.ensure(4 * (kMaxKeys + 1)));
  CHK(b.bm_off.ensure(4 * (n + 1)));
  unsigned long long* bm_cnt = c->rs_bm.as<unsigned long long>();
  unsigned long long* bm_card = bm_cnt + n;
  unsigned long long* tot = bm_cnt + 2 * n;  // #A, #B, #R, big bytes, then the two scan totals
  HIPCHK(hipMemsetAsync(c->rs_bm.p, 0, 16 * n + 64, s));
  launch_rsel_plan(s, a->desc.as<CDesc>(), a->bm.as<uint32_t>(), a->payload.as<uint8_t>(), C, ra,
                   c->ro_info.as<uint32_t>(), c->rs_card.as<uint32_t>(), c->ro_size.as<uint64_t>(),
                   c->rs_keep.as<uint64_t>(), bm_cnt, bm_card, tot);
  launch_exclusive_scan(s, c->ro_size.as<uint64_t>(), c->ro_size.as<uint64_t>(), C, c->ro_part.as<uint64_t>(),
                        reinterpret_cast<uint64_t*>(tot + 4));
  launch_exclusive_scan(s, c->rs_keep.as<uint64_t>(), c->rs_keep.as<uint64_t>(), C, c->ro_part.as<uint64_t>(),
                        reinterpret_cast<uint64_t*>(tot + 5));
  launch_rsel_write(s, a->desc.as<CDesc>(), a->bm.as<uint32_t>(), a->payload.as<uint8_t>(), C, ra,
                    c->ro_info.as<uint32_t>(), c->rs_card.as<uint32_t>(), c->ro_size.as<uint64_t>(),
                    c->rs_keep.as<uint64_t>(), b.desc.as<CDesc>(), b.keys.as<uint16_t>(), b.bm.as<uint32_t>(),
                    b.payload.as<uint8_t>());
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> h(2 * n + 8);
  HIPCHK(hipMemcpyAsync(h.data(), c->rs_bm.p, 8 * (2 * n + 6), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const unsigned long long* t = h.data() + 2 * n;
  const uint64_t C2 = t[5];
  launch_dec_key_off(s, b.keys.as<uint16_t>(), C2, b.key_off.as<uint32_t>());
  b.n_bm = n;
  b.n_ctr = C2;
  b.key_major = true;
  for (int k = 0; k < 3; k++) b.n_kind[k] = (int64_t)t[k];
  b.max_ser = t[3];
  b.payload_bytes = t[4];
  b.h_bm_off.assign(n + 1, 0);
  b.h_bm_nctr.resize(n);
  b.h_bm_card.resize(n);
  for (size_t i = 0; i < n; i++) {
    b.h_bm_nctr[i] = (uint32_t)h[i];
    b.h_bm_off[i + 1] = b.h_bm_off[i] + (uint32_t)h[i];
    b.h_bm_card[i] = (int64_t)h[n + i];
    b.long_card += (int64_t)h[n + i];
  }
  HIPCHK(hipMemcpyAsync(b.bm_off.p, b.h_bm_off.data(), 4 * (n + 1), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));  // the host vector above goes out of scope
  HIPCHK(hipGetLastError());
  b.live = true;
  guard.ids.clear();
  *out_id = bid;
  return RBG_OK;
}

// HIP-event phase timing of the next max_ops ops (Ctx::mark); max_ops <= 0 turns it off
int ctx_profile(Ctx* c, int max_ops, bool compute_only) {
  CHK(sync_streams(c));
  c->prof_free();
  c->prof_compute_only = compute_only;
  if (max_ops <= 0) return RBG_OK;
  c->prof_ev.resize(4 * (size_t)max_ops);
  for (hipEvent_t& e : c->prof_ev) HIPCHK(hipEventCreate(&e));
  c->prof_cap = (size_t)max_ops;
  c->prof_n = 0;
  CHK(c->rd_ctr.ensure(8));
  HIPCHK(hipMemsetAsync(c->rd_ctr.p, 0, 8, c->stream));
  return RBG_OK;
}

// ---------------------------------------------------------------------------
// thread-local one-shot contexts
// ---------------------------------------------------------------------------
static std::mutex g_dev_mu;
static uint64_t g_dev_mask = 1;

struct TLCtx {
  std::unique_ptr<Ctx> ctx;
  int device = -1;
};
static thread_local TLCtx tl;

int tl_ctx(Ctx** out) {
  int dev;
  {
    std::lock_guard<std::mutex> g(g_dev_mu);
    uint64_t m = g_dev_mask;
    dev = m ? __builtin_ctzll(m) : 0;
  }
  if (!tl.ctx || tl.device != dev) {
    std::unique_ptr<Ctx> c(new Ctx());
    CHK(ctx_init(c.get(), dev));
    tl.ctx = std::move(c);
    tl.device = dev;
  }
  CHK(enter(tl.ctx.get()));
  *out = tl.ctx.get();
  return RBG_OK;
}

}  // namespace rbg

// The entry points that only read or write the process-wide state above: the error text, the eviction count,
// the one-shot device mask, the output-buffer cache.
using namespace rbg;

extern "C" {

void rbg_trim(void) {
  std::lock_guard<std::mutex> g(g_out_mu);
  for (const auto& e : g_out_cache) std::free(e.first);
  g_out_cache.clear();
}

uint64_t rbg_pool_evictions(void) { return g_pool_evictions.load(); }
const char* rbg_last_error(void) { return g_err.c_str(); }

void rbg_free(rbg_buffer* buf) {
  if (!buf) return;
  if (buf->data) {
    std::lock_guard<std::mutex> g(g_out_mu);
    const auto it = g_out_live.find(buf->data);
    if (it != g_out_live.end()) {  // a large result buffer: kept for reuse (the oldest kept one freed)
      g_out_cache.emplace_back(it->first, it->second);
      g_out_live.erase(it);
      while (g_out_cache.size() > kOutCacheMax || (!g_out_cache.empty() && out_cache_bytes() > kOutCacheBytes)) {
        std::free(g_out_cache.front().first);
        g_out_cache.erase(g_out_cache.begin());
      }
      buf->data = nullptr;
      buf->len = 0;
      return;
    }
  }
  std::free(buf->data);
  buf->data = nullptr;
  buf->len = 0;
}

int rbg_set_devices(uint64_t mask) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    set_err("no HIP device");
    return RBG_ERR_DEVICE;
  }
  uint64_t usable = mask & ((n >= 64) ? ~0ULL : ((1ULL << n) - 1));
  if (!usable) {
    set_err("device mask selects no present device");
    return RBG_ERR_DEVICE;
  }
  std::lock_guard<std::mutex> g(g_dev_mu);
  g_dev_mask = usable;
  return __builtin_popcountll(usable);
}

}  // extern "C"
