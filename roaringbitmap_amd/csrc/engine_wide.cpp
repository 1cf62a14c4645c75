// The aggregations over a key-major batch (engine.hpp: the host units): FastAggregation's dispatch (ctx_wide),
// the chain order of the horizontal forms and the priority-queue forms (pq.hip).
#include <algorithm>
#include <utility>

#include "engine.hpp"

namespace rbg {

// Chain order of horizontal_or / horizontal_xor (RB/FastAggregation.java:124-289): the
// reference drains a java.util.PriorityQueue of one container pointer per bitmap, ordered
// by key, then larger cardinality first (RB/RoaringArray.java:708-713), with the heap's own
// tie order.  The heap is replayed here over the container table (keys and cardinalities
// only -- no payload); order[key_off[k] + j] = the j-th container of key k's chain.
// *identity: the chain order is the batch's own (no key needed sorting): no order table
static int horizontal_order(Ctx* c, Batch* B, bool* identity) {
  *identity = B->h_chain_identity;
  if (*identity) return RBG_OK;
  CHK(batch_host_index(c, B));
  std::vector<uint32_t> order;
  // Within a key the heap pops by larger cardinality first; only equal cardinalities pop in
  // the heap's tie order, which depends on everything polled before.  The chain's order
  // matters only at keys holding a run container (the wide kernel types run-free keys from
  // the result alone, wide.hip), so unless such a key has two containers of equal
  // cardinality the order is the per-key sort by cardinality and the replay is skipped.
  if (B->key_major || B->n_bm == 1) {
    const std::vector<CDesc>& D = B->h_desc;
    const size_t n = B->n_ctr;
    std::vector<std::pair<uint32_t, uint32_t>> rkeys;  // segments of keys holding a run container
    std::vector<uint32_t> seg;
    bool tie = false;
    for (size_t p = 0; p < n && !tie;) {
      size_t e = p;
      bool has_r = false;
      while (e < n && D[e].key == D[p].key) has_r |= D[e++].kind == DK_R;
      if (has_r && e - p > 1) {
        seg.resize(e - p);
        for (size_t q = p; q < e; q++) seg[q - p] = D[q].card;
        std::sort(seg.begin(), seg.end());
        tie = std::adjacent_find(seg.begin(), seg.end()) != seg.end();
        rkeys.emplace_back((uint32_t)p, (uint32_t)e);
      }
      p = e;
    }
    if (!tie && rkeys.empty()) {
      *identity = B->h_chain_identity = true;
      return RBG_OK;
    }
    if (!tie) {
      order.resize(n);
      for (size_t q = 0; q < n; q++) order[q] = (uint32_t)q;
      for (const auto& pe : rkeys)
        std::sort(order.begin() + pe.first, order.begin() + pe.second,
                  [&](uint32_t x, uint32_t y) { return D[x].card > D[y].card; });
      CHK(c->order.ensure(4 * std::max<size_t>(n, 1)));
      if (n) HIPCHK(hipMemcpyAsync(c->order.p, order.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));  // `order` is a stack vector
      return RBG_OK;
    }
    order.clear();
  }
  order.reserve(B->n_ctr);
  auto ptr = [&](uint32_t bm, uint32_t i) {
    const uint32_t pos = B->h_pos[B->h_pos_off[bm] + i];
    const CDesc& d = B->h_desc[pos];
    return HPtr{bm, i, d.key, d.card, pos};
  };
  auto has = [&](uint32_t bm, uint32_t i) { return B->h_pos_off[bm] + i < B->h_pos_off[bm + 1]; };
  JHeap pq;
  for (uint32_t b = 0; b < B->n_bm; b++)
    if (has(b, 0)) pq.add(ptr(b, 0));
  auto advance_add = [&](const HPtr& x) {
    if (has(x.bm, x.i + 1)) pq.add(ptr(x.bm, x.i + 1));
  };
  while (!pq.q.empty()) {
    const HPtr x1 = pq.poll();
    order.push_back(x1.pos);
    if (pq.q.empty() || pq.q[0].key != x1.key) {
      advance_add(x1);
      continue;
    }
    const HPtr x2 = pq.poll();
    order.push_back(x2.pos);
    while (!pq.q.empty() && pq.q[0].key == x1.key) {
      const HPtr x = pq.poll();
      order.push_back(x.pos);
      if (has(x.bm, x.i + 1)) pq.add(ptr(x.bm, x.i + 1));
      else if (pq.q.empty()) break;
    }
    advance_add(x1);
    advance_add(x2);
  }
  if (order.size() != B->n_ctr) {
    set_err("horizontal order: container table inconsistent");
    return RBG_ERR_DEVICE;
  }
  CHK(c->order.ensure(4 * std::max<size_t>(order.size(), 1)));
  if (!order.empty())
    HIPCHK(hipMemcpyAsync(c->order.p, order.data(), 4 * order.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // `order` is a stack vector
  return RBG_OK;
}

// FastAggregation.priorityqueue_or / priorityqueue_xor (RB/FastAggregation.java:677-812).
// The reference keeps a java.util.PriorityQueue of bitmaps ordered by
// (int)(sizes[a] - sizes[b]) over getLongSizeInBytes.  The host adds the inputs and plans
// the first step; the queue then runs on the device (pq.hip): N - 1 step launches, each
// planning the next, with no host read-back in between.
namespace {
// host side of the queue for the first step (same operations as pq.hip's PQWave)
struct PQHost {
  std::vector<PQEnt>& heap;
  std::vector<int32_t>& nodes;
  std::vector<uint8_t>& tmp;
  std::vector<int32_t>& slots;
  void add(PQStep& c, PQEnt x) {  // OpenJDK PriorityQueue.siftUp
    int k = c.heap_n++;
    while (k > 0) {
      const int p = (k - 1) >> 1;
      if (pq_cmp(x.size, heap[p].size) >= 0) break;
      heap[k] = heap[p];
      k = p;
    }
    heap[k] = x;
  }
  PQEnt poll(PQStep& c) {  // PriorityQueue.poll + siftDown
    const PQEnt r = heap[0];
    const int n = --c.heap_n;
    if (n == 0) return r;
    const PQEnt x = heap[n];
    int k = 0;
    const int half = n >> 1;
    while (k < half) {
      int ch = 2 * k + 1;
      if (ch + 1 < n && pq_cmp(heap[ch].size, heap[ch + 1].size) > 0) ch++;
      if (pq_cmp(x.size, heap[ch].size) <= 0) break;
      heap[k] = heap[ch];
      k = ch;
    }
    heap[k] = x;
    return r;
  }
  int32_t node(int i) { return nodes[i]; }
  void set_node(int i, int32_t v) { nodes[i] = v; }
  bool istmp(int i) { return tmp[i] != 0; }
  void set_istmp(int i) { tmp[i] = 1; }
  int slot_pop(PQStep& c) { return slots[--c.slot_top]; }
  void slot_push(PQStep& c, int s) { slots[c.slot_top++] = s; }
};
}  // namespace

static int ctx_pq(Ctx* c, int op, Batch* B, int32_t id, int key_lo, int key_hi) {
  if (key_lo != 0 || key_hi != kMaxKeys) {
    set_err("priorityqueue aggregations need the full key range (the queue order depends on every key)");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  hipStream_t s = c->stream;
  const size_t N = B->n_bm;
  const size_t ub = std::min<size_t>(kMaxKeys, std::max<size_t>(B->n_ctr, 1));
  OutCtx oc;
  CHK(prepare_output(c, ub, kStagedMax * ub + B->max_ser, &oc, false));
  c->r().pending_src = {id};
  c->mark(0);
  // one task per union key (an empty aggregate has none: new RoaringBitmap())
  launch_plan_wide(s, N ? 0 : 1, B->key_off.as<uint32_t>(), N ? (uint32_t)N : 0xFFFFFFFFu, 0, kMaxKeys,
                   c->by_key.as<Task>(), c->flag.as<uint8_t>(), c->wg_count.as<uint32_t>(), c->zlb, c->ztile);
  launch_compact(s, c->flag.as<uint8_t>(), c->by_key.as<Task>(), c->wg_count.as<uint32_t>(), c->r().tasks.as<Task>(),
                 c->r().ntasks.as<uint32_t>());
  c->mark(1);
  if (!N) {
    c->mark(2);
    launch_place(s, c->r().ntasks.as<uint32_t>(), oc, c->r().info.as<ResultInfo>());
    c->r().last = 1;
    c->mark(3);
    HIPCHK(hipGetLastError());
    return RBG_OK;
  }
  uint32_t h_nt = 0;
  HIPCHK(hipMemcpyAsync(&h_nt, c->r().ntasks.p, 4, hipMemcpyDeviceToHost, s));
  std::vector<unsigned long long> leaf(N);
  DevBuf dsz;
  CHK(dsz.ensure(8 * N));
  HIPCHK(hipMemsetAsync(dsz.p, 0, 8 * N, s));
  launch_pq_leaf_sizes(s, B->desc.as<CDesc>(), B->bm.as<uint32_t>(), B->payload.as<uint8_t>(), B->n_ctr,
                       dsz.as<unsigned long long>());
  HIPCHK(hipMemcpyAsync(leaf.data(), dsz.p, 8 * N, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));

  // Temps: at most N/2 + 1 are live at once (every priorityqueue_or temp starts from two
  // inputs; a priorityqueue_xor step allocates one while its operands are still queued).
  // Each has one 16 B state per union key; containers that are not input clones live in
  // 8 KiB arena blocks from the key's own pool: floor(n_t / 2) blocks for a key held by
  // n_t inputs (pq.hip), at most half the batch's containers in all.
  const size_t n_slots = N / 2 + 2;
  const size_t stride = std::max<uint32_t>(h_nt, 1);
  const size_t st_bytes = n_slots * stride * sizeof(PQState);
  std::vector<Task> h_tasks(h_nt);
  if (h_nt) HIPCHK(hipMemcpyAsync(h_tasks.data(), c->r().tasks.p, sizeof(Task) * h_nt, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<uint32_t> kbase(stride, 0);
  std::vector<int32_t> ktop(stride, 0);
  size_t free_b = 0, total_b = 0;
  pool_clear(c);  // pooled buffers would count as used
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = free_b / 10 * 9;
  // pools of floor(n_t / 2) blocks never run out; when they do not all fit, every pool is
  // capped at the largest size that fits (a key that needs more ends the op with
  // RBG_ERR_OUT_OF_MEMORY, as a full arena did)
  auto pool_blocks = [&](int32_t cap) {
    size_t n = 0;
    for (uint32_t t = 0; t < h_nt; t++) n += (size_t)std::min(h_tasks[t].b / 2, cap);
    return n;
  };
  int32_t cap = 0;
  for (uint32_t t = 0; t < h_nt; t++) cap = std::max(cap, h_tasks[t].b / 2);
  if (st_bytes + pool_blocks(cap) * 8192 > budget) {
    int32_t lo = 0, hi = cap;  // the largest cap that fits
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo + 1) / 2;
      if (st_bytes + pool_blocks(mid) * 8192 <= budget) lo = mid;
      else hi = mid - 1;
    }
    if (lo < 1 && cap >= 1) {
      set_err("priorityqueue: " + std::to_string(n_slots) + " temps x " + std::to_string(stride) +
              " union keys need more than the free device memory; use FastAggregation.or / xor");
      return RBG_ERR_OUT_OF_MEMORY;
    }
    cap = lo;
  }
  size_t n_blk = 0;
  for (uint32_t t = 0; t < h_nt; t++) {
    kbase[t] = (uint32_t)n_blk;
    ktop[t] = std::min(h_tasks[t].b / 2, cap);
    n_blk += (size_t)ktop[t];
  }
  n_blk = std::max<size_t>(n_blk, 1);
  // host: add every input, plan the first step
  std::vector<PQEnt> heap(N);
  std::vector<int32_t> nodes(2 * N);
  std::vector<uint8_t> tmp(2 * N, 0);
  std::vector<int32_t> slots(n_slots);
  for (size_t k = 0; k < N; k++) nodes[k] = (int32_t)k;
  for (size_t k = 0; k < n_slots; k++) slots[k] = (int32_t)(n_slots - 1 - k);
  PQCtl ctl{};
  ctl.step.or_mode = op == RBG_WIDE_PQ_OR;
  ctl.step.n_nodes = (int32_t)N;
  ctl.step.slot_top = (int32_t)n_slots;
  ctl.step.rel1 = ctl.step.rel2 = -1;
  PQHost hm{heap, nodes, tmp, slots};
  for (size_t k = 0; k < N; k++) hm.add(ctl.step, PQEnt{8 + (int64_t)leaf[k], (int32_t)k, 0});
  pq_plan(hm, ctl.step);
  // Block ids level-major: pool position j of key t is block lvl[j] + rank[t], with the keys
  // ranked by pool size (largest first, stable), so level j holds the keys with more than j
  // blocks contiguously.  Keys pop their positions 0, 1, ... in order, so the workgroups of
  // neighbouring keys write neighbouring blocks (uniform data: one contiguous level per
  // step instead of blocks a pool apart).
  std::vector<uint32_t> order(h_nt);
  for (uint32_t t = 0; t < h_nt; t++) order[t] = t;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ktop[x] > ktop[y]; });
  std::vector<uint32_t> rank(h_nt);
  for (uint32_t i = 0; i < h_nt; i++) rank[order[i]] = i;
  const int32_t max_cap = h_nt ? ktop[order[0]] : 0;
  std::vector<size_t> lvl(max_cap + 1, 0);
  for (int32_t j = 0, i = (int32_t)h_nt; j < max_cap; j++) {  // keys with more than j blocks: the first i
    while (i > 0 && ktop[order[i - 1]] <= j) i--;
    lvl[j + 1] = lvl[j] + (size_t)i;
  }
  std::vector<int32_t> stack(n_blk);
  for (uint32_t t = 0; t < h_nt; t++)
    for (int32_t i = 0; i < ktop[t]; i++) stack[kbase[t] + i] = (int32_t)(lvl[ktop[t] - 1 - i] + rank[t]);
  // device copies
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_heap = al(sizeof(PQCtl)), o_node = o_heap + al(16 * N), o_tmp = o_node + al(8 * N),
               o_slots = o_tmp + al(2 * N), o_stack = o_slots + al(4 * n_slots), o_base = o_stack + al(4 * n_blk),
               o_top = o_base + al(4 * stride), o_end = o_top + al(4 * stride);
  DevBuf meta, states, arena;
  CHK(meta.ensure(o_end));
  CHK(states.ensure(st_bytes));
  CHK(arena.ensure(n_blk * 8192));
  uint8_t* mb = meta.as<uint8_t>();
  HIPCHK(hipMemcpyAsync(mb, &ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(mb + o_heap, heap.data(), 16 * N, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(mb + o_node, nodes.data(), 8 * N, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(mb + o_tmp, tmp.data(), 2 * N, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(mb + o_slots, slots.data(), 4 * n_slots, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(mb + o_stack, stack.data(), 4 * n_blk, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(mb + o_base, kbase.data(), 4 * stride, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(mb + o_top, ktop.data(), 4 * stride, hipMemcpyHostToDevice, s));
  const PQDev D{reinterpret_cast<PQCtl*>(mb), reinterpret_cast<PQEnt*>(mb + o_heap),
                reinterpret_cast<int32_t*>(mb + o_node), mb + o_tmp, reinterpret_cast<int32_t*>(mb + o_slots),
                states.as<PQState>(), stride, arena.as<uint64_t>(), reinterpret_cast<int32_t*>(mb + o_stack),
                reinterpret_cast<const uint32_t*>(mb + o_base), reinterpret_cast<int32_t*>(mb + o_top)};
  const PQArgs pa{B->desc.as<CDesc>(), B->bm.as<uint32_t>(), B->payload.as<uint8_t>()};
  const int grid = grid_for(h_nt, 65536);
  for (size_t k = 0; k + 1 < N; k++) {
    launch_pq_step(s, grid, c->r().tasks.as<Task>(), c->r().ntasks.as<uint32_t>(), pa, D);
    if ((k & 1023) == 1023) HIPCHK(hipGetLastError());
  }
  c->mark(2);
  launch_pq_final(s, grid, c->r().tasks.as<Task>(), c->r().ntasks.as<uint32_t>(), pa, op == RBG_WIDE_PQ_OR ? 1 : 0, D, oc);
  HIPCHK(hipGetLastError());
  launch_place(s, c->r().ntasks.as<uint32_t>(), oc, c->r().info.as<ResultInfo>());
  PQCtl done{};
  HIPCHK(hipMemcpyAsync(&done, mb, sizeof(done), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));  // the temps are freed on return
  if (done.err || !done.step.final_step) {
    set_err(done.err ? "priorityqueue: a key's block pool ran out (" + std::to_string(n_blk) + " x 8 KiB in all)"
                     : std::string("priorityqueue: the device queue did not finish"));
    return done.err ? RBG_ERR_OUT_OF_MEMORY : RBG_ERR_DEVICE;
  }
  c->r().last = 1;
  c->mark(3);
  HIPCHK(hipGetLastError());
  return RBG_OK;
}

// FastAggregation dispatch (RB/FastAggregation.java:26-101,653-666,823-836)
// start_override >= 0: naive_and starts from that input (key-range shards pass the
// input with the fewest containers over the WHOLE universe, RB/FastAggregation.java:333-339)
// Wide ops whose kernels read array payloads at any 2 B alignment (a packed batch): every op that runs
// the per-key OR / XOR kernels or workShyAnd (k_wide, k_shy_wave, and the queue / horizontal / parallel
// forms, which reduce to them on a batch without run containers).  naive_and's chains (N <= 10, the
// Iterator forms, the buffer package's and chains) materialise through the slot-aligned helpers.
bool wide_reads_packed(int op, size_t n) {
  switch (op) {
    case RBG_WIDE_OR:
    case RBG_WIDE_XOR:
    case RBG_WIDE_WORKSHY_AND:
    case RBG_WIDE_PARALLEL_OR:
    case RBG_WIDE_PARALLEL_XOR:
    case RBG_WIDE_BUFFER_OR_MUTABLE:
    case RBG_WIDE_HORIZONTAL_OR:
    case RBG_WIDE_HORIZONTAL_XOR:
    case RBG_WIDE_PQ_OR:
    case RBG_WIDE_PQ_XOR: return true;
    case RBG_WIDE_AND: return n > 10;  // FastAggregation.and: workShyAnd above 10 inputs (RB/FastAggregation.java:38)
    default: return false;
  }
}

int ctx_wide(Ctx* c, int op, int32_t id, int key_lo, int key_hi, const int32_t* ids, bool card_only,
             int* host_card_out, bool* host_card_valid, int32_t start_override) {
  Batch* B;
  CHK(get_batch(c, id, &B));
  if (!B->key_major) {
    set_err("wide ops need a key-major batch");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  if (B->packed && !card_only && !wide_reads_packed(op, B->n_bm)) {
    set_err("this wide op needs slot-aligned payloads (load the batch without packing)");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  key_lo = std::max(0, key_lo);
  key_hi = std::min(kMaxKeys, key_hi);
  if (host_card_valid) *host_card_valid = false;
  if (!card_only && (op == RBG_WIDE_PQ_OR || op == RBG_WIDE_PQ_XOR)) {
    // Without run containers the queue's order cannot show in the bytes: every container of
    // its algebra ends BY_CARD of its set (pq.hip: lazy bitmaps are repaired to BY_CARD or
    // RunContainer.full; an exact bitmap only comes from an input bitmap, over 4096 values;
    // an array from ArrayContainer.lazyor holds at most 1024; the pairwise XOR types are
    // BY_CARD), and a key held by one input is that input's container, as in naive_or /
    // naive_xor, which then give the same bytes.
    if (B->n_kind[DK_R] != 0 || key_lo != 0 || key_hi != kMaxKeys) return ctx_pq(c, op, B, id, key_lo, key_hi);
    op = op == RBG_WIDE_PQ_OR ? RBG_WIDE_OR : RBG_WIDE_XOR;
  }
  // BufferFastAggregation's and chains: the heap forms' dispatch, with the buffer package's run AND run
  bool buffer = false;
  if (!card_only && op >= RBG_WIDE_BUFFER_AND && op <= RBG_WIDE_BUFFER_AND_ITER) {
    buffer = true;
    op = op == RBG_WIDE_BUFFER_AND ? RBG_WIDE_AND : op == RBG_WIDE_BUFFER_NAIVE_AND ? RBG_WIDE_NAIVE_AND : RBG_WIDE_AND_ITER;
  }
  hipStream_t s = c->stream;
  const size_t N = B->n_bm;
  int mode = WIDE_OR, plan_mode = 0;
  uint32_t start_bm = 0, chain = 0;
  const uint32_t* order = nullptr;
  std::vector<uint8_t> skip;
  if (card_only) {
    // andCardinality: 0 -> 0, 1 -> card, >= 2 -> per-key AND sum (== andCardinality / workShyAndCardinality)
    // orCardinality : 0 -> 0, 1 -> card, >= 2 -> per-key OR sum (== orCardinality / horizontalOrCardinality)
    if (op != RBG_WIDE_CARD_AND && op != RBG_WIDE_CARD_OR) return RBG_ERR_ILLEGAL_ARGUMENT;
    const bool full_range = key_lo == 0 && key_hi == kMaxKeys;
    if (N == 0 || (N == 1 && full_range)) {
      const int64_t cc = N ? B->h_bm_card[0] : 0;
      *host_card_out = (int32_t)(uint32_t)(uint64_t)cc;
      *host_card_valid = true;
      CHK(main_set(c));  // no op bracket: set 0's `last` changes
      c->r().last = 2;
      return RBG_OK;
    }
    if (op == RBG_WIDE_CARD_AND && N >= 2) {
      mode = WIDE_AND_SHY_CARD;
      plan_mode = 1;
    } else {
      mode = WIDE_OR_CARD;  // also a single input restricted to a key range
    }
  } else {
    switch (op) {
      case RBG_WIDE_OR: mode = WIDE_OR; break;
      case RBG_WIDE_XOR: mode = WIDE_XOR; break;
      case RBG_WIDE_AND:
      case RBG_WIDE_AND_ITER:
      case RBG_WIDE_NAIVE_AND:
      case RBG_WIDE_WORKSHY_AND:
        plan_mode = 1;
        if (op == RBG_WIDE_WORKSHY_AND && N == 0) {
          set_err("workShyAnd needs at least one bitmap");  // bitmaps[0] on an empty array
          return RBG_ERR_ILLEGAL_ARGUMENT;
        }
        if ((op == RBG_WIDE_AND && N > 10) || op == RBG_WIDE_WORKSHY_AND) {
          mode = WIDE_AND_SHY;
        } else {
          mode = WIDE_AND_NAIVE;
          skip.assign(std::max<size_t>(N, 1), 0);
          if (op != RBG_WIDE_AND_ITER) {
            // the input with the fewest containers, first on ties (:333-339)
            if (start_override >= 0 && (size_t)start_override < N) {
              start_bm = (uint32_t)start_override;
            } else {
              for (size_t i = 1; i < N; i++)
                if (B->h_bm_nctr[i] < B->h_bm_nctr[start_bm]) start_bm = (uint32_t)i;
            }
            for (size_t i = 0; i < N; i++)
              skip[i] = (i == start_bm) || (ids && ids[i] == ids[start_bm]);  // :341 identity skip
          } else {
            start_bm = 0;  // naive_and(Iterator): clone of the first input, :309-313
            skip[0] = 1;
          }
        }
        break;
      case RBG_WIDE_PARALLEL_OR: mode = WIDE_LAZY_CHAIN; chain = kChainLimit16; break;
      case RBG_WIDE_PARALLEL_XOR: mode = WIDE_XOR_CHAIN; break;
      case RBG_WIDE_BUFFER_OR_MUTABLE: mode = WIDE_LAZY_CHAIN; break;
      case RBG_WIDE_HORIZONTAL_OR:
      case RBG_WIDE_HORIZONTAL_XOR:
        mode = op == RBG_WIDE_HORIZONTAL_OR ? WIDE_LAZY_CHAIN : WIDE_XOR_CHAIN;
        chain = op == RBG_WIDE_HORIZONTAL_OR ? kChainN1Clone : kChainKeepEmpty;
        bool identity;
        CHK(horizontal_order(c, B, &identity));
        order = identity ? nullptr : c->order.as<uint32_t>();
        break;
      default: return RBG_ERR_ILLEGAL_ARGUMENT;
    }
  }
  if (N == 0) {
    // empty aggregate: empty bitmap (:329-331 for and; naive_or/xor of nothing)
    plan_mode = 2;
  }
  // the buffer naive_and chain may keep run containers of more than 2047 runs: they go to the
  // big-run arena (with_big_runs)
  const bool big_runs = buffer && mode == WIDE_AND_NAIVE && N > 0;
  return with_big_runs(c, big_runs, "naive_and", [&](const BigRuns& big) -> int {
    const size_t ub = std::min<size_t>(kMaxKeys, std::max<size_t>(B->n_ctr, 1));
    OutCtx oc;
    CHK(prepare_output(c, ub, kStagedMax * ub + B->max_ser + big.cap, &oc, card_only));
    // OR results are bitmaps whenever more than 4096 values survive: write those in place
    // (8192 t < kStagedMax ub, inside the payload region)
    if (!card_only && (mode == WIDE_OR || mode == WIDE_LAZY_CHAIN)) oc.spec = c->r().pending.spec = 1;
    c->r().pending_src = {id};
    if (!skip.empty()) {
      CHK(c->skip.ensure(skip.size()));
      HIPCHK(hipMemcpyAsync(c->skip.p, skip.data(), skip.size(), hipMemcpyHostToDevice, s));
    }
    const uint32_t n_req = plan_mode == 2 ? 0xFFFFFFFFu : (uint32_t)N;
    c->mark(0);
    launch_plan_wide(s, plan_mode == 0 ? 0 : 1, B->key_off.as<uint32_t>(), n_req, key_lo, key_hi,
                     c->by_key.as<Task>(), c->flag.as<uint8_t>(), c->wg_count.as<uint32_t>(), c->zlb, c->ztile);
    launch_compact(s, c->flag.as<uint8_t>(), c->by_key.as<Task>(), c->wg_count.as<uint32_t>(), c->r().tasks.as<Task>(),
                   c->r().ntasks.as<uint32_t>());
    WideArgs wa{};
    wa.desc = B->desc.as<CDesc>();
    wa.bm = B->bm.as<uint32_t>();
    wa.payload = B->payload.as<uint8_t>();
    wa.skip = skip.empty() ? nullptr : c->skip.as<uint8_t>();
    wa.start_bm = start_bm;
    // (the all-array path streams a key's slots as one run of values: they must be back to back)
    wa.all_array = (B->n_kind[DK_B] == 0 && B->n_kind[DK_R] == 0 && !B->gapped) ? 1u : 0u;
    wa.slot32 = B->payload_bytes < (1ull << 36) ? 1u : 0u;
    wa.order = order;
    wa.chain = chain;
    wa.rd_bytes = c->prof_cap > 0 && c->rd_ctr.p ? c->rd_ctr.as<unsigned long long>() : nullptr;
    wa.buffer = buffer ? 1u : 0u;
    wa.big = big;
    c->mark(1);
    launch_wide(s, mode, grid_for(ub, 65536), c->r().tasks.as<Task>(), c->r().ntasks.as<uint32_t>(), wa, oc,
                c->r().task_card.as<uint32_t>());
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
  });
}

}  // namespace rbg
