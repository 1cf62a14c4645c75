// Kernel launch interface of the engine (host side <-> kernels.hip / wide.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device.hpp"

namespace rbg {

// workgroups of a grid-stride launch over `items` at `per_block` each: at least one, at most `cap`
static inline unsigned grid_for(uint64_t items, uint64_t per_block, uint64_t cap) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, cap));
}

enum OpCode : int { OP_AND = 0, OP_OR = 1, OP_XOR = 2, OP_ANDNOT = 3 };

// wide-op flavours (wide.hip)
enum WideMode : int {
  WIDE_OR = 0,         // FastAggregation.naive_or
  WIDE_OR_CARD = 1,    // horizontalOrCardinality
  WIDE_XOR = 2,        // naive_xor
  WIDE_AND_SHY = 3,    // workShyAnd
  WIDE_AND_SHY_CARD = 4,  // workShyAndCardinality
  WIDE_AND_NAIVE = 5,  // naive_and chain (WideArgs::buffer: BufferFastAggregation's)
  WIDE_LAZY_CHAIN = 6,  // lazyIOR chain + repairAfterLazy: ParallelAggregation.or, BufferFastAggregation.or(Mutable...),
                        // horizontal_or
  WIDE_XOR_CHAIN = 7,   // clone + ixor chain without restart: ParallelAggregation.xor, horizontal_xor
};

// WideArgs::chain flags
constexpr uint32_t kChainLimit16 = 1;  // ParallelAggregation.or: 16+ containers per key take the lazy-bitmap branch
constexpr uint32_t kChainN1Clone = 2;  // a key of one container is a plain clone (no repairAfterLazy)
constexpr uint32_t kChainKeepEmpty = 4;  // horizontal_xor appends empty results

struct WideArgs {
  const CDesc* desc;      // key-major container table
  const uint32_t* bm;     // input bitmap index per container
  const uint8_t* payload; // arena
  const uint8_t* skip;    // naive_and: per input bitmap, 1 = skip (identity with the start)
  uint32_t start_bm;      // naive_and: input bitmap the chain starts from
  uint32_t all_array;     // every container is an array: a key segment is one contiguous u16 value stream
  uint32_t slot32;        // every slot offset / 16 fits 32 bits (payload < 64 GiB)
  const uint32_t* order;  // chain modes: container index at chain position j of a key segment (null: input order)
  uint32_t chain;         // chain modes: kChain* flags
  unsigned long long* rd_bytes;  // workShyAnd: payload + 4 B per container it read, summed (null: not counted)
  uint32_t buffer;        // naive_and: the buffer package's chain (MappeableRunContainer.iand(R) keeps the merged runs)
  BigRuns big;            // naive_and (buffer): results of more than 2047 runs
};

// priority-queue aggregations (pq.hip): the size-ordered queue runs on the device.  Each
// step launch combines two nodes (an input bitmap of the batch, or an intermediate temp)
// over every union key; the launch's last workgroup folds the result size into the
// queue and writes the next step, so the host only enqueues N - 1 launches.
//   PQ_XOR  RoaringBitmap.xor(x1, x2)                 (priorityqueue_xor)
//   PQ_LOR  RoaringBitmap.lazyor(x1, x2), static      (priorityqueue_or, two inputs)
//   PQ_LIOR x1.lazyor(x2), in place on the temp x1    (one temp)
//   PQ_LFL  RoaringBitmap.lazyorfromlazyinputs(x1, x2) (two temps)
enum PQOp : int { PQ_XOR = 0, PQ_LOR = 1, PQ_LIOR = 2, PQ_LFL = 3 };
// container kinds of a node: DK_A / DK_B (exact) / DK_R, and a lazy bitmap (card -1 in the reference)
enum PQKind : int { PK_A = 0, PK_BE = 1, PK_R = 2, PK_BL = 3 };
struct __align__(16) PQState {  // per key of a temp
  uint32_t card;
  uint16_t nruns;
  uint8_t kind;     // PQKind
  uint8_t present;  // the temp holds this key
  int32_t src;      // >= 0: an unchanged clone of this input container (desc index)
  int32_t blk;      // else: the 8 KiB block of the set arena holding the container
};
// A queue entry: the node's getLongSizeInBytes is fixed while it is queued.
struct PQEnt {
  int64_t size;
  int32_t node;
  int32_t pad;
};
// The step the next launch runs, and the queue's scalar state.  Node references:
// >= 0 input bitmap of the batch, < 0 temp slot -1 - ref.
struct PQStep {
  int32_t op, final_step, a, b, o;
  int32_t target;      // node index whose size the step's result gives
  int32_t rel1, rel2;  // temp slots freed after the step (-1: none)
  int32_t heap_n, n_nodes, slot_top, or_mode;
};
// A step's workgroups report in kPQGroups groups (blockIdx % kPQGroups), each counter and
// size word in a cache line of its own: one contended address serialises its atomics
// (~12 ns each), so a launch of G workgroups pays G / kPQGroups of them on the longest chain.
constexpr int kPQGroups = 8;
struct __align__(128) PQLine {
  uint32_t done;  // workgroups of the group finished in the running step
  uint32_t pad;
  unsigned long long size;  // the group's share of the step's result size
  uint8_t pad2[112];
};
struct PQCtl {
  PQStep step;
  uint32_t done;  // groups finished in the running step
  uint32_t err;   // a key's block pool ran out (cannot happen: see ctx_pq)
  uint8_t pad[72];
  PQLine grp[kPQGroups];
};
struct PQDev {
  PQCtl* ctl;
  PQEnt* heap;        // java.util.PriorityQueue array order
  int32_t* node;      // node index -> reference
  uint8_t* istmp;     // priorityqueue_or: node holds a temp
  int32_t* slots;     // free temp slots (stack)
  PQState* states;    // temp slot s: states[s * stride + task]
  uint64_t stride;
  uint64_t* arena;    // 8 KiB blocks (1024 words)
  // Per key, a private pool of arena blocks: the free blocks of key t are
  // kstack[kbase[t] .. kbase[t] + ktop[t]).  Only the workgroup of key t touches them.
  int32_t* kstack;
  const uint32_t* kbase;
  int32_t* ktop;
};
struct PQArgs {
  const CDesc* desc;
  const uint32_t* bm;
  const uint8_t* payload;
};

// The queue (RB/FastAggregation.java:758-781 / :799-811) after the host has added every
// input: pq_finish folds a step's result size in, pq_plan polls the next pair.  M gives
// the heap operations and node table: sequential on the host (the first step), a wave of
// the scheduling workgroup on the device.
template <class M>
__host__ __device__ inline void pq_finish(M& m, PQStep& c, int64_t size) {
  m.add(c, PQEnt{size, c.target, 0});
  if (c.rel1 >= 0) m.slot_push(c, c.rel1);
  if (c.rel2 >= 0) m.slot_push(c, c.rel2);
}
template <class M>
__host__ __device__ inline void pq_plan(M& m, PQStep& c) {
  if (c.heap_n <= 1) {
    c.final_step = 1;
    c.a = c.heap_n ? m.node(m.poll(c).node) : 0;
    return;
  }
  const int x1 = m.poll(c).node;
  const int x2 = m.poll(c).node;
  c.rel1 = c.rel2 = -1;
  if (c.or_mode) {
    const bool t1 = m.istmp(x1), t2 = m.istmp(x2);
    if (t1 && t2) {  // lazyorfromlazyinputs(buffer[x1], buffer[x2]) into x1's temp
      c.op = PQ_LFL;
      c.a = m.node(x1);
      c.b = m.node(x2);
      c.o = c.a;
      c.target = x1;
      c.rel1 = -1 - c.b;
    } else if (t2) {  // buffer[x2].lazyor(buffer[x1])
      c.op = PQ_LIOR;
      c.a = m.node(x2);
      c.b = m.node(x1);
      c.o = c.a;
      c.target = x2;
    } else if (t1) {  // buffer[x1].lazyor(buffer[x2])
      c.op = PQ_LIOR;
      c.a = m.node(x1);
      c.b = m.node(x2);
      c.o = c.a;
      c.target = x1;
    } else {  // RoaringBitmap.lazyor(buffer[x1], buffer[x2]) into a new temp
      c.op = PQ_LOR;
      c.a = m.node(x1);
      c.b = m.node(x2);
      c.o = -1 - m.slot_pop(c);
      m.set_node(x1, c.o);
      m.set_istmp(x1);
      c.target = x1;
    }
  } else {  // pq.add(RoaringBitmap.xor(x1, x2))
    c.op = PQ_XOR;
    c.a = m.node(x1);
    c.b = m.node(x2);
    c.o = -1 - m.slot_pop(c);
    c.target = c.n_nodes++;
    m.set_node(c.target, c.o);
    if (c.a < 0) c.rel1 = -1 - c.a;
    if (c.b < 0) c.rel2 = -1 - c.b;
  }
}
// java.util.PriorityQueue's comparator over getLongSizeInBytes: (int)(sizes[a] - sizes[b])
__host__ __device__ inline int pq_cmp(int64_t a, int64_t b) { return (int)(int32_t)(uint32_t)(uint64_t)(a - b); }

// sizes[bm] += 2 + getSizeInBytes over the batch's containers (sizes zeroed by the caller)
void launch_pq_leaf_sizes(hipStream_t s, const CDesc* desc, const uint32_t* bm, const uint8_t* payload, uint64_t n,
                          unsigned long long* sizes);
// one step of the queue (the step record in D.ctl), then the next step's plan
void launch_pq_step(hipStream_t s, int grid, const Task* tasks, const uint32_t* nt, PQArgs args, PQDev D);
// the root node as the op's result records (repair: priorityqueue_or's repairAfterLazy)
void launch_pq_final(hipStream_t s, int grid, const Task* tasks, const uint32_t* nt, PQArgs args, int repair,
                     PQDev D, OutCtx oc);

// bit-sliced index (bsi.hip); ops in the order of BitmapSliceIndex.Operation
// (bsi/src/main/java/org/roaringbitmap/bsi/BitmapSliceIndex.java:23-38)
// BSI_ALL: compareUsingMinMax's "all" (BSI/:516: ebM, or and(ebM, foundSet));
// BSI_SUM_ONLY: sum(foundSet) alone
enum BsiOp : int { BSI_EQ = 0, BSI_NEQ = 1, BSI_LE = 2, BSI_LT = 3, BSI_GE = 4, BSI_GT = 5, BSI_RANGE = 6,
                   BSI_ALL = 7, BSI_SUM_ONLY = 8 };
constexpr int kBsiMaxInputs = 34;  // ebM + up to 32 slices + foundSet
// BSI sum words (u64): per-slice |bA[x] & found| at [x], the found count at [kBsiMaxInputs],
// then sum(found) = (sum, count) as Java longs at [kBsiSumOut], [kBsiSumOut + 1]
constexpr int kBsiSumOut = kBsiMaxInputs + 1;
constexpr int kBsiSumWords = kBsiSumOut + 2;
// k_bsi_types adds its per-block sums into one of kBsiSumReps replicas of 64 words after
// those (block b: replica b % kBsiSumReps), so no sum word takes more than a few dozen
// atomics; k_bsi_sum_final adds the replicas.  All of it is zeroed by the plan kernel.
constexpr int kBsiSumReps = 16;
constexpr int kBsiSumAll = kBsiSumWords + 64 * kBsiSumReps;
constexpr int kOwenOrder = 64;  // bytes per task of an owenGreatEqual chain order
struct BsiArgs {
  int op;         // BsiOp
  int nbits;      // slices
  int has_found;  // input nbits+1 is the foundSet
  uint32_t pred0;  // predicate (RANGE: start)
  uint32_t pred1;  // RANGE: end
  // buffer package (bsi/.../bsi/buffer/BitSliceIndexBase.java): its own compare circuit and
  // ImmutableRoaringBitmap's pairwise types (bsi.hip, "Buffer-package BSI")
  int buffer;
  int found_input;      // input index of the found set (nbits + 1 of the batch; the buffer kernel may run
                        // with nbits = 0 over the same batch)
  uint32_t owen_zeros;  // GE / RANGE: slice positions of owenGreatEqual's orInputs (0 bits of start - 1)
  uint32_t owen_ones;   //   and of its spine ANDs (1 bits), both within [leastSignifZero, nbits)
  const uint8_t* owen_order;  // per task kOwenOrder bytes: [0] = n, [1 + k] = orInput of chain position k
                              // (the horizontal_or queue's poll order); null: top-down order
  void* owen_tb;              // per task 32 x 16 B: each orInput's (kind, card, src) (k_bsi_owen_pre)
  uint32_t* task_keys;        // k_bsi_owen_pre: key of each task
  BigRuns big;
};

// Workgroups of `kernel` (256 threads) that are resident on the whole device at
// once: CUs x occupancy.  Task kernels launch at most this many workgroups and
// stride over their tasks, so no workgroup waits for a dispatch slot and no
// wave pays a launch per task (cached per kernel).
int resident_grid(const void* kernel, int block = 256);  // workgroups of `block` threads resident at once
// A task kernel K (256 threads, `per_block` tasks per workgroup at a time) over a list of at most `tasks`
// tasks: one workgroup per `per_block` of them, at least one, at most the resident grid
template <auto K, class... A>
static inline void launch_resident(hipStream_t s, int tasks, int per_block, A... args) {
  const int g = std::max(1, std::min((tasks + per_block - 1) / per_block, resident_grid((const void*)K)));
  hipLaunchKernelGGL(K, dim3(g), dim3(256), 0, s, args...);
}
// a run-time op / mode / flag as a type, to pick a kernel's template instance: f(Int<OP_AND>{}) ...
template <int V>
using Int = std::integral_constant<int, V>;

// plan kernels also zero the op's look-back header (zlb, 32 u64) and tile statuses (ztile, 128 u64)
void launch_plan_wide(hipStream_t s, int mode, const uint32_t* key_off, uint32_t n_req, int key_lo, int key_hi,
                      Task* by_key, uint8_t* flag, uint32_t* wg_count, uint64_t* zlb, uint64_t* ztile);
void launch_compact(hipStream_t s, const uint8_t* flag, const Task* by_key, const uint32_t* wg_count, Task* tasks,
                    uint32_t* n_tasks);
// pairwise.hip: plan (key alignment + descriptor resolution) and the wave-per-key compute
// plan + compaction in one launch: tasks[] in key order, *n_tasks (PlanOut, device.hpp; wg_epoch zeroed
// once per context); only keys in [key_lo, key_hi).
void launch_plan_pairwise(hipStream_t s, int op, int key_lo, int key_hi, BmView A, BmView B, PlanOut po, uint32_t* err);
// mode 0: materialise results (task slots + records); mode 1: andCardinality into task_card
// A dense key range of the pairwise compute kernel: the record of key k is at position k - key_lo.
struct PwDirect {
  int key_lo;
};
// dense: null = tasks / nt from launch_plan_pairwise (sparse ranges), run by k_pair_wave; else tasks /
// nt[0..1] from launch_plan_balanced (dense ranges), records at key positions (dense->key_lo), run by
// k_pair_cu (one 16-wave workgroup per CU, tasks claimed from the CU's share)
void launch_pairwise(hipStream_t s, int op, int mode, int grid, const PTask* tasks, const uint32_t* nt,
                     const uint8_t* pa, const uint8_t* pb, OutCtx oc, uint32_t* task_card, const PwDirect* dense);
// dense key ranges: every key's task resolved and ordered by estimated cost within its 256-key segment
// (heaviest first, rotated by the segment index) into tasks[]; n_tasks[0] = n_tasks[1] = nkeys (records
// and list positions, one per key: keys without a task are marked, with an empty record / a zero count)
// (no compaction: po.wg_epoch / po.epoch are not used)
void launch_plan_balanced(hipStream_t s, int op, int mode, int key_lo, uint32_t nkeys, BmView A, BmView B, PlanOut po,
                          OutCtx oc, uint32_t* task_card);
void launch_wide(hipStream_t s, int mode, int grid, const Task* tasks, const uint32_t* nt, WideArgs args, OutCtx oc,
                 uint32_t* task_card);
// result materialisation: k_place = compaction scan over the task records
// (container index + payload offset per kept container, ResultInfo); the
// portable serialization (payload copies, descriptors, offsets, run flags,
// cookie) runs only when the result is fetched
void launch_place(hipStream_t s, const uint32_t* nt, OutCtx oc, ResultInfo* info);
// placement + serialization in one launch from the compute kernel's per-tile sums (OutCtx::tile_agg):
// one workgroup per kAggTile records, no look-back; also writes info, the totals word and the result's
// cardinality like k_place.  max_tasks: an upper bound of *nt (the grid)
void launch_serialize_agg(hipStream_t s, const uint32_t* nt, OutCtx oc, ResultInfo* info, size_t max_tasks);
void launch_spec_fix(hipStream_t s, const uint32_t* nt, OutCtx oc);
void launch_serialize(hipStream_t s, const uint32_t* nt, OutCtx oc);
// key shard of a global bitmap: payloads into payload_dst, 4 B descriptors into desc, global
// offsets (off0 + local offset) into offs (nullable), one run-flag byte per container into runb (nullable)
void launch_serialize_shard(hipStream_t s, int grid, const uint32_t* nt, OutCtx oc, uint8_t* payload_dst, uint64_t off0,
                            uint8_t* desc, uint8_t* offs, uint8_t* runb);
// the same with the global layout in device memory (lay: world x {containers, payload bytes, has_run}
// int64); out is laid out as the whole global bitmap, runb one byte per global container (nullable);
// rank 0 also writes the cookie.  emit = false: the payload is already in place.
void launch_serialize_shard_dyn(hipStream_t s, int grid, const uint32_t* nt, OutCtx oc, const int64_t* lay, int rank,
                                int world, uint8_t* out, uint8_t* runb, bool emit);
// in-place OR's types after an OR (x1.or(x2), RB/RoaringBitmap.java:2481-2523): a full result of
// bitmap x1 | array x2 stays a bitmap (ones: 8192 bytes of 0xFF)
void launch_ior_fix(hipStream_t s, const uint32_t* nt, ORec* recs, BmView A, BmView B, const uint8_t* ones);
// dst[0..2] = the pending result's (containers, payload bytes, has_run) from k_place's ResultInfo
void launch_layout_out(hipStream_t s, const ResultInfo* info, int64_t* dst);
void launch_reduce_card(hipStream_t s, const uint32_t* task_card, const uint32_t* nt, ResultInfo* info,
                        const uint32_t* err);
void launch_batch_bytes(hipStream_t s, const CDesc* desc, uint64_t n, const uint8_t* payload, unsigned long long* out);
// dst[it.dst .. +it.len) = src[it.src .. +it.len) for every item (wave per item; src needs 16 B read slack)
struct GatherItem {
  uint64_t src, dst, len;
};
void launch_gather(hipStream_t s, const GatherItem* items, uint64_t n, const uint8_t* src, uint8_t* dst);

// block 0 also zeroes zsums (kBsiSumWords u64) and zdefer[0] (either may be null)
void launch_plan_bsi(hipStream_t s, const uint32_t* key_off, const uint32_t* bm, uint32_t need, Task* by_key,
                     uint8_t* flag, uint32_t* wg_count, uint64_t* zlb, uint64_t* ztile, unsigned long long* zsums,
                     uint32_t* zdefer);
// sums: kBsiSumWords u64 (per-slice |bA[x] & found|, the found count, then the final (sum, count)
// written by k_bsi_sum_final); null = no sum
// scratch of the register-resident compare kernels (bsi.hip), per task of the op
// (stride = task capacity; the tables are transposed, row-major over the tasks):
// defer: 1 + stride u32, cnts: 128 x 4 rows of stride ints, kin: 34 rows of stride x 16 B.
// Null: the streamed kernel only.
struct BsiScratch {
  uint32_t* defer;
  int* cnts;
  void* kin;
  size_t stride;
  void* table;  // 34 x 16 B per task: each input's container of the key
  // The task list and the input table depend on the batch only: a batch keeps them across queries
  // (table_ready: k_bsi_table skipped).  The zeroing the plan kernel does per query is then done by
  // block 0 of k_bsi_reg (zlb / ztile: placement look-back, zsums: sum words, zdefer: defer count),
  // and the batch's task count is copied to nt_dst (the context's, which k_place reads).
  bool table_ready;
  uint64_t* zlb;
  uint64_t* ztile;
  unsigned long long* zsums;
  const uint32_t* nt_src;
  uint32_t* nt_dst;
  // k_bsi_reg's unit pools: one counter per group of kBsiGroup workgroups, 64 B apart (kBsiClaimWords
  // words, zero before every query: k_bsi_types zeroes them after k_bsi_reg)
  unsigned int* claims;
};
#ifndef RBG_BSI_GROUP
#define RBG_BSI_GROUP 128
#endif
constexpr int kBsiGroup = RBG_BSI_GROUP;  // workgroups per k_bsi_reg unit pool
constexpr int kBsiMaxGroups = 1024;  // groups of a resident k_bsi_reg grid (at most 4 workgroups per CU)
constexpr int kBsiClaimWords = 16 * kBsiMaxGroups;
// true: compare `op` over `nbits` slices runs the register-resident kernels (k_bsi_table, k_bsi_reg, ...)
bool bsi_reg_path(int op, int nbits);
void launch_bsi_table(hipStream_t s, const Task* tasks, const uint32_t* nt, WideArgs args, void* table, size_t stride);
void launch_bsi_sums_out(hipStream_t s, const unsigned long long* sums, void* dst);  // 2 x u64 at kBsiSumOut
// sums_dst (nullable): (sum, count) also written there by the final sum kernel (two int64, device memory)
void launch_bsi(hipStream_t s, int grid, const Task* tasks, const uint32_t* nt, WideArgs args, BsiArgs p, OutCtx oc,
                unsigned long long* sums, BsiScratch* sc, void* sums_dst = nullptr);
// buffer-package compare (p.buffer): k_bsi_owen_pre writes the orInput types of owenGreatEqual per
// task (p.owen_tb, p.task_keys) for the host's horizontal_or queue replay; k_bsi_buf runs the circuit
void launch_bsi_owen_pre(hipStream_t s, int grid, const Task* tasks, const uint32_t* nt, WideArgs args, BsiArgs p);
void launch_bsi_buf(hipStream_t s, int grid, const Task* tasks, const uint32_t* nt, WideArgs args, BsiArgs p, OutCtx oc);
// ImmutableRoaringBitmap.and / andNot (op OP_AND / OP_ANDNOT) over the pairwise plan's task list, the
// buffer package's container types (workgroup per task; run results above 2047 runs to `big`)
void launch_pair_buf(hipStream_t s, int op, int grid, const PTask* tasks, const uint32_t* nt, const uint8_t* pa,
                     const uint8_t* pb, OutCtx oc, BigRuns big);

// static add / remove / flip(rb, rangeStart, rangeEnd) (rangemut.hip); hbs > hbl: no key in the range
// RMUT_ADD_INPLACE: x.add(rangeStart, rangeEnd) (RB/RoaringBitmap.java:1181), Container.iadd on every key
// RMUT_DERUN: removeRunCompression (RB/RoaringBitmap.java:2738-2749), every run container by cardinality
// RMUT_LIMIT: limit(maxcardinality) (RB/RoaringBitmap.java:2457-2476): keys below hbs cloned, key hbs cut to its
// first lbs values (lbs = 0: none), the rest dropped
// RMUT_RANGE: bitmapOfRange(min, max) (RB/RoaringBitmap.java:588-615), add over an empty bitmap whose
// containers are all RunContainer.rangeOfOnes (run containers even for one or two values)
enum RmutOp : int { RMUT_ADD = 0, RMUT_REMOVE = 1, RMUT_FLIP = 2, RMUT_ADD_INPLACE = 3, RMUT_DERUN = 4, RMUT_LIMIT = 5,
                    RMUT_RANGE = 6 };
struct RmutArgs {
  int op, hbs, lbs, hbl, lbl;
};
// RoaringBitmap.addOffset (RB/RoaringBitmap.java:230-288), addoffset.hip: offset = 65536 co + off, off in
// [0, 65535]; none: a container offset outside [-65536, 65535] (an empty result)
struct AoffArgs {
  int co, off, none;
};
// plan + compute over operand A; grid: an upper bound of the task count
void launch_aoff(hipStream_t s, BmView A, AoffArgs aa, PlanOut po, OutCtx oc, int grid);
void launch_rmut(hipStream_t s, BmView A, RmutArgs ra, bool buf, PlanOut po, OutCtx oc, BigRuns big, int grid);

// RoaringBitmap.orNot (ornot.hip): the reference's key-loop bound, computed on the device
struct OrNotPlan {
  int32_t k_end;       // keys [0, k_end) the loop reaches
  int32_t neg;         // maxSize < 0 (the reference's NegativeArraySizeException)
  int32_t max_size;
  int32_t correction;
};
// k_ornot_scan -> k_plan_ornot -> k_ornot over single-bitmap batches A (x1) and B (x2); flags: 1 in place,
// 2 the buffer package's types (RBG_ORNOT_INPLACE / RBG_ORNOT_BUFFER)
void launch_ornot(hipStream_t s, BmView A, BmView B, int max_key, int last_run, int flags, OrNotPlan* plan, PlanOut po,
                  OutCtx oc, int grid);

// batched andCardinality over pairs (2i, 2i+1) of a bitmap-major batch: per-pair key
// alignment (count, scan, emit), then one wave per matched key; pairs of more than 64
// keys take one wave per pair.  Scratch: cnt (n_pairs u64), part (scan_parts(n_pairs)
// u64), tot (u64: items | large pairs << 32), items (batch_pair_items_cap), large (n_pairs).
struct PairItem {  // one matched key of a pair: both descriptors resolved (32 B, scalar-loaded)
  uint64_t slot_a, slot_b;
  uint32_t card_a, card_b;
  uint32_t pair;
  uint8_t kind_a, kind_b, pad0, pad1;
};
void launch_batch_and_card(hipStream_t s, uint64_t n_pairs, const uint32_t* bm_off, const uint16_t* keys,
                           const CDesc* desc, const uint8_t* payload, int32_t* out, uint64_t* cnt, uint64_t* part,
                           uint64_t* tot, PairItem* items, uint32_t* large);
uint64_t batch_pair_items_cap(const uint32_t* h_bm_nctr, uint64_t n_pairs);

// synthetic generators (synth.hip)
// C3 uniform key slice [key_lo, key_lo + nkeys): pass 0 writes per-key slot bytes,
// pass 1 (given the exclusive per-key byte offsets) fills desc/keys/bm/payload
void launch_synth_c3u(hipStream_t s, uint64_t seed, uint32_t n, int key_lo, int nkeys, unsigned long long* key_bytes,
                      const unsigned long long* key_base, CDesc* desc, uint16_t* keys, uint32_t* bm,
                      uint8_t* payload, int pass);
// C3 clustered: keys/bm of every container given (host CSR); fills desc + 8192 B bitmap slots
void launch_synth_c3c(hipStream_t s, uint64_t seed, uint64_t n_ctr, const uint16_t* keys, const uint32_t* bm,
                      CDesc* desc, uint8_t* payload);
void launch_sum_cards(hipStream_t s, const CDesc* desc, uint64_t n, unsigned long long* out);
// C5 BSI rows 0..rows-1 (nbits slices): pass 0 cards[(key, input)] + minmax, pass 1 fills at pos[(key, input)]
void launch_synth_c5(hipStream_t s, uint64_t seed, uint64_t rows, int key_lo, int nbits, int nkeys, int pass,
                     uint32_t* cards,
                     const uint32_t* pos, unsigned int* minmax, CDesc* desc, uint16_t* keys, uint32_t* bm,
                     uint8_t* payload);
// array payloads for host-built descriptors (C4 pairs)
void launch_synth_arrays(hipStream_t s, uint64_t seed, const CDesc* desc, uint64_t n, uint8_t* payload);
// force < 0: C2 mix (kind drawn per key); force = DK_A/DK_B/DK_R: every key drawn from that family
void launch_synth_c2(hipStream_t s, uint64_t seed, int force, CDesc* desc, uint16_t* keys, uint8_t* payload);

// runopt.hip: device-wide exclusive scan of u64 (part: scan_parts(n) u64 scratch;
// *total = sum), and RoaringBitmap.runOptimize over a batch
uint64_t scan_parts(uint64_t n);
void launch_exclusive_scan(hipStream_t s, const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* part,
                           uint64_t* total);
// the arrays the new batch shares with the input (keys, input index, key CSR, bitmap CSR), copied by
// the write kernel
struct RoCopy {
  const uint16_t* keys;
  uint16_t* out_keys;
  const uint32_t* bm;
  uint32_t* out_bm;
  const uint32_t* koff;
  uint32_t* out_koff;
  uint64_t n_koff;
  const uint32_t* boff;
  uint32_t* out_boff;
  uint64_t n_boff;
};
// runOptimize of every container, each written at its own slot offset of the new payload (the input's
// layout; a converted container is never larger); per workgroup g (of runopt_groups(n)) wstat[4 g + k] =
// {#A, #B, #R, serialized payload bytes} of its containers
uint64_t runopt_groups(uint64_t n);
void launch_runopt(hipStream_t s, const CDesc* desc, const uint8_t* payload, uint64_t n, CDesc* out_desc,
                   uint8_t* out_payload, RoCopy cp, unsigned long long* wstat);
// flags[bitmap] = 1 where the (new) batch holds a run container; flags zeroed by the caller
void launch_runopt_flags(hipStream_t s, const CDesc* desc, const uint32_t* bm, uint64_t n, uint32_t* flags);

// runopt.hip: selectRangeWithoutCopy of every bitmap of a batch (range-restricted aggregations): the
// range's first / last key and low bits (lbs..lbl kept on those keys)
struct RselArgs {
  int hbs, lbs, hbl, lbl;
  int buf;  // the buffer package's cut: MappeableBitmapContainer.remove makes an array below 4096 values
};
void launch_rsel_plan(hipStream_t s, const CDesc* desc, const uint32_t* bm, const uint8_t* payload, uint64_t n,
                      RselArgs ra, uint32_t* info, uint32_t* card, uint64_t* size, uint64_t* keep,
                      unsigned long long* bm_cnt, unsigned long long* bm_card, unsigned long long* totals);
void launch_rsel_write(hipStream_t s, const CDesc* desc, const uint32_t* bm, const uint8_t* payload, uint64_t n,
                       RselArgs ra, const uint32_t* info, const uint32_t* card, const uint64_t* off,
                       const uint64_t* idx, CDesc* out_desc, uint16_t* out_keys, uint32_t* out_bm,
                       uint8_t* out_payload);

// rankdir.hip: the rank directory of a single-bitmap key-major batch and the point queries over it
// (rank / select / contains / nextValue / previousValue, RB/RoaringBitmap.java:1693, 2574-2624, 2820-2883)
// == RBG_PQ_* (roaring_mi355x.h)
enum PointOp : int { PT_RANK = 0, PT_SELECT = 1, PT_CONTAINS = 2, PT_NEXT = 3, PT_PREV = 4 };
struct PointArgs {
  const uint32_t* key_off;  // the batch's key CSR (65,537 entries)
  const CDesc* desc;
  const uint8_t* payload;
  const uint64_t* cum;      // n_ctr + 1: values before each container, then the cardinality
  const uint64_t* aux_off;  // n_ctr + 1: byte offset of each container's directory in aux
  const uint8_t* aux;       // B: 128 u16 (set bits before each block of 8 words), R: u16 per run (values before it)
  uint32_t n_ctr;
};
// cum[i] = card, aux_off[i] = directory bytes of container i: both then scanned (launch_exclusive_scan)
void launch_rd_sizes(hipStream_t s, const CDesc* desc, const uint8_t* payload, uint64_t n, uint64_t* cum,
                     uint64_t* aux_off);
void launch_rd_fill(hipStream_t s, const CDesc* desc, const uint8_t* payload, uint64_t n, const uint64_t* aux_off,
                    uint8_t* aux);
// out[i] = op(q[i]) for n queries, in query order (-1: no such value)
void launch_point(hipStream_t s, int op, PointArgs a, const uint32_t* q, uint64_t n, long long* out);

// expand.hip: the values of ranks [first, first + count) of the bitmap (RoaringBitmap.toArray,
// RB/RoaringBitmap.java:3224; BatchIterator.nextBatch), ascending, into out[0 .. count): u32, or i64
// zero-extended (out64).  first + count <= cardinality; a needs the batch's rank directory.
void launch_to_values(hipStream_t s, PointArgs a, uint64_t first, uint64_t count, bool out64, void* out);

// build.hip: a one-bitmap key-major batch from n u32 values in device memory (any order, duplicates
// allowed), RoaringBitmap.add(int...) / bitmapOf (RB/RoaringBitmap.java:483-570) [+ runOptimize].
// flag: 65,536 bytes, zeroed by the caller; keys: min(n, 65536) u16; key_off: 65,537 u32; *n_ctr = C
void launch_bld_keys(hipStream_t s, const uint32_t* v, uint64_t n, uint8_t* flag, uint16_t* keys, uint32_t* key_off,
                     unsigned long long* n_ctr);
// ws: C bitmaps of 8 KiB, zeroed by the caller
void launch_bld_scatter(hipStream_t s, const uint32_t* v, uint64_t n, const uint32_t* key_off, uint32_t* ws);
constexpr size_t kBldInfoBytes = 8;  // per container: the plan's (card, nruns, kind)
// size[i] = slot bytes of container i; totals (u64, zeroed by the caller) += {#A, #B, #R, serialized
// payload bytes, cardinality}
void launch_bld_plan(hipStream_t s, const uint8_t* ws, uint64_t n_ctr, int run_optimize, void* info, uint64_t* size,
                     unsigned long long* totals);
// off: the exclusive scan of size[]; also writes bm_off = {0, C}
void launch_bld_write(hipStream_t s, const uint8_t* ws, uint64_t n_ctr, const void* info, const uint64_t* off,
                      const uint16_t* keys, CDesc* desc, uint32_t* bm, uint32_t* bm_off, uint8_t* payload);

// bitset.hip: the same batch from a dense bitset in device memory, BitSetUtil.bitmapOf(long[]) / (ByteBuffer)
// (RB/BitSetUtil.java:160-174, 185-259) [+ runOptimize].  bits: nbytes <= 2^29 bytes of little-endian 64-bit
// words, 8 B aligned, the last word possibly cut short; no byte at or past nbytes is read.  The three
// launches stand where launch_bld_keys, launch_bld_plan and launch_bld_write stand, with the same arguments
// otherwise; there is no workspace.
void launch_bits_flags(hipStream_t s, const uint8_t* bits, uint64_t nbytes, uint8_t* flag, uint16_t* keys,
                       uint32_t* key_off, unsigned long long* n_ctr);
void launch_bits_plan(hipStream_t s, const uint8_t* bits, uint64_t nbytes, const uint16_t* keys, uint64_t n_ctr,
                      int run_optimize, void* info, uint64_t* size, unsigned long long* totals);
void launch_bits_write(hipStream_t s, const uint8_t* bits, uint64_t nbytes, const uint16_t* keys, uint64_t n_ctr,
                       const void* info, const uint64_t* off, CDesc* desc, uint32_t* bm, uint32_t* bm_off,
                       uint8_t* payload);
// a mask of n elements (one byte each, nonzero = set) as ceil(n / 64) words; bits at or past n are zero
void launch_bits_pack(hipStream_t s, const uint8_t* mask, uint64_t n, uint64_t* words);
// BitSetUtil.toLongArray (:67-108) over the bit positions [first, first + n), first + n <= 2^32, of a
// one-bitmap key-major batch: ceil(n / 64) words (first % 64 == 0; out 8 B aligned; bits at or past n zero) or,
// with mask, n bytes of 0 / 1 (any first).  Writes every word / byte of the window once and nothing else.
void launch_bits_expand(hipStream_t s, const uint32_t* key_off, const CDesc* desc, const uint8_t* payload,
                        uint64_t first, uint64_t n, bool mask, void* out);

// rangebitmap.hip: one query of a resident range-encoded index (RB/RangeBitmap.java), a wave per block of
// 65,536 rows.  The wave replays the block's part of SingleEvaluation / DoubleEvaluation over its registers,
// ANDs the context's container of that key in, and either stores the block's 8 KiB of bits at out + 8192 k
// (zeros for a block the context has no key for: the whole workspace is written) or adds its cardinality to
// *count.
enum RbMode : int {
  RBM_LTE = 0,      // evaluateHorizontalSliceRange (:671-734)
  RBM_GT = 1,       // the same, flipped over the block's rows (:562-565)
  RBM_EQ = 2,       // evaluateHorizontalSlicePoint (:736-770)
  RBM_NEQ = 3,      // the same, flipped (:438-441)
  RBM_BETWEEN = 4,  // DoubleEvaluation.evaluateHorizontalSlice (:1016-1061): t0 < value <= t1
};
struct RbArgs {
  const CDesc* dir;       // n_blocks x nslices slots of the arena; kind kAbsent where the block's mask has no bit
  const uint64_t* masks;  // the blocks' container masks
  const uint8_t* arena;
  uint32_t n_blocks, nslices;
  uint64_t max_rid, mask;
  uint64_t t0, t1;
  BmView ctx;      // the context bitmap (has_ctx)
  int has_ctx;
  int ctx_minus;   // count only, RBM_LTE with a context: |context \ bits| per visited key (countRange, :659-661)
  int ctx_first;   // count only, RBM_BETWEEN with a context: every key from the context's first to its last is
                   // intersected with the context's FIRST container (count, :984-1012, never advances contextPos)
  uint8_t* out;    // 8192 n_blocks bytes, 16 B aligned; null: count
  unsigned long long* count;  // zeroed by the caller
};
void launch_rb_query(hipStream_t s, int mode, const RbArgs& a);

// rangebitmap_build.hip: a resident range-encoded index from n u64 values in device memory, row r = values[r]
// (RangeBitmap.Appender.add / append, :1511-1588).  Block k is rows [65536 k, 65536 (k + 1)); cell (k, i) holds
// the block's rows whose value has bit i clear.
// *max (zeroed by the caller) = the largest value, unsigned
void launch_rbb_max(hipStream_t s, const uint64_t* v, uint64_t n, unsigned long long* max);
// One pass over the blocks [k_lo, k_hi).  ws: (k_hi - k_lo) x nslices bitmaps of 8 KiB, every word of which the
// transpose writes (zeros at and past row n), so the caller zeroes nothing.
void launch_rbb_transpose(hipStream_t s, const uint64_t* v, uint64_t n, uint64_t mask, uint32_t k_lo, uint32_t k_hi,
                          int nslices, uint8_t* ws);
constexpr size_t kRbbInfoBytes = 8;  // per (block, slice) cell: the plan's (card, nruns, kind); card 0: no container
// info / size: n_blocks x nslices cells (the pass fills its own; size = slot bytes, 0 for an empty cell);
// *payload (zeroed by the caller) += the stream's payload bytes of the pass (a run: 4 per run)
void launch_rbb_plan(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int nslices, void* info,
                     uint64_t* size, unsigned long long* payload);
// off: the exclusive scan of size[] over all cells.  Writes the pass's slots and directory entries (an empty
// cell: kind kAbsent) and the blocks' container masks.
void launch_rbb_write(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int nslices, const void* info,
                      const uint64_t* off, CDesc* dir, uint64_t* masks, uint8_t* arena);

// bsibuild.hip: the key-major batch [ebM, bA[0..nbits-1]] of a bit-sliced index from n (column, value)
// pairs in device memory (RoaringBitmapSliceIndex.setValue, BSI/:299-347) [+ runOptimize].
// mm: {min, max} of the values, set to {INT_MAX, INT_MIN} by the caller
void launch_bsib_minmax(hipStream_t s, const int32_t* v, uint64_t n, int* mm);
// One pass over the key indices [k_lo, k_hi) of the K present keys (pkey_off: launch_bld_keys' CSR over
// the columns), m = nbits + 1 inputs.  ws: (k_hi - k_lo) x m bitmaps of 8 KiB, zeroed by the caller, below
// 2^31 words.
void launch_bsib_scatter(hipStream_t s, const uint32_t* col, const int32_t* val, uint64_t n, const uint32_t* pkey_off,
                         uint32_t k_lo, uint32_t k_hi, int m, uint32_t* ws);
constexpr size_t kBsibInfoBytes = 8;  // per (key index, input) cell: the plan's (card, nruns, kind)
// a cell's size word: container count (0 / 1) << kBsibCountShift | slot bytes; one scan places both
constexpr int kBsibCountShift = 40;
// info / size: K x m cells (the pass fills its own); per (4 u64 per input: containers, cardinality,
// serialized payload bytes, run containers) and kinds (3 u64) are added to: zeroed by the caller
// ebm_run (may be null; indexed by key index): cell 0 of a flagged key is a run container of one run (the
// full ebM' of an in-place union, bsiadd.hip)
void launch_bsib_plan(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int m, int run_optimize,
                      void* info, uint64_t* size, unsigned long long* per, unsigned long long* kinds,
                      const uint8_t* ebm_run = nullptr);
// scan: the exclusive scan of size[] over all K x m cells; pkeys: the K present keys
void launch_bsib_write(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int m, const void* info,
                       const uint64_t* scan, const uint16_t* pkeys, CDesc* desc, uint16_t* keys, uint32_t* bm,
                       uint8_t* payload);
// the batch's key CSR (65,537 entries); scan[K m] = the scan's total
void launch_bsib_key_off(hipStream_t s, const uint32_t* pkey_off, const uint64_t* scan, int m, uint32_t* key_off);

// bsiadd.hip: the sum of two run-free key-major batches [ebM, bA[0..n-1]] (RoaringBitmapSliceIndex.add,
// BSI/:66-95) into the workspace layout of the build above, m = 2 + max(na, nb) cells per present key:
// ebM', the slices, the carry out of the top input slice
struct BsiAddSide {
  const uint32_t* key_off;  // the batch's key CSR; null: the side takes no part (an empty operand)
  const CDesc* desc;
  const uint32_t* bm;  // input index per container
  const uint8_t* payload;
  int n;  // slices
};
// flag[key] = 1 for every container key of both batches (flag: 65,536 bytes, zeroed by the caller)
void launch_bsia_keys(hipStream_t s, const uint16_t* ka, uint64_t na, const uint16_t* kb, uint64_t nb, uint8_t* flag);
// one pass over the key indices [k_lo, k_hi); writes every cell of the pass and ebm_run[k_lo..k_hi)
void launch_bsi_add(hipStream_t s, BsiAddSide a, BsiAddSide b, const uint16_t* pkeys, uint32_t k_lo, uint32_t k_hi,
                    int m, uint8_t* ws, uint8_t* ebm_run);
// minValue() / maxValue() (BSI/:97-138) over the n_keys keys of a pass's workspace; mm = {min, max} as
// unsigned, set to {~0u, 0} by the caller
void launch_bsia_minmax(hipStream_t s, const uint8_t* ws, uint32_t n_keys, int m, uint32_t* mm);

// bsiset.hip: n (column, value) pairs, in order, written into a key-major batch [ebM, bA[0..a.n-1]]
// (RoaringBitmapSliceIndex.setValues, BSI/:349-357) in the workspace layout of the build above, m = 1 + d' cells
// per present key (the operand's keys and the columns'), d' >= a.n the depth after ensureCapacityInternal.
// One pass over the key indices [k_lo, k_hi): the operand's containers into the cells (every cell written) and
// ebm_run[k_lo..k_hi) = 1 where ebM's container is a full run container; *bad |= 1 for any other run container
void launch_bsis_expand(hipStream_t s, BsiAddSide a, const uint16_t* pkeys, uint32_t k_lo, uint32_t k_hi, int m,
                        uint8_t* ws, uint8_t* ebm_run, uint32_t* bad);
// tab[(key index - k_lo) * 65536 + (column & 0xFFFF)] = the highest pair index + 1 of the column; tab zeroed by
// the caller, n < 2^32
void launch_bsis_last(hipStream_t s, const uint32_t* col, uint64_t n, const uint32_t* pkey_off, uint32_t k_lo,
                      uint32_t k_hi, uint32_t* tab);
// the pair that holds its column's tab entry sets the column in cell 0 and sets or clears it in cells 1..m-1 by
// the bits of its value; ws: the pass's cells, below 2^31 words
void launch_bsis_apply(hipStream_t s, const uint32_t* col, const int32_t* val, uint64_t n, const uint32_t* pkey_off,
                       uint32_t k_lo, uint32_t k_hi, int m, const uint32_t* tab, uint32_t* ws);

// mutate.hip: a batch of values added to (op 0) or removed from (op 1) a resident bitmap, RoaringBitmap.add(int...)
// / addN / remove(int) (RB/RoaringBitmap.java:483-570, 2637-2648).  a: the operand (n == 0: an empty bitmap, whose
// key CSR is not read).  touched: launch_bld_keys' flags over the values.
// flag[key] = touched | present (add), touched & present (remove): the input of the second key scan
void launch_mut_flags(hipStream_t s, const uint8_t* touched, const uint32_t* a_key_off, bool a_has, int op,
                      uint8_t* flag);
// cell_keys / cell_off: the keys with an 8 KiB cell and their CSR (65,537 entries; a key has a cell iff its two
// entries differ); writes every cell of ws, was_run[] and old_card[]
void launch_mut_expand(hipStream_t s, BmView a, const uint16_t* cell_keys, uint32_t n_cells, uint8_t* ws,
                       uint8_t* was_run, uint32_t* old_card);
// v is read once more here: it must not have changed since launch_bld_keys
void launch_mut_apply(hipStream_t s, const uint32_t* v, uint64_t n, int op, const uint32_t* cell_off, uint32_t* ws);
constexpr size_t kMutInfoBytes = 8;  // per candidate key: the plan's (card, nruns, kind, kept / touched)
// a candidate's size word: 1 << kMutCountShift | slot bytes when kept, else 0; one scan places both (a batch
// holds at most 65,536 slots of at most 131,088 B)
constexpr int kMutCountShift = 44;
// cand_keys: the keys the result may hold, ascending.  totals (7 u64, zeroed by the caller) += {#A, #B, #R,
// serialized payload bytes, cardinality, values added or removed, serialized bytes of containers above 8,194 B}
void launch_mut_plan(hipStream_t s, BmView a, const uint16_t* cand_keys, uint64_t n_cand, const uint32_t* cell_off,
                     const uint8_t* ws, const uint8_t* was_run, const uint32_t* old_card, void* info, uint64_t* size,
                     unsigned long long* totals);
// off: the exclusive scan of size[]; n_out: the kept keys; also writes bm_off = {0, n_out}
void launch_mut_write(hipStream_t s, BmView a, const uint16_t* cand_keys, uint64_t n_cand, uint32_t n_out,
                      const uint32_t* cell_off, const uint8_t* ws, const void* info, const uint64_t* off, CDesc* desc,
                      uint16_t* keys, uint32_t* bm, uint32_t* bm_off, uint8_t* payload);

// bsival.hip: values out of a key-major batch [ebM, bA[0..nbits-1], foundSet?]
struct BsiValArgs {
  const uint32_t* key_off;  // the batch's key CSR (65,537 entries)
  const CDesc* desc;
  const uint32_t* bm;  // input index per container
  const uint8_t* payload;
  int nbits;
};
// out[i] = getValue(q[i]) (BSI/:181-196), -1 where ebM lacks the column; in query order
void launch_bsi_get_values(hipStream_t s, BsiValArgs a, const uint32_t* q, uint64_t n, long long* out);
// cards[k] = cardinality of ebM's container of key k (65,536 u64), to be scanned (launch_exclusive_scan)
void launch_bsi_pair_cards(hipStream_t s, BsiValArgs a, uint64_t* cards);
// toPairList() (BBSI/:534-549): every column of ebM ascending (u32, or i64 zero-extended) with its value
// (i32 or i64); base: the exclusive scan of cards
void launch_bsi_pairs(hipStream_t s, BsiValArgs a, const uint64_t* base, bool cols64, bool vals64, void* cols,
                      void* vals);

// bsiin.hip: the buffer package's parallelIn (BBSI/:611-639) over a key-major batch [ebM, bA[0..nbits-1],
// foundSet?] into the workspace layout of the build above with m = 1 cell per candidate key
constexpr uint32_t kBsiInLdsList = 4096;  // value lists up to this length are searched in LDS (16 KiB)
// list[0..n) (n < 2^31) sorted ascending with repeats dropped, in place; *n_out (device) = the entries left.
// scratch: n u32; temp: bsiin_sort_temp_bytes(n) bytes.  -> hipError_t
size_t bsiin_sort_temp_bytes(uint64_t n);
int launch_bsiin_sort_unique(hipStream_t s, void* temp, size_t temp_bytes, uint32_t* list, uint32_t* scratch,
                             unsigned long long* n_out, uint64_t n);
// flag[key] = 1 for every candidate key (65,536 bytes, all written); cards[key] = cardinality of the
// container of the foundSet (has_found) or of ebM under the key (65,536 u64), to be scanned
void launch_bsiin_keys(hipStream_t s, BsiValArgs a, int has_found, uint8_t* flag, uint64_t* cards);
// one pass over the candidate key indices [k_lo, k_hi): writes every cell of the pass and run[k_lo..k_hi).
// list: n >= 1 ascending distinct values (as unsigned bit patterns); rank: the exclusive scan of cards;
// aligned: parallelExec's batchSize is 65,536
void launch_bsi_in(hipStream_t s, BsiValArgs a, int has_found, const uint32_t* list, uint32_t n, const uint16_t* pkeys,
                   uint32_t k_lo, uint32_t k_hi, const uint64_t* rank, bool aligned, uint8_t* ws, uint8_t* run);

// bsitr.hip: the buffer package's parallelTransposeWithCount (BBSI/:551-597) over a key-major batch [ebM,
// bA[0..nbits-1], foundSet?]: a count table of 65,536 u32 per result key (value >> 16), then m cells of 8 KiB
// per result key in the workspace layout of the build above (the existence cell, then one per count bit)
struct BsiTrSweep {
  uint8_t* rflag;         // mode 0: rflag[value >> 16] = 1 (65,536 bytes, zeroed by the caller)
  const uint32_t* rkoff;  // modes 1, 2: result key -> result key index (launch_bld_keys' CSR over rflag)
  uint32_t* tab;          // mode 1: (k_hi - k_lo) x 65,536 counts, zeroed by the caller
  uint32_t k_lo, k_hi;    // mode 1: the result key indices of the pass
  const uint8_t* isfull;  // mode 2: per result key index, all 65,536 values present
  const uint64_t* rank;   // mode 2: per input key, the columns of fixed below key << 16
  unsigned long long* n_pairs;  // mode 2: pairs written (zeroed by the caller)
  uint32_t* out_rank;           // mode 2: cap entries each, in no particular order
  uint32_t* out_val;
  unsigned long long cap;
  const uint32_t* fidx;  // mode 4: per result key index, its index among the full keys, or ~0u
  uint32_t* bits;        // mode 4: per (full key, batch) a bitmap of 2,048 words, zeroed by the caller
  uint32_t n_batches, batch_size;  // mode 4: parallelExec's batches of fixed
};
// one workgroup per candidate key ckeys[0..*n_ckeys) (launch_bsiin_keys' flags through launch_bld_keys); grid:
// an upper bound of *n_ckeys known on the host (ebM's containers).  mode 0 / 1 / 2: see BsiTrSweep
void launch_bsitr_sweep(hipStream_t s, int mode, BsiValArgs a, int has_found, const uint16_t* ckeys,
                        const unsigned long long* n_ckeys, uint32_t grid, BsiTrSweep p);
// mode 4: bits[(fidx * n_batches + rank / batch_size) * 2048 ...] gets the low half of the value of every column
// whose value lies in a full key.  launch_bsitr_full_runs then walks a full key's batches in order (a workgroup
// per full key) and sets run[fki[f]] = 1 where the key is RunContainer.full()
void launch_bsitr_full_runs(hipStream_t s, const uint32_t* bits, uint32_t n_full, uint32_t n_batches,
                            const uint32_t* fki, uint8_t* run);
// mode 3 (the sparse route): out_val = the value of every column of ebM & fixed, *n_pairs of them.  Then
// vals[0..n) sorted into `sorted` and run-length encoded into (uniq, counts), *n_out runs; temp:
// bsitr_sort_temp_bytes(n) bytes; n < 2^31.  -> hipError_t
size_t bsitr_sort_temp_bytes(uint64_t n);
int launch_bsitr_sort_rle(hipStream_t s, void* temp, size_t temp_bytes, const uint32_t* vals, uint32_t* sorted,
                          uint32_t* uniq, int32_t* counts, unsigned long long* n_out, uint64_t n);
// the cells of the result key indices [k_lo, k_hi) from their count tables (m - 1 <= 32 count bits); writes
// every cell of the pass.  stats: also mm = {min, max} of the non-zero counts ({~0u, 0} set by the caller),
// kcard[ki] += the key's distinct values, isfull[ki] = 1 and *n_full += 1 for a key that reaches 65,536
// (kcard, isfull, n_full zeroed by the caller)
void launch_bsitr_cells(hipStream_t s, const uint32_t* tab, uint32_t k_lo, uint32_t k_hi, int m, uint8_t* cells,
                        bool stats, uint32_t* mm, uint32_t* kcard, uint8_t* isfull, unsigned long long* n_full);

// decode.hip: portable-format decode on the device
enum DecErr : uint32_t {
  DEC_OK = 0,
  DEC_TRUNC_COOKIE,
  DEC_BAD_COOKIE,
  DEC_TRUNC_SIZE,
  DEC_SIZE_LARGE,
  DEC_SIZE_NEG,
  DEC_TRUNC_FLAGS,
  DEC_TRUNC_DESC,
  DEC_KEY_ORDER,
  DEC_TRUNC_OFFSETS,
  DEC_TRUNC_RUNS,
  DEC_TRUNC_PAYLOAD,
};
struct DecHead {  // per input: table geometry (byte positions within the input)
  uint64_t pay_pos;
  uint32_t desc_pos, flags_pos, off_pos;
  int32_t size;
  uint32_t flags;
  uint32_t pad;
};
struct DecCtr {  // per container, input order
  uint64_t src;  // payload byte offset in the raw upload
  uint32_t len;  // serialized payload bytes
  uint32_t card;
  uint32_t bm;
  uint32_t kind;
};
void launch_dec_head(hipStream_t s, const uint8_t* raw, const uint64_t* in_off, const uint64_t* in_len, uint64_t n,
                     DecHead* hd, uint64_t* nctr, uint64_t* nch, uint32_t* err, uint32_t* any_err);
// bm_card and bm_flag zeroed by the caller; *n_chunks = sum of nch (device), max_chunks its host bound
void launch_dec_ctrs(hipStream_t s, const uint8_t* raw, const uint64_t* in_off, const uint64_t* in_len, uint64_t n,
                     const DecHead* hd, const uint64_t* ctr_base, const uint64_t* nch, const uint64_t* ch_base,
                     const uint64_t* n_chunks, uint64_t max_chunks, uint32_t* map, DecCtr* q, uint16_t* qkey,
                     uint64_t* bm_card, uint32_t* bm_flag, uint64_t* consumed, uint32_t* err, uint32_t* any_err);
size_t dec_sort_temp_bytes(uint64_t C);
// stable sort of the container keys: perm[p] = input-order index of key-major position p
int launch_dec_sort(hipStream_t s, void* temp, size_t temp_bytes, const uint16_t* qkey, uint16_t* skey,
                    uint32_t* iota, uint32_t* perm, uint64_t C);
void launch_dec_key_off(hipStream_t s, const uint16_t* skey, uint64_t C, uint32_t* key_off);
// perm null: input order.  totals (may be null) += {#A, #B, #R, bytes of payloads above 8194 B}.
// packed: array payloads at their exact length (2 B granularity, as in the portable format) instead of
// 16 B slots -- only for batches of arrays alone (every other slot stays 16 B aligned that way)
void launch_dec_sizes(hipStream_t s, const DecCtr* q, const uint32_t* perm, uint64_t C, uint64_t* size,
                      unsigned long long* totals, bool packed = false);
void launch_dec_fill(hipStream_t s, const uint8_t* raw, const DecCtr* q, const uint16_t* qkey, const uint32_t* perm,
                     const uint64_t* slot, uint64_t C, CDesc* desc, uint16_t* keys, uint32_t* bm, uint8_t* payload,
                     uint64_t* bm_card, bool packed = false);  // bm_card: run cardinalities are re-derived from the runs

}  // namespace rbg
