// RoaringBitmap.orNot on the MI355X: the static RoaringBitmap.orNot(x1, x2, rangeEnd)
// (RB/RoaringBitmap.java:1521-1603) and x1.orNot(x2, rangeEnd) in place (:1431-1506).
//
// Per key k <= maxKey = (rangeEnd - 1) >>> 16, with end = lastRun at maxKey, else 65536:
//   x1 and x2 : c1.orNot(c2, end) = c1.or(c2.not(0, end).iremove(end, 0x10000)) (RB/Container.java
//               :191-196; the in-place form iorNot :536-541 ends in ior)
//   x1 only   : full, or c1.ior(rangeOfOnes(0, lastRun)) at maxKey
//   x2 only   : c2.not(0, end) -- not clipped at rangeEnd
//   neither   : full, or rangeOfOnes(0, lastRun) at maxKey
// empty results dropped; then x1's containers above maxKey, as they are.  The reference sizes its
// key array with maxSize = min(maxKey + 1 + remainder - correction + |x1|, 65536) and stops the key
// loop once that many containers are out -- which can cut the result short (correction counts full
// x2 containers, some of which sit under an x1 container); k_ornot_scan computes the same bound.
//
//   k_ornot_scan : one workgroup: remainder, correction, maxSize, and the number of keys the loop
//                  reaches (an exact walk only when maxSize < maxKey + 1)
//   k_plan_ornot : one thread per key (the pairwise plan's compaction): the reached keys [0, k_end)
//                  and x1's keys above maxKey, in key order
//   k_ornot      : one wave per task; the container in registers (wave.hpp), typed as the
//                  reference's chain: not() -> iremove -> or / ior.  Full containers (the bulk of a
//                  dense result) reference one constant run payload; nothing is staged for them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

// 1024-thread block sum / inclusive scan (LDS `red` of 17 ints)
__device__ __forceinline__ int ornot_block_sum(int v, int* red) {
  v = wave_sum_i(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) s += red[i];
  __syncthreads();
  return s;
}
__device__ __forceinline__ int ornot_block_incl(int v, int* red, int* total) {
  const int incl = dpp_incl_scan(v);
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = incl;
  __syncthreads();
  int before = 0, s = 0;
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    before += i < w ? red[i] : 0;
    s += red[i];
  }
  __syncthreads();
  *total = s;
  return before + incl;
}

// RB/RoaringBitmap.java:1527-1548 (static) / :1436-1458 (in place): remainder = x1's keys above
// maxKey; correction = full x2 containers among indices [0, |x2| - remainder), up to and including the
// first key >= maxKey; maxSize.  The loop `for key <= maxKey && size < maxSize` reaches key k iff the
// non-empty results before k number fewer than maxSize; a result is empty only for an x2-only full
// container below maxKey (its complement), so that count is k - E(k), E(k) = such keys below k.
__global__ __launch_bounds__(1024) void k_ornot_scan(const uint32_t* __restrict__ koa, int na,
                                                     const uint32_t* __restrict__ kob, const CDesc* __restrict__ db,
                                                     int nb, int max_key, OrNotPlan* __restrict__ plan) {
  __shared__ int red[17];
  const int th = threadIdx.x;
  const int rem = na - (int)koa[max_key + 1];
  const int lim = nb - rem;
  int last = -1;
  if (lim > 0) last = min(max_key < 0 ? 0 : (int)kob[max_key], lim - 1);
  int c = 0;
  for (int i = th; i <= last; i += 1024) c += db[i].card == 65536u;
  const int corr = ornot_block_sum(c, red);
  const int max_size = min(max_key + 1 + rem - corr + na, 65536);
  int k_end = max_key + 1;
  if (max_size < 0) {
    k_end = 0;
  } else if (max_size < max_key + 1) {  // the bound can bind: walk the keys in 1024-key segments
    int e_before = 0, reached = 0;
    for (int s0 = 0; s0 <= max_key; s0 += 1024) {
      const int k = s0 + th;
      int e = 0;
      if (k < max_key) {
        const uint32_t b0 = kob[k];
        e = kob[k + 1] > b0 && koa[k + 1] == koa[k] && db[b0].card == 65536u;
      }
      int tot;
      const int incl = ornot_block_incl(e, red, &tot);
      const int nonempty_before = k - (e_before + incl - e);
      reached += ornot_block_sum(k <= max_key && nonempty_before < max_size, red);
      e_before += tot;
    }
    k_end = reached;
  }
  if (th == 0) {
    plan->k_end = k_end;
    plan->neg = max_size < 0 ? 1 : 0;
    plan->max_size = max_size;
    plan->correction = corr;
  }
}

// one thread per key: tasks for the keys the loop reaches and for x1's keys above maxKey
__global__ __launch_bounds__(256) void k_plan_ornot(BmView A, BmView B, int max_key,
                                                    const OrNotPlan* __restrict__ plan, PlanOut po, uint32_t* err) {
  plan_zero(po.zlb, po.ztile);
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  PTask t;
  resolve<0>(A, k, t);
  resolve<1>(B, k, t);
  t.key = (uint16_t)k;
  const int k_end = plan->k_end;
  int f = (int)k < k_end || ((int)k > max_key && t.kind_a != kAbsent);
  if (plan->neg) f = 0;
  plan_emit(f, t, po, err);
}

// bits [0, e) of container word w
__device__ __forceinline__ uint64_t prefix_mask(int w, int e) {
  const int lo = 64 * w;
  if (e >= lo + 64) return ~0ull;
  if (e <= lo) return 0ull;
  return (1ull << (e - lo)) - 1;
}
// ... of register k of the wave layout (WCtr: w[2 i + j] = word 128 i + 2 lane + j)
__device__ __forceinline__ uint64_t wprefix(int k, int e) {
  return prefix_mask(128 * (k >> 1) + 2 * lane_id() + (k & 1), e);
}

// One task, one wave (20 waves per CU in flight: the per-task chain is a few dependent memory
// latencies, so the task rate comes from the waves in flight).  Result types:
//  * c2.not(0, e): ArrayContainer.not (RB/ArrayContainer.java:876-925, through toBitmapContainer().not
//    above 4096 values) and BitmapContainer.not = clone().inot (RB/BitmapContainer.java:994-997, 679-687)
//    give an array at <= 4096 values, else a bitmap; RunContainer.not (RB/RunContainer.java:1900-1918)
//    ends in toEfficientContainer;
//  * .iremove(e, 0x10000) (both present, e < 65536): an array stays an array, a bitmap becomes one at
//    <= 4096 values (RB/BitmapContainer.java:788-802), a run container stays one; BUF: the buffer
//    package's MappeableBitmapContainer.iremove converts only below 4096 values
//    (RB/buffer/MappeableBitmapContainer.java:1003-1017), so a 4096-value bitmap keeps its words;
//  * rangeOfOnes(0, e) (RB/Container.java:29-37): an array up to 2 values, else a run container;
//  * c1.or / c1.ior of that: the pairwise OR rule (device.hpp); Container.ior's one difference,
//    BitmapContainer.ior(ArrayContainer) keeping a full bitmap (RB/BitmapContainer.java:740-757),
//    applies to x1-only at maxKey in both forms and to both-present in the in-place form.
template <bool INPLACE, bool BUF>
__device__ __forceinline__ void ornot_task(uint32_t t, const PTask& tk, const uint8_t* pa, const uint8_t* pb,
                                           int max_key, int last_run, const OutCtx& oc, uint32_t* lds) {
  const int key = tk.key;
  const bool ia = tk.kind_a != kAbsent, ib = tk.kind_b != kAbsent;
  if (key > max_key) {  // x1's containers above the range, appended as they are (:1493-1500 / :1588-1596)
    w_clone(t, tk, pa, oc, lds);
    return;
  }
  const int e = key == max_key ? last_run : 65536;
  if (!ib && e == 65536) {
    // RunContainer.full(); at maxKey with lastRun = 0x10000, x1's c1.ior(full run) and the full
    // rangeOfOnes are full run containers as well (RunContainer.or / BitmapContainer.ior(RunContainer) /
    // RunContainer.ior return full() on a full union)
    w_full_run(t, (uint32_t)key, oc, lds);
    return;
  }
  if (!ia && !ib) {  // rangeOfOnes(0, lastRun) at maxKey
    w_range_of_ones(t, (uint32_t)key, 0, e - 1, true, oc, lds);
    return;
  }
  WCtr x, y;
  const int kx = ia ? tk.kind_a : DK_A, cx = ia ? (int)tk.card_a : 0;
  if (ia) w_materialize(CDesc{tk.slot_a, tk.card_a, tk.key, tk.kind_a, 0}, pa, lds, x);
  int ky, cy;
  if (ib) {
    w_materialize(CDesc{tk.slot_b, tk.card_b, tk.key, tk.kind_b, 0}, pb, lds, y);
#pragma unroll
    for (int k = 0; k < 16; k++) y.w[k] ^= wprefix(k, e);
    cy = w_card(y);
    ky = tk.kind_b == DK_R ? eff(cy, w_runs(y)) : by_card(cy);
    if (ia && e < 65536) {
#pragma unroll
      for (int k = 0; k < 16; k++) y.w[k] &= wprefix(k, e);
      cy = w_card(y);
      if (ky == DK_B && (BUF ? cy < 4096 : cy <= 4096)) ky = DK_A;
    }
  } else {  // x1 only, maxKey: c1.ior(rangeOfOnes(0, e))
#pragma unroll
    for (int k = 0; k < 16; k++) y.w[k] = wprefix(k, e);
    cy = e;
    ky = e <= 2 ? DK_A : DK_R;
  }
  int kz, cz;
  if (ia) {
#pragma unroll
    for (int k = 0; k < 16; k++) x.w[k] |= y.w[k];
    cz = w_card(x);
    kz = pairwise_needs_runs(OPR_OR, kx, cx, ky, cy) ? eff(cz, w_runs(x)) : pairwise_kind(OPR_OR, kx, ky, cz);
    if ((INPLACE || !ib) && kx == DK_B && ky == DK_A) kz = DK_B;
  } else {  // x2 only: its complement, dropped when empty
    if (cy == 0) {
      w_drop(t, (uint32_t)key, oc, lds);
      return;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) x.w[k] = y.w[k];
    cz = cy;
    kz = ky;
  }
  w_emit(t, (uint32_t)key, x, cz, kz, oc, lds);
}

constexpr int kOrnWaves = 4;

// INPLACE: x1.orNot (iorNot, ior); BUF: the buffer package's ImmutableRoaringBitmap.orNot /
// MutableRoaringBitmap.orNot (RB/buffer/ImmutableRoaringBitmap.java:484-548, MutableRoaringBitmap.java
// :962-1030).
template <bool INPLACE, bool BUF>
__global__ __launch_bounds__(256, 3) void k_ornot(const PTask* __restrict__ tasks, const uint32_t* __restrict__ n_tasks,
                                               const uint8_t* pa, const uint8_t* pb, int max_key, int last_run,
                                               OutCtx oc) {
  __shared__ __align__(16) uint32_t lds_all[kOrnWaves][2048];
  for_each_wave_task(tasks, n_tasks, lds_all, [&](uint32_t t, const PTask& tk, uint32_t* lds) {
    ornot_task<INPLACE, BUF>(t, tk, pa, pb, max_key, last_run, oc, lds);
  });
}

void launch_ornot(hipStream_t s, BmView A, BmView B, int max_key, int last_run, int flags, OrNotPlan* plan, PlanOut po,
                  OutCtx oc, int grid) {
  hipLaunchKernelGGL(k_ornot_scan, dim3(1), dim3(1024), 0, s, A.key_off, A.n, B.key_off, B.desc, B.n, max_key, plan);
  hipLaunchKernelGGL(k_plan_ornot, dim3(256), dim3(256), 0, s, A, B, max_key, plan, po, oc.err);
  auto run = [&](auto inplace, auto buf) {
    launch_resident<k_ornot<decltype(inplace)::value != 0, decltype(buf)::value != 0>>(
        s, grid, kOrnWaves, po.tasks, po.n_tasks, A.payload, B.payload, max_key, last_run, oc);
  };
  switch (flags & 3) {
    case 0: run(Int<0>{}, Int<0>{}); break;
    case 1: run(Int<1>{}, Int<0>{}); break;
    case 2: run(Int<0>{}, Int<1>{}); break;
    default: run(Int<1>{}, Int<1>{}); break;
  }
}

}  // namespace rbg
