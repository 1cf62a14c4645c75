// Static range mutations on the MI355X: RoaringBitmap.add(rb, rangeStart, rangeEnd)
// (RB/RoaringBitmap.java:298-345), remove(rb, ...) (:995-1040), flip(rb, ...) (:626-668), and the
// buffer package's MutableRoaringBitmap.add / remove / flip (RB/buffer/MutableRoaringBitmap.java
// :152-205, 649-700, 455-505; ImmutableRoaringBitmap.flip :592-640).
//
// Keys outside [hbStart, hbLast] are cloned.  Inside, per key with the cut [lo, hi]:
//   add    : Container.add(lo, hi + 1) on the first / last key (a missing key: rangeOfOnes), a full run
//            container on every key between them
//   remove : Container.remove(lo, hi + 1) on the first / last key unless the cut covers the whole key;
//            the keys between (and fully covered ones) dropped, emptied containers dropped
//   flip   : Container.not(lo, hi + 1) on every key (a missing key: rangeOfOnes), emptied dropped
// Result types (the per-key container methods):
//   add    : ArrayContainer.add -> an array, or above 4096 values toBitmapContainer().iadd, a bitmap
//            (RB/ArrayContainer.java:103-135); BitmapContainer.add a bitmap, full included (:131-143);
//            RunContainer.add = clone().iadd, a run container whatever its size (RB/RunContainer.java:242)
//   remove : an array stays one; a bitmap becomes an array at <= 4096 values (RB/BitmapContainer.java
//            :1166-1181), the buffer package's below 4096 (RB/buffer/MappeableBitmapContainer.java
//            :1597-1612); a run container keeps its clipped runs
//   flip   : arrays / bitmaps by cardinality (ArrayContainer.not, BitmapContainer.inot), run containers
//            through toEfficientContainer (RB/RunContainer.java:1900-1918)
//   x.add(rangeStart, rangeEnd) in place (RB/RoaringBitmap.java:1181-1206, RB/buffer/MutableRoaringBitmap.java
//            :831-858): Container.iadd on every key of the range, the keys between included (an array there
//            becomes a full bitmap, a bitmap stays one, a run container a full run); the in-place remove and
//            flip end in the static forms' containers (iremove / inot keep remove / not's thresholds)
// Run results that stay run containers whatever their size (add / remove of an input with more than
// 2047 runs) go to the big-run arena (w_place_big_runs), as the buffer package's run AND results do.
//
//   k_plan_rmut : one thread per key (the pairwise plan's compaction), the keys that give a container
//   k_rmut      : one wave per task, the container in registers (wave.hpp)
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

__device__ __forceinline__ void rmut_cut(int key, const RmutArgs& ra, int* lo, int* hi) {
  *lo = key == ra.hbs ? ra.lbs : 0;
  *hi = key == ra.hbl ? ra.lbl : 65535;
}

__global__ __launch_bounds__(256) void k_plan_rmut(BmView A, RmutArgs ra, PlanOut po, uint32_t* err) {
  plan_zero(po.zlb, po.ztile);
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  PTask t;
  resolve<0>(A, k, t);
  ptask_absent<1>(t);
  t.key = (uint16_t)k;
  const bool present = t.kind_a != kAbsent;
  const bool in = (int)k >= ra.hbs && (int)k <= ra.hbl;
  int f;
  if (ra.op == RMUT_LIMIT) {
    f = present && ((int)k < ra.hbs || ((int)k == ra.hbs && ra.lbs > 0));
  } else if (!in || ra.op == RMUT_DERUN) {
    f = present;
  } else if (ra.op == RMUT_REMOVE) {
    int lo, hi;
    rmut_cut((int)k, ra, &lo, &hi);
    f = present && !(lo == 0 && hi == 65535);
  } else {
    f = 1;
  }
  plan_emit(f, t, po, err);
}

template <int OP, bool BUF>
__device__ __forceinline__ void rmut_task(uint32_t t, const PTask& tk, const uint8_t* pa, const RmutArgs& ra,
                                          const OutCtx& oc, const BigRuns& big, uint32_t* lds) {
  const int key = tk.key;
  const bool present = tk.kind_a != kAbsent;
  if (OP == RMUT_DERUN && tk.kind_a == DK_R) {  // RunContainer.toBitmapOrArrayContainer (RB/RunContainer.java:2300-2323)
    WCtr x;
    w_materialize(CDesc{tk.slot_a, tk.card_a, tk.key, tk.kind_a, 0}, pa, lds, x);
    const int c = (int)tk.card_a;
    w_emit(t, (uint32_t)key, x, c, by_card(c), oc, lds);
    return;
  }
  if (OP == RMUT_LIMIT && key == ra.hbs) {  // Container.limit(lbs): the first lbs values
    WCtr x;
    w_materialize(CDesc{tk.slot_a, tk.card_a, tk.key, tk.kind_a, 0}, pa, lds, x);
    const int n = ra.lbs;
    int base = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int c0 = __popcll(x.w[2 * i]), c1 = __popcll(x.w[2 * i + 1]);
      int tot;
      const int p0 = base + wave_excl(c0 + c1, &tot);
      base += tot;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int pre = p0 + (j ? c0 : 0), cw = j ? c1 : c0;
        uint64_t& w = x.w[2 * i + j];
        if (pre >= n) {
          w = 0;
        } else if (pre + cw > n) {  // keep the word's lowest n - pre set bits
          uint64_t rest = w;
          for (int q = 0; q < n - pre; q++) rest &= rest - 1;
          w ^= rest;
        }
      }
    }
    w_emit(t, (uint32_t)key, x, n, tk.kind_a == DK_B ? by_card(n) : tk.kind_a, oc, lds, &big);
    return;
  }
  if (OP == RMUT_DERUN || OP == RMUT_LIMIT || key < ra.hbs || key > ra.hbl) {  // cloned: outside the range,
                                                                                // not a run container, or kept whole
    w_clone(t, tk, pa, oc, lds);
    return;
  }
  int lo, hi;
  rmut_cut(key, ra, &lo, &hi);
  constexpr bool ADD = OP == RMUT_ADD || OP == RMUT_ADD_INPLACE || OP == RMUT_RANGE;
  if ((OP == RMUT_ADD || OP == RMUT_RANGE) && key != ra.hbs && key != ra.hbl) {  // rangeOfOnes(0, 65536)
    w_full_run(t, (uint32_t)key, oc, lds);
    return;
  }
  if (!present) {  // add / flip: Container.rangeOfOnes(lo, hi + 1); bitmapOfRange: RunContainer's, never an array
    w_range_of_ones(t, (uint32_t)key, lo, hi, OP != RMUT_RANGE, oc, lds);
    return;
  }
  WCtr x;
  w_materialize(CDesc{tk.slot_a, tk.card_a, tk.key, tk.kind_a, 0}, pa, lds, x);
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint64_t m = wrange(k, lo, hi);
    if (ADD) x.w[k] |= m;
    else if (OP == RMUT_REMOVE) x.w[k] &= ~m;
    else x.w[k] ^= m;
  }
  const int c = w_card(x);
  if (c == 0) {  // remove / flip emptied the container: dropped
    w_drop(t, (uint32_t)key, oc, lds);
    return;
  }
  const int kx = tk.kind_a;
  int kind;
  if (ADD) kind = kx == DK_A ? by_card(c) : kx;
  else if (OP == RMUT_REMOVE) kind = kx == DK_B ? ((BUF ? c < 4096 : c <= 4096) ? DK_A : DK_B) : kx;
  else kind = kx == DK_R ? eff(c, w_runs(x)) : by_card(c);
  // add / remove keep a run container one whatever its size; flip's toEfficientContainer at most 2047 runs
  w_emit(t, (uint32_t)key, x, c, kind, oc, lds, OP != RMUT_FLIP ? &big : nullptr);
}

constexpr int kRmWaves = 4;

template <int OP, bool BUF>
__global__ __launch_bounds__(256, 4) void k_rmut(const PTask* __restrict__ tasks, const uint32_t* __restrict__ n_tasks,
                                              const uint8_t* pa, RmutArgs ra, OutCtx oc, BigRuns big) {
  __shared__ __align__(16) uint32_t lds_all[kRmWaves][2048];
  for_each_wave_task(tasks, n_tasks, lds_all, [&](uint32_t t, const PTask& tk, uint32_t* lds) {
    rmut_task<OP, BUF>(t, tk, pa, ra, oc, big, lds);
  });
}

void launch_rmut(hipStream_t s, BmView A, RmutArgs ra, bool buf, PlanOut po, OutCtx oc, BigRuns big, int grid) {
  hipLaunchKernelGGL(k_plan_rmut, dim3(256), dim3(256), 0, s, A, ra, po, oc.err);
  auto run = [&](auto op, auto b) {
    launch_resident<k_rmut<decltype(op)::value, decltype(b)::value != 0>>(s, grid, kRmWaves, po.tasks, po.n_tasks,
                                                                         A.payload, ra, oc, big);
  };
  switch (ra.op) {
    case RMUT_ADD: run(Int<RMUT_ADD>{}, Int<0>{}); break;
    case RMUT_ADD_INPLACE: run(Int<RMUT_ADD_INPLACE>{}, Int<0>{}); break;
    case RMUT_DERUN: run(Int<RMUT_DERUN>{}, Int<0>{}); break;
    case RMUT_LIMIT: run(Int<RMUT_LIMIT>{}, Int<0>{}); break;
    case RMUT_RANGE: run(Int<RMUT_RANGE>{}, Int<0>{}); break;
    case RMUT_FLIP: run(Int<RMUT_FLIP>{}, Int<0>{}); break;
    default: buf ? run(Int<RMUT_REMOVE>{}, Int<1>{}) : run(Int<RMUT_REMOVE>{}, Int<0>{}); break;
  }
}

}  // namespace rbg
