// RoaringBitmap.addOffset(x, offset) on the MI355X (RB/RoaringBitmap.java:230-288; the buffer package's
// MutableRoaringBitmap.addOffset, RB/buffer/MutableRoaringBitmap.java:84-142, types alike).
//
// offset = 65536 co + off, off in [0, 65535] (the reference's floor division).  off == 0: every container
// is cloned under key + co (keys outside [0, 65535] dropped).  Otherwise output key k is the union of
//   P: the part of input container k - co - 1 that crosses 65536 (Util.addOffset's high part, values
//      v + off - 65536)
//   Q: the part of input container k - co that stays (the low part, values v + off)
// and its type is what the reference's chain gives (RB/Util.java:32-126, then Container.ior of the low
// part into the previous high part, then RoaringBitmap.repairAfterLazy :2752-2757):
//   parts: an array's are arrays; a bitmap's go through BitmapContainer.repairAfterLazy (<= 4096 values
//          an array; never full, as a part of a shifted container cannot be); a run container's are run
//          containers (toEfficientContainer at the end)
//   one part: its type (a run part through toEfficientContainer)
//   two parts (disjoint: P below off, Q from off up): with a bitmap part, a bitmap, or a full run
//          container when full -- except bitmap P OR array Q (BitmapContainer.ior(ArrayContainer),
//          RB/BitmapContainer.java:740-757), which keeps a full bitmap; else with a run part,
//          toEfficientContainer; else two arrays by cardinality (ArrayContainer.ior :726-745)
//
//   k_plan_aoff : one thread per output key, the keys with an input container at k - co or k - co - 1
//   k_aoff      : one wave per contiguous chunk of tasks: P and Q materialised in registers, the words
//                 of both that reach the output written into an 8 KiB LDS window at a wave-uniform word
//                 offset, the output read from it as a funnel shift of adjacent words; the next key's
//                 P is this key's Q, kept in registers
#include <algorithm>

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

__global__ __launch_bounds__(256) void k_plan_aoff(BmView A, AoffArgs aa, PlanOut po, uint32_t* err) {
  plan_zero(po.zlb, po.ztile);
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  PTask t;
  t.key = (uint16_t)k;
  const int q = k - aa.co, p = q - 1;
  if (!aa.none && q >= 0 && q <= 65535) resolve<0>(A, (uint32_t)q, t);
  else ptask_absent<0>(t);
  if (!aa.none && aa.off != 0 && p >= 0 && p <= 65535) resolve<1>(A, (uint32_t)p, t);
  else ptask_absent<1>(t);
  plan_emit(t.kind_a != kAbsent || t.kind_b != kAbsent, t, po, err);
}

// the kind of a nonempty part of an input container of kind `kind` holding `pc` values
__device__ __forceinline__ int part_kind(int kind, int pc) {
  if (kind == DK_B) return by_card(pc);  // BitmapContainer.repairAfterLazy (RB/BitmapContainer.java:1205-1215)
  return kind;
}

// Per-wave state across consecutive tasks: a task whose P is the previous task's Q (output keys k - 1
// and k) takes it from the registers, so each input container is materialised once per chunk.
struct AoffCarry {
  WCtr q;         // the previous task's Q container (all its bits)
  int prev_key;   // key of the previous task (-2: none)
  int prev_q;     // the previous task had a Q container
  int prev_high;  // that container's values in [s, 65535]: the next key's P part
};

__device__ __forceinline__ void aoff_task(uint32_t t, const PTask& tk, const uint8_t* pa, const AoffArgs& aa,
                                          const OutCtx& oc, uint32_t* lds, AoffCarry& cy) {
  const int key = tk.key;
  if (aa.off == 0) {  // a clone under the shifted key
    w_clone(t, tk, pa, oc, lds);
    return;
  }
  const int s = 65536 - aa.off;  // P's part is its bits [s, 65535], Q's its bits [0, s - 1]
  const int sb = s >> 6, r = s & 63;
  WCtr p;
  int cp = 0;
  if (tk.kind_b != kAbsent && cy.prev_key == key - 1 && cy.prev_q) {
    p = cy.q;
    cp = cy.prev_high;
  } else if (tk.kind_b != kAbsent) {
    w_materialize(CDesc{tk.slot_b, tk.card_b, tk.key, tk.kind_b, 0}, pa, lds, p);
#pragma unroll
    for (int k = 0; k < 16; k++) cp += __popcll(p.w[k] & wrange(k, s, 65535));
    cp = wave_sum_i(cp);
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) p.w[k] = 0;
  }
  int cq = 0, qhigh = 0;
  if (tk.kind_a != kAbsent) {
    w_materialize(CDesc{tk.slot_a, tk.card_a, tk.key, tk.kind_a, 0}, pa, lds, cy.q);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      cq += __popcll(cy.q.w[k] & wrange(k, 0, s - 1));
      qhigh += __popcll(cy.q.w[k] & wrange(k, s, 65535));
    }
    cq = wave_sum_i(cq);
    qhigh = wave_sum_i(qhigh);
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) cy.q.w[k] = 0;
  }
  cy.prev_key = key;
  cy.prev_q = tk.kind_a != kAbsent;
  cy.prev_high = qhigh;
  // window W[j] = (P || Q) word j + sb, j in [0, 1024]: P's words from sb on, Q's words up to sb
  uint64_t* win = reinterpret_cast<uint64_t*>(lds);
  const int l = lane_id();
  wsync();
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int w = 128 * (k >> 1) + 2 * l + (k & 1);
    if (w >= sb) win[w - sb] = p.w[k];
    if (w <= sb) win[w + 1024 - sb] = cy.q.w[k];
  }
  wsync();
  // output bit b = window bit b + r
  WCtr& x = p;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int w = 128 * (k >> 1) + 2 * l + (k & 1);
    const uint64_t lo = win[w];
    x.w[k] = r ? (lo >> r) | (win[w + 1] << (64 - r)) : lo;
  }
  const int c = w_card(x);
  if (c == 0) {  // both parts empty
    w_drop(t, (uint32_t)key, oc, lds);
    return;
  }
  int kind;
  if (cp == 0 || cq == 0) {
    const int pk = cp ? part_kind(tk.kind_b, cp) : part_kind(tk.kind_a, cq);
    kind = pk == DK_R ? eff(c, w_runs(x)) : pk;
  } else {
    const int tp = part_kind(tk.kind_b, cp), tq = part_kind(tk.kind_a, cq);
    if (tp == DK_B || tq == DK_B) kind = (c == 65536 && !(tp == DK_B && tq == DK_A)) ? DK_R : DK_B;
    else if (tp == DK_R || tq == DK_R) kind = eff(c, w_runs(x));
    else kind = by_card(c);
  }
  // a run result here holds <= 2047 runs (toEfficientContainer, or the full container)
  w_emit(t, (uint32_t)key, x, c, kind, oc, lds);
}

constexpr int kAoWaves = 4;
constexpr int kAoLds = 2064;  // u32 per wave: the 8 KiB scratch / staging area and the window's 1025th word

// one wave per contiguous chunk of tasks (consecutive keys share an input container)
__global__ __launch_bounds__(256) void k_aoff(const PTask* __restrict__ tasks, const uint32_t* __restrict__ n_tasks,
                                              const uint8_t* pa, AoffArgs aa, OutCtx oc) {
  __shared__ __align__(16) uint32_t lds_all[kAoWaves][kAoLds];
  AoffCarry cy;
  cy.prev_key = -2;
  cy.prev_q = 0;
  cy.prev_high = 0;
  for_each_wave_task<kChunked>(tasks, n_tasks, lds_all, [&](uint32_t t, const PTask& tk, uint32_t* lds) {
    aoff_task(t, tk, pa, aa, oc, lds, cy);
  });
}

void launch_aoff(hipStream_t s, BmView A, AoffArgs aa, PlanOut po, OutCtx oc, int grid) {
  hipLaunchKernelGGL(k_plan_aoff, dim3(256), dim3(256), 0, s, A, aa, po, oc.err);
  launch_resident<k_aoff>(s, grid, kAoWaves, po.tasks, po.n_tasks, A.payload, aa, oc);
}

}  // namespace rbg
