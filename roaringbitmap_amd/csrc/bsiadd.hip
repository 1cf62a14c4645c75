// The column-wise sum of two resident bit-sliced indexes: RoaringBitmapSliceIndex.add (BSI/:66-95; the
// buffer package's MutableBitSliceIndex.add, bsi/.../buffer/MutableBitSliceIndex.java:121-130, 201-262) for
// two run-free key-major batches [ebM, bA[0..na-1]] and [ebM, bA[0..nb-1]], as a new batch in bsibuild.hip's
// workspace layout so that its plan / scan / write stages type and place the result:
//
//   k_bsia_keys    flag[key] for every container of both batches; k_bld_key_scan (build.hip) turns the
//                  flags into the K present keys and their CSR, as for the build's columns
//   k_bsi_add      one wave per present key.  Cell 0 of the key = ebM_a | ebM_b, with a per-key flag where
//                  Container.ior leaves a full result as a one-run run container.  Then the reference's
//                  addDigit chain as a ripple-carry adder over the key's 1024 words: the carry stays in
//                  registers, slice i of either side is materialised (a missing container is zero),
//                  s = a ^ b ^ c goes to cell 1 + i, c = (a & b) | (c & (a ^ b)); the carry left after the
//                  last input slice goes to the top cell.  Every cell of the key is written: the
//                  workspace needs no memset.  ebM is never consulted (addDigit does not).
//   k_bsia_minmax  minValue() / maxValue() (BSI/:97-138) from the workspace: per 64-bit word the descent
//                  from the top slice down, cand = ebM' word, max keeps cand & s_i and min cand & ~s_i
//                  where that is non-zero; one wave per key, or per 1 KiB chunk of a key when the keys
//                  are few; one unsigned atomic min / max per wave.
//
// A key's chain does not depend on other keys (the reference's global carry.isEmpty() only ends the
// recursion early), and with run-free inputs every slice container of the reference's result has the type
// its final cardinality gives (xor / and results), which is what k_bsib_plan assigns.
#include <algorithm>

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

constexpr uint32_t kBsiaSplitKeys = 512;  // k_bsia_minmax: below, eight waves share a key

__global__ __launch_bounds__(256) void k_bsia_keys(const uint16_t* __restrict__ ka, uint64_t na,
                                                   const uint16_t* __restrict__ kb, uint64_t nb,
                                                   uint8_t* __restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += stride)
    flag[i < na ? ka[i] : kb[i - na]] = 1;
}

// cell (ki, j) of the pass at ws + 8192 ((ki - k_lo) m + j), m = 2 + max(na, nb); ebm_run[ki]: ebM' is full
// and the reference holds it as a run container
__global__ __launch_bounds__(256) void k_bsi_add(const BsiAddSide A, const BsiAddSide B,
                                                 const uint16_t* __restrict__ pkeys, uint32_t k_lo, uint32_t k_hi,
                                                 int m, uint8_t* __restrict__ ws, uint8_t* __restrict__ ebm_run) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const uint32_t ki = k_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ki >= k_hi) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint32_t key = uni(pkeys[ki]);
  uint32_t pa = 0, ea = 0, pb = 0, eb = 0;
  if (A.key_off) {
    pa = uni(A.key_off[key]);
    ea = uni(A.key_off[key + 1]);
  }
  if (B.key_off) {
    pb = uni(B.key_off[key]);
    eb = uni(B.key_off[key + 1]);
  }
  uint8_t* cell = ws + 8192ull * ((uint64_t)(ki - k_lo) * (uint64_t)m);
  WCtr x, y, c;
  {  // ebM' = ebM_a | ebM_b (this.ebM.or(otherBsi.ebM), in place)
    const bool ha = seg_find(A.bm, pa, ea, 0), hb = seg_find(B.bm, pb, eb, 0);
    int kind_b = -1;
    if (ha) w_materialize(A.desc[pa], A.payload, lds, x);
    else w_zero(x);
    if (hb) {
      const CDesc d = B.desc[pb];
      kind_b = d.kind;
      w_materialize(d, B.payload, lds, y);
#pragma unroll
      for (int k = 0; k < 16; k++) x.w[k] |= y.w[k];
    }
    w_store_bitmap(cell, x);
    // Container.ior: a full result is RunContainer.full() when the other side is a bitmap
    // (BitmapContainer.ior(BitmapContainer), ArrayContainer.ior -> BitmapContainer.or(ArrayContainer));
    // this = bitmap, other = array stays a bitmap; a key of one side alone is a clone
    bool run = false;
    if (ha && hb && kind_b == DK_B) run = w_card(x) == 65536;
    if (lane_id() == 0) ebm_run[ki] = run ? 1 : 0;
  }
  w_zero(c);
  const int top = m - 2;  // max(na, nb)
  for (int i = 0; i < top; i++) {
    const uint32_t j = (uint32_t)i + 1;
    const bool ha = i < A.n && seg_find(A.bm, pa, ea, j), hb = i < B.n && seg_find(B.bm, pb, eb, j);
    if (ha) w_materialize(A.desc[pa], A.payload, lds, x);
    else w_zero(x);
    if (hb) w_materialize(B.desc[pb], B.payload, lds, y);
    else w_zero(y);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const uint64_t t = x.w[k] ^ y.w[k];
      x.w[k] = (x.w[k] & y.w[k]) | (c.w[k] & t);  // the carry out
      y.w[k] = t ^ c.w[k];                        // the sum
      c.w[k] = x.w[k];
    }
    w_store_bitmap(cell + 8192ull * j, y);
  }
  w_store_bitmap(cell + 8192ull * (uint64_t)(m - 1), c);
}

// mm[0] = min, mm[1] = max over the columns of ebM', slices as unsigned bits (set to {~0u, 0} by the caller).
// A key's bitmaps are eight 1 KiB chunks (a lane owns two 64-bit words of a chunk); `split` (1 or 8) waves
// share a key, 8 / split chunks each.  The descent is a chain of m - 1 dependent steps per chunk, so the
// next slice's words are requested before the current ones are used.
__global__ __launch_bounds__(256) void k_bsia_minmax(const uint8_t* __restrict__ ws, uint32_t n_keys, int m,
                                                     uint32_t split, uint32_t* __restrict__ mm) {
  const int lane = lane_id();
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= split * n_keys) return;
  const uint32_t per = 8u / split, c0 = (w % split) * per;
  const uint4* key = reinterpret_cast<const uint4*>(ws + 8192ull * ((uint64_t)(w / split) * (uint64_t)m)) + lane;
  uint32_t lo = 0xFFFFFFFFu, hi = 0;
  for (uint32_t ch = c0; ch < c0 + per; ch++) {
    const uint4* cell = key + 64 * ch;
    const uint4 e = cell[0];
    const uint64_t e0 = (uint64_t)e.x | ((uint64_t)e.y << 32), e1 = (uint64_t)e.z | ((uint64_t)e.w << 32);
    if (__ballot((e0 | e1) != 0) == 0) continue;  // wave-uniform: no column in this chunk
    uint64_t mx0 = e0, mx1 = e1, mn0 = e0, mn1 = e1;
    uint32_t vx0 = 0, vx1 = 0, vn0 = 0, vn1 = 0;
    uint4 nxt = cell[512 * (m - 1)];
    for (int sl = m - 2; sl >= 0; sl--) {  // slice sl in cell 1 + sl; bit 32 exists only in a refused sum
      const uint4 v = nxt;
      if (sl > 0) nxt = cell[512 * sl];
      const uint64_t s0 = (uint64_t)v.x | ((uint64_t)v.y << 32), s1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
      const uint32_t bit = sl < 32 ? 1u << sl : 0u;
      uint64_t t = mx0 & s0;
      if (t) mx0 = t, vx0 |= bit;
      t = mx1 & s1;
      if (t) mx1 = t, vx1 |= bit;
      t = mn0 & ~s0;
      if (t) mn0 = t;
      else vn0 |= bit;
      t = mn1 & ~s1;
      if (t) mn1 = t;
      else vn1 |= bit;
    }
    if (e0) lo = min(lo, vn0), hi = max(hi, vx0);
    if (e1) lo = min(lo, vn1), hi = max(hi, vx1);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
  }
  if (lane == 0 && lo <= hi) {
    atomicMin(&mm[0], lo);
    atomicMax(&mm[1], hi);
  }
}

void launch_bsia_keys(hipStream_t s, const uint16_t* ka, uint64_t na, const uint16_t* kb, uint64_t nb, uint8_t* flag) {
  if (!(na + nb)) return;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((na + nb + 255) / 256, 4096));
  hipLaunchKernelGGL(k_bsia_keys, dim3(grid), dim3(256), 0, s, ka, na, kb, nb, flag);
}

void launch_bsi_add(hipStream_t s, BsiAddSide a, BsiAddSide b, const uint16_t* pkeys, uint32_t k_lo, uint32_t k_hi,
                    int m, uint8_t* ws, uint8_t* ebm_run) {
  if (k_hi <= k_lo) return;
  hipLaunchKernelGGL(k_bsi_add, dim3((k_hi - k_lo + 3) / 4), dim3(256), 0, s, a, b, pkeys, k_lo, k_hi, m, ws, ebm_run);
}

void launch_bsia_minmax(hipStream_t s, const uint8_t* ws, uint32_t n_keys, int m, uint32_t* mm) {
  if (!n_keys) return;
  // measured: a wave per chunk wins at 16 and 256 keys, a wave per key at 1,024 (one wave per
  // SIMD of the device already)
  const uint32_t split = n_keys < kBsiaSplitKeys ? 8u : 1u;
  hipLaunchKernelGGL(k_bsia_minmax, dim3((split * n_keys + 3) / 4), dim3(256), 0, s, ws, n_keys, m, split, mm);
}

}  // namespace rbg
