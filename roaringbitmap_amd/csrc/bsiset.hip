// (column, value) pairs written into a resident bit-sliced index: RoaringBitmapSliceIndex.setValues(List<Pair>)
// (BSI/:349-357; setValue, :299-313, is its n == 1 case; the buffer package's MutableBitSliceIndex.setValues,
// bsi/.../buffer/MutableBitSliceIndex.java:146-195, is the same loop) for a key-major batch [ebM, bA[0..d-1]]
// and n pairs in order, columns repeated at will, as a new batch in bsibuild.hip's workspace layout so that
// its plan / scan / write stages type and place the result.  m = 1 + d' cells per present key (d': the depth
// after ensureCapacityInternal, BSI/:315-326), and after a pass's cells a table of 65,536 u32 per key:
//
//   k_bsia_keys (bsiadd.hip) and k_bld_keys / k_bld_key_scan (build.hip): the present keys are the
//                   operand's container keys and the columns' high halves
//   k_bsis_expand   one wave per present key: the operand's containers of the key materialised into the
//                   cells, a missing container and every grown slice as zeros.  Every cell of the pass is
//                   written: the workspace needs no memset.  A full run container of ebM stays one
//                   (RunContainer.add returns this for a value inside a run, RB/RunContainer.java:248-263):
//                   the per-key flag k_bsib_plan reads.  Any other run container raises *bad.
//   k_bsis_last     tab[key index][column & 0xFFFF] = max(pair index + 1): setValueInternal runs in pair
//                   order, so the pair with the highest index decides a column
//   k_bsis_apply    one pair per lane; the pair that holds its column's table entry ORs the column's bit into
//                   ebM's cell and, per slice i < d', ORs it in where bit i of the value is set and ANDs it
//                   out otherwise (BSI/:304-313).  One pair per column applies, so a bit is never set and
//                   cleared in one pass; different columns of a word meet in atomics.  Lanes whose neighbours
//                   hit the same 32-bit word combine their bits first (wave.hpp: LaneGroup, over two words:
//                   the bits to set and the bits to clear), and the last lane of such a group reads the word
//                   and issues an atomic only for what would change.
//
// Types: ArrayContainer.add turns into a bitmap container above 4,096 values (RB/ArrayContainer.java:143-171),
// BitmapContainer.remove into an array container at 4,096 (RB/BitmapContainer.java:1184-1202),
// BitmapContainer.add returns this (:149-159) and RoaringBitmap.remove drops an emptied container, so with
// run-free slices every result container has the type its final cardinality gives -- a container of 65,536
// values is a bitmap container -- which is what k_bsib_plan assigns without run_optimize.
#include <algorithm>

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

// cell (ki, j) of the pass at ws + 8192 ((ki - k_lo) m + j), m = 1 + d' >= 1 + A.n
__global__ __launch_bounds__(256) void k_bsis_expand(const BsiAddSide A, const uint16_t* __restrict__ pkeys,
                                                     uint32_t k_lo, uint32_t k_hi, int m, uint8_t* __restrict__ ws,
                                                     uint8_t* __restrict__ ebm_run, uint32_t* __restrict__ bad) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const uint32_t ki = k_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ki >= k_hi) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint32_t key = uni(pkeys[ki]);
  uint32_t p = uni(A.key_off[key]);
  const uint32_t e = uni(A.key_off[key + 1]);
  uint8_t* cell = ws + 8192ull * ((uint64_t)(ki - k_lo) * (uint64_t)m);
  WCtr x;
  bool run = false, refused = false;
  for (int j = 0; j < m; j++) {
    w_zero(x);
    if (j <= A.n && seg_find(A.bm, p, e, (uint32_t)j)) {
      const CDesc d = A.desc[p];
      if (d.kind != DK_R) {
        w_materialize(d, A.payload, lds, x);
      } else if (j == 0 && d.card == 65536) {
        w_ones(x);
        run = true;
      } else {
        refused = true;  // the engine refuses the call: the cells are never read
      }
    }
    w_store_bitmap(cell + 8192ull * (uint64_t)j, x);
  }
  if (lane_id() == 0) {
    ebm_run[ki] = run ? 1 : 0;
    if (refused) atomicOr(bad, 1u);
  }
}

// tab: (k_hi - k_lo) x 65,536 u32, zeroed by the caller; n < 2^32
__global__ __launch_bounds__(256) void k_bsis_last(const uint32_t* __restrict__ col, uint64_t n,
                                                   const uint32_t* __restrict__ pkey_off, uint32_t k_lo,
                                                   uint32_t k_hi, uint32_t* __restrict__ tab) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t x = col[i];
    const uint32_t ki = pkey_off[x >> 16];
    if (ki < k_lo || ki >= k_hi) continue;
    uint32_t* t = tab + ((uint64_t)(ki - k_lo) * 65536u + (x & 0xFFFFu));
    const uint32_t v = (uint32_t)i + 1u;
    if (__hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(t, v);
  }
}

// Every wave runs whole rounds of 64 pairs and the loop over the m cells is wave-uniform, so every lane takes
// part in every scan; a lane past the end, outside the pass or overruled by a later pair holds a word index no
// pair has and no bits.  tab: k_bsis_last's.
// ws: (k_hi - k_lo) x m bitmaps, the word index (< 2^31: the engine bounds a pass) of cell j is idx + 2048 j.
__global__ __launch_bounds__(256) void k_bsis_apply(const uint32_t* __restrict__ col, const int32_t* __restrict__ val,
                                                    uint64_t n, const uint32_t* __restrict__ pkey_off, uint32_t k_lo,
                                                    uint32_t k_hi, int m, const uint32_t* __restrict__ tab,
                                                    uint32_t* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (uint64_t)gridDim.x * 4;
  for (uint64_t base = wave * 64; base < n; base += nw * 64) {
    const uint64_t i = base + lane;
    uint32_t idx = 0xFFFFFFFFu, bit = 0;
    uint64_t mask = 0;  // bit j: the pair's column belongs to cell j; bit 0 (ebM) marks a pair that applies
    if (i < n) {
      const uint32_t x = col[i];
      const uint32_t ki = pkey_off[x >> 16];
      if (ki >= k_lo && ki < k_hi && tab[(uint64_t)(ki - k_lo) * 65536u + (x & 0xFFFFu)] == (uint32_t)i + 1u) {
        idx = (ki - k_lo) * (uint32_t)m * 2048u + ((x & 0xFFFFu) >> 5);
        bit = 1u << (x & 31);
        mask = ((uint64_t)(uint32_t)val[i] << 1) | 1u;  // values are below 2^31: cell 32 (slice 31) is cleared
      }
    }
    if (__ballot(mask != 0) == 0) continue;  // wave-uniform: no pair of the round applies in the pass
    const LaneGroup g = lane_group(idx);
    for (int j = 0; j < m; j++) {
      const bool on = (mask >> j) & 1u;
      const uint32_t sbits = g.merge(on ? bit : 0u), cbits = g.merge(on ? 0u : bit);
      if (g.last && idx != 0xFFFFFFFFu) {
        uint32_t* w = ws + ((uint64_t)idx + 2048u * (uint32_t)j);
        const uint32_t cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((cur & sbits) != sbits) atomicOr(w, sbits);
        if (cur & cbits) atomicAnd(w, ~cbits);
      }
    }
  }
}

void launch_bsis_expand(hipStream_t s, BsiAddSide a, const uint16_t* pkeys, uint32_t k_lo, uint32_t k_hi, int m,
                        uint8_t* ws, uint8_t* ebm_run, uint32_t* bad) {
  if (k_hi <= k_lo) return;
  hipLaunchKernelGGL(k_bsis_expand, dim3((k_hi - k_lo + 3) / 4), dim3(256), 0, s, a, pkeys, k_lo, k_hi, m, ws, ebm_run,
                     bad);
}

void launch_bsis_last(hipStream_t s, const uint32_t* col, uint64_t n, const uint32_t* pkey_off, uint32_t k_lo,
                      uint32_t k_hi, uint32_t* tab) {
  if (!n || k_hi <= k_lo) return;
  hipLaunchKernelGGL(k_bsis_last, dim3(grid_for(n, 1024, 4096)), dim3(256), 0, s, col, n, pkey_off, k_lo, k_hi, tab);
}

void launch_bsis_apply(hipStream_t s, const uint32_t* col, const int32_t* val, uint64_t n, const uint32_t* pkey_off,
                       uint32_t k_lo, uint32_t k_hi, int m, const uint32_t* tab, uint32_t* ws) {
  if (!n || k_hi <= k_lo) return;
  hipLaunchKernelGGL(k_bsis_apply, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, s, col, val, n, pkey_off, k_lo,
                     k_hi, m, tab, ws);
}

}  // namespace rbg
