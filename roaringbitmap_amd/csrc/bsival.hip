// Values out of a resident bit-sliced index, the key-major batch [ebM, bA[0..nbits-1], foundSet?]:
//
//   k_bsi_get_values  RoaringBitmapSliceIndex.getValue (BSI/:181-196) for n columns, the loop body of the
//                     buffer package's batchIn / transposeWithCount (BBSI/:551-639).  One lane per query:
//                     the key's segment of the container table (at most 34 containers, ebM first), one
//                     membership test per container (A: binary search, B: bit test, R: binary search over
//                     the run starts), bit input - 1 of the value for every slice that has the column;
//                     -1 where ebM lacks it.  Inputs above nbits (the foundSet) are skipped.
//   k_bsi_pair_cards  per key the cardinality of ebM's container (0: none); its exclusive scan gives every
//                     key's first output position
//   k_bsi_pairs       toPairList() (BBSI/:534-549): one workgroup per key of ebM.  ebM's container becomes
//                     an 8 KiB bitmap in LDS whatever its type, a thread owns 8 of its words, a workgroup
//                     scan of their popcounts places the thread's columns.  The values come a word (32
//                     columns) at a time: the same word of every slice container of the key (B: one load,
//                     A: a binary search and the values inside the word, R: the runs that overlap it; the
//                     descriptors staged in LDS once per key) is spread over 32 value registers.
#include <algorithm>

#include "bsival.hpp"

namespace rbg {

// membership of the low 16 bits `low` in a container
__device__ __forceinline__ bool bsiv_has(const CDesc& d, const uint8_t* __restrict__ payload, uint32_t low) {
  const uint8_t* slot = payload + d.slot;
  if (d.kind == DK_B) return (reinterpret_cast<const uint32_t*>(slot)[low >> 5] >> (low & 31)) & 1u;
  if (d.kind == DK_A) {
    const uint16_t* v = reinterpret_cast<const uint16_t*>(slot);
    uint32_t lo = 0, hi = d.card;  // -> the first value >= low
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (v[mid] < low) lo = mid + 1;
      else hi = mid;
    }
    return lo < d.card && v[lo] == low;
  }
  const uint32_t nr = *reinterpret_cast<const uint16_t*>(slot + 2);
  const uint32_t* runs = reinterpret_cast<const uint32_t*>(slot + 4);  // start | (length - 1) << 16
  uint32_t lo = 0, hi = nr;  // -> the first run that starts above low
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((runs[mid] & 0xFFFFu) <= low) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return false;
  const uint32_t r = runs[lo - 1];
  return low - (r & 0xFFFFu) <= (r >> 16);
}

__global__ __launch_bounds__(256) void k_bsi_get_values(const BsiValArgs a, const uint32_t* __restrict__ q, uint64_t n,
                                                        long long* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t x = q[i], low = x & 0xFFFFu;
    const uint32_t c0 = a.key_off[x >> 16], c1 = a.key_off[(x >> 16) + 1];
    long long v = -1;
    // (key, input) order: ebM's container, if the key has one, is the segment's first
    if (c0 < c1 && a.bm[c0] == 0 && bsiv_has(a.desc[c0], a.payload, low)) {
      v = 0;
      for (uint32_t c = c0 + 1; c < c1; c++) {
        const uint32_t in = a.bm[c];
        if (in > (uint32_t)a.nbits) break;  // the foundSet
        if (bsiv_has(a.desc[c], a.payload, low)) v |= 1ll << (in - 1);
      }
    }
    out[i] = v;
  }
}

__global__ __launch_bounds__(256) void k_bsi_pair_cards(const BsiValArgs a, uint64_t* __restrict__ cards) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;  // 256 workgroups: every key
  const uint32_t c0 = a.key_off[k], c1 = a.key_off[k + 1];
  cards[k] = c0 < c1 && a.bm[c0] == 0 ? (uint64_t)a.desc[c0].card : 0ull;
}

template <bool C64, bool V64>
__global__ __launch_bounds__(256) void k_bsi_pairs(const BsiValArgs a, const uint64_t* __restrict__ base,
                                                   void* __restrict__ cols, void* __restrict__ vals) {
  __shared__ __align__(16) uint32_t bmp[2048];
  __shared__ CDesc sd[kBsiMaxInputs];
  __shared__ uint32_t sin[kBsiMaxInputs];
  __shared__ int wtot[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t k = blockIdx.x; k < 65536u; k += gridDim.x) {
    const uint32_t c0 = a.key_off[k], c1 = a.key_off[k + 1];
    if (c0 == c1 || a.bm[c0] != 0) continue;  // uniform over the workgroup
    __syncthreads();                         // the previous key's readers are done
    const CDesc e = a.desc[c0];
    const uint32_t ns = min(c1 - c0 - 1, (uint32_t)kBsiMaxInputs);
    if ((uint32_t)t < ns) {
      sd[t] = a.desc[c0 + 1 + t];
      sin[t] = a.bm[c0 + 1 + t];
    }
    bsiv_stage_bitmap(e, a.payload, bmp, t);
    __syncthreads();
    uint32_t mine[8];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      mine[j] = bmp[8 * t + j];
      cnt += __popc(mine[j]);
    }
    const int sc = dpp_incl_scan(cnt);
    if (lane == 63) wtot[w] = sc;
    __syncthreads();
    uint64_t o = base[k] + (uint64_t)(sc - cnt);
    for (int i = 0; i < w; i++) o += (uint64_t)wtot[i];
    const uint32_t top = k << 16;
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
      const uint32_t word = mine[j];
      if (!word) continue;
      // the values of the word's 32 columns, a slice at a time: one word of the slice's container per
      // slice instead of one membership test per column (v[] is indexed by unrolled loops only: registers)
      uint32_t v[32];
#pragma unroll
      for (int b = 0; b < 32; b++) v[b] = 0;
      for (uint32_t s = 0; s < ns; s++) {
        if (sin[s] > (uint32_t)a.nbits) break;  // the foundSet
        const uint32_t sw = bsiv_word(sd[s], a.payload, (uint32_t)(8 * t + j)) & word;
        if (!sw) continue;
        const uint32_t sh = sin[s] - 1;
#pragma unroll
        for (int b = 0; b < 32; b++) v[b] |= ((sw >> b) & 1u) << sh;
      }
      const uint32_t low0 = (uint32_t)(32 * (8 * t + j));
#pragma unroll
      for (int b = 0; b < 32; b++) {
        if ((word >> b) & 1u) {
          if (C64) reinterpret_cast<long long*>(cols)[o] = (long long)(uint64_t)(top | (low0 + b));
          else reinterpret_cast<uint32_t*>(cols)[o] = top | (low0 + b);
          if (V64) reinterpret_cast<long long*>(vals)[o] = (long long)(uint64_t)v[b];
          else reinterpret_cast<int32_t*>(vals)[o] = (int32_t)v[b];
          o++;
        }
      }
    }
  }
}

void launch_bsi_get_values(hipStream_t s, BsiValArgs a, const uint32_t* q, uint64_t n, long long* out) {
  if (!n) return;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 256 * 32));
  hipLaunchKernelGGL(k_bsi_get_values, dim3(grid), dim3(256), 0, s, a, q, n, out);
}

void launch_bsi_pair_cards(hipStream_t s, BsiValArgs a, uint64_t* cards) {
  hipLaunchKernelGGL(k_bsi_pair_cards, dim3(256), dim3(256), 0, s, a, cards);
}

void launch_bsi_pairs(hipStream_t s, BsiValArgs a, const uint64_t* base, bool cols64, bool vals64, void* cols,
                      void* vals) {
  const dim3 grid(256 * 8), block(256);
  if (cols64 && vals64) hipLaunchKernelGGL((k_bsi_pairs<true, true>), grid, block, 0, s, a, base, cols, vals);
  else if (cols64) hipLaunchKernelGGL((k_bsi_pairs<true, false>), grid, block, 0, s, a, base, cols, vals);
  else if (vals64) hipLaunchKernelGGL((k_bsi_pairs<false, true>), grid, block, 0, s, a, base, cols, vals);
  else hipLaunchKernelGGL((k_bsi_pairs<false, false>), grid, block, 0, s, a, base, cols, vals);
}

}  // namespace rbg
