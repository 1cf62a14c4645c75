// A resident bitmap back into its values: RoaringBitmap.toArray() (RB/RoaringBitmap.java:3224), and
// the window of ranks [first, first + count) that BatchIterator.nextBatch / limit walk, ascending and
// unsigned, as u32 or zero-extended i64.
//
// k_to_values: one wave per container, over the containers the window touches.  The batch's rank
// directory (rankdir.hip) places everything, so no wave waits for another:
//   cum[]   the container's first output index; the window's first container by binary search
//   A       a strided copy of the window's values with the key OR-ed in
//   B       16 chunks of 64 words.  A chunk's first rank is a directory entry (dir[8 j]), so chunks
//           outside the window are skipped unread; a lane takes one word of the chunk, the lanes'
//           popcounts are scanned, every lane drops its bits' positions into the wave's LDS stage
//           (at most 4,096 u16) and the wave writes the staged values out in rank order, 64
//           consecutive outputs per store.
//   R       parallel over output positions: a lane finds the run of its rank in the per-run
//           "values before" directory (binary search, as select does), so one run of 65,536 values
//           is 1,024 coalesced stores and not one lane's loop.
#include <algorithm>

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

template <bool OUT64>
__device__ __forceinline__ void put_value(void* out, uint64_t at, uint32_t v) {
  if (OUT64) reinterpret_cast<long long*>(out)[at] = (long long)(uint64_t)v;
  else reinterpret_cast<uint32_t*>(out)[at] = v;
}

// first < cum[n_ctr] and count >= 1 (the host clips the window to the cardinality)
template <bool OUT64>
__global__ __launch_bounds__(256) void k_to_values(const PointArgs a, uint64_t first, uint64_t count,
                                                   void* __restrict__ out) {
  __shared__ __align__(16) uint16_t stage_all[4][4096];
  uint16_t* st = stage_all[threadIdx.x >> 6];
  const int lane = lane_id();
  const uint64_t end = first + count;
  uint32_t lo = 0, hi = a.n_ctr;  // -> the first container whose end prefix is above `first`
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.cum[mid + 1] <= first) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t ci = lo + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); ci < a.n_ctr; ci += nw) {
    const uint64_t base = a.cum[ci];
    if (base >= end) break;
    const CDesc d = a.desc[ci];
    // ranks [r0, r1) of the container go to out[o .. o + r1 - r0)
    const uint32_t r0 = first > base ? (uint32_t)(first - base) : 0u;
    const uint32_t r1 = end - base < d.card ? (uint32_t)(end - base) : d.card;
    const uint64_t o = base + r0 - first;
    const uint32_t top = (uint32_t)d.key << 16;
    const uint8_t* slot = a.payload + d.slot;
    if (d.kind == DK_A) {
      const uint16_t* v = reinterpret_cast<const uint16_t*>(slot);
      for (uint32_t r = r0 + lane; r < r1; r += 64) put_value<OUT64>(out, o + (r - r0), top | v[r]);
    } else if (d.kind == DK_B) {
      const uint16_t* dir = reinterpret_cast<const uint16_t*>(a.aux + a.aux_off[ci]);
      const uint64_t* words = reinterpret_cast<const uint64_t*>(slot);
      for (int j = 0; j < 16; j++) {
        const uint32_t cb = dir[8 * j], ce = j < 15 ? (uint32_t)dir[8 * j + 8] : d.card;
        if (ce <= r0 || cb >= r1 || ce == cb) continue;  // wave-uniform
        uint64_t w = words[64 * j + lane];
        const int pc = __popcll(w);
        int p = dpp_incl_scan(pc) - pc;
        const uint32_t bit0 = (uint32_t)(64 * j + lane) * 64u;
        wsync();  // the previous chunk's readers are done
        while (w) {
          st[p++] = (uint16_t)(bit0 + __builtin_ctzll(w));
          w &= w - 1;
        }
        wsync();
        const uint32_t k0 = cb > r0 ? cb : r0, k1 = ce < r1 ? ce : r1;
        for (uint32_t r = k0 + lane; r < k1; r += 64) put_value<OUT64>(out, o + (r - r0), top | st[r - cb]);
      }
    } else {
      const uint32_t nr = *reinterpret_cast<const uint16_t*>(slot + 2);
      const uint32_t* pairs = reinterpret_cast<const uint32_t*>(slot + 4);
      const uint16_t* dir = reinterpret_cast<const uint16_t*>(a.aux + a.aux_off[ci]);
      for (uint32_t r = r0 + lane; r < r1; r += 64) {
        uint32_t l = 1, h = nr;  // -> the first run with more than r values before it
        while (l < h) {
          const uint32_t mid = (l + h) >> 1;
          if (dir[mid] <= r) l = mid + 1;
          else h = mid;
        }
        put_value<OUT64>(out, o + (r - r0), top | ((pairs[l - 1] & 0xFFFF) + (r - dir[l - 1])));
      }
    }
  }
}

void launch_to_values(hipStream_t s, PointArgs a, uint64_t first, uint64_t count, bool out64, void* out) {
  if (!count || !a.n_ctr) return;
  // the containers of the window are not known to the host: the grid covers every container (up to
  // a resident one), waves past the window leave at once
  const uint64_t by_ctr = ((uint64_t)a.n_ctr + 3) / 4, by_val = (count + 255) / 256;
  const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min(by_ctr, by_val), 256 * 8))), block(256);
  if (out64) hipLaunchKernelGGL(k_to_values<true>, grid, block, 0, s, a, first, count, out);
  else hipLaunchKernelGGL(k_to_values<false>, grid, block, 0, s, a, first, count, out);
}

}  // namespace rbg
