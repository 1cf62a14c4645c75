// Point queries against one resident bitmap: rank, select, contains, next / previous value
// (RB/RoaringBitmap.java:1693, 2574-2624, 2820-2883), many independent queries per launch.
//
// The rank directory of a batch (built once, on the device, by k_rd_sizes -> two scans -> k_rd_fill):
//   cum[n_ctr + 1]   exclusive prefix of CDesc::card in 64 bits (FastRankRoaringBitmap's
//                    highToCumulatedCardinality, RB/FastRankRoaringBitmap.java); cum[n_ctr] = cardinality
//   aux_off[n_ctr+1] byte offset of each container's directory in the aux arena
//   aux              B: 128 u16, the set bits before each block of 8 words (256 B; the last entry is
//                       at most 127 * 512 = 65,024)
//                    R: one u16 per run, the values before it (at most 65,535), padded to 16 B
//                    A: nothing
// so that no query reads more of a container than a binary search's probes or one 64 B block.
//
// k_point<OP>: one lane per query.  Queries are scattered, so every load is a dependent gather of its
// own cache line; the kernel keeps its registers low (full occupancy hides the latency) and has no
// loop over a container's payload.
#include <algorithm>

#include "kernels.hpp"

namespace rbg {

__device__ __forceinline__ uint32_t round16u(uint32_t x) { return (x + 15u) & ~15u; }

// cum[i] = card, aux_off[i] = directory bytes of container i (both scanned in place afterwards)
__global__ __launch_bounds__(256) void k_rd_sizes(const CDesc* __restrict__ desc, const uint8_t* __restrict__ payload,
                                                  uint64_t n, uint64_t* __restrict__ cum,
                                                  uint64_t* __restrict__ aux_off) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CDesc d = desc[i];
  uint32_t sz = 0;
  if (d.kind == DK_B) sz = 256;
  else if (d.kind == DK_R) sz = round16u(2u * *reinterpret_cast<const uint16_t*>(payload + d.slot + 2));
  cum[i] = d.card;
  aux_off[i] = sz;
}

// one wave per container
__global__ __launch_bounds__(256) void k_rd_fill(const CDesc* __restrict__ desc, const uint8_t* __restrict__ payload,
                                                 uint64_t n, const uint64_t* __restrict__ aux_off,
                                                 uint8_t* __restrict__ aux) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nw) {
    const CDesc d = desc[i];
    uint16_t* dir = reinterpret_cast<uint16_t*>(aux + aux_off[i]);
    if (d.kind == DK_B) {  // lane l: blocks l and 64 + l
      const uint4* p = reinterpret_cast<const uint4*>(payload + d.slot);
      int c0 = 0, c1 = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint4 a = p[4 * lane + j], b = p[4 * (64 + lane) + j];
        c0 += __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w);
        c1 += __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
      }
      const int s0 = dpp_incl_scan(c0), s1 = dpp_incl_scan(c1);
      const int t0 = lane63(s0);
      dir[lane] = (uint16_t)(s0 - c0);
      dir[64 + lane] = (uint16_t)(t0 + s1 - c1);
    } else if (d.kind == DK_R) {
      const int nr = *reinterpret_cast<const uint16_t*>(payload + d.slot + 2);
      const uint32_t* pairs = reinterpret_cast<const uint32_t*>(payload + d.slot + 4);
      int carry = 0;
      for (int base = 0; base < nr; base += 64) {  // nr is wave-uniform: every lane runs every scan
        const int r = base + lane;
        const int len = r < nr ? (int)(pairs[r] >> 16) + 1 : 0;
        const int s = dpp_incl_scan(len);
        if (r < nr) dir[r] = (uint16_t)(carry + s - len);
        carry += lane63(s);
      }
    }
  }
}

struct PtHit {
  uint32_t rank;  // values of the container <= low
  bool in;        // low is one of them
};

__device__ __forceinline__ PtHit rank_in(const PointArgs& a, uint32_t ci, const CDesc d, uint32_t low) {
  const uint8_t* slot = a.payload + d.slot;
  if (d.kind == DK_A) {
    const uint16_t* v = reinterpret_cast<const uint16_t*>(slot);
    uint32_t lo = 0, hi = d.card;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (v[mid] <= low) lo = mid + 1;
      else hi = mid;
    }
    return PtHit{lo, lo > 0 && v[lo - 1] == low};
  }
  if (d.kind == DK_B) {
    const uint32_t wi = low >> 6, bit = low & 63;
    const uint64_t mask = ~0ull >> (63 - bit);
    const uint32_t blk = wi >> 3, k = wi & 7;
    const uint16_t* dir = reinterpret_cast<const uint16_t*>(a.aux + a.aux_off[ci]);
    const uint4* p = reinterpret_cast<const uint4*>(slot) + 4 * blk;
    uint32_t r = dir[blk];
    uint64_t cur = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint4 q = p[j];
      uint64_t x0, x1;
      u4_to_words(q, x0, x1);
      const uint32_t i0 = 2 * j, i1 = 2 * j + 1;
      r += (uint32_t)__popcll(x0 & (i0 < k ? ~0ull : (i0 == k ? mask : 0ull)));
      r += (uint32_t)__popcll(x1 & (i1 < k ? ~0ull : (i1 == k ? mask : 0ull)));
      cur = i0 == k ? x0 : cur;
      cur = i1 == k ? x1 : cur;
    }
    return PtHit{r, ((cur >> bit) & 1) != 0};
  }
  const uint32_t nr = *reinterpret_cast<const uint16_t*>(slot + 2);
  const uint32_t* pairs = reinterpret_cast<const uint32_t*>(slot + 4);
  uint32_t lo = 0, hi = nr;  // -> runs whose start <= low
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((pairs[mid] & 0xFFFF) <= low) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return PtHit{0, false};
  const uint16_t* dir = reinterpret_cast<const uint16_t*>(a.aux + a.aux_off[ci]);
  const uint32_t p = pairs[lo - 1];
  const uint32_t off = low - (p & 0xFFFF), len = p >> 16;
  return PtHit{(uint32_t)dir[lo - 1] + min(off, len) + 1, off <= len};
}

// the k-th value (0-based, k < card) of container ci
__device__ __forceinline__ uint32_t select_in(const PointArgs& a, uint32_t ci, const CDesc d, uint32_t k) {
  const uint8_t* slot = a.payload + d.slot;
  if (d.kind == DK_A) return reinterpret_cast<const uint16_t*>(slot)[k];
  const uint16_t* dir = reinterpret_cast<const uint16_t*>(a.aux + a.aux_off[ci]);
  if (d.kind == DK_B) {
    uint32_t lo = 1, hi = 128;  // -> the first block whose entry is above k; the one before holds the bit
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (dir[mid] <= k) lo = mid + 1;
      else hi = mid;
    }
    const uint32_t blk = lo - 1;
    k -= dir[blk];
    const uint4* p = reinterpret_cast<const uint4*>(slot) + 4 * blk;
    uint64_t word = 0;
    uint32_t wi = 0;
    bool found = false;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint4 q = p[j];
      uint64_t x[2];
      u4_to_words(q, x[0], x[1]);
#pragma unroll
      for (uint32_t h = 0; h < 2; h++) {
        const uint32_t c = (uint32_t)__popcll(x[h]);
        const bool here = !found && k < c;
        word = here ? x[h] : word;
        wi = here ? 2 * j + h : wi;
        k -= (!found && !here) ? c : 0;
        found = found || here;
      }
    }
    uint32_t pos = 0;  // the k-th set bit of word: halve the window six times
#pragma unroll
    for (uint32_t sh = 32; sh >= 1; sh >>= 1) {
      const uint32_t c = (uint32_t)__popcll(word & ((1ull << sh) - 1));
      const bool up = k >= c;
      k -= up ? c : 0;
      word = up ? word >> sh : word;
      pos += up ? sh : 0;
    }
    return (blk * 8 + wi) * 64 + pos;
  }
  const uint32_t nr = *reinterpret_cast<const uint16_t*>(slot + 2);
  const uint32_t* pairs = reinterpret_cast<const uint32_t*>(slot + 4);
  uint32_t lo = 1, hi = nr;  // -> the first run with more than k values before it
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (dir[mid] <= k) lo = mid + 1;
    else hi = mid;
  }
  return (pairs[lo - 1] & 0xFFFF) + (k - dir[lo - 1]);
}

__device__ __forceinline__ long long value_of(const CDesc d, uint32_t low) {
  return (long long)(((uint32_t)d.key << 16) | low);
}

template <int OP>
__global__ __launch_bounds__(256) void k_point(const PointArgs a, const uint32_t* __restrict__ q, uint64_t n,
                                               long long* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t x = q[i];
    long long res;
    if (OP == PT_SELECT) {
      // RB/RoaringBitmap.java:2820-2835 with j unsigned; -1 where the reference throws
      const uint64_t total = a.cum[a.n_ctr];
      if (x >= total) {
        res = -1;
      } else {
        uint32_t lo = 0, hi = a.n_ctr;  // -> the first container whose end prefix is above x
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (a.cum[mid + 1] <= x) lo = mid + 1;
          else hi = mid;
        }
        const CDesc d = a.desc[lo];
        res = value_of(d, select_in(a, lo, d, (uint32_t)(x - a.cum[lo])));
      }
    } else {
      // the key's container through the key CSR: key_off[key] is also the first container of a larger
      // key when the key is absent
      const uint32_t key = x >> 16, low = x & 0xFFFF;
      const uint32_t ci = a.key_off[key];
      const bool present = a.key_off[key + 1] != ci;
      const uint64_t base = a.cum[ci];
      CDesc d = {};
      PtHit h{0, false};
      if (present) {
        d = a.desc[ci];
        h = rank_in(a, ci, d, low);
      }
      const uint64_t r = base + h.rank;  // rankLong(x), RB/RoaringBitmap.java:2574-2592
      if (OP == PT_RANK) {
        res = (long long)r;
      } else if (OP == PT_CONTAINS) {
        res = h.in ? 1 : 0;
      } else if (h.in) {
        res = (long long)x;
      } else if (OP == PT_NEXT) {  // select(rankLong(x)): in this container, or the next one's first value
        if (r == a.cum[a.n_ctr]) {
          res = -1;
        } else if (present && h.rank < d.card) {
          res = value_of(d, select_in(a, ci, d, h.rank));
        } else {
          const uint32_t cj = present ? ci + 1 : ci;
          const CDesc e = a.desc[cj];
          res = value_of(e, select_in(a, cj, e, 0));
        }
      } else {  // PT_PREV: select(rankLong(x) - 1): in this container, or the one before's last value
        if (r == 0) {
          res = -1;
        } else if (present && h.rank > 0) {
          res = value_of(d, select_in(a, ci, d, h.rank - 1));
        } else {
          const uint32_t cj = ci - 1;
          const CDesc e = a.desc[cj];
          res = value_of(e, select_in(a, cj, e, e.card - 1));
        }
      }
    }
    out[i] = res;
  }
}

void launch_rd_sizes(hipStream_t s, const CDesc* desc, const uint8_t* payload, uint64_t n, uint64_t* cum,
                     uint64_t* aux_off) {
  if (!n) return;
  hipLaunchKernelGGL(k_rd_sizes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, desc, payload, n, cum, aux_off);
}

void launch_rd_fill(hipStream_t s, const CDesc* desc, const uint8_t* payload, uint64_t n, const uint64_t* aux_off,
                    uint8_t* aux) {
  if (!n) return;
  const uint64_t grid = std::min<uint64_t>((n + 3) / 4, 256 * 8);
  hipLaunchKernelGGL(k_rd_fill, dim3((unsigned)grid), dim3(256), 0, s, desc, payload, n, aux_off, aux);
}

void launch_point(hipStream_t s, int op, PointArgs a, const uint32_t* q, uint64_t n, long long* out) {
  if (!n) return;
  const dim3 grid((unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 8)), block(256);
  switch (op) {
    case PT_RANK: hipLaunchKernelGGL(k_point<PT_RANK>, grid, block, 0, s, a, q, n, out); break;
    case PT_SELECT: hipLaunchKernelGGL(k_point<PT_SELECT>, grid, block, 0, s, a, q, n, out); break;
    case PT_CONTAINS: hipLaunchKernelGGL(k_point<PT_CONTAINS>, grid, block, 0, s, a, q, n, out); break;
    case PT_NEXT: hipLaunchKernelGGL(k_point<PT_NEXT>, grid, block, 0, s, a, q, n, out); break;
    default: hipLaunchKernelGGL(k_point<PT_PREV>, grid, block, 0, s, a, q, n, out); break;
  }
}

}  // namespace rbg
