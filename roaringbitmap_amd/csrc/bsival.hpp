// Pieces of bsival.hip that bsiin.hip shares: a container as an 8 KiB bitmap in LDS, and one 32-column word
// of a container whatever its type.
#pragma once

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

// word w (32 values, 0 <= w < 2048) of a container's bitmap
__device__ __forceinline__ uint32_t bsiv_word(const CDesc& d, const uint8_t* __restrict__ payload, uint32_t w) {
  const uint8_t* slot = payload + d.slot;
  if (d.kind == DK_B) return reinterpret_cast<const uint32_t*>(slot)[w];
  const uint32_t base = 32u * w, top = base + 31u;
  uint32_t out = 0;
  if (d.kind == DK_A) {
    const uint16_t* v = reinterpret_cast<const uint16_t*>(slot);
    uint32_t lo = 0, hi = d.card;  // -> the first value >= base
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (v[mid] < base) lo = mid + 1;
      else hi = mid;
    }
    for (; lo < d.card && v[lo] <= top; lo++) out |= 1u << (v[lo] & 31);
    return out;
  }
  const uint32_t nr = *reinterpret_cast<const uint16_t*>(slot + 2);
  const uint32_t* runs = reinterpret_cast<const uint32_t*>(slot + 4);  // start | (length - 1) << 16
  uint32_t lo = 0, hi = nr;  // -> the first run that starts above base
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((runs[mid] & 0xFFFFu) <= base) lo = mid + 1;
    else hi = mid;
  }
  for (uint32_t i = lo ? lo - 1 : 0; i < nr; i++) {  // the run that may cover base, then those that start inside
    const uint32_t s = runs[i] & 0xFFFFu, e = s + (runs[i] >> 16);
    if (s > top) break;
    if (e < base) continue;
    const uint32_t a = s > base ? s - base : 0u, b = e < top ? e - base : 31u;
    out |= (~0u << a) & (~0u >> (31u - b));
  }
  return out;
}

// Container e as a bitmap in bmp[2048] (LDS), by a workgroup of 256 threads (t = threadIdx.x; e is uniform
// over the workgroup).  The caller's __syncthreads() follows before bmp is read.
__device__ __forceinline__ void bsiv_stage_bitmap(const CDesc& e, const uint8_t* __restrict__ payload, uint32_t* bmp,
                                                  int t) {
  const uint8_t* slot = payload + e.slot;
  if (e.kind == DK_B) {
    const uint4* src = reinterpret_cast<const uint4*>(slot);
    reinterpret_cast<uint4*>(bmp)[t] = src[t];
    reinterpret_cast<uint4*>(bmp)[256 + t] = src[256 + t];
    return;
  }
  for (int i = t; i < 2048; i += 256) bmp[i] = 0;
  __syncthreads();
  if (e.kind == DK_A) {
    const uint16_t* v = reinterpret_cast<const uint16_t*>(slot);
    for (uint32_t i = t; i < e.card; i += 256) atomicOr(&bmp[v[i] >> 5], 1u << (v[i] & 31));
  } else {
    const uint32_t nr = *reinterpret_cast<const uint16_t*>(slot + 2);
    const uint32_t* runs = reinterpret_cast<const uint32_t*>(slot + 4);
    for (uint32_t i = t; i < nr; i += 256) {
      const uint32_t s = runs[i] & 0xFFFFu, last = s + (runs[i] >> 16);  // last <= 65535
      const uint32_t w0 = s >> 5, w1 = last >> 5;
      const uint32_t m0 = ~0u << (s & 31), m1 = ~0u >> (31 - (last & 31));
      if (w0 == w1) {
        atomicOr(&bmp[w0], m0 & m1);
      } else {
        atomicOr(&bmp[w0], m0);
        for (uint32_t x = w0 + 1; x < w1; x++) bmp[x] = ~0u;  // words inside one run: no other writer
        atomicOr(&bmp[w1], m1);
      }
    }
  }
}

}  // namespace rbg
