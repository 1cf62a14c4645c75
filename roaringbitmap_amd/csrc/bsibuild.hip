// A bit-sliced index from (column, value) pairs, on the device: RoaringBitmapSliceIndex.setValue for
// every pair (BSI/:299-347), optionally followed by runOptimize() (BSI/:141-150), as the key-major
// slot-aligned batch [ebM, bA[0], ..., bA[nbits - 1]] that rbg_ctx_load of the host builder's bitmaps
// gives.  The n pairs (u32 column, i32 value >= 0, any order, columns distinct) are never sorted:
//
//   k_bsib_minmax   min and max of the values (one atomic pair per wave)
//   k_bld_keys / k_bld_key_scan (build.hip) on the columns: the K present keys and the CSR key -> key index
//   k_bsib_scatter  a zeroed workspace holds, for every key index of the pass, m = nbits + 1 bitmaps of
//                   8 KiB: input 0 (ebM), then the slices.  Every pair ORs its column's bit into input 0
//                   and into input 1 + i for every set bit i of its value: one atomic per group of
//                   neighbouring lanes that hit the same 32-bit word (wave.hpp: LaneGroup, computed once per
//                   round since the inputs of a pair share the word), after reading the word.
//   k_bsib_plan     one wave per (key index, input): cardinality (and run count), the container's type
//                   and slot size; an empty bitmap is no container.  A wave keeps one input, so the
//                   per-input totals (containers, cardinality, serialized bytes, run containers) cost
//                   one set of atomics per wave.
//   (one scan of [container count << 40 | slot bytes] over the (key index, input) cells: key-major order)
//   k_bsib_write    one wave per non-empty cell: the slot (wave.hpp: w_write_slot), the CDesc, keys[],
//                   bm[] = input
//   k_bsib_key_off  the batch's key CSR over its containers
//
// (bsiadd.hip fills the same workspace with the sum of two indexes and shares the plan, scan, write and key
// CSR stages; its only extension is the plan's ebm_run flag.  bsiin.hip fills it with one cell per key, the
// result of an IN-list query, and passes its full-container flag through the same argument.)
//
// Types: by_card, and with run_optimize runopt_kind (device.hpp).
//
// The workspace is K x m x 8 KiB, so the engine walks the key indices in passes [k_lo, k_hi) under a byte
// budget; a pass scatters only the pairs whose key index it covers.
#include <algorithm>
#include <climits>

#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

// mm[0] = min, mm[1] = max (set to INT_MAX / INT_MIN by the caller)
__global__ __launch_bounds__(256) void k_bsib_minmax(const int32_t* __restrict__ v, uint64_t n, int* __restrict__ mm) {
  int lo = INT_MAX, hi = INT_MIN;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int x = v[i];
    lo = min(lo, x);
    hi = max(hi, x);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = min(lo, __shfl_xor(lo, d, 64));
    hi = max(hi, __shfl_xor(hi, d, 64));
  }
  if ((threadIdx.x & 63) == 0 && lo <= hi) {
    atomicMin(&mm[0], lo);
    atomicMax(&mm[1], hi);
  }
}

// Every wave runs whole rounds of 64 pairs and the loop over the m inputs is wave-uniform, so every lane
// takes part in every scan; a lane past the end or outside the pass holds a word index no pair has and no
// bits.  ws: (k_hi - k_lo) x m bitmaps; the word index (< 2^31: the engine bounds a pass) of input j is
// idx + 2048 j.
__global__ __launch_bounds__(256) void k_bsib_scatter(const uint32_t* __restrict__ col, const int32_t* __restrict__ val,
                                                      uint64_t n, const uint32_t* __restrict__ pkey_off, uint32_t k_lo,
                                                      uint32_t k_hi, int m, uint32_t* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (uint64_t)gridDim.x * 4;
  for (uint64_t base = wave * 64; base < n; base += nw * 64) {
    const uint64_t i = base + lane;
    uint32_t idx = 0xFFFFFFFFu, bit = 0, mask = 0;
    if (i < n) {
      const uint32_t x = col[i];
      const uint32_t ki = pkey_off[x >> 16];
      if (ki >= k_lo && ki < k_hi) {
        idx = (ki - k_lo) * (uint32_t)m * 2048u + ((x & 0xFFFFu) >> 5);
        bit = 1u << (x & 31);
        mask = ((uint32_t)val[i] << 1) | 1u;  // bit j: the pair belongs to input j (values are below 2^31)
      }
    }
    if (__ballot(mask != 0) == 0) continue;  // wave-uniform: no pair of the round belongs to the pass
    const LaneGroup g = lane_group(idx);
    for (int j = 0; j < m; j++) {
      const uint32_t bits = g.merge((mask >> j) & 1u ? bit : 0u);
      if (bits && g.last) {
        uint32_t* w = ws + ((uint64_t)idx + 2048u * (uint32_t)j);
        const uint32_t cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((cur & bits) != bits) atomicOr(w, bits);
      }
    }
  }
}

struct BsibInfo {
  uint32_t card;  // 0: no container
  uint16_t nruns;
  uint8_t kind;
  uint8_t pad;
};
static_assert(sizeof(BsibInfo) == kBsibInfoBytes, "the engine sizes the plan's table by kBsibInfoBytes");

// Cell (ki, j) of the pass: its bitmap at ws + 8192 ((ki - k_lo) m + j), its info / size entry at ki m + j.
// Wave w of the first R m waves takes input w % m and the key indices k_lo + w / m + R r.
// per (u64, zeroed by the caller): per input {containers, cardinality, serialized payload bytes, run
// containers}; kinds: containers of kind A / B / R
__global__ __launch_bounds__(256) void k_bsib_plan(const uint8_t* __restrict__ ws, uint32_t k_lo, uint32_t k_hi, int m,
                                                   uint32_t R, int run_optimize, BsibInfo* __restrict__ info,
                                                   uint64_t* __restrict__ size, unsigned long long* __restrict__ per,
                                                   unsigned long long* __restrict__ kinds,
                                                   const uint8_t* __restrict__ ebm_run) {
  const int lane = lane_id();
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wave >= R * (uint32_t)m) return;
  const uint32_t j = wave % (uint32_t)m;
  unsigned long long cnt[3] = {0, 0, 0}, ser = 0, cards = 0;
  for (uint32_t ki = k_lo + wave / (uint32_t)m; ki < k_hi; ki += R) {
    const uint64_t cell = (uint64_t)ki * m + j;
    WCtr x;
    w_load_bitmap(ws + 8192ull * ((uint64_t)(ki - k_lo) * m + j), x);
    const int card = w_card(x);
    if (card == 0) {  // wave-uniform
      if (lane == 0) {
        info[cell] = BsibInfo{0, 0, 0, 0};
        size[cell] = 0;
      }
      continue;
    }
    int kind = by_card(card), nruns = 0;
    if (run_optimize) {
      nruns = w_runs(x);
      kind = runopt_kind(kind, card, nruns);
    }
    if (ebm_run && j == 0 && ebm_run[ki]) {  // the full ebM' of bsiadd.hip (wave-uniform)
      kind = DK_R;
      nruns = 1;
    }
    const uint32_t len = ser_len_of(kind, (uint32_t)card, (uint32_t)nruns);
    if (lane == 0) {
      info[cell] = BsibInfo{(uint32_t)card, (uint16_t)nruns, (uint8_t)kind, 0};
      size[cell] = (1ull << kBsibCountShift) | slot_bytes(kind, len);
    }
    cnt[kind]++;
    ser += len;
    cards += (unsigned long long)card;
  }
  if (lane == 0) {
    const unsigned long long nc = cnt[0] + cnt[1] + cnt[2];
    if (nc) {
      atomicAdd(&per[4 * j + 0], nc);
      atomicAdd(&per[4 * j + 1], cards);
      atomicAdd(&per[4 * j + 2], ser);
      if (cnt[2]) atomicAdd(&per[4 * j + 3], cnt[2]);
      for (int k = 0; k < 3; k++)
        if (cnt[k]) atomicAdd(&kinds[k], cnt[k]);
    }
  }
}

// scan: the exclusive scan of size[] (container index << 40 | payload offset)
__global__ __launch_bounds__(256, 4) void k_bsib_write(const uint8_t* __restrict__ ws, uint32_t k_lo, uint32_t k_hi,
                                                       int m, const BsibInfo* __restrict__ info,
                                                       const uint64_t* __restrict__ scan,
                                                       const uint16_t* __restrict__ pkeys, CDesc* __restrict__ desc,
                                                       uint16_t* __restrict__ keys, uint32_t* __restrict__ bm,
                                                       uint8_t* __restrict__ payload) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4, cells = (uint64_t)(k_hi - k_lo) * m;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < cells; i += nw) {
    const uint64_t cell = (uint64_t)k_lo * m + i;
    const BsibInfo in = info[cell];
    if (in.card == 0) continue;  // wave-uniform
    const uint64_t sc = scan[cell];
    const uint64_t o = sc & ((1ull << kBsibCountShift) - 1), ci = sc >> kBsibCountShift;
    const int kind = in.kind;
    WCtr x;
    w_load_bitmap(ws + 8192ull * i, x);
    w_write_slot(kind, x, (int)in.card, lds, payload + o);
    if (lane == 0) {
      const uint16_t key = pkeys[k_lo + i / (uint64_t)m];
      desc[ci] = CDesc{o, in.card, key, (uint8_t)kind, 0};
      keys[ci] = key;
      bm[ci] = (uint32_t)(i % (uint64_t)m);
    }
  }
}

// key_off[k] = containers before key k: the container index of key k's first cell (pkey_off[k] is the
// index of the first present key >= k); scan[K m] holds the totals
__global__ __launch_bounds__(256) void k_bsib_key_off(const uint32_t* __restrict__ pkey_off,
                                                      const uint64_t* __restrict__ scan, int m,
                                                      uint32_t* __restrict__ key_off) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k > 65536) return;
  key_off[k] = (uint32_t)(scan[(uint64_t)pkey_off[k] * m] >> kBsibCountShift);
}

void launch_bsib_minmax(hipStream_t s, const int32_t* v, uint64_t n, int* mm) {
  if (!n) return;
  hipLaunchKernelGGL(k_bsib_minmax, dim3(grid_for(n, 1024, 2048)), dim3(256), 0, s, v, n, mm);
}

void launch_bsib_scatter(hipStream_t s, const uint32_t* col, const int32_t* val, uint64_t n, const uint32_t* pkey_off,
                         uint32_t k_lo, uint32_t k_hi, int m, uint32_t* ws) {
  if (!n || k_hi <= k_lo) return;
  const dim3 grid(grid_for(n, 256, 256 * 16)), block(256);
  hipLaunchKernelGGL(k_bsib_scatter, grid, block, 0, s, col, val, n, pkey_off, k_lo, k_hi, m, ws);
}

void launch_bsib_plan(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int m, int run_optimize,
                      void* info, uint64_t* size, unsigned long long* per, unsigned long long* kinds,
                      const uint8_t* ebm_run) {
  if (k_hi <= k_lo) return;
  const uint32_t R = std::max<uint32_t>(1, std::min<uint32_t>(k_hi - k_lo, 16384u / (uint32_t)m));
  hipLaunchKernelGGL(k_bsib_plan, dim3((R * (uint32_t)m + 3) / 4), dim3(256), 0, s, ws, k_lo, k_hi, m, R, run_optimize,
                     reinterpret_cast<BsibInfo*>(info), size, per, kinds, ebm_run);
}

void launch_bsib_write(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int m, const void* info,
                       const uint64_t* scan, const uint16_t* pkeys, CDesc* desc, uint16_t* keys, uint32_t* bm,
                       uint8_t* payload) {
  if (k_hi <= k_lo) return;
  hipLaunchKernelGGL(k_bsib_write, dim3(grid_for((uint64_t)(k_hi - k_lo) * m, 4, 4096)), dim3(256), 0, s, ws, k_lo,
                     k_hi, m, reinterpret_cast<const BsibInfo*>(info), scan, pkeys, desc, keys, bm, payload);
}

void launch_bsib_key_off(hipStream_t s, const uint32_t* pkey_off, const uint64_t* scan, int m, uint32_t* key_off) {
  hipLaunchKernelGGL(k_bsib_key_off, dim3(257), dim3(256), 0, s, pkey_off, scan, m, key_off);
}

}  // namespace rbg
