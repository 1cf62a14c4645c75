// A bitmap from values, on the device: RoaringBitmap.add(int...) / addN / bitmapOf
// (RB/RoaringBitmap.java:483-570), optionally followed by runOptimize() (:2764-2774), as a
// single-bitmap key-major slot-aligned batch -- what rbg_ctx_load of the host builder's bytes
// (format.cpp: build_from_values) gives.  The n values (u32, any order, duplicates allowed) are
// never sorted:
//
//   k_bld_keys     marks flag[v >> 16] (plain byte stores; every writer stores the same 1)
//   k_bld_key_scan scans the 65,536 flags (256 workgroups of 256 keys): keys[], the key CSR
//                  key_off[65537] (key_off[k] is also key k's container index), the container count C
//   k_bld_scatter  ORs every value's bit into its container's 8 KiB bitmap of a zeroed workspace
//                  (C bitmaps), one atomic per group of neighbouring lanes that hit the same
//                  32-bit word (wave.hpp: LaneGroup)
//   k_bld_plan     one wave per container: cardinality (and run count) from registers, the
//                  container's type and slot size, the batch totals
//   (scan of the slot sizes)
//   k_bld_write    one wave per container: the slot (wave.hpp: w_write_slot), the CDesc, keys[],
//                  bm[] = 0
//
// Types (format.cpp: make_ctr with kind_hint -1): by_card, and with run_optimize runopt_kind
// (device.hpp).
#include "build.hpp"

namespace rbg {

__global__ __launch_bounds__(256) void k_bld_keys(const uint32_t* __restrict__ v, uint64_t n,
                                                  uint8_t* __restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) flag[v[i] >> 16] = 1;
}

// 256 workgroups of 256 keys: workgroup b counts the flags of the b chunks before its own (thread t
// sums chunk t, 256 bytes), then scans its own 256 flags
__global__ __launch_bounds__(256) void k_bld_key_scan(const uint8_t* __restrict__ flag, uint16_t* __restrict__ keys,
                                                      uint32_t* __restrict__ key_off,
                                                      unsigned long long* __restrict__ n_ctr) {
  __shared__ int wtot[8];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.x;
  int c = 0;
  if (t < b) {
    const uint4* f4 = reinterpret_cast<const uint4*>(flag) + 16 * t;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint4 f = f4[j];
      c += __popc(f.x) + __popc(f.y) + __popc(f.z) + __popc(f.w);  // a flag byte is 0 or 1
    }
  }
  const uint32_t k = 256u * b + t;
  const int on = flag[k];
  const int sc = dpp_incl_scan(c), so = dpp_incl_scan(on);
  if (lane == 63) {
    wtot[w] = sc;
    wtot[4 + w] = so;
  }
  __syncthreads();
  int p = so - on;
#pragma unroll
  for (int i = 0; i < 4; i++) p += wtot[i] + (i < w ? wtot[4 + i] : 0);
  key_off[k] = (uint32_t)p;
  if (on) keys[p] = (uint16_t)k;
  if (k == 65535) {
    key_off[65536] = (uint32_t)(p + on);
    *n_ctr = (unsigned long long)(p + on);
  }
}

// Every wave runs whole rounds of 64 values (the trip count is wave-uniform, so every lane takes
// part in every scan); a lane past the end holds a word index no value has and no bits.
// The word is read first (from L2, where the atomics execute) and the atomic skipped when its bits
// are all set already.  Bits are only ever set, so a stale read can cost an atomic but never lose one.
// (18x on 2^27 values of one key, -16 % on sorted dense input: DESIGN §3.9,
// profiles/from_values/build_perf.txt)
__global__ __launch_bounds__(256) void k_bld_scatter(const uint32_t* __restrict__ v, uint64_t n,
                                                     const uint32_t* __restrict__ key_off,
                                                     uint32_t* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (uint64_t)gridDim.x * 4;
  for (uint64_t base = wave * 64; base < n; base += nw * 64) {
    const uint64_t i = base + lane;
    uint32_t idx = 0xFFFFFFFFu, bits = 0;
    if (i < n) {
      const uint32_t x = v[i];
      // container index < 65,536, 2,048 words each: the word index fits 27 bits
      idx = key_off[x >> 16] * 2048u + ((x & 0xFFFFu) >> 5);
      bits = 1u << (x & 31);
    }
    bits = merge_same_word(idx, bits);
    const bool last = from_next_lane(idx, 0xFFFFFFFFu) != idx;
    if (bits && last) {
      const uint32_t cur = __hip_atomic_load(&ws[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((cur & bits) != bits) atomicOr(&ws[idx], bits);
    }
  }
}

// the plan and write stages over the scattered workspace (build.hpp: the bodies, shared with bitset.hip)
__global__ __launch_bounds__(256) void k_bld_plan(const uint8_t* __restrict__ ws, uint64_t n, int run_optimize,
                                                  BldInfo* __restrict__ info, uint64_t* __restrict__ size,
                                                  unsigned long long* __restrict__ totals) {
  bld_plan_body(WsSource{ws}, n, run_optimize, info, size, totals);
}

__global__ __launch_bounds__(256, 4) void k_bld_write(const uint8_t* __restrict__ ws, uint64_t n,
                                                      const BldInfo* __restrict__ info,
                                                      const uint64_t* __restrict__ off,
                                                      const uint16_t* __restrict__ keys, CDesc* __restrict__ desc,
                                                      uint32_t* __restrict__ bm, uint32_t* __restrict__ bm_off,
                                                      uint8_t* __restrict__ payload) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  bld_write_body(WsSource{ws}, n, info, off, keys, desc, bm, bm_off, payload, lds_all);
}

void launch_bld_keys(hipStream_t s, const uint32_t* v, uint64_t n, uint8_t* flag, uint16_t* keys, uint32_t* key_off,
                     unsigned long long* n_ctr) {
  if (n) hipLaunchKernelGGL(k_bld_keys, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, s, v, n, flag);
  hipLaunchKernelGGL(k_bld_key_scan, dim3(256), dim3(256), 0, s, (const uint8_t*)flag, keys, key_off, n_ctr);
}

void launch_bld_scatter(hipStream_t s, const uint32_t* v, uint64_t n, const uint32_t* key_off, uint32_t* ws) {
  if (!n) return;
  const dim3 grid(grid_for(n, 256, 256 * 16)), block(256);
  hipLaunchKernelGGL(k_bld_scatter, grid, block, 0, s, v, n, key_off, ws);
}

void launch_bld_plan(hipStream_t s, const uint8_t* ws, uint64_t n_ctr, int run_optimize, void* info, uint64_t* size,
                     unsigned long long* totals) {
  if (!n_ctr) return;
  hipLaunchKernelGGL(k_bld_plan, dim3(grid_for(n_ctr, 4, 4096)), dim3(256), 0, s, ws, n_ctr, run_optimize,
                     reinterpret_cast<BldInfo*>(info), size, totals);
}

void launch_bld_write(hipStream_t s, const uint8_t* ws, uint64_t n_ctr, const void* info, const uint64_t* off,
                      const uint16_t* keys, CDesc* desc, uint32_t* bm, uint32_t* bm_off, uint8_t* payload) {
  if (!n_ctr) return;
  hipLaunchKernelGGL(k_bld_write, dim3(grid_for(n_ctr, 4, 4096)), dim3(256), 0, s, ws, n_ctr,
                     reinterpret_cast<const BldInfo*>(info), off, keys, desc, bm, bm_off, payload);
}

}  // namespace rbg
