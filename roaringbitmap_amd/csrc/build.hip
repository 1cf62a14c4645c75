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
//                  (C bitmaps).  Lanes of a wave whose neighbours hit the same 32-bit word
//                  combine their bits first (a DPP scan over the lanes); only the last lane of
//                  each group of equal neighbours issues the atomic, so sorted, clustered or
//                  repeated input does not serialise 64 atomics at one address.
//   k_bld_plan     one wave per container: cardinality (and run count) from registers, the
//                  container's type and slot size, the batch totals
//   (scan of the slot sizes)
//   k_bld_write    one wave per container: the slot (A padded to 16 B with its last value,
//                  R = [u16 pad][u16 nruns][u32 (start, len - 1)]), the CDesc, keys[], bm[] = 0
//
// Types (format.cpp: make_ctr with kind_hint -1): card <= 4096 -> A, else B; with run_optimize
// A -> R iff 2 card > 2 + 4 nruns (RB/ArrayContainer.java:1085-1099), B -> R iff
// 2 + 4 nruns < 8192 (RB/BitmapContainer.java:1218-1237).  Either way a run result has at most
// 2,047 runs, so it fits the wave's 8 KiB stage.
#include <algorithm>

#include "kernels.hpp"
#include "wave.hpp"

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

// lane l receives lane l + 1's value; lane 63 receives `last`
__device__ __forceinline__ uint32_t next_lane_or(uint32_t x, uint32_t last) {
  return __builtin_amdgcn_update_dpp(last, x, 0x130, 0xf, 0xf, false);  // wave_shl:1
}

// One DPP step of the combining scan: a lane ORs in the bits of the lane `ctrl` points at when both
// address the same word.  A lane without a source keeps its own word index as the source's (old =
// its own values), which ORs its own bits again: harmless.
#define BLD_STEP(ctrl, rmask)                                                                         \
  {                                                                                                   \
    const uint32_t si = __builtin_amdgcn_update_dpp(idx, idx, ctrl, rmask, 0xf, false);               \
    const uint32_t sb = __builtin_amdgcn_update_dpp(bits, bits, ctrl, rmask, 0xf, false);             \
    bits |= si == idx ? sb : 0u;                                                                      \
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
    // After the scan a lane holds the bits of every lane before it in its group of equal
    // neighbours (a lane may also pick up bits of the same word from further away: they belong
    // to the word too).
    BLD_STEP(0x111, 0xf)  // row_shr:1
    BLD_STEP(0x112, 0xf)  // row_shr:2
    BLD_STEP(0x114, 0xf)  // row_shr:4
    BLD_STEP(0x118, 0xf)  // row_shr:8
    BLD_STEP(0x142, 0xa)  // row_bcast:15 -> rows 1, 3
    BLD_STEP(0x143, 0xc)  // row_bcast:31 -> rows 2, 3
    const uint32_t nxt = next_lane_or(idx, 0xFFFFFFFFu);
    if (bits && nxt != idx) {
      const uint32_t cur = __hip_atomic_load(&ws[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((cur & bits) != bits) atomicOr(&ws[idx], bits);
    }
  }
}
#undef BLD_STEP

struct BldInfo {
  uint32_t card;
  uint16_t nruns;
  uint8_t kind;
  uint8_t pad;
};
static_assert(sizeof(BldInfo) == kBldInfoBytes, "the engine sizes the plan's table by kBldInfoBytes");

__device__ __forceinline__ uint64_t bld_slot_size(int kind, uint32_t ser_len) {
  return kind == DK_R ? (uint64_t)((ser_len + 2 + 15) & ~15u) : (uint64_t)((ser_len + 15) & ~15u);
}

// totals (u64, zeroed by the caller): [0..2] containers of kind A / B / R, [3] serialized payload
// bytes, [4] cardinality
__global__ __launch_bounds__(256) void k_bld_plan(const uint8_t* __restrict__ ws, uint64_t n, int run_optimize,
                                                  BldInfo* __restrict__ info, uint64_t* __restrict__ size,
                                                  unsigned long long* __restrict__ totals) {
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  unsigned long long cnt[3] = {0, 0, 0}, ser = 0, cards = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nw) {
    WCtr x;
    w_load_bitmap(ws + 8192 * i, x);
    const int card = w_card(x);
    int kind = by_card(card), nruns = 0;
    if (run_optimize) {
      nruns = w_runs(x);
      if (kind == DK_A ? 2 * card > 2 + 4 * nruns : 2 + 4 * nruns < 8192) kind = DK_R;
    }
    const uint32_t len = kind == DK_A ? 2u * card : kind == DK_B ? 8192u : 2u + 4u * nruns;
    if (lane == 0) {
      info[i] = BldInfo{(uint32_t)card, (uint16_t)nruns, (uint8_t)kind, 0};
      size[i] = bld_slot_size(kind, len);
    }
    cnt[kind]++;
    ser += len;
    cards += (unsigned long long)card;
  }
  if (lane == 0) {  // one add per counter per wave
    for (int k = 0; k < 3; k++)
      if (cnt[k]) atomicAdd(&totals[k], cnt[k]);
    if (ser) atomicAdd(&totals[3], ser);
    if (cards) atomicAdd(&totals[4], cards);
  }
}

__global__ __launch_bounds__(256, 4) void k_bld_write(const uint8_t* __restrict__ ws, uint64_t n,
                                                      const BldInfo* __restrict__ info,
                                                      const uint64_t* __restrict__ off,
                                                      const uint16_t* __restrict__ keys, CDesc* __restrict__ desc,
                                                      uint32_t* __restrict__ bm, uint32_t* __restrict__ bm_off,
                                                      uint8_t* __restrict__ payload) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the bitmap CSR of a one-bitmap batch
    bm_off[0] = 0;
    bm_off[1] = (uint32_t)n;
  }
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nw) {
    const BldInfo in = info[i];
    const uint64_t o = off[i];
    uint8_t* dst = payload + o;
    const int kind = in.kind, card = (int)in.card;
    WCtr x;
    w_load_bitmap(ws + 8192 * i, x);
    if (kind == DK_B) {
      w_store_bitmap(dst, x);
    } else {
      uint32_t copy = w_stage(kind, x, card, lds);
      if (kind == DK_A) {  // pad the slot to 16 B with the last value (batch layout)
        uint16_t* st = reinterpret_cast<uint16_t*>(lds);
        const uint32_t c = in.card, padded = (2u * c + 15) & ~15u;
        const uint16_t last = st[c - 1];
        for (uint32_t q = c + lane; q < padded / 2; q += 64) st[q] = last;
        wsync();
        copy = padded;
      } else if (lane == 0) {
        *reinterpret_cast<uint16_t*>(dst) = 0;  // the u16 in front of the run count
      }
      copy_lds_to_global<64>(dst + (kind == DK_R ? 2 : 0), lds, copy, lane);
      wsync();
    }
    if (lane == 0) {
      desc[i] = CDesc{o, in.card, keys[i], (uint8_t)kind, 0};
      bm[i] = 0;
    }
  }
}

static unsigned bld_grid(uint64_t items, uint64_t per_block, uint64_t cap) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, cap));
}

void launch_bld_keys(hipStream_t s, const uint32_t* v, uint64_t n, uint8_t* flag, uint16_t* keys, uint32_t* key_off,
                     unsigned long long* n_ctr) {
  if (n) hipLaunchKernelGGL(k_bld_keys, dim3(bld_grid(n, 256, 256 * 16)), dim3(256), 0, s, v, n, flag);
  hipLaunchKernelGGL(k_bld_key_scan, dim3(256), dim3(256), 0, s, (const uint8_t*)flag, keys, key_off, n_ctr);
}

void launch_bld_scatter(hipStream_t s, const uint32_t* v, uint64_t n, const uint32_t* key_off, uint32_t* ws) {
  if (!n) return;
  const dim3 grid(bld_grid(n, 256, 256 * 16)), block(256);
  hipLaunchKernelGGL(k_bld_scatter, grid, block, 0, s, v, n, key_off, ws);
}

void launch_bld_plan(hipStream_t s, const uint8_t* ws, uint64_t n_ctr, int run_optimize, void* info, uint64_t* size,
                     unsigned long long* totals) {
  if (!n_ctr) return;
  hipLaunchKernelGGL(k_bld_plan, dim3(bld_grid(n_ctr, 4, 4096)), dim3(256), 0, s, ws, n_ctr, run_optimize,
                     reinterpret_cast<BldInfo*>(info), size, totals);
}

void launch_bld_write(hipStream_t s, const uint8_t* ws, uint64_t n_ctr, const void* info, const uint64_t* off,
                      const uint16_t* keys, CDesc* desc, uint32_t* bm, uint32_t* bm_off, uint8_t* payload) {
  if (!n_ctr) return;
  hipLaunchKernelGGL(k_bld_write, dim3(bld_grid(n_ctr, 4, 4096)), dim3(256), 0, s, ws, n_ctr,
                     reinterpret_cast<const BldInfo*>(info), off, keys, desc, bm, bm_off, payload);
}

}  // namespace rbg
