// Dense bitsets and resident bitmaps, both ways, on the device: BitSetUtil (RB/BitSetUtil.java).
//
// Build: bitmapOf(long[] words) (:160-174) with containerOf (:270-283), and bitmapOf(ByteBuffer) (:185-259).
// Block b is words [1024 b, 1024 b + 1024) of the input, zero padded at the end; an all-zero block gives no
// container, another gives key b: an array up to 4,096 bits, else a bitmap; never a run container unless
// runOptimize() (RB/RoaringBitmap.java:2764-2774) follows (run_optimize: runopt_kind, device.hpp).  The
// caller's words ARE the workspace of 8 KiB bitmaps that build.hip has to scatter into, so nothing is
// zeroed, scattered or copied; the input is read three times and the payload written once:
//
//   k_bits_flags   one wave per block: flag[b] = the block holds a bit
//   k_bld_key_scan (build.hip) keys[], the key CSR, the container count C
//   k_bits_plan    build.hpp's plan stage, container i read from words + 8192 keys[i]
//   (scan of the slot sizes)
//   k_bits_write   build.hpp's write stage over the same source
//
// The input is only 8 B aligned and ends anywhere, in the middle of a word too (a tail of 1..7 bytes is a
// last word, :238-251): wave.hpp's w_load_bitmap_bounded reads no byte at or past the end.
//
// A mask (one byte per element, nonzero = set) is first packed into such words (k_bits_pack): 1 + 1/8 + 3/8
// bytes moved per element against 3 for stages that would each read the bytes themselves.
//
// Expansion: toLongArray (:67-108) over a window of bit positions [first, first + n), as packed words or as
// mask bytes.  k_bits_expand: one wave per key the window touches.  The key's container is found through the
// batch's key CSR (absent: zeros), materialised into registers (wave.hpp: w_materialize; a bitmap container is
// just loaded) and its part of the window stored.  Every word or byte of the window is written exactly once,
// nothing outside it, with no atomics and no zeroing before.
#include <algorithm>

#include "build.hpp"

namespace rbg {

struct BitsSource {
  const uint8_t* bits;   // the caller's packed words, 8 B aligned
  uint64_t nbytes;       // readable bytes
  const uint16_t* keys;  // container i is block keys[i]
  __device__ __forceinline__ void load(uint64_t i, WCtr& x) const {
    const uint64_t o = 8192ull * keys[i];  // below nbytes: the block was flagged
    w_load_bitmap_bounded(bits + o, nbytes - o, x);
  }
};

__global__ __launch_bounds__(256) void k_bits_flags(const uint8_t* __restrict__ bits, uint64_t nbytes, uint32_t nblocks,
                                                    uint8_t* __restrict__ flag) {
  const uint32_t nw = gridDim.x * 4;
  for (uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6); b < nblocks; b += nw) {
    WCtr x;
    w_load_bitmap_bounded(bits + 8192ull * b, nbytes - 8192ull * b, x);
    uint64_t any = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) any |= x.w[k];
    const bool on = __ballot(any != 0) != 0;
    if (lane_id() == 0 && on) flag[b] = 1;
  }
}

__global__ __launch_bounds__(256) void k_bits_plan(BitsSource src, uint64_t n, int run_optimize,
                                                   BldInfo* __restrict__ info, uint64_t* __restrict__ size,
                                                   unsigned long long* __restrict__ totals) {
  bld_plan_body(src, n, run_optimize, info, size, totals);
}

__global__ __launch_bounds__(256, 4) void k_bits_write(BitsSource src, uint64_t n, const BldInfo* __restrict__ info,
                                                       const uint64_t* __restrict__ off, CDesc* __restrict__ desc,
                                                       uint32_t* __restrict__ bm, uint32_t* __restrict__ bm_off,
                                                       uint8_t* __restrict__ payload) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  bld_write_body(src, n, info, off, src.keys, desc, bm, bm_off, payload, lds_all);
}

// bit i of the result = byte i of w is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) {
  const uint32_t t = (w | ((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u;  // 0x80 in every nonzero byte
  return (t * 0x00204081u) >> 28;  // bits 7, 15, 23, 31 -> 28..31 (the partial products never meet)
}
// byte i of the result = bit i of nib (4 bits)
__device__ __forceinline__ uint32_t bits_to_bytes(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }

// A mask of n elements as ceil(n / 64) words, written 16 bits at a time: thread g packs elements
// [16 g, 16 g + 16), those at or past n being zero whatever the memory holds; n_units = 4 ceil(n / 64).
__global__ __launch_bounds__(256) void k_bits_pack(const uint8_t* __restrict__ mask, uint64_t n, uint64_t n_units,
                                                   uint16_t* __restrict__ out) {
  const bool aligned = (reinterpret_cast<uintptr_t>(mask) & 15) == 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_units; g += stride) {
    const uint64_t base = 16 * g;
    uint32_t bits = 0;
    if (aligned && base + 16 <= n) {
      const uint4 v = ld_in(reinterpret_cast<const uint4*>(mask + base));
      bits = nonzero_bytes(v.x) | (nonzero_bytes(v.y) << 4) | (nonzero_bytes(v.z) << 8) | (nonzero_bytes(v.w) << 12);
    } else {
      for (uint32_t j = 0; j < 16 && base + j < n; j++) bits |= (mask[base + j] != 0 ? 1u : 0u) << j;
    }
    out[g] = (uint16_t)bits;
  }
}

struct ExpandArgs {
  const uint32_t* key_off;  // the batch's key CSR (65,537 entries)
  const CDesc* desc;
  const uint8_t* payload;
  uint64_t first, n;  // the window of bit positions; first + n <= 2^32, n >= 1; packed: first % 64 == 0
  void* out;          // packed: ceil(n / 64) u64, 8 B aligned; mask: n bytes
};

// 16 bits of the wave's LDS bitmap from container bit cb on, cb in [-15, 65535]; bits outside the container
// come out as anything (the caller stores none of them)
__device__ __forceinline__ uint32_t lds_bits16(const uint32_t* lds, int cb) {
  const int wi = cb >> 5;
  const uint32_t lo = lds[wi < 0 ? 0 : wi], hi = lds[wi + 1 > 2047 ? 2047 : wi + 1];
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (cb & 31)) & 0xFFFFu;
}

template <bool MASK>
__global__ __launch_bounds__(256, 4) void k_bits_expand(const ExpandArgs a) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const int lane = lane_id();
  const uint64_t end = a.first + a.n;
  const uint32_t k0 = (uint32_t)(a.first >> 16), nk = (uint32_t)((end - 1) >> 16) - k0 + 1;
  const uint32_t nw = gridDim.x * 4;
  for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < nk; t += nw) {
    const uint32_t key = k0 + t;  // <= 65535
    const uint32_t p = a.key_off[key];
    WCtr x;
    if (a.key_off[key + 1] > p) {
      const CDesc d = a.desc[p];
      w_materialize(d, a.payload, lds, x);
    } else {
      w_zero(x);
    }
    if (!MASK) {
      uint64_t* out = reinterpret_cast<uint64_t*>(a.out);
      const int64_t nwords = (int64_t)((a.n + 63) >> 6);
      const int64_t w0 = (int64_t)key * 1024 - (int64_t)(a.first >> 6);  // output index of the container's word 0
      const uint64_t tail = (a.n & 63) ? (~0ull >> (64 - (a.n & 63))) : ~0ull;  // bits at or past n are zero
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int64_t oi = w0 + 128 * i + 2 * lane;
        uint64_t v0 = x.w[2 * i], v1 = x.w[2 * i + 1];
        if (oi == nwords - 1) v0 &= tail;
        if (oi + 1 == nwords - 1) v1 &= tail;
        const bool in0 = oi >= 0 && oi < nwords, in1 = oi + 1 >= 0 && oi + 1 < nwords;
        if (in0 && in1 && (reinterpret_cast<uintptr_t>(out + oi) & 15) == 0) {
          *reinterpret_cast<uint4*>(out + oi) =
              make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32));
        } else {
          if (in0) out[oi] = v0;
          if (in1) out[oi + 1] = v1;
        }
      }
    } else {
      // through the wave's LDS bitmap, in 16 B units of the output's own alignment: a lane turns 16 bits into
      // 16 bytes, the wave stores 1 KiB at a time; the units the window's ends cut go out byte by byte
      wsync();
      w_write_lds(lds, x);
      wsync();
      uint8_t* out = reinterpret_cast<uint8_t*>(a.out);
      const int64_t cbase = (int64_t)key * 65536 - (int64_t)a.first;  // output index of the container's bit 0
      const int64_t o_lo = cbase > 0 ? cbase : 0;
      const int64_t o_hi = cbase + 65536 < (int64_t)a.n ? cbase + 65536 : (int64_t)a.n;
      const uintptr_t base = reinterpret_cast<uintptr_t>(out);
      const uintptr_t u_end = base + (uintptr_t)o_hi;
      for (uintptr_t u = ((base + (uintptr_t)o_lo) & ~(uintptr_t)15) + 16u * lane; u < u_end; u += 1024) {
        const int64_t o = (int64_t)u - (int64_t)base;  // >= o_lo - 15
        const uint32_t bits = lds_bits16(lds, (int)(o - cbase));
        if (o >= o_lo && o + 16 <= o_hi) {
          *reinterpret_cast<uint4*>(u) = make_uint4(bits_to_bytes(bits & 15), bits_to_bytes((bits >> 4) & 15),
                                                    bits_to_bytes((bits >> 8) & 15), bits_to_bytes(bits >> 12));
        } else {
          for (int j = 0; j < 16; j++)
            if (o + j >= o_lo && o + j < o_hi) out[o + j] = (uint8_t)((bits >> j) & 1u);
        }
      }
    }
  }
}

void launch_bits_flags(hipStream_t s, const uint8_t* bits, uint64_t nbytes, uint8_t* flag, uint16_t* keys,
                       uint32_t* key_off, unsigned long long* n_ctr) {
  const uint64_t nblocks = (nbytes + 8191) / 8192;  // <= 65,536: the engine refuses more than 2^32 bits
  if (nblocks)
    hipLaunchKernelGGL(k_bits_flags, dim3(grid_for(nblocks, 4, 4096)), dim3(256), 0, s, bits, nbytes,
                       (uint32_t)nblocks, flag);
  launch_bld_keys(s, nullptr, 0, flag, keys, key_off, n_ctr);  // the scan alone
}

void launch_bits_plan(hipStream_t s, const uint8_t* bits, uint64_t nbytes, const uint16_t* keys, uint64_t n_ctr,
                      int run_optimize, void* info, uint64_t* size, unsigned long long* totals) {
  if (!n_ctr) return;
  hipLaunchKernelGGL(k_bits_plan, dim3(grid_for(n_ctr, 4, 4096)), dim3(256), 0, s, BitsSource{bits, nbytes, keys},
                     n_ctr, run_optimize, reinterpret_cast<BldInfo*>(info), size, totals);
}

void launch_bits_write(hipStream_t s, const uint8_t* bits, uint64_t nbytes, const uint16_t* keys, uint64_t n_ctr,
                       const void* info, const uint64_t* off, CDesc* desc, uint32_t* bm, uint32_t* bm_off,
                       uint8_t* payload) {
  if (!n_ctr) return;
  hipLaunchKernelGGL(k_bits_write, dim3(grid_for(n_ctr, 4, 4096)), dim3(256), 0, s, BitsSource{bits, nbytes, keys},
                     n_ctr, reinterpret_cast<const BldInfo*>(info), off, desc, bm, bm_off, payload);
}

void launch_bits_pack(hipStream_t s, const uint8_t* mask, uint64_t n, uint64_t* words) {
  const uint64_t n_units = 4 * ((n + 63) / 64);
  if (!n_units) return;
  hipLaunchKernelGGL(k_bits_pack, dim3(grid_for(n_units, 256, 65536)), dim3(256), 0, s, mask, n, n_units,
                     reinterpret_cast<uint16_t*>(words));
}

void launch_bits_expand(hipStream_t s, const uint32_t* key_off, const CDesc* desc, const uint8_t* payload,
                        uint64_t first, uint64_t n, bool mask, void* out) {
  if (!n) return;
  const ExpandArgs a{key_off, desc, payload, first, n, out};
  const uint64_t nk = ((first + n - 1) >> 16) - (first >> 16) + 1;
  const dim3 grid(grid_for(nk, 4, 4096)), block(256);
  if (mask) hipLaunchKernelGGL(k_bits_expand<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_bits_expand<false>, grid, block, 0, s, a);
}

}  // namespace rbg
