// Range-encoded index queries on the device: RangeBitmap (RB/RangeBitmap.java).
//
// An index is up to 64 range-encoded bit slices over blocks of 65,536 rows; slice i of a block holds the rows
// whose value has bit i CLEAR (Appender.add, :1511-1533).  Every query form evaluates each block on its own
// (SingleEvaluation :418-901, DoubleEvaluation :903-1281): the block's slice containers are ORed / ANDed /
// removed, slice 0 upward, into one 8 KiB bitset, which is then cut to the block's rows, ANDed with the
// context's container of that key and typed.  k_rb_query is that loop with a wave per block: the bitset lives
// in the wave's registers (WCtr; `between` holds two, low and high, and a third for the container both take),
// a slice container is combined through wave.hpp's w_combine / w_materialize from its slot in the index's
// arena (rangebitmap_format.hpp: the records re-laid at load into 16 B aligned slots with a directory entry
// per (block, slice), so no record is ever walked on the device).
//
// The reference's `empty` / `full` flags (:424, :1283-1357) only save work on bits known to be all zero or
// all one; they never change a bit, so the kernel does not carry them.  What it does follow is the skip rule:
// slices below the most significant position where both the threshold and the block's mask are 0 are not
// read (:672-685, :1018-1031).
//
// Output: the bits of block k at out + 8192 k (every block is written, so the workspace needs no zeroing), from
// which the dense-bitset builder (bitset.hip, run_optimize) makes the result batch; or, out == null, the
// cardinalities summed into one word, a block's bits never leaving the registers.
#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

// rows [0, limit) of the block, limit in 1..65536
__device__ __forceinline__ void w_set_rows(WCtr& x, int limit) {
#pragma unroll
  for (int k = 0; k < 16; k++) x.w[k] = wrange(k, 0, limit - 1);
}
__device__ __forceinline__ void w_flip_rows(WCtr& x, int limit) {
#pragma unroll
  for (int k = 0; k < 16; k++) x.w[k] ^= wrange(k, 0, limit - 1);
}

// x = x OP container (op: 0 and, 1 or, 3 andnot; wave-uniform)
__device__ __forceinline__ void rb_apply(int op, const CDesc& d, const uint8_t* arena, uint32_t* lds, WCtr& x) {
  if (op == 0) w_combine<0>(d, arena, lds, x);
  else if (op == 1) w_combine<1>(d, arena, lds, x);
  else w_combine<3>(d, arena, lds, x);
}

// 64 - numberOfLeadingZeros(~(t | cm) & mask): the slices below this position are wasted work (:674)
__device__ __forceinline__ int rb_skip(uint64_t t, uint64_t cm, uint64_t mask) {
  const uint64_t z = ~(t | cm) & mask;
  return z ? 64 - __clzll((long long)z) : 0;
}

// evaluateHorizontalSliceRange (:671-734): x = the block's rows with value <= t
__device__ __forceinline__ void rb_eval_range(const RbArgs& a, const CDesc* dir, uint64_t cm, int limit, uint32_t* lds,
                                              WCtr& x) {
  const uint64_t t = a.t0;
  const int skip = rb_skip(t, cm, a.mask);
  int slice;
  if (skip > 0) {
    w_zero(x);
    slice = skip;
  } else {
    if (t & 1) {
      w_set_rows(x, limit);
    } else {
      w_zero(x);
      if (cm & 1) rb_apply(1, dir[0], a.arena, lds, x);
    }
    slice = 1;
  }
#pragma unroll 1
  for (; slice < (int)a.nslices; slice++)
    if ((cm >> slice) & 1) rb_apply((t >> slice) & 1 ? 1 : 0, dir[slice], a.arena, lds, x);
}

// evaluateHorizontalSlicePoint (:736-770): x = the block's rows with value == t
__device__ __forceinline__ void rb_eval_point(const RbArgs& a, const CDesc* dir, uint64_t cm, int limit, uint32_t* lds,
                                              WCtr& x) {
  const uint64_t v = a.t0;
  // a slice the value lacks and the block has no container for: no row has that bit clear
  if (~(v | cm) & a.mask) {
    w_zero(x);
    return;
  }
  w_set_rows(x, limit);
#pragma unroll 1
  for (int slice = 0; slice < (int)a.nslices; slice++)
    if ((cm >> slice) & 1) rb_apply((v >> slice) & 1 ? 3 : 0, dir[slice], a.arena, lds, x);
}

// DoubleEvaluation.evaluateHorizontalSlice (:1016-1061) and the AND of compute (:919-933):
// x = the block's rows with lower < value <= upper
__device__ __forceinline__ void rb_eval_between(const RbArgs& a, const CDesc* dir, uint64_t cm, int limit,
                                                uint32_t* lds, WCtr& x) {
  uint64_t lower = a.t0, upper = a.t1;
  const int skip_low = rb_skip(lower, cm, a.mask), skip_high = rb_skip(upper, cm, a.mask);
  if (skip_low == 64) lower = 0;
  else if (skip_low > 0) lower &= ~0ull << skip_low;
  if (skip_high == 64) upper = 0;
  else if (skip_high > 0) upper &= ~0ull << skip_high;
  WCtr low, y;  // x is `high`
  // setupFirstSlice (:1063-1076); a copy (skip == 0 with the threshold's bit 0 clear) implies cm & 1
  if (upper & 1) w_set_rows(x, limit);
  else w_zero(x);
  if (lower & 1) w_set_rows(low, limit);
  else w_zero(low);
  const bool copy_high = !(upper & 1) && skip_high == 0 && (cm & 1);
  const bool copy_low = !(lower & 1) && skip_low == 0 && (cm & 1);
  if (copy_high | copy_low) {
    w_materialize(dir[0], a.arena, lds, y);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      if (copy_high) x.w[k] |= y.w[k];
      if (copy_low) low.w[k] |= y.w[k];
    }
  }
#pragma unroll 1
  for (int slice = 1; slice < (int)a.nslices; slice++) {
    if (!((cm >> slice) & 1)) continue;
    w_materialize(dir[slice], a.arena, lds, y);
    const bool or_high = (upper >> slice) & 1, or_low = (lower >> slice) & 1;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      x.w[k] = or_high ? x.w[k] | y.w[k] : x.w[k] & y.w[k];
      low.w[k] = or_low ? low.w[k] | y.w[k] : low.w[k] & y.w[k];
    }
  }
  w_flip_rows(low, limit);
#pragma unroll
  for (int k = 0; k < 16; k++) x.w[k] &= low.w[k];
}

template <int MODE>
__global__ __launch_bounds__(256) void k_rb_query(const RbArgs a) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const uint32_t nw = gridDim.x * 4;
  long long cnt = 0;
  for (uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6); b < a.n_blocks; b += nw) {
    const uint32_t k = uni(b);
    WCtr x;
    CDesc cd{};
    if (a.has_ctx) {  // keys the context lacks are skipped, those past its last key never visited (:468-472)
      uint32_t p = a.ctx.key_off[k];
      bool visit = a.ctx.key_off[k + 1] > p;
      if (a.ctx_first) {  // ctx.n >= 1: an empty context never reaches the kernel
        visit = k >= a.ctx.desc[0].key && k <= a.ctx.desc[a.ctx.n - 1].key;
        p = 0;
      }
      if (!visit) {
        if (a.out) {
          w_zero(x);
          w_store_bitmap(a.out + 8192ull * k, x);
        }
        continue;
      }
      cd = a.ctx.desc[p];
    }
    const uint64_t rem = a.max_rid - 65536ull * k;  // >= 1: k < ceil(max_rid / 65536)
    const int limit = rem < 65536 ? (int)rem : 65536;
    const uint64_t cm = a.masks[k];
    const CDesc* dir = a.dir + (size_t)k * a.nslices;
    if (MODE == RBM_LTE || MODE == RBM_GT) rb_eval_range(a, dir, cm, limit, lds, x);
    else if (MODE == RBM_EQ || MODE == RBM_NEQ) rb_eval_point(a, dir, cm, limit, lds, x);
    else rb_eval_between(a, dir, cm, limit, lds, x);
    if (MODE == RBM_GT || MODE == RBM_NEQ) w_flip_rows(x, limit);
    if (a.has_ctx) w_combine<0>(cd, a.ctx.payload, lds, x);
    if (a.out) {
      w_store_bitmap(a.out + 8192ull * k, x);
    } else {
      const int c = w_card(x);
      cnt += a.ctx_minus ? (int)cd.card - c : c;
    }
  }
  if (!a.out && lane_id() == 0 && cnt) atomicAdd(a.count, (unsigned long long)cnt);
}

void launch_rb_query(hipStream_t s, int mode, const RbArgs& a) {
  if (!a.n_blocks) return;
  const dim3 grid(grid_for(a.n_blocks, 4, 4096)), block(256);
  switch (mode) {
    case RBM_LTE: hipLaunchKernelGGL(k_rb_query<RBM_LTE>, grid, block, 0, s, a); break;
    case RBM_GT: hipLaunchKernelGGL(k_rb_query<RBM_GT>, grid, block, 0, s, a); break;
    case RBM_EQ: hipLaunchKernelGGL(k_rb_query<RBM_EQ>, grid, block, 0, s, a); break;
    case RBM_NEQ: hipLaunchKernelGGL(k_rb_query<RBM_NEQ>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(k_rb_query<RBM_BETWEEN>, grid, block, 0, s, a); break;
  }
}

}  // namespace rbg
