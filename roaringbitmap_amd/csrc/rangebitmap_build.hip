// A resident range-encoded index from a value tensor, on the device: RangeBitmap.Appender (RB/RangeBitmap.java:
// add :1511-1533, append :1543-1588) for n rows at once, as the directory, masks and arena that
// rangebitmap_format.hpp's walk of the Appender's stream gives (engine_rangebitmap.cpp: ctx_rb_load).
//
// Row r is values[r]; block k is rows [65536 k, 65536 (k + 1)); cell (k, i) holds the block's rows whose value
// has bit i CLEAR.  The row position is the array index, so nothing is scattered, sorted or combined with
// atomics (unlike bsibuild.hip, where the column decides the position):
//
//   k_rbb_max        the largest value, unsigned (one atomic per wave); the host refuses one outside the mask
//   k_rbb_transpose  a wave takes 1,024 consecutive rows as 16 groups of 64, one u64 per lane (a coalesced
//                    512 B load each).  For slice i, __ballot(bit i of ~v & mask, row < n) IS the 64-bit word of
//                    cell (k, i) for that group; lane i keeps the words of slice i, so after the 16 groups it
//                    stores 128 contiguous bytes into its cell.  Every word of every cell of the pass is
//                    written, zeros at and past row n included: the workspace is never zeroed.
//   k_rbb_plan       build.hpp's plan stage, one wave per cell: cardinality and run count, then the kind by THIS
//                    stream's typing (not the batch builders'): slices 0-4 are BitmapContainers put through
//                    runOptimize (runopt_kind(DK_B, c, r): a run iff 2 + 4 r < 8192, else a bitmap of any
//                    cardinality), slices 5 and up RunContainers put through toEfficientContainer (eff(c, r)).
//                    An empty cell is no container.
//   (the exclusive scan of the slot sizes over all cells)
//   k_rbb_write      build.hpp's write stage: the slot (wave.hpp: w_write_slot) and the directory entry
//                    dir[k nslices + i], kAbsent for an empty cell; a run's entry carries cardinality 0, as the
//                    loader's does
//   k_rbb_masks      bit i of block k's mask = cell (k, i) is not empty
//
// The workspace is n_blocks x nslices x 8 KiB, so the engine walks the blocks in passes [k_lo, k_hi) under a byte
// budget.  All byte offsets are 64-bit.
#include <algorithm>

#include "build.hpp"

namespace rbg {

static_assert(sizeof(BldInfo) == kRbbInfoBytes, "the engine sizes the plan's table by kRbbInfoBytes");

__global__ __launch_bounds__(256) void k_rbb_max(const uint64_t* __restrict__ v, uint64_t n,
                                                 unsigned long long* __restrict__ out) {
  unsigned long long hi = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    hi = max(hi, (unsigned long long)v[i]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) hi = max(hi, (unsigned long long)__shfl_xor(hi, d, 64));
  if ((threadIdx.x & 63) == 0 && hi) atomicMax(out, hi);
}

constexpr int kRbbGroups = 16;                  // 64-row groups per wave task
constexpr int kRbbTaskRows = 64 * kRbbGroups;   // 1,024 rows: 128 B of every cell
constexpr int kRbbTasksPerBlock = 65536 / kRbbTaskRows;

// Task t of the pass: block k_lo + t / 64, rows [1024 (t % 64), +1024) of it.  The loop over the slices is
// wave-uniform; a ballot lands in scalar registers and lane i takes it with one select per half.
__global__ __launch_bounds__(256) void k_rbb_transpose(const uint64_t* __restrict__ v, uint64_t n, uint64_t mask,
                                                       uint32_t k_lo, uint64_t n_tasks, int nslices,
                                                       uint8_t* __restrict__ ws) {
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tasks; t += nw) {
    const uint64_t kb = t / kRbbTasksPerBlock, sub = t % kRbbTasksPerBlock;  // block of the pass, task of the block
    const uint64_t row0 = ((uint64_t)k_lo + kb) * 65536 + sub * kRbbTaskRows + lane;
    uint64_t c[kRbbGroups], w[kRbbGroups];
#pragma unroll
    for (int g = 0; g < kRbbGroups; g++) {
      const uint64_t r = row0 + 64 * g;
      c[g] = r < n ? ~__builtin_nontemporal_load(v + r) & mask : 0;  // a row at or past n is in no slice
      w[g] = 0;
    }
#pragma unroll 1
    for (int i = 0; i < nslices; i++) {
      const bool mine = lane == i;
#pragma unroll
      for (int g = 0; g < kRbbGroups; g++) {
        const uint64_t b = __ballot((c[g] >> i) & 1);
        w[g] = mine ? b : w[g];
      }
    }
    if (lane < nslices) {
      uint4* dst = reinterpret_cast<uint4*>(ws + 8192ull * (kb * (uint64_t)nslices + lane) + 8ull * kRbbGroups * sub);
#pragma unroll
      for (int g = 0; g < kRbbGroups; g += 2)
        dst[g / 2] = make_uint4((uint32_t)w[g], (uint32_t)(w[g] >> 32), (uint32_t)w[g + 1], (uint32_t)(w[g + 1] >> 32));
    }
  }
}

// Cell j of the pass: block k_lo + j / nslices, slice j % nslices; its bitmap at ws + 8192 j, its info / size
// entry at k_lo nslices + j.
__global__ __launch_bounds__(256) void k_rbb_plan(const uint8_t* __restrict__ ws, uint64_t cell0, uint64_t cells,
                                                  uint32_t nslices, BldInfo* __restrict__ info,
                                                  uint64_t* __restrict__ size, unsigned long long* __restrict__ payload) {
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  unsigned long long bytes = 0;
  for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < cells; j += nw) {
    WCtr x;
    w_load_bitmap(ws + 8192ull * j, x);
    const int card = w_card(x);
    if (card == 0) {  // wave-uniform
      if (lane == 0) {
        info[cell0 + j] = BldInfo{0, 0, 0, 0};
        size[cell0 + j] = 0;
      }
      continue;
    }
    const int nruns = w_runs(x);
    const int kind = (cell0 + j) % nslices < 5 ? runopt_kind(DK_B, card, nruns) : eff(card, nruns);
    const uint32_t len = ser_len_of(kind, (uint32_t)card, (uint32_t)nruns);
    if (lane == 0) {
      info[cell0 + j] = BldInfo{(uint32_t)card, (uint16_t)nruns, (uint8_t)kind, 0};
      size[cell0 + j] = slot_bytes(kind, len);
    }
    bytes += kind == DK_R ? len - 2 : len;  // a run record's count is its size field, not payload
  }
  if (lane == 0 && bytes) atomicAdd(payload, bytes);
}

__global__ __launch_bounds__(256) void k_rbb_write(const uint8_t* __restrict__ ws, uint64_t cell0, uint64_t cells,
                                                   uint32_t nslices, const BldInfo* __restrict__ info,
                                                   const uint64_t* __restrict__ off, CDesc* __restrict__ dir,
                                                   uint8_t* __restrict__ arena) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < cells; j += nw) {
    const uint64_t cell = cell0 + j;
    const BldInfo in = info[cell];
    const uint16_t key = (uint16_t)(cell / nslices);
    if (in.card == 0) {  // wave-uniform
      if (lane == 0) dir[cell] = CDesc{0, 0, key, kAbsent, 0};
      continue;
    }
    const uint64_t o = off[cell];
    const int kind = in.kind;
    WCtr x;
    w_load_bitmap(ws + 8192ull * j, x);
    w_write_slot(kind, x, (int)in.card, lds, arena + o);
    if (lane == 0) dir[cell] = CDesc{o, kind == DK_R ? 0u : in.card, key, (uint8_t)kind, 0};
  }
}

__global__ __launch_bounds__(256) void k_rbb_masks(const BldInfo* __restrict__ info, uint32_t k_lo, uint32_t k_hi,
                                                   uint32_t nslices, uint64_t* __restrict__ masks) {
  const uint32_t k = k_lo + blockIdx.x * 256 + threadIdx.x;
  if (k >= k_hi) return;
  uint64_t m = 0;
  for (uint32_t i = 0; i < nslices; i++) m |= (uint64_t)(info[(uint64_t)k * nslices + i].card != 0) << i;
  masks[k] = m;
}

void launch_rbb_max(hipStream_t s, const uint64_t* v, uint64_t n, unsigned long long* max) {
  if (!n) return;
  hipLaunchKernelGGL(k_rbb_max, dim3(grid_for(n, 1024, 2048)), dim3(256), 0, s, v, n, max);
}

void launch_rbb_transpose(hipStream_t s, const uint64_t* v, uint64_t n, uint64_t mask, uint32_t k_lo, uint32_t k_hi,
                          int nslices, uint8_t* ws) {
  if (k_hi <= k_lo) return;
  const uint64_t n_tasks = (uint64_t)(k_hi - k_lo) * kRbbTasksPerBlock;
  hipLaunchKernelGGL(k_rbb_transpose, dim3(grid_for(n_tasks, 4, 16384)), dim3(256), 0, s, v, n, mask, k_lo, n_tasks,
                     nslices, ws);
}

void launch_rbb_plan(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int nslices, void* info,
                     uint64_t* size, unsigned long long* payload) {
  if (k_hi <= k_lo) return;
  const uint64_t cells = (uint64_t)(k_hi - k_lo) * nslices;
  hipLaunchKernelGGL(k_rbb_plan, dim3(grid_for(cells, 4, 4096)), dim3(256), 0, s, ws, (uint64_t)k_lo * nslices, cells,
                     (uint32_t)nslices, reinterpret_cast<BldInfo*>(info), size, payload);
}

void launch_rbb_write(hipStream_t s, const uint8_t* ws, uint32_t k_lo, uint32_t k_hi, int nslices, const void* info,
                      const uint64_t* off, CDesc* dir, uint64_t* masks, uint8_t* arena) {
  if (k_hi <= k_lo) return;
  const uint64_t cells = (uint64_t)(k_hi - k_lo) * nslices;
  hipLaunchKernelGGL(k_rbb_write, dim3(grid_for(cells, 4, 4096)), dim3(256), 0, s, ws, (uint64_t)k_lo * nslices, cells,
                     (uint32_t)nslices, reinterpret_cast<const BldInfo*>(info), off, dir, arena);
  hipLaunchKernelGGL(k_rbb_masks, dim3((k_hi - k_lo + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const BldInfo*>(info), k_lo, k_hi, (uint32_t)nslices, masks);
}

}  // namespace rbg
