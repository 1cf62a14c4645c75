// The plan and write stages of the device builders, shared by their sources: one wave per container reads its
// 65,536 bits through SRC and types, sizes and writes it.
//   build.hip   WsSource: container i is bitmap i of a workspace the scatter filled (from values)
//   bitset.hip  BitsSource: container i is block keys[i] of the caller's own packed words (from a dense bitset)
// SRC::load(i, x) fills the wave's registers with container i (wave-uniform i).
#pragma once
#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

struct BldInfo {
  uint32_t card;
  uint16_t nruns;
  uint8_t kind;
  uint8_t pad;
};
static_assert(sizeof(BldInfo) == kBldInfoBytes, "the engine sizes the plan's table by kBldInfoBytes");

struct WsSource {
  const uint8_t* ws;  // n bitmaps of 8 KiB, 16 B aligned
  __device__ __forceinline__ void load(uint64_t i, WCtr& x) const { w_load_bitmap(ws + 8192 * i, x); }
};

// totals (u64, zeroed by the caller): [0..2] containers of kind A / B / R, [3] serialized payload
// bytes, [4] cardinality
template <class SRC>
__device__ __forceinline__ void bld_plan_body(const SRC& src, uint64_t n, int run_optimize, BldInfo* __restrict__ info,
                                              uint64_t* __restrict__ size, unsigned long long* __restrict__ totals) {
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  unsigned long long cnt[3] = {0, 0, 0}, ser = 0, cards = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nw) {
    WCtr x;
    src.load(i, x);
    const int card = w_card(x);
    int kind = by_card(card), nruns = 0;
    if (run_optimize) {
      nruns = w_runs(x);
      kind = runopt_kind(kind, card, nruns);
    }
    const uint32_t len = ser_len_of(kind, (uint32_t)card, (uint32_t)nruns);
    if (lane == 0) {
      info[i] = BldInfo{(uint32_t)card, (uint16_t)nruns, (uint8_t)kind, 0};
      size[i] = slot_bytes(kind, len);
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

// lds_all: the workgroup's four 8 KiB stages, one per wave
template <class SRC>
__device__ __forceinline__ void bld_write_body(const SRC& src, uint64_t n, const BldInfo* __restrict__ info,
                                               const uint64_t* __restrict__ off, const uint16_t* __restrict__ keys,
                                               CDesc* __restrict__ desc, uint32_t* __restrict__ bm,
                                               uint32_t* __restrict__ bm_off, uint8_t* __restrict__ payload,
                                               uint32_t (*lds_all)[2048]) {
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
    const int kind = in.kind;
    WCtr x;
    src.load(i, x);
    w_write_slot(kind, x, (int)in.card, lds, payload + o);
    if (lane == 0) {
      desc[i] = CDesc{o, in.card, keys[i], (uint8_t)kind, 0};
      bm[i] = 0;
    }
  }
}

}  // namespace rbg
