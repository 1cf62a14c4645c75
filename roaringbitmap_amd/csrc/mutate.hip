// A batch of values added to or removed from a resident bitmap: RoaringBitmap.add(int...) / addN
// (RB/RoaringBitmap.java:483, 498-570), add(int) (:1162), remove(int) (:2637-2648), checkedAdd (:1610),
// checkedRemove (:1646) over n values (u32, any order, duplicates allowed) and one single-bitmap key-major
// batch, as a new batch.  For adds alone or removes alone the result does not depend on the order of the
// values, so it is computed per key from the final bit set:
//
//   array / bitmap container   ArrayContainer.add turns into a bitmap container above 4,096 values
//                              (RB/ArrayContainer.java:143-171), BitmapContainer.remove into an array
//                              container at 4,096 (RB/BitmapContainer.java:1184-1202), BitmapContainer.add
//                              returns this: the type the final cardinality gives (by_card)
//   run container              RunContainer.add / remove (RB/RunContainer.java:248-302, 2038-2070) return
//                              this: a run container of the maximal runs of the final bit set, 1 to 32,768
//   new key (add)              a fresh ArrayContainer: by_card
//   emptied container          dropped (remove(int), :2645-2647)
//   key no value touches       its container as it is, slot bytes copied
//
// Only touched keys get an 8 KiB cell.  The keys come from launch_bld_keys (build.hip) over the values and,
// through k_mut_flags, over the operand's key CSR: `cell` is the CSR of the keys with a cell (add: every
// touched key; remove: touched and present), `cand` the CSR of the keys the result may hold (add: touched or
// present; remove: the operand's own).
//
//   k_mut_flags   flag[key] = touched | present (add) or touched & present (remove), for the second key scan
//   k_mut_expand  one wave per cell: the operand's container of the key materialised into the cell, a new
//                 key as zeros.  Every cell is written: the workspace needs no memset.  was_run and the old
//                 cardinality are kept per cell.
//   k_mut_apply   one value per lane in whole rounds of 64; lanes of one 32-bit word combine their bits
//                 (wave.hpp: merge_same_word) and the last lane of such a group reads the word and issues
//                 one atomicOr (add) / atomicAnd of the complement (remove) only when a bit would change.
//                 Bits move one way within a launch, so a stale read can cost an atomic but never lose one.
//   k_mut_plan    64 candidate keys per wave: an untouched key by one lane from the operand's CDesc (a run
//                 container's run count is the one u16 read from its slot), the touched keys among them by the
//                 whole wave in turn from their cells (cardinality, and for was_run the run count); kind, kept
//                 or dropped, slot size, the totals
//   (one scan of keep << kMutCountShift | slot bytes: dropped keys are compacted out)
//   k_mut_write   one wave per kept key: a touched A / B / R of at most 2,047 runs through w_write_slot, a
//                 longer touched R straight from the registers to global memory (w_stage_runs_chunk without
//                 the LDS cap, as w_place_big_runs), an untouched slot copied in 16-byte vectors; CDesc,
//                 keys[], bm[] = 0, bm_off = {0, C'}
#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

struct MutInfo {
  uint32_t card;
  uint16_t nruns;  // R: 1..32,768
  uint8_t kind;
  uint8_t flags;  // 1 kept, 2 touched
};
static_assert(sizeof(MutInfo) == kMutInfoBytes, "the engine sizes the plan's table by kMutInfoBytes");

__global__ __launch_bounds__(256) void k_mut_flags(const uint8_t* __restrict__ touched,
                                                   const uint32_t* __restrict__ a_key_off, int a_has, int op,
                                                   uint8_t* __restrict__ flag) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;  // 256 workgroups: one thread per key
  const int t = touched[k];
  const int p = a_has ? a_key_off[k + 1] != a_key_off[k] : 0;
  flag[k] = (uint8_t)(op == 0 ? (t | p) : (t & p));
}

__global__ __launch_bounds__(256) void k_mut_expand(const BmView A, const uint16_t* __restrict__ cell_keys,
                                                    uint32_t n_cells, uint8_t* __restrict__ ws,
                                                    uint8_t* __restrict__ was_run, uint32_t* __restrict__ old_card) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const uint32_t ci = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ci >= n_cells) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint32_t key = uni(cell_keys[ci]);
  uint32_t p = 0, e = 0;
  if (A.n) {
    p = uni(A.key_off[key]);
    e = uni(A.key_off[key + 1]);
  }
  WCtr x;
  int run = 0, card = 0;
  if (p < e) {
    const CDesc d = A.desc[p];
    w_materialize(d, A.payload, lds, x);
    run = d.kind == DK_R;
    card = w_card(x);
  } else {
    w_zero(x);
  }
  w_store_bitmap(ws + 8192ull * ci, x);
  if (lane_id() == 0) {
    was_run[ci] = (uint8_t)run;
    old_card[ci] = (uint32_t)card;
  }
}

// cell_off: the cell CSR (65,537 entries): a key has a cell iff its two entries differ.  ws: n_cells <=
// 65,536 bitmaps, so a word index fits 27 bits.
__global__ __launch_bounds__(256) void k_mut_apply(const uint32_t* __restrict__ v, uint64_t n, int op,
                                                   const uint32_t* __restrict__ cell_off,
                                                   uint32_t* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (uint64_t)gridDim.x * 4;
  for (uint64_t base = wave * 64; base < n; base += nw * 64) {
    const uint64_t i = base + lane;
    uint32_t idx = 0xFFFFFFFFu, bits = 0;
    if (i < n) {
      const uint32_t x = v[i];
      const uint32_t ci = cell_off[x >> 16];
      if (cell_off[(x >> 16) + 1] != ci) {  // a remove under an absent key has no cell
        idx = ci * 2048u + ((x & 0xFFFFu) >> 5);
        bits = 1u << (x & 31);
      }
    }
    bits = merge_same_word(idx, bits);
    const bool last = from_next_lane(idx, 0xFFFFFFFFu) != idx;
    if (bits && last) {
      const uint32_t cur = __hip_atomic_load(&ws[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (op == 0) {
        if ((cur & bits) != bits) atomicOr(&ws[idx], bits);
      } else {
        if (cur & bits) atomicAnd(&ws[idx], ~bits);
      }
    }
  }
}

// totals (u64, zeroed by the caller): [0..2] kept containers of kind A / B / R, [3] serialized payload
// bytes, [4] cardinality, [5] values added or removed, [6] serialized bytes of containers above 8,194 B
__global__ __launch_bounds__(256) void k_mut_plan(const BmView A, const uint16_t* __restrict__ cand_keys,
                                                  uint64_t n_cand, const uint32_t* __restrict__ cell_off,
                                                  const uint8_t* __restrict__ ws,
                                                  const uint8_t* __restrict__ was_run,
                                                  const uint32_t* __restrict__ old_card, MutInfo* __restrict__ info,
                                                  uint64_t* __restrict__ size, unsigned long long* __restrict__ totals) {
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  // A wave takes 64 candidates at a time, one per lane: an untouched one is planned by its lane alone, the
  // touched ones among them by the whole wave in turn.  The sums go through a wave reduction, one add per
  // counter per wave and round.  (One wave per candidate, each ending in its own atomics on the totals' one
  // cache line, took 0.60 ms per launch over 65,536 untouched keys, of a 0.76 ms call: DESIGN §3.18,
  // profiles/mutate/mutate_kernel_times_wave_per_candidate.txt.)
  for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < n_cand; base += nw * 64) {
    const uint64_t i = base + lane;
    const bool in = i < n_cand;
    uint32_t key = 0, ci = 0;
    bool touched = false;
    int card = 0, kind = DK_A, nruns = 0, delta = 0;
    if (in) {
      key = cand_keys[i];
      ci = cell_off[key];
      touched = cell_off[key + 1] != ci;
      if (!touched) {  // a candidate no value touches is a key of the operand
        const CDesc d = A.desc[A.key_off[key]];
        card = (int)d.card;
        kind = d.kind;
        if (kind == DK_R) nruns = *reinterpret_cast<const uint16_t*>(A.payload + d.slot + 2);
      }
    }
    for (uint64_t m = __ballot(touched); m; m &= m - 1) {  // wave-uniform
      const int src = __builtin_ctzll(m);
      const uint32_t tci = uni((uint32_t)__shfl((int)ci, src));
      WCtr x;
      w_load_bitmap(ws + 8192ull * tci, x);
      const int c = w_card(x);
      int k = by_card(c), nr = 0;
      if (uni(was_run[tci])) {
        nr = w_runs(x);
        k = DK_R;
      }
      if (lane == src) {
        card = c;
        kind = k;
        nruns = nr;
        const int oc = (int)old_card[tci];
        delta = c > oc ? c - oc : oc - c;
      }
    }
    const bool keep = in && card != 0;
    const uint32_t len = keep ? ser_len_of(kind, (uint32_t)card, (uint32_t)nruns) : 0u;
    if (in) {
      info[i] = MutInfo{(uint32_t)card, (uint16_t)nruns, (uint8_t)kind, (uint8_t)((keep ? 1 : 0) | (touched ? 2 : 0))};
      size[i] = keep ? ((1ull << kMutCountShift) | slot_bytes(kind, len)) : 0ull;
    }
    // 64 candidates: every sum fits 32 bits (64 x 131,074 serialized bytes, 64 x 65,536 values)
    const int n_a = wave_sum_i(keep && kind == DK_A), n_b = wave_sum_i(keep && kind == DK_B),
              n_r = wave_sum_i(keep && kind == DK_R), ser = wave_sum_i((int)len), cards = wave_sum_i(keep ? card : 0),
              changed = wave_sum_i(delta), big = wave_sum_i(len > 8194u ? (int)len : 0);
    if (lane == 0) {
      if (n_a) atomicAdd(&totals[0], (unsigned long long)n_a);
      if (n_b) atomicAdd(&totals[1], (unsigned long long)n_b);
      if (n_r) atomicAdd(&totals[2], (unsigned long long)n_r);
      if (ser) atomicAdd(&totals[3], (unsigned long long)ser);
      if (cards) atomicAdd(&totals[4], (unsigned long long)cards);
      if (changed) atomicAdd(&totals[5], (unsigned long long)changed);
      if (big) atomicAdd(&totals[6], (unsigned long long)big);
    }
  }
}

// n 16-byte vectors from src to dst, both 16 B aligned: four loads in flight per lane
__device__ __forceinline__ void w_copy_slot(uint8_t* dst, const uint8_t* src, uint32_t nvec) {
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (uint32_t j = lane_id(); j < nvec; j += 256) {
    uint4 a[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (j + 64 * k < nvec) a[k] = ld_in(s4 + j + 64 * k);
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (j + 64 * k < nvec) d4[j + 64 * k] = a[k];
  }
}

// off: the exclusive scan of size[]: container index << kMutCountShift | payload offset
__global__ __launch_bounds__(256, 4) void k_mut_write(const BmView A, const uint16_t* __restrict__ cand_keys,
                                                      uint64_t n_cand, uint32_t n_out,
                                                      const uint32_t* __restrict__ cell_off,
                                                      const uint8_t* __restrict__ ws,
                                                      const MutInfo* __restrict__ info,
                                                      const uint64_t* __restrict__ off, CDesc* __restrict__ desc,
                                                      uint16_t* __restrict__ keys, uint32_t* __restrict__ bm,
                                                      uint32_t* __restrict__ bm_off, uint8_t* __restrict__ payload) {
  __shared__ __align__(16) uint32_t lds_all[4][2048];
  uint32_t* lds = lds_all[threadIdx.x >> 6];
  const int lane = lane_id();
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the bitmap CSR of a one-bitmap batch
    bm_off[0] = 0;
    bm_off[1] = n_out;
  }
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n_cand; i += nw) {
    MutInfo in = info[i];
    in.card = uni(in.card);  // one record per wave: every branch below is wave-uniform
    in.nruns = (uint16_t)uni(in.nruns);
    in.kind = (uint8_t)uni(in.kind);
    in.flags = (uint8_t)uni(in.flags);
    if (!(in.flags & 1)) continue;  // dropped
    const uint64_t word = off[i];
    const uint64_t o = word & ((1ull << kMutCountShift) - 1);
    const uint32_t j = (uint32_t)(word >> kMutCountShift);
    const uint32_t key = uni(cand_keys[i]);
    const int kind = in.kind;
    uint8_t* dst = payload + o;
    if (in.flags & 2) {
      WCtr x;
      w_load_bitmap(ws + 8192ull * uni(cell_off[key]), x);
      if (kind != DK_R || in.nruns <= 2047) {
        w_write_slot(kind, x, (int)in.card, lds, dst);
      } else {  // does not fit the LDS stage: [u16 0][u16 nruns][(start, length - 1) pairs] from the registers
        const int nr = in.nruns;
        uint16_t* st = reinterpret_cast<uint16_t*>(dst + 2);
        w_stage_runs_chunk<0, (1 << 30)>(x, st, 0, 0);  // ends as absolute positions first
        __threadfence_block();
        wsync();
        for (int p = lane; p < nr; p += 64) st[2 + 2 * p] = (uint16_t)(st[2 + 2 * p] - st[1 + 2 * p]);
        if (lane == 0) {
          st[0] = (uint16_t)nr;
          *reinterpret_cast<uint16_t*>(dst) = 0;
        }
      }
    } else {
      const CDesc d = A.desc[uni(A.key_off[key])];
      const uint32_t len = ser_len_of(kind, in.card, in.nruns);
      w_copy_slot(dst, A.payload + d.slot, (uint32_t)(slot_bytes(kind, len) >> 4));
    }
    if (lane == 0) {
      desc[j] = CDesc{o, in.card, (uint16_t)key, (uint8_t)kind, 0};
      keys[j] = (uint16_t)key;
      bm[j] = 0;
    }
  }
}

void launch_mut_flags(hipStream_t s, const uint8_t* touched, const uint32_t* a_key_off, bool a_has, int op,
                      uint8_t* flag) {
  hipLaunchKernelGGL(k_mut_flags, dim3(256), dim3(256), 0, s, touched, a_key_off, a_has ? 1 : 0, op, flag);
}

void launch_mut_expand(hipStream_t s, BmView a, const uint16_t* cell_keys, uint32_t n_cells, uint8_t* ws,
                       uint8_t* was_run, uint32_t* old_card) {
  if (!n_cells) return;
  hipLaunchKernelGGL(k_mut_expand, dim3((n_cells + 3) / 4), dim3(256), 0, s, a, cell_keys, n_cells, ws, was_run,
                     old_card);
}

void launch_mut_apply(hipStream_t s, const uint32_t* v, uint64_t n, int op, const uint32_t* cell_off, uint32_t* ws) {
  if (!n) return;
  hipLaunchKernelGGL(k_mut_apply, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, s, v, n, op, cell_off, ws);
}

void launch_mut_plan(hipStream_t s, BmView a, const uint16_t* cand_keys, uint64_t n_cand, const uint32_t* cell_off,
                     const uint8_t* ws, const uint8_t* was_run, const uint32_t* old_card, void* info, uint64_t* size,
                     unsigned long long* totals) {
  if (!n_cand) return;
  hipLaunchKernelGGL(k_mut_plan, dim3(grid_for(n_cand, 256, 4096)), dim3(256), 0, s, a, cand_keys, n_cand, cell_off, ws,
                     was_run, old_card, reinterpret_cast<MutInfo*>(info), size, totals);
}

void launch_mut_write(hipStream_t s, BmView a, const uint16_t* cand_keys, uint64_t n_cand, uint32_t n_out,
                      const uint32_t* cell_off, const uint8_t* ws, const void* info, const uint64_t* off, CDesc* desc,
                      uint16_t* keys, uint32_t* bm, uint32_t* bm_off, uint8_t* payload) {
  if (!n_cand) return;
  hipLaunchKernelGGL(k_mut_write, dim3(grid_for(n_cand, 4, 4096)), dim3(256), 0, s, a, cand_keys, n_cand, n_out,
                     cell_off, ws, reinterpret_cast<const MutInfo*>(info), off, desc, keys, bm, bm_off, payload);
}

}  // namespace rbg
