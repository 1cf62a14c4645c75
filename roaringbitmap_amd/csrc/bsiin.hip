// WHERE value IN (v1, ..., vn) over a resident bit-sliced index: the buffer package's parallelIn
// (bsi/.../buffer/BitSliceIndexBase.java, BBSI/:611-639, with parallelExec :99-136 and parallelMR :148-164)
// for the key-major batch [ebM, bA[0..nbits-1], foundSet?] and a sorted, distinct value list in device
// memory, as a one-bitmap batch in bsibuild.hip's workspace layout (m = 1 cell per key) so that its plan /
// scan / write stages type and place the result:
//
//   k_bsiin_keys  per key of the universe: flag[key] = 1 where the key is a candidate (ebM has a container
//                 and, with a foundSet, the foundSet has one too) and cards[key] = the cardinality of the
//                 container of `fixed` (the foundSet, or ebM without one).  k_bld_key_scan (build.hip) turns
//                 the flags into the K candidate keys; the exclusive scan of cards gives r(key), the number
//                 of values of `fixed` below key << 16, which decides where parallelExec's batches fall.
//   k_bsi_in      one workgroup per candidate key.  ebM's container becomes an 8 KiB bitmap in LDS whatever
//                 its type; a thread owns 8 of its words and ANDs the foundSet's words in.  Per non-zero
//                 word the values are rebuilt a slice word at a time (k_bsi_pairs' transposition) and
//                 looked up in the list together: one branch-free binary search whose steps are uniform
//                 (the list length decides them) with independent probes per step, a probe made only for
//                 a column that is present.  A word of up to four columns keeps four value registers
//                 instead of 32.  An array slice is walked with a per-thread cursor (one binary search per
//                 slice and thread, not per slice and word).  The list sits in LDS up to kBsiInLdsList
//                 values and is searched in global memory above.  The surviving bits are the key's result
//                 cell; every cell of the pass is written, so the workspace needs no memset.
//
// A long list is sorted and de-duplicated on the device (hipcub's radix sort and unique, as decode.hip sorts
// its keys): the host's std::sort of 2^20 values alone took longer than the rest of the query.
//
// Types: batchIn's add() and the lazy or of parallelMR both type a container by its final
// cardinality, except that a full container is RunContainer.full() when its 65,536 columns come from two or
// more batches -- always, unless batchSize == 65536 and r(key) % 65536 == 0.  run[ki] carries that to
// k_bsib_plan's ebm_run argument.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "bsival.hpp"

namespace rbg {

__global__ __launch_bounds__(256) void k_bsiin_keys(const BsiValArgs a, int has_found, uint8_t* __restrict__ flag,
                                                    uint64_t* __restrict__ cards) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;  // 256 workgroups: every key
  const uint32_t c0 = a.key_off[k], c1 = a.key_off[k + 1];
  // (key, input) order: ebM's container is the segment's first, the foundSet's its last
  const bool he = c0 < c1 && a.bm[c0] == 0;
  const bool hf = has_found && c0 < c1 && a.bm[c1 - 1] == (uint32_t)a.nbits + 1;
  flag[k] = he && (hf || !has_found) ? 1 : 0;
  cards[k] = has_found ? (hf ? (uint64_t)a.desc[c1 - 1].card : 0ull) : (he ? (uint64_t)a.desc[c0].card : 0ull);
}

// One word (32 columns, wi of 2048) of a key: the candidate columns of `word` whose value is in the list.
// The values are rebuilt a slice word at a time and all looked up together: a branch-free binary search whose
// steps are uniform, the probes of one step independent.  W = 32: every column of the word has a value
// register; W = 4: a word of at most four columns keeps those alone (bp: their bit positions, 32 = none), an
// eighth of the work.  v[], pos[] and bp[] are indexed by unrolled loops only: registers.
template <int W>
__device__ __forceinline__ uint32_t bsiin_word(const BsiValArgs& a, const CDesc* sd, const uint32_t* sin, uint32_t ns,
                                               uint16_t (*cur)[256], const uint32_t* L, uint32_t n, uint32_t top,
                                               uint32_t wi, uint32_t word, int t) {
  uint32_t bp[W], v[W], pos[W];
  uint32_t rem = word;
#pragma unroll
  for (int i = 0; i < W; i++) {
    bp[i] = W == 32 ? (uint32_t)i : rem ? (uint32_t)__ffs(rem) - 1u : 32u;
    rem &= rem - 1;
    v[i] = 0, pos[i] = 0;
  }
  for (uint32_t s = 0; s < ns; s++) {
    if (sin[s] > (uint32_t)a.nbits) break;  // the foundSet
    uint32_t sw;
    if (sd[s].kind == DK_A) {  // uniform over the workgroup
      const uint16_t* av = reinterpret_cast<const uint16_t*>(a.payload + sd[s].slot);
      const uint32_t card = sd[s].card, base = 32u * wi;
      uint32_t c = cur[s][t];
      while (c < card && av[c] < base) c++;  // values under words that hold no candidate
      sw = 0;
      for (; c < card && av[c] <= base + 31u; c++) sw |= 1u << (av[c] & 31);
      cur[s][t] = (uint16_t)c;
      sw &= word;
    } else {
      sw = bsiv_word(sd[s], a.payload, wi) & word;
    }
    if (!sw) continue;
    const uint32_t sh = sin[s] - 1;
#pragma unroll
    for (int i = 0; i < W; i++) v[i] |= ((sw >> (bp[i] & 31)) & 1u) << sh;
  }
  // pos[i] -> the number of list entries <= v[i]; it stays 0 where the word has no column
  for (uint32_t half = top; half; half >>= 1) {
#pragma unroll
    for (int i = 0; i < W; i++) {
      const uint32_t p = pos[i] + half;
      const bool on = W == 32 ? (word >> i) & 1u : bp[i] < 32;
      if (on && p <= n && L[p - 1] <= v[i]) pos[i] = p;
    }
  }
  uint32_t keep = 0;
#pragma unroll
  for (int i = 0; i < W; i++)
    if (pos[i] && L[pos[i] - 1] == v[i]) keep |= 1u << (bp[i] & 31);
  return keep;
}

// list[0..n): ascending, distinct, n >= 1; top: the largest power of two <= n.  LDSL: the list is staged in
// dynamic LDS (n <= kBsiInLdsList).  aligned: batchSize == 65536.  Cell ki - k_lo of ws, run[ki].
template <bool LDSL>
__global__ __launch_bounds__(256) void k_bsi_in(const BsiValArgs a, int has_found, const uint32_t* __restrict__ list,
                                                uint32_t n, uint32_t top, const uint16_t* __restrict__ pkeys,
                                                uint32_t k_lo, const uint64_t* __restrict__ rank, int aligned,
                                                uint8_t* __restrict__ ws, uint8_t* __restrict__ run) {
  extern __shared__ uint32_t slist[];
  __shared__ __align__(16) uint32_t bmp[2048];
  __shared__ CDesc sd[kBsiMaxInputs];
  __shared__ uint32_t sin[kBsiMaxInputs];
  __shared__ int wtot[4];
  __shared__ uint16_t cur[32][256];  // per array slice: the thread's position in the slice's values
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t ki = k_lo + blockIdx.x;
  const uint32_t key = pkeys[ki];
  const uint32_t c0 = a.key_off[key], c1 = a.key_off[key + 1];  // a candidate key: c0 < c1, ebM first
  const CDesc e = a.desc[c0];
  const uint32_t ns = min(c1 - c0 - 1, (uint32_t)kBsiMaxInputs);
  if ((uint32_t)t < ns) {
    sd[t] = a.desc[c0 + 1 + t];
    sin[t] = a.bm[c0 + 1 + t];
  }
  if (LDSL)
    for (uint32_t i = t; i < n; i += 256) slist[i] = list[i];
  bsiv_stage_bitmap(e, a.payload, bmp, t);
  __syncthreads();
  const uint32_t* L = LDSL ? slist : list;
  {
    // cur[s][t] = the values of array slice s below the thread's first column, 256 t: one binary search per
    // slice and thread instead of one per slice and word, eight slices' searches in flight together
    const uint32_t first = 256u * (uint32_t)t;
    for (uint32_t s0 = 0; s0 < ns && s0 < 32; s0 += 8) {
      const uint16_t* vp[8];
      uint32_t cd[8], lo[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t s = s0 + k;
        const bool on = s < ns && sin[s] <= (uint32_t)a.nbits && sd[s].kind == DK_A;
        vp[k] = reinterpret_cast<const uint16_t*>(a.payload + (on ? sd[s].slot : 0));
        cd[k] = on ? sd[s].card : 0u;
        lo[k] = 0;
      }
      for (uint32_t half = 4096; half; half >>= 1) {  // an array holds at most 4,096 values
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const uint32_t p = lo[k] + half;
          if (p <= cd[k] && vp[k][p - 1] < first) lo[k] = p;
        }
      }
#pragma unroll
      for (int k = 0; k < 8; k++) cur[s0 + k][t] = (uint16_t)lo[k];
    }
  }
  int cnt = 0;
#pragma unroll 1
  for (int j = 0; j < 8; j++) {
    const uint32_t wi = (uint32_t)(8 * t + j);
    uint32_t word = bmp[wi];
    if (word && has_found) word &= bsiv_word(sd[ns - 1], a.payload, wi);  // a candidate key: the segment's last
    uint32_t keep = 0;
    if (word && __popc(word) <= 4) keep = bsiin_word<4>(a, sd, sin, ns, cur, L, n, top, wi, word, t);
    else if (word) keep = bsiin_word<32>(a, sd, sin, ns, cur, L, n, top, wi, word, t);
    bmp[wi] = keep;  // the thread's own word: nobody else reads it
    cnt += __popc(keep);
  }
  uint4* cell = reinterpret_cast<uint4*>(ws + 8192ull * (uint64_t)(ki - k_lo)) + 2 * t;
  cell[0] = reinterpret_cast<const uint4*>(bmp)[2 * t];
  cell[1] = reinterpret_cast<const uint4*>(bmp)[2 * t + 1];
  const int sc = dpp_incl_scan(cnt);
  if (lane == 63) wtot[w] = sc;
  __syncthreads();
  if (t == 0) {
    const bool full = wtot[0] + wtot[1] + wtot[2] + wtot[3] == 65536;
    run[ki] = full && !(aligned && (rank[key] & 0xFFFFull) == 0) ? 1 : 0;
  }
}

size_t bsiin_sort_temp_bytes(uint64_t n) {
  size_t a = 0, b = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 32,
                                          (hipStream_t)0);
  (void)hipcub::DeviceSelect::Unique(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                     (unsigned long long*)nullptr, (int)n, (hipStream_t)0);
  return std::max(a, b) + 256;
}

int launch_bsiin_sort_unique(hipStream_t s, void* temp, size_t temp_bytes, uint32_t* list, uint32_t* scratch,
                             unsigned long long* n_out, uint64_t n) {
  hipError_t e = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, (const uint32_t*)list, scratch, (int)n, 0, 32, s);
  if (e != hipSuccess) return (int)e;
  return (int)hipcub::DeviceSelect::Unique(temp, temp_bytes, (const uint32_t*)scratch, list, n_out, (int)n, s);
}

void launch_bsiin_keys(hipStream_t s, BsiValArgs a, int has_found, uint8_t* flag, uint64_t* cards) {
  hipLaunchKernelGGL(k_bsiin_keys, dim3(256), dim3(256), 0, s, a, has_found, flag, cards);
}

void launch_bsi_in(hipStream_t s, BsiValArgs a, int has_found, const uint32_t* list, uint32_t n, const uint16_t* pkeys,
                   uint32_t k_lo, uint32_t k_hi, const uint64_t* rank, bool aligned, uint8_t* ws, uint8_t* run) {
  if (k_hi <= k_lo || !n) return;
  uint32_t top = 1;
  while (top <= n / 2) top *= 2;
  const dim3 grid(k_hi - k_lo), block(256);
  if (n <= kBsiInLdsList)
    hipLaunchKernelGGL(k_bsi_in<true>, grid, block, 4 * (size_t)n, s, a, has_found, list, n, top, pkeys, k_lo, rank,
                       aligned ? 1 : 0, ws, run);
  else
    hipLaunchKernelGGL(k_bsi_in<false>, grid, block, 0, s, a, has_found, list, n, top, pkeys, k_lo, rank,
                       aligned ? 1 : 0, ws, run);
}

}  // namespace rbg
