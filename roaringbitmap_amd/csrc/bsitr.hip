// GROUP BY value / COUNT(*) over a resident bit-sliced index: the buffer package's parallelTransposeWithCount
// (bsi/.../buffer/BitSliceIndexBase.java, BBSI/:551-597, with parallelExec :99-136) for the key-major batch
// [ebM, bA[0..nbits-1], foundSet?].  The result is a new index whose columns are the distinct 32-bit values of
// the columns in ebM & fixed and whose values are how many columns held each, laid out in bsibuild.hip's
// workspace (m cells of 8 KiB per result key: the existence cell, then one per count bit) so that its plan /
// scan / write stages type and place it:
//
//   k_bsitr_sweep<0>  one workgroup per candidate input key (k_bsiin_keys' flags).  ebM's container, and the
//                     foundSet's, become 8 KiB bitmaps in LDS; a thread owns 8 words; per non-zero word the
//                     values are rebuilt a slice word at a time (bsiv_word) and rflag[value >> 16] is set.
//                     k_bld_key_scan turns the flags into the K' result keys and the key -> slot map.
//   k_bsitr_sweep<1>  the same rebuild; a column whose result key lies in the pass adds 1 to the key's count
//                     table (65,536 x u32, zeroed by the caller).  Equal addresses within a wave instruction are
//                     combined first: up to kBsitrPeel distinct addresses are peeled off by ballot (the first
//                     lane of each adds the number of lanes that share it), the lanes left over add 1 each.  A
//                     column of few distinct values therefore issues one atomic per wave and value, not 64 on
//                     one address; scattered values fall through to one atomic per column.
//   k_bsitr_cells     one workgroup per result key and sixteenth of its table: a wave ballot over 64
//                     consecutive counts is one 64-bit word of a cell (count != 0: the existence cell; bit i:
//                     slice i), staged in LDS and written as 512-byte segments.  Every cell of the pass is
//                     written, so the cells need no memset.  In the first sweep it also reduces the smallest
//                     and largest non-zero count and each key's cardinality (a key that reaches 65,536 is
//                     counted as full).
//                     The combined (address, count) pairs stay in a per-wave register cache of kBsitrCache
//                     entries until displaced or the key ends, so three distinct values over 2^24 columns cost
//                     a few atomics per wave and key instead of one per wave instruction.
//   k_bsitr_sweep<3>  the sparse route: the value of every column of ebM & fixed, unordered, for hipcub's radix
//                     sort and run-length encode; the (value, count) pairs then go through the build
//                     (bsibuild.hip) as (column, value) pairs.
//   k_bsitr_sweep<4>  only when a full result key can be RunContainer.full(): the value of every
//                     column that lies in a full key is set in a bitmap per (full key, batch of parallelExec), the
//                     batch from the column's rank in fixed; k_bsitr_full_runs walks a key's batches in order.
//   k_bsitr_sweep<2>  the same question when those bitmaps exceed the byte budget: (rank of the column in
//                     fixed, value) of every such column, for the host to sort and evaluate.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "bsival.hpp"

namespace rbg {

#ifndef RBG_BSITR_PEEL
#define RBG_BSITR_PEEL 4
#endif
constexpr int kBsitrPeel = RBG_BSITR_PEEL;  // distinct addresses of a wave instruction combined before the global atomic

constexpr int kBsitrCache = 4;  // (address, count) pairs a wave keeps in registers across its key

// The values of the columns of `word` (32 columns, wi of 2048) of a key, a slice word at a time; v[] is
// indexed by unrolled loops only: registers.
__device__ __forceinline__ void bsitr_values(const BsiValArgs& a, const CDesc* sd, const uint32_t* sin, uint32_t ns,
                                             uint32_t wi, uint32_t word, uint32_t (&v)[32]) {
#pragma unroll
  for (int i = 0; i < 32; i++) v[i] = 0;
  for (uint32_t s = 0; s < ns; s++) {
    if (sin[s] > (uint32_t)a.nbits) break;  // the foundSet
    const uint32_t sw = bsiv_word(sd[s], a.payload, wi) & word;
    if (!sw) continue;
    const uint32_t sh = sin[s] - 1;
#pragma unroll
    for (int i = 0; i < 32; i++) v[i] |= ((sw >> i) & 1u) << sh;
  }
}

// MODE 0: flags; MODE 1: counts of the result keys [k_lo, k_hi); MODE 2: (rank, value) of full keys; MODE 3: the
// value of every column
template <int MODE>
__global__ __launch_bounds__(256) void k_bsitr_sweep(const BsiValArgs a, int has_found, const uint16_t* __restrict__ ckeys,
                                                    const unsigned long long* __restrict__ n_ckeys, BsiTrSweep p) {
  __shared__ __align__(16) uint32_t bmp[2048];
  __shared__ __align__(16) uint32_t fbm[2048];
  __shared__ CDesc sd[kBsiMaxInputs];
  __shared__ uint32_t sin[kBsiMaxInputs];
  __shared__ int wtot[4];
  if ((unsigned long long)blockIdx.x >= *n_ckeys) return;  // the grid is sized by ebM's containers
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t key = ckeys[blockIdx.x];
  const uint32_t c0 = a.key_off[key], c1 = a.key_off[key + 1];  // a candidate key: c0 < c1, ebM first
  const CDesc e = a.desc[c0];
  const uint32_t ns = min(c1 - c0 - 1, (uint32_t)kBsiMaxInputs);
  if ((uint32_t)t < ns) {
    sd[t] = a.desc[c0 + 1 + t];
    sin[t] = a.bm[c0 + 1 + t];
  }
  bsiv_stage_bitmap(e, a.payload, bmp, t);
  if (has_found) bsiv_stage_bitmap(a.desc[c1 - 1], a.payload, fbm, t);  // a candidate key: the segment's last
  __syncthreads();
  uint32_t before = 0;  // MODE 2: columns of fixed in front of the thread's current word
  if (MODE == 2 || MODE == 4) {
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) cnt += __popc(has_found ? fbm[8 * t + j] : bmp[8 * t + j]);
    const int sc = dpp_incl_scan(cnt);
    if (lane == 63) wtot[w] = sc;
    __syncthreads();
    before = (uint32_t)(sc - cnt);
    for (int i = 0; i < w; i++) before += (uint32_t)wtot[i];
  }
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t ca[kBsitrCache], cc[kBsitrCache];  // MODE 1: the wave's pending (address, count) pairs, uniform
  int rr = 0;
#pragma unroll
  for (int c = 0; c < kBsitrCache; c++) ca[c] = 0, cc[c] = 0;
#pragma unroll 1
  for (int j = 0; j < 8; j++) {
    const uint32_t wi = (uint32_t)(8 * t + j);
    const uint32_t fw = has_found ? fbm[wi] : bmp[wi];
    const uint32_t word = bmp[wi] & fw;
    if (__ballot(word != 0) != 0) {  // the loop below is uniform over the wave: ballots inside
      uint32_t v[32];
      if (word) bsitr_values(a, sd, sin, ns, wi, word, v);
#pragma unroll
      for (int i = 0; i < 32; i++) {
        const bool on = (word >> i) & 1u;
        if (MODE == 0) {
          if (on) p.rflag[v[i] >> 16] = 1;
        } else if (MODE == 1) {
          uint32_t idx = 0;
          bool act = false;
          if (on) {
            const uint32_t s = p.rkoff[v[i] >> 16];
            act = s >= p.k_lo && s < p.k_hi;
            idx = (s - p.k_lo) * 65536u + (v[i] & 0xFFFFu);  // below 2^30: a pass holds at most 16,384 keys
          }
          uint64_t rem = __ballot(act);
          for (int r = 0; r < kBsitrPeel && rem; r++) {
            const int leader = __ffsll((unsigned long long)rem) - 1;
            const uint32_t a0 = (uint32_t)__shfl((int)idx, leader);
            const bool mine = act && idx == a0;
            const uint64_t same = __ballot(mine);
            const uint32_t n = (uint32_t)__popcll(same);
            if (r == 0 && n == 1) break;  // scattered values: one atomic per column below
            // (a0, n) is uniform over the wave: into the wave's cache of kBsitrCache addresses, which goes
            // to memory when an address is displaced and at the end of the key
            bool held = false;
#pragma unroll
            for (int c = 0; c < kBsitrCache; c++)
              if (ca[c] == a0 && cc[c]) {
                cc[c] += n;
                held = true;
              }
            if (!held) {
#pragma unroll
              for (int c = 0; c < kBsitrCache; c++)
                if (c == rr) {
                  if (cc[c] && lane == 0) atomicAdd(&p.tab[ca[c]], cc[c]);
                  ca[c] = a0;
                  cc[c] = n;
                }
              rr = (rr + 1) % kBsitrCache;
            }
            rem &= ~same;
            if (mine) act = false;
          }
          if (act) atomicAdd(&p.tab[idx], 1u);
        } else if (MODE == 4) {
          if (on) {
            const uint32_t f = p.fidx[p.rkoff[v[i] >> 16]];
            if (f != 0xFFFFFFFFu) {
              const uint64_t rk = p.rank[key] + before + (uint32_t)__popc(fw & ((1u << i) - 1u));
              const uint32_t b = (uint32_t)(rk / p.batch_size);
              if (b < p.n_batches)
                atomicOr(&p.bits[((size_t)f * p.n_batches + b) * 2048u + ((v[i] & 0xFFFFu) >> 5)], 1u << (v[i] & 31u));
            }
          }
        } else {
          bool hit = on;
          if (MODE == 2 && on) hit = p.isfull[p.rkoff[v[i] >> 16]] != 0;
          const uint64_t m = __ballot(hit);
          if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(p.n_pairs, (unsigned long long)__popcll(m));
            base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), leader) << 32) |
                   (unsigned long long)(uint32_t)__shfl((int)(uint32_t)base, leader);
            const unsigned long long at = base + (unsigned long long)__popcll(m & below);
            if (hit && at < p.cap) {
              if (MODE == 2)
                p.out_rank[at] = (uint32_t)(p.rank[key] + before + (uint32_t)__popc(fw & ((1u << i) - 1u)));
              p.out_val[at] = v[i];
            }
          }
        }
      }
    }
    if (MODE == 2 || MODE == 4) before += (uint32_t)__popc(fw);
  }
  if (MODE == 1) {
#pragma unroll
    for (int c = 0; c < kBsitrCache; c++)
      if (cc[c] && lane == 0) atomicAdd(&p.tab[ca[c]], cc[c]);
  }
}

// grid (16, keys of the pass): workgroup (c, kl) turns counts [4096 c, 4096 c + 4096) of key k_lo + kl into
// 64 words of each of the key's m cells (cell 0: count != 0; cell 1 + i: bit i of the count)
__global__ __launch_bounds__(256) void k_bsitr_cells(const uint32_t* __restrict__ tab, uint32_t k_lo, int m,
                                                    uint64_t* __restrict__ cells, int stats, uint32_t* __restrict__ mm,
                                                    uint32_t* __restrict__ kcard, uint8_t* __restrict__ isfull,
                                                    unsigned long long* __restrict__ n_full) {
  __shared__ uint64_t st[kBsiMaxInputs][64];
  __shared__ uint32_t red[3][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t c = blockIdx.x, kl = blockIdx.y;
  const uint32_t* T = tab + (size_t)kl * 65536u + 4096u * c + 1024u * (uint32_t)w + (uint32_t)lane;
  uint32_t cnt[16];
#pragma unroll
  for (int s = 0; s < 16; s++) cnt[s] = T[64 * s];
  uint32_t mn = 0xFFFFFFFFu, mx = 0, card = 0;
#pragma unroll
  for (int s = 0; s < 16; s++) {  // unrolled: cnt[] stays in registers
    const uint32_t x = cnt[s];
    const uint64_t nz = __ballot(x != 0);
    uint64_t mine = 0;
    if (nz) {  // wave-uniform
      if (lane == 0) mine = nz;
      for (int i = 1; i < m; i++) {
        const uint64_t b = __ballot((x >> (i - 1)) & 1u);
        if (lane == i) mine = b;
      }
      if (x) {
        mn = min(mn, x);
        mx = max(mx, x);
      }
      card += (uint32_t)__popcll(nz);
    }
    if (lane < m) st[lane][16 * w + s] = mine;
  }
  __syncthreads();
  uint64_t* out = cells + (size_t)kl * (size_t)m * 1024u + 64u * c;
  for (int e = t; e < 64 * m; e += 256) out[(size_t)(e >> 6) * 1024u + (size_t)(e & 63)] = st[e >> 6][e & 63];
  if (!stats) return;
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, d));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
  }
  if (lane == 0) {
    red[0][w] = mn;
    red[1][w] = mx;
    red[2][w] = card;  // wave-uniform already
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t n = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    if (n) {
      atomicMin(&mm[0], min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3])));
      atomicMax(&mm[1], max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
      const uint32_t old = atomicAdd(&kcard[k_lo + kl], n);
      if (old + n == 65536u) {  // the workgroup that completes the key
        isfull[k_lo + kl] = 1;
        atomicAdd(n_full, 1ull);
      }
    }
  }
}

void launch_bsitr_sweep(hipStream_t s, int mode, BsiValArgs a, int has_found, const uint16_t* ckeys,
                        const unsigned long long* n_ckeys, uint32_t grid, BsiTrSweep p) {
  if (!grid) return;
  if (mode == 0) hipLaunchKernelGGL(k_bsitr_sweep<0>, dim3(grid), dim3(256), 0, s, a, has_found, ckeys, n_ckeys, p);
  else if (mode == 1) hipLaunchKernelGGL(k_bsitr_sweep<1>, dim3(grid), dim3(256), 0, s, a, has_found, ckeys, n_ckeys, p);
  else if (mode == 2) hipLaunchKernelGGL(k_bsitr_sweep<2>, dim3(grid), dim3(256), 0, s, a, has_found, ckeys, n_ckeys, p);
  else if (mode == 3) hipLaunchKernelGGL(k_bsitr_sweep<3>, dim3(grid), dim3(256), 0, s, a, has_found, ckeys, n_ckeys, p);
  else hipLaunchKernelGGL(k_bsitr_sweep<4>, dim3(grid), dim3(256), 0, s, a, has_found, ckeys, n_ckeys, p);
}

// One workgroup per full result key: its batches in order, d = the distinct values of the key in the batch, U = the
// union so far (a thread keeps 8 words of it); batches that bring no value do not count.  RunContainer.full() iff
// some contributing batch t >= 2 has U == 65536 and d > 4096.
__global__ __launch_bounds__(256) void k_bsitr_full_runs(const uint32_t* __restrict__ bits, uint32_t n_batches,
                                                        const uint32_t* __restrict__ fki, uint8_t* __restrict__ run) {
  __shared__ int red[2][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint32_t u[8];
#pragma unroll
  for (int k = 0; k < 8; k++) u[k] = 0;
  uint32_t contributing = 0, is_run = 0;
  for (uint32_t j = 0; j < n_batches; j++) {
    const uint4* src = reinterpret_cast<const uint4*>(bits + ((size_t)blockIdx.x * n_batches + j) * 2048u) + 2 * t;
    const uint4 x0 = src[0], x1 = src[1];
    const uint32_t x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    int d = 0, un = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      d += __popc(x[k]);
      u[k] |= x[k];
      un += __popc(u[k]);
    }
    const int ds = wave_sum_i(d), us = wave_sum_i(un);
    if (lane == 0) {
      red[0][w] = ds;
      red[1][w] = us;
    }
    __syncthreads();
    const int D = red[0][0] + red[0][1] + red[0][2] + red[0][3], U = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    __syncthreads();  // red is written again in the next batch
    if (D > 0) {
      contributing++;
      if (contributing >= 2 && U == 65536 && D > 4096) is_run = 1;
    }
  }
  if (t == 0) run[fki[blockIdx.x]] = (uint8_t)is_run;
}

void launch_bsitr_full_runs(hipStream_t s, const uint32_t* bits, uint32_t n_full, uint32_t n_batches,
                            const uint32_t* fki, uint8_t* run) {
  if (!n_full) return;
  hipLaunchKernelGGL(k_bsitr_full_runs, dim3(n_full), dim3(256), 0, s, bits, n_batches, fki, run);
}

size_t bsitr_sort_temp_bytes(uint64_t n) {
  size_t a = 0, b = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 32,
                                          (hipStream_t)0);
  (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr,
                                              (unsigned long long*)nullptr, (int)n, (hipStream_t)0);
  return std::max(a, b) + 256;
}

int launch_bsitr_sort_rle(hipStream_t s, void* temp, size_t temp_bytes, const uint32_t* vals, uint32_t* sorted,
                          uint32_t* uniq, int32_t* counts, unsigned long long* n_out, uint64_t n) {
  hipError_t e = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, vals, sorted, (int)n, 0, 32, s);
  if (e != hipSuccess) return (int)e;
  return (int)hipcub::DeviceRunLengthEncode::Encode(temp, temp_bytes, (const uint32_t*)sorted, uniq, counts, n_out, (int)n,
                                                    s);
}

void launch_bsitr_cells(hipStream_t s, const uint32_t* tab, uint32_t k_lo, uint32_t k_hi, int m, uint8_t* cells,
                        bool stats, uint32_t* mm, uint32_t* kcard, uint8_t* isfull, unsigned long long* n_full) {
  if (k_hi <= k_lo) return;
  hipLaunchKernelGGL(k_bsitr_cells, dim3(16, k_hi - k_lo), dim3(256), 0, s, tab, k_lo, m,
                     reinterpret_cast<uint64_t*>(cells), stats ? 1 : 0, mm, kcard, isfull, n_full);
}

}  // namespace rbg
