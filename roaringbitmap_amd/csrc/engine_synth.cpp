// The bench workload synthesizers (engine.hpp: the host units): batches C2 .. C5 generated on the device
// (synth.hip), and the per-key byte counts of the C3 workloads.
#include <algorithm>

#include "engine.hpp"

namespace rbg {

// C2: one bitmap of 65536 containers (kind 0: the mix; 16 + DK_A/DK_B/DK_R: the same generator with one
// container family)
int synth_c2(Ctx* c, int kind, uint64_t seed, int32_t* out_id) {
  const int32_t id = new_batch(c);
  Batch& b = *c->batches[id];
  const size_t C = kMaxKeys;
  b.n_bm = 1;
  b.n_ctr = C;
  b.key_major = true;
  b.payload_bytes = (size_t)kSlotBytes * C;
  CHK(b.keys.ensure(2 * C + 16));
  CHK(b.desc.ensure(sizeof(CDesc) * C + 16));
  CHK(b.bm.ensure(4 * C + 16));
  CHK(b.key_off.ensure(4 * (kMaxKeys + 1)));
  CHK(b.bm_off.ensure(8));
  CHK(b.payload.ensure(b.payload_bytes + 64));
  std::vector<uint32_t> key_off(kMaxKeys + 1);
  for (int k = 0; k <= kMaxKeys; k++) key_off[k] = (uint32_t)k;
  b.h_bm_off = {0u, (uint32_t)C};
  b.h_bm_nctr = {(uint32_t)C};
  hipStream_t s = c->stream;
  HIPCHK(hipMemsetAsync(b.bm.p, 0, 4 * C, s));
  HIPCHK(hipMemcpyAsync(b.key_off.p, key_off.data(), 4 * (kMaxKeys + 1), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b.bm_off.p, b.h_bm_off.data(), 8, hipMemcpyHostToDevice, s));
  launch_synth_c2(s, seed, kind == 0 ? -1 : kind - 16, b.desc.as<CDesc>(), b.keys.as<uint16_t>(), b.payload.as<uint8_t>());
  HIPCHK(hipGetLastError());
  std::vector<CDesc> d(C);
  HIPCHK(hipMemcpyAsync(d.data(), b.desc.p, sizeof(CDesc) * C, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int64_t card = 0;
  for (const CDesc& x : d) {
    b.n_kind[x.kind]++;
    card += x.card;
  }
  b.long_card = card;
  b.h_bm_card = {card};
  b.ser_bytes = 0;
  b.live = true;
  *out_id = id;
  return RBG_OK;
}

// C3 synthetic key slice [key_lo, key_hi) of n bitmaps (kind 1 uniform, 2 clustered)
int synth_c3(Ctx* c, int kind, uint64_t seed, size_t n, int key_lo, int key_hi, int32_t* out_id) {
  key_lo = std::max(0, key_lo);
  key_hi = std::min(kMaxKeys, key_hi);
  if (n == 0 || n > 0x7FFFFFFF || key_hi < key_lo) {
    set_err("synthetic C3 needs 0 < n and key_lo <= key_hi");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  const int nkeys = key_hi - key_lo;
  hipStream_t s = c->stream;
  std::vector<uint32_t> key_off(kMaxKeys + 1, 0);
  std::vector<uint16_t> h_keys;
  std::vector<uint32_t> h_bm, nctr(n, 0);
  if (kind == 1) {
    for (int k = 0; k < kMaxKeys; k++) {
      const bool in = k >= key_lo && k < key_hi;
      key_off[k + 1] = key_off[k] + (in ? (uint32_t)n : 0u);
    }
    for (size_t i = 0; i < n; i++) nctr[i] = (uint32_t)nkeys;
  } else {
    std::vector<uint32_t> base(n);
    for (size_t i = 0; i < n; i++) {
      base[i] = c3c_base(seed, (uint32_t)i);
      for (uint32_t k = base[i]; k < base[i] + 16; k++)
        if ((int)k >= key_lo && (int)k < key_hi) {
          key_off[k + 1]++;
          nctr[i]++;
        }
    }
    for (int k = 0; k < kMaxKeys; k++) key_off[k + 1] += key_off[k];
    h_keys.resize(key_off[kMaxKeys]);
    h_bm.resize(key_off[kMaxKeys]);
    std::vector<uint32_t> cur(key_off.begin(), key_off.end() - 1);
    for (size_t i = 0; i < n; i++)  // ascending i: input order within each key
      for (uint32_t k = base[i]; k < base[i] + 16; k++)
        if ((int)k >= key_lo && (int)k < key_hi) {
          h_keys[cur[k]] = (uint16_t)k;
          h_bm[cur[k]++] = (uint32_t)i;
        }
  }
  const size_t C = key_off[kMaxKeys];
  const int32_t id = new_batch(c);
  Batch& b = *c->batches[id];
  b.n_bm = n;
  b.n_ctr = C;
  b.key_major = true;
  b.h_bm_nctr = nctr;
  b.h_bm_card.assign(n, 0);
  CHK(b.keys.ensure(2 * C + 16));
  CHK(b.desc.ensure(sizeof(CDesc) * C + 16));
  CHK(b.bm.ensure(4 * C + 16));
  CHK(b.key_off.ensure(4 * (kMaxKeys + 1)));
  CHK(b.bm_off.ensure(8));
  HIPCHK(hipMemcpyAsync(b.key_off.p, key_off.data(), 4 * (kMaxKeys + 1), hipMemcpyHostToDevice, s));
  if (kind == 1) {
    CHK(main_set(c));  // set 0's scratch is borrowed
    CHK(c->r().scratch.ensure(16 * (size_t)kMaxKeys));
    unsigned long long* kb = c->r().scratch.as<unsigned long long>();
    launch_synth_c3u(s, seed, (uint32_t)n, key_lo, nkeys, kb, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    std::vector<unsigned long long> bytes(nkeys + 1, 0);
    if (nkeys) HIPCHK(hipMemcpyAsync(bytes.data(), kb, 8 * nkeys, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    unsigned long long tot = 0;
    for (int k = 0; k < nkeys; k++) {
      const unsigned long long x = bytes[k];
      bytes[k] = tot;
      tot += x;
    }
    b.payload_bytes = tot;
    CHK(b.payload.ensure(tot + 64));
    HIPCHK(hipMemcpyAsync(kb, bytes.data(), 8 * std::max(nkeys, 1), hipMemcpyHostToDevice, s));
    launch_synth_c3u(s, seed, (uint32_t)n, key_lo, nkeys, nullptr, kb, b.desc.as<CDesc>(), b.keys.as<uint16_t>(),
                     b.bm.as<uint32_t>(), b.payload.as<uint8_t>(), 1);
    b.n_kind[DK_A] = (int64_t)C;
    b.packed = true;
  } else {
    b.payload_bytes = 8192 * C;
    CHK(b.payload.ensure(b.payload_bytes + 64));
    if (C) {
      HIPCHK(hipMemcpyAsync(b.keys.p, h_keys.data(), 2 * C, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(b.bm.p, h_bm.data(), 4 * C, hipMemcpyHostToDevice, s));
    }
    launch_synth_c3c(s, seed, C, b.keys.as<uint16_t>(), b.bm.as<uint32_t>(), b.desc.as<CDesc>(),
                     b.payload.as<uint8_t>());
    b.n_kind[DK_B] = (int64_t)C;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(c->scalar.p, 0, 8, s));
  launch_sum_cards(s, b.desc.as<CDesc>(), C, c->scalar.as<unsigned long long>());
  unsigned long long card = 0;
  HIPCHK(hipMemcpyAsync(&card, c->scalar.p, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  b.long_card = (int64_t)card;
  b.ser_bytes = 0;
  b.live = true;
  *out_id = id;
  return RBG_OK;
}

// C4: n pairs = 2n small bitmaps, bitmap-major (pairs adjacent).  Each bitmap has
// K in [1,4] keys from [0,64), each an array container of card in [16,512].
int synth_c4(Ctx* c, uint64_t seed, size_t n_pairs, int32_t* out_id) {
  const size_t nb = 2 * n_pairs;
  if (nb == 0 || nb > 0x7FFFFFFF) return RBG_ERR_ILLEGAL_ARGUMENT;
  const int32_t id = new_batch(c);
  Batch& b = *c->batches[id];
  b.n_bm = nb;
  b.key_major = false;
  b.h_bm_off.assign(nb + 1, 0);
  b.h_bm_nctr.resize(nb);
  b.h_bm_card.resize(nb);
  std::vector<CDesc> d;
  d.reserve(nb * 5 / 2 + 16);
  uint64_t off = 0;
  for (size_t j = 0; j < nb; j++) {
    const uint64_t h = splitmix64(seed ^ (0xC4000000ULL + j));
    const int K = 1 + (int)(h % 4);
    uint64_t used = 0;
    int got = 0;
    for (uint64_t t = 1; got < K; t++) {
      const int k = (int)(splitmix64(h + t) & 63);
      if (!((used >> k) & 1)) {
        used |= 1ULL << k;
        got++;
      }
    }
    int64_t card_sum = 0;
    for (int k = 0; k < 64; k++)
      if ((used >> k) & 1) {
        const uint32_t card = 16 + (uint32_t)(splitmix64(h ^ ((uint64_t)k << 40)) % 497);
        d.push_back(CDesc{off, card, (uint16_t)k, DK_A, 0});
        off += (2 * card + 15) & ~15ull;
        card_sum += card;
      }
    b.h_bm_nctr[j] = (uint32_t)K;
    b.h_bm_off[j + 1] = b.h_bm_off[j] + (uint32_t)K;
    b.h_bm_card[j] = card_sum;
    b.long_card += card_sum;
  }
  const size_t C = d.size();
  b.n_ctr = C;
  b.n_kind[DK_A] = (int64_t)C;
  b.payload_bytes = off;
  CHK(b.desc.ensure(sizeof(CDesc) * C + 16));
  CHK(b.keys.ensure(2 * C + 16));
  CHK(b.bm.ensure(4 * C + 16));
  CHK(b.bm_off.ensure(4 * (nb + 1)));
  CHK(b.payload.ensure(off + 64));
  hipStream_t s = c->stream;
  std::vector<uint16_t> hk(C);
  std::vector<uint32_t> hbm(C);
  for (size_t j = 0; j < nb; j++)
    for (uint32_t p = b.h_bm_off[j]; p < b.h_bm_off[j + 1]; p++) {
      hk[p] = d[p].key;
      hbm[p] = (uint32_t)j;
    }
  HIPCHK(hipMemcpyAsync(b.desc.p, d.data(), sizeof(CDesc) * C, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b.keys.p, hk.data(), 2 * C, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b.bm.p, hbm.data(), 4 * C, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b.bm_off.p, b.h_bm_off.data(), 4 * (nb + 1), hipMemcpyHostToDevice, s));
  launch_synth_arrays(s, seed, b.desc.as<CDesc>(), C, b.payload.as<uint8_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  b.live = true;
  *out_id = id;
  return RBG_OK;
}

// C5: a bit-sliced index over rows 0..rows-1 with 31 slices, as the key-major batch
// [ebM, bA[0..30]] of rbg_ctx_bsi; the value min / max go to b.bsi_min / bsi_max
int synth_c5(Ctx* c, uint64_t seed, size_t rows, int key_lo, int key_hi, int32_t* out_id) {
  const int nbits = 31, nin = nbits + 1;
  if (rows == 0 || rows > (1ull << 32)) return RBG_ERR_ILLEGAL_ARGUMENT;
  key_lo = std::max(0, key_lo);
  key_hi = (int)std::min<uint64_t>((uint64_t)std::min(key_hi, kMaxKeys), (rows + 65535) / 65536);
  const int nkeys = std::max(0, key_hi - key_lo);
  hipStream_t s = c->stream;
  const size_t G = (size_t)nkeys * nin;
  CHK(main_set(c));  // set 0's scratch is borrowed
  CHK(c->r().scratch.ensure(8 * G + 64));
  uint32_t* cards = c->r().scratch.as<uint32_t>();
  uint32_t* pos = cards + G;
  unsigned int* mm = reinterpret_cast<unsigned int*>(c->scalar.p);
  const unsigned int mm0[2] = {0xFFFFFFFFu, 0u};
  HIPCHK(hipMemcpyAsync(mm, mm0, 8, hipMemcpyHostToDevice, s));
  launch_synth_c5(s, seed, rows, key_lo, nbits, nkeys, 0, cards, nullptr, mm, nullptr, nullptr, nullptr, nullptr);
  std::vector<uint32_t> h(G);
  unsigned int mmh[2];
  HIPCHK(hipMemcpyAsync(h.data(), cards, 4 * G, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(mmh, mm, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<uint32_t> key_off(kMaxKeys + 1, 0), hp(G, 0);
  uint32_t C = 0;
  for (int k = 0; k < kMaxKeys; k++) {
    const int j = k - key_lo;
    if (j >= 0 && j < nkeys)
      for (int i = 0; i < nin; i++)
        if (h[(size_t)j * nin + i]) hp[(size_t)j * nin + i] = C++;
    key_off[k + 1] = C;
  }
  const int32_t id = new_batch(c);
  Batch& b = *c->batches[id];
  b.n_bm = nin;
  b.n_ctr = C;
  b.key_major = true;
  b.payload_bytes = (size_t)kSlotBytes * C;
  b.h_bm_nctr.assign(nin, 0);
  b.h_bm_card.assign(nin, 0);
  for (int k = 0; k < nkeys; k++)
    for (int i = 0; i < nin; i++)
      if (h[(size_t)k * nin + i]) {
        b.h_bm_nctr[i]++;
        b.h_bm_card[i] += h[(size_t)k * nin + i];
      }
  for (int i = 0; i < nin; i++) b.long_card += b.h_bm_card[i];
  CHK(b.keys.ensure(2 * (size_t)C + 16));
  CHK(b.desc.ensure(sizeof(CDesc) * (size_t)C + 16));
  CHK(b.bm.ensure(4 * (size_t)C + 16));
  CHK(b.key_off.ensure(4 * (kMaxKeys + 1)));
  CHK(b.bm_off.ensure(8));
  CHK(b.payload.ensure(b.payload_bytes + 64));
  HIPCHK(hipMemcpyAsync(b.key_off.p, key_off.data(), 4 * (kMaxKeys + 1), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(pos, hp.data(), 4 * G, hipMemcpyHostToDevice, s));
  launch_synth_c5(s, seed, rows, key_lo, nbits, nkeys, 1, nullptr, pos, nullptr, b.desc.as<CDesc>(),
                  b.keys.as<uint16_t>(),
                  b.bm.as<uint32_t>(), b.payload.as<uint8_t>());
  HIPCHK(hipGetLastError());
  std::vector<CDesc> d(C);
  if (C) HIPCHK(hipMemcpyAsync(d.data(), b.desc.p, sizeof(CDesc) * C, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (const CDesc& x : d) b.n_kind[x.kind]++;
  b.bsi_min = (int32_t)mmh[0];
  b.bsi_max = (int32_t)mmh[1];
  b.live = true;
  *out_id = id;
  return RBG_OK;
}

}  // namespace rbg

using namespace rbg;

extern "C" {

int rbg_synth_key_bytes(int kind, uint64_t seed, size_t n, uint64_t* out) {
  if (!out || (kind != 1 && kind != 2)) return RBG_ERR_ILLEGAL_ARGUMENT;
  for (int k = 0; k < kMaxKeys; k++) out[k] = 0;
  for (size_t i = 0; i < n; i++) {
    if (kind == 1) {
      for (int k = 0; k < kMaxKeys; k++) out[k] += 4 + 2 * (uint64_t)c3u_card(seed, (uint32_t)i, (uint32_t)k);
    } else {
      const uint32_t b0 = c3c_base(seed, (uint32_t)i);
      for (uint32_t k = b0; k < b0 + 16; k++) out[k] += 4 + 8192;
    }
  }
  return RBG_OK;
}

}  // extern "C"
