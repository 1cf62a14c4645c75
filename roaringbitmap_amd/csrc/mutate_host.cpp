// rbg_mutate_values_host: a batch of values added to or removed from a serialized bitmap on the host, with no
// device (include/roaring_mi355x_mutate.h: the rule and the Java it replaces).  Host-only: this unit and
// format.cpp are all the stand-alone sanitizer program links.
//
// The values are sorted and made distinct (the result of a batch of adds alone, or of removes alone, does not
// depend on order or duplicates); then one walk over the operand's containers and the values' keys.  A key
// no value touches keeps its payload bytes; a touched one goes through its 65,536-bit set.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/roaring_mi355x.h"
#include "format.hpp"

namespace rbg {
namespace {

struct OutCtr {
  uint16_t key;
  uint8_t kind;
  uint32_t card;
  const uint8_t* src;  // the serialized payload: the operand's bytes or own
  uint32_t len;
  std::vector<uint8_t> own;
};

inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline void wr16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v & 0xFF);
  p[1] = (uint8_t)((v >> 8) & 0xFF);
}
inline void wr32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; i++) p[i] = (uint8_t)((v >> (8 * i)) & 0xFF);
}

// the container's bit set; a run that would pass 65,535 (no valid container has one) is cut there
void expand(const uint8_t* buf, const HostCtr& c, uint64_t* w) {
  const uint8_t* q = buf + c.ser_off;
  std::memset(w, 0, 8192);
  if (c.kind == KA) {
    for (uint32_t i = 0; i < c.card; i++) {
      const uint32_t x = rd16(q + 2 * i);
      w[x >> 6] |= 1ull << (x & 63);
    }
  } else if (c.kind == KB) {
    for (int i = 0; i < 1024; i++) {
      uint64_t x = 0;
      for (int j = 0; j < 8; j++) x |= (uint64_t)q[8 * i + j] << (8 * j);
      w[i] = x;
    }
  } else {
    for (uint32_t r = 0; r < c.nruns; r++) {
      const uint32_t s = rd16(q + 2 + 4 * r), e = std::min<uint32_t>(s + rd16(q + 4 + 4 * r), 65535u);
      for (uint32_t x = s; x <= e; x++) w[x >> 6] |= 1ull << (x & 63);
    }
  }
}

uint32_t card_of(const uint64_t* w) {
  uint32_t c = 0;
  for (int i = 0; i < 1024; i++) c += (uint32_t)__builtin_popcountll(w[i]);
  return c;
}

// the payload of the bit set as a container of `kind` (card >= 1)
void encode(const uint64_t* w, int kind, uint32_t card, std::vector<uint8_t>* out) {
  if (kind == KB) {
    out->resize(8192);
    for (int i = 0; i < 1024; i++)
      for (int j = 0; j < 8; j++) (*out)[8 * i + j] = (uint8_t)(w[i] >> (8 * j));
    return;
  }
  if (kind == KA) {
    out->resize(2 * (size_t)card);
    size_t p = 0;
    for (int i = 0; i < 1024; i++)
      for (uint64_t x = w[i]; x; x &= x - 1, p += 2) wr16(out->data() + p, (uint32_t)(64 * i + __builtin_ctzll(x)));
    return;
  }
  out->assign(2, 0);  // the maximal runs of the set, (start, length - 1)
  uint32_t nr = 0;
  int start = -1;
  for (int x = 0; x <= 65536; x++) {
    const bool on = x < 65536 && ((w[x >> 6] >> (x & 63)) & 1);
    if (on && start < 0) start = x;
    if (!on && start >= 0) {
      const size_t p = out->size();
      out->resize(p + 4);
      wr16(out->data() + p, (uint32_t)start);
      wr16(out->data() + p + 2, (uint32_t)(x - 1 - start));
      nr++;
      start = -1;
    }
  }
  wr16(out->data(), nr);
}

}  // namespace

static int mutate_values_host(const uint8_t* buf, size_t len, int op, const uint32_t* values, size_t n,
                              std::vector<uint8_t>* out, uint64_t* changed, std::string* err) {
  HostBitmap hb;
  const int st = parse(buf, len, &hb, err);
  if (st) return st;
  std::vector<uint32_t> v(values, values + n);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  std::vector<OutCtr> cs;
  cs.reserve(hb.ctrs.size() + 16);
  std::vector<uint64_t> w(1024);
  uint64_t delta = 0;
  size_t ci = 0, vi = 0;
  while (ci < hb.ctrs.size() || vi < v.size()) {
    const uint32_t kc = ci < hb.ctrs.size() ? hb.ctrs[ci].key : 0x10000u;
    const uint32_t kv = vi < v.size() ? v[vi] >> 16 : 0x10000u;
    if (kc < kv) {  // untouched
      const HostCtr& c = hb.ctrs[ci++];
      cs.push_back(OutCtr{c.key, c.kind, c.card, buf + c.ser_off, c.ser_len, {}});
      continue;
    }
    size_t ve = vi;
    while (ve < v.size() && (v[ve] >> 16) == kv) ve++;
    if (kv < kc && op == 1) {  // a remove under an absent key
      vi = ve;
      continue;
    }
    const bool present = kc == kv;
    int kind = KA;  // a new key: a fresh ArrayContainer
    uint32_t old = 0;
    if (present) {
      expand(buf, hb.ctrs[ci], w.data());
      old = card_of(w.data());
      kind = hb.ctrs[ci].kind;
      ci++;
    } else {
      std::fill(w.begin(), w.end(), 0ull);
    }
    for (; vi < ve; vi++) {
      const uint32_t x = v[vi] & 0xFFFFu;
      if (op == 0) w[x >> 6] |= 1ull << (x & 63);
      else w[x >> 6] &= ~(1ull << (x & 63));
    }
    const uint32_t card = card_of(w.data());
    delta += card > old ? card - old : old - card;
    if (!card) continue;  // emptied: dropped
    if (kind != KR) kind = card > (uint32_t)kArrayMax ? KB : KA;
    cs.push_back(OutCtr{(uint16_t)kv, (uint8_t)kind, card, nullptr, 0, {}});
    OutCtr& o = cs.back();
    encode(w.data(), kind, card, &o.own);
    o.len = (uint32_t)o.own.size();
  }
  // RB/RoaringArray.java:896-940
  const size_t size = cs.size();
  bool has_run = false;
  size_t total = 0;
  for (const OutCtr& c : cs) {
    has_run |= c.kind == KR;
    total += c.len;
  }
  const size_t head = header_size(size, has_run);
  out->assign(head + total, 0);
  uint8_t* p = out->data();
  size_t pos;
  if (has_run) {
    wr32(p, kCookieRun | (uint32_t)((size - 1) << 16));
    pos = 4;
    for (size_t i = 0; i < size; i++)
      if (cs[i].kind == KR) p[pos + i / 8] |= (uint8_t)(1u << (i % 8));
    pos += (size + 7) / 8;
  } else {
    wr32(p, kCookieNoRun);
    wr32(p + 4, (uint32_t)size);
    pos = 8;
  }
  for (const OutCtr& c : cs) {
    wr16(p + pos, c.key);
    wr16(p + pos + 2, c.card - 1);
    pos += 4;
  }
  if (!has_run || size >= (size_t)kNoOffsetThreshold) {
    uint32_t start = (uint32_t)head;
    for (const OutCtr& c : cs) {
      wr32(p + pos, start);
      pos += 4;
      start += c.len;
    }
  }
  for (const OutCtr& c : cs) {
    if (c.len) std::memcpy(p + pos, c.src ? c.src : c.own.data(), c.len);
    pos += c.len;
  }
  *changed = delta;
  return RBG_OK;
}

}  // namespace rbg

extern "C" int rbg_mutate_values_host(const uint8_t* buf, size_t len, int op, const uint32_t* values, size_t n,
                                      rbg_buffer* out, uint64_t* changed) {
  if (!out || !changed || (op != RBG_MUT_ADD && op != RBG_MUT_REMOVE) || (n && !values) || (!buf && len))
    return RBG_ERR_ILLEGAL_ARGUMENT;
  std::vector<uint8_t> bytes;
  std::string err;
  const int st = rbg::mutate_values_host(buf, len, op, values, n, &bytes, changed, &err);
  if (st) return st;
  uint8_t* p = (uint8_t*)std::malloc(bytes.size() ? bytes.size() : 1);
  if (!p) return RBG_ERR_OUT_OF_MEMORY;
  std::memcpy(p, bytes.data(), bytes.size());
  out->data = p;
  out->len = bytes.size();
  return RBG_OK;
}
