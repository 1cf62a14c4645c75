// Host-side format layer of the range-encoded index (see rangebitmap_format.hpp).
#include "rangebitmap_format.hpp"

#include <cstring>

#include "../../include/roaring_mi355x.h"

namespace rbg {

static inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static inline uint32_t rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

int rb_parse(const uint8_t* p, size_t n, RbIndex* out, std::string* err) {
  *out = RbIndex{};
  auto trunc = [&](const char* what) {
    if (err) *err = std::string("truncated range bitmap: ") + what;
    return RBG_ERR_TRUNCATED;
  };
  auto invalid = [&](const std::string& what) {
    if (err) *err = what;
    return RBG_ERR_INVALID_FORMAT;
  };
  if (!p && n) return RBG_ERR_ILLEGAL_ARGUMENT;
  // the header, each field judged as soon as it is there (map, :65-85)
  if (n < 2) return trunc("cookie");
  const uint32_t cookie = rd16(p);
  if (cookie != kRbCookie)
    return invalid("invalid cookie for range bitmap (expected " + std::to_string(kRbCookie) + " but got " +
                   std::to_string(cookie) + ")");
  if (n < 3) return trunc("base");
  if (p[2] != 2) return invalid("Unsupported base for range bitmap: " + std::to_string((int)p[2]));
  if (n < 4) return trunc("slice count");
  const uint32_t nslices = p[3];
  // rangeMask(maxValue | 1) has 1..64 bits (:1622-1630); the reference would shift by 64 - 0 or past 64
  if (nslices < 1 || nslices > 64) return invalid("range bitmap slice count " + std::to_string(nslices) + " not in 1..64");
  if (n < 10) return trunc("header");
  const uint32_t n_blocks = rd16(p + 4);
  const uint64_t max_rid = rd32(p + 6);
  if ((max_rid + 0xFFFF) >> 16 != n_blocks)
    return invalid("range bitmap of " + std::to_string(max_rid) + " rows in " + std::to_string(n_blocks) + " blocks");
  const size_t bpm = (nslices + 7) >> 3;
  out->nslices = nslices;
  out->n_blocks = n_blocks;
  out->max_rid = max_rid;
  out->mask = ~0ull >> (64 - nslices);
  size_t pos = 10;
  if (n - pos < (size_t)n_blocks * bpm) return trunc("masks");
  out->masks.resize(n_blocks);
  for (uint32_t k = 0; k < n_blocks; k++) {
    uint64_t m = 0;  // exactly bytesPerMask bytes (getContainerMask, :1359-1373, reads 4 or 8 and masks)
    for (size_t j = 0; j < bpm; j++) m |= (uint64_t)p[pos + j] << (8 * j);
    out->masks[k] = m & out->mask;
    pos += bpm;
  }
  out->dir.resize((size_t)n_blocks * nslices);
  uint64_t arena = 0;
  for (uint32_t k = 0; k < n_blocks; k++) {
    for (uint32_t i = 0; i < nslices; i++) {
      if (!((out->masks[k] >> i) & 1)) continue;
      if (n - pos < 3) return trunc("container header");
      const uint8_t type = p[pos];
      const uint32_t size = rd16(p + pos + 1);
      if (type > RBT_ARRAY) return invalid("Unknown type " + std::to_string((int)type));
      pos += 3;
      RbEntry& e = out->dir[(size_t)k * nslices + i];
      uint64_t len, slot;
      if (type == RBT_BITMAP) {
        e.kind = 1;
        e.card = size ? size : 65536;  // (char) cardinality: a full container stores 0 (:1565)
        len = 8192;
        slot = 8192;
      } else if (type == RBT_RUN) {
        e.kind = 2;
        e.nruns = size;
        len = 4ull * size;
        slot = (4 + len + 15) & ~15ull;
      } else {
        e.kind = 0;
        e.card = size;
        len = 2ull * size;
        slot = (len + 15) & ~15ull;
      }
      if (n - pos < len) return trunc("container payload");
      e.src = pos;
      e.slot = arena;
      arena += slot;
      pos += (size_t)len;
      out->payload_bytes += len;
    }
  }
  out->arena_bytes = arena;
  out->stream_bytes = pos;
  return RBG_OK;
}

void rb_relay(const uint8_t* p, const RbIndex& idx, uint8_t* arena) {
  for (const RbEntry& e : idx.dir) {
    if (e.kind == kRbAbsent) continue;
    uint8_t* dst = arena + e.slot;
    if (e.kind == 2) {
      dst[0] = dst[1] = 0;
      dst[2] = (uint8_t)(e.nruns & 0xFF);
      dst[3] = (uint8_t)(e.nruns >> 8);
      if (e.nruns) std::memcpy(dst + 4, p + e.src, 4ull * e.nruns);
    } else if (e.kind == 1) {
      std::memcpy(dst, p + e.src, 8192);
    } else if (e.card) {
      std::memcpy(dst, p + e.src, 2ull * e.card);
    }
  }
}

int rb_emit(const RbIndex& idx, const uint8_t* arena, uint64_t arena_bytes, std::vector<uint8_t>* out, std::string* err) {
  auto invalid = [&](const char* what) {
    if (err) *err = std::string("range bitmap directory: ") + what;
    return RBG_ERR_INVALID_FORMAT;
  };
  out->clear();
  if (idx.nslices < 1 || idx.nslices > 64 || idx.n_blocks > 0xFFFF || idx.max_rid > 0xFFFFFFFFull ||
      (idx.max_rid + 0xFFFF) >> 16 != idx.n_blocks || idx.masks.size() != idx.n_blocks ||
      idx.dir.size() != (size_t)idx.n_blocks * idx.nslices)
    return invalid("the header does not describe it");
  auto put16 = [&](uint32_t v) {
    out->push_back((uint8_t)(v & 0xFF));
    out->push_back((uint8_t)((v >> 8) & 0xFF));
  };
  put16(kRbCookie);
  out->push_back(2);
  out->push_back((uint8_t)idx.nslices);
  put16(idx.n_blocks);
  put16((uint32_t)(idx.max_rid & 0xFFFF));
  put16((uint32_t)(idx.max_rid >> 16));
  const size_t bpm = (idx.nslices + 7) >> 3;
  for (uint64_t m : idx.masks)
    for (size_t j = 0; j < bpm; j++) out->push_back((uint8_t)(m >> (8 * j)));
  for (size_t j = 0; j < idx.dir.size(); j++) {
    const RbEntry& e = idx.dir[j];
    const bool in_mask = (idx.masks[j / idx.nslices] >> (j % idx.nslices)) & 1;
    if (in_mask != (e.kind != kRbAbsent)) return invalid("a mask and its entries disagree");
    if (!in_mask) continue;
    if (e.kind > 2 || (e.slot & 1)) return invalid("an entry of no known kind or an odd slot");
    if (e.slot > arena_bytes) return invalid("a slot outside the arena");
    const uint64_t room = arena_bytes - e.slot;
    const uint8_t* src = arena + e.slot;
    uint64_t len;
    if (e.kind == 1) {
      if (e.card < 1 || e.card > 65536) return invalid("a bitmap's cardinality");
      out->push_back(RBT_BITMAP);
      put16(e.card & 0xFFFF);
      len = 8192;
    } else if (e.kind == 2) {
      if (room < 4) return invalid("a slot outside the arena");
      const uint32_t nruns = rd16(src + 2);
      out->push_back(RBT_RUN);
      put16(nruns);
      len = 4ull * nruns + 4;
    } else {
      if (e.card > 0xFFFF) return invalid("an array's cardinality");
      out->push_back(RBT_ARRAY);
      put16(e.card);
      len = 2ull * e.card;
    }
    if (room < len) return invalid("a slot outside the arena");
    const size_t skip = e.kind == 2 ? 4 : 0;
    out->insert(out->end(), src + skip, src + len);
  }
  return RBG_OK;
}

}  // namespace rbg
