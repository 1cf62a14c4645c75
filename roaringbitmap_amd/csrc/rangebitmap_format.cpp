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

}  // namespace rbg
