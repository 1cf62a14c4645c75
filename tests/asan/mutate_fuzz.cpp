// Host AddressSanitizer / UBSan driver of the host form of the point mutations
// (roaringbitmap_amd/csrc/mutate_host.cpp over format.cpp): every bitmap given on the command line, and
// truncated copies of it, take random and hand-made batches of adds and of removes through
// rbg_mutate_values_host.  Every input lives in a heap block of exactly its length, so a read past the end is
// a sanitizer report.  Whatever comes out must parse; for the well-formed bitmaps (file names starting with
// "bitmapwith") the cardinalities must also add up: |card' - card| == changed, adding twice changes nothing
// the second time, and removing what was added to an empty bitmap empties it.  Prints "<n> failures".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/roaring_mi355x.h"
#include "../../roaringbitmap_amd/csrc/format.hpp"

using namespace rbg;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t x = (g_state += 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

static long g_fail = 0, g_ok = 0, g_refused = 0;

static void fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  g_fail++;
}

// one call on exact-length copies of the input and the values; -> status, the result in *res
static int call(const uint8_t* src, size_t n, int op, const std::vector<uint32_t>& v, std::vector<uint8_t>* res,
                uint64_t* changed) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(exact.get(), src, n);
  std::unique_ptr<uint32_t[]> vals(new uint32_t[v.size() ? v.size() : 1]);
  if (!v.empty()) std::memcpy(vals.get(), v.data(), 4 * v.size());
  rbg_buffer out{nullptr, 0};
  *changed = ~0ull;
  const int st = rbg_mutate_values_host(exact.get(), n, op, v.empty() ? nullptr : vals.get(), v.size(), &out, changed);
  res->clear();
  if (st == 0) {
    g_ok++;
    res->assign(out.data, out.data + out.len);
    std::free(out.data);
    HostBitmap hb;
    std::string err;
    if (parse(res->data(), res->size(), &hb, &err) != 0 || hb.consumed != res->size()) fail("the result does not parse");
  } else if (st == -1 || st == -2) {
    g_refused++;
    if (out.data) fail("a refused call left a buffer");
  } else {
    fail("unexpected status");
  }
  return st;
}

static int64_t card_of(const std::vector<uint8_t>& b) {
  HostBitmap hb;
  std::string err;
  return parse(b.data(), b.size(), &hb, &err) == 0 ? hb.card : -1;
}

// batches for a bitmap whose keys are `keys`: scattered, clustered into present keys, the ends of a key, and
// the bitmap's own values and their neighbours
static std::vector<std::vector<uint32_t>> batches(const uint8_t* src, size_t n) {
  std::vector<std::vector<uint32_t>> out;
  out.push_back({});
  out.push_back({0u, 0xFFFFFFFFu, 0xFFFFu, 0x10000u, 0xFFFF0000u});
  std::vector<uint32_t> own;
  std::string err;
  if (values_of_serialized(src, n, &own, &err) != 0) own.clear();
  std::vector<uint32_t> v;
  for (int i = 0; i < 3000; i++) v.push_back((uint32_t)rnd());
  out.push_back(v);
  v.clear();
  for (int i = 0; i < 5000; i++) v.push_back((uint32_t)(rnd() % (40u << 16)));
  out.push_back(v);
  if (!own.empty()) {
    v.clear();
    for (int i = 0; i < 4000; i++) {
      const uint32_t x = own[rnd() % own.size()];
      v.push_back(x + (uint32_t)(rnd() % 3) - 1u);  // a value, or a neighbour: run ends, splits, joins
    }
    out.push_back(v);
    v.assign(own.begin(), own.begin() + (own.size() < 200000 ? own.size() : 200000));  // empties whole containers
    out.push_back(v);
    const uint32_t key = own[rnd() % own.size()] & 0xFFFF0000u;
    v.clear();
    for (uint32_t x = 0; x < 65536; x++) v.push_back(key | x);  // one whole key
    out.push_back(v);
  }
  return out;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::printf("cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> buf;
    uint8_t tmp[65536];
    size_t got;
    while ((got = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    std::fclose(f);
    const size_t n = buf.size();
    const char* base = std::strrchr(argv[a], '/');
    base = base ? base + 1 : argv[a];
    const bool good = std::strncmp(base, "bitmapwith", 10) == 0;
    const std::vector<std::vector<uint32_t>> bs = batches(buf.data(), n);
    std::vector<uint8_t> r1, r2;
    uint64_t c1, c2;
    for (const std::vector<uint32_t>& v : bs)
      for (int op = 0; op < 2; op++) {
        const int st = call(buf.data(), n, op, v, &r1, &c1);
        if (!good) continue;
        if (st != 0) {
          fail("a well-formed bitmap was refused");
          continue;
        }
        const int64_t before = card_of(buf), after = card_of(r1);
        if ((op == 0 ? after - before : before - after) != (int64_t)c1) fail("changed does not match the cardinalities");
        if (call(r1.data(), r1.size(), op, v, &r2, &c2) != 0 || c2 != 0 || r2 != r1) fail("the same batch twice");
      }
    // truncated copies: a stride through the file, every length near its start
    for (size_t cut = 0; cut < n; cut += (cut < 64 ? 1 : 1 + n / 97))
      for (int op = 0; op < 2; op++) call(buf.data(), cut, op, bs[2], &r1, &c1);
  }
  // from the empty bitmap: add, then remove the same values
  {
    const uint8_t empty[8] = {0x3A, 0x30, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> v;
    for (int i = 0; i < 20000; i++) v.push_back((uint32_t)(rnd() % (3u << 16)));
    std::vector<uint8_t> r1, r2;
    uint64_t c1, c2;
    if (call(empty, 8, 0, v, &r1, &c1) != 0 || card_of(r1) != (int64_t)c1) fail("add into the empty bitmap");
    if (call(r1.data(), r1.size(), 1, v, &r2, &c2) != 0 || c2 != c1 || r2 != std::vector<uint8_t>(empty, empty + 8))
      fail("removing what was added");
    rbg_buffer out{nullptr, 0};
    uint64_t ch;
    if (rbg_mutate_values_host(empty, 8, 2, v.data(), v.size(), &out, &ch) != -3) fail("op 2 is refused");
    if (rbg_mutate_values_host(empty, 8, 0, nullptr, 5, &out, &ch) != -3) fail("null values are refused");
    if (rbg_mutate_values_host(empty, 8, 0, v.data(), v.size(), nullptr, &ch) != -3) fail("a null out is refused");
    if (rbg_mutate_values_host(empty, 8, 0, v.data(), v.size(), &out, nullptr) != -3) fail("a null changed is refused");
  }
  std::printf("%ld results, %ld refused inputs\n%ld failures\n", g_ok, g_refused, g_fail);
  return g_fail ? 1 : 0;
}
