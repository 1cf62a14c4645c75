// Host AddressSanitizer / UBSan driver of the range-encoded index's format layer
// (roaringbitmap_amd/csrc/rangebitmap_format.cpp): every stream given on the command line, every truncation of
// it (all of them up to 4 KiB, then a stride), and seeded byte mutations go through rb_parse, and whatever
// parses goes through rb_relay into an arena of exactly the announced size.  Every input lives in a heap block
// of exactly its length, so a read past the end is a sanitizer report.  Prints "<n> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../roaringbitmap_amd/csrc/rangebitmap_format.hpp"

using namespace rbg;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t x = (g_state += 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

static long g_fail = 0, g_ok = 0, g_trunc = 0, g_invalid = 0;

// status of one input; the directory's invariants are checked for whatever parses
static int run(const uint8_t* src, size_t n) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(exact.get(), src, n);
  RbIndex idx;
  std::string err;
  const int st = rb_parse(exact.get(), n, &idx, &err);
  if (st == 0) {
    g_ok++;
    uint64_t arena = 0;
    for (const RbEntry& e : idx.dir) {
      if (e.kind == kRbAbsent) continue;
      const uint64_t len = e.kind == 1 ? 8192 : e.kind == 2 ? 4ull * e.nruns : 2ull * e.card;
      const uint64_t slot = e.kind == 1 ? 8192 : e.kind == 2 ? (4 + len + 15) & ~15ull : (len + 15) & ~15ull;
      if (e.src + len > n || e.slot != arena || (e.slot & 15)) g_fail++;
      arena += slot;
    }
    if (arena != idx.arena_bytes || idx.stream_bytes > n || idx.dir.size() != (size_t)idx.n_blocks * idx.nslices ||
        idx.nslices < 1 || idx.nslices > 64 || ((idx.max_rid + 0xFFFF) >> 16) != idx.n_blocks)
      g_fail++;
    std::unique_ptr<uint8_t[]> out(new uint8_t[idx.arena_bytes ? idx.arena_bytes : 1]());
    rb_relay(exact.get(), idx, out.get());
  } else if (st == -2) {
    g_trunc++;
  } else if (st == -1) {
    g_invalid++;
    if (err.empty()) g_fail++;
  } else {
    g_fail++;
  }
  return st;
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
    if (run(buf.data(), n) != 0) {  // the inputs are valid streams
      std::printf("%s does not parse\n", argv[a]);
      g_fail++;
    }
    // a valid stream cut anywhere is truncated, never anything else
    for (size_t cut = 0; cut < n; cut += (cut < 4096 ? 1 : 997))
      if (run(buf.data(), cut) != -2) g_fail++;
    // mutations: one to three bytes, half of them in the header, the masks and the first records
    for (int m = 0; m < 1500; m++) {
      std::vector<uint8_t> mut(buf);
      const int k = 1 + (int)(rnd() % 3);
      for (int i = 0; i < k; i++) {
        const size_t span = (rnd() & 1) ? (n < 64 ? n : 64) : n;
        if (span) mut[rnd() % span] = (uint8_t)rnd();
      }
      const size_t len = (rnd() % 4 == 0 && n) ? rnd() % n : n;
      run(mut.data(), len);
    }
  }
  // pure noise behind a good header
  for (int m = 0; m < 500; m++) {
    std::vector<uint8_t> noise(10 + rnd() % 300);
    for (uint8_t& b : noise) b = (uint8_t)rnd();
    noise[0] = 0x0D;
    noise[1] = 0xF0;
    noise[2] = 2;
    if (m & 1) noise[3] = (uint8_t)(1 + rnd() % 64);
    run(noise.data(), noise.size());
  }
  run(nullptr, 0);
  std::printf("%ld parsed, %ld truncated, %ld invalid\n%ld failures\n", g_ok, g_trunc, g_invalid, g_fail);
  return g_fail ? 1 : 0;
}
