// Host AddressSanitizer / UBSan driver of the range-encoded index's way back to a stream
// (roaringbitmap_amd/csrc/rangebitmap_format.cpp: rb_emit): every stream given on the command line goes through
// rb_parse, rb_relay into an arena of exactly the announced size and rb_emit, and the bytes that come out must be
// the bytes the parser consumed; every truncation of it (all of them up to 4 KiB, then a stride) must be refused
// by the parser and never reach the emitter; directories that do not fit their arena or their header must be
// refused by the emitter.  Every input lives in a heap block of exactly its length, so a read past the end is a
// sanitizer report.  Prints "<n> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../roaringbitmap_amd/csrc/rangebitmap_format.hpp"

using namespace rbg;

static long g_fail = 0, g_ok = 0, g_trunc = 0, g_refused = 0;

static void fail(const char* what, size_t n) {
  std::printf("FAIL %s (input of %zu bytes)\n", what, n);
  g_fail++;
}

// parse, re-lay, emit; -> the parser's status
static int run(const uint8_t* src, size_t n) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(exact.get(), src, n);
  RbIndex idx;
  std::string err;
  const int st = rb_parse(exact.get(), n, &idx, &err);
  if (st != 0) {
    if (st == -2) g_trunc++;
    return st;
  }
  g_ok++;
  std::unique_ptr<uint8_t[]> arena(new uint8_t[idx.arena_bytes ? idx.arena_bytes : 1]());
  rb_relay(exact.get(), idx, arena.get());
  std::vector<uint8_t> out;
  if (rb_emit(idx, arena.get(), idx.arena_bytes, &out, &err) != 0) {
    fail("a parsed stream is not emitted", n);
    return st;
  }
  if (out.size() != idx.stream_bytes || std::memcmp(out.data(), exact.get(), out.size()) != 0)
    fail("the emitted bytes are not the parsed ones", n);
  // what was emitted parses to the same directory
  RbIndex again;
  if (rb_parse(out.data(), out.size(), &again, &err) != 0 || again.arena_bytes != idx.arena_bytes ||
      again.payload_bytes != idx.payload_bytes || again.stream_bytes != out.size())
    fail("the emitted bytes do not parse back", n);
  // a directory that does not fit: an arena cut short, a header that lies, a mask that disagrees
  if (idx.arena_bytes) {
    for (uint64_t cut : {idx.arena_bytes - 1, idx.arena_bytes / 2, (uint64_t)0}) {
      std::unique_ptr<uint8_t[]> small(new uint8_t[cut ? cut : 1]());
      std::memcpy(small.get(), arena.get(), cut);
      // the last slot's padding may be all that is missing: only an arena of nothing is refused for certain,
      // and whatever is emitted is read from inside the exact-size block
      const int es = rb_emit(idx, small.get(), cut, &out, &err);
      if (es == 0 && cut == 0) fail("an arena of nothing is emitted", n);
      else if (es != 0) g_refused++;
    }
  }
  if (idx.n_blocks) {
    RbIndex bad = idx;
    bad.masks[0] ^= 1;
    if (rb_emit(bad, arena.get(), idx.arena_bytes, &out, &err) == 0) fail("a disagreeing mask is emitted", n);
    else g_refused++;
    bad = idx;
    bad.dir.pop_back();
    if (rb_emit(bad, arena.get(), idx.arena_bytes, &out, &err) == 0) fail("a short directory is emitted", n);
    else g_refused++;
  }
  RbIndex bad = idx;
  bad.nslices = 65;
  if (rb_emit(bad, arena.get(), idx.arena_bytes, &out, &err) == 0) fail("65 slices are emitted", n);
  else g_refused++;
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
    RbIndex probe;
    if (rb_parse(buf.data(), buf.size(), &probe, nullptr) != 0) {
      std::printf("%s does not parse\n", argv[a]);
      g_fail++;
      continue;
    }
    run(buf.data(), buf.size());
    // cut anywhere inside what the parser consumed it is truncated and nothing is emitted
    const size_t n = (size_t)probe.stream_bytes;
    for (size_t cut = 0; cut < n; cut += (cut < 4096 ? 1 : 997))
      if (run(buf.data(), cut) != -2) fail("a cut stream is not truncated", cut);
  }
  std::printf("%ld emitted, %ld truncated, %ld refused\n%ld failures\n", g_ok, g_trunc, g_refused, g_fail);
  return g_fail ? 1 : 0;
}
