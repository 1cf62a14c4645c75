// Upload and decode of serialized bitmaps (engine.hpp: the host units): staged host-to-device copy of the
// bytes, then the device decode into a batch's slotted arena (decode.hip).
#include <algorithm>
#include <atomic>
#include <thread>

#include "engine.hpp"

namespace rbg {

// ---------------------------------------------------------------------------
// upload: the host concatenates the serialized inputs (16 B aligned) and copies
// them once; decode.hip parses every header and places every payload on the GPU
// ---------------------------------------------------------------------------
static const char* dec_message(uint32_t e, int* status) {
  *status = RBG_ERR_TRUNCATED;
  switch (e) {
    case DEC_TRUNC_COOKIE: return "truncated input: cookie";
    case DEC_BAD_COOKIE: *status = RBG_ERR_INVALID_FORMAT; return "I failed to find one of the right cookies.";
    case DEC_TRUNC_SIZE: return "truncated input: size";
    case DEC_SIZE_LARGE: *status = RBG_ERR_INVALID_FORMAT; return "Size too large";
    case DEC_SIZE_NEG: *status = RBG_ERR_INVALID_FORMAT; return "negative container count";
    case DEC_TRUNC_FLAGS: return "truncated input: run flags";
    case DEC_TRUNC_DESC: return "truncated input: descriptors";
    case DEC_KEY_ORDER: *status = RBG_ERR_INVALID_FORMAT; return "container keys are not strictly increasing";
    case DEC_TRUNC_OFFSETS: return "truncated input: offsets";
    case DEC_TRUNC_RUNS: return "truncated input: run count";
    default: return "truncated input: container payload";
  }
}

static int dec_report(Ctx* c, size_t n) {
  std::vector<uint32_t> e(n);
  HIPCHK(hipMemcpy(e.data(), c->dec.err.p, 4 * n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++)
    if (e[i]) {
      int st;
      const char* m = dec_message(e[i], &st);
      set_err("input " + std::to_string(i) + ": " + m);
      return st;
    }
  set_err("decode reported an error but no input carries one");
  return RBG_ERR_DEVICE;
}

// Host side of an upload: the inputs are copied into pinned staging (worker
// threads over <= 4 MiB pieces, in offset order) and each ~32 MiB group goes to the
// device as soon as its pieces are staged, so the copies overlap the DMA.
static int stage_upload(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n, const uint64_t* dst_off,
                        uint64_t raw_bytes) {
  uint8_t* pin = reinterpret_cast<uint8_t*>(c->pinned);
  uint8_t* dev = c->raw.as<uint8_t>();
  hipStream_t s = c->stream;
  constexpr uint64_t kPiece = 4ull << 20, kGroup = 32ull << 20;
  if (raw_bytes <= kGroup) {
    for (size_t i = 0; i < n; i++)
      if (lens[i]) std::memcpy(pin + dst_off[i], bufs[i], lens[i]);
    if (raw_bytes) HIPCHK(hipMemcpyAsync(dev, pin, raw_bytes, hipMemcpyHostToDevice, s));
    return RBG_OK;
  }
  struct Piece {
    uint64_t dst;
    const uint8_t* src;
    uint64_t len;
    uint32_t g0, g1;  // groups the piece touches (pieces are smaller than a group)
  };
  std::vector<Piece> pieces;
  for (size_t i = 0; i < n; i++)
    for (uint64_t o = 0; o < lens[i]; o += kPiece) {
      const uint64_t d = dst_off[i] + o;
      const uint64_t l = std::min<uint64_t>(kPiece, lens[i] - o);
      pieces.push_back(Piece{d, bufs[i] + o, l, (uint32_t)(d / kGroup), (uint32_t)((d + l - 1) / kGroup)});
    }
  const uint32_t groups = (uint32_t)((raw_bytes + kGroup - 1) / kGroup);
  std::unique_ptr<std::atomic<int>[]> left(new std::atomic<int>[groups]);
  for (uint32_t g = 0; g < groups; g++) left[g].store(0);
  for (const Piece& p : pieces) {
    left[p.g0].fetch_add(1);
    if (p.g1 != p.g0) left[p.g1].fetch_add(1);
  }
  std::atomic<size_t> next{0};
  const int nthr = (int)std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (int t = 0; t < nthr; t++)
    th.emplace_back([&]() {
      for (size_t k; (k = next.fetch_add(1)) < pieces.size();) {
        std::memcpy(pin + pieces[k].dst, pieces[k].src, pieces[k].len);
        left[pieces[k].g0].fetch_sub(1, std::memory_order_release);
        if (pieces[k].g1 != pieces[k].g0) left[pieces[k].g1].fetch_sub(1, std::memory_order_release);
      }
    });
  int st = RBG_OK;
  for (uint32_t g = 0; g < groups; g++) {
    while (left[g].load(std::memory_order_acquire) > 0) std::this_thread::yield();
    const uint64_t lo = (uint64_t)g * kGroup, hi = std::min<uint64_t>(raw_bytes, lo + kGroup);
    if (st == RBG_OK && hipMemcpyAsync(dev + lo, pin + lo, hi - lo, hipMemcpyHostToDevice, s) != hipSuccess) {
      set_err("host-to-device copy of the upload failed");
      st = RBG_ERR_DEVICE;
    }
  }
  for (auto& x : th) x.join();
  return st;
}

// The serialized inputs at 16 B aligned offsets of one upload into c->raw: off[i] (host)
static int ctx_upload_raw(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n,
                          std::vector<uint64_t>* off) {
  if (n && (!bufs || !lens)) return RBG_ERR_ILLEGAL_ARGUMENT;
  for (size_t i = 0; i < n; i++)
    if (!bufs[i] && lens[i]) return RBG_ERR_ILLEGAL_ARGUMENT;
  off->assign(n, 0);
  uint64_t raw_bytes = 0;
  for (size_t i = 0; i < n; i++) {
    (*off)[i] = raw_bytes;
    raw_bytes = round16(raw_bytes + lens[i]);
  }
  CHK(c->raw.ensure(raw_bytes + 64));
  CHK(pinned_ensure(c, raw_bytes + 64));
  CHK(stage_upload(c, bufs, lens, n, off->data(), raw_bytes));
  dbg(c->stream, "load: host staging copy");
  return RBG_OK;
}

// Device decode of n uploaded inputs (c->raw at off[i], len[i] bytes) into one batch.
// key_major: containers sorted by (key, input) with a key CSR (operands of every op);
// otherwise input order (bitmap-major, batched andCardinality)
static int ctx_decode_raw(Ctx* c, const uint64_t* off, const size_t* lens, size_t n, bool key_major,
                          int32_t* out_id, bool pack_arrays = false) {
  DecBufs& d = c->dec;
  hipStream_t s = c->stream;
  std::vector<uint64_t> meta(2 * n + 2, 0);  // in_off[n], in_len[n]
  for (size_t i = 0; i < n; i++) {
    meta[i] = off[i];
    meta[n + i] = lens[i];
  }
  CHK(d.meta.ensure(8 * (2 * n + 2)));
  CHK(d.head.ensure(sizeof(DecHead) * n + 16));
  CHK(d.nctr.ensure(8 * n + 16));
  CHK(d.base.ensure(8 * n + 16));
  CHK(d.nch.ensure(8 * n + 16));
  CHK(d.chbase.ensure(8 * n + 16));
  CHK(d.flag.ensure(4 * n + 16));
  CHK(d.err.ensure(4 * n + 16));
  CHK(d.card.ensure(8 * n + 16));
  CHK(d.cons.ensure(8 * n + 16));
  CHK(d.part.ensure(8 * (scan_parts(std::max<size_t>(n, 1)) + 1)));
  CHK(c->scalar.ensure(64));
  const uint64_t* in_off = d.meta.as<uint64_t>();
  const uint64_t* in_len = in_off + n;
  unsigned long long* sc = c->scalar.as<unsigned long long>();  // [0] any error, [1] C, [2..5] totals, [6] bytes,
                                                                // [7] chunks
  HIPCHK(hipMemcpyAsync(d.meta.p, meta.data(), 8 * (2 * n + 2), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(sc, 0, 64, s));
  dbg(s, "load: H2D");
  uint32_t* any_err = reinterpret_cast<uint32_t*>(sc);
  launch_dec_head(s, c->raw.as<uint8_t>(), in_off, in_len, n, d.head.as<DecHead>(), d.nctr.as<uint64_t>(),
                  d.nch.as<uint64_t>(), d.err.as<uint32_t>(), any_err);
  launch_exclusive_scan(s, d.nctr.as<uint64_t>(), d.base.as<uint64_t>(), n, d.part.as<uint64_t>(),
                        reinterpret_cast<uint64_t*>(sc + 1));
  launch_exclusive_scan(s, d.nch.as<uint64_t>(), d.chbase.as<uint64_t>(), n, d.part.as<uint64_t>(),
                        reinterpret_cast<uint64_t*>(sc + 7));
  HIPCHK(hipGetLastError());
  unsigned long long h[8] = {};
  HIPCHK(hipMemcpyAsync(h, sc, 64, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (h[0]) return dec_report(c, n);
  const uint64_t C = h[1];
  if (C > 0x7FFFFFFFull) {
    set_err("a batch holds at most 2^31 - 1 containers");
    return RBG_ERR_ILLEGAL_ARGUMENT;
  }
  dbg(s, "load: headers");
  const uint64_t n_chunks = h[7];
  CHK(d.q.ensure(sizeof(DecCtr) * C + 16));
  CHK(d.qkey.ensure(2 * C + 16));
  CHK(d.chmap.ensure(4 * n_chunks + 16));
  HIPCHK(hipMemsetAsync(d.card.p, 0, 8 * n + 16, s));
  HIPCHK(hipMemsetAsync(d.flag.p, 0, 4 * n + 16, s));
  launch_dec_ctrs(s, c->raw.as<uint8_t>(), in_off, in_len, n, d.head.as<DecHead>(), d.base.as<uint64_t>(),
                  d.nch.as<uint64_t>(), d.chbase.as<uint64_t>(), reinterpret_cast<uint64_t*>(sc + 7), n_chunks,
                  d.chmap.as<uint32_t>(), d.q.as<DecCtr>(), d.qkey.as<uint16_t>(), d.card.as<uint64_t>(),
                  d.flag.as<uint32_t>(), d.cons.as<uint64_t>(), d.err.as<uint32_t>(), any_err);
  const int32_t id = new_batch(c);
  Batch& b = *c->batches[id];
  BatchGuard guard{c, {id}};  // dropped unless the load completes
  b.n_bm = n;
  b.n_ctr = C;
  b.key_major = key_major;
  CHK(b.keys.ensure(2 * C + 16));
  CHK(b.desc.ensure(sizeof(CDesc) * C + 16));
  CHK(b.bm.ensure(4 * C + 16));
  CHK(b.bm_off.ensure(4 * (n + 1)));
  const uint32_t* perm = nullptr;
  if (key_major) {
    CHK(b.key_off.ensure(4 * (kMaxKeys + 1)));
    const uint16_t* sorted = d.qkey.as<uint16_t>();
    if (n > 1 && C > 0) {  // one bitmap is key-sorted already
      const size_t tb = dec_sort_temp_bytes(C);
      CHK(d.sort.ensure(tb + 16));
      CHK(d.skey.ensure(2 * C + 16));
      CHK(d.iota.ensure(4 * C + 16));
      CHK(d.perm.ensure(4 * C + 16));
      if (launch_dec_sort(s, d.sort.p, tb, d.qkey.as<uint16_t>(), d.skey.as<uint16_t>(), d.iota.as<uint32_t>(),
                          d.perm.as<uint32_t>(), C) != 0) {
        set_err("radix sort of the container keys failed");
        return RBG_ERR_DEVICE;
      }
      sorted = d.skey.as<uint16_t>();
      perm = d.perm.as<uint32_t>();
    }
    launch_dec_key_off(s, sorted, C, b.key_off.as<uint32_t>());
  }
  dbg(s, "load: containers + sort");
  CHK(d.size.ensure(8 * C + 16));
  CHK(d.cpart.ensure(8 * (scan_parts(std::max<uint64_t>(C, 1)) + 1)));
  launch_dec_sizes(s, d.q.as<DecCtr>(), perm, C, d.size.as<uint64_t>(), sc + 2);
  launch_exclusive_scan(s, d.size.as<uint64_t>(), d.size.as<uint64_t>(), C, d.cpart.as<uint64_t>(),
                        reinterpret_cast<uint64_t*>(sc + 6));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, sc, 64, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (h[0]) return dec_report(c, n);
  for (int k = 0; k < 3; k++) b.n_kind[k] = (int64_t)h[2 + k];
  b.max_ser = h[5];
  // a key-major batch of arrays alone, for the wide ops: the array payloads packed as in the portable
  // format (2 B granularity) instead of 16 B slots -- the wide kernels' fastest layout
  const bool packed = pack_arrays && key_major && C > 0 && b.n_kind[DK_B] == 0 && b.n_kind[DK_R] == 0;
  if (packed) {
    launch_dec_sizes(s, d.q.as<DecCtr>(), perm, C, d.size.as<uint64_t>(), nullptr, true);
    launch_exclusive_scan(s, d.size.as<uint64_t>(), d.size.as<uint64_t>(), C, d.cpart.as<uint64_t>(),
                          reinterpret_cast<uint64_t*>(sc + 6));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, sc, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    b.packed = true;
  }
  b.payload_bytes = h[6];
  CHK(b.payload.ensure(b.payload_bytes + 64));
  dbg(s, "load: sizes + payload alloc");
  launch_dec_fill(s, c->raw.as<uint8_t>(), d.q.as<DecCtr>(), d.qkey.as<uint16_t>(), perm, d.size.as<uint64_t>(), C,
                  b.desc.as<CDesc>(), b.keys.as<uint16_t>(), b.bm.as<uint32_t>(), b.payload.as<uint8_t>(),
                  d.card.as<uint64_t>(), packed);
  HIPCHK(hipGetLastError());
  std::vector<uint64_t> nctr(n), card(n), cons(n);
  if (n) {
    HIPCHK(hipMemcpyAsync(nctr.data(), d.nctr.p, 8 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(card.data(), d.card.p, 8 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cons.data(), d.cons.p, 8 * n, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  b.h_bm_off.assign(n + 1, 0);
  b.h_bm_nctr.resize(n);
  b.h_bm_card.resize(n);
  for (size_t i = 0; i < n; i++) {
    b.h_bm_nctr[i] = (uint32_t)nctr[i];
    b.h_bm_off[i + 1] = b.h_bm_off[i] + (uint32_t)nctr[i];
    b.h_bm_card[i] = (int64_t)card[i];
    b.long_card += (int64_t)card[i];
    b.ser_bytes += (int64_t)cons[i];
  }
  HIPCHK(hipMemcpyAsync(b.bm_off.p, b.h_bm_off.data(), 4 * (n + 1), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  dbg(s, "load: fill + readback");
  guard.ids.clear();
  b.live = true;
  *out_id = id;
  return RBG_OK;
}

int ctx_load_impl(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n, bool key_major, int32_t* out_id,
                  bool pack_arrays) {
  std::vector<uint64_t> off;
  CHK(ctx_upload_raw(c, bufs, lens, n, &off));
  return ctx_decode_raw(c, off.data(), lens, n, key_major, out_id, pack_arrays);
}

// pack_arrays: a batch of arrays alone is decoded packed (wide ops and fetches only, see Batch::packed)
int ctx_load(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* out_id,
             bool pack_arrays) {
  return ctx_load_impl(c, bufs, lens, n, true, out_id, pack_arrays);
}

// n serialized bitmaps in ONE upload, each decoded into a batch of its own (the operands of a
// pairwise op: one staging pass and DMA for both); ids[i] = batch of bitmap i
int ctx_load_separate(Ctx* c, const uint8_t* const* bufs, const size_t* lens, size_t n, int32_t* ids) {
  std::vector<uint64_t> off;
  CHK(ctx_upload_raw(c, bufs, lens, n, &off));
  BatchGuard g{c, {}};
  for (size_t i = 0; i < n; i++) {
    CHK(ctx_decode_raw(c, &off[i], &lens[i], 1, true, &ids[i]));
    g.ids.push_back(ids[i]);
  }
  g.ids.clear();
  return RBG_OK;
}

}  // namespace rbg
