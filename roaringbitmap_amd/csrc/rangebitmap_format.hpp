// Host-side format layer of the range-encoded index: validation and one walk of a serialized RangeBitmap
// (RB/RangeBitmap.java: map :65-85, Appender.serialize :1483-1504, append :1543-1588).  No HIP in it.
// RB/ = RoaringBitmap/src/main/java/org/roaringbitmap/.
//
// Stream, little-endian, nothing aligned:
//   u16 cookie 0xF00D | u8 base (2) | u8 sliceCount (1..64) | u16 maxKey (blocks of 65,536 rows) | u32 maxRid (rows)
//   maxKey masks of (sliceCount + 7) >> 3 bytes: bit i = the block has a container of slice i
//   per block, per slice of its mask, ascending: [u8 type][u16 size][payload]
//     BITMAP 0: size = cardinality as a Java char (65,536 stored as 0; any cardinality >= 1), 8192 B
//     RUN    1: size = run count, 4 B per run (start, length - 1)
//     ARRAY  2: size = cardinality, 2 B per value
// A record's position is known only from every record before it, so the walk happens once, here: it yields a
// directory entry per (block, slice) and the size of an arena in which every container has a 16 B aligned
// slot of the engine's own layout (device.hpp: CDesc), which relay() then fills.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rbg {

constexpr uint32_t kRbCookie = 0xF00D;  // RB/RangeBitmap.java:29
constexpr uint8_t kRbAbsent = 0xFF;     // directory entry of a slice the block's mask lacks
enum RbType : uint8_t { RBT_BITMAP = 0, RBT_RUN = 1, RBT_ARRAY = 2 };  // :30-32

// One (block, slice) of the directory: the engine's container kind (0 array, 1 bitmap, 2 run; kRbAbsent), the
// cardinality (bitmap: the wrapped field undone, 1..65,536; run: 0, not stored), the run count, where the
// payload lies in the stream and where its slot lies in the arena.
struct RbEntry {
  uint8_t kind = kRbAbsent;
  uint32_t card = 0;
  uint32_t nruns = 0;
  uint64_t src = 0;   // stream offset of the payload (behind the 3 header bytes)
  uint64_t slot = 0;  // arena offset, 16 B aligned; a run slot is [u16 0][u16 nruns][pairs]
};

struct RbIndex {
  uint32_t nslices = 0;
  uint32_t n_blocks = 0;  // maxKey
  uint64_t max_rid = 0;
  uint64_t mask = 0;                // -1 >>> (64 - sliceCount)
  std::vector<uint64_t> masks;      // per block, exactly bytesPerMask bytes of it
  std::vector<RbEntry> dir;         // n_blocks * nslices, block-major
  uint64_t arena_bytes = 0;         // sum of the slots
  uint64_t stream_bytes = 0;        // header + masks + records: what the walk consumed
  uint64_t payload_bytes = 0;       // container payload bytes of the stream (what a query may have to read)
};

// Status codes follow include/roaring_mi355x.h: 0, RBG_ERR_INVALID_FORMAT (-1: cookie, base, slice count, type
// byte, maxKey != ceil(maxRid / 65536)), RBG_ERR_TRUNCATED (-2: the stream ends inside the header, the masks or
// a record).
int rb_parse(const uint8_t* p, size_t n, RbIndex* out, std::string* err);
// every container of the directory into its slot of arena (arena_bytes, zeroed by the caller)
void rb_relay(const uint8_t* p, const RbIndex& idx, uint8_t* arena);
// The inverse of rb_relay, Appender.serialize (:1483-1504): the stream of a directory (nslices, n_blocks,
// max_rid, masks and per entry kind, card and slot; src and nruns are not read), its containers taken from
// their slots of an arena of arena_bytes.  A run's count is read from its slot, a bitmap's size field is its
// cardinality as a Java char (65,536 written as 0).  For what rb_parse and rb_relay made of a stream these are
// the bytes rb_parse consumed.  RBG_ERR_INVALID_FORMAT for a directory that does not fit its header or a slot
// that leaves the arena.
int rb_emit(const RbIndex& idx, const uint8_t* arena, uint64_t arena_bytes, std::vector<uint8_t>* out, std::string* err);

}  // namespace rbg
