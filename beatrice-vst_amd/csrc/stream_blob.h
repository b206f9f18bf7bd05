// stream_blob.h -- the format of one stream's blob (BeatriceBatch_ExportStreams / BeatriceBatch_ImportStreams, batch.hip; the device side:
// stream_blob.hip) and everything that decides whether a blob is taken.  Plain C++17, no HIP: tests/test_cpu_stream_blob_format.py compiles
// it with g++ into a driver of its own.
//
// A blob is a short-lived token between two batches of the SAME library build, not a storage format: a reader takes exactly what this
// build writes and refuses everything else.  One blob, blob_bytes long (a multiple of 16, the same for every stream of a batch):
//
//   Header                      magic, version, blob size, hops per step, the source batch's step counter, the sizes of the fixed parts,
//                               a check word over header + ring shapes (any altered field is refused, the counter included)
//   RingShape[n_rings]          (C, n, m) of every ring of the three arenas in arena order: the layout fingerprint
//   int32[kIndices]             every speaker-table index of the stream's settings -- what entry_map is applied to
//   settings                    the batch's StreamCfg as it is in memory (its table indices are replaced by the mapped ones on import)
//   engine                      the stream's std::mt19937 in its textual form, zero padded
//   state (16-byte aligned)     every ring's m slots in slot order, each ring padded to 4 floats; the pitch head's previous bin; the
//                               48 kHz wrapper's history
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <random>
#include <sstream>
#include <string>
#include <vector>

namespace bhip {
namespace sblob {

constexpr uint32_t kMagic = 0x42535442u;   // "BTSB"
constexpr uint32_t kVersion = 1;
// target, additive and codebook speaker, the four installed key/value entries, the codebook of each hop of the last step
constexpr int kIndices = 3 + 4 + 8;
constexpr uint32_t kEngineBytes = 7168;    // 624 words + the position, ten digits and a blank each at most
constexpr int kMaxRound = 16;              // blobs per staging round (stream_blob.hip)

struct RingShape { int32_t C, n, m; };
struct Header {
  uint32_t magic, version;
  uint64_t blob_bytes;
  int32_t H, counter;
  uint32_t n_rings, cfg_bytes, w48_bytes, engine_bytes;
  uint64_t check;   // fnv-1a over the header (this field as zero) and the ring shapes
};
static_assert(sizeof(Header) == 48 && sizeof(RingShape) == 12, "blob header layout");

// one piece of a stream's device state inside a blob: m slots of slot_floats 4-byte words at word `off` of the blob
struct Piece { uint32_t slot_floats; int32_t m; uint64_t off; };

struct Layout {
  int H = 0;
  uint32_t cfg_bytes = 0, w48_bytes = 0;
  std::vector<RingShape> rings;
  std::vector<Piece> pieces;   // the rings in order, then the previous bin, then the 48 kHz wrapper's history
  size_t off_shapes = 0, off_indices = 0, off_cfg = 0, off_engine = 0, off_state = 0, blob_bytes = 0;
  size_t header_bytes() const { return off_indices; }   // Header + ring shapes
};

inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// w48_bytes must be a multiple of 4 (it is copied as words)
inline Layout make_layout(int H, const RingShape* rings, int n_rings, uint32_t cfg_bytes, uint32_t w48_bytes) {
  Layout l;
  l.H = H; l.cfg_bytes = cfg_bytes; l.w48_bytes = w48_bytes;
  l.rings.assign(rings, rings + n_rings);
  l.off_shapes = sizeof(Header);
  l.off_indices = l.off_shapes + sizeof(RingShape) * (size_t)n_rings;
  l.off_cfg = round_up(l.off_indices + sizeof(int32_t) * kIndices, 8);
  l.off_engine = l.off_cfg + cfg_bytes;
  l.off_state = round_up(l.off_engine + kEngineBytes, 16);
  size_t w = l.off_state / 4;
  auto piece = [&](uint32_t slot_floats, int32_t m) {
    l.pieces.push_back(Piece{slot_floats, m, (uint64_t)w});
    w += round_up((size_t)slot_floats * (size_t)m, 4);
  };
  for (int i = 0; i < n_rings; ++i) piece((uint32_t)rings[i].C * (uint32_t)rings[i].n, rings[i].m);
  piece(1, 1);
  piece(w48_bytes / 4, 1);
  l.blob_bytes = w * 4;
  return l;
}

inline uint64_t fnv1a(const unsigned char* p, size_t n, uint64_t h = 1469598103934665603ull) {
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
inline uint64_t header_check(const Header& h, const unsigned char* shapes, size_t shape_bytes) {
  Header z = h;
  z.check = 0;
  return fnv1a(shapes, shape_bytes, fnv1a(reinterpret_cast<const unsigned char*>(&z), sizeof(z)));
}

// the header and the ring shapes of a blob of layout `l` written at `blob` (at least l.header_bytes() long)
inline void write_header(const Layout& l, int counter, unsigned char* blob) {
  Header h{};
  h.magic = kMagic; h.version = kVersion; h.blob_bytes = l.blob_bytes; h.H = l.H; h.counter = counter;
  h.n_rings = (uint32_t)l.rings.size(); h.cfg_bytes = l.cfg_bytes; h.w48_bytes = l.w48_bytes; h.engine_bytes = kEngineBytes;
  const size_t shape_bytes = sizeof(RingShape) * l.rings.size();
  if (shape_bytes) std::memcpy(blob + l.off_shapes, l.rings.data(), shape_bytes);
  h.check = header_check(h, blob + l.off_shapes, shape_bytes);
  std::memcpy(blob, &h, sizeof(h));
}

enum Refusal { kOk = 0, kTruncated, kMagicBad, kVersionBad, kSizeBad, kHopsBad, kCounterBad, kLayoutBad, kCheckBad, kIndexUnmapped, kIndexRange };

// Is the header at `blob` (avail bytes readable) one this build wrote for a batch of layout `l`?  wrap: the step counter's wrap.
inline Refusal validate_header(const Layout& l, const unsigned char* blob, size_t avail, int wrap, int* counter_out = nullptr) {
  if (avail < sizeof(Header)) return kTruncated;
  Header h;
  std::memcpy(&h, blob, sizeof(h));
  if (h.magic != kMagic) return kMagicBad;
  if (h.version != kVersion) return kVersionBad;
  if (h.blob_bytes != l.blob_bytes) return kSizeBad;
  if (h.H != l.H) return kHopsBad;
  if (h.counter < 0 || h.counter >= wrap) return kCounterBad;
  if (h.n_rings != l.rings.size() || h.cfg_bytes != l.cfg_bytes || h.w48_bytes != l.w48_bytes || h.engine_bytes != kEngineBytes) return kLayoutBad;
  if (avail < l.header_bytes() || avail < l.blob_bytes) return kTruncated;
  const size_t shape_bytes = sizeof(RingShape) * l.rings.size();
  if (shape_bytes && std::memcmp(blob + l.off_shapes, l.rings.data(), shape_bytes) != 0) return kLayoutBad;
  if (h.check != header_check(h, blob + l.off_shapes, shape_bytes)) return kCheckBad;
  if (counter_out) *counter_out = h.counter;
  return kOk;
}

// The blob's table indices through entry_map (index i becomes entry_map[i]; NULL, 0: kept, and bounded by the table's capacity
// max_entries as BeatriceBatch_SetTargetSpeaker bounds them).  A mapped index must name one of the destination's n_speakers entries.
// (map_index_list: the same for indices that never were in a blob -- BeatriceBatch_MoveStreamsInFlight, settings host to host)
inline Refusal map_index_list(const int32_t* idx /* [kIndices] */, const int* entry_map, int n_map, int n_speakers, int max_entries,
                              int32_t* mapped /* [kIndices] */) {
  for (int i = 0; i < kIndices; ++i) {
    if (!entry_map) {
      if (idx[i] < 0 || idx[i] >= max_entries) return kIndexRange;
      mapped[i] = idx[i];
      continue;
    }
    if (idx[i] < 0 || idx[i] >= n_map) return kIndexUnmapped;
    const int to = entry_map[idx[i]];
    if (to < 0 || to >= n_speakers) return kIndexRange;
    mapped[i] = to;
  }
  return kOk;
}
inline Refusal map_indices(const Layout& l, const unsigned char* blob, const int* entry_map, int n_map, int n_speakers, int max_entries,
                           int32_t* mapped /* [kIndices] */) {
  int32_t idx[kIndices];
  std::memcpy(idx, blob + l.off_indices, sizeof(idx));
  return map_index_list(idx, entry_map, n_map, n_speakers, max_entries, mapped);
}
// two batches whose blobs are interchangeable: what validate_header holds a blob's header against
inline bool same_layout(const Layout& a, const Layout& b) {
  return a.H == b.H && a.cfg_bytes == b.cfg_bytes && a.w48_bytes == b.w48_bytes && a.blob_bytes == b.blob_bytes && a.rings.size() == b.rings.size() &&
         (a.rings.empty() || std::memcmp(a.rings.data(), b.rings.data(), sizeof(RingShape) * a.rings.size()) == 0);
}

// How far a ring of m slots turns between the source's counter and the destination's: slot j of the blob lands in slot
// (j + turn) % m, the arithmetic of ring_rotate_kernel (kernels_misc.hip.h).  wrap is a multiple of every m (RingArena::build).
inline int counter_shift(int dst_counter, int src_counter, int wrap) {
  const int d = (dst_counter - src_counter) % wrap;
  return d < 0 ? d + wrap : d;
}
inline int turn(int shift, int m) { return m > 1 ? shift % m : 0; }

// the lottery's engine: its textual form (operator<<), zero padded to kEngineBytes
inline bool engine_out(const std::mt19937& e, unsigned char* dst) {
  std::ostringstream os;
  os << e;
  const std::string s = os.str();
  if (s.size() + 1 > kEngineBytes) return false;
  std::memset(dst, 0, kEngineBytes);
  std::memcpy(dst, s.data(), s.size());
  return true;
}
inline bool engine_in(const unsigned char* src, std::mt19937* e) {
  if (src[kEngineBytes - 1] != 0) return false;
  std::istringstream is(std::string(reinterpret_cast<const char*>(src)));
  std::mt19937 got;
  is >> got;
  if (is.fail()) return false;
  *e = got;
  return true;
}

}  // namespace sblob
}  // namespace bhip
