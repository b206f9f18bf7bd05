// wrapper_blob.h -- the format of one stream's WRAPPER blob (BeatriceBatch_ExportStreamWrappers / BeatriceBatch_ImportStreamWrappers,
// batch_wrappers.hip.h) and everything that decides whether such a blob is taken.  Plain C++17, no HIP:
// tests/test_cpu_wrapper_blob_format.py compiles it with g++ into a driver of its own.
//
// It is the second token of a stream that moves between two batches with clocks per stream (BeatriceBatch_ConfigureWrapperRates): the
// stream blob (stream_blob.h) carries the model's state and the stream's settings, this one the host side of the stream -- what
// BeatriceBatch_SetStreamRate restarts, plus what it keeps.  Like the stream blob it is a short-lived token between two batches of the
// SAME library build, not a storage format: a reader takes exactly what this build writes and refuses everything else.  One blob,
// kBlobBytes long (a multiple of 16, the same for every stream of every batch):
//
//   Header                      magic, version, blob size, a check word over everything else (header and state), then the control fields:
//                               the stream's host rate, its two resampler clocks and its FIFO fill, both gain clocks (target and present
//                               gain in dB, input | output)
//   state (16-byte aligned)     the stream's wrapn::StreamState as it is in device memory: the two filter histories of each resampling
//                               direction and the 480-sample FIFO
//
// WHAT validate() PROMISES THE KERNELS.  The control fields steer index arithmetic on the device (wrapper.hip.h resample_one, the FIFO
// pieces), so a blob is only taken if no later call can index out of bounds with it.  hi / lo is the rate's ratio, fixed by the rate alone
// (wrapn::RateClass::configure, wrapper_plan.h, which the batch runs on the blob's rate and which bounds the history by kMaxHist); a call's
// Dir is made by wrapn::to_inner / to_outer from the class and the clocks, and the kernels read x = [hist | n_in] and a tap table of 32 hi + 1 entries:
//   decimating (resample_one, d.decimate):  n_out = (phase0 + n_in lo) / hi, so for every o < n_out the input count
//     k = ceil(((o + 1) hi - phase0) / lo) is <= n_in; with phase0 < hi it is >= 1, and ph = phase0 + k lo - (o + 1) hi lies in [0, lo).
//     The taps walked are lo - ph, 2 lo - ph, ... below 32 hi: all in [1, 32 hi), and at most ceil((32 hi - 1) / lo) <= 32 hi / lo + 1 =
//     hist of them, read downwards from x[hist + k - 1] -- the lowest index is >= k >= 1, the highest hist + n_in - 1.
//   interpolating:  the clock of output o is phase0 + (o + 1) lo, `pushed` = clock / hi, ph = clock % hi in [0, hi) for phase0 >= 0: exactly
//     32 taps ph, ph + hi, ... < 32 hi, read downwards from x[hist + pushed - 1] with hist = 33 -- the lowest index is pushed + 1 >= 1.
//     pushed <= n_in: towards 48 kHz n_out = ((n_in + 1) hi - phase_up - 1) / lo bounds the last clock by (n_in + 1) hi - 1; towards the
//     host n_out = (n_in hi + phase_down - phase_up) / lo bounds it by n_in hi + phase_down, and phase_down < hi.
// Both need exactly 0 <= phase < hi of either clock, which validate() checks against the `hi` the caller derived from the blob's own
// rate.  The FIFO pieces are [fill, fill + take) with take = min(480 - fill, rest): inside the FIFO for 0 <= fill < 480.  A clock pair
// that is in range but that no run of calls could have produced (the two clocks of a stream are coupled) can make the block count of
// to_outer differ from the block handed in: the call is then refused with -2 by the plan's own check (wrapn::plan_clocks), before any launch and with no clock moved.
// The gain values only feed host arithmetic (GainClock::advance); they must be finite so that a ramp ends.  The state is data.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "wrapper_plan.h"

namespace bhip {
namespace wblob {

constexpr uint32_t kMagic = 0x42575442u;   // "BTWB"
constexpr uint32_t kVersion = 1;
constexpr int kFifo = wrapn::kBlock;       // 10 ms at 48 kHz
// wrapn::StreamState: two histories of kMaxHist and two of 32 + 1 samples, the FIFO (batch.hip holds the two sizes equal)
constexpr uint32_t kStateBytes = 4u * (2u * wrapn::kMaxHist + 2u * (wrapn::kTapsPerOutput + 1) + wrapn::kBlock);

struct Header {
  uint32_t magic, version;
  uint64_t blob_bytes;
  uint64_t check;                  // fnv-1a over the header (this field as zero) and the state
  double rate;
  int32_t phase_down, phase_up, fill, reserved;
  double in_target_db, in_now_db, out_target_db, out_now_db;
};
static_assert(sizeof(Header) == 80 && sizeof(Header) % 16 == 0 && kStateBytes % 16 == 0, "wrapper blob layout");

constexpr size_t kOffState = sizeof(Header);
constexpr size_t kBlobBytes = kOffState + kStateBytes;

inline uint64_t fnv1a(const unsigned char* p, size_t n, uint64_t h = 1469598103934665603ull) {
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
inline uint64_t blob_check(const Header& h, const unsigned char* state) {
  Header z = h;
  z.check = 0;
  return fnv1a(state, kStateBytes, fnv1a(reinterpret_cast<const unsigned char*>(&z), sizeof(z)));
}

// the header of a blob whose state already sits at blob + kOffState (the check word covers it)
inline void write_header(double rate, int phase_down, int phase_up, int fill, double in_target_db, double in_now_db, double out_target_db,
                         double out_now_db, unsigned char* blob) {
  Header h{};
  h.magic = kMagic; h.version = kVersion; h.blob_bytes = kBlobBytes; h.rate = rate;
  h.phase_down = phase_down; h.phase_up = phase_up; h.fill = fill;
  h.in_target_db = in_target_db; h.in_now_db = in_now_db; h.out_target_db = out_target_db; h.out_now_db = out_now_db;
  h.check = blob_check(h, blob + kOffState);
  std::memcpy(blob, &h, sizeof(h));
}

enum Refusal { kOk = 0, kTruncated, kMagicBad, kVersionBad, kSizeBad, kCheckBad, kPhaseBad, kFillBad, kGainBad };

// Is `blob` (avail bytes readable) a blob of this build's format?  Its rate comes back: the caller derives hi from it (wrapn::RateClass::configure)
// and then asks validate().
inline Refusal read_rate(const unsigned char* blob, size_t avail, double* rate) {
  if (avail < sizeof(Header)) return kTruncated;
  Header h;
  std::memcpy(&h, blob, sizeof(h));
  if (h.magic != kMagic) return kMagicBad;
  if (h.version != kVersion) return kVersionBad;
  if (h.blob_bytes != kBlobBytes) return kSizeBad;
  if (avail < kBlobBytes) return kTruncated;
  if (rate) *rate = h.rate;
  return kOk;
}

// Everything: the format, the check word, and the ranges the kernels' index arithmetic needs (above) for a rate whose ratio is hi / lo.
inline Refusal validate(const unsigned char* blob, size_t avail, int hi, Header* out = nullptr) {
  const Refusal r = read_rate(blob, avail, nullptr);
  if (r != kOk) return r;
  Header h;
  std::memcpy(&h, blob, sizeof(h));
  if (h.check != blob_check(h, blob + kOffState)) return kCheckBad;
  if (h.phase_down < 0 || h.phase_down >= hi || h.phase_up < 0 || h.phase_up >= hi) return kPhaseBad;
  if (h.fill < 0 || h.fill >= kFifo) return kFillBad;
  if (!std::isfinite(h.in_target_db) || !std::isfinite(h.in_now_db) || !std::isfinite(h.out_target_db) || !std::isfinite(h.out_now_db)) return kGainBad;
  if (out) *out = h;
  return kOk;
}

}  // namespace wblob
}  // namespace bhip
