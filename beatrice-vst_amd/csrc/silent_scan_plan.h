// silent_scan_plan.h -- the host side of BeatriceBatch_ScanSilentBlocks* (include/beatrice_batch.h) without HIP: what a call is
// refused for, which of the kernel's two paths it takes, its grid, the ring of tickets, and why an accepted call keeps every read of
// the kernel (silent_scan.hip) inside the caller's cells.  Plain C++17: batch.hip decides on it, tests/test_cpu_silent_scan_abi.py
// compiles it alone into a program of its own and walks it there.
//
// The geometry.  n_cells cells, cell c at float c * cell_stride of d_blocks.  A cell holds blocks_per_cell (J) planar blocks
// [channels][n_samples] back to back; or, with per-cell lengths (J = 1), one block [channels][len[c]] at its start, len[c] <= n_samples.
// Block (c, j) therefore occupies the floats
//     [c * cell_stride + j * channels * n_samples,  c * cell_stride + j * channels * n_samples + channels * len)      len = n_samples or len[c]
// and the kernel reads exactly those: lane l of the block's wavefront reads sample i (4-byte path) or samples 4i .. 4i + 3 (16-byte path,
// len a multiple of four) of each channel for i = l, l + 64, ... while i < len (i < len / 4), at channel offset ch * len.
//
// Why they stay inside cell c: the last float read is block_last(c, j) = c * cell_stride + j * channels * n_samples + channels * len - 1
//     <= c * cell_stride + (j + 1) * channels * n_samples - 1      (len <= n_samples: checked per cell)
//     <= c * cell_stride + J * channels * n_samples - 1            (j <= J - 1)
//     <= c * cell_stride + cell_stride - 1                         (cell_stride >= J * channels * n_samples: checked)
// and the first is >= c * cell_stride.  Nothing is rounded up: a block whose length or address is no multiple of four floats takes the
// 4-byte path as a whole, so no 16-byte load ever straddles a block's end.  All of it is 64-bit arithmetic that cannot wrap:
// n_cells * J <= 2^20 and cell_stride <= 2^40 bound every offset by 2^60 floats; the kernel's sample counter is 32-bit and n_samples
// <= 2^30 keeps i + 64 inside it.
#pragma once
#include <cstdint>

namespace bhip {
namespace sscan {

constexpr long long kMaxBlocks = 1ll << 20;    // blocks of one call
constexpr long long kMaxStride = 1ll << 40;    // floats between two cells
constexpr long long kMaxSamples = 1ll << 30;   // samples of a block: the kernel's 32-bit sample counter steps by 64 and stays far from its end
constexpr int kWavesPerGroup = 4, kThreads = 64 * kWavesPerGroup;   // one wavefront per block
constexpr int kTickets = 4;                    // scans that may be outstanding at once

struct Geometry {
  long long n_cells = 0, J = 0, channels = 0, n = 0, stride = 0;
  bool ragged = false;   // per-cell lengths
  long long blocks() const { return n_cells * J; }
  long long block_first(long long c, long long j) const { return c * stride + j * channels * n; }
  long long block_last(long long c, long long j, long long len) const { return block_first(c, j) + channels * len - 1; }   // (len >= 1)
};

// The refusals of BeatriceBatch_ScanSilentBlocksBegin (-1, nothing enqueued), in the order of the header's list.  `flags_given`: the
// one-call form's host array.  On success *g holds the call.
inline bool accept(const void* d_blocks, long long n_cells, long long blocks_per_cell, long long channels, long long n_samples,
                   long long cell_stride, const int* cell_samples, bool flags_given, Geometry* g) {
  if (!d_blocks || !flags_given) return false;
  if (n_cells < 1 || blocks_per_cell < 1 || (channels != 1 && channels != 2) || n_samples < 1) return false;
  if (n_cells > kMaxBlocks || blocks_per_cell > kMaxBlocks || n_cells * blocks_per_cell > kMaxBlocks) return false;
  if (cell_stride > kMaxStride || n_samples > kMaxSamples || cell_stride < blocks_per_cell * channels * n_samples) return false;
  if (cell_samples) {
    if (blocks_per_cell != 1) return false;
    for (long long c = 0; c < n_cells; ++c) if (cell_samples[c] < 0 || cell_samples[c] > n_samples) return false;
  }
  g->n_cells = n_cells; g->J = blocks_per_cell; g->channels = channels; g->n = n_samples; g->stride = cell_stride;
  g->ragged = cell_samples != nullptr;
  return true;
}

// The 16-byte path: every block's base and every channel's offset a multiple of four floats, every length too -- the base address,
// the stride and n_samples are (block (c, j) starts c * stride + j * channels * n floats behind the base, its second channel n
// further).  Per-cell lengths always take the 4-byte path.
inline bool vector_path(const void* d_blocks, const Geometry& g) {
  return !g.ragged && reinterpret_cast<std::uintptr_t>(d_blocks) % 16 == 0 && g.n % 4 == 0 && g.stride % 4 == 0;
}
// The last float the plan lets lane `lane` read in block (c, j) of length len; -1: the lane reads nothing.  lane_last and block_last are
// the closed forms of the kernel's loops (silent_scan.hip: `for (i = lane; i < items; i += 64)` per channel at offset ch * len) for the
// stand-alone program of tests/test_cpu_silent_scan_abi.py, which walks the same loops on the CPU: that is a MODEL of the kernel, sharing
// this header's geometry but not the kernel's code.  The kernel itself is held to the same bounds on the GPU by loud floats right in front
// of and right behind every block (tests/test_gpu_silent_scan.py::test_every_position).  Whoever changes the kernel's loops changes both.
inline long long lane_last(const Geometry& g, bool vec, long long c, long long j, long long len, int lane) {
  const long long items = vec ? len / 4 : len, w = vec ? 4 : 1;
  if (lane >= items) return -1;
  const long long i = lane + (items - 1 - lane) / 64 * 64;   // the lane's last item
  return g.block_first(c, j) + (g.channels - 1) * len + i * w + (w - 1);
}

inline unsigned grid(const Geometry& g) { return (unsigned)((g.blocks() + kWavesPerGroup - 1) / kWavesPerGroup); }

// kTickets scans may be outstanding.  A ticket = (serial << 2) | entry: the entry of the staging ring it occupies, and a serial number
// that tells it from every earlier holder of that entry, so a ticket that has ended (or was never given out) is recognised as such.
class TicketRing {
 public:
  explicit TicketRing(unsigned serial = 0) : serial_(serial) {}   // (where the serial numbers start: the header's test walks their wrap)
  int free_entry() const {   // -1: kTickets are out (BeatriceBatch_ScanSilentBlocksBegin's -3)
    for (int e = 0; e < kTickets; ++e) if (!out_[e]) return e;
    return -1;
  }
  int free_entries() const { int n = 0; for (int e = 0; e < kTickets; ++e) n += out_[e] ? 0 : 1; return n; }
  int issue(int e, long long n_blocks) {   // entry e (free_entry) is now out; returns its ticket (>= 0)
    serial_ = (serial_ + 1) & 0x0fffffff;
    ticket_[e] = (int)(serial_ << 2) | e;
    blocks_[e] = n_blocks;
    out_[e] = true;
    return ticket_[e];
  }
  int entry_of(int ticket) const {   // -1: unknown, or already ended
    if (ticket < 0) return -1;
    const int e = ticket & 3;
    return out_[e] && ticket_[e] == ticket ? e : -1;
  }
  long long blocks_of(int e) const { return blocks_[e]; }
  void end(int e) { out_[e] = false; }
 private:
  bool out_[kTickets] = {false, false, false, false};
  int ticket_[kTickets] = {-1, -1, -1, -1};
  long long blocks_[kTickets] = {0, 0, 0, 0};
  unsigned serial_;
};

}  // namespace sscan
}  // namespace bhip
