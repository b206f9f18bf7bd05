// bound_move_plan.h -- what the host decides when a stream moves between two bindings with clocks per stream (mode P:
// BeatriceBatch_ConfigureWrapperRates + BindResidentBlocksRagged + ProcessBlocksRaggedDevice) WITHOUT a drain
// (BeatriceBatch_BoundStreamQuiescent / MoveBoundStreamsInFlight / ExportBoundStreamsInFlight / ImportBoundStreamsInFlight,
// batch_wrappers.hip.h; the kernels: bound_move.hip): when a bound stream is at rest, in which order a call is refused, where the hop a
// stream carries goes in the destination, how the two forms of the 480-sample FIFO turn into each other, and the bounds of every index
// the kernels use.  Plain C++17, no HIP: tests/test_cpu_bound_move_plan.py walks it with a stand-alone program under the sanitizers
// against a brute-force model of the call / job / tick pipeline; rbr_step (the mark) and the entry points call it and restate none of it.
//
// WHAT A BOUND STREAM OWNS beyond its model rings and settings (stream_move_plan.h moves those): its wrapn::StreamState on the device,
// the 240 output samples of its LAST FIRED HOP in the ticks' resident output slots -- the output half of its next block reads them:
// 48 kHz sample t comes from hop hop_base + t / 480 - 1 at offset t % 480, zero-stuffed (wrapr_post_kernel), a block starts at
// t0 = t48 and t48 / 480 hops have fired since the restart, so exactly one old hop is still wanted, from offset fill = t48 % 480 on --
// and on the host its rate, its three clocks, both gain clocks and its sample and hop counts.
//
// AT REST, two rules.
//   (a) No step of the stream is inside the ticks: smove::Presence, marked by the ragged branch of tick_run.
//   (b) The output half of every call the stream was active in has been launched: no Job still owed belongs to such a call.  rbr_step
//       pushes the job of call c in call c and launches it in the first call k with c + delay <= k, jobs in order: the job of call c is
//       launched during call c + delay (or at a drained point before).  So with c the stream's last active call, (b) holds once call
//       c + delay has been made -- `calls` (the calls made so far; the next call's number) >= c + delay + 1 -- which a scheduler reaches
//       by handing in n_samples[s] = 0 for `delay` calls.  Every call launches at least one tick, and delay = stages - 1, so the step
//       fed by the stream's last present tick T (in call c) has left the last stage by then as well: ticks >= T + 1 + delay = T + stages.
//       The verdict asks the job queue itself (the oldest call still owed), which is also right behind a drain.
//   From then on every launch enqueued leaves the stream's StreamState, its slot-map entries and its cell of every resident slot alone:
//   the input half returns at once for an inactive record, the output half writes zeros into the caller's block and touches no state, and
//   every tick body skips an absent row.
//
// THE CARRIED HOP.  The destination keeps its own hop numbering: its next hop is number hops_s[t], so the carried one is "hop
// hops_s[t] - 1" and its slot-map entry is carried_entry(); it goes into the stream's cell of the resident slot the destination took
// most recently (dest_slot()), which gives it the lifetime of a native hop fired in the destination's latest step.  hop_base() makes
// wrapr_post_kernel's index (hop_base + k) % map_ring, k = t / 480 - 1 >= 0, hit that entry for k = fired - 1 and the entries the
// stream's own hops will write (hop g at g % map_ring) for every later k: only the residue modulo map_ring matters, and it is taken
// non-negative, so every index stays in [0, map_ring).
//
// THE TWO FIFO FORMS.  The in-order form (wrapr_refill_kernel) keeps the zero-stuffed output of the last hop in FIFO places [fill, 480);
// the bound form keeps it in the resident slots and leaves stale input in those places.  Places [0, fill) are the same in both: the inner
// samples taken since the last hop.  fifo_place() writes the in-order form from the bound one, hop_place() reads it back.
#pragma once
#include <vector>

#include "stream_move_plan.h"
#include "wrapper_plan.h"

namespace bhip {
namespace bmove {

constexpr long long kNever = -1;
constexpr int kFifo = wrapn::kBlock;   // 480 places
constexpr int kHop = kFifo / 2;        // 240 output samples per hop

// ---- rule (b): the mark rbr_step sets for every stream that hands in a block, and the question ----
struct Marks {
  std::vector<long long> last_active;   // [B] the stream's last active call of this binding
  void start(int B) { last_active.assign((size_t)B, kNever); }
  void active(int s, long long call) { last_active[(size_t)s] = call; }
  // oldest_owed: the call of the oldest job still in the queue, `calls` when none is
  bool outputs_launched(int s, long long oldest_owed) const { return last_active[(size_t)s] < oldest_owed; }
};
// the call that must have been made for (b) to hold behind a last active call c, without a drain
inline long long rule_b_call(long long c, int delay) { return c + delay; }

// ---- the order of the refusals (stream_move_plan.h's: all -1 of every side, then -3, then the work) ----
using smove::Verdict;
using smove::kGo;
using smove::kRefused;
using smove::kBusy;

struct Side {
  bool bound_ragged = false;   // mode P (batch_modes.h: where ProcessBlocksRaggedDevice is allowed)
  int B = 0, n = 0;
  const int* streams = nullptr;
  bool pointers_ok = false;
};
inline Verdict args(const Side& s) { return s.pointers_ok && s.bound_ragged && smove::streams_ok(s.B, s.n, s.streams) ? kGo : kRefused; }

struct Rest {
  const smove::Presence* seen = nullptr;
  long long ticks = 0;
  int stages = 0;
  const Marks* marks = nullptr;
  long long oldest_owed = 0;
  const unsigned char* reset_pending = nullptr;     // nullptr: none pending, or a destination (the import cancels them)
  const unsigned char* restart_pending = nullptr;   // likewise (RestartStreamInFlight / SetStreamRateInFlight no block has taken)
};
inline bool quiescent(const Rest& r, int s) { return r.seen->quiescent(s, r.ticks, r.stages) && r.marks->outputs_launched(s, r.oldest_owed); }
inline Verdict at_rest(const Side& s, const Rest& r) {
  for (int i = 0; i < s.n; ++i) {
    const int st = s.streams[i];
    if (!quiescent(r, st)) return kBusy;
    if ((r.reset_pending && r.reset_pending[st]) || (r.restart_pending && r.restart_pending[st])) return kBusy;
  }
  return kGo;
}
// the whole order in one place: arguments and mode, the blobs, the pairing of a move, the rate on the destination, then rest
inline Verdict verdict(bool args_ok, bool blobs_ok, bool pairing_ok, bool rate_ok, bool rest_ok) {
  if (!args_ok || !blobs_ok || !pairing_ok || !rate_ok) return kRefused;
  return rest_ok ? kGo : kBusy;
}

// a rate on a binding made for blocks of at most max_samples whose ring of resident slots and slot map were sized for hops_cap hops per call
inline bool rate_fits(double rate, int max_samples, int hops_cap) {
  wrapn::RateClass c;
  if (!std::isfinite(rate) || !c.configure(rate)) return false;
  const int longest = wrapn::longest_block(rate);
  return wrapn::most_hops(max_samples < longest ? max_samples : longest, rate) <= hops_cap;
}

// ---- the carried hop ----
inline long long mod_ring(long long v, int ring) { return ((v % ring) + ring) % ring; }
inline long long hops_since_restart(long long t48) { return t48 / kFifo; }
inline bool has_hop(long long t48) { return t48 >= kFifo; }
inline int fill_of(long long t48) { return (int)(t48 % kFifo); }
// the slot-map entry of a stream's last fired hop, source or destination: hop number hops_s - 1
inline int carried_entry(long long hops_s, int map_ring) { return (int)mod_ring(hops_s - 1, map_ring); }
// the resident slot the destination took most recently (io_host: the slot its next step takes)
inline int dest_slot(int io_host, int io_slots) { return (int)mod_ring((long long)io_host - 1, io_slots); }
inline int hop_base(long long dst_hops_s, long long t48, int map_ring) { return (int)mod_ring(dst_hops_s - hops_since_restart(t48), map_ring); }
// the sample count a blob's stream starts with: the blob holds the fill, and its places [fill, 480) stand for one fired hop (zeros
// where none was)
inline long long t48_of_blob(int fill) { return (long long)kFifo + fill; }

// ---- the FIFO split at `fill` ----
// place i of the in-order FIFO from the bound form: the stream's own place below fill, the zero-stuffed hop from fill on
// (constexpr: the kernels of bound_move.hip call the same two functions)
constexpr float fifo_place(int i, int fill, const float* fifo, const float* hop /* nullptr: no hop fired */) {
  return i < fill ? fifo[i] : ((i & 1) || !hop ? 0.0f : hop[i >> 1]);
}
// sample j of the carried hop from the in-order FIFO: its even place when that is at or above fill (what is below was read long ago)
constexpr float hop_place(int j, int fill, const float* fifo) { return 2 * j >= fill ? fifo[2 * j] : 0.0f; }

// ---- what the kernels index, for one stream of a round ----
struct Geometry { int B = 0, io_slots = 0, map_ring = 0; };   // one binding: streams, resident slots, slot-map entries per stream
struct Item {
  int stream = 0;      // the stream's row of d_wrap, of slot_map and of every resident slot
  int entry = 0;       // slot_map[stream][entry]: read (source) or written (destination)
  int slot = 0;        // destination: the resident slot written and named; source: unused (the kernel reads it from the map and checks it)
  int fill = 0;        // FIFO places below are the stream's own
  int has_hop = 0;     // source: a hop has fired since the restart
};
inline bool item_ok(const Geometry& g, const Item& it) {
  return g.B >= 1 && g.io_slots >= 1 && g.map_ring >= 1 && it.stream >= 0 && it.stream < g.B && it.entry >= 0 && it.entry < g.map_ring &&
         it.slot >= 0 && it.slot < g.io_slots && it.fill >= 0 && it.fill < kFifo;
}
inline Item source_item(int s, long long hops_s, long long t48, int fill, int map_ring) {
  Item it;
  it.stream = s; it.entry = carried_entry(hops_s, map_ring); it.slot = 0; it.fill = fill; it.has_hop = has_hop(t48) ? 1 : 0;
  return it;
}
inline Item dest_item(int t, long long hops_s, int fill, int io_host, int io_slots, int map_ring) {
  Item it;
  it.stream = t; it.entry = carried_entry(hops_s, map_ring); it.slot = dest_slot(io_host, io_slots); it.fill = fill; it.has_hop = 1;
  return it;
}

}  // namespace bmove
}  // namespace bhip
