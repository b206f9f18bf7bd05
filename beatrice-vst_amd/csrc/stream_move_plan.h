// stream_move_plan.h -- what the host decides when a stream moves between two tick-mode batches WITHOUT a drain
// (BeatriceBatch_StreamQuiescent / ExportStreamsInFlight / ImportStreamsInFlight / MoveStreamsInFlight, batch.hip; the kernels:
// stream_blob.hip): when a stream is at rest, which counter is its own, how far a ring turns on the way in, and in which order a call is
// refused.  Plain C++17, no HIP: tests/test_cpu_stream_move_plan.py walks it with a stand-alone program under the sanitizers, and
// batch_tick.hip.h (the marks) and batch.hip (the questions) call it and restate none of it.
//
// At rest.  The step fed by tick T is at stage s in the launch of tick T + s, and has left the last of `stages` stages once tick
// T + stages - 1 has been launched -- once `ticks` (the ticks launched so far; the next tick's number) >= T + stages.  A stream is quiescent
// when that holds for the tick that fed its last present step, or when it has taken part in no step since the last drained point.  Every
// launch enqueued from then on leaves the stream's rows alone (an absent row is skipped by every body), so a gather or a scatter of its
// rings enqueued between two ticks reads and writes state nobody else touches, at the stream's own counter.
//
// The marks cost the common path one scalar: while every stream takes part in every step (the common counter) a feeding tick sets
// `last_feed`; the ragged branch of tick_run, which loops over the streams anyway, marks the present ones one by one.  A stream's mark is
// the later of the two, so the step in which the batch turns ragged needs no hand-over.
//
// At rest around the 48 kHz wrapper (mode F, BeatriceBatch_BindResidentIO48k; BeatriceBatch_Stream48kQuiescent / ExportStreams48kInFlight /
// ImportStreams48kInFlight / MoveStreams48kInFlight).  The wrapper's output half runs ONE LAUNCH LATE: the step fed by tick T leaves the
// last stage in the launch of tick T + stages - 1, and its 48 kHz block is produced -- the stream's Wrap48State read and written -- by the
// wrapper launch in front of tick T + stages, or by the flush launch of a drain that gets there first.  So a stream of an F batch is at
// rest when it has taken part in no step since the last drained point, or when the wrapper launch that carries the output half of its
// last present step has been enqueued: ticks - last_step_of(s) >= stages + 1 (kRuleAround48k: one launch more than the plain rule).  A
// drain has flushed that launch before it calls drained(), which clears the marks.  From that launch on no launch reads or writes the
// stream's rings, its previous bin or its Wrap48State until the stream is fed again: every tick body skips an absent row, an absent
// stream's input half of the wrapper launch returns before it reads the state, and its output half copies its own down-mix and touches no
// state.  A travelling reset of the stream (BeatriceBatch_ResetStreamInFlight) lives exactly as long -- its last clear goes in front of
// that same wrapper launch -- so a stream at rest by this rule has no reset travelling either.
#pragma once
#include <algorithm>
#include <vector>

#include "stream_blob.h"

namespace bhip {
namespace smove {

constexpr long long kNever = -1;

struct Presence {
  std::vector<long long> last_present;   // [B] the tick that fed the stream's last present step while the batch was ragged
  long long last_feed = kNever;          // the last tick that fed a step of the common counter: every stream took part
  void start(int B) { last_present.assign((size_t)B, kNever); last_feed = kNever; }
  // a drained point (tick_drain has run the pipeline empty; tick_relevel): no step of any stream is inside
  void drained() { std::fill(last_present.begin(), last_present.end(), kNever); last_feed = kNever; }
  void fed_all(long long tick) { last_feed = tick; }
  void fed(int s, long long tick) { last_present[(size_t)s] = tick; }
  long long last_step_of(int s) const { return std::max(last_present[(size_t)s], last_feed); }
  bool quiescent(int s, long long ticks, int stages) const {
    const long long t = last_step_of(s);
    return t == kNever || ticks - t >= stages;
  }
};

// Which rule a call asks: the plain one (mode D) or the one around the 48 kHz wrapper (mode F), whose launches_behind_last_stage() more
// launches must have been enqueued.
enum Rule { kRulePlain = 0, kRuleAround48k = 1 };
inline int launches_behind_last_stage(Rule r) { return r == kRuleAround48k ? 1 : 0; }
inline bool quiescent(const Presence& p, Rule r, int s, long long ticks, int stages) { return p.quiescent(s, ticks, stages + launches_behind_last_stage(r)); }

// A stream's OWN counter: the counter of the next step it takes part in (tick::State::hop_s while the batch is ragged, the batch's one
// counter otherwise).  A blob's header carries it on the way out; on the way in the rings turn by the difference to the DESTINATION
// stream's own counter -- the batch's counter is only right at a drained point.
inline int own_counter(bool ragged, const std::vector<int>& hop_s, int s, int hop_host) { return ragged ? hop_s[(size_t)s] : hop_host; }
inline int import_shift(int dst_own_counter, int blob_counter, int wrap) { return sblob::counter_shift(dst_own_counter, blob_counter, wrap); }

// every stream named once and in range (the drained calls ask the same)
inline bool streams_ok(int B, int n, const int* streams) {
  if (n < 1 || n > B || !streams) return false;
  std::vector<char> seen((size_t)B, 0);
  for (int i = 0; i < n; ++i) {
    if (streams[i] < 0 || streams[i] >= B || seen[(size_t)streams[i]]) return false;
    seen[(size_t)streams[i]] = 1;
  }
  return true;
}

// The order of the refusals.  A call is all or nothing: every -1 of every side first (args(), then what the caller validates itself: the
// blobs of an import, the pairing of a move), then -3 (at_rest()), and only then anything is allocated, staged or launched (-2).
enum Verdict { kGo = 0, kRefused = -1, kBusy = -3 };
struct Side {
  bool plain_tick = false;   // mode D (batch_modes.h): what the plain calls ask for
  bool around48k = false;    // mode F: what the 48k calls ask for
  Rule rule = kRulePlain;    // the calls this side belongs to
  int B = 0, n = 0;
  const int* streams = nullptr;
  bool pointers_ok = false;  // every other pointer of the call (the NULL / 0 pairing of entry_map included)
};
inline Verdict args(const Side& s) {
  return s.pointers_ok && (s.rule == kRuleAround48k ? s.around48k : s.plain_tick) && streams_ok(s.B, s.n, s.streams) ? kGo : kRefused;
}
// reset_pending: the batch's flags of BeatriceBatch_ResetStreamInFlight no step has taken yet, nullptr where they do not refuse (a
// destination: the import cancels them)
inline Verdict at_rest(const Side& s, const Presence& p, long long ticks, int stages, const unsigned char* reset_pending) {
  for (int i = 0; i < s.n; ++i) {
    if (!quiescent(p, s.rule, s.streams[i], ticks, stages)) return kBusy;
    if (reset_pending && reset_pending[s.streams[i]]) return kBusy;
  }
  return kGo;
}

}  // namespace smove
}  // namespace bhip
