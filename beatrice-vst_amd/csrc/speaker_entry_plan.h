// speaker_entry_plan.h -- when an entry of the speaker tables is FREE: nothing the host has enqueued or is about to enqueue reads it, so
// BeatriceBatch_MorphSpeakersInFlight / InstallSpeakersInFlight may rewrite its tables between two ticks, and BeatriceBatch_SpeakerEntryBusy
// answers 0.  Plain C++17, no HIP: tests/test_cpu_speaker_entry_plan.py walks it with a stand-alone program under the sanitizers against a
// brute-force model of the pipeline, and batch.hip (recount, entry_named), batch_tick.hip.h (the feed, the clear) and batch_wrappers.hip.h
// (a filling step that is dropped) call it and restate none of it.
//
// An entry is busy by
//   (a) a NAME: some stream's settings name it -- target, additive or codebook speaker, one of the four installed key/value blocks.  Kept
//       by count (refs), per stream what was counted last (named), so that no step has to look at every stream;
//   (b) a STEP: no stream names it any more, but a step that was fed while it was named has not left the tick pipeline yet, or has not
//       even been fed (below).  Kept as one stamp per entry, written when its last name goes: free_at = the first value of `ticks` (the
//       ticks launched so far; the next tick's number) at which every such step has left the last stage;
//   (c) its codebook may be what a step drew through a morph entry that is itself busy by (a) or (b): a walk over the table's morph entries
//       at call time (batch.hip entry_busy), built on the two answers here.
//
// The stamp.  The step fed by tick T is at stage s in the launch of tick T + s and has left the last of `stages` stages once
// ticks >= T + stages.  When an entry's last name goes, the last step that can read it is
//   - the step fed last (Clock::last_feed_tick): a setter called between two launches.  The step fed next takes the new settings;
//   - the step about to be fed (Clock::tick), `next_step_too`: the per-hop key/value install at several hops per step, made inside the feed
//     itself -- the step's early hops still run on the blocks installed before;
//     The same feed may take the entry's LAST name afterwards by another way (the lottery draws a stream's codebook behind the install):
//     name() remembers the feed that replaced a block naming the entry (read_from), and a stamp made later counts from it at least;
//   - the step STILL FILLING (Clock::filling): see G below.  Its tick is not known yet; the entry waits, and fed() stamps it.
// A stream that sits steps out (the silent-block rule, a stream of P that fires no hop or hands in no samples) is not looked at: its names
// are stamped from the batch's last feed although its own last step went in earlier.  That errs on the safe side -- busy a little longer,
// never free too early -- and is the whole slack of the rule: an entry is free NO LATER than `stages` ticks after the base above.
//
// Rule (b) mode by mode (batch_modes.h).  Outside tick mode nothing is in flight between two calls and (b) does not apply.
//   D, E  plain tick mode, host streaming: one tick per call, feeding or not.  The rule above.
//   F     48 kHz blocks around the ticks, H = 1, 2, 4: the model side IS the plain tick pipeline -- one feeding tick per call, the settings
//         taken at the feed.  What F adds is the wrapper launch in front of each tick, whose input half resamples into the resident slot
//         and whose output half runs one launch late (stream_move_plan.h); both read the stream's wrapper state and the resident audio
//         and NO speaker table.  So an entry is free exactly when D says so: D's rule unchanged, no launch more.
//   P     any-rate blocks with clocks per stream, H = 1: a tick is launched for every FIFO piece in which some stream fires, one idle tick
//         if none does -- a call launches one or several ticks, of which 0 or more feed.  The stamps are in ticks, so nothing changes:
//         Clock::last_feed_tick is the last FEEDING tick however many calls ago.  The streams that do not fire sit the step out (above).
//   G     any-rate blocks with one set of clocks, H = 1, 2, 4.  At H = 1 as P without the sit-outs.  At H = 2 or 4 a step fills over
//         several calls and is fed (with the settings of that moment) when its last hop fires; ticks are launched for full steps only.
//         While a step is filling -- a hop has fired into it, it has not been fed -- a name that goes is stamped as if that step still
//         read the entry: the caller was told "the first hop of the next step fed", and a hop already fired belongs to a step the caller
//         cannot see the end of.  The step's feed tick is unknown (a drain in between launches idle ticks and moves it), so the entry WAITS
//         and the feed stamps it: free_at = that tick + stages.  Neither BeatriceBatch_Synchronize nor the clear at a drained point frees a
//         waiting entry: the filling step, like the output blocks still owed (BeatriceBatch_ResidentBlocksOwed), survives a drain.  The
//         wait ends without a feed only when the filling step is dropped (BeatriceBatch_FlushResidentBlocks starting the binding over,
//         an unbind): filling_dropped().  A step counts as filling from the end of the call that fired its first hop without completing it
//         until its feed is over (step_open_during_feed / step_open_after_call below, kept in
//         BeatriceBatch::ResidentBlocks::step_open); a step that one call starts and completes never does.  The same step's early hops
//         running on key/value blocks installed before is next_step_too, as in D: made inside the feed, stamped from that feed.
#pragma once
#include <algorithm>
#include <vector>

#include "batch_modes.h"

namespace bhip {
namespace sentry {

// What the stamp reads of the tick pipeline at the moment a name goes (tick::State, BeatriceBatch::ResidentBlocks).
struct Clock {
  long long tick = 0;             // ticks launched so far = the number of the next tick
  long long last_feed_tick = 0;   // the last tick that fed a step
  int stages = 0;                 // depth of the pipeline (tick::Plan::count())
  bool filling = false;           // G at several hops per step: a hop has fired into a step that has not been fed
};

constexpr bool rule_b_applies(modes::Mode m) {
  return m == modes::Mode::D || m == modes::Mode::E || m == modes::Mode::F || m == modes::Mode::G || m == modes::Mode::P;
}
// G's filling step, from what the binding counts (hops fired, H hops per step), at the two moments the flag is written by one call of
// the uniform any-rate blocks: while the call's feed number `feed` (0: its first) runs -- open only if an EARLIER call left that step
// filling --, and once the call's feeds are over.
constexpr bool step_open_during_feed(long long hops_before_call, int H, int feed) { return H > 1 && feed == 0 && hops_before_call % H != 0; }
constexpr bool step_open_after_call(long long hops_after_call, int H) { return H > 1 && hops_after_call % H != 0; }

constexpr long long kLongAgo = -1000;   // (tick::State::last_feed_tick before the first feed)

struct Plan {
  int per_stream = 0;               // names a stream's settings hold
  std::vector<int> refs;            // [entries] names of the entry among all streams' settings
  std::vector<long long> free_at;   // [entries] rule (b)'s stamp
  std::vector<long long> read_from; // [entries] the last feed that replaced a key/value block naming the entry (next_step_too)
  std::vector<char> waits;          // [entries] ... which the feed of the filling step has still to write
  std::vector<int> waiting;         // the entries with waits set
  std::vector<int> named;           // [streams][per_stream] what name() last counted

  // every stream on entry 0 (StreamCfg's defaults)
  void start(int streams, int entries, int names_per_stream) {
    per_stream = names_per_stream;
    refs.assign((size_t)entries, 0); free_at.assign((size_t)entries, 0); waits.assign((size_t)entries, 0); waiting.clear();
    read_from.assign((size_t)entries, kLongAgo);
    named.assign((size_t)streams * names_per_stream, 0);
    if (entries > 0) refs[0] = streams * names_per_stream;
  }
  // Brings the counts up to stream s's settings (now[per_stream]); an entry whose last name goes is stamped.
  void name(int s, const int* now, const Clock& c, bool next_step_too) {
    int* seen = &named[(size_t)s * per_stream];
    for (int i = 0; i < per_stream; ++i) {
      if (seen[i] == now[i]) continue;
      ++refs[(size_t)now[i]];
      if (next_step_too) read_from[(size_t)seen[i]] = c.tick;   // (the step being fed still runs on it, whoever else names it)
      if (--refs[(size_t)seen[i]] == 0) last_name_gone(seen[i], c, next_step_too);
      seen[i] = now[i];
    }
  }
  // A step has been fed by tick `tick`: the filling step, if entries waited for one.
  void fed(long long tick, int stages) {
    if (waiting.empty()) return;
    for (int e : waiting) { waits[(size_t)e] = 0; free_at[(size_t)e] = std::max(free_at[(size_t)e], tick + stages); }
    waiting.clear();
  }
  // The filling step will never be fed (the binding starts over or ends): what waited for it falls back to the last step that was.
  void filling_dropped(long long last_feed_tick, int stages) { fed(last_feed_tick, stages); }
  // A drained point at which the tick counter starts over (tick mode comes on): the pipeline is empty, stamps of an earlier stay mean
  // nothing.  An entry that waits for a filling step is not freed.
  void clear_at_drained_point() { std::fill(free_at.begin(), free_at.end(), 0); std::fill(read_from.begin(), read_from.end(), kLongAgo); }

  bool named_now(int e) const { return refs[(size_t)e] > 0; }                                             // (a)
  bool read_by_a_step(int e, long long ticks) const { return waits[(size_t)e] != 0 || ticks < free_at[(size_t)e]; }   // (b)
  bool busy(int e, long long ticks, modes::Mode m) const { return named_now(e) || (rule_b_applies(m) && read_by_a_step(e, ticks)); }

 private:
  void last_name_gone(int e, const Clock& c, bool next_step_too) {
    if (c.filling && !next_step_too) {
      if (!waits[(size_t)e]) { waits[(size_t)e] = 1; waiting.push_back(e); }
      return;
    }
    // (an entry that still waits keeps waiting: a name that came and went inside the feed does not shorten it)
    free_at[(size_t)e] = (next_step_too ? c.tick : std::max(c.last_feed_tick, read_from[(size_t)e])) + c.stages;
  }
};

}  // namespace sentry
}  // namespace bhip
