// wrapper_turnover_plan.h -- the tap tables of a bound batch with clocks per stream (BeatriceBatch_BindResidentBlocksRagged) while streams
// change their rate INSIDE the binding (BeatriceBatch_SetStreamRateInFlight / RestartStreamInFlight, batch_wrappers.hip.h): which rate
// classes are live, where each one's two tables sit in the batch's tap buffer, when a place may be written again and when a buffer may be
// freed.  Plain C++17, no HIP: tests/test_cpu_wrapper_turnover_plan.py walks it with a stand-alone program under the sanitizers.
//
// The problem.  A call's per-stream record (wrapn::RagStream) names its two tap tables by FLOAT OFFSET into the tap buffer.  The record
// written at call k is read twice: by the input half, launched in call k, and by the output half, launched in call k + delay (or earlier,
// at a drain).  Both launches are handed whatever buffer is the batch's at THEIR launch time.  So from the moment a record is written until
// its output half has been launched, the offsets it names must hold the taps it was planned with, in every buffer the batch may hold.
//
// The rules that give that:
//   (1) A class keeps its place [off, off + floats) from the call that makes it until it is released.  Buffers only grow, and a new
//       buffer is filled with every held class at its old offset before it becomes the batch's: offsets are stable across buffers.
//   (2) A class is released -- its place free to be written again -- only when no stream is on it AND no record that may still be read names
//       it.  `last_ref` is the newest call issued while a stream was on the class; its output half is launched during call
//       last_ref + delay, i.e. while `calls` (the calls issued so far) <= last_ref + delay.  Release needs calls >= last_ref + delay + 2:
//       "delay + 1 calls have passed since a stream last used it" (one more than the launch order needs).  A class no call was issued under
//       -- set and left between two calls -- is named by no record and goes at once.
//   (3) Writes into the buffer are copies enqueued on the batch's stream, behind every launch enqueued so far.  A place is written only
//       while free, so the launches in front of the copy do not read it, and the launches behind it see the copy done.  (A copy still
//       pending from a class that came and went between two calls lands in free space or is overwritten by the later copy of the same
//       floats: the last copy enqueued over a float decides it.)
//   (4) A buffer that is replaced was handed only to launches already enqueued; no launch to come reads it.  Whether those launches have
//       RUN is not something call counts say: a replaced buffer (and its pinned staging) is kept until a drained point -- the unbind -- and
//       freed there.  Buffers at least double, so the kept ones together are smaller than the one in use.
//
// Every read stays in bounds: a record's table is [off_down or off_up, + 32 hi + 1) inside its class's place, the place lies inside
// [0, capacity) of the buffer it was made in (plan() only hands out such places), and every later buffer is at least as long (1).
//
// The bound on live classes: at most B classes have a stream on them.  Every other held class has last_ref in
// [calls - delay - 1, calls - 1] once reap() has run (2), and a call is issued under at most B classes: B * (delay + 1) more.
// live_bound() = B * (delay + 2).
#pragma once
#include <algorithm>
#include <vector>

namespace wturn {

constexpr int kMaxCapacity = 1 << 30;   // floats: offsets travel as int in the records

struct Slot {
  bool held = false;
  double rate = 0.0;
  int off = 0, floats = 0, n_down = 0;   // the place: the down table's n_down floats, then the up table
  int users = 0;                         // streams on this class
  long long joined = 0;                  // calls issued when its first present user came
  long long last_ref = -1;               // newest call issued under it (-1: none)
  int off_down() const { return off; }
  int off_up() const { return off + n_down; }
};

struct Place { int index = -1, off = 0, capacity = 0; bool grows = false; };   // index -1: no room below kMaxCapacity

class TapArena {
 public:
  int B = 0, delay = 0, capacity = 0;
  std::vector<Slot> slots;   // the index is the batch's class index while the binding stands

  void start(int streams, int delay_calls) { B = streams; delay = delay_calls; capacity = 0; slots.clear(); }
  // the classes the binding starts with, in the order of the buffer BeatriceBatch_ConfigureWrapperRates built: one after the other
  int add_initial(double rate, int n_down, int n_up, int users) {
    Slot s;
    s.held = true; s.rate = rate; s.off = capacity; s.n_down = n_down; s.floats = n_down + n_up; s.users = users;
    capacity += s.floats;
    slots.push_back(s);
    return (int)slots.size() - 1;
  }
  int live_bound() const { return B * (delay + 2); }
  int held() const { int n = 0; for (const Slot& s : slots) n += s.held ? 1 : 0; return n; }
  bool releasable(const Slot& s, long long calls) const { return s.held && s.users == 0 && (s.last_ref < 0 || calls >= s.last_ref + delay + 2); }
  void reap(long long calls) { for (Slot& s : slots) if (releasable(s, calls)) s.held = false; }
  // a held class of that rate: its place is intact, with or without streams on it
  int find(double rate) const {
    for (size_t i = 0; i < slots.size(); ++i) if (slots[i].held && slots[i].rate == rate) return (int)i;
    return -1;
  }
  // where a class of `floats` floats would go, on the arena as it stands (reap first): the first gap between the held places that takes
  // it, else behind the last one in a buffer of at least twice the length.  Nothing is changed: commit() does that once the caller has
  // the buffer.
  Place plan(int floats) const {
    Place p;
    std::vector<std::pair<int, int>> taken;
    for (const Slot& s : slots) if (s.held) taken.emplace_back(s.off, s.off + s.floats);
    std::sort(taken.begin(), taken.end());
    int at = 0;
    for (const std::pair<int, int>& t : taken) {
      if (t.first - at >= floats) break;
      at = std::max(at, t.second);
    }
    if (floats < 1 || floats > kMaxCapacity - at) return p;
    p.off = at;
    p.grows = at + floats > capacity;
    p.capacity = capacity;
    if (p.grows) {
      long long want = std::max<long long>(2LL * capacity, (long long)at + floats);
      p.capacity = (int)std::min<long long>(want, kMaxCapacity);
    }
    for (size_t i = 0; i < slots.size() && p.index < 0; ++i) if (!slots[i].held) p.index = (int)i;
    if (p.index < 0) p.index = (int)slots.size();
    return p;
  }
  void commit(const Place& p, double rate, int n_down, int n_up) {
    if (p.index == (int)slots.size()) slots.emplace_back();
    Slot& s = slots[p.index];
    s = Slot{};
    s.held = true; s.rate = rate; s.off = p.off; s.n_down = n_down; s.floats = n_down + n_up;
    capacity = p.capacity;
  }
  // a stream comes to / leaves class i between two calls, `calls` issued so far
  void join(int i, long long calls) {
    Slot& s = slots[i];
    if (s.users++ == 0) s.joined = calls;
  }
  void leave(int i, long long calls) {
    Slot& s = slots[i];
    if (--s.users > 0) return;
    if (calls > s.joined) s.last_ref = calls - 1;
    if (s.last_ref < 0) s.held = false;
  }
};

}  // namespace wturn
