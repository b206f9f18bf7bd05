// tick_order_plan.h -- the dispatch ORDER of a table launch (fuse.hip.h; the batch's tick): which workgroup sits at which index, for a full
// tick, for a fill's or a drain's range of stages, and which of those lists a tick takes.  Host arithmetic over plain span rows, no HIP:
// fuse::TableBuilder collects the rows, batch_tick.hip.h uploads what comes back, tests/test_cpu_tick_order_plan.py checks it without a GPU.
#pragma once
#include <cstddef>
#include <vector>

namespace fuse {

struct Span { int first, gx, type, arg; };  // workgroups [first, next first) run body `type` with its argument block `arg`
constexpr int kMaxSpans = 64;
// (bits 16-23 of Span::arg: the body's pipeline stage, see StepPairs)
constexpr int kMaxStepPairs = 32;   // pipeline stages a launch carries {step counter, I/O slot} pairs for (StepPairs, fuse.hip.h)
// One workgroup of a launch whose dispatch ORDER is free (Table::desc): body type, argument block | stage << 16 (as Span::arg),
// the workgroup's index inside its body, the body's grid x-extent.  With a descriptor per workgroup the order is free:
// two_halves() puts every body with weights on one half of the chip.
struct WgDesc { int type, arg, local, gx; };

// One body as the order sees it.  cost: estimated time of ALL its workgroups (us, from the launch's timelines); pinned / group: two_halves
struct SpanRow { int type, arg, gx, n_wg; double cost; bool pinned; int group; };
static inline int stage_of(int arg) { return (arg >> 16) & 0xff; }

// the workgroups in the order the bodies were added (every body a contiguous run)
static inline std::vector<WgDesc> in_span_order(const SpanRow* rows, int n_rows) {
  std::vector<WgDesc> out;
  for (int i = 0; i < n_rows; ++i)
    for (int w = 0; w < rows[i].n_wg; ++w) out.push_back(WgDesc{rows[i].type, rows[i].arg, w, rows[i].gx});
  return out;
}
// Two HALVES of the chip.  Workgroup i of a launch runs on XCD i % 8 (observed; used for speed only), so the indices with
// i % 8 < 4 and those with i % 8 >= 4 are two queues, four XCDs each.  A body flagged `pinned` goes whole into ONE queue (the
// one with less estimated time so far, cost; spans that name the same `group` >= 0 share a queue: the linked GRU cells of a
// step's hops), so its weights pass through four of the eight L2s instead of all of them; the other bodies are dealt to both
// queues, more to the one that is behind.  Order inside a queue = the order added.  The launch's memory-side traffic falls by
// half the pinned bodies' weights x 8 (profiles/r05_notes.md); what it may cost is balance: the two halves no longer share one
// queue of work.
// stage_lo .. stage_hi: only the bodies of these stages (a partly filled tick's list, balanced over the halves for what it holds)
struct QueueItem { int span, local; };   // workgroup `local` of rows[span]
struct Queues { std::vector<QueueItem> q[4]; };
static inline Queues halves_queues(const SpanRow* rows, int n_rows, const int NQ, const int stage_lo, const int stage_hi) {
  Queues out;
  double load[4] = {0, 0, 0, 0};
  int group_q[kMaxSpans];
  for (int& g : group_q) g = -1;
  auto lightest = [&]() { int h = 0; for (int x = 1; x < NQ; ++x) if (load[x] < load[h]) h = x; return h; };
  for (int i = 0; i < n_rows; ++i) {
    const SpanRow& r = rows[i];
    if (stage_of(r.arg) < stage_lo || stage_of(r.arg) > stage_hi) continue;
    const double c = r.n_wg > 0 ? r.cost / r.n_wg : 0.0;
    if (r.pinned) {
      int h = lightest();
      if (r.group >= 0 && r.group < kMaxSpans) { if (group_q[r.group] >= 0) h = group_q[r.group]; else group_q[r.group] = h; }
      for (int w = 0; w < r.n_wg; ++w) out.q[h].push_back(QueueItem{i, w});
      load[h] += r.cost;
    } else {
      for (int w = 0; w < r.n_wg; ++w) { const int h = lightest(); out.q[h].push_back(QueueItem{i, w}); load[h] += c; }
    }
  }
  return out;
}
// ... and the queues laid over the launch's indices
static inline std::vector<WgDesc> two_halves(const SpanRow* rows, int n_rows, const int NQ = 2 /* queues: 2 halves or 4 quarters of the chip */,
                                             const int stage_lo = 0, const int stage_hi = 255) {
  const Queues queues = halves_queues(rows, n_rows, NQ, stage_lo, stage_hi);
  const std::vector<QueueItem>* q = queues.q;
  std::vector<WgDesc> out;
  auto emit = [&](const QueueItem& x) { const SpanRow& r = rows[x.span]; out.push_back(WgDesc{r.type, r.arg, x.local, r.gx}); };
  size_t at[4] = {0, 0, 0, 0};
  auto all_have = [&]() { for (int h = 0; h < NQ; ++h) if (at[h] >= q[h].size()) return false; return true; };
  while (all_have()) {   // 8 / NQ consecutive indices (= XCDs) for each queue in turn
    for (int h = 0; h < NQ; ++h)
      for (int j = 0; j < 8 / NQ; ++j) {
        if (at[h] < q[h].size()) emit(q[h][at[h]++]);
        else out.push_back(WgDesc{-1, 0, 0, 1});   // (a filler index: that slot's turn passes)
      }
  }
  for (bool more = true; more;) {   // (the longer queues' rests go to all eight XCDs, round-robin)
    more = false;
    for (int h = 0; h < NQ; ++h) if (at[h] < q[h].size()) { emit(q[h][at[h]++]); more = true; }
  }
  return out;
}

// The plain order with the workgroups of EMPTY stages left out, for the two shapes a fill and a drain go through: stages 0 .. k occupied
// (shape 0, entry k) and stages k .. last occupied (shape 1, entry k); one list, entry [shape][k] = all[off .. off + n).  A partly filled
// launch otherwise dispatches every stage's workgroups only for most of them to leave at once -- thousands of slot turns per launch in a
// run of few steps.  From range_halves_from occupied stages on (halves_mode != 0) an entry is the halves order worked out for exactly the
// stages it holds (round 6: a nearly full tick gains from the halves what a full one does; profiles/r06_notes.md section 9).  Very large
// tables (and plans with more stages than a launch carries pairs for) get none: every n = 0, the tick runs the plain list.
struct RangeIndex { size_t off[2][kMaxStepPairs] = {}; int n[2][kMaxStepPairs] = {}; };
struct RangeLists { std::vector<WgDesc> all; RangeIndex at; };
static inline RangeLists range_lists(const SpanRow* rows, int n_rows, const std::vector<WgDesc>& plain, int n_stages, int halves_mode, int range_halves_from) {
  RangeLists r;
  if (plain.size() > 16384 || n_stages > kMaxStepPairs) return r;
  for (int shape = 0; shape < 2; ++shape)
    for (int s0 = 0; s0 < n_stages; ++s0) {
      r.at.off[shape][s0] = r.all.size();
      const int occupied = shape == 0 ? s0 + 1 : n_stages - s0;
      if (halves_mode != 0 && occupied >= range_halves_from) {
        const std::vector<WgDesc> part = shape == 0 ? two_halves(rows, n_rows, 2, 0, s0) : two_halves(rows, n_rows, 2, s0, 255);
        r.all.insert(r.all.end(), part.begin(), part.end());
      } else {
        for (const WgDesc& d : plain)
          if (shape == 0 ? stage_of(d.arg) <= s0 : stage_of(d.arg) >= s0) r.all.push_back(d);
      }
      r.at.n[shape][s0] = (int)(r.all.size() - r.at.off[shape][s0]);
    }
  return r;
}

// The list of a partly filled tick.  hop[s] >= 0: stage s has a step in this launch.  Occupied stages 0 .. k: {0, k}; k .. last: {1, k};
// anything else (a hole, no stage, an entry that was not built): shape -1 = the plain list.  (All occupied: the caller's full tick.)
struct RangePick { int shape, at; };
static inline RangePick pick_range(const int* hop, int n_stages, const RangeIndex& ranges) {
  int lo = n_stages, hi = -1, occupied = 0;
  for (int s = 0; s < n_stages; ++s) if (hop[s] >= 0) { lo = s < lo ? s : lo; hi = s; ++occupied; }
  const int shape = occupied == 0 || occupied != hi - lo + 1 ? -1 : (lo == 0 ? 0 : (hi == n_stages - 1 ? 1 : -1));
  const int at = shape == 0 ? hi : lo;
  return shape >= 0 && at < kMaxStepPairs && ranges.n[shape][at] > 0 ? RangePick{shape, at} : RangePick{-1, 0};
}

}  // namespace fuse
