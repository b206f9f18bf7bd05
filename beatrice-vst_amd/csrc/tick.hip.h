// tick.hip.h -- "tick" pipelining of the batch: every LAYER of the per-hop chain is its own pipeline stage.
// (Included by batch.hip after struct BeatriceBatch; not a stand-alone header.)
//
// Why: at a few hundred streams a step is a string of ~40 dependent, latency-bound launches, each using a fraction of
// the chip for 4-9 us.  Streams never exchange data and every mutable thing is per-stream
// state, so consecutive steps can overlap as long as stage s of step t+1 runs after stage s of step t.  A tick is ONE
// launch in which stage s works on step (tick - s): ~1900 independent workgroups of 26 different steps fill the chip, and
// the only synchronisation is the kernel boundary between ticks.  Outputs are bit-identical to the in-order chain: the same
// kernel bodies run on the same data, only later.  A step's output appears n_stages - 1 ticks after its input was
// fed; BeatriceBatch_Synchronize drains the pipeline.  For callers that enqueue steps ahead of their completion
// (resident audio); a server that needs each hop back before the next runs the in-order chain.
//
// What makes it safe:
//   * every ring a LATER stage reads holds one more step slot than the in-order chain needs (State::create with
//     pipe_slack; the block scratch xa, read again four stages on, holds five), the small non-ring outputs of the pitch
//     head are double-buffered by step parity;
//   * each stage has its own {step counter, I/O slot} pair, computed by the host (which knows the step every stage is
//     at) and passed to the launch BY VALUE (fuse::StepPairs in the kernel arguments; a workgroup leaves its body's pair
//     in LDS, ring.h stepc): no launch to publish counters, no dependent global load at the start of a workgroup;
//     -1 = "no step this tick" (fill, drain);
//   * per-stream settings are versioned: a change goes once into a slot of a snapshot ring on the device (staged in a
//     ring of pinned host copies and fetched by the prologue kernel itself), and the same prologue kernel copies the
//     byte range a consumer stage reads from its step's snapshot into that stage's private arrays at the tick the step
//     arrives there (consumers: k-NN, pitch head, conditioning mix, the attention half of each block).
#pragma once
#include <tuple>
#include <type_traits>
#include <utility>

#include "chain_layers.hip.h"
#include "fuse.hip.h"
#include "hip_owned.h"
#include "rowchain.hip.h"
#include "tail_stages.hip.h"
#include "tick_reset.hip.h"

namespace tick {

constexpr int kRangeHalvesFrom = 99;   // a partly filled tick with at least this many occupied stages runs in its own halves order (99: none does)
constexpr int kMaxStages = fuse::kMaxStepPairs, kRing = 64, kMaxCopies = 16;  // (copies: 7 consumers + the snapshot upload)

struct Copy { unsigned char* dst; const unsigned char* src; int bytes; };
constexpr int kCopyChunk = 4096;  // bytes one workgroup moves (256 lanes x 16 bytes, one round trip)
struct Prolog {
  int n_stages;
  int hop[kMaxStages], io[kMaxStages];
  int n_copies;
  Copy copy[kMaxCopies];
  int first_chunk[kMaxCopies + 1];  // workgroups [first_chunk[c], first_chunk[c + 1]) perform copy c
};
// Settings traffic of a tick, one launch (only on ticks that have any): entry 0 may be the upload of a new snapshot --
// its source is PINNED HOST memory, read by the kernel itself over PCIe (a copy command in the stream costs a switch to the
// copy engine and back, ~40 us per tick when settings change every step) -- the others move a consumer stage's byte range
// from an OLDER snapshot slot into that stage's private copy.  One workgroup per 4 KB.
static __global__ __launch_bounds__(256) void prologue_kernel(const Prolog p) {
  int c = 0;
  while (c + 1 < p.n_copies && (int)blockIdx.x >= p.first_chunk[c + 1]) ++c;
  const Copy cp = p.copy[c];
  const int at = ((int)blockIdx.x - p.first_chunk[c]) * kCopyChunk + (int)threadIdx.x * 16;
  if (at + 16 <= cp.bytes) *reinterpret_cast<uint4*>(cp.dst + at) = *reinterpret_cast<const uint4*>(cp.src + at);  // (ranges are multiples of 16 bytes)
}

using namespace bhip;
using namespace wave_layers;
// Tilings of the tick launch.  Everything runs in 512-thread workgroups, two per CU (<= 128 VGPRs, <= 78 KB of LDS): the
// stream-stationary bodies (conditioned blocks as two row-local chains each, rowchain.hip.h; the fused upsampler tail)
// and the remaining layers as rc::conv_rows_body: 32 rows (two MFMA row tiles sharing every weight fragment) x the layer's
// width (the three 256-column layers with long reductions: 128-column slabs) per workgroup, the A operand streamed through
// LDS one 256-long reduction segment at a time, weights prefetched four to eight k-blocks ahead.  A tick wants MFMA density
// and occupancy, not the shortest dependent chain: per-layer launches with 16x32 tiles and 128-wide k-chunks (the in-order
// chain's choice) measured 0.224 ms per tick at 256 streams, 16x64 tiles in 256-thread workgroups 0.104, this layout 0.078.
// (Measured at 256 / 1024 streams: one row tile, full width 3.18 / 3.83 M frames/s; the three long
//  layers as 32 rows x 128 columns 3.27 / 3.85; every conv_rows body with two row tiles 3.29 / 3.98)
constexpr int kRbCols = 128;   // column slab of the three long layers (f4, f5, rb)
constexpr int kMidRt = 2, kRbRt = 2, kP1Rt = kMidRt;   // row tiles of 16 per workgroup
// (phone.f3 with ONE row tile: it runs in the launch's second round, where short workgroups matter more than traffic --
//  32 workgroups of 28 us end the launch later than 64 of 18 us: 3.45 -> 3.55 M frames/s at 256 streams)
constexpr int kF3Rt = 1;

// The sparse table exists at one hop per step only (batch_tick.hip.h tick_run: measured no gain at two hops, a loss at four)
constexpr bool sparse_table_at(int H) { return H == 1; }

enum BodyType {
  T_F1, T_FFT, T_F2, T_F3, T_F4, T_F5, T_P1, T_RB, T_P23, T_POUT, T_HEAD, T_OUT, T_COND, T_INP, T_UP1, T_RES1A, T_RES1B, T_UP2,
  T_QGRU, T_PGRU, T_VQ, T_TAIL1, T_TAIL2, T_TAIL3, T_BLKA1, T_BLKA2, T_BLKA4, T_BLKA8, T_BLKB, T_BLKBQ,
  T_F4S, T_F5S, T_RBS, T_P1S, T_UP1S, T_TAIL1S, T_TAIL2S, T_QGRU1, T_PGRU1, T_QGRUM, T_PGRUM, T_COUNT
};
// What the host knows of a body type whatever the hops per step: the ONE list a new type is entered in (the enum above gives it its
// number, Ops<H>::L below its kernel body; both are checked against this list when they are compiled).
// Placement on the halves of the chip (fuse::two_halves): the bodies with the weights go whole to one half; the GRU cells of a step's
// hops, linked inside the launch, share one.  A type states its class: there is no default.
enum Placement { kDealt /* hardly any weights: dealt to both halves */, kPinned, kPinnedPhoneGru /* group 0 */, kPinnedPitchGru /* group 1 */ };
struct Body {
  BodyType type;
  const char* name;   // profile name
  int cap;            // bodies of the type a table may hold (its argument bank)
  Placement place;
  BodyType sparse;    // the type's form in the sparse table (itself: the same body in both -- the default)
  bool spread;        // per-stream bodies asked for on all eight XCDs (what kDealt does: checked below)
  constexpr Body(BodyType t, const char* n, int c, Placement p, BodyType s = T_COUNT, bool sp = false) : type(t), name(n), cap(c), place(p), sparse(s == T_COUNT ? t : s), spread(sp) {}
};
constexpr Body kBodies[] = {
    {T_F1, "phone.f1", 1, kDealt}, {T_FFT, "pitch.fft", 1, kDealt}, {T_F2, "phone.f2", 1, kPinned}, {T_F3, "phone.f3", 1, kPinned},
    {T_F4, "phone.f4", 1, kPinned, T_F4S}, {T_F5, "phone.f5", 1, kPinned, T_F5S}, {T_P1, "pitch.p1", 1, kPinned, T_P1S}, {T_RB, "phone.rb", 4, kPinned, T_RBS},
    {T_P23, "pitch.p23", 2, kPinned}, {T_POUT, "pitch.out", 1, kPinned}, {T_HEAD, "pitch.head", 1, kDealt}, {T_OUT, "phone.out", 1, kPinned},
    {T_COND, "wave.cond", 1, kDealt}, {T_INP, "wave.inp", 1, kPinned}, {T_UP1, "wave.up1", 1, kPinned, T_UP1S}, {T_RES1A, "wave.res1a", 1, kPinned},
    {T_RES1B, "wave.res1b", 1, kPinned}, {T_UP2, "wave.up2", 1, kPinned}, {T_QGRU, "pitch.gru", 1, kPinnedPitchGru}, {T_PGRU, "phone.gru", 1, kPinnedPhoneGru},
    {T_VQ, "phone.vq", 1, kDealt, T_COUNT, true}, {T_TAIL1, "wave.tail1", 1, kDealt, T_TAIL1S, true}, {T_TAIL2, "wave.tail2", 1, kDealt, T_TAIL2S, true},
    {T_TAIL3, "wave.tail3", 1, kDealt, T_COUNT, true}, {T_BLKA1, "wave.blk.a", 1, kPinned}, {T_BLKA2, "wave.blk.a", 1, kPinned},
    {T_BLKA4, "wave.blk.a", 1, kPinned}, {T_BLKA8, "wave.blk.a", 1, kPinned}, {T_BLKB, "wave.blk.b", 4, kPinned}, {T_BLKBQ, "wave.blk.bq", 4, kPinned},
    {T_F4S, "phone.f4", 1, kPinned}, {T_F5S, "phone.f5", 1, kPinned}, {T_RBS, "phone.rb", 4, kPinned}, {T_P1S, "pitch.p1", 1, kPinned},
    {T_UP1S, "wave.up1", 1, kPinned}, {T_TAIL1S, "wave.tail1", 1, kDealt, T_COUNT, true}, {T_TAIL2S, "wave.tail2", 1, kDealt, T_COUNT, true},
    {T_QGRU1, "pitch.gru", 1, kPinnedPitchGru}, {T_PGRU1, "phone.gru", 1, kPinnedPhoneGru}, {T_QGRUM, "pitch.gru", 2, kPinnedPitchGru}, {T_PGRUM, "phone.gru", 2, kPinnedPhoneGru}};
constexpr bool bodies_in_order() {
  for (int i = 0; i < T_COUNT; ++i) {
    const Body& b = kBodies[i], & s = kBodies[b.sparse];
    if (b.type != i || s.sparse != s.type || s.cap != b.cap || s.place != b.place || (b.spread && b.place != kDealt)) return false;
  }
  return true;
}
static_assert(sizeof(kBodies) / sizeof(kBodies[0]) == T_COUNT && bodies_in_order(), "kBodies: one entry per BodyType, in the enum's order; a sparse form is placed like its full one");
static_assert(T_COUNT <= 64, "TableBuilder::only, BeatriceBatchMeas_TickOnlyTypes: a type is a bit of a 64-bit mask");
// a row of Ops<H>::L: the kernel body that runs type T at H hops per step
template <BodyType T, class Op> struct Row { static constexpr BodyType type = T; using op = Op; };

// The bodies of a tick with H hops per stage (H = 1: a step is one 10 ms hop of every stream; H = 2: two -- every stage then
// works on twice the rows per weight fragment and per launch, and a launch's fixed costs are paid once per two hops; the two
// recurrent layers run their two hops one after the other inside a workgroup).  Same layer types as the in-order chain at H hops
// per step: rows are (stream, frame of the step), the recurrences (GRU, pitch head, the tail's histories) run in frame order.
template <int H>
struct Ops {
  using PL = PhoneLayers<H>;
  using QL1 = PitchLayers<H>;
  using OpF2 = rc::ConvRowsOp<typename PL::F2, 0, kMidRt>;
  using OpF3 = rc::ConvRowsOp<typename PL::F3, 0, kF3Rt>;
  using OpF4 = rc::ConvRowsOp<typename PL::F4, kRbCols, kRbRt>;
  using OpF5 = rc::ConvRowsOp<typename PL::F5, kRbCols, kRbRt>;
  using OpRB = rc::ConvRowsOp<typename PL::RBL, kRbCols, kRbRt>;
  using OpOUT = rc::ConvRowsOp<typename PL::OUTL>;
  using OpP1 = rc::ConvRowsOp<typename QL1::P1, 0, kP1Rt>;
  using OpP23 = rc::ConvRowsOp<typename QL1::P23>;
  using OpPOUT = rc::ConvRowsOp<typename QL1::POUT>;
  using OpINP = rc::ConvRowsOp<INP<H>>;
  using OpUP1 = rc::ConvRowsOp<UP<256, 128, 5, H>, 128, kMidRt>;   // 640 columns: five slabs
  using OpRES1A = rc::ConvRowsOp<RES<128, 1, 5 * H>, 0, kMidRt>;
  using OpRES1B = rc::ConvRowsOp<RES<128, 3, 5 * H>, 0, kMidRt>;
  using OpUP2 = rc::ConvRowsOp<UP<128, 64, 4, 5 * H>, 0, kMidRt>;
  // The SPARSE table (the first ticks of a fill, while only front-end stages have a step): the bodies whose workgroups last longest
  // in half-size pieces -- one row tile per convolution workgroup (and half the streams per tail workgroup, unused: see tick_run).  A
  // partly filled launch lasts as long as its longest workgroup and has idle slots to spare, so shorter workgroups in larger
  // numbers are what it wants (in a full tick they cost ~3 %: twice the weight traffic per row, more prologues).  Same arithmetic,
  // same rings: a tick may use either table.  Where no sparse table is ever built (sparse_table_at) the types keep their places in
  // the list as fuse::Absent: the table kernels of that H hold none of their code.
  template <class Op> using Sparse = std::conditional_t<sparse_table_at(H), Op, fuse::Absent<Op>>;
  using OpF4s = Sparse<rc::ConvRowsOp<typename PL::F4, kRbCols, 1>>;
  using OpF5s = Sparse<rc::ConvRowsOp<typename PL::F5, kRbCols, 1>>;
  using OpRBs = Sparse<rc::ConvRowsOp<typename PL::RBL, kRbCols, 1>>;
  using OpP1s = Sparse<rc::ConvRowsOp<typename QL1::P1, 0, 1>>;
  using OpUP1s = Sparse<rc::ConvRowsOp<UP<256, 128, 5, H>, 128, 1>>;
  // the tail's stages: streams per workgroup so that a workgroup holds the same number of rows at every H (80 / 240 / 480; H = 2: T2 160).
  // H = 4: a stream's 320 / 960 frames of a step do not fit the LDS -- T2 and T3 run the step as two sub-steps of two hops, one after
  // the other inside the workgroup, the layers' histories carried in LDS (tail_stages.hip.h prologue / carry_histories)
  static constexpr int NSUB = H > 2 ? H / 2 : 1;
  using T1 = tst::T1OpS<(H == 1 ? tst::kT1Streams : (H == 2 ? 2 : 1)), H>;
  using T2 = tst::T2OpS<(H == 1 ? tst::kT2Streams : 1), H, NSUB>;
  using T3 = tst::T3OpS<(H == 1 ? tst::kT3Streams : 1), H, NSUB>;
  using T1s = Sparse<tst::T1OpS<(H == 1 ? 2 : 1), H>>;
  using T2s = Sparse<tst::T2OpS<(H == 1 ? 2 : 1), H, NSUB>>;
  // The GRUs: the rows cell (rowchain.hip.h gru_rows_body; 32 streams x 64 hidden units per workgroup, all three gates of a column
  // tile in one wavefront, the weights streamed).  Hop t of a step needs the whole state vector of hop t - 1: with several hops per step the cell of hop t PUBLISHES
  // its state as tagged granules and the cell of hop t + 1 -- another set of workgroups of the SAME launch and stage, later in
  // dispatch order (tick_build_table) -- polls them (GruArgs::link_*): the one place where workgroups of a tick wait for each other.
  // GruQ / GruP: hop 0 (publishes when H > 1); GruQm / GruPm: hops 1 .. H - 2 (poll and publish; H = 4: two of each, every link
  // its own granule array); GruQ1 / GruP1: the last hop (polls)
  static_assert(H <= 4, "link arrays: tick::State");
  // (one hop per step: both cells stay column-split -- there the cells sit at the END of the dispatch order, and 16-32 workgroups of
  //  17-25 us end the launch later than 64-128 of 9-12 us: 61.8 -> 68.9 us per tick at 256 streams, profiles/gru_rows_notes.md section 5)
  using GruQ = std::conditional_t<H == 1, GruOp<128, 128, 2, 0>, rc::GruRowsOp<128, 128, 1>>;
  // (the phone cell of hop 0 at four hops per step is the rows cell as well: the one VGPR spill it used to bring to the common four-hop
  //  kernel sat in the tail's T1 -- the operand of its output ring's `hop % m` -- and T1 now keeps that position as a scalar,
  //  tail_stages.hip.h res_res_up_body; profiles/tail_substeps_notes.md)
  using GruP = std::conditional_t<H == 1, GruOp<256, 256, 2, 0>, rc::GruRowsOp<256, 256, 1>>;
  using GruQ1 = std::conditional_t<H == 1, rc::NopOp, rc::GruRowsOp<128, 128, 2>>;
  using GruP1 = std::conditional_t<H == 1, rc::NopOp, rc::GruRowsOp<256, 256, 2>>;
  using GruQm = std::conditional_t<H <= 2, rc::NopOp, rc::GruRowsOp<128, 128, 3>>;
  using GruPm = std::conditional_t<H <= 2, rc::NopOp, rc::GruRowsOp<256, 256, 3>>;
  using Vq = std::conditional_t<H == 1, VqOp, VqRowsOp<H>>;   // (several hops: a stream's rows in one workgroup, the codebook read once)
  // The type list of the table kernels, in the enum's order (checked): position = BodyType = the type's bit in the measurement masks
  template <class... Rs> struct List {
    template <int... Is> static constexpr bool in_order(std::integer_sequence<int, Is...>) { return ((Rs::type == Is) && ...); }
    static_assert(sizeof...(Rs) == T_COUNT && in_order(std::make_integer_sequence<int, sizeof...(Rs)>{}), "Ops<H>::L: one Row per BodyType, in the enum's order");
    using Tab = fuse::Table<fuse::Many<typename Rs::op, kBodies[Rs::type].cap>...>;
    using Builder = fuse::TableBuilder<fuse::Many<typename Rs::op, kBodies[Rs::type].cap>...>;
    template <BodyType T> using Op = typename std::tuple_element_t<T, std::tuple<Rs...>>::op;
  };
  using L = List<
      Row<T_F1, F1Op2>, Row<T_FFT, FftOp2>, Row<T_F2, OpF2>, Row<T_F3, OpF3>, Row<T_F4, OpF4>, Row<T_F5, OpF5>, Row<T_P1, OpP1>, Row<T_RB, OpRB>,
      Row<T_P23, OpP23>, Row<T_POUT, OpPOUT>, Row<T_HEAD, HeadOp8>, Row<T_OUT, OpOUT>, Row<T_COND, CondOp2>, Row<T_INP, OpINP>, Row<T_UP1, OpUP1>,
      Row<T_RES1A, OpRES1A>, Row<T_RES1B, OpRES1B>, Row<T_UP2, OpUP2>, Row<T_QGRU, GruQ>, Row<T_PGRU, GruP>, Row<T_VQ, Vq>, Row<T_TAIL1, T1>,
      Row<T_TAIL2, T2>, Row<T_TAIL3, T3>, Row<T_BLKA1, rc::BlockAOp<1, H>>, Row<T_BLKA2, rc::BlockAOp<2, H>>, Row<T_BLKA4, rc::BlockAOp<4, H>>,
      Row<T_BLKA8, rc::BlockAOp<8, H>>, Row<T_BLKB, rc::BlockBOpH<H>>, Row<T_BLKBQ, rc::BlockBqOpH<H>>, Row<T_F4S, OpF4s>, Row<T_F5S, OpF5s>,
      Row<T_RBS, OpRBs>, Row<T_P1S, OpP1s>, Row<T_UP1S, OpUP1s>, Row<T_TAIL1S, T1s>, Row<T_TAIL2S, T2s>, Row<T_QGRU1, GruQ1>, Row<T_PGRU1, GruP1>,
      Row<T_QGRUM, GruQm>, Row<T_PGRUM, GruPm>>;
  using Tab = typename L::Tab;
  using Builder = typename L::Builder;
  template <BodyType T> using Op = typename L::template Op<T>;
};

// Stage of each body.  Front end: the in-order chain's launch order, the pitch estimator zipped into the content
// encoder's stages from the fourth launch on (its spectrum ring then has its reader one stage later, like every other
// ring).  A conditioned block is two stages (rowchain.hip.h).  The same plan at every number of hops per step.
struct Plan {
  static constexpr int F1 = 0, F2 = 1, F3 = 2, F4 = 3, FFT = 3, F5 = 4, P1 = 4, RB0 = 5, P2 = 5, QGRU = 7, POUT = 8, PGRU = 9, HEAD = 9,
                       OUT = 10, COND = 10, VQ = 11, INP = 12, BLK0 = 13;
  static constexpr int per_block = 2;  // stages per conditioned block
  int blk(int b) const { return BLK0 + per_block * b; }
  int up1() const { return blk(B_NBLOCKS); }
  int tail() const { return up1() + 4; }   // first of the tail's three stages (tail_stages.hip.h; the in-order chain's one-workgroup-per-stream
                                           // tail, wave_tail.hip.h, is no body of a tick: it shares only the state block's layout)
  int count() const { return tail() + 3; }
};
constexpr int kMaxHops = 4;   // hops per stage per tick the launch is built for (Ops<1>, Ops<2>, Ops<4>)
static_assert(Plan::BLK0 + Plan::per_block * B_NBLOCKS + 7 <= kMaxStages && kMaxStages + 2 <= kRing && kMaxStages <= fuse::kMaxStepPairs, "stage bookkeeping");

struct Consumer {  // a kernel that reads per-stream settings: its private copy of a byte range of the settings block
  int stage;
  size_t off, bytes;    // range in the settings snapshot
  unsigned char* dst;   // its private copy on the device
  int held;             // snapshot the private copy currently equals (-1: none)
};

struct State {
  bool on = false;
  DevBuf<unsigned char> d_table;         // Ops<H>::Tab on the device
  int table_total = 0;
  DevBuf<unsigned char> d_table_sparse;  // the same stages with the long bodies in half-size pieces (fill and drain ticks)
  int table_sparse_total = 0;
  double table_flops = 0, table_bytes = 0;  // algorithmic work of one full tick (sum over the bodies)
  DevBuf<fuse::WgDesc> d_desc;       // dispatch order of the full / the sparse table by workgroup (tick_build_table_h)
  DevBuf<fuse::WgDesc> d_desc_sparse;
  // the full table's workgroups in plain span order (every body on all eight XCDs): the order of PARTLY FILLED ticks -- with few stages
  // occupied a body confined to half the chip leaves the other half idle (a 20-step run: 3.78 -> 3.51 M frames/s with the halves everywhere)
  DevBuf<fuse::WgDesc> d_desc_plain;
  int table_total_plain = 0;
  // ... and the same order with the workgroups of EMPTY stages left out, for a fill's and a drain's shapes (fuse::RangeLists); one buffer
  DevBuf<fuse::WgDesc> d_desc_ranges;
  fuse::RangeIndex range;
  DevBuf<unsigned long long> d_trace;     // BEATRICE_HIP_TICK_TRACE=<file>: per-workgroup timeline of the last full tick
  bool table_dirty = true;
  DevBuf<unsigned char> d_snap;     // [kRing][snap_bytes] settings snapshots
  static constexpr int kStaging = 16;
  StagedRing<unsigned char> stage;  // [kStaging][snap_bytes]: a snapshot on its way to the device
  size_t snap_bytes = 0;
  long long tick = 0, n_fed = 0, last_feed_tick = -1000;
  long long fed_step[kRing];        // step fed at tick (index tick % kRing), -1 none
  int snap_of_step[kRing], hop_of_step[kRing], io_of_step[kRing];
  int snap_cur = -1, snap_next = 0;
  std::vector<Consumer> consumers;
  Plan plan;
  // Ragged steps (the shell's silent-block rule per stream, BeatriceBatch_SetSilentStreams in tick mode): a stream that sits a
  // step out does not advance -- so every stream has its OWN step counter from then on, and a step carries the counters of its
  // streams (-1: absent) through the stages, like its settings: [kRing][row] on the device, staged through pinned copies.
  bool ragged = false;
  int row = 0;                        // ints per step (B rounded up to a multiple of 4: the prologue copies 16-byte pieces)
  std::vector<int> hop_s;             // [B] the streams' counters on the host
  DevBuf<int> d_hopv;                 // [kRing][row]
  StagedRing<int> hopv;               // [kStaging][row]: a step's counters on their way to the device
  bool step_ragged[kRing] = {};       // step u (at [u % kRing]) carries per-stream counters
  // back to one counter at a drained point (batch_tick.hip.h tick_relevel): the table of the batch's rings, the streams' deficits
  DevBuf<FreezeRing> d_ring_table;    // [n_ring_table]
  int n_ring_table = 0;
  DevBuf<int> d_shift;                // [B]
  // several hops per step: the granules that link the GRU cells of a step's hops inside a launch (fused_small.hip.h GruArgs::link_*)
  DevBuf<unsigned long long> d_link_q;      // [H - 1][B][128]: link t = hop t's state for hop t + 1
  DevBuf<unsigned long long> d_link_p;      // [H - 1][B][256]
  PinnedBuf<int> h_link_dead;               // a cell gave a wait up
  // Streams that start over inside the pipeline (BeatriceBatch_ResetStreamInFlight; tick_reset.hip.h, batch_tick.hip.h tick_reset_*)
  struct Travelling { int stream, counter; long long tick; };   // a reset on its way: the stream's counter of the step it applies to, the tick that step was fed in
  std::vector<unsigned char> reset_pending;   // [B] asked for; applies to the next step fed that the stream takes part in
  bool any_reset_pending = false;
  std::vector<Travelling> resets;
  DevBuf<ResetRing> d_reset_rings;            // [n_reset_rings] the pieces of the three arenas that have a window (+ the previous bin)
  int n_reset_rings = 0;
  std::vector<int> reset_stage;               // [n_reset_rings] cleared before this stage's tick of the step
  std::vector<unsigned char> reset_spare;     // [n_reset_rings] ... but for the slot the step itself has written
  std::vector<int> reset_m;                   // [n_reset_rings] the ring's slot count
  int reset_wrap_first = -1;                  // the rows of Wrap48State (hist_in, ztail, fpend; mode F, tick_reset_wrap48) are the table's last three
  static constexpr int kResetStaging = 8;
  StagedRing<int> reset_list;                 // [kResetStaging][reset_list_ints]: a tick's work list, read by the kernels in place
  size_t reset_list_ints = 0;
  long long reset_serial = 0, reset_launches = 0;   // lists written so far; ticks that carried a reset launch
  DevBuf<float> d_gru_keep;                   // [B][256] | [B][128]: the frame a restarted cell's state ring held before the step
};

}  // namespace tick
