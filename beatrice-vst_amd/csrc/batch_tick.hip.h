// batch_tick.hip.h -- the batch's tick mode: the workgroup table of one tick, the per-tick host work (settings snapshots, step pairs, launch), drain, enable / leave
// (Part of batch.hip's translation unit: included there, after struct BeatriceBatch and the helpers above it; not a stand-alone header.)
#pragma once

// ---- tick pipelining (tick.hip.h) ---------------------------------------------------------------------------------
#ifdef BEATRICE_HIP_MEASUREMENT_BUILD
// MEASUREMENT BUILDS ONLY (results are wrong by construction): the tick launch with only the body TYPES of this mask (tick::BodyType
// bit numbers), for per-body instruction counters (tools/debug/tick_inst_by_body.py); BeatriceBatchMeas_TickOnlyTypes below
static unsigned long long g_tick_only_types = ~0ull;
#endif
// One table under construction.  A body is added by naming its type: the kernel body, the profile name, the argument bank and the
// placement on the halves of the chip come from tick.hip.h's lists (kBodies, Ops<H>::L)
template <class Op, class A> static inline auto tick_body_info(const char* name, const A& a, int) -> decltype(Op::info(name, a)) { return Op::info(name, a); }
template <class Op, class A> static inline auto tick_body_info(const char*, const A& a, long) -> decltype(Op::info(a)) { return Op::info(a); }   // (the op names itself)
template <int H>
struct TickTable {
  using O = tick::Ops<H>;
  std::unique_ptr<typename O::Builder> tb = std::make_unique<typename O::Builder>();
  bool sparse = false;
  int drop = 0;   // measurement builds: BEATRICE_HIP_TICK_DROP
  bool keep(int group) const { return ((drop >> group) & 1) == 0; }
  // ... with work figures and a grid stated at the site (the bodies whose ops have no info() / grid())
  template <tick::BodyType T, class Args>
  void add_as(const bhip::LaunchInfo& info, const Args& a, dim3 grid, int stage, bool on, double wg_cost) {
    constexpr tick::Placement place = tick::kBodies[T].place;
    tb->template add<T>(info, a, grid, stage, on, wg_cost, place != tick::kDealt, place == tick::kPinnedPhoneGru ? 0 : (place == tick::kPinnedPitchGru ? 1 : -1));
  }
  // (a type with a sparse form -- one row tile per workgroup, tick.hip.h -- goes into the sparse table in that form)
  template <tick::BodyType T, class Args>
  void add_body(const Args& a, int stage, int drop_group, double wg_cost) {
    using Op = typename O::template Op<T>;
    if (sparse && tick::kBodies[T].sparse != T) return add_body<tick::kBodies[T].sparse>(a, stage, drop_group, wg_cost);
    add_as<T>(tick_body_info<Op>(tick::kBodies[T].name, a, 0), a, Op::grid(a), stage, keep(drop_group), wg_cost);
  }
};
// A GRU cell of the tick: one description for every hop of a step and every H.  T0 / TM / TL: the types of hop 0, of the hops between
// and of the last hop (tick.hip.h GruQ / GruQm / GruQ1); link: [H - 1][B][width] granules between the hops
template <tick::BodyType T0, tick::BodyType TM, tick::BodyType TL>
struct TickGruCell {
  Ring x, h;
  const float *wih, *whh, *bih, *bhh;
  unsigned long long* link;
  int width, stage;
  double cost0, cost;   // time of a workgroup of hop 0 / of the later hops (us): what two_halves balances on
  int* link_dead;
  int passes;
  template <int H>
  void add(TickTable<H>& tt, int B, int t) const {
    auto at = [&](int u) { return link + (size_t)u * B * width; };
    const GruArgs g{x, h, wih, whh, bih, bhh, nullptr, B, t, t + 1 < H ? at(t) : nullptr, t > 0 ? at(t - 1) : nullptr, H > 1 ? link_dead : nullptr, passes};
    if (t == 0) tt.template add_body<T0>(g, stage, 1, cost0);
    else if constexpr (H > 1) {
      if (t == H - 1) tt.template add_body<TL>(g, stage, 1, cost);
      else if constexpr (H > 2) tt.template add_body<TM>(g, stage, 1, cost);
    }
  }
};
template <int H>
bool tick_build_table_h(BeatriceBatch* b, const bool sparse) {
  using namespace tick;
  using O = Ops<H>;
  using Tab = typename O::Tab;
  State& k = b->tk;
  if (sparse && !sparse_table_at(H)) { k.table_sparse_total = 0; return true; }   // (no tick of this H runs it: tick_run; its types are fuse::Absent)
  TickTable<H> tt;
  tt.sparse = sparse;
  const auto& tb = tt.tb;
  const PhoneWeights& pw = b->phone_m->w;
  const PitchWeights& qw = b->pitch_m->w;
  const WaveWeights& ww = b->wave_m->w;
  const PhoneState& ps = b->phone;
  const PitchState& qs = b->pitch;
  const WaveState& ws = b->wave;
  const int B = b->B;
  const Plan pl = k.plan;
  // measurement aid, MEASUREMENT BUILDS ONLY (tools/debug/build_variant.sh <name> -DBEATRICE_HIP_MEASUREMENT_BUILD; the
  // product library has no switch that changes results): BEATRICE_HIP_TICK_DROP=<bit mask> leaves groups of bodies out of
  // the launch (the group numbers at the add_body calls)
#ifdef BEATRICE_HIP_MEASUREMENT_BUILD
  static const int drop = bhip::meas_env("BEATRICE_HIP_TICK_DROP") ? std::atoi(bhip::meas_env("BEATRICE_HIP_TICK_DROP")) : 0;
  tt.drop = drop;
  tb->only = g_tick_only_types;
#endif
  // (every body takes its step counter from the launch's StepPairs -- a null counter pointer says so, ring.h stepc)
  auto conv = [&](const Ring& in, const Ring& out, const float* w, const float* bias) { return conv_args(in, out, w, bias, nullptr, B); };
  // (workgroups are dispatched in this order: the longest-running bodies first)
  // The GRU cells of a step's hops, linked inside the launch (tick.hip.h): hop 0 publishes into link 0, hop t polls link t - 1 and
  // publishes into link t, the last hop only polls.  A cell must find its predecessor's states published when it starts (it holds a
  // slot while it waits), so the hops sit far apart in dispatch order: hop 0 ahead of every other body, the later ones at the points
  // marked gru_at() below, each behind at least one more round of the launch's workgroups.
  // (GruArgs::passes, the column-split cells only -- both cells at one hop per step: two row groups per workgroup from 512
  //  streams on; BEATRICE_HIP_GRU_PASSES overrides, for measurements.  The rows cells stream their weights and ignore it)
  // time of a rows cell's workgroup (us; the means of a full four-hop tick's timeline at 256 streams, profiles/gru_rows_notes.md
  // section 6: phone 23.8 / 25.9, pitch 11.0 / 20.0 / 15.8 by hop): what two_halves balances on
  // (two hops per step: no timeline taken; with the pitch cell at 17 the tick measured 109.1 -> 113.6 us against the parent, at 14
  //  108.4 -> 107.2, section 5 of the notes: the halves' balance there is the one that 14 gives)
  constexpr double kGruRowsCostP = 25, kGruRowsCostQ = H == 2 ? 14 : 17;
  static const int gru_passes_env = bhip::meas_env("BEATRICE_HIP_GRU_PASSES") ? std::atoi(bhip::meas_env("BEATRICE_HIP_GRU_PASSES")) : 0;
  const int gru_passes = gru_passes_env > 0 ? gru_passes_env : (B >= 512 ? 2 : 1);
  // (hop 0: the column-split cells at one hop per step, 19 / 12 us; at two and four hops every cell is the rows cell, tick.hip.h GruP / GruQ.
  //  The hop-0 phone cell at FOUR hops: its workgroups last 16 us (hop 0 polls nothing), but the figure is the WEIGHT of the phone cells'
  //  half of the chip in two_halves, and where the other pinned bodies land moves the launch by more than the cell is worth -- 256 x 4
  //  with 12 / 25 / 38 / 50 / 76: 200.7 / 206.7 / 201.4 / 201.7 / 200.4 us against the parent's 203.4.  76 = 19 x 128 / 32 is the
  //  column-split cell's total over the rows cell's 32 workgroups (38 from 512 streams on, where that cell walked two row groups per
  //  workgroup and weighed half as much per stream): every other body stays on the half that the order had it on with the column-split
  //  cell; profiles/tail_substeps_notes.md section 4.  BEATRICE_HIP_GRU_COST0, measurement builds: that scan's knob)
  const double gru_cost0_p = H == 1 ? 19 : (H == 2 ? kGruRowsCostP : (B >= 512 ? 38 : 76));
  static const double gru_cost0_env = bhip::meas_env("BEATRICE_HIP_GRU_COST0") ? std::atof(bhip::meas_env("BEATRICE_HIP_GRU_COST0")) : 0.0;
  const TickGruCell<T_PGRU, T_PGRUM, T_PGRU1> pgru{ps.rb[3], ps.h, pw.gru_wih, pw.gru_whh, pw.gru_bih, pw.gru_bhh, k.d_link_p, 256, Plan::PGRU,
                                                  gru_cost0_env > 0 ? gru_cost0_env : gru_cost0_p, kGruRowsCostP, k.h_link_dead, gru_passes};
  const TickGruCell<T_QGRU, T_QGRUM, T_QGRU1> qgru{qs.p[2], qs.h, qw.gru_wih, qw.gru_whh, qw.gru_bih, qw.gru_bhh, k.d_link_q, 128, Plan::QGRU,
                                                  H == 1 ? 12 : kGruRowsCostQ, kGruRowsCostQ, k.h_link_dead, gru_passes};
  auto add_pgru = [&](int t) { pgru.add(tt, B, t); };
  auto add_qgru = [&](int t) { qgru.add(tt, B, t); };
  // gru_at(point): the hops placed at insertion point 0 (behind the conditioned blocks), 1 (behind the tail), 2 / 3 (where the second
  // hop of a two-hop step has always been: behind phone.f2 / wave.inp).  H = 1: the only hop at 2 (phone) and 3 (pitch), at the END of the
  // dispatch order; H = 2: hop 1 at 2 and 3; H = 4: hops 1, 2 at 0, 1 and hop 3 at 2 / 3
  auto gru_at = [&](int point) {
    if constexpr (H <= 2) { if (point == 2) add_pgru(H - 1); if (point == 3) add_qgru(H - 1); }
    if constexpr (H == 4) {
      if (point == 0) { add_pgru(1); add_qgru(1); }
      if (point == 1) { add_pgru(2); add_qgru(2); }
      if (point == 2) add_pgru(3);
      if (point == 3) add_qgru(3);
    }
  };
  if constexpr (H > 1) { add_pgru(0); add_qgru(0); }
  // ---- longest workgroups first (measured, two per CU): f5 48 us, p1 46, f4 45, rb 42, block halves 41 / 38, tail 36
  // (the sparse table: these in one row tile per workgroup, tick.hip.h)
  tt.template add_body<T_F5>(conv(ps.f[3], ps.f[4], pw.f_w[3], pw.f_b[3]), Plan::F5, 6, 30);
  tt.template add_body<T_P1>(conv(qs.spec, qs.p[0], qw.p_w[0], qw.p_b[0]), Plan::P1, 2, 41);
  tt.template add_body<T_F4>(conv(ps.f[2], ps.f[3], pw.f_w[2], pw.f_b[2]), Plan::F4, 6, 28);
  for (int i = 0; i < 4; ++i) tt.template add_body<T_RB>(conv(i == 0 ? ps.f[4] : ps.rb[i - 1], ps.rb[i], pw.rb_w[i], pw.rb_b[i]), Plan::RB0 + i, 6, 39);
  // conditioned blocks: two row-local chains each
  for (int blk = 0; blk < B_NBLOCKS; ++blk) {
    const WaveState::Scratch& sc = ws.scr[blk];  // one scratch set per block: all four blocks are in flight at once
    const int s0 = pl.blk(blk);
    const rc::BlockBArgs ba{sc.xa, ws.x[blk + 1], ww.q_w[blk], ww.q_b[blk], ww.o_w[blk], ww.o_b[blk], ws.d_kt[blk], ws.d_v[blk],
                            b->dev_view<int>(b->off.perm[blk]), b->dev_view<int>(b->off.tile_slot[blk]), nullptr};
    tt.template add_as<T_BLKB>(LaunchInfo{kBodies[T_BLKB].name, 2.0 * B * H * (256.0 * 256 * 2 + 256.0 * 384 * 2), 4.0 * (2.0 * 256 * 256 + 2.0 * 256 * 384 + B * H * 3.0 * 256)}, ba,
                               dim3(ws.n_tiles_max, 1), s0 + 1, tt.keep(5), 43.0);
    if (quads_on(b)) {  // rows without 15 neighbours on their K/V slot: one workgroup per quad (rebuild_tiles decides which rows)
      const rc::BlockBqArgs bq{sc.xa, ws.x[blk + 1], ww.q_w[blk], ww.q_b[blk], ww.o_w[blk], ww.o_b[blk], ws.d_ktp[blk], ws.d_vp[blk],
                               b->dev_view<int>(b->off.qperm[blk]), b->dev_view<int>(b->off.qslot[blk]), nullptr};
      // (a slot leaves at most 7 rows = 2 quads to this list: <= n_slots workgroups of two quads)
      tt.template add_as<T_BLKBQ>(LaunchInfo{kBodies[T_BLKBQ].name, 0.0, 0.0}, bq, dim3(std::min(2 * ws.n_tiles_max, ws.n_slots), 1), s0 + 1, tt.keep(5), 42.0);
    }
  }
  for (int blk = 0; blk < B_NBLOCKS; ++blk) {
    const rc::BlockAArgs aa{ws.x[blk], ws.scr[blk].xa, ww.c1_w[blk], ww.c1_b[blk], ww.c2_w[blk], ww.c2_b[blk], nullptr, B};
    switch (blk) {   // (the block's dilation is its type)
      case 0: tt.template add_body<T_BLKA1>(aa, pl.blk(blk), 5, 38); break;
      case 1: tt.template add_body<T_BLKA2>(aa, pl.blk(blk), 5, 38); break;
      case 2: tt.template add_body<T_BLKA4>(aa, pl.blk(blk), 5, 38); break;
      default: tt.template add_body<T_BLKA8>(aa, pl.blk(blk), 5, 38); break;
    }
  }
  gru_at(0);
  // (the k-NN lookup: one workgroup per stream walks the step's hops against the stream's codebook -- 35 us at four hops per step with
  //  64 speakers' codebooks in play.  At the end of the table, where round 2 had put it by its one-hop cost, it ENDED the launch: 256
  //  workgroups alone on the chip from 229 to 283 us of configs[3]'s tick, profiles/r06_notes.md section 3.  Present only while some stream has k > 0)
  { const VqArgs a{H, ps.raw, phone_vector_ring(ps), nullptr, ps.d_cbT, ps.d_cnorm, ps.d_vqk}; tt.template add_as<T_VQ>(LaunchInfo{kBodies[T_VQ].name, 0, 4.0 * B * H * 256}, a, dim3(B, 1), Plan::VQ, !ps.skip_vq, 9.0 * H); }
  {
    // the tail as three stages, several streams per workgroup (tail_stages.hip.h); same weights, same state block
    tst::StageArgs t1{}, t2{}, t3{};
    t1.in = ws.ya2; t1.out = ws.ya3; t2.in = ws.ya3; t2.out = ws.ya4; t3.in = ws.ya4;
    for (tst::StageArgs* t : {&t1, &t2, &t3}) { t->state = ws.tail.base; t->hop = nullptr; t->B = B; }
    t1.w[0] = ww.ra_w[1]; t1.b[0] = ww.ra_b[1]; t1.w[1] = ww.rb_w[1]; t1.b[1] = ww.rb_b[1]; t1.w[2] = ww.up_w[2]; t1.b[2] = ww.up_b[2];
    t2.w[0] = ww.ra_w[2]; t2.b[0] = ww.ra_b[2]; t2.w[1] = ww.rb_w[2]; t2.b[1] = ww.rb_b[2]; t2.w[2] = ww.up_w[3]; t2.b[2] = ww.up_b[3];
    t3.w[0] = ww.ra_w[3]; t3.b[0] = ww.ra_b[3]; t3.w[1] = ww.rb_w[3]; t3.b[1] = ww.rb_b[3];
    t3.fin_w = ww.fin_w; t3.fin_b = ww.fin_b; t3.d_out = ws.d_out; t3.io_stride = ws.io_stride;
    // (the sparse forms are never occupied while the sparse table is in use; kept so that the two tables hold the same stages)
    tt.template add_body<T_TAIL1>(t1, pl.tail(), 4, 28);
    tt.template add_body<T_TAIL2>(t2, pl.tail() + 1, 4, 11.5 * H);
    tt.template add_body<T_TAIL3>(t3, pl.tail() + 2, 4, 6.5 * H);
  }
  gru_at(1);
  // ---- everything else, longest workgroups first (they start when the heavy ones above leave their slots)
  // (the pitch head: few workgroups that walk a step's hops one after the other -- 10 us per workgroup at two hops per step, 21 at four;
  //  at the end of the table, where its instruction count would put it, it ENDED the launch: round 5's timelines, profiles/r05_notes.md)
  { PitchHeadArgs a = head_args(qw, qs); a.hop = nullptr; tt.template add_as<T_HEAD>(head_info(qs), a, dim3((B + 7) / 8, 1), Plan::HEAD, tt.keep(0), 7.5 * H); }
  tt.template add_body<T_F3>(conv(ps.f[1], ps.f[2], pw.f_w[1], pw.f_b[1]), Plan::F3, 6, 15);
  tt.template add_body<T_UP1>(conv(ws.x[4], ws.ya1, ww.up_w[0], ww.up_b[0]), pl.up1(), 7, 14);
  tt.template add_body<T_RES1B>(conv(ws.yb1, ws.yc1, ww.rb_w[0], ww.rb_b[0]), pl.up1() + 2, 7, 13);
  tt.template add_body<T_RES1A>(conv(ws.ya1, ws.yb1, ww.ra_w[0], ww.ra_b[0]), pl.up1() + 1, 7, 13);
  tt.template add_body<T_UP2>(conv(ws.yc1, ws.ya2, ww.up_w[1], ww.up_b[1]), pl.up1() + 3, 7, 13);
  tt.template add_body<T_F2>(conv(ps.f[0], ps.f[1], pw.f_w[0], pw.f_b[0]), Plan::F2, 6, 15);
  gru_at(2);
  tt.template add_body<T_POUT>(conv(qs.h, qs.logits, qw.out_w, qw.out_b), Plan::POUT, 2, 11);
  for (int i = 0; i < 2; ++i) tt.template add_body<T_P23>(conv(qs.p[i], qs.p[i + 1], qw.p_w[i + 1], qw.p_b[i + 1]), Plan::P2 + i, 2, 10);
  { const Ring phone_in{ws.d_phone, B_PHONE_CH, H, ws.front_slots}; ConvArgs a = conv(phone_in, ws.x[0], ww.inp_w, ww.inp_b); a.res = ws.e; tt.template add_body<T_INP>(a, Plan::INP, 3, 7.5); }
  gru_at(3);
  { FftArgs a = fft_args(qw, qs); a.hop = nullptr; tt.template add_as<T_FFT>(fft_info(qs), FftArgs2{a, B}, dim3((B + 1) / 2, H), Plan::FFT, tt.keep(0), 8.7); }
  tt.template add_body<T_OUT>(conv(ps.h, phone_out_ring(ps), pw.out_w, pw.out_b), Plan::OUT, 3, 4.5);
  { F1Args a = f1_args(pw, ps); a.hop = nullptr; a.hop_publish = nullptr; a.hop_publish_wave = nullptr; tt.template add_as<T_F1>(f1_info(ps), F1Args2{a, B}, dim3((B + 1) / 2, H), Plan::F1, tt.keep(0), 3.7); }
  { CondArgs a = cond_args(ww, ws); a.hop = nullptr; a.hop_next_out = nullptr; tt.template add_as<T_COND>(cond_info(ws), a, dim3((B * H + 1) / 2, 1), Plan::COND, tt.keep(0), 1.5); }
  if (!tb->ok) return false;
  // (XCD-aware placement -- bodies with many weights pinned to one XCD, or to the XCDs of equal index modulo 2 / 4, so that their weights
  //  stay in fewer L2s -- was measured in rounds 2 and 4: memory-side traffic / 4, the launch 4-8 % slower; the switch went with the
  //  span lookup in round 5.  Its successor is fuse::two_halves (tick_order_plan.h): the same idea at the granularity that costs nothing;
  //  which bodies it pins -- the ones with the weights, each on one half of the chip -- is tick::kBodies' placement column)
  // Dispatch order by workgroup (fuse::WgDesc, one descriptor per workgroup read by a scalar load): the bodies in the order added above,
  // every body a contiguous run.  (Round 5 also measured the short workgroups dealt AMONG the long MFMA-dense ones: 7.7 % slower,
  // profiles/r05_notes.md section 4; round 6 the short ones as a KERNEL OF THEIR OWN at twice the occupancy, beside or behind the dense
  // one: 8-12 % slower, profiles/r06_notes.md section 1, tools/experiments/r06_two_kernel_tick.patch.)
  static const int halves_mode = bhip::meas_env("BEATRICE_HIP_TICK_HALVES") ? std::atoi(bhip::meas_env("BEATRICE_HIP_TICK_HALVES")) : 2;   // 0: every body on all XCDs; 2 (default): halves; 4: quarters
  {
    const fuse::SpanRow* rows = tb->rows;
    const int n_rows = tb->t.n_spans;
    const std::vector<fuse::WgDesc> plain = fuse::in_span_order(rows, n_rows);
    // (the sparse table only ever runs partly filled ticks)
    const std::vector<fuse::WgDesc> desc = halves_mode != 0 && !sparse ? fuse::two_halves(rows, n_rows, halves_mode == 4 ? 4 : 2) : plain;
    auto upload = [&](const std::vector<fuse::WgDesc>& v, DevBuf<fuse::WgDesc>& d_desc) {
      if (v.size() > d_desc.size() && !d_desc.alloc(v.size(), "tick dispatch order", false)) return false;
      if (!v.empty()) BHIP_TRY(hipMemcpy(d_desc, v.data(), sizeof(fuse::WgDesc) * v.size(), hipMemcpyHostToDevice));
      return true;
    };
    if (!sparse) {   // (the order of partly filled ticks: tick_launch)
      if (!upload(plain, k.d_desc_plain)) return false;
      k.table_total_plain = (int)plain.size();
      // the fill / drain shapes without the empty stages' workgroups (tick::State::d_desc_ranges)
      static const int range_halves_from = bhip::meas_env("BEATRICE_HIP_TICK_RANGE_HALVES") ? std::atoi(bhip::meas_env("BEATRICE_HIP_TICK_RANGE_HALVES")) : kRangeHalvesFrom;
      const fuse::RangeLists r = fuse::range_lists(rows, n_rows, plain, pl.count(), halves_mode, range_halves_from);
      k.range = r.at;
      if (!r.all.empty() && !upload(r.all, k.d_desc_ranges)) return false;
    }
    tb->t.total = (int)desc.size();   // (two_halves may add filler indices)
    if (!upload(desc, sparse ? k.d_desc_sparse : k.d_desc)) return false;
  }
  if (bhip::meas_env("BEATRICE_HIP_TICK_TRACE")) {
    if (!k.d_trace.alloc((size_t)3 * tb->t.total, "tick trace", false)) return false;
    tb->t.trace = k.d_trace;
  }
  if (sparse) {
    tb->t.trace = nullptr;
    BHIP_TRY(hipMemcpy(k.d_table_sparse, &tb->t, sizeof(Tab), hipMemcpyHostToDevice));
    k.table_sparse_total = tb->t.total;
    return true;
  }
  BHIP_TRY(hipMemcpy(k.d_table, &tb->t, sizeof(Tab), hipMemcpyHostToDevice));
  k.table_total = tb->t.total;
  k.table_flops = tb->flops;
  k.table_bytes = tb->bytes;
  // who reads which part of the settings block, and where its private copy lives
  k.consumers.clear();
  unsigned char* d = b->settings.d;
  k.consumers.push_back(Consumer{Plan::VQ, b->off.cbT, b->off.min_q - b->off.cbT, d + b->off.cbT, -1});
  k.consumers.push_back(Consumer{Plan::HEAD, b->off.min_q, b->off.add_idx - b->off.min_q, d + b->off.min_q, -1});
  k.consumers.push_back(Consumer{Plan::COND, b->off.add_idx, b->off.front_bytes - b->off.add_idx, d + b->off.add_idx, -1});
  for (int blk = 0; blk < B_NBLOCKS; ++blk) {
    const size_t lo = b->off.perm[blk], hi = blk + 1 < B_NBLOCKS ? b->off.perm[blk + 1] : b->off.front_bytes + b->off.wave_bytes;
    k.consumers.push_back(Consumer{pl.blk(blk) + 1, lo, hi - lo, d + lo, -1});
  }
  k.table_dirty = false;
  return true;
}
bool tick_build_table(BeatriceBatch* b, const bool sparse = false) {
  switch (b->H) {
    case 1: return tick_build_table_h<1>(b, sparse);
    case 2: return tick_build_table_h<2>(b, sparse);
    case 4: return tick_build_table_h<4>(b, sparse);
    default: return false;
  }
}
// the launch of one tick: the table kernel of the batch's hops per step
static void tick_launch(BeatriceBatch* b, const bool sparse, const bool full, hipStream_t st, const fuse::StepPairs& pairs) {
  tick::State& k = b->tk;
  const void* t = sparse ? k.d_table_sparse.get() : k.d_table.get();
  // full = every stage has a step: the order that confines the bodies with the weights to halves of the chip; a partly filled tick
  // (fill, drain) runs the same table in plain span order -- without the workgroups of its empty stages where the occupied stages
  // are 0 .. k or k .. last (tick::State::d_desc_ranges)
  const fuse::WgDesc* desc = sparse ? k.d_desc_sparse.get() : (full ? k.d_desc.get() : k.d_desc_plain.get());
  int total = sparse ? k.table_sparse_total : (full ? k.table_total : k.table_total_plain);
  static const bool no_ranges = bhip::meas_env("BEATRICE_HIP_TICK_NO_RANGES") != nullptr;   // A/B switch for measurements
  if (!sparse && !full && !no_ranges && k.d_desc_ranges.get() != nullptr) {
    const fuse::RangePick pick = fuse::pick_range(pairs.hop, k.plan.count(), k.range);
    if (pick.shape >= 0) { desc = k.d_desc_ranges + k.range.off[pick.shape][pick.at]; total = k.range.n[pick.shape][pick.at]; }
  }
  if (total <= 0) return;
  // (k.ragged: the second instance of the launch, once a stream has sat a step out -- at several hops per step a stream sits a WHOLE step out)
  if (b->H == 1) fuse::launch_table_w<4>(static_cast<const tick::Ops<1>::Tab*>(t), desc, total, st, pairs, k.ragged);
  else if (b->H == 2) fuse::launch_table_w<4>(static_cast<const tick::Ops<2>::Tab*>(t), desc, total, st, pairs, k.ragged);
  else fuse::launch_table_w<4>(static_cast<const tick::Ops<4>::Tab*>(t), desc, total, st, pairs, k.ragged);
}

// One tick: every stage advances by one step; `feeding` = a new step enters at stage 0.
// BEATRICE_HIP_TICK_HOSTPROF=1: host time of tick_run by section, printed when the process ends (measurement aid)
struct HostProf {
  static constexpr int N = 5;
  static bool on() { static const bool v = bhip::meas_env("BEATRICE_HIP_TICK_HOSTPROF") != nullptr; return v; }
  struct Totals { double us[N] = {}; long long calls = 0; ~Totals() { if (calls) std::fprintf(stderr, "tick_run host us per call: settings/kv %.1f, table %.1f, snapshot upload %.1f, copies %.1f, launch %.1f (%lld calls)\n", us[0] / calls, us[1] / calls, us[2] / calls, us[3] / calls, us[4] / calls, calls); } };
  static Totals& totals() { static Totals t; return t; }
  std::chrono::steady_clock::time_point t0;
  HostProf() { if (on()) { t0 = std::chrono::steady_clock::now(); totals().calls += 1; } }
  void lap(int i) {
    if (!on()) return;
    const auto t1 = std::chrono::steady_clock::now();
    totals().us[i] += std::chrono::duration<double, std::micro>(t1 - t0).count();
    t0 = t1;
  }
};
// ---- a stream starts over inside the pipeline (BeatriceBatch_ResetStreamInFlight; the device side and the reasoning: tick_reset.hip.h)
// The table of what a reset that applies to step k clears, and when: "before stage s" = in front of the launch of tick k + s, `spare`
// = but for the slot step k itself has written (the ring's producer ran one tick earlier).  Every ring of the three arenas is accounted
// for here (the count is checked against the arenas):
//   phone   audio                      before F1 (0), whole          -- written and read, with history, by F1 alone
//           f[0] .. f[4]               before F2 .. F5, RB0, spare   -- producer at the stage before, one reader with history
//           rb[0] .. rb[2]             before RB1 .. RB3, spare      -- (a residual block takes its residual from the same ring, same stage)
//           rb[3], raw                 nothing                       -- read at the step's own frames only (GRU input; k-NN input)
//           h                          NO WINDOW: cell run again after tick k + PGRU (phone.out reads step k - 1's last frame in the
//                                      launch in which the cell of step k reads it as its previous state)
//   pitch   audio                      before FFT (3), whole
//           spec, p[0], p[1]           before P1, P2, P3, spare
//           p[2], logits               nothing
//           h                          NO WINDOW: cell run again after tick k + QGRU (pitch.out, and the head one tick later, read
//                                      step k - 1's frame: it is put back after the restart)
//           d_prev_q (no ring)         before HEAD, whole
//   wave    e                          nothing                       -- (conditioning of the step's own frames)
//           x[0] .. x[3]               before block i's first half, spare -- written by wave.inp / the block before's second half, read
//                                                                      with history by the dilated convolution only (the residual is the
//                                                                      same body); the spare slots of boundary_slots are history nobody reads
//           x[4]                       before up1, spare
//           scratch h1, xa, q, sc, o   nothing                       -- xa: the second half reads the step's own frames, the others are unused here
//           ya1, yb1, yc1              before res1a, res1b, up2, spare
//           ya2                        before the tail's first stage, spare
//           tail                       its three parts (YB2 YC2 | YA3 YB3 YC3 | YA4 YB4 YC4) before the tail stage that owns them, whole;
//                                      the sub-steps' carried frames live in LDS
//           ya3, ya4                   nothing                       -- their two-frame histories are TS_YA3 / TS_YA4 of the tail block
//   wrapper (mode F) Wrap48State   hist_in before the WRAPPER launch of tick k (its input half reads step k), whole; ztail and fpend
//                                      before the wrapper launch that runs step k's output half -- the one in front of tick k + stages, or
//                                      the flush launch of a drain -- whole.  Every form of wrap48_tick_kernel reads a stream's state
//                                      once when a launch starts and writes it once when it ends, so a clear between two launches is exact
constexpr int kResetWrapIn = -2, kResetWrapOut = -3;   // (in the place of a stage in State::reset_stage)
static bool tick_reset_prepare(BeatriceBatch* b) {
  using namespace tick;
  State& k = b->tk;
  if ((int)k.reset_pending.size() != b->B) { k.reset_pending.assign(b->B, 0); k.any_reset_pending = false; }
  if (k.d_reset_rings) return true;
  const Plan pl = k.plan;
  const PhoneState& ps = b->phone;
  const PitchState& qs = b->pitch;
  const WaveState& ws = b->wave;
  std::vector<ResetRing> rings;
  std::vector<int> stage;
  std::vector<unsigned char> spare;
  size_t accounted = 0;
  auto clear = [&](const Ring& r, int before_stage, bool sp) {
    rings.push_back(ResetRing{r.base, (unsigned)ring_stream_floats(r), (unsigned)(r.n * r.C), r.m});
    stage.push_back(before_stage); spare.push_back(sp ? 1 : 0); ++accounted;
  };
  auto nothing = [&](const Ring& r) { if (r.base) ++accounted; };
  clear(ps.audio, Plan::F1, false);
  clear(ps.f[0], Plan::F2, true); clear(ps.f[1], Plan::F3, true); clear(ps.f[2], Plan::F4, true); clear(ps.f[3], Plan::F5, true); clear(ps.f[4], Plan::RB0, true);
  for (int i = 0; i < 3; ++i) clear(ps.rb[i], Plan::RB0 + i + 1, true);
  nothing(ps.rb[3]); nothing(ps.raw); nothing(ps.h);   // (h: the restarted cell)
  clear(qs.audio, Plan::FFT, false);
  clear(qs.spec, Plan::P1, true); clear(qs.p[0], Plan::P2, true); clear(qs.p[1], Plan::P2 + 1, true);
  nothing(qs.p[2]); nothing(qs.logits); nothing(qs.h);
  nothing(ws.e);
  for (int blk = 0; blk < B_NBLOCKS; ++blk) clear(ws.x[blk], pl.blk(blk), true);
  clear(ws.x[B_NBLOCKS], pl.up1(), true);
  for (const WaveState::Scratch& sc : ws.scr) { nothing(sc.h1); nothing(sc.xa); nothing(sc.q); nothing(sc.sc); nothing(sc.o); }
  clear(ws.ya1, pl.up1() + 1, true); clear(ws.yb1, pl.up1() + 2, true); clear(ws.yc1, pl.up1() + 3, true);
  clear(ws.ya2, pl.tail(), true);
  {
    const int part[4] = {TS_YB2, TS_YA3, TS_YA4, TAIL_STATE_FLOATS};
    for (int i = 0; i < 3; ++i) {
      rings.push_back(ResetRing{ws.tail.base + part[i], (unsigned)TAIL_STATE_FLOATS, (unsigned)(part[i + 1] - part[i]), 1});
      stage.push_back(pl.tail() + i); spare.push_back(0);
    }
    ++accounted;
  }
  nothing(ws.ya3); nothing(ws.ya4);
  rings.push_back(ResetRing{reinterpret_cast<float*>(qs.d_prev_q), 1u, 1u, 1});   // (an int; zero is zero)
  stage.push_back(Plan::HEAD); spare.push_back(0);
  if (accounted != ps.arena.rings.size() + qs.arena.rings.size() + ws.arena.rings.size() || ws.tail.C != TAIL_STATE_FLOATS || ws.tail.n * ws.tail.m != 1) {
    std::fprintf(stderr, "beatrice_hip: the in-flight reset table does not cover the batch's rings\n");
    return false;
  }
  // The 48 kHz wrapper around the ticks (mode F): the three parts of Wrap48State, each whole.  They belong to no stage of the tick: the
  // input half's history is cleared in front of the wrapper launch of the step's own tick, the output half's two parts in front of the
  // wrapper launch ONE LAUNCH BEHIND the step's last stage (tick_reset_wrap48 below; neither sentinel is a stage tick_reset_launch meets)
  const int wrap_first = (int)rings.size();
  {
    float* w = reinterpret_cast<float*>(b->d_w48.get());
    const unsigned stride = (unsigned)(sizeof(Wrap48State) / sizeof(float));
    const size_t part[3] = {offsetof(Wrap48State, hist_in), offsetof(Wrap48State, ztail), offsetof(Wrap48State, fpend)};
    const unsigned len[3] = {30u, 16u, 240u};
    static_assert(sizeof(Wrap48State) == sizeof(float) * (30 + 16 + 240), "the in-flight reset clears every part of Wrap48State");
    for (int i = 0; i < 3; ++i) {
      rings.push_back(ResetRing{w + part[i] / sizeof(float), stride, len[i], 1});
      stage.push_back(i == 0 ? kResetWrapIn : kResetWrapOut); spare.push_back(0);
    }
  }
  DevBuf<ResetRing> d_rings;
  DevBuf<float> keep;
  StagedRing<int> list;
  // (a tick's list: at most one item per ring and stream -- the resets at one depth of the pipeline are of different streams -- and the
  //  two cells' {stream, counter} pairs behind them)
  const size_t list_ints = 4 * rings.size() * (size_t)b->B + 2 * 2 * (size_t)b->B;
  if (!d_rings.alloc(rings.size(), "reset ring table", false) ||
      !hip_ok(hipMemcpy(d_rings, rings.data(), sizeof(ResetRing) * rings.size(), hipMemcpyHostToDevice), "reset ring table up") ||
      !keep.alloc((size_t)b->B * (256 + 128), "reset gru keep", false) || !list.alloc(State::kResetStaging, list_ints, "reset work list"))
    return false;
  k.n_reset_rings = (int)rings.size(); k.d_reset_rings = std::move(d_rings); k.reset_stage = std::move(stage); k.reset_spare = std::move(spare);
  k.reset_wrap_first = wrap_first;
  k.reset_m.clear();
  for (const ResetRing& r : rings) k.reset_m.push_back(r.m);
  k.d_gru_keep = std::move(keep); k.reset_list = std::move(list); k.reset_list_ints = list_ints;
  return true;
}
// In front of the launch of tick k.tick: what the resets that are travelling need cleared before it, and the cells to run again behind
// the tick before.  Nothing is launched on a tick that has no such work.
static bool tick_reset_launch(BeatriceBatch* b, hipStream_t st) {
  using namespace tick;
  State& k = b->tk;
  const int n_stages = k.plan.count(), B = b->B;
  int n_items = 0, n_p = 0, n_q = 0;
  int* list = nullptr;
  auto claim = [&]() {
    if (!list) list = k.reset_list.claim((int)(k.reset_serial % State::kResetStaging));
    return list != nullptr;
  };
  const size_t off_p = 4 * (size_t)k.n_reset_rings * B, off_q = off_p + 2 * (size_t)B;
  size_t keep_n = 0;
  for (const State::Travelling& r : k.resets) {
    const int d = (int)(k.tick - r.tick);   // the stage the reset's step reaches in this tick
    if (d < n_stages) k.resets[keep_n++] = r;
    if (d >= n_stages) continue;   // (mode F: its last clear went in front of this tick's wrapper launch, tick_reset_wrap48)
    for (int i = 0; i < k.n_reset_rings; ++i) {
      if (k.reset_stage[i] != d) continue;
      if (!claim()) return false;
      const ResetItem it{i, r.stream, k.reset_spare[i] ? r.counter % k.reset_m[i] : -1, 0};   // (ring_pos: the slot of the stream's counter)
      std::memcpy(list + 4 * (size_t)n_items++, &it, sizeof(it));
    }
    if (d == Plan::PGRU + 1 || d == Plan::QGRU + 1) {
      if (!claim()) return false;
      int* g = d == Plan::PGRU + 1 ? list + off_p + 2 * (size_t)n_p++ : list + off_q + 2 * (size_t)n_q++;
      g[0] = r.stream; g[1] = r.counter;
    }
  }
  k.resets.resize(keep_n);
  if (!list) return true;
  if (n_items > 0)
    hipLaunchKernelGGL(ring_reset_kernel, dim3(n_items), dim3(256), 0, st, k.d_reset_rings.get(), k.n_reset_rings, reinterpret_cast<const ResetItem*>(list), B);
  const int H = b->H;
  if (n_p > 0) {
    const PhoneWeights& pw = b->phone_m->w;
    const GruArgs g{b->phone.rb[3], b->phone.h, pw.gru_wih, pw.gru_whh, pw.gru_bih, pw.gru_bhh, nullptr, B, 0, nullptr, nullptr, nullptr, 1};
    const int2* items = reinterpret_cast<const int2*>(list + off_p);
    for (int ph = -1; ph <= H; ++ph)
      hipLaunchKernelGGL((gru_restart_kernel<256, 256>), dim3(n_p, 256 / 16), dim3(384), 0, st, g, items, k.d_gru_keep.get(), ph < 0 ? kGruSave : (ph == H ? kGruRestore : ph));
  }
  if (n_q > 0) {
    const PitchWeights& qw = b->pitch_m->w;
    const GruArgs g{b->pitch.p[2], b->pitch.h, qw.gru_wih, qw.gru_whh, qw.gru_bih, qw.gru_bhh, nullptr, B, 0, nullptr, nullptr, nullptr, 1};
    const int2* items = reinterpret_cast<const int2*>(list + off_q);
    for (int ph = -1; ph <= H; ++ph)
      hipLaunchKernelGGL((gru_restart_kernel<128, 128>), dim3(n_q, 128 / 16), dim3(384), 0, st, g, items, k.d_gru_keep + (size_t)B * 256, ph < 0 ? kGruSave : (ph == H ? kGruRestore : ph));
  }
  if (!k.reset_list.mark((int)(k.reset_serial % State::kResetStaging), st)) return false;
  k.reset_serial += 1;
  k.reset_launches += 1;
  return hip_ok(hipGetLastError(), "in-flight reset");
}
// Mode F, in front of a launch of the 48 kHz wrapper (the one of tick k.tick, or -- `flush` -- the one a drain sends behind the last
// tick): the parts of Wrap48State the travelling resets need cleared before it.  A reset whose step was fed by tick r.tick clears the
// input half's history before the wrapper launch of that very tick, and the output half's tail and FIFO before the wrapper launch that
// follows tick r.tick + stages - 1, the one that emits the step's block.  That is one launch behind the step's last stage: a reset stays
// in the list until tick_reset_launch of tick r.tick + stages drops it, or the flush does.  Nothing is launched where no reset is due.
static bool tick_reset_wrap48(BeatriceBatch* b, hipStream_t st, const bool flush) {
  using namespace tick;
  State& k = b->tk;
  if (k.resets.empty() || k.reset_wrap_first < 0) return true;
  const int n_stages = k.plan.count();
  int n_items = 0;
  int* list = nullptr;
  size_t keep_n = 0;
  for (const State::Travelling& r : k.resets) {
    const long long d = k.tick - r.tick;
    const bool in_half = !flush && d == 0, out_half = d == n_stages;
    if (!flush || d < n_stages) k.resets[keep_n++] = r;   // (behind the flush no tick follows that would drop it, and the next tick has the same number)
    if (!in_half && !out_half) continue;
    if (!list && !(list = k.reset_list.claim((int)(k.reset_serial % State::kResetStaging)))) return false;
    for (int i = k.reset_wrap_first; i < k.n_reset_rings; ++i) {
      if (k.reset_stage[i] != (in_half ? kResetWrapIn : kResetWrapOut)) continue;
      const ResetItem it{i, r.stream, -1, 0};
      std::memcpy(list + 4 * (size_t)n_items++, &it, sizeof(it));
    }
  }
  k.resets.resize(keep_n);
  if (!list) return true;
  hipLaunchKernelGGL(ring_reset_kernel, dim3(n_items), dim3(256), 0, st, k.d_reset_rings.get(), k.n_reset_rings, reinterpret_cast<const ResetItem*>(list), b->B);
  if (!k.reset_list.mark((int)(k.reset_serial % State::kResetStaging), st)) return false;
  k.reset_serial += 1;
  return hip_ok(hipGetLastError(), "in-flight reset of the 48 kHz wrapper");
}
// The drained form of a reset for the streams still waiting for their step (leaving tick mode: the in-order chain takes the batch over;
// out of mode F the stream's wrapper state with the rest, as BeatriceBatch_ResetStream clears it)
static bool tick_reset_settle(BeatriceBatch* b) {
  tick::State& k = b->tk;
  bool ok = true;
  for (int s = 0; s < (int)k.reset_pending.size() && ok && k.any_reset_pending; ++s) {
    if (!k.reset_pending[s]) continue;
    ok = b->phone.arena.zero_stream(s, b->stream) && b->pitch.arena.zero_stream(s, b->stream) && b->wave.arena.zero_stream(s, b->stream) &&
         hip_ok(hipMemsetAsync(b->pitch.d_prev_q + s, 0, sizeof(int), b->stream), "prev_q") &&
         (!b->r48.on || hip_ok(hipMemsetAsync(b->d_w48 + s, 0, sizeof(Wrap48State), b->stream), "w48 reset"));
    // (a switch made since the call: the new stream starts on all four blocks of the target it has now, as in advance_kv)
    if (ok && b->cfg[s].kv_set_count < B_NBLOCKS) ok = BeatriceBatch_FlushSpeaker(b, s) == 0;
  }
  std::fill(k.reset_pending.begin(), k.reset_pending.end(), 0);
  k.any_reset_pending = false;
  return ok && hip_ok(hipStreamSynchronize(b->stream), "reset settle");
}
bool tick_run(BeatriceBatch* b, bool feeding) {
  using namespace tick;
  State& k = b->tk;
  HostProf prof;
  if (feeding) {
    advance_kv(b);
    draw_codebooks(b);
    if (b->vq_dirty) { update_vq_mode(b); b->vq_dirty = false; }   // (drains the pipeline if the k-NN stage comes or goes)
  }
  prof.lap(0);
  if (k.table_dirty && !(tick_build_table(b, true) && tick_build_table(b, false))) return false;   // (the full table last: it clears table_dirty)
  prof.lap(1);
  hipStream_t st = b->stream;
  Copy upload{nullptr, nullptr, 0};
  int upload_stage = -1;
  if (feeding) {
    bool dirty = b->front_dirty || k.snap_cur < 0;
    for (bool w : b->wave_dirty) dirty = dirty || w;
    if (dirty) {  // a new version of the settings: one upload into the next slot of the snapshot ring
      const int serial = k.snap_next++;
      const size_t off = 0, len = k.snap_bytes;
      unsigned char* dst = k.d_snap + (size_t)(serial % kRing) * k.snap_bytes;
      // through a ring of pinned staging copies, so that the host may run several settings changes ahead of the device
      // (the batch's two-deep mirror would make every second change wait for the copy of the change before it); the
      // tick's prologue kernel reads the staging copy straight from host memory (tick.hip.h)
      const int si = serial % State::kStaging;
      unsigned char* src = k.stage.claim(si);
      if (!src) return false;
      std::memcpy(src, b->settings.h + off, len);
      upload = Copy{dst, src, (int)len};
      upload_stage = si;
      k.snap_cur = serial;
      b->front_dirty = false;
      for (bool& w : b->wave_dirty) w = false;
    }
    const long long u = k.n_fed;
    k.fed_step[k.tick % kRing] = u;
    k.snap_of_step[u % kRing] = k.snap_cur;
    k.hop_of_step[u % kRing] = b->hop_host;
    k.io_of_step[u % kRing] = b->io_host;
  } else {
    k.fed_step[k.tick % kRing] = -1;
  }
  // ragged steps: the flags of BeatriceBatch_SetSilentStreams name the streams that sit THIS step out
  Copy hv_upload{nullptr, nullptr, 0};
  int hv_stage = -1;
  if (feeding) {
    BeatriceBatch::SilentRule& sr = b->silent;
    if (!k.ragged && sr.on && sr.any_next) {   // the first stream to stand still: from here on every stream has its own counter
      if (!k.d_hopv) {
        const int row = (b->B + 3) & ~3;
        DevBuf<int> d_hopv;
        StagedRing<int> hopv;
        if (!d_hopv.alloc((size_t)kRing * row, "tick hopv", false) || !hopv.alloc(State::kStaging, row, "tick hopv staging")) return false;
        k.row = row; k.d_hopv = std::move(d_hopv); k.hopv = std::move(hopv);
      }
      k.hop_s.assign(b->B, b->hop_host);
      k.ragged = true;
    }
    const long long u = k.n_fed;
    k.step_ragged[u % kRing] = k.ragged;
    if (k.ragged) {
      const int si = (int)(u % State::kStaging);
      int* h = k.hopv.claim(si);
      if (!h) return false;
      for (int s = 0; s < b->B; ++s) {
        const bool out = sr.any_next && sr.next[s];
        h[s] = out ? -1 : k.hop_s[s];
        if (!out) { k.hop_s[s] = hop_next(k.hop_s[s]); b->mv.seen.fed(s, k.tick); }   // (stream_move_plan.h: the stream has a step inside from this tick on)
      }
      for (int s = b->B; s < k.row; ++s) h[s] = -1;
      hv_upload = Copy{reinterpret_cast<unsigned char*>(k.d_hopv + (size_t)(u % kRing) * k.row), reinterpret_cast<const unsigned char*>(h), (int)(sizeof(int) * k.row)};
      hv_stage = si;
      if (k.any_reset_pending) {   // a stream starts over at this step (BeatriceBatch_ResetStreamInFlight) -- one that sits it out, at its next present step
        bool left = false;
        for (int s = 0; s < b->B; ++s) {
          if (!k.reset_pending[s]) continue;
          if (h[s] < 0) { left = true; continue; }
          k.resets.push_back(State::Travelling{s, h[s], k.tick});
          k.reset_pending[s] = 0;
        }
        k.any_reset_pending = left;
      }
    }
    if (!k.ragged) b->mv.seen.fed_all(k.tick);   // (the common counter: every stream takes part)
    if (!k.ragged && k.any_reset_pending) {
      for (int s = 0; s < b->B; ++s)
        if (k.reset_pending[s]) { k.resets.push_back(State::Travelling{s, b->hop_host, k.tick}); k.reset_pending[s] = 0; }
      k.any_reset_pending = false;
    }
    if (sr.any_next) { std::fill(sr.next.begin(), sr.next.end(), 0); sr.any_next = false; }
  }
  prof.lap(2);
  Prolog p{};
  p.n_stages = k.plan.count();
  auto step_at = [&k](int stage) -> long long {
    const long long t2 = k.tick - stage;
    return t2 >= 0 ? k.fed_step[t2 % kRing] : -1;
  };
  for (int s = 0; s < p.n_stages; ++s) {
    const long long u = step_at(s);
    p.hop[s] = u < 0 ? -1 : k.hop_of_step[u % kRing];
    p.io[s] = u < 0 ? 0 : k.io_of_step[u % kRing];
  }
  for (Consumer& c : k.consumers) {
    const long long u = step_at(c.stage);
    if (u < 0) continue;
    const int want = k.snap_of_step[u % kRing];
    if (want == c.held) continue;
    p.copy[p.n_copies++] = Copy{c.dst, k.d_snap + (size_t)(want % kRing) * k.snap_bytes + c.off, (int)c.bytes};
    c.held = want;
  }
  if (upload.bytes > 0) {  // first, so that entry order = age; (a consumer never needs the snapshot uploaded in its own tick: none sits at stage 0)
    for (int i = p.n_copies; i > 0; --i) p.copy[i] = p.copy[i - 1];
    p.copy[0] = upload;
    p.n_copies += 1;
  }
  if (hv_upload.bytes > 0) p.copy[p.n_copies++] = hv_upload;   // (read by stage 0 of the launch that follows: the prologue runs before it)
  if (p.n_copies > 0) {  // (only on ticks where the settings changed or a change arrives at a consumer)
    int chunks = 0;
    for (int i = 0; i < p.n_copies; ++i) { p.first_chunk[i] = chunks; chunks += (p.copy[i].bytes + kCopyChunk - 1) / kCopyChunk; }
    p.first_chunk[p.n_copies] = chunks;
    hipLaunchKernelGGL(prologue_kernel, dim3(chunks), dim3(256), 0, st, p);
    if (upload_stage >= 0 && !k.stage.mark(upload_stage, st)) return false;
    if (hv_stage >= 0 && !k.hopv.mark(hv_stage, st)) return false;
  }
  if (b->r48.on && (feeding || b->r48.deferred_slot >= 0)) {
    // one launch for both ends of the 48 kHz wrapper: the block entering the pipeline -> its 16 kHz hop, straight into the
    // resident slot; and the step the PREVIOUS tick completed leaves through the up-sampler and the 480-sample FIFO
    // (resample.h:346-361: the block emitted for step j carries the model output of step j - 1) into the 48 kHz slot of step j
    BeatriceBatch::Resident48& r = b->r48;
    Wrap48TickArgs wa{};
    wa.channels = r.channels; wa.st = b->d_w48; wa.coef_down = b->d_coef_down; wa.coef_up = b->d_coef_up; wa.H = b->H;
    auto counters_of = [&k](long long u) -> const int* { return u >= 0 && k.step_ragged[u % kRing] ? k.d_hopv + (size_t)(u % kRing) * k.row : nullptr; };
    if (feeding) {
      wa.n_pre = b->B;
      wa.in48 = r.d_in48 + (size_t)b->io_host * b->B * b->H * r.channels * 480;
      wa.in16 = r.d_in16 + (size_t)b->io_host * b->B * b->H * B_IN_HOP;
      wa.hv_pre = counters_of(k.n_fed);   // (the step being fed; its row was written by the prologue launch above)
    }
    if (r.deferred_slot >= 0) {
      wa.n_post = b->B;
      wa.out48 = r.d_out48 + (size_t)r.deferred_slot * b->B * b->H * r.channels * 480;
      wa.model_out = r.d_out24 + (size_t)r.deferred_slot * b->B * b->H * B_OUT_HOP;
      wa.hv_post = counters_of(r.deferred_step);
      wa.in48_post = r.d_in48 + (size_t)r.deferred_slot * b->B * b->H * r.channels * 480;
      r.deferred_slot = -1;
    }
    if (!k.resets.empty() && !tick_reset_wrap48(b, st, false)) return false;   // (behind the wrapper launch before, in front of this one)
    hipLaunchKernelGGL(wrap48_tick_kernel, dim3(wrap48_tick_grid(wa)), dim3(256), 0, st, wa);
  }
  prof.lap(3);
  fuse::StepPairs pairs;
  pairs.hopv = k.ragged ? k.d_hopv.get() : nullptr;
  pairs.n_streams = k.row;
  for (int s = 0; s < fuse::kMaxStepPairs; ++s) {
    pairs.hop[s] = s < p.n_stages ? p.hop[s] : -1; pairs.io[s] = s < p.n_stages ? p.io[s] : 0;
    const long long u = s < p.n_stages ? step_at(s) : -1;
    pairs.hv[s] = u >= 0 && k.step_ragged[u % kRing] ? (int)(u % kRing) : -1;
  }
  // The sparse table (tick.hip.h) while only front-end stages have a step -- the first ticks of a fill: measured per tick on a
  // 20-step run (tools/debug/fill_drain.sh) 31 us against 42-45; from the first conditioned block on, and in the drain, the
  // half-size bodies LOSE (51-54 us against 45-48; two streams per tail workgroup 39 against 37), so there the full table runs
  int highest = -1;
  for (int s = 0; s < p.n_stages; ++s) if (p.hop[s] >= 0) highest = s;
  static const bool no_sparse = bhip::meas_env("BEATRICE_HIP_TICK_NO_SPARSE") != nullptr;   // A/B switch for measurements
  // (one hop per step only: at two hops per step it measured no difference, at four the half-size bodies cost 1 % of a 20-step run --
  //  5 196 against 5 138 us of launches, profiles/r05_notes.md)
  const bool sparse = highest >= 0 && highest < Plan::BLK0 && !no_sparse && sparse_table_at(b->H);
  int occupied = 0;
  for (int s = 0; s < p.n_stages; ++s) occupied += p.hop[s] >= 0 ? 1 : 0;
  if (!k.resets.empty() && !tick_reset_launch(b, st)) return false;   // (behind the prologue and the tick before, in front of this tick's launch)
  tick_launch(b, sparse, occupied == p.n_stages, st, pairs);
  if (b->r48.on) {  // the step this tick completed: its 48 kHz block is produced by the wrapper launch of the next tick (or of the drain)
    const long long u = step_at(k.plan.count() - 1);
    if (u >= 0) { b->r48.deferred_slot = k.io_of_step[u % kRing]; b->r48.deferred_step = u; }
  }
  if (feeding) {
    b->last_parity = b->hop_host % 3;
    b->last_hop = b->hop_host;
    b->hop_host = hop_next(b->hop_host);
    b->io_host = (b->io_host + 1) % b->io_slots;
    b->steps_enqueued += 1;
    k.n_fed += 1;
    k.last_feed_tick = k.tick;
    b->entries.fed(k.tick, k.plan.count());   // (speaker_entry_plan.h: entries that waited for a filling step get their stamp)
  }
  prof.lap(4);
  k.tick += 1;
  b->inflight = true;
  return hip_ok(hipGetLastError(), "tick launch");
}
// Ragged steps leave every stream at a step counter of its own; at a DRAINED point (no step inside the pipeline) the batch is brought
// back to one counter: the rings of every stream that lags are rotated forward by its deficit (ring_rotate_kernel), after which all
// streams stand at the batch's counter -- the common launch runs again (the ragged instance costs +16 %), and the in-order chain,
// which has one counter for all streams, can take the batch over (leaving tick mode used to be refused for good).
static bool tick_relevel(BeatriceBatch* b) {
  using namespace tick;
  State& k = b->tk;
  if (!k.ragged) return true;
  std::vector<int> shift(b->B, 0);
  bool any = false;
  for (int s = 0; s < b->B; ++s) {
    int d = b->hop_host - k.hop_s[s];
    if (d < 0) d += B_HOP_WRAP;
    shift[s] = d;
    any = any || d != 0;
  }
  if (any) {
    if (!k.d_ring_table) {
      std::vector<FreezeRing> rings;
      for (const RingArena* a : {&b->phone.arena, &b->pitch.arena, &b->wave.arena})
        for (const Ring* r : a->rings) {
          if (r->m > kMaxRotateSlots) return false;
          rings.push_back(FreezeRing{r->base, r->n * r->C, r->m, 0});
        }
      DevBuf<FreezeRing> d_rings;
      DevBuf<int> d_shift;
      if (!d_rings.alloc(rings.size(), "ring table", false) ||
          !hip_ok(hipMemcpy(d_rings, rings.data(), sizeof(FreezeRing) * rings.size(), hipMemcpyHostToDevice), "ring table up") ||
          !d_shift.alloc(b->B, "ring shifts", false))
        return false;
      k.n_ring_table = (int)rings.size(); k.d_ring_table = std::move(d_rings); k.d_shift = std::move(d_shift);
    }
    if (!hip_ok(hipMemcpyAsync(k.d_shift, shift.data(), sizeof(int) * b->B, hipMemcpyHostToDevice, b->stream), "ring shifts up")) return false;   // (pageable source: staged before the call returns)
    hipLaunchKernelGGL(ring_rotate_kernel, dim3(k.n_ring_table, b->B), dim3(256), 0, b->stream, k.d_ring_table.get(), k.d_shift.get());
    if (!hip_ok(hipGetLastError(), "ring rotate")) return false;
  }
  k.hop_s.assign(b->B, b->hop_host);
  k.ragged = false;
  for (bool& r : k.step_ragged) r = false;
  return true;
}
// ticks without new input until the last step fed has left the last stage
// output half of one call of the any-rate wrapper around the ticks (BeatriceBatch_BindResidentBlocks): its block's inner
// samples gathered from the resident model outputs, second resampling direction, output gain, into the call's slot
bool rb_post(BeatriceBatch* b, const BeatriceBatch::ResidentBlocks::Job& j) {
  BeatriceBatch::ResidentBlocks& r = b->rb;
  const size_t nt = b->wrap.taps_down.size();
  const int slot = (int)(j.call % r.n_slots), ge = (int)(j.call % r.ring);
  if (r.ragged)   // clocks per stream: the call's records name every stream's directions, sample count and block
    hipLaunchKernelGGL(wrapn::wrapr_post_kernel, dim3(b->B), dim3(256), 0, b->stream, r.d_out24, b->B, r.d_map, r.map_ring, b->d_wrap,
                       r.gains.host(ge) + b->B, b->rw.d_taps.get(), r.h_rs + (size_t)ge * b->B,
                       r.d_out + (size_t)slot * b->B * r.cell, r.channels);
  else   // (the gain segments where the host wrote them: pinned memory)
    hipLaunchKernelGGL(wrapn::wrap_post_kernel, dim3(b->B), dim3(256), 0, b->stream, r.d_out24, r.io_slots, b->B, b->H, j.t0, b->d_wrap,
                       r.gains.host(ge) + b->B, b->d_wrap_taps + (j.dout.decimate ? 0 : nt), j.dout,
                       r.d_out + (size_t)slot * b->B * r.channels * r.n, r.channels);
  // (the event frees the ring entry for the host)
  if (!r.gains.mark(ge, b->stream)) return false;
  return hip_ok(hipGetLastError(), "wrapper output half");
}
bool tick_drain(BeatriceBatch* b) {
  bool ok = true;
  if (b->tk.on && b->tk.d_trace && b->tk.last_feed_tick == b->tk.tick - 1 && b->tk.n_fed > b->tk.plan.count()) {
    // measurement aid: the tick just enqueued had every stage busy; dump its per-workgroup timeline (100 MHz wall clock)
    std::vector<unsigned long long> tr((size_t)3 * b->tk.table_total);
    if (hip_ok(hipStreamSynchronize(b->stream), "trace sync") &&
        hip_ok(hipMemcpy(tr.data(), b->tk.d_trace, tr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost), "trace copy"))
      if (FILE* f = std::fopen(bhip::meas_env("BEATRICE_HIP_TICK_TRACE"), "w")) {
        for (size_t i = 0; i < tr.size(); i += 3) std::fprintf(f, "%llu %llu %llu\n", tr[i], tr[i + 1], tr[i + 2]);
        std::fclose(f);
      }
  }
  while (ok && b->tk.on && b->tk.tick <= b->tk.last_feed_tick + b->tk.plan.count() - 1) ok = tick_run(b, false);
  if (ok && b->r48.on && b->r48.deferred_slot >= 0) {  // the 48 kHz block of the step the last tick completed
    BeatriceBatch::Resident48& r = b->r48;
    Wrap48TickArgs wa{};
    wa.channels = r.channels; wa.st = b->d_w48; wa.coef_down = b->d_coef_down; wa.coef_up = b->d_coef_up; wa.H = b->H;
    wa.n_post = b->B;
    wa.out48 = r.d_out48 + (size_t)r.deferred_slot * b->B * b->H * r.channels * 480;
    wa.model_out = r.d_out24 + (size_t)r.deferred_slot * b->B * b->H * B_OUT_HOP;
    wa.hv_post = r.deferred_step >= 0 && b->tk.step_ragged[r.deferred_step % tick::kRing] ? b->tk.d_hopv + (size_t)(r.deferred_step % tick::kRing) * b->tk.row : nullptr;
    wa.in48_post = r.d_in48 + (size_t)r.deferred_slot * b->B * b->H * r.channels * 480;
    r.deferred_slot = -1;
    ok = b->tk.resets.empty() || tick_reset_wrap48(b, b->stream, true);   // (a reset whose step is the one this launch emits)
    hipLaunchKernelGGL(wrap48_tick_kernel, dim3(wrap48_tick_grid(wa)), dim3(256), 0, b->stream, wa);
    ok = ok && hip_ok(hipGetLastError(), "wrap48 flush");
  }
  // every model hop that entered the pipeline has left it: the output halves still owed, in order.  With several hops per step
  // the hops of a step that is not full yet have not entered: the calls that end on them stay owed until later calls fill the
  // step (BeatriceBatch_ResidentBlocksOwed)
  while (ok && b->rb.on && !b->rb.jobs.empty() && b->rb.jobs.front().last_hop() < b->rb.hops_fed()) {
    ok = rb_post(b, b->rb.jobs.front());
    b->rb.jobs.pop_front();
  }
  if (ok && b->tk.on && b->tk.ragged) ok = tick_relevel(b);   // (nothing is in flight: back to one counter and the common launch)
  if (ok && b->tk.on) b->mv.seen.drained();
  return ok;
}
int tick_enable(BeatriceBatch* b, bool on) {
  using namespace tick;
  State& k = b->tk;
  if (on == k.on) return 0;
  if (on) {
    // one 10 ms hop per step, resident I/O with enough slots
    // that a step's input is still there when the pitch head reads it nine ticks on and outputs have somewhere to land
    if ((b->H != 1 && b->H != 2 && b->H != 4) || b->B > 4096 || b->io_slots < k.plan.count() + 1 || b->io_slots > stepc::kImmediateMaxSlot + 1) return -1;   // (the slot index travels in 12 bits of an immediate, ring.h stepc)
    if (!sync_all(b)) return -2;
    if (b->pipelined) { drop_graph(b); set_plan(b, 1); }
    k.snap_bytes = b->off.front_bytes + b->off.wave_bytes;
    if (!k.d_table) {   // (each group into locals first: a failure half-way leaves the batch as it was)
      const size_t tab_bytes = std::max(std::max(sizeof(Ops<1>::Tab), sizeof(Ops<2>::Tab)), sizeof(Ops<4>::Tab));
      DevBuf<unsigned char> table, table_sparse, snap;
      StagedRing<unsigned char> stage;
      if (!table.alloc(tab_bytes, "tick table", false) || !table_sparse.alloc(tab_bytes, "tick sparse table", false) ||
          !snap.alloc(k.snap_bytes * kRing, "tick snapshots", false) || !stage.alloc(State::kStaging, k.snap_bytes, "tick staging"))
        return -2;
      k.d_table = std::move(table); k.d_table_sparse = std::move(table_sparse); k.d_snap = std::move(snap); k.stage = std::move(stage);
    }
    if (b->H > 1 && !k.d_link_p) {   // the granules between the GRU cells of a step's hops (tick.hip.h); tag 0 = never written
      DevBuf<unsigned long long> link_q, link_p;
      PinnedBuf<int> dead;
      if (!link_q.alloc((size_t)(b->H - 1) * b->B * 128, "tick gru link") || !link_p.alloc((size_t)(b->H - 1) * b->B * 256, "tick gru link") ||
          !dead.alloc(1, "tick gru link flag"))
        return -2;
      k.d_link_q = std::move(link_q); k.d_link_p = std::move(link_p); k.h_link_dead = std::move(dead);
    }
    // the plain-order K / V copies the quad bodies read (rowchain.hip.h block_bq_body) exist in tick mode only: ~3 MB per
    // speaker that the in-order, stage-pipelined and large-batch modes never read
    if (!b->wave.legacy && !b->wave.d_ktp[0]) {
      const size_t kvf = (size_t)b->wave.n_slots * B_HID * B_KV_LEN;
      bool ok = true;
      for (int blk = 0; blk < B_NBLOCKS && ok; ++blk)
        ok = hip_ok(hipMalloc(reinterpret_cast<void**>(&b->wave.d_ktp[blk]), sizeof(float) * kvf), "plain K") &&
             hip_ok(hipMalloc(reinterpret_cast<void**>(&b->wave.d_vp[blk]), sizeof(float) * kvf), "plain V") &&
             hip_ok(hipMemset(b->wave.d_ktp[blk], 0, sizeof(float) * kvf), "plain K zero") && hip_ok(hipMemset(b->wave.d_vp[blk], 0, sizeof(float) * kvf), "plain V zero");
      // every entry that may hold a table (real speakers and morph slots): re-projected from the raw embeddings the batch keeps
      if (ok && b->n_speakers > 0) ok = project_speakers(b, 0, b->max_speakers);
      if (!ok) {
        for (int blk = 0; blk < B_NBLOCKS; ++blk) {
          if (b->wave.d_ktp[blk]) (void)hipFree(b->wave.d_ktp[blk]);
          if (b->wave.d_vp[blk]) (void)hipFree(b->wave.d_vp[blk]);
          b->wave.d_ktp[blk] = b->wave.d_vp[blk] = nullptr;
        }
        return -2;
      }
    }
    if (!hip_ok(hipDeviceSynchronize(), "tick sync")) return -2;
    k.tick = 0; k.n_fed = 0; k.last_feed_tick = -1000; k.snap_cur = -1; k.snap_next = 0;
    b->entries.clear_at_drained_point();   // (stamps of an earlier stay in tick mode: the pipeline is empty)
    k.resets.clear(); k.reset_pending.assign(b->B, 0); k.any_reset_pending = false; k.reset_launches = 0;
    k.ragged = false;
    b->mv.seen.start(b->B);
    for (bool& r : k.step_ragged) r = false;
    for (long long& f : k.fed_step) f = -1;
    k.table_dirty = true;
    k.on = true;
    for (int blk = 0; blk < B_NBLOCKS; ++blk) rebuild_tiles(b, blk);  // (tick mode cuts the attention rows into tiles AND quads)
    return 0;
  }
  if (!sync_all(b)) return -2;  // drains; streams that have sat steps out come back to the batch's counter (tick_relevel)
  if (k.ragged) return -2;
  if (k.any_reset_pending && !tick_reset_settle(b)) return -2;   // resets still waiting for their step: the drained form, now
  k.on = false;
  if (b->silent.on && !b->silent.d_rings) b->silent.on = false;   // (the rule was enabled for tick mode only)
  for (int blk = 0; blk < B_NBLOCKS; ++blk) {   // (see above: tick mode's own copies of the K / V tables)
    if (b->wave.d_ktp[blk]) (void)hipFree(b->wave.d_ktp[blk]);
    if (b->wave.d_vp[blk]) (void)hipFree(b->wave.d_vp[blk]);
    b->wave.d_ktp[blk] = b->wave.d_vp[blk] = nullptr;
  }
  k.table_dirty = true;
  for (int blk = 0; blk < B_NBLOCKS; ++blk) rebuild_tiles(b, blk);
  // the in-order chain reads its counters from device memory: hand them the host's values
  const int pair[2] = {b->hop_host, b->io_host};
  if (!hip_ok(hipMemcpy(b->d_hop_next, pair, sizeof(pair), hipMemcpyHostToDevice), "tick leave")) return -2;
  b->front_dirty = true;
  for (bool& w : b->wave_dirty) w = true;
  return 0;
}

