// batch_wrappers.hip.h -- the host-side wrappers of the batch API: 48 kHz blocks (in order and around the ticks), any host rate with gains (in order and around the ticks)
// (Part of batch.hip's translation unit: included there, after struct BeatriceBatch and the helpers above it; not a stand-alone header.)
#pragma once

// ---- 48 kHz blocks with the wrapper on the device ----------------------------------------------
static bool step_48k(BeatriceBatch* b, const float* d_in48, float* d_out48, int channels) {
  BeatriceBatch::SilentRule& sr = b->silent;
  const unsigned char* frozen = nullptr;
  int flag_slot = -1;
  if (sr.on && sr.any_next) {   // this step's flags travel to the device through a ring of staging copies; a slot is reused only
    const int e = (int)(sr.steps % BeatriceBatch::SilentRule::kDepth);   // after the step that read it has finished (its event)
    unsigned char* h = sr.flags.claim(e);
    if (!h) return false;
    std::memcpy(h, sr.next.data(), b->B);
    unsigned char* d = sr.flags.dev(e);
    BHIP_TRY(hipMemcpyAsync(d, h, b->B, hipMemcpyHostToDevice, b->stream));
    frozen = d;
    flag_slot = e;
  }
  if (sr.on) ++sr.steps;
  // the FIFO of the reference emits the PREVIOUS block's model output first (resample.h:346-361)
  hipLaunchKernelGGL(wrap48_post_kernel, dim3(b->B), dim3(256), 0, b->stream, b->d_w48, b->d_coef_up, d_out48, channels, frozen, d_in48);
  hipLaunchKernelGGL(wrap48_pre_kernel, dim3(b->B), dim3(256), 0, b->stream, d_in48, channels, b->d_w48, b->d_coef_down, b->d_in, frozen);
  if (frozen)
    hipLaunchKernelGGL(freeze_save_kernel, dim3(sr.n_rings, b->B), dim3(256), 0, b->stream, sr.d_rings, sr.d_keep, b->B, b->pitch.d_prev_q, sr.d_keep_prev_q);
  sr.in_block_step = true;
  const bool ok = step_device(b, nullptr, nullptr);   // (advance_kv / draw_codebooks skip the flagged streams)
  sr.in_block_step = false;
  if (frozen) {
    std::fill(sr.next.begin(), sr.next.end(), 0);
    sr.any_next = false;
  }
  if (!ok) return false;
  if (frozen)
    hipLaunchKernelGGL(freeze_fix_kernel, dim3(sr.n_rings, b->B), dim3(256), 0, b->stream, sr.d_rings, sr.d_keep, b->B, frozen, b->last_hop,
                       b->pitch.d_prev_q, sr.d_keep_prev_q);
  hipLaunchKernelGGL(wrap48_latch_kernel, dim3((b->B * 240 + 255) / 256), dim3(256), 0, b->stream, b->d_w48, b->wave.d_out, b->B, frozen);
  if (flag_slot >= 0 && !sr.flags.mark(flag_slot, b->stream)) return false;
  return hip_ok(hipGetLastError(), "wrap48");
}
static bool freeze_prepare(BeatriceBatch* b);
// The shell's rule "a block whose down-mix is all zeros is not converted" (reference src/vst/processor.cc:204-214), per stream,
// for the in-order 48 kHz blocks: BeatriceBatch_ConvertBlocks48k (host buffers) finds the silent streams itself, exactly as the
// shell does (every sample of (L + R) * 0.5, or of L, equal to 0.0f); with device buffers the caller names them for the next
// block with BeatriceBatch_SetSilentStreams.  A silent stream's output block is its (zero) down-mix on every channel; its model
// state, its wrapper state (filter histories, the pending 10 ms of the FIFO), its pending key/value installs and its codebook
// lottery stand still, as if the block had never existed.
int BeatriceBatch_EnableSilentBlockRule(BeatriceBatch* b, int enable) {
  BATCH_OPEN(b);
  // (G, P refuse both directions: a resident-block binding owns the rule's flags while it is bound -- BindResidentBlocksRagged names the
  // streams whose FIFO did not fire through silent.next; switching the rule off underneath it would advance every stream on every fired
  // step while the key/value installs and the codebook lottery still skip the flagged ones)
  BATCH_GATE(b, enable ? Entry::EnableSilentBlockRule_1 : Entry::EnableSilentBlockRule_0);
  BeatriceBatch::SilentRule& sr = b->silent;
  if (!enable) {
    if (sr.on) { (void)sync_all(b); if (b->rw.ready) sr.on = false; else sr = {}; }   // (the per-stream wrapper keeps the freeze machinery)
    return 0;
  }
  if (sr.on) return 0;
  if (b->tk.on) {   // tick mode (plain resident I/O): the flagged streams sit the next STEP out -- their step counters stand still and
                    // travel with every step from then on (batch_tick.hip.h, ragged steps); with the 48 kHz wrapper around the ticks
                    // (BindResidentIO48k) that is the shell's rule on its blocks -- at two / four blocks per step on a stream's WHOLE step
    sr.next.assign(b->B, 0);
    sr.any_next = false;
    sr.on = true;
    return 0;
  }
  if (!sync_all(b)) return -2;   // the in-order chain, one block per step
  if (!freeze_prepare(b)) return -2;
  sr.on = true;
  drop_graph(b);
  return 0;
}
// what a step that leaves some streams standing needs (the silent-block rule of the 48 kHz blocks, and the per-stream clocks of
// BeatriceBatch_ProcessBlocksRagged): the list of state rings to put back, room for the single-slot ones, the flag staging
static bool freeze_prepare(BeatriceBatch* b) {
  BeatriceBatch::SilentRule& sr = b->silent;
  if (sr.d_rings) return true;
  std::vector<FreezeRing> rings;
  size_t keep = 0;
  for (const RingArena* a : {&b->phone.arena, &b->pitch.arena, &b->wave.arena})
    for (const Ring* r : a->rings) {
      FreezeRing f{r->base, r->n * r->C, r->m, 0};
      if (r->m == 1) { f.keep_off = keep; keep += (size_t)b->B * f.slot_floats; }
      rings.push_back(f);
    }
  DevBuf<FreezeRing> d_rings;
  DevBuf<float> d_keep;
  DevBuf<int> d_keep_prev_q;
  StagedRing<unsigned char> flags;
  if (!d_rings.alloc(rings.size(), "silent rings", false) ||
      !hip_ok(hipMemcpy(d_rings, rings.data(), sizeof(FreezeRing) * rings.size(), hipMemcpyHostToDevice), "silent rings up") ||
      !d_keep.alloc(std::max<size_t>(keep, 1), "silent keep", false) || !d_keep_prev_q.alloc(b->B, "silent prev_q", false) ||
      !flags.alloc(BeatriceBatch::SilentRule::kDepth, b->B, "silent flags", true))
    return false;
  sr.n_rings = (int)rings.size();
  sr.d_rings = std::move(d_rings); sr.d_keep = std::move(d_keep); sr.d_keep_prev_q = std::move(d_keep_prev_q); sr.flags = std::move(flags);
  sr.next.assign(b->B, 0);
  sr.any_next = false;
  return true;
}
// streams whose NEXT 48 kHz block is silent by the shell's rule (flags[B], non-zero = silent); cleared by that block
int BeatriceBatch_SetSilentStreams(BeatriceBatch* b, const unsigned char* flags) {
  if (!b || !b->ok) return -2;
  BATCH_GATE(b, Entry::SetSilentStreams);
  if (!flags) return -1;
  b->silent.any_next = false;
  for (int s = 0; s < b->B; ++s) { b->silent.next[s] = flags[s] ? 1 : 0; b->silent.any_next = b->silent.any_next || flags[s]; }
  return 0;
}
// Throughput form of the 48 kHz wrapper: n_slots resident 48 kHz blocks per direction, the tick pipeline between them.
// Block k (BeatriceBatch_ConvertBlocks48kDevice(b, NULL, NULL, channels)) is read from slot k mod n_slots; its converted
// block lands in the same slot of d_out48 BeatriceBatch_TickStages() - 1 calls later (or after BeatriceBatch_Synchronize).
// Same samples as the in-order BeatriceBatch_ConvertBlocks48kDevice.  NULL pointers unbind.
int BeatriceBatch_BindResidentIO48k(BeatriceBatch* b, const float* d_in48, float* d_out48, int channels, int n_slots) {
  BATCH_OPEN(b);
  const bool bind = d_in48 || d_out48;
  if (bind) BATCH_GATE(b, Entry::BindResidentIO48k_bind);
  BeatriceBatch::Resident48& r = b->r48;
  if (r.on) {
    if (!sync_all(b)) return -2;
    const int rc = tick_enable(b, false);
    if (rc) return rc;
    (void)bind_io(b, nullptr, nullptr, 0);
    r = {};
  }
  if (!bind) return 0;
  BATCH_GATE(b, Entry::BindResidentIO48k_bind);   // (again: the mode the batch is in now that it has left F)
  if (!d_in48 || !d_out48 || channels < 1 || channels > 2 || n_slots < b->tk.plan.count() + 1) return -1;
  // (with H hops per step a slot holds H blocks per stream, [B][H][channels][480], and a call converts them all)
  DevBuf<float> d_in16, d_out24;
  const bool ok = d_in16.alloc((size_t)n_slots * b->B * b->H * B_IN_HOP, "r48 in16") && d_out24.alloc((size_t)n_slots * b->B * b->H * B_OUT_HOP, "r48 out24", false) &&
                  bind_io(b, d_in16, d_out24, n_slots) == 0 && tick_enable(b, true) == 0;
  if (!ok) {
    (void)tick_enable(b, false);
    (void)bind_io(b, nullptr, nullptr, 0);
    return -2;
  }
  r.d_in16 = std::move(d_in16); r.d_out24 = std::move(d_out24);
  r.d_in48 = d_in48; r.d_out48 = d_out48; r.channels = channels; r.n_slots = n_slots; r.on = true;
  return 0;
}
int BeatriceBatch_ConvertBlocks48kDevice(BeatriceBatch* b, const float* d_in, float* d_out, int channels) {
  BATCH_ENTER(b, d_in || d_out ? Entry::ConvertBlocks48kDevice_ptrs : Entry::ConvertBlocks48kDevice_NULL);
  if (!d_in && !d_out) return channels == b->r48.channels ? (tick_run(b, true) ? 0 : -2) : -1;   // (F: the next resident block)
  if (channels < 1 || channels > 2 || !d_in || !d_out) return -1;  // per 10 ms block, in order
  return step_48k(b, d_in, d_out, channels) ? 0 : -2;
}
int BeatriceBatch_ConvertBlocks48k(BeatriceBatch* b, const float* in, float* out, int channels) {
  BATCH_ENTER(b, Entry::ConvertBlocks48k);
  if (channels < 1 || channels > 2 || !in || !out) return -1;
  const size_t n = (size_t)b->B * channels * 480;
  float* h_in = b->h_io48;
  float* h_out = b->h_io48 + (size_t)b->B * 2 * 480;
  float* d_in = b->d_io48;
  float* d_out = b->d_io48 + (size_t)b->B * 2 * 480;
  if (b->silent.on) {   // the shell's test, per stream: every sample of the down-mix equal to 0.0f
    BeatriceBatch::SilentRule& sr = b->silent;
    sr.any_next = false;
    for (int st = 0; st < b->B; ++st) {
      const float* src = in + (size_t)st * channels * 480;
      bool sil = true;
      for (int i = 0; i < 480 && sil; ++i) {
        float m = src[i];
        if (channels >= 2) { m = m + src[480 + i]; m = m * 0.5f; }
        sil = !(m != 0.0f);
      }
      sr.next[st] = sil ? 1 : 0;
      sr.any_next = sr.any_next || sil;
    }
  }
  std::memcpy(h_in, in, sizeof(float) * n);
  bool ok = hip_ok(hipMemcpyAsync(d_in, h_in, sizeof(float) * n, hipMemcpyHostToDevice, b->stream), "in48");
  ok = ok && step_48k(b, d_in, d_out, channels);
  ok = ok && hip_ok(hipMemcpyAsync(h_out, d_out, sizeof(float) * n, hipMemcpyDeviceToHost, b->stream), "out48");
  ok = hip_ok(hipStreamSynchronize(b->stream), "sync") && ok;
  b->inflight = false;
  if (ok) std::memcpy(out, h_out, sizeof(float) * n);
  else std::memset(out, 0, sizeof(float) * n);
  return ok ? 0 : -2;
}

// ---- the shell's silent-block test on blocks that live on the device (silent_scan_plan.h, silent_scan.hip) ------------
// What the loop of BeatriceBatch_ConvertBlocks48k above does on host buffers, for a caller whose audio is resident: the flags that
// BeatriceBatch_SetSilentStreams / ProcessBlocksRaggedDevice's n_samples = 0 take.  A scan is the caller's question about the caller's
// memory: it runs on a stream of its own (or the caller's), reads no state of the batch but the scan's own ring and -- the bound form --
// where the resident slots are, and writes none.  Results: the kernel stores one byte per block into the entry's DEVICE buffer and one
// copy on the scan's stream brings them to the entry's pinned block (not the kernel's own stores over the host link: a byte per
// wavefront, each its own transaction); the event behind that copy is all an End waits for.
namespace {
int scan_begin(BeatriceBatch* b, const float* d_blocks, const sscan::Geometry& g, const int* cell_samples, hipStream_t st) {
  BeatriceBatch::SilentScan& sc = b->scan;
  const int e = sc.tickets.free_entry();
  if (e < 0) return -3;
  if (!st) {
    if (!sc.stream && !sc.stream.create("scan stream")) return -2;
    st = sc.stream;
  }
  BeatriceBatch::SilentScan::Entry& en = sc.entry[e];
  const size_t need = (size_t)g.blocks();
  if (en.d_flags.size() < need) {   // (a free entry has no reader left: its last End waited for its event)
    size_t cap = 1024;
    while (cap < need) cap *= 2;
    DevBuf<unsigned char> d_flags;
    PinnedBuf<unsigned char> h_flags;
    PinnedBuf<int> h_len;
    if (!d_flags.alloc(cap, "scan flags", false) || !h_flags.alloc(cap, "scan flags host") || !h_len.alloc(cap, "scan lengths")) return -2;
    en.d_flags = std::move(d_flags); en.h_flags = std::move(h_flags); en.h_len = std::move(h_len);
  }
  if (!en.done && !en.done.create("scan event")) return -2;
  const int* len = nullptr;
  if (g.ragged) {   // the kernel reads the lengths in place
    std::memcpy(en.h_len.get(), cell_samples, sizeof(int) * (size_t)g.n_cells);
    len = en.h_len;
  }
  const bool ok = silent_scan(d_blocks, g, sscan::vector_path(d_blocks, g), len, en.d_flags, st) &&
                  hip_ok(hipMemcpyAsync(en.h_flags.get(), en.d_flags.get(), need, hipMemcpyDeviceToHost, st), "scan flags down") &&
                  hip_ok(hipEventRecord(en.done, st), "scan event");
  if (!ok) {   // no ticket is given out, so the entry stays free: whatever of the scan was enqueued is waited for before a later Begin may
    (void)hipStreamSynchronize(st);   // reuse or regrow the buffers it writes and reads
    return -2;
  }
  return sc.tickets.issue(e, g.blocks());
}
int scan_end(BeatriceBatch* b, int ticket, unsigned char* flags) {
  BeatriceBatch::SilentScan& sc = b->scan;
  const int e = sc.tickets.entry_of(ticket);
  if (e < 0) return -1;
  const bool ok = hip_ok(hipEventSynchronize(sc.entry[e].done), "scan wait");
  if (ok) std::memcpy(flags, sc.entry[e].h_flags.get(), (size_t)sc.tickets.blocks_of(e));
  sc.tickets.end(e);
  return ok ? 0 : -2;
}
}  // namespace
int BeatriceBatch_ScanSilentBlocksBegin(BeatriceBatch* b, const float* d_blocks, int n_cells, int blocks_per_cell, int channels, int n_samples,
                                        long long cell_stride, const int* cell_samples, void* hip_stream) {
  BATCH_OPEN(b);
  sscan::Geometry g;
  if (!sscan::accept(d_blocks, n_cells, blocks_per_cell, channels, n_samples, cell_stride, cell_samples, true, &g)) return -1;
  return scan_begin(b, d_blocks, g, cell_samples, static_cast<hipStream_t>(hip_stream));
}
int BeatriceBatch_ScanSilentBlocksEnd(BeatriceBatch* b, int ticket, unsigned char* flags) {
  BATCH_OPEN(b);
  if (!flags) return -1;
  return scan_end(b, ticket, flags);
}
int BeatriceBatch_ScanSilentBlocks(BeatriceBatch* b, const float* d_blocks, int n_cells, int blocks_per_cell, int channels, int n_samples,
                                   long long cell_stride, const int* cell_samples, void* hip_stream, unsigned char* flags) {
  BATCH_OPEN(b);
  sscan::Geometry g;
  if (!sscan::accept(d_blocks, n_cells, blocks_per_cell, channels, n_samples, cell_stride, cell_samples, flags != nullptr, &g)) return -1;
  const int ticket = scan_begin(b, d_blocks, g, cell_samples, static_cast<hipStream_t>(hip_stream));
  return ticket < 0 ? ticket : scan_end(b, ticket, flags);
}
// Mode F: the slots the NEXT n_calls calls of BeatriceBatch_ConvertBlocks48kDevice(b, NULL, NULL, channels) read -- call k reads slot
// (the host's slot counter + k) mod n_slots, tick_run -- as cells [B][H][channels][480].  The ring of slots may wrap inside the range: two
// scans then, side by side.
int BeatriceBatch_ScanBoundBlocks48k(BeatriceBatch* b, int n_calls, unsigned char* step_flags, unsigned char* block_flags, void* hip_stream) {
  BATCH_ENTER(b, Entry::ConvertBlocks48kDevice_NULL);
  const BeatriceBatch::Resident48& r = b->r48;
  const long long per_slot = (long long)b->B * b->H;
  if (!step_flags || n_calls < 1 || n_calls > r.n_slots || n_calls * per_slot > sscan::kMaxBlocks) return -1;
  const int first = b->io_host, n1 = std::min(n_calls, r.n_slots - first), n2 = n_calls - n1;
  const long long cell = (long long)b->H * r.channels * 480;
  if (b->scan.tickets.free_entries() < (n2 > 0 ? 2 : 1)) return -3;
  sscan::Geometry g1, g2;
  const float* p1 = r.d_in48 + (size_t)first * b->B * cell;
  if (!sscan::accept(p1, (long long)n1 * b->B, b->H, r.channels, 480, cell, nullptr, true, &g1) ||
      (n2 > 0 && !sscan::accept(r.d_in48, (long long)n2 * b->B, b->H, r.channels, 480, cell, nullptr, true, &g2)))
    return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const int t1 = scan_begin(b, p1, g1, nullptr, st);
  if (t1 < 0) return t1;
  const int t2 = n2 > 0 ? scan_begin(b, r.d_in48, g2, nullptr, st) : 0;
  std::vector<unsigned char> blocks((size_t)(n_calls * per_slot));
  int rc = scan_end(b, t1, blocks.data());
  if (n2 > 0 && t2 >= 0) { const int rc2 = scan_end(b, t2, blocks.data() + (size_t)(n1 * per_slot)); rc = rc ? rc : rc2; }
  if (t2 < 0) rc = t2;
  if (rc) return rc;
  for (long long i = 0; i < n_calls * (long long)b->B; ++i) {   // footnote (6): a stream sits a step out when ALL its blocks of the step are silent
    unsigned char all = 1;
    for (int hh = 0; hh < b->H; ++hh) all = all && blocks[(size_t)(i * b->H + hh)];
    step_flags[i] = all;
  }
  if (block_flags) std::memcpy(block_flags, blocks.data(), blocks.size());
  return 0;
}

// ---- host-rate blocks with the whole wrapper on the device (wrapper.hip.h) -------------------------------------------
namespace { constexpr int kInnerStride = wrapn::kMaxSamples + 64; }
int BeatriceBatch_ConfigureWrapper(BeatriceBatch* b, double sample_rate) {
  BATCH_ENTER(b, Entry::ConfigureWrapper);   // (G, P: the binding restarts the wrapper itself when it is made and released; several hops per step: for BeatriceBatch_BindResidentBlocks)
  if (!sync_all(b)) return -2;
  // rate <= 0, or a ratio whose filter history exceeds the state block: refused on a class of its own, so that the configured one -- its
  // ratio, its tables, `ready` -- stands and the next blocks go on as if nobody had asked
  wrapn::RateClass fresh;
  if (!fresh.configure(sample_rate)) return -1;
  b->wrap = std::move(fresh);
  b->wrap_clk = b->wrap.start();
  const int B = b->B;
  const size_t nt = b->wrap.taps_down.size();
  bool ok = true;
  if (!b->d_wrap) {
    DevBuf<wrapn::StreamState> state;
    DevBuf<float> inner, io;
    PinnedBuf<float> h_io;
    Mirror<wrapn::GainSeg> gains;
    ok = state.alloc(B, "wrap state", false) && inner.alloc((size_t)B * kInnerStride, "wrap inner", false) &&
         io.alloc((size_t)B * 4 * wrapn::kMaxSamples, "wrap io", false) && h_io.alloc((size_t)B * 4 * wrapn::kMaxSamples, "wrap io host") &&
         gains.alloc(2 * (size_t)B, 2 * (size_t)B, "wrap gains", false);
    if (ok) {
      b->d_wrap = std::move(state); b->d_wrap_inner = std::move(inner); b->d_wrap_io = std::move(io); b->h_wrap_io = std::move(h_io);
      b->wrap_gains = std::move(gains);
      b->gain_in.assign(B, wrapn::GainClock());
      b->gain_out.assign(B, wrapn::GainClock());
    }
  }
  ok = ok && b->d_wrap_taps.alloc(2 * nt, "wrap taps", false) &&
       hip_ok(hipMemcpy(b->d_wrap_taps, b->wrap.taps_down.data(), sizeof(float) * nt, hipMemcpyHostToDevice), "taps down") &&
       hip_ok(hipMemcpy(b->d_wrap_taps + nt, b->wrap.taps_up.data(), sizeof(float) * nt, hipMemcpyHostToDevice), "taps up") &&
       hip_ok(hipMemset(b->d_wrap, 0, sizeof(wrapn::StreamState) * B), "wrap state0") && hip_ok(hipDeviceSynchronize(), "wrap sync");
  b->wrap_gains_constant = false;
  // (a new rate restarts the resampler and the FIFO as the reference's SetSampleRate does; the gains keep their state,
  //  now ramping at the new rate: reference processor_core_2.cc:421-429)
  return ok ? 0 : -2;
}
// reference ProcessorCore2::SetInputGain / SetOutputGain (processor_core_2.cc:488-496): the target; the ramp follows at 2 dB/ms
int BeatriceBatch_SetInputGain(BeatriceBatch* b, int stream, double db) {
  BATCH_OPEN(b);
  if (stream < -1 || stream >= b->B || b->gain_in.empty()) return -1;
  for (int s = (stream < 0 ? 0 : stream); s < (stream < 0 ? b->B : stream + 1); ++s) b->gain_in[s].target_db = db;
  return 0;
}
int BeatriceBatch_SetOutputGain(BeatriceBatch* b, int stream, double db) {
  BATCH_OPEN(b);
  if (stream < -1 || stream >= b->B || b->gain_out.empty()) return -1;
  for (int s = (stream < 0 ? 0 : stream); s < (stream < 0 ? b->B : stream + 1); ++s) b->gain_out[s].target_db = db;
  return 0;
}
static bool wrap_chunk(BeatriceBatch* b, const float* d_in, float* d_out, int channels, int n) {
  using namespace wrapn;
  const int B = b->B;
  hipStream_t st = b->stream;
  const RateClass& w = b->wrap;
  ClockPlan p;
  if (!plan_clocks(w, b->wrap_clk, n, p)) return false;   // (a plan that does not fit: no clock has moved)
  // gains: this call's segment per stream; the device copy is refreshed unless it already holds the same constants
  bool all_constant = true;
  GainSeg* seg = b->wrap_gains.h;
  for (int s = 0; s < B; ++s) {
    const GainSeg gi = b->gain_in[s].advance(n, w.rate), go = b->gain_out[s].advance(n, w.rate);
    all_constant = all_constant && gi.step == 1.0 && go.step == 1.0 && seg[s].step == 1.0 && seg[B + s].step == 1.0 &&
                   seg[s].amp0 == gi.amp0 && seg[B + s].amp0 == go.amp0;
    seg[s] = gi;
    seg[B + s] = go;
  }
  if (!(all_constant && b->wrap_gains_constant)) {
    const size_t off = 0, len = 2 * (size_t)B;
    GainSeg* dst = nullptr;
    if (!b->wrap_gains.push_parts(st, 1, &off, &len, &dst)) return false;
    b->wrap_gains_constant = all_constant;
  }
  const size_t nt = w.taps_down.size();
  hipLaunchKernelGGL(wrap_in_kernel, dim3(B), dim3(256), 0, st, d_in, channels, n, b->d_wrap, b->wrap_gains.d, b->d_wrap_taps + (p.din.decimate ? 0 : nt), p.din,
                     b->d_wrap_inner, kInnerStride);
  for (int c = 0; c < p.cut.n; ++c) {  // the exact-480 FIFO; a model hop every time it fills
    const int fires = p.cut.fires[c];
    hipLaunchKernelGGL(wrap_fifo_kernel, dim3(B), dim3(256), 0, st, b->d_wrap_inner, kInnerStride, b->d_wrap, (int)p.cut.at[c], (int)p.cut.fill[c], (int)p.cut.take[c], fires, b->d_in, B_IN_HOP);
    if (!fires) continue;
    if (!step_device(b, nullptr, nullptr)) return false;
    hipLaunchKernelGGL(wrap_refill_kernel, dim3((B * kBlock + 255) / 256), dim3(256), 0, st, b->d_wrap, b->wave.d_out, B);
  }
  hipLaunchKernelGGL(wrap_out_kernel, dim3(B), dim3(256), 0, st, b->d_wrap_inner, kInnerStride, b->d_wrap, b->wrap_gains.d + B,
                     b->d_wrap_taps + (p.dout.decimate ? 0 : nt), p.dout, d_out, channels);
  return hip_ok(hipGetLastError(), "wrapper launch");
}
// in / out: [B][channels][n] planar at the configured host rate; any n >= 1 (long blocks are processed in pieces)
int BeatriceBatch_ProcessBlocksDevice(BeatriceBatch* b, const float* d_in, float* d_out, int channels, int n) {
  BATCH_ENTER(b, d_in || d_out ? Entry::ProcessBlocksDevice_ptrs : Entry::ProcessBlocksDevice_NULL);
  if (!d_in && !d_out) {   // (G: the next resident block)
    if (channels != b->rb.channels || n != b->rb.n) return -1;
    if (b->rb.dead) return -2;
    if (!rb_step(b)) { b->rb.dead = true; return -2; }   // (a call that failed behind its commit -- a launch, a tick, the gain ring -- leaves the binding unusable, not silently skewed)
    return 0;
  }
  if (channels < 1 || channels > 2 || !d_in || !d_out || n < 1) return -1;
  if (n > wrapn::longest_block(b->wrap.rate)) return -1;  // the planar layout [B][channels][n] cannot be cut without copies: callers pass blocks of at most that many samples
  return wrap_chunk(b, d_in, d_out, channels, n) ? 0 : -2;
}
int BeatriceBatch_MaxWrapperBlock(const BeatriceBatch* b) { return b && b->ok && b->wrap.ready ? wrapn::longest_block(b->wrap.rate) : 0; }

// ---- clocks per stream: a batch whose streams come from different hosts -------------------------------------------------------------
// rates[B]: the host rate of every stream (streams of equal rate share their tap tables).  Restarts every stream's resampler
// pair and FIFO as SetSampleRate does; the gains keep their state.  In-order mode, one hop per step.
int BeatriceBatch_ConfigureWrapperRates(BeatriceBatch* b, const double* rates) {
  BATCH_ENTER(b, Entry::ConfigureWrapperRates);
  if (!rates) return -1;
  if (!sync_all(b)) return -2;
  BeatriceBatch::RaggedWrap& r = b->rw;
  const int B = b->B;
  std::vector<wrapn::RateClass> classes;
  std::vector<int> cls(B);
  for (int s = 0; s < B; ++s) {
    int c = -1;
    for (size_t i = 0; i < classes.size(); ++i) if (classes[i].rate == rates[s]) { c = (int)i; break; }
    if (c < 0) {
      wrapn::RateClass p;
      if (!p.configure(rates[s])) return -1;
      classes.push_back(p);
      c = (int)classes.size() - 1;
    }
    cls[s] = c;
  }
  // the uniform wrapper's per-stream state, inner buffer, I/O staging and gain mirrors are shared with this mode
  if (!b->d_wrap) { const int rc = BeatriceBatch_ConfigureWrapper(b, rates[0]); if (rc) return rc; }
  if (!freeze_prepare(b)) return -2;
  std::vector<float> taps;
  std::vector<int> taps_down_off, taps_up_off;
  for (const wrapn::RateClass& p : classes) {
    taps_down_off.push_back((int)taps.size()); taps.insert(taps.end(), p.taps_down.begin(), p.taps_down.end());
    taps_up_off.push_back((int)taps.size()); taps.insert(taps.end(), p.taps_up.begin(), p.taps_up.end());
  }
  DevBuf<float> d_taps;
  StagedRing<wrapn::RagStream> rs;
  DevBuf<unsigned char> d_frozen;
  bool ok = d_taps.alloc(taps.size(), "ragged taps", false) &&
            hip_ok(hipMemcpy(d_taps, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice), "ragged taps up");
  const bool first = r.rs.entries() == 0;   // (the staging of the records is built once; the taps with every call)
  if (first) ok = ok && rs.alloc(r.kStage, B, "ragged records", true) && d_frozen.alloc((size_t)wrapn::kMaxChunks * B, "ragged flags", false);
  ok = ok && hip_ok(hipMemset(b->d_wrap, 0, sizeof(wrapn::StreamState) * B), "ragged state0") && hip_ok(hipDeviceSynchronize(), "ragged sync");
  if (!ok) return -2;
  r.d_taps = std::move(d_taps); r.taps_down_off = taps_down_off; r.taps_up_off = taps_up_off;
  // (drained: what a binding's rate changes outgrew goes now, wrapper_turnover_plan.h rule 4)
  r.arena.start(0, 0); r.h_taps.reset(); r.d_taps_outgrown.clear(); r.h_taps_outgrown.clear();
  if (first) { r.rs = std::move(rs); r.d_frozen = std::move(d_frozen); }
  r.classes = classes;
  r.cls = cls;
  r.clk.resize(B);
  for (int s = 0; s < B; ++s) r.clk[s] = classes[cls[s]].start();
  b->wrap.ready = false;          // (the uniform entry points are off until BeatriceBatch_ConfigureWrapper is called again)
  b->wrap_gains_constant = false;
  drop_graph(b);
  r.ready = true;
  return 0;
}
// One active stream's share of a call with per-stream clocks, planned on the state the call would leave (rw.next): its gain segments, the
// two resampling directions and the pieces its inner samples are cut into at the 480-sample FIFO.  false: the plan does not fit the
// kernels' buffers -- the caller refuses the call, and no clock of any of its streams has moved.
static bool rag_plan(BeatriceBatch* b, int s, int n, wrapn::RagStream& q, wrapn::GainSeg* seg) {
  BeatriceBatch::RaggedWrap& r = b->rw;
  const int c = r.cls[s];
  wrapn::CallPlan p;
  if (!r.next.plan(r.classes[c], s, n, p)) return false;
  q.din = p.din; q.dout = p.dout;
  p.cut.put(q);
  q.taps_in = q.din.decimate ? r.taps_down_off[c] : r.taps_up_off[c];
  q.taps_out = q.dout.decimate ? r.taps_down_off[c] : r.taps_up_off[c];
  seg[s] = p.gain_in; seg[b->B + s] = p.gain_out;
  return true;
}
// the streams that fire a model hop in piece `ci` of such a call: silent.next flags the others for the step that follows
struct RagFires { bool any, any_out; };
static RagFires rag_fires(BeatriceBatch* b, const wrapn::RagStream* rs, int ci) {
  RagFires f{false, false};
  for (int s = 0; s < b->B; ++s) {
    const bool fires = rs[s].active && ci < rs[s].n_chunks && rs[s].fires[ci];
    b->silent.next[s] = fires ? 0 : 1;
    f.any = f.any || fires; f.any_out = f.any_out || !fires;
  }
  return f;
}
// Host buffers through the wrapper's pinned staging pair: cnt floats in, what `enqueue(d_in, d_out)` puts on the stream, cnt floats out,
// everything waited for; zeros where anything failed.
extern "C++" template <class F>
static int wrap_round_trip(BeatriceBatch* b, const float* in, float* out, size_t cnt, F enqueue) {
  const size_t half = (size_t)b->B * 2 * wrapn::kMaxSamples, bytes = sizeof(float) * std::max<size_t>(cnt, 1);
  float* h_in = b->h_wrap_io; float* h_out = h_in + half; float* d_in = b->d_wrap_io; float* d_out = d_in + half;
  std::memcpy(h_in, in, sizeof(float) * cnt);
  bool ok = hip_ok(hipMemcpyAsync(d_in, h_in, bytes, hipMemcpyHostToDevice, b->stream), "wrap in");
  ok = ok && enqueue(d_in, d_out);
  ok = ok && hip_ok(hipMemcpyAsync(h_out, d_out, bytes, hipMemcpyDeviceToHost, b->stream), "wrap out");
  ok = hip_ok(hipStreamSynchronize(b->stream), "wrap sync") && ok;
  b->inflight = false;
  if (ok) std::memcpy(out, h_out, sizeof(float) * cnt);
  else std::memset(out, 0, sizeof(float) * cnt);
  return ok ? 0 : -2;
}
// One call = for every stream s a block of n_samples[s] host samples at ITS rate (0: the stream sits this call out).  in / out:
// the streams' planar blocks [channels][n_samples[s]] one after the other.  apply_silent_rule != 0: a block whose down-mix is
// all zeros is not converted (src/vst/processor.cc:204-214): nothing of that stream moves -- gains, resampler clocks, FIFO,
// model state, key/value installs, codebook lottery -- and its output block is zeros.  Streams fire their model hops when
// THEIR 480-sample FIFO fills; a step runs for the streams that fire in it and leaves the others standing.
int BeatriceBatch_ProcessBlocksRagged(BeatriceBatch* b, const float* in, float* out, int channels, const int* n_samples, int apply_silent_rule) {
  using namespace wrapn;
  BATCH_ENTER(b, Entry::ProcessBlocksRagged);
  BeatriceBatch::RaggedWrap& r = b->rw;
  if (!in || !out || !n_samples || channels < 1 || channels > 2) return -1;
  const int B = b->B;
  hipStream_t st = b->stream;
  size_t total = 0;
  for (int s = 0; s < B; ++s) {
    if (n_samples[s] < 0 || n_samples[s] > longest_block(r.rate(s))) return -1;
    total += (size_t)channels * n_samples[s];
  }
  const int e = (int)(r.calls % r.kStage);
  RagStream* rs = r.rs.claim(e);
  if (!rs) return -2;
  GainSeg* seg = b->wrap_gains.h;
  int max_chunks = 0;
  size_t off = 0;
  // (all or nothing: the streams are planned on the state the call would leave, which becomes the batch's once the last plan stands --
  //  otherwise host and device state of the streams planned before a refusal would part ways)
  r.next.begin(r.clk, b->gain_in, b->gain_out);
  for (int s = 0; s < B; ++s) {
    RagStream& q = rs[s];
    q = RagStream{};
    const int n = n_samples[s];
    q.io_off = (long long)off; q.n = n;
    bool active = n > 0;
    if (active && apply_silent_rule) {   // the shell's own test on the down-mix
      const float* src = in + off;
      bool sil = true;
      for (int i = 0; i < n && sil; ++i) {
        float m = src[i];
        if (channels >= 2) { m = m + src[n + i]; m = m * 0.5f; }
        sil = !(m != 0.0f);
      }
      active = !sil;
    }
    off += (size_t)channels * n;
    q.active = active ? 1 : 0;
    if (!active) { seg[s] = GainSeg{1.0, 1.0, 1.0}; seg[B + s] = GainSeg{1.0, 1.0, 1.0}; continue; }
    if (!rag_plan(b, s, n, q, seg)) return -2;
    max_chunks = std::max(max_chunks, q.n_chunks);
  }
  r.next.commit(r.clk, b->gain_in, b->gain_out);
  // uploads: the per-stream records of this call, the gain segments, the audio
  RagStream* d_rs = r.rs.dev(e);
  bool up = hip_ok(hipMemcpyAsync(d_rs, rs, sizeof(RagStream) * B, hipMemcpyHostToDevice, st), "ragged records up");
  { const size_t o0 = 0, len = 2 * (size_t)B; GainSeg* dst = nullptr; up = up && b->wrap_gains.push_parts(st, 1, &o0, &len, &dst); }
  b->wrap_gains_constant = false;
  if (!up) return -2;
  return wrap_round_trip(b, in, out, total, [&](const float* d_in, float* d_out) {
    hipLaunchKernelGGL(wrapr_in_kernel, dim3(B), dim3(256), 0, st, d_in, channels, b->d_wrap, b->wrap_gains.d, r.d_taps, d_rs, b->d_wrap_inner, kInnerStride);
    BeatriceBatch::SilentRule& sr = b->silent;
    bool ok = true;
    for (int ci = 0; ci < max_chunks && ok; ++ci) {
      const RagFires f = rag_fires(b, rs, ci);
      unsigned char* d_flags = r.d_frozen + (size_t)ci * B;
      hipLaunchKernelGGL(wrapr_fifo_kernel, dim3(B), dim3(256), 0, st, b->d_wrap_inner, kInnerStride, b->d_wrap, d_rs, ci, b->d_in, d_flags, nullptr, 0, 0);
      if (!f.any) { std::fill(sr.next.begin(), sr.next.end(), 0); continue; }
      sr.any_next = f.any_out;
      if (f.any_out)
        hipLaunchKernelGGL(freeze_save_kernel, dim3(sr.n_rings, B), dim3(256), 0, st, sr.d_rings, sr.d_keep, B, b->pitch.d_prev_q, sr.d_keep_prev_q);
      sr.in_block_step = true;
      ok = step_device(b, nullptr, nullptr);   // (advance_kv / draw_codebooks skip the streams flagged in sr.next)
      sr.in_block_step = false;
      std::fill(sr.next.begin(), sr.next.end(), 0);
      sr.any_next = false;
      if (!ok) break;
      if (f.any_out)
        hipLaunchKernelGGL(freeze_fix_kernel, dim3(sr.n_rings, B), dim3(256), 0, st, sr.d_rings, sr.d_keep, B, d_flags, b->last_hop, b->pitch.d_prev_q, sr.d_keep_prev_q);
      hipLaunchKernelGGL(wrapr_refill_kernel, dim3((B * kBlock + 255) / 256), dim3(256), 0, st, b->d_wrap, b->wave.d_out, B, d_flags);
    }
    if (ok) {
      hipLaunchKernelGGL(wrapr_out_kernel, dim3(B), dim3(256), 0, st, b->d_wrap_inner, kInnerStride, b->d_wrap, b->wrap_gains.d + B, r.d_taps, d_rs, d_out, channels);
      ok = hip_ok(hipGetLastError(), "ragged wrapper launch") && r.rs.mark(e, st);
    }
    r.calls += 1;
    return ok;
  });
}

// ---- one stream's host side on its own: its rate, its restart, its wrapper blob (beatrice_batch.h; the blob: wrapper_blob.h) -------
// Where BeatriceBatch_ProcessBlocksRagged is allowed -- in order, one hop per step, after BeatriceBatch_ConfigureWrapperRates, no
// binding -- a stream's rate, clocks, gain clocks and StreamState can be set, restarted and moved without touching another stream.
// Everything that can be refused or can fail is done before anything is committed: the new class tables are built and uploaded into a
// buffer of their own first, the device state is written next, the host's bookkeeping last.
namespace {
static_assert(sizeof(wrapn::StreamState) == wblob::kStateBytes && wblob::kFifo == wrapn::kBlock, "wrapper_blob.h restates the wrapper's state block");
static_assert(offsetof(wrapn::StreamState, fifo) + sizeof(float) * wrapn::kBlock == sizeof(wrapn::StreamState), "bound_move.hip: the FIFO is the state's last member");
bool rag_settings_allowed(const BeatriceBatch* b) { return modes::allowed(Entry::ProcessBlocksRagged, flags_of(b)); }
// The batch's rate classes once every stream s runs at want[s]: the old classes still in use keep their order, the rates no stream has
// had yet (`fresh`, configured by the caller) follow; classes no stream uses any more are gone.  Unchanged set: nothing is built.
struct RagTables {
  bool rebuilt = false;
  std::vector<wrapn::RateClass> classes;
  std::vector<int> cls, taps_down_off, taps_up_off;
  DevBuf<float> d_taps;
};
bool rag_retable(const BeatriceBatch* b, const std::vector<double>& want, const std::vector<wrapn::RateClass>& fresh, RagTables& t) {
  const BeatriceBatch::RaggedWrap& r = b->rw;
  const int B = b->B;
  auto used = [&](double rate) { for (int s = 0; s < B; ++s) if (want[s] == rate) return true; return false; };
  for (const wrapn::RateClass& p : r.classes) if (used(p.rate)) t.classes.push_back(p);
  t.rebuilt = t.classes.size() != r.classes.size();
  for (const wrapn::RateClass& p : fresh) {
    bool have = false;
    for (const wrapn::RateClass& q : t.classes) have = have || q.rate == p.rate;
    if (!have && used(p.rate)) { t.classes.push_back(p); t.rebuilt = true; }
  }
  t.cls.assign(B, -1);
  for (int s = 0; s < B; ++s)
    for (size_t i = 0; i < t.classes.size(); ++i) if (t.classes[i].rate == want[s]) { t.cls[s] = (int)i; break; }
  for (int s = 0; s < B; ++s) if (t.cls[s] < 0) return false;   // (cannot be: every rate wanted is an old class's or a fresh one's)
  if (!t.rebuilt) return true;
  std::vector<float> taps;
  for (const wrapn::RateClass& p : t.classes) {
    t.taps_down_off.push_back((int)taps.size()); taps.insert(taps.end(), p.taps_down.begin(), p.taps_down.end());
    t.taps_up_off.push_back((int)taps.size()); taps.insert(taps.end(), p.taps_up.begin(), p.taps_up.end());
  }
  return t.d_taps.alloc(taps.size(), "ragged taps", false) &&
         hip_ok(hipMemcpy(t.d_taps, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice), "ragged taps up");
}
// (after a drain: no launch reads the old table any more)
void rag_commit(BeatriceBatch* b, RagTables& t) {
  BeatriceBatch::RaggedWrap& r = b->rw;
  if (t.rebuilt) {
    r.d_taps = std::move(t.d_taps); r.taps_down_off = std::move(t.taps_down_off); r.taps_up_off = std::move(t.taps_up_off);
    r.classes = std::move(t.classes);
  }
  r.cls = std::move(t.cls);
}
// the class of `rate` among the batch's and those configured so far for this call; a rate none has had is configured (nullptr: refused)
const wrapn::RateClass* rag_class_of(const BeatriceBatch* b, double rate, std::vector<wrapn::RateClass>& fresh) {
  if (!std::isfinite(rate)) return nullptr;
  for (const wrapn::RateClass& p : b->rw.classes) if (p.rate == rate) return &p;
  for (const wrapn::RateClass& p : fresh) if (p.rate == rate) return &p;
  wrapn::RateClass p;
  if (!p.configure(rate)) return nullptr;
  fresh.push_back(p);
  return &fresh.back();
}
// reference SetSampleRate for ONE stream (processor_core_2.cc:421-429): resampler pair and FIFO start over at `rate`, the gains keep
// their state and ramp at the new rate from the next block on
int rag_restart(BeatriceBatch* b, int s, double rate) {
  BeatriceBatch::RaggedWrap& r = b->rw;
  std::vector<wrapn::RateClass> fresh;
  if (!rag_class_of(b, rate, fresh)) return -1;
  std::vector<double> want = b->rw.rates();
  want[s] = rate;
  RagTables t;
  if (!rag_retable(b, want, fresh, t) || !sync_all(b)) return -2;
  if (!hip_ok(hipMemsetAsync(b->d_wrap + s, 0, sizeof(wrapn::StreamState), b->stream), "stream wrapper state0") ||
      !hip_ok(hipStreamSynchronize(b->stream), "stream wrapper sync"))
    return -2;
  rag_commit(b, t);
  r.clk[s] = r.classes[r.cls[s]].start();
  b->wrap_gains_constant = false;
  return 0;
}
// the piece table of the wrapper blobs (once per batch) and staging for min(n, 16) of them
bool wblob_prepare(BeatriceBatch* b, int n) {
  BeatriceBatch::RaggedWrap& r = b->rw;
  if (!r.d_blob_piece) {
    const unsigned words = (unsigned)(sizeof(wrapn::StreamState) / sizeof(float));
    const BlobPiece piece{reinterpret_cast<float*>(b->d_wrap.get()), words, words, 1, (unsigned long long)(wblob::kOffState / sizeof(float))};
    DevBuf<BlobPiece> d_piece;
    if (!d_piece.alloc(1, "wrapper blob piece", false) || !hip_ok(hipMemcpy(d_piece, &piece, sizeof(piece), hipMemcpyHostToDevice), "wrapper blob piece up")) return false;
    r.d_blob_piece = std::move(d_piece);
  }
  const int want = std::min(n, sblob::kMaxRound);
  if (r.blob_cap < want) {
    PinnedBuf<unsigned char> h_stage;
    DevBuf<unsigned char> d_stage;
    if (!h_stage.alloc((size_t)want * wblob::kBlobBytes, "wrapper blob staging", false) || !d_stage.alloc((size_t)want * wblob::kBlobBytes, "wrapper blob staging")) return false;
    r.h_blob_stage = std::move(h_stage); r.d_blob_stage = std::move(d_stage); r.blob_cap = want;
  }
  return true;
}
}  // namespace

int BeatriceBatch_SetStreamRate(BeatriceBatch* b, int stream, double host_sample_rate) {
  BATCH_OPEN(b);
  if (!rag_settings_allowed(b) || stream < 0 || stream >= b->B) return -1;
  if (b->rw.rate(stream) == host_sample_rate) return 0;   // (the reference's SetSampleRate: an equal rate is no call at all)
  return rag_restart(b, stream, host_sample_rate);
}
int BeatriceBatch_RestartStreamWrapper(BeatriceBatch* b, int stream) {
  BATCH_OPEN(b);
  if (!rag_settings_allowed(b) || stream < 0 || stream >= b->B) return -1;
  return rag_restart(b, stream, b->rw.rate(stream));
}
double BeatriceBatch_StreamRate(const BeatriceBatch* b, int stream) {
  if (!b || !b->ok || !rag_settings_allowed(b) || stream < 0 || stream >= b->B) return 0.0;
  return b->rw.rate(stream);
}
size_t BeatriceBatch_WrapperBlobBytes(const BeatriceBatch* b) { return b && b->ok && rag_settings_allowed(b) ? wblob::kBlobBytes : 0; }

int BeatriceBatch_ExportStreamWrappers(BeatriceBatch* b, int n, const int* streams, void* blobs) {
  BATCH_OPEN(b);
  if (!rag_settings_allowed(b) || !blob_streams_ok(b, n, streams) || !blobs) return -1;
  if (!wblob_prepare(b, n) || !sync_all(b)) return -2;
  BeatriceBatch::RaggedWrap& r = b->rw;
  unsigned char* out = static_cast<unsigned char*>(blobs);
  for (int at = 0; at < n; at += r.blob_cap) {
    BlobRound round{};
    round.n = std::min(r.blob_cap, n - at);
    for (int j = 0; j < round.n; ++j) round.streams[j] = streams[at + j];
    if (!stream_gather(r.d_blob_piece, 1, round, reinterpret_cast<float*>(r.d_blob_stage.get()), wblob::kBlobBytes / sizeof(float), b->stream) ||
        !hip_ok(hipMemcpyAsync(r.h_blob_stage, r.d_blob_stage, (size_t)round.n * wblob::kBlobBytes, hipMemcpyDeviceToHost, b->stream), "wrapper blobs down") ||
        !hip_ok(hipStreamSynchronize(b->stream), "wrapper gather"))
      return -2;
    for (int j = 0; j < round.n; ++j) {
      const int s = round.streams[j];
      unsigned char* blob = r.h_blob_stage + (size_t)j * wblob::kBlobBytes;
      const wrapn::Clocks& c = r.clk[s];
      wblob::write_header(r.rate(s), c.phase_down, c.phase_up, c.fill, b->gain_in[s].target_db, b->gain_in[s].now_db,
                          b->gain_out[s].target_db, b->gain_out[s].now_db, blob);
      std::memcpy(out + (size_t)(at + j) * wblob::kBlobBytes, blob, wblob::kBlobBytes);
    }
  }
  return 0;
}

int BeatriceBatch_ImportStreamWrappers(BeatriceBatch* b, int n, const int* streams, const void* blobs) {
  BATCH_OPEN(b);
  if (!rag_settings_allowed(b) || !blob_streams_ok(b, n, streams) || !blobs) return -1;
  BeatriceBatch::RaggedWrap& r = b->rw;
  const unsigned char* in = static_cast<const unsigned char*>(blobs);
  std::vector<wblob::Header> taken(n);
  std::vector<wrapn::RateClass> fresh;
  std::vector<double> want = b->rw.rates();
  for (int i = 0; i < n; ++i) {   // every blob is looked at before anything is drained, built, uploaded or written
    const unsigned char* blob = in + (size_t)i * wblob::kBlobBytes;
    double rate = 0.0;
    if (wblob::read_rate(blob, wblob::kBlobBytes, &rate) != wblob::kOk) return -1;
    const wrapn::RateClass* p = rag_class_of(b, rate, fresh);   // (the rate through RateClass::configure: its hi bounds the clocks)
    if (!p || wblob::validate(blob, wblob::kBlobBytes, p->hi, &taken[i]) != wblob::kOk) return -1;
    want[streams[i]] = rate;
  }
  RagTables t;
  if (!rag_retable(b, want, fresh, t) || !wblob_prepare(b, n) || !sync_all(b)) return -2;
  for (int at = 0; at < n; at += r.blob_cap) {
    BlobRound round{};
    round.n = std::min(r.blob_cap, n - at);
    for (int j = 0; j < round.n; ++j) round.streams[j] = streams[at + j];
    std::memcpy(r.h_blob_stage, in + (size_t)at * wblob::kBlobBytes, (size_t)round.n * wblob::kBlobBytes);
    if (!hip_ok(hipMemcpyAsync(r.d_blob_stage, r.h_blob_stage, (size_t)round.n * wblob::kBlobBytes, hipMemcpyHostToDevice, b->stream), "wrapper blobs up") ||
        !stream_scatter(r.d_blob_piece, 1, round, reinterpret_cast<const float*>(r.d_blob_stage.get()), wblob::kBlobBytes / sizeof(float), b->stream) ||
        !hip_ok(hipStreamSynchronize(b->stream), "wrapper scatter"))
      return -2;
  }
  rag_commit(b, t);
  for (int i = 0; i < n; ++i) {
    const int s = streams[i];
    const wblob::Header& h = taken[i];
    r.clk[s] = wrapn::Clocks{h.phase_down, h.phase_up, h.fill};
    b->gain_in[s].target_db = h.in_target_db; b->gain_in[s].now_db = h.in_now_db;
    b->gain_out[s].target_db = h.out_target_db; b->gain_out[s].now_db = h.out_now_db;
  }
  b->wrap_gains_constant = false;
  return 0;
}

// ---- the same wrapper around the TICK pipeline (throughput form, resident blocks) ------------------------------------------------
// One call = one host-rate block per stream from slot `call mod n_slots` of d_in: gains and the first resampling direction, the
// 480-sample accumulation, a model hop into the tick pipeline every time it fills (one tick per hop, at least one tick per
// call so that a hop is out of the pipeline TickStages() - 1 calls after it went in); then the output half of the call made
// `delay` = TickStages() - 1 calls ago, into ITS slot of d_out.  Everything that is control is on the host, as in wrap_chunk.
// What both forms of the resident blocks bind, all or nothing: the ticks' resident 16 / 24 kHz slots and the gain ring of `nr` (the caller has set
// its delay, ring, H and io_slots, and allocated what only its form has), resident I/O on those slots, tick mode.  `nr` then becomes the batch's.
static bool rb_bind(BeatriceBatch* b, BeatriceBatch::ResidentBlocks& nr) {
  const size_t rows = (size_t)nr.io_slots * b->B * nr.H;
  const bool ok = nr.d_in16.alloc(rows * B_IN_HOP, "rb in16") && nr.d_out24.alloc(rows * B_OUT_HOP, "rb out24") &&
                  nr.gains.alloc(nr.ring, 2 * (size_t)b->B, "rb gains") && hip_ok(hipDeviceSynchronize(), "rb sync") &&
                  bind_io(b, nr.d_in16, nr.d_out24, nr.io_slots) == 0 && tick_enable(b, true) == 0;
  if (!ok) {
    (void)tick_enable(b, false);
    (void)bind_io(b, nullptr, nullptr, 0);
    return false;
  }
  b->rb = std::move(nr);
  return true;
}
// leaves either form of the resident blocks: the pipeline drained, tick mode off, the wrapper restarted at its rate(s).  A restart that
// fails is not swallowed: -2, the binding is gone, and the wrapper whose state could not be restarted is marked not configured -- its
// in-order entry points are refused until BeatriceBatch_ConfigureWrapper[Rates] succeeds (what a failed bind leaves, too)
static int rb_unbind(BeatriceBatch* b) {
  BeatriceBatch::ResidentBlocks& r = b->rb;
  if (!sync_all(b)) return -2;
  const int rc = tick_enable(b, false);
  if (rc) return rc;
  (void)bind_io(b, nullptr, nullptr, 0);
  const bool ragged = r.ragged;
  b->entries.filling_dropped(b->tk.last_feed_tick, b->tk.plan.count());   // (speaker_entry_plan.h: a step still filling ends with the binding)
  r = {};
  if (ragged) {
    b->silent.on = false;   // (the flags of the ragged steps were the binding's own)
    if (BeatriceBatch_ConfigureWrapperRates(b, b->rw.rates().data()) != 0) { b->rw.ready = false; return -2; }
  } else {
    // the wrapper restarts, as after a sample-rate change (the gains keep their state)
    if (BeatriceBatch_ConfigureWrapper(b, b->wrap.rate) != 0) { b->wrap.ready = false; return -2; }
  }
  return 0;
}
// Calls after which a call's output block is out.  One hop per step: every call runs at least one tick, so TickStages() - 1 calls
// behind the call that fed its newest hop.  H hops per step: ticks run only when a step is full (an idle tick per call would carry a
// quarter-filled pipeline and cost what a full one does) -- the newest hop waits until up to H - 1 further hops have filled its step
// and TickStages() - 1 further steps have gone in behind it, each call bringing at least m_lo inner samples (the two clocks make a
// call's count vary by one).  -1: blocks too short to bound it (H > 1 only).
static int rb_delay(const BeatriceBatch* b, int n) {
  const int stages = b->tk.plan.count();
  if (b->H == 1) return stages - 1;
  const long long m_lo = (long long)std::floor(n * 48000.0 / b->wrap.rate) - 1;
  if (m_lo < 1) return -1;
  const long long hops = (long long)(b->H - 1) + (long long)(stages - 1) * b->H;
  return (int)((hops * wrapn::kBlock + m_lo - 1) / m_lo) + 1;   // (+ 1: the output half rides in the launch of the call after)
}
// synthetic: a call BeatriceBatch_FlushResidentBlocks makes up -- a block of zeros that is no call of the caller's: it reads no slot, owes no
// output block and does not count (the call counter stands), but moves the wrapper and fires hops as a block of silence would
static bool rb_step(BeatriceBatch* b, const bool synthetic) {
  using namespace wrapn;
  BeatriceBatch::ResidentBlocks& r = b->rb;
  const int B = b->B, n = r.n, H = r.H;
  hipStream_t st = b->stream;
  const RateClass& w = b->wrap;
  const long long call = r.calls;
  const int ge = (int)(call % r.ring);
  // this call's gain segments: input half now, output half when its job runs.  The kernels read them where they are written (pinned
  // memory): the entry is free again once the output half that read it last has run
  GainSeg* seg = r.gains.claim(ge);
  if (!seg) return false;
  ClockPlan p;
  if (!plan_clocks(w, b->wrap_clk, n, p)) return false;   // (a plan that does not fit: no clock has moved)
  for (int s = 0; s < B; ++s) { seg[s] = b->gain_in[s].advance(n, w.rate); seg[B + s] = b->gain_out[s].advance(n, w.rate); }
  const size_t nt = w.taps_down.size();
  WrapCallArgs a{};
  a.din = p.din;
  a.src = synthetic ? r.d_zero.get() : r.d_in + (size_t)(call % r.n_slots) * B * r.channels * n;
  a.channels = r.channels; a.n = n; a.st = b->d_wrap; a.gain_in = seg; a.taps_in = b->d_wrap_taps + (a.din.decimate ? 0 : nt);
  a.inner = b->d_wrap_inner; a.stride = kInnerStride; a.in16 = r.d_in16; a.row16 = H * B_IN_HOP; a.B = B; a.H = H;
  // the 480-sample accumulation; a model hop every time it fills (the per-stream FIFO array holds it), into its place: hop
  // hops_fired % H of the step that goes in next -- the steps this call fills take the resident slots from io_host on
  p.cut.put(a);
  int steps = 0, slot = b->io_host;
  const long long hops_before = r.hops_fired;
  for (int c = 0; c < a.n_chunks; ++c) {
    a.in16_off[c] = (long long)((size_t)slot * B * H + (size_t)(r.hops_fired % H)) * B_IN_HOP;
    if (!a.fires[c]) continue;
    ++r.hops_fired;
    if (r.hops_fired % H == 0) { ++steps; slot = (slot + 1) % r.io_slots; }   // the step is full
  }
  // several hops per step: the output half of the oldest call that is due rides in this launch (its hops left the ticks with the
  // previous call at the latest: `delay` counts this call)
  const BeatriceBatch::ResidentBlocks::Job* due = nullptr;
  if (H > 1 && !r.jobs.empty() && r.jobs.front().call + r.delay <= call && r.jobs.front().last_hop() < r.hops_done) due = &r.jobs.front();
  int due_ge = -1;
  if (due) {
    due_ge = (int)(due->call % r.ring);
    a.n_post = B; a.out24 = r.d_out24; a.io_slots = r.io_slots; a.t0 = due->t0; a.gain_out = r.gains.host(due_ge) + B;
    a.taps_out = b->d_wrap_taps + (due->dout.decimate ? 0 : nt); a.dout = due->dout;
    a.out = r.d_out + (size_t)(due->call % r.n_slots) * B * r.channels * n;
  }
  hipLaunchKernelGGL(wrap_call_kernel, dim3(B + a.n_post), dim3(256), 0, st, a);
  if (due) {
    if (!r.gains.mark(due_ge, st)) return false;
    r.jobs.pop_front();
  }
  // (never more than one call comes due per call under the bind-time bound; should the queue have fallen behind, the rest follow here)
  while (H > 1 && !r.jobs.empty() && r.jobs.front().call + r.delay <= call && r.jobs.front().last_hop() < r.hops_done) {
    if (!rb_post(b, r.jobs.front())) return false;
    r.jobs.pop_front();
  }
  // (speaker_entry_plan.h: a step that an earlier call left filling stays open until its feed is over; a step this call fills alone never is)
  for (int i = 0; i < steps; ++i) {
    r.step_open = sentry::step_open_during_feed(hops_before, H, i);
    if (!tick_run(b, true)) return false;   // the full steps: into the pipeline
  }
  r.step_open = sentry::step_open_after_call(r.hops_fired, H);
  if (steps == 0 && H == 1 && !tick_run(b, false)) return false;          // one hop per step: the pipeline advances with every call
  r.hops_done = r.hops_fed();
  if (!synthetic) r.jobs.push_back(BeatriceBatch::ResidentBlocks::Job{call, r.t48, p.dout});
  r.t48 += p.din.n_out;
  if (!synthetic) r.calls = call + 1;
  bool ok = hip_ok(hipGetLastError(), "wrapper launch");
  // one hop per step: after `delay` calls a call's hops are out, its output half runs behind this call's tick
  while (ok && H == 1 && !r.jobs.empty() && r.jobs.front().call + r.delay <= call) {
    ok = rb_post(b, r.jobs.front());
    r.jobs.pop_front();
  }
  b->inflight = true;
  return ok;
}
// d_in / d_out: [n_slots][B][channels][n] planar blocks at the configured host rate (BeatriceBatch_ConfigureWrapper first).
// Call k (BeatriceBatch_ProcessBlocksDevice(b, NULL, NULL, channels, n)) reads slot k mod n_slots; its output block is in the
// same slot of d_out BeatriceBatch_ResidentBlocksDelay() calls later (or after BeatriceBatch_Synchronize).  Same samples as
// the in-order BeatriceBatch_ProcessBlocksDevice.  n_slots > delay + 1.  NULL pointers unbind.
int BeatriceBatch_BindResidentBlocks(BeatriceBatch* b, const float* d_in, float* d_out, int channels, int n, int n_slots) {
  BATCH_OPEN(b);
  const bool bind = d_in || d_out;
  if (bind) BATCH_GATE(b, Entry::BindResidentBlocks_bind);
  BeatriceBatch::ResidentBlocks& r = b->rb;
  if (r.on) { const int rc = rb_unbind(b); if (rc) return rc; }
  if (!bind) return 0;
  BATCH_GATE(b, Entry::BindResidentBlocks_bind);   // (again: the mode the batch is in now that it has left G / P)
  const int stages = b->tk.plan.count();
  const int H = b->H;
  if (!d_in || !d_out || channels < 1 || channels > 2 || n < 1 || n > wrapn::longest_block(b->wrap.rate)) return -1;
  const int delay = rb_delay(b, n);
  if (delay < 0 || n_slots < delay + 2) return -1;
  // binding restarts the resampler pair and the FIFO (their in-order form keeps processed samples in the FIFO, this one does not)
  if (BeatriceBatch_ConfigureWrapper(b, b->wrap.rate) != 0) { b->wrap.ready = false; return -2; }
  // model hops a call can fire: ceil(inner samples / 480) + 1; a hop's resident output is read until `delay` calls after the
  // call in which the NEXT hop fired.  With H hops per step a slot holds a step: the hops of (delay + 2) calls are that many / H steps.
  const int hops_per_call = wrapn::most_hops(n, b->wrap.rate);
  BeatriceBatch::ResidentBlocks nr;
  nr.delay = delay;
  nr.ring = nr.delay + 3;
  nr.H = H;
  nr.io_slots = std::max(stages + 1, H == 1 ? (nr.delay + 2) * hops_per_call + 2 : ((nr.delay + 2) * hops_per_call + H - 1) / H + 3);
  if (nr.io_slots > stepc::kImmediateMaxSlot + 1) return -1;   // (tick mode's limit on resident slots)
  if (!rb_bind(b, nr)) return -2;
  r.d_in = d_in; r.d_out = d_out; r.channels = channels; r.n = n; r.n_slots = n_slots; r.on = true;
  return 0;
}
// ---- the wrapper with clocks PER STREAM around the tick pipeline (BeatriceBatch_ConfigureWrapperRates, then
// BeatriceBatch_BindResidentBlocksRagged / BeatriceBatch_ProcessBlocksRaggedDevice): what the reference gives every plugin instance
// (src/common/resample.h:401-438), in the throughput form.  A call = for every stream a block of n_samples[s] host samples at ITS
// rate from its cell of slot `call mod n_slots`; a stream fires a model hop when ITS 480-sample FIFO fills, and the step that goes
// into the ticks then carries the streams that fired -- the others sit it out with their own step counters (the tick launch's ragged
// steps, batch_tick.hip.h), so a stream's hops ride in steps of their own and slot_map remembers which.  Output half `delay` =
// TickStages() - 1 calls later, from the records the call left on the device.
static int rbr_step(BeatriceBatch* b, const int* n_samples) {
  using namespace wrapn;
  BeatriceBatch::ResidentBlocks& r = b->rb;
  BeatriceBatch::RaggedWrap& rw = b->rw;
  const int B = b->B;
  hipStream_t st = b->stream;
  for (int s = 0; s < B; ++s) if (n_samples[s] < 0 || n_samples[s] > std::min(r.max_samples, longest_block(rw.rate(s)))) return -1;
  const long long call = r.calls;
  const int ge = (int)(call % r.ring);
  // (records and gain segments are read by the kernels where they are written, pinned memory: the ring entry is free again once the
  //  output half that read it last has run)
  GainSeg* seg = r.gains.claim(ge);
  if (!seg) return -2;
  RagStream* rs = r.h_rs + (size_t)ge * B;
  // all or nothing, as BeatriceBatch_ProcessBlocksRagged: the clocks move when every stream's plan stands
  rw.next.begin(rw.clk, b->gain_in, b->gain_out);
  int max_chunks = 0;
  for (int s = 0; s < B; ++s) {
    RagStream& q = rs[s];
    q = RagStream{};
    const int n = n_samples[s];
    q.io_off = (long long)s * r.cell; q.n = n;
    q.active = n > 0 ? 1 : 0;
    q.hop0 = r.hops_s[s]; q.t0 = r.t48_s[s]; q.hop_base = r.hop_base_s[s];
    if (!q.active) { seg[s] = GainSeg{1.0, 1.0, 1.0}; seg[B + s] = GainSeg{1.0, 1.0, 1.0}; continue; }
    q.restart = r.restart_s[s];   // (a restart travels with the stream's first block behind it: both halves of this call)
    if (!rag_plan(b, s, n, q, seg)) return -2;
    max_chunks = std::max(max_chunks, q.n_chunks);
  }
  rw.next.commit(rw.clk, b->gain_in, b->gain_out);
  bool fire_at[kMaxChunks] = {};   // piece c: does any stream fire in it?
  for (int s = 0; s < B; ++s) {   // (the plan stands: the streams' sample and hop counts move)
    if (!rs[s].active) continue;
    r.restart_s[s] = 0;
    r.marks.active(s, call);   // (bound_move_plan.h rule (b): the output half of this call is owed for the stream)
    r.t48_s[s] += rs[s].din.n_out;
    for (int c = 0; c < rs[s].n_chunks; ++c) { r.hops_s[s] += rs[s].fires[c]; fire_at[c] = fire_at[c] || rs[s].fires[c]; }
  }
  // one launch for every stream's input half and FIFO pieces; piece c belongs to the c-th step this call feeds (if any stream fires in
  // it), which takes the next resident slot
  WraprCallArgs a{};
  a.in = r.d_in + (size_t)(call % r.n_slots) * B * r.cell; a.channels = r.channels; a.st = b->d_wrap; a.gain = seg; a.taps_all = rw.d_taps;
  a.rs = rs; a.inner = b->d_wrap_inner; a.stride = kInnerStride; a.in16 = r.d_in16; a.B = B; a.slot_map = r.d_map; a.map_ring = r.map_ring;
  for (int ci = 0, slot = b->io_host; ci < max_chunks; ++ci) {
    a.slot[ci] = slot;
    if (fire_at[ci]) slot = (slot + 1) % r.io_slots;
  }
  hipLaunchKernelGGL(wrapr_call_kernel, dim3(B), dim3(256), 0, st, a);
  BeatriceBatch::SilentRule& sr = b->silent;
  int ticks = 0;
  for (int ci = 0; ci < max_chunks; ++ci) {
    if (!fire_at[ci]) continue;
    sr.any_next = rag_fires(b, rs, ci).any_out;   // (tick_run: the flagged streams sit this step out, and clears the flags)
    if (!tick_run(b, true)) return -2;
    std::fill(sr.next.begin(), sr.next.end(), 0);
    sr.any_next = false;
    ++ticks;
  }
  if (ticks == 0 && !tick_run(b, false)) return -2;   // the pipeline advances with every call
  r.jobs.push_back(BeatriceBatch::ResidentBlocks::Job{call, 0, Dir{}});
  r.calls = call + 1;
  bool ok = true;
  while (ok && !r.jobs.empty() && r.jobs.front().call + r.delay <= call) {
    ok = rb_post(b, r.jobs.front());
    r.jobs.pop_front();
  }
  b->inflight = true;
  return ok ? 0 : -2;
}
int BeatriceBatch_ProcessBlocksRaggedDevice(BeatriceBatch* b, const int* n_samples) {
  BATCH_ENTER(b, Entry::ProcessBlocksRaggedDevice);
  if (!n_samples) return -1;
  return rbr_step(b, n_samples);
}
// d_in / d_out: [n_slots][B][channels * max_samples]: stream s's block of a call, planar [channels][n_samples[s]], at the start of its cell
int BeatriceBatch_BindResidentBlocksRagged(BeatriceBatch* b, const float* d_in, float* d_out, int channels, int max_samples, int n_slots) {
  BATCH_OPEN(b);
  const bool bind = d_in || d_out;
  if (bind) BATCH_GATE(b, Entry::BindResidentBlocksRagged_bind);
  BeatriceBatch::ResidentBlocks& r = b->rb;
  if (r.on) { const int rc = rb_unbind(b); if (rc) return rc; }
  if (!bind) return 0;
  BATCH_GATE(b, Entry::BindResidentBlocksRagged_bind);   // (again: the mode the batch is in now that it has left G / P)
  const int stages = b->tk.plan.count();
  if (!d_in || !d_out || channels < 1 || channels > 2 || max_samples < 1 || n_slots < stages + 1) return -1;
  const int B = b->B;
  // binding restarts every stream's resampler pair and FIFO (their in-order form keeps processed samples in the FIFO, this one does not)
  const std::vector<double> rates = b->rw.rates();
  if (BeatriceBatch_ConfigureWrapperRates(b, rates.data()) != 0) { b->rw.ready = false; return -2; }
  // steps a call can feed = the most hops one stream can fire in it; a hop's resident output is read until `delay` calls after the call
  // in which the stream's NEXT hop fired
  int hops_per_call = 1;
  for (int s = 0; s < B; ++s) hops_per_call = std::max(hops_per_call, wrapn::most_hops(std::min(max_samples, wrapn::longest_block(rates[s])), rates[s]));
  BeatriceBatch::ResidentBlocks nr;
  nr.delay = stages - 1;
  nr.ring = nr.delay + 3;
  nr.H = 1;
  nr.io_slots = std::max(stages + 1, (nr.delay + 2) * hops_per_call + 2);
  if (nr.io_slots > stepc::kImmediateMaxSlot + 1) return -1;
  nr.map_ring = nr.io_slots;
  if (!nr.h_rs.alloc((size_t)nr.ring * B, "rb records host") || !nr.d_map.alloc((size_t)B * nr.map_ring, "rb slot map") || !rb_bind(b, nr)) return -2;
  b->silent.next.assign(B, 0);   // the ragged steps' flags (tick_run): set per tick by rbr_step, not by the caller
  b->silent.any_next = false;
  b->silent.on = true;
  r.d_in = d_in; r.d_out = d_out; r.channels = channels; r.max_samples = max_samples; r.cell = channels * max_samples; r.n = 0;
  r.n_slots = n_slots; r.ragged = true;
  r.t48_s.assign(B, 0);
  r.hops_s.assign(B, 0);
  r.hop_base_s.assign(B, 0);
  r.restart_s.assign(B, 0);
  r.marks.start(B);
  r.hops_cap = hops_per_call;
  // the classes as BeatriceBatch_ConfigureWrapperRates has just laid them out: from here on they keep index and place (wrapper_turnover_plan.h)
  BeatriceBatch::RaggedWrap& rw = b->rw;
  rw.arena.start(B, r.delay);
  for (size_t c = 0; c < rw.classes.size(); ++c)
    rw.arena.add_initial(rw.classes[c].rate, (int)rw.classes[c].taps_down.size(), (int)rw.classes[c].taps_up.size(), (int)std::count(rw.cls.begin(), rw.cls.end(), (int)c));
  r.on = true;
  return 0;
}
// ---- a stream's rate, its restart and its slot's turn-over INSIDE that binding (beatrice_batch.h; the tap tables: wrapper_turnover_plan.h) -------
// Nothing drains, nothing is waited for, no tick runs: the host's clocks start over here, the device learns of it from the record of the
// stream's next block (rbr_step, wrapn::RagStream), and the calls that are owed finish on the old rate, taps and output history.  Everything
// that can be refused or can fail -- the rate, the room for its hops, the table's place, buffer and upload, the reset table -- comes before
// the first thing that is committed.
namespace {
bool rbr_settings_allowed(const BeatriceBatch* b) { return modes::allowed(Entry::ProcessBlocksRaggedDevice, flags_of(b)); }
// a rate no held class has: its class gets a place in the tap buffer and goes up; its index (-2: no room, or HIP failed -- nothing is changed)
int rbr_place(BeatriceBatch* b, wrapn::RateClass& fresh) {
  BeatriceBatch::RaggedWrap& rw = b->rw;
  wturn::TapArena& ar = rw.arena;
  const double rate = fresh.rate;
  const int n_down = (int)fresh.taps_down.size(), n_up = (int)fresh.taps_up.size(), floats = n_down + n_up;
  ar.reap(b->rb.calls);
  const wturn::Place p = ar.plan(floats);
  if (p.index < 0) return -2;
  auto put = [](float* h, int off, const wrapn::RateClass& k) {
    std::memcpy(h + off, k.taps_down.data(), sizeof(float) * k.taps_down.size());
    std::memcpy(h + off + k.taps_down.size(), k.taps_up.data(), sizeof(float) * k.taps_up.size());
  };
  if (p.grows || !rw.h_taps) {
    // a longer buffer (or the first staging): every held class at its old offset, the new one behind them, one copy; the launches to
    // come get this buffer, the ones enqueued keep theirs
    DevBuf<float> d_taps;
    PinnedBuf<float> h_taps;
    if ((p.grows && !d_taps.alloc((size_t)p.capacity, "ragged taps", false)) || !h_taps.alloc((size_t)p.capacity, "ragged taps staging")) return -2;
    int end = p.off + floats;
    for (size_t i = 0; i < ar.slots.size(); ++i) {
      if (!ar.slots[i].held) continue;
      put(h_taps, ar.slots[i].off, rw.classes[i]);
      end = std::max(end, ar.slots[i].off + ar.slots[i].floats);
    }
    put(h_taps, p.off, fresh);
    const bool ok = p.grows ? hip_ok(hipMemcpyAsync(d_taps, h_taps, sizeof(float) * (size_t)end, hipMemcpyHostToDevice, b->stream), "ragged taps up")
                            : hip_ok(hipMemcpyAsync(rw.d_taps + p.off, h_taps + p.off, sizeof(float) * (size_t)floats, hipMemcpyHostToDevice, b->stream), "ragged class up");
    if (!ok) { (void)hipStreamSynchronize(b->stream); return -2; }   // (the staging is about to go: nothing may still read it)
    if (p.grows) { rw.d_taps_outgrown.push_back(std::move(rw.d_taps)); rw.d_taps = std::move(d_taps); }
    if (rw.h_taps) rw.h_taps_outgrown.push_back(std::move(rw.h_taps));
    rw.h_taps = std::move(h_taps);
  } else {
    put(rw.h_taps, p.off, fresh);   // (a free place: no copy that matters is pending on these floats, rule 3)
    if (!hip_ok(hipMemcpyAsync(rw.d_taps + p.off, rw.h_taps + p.off, sizeof(float) * (size_t)floats, hipMemcpyHostToDevice, b->stream), "ragged class up")) return -2;
  }
  ar.commit(p, rate, n_down, n_up);
  const int c = p.index;
  if ((int)rw.classes.size() <= c) { rw.classes.resize(c + 1); rw.taps_down_off.resize(c + 1); rw.taps_up_off.resize(c + 1); }
  rw.classes[c] = std::move(fresh);
  rw.taps_down_off[c] = ar.slots[c].off_down(); rw.taps_up_off[c] = ar.slots[c].off_up();
  return c;
}
int rbr_restart(BeatriceBatch* b, int s, double rate, bool reset_model) {
  BeatriceBatch::ResidentBlocks& r = b->rb;
  BeatriceBatch::RaggedWrap& rw = b->rw;
  if (!std::isfinite(rate)) return -1;
  const int old = rw.cls[s];
  int c = rate == rw.rate(s) ? old : rw.arena.find(rate);
  wrapn::RateClass fresh;
  if (c < 0 && !fresh.configure(rate)) return -1;   // (what BeatriceBatch_SetStreamRate refuses)
  if (wrapn::most_hops(std::min(r.max_samples, wrapn::longest_block(rate)), rate) > r.hops_cap) return -1;   // (the slot ring and slot map: sized at bind time)
  if (reset_model && !tick_reset_prepare(b)) return -2;
  if (c < 0) c = rbr_place(b, fresh);
  if (c < 0) return c;
  if (c != old) {   // (nothing below fails)
    rw.arena.join(c, r.calls);
    rw.arena.leave(old, r.calls);
    rw.cls[s] = c;
  }
  rw.clk[s] = rw.classes[c].start();
  r.t48_s[s] = 0;
  r.hop_base_s[s] = r.hops_s[s];
  r.restart_s[s] = 1;
  if (!reset_model) return 0;
  // the slot goes to a new caller: what BeatriceBatch_ResetStreamInFlight does in plain tick mode -- the stream's next present step is
  // the first of a new stream (tick_run carries the reset to it, also past steps it sits out), all four key/value blocks installed there
  b->tk.reset_pending[s] = 1;
  b->tk.any_reset_pending = true;
  return BeatriceBatch_FlushSpeaker(b, s);
}
}  // namespace
int BeatriceBatch_SetStreamRateInFlight(BeatriceBatch* b, int stream, double host_sample_rate) {
  BATCH_OPEN(b);
  if (!rbr_settings_allowed(b) || stream < 0 || stream >= b->B) return -1;
  if (b->rw.rate(stream) == host_sample_rate) return 0;   // (the reference's SetSampleRate: an equal rate is no call at all)
  return rbr_restart(b, stream, host_sample_rate, false);
}
int BeatriceBatch_RestartStreamInFlight(BeatriceBatch* b, int stream, double host_sample_rate, int reset_model) {
  BATCH_OPEN(b);
  if (!rbr_settings_allowed(b) || stream < 0 || stream >= b->B) return -1;
  return rbr_restart(b, stream, host_sample_rate == 0.0 ? b->rw.rate(stream) : host_sample_rate, reset_model != 0);
}
double BeatriceBatch_BoundStreamRate(const BeatriceBatch* b, int stream) {
  if (!b || !b->ok || !rbr_settings_allowed(b) || stream < 0 || stream >= b->B) return 0.0;
  return b->rw.rate(stream);
}
// ---- a bound stream from one such binding into another, or into the two blobs and back, nothing drained (beatrice_batch.h; every
// decision: bound_move_plan.h; the kernels: bound_move.hip) ------------------------------------------------------------------------
// The streams named are at rest by both rules, so the launches enqueued on the batch's stream from here on leave their wrapper state, their
// slot-map entries and their cells of the resident slots alone until they are fed again.  The model rings go the way of the tick-mode
// calls (move_rings_fenced / export_rounds / import_rounds_in_flight), each stream turned at its own counter; the wrapper state, the hop
// the stream carries and the destination's slot-map entry by one more launch per round of 16; rate, clocks, gain clocks and the 48 kHz
// sample count from host to host.  No tick is launched, no output half runs, nothing is waited for but an export's own copy.
namespace {
struct BoundSideOf : bmove::Side {
  BoundSideOf(const BeatriceBatch* b, int n_, const int* streams_, bool pointers_ok_) {
    bound_ragged = rbr_settings_allowed(b);
    B = b->B; n = n_; streams = streams_; pointers_ok = pointers_ok_;
  }
};
static bmove::Rest bound_rest(const BeatriceBatch* b, bool is_source) {
  const tick::State& k = b->tk;
  bmove::Rest r;
  r.seen = &b->mv.seen; r.ticks = k.tick; r.stages = k.plan.count(); r.marks = &b->rb.marks;
  r.oldest_owed = b->rb.jobs.empty() ? b->rb.calls : b->rb.jobs.front().call;
  if (is_source) {   // (a destination's pending reset or restart is cancelled, not refused)
    if (k.any_reset_pending && (int)k.reset_pending.size() == b->B) r.reset_pending = k.reset_pending.data();
    r.restart_pending = b->rb.restart_s.data();
  }
  return r;
}
static BoundSide bound_side(BeatriceBatch* b) {
  return BoundSide{reinterpret_cast<float*>(b->d_wrap.get()), b->rb.d_out24.get(), b->rb.d_map.get(), b->B, b->rb.io_slots, b->rb.map_ring};
}
static bmove::Item bound_source_item(const BeatriceBatch* b, int s) {
  return bmove::source_item(s, b->rb.hops_s[s], b->rb.t48_s[s], b->rw.clk[s].fill, b->rb.map_ring);
}
static bmove::Item bound_dest_item(const BeatriceBatch* b, int t, int fill) {
  return bmove::dest_item(t, b->rb.hops_s[t], fill, b->io_host, b->rb.io_slots, b->rb.map_ring);
}
// a stream's host side as it travels
struct BoundTaken { double rate; wrapn::Clocks clk; wrapn::GainClock gain_in, gain_out; long long t48; };
bool bound_rates_fit(const BeatriceBatch* b, const std::vector<BoundTaken>& w) {
  for (const BoundTaken& t : w) if (!bmove::rate_fits(t.rate, b->rb.max_samples, b->rb.hops_cap)) return false;
  return true;
}
// The destination acquires every stream's class as BeatriceBatch_SetStreamRateInFlight does (a rate no held class has is placed and goes
// up: it may allocate) and joins it at once, so that the next placement's reap keeps it; the streams leave their old classes in
// bound_commit.  -2: nothing is joined any more, no stream's class has changed.
int bound_acquire(BeatriceBatch* b, const std::vector<BoundTaken>& w, std::vector<int>* cls) {
  BeatriceBatch::RaggedWrap& rw = b->rw;
  cls->assign(w.size(), -1);
  for (size_t i = 0; i < w.size(); ++i) {
    int c = rw.arena.find(w[i].rate);
    if (c < 0) {
      wrapn::RateClass fresh;
      c = fresh.configure(w[i].rate) ? rbr_place(b, fresh) : -2;   // (cannot be refused here: bound_rates_fit has configured it)
    }
    if (c < 0) {
      for (size_t j = 0; j < i; ++j) rw.arena.leave((*cls)[j], b->rb.calls);
      return -2;
    }
    rw.arena.join(c, b->rb.calls);
    (*cls)[i] = c;
  }
  return 0;
}
// the host's bookkeeping, last (nothing here fails)
void bound_commit(BeatriceBatch* b, int n, const int* streams, const std::vector<BoundTaken>& w, const std::vector<int>& cls) {
  BeatriceBatch::ResidentBlocks& r = b->rb;
  BeatriceBatch::RaggedWrap& rw = b->rw;
  for (int i = 0; i < n; ++i) {
    const int t = streams[i];
    rw.arena.leave(rw.cls[t], r.calls);
    rw.cls[t] = cls[i];
    rw.clk[t] = w[i].clk;
    b->gain_in[t] = w[i].gain_in; b->gain_out[t] = w[i].gain_out;
    r.hop_base_s[t] = bmove::hop_base(r.hops_s[t], w[i].t48, r.map_ring);
    r.t48_s[t] = w[i].t48;
    r.restart_s[t] = 0;   // (a restart still waiting for the slot's next block: the stream that arrives replaces what it would start over)
  }
}
}  // namespace

int BeatriceBatch_BoundStreamQuiescent(const BeatriceBatch* b, int stream) {
  if (!b || !b->ok || !rbr_settings_allowed(b) || stream < 0 || stream >= b->B) return -1;
  return bmove::quiescent(bound_rest(b, false), stream) ? 1 : 0;
}
size_t BeatriceBatch_BoundWrapperBlobBytes(const BeatriceBatch* b) { return b && b->ok && rbr_settings_allowed(b) ? wblob::kBlobBytes : 0; }

int BeatriceBatch_MoveBoundStreamsInFlight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams,
                                           const int* entry_map, int n_map) {
  if (!src || !dst || src == dst) return -1;
  if (!src->ok || !dst->ok) return -2;
  if (src->device != dst->device) return -1;
  const DeviceScope dev_(dst->device);
  const bool map_ok = n_map >= 0 && (entry_map == nullptr) == (n_map == 0);
  const BoundSideOf from(src, n, src_streams, map_ok), to(dst, n, dst_streams, map_ok);
  if (bmove::args(from) != bmove::kGo || bmove::args(to) != bmove::kGo || !sblob::same_layout(src->sb.layout, dst->sb.layout)) return -1;
  std::vector<Taken> taken;
  if (!move_take(src, dst, n, src_streams, entry_map, n_map, &taken)) return -1;
  std::vector<BoundTaken> w(n);
  for (int i = 0; i < n; ++i) {
    const int s = src_streams[i];
    w[i] = BoundTaken{src->rw.rate(s), src->rw.clk[s], src->gain_in[s], src->gain_out[s], src->rb.t48_s[s]};
  }
  if (!bound_rates_fit(dst, w)) return -1;
  if (bmove::at_rest(from, bound_rest(src, true)) != bmove::kGo || bmove::at_rest(to, bound_rest(dst, false)) != bmove::kGo) return -3;
  std::vector<int> cls;
  if (bound_acquire(dst, w, &cls) != 0) return -2;
  const int rc = move_rings_fenced(src, dst, n, src_streams, dst_streams, taken, [&](bool ok) {
    for (int at = 0; at < n && ok; at += sblob::kMaxRound) {
      BoundRound round{};
      round.n = std::min(sblob::kMaxRound, n - at);
      for (int j = 0; j < round.n; ++j) {
        round.src[j] = bound_source_item(src, src_streams[at + j]);
        round.dst[j] = bound_dest_item(dst, dst_streams[at + j], round.src[j].fill);
      }
      ok = bound_move(bound_side(src), bound_side(dst), round, dst->stream);
    }
    return ok;
  });
  if (rc) {
    for (int c : cls) dst->rw.arena.leave(c, dst->rb.calls);
    return rc;
  }
  bound_commit(dst, n, dst_streams, w, cls);
  blobs_settle(dst, n, dst_streams, taken);
  return 0;
}

int BeatriceBatch_ExportBoundStreamsInFlight(BeatriceBatch* b, int n, const int* streams, void* stream_blobs, void* wrapper_blobs) {
  BATCH_OPEN(b);
  const BoundSideOf side(b, n, streams, stream_blobs != nullptr && wrapper_blobs != nullptr);
  if (bmove::args(side) != bmove::kGo) return -1;
  if (bmove::at_rest(side, bound_rest(b, true)) != bmove::kGo) return -3;
  BeatriceBatch::RaggedWrap& r = b->rw;
  if (!blob_prepare(b, n) || !wblob_prepare(b, n) || (!b->mv.ev_export && !b->mv.ev_export.create("export event")) ||
      (!r.ev_bound_export && !r.ev_bound_export.create("bound export event")))
    return -2;
  const int rc = export_rounds(b, n, streams, stream_blobs, true);
  if (rc) return rc;
  unsigned char* out = static_cast<unsigned char*>(wrapper_blobs);
  for (int at = 0; at < n; at += r.blob_cap) {
    BoundRound round{};
    round.n = std::min(r.blob_cap, n - at);
    for (int j = 0; j < round.n; ++j) round.src[j] = bound_source_item(b, streams[at + j]);
    if (!bound_gather(bound_side(b), round, reinterpret_cast<float*>(r.d_blob_stage.get()), wblob::kBlobBytes / sizeof(float), wblob::kOffState / sizeof(float), b->stream) ||
        !hip_ok(hipMemcpyAsync(r.h_blob_stage, r.d_blob_stage, (size_t)round.n * wblob::kBlobBytes, hipMemcpyDeviceToHost, b->stream), "bound wrapper blobs down") ||
        !hip_ok(hipEventRecord(r.ev_bound_export, b->stream), "bound export event") || !hip_ok(hipEventSynchronize(r.ev_bound_export), "bound gather"))
      return -2;
    for (int j = 0; j < round.n; ++j) {
      const int s = streams[at + j];
      unsigned char* blob = r.h_blob_stage + (size_t)j * wblob::kBlobBytes;
      const wrapn::Clocks& c = r.clk[s];
      wblob::write_header(r.rate(s), c.phase_down, c.phase_up, c.fill, b->gain_in[s].target_db, b->gain_in[s].now_db,
                          b->gain_out[s].target_db, b->gain_out[s].now_db, blob);
      std::memcpy(out + (size_t)(at + j) * wblob::kBlobBytes, blob, wblob::kBlobBytes);
    }
  }
  return 0;
}

int BeatriceBatch_ImportBoundStreamsInFlight(BeatriceBatch* b, int n, const int* streams, const void* stream_blobs, const void* wrapper_blobs,
                                             const int* entry_map, int n_map) {
  BATCH_OPEN(b);
  const BoundSideOf side(b, n, streams, stream_blobs != nullptr && wrapper_blobs != nullptr && n_map >= 0 && (entry_map == nullptr) == (n_map == 0));
  if (bmove::args(side) != bmove::kGo) return -1;
  std::vector<Taken> taken;
  if (!blobs_take(b, n, stream_blobs, entry_map, n_map, &taken)) return -1;
  BeatriceBatch::RaggedWrap& r = b->rw;
  const unsigned char* in = static_cast<const unsigned char*>(wrapper_blobs);
  std::vector<BoundTaken> w(n);
  for (int i = 0; i < n; ++i) {   // (what BeatriceBatch_ImportStreamWrappers refuses)
    const unsigned char* blob = in + (size_t)i * wblob::kBlobBytes;
    double rate = 0.0;
    if (wblob::read_rate(blob, wblob::kBlobBytes, &rate) != wblob::kOk || !std::isfinite(rate)) return -1;
    wrapn::RateClass probe;   // (the rate through RateClass::configure: its hi bounds the clocks)
    wblob::Header h;
    if (!probe.configure(rate) || wblob::validate(blob, wblob::kBlobBytes, probe.hi, &h) != wblob::kOk) return -1;
    w[i] = BoundTaken{rate, wrapn::Clocks{h.phase_down, h.phase_up, h.fill}, wrapn::GainClock{h.in_target_db, h.in_now_db},
                      wrapn::GainClock{h.out_target_db, h.out_now_db}, bmove::t48_of_blob(h.fill)};
  }
  if (!bound_rates_fit(b, w)) return -1;
  if (bmove::at_rest(side, bound_rest(b, false)) != bmove::kGo) return -3;
  if (!wblob_prepare(b, n)) return -2;
  BeatriceBatch::StreamMoves::Staged& st = r.bound_staged[r.bound_imports % BeatriceBatch::StreamMoves::kCalls];
  if (st.marked && !hip_ok(hipEventSynchronize(st.done), "bound import staging entry")) return -2;
  st.marked = false;
  const size_t bytes = (size_t)n * wblob::kBlobBytes;
  if (st.h.size() < bytes) {
    PinnedBuf<unsigned char> h;
    if (!h.alloc(bytes, "bound import staging", false)) return -2;
    st.h = std::move(h);
  }
  if (!st.done && !st.done.create("bound import staging event")) return -2;
  std::vector<int> cls;
  if (bound_acquire(b, w, &cls) != 0) return -2;
  auto fail = [&]() { for (int c : cls) r.arena.leave(c, b->rb.calls); return -2; };
  if (import_rounds_in_flight(b, n, streams, stream_blobs, taken) != 0) return fail();
  std::memcpy(st.h, wrapper_blobs, bytes);
  for (int at = 0; at < n; at += r.blob_cap) {
    BoundRound round{};
    round.n = std::min(r.blob_cap, n - at);
    for (int j = 0; j < round.n; ++j) round.dst[j] = bound_dest_item(b, streams[at + j], w[at + j].clk.fill);
    if (!hip_ok(hipMemcpyAsync(r.d_blob_stage, st.h + (size_t)at * wblob::kBlobBytes, (size_t)round.n * wblob::kBlobBytes, hipMemcpyHostToDevice, b->stream), "bound wrapper blobs up") ||
        !bound_scatter(bound_side(b), round, reinterpret_cast<const float*>(r.d_blob_stage.get()), wblob::kBlobBytes / sizeof(float), wblob::kOffState / sizeof(float), b->stream))
      return fail();
  }
  if (!hip_ok(hipEventRecord(st.done, b->stream), "bound import staging event")) return fail();
  st.marked = true;
  r.bound_imports += 1;
  bound_commit(b, n, streams, w, cls);
  blobs_settle(b, n, streams, taken);
  return 0;
}
int BeatriceBatch_ResidentBlocksDelay(const BeatriceBatch* b) { return b && b->ok && b->rb.on ? b->rb.delay : -1; }
int BeatriceBatch_ResidentBlocksDelayFor(const BeatriceBatch* b, int n) { return b && b->ok && b->wrap.ready && n >= 1 ? rb_delay(b, n) : -1; }
// End of the material: every call made so far gets its output block as if silence had followed.  Several hops per step: whole made-up blocks
// of zeros of the binding's length go through the running wrapper (no caller slot is read or written for them; the gain clocks advance
// through them) until the newest hop a call needs lies in a full step.  Every full step they bring runs, an extra one included; a hop fired
// beyond the last full step is dropped when the binding then starts over as a new one does (beatrice_batch.h).
int BeatriceBatch_FlushResidentBlocks(BeatriceBatch* b) {
  BATCH_ENTER(b, Entry::FlushResidentBlocks);
  BeatriceBatch::ResidentBlocks& r = b->rb;
  if (r.dead) return -2;
  if (!sync_all(b)) return -2;           // (one hop per step and clocks per stream: everything is out now)
  if (r.jobs.empty()) return 0;
  if (r.ragged || r.H == 1) return -2;   // (cannot be: nothing stays owed there)
  if (!r.d_zero && !r.d_zero.alloc((size_t)b->B * r.channels * r.n, "rb zeros")) return -2;
  for (int guard = 0; !r.jobs.empty() && guard < 64 * r.H; ++guard) {
    const long long fed = r.hops_fed();
    if (!hip_ok(hipStreamSynchronize(b->stream), "flush sync") || !rb_step(b, true)) { r.dead = true; return -2; }   // (the made-up calls share one gain ring entry: one at a time)
    if (r.hops_fed() > fed && !sync_all(b)) return -2;   // a step went in: drained, the output halves of everything fed have run
  }
  if (!r.jobs.empty()) { r.dead = true; return -2; }
  // the binding starts over: resampler pair and FIFO as after BeatriceBatch_BindResidentBlocks (the gains keep their state), call 0 reads slot 0
  r.on = false;
  const int rc = BeatriceBatch_ConfigureWrapper(b, b->wrap.rate);
  r.on = true;
  if (rc != 0) { r.dead = true; return -2; }
  r.calls = 0; r.t48 = 0; r.hops_fired = 0; r.hops_done = 0; r.step_open = false;
  b->entries.filling_dropped(b->tk.last_feed_tick, b->tk.plan.count());   // (a hop fired beyond the last full step is gone with its step)
  r.gains.forget();
  b->io_host = 0;   // (hop k of the binding rides in resident slot (k / H) mod io_slots: wrap_post_kernel)
  return 0;
}
int BeatriceBatch_ResidentBlocksOwed(const BeatriceBatch* b) { return b && b->ok && b->rb.on ? (int)b->rb.jobs.size() : -1; }
int BeatriceBatch_ProcessBlocks(BeatriceBatch* b, const float* in, float* out, int channels, int n) {
  BATCH_ENTER(b, Entry::ProcessBlocks);
  if (channels < 1 || channels > 2 || !in || !out || n < 1 || n > wrapn::longest_block(b->wrap.rate)) return -1;
  return wrap_round_trip(b, in, out, (size_t)b->B * channels * n, [&](const float* d_in, float* d_out) { return wrap_chunk(b, d_in, d_out, channels, n); });
}

