// batch.hip -- N-stream extension ABI (include/beatrice_batch.h).
//
// One BeatriceBatch = B independent streams advancing one hop per call, sharing the immutable model
// objects.  Host-side it mirrors, per stream, the settings and the call protocol that the reference
// host keeps per plugin instance (reference src/common/processor_core_2.cc; line references at each
// function).  Device-side it is phone_forward -> pitch_forward -> wave_forward on one HIP stream,
// replayed from a hipGraph (the chain has ~70 launches per hop; hop position is read from device
// memory by the kernels, so one captured graph serves every hop).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <type_traits>
#include <chrono>
#include <deque>
#include <vector>

#include "abi_objects.h"
#include "batch_modes.h"
#include "bound_move_plan.h"
#include "beatrice_batch.h"
#include "silent_scan_plan.h"
#include "speaker_entry_plan.h"
#include "stream_blob.h"
#include "stream_move_plan.h"
#include "tick.hip.h"
#include "wrapper.hip.h"
#include "wrapper_blob.h"
#include "wrapper_turnover_plan.h"

using namespace bhip;

namespace {

struct StreamCfg {
  int target_speaker = 0;
  int kv_set_count = B_NBLOCKS;  // reference: key_value_speaker_embedding_set_count_ (processor_core_2.h:134)
  int kv_slot[B_NBLOCKS] = {0, 0, 0, 0};
  int kv_delay = 0;               // hops before the pending blocks start to install (staged morph: the reference computes the means first)
  int codebook_speaker = 0;       // after a step: the codebook of its last hop
  int codebook_row[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // codebook of each hop of the step (a morphing stream draws one per hop)
  int additive_speaker = 0;
  int formant_index = 4;
  int vq_k = 0;
  int min_q = 1, max_q = B_PITCH_BINS - 1;
  PitchParams pitch{52.0, 1.0, 0.0, 0.0, 0, 0};  // defaults: processor_core_2.h:105-110
};

// A table entry that is a morph of real speakers (BeatriceBatch_MorphSpeaker): what the per-hop codebook
// lottery needs (reference processor_core_2.cc:94-121)
struct MorphSlot {
  bool active = false;
  int n_speakers = 0;           // real speakers the weights refer to
  int n_odds = 0;               // min(n_speakers, 8)
  int order[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float odds[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // pruned weights in `order`
};

// Pinned host copy of a small per-stream device array.  Double-buffered: push() sends the buffer the
// host has been editing and flips to the other one (brought up to date first), so the host never writes
// into memory an asynchronous copy may still be reading and no step has to wait for the previous one
// just because a setting changed.  The flip only blocks if the copy issued TWO pushes ago is unfinished.
template <class T>
struct Mirror {
  T* h = nullptr;  // the buffer being edited
  DevBuf<T> d;
  size_t n = 0;
  PinnedBuf<T> buf[2];
  Event sent[2];
  bool pending[2] = {false, false};
  int cur = 0;
  // n_host elements per pinned buffer (zeroed); the device array has n_dev, zeroed if asked
  bool alloc(size_t n_host, size_t n_dev, const char* what, bool zero_dev) {
    Mirror m;
    m.n = n_host;
    for (int i = 0; i < 2; ++i) if (!m.buf[i].alloc(n_host, what) || !m.sent[i].create(what)) return false;
    if (!m.d.alloc(n_dev, what, zero_dev)) return false;
    m.h = m.buf[0];
    *this = std::move(m);
    return true;
  }
  // sends [off, off + len) of the edited buffer to dst (nullptr: d + off) for each part, then flips
  bool push_parts(hipStream_t s, int n_parts, const size_t* off, const size_t* len, T* const* dst) {
    for (int i = 0; i < n_parts; ++i)
      BHIP_TRY(hipMemcpyAsync(dst[i] ? dst[i] : d + off[i], buf[cur] + off[i], sizeof(T) * len[i], hipMemcpyHostToDevice, s));
    return flip(s);
  }
  bool flip(hipStream_t s) {
    BHIP_TRY(hipEventRecord(sent[cur], s));
    pending[cur] = true;
    const int nxt = cur ^ 1;
    if (pending[nxt]) { BHIP_TRY(hipEventSynchronize(sent[nxt])); pending[nxt] = false; }
    std::memcpy(buf[nxt], buf[cur], sizeof(T) * n);
    cur = nxt;
    h = buf[cur];
    return true;
  }
};

}  // namespace

struct BeatriceBatch {
  const Beatrice20rc0_PhoneExtractor* phone_m = nullptr;
  const Beatrice20rc0_PitchEstimator* pitch_m = nullptr;
  const Beatrice20rc0_WaveformGenerator* wave_m = nullptr;
  const Beatrice20rc0_EmbeddingSetter* embed_m = nullptr;
  int B = 0, max_speakers = 0, n_speakers = 0;
  int device = -1;  // the GPU of the model objects the batch was created from; every entry point runs with it current (DeviceScope)
  int H = 1;  // hops per step (block mode when > 1)
  bool ok = false;
  hipStream_t stream = nullptr;  // stream_own, or the caller's (BeatriceBatch_SetStream)
  Stream stream_own;
  PhoneState phone;
  PitchState pitch;
  WaveState wave;
  DevBuf<float> d_in;  // [B][H*160], shared by phone and pitch
  // speaker tables on device
  DevBuf<float> d_cb_raw, d_cbT, d_cnorm, d_add_raw, d_frm_raw, d_kv_raw;
  // per-stream settings
  std::vector<StreamCfg> cfg;
  std::vector<MorphSlot> morph;  // [max_speakers]
  int n_morph_slots = 0;
  // Which table entries the streams' settings name and which a step may still read (entry_busy; BeatriceBatch_SpeakerEntryBusy): the
  // counts, the stamps and their rule are speaker_entry_plan.h's.  A stream names kNamed entries -- target, additive and codebook
  // speaker, the four installed key/value entries (a pending install names the target).
  static constexpr int kNamed = 3 + B_NBLOCKS;
  sentry::Plan entries;
  // BeatriceBatch_MorphSpeakersInFlight: a call's descriptors, read by its kernels in place (the host runs ahead of the device)
  static constexpr int kMorphStaging = 8;
  StagedRing<MorphDesc> morph_descs;      // [kMorphStaging][max_speakers]
  long long morph_calls = 0;
  // BeatriceBatch_InstallSpeakersInFlight: a call's tables and its descriptors (only `slot` is used), likewise; allocated by the first
  // call -- kInstallStaging x min(kInstallEntries, max_speakers) x 449 KB of pinned memory, 29 MB at most
  static constexpr int kInstallStaging = 4, kInstallEntries = 16;
  StagedRing<float> install_tables;       // [kInstallStaging][cap][kInstallEntryFloats]
  PinnedBuf<MorphDesc> install_descs;     // [kInstallStaging][cap], an entry's readers are those of install_tables' entry
  long long install_calls = 0;
  // the codebook lottery's engine belongs to the stream, as the reference's belongs to the plugin instance
  // (processor_core_2.h:48,145): a stream's draws do not depend on which other streams share its batch
  std::vector<std::mt19937> lottery;  // [B]
  bool lottery_seeded = false;        // a caller's seed has been applied (first BeatriceBatch_MorphSpeaker, or BeatriceBatch_SeedLottery)
  // every per-stream setting array the kernels read lives in ONE device block with one pinned mirror, so a
  // step after any change costs a single small host-to-device copy (a dozen separate copies cost ~50 us of
  // stream time per step with 64 rotating speakers)
  Mirror<unsigned char> settings;
  // layout: [front part: arrays the front end reads][wave part: attention tile lists], and on the device the wave
  // part four times -- the waveform generator of step t reads copy t & 3, so a change can be pushed for step t while
  // the generator stages of steps t-1..t-3 are still running (their copies are refreshed when their slot comes up)
  struct { size_t cbT, cnorm, vqk, min_q, max_q, add_idx, frm_idx, params, perm[B_NBLOCKS], tile_slot[B_NBLOCKS], qperm[B_NBLOCKS], qslot[B_NBLOCKS], front_bytes, wave_bytes; } off{};
  bool front_dirty = true, wave_dirty[4] = {true, true, true, true};  // [kSlots]
  template <class T> T* host_view(size_t o) { return reinterpret_cast<T*>(settings.h + o); }
  template <class T> T* dev_view(size_t o) { return reinterpret_cast<T*>(settings.d + o); }
  void* module_owned[8 + 2 * B_NBLOCKS] = {};  // the modules' own (now unused) setting arrays, handed back before destroy()
  int pending_kv = 0;  // streams with kv_set_count < 4
  std::vector<int> row_slot[B_NBLOCKS];  // [B*H] K/V slot of attention row (stream, hop in step)
  bool kv_transient = false;  // rows of the last step's early hops still hold pre-switch slots (H > 1)
  bool vq_dirty = true;   // a VQ setting changed since the k-NN launch was last (de)selected
  // BeatriceBatch_ExportStreams / ImportStreams (stream_blob.h, stream_blob.hip): the blob's layout, fixed when the batch is created; the
  // piece table and the staging pair -- pinned host and device, `cap` = min(n, 16) blobs each -- are made by the first call that needs them
  struct StreamBlobs {
    sblob::Layout layout;
    DevBuf<BlobPiece> d_pieces;
    int n_pieces = 0, cap = 0;
    PinnedBuf<unsigned char> h_stage;
    DevBuf<unsigned char> d_stage;
  } sb;
  // BeatriceBatch_StreamQuiescent / ExportStreamsInFlight / ImportStreamsInFlight / MoveStreamsInFlight and their 48k siblings of mode F (stream_move_plan.h): which streams
  // have a step inside the tick pipeline (marked by tick_run, cleared at every drained point); the event behind an in-flight export's
  // copy; the pinned staging of the in-flight imports, a ring of two CALLS (an entry holds all the blobs of its call and grows with it;
  // its event: the call's last scatter has run); the two events of a move between batches on different streams -- the source batch's own
  // marks what the move may read, the destination's what it has read
  struct StreamMoves {
    smove::Presence seen;
    Event ev_export, ev_src, ev_dst;
    static constexpr int kCalls = 2;
    struct Staged { PinnedBuf<unsigned char> h; Event done; bool marked = false; } staged[kCalls];
    long long imports = 0;
  } mv;
  bool inflight = false;  // device-variant steps have been enqueued since the last synchronisation
  // staging for the host variant
  PinnedBuf<float> h_in, h_out;
  // One step = a chain of stages: stage 0 the front end (content encoder + pitch estimator + conditioning mix),
  // stages 1.. consecutive parts of the waveform generator (WavePart).  Each stage is its own launch (graph).
  // With pipelining off all stages go to `stream`, in order.  With a pipeline depth of n = 2..4 there are n
  // stages on n HIP streams, and stage s of step t+1 overlaps stage s+1 of step t whenever the caller enqueues
  // steps ahead of their completion: the chain is a string of ~40 launches that are each latency-bound and leave
  // most of the chip idle, so several steps in flight at different depths of the chain fill it.  Ordering:
  //   stage s of step t   after stage s-1 of step t        (data of the same step)
  //   stage s of step t   after stage s+1 of step t-3      (buffers that cross a stage boundary hold three steps:
  //                                                          three-slot phone / conditioning buffers, two spare slots
  //                                                          on the rings x[], ya2; the stages' scratch is private.
  //                                                          One step of slack keeps the ~20 us cross-stream hand-over
  //                                                          off the critical path: +2 % over two-step buffers)
  //   stage 0 of step t   after the last stage of step t-4 (counter pairs and attention tile lists have 4 copies)
  // Outputs are identical; a step that is waited for before the next is enqueued runs exactly as without pipelining.
  static constexpr int kMaxStages = 4, kSlots = 4;
  int n_stages = 2;      // stages of the current plan (2 when pipelining is off: front end, whole generator)
  bool pipelined = false;
  WavePart part[kMaxStages] = {};                 // [s], s >= 1
  Stream stage_stream_own[kMaxStages];            // [s], s >= 1; stage 0 runs on `stream`
  Event ev_done[kMaxStages][kSlots];              // stage s of step t enqueued/done, at [t & 3]
  long long steps_enqueued = 0;
  int hop_host = 0;     // mirror of the device step counter (same increments, same wrap)
  int last_parity = 0;  // slot (step counter mod 3) of the last enqueued step's phone vectors
  DevBuf<int> d_hop_wave;     // int[4][2]: {counter, I/O slot} of step t at [t & 3], for the waveform generator's stages
  bool use_graph = true;
  hipGraph_t graph[kMaxStages][kSlots] = {};      // pipelined: stage 0 uses [0][0] only; in order: [0][slot] holds the whole step
  hipGraphExec_t exec[kMaxStages][kSlots] = {};
  Event ev0, ev1;             // (timing enabled)
  DevBuf<int> d_hop_next;     // {step counter, resident-I/O slot}, double-buffered: first kernels read it, the last one writes it
  float* own_d_out = nullptr; // the waveform module's output buffer while a resident output buffer is bound
  int io_slots = 0;           // > 0: resident I/O bound (BeatriceBatch_BindResidentIO)
  bool io_mapped = false;     // BeatriceBatch_ConvertFrames: the chain reads the pinned input mirror and writes the pinned output mirror itself
  bool want_mapped = false;   // (set around the step ConvertFrames enqueues)
  float* dev_d_out = nullptr; // the waveform module's device output buffer while io_mapped
  int io_host = 0;            // mirror of the device's resident-I/O slot counter
  int last_hop = 0;           // step counter of the last enqueued step (selects the slot of the pitch head's outputs)
  tick::State tk;             // tick pipelining (tick.hip.h)
  // host streaming (BeatriceBatch_EnableHostStreaming): tick pipelining fed from / drained to HOST buffers, the copies
  // on their own streams beside the ticks
  struct HostStream {
    bool on = false;
    int n_slots = 0;
    DevBuf<float> d_in, d_out;                 // [n_slots][B][160], [n_slots][B][240]: the resident I/O the ticks use
    PinnedBuf<float> h_in, h_out;              // pinned mirrors
    Stream s_in, s_out;
    std::vector<Event> ev_in, ev_out;          // per slot: upload done / download done
    std::vector<Event> ev_tick;                // ring over ticks: tick launched (recorded on the batch's stream)
    struct Pending { long long step; int slot; long long done_tick; bool fetched; };
    std::deque<Pending> pending;               // steps fed and not yet handed back, oldest first
    long long fed = 0;
    long long rec[2] = {-1, -1};               // ticks whose events were recorded last and second to last
    bool mapped = false;                       // the ticks read and write the pinned mirrors themselves (no copies, no copy streams)
    std::vector<long long> tick_of_ev;         // which tick the event in ev_tick[i] was recorded behind
  } hs;
  // any-rate device wrapper (wrapper.hip.h): the reference host's gains, resampler pair and 480-sample FIFO for all streams
  wrapn::RateClass wrap;                            // (wrapper_plan.h: everything the host decides about a call)
  wrapn::Clocks wrap_clk{};
  std::vector<wrapn::GainClock> gain_in, gain_out;  // [B]
  DevBuf<wrapn::StreamState> d_wrap;                // [B]
  DevBuf<float> d_wrap_taps, d_wrap_inner, d_wrap_io;   // taps: down | up; inner [B][kInnerStride]
  PinnedBuf<float> h_wrap_io;
  Mirror<wrapn::GainSeg> wrap_gains;                // [2][B]: input | output segments of the current call
  bool wrap_gains_constant = false;                 // the device copy holds constant segments that are still right
  // 48 kHz device wrapper (configs[4])
  DevBuf<Wrap48State> d_w48;
  // the same wrapper around the TICK pipeline (BeatriceBatch_BindResidentIO48k): resident 48 kHz slots, own 16 / 24 kHz slots between
  struct Resident48 {
    bool on = false;
    int channels = 0, n_slots = 0;
    const float* d_in48 = nullptr;   // [n_slots][B][channels][480]
    float* d_out48 = nullptr;        // [n_slots][B][channels][480]
    DevBuf<float> d_in16, d_out24;                // [n_slots][B][160], [n_slots][B][240]: the resident I/O of the ticks
    int deferred_slot = -1;                       // step completed by the last tick, its 48 kHz block not yet produced
    long long deferred_step = -1;                 // ... and which step that was (its per-stream counters name its silent streams)
  } r48;
  DevBuf<float> d_coef_down, d_coef_up, d_io48;   // io: in [B][2][480] | out [B][2][480]
  PinnedBuf<float> h_io48;
  // The shell's silent-block rule per stream (BeatriceBatch_EnableSilentBlockRule; kernels_misc.hip.h freeze_*): streams
  // flagged for the next 48 kHz block stand still -- model state, wrapper state, key/value installs, codebook lottery
  struct SilentRule {
    bool on = false;
    std::vector<unsigned char> next;    // [B] flags of the step to come (cleared by the step)
    bool any_next = false;
    bool in_block_step = false;         // the step being enqueued belongs to a 48 kHz block (only those honour `next`)
    static constexpr int kDepth = 4;
    StagedRing<unsigned char> flags;    // [kDepth][B]: a step's flags, pinned staging and device copy; an entry's event: its upload AND the step that reads the device copy are done
    DevBuf<FreezeRing> d_rings;
    int n_rings = 0;
    DevBuf<float> d_keep;               // copies of the single-slot rings, all streams
    DevBuf<int> d_keep_prev_q;          // [B]
    long long steps = 0;
  } silent;
  // The any-rate wrapper with clocks PER STREAM (BeatriceBatch_ConfigureWrapperRates / ProcessBlocksRagged; wrapper.hip.h
  // RagStream): every stream its own host rate, block length and FIFO phase; a stream may sit a call out
  struct RaggedWrap {
    bool ready = false;
    std::vector<wrapn::RateClass> classes;         // one per distinct host rate: ratio and tap tables
    std::vector<int> cls;                          // [B] class of each stream
    std::vector<wrapn::Clocks> clk;                // [B] the stream's two resampler clocks and its FIFO fill
    wrapn::CallPlanner next;                       // the state a call being planned would leave: the batch's once every stream's plan stands
    double rate(int s) const { return classes[cls[s]].rate; }
    std::vector<double> rates() const { std::vector<double> v(cls.size()); for (size_t s = 0; s < v.size(); ++s) v[s] = rate((int)s); return v; }
    std::vector<int> taps_down_off, taps_up_off;   // per class: float offsets into d_taps
    DevBuf<float> d_taps;
    // Inside a binding with clocks per stream (BeatriceBatch_SetStreamRateInFlight, wrapper_turnover_plan.h): the classes keep their
    // index and their place in d_taps while a call that is owed names them -- `arena` slot i is classes[i] (a slot that is not held: a
    // class that is gone, its index free); new tables go up through pinned staging of the buffer's length; a buffer that was outgrown,
    // and its staging, wait for the unbind (launches already enqueued hold them)
    wturn::TapArena arena;
    PinnedBuf<float> h_taps;
    std::vector<DevBuf<float>> d_taps_outgrown;
    std::vector<PinnedBuf<float>> h_taps_outgrown;
    static constexpr int kStage = 4;
    StagedRing<wrapn::RagStream> rs;               // [kStage][B]: a call's per-stream records, pinned staging and device copy
    long long calls = 0;
    DevBuf<unsigned char> d_frozen;                // [kMaxChunks][B]: per FIFO chunk, the streams that do not fire a hop in it
    // BeatriceBatch_ExportStreamWrappers / ImportStreamWrappers (wrapper_blob.h): the one-piece table over d_wrap for stream_gather /
    // stream_scatter and the staging pair -- `blob_cap` = min(n, 16) blobs each -- made by the first call that needs them
    DevBuf<BlobPiece> d_blob_piece;
    PinnedBuf<unsigned char> h_blob_stage;
    DevBuf<unsigned char> d_blob_stage;
    int blob_cap = 0;
    // the in-flight form of the two (BeatriceBatch_ExportBoundStreamsInFlight / ImportBoundStreamsInFlight): the event behind an export's
    // copy; pinned staging of the imports, a ring of two CALLS as StreamMoves::Staged (the device staging is shared with the drained
    // calls: everything that uses it is on the batch's stream, in order)
    Event ev_bound_export;
    StreamMoves::Staged bound_staged[StreamMoves::kCalls];
    long long bound_imports = 0;
  } rw;
  // The any-rate wrapper around the tick pipeline (BeatriceBatch_BindResidentBlocks): host-rate blocks resident on the device,
  // the input half of the chain in front of the ticks, the output half `delay` calls later (wrapper.hip.h wrap_post_kernel)
  struct ResidentBlocks {
    bool on = false;
    bool dead = false;   // a call of the uniform form failed (rb_step).  A plan that is refused moves no clock; what this guards is a failure after
                         // the commit -- a launch, a tick, the gain ring: host and device wrapper state may no longer agree, every further call
                         // is refused with -2 until the binding is released
    int channels = 0, n = 0, n_slots = 0, io_slots = 0, delay = 0, ring = 0;
    const float* d_in = nullptr;   // [n_slots][B][channels][n]
    float* d_out = nullptr;        // [n_slots][B][channels][n]
    DevBuf<float> d_in16, d_out24;                 // [io_slots][B][H][160], [io_slots][B][H][240]: the resident I/O of the ticks
    StagedRing<wrapn::GainSeg> gains;                        // [ring][2][B]: a call's input | output segments, read by the kernels in place; an entry's
                                                             // event: the output half that read it has run (it guards h_rs[entry] of the per-stream form too)
    long long calls = 0, t48 = 0;                            // calls so far; 48 kHz samples fed so far
    long long hops_fired = 0;                                // model hops the FIFO has fired; hop k = hop k % H of step k / H
    long long hops_done = 0;                                 // hops of the steps fed by the end of the previous call
    int H = 1;                                               // hops per step of the batch
    long long hops_fed() const { return hops_fired / H * H; }   // ... of which the hops of full steps are inside (or through) the ticks
    bool step_open = false;                                  // a hop has fired into a step that is not fed yet, or is being fed (speaker_entry_plan.h)
    struct Job {
      long long call, t0; wrapn::Dir dout;
      long long last_hop() const { return (t0 + dout.n_in - 1) / wrapn::kBlock - 1; }   // the newest model hop its samples come from (wrap_post_kernel)
    };
    std::deque<Job> jobs;                                    // calls whose output half is still to run, oldest first
    DevBuf<float> d_zero;                                    // [B][channels][n] zeros: the input of the calls BeatriceBatch_FlushResidentBlocks makes up
    // the form with clocks PER STREAM (BeatriceBatch_BindResidentBlocksRagged; the rates, clocks and tap tables are `rw`'s): a slot
    // holds one cell of channels x max_samples floats per stream; a call's per-stream records stay on the device until its output
    // half has run; slot_map[b][g mod map_ring] = the resident slot of the step that stream b's hop g rode in
    bool ragged = false;
    int max_samples = 0, cell = 0, map_ring = 0;
    PinnedBuf<wrapn::RagStream> h_rs;                        // [ring][B], read by the kernels in place
    DevBuf<int> d_map;                                       // [B][map_ring]
    std::vector<long long> t48_s;                            // [B] 48 kHz samples of the stream fed so far
    std::vector<int> hops_s;                                 // [B] model hops the stream has fired
    // a stream that starts over inside the binding (BeatriceBatch_SetStreamRateInFlight / RestartStreamInFlight): t48_s counts from the
    // restart, hops_s goes on; the record of the stream's next block carries the restart to both wrapper kernels (wrapn::RagStream)
    std::vector<int> hop_base_s;                             // [B] hops_s at the stream's last restart
    std::vector<unsigned char> restart_s;                    // [B] the restart has not travelled yet
    int hops_cap = 0;                                        // hops one stream may fire per call: what io_slots and slot_map were sized for
    // BeatriceBatch_BoundStreamQuiescent / MoveBoundStreamsInFlight / ExportBoundStreamsInFlight / ImportBoundStreamsInFlight
    // (bound_move_plan.h): every stream's last active call of the binding
    bmove::Marks marks;
  } rb;
  // BeatriceBatch_ScanSilentBlocks* (silent_scan_plan.h, silent_scan.hip): the shell's test on blocks the caller keeps on the device.
  // Beside the batch, not of it: a stream of its own, a ring of kTickets staging entries -- the kernel's flags on the device, the pinned
  // copy its one download lands in, the per-cell lengths the kernel reads in place -- each grown by the Begin that needs more, and the
  // event behind an entry's download.  No step looks at any of it.
  struct SilentScan {
    sscan::TicketRing tickets;
    Stream stream;                       // made by the first call that passes no stream of its own
    struct Entry {
      DevBuf<unsigned char> d_flags;     // [cap] one byte per block
      PinnedBuf<unsigned char> h_flags;  // [cap]
      PinnedBuf<int> h_len;              // [cap] (cells <= blocks)
      Event done;
    } entry[sscan::kTickets];
    void settle() { for (Entry& e : entry) if (e.done) (void)hipEventSynchronize(e.done); }   // (before the entries are freed)
  } scan;
};

namespace {

hipStream_t stage_stream(const BeatriceBatch* b, int s) { return b->pipelined && s > 0 ? b->stage_stream_own[s].get() : b->stream; }
hipStream_t wave_stream(const BeatriceBatch* b) { return stage_stream(b, b->n_stages - 1); }  // where a step's output appears
bool tick_drain(BeatriceBatch* b);
void drop_graph(BeatriceBatch* b);
// Waits for the steps enqueued so far (needed before the graph or a speaker table they use is replaced;
// the pinned setting mirrors are double-buffered and do not need it).
bool sync_all(BeatriceBatch* b) {
  bool ok = !b->tk.on || tick_drain(b);  // steps still inside the tick pipeline come out first
  ok = hip_ok(hipStreamSynchronize(b->stream), "sync") && ok;
  for (int s = 1; s < BeatriceBatch::kMaxStages; ++s)
    if (b->stage_stream_own[s]) ok = hip_ok(hipStreamSynchronize(b->stage_stream_own[s]), "sync stage") && ok;
  b->inflight = false;
  // a one-stream batch runs the modules' team launches (team.hip.h): a timeout voids the steps since the last synchronisation; the
  // stream restarts from silence on the per-layer launches (engine.h team_recover)
  if (team_timed_out(b->phone) || team_timed_out(b->pitch) || team_timed_out(b->wave)) {
    std::fprintf(stderr, "beatrice_hip: a team launch timed out; the batch's stream was reset and continues on the per-layer launches\n");
    // (each module recovers for itself: the one whose team gave a wait up restarts from silence, the others' state is valid and stays)
    const bool pitch_too = team_timed_out(b->pitch);
    team_recover(b->phone, b->stream); team_recover(b->pitch, b->stream); team_recover(b->wave, b->stream);
    if (pitch_too) (void)hipMemsetAsync(b->pitch.d_prev_q, 0, sizeof(int) * b->B, b->stream);   // (the one piece of the pitch estimator's state outside its rings)
    drop_graph(b);
    ok = false;
  }
  if (b->tk.h_link_dead && *b->tk.h_link_dead) {   // a GRU cell of a tick gave up waiting for the cell of the hop before (tick.hip.h): results are void
    std::fprintf(stderr, "beatrice_hip: tick launch: a linked GRU cell timed out\n");
    b->ok = false;
    ok = false;
  }
  return ok;
}
// Experiment switch: BEATRICE_HIP_CUMASK="lo-hi;lo-hi;..." gives the stream of stage 0, 1, ... a CU mask (CU index
// ranges), so that concurrently running stages do not land on the same CUs.
bool make_stage_stream(Stream& st, int stage) {
  hipStream_t s = nullptr;
  const char* spec = std::getenv("BEATRICE_HIP_CUMASK");
  if (spec) {
    std::string sp(spec);
    size_t pos = 0;
    for (int i = 0; i < stage && pos != std::string::npos; ++i) { pos = sp.find(';', pos); if (pos != std::string::npos) ++pos; }
    if (pos != std::string::npos && pos < sp.size()) {
      int lo = 0, hi = -1;
      if (std::sscanf(sp.c_str() + pos, "%d-%d", &lo, &hi) == 2 && lo >= 0 && hi >= lo && hi < 512) {
        uint32_t mask[16] = {};
        for (int c = lo; c <= hi; ++c) mask[c >> 5] |= 1u << (c & 31);
        if (!hip_ok(hipExtStreamCreateWithCUMask(&s, 16, mask), "cu mask stream")) return false;
        st.adopt(s);
        return true;
      }
    }
  }
  if (!make_stream(&s)) return false;
  st.adopt(s);
  return true;
}

// stage plans by pipeline depth (waveform parts: 1 input mix, 2..5 blocks, 6 upsampler GEMMs, 7 tail); the cuts
// balance the measured stage times at 256 streams (front end 83 us, generator 200 us)
void set_plan(BeatriceBatch* b, int depth) {
  b->pipelined = depth >= 2;
  b->n_stages = depth < 2 ? 2 : depth;
  switch (b->n_stages) {
    case 2: b->part[1] = WavePart{1, 7, 0}; break;
    case 3: b->part[1] = WavePart{1, 4, 0}; b->part[2] = WavePart{5, 7, 1}; break;
    default: b->part[1] = WavePart{1, 3, 0}; b->part[2] = WavePart{4, 5, 1}; b->part[3] = WavePart{6, 7, 2}; break;
  }
}
void settle(BeatriceBatch* b) {
  if (b->inflight) (void)sync_all(b);
}

// Tick mode splits the attention rows of a step between two kinds of workgroup (rowchain.hip.h): 16-row tiles that share a
// K/V slot (block_b_body) and quads of <= 4 rows (block_bq_body).  BEATRICE_HIP_TICK_NO_QUADS: A/B switch for measurements.
bool quads_on(const BeatriceBatch* b) {
  static const bool no_quads = bhip::meas_env("BEATRICE_HIP_TICK_NO_QUADS") != nullptr;
  return b->tk.on && b->wave.d_ktp[0] != nullptr && !no_quads;
}
void rebuild_tiles(BeatriceBatch* b, int blk) {
  // attention rows (stream, hop in step) grouped by K/V slot, ascending slot then ascending row, 16 per tile
  const int nt = b->wave.n_tiles_max, rows = b->B * b->H;
  int* perm = b->host_view<int>(b->off.perm[blk]);
  int* slot = b->host_view<int>(b->off.tile_slot[blk]);
  for (bool& d : b->wave_dirty) d = true;
  const std::vector<int>& rs = b->row_slot[blk];
  std::fill(perm, perm + (size_t)nt * 16, -1);
  std::fill(slot, slot + nt, -1);
  std::vector<int> order(rows);
  for (int i = 0; i < rows; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return rs[x] < rs[y]; });
  // In-order modes: every row in a tile of its slot (at most one partial tile per slot).  Tick mode: a slot's rows fill whole
  // tiles first; a remainder of >= 8 rows is one more (padded) tile, a smaller one goes to the quad list -- with 64 speakers
  // on 256 streams that is 64 quads instead of 64 tiles with 12 of 16 rows empty.
  const bool quads = quads_on(b);
  int* qperm = b->host_view<int>(b->off.qperm[blk]);
  int* qslot = b->host_view<int>(b->off.qslot[blk]);
  std::fill(qperm, qperm + (size_t)nt * 16, -1);
  std::fill(qslot, qslot + (size_t)nt * 4, -1);
  int tile = 0, quad = 0;
  for (int i = 0; i < rows;) {
    const int sl = rs[order[i]];
    int n = 1;
    while (i + n < rows && rs[order[i + n]] == sl) ++n;
    int at = 0;
    while (n - at >= (quads ? 8 : 1)) {
      const int take = std::min(16, n - at);
      slot[tile] = sl;
      for (int e = 0; e < take; ++e) perm[tile * 16 + e] = order[i + at + e];
      ++tile; at += take;
    }
    while (at < n) {
      const int take = std::min(4, n - at);
      qslot[quad] = sl;
      for (int e = 0; e < take; ++e) qperm[quad * 4 + e] = order[i + at + e];
      ++quad; at += take;
    }
    i += n;
  }
}

void fill_row_slots(BeatriceBatch* b, int s) {
  for (int blk = 0; blk < B_NBLOCKS; ++blk)
    for (int hh = 0; hh < b->H; ++hh) b->row_slot[blk][(size_t)s * b->H + hh] = b->cfg[s].kv_slot[blk];
}

// Brings the entry reference counts up to stream s's settings.  An entry whose last reference goes is still read by the steps inside the
// tick pipeline that were fed while it was named: the last of them is the step fed last -- or the one about to be fed
// (next_step_too: advance_kv at several hops per step, whose early hops still run on the blocks installed before).
// What the stamp reads of the pipeline (speaker_entry_plan.h): the tick counters, and whether a step of the uniform any-rate blocks is
// still filling.
sentry::Clock entry_clock(const BeatriceBatch* b) {
  return {b->tk.tick, b->tk.last_feed_tick, b->tk.plan.count(), b->rb.on && b->rb.step_open};
}
void recount(BeatriceBatch* b, int s, bool next_step_too = false) {
  const StreamCfg& c = b->cfg[s];
  const int now[BeatriceBatch::kNamed] = {c.target_speaker, c.additive_speaker, c.codebook_speaker, c.kv_slot[0], c.kv_slot[1], c.kv_slot[2], c.kv_slot[3]};
  b->entries.name(s, now, entry_clock(b), next_step_too);
}

void sync_stream_arrays(BeatriceBatch* b, int s) {
  const StreamCfg& c = b->cfg[s];
  recount(b, s);
  for (int hh = 0; hh < b->H; ++hh) {  // k-NN rows are (stream, hop in step)
    b->host_view<const float*>(b->off.cbT)[(size_t)s * b->H + hh] = b->d_cbT + (size_t)c.codebook_row[hh] * B_PHONE_CH * B_CODEBOOK;
    b->host_view<const float*>(b->off.cnorm)[(size_t)s * b->H + hh] = b->d_cnorm + (size_t)c.codebook_row[hh] * B_CODEBOOK;
  }
  b->host_view<int>(b->off.vqk)[s] = c.vq_k;
  b->host_view<int>(b->off.min_q)[s] = c.min_q;
  b->host_view<int>(b->off.max_q)[s] = c.max_q;
  b->host_view<int>(b->off.add_idx)[s] = c.additive_speaker;
  b->host_view<int>(b->off.frm_idx)[s] = c.formant_index;
  b->host_view<PitchParams>(b->off.params)[s] = c.pitch;
  b->front_dirty = true;
}

// A BeatriceBatch_ResetStreamInFlight of stream s that no step has taken yet (tick mode keeps the flags; they exist once the first
// such call has sized them).
bool reset_waits_for(const BeatriceBatch* b, int s) {
  return b->tk.on && b->tk.any_reset_pending && (int)b->tk.reset_pending.size() == b->B && b->tk.reset_pending[s] != 0;
}
// processor_core_2.cc:270,414: `while (SetKeyValueSpeakerEmbedding());` -- every block still to come, now
void flush_kv(StreamCfg& c) {
  c.kv_delay = 0;
  for (; c.kv_set_count < B_NBLOCKS; ++c.kv_set_count) c.kv_slot[c.kv_set_count] = c.target_speaker;
}

// One K/V block per stream per hop, as the reference host does before its three per-hop calls
// (processor_core_2.cc:179-181, processor_core_2.h:161-169).
void advance_kv(BeatriceBatch* b) {
  if (b->pending_kv == 0 && !b->kv_transient) return;
  bool dirty[B_NBLOCKS] = {false, false, false, false};
  bool advanced = false, mixed_left = false;
  const int H = b->H;
  for (int s = 0; s < b->B; ++s) {
    StreamCfg& c = b->cfg[s];
    if (b->silent.any_next && b->silent.next[s]) {   // a silent block: the reference does not reach its per-hop protocol
      // (several hops per step: a switch that completed INSIDE the stream's last step left its rows on mixed key/value entries -- hop 0 had
      //  one new block, hop 1 two ... --; they are brought to the settled entries in the stream's next step, so the pass must come back for it)
      for (int hh = 0; hh < H && H > 1 && !mixed_left; ++hh)
        for (int blk = 0; blk < B_NBLOCKS; ++blk) mixed_left = mixed_left || b->row_slot[blk][(size_t)s * H + hh] != c.kv_slot[blk];
      continue;
    }
    bool installed = false;
    // A BeatriceBatch_ResetStreamInFlight that this step takes: the step is the first of a new stream, on all four blocks of the target the
    // stream has NOW (the flush at the call covered the target of that moment; a switch made since, while the stream sat out or in the
    // same gap, must not install one block per hop behind the reset).
    if (c.kv_set_count < B_NBLOCKS && reset_waits_for(b, s)) {
      flush_kv(c);
      advanced = true;
      installed = true;
    }
    for (int hh = 0; hh < H; ++hh) {  // the hops of this step, each preceded by one block install
      if (c.kv_delay > 0) {
        --c.kv_delay;
      } else if (c.kv_set_count < B_NBLOCKS) {
        c.kv_slot[c.kv_set_count] = c.target_speaker;
        ++c.kv_set_count;
        advanced = true;
        installed = true;
      }
      for (int blk = 0; blk < B_NBLOCKS; ++blk) {
        int& rs = b->row_slot[blk][(size_t)s * H + hh];
        if (rs != c.kv_slot[blk]) { rs = c.kv_slot[blk]; dirty[blk] = true; }
      }
    }
    if (installed) recount(b, s, H > 1);
  }
  int still = 0;
  for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++still;
  b->pending_kv = still;
  b->kv_transient = (advanced && H > 1) || mixed_left;
  for (int blk = 0; blk < B_NBLOCKS; ++blk) if (dirty[blk]) rebuild_tiles(b, blk);
}

// what changed since the last step goes to the device: the front part as it is, the wave part into the copy the
// waveform generator of THIS step (parity) will read
bool push_settings(BeatriceBatch* b, int parity /* slot: step & 3 */) {
  size_t off[2], len[2];
  unsigned char* dst[2];
  int n = 0;
  if (b->front_dirty) { off[n] = 0; len[n] = b->off.front_bytes; dst[n] = nullptr; ++n; }
  if (b->wave_dirty[parity]) {
    off[n] = b->off.front_bytes; len[n] = b->off.wave_bytes;
    dst[n] = b->settings.d + b->off.front_bytes + (size_t)parity * b->off.wave_bytes; ++n;
  }
  if (n == 0) return true;
  b->front_dirty = false;
  b->wave_dirty[parity] = false;
  return b->settings.push_parts(b->stream, n, off, len, dst);
}

// Front end.  Latency-bound regime (a few hundred rows): the pitch estimator's launches are paired into the
// content encoder's (front.hip); elsewhere the modules run one after the other.  (Running them as parallel
// graph branches was measured and buys nothing on ROCm 7.2 / MI355X, profiles/r01_notes.md.)
void enqueue_front(BeatriceBatch* b, hipStream_t st) {
  static const bool no_pairs = bhip::meas_env("BEATRICE_HIP_NO_PAIRS") != nullptr;  // A/B switch for measurements
  if (!no_pairs && front_forward(b->phone_m->w, b->phone, b->pitch_m->w, b->pitch, b->wave_m->w, b->wave, st)) return;
  phone_forward(b->phone_m->w, b->phone, st);
  pitch_forward(b->pitch_m->w, b->pitch, st);
  wave_cond(b->wave_m->w, b->wave, st);
}
void enqueue_wave(BeatriceBatch* b, int stage, int slot, hipStream_t st) {
  b->wave.hop = b->d_hop_wave + 2 * slot;
  for (int blk = 0; blk < B_NBLOCKS; ++blk) {  // this slot's copy of the attention tile lists
    b->wave.d_perm[blk] = b->dev_view<int>(b->off.perm[blk] + (size_t)slot * b->off.wave_bytes);
    b->wave.d_tile_slot[blk] = b->dev_view<int>(b->off.tile_slot[blk] + (size_t)slot * b->off.wave_bytes);
  }
  wave_forward(b->wave_m->w, b->wave, st, /*cond_done=*/true, b->part[stage]);
}

void drop_graph(BeatriceBatch* b) {
  for (auto& per_stage : b->exec) for (hipGraphExec_t& e : per_stage) { if (e) (void)hipGraphExecDestroy(e); e = nullptr; }
  for (auto& per_stage : b->graph) for (hipGraph_t& g : per_stage) { if (g) (void)hipGraphDestroy(g); g = nullptr; }
}

template <class F>
bool capture(hipStream_t st, hipGraph_t* graph, hipGraphExec_t* exec, F enqueue) {
  BHIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  enqueue();
  BHIP_TRY(hipStreamEndCapture(st, graph));
  BHIP_TRY(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
  return true;
}

// pipelining off: the whole step as ONE launch on the batch's stream (a second graph launch per step costs ~15 us)
bool run_step_in_order(BeatriceBatch* b, int slot) {
  hipStream_t st = b->stream;
  auto enqueue_slot = [b, st](int sl) { enqueue_front(b, st); for (int s = 1; s < b->n_stages; ++s) enqueue_wave(b, s, sl, st); };
  if (!b->use_graph) { if (slot >= 0) enqueue_slot(slot); return hip_ok(hipGetLastError(), "step launch"); }
  if (slot < 0 || !b->exec[0][slot])  // first use: capture the variants of all four slots at once, so that no later step pays for a capture
    for (int sl = 0; sl < BeatriceBatch::kSlots; ++sl)
      if (!b->exec[0][sl] && !capture(st, &b->graph[0][sl], &b->exec[0][sl], [&] { enqueue_slot(sl); })) return false;
  if (slot < 0) return true;  // capture only (BeatriceBatch_Prepare)
  BHIP_TRY(hipGraphLaunch(b->exec[0][slot], st));
  return true;
}

bool run_stage(BeatriceBatch* b, int stage, int slot) {
  hipStream_t st = stage_stream(b, stage);
  auto enqueue_slot = [b, stage, st](int sl) { if (stage == 0) enqueue_front(b, st); else enqueue_wave(b, stage, sl, st); };
  if (!b->use_graph) { if (slot >= 0) enqueue_slot(slot); return hip_ok(hipGetLastError(), "stage launch"); }
  const int g = stage == 0 || slot < 0 ? 0 : slot;  // the front end reads its counter through one fixed pointer
  if (slot < 0 || !b->exec[stage][g])  // first use: every slot's variant of this stage at once (no capture inside a later step)
    for (int sl = 0; sl < (stage == 0 ? 1 : BeatriceBatch::kSlots); ++sl)
      if (!b->exec[stage][sl] && !capture(st, &b->graph[stage][sl], &b->exec[stage][sl], [&] { enqueue_slot(sl); })) return false;
  if (slot < 0) return true;  // capture only (BeatriceBatch_Prepare)
  BHIP_TRY(hipGraphLaunch(b->exec[stage][g], st));
  return true;
}

// the k-NN launch is dropped while no stream uses the codebook (phone.out then writes the module output)
void update_vq_mode(BeatriceBatch* b) {
  bool none = true;
  for (const StreamCfg& c : b->cfg) none = none && c.vq_k == 0;
  if (none != b->phone.skip_vq) { settle(b); b->phone.skip_vq = none; drop_graph(b); b->tk.table_dirty = true; }
}

// streams whose target is a morphed entry draw the codebook of ONE real speaker per hop, with the
// morph weights as odds (reference processor_core_2.cc:94-121: same draws, same order of operations), from
// the stream's own engine
void draw_codebooks(BeatriceBatch* b) {
  if (b->n_morph_slots == 0) return;
  for (int s = 0; s < b->B; ++s) {
    StreamCfg& c = b->cfg[s];
    MorphSlot& m = b->morph[c.target_speaker];
    if (!m.active) continue;
    if (b->silent.any_next && b->silent.next[s]) continue;   // no hop, no draw
    std::mt19937& rng = b->lottery[s];
    float sum = 0.0f;
    for (int i = 0; i < m.n_odds; ++i) sum += m.odds[i];
    for (int hh = 0; hh < b->H; ++hh) {
      int idx = m.order[0];
      if (sum <= std::numeric_limits<float>::epsilon()) {
        idx = std::uniform_int_distribution<int>(0, m.n_speakers - 1)(rng);
      } else {
        float r = std::uniform_real_distribution<float>(0.0f, sum)(rng);
        for (int i = 0; i < m.n_odds; ++i) {
          r -= m.odds[i];
          if (r < 0.0f) { idx = m.order[i]; break; }
        }
      }
      c.codebook_row[hh] = idx;
    }
    c.codebook_speaker = c.codebook_row[b->H - 1];
    sync_stream_arrays(b, s);
  }
}

bool tick_run(BeatriceBatch* b, bool feeding);
bool project_speakers(BeatriceBatch* b, int first, int count);
// Host-buffer steps (BeatriceBatch_ConvertFrames) let the kernels read the pinned input mirror and write the pinned output
// mirror directly: two copy commands around the chain cost a switch to the copy engine and back each (0.35 -> 0.31 ms per
// step at 256 streams); every other kind of step uses the device buffers.
bool set_io_mapped(BeatriceBatch* b, bool on) {
  if (on == b->io_mapped) return true;
  if (on && (b->io_slots > 0 || b->tk.on || b->pipelined)) return true;   // not applicable: ConvertFrames copies as before
  if (!sync_all(b)) return false;
  drop_graph(b);  // kernel arguments change
  if (on) {
    b->dev_d_out = b->wave.d_out;
    b->phone.d_in = b->pitch.d_in = b->h_in;
    b->wave.d_out = b->h_out;
  } else {
    b->phone.d_in = b->pitch.d_in = b->d_in;
    b->wave.d_out = b->dev_d_out;
    b->dev_d_out = nullptr;
  }
  b->io_mapped = on;
  return true;
}

bool step_device(BeatriceBatch* b, const float* d_in, float* d_out) {
  if (b->io_slots > 0 && (d_in || d_out)) return false;  // resident I/O is bound: the step reads and writes its slots
  if (b->io_mapped != b->want_mapped && !set_io_mapped(b, b->want_mapped)) return false;
  if (b->tk.on) return tick_run(b, true);
  if (b->silent.any_next && !b->silent.in_block_step) {   // flags name streams of the next 48 kHz BLOCK: any other kind
    std::fill(b->silent.next.begin(), b->silent.next.end(), 0);           // of step runs for every stream
    b->silent.any_next = false;
  }
  advance_kv(b);
  draw_codebooks(b);
  if (b->vq_dirty) { update_vq_mode(b); b->vq_dirty = false; }
  const long long t = b->steps_enqueued;
  const int slot = b->hop_host & 3, slot2 = (slot + 1) & 3 /* step t-3 */, last = b->n_stages - 1;
  hipStream_t fs = b->stream;
  if (!b->pipelined) {
    if (!push_settings(b, slot)) return false;
    if (d_in && d_in != b->d_in)
      BHIP_TRY(hipMemcpyAsync(b->d_in, d_in, sizeof(float) * b->B * b->H * B_IN_HOP, hipMemcpyDeviceToDevice, fs));
    if (!run_step_in_order(b, slot)) return false;
    if (d_out && d_out != b->wave.d_out)
      BHIP_TRY(hipMemcpyAsync(d_out, b->wave.d_out, sizeof(float) * b->B * b->H * B_OUT_HOP, hipMemcpyDeviceToDevice, fs));
    b->last_parity = b->hop_host % 3;
    b->last_hop = b->hop_host;
    b->hop_host = hop_next(b->hop_host);
    if (b->io_slots > 0) b->io_host = (b->io_host + 1) % b->io_slots;
    b->steps_enqueued = t + 1;
    b->inflight = true;
    return true;
  }
  // ordering rules: see the comment at BeatriceBatch::n_stages
  if (t >= 3) BHIP_TRY(hipStreamWaitEvent(fs, b->ev_done[1][slot2], 0));
  if (t >= 4) BHIP_TRY(hipStreamWaitEvent(fs, b->ev_done[last][slot], 0));
  if (!push_settings(b, slot)) return false;
  if (d_in && d_in != b->d_in)
    BHIP_TRY(hipMemcpyAsync(b->d_in, d_in, sizeof(float) * b->B * b->H * B_IN_HOP, hipMemcpyDeviceToDevice, fs));
  if (!run_stage(b, 0, slot)) return false;
  BHIP_TRY(hipEventRecord(b->ev_done[0][slot], fs));
  for (int s = 1; s <= last; ++s) {
    hipStream_t st = stage_stream(b, s);
    BHIP_TRY(hipStreamWaitEvent(st, b->ev_done[s - 1][slot], 0));
    if (s < last && t >= 3) BHIP_TRY(hipStreamWaitEvent(st, b->ev_done[s + 1][slot2], 0));
    if (!run_stage(b, s, slot)) return false;
    if (s == last && d_out && d_out != b->wave.d_out)
      BHIP_TRY(hipMemcpyAsync(d_out, b->wave.d_out, sizeof(float) * b->B * b->H * B_OUT_HOP, hipMemcpyDeviceToDevice, st));
    BHIP_TRY(hipEventRecord(b->ev_done[s][slot], st));
  }
  b->last_parity = b->hop_host % 3;
  b->last_hop = b->hop_host;
  b->hop_host = hop_next(b->hop_host);
  if (b->io_slots > 0) b->io_host = (b->io_host + 1) % b->io_slots;
  b->steps_enqueued = t + 1;
  b->inflight = true;
  return true;
}

#include "batch_tick.hip.h"      // tick mode: table, per-tick host work, drain, enable

using modes::Entry;
modes::Flags flags_of(const BeatriceBatch* b) {
  return {b->tk.on, b->hs.on, b->r48.on, b->rb.on, b->rb.ragged, b->silent.on, b->pipelined, b->io_slots > 0, b->H, b->wrap.ready, b->rw.ready};
}
// (a) some stream's settings name the entry; (b) in tick mode and every mode around it (D, E, F, G, P): a step that named it is still
// inside the pipeline, or still filling (speaker_entry_plan.h; a drain runs the ticks that bring tk.tick up to every stamp)
bool entry_named(const BeatriceBatch* b, int e) { return b->entries.busy(e, b->tk.tick, modes::mode_of(flags_of(b))); }
// ... or (c) its CODEBOOK may be what a step drew: recount() counts the codebook of a stream's last hop, not the lottery's candidates
// (draw_codebooks), so an entry is also busy while an active morph entry m that is itself named -- (a) or (b): the steps that could have
// drawn from m's list are exactly the steps that named m -- lists it with positive odds, or with any odds when all of m's are zero (the
// lottery then draws from all of m's speakers).  A walk over the table's morph entries at call time; no step looks at this.
bool entry_busy(const BeatriceBatch* b, int e) {
  if (entry_named(b, e)) return true;
  if (b->n_morph_slots == 0) return false;
  for (int m = 0; m < b->max_speakers; ++m) {
    const MorphSlot& ms = b->morph[m];
    if (!ms.active || m == e) continue;
    float sum = 0.0f;
    for (int i = 0; i < ms.n_odds; ++i) sum += ms.odds[i];
    bool listed = sum <= std::numeric_limits<float>::epsilon() && e < ms.n_speakers;
    for (int i = 0; i < ms.n_odds; ++i) listed = listed || (ms.order[i] == e && ms.odds[i] > 0.0f);
    if (listed && entry_named(b, m)) return true;
  }
  return false;
}
// The opening of every BeatriceBatch_* entry point: the batch's device for the call's duration, -2 for a missing or unhealthy batch; then
// -1 for what the batch's mode refuses (batch_modes.h), before anything is drained, synchronised, bound or written.
#define BATCH_OPEN(b) const DeviceScope dev_((b) ? (b)->device : -1); if (!(b) || !(b)->ok) return -2
#define BATCH_GATE(b, entry) if (!modes::allowed(entry, flags_of(b))) return -1
#define BATCH_ENTER(b, entry) BATCH_OPEN(b); BATCH_GATE(b, entry)

template <class F>
int for_streams(BeatriceBatch* b, int stream, F f) {
  BATCH_OPEN(b);
  if (stream < -1 || stream >= b->B) return -1;
  const int lo = stream < 0 ? 0 : stream, hi = stream < 0 ? b->B : stream + 1;
  for (int s = lo; s < hi; ++s) { f(b->cfg[s]); sync_stream_arrays(b, s); }
  return 0;
}

int midi_to_bin(double note) {
  // reference processor_core_2.cc:561-583: clamp note to [0,128], bin = round((note-33)*8), clamp 1..447
  note = std::min(std::max(note, 0.0), 128.0);
  const int q = (int)std::round((note - 33.0) * (BEATRICE_PITCH_BINS_PER_OCTAVE / 12.0));
  return std::min(std::max(q, 1), B_PITCH_BINS - 1);
}

}  // namespace

// ---- device-resident parameter blobs (multi-GPU load) ------------------------
// Rank 0 reads and packs a model file once; the other ranks allocate an empty blob of the same size, the caller
// broadcasts device memory to device memory (RCCL over xGMI) and marks the model ready: what travels is exactly
// what the kernels read (MFMA-fragment order), no host round trip and no repacking on the receivers.
namespace {
template <class Model, class Weights>
int model_blob(Model* m, int allocate, void** d_ptr, size_t* n_bytes) {
  if (!m || !d_ptr || !n_bytes) return -1;
  const DeviceScope dev_(m->device);
  const size_t n = Weights::n_floats();
  if (allocate && !m->loaded && m->blob.n_floats != n) {
    if (!m->blob.alloc(n)) return -2;
  }
  if (!m->blob.d || m->blob.n_floats != n) return -1;
  *d_ptr = m->blob.d;
  *n_bytes = n * sizeof(float);
  return 0;
}
template <class Model>
int model_ready(Model* m) {
  if (!m || !m->blob.d) return -1;
  const DeviceScope dev_(m->device);
  if (!hip_ok(hipDeviceSynchronize(), "blob ready")) return -2;
  m->w.bind(m->blob.d);
  m->loaded = true;
  return 0;
}
}  // namespace

extern "C" {
static bool rb_step(BeatriceBatch* b, bool synthetic = false);

// ---- memory loaders ---------------------------------------------------------------------------
#define BHIP_MEMORY_LOADER(Name, Obj, KIND, Weights)                                                        \
  Beatrice_ErrorCode BeatriceHip_Load##Name##FromMemory(Obj* m, const void* bytes, size_t size) {           \
    std::vector<float> host;                                                                                \
    const Beatrice_ErrorCode e = parse_model_bytes(static_cast<const unsigned char*>(bytes), size, KIND,   \
                                                   (long)Weights::n_floats(), &host);                       \
    if (e) return e;                                                                                        \
    const DeviceScope dev_(m->device);                                                                      \
    m->loaded = false;                                                                                      \
    Weights::pack_host(host.data());                                                                        \
    if (!m->blob.upload(host.data(), host.size())) return Beatrice_kFileOpenError;                          \
    m->w.bind(m->blob.d);                                                                                   \
    m->loaded = true;                                                                                       \
    return Beatrice_kSuccess;                                                                               \
  }
BHIP_MEMORY_LOADER(PhoneExtractor, Beatrice20rc0_PhoneExtractor, KIND_PHONE, PhoneWeights)
BHIP_MEMORY_LOADER(PitchEstimator, Beatrice20rc0_PitchEstimator, KIND_PITCH, PitchWeights)
BHIP_MEMORY_LOADER(WaveformGenerator, Beatrice20rc0_WaveformGenerator, KIND_WAVE, WaveWeights)
BHIP_MEMORY_LOADER(EmbeddingSetter, Beatrice20rc0_EmbeddingSetter, KIND_EMBED, EmbedWeights)

int BeatriceHip_SetDevice(int ordinal) {
  int n = 0;
  if (ordinal < -1 || (ordinal >= 0 && (hipGetDeviceCount(&n) != hipSuccess || ordinal >= n))) return -1;
  set_target_device(ordinal);
  return 0;
}
int BeatriceHip_GetDevice(void) { return target_device(); }
int BeatriceBatch_Device(const BeatriceBatch* b) { return b ? b->device : -1; }

int BeatriceHip_ModelBlob(int kind, void* model, int allocate, void** d_ptr, size_t* n_bytes) {
  switch (kind) {
    case KIND_PHONE: return model_blob<Beatrice20rc0_PhoneExtractor, PhoneWeights>(static_cast<Beatrice20rc0_PhoneExtractor*>(model), allocate, d_ptr, n_bytes);
    case KIND_PITCH: return model_blob<Beatrice20rc0_PitchEstimator, PitchWeights>(static_cast<Beatrice20rc0_PitchEstimator*>(model), allocate, d_ptr, n_bytes);
    case KIND_WAVE: return model_blob<Beatrice20rc0_WaveformGenerator, WaveWeights>(static_cast<Beatrice20rc0_WaveformGenerator*>(model), allocate, d_ptr, n_bytes);
    case KIND_EMBED: return model_blob<Beatrice20rc0_EmbeddingSetter, EmbedWeights>(static_cast<Beatrice20rc0_EmbeddingSetter*>(model), allocate, d_ptr, n_bytes);
    default: return -1;
  }
}
int BeatriceHip_ModelBlobReady(int kind, void* model) {
  switch (kind) {
    case KIND_PHONE: return model_ready(static_cast<Beatrice20rc0_PhoneExtractor*>(model));
    case KIND_PITCH: return model_ready(static_cast<Beatrice20rc0_PitchEstimator*>(model));
    case KIND_WAVE: return model_ready(static_cast<Beatrice20rc0_WaveformGenerator*>(model));
    case KIND_EMBED: return model_ready(static_cast<Beatrice20rc0_EmbeddingSetter*>(model));
    default: return -1;
  }
}

// ---- lifecycle ----------------------------------------------------------------------------------
BeatriceBatch* BeatriceBatch_Create(const Beatrice20rc0_PhoneExtractor* phone, const Beatrice20rc0_PitchEstimator* pitch,
                                    const Beatrice20rc0_WaveformGenerator* wave, const Beatrice20rc0_EmbeddingSetter* embed,
                                    int n_streams, int max_speakers) {
  return BeatriceBatch_CreateBlock(phone, pitch, wave, embed, n_streams, max_speakers, 1);
}

BeatriceBatch* BeatriceBatch_CreateBlock(const Beatrice20rc0_PhoneExtractor* phone, const Beatrice20rc0_PitchEstimator* pitch,
                                         const Beatrice20rc0_WaveformGenerator* wave, const Beatrice20rc0_EmbeddingSetter* embed,
                                         int n_streams, int max_speakers, int hops_per_step) {
  auto* b = new BeatriceBatch();
  if (!phone || !pitch || !wave || !embed || !phone->loaded || !pitch->loaded || !wave->loaded || !embed->loaded ||
      n_streams < 1 || max_speakers < 1 || (hops_per_step != 1 && hops_per_step != 2 && hops_per_step != 4 && hops_per_step != 8))
    return b;  // unhealthy object; every call on it fails with -2
  if (pitch->device != phone->device || wave->device != phone->device || embed->device != phone->device) return b;  // one GPU per batch
  b->device = phone->device;
  const DeviceScope dev_(b->device);
  b->phone_m = phone; b->pitch_m = pitch; b->wave_m = wave; b->embed_m = embed;
  b->B = n_streams; b->max_speakers = max_speakers; b->H = hops_per_step;
  const int B = n_streams, S = max_speakers, H = hops_per_step;
  bool ok = make_stage_stream(b->stream_own, 0);
  b->stream = b->stream_own;
  ok = ok && b->d_in.alloc((size_t)B * H * B_IN_HOP, "d_in");
  // the front end's outputs (phone vector, conditioning mix) have three step slots: see `pipelined`
  const bool slack = H <= tick::kMaxHops;  // rings sized so that every layer can be its own pipeline stage (tick.hip.h)
  ok = ok && b->phone.create(B, H, b->d_in, 3, slack) && b->pitch.create(B, H, b->d_in, true, slack) &&
       b->wave.create(B, H, S, S, 9, b->phone.d_phone, b->pitch.d_q, b->pitch.d_feat, 3, slack);
  b->wave.q_slots = b->pitch.q_slots;
  // The modules advance in lockstep: one step counter, with no launch spent on incrementing it.  The step's
  // first kernels (phone.f1, pitch.fft) read the pair {counter, I/O slot} from d_hop_next; phone.f1 publishes
  // it to phone.d_hop for the rest of the front end and to d_hop_wave[counter & 1] for the waveform generator
  // (which may lag one step behind); the front end's last body (wave.cond) stores the next pair to d_hop_next.
  ok = ok && b->d_hop_next.alloc(2, "hop_next") && b->d_hop_wave.alloc(8, "hop_wave");
  b->pitch.hop = b->phone.d_hop; b->wave.hop = b->d_hop_wave;
  b->phone.hop_in = b->d_hop_next; b->pitch.hop_in = b->d_hop_next;
  b->phone.hop_publish = b->phone.d_hop; b->phone.hop_publish_wave = b->d_hop_wave;
  b->wave.front_hop = b->phone.d_hop; b->wave.front_next_out = b->d_hop_next;
  b->phone.advance_hop = false; b->pitch.advance_hop = false; b->wave.advance_hop = false;
  for (int s = 0; s < BeatriceBatch::kMaxStages && ok; ++s) {  // (stage streams are created when a pipeline depth asks for them)
    for (int k = 0; k < BeatriceBatch::kSlots && ok; ++k) ok = b->ev_done[s][k].create("ev");
  }
  set_plan(b, 1);
  const size_t cbf = (size_t)S * B_CODEBOOK * B_PHONE_CH, kvf = (size_t)S * B_KV_LEN * B_KV_CH;
  // (zeroed: entries the caller never fills -- a morph entry's codebook, speakers added later -- project to zeros, not to garbage)
  ok = ok && b->d_cb_raw.alloc(cbf, "cb") && b->d_cbT.alloc(cbf, "cbT") && b->d_cnorm.alloc((size_t)S * B_CODEBOOK, "cnorm") &&
       b->d_add_raw.alloc((size_t)S * B_HID, "add") && b->d_frm_raw.alloc((size_t)9 * B_HID, "frm") && b->d_kv_raw.alloc(kvf, "kv");
  b->cfg.assign(B, StreamCfg());
  b->morph.assign(S, MorphSlot());
  b->entries.start(B, S, BeatriceBatch::kNamed);   // (StreamCfg's defaults: every stream on entry 0)
  b->lottery.resize(B);
  for (int s = 0; s < B; ++s) b->lottery[s].seed(5489u + (unsigned)s);
  {  // layout of the settings block (256-byte aligned arrays)
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    const size_t nt = ok ? (size_t)b->wave.n_tiles_max : 1;
    b->off.cbT = take(sizeof(float*) * B * H); b->off.cnorm = take(sizeof(float*) * B * H); b->off.vqk = take(sizeof(int) * B);
    // (grouped by consumer: k-NN | pitch head | conditioning mix -- tick mode copies a consumer's range as one piece)
    b->off.min_q = take(sizeof(int) * B); b->off.max_q = take(sizeof(int) * B); b->off.params = take(sizeof(PitchParams) * B);
    b->off.add_idx = take(sizeof(int) * B); b->off.frm_idx = take(sizeof(int) * B);
    b->off.front_bytes = o;
    for (int blk = 0; blk < B_NBLOCKS; ++blk) {
      b->off.perm[blk] = take(sizeof(int) * nt * 16); b->off.tile_slot[blk] = take(sizeof(int) * nt);
      // tick mode: the same rows as quads of <= 4 rows per K/V slot, four quads to a tile (rowchain.hip.h block_b_body)
      b->off.qperm[blk] = take(sizeof(int) * nt * 16); b->off.qslot[blk] = take(sizeof(int) * nt * 4);
    }
    b->off.wave_bytes = o - b->off.front_bytes;
  }
  const size_t dev_bytes = b->off.front_bytes + BeatriceBatch::kSlots * b->off.wave_bytes;
  ok = ok && b->settings.alloc(b->off.front_bytes + b->off.wave_bytes, dev_bytes, "settings", true);
  if (ok) {  // the kernels read the block instead of the modules' own arrays
    void** keep = b->module_owned;
    auto swap_in = [&keep](auto*& member, auto* view) { *keep++ = (void*)member; member = view; };
    swap_in(b->phone.d_cbT, b->dev_view<const float*>(b->off.cbT));
    swap_in(b->phone.d_cnorm, b->dev_view<const float*>(b->off.cnorm));
    swap_in(b->phone.d_vqk, b->dev_view<int>(b->off.vqk));
    swap_in(b->pitch.d_min_q, b->dev_view<int>(b->off.min_q));
    swap_in(b->pitch.d_max_q, b->dev_view<int>(b->off.max_q));
    swap_in(b->pitch.d_params, b->dev_view<PitchParams>(b->off.params));
    swap_in(b->wave.d_add_idx, b->dev_view<int>(b->off.add_idx));
    swap_in(b->wave.d_frm_idx, b->dev_view<int>(b->off.frm_idx));
    for (int blk = 0; blk < B_NBLOCKS; ++blk) {
      swap_in(b->wave.d_perm[blk], b->dev_view<int>(b->off.perm[blk]));
      swap_in(b->wave.d_tile_slot[blk], b->dev_view<int>(b->off.tile_slot[blk]));
    }
  }
  ok = ok && b->h_in.alloc((size_t)B * H * B_IN_HOP, "h_in") && b->h_out.alloc((size_t)B * H * B_OUT_HOP, "h_out") &&
       b->ev0.create("ev0", true) && b->ev1.create("ev1", true);
  {  // 48 kHz wrapper: 33-entry Hann-windowed sinc tables of the ratio-1/1 resampler pair
    //   (reference resample.h:209-230 with cutoffs 0.99*16000/48000 in, 0.99*24000/48000 out, :412-417)
    float cd[33], cu[33];
    const double pi = 3.14159265358979323846, cut_d = 0.99 * 16000.0 / 48000.0, cut_u = 0.99 * 24000.0 / 48000.0;
    auto sinc = [&](double x) { return std::abs(x) < 1e-8 ? 1.0 : std::sin(x * pi) / (x * pi); };
    for (int i = 0; i < 33; ++i) {
      const double x = static_cast<double>(i - 16) / 1.0;
      const double hann = 0.5 - 0.5 * std::cos(pi * 2.0 / 32.0 * static_cast<double>(i));
      cd[i] = static_cast<float>(cut_d * sinc(x * cut_d) * hann);
      cu[i] = static_cast<float>(cut_u * sinc(x * cut_u) * hann);
    }
    ok = ok && b->d_w48.alloc(B, "w48") && b->d_coef_down.alloc(33, "cd", false) && b->d_coef_up.alloc(33, "cu", false) &&
         hip_ok(hipMemcpy(b->d_coef_down, cd, sizeof(cd), hipMemcpyHostToDevice), "cd up") &&
         hip_ok(hipMemcpy(b->d_coef_up, cu, sizeof(cu), hipMemcpyHostToDevice), "cu up") &&
         b->d_io48.alloc((size_t)B * 4 * 480, "io48", false) && b->h_io48.alloc((size_t)B * 4 * 480, "hio48");
  }
  ok = ok && hip_ok(hipDeviceSynchronize(), "create sync");  // NULL-stream memsets vs the non-blocking stream
  b->ok = ok;
  if (ok) {
    for (int blk = 0; blk < B_NBLOCKS; ++blk) b->row_slot[blk].assign((size_t)B * H, 0);
    for (int s = 0; s < B; ++s) { sync_stream_arrays(b, s); fill_row_slots(b, s); }
    for (int blk = 0; blk < B_NBLOCKS; ++blk) rebuild_tiles(b, blk);
    std::vector<sblob::RingShape> shapes;
    for (const RingArena* a : {&b->phone.arena, &b->pitch.arena, &b->wave.arena})
      for (const Ring* r : a->rings) shapes.push_back(sblob::RingShape{r->C, r->n, r->m});
    b->sb.layout = sblob::make_layout(H, shapes.data(), (int)shapes.size(), (uint32_t)sizeof(StreamCfg), (uint32_t)sizeof(Wrap48State));
  }
  return b;
}

void BeatriceBatch_Destroy(BeatriceBatch* b) {
  const DeviceScope dev_(b ? b->device : -1);
  if (!b) return;
  if (b->stream) (void)sync_all(b);
  b->scan.settle();
  drop_graph(b);
  if (b->own_d_out) { b->wave.d_out = b->own_d_out; b->own_d_out = nullptr; }
  if (b->io_mapped) { b->wave.d_out = b->dev_d_out; b->phone.d_in = b->pitch.d_in = b->d_in; b->io_mapped = false; }  // (the modules free what they allocated)
  if (b->module_owned[0]) {  // hand the modules their own arrays back so that destroy() frees what it allocated
    void** keep = b->module_owned;
    auto swap_out = [&keep](auto*& member) { member = static_cast<std::remove_reference_t<decltype(member)>>(*keep++); };
    swap_out(b->phone.d_cbT); swap_out(b->phone.d_cnorm); swap_out(b->phone.d_vqk);
    swap_out(b->pitch.d_min_q); swap_out(b->pitch.d_max_q); swap_out(b->pitch.d_params);
    swap_out(b->wave.d_add_idx); swap_out(b->wave.d_frm_idx);
    for (int blk = 0; blk < B_NBLOCKS; ++blk) { swap_out(b->wave.d_perm[blk]); swap_out(b->wave.d_tile_slot[blk]); }
  }
  b->phone.destroy(); b->pitch.destroy(); b->wave.destroy();
  delete b;   // (everything the batch owns is freed here: synchronised, and with its device still current)
}

int BeatriceBatch_IsHealthy(const BeatriceBatch* b) { return b && b->ok ? 1 : 0; }
int BeatriceBatch_NumStreams(const BeatriceBatch* b) { return b ? b->B : 0; }
int BeatriceBatch_HopsPerStep(const BeatriceBatch* b) { return b ? b->H : 0; }
size_t BeatriceBatch_StateBytes(const BeatriceBatch* b) {
  const DeviceScope dev_(b ? b->device : -1);
  return b && b->ok ? sizeof(float) * (b->phone.arena.floats + b->pitch.arena.floats + b->wave.arena.floats) : 0;
}

// ---- speaker tables -----------------------------------------------------------------------------
namespace {
bool project_speakers(BeatriceBatch* b, int first, int count) {
  hipStream_t s = b->stream;
  const EmbedWeights& w = b->embed_m->w;
  codebook_prepare(b->d_cb_raw + (size_t)first * B_CODEBOOK * B_PHONE_CH, count,
                   b->d_cbT + (size_t)first * B_PHONE_CH * B_CODEBOOK, b->d_cnorm + (size_t)first * B_CODEBOOK, s);
  embed_project_rows(w.add_w, w.add_b, b->d_add_raw + (size_t)first * B_HID, b->wave.d_add_tab + (size_t)first * B_HID, count, s);
  for (int blk = 0; blk < B_NBLOCKS; ++blk)
    embed_project_kv(w, blk, b->d_kv_raw + (size_t)first * B_KV_LEN * B_KV_CH, count,
                     b->wave.d_kt[blk] + (size_t)first * B_HID * B_KV_LEN, b->wave.d_v[blk] + (size_t)first * B_KV_LEN * B_HID, s,
                     b->wave.d_ktp[blk] ? b->wave.d_ktp[blk] + (size_t)first * B_HID * B_KV_LEN : nullptr,
                     b->wave.d_vp[blk] ? b->wave.d_vp[blk] + (size_t)first * B_KV_LEN * B_HID : nullptr);
  return hip_ok(hipStreamSynchronize(s), "project speakers");
}
}  // namespace

int BeatriceBatch_SetSpeakerTables(BeatriceBatch* b, int n, const float* codebooks, const float* additive, const float* formant,
                                   const float* kv) {
  BATCH_OPEN(b);
  if (n < 1 || n > b->max_speakers || !codebooks || !additive || !formant || !kv) return -1;
  bool ok = sync_all(b) &&
            hip_ok(hipMemcpy(b->d_cb_raw, codebooks, sizeof(float) * n * B_CODEBOOK * B_PHONE_CH, hipMemcpyHostToDevice), "cb") &&
            hip_ok(hipMemcpy(b->d_add_raw, additive, sizeof(float) * n * B_HID, hipMemcpyHostToDevice), "add") &&
            hip_ok(hipMemcpy(b->d_frm_raw, formant, sizeof(float) * 9 * B_HID, hipMemcpyHostToDevice), "frm") &&
            hip_ok(hipMemcpy(b->d_kv_raw, kv, sizeof(float) * n * B_KV_LEN * B_KV_CH, hipMemcpyHostToDevice), "kv");
  if (!ok || !hip_ok(hipDeviceSynchronize(), "tables sync")) return -2;
  b->n_speakers = n;
  for (MorphSlot& m : b->morph) m.active = false;
  b->n_morph_slots = 0;
  const EmbedWeights& w = b->embed_m->w;
  embed_project_rows(w.frm_w, w.frm_b, b->d_frm_raw, b->wave.d_frm_tab, 9, b->stream);
  return project_speakers(b, 0, n) ? 0 : -2;
}

// The four raw tables as they sit on the device, for callers that fill them device-to-device (a broadcast from the
// rank that read the file): [0] codebooks [S][512][128], [1] additive [S][256], [2] formant [9][256], [3] key/value
// [S][384][128]; then BeatriceBatch_ProjectSpeakerTables(b, n) does what SetSpeakerTables does after its upload.
int BeatriceBatch_SpeakerTablesDevice(BeatriceBatch* b, void** d_ptrs, size_t* n_bytes) {
  BATCH_OPEN(b);
  if (!d_ptrs || !n_bytes) return -1;
  const size_t S = (size_t)b->max_speakers;
  d_ptrs[0] = b->d_cb_raw; n_bytes[0] = sizeof(float) * S * B_CODEBOOK * B_PHONE_CH;
  d_ptrs[1] = b->d_add_raw; n_bytes[1] = sizeof(float) * S * B_HID;
  d_ptrs[2] = b->d_frm_raw; n_bytes[2] = sizeof(float) * 9 * B_HID;
  d_ptrs[3] = b->d_kv_raw; n_bytes[3] = sizeof(float) * S * B_KV_LEN * B_KV_CH;
  return 0;
}
int BeatriceBatch_ProjectSpeakerTables(BeatriceBatch* b, int n) {
  BATCH_OPEN(b);
  if (n < 1 || n > b->max_speakers) return -1;
  if (!sync_all(b) || !hip_ok(hipDeviceSynchronize(), "tables sync")) return -2;
  b->n_speakers = n;
  for (MorphSlot& m : b->morph) m.active = false;
  b->n_morph_slots = 0;
  const EmbedWeights& w = b->embed_m->w;
  embed_project_rows(w.frm_w, w.frm_b, b->d_frm_raw, b->wave.d_frm_tab, 9, b->stream);
  return project_speakers(b, 0, n) ? 0 : -2;
}

int BeatriceBatch_UpdateSpeaker(BeatriceBatch* b, int spk, const float* codebook, const float* additive, const float* kv) {
  BATCH_OPEN(b);
  if (spk < 0 || spk >= b->max_speakers) return -1;
  bool ok = sync_all(b);
  if (codebook) ok = ok && hip_ok(hipMemcpy(b->d_cb_raw + (size_t)spk * B_CODEBOOK * B_PHONE_CH, codebook, sizeof(float) * B_CODEBOOK * B_PHONE_CH, hipMemcpyHostToDevice), "cb1");
  if (additive) ok = ok && hip_ok(hipMemcpy(b->d_add_raw + (size_t)spk * B_HID, additive, sizeof(float) * B_HID, hipMemcpyHostToDevice), "add1");
  if (kv) ok = ok && hip_ok(hipMemcpy(b->d_kv_raw + (size_t)spk * B_KV_LEN * B_KV_CH, kv, sizeof(float) * B_KV_LEN * B_KV_CH, hipMemcpyHostToDevice), "kv1");
  if (!ok || !hip_ok(hipDeviceSynchronize(), "speaker sync")) return -2;
  if (spk >= b->n_speakers) b->n_speakers = spk + 1;
  if (b->morph[spk].active) { b->morph[spk].active = false; --b->n_morph_slots; }  // the caller's data replaces a morph
  return project_speakers(b, spk, 1) ? 0 : -2;
}

// ---- speaker morphing ----------------------------------------------------------------------------
// Weight preparation as the reference host does it (voice_morph_state.h:87-104: entries below 0.01
// dropped; processor_core_2.cc:507-532: the eight largest kept, in descending order), then the additive
// and the 384 key/value embeddings of entry `slot` become weighted spherical means computed on the
// device (morph.hip), and their projections are refreshed.
struct MorphPlan { MorphDesc desc; MorphSlot slot; };
static MorphPlan plan_morph(int slot, const float* weights, int n_weights) {
  std::vector<float> w(weights, weights + n_weights);
  for (float& v : w) if (v < 0.01f) v = 0.0f;
  std::vector<int> order(n_weights);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&w](const int x, const int y) -> bool { return w[x] > w[y]; });
  const int keep = std::min(n_weights, 8);
  // SphericalAverage::SetWeights (spherical_average.h:142-199): points in `order` until the first zero weight
  MorphPlan p{};
  int& n_active = p.desc.n_active;
  int* spk = p.desc.speaker;
  float* wn = p.desc.weight;
  float sum = 0.0f;
  for (int i = 0; i < keep; ++i) {
    if (w[order[i]] == 0.0f) break;
    spk[n_active] = order[i]; wn[n_active] = w[order[i]]; ++n_active;
  }
  for (int i = 0; i < n_active; ++i) sum += wn[i];
  if (n_active > 0 && sum > 0.0f) { const float inv = 1.0f / sum; for (int i = 0; i < n_active; ++i) wn[i] *= inv; }
  else n_active = 0;
  p.desc.slot = slot;
  p.slot.active = true;
  p.slot.n_speakers = n_weights;
  p.slot.n_odds = keep;
  for (int i = 0; i < 8; ++i) { p.slot.order[i] = i < keep ? order[i] : 0; p.slot.odds[i] = i < keep ? w[order[i]] : 0.0f; }
  return p;
}
// entry p.desc.slot now holds the morph: what the lottery needs, and the engines' one seeding
static void adopt_morph(BeatriceBatch* b, const MorphPlan& p, unsigned seed) {
  const int slot = p.desc.slot;
  if (slot >= b->n_speakers) b->n_speakers = slot + 1;
  if (!b->morph[slot].active) ++b->n_morph_slots;
  b->morph[slot] = p.slot;
  // The engines are seeded ONCE per batch, as the reference seeds its engine once per instance (processor_core_2.h:48,145) and
  // never again when morph weights move (:94-121): only the first morph of the batch's life applies `seed`; a caller that
  // moves weights every step keeps each stream's draw SEQUENCE running, and a morph on one entry leaves the draws of the
  // streams on other entries alone.  BeatriceBatch_SeedLottery re-seeds explicitly.
  if (!b->lottery_seeded) {
    for (int st = 0; st < b->B; ++st) b->lottery[st].seed(seed + (unsigned)st);
    b->lottery_seeded = true;
  }
}
static bool morph_weights_ok(const BeatriceBatch* b, const float* weights, int n_weights) {
  return weights && n_weights >= 1 && n_weights <= 256 && n_weights <= b->n_speakers;
}
static int morph_into(BeatriceBatch* b, int slot, const float* weights, int n_weights, unsigned seed) {
  if (!morph_weights_ok(b, weights, n_weights) || slot < n_weights || slot >= b->max_speakers) return -1;
  const MorphPlan p = plan_morph(slot, weights, n_weights);
  const MorphDesc& d = p.desc;
  bool ok = sync_all(b);
  ok = ok && spherical_mean_rows(b->d_add_raw, B_HID, 1, B_HID, d.n_active, d.speaker, d.weight, b->d_add_raw + (size_t)slot * B_HID, b->stream);
  ok = ok && spherical_mean_rows(b->d_kv_raw, (size_t)B_KV_LEN * B_KV_CH, B_KV_LEN, B_KV_CH, d.n_active, d.speaker, d.weight,
                                 b->d_kv_raw + (size_t)slot * B_KV_LEN * B_KV_CH, b->stream);
  if (!ok) return -2;
  if (slot >= b->n_speakers) b->n_speakers = slot + 1;
  if (!project_speakers(b, slot, 1)) return -2;
  adopt_morph(b, p, seed);
  return 0;
}
int BeatriceBatch_MorphSpeaker(BeatriceBatch* b, int slot, const float* weights, int n_weights, unsigned seed) {
  BATCH_OPEN(b);
  if (const int rc = morph_into(b, slot, weights, n_weights, seed)) return rc;
  // streams already on this entry re-install its key/value blocks, one per hop, like after a speaker switch
  for (StreamCfg& c : b->cfg) if (c.target_speaker == slot) { c.kv_set_count = 0; c.kv_delay = 0; }
  b->pending_kv = 0;
  for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++b->pending_kv;
  return 0;
}
// The reference's timeline of a weight change for streams that are ALREADY morphing (processor_core_2.cc:51-177): on the next
// hop h0 the new additive embedding is in force and the codebook lottery draws with the new odds; the key/value means are
// computed a quarter per hop over h0 .. h0+3 while the OLD key/value blocks keep playing; at h0+4 the new embeddings are
// registered and installed one block per hop, h0+4 .. h0+7.  In place that cannot be done (BeatriceBatch_MorphSpeaker
// overwrites the entry every stream on it is reading), so the new morph goes into ANOTHER table entry `slot` and the streams
// on `from_slot` move over: additive embedding and lottery at once, key/value blocks after four hops.  `slot` must not be an
// entry whose key/value blocks some stream still has installed (-3: use a third entry, as a caller that moves the weights
// faster than every eight hops needs anyway -- the reference never installs new blocks while the weights keep moving, and
// neither do streams here: each call restarts their four-hop wait).
int BeatriceBatch_MorphSpeakerStaged(BeatriceBatch* b, int slot, int from_slot, const float* weights, int n_weights, unsigned seed) {
  BATCH_OPEN(b);
  if (from_slot < 0 || from_slot >= b->max_speakers || from_slot == slot) return -1;
  if (slot >= 0 && slot < b->max_speakers)
    for (const StreamCfg& c : b->cfg) {
      for (int blk = 0; blk < B_NBLOCKS; ++blk) if (c.kv_slot[blk] == slot) return -3;
      // ... or is on its way there: installs still pending from an earlier staged call, or a stream that took `slot` by
      // another route (its additive row and key/value tables would be overwritten under it)
      if (c.target_speaker == slot || c.additive_speaker == slot) return -3;
    }
  if (const int rc = morph_into(b, slot, weights, n_weights, seed)) return rc;
  for (int s = 0; s < b->B; ++s) {
    StreamCfg& c = b->cfg[s];
    if (c.target_speaker != from_slot) continue;
    c.target_speaker = slot;
    c.additive_speaker = slot;
    c.kv_set_count = 0;
    c.kv_delay = 4;
    sync_stream_arrays(b, s);
  }
  b->pending_kv = 0;
  for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++b->pending_kv;
  return 0;
}
// Many entries in one call, and in tick mode and every mode around it (D, E, F, G, P) WITHOUT the drain (beatrice_batch.h): the entries
// are refused while anything still reads them (entry_busy), so their tables may be rewritten between two ticks -- two launches on the
// batch's stream in front of the next tick (morph.hip: all solves, all projections), the descriptors in a pinned ring because the host
// runs ahead.  The wrapper launches of F, G and P ride on the same stream and read no speaker table.
int BeatriceBatch_MorphSpeakersInFlight(BeatriceBatch* b, int n, const int* slots, const int* from_slots, const float* weights, int n_weights,
                                        unsigned seed) {
  BATCH_OPEN(b);
  const int S = b->max_speakers;
  if (n < 1 || n > S || !slots || !from_slots || !morph_weights_ok(b, weights, n_weights)) return -1;
  std::vector<char> is_slot(S, 0), is_from(S, 0);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < n_weights || slots[i] >= S || is_slot[slots[i]]) return -1;
    is_slot[slots[i]] = 1;
  }
  for (int i = 0; i < n; ++i) {
    const int f = from_slots[i];
    if (f == -1) continue;
    if (f < 0 || f >= S || is_slot[f] || is_from[f]) return -1;   // (is_slot: its own slot, or another pair's)
    is_from[f] = 1;
  }
  for (int i = 0; i < n; ++i) if (entry_busy(b, slots[i])) return -3;
  const bool in_flight = sentry::rule_b_applies(modes::mode_of(flags_of(b)));   // (D, E, F, G, P: entry_busy has asked rule (b))
  if (!b->morph_descs.entries() && !b->morph_descs.alloc(BeatriceBatch::kMorphStaging, (size_t)S, "morph descriptors")) return -2;
  if (!in_flight && !sync_all(b)) return -2;
  const int ring = (int)(b->morph_calls % BeatriceBatch::kMorphStaging);
  MorphDesc* descs = b->morph_descs.claim(ring);
  if (!descs) return -2;
  std::vector<MorphPlan> plans(n);
  for (int i = 0; i < n; ++i) {
    plans[i] = plan_morph(slots[i], weights + (size_t)i * n_weights, n_weights);
    descs[i] = plans[i].desc;
  }
  const EmbedWeights& w = b->embed_m->w;
  MorphProjectArgs pa{};
  pa.descs = descs; pa.n = n; pa.n_entries = S;
  pa.add_raw = b->d_add_raw; pa.kv_raw = b->d_kv_raw; pa.add_w = w.add_w; pa.add_b = w.add_b; pa.add_tab = b->wave.d_add_tab;
  for (int blk = 0; blk < B_NBLOCKS; ++blk) {
    pa.k_w[blk] = w.k_w[blk]; pa.k_b[blk] = w.k_b[blk]; pa.v_w[blk] = w.v_w[blk]; pa.v_b[blk] = w.v_b[blk];
    pa.kt[blk] = b->wave.d_kt[blk]; pa.v[blk] = b->wave.d_v[blk]; pa.kt_plain[blk] = b->wave.d_ktp[blk]; pa.v_plain[blk] = b->wave.d_vp[blk];
  }
  bool ok = spherical_mean_entries(descs, n, S, b->d_add_raw, b->d_kv_raw, b->stream) && morph_project_entries(pa, b->stream);
  ok = b->morph_descs.mark(ring, b->stream) && ok;
  b->morph_calls += 1;
  if (!in_flight) ok = hip_ok(hipStreamSynchronize(b->stream), "morph entries") && ok;
  if (!ok) return -2;
  for (const MorphPlan& p : plans) adopt_morph(b, p, seed);
  for (int s = 0; s < b->B; ++s) {   // the streams on a from_slot move over, on BeatriceBatch_MorphSpeakerStaged's timeline
    StreamCfg& c = b->cfg[s];
    if (!is_from[c.target_speaker]) continue;
    int to = -1;
    for (int i = 0; i < n && to < 0; ++i) if (from_slots[i] == c.target_speaker) to = slots[i];
    c.target_speaker = to;
    c.additive_speaker = to;
    c.kv_set_count = 0;
    c.kv_delay = 4;
    sync_stream_arrays(b, s);
  }
  b->pending_kv = 0;
  for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++b->pending_kv;
  return 0;
}
int BeatriceBatch_SpeakerEntryBusy(const BeatriceBatch* b, int entry) {
  if (!b || !b->ok || entry < 0 || entry >= b->max_speakers) return -1;
  return entry_busy(b, entry) ? 1 : 0;
}
// BeatriceBatch_UpdateSpeaker for n entries in one call, and in D, E, F, G and P without the drain, on the same terms
// as the morph call above: entries nothing reads (entry_busy) are rewritten between two ticks by two launches on the batch's stream.  The
// caller's tables are copied into a pinned ring entry here, on the calling thread; install_entries_kernel (install.hip) reads them in
// place and writes the raw tables, the transposed codebooks and their norms, morph_project_kernel (morph.hip) projects the rest.
int BeatriceBatch_MaxInstallEntries(const BeatriceBatch* b) { return b ? std::min(BeatriceBatch::kInstallEntries, b->max_speakers) : 0; }
int BeatriceBatch_InstallSpeakersInFlight(BeatriceBatch* b, int n, const int* entries, const float* codebooks, const float* additive,
                                          const float* key_value) {
  BATCH_OPEN(b);
  const int S = b->max_speakers, cap = BeatriceBatch_MaxInstallEntries(b);
  if (n < 1 || n > cap || !entries || !codebooks || !additive || !key_value) return -1;
  std::vector<char> is_entry(S, 0);
  for (int i = 0; i < n; ++i) {
    if (entries[i] < 0 || entries[i] >= S || is_entry[entries[i]]) return -1;
    is_entry[entries[i]] = 1;
  }
  for (int i = 0; i < n; ++i) if (entry_busy(b, entries[i])) return -3;
  const bool in_flight = sentry::rule_b_applies(modes::mode_of(flags_of(b)));   // (D, E, F, G, P: entry_busy has asked rule (b))
  if (!b->install_tables.entries()) {
    StagedRing<float> tables;
    PinnedBuf<MorphDesc> descs;
    if (!tables.alloc(BeatriceBatch::kInstallStaging, (size_t)cap * kInstallEntryFloats, "install staging") ||
        !descs.alloc((size_t)BeatriceBatch::kInstallStaging * cap, "install descriptors")) return -2;
    b->install_tables = std::move(tables); b->install_descs = std::move(descs);
  }
  if (!in_flight && !sync_all(b)) return -2;
  // (the ring entry of kInstallStaging calls ago: a wait only if the device is that many installs behind the host)
  const int ring = (int)(b->install_calls % BeatriceBatch::kInstallStaging);
  float* staged = b->install_tables.claim(ring);
  if (!staged) return -2;
  MorphDesc* descs = b->install_descs + (size_t)ring * cap;
  constexpr size_t n_cb = (size_t)B_CODEBOOK * B_PHONE_CH, n_kv = (size_t)B_KV_LEN * B_KV_CH;
  for (int i = 0; i < n; ++i) {
    float* dst = staged + (size_t)i * kInstallEntryFloats;
    std::memcpy(dst, codebooks + (size_t)i * n_cb, sizeof(float) * n_cb);
    std::memcpy(dst + n_cb, additive + (size_t)i * B_HID, sizeof(float) * B_HID);
    std::memcpy(dst + n_cb + B_HID, key_value + (size_t)i * n_kv, sizeof(float) * n_kv);
    descs[i] = MorphDesc{};
    descs[i].slot = entries[i];
  }
  const EmbedWeights& w = b->embed_m->w;
  MorphProjectArgs pa{};
  pa.descs = descs; pa.n = n; pa.n_entries = S;
  pa.add_raw = b->d_add_raw; pa.kv_raw = b->d_kv_raw; pa.add_w = w.add_w; pa.add_b = w.add_b; pa.add_tab = b->wave.d_add_tab;
  for (int blk = 0; blk < B_NBLOCKS; ++blk) {
    pa.k_w[blk] = w.k_w[blk]; pa.k_b[blk] = w.k_b[blk]; pa.v_w[blk] = w.v_w[blk]; pa.v_b[blk] = w.v_b[blk];
    pa.kt[blk] = b->wave.d_kt[blk]; pa.v[blk] = b->wave.d_v[blk]; pa.kt_plain[blk] = b->wave.d_ktp[blk]; pa.v_plain[blk] = b->wave.d_vp[blk];
  }
  bool ok = install_entries(descs, staged, n, S, b->d_cb_raw, b->d_add_raw, b->d_kv_raw, b->d_cbT, b->d_cnorm, b->stream) &&
            morph_project_entries(pa, b->stream);
  ok = b->install_tables.mark(ring, b->stream) && ok;
  b->install_calls += 1;
  if (!in_flight) ok = hip_ok(hipStreamSynchronize(b->stream), "install entries") && ok;
  if (!ok) return -2;
  for (int i = 0; i < n; ++i) {
    const int e = entries[i];
    if (e >= b->n_speakers) b->n_speakers = e + 1;
    if (b->morph[e].active) { b->morph[e].active = false; --b->n_morph_slots; }   // the caller's data replaces a morph
  }
  return 0;
}
// the codebook lottery's engine of one stream (or of all, -1): std::mt19937(seed), e.g. a value derived from the
// stream's global identity when streams are sharded over several batches / GPUs
int BeatriceBatch_SeedLottery(BeatriceBatch* b, int stream, unsigned seed) {
  BATCH_OPEN(b);
  if (stream < -1 || stream >= b->B) return -1;
  for (int s = (stream < 0 ? 0 : stream); s < (stream < 0 ? b->B : stream + 1); ++s) b->lottery[s].seed(seed);
  b->lottery_seeded = true;  // a later BeatriceBatch_MorphSpeaker keeps these engines
  return 0;
}
// copies the morphed entry's raw embeddings back (test / inspection hook; any pointer may be NULL)
int BeatriceBatch_GetSpeakerEmbeddings(BeatriceBatch* b, int speaker, float* additive, float* key_value) {
  BATCH_OPEN(b);
  if (speaker < 0 || speaker >= b->max_speakers) return -1;
  bool ok = sync_all(b);
  if (additive) ok = ok && hip_ok(hipMemcpy(additive, b->d_add_raw + (size_t)speaker * B_HID, sizeof(float) * B_HID, hipMemcpyDeviceToHost), "add");
  if (key_value) ok = ok && hip_ok(hipMemcpy(key_value, b->d_kv_raw + (size_t)speaker * B_KV_LEN * B_KV_CH, sizeof(float) * B_KV_LEN * B_KV_CH, hipMemcpyDeviceToHost), "kv");
  return ok ? 0 : -2;
}

// ---- per-stream settings (reference ProcessorCore2 setters) ------------------------------------
// processor_core_2.cc:431-466: codebook + additive switch at once, K/V re-registered and installed
// one block per following hop.
int BeatriceBatch_SetTargetSpeaker(BeatriceBatch* b, int stream, int speaker) {
  BATCH_OPEN(b);
  if (speaker < 0 || speaker >= b->max_speakers) return -1;
  const int r = for_streams(b, stream, [&](StreamCfg& c) {
    c.target_speaker = speaker; c.codebook_speaker = speaker; c.additive_speaker = speaker; c.kv_set_count = 0; c.kv_delay = 0;
    for (int& cr : c.codebook_row) cr = speaker;
  });
  if (r == 0) { b->pending_kv = 0; for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++b->pending_kv; }
  return r;
}
// The same for n (stream, speaker) pairs in one call -- a server that moves many streams before a step (BASELINE.json configs[3]:
// 64 rotating speakers) pays the bookkeeping of the pending key/value installs once, not once per stream.  All or nothing: an
// invalid pair changes nothing.
int BeatriceBatch_SetTargetSpeakers(BeatriceBatch* b, int n, const int* streams, const int* speakers) {
  BATCH_OPEN(b);
  if (n < 0 || (n > 0 && (!streams || !speakers))) return -1;
  for (int i = 0; i < n; ++i)
    if (streams[i] < 0 || streams[i] >= b->B || speakers[i] < 0 || speakers[i] >= b->max_speakers) return -1;
  for (int i = 0; i < n; ++i) {
    StreamCfg& c = b->cfg[streams[i]];
    c.target_speaker = speakers[i]; c.codebook_speaker = speakers[i]; c.additive_speaker = speakers[i]; c.kv_set_count = 0; c.kv_delay = 0;
    for (int& cr : c.codebook_row) cr = speakers[i];
    sync_stream_arrays(b, streams[i]);
  }
  b->pending_kv = 0;
  for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++b->pending_kv;
  return 0;
}
// processor_core_2.cc:270,414: `while (SetKeyValueSpeakerEmbedding());`
int BeatriceBatch_FlushSpeaker(BeatriceBatch* b, int stream) {
  const DeviceScope dev_(b ? b->device : -1);
  const int r = for_streams(b, stream, [&](StreamCfg& c) { flush_kv(c); });
  if (r == 0) {
    for (int s = (stream < 0 ? 0 : stream); s < (stream < 0 ? b->B : stream + 1); ++s) fill_row_slots(b, s);
    b->pending_kv = 0;
    for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++b->pending_kv;
    for (int blk = 0; blk < B_NBLOCKS; ++blk) rebuild_tiles(b, blk);
  }
  return r;
}
// processor_core_2.cc:468-481
int BeatriceBatch_SetFormantShift(BeatriceBatch* b, int stream, double shift) {
  shift = std::min(std::max(shift, -2.0), 2.0);
  const int idx = (int)std::round(shift * 2.0 + 4.0);
  return for_streams(b, stream, [&](StreamCfg& c) { c.formant_index = idx; });
}
// processor_core_2.cc:585-590
int BeatriceBatch_SetVQNumNeighbors(BeatriceBatch* b, int stream, int k) {
  k = std::min(std::max(k, 0), 8);
  if (b) b->vq_dirty = true;
  return for_streams(b, stream, [&](StreamCfg& c) { c.vq_k = k; });
}
int BeatriceBatch_SetMinSourcePitch(BeatriceBatch* b, int stream, double note) {
  const int q = midi_to_bin(note);
  return for_streams(b, stream, [&](StreamCfg& c) { c.min_q = q; });
}
int BeatriceBatch_SetMaxSourcePitch(BeatriceBatch* b, int stream, double note) {
  const int q = midi_to_bin(note);
  return for_streams(b, stream, [&](StreamCfg& c) { c.max_q = q; });
}
// processor_core_2.cc:483-486, 534-559
int BeatriceBatch_SetPitchShift(BeatriceBatch* b, int stream, double v) {
  v = std::min(std::max(v, -24.0), 24.0);
  return for_streams(b, stream, [&](StreamCfg& c) { c.pitch.pitch_shift = v; });
}
int BeatriceBatch_SetAverageSourcePitch(BeatriceBatch* b, int stream, double v) {
  v = std::min(std::max(v, 0.0), 128.0);
  return for_streams(b, stream, [&](StreamCfg& c) { c.pitch.average_source_pitch = v; });
}
int BeatriceBatch_SetIntonationIntensity(BeatriceBatch* b, int stream, double v) {
  return for_streams(b, stream, [&](StreamCfg& c) { c.pitch.intonation_intensity = v; });
}
int BeatriceBatch_SetPitchCorrection(BeatriceBatch* b, int stream, double v) {
  v = std::min(std::max(v, 0.0), 1.0);
  return for_streams(b, stream, [&](StreamCfg& c) { c.pitch.pitch_correction = v; });
}
int BeatriceBatch_SetPitchCorrectionType(BeatriceBatch* b, int stream, int type) {
  if (type < 0 || type > 1) return -1;
  return for_streams(b, stream, [&](StreamCfg& c) { c.pitch.pitch_correction_type = type; });
}
// processor_core_2.cc:258-291: fresh contexts, then speaker (all four blocks at once) and the other
// settings re-applied -- here the settings persist per stream, only the state is zeroed.
int BeatriceBatch_ResetStream(BeatriceBatch* b, int stream) {
  BATCH_OPEN(b);
  if (stream < -1 || stream >= b->B) return -1;
  const int lo = stream < 0 ? 0 : stream, hi = stream < 0 ? b->B : stream + 1;
  bool ok = !(b->pipelined || b->tk.on) || sync_all(b);  // later stages of earlier steps may still be running (own streams / later ticks)
  for (int s = lo; s < hi && ok; ++s) {
    ok = b->phone.arena.zero_stream(s, b->stream) && b->pitch.arena.zero_stream(s, b->stream) &&
         b->wave.arena.zero_stream(s, b->stream) &&
         hip_ok(hipMemsetAsync(b->pitch.d_prev_q + s, 0, sizeof(int), b->stream), "prev_q") &&
         hip_ok(hipMemsetAsync(b->d_w48 + s, 0, sizeof(Wrap48State), b->stream), "w48 reset");
  }
  if (!ok) return -2;
  return BeatriceBatch_FlushSpeaker(b, stream);
}
// The same as a per-stream setting that travels with the next step (beatrice_batch.h; tick_reset.hip.h): in plain tick mode, in host
// streaming and around the resident 48 kHz blocks (mode F) nothing drains -- the stream is marked, its key/value blocks are installed as
// BeatriceBatch_FlushSpeaker does, and tick_run carries the reset through the stages with the step it applies to (in F also through the
// wrapper's two halves, batch_tick.hip.h tick_reset_wrap48).  Every other mode: BeatriceBatch_ResetStream.
int BeatriceBatch_ResetStreamInFlight(BeatriceBatch* b, int stream) {
  BATCH_OPEN(b);
  if (stream < -1 || stream >= b->B) return -1;
  const modes::Mode mode = modes::mode_of(flags_of(b));
  if (mode != modes::Mode::D && mode != modes::Mode::E && mode != modes::Mode::F) return BeatriceBatch_ResetStream(b, stream);
  if (!tick_reset_prepare(b)) return -2;
  for (int s = (stream < 0 ? 0 : stream); s < (stream < 0 ? b->B : stream + 1); ++s) b->tk.reset_pending[s] = 1;
  b->tk.any_reset_pending = true;
  return BeatriceBatch_FlushSpeaker(b, stream);
}
long long BeatriceBatch_TicksLaunched(const BeatriceBatch* b) { return b && b->tk.on ? b->tk.tick : 0; }

// ---- a stream's state from one batch into another (beatrice_batch.h; the blob: stream_blob.h, the kernels: stream_blob.hip) -----------
// What travels is what BeatriceBatch_ResetStream clears -- the stream's part of the three arenas, the pitch head's previous bin, its
// Wrap48State -- plus its StreamCfg and its lottery engine.  Both calls work at a drained point (sync_all: every stream stands at the
// batch's one counter, tick_relevel has run), so a blob is "the stream before step `counter`", and the destination, which stands at a
// counter of its own, turns every ring by the difference as it takes the blob in.
namespace {
bool blob_streams_ok(const BeatriceBatch* b, int n, const int* streams) { return smove::streams_ok(b->B, n, streams); }
// the piece table (once per batch, the way tick_reset_prepare builds its ring table) ...
bool blob_pieces(BeatriceBatch* b) {
  BeatriceBatch::StreamBlobs& sb = b->sb;
  const sblob::Layout& l = sb.layout;
  if (!sb.d_pieces) {
    std::vector<BlobPiece> pieces;
    for (const RingArena* a : {&b->phone.arena, &b->pitch.arena, &b->wave.arena})
      for (const Ring* r : a->rings) pieces.push_back(BlobPiece{r->base, (unsigned)ring_stream_floats(*r), (unsigned)(r->n * r->C), r->m, 0});
    pieces.push_back(BlobPiece{reinterpret_cast<float*>(b->pitch.d_prev_q), 1u, 1u, 1, 0});   // (an int: copied as a word)
    const unsigned w48 = (unsigned)(sizeof(Wrap48State) / sizeof(float));
    pieces.push_back(BlobPiece{reinterpret_cast<float*>(b->d_w48.get()), w48, w48, 1, 0});
    if (pieces.size() != l.pieces.size()) return false;
    for (size_t i = 0; i < pieces.size(); ++i) {
      if (pieces[i].slot_floats != l.pieces[i].slot_floats || pieces[i].m != l.pieces[i].m) return false;
      pieces[i].blob_off = l.pieces[i].off;
    }
    DevBuf<BlobPiece> d_pieces;
    if (!d_pieces.alloc(pieces.size(), "blob piece table", false) ||
        !hip_ok(hipMemcpy(d_pieces, pieces.data(), sizeof(BlobPiece) * pieces.size(), hipMemcpyHostToDevice), "blob piece table up"))
      return false;
    sb.n_pieces = (int)pieces.size(); sb.d_pieces = std::move(d_pieces);
  }
  return true;
}
// ... and staging for min(n, 16) blobs
bool blob_prepare(BeatriceBatch* b, int n) {
  if (!blob_pieces(b)) return false;
  BeatriceBatch::StreamBlobs& sb = b->sb;
  const sblob::Layout& l = sb.layout;
  const int want = std::min(n, sblob::kMaxRound);
  if (sb.cap < want) {
    PinnedBuf<unsigned char> h_stage;
    DevBuf<unsigned char> d_stage;
    if (!h_stage.alloc((size_t)want * l.blob_bytes, "blob staging", false) || !d_stage.alloc((size_t)want * l.blob_bytes, "blob staging")) return false;
    sb.h_stage = std::move(h_stage); sb.d_stage = std::move(d_stage); sb.cap = want;
  }
  return true;
}
void blob_indices_of(const StreamCfg& c, int32_t* idx) {
  idx[0] = c.target_speaker; idx[1] = c.additive_speaker; idx[2] = c.codebook_speaker;
  for (int i = 0; i < B_NBLOCKS; ++i) idx[3 + i] = c.kv_slot[i];
  for (int i = 0; i < 8; ++i) idx[3 + B_NBLOCKS + i] = c.codebook_row[i];
}
void blob_indices_into(StreamCfg& c, const int32_t* idx) {
  c.target_speaker = idx[0]; c.additive_speaker = idx[1]; c.codebook_speaker = idx[2];
  for (int i = 0; i < B_NBLOCKS; ++i) c.kv_slot[i] = idx[3 + i];
  for (int i = 0; i < 8; ++i) c.codebook_row[i] = idx[3 + B_NBLOCKS + i];
}
// the settings of a blob hold what the setters can have put there (the table indices are checked apart: sblob::map_indices)
bool blob_cfg_ok(const StreamCfg& c) {
  return c.kv_set_count >= 0 && c.kv_set_count <= B_NBLOCKS && c.kv_delay >= 0 && c.kv_delay <= 4 && c.formant_index >= 0 && c.formant_index <= 8 &&
         c.vq_k >= 0 && c.vq_k <= 8 && c.min_q >= 1 && c.min_q < B_PITCH_BINS && c.max_q >= 1 && c.max_q < B_PITCH_BINS &&
         c.pitch.pitch_correction_type >= 0 && c.pitch.pitch_correction_type <= 1;
}
static_assert(sblob::kIndices == 3 + B_NBLOCKS + 8 && std::is_trivially_copyable<StreamCfg>::value && sizeof(Wrap48State) % sizeof(float) == 0, "blob settings");
}  // namespace

size_t BeatriceBatch_StreamBlobBytes(const BeatriceBatch* b) { return b && b->ok ? b->sb.layout.blob_bytes : 0; }

namespace {
// The rounds of an export, drained or in flight: gather, copy down, the host part of every blob.  In flight nothing was drained: the
// launch and the copy go behind the ticks already enqueued, the call waits for an event behind its own copy, and a blob's counter is
// the stream's own (smove::own_counter) -- which at a drained point is the batch's.
int export_rounds(BeatriceBatch* b, int n, const int* streams, void* blobs, bool in_flight) {
  BeatriceBatch::StreamBlobs& sb = b->sb;
  const sblob::Layout& l = sb.layout;
  unsigned char* out = static_cast<unsigned char*>(blobs);
  for (int at = 0; at < n; at += sb.cap) {
    BlobRound round{};
    round.n = std::min(sb.cap, n - at);
    for (int j = 0; j < round.n; ++j) round.streams[j] = streams[at + j];
    if (!stream_gather(sb.d_pieces, sb.n_pieces, round, reinterpret_cast<float*>(sb.d_stage.get()), l.blob_bytes / sizeof(float), b->stream) ||
        !hip_ok(hipMemcpyAsync(sb.h_stage, sb.d_stage, (size_t)round.n * l.blob_bytes, hipMemcpyDeviceToHost, b->stream), "blobs down"))
      return -2;
    if (in_flight ? !(hip_ok(hipEventRecord(b->mv.ev_export, b->stream), "export event") && hip_ok(hipEventSynchronize(b->mv.ev_export), "stream gather"))
                  : !hip_ok(hipStreamSynchronize(b->stream), "stream gather"))
      return -2;
    for (int j = 0; j < round.n; ++j) {
      unsigned char* blob = sb.h_stage + (size_t)j * l.blob_bytes;
      const int s = round.streams[j];
      const StreamCfg& c = b->cfg[s];
      int32_t idx[sblob::kIndices];
      blob_indices_of(c, idx);
      std::memset(blob, 0, l.off_state);
      sblob::write_header(l, smove::own_counter(in_flight && b->tk.ragged, b->tk.hop_s, s, b->hop_host), blob);
      std::memcpy(blob + l.off_indices, idx, sizeof(idx));
      std::memcpy(blob + l.off_cfg, &c, sizeof(c));
      if (!sblob::engine_out(b->lottery[s], blob + l.off_engine)) return -2;
      std::memcpy(out + (size_t)(at + j) * l.blob_bytes, blob, l.blob_bytes);
    }
  }
  return 0;
}
}  // namespace

int BeatriceBatch_ExportStreams(BeatriceBatch* b, int n, const int* streams, void* blobs) {
  BATCH_OPEN(b);
  if (!blob_streams_ok(b, n, streams) || !blobs) return -1;
  // a reset that waits for the stream's next step has not happened yet: the rings still hold what it is to clear
  for (int i = 0; i < n; ++i) if (reset_waits_for(b, streams[i])) return -3;
  if (!blob_prepare(b, n) || !sync_all(b)) return -2;
  return export_rounds(b, n, streams, blobs, false);
}

namespace {
struct Taken { StreamCfg cfg; std::mt19937 engine; int counter; };
// every blob is looked at before anything is drained, staged, uploaded or written
bool blobs_take(const BeatriceBatch* b, int n, const void* blobs, const int* entry_map, int n_map, std::vector<Taken>* taken) {
  const sblob::Layout& l = b->sb.layout;
  const unsigned char* in = static_cast<const unsigned char*>(blobs);
  taken->resize(n);
  for (int i = 0; i < n; ++i) {
    const unsigned char* blob = in + (size_t)i * l.blob_bytes;
    Taken& t = (*taken)[i];
    int32_t idx[sblob::kIndices];
    if (sblob::validate_header(l, blob, l.blob_bytes, B_HOP_WRAP, &t.counter) != sblob::kOk ||
        sblob::map_indices(l, blob, entry_map, n_map, b->n_speakers, b->max_speakers, idx) != sblob::kOk)
      return false;
    std::memcpy(&t.cfg, blob + l.off_cfg, sizeof(StreamCfg));
    if (!blob_cfg_ok(t.cfg) || !sblob::engine_in(blob + l.off_engine, &t.engine)) return false;
    blob_indices_into(t.cfg, idx);
  }
  return true;
}
// the settings, as a change of every setting of the stream at once: the existing path takes them to the device with the next step
void blobs_settle(BeatriceBatch* b, int n, const int* streams, const std::vector<Taken>& taken) {
  for (int i = 0; i < n; ++i) {
    const int s = streams[i];
    b->cfg[s] = taken[i].cfg;
    b->lottery[s] = taken[i].engine;
    sync_stream_arrays(b, s);   // (recount, the front part of the settings block)
    fill_row_slots(b, s);       // (a pending install moves them block by block from the next step on: advance_kv)
    if ((int)b->tk.reset_pending.size() == b->B) b->tk.reset_pending[s] = 0;   // a reset still waiting for this slot's next step: the blob replaces what it would clear
  }
  if (b->tk.any_reset_pending) {
    b->tk.any_reset_pending = false;
    for (const unsigned char p : b->tk.reset_pending) b->tk.any_reset_pending = b->tk.any_reset_pending || p != 0;
  }
  b->pending_kv = 0;
  for (const StreamCfg& c : b->cfg) if (c.kv_set_count < B_NBLOCKS) ++b->pending_kv;
  b->vq_dirty = true;
  for (int blk = 0; blk < B_NBLOCKS; ++blk) rebuild_tiles(b, blk);   // (marks every copy of the wave part for upload)
}
}  // namespace

int BeatriceBatch_ImportStreams(BeatriceBatch* b, int n, const int* streams, const void* blobs, const int* entry_map, int n_map) {
  BATCH_OPEN(b);
  if (!blob_streams_ok(b, n, streams) || !blobs || n_map < 0 || (entry_map == nullptr) != (n_map == 0)) return -1;
  BeatriceBatch::StreamBlobs& sb = b->sb;
  const sblob::Layout& l = sb.layout;
  const unsigned char* in = static_cast<const unsigned char*>(blobs);
  std::vector<Taken> taken;
  if (!blobs_take(b, n, blobs, entry_map, n_map, &taken)) return -1;
  if (!blob_prepare(b, n) || !sync_all(b)) return -2;
  for (int at = 0; at < n; at += sb.cap) {
    BlobRound round{};
    round.n = std::min(sb.cap, n - at);
    for (int j = 0; j < round.n; ++j) {
      round.streams[j] = streams[at + j];
      round.shift[j] = sblob::counter_shift(b->hop_host, taken[at + j].counter, B_HOP_WRAP);
    }
    std::memcpy(sb.h_stage, in + (size_t)at * l.blob_bytes, (size_t)round.n * l.blob_bytes);
    if (!hip_ok(hipMemcpyAsync(sb.d_stage, sb.h_stage, (size_t)round.n * l.blob_bytes, hipMemcpyHostToDevice, b->stream), "blobs up") ||
        !stream_scatter(sb.d_pieces, sb.n_pieces, round, reinterpret_cast<const float*>(sb.d_stage.get()), l.blob_bytes / sizeof(float), b->stream) ||
        !hip_ok(hipStreamSynchronize(b->stream), "stream scatter"))
      return -2;
  }
  blobs_settle(b, n, streams, taken);
  return 0;
}

// ---- the same between two batches that both go on ticking (beatrice_batch.h; the rules: stream_move_plan.h) --------------------------------
// Nothing drains and no tick is launched: the streams named are at rest (no step of theirs is inside the pipeline), every launch enqueued
// from here on skips their rows until they are fed again, so the gather, the scatter or the ring-to-ring move, enqueued on the batch's
// stream between two ticks, touches state nobody else reads or writes.  Each stream is taken, and turned, at its OWN counter.
namespace {
struct MoveSide : smove::Side {   // one batch's part of a call
  MoveSide(const BeatriceBatch* b, int n_, const int* streams_, bool pointers_ok_, smove::Rule rule_ = smove::kRulePlain) {
    const modes::Mode mode = modes::mode_of(flags_of(b));
    plain_tick = mode == modes::Mode::D; around48k = mode == modes::Mode::F; rule = rule_;
    B = b->B; n = n_; streams = streams_; pointers_ok = pointers_ok_;
  }
};
smove::Verdict move_at_rest(const BeatriceBatch* b, const smove::Side& s, bool is_source) {
  const tick::State& k = b->tk;
  const bool flags = is_source && k.any_reset_pending && (int)k.reset_pending.size() == b->B;   // (a destination's pending reset is cancelled, not refused)
  return smove::at_rest(s, b->mv.seen, k.tick, k.plan.count(), flags ? k.reset_pending.data() : nullptr);
}
int move_own_counter(const BeatriceBatch* b, int s) { return smove::own_counter(b->tk.ragged, b->tk.hop_s, s, b->hop_host); }
}  // namespace

namespace {
// (the four calls of mode D and the four of mode F are one body each: what differs is the mode asked for and the rule asked, both in MoveSide)
int stream_quiescent(const BeatriceBatch* b, int stream, smove::Rule rule) {
  if (!b || !b->ok || modes::mode_of(flags_of(b)) != (rule == smove::kRuleAround48k ? modes::Mode::F : modes::Mode::D) || stream < 0 || stream >= b->B) return -1;
  return smove::quiescent(b->mv.seen, rule, stream, b->tk.tick, b->tk.plan.count()) ? 1 : 0;
}
int export_streams_in_flight(BeatriceBatch* b, int n, const int* streams, void* blobs, smove::Rule rule);
int import_streams_in_flight(BeatriceBatch* b, int n, const int* streams, const void* blobs, const int* entry_map, int n_map, smove::Rule rule);
int move_streams_in_flight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams, const int* entry_map, int n_map, smove::Rule rule);
}  // namespace

int BeatriceBatch_StreamQuiescent(const BeatriceBatch* b, int stream) { return stream_quiescent(b, stream, smove::kRulePlain); }
int BeatriceBatch_ExportStreamsInFlight(BeatriceBatch* b, int n, const int* streams, void* blobs) { return export_streams_in_flight(b, n, streams, blobs, smove::kRulePlain); }
int BeatriceBatch_ImportStreamsInFlight(BeatriceBatch* b, int n, const int* streams, const void* blobs, const int* entry_map, int n_map) {
  return import_streams_in_flight(b, n, streams, blobs, entry_map, n_map, smove::kRulePlain);
}
int BeatriceBatch_MoveStreamsInFlight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams,
                                      const int* entry_map, int n_map) {
  return move_streams_in_flight(src, dst, n, src_streams, dst_streams, entry_map, n_map, smove::kRulePlain);
}
// ---- ... and between two batches that both go on converting resident 48 kHz blocks (mode F; beatrice_batch.h footnote (14)) ------------
// The same calls with the second quiescence rule (stream_move_plan.h kRuleAround48k): the wrapper's output half runs one launch behind the
// step's last stage, so a stream is at rest one launch later than in D.  The blob and the piece table already hold its Wrap48State.
int BeatriceBatch_Stream48kQuiescent(const BeatriceBatch* b, int stream) { return stream_quiescent(b, stream, smove::kRuleAround48k); }
int BeatriceBatch_ExportStreams48kInFlight(BeatriceBatch* b, int n, const int* streams, void* blobs) { return export_streams_in_flight(b, n, streams, blobs, smove::kRuleAround48k); }
int BeatriceBatch_ImportStreams48kInFlight(BeatriceBatch* b, int n, const int* streams, const void* blobs, const int* entry_map, int n_map) {
  return import_streams_in_flight(b, n, streams, blobs, entry_map, n_map, smove::kRuleAround48k);
}
int BeatriceBatch_MoveStreams48kInFlight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams,
                                         const int* entry_map, int n_map) {
  return move_streams_in_flight(src, dst, n, src_streams, dst_streams, entry_map, n_map, smove::kRuleAround48k);
}

namespace {
int export_streams_in_flight(BeatriceBatch* b, int n, const int* streams, void* blobs, const smove::Rule rule) {
  BATCH_OPEN(b);
  const MoveSide side(b, n, streams, blobs != nullptr, rule);
  if (smove::args(side) != smove::kGo) return -1;
  if (move_at_rest(b, side, true) != smove::kGo) return -3;
  if (!blob_prepare(b, n) || (!b->mv.ev_export && !b->mv.ev_export.create("export event"))) return -2;
  return export_rounds(b, n, streams, blobs, true);
}
// the rings of an in-flight import: the blobs into the call's pinned staging entry, up and scattered round by round on the batch's stream,
// each stream turned to its own counter; nothing is waited for but the entry's previous user
int import_rounds_in_flight(BeatriceBatch* b, int n, const int* streams, const void* blobs, const std::vector<Taken>& taken) {
  if (!blob_prepare(b, n)) return -2;   // (the device staging of a round is the drained calls': everything that uses it is on the batch's stream, in order)
  BeatriceBatch::StreamBlobs& sb = b->sb;
  const sblob::Layout& l = sb.layout;
  BeatriceBatch::StreamMoves::Staged& st = b->mv.staged[b->mv.imports % BeatriceBatch::StreamMoves::kCalls];
  if (st.marked && !hip_ok(hipEventSynchronize(st.done), "import staging entry")) return -2;   // (the call before the last has not been scattered yet)
  st.marked = false;
  const size_t bytes = (size_t)n * l.blob_bytes;
  if (st.h.size() < bytes) {
    PinnedBuf<unsigned char> h;
    if (!h.alloc(bytes, "import staging", false)) return -2;
    st.h = std::move(h);
  }
  if (!st.done && !st.done.create("import staging event")) return -2;
  std::memcpy(st.h, blobs, bytes);
  for (int at = 0; at < n; at += sb.cap) {
    BlobRound round{};
    round.n = std::min(sb.cap, n - at);
    for (int j = 0; j < round.n; ++j) {
      round.streams[j] = streams[at + j];
      round.shift[j] = smove::import_shift(move_own_counter(b, streams[at + j]), taken[at + j].counter, B_HOP_WRAP);
    }
    if (!hip_ok(hipMemcpyAsync(sb.d_stage, st.h + (size_t)at * l.blob_bytes, (size_t)round.n * l.blob_bytes, hipMemcpyHostToDevice, b->stream), "blobs up") ||
        !stream_scatter(sb.d_pieces, sb.n_pieces, round, reinterpret_cast<const float*>(sb.d_stage.get()), l.blob_bytes / sizeof(float), b->stream))
      return -2;
  }
  if (!hip_ok(hipEventRecord(st.done, b->stream), "import staging event")) return -2;
  st.marked = true;
  b->mv.imports += 1;
  return 0;
}

int import_streams_in_flight(BeatriceBatch* b, int n, const int* streams, const void* blobs, const int* entry_map, int n_map, const smove::Rule rule) {
  BATCH_OPEN(b);
  const MoveSide side(b, n, streams, blobs != nullptr && n_map >= 0 && (entry_map == nullptr) == (n_map == 0), rule);
  if (smove::args(side) != smove::kGo) return -1;
  std::vector<Taken> taken;
  if (!blobs_take(b, n, blobs, entry_map, n_map, &taken)) return -1;
  if (move_at_rest(b, side, false) != smove::kGo) return -3;
  const int rc = import_rounds_in_flight(b, n, streams, blobs, taken);
  if (rc) return rc;
  blobs_settle(b, n, streams, taken);
  return 0;
}
// the settings part of a move, host to host, with the checks the blob path makes
bool move_take(const BeatriceBatch* src, const BeatriceBatch* dst, int n, const int* src_streams, const int* entry_map, int n_map, std::vector<Taken>* taken) {
  taken->resize(n);
  for (int i = 0; i < n; ++i) {
    Taken& t = (*taken)[i];
    int32_t idx[sblob::kIndices], mapped[sblob::kIndices];
    t.cfg = src->cfg[src_streams[i]];
    t.engine = src->lottery[src_streams[i]];
    t.counter = move_own_counter(src, src_streams[i]);
    blob_indices_of(t.cfg, idx);
    if (sblob::map_index_list(idx, entry_map, n_map, dst->n_speakers, dst->max_speakers, mapped) != sblob::kOk || !blob_cfg_ok(t.cfg)) return false;
    blob_indices_into(t.cfg, mapped);
  }
  return true;
}
// The rings from batch to batch on the destination's stream, and `also(ok)` -- what else the call enqueues there -- inside the same fence.
// Different streams: the move waits for the source's launches enqueued so far, and whatever the source enqueues later -- a reset, an
// import or a present step of the slot -- waits for the move.
extern "C++" template <class F>
int move_rings_fenced(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams, const std::vector<Taken>& taken, F also) {
  if (!blob_pieces(src) || !blob_pieces(dst) || src->sb.n_pieces != dst->sb.n_pieces) return -2;
  const bool two_streams = src->stream != dst->stream;
  if (two_streams) {
    if ((!src->mv.ev_src && !src->mv.ev_src.create("move source event")) || (!dst->mv.ev_dst && !dst->mv.ev_dst.create("move destination event")) ||
        !hip_ok(hipEventRecord(src->mv.ev_src, src->stream), "move source event") ||
        !hip_ok(hipStreamWaitEvent(dst->stream, src->mv.ev_src, 0), "move waits for the source"))
      return -2;
  }
  bool ok = true;
  for (int at = 0; at < n && ok; at += sblob::kMaxRound) {
    MoveRound round{};
    round.n = std::min(sblob::kMaxRound, n - at);
    for (int j = 0; j < round.n; ++j) {
      round.src[j] = src_streams[at + j];
      round.dst[j] = dst_streams[at + j];
      round.shift[j] = smove::import_shift(move_own_counter(dst, dst_streams[at + j]), taken[at + j].counter, B_HOP_WRAP);
    }
    ok = stream_move(src->sb.d_pieces, dst->sb.d_pieces, dst->sb.n_pieces, round, dst->stream);
  }
  ok = also(ok);
  if (two_streams)   // (also behind a launch that failed: the source must never overtake what WAS enqueued)
    ok = hip_ok(hipEventRecord(dst->mv.ev_dst, dst->stream), "move destination event") &&
         hip_ok(hipStreamWaitEvent(src->stream, dst->mv.ev_dst, 0), "source waits for the move") && ok;
  return ok ? 0 : -2;
}

int move_streams_in_flight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams, const int* entry_map, int n_map,
                           const smove::Rule rule) {
  if (!src || !dst || src == dst) return -1;
  if (!src->ok || !dst->ok) return -2;
  if (src->device != dst->device) return -1;
  const DeviceScope dev_(dst->device);
  const bool map_ok = n_map >= 0 && (entry_map == nullptr) == (n_map == 0);
  const MoveSide from(src, n, src_streams, map_ok, rule), to(dst, n, dst_streams, map_ok, rule);
  if (smove::args(from) != smove::kGo || smove::args(to) != smove::kGo || !sblob::same_layout(src->sb.layout, dst->sb.layout)) return -1;
  std::vector<Taken> taken;
  if (!move_take(src, dst, n, src_streams, entry_map, n_map, &taken)) return -1;
  if (move_at_rest(src, from, true) != smove::kGo || move_at_rest(dst, to, false) != smove::kGo) return -3;
  const int rc = move_rings_fenced(src, dst, n, src_streams, dst_streams, taken, [](bool ok) { return ok; });
  if (rc) return rc;
  blobs_settle(dst, n, dst_streams, taken);
  return 0;
}
}  // namespace

// ---- per-hop ------------------------------------------------------------------------------------
int BeatriceBatch_ConvertFramesDevice(BeatriceBatch* b, const float* d_in, float* d_out) {
  BATCH_ENTER(b, d_in || d_out ? Entry::ConvertFramesDevice_ptrs : Entry::ConvertFramesDevice_NULL);
  return step_device(b, d_in, d_out) ? 0 : -2;
}
// Resident I/O: the caller keeps n_slots steps of input and output on the device,
//   d_in [n_slots][B][H*160], d_out [n_slots][B][H*240];
// step k (BeatriceBatch_ConvertFramesDevice(b, NULL, NULL)) reads slot k mod n_slots and writes the same
// slot of d_out, with no copy: the slot index lives next to the step counter in device memory and is
// advanced by the last kernel, so the captured graph stays valid.  NULL pointers unbind.
// (bind_io: the binding itself, for the modes that bind slots of their own on their way in and out)
static int bind_io(BeatriceBatch* b, const float* d_in, float* d_out, int n_slots) {
  const bool bind = d_in != nullptr || d_out != nullptr;
  if (bind && (!d_in || !d_out || n_slots < 1)) return -1;
  if (!set_io_mapped(b, false) || !sync_all(b)) return -2;
  b->io_host = 0;
  drop_graph(b);  // kernel arguments change
  if (b->own_d_out) { b->wave.d_out = b->own_d_out; b->own_d_out = nullptr; }
  b->phone.d_in = b->pitch.d_in = b->d_in;
  b->phone.io_stride = b->pitch.io_stride = b->wave.io_stride = 0;
  b->wave.io_slots = b->io_slots = 0;
  if (bind) {
    b->own_d_out = b->wave.d_out;
    b->wave.d_out = d_out;
    b->phone.d_in = b->pitch.d_in = const_cast<float*>(d_in);
    b->phone.io_stride = b->pitch.io_stride = (size_t)b->B * b->H * B_IN_HOP;
    b->wave.io_stride = (size_t)b->B * b->H * B_OUT_HOP;
    b->wave.io_slots = b->io_slots = n_slots;
  }
  const int zero = 0;  // the next step starts at slot 0
  return hip_ok(hipMemcpy(b->d_hop_next + 1, &zero, sizeof(int), hipMemcpyHostToDevice), "slot0") ? 0 : -2;
}
int BeatriceBatch_BindResidentIO(BeatriceBatch* b, const float* d_in, float* d_out, int n_slots) {
  BATCH_ENTER(b, d_in || d_out ? Entry::BindResidentIO_bind : Entry::BindResidentIO_unbind);
  return bind_io(b, d_in, d_out, n_slots);
}

int BeatriceBatch_ConvertFrames(BeatriceBatch* b, const float* in, float* out) {
  const DeviceScope dev_(b ? b->device : -1);
  if (!b || !b->ok) { if (b && out) std::memset(out, 0, sizeof(float) * b->B * b->H * B_OUT_HOP); return -2; }
  BATCH_GATE(b, Entry::ConvertFrames);
  const size_t n_in = (size_t)b->B * b->H * B_IN_HOP, n_out = (size_t)b->B * b->H * B_OUT_HOP;
  b->want_mapped = true;
  bool ok = set_io_mapped(b, true);
  std::memcpy(b->h_in, in, sizeof(float) * n_in);
  if (!b->io_mapped) ok = ok && hip_ok(hipMemcpyAsync(b->d_in, b->h_in, sizeof(float) * n_in, hipMemcpyHostToDevice, b->stream), "in");
  ok = ok && step_device(b, nullptr, nullptr);
  if (!b->io_mapped) ok = ok && hip_ok(hipMemcpyAsync(b->h_out, b->wave.d_out, sizeof(float) * n_out, hipMemcpyDeviceToHost, wave_stream(b)), "out");
  b->want_mapped = false;
  ok = sync_all(b) && ok;
  if (ok) std::memcpy(out, b->h_out, sizeof(float) * n_out);
  else std::memset(out, 0, sizeof(float) * n_out);
  return ok ? 0 : -2;
}
#include "batch_wrappers.hip.h"  // 48 kHz and any-rate wrappers, in order and around the ticks

// Test hook (beatrice_batch.h): the wave module's team launch of a one-stream batch "times out" at the next synchronisation (sync_all's recovery path)
int BeatriceBatch_InjectTeamTimeout(BeatriceBatch* b) {
  if (!b || !b->ok || !b->wave.d_team_dead || b->wave.team_off) return -1;
  *b->wave.d_team_dead = 1;
  return 0;
}
// Test hook (beatrice_batch.h): a FRESH batch starts at another step counter -- the host mirror and the device's copy, as the tick-leave path
// hands them to the in-order chain (tick_enable).  Nothing has been enqueued, so nothing is waited for.
static_assert(BEATRICE_HIP_STEP_WRAP == B_HOP_WRAP, "beatrice_batch.h names the step counter's wrap");
int BeatriceBatch_SetStepCounter(BeatriceBatch* b, int counter) {
  BATCH_OPEN(b);
  if (counter < 0 || counter >= B_HOP_WRAP) return -1;
  if (b->steps_enqueued != 0 || b->tk.on || b->hs.on || b->r48.on || b->rb.on || b->io_slots > 0) return -1;
  const int pair[2] = {counter, b->io_host};
  if (!hip_ok(hipMemcpy(b->d_hop_next, pair, sizeof(pair), hipMemcpyHostToDevice), "step counter")) return -2;
  b->hop_host = counter;
  b->front_dirty = true;
  for (bool& w : b->wave_dirty) w = true;
  return 0;
}
int BeatriceBatch_StepCounter(const BeatriceBatch* b) { return b ? b->hop_host : -1; }
int BeatriceBatch_Synchronize(BeatriceBatch* b) {
  BATCH_OPEN(b);
  return sync_all(b) ? 0 : -2;
}

int BeatriceBatch_SetStream(BeatriceBatch* b, void* hip_stream) {
  BATCH_OPEN(b);
  (void)sync_all(b);
  drop_graph(b);
  b->stream_own.reset();
  b->stream = static_cast<hipStream_t>(hip_stream);
  return 0;
}
void* BeatriceBatch_GetStream(const BeatriceBatch* b) { return b ? b->stream : nullptr; }
int BeatriceBatch_EnableGraph(BeatriceBatch* b, int enable) {
  BATCH_OPEN(b);
  (void)sync_all(b);
  b->use_graph = enable != 0;
  if (!b->use_graph) drop_graph(b);
  return 0;
}
#include "batch_host_stream.hip.h"  // BeatriceBatch_StreamFrames

// Throughput mode for callers that enqueue steps ahead (BeatriceBatch_ConvertFramesDevice without waiting,
// resident I/O): the front end of step t+1 runs on the batch's stream while the waveform generator of step t
// runs on a second stream.  Same results; a step's output is complete when BeatriceBatch_Synchronize returns
// (or, stream-ordered, on BeatriceBatch_GetWaveStream).  Off by default: everything in order on one stream.
int BeatriceBatch_EnableTickPipeline(BeatriceBatch* b, int enable) {
  BATCH_ENTER(b, enable ? Entry::EnableTickPipeline_1 : Entry::EnableTickPipeline_0);
  return tick_enable(b, enable != 0);
}
int BeatriceBatch_TickStages(const BeatriceBatch* b) { return b ? b->tk.plan.count() : 0; }
// Measurement hook: `ticks` more ticks (each feeding a step from the resident slots), every tick's pipeline launch
// between one pair of HIP events on the batch's stream; returns the mean duration per launch and its algorithmic work.
// Call with the pipeline full (at least BeatriceBatch_TickStages steps fed) for the steady-state figure.
int BeatriceBatch_TimeTickLaunch(BeatriceBatch* b, int ticks, float* us_per_launch, double* flops, double* bytes) {
  BATCH_ENTER(b, Entry::TimeTickLaunch);
  if (ticks < 1 || ticks > 64 || !us_per_launch) return -1;
  // ONE pair of events around `ticks` back-to-back launches (an event pair per launch adds two commands between
  // consecutive launches and reads ~5 us long against rocprofv3's kernel durations); the figure includes the boundary
  // between two ticks, which belongs to the launch's cost
  Event ev[2];
  bool ok = ev[0].create("tick ev", true) && ev[1].create("tick ev", true);
  ok = ok && hip_ok(hipEventRecord(ev[0], b->stream), "tick ev0");
  for (int i = 0; i < ticks && ok; ++i) ok = tick_run(b, true);
  ok = ok && hip_ok(hipEventRecord(ev[1], b->stream), "tick ev1") && hip_ok(hipStreamSynchronize(b->stream), "tick time sync");
  float ms = 0;
  ok = ok && hip_ok(hipEventElapsedTime(&ms, ev[0], ev[1]), "tick elapsed");
  if (!ok) return -2;
  *us_per_launch = (float)(1000.0 * ms / ticks);
  if (flops) *flops = b->tk.table_flops;
  if (bytes) *bytes = b->tk.table_bytes;
  return 0;
}
#ifdef BEATRICE_HIP_MEASUREMENT_BUILD
// MEASUREMENT BUILDS ONLY: from the next tick on the launch holds only the bodies whose tick::BodyType bit is set in `mask`
// (the other stages' outputs go stale: instruction counters and timings per body type, never results)
extern "C" int BeatriceBatchMeas_TickOnlyTypes(BeatriceBatch* b, unsigned long long mask) {
  const DeviceScope dev_(b ? b->device : -1);
  if (!b || !b->ok || !b->tk.on) return -1;
  if (!hip_ok(hipStreamSynchronize(b->stream), "meas sync")) return -2;
  g_tick_only_types = mask;
  b->tk.table_dirty = true;
  return 0;
}
#endif
int BeatriceBatch_EnablePipelining(BeatriceBatch* b, int enable) {
  BATCH_OPEN(b);
  modes::Flags f = flags_of(b);
  if (enable < 1) f.silent = false;   // (the rule stands in the way of n >= 1 only: switching off is the cell of the same mode without the rule)
  if (!modes::allowed(Entry::EnablePipelining, f) || enable < 0 || enable > BeatriceBatch::kMaxStages) return -1;
  if (!set_io_mapped(b, false) || !sync_all(b)) return -2;
  drop_graph(b);  // stages are captured on the streams they will run on
  set_plan(b, enable == 1 ? 2 : enable);  // 1 = the default depth
  for (int s = 1; s < b->n_stages && b->pipelined; ++s)  // every stream takes a hardware queue: only those in use exist
    if (!b->stage_stream_own[s] && !make_stage_stream(b->stage_stream_own[s], s)) return -2;
  return 0;
}
void* BeatriceBatch_GetWaveStream(const BeatriceBatch* b) { return b ? wave_stream(b) : nullptr; }
// Captures the hipGraphs of the current mode now (nothing is executed), so that the first steps do not pay for it.
int BeatriceBatch_Prepare(BeatriceBatch* b) {
  BATCH_OPEN(b);
  if (b->vq_dirty) { update_vq_mode(b); b->vq_dirty = false; }
  if (!b->use_graph) return 0;
  bool ok = true;
  if (!b->pipelined) ok = run_step_in_order(b, -1);
  else for (int s = 0; s < b->n_stages && ok; ++s) ok = run_stage(b, s, -1);
  return ok ? 0 : -2;
}
float* BeatriceBatch_DeviceInput(BeatriceBatch* b) { return b && b->ok ? b->d_in.get() : nullptr; }
float* BeatriceBatch_DeviceOutput(BeatriceBatch* b) {
  const DeviceScope dev_(b ? b->device : -1);
  return b && b->ok && set_io_mapped(b, false) ? b->wave.d_out : nullptr;
}

int BeatriceBatch_GetIntermediates(BeatriceBatch* b, float* phone, int* q_raw, int* q, float* feat) {
  BATCH_OPEN(b);
  bool ok = sync_all(b);
  if (phone) {  // the phone vectors of the last step sit in one of the three step slots of a per-stream ring
    const size_t row = sizeof(float) * b->H * B_PHONE_CH;
    ok = ok && hip_ok(hipMemcpy2D(phone, row, b->phone.d_phone + (size_t)b->last_parity * b->H * B_PHONE_CH, row * b->phone.out_slots, row,
                                  b->B, hipMemcpyDeviceToHost), "phone");
  }
  const size_t qo = (size_t)(b->last_hop % b->pitch.q_slots) * b->B * b->H;  // the pitch head's outputs are double-buffered by step
  if (q_raw) ok = ok && hip_ok(hipMemcpy(q_raw, b->pitch.d_q_raw + qo, sizeof(int) * b->B * b->H, hipMemcpyDeviceToHost), "q_raw");
  if (q) ok = ok && hip_ok(hipMemcpy(q, b->pitch.d_q + qo, sizeof(int) * b->B * b->H, hipMemcpyDeviceToHost), "q");
  if (feat) ok = ok && hip_ok(hipMemcpy(feat, b->pitch.d_feat + qo * 4, sizeof(float) * b->B * b->H * 4, hipMemcpyDeviceToHost), "feat");
  return ok ? 0 : -2;
}

namespace {
struct KernelRow { std::string name; int launches = 0; double us = 0, flops = 0, bytes = 0; };
struct ProfileHook : LaunchHook {
  std::vector<KernelRow> rows;
  int repeats = 1;
  hipEvent_t e0, e1;
  bool ok = true;
  void on_launch(const LaunchInfo& info, hipStream_t stream, void (*thunk)(void*), void* ctx) override {
    // launches that update state in place run once (the tail rewrites its history block, the pitch head its previous
    // bin, the GRUs their state, hop_advance the counter); everything else only writes this step's ring slots
    const bool once = std::strstr(info.name, "hop_advance") || std::strstr(info.name, "wave.tail") || std::strstr(info.name, "pitch.head") ||
                      std::strstr(info.name, "gru");
    const int reps = once ? 1 : repeats;
    ok = ok && hip_ok(hipEventRecord(e0, stream), "p0");
    for (int i = 0; i < reps; ++i) thunk(ctx);
    float ms = 0.f;
    ok = ok && hip_ok(hipEventRecord(e1, stream), "p1") && hip_ok(hipEventSynchronize(e1), "ps") &&
         hip_ok(hipEventElapsedTime(&ms, e0, e1), "pe");
    KernelRow* row = nullptr;
    for (auto& r : rows) if (r.name == info.name) row = &r;
    if (!row) { rows.push_back(KernelRow{info.name}); row = &rows.back(); }
    row->launches += 1;
    row->us += 1000.0 * ms / reps;
    row->flops = info.flops;
    row->bytes = info.bytes;
  }
};
}  // namespace

int BeatriceBatch_ProfileKernels(BeatriceBatch* b, int repeats, int max_entries, char* names, int* launches, double* mean_us,
                                 double* flops, double* bytes) {
  BATCH_ENTER(b, Entry::ProfileKernels);
  if (repeats < 1 || max_entries < 1 || !names || !launches || !mean_us || !flops || !bytes) return -1;
  if (!sync_all(b)) return -2;
  advance_kv(b);
  if (b->vq_dirty) { update_vq_mode(b); b->vq_dirty = false; }
  const int slot = b->hop_host & 3;
  if (!push_settings(b, slot)) return -2;
  ProfileHook hook;
  hook.repeats = repeats;
  hook.e0 = b->ev0;
  hook.e1 = b->ev1;
  launch_hook() = &hook;
  enqueue_front(b, b->stream);  // one step, eagerly, every stage on the batch's stream
  for (int st = 1; st < b->n_stages; ++st) enqueue_wave(b, st, slot, b->stream);
  launch_hook() = nullptr;
  b->last_parity = b->hop_host % 3;
  b->last_hop = b->hop_host;
  b->hop_host = hop_next(b->hop_host);
  if (b->io_slots > 0) b->io_host = (b->io_host + 1) % b->io_slots;
  b->steps_enqueued += 1;
  if (!hook.ok || !sync_all(b)) return -2;
  const int n = std::min<int>((int)hook.rows.size(), max_entries);
  for (int i = 0; i < n; ++i) {
    std::memset(names + 64 * i, 0, 64);
    std::strncpy(names + 64 * i, hook.rows[i].name.c_str(), 63);
    launches[i] = hook.rows[i].launches;
    mean_us[i] = hook.rows[i].us / hook.rows[i].launches;
    flops[i] = hook.rows[i].flops;
    bytes[i] = hook.rows[i].bytes;
  }
  return n;
}

int BeatriceBatch_TimeSteps(BeatriceBatch* b, int steps, float* ms) {
  BATCH_ENTER(b, Entry::TimeSteps);
  if (steps < 1 || !ms) return -1;
  bool ok = sync_all(b) && hip_ok(hipEventRecord(b->ev0, b->stream), "ev0");
  for (int i = 0; i < steps && ok; ++i) ok = step_device(b, nullptr, nullptr);
  ok = ok && hip_ok(hipEventRecord(b->ev1, wave_stream(b)), "ev1") && hip_ok(hipEventSynchronize(b->ev1), "evsync") &&
       hip_ok(hipEventElapsedTime(ms, b->ev0, b->ev1), "elapsed");
  return (sync_all(b) && ok) ? 0 : -2;
}

}  // extern "C"
