// tick_reset.hip.h -- a stream starts over INSIDE the tick pipeline (BeatriceBatch_ResetStreamInFlight, batch_tick.hip.h).
// (Included by tick.hip.h; not a stand-alone header.)
//
// In tick mode stage s works on the step fed s ticks earlier, so a stream's state is not "at" one step: every ring belongs to the
// stage that writes it and the stage that reads it.  A reset that applies to step k therefore reaches stage s just before tick
// k + s: the host (tick_run) keeps the resets that are travelling and, in front of the tick launch of every tick that needs it,
// enqueues ring_reset_kernel with the pieces to clear before THAT tick.  Ticks with no reset travelling launch nothing.
//
//   * a ring written by stage p and read, with history, by stage p + 1: at tick k + p the producer writes step k's frames while the
//     consumer, in the same launch, still reads step k - 1's history -- the ring is cleared between ticks k + p and k + p + 1, and
//     the clear spares the slot step k has just written (ring_pos at the stream's own counter for that step);
//   * state one stage updates in place (the audio rings, the three parts of the tail's history block, the pitch head's previous
//     bin): cleared whole right before that stage's tick of step k;
//   * the two GRU state rings have NO window: the cell of step k (stage g) reads the last frame of step k - 1 in the same launch in
//     which the next stage (phone.out; pitch.out, and the pitch head one more tick on) reads that very frame as step k - 1's own.
//     The tick runs the cell on the old state; between ticks k + g and k + g + 1 -- before any reader of step k's state -- the cell
//     of that stream is run again from a zero state (gru_restart_kernel: the tick's own cell body on a one-stream view of the rings,
//     the previous frame saved, zeroed and put back around it);
//   * outputs without history (read at the step's own frames only) need nothing;
//   * around the resident 48 kHz blocks (mode F) the stream's Wrap48State belongs to no stage: the wrapper launch in front of tick k
//     reads and writes the input half's history for step k, and the launch in front of tick k + stages (or the flush of a drain)
//     runs step k's OUTPUT half -- one launch behind the step's last stage.  Each part is cleared whole in front of the wrapper launch
//     that uses it for step k; every form of wrap48_tick_kernel holds the state in registers during a launch, so no body of it knows
//     about resets (batch_tick.hip.h tick_reset_wrap48).  The 30 floats of the history go ring_reset_kernel's scalar way.
// The (ring -> clear-before-stage, spare?) table is built in batch_tick.hip.h tick_reset_prepare.
#pragma once

namespace tick {

// a piece of per-stream state: stream b's part is m slots of slot_floats floats at base + b * stride
struct ResetRing { float* base; unsigned stride; unsigned slot_floats; int m; };
// one piece to clear: every slot of rings[ring] of `stream` but slot `spare` (-1: all of them)
struct ResetItem { int ring, stream, spare, pad; };

// One workgroup per (ring, stream) piece of the tick's work list; the list sits in PINNED HOST memory (a StagedRing entry written by
// tick_run, like the per-stream counters of ragged steps), so the host may run ahead of the device.  16-byte stores wherever the piece
// allows them (every ring does; the single word of the pitch head's previous bin goes the scalar way, and so do the parts of a
// Wrap48State that are no multiple of four floats or, in every other stream's 1 144 bytes, do not start on a 16-byte boundary).
static __global__ __launch_bounds__(256) void ring_reset_kernel(const ResetRing* __restrict__ rings, const int n_rings, const ResetItem* __restrict__ items, const int n_streams) {
  const ResetItem it = items[blockIdx.x];
  if (it.ring < 0 || it.ring >= n_rings || it.stream < 0 || it.stream >= n_streams) return;
  const ResetRing r = rings[it.ring];
  float* p = r.base + (size_t)it.stream * r.stride;
  const unsigned n = r.slot_floats * (unsigned)r.m;
  const unsigned lo = it.spare >= 0 && it.spare < r.m ? (unsigned)it.spare * r.slot_floats : n;
  const unsigned hi = lo < n ? lo + r.slot_floats : n;
  if ((r.slot_floats & 3u) == 0 && (reinterpret_cast<unsigned long long>(p) & 15ull) == 0) {
    uint4* q = reinterpret_cast<uint4*>(p);
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (unsigned i = threadIdx.x; i < n / 4; i += 256) if (4 * i < lo || 4 * i >= hi) q[i] = z;
  } else {
    for (unsigned i = threadIdx.x; i < n; i += 256) if (i < lo || i >= hi) p[i] = 0.0f;
  }
}

// The GRU cell of one stream run again from a zero state (see above).  items[i] = {stream, the stream's counter of the step}; phase
// kGruSave: the frame before the step's first (the state the tick's cell started from) -> keep[stream], then zeroed; phase t >= 0:
// the cell of hop t of the step, as the in-order chain runs it (previous state = frame t - 1 of the ring); phase kGruRestore: the
// saved frame back (stages further on still read it as the step before's own).  Grid (items, HID / 16), one launch per phase.
constexpr int kGruSave = -1, kGruRestore = -2;
template <int IN, int HID>
static __global__ __launch_bounds__(384) void gru_restart_kernel(const GruArgs a, const int2* __restrict__ items, float* __restrict__ keep, const int phase) {
  __shared__ __attribute__((aligned(16))) float lds[16 * (IN + 2) + 16 * (HID + 2) + 6 * 256];
  const int2 it = items[blockIdx.x];
  if (it.x < 0 || it.x >= a.B || it.y < 0) return;
  GruArgs g = a;
  g.x.base += (size_t)it.x * ring_stream_floats(a.x);
  g.h.base += (size_t)it.x * ring_stream_floats(a.h);
  g.B = 1; g.link_out = nullptr; g.link_in = nullptr; g.link_dead = nullptr; g.passes = 1;
  if (phase < 0) {
    if (blockIdx.y != 0) return;
    float* f = ring_frame(g.h, 0, ring_pos(g.h, it.y), -1);
    float* kp = keep + (size_t)it.x * HID;
    for (int i = threadIdx.x; i < HID; i += 384) {
      if (phase == kGruSave) { kp[i] = f[i]; f[i] = 0.0f; }
      else f[i] = kp[i];
    }
    return;
  }
  g.t = phase;
  g.hop = stepc::immediate(it.y);
  gru_fused_body<IN, HID, 1, false, 0>(g, 0, blockIdx.y, lds);
}

}  // namespace tick
