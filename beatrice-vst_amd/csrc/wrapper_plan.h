// wrapper_plan.h -- everything about a call of the any-rate wrapper (wrapper.hip.h, batch_wrappers.hip.h) that is a function of numbers the
// host already has: the rate's ratio and tap tables, the two fractional clocks of the resampler pair, how many 48 kHz samples a block
// yields, where the 480-sample FIFO cuts them and when a model hop fires, each stream's gain segment.  Plain C++17, no HIP:
// tests/test_cpu_wrapper_plan.py compiles it with g++ into a driver of its own and holds it against the oracle's restatement of the same
// clocks (oracle/wrapper_oracle.c).  The four ways of driving the wrapper plan a call here, commit, and launch.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace wrapn {

constexpr int kTapsPerOutput = 32;   // filter length in low-rate samples (reference resample.h:415)
constexpr int kBlock = 480;          // 10 ms at 48 kHz
constexpr int kMaxSamples = 4096;    // largest host block per call
constexpr int kMaxChunks = 12;      // FIFO pieces one call can cut its inner samples into: ceil(4096 / 480) + 2
constexpr int kMaxHist = kTapsPerOutput * 8 + 1;   // history of the high-rate side: 32 * hi / lo + 1, host rates up to 384 kHz

struct GainSeg { double amp0, goal, step; };   // per stream and call: amplitude before the first sample, goal, per-sample factor
                                                // (step > 1 ramps up, < 1 down, == 1: constant amp0)

// what a resampling direction needs for one call (identical for every stream)
struct Dir {
  int decimate;      // 1: high -> low rate (reference Downsample), 0: low -> high (Upsample)
  int hi, lo;        // rate ratio
  int phase0;        // the direction's fractional clock before the call
  int n_in, n_out;
  int n_taps;        // table length (32 * hi + 1)
  int hist;          // history length kept between calls
  float scale;       // Downsample's make-up gain lo / hi
};

// smallest-denominator search on the Stern-Brocot tree, parts < 1000 (reference resample.h:25-46)
inline void simple_fraction(double ratio, int* numer, int* denom) {
  int a = 0, b = 1, c = 1, d = 0;
  for (;;) {
    const int mn = a + c, md = b + d;
    const bool big = mn >= 1000 || md >= 1000;
    if (ratio * md < mn) {
      if (big) { *numer = a; *denom = b; return; }
      c = mn; d = md;
    } else {
      if (big) { *numer = c; *denom = d; return; }
      a = mn; b = md;
    }
  }
}

// what moves with every call: the two fractional clocks of the resampler pair and the samples waiting in the 480-sample FIFO
struct Clocks { int phase_down, phase_up, fill; };

// what a host rate fixes: the ratio and the two tap tables.  Streams of equal rate share one; a call only reads it.
struct RateClass {
  bool ready = false, high_is_outer = true;
  double rate = 0.0;
  int hi = 1, lo = 1;
  std::vector<float> taps_down, taps_up;
  int hist_high() const { return kTapsPerOutput * hi / lo + 1; }
  int hist_low() const { return kTapsPerOutput + 1; }
  Clocks start() const { return Clocks{hi - 1, hi - 1, 0}; }   // a stream after SetSampleRate
  // reference resample.h:209-237 with the cutoffs of :412-417
  bool configure(double sr) {
    ready = false;
    rate = sr;
    if (!(sr > 0.0)) return false;
    const double inner = 48000.0, pi = 3.14159265358979323846;
    const double cutoff_in = 0.99 * 16000.0 / std::fmin(std::fmax(sr, 16000.0), 48000.0), cutoff_out = 0.99 * 24000.0 / std::fmin(std::fmax(sr, 24000.0), 48000.0);
    high_is_outer = sr >= inner;
    const double high = high_is_outer ? sr : inner, low = high_is_outer ? inner : sr;
    const double cut_down = high_is_outer ? cutoff_in : cutoff_out, cut_up = high_is_outer ? cutoff_out : cutoff_in;
    simple_fraction(high / low, &hi, &lo);
    if (hi == 0 || lo == 0 || hist_high() > kMaxHist) return false;
    const int n = kTapsPerOutput * hi + 1, mid = n / 2;
    taps_down.resize(n);
    taps_up.resize(n);
    auto sinc = [pi](double x) { return std::abs(x) < 1e-8 ? 1.0 : std::sin(x * pi) / (x * pi); };
    for (int i = 0; i < n; ++i) {
      const double x = static_cast<double>(i - mid) / static_cast<double>(hi);
      const double hann = 0.5 - 0.5 * std::cos(pi * 2.0 / static_cast<double>(n - 1) * static_cast<double>(i));
      taps_down[i] = static_cast<float>(cut_down * sinc(x * cut_down) * hann);
      taps_up[i] = static_cast<float>(cut_up * sinc(x * cut_up) * hann);
    }
    ready = true;
    return true;
  }
};

// One direction of the pair for a call of n_in samples; advances that direction's clock.  Downsample: reference resample.h:130-159
inline Dir downsample(const RateClass& c, Clocks& k, int n_in) {
  Dir d{};
  d.decimate = 1; d.hi = c.hi; d.lo = c.lo; d.phase0 = k.phase_down; d.n_in = n_in; d.n_taps = (int)c.taps_down.size(); d.hist = c.hist_high();
  d.scale = static_cast<float>(c.lo) / static_cast<float>(c.hi);
  const long long total = k.phase_down + (long long)n_in * c.lo;
  d.n_out = (int)(total / c.hi);
  k.phase_down = (int)(total % c.hi);
  return d;
}
// Upsample (:168-206); how many samples come out is the caller's to derive from the clocks
inline Dir upsample(const RateClass& c, Clocks& k, int n_in, long long n_out) {
  Dir d{};
  d.decimate = 0; d.hi = c.hi; d.lo = c.lo; d.phase0 = k.phase_up; d.n_in = n_in; d.n_out = (int)n_out; d.n_taps = (int)c.taps_up.size(); d.hist = c.hist_low();
  d.scale = 1.0f;
  k.phase_up = (int)((k.phase_up + (long long)d.n_out * c.lo) % c.hi);
  return d;
}
// the direction host -> 48 kHz for a block of n host samples
inline Dir to_inner(const RateClass& c, Clocks& k, int n) {
  return c.high_is_outer ? downsample(c, k, n) : upsample(c, k, n, (((long long)n + 1) * c.hi - k.phase_up - 1) / c.lo);
}
// the direction 48 kHz -> host for m inner samples; towards a higher host rate the count couples the two clocks (reference resample.h:171-177)
inline Dir to_outer(const RateClass& c, Clocks& k, int m) {
  return c.high_is_outer ? upsample(c, k, m, ((long long)m * c.hi + k.phase_down - k.phase_up) / c.lo) : downsample(c, k, m);
}

// The exact-480 FIFO (reference resample.h:343-363) on m inner samples: piece i swaps inner samples [at, at + take) with FIFO positions
// [fill, fill + take); a model hop fires every time that completes the block.  false: more pieces than the kernels' records hold.
struct FifoCut {
  int n, fill_after;
  short at[kMaxChunks], fill[kMaxChunks], take[kMaxChunks];
  unsigned char fires[kMaxChunks];
  template <class Rec> void put(Rec& q) const {   // into the record a launch reads (WrapCallArgs, RagStream)
    q.n_chunks = n;
    std::memcpy(q.at, at, sizeof(at)); std::memcpy(q.fill, fill, sizeof(fill)); std::memcpy(q.take, take, sizeof(take)); std::memcpy(q.fires, fires, sizeof(fires));
  }
};
inline bool fifo_cut(int fill, int m, FifoCut& c) {
  c = FifoCut{};   // (the pieces a call does not have are zeros in the kernels' records)
  for (int at = 0; at < m;) {
    const int take = std::min(kBlock - fill, m - at);
    if (c.n >= kMaxChunks) return false;
    c.at[c.n] = (short)at; c.fill[c.n] = (short)fill; c.take[c.n] = (short)take;
    c.fires[c.n] = fill + take == kBlock ? 1 : 0;
    fill = c.fires[c.n] ? 0 : fill + take;
    at += take;
    ++c.n;
  }
  c.fill_after = fill;
  return true;
}

// the reference's gain context (gain.h:19-72), per stream, on the host: now in dB as a double
struct GainClock {
  double target_db = 0.0, now_db = 0.0;
  static double db_to_amp(double db) { return std::pow(10.0, db * 0.05); }
  // this call's segment + the state after n samples (the same loop the host layer's GainRamp::Apply runs, without data)
  GainSeg advance(int n, double rate) {
    const double goal = db_to_amp(target_db);
    double amp = db_to_amp(now_db);
    GainSeg g{amp, goal, 1.0};
    const double per_sample_db = 2.0 / (rate * 0.001);
    int i = 0;
    if (amp < goal) {
      g.step = db_to_amp(per_sample_db);
      while (i < n && amp < goal) { amp = std::fmin(amp * g.step, goal); ++i; }
    } else if (amp > goal) {
      g.step = db_to_amp(-per_sample_db);
      while (i < n && amp > goal) { amp = std::fmax(amp * g.step, goal); ++i; }
    }
    now_db = 20.0 * std::log10(amp);
    return g;
  }
};

// A block of n host samples through the clocks: the two directions and the cut between them.  Computed on a copy; the clocks move only
// when the plan fits the kernels' buffers and the block comes back with its own length (the two clocks are coupled so that it does).
struct ClockPlan { Dir din, dout; FifoCut cut; };
inline bool plan_clocks(const RateClass& c, Clocks& k, int n, ClockPlan& p) {
  Clocks next = k;
  p.din = to_inner(c, next, n);
  const int m = p.din.n_out;
  if (m < 0 || m > kMaxSamples || !fifo_cut(next.fill, m, p.cut)) return false;
  next.fill = p.cut.fill_after;
  p.dout = to_outer(c, next, m);
  if (p.dout.n_out != n) return false;
  k = next;
  return true;
}
// ... and one stream's whole share of a call: its gain segments too.  A refusal leaves the clocks and both gain clocks as they were.
struct CallPlan : ClockPlan { GainSeg gain_in, gain_out; };
inline bool plan_call(const RateClass& c, Clocks& k, GainClock& gain_in, GainClock& gain_out, int n, CallPlan& p) {
  if (!plan_clocks(c, k, n, p)) return false;
  p.gain_in = gain_in.advance(n, c.rate);
  p.gain_out = gain_out.advance(n, c.rate);
  return true;
}
// A call with clocks per stream is all or nothing: its streams are planned on the state the call would leave, which becomes the batch's
// only when every stream's plan stands -- otherwise host and device state of the streams planned before the refusal would part ways.
struct CallPlanner {
  std::vector<Clocks> clk;
  std::vector<GainClock> gain_in, gain_out;
  void begin(const std::vector<Clocks>& k, const std::vector<GainClock>& gi, const std::vector<GainClock>& go) { clk = k; gain_in = gi; gain_out = go; }
  bool plan(const RateClass& c, int s, int n, CallPlan& p) { return plan_call(c, clk[s], gain_in[s], gain_out[s], n, p); }
  void commit(std::vector<Clocks>& k, std::vector<GainClock>& gi, std::vector<GainClock>& go) { k.swap(clk); gi.swap(gain_in); go.swap(gain_out); }
};

// host samples per call so that neither side exceeds the kernels' LDS buffers
inline int longest_block(double rate) { return std::max(1, (int)std::floor((kMaxSamples - 8) * std::min(1.0, rate / 48000.0))); }
// model hops a call of n host samples can fire: ceil(inner samples / 480) + 1
inline int most_hops(int n, double rate) { return ((int)std::ceil(n * 48000.0 / rate) + 2 + kBlock - 1) / kBlock + 1; }

}  // namespace wrapn
