"""The any-rate wrapper's host-side plan (beatrice-vst_amd/csrc/wrapper_plan.h) without a GPU.  The header is plain C++17 without HIP: a
stand-alone driver with its own main is compiled against it with g++ under the address and undefined-behaviour sanitizers and walks
scripts of calls -- block lengths, gain targets set before given calls -- through the same plan / commit path the batch's steppers use.
The yardstick is the oracle's restatement of the same clocks (oracle/libwrapper_oracle.so, pinned to the reference by
tests/test_wrapper_oracle.py): one oracle processor per stream, a hop callback that only counts.  After every call the hops fired, the
FIFO fill and both gains' target and present value must be EQUAL -- the integers as integers, the doubles bit for bit (both sides run
the same double recurrence on the same libm)."""
import ctypes as C
import math
import os
import random
import subprocess

import numpy as np
import pytest

import wrapperlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import wrapper_edge_cases

# ... and the rates of tests/wrapper_edge_cases.py: ratios 4, 6 and 8 on both sides of 48 kHz, tables beyond 7168 taps, truncated fractions
RATES = [16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000] + [r for r in wrapper_edge_cases.RATES if r not in (22050.0, 48000.0)]
_f32p = C.POINTER(C.c_float)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "wrapper_plan.h"
using namespace wrapn;

static void print_cut(const FifoCut& c) {
  int hops = 0;
  for (int i = 0; i < c.n; ++i) hops += c.fires[i];
  std::printf(" hops %d fill %d pieces %d", hops, c.fill_after, c.n);
  for (int i = 0; i < c.n; ++i) std::printf(" %d:%d:%d:%d", c.at[i], c.fill[i], c.take[i], c.fires[i]);
}
static void print_plan(int s, int n, const CallPlan& p) {
  std::printf("plan %d n %d m %d out %d", s, n, p.din.n_out, p.dout.n_out);
  print_cut(p.cut);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<RateClass> cls;
  std::vector<Clocks> clk;
  std::vector<GainClock> gin, gout;
  CallPlanner next;
  auto state = [&]() {
    for (size_t s = 0; s < cls.size(); ++s)
      std::printf("state %zu %d %d %d %a %a %a %a\n", s, clk[s].phase_down, clk[s].phase_up, clk[s].fill, gin[s].target_db, gin[s].now_db,
                  gout[s].target_db, gout[s].now_db);
  };
  char word[32], num[64];
  while (std::fscanf(f, "%31s", word) == 1) {
    if (!std::strcmp(word, "configure")) {          // a rate a class is asked to take: refused, or its ratio
      if (std::fscanf(f, "%63s", num) != 1) return 2;
      RateClass c;
      const bool ok = c.configure(std::strtod(num, nullptr));
      if (ok) std::printf("configure 1 %d %d %d %d\n", c.hi, c.lo, (int)c.taps_down.size(), (int)c.taps_up.size());
      else std::printf("configure 0\n");
    } else if (!std::strcmp(word, "fraction")) {
      int a = -1, b = -1;
      if (std::fscanf(f, "%63s", num) != 1) return 2;
      simple_fraction(std::strtod(num, nullptr), &a, &b);
      std::printf("fraction %d %d\n", a, b);
    } else if (!std::strcmp(word, "longest")) {
      if (std::fscanf(f, "%63s", num) != 1) return 2;
      std::printf("longest %d\n", longest_block(std::strtod(num, nullptr)));
    } else if (!std::strcmp(word, "most_hops")) {
      int n;
      if (std::fscanf(f, "%d %63s", &n, num) != 2) return 2;
      std::printf("most_hops %d\n", most_hops(n, std::strtod(num, nullptr)));
    } else if (!std::strcmp(word, "cut")) {          // the FIFO cut alone
      int fill, m;
      if (std::fscanf(f, "%d %d", &fill, &m) != 2) return 2;
      FifoCut c;
      if (fifo_cut(fill, m, c)) { std::printf("cut 1"); print_cut(c); std::printf("\n"); }
      else std::printf("cut 0\n");
    } else if (!std::strcmp(word, "stream")) {       // one more stream, as after SetSampleRate
      if (std::fscanf(f, "%63s", num) != 1) return 2;
      RateClass c;
      if (!c.configure(std::strtod(num, nullptr))) return 3;
      cls.push_back(c); clk.push_back(c.start()); gin.push_back(GainClock()); gout.push_back(GainClock());
      std::printf("stream %d %d\n", c.hi, c.lo);
    } else if (!std::strcmp(word, "gain_in") || !std::strcmp(word, "gain_out")) {
      int s;
      if (std::fscanf(f, "%d %63s", &s, num) != 2 || s < 0 || s >= (int)cls.size()) return 2;
      (word[5] == 'i' ? gin : gout)[s].target_db = std::strtod(num, nullptr);
    } else if (!std::strcmp(word, "call")) {         // a block per stream (0: the stream sits the call out), all or nothing
      std::vector<int> n(cls.size());
      for (int& v : n) if (std::fscanf(f, "%d", &v) != 1) return 2;
      std::vector<CallPlan> plans(cls.size());
      next.begin(clk, gin, gout);
      bool ok = true;
      for (size_t s = 0; s < cls.size() && ok; ++s) if (n[s] > 0) ok = next.plan(cls[s], (int)s, n[s], plans[s]);
      if (ok) next.commit(clk, gin, gout);
      std::printf("call %d\n", ok ? 1 : 0);
      for (size_t s = 0; s < cls.size() && ok; ++s) if (n[s] > 0) print_plan((int)s, n[s], plans[s]);
      state();
    } else if (!std::strcmp(word, "direct")) {       // the plan function itself on the stream's own state
      int s, n;
      if (std::fscanf(f, "%d %d", &s, &n) != 2 || s < 0 || s >= (int)cls.size()) return 2;
      CallPlan p;
      const bool ok = plan_call(cls[s], clk[s], gin[s], gout[s], n, p);
      std::printf("call %d\n", ok ? 1 : 0);
      if (ok) print_plan(s, n, p);
      state();
    } else {
      return 2;
    }
  }
  std::fclose(f);
  std::printf("end\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("wrapper_plan")
    src = d / "wrapper_plan_driver.cc"
    src.write_text(DRIVER)
    exe = d / "wrapper_plan_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "beatrice-vst_amd", "csrc"),
                    "-o", str(exe), str(src)], check=True)

    def run(script):
        path = d / "script.txt"
        path.write_text("\n".join(script) + "\n")
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.endswith("end\n"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return [line.split() for line in r.stdout.splitlines()[:-1]]
    return run


@pytest.fixture(scope="module")
def wo():
    if not os.path.exists(wrapperlib.ORACLE_WRAPPER):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "oracle"), "libwrapper_oracle.so"], env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    return wrapperlib.oracle_wrapper()


def longest(rate):
    """the longest block at a rate, from what it is for: neither side of the first direction above the kernels' 4096 - 8 samples"""
    return max(1, math.floor((4096 - 8) * min(1.0, rate / 48000.0)))


class OracleStream:
    """one oracle processor: blocks of zeros go in, the hops are counted"""
    def __init__(self, wo, rate):
        self.wo, self.hops = wo, 0

        def hop(_in160, _out240, _user):
            self.hops += 1
        self.cb = wrapperlib.HOP_FN(hop)
        self.p = wo.f_create(float(rate), self.cb, None)
        self.x = np.zeros(8192, np.float32)
        self.y = np.zeros(8192, np.float32)

    def gain(self, which, db):
        (self.wo.f_in_gain if which == "gain_in" else self.wo.f_out_gain)(self.p, db)

    def call(self, n):
        """-> (hops fired in the call, fill after, (input target, input now, output target, output now))"""
        before = self.hops
        assert self.wo.f_process(self.p, self.x.ctypes.data_as(_f32p), self.y.ctypes.data_as(_f32p), n) == 0
        return self.hops - before, self.wo.f_fifo_fill(self.p), self.wo.gain_state(self.p)

    def state(self):
        return self.wo.f_fifo_fill(self.p), self.wo.gain_state(self.p)

    def close(self):
        self.wo.f_destroy(self.p)


def check_plan(line, s, n):
    """a `plan` line of the driver: the stream, its block, and the pieces as the kernels need them -> (inner samples, hops, fill after)"""
    assert line[0] == "plan" and int(line[1]) == s and int(line[3]) == n, line
    m, out, hops, fill, k = int(line[5]), int(line[7]), int(line[9]), int(line[11]), int(line[13])
    assert out == n, line                                   # a block comes back with its own length
    pieces = [tuple(int(v) for v in p.split(":")) for p in line[14:]]
    assert len(pieces) == k and k <= 12
    at = 0
    for i, (a, f, take, fires) in enumerate(pieces):       # consecutive, inside the FIFO, a hop exactly when it fills
        assert a == at and take >= 1 and 0 <= f and f + take <= 480 and fires == (1 if f + take == 480 else 0), line
        assert i == 0 or (pieces[i - 1][3] == 1 and f == 0), line
        at += take
    assert at == m and sum(p[3] for p in pieces) == hops
    if pieces:
        assert fill == (0 if pieces[-1][3] else pieces[-1][1] + pieces[-1][2]), line
    return m, hops, fill


def check_state(line, s, fill, gains):
    assert line[0] == "state" and int(line[1]) == s, line
    assert int(line[4]) == fill, (line, fill)
    got = tuple(float.fromhex(v) for v in line[5:9])
    assert [g.hex() for g in got] == [w.hex() for w in gains], (line, [w.hex() for w in gains])   # bit for bit


def lengths_for(rate, hi):
    """1, 97, 480, the longest block at the rate, and a seeded sequence of mixed lengths: long enough that both fractional clocks wrap
    (>= 2 hi host samples) and that at least 30 hops fire"""
    L = longest(rate)
    rng = random.Random(1000 + rate)
    n_longest = max(6, math.ceil(20 * 480 * max(1.0, rate / 48000.0) / L))   # (six up to 96 kHz; above, a block is few inner samples: 20 hops' worth)
    return [1] * max(2 * hi, 600) + [97] * 40 + [480] * 12 + [L] * n_longest + [rng.choice([1, 2, 7, 97, 441, 480, 512, L, rng.randint(1, L)]) for _ in range(40)]


@pytest.mark.parametrize("rate", RATES)
def test_one_stream_against_the_oracle(driver, wo, rate):
    hi = max(wo.fraction(max(rate, 48000) / min(rate, 48000)))
    ns = lengths_for(rate, hi)
    first97 = ns.index(97)
    first480 = ns.index(480)
    # a ramp that spans several calls (and, for the short blocks, ends inside one), a target changed in the middle of a ramp, a ramp that
    # ends inside a call, and -- below -- a target equal to the present value, in the middle of a ramp and at rest
    events = {10: [("gain_in", -12.0)], 50: [("gain_in", 3.0)], first97: [("gain_out", -60.0)], first97 + 3: [("gain_out", 0.0)],
              first97 + 8: [("gain_in", -40.0)], first480 + 2: [("gain_out", -6.0)], first480 + 6: [("gain_in", -40.0)]}
    # (the 43 dB towards -40 dB take 21.5 ms: two 97-sample calls from 16 kHz up, one call -- 16 ms at 6 kHz -- below)
    mid_ramp = first97 + (10 if rate >= 16000 else 9)
    present = {mid_ramp: "gain_in", first480 + 4: "gain_out"}
    o = OracleStream(wo, rate)
    script, want = ["longest %r" % float(rate), "stream %r" % float(rate)], []
    for i, n in enumerate(ns):
        for which, db in events.get(i, []):
            o.gain(which, db)
            script.append("%s 0 %s" % (which, float(db).hex()))
        if i in present:
            g = o.state()[1]
            db = g[1] if present[i] == "gain_in" else g[3]
            if i == mid_ramp:
                assert g[0] != g[1]   # (the ramp towards -40 dB is still under way)
            o.gain(present[i], db)
            script.append("%s 0 %s" % (present[i], db.hex()))
        script.append("call %d" % n)
        want.append(o.call(n))
    o.close()
    out = driver(script)
    assert out[0] == ["longest", str(longest(rate))]
    assert out[1][0] == "stream" and int(out[1][1]) == hi
    assert sum(ns) >= 2 * hi and sum(w[0] for w in want) >= 30
    assert len(out) == 2 + 3 * len(ns)
    for i, (n, (hops, fill, gains)) in enumerate(zip(ns, want)):
        call, plan, state = out[2 + 3 * i: 5 + 3 * i]
        assert call == ["call", "1"], (i, n, call)
        m, got_hops, got_fill = check_plan(plan, 0, n)
        assert (got_hops, got_fill) == (hops, fill), (i, n, plan, hops, fill)
        check_state(state, 0, fill, gains)


def test_streams_of_different_rates_in_one_call_and_one_that_sits_out(driver, wo):
    """Several streams through the commit path of BeatriceBatch_ProcessBlocksRagged: every stream equals its own oracle, whatever the
    others do; a stream without a block (n = 0) does not move -- neither its clocks nor its gains, whose targets were just changed."""
    rates = [44100, 48000, 96000, 22050, 16000]
    rng = random.Random(7)
    streams = [OracleStream(wo, r) for r in rates]
    script = ["stream %r" % float(r) for r in rates]
    want, calls = [], []
    for k in range(60):
        n = [rng.choice([0, 1, 97, 300, 480, rng.randint(1, longest(r))]) for r in rates]
        if k % 4 == 1:
            n[1] = 0
        if k in (3, 9, 20, 21, 40):
            for s in range(len(rates)):
                db = rng.choice([-30.0, -6.0, 0.0, 4.5])
                which = rng.choice(["gain_in", "gain_out"])
                streams[s].gain(which, db)
                script.append("%s %d %s" % (which, s, float(db).hex()))
        script.append("call " + " ".join(str(v) for v in n))
        calls.append(n)
        want.append([o.call(v) if v > 0 else (0,) + o.state() for o, v in zip(streams, n)])
    assert any(n[1] == 0 and w[1][2][0] != w[1][2][1] for n, w in zip(calls, want))   # it sat a call out with a ramp under way
    out = driver(script)[len(rates):]
    at = 0
    for n, w in zip(calls, want):
        assert out[at] == ["call", "1"]
        at += 1
        for s, v in enumerate(n):
            if v > 0:
                _, hops, fill = check_plan(out[at], s, v)
                assert (hops, fill) == w[s][:2]
                at += 1
        for s in range(len(rates)):
            check_state(out[at], s, w[s][1], w[s][2])
            at += 1
    assert at == len(out)
    for o in streams:
        o.close()


def test_a_refused_call_moves_nothing(driver, wo):
    """All or nothing: a later stream's block that the plan must refuse (96 kHz, far above the longest block: the entry points' own range
    check would stop it earlier) leaves the clocks and gain clocks of EVERY stream of the call bit-equal to before -- those planned before
    it too, with their ramps under way; so does the plan function itself, handed that block.  The streams go on equal to their oracles."""
    rates = [44100, 96000, 16000]
    streams = [OracleStream(wo, r) for r in rates]
    script = ["stream %r" % float(r) for r in rates]
    good = [[300, 777, 100], [1, 480, 97], [441, 960, 160]]
    want = []
    for s in range(3):
        streams[s].gain("gain_in", -60.0)
        streams[s].gain("gain_out", -50.0)
        script += ["gain_in %d %s" % (s, (-60.0).hex()), "gain_out %d %s" % (s, (-50.0).hex())]
    for n in good[:2]:
        script.append("call " + " ".join(map(str, n)))
        want.append([o.call(v) for o, v in zip(streams, n)])
    script += ["call 300 20000 100", "call 300 4088 5000", "direct 1 20000", "direct 2 5000"]
    script.append("call " + " ".join(map(str, good[2])))
    want.append([o.call(v) for o, v in zip(streams, good[2])])
    out = driver(script)[3:]
    blocks, at = [], 0
    while at < len(out):                      # a `call` line, the plans of an accepted call, a `state` line per stream
        assert out[at][0] == "call"
        end = at + 1
        while end < len(out) and out[end][0] != "call":
            end += 1
        blocks.append(out[at:end])
        at = end
    assert [b[0][1] for b in blocks] == ["1", "1", "0", "0", "0", "0", "1"]
    assert all(g[0] != g[1] and g[2] != g[3] for _, _, g in want[1])   # (every ramp under way when the refusals come)
    for b in blocks[2:6]:
        assert len(b) == 4 and b[1:] == blocks[1][-3:], b           # no plan lines; every stream's state as the last good call left it
    for b, w in zip([blocks[0], blocks[1], blocks[6]], want):
        for s in range(3):
            check_state(b[-3 + s], s, w[s][1], w[s][2])
    for o in streams:
        o.close()


def test_what_configure_refuses_and_the_small_quantities(driver, wo):
    """The refusals of RateClass::configure (the list tests/test_gpu_stream_wrapper_lifecycle.py uses on the GPU), simple_fraction against
    the oracle's wo_fraction on the rates of this file, the FIFO cut alone, and the two derived quantities against what they are for."""
    bad = ["0.0", "nan", "1e9", "-44100.0", "inf"]
    script = ["configure " + v for v in bad] + ["configure %r" % float(r) for r in RATES]
    ratios = [max(r, 48000) / min(r, 48000) for r in RATES]
    script += ["fraction " + v.hex() for v in ratios]
    script += ["cut 0 0", "cut 479 1", "cut 1 4096", "cut 479 4096", "cut 479 6000", "cut 0 5760", "cut 0 5761"]
    script += ["longest %r" % float(r) for r in RATES]
    hops_cases = [(n, r) for r in RATES for n in (1, 480, longest(r))]
    script += ["most_hops %d %r" % (n, float(r)) for n, r in hops_cases]
    out = driver(script)
    for line in out[:len(bad)]:
        assert line == ["configure", "0"]
    out = out[len(bad):]
    for r, ratio, line, frac in zip(RATES, ratios, out[:len(RATES)], out[len(RATES):2 * len(RATES)]):
        hi, lo = wo.fraction(ratio)
        assert line == ["configure", "1", str(hi), str(lo), str(32 * hi + 1), str(32 * hi + 1)]
        assert frac == ["fraction", str(hi), str(lo)]
    assert {int(line[2]) for line in out[:len(RATES)]} >= {1, 2, 3, 160, 320}
    out = out[2 * len(RATES):]
    assert out[0] == ["cut", "1", "hops", "0", "fill", "0", "pieces", "0"]
    assert out[1] == ["cut", "1", "hops", "1", "fill", "0", "pieces", "1", "0:479:1:1"]
    assert out[2][:8] == ["cut", "1", "hops", "8", "fill", "257", "pieces", "9"] and out[2][8] == "0:1:479:1" and out[2][-1] == "3839:0:257:0"
    assert out[3][:8] == ["cut", "1", "hops", "9", "fill", "255", "pieces", "10"] and out[3][8] == "0:479:1:1"
    assert out[4] == ["cut", "0"]                                   # more pieces than a call's record holds
    assert out[5][:8] == ["cut", "1", "hops", "12", "fill", "0", "pieces", "12"] and out[6] == ["cut", "0"]
    out = out[7:]
    for r, line in zip(RATES, out):
        assert line == ["longest", str(longest(r))]
        assert math.ceil(longest(r) * 48000 / r) <= 4096 and longest(r) <= 4096 - 8
    out = out[len(RATES):]
    for (n, r), line in zip(hops_cases, out):
        # a call's inner samples are at most ceil(n 48000 / rate) + 1 (the clocks make the count vary by one), and a FIFO that holds f of
        # its 480 samples fires floor((f + m) / 480) times: at most ceil(m / 480) -- what the bound must cover, and by no more than two
        m_max = math.ceil(n * 48000 / r) + 1
        assert -(-m_max // 480) <= int(line[1]) <= -(-m_max // 480) + 2, (n, r, line)
