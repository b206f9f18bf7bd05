"""A CPU witness of the any-rate wrapper's index arithmetic at the rates and blocks of tests/wrapper_edge_cases.py, so that kernel paths no
test has run before do not get their first run as an experiment on a GPU.  A stand-alone C++17 program (its own main, g++ with the address
and undefined-behaviour sanitizers) includes beatrice-vst_amd/csrc/wrapper_plan.h alone, walks every (case, call) of the table through
plan_clocks and, for every output o of both directions, restates resample_one's index walk (csrc/wrapper.hip.h) and checks it against the
kernels' buffers.  It prints what the header derives for every case; this file holds that against the table's own derivation and holds the
COVERAGE CONDITION: every class in every one of the four kernel forms, the boundary pair on the two sides of kTapsLds, a call without an
inner sample and a call with the most FIFO pieces in every form."""
import os
import re
import subprocess

import pytest

import wrapper_edge_cases as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "beatrice-vst_amd", "csrc")

WITNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "wrapper_plan.h"
using namespace wrapn;

static int fails = 0;
#define HOLD(cond, ...) do { if (!(cond)) { ++fails; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Reach { long long x_lo, x_hi, tap_lo, tap_hi, taps_most; };

// resample_one (wrapper.hip.h) without data: the x and tap indices output o of direction d touches
static void walk(const Dir& d, int o, Reach& r) {
  const int last = d.n_taps - 1;
  long long pos, tap, step, count = 0;
  if (d.decimate) {
    const long long need = (long long)(o + 1) * d.hi - d.phase0;
    const int k = (int)((need + d.lo - 1) / d.lo);
    const int ph = (int)(d.phase0 + (long long)k * d.lo - (long long)(o + 1) * d.hi);
    pos = d.hist + k - 1; tap = d.lo - ph; step = d.lo;
  } else {
    const long long clock = d.phase0 + (long long)(o + 1) * d.lo;
    pos = d.hist + (int)(clock / d.hi) - 1; tap = (int)(clock % d.hi); step = d.hi;
  }
  for (; tap < last; tap += step) {
    if (pos > r.x_hi) r.x_hi = pos;
    if (pos < r.x_lo) r.x_lo = pos;
    if (tap > r.tap_hi) r.tap_hi = tap;
    if (tap < r.tap_lo) r.tap_lo = tap;
    --pos; ++count;
  }
  if (count > r.taps_most) r.taps_most = count;
}

// one direction of one call against the kernels' buffers: x[kMaxHist + kMaxSamples] = [hist | n_in], the table, the state block
static void direction(const char* id, int call, const char* which, const Dir& d, const RateClass& c) {
  HOLD(d.n_in >= 0 && d.n_in <= kMaxSamples, "%s call %d %s n_in %d", id, call, which, d.n_in);
  HOLD(d.n_out >= 0 && d.n_out <= kMaxSamples, "%s call %d %s n_out %d", id, call, which, d.n_out);
  HOLD(d.hist >= 1 && d.hist <= kMaxHist && d.hist == (d.decimate ? c.hist_high() : c.hist_low()), "%s call %d %s hist %d", id, call, which, d.hist);
  HOLD(d.hist + d.n_in <= kMaxHist + kMaxSamples, "%s call %d %s hist + n_in %d", id, call, which, d.hist + d.n_in);
  HOLD(d.n_taps == kTapsPerOutput * c.hi + 1 && d.n_taps == (int)(d.decimate ? c.taps_down : c.taps_up).size(), "%s call %d %s n_taps %d", id, call, which, d.n_taps);
  Reach r{1LL << 40, -1, 1LL << 40, -1, 0};
  for (int o = 0; o < d.n_out; ++o) walk(d, o, r);
  if (d.n_out > 0) {
    HOLD(r.x_lo >= 0, "%s call %d %s smallest x index %lld", id, call, which, r.x_lo);
    HOLD(r.x_hi < d.hist + d.n_in, "%s call %d %s largest x index %lld of %d", id, call, which, r.x_hi, d.hist + d.n_in);
    HOLD(r.tap_lo >= 0 && r.tap_hi < d.n_taps, "%s call %d %s taps [%lld, %lld] of %d", id, call, which, r.tap_lo, r.tap_hi, d.n_taps);
    HOLD(r.taps_most <= d.hist, "%s call %d %s %lld taps per output, history %d", id, call, which, r.taps_most, d.hist);
  }
  // the state write-back hist[i] = x[n_in + i], i < hist: the newest `hist` samples
  HOLD(d.n_in >= 0 && d.n_in + d.hist <= d.hist + d.n_in && d.n_in + d.hist <= kMaxHist + kMaxSamples, "%s call %d %s write-back", id, call, which);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  // the most pieces any accepted call can have: a plan of at most kMaxSamples inner samples, whatever the fill
  int most_pieces = 0;
  for (int fill = 0; fill < kBlock; ++fill) {
    FifoCut c;
    HOLD(fifo_cut(fill, kMaxSamples, c), "cut fill %d", fill);
    if (c.n > most_pieces) most_pieces = c.n;
  }
  std::printf("limits %d %d %d %d %d\n", kMaxHist, kMaxSamples, kMaxChunks, kBlock, most_pieces);
  char id[128], num[64];
  int n_calls;
  while (std::fscanf(f, "%127s %63s %d", id, num, &n_calls) == 3) {
    const double rate = std::strtod(num, nullptr);
    RateClass c;
    if (!c.configure(rate)) { std::printf("refused %s %d %d %d\n", id, c.hi, c.lo, c.hist_high()); for (int i = 0, n; i < n_calls; ++i) if (std::fscanf(f, "%d", &n) != 1) return 2; continue; }
    Clocks k = c.start();
    const int longest = longest_block(rate);
    long long sum_m = 0;
    int min_m = 1 << 30, max_m = 0, max_pieces = 0, zero_calls = 0, full_calls = 0, max_hops = 0, hops_cap = 0;
    for (int call = 0; call < n_calls; ++call) {
      int n;
      if (std::fscanf(f, "%d", &n) != 1) return 2;
      HOLD(n >= 1 && n <= longest, "%s call %d n %d longest %d", id, call, n, longest);
      ClockPlan p;
      const bool ok = plan_clocks(c, k, n, p);
      HOLD(ok, "%s call %d n %d: plan refused", id, call, n);
      if (!ok) continue;
      const int m = p.din.n_out;
      HOLD(p.din.n_in == n && p.dout.n_in == m && p.dout.n_out == n, "%s call %d n %d m %d", id, call, n, m);
      HOLD(p.din.decimate == (c.high_is_outer ? 1 : 0) && p.dout.decimate == (c.high_is_outer ? 0 : 1), "%s call %d directions", id, call);
      direction(id, call, "in", p.din, c);
      direction(id, call, "out", p.dout, c);
      HOLD(p.cut.n >= 0 && p.cut.n <= kMaxChunks, "%s call %d pieces %d", id, call, p.cut.n);
      int at = 0, hops = 0;
      for (int i = 0; i < p.cut.n; ++i) {      // the pieces inside the inner samples and inside the FIFO
        HOLD(p.cut.at[i] == at && p.cut.take[i] >= 1 && p.cut.fill[i] >= 0 && p.cut.fill[i] + p.cut.take[i] <= kBlock, "%s call %d piece %d", id, call, i);
        at += p.cut.take[i]; hops += p.cut.fires[i];
      }
      HOLD(at == m, "%s call %d pieces cover %d of %d", id, call, at, m);
      const int cap = most_hops(n, rate);     // what a binding sizes its slot ring by
      HOLD(hops <= cap, "%s call %d hops %d most_hops %d", id, call, hops, cap);
      if (hops > max_hops) max_hops = hops;
      if (cap > hops_cap) hops_cap = cap;
      sum_m += m;
      if (m < min_m) min_m = m;
      if (m > max_m) max_m = m;
      if (p.cut.n > max_pieces) max_pieces = p.cut.n;
      if (m == 0) ++zero_calls;
      if (p.cut.n == most_pieces) ++full_calls;
    }
    std::printf("case %s %d %d %d %d %d %d %d %lld %d %d %d %d %d %d %d\n", id, c.hi, c.lo, (int)c.taps_down.size(), c.hist_high(), c.high_is_outer ? 1 : 0,
                longest, n_calls, sum_m, min_m, max_m, max_pieces, zero_calls, full_calls, max_hops, hops_cap);
  }
  std::fclose(f);
  std::printf("end %d\n", fails);
  return fails ? 1 : 0;
}
"""

FIELDS = ("hi", "lo", "n_taps", "hist", "high_is_outer", "longest", "calls", "sum_m", "min_m", "max_m", "max_pieces", "zero_calls", "full_calls",
          "max_hops", "hops_cap")


def kernel_constant(name, header="wrapper.hip.h"):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr int %s = ([^;]+);" % name, text)
    assert m, name
    return m.group(1)


@pytest.fixture(scope="module")
def witness(tmp_path_factory):
    d = tmp_path_factory.mktemp("wrapper_edge_witness")
    src, exe, script = d / "witness.cc", d / "witness", d / "cases.txt"
    src.write_text(WITNESS)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    lines = ["%s %r %d %s" % (c.id, c.rate, len(c.blocks), " ".join(map(str, c.blocks))) for c in E.CASES]
    lines += ["turnover-leg-%d %r %d %s" % (i, rate, len(blocks), " ".join(map(str, blocks))) for i, (rate, blocks) in enumerate(E.TURNOVER_LEGS)]
    lines += ["refused-%g %r 1 1" % (rate, rate) for rate in E.REFUSED_RATES]
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "end 0", (r.returncode, "\n".join(line for line in out if line.startswith("FAIL"))[:4000], r.stderr[-4000:])
    res = {"limits": [int(v) for v in out[0].split()[1:]], "case": {}, "refused": {}}
    for line in out[1:-1]:
        w = line.split()
        if w[0] == "case":
            res["case"][w[1]] = dict(zip(FIELDS, (int(v) for v in w[2:])))
        else:
            assert w[0] == "refused", line
            res["refused"][w[1]] = tuple(int(v) for v in w[2:])
    return res


def test_the_index_walk_stays_inside_the_kernels_buffers_and_the_header_derives_what_the_table_states(witness):
    """(the bounds themselves are held by the program: it ends with `end 0`, no FAIL line and no sanitizer report)"""
    max_hist, max_samples, max_chunks, block, most_pieces = witness["limits"]
    assert (max_hist, max_samples, max_chunks, block) == (E.MAX_HIST, E.MAX_SAMPLES, E.MAX_CHUNKS, E.BLOCK)
    assert int(kernel_constant("kTapsLds")) == E.TAPS_LDS
    # 4096 inner samples behind a FIFO that lacks one sample: 1 + 8 x 480 + 255 -> ten pieces; the records hold twelve
    assert most_pieces == 10 <= max_chunks
    assert len(witness["case"]) == len(E.CASES) + len(E.TURNOVER_LEGS)
    for c in E.CASES:
        got, r, k = witness["case"][c.id], E.Rate(c.rate), E.Clocks(E.Rate(c.rate))
        assert r.accepted and (r.hi, r.lo) == E.RATES[c.rate], c.id                # the fractions the table states
        plan = [k.call(n) for n in c.blocks]
        want = dict(hi=r.hi, lo=r.lo, n_taps=r.n_taps, hist=r.hist, high_is_outer=int(r.high_is_outer), longest=r.longest, calls=len(c.blocks),
                    sum_m=sum(m for m, _ in plan), min_m=min(m for m, _ in plan), max_m=max(m for m, _ in plan), max_pieces=max(p for _, p in plan),
                    zero_calls=sum(1 for m, _ in plan if m == 0), full_calls=sum(1 for _, p in plan if p == most_pieces))
        assert {f: got[f] for f in want} == want, c.id
        assert got["hist"] <= max_hist and got["max_m"] <= max_samples
    for rate, hist in E.REFUSED_RATES.items():
        r = E.Rate(rate)
        assert witness["refused"]["refused-%g" % rate] == (r.hi, r.lo, hist) and r.hist == hist > max_hist and not r.accepted


def coverage(witness):
    """form -> {"classes": class -> [case ids], "zero": calls without an inner sample, "full": calls with the most pieces}"""
    cov = {}
    for form in (1, 2, 3, 4):
        row = {"classes": {name: [] for name in E.CLASSES}, "zero": 0, "full": 0}
        for c in E.cases_of_form(form):
            for name in E.Rate(c.rate).classes():
                row["classes"][name].append(c.id)
            row["zero"] += witness["case"][c.id]["zero_calls"]
            row["full"] += witness["case"][c.id]["full_calls"]
        cov[form] = row
    return cov


def test_coverage_condition(witness):
    cov = coverage(witness)
    print("\nclass x form: cases of the table (calls without an inner sample / calls with %d FIFO pieces in the last rows)" % witness["limits"][4])
    print("| class | form 1 | form 2 | form 3 | form 4 |")
    print("|---|---|---|---|---|")
    for name in E.CLASSES:
        print("| %s | %s |" % (name, " | ".join(str(len(cov[f]["classes"][name])) for f in (1, 2, 3, 4))))
    print("| calls with n_out = 0 | %s |" % " | ".join(str(cov[f]["zero"]) for f in (1, 2, 3, 4)))
    print("| calls with the most pieces | %s |" % " | ".join(str(cov[f]["full"]) for f in (1, 2, 3, 4)))
    for form in (1, 2, 3, 4):
        for name in E.CLASSES:
            assert cov[form]["classes"][name], "form %d never runs class %s" % (form, name)
        assert cov[form]["zero"] >= 1, "form %d: no call without an inner sample" % form
        assert cov[form]["full"] >= 1, "form %d: no call with the most FIFO pieces" % form
    # every class has a rate, and the boundary pair falls on the two sides of kTapsLds, next to it
    assert {name for r in E.RATES for name in E.Rate(r).classes()} == set(E.CLASSES)
    last, first = E.Rate(47784.75), E.Rate(47785.75)
    lds = int(kernel_constant("kTapsLds"))
    assert last.n_taps == 7137 <= lds < first.n_taps == 7169 and first.hi == last.hi + 1
    assert witness["case"]["47784.75-steady-stereo"]["n_taps"] == 7137 and witness["case"]["47785.75-steady-mono"]["n_taps"] == 7169
    # the mixes put the LDS and the global table, no hop and several hops per call into one launch
    name, _, cases = E.mix_cases(E.MIXES[0])
    assert [c.rate for c in cases] == [384000.0, 6000.0, 47952.0]
    assert [E.Rate(c.rate).taps_in_lds for c in cases] == [True, True, False]
    longest = E.mix_cases(E.MIXES[2])[2]
    assert witness["case"][longest[0].id]["max_hops"] <= 2 and witness["case"][longest[1].id]["max_hops"] >= 8
    # the turnover walk grows the tap arena: two tables per class, from 44.1 kHz's to 47 952 Hz's
    taps = [2 * witness["case"]["turnover-leg-%d" % i]["n_taps"] for i in range(len(E.TURNOVER_LEGS))]
    assert taps[0] == 10242 and taps[1] == 63938 and [r for r, _ in E.TURNOVER_LEGS] == [44100.0, 47952.0, 6000.0, 384000.0]
