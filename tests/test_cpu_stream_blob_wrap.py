"""sblob::counter_shift and sblob::turn (beatrice-vst_amd/csrc/stream_blob.h) with source and destination on opposite sides of the step
counter's wrap.  tests/test_cpu_stream_blob_format.py holds the turn against the closed form (slot of age a = (counter - a) mod m) for
m <= 17 and a few counters; here a ring with contents is turned and read back, the turn is held against rotating STEP BY STEP with the
counter's own increment (hop_next: wrap - 1 is followed by 0), for every slot count that divides the wrap up to 24 -- no ring of a batch
has more -- and for the pairs tests/test_gpu_counter_wrap.py moves streams between: wrap-3 -> 5 (shift 8) and 5 -> wrap-3 (shift
wrap - 8, walked in full: twelve million increments).  HIP-free: a stand-alone driver compiled with g++ under the address and
undefined-behaviour sanitizers, run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "stream_blob.h"
using namespace bhip::sblob;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (m %d src %d dst %d)\n", __LINE__, #c, m, src, dst); return 1; } } while (0)
constexpr int kWrap = 12252240;   // lcm(1..17), the step counter's wrap
static int next(int c) { return c + 1 >= kWrap ? 0 : c + 1; }   // the counter's own increment
static int back(int c, int age) { int v = c - age; return v < 0 ? v + kWrap : v; }   // the counter `age` steps earlier
int main() {
  std::vector<int> ms;
  for (int m = 1; m <= 24; ++m) if (kWrap % m == 0) ms.push_back(m);
  { int m = (int)ms.size(), src = 0, dst = 0; CHECK(m == 22); }   // 1..18, 20, 21, 22, 24
  const int pairs[][2] = {{kWrap - 3, 5}, {5, kWrap - 3}, {kWrap - 1, 0}, {0, kWrap - 1}, {kWrap - 24, 23}, {23, kWrap - 24}, {kWrap - 2, kWrap - 2}, {0, 0}};
  for (const auto& p : pairs) {
    const int src = p[0], dst = p[1];
    const int shift = counter_shift(dst, src, kWrap);
    { int m = 0; CHECK(shift >= 0 && shift < kWrap); }
    if (src == kWrap - 3 && dst == 5) { int m = 0; CHECK(shift == 8); }
    if (src == 5 && dst == kWrap - 3) { int m = 0; CHECK(shift == kWrap - 8); }
    // step by step: the counter walks from src to dst with its own increment, and every ring's write slot walks with it, one slot per step
    std::vector<int> slot(ms.size());
    for (size_t i = 0; i < ms.size(); ++i) slot[i] = src % ms[i];
    const bool walk = shift < 1000 || (src == 5 && dst == kWrap - 3);   // (one walk the long way round is enough; the others: contents only)
    int c = src, walked = 0;
    while (walk && c != dst) {
      c = next(c);
      ++walked;
      for (size_t i = 0; i < ms.size(); ++i) slot[i] = slot[i] + 1 == ms[i] ? 0 : slot[i] + 1;
    }
    { int m = 0; CHECK(!walk || walked == shift); }
    for (size_t i = 0; i < ms.size(); ++i) {
      const int m = ms[i], t = turn(shift, m);
      CHECK(t >= 0 && t < m);
      if (!walk) slot[i] = dst % m;
      CHECK(slot[i] == dst % m);                          // (m divides the wrap: the walk lands where the destination's counter points)
      CHECK((src % m + t) % m == slot[i]);                // the turn = the walk
      // a ring with contents: the source wrote the step of counter c at slot c % m; turned as ring_rotate_kernel / the import's scatter
      // turn it (slot j to j + t), the destination finds the step `age` steps back where ITS counter says
      std::vector<int> ring(m), turned(m);
      for (int age = 1; age <= m; ++age) ring[back(src, age) % m] = 1000 + age;
      for (int j = 0; j < m; ++j) turned[j + t >= m ? j + t - m : j + t] = ring[j];
      for (int age = 1; age <= m; ++age) CHECK(turned[back(dst, age) % m] == 1000 + age);
    }
  }
  std::printf("ok\n");
  return 0;
}
"""


def test_turn_equals_rotating_step_by_step_across_the_wrap(tmp_path):
    src = tmp_path / "stream_blob_wrap_driver.cc"
    src.write_text(DRIVER)
    exe = tmp_path / "stream_blob_wrap_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
