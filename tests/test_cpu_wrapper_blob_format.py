"""The format of a stream's WRAPPER blob and what BeatriceBatch_ImportStreamWrappers refuses (beatrice-vst_amd/csrc/wrapper_blob.h).  The
header is plain C++17 without HIP: a stand-alone driver with its own main is compiled against it with g++ under the address and
undefined-behaviour sanitizers and run here, on the CPU, as tests/test_cpu_stream_blob_format.py does for the stream blob's header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <limits>
#include <vector>
#include "wrapper_blob.h"
using namespace bhip::wblob;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// a header with its fields set by `edit` and a check word that FITS: only the range rules can refuse it
template <class F>
static std::vector<unsigned char> resealed(const std::vector<unsigned char>& blob, F edit) {
  std::vector<unsigned char> b(blob);
  Header h;
  std::memcpy(&h, b.data(), sizeof(h));
  edit(h);
  h.check = blob_check(h, b.data() + kOffState);
  std::memcpy(b.data(), &h, sizeof(h));
  return b;
}

int main() {
  // the layout: the fixed header, the state right behind it on a 16-byte boundary, a size that keeps blobs side by side aligned
  CHECK(sizeof(Header) == 80 && kOffState == 80 && kOffState % 16 == 0);
  CHECK(kStateBytes == 4 * (257 + 33 + 257 + 33 + 480) && kStateBytes % 16 == 0);
  CHECK(kBlobBytes == kOffState + kStateBytes && kBlobBytes % 16 == 0);
  CHECK(offsetof(Header, magic) == 0 && offsetof(Header, version) == 4 && offsetof(Header, blob_bytes) == 8 && offsetof(Header, check) == 16);
  CHECK(offsetof(Header, rate) == 24 && offsetof(Header, phase_down) == 32 && offsetof(Header, phase_up) == 36 && offsetof(Header, fill) == 40);
  CHECK(offsetof(Header, in_target_db) == 48 && offsetof(Header, in_now_db) == 56 && offsetof(Header, out_target_db) == 64 && offsetof(Header, out_now_db) == 72);

  // a good blob (44.1 kHz: hi / lo = 160 / 147) validates and gives every field back
  const int hi = 160;
  std::vector<unsigned char> blob(kBlobBytes, 0);
  for (size_t i = kOffState; i < kBlobBytes; ++i) blob[i] = (unsigned char)(i * 37u + 11u);
  write_header(44100.0, 17, 159, 463, -40.0, -12.5, 6.0, 0.25, blob.data());
  double rate = 0.0;
  CHECK(read_rate(blob.data(), blob.size(), &rate) == kOk && rate == 44100.0);
  Header got;
  CHECK(validate(blob.data(), blob.size(), hi, &got) == kOk);
  CHECK(got.rate == 44100.0 && got.phase_down == 17 && got.phase_up == 159 && got.fill == 463);
  CHECK(got.in_target_db == -40.0 && got.in_now_db == -12.5 && got.out_target_db == 6.0 && got.out_now_db == 0.25);

  // every single byte altered -- header and state, one at a time -- is refused
  for (size_t i = 0; i < kBlobBytes; ++i) {
    for (const unsigned char flip : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xff}) {
      std::vector<unsigned char> bad(blob);
      bad[i] ^= flip;
      if (validate(bad.data(), bad.size(), hi) == kOk) { std::printf("altered byte %zu (^%02x) was taken\n", i, (unsigned)flip); return 1; }
    }
  }
  {  // ... every header field by name, with its own reason
    struct Case { size_t off; Refusal why; } cases[] = {
      {offsetof(Header, magic), kMagicBad}, {offsetof(Header, version), kVersionBad}, {offsetof(Header, blob_bytes), kSizeBad},
      {offsetof(Header, check), kCheckBad}, {offsetof(Header, rate), kCheckBad}, {offsetof(Header, phase_down), kCheckBad},
      {offsetof(Header, phase_up), kCheckBad}, {offsetof(Header, fill), kCheckBad}, {offsetof(Header, reserved), kCheckBad},
      {offsetof(Header, in_target_db), kCheckBad}, {offsetof(Header, in_now_db), kCheckBad}, {offsetof(Header, out_target_db), kCheckBad},
      {offsetof(Header, out_now_db), kCheckBad}, {kOffState, kCheckBad}, {kBlobBytes - 1, kCheckBad}};
    for (const Case& c : cases) {
      std::vector<unsigned char> bad(blob);
      bad[c.off] ^= 0x04;
      CHECK(validate(bad.data(), bad.size(), hi) == c.why);
    }
    // the first three also stop read_rate, which is asked before a rate is trusted
    for (const size_t off : {offsetof(Header, magic), offsetof(Header, version), offsetof(Header, blob_bytes)}) {
      std::vector<unsigned char> bad(blob);
      bad[off] ^= 0x04;
      CHECK(read_rate(bad.data(), bad.size(), &rate) != kOk);
    }
  }

  // every truncation (the copy is exactly as long as what is offered: a read past it is the sanitizer's to report)
  for (size_t n = 0; n < kBlobBytes; n += (n < sizeof(Header) + 2 ? 1 : 97)) {
    std::vector<unsigned char> cut(blob.begin(), blob.begin() + n);
    CHECK(validate(cut.data(), cut.size(), hi) == kTruncated && read_rate(cut.data(), cut.size(), &rate) == kTruncated);
  }
  {
    std::vector<unsigned char> cut(blob.begin(), blob.begin() + kBlobBytes - 1);
    CHECK(validate(cut.data(), cut.size(), hi) == kTruncated);
  }

  // the range rules, with a check word that fits: phases in [0, hi), at hi = 1 (48 kHz), 2 (96 kHz) and 160 (44.1 kHz)
  for (const int h_i : {1, 2, 160}) {
    for (const int ph : {0, h_i - 1}) {
      CHECK(validate(resealed(blob, [&](Header& h) { h.phase_down = ph; h.phase_up = h_i - 1 - ph; }).data(), kBlobBytes, h_i) == kOk);
    }
    for (const int ph : {-1, h_i, h_i + 1, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
      CHECK(validate(resealed(blob, [&](Header& h) { h.phase_down = ph; h.phase_up = 0; }).data(), kBlobBytes, h_i) == kPhaseBad);
      CHECK(validate(resealed(blob, [&](Header& h) { h.phase_down = 0; h.phase_up = ph; }).data(), kBlobBytes, h_i) == kPhaseBad);
    }
    // the FIFO fill in [0, 480)
    for (const int f : {0, 1, 479}) CHECK(validate(resealed(blob, [&](Header& h) { h.phase_down = h.phase_up = 0; h.fill = f; }).data(), kBlobBytes, h_i) == kOk);
    for (const int f : {-1, 480, 481, std::numeric_limits<int>::max()})
      CHECK(validate(resealed(blob, [&](Header& h) { h.phase_down = h.phase_up = 0; h.fill = f; }).data(), kBlobBytes, h_i) == kFillBad);
  }
  // the good blob's own clocks (17, 159) are out of range for the ratio of another rate
  CHECK(validate(blob.data(), blob.size(), 2) == kPhaseBad && validate(blob.data(), blob.size(), 159) == kPhaseBad);
  // all four gain values finite
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (const double v : {nan, inf, -inf}) {
    CHECK(validate(resealed(blob, [&](Header& h) { h.in_target_db = v; }).data(), kBlobBytes, hi) == kGainBad);
    CHECK(validate(resealed(blob, [&](Header& h) { h.in_now_db = v; }).data(), kBlobBytes, hi) == kGainBad);
    CHECK(validate(resealed(blob, [&](Header& h) { h.out_target_db = v; }).data(), kBlobBytes, hi) == kGainBad);
    CHECK(validate(resealed(blob, [&](Header& h) { h.out_now_db = v; }).data(), kBlobBytes, hi) == kGainBad);
  }
  // the rate is the batch's to judge (RateClass::configure): the header only carries it
  CHECK(validate(resealed(blob, [&](Header& h) { h.rate = nan; }).data(), kBlobBytes, hi) == kOk);
  std::printf("ok\n");
  return 0;
}
"""


def test_a_good_wrapper_blob_validates_and_every_damaged_one_is_refused(tmp_path):
    src = tmp_path / "wrapper_blob_driver.cc"
    src.write_text(DRIVER)
    exe = tmp_path / "wrapper_blob_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
