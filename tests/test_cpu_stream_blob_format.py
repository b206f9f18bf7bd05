"""The format of a stream's blob and what BeatriceBatch_ImportStreams refuses (beatrice-vst_amd/csrc/stream_blob.h).  The header is plain
C++17 without HIP: a stand-alone driver with its own main is compiled against it with g++ under the address and undefined-behaviour
sanitizers and run here, on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "stream_blob.h"
using namespace bhip::sblob;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
constexpr int kWrap = 12252240;   // lcm(1..17), the step counter's wrap
int main() {
  const RingShape shapes[] = {{1, 160, 3}, {64, 32, 2}, {256, 2, 17}, {128, 5, 4}, {1536, 1, 1}, {3, 7, 5}};
  const int n_rings = (int)(sizeof(shapes) / sizeof(shapes[0]));
  const uint32_t cfg_bytes = 136, w48_bytes = 286 * 4;
  const Layout l = make_layout(2, shapes, n_rings, cfg_bytes, w48_bytes);

  // the layout: every part where the next one starts, pieces 16-byte aligned and in order, nothing overlaps, the size a multiple of 16
  CHECK(l.off_shapes == sizeof(Header) && l.off_indices == l.off_shapes + 12u * n_rings && l.header_bytes() == l.off_indices);
  CHECK(l.off_cfg >= l.off_indices + 4u * kIndices && l.off_cfg % 8 == 0 && l.off_engine == l.off_cfg + cfg_bytes);
  CHECK(l.off_state >= l.off_engine + kEngineBytes && l.off_state % 16 == 0 && l.blob_bytes % 16 == 0);
  CHECK((int)l.pieces.size() == n_rings + 2);
  size_t at = l.off_state / 4;
  for (int i = 0; i < n_rings + 2; ++i) {
    const Piece& p = l.pieces[i];
    CHECK(p.off == at && p.off % 4 == 0);
    if (i < n_rings) CHECK(p.slot_floats == (uint32_t)(shapes[i].C * shapes[i].n) && p.m == shapes[i].m);
    at += round_up((size_t)p.slot_floats * p.m, 4);
  }
  CHECK(l.pieces[n_rings].slot_floats == 1 && l.pieces[n_rings].m == 1 && l.pieces[n_rings + 1].slot_floats == 286 && l.pieces[n_rings + 1].m == 1);
  CHECK(at * 4 == l.blob_bytes);

  // a good blob validates; its counter comes back
  std::vector<unsigned char> blob(l.blob_bytes, 0);
  write_header(l, 4711, blob.data());
  const int32_t idx[kIndices] = {2, 2, 1, 0, 0, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1};
  std::memcpy(blob.data() + l.off_indices, idx, sizeof(idx));
  int counter = -1;
  CHECK(validate_header(l, blob.data(), blob.size(), kWrap, &counter) == kOk && counter == 4711);

  // every single header field altered -- each byte of the header and of the ring shapes, one at a time -- is refused
  for (size_t i = 0; i < l.header_bytes(); ++i) {
    for (const unsigned char flip : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xff}) {
      std::vector<unsigned char> bad(blob);
      bad[i] ^= flip;
      if (validate_header(l, bad.data(), bad.size(), kWrap) == kOk) { std::printf("altered byte %zu (^%02x) was taken\n", i, (unsigned)flip); return 1; }
    }
  }
  {  // ... and by name, with the reason
    struct Case { size_t off; Refusal why; } cases[] = {
      {offsetof(Header, magic), kMagicBad}, {offsetof(Header, version), kVersionBad}, {offsetof(Header, blob_bytes), kSizeBad},
      {offsetof(Header, H), kHopsBad}, {offsetof(Header, n_rings), kLayoutBad}, {offsetof(Header, cfg_bytes), kLayoutBad},
      {offsetof(Header, w48_bytes), kLayoutBad}, {offsetof(Header, engine_bytes), kLayoutBad}, {offsetof(Header, check), kCheckBad}};
    for (const Case& c : cases) {
      std::vector<unsigned char> bad(blob);
      bad[c.off] ^= 0x04;
      CHECK(validate_header(l, bad.data(), bad.size(), kWrap) == c.why);
    }
    std::vector<unsigned char> bad(blob);
    bad[offsetof(Header, counter)] ^= 0x01;   // another counter in range: only the check word can tell
    CHECK(validate_header(l, bad.data(), bad.size(), kWrap) == kCheckBad);
    Header h;
    std::memcpy(&h, blob.data(), sizeof(h));
    for (const int c : {-1, kWrap, kWrap + 5}) {   // out of range, with a check word that fits: still refused
      Header o = h;
      o.counter = c;
      o.check = header_check(o, blob.data() + l.off_shapes, l.header_bytes() - l.off_shapes);
      std::vector<unsigned char> b2(blob);
      std::memcpy(b2.data(), &o, sizeof(o));
      CHECK(validate_header(l, b2.data(), b2.size(), kWrap) == kCounterBad);
    }
    Header o = h;
    o.counter = kWrap - 1;
    o.check = header_check(o, blob.data() + l.off_shapes, l.header_bytes() - l.off_shapes);
    std::vector<unsigned char> b2(blob);
    std::memcpy(b2.data(), &o, sizeof(o));
    CHECK(validate_header(l, b2.data(), b2.size(), kWrap, &counter) == kOk && counter == kWrap - 1);
  }

  // every truncation of the header (the copy is exactly as long as what is offered: a read past it is the sanitizer's to report)
  for (size_t n = 0; n < l.header_bytes(); ++n) {
    std::vector<unsigned char> cut(blob.begin(), blob.begin() + n);
    CHECK(validate_header(l, cut.data(), cut.size(), kWrap) == kTruncated);
  }
  {  // the header whole, the rest short
    std::vector<unsigned char> cut(blob.begin(), blob.begin() + l.blob_bytes - 1);
    CHECK(validate_header(l, cut.data(), cut.size(), kWrap) == kTruncated);
  }

  // a batch with other hops per step
  CHECK(validate_header(make_layout(1, shapes, n_rings, cfg_bytes, w48_bytes), blob.data(), blob.size(), kWrap) == kHopsBad);
  CHECK(validate_header(make_layout(4, shapes, n_rings, cfg_bytes, w48_bytes), blob.data(), blob.size(), kWrap) == kHopsBad);
  // a ring table that differs in one m: with the same total size (two rings of equal slot size trade a slot) and with another
  {
    RingShape other[n_rings];
    for (int i = 0; i < n_rings; ++i) other[i] = shapes[i];
    other[2].m = 16;
    CHECK(validate_header(make_layout(2, other, n_rings, cfg_bytes, w48_bytes), blob.data(), blob.size(), kWrap) != kOk);
    const RingShape same_size[] = {{4, 4, 3}, {4, 4, 5}}, traded[] = {{4, 4, 4}, {4, 4, 4}}, one_m[] = {{4, 4, 3}, {4, 4, 5}};
    const Layout a = make_layout(2, same_size, 2, cfg_bytes, w48_bytes), t = make_layout(2, traded, 2, cfg_bytes, w48_bytes);
    CHECK(a.blob_bytes == t.blob_bytes);
    std::vector<unsigned char> ba(a.blob_bytes, 0);
    write_header(a, 1, ba.data());
    CHECK(validate_header(make_layout(2, one_m, 2, cfg_bytes, w48_bytes), ba.data(), ba.size(), kWrap) == kOk);
    CHECK(validate_header(t, ba.data(), ba.size(), kWrap) == kLayoutBad);
  }
  // other sizes of the two fixed structs, one ring more or fewer
  CHECK(validate_header(make_layout(2, shapes, n_rings, cfg_bytes + 8, w48_bytes), blob.data(), blob.size(), kWrap) != kOk);
  CHECK(validate_header(make_layout(2, shapes, n_rings, cfg_bytes, w48_bytes + 16), blob.data(), blob.size(), kWrap) != kOk);
  CHECK(validate_header(make_layout(2, shapes, n_rings - 1, cfg_bytes, w48_bytes), blob.data(), blob.size(), kWrap) != kOk);

  // entry_map: index i becomes entry_map[i]
  int32_t mapped[kIndices];
  const int map3[] = {1, 2, 0};
  CHECK(map_indices(l, blob.data(), map3, 3, 3, 4, mapped) == kOk);
  for (int i = 0; i < kIndices; ++i) CHECK(mapped[i] == map3[idx[i]]);
  CHECK(map_indices(l, blob.data(), nullptr, 0, 3, 4, mapped) == kOk);
  for (int i = 0; i < kIndices; ++i) CHECK(mapped[i] == idx[i]);
  // a map too short for an index the blob names (2), for every such length
  for (int n_map = 0; n_map <= 2; ++n_map) CHECK(map_indices(l, blob.data(), map3, n_map, 3, 4, mapped) == kIndexUnmapped);
  // a mapped index at n_speakers, and below zero -- in every position
  for (int pos = 0; pos < 3; ++pos) {
    int bad[] = {1, 2, 0};
    bad[pos] = 3;
    CHECK(map_indices(l, blob.data(), bad, 3, 3, 4, mapped) == kIndexRange);
    CHECK(map_indices(l, blob.data(), bad, 3, 4, 4, mapped) == kOk);   // (the same map into a table of four)
    bad[pos] = -1;
    CHECK(map_indices(l, blob.data(), bad, 3, 3, 4, mapped) == kIndexRange);
  }
  // a blob whose own index is out of range, in every one of its positions, with a map and without
  for (int i = 0; i < kIndices; ++i)
    for (const int32_t v : {-1, 4, 1 << 30}) {
      std::vector<unsigned char> bad(blob);
      std::memcpy(bad.data() + l.off_indices + 4 * i, &v, 4);
      CHECK(map_indices(l, bad.data(), map3, 3, 3, 4, mapped) == kIndexUnmapped);
      CHECK(map_indices(l, bad.data(), nullptr, 0, 3, 4, mapped) == kIndexRange);
    }

  // the turn of a ring between two counters is ring_rotate_kernel's: what the source wrote at slot c % m is found at (c + d) % m
  CHECK(counter_shift(10, 4, kWrap) == 6 && counter_shift(4, 10, kWrap) == kWrap - 6 && counter_shift(0, kWrap - 1, kWrap) == 1 && counter_shift(7, 7, kWrap) == 0);
  for (int m = 1; m <= 17; ++m)
    for (const int src : {0, 5, kWrap - 3})
      for (const int dst : {0, 1, 6, 26, kWrap - 1}) {
        const int t = turn(counter_shift(dst, src, kWrap), m);
        CHECK(t >= 0 && t < m);
        for (int age = 0; age < m; ++age) {   // the slot of the step `age` steps before the counter, on either side
          const int s_slot = ((src - age) % m + m) % m, d_slot = ((dst - age) % m + m) % m;
          CHECK(m == 1 ? t == 0 : (s_slot + t) % m == d_slot);
        }
      }

  // the engine continues its sequence; a damaged text is refused
  {
    std::mt19937 e(7);
    for (int i = 0; i < 1000; ++i) (void)e();
    std::vector<unsigned char> text(kEngineBytes, 0xee);
    CHECK(engine_out(e, text.data()));
    std::mt19937 back(1);
    CHECK(engine_in(text.data(), &back) && back == e);
    for (int i = 0; i < 2000; ++i) CHECK(back() == e());
    std::vector<unsigned char> bad(text);
    bad[kEngineBytes - 1] = '1';   // not terminated
    CHECK(!engine_in(bad.data(), &back));
    bad = text;
    bad[3] = 'x';
    CHECK(!engine_in(bad.data(), &back));
    std::vector<unsigned char> empty(kEngineBytes, 0);
    CHECK(!engine_in(empty.data(), &back));
  }
  std::printf("ok\n");
  return 0;
}
"""


def test_a_good_blob_validates_and_every_damaged_one_is_refused(tmp_path):
    src = tmp_path / "stream_blob_driver.cc"
    src.write_text(DRIVER)
    exe = tmp_path / "stream_blob_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
