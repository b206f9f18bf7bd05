"""BeatriceBatch_ScanSilentBlocksBegin / ScanSilentBlocksEnd / ScanSilentBlocks / ScanBoundBlocks48k without a GPU: exported, declared and
typed; the yardstick of the GPU tests (tests/silent_ref.py) held against the library's host-side statement of the shell's rule
(ProcessorProxy::ProcessChannels on the oracle core); and csrc/silent_scan_plan.h -- plain C++17 -- walked by a stand-alone program of its
own under the address and undefined-behaviour sanitizers, as tests/test_cpu_wrapper_blob_format.py does for the wrapper blob's header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import silent_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_ScanSilentBlocksBegin", "BeatriceBatch_ScanSilentBlocksEnd", "BeatriceBatch_ScanSilentBlocks",
       "BeatriceBatch_ScanBoundBlocks48k")


def test_the_library_exports_the_four_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_four_symbols():
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    b, i = r"\s*BeatriceBatch\s*\*\s*\w+\s*", r"\s*int\s+\w+\s*"
    geometry = (r",\s*const\s+float\s*\*\s*\w+\s*," + i + "," + i + "," + i + "," + i + r",\s*long\s+long\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*"
                r",\s*void\s*\*\s*\w+\s*")
    u8 = r",\s*unsigned\s+char\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_ScanSilentBlocksBegin\s*\(" + b + geometry + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ScanSilentBlocksEnd\s*\(" + b + "," + i + u8 + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ScanSilentBlocks\s*\(" + b + geometry + u8 + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ScanBoundBlocks48k\s*\(" + b + "," + i + u8 + u8 + r",\s*void\s*\*\s*\w+\s*\)\s*;", text)


def test_the_ctypes_table_types_the_four_symbols(bv):
    i32p, u8p, vp, i, ll = C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.c_void_p, C.c_int, C.c_longlong
    assert bv._BATCH["BeatriceBatch_ScanSilentBlocksBegin"] == (i, [vp, vp, i, i, i, i, ll, i32p, vp])
    assert bv._BATCH["BeatriceBatch_ScanSilentBlocksEnd"] == (i, [vp, i, u8p])
    assert bv._BATCH["BeatriceBatch_ScanSilentBlocks"] == (i, [vp, vp, i, i, i, i, ll, i32p, vp, u8p])
    assert bv._BATCH["BeatriceBatch_ScanBoundBlocks48k"] == (i, [vp, i, u8p, u8p, vp])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    for name in ("scan_silent_blocks", "scan_silent_blocks_begin", "scan_silent_blocks_end", "scan_bound_blocks_48k"):
        assert callable(getattr(bv.Batch, name))


def test_the_mode_table_has_no_row_for_them():
    """The generic scan works in every mode, the bound one is gated on the row of ConvertBlocks48kDevice(NULL): csrc/batch_modes.h keeps
    the rows of the GPU matrix.  A guard, not a test of the feature: it holds on a tree without the scan as well, and fails the day
    someone gives these calls a row."""
    text = open(os.path.join(REPO, "beatrice-vst_amd", "csrc", "batch_modes.h")).read()
    for name in NEW:
        assert name.replace("BeatriceBatch_", "") not in text
    assert "Scan" not in text


@pytest.mark.parametrize("channels", [1, 2])
def test_the_yardstick_is_the_flag_the_host_layer_returns(built, model_dir, channels):
    """silent_ref.shell_silent against ProcessorProxy::ProcessChannels (the host layer's copy of reference src/vst/processor.cc:183-214) on
    every row of the edge table at n = 480.  It pins the yardstick, not the feature: it needs nothing of the scan and passes without it."""
    from test_host_proxy import K_MODEL, Proxy
    _f32p = C.POINTER(C.c_float)
    n = 480
    p = Proxy(48000.0)
    assert p.call("SetString", K_MODEL, (model_dir + "/model.toml").encode()) == 0
    rows = silent_ref.edge_table(n, channels)
    seen = set()
    for name, block in rows:
        in0 = np.ascontiguousarray(block[0])
        in1 = np.ascontiguousarray(block[1]) if channels == 2 else None
        o0, o1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        flag = p.call("ProcessChannels", in0.ctypes.data_as(_f32p), in1.ctypes.data_as(_f32p) if in1 is not None else None,
                      o0.ctypes.data_as(_f32p), o1.ctypes.data_as(_f32p) if channels == 2 else None, n)
        assert flag in (0, 1), (name, flag)
        assert silent_ref.shell_silent(block) == flag, name
        seen.add(flag)
    p.close()
    assert seen == {0, 1}
    want = {"all +0": 1, "all -0": 1, "tiny at 0": 1 if channels == 2 else 0, "3 x tiny at n-1": 0, "nan": 0, "inf": 0}
    if channels == 2:
        want.update({"L = -R": 1, "tiny in channel 1 only": 1, "3 x tiny in channel 1 only": 0, "sum overflows": 0, "tiny in both channels": 0})
    got = {name: silent_ref.shell_silent(block) for name, block in rows}
    for name, flag in want.items():
        assert got[name] == flag, name
    assert silent_ref.shell_silent(np.zeros((channels, 0), np.float32)) == 1   # (vacuously, as the host loop has it)


DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "silent_scan_plan.h"
using namespace bhip::sscan;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// Every float the plan lets any lane read in any block of an accepted call is touched in a buffer that is EXACTLY the caller's cells
// long, offset so that the base has the alignment the path was chosen for: a read outside is the sanitizer's to report.  Also held
// against the closed forms: the block's own range, and the cell.
static int walk(long long n_cells, long long J, long long ch, long long n, long long stride, const int* lens, int misalign) {
  float* raw = static_cast<float*>(std::malloc(sizeof(float) * (size_t)(n_cells * stride + misalign)));   // (16-byte aligned, and not a float longer)
  CHECK(raw && reinterpret_cast<std::uintptr_t>(raw) % 16 == 0);
  for (long long i = 0; i < n_cells * stride + misalign; ++i) raw[i] = 0.0f;
  float* base = raw + misalign;
  const long long room = n_cells * stride;   // the caller's memory: [base, base + room)
  Geometry g;
  CHECK(accept(base, n_cells, J, ch, n, stride, lens, true, &g));
  const bool vec = vector_path(base, g);
  CHECK(vec == (!lens && misalign == 0 && n % 4 == 0 && stride % 4 == 0));
  CHECK(grid(g) * (unsigned)kWavesPerGroup >= (unsigned)g.blocks() && (grid(g) - 1) * (unsigned)kWavesPerGroup < (unsigned)g.blocks());
  volatile float acc = 0.0f;
  for (long long c = 0; c < n_cells; ++c)
    for (long long j = 0; j < J; ++j) {
      const long long len = lens ? lens[c] : n;
      long long covered = 0;
      for (int lane = 0; lane < 64; ++lane) {
        const long long last = lane_last(g, vec, c, j, len, lane);
        if (last < 0) { CHECK(lane >= (vec ? len / 4 : len)); continue; }
        CHECK(last >= g.block_first(c, j) && last <= g.block_last(c, j, len));
        CHECK(last >= c * stride && last < (c + 1) * stride && last < room);
        if (vec) CHECK((g.block_first(c, j) % 4) == 0 && (len % 4) == 0 && (reinterpret_cast<std::uintptr_t>(base + last - 3) % 16) == 0);
        // the lane's items, as the kernel's loop walks them
        const long long items = vec ? len / 4 : len, w = vec ? 4 : 1;
        for (long long i = lane; i < items; i += 64)
          for (long long k = 0; k < ch; ++k)
            for (long long q = 0; q < w; ++q) { acc = acc + base[g.block_first(c, j) + k * len + i * w + q]; ++covered; }
      }
      CHECK(covered == ch * len);   // every sample of the block, once
      if (len > 0) CHECK(g.block_last(c, j, len) < (c + 1) * stride);
    }
  CHECK(acc == 0.0f);
  std::free(raw);
  return 0;
}

int main() {
  float x[64];
  const int good_lens[3] = {0, 7, 16}, bad_lo[3] = {0, -1, 16}, bad_hi[3] = {0, 17, 16};
  Geometry g;
  // ---- the refusals, each alone against a call that is otherwise good
  CHECK(accept(x, 3, 1, 2, 16, 32, nullptr, true, &g));
  CHECK(g.n_cells == 3 && g.J == 1 && g.channels == 2 && g.n == 16 && g.stride == 32 && !g.ragged && g.blocks() == 3);
  CHECK(!accept(nullptr, 3, 1, 2, 16, 32, nullptr, true, &g));
  CHECK(!accept(x, 3, 1, 2, 16, 32, nullptr, false, &g));          // (the one-call form's NULL flags)
  CHECK(!accept(x, 0, 1, 2, 16, 32, nullptr, true, &g) && !accept(x, -1, 1, 2, 16, 32, nullptr, true, &g));
  CHECK(!accept(x, 3, 0, 2, 16, 32, nullptr, true, &g) && !accept(x, 3, -4, 2, 16, 32, nullptr, true, &g));
  CHECK(!accept(x, 3, 1, 0, 16, 32, nullptr, true, &g) && !accept(x, 3, 1, 3, 16, 48, nullptr, true, &g) && !accept(x, 3, 1, -1, 16, 32, nullptr, true, &g));
  CHECK(!accept(x, 3, 1, 2, 0, 32, nullptr, true, &g) && !accept(x, 3, 1, 2, -16, 32, nullptr, true, &g));
  CHECK(!accept(x, 3, 1, 2, 16, 31, nullptr, true, &g) && !accept(x, 3, 1, 2, 16, 0, nullptr, true, &g) && !accept(x, 3, 1, 2, 16, -32, nullptr, true, &g));
  CHECK(!accept(x, 3, 2, 2, 16, 63, nullptr, true, &g) && accept(x, 3, 2, 2, 16, 64, nullptr, true, &g));
  CHECK(accept(x, 3, 1, 2, 16, 32, good_lens, true, &g) && g.ragged);
  CHECK(!accept(x, 3, 2, 2, 16, 64, good_lens, true, &g));         // (per-cell lengths need one block per cell)
  CHECK(!accept(x, 3, 1, 2, 16, 32, bad_lo, true, &g) && !accept(x, 3, 1, 2, 16, 32, bad_hi, true, &g));
  CHECK(accept(x, 1 << 20, 1, 1, 1, 1, nullptr, true, &g) && accept(x, 1 << 18, 4, 1, 1, 4, nullptr, true, &g) && grid(g) == (1u << 18));
  CHECK(!accept(x, (1 << 20) + 1, 1, 1, 1, 1, nullptr, true, &g) && !accept(x, 1 << 18, 5, 1, 1, 5, nullptr, true, &g));
  CHECK(!accept(x, 0x7fffffff, 0x7fffffff, 2, 0x7fffffff, 0x7fffffffffffffffll, nullptr, true, &g));   // (nothing wraps on the way to the answer)
  CHECK(!accept(x, 2, 1, 1, 16, kMaxStride + 1, nullptr, true, &g) && accept(x, 2, 1, 1, 16, kMaxStride, nullptr, true, &g));
  CHECK(accept(x, 1, 1, 1, kMaxSamples, kMaxStride, nullptr, true, &g) && !accept(x, 1, 1, 1, kMaxSamples + 1, kMaxStride, nullptr, true, &g));
  CHECK(kMaxSamples + 64 <= 0x7fffffffll && !accept(x, 1, 1, 1, 0x7fffffff, kMaxStride, nullptr, true, &g));   // (the kernel's 32-bit sample counter, stepping by 64)

  // ---- the path: 16-byte loads only when base, length and every offset are multiples of four floats
  alignas(16) static float a[4096];
  CHECK(accept(a, 2, 4, 2, 480, 3840, nullptr, true, &g) && vector_path(a, g));
  CHECK(accept(a + 1, 2, 4, 2, 480, 3840, nullptr, true, &g) && !vector_path(a + 1, g) && !vector_path(a + 2, g) && !vector_path(a + 3, g) && vector_path(a + 4, g));
  CHECK(accept(a, 2, 1, 2, 441, 882, nullptr, true, &g) && !vector_path(a, g));
  CHECK(accept(a, 2, 1, 2, 480, 961, nullptr, true, &g) && !vector_path(a, g));      // (the second cell's base is off by one float)
  CHECK(accept(a, 2, 1, 2, 480, 962, nullptr, true, &g) && !vector_path(a, g) && accept(a, 2, 1, 2, 480, 964, nullptr, true, &g) && vector_path(a, g));
  const int lens480[2] = {480, 480};
  CHECK(accept(a, 2, 1, 2, 480, 960, lens480, true, &g) && !vector_path(a, g));       // (per-cell lengths: always the 4-byte path)

  // ---- accepted geometries: every read inside the block, the cell and the caller's memory
  const long long ns[] = {1, 3, 4, 5, 63, 64, 65, 160, 256, 257, 441, 480, 4088};
  for (const long long n : ns)
    for (const long long ch : {1ll, 2ll})
      for (const long long J : {1ll, 4ll})
        for (const long long pad : {0ll, 1ll, 4ll})
          for (const int mis : {0, 1})
            if (walk(3, J, ch, n, J * ch * n + pad, nullptr, mis) != 0) return 1;
  {
    const int lens[5] = {0, 1, 441, 480, 37};
    for (const long long ch : {1ll, 2ll})
      for (const long long pad : {0ll, 3ll})
        for (const int mis : {0, 1})
          if (walk(5, 1, ch, 480, ch * 480 + pad, lens, mis) != 0) return 1;
  }

  // ---- the ticket ring: four out, a fifth refused, ends in any order, no second end
  TicketRing r;
  int t[4];
  CHECK(r.free_entries() == 4);
  for (int k = 0; k < 4; ++k) {
    const int e = r.free_entry();
    CHECK(e == k);
    t[k] = r.issue(e, 100 + k);
    CHECK(t[k] >= 0 && r.entry_of(t[k]) == e && r.blocks_of(e) == 100 + k);
    for (int q = 0; q < k; ++q) CHECK(t[q] != t[k]);
  }
  CHECK(r.free_entry() == -1 && r.free_entries() == 0);            // (Begin answers -3 and touches nothing)
  for (int k = 0; k < 4; ++k) CHECK(r.entry_of(t[k]) == k);        // ... nothing
  CHECK(r.entry_of(-1) == -1 && r.entry_of(-3) == -1 && r.entry_of(0) == -1 && r.entry_of(3) == -1 && r.entry_of(t[3] + 4) == -1 && r.entry_of(0x7fffffff) == -1);
  const int order[4] = {2, 0, 3, 1};
  for (int k = 0; k < 4; ++k) {
    const int e = r.entry_of(t[order[k]]);
    CHECK(e == order[k]);
    r.end(e);
    CHECK(r.entry_of(t[order[k]]) == -1);                          // a double end is an unknown ticket
    CHECK(r.free_entries() == k + 1);
  }
  // an entry's next holder has another ticket: the old one stays unknown
  std::vector<int> seen(t, t + 4);
  for (int round = 0; round < 1000; ++round) {
    const int e = r.free_entry();
    CHECK(e == 0);
    const int tk = r.issue(e, 1);
    CHECK(tk >= 0 && (tk & 3) == e && r.entry_of(tk) == e);
    for (const int old : seen) CHECK(old != tk && (r.entry_of(old) == -1));
    if (seen.size() < 64) seen.push_back(tk);
    r.end(e);
  }
  {  // the serial number wraps without ever handing out a negative ticket, or one that is out
    TicketRing w((1u << 28) - 8);
    int prev = -1;
    for (int k = 0; k < 16; ++k) {
      const int tk = w.issue(0, 1);
      CHECK(tk >= 0 && tk != prev && w.entry_of(tk) == 0 && w.entry_of(prev) == -1);
      w.end(0);
      prev = tk;
    }
  }
  std::printf("ok\n");
  return 0;
}
"""


def test_the_plan_refuses_chooses_and_keeps_every_read_inside_the_cells(tmp_path):
    src = tmp_path / "silent_scan_plan_driver.cc"
    src.write_text(DRIVER)
    exe = tmp_path / "silent_scan_plan_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
