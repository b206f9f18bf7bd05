"""The mode table the library gates its entry points on (beatrice-vst_amd/csrc/batch_modes.h) against its restatement by hand, MATRIX of
tests/test_gpu_mode_matrix.py: a cell the table refuses and MATRIX does not list is a refusal no GPU test walks; a cell MATRIX lists and the table
allows is a probe that would fail on the GPU.  The header is plain C++: a dumper of a few lines is compiled against it with g++, no GPU needed."""
import os
import subprocess

import test_gpu_mode_matrix as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the flags a batch has after mm.enter(mode): the header derives the mode from them, the dumper checks that it comes out as the letter
MODES = {"in_order": ("A", "{}"), "stage_pipelining": ("B", "{.pipelined = true}"), "resident_io": ("C", "{.io = true}"), "tick": ("D", "{.tk = true, .io = true}"),
         "host_streaming": ("E", "{.tk = true, .hs = true, .io = true}"), "blocks48k_around_ticks": ("F", "{.tk = true, .r48 = true, .io = true}"),
         "resident_blocks": ("G", "{.tk = true, .rb = true, .io = true, .wrap_ready = true}"),
         "resident_blocks_per_stream_clocks": ("P", "{.tk = true, .rb = true, .ragged = true, .silent = true, .io = true, .rates_ready = true}"),
         "silent_rule_in_order": ("S", "{.silent = true}")}
# each mode's own entry point per step (the header's list of modes)
OWN = {"in_order": ["ConvertFrames", "ConvertFramesDevice(ptrs)"], "stage_pipelining": ["ConvertFrames", "ConvertFramesDevice(ptrs)"], "resident_io": ["ConvertFramesDevice(NULL)"],
       "tick": ["ConvertFramesDevice(NULL)"], "host_streaming": ["StreamFrames"], "blocks48k_around_ticks": ["ConvertBlocks48kDevice(NULL)"], "resident_blocks": ["ProcessBlocksDevice(NULL)"],
       "resident_blocks_per_stream_clocks": ["ProcessBlocksRaggedDevice"], "silent_rule_in_order": ["ConvertBlocks48k", "ConvertBlocks48kDevice(ptrs)"]}

DUMPER = """
#include <cstdio>
#include <initializer_list>
#include "batch_modes.h"
using namespace bhip::modes;
static void dump(const char* mode, Mode m, Flags f) {
  if (mode_of(f) != m) std::printf("mode_of %s\\n", mode);
  for (int H : {1, 2, 4, 8}) {
    f.H = H;
    std::printf("%s %d", mode, H);
    for (int e = 0; e < kEntries; ++e) if (!allowed((Entry)e, f)) std::printf("|%s", kTable[e].name);
    std::printf("\\n");
  }
}
int main() {
  for (const Row& r : kTable) std::printf("entry|%s\\n", r.name);
DUMPS  return 0;
}
"""


def table(tmp_path):
    body = "".join('  dump("%s", Mode::%s, Flags%s);\n' % (mode, letter, flags) for mode, (letter, flags) in MODES.items())
    src = tmp_path / "dump_modes.cc"
    src.write_text(DUMPER.replace("DUMPS", body))
    exe = tmp_path / "dump_modes"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert not [ln for ln in lines if ln.startswith("mode_of")], "mode_of() does not derive the mode from its own flags: %s" % lines
    entries = [ln.split("|", 1)[1] for ln in lines if ln.startswith("entry|")]
    refused = {}
    for ln in lines:
        if not ln.startswith("entry|"):
            head, *names = ln.split("|")
            mode, H = head.split()
            refused[(mode, int(H))] = set(names)
    return entries, refused


def test_mode_table_is_the_matrix_of_the_gpu_test(tmp_path):
    entries, refused = table(tmp_path)
    assert len(entries) == len(set(entries)) and set(entries) == set(mm.PROBES), set(entries) ^ set(mm.PROBES)
    assert set(MODES) == set(mm.MATRIX) == {m for m, _ in mm.MODES_AT}
    for mode, H in mm.MODES_AT:
        want = set(mm.refused(mode, H))
        got = refused[(mode, H)]
        assert got == want, "mode %s, H = %d: the table alone refuses %s, MATRIX alone %s" % (mode, H, sorted(got - want), sorted(want - got))
        assert not [n for n in OWN[mode] if n in got], "mode %s, H = %d: its own entry point is refused" % (mode, H)
