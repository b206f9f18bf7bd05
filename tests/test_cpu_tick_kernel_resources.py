"""Spills and scratch of the tick launch's six table kernels (fuse::table_kernel_w: one, two and four hops per step, common and
ragged), read from the kernel metadata of the gfx950 code object inside the built libbeatrice_hip.so.  Metadata only: nothing is
compiled and no GPU is needed.

A table kernel holds every body of its type list whether a table ever contains it or not, and a body that never runs still costs the
others registers and scratch: with the one-workgroup-per-stream tail and (at two and four hops) the sparse table's types compiled in,
the common four-hop kernel reported 121 VGPR spills and 448 bytes of scratch per lane, of which 75 and 332 belonged to code that no
tick executes (profiles/live_bodies_notes.md).  The bounds below are the kernels with their live bodies only; a body that comes back
into a list it has no table for shows up here.  The common four-hop kernel is pinned to the figure of this commit (the tail stages'
live spills are gone as well: section 2 of the notes); whoever moves it records the new figure there."""
import os
import re
import shutil
import subprocess

import pytest

LLVM_BIN = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
# (hops per step, ragged) -> (.vgpr_spill_count, .private_segment_fixed_size): no instance may be above these
LIVE_BODIES_ONLY = {(4, False): (46, 116), (4, True): (68, 144), (2, False): (25, 56), (2, True): (46, 56), (1, False): (25, 56), (1, True): (46, 56)}
# the common four-hop kernel (the headline's launch) at this commit, as profiles/live_bodies_notes.md records it
FOUR_HOPS_COMMON = (17, 52)


def _tool(name):
    return shutil.which(name) or (os.path.join(LLVM_BIN, name) if os.path.exists(os.path.join(LLVM_BIN, name)) else None)


@pytest.fixture(scope="module")
def table_kernels(bv, built, tmp_path_factory):
    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if bundler is None or readelf is None:
        pytest.skip("clang-offload-bundler / llvm-readelf not found")
    lib = os.path.join(os.path.dirname(os.path.abspath(bv.__file__)), "csrc", "libbeatrice_hip.so")
    blob = open(lib, "rb").read()
    d = tmp_path_factory.mktemp("code_objects")
    # the library holds one offload bundle per translation unit, one after the other: each to a file of its own for the bundler
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    assert starts, "no offload bundle in %s" % lib
    found = {}
    for i, at in enumerate(starts):
        end = starts[i + 1] if i + 1 < len(starts) else len(blob)
        bundle, co = str(d / ("bundle%d" % i)), str(d / ("code%d.co" % i))
        open(bundle, "wb").write(blob[at:end])
        r = subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + bundle, "--targets=" + TARGET, "--output=" + co], capture_output=True, text=True)
        if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "table_kernel_w" not in name:
                continue
            hops = re.search(r"BlockAOpILi1ELi(\d)E", name)   # (rc::BlockAOp<1, H> is in every list)
            ragged = re.search(r"table_kernel_wILi\d+ELb([01])E", name)
            assert hops and ragged, name[:120]
            value = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
            found[(int(hops.group(1)), ragged.group(1) == "1")] = (value("vgpr_spill_count"), value("private_segment_fixed_size"))
    return found


def test_all_six_table_kernels_are_in_the_library(table_kernels):
    assert sorted(table_kernels) == sorted(LIVE_BODIES_ONLY)


@pytest.mark.parametrize("hops,ragged", sorted(LIVE_BODIES_ONLY))
def test_no_table_kernel_is_above_its_live_bodies(table_kernels, hops, ragged):
    spills, scratch = table_kernels[(hops, ragged)]
    print("table kernel, %d hop(s) per step, %s: %d VGPR spills, %d bytes of scratch per lane" % (hops, "ragged" if ragged else "common", spills, scratch))
    bound = LIVE_BODIES_ONLY[(hops, ragged)]
    assert spills <= bound[0] and scratch <= bound[1]


def test_common_four_hop_kernel_is_where_the_notes_record_it(table_kernels):
    assert table_kernels[(4, False)] == FOUR_HOPS_COMMON
