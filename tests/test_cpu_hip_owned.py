"""The owning types of the batch's host side (beatrice-vst_amd/csrc/hip_owned.h) against a counting stand-in for hip/hip_runtime.h: every
create raises a live count per kind and every free lowers it (a free of something not live aborts), the k-th create can be told to fail, and
hipEventSynchronize / hipEventRecord are counted.  The header is plain C++17: a driver is compiled against it with g++, no GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STAND_IN = r"""
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <set>
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipStream_t* hipStream_t;
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1;
namespace fake {
enum Kind { DEV, PINNED, EVENT, STREAM, KINDS };
inline std::set<void*> live[KINDS];
inline int creates = 0, fail_at = 0;          // fail_at = k: the k-th create from now on fails (0: none)
inline int syncs = 0, records = 0, untimed_events = 0;
inline hipStream_t last_record_stream = nullptr;
inline size_t total_live() { size_t n = 0; for (auto& s : live) n += s.size(); return n; }
inline hipError_t create(Kind k, void** out, size_t bytes) {
  ++creates;
  if (fail_at > 0 && --fail_at == 0) return hipErrorOutOfMemory;
  *out = std::malloc(bytes ? bytes : 1);
  live[k].insert(*out);
  return hipSuccess;
}
inline hipError_t destroy(Kind k, void* p) {
  if (!live[k].erase(p)) { std::fprintf(stderr, "free of something not live (kind %d)\n", (int)k); std::abort(); }
  std::free(p);
  return hipSuccess;
}
}  // namespace fake
inline hipError_t hipMalloc(void** p, size_t n) { return fake::create(fake::DEV, p, n); }
inline hipError_t hipMemset(void*, int, size_t) { return hipSuccess; }
inline hipError_t hipFree(void* p) { return fake::destroy(fake::DEV, p); }
inline hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return fake::create(fake::PINNED, p, n); }
inline hipError_t hipHostFree(void* p) { return fake::destroy(fake::PINNED, p); }
inline hipError_t hipEventCreate(hipEvent_t* e) { return fake::create(fake::EVENT, reinterpret_cast<void**>(e), 1); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  if (flags == hipEventDisableTiming) ++fake::untimed_events;
  return fake::create(fake::EVENT, reinterpret_cast<void**>(e), 1);
}
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake::destroy(fake::EVENT, e); }
inline hipError_t hipEventSynchronize(hipEvent_t e) { if (!fake::live[fake::EVENT].count(e)) std::abort(); ++fake::syncs; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { if (!fake::live[fake::EVENT].count(e)) std::abort(); ++fake::records; fake::last_record_stream = s; return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return fake::create(fake::STREAM, reinterpret_cast<void**>(s), 1); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake::destroy(fake::STREAM, s); }
"""

DRIVER = r"""
#include "hip_owned.h"
using namespace bhip;
bool bhip::hip_ok(hipError_t e, const char*) { return e == hipSuccess; }
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
struct Group { DevBuf<float> d; PinnedBuf<int> p; StagedRing<short> r; };
static bool build(Group& g) {   // the way the library builds a lazily made group: locals first, moved into place when all is there
  Group n;
  if (!n.d.alloc(10, "d") || !n.p.alloc(10, "p") || !n.r.alloc(3, 5, "r", true)) return false;
  g = std::move(n);
  return true;
}
int main() {
  using fake::live; using fake::DEV; using fake::PINNED; using fake::EVENT; using fake::STREAM;
  {  // scope exit, reset()
    DevBuf<float> d; PinnedBuf<int> p; Event e, t; Stream s;
    CHECK(!d.get() && d.size() == 0 && !p.get() && !e.get() && !s.get() && fake::total_live() == 0);
    CHECK(d.alloc(7, "d") && p.alloc(9, "p") && e.create("e") && t.create("t", true) && s.create("s"));
    CHECK(d.get() && d.size() == 7 && p.size() == 9 && p[8] == 0 && fake::untimed_events == 1);
    CHECK(live[DEV].size() == 1 && live[PINNED].size() == 1 && live[EVENT].size() == 2 && live[STREAM].size() == 1);
    d.reset(); s.reset();
    CHECK(!d.get() && d.size() == 0 && live[DEV].empty() && live[STREAM].empty());
    CHECK(d.alloc(3, "again") && d.alloc(4, "and again") && live[DEV].size() == 1);   // alloc over a held buffer frees it
  }
  CHECK(fake::total_live() == 0);
  {  // move construction and move assignment: one owner at a time, no double free
    DevBuf<float> a;
    CHECK(a.alloc(4, "a"));
    float* raw = a.get();
    DevBuf<float> b(std::move(a));
    CHECK(!a.get() && b.get() == raw && b.size() == 4 && live[DEV].size() == 1);
    DevBuf<float> c;
    CHECK(c.alloc(5, "c") && live[DEV].size() == 2);
    c = std::move(b);
    CHECK(c.get() == raw && live[DEV].size() == 1);   // what c held is gone
    c = {};
    CHECK(!c.get() && live[DEV].empty());
    Event e; CHECK(e.create("e")); Event f(std::move(e)); CHECK(!e.get() && f.get()); e = std::move(f); CHECK(e.get() && !f.get() && live[EVENT].size() == 1);
    Stream s; CHECK(s.create("s")); Stream u(std::move(s)); s = std::move(u); CHECK(s.get() && !u.get() && live[STREAM].size() == 1);
    hipStream_t made_elsewhere = nullptr;
    CHECK(hipStreamCreateWithFlags(&made_elsewhere, 0) == hipSuccess);
    s.adopt(made_elsewhere);
    CHECK(s.get() == made_elsewhere && live[STREAM].size() == 1);
    PinnedBuf<int> p; CHECK(p.alloc(2, "p")); PinnedBuf<int> q(std::move(p)); p = std::move(q); CHECK(p.get() && !q.get() && live[PINNED].size() == 1);
    StagedRing<short> r; CHECK(r.alloc(2, 3, "r", true)); StagedRing<short> r2(std::move(r)); r = std::move(r2); CHECK(r.entries() == 2 && r2.entries() == 0);
  }
  CHECK(fake::total_live() == 0);
  {  // a group whose k-th create fails leaves nothing behind, and the target as it was
    fake::creates = 0;
    Group whole;
    CHECK(build(whole));
    const int n = fake::creates;
    CHECK(n == 7);   // DevBuf, PinnedBuf, ring: pinned + device + 3 events
    const size_t held = fake::total_live();
    float* kept = whole.d.get();
    for (int k = 1; k <= n; ++k) {
      Group g;
      fake::fail_at = k;
      CHECK(!build(g));
      CHECK(fake::fail_at == 0 && fake::total_live() == held && !g.d.get() && !g.p.get() && g.r.entries() == 0);
      fake::fail_at = k;
      CHECK(!build(whole));   // over a built group: the old one stays
      CHECK(fake::total_live() == held && whole.d.get() == kept && whole.r.entries() == 3);
    }
  }
  CHECK(fake::total_live() == 0);
  {  // claim waits exactly when the entry is marked; mark records on the stream given; forget clears without waiting
    StagedRing<short> r;
    CHECK(r.alloc(3, 5, "ring", true));
    Stream s; CHECK(s.create("s"));
    fake::syncs = fake::records = 0;
    short* e1 = r.claim(1);
    CHECK(e1 == r.host(1) && e1 == r.host(0) + 5 && r.dev(2) == r.dev(0) + 10 && fake::syncs == 0);
    CHECK(r.mark(1, s) && fake::records == 1 && fake::last_record_stream == s.get());
    CHECK(r.claim(0) && r.claim(2) && fake::syncs == 0);   // other entries do not wait
    CHECK(r.claim(1) == e1 && fake::syncs == 1);
    CHECK(r.claim(1) == e1 && fake::syncs == 1);           // the mark went with the wait
    CHECK(r.mark(0, s) && r.mark(2, s) && fake::records == 3);
    r.forget();
    CHECK(fake::syncs == 1 && r.claim(0) && r.claim(2) && fake::syncs == 1);
    CHECK(r.mark(2, s));
    r.reset();
    CHECK(r.entries() == 0 && live[EVENT].empty() && live[PINNED].empty() && live[DEV].empty());
    StagedRing<short> host_only;
    CHECK(host_only.alloc(4, 2, "host only") && live[DEV].empty() && live[PINNED].size() == 1 && live[EVENT].size() == 4);
  }
  CHECK(fake::total_live() == 0);
  std::printf("ok\n");
  return 0;
}
"""


def test_owners_free_once_and_rings_wait_when_marked(tmp_path):
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text(STAND_IN)
    src = tmp_path / "owned_driver.cc"
    src.write_text(DRIVER)
    exe = tmp_path / "owned_driver"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(tmp_path), "-I", os.path.join(ROOT, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
