// The tail stages' T1, T2 and T3 bodies at four hops per step (tail_stages.hip.h, the shapes of the tick launch: one stream per workgroup,
// T2 and T3 in two sub-steps) as launches of their own, with the argument block READ FROM A TABLE IN DEVICE MEMORY as in the tick launch --
// its pointers are then generic to the compiler, and -DTST_GLOBAL=0 compiles to flat loads and stores as the tick's bodies did.
// Built twice (tools/README.md): tail_stage_loop_flat with -DTST_GLOBAL=0, tail_stage_loop_global without; run one after the other,
// they print the same checksums at copies = 1 (compare the two outputs with `diff` after cutting the timing fields, tools/README.md).
// TST_GLOBAL=0 is NOT the code before the change: it is the new 32-bit-offset addressing over generic pointers (ring.h FBase), so
// the pair isolates the form of the accesses; the deciding A/B is the product against its parent commit.
//   ./tail_stage_loop_<form> [B] [copies]    copies > 1: that many launches' worth of workgroups in one grid (two per CU at B = 256);
//                                            the copies of a workgroup then read and rewrite ONE stream's state block and ring slots
//                                            in the same launch -- timing only, the checksums of such a run are not to be compared
// The probes are compiled as the tick launch is: 512 threads, __launch_bounds__(512, 4) = at most 128 VGPRs, two workgroups per CU by
// registers (T1's 65 KB of LDS allow two as well, T2's 45 KB three); compiled alone they spill 9 (T1) and 14 (T2) VGPRs, the table kernel 121.
// Prints per body: median of 7 timings (20 launches each), spread = max - min of the 7, checksum of everything the body wrote.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv_gemm.hip.h"
#include "tail_stages.hip.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <class Op>
__global__ __launch_bounds__(512, 4) void probe(const tst::StageArgs* __restrict__ table, int wgs) {
  __shared__ __attribute__((aligned(16))) float lds[Op::LDS_FLOATS];
  const tst::StageArgs a = table[0];   // (uniform: scalar loads; the pointers are generic from here on)
  Op::run(a, blockIdx.x % wgs, 0, lds);
}

static float* device_floats(size_t n, unsigned seed, float amp) {
  std::vector<float> h(n);
  unsigned s = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = amp * ((float)(s >> 8) / 8388608.0f - 1.0f); }
  float* d; CHECK(hipMalloc(&d, n * 4)); CHECK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
  return d;
}
static double checksum(const float* d, size_t n) {
  std::vector<float> h(n);
  CHECK(hipMemcpy(h.data(), d, n * 4, hipMemcpyDeviceToHost));
  double s = 0; for (size_t i = 0; i < n; ++i) s += (double)h[i] * (double)(1 + i % 7);
  return s;
}

template <class Op>
static void run(const char* name, const tst::StageArgs& a, int copies, const float* out, size_t n_out, const float* state, size_t n_state) {
  tst::StageArgs* table; CHECK(hipMalloc(&table, sizeof(a))); CHECK(hipMemcpy(table, &a, sizeof(a), hipMemcpyHostToDevice));
  const int wgs = Op::grid(a).x, total = wgs * copies;
  hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  for (int it = 0; it < 5; ++it) hipLaunchKernelGGL(probe<Op>, dim3(total), dim3(512), 0, 0, table, wgs);
  CHECK(hipDeviceSynchronize());
  std::vector<float> us;
  for (int rep = 0; rep < 7; ++rep) {
    CHECK(hipEventRecord(e0));
    for (int it = 0; it < 20; ++it) hipLaunchKernelGGL(probe<Op>, dim3(total), dim3(512), 0, 0, table, wgs);
    CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
    us.push_back(ms * 1000.0f / 20);
  }
  std::sort(us.begin(), us.end());
  printf("%s TST_GLOBAL=%d: %d workgroups, median %.2f us per launch, spread %.2f; checksum out %.9g state %.9g\n", name, TST_GLOBAL, total, us[3],
         us[6] - us[0], checksum(out, n_out), checksum(state, n_state));
  CHECK(hipFree(table));
}

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 256, copies = argc > 2 ? atoi(argv[2]) : 1;
  constexpr int H = 4;
  // rings of two step slots: up2's output (64 channels, 20 H frames per step), T1's (32 x 80 H), T2's (16 x 240 H)
  const size_t n_in = (size_t)B * 2 * 20 * H * 64, n_mid = (size_t)B * 2 * 80 * H * 32, n_out = (size_t)B * 2 * 240 * H * 16, n_state = (size_t)B * TAIL_STATE_FLOATS;
  float* ring_in = device_floats(n_in, 1, 0.5f);
  float* ring_mid = device_floats(n_mid, 2, 0.5f);
  float* ring_out = device_floats(n_out, 3, 0.5f);
  float* state1 = device_floats(n_state, 4, 0.5f);
  float* state2 = device_floats(n_state, 4, 0.5f);
  float* w = device_floats(3 * 30000, 5, 0.05f);
  float* bias = device_floats(1024, 6, 0.1f);
  tst::StageArgs a{};
  a.hop = stepc::immediate(0); a.B = B;
  for (int i = 0; i < 3; ++i) { a.w[i] = w + i * 30000; a.b[i] = bias + i * 128; }
  a.fin_w = w; a.fin_b = bias; a.d_out = nullptr;
  a.state = state1; a.in = Ring{ring_in, 64, 20 * H, 2}; a.out = Ring{ring_mid, 32, 80 * H, 2};
  // (the bodies rewrite their histories in the state block every launch: the checksums are those after the same number of launches)
  run<tst::T1OpS<1, H>>("T1 (1 stream, 80 frames)", a, copies, ring_mid, n_mid, state1, n_state);
  float* ring_mid2 = device_floats(n_mid, 2, 0.5f);   // (T2's input as it was before T1 ran: the two bodies are timed apart)
  a.state = state2; a.in = Ring{ring_mid2, 32, 80 * H, 2}; a.out = Ring{ring_out, 16, 240 * H, 2};
  run<tst::T2OpS<1, H, 2>>("T2 (1 stream, 2 x 160 frames)", a, copies, ring_out, n_out, state2, n_state);
  float* ring_out2 = device_floats(n_out, 3, 0.5f);   // (T3's input as it was before T2 ran)
  float* state3 = device_floats(n_state, 4, 0.5f);
  const size_t n_samples = (size_t)B * 240 * H;
  float* samples; CHECK(hipMalloc(&samples, n_samples * 4)); CHECK(hipMemset(samples, 0, n_samples * 4));
  a.state = state3; a.in = Ring{ring_out2, 16, 240 * H, 2}; a.out = Ring{}; a.d_out = samples; a.io_stride = 0;
  run<tst::T3OpS<1, H, 2>>("T3 (1 stream, 2 x 480 frames)", a, copies, samples, n_samples, state3, n_state);
  return 0;
}
