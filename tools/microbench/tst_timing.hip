// Per-phase timing of the tail-stage bodies (tail_stages.hip.h) as launches of their own: B streams, zero data.
//   ./tst_timing [B] [copies]     copies > 1: that many launches' worth of workgroups in one grid (co-residency with itself)
// The one-hop bodies of the full table (T1Op, T2Op) and the three bodies of the four-hop table (one stream per workgroup; T2 and T3 in
// two sub-steps, a line per sub-step).
#define TST_TIMING
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv_gemm.hip.h"
#include "tail_stages.hip.h"
constexpr int kStamps = 32;   // per workgroup (tail_stages.hip.h TST_STAMP: sub-step u at [10 u, 10 u + 8])
template <class Op>
__global__ __launch_bounds__(512, 4) void probe(const tst::StageArgs a, int wgs) {
  __shared__ __attribute__((aligned(16))) float lds[Op::LDS_FLOATS];
  Op::run(a, blockIdx.x % wgs, 0, lds);
}
template <class Op>
void run(const char* name, tst::StageArgs a, int copies, unsigned long long* st, int nsub) {
  const int wgs = Op::grid(a).x, total = wgs * copies;
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipMemset(st, 0, (size_t)total * kStamps * 8);
  for (int it = 0; it < 3; ++it) hipLaunchKernelGGL(probe<Op>, dim3(total), dim3(512), 0, 0, a, wgs);
  hipEventRecord(e0);
  for (int it = 0; it < 10; ++it) hipLaunchKernelGGL(probe<Op>, dim3(total), dim3(512), 0, 0, a, wgs);
  hipEventRecord(e1); hipDeviceSynchronize();
  float ms; hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> h((size_t)total * kStamps);
  hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost);
  auto mean = [&](int from, int to) {
    double s = 0; for (int w = 0; w < total; ++w) s += (double)(h[(size_t)w * kStamps + to] - h[(size_t)w * kStamps + from]);
    return s / total;
  };
  printf("%s: %d workgroups, %.2f us per launch; wavefront 0, shader cycles per phase\n", name, total, ms * 100.0);
  for (int u = 0; u < nsub; ++u) {
    printf("  sub-step %d:", u);
    for (int i = 0; i < 8; ++i) printf(" %.0f", mean(10 * u + i, 10 * u + i + 1));
    printf("\n");
  }
  printf("  total %.0f\n", mean(0, 10 * (nsub - 1) + 8));
}
int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 256, copies = argc > 2 ? atoi(argv[2]) : 1;
  constexpr int H = 4;   // (the buffers are those of the four-hop shapes; the one-hop bodies use a part of them)
  const size_t n_in = (size_t)B * 2 * 20 * H * 64, n_mid = (size_t)B * 2 * 80 * H * 32, n_out = (size_t)B * 2 * 240 * H * 16, n_smp = (size_t)B * 240 * H;
  float *ring_in, *ring_mid, *ring_out, *state, *w, *bias, *out; unsigned long long* st;
  hipMalloc(&ring_in, n_in * 4); hipMalloc(&ring_mid, n_mid * 4); hipMalloc(&ring_out, n_out * 4);
  hipMalloc(&state, (size_t)B * TAIL_STATE_FLOATS * 4); hipMalloc(&w, 1 << 20); hipMalloc(&bias, 4096); hipMalloc(&out, n_smp * 4);
  hipMalloc(&st, (size_t)B * copies * kStamps * 8);
  hipMemset(ring_in, 0, n_in * 4); hipMemset(ring_mid, 0, n_mid * 4); hipMemset(ring_out, 0, n_out * 4);
  hipMemset(state, 0, (size_t)B * TAIL_STATE_FLOATS * 4); hipMemset(w, 0, 1 << 20); hipMemset(bias, 0, 4096);
  hipMemcpyToSymbol(HIP_SYMBOL(g_tst_stamps), &st, sizeof(st));
  int* hop; hipMalloc(&hop, 8); hipMemset(hop, 0, 8);
  tst::StageArgs a{};
  a.state = state; a.hop = hop; a.B = B; a.fin_w = w; a.fin_b = bias; a.d_out = out;
  for (int i = 0; i < 3; ++i) { a.w[i] = w + i * 30000; a.b[i] = bias; }
  printf("phases of a sub-step: prologue (loads + stores) | barrier | resA | barrier | resB | barrier | up (T3: output conv) | state out, or the sub-step boundary (two barriers and the history copy)\n");
  a.in = Ring{ring_in, 64, 20, 2}; a.out = Ring{ring_mid, 32, 80, 2};
  run<tst::T1Op>("T1, one hop, 4 streams", a, copies, st, 1);
  a.in = Ring{ring_mid, 32, 80, 2}; a.out = Ring{ring_out, 16, 240, 2};
  run<tst::T2Op>("T2, one hop, 3 streams", a, copies, st, 1);
  a.in = Ring{ring_in, 64, 20 * H, 2}; a.out = Ring{ring_mid, 32, 80 * H, 2};
  run<tst::T1OpS<1, H>>("T1, four hops, 1 stream x 80 frames", a, copies, st, 1);
  a.in = Ring{ring_mid, 32, 80 * H, 2}; a.out = Ring{ring_out, 16, 240 * H, 2};
  run<tst::T2OpS<1, H, 2>>("T2, four hops, 1 stream x 2 x 160 frames", a, copies, st, 2);
  a.in = Ring{ring_out, 16, 240 * H, 2}; a.out = Ring{};
  run<tst::T3OpS<1, H, 2>>("T3, four hops, 1 stream x 2 x 480 frames", a, copies, st, 2);
  return 0;
}
