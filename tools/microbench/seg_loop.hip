// The segment loop of the row-local bodies (rc::mma_segment_rt, rowchain.hip.h) ALONE: 512-thread workgroups,
// two per CU, the A operand in k-permuted LDS tiles, the packed weights of a layer of the real size streaming past -- no row
// gather from a ring, no epilogue beyond one store per accumulator.  What it answers: how far from the FP32-MFMA peak is the
// loop by itself, and what do the form of the weight loads (rc::WLane: a per-lane generic pointer taken from a table in device
// memory, flat loads as in the tick launch; rc::WGlobal: global loads off a scalar base) and the prefetch depth change?
//   ./seg_loop [rows = 1024] [launches per timing = 20] [timings = 7]
// Shapes: phone.rb (K 1280, RT 2, CG 2), a block's 1x1 layers (K 256, RT 1, CG 2), blk.a's k3 conv (K 768, RT 1, CG 2); N = 256.
// Prints per variant the median TFLOP/s over the timings, their spread, the fraction of the box's measured peak
// (peaks_mfma_f32_tflops) and a checksum of the output's bits, which must be the same for every variant of a shape (exit 1).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rowchain.hip.h"
#include "peaks.hip"

struct SegArgs {
  const float* a;   // [rows][512]: what the two LDS slots hold (segment s reads slot s & 1)
  const float* w;   // packed fragments [16 column tiles][K / 16][64] float4
  float* out;       // [rows][256]
  int rows;
};

// `tab` lives in device memory: the pointers read from it are generic to the compiler, as those of the tick launch's table are
template <class W, int RT, int NSEG, int D>
__global__ __launch_bounds__(512, 4) void seg_kernel(const SegArgs* tab) {
  constexpr int CG = 2, K = NSEG * 256;
  __shared__ __attribute__((aligned(16))) float lds[2 * RT * rc::TILE];
  const SegArgs a = *tab;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * 16 * RT;
  for (int i = tid; i < 2 * RT * 16 * 64; i += 512) {   // 16-byte pieces: slot, tile, row, piece
    const int q = i & 63, r = (i >> 6) & 15, t = (i >> 10) % RT, sl = i / (1024 * RT);
    const int m = row0 + 16 * t + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < a.rows) v = *reinterpret_cast<const float4*>(a.a + (size_t)m * 512 + sl * 256 + 4 * q);
    rc::store_perm4(lds + (sl * RT + t) * rc::TILE + r * rc::AS, 4 * q, v.x, v.y, v.z, v.w);
  }
  __syncthreads();
  W wfc[CG];
#pragma unroll
  for (int c = 0; c < CG; ++c) wfc[c] = W::make(reinterpret_cast<const float4*>(a.w) + (size_t)(wave + rc::NWAVE * c) * (K / 16) * 64, lane);
  f32x4 tot[RT][CG];
#pragma unroll
  for (int s = 0; s < NSEG; ++s) {
    f32x4 acc[RT][CG];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int c = 0; c < CG; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    W wfs[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) wfs[c] = wfc[c].at((size_t)s * 16 * 64);
    const float* ap = lds + (s & 1) * RT * rc::TILE + (lane & 15) * rc::AS + rc::lane_koff(lane);
    rc::mma_segment_rt<RT, CG, 16, D>(acc, ap, rc::TILE, wfs);
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int c = 0; c < CG; ++c) {
        if (s == 0) tot[t][c] = acc[t][c];
        else { tot[t][c][0] = tot[t][c][0] + acc[t][c][0]; tot[t][c][1] = tot[t][c][1] + acc[t][c][1]; tot[t][c][2] = tot[t][c][2] + acc[t][c][2]; tot[t][c][3] = tot[t][c][3] + acc[t][c][3]; }
      }
    if (s + 1 < NSEG) __syncthreads();   // (the product's one barrier per segment)
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int m = row0 + 16 * t + (lane & 15);
    if (m >= a.rows) continue;
#pragma unroll
    for (int c = 0; c < CG; ++c)
      *reinterpret_cast<float4*>(a.out + (size_t)m * 256 + (wave + rc::NWAVE * c) * 16 + (lane >> 4) * 4) = make_float4(tot[t][c][0], tot[t][c][1], tot[t][c][2], tot[t][c][3]);
  }
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
static double g_peak = 0.0;
static int g_rows = 1024, g_launches = 20, g_timings = 7;
static float *g_a, *g_w, *g_out;
static SegArgs* g_tab;

struct Result { double tf, spread; uint64_t sum; };
template <class W, int RT, int NSEG, int D>
static Result run_one(const char* shape, const char* loads) {
  const dim3 grid((g_rows + 16 * RT - 1) / (16 * RT));
  (void)hipMemset(g_out, 0, (size_t)g_rows * 256 * 4);
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int it = 0; it < 3; ++it) hipLaunchKernelGGL((seg_kernel<W, RT, NSEG, D>), grid, dim3(512), 0, 0, g_tab);
  std::vector<double> tf;
  for (int r = 0; r < g_timings; ++r) {
    (void)hipEventRecord(e0);
    for (int it = 0; it < g_launches; ++it) hipLaunchKernelGGL((seg_kernel<W, RT, NSEG, D>), grid, dim3(512), 0, 0, g_tab);
    (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "launch failed: %s %s D %d\n", shape, loads, D); exit(2); }
    float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
    tf.push_back(2.0 * g_rows * (NSEG * 256.0) * 256.0 * g_launches / (ms * 1e-3) / 1e12);
  }
  std::sort(tf.begin(), tf.end());
  std::vector<uint32_t> h((size_t)g_rows * 256);
  (void)hipMemcpy(h.data(), g_out, h.size() * 4, hipMemcpyDeviceToHost);
  uint64_t sum = 1469598103934665603ull;
  for (uint32_t v : h) sum = (sum ^ v) * 1099511628211ull;
  const Result res{tf[tf.size() / 2], tf.back() - tf.front(), sum};
  printf("%-10s K %4d RT %d CG 2  %-6s D %d  %7.3f TFLOP/s  spread %.3f  %.3f of peak  checksum %016llx\n", shape, NSEG * 256, RT, loads, D, res.tf,
         res.spread, g_peak > 0 ? res.tf / g_peak : 0.0, (unsigned long long)res.sum);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return res;
}
template <int RT, int NSEG>
static bool run_shape(const char* shape) {
  const Result r[6] = {run_one<rc::WLane, RT, NSEG, 2>(shape, "flat"),     run_one<rc::WLane, RT, NSEG, 4>(shape, "flat"),
                       run_one<rc::WLane, RT, NSEG, 8>(shape, "flat"),     run_one<rc::WGlobal, RT, NSEG, 2>(shape, "global"),
                       run_one<rc::WGlobal, RT, NSEG, 4>(shape, "global"), run_one<rc::WGlobal, RT, NSEG, 8>(shape, "global")};
  bool same = true;
  for (int i = 1; i < 6; ++i) same = same && r[i].sum == r[0].sum;
  if (!same) fprintf(stderr, "%s: the variants' outputs DIFFER in their bits\n", shape);
  return same;
}

int main(int argc, char** argv) {
  if (argc > 1) g_rows = atoi(argv[1]);
  if (argc > 2) g_launches = atoi(argv[2]);
  if (argc > 3) g_timings = atoi(argv[3]);
  if (g_rows < 1 || g_rows > (1 << 20) || g_launches < 1 || g_timings < 1) { fprintf(stderr, "usage: seg_loop [rows] [launches] [timings]\n"); return 2; }
  const size_t na = (size_t)g_rows * 512, nw = (size_t)1280 * 256;   // the largest layer's weights
  if (hipMalloc(&g_a, na * 4) != hipSuccess || hipMalloc(&g_w, nw * 4) != hipSuccess || hipMalloc(&g_out, (size_t)g_rows * 256 * 4) != hipSuccess ||
      hipMalloc(&g_tab, sizeof(SegArgs)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 2; }
  std::vector<float> ha(na), hw(nw);
  uint32_t s = 12345u;
  for (float& v : ha) v = (float)((int)(lcg(s) >> 8) % 2001 - 1000) * 1e-3f;
  for (float& v : hw) v = (float)((int)(lcg(s) >> 8) % 2001 - 1000) * 1e-3f;
  (void)hipMemcpy(g_a, ha.data(), na * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(g_w, hw.data(), nw * 4, hipMemcpyHostToDevice);
  const SegArgs tab{g_a, g_w, g_out, g_rows};
  (void)hipMemcpy(g_tab, &tab, sizeof(tab), hipMemcpyHostToDevice);
  g_peak = peaks_mfma_f32_tflops(20000, 3);
  hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
  printf("%d rows, %d CUs, peaks_mfma_f32_tflops %.2f; median of %d timings of %d launches\n", g_rows, p.multiProcessorCount, g_peak, g_timings, g_launches);
  bool ok = true;
  ok = run_shape<2, 5>("phone.rb") && ok;
  ok = run_shape<1, 1>("blk.1x1") && ok;
  ok = run_shape<1, 3>("blk.a.k3") && ok;
  return ok ? 0 : 1;
}
