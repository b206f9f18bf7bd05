// One GRU cell of the tick launch as a launch of its own, in three forms beside each other: the column-split cell (fused_small.hip.h
// gru_fused_body, 32 streams x 16 hidden units per workgroup, 384 threads), the rows cell of the tick tables (rowchain.hip.h
// gru_rows_body, 32 streams x 64 hidden units) and its other split, 16 streams x 128 hidden units (RT = 1: half the gather per
// workgroup, every weight streamed once per 16 rows instead of once per 32).  One cell, no links, both GRU sizes.  The argument block
// is READ FROM A TABLE IN DEVICE MEMORY as in the tick launch (its pointers are then generic to the compiler), and the probes are
// compiled as the tick launch is: 512 threads, __launch_bounds__(512, 4).
//   ./gru_cell [B] [copies]    copies > 1: that many launches' worth of workgroups in one grid; the copies of a workgroup read and
//                              rewrite the same rows (the same values: a cell at a fixed step counter is idempotent)
// Prints per form: median of 7 timings (20 launches each), spread = max - min of the 7, checksum of the state ring -- the three
// checksums of a size are equal (the forms are bit-identical).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv_gemm.hip.h"
#include "fused_small.hip.h"
#include "rowchain.hip.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <class Op>
__global__ __launch_bounds__(512, 4) void probe(const GruArgs* __restrict__ table, int gx, int wgs) {
  __shared__ __attribute__((aligned(16))) float lds[Op::LDS_FLOATS];
  const GruArgs a = table[0];   // (uniform: scalar loads; the pointers are generic from here on)
  const int id = blockIdx.x % wgs;
  if ((int)threadIdx.x < Op::NTHR) Op::run(a, id % gx, id / gx, lds);
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
static void run(const char* name, GruArgs a, int copies, int H) {
  const size_t n_state = (size_t)a.B * 2 * H;
  float* state = device_floats(n_state, 2, 0.5f);   // (every form starts from the same state ring)
  a.h.base = state;
  GruArgs* table; CHECK(hipMalloc(&table, sizeof(a))); CHECK(hipMemcpy(table, &a, sizeof(a), hipMemcpyHostToDevice));
  const dim3 g = Op::grid(a);
  const int wgs = g.x * g.y, total = wgs * copies;
  hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  for (int it = 0; it < 5; ++it) hipLaunchKernelGGL(probe<Op>, dim3(total), dim3(512), 0, 0, table, (int)g.x, wgs);
  CHECK(hipDeviceSynchronize());
  std::vector<float> us;
  for (int rep = 0; rep < 7; ++rep) {
    CHECK(hipEventRecord(e0));
    for (int it = 0; it < 20; ++it) hipLaunchKernelGGL(probe<Op>, dim3(total), dim3(512), 0, 0, table, (int)g.x, wgs);
    CHECK(hipEventRecord(e1)); CHECK(hipDeviceSynchronize());
    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
    us.push_back(ms * 1000.0f / 20);
  }
  std::sort(us.begin(), us.end());
  printf("%-44s %4d workgroups, median %.2f us per launch, spread %.2f; checksum state %.9g\n", name, total, us[3], us[6] - us[0], checksum(state, n_state));
  CHECK(hipFree(table)); CHECK(hipFree(state));
}

template <int IN, int H>
static void cell(const char* what, int B, int copies) {
  // x: a ring of one frame per step, two step slots; h: the same (the previous state = frame -1)
  float* x = device_floats((size_t)B * 2 * IN, 1, 0.5f);
  float* wih = device_floats((size_t)IN * 3 * H, 3, 0.05f);
  float* whh = device_floats((size_t)H * 3 * H, 4, 0.05f);
  float* bih = device_floats(3 * H, 5, 0.1f);
  float* bhh = device_floats(3 * H, 6, 0.1f);
  GruArgs a{};
  a.x = Ring{x, IN, 1, 2}; a.h = Ring{nullptr, H, 1, 2};
  a.wih = wih; a.whh = whh; a.bih = bih; a.bhh = bhh;
  a.hop = stepc::immediate(0); a.B = B; a.t = 0; a.passes = 1;
  char name[96];
  snprintf(name, sizeof name, "%s, 32 streams x 16 units (column split)", what); run<GruOp<IN, H, 2, 0>>(name, a, copies, H);
  snprintf(name, sizeof name, "%s, 32 streams x 64 units (rows)", what); run<rc::GruRowsOp<IN, H, 0, 2>>(name, a, copies, H);
  snprintf(name, sizeof name, "%s, 16 streams x 128 units (rows)", what); run<rc::GruRowsOp<IN, H, 0, 1>>(name, a, copies, H);
  CHECK(hipFree(x)); CHECK(hipFree(wih)); CHECK(hipFree(whh)); CHECK(hipFree(bih)); CHECK(hipFree(bhh));
}

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 256, copies = argc > 2 ? atoi(argv[2]) : 1;
  cell<256, 256>("phone GRU 256 -> 256", B, copies);
  cell<128, 128>("pitch GRU 128 -> 128", B, copies);
  return 0;
}
