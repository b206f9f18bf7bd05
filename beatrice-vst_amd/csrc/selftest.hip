// selftest.hip -- device-side exhaustive checks of the packed scalar functions of spec_math.hip.h against their scalar
// definitions (which the parity tests pin to the oracle).  Test infrastructure exported from the product library because
// the functions under test are device code: BeatriceHip_MathSelfTest(which) sweeps all 2^32 float32 bit patterns (NaNs
// excluded) and returns the number of inputs whose results differ in any bit; -1 on a HIP failure.
//   which: 0 exp2 vs exp, 1 tanh2 vs tanh, 2 gelu2 vs gelu, 3 sigmoid2 vs sigmoid
// BeatriceHip_MathEval(which, bits, n, out_bits) evaluates one function at n caller-chosen points and hands the result bits back, so a
// test can compare the device functions with oracle/spec_math.h directly (tests/test_gpu_spec_math.py).
//   which: 0 exp, 1 tanh, 2 gelu, 3 sigmoid, 4 log, 5 lrelu (scalar); 6 exp2, 7 tanh2, 8 gelu2, 9 sigmoid2 (points taken in pairs)
#include <hip/hip_runtime.h>

#include "engine.h"
#include "spec_math.hip.h"

namespace {
template <int WHICH>
__global__ __launch_bounds__(256) void sweep_kernel(unsigned long long* bad, unsigned* first_bad) {
  // thread t of the grid covers patterns 2 (t + k * stride), + 1
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long mine = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 31); i += stride) {
    const uint32_t b0 = (uint32_t)(2 * i), b1 = b0 + 1;
    const float x0 = __uint_as_float(b0), x1 = __uint_as_float(b1);
    const bsp::f32x2 x{x0, x1};
    bsp::f32x2 got;
    float w0, w1;
    if (WHICH == 0) { got = bsp::exp2(x); w0 = bsp::exp(x0); w1 = bsp::exp(x1); }
    else if (WHICH == 1) { got = bsp::tanh2(x); w0 = bsp::tanh(x0); w1 = bsp::tanh(x1); }
    else if (WHICH == 2) { got = bsp::gelu2(x); w0 = bsp::gelu(x0); w1 = bsp::gelu(x1); }
    else { got = bsp::sigmoid2(x); w0 = bsp::sigmoid(x0); w1 = bsp::sigmoid(x1); }
    const bool n0 = x0 != x0, n1 = x1 != x1;
    if (!n0 && __float_as_uint(got.x) != __float_as_uint(w0)) { ++mine; atomicMin(first_bad, b0); }
    if (!n1 && __float_as_uint(got.y) != __float_as_uint(w1)) { ++mine; atomicMin(first_bad, b1); }
  }
  if (mine) atomicAdd(bad, mine);
}

template <int WHICH>
__global__ __launch_bounds__(256) void eval_kernel(const uint32_t* __restrict__ bits, size_t n, uint32_t* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (WHICH < 6) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const float x = __uint_as_float(bits[i]);
      float y;
      if (WHICH == 0) y = bsp::exp(x);
      else if (WHICH == 1) y = bsp::tanh(x);
      else if (WHICH == 2) y = bsp::gelu(x);
      else if (WHICH == 3) y = bsp::sigmoid(x);
      else if (WHICH == 4) y = bsp::log(x);
      else y = bsp::lrelu(x);
      out[i] = __float_as_uint(y);
    }
  } else {
    // pair p holds points 2p and 2p + 1; an odd count pairs the last point with itself
    const size_t pairs = (n + 1) / 2;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += stride) {
      const size_t i0 = 2 * p, i1 = (2 * p + 1 < n) ? 2 * p + 1 : i0;
      const bsp::f32x2 x{__uint_as_float(bits[i0]), __uint_as_float(bits[i1])};
      bsp::f32x2 y;
      if (WHICH == 6) y = bsp::exp2(x);
      else if (WHICH == 7) y = bsp::tanh2(x);
      else if (WHICH == 8) y = bsp::gelu2(x);
      else y = bsp::sigmoid2(x);
      out[i0] = __float_as_uint(y.x);
      if (i1 != i0) out[i1] = __float_as_uint(y.y);
    }
  }
}
}  // namespace

extern "C" int BeatriceHip_MathEval(int which, const uint32_t* bits, size_t n, uint32_t* out_bits) {
  if (which < 0 || which > 9 || (n && (!bits || !out_bits))) return -1;
  if (n == 0) return 0;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_in), n * 4) != hipSuccess) return -1;
  if (hipMalloc(reinterpret_cast<void**>(&d_out), n * 4) != hipSuccess) { (void)hipFree(d_in); return -1; }
  bool ok = hipMemcpy(d_in, bits, n * 4, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    const size_t blocks = (n + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(256);
    switch (which) {
      case 0: hipLaunchKernelGGL(eval_kernel<0>, grid, block, 0, 0, d_in, n, d_out); break;
      case 1: hipLaunchKernelGGL(eval_kernel<1>, grid, block, 0, 0, d_in, n, d_out); break;
      case 2: hipLaunchKernelGGL(eval_kernel<2>, grid, block, 0, 0, d_in, n, d_out); break;
      case 3: hipLaunchKernelGGL(eval_kernel<3>, grid, block, 0, 0, d_in, n, d_out); break;
      case 4: hipLaunchKernelGGL(eval_kernel<4>, grid, block, 0, 0, d_in, n, d_out); break;
      case 5: hipLaunchKernelGGL(eval_kernel<5>, grid, block, 0, 0, d_in, n, d_out); break;
      case 6: hipLaunchKernelGGL(eval_kernel<6>, grid, block, 0, 0, d_in, n, d_out); break;
      case 7: hipLaunchKernelGGL(eval_kernel<7>, grid, block, 0, 0, d_in, n, d_out); break;
      case 8: hipLaunchKernelGGL(eval_kernel<8>, grid, block, 0, 0, d_in, n, d_out); break;
      default: hipLaunchKernelGGL(eval_kernel<9>, grid, block, 0, 0, d_in, n, d_out); break;
    }
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(out_bits, d_out, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
  }
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return ok ? 0 : -1;
}

extern "C" long long BeatriceHip_MathSelfTest(int which, unsigned* first_bad_bits) {
  unsigned long long* d_bad = nullptr;
  unsigned* d_first = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_bad), 8) != hipSuccess) return -1;
  if (hipMalloc(reinterpret_cast<void**>(&d_first), 4) != hipSuccess) { (void)hipFree(d_bad); return -1; }
  (void)hipMemset(d_bad, 0, 8);
  (void)hipMemset(d_first, 0xff, 4);
  const dim3 grid(256 * 16), block(256);
  switch (which) {
    case 0: hipLaunchKernelGGL(sweep_kernel<0>, grid, block, 0, 0, d_bad, d_first); break;
    case 1: hipLaunchKernelGGL(sweep_kernel<1>, grid, block, 0, 0, d_bad, d_first); break;
    case 2: hipLaunchKernelGGL(sweep_kernel<2>, grid, block, 0, 0, d_bad, d_first); break;
    case 3: hipLaunchKernelGGL(sweep_kernel<3>, grid, block, 0, 0, d_bad, d_first); break;
    default: (void)hipFree(d_bad); (void)hipFree(d_first); return -1;
  }
  unsigned long long bad = 0;
  unsigned first = 0xffffffffu;
  const bool ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost) == hipSuccess &&
                  hipMemcpy(&first, d_first, 4, hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(d_bad);
  (void)hipFree(d_first);
  if (first_bad_bits) *first_bad_bits = first;
  return ok ? (long long)bad : -1;
}
