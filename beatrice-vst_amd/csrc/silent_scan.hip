// silent_scan.hip -- the shell's silent-block test on blocks that live on the device (BeatriceBatch_ScanSilentBlocks*, batch.hip).
//
// The rule (reference src/vst/processor.cc:204-214, BeatriceBatch_ConvertBlocks48k's host loop): a block is silent when no sample of its
// down-mix -- x[i], or (x0[i] + x1[i]) * 0.5f -- differs from 0.0f, in float32 with subnormals kept.  One wavefront takes one block:
// its lanes walk the samples 64 (or, by 16-byte loads, 256) at a time, each lane keeps "one of mine differed", one ballot joins the 64
// answers and lane 0 stores the block's byte.  No LDS, no atomics, nothing between workgroups.  Which floats a lane reads, and why they
// are the caller's, is silent_scan_plan.h's subject; the loops below are exactly the ones it describes.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "silent_scan_plan.h"

namespace bhip {

namespace {

using sscan::kThreads;
using sscan::kWavesPerGroup;

__device__ __forceinline__ bool differs(const float m) { return m != 0.0f; }   // (true for NaN)
__device__ __forceinline__ float downmix(const float l, const float r) { float m = l + r; m = m * 0.5f; return m; }

// kVec: every block's base, length and channel offset are multiples of four floats (sscan::vector_path)
template <bool kVec>
__global__ __launch_bounds__(kThreads) void silent_scan_kernel(const float* __restrict__ blocks, const int n_blocks, const int J, const int channels,
                                                               const int n, const long long stride, const int* __restrict__ cell_len,
                                                               unsigned char* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int blk = (int)blockIdx.x * kWavesPerGroup + (int)(threadIdx.x >> 6);   // (n_blocks <= 2^20)
  if (blk >= n_blocks) return;   // (a whole wavefront)
  const int c = blk / J, j = blk - c * J;
  const int len = cell_len ? cell_len[c] : n;   // (per-cell lengths: J == 1, the block sits at the start of its cell)
  const float* x0 = blocks + (long long)c * stride + (long long)j * channels * n;
  const float* x1 = x0 + len;
  // Every load is issued whatever the samples before it were, and the compares are joined with | (no short-circuit): a lane's loads
  // of an unrolled group are in flight together, and both channels of the 16-byte path stay whole 16-byte loads.
  // (i += 64 cannot wrap: len <= sscan::kMaxSamples = 2^30)
  int loud = 0;
  if (kVec) {
    const float4* v0 = reinterpret_cast<const float4*>(x0);
    const float4* v1 = reinterpret_cast<const float4*>(x1);
    const int items = len / 4;
    if (channels == 1) {
#pragma unroll 4
      for (int i = lane; i < items; i += 64) {
        const float4 a = v0[i];
        loud |= (int)differs(a.x) | (int)differs(a.y) | (int)differs(a.z) | (int)differs(a.w);
      }
    } else {
#pragma unroll 4
      for (int i = lane; i < items; i += 64) {
        const float4 a = v0[i], r = v1[i];
        loud |= (int)differs(downmix(a.x, r.x)) | (int)differs(downmix(a.y, r.y)) | (int)differs(downmix(a.z, r.z)) | (int)differs(downmix(a.w, r.w));
      }
    }
  } else {
    if (channels == 1) {
#pragma unroll 4
      for (int i = lane; i < len; i += 64) loud |= (int)differs(x0[i]);
    } else {
#pragma unroll 4
      for (int i = lane; i < len; i += 64) loud |= (int)differs(downmix(x0[i], x1[i]));
    }
  }
  const unsigned long long any = __ballot(loud != 0);
  if (lane == 0) flags[blk] = any == 0 ? 1 : 0;
}

}  // namespace

bool silent_scan(const float* d_blocks, const sscan::Geometry& g, bool vec, const int* cell_len, unsigned char* d_flags, hipStream_t stream) {
  if (g.blocks() < 1 || g.blocks() > sscan::kMaxBlocks || g.n > sscan::kMaxSamples) return false;
  const dim3 grid(sscan::grid(g)), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(silent_scan_kernel<true>, grid, block, 0, stream, d_blocks, (int)g.blocks(), (int)g.J, (int)g.channels, (int)g.n, g.stride,
                       cell_len, d_flags);
  else
    hipLaunchKernelGGL(silent_scan_kernel<false>, grid, block, 0, stream, d_blocks, (int)g.blocks(), (int)g.J, (int)g.channels, (int)g.n, g.stride,
                       cell_len, d_flags);
  return hip_ok(hipGetLastError(), "silent scan launch");
}

}  // namespace bhip
