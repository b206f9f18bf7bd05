// install.hip -- a caller's speaker tables go from pinned host staging into table entries in ONE launch
// (BeatriceBatch_InstallSpeakersInFlight, batch.hip).
//
// What it replaces: BeatriceBatch_UpdateSpeaker's three blocking copies and codebook_prep_kernel (kernels_misc.hip.h), whose thread j
// walks codebook row j with a 512-byte stride -- fine in device memory, not over the host link.  Here every staged byte crosses the link
// exactly once, as 16-byte loads of consecutive lanes, and everything derived from it is made on the way: the raw tables are plain
// copies; a tile of kRows codebook rows passes through LDS to come out as kRows consecutive floats of each of the 128 rows of the
// transposed table, and one thread per row sums its squares from the same tile.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "spec_math.hip.h"

namespace bhip {

namespace {

// A unit of work = kUnit floats of one entry's staging, one workgroup: a tile of kRows codebook rows, kRows key/value tokens, or the
// additive row (a quarter of a wavefront's worth: the one short unit).
constexpr int kThreads = 256, kRows = 64, kUnit = kRows * B_PHONE_CH;
constexpr int kPerThread = kUnit / 4 / kThreads;   // float4 per thread
constexpr int kCbUnits = B_CODEBOOK / kRows, kKvUnits = B_KV_LEN * B_KV_CH / kUnit, kUnits = kCbUnits + kKvUnits + 1;
// LDS tile [kRows][kPitch]: a pitch of 129 words puts the 64 rows of one column on 64 different words mod 32 per half-wave, so the
// transposed reads (lane = row, fixed channel) and the norm chains (thread = row, channel ascending) are conflict-free ds_read_b32.
// The price is on the other side: a row's float4 goes in as four ds_write_b32 that are 4-way conflicted (channels 4q + k, q = 0 .. 31,
// cover 8 banks) -- 32 writes per thread, against 128 + 32 dependent reads.
constexpr int kPitch = B_PHONE_CH + 1;
static_assert(B_PHONE_CH == B_KV_CH && B_CODEBOOK % kRows == 0 && (B_KV_LEN * B_KV_CH) % kUnit == 0 && kUnit % (4 * kThreads) == 0, "units");
static_assert(B_HID / 4 <= kThreads && B_PHONE_CH % (kThreads / 64) == 0, "units");
static_assert(kInstallEntryFloats == B_CODEBOOK * B_PHONE_CH + B_HID + B_KV_LEN * B_KV_CH, "staging layout");

__global__ __launch_bounds__(kThreads) void install_entries_kernel(const MorphDesc* __restrict__ descs, const float* __restrict__ staged,
                                                                   const int n, const int n_entries, float* __restrict__ cb_raw,
                                                                   float* __restrict__ add_raw, float* __restrict__ kv_raw,
                                                                   float* __restrict__ cbT, float* __restrict__ cnorm) {
  __shared__ float tile[kRows * kPitch];
  const int i = blockIdx.x / kUnits, u = blockIdx.x % kUnits, t = threadIdx.x;
  if (i >= n) return;
  const int slot = descs[i].slot;
  if (slot < 0 || slot >= n_entries) return;   // (a descriptor the host did not write: nothing is touched)
  const float* entry = staged + (size_t)i * kInstallEntryFloats;   // [codebook 512 x 128][additive 256][key/value 384 x 128]
  if (u == kUnits - 1) {
    if (t < B_HID / 4)
      reinterpret_cast<float4*>(add_raw + (size_t)slot * B_HID)[t] = reinterpret_cast<const float4*>(entry + B_CODEBOOK * B_PHONE_CH)[t];
    return;
  }
  const bool is_cb = u < kCbUnits;
  const float4* src = reinterpret_cast<const float4*>(is_cb ? entry + (size_t)u * kUnit
                                                            : entry + B_CODEBOOK * B_PHONE_CH + B_HID + (size_t)(u - kCbUnits) * kUnit);
  float4* dst = reinterpret_cast<float4*>(is_cb ? cb_raw + (size_t)slot * B_CODEBOOK * B_PHONE_CH + (size_t)u * kUnit
                                                : kv_raw + (size_t)slot * B_KV_LEN * B_KV_CH + (size_t)(u - kCbUnits) * kUnit);
  float4 x[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) x[k] = src[t + kThreads * k];   // all of the unit's host reads in flight at once
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) dst[t + kThreads * k] = x[k];
  if (!is_cb) return;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int f = t + kThreads * k, r = f / (B_PHONE_CH / 4), c = (f % (B_PHONE_CH / 4)) * 4;
    float* p = tile + r * kPitch + c;
    p[0] = x[k].x; p[1] = x[k].y; p[2] = x[k].z; p[3] = x[k].w;
  }
  __syncthreads();
  const int j0 = u * kRows, lane = t & 63, wave = t >> 6;
  float* dstT = cbT + (size_t)slot * B_PHONE_CH * B_CODEBOOK + j0 + lane;
  for (int c = wave; c < B_PHONE_CH; c += kThreads / 64) dstT[(size_t)c * B_CODEBOOK] = tile[lane * kPitch + c];
  if (t < kRows) {   // codebook_prep_kernel's chain, so its bits: one fma per channel, ascending, from 0
    float a = 0.0f;
    for (int c = 0; c < B_PHONE_CH; ++c) {
      const float v = tile[t * kPitch + c];
      a = bsp::fma(v, v, a);
    }
    cnorm[(size_t)slot * B_CODEBOOK + j0 + t] = a;
  }
}

}  // namespace

bool install_entries(const MorphDesc* descs, const float* staged, int n, int n_entries, float* d_cb_raw, float* d_add_raw, float* d_kv_raw,
                     float* d_cbT, float* d_cnorm, hipStream_t stream) {
  if (n < 1) return false;
  hipLaunchKernelGGL(install_entries_kernel, dim3(n * kUnits), dim3(kThreads), 0, stream, descs, staged, n, n_entries, d_cb_raw, d_add_raw,
                     d_kv_raw, d_cbT, d_cnorm);
  return hip_ok(hipGetLastError(), "install entries launch");
}

}  // namespace bhip
