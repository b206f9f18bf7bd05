// morph.hip -- speaker morphing on the device: the weighted spherical means that turn the embeddings
// of up to eight real speakers into one synthetic speaker.
//
// What it replaces: the morph branch of the reference host (reference src/common/processor_core_2.cc:
// 124-172), which runs SphericalAverage<float, M> (reference src/common/spherical_average.h:80-444) on
// the audio thread -- one solve for the additive embedding (M = 256) and 384 solves for the key/value
// tokens (M = 128), spread over four hops because they cost ~1.6 ms each hop on a CPU.  The solves are
// independent, so here each one is ONE wavefront: the M dimensions live across the 64 lanes, every dot
// product is a lane-partial followed by an xor-butterfly wave sum, and all 385 run in one launch.
//
// Same algorithm, same constants, same quirks as host/spherical_mean.h (which is bit-exact to the
// reference): start from the normalised weighted mean, at most four Buss-Fillmore steps preconditioned
// by a two-slot L-BFGS memory, result = combination of the un-normalised points.  Not the same rounding:
// the host sums dot products sequentially and uses glibc's acos/sin, the device sums across lanes and
// uses the ROCm device library, so results agree to float rounding (tests: <= 2e-6 relative), not bit
// for bit.  Nothing downstream of these embeddings takes a discrete decision, so PCM stays within 1e-4.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "spec_math.hip.h"

namespace bhip {

namespace {

constexpr int kMaxPoints = 8;  // reference processor_core_2.h:26 (kSphAvgMaxNSpeakers)
constexpr int kMaxSteps = 4;   // reference processor_core_2.h:137 (kSphAvgMaxNUpdates)

struct SphMeanArgs {
  const float* table;   // [speaker][rows][dim] raw embeddings
  float* out;           // [rows][dim] of the destination speaker
  size_t speaker_stride;
  int n_active;
  int speaker[kMaxPoints];
  float weight[kMaxPoints];  // already normalised to sum 1, descending
};

// DPL = dimensions per lane (dim = 64 * DPL); lane owns dimensions lane + 64 * i.  One solve = one wavefront; mem_s / mem_t are the
// wavefront's own LDS (no barrier anywhere: a wavefront's LDS accesses complete in order)
template <int DPL>
__device__ __forceinline__ void sph_mean_solve(const SphMeanArgs& a, const int row, const int lane, float (&mem_s)[2][64 * DPL],
                                               float (&mem_t)[2][64 * DPL]) {
  constexpr int DIM = 64 * DPL;
  const int N = a.n_active;
  const float eps = 1.1920928955078125e-07f;  // FLT_EPSILON

  auto dot = [&](const float* x, const float* y) {
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) p = p + x[i] * y[i];
    return bsp::wsum64(p);
  };
  auto normalize = [&](float* x) -> bool {
    const float norm = sqrtf(dot(x, x));
    if (!(norm > 0.0f)) return false;
    const float inv = 1.0f / norm;
#pragma unroll
    for (int i = 0; i < DPL; ++i) x[i] = x[i] * inv;
    return true;
  };
  // sin(x)/x as the reference evaluates it: the magnitude is truncated to an integer before the
  // small-angle tests (unqualified abs() on a float, see host/spherical_mean.h), so 1 for |x| < 1
  auto sinc = [&](float x) -> float {
    const int ax = abs(static_cast<int>(x));
    return ax >= 1 ? static_cast<float>(sin(static_cast<double>(x)) / static_cast<double>(x)) : 1.0f;
  };

  float raw[kMaxPoints][DPL], unit[kMaxPoints][DPL], coef[kMaxPoints];
#pragma unroll
  for (int n = 0; n < kMaxPoints; ++n) {
    coef[n] = 0.0f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      raw[n][i] = n < N ? a.table[(size_t)a.speaker[n] * a.speaker_stride + (size_t)row * DIM + lane + 64 * i] : 0.0f;
      unit[n][i] = raw[n][i];
    }
    if (n < N) normalize(unit[n]);
  }

  float q[DPL], g[DPL], d[DPL];
  // L-BFGS memory: two (step, gradient change) pairs, selected by a run-time slot -> kept in LDS (mem_s, mem_t)
  float rho[2] = {0.0f, 0.0f}, alpha[2] = {0.0f, 0.0f};
  int slot = 0;
  float gamma = 1.0f;
#pragma unroll
  for (int i = 0; i < DPL; ++i) {
    q[i] = 0.0f; g[i] = 0.0f; d[i] = 0.0f;
    mem_s[0][lane + 64 * i] = 0.0f; mem_s[1][lane + 64 * i] = 0.0f;
    mem_t[0][lane + 64 * i] = 0.0f; mem_t[1][lane + 64 * i] = 0.0f;
  }

  // coefficients, tangent gradient and preconditioned direction at the current q
  auto gradient = [&]() {
    float denom = 0.0f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) g[i] = 0.0f;
#pragma unroll
    for (int n = 0; n < kMaxPoints; ++n) {
      if (n >= N) continue;
      float c = dot(unit[n], q);
      c = c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c);
      const float theta = static_cast<float>(acos(static_cast<double>(c)));
      const float inv_sinc = 1.0f / (sinc(theta) + eps);
      denom = denom + a.weight[n] * c * inv_sinc;
      coef[n] = a.weight[n] * inv_sinc;
      const float k = -2.0f * coef[n];
#pragma unroll
      for (int i = 0; i < DPL; ++i) g[i] = g[i] + k * unit[n][i];
    }
    const float inv_denom = 1.0f / (denom + eps);
#pragma unroll
    for (int n = 0; n < kMaxPoints; ++n) coef[n] = coef[n] * inv_denom;
    {  // project g onto the tangent space at q
      const float k = -dot(q, g);
#pragma unroll
      for (int i = 0; i < DPL; ++i) g[i] = g[i] + k * q[i];
    }
#pragma unroll
    for (int i = 0; i < DPL; ++i) d[i] = g[i];
    for (int k = 0; k < 2; ++k) {  // two-loop recursion, newest pair first
      const int m = (slot - k - 1 + 2) % 2;
      float sv[DPL], tv[DPL];
#pragma unroll
      for (int i = 0; i < DPL; ++i) { sv[i] = mem_s[m][lane + 64 * i]; tv[i] = mem_t[m][lane + 64 * i]; }
      const float al = rho[m] * dot(sv, d);
      if (m == 0) alpha[0] = al; else alpha[1] = al;
#pragma unroll
      for (int i = 0; i < DPL; ++i) d[i] = d[i] + (-al) * tv[i];
    }
#pragma unroll
    for (int i = 0; i < DPL; ++i) d[i] = d[i] * gamma;
    for (int k = 0; k < 2; ++k) {
      const int m = (slot + k) % 2;
      float sv[DPL], tv[DPL];
#pragma unroll
      for (int i = 0; i < DPL; ++i) { sv[i] = mem_s[m][lane + 64 * i]; tv[i] = mem_t[m][lane + 64 * i]; }
      const float beta = rho[m] * dot(tv, d);
      const float al = m == 0 ? alpha[0] : alpha[1];
#pragma unroll
      for (int i = 0; i < DPL; ++i) d[i] = d[i] + (al - beta) * sv[i];
    }
  };

  bool started = false;
  if (N > 0) {
#pragma unroll
    for (int n = 0; n < kMaxPoints; ++n) {
      if (n >= N) continue;
#pragma unroll
      for (int i = 0; i < DPL; ++i) q[i] = n == 0 ? a.weight[0] * unit[0][i] : q[i] + a.weight[n] * unit[n][i];
    }
    started = normalize(q);
  }
  if (started) {
    gradient();
    for (int it = 0; it < kMaxSteps; ++it) {
      const float step = sqrtf(dot(d, d));
      if (!(step >= 8.0f * eps)) break;  // converged
      float sv[DPL], tv[DPL];
#pragma unroll
      for (int i = 0; i < DPL; ++i) { sv[i] = q[i]; q[i] = q[i] - d[i]; }
      normalize(q);
#pragma unroll
      for (int i = 0; i < DPL; ++i) { sv[i] = q[i] - sv[i]; tv[i] = g[i]; }
      // as on the host, the recursion inside this gradient() already sees the slot being replaced
      // with its NEW step and with the OLD GRADIENT parked where the gradient change will go
#pragma unroll
      for (int i = 0; i < DPL; ++i) { mem_s[slot][lane + 64 * i] = sv[i]; mem_t[slot][lane + 64 * i] = tv[i]; }
      gradient();
#pragma unroll
      for (int i = 0; i < DPL; ++i) tv[i] = g[i] - tv[i];
      {
        const float k = -dot(q, tv);
#pragma unroll
        for (int i = 0; i < DPL; ++i) tv[i] = tv[i] + k * q[i];
      }
#pragma unroll
      for (int i = 0; i < DPL; ++i) mem_t[slot][lane + 64 * i] = tv[i];
      gamma = dot(sv, tv);
      const float r = 1.0f / gamma;
      if (slot == 0) rho[0] = r; else rho[1] = r;
      gamma = gamma / dot(tv, tv);
      slot = (slot + 1) % 2;
    }
  }
  // un-normalised combination of the ORIGINAL points with the final coefficients (zeros when the
  // weighted mean degenerated, like the host)
  float* o = a.out + (size_t)row * DIM;
#pragma unroll
  for (int i = 0; i < DPL; ++i) {
    float y = coef[0] * raw[0][i];
#pragma unroll
    for (int n = 1; n < kMaxPoints; ++n) if (n < N) y = y + coef[n] * raw[n][i];
    o[lane + 64 * i] = started ? y : 0.0f;
  }
}

template <int DPL>
__global__ __launch_bounds__(64) void sph_mean_kernel(const SphMeanArgs a) {
  __shared__ float mem_s[2][64 * DPL], mem_t[2][64 * DPL];
  sph_mean_solve<DPL>(a, blockIdx.x, threadIdx.x, mem_s, mem_t);
}

// ---- many entries in one call (BeatriceBatch_MorphSpeakersInFlight) ---------------------------------------------------------------
// The same solves for n entries in ONE launch: solve i * 385 + r is entry i's additive row (r = 0, 256 dimensions) or its key/value
// token r - 1 (128 dimensions), still one wavefront each with sph_mean_solve's arithmetic, kWaves of them to a workgroup.  What to
// solve is read from the descriptors (pinned host memory the caller wrote ahead of the device), not passed by value.
constexpr int kSolvesPerEntry = 1 + B_KV_LEN;
constexpr int kWaves = 4;

__device__ __forceinline__ bool desc_ok(const MorphDesc& d, const int n_entries) {
  bool ok = d.slot >= 0 && d.slot < n_entries && d.n_active >= 0 && d.n_active <= kMaxPoints;
#pragma unroll
  for (int n = 0; n < kMaxPoints; ++n) ok = ok && (n >= d.n_active || (d.speaker[n] >= 0 && d.speaker[n] < n_entries));
  return ok;
}

__global__ __launch_bounds__(64 * kWaves) void sph_mean_batched_kernel(const MorphDesc* __restrict__ descs, const int n, const int n_entries,
                                                                       float* add_raw, float* kv_raw) {
  __shared__ float mem[kWaves][2][2][B_HID];   // [wave][s | t][pair][dimension]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int solve = blockIdx.x * kWaves + wave;
  if (solve >= n * kSolvesPerEntry) return;
  const MorphDesc d = descs[solve / kSolvesPerEntry];
  if (!desc_ok(d, n_entries)) return;
  const int r = solve % kSolvesPerEntry;
  SphMeanArgs a{};
  a.n_active = d.n_active;
#pragma unroll
  for (int i = 0; i < kMaxPoints; ++i) { a.speaker[i] = d.speaker[i]; a.weight[i] = d.weight[i]; }
  if (r == 0) {
    a.table = add_raw; a.speaker_stride = B_HID; a.out = add_raw + (size_t)d.slot * B_HID;
    sph_mean_solve<4>(a, 0, lane, mem[wave][0], mem[wave][1]);
  } else {
    a.table = kv_raw; a.speaker_stride = (size_t)B_KV_LEN * B_KV_CH; a.out = kv_raw + (size_t)d.slot * B_KV_LEN * B_KV_CH;
    sph_mean_solve<2>(a, r - 1, lane, *reinterpret_cast<float(*)[2][B_KV_CH]>(&mem[wave][0][0][0]),
                      *reinterpret_cast<float(*)[2][B_KV_CH]>(&mem[wave][1][0][0]));
  }
}

// The projections of those entries, all four blocks, in one launch.  kv_project_kernel takes one workgroup per (token, entry) and
// reads both 128 x 256 weight matrices for every token; here a workgroup owns kTile tokens of one (entry, block, K or V): thread c
// walks column c of the matrix once, each weight held in a register for all kTile tokens, whose rows are staged in LDS (read as
// broadcasts) and whose chains live in registers.  Every output is still the single fma chain over e = 0 .. 127 ascending with the
// bias added last -- the same bits, 1 / kTile of the weight traffic.  Behind
// the key/value workgroups: the additive rows, kAddTile entries to a workgroup, with dense_rows_kernel's chain.
constexpr int kTile = 32, kTiles = B_KV_LEN / kTile, kAddTile = 16;
static_assert(B_KV_LEN % kTile == 0 && kTile % 4 == 0 && B_KV_CH % 4 == 0, "token tiles");

__global__ __launch_bounds__(256) void morph_project_kernel(const MorphProjectArgs a) {
  __shared__ __attribute__((aligned(16))) float rows[kAddTile * B_HID];   // (>= kTile * B_KV_CH)
  static_assert(kAddTile * B_HID >= kTile * B_KV_CH, "LDS tile");
  const int c = threadIdx.x;
  const int n_kv = a.n * B_NBLOCKS * 2 * kTiles;
  if ((int)blockIdx.x >= n_kv) {   // ---- additive rows of entries e0 .. e0 + kAddTile - 1 of the list
    const int e0 = ((int)blockIdx.x - n_kv) * kAddTile;
    int slot[kAddTile];
#pragma unroll
    for (int r = 0; r < kAddTile; ++r) {
      const int s = e0 + r < a.n ? a.descs[e0 + r].slot : -1;
      slot[r] = s >= 0 && s < a.n_entries ? s : -1;
      rows[r * B_HID + c] = slot[r] >= 0 ? a.add_raw[(size_t)slot[r] * B_HID + c] : 0.0f;
    }
    __syncthreads();
    float acc[kAddTile];
#pragma unroll
    for (int r = 0; r < kAddTile; ++r) acc[r] = 0.0f;
#pragma unroll 8
    for (int k = 0; k < B_HID; ++k) {
      const float w = a.add_w[(size_t)k * B_HID + c];
#pragma unroll
      for (int r = 0; r < kAddTile; ++r) acc[r] = bsp::fma(rows[r * B_HID + k], w, acc[r]);
    }
    const float bias = a.add_b[c];
#pragma unroll
    for (int r = 0; r < kAddTile; ++r) if (slot[r] >= 0) a.add_tab[(size_t)slot[r] * B_HID + c] = acc[r] + bias;
    return;
  }
  // ---- key/value tokens j0 .. j0 + kTile - 1 of (entry, block), K^T (is_v = 0) or V
  int g = blockIdx.x;
  const int tile = g % kTiles; g /= kTiles;
  const int is_v = g & 1; g >>= 1;
  const int blk = g % B_NBLOCKS, slot = a.descs[g / B_NBLOCKS].slot;
  if (slot < 0 || slot >= a.n_entries) return;
  const int j0 = tile * kTile;
  {  // the tile TRANSPOSED, [e][token]: one 16-byte broadcast read then gives four tokens' values at one e
    const float4* src = reinterpret_cast<const float4*>(a.kv_raw + ((size_t)slot * B_KV_LEN + j0) * B_KV_CH);
    for (int i = c; i < kTile * B_KV_CH / 4; i += 256) {
      const float4 x = src[i];
      const int t = i / (B_KV_CH / 4), e = (i % (B_KV_CH / 4)) * 4;
      rows[(e + 0) * kTile + t] = x.x; rows[(e + 1) * kTile + t] = x.y; rows[(e + 2) * kTile + t] = x.z; rows[(e + 3) * kTile + t] = x.w;
    }
  }
  const float* __restrict__ wm = (is_v ? a.v_w[blk] : a.k_w[blk]) + c;
  const float bias = is_v ? a.v_b[blk][c] : a.k_b[blk][c];
  __syncthreads();
  // kTile independent chains, as pairs (v_pk_fma_f32: the bits of v_fma_f32); weight e of the column is loaded once and serves them all
  bsp::f32x2 acc[kTile / 2];
#pragma unroll
  for (int q = 0; q < kTile / 2; ++q) acc[q] = bsp::splat2(0.0f);
#pragma unroll 4
  for (int e = 0; e < B_KV_CH; ++e) {
    const bsp::f32x2 w = bsp::splat2(wm[e * B_HID]);
#pragma unroll
    for (int q = 0; q < kTile / 4; ++q) {
      const float4 x = *reinterpret_cast<const float4*>(rows + e * kTile + 4 * q);
      acc[2 * q] = bsp::fma2(bsp::f32x2{x.x, x.y}, w, acc[2 * q]);
      acc[2 * q + 1] = bsp::fma2(bsp::f32x2{x.z, x.w}, w, acc[2 * q + 1]);
    }
  }
  // the layouts kv_project_kernel writes: MFMA B-fragment order (K^T: k = channel, n = token; V: k = token, n = channel), and
  // plain order (K^T [channel][token], V [token][channel]) when the batch holds those copies
  float* packed = (is_v ? a.v[blk] : a.kt[blk]) + (size_t)slot * B_HID * B_KV_LEN;
  float* plain = is_v ? a.v_plain[blk] : a.kt_plain[blk];
  if (plain) plain += (size_t)slot * B_HID * B_KV_LEN;
#pragma unroll
  for (int q = 0; q < kTile / 4; ++q) {
    const int j = j0 + 4 * q;
    const float y[4] = {acc[2 * q][0] + bias, acc[2 * q][1] + bias, acc[2 * q + 1][0] + bias, acc[2 * q + 1][1] + bias};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (is_v) {
        packed[packed_w_offset_dev(B_KV_LEN, j + i, c)] = y[i];
        if (plain) plain[(size_t)(j + i) * B_HID + c] = y[i];
      } else {
        packed[packed_w_offset_dev(B_HID, c, j + i)] = y[i];
      }
    }
    if (!is_v && plain) *reinterpret_cast<float4*>(plain + (size_t)c * B_KV_LEN + j) = make_float4(y[0], y[1], y[2], y[3]);
  }
}

}  // namespace

bool spherical_mean_entries(const MorphDesc* descs, int n, int n_entries, float* d_add_raw, float* d_kv_raw, hipStream_t stream) {
  if (n < 1) return false;
  hipLaunchKernelGGL(sph_mean_batched_kernel, dim3((n * kSolvesPerEntry + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream, descs, n, n_entries,
                     d_add_raw, d_kv_raw);
  return hip_ok(hipGetLastError(), "batched spherical mean launch");
}

bool morph_project_entries(const MorphProjectArgs& a, hipStream_t stream) {
  if (a.n < 1) return false;
  const int grid = a.n * B_NBLOCKS * 2 * kTiles + (a.n + kAddTile - 1) / kAddTile;
  hipLaunchKernelGGL(morph_project_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hip_ok(hipGetLastError(), "batched morph projection launch");
}

// rows x dim spherical means: out[row] = mean over points table[speaker[n]][row] with weights w[n]
bool spherical_mean_rows(const float* d_table, size_t speaker_stride, int rows, int dim, int n_active, const int* speakers,
                         const float* weights, float* d_out, hipStream_t stream) {
  if (n_active < 0 || n_active > kMaxPoints || (dim != 128 && dim != 256)) return false;
  SphMeanArgs a{};
  a.table = d_table; a.out = d_out; a.speaker_stride = speaker_stride; a.n_active = n_active;
  for (int n = 0; n < n_active; ++n) { a.speaker[n] = speakers[n]; a.weight[n] = weights[n]; }
  if (dim == 128) hipLaunchKernelGGL(sph_mean_kernel<2>, dim3(rows), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(sph_mean_kernel<4>, dim3(rows), dim3(64), 0, stream, a);
  return hip_ok(hipGetLastError(), "spherical mean launch");
}

}  // namespace bhip
