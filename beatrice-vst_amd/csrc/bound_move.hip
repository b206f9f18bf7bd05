// bound_move.hip -- a bound stream's wrapper state from one binding with clocks per stream into another, or into wrapper blobs and back
// (BeatriceBatch_MoveBoundStreamsInFlight / ExportBoundStreamsInFlight / ImportBoundStreamsInFlight, batch_wrappers.hip.h; what is
// moved, where it goes and the bounds of every index: bound_move_plan.h).
//
// One workgroup per stream, rounds of up to 16 as stream_blob.hip's.  A stream's wrapn::StreamState is 1060 words (two filter histories
// per direction, then the 480 places of the FIFO: 16-byte units, rows 16-byte aligned), the hop it carries 240 words in its cell of a
// resident output slot.
//   move:    the state row as it is (the bound form: places [fill, 480) of the FIFO are stale input nobody reads), the carried hop from
//            the cell the source's slot map names into the destination's cell, the destination's slot-map entry.
//   gather:  the state into the blob with the FIFO in the in-order form: the stream's own places below fill, the zero-stuffed hop from
//            fill on (bmove::fifo_place).
//   scatter: the blob's state row as it is, the hop's samples back out of the even places at or above fill (bmove::hop_place), the
//            slot-map entry.
// A slot-map value is device data: a source entry outside [0, io_slots) reads no memory, the hop then counts as zeros.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "wrapper_blob.h"

namespace bhip {

namespace {

constexpr int kThreads = 256;
constexpr int kStateWords = (int)(wblob::kStateBytes / sizeof(float));
constexpr int kFifoAt = kStateWords - bmove::kFifo;   // the FIFO is the state's last member (batch_wrappers.hip.h holds the offset equal)
static_assert(kStateWords % 4 == 0 && kFifoAt % 4 == 0 && bmove::kHop % 4 == 0, "16-byte units");

// the source stream's carried hop: nullptr when none has fired, or when the map names no slot of the side
__device__ __forceinline__ const float* carried_hop(const BoundSide& s, const bmove::Item& it) {
  if (!it.has_hop) return nullptr;
  const int slot = s.slot_map[(size_t)it.stream * s.map_ring + it.entry];
  if (slot < 0 || slot >= s.io_slots) return nullptr;
  return s.out24 + ((size_t)slot * s.B + it.stream) * bmove::kHop;
}
__device__ __forceinline__ float* dest_cell(const BoundSide& d, const bmove::Item& it) {
  return d.out24 + ((size_t)it.slot * d.B + it.stream) * bmove::kHop;
}

__global__ __launch_bounds__(kThreads) void bound_move_kernel(const BoundSide src, const BoundSide dst, const BoundRound round) {
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= round.n) return;
  const bmove::Item from = round.src[j], to = round.dst[j];
  const uint4* s4 = reinterpret_cast<const uint4*>(src.st + (size_t)from.stream * kStateWords);
  uint4* d4 = reinterpret_cast<uint4*>(dst.st + (size_t)to.stream * kStateWords);
  for (int i = tid; i < kStateWords / 4; i += kThreads) d4[i] = s4[i];
  const float* hop = carried_hop(src, from);
  uint4* c4 = reinterpret_cast<uint4*>(dest_cell(dst, to));
  for (int i = tid; i < bmove::kHop / 4; i += kThreads) c4[i] = hop ? reinterpret_cast<const uint4*>(hop)[i] : uint4{0u, 0u, 0u, 0u};
  if (tid == 0) dst.slot_map[(size_t)to.stream * dst.map_ring + to.entry] = to.slot;
}

__global__ __launch_bounds__(kThreads) void bound_gather_kernel(const BoundSide src, const BoundRound round, float* __restrict__ staging,
                                                                const size_t blob_floats, const size_t state_off) {
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= round.n) return;
  const bmove::Item from = round.src[j];
  const float* st = src.st + (size_t)from.stream * kStateWords;
  float* out = staging + (size_t)j * blob_floats + state_off;
  const uint4* s4 = reinterpret_cast<const uint4*>(st);
  uint4* o4 = reinterpret_cast<uint4*>(out);
  for (int i = tid; i < kFifoAt / 4; i += kThreads) o4[i] = s4[i];   // (the four histories)
  const float* hop = carried_hop(src, from);
  for (int i = tid; i < bmove::kFifo; i += kThreads) out[kFifoAt + i] = bmove::fifo_place(i, from.fill, st + kFifoAt, hop);
}

__global__ __launch_bounds__(kThreads) void bound_scatter_kernel(const BoundSide dst, const BoundRound round, const float* __restrict__ staging,
                                                                 const size_t blob_floats, const size_t state_off) {
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= round.n) return;
  const bmove::Item to = round.dst[j];
  const float* in = staging + (size_t)j * blob_floats + state_off;
  const uint4* i4 = reinterpret_cast<const uint4*>(in);
  uint4* d4 = reinterpret_cast<uint4*>(dst.st + (size_t)to.stream * kStateWords);
  for (int i = tid; i < kStateWords / 4; i += kThreads) d4[i] = i4[i];
  float* cell = dest_cell(dst, to);
  for (int i = tid; i < bmove::kHop; i += kThreads) cell[i] = bmove::hop_place(i, to.fill, in + kFifoAt);
  if (tid == 0) dst.slot_map[(size_t)to.stream * dst.map_ring + to.entry] = to.slot;
}

bool side_ok(const BoundSide& s) { return s.st && s.out24 && s.slot_map && s.B >= 1 && s.io_slots >= 1 && s.map_ring >= 1; }
bool items_ok(const BoundSide& s, int n, const bmove::Item* items) {
  if (!side_ok(s) || n < 1 || n > 16) return false;
  const bmove::Geometry g{s.B, s.io_slots, s.map_ring};
  for (int j = 0; j < n; ++j) if (!bmove::item_ok(g, items[j])) return false;
  return true;
}
// (16-byte units: the staging buffer is the wrapper blobs', whose state sits at a multiple of 16 bytes in a blob that is one)
bool staging_ok(const void* p, size_t blob_floats, size_t state_off) {
  return p && blob_floats % 4 == 0 && state_off % 4 == 0 && state_off + kStateWords <= blob_floats && (reinterpret_cast<unsigned long long>(p) & 15ull) == 0;
}

}  // namespace

bool bound_move(const BoundSide& src, const BoundSide& dst, const BoundRound& round, hipStream_t stream) {
  if (!items_ok(src, round.n, round.src) || !items_ok(dst, round.n, round.dst)) return false;
  hipLaunchKernelGGL(bound_move_kernel, dim3(round.n), dim3(kThreads), 0, stream, src, dst, round);
  return hip_ok(hipGetLastError(), "bound move launch");
}
bool bound_gather(const BoundSide& src, const BoundRound& round, float* d_staging, size_t blob_floats, size_t state_off, hipStream_t stream) {
  if (!items_ok(src, round.n, round.src) || !staging_ok(d_staging, blob_floats, state_off)) return false;
  hipLaunchKernelGGL(bound_gather_kernel, dim3(round.n), dim3(kThreads), 0, stream, src, round, d_staging, blob_floats, state_off);
  return hip_ok(hipGetLastError(), "bound gather launch");
}
bool bound_scatter(const BoundSide& dst, const BoundRound& round, const float* d_staging, size_t blob_floats, size_t state_off, hipStream_t stream) {
  if (!items_ok(dst, round.n, round.dst) || !staging_ok(d_staging, blob_floats, state_off)) return false;
  hipLaunchKernelGGL(bound_scatter_kernel, dim3(round.n), dim3(kThreads), 0, stream, dst, round, d_staging, blob_floats, state_off);
  return hip_ok(hipGetLastError(), "bound scatter launch");
}

}  // namespace bhip
