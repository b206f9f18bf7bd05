// stream_blob.hip -- a stream's device state out of a batch into blobs and back (BeatriceBatch_ExportStreams / BeatriceBatch_ImportStreams,
// batch.hip; the blob's format and what is refused: stream_blob.h).
//
// Both directions are one launch per round of up to 16 streams over the batch's piece table (engine.h BlobPiece: every ring of the three
// arenas, the pitch head's previous bin, the 48 kHz wrapper's history), grid (pieces, streams of the round, kSplit).  The blobs sit in a
// device staging buffer in the blob's own layout, so the copy between it and pinned host memory is one plain transfer.
//   gather:  stream streams[j]'s m slots of a piece, in slot order, to the piece's place in blob j.
//   scatter: the way back, and the destination batch stands at another step counter than the source did: a ring of m > 1 slots is
//            indexed by counter % m, so slot i of the blob belongs in slot (i + shift) % m (ring_rotate_kernel's move, kernels_misc.hip.h).
//            Source and destination are different buffers, so the turn is folded into the destination index of a plain copy -- no
//            register array of up to 64 slots per lane as the in-place rotation needs.
//   move:    both at once between two batches on one device (BeatriceBatch_MoveStreamsInFlight): from the source batch's piece table
//            straight into the destination's, turned the same way; no staging buffer.
// 16-byte loads and stores wherever a piece's slot is a multiple of four words and both ends are aligned (every ring is: arenas pad rings
// to 64 words, blobs pad pieces to 4); the previous bin and the wrapper's history (286 words per stream) go word by word.
#include <hip/hip_runtime.h>

#include "engine.h"

namespace bhip {

namespace {

constexpr int kThreads = 256, kSplit = 4;   // (the largest ring of a stream is a few hundred KB: four workgroups of 16-byte lanes each)

__device__ __forceinline__ bool aligned16(const void* a, const void* b) {
  return ((reinterpret_cast<unsigned long long>(a) | reinterpret_cast<unsigned long long>(b)) & 15ull) == 0;
}

__global__ __launch_bounds__(kThreads) void stream_gather_kernel(const BlobPiece* __restrict__ pieces, const BlobRound round,
                                                                 float* __restrict__ staging, const size_t blob_floats) {
  const BlobPiece p = pieces[blockIdx.x];
  const int j = blockIdx.y;
  if (j >= round.n) return;
  const float* src = p.base + (size_t)round.streams[j] * p.stride;
  float* dst = staging + (size_t)j * blob_floats + p.blob_off;
  const unsigned n = p.slot_floats * (unsigned)p.m, first = blockIdx.z * kThreads + threadIdx.x, step = kThreads * kSplit;
  if ((p.slot_floats & 3u) == 0 && aligned16(src, dst)) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (unsigned i = first; i < n / 4; i += step) d4[i] = s4[i];
  } else {
    for (unsigned i = first; i < n; i += step) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(kThreads) void stream_scatter_kernel(const BlobPiece* __restrict__ pieces, const BlobRound round,
                                                                  const float* __restrict__ staging, const size_t blob_floats) {
  const BlobPiece p = pieces[blockIdx.x];
  const int j = blockIdx.y;
  if (j >= round.n) return;
  const float* src = staging + (size_t)j * blob_floats + p.blob_off;
  float* dst = p.base + (size_t)round.streams[j] * p.stride;
  const unsigned m = (unsigned)p.m, turn = m > 1 ? (unsigned)round.shift[j] % m : 0u;
  const unsigned n = p.slot_floats * m, first = blockIdx.z * kThreads + threadIdx.x, step = kThreads * kSplit;
  if ((p.slot_floats & 3u) == 0 && aligned16(src, dst)) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const unsigned per = p.slot_floats / 4;   // (a 16-byte unit never straddles two slots)
    for (unsigned i = first; i < n / 4; i += step) {
      const unsigned slot = i / per, e = i - slot * per;
      const unsigned to = slot + turn >= m ? slot + turn - m : slot + turn;
      d4[to * per + e] = s4[i];
    }
  } else {
    for (unsigned i = first; i < n; i += step) {
      const unsigned slot = i / p.slot_floats, e = i - slot * p.slot_floats;
      const unsigned to = slot + turn >= m ? slot + turn - m : slot + turn;
      dst[to * p.slot_floats + e] = src[i];
    }
  }
}

// Ring to ring between two batches on one device (BeatriceBatch_MoveStreamsInFlight): gather and scatter in one, no blob between.  The
// two piece tables are of one layout (the host holds sblob::same_layout before it launches), so piece i of both names the same ring with
// the same slot size and slot count; only base and per-stream stride are each batch's own.  The turn goes into the destination slot as
// above.
__global__ __launch_bounds__(kThreads) void stream_move_kernel(const BlobPiece* __restrict__ src_pieces, const BlobPiece* __restrict__ dst_pieces,
                                                               const MoveRound round) {
  const BlobPiece ps = src_pieces[blockIdx.x], pd = dst_pieces[blockIdx.x];
  const int j = blockIdx.y;
  if (j >= round.n) return;
  const float* src = ps.base + (size_t)round.src[j] * ps.stride;
  float* dst = pd.base + (size_t)round.dst[j] * pd.stride;
  const unsigned m = (unsigned)pd.m, turn = m > 1 ? (unsigned)round.shift[j] % m : 0u;
  const unsigned n = pd.slot_floats * m, first = blockIdx.z * kThreads + threadIdx.x, step = kThreads * kSplit;
  if ((pd.slot_floats & 3u) == 0 && aligned16(src, dst)) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const unsigned per = pd.slot_floats / 4;
    for (unsigned i = first; i < n / 4; i += step) {
      const unsigned slot = i / per, e = i - slot * per;
      const unsigned to = slot + turn >= m ? slot + turn - m : slot + turn;
      d4[to * per + e] = s4[i];
    }
  } else {   // (the previous bin, the 48 kHz wrapper's history)
    for (unsigned i = first; i < n; i += step) {
      const unsigned slot = i / pd.slot_floats, e = i - slot * pd.slot_floats;
      const unsigned to = slot + turn >= m ? slot + turn - m : slot + turn;
      dst[to * pd.slot_floats + e] = src[i];
    }
  }
}

bool round_ok(int n_pieces, const BlobRound& round) { return n_pieces >= 1 && round.n >= 1 && round.n <= 16; }

}  // namespace

bool stream_move(const BlobPiece* d_src_pieces, const BlobPiece* d_dst_pieces, int n_pieces, const MoveRound& round, hipStream_t stream) {
  if (n_pieces < 1 || round.n < 1 || round.n > 16) return false;
  hipLaunchKernelGGL(stream_move_kernel, dim3(n_pieces, round.n, kSplit), dim3(kThreads), 0, stream, d_src_pieces, d_dst_pieces, round);
  return hip_ok(hipGetLastError(), "stream move launch");
}

bool stream_gather(const BlobPiece* d_pieces, int n_pieces, const BlobRound& round, float* d_staging, size_t blob_floats, hipStream_t stream) {
  if (!round_ok(n_pieces, round)) return false;
  hipLaunchKernelGGL(stream_gather_kernel, dim3(n_pieces, round.n, kSplit), dim3(kThreads), 0, stream, d_pieces, round, d_staging, blob_floats);
  return hip_ok(hipGetLastError(), "stream gather launch");
}
bool stream_scatter(const BlobPiece* d_pieces, int n_pieces, const BlobRound& round, const float* d_staging, size_t blob_floats, hipStream_t stream) {
  if (!round_ok(n_pieces, round)) return false;
  hipLaunchKernelGGL(stream_scatter_kernel, dim3(n_pieces, round.n, kSplit), dim3(kThreads), 0, stream, d_pieces, round, d_staging, blob_floats);
  return hip_ok(hipGetLastError(), "stream scatter launch");
}

}  // namespace bhip
