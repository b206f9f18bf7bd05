// Every body of the tick launch as a kernel of its own under the launch's register budget (512 threads, two workgroups per CU):
// registers and spills per body (the table kernel reports only the maximum over all of them).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I beatrice-vst_amd/csrc -c tools/experiments/body_resources.hip -o /tmp/br.o
//   then tools/experiments/body_resources.sh
#include <hip/hip_runtime.h>
#include <type_traits>

#include "tick.hip.h"

template <class Op, int TAG>
__global__ __launch_bounds__(512, 4) void body_kernel(const typename Op::Args a) {
  __shared__ __attribute__((aligned(16))) float lds[Op::LDS_FLOATS > 0 ? Op::LDS_FLOATS : 1];
  if (threadIdx.x == 0) { stepc::pair[0] = 1; stepc::pair[1] = 0; }
  __syncthreads();
  if ((int)threadIdx.x < Op::NTHR) Op::template run_t<false>(a, blockIdx.x, blockIdx.y, lds);
}
#define INST(H, NAME) template __global__ void body_kernel<typename tick::Ops<H>::NAME, H>(const typename tick::Ops<H>::NAME::Args)
#define EACH(NAME) INST(1, NAME); INST(2, NAME); INST(4, NAME)
EACH(OpF2); EACH(OpF3); EACH(OpF4); EACH(OpF5); EACH(OpRB); EACH(OpOUT); EACH(OpP1); EACH(OpP23); EACH(OpPOUT); EACH(OpINP);
EACH(OpUP1); EACH(OpRES1A); EACH(OpRES1B); EACH(OpUP2); EACH(T1); EACH(T2); EACH(T3); EACH(GruQ); EACH(GruP); EACH(Vq);
INST(2, GruQ1); INST(2, GruP1); INST(4, GruQ1); INST(4, GruP1); INST(4, GruQm); INST(4, GruPm);   // the linked cells: last hop; middle hops
// the rows cell of the tick tables at the phone GRU's size in every link form (EACH(GruP) above holds its hop-0 form at two and four hops),
// and its other split, 16 streams x 128 hidden units
template __global__ void body_kernel<rc::GruRowsOp<256, 256, 1>, 0>(const GruArgs);
template __global__ void body_kernel<rc::GruRowsOp<256, 256, 0, 1>, 0>(const GruArgs); template __global__ void body_kernel<rc::GruRowsOp<128, 128, 0, 1>, 0>(const GruArgs);
// the sparse table's bodies (one hop per step only: tick::sparse_table_at)
INST(1, OpF4s); INST(1, OpF5s); INST(1, OpRBs); INST(1, OpP1s); INST(1, OpUP1s); INST(1, T1s); INST(1, T2s);
template __global__ void body_kernel<F1Op2, 0>(const F1Op2::Args);
template __global__ void body_kernel<FftOp2, 0>(const FftOp2::Args);
template __global__ void body_kernel<HeadOp8, 0>(const HeadOp8::Args);
template __global__ void body_kernel<CondOp2, 0>(const CondOp2::Args);
#define BLOCKS(H) \
  template __global__ void body_kernel<rc::BlockAOp<1, H>, 0>(const rc::BlockAArgs); template __global__ void body_kernel<rc::BlockAOp<2, H>, 0>(const rc::BlockAArgs); \
  template __global__ void body_kernel<rc::BlockAOp<4, H>, 0>(const rc::BlockAArgs); template __global__ void body_kernel<rc::BlockAOp<8, H>, 0>(const rc::BlockAArgs); \
  template __global__ void body_kernel<rc::BlockBOpH<H>, 0>(const rc::BlockBArgs); template __global__ void body_kernel<rc::BlockBqOpH<H>, 0>(const rc::BlockBqArgs)
BLOCKS(1); BLOCKS(2); BLOCKS(4);

// ... and the six table kernels themselves (the launch's own: fuse::table_kernel_w at the tick's register budget, common and ragged)
template <bool RAG, class... Ms>
const void* table_kernel_of(const fuse::Table<Ms...>*) { return reinterpret_cast<const void*>(&fuse::table_kernel_w<4, RAG, Ms...>); }
#define TABLES(H) template const void* table_kernel_of<false>(const tick::Ops<H>::Tab*); template const void* table_kernel_of<true>(const tick::Ops<H>::Tab*)
TABLES(1); TABLES(2); TABLES(4);
