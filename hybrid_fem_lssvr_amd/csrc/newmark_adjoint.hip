// Adjoint sensitivities of the Newmark loop of  rho u_tt + d u_t - (a u')' + c u = f(x, t)  (DESIGN.md section 34).  The
// backward sweep solves  A lambda^{n+1} = B_{n+1}  with lssvr_tridiag_bc_solve_multi on the forward loop's own bands
// (A is symmetric), the chunk pass of chunk_sens.hip turns its states into gradients, and this file adds what no other
// kernel does:
//   adjoint advance   ONE launch between two backward solves: the transposed Newmark recurrences, which turn
//                     lambda^{n+1} and the bars (vbar, abar) of level n+1 into the bars of level n and B_n, the next
//                     right-hand side (lssvr_newmark_adj.hpp: nm_adj_row).  One thread per node; lambda is an input, so
//                     unlike the forward advance nothing is recomputed and nothing needs a barrier.
// No reduction, no atomics, no LDS, no scratch; 256 threads, at most 1024 workgroups, grid-stride.
// FP64, -ffp-contract=off.
#include "lssvr_newmark_adj.hpp"

namespace lssvr {

namespace {

__global__ __launch_bounds__(kBlock) void newmark_adjoint_advance_kernel(NmAdjArgs a) {
  const int64_t n = a.ne + 1, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) nm_adj_row(a, i);
}

}  // namespace

hipError_t newmark_adjoint_advance(const NmAdjArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(newmark_adjoint_advance_kernel, dim3((unsigned)sens_blocks(a.ne + 1)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

void newmark_adjoint_advance_host(const NmAdjArgs& a) {
  for (int64_t i = 0; i <= a.ne; ++i) nm_adj_row(a, i);
}

}  // namespace lssvr
