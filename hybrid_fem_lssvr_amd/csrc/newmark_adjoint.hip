// Adjoint sensitivities of the Newmark loop of  rho u_tt + d u_t - (a u')' + c u = f(x, t)  (DESIGN.md section 34).  The
// backward sweep solves  A lambda^{n+1} = B_{n+1}  with lssvr_tridiag_bc_solve_multi on the forward loop's own bands
// (A is symmetric), and this file adds what no other kernel does:
//   adjoint advance   ONE launch between two backward solves: the transposed Newmark recurrences, which turn
//                     lambda^{n+1} and the bars (vbar, abar) of level n+1 into the bars of level n and B_n, the next
//                     right-hand side (lssvr_newmark_adj.hpp: nm_adj_row).  One thread per node; lambda is an input, so
//                     unlike the forward advance nothing is recomputed and nothing needs a barrier.
//   sensitivity       the pass that turns a chunk of m <= 8 consecutive levels into gradients, summed over time:
//     dJ/da_eq   = -sum_n (w_q / h_e) dlambda^n_e du^n_e      dJ/dc_eq     = -sum_n h_e w_q lambda^n_eq u^n_eq
//     dJ/drho_eq = -sum_n h_e w_q lambda^n_eq acc^n_eq        dJ/dd_eq     = -sum_n h_e w_q lambda^n_eq v^n_eq
//     dJ/df_{r,eq} = +sum_n phi_r(t_n) h_e w_q lambda^n_eq
//                     and the end gradients dJ/dg(t_n), dJ/dkappa.  One thread per TABLE ENTRY, as in timestep_sens.hip
//                     and for its reasons: every store of a wave is 64 consecutive doubles whatever nquad is, the 4 + R
//                     sums stay in registers over the chunk and each table is written once per chunk.
// No reduction, no atomics, no LDS, no scratch; 256 threads, at most 1024 workgroups, grid-stride.
// FP64, -ffp-contract=off.
#include "lssvr_newmark_adj.hpp"
#include "lssvr_p1.hpp"

namespace lssvr {

namespace {

__global__ __launch_bounds__(kBlock) void newmark_adjoint_advance_kernel(NmAdjArgs a) {
  const int64_t n = a.ne + 1, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) nm_adj_row(a, i);
}

__global__ __launch_bounds__(kBlock) void newmark_sensitivity_kernel(NmSensArgs a, QuadRule q) {
  if (a.ga || a.gc || a.grho || a.gd || a.gf) {
    const int64_t tab = a.ne * (int64_t)a.nquad, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < tab; idx += stride) nm_sens_entry(a, q, idx);
  }
  if (a.out_g && blockIdx.x == 0 && threadIdx.x == 0) nm_sens_ends(a);
}

}  // namespace

hipError_t newmark_adjoint_advance(const NmAdjArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(newmark_adjoint_advance_kernel, dim3((unsigned)sens_blocks(a.ne + 1)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

void newmark_adjoint_advance_host(const NmAdjArgs& a) {
  for (int64_t i = 0; i <= a.ne; ++i) nm_adj_row(a, i);
}

hipError_t newmark_sensitivity(const NmSensArgs& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return hipErrorInvalidValue;
  const bool tables = a.ga || a.gc || a.grho || a.gd || a.gf;
  hipLaunchKernelGGL(newmark_sensitivity_kernel, dim3((unsigned)(tables ? sens_blocks(a.ne * (int64_t)a.nquad) : 1)),
                     dim3(kBlock), 0, s, a, q);
  return hipGetLastError();
}

bool newmark_sensitivity_host(const NmSensArgs& a) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return false;
  const int64_t tab = a.ne * (int64_t)a.nquad;
  if (a.ga || a.gc || a.grho || a.gd || a.gf)
    for (int64_t idx = 0; idx < tab; ++idx) nm_sens_entry(a, q, idx);
  if (a.out_g) nm_sens_ends(a);
  return true;
}

}  // namespace lssvr
