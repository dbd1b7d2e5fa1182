// Adjoint sensitivities of the P1 solve of -(a u')' + b u' + c u = f.  For a functional J(u)
// with p = dJ/du, the adjoint z solves the transposed bands (sub and sup exchanged) with load p, zero end data and the
// primal's end kinds and kappa; the existing tridiagonal solves do that.  This file adds the pass after it: from nc
// pairs (U[j], Z[j]) the gradients of J with respect to every entry of the tables a_quad, b_quad, c_quad, rhs_quad
//   dJ/da_eq = -(w_q / h_e) dz_e du_e      dJ/db_eq = -w_q z_eq du_e
//   dJ/dc_eq = -h_e w_q z_eq u_eq          dJ/df_eq = +h_e w_q z_eq
// and with respect to the end data (lssvr_sens.hpp).  The inputs are x, U, Z and the quadrature rule; none of the four
// tables is read, because given u and z the gradient does not depend on them.
// One thread per TABLE ENTRY idx = e nquad + q, in memory order, with an inner loop over the cases: every store of a
// wave is 64 consecutive doubles, whatever nquad is (a thread per element would store with a stride of nquad doubles).
// The nquad lanes of one element read the same x, U and Z entries, which the memory pipeline serves from one line.
// One pass with no reduction, no atomics, no LDS and no scratch; the end gradients, 4 nc values, are written by the
// first thread of the same launch.  FP64, -ffp-contract=off.
#include "lssvr_sens.hpp"
#include "lssvr_p1.hpp"

namespace lssvr {

namespace {

__global__ __launch_bounds__(kBlock) void p1_sensitivity_kernel(SensArgs a, QuadRule q) {
  const int64_t tab = a.ne * (int64_t)a.nquad, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < tab; idx += stride) sens_entry(a, q, idx);
  if (a.out_ends && blockIdx.x == 0 && threadIdx.x == 0)
    for (int j = 0; j < a.nc; ++j) sens_ends(a, j);
}

}  // namespace

hipError_t p1_sensitivity(const SensArgs& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(p1_sensitivity_kernel, dim3((unsigned)sens_blocks(a.ne * (int64_t)a.nquad)), dim3(kBlock), 0, s,
                     a, q);
  return hipGetLastError();
}

bool p1_sensitivity_host(const SensArgs& a) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return false;
  const int64_t tab = a.ne * (int64_t)a.nquad;
  for (int64_t idx = 0; idx < tab; ++idx) sens_entry(a, q, idx);
  if (a.out_ends)
    for (int j = 0; j < a.nc; ++j) sens_ends(a, j);
  return true;
}

}  // namespace lssvr
