// Adjoint sensitivities of the semilinear P1 solve of -(a u')' + b u' + c u + g(x, u) = f.  At
// the converged u* the adjoint z solves the TRANSPOSED Newton Jacobian K + M(g_u(., u*_h)) with load p = dJ/du -- the bands
// of one lssvr_p1_assemble with c_quad = c + g_u from one lssvr_nl_linearize, through the existing tridiagonal solves.
// This file adds the pass after it: the gradients with respect to the tables a, b, c, f and the end data, which are
// those of sensitivity.hip with u = u* (sens_entry and sens_ends, called unchanged: bit-equal to lssvr_p1_sensitivity),
// and with respect to every entry of the tables q_k of the reaction law,
//   POLY  dJ/dq_k,eq = -h_e w_q z_eq u_eq^k         EXP  dJ/dq_0,eq = -h_e w_q z_eq exp(q_1 u_eq)
//                                                        dJ/dq_1,eq = -h_e w_q z_eq q_0 u_eq exp(q_1 u_eq)
// (lssvr_nl_sens.hpp).  ONE launch in the shape of p1_sensitivity_kernel: one thread per TABLE ENTRY idx = e nquad + q,
// in memory order, with an inner loop over the cases, so every store of a wave is 64 consecutive doubles in each of the
// 4 + nterm tables; the grid-stride loop is capped by sens_blocks.  No reduction, no atomics, no LDS and no scratch; the
// end gradients are written by the first thread of the same launch.  FP64, -ffp-contract=off.
#include "lssvr_nl_sens.hpp"
#include "lssvr_p1.hpp"

namespace lssvr {

namespace {

// (the tables of sens_entry first, then gq: a.s with four nullptr tables costs neither loads nor arithmetic)
LSSVR_SENS_HD void nl_sens_at(const NlSensArgs& a, const QuadRule& q, int64_t idx) {
  if (a.s.ga || a.s.gb || a.s.gc || a.s.gf) sens_entry(a.s, q, idx);
  if (a.gq) nl_sens_entry(a, q, idx);
}

__global__ __launch_bounds__(kBlock) void nl_sensitivity_kernel(NlSensArgs a, QuadRule q) {
  const int64_t tab = a.s.ne * (int64_t)a.s.nquad, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < tab; idx += stride) nl_sens_at(a, q, idx);
  if (a.s.out_ends && blockIdx.x == 0 && threadIdx.x == 0)
    for (int j = 0; j < a.s.nc; ++j) sens_ends(a.s, j);
}

}  // namespace

hipError_t nl_sensitivity(const NlSensArgs& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.s.nquad, q)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nl_sensitivity_kernel, dim3((unsigned)sens_blocks(a.s.ne * (int64_t)a.s.nquad)), dim3(kBlock), 0,
                     s, a, q);
  return hipGetLastError();
}

bool nl_sensitivity_host(const NlSensArgs& a) {
  QuadRule q;
  if (!quad_rule(a.s.nquad, q)) return false;
  const int64_t tab = a.s.ne * (int64_t)a.s.nquad;
  for (int64_t idx = 0; idx < tab; ++idx) nl_sens_at(a, q, idx);
  if (a.s.out_ends)
    for (int j = 0; j < a.s.nc; ++j) sens_ends(a.s, j);
  return true;
}

}  // namespace lssvr
