// Adjoint sensitivities of the BDF loop of  rho u_t - (a u')' + c u = f(x, t)  (DESIGN.md section 32).  The backward
// sweep is made of the forward loop's own calls -- lssvr_ts_rhs with U0 = lambda^{n+1}, U1 = lambda^{n+2}, the row p_n as
// the load and phi = 1, then lssvr_tridiag_bc_solve_multi on the bands the forward loop assembled, with zero end data --
// and this file adds the pass that turns the adjoint states into gradients, summed over time:
//   dJ/da_eq   = -sum_n (w_q / h_e) dlambda^n_e du^n_e      dJ/dc_eq     = -sum_n h_e w_q lambda^n_eq u^n_eq
//   dJ/drho_eq = -sum_n h_e w_q lambda^n_eq w^n_eq          dJ/df_{r,eq} = +sum_n phi_r(t_n) h_e w_q lambda^n_eq
// (w^n: the nodal BDF difference) and the end gradients dJ/dg(t_n), dJ/dkappa (lssvr_ts_sens.hpp).
// ONE launch takes a chunk of m <= 8 consecutive steps: one thread per TABLE ENTRY, as in sensitivity.hip and for its
// reason (every store of a wave is 64 consecutive doubles whatever nquad is), an inner loop over the chunk's steps with
// the 3 + R sums in registers, one store per table.  A launch per step into per-step tables and a sum over time would
// move N times the table bytes; here a table is written once per chunk, and the mesh, the rule and two of the three
// trajectory rows of a step are reused from the step before.  No reduction, no atomics, no LDS, no scratch; the end
// gradients, 2 m + 2 values, are written by the first thread of the same launch.  FP64, -ffp-contract=off.
#include "lssvr_ts_sens.hpp"
#include "lssvr_p1.hpp"

namespace lssvr {

namespace {

__global__ __launch_bounds__(kBlock) void ts_sensitivity_kernel(TsSensArgs a, QuadRule q) {
  if (a.ga || a.gc || a.grho || a.gf) {
    const int64_t tab = a.ne * (int64_t)a.nquad, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < tab; idx += stride) ts_sens_entry(a, q, idx);
  }
  if (a.out_g && blockIdx.x == 0 && threadIdx.x == 0) ts_sens_ends(a);
}

}  // namespace

hipError_t ts_sensitivity(const TsSensArgs& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return hipErrorInvalidValue;
  const bool tables = a.ga || a.gc || a.grho || a.gf;
  hipLaunchKernelGGL(ts_sensitivity_kernel, dim3((unsigned)(tables ? sens_blocks(a.ne * (int64_t)a.nquad) : 1)),
                     dim3(kBlock), 0, s, a, q);
  return hipGetLastError();
}

bool ts_sensitivity_host(const TsSensArgs& a) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return false;
  const int64_t tab = a.ne * (int64_t)a.nquad;
  if (a.ga || a.gc || a.grho || a.gf)
    for (int64_t idx = 0; idx < tab; ++idx) ts_sens_entry(a, q, idx);
  if (a.out_g) ts_sens_ends(a);
  return true;
}

}  // namespace lssvr
