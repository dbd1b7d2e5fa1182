// The chunk pass of the time-loop adjoint sensitivities: it turns the adjoint states of m <= 8 consecutive levels of a
// backward sweep into gradients, summed over time.  Written once and instantiated for the three loops
// (lssvr_chunk_sens.hpp says what each supplies):
//   BDF loop of  rho u_t - (a u')' + c u = f(x, t)  (DESIGN.md section 32).  The backward sweep is made of the forward
//     loop's own calls -- lssvr_ts_rhs with U0 = lambda^{n+1}, U1 = lambda^{n+2}, the row p_n as the load and phi = 1,
//     then lssvr_tridiag_bc_solve_multi on the bands the forward loop assembled, with zero end data.
//       dJ/drho_eq = -sum_n h_e w_q lambda^n_eq w^n_eq         (w^n: the nodal BDF difference)
//   Newmark loop of  rho u_tt + d u_t - (a u')' + c u = f(x, t)  (section 34).  The backward sweep alternates
//     lssvr_tridiag_bc_solve_multi on the forward loop's bands with the adjoint advance of newmark_adjoint.hip.
//       dJ/drho_eq = -sum_n h_e w_q lambda^n_eq acc^n_eq       dJ/dd_eq = -sum_n h_e w_q lambda^n_eq v^n_eq
//   semilinear BDF loop of  rho u_t - (a u')' + c u + g(x, u) = f(x, t)  (section 36).  The BDF pass, with one matrix
//     J_n per level (timestep_nl_adjoint.hip writes its end entries) and, per table q_k of the law,
//       dJ/dq_{k,eq} = -sum_n h_e w_q lambda^n_eq dg/dq_k(u^n_eq)      (lssvr_chunk_sens.hpp: ChunkNlGq)
//   all:
//       dJ/da_eq   = -sum_n (w_q / h_e) dlambda^n_e du^n_e     dJ/dc_eq = -sum_n h_e w_q lambda^n_eq u^n_eq
//       dJ/df_{r,eq} = +sum_n phi_r(t_n) h_e w_q lambda^n_eq
//     and the end gradients dJ/dg(t_n), dJ/dkappa.
// ONE launch takes a chunk: one thread per TABLE ENTRY, as in sensitivity.hip and for its reason (every store of a wave
// is 64 consecutive doubles whatever nquad is), an inner loop over the chunk's levels with the sums in registers, one
// store per table.  A launch per level into per-level tables and a sum over time would move N times the table bytes;
// here a table is written once per chunk, and the mesh and the rule (and for BDF two of the three trajectory rows of a
// step) are reused from the level before.  No reduction, no atomics, no LDS, no scratch; 256 threads, at most 1024
// workgroups, grid-stride; the end gradients, 2 m + 2 values, are written by the first thread of the same launch.
// FP64, -ffp-contract=off.
#include "lssvr_chunk_sens.hpp"
#include "lssvr_p1.hpp"

namespace lssvr {

namespace {

template <class Args> LSSVR_SENS_HD bool any_table(const Args& a) {
  return a.ga || a.gc || a.grho || ChunkScheme<Args>::gd(a) || a.gf || ChunkScheme<Args>::gq(a);
}

template <class Args> __global__ __launch_bounds__(kBlock) void chunk_sensitivity_kernel(Args a, QuadRule q) {
  if (any_table(a)) {
    const int64_t tab = a.ne * (int64_t)a.nquad, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < tab; idx += stride)
      chunk_sens_entry(a, q, idx);
  }
  if (a.out_g && blockIdx.x == 0 && threadIdx.x == 0) chunk_sens_ends(a);
}

}  // namespace

template <class Args> hipError_t chunk_sensitivity(const Args& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(chunk_sensitivity_kernel<Args>,
                     dim3((unsigned)(any_table(a) ? sens_blocks(a.ne * (int64_t)a.nquad) : 1)), dim3(kBlock), 0, s, a,
                     q);
  return hipGetLastError();
}

template <class Args> bool chunk_sensitivity_host(const Args& a) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return false;
  const int64_t tab = a.ne * (int64_t)a.nquad;
  if (any_table(a))
    for (int64_t idx = 0; idx < tab; ++idx) chunk_sens_entry(a, q, idx);
  if (a.out_g) chunk_sens_ends(a);
  return true;
}

template hipError_t chunk_sensitivity(const TsSensArgs&, hipStream_t);
template hipError_t chunk_sensitivity(const NmSensArgs&, hipStream_t);
template hipError_t chunk_sensitivity(const TsNlSensArgs&, hipStream_t);
template bool chunk_sensitivity_host(const TsSensArgs&);
template bool chunk_sensitivity_host(const NmSensArgs&);
template bool chunk_sensitivity_host(const TsNlSensArgs&);

}  // namespace lssvr
