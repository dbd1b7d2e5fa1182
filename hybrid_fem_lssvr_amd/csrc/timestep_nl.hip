// Semilinear transient problems  rho u_t - (a u')' + c u + g(x, u) = f(x, t)  on the P1 mesh:
// BDF1 / BDF2 as in section 26, each step solved by a fixed number of Newton iterations.  The iterate v_k -> v_{k+1} of
// step n+1 is the LINEAR problem with the reaction  c + alpha rho / dt + g_u(x, v_k,h)  and the right-hand side
// r + L(-g + g_u v_k,h),  r the vector of lssvr_ts_rhs (once per step), v_k,h the P1 interpolant and L the P1 load
// assembly; the solve is lssvr_tridiag_bc_solve_multi and the monitor lssvr_nl_residual.  This file adds the one piece
// that changes every iteration:
//   nl_assemble   the three bands of the Newton matrix and its right-hand side in ONE pass, without the two
//                 [ne][nquad] tables that lssvr_nl_linearize -> lssvr_p1_assemble_react put through memory
// One thread per NODE gathers its right and its left element (the race-free gather of p1_node_react, lssvr_p1.hpp): no
// atomics, no LDS, no scratch.  The sums are those of p1_element / p1_element_mass / p1_node_react in their order and
// g, g_u come from nl_family, so the result is bit-equal to the chain it replaces.  The element routine is
// __host__ __device__ (lssvr_ts_nl.hpp, shared with timestep_nl_adjoint.hip): lssvr_ts_nl_assemble_host runs the same
// code (bit-equal but for exp, libm on the host).
// FP64, -ffp-contract=off.
#include "lssvr_ts_nl.hpp"

namespace lssvr {

namespace {

// Node i, in p1_node_react's order:  d = 0; d += k + ll (right element); d += k + rr (left element);  l likewise with
// fl, fr;  off[i] = lr - k of the right element;  rhs[i] = r[i] + l
LSSVR_TSNL_HD void ts_nl_node(const TsNlArgs& a, const QuadRule& q, int64_t i) {
  double d = 0.0, l = 0.0;
  if (i < a.ne) {
    const TsNlElem el = ts_nl_element(a, q, i);
    d += el.k + el.ll;
    l += el.fl;
    a.off[i] = el.lr - el.k;
  }
  if (i > 0) {
    const TsNlElem el = ts_nl_element(a, q, i - 1);
    d += el.k + el.rr;
    l += el.fr;
  }
  a.diag[i] = d;
  a.rhs[i] = a.r[i] + l;
}

__global__ __launch_bounds__(kTsNlBlock) void ts_nl_assemble_kernel(TsNlArgs a, QuadRule q) {
  const int64_t stride = (int64_t)gridDim.x * kTsNlBlock;
  for (int64_t i = (int64_t)blockIdx.x * kTsNlBlock + threadIdx.x; i <= a.ne; i += stride) ts_nl_node(a, q, i);
}

}  // namespace

hipError_t ts_nl_assemble(const TsNlArgs& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ts_nl_assemble_kernel, dim3(ts_nl_blocks(a.ne)), dim3(kTsNlBlock), 0, s, a, q);
  return hipGetLastError();
}

bool ts_nl_assemble_host(const TsNlArgs& a) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return false;
  for (int64_t i = 0; i <= a.ne; ++i) ts_nl_node(a, q, i);
  return true;
}

}  // namespace lssvr
