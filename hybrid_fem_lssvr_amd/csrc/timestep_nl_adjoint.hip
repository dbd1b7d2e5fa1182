// The backward step of the semilinear BDF loop  rho u_t - (a u')' + c u + g(x, u) = f(x, t)  (DESIGN.md section 36).
// The adjoint of the CONVERGED implicit step n solves  J_n lambda^n = B_n  with
//   J_n = K + M(c + alpha_n rho / dt + g_u(., u^n_h))            linearised AT u^n, symmetric (no convection)
//   B_n = p_n + (1/dt) M_rho (beta0_{n+1} lambda^{n+1} + beta1_{n+2} lambda^{n+2})
// ONE launch per level, one thread per NODE, writes all that the solve and the chunk pass need of it:
//   diag, off      the bands of J_n: the per-point sums of ts_nl_element (lssvr_ts_nl.hpp) in their order, gathered as
//                  ts_nl_assemble gathers them -- bit-equal to lssvr_ts_nl_assemble at v = u^n, whose Newton load is
//                  not needed here and not written
//   B              the row of ts_rhs_row (lssvr_ts.hpp) -- bit-equal to lssvr_ts_rhs
//   band_ends      {off[0], off[ne-1]}, by the threads that form them, into the chunk's row of this level
// It replaces the chain lssvr_ts_rhs + lssvr_ts_nl_assemble + two slices.  No atomics, no LDS, no scratch.  The node
// routine is __host__ __device__: lssvr_semilinear_adjoint_step_host runs the same code (bit-equal but for exp, libm on
// the host).  FP64, -ffp-contract=off.
#include "lssvr_ts.hpp"
#include "lssvr_ts_nl.hpp"

namespace lssvr {

namespace {

// Node i, in ts_nl_node's order:  d = 0; d += k + ll (right element); d += k + rr (left element);  off[i] = lr - k of
// the right element;  B[i] = ts_rhs_row
LSSVR_TSNL_HD void ts_nl_adjoint_node(const TsNlAdjArgs& a, const QuadRule& q, int64_t i) {
  const TsNlArgs& nl = a.nl;
  double d = 0.0;
  if (i < nl.ne) {
    const TsNlElem el = ts_nl_element(nl, q, i);
    d += el.k + el.ll;
    const double o = el.lr - el.k;
    nl.off[i] = o;
    if (i == 0) a.band_ends[0] = o;
    if (i == nl.ne - 1) a.band_ends[1] = o;
  }
  if (i > 0) {
    const TsNlElem el = ts_nl_element(nl, q, i - 1);
    d += el.k + el.rr;
  }
  nl.diag[i] = d;
  a.B[i] = ts_rhs_row(a.rhs, 0, i);
}

__global__ __launch_bounds__(kTsNlBlock) void ts_nl_adjoint_step_kernel(TsNlAdjArgs a, QuadRule q) {
  const int64_t stride = (int64_t)gridDim.x * kTsNlBlock;
  for (int64_t i = (int64_t)blockIdx.x * kTsNlBlock + threadIdx.x; i <= a.nl.ne; i += stride)
    ts_nl_adjoint_node(a, q, i);
}

}  // namespace

hipError_t ts_nl_adjoint_step(const TsNlAdjArgs& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.nl.nquad, q)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ts_nl_adjoint_step_kernel, dim3(ts_nl_blocks(a.nl.ne)), dim3(kTsNlBlock), 0, s, a, q);
  return hipGetLastError();
}

bool ts_nl_adjoint_step_host(const TsNlAdjArgs& a) {
  QuadRule q;
  if (!quad_rule(a.nl.nquad, q)) return false;
  for (int64_t i = 0; i <= a.nl.ne; ++i) ts_nl_adjoint_node(a, q, i);
  return true;
}

}  // namespace lssvr
