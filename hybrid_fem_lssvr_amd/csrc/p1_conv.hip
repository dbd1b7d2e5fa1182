// P1 assembly of -(a u')' + b u' + c u = f: the bands of lssvr_p1_assemble_react plus the Galerkin matrix of the
// convection term,
//   C_e[i][j] = sum_q w_q b(x_q) phi_i(xi_q) * s_j,   s_0 = -1, s_1 = +1   (h phi_j' = -+1, the h cancels),
// which is not symmetric: the one `off` band becomes `sub` (u_i in row i+1) and `sup` (u_{i+1} in row i).
// With beta0_e = sum_q w_q b_q (1 - xi_q) and beta1_e = sum_q w_q b_q xi_q (beta0 + beta1 = the quadrature mean of b):
//   sub[i]  = -k_i + m_i[0][1] - beta1_i,      sup[i] = -k_i + m_i[0][1] + beta0_i,
//   diag[i] = (k_i + m_i[0][0] - beta0_i) + (k_{i-1} + m_{i-1}[1][1] + beta1_{i-1}).
// tridiag.hip solves these bands.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_p1.hpp"

namespace lssvr {

struct ElemConv {
  double b0, b1;
};

__device__ __forceinline__ ElemConv p1_element_conv(const P1ConvArgs& p, const QuadRule& q, int64_t e) {
  double b0 = 0.0, b1 = 0.0;
  for (int k = 0; k < p.nquad; ++k) {
    const double xi = q.xi[k];
    const double bq = p.b_quad[e * p.nquad + k];
    b0 += (q.wt[k] * (1.0 - xi)) * bq;
    b1 += (q.wt[k] * xi) * bq;
  }
  return ElemConv{b0, b1};
}

// p1_node_react with the two off-diagonal bands; the same race-free gather per node (no atomics, bitwise
// reproducible).  An absent table contributes exact zeros, so b_quad == NULL gives sub == sup == the `off` of
// p1_node_react (of p1_node without c_quad), and diag and load theirs, bit for bit.
template <bool SIN>
__device__ __forceinline__ void p1_node_conv(const P1ConvArgs& p, const QuadRule& q, int64_t i) {
  double d = 0.0, l = 0.0;
  if (i < p.ne) {
    const ElemLocal r = p1_element<SIN>(p, q, i);
    const ElemMass m = p.c_quad ? p1_element_mass(p, q, i) : ElemMass{0.0, 0.0, 0.0};
    const ElemConv c = p.b_quad ? p1_element_conv(p, q, i) : ElemConv{0.0, 0.0};
    d += (r.k + m.ll) - c.b0;
    l += r.fl;
    band_store(p, &p.sub[i], (m.lr - r.k) - c.b1);
    band_store(p, &p.sup[i], (m.lr - r.k) + c.b0);
    if (p.kloc) p.kloc[i] = r.k;
    if (p.floc) {
      p.floc[2 * i] = r.fl;
      p.floc[2 * i + 1] = r.fr;
    }
  }
  if (i > 0) {
    const ElemLocal r = p1_element<SIN>(p, q, i - 1);
    const ElemMass m = p.c_quad ? p1_element_mass(p, q, i - 1) : ElemMass{0.0, 0.0, 0.0};
    const ElemConv c = p.b_quad ? p1_element_conv(p, q, i - 1) : ElemConv{0.0, 0.0};
    d += (r.k + m.rr) + c.b1;
    l += r.fr;
  }
  band_store(p, &p.diag[i], d);
  band_store(p, &p.load[i], l);
}

template <bool SIN>
__global__ __launch_bounds__(kBlock) void p1_assemble_conv_kernel(P1ConvArgs p, QuadRule q) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= p.ne; i += (int64_t)gridDim.x * kBlock)
    p1_node_conv<SIN>(p, q, i);
}

hipError_t p1_assemble_conv(const P1ConvArgs& a, hipStream_t s) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return hipErrorInvalidValue;
  const int64_t nn = a.ne + 1;
  const unsigned blocks = (unsigned)((nn + kBlock - 1) / kBlock < 16384 ? (nn + kBlock - 1) / kBlock : 16384);
  if (a.rhs_id == LSSVR_RHS_SIN)
    hipLaunchKernelGGL(p1_assemble_conv_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, a, q);
  else
    hipLaunchKernelGGL(p1_assemble_conv_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, a, q);
  return hipGetLastError();
}

}  // namespace lssvr
