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
// __host__ __device__: lssvr_ts_nl_assemble_host runs the same code (bit-equal but for exp, libm on the host).
// FP64, -ffp-contract=off.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_nl_family.hpp"
#include "lssvr_p1.hpp"

#define LSSVR_TSNL_HD __host__ __device__ __forceinline__

namespace lssvr {

namespace {

// threads per workgroup (four waves) and the grid cap of the grid-stride loop (that of p1_assemble_react)
constexpr int kTsNlBlock = 256;
constexpr int kTsNlMaxBlocks = 16384;

// what one element gives its two nodes: k = abar / h, the two loads and the mass matrix of c_eff
struct TsNlElem {
  double k, fl, fr, ll, lr, rr;
};

// Element e.  Per quadrature point (xi, w), idx = e nquad + k:
//   u_h   = u_e + (u_{e+1} - u_e) xi;   g, d = nl_family at (idx, u_h)
//   c_eff = cs + d;   f_eff = (0 - g) + d u_h
//   sl += (w (1 - xi)) f_eff;  sr += (w xi) f_eff;  am += w a                         (p1_element)
//   wc = w c_eff;  ll += wc ((1 - xi)(1 - xi));  lr += wc ((1 - xi) xi);  rr += wc (xi xi)      (p1_element_mass)
// then k = am / h (no a_quad: 1 / h), fl = h sl, fr = h sr, ll = h ll, lr = h lr, rr = h rr.
LSSVR_TSNL_HD TsNlElem ts_nl_element(const TsNlArgs& a, const QuadRule& q, int64_t e) {
  const int64_t tab = a.ne * (int64_t)a.nquad;
  const double h = a.x[e + 1] - a.x[e];
  const double u0 = a.u[e];
  const double du = a.u[e + 1] - u0;
  double sl = 0.0, sr = 0.0, am = 0.0, ll = 0.0, lr = 0.0, rr = 0.0;
  for (int k = 0; k < a.nquad; ++k) {
    const int64_t idx = e * a.nquad + k;
    const double xi = q.xi[k];
    const double uh = u0 + du * xi;
    double g, d;
    nl_family(a.kind, a.nterm, a.q_quad, tab, idx, uh, g, d);
    const double c = a.cs_quad[idx] + d;
    const double f = (0.0 - g) + d * uh;
    sl += (q.wt[k] * (1.0 - xi)) * f;
    sr += (q.wt[k] * xi) * f;
    if (a.a_quad) am += q.wt[k] * a.a_quad[idx];
    const double wc = q.wt[k] * c;
    ll += wc * ((1.0 - xi) * (1.0 - xi));
    lr += wc * ((1.0 - xi) * xi);
    rr += wc * (xi * xi);
  }
  TsNlElem r;
  r.k = (a.a_quad ? am : 1.0) / h;
  r.fl = h * sl;
  r.fr = h * sr;
  r.ll = h * ll;
  r.lr = h * lr;
  r.rr = h * rr;
  return r;
}

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
  const int64_t b = (a.ne + 1 + kTsNlBlock - 1) / kTsNlBlock;
  const unsigned blocks = (unsigned)(b < kTsNlMaxBlocks ? b : kTsNlMaxBlocks);
  hipLaunchKernelGGL(ts_nl_assemble_kernel, dim3(blocks), dim3(kTsNlBlock), 0, s, a, q);
  return hipGetLastError();
}

bool ts_nl_assemble_host(const TsNlArgs& a) {
  QuadRule q;
  if (!quad_rule(a.nquad, q)) return false;
  for (int64_t i = 0; i <= a.ne; ++i) ts_nl_node(a, q, i);
  return true;
}

}  // namespace lssvr
