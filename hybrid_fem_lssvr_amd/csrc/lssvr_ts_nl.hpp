// What timestep_nl.hip (the Newton matrix and load of a semilinear time step) and
// timestep_nl_adjoint.hip (the Jacobian of the backward step, section 36) share: the launch constants and the one inline
// element routine behind every band of both.  Device kernels and host mirrors call the same routine; with
// -ffp-contract=off they are bit-equal (but for exp, libm on the host).
#pragma once
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_nl_family.hpp"
#include "lssvr_p1.hpp"

#define LSSVR_TSNL_HD __host__ __device__ __forceinline__

namespace lssvr {

// threads per workgroup (four waves) and the grid cap of the grid-stride loop (that of p1_assemble_react)
constexpr int kTsNlBlock = 256;
constexpr int kTsNlMaxBlocks = 16384;

inline unsigned ts_nl_blocks(int64_t ne) {
  const int64_t b = (ne + 1 + kTsNlBlock - 1) / kTsNlBlock;
  return (unsigned)(b < kTsNlMaxBlocks ? b : kTsNlMaxBlocks);
}

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

}  // namespace lssvr
