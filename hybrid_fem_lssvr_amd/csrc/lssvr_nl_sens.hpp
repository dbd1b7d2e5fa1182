// The one routine behind dJ/dq_k of nl_sensitivity.hip: the device kernel and the host mirror
// call it, and with -ffp-contract=off they are bit-equal, except for exp, which is libm on the host and the device
// library's on the GPU.  The four tables a, b, c, f and the end gradients are sens_entry and sens_ends of lssvr_sens.hpp,
// unchanged.
#pragma once
#include "lssvr_sens.hpp"

#include <cmath>

namespace lssvr {

// the largest nterm (LSSVR_NL_POLY): the k-loop below is unrolled over it with the uniform bound nterm, so no lane
// indexes a private array
constexpr int kNlSensMaxTerms = 6;

// Entry idx = e * nquad + k of the nterm tables of gq, for every case.  With xi, w, h, om of sens_point and
// (u0, u1) = U[j][e], U[j][e+1], (z0, z1) likewise, exactly as sens_entry forms them, the order of every operation:
//   zq = z0 om + z1 xi;   s = (h w) zq;   uq = u0 om + u1 xi
//   POLY   p_0 = 1;  p_k = p_{k-1} uq;  gq_0 = -s;  gq_k = -(s p_k)       k = 1 .. nterm-1
//          (p_1 = 1 uq is uq itself: gq_0 is -gf and gq_1 is gc of sens_entry, bit for bit)
//   EXP    E = exp(q_1 uq);  gq_0 = -(s E);  gq_1 = -(s ((q_0 uq) E))
LSSVR_SENS_HD void nl_sens_entry(const NlSensArgs& a, const QuadRule& q, int64_t idx) {
  const SensArgs& b = a.s;
  const int64_t tab = b.ne * (int64_t)b.nquad;
  const SensPoint p = sens_point(b.x, b.ne, b.nquad, q, idx);
  const bool is_exp = a.kind == LSSVR_NL_EXP;
  const double q0 = is_exp ? a.q_tabs[idx] : 0.0, q1 = is_exp ? a.q_tabs[tab + idx] : 0.0;
  for (int j = 0; j < b.nc; ++j) {
    const double* u = sens_u(b, j) + p.e;
    const double* z = sens_z(b, j) + p.e;
    const double u0 = u[0], u1 = u[1], z0 = z[0], z1 = z[1];
    const double s = p.hw * (z0 * p.om + z1 * p.xi);
    const double uq = u0 * p.om + u1 * p.xi;
    double* g = a.gq + (int64_t)j * a.nterm * tab + idx;
    if (is_exp) {
      const double E = exp(q1 * uq);
      g[0] = -(s * E);
      g[tab] = -(s * ((q0 * uq) * E));
    } else {
      g[0] = -s;
      double pk = 1.0;
#pragma unroll
      for (int k = 1; k < kNlSensMaxTerms; ++k) {
        if (k < a.nterm) {
          pk = pk * uq;
          g[k * tab] = -(s * pk);
        }
      }
    }
  }
}

}  // namespace lssvr
