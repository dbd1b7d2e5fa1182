// The tabulated family of g(x, u) of the semilinear problems, shared by nonlinear.hip and
// timestep_nl.hip: one inline routine for the device and for the host mirrors, so every caller forms g and g_u with
// the same operations in the same order.
// FP64, -ffp-contract=off.
#pragma once
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

#include <cmath>

namespace lssvr {

// g and d = g_u at one point, idx its position in every one of the nterm tables q_tabs (each of tab doubles), uh the
// value of the P1 interpolant there.  The order of every sum:
//   POLY   g = q_K;  g = g u_h + q_k            k = K-1 .. 0      (K = nterm - 1)
//          d = (double)K q_K;  d = d u_h + (double)k q_k           k = K-1 .. 1;  nterm = 1: d = 0
//   EXP    E = exp(q_1 u_h);  g = q_0 E;  d = (q_0 q_1) E
__host__ __device__ __forceinline__ void nl_family(int kind, int nterm, const double* q_tabs, int64_t tab, int64_t idx,
                                                   double uh, double& g, double& d) {
  if (kind == LSSVR_NL_EXP) {
    const double q0 = q_tabs[idx], q1 = q_tabs[tab + idx];
    const double E = exp(q1 * uh);
    g = q0 * E;
    d = (q0 * q1) * E;
  } else {
    const int K = nterm - 1;
    const double qK = q_tabs[(int64_t)K * tab + idx];
    g = qK;
    d = K == 0 ? 0.0 : (double)K * qK;
    for (int j = K - 1; j >= 0; --j) {
      const double qj = q_tabs[(int64_t)j * tab + idx];
      g = g * uh + qj;
      if (j >= 1) d = d * uh + (double)j * qj;
    }
  }
}

}  // namespace lssvr
