// What timestep.hip (fixed step) and timestep_adapt.hip (variable step, section 30) share: the
// launch constants and the one inline routine behind the right-hand side of a BDF step.  Device kernels and host
// mirrors call the same routine; with -ffp-contract=off they are bit-equal.
#pragma once
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

#define LSSVR_TS_HD __host__ __device__ __forceinline__

namespace lssvr {

// threads per workgroup (four waves) and the grid cap of the grid-stride loops
constexpr int kTsBlock = 256;
constexpr int kTsMaxBlocks = 1024;

inline int64_t ts_blocks(int64_t n) {
  const int64_t b = (n + kTsBlock - 1) / kTsBlock;
  return b < 1 ? 1 : (b < kTsMaxBlocks ? b : kTsMaxBlocks);
}

// v_i = beta0 U0_i + beta1 U1_i; beta1 == 0 reads no U1 (BDF1, and the first step of BDF2)
LSSVR_TS_HD double ts_blend(const double* __restrict__ U0, const double* __restrict__ U1, double beta0, double beta1,
                            int64_t i) {
  const double v = beta0 * U0[i];
  return beta1 == 0.0 ? v : v + beta1 * U1[i];
}

// Row i of case j.  The order of every sum:
//   v        = beta0 U0 + beta1 U1                          (ts_blend)
//   m        = (moff[i-1] v[i-1] + mdiag[i] v[i]) + moff[i] v[i+1]      (rows 0 and ne: the term of the missing
//                                                                          neighbour is left out, not added as 0)
//   out      = ((inv_dt m + phi[0] loads[0][i]) + phi[1] loads[1][i]) + ...     r ascending
LSSVR_TS_HD double ts_rhs_row(const TsRhsArgs& a, int j, int64_t i) {
  const int64_t n = a.ne + 1;
  const double* U0 = a.U0 + (int64_t)j * n;
  const double* U1 = a.beta1 == 0.0 ? nullptr : a.U1 + (int64_t)j * n;
  double m = a.mdiag[i] * ts_blend(U0, U1, a.beta0, a.beta1, i);
  if (i > 0) m = a.moff[i - 1] * ts_blend(U0, U1, a.beta0, a.beta1, i - 1) + m;
  if (i < a.ne) m = m + a.moff[i] * ts_blend(U0, U1, a.beta0, a.beta1, i + 1);
  double s = a.inv_dt * m;
  const double* phi = a.phi + (int64_t)j * a.R;
  for (int r = 0; r < a.R; ++r) s = s + phi[r] * a.loads[(int64_t)r * n + i];
  return s;
}

}  // namespace lssvr
