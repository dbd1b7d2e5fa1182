// Transient problems  rho u_t - (a u')' + c u = f(x, t)  on the P1 mesh, BDF1 / BDF2 with a fixed step dt (DESIGN.md
// section 26).  Step n+1 solves  A_alpha u^{n+1} = (1/dt) M (beta0 u^n + beta1 u^{n-1}) + load(t_{n+1}),  A_alpha the
// bands of lssvr_p1_assemble_react with c_quad = c + alpha rho / dt and M = (mdiag, moff) those of the same entry with
// a_quad = 0 and c_quad = rho; the solve is lssvr_tridiag_bc_solve_multi.  This file adds what goes around it:
//   rhs           the right-hand side of one step, for nc cases at once
//   source_table  for one snapshot, the right-hand-side table  f(., t) - rho I_h w  of its elliptic enhancement problem
// Both are one pass over their output with no reduction, no atomics, no LDS and no scratch; every scalar that changes
// from step to step (phi, the end data) is read from device memory, so a time loop issues no copy and no
// synchronisation.  Each value comes from one inline routine that the host mirrors (lssvr_ts_*_host) call too: with
// -ffp-contract=off the two are bit-equal.
// FP64, -ffp-contract=off.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

#define LSSVR_TS_HD __host__ __device__ __forceinline__

namespace lssvr {

namespace {

// threads per workgroup (four waves) and the grid cap of the grid-stride loops
constexpr int kTsBlock = 256;
constexpr int kTsMaxBlocks = 1024;

int64_t ts_blocks(int64_t n) {
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

__global__ __launch_bounds__(kTsBlock) void ts_rhs_kernel(TsRhsArgs a, double* __restrict__ out) {
  const int64_t n = a.ne + 1, stride = (int64_t)gridDim.x * kTsBlock;
  for (int64_t i = (int64_t)blockIdx.x * kTsBlock + threadIdx.x; i < n; i += stride)
    for (int j = 0; j < a.nc; ++j) out[(int64_t)j * n + i] = ts_rhs_row(a, j, i);
}

// w_i = inv_dt ((alpha U2_i - beta0 U0_i) - beta1 U1_i), the nodal BDF difference; beta1 == 0 reads no U1
LSSVR_TS_HD double ts_diff(const TsSourceArgs& a, int64_t i) {
  const double d = a.alpha * a.U2[i] - a.beta0 * a.U0[i];
  return a.inv_dt * (a.beta1 == 0.0 ? d : d - a.beta1 * a.U1[i]);
}

// Entry (e, k) of the table.  The order of every sum:
//   f        = (phi[0] ftab[0] + phi[1] ftab[1]) + ...         r ascending
//   I_h w    = w_e + (w_{e+1} - w_e) (k / (n_colloc - 1))      the division first
//   out      = f - rho_tab (I_h w)
LSSVR_TS_HD double ts_source_entry(const TsSourceArgs& a, int64_t e, int k, int64_t idx) {
  const int64_t tab = a.ne * (int64_t)a.n_colloc;
  double f = a.phi[0] * a.ftab[idx];
  for (int r = 1; r < a.R; ++r) f = f + a.phi[r] * a.ftab[(int64_t)r * tab + idx];
  const double w0 = ts_diff(a, e), w1 = ts_diff(a, e + 1);
  const double t = (double)k / (double)(a.n_colloc - 1);
  return f - a.rho_tab[idx] * (w0 + (w1 - w0) * t);
}

// idx runs over the table in memory order, so both layouts are read and written coalesced
LSSVR_TS_HD void ts_source_at(const TsSourceArgs& a, bool point_major, int64_t idx, double* __restrict__ out) {
  int64_t e;
  int k;
  if (point_major) {
    k = (int)(idx / a.ne);
    e = idx - (int64_t)k * a.ne;
  } else {
    e = idx / a.n_colloc;
    k = (int)(idx - e * a.n_colloc);
  }
  out[idx] = ts_source_entry(a, e, k, idx);
}

template <bool PM>
__global__ __launch_bounds__(kTsBlock) void ts_source_table_kernel(TsSourceArgs a, double* __restrict__ out) {
  const int64_t tab = a.ne * (int64_t)a.n_colloc, stride = (int64_t)gridDim.x * kTsBlock;
  for (int64_t idx = (int64_t)blockIdx.x * kTsBlock + threadIdx.x; idx < tab; idx += stride)
    ts_source_at(a, PM, idx, out);
}

}  // namespace

hipError_t ts_rhs(const TsRhsArgs& a, double* out, hipStream_t s) {
  hipLaunchKernelGGL(ts_rhs_kernel, dim3((unsigned)ts_blocks(a.ne + 1)), dim3(kTsBlock), 0, s, a, out);
  return hipGetLastError();
}

void ts_rhs_host(const TsRhsArgs& a, double* out) {
  const int64_t n = a.ne + 1;
  for (int j = 0; j < a.nc; ++j)
    for (int64_t i = 0; i < n; ++i) out[(int64_t)j * n + i] = ts_rhs_row(a, j, i);
}

hipError_t ts_source_table(const TsSourceArgs& a, bool point_major, double* out, hipStream_t s) {
  const dim3 grid((unsigned)ts_blocks(a.ne * (int64_t)a.n_colloc)), block(kTsBlock);
  if (point_major)
    hipLaunchKernelGGL(ts_source_table_kernel<true>, grid, block, 0, s, a, out);
  else
    hipLaunchKernelGGL(ts_source_table_kernel<false>, grid, block, 0, s, a, out);
  return hipGetLastError();
}

void ts_source_table_host(const TsSourceArgs& a, bool point_major, double* out) {
  const int64_t tab = a.ne * (int64_t)a.n_colloc;
  for (int64_t idx = 0; idx < tab; ++idx) ts_source_at(a, point_major, idx, out);
}

}  // namespace lssvr
