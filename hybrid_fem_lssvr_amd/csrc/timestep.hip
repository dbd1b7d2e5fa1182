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
#include "lssvr_ts.hpp"

namespace lssvr {

namespace {

// ts_blend and ts_rhs_row, the routines behind a row of the right-hand side, live in lssvr_ts.hpp: timestep_adapt.hip
// runs the same ones
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
