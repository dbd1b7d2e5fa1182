// The routines behind every value of timestep_sens.hip: the device kernel and the host mirror call
// them, and with -ffp-contract=off they are bit-equal.
#pragma once
#include "lssvr_sens.hpp"

namespace lssvr {

// w = inv_dt ((alpha u2 - beta0 u0) - beta1 u1), the nodal BDF difference of a step from u2 = u^n, u0 = u^{n-1},
// u1 = u^{n-2}: the order of ts_diff (timestep.hip); beta1 == 0 leaves u1 out
LSSVR_SENS_HD double ts_sens_diff(double alpha, double beta0, double beta1, double inv_dt, double u2, double u0,
                                  double u1) {
  const double d = alpha * u2 - beta0 * u0;
  return inv_dt * (beta1 == 0.0 ? d : d - beta1 * u1);
}

// Entry idx = e * nquad + k of the tables ga, gc, grho and gf[r], for the m steps of the chunk.  Row i of Z belongs to
// step n = n0 + m - 1 - i: the rows stand in the order in which the backward sweep produced them, n descending.  With
// xi, w the point and weight k of the rule on [0, 1], h = x[e+1] - x[e], om = 1 - xi, wh = w / h, hw = h w (each formed
// once), (u0, u1) = u^n[e], u^n[e+1], (p0, p1) of u^{n-1}, (q0, q1) of u^{n-2} (0 for n < 2: there is no such row) and
// (z0, z1) = Z[i][e], Z[i][e+1], every sum starts from
//   s = accumulate ? what the output holds : 0
// and takes the steps one after the other, i = 0 .. m-1, one rounding per operation:
//   zq  = z0 om + z1 xi;      t = hw zq
//   sa  = sa - ((wh (z1 - z0)) (u1 - u0))
//   sc  = sc - (t (u0 om + u1 xi))
//   wj  = inv_dt ((alpha uj - beta0 pj) - beta1 qj), j = 0, 1      (ts_sens_diff; (alpha, beta0, beta1) = coef[i])
//   sr  = sr - (t (w0 om + w1 xi))
//   sf_r = sf_r + phi[n-1][r] t                                     r = 0 .. R-1
// and the sums are stored once.  Because a sum CONTINUES from the stored value, a sweep gives the same bits however it
// is cut into chunks.  The three rows of the trajectory rotate through registers: a step loads row n-2 only.  A table
// that is not asked for costs neither arithmetic that only it needs nor a store.
LSSVR_SENS_HD void ts_sens_entry(const TsSensArgs& a, const QuadRule& q, int64_t idx) {
  const int64_t tab = a.ne * (int64_t)a.nquad, n1 = a.ne + 1;
  const int64_t e = tab <= (int64_t)0xffffffffu ? (int64_t)((uint32_t)idx / (uint32_t)a.nquad) : idx / a.nquad;
  const int k = (int)(idx - e * a.nquad);
  const double xi = sens_pick(q.xi, k), w = sens_pick(q.wt, k);
  const double h = a.x[e + 1] - a.x[e];
  const double om = 1.0 - xi, wh = w / h, hw = h * w;
  const int64_t nhi = a.n0 + a.m - 1;
  const bool acc = a.accumulate != 0;
  double sa = acc && a.ga ? a.ga[idx] : 0.0;
  double sc = acc && a.gc ? a.gc[idx] : 0.0;
  double sr = acc && a.grho ? a.grho[idx] : 0.0;
  double sf[kTsSensMaxTerms];
#pragma unroll
  for (int r = 0; r < kTsSensMaxTerms; ++r) sf[r] = acc && a.gf && r < a.R ? a.gf[(int64_t)r * tab + idx] : 0.0;
  const double* row = a.Utraj + nhi * n1 + e;
  double u0 = row[0], u1 = row[1];
  double p0 = (row - n1)[0], p1 = (row - n1)[1];             // (n0 >= 1: row nhi - 1 exists)
  for (int i = 0; i < a.m; ++i) {
    const int64_t n = nhi - i;
    double q0 = 0.0, q1 = 0.0;
    if (n >= 2) {
      const double* r2 = a.Utraj + (n - 2) * n1 + e;
      q0 = r2[0];
      q1 = r2[1];
    }
    const double* z = a.Z + (int64_t)i * n1 + e;
    const double z0 = z[0], z1 = z[1];
    const double t = hw * (z0 * om + z1 * xi);
    if (a.ga) sa = sa - ((wh * (z1 - z0)) * (u1 - u0));
    if (a.gc) sc = sc - (t * (u0 * om + u1 * xi));
    if (a.grho) {
      const double al = a.coef[i][0], b0 = a.coef[i][1], b1 = a.coef[i][2];
      const double w0 = ts_sens_diff(al, b0, b1, a.inv_dt, u0, p0, q0);
      const double w1 = ts_sens_diff(al, b0, b1, a.inv_dt, u1, p1, q1);
      sr = sr - (t * (w0 * om + w1 * xi));
    }
    if (a.gf) {
      const double* phi = a.phi + (n - 1) * a.R;
#pragma unroll
      for (int r = 0; r < kTsSensMaxTerms; ++r)
        if (r < a.R) sf[r] = sf[r] + phi[r] * t;
    }
    u0 = p0, u1 = p1, p0 = q0, p1 = q1;
  }
  if (a.ga) a.ga[idx] = sa;
  if (a.gc) a.gc[idx] = sc;
  if (a.grho) a.grho[idx] = sr;
  if (a.gf) {
#pragma unroll
    for (int r = 0; r < kTsSensMaxTerms; ++r)
      if (r < a.R) a.gf[(int64_t)r * tab + idx] = sf[r];
  }
}

// The end gradients of the chunk: out_g[n][s] of every step n of the chunk, and out_kappa[s] continued from what it
// holds (accumulate) or from 0.  With z = Z[i], B = Brows[i] (the adjoint right-hand side of step n, natural end rows
// included), u = u^n and (s0, sn) = band_ends[band_row[i]], the end entries {sub[0], sup[ne-1]} of step n's matrix:
//   Dirichlet end:  out_g[n][0] = B_0 - s0 z_1,   out_g[n][1] = B_ne - sn z_{ne-1};   kappa is left alone
//   Robin end:      out_g[n][s] = z_end;          kappa_s = kappa_s - (z_end u_end),   i = 0 .. m-1 in turn
LSSVR_SENS_HD void ts_sens_ends(const TsSensArgs& a) {
  const int64_t n1 = a.ne + 1, nhi = a.n0 + a.m - 1;
  for (int s = 0; s < 2; ++s) {
    const int64_t end = s ? a.ne : 0, inner = s ? a.ne - 1 : 1;
    double kap = a.accumulate ? a.out_kappa[s] : 0.0;
    for (int i = 0; i < a.m; ++i) {
      const int64_t n = nhi - i;
      const double* z = a.Z + (int64_t)i * n1;
      if (a.kind[s] == LSSVR_END_ROBIN) {
        a.out_g[2 * n + s] = z[end];
        kap = kap - (z[end] * a.Utraj[n * n1 + end]);
      } else {
        a.out_g[2 * n + s] = a.Brows[(int64_t)i * n1 + end] - a.band_ends[2 * a.band_row[i] + s] * z[inner];
      }
    }
    a.out_kappa[s] = kap;
  }
}

}  // namespace lssvr
