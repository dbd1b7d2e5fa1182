// The routines behind every value of newmark_adjoint.hip: the device kernels and the host
// mirrors call them, and with -ffp-contract=off they are bit-equal.
#pragma once
#include "lssvr_sens.hpp"

namespace lssvr {

// (M lam)_i of the bands (diag [ne+1], off [ne]), the order of wave_row (wave.hip):
//   (off[i-1] lam[i-1] + diag[i] lam[i]) + off[i] lam[i+1]
// rows 0 and ne: the term of the missing neighbour is left out, not added as 0
LSSVR_SENS_HD double nm_band_row(const double* diag, const double* off, const double* lam, int64_t i, int64_t ne) {
  double s = diag[i] * lam[i];
  if (i > 0) s = off[i - 1] * lam[i - 1] + s;
  if (i < ne) s = s + off[i] * lam[i + 1];
  return s;
}

// Node i of one call between two backward solves.  With (vb, ab) = Vbar[i], Abar[i], the bars of level n+1, and
// p = P[i] (P NULL: p_n = 0, nothing is added), the order of every operation:
//   no lam (the first call of a sweep):
//     B_out = p + c_m (ab + c_va vb)                     (P NULL: the product alone)
//   else
//     as = ab + c_va vb
//     y  = (M_rho lam)_i,  z = (M_d lam)_i               (nm_band_row; z only with damping bands)
//     ut = (c_m y + c_d z) - c_m as;   vt = vb - z       (no damping bands: ut = c_m y - c_m as, vt = vb)
//     ub = p + ut                                        (P NULL: ub = ut)
//     vn = dt ut + vt;   an = c_u2 ut + c_v1 vt
//     V_out = vn;  A_out = an;  U_out = ub (unless NULL);  B_out = ub + c_m (an + c_va vn) (unless NULL)
// lam is an input of the launch, so no thread reads what another writes.
LSSVR_SENS_HD void nm_adj_row(const NmAdjArgs& a, int64_t i) {
  const double vb = a.Vbar[i], ab = a.Abar[i];
  if (!a.lam) {
    const double t = a.c_m * (ab + a.c_va * vb);
    a.B_out[i] = a.P ? a.P[i] + t : t;
    return;
  }
  const double as = ab + a.c_va * vb;
  const double y = nm_band_row(a.mdiag, a.moff, a.lam, i, a.ne);
  double ut, vt;
  if (a.ddiag) {
    const double z = nm_band_row(a.ddiag, a.doff, a.lam, i, a.ne);
    ut = (a.c_m * y + a.c_d * z) - a.c_m * as;
    vt = vb - z;
  } else {
    ut = a.c_m * y - a.c_m * as;
    vt = vb;
  }
  const double ub = a.P ? a.P[i] + ut : ut;
  const double vn = a.dt * ut + vt;
  const double an = a.c_u2 * ut + a.c_v1 * vt;
  a.V_out[i] = vn;
  a.A_out[i] = an;
  if (a.U_out) a.U_out[i] = ub;
  if (a.B_out) a.B_out[i] = ub + a.c_m * (an + a.c_va * vn);
}

// Entry idx = e * nquad + k of the tables ga, gc, grho, gd and gf[r], for the m levels of the chunk.  Row i of Z belongs
// to level n = n0 + m - 1 - i: the rows stand in the order in which the backward sweep produced them, n descending.
// With xi, w the point and weight k of the rule on [0, 1], h = x[e+1] - x[e], om = 1 - xi, wh = w / h, hw = h w (each
// formed once), (u0, u1) = u^n[e], u^n[e+1], (a0, a1) of acc^n, (v0, v1) of v^n and (z0, z1) = Z[i][e], Z[i][e+1], every
// sum starts from
//   s = accumulate ? what the output holds : 0
// and takes the levels one after the other, i = 0 .. m-1, one rounding per operation:
//   t   = hw (z0 om + z1 xi)
//   sa  = sa - ((wh (z1 - z0)) (u1 - u0))
//   sc  = sc - (t (u0 om + u1 xi))
//   sr  = sr - (t (a0 om + a1 xi))
//   sd  = sd - (t (v0 om + v1 xi))
//   sf_r = sf_r + phi[n][r] t                                       r = 0 .. R-1
// and the sums are stored once.  Because a sum CONTINUES from the stored value, a sweep gives the same bits however it
// is cut into chunks.  A table that is not asked for costs neither arithmetic nor a load of the trajectory that only
// it reads, nor a store.
LSSVR_SENS_HD void nm_sens_entry(const NmSensArgs& a, const QuadRule& q, int64_t idx) {
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
  double sd = acc && a.gd ? a.gd[idx] : 0.0;
  double sf[kNmSensMaxTerms];
#pragma unroll
  for (int r = 0; r < kNmSensMaxTerms; ++r) sf[r] = acc && a.gf && r < a.R ? a.gf[(int64_t)r * tab + idx] : 0.0;
  for (int i = 0; i < a.m; ++i) {
    const int64_t n = nhi - i, o = n * n1 + e;
    const double* z = a.Z + (int64_t)i * n1 + e;
    const double z0 = z[0], z1 = z[1];
    const double t = hw * (z0 * om + z1 * xi);
    if (a.ga || a.gc) {
      const double u0 = a.Utraj[o], u1 = a.Utraj[o + 1];
      if (a.ga) sa = sa - ((wh * (z1 - z0)) * (u1 - u0));
      if (a.gc) sc = sc - (t * (u0 * om + u1 * xi));
    }
    if (a.grho) sr = sr - (t * (a.Atraj[o] * om + a.Atraj[o + 1] * xi));
    if (a.gd) sd = sd - (t * (a.Vtraj[o] * om + a.Vtraj[o + 1] * xi));
    if (a.gf) {
      const double* phi = a.phi + n * a.R;
#pragma unroll
      for (int r = 0; r < kNmSensMaxTerms; ++r)
        if (r < a.R) sf[r] = sf[r] + phi[r] * t;
    }
  }
  if (a.ga) a.ga[idx] = sa;
  if (a.gc) a.gc[idx] = sc;
  if (a.grho) a.grho[idx] = sr;
  if (a.gd) a.gd[idx] = sd;
  if (a.gf) {
#pragma unroll
    for (int r = 0; r < kNmSensMaxTerms; ++r)
      if (r < a.R) a.gf[(int64_t)r * tab + idx] = sf[r];
  }
}

// The end gradients of the chunk: out_g[n][s] of every level n of the chunk, and out_kappa[s] continued from what it
// holds (accumulate) or from 0.  With z = Z[i], B = Brows[i] (the right-hand side of the solve that gave z), u = u^n
// and (s0, sn) = band_ends, the end entries {sub[0], sup[ne-1]} of that solve's matrix:
//   Dirichlet end:  out_g[n][0] = B_0 - s0 z_1,   out_g[n][1] = B_ne - sn z_{ne-1};   kappa is left alone
//   Robin end:      out_g[n][s] = z_end;          kappa_s = kappa_s - (z_end u_end),   i = 0 .. m-1 in turn
LSSVR_SENS_HD void nm_sens_ends(const NmSensArgs& a) {
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
        a.out_g[2 * n + s] = a.Brows[(int64_t)i * n1 + end] - a.band_ends[s] * z[inner];
      }
    }
    a.out_kappa[s] = kap;
  }
}

}  // namespace lssvr
