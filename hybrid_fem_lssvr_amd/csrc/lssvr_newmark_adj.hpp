// The routines behind every value of newmark_adjoint.hip: the device kernel and the host mirror
// call them, and with -ffp-contract=off they are bit-equal.
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

}  // namespace lssvr
