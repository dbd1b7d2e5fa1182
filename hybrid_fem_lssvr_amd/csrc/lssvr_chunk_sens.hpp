// The routines behind every value of chunk_sens.hip, the chunk pass of the BDF loop and of the
// Newmark loop (section 34) and of the semilinear BDF loop (section 36): the device kernel and the host mirror call
// them, and with -ffp-contract=off they are bit-equal (but for exp of the semilinear EXP law, libm on the host).  One
// routine per job; ChunkScheme<Args> supplies, at compile time, the few points at which the loops differ.
#pragma once
#include "lssvr_nl_sens.hpp"

namespace lssvr {

// w = inv_dt ((alpha u2 - beta0 u0) - beta1 u1), the nodal BDF difference of a step from u2 = u^n, u0 = u^{n-1},
// u1 = u^{n-2}: the order of ts_diff (timestep.hip); beta1 == 0 leaves u1 out
LSSVR_SENS_HD double ts_sens_diff(double alpha, double beta0, double beta1, double inv_dt, double u2, double u0,
                                  double u1) {
  const double d = alpha * u2 - beta0 * u0;
  return inv_dt * (beta1 == 0.0 ? d : d - beta1 * u1);
}

// What a loop's chunk pass has of its own: where a level takes (u0, u1) = u^n[e], u^n[e+1] and the nodal pair (r0, r1)
// of the rho term, whether there is a table d with its pair, which row of phi is phi(t_n), and which row of band_ends
// belongs to step row i.  begin() is called once per entry, load() once per level before the pairs are used, in the
// order i = 0 .. m-1 (n descending), next() after the level.  Gq holds the running sums of the tables gq of a law
// g(x, u) (gq(a): where they go; nullptr: none): begin() once per entry, add() once per level, store() at the end.
template <class Args> struct ChunkScheme;

// a scheme without a law: no sums, no code
struct ChunkNoGq {
  template <class Args> LSSVR_SENS_HD void begin(const Args&, int64_t, int64_t, bool) {}
  template <class Args> LSSVR_SENS_HD void add(const Args&, double, double) {}
  template <class Args> LSSVR_SENS_HD void store(const Args&, int64_t, int64_t) const {}
};

// BDF: (r0, r1) = (w0, w1), wj = inv_dt ((alpha uj - beta0 pj) - beta1 qj) (ts_sens_diff; (alpha, beta0, beta1) =
// coef[i]) with (p0, p1) of u^{n-1} and (q0, q1) of u^{n-2} (0 for n < 2: there is no such row).  The three rows of the
// trajectory rotate through registers: a level loads row n-2 only.  No table d; phi(t_n) is row n-1.
template <> struct ChunkScheme<TsSensArgs> {
  double u0, u1, p0, p1, q0, q1;
  LSSVR_SENS_HD void begin(const TsSensArgs& a, int64_t e, int64_t nhi) {
    const double* row = a.Utraj + nhi * (a.ne + 1) + e;
    u0 = row[0], u1 = row[1];
    p0 = (row - (a.ne + 1))[0], p1 = (row - (a.ne + 1))[1];      // (n0 >= 1: row nhi - 1 exists)
  }
  LSSVR_SENS_HD void load(const TsSensArgs& a, int64_t e, int64_t n) {
    q0 = 0.0, q1 = 0.0;
    if (n >= 2) {
      const double* r2 = a.Utraj + (n - 2) * (a.ne + 1) + e;
      q0 = r2[0];
      q1 = r2[1];
    }
  }
  LSSVR_SENS_HD void rho_pair(const TsSensArgs& a, int i, double& r0, double& r1) const {
    const double al = a.coef[i][0], b0 = a.coef[i][1], b1 = a.coef[i][2];
    r0 = ts_sens_diff(al, b0, b1, a.inv_dt, u0, p0, q0);
    r1 = ts_sens_diff(al, b0, b1, a.inv_dt, u1, p1, q1);
  }
  LSSVR_SENS_HD void d_pair(const TsSensArgs&, double&, double&) const {}
  LSSVR_SENS_HD void next() { u0 = p0, u1 = p1, p0 = q0, p1 = q1; }
  static LSSVR_SENS_HD double* gd(const TsSensArgs&) { return nullptr; }
  static LSSVR_SENS_HD int64_t phi_row(int64_t n) { return n - 1; }
  static LSSVR_SENS_HD int band_row(const TsSensArgs& a, int i) { return a.band_row[i]; }
  using Gq = ChunkNoGq;
  static LSSVR_SENS_HD double* gq(const TsSensArgs&) { return nullptr; }
};

// Newmark: (r0, r1) of acc^n = Atraj[n] and the pair of the table d of v^n = Vtraj[n]; phi(t_n) is row n; one matrix
// for the whole chunk.  A table that is not asked for costs no load of the trajectory that only it reads: u^n is read
// for ga and gc alone.
template <> struct ChunkScheme<NmSensArgs> {
  double u0, u1;
  int64_t o;
  LSSVR_SENS_HD void begin(const NmSensArgs&, int64_t, int64_t) {}
  LSSVR_SENS_HD void load(const NmSensArgs& a, int64_t e, int64_t n) {
    o = n * (a.ne + 1) + e;
    if (a.ga || a.gc) u0 = a.Utraj[o], u1 = a.Utraj[o + 1];
  }
  LSSVR_SENS_HD void rho_pair(const NmSensArgs& a, int, double& r0, double& r1) const {
    r0 = a.Atraj[o], r1 = a.Atraj[o + 1];
  }
  LSSVR_SENS_HD void d_pair(const NmSensArgs& a, double& d0, double& d1) const {
    d0 = a.Vtraj[o], d1 = a.Vtraj[o + 1];
  }
  LSSVR_SENS_HD void next() {}
  static LSSVR_SENS_HD double* gd(const NmSensArgs& a) { return a.gd; }
  static LSSVR_SENS_HD int64_t phi_row(int64_t n) { return n; }
  static LSSVR_SENS_HD int band_row(const NmSensArgs&, int) { return 0; }
  using Gq = ChunkNoGq;
  static LSSVR_SENS_HD double* gq(const NmSensArgs&) { return nullptr; }
};

// The sums of gq [nterm][tab] at one entry.  With s = hw (z0 om + z1 xi) and uq = u0 om + u1 xi of the level, as
// chunk_sens_entry forms them for sc, level by level, one rounding per operation (the per-level terms are those of
// nl_sens_entry, lssvr_nl_sens.hpp):
//   POLY   p_0 = 1;  p_k = p_{k-1} uq;  gq_0 = gq_0 - s;  gq_k = gq_k - (s p_k)       k = 1 .. nterm-1
//          (p_1 = 1 uq is uq itself: gq_1 is gc, and with phi = 1 gq_0 is -gf, bit for bit)
//   EXP    E = exp(q_1 uq);  gq_0 = gq_0 - (s E);  gq_1 = gq_1 - (s ((q_0 uq) E))
// The k-loops are unrolled over kNlSensMaxTerms with the uniform bound nterm: no lane indexes a private array.
struct ChunkNlGq {
  double g[kNlSensMaxTerms];
  double q0, q1;
  LSSVR_SENS_HD void begin(const TsNlSensArgs& a, int64_t tab, int64_t idx, bool acc) {
    const bool is_exp = a.law == LSSVR_NL_EXP;
    q0 = is_exp ? a.q_tabs[idx] : 0.0;
    q1 = is_exp ? a.q_tabs[tab + idx] : 0.0;
#pragma unroll
    for (int k = 0; k < kNlSensMaxTerms; ++k) g[k] = acc && k < a.nterm ? a.gq[(int64_t)k * tab + idx] : 0.0;
  }
  LSSVR_SENS_HD void add(const TsNlSensArgs& a, double s, double uq) {
    if (a.law == LSSVR_NL_EXP) {
      const double E = exp(q1 * uq);
      g[0] = g[0] - (s * E);
      g[1] = g[1] - (s * ((q0 * uq) * E));
    } else {
      g[0] = g[0] - s;
      double pk = 1.0;
#pragma unroll
      for (int k = 1; k < kNlSensMaxTerms; ++k) {
        if (k < a.nterm) {
          pk = pk * uq;
          g[k] = g[k] - (s * pk);
        }
      }
    }
  }
  LSSVR_SENS_HD void store(const TsNlSensArgs& a, int64_t tab, int64_t idx) const {
#pragma unroll
    for (int k = 0; k < kNlSensMaxTerms; ++k)
      if (k < a.nterm) a.gq[(int64_t)k * tab + idx] = g[k];
  }
};

// semilinear BDF: the BDF scheme with one matrix per level (band_ends [m][2]: step row i has row i) and the law's sums
template <> struct ChunkScheme<TsNlSensArgs> : ChunkScheme<TsSensArgs> {
  static LSSVR_SENS_HD int band_row(const TsNlSensArgs&, int i) { return i; }
  using Gq = ChunkNlGq;
  static LSSVR_SENS_HD double* gq(const TsNlSensArgs& a) { return a.gq; }
};

// Entry idx = e * nquad + k of the tables ga, gc, grho, gd (a scheme with a table d) and gf[r], for the m levels of the
// chunk.  Row i of Z belongs to level n = n0 + m - 1 - i: the rows stand in the order in which the backward sweep
// produced them, n descending.  With xi, om, wh, hw of sens_point, (u0, u1) = u^n[e], u^n[e+1], (r0, r1) and (d0, d1)
// the scheme's pairs of level n and (z0, z1) = Z[i][e], Z[i][e+1], every sum starts from
//   s = accumulate ? what the output holds : 0
// and takes the levels one after the other, i = 0 .. m-1, one rounding per operation:
//   t   = hw (z0 om + z1 xi)
//   sa  = sa - ((wh (z1 - z0)) (u1 - u0))
//   sc  = sc - (t (u0 om + u1 xi))
//   sr  = sr - (t (r0 om + r1 xi))
//   sd  = sd - (t (d0 om + d1 xi))
//   sf_r = sf_r + phi(t_n)[r] t                                     r = 0 .. R-1
//   the scheme's Gq sums with (t, u0 om + u1 xi)                    (a scheme with a law)
// and the sums are stored once.  Because a sum CONTINUES from the stored value, a sweep gives the same bits however it
// is cut into chunks.  A table that is not asked for costs neither arithmetic that only it needs nor a store.
template <class Args> LSSVR_SENS_HD void chunk_sens_entry(const Args& a, const QuadRule& q, int64_t idx) {
  using S = ChunkScheme<Args>;
  const int64_t tab = a.ne * (int64_t)a.nquad, n1 = a.ne + 1;
  const SensPoint p = sens_point(a.x, a.ne, a.nquad, q, idx);
  const int64_t nhi = a.n0 + a.m - 1;
  const bool acc = a.accumulate != 0;
  double* const gd = S::gd(a);
  double* const gq = S::gq(a);
  double sa = acc && a.ga ? a.ga[idx] : 0.0;
  double sc = acc && a.gc ? a.gc[idx] : 0.0;
  double sr = acc && a.grho ? a.grho[idx] : 0.0;
  double sd = acc && gd ? gd[idx] : 0.0;
  double sf[kChunkSensMaxTerms];
#pragma unroll
  for (int r = 0; r < kChunkSensMaxTerms; ++r) sf[r] = acc && a.gf && r < a.R ? a.gf[(int64_t)r * tab + idx] : 0.0;
  typename S::Gq sq;
  if (gq) sq.begin(a, tab, idx, acc);
  S s;
  s.begin(a, p.e, nhi);
  for (int i = 0; i < a.m; ++i) {
    const int64_t n = nhi - i;
    s.load(a, p.e, n);
    const double* z = a.Z + (int64_t)i * n1 + p.e;
    const double z0 = z[0], z1 = z[1];
    const double t = p.hw * (z0 * p.om + z1 * p.xi);
    if (a.ga) sa = sa - ((p.wh * (z1 - z0)) * (s.u1 - s.u0));
    if (a.gc) sc = sc - (t * (s.u0 * p.om + s.u1 * p.xi));
    if (a.grho) {
      double r0, r1;
      s.rho_pair(a, i, r0, r1);
      sr = sr - (t * (r0 * p.om + r1 * p.xi));
    }
    if (gd) {
      double d0, d1;
      s.d_pair(a, d0, d1);
      sd = sd - (t * (d0 * p.om + d1 * p.xi));
    }
    if (a.gf) {
      const double* phi = a.phi + S::phi_row(n) * a.R;
#pragma unroll
      for (int r = 0; r < kChunkSensMaxTerms; ++r)
        if (r < a.R) sf[r] = sf[r] + phi[r] * t;
    }
    if (gq) sq.add(a, t, s.u0 * p.om + s.u1 * p.xi);
    s.next();
  }
  if (a.ga) a.ga[idx] = sa;
  if (a.gc) a.gc[idx] = sc;
  if (a.grho) a.grho[idx] = sr;
  if (gd) gd[idx] = sd;
  if (a.gf) {
#pragma unroll
    for (int r = 0; r < kChunkSensMaxTerms; ++r)
      if (r < a.R) a.gf[(int64_t)r * tab + idx] = sf[r];
  }
  if (gq) sq.store(a, tab, idx);
}

// The end gradients of the chunk: out_g[n][s] of every level n of the chunk, and out_kappa[s] continued from what it
// holds (accumulate) or from 0.  With z = Z[i], B = Brows[i] (the right-hand side of the solve that gave z, natural end
// rows included), u = u^n and (s0, sn) = band_ends[the scheme's row of step row i], the end entries {sub[0], sup[ne-1]}
// of that solve's matrix:
//   Dirichlet end:  out_g[n][0] = B_0 - s0 z_1,   out_g[n][1] = B_ne - sn z_{ne-1};   kappa is left alone
//   Robin end:      out_g[n][s] = z_end;          kappa_s = kappa_s - (z_end u_end),   i = 0 .. m-1 in turn
template <class Args> LSSVR_SENS_HD void chunk_sens_ends(const Args& a) {
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
        a.out_g[2 * n + s] =
            a.Brows[(int64_t)i * n1 + end] - a.band_ends[2 * ChunkScheme<Args>::band_row(a, i) + s] * z[inner];
      }
    }
    a.out_kappa[s] = kap;
  }
}

}  // namespace lssvr
