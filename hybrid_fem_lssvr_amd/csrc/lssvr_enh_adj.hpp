// The routines behind every value of enhance_adjoint*.hip: the device kernel and the host mirror
// call enh_adj_element / enh_adj_gather, and with -ffp-contract=off they are bit-equal.  NOTHING here is an fma, a
// hardware reciprocal or a library call: every operation is one IEEE rounding, in the order that
// scripts/proto/enhance_adjoint_proto.py::kernel_adjoint restates in numpy.  (The forward lane kernel's recurrences are
// written with fma and its reciprocals with a Newton step; this header carries its own plain copies.)
//
// One element, given Wbar = dJ/dW of its row (notation of oracle/lssvr_oracle.py::solve_bc_eliminated):
//   pass 1 over the points:  rows Abar_k = Ahat2_k - Ahat1_k C,  S = sum_k Abar_k Abar_k^T + eps (I + C^T C)   (direct Gram)
//   LDL^T of S (no square roots), y = S^-1 (Wbar_2 - C^T Wbar_1),  yh = (-C y, y)
//   pass 2 over the points:  the six evaluations (L, D1, D2) . (yh, w),  q_k = Ahat_k yh,  e_k = ftil_k - Ahat_k w,
//                            the table rows, and t = Ahat1^T q
//   (gl, gr) = B1^-T (Wbar_1 + eps C y - t)
// Ahat_k = -a_k D2 - (da_k / scl) D1 + (c_k / scl^2) L has the columns Ahat_k[0] = c_k / scl^2 and
// Ahat_k[1] = (c_k / scl^2) t_k - da_k / scl (L_0 = 1, L_1 = t), so q_k and Ahat_k w come from the six evaluations and
// the row itself is needed in pass 1 only.
#pragma once
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

#define LSSVR_EA_HD __host__ __device__ __forceinline__

namespace lssvr {

// points per staging round of the device kernel (the host mirror reads and writes memory directly)
constexpr int kEaStageK = 8;
constexpr int kEaStageArr = 64 * (kEaStageK + 1);
constexpr int kEaTilePerWave = 4 * kEaStageArr;          // f, a, da, c in; gf, ga, gda, gc out, in place
static_assert(kEaTilePerWave >= 64 * kEnhAdjMaxM, "the W / Wbar tile of a wave goes through the same area");

// L_p(t), p < M:  (p+1) L_{p+1} = (2p+1) t L_p - p L_{p-1}
template <int M>
LSSVR_EA_HD void ea_legendre_p(double t, double (&L)[M]) {
  L[0] = 1.0;
  L[1] = t;
#pragma unroll
  for (int p = 1; p < M - 1; ++p) {
    const double al = (double)(2 * p + 1) / (double)(p + 1);
    const double be = (double)p / (double)(p + 1);
    L[p + 1] = (al * t) * L[p] - be * L[p - 1];
  }
}

// D1[p] = L'_p(t), p < M:  r_m = L'_{m+1},  r_0 = 1, r_1 = 3 t,  m r_m = (2m+1) t r_{m-1} - (m+1) r_{m-2}
template <int M>
LSSVR_EA_HD void ea_legendre_d1(double t, double (&D1)[M]) {
  D1[0] = 0.0;
  D1[1] = 1.0;
  if constexpr (M > 2) D1[2] = 3.0 * t;
#pragma unroll
  for (int m = 2; m < M - 1; ++m) {
    const double al = (double)(2 * m + 1) / (double)m;
    const double be = (double)(m + 1) / (double)m;
    D1[m + 1] = (al * t) * D1[m] - be * D1[m - 1];
  }
}

// D2[p] = L''_p(t), p < M:  q_m = L''_{m+2},  q_0 = 3, q_1 = 15 t,  m q_m = (2m+3) t q_{m-1} - (m+3) q_{m-2}
template <int M>
LSSVR_EA_HD void ea_legendre_d2(double t, double (&D2)[M]) {
  D2[0] = 0.0;
  D2[1] = 0.0;
  if constexpr (M > 2) D2[2] = 3.0;
  if constexpr (M > 3) D2[3] = 15.0 * t;
#pragma unroll
  for (int m = 2; m < M - 2; ++m) {
    const double al = (double)(2 * m + 3) / (double)m;
    const double be = (double)(m + 3) / (double)m;
    D2[m + 2] = (al * t) * D2[m + 1] - be * D2[m];
  }
}

// sum_{p >= FIRST} T[p] v[p], from 0.0, in the order of p
template <int FIRST, int M>
LSSVR_EA_HD double ea_dot(const double (&T)[M], const double (&v)[M]) {
  double s = 0.0;
#pragma unroll
  for (int p = FIRST; p < M; ++p) s = s + T[p] * v[p];
  return s;
}

// np.linspace(a, b, n)[k] (lssvr_device.hpp::linspace_at, host and device)
LSSVR_EA_HD double ea_linspace_at(double a, double b, double delta, double step, int k, int n) {
  if (k == n - 1) return b;
  const double y = (step == 0.0) ? ((double)k / (double)(n - 1)) * delta : (double)k * step;
  return y + a;
}

// The host mirror's view of the tables and rows: memory itself.  The device kernel (enhance_adjoint_impl.hpp) hands
// enh_adj_element a view with the same five members that goes through the wave's LDS area.
struct EaHostIO {
  const EnhAdjArgs& p;
  int64_t e;
  LSSVR_EA_HD void stage_in(int, bool) {}
  LSSVR_EA_HD void stage_out(int) {}
  LSSVR_EA_HD void in(int k, bool with_f, double& f, double& a, double& da, double& c) const {
    const int64_t g = e * p.n + k;
    f = with_f ? p.rhs_values[g] : 0.0;
    a = p.a_values ? p.a_values[g] : 1.0;
    da = p.da_values ? p.da_values[g] : 0.0;
    c = p.c_values ? p.c_values[g] : 0.0;
  }
  LSSVR_EA_HD void out(int k, double ga, double gda, double gc, double gf) const {
    const int64_t g = e * p.n + k;
    if (p.ga) p.ga[g] = ga;
    if (p.gda) p.gda[g] = gda;
    if (p.gc) p.gc[g] = gc;
    if (p.gf) p.gf[g] = gf;
  }
  template <int M>
  LSSVR_EA_HD void rows(double (&w)[M], double (&wb)[M]) const {
    for (int i = 0; i < M; ++i) {
      w[i] = p.W[e * M + i];
      wb[i] = p.Wbar[e * M + i];
    }
  }
};

// Element `ec` of the launch -> (gl, gr), and its rows of the tables that are asked for through io.out.  Every lane of a
// wave makes the same io calls (the loops run to p.n for every element, a fallback element included: its values are
// replaced at the end), so a view may load and store cooperatively.
template <int M, class IO>
LSSVR_EA_HD void enh_adj_element(const EnhAdjArgs& p, int64_t ec, IO& io, double& gl, double& gr) {
  constexpr int MR = M - 2;
  constexpr int NT = MR * (MR + 1) / 2;
  const int n = p.n;
  const double xa = p.x[ec], xb = p.x[ec + 1];
  const bool fb = p.status && p.status[ec] == LSSVR_ST_FALLBACK;
  const double oldlen = xb - xa;
  const double off = (-xb - xa) / oldlen;
  const double scl = 2.0 / oldlen;
  const double step = oldlen / (double)(n - 1);
  const double scl2 = scl * scl;
  const double inv_scl2 = 1.0 / scl2;
  const double eps = 1.0 / (p.gamma * (scl2 * scl2));
  const double hs = 0.5 * oldlen;                       // 1 / scl
  const double ta = off + scl * xa, tb = off + scl * xb;
  const double idet = 1.0 / (tb - ta);
  double C0[MR], C1[MR];
  {
    double La[M], Lb[M];
    ea_legendre_p<M>(ta, La);
    ea_legendre_p<M>(tb, Lb);
#pragma unroll
    for (int j = 0; j < MR; ++j) {
      C0[j] = (tb * La[j + 2] - ta * Lb[j + 2]) * idet;
      C1[j] = (Lb[j + 2] - La[j + 2]) * idet;
    }
  }

  // ---- pass 1: S = sum_k Abar_k Abar_k^T, packed lower triangle ---------------------------------------------------
  double S[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) S[i] = 0.0;
  for (int k = 0; k < n; ++k) {
    if ((k & (kEaStageK - 1)) == 0) io.stage_in(k, false);
    double fk, ak, dak, ck;
    io.in(k, false, fk, ak, dak, ck);
    const double t = off + scl * ea_linspace_at(xa, xb, oldlen, step, k, n);
    const double bk = dak * hs, cs = ck * inv_scl2;
    double L[M], D1[M], D2[M], Ab[MR];
    ea_legendre_p<M>(t, L);
    ea_legendre_d1<M>(t, D1);
    ea_legendre_d2<M>(t, D2);
    const double A0 = cs, A1 = cs * t - bk;
#pragma unroll
    for (int j = 0; j < MR; ++j)
      Ab[j] = ((cs * L[j + 2] - bk * D1[j + 2]) - ak * D2[j + 2]) - (A0 * C0[j] + A1 * C1[j]);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) S[tri(i, j)] = S[tri(i, j)] + Ab[i] * Ab[j];
  }
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double cc = C0[i] * C0[j] + C1[i] * C1[j];
      if (i == j) cc = cc + 1.0;
      S[tri(i, j)] = S[tri(i, j)] + eps * cc;
    }
  // ---- LDL^T in place: unit L below the diagonal, the diagonal holds 1 / d_j ------------------------------------------
#pragma unroll
  for (int j = 0; j < MR; ++j) {
    const double rinv = 1.0 / S[tri(j, j)];
    S[tri(j, j)] = rinv;
#pragma unroll
    for (int c = j + 1; c < MR; ++c) {
      const double lcj = S[tri(c, j)] * rinv;
#pragma unroll
      for (int i = c; i < MR; ++i) S[tri(i, c)] = S[tri(i, c)] - S[tri(i, j)] * lcj;
      S[tri(c, j)] = lcj;
    }
  }
  // ---- y = S^-1 (Wbar_2 - C^T Wbar_1),  yh = (-C y, y) ---------------------------------------------------------------
  double w[M], wb[M], yh[M];
  io.template rows<M>(w, wb);
#pragma unroll
  for (int j = 0; j < MR; ++j) yh[j + 2] = wb[j + 2] - (C0[j] * wb[0] + C1[j] * wb[1]);
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    double s = yh[i + 2];
#pragma unroll
    for (int j = 0; j < i; ++j) s = s - S[tri(i, j)] * yh[j + 2];
    yh[i + 2] = s;
  }
#pragma unroll
  for (int i = MR - 1; i >= 0; --i) {
    double s = yh[i + 2] * S[tri(i, i)];
#pragma unroll
    for (int j = i + 1; j < MR; ++j) s = s - S[tri(j, i)] * yh[j + 2];
    yh[i + 2] = s;
  }
  yh[0] = 0.0;
  yh[1] = 0.0;
#pragma unroll
  for (int j = 0; j < MR; ++j) {
    yh[0] = yh[0] - C0[j] * yh[j + 2];
    yh[1] = yh[1] - C1[j] * yh[j + 2];
  }

  // ---- pass 2: q_k, e_k, the table rows, t = Ahat1^T q -------------------------------------------------------------
  const bool tables = p.ga || p.gda || p.gc || p.gf;
  double t0 = 0.0, t1 = 0.0;
  for (int k = 0; k < n; ++k) {
    if ((k & (kEaStageK - 1)) == 0) io.stage_in(k, tables);
    double fk, ak, dak, ck;
    io.in(k, tables, fk, ak, dak, ck);
    const double t = off + scl * ea_linspace_at(xa, xb, oldlen, step, k, n);
    const double bk = dak * hs, cs = ck * inv_scl2;
    double L[M], D1[M], D2[M];
    ea_legendre_p<M>(t, L);
    ea_legendre_d1<M>(t, D1);
    ea_legendre_d2<M>(t, D2);
    const double Ly = ea_dot<0, M>(L, yh), D1y = ea_dot<1, M>(D1, yh), D2y = ea_dot<2, M>(D2, yh);
    const double q = (cs * Ly - bk * D1y) - ak * D2y;
    t0 = t0 + cs * q;
    t1 = t1 + (cs * t - bk) * q;
    if (tables) {
      double va = 0.0, vda = 0.0, vc = 0.0;
      const double vf = fb ? 0.0 : q * inv_scl2;
      if (p.ga || p.gda || p.gc) {
        const double Lw = ea_dot<0, M>(L, w), D1w = ea_dot<1, M>(D1, w), D2w = ea_dot<2, M>(D2, w);
        const double e = fk * inv_scl2 - ((cs * Lw - bk * D1w) - ak * D2w);
        if (p.ga) va = fb ? 0.0 : -(e * D2y - q * D2w);
        if (p.gda) vda = fb ? 0.0 : -((e * D1y - q * D1w) * hs);
        if (p.gc) vc = fb ? 0.0 : (e * Ly - q * Lw) * inv_scl2;
      }
      io.out(k, va, vda, vc, vf);
      if ((k & (kEaStageK - 1)) == kEaStageK - 1 || k == n - 1) io.stage_out(k & ~(kEaStageK - 1));
    }
  }
  const double z0 = (wb[0] - eps * yh[0]) - t0;
  const double z1 = (wb[1] - eps * yh[1]) - t1;
  gl = fb ? 0.5 * (wb[0] - wb[1]) : (tb * z0 - z1) * idet;
  gr = fb ? 0.5 * (wb[0] + wb[1]) : (z1 - ta * z0) * idet;
}

// Node i of the launch: gu_i = gr(element i-1) + gl(element i), the left element's term first.  Where the forward call
// replaced the nodal value by the Dirichlet value (oracle/lssvr_oracle.py::boundary_values, the comparison of the forward
// kernels) the end's term goes to gbc[side] and gu gets 0; gbc of an end that is not replaced is 0.
LSSVR_EA_HD void enh_adj_gather(const EnhAdjArgs& p, int64_t i) {
  const double* pr = p.pairs;
  double v = i == 0 ? pr[0] : (i == p.ne ? pr[2 * (p.ne - 1) + 1] : pr[2 * (i - 1) + 1] + pr[2 * i]);
  if (i == 0) {
    const bool rep = p.elem_offset == 0 && p.x[0] == p.gxmin;
    if (p.gbc) p.gbc[0] = rep ? v : 0.0;
    if (rep) v = 0.0;
  }
  if (i == p.ne) {
    const bool rep = p.elem_offset + p.ne == p.ne_global && p.x[p.ne] == p.gxmax;
    if (p.gbc) p.gbc[1] = rep ? v : 0.0;
    if (rep) v = 0.0;
  }
  if (p.gu) p.gu[i] = v;
}

}  // namespace lssvr
