// A posteriori error indicator and h / hp refinement of the enhanced solution (no reference
// counterpart: Hybrid-FEM-LSSVR-Dual.py computes its per-element slack and discards it).
//   - derivatives of the enhanced solution at query points (lssvr_eval_deriv)
//   - per-element residual indicator  eta_e^2 = h_e^2 ||f + u_e''||_e^2 + h_e/2 (J_e^2 + J_{e+1}^2)
//     with J_i = u_{i-1}'(x_i) - u_i'(x_i) (lssvr_estimate) and its deterministic reduction
//   - the same for -(a u')' = f: residual f + a u'' + a' u', J_i the jump of the flux a u' (lssvr_estimate_varcoef)
//   - the boundary term of a Robin end (lssvr_estimate_ends) and the flux jump across the seam of a
//     periodic domain (lssvr_estimate_seam, section 22): one thread each, in place on eta2 and out3
//   - threshold marking + bisection into a new ascending node array (lssvr_refine), and the same three kernels with
//     the raise-or-bisect rule and the degrees of the new mesh (lssvr_refine_hp)
// The block scan, the per-block reduction tree and its finish kernel are lssvr_adapt.hpp's.
// DESIGN.md section 11 has the derivation, the mapping and the measured numbers.
#include <cmath>
#include <type_traits>

#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_eval.hpp"
#include "lssvr_adapt.hpp"

namespace lssvr {

// ---------------------------------------------------------------------------
// Gauss-Legendre on [-1, 1] (host): Newton on P_nq from the Tricomi-type initial guess, in
// long double, mirrored so that the rule is exactly symmetric.  Ascending nodes.
// ---------------------------------------------------------------------------
bool gauss_rule(int nq, double* xi, double* wt) {
  if (nq < 1 || nq > kAdaptMaxNq) return false;
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int i = 0; i < (nq + 1) / 2; ++i) {
    long double z = std::cos(pi * ((long double)i + 0.75L) / ((long double)nq + 0.5L));  // descending
    long double dp = 1.0L;
    for (int it = 0; it < 100; ++it) {
      long double p0 = 1.0L, p1 = z;
      for (int k = 1; k < nq; ++k) {
        const long double p2 = ((2 * k + 1) * z * p1 - k * p0) / (k + 1);
        p0 = p1;
        p1 = p2;
      }
      dp = nq * (z * p1 - p0) / (z * z - 1.0L);
      const long double dz = p1 / dp;
      z -= dz;
      if (std::fabs(dz) < 1e-19L) break;
    }
    {   // derivative at the converged root, for the weight
      long double p0 = 1.0L, p1 = z;
      for (int k = 1; k < nq; ++k) {
        const long double p2 = ((2 * k + 1) * z * p1 - k * p0) / (k + 1);
        p0 = p1;
        p1 = p2;
      }
      dp = nq * (z * p1 - p0) / (z * z - 1.0L);
    }
    if (2 * i + 1 == nq) z = 0.0L;
    const long double w = 2.0L / ((1.0L - z * z) * dp * dp);
    xi[nq - 1 - i] = (double)z;
    xi[i] = -(double)z;
    wt[i] = wt[nq - 1 - i] = (double)w;
  }
  return true;
}

namespace {

// sum_k c_k P_k^(ORDER)(t), ORDER = 1 or 2, by the forward recurrences
//   P_{k+1} = ((2k+1) t P_k - k P_{k-1}) / (k+1),  P'_{k+1} = P'_{k-1} + (2k+1) P_k,
//   P''_{k+1} = P''_{k-1} + (2k+1) P'_k
template <int ORDER>
__device__ __forceinline__ double legendre_deriv_sum(const double* __restrict__ c, int M, double t) {
  if (M <= ORDER) return 0.0;
  double p0 = 1.0, p1 = t, d0 = 0.0, d1 = 1.0, s0 = 0.0, s1 = 0.0;
  double acc = ORDER == 1 ? c[1] : 0.0;
#pragma unroll 1
  for (int k = 1; k + 1 < M; ++k) {
    const double a = (double)(2 * k + 1);
    const double p2 = (a * t * p1 - (double)k * p0) / (double)(k + 1);
    const double d2 = d0 + a * p1;
    const double s2 = s0 + a * d1;
    acc = fma(c[k + 1], ORDER == 1 ? d2 : s2, acc);
    p0 = p1; p1 = p2;
    d0 = d1; d1 = d2;
    s0 = s1; s1 = s2;
  }
  return acc;
}

template <int ORDER>
__global__ __launch_bounds__(kBlock) void eval_deriv_kernel(const double* __restrict__ x,
                                                             const double* __restrict__ W, int64_t ne,
                                                             int M, const double* __restrict__ xq,
                                                             int64_t P, double* __restrict__ out,
                                                             int64_t* __restrict__ elem) {
  const double x0 = x[0];
  const double inv_h = (double)ne / (x[ne] - x0);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P;
       i += (int64_t)gridDim.x * kBlock) {
    const double xi = xq[i];
    int64_t j = -1;
    double v = 0.0;
    if (xi == xi) {      // NaN: elem -1, value 0 (lssvr_eval's rule)
      j = locate(x, ne, xi, x0, inv_h);
      const DomainMap dm = map_params(x[j], x[j + 1]);
      const double t = dm.off + dm.scl * xi;
      const double s = legendre_deriv_sum<ORDER>(W + j * M, M, t);
      v = ORDER == 1 ? s * dm.scl : s * (dm.scl * dm.scl);
    }
    out[i] = v;
    if (elem) elem[i] = j;
  }
}

// ---------------------------------------------------------------------------
// estimator
// ---------------------------------------------------------------------------
// (chunk geometry kEstBlock / est_blocks / ref_blocks and stage_rows: lssvr_adapt.hpp)
__device__ __forceinline__ double est_point(double a, double b, double xi) {
  const double mid = 0.5 * (a + b);
  const double half = 0.5 * (b - a);
  return mid + half * xi;
}

// (end_derivs, load_row_global, fill_table, neighbour_end and end_jumps: lssvr_adapt.hpp)

// eta2 and the left jump of element e from acc = the Gauss sum of the squared residual on [-1, 1]; the lane's
// running {sum, max, non-finite count}
__device__ __forceinline__ void store_indicator(double* __restrict__ eta2_out, double* __restrict__ jump, int64_t e,
                                                int64_t ne, double h, double acc, double jl, double jr, double& bsum,
                                                double& bmax, double& bcnt) {
  const double half = 0.5 * h;
  const double eta2 = (h * h) * (half * acc) + half * (jl * jl + jr * jr);
  eta2_out[e] = eta2;
  if (jump) {
    jump[e] = jl;
    if (e + 1 == ne) jump[ne] = 0.0;
  }
  if (fabs(eta2) < INFINITY) {
    bsum += eta2;
    bmax = fmax(bmax, eta2);
  } else {
    bcnt += 1.0;
  }
}

// RHS: 0 = LSSVR_RHS_ARRAY (rhs[e*nq + q]), 1 = LSSVR_RHS_SIN, 2 = LSSVR_RHS_ARRAY_PM (rhs[q*ne + e])
// Dynamic LDS: T[nq*MT] (P_k''(xi_q)) | xi[nq] | wt[nq] | rows[kEstBlock*ms] | dl[kEstBlock] | dr[kEstBlock] |
// red[3*kEstBlock].  The rule is copied to LDS: indexed by a loop counter in the kernel arguments it would
// be held in 2*nq*2 VGPRs.
template <int MT, int RHS>
__global__ __launch_bounds__(kEstBlock) void estimate_kernel(EstimateArgs p, GaussRuleN g) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nq = p.nq, M = p.M, ms = p.ms;
  const int64_t ne = p.ne;
  double* T = lds;
  double* sxi = T + nq * MT;
  double* swt = sxi + nq;
  double* rows = swt + nq;
  double* sdl = rows + kEstBlock * ms;
  double* sdr = sdl + kEstBlock;
  double* red = sdr + kEstBlock;
  if (tid < nq) {
    sxi[tid] = g.xi[tid];
    swt[tid] = g.wt[tid];
    fill_table<MT, 1>(T + tid * MT, g.xi[tid], M);
  }
  double bsum = 0.0, bmax = 0.0, bcnt = 0.0;
  for (int64_t c0 = (int64_t)blockIdx.x * kEstBlock; c0 < ne; c0 += (int64_t)gridDim.x * kEstBlock) {
    const int nrow = (int)(ne - c0 < kEstBlock ? ne - c0 : kEstBlock);
    stage_rows(rows, p.W + c0 * M, nrow * M, M, ms, tid);
    __syncthreads();
    const int64_t e = c0 + tid;
    const bool valid = tid < nrow;
    double c[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) c[k] = (valid && k < M) ? rows[tid * ms + k] : 0.0;
    double a = 0.0, b = 1.0;
    if (valid) {
      a = p.x[e];
      b = p.x[e + 1];
    }
    const DomainMap dm = map_params(a, b);
    double dl, dr;
    end_derivs<MT>(c, dm.scl, dl, dr);
    sdl[tid] = dl;
    sdr[tid] = dr;
    __syncthreads();
    if (valid) {
      double jl, jr;
      end_jumps<MT, false>(p.W, p.x, nullptr, e, ne, M, tid, nrow, sdl, sdr, dl, dr, jl, jr);
      // interior residual f + u'' at the nq Gauss points
      const double scl2 = dm.scl * dm.scl;
      double acc = 0.0;
#pragma unroll 1
      for (int q = 0; q < nq; ++q) {
        double s = 0.0;
#pragma unroll
        for (int k = 2; k < MT; ++k) s = fma(c[k], T[q * MT + k], s);
        double f;
        if constexpr (RHS == 1) f = p.rhs_amp * sin_reduced(p.rhs_omega * est_point(a, b, sxi[q]));
        else if constexpr (RHS == 2) f = p.rhs_values[(int64_t)q * ne + e];
        else f = p.rhs_values[e * nq + q];
        const double r = f + s * scl2;
        acc = fma(swt[q], r * r, acc);
      }
      store_indicator(p.eta2, p.jump, e, ne, dm.oldlen, acc, jl, jr, bsum, bmax, bcnt);
    }
    __syncthreads();      // rows / sdl / sdr are rewritten by the next chunk
  }
  reduce_partials<kEstBlock, 3>(red, tid, {bsum, bmax, bcnt}, p.work);
}

// Variable coefficients, -(a u')' = f (TS = 2), and the reaction term, -(a u')' + c u = f (TS = 3, Args =
// EstimateReactArgs): residual f + a u'' + a' u' [- c u] and the jump of the flux a u',
//   J_e = aR_{e-1} u_{e-1}'(x_e) - aL_e u_e'(x_e)   (a_ends[2e] = aL_e, a_ends[2e+1] = aR_e).
// The structure of estimate_kernel: a lane per element, W staged through LDS, the neighbours' end fluxes from
// LDS and recomputed from HBM only at chunk edges (the same products of the same values: bit-identical).
// PM: the a, a', [c,] f tables are point-major t[q*ne + e], else element-major t[e*nq + q].
// Dynamic LDS: T[nq*MT] pairs {P_k'(xi_q), P_k''(xi_q)} or triples {P_k', P_k'', P_k} | wt[nq] | rows[kEstBlock*ms] |
// fl[kEstBlock] | fr[kEstBlock] | red[3*kEstBlock].
template <int MT, bool PM, int TS, typename Args>
__device__ __forceinline__ void estimate_tables_body(const Args& p, const GaussRuleN& g) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nq = p.nq, M = p.M, ms = p.ms;
  const int64_t ne = p.ne;
  double* T = lds;
  double* swt = T + TS * nq * MT;
  double* rows = swt + nq;
  double* sfl = rows + kEstBlock * ms;
  double* sfr = sfl + kEstBlock;
  double* red = sfr + kEstBlock;
  if (tid < nq) {
    swt[tid] = g.wt[tid];
    fill_table<MT, TS>(T + TS * tid * MT, g.xi[tid], M);
  }
  double bsum = 0.0, bmax = 0.0, bcnt = 0.0;
  for (int64_t c0 = (int64_t)blockIdx.x * kEstBlock; c0 < ne; c0 += (int64_t)gridDim.x * kEstBlock) {
    const int nrow = (int)(ne - c0 < kEstBlock ? ne - c0 : kEstBlock);
    stage_rows(rows, p.W + c0 * M, nrow * M, M, ms, tid);
    __syncthreads();
    const int64_t e = c0 + tid;
    const bool valid = tid < nrow;
    double c[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) c[k] = (valid && k < M) ? rows[tid * ms + k] : 0.0;
    double xa = 0.0, xb = 1.0, aL = 0.0, aR = 0.0;
    if (valid) {
      xa = p.x[e];
      xb = p.x[e + 1];
      aL = p.a_ends[2 * e];
      aR = p.a_ends[2 * e + 1];
    }
    const DomainMap dm = map_params(xa, xb);
    double dl, dr;
    end_derivs<MT>(c, dm.scl, dl, dr);
    const double fl = aL * dl, fr = aR * dr;
    sfl[tid] = fl;
    sfr[tid] = fr;
    __syncthreads();
    if (valid) {
      double jl, jr;
      end_jumps<MT, true>(p.W, p.x, p.a_ends, e, ne, M, tid, nrow, sfl, sfr, fl, fr, jl, jr);
      // interior residual at the nq Gauss points
      const double scl2 = dm.scl * dm.scl;
      double acc = 0.0;
#pragma unroll 1
      for (int q = 0; q < nq; ++q) {
        const double* Tq = T + TS * q * MT;
        double s1 = 0.0, s2 = 0.0, s0 = c[0];     // u = sum_k c_k P_k, P_0 = 1
#pragma unroll
        for (int k = 1; k < MT; ++k) {
          s1 = fma(c[k], Tq[TS * k], s1);
          s2 = fma(c[k], Tq[TS * k + 1], s2);
          if constexpr (TS == 3) s0 = fma(c[k], Tq[TS * k + 2], s0);
        }
        const int64_t i = PM ? (int64_t)q * ne + e : e * nq + q;
        double r = p.rhs_values[i] + p.a_values[i] * (s2 * scl2) + p.da_values[i] * (s1 * dm.scl);
        if constexpr (TS == 3) r = r - p.c_values[i] * s0;
        acc = fma(swt[q], r * r, acc);
      }
      store_indicator(p.eta2, p.jump, e, ne, dm.oldlen, acc, jl, jr, bsum, bmax, bcnt);
    }
    __syncthreads();      // rows / sfl / sfr are rewritten by the next chunk
  }
  reduce_partials<kEstBlock, 3>(red, tid, {bsum, bmax, bcnt}, p.work);
}

template <int MT, bool PM>
__global__ __launch_bounds__(kEstBlock) void estimate_vc_kernel(EstimateVcArgs p, GaussRuleN g) {
  estimate_tables_body<MT, PM, 2>(p, g);
}

template <int MT, bool PM>
__global__ __launch_bounds__(kEstBlock) void estimate_react_kernel(EstimateReactArgs p, GaussRuleN g) {
  estimate_tables_body<MT, PM, 3>(p, g);
}

// The boundary term of the indicator at a Robin end a du/dn + kappa u = g, after an estimator
// has written eta2 and out3: with the end element's row,
//   J = g - kappa u_e(x_end) - a du_e/dn,   du_e/dn = -u_e'(x_0) at the left end, +u_e'(x_ne) at the right one,
// eta2[e] += h_e/2 J^2, and out3 follows: sum += the added term, max = max(max, new eta2); a value that stops being
// finite leaves the sum as it is and raises the non-finite count (one that was not finite is already counted).  One
// thread does both ends one after the other -- ne == 1 has them in one element -- so there is no atomic and the
// result is reproducible.  P_k(+-1) = (+-1)^k, P_k'(+-1) = (+-1)^(k+1) k(k+1)/2.
__global__ void estimate_ends_kernel(EstimateEndsArgs p) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double sum = p.out3[0], mx = p.out3[1], cnt = p.out3[2];
  for (int side = 0; side < 2; ++side) {
    if (p.kind[side] != 1) continue;
    const int64_t e = side ? p.ne - 1 : 0;
    const double* c = p.W + e * p.M;
    const DomainMap dm = map_params(p.x[e], p.x[e + 1]);
    double val = 0.0, der = 0.0;
    for (int k = 0; k < p.M; ++k) {
      const double w = (double)(k * (k + 1) / 2);
      const bool flip = side == 0 && (k & 1);          // (-1)^k at the left end
      val = fma(c[k], flip ? -1.0 : 1.0, val);
      der = fma(c[k], (side == 0 && !(k & 1)) ? -w : w, der);
    }
    der *= dm.scl;
    const double dn = side ? der : -der;
    const double J = p.g[side] - p.kappa[side] * val - p.a[side] * dn;
    const double add = (0.5 * dm.oldlen) * (J * J);
    const double old = p.eta2[e];
    const double now = old + add;
    p.eta2[e] = now;
    if (fabs(old) < INFINITY) {
      if (fabs(now) < INFINITY) {
        sum += add;
        mx = fmax(mx, now);
      } else {
        cnt += 1.0;
      }
    }
  }
  p.out3[0] = sum;
  p.out3[1] = mx;
  p.out3[2] = cnt;
}

// The seam term of the indicator on a periodic domain, after an estimator has written eta2 and
// out3 with J_0 = J_ne = 0: node ne is node 0, and the flux jumps across it like across any interior node,
//   J = a[0] u_{ne-1}'(x_ne) - a[1] u_0'(x_0),   eta2[ne-1] += h_{ne-1}/2 J^2,   eta2[0] += h_0/2 J^2,
// with the end derivatives of estimate_ends_kernel; out3 follows as there.  One thread does element ne-1 and then
// element 0 (ne >= 2: two elements), so there is no atomic and the result is reproducible.
__global__ void estimate_seam_kernel(EstimateSeamArgs p) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double sum = p.out3[0], mx = p.out3[1], cnt = p.out3[2];
  double der[2], len[2];                 // side 0: u_0'(x_0), h_0; side 1: u_{ne-1}'(x_ne), h_{ne-1}
  for (int side = 0; side < 2; ++side) {
    const int64_t e = side ? p.ne - 1 : 0;
    const double* c = p.W + e * p.M;
    const DomainMap dm = map_params(p.x[e], p.x[e + 1]);
    double d = 0.0;
    for (int k = 0; k < p.M; ++k) {
      const double w = (double)(k * (k + 1) / 2);
      d = fma(c[k], (side == 0 && !(k & 1)) ? -w : w, d);
    }
    der[side] = d * dm.scl;
    len[side] = dm.oldlen;
  }
  const double J = p.a[0] * der[1] - p.a[1] * der[0];
  for (int side = 1; side >= 0; --side) {
    const int64_t e = side ? p.ne - 1 : 0;
    const double add = (0.5 * len[side]) * (J * J);
    const double old = p.eta2[e];
    const double now = old + add;
    p.eta2[e] = now;
    if (fabs(old) < INFINITY) {
      if (fabs(now) < INFINITY) {
        sum += add;
        mx = fmax(mx, now);
      } else {
        cnt += 1.0;
      }
    }
  }
  p.out3[0] = sum;
  p.out3[1] = mx;
  p.out3[2] = cnt;
}

__global__ __launch_bounds__(kBlock) void estimate_points_kernel(const double* __restrict__ x, int64_t ne,
                                                                  int nq, GaussRuleN g,
                                                                  double* __restrict__ xq) {
  const int64_t total = ne * nq;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t e = i / nq;
    const int q = (int)(i - e * nq);
    xq[i] = est_point(x[e], x[e + 1], g.xi[q]);
  }
}

// ---------------------------------------------------------------------------
// marking + bisection: count per block, one-block scan, scatter.  One text for lssvr_refine (HP = false) and
// lssvr_refine_hp (HP = true): the h instance reads no sigma / deg and writes no deg_new / counts2.
// ---------------------------------------------------------------------------
struct RefineArgs {
  const double* x;
  int64_t ne;
  const double* eta2;
  const double* mx;          // the device max of the finite eta2 (out3[1] of lssvr_estimate)
  double theta2, h2min;
  const double* sigma;       // HP only, from here on
  const int32_t* deg;
  double sigma_min;
  int dM, M_max;
};

// 0: unchanged, 1: bisected, 2: degree raised (HP only).  Element e is marked iff eta2[e] is non-finite, or max > 0
// and eta2[e] >= theta^2 * max; a marked element is raised where its coefficients decay fast enough and the degree
// has room, else bisected where it is at least 2 h_min long
template <bool HP>
__device__ __forceinline__ int action(const RefineArgs& p, int64_t e, double m_max) {
  if (!indicator_marked(p.eta2[e], m_max, p.theta2)) return 0;
  if constexpr (HP) {
    if (p.sigma[e] >= p.sigma_min && (int64_t)p.deg[e] + p.dM <= p.M_max) return 2;      // NaN compares false
  }
  return p.x[e + 1] - p.x[e] >= p.h2min ? 1 : 0;
}

// cnt[block] = bisected | raised << 32 (each at most kBlock; raised = 0 without HP)
template <bool HP>
__global__ __launch_bounds__(kBlock) void refine_count_kernel(RefineArgs p, int64_t* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double m_max = p.mx[0];
  const int act = e < p.ne ? action<HP>(p, e, m_max) : 0;
  int64_t n = __syncthreads_count(act == 1);
  if constexpr (HP) n |= (int64_t)__syncthreads_count(act == 2) << 32;
  if (threadIdx.x == 0) cnt[blockIdx.x] = n;
}

// exclusive offsets of the nb bisected counts, in place: every thread sums a contiguous run of counts, one workgroup
// scan of the 256 run sums, then every thread writes its run's offsets; HP: the two totals to counts2 = {bisected,
// raised}
template <bool HP>
__global__ __launch_bounds__(kBlock) void refine_scan_kernel(int64_t* __restrict__ cnt, int64_t nb, int64_t ne,
                                                              int64_t* __restrict__ ne_new,
                                                              int64_t* __restrict__ counts2) {
  constexpr int NL = HP ? 2 : 1;
  const int tid = threadIdx.x;
  const int64_t per = (nb + kBlock - 1) / kBlock;
  const int64_t lo = tid * per < nb ? tid * per : nb;
  const int64_t hi = lo + per < nb ? lo + per : nb;
  int64_t sum[NL] = {}, total[NL];
  for (int64_t i = lo; i < hi; ++i) {
    sum[0] += cnt[i] & 0xffffffffLL;
    if constexpr (HP) sum[1] += cnt[i] >> 32;
  }
  block_scan<NL>(sum, total);
  int64_t run = sum[0];
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t v = cnt[i] & 0xffffffffLL;
    cnt[i] = run;
    run += v;
  }
  if (tid == kBlock - 1) {
    *ne_new = ne + total[0];
    if constexpr (HP) {
      counts2[0] = total[0];
      counts2[1] = total[1];
    }
  }
}

template <bool HP>
__global__ __launch_bounds__(kBlock) void refine_scatter_kernel(RefineArgs p, const int64_t* __restrict__ offs,
                                                                 double* __restrict__ x_new,
                                                                 int32_t* __restrict__ deg_new,
                                                                 int64_t* __restrict__ parent) {
  __shared__ int wsum[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t e = (int64_t)blockIdx.x * kBlock + tid;
  const double m_max = p.mx[0];
  const int act = e < p.ne ? action<HP>(p, e, m_max) : 0;
  const bool m = act == 1;
  const unsigned long long bal = __ballot(m);
  const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
  if (lane == 0) wsum[wv] = __popcll(bal);
  __syncthreads();
  int before = below;
  for (int w = 0; w < wv; ++w) before += wsum[w];
  if (e < p.ne) {
    const int64_t pos = e + offs[blockIdx.x] + before;
    const double a = p.x[e], b = p.x[e + 1];
    x_new[pos] = a;
    if (parent) parent[pos] = e;
    if (m) {
      x_new[pos + 1] = 0.5 * (a + b);
      if (parent) parent[pos + 1] = e;
    }
    if constexpr (HP) {
      const int32_t d = p.deg[e];
      deg_new[pos] = act == 2 ? d + p.dM : d;
      if (m) deg_new[pos + 1] = d;
    }
    if (e + 1 == p.ne) x_new[pos + 1 + (m ? 1 : 0)] = b;
  }
}

// the three launches of both host entries; work: ref_blocks(ne) int64 counters
template <bool HP>
hipError_t launch_refine(const RefineArgs& p, void* work, double* x_new, int32_t* deg_new, int64_t* parent,
                         int64_t* ne_new, int64_t* counts2, hipStream_t s) {
  const int64_t nb = ref_blocks(p.ne);
  int64_t* cnt = static_cast<int64_t*>(work);
  hipLaunchKernelGGL(refine_count_kernel<HP>, dim3((unsigned)nb), dim3(kBlock), 0, s, p, cnt);
  hipLaunchKernelGGL(refine_scan_kernel<HP>, dim3(1), dim3(kBlock), 0, s, cnt, nb, p.ne, ne_new, counts2);
  hipLaunchKernelGGL(refine_scatter_kernel<HP>, dim3((unsigned)nb), dim3(kBlock), 0, s, p, cnt, x_new, deg_new,
                     parent);
  return hipGetLastError();
}

}  // namespace

int64_t adapt_work_bytes(int64_t ne) {
  const int64_t a = 3 * est_blocks(ne), b = ref_blocks(ne);
  return 8 * (a > b ? a : b);
}

hipError_t eval_deriv(const double* x, const double* W, int64_t ne, int M, int order, const double* xq,
                      int64_t P, double* out, int64_t* elem, hipStream_t s) {
  if (order == 0) return eval_points(x, W, ne, M, xq, P, out, elem, s);   // the same kernel: bit-equal
  if (P == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((P + kBlock - 1) / kBlock < 16384 ? (P + kBlock - 1) / kBlock : 16384);
  if (order == 1)
    hipLaunchKernelGGL(eval_deriv_kernel<1>, dim3(blocks), dim3(kBlock), 0, s, x, W, ne, M, xq, P, out, elem);
  else
    hipLaunchKernelGGL(eval_deriv_kernel<2>, dim3(blocks), dim3(kBlock), 0, s, x, W, ne, M, xq, P, out, elem);
  return hipGetLastError();
}

hipError_t estimate_points(const double* x, int64_t ne, int nq, double* xq, hipStream_t s) {
  GaussRuleN g{};
  if (!gauss_rule(nq, g.xi, g.wt)) return hipErrorInvalidValue;
  if (ne == 0) return hipSuccess;
  const int64_t total = ne * nq;
  const unsigned blocks = (unsigned)((total + kBlock - 1) / kBlock < 8192 ? (total + kBlock - 1) / kBlock : 8192);
  hipLaunchKernelGGL(estimate_points_kernel, dim3(blocks), dim3(kBlock), 0, s, x, ne, nq, g, xq);
  return hipGetLastError();
}

// the host path the three estimators share: `pick(std::integral_constant<int, MT>)` names the kernel of the row
// bucket MT; its LDS coefficient table holds tab_rows * MT + tab_extra doubles per quadrature point
template <typename Args, typename Pick>
static hipError_t launch_estimate_any(Args a, int tab_rows, int tab_extra, double* out3, hipStream_t s, Pick pick) {
  GaussRuleN g{};
  if (!gauss_rule(a.nq, g.xi, g.wt)) return hipErrorInvalidValue;
  a.ms = a.M | 1;                                   // odd row stride: conflict-free ds_read_b64
  const int64_t nb = est_blocks(a.ne);
  const int MT = a.M <= 12 ? 12 : (a.M <= 22 ? 22 : 33);
  const size_t lds =
      sizeof(double) * ((size_t)a.nq * (tab_rows * MT + tab_extra) + (size_t)kEstBlock * a.ms + 5 * kEstBlock);
  void (*kernel)(Args, GaussRuleN);
  if (MT == 12) kernel = pick(std::integral_constant<int, 12>{});
  else if (MT == 22) kernel = pick(std::integral_constant<int, 22>{});
  else kernel = pick(std::integral_constant<int, 33>{});
  hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(kEstBlock), lds, s, a, g);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(finish_kernel<3>, dim3(1), dim3(kBlock), 0, s, a.work, (int)nb, out3);
  return hipGetLastError();
}

hipError_t estimate(EstimateArgs a, int rhs_mode, double* out3, hipStream_t s) {
  return launch_estimate_any(a, 1, 2, out3, s, [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    return rhs_mode == 1 ? estimate_kernel<MT, 1> : rhs_mode == 2 ? estimate_kernel<MT, 2> : estimate_kernel<MT, 0>;
  });
}

hipError_t estimate_varcoef(EstimateVcArgs a, bool point_major, double* out3, hipStream_t s) {
  return launch_estimate_any(a, 2, 1, out3, s, [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    return point_major ? estimate_vc_kernel<MT, true> : estimate_vc_kernel<MT, false>;
  });
}

hipError_t estimate_react(EstimateReactArgs a, bool point_major, double* out3, hipStream_t s) {
  return launch_estimate_any(a, 3, 1, out3, s, [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    return point_major ? estimate_react_kernel<MT, true> : estimate_react_kernel<MT, false>;
  });
}

hipError_t estimate_ends(const EstimateEndsArgs& a, hipStream_t s) {
  if (a.kind[0] != 1 && a.kind[1] != 1) return hipSuccess;       // two Dirichlet ends: nothing is added
  hipLaunchKernelGGL(estimate_ends_kernel, dim3(1), dim3(1), 0, s, a);
  return hipGetLastError();
}

hipError_t estimate_seam(const EstimateSeamArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(estimate_seam_kernel, dim3(1), dim3(1), 0, s, a);
  return hipGetLastError();
}

hipError_t refine(const double* x, int64_t ne, const double* eta2, const double* eta2_max, double theta,
                  double h_min, void* work, double* x_new, int64_t* parent, int64_t* ne_new, hipStream_t s) {
  const RefineArgs p{x, ne, eta2, eta2_max, theta * theta, 2.0 * h_min, nullptr, nullptr, 0.0, 0, 0};
  return launch_refine<false>(p, work, x_new, nullptr, parent, ne_new, nullptr, s);
}

hipError_t refine_hp(const double* x, int64_t ne, const double* eta2, const double* eta2_max, double theta,
                     double h_min, const double* sigma, const int32_t* deg, double sigma_min, int dM, int M_max,
                     void* work, double* x_new, int32_t* deg_new, int64_t* parent, int64_t* ne_new, int64_t* counts2,
                     hipStream_t s) {
  const RefineArgs p{x, ne, eta2, eta2_max, theta * theta, 2.0 * h_min, sigma, deg, sigma_min, dM, M_max};
  return launch_refine<true>(p, work, x_new, deg_new, parent, ne_new, counts2, s);
}

}  // namespace lssvr
