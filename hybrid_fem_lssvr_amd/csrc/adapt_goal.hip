// Goal-oriented error estimation (dual-weighted residual; no reference counterpart): the
// residual of the enhanced primal solution u_e (row e of Wu), weighted with the enhanced dual solution z_e (row e of
// Wz), for a quantity of interest J(u) = int j u dx of -(a u')' + c u = f:
//   eta_e = int_e R z_e dx - 1/2 (J_e z_e(x_e) + J_{e+1} z_e(x_{e+1}))
//           [+ (g - kappa u_e - a du_e/dn) z_e at a Robin end]
//   R = f + a u_e'' + a' u_e' - c u_e,   J_i = aR_{i-1} u_{i-1}'(x_i) - aL_i u_i'(x_i)   (J_0 = J_ne = 0)
// signed, with eta_e^2 for the marking of lssvr_refine and q_e = int_e j u_e dx, so that sum eta_e + sum q_e is the
// corrected value of J.  The structure of adapt.hip's estimate_tables_body: a lane per element, both row sets staged
// through LDS at the odd stride, the neighbours' end fluxes from LDS and recomputed from HBM only at chunk edges, the
// per-block tree and the one-workgroup finish of lssvr_adapt.hpp (four slots); no atomics, every output bitwise
// reproducible.
#include <cmath>
#include <type_traits>

#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_adapt.hpp"

namespace lssvr {

// One wave per chunk: two row sets of kEstBlock rows at ldw = 33 and the table of 32 points do not fit 64 KiB of LDS
// (97 KiB); with 64 rows the largest launch (M = 33, nq = 32) takes 61 KiB.
constexpr int kGoalBlock = 64;

static int64_t goal_blocks(int64_t ne) { return chunk_blocks<kGoalBlock>(ne); }

int64_t goal_work_bytes(int64_t ne) { return 8 * 4 * goal_blocks(ne); }

namespace {

// sum_k c_k (+-1)^k = the element's value at its left (side 0) or right (side 1) end, P_k(+-1) = (+-1)^k
template <int MT>
__device__ __forceinline__ double end_value(const double (&c)[MT], int side) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < MT; ++k) s = fma(c[k], (side == 0 && (k & 1)) ? -1.0 : 1.0, s);
  return s;
}

// PM: the a, a', [c,] f, j tables are point-major t[q*ne + e], else element-major t[e*nq + q]; REACT: c_values given.
// Dynamic LDS: T[nq*MT] triples {P_k', P_k'', P_k}(xi_q) | wt[nq] | rowsU[kGoalBlock*ms] | rowsZ[kGoalBlock*ms] |
// fl[kGoalBlock] | fr[kGoalBlock] | red[4*kGoalBlock].
template <int MT, bool PM, bool REACT>
__global__ __launch_bounds__(kGoalBlock) void estimate_goal_kernel(GoalArgs p, GaussRuleN g) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nq = p.nq, M = p.M, ms = p.ms;
  const int64_t ne = p.ne;
  double* T = lds;
  double* swt = T + 3 * nq * MT;
  double* rows_u = swt + nq;
  double* rows_z = rows_u + kGoalBlock * ms;
  double* sfl = rows_z + kGoalBlock * ms;
  double* sfr = sfl + kGoalBlock;
  double* red = sfr + kGoalBlock;
  if (tid < nq) {
    swt[tid] = g.wt[tid];
    fill_table<MT, 3>(T + 3 * tid * MT, g.xi[tid], M);
  }
  double bsum = 0.0, bmax = 0.0, bcnt = 0.0, bq = 0.0;
  for (int64_t c0 = (int64_t)blockIdx.x * kGoalBlock; c0 < ne; c0 += (int64_t)gridDim.x * kGoalBlock) {
    const int nrow = (int)(ne - c0 < kGoalBlock ? ne - c0 : kGoalBlock);
    stage_rows<kGoalBlock>(rows_u, p.Wu + c0 * M, nrow * M, M, ms, tid);
    stage_rows<kGoalBlock>(rows_z, p.Wz + c0 * M, nrow * M, M, ms, tid);
    __syncthreads();
    const int64_t e = c0 + tid;
    const bool valid = tid < nrow;
    double c[MT], z[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      c[k] = (valid && k < M) ? rows_u[tid * ms + k] : 0.0;
      z[k] = (valid && k < M) ? rows_z[tid * ms + k] : 0.0;
    }
    double xa = 0.0, xb = 1.0, aL = 0.0, aR = 0.0;
    if (valid) {
      xa = p.x[e];
      xb = p.x[e + 1];
      aL = p.a_ends[2 * e];
      aR = p.a_ends[2 * e + 1];
    }
    const DomainMap dm = map_params(xa, xb);
    double zl = end_value<MT>(z, 0), zr = end_value<MT>(z, 1);
    if (p.jump_free) {
      // weight with z_e - I_h z_e, I_h the linear interpolant of z_e at the element's two nodes (P_0 = 1, P_1 = t):
      // the weight vanishes at the nodes, so the jump and end terms drop out and eta_e is the element's own
      // interior term -- what a bisection of THIS element can reduce
      z[0] -= 0.5 * (zl + zr);
      z[1] -= 0.5 * (zr - zl);
      zl = zr = 0.0;
    }
    double dl, dr;
    end_derivs<MT>(c, dm.scl, dl, dr);
    const double fl = aL * dl, fr = aR * dr;
    sfl[tid] = fl;
    sfr[tid] = fr;
    __syncthreads();
    if (valid) {
      double jl, jr;
      end_jumps<MT, true>(p.Wu, p.x, p.a_ends, e, ne, M, tid, nrow, sfl, sfr, fl, fr, jl, jr);
      // int_e R z and int_e j u at the nq Gauss points
      const double scl2 = dm.scl * dm.scl;
      double acc = 0.0, qacc = 0.0;
#pragma unroll 1
      for (int q = 0; q < nq; ++q) {
        const double* Tq = T + 3 * q * MT;
        double s1 = 0.0, s2 = 0.0, s0 = c[0], zq = z[0];     // u = sum_k c_k P_k, P_0 = 1
#pragma unroll
        for (int k = 1; k < MT; ++k) {
          s1 = fma(c[k], Tq[3 * k], s1);
          s2 = fma(c[k], Tq[3 * k + 1], s2);
          s0 = fma(c[k], Tq[3 * k + 2], s0);
          zq = fma(z[k], Tq[3 * k + 2], zq);
        }
        const int64_t i = PM ? (int64_t)q * ne + e : e * nq + q;
        double r = p.rhs_values[i] + p.a_values[i] * (s2 * scl2) + p.da_values[i] * (s1 * dm.scl);
        if constexpr (REACT) r = r - p.c_values[i] * s0;
        acc = fma(swt[q], r * zq, acc);
        qacc = fma(swt[q], p.goal_values[i] * s0, qacc);
      }
      const double half = 0.5 * dm.oldlen;
      double eta = half * acc - 0.5 * (jl * zl + jr * zr);
      // a Robin end a du/dn + kappa u = g: (g - kappa u_e(x_end) - a du_e/dn) z_e(x_end), du_e/dn = -u_e' at the left
      // end and +u_e' at the right one; ne == 1 has both in this element.  Added here, before eta^2 and the
      // reduction: a signed term can lower eta^2, so a max taken before it could not be mended afterwards.
      if (e == 0 && p.kind[0] == 1) eta += (p.g[0] - p.kappa[0] * end_value<MT>(c, 0) - p.a_bnd[0] * (-dl)) * zl;
      if (e + 1 == ne && p.kind[1] == 1) eta += (p.g[1] - p.kappa[1] * end_value<MT>(c, 1) - p.a_bnd[1] * dr) * zr;
      const double eta2 = eta * eta;
      const double qe = half * qacc;
      p.eta[e] = eta;
      p.eta2[e] = eta2;
      if (p.q) p.q[e] = qe;
      if (fabs(eta2) < INFINITY) {        // (an eta whose square overflows cannot be marked by its size either)
        bsum += eta;
        bmax = fmax(bmax, eta2);
      } else {
        bcnt += 1.0;
      }
      if (fabs(qe) < INFINITY) bq += qe;
    }
    __syncthreads();      // rows / sfl / sfr are rewritten by the next chunk
  }
  // the per-lane {sum eta, max eta^2, non-finite count, sum q} -> work[4*blockIdx.x ..]
  reduce_partials<kGoalBlock, 4>(red, tid, {bsum, bmax, bcnt, bq}, p.work);
}

template <int MT>
void (*pick_goal(bool pm, bool react))(GoalArgs, GaussRuleN) {
  if (pm) return react ? estimate_goal_kernel<MT, true, true> : estimate_goal_kernel<MT, true, false>;
  return react ? estimate_goal_kernel<MT, false, true> : estimate_goal_kernel<MT, false, false>;
}

}  // namespace

hipError_t estimate_goal(GoalArgs a, bool point_major, double* out4, hipStream_t s) {
  GaussRuleN g{};
  if (!gauss_rule(a.nq, g.xi, g.wt)) return hipErrorInvalidValue;
  a.ms = a.M | 1;                                   // odd row stride: conflict-free ds_read_b64
  const int64_t nb = goal_blocks(a.ne);
  const int MT = a.M <= 12 ? 12 : (a.M <= 22 ? 22 : 33);
  const size_t lds =
      sizeof(double) * ((size_t)a.nq * (3 * MT + 1) + (size_t)2 * kGoalBlock * a.ms + 6 * kGoalBlock);
  const bool react = a.c_values != nullptr;
  void (*kernel)(GoalArgs, GaussRuleN) = MT == 12   ? pick_goal<12>(point_major, react)
                                         : MT == 22 ? pick_goal<22>(point_major, react)
                                                    : pick_goal<33>(point_major, react);
  hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(kGoalBlock), lds, s, a, g);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(finish_kernel<4>, dim3(1), dim3(kBlock), 0, s, a.work, (int)nb, out4);
  return hipGetLastError();
}

}  // namespace lssvr
