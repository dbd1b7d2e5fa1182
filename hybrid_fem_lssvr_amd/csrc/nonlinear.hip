// Semilinear problems  -(a u')' + b u' + c u + g(x, u) = f  on the P1 mesh by a damped Newton iteration (DESIGN.md
// section 27).  A Newton step is the LINEAR problem with the reaction c + g_u(x, u_h) and the right-hand side
// f - g(x, u_h) + g_u(x, u_h) u_h, u_h the P1 interpolant of the iterate: the assembly and the solves are the entries
// that exist.  This file adds what goes around them:
//   linearize   the tables c_eff, f_eff and f_res at any set of points of the elements (one kernel for the quadrature
//               points of the assembly, the collocation points and the Gauss points of the indicator)
//   residual    the four numbers the loop reads per trial point: max |K u + ends - load|, max |u_new - u|, max |u_new|
//               and the count of non-finite entries -- per-block partials, then a one-block finish; no atomics
//   step        out = u + lambda (u_new - u), the trial point of the line search
// g comes from a tabulated family: POLY  g = sum_k q_k(x) u^k  (Horner) and EXP  g = q_0(x) exp(q_1(x) u).
// No atomics, no LDS for the tables, no scratch; every value comes from one inline routine that the host mirrors
// (lssvr_nl_*_host) call too: with -ffp-contract=off the two are bit-equal, except for exp, which is libm on the host
// and the device library's on the GPU.
// FP64, -ffp-contract=off.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_nl_family.hpp"

#include <cmath>

#define LSSVR_NL_HD __host__ __device__ __forceinline__

namespace lssvr {

namespace {

// threads per workgroup (four waves) and the grid cap of the grid-stride loops
constexpr int kNlBlock = 256;
constexpr int kNlMaxBlocks = 1024;

int64_t nl_blocks(int64_t n) {
  const int64_t b = (n + kNlBlock - 1) / kNlBlock;
  return b < 1 ? 1 : (b < kNlMaxBlocks ? b : kNlMaxBlocks);
}

// Entry (e, k) of the tables, idx its position in memory.  The order of every sum:
//   u_h    = u_e + (u_{e+1} - u_e) t_k
//   g, d   = g and g_u of the family at (point, u_h): nl_family (lssvr_nl_family.hpp)
//   c_eff  = c + d  (no c_tab: c = 0);   f_eff = (f - g) + d u_h;   f_res = f - g
LSSVR_NL_HD void nl_entry(const NlLinArgs& a, int64_t e, int k, int64_t idx) {
  const int64_t tab = a.ne * (int64_t)a.n;
  const double u0 = a.u[e];
  const double uh = u0 + (a.u[e + 1] - u0) * a.t_local[k];
  double g, d;
  nl_family(a.kind, a.nterm, a.q_tabs, tab, idx, uh, g, d);
  const double fr = a.f_tab[idx] - g;
  if (a.c_eff) a.c_eff[idx] = (a.c_tab ? a.c_tab[idx] : 0.0) + d;
  if (a.f_eff) a.f_eff[idx] = fr + d * uh;
  if (a.f_res) a.f_res[idx] = fr;
}

// idx runs over the table in memory order, so both layouts are read and written coalesced
LSSVR_NL_HD void nl_entry_at(const NlLinArgs& a, bool point_major, int64_t idx) {
  int64_t e;
  int k;
  if (point_major) {
    k = (int)(idx / a.ne);
    e = idx - (int64_t)k * a.ne;
  } else {
    e = idx / a.n;
    k = (int)(idx - e * a.n);
  }
  nl_entry(a, e, k, idx);
}

template <bool PM>
__global__ __launch_bounds__(kNlBlock) void nl_linearize_kernel(NlLinArgs a) {
  const int64_t tab = a.ne * (int64_t)a.n, stride = (int64_t)gridDim.x * kNlBlock;
  for (int64_t idx = (int64_t)blockIdx.x * kNlBlock + threadIdx.x; idx < tab; idx += stride)
    nl_entry_at(a, PM, idx);
}

// The four numbers of the residual as they are accumulated: three maxima of absolute values and a count.  A value
// that is not finite raises the count and joins no maximum, so the maxima are those of finite numbers >= 0: they do
// not depend on the order, and the count is a sum of integers (held in a double: exact below 2^53).
struct NlAcc {
  double r, du, un, bad;
};

LSSVR_NL_HD void nl_take(double v, double& m, double& bad) {
  const double av = fabs(v);
  if (!(av < INFINITY))
    bad = bad + 1.0;
  else if (av > m)
    m = av;
}

LSSVR_NL_HD void nl_merge(NlAcc& s, const NlAcc& o) {
  if (o.r > s.r) s.r = o.r;
  if (o.du > s.du) s.du = o.du;
  if (o.un > s.un) s.un = o.un;
  s.bad = s.bad + o.bad;
}

// Row i.  The order of every sum:
//   r_i = ((sub[i-1] u[i-1] + diag[i] u[i]) + sup[i] u[i+1]) - load[i]      (rows 0 and ne: the term of the missing
//                                                                             neighbour is left out, not added as 0)
//   a Robin end row:  r_i = r_i + (kappa u_i - g);   a Dirichlet end row:  r_i = 0
LSSVR_NL_HD void nl_residual_row(const NlResArgs& a, int64_t i, NlAcc& s) {
  const int end = i == 0 ? 0 : (i == a.ne ? 1 : -1);
  double r = 0.0;
  if (end < 0 || a.kind[end] == LSSVR_END_ROBIN) {
    double m = a.diag[i] * a.u[i];
    if (i > 0) m = a.sub[i - 1] * a.u[i - 1] + m;
    if (i < a.ne) m = m + a.sup[i] * a.u[i + 1];
    r = m - a.load[i];
    if (end >= 0) r = r + (a.kappa[end] * a.u[i] - a.end_values[end]);
  }
  nl_take(r, s.r, s.bad);
  nl_take(a.u_new[i] - a.u[i], s.du, s.bad);
  nl_take(a.u_new[i], s.un, s.bad);
}

// the workgroup's sum of its threads' accumulators, in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ NlAcc nl_block_reduce(NlAcc s) {
  __shared__ NlAcc sh[kNlBlock];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = kNlBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      NlAcc t = sh[threadIdx.x];
      nl_merge(t, sh[threadIdx.x + w]);
      sh[threadIdx.x] = t;
    }
    __syncthreads();
  }
  return sh[0];
}

// work[block] = the accumulator of the rows block, block + gridDim, ... of 256 rows each
__global__ __launch_bounds__(kNlBlock) void nl_residual_kernel(NlResArgs a, NlAcc* __restrict__ work) {
  const int64_t n = a.ne + 1, stride = (int64_t)gridDim.x * kNlBlock;
  NlAcc s{0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kNlBlock + threadIdx.x; i < n; i += stride) nl_residual_row(a, i, s);
  s = nl_block_reduce(s);
  if (threadIdx.x == 0) work[blockIdx.x] = s;
}

// one workgroup: out4 = the merge of the nb <= 1024 partials
__global__ __launch_bounds__(kNlBlock) void nl_residual_finish_kernel(const NlAcc* __restrict__ work, int nb,
                                                                      double* __restrict__ out4) {
  NlAcc s{0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += kNlBlock) nl_merge(s, work[b]);
  s = nl_block_reduce(s);
  if (threadIdx.x == 0) {
    out4[0] = s.r;
    out4[1] = s.du;
    out4[2] = s.un;
    out4[3] = s.bad;
  }
}

// out_i = u_i + lambda (u_new_i - u_i)
LSSVR_NL_HD double nl_step_at(const double* __restrict__ u, const double* __restrict__ u_new, double lambda,
                              int64_t i) {
  return u[i] + lambda * (u_new[i] - u[i]);
}

__global__ __launch_bounds__(kNlBlock) void nl_step_kernel(const double* __restrict__ u,
                                                           const double* __restrict__ u_new, double lambda, int64_t n,
                                                           double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kNlBlock;
  for (int64_t i = (int64_t)blockIdx.x * kNlBlock + threadIdx.x; i < n; i += stride)
    out[i] = nl_step_at(u, u_new, lambda, i);
}

}  // namespace

hipError_t nl_linearize(const NlLinArgs& a, bool point_major, hipStream_t s) {
  const dim3 grid((unsigned)nl_blocks(a.ne * (int64_t)a.n)), block(kNlBlock);
  if (point_major)
    hipLaunchKernelGGL(nl_linearize_kernel<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(nl_linearize_kernel<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

void nl_linearize_host(const NlLinArgs& a, bool point_major) {
  const int64_t tab = a.ne * (int64_t)a.n;
  for (int64_t idx = 0; idx < tab; ++idx) nl_entry_at(a, point_major, idx);
}

int64_t nl_residual_work_bytes(int64_t ne) {
  return ne < 1 ? 0 : nl_blocks(ne + 1) * (int64_t)sizeof(NlAcc);
}

hipError_t nl_residual(const NlResArgs& a, double* out4, void* work, hipStream_t s) {
  const int nb = (int)nl_blocks(a.ne + 1);
  NlAcc* w = static_cast<NlAcc*>(work);
  hipLaunchKernelGGL(nl_residual_kernel, dim3((unsigned)nb), dim3(kNlBlock), 0, s, a, w);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nl_residual_finish_kernel, dim3(1), dim3(kNlBlock), 0, s, w, nb, out4);
  return hipGetLastError();
}

void nl_residual_host(const NlResArgs& a, double* out4) {
  NlAcc s{0.0, 0.0, 0.0, 0.0};
  for (int64_t i = 0; i <= a.ne; ++i) nl_residual_row(a, i, s);
  out4[0] = s.r;
  out4[1] = s.du;
  out4[2] = s.un;
  out4[3] = s.bad;
}

hipError_t nl_step(const double* u, const double* u_new, double lambda, int64_t ne, double* out, hipStream_t s) {
  hipLaunchKernelGGL(nl_step_kernel, dim3((unsigned)nl_blocks(ne + 1)), dim3(kNlBlock), 0, s, u, u_new, lambda, ne + 1,
                     out);
  return hipGetLastError();
}

void nl_step_host(const double* u, const double* u_new, double lambda, int64_t ne, double* out) {
  for (int64_t i = 0; i <= ne; ++i) out[i] = nl_step_at(u, u_new, lambda, i);
}

}  // namespace lssvr
