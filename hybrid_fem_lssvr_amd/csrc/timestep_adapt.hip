// Adaptive time stepping for  rho u_t - (a u')' + c u = f(x, t):  variable-step BDF2 with a local error estimate
// (DESIGN.md section 30).  With h the trial step, an attempt solves
//   (K + s M) u^{n+1} = (1/h) M (beta0 u^n + beta1 u^{n-1}) + load(t_{n+1}),   s = alpha / h,
// K = (kdiag, koff) the bands of -(a u')' + c u and M = (mdiag, moff) the mass bands of rho, both assembled once.  This
// file adds what changes with h:
//   step    the attempt's matrix K + s M AND its right-hand side, in one pass over the nodes
//   error   the four numbers the controller reads: the scaled and the plain maximum of the estimate
//           e = ((w3 U3 + w2 U2) + w1 U1) + w0 U0  (a divided difference, its weights from the host), max |U3| and
//           the count of rows that are not finite; per-workgroup partials, then one workgroup merges them
// No atomics, no inline assembly, no scratch; the step kernel uses no LDS.  Each value comes from one inline routine
// that the host mirrors (lssvr_ts_step_host, lssvr_ts_error_host) call too: with -ffp-contract=off the two are
// bit-equal.  A maximum of finite numbers does not depend on the order and the count is a sum of integers, so the
// error's four numbers are bitwise reproducible.
// FP64, -ffp-contract=off.
#include "lssvr_ts.hpp"

namespace lssvr {

namespace {

// Node i.  Every value is formed before the first store, so the mass bands are read once for both outputs:
//   adiag[i] = kdiag[i] + s mdiag[i],  aoff[i] = koff[i] + s moff[i]     (the product first; skipped without
//                                                                          write_bands: s is the previous attempt's)
//   b[i]     = ts_rhs_row, the routine of lssvr_ts_rhs, case 0
LSSVR_TS_HD void ts_step_at(const TsStepArgs& a, int64_t i, double* __restrict__ b) {
  const double r = ts_rhs_row(a.rhs, 0, i);
  if (a.write_bands) {
    const double d = a.kdiag[i] + a.s * a.rhs.mdiag[i];
    if (i < a.rhs.ne) {
      const double o = a.koff[i] + a.s * a.rhs.moff[i];
      a.aoff[i] = o;
    }
    a.adiag[i] = d;
  }
  b[i] = r;
}

__global__ __launch_bounds__(kTsBlock) void ts_step_kernel(TsStepArgs a, double* __restrict__ b) {
  const int64_t n = a.rhs.ne + 1, stride = (int64_t)gridDim.x * kTsBlock;
  for (int64_t i = (int64_t)blockIdx.x * kTsBlock + threadIdx.x; i < n; i += stride) ts_step_at(a, i, b);
}

// The four numbers of the estimate as they are accumulated: three maxima of finite values >= 0 and a count (held in a
// double: exact below 2^53).
struct TsAcc {
  double q, e, u, bad;
};

LSSVR_TS_HD void ts_merge(TsAcc& s, const TsAcc& o) {
  if (o.q > s.q) s.q = o.q;
  if (o.e > s.e) s.e = o.e;
  if (o.u > s.u) s.u = o.u;
  s.bad = s.bad + o.bad;
}

// Row i; a Dirichlet end row is data, not solution, and is skipped whole.  The order of every sum:
//   e   = ((w3 U3 + w2 U2) + w1 U1) + w0 U0        w1 == 0 reads no U1, w0 == 0 reads no U0
//   sc  = atol + rtol max(|U3|, |U2|)               max(x, y) = x > y ? x : y
// A row whose e or sc is not finite raises the count and joins neither maximum of e; |U3| joins its maximum when it is
// finite.
LSSVR_TS_HD void ts_error_row(const TsErrArgs& a, int64_t i, TsAcc& s) {
  if ((i == 0 && a.kind[0] == LSSVR_END_DIRICHLET) || (i == a.ne && a.kind[1] == LSSVR_END_DIRICHLET)) return;
  const double u3 = a.U3[i], u2 = a.U2[i];
  double e = a.w3 * u3 + a.w2 * u2;
  if (a.w1 != 0.0) e = e + a.w1 * a.U1[i];
  if (a.w0 != 0.0) e = e + a.w0 * a.U0[i];
  const double a3 = fabs(u3), a2 = fabs(u2), ae = fabs(e);
  const double sc = a.atol + a.rtol * (a3 > a2 ? a3 : a2);
  if (!(ae < INFINITY) || !(sc < INFINITY)) {
    s.bad = s.bad + 1.0;
  } else {
    const double q = ae / sc;
    if (q > s.q) s.q = q;
    if (ae > s.e) s.e = ae;
  }
  if (a3 < INFINITY && a3 > s.u) s.u = a3;
}

// the workgroup's merge of its threads' accumulators, in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ TsAcc ts_block_reduce(TsAcc s) {
  __shared__ TsAcc sh[kTsBlock];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = kTsBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      TsAcc t = sh[threadIdx.x];
      ts_merge(t, sh[threadIdx.x + w]);
      sh[threadIdx.x] = t;
    }
    __syncthreads();
  }
  return sh[0];
}

// work[block] = the accumulator of the rows block, block + gridDim, ... of 256 rows each
__global__ __launch_bounds__(kTsBlock) void ts_error_kernel(TsErrArgs a, TsAcc* __restrict__ work) {
  const int64_t n = a.ne + 1, stride = (int64_t)gridDim.x * kTsBlock;
  TsAcc s{0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kTsBlock + threadIdx.x; i < n; i += stride) ts_error_row(a, i, s);
  s = ts_block_reduce(s);
  if (threadIdx.x == 0) work[blockIdx.x] = s;
}

// one workgroup: out4 = the merge of the nb <= 1024 partials
__global__ __launch_bounds__(kTsBlock) void ts_error_finish_kernel(const TsAcc* __restrict__ work, int nb,
                                                                   double* __restrict__ out4) {
  TsAcc s{0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += kTsBlock) ts_merge(s, work[b]);
  s = ts_block_reduce(s);
  if (threadIdx.x == 0) {
    out4[0] = s.q;
    out4[1] = s.e;
    out4[2] = s.u;
    out4[3] = s.bad;
  }
}

}  // namespace

hipError_t ts_step(const TsStepArgs& a, double* b, hipStream_t s) {
  hipLaunchKernelGGL(ts_step_kernel, dim3((unsigned)ts_blocks(a.rhs.ne + 1)), dim3(kTsBlock), 0, s, a, b);
  return hipGetLastError();
}

void ts_step_host(const TsStepArgs& a, double* b) {
  for (int64_t i = 0; i <= a.rhs.ne; ++i) ts_step_at(a, i, b);
}

int64_t ts_error_work_bytes(int64_t ne) {
  return ne < 1 ? 0 : ts_blocks(ne + 1) * (int64_t)sizeof(TsAcc);
}

hipError_t ts_error(const TsErrArgs& a, double* out4, void* work, hipStream_t s) {
  const int nb = (int)ts_blocks(a.ne + 1);
  TsAcc* w = static_cast<TsAcc*>(work);
  hipLaunchKernelGGL(ts_error_kernel, dim3((unsigned)nb), dim3(kTsBlock), 0, s, a, w);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ts_error_finish_kernel, dim3(1), dim3(kTsBlock), 0, s, w, nb, out4);
  return hipGetLastError();
}

void ts_error_host(const TsErrArgs& a, double* out4) {
  TsAcc s{0.0, 0.0, 0.0, 0.0};
  for (int64_t i = 0; i <= a.ne; ++i) ts_error_row(a, i, s);
  out4[0] = s.q;
  out4[1] = s.e;
  out4[2] = s.u;
  out4[3] = s.bad;
}

}  // namespace lssvr
