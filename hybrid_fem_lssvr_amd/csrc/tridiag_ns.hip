// Device tridiagonal solve for the NON-SYMMETRIC P1 system of -(a u')' + b u' + c u = f (p1_conv.hip) with
// Dirichlet data on both end dofs: row i is  sub[i-1] u[i-1] + diag[i] u[i] + sup[i] u[i+1] = load[i].
//
// Algorithm: the recursive substructuring of tridiag.hip.  Every kLc-th (8th) unknown is a separator; one thread
// condenses the kLc-1 unknowns between two separators onto them (two O(1)-state sweeps, nothing stored), the
// separators form a tridiagonal system kLc times smaller, which is solved the same way until <= kBase unknowns
// remain (parallel cyclic reduction in LDS); going back up, each thread re-solves its chunk with the now-known
// separator values.  The lower and the upper band are separate arrays at every level, the caller's included.
//
// NO PIVOTING at any level.  That is safe when every row is diagonally dominant, |sub[i-1]| + |sup[i]| <= diag[i]:
// row dominance is inherited by every Schur complement of Gaussian elimination, so it holds for the condensed
// chunks, for every reduced separator system and for every step of the cyclic reduction, and no divisor can
// vanish.  The assembled rows are dominant when, on every element, the cell Peclet number
// |bbar_e| h_e / (2 abar_e) <= 1 and c >= 0.  Outside that the solve may divide by a
// small number without notice: the caller refines the mesh first.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

namespace lssvr {

namespace {

constexpr int kNsBase = 512;     // unknowns of the base level: one workgroup, one unknown per thread
constexpr int kNsLc = 8;         // chunk length of every level (tridiag.hip: 8 measured fastest, one 64-byte run each)

// row i: lo[i] x[i-1] + d[i] x[i] + up[i] x[i+1] = r[i] - [i==0] bl[0]*u0 - [i==m-1] br[0]*u1
struct NsSys {
  const double* lo;
  const double* d;
  const double* up;
  const double* r;
  const double* bl;
  const double* br;
  double u0, u1;
  int64_t m;
};

__device__ __forceinline__ double ns_lo(const NsSys& s, int64_t i) { return i == 0 ? 0.0 : s.lo[i]; }
__device__ __forceinline__ double ns_up(const NsSys& s, int64_t i) { return i == s.m - 1 ? 0.0 : s.up[i]; }
__device__ __forceinline__ double ns_r(const NsSys& s, int64_t i) {
  double v = s.r[i];
  if (i == 0 && s.bl) v -= s.bl[0] * s.u0;
  if (i == s.m - 1 && s.br) v -= s.br[0] * s.u1;
  return v;
}

// x_interior = y + v * x_{left separator} + w * x_{right separator}, at the first (F) and last (L) interior unknown
struct NsEnds {
  double yF, vF, wF, yL, vL, wL;
};

// The kLc-1 interior rows of a chunk, loaded back to back before they are used: a thread walks its own 64-byte
// stretch of every array, so its uses of a 128-byte line must be adjacent in time (tridiag.hip, kBatch).
struct NsRows {
  double lo[kNsLc - 1], d[kNsLc - 1], up[kNsLc - 1], r[kNsLc - 1];
};

// rows b .. b+kNsLc-2 clipped to [b, e): entries outside are a copy of row b and are never used
__device__ __forceinline__ void ns_load(const NsSys& s, int64_t b, int64_t e, NsRows& rb) {
#pragma unroll
  for (int t = 0; t < kNsLc - 1; ++t) {
    const int64_t i = (b + t < e) ? b + t : b;
    rb.lo[t] = ns_lo(s, i);
    rb.d[t] = s.d[i];
    rb.up[t] = ns_up(s, i);
    rb.r[t] = ns_r(s, i);
  }
}

// chunk j: interior unknowns [j*kLc, min(j*kLc + kLc-1, m)), never empty for j < nc = ceil(m / kLc)
__global__ __launch_bounds__(kBlock) void tri_ns_condense_kernel(NsSys s, int64_t nc, NsEnds* __restrict__ ends) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nc) return;
  const int64_t b = j * kNsLc;
  const int64_t e = (b + kNsLc - 1 < s.m) ? b + kNsLc - 1 : s.m;
  const int len = (int)(e - b);
  NsRows rb;
  ns_load(s, b, e, rb);
  NsEnds c;
  {  // downward sweep -> values at the last interior unknown; one division per row
    double den = 1.0 / rb.d[0];
    double y = rb.r[0] * den, v = -rb.lo[0] * den, cp = rb.up[0] * den;
#pragma unroll
    for (int t = 1; t < kNsLc - 1; ++t) {
      if (t < len) {
        const double l = rb.lo[t];
        den = 1.0 / (rb.d[t] - l * cp);
        y = (rb.r[t] - l * y) * den;
        v = (-l * v) * den;
        cp = rb.up[t] * den;
      }
    }
    c.yL = y;
    c.vL = v;
    c.wL = -cp;
  }
  {  // upward sweep -> values at the first interior unknown
    double den = 1.0, bp = 0.0, y = 0.0, w = 0.0;
#pragma unroll
    for (int t = kNsLc - 2; t >= 0; --t) {
      if (t < len) {
        if (t == len - 1) {
          den = 1.0 / rb.d[t];
          y = rb.r[t] * den;
          w = -rb.up[t] * den;
        } else {
          const double u = rb.up[t];
          den = 1.0 / (rb.d[t] - u * bp);
          y = (rb.r[t] - u * y) * den;
          w = (-u * w) * den;
        }
        bp = rb.lo[t] * den;
      }
    }
    c.yF = y;
    c.wF = w;
    c.vF = -bp;
  }
  ends[j] = c;
}

// separator j sits at p = j*kLc + kLc-1 < m (j < ns = m / kLc), between chunk j (left) and chunk j+1 (right)
__global__ __launch_bounds__(kBlock) void tri_ns_reduce_kernel(NsSys s, int64_t ns, int64_t nc,
                                                                const NsEnds* __restrict__ ends,
                                                                double* __restrict__ LO, double* __restrict__ D,
                                                                double* __restrict__ UP, double* __restrict__ R) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= ns) return;
  const int64_t p = j * kNsLc + kNsLc - 1;
  const double l = s.lo[p];
  const double u = ns_up(s, p);
  const NsEnds cl = ends[j];
  double dd = s.d[p] + l * cl.wL;
  double rr = ns_r(s, p) - l * cl.yL;
  double uu = 0.0;
  if (j + 1 < nc) {
    const NsEnds cr = ends[j + 1];
    dd += u * cr.vF;
    rr -= u * cr.yF;
    uu = u * cr.wF;
  }
  LO[j] = l * cl.vL;
  D[j] = dd;
  UP[j] = uu;
  R[j] = rr;
}

// re-solve every chunk with its separator values X[ns] known; x (length m) receives the whole level's solution
__global__ __launch_bounds__(kBlock) void tri_ns_expand_kernel(NsSys s, int64_t ns, int64_t nc,
                                                                const double* __restrict__ X,
                                                                double* __restrict__ x) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nc) return;
  const int64_t b = j * kNsLc;
  const int64_t e = (b + kNsLc - 1 < s.m) ? b + kNsLc - 1 : s.m;
  const int len = (int)(e - b);
  const double xl = j > 0 ? X[j - 1] : 0.0;
  const double xr = j < ns ? X[j] : 0.0;
  NsRows rb;
  ns_load(s, b, e, rb);
  // forward elimination; the modified coefficients stay in registers, the back substitution only stores
  double cc[kNsLc - 1], yy[kNsLc - 1];
  double c = 0.0, y = 0.0;
#pragma unroll
  for (int t = 0; t < kNsLc - 1; ++t) {
    if (t < len) {
      double ri = rb.r[t];
      if (t == 0) ri -= rb.lo[t] * xl;
      if (t == len - 1) ri -= rb.up[t] * xr;
      const double l = rb.lo[t];
      const double den = 1.0 / (t == 0 ? rb.d[t] : rb.d[t] - l * c);
      y = (t == 0 ? ri : ri - l * y) * den;
      c = rb.up[t] * den;
    }
    cc[t] = c;
    yy[t] = y;
  }
  double xn = 0.0;
#pragma unroll
  for (int t = kNsLc - 2; t >= 0; --t) {
    if (t < len) {
      xn = (t == len - 1) ? yy[t] : yy[t] - cc[t] * xn;
      x[b + t] = xn;
    }
  }
  if (j < ns) x[b + kNsLc - 1] = xr;
}

// Parallel cyclic reduction of row i (li, di, ui, ri) of an m-row system in LDS, all kNsBase threads of the one
// workgroup together, ceil(log2 m) steps.  Each step eliminates x[i-st] and x[i+st] from row i with the rows st away:
// the new lower band comes from their lower band, the new upper band from their upper band.  Returns x[i].
__device__ __forceinline__ double ns_pcr(double li, double di, double ui, double ri, int i, int m, double* lo,
                                         double* d, double* up, double* r) {
  const bool in = i < m;
  for (int st = 1; st < m; st <<= 1) {
    lo[i] = li;
    d[i] = di;
    up[i] = ui;
    r[i] = ri;
    __syncthreads();
    if (in) {
      double nl = 0.0, nu = 0.0;
      if (i - st >= 0) {
        const double al = -li / d[i - st];
        di += al * up[i - st];
        ri += al * r[i - st];
        nl = al * lo[i - st];
      }
      if (i + st < m) {
        const double be = -ui / d[i + st];
        di += be * lo[i + st];
        ri += be * r[i + st];
        nu = be * up[i + st];
      }
      li = nl;
      ui = nu;
    }
    __syncthreads();
  }
  return ri / di;
}

// Base level (m <= kNsBase): cyclic reduction, then ONE step of iterative refinement with the residual of the
// original rows.  Cyclic reduction computes every unknown by its own chain of eliminations, so the rounding errors of
// neighbouring unknowns are unrelated, and the matrix amplifies such a rough error by |A| in the residual: at 510
// unknowns of a P1 Laplacian the residual came out at 1.15 times the rounding-level bar the chunked levels meet with
// room to spare (measured on an MI355X).  The correction costs a second reduction of one
// workgroup, a few microseconds.
__global__ __launch_bounds__(kNsBase) void tri_ns_base_kernel(NsSys s, double* __restrict__ x) {
  __shared__ double lo[kNsBase], d[kNsBase], up[kNsBase], r[kNsBase];
  const int i = threadIdx.x;
  const int m = (int)s.m;
  const bool in = i < m;
  double li = 0.0, di = 1.0, ui = 0.0, ri = 0.0;
  if (in) {
    li = ns_lo(s, i);
    di = s.d[i];
    ui = ns_up(s, i);
    ri = ns_r(s, i);
  }
  const double xi = ns_pcr(li, di, ui, ri, i, m, lo, d, up, r);
  // residual of row i with fused multiply-adds (one rounding each): r - lo x[i-1] - d x[i] - up x[i+1]
  r[i] = xi;
  __syncthreads();
  double res = 0.0;
  if (in) {
    res = fma(-di, xi, ri);
    if (i > 0) res = fma(-li, r[i - 1], res);
    if (i + 1 < m) res = fma(-ui, r[i + 1], res);
  }
  __syncthreads();
  const double dx = ns_pcr(li, di, ui, res, i, m, lo, d, up, r);
  if (in) x[i] = xi + dx;
}

__global__ void tri_ns_ends_kernel(double* u, int64_t ne, double u0, double u1) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    u[0] = u0;
    u[ne] = u1;
  }
}

// workspace (in doubles) of the levels above the base: ends[6*nc] + reduced LO, D, UP, R, X [5*ns]
int64_t ns_level_doubles(int64_t m) {
  int64_t tot = 0;
  while (m > kNsBase) {
    const int64_t nc = (m + kNsLc - 1) / kNsLc, ns = m / kNsLc;
    tot += 6 * nc + 5 * ns + 16;
    m = ns;
  }
  return tot + 16;
}

hipError_t ns_solve_level(const NsSys& s, double* x, double* work, hipStream_t st) {
  if (s.m <= 0) return hipSuccess;
  if (s.m <= kNsBase) {
    hipLaunchKernelGGL(tri_ns_base_kernel, dim3(1), dim3((unsigned)kNsBase), 0, st, s, x);
    return hipGetLastError();
  }
  const int64_t nc = (s.m + kNsLc - 1) / kNsLc, ns = s.m / kNsLc;
  NsEnds* ends = reinterpret_cast<NsEnds*>(work);
  double* LO = reinterpret_cast<double*>(ends + nc);
  double* D = LO + ns;
  double* UP = D + ns;
  double* R = UP + ns;
  double* X = R + ns;
  double* next = X + ns + 16;
  const unsigned gc = (unsigned)((nc + kBlock - 1) / kBlock);
  const unsigned gs = (unsigned)((ns + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(tri_ns_condense_kernel, dim3(gc), dim3(kBlock), 0, st, s, nc, ends);
  hipLaunchKernelGGL(tri_ns_reduce_kernel, dim3(gs), dim3(kBlock), 0, st, s, ns, nc, ends, LO, D, UP, R);
  const NsSys red{LO, D, UP, R, nullptr, nullptr, 0.0, 0.0, ns};
  const hipError_t err = ns_solve_level(red, X, next, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(tri_ns_expand_kernel, dim3(gc), dim3(kBlock), 0, st, s, ns, nc, X, x);
  return hipGetLastError();
}

}  // namespace

int64_t tridiag_ns_work_bytes(int64_t ne) {
  const int64_t m = ne > 1 ? ne - 1 : 0;
  return 8 * ns_level_doubles(m) + 256;
}

hipError_t tridiag_ns_dirichlet_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                      int64_t ne, double u0, double u1, double* u, void* work, hipStream_t st) {
  hipLaunchKernelGGL(tri_ns_ends_kernel, dim3(1), dim3(64), 0, st, u, ne, u0, u1);
  const int64_t m = ne - 1;
  if (m <= 0) return hipGetLastError();
  // interior unknown k <-> node k+1: lo = sub[k] (u_k in row k+1), d = diag[k+1], up = sup[k+1], r = load[k+1];
  // the end rows lose sub[0] * u0 and sup[ne-1] * u1 to the right-hand side
  const NsSys s{sub, diag + 1, sup + 1, load + 1, sub, sup + (ne - 1), u0, u1, m};
  return ns_solve_level(s, u + 1, reinterpret_cast<double*>(work), st);
}

}  // namespace lssvr
