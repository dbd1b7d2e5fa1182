// Device tridiagonal solve with Dirichlet data on both end dofs, for the assembled P1 systems: the symmetric bands
// of -(a u')' + c u = f -- `enforce(A, b, D=basis.get_dofs())` + `solve(A, b)` (Dual.py:129-130), SURVEY.md section
// 8(f) "next-1" -- and the non-symmetric bands of -(a u')' + b u' + c u = f (p1_conv.hip), where row i is
// sub[i-1] u[i-1] + diag[i] u[i] + sup[i] u[i+1] = load[i].  One set of kernels serves both entries: the lower and
// the upper band are separate arrays at every level, and the symmetric entry points them at off and off + 1.
//
// Algorithm: recursive substructuring (static condensation).  Every kLc-th (8th) unknown is a separator; one thread
// condenses the kLc-1 unknowns between two separators onto them (two O(1)-state sweeps, nothing stored), the
// separators form a tridiagonal system kLc times smaller, which is solved the same way until <= kBase unknowns
// remain (parallel cyclic reduction in LDS).  Going back up, each thread re-solves its chunk with the now-known
// separator values.
//
// NO PIVOTING at any level.  That is safe when every row is diagonally dominant, |sub[i-1]| + |sup[i]| <= diag[i]:
// row dominance is inherited by every Schur complement of Gaussian elimination, so it holds for the condensed
// chunks, for every reduced separator system and for every step of the cyclic reduction, and no divisor can
// vanish.  The symmetric P1 matrix is SPD (Schur complements of SPD are SPD).  The non-symmetric rows are dominant
// when, on every element, the cell Peclet number |bbar_e| h_e / (2 abar_e) <= 1 and c >= 0.
// Outside that the solve may divide by a small number without notice: the caller refines the mesh first.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

namespace lssvr {

namespace {

// Chunk length of every level: 8 at every size (round 2, one run: 1e7 unknowns 432 us against 675 us with chunks of
// 16 and 818 us with 32 -- a thread's 64-byte run of each array is one batch, a 128-byte line is shared by two
// neighbouring lanes of the same load instruction; 4 is as fast, with twice the levels).  Each row costs ONE
// division (1/den) and three multiplications in every sweep -- with three divisions per row the sweeps were bound by
// the FP64 division chain: 101 -> 55 us at 1e5 unknowns, 177 -> 91 us at 1e6.
constexpr int kLc = 8;
constexpr int kBase = 512;       // unknowns of the base level: one workgroup, one unknown per thread

// row i: lo[i] x[i-1] + d[i] x[i] + up[i] x[i+1] = r[i] - [i==0] bl[0]*u0 - [i==m-1] br[0]*u1
struct TriSys {
  const double* lo;
  const double* d;
  const double* up;
  const double* r;
  const double* bl;
  const double* br;
  double u0, u1;
  int64_t m;
};

__device__ __forceinline__ double lo_at(const TriSys& s, int64_t i) { return i == 0 ? 0.0 : s.lo[i]; }
__device__ __forceinline__ double up_at(const TriSys& s, int64_t i) { return i == s.m - 1 ? 0.0 : s.up[i]; }
__device__ __forceinline__ double r_at(const TriSys& s, int64_t i) {
  double v = s.r[i];
  if (i == 0 && s.bl) v -= s.bl[0] * s.u0;
  if (i == s.m - 1 && s.br) v -= s.br[0] * s.u1;
  return v;
}

// x_interior = y + v * x_{left separator} + w * x_{right separator}; only the values at the first (F) and last (L)
// interior unknown are needed for the reduced system.
struct ChunkEnds {
  double yF, vF, wF, yL, vL, wL;
};

// The kLc-1 interior rows of a chunk, loaded back to back into registers before they are used: a thread walks its
// own 64-byte stretch of every array, so its uses of a 128-byte line must be adjacent in time or the line is evicted
// from the 32 KB L1 by the other 63 lanes' lines in between (measured: 1.6x less time at 1e7 unknowns than one load
// per step).
struct ChunkRows {
  double lo[kLc - 1], d[kLc - 1], up[kLc - 1], r[kLc - 1];
};

// rows b .. b+kLc-2 clipped to [b, e): entries outside are a copy of row b and are never used
__device__ __forceinline__ void load_rows(const TriSys& s, int64_t b, int64_t e, ChunkRows& rb) {
#pragma unroll
  for (int t = 0; t < kLc - 1; ++t) {
    const int64_t i = (b + t < e) ? b + t : b;
    rb.lo[t] = lo_at(s, i);
    rb.d[t] = s.d[i];
    rb.up[t] = up_at(s, i);
    rb.r[t] = r_at(s, i);
  }
}

// chunk j: interior unknowns [j*kLc, min(j*kLc + kLc-1, m)), never empty for j < nc = ceil(m / kLc)
__global__ __launch_bounds__(kBlock) void tri_condense_kernel(TriSys s, int64_t nc, ChunkEnds* __restrict__ ends) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nc) return;
  const int64_t b = j * kLc;
  const int64_t e = (b + kLc - 1 < s.m) ? b + kLc - 1 : s.m;
  const int len = (int)(e - b);
  ChunkRows rb;
  load_rows(s, b, e, rb);
  ChunkEnds c;
  {  // downward sweep -> values at the last interior unknown; one division per row (1/den), three multiplications
    double den = 1.0 / rb.d[0];
    double y = rb.r[0] * den, v = -rb.lo[0] * den, cp = rb.up[0] * den;
#pragma unroll
    for (int t = 1; t < kLc - 1; ++t) {
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
    c.wL = -cp;               // rhs -up[e-1] e_last  ->  -up[e-1]/den_last  (den holds 1/den)
  }
  {  // upward sweep -> values at the first interior unknown
    double den = 1.0, bp = 0.0, y = 0.0, w = 0.0;
#pragma unroll
    for (int t = kLc - 2; t >= 0; --t) {
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
__global__ __launch_bounds__(kBlock) void tri_reduce_kernel(TriSys s, int64_t ns, int64_t nc,
                                                             const ChunkEnds* __restrict__ ends,
                                                             double* __restrict__ LO, double* __restrict__ D,
                                                             double* __restrict__ UP, double* __restrict__ R) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= ns) return;
  const int64_t p = j * kLc + kLc - 1;
  const double l = s.lo[p];
  const double u = up_at(s, p);
  const ChunkEnds cl = ends[j];
  double dd = s.d[p] + l * cl.wL;
  double rr = r_at(s, p) - l * cl.yL;
  double uu = 0.0;
  if (j + 1 < nc) {
    const ChunkEnds cr = ends[j + 1];
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
__global__ __launch_bounds__(kBlock) void tri_expand_kernel(TriSys s, int64_t ns, int64_t nc,
                                                             const double* __restrict__ X, double* __restrict__ x) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nc) return;
  const int64_t b = j * kLc;
  const int64_t e = (b + kLc - 1 < s.m) ? b + kLc - 1 : s.m;
  const int len = (int)(e - b);
  const double xl = j > 0 ? X[j - 1] : 0.0;
  const double xr = j < ns ? X[j] : 0.0;
  ChunkRows rb;
  load_rows(s, b, e, rb);
  // forward elimination; the modified coefficients stay in registers (kLc-1 = 7 of each), so the back substitution
  // touches memory only to store the solution
  double cc[kLc - 1], yy[kLc - 1];
  double c = 0.0, y = 0.0;
#pragma unroll
  for (int t = 0; t < kLc - 1; ++t) {
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
  for (int t = kLc - 2; t >= 0; --t) {
    if (t < len) {
      xn = (t == len - 1) ? yy[t] : yy[t] - cc[t] * xn;
      x[b + t] = xn;
    }
  }
  if (j < ns) x[b + kLc - 1] = xr;
}

// Parallel cyclic reduction of row i (li, di, ui, ri) of an m-row system in LDS, all kBase threads of the one
// workgroup together, ceil(log2 m) steps.  Each step eliminates x[i-st] and x[i+st] from row i with the rows st
// away: the new lower band comes from their lower band, the new upper band from their upper band.  Returns x[i].
__device__ __forceinline__ double tri_pcr(double li, double di, double ui, double ri, int i, int m, double* lo,
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

// Base level (m <= kBase unknowns): parallel cyclic reduction, one workgroup of kBase threads -- a serial Thomas
// sweep by one thread would pay a global-memory round trip per unknown (~100 us for 100 unknowns; this takes a few
// us).  PCR needs no pivoting for the SPD / diagonally dominant systems that reach this level.
// kRefine (the non-symmetric entry): then ONE step of iterative refinement with the residual of the original rows.
// Cyclic reduction computes every unknown by its own chain of eliminations, so the rounding errors of neighbouring
// unknowns are unrelated, and the matrix amplifies such a rough error by |A| in the residual: at 510 unknowns of a
// P1 Laplacian the residual came out at 1.15 times the rounding-level bar the chunked levels meet with room to
// spare (measured on an MI355X).  The correction costs a second reduction of one workgroup, a
// few microseconds.  The symmetric entry does without it: the step would change its bits and its time.
template <bool kRefine>
__global__ __launch_bounds__(kBase) void tri_base_kernel(TriSys s, double* __restrict__ x) {
  __shared__ double lo[kBase], d[kBase], up[kBase], r[kBase];
  const int i = threadIdx.x;
  const int m = (int)s.m;
  const bool in = i < m;
  double li = 0.0, di = 1.0, ui = 0.0, ri = 0.0;
  if (in) {
    li = lo_at(s, i);
    di = s.d[i];
    ui = up_at(s, i);
    ri = r_at(s, i);
  }
  double xi = tri_pcr(li, di, ui, ri, i, m, lo, d, up, r);
  if constexpr (kRefine) {
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
    xi += tri_pcr(li, di, ui, res, i, m, lo, d, up, r);
  }
  if (in) x[i] = xi;
}

__global__ void tri_ends_kernel(double* u, int64_t ne, double u0, double u1) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    u[0] = u0;
    u[ne] = u1;
  }
}

// workspace (in doubles) of the levels above the base: ends[6*nc] + reduced LO, D, UP, R, X [5*ns]
int64_t level_doubles(int64_t m) {
  int64_t tot = 0;
  while (m > kBase) {
    const int64_t nc = (m + kLc - 1) / kLc, ns = m / kLc;
    tot += 6 * nc + 5 * ns + 16;
    m = ns;
  }
  return tot + 16;
}

template <bool kRefine>
hipError_t solve_level(const TriSys& s, double* x, double* work, hipStream_t st) {
  if (s.m <= 0) return hipSuccess;
  if (s.m <= kBase) {
    hipLaunchKernelGGL(tri_base_kernel<kRefine>, dim3(1), dim3((unsigned)kBase), 0, st, s, x);
    return hipGetLastError();
  }
  const int64_t nc = (s.m + kLc - 1) / kLc, ns = s.m / kLc;
  ChunkEnds* ends = reinterpret_cast<ChunkEnds*>(work);
  double* LO = reinterpret_cast<double*>(ends + nc);
  double* D = LO + ns;
  double* UP = D + ns;
  double* R = UP + ns;
  double* X = R + ns;
  double* next = X + ns + 16;
  const unsigned gc = (unsigned)((nc + kBlock - 1) / kBlock);
  const unsigned gs = (unsigned)((ns + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(tri_condense_kernel, dim3(gc), dim3(kBlock), 0, st, s, nc, ends);
  hipLaunchKernelGGL(tri_reduce_kernel, dim3(gs), dim3(kBlock), 0, st, s, ns, nc, ends, LO, D, UP, R);
  const TriSys red{LO, D, UP, R, nullptr, nullptr, 0.0, 0.0, ns};
  const hipError_t err = solve_level<kRefine>(red, X, next, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(tri_expand_kernel, dim3(gc), dim3(kBlock), 0, st, s, ns, nc, X, x);
  return hipGetLastError();
}

// u[0] = u0, u[ne] = u1, then the ne-1 interior unknowns of s into u[1 ..]
template <bool kRefine>
hipError_t dirichlet_solve(const TriSys& s, int64_t ne, double* u, void* work, hipStream_t st) {
  hipLaunchKernelGGL(tri_ends_kernel, dim3(1), dim3(64), 0, st, u, ne, s.u0, s.u1);
  if (s.m <= 0) return hipGetLastError();
  return solve_level<kRefine>(s, u + 1, reinterpret_cast<double*>(work), st);
}

}  // namespace

int64_t tridiag_work_bytes(int64_t ne) {
  const int64_t m = ne > 1 ? ne - 1 : 0;
  return 8 * level_doubles(m) + 256;
}

// interior unknown k <-> node k+1: lo = off[k] (u_k in row k+1), d = diag[k+1], up = off[k+1], r = load[k+1]; the end
// rows lose off[0] * u0 and off[ne-1] * u1 to the right-hand side
hipError_t tridiag_dirichlet_solve(const double* diag, const double* off, const double* load, int64_t ne, double u0,
                                   double u1, double* u, void* work, hipStream_t st) {
  const TriSys s{off, diag + 1, off + 1, load + 1, off, off + (ne - 1), u0, u1, ne - 1};
  return dirichlet_solve<false>(s, ne, u, work, st);
}

// the same with lo = sub[k], up = sup[k+1]; the end rows lose sub[0] * u0 and sup[ne-1] * u1
hipError_t tridiag_ns_dirichlet_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                      int64_t ne, double u0, double u1, double* u, void* work, hipStream_t st) {
  const TriSys s{sub, diag + 1, sup + 1, load + 1, sub, sup + (ne - 1), u0, u1, ne - 1};
  return dirichlet_solve<true>(s, ne, u, work, st);
}

}  // namespace lssvr
