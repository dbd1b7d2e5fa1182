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
// (tridiag_pivot.hip is the solver that pivots: lssvr_tridiag_pivot_solve_multi)
//
// Several right-hand sides on one matrix.  Everything except the y recurrence and the
// right-hand side is independent of the load, so every kernel takes NC cases: it loads the three bands of a chunk
// once, computes the pivots (1/den), cp, v, w, bp and cc[] once and keeps them in registers, and then sends one case
// after the other through the y recurrence alone.  A call is cut into passes of kTriMultiCases cases; a pass of one
// case -- every call of the single-RHS entries is one -- runs the NC = 1 instantiation.  The operations of a case
// and their order do not depend on NC (the build has -ffp-contract=off, so a product and a sum are never fused unless
// the source says fma()), so row q of a multi call has the bits of the single entry on case q.
//
// Free ends.  A Robin end a du/dn + kappa u = g keeps its end node as an unknown: the system
// then starts at node 0 (ends at node ne), that row has no known neighbour (bl / br NULL), and the kernels add kappa
// to its diagonal and g to its right-hand side where they read them -- the caller's bands are never written.  The
// kernels are templates on the type of their cases: TriCases is the Dirichlet text, unchanged, TriCasesFree adds the
// two end terms; the reduced levels of either are TriCases.  With both ends Dirichlet the TriCasesFree instantiation
// performs the operations of the TriCases one, bit for bit.
//
// Periodic ends.  Node ne is node 0 and the matrix gains two corner entries.  The seam value s
// is one more separator: the Dirichlet kernels above, called as they are, give y (end values 0) for every case and z
// (zero load, end values 1) once per call; tri_seam_kernel solves the seam row for s, tri_seam_combine_kernel writes
// u = y + s z.  Row dominance of the cyclic matrix is that of its Schur complement, so no pivoting here either.
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

// The cases of one pass on s: s.r is the right-hand side of the first, case q is rs doubles further on, and its end
// values are bc[2q], bc[2q+1] -- or, with bc NULL, s.u0 and s.u1 (by value: the single entries, and zeros for a multi
// call without bc).  A pass holds 1 <= nlive <= NC cases; slot q >= nlive repeats case nlive-1 (loads in bounds) and
// stores nothing.
struct TriCases {
  TriSys s;
  int64_t rs;
  const double* bc;
  int nlive;
};

// TriCases whose first (f0) / last (f1) row is the row of a free end node: the kernels add k0 / k1 to its diagonal
// and the end value of the case (g of the Robin condition) to its right-hand side; s.bl / s.br is NULL there.  An end
// that is not free is a Dirichlet end as in TriCases.
struct TriCasesFree : TriCases {
  double k0, k1;
  int f0, f1;
};

__device__ __forceinline__ double lo_at(const TriSys& s, int64_t i) { return i == 0 ? 0.0 : s.lo[i]; }
__device__ __forceinline__ double up_at(const TriSys& s, int64_t i) { return i == s.m - 1 ? 0.0 : s.up[i]; }
template <int NC>
__device__ __forceinline__ int case_of(const TriCases& tc, int q) {
  if constexpr (NC == 1)
    return 0;       // a pass of one case has no idle slot
  else
    return q < tc.nlive ? q : tc.nlive - 1;
}
// the right-hand side of row i for case c
__device__ __forceinline__ double r_at(const TriCases& tc, int c, int64_t i) {
  const TriSys& s = tc.s;
  double v = s.r[c * tc.rs + i];
  if (i == 0 && s.bl) v -= s.bl[0] * (tc.bc ? tc.bc[2 * c] : s.u0);
  if (i == s.m - 1 && s.br) v -= s.br[0] * (tc.bc ? tc.bc[2 * c + 1] : s.u1);
  return v;
}
__device__ __forceinline__ double r_at(const TriCasesFree& tc, int c, int64_t i) {
  double v = r_at(static_cast<const TriCases&>(tc), c, i);
  if (i == 0 && tc.f0) v += tc.bc ? tc.bc[2 * c] : tc.s.u0;
  if (i == tc.s.m - 1 && tc.f1) v += tc.bc ? tc.bc[2 * c + 1] : tc.s.u1;
  return v;
}
// the diagonal of row i
__device__ __forceinline__ double d_at(const TriCases& tc, int64_t i) { return tc.s.d[i]; }
__device__ __forceinline__ double d_at(const TriCasesFree& tc, int64_t i) {
  double v = tc.s.d[i];
  if (i == 0 && tc.f0) v += tc.k0;
  if (i == tc.s.m - 1 && tc.f1) v += tc.k1;
  return v;
}

// x_interior = y + v * x_{left separator} + w * x_{right separator}; only the values at the first (F) and last (L)
// interior unknown are needed for the reduced system.  v and w do not depend on the load: one per chunk ...
struct ChunkEndsShared {
  double vF, wF, vL, wL;
};
// ... and y, one per chunk and case
struct ChunkEndsCase {
  double yF, yL;
};

// The kLc-1 interior rows of a chunk, loaded back to back into registers before they are used: a thread walks its
// own 64-byte stretch of every array, so its uses of a 128-byte line must be adjacent in time or the line is evicted
// from the 32 KB L1 by the other 63 lanes' lines in between (measured: 1.6x less time at 1e7 unknowns than one load
// per step).  The right-hand sides follow case by case, in the same way (load_case_rows).
struct ChunkRows {
  double lo[kLc - 1], d[kLc - 1], up[kLc - 1];
};

// rows b .. b+kLc-2 clipped to [b, e): entries outside are a copy of row b and are never used
template <typename TC>
__device__ __forceinline__ void load_rows(const TC& tc, int64_t b, int64_t e, ChunkRows& rb) {
  const TriSys& s = tc.s;
#pragma unroll
  for (int t = 0; t < kLc - 1; ++t) {
    const int64_t i = (b + t < e) ? b + t : b;
    rb.lo[t] = lo_at(s, i);
    rb.d[t] = d_at(tc, i);
    rb.up[t] = up_at(s, i);
  }
}

// the right-hand sides of those rows for case c: the kLc-1 values back to back
template <typename TC>
__device__ __forceinline__ void load_case_rows(const TC& tc, int c, int64_t b, int64_t e,
                                               double (&r)[kLc - 1]) {
#pragma unroll
  for (int t = 0; t < kLc - 1; ++t) r[t] = r_at(tc, c, (b + t < e) ? b + t : b);
}

// chunk j: interior unknowns [j*kLc, min(j*kLc + kLc-1, m)), never empty for j < nc = ceil(m / kLc); es[nc] once,
// ec[nlive][nc] per case
template <int NC, typename TC>
__global__ __launch_bounds__(kBlock) void tri_condense_kernel(TC tc, int64_t nc,
                                                              ChunkEndsShared* __restrict__ es,
                                                              ChunkEndsCase* __restrict__ ec) {
  const TriSys& s = tc.s;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nc) return;
  const int64_t b = j * kLc;
  const int64_t e = (b + kLc - 1 < s.m) ? b + kLc - 1 : s.m;
  const int len = (int)(e - b);
  ChunkRows rb;
  load_rows(tc, b, e, rb);
  double dd[kLc - 1], du[kLc - 1];       // 1/den of the downward and of the upward sweep
  ChunkEndsShared c;
  {  // downward sweep -> values at the last interior unknown; one division per row (1/den), three multiplications
    double den = 1.0 / rb.d[0];
    double v = -rb.lo[0] * den, cp = rb.up[0] * den;
    dd[0] = den;
#pragma unroll
    for (int t = 1; t < kLc - 1; ++t) {
      if (t < len) {
        const double l = rb.lo[t];
        den = 1.0 / (rb.d[t] - l * cp);
        v = (-l * v) * den;
        cp = rb.up[t] * den;
      }
      dd[t] = den;
    }
    c.vL = v;
    c.wL = -cp;               // rhs -up[e-1] e_last  ->  -up[e-1]/den_last  (den holds 1/den)
  }
  {  // upward sweep -> values at the first interior unknown
    double den = 1.0, bp = 0.0, w = 0.0;
#pragma unroll
    for (int t = kLc - 2; t >= 0; --t) {
      if (t < len) {
        if (t == len - 1) {
          den = 1.0 / rb.d[t];
          w = -rb.up[t] * den;
        } else {
          const double u = rb.up[t];
          den = 1.0 / (rb.d[t] - u * bp);
          w = (-u * w) * den;
        }
        bp = rb.lo[t] * den;
      }
      du[t] = den;
    }
    c.wF = w;
    c.vF = -bp;
  }
  es[j] = c;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    double r[kLc - 1];
    load_case_rows(tc, case_of<NC>(tc, q), b, e, r);
    ChunkEndsCase cq;
    {
      double y = r[0] * dd[0];
#pragma unroll
      for (int t = 1; t < kLc - 1; ++t)
        if (t < len) y = (r[t] - rb.lo[t] * y) * dd[t];
      cq.yL = y;
    }
    {
      double y = 0.0;
#pragma unroll
      for (int t = kLc - 2; t >= 0; --t)
        if (t < len) y = (t == len - 1) ? r[t] * du[t] : (r[t] - rb.up[t] * y) * du[t];
      cq.yF = y;
    }
    if (q < tc.nlive) ec[q * nc + j] = cq;
  }
}

// separator j sits at p = j*kLc + kLc-1 < m (j < ns = m / kLc), between chunk j (left) and chunk j+1 (right): one LO,
// D, UP [ns], R[nlive][ns]
template <int NC, typename TC>
__global__ __launch_bounds__(kBlock) void tri_reduce_kernel(TC tc, int64_t ns, int64_t nc,
                                                            const ChunkEndsShared* __restrict__ es,
                                                            const ChunkEndsCase* __restrict__ ec,
                                                            double* __restrict__ LO, double* __restrict__ D,
                                                            double* __restrict__ UP, double* __restrict__ R) {
  const TriSys& s = tc.s;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= ns) return;
  const int64_t p = j * kLc + kLc - 1;
  const double l = s.lo[p];
  const double u = up_at(s, p);
  const bool right = j + 1 < nc;
  const ChunkEndsShared cl = es[j];
  double dd = d_at(tc, p) + l * cl.wL;
  double uu = 0.0;
  if (right) {
    const ChunkEndsShared cr = es[j + 1];
    dd += u * cr.vF;
    uu = u * cr.wF;
  }
  LO[j] = l * cl.vL;
  D[j] = dd;
  UP[j] = uu;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const int c = case_of<NC>(tc, q);
    double rr = r_at(tc, c, p) - l * ec[c * nc + j].yL;
    if (right) rr -= u * ec[c * nc + j + 1].yF;
    if (q < tc.nlive) R[q * ns + j] = rr;
  }
}

// re-solve every chunk with its separator values X[nlive][ns] known; x + q*xs (length m) receives the whole level's
// solution of case q
template <int NC, typename TC>
__global__ __launch_bounds__(kBlock) void tri_expand_kernel(TC tc, int64_t ns, int64_t nc,
                                                            const double* __restrict__ X, double* __restrict__ x,
                                                            int64_t xs) {
  const TriSys& s = tc.s;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nc) return;
  const int64_t b = j * kLc;
  const int64_t e = (b + kLc - 1 < s.m) ? b + kLc - 1 : s.m;
  const int len = (int)(e - b);
  ChunkRows rb;
  load_rows(tc, b, e, rb);
  // the factorisation of the chunk, once: 1/den and the modified upper band of every row stay in registers (kLc-1 = 7
  // of each), so the back substitution of a case touches memory only to store the solution
  double cc[kLc - 1], dn[kLc - 1];
  double c = 0.0, den = 1.0, upl = 0.0;
#pragma unroll
  for (int t = 0; t < kLc - 1; ++t) {
    if (t < len) {
      const double l = rb.lo[t];
      den = 1.0 / (t == 0 ? rb.d[t] : rb.d[t] - l * c);
      c = rb.up[t] * den;
      if (t == len - 1) upl = rb.up[t];
    }
    cc[t] = c;
    dn[t] = den;
  }
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const int cs = case_of<NC>(tc, q);
    const double xl = j > 0 ? X[cs * ns + j - 1] : 0.0;
    const double xr = j < ns ? X[cs * ns + j] : 0.0;
    double r[kLc - 1];
    load_case_rows(tc, cs, b, e, r);
    double yy[kLc - 1];
    double y = 0.0;
#pragma unroll
    for (int t = 0; t < kLc - 1; ++t) {
      if (t < len) {
        double ri = r[t];
        if (t == 0) ri -= rb.lo[t] * xl;
        if (t == len - 1) ri -= upl * xr;
        y = (t == 0 ? ri : ri - rb.lo[t] * y) * dn[t];
      }
      yy[t] = y;
    }
    if (q < tc.nlive) {
      double* xq = x + q * xs;
      double xn = 0.0;
#pragma unroll
      for (int t = kLc - 2; t >= 0; --t) {
        if (t < len) {
          xn = (t == len - 1) ? yy[t] : yy[t] - cc[t] * xn;
          xq[b + t] = xn;
        }
      }
      if (j < ns) xq[b + kLc - 1] = xr;
    }
  }
}

// Parallel cyclic reduction of row i (li, di, ui, rin[NC]) of an m-row system in LDS, all kBase threads of the one
// workgroup together, ceil(log2 m) steps.  Each step eliminates x[i-st] and x[i+st] from row i with the rows st
// away: the new lower band comes from their lower band, the new upper band from their upper band.  The matrix is
// reduced once, every step's two multipliers serve all the cases.  x receives x[i] of every case.
template <int NC>
__device__ __forceinline__ void tri_pcr(double li, double di, double ui, const double (&rin)[NC], int i, int m,
                                        double* lo, double* d, double* up, double (*r)[kBase], double (&x)[NC]) {
  const bool in = i < m;
  double ri[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) ri[q] = rin[q];
  for (int st = 1; st < m; st <<= 1) {
    lo[i] = li;
    d[i] = di;
    up[i] = ui;
#pragma unroll
    for (int q = 0; q < NC; ++q) r[q][i] = ri[q];
    __syncthreads();
    if (in) {
      double nl = 0.0, nu = 0.0;
      if (i - st >= 0) {
        const double al = -li / d[i - st];
        di += al * up[i - st];
#pragma unroll
        for (int q = 0; q < NC; ++q) ri[q] += al * r[q][i - st];
        nl = al * lo[i - st];
      }
      if (i + st < m) {
        const double be = -ui / d[i + st];
        di += be * lo[i + st];
#pragma unroll
        for (int q = 0; q < NC; ++q) ri[q] += be * r[q][i + st];
        nu = be * up[i + st];
      }
      li = nl;
      ui = nu;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NC; ++q) x[q] = ri[q] / di;
}

// Base level (m <= kBase unknowns): parallel cyclic reduction, one workgroup of kBase threads -- a serial Thomas
// sweep by one thread would pay a global-memory round trip per unknown (~100 us for 100 unknowns; this takes a few
// us).  PCR needs no pivoting for the SPD / diagonally dominant systems that reach this level.  One matrix and NC
// right-hand sides in LDS, (3 + NC) * 4 KiB.
// kRefine (the non-symmetric entry): then ONE step of iterative refinement with the residual of the original rows.
// Cyclic reduction computes every unknown by its own chain of eliminations, so the rounding errors of neighbouring
// unknowns are unrelated, and the matrix amplifies such a rough error by |A| in the residual: at 510 unknowns of a
// P1 Laplacian the residual came out at 1.15 times the rounding-level bar the chunked levels meet with room to
// spare (measured on an MI355X).  The correction costs a second reduction of one workgroup, a
// few microseconds.  The symmetric entry does without it: the step would change its bits and its time.
template <int NC, bool kRefine, typename TC>
__global__ __launch_bounds__(kBase) void tri_base_kernel(TC tc, double* __restrict__ x, int64_t xs) {
  const TriSys& s = tc.s;
  __shared__ double lo[kBase], d[kBase], up[kBase], r[NC][kBase];
  const int i = threadIdx.x;
  const int m = (int)s.m;
  const bool in = i < m;
  double li = 0.0, di = 1.0, ui = 0.0, ri[NC], xi[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) ri[q] = 0.0;
  if (in) {
    li = lo_at(s, i);
    di = d_at(tc, i);
    ui = up_at(s, i);
#pragma unroll
    for (int q = 0; q < NC; ++q) ri[q] = r_at(tc, case_of<NC>(tc, q), i);
  }
  tri_pcr<NC>(li, di, ui, ri, i, m, lo, d, up, r, xi);
  if constexpr (kRefine) {
    // case by case, the residual of row i with fused multiply-adds (one rounding each): r - lo x[i-1] - d x[i] -
    // up x[i+1]
#pragma unroll
    for (int q = 0; q < NC; ++q) r[q][i] = xi[q];
    __syncthreads();
    double res[NC], dx[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      res[q] = 0.0;
      if (in) {
        res[q] = fma(-di, xi[q], ri[q]);
        if (i > 0) res[q] = fma(-li, r[q][i - 1], res[q]);
        if (i + 1 < m) res[q] = fma(-ui, r[q][i + 1], res[q]);
      }
    }
    __syncthreads();
    tri_pcr<NC>(li, di, ui, res, i, m, lo, d, up, r, dx);
#pragma unroll
    for (int q = 0; q < NC; ++q) xi[q] += dx[q];
  }
  if (in) {
#pragma unroll
    for (int q = 0; q < NC; ++q)
      if (q < tc.nlive) x[q * xs + i] = xi[q];
  }
}

// u[q][0] = bc[q][0], u[q][ne] = bc[q][1] for all the cases of a call (u0, u1 without bc)
__global__ void tri_ends_kernel(double* u, int64_t ne, int nc, const double* bc, double u0, double u1) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nc) return;
  u[q * (ne + 1)] = bc ? bc[2 * q] : u0;
  u[q * (ne + 1) + ne] = bc ? bc[2 * q + 1] : u1;
}

// the same for a solve with free ends: only a Dirichlet end (f0 / f1 zero) has its value written, a free end is an
// unknown of the solve (bc NULL: zeros)
__global__ void tri_free_ends_kernel(double* u, int64_t ne, int nc, const double* bc, int f0, int f1) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nc) return;
  if (!f0) u[q * (ne + 1)] = bc ? bc[2 * q] : 0.0;
  if (!f1) u[q * (ne + 1) + ne] = bc ? bc[2 * q + 1] : 0.0;
}

// workspace (in doubles) of the levels above the base with K cases in a pass: es[4*nc] + ec[K][2*nc] + LO, D, UP
// [3*ns] + R, X [K][2*ns]
int64_t level_doubles(int64_t m, int64_t K) {
  int64_t tot = 0;
  while (m > kBase) {
    const int64_t nc = (m + kLc - 1) / kLc, ns = m / kLc;
    tot += (4 + 2 * K) * nc + (3 + 2 * K) * ns + 16;
    m = ns;
  }
  return tot + 16;
}

// one level for the NC slots of a pass: case q's solution of this level at x + q*xs (TC: TriCases, or TriCasesFree at
// the top level of a solve with free ends; the reduced system of either is a TriCases)
template <int NC, bool kRefine, typename TC>
hipError_t solve_level(const TC& tc, double* x, int64_t xs, double* work, hipStream_t st) {
  const TriSys& s = tc.s;
  if (s.m <= 0) return hipSuccess;
  if (s.m <= kBase) {
    hipLaunchKernelGGL((tri_base_kernel<NC, kRefine, TC>), dim3(1), dim3((unsigned)kBase), 0, st, tc, x, xs);
    return hipGetLastError();
  }
  const int64_t nc = (s.m + kLc - 1) / kLc, ns = s.m / kLc;
  // (the per-case arrays hold the live cases only: idle slots store nothing, and the workspace of a call with fewer
  // cases than a pass is sized for those)
  const int64_t K = tc.nlive;
  ChunkEndsShared* es = reinterpret_cast<ChunkEndsShared*>(work);
  ChunkEndsCase* ec = reinterpret_cast<ChunkEndsCase*>(es + nc);
  double* LO = reinterpret_cast<double*>(ec + K * nc);
  double* D = LO + ns;
  double* UP = D + ns;
  double* R = UP + ns;
  double* X = R + K * ns;
  double* next = X + K * ns + 16;
  const unsigned gc = (unsigned)((nc + kBlock - 1) / kBlock);
  const unsigned gs = (unsigned)((ns + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((tri_condense_kernel<NC, TC>), dim3(gc), dim3(kBlock), 0, st, tc, nc, es, ec);
  hipLaunchKernelGGL((tri_reduce_kernel<NC, TC>), dim3(gs), dim3(kBlock), 0, st, tc, ns, nc, es, ec, LO, D, UP, R);
  const TriCases red{TriSys{LO, D, UP, R, nullptr, nullptr, 0.0, 0.0, ns}, ns, nullptr, tc.nlive};
  const hipError_t err = solve_level<NC, kRefine>(red, X, ns, next, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((tri_expand_kernel<NC, TC>), dim3(gc), dim3(kBlock), 0, st, tc, ns, nc, X, x, xs);
  return hipGetLastError();
}

// The unknowns of `all` (its s, its stride, the end values of case 0; nlive is set here) for the nc cases that follow
// s.r at that stride, kTriMultiCases to a pass, into x + q*stride; the passes reuse the one workspace in stream order.
// A pass of one case runs the NC = 1 instantiation, a pass of 2 .. kTriMultiCases cases the NC = kTriMultiCases one.
template <bool kRefine, typename TC>
hipError_t solve_passes(const TC& all, int nc, double* x, void* work, hipStream_t st) {
  const int64_t stride = all.rs;
  for (int q0 = 0; q0 < nc; q0 += kTriMultiCases) {
    TC tc = all;
    tc.nlive = nc - q0 < kTriMultiCases ? nc - q0 : kTriMultiCases;
    if (tc.bc) tc.bc += 2 * (int64_t)q0;
    tc.s.r += q0 * stride;
    double* xq = x + q0 * stride;
    const hipError_t err =
        tc.nlive == 1 ? solve_level<1, kRefine>(tc, xq, stride, reinterpret_cast<double*>(work), st)
                      : solve_level<kTriMultiCases, kRefine>(tc, xq, stride, reinterpret_cast<double*>(work), st);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

// u[q][0], u[q][ne] = the end values of case q, then the ne-1 interior unknowns of s into u[q][1 ..], for the nc
// cases that follow s.r at a stride of ne+1.  The end values are bc[nc][2] on the device or, with bc NULL, s.u0 and
// s.u1 for every case.
template <bool kRefine>
hipError_t dirichlet_solve(const TriSys& s, int64_t ne, int nc, const double* bc, double* u, void* work,
                           hipStream_t st) {
  hipLaunchKernelGGL(tri_ends_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, st, u, ne, nc, bc, s.u0, s.u1);
  if (s.m <= 0) return hipGetLastError();
  return solve_passes<kRefine>(TriCases{s, ne + 1, bc, 0}, nc, u + 1, work, st);
}

// The solve with free ends on the bands diag[ne+1], lo[ne], up[ne] (lo[i]: u_i in row i+1, up[i]: u_{i+1} in row i)
// and load[nc][ne+1]: unknown k is node k + sh, sh = 0 with a free left end and 1 with a Dirichlet one, so the band
// pointers are shifted by sh (lo by sh - 1: lo_at never reads entry 0 of a system) and there are ne - 1 + f0 + f1
// unknowns -- at least one unless ne == 1 with two Dirichlet ends.  A Dirichlet end hands its neighbour's row
// lo[0] * value (up[ne-1] * value) as in dirichlet_solve and has its value written by tri_free_ends_kernel.
template <bool kRefine>
hipError_t free_solve(const double* diag, const double* lo, const double* up, const double* load, int64_t ne, int nc,
                      bool f0, bool f1, double k0, double k1, const double* bc, double* u, void* work,
                      hipStream_t st) {
  if (!f0 || !f1)
    hipLaunchKernelGGL(tri_free_ends_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, st, u, ne, nc, bc,
                       (int)f0, (int)f1);
  const int sh = f0 ? 0 : 1;
  const int64_t m = ne - 1 + (f0 ? 1 : 0) + (f1 ? 1 : 0);
  if (m <= 0) return hipGetLastError();
  const TriSys s{lo + sh - 1, diag + sh, up + sh, load + sh, f0 ? nullptr : lo, f1 ? nullptr : up + (ne - 1),
                 0.0,         0.0,       m};
  TriCasesFree all{};
  static_cast<TriCases&>(all) = TriCases{s, ne + 1, bc, 0};
  all.k0 = k0;
  all.k1 = k1;
  all.f0 = f0;
  all.f1 = f1;
  return solve_passes<kRefine>(all, nc, u + sh, work, st);
}

// Periodic ends: node ne is node 0, its value s the one unknown beside the ne - 1 interior
// ones.  With y[q] the Dirichlet solve of case q for the end values (0, 0) -- already in u -- and z the solve with
// zero load for the end values (1, 1), u_int = y + s z, and the seam row
//   (d[0] + d[ne]) s + up[0] u[1] + lo[ne-1] u[ne-1] = load[0] + load[ne]
// gives s: the Schur complement on this one separator.  One thread per case, a plain division, no atomics.
__global__ void tri_seam_kernel(const double* __restrict__ d, const double* __restrict__ lo,
                                const double* __restrict__ up, const double* __restrict__ load,
                                const double* __restrict__ y, const double* __restrict__ z, int64_t ne, int nc,
                                double* __restrict__ s) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nc) return;
  const double* lq = load + q * (ne + 1);
  const double* yq = y + q * (ne + 1);
  const double u0 = up[0], l1 = lo[ne - 1];
  const double num = ((lq[0] + lq[ne]) - u0 * yq[1]) - l1 * yq[ne - 1];
  const double den = ((d[0] + d[ne]) + u0 * z[1]) + l1 * z[ne - 1];
  s[q] = num / den;
}

// u[q] = y[q] + s[q] z in place over the y that the passes wrote, and u[q][0] = u[q][ne] = s[q]; blockIdx.y strides
// over the cases, blockIdx.x over the nodes
__global__ __launch_bounds__(kBlock) void tri_seam_combine_kernel(double* __restrict__ u,
                                                                  const double* __restrict__ z,
                                                                  const double* __restrict__ s, int64_t ne, int nc) {
  for (int q = blockIdx.y; q < nc; q += gridDim.y) {
    const double sq = s[q];
    double* uq = u + q * (ne + 1);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= ne; i += (int64_t)gridDim.x * kBlock)
      uq[i] = (i == 0 || i == ne) ? sq : uq[i] + sq * z[i];
  }
}

// work: the workspace of the Dirichlet passes, then z[ne+1], the zero load [ne+1] and s[nc].  z is solved once per
// call, as a pass of one case with its end values by value; the nc cases then run through solve_passes with zero end
// values, straight into u.
template <bool kRefine>
hipError_t periodic_solve(const double* diag, const double* lo, const double* up, const double* load, int64_t ne,
                          int nc, double* u, void* work, hipStream_t st) {
  double* z = reinterpret_cast<double*>(static_cast<char*>(work) + tridiag_multi_work_bytes(ne, nc));
  double* zero = z + (ne + 1);
  double* s = zero + (ne + 1);
  hipError_t err = hipMemsetAsync(zero, 0, sizeof(double) * (size_t)(ne + 1), st);
  if (err != hipSuccess) return err;
  const TriSys sys{lo, diag + 1, up + 1, zero + 1, lo, up + (ne - 1), 1.0, 1.0, ne - 1};
  err = solve_passes<kRefine>(TriCases{sys, ne + 1, nullptr, 0}, 1, z + 1, work, st);
  if (err != hipSuccess) return err;
  TriSys sy = sys;
  sy.r = load + 1;
  sy.u0 = sy.u1 = 0.0;
  err = solve_passes<kRefine>(TriCases{sy, ne + 1, nullptr, 0}, nc, u + 1, work, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(tri_seam_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, st, diag, lo, up, load, u, z, ne,
                     nc, s);
  const int64_t gx = (ne + kBlock) / kBlock;
  hipLaunchKernelGGL(tri_seam_combine_kernel, dim3((unsigned)(gx < 4096 ? gx : 4096), (unsigned)(nc < 64 ? nc : 64)),
                     dim3(kBlock), 0, st, u, z, s, ne, nc);
  return hipGetLastError();
}

}  // namespace

// it grows with nc up to kTriMultiCases, the cases of one pass
int64_t tridiag_multi_work_bytes(int64_t ne, int nc) {
  const int64_t m = ne > 1 ? ne - 1 : 0;
  return 8 * level_doubles(m, nc < kTriMultiCases ? (nc > 1 ? nc : 1) : kTriMultiCases) + 256;
}

int64_t tridiag_work_bytes(int64_t ne) { return tridiag_multi_work_bytes(ne, 1); }

// sized for two free ends, ne + 1 unknowns, whatever the kinds of a call are
int64_t tridiag_bc_work_bytes(int64_t ne, int nc) {
  return 8 * level_doubles(ne + 1, nc < kTriMultiCases ? (nc > 1 ? nc : 1) : kTriMultiCases) + 256;
}

// interior unknown k <-> node k+1: lo = off[k] (u_k in row k+1), d = diag[k+1], up = off[k+1], r = load[k+1]; the end
// rows lose off[0] * u[0] and off[ne-1] * u[ne] to the right-hand side
hipError_t tridiag_dirichlet_solve(const double* diag, const double* off, const double* load, int64_t ne, int nc,
                                   const double* bc, double u0, double u1, double* u, void* work, hipStream_t st) {
  const TriSys s{off, diag + 1, off + 1, load + 1, off, off + (ne - 1), u0, u1, ne - 1};
  return dirichlet_solve<false>(s, ne, nc, bc, u, work, st);
}

// the same with lo = sub[k], up = sup[k+1]; the end rows lose sub[0] * u[0] and sup[ne-1] * u[ne]
hipError_t tridiag_ns_dirichlet_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                      int64_t ne, int nc, const double* bc, double u0, double u1, double* u,
                                      void* work, hipStream_t st) {
  const TriSys s{sub, diag + 1, sup + 1, load + 1, sub, sup + (ne - 1), u0, u1, ne - 1};
  return dirichlet_solve<true>(s, ne, nc, bc, u, work, st);
}

// free ends: the symmetric bands (lo = up = off) and the non-symmetric ones
hipError_t tridiag_bc_solve(const double* diag, const double* off, const double* load, int64_t ne, int nc, bool f0,
                            bool f1, double k0, double k1, const double* bc, double* u, void* work, hipStream_t st) {
  return free_solve<false>(diag, off, off, load, ne, nc, f0, f1, k0, k1, bc, u, work, st);
}

hipError_t tridiag_ns_bc_solve(const double* diag, const double* sub, const double* sup, const double* load,
                               int64_t ne, int nc, bool f0, bool f1, double k0, double k1, const double* bc,
                               double* u, void* work, hipStream_t st) {
  return free_solve<true>(diag, sub, sup, load, ne, nc, f0, f1, k0, k1, bc, u, work, st);
}

// periodic ends: the workspace of the Dirichlet passes + z and its zero load (16 (ne+1) bytes) + s[nc]
int64_t tridiag_periodic_work_bytes(int64_t ne, int nc) {
  return tridiag_multi_work_bytes(ne, nc) + 16 * (ne + 1) + 8 * (int64_t)(nc > 1 ? nc : 1) + 256;
}

hipError_t tridiag_periodic_solve(const double* diag, const double* off, const double* load, int64_t ne, int nc,
                                  double* u, void* work, hipStream_t st) {
  return periodic_solve<false>(diag, off, off, load, ne, nc, u, work, st);
}

hipError_t tridiag_ns_periodic_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                     int64_t ne, int nc, double* u, void* work, hipStream_t st) {
  return periodic_solve<true>(diag, sub, sup, load, ne, nc, u, work, st);
}

}  // namespace lssvr
