// Sturm-Liouville eigenproblems  -(a u')' + c u = lambda rho u  on the P1 mesh: the kernels of
// block inverse iteration with a fixed shift sigma and a Rayleigh-Ritz step.  K holds the bands of
// lssvr_p1_assemble_react (c_quad = c), M those of the same entry with a_quad = 0 and c_quad = rho; the shifted solve
// Z = (K - sigma M)^-1 Y is lssvr_tridiag_bc_solve_multi or lssvr_tridiag_pivot_solve_multi.  This file adds what goes
// around it, with no host round trip per step:
//   apply    MZ = M Z, KZ = K Z and the Gram matrices A = Z^T K Z, B = Z^T M Z
//   ritz     theta ascending in |theta - sigma| and Q with Q^T A Q = diag theta, Q^T B Q = I  (one thread; also on the host)
//   rotate   X = Z Q, Y = (MZ) Q, res2_j = |(KZ) Q_j - theta_j (MZ) Q_j|^2 and |X_j|^2, every column signed
//   count    the negative pivots of LDL^T (K - s M) for ns shifts (Sturm count; one lane per shift; also on the host)
//   rayleigh the Rayleigh quotient of an enhanced mode W[ne][M]
// Vectors are case-major [nb][ne+1], the layout of the multi solvers.  The unknowns are the nodes sh .. hi-1 (a
// Dirichlet end is no unknown); every output row outside them is exactly 0, and input rows outside them are not read.
// A Robin end adds kappa to K's end diagonal by value; the bands are read only.
//
// Reductions: a fixed two-stage order -- wave (shuffles, halving offsets), then the block's waves in order, into
// `work`; then one finishing workgroup per sum adds the blocks' partials, strided in index order and through the same
// tree.  No atomics: bitwise reproducible.
// FP64, -ffp-contract=off, no LDS beyond the reductions' staging, no scratch.
#include <cfloat>
#include <cmath>

#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_adapt.hpp"

#define LSSVR_EIG_HD __host__ __device__ __forceinline__

namespace lssvr {

namespace {

// nodes per workgroup (four waves) and the grid cap of the grid-stride loops: the partials of a reduction are
// kEigMaxBlocks rows at most
constexpr int kEigBlock = 256;
constexpr int kEigMaxBlocks = 1024;
constexpr int kEigWaves = kEigBlock / 64;
// elements per workgroup of the Rayleigh kernel (one wave, as adapt_goal.hip: the staged rows and the table fit LDS)
constexpr int kRayBlock = 64;

int64_t eig_blocks(int64_t n) {
  const int64_t b = (n + kEigBlock - 1) / kEigBlock;
  return b < 1 ? 1 : (b < kEigMaxBlocks ? b : kEigMaxBlocks);
}
int64_t ray_blocks(int64_t ne) { return chunk_blocks<kRayBlock>(ne); }

// The NS sums of a workgroup of kEigBlock threads -> out[0 .. NS): lanes by shuffles at offsets 32 .. 1, then the four
// waves in order.  Every thread of the workgroup calls it.  red: kEigWaves * NS doubles of LDS.
template <int NS, int BLOCK>
__device__ __forceinline__ void eig_block_sums(double (&v)[NS], double* __restrict__ red, double* __restrict__ out) {
  constexpr int kW = BLOCK / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[s] += __shfl_down(v[s], off, 64);
    if (lane == 0) red[wave * NS + s] = v[s];
  }
  __syncthreads();
  for (int t = tid; t < NS; t += BLOCK) {
    double s = red[t];
    for (int w = 1; w < kW; ++w) s += red[w * NS + t];
    out[t] = s;
  }
}

// One workgroup per sum t = blockIdx.x < ns: thread i adds part[i][t], part[i + kEigBlock][t], ... in index order, then
// the workgroup's fixed tree (eig_block_sums) -- the same order in every run.  sym > 0: the ns = sym (sym + 1) sums are
// the packed triangles of two symmetric sym x sym matrices (tri(i, j), j <= i), written out in full, A then B.
__global__ __launch_bounds__(kEigBlock) void eig_finish_kernel(const double* __restrict__ part, int nblk, int ns,
                                                                double* __restrict__ out, int sym) {
  __shared__ double red[kEigWaves];
  __shared__ double total;
  const int t = blockIdx.x;
  double v[1] = {0.0};
  for (int b = threadIdx.x; b < nblk; b += kEigBlock) v[0] += part[(int64_t)b * ns + t];
  eig_block_sums<1, kEigBlock>(v, red, &total);
  if (threadIdx.x != 0) return;
  const double s = total;
  if (sym <= 0) {
    out[t] = s;
    return;
  }
  const int half = ns / 2, which = t / half, r = t - which * half;
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= r) ++i;
  const int j = r - i * (i + 1) / 2;
  double* m = out + which * sym * sym;
  m[i * sym + j] = s;
  m[j * sym + i] = s;
}

// the bands of K and M, the ends and the range of the unknowns
struct EigBands {
  const double* kd;
  const double* ko;
  const double* md;
  const double* mo;
  double k0, k1;
  int f0, f1;
  int64_t ne;
};
LSSVR_EIG_HD int64_t eig_first(int f0) { return f0 ? 0 : 1; }
LSSVR_EIG_HD int64_t eig_last(int f1, int64_t ne) { return f1 ? ne + 1 : ne; }      // one past the last unknown
LSSVR_EIG_HD double eig_kdiag(const EigBands& b, int64_t i) {
  double v = b.kd[i];
  if (i == 0 && b.f0) v += b.k0;
  if (i == b.ne && b.f1) v += b.k1;
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(kEigBlock) void eig_apply_kernel(EigBands b, const double* __restrict__ Z,
                                                               double* __restrict__ MZ, double* __restrict__ KZ,
                                                               double* __restrict__ part) {
  constexpr int NT = NB * (NB + 1) / 2, NS = 2 * NT;
  __shared__ double red[kEigWaves * NS];
  const int64_t n = b.ne + 1, sh = eig_first(b.f0), hi = eig_last(b.f1, b.ne);
  double g[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) g[s] = 0.0;
  for (int64_t i0 = (int64_t)blockIdx.x * kEigBlock; i0 < n; i0 += (int64_t)gridDim.x * kEigBlock) {
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < n, unk = in && i >= sh && i < hi;
    const bool hasl = unk && i > sh, hasr = unk && i + 1 < hi;
    const double dk = unk ? eig_kdiag(b, i) : 0.0, dm = unk ? b.md[i] : 0.0;
    const double lk = hasl ? b.ko[i - 1] : 0.0, lm = hasl ? b.mo[i - 1] : 0.0;
    const double uk = hasr ? b.ko[i] : 0.0, um = hasr ? b.mo[i] : 0.0;
    double z[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const double* zc = Z + c * n;
      const double z0 = unk ? zc[i] : 0.0, zl = hasl ? zc[i - 1] : 0.0, zr = hasr ? zc[i + 1] : 0.0;
      const double kz = (lk * zl + dk * z0) + uk * zr;
      const double mz = (lm * zl + dm * z0) + um * zr;
      if (in) {
        KZ[c * n + i] = kz;
        MZ[c * n + i] = mz;
      }
      z[c] = z0;
#pragma unroll
      for (int c2 = 0; c2 <= c; ++c2) {
        g[tri(c, c2)] += z[c2] * kz;
        g[NT + tri(c, c2)] += z[c2] * mz;
      }
    }
  }
  eig_block_sums<NS, kEigBlock>(g, red, part + (int64_t)blockIdx.x * NS);
}

// ---------------------------------------------------------------------------------------------------------------------
// rotate
// ---------------------------------------------------------------------------------------------------------------------
// column j of (v_0 .. v_{NB-1}) Q: one expression for the vectors and for the value that decides a column's sign
template <int NB>
__device__ __forceinline__ double eig_combine(const double (&v)[NB], const double* q, int j) {
  double s = v[0] * q[j];
#pragma unroll
  for (int c = 1; c < NB; ++c) s += v[c] * q[c * NB + j];
  return s;
}

template <int NB>
__global__ __launch_bounds__(kEigBlock) void eig_rotate_kernel(const double* __restrict__ Z,
                                                                const double* __restrict__ MZ,
                                                                const double* __restrict__ KZ,
                                                                const double* __restrict__ Q,
                                                                const double* __restrict__ theta, int64_t ne, int f0,
                                                                int f1, double* __restrict__ X, double* __restrict__ Y,
                                                                double* __restrict__ part) {
  constexpr int NS = 2 * NB;
  __shared__ double red[kEigWaves * NS];
  __shared__ double sq[NB * NB], sth[NB], sgn[NB];
  const int tid = threadIdx.x;
  const int64_t n = ne + 1, sh = eig_first(f0), hi = eig_last(f1, ne);
  if (tid < NB) {
    // the first unknown's value of column tid, as the thread that owns that node computes it below
    double zf[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) zf[c] = Z[c * n + sh];
    sgn[tid] = eig_combine<NB>(zf, Q, tid) < 0.0 ? -1.0 : 1.0;
    sth[tid] = theta[tid];
  }
  __syncthreads();
  for (int t = tid; t < NB * NB; t += kEigBlock) sq[t] = Q[t] * sgn[t % NB];
  __syncthreads();
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  for (int64_t i0 = (int64_t)blockIdx.x * kEigBlock; i0 < n; i0 += (int64_t)gridDim.x * kEigBlock) {
    const int64_t i = i0 + tid;
    const bool in = i < n, unk = in && i >= sh && i < hi;
    double v[NB], y[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) v[c] = unk ? Z[c * n + i] : 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double x = eig_combine<NB>(v, sq, j);
      if (in) X[j * n + i] = x;
      acc[NB + j] += x * x;
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) v[c] = unk ? MZ[c * n + i] : 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      y[j] = eig_combine<NB>(v, sq, j);
      if (in) Y[j * n + i] = y[j];
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) v[c] = unk ? KZ[c * n + i] : 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double r = eig_combine<NB>(v, sq, j) - sth[j] * y[j];
      acc[j] += r * r;
    }
  }
  eig_block_sums<NS, kEigBlock>(acc, red, part + (int64_t)blockIdx.x * NS);
}

// ---------------------------------------------------------------------------------------------------------------------
// ritz: the nb x nb pencil (A, B), nb <= kEigMaxNb, by one thread; the same text runs on the host
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kEigMaxNb = 8;
// sweeps of the cyclic Jacobi iteration at most (it ends with the first sweep that rotates nothing; an 8 x 8 matrix
// takes 6 to 8, and a few more until the last off-diagonal entries underflow)
constexpr int kRitzSweeps = 20;
// a Cholesky pivot of B at or below this fraction of B's own diagonal entry is a dependent column: the rounding of
// the pivot itself is a few 2^-53 of that entry
constexpr double kRitzDepTol = 0x1p-46;
// doubles / ints of workspace eig_ritz needs
constexpr int kRitzWork = 4 * kEigMaxNb * kEigMaxNb + 3 * kEigMaxNb;

// sqrt(x) for finite x > 0 from +, *, / and exact scalings only, so that host and device agree bit for bit: x = m 4^e
// with m in [0.5, 2), a linear first guess (3 % off at most) and five Newton steps (the fourth is already at rounding)
LSSVR_EIG_HD double eig_sqrt(double x) {
  if (!(x > 0.0)) return 0.0;
  int e;
  double m = frexp(x, &e);
  if (e & 1) {
    m *= 2.0;
    e -= 1;
  }
  double y = 0.485 + 0.485 * m;
#pragma unroll
  for (int it = 0; it < 5; ++it) y = 0.5 * (y + m / y);
  return ldexp(y, e / 2);
}

// A, B: nb x nb row-major (symmetric; B positive definite up to dependent columns) -> theta[nb], Q[nb][nb] row-major
// (column j the vector of theta[j]), ordered by |theta - sigma| ascending (ties by index).  Returns the number of
// dependent columns of B; their vectors are zero, their theta 0, and they come last.  ws: kRitzWork doubles, iw:
// kEigMaxNb ints (LDS on the device: arrays indexed at run time must not live in registers).
LSSVR_EIG_HD int eig_ritz(const double* A, const double* B, int nb, double sigma, double* theta, double* Q, double* ws,
                          int* iw) {
  constexpr int LD = kEigMaxNb;
  double* C = ws;
  double* L = C + LD * LD;
  double* V = L + LD * LD;
  double* T = V + LD * LD;
  double* rinv = T + LD * LD;
  double* key = rinv + LD;
  double* th = key + LD;
  int bad = 0;
  // B = L L^T
  for (int j = 0; j < nb; ++j) {
    double d = B[j * nb + j];
    for (int k = 0; k < j; ++k) d -= L[j * LD + k] * L[j * LD + k];
    const bool ok = d > kRitzDepTol * B[j * nb + j] && d <= DBL_MAX;
    const double ljj = ok ? eig_sqrt(d) : 0.0;
    rinv[j] = ok ? 1.0 / ljj : 0.0;
    bad += ok ? 0 : 1;
    L[j * LD + j] = ljj;
    for (int i = j + 1; i < nb; ++i) {
      double s = B[i * nb + j];
      for (int k = 0; k < j; ++k) s -= L[i * LD + k] * L[j * LD + k];
      L[i * LD + j] = s * rinv[j];
    }
  }
  // T = L^-1 A, C = T L^-T; a dependent column gives a zero row and column
  for (int c = 0; c < nb; ++c)
    for (int i = 0; i < nb; ++i) {
      double s = A[i * nb + c];
      for (int k = 0; k < i; ++k) s -= L[i * LD + k] * T[k * LD + c];
      T[i * LD + c] = s * rinv[i];
    }
  for (int r = 0; r < nb; ++r)
    for (int j = 0; j < nb; ++j) {
      double s = T[r * LD + j];
      for (int k = 0; k < j; ++k) s -= L[j * LD + k] * C[r * LD + k];
      C[r * LD + j] = s * rinv[j];
    }
  for (int i = 0; i < nb; ++i)
    for (int j = 0; j < nb; ++j) {
      if (j < i) C[i * LD + j] = C[j * LD + i] = 0.5 * (C[i * LD + j] + C[j * LD + i]);
      V[i * LD + j] = i == j ? 1.0 : 0.0;
    }
  // cyclic Jacobi: C -> diag, V the rotations
  for (int sweep = 0; sweep < kRitzSweeps; ++sweep) {
    int rotated = 0;
    for (int p = 0; p + 1 < nb; ++p)
      for (int q = p + 1; q < nb; ++q) {
        const double apq = C[p * LD + q];
        if (apq == 0.0) continue;
        const double app = C[p * LD + p], aqq = C[q * LD + q], g = fabs(apq);
        if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
          C[p * LD + q] = C[q * LD + p] = 0.0;
          continue;
        }
        const double tau = (aqq - app) / (2.0 * apq);
        double t;
        if (fabs(tau) >= 0x1p500)
          t = 0.5 / tau;
        else
          t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + eig_sqrt(1.0 + tau * tau));
        const double cs = 1.0 / eig_sqrt(1.0 + t * t), sn = t * cs;
        C[p * LD + p] = app - t * apq;
        C[q * LD + q] = aqq + t * apq;
        C[p * LD + q] = C[q * LD + p] = 0.0;
        for (int r = 0; r < nb; ++r) {
          if (r != p && r != q) {
            const double arp = C[r * LD + p], arq = C[r * LD + q];
            C[r * LD + p] = C[p * LD + r] = cs * arp - sn * arq;
            C[r * LD + q] = C[q * LD + r] = sn * arp + cs * arq;
          }
          const double vrp = V[r * LD + p], vrq = V[r * LD + q];
          V[r * LD + p] = cs * vrp - sn * vrq;
          V[r * LD + q] = sn * vrp + cs * vrq;
        }
        ++rotated;
      }
    if (!rotated) break;
  }
  // T = L^-T V (back substitution, column by column); the order
  for (int j = 0; j < nb; ++j) {
    for (int i = nb - 1; i >= 0; --i) {
      double s = V[i * LD + j];
      for (int k = i + 1; k < nb; ++k) s -= L[k * LD + i] * T[k * LD + j];
      T[i * LD + j] = s * rinv[i];
    }
    const bool dep = rinv[j] == 0.0;
    th[j] = dep ? 0.0 : C[j * LD + j];
    key[j] = dep ? INFINITY : fabs(th[j] - sigma);
    iw[j] = j;
  }
  for (int j = 1; j < nb; ++j) {      // insertion sort: stable
    const int pj = iw[j];
    int k = j - 1;
    while (k >= 0 && key[iw[k]] > key[pj]) {
      iw[k + 1] = iw[k];
      --k;
    }
    iw[k + 1] = pj;
  }
  for (int j = 0; j < nb; ++j) {
    theta[j] = th[iw[j]];
    for (int i = 0; i < nb; ++i) Q[i * nb + j] = T[i * LD + iw[j]];
  }
  return bad;
}

__global__ __launch_bounds__(64) void eig_ritz_kernel(const double* __restrict__ A, const double* __restrict__ B, int nb,
                                                       double sigma, double* __restrict__ theta, double* __restrict__ Q,
                                                       int* __restrict__ info) {
  __shared__ double ws[kRitzWork];
  __shared__ int iw[kEigMaxNb];
  if (threadIdx.x == 0) {
    const int bad = eig_ritz(A, B, nb, sigma, theta, Q, ws, iw);
    if (info) info[0] = bad;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// count
// ---------------------------------------------------------------------------------------------------------------------
// the negative pivots of LDL^T (K - s M) over the unknowns: d_i = alpha_i - beta_{i-1}^2 / d_{i-1}, a pivot with
// |d| < pivmin becomes -pivmin (dstebz)
LSSVR_EIG_HD int eig_count(const EigBands& b, double s, double pivmin) {
  const int64_t sh = eig_first(b.f0), hi = eig_last(b.f1, b.ne);
  if (hi <= sh) return 0;
  double d = eig_kdiag(b, sh) - s * b.md[sh];
  if (fabs(d) < pivmin) d = -pivmin;
  int cnt = d < 0.0 ? 1 : 0;
  for (int64_t i = sh + 1; i < hi; ++i) {
    const double be = b.ko[i - 1] - s * b.mo[i - 1];
    d = (eig_kdiag(b, i) - s * b.md[i]) - be * be / d;
    if (fabs(d) < pivmin) d = -pivmin;
    cnt += d < 0.0 ? 1 : 0;
  }
  return cnt;
}

__global__ __launch_bounds__(64) void eig_count_kernel(EigBands b, const double* __restrict__ shifts, int ns,
                                                        double pivmin, int* __restrict__ counts) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= ns) return;
  counts[t] = eig_count(b, shifts[t], pivmin);
}

// ---------------------------------------------------------------------------------------------------------------------
// rayleigh
// ---------------------------------------------------------------------------------------------------------------------
struct RayArgs {
  const double* x;
  const double* W;
  int64_t ne;
  int M, nq, ms;
  const double* a_values;
  const double* c_values;
  const double* rho_values;
  int kind[2];
  double kappa[2];
  double* work;
};

// sum_k c_k (+-1)^k: the element's value at its left (side 0) or right (side 1) end
template <int MT>
__device__ __forceinline__ double ray_end_value(const double (&c)[MT], int side) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < MT; ++k) s = fma(c[k], (side == 0 && (k & 1)) ? -1.0 : 1.0, s);
  return s;
}

// A lane per element, the rows staged through LDS at the odd stride (adapt_goal.hip's structure).  Dynamic LDS:
// T[nq*MT] triples {P_k', P_k'', P_k}(xi_q) of fill_table (P_k'' is not used) | wt[nq] | rows[kRayBlock*ms] | red[3].
// Per block {numerator, denominator, sum |terms| of the numerator} -> work[3*blockIdx.x ..].
template <int MT, bool PM>
__global__ __launch_bounds__(kRayBlock) void eig_rayleigh_kernel(RayArgs p, GaussRuleN g) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nq = p.nq, M = p.M, ms = p.ms;
  const int64_t ne = p.ne;
  double* T = lds;
  double* swt = T + 3 * nq * MT;
  double* rows = swt + nq;
  double* red = rows + kRayBlock * ms;
  if (tid < nq) {
    swt[tid] = g.wt[tid];
    fill_table<MT, 3>(T + 3 * tid * MT, g.xi[tid], M);
  }
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t c0 = (int64_t)blockIdx.x * kRayBlock; c0 < ne; c0 += (int64_t)gridDim.x * kRayBlock) {
    const int nrow = (int)(ne - c0 < kRayBlock ? ne - c0 : kRayBlock);
    stage_rows<kRayBlock>(rows, p.W + c0 * M, nrow * M, M, ms, tid);
    __syncthreads();
    const int64_t e = c0 + tid;
    if (tid < nrow) {
      double c[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k) c[k] = k < M ? rows[tid * ms + k] : 0.0;
      const DomainMap dm = map_params(p.x[e], p.x[e + 1]);
      double num = 0.0, den = 0.0, mag = 0.0;
#pragma unroll 1
      for (int q = 0; q < nq; ++q) {
        const double* Tq = T + 3 * q * MT;
        double s1 = 0.0, s0 = c[0];
#pragma unroll
        for (int k = 1; k < MT; ++k) {
          s1 = fma(c[k], Tq[3 * k], s1);
          s0 = fma(c[k], Tq[3 * k + 2], s0);
        }
        const int64_t i = PM ? (int64_t)q * ne + e : e * nq + q;
        const double du = s1 * dm.scl;
        const double ta = p.a_values[i] * (du * du), tc = p.c_values[i] * (s0 * s0);
        num = fma(swt[q], ta + tc, num);
        mag = fma(swt[q], fabs(ta) + fabs(tc), mag);
        den = fma(swt[q], p.rho_values[i] * (s0 * s0), den);
      }
      const double half = 0.5 * dm.oldlen;
      num *= half;
      den *= half;
      mag *= half;
      // a Robin end a du/dn + kappa u = 0 adds kappa u(x_end)^2 to the form; ne == 1 has both ends in this element
      if (e == 0 && p.kind[0] == 1) {
        const double v = ray_end_value<MT>(c, 0), tk = p.kappa[0] * (v * v);
        num += tk;
        mag += fabs(tk);
      }
      if (e + 1 == ne && p.kind[1] == 1) {
        const double v = ray_end_value<MT>(c, 1), tk = p.kappa[1] * (v * v);
        num += tk;
        mag += fabs(tk);
      }
      acc[0] += num;
      acc[1] += den;
      acc[2] += mag;
    }
    __syncthreads();      // rows are rewritten by the next chunk
  }
  eig_block_sums<3, kRayBlock>(acc, red, p.work + 3 * (int64_t)blockIdx.x);
}

template <int NB>
hipError_t launch_apply(const EigBands& b, const double* Z, double* MZ, double* KZ, double* gram, double* work,
                        hipStream_t st) {
  const int64_t nblk = eig_blocks(b.ne + 1);
  hipLaunchKernelGGL((eig_apply_kernel<NB>), dim3((unsigned)nblk), dim3(kEigBlock), 0, st, b, Z, MZ, KZ, work);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(eig_finish_kernel, dim3(NB * (NB + 1)), dim3(kEigBlock), 0, st, work, (int)nblk, NB * (NB + 1), gram,
                     NB);
  return hipGetLastError();
}

template <int NB>
hipError_t launch_rotate(const double* Z, const double* MZ, const double* KZ, const double* Q, const double* theta,
                         int64_t ne, int f0, int f1, double* X, double* Y, double* res2, double* work, hipStream_t st) {
  const int64_t nblk = eig_blocks(ne + 1);
  hipLaunchKernelGGL((eig_rotate_kernel<NB>), dim3((unsigned)nblk), dim3(kEigBlock), 0, st, Z, MZ, KZ, Q, theta, ne, f0,
                     f1, X, Y, work);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(eig_finish_kernel, dim3(2 * NB), dim3(kEigBlock), 0, st, work, (int)nblk, 2 * NB, res2, 0);
  return hipGetLastError();
}

}  // namespace

int64_t eig_work_bytes(int64_t ne, int nb) {
  if (ne < 0 || nb < 1) return 0;
  if (nb > kEigMaxNb) nb = kEigMaxNb;
  const int64_t grams = eig_blocks(ne + 1) * nb * (nb + 1), ray = 3 * ray_blocks(ne);
  return 8 * ((grams > ray ? grams : ray) + 16);
}

#define LSSVR_EIG_NB_SWITCH(nb, CALL)  \
  switch (nb) {                        \
    case 1: return CALL(1);            \
    case 2: return CALL(2);            \
    case 3: return CALL(3);            \
    case 4: return CALL(4);            \
    case 5: return CALL(5);            \
    case 6: return CALL(6);            \
    case 7: return CALL(7);            \
    case 8: return CALL(8);            \
    default: return hipErrorInvalidValue; \
  }

hipError_t eig_apply(const EigArgs& a, const double* Z, double* MZ, double* KZ, double* gram, void* work,
                     hipStream_t st) {
  const EigBands b{a.kdiag, a.koff, a.mdiag, a.moff, a.k0, a.k1, a.f0 ? 1 : 0, a.f1 ? 1 : 0, a.ne};
  double* w = reinterpret_cast<double*>(work);
#define LSSVR_EIG_APPLY(N) launch_apply<N>(b, Z, MZ, KZ, gram, w, st)
  LSSVR_EIG_NB_SWITCH(a.nb, LSSVR_EIG_APPLY)
#undef LSSVR_EIG_APPLY
}

hipError_t eig_rotate(const double* Z, const double* MZ, const double* KZ, const double* Q, const double* theta,
                      int64_t ne, int nb, bool f0, bool f1, double* X, double* Y, double* res2, void* work,
                      hipStream_t st) {
  double* w = reinterpret_cast<double*>(work);
#define LSSVR_EIG_ROTATE(N) launch_rotate<N>(Z, MZ, KZ, Q, theta, ne, f0 ? 1 : 0, f1 ? 1 : 0, X, Y, res2, w, st)
  LSSVR_EIG_NB_SWITCH(nb, LSSVR_EIG_ROTATE)
#undef LSSVR_EIG_ROTATE
}

hipError_t eig_ritz_device(const double* A, const double* B, int nb, double sigma, double* theta, double* Q,
                           int32_t* info, hipStream_t st) {
  hipLaunchKernelGGL(eig_ritz_kernel, dim3(1), dim3(64), 0, st, A, B, nb, sigma, theta, Q, reinterpret_cast<int*>(info));
  return hipGetLastError();
}

int eig_ritz_host(const double* A, const double* B, int nb, double sigma, double* theta, double* Q) {
  double ws[kRitzWork];
  int iw[kEigMaxNb];
  return eig_ritz(A, B, nb, sigma, theta, Q, ws, iw);
}

hipError_t eig_count_device(const EigArgs& a, const double* shifts, int ns, double pivmin, int32_t* counts,
                            hipStream_t st) {
  const EigBands b{a.kdiag, a.koff, a.mdiag, a.moff, a.k0, a.k1, a.f0 ? 1 : 0, a.f1 ? 1 : 0, a.ne};
  hipLaunchKernelGGL(eig_count_kernel, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, st, b, shifts, ns, pivmin,
                     reinterpret_cast<int*>(counts));
  return hipGetLastError();
}

void eig_count_host(const EigArgs& a, const double* shifts, int ns, double pivmin, int32_t* counts) {
  const EigBands b{a.kdiag, a.koff, a.mdiag, a.moff, a.k0, a.k1, a.f0 ? 1 : 0, a.f1 ? 1 : 0, a.ne};
  for (int t = 0; t < ns; ++t) counts[t] = eig_count(b, shifts[t], pivmin);
}

hipError_t eig_rayleigh(const EigRayleighArgs& a, bool point_major, double* out3, hipStream_t st) {
  GaussRuleN g{};
  if (!gauss_rule(a.nq, g.xi, g.wt)) return hipErrorInvalidValue;
  RayArgs p{};
  p.x = a.x;
  p.W = a.W;
  p.ne = a.ne;
  p.M = a.M;
  p.nq = a.nq;
  p.ms = a.M | 1;                                   // odd row stride: conflict-free ds_read_b64
  p.a_values = a.a_values;
  p.c_values = a.c_values;
  p.rho_values = a.rho_values;
  for (int i = 0; i < 2; ++i) {
    p.kind[i] = a.kind[i];
    p.kappa[i] = a.kappa[i];
  }
  p.work = reinterpret_cast<double*>(a.work);
  const int64_t nblk = ray_blocks(a.ne);
  const int MT = a.M <= 12 ? 12 : (a.M <= 22 ? 22 : 33);
  const size_t lds = sizeof(double) * ((size_t)a.nq * (3 * MT + 1) + (size_t)kRayBlock * p.ms + 3);
  void (*kernel)(RayArgs, GaussRuleN) =
      MT == 12   ? (point_major ? eig_rayleigh_kernel<12, true> : eig_rayleigh_kernel<12, false>)
      : MT == 22 ? (point_major ? eig_rayleigh_kernel<22, true> : eig_rayleigh_kernel<22, false>)
                 : (point_major ? eig_rayleigh_kernel<33, true> : eig_rayleigh_kernel<33, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(kRayBlock), lds, st, p, g);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(eig_finish_kernel, dim3(3), dim3(kEigBlock), 0, st, p.work, (int)nblk, 3, out3, 0);
  return hipGetLastError();
}

}  // namespace lssvr
