// What the estimator / refinement kernels (adapt.hip), the smoothness / grouping kernels (adapt_hp.hip) and the
// goal-oriented estimator (adapt_goal.hip) share: the chunk geometry, the coalesced staging of W rows through LDS, the
// marking predicate, the one-workgroup exclusive scan, the deterministic reduction (per-block tree + finish kernel),
// and the Legendre table, end values and flux jumps of the estimators.
#pragma once
#include <cmath>
#include <cstdint>

#include "lssvr_device.hpp"

namespace lssvr {

constexpr int kEstBlock = 128;          // elements per workgroup chunk (two waves)
constexpr int kEstMaxBlocks = 4096;     // grid cap: partials of the reduction in `work`

// workgroups of a grid-stride launch over chunks of BLOCK elements
template <int BLOCK>
inline int64_t chunk_blocks(int64_t ne) {
  const int64_t b = (ne + BLOCK - 1) / BLOCK;
  return b < 1 ? 1 : (b < kEstMaxBlocks ? b : kEstMaxBlocks);
}
inline int64_t est_blocks(int64_t ne) { return chunk_blocks<kEstBlock>(ne); }
inline int64_t ref_blocks(int64_t ne) {
  const int64_t b = (ne + kBlock - 1) / kBlock;
  return b < 1 ? 1 : b;
}

// the chunk's contiguous `total` = nrow*M doubles of W from `src` (coalesced) into LDS rows of odd stride ms;
// column stepping: i += BLOCK  ->  (row, col) += (BLOCK / M, BLOCK % M).  BLOCK: the workgroup size.
template <int BLOCK = kEstBlock>
__device__ __forceinline__ void stage_rows(double* __restrict__ rows, const double* __restrict__ src, int total,
                                           int M, int ms, int tid) {
  const int qM = BLOCK / M, rM = BLOCK - (BLOCK / M) * M;
  int r = tid / M, col = tid - (tid / M) * M;
  for (int i = tid; i < total; i += BLOCK) {
    rows[r * ms + col] = src[i];
    r += qM;
    col += rM;
    if (col >= M) {
      col -= M;
      ++r;
    }
  }
}

// the indicator half of the marking rule: eta2 is non-finite, or max > 0 and eta2 >= theta^2 * max;
// mx = the device max of the finite eta2 (out3[1] of lssvr_estimate)
__device__ __forceinline__ bool indicator_marked(double v, double mx, double theta2) {
  return !(fabs(v) < INFINITY) || (mx > 0.0 && v >= theta2 * mx);
}

// One workgroup of kBlock threads, NL lanes of int64 (integer: exact): v[l] = this thread's run sum in, the exclusive
// prefix of the kBlock run sums out (Hillis-Steele over LDS); total[l] = the sum of all of them.  Every thread of the
// workgroup calls it, once per kernel.
template <int NL>
__device__ __forceinline__ void block_scan(int64_t (&v)[NL], int64_t (&total)[NL]) {
  __shared__ int64_t sh[NL][kBlock];
  const int tid = threadIdx.x;
#pragma unroll
  for (int l = 0; l < NL; ++l) sh[l][tid] = v[l];
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    int64_t add[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) add[l] = tid >= off ? sh[l][tid - off] : 0;
    __syncthreads();
#pragma unroll
    for (int l = 0; l < NL; ++l) sh[l][tid] += add[l];
    __syncthreads();
  }
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    v[l] = sh[l][tid] - v[l];
    total[l] = sh[l][kBlock - 1];
  }
}

// Workgroup tree (halving offsets: a fixed order, bitwise reproducible) of the BLOCK threads' NS values v[] ->
// out[NS*blockIdx.x ..]: slot 1 is a maximum, the other slots are sums.  red: NS*BLOCK doubles of LDS, slot-major.
template <int BLOCK, int NS>
__device__ __forceinline__ void reduce_partials(double* __restrict__ red, int tid, const double (&v)[NS],
                                                double* __restrict__ out) {
#pragma unroll
  for (int s = 0; s < NS; ++s) red[s * BLOCK + tid] = v[s];
  __syncthreads();
  for (int off = BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const double a = red[s * BLOCK + tid], b = red[s * BLOCK + tid + off];
        red[s * BLOCK + tid] = s == 1 ? fmax(a, b) : a + b;
      }
    }
    __syncthreads();
  }
  if (tid < NS) out[NS * blockIdx.x + tid] = red[tid * BLOCK];
}

// one workgroup: the nb per-block partials part[NS*i ..] in a fixed order -> out[0..NS) (bitwise reproducible)
template <int NS>
__global__ __launch_bounds__(kBlock) void finish_kernel(const double* __restrict__ part, int nb,
                                                         double* __restrict__ out) {
  __shared__ double sh[NS * kBlock];
  const int tid = threadIdx.x;
  double v[NS] = {};
  for (int i = tid; i < nb; i += kBlock) {
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = s == 1 ? fmax(v[s], part[NS * i + s]) : v[s] + part[NS * i + s];
  }
  reduce_partials<kBlock, NS>(sh, tid, v, out);
}

// ---------------------------------------------------------------------------
// The pieces the estimators are made of (one text each: adapt.hip's three kernels and adapt_goal.hip's differ in their
// tables and in what they integrate only).
// ---------------------------------------------------------------------------
// u_e'(x_e) and u_e'(x_{e+1}) from P_k'(+-1) = (+-1)^(k+1) k(k+1)/2
template <int MT>
__device__ __forceinline__ void end_derivs(const double (&c)[MT], double scl, double& dl, double& dr) {
  double sl = 0.0, sr = 0.0;
#pragma unroll
  for (int k = 1; k < MT; ++k) {
    const double w = (double)(k * (k + 1) / 2);
    sr = fma(c[k], w, sr);
    sl = fma(c[k], (k & 1) ? w : -w, sl);
  }
  dl = sl * scl;
  dr = sr * scl;
}

template <int MT>
__device__ __forceinline__ void load_row_global(const double* __restrict__ W, int64_t e, int M,
                                                double (&c)[MT]) {
#pragma unroll
  for (int k = 0; k < MT; ++k) c[k] = k < M ? W[e * M + k] : 0.0;
}

// Row t of the LDS coefficient table, TS entries per degree k: {P_k''} (TS = 1), {P_k', P_k''} (2) or
// {P_k', P_k'', P_k} (3) at t, by the forward recurrences
//   P_{k+1} = ((2k+1) t P_k - k P_{k-1}) / (k+1),  P'_{k+1} = P'_{k-1} + (2k+1) P_k,
//   P''_{k+1} = P''_{k-1} + (2k+1) P'_k;
// degrees >= M are zero.
template <int MT, int TS>
__device__ __forceinline__ void fill_table(double* __restrict__ Tq, double t, int M) {
  auto put = [&](int k, double d, double s, double v) {
    const bool in = k < M;
    if constexpr (TS == 1) {
      Tq[k] = in ? s : 0.0;
    } else {
      Tq[TS * k] = in ? d : 0.0;
      Tq[TS * k + 1] = in ? s : 0.0;
      if constexpr (TS == 3) Tq[TS * k + 2] = in ? v : 0.0;
    }
  };
  double p0 = 1.0, p1 = t, d0 = 0.0, d1 = 1.0, s0 = 0.0, s1 = 0.0;
  put(0, 0.0, 0.0, 1.0);
  if (MT > 1) put(1, 1.0, 0.0, t);
  for (int k = 1; k + 1 < MT; ++k) {
    const double a = (double)(2 * k + 1);
    const double p2 = (a * t * p1 - (double)k * p0) / (double)(k + 1);
    const double d2 = d0 + a * p1;
    const double s2 = s0 + a * d1;
    put(k + 1, d2, s2, p2);
    p0 = p1; p1 = p2;
    d0 = d1; d1 = d2;
    s0 = s1; s1 = s2;
  }
}

// End value of the neighbour `en` at the node it shares with the chunk (side 0: its left end, 1: its right end),
// recomputed from HBM: the same function on the same row as the lane that owns it, so bit-identical.  FLUX: scaled
// by a_ends to the flux a u'.
template <int MT, bool FLUX>
__device__ __forceinline__ double neighbour_end(const double* __restrict__ W, const double* __restrict__ x,
                                                const double* __restrict__ a_ends, int64_t en, int M, int side) {
  double cn[MT];
  load_row_global<MT>(W, en, M, cn);
  const DomainMap dn = map_params(x[en], x[en + 1]);
  double l, r;
  end_derivs<MT>(cn, dn.scl, l, r);
  const double d = side ? r : l;
  if constexpr (FLUX) return a_ends[2 * en + side] * d;
  else return d;
}

// Jumps at both ends of element e = c0 + tid from its own end values (vl, vr): the neighbours' come from the chunk's
// LDS arrays sl / sr, from neighbour_end at the two chunk edges; J_0 = J_ne = 0.
template <int MT, bool FLUX>
__device__ __forceinline__ void end_jumps(const double* __restrict__ W, const double* __restrict__ x,
                                          const double* __restrict__ a_ends, int64_t e, int64_t ne, int M, int tid,
                                          int nrow, const double* sl, const double* sr, double vl, double vr,
                                          double& jl, double& jr) {
  double r_prev = 0.0, l_next = 0.0;
  if (e > 0) r_prev = tid > 0 ? sr[tid - 1] : neighbour_end<MT, FLUX>(W, x, a_ends, e - 1, M, 1);
  if (e + 1 < ne) l_next = tid + 1 < nrow ? sl[tid + 1] : neighbour_end<MT, FLUX>(W, x, a_ends, e + 1, M, 0);
  jl = e > 0 ? r_prev - vl : 0.0;
  jr = e + 1 < ne ? vr - l_next : 0.0;
}

}  // namespace lssvr
