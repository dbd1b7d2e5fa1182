// hp-adaptive refinement (no reference counterpart): what surrounds the choice of the degrees of
// a mesh that lssvr_enhance_subset enhances with one degree per element.
//   - decay rate of each element's Legendre coefficients (lssvr_smoothness)
//   - stable counting sort of the element indices by degree (lssvr_group_by_degree)
// The marking itself (lssvr_refine_hp: raise the degree where the decay is fast, bisect where it is not) is the HP
// instance of adapt.hip's marking kernels.
// The structure of adapt.hip: a lane per element, W staged through LDS at an odd stride, no atomics, every output
// bitwise reproducible from run to run.
#include <cmath>

#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_adapt.hpp"

namespace lssvr {

namespace {

// ---------------------------------------------------------------------------
// smoothness
// ---------------------------------------------------------------------------
// sigma of one staged row c[0..M): the envelope env_p = max_{p <= q < M} |c_q| does not increase with p, so the
// points kept (env_p >= 2^-52 max |c|, env_p > 0) are p = 1..K.  y_p = ln env_p overwrites c[p] in LDS: one log
// per coefficient, the centred sums read it back.
__device__ __forceinline__ double decay_rate(double* __restrict__ c, int M) {
  double mx = 0.0;
  bool finite = true;
  for (int p = 0; p < M; ++p) {
    const double a = fabs(c[p]);
    finite = finite && a < INFINITY;
    mx = fmax(mx, a);
  }
  if (!finite) return NAN;
  if (mx == 0.0 || M < 3) return INFINITY;
  const double thr = 0x1p-52 * mx;
  double env = 0.0, sy = 0.0;
  int K = 0;
  for (int p = M - 1; p >= 1; --p) {
    env = fmax(env, fabs(c[p]));
    if (env > 0.0 && env >= thr) {
      const double y = log(env);
      c[p] = y;
      sy += y;
      ++K;
    }
  }
  if (K < 2) return INFINITY;
  const double pbar = 0.5 * (double)(K + 1), ybar = sy / (double)K;
  double sxy = 0.0, sxx = 0.0;
  for (int p = 1; p <= K; ++p) {
    const double dp = (double)p - pbar;
    sxy = fma(dp, c[p] - ybar, sxy);
    sxx = fma(dp, dp, sxx);
  }
  return -(sxy / sxx);
}

// Dynamic LDS: rows[kEstBlock * ms], ms = ldw | 1 (odd: conflict-free ds_read_b64 / ds_write_b64 down a column)
__global__ __launch_bounds__(kEstBlock) void smoothness_kernel(const double* __restrict__ W, int ldw, int ms,
                                                               const int32_t* __restrict__ deg, int64_t ne,
                                                               double* __restrict__ sigma) {
  extern __shared__ double rows[];
  const int tid = threadIdx.x;
  for (int64_t c0 = (int64_t)blockIdx.x * kEstBlock; c0 < ne; c0 += (int64_t)gridDim.x * kEstBlock) {
    const int nrow = (int)(ne - c0 < kEstBlock ? ne - c0 : kEstBlock);
    stage_rows(rows, W + c0 * ldw, nrow * ldw, ldw, ms, tid);
    __syncthreads();
    if (tid < nrow) {
      const int M = deg[c0 + tid];
      // a degree the row cannot hold reads nothing
      sigma[c0 + tid] = (M >= 2 && M <= ldw) ? decay_rate(rows + tid * ms, M) : NAN;
    }
    __syncthreads();      // rows are rewritten by the next chunk
  }
}

// ---------------------------------------------------------------------------
// grouping by degree: per-workgroup histograms, one scanning workgroup, scatter
// ---------------------------------------------------------------------------
constexpr int kGroupBins = 32;          // degrees 2 .. 33
constexpr int kGroupMaxBlocks = 1024;   // grid cap: kGroupBins counters per workgroup in `work`

struct GroupGeom {
  int64_t tiles, per;     // tiles of kBlock elements; tiles per workgroup (a contiguous run: the sort is stable)
  int nb;
};
GroupGeom group_geom(int64_t ne) {
  GroupGeom g;
  g.tiles = ne < 1 ? 1 : (ne + kBlock - 1) / kBlock;
  g.nb = (int)(g.tiles < kGroupMaxBlocks ? g.tiles : kGroupMaxBlocks);
  g.per = (g.tiles + g.nb - 1) / g.nb;
  return g;
}

__device__ __forceinline__ int degree_bin(const int32_t* __restrict__ deg, int64_t e, int64_t ne) {
  if (e >= ne) return -1;
  const int d = deg[e];
  return d >= 2 && d < 2 + kGroupBins ? d - 2 : -1;      // outside 2 .. 33: in no bin
}

// hist[bin * nb + block]: bin-major, so that ONE exclusive scan of the array in that order is the start of every
// (bin, block) run in ids.  Lane b of every wave counts bin b from the wave's ballots.
__global__ __launch_bounds__(kBlock) void group_hist_kernel(const int32_t* __restrict__ deg, int64_t ne,
                                                            int64_t per, int64_t* __restrict__ hist) {
  __shared__ int64_t wacc[kBlock / 64][kGroupBins];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * per;
  int64_t acc = 0;
  for (int64_t t = t0; t < t0 + per; ++t) {
    const int bin = degree_bin(deg, t * kBlock + tid, ne);
#pragma unroll 4
    for (int b = 0; b < kGroupBins; ++b) {
      const unsigned long long bal = __ballot(bin == b);
      if (lane == b) acc += __popcll(bal);
    }
  }
  if (lane < kGroupBins) wacc[wv][lane] = acc;
  __syncthreads();
  if (tid < kGroupBins) {
    int64_t s = 0;
    for (int w = 0; w < kBlock / 64; ++w) s += wacc[w][tid];
    hist[(int64_t)tid * gridDim.x + blockIdx.x] = s;
  }
}

// exclusive offsets of the n = kGroupBins * nb counts, in place (refine_scan_kernel's scheme); the offset of every
// bin's first entry is the start of its degree in ids
__global__ __launch_bounds__(kBlock) void group_scan_kernel(int64_t* __restrict__ hist, int nb,
                                                            int64_t* __restrict__ offsets) {
  const int tid = threadIdx.x;
  const int n = kGroupBins * nb;
  const int per = (n + kBlock - 1) / kBlock;
  const int lo = tid * per < n ? tid * per : n;
  const int hi = lo + per < n ? lo + per : n;
  int64_t sum[1] = {}, total[1];
  for (int i = lo; i < hi; ++i) sum[0] += hist[i];
  block_scan<1>(sum, total);
  int64_t run = sum[0];
  for (int i = lo; i < hi; ++i) {
    const int64_t v = hist[i];
    hist[i] = run;
    if (i % nb == 0) offsets[2 + i / nb] = run;
    run += v;
  }
  if (tid == kBlock - 1) offsets[2 + kGroupBins] = total[0];
  if (tid < 2) offsets[tid] = 0;
}

// position of element e = base of its (bin, block) run + elements of the bin in the earlier tiles of the block
// + those in the lower waves of the tile + those in the lower lanes of the wave (ballot rank)
__global__ __launch_bounds__(kBlock) void group_scatter_kernel(const int32_t* __restrict__ deg, int64_t ne,
                                                               int64_t per, const int64_t* __restrict__ hist,
                                                               int64_t* __restrict__ ids) {
  __shared__ int64_t base[kGroupBins];
  __shared__ int wcnt[kBlock / 64][kGroupBins];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * per;
  if (tid < kGroupBins) base[tid] = hist[(int64_t)tid * gridDim.x + blockIdx.x];
  for (int64_t t = t0; t < t0 + per; ++t) {
    const int64_t e = t * kBlock + tid;
    const int bin = degree_bin(deg, e, ne);
    int rank = 0, mine = 0;
#pragma unroll 4
    for (int b = 0; b < kGroupBins; ++b) {
      const unsigned long long bal = __ballot(bin == b);
      if (bin == b)
        rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
      if (lane == b) mine = __popcll(bal);
    }
    if (lane < kGroupBins) wcnt[wv][lane] = mine;
    __syncthreads();      // base (first tile) and wcnt are written
    if (bin >= 0) {
      int64_t pos = base[bin] + rank;
      for (int w = 0; w < wv; ++w) pos += wcnt[w][bin];
      ids[pos] = e;
    }
    __syncthreads();      // every lane has read base and wcnt
    if (tid < kGroupBins) {
      int s = 0;
      for (int w = 0; w < kBlock / 64; ++w) s += wcnt[w][tid];
      base[tid] += s;
    }
    __syncthreads();      // wcnt is rewritten by the next tile
  }
}

}  // namespace

hipError_t smoothness(const double* W, int ldw, const int32_t* deg, int64_t ne, double* sigma, hipStream_t s) {
  const int ms = ldw | 1;
  const size_t lds = sizeof(double) * (size_t)kEstBlock * ms;
  hipLaunchKernelGGL(smoothness_kernel, dim3((unsigned)est_blocks(ne)), dim3(kEstBlock), lds, s, W, ldw, ms, deg, ne,
                     sigma);
  return hipGetLastError();
}

int64_t group_work_bytes(int64_t ne) { return 8 * (int64_t)kGroupBins * group_geom(ne).nb; }

hipError_t group_by_degree(const int32_t* deg, int64_t ne, int64_t* ids, int64_t* offsets, void* work,
                           hipStream_t s) {
  const GroupGeom g = group_geom(ne);
  int64_t* hist = static_cast<int64_t*>(work);
  hipLaunchKernelGGL(group_hist_kernel, dim3((unsigned)g.nb), dim3(kBlock), 0, s, deg, ne, g.per, hist);
  hipLaunchKernelGGL(group_scan_kernel, dim3(1), dim3(kBlock), 0, s, hist, g.nb, offsets);
  hipLaunchKernelGGL(group_scatter_kernel, dim3((unsigned)g.nb), dim3(kBlock), 0, s, deg, ne, g.per, hist, ids);
  return hipGetLastError();
}

}  // namespace lssvr
