// hp-adaptive refinement (no reference counterpart): what chooses the degrees of a mesh that
// lssvr_enhance_subset enhances with one degree per element.
//   - decay rate of each element's Legendre coefficients (lssvr_smoothness)
//   - threshold marking, then raise the degree where the decay is fast, bisect where it is not (lssvr_refine_hp)
//   - stable counting sort of the element indices by degree (lssvr_group_by_degree)
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
// hp marking: count per block, one-block scan, scatter (the launches of lssvr_refine)
// ---------------------------------------------------------------------------
struct RefineHpArgs {
  const double* x;
  int64_t ne;
  const double* eta2;
  const double* mx;
  double theta2, h2min;
  const double* sigma;
  const int32_t* deg;
  double sigma_min;
  int dM, M_max;
};

// 0: unchanged, 1: bisected, 2: degree raised
__device__ __forceinline__ int hp_action(const RefineHpArgs& p, int64_t e, double m_max) {
  if (!indicator_marked(p.eta2[e], m_max, p.theta2)) return 0;
  if (p.sigma[e] >= p.sigma_min && (int64_t)p.deg[e] + p.dM <= p.M_max) return 2;      // NaN compares false
  return p.x[e + 1] - p.x[e] >= p.h2min ? 1 : 0;
}

// cnt[block] = bisected | raised << 32 (each at most kBlock)
__global__ __launch_bounds__(kBlock) void refine_hp_count_kernel(RefineHpArgs p, int64_t* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double m_max = p.mx[0];
  const int act = e < p.ne ? hp_action(p, e, m_max) : 0;
  const int ns = __syncthreads_count(act == 1);
  const int nr = __syncthreads_count(act == 2);
  if (threadIdx.x == 0) cnt[blockIdx.x] = (int64_t)ns | ((int64_t)nr << 32);
}

// refine_scan_kernel of adapt.hip on the packed counts: exclusive offsets of the bisected counts in place, the two
// totals to counts2 = {bisected, raised}
__global__ __launch_bounds__(kBlock) void refine_hp_scan_kernel(int64_t* __restrict__ cnt, int64_t nb, int64_t ne,
                                                                int64_t* __restrict__ ne_new,
                                                                int64_t* __restrict__ counts2) {
  __shared__ int64_t sh[kBlock];
  __shared__ int64_t shr[kBlock];
  const int tid = threadIdx.x;
  const int64_t per = (nb + kBlock - 1) / kBlock;
  const int64_t lo = tid * per < nb ? tid * per : nb;
  const int64_t hi = lo + per < nb ? lo + per : nb;
  int64_t s = 0, r = 0;
  for (int64_t i = lo; i < hi; ++i) {
    s += cnt[i] & 0xffffffffLL;
    r += cnt[i] >> 32;
  }
  sh[tid] = s;
  shr[tid] = r;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const int64_t add = tid >= off ? sh[tid - off] : 0;
    const int64_t addr = tid >= off ? shr[tid - off] : 0;
    __syncthreads();
    sh[tid] += add;
    shr[tid] += addr;
    __syncthreads();
  }
  int64_t run = sh[tid] - s;
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t v = cnt[i] & 0xffffffffLL;
    cnt[i] = run;
    run += v;
  }
  if (tid == kBlock - 1) {
    *ne_new = ne + sh[kBlock - 1];
    counts2[0] = sh[kBlock - 1];
    counts2[1] = shr[kBlock - 1];
  }
}

__global__ __launch_bounds__(kBlock) void refine_hp_scatter_kernel(RefineHpArgs p, const int64_t* __restrict__ offs,
                                                                   double* __restrict__ x_new,
                                                                   int32_t* __restrict__ deg_new,
                                                                   int64_t* __restrict__ parent) {
  __shared__ int wsum[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t e = (int64_t)blockIdx.x * kBlock + tid;
  const double m_max = p.mx[0];
  const int act = e < p.ne ? hp_action(p, e, m_max) : 0;
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
    const int32_t d = p.deg[e];
    x_new[pos] = a;
    deg_new[pos] = act == 2 ? d + p.dM : d;
    if (parent) parent[pos] = e;
    if (m) {
      x_new[pos + 1] = 0.5 * (a + b);
      deg_new[pos + 1] = d;
      if (parent) parent[pos + 1] = e;
    }
    if (e + 1 == p.ne) x_new[pos + 1 + (m ? 1 : 0)] = b;
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
  __shared__ int64_t sh[kBlock];
  const int tid = threadIdx.x;
  const int n = kGroupBins * nb;
  const int per = (n + kBlock - 1) / kBlock;
  const int lo = tid * per < n ? tid * per : n;
  const int hi = lo + per < n ? lo + per : n;
  int64_t s = 0;
  for (int i = lo; i < hi; ++i) s += hist[i];
  sh[tid] = s;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const int64_t add = tid >= off ? sh[tid - off] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  int64_t run = sh[tid] - s;
  for (int i = lo; i < hi; ++i) {
    const int64_t v = hist[i];
    hist[i] = run;
    if (i % nb == 0) offsets[2 + i / nb] = run;
    run += v;
  }
  if (tid == kBlock - 1) offsets[2 + kGroupBins] = sh[kBlock - 1];
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

hipError_t refine_hp(const double* x, int64_t ne, const double* eta2, const double* eta2_max, double theta,
                     double h_min, const double* sigma, const int32_t* deg, double sigma_min, int dM, int M_max,
                     void* work, double* x_new, int32_t* deg_new, int64_t* parent, int64_t* ne_new, int64_t* counts2,
                     hipStream_t s) {
  const int64_t nb = ref_blocks(ne);
  int64_t* cnt = static_cast<int64_t*>(work);
  const RefineHpArgs p{x, ne, eta2, eta2_max, theta * theta, 2.0 * h_min, sigma, deg, sigma_min, dM, M_max};
  hipLaunchKernelGGL(refine_hp_count_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, p, cnt);
  hipLaunchKernelGGL(refine_hp_scan_kernel, dim3(1), dim3(kBlock), 0, s, cnt, nb, ne, ne_new, counts2);
  hipLaunchKernelGGL(refine_hp_scatter_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, p, cnt, x_new, deg_new,
                     parent);
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
