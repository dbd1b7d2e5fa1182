// What the estimator / h-refinement kernels (adapt.hip) and the hp kernels (adapt_hp.hip) share: the chunk
// geometry, the coalesced staging of W rows through LDS and the marking predicate.
#pragma once
#include <cmath>
#include <cstdint>

#include "lssvr_device.hpp"

namespace lssvr {

constexpr int kEstBlock = 128;          // elements per workgroup chunk (two waves)
constexpr int kEstMaxBlocks = 4096;     // grid cap: partials of the reduction in `work`

inline int64_t est_blocks(int64_t ne) {
  const int64_t b = (ne + kEstBlock - 1) / kEstBlock;
  return b < 1 ? 1 : (b < kEstMaxBlocks ? b : kEstMaxBlocks);
}
inline int64_t ref_blocks(int64_t ne) {
  const int64_t b = (ne + kBlock - 1) / kBlock;
  return b < 1 ? 1 : b;
}

// the chunk's contiguous `total` = nrow*M doubles of W from `src` (coalesced) into LDS rows of odd stride ms;
// column stepping: i += kEstBlock  ->  (row, col) += (kEstBlock / M, kEstBlock % M)
__device__ __forceinline__ void stage_rows(double* __restrict__ rows, const double* __restrict__ src, int total,
                                           int M, int ms, int tid) {
  const int qM = kEstBlock / M, rM = kEstBlock - (kEstBlock / M) * M;
  int r = tid / M, col = tid - (tid / M) * M;
  for (int i = tid; i < total; i += kEstBlock) {
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

}  // namespace lssvr
