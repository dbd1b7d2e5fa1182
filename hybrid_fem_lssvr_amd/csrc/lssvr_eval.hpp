// Point location and evaluation of the enhanced solution (Dual.py:176-203), shared by
// lssvr_eval / lssvr_eval_error (fem_eval.hip) and the derivative / estimator kernels (adapt.hip).
#pragma once
#include "lssvr_device.hpp"

namespace lssvr {

// Element of a query point: the first j with x[j] <= xq <= x[j+1]
//   == clamp(#{nodes < xq} - 1, 0, ne-1)      (a point on an interior node takes
// the left element; outside the mesh the first / last element extrapolates).
__device__ __forceinline__ int64_t locate(const double* __restrict__ x, int64_t ne, double xq,
                                          double x0, double inv_h) {
  // uniform-mesh guess, verified against the actual nodes
  double g = (xq - x0) * inv_h;
  int64_t j = g > 0.0 ? (g < (double)(ne - 1) ? (int64_t)g : ne - 1) : 0;
#pragma unroll 1
  for (int it = 0; it < 3; ++it) {
    const bool lo_ok = (j == 0) || (x[j] < xq);
    const bool hi_ok = (j == ne - 1) || (xq <= x[j + 1]);
    if (lo_ok && hi_ok) return j;
    j += lo_ok ? 1 : -1;
  }
  // general mesh: lower_bound over the ne+1 nodes
  int64_t lo = 0, hi = ne + 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (x[mid] < xq) lo = mid + 1; else hi = mid;
  }
  j = lo - 1;
  return j < 0 ? 0 : (j > ne - 1 ? ne - 1 : j);
}

// value of the hybrid solution at one point (Dual.py:182-201); j_out = element used (-1: NaN)
__device__ __forceinline__ double eval_point(const double* __restrict__ x,
                                             const double* __restrict__ W, int64_t ne, int M,
                                             double xi, double x0, double inv_h, int64_t& j_out) {
  if (xi != xi) {  // NaN: no branch of Dual.py:182-201 fires, the zero stays
    j_out = -1;
    return 0.0;
  }
  {
    const int64_t j = locate(x, ne, xi, x0, inv_h);
    j_out = j;
    const DomainMap dm = map_params(x[j], x[j + 1]);
    const double t = dm.off + dm.scl * xi;      // mapdomain, two roundings
    const double* c = W + j * M;
    double c0, c1;
    if (M == 1) {
      c0 = c[0];
      c1 = 0.0;
    } else if (M == 2) {
      c0 = c[0];
      c1 = c[1];
    } else {
      // numpy legval: c0 = c[-i] - (c1*(nd-1))/nd ; c1 = tmp + (c1*x*(2*nd-1))/nd
      int nd = M;
      c0 = c[M - 2];
      c1 = c[M - 1];
      for (int k = 3; k <= M; ++k) {
        const double tmp = c0;
        nd = nd - 1;
        c0 = c[M - k] - (c1 * (double)(nd - 1)) / (double)nd;
        c1 = tmp + ((c1 * t) * (double)(2 * nd - 1)) / (double)nd;
      }
    }
    return c0 + c1 * t;
  }
}

}  // namespace lssvr
