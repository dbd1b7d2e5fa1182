// The one routine behind every value of sensitivity.hip: the device kernel and the host mirror
// call it, and with -ffp-contract=off they are bit-equal.
#pragma once
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

#define LSSVR_SENS_HD __host__ __device__ __forceinline__

namespace lssvr {

// the grid cap of the grid-stride loop (256 threads per workgroup: kBlock)
constexpr int kSensMaxBlocks = 1024;

inline int64_t sens_blocks(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return b < 1 ? 1 : (b < kSensMaxBlocks ? b : kSensMaxBlocks);
}

// t[k] for a k that differs from lane to lane: a chain of selects, so the rule stays in the kernel arguments and no
// lane indexes memory with it
LSSVR_SENS_HD double sens_pick(const double (&t)[5], int k) {
  double v = t[0];
#pragma unroll
  for (int i = 1; i < 5; ++i) v = k == i ? t[i] : v;
  return v;
}

// Entry idx = e * nquad + k of a table [ne][nquad], the start of every sensitivity pass: the element e and, with xi, w
// the point and weight k of the rule on [0, 1] and h = x[e+1] - x[e], om = 1 - xi, wh = w / h, hw = h w, each formed
// once
struct SensPoint {
  int64_t e;
  double xi, w, om, wh, hw;
};
LSSVR_SENS_HD SensPoint sens_point(const double* x, int64_t ne, int nquad, const QuadRule& q, int64_t idx) {
  // (a table below 2^32 entries: the 32-bit quotient is the same number and a fraction of the instructions)
  const int64_t e = ne * (int64_t)nquad <= (int64_t)0xffffffffu ? (int64_t)((uint32_t)idx / (uint32_t)nquad)
                                                               : idx / nquad;
  const int k = (int)(idx - e * nquad);
  const double xi = sens_pick(q.xi, k), w = sens_pick(q.wt, k);
  const double h = x[e + 1] - x[e];
  return SensPoint{e, xi, w, 1.0 - xi, w / h, h * w};
}

// U and Z of case j
LSSVR_SENS_HD const double* sens_u(const SensArgs& a, int j) {
  return a.U + (a.nu == 1 ? 0 : (int64_t)j * (a.ne + 1));
}
LSSVR_SENS_HD const double* sens_z(const SensArgs& a, int j) { return a.Z + (int64_t)j * (a.ne + 1); }

// Entry idx = e * nquad + k of the four tables, for every case.  With xi, w, h, om of sens_point,
// (u0, u1) = U[j][e], U[j][e+1] and (z0, z1) likewise, the order of every operation:
//   du = u1 - u0;   dz = z1 - z0
//   uq = u0 om + u1 xi;             zq = z0 om + z1 xi
//   ga = -(((w / h) dz) du)
//   gb = -((w zq) du)
//   gc = -(((h w) zq) uq)
//   gf = (h w) zq
// The mesh and the rule are read once for all cases; a table that is not asked for costs neither arithmetic that only
// it needs nor a store.
LSSVR_SENS_HD void sens_entry(const SensArgs& a, const QuadRule& q, int64_t idx) {
  const int64_t tab = a.ne * (int64_t)a.nquad;
  const SensPoint p = sens_point(a.x, a.ne, a.nquad, q, idx);
  for (int j = 0; j < a.nc; ++j) {
    const double* u = sens_u(a, j) + p.e;
    const double* z = sens_z(a, j) + p.e;
    const double u0 = u[0], u1 = u[1], z0 = z[0], z1 = z[1];
    const double du = u1 - u0;
    const double zq = z0 * p.om + z1 * p.xi;
    const int64_t o = (int64_t)j * tab + idx;
    if (a.ga) a.ga[o] = -((p.wh * (z1 - z0)) * du);
    if (a.gb) a.gb[o] = -((p.w * zq) * du);
    if (a.gc) a.gc[o] = -((p.hw * zq) * (u0 * p.om + u1 * p.xi));
    if (a.gf) a.gf[o] = p.hw * zq;
  }
}

// out_ends[j] = (dJ/dg_0, dJ/dg_ne, dJ/dkappa_0, dJ/dkappa_ne) of case j.  With p = P[j] (0 without P), s0 = sub[0] and
// sn = sup[ne-1] of the raw bands:
//   Dirichlet end:  dJ/dg_0 = p_0 - s0 z_1,   dJ/dg_ne = p_ne - sn z_{ne-1},   dJ/dkappa = 0
//   Robin end:      dJ/dg = z_end,            dJ/dkappa = -(z_end u_end)
LSSVR_SENS_HD void sens_ends(const SensArgs& a, int j) {
  const double* u = sens_u(a, j);
  const double* z = sens_z(a, j);
  const double* p = a.P ? a.P + (int64_t)j * (a.ne + 1) : nullptr;
  double* out = a.out_ends + 4 * j;
  for (int s = 0; s < 2; ++s) {
    const int64_t end = s ? a.ne : 0, inner = s ? a.ne - 1 : 1;
    if (a.kind[s] == LSSVR_END_ROBIN) {
      out[s] = z[end];
      out[2 + s] = -(z[end] * u[end]);
    } else {
      out[s] = (p ? p[end] : 0.0) - a.band_ends[s] * z[inner];
      out[2 + s] = 0.0;
    }
  }
}

}  // namespace lssvr
