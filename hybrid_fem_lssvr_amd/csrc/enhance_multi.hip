// Several load cases on one mesh (lssvr_enhance_multi): ONE Gram contraction and ONE LDL^T per element, a
// right-hand side vector, two triangular solves and a coefficient row per case.  Lane per element, registers only,
// M = 2 .. kReactSmallMaxM = 16; above, capi.hip runs the wave kernels once per case.
//
// The per-element system S = G + eps (I + C^T C) depends on the mesh, the a / a' / c tables, gamma, M and n_colloc;
// the right-hand side f, the nodal values u and the Dirichlet values enter only r and the lifting d = (d0, d1).  So
// one lane forms rho_k and G exactly as enhance_small_body<M, RHS, true, RX> does (enhance_small_impl.hpp: same
// helpers, same order of operations) and, in the same loop over the collocation points, accumulates
// r^(j) += rho_k phi_k^(j) for the NC cases of the pass, phi_k^(j) from f_k^(j) and that case's (d0, d1).  After the
// ridge and the factorisation each case takes its two triangular solves and its row goes through the LDS transpose.
//
// NC = kMultiRC<M> cases per pass (registers: DESIGN.md section 16) -- more cases are more passes, each of which
// reads the coefficient tables again; a pass of one case runs the NC = 1 instantiation, a pass of 1 < nc < NC cases
// the NC one with the last case repeated in the idle slots (loads in bounds, stores masked).
#include "enhance_small_impl.hpp"

namespace lssvr {

// Cases per pass.  Chosen from the kernel resource remarks of this file so that no instantiation has scratch:
// two resident waves per SIMD (<= 256 registers) up to M = 8; from M = 9 a second case already costs the second wave
// (the one-case kernel holds 236 VGPRs), so those degrees take the one-wave VGPR + AGPR budget and fill it.
constexpr int multi_rc(int M) {
  return M == 2 ? 8 : M <= 6 ? 4 : M == 7 ? 3 : M == 8 ? 2 : M <= 13 ? 4 : M == 14 ? 2 : 1;
}
// point-major tables: points requested ahead.  One case: the single-case kernels' depths.  More: two, and four where
// the kernel runs at one wave per SIMD anyway and has the registers (M = 9 .. 11) -- with no second wave to switch
// to, two points (~400 FP64 instructions) do not span the latency of HBM.
constexpr int multi_pf(int M, bool rx, int nc) {
  return nc == 1 ? (rx ? kPrefetchReact : kPrefetch) : (M >= 9 && M <= 11) ? 4 : 2;
}
template <int M>
constexpr int kMultiRC = multi_rc(M);
constexpr int kMultiMaxRC = 8;

// element-major tables: (2 or 3 coefficient arrays + NC right-hand sides) staged per wave, kStageK points deep while
// four arrays suffice (the reaction kernel's footprint), four points deep beyond (80 KB per workgroup at most: two
// workgroups per CU)
template <bool RX, int NC>
constexpr int kMultiArrays = (RX ? 3 : 2) + NC;
template <bool RX, int NC>
constexpr int kMultiStageK = kMultiArrays<RX, NC> <= 4 ? kStageK : 4;
template <int M, int RHS, bool RX, int NC>
constexpr int kMultiTilePerWave =
    (RHS == LSSVR_RHS_ARRAY && kMultiArrays<RX, NC> * 64 * (kMultiStageK<RX, NC> + 1) > 64 * M)
        ? kMultiArrays<RX, NC> * 64 * (kMultiStageK<RX, NC> + 1)
        : 64 * M;

template <int M, int RHS, bool RX, int NC>
__device__ __forceinline__ void enhance_multi_body(const EnhanceMultiArgs& p, const unsigned block,
                                                   double* __restrict__ tile) {
  static_assert(RHS == LSSVR_RHS_ARRAY || RHS == LSSVR_RHS_ARRAY_PM, "tabulated right-hand sides only");
  static_assert(NC >= 1 && NC <= kMultiMaxRC, "cases per pass");
  constexpr int MR = M - 2;
  constexpr int MR1 = MR > 0 ? MR : 1;
  constexpr int NT = MR1 * (MR1 + 1) / 2;
  constexpr int KS = kMultiStageK<RX, NC>;
  constexpr int SA = 64 * (KS + 1);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int64_t e = (int64_t)block * kBlock + tid;
  // Every lane runs the body (lanes past the end on a duplicate of the last element, their stores masked)
  const bool live = e < p.ne;
  const int64_t ec = live ? e : p.ne - 1;
  const int nc = NC == 1 ? 1 : p.nc;                          // cases of this pass, 1 .. NC
  // the case a slot works on: its own, or the last one's again in an idle slot
  auto slot_case = [&](const int j) { return j < nc ? j : nc - 1; };
  const int n = p.n;
  const int64_t fstride = p.ne * (int64_t)n;
  double* const wt = tile + (tid >> 6) * kMultiTilePerWave<M, RHS, RX, NC>;

  const double a = p.x[ec];
  const double b = p.x[ec + 1];
  const int64_t eg = ec + p.elem_offset;
  // Dual.py:65-75 with the case's own Dirichlet pair
  const bool lb = (eg == 0 && a == p.gxmin);
  const bool rb = (eg == p.ne_global - 1 && b == p.gxmax);
  double gl[NC], gr[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int jc = slot_case(j);
    const double* const uj = p.u + (int64_t)jc * (p.ne + 1);
    const double bl = p.bc_values ? p.bc_values[2 * jc] : 0.0;
    const double br = p.bc_values ? p.bc_values[2 * jc + 1] : 0.0;
    gl[j] = lb ? bl : uj[ec];
    gr[j] = rb ? br : uj[ec + 1];
  }

  const DomainMap dm = map_params(a, b);
  const double step = dm.oldlen / (double)(n - 1);
  const double scl2 = dm.scl * dm.scl;
  const double inv_scl2 = rcp_newton(scl2);
  const double eps = rcp_newton(p.gamma * (scl2 * scl2));   // 1 / (gamma * scl^4)

  // boundary rows, eliminated as w_{0,1} = d - C v (enhance_small_body); d per case
  double d0[NC], d1[NC];
  double C0[MR1], C1[MR1];
  {
    const double ta = dm.off + dm.scl * a;
    const double tb = dm.off + dm.scl * b;
    double La[M], Lb[M];
    legendre_p<M>(ta, La);
    legendre_p<M>(tb, Lb);
    const double idet = rcp_newton(tb - ta);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      d0[j] = (tb * gl[j] - ta * gr[j]) * idet;
      d1[j] = (gr[j] - gl[j]) * idet;
    }
#pragma unroll
    for (int j = 0; j < MR; ++j) {
      C0[j] = (tb * La[j + 2] - ta * Lb[j + 2]) * idet;
      C1[j] = (Lb[j + 2] - La[j + 2]) * idet;
    }
  }

  double G[NT], rv[NC][MR1];
  bool ok = true;
  if constexpr (MR > 0) {
#pragma unroll
    for (int i = 0; i < NT; ++i) G[i] = 0.0;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int i = 0; i < MR; ++i) rv[j][i] = 0.0;

    // one collocation point: rho_k and the update of G ONCE, phi_k and r per case
    auto point = [&](const int k, const double (&fk)[NC], const double ak, const double dak,
                     [[maybe_unused]] const double ck) {
      const double xk = linspace_at(a, b, dm.oldlen, step, k, n);
      const double tk = dm.off + dm.scl * xk;
      double rho[MR];
      legendre_d2<MR>(tk, rho);
      const double bk = dak * (0.5 * dm.oldlen);          // a'/scl as a' (h/2), as enhance_small_body
      double r1[MR + 1];
      legendre_d1<MR + 1>(tk, r1);
#pragma unroll
      for (int j = 0; j < MR; ++j) rho[j] = fma(ak, rho[j], bk * (r1[j + 1] - C1[j]));
      double phi[NC];
#pragma unroll
      for (int j = 0; j < NC; ++j) phi[j] = -fma(bk, d1[j], fk[j] * inv_scl2);
      if constexpr (RX) {
        const double cs = ck * inv_scl2;                    // c / scl^2
        double Lk[M];
        legendre_p<M>(tk, Lk);
#pragma unroll
        for (int j = 0; j < MR; ++j) rho[j] = fma(-cs, Lk[j + 2] - fma(tk, C1[j], C0[j]), rho[j]);
#pragma unroll
        for (int j = 0; j < NC; ++j) phi[j] = fma(cs, fma(tk, d1[j], d0[j]), phi[j]);
      }
#pragma unroll
      for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) G[tri(i, j)] = fma(rho[i], rho[j], G[tri(i, j)]);
#pragma unroll
        for (int j = 0; j < NC; ++j) rv[j][i] = fma(rho[i], phi[j], rv[j][i]);
      }
    };

    if constexpr (RHS == LSSVR_RHS_ARRAY_PM) {
      // point-major tables t[k * ne + e], each case's slab alike: direct loads, the next PF points requested before
      // the current PF are worked on (enhance_small_body); past the last point the index is clamped
      constexpr int PF = multi_pf(M, RX, NC);
      const int64_t ps = p.ne;
      const double* const tf = p.rhs_values + ec;
      const double* const ta = p.a_values + ec;
      const double* const td = p.da_values + ec;
      [[maybe_unused]] const double* tc = nullptr;
      if constexpr (RX) tc = p.c_values + ec;
      int64_t fo[NC];                                       // slab of each slot's case
#pragma unroll
      for (int j = 0; j < NC; ++j) fo[j] = (int64_t)slot_case(j) * fstride;
      double cf[PF][NC], ca[PF], cdv[PF];
      [[maybe_unused]] double cc[PF];
      auto fetch = [&](const int k, double (&f_)[NC], double& a_, double& d_, [[maybe_unused]] double& c_) {
        const int64_t g = (int64_t)min(k, n - 1) * ps;
#pragma unroll
        for (int j = 0; j < NC; ++j) f_[j] = __builtin_nontemporal_load(tf + fo[j] + g);
        a_ = __builtin_nontemporal_load(ta + g);
        d_ = __builtin_nontemporal_load(td + g);
        if constexpr (RX) c_ = __builtin_nontemporal_load(tc + g);
      };
#pragma unroll
      for (int i = 0; i < PF; ++i) fetch(i, cf[i], ca[i], cdv[i], cc[i]);
      for (int k = 0; k < n; k += PF) {
        double nf[PF][NC], na[PF], nd[PF];
        [[maybe_unused]] double ncv[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) fetch(k + PF + i, nf[i], na[i], nd[i], ncv[i]);
#pragma unroll
        for (int i = 0; i < PF; ++i)
          if (k + i < n) point(k + i, cf[i], ca[i], cdv[i], RX ? cc[i] : 0.0);
#pragma unroll
        for (int i = 0; i < PF; ++i) {
#pragma unroll
          for (int j = 0; j < NC; ++j) cf[i][j] = nf[i][j];
          ca[i] = na[i];
          cdv[i] = nd[i];
          if constexpr (RX) cc[i] = ncv[i];
        }
      }
    } else {
      // element-major tables t[e * n + k]: the wave stages KS points of its 64 rows per array through LDS, row pitch
      // KS + 1 (enhance_small_body); arrays 0 .. NC-1 are the cases' f, then a, a' (, c)
      const int64_t e0 = (int64_t)block * kBlock + (tid & ~63);
      for (int k = 0; k < n; ++k) {
        if ((k & (KS - 1)) == 0) {
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int i = 0; i < KS; ++i) {
            const int idx = i * 64 + lane;
            const int row = idx / KS, kk = idx % KS;
            const int64_t er = e0 + row;
            const bool in = (er < p.ne) && (k + kk < n);
            const int64_t g = in ? er * n + (k + kk) : 0;
            const int s = row * (KS + 1) + kk;
#pragma unroll
            for (int j = 0; j < NC; ++j)
              wt[j * SA + s] = in ? p.rhs_values[(int64_t)slot_case(j) * fstride + g] : 0.0;
            wt[NC * SA + s] = in ? p.a_values[g] : 0.0;
            wt[(NC + 1) * SA + s] = in ? p.da_values[g] : 0.0;
            if constexpr (RX) wt[(NC + 2) * SA + s] = in ? p.c_values[g] : 0.0;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
        const int s = lane * (KS + 1) + (k & (KS - 1));
        double fk[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) fk[j] = wt[j * SA + s];
        double ck = 0.0;
        if constexpr (RX) ck = wt[(NC + 2) * SA + s];
        point(k, fk, wt[NC * SA + s], wt[(NC + 1) * SA + s], ck);
      }
    }

    // S = G + eps (I + C^T C),  rhs = r + eps C^T d
#pragma unroll
    for (int i = 0; i < MR; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double cc = fma(C0[i], C0[j], C1[i] * C1[j]);
        if (i == j) cc += 1.0;
        G[tri(i, j)] = fma(eps, cc, G[tri(i, j)]);
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) rv[j][i] = fma(eps, fma(C0[i], d0[j], C1[i] * d1[j]), rv[j][i]);
    }
    // LDL^T, ONCE (lower, in place; unit L below the diagonal, the diagonal holds 1/d_j): enhance_small_body's
#pragma unroll
    for (int j = 0; j < MR; ++j) {
      ok = ok && (G[tri(j, j)] > 0.0);
      const double rinv = rcp_newton(G[tri(j, j)]);
      G[tri(j, j)] = rinv;
#pragma unroll
      for (int c = j + 1; c < MR; ++c) {
        const double lcj = G[tri(c, j)] * rinv;
#pragma unroll
        for (int i = c; i < MR; ++i) G[tri(i, c)] = fma(-G[tri(i, j)], lcj, G[tri(i, c)]);
        G[tri(c, j)] = lcj;
      }
    }
  }

  // per case: the two triangular solves, status / fallback (Dual.py:164-169), the row through the LDS transpose
  const int64_t base = ((int64_t)block * kBlock + (tid & ~63)) * M;
  const int64_t total = p.ne * M;
  int nfail = 0;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    if (j < nc) {                                           // (uniform: nc is a kernel argument)
      double w[M];
      bool okj = ok;
      if constexpr (MR == 0) {
        w[0] = d0[j];
        w[1] = d1[j];
        okj = isfinite(d0[j]) && isfinite(d1[j]);
      } else {
#pragma unroll
        for (int i = 0; i < MR; ++i) {                      // forward  L y = rhs
          double s = rv[j][i];
#pragma unroll
          for (int q = 0; q < i; ++q) s = fma(-G[tri(i, q)], rv[j][q], s);
          rv[j][i] = s;
        }
#pragma unroll
        for (int i = MR - 1; i >= 0; --i) {                 // backward L^T z = D^-1 y
          double s = rv[j][i] * G[tri(i, i)];
#pragma unroll
          for (int q = i + 1; q < MR; ++q) s = fma(-G[tri(q, i)], rv[j][q], s);
          rv[j][i] = s;
        }
        double w0 = d0[j], w1 = d1[j];
#pragma unroll
        for (int q = 0; q < MR; ++q) {
          const double v = rv[j][q];
          w[q + 2] = v;
          w0 = fma(-C0[q], v, w0);
          w1 = fma(-C1[q], v, w1);
          okj = okj && (fabs(v) < 1.0e300);
        }
        w[0] = w0;
        w[1] = w1;
        okj = okj && (fabs(w0) < 1.0e300) && (fabs(w1) < 1.0e300);
      }
      if (!okj) {
#pragma unroll
        for (int i = 0; i < M; ++i) w[i] = 0.0;
        w[0] = 0.5 * (gl[j] + gr[j]);
        w[1] = 0.5 * (gr[j] - gl[j]);
        if (live) ++nfail;
      }
      if (live && p.status) {
        int32_t* const sj = p.status + (int64_t)j * p.ne + ec;
        const int st = okj ? LSSVR_ST_OK : LSSVR_ST_FALLBACK;
        if (total <= kWriteThroughMaxDoubles) __hip_atomic_store(sj, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else *sj = st;
      }
      // coalesced store: the wave transposes its 64 x M tile through its own LDS (the staging reads, and the
      // previous case's tile reads, are done)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < M; ++i) wt[lane * M + i] = w[i];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      double* const Wj = p.W + (int64_t)j * total;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const int64_t idx = base + (int64_t)i * 64 + lane;
        if (idx < total) {
          // small outputs written through, large ones non-temporal (see kWriteThroughMaxDoubles)
          if (total <= kWriteThroughMaxDoubles)
            __hip_atomic_store(&Wj[idx], wt[i * 64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          else __builtin_nontemporal_store(wt[i * 64 + lane], &Wj[idx]);
        }
      }
    }
  }
  if (nfail && p.fail_count) atomicAdd(p.fail_count, nfail);   // once per (case, element)
}

template <int M, int RHS, bool RX, int NC>
__global__ __launch_bounds__(kBlock) void enhance_multi_kernel(EnhanceMultiArgs p) {
  __shared__ double tile[(kBlock / 64) * kMultiTilePerWave<M, RHS, RX, NC>];
  enhance_multi_body<M, RHS, RX, NC>(p, blockIdx.x, tile);
}

// ----------------------------------------------------------------------------
// dispatch: ceil(ncases / RC) passes, each on its own slice of the case-major arrays
// ----------------------------------------------------------------------------
template <int M, int NC>
static hipError_t launch_multi_pass(const EnhanceMultiArgs& a, hipStream_t s, const LaunchOpts* o) {
  const dim3 grid((unsigned)((a.ne + kBlock - 1) / kBlock)), blk(kBlock);
  const bool pm = a.tab_ps != 1;
  if (a.c_values) {
    if (pm) return launch(enhance_multi_kernel<M, LSSVR_RHS_ARRAY_PM, true, NC>, grid, blk, s, o, a);
    return launch(enhance_multi_kernel<M, LSSVR_RHS_ARRAY, true, NC>, grid, blk, s, o, a);
  }
  if (pm) return launch(enhance_multi_kernel<M, LSSVR_RHS_ARRAY_PM, false, NC>, grid, blk, s, o, a);
  return launch(enhance_multi_kernel<M, LSSVR_RHS_ARRAY, false, NC>, grid, blk, s, o, a);
}

template <int M>
static hipError_t launch_multi(const EnhanceMultiArgs& a0, int ncases, hipStream_t s, const LaunchOpts* o) {
  constexpr int RC = kMultiRC<M>;
  for (int c0 = 0; c0 < ncases; c0 += RC) {
    EnhanceMultiArgs a = a0;
    a.nc = ncases - c0 < RC ? ncases - c0 : RC;
    a.u += (int64_t)c0 * (a.ne + 1);
    a.rhs_values += (int64_t)c0 * a.ne * a.n;
    a.W += (int64_t)c0 * a.ne * M;
    if (a.status) a.status += (int64_t)c0 * a.ne;
    if (a.bc_values) a.bc_values += 2 * (int64_t)c0;
    // a timed call: the first pass carries the begin stamp, the last one the end stamp
    LaunchOpts lo;
    if (o && c0 == 0) lo.start = o->start;
    if (o && c0 + RC >= ncases) lo.stop = o->stop;
    hipError_t e;
    if constexpr (RC > 1) {
      e = a.nc == 1 ? launch_multi_pass<M, 1>(a, s, &lo) : launch_multi_pass<M, RC>(a, s, &lo);
    } else {
      e = launch_multi_pass<M, 1>(a, s, &lo);
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int enhance_multi_rc(int M) { return (M >= 2 && M <= kReactSmallMaxM) ? multi_rc(M) : 1; }

#define LSSVR_RANGE_MULTI(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#define LSSVR_MULTI_CASE(MM) \
  case MM:                   \
    return launch_multi<MM>(a, ncases, s, o);
static_assert(kReactSmallMaxM == 16, "LSSVR_RANGE_MULTI instantiates M = 2 .. kReactSmallMaxM");
hipError_t enhance_multi(const EnhanceMultiArgs& a, int ncases, hipStream_t s, const LaunchOpts* o) {
  switch (a.M) {
    LSSVR_RANGE_MULTI(LSSVR_MULTI_CASE)
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace lssvr
