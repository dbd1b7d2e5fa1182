// Per-element LSSVR enhancement, large-degree path for POISSON rows (23 <= M <= 33; any M >= 2 on
// request): the Chebyshev-moment form of the Legendre Gram contraction (DESIGN.md section 2b,
// enhance_small_cheb.hpp) as a SEQUENCE of kernels with a caller-provided workspace in between.
//
//   G_ik = sum_k' T_i(t_k') T_k(t_k') = 1/2 (m_{i+k} + m_{|i-k|}),   m_d = sum_k' T_d(t_k'), d <= 60:
// the 31 x 31 Gram matrix of a degree-32 element is determined by 61 power sums -- O(n M) work per
// element instead of the O(n M^2) of the direct contraction (which enhance_large.hip runs on the f64
// matrix cores and which stays in the library for variable-coefficient rows, subsets, callers
// without a workspace and as LSSVR_SOLVER_PRIMAL_WAVE, the A/B reference: DESIGN.md section 7).
//
//   moments_kernel: ONE ELEMENT PER LANE.  The lane walks the collocation points of its element:
//     abscissa and t_k in numpy's arithmetic, f(x_k) by the rotation-carried (sin, cos) pair with
//     numpy's argument rounding restored to first order (enhance_small_cheb.hpp), T_0..T_30 by the
//     two-term recurrence with two registers of state, and accumulates m_1..m_30 (adds), the squares
//     T_j^2 (j = 16..30) and neighbour products T_j T_{j+1} (j = 15..29) that give the upper moments
//     (T_j^2 = (T_2j + T_0)/2, T_j T_{j+1} = (T_{2j+1} + T_1)/2), and the right-hand side
//     r_i = sum T_i phi: 91 accumulators, ~135 instructions per point, no cross-lane traffic.  The
//     96 numbers per element (moments, end points, boundary values, r) go to the workspace.  The
//     kernel is the same for every M (degree 30 always).
//   solve: n >= 2 (M-2): solve4_parity_kernel of enhance_large_parity.hip (even / odd split);
//     otherwise solve4_kernel below, rounds of FOUR elements per wave: lane (g = lane >> 4,
//     q = lane & 15) builds columns q and q + 16 of  S2 = m_{i+c} + m_{|i-c|} + 2 eps (N + C_z^T C_z)
//     straight from the moments (two conflict-free LDS reads, one table read and four FMAs per
//     entry; first-order boundary rows and compile-time ridge tables as in the lane kernel), the
//     right-hand side rides along as row / column 31, then the four-systems-per-wave DPP-broadcast
//     LDL^T of lssvr_wave.hpp (16 lanes per system, two columns per lane, factor frozen in
//     registers, no LDS, no cross-row permutes), DPP back-substitution, v = Y z through LDS,
//     w_{0,1} by row reductions; n <= M + 12: followed by refinement steps (residual_kernel +
//     solve4_kernel<2>).
// MEASURED (MI355X, M = 33, 64 points): 242 us at 1e5 elements and 2.04 ms at 1e6 with solve4_kernel,
// 195 us and 1.5 ms with the parity-split solve, against 352-395 us and 3.2 ms of enhance_large.hip.
// (A fused single-kernel form of the two phases -- sixteen elements per wave, moments through LDS
// atomics -- took 407-490 us / 3.3-3.9 ms: 91 accumulators plus 128 column registers leave two
// long-lived waves per SIMD.  It was removed; DESIGN.md section 3.8 keeps its numbers.)
#include "cheb_tables.hpp"
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_wave.hpp"

namespace lssvr {

using namespace wave;

namespace {

constexpr int kReseedLarge = 64;         // rotation-carried rhs: re-seeded every 64 points
constexpr int kTop = 30;                 // highest Chebyshev degree of a row (M = 33)

// sum over the 16 lanes of a DPP row
__device__ __forceinline__ double row_sum16(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// zero-padded device copies of the constant tables for run-time indexed reads
struct ChebDeviceTables {
  double Y[32][64];      // Y[j][i] = cheb::kY[j][i]  (v = Y z), zero beyond 30
  double N[32][32];      // N = Y^T Y
  double alpha[32], b[32], slope[32];
};

constexpr ChebDeviceTables make_cheb_device_tables() {
  ChebDeviceTables t{};
  for (int j = 0; j < 31; ++j) {
    for (int i = 0; i < 31; ++i) {
      t.Y[j][i] = cheb::kY[j][i];
      t.N[j][i] = cheb::kN[j][i];
    }
    t.alpha[j] = cheb::kAlpha[j];
    t.b[j] = cheb::kB[j];
    t.slope[j] = cheb::kSlope[j];
  }
  return t;
}

__device__ const ChebDeviceTables kTab = make_cheb_device_tables();

// X = Y^-1 (rho_j = sum_i X[i][j] T_i), zero padded: the ridge-dominated cold path only
struct ChebInverseTable {
  double X[32][32];
};
constexpr ChebInverseTable make_cheb_inverse_table() {
  ChebInverseTable t{};
  for (int i = 0; i < 31; ++i)
    for (int j = 0; j < 31; ++j) t.X[i][j] = cheb::kX[i][j];
  return t;
}
__device__ const ChebInverseTable kInv = make_cheb_inverse_table();

}  // namespace


// ---------------------------------------------------------------------------------------------
// The solve of four elements (one per 16-lane DPP row), from their moments mo[0..60], end points
// and boundary values (mo[61..63], ro[31]) and right-hand sides ro[0..30] (LDS, this lane's
// element) to the stored coefficient row.  Lane (g = lane >> 4, q = lane & 15) owns columns q and
// q + 16 of its element's system.  Z: this row's 64 doubles of LDS ([32, 64) stay zero).
// ---------------------------------------------------------------------------------------------
// Ntab (row stride 32) / Ytab (row stride 64): LDS copies of the device tables.
// MODE (iterative refinement of the near-square regime, refine_steps() below): 0 = plain solve;
// 1 = also store the Chebyshev coefficients z to zout[0..32); 2 = a refinement step: ro[] holds
// sum_k T_i(t_k) e_k of the point residual e = phi2 - 2 T zold (residual_kernel), the ridge part
// of the residual is formed here from the ridge entries of S as they are built, the solve gives
// the correction and z = zold + dz goes on to W and to zout.
template <int MODE>
__device__ __forceinline__ void solve_four(const EnhanceArgs& p, const int lane, const int64_t e_raw,
                                           const double* __restrict__ mo,
                                           const double* __restrict__ ro, double* __restrict__ Z,
                                           const double* __restrict__ Ntab,
                                           const double* __restrict__ Ytab,
                                           const double* __restrict__ zold = nullptr,
                                           double* __restrict__ zout = nullptr) {
  const int M = p.M, MR = M - 2;
  int q = lane & 15;
  asm volatile("" : "+v"(q));
  Z[32 + q] = 0.0;
  Z[48 + q] = 0.0;
  const int cA = q, cB = q + 16;
  const bool inA = cA < MR, inB = cB < MR;
  const double alA = inA ? kTab.alpha[cA] : 0.0, bA = inA ? kTab.b[cA] : 0.0;
  const double alB = inB ? kTab.alpha[cB] : 0.0, bB = inB ? kTab.b[cB] : 0.0;
  const double slA = kTab.slope[cA], slB = kTab.slope[cB < 31 ? cB : 30];
  const bool q_even = (q & 1) == 0;                 // cA and cB have the parity of q

  {
    bool live = e_raw < p.ne;
    const int64_t e = live ? e_raw : p.ne - 1;
    int64_t id = e;
    if (p.elem_ids) {
      id = p.elem_ids[e];
      if (id < 0 || id >= p.ne_mesh) {     // out-of-range id: nothing of the mesh is touched
        if (live && q == 0 && p.fail_count) atomicAdd(p.fail_count, 1);
        live = false;
        id = 0;
      }
    }
    const double a = mo[61], b = mo[62], gl = mo[63], gr = ro[31];
    const double inv_gamma = p.gamma_values ? rcp_newton(p.gamma_values[id]) : p.inv_gamma;
    const DomainMap dm = map_params(a, b);
    const double hh = 0.5 * dm.oldlen;
    const double inv_scl2 = hh * hh;
    const double eps2 = (2.0 * inv_gamma) * (inv_scl2 * inv_scl2);
    if (ridge_dominated(eps2, M)) live = false;       // solved by ridge_fixup_kernel

    // ---- boundary rows to first order (enhance_small_cheb.hpp); exact recurrence when the wave
    // holds an element beyond the first-order range
    const double ta = dm.off + dm.scl * a;
    const double tb = dm.off + dm.scl * b;
    const double ea = 1.0 + ta, eb = 1.0 - tb;
    const double sig = 0.5 * (ea + eb), del = 0.5 * (ea - eb);
    const double amax = 0.5 * (double)((M - 1) * M);
    const bool slow = amax * fmax(fabs(ea), fabs(eb)) >= 1.0e-6;
    const bool any_slow = __any(slow);
    double idet = 0.5 * fma(sig, 1.0 + sig, 1.0);
    if (any_slow) idet = rcp_newton(tb - ta);
    const double d0 = (tb * gl - ta * gr) * idet;
    const double d1 = (gr - gl) * idet;
    // this lane's own (C0, C1) of w_{0,1} = d - C v for its two columns (v-basis)
    double C0A, C1A, C0B, C1B;
    if (q_even) {
      C0A = fma(-slA, sig, 1.0);
      C1A = slA * del;
      C0B = fma(-slB, sig, 1.0);
      C1B = slB * del;
    } else {
      C0A = (slA - 1.0) * del;
      C1A = fma(-(slA - 1.0), sig, 1.0);
      C0B = (slB - 1.0) * del;
      C1B = fma(-(slB - 1.0), sig, 1.0);
    }
    double C0zA = 0.0, C1zA = 0.0, C0zB = 0.0, C1zB = 0.0;    // cold path: columns of C_z = C Y
    if (any_slow) {
      // exact L_{c+2}(ta), L_{c+2}(tb) by the Legendre recurrence, latched at degrees cA+2, cB+2
      double am1 = 1.0, a0 = ta, bm1 = 1.0, b0 = tb;
      double LaA = 0.0, LbA = 0.0, LaB = 0.0, LbB = 0.0;
      for (int m = 1; m <= MR; ++m) {
        const double inv = 1.0 / (double)(m + 1);
        const double a1 = ((double)(2 * m + 1) * ta * a0 - (double)m * am1) * inv;
        const double b1 = ((double)(2 * m + 1) * tb * b0 - (double)m * bm1) * inv;
        am1 = a0; a0 = a1;
        bm1 = b0; b0 = b1;
        if (m == cA + 1) { LaA = a1; LbA = b1; }
        if (m == cB + 1) { LaB = a1; LbB = b1; }
      }
      C0A = (tb * LaA - ta * LbA) * idet;
      C1A = (LbA - LaA) * idet;
      C0B = (tb * LaB - ta * LbB) * idet;
      C1B = (LbB - LaB) * idet;
      if (!inA) C0A = C1A = 0.0;
      if (!inB) C0B = C1B = 0.0;
      // C_z[., c] = sum_{j <= c, j = c mod 2} C[., j] Y[j][c]; C[., j] lives in lane (j & 15) of
      // this 16-lane row, first or second column (cold path: plain shuffles)
      const int rowbase = lane & ~15;
      for (int t = 0; t < 16; ++t) {
        const int jA = cA - 2 * t, jB = cB - 2 * t;
        const int sA = rowbase + ((jA >= 0 ? jA : 0) & 15), sB = rowbase + ((jB >= 0 ? jB : 0) & 15);
        const double a0A = __shfl(C0A, sA), a1A = __shfl(C1A, sA);       // jA < 16 always
        const double b0lo = __shfl(C0A, sB), b1lo = __shfl(C1A, sB);
        const double b0hi = __shfl(C0B, sB), b1hi = __shfl(C1B, sB);
        if (jA >= 0 && inA) {
          const double y = Ytab[jA * 64 + cA];
          C0zA = fma(a0A, y, C0zA);
          C1zA = fma(a1A, y, C1zA);
        }
        if (jB >= 0 && inB) {
          const double y = Ytab[jB * 64 + cB];
          C0zB = fma(jB < 16 ? b0lo : b0hi, y, C0zB);
          C1zB = fma(jB < 16 ? b1lo : b1hi, y, C1zB);
        }
      }
    }
    if (!inA) C0A = C1A = 0.0;
    if (!inB) C0B = C1B = 0.0;

    // ---- right-hand side entries of this lane's columns, then the two columns of S2 --------------
    double rhsA = 0.0, rhsB = 0.0;
    [[maybe_unused]] double rzA = 0.0, rzB = 0.0;      // MODE 2: (ridge part of S) zold, this lane's columns
    const double e_d = eps2 * (q_even ? d0 : d1);
    const double q_c = eps2 * (q_even ? fma(del, d1, -(sig * d0)) : fma(del, d0, -(sig * d1)));
    if constexpr (MODE != 2) {
      if (any_slow) {
        rhsA = fma(eps2, fma(C0zA, d0, C1zA * d1), ro[cA]);
        rhsB = fma(eps2, fma(C0zB, d0, C1zB * d1), ro[cB]);
      } else {
        rhsA = fma(bA, q_c, fma(alA, e_d, ro[cA]));
        rhsB = fma(bB, q_c, fma(alB, e_d, ro[cB]));
      }
      if (!inA) rhsA = 0.0;
      if (!inB) rhsB = 0.0;
      wave_lds_sync();                 // previous round's readers of Z are done
      Z[cA] = rhsA;
      Z[cB] = rhsB;
      wave_lds_sync();
    }
    double A[kLP], B[kLP];
    {
      const double es = eps2 * sig, ed = eps2 * del;
      const int cBc = cB < 31 ? cB : 0;                    // (lane 15's second column is the rhs)
      // the 62 table entries N[i][c] first, straight into the column registers: all loads in
      // flight at once
#pragma unroll
      for (int i = 0; i < kLP - 1; ++i) {
        A[i] = Ntab[i * 32 + cA];
        B[i] = Ntab[i * 32 + cBc];
      }
      // one column at a time (half the coefficient registers live): first-order ridge
      //   same parity:  eps2 (N_ic + al_i al_c) - es (al_i b_c + b_i al_c),   opposite:  ed (al_i b_c + b_i al_c)
      auto column = [&](double (&X)[kLP], const int cx, const double alc, const double bc,
                        const double C0z, const double C1z, const bool inx, [[maybe_unused]] double& rz) {
        const double u1 = fma(eps2, alc, -(es * bc)), u2 = -(es * alc), u3 = ed * bc, u4 = ed * alc;
        const double Xe = q_even ? u1 : u3, Ye = q_even ? u2 : u4;       // even rows
        const double Xo = q_even ? u3 : u1, Yo = q_even ? u4 : u2;       // odd rows
#pragma unroll
        for (int i = 0; i < kLP - 1; ++i) {
          double v = mo[i + cx] + mo[(i >= cx) ? i - cx : cx - i];
          if (any_slow) {
            // C_z[., i]: lane (i & 15) of the row, first / second column
            const int si = (lane & ~15) + (i & 15);
            const double f0 = __shfl(i < 16 ? C0zA : C0zB, si), f1 = __shfl(i < 16 ? C1zA : C1zB, si);
            if constexpr (MODE == 2) rz = fma(eps2 * fma(f0, C0z, fma(f1, C1z, X[i])), zold[i], rz);
            v = fma(eps2, fma(f0, C0z, fma(f1, C1z, X[i])), v);
          } else {
            if constexpr (MODE == 2)
              rz = fma(fma(cheb::kB[i], (i & 1) ? Yo : Ye, fma(cheb::kAlpha[i], (i & 1) ? Xo : Xe, eps2 * X[i])),
                       zold[i], rz);
            v = fma(eps2, X[i], v);
            v = fma(cheb::kAlpha[i], (i & 1) ? Xo : Xe, v);
            v = fma(cheb::kB[i], (i & 1) ? Yo : Ye, v);
          }
          X[i] = inx ? v : 0.0;
        }
      };
      column(A, cA, alA, bA, C0zA, C1zA, inA, rzA);
      column(B, cBc, alB, bB, C0zB, C1zB, inB, rzB);
      if constexpr (MODE == 2) {
        // residual of the normal equations: the Gram part through the points (ro), the ridge part here
        const double ridA = any_slow ? eps2 * fma(C0zA, d0, C1zA * d1) : fma(bA, q_c, alA * e_d);
        const double ridB = any_slow ? eps2 * fma(C0zB, d0, C1zB * d1) : fma(bB, q_c, alB * e_d);
        rhsA = inA ? ro[cA] + (ridA - rzA) : 0.0;
        rhsB = inB ? ro[cB] + (ridB - rzB) : 0.0;
        wave_lds_sync();
        Z[cA] = rhsA;
        Z[cB] = rhsB;
        wave_lds_sync();
      }
      if (cB == kRhsRow) {           // column 31 carries the right-hand side as a column
#pragma unroll
        for (int i = 0; i < kLP - 1; ++i) B[i] = Z[i];
      }
      A[kRhsRow] = rhsA;             // ... and every column carries it as row 31
      B[kRhsRow] = rhsB;
    }

    // ---- LDL^T factor + solve of the MR x MR block, four systems in lock step -----------------
    bool lane_ok;
    double zA, zB;
    ldlt_solve_dpp4(A, B, q, MR, lane_ok, zA, zB);
    if constexpr (MODE == 2) {
      zA += zold[cA];
      zB += zold[cB];                  // (zold[31] = 0)
    }
    if constexpr (MODE >= 1) {
      if (e_raw < p.ne) {
        zout[cA] = inA ? zA : 0.0;
        zout[cB] = inB ? zB : 0.0;
      }
    }
    // v = Y z (bubble Legendre coefficients): v_j = sum_{i >= j, i = j mod 2} Y[j][i] z_i
    wave_lds_sync();
    Z[cA] = inA ? zA : 0.0;
    Z[cB] = inB ? zB : 0.0;
    wave_lds_sync();
    double vA = 0.0, vB = 0.0;
    {
      const int jB = cB < 31 ? cB : 30;
      double yA[16], yB[16];             // (all 32 table loads in flight before the first use)
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        yA[t] = Ytab[cA * 64 + cA + 2 * t];
        yB[t] = Ytab[jB * 64 + cB + 2 * t];
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        vA = fma(yA[t], Z[cA + 2 * t], vA);
        vB = fma(yB[t], Z[cB + 2 * t], vB);
      }
      if (!inA) vA = 0.0;
      if (!inB) vB = 0.0;
    }
    const double w0 = d0 - row_sum16(fma(C0A, vA, C0B * vB));
    const double w1 = d1 - row_sum16(fma(C1A, vA, C1B * vB));
    const double bad = row_sum16((lane_ok && fabs(vA) < 1.0e300 && fabs(vB) < 1.0e300) ? 0.0 : 1.0);
    const bool ok = (bad == 0.0) && (fabs(w0) < 1e300) && (fabs(w1) < 1e300);

    // ---- store: lane q -> W[e][q+2], W[e][q+18]; lane 0 also writes w0, w1 -------------------
    if (live) {
      double* const Wrow = p.W + id * (p.ldw ? p.ldw : (int64_t)M);
      if (inA) Wrow[cA + 2] = ok ? vA : 0.0;
      if (inB) Wrow[cB + 2] = ok ? vB : 0.0;
      if (q == 0) {
        Wrow[0] = ok ? w0 : 0.5 * (gl + gr);
        Wrow[1] = ok ? w1 : 0.5 * (gr - gl);
        if (p.status) p.status[id] = ok ? LSSVR_ST_OK : LSSVR_ST_FALLBACK;
        if (!ok && p.fail_count) atomicAdd(p.fail_count, 1);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// RIDGE-DOMINATED element (lssvr_device.hpp::ridge_dominated): the whole solve of ONE element by the
// wave that accumulated its moments, in the Legendre-bubble basis (the lane kernel's cheb_ridge_solve,
// wave-cooperative):  S2_v = X^T (m_{i+k} + m_{|i-k|}) X + eps2 (I + C^T C),  rhs2_v = X^T r2 + eps2 C^T d,
// exact boundary rows, LDL^T and the substitutions in the wave's LDS tile, then W / status of the element.
// The solve kernels skip such elements (same predicate).  Cold: coarse elements with a small gamma only.
//   rec: the element's 96 workspace numbers (global, written by this wave);  tl: >= 1216 doubles of LDS.
// ---------------------------------------------------------------------------------------------
// (Scalars instead of the EnhanceArgs: a reference would put the kernel's whole argument block on its stack.)
__device__ __attribute__((noinline)) void ridge_wave_solve(double* __restrict__ Wrow, int32_t* __restrict__ status,
                                                           int32_t* __restrict__ fail_count, const int M,
                                                           const double* __restrict__ rec,
                                                           double* __restrict__ tl, const int lane,
                                                           const double eps2) {
  constexpr int kP = 33;                       // row pitch of the matrix
  const int MR = M - 2;
  double* const mo = tl;                       // m_0..m_60 | a b g_l | r_0..r_30 | g_r
  double* const c0 = tl + 96;
  double* const c1 = tl + 128;
  double* const xr = tl + 160;
  double* const S = tl + 192;
  wave_lds_sync();
  // (system-scope loads: the rows were stored write-through by other lanes of this wave)
  mo[lane] = __hip_atomic_load(rec + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (lane < 32) mo[64 + lane] = __hip_atomic_load(rec + 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  wave_lds_sync();
  const double a = mo[61], b = mo[62], gl = mo[63], gr = mo[95];
  const DomainMap dm = map_params(a, b);
  const double ta = dm.off + dm.scl * a;
  const double tb = dm.off + dm.scl * b;
  const double idet = 1.0 / (tb - ta);
  const double d0 = (tb * gl - ta * gr) * idet;
  const double d1 = (gr - gl) * idet;
  if (lane == 0) {                             // exact boundary rows: L_{j+2}(ta), L_{j+2}(tb)
    double am1 = 1.0, a0 = ta, bm1 = 1.0, b0 = tb;
    for (int pp = 1; pp < M - 1; ++pp) {
      const double inv = 1.0 / (double)(pp + 1);
      const double a1 = ((double)(2 * pp + 1) * ta * a0 - (double)pp * am1) * inv;
      const double b1 = ((double)(2 * pp + 1) * tb * b0 - (double)pp * bm1) * inv;
      am1 = a0; a0 = a1;
      bm1 = b0; b0 = b1;
      c0[pp - 1] = (tb * a1 - ta * b1) * idet;
      c1[pp - 1] = (b1 - a1) * idet;
    }
  }
  // A = G2 X  (G2[i][k] = m_{i+k} + m_{|i-k|}), every entry by one lane
  for (int idx = lane; idx < MR * 32; idx += 64) {
    const int i = idx >> 5, j = idx & 31;
    if (j < MR) {
      double s = 0.0;
      for (int k = (j & 1); k <= j; k += 2) {
        const int dk = i > k ? i - k : k - i;
        s = fma(mo[i + k] + mo[dk], kInv.X[k][j], s);
      }
      S[i * kP + j] = s;
    }
  }
  wave_lds_sync();
  // S = X^T A + ridge in place: lane j owns column j (row i reads rows <= i of its own column only, so
  // descending rows need no synchronisation);  rhs2_v likewise
  if (lane < MR) {
    const int j = lane;
    const double c0j = c0[j], c1j = c1[j];
    for (int i = MR - 1; i >= 0; --i) {
      double s = 0.0;
      for (int k = (i & 1); k <= i; k += 2) s = fma(kInv.X[k][i], S[k * kP + j], s);
      double cc = fma(c0[i], c0j, c1[i] * c1j);
      if (i == j) cc += 1.0;
      S[i * kP + j] = fma(eps2, cc, s);
    }
    double r = 0.0;
    for (int i = (j & 1); i <= j; i += 2) r = fma(kInv.X[i][j], mo[64 + i], r);
    xr[j] = fma(eps2, fma(c0j, d0, c1j * d1), r);
  }
  wave_lds_sync();
  // LDL^T (right-looking, lower part; unit L below the diagonal, the diagonal holds 1/d_j)
  bool ok = true;
  for (int j = 0; j < MR; ++j) {
    const double dj = S[j * kP + j];
    ok = ok && (dj > 0.0);
    const double rinv = 1.0 / dj;
    for (int idx = (j + 1) * 32 + lane; idx < MR * 32; idx += 64) {
      const int i = idx >> 5, c = idx & 31;
      if (c > j && c <= i) S[i * kP + c] = fma(-S[i * kP + j], S[c * kP + j] * rinv, S[i * kP + c]);
    }
    wave_lds_sync();
    if (lane > j && lane < MR) S[lane * kP + j] *= rinv;
    if (lane == 0) S[j * kP + j] = rinv;
    wave_lds_sync();
  }
  for (int j = 0; j < MR - 1; ++j) {           // L y = rhs
    const double xj = xr[j];
    if (lane > j && lane < MR) xr[lane] = fma(-S[lane * kP + j], xj, xr[lane]);
    wave_lds_sync();
  }
  if (lane < MR) xr[lane] *= S[lane * kP + lane];
  wave_lds_sync();
  for (int j = MR - 1; j > 0; --j) {           // L^T v = D^-1 y
    const double vj = xr[j];
    if (lane < j) xr[lane] = fma(-S[j * kP + lane], vj, xr[lane]);
    wave_lds_sync();
  }
  const double v = lane < MR ? xr[lane] : 0.0;
  double w0 = d0, w1 = d1;
  for (int j = 0; j < MR; ++j) {               // (every lane the same sum, in order)
    w0 = fma(-c0[j], xr[j], w0);
    w1 = fma(-c1[j], xr[j], w1);
  }
  ok = ok && !__any(!(fabs(v) < 1.0e300)) && (fabs(w0) < 1.0e300) && (fabs(w1) < 1.0e300);
  if (lane < MR) Wrow[lane + 2] = ok ? v : 0.0;
  if (lane == 0) {
    Wrow[0] = ok ? w0 : 0.5 * (gl + gr);
    Wrow[1] = ok ? w1 : 0.5 * (gr - gl);
    if (status) *status = ok ? LSSVR_ST_OK : LSSVR_ST_FALLBACK;
    if (!ok && fail_count) atomicAdd(fail_count, 1);
  }
  wave_lds_sync();
}

// =============================================================================================
// The same two phases as TWO kernels with a caller-provided workspace in between (96 doubles per
// element: lssvr_enhance_work_bytes): the solve kernel then holds nothing but the two columns per
// lane and fits the register budget of three resident waves per SIMD, its waves are short (four
// elements each) and the tables sit in LDS -- what the fused kernel above lacks.
// This pair is the DEFAULT for Poisson rows above M = 22 whenever the caller passes a workspace
// (lssvr_enhance_ws): 242 us at 1e5 elements and 2.04 ms at 1e6 (M = 33, 64 points) against
// 352-395 us and 3.2 ms of enhance_large_kernel; where n >= 2 (M-2) the second kernel is the
// parity-split solve4_parity_kernel of enhance_large_parity.hip instead (195 us / 1.5 ms).
// =============================================================================================
constexpr int kWsStride = kMomentWsStride; // per element: m_0..m_60 at [0, 61), r_0..r_30 at [64, 95)

// Phase 1 alone, ONE ELEMENT PER LANE (no slices, no reduction): 91 accumulators, all points.
constexpr int kMomBlock = 256;
template <int RHS>
__global__ __launch_bounds__(kMomBlock, 2) void moments_kernel(EnhanceArgs p, double* __restrict__ ws) {
  __shared__ double mtile[(kMomBlock / 64) * 64 * 33];      // 16.5 KB per wave: the store transposition
  const int64_t e = (int64_t)blockIdx.x * kMomBlock + threadIdx.x;
  const bool live = e < p.ne;
  const int64_t ec = live ? e : p.ne - 1;
  int64_t id = ec;
  if (p.elem_ids) {
    id = p.elem_ids[ec];
    if (id < 0 || id >= p.ne_mesh) id = 0;
  }
  const int n = p.n;
  const double a = p.x[id];
  const double b = p.x[id + 1];
  const DomainMap dm = map_params(a, b);
  const double step = dm.oldlen / (double)(n - 1);
  const double hh = 0.5 * dm.oldlen;
  const double inv_scl2 = hh * hh;
  double mom[kTop + 1], sq[15], nb[15], rr[kTop + 1];
#pragma unroll
  for (int d = 0; d <= kTop; ++d) mom[d] = rr[d] = 0.0;
#pragma unroll
  for (int j = 0; j < 15; ++j) sq[j] = nb[j] = 0.0;
  double rs = 0.0, rc = 1.0, sd = 0.0, cd = 1.0, th0 = 0.0, dth = 0.0, kappa = 0.0;
  if constexpr (RHS == LSSVR_RHS_SIN) {
    dth = p.rhs_omega * step;
    sincos_tab(dth, sd, cd, p.trig);
    kappa = -2.0 * (p.rhs_amp * inv_scl2);
  }
  [[maybe_unused]] const double fscale = -2.0 * inv_scl2;
  for (int k0 = 0; k0 < n; k0 += kReseedLarge) {
    if constexpr (RHS == LSSVR_RHS_SIN) {
      const double x0 = (k0 == 0) ? a : fma((double)k0, step, a);
      th0 = p.rhs_omega * x0;
      sincos_tab(th0, rs, rc, p.trig);
      rs *= kappa;
      rc *= kappa;
    }
    const int k1 = min(k0 + kReseedLarge, n);
    for (int k = k0; k < k1; ++k) {
      const double xk = (k == n - 1) ? b : (double)k * step + a;
      const double tk = dm.off + dm.scl * xk;
      double phi2;
      if constexpr (RHS == LSSVR_RHS_SIN) {
        const double arg = p.rhs_omega * xk;
        const double delta = fma(-(double)(k - k0), dth, arg - th0);
        phi2 = fma(rc, delta, rs);
        if (__any(!(fabs(delta) < 1.0e-7))) phi2 = kappa * sin_tab(arg, p.trig);
        const double rs_next = fma(rs, cd, rc * sd);
        rc = fma(rc, cd, -(rs * sd));
        rs = rs_next;
      } else {
        phi2 = p.rhs_values[ec * p.tab_es + k * p.tab_ps] * fscale;
      }
      double Tm2 = 1.0, Tm1 = tk;
      const double tt = tk + tk;
      rr[0] += phi2;
      mom[1] += Tm1;
      rr[1] = fma(Tm1, phi2, rr[1]);
#pragma unroll
      for (int d = 2; d <= kTop; ++d) {
        const double Td = fma(tt, Tm1, -Tm2);
        mom[d] += Td;
        rr[d] = fma(Td, phi2, rr[d]);
        if (d - 1 >= 15) nb[d - 1 - 15] = fma(Tm1, Td, nb[d - 1 - 15]);
        if (d >= 16) sq[d - 16] = fma(Td, Td, sq[d - 16]);
        Tm2 = Tm1;
        Tm1 = Td;
      }
    }
  }
  // ---- the 96 numbers of the element -> workspace row, COALESCED: written lane by lane (every store
  // instruction 64 rows apart, 768 B stride) they cost 64 cache-line transactions per instruction --
  // 6 144 per wave, which at 1e5 elements was a third of the kernel (a two-lanes-per-element build with
  // twice the store instructions took 50 us MORE, which is how it showed).  Three passes of 32 columns
  // through a wave-private LDS tile (row pitch 33: conflict-free both ways) turn them into stores of
  // two 256-byte row segments each: 4 full lines per instruction.
  const double m0 = (double)n;
  const int64_t eg = id + p.elem_offset;
  const double gl = (eg == 0 && a == p.gxmin) ? p.bc_left : p.u[id];          // Dual.py:65-75 rule
  const double gr = (eg == p.ne_global - 1 && b == p.gxmax) ? p.bc_right : p.u[id + 1];
  auto column = [&](auto ic) -> double {                 // workspace column `c` of this lane's element
    constexpr int c = decltype(ic)::value;
    if constexpr (c == 0) return m0;
    else if constexpr (c <= kTop) return mom[c];
    else if constexpr (c <= 60) {
      if constexpr (c & 1) return fma(2.0, nb[(c - 1) / 2 - 15], -mom[1]);   // m_{2j+1} = 2 sum T_j T_{j+1} - m_1
      else return fma(2.0, sq[c / 2 - 16], -m0);                            // m_{2j}   = 2 sum T_j^2 - m_0
    } else if constexpr (c == 61) return a;
    else if constexpr (c == 62) return b;
    else if constexpr (c == 63) return gl;
    else if constexpr (c < 95) return rr[c - 64];
    else return gr;
  };
  const int lane = threadIdx.x & 63;
  double* const tl = mtile + (threadIdx.x >> 6) * (64 * 33);
  const int64_t e0 = (int64_t)blockIdx.x * kMomBlock + (threadIdx.x & ~63);      // the wave's first element
  static_for<0, 3>([&](auto pc) {
    constexpr int c0 = decltype(pc)::value * 32;
    wave_lds_sync();                                   // the previous pass's reads are done
    static_for<0, 32>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      tl[lane * 33 + j] = column(std::integral_constant<int, c0 + j>{});
    });
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const int row = 2 * i + (lane >> 5), cc = lane & 31;
      // write-through (system-scope) stores: the rows drain while other waves still accumulate instead of
      // waiting in the caches for the end-of-kernel release that precedes the solve kernel (-3 us of the pair
      // at 1e5 elements, -0.5 % at 1e6: alternating A/B)
      if (e0 + row < p.ne)
        __hip_atomic_store(&ws[(e0 + row) * kWsStride + c0 + cc], tl[row * 33 + cc], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
  });
}

// ---- ridge-dominated elements (coarse elements with a small gamma; none on a BASELINE mesh): the solve kernels skip
// them (lssvr_device.hpp::ridge_dominated) and this kernel, the LAST of the sequence, solves them in the
// Legendre-bubble basis from their workspace rows (ridge_wave_solve): one lane tests one element, a wave solves its
// elements one at a time.  On an ordinary mesh it reads 16 B per element and exits (~2 us of the sequence).
__global__ __launch_bounds__(256) void ridge_fixup_kernel(EnhanceArgs p, const double* __restrict__ ws) {
  __shared__ double rtile[4 * 1216];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool valid = e < p.ne;
  int64_t id = valid ? e : p.ne - 1;
  if (p.elem_ids) {
    id = p.elem_ids[id];
    if (id < 0 || id >= p.ne_mesh) {       // (counted by the solve kernel)
      id = 0;
      valid = false;
    }
  }
  const double h2 = 0.5 * (p.x[id + 1] - p.x[id]);
  const double is2 = h2 * h2;
  const double inv_gamma = p.gamma_values ? rcp_newton(p.gamma_values[id]) : p.inv_gamma;
  const double eps2 = (2.0 * inv_gamma) * (is2 * is2);                 // the solve kernels' expression
  unsigned long long rmask = __ballot(valid && ridge_dominated(eps2, p.M));
  if (!rmask) return;
  const int lane = threadIdx.x & 63;
  double* const tile = rtile + (threadIdx.x >> 6) * 1216;
  const int64_t w0 = e - lane;                       // the wave's first element
  while (rmask) {
    const int t = __builtin_ctzll(rmask);
    rmask &= rmask - 1;
    const int64_t idm = (int64_t)__builtin_bit_cast(
        unsigned long long, readlane_f64(__builtin_bit_cast(double, (unsigned long long)id), t));
    ridge_wave_solve(p.W + idm * (p.ldw ? p.ldw : (int64_t)p.M), p.status ? p.status + idm : nullptr,
                     p.fail_count, p.M, ws + (w0 + t) * kWsStride, tile, lane, readlane_f64(eps2, t));
  }
}

// Phase 2 alone: a workgroup of four waves = sixteen elements (four per wave); the moments come
// from the workspace through LDS, the tables N and Y are copied to LDS once per workgroup (read
// from the device tables they cost every wave ~60 exposed L1/L2 round trips: 58 % of its life in
// s_waitcnt).  Two resident waves per SIMD without spills (216 VGPRs) beat three with 73 spilled
// registers (242 against 263 us at 1e5 elements).  MODE: see solve_four; zws = 32 doubles per element.
constexpr int kS4Stride = 112;           // LDS per element: 96 + 16 (groups of a half on disjoint banks)
constexpr int kS4Waves = 4;
constexpr int kS4WaveDoubles = 4 * kS4Stride + 4 * 64;
constexpr int kZStride = 32;
template <int MODE>
__global__ __launch_bounds__(64 * kS4Waves, 2) void solve4_kernel(EnhanceArgs p,
                                                                   const double* __restrict__ ws,
                                                                   double* __restrict__ zws,
                                                                   unsigned nxcd) {
  __shared__ double2_t lds2[(32 * 32 + 32 * 64 + kS4Waves * kS4WaveDoubles +
                             (MODE == 2 ? kS4Waves * 4 * kZStride : 0)) / 2];
  double* const Nl = reinterpret_cast<double*>(lds2);
  double* const Yl = Nl + 32 * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* const lds = Yl + 32 * 64 + wave * kS4WaveDoubles;
#pragma unroll
  for (int t = 0; t < (32 * 32) / (64 * kS4Waves); ++t)
    Nl[t * 64 * kS4Waves + tid] = (&kTab.N[0][0])[t * 64 * kS4Waves + tid];
#pragma unroll
  for (int t = 0; t < (32 * 64) / (64 * kS4Waves); ++t)
    Yl[t * 64 * kS4Waves + tid] = (&kTab.Y[0][0])[t * 64 * kS4Waves + tid];
  const unsigned xcd = blockIdx.x % nxcd, slot = blockIdx.x / nxcd;
  const int64_t blk = (int64_t)xcd * (gridDim.x / nxcd) + slot;
  const int64_t E0 = (blk * kS4Waves + wave) * 4;
  const int64_t Ec = E0 < p.ne ? E0 : p.ne - 1;       // (a wave past the end works on duplicates, stores masked)
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int idx = k * 64 + lane;                  // 384 = 4 x 96 doubles
    const int el = idx / kWsStride, j = idx % kWsStride;
    const int64_t e = (Ec + el < p.ne) ? Ec + el : p.ne - 1;
    lds[el * kS4Stride + j] = ws[e * kWsStride + j];
  }
  const int g = lane >> 4;
  [[maybe_unused]] double* zl = nullptr;
  if constexpr (MODE == 2) {
    zl = Yl + 32 * 64 + kS4Waves * kS4WaveDoubles + wave * (4 * kZStride);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int idx = k * 64 + lane;                // 128 = 4 x 32 doubles
      const int el = idx / kZStride, j = idx % kZStride;
      const int64_t e = (Ec + el < p.ne) ? Ec + el : p.ne - 1;
      zl[idx] = zws[e * kZStride + j];
    }
    zl += g * kZStride;
  }
  __syncthreads();
  double* const Z = lds + 4 * kS4Stride + g * 64;
  const int64_t eo = (E0 + g < p.ne) ? E0 + g : p.ne - 1;
  solve_four<MODE>(p, lane, E0 + g, lds + g * kS4Stride, lds + g * kS4Stride + 64, Z, Nl, Yl, zl,
                         MODE >= 1 ? zws + eo * kZStride : nullptr);
}

// Point residual of a refinement step, ONE ELEMENT PER LANE like moments_kernel:
//   e_k = phi2_k - 2 sum_i z_i T_i(t_k)  (Clenshaw),   r_i = sum_k T_i(t_k) e_k  -> ws[e][64 + i]
// (the corrected semi-normal equations: the residual goes through the rows, never through the Gram
// matrix, so the correction recovers the digits the normal equations lost -- DESIGN.md section 2).
template <int RHS>
__global__ __launch_bounds__(256) void residual_kernel(EnhanceArgs p, double* __restrict__ ws,
                                                       const double* __restrict__ zws) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = e < p.ne;
  const int64_t ec = live ? e : p.ne - 1;
  int64_t id = ec;                             // position in the launch -> mesh index
  if (p.elem_ids) {
    id = p.elem_ids[ec];
    if (id < 0 || id >= p.ne_mesh) id = 0;     // (skipped by the solve kernel)
  }
  const int n = p.n;
  const double a = p.x[id];
  const double b = p.x[id + 1];
  const DomainMap dm = map_params(a, b);
  const double step = dm.oldlen / (double)(n - 1);
  const double hh = 0.5 * dm.oldlen;
  const double inv_scl2 = hh * hh;
  double z[kTop + 1], rr[kTop + 1];
#pragma unroll
  for (int d = 0; d <= kTop; ++d) {
    z[d] = zws[ec * kZStride + d];
    rr[d] = 0.0;
  }
  double rs = 0.0, rc = 1.0, sd = 0.0, cd = 1.0, th0 = 0.0, dth = 0.0, kappa = 0.0;
  if constexpr (RHS == LSSVR_RHS_SIN) {
    dth = p.rhs_omega * step;
    sincos_tab(dth, sd, cd, p.trig);
    kappa = -2.0 * (p.rhs_amp * inv_scl2);
  }
  [[maybe_unused]] const double fscale = -2.0 * inv_scl2;
  for (int k0 = 0; k0 < n; k0 += kReseedLarge) {
    if constexpr (RHS == LSSVR_RHS_SIN) {
      const double x0 = (k0 == 0) ? a : fma((double)k0, step, a);
      th0 = p.rhs_omega * x0;
      sincos_tab(th0, rs, rc, p.trig);
      rs *= kappa;
      rc *= kappa;
    }
    const int k1 = min(k0 + kReseedLarge, n);
    for (int k = k0; k < k1; ++k) {
      const double xk = (k == n - 1) ? b : (double)k * step + a;
      const double tk = dm.off + dm.scl * xk;
      double phi2;                                     // (the same values as moments_kernel's)
      if constexpr (RHS == LSSVR_RHS_SIN) {
        const double arg = p.rhs_omega * xk;
        const double delta = fma(-(double)(k - k0), dth, arg - th0);
        phi2 = fma(rc, delta, rs);
        if (__any(!(fabs(delta) < 1.0e-7))) phi2 = kappa * sin_tab(arg, p.trig);
        const double rs_next = fma(rs, cd, rc * sd);
        rc = fma(rc, cd, -(rs * sd));
        rs = rs_next;
      } else {
        phi2 = p.rhs_values[ec * p.tab_es + k * p.tab_ps] * fscale;
      }
      const double tt = tk + tk;
      double b1 = 0.0, b2 = 0.0;
#pragma unroll
      for (int d = kTop; d >= 1; --d) {
        const double b0 = fma(tt, b1, z[d]) - b2;
        b2 = b1;
        b1 = b0;
      }
      const double Tz = fma(tk, b1, z[0]) - b2;
      const double ek = fma(-2.0, Tz, phi2);
      double Tm2 = 1.0, Tm1 = tk;
      rr[0] += ek;
      rr[1] = fma(Tm1, ek, rr[1]);
#pragma unroll
      for (int d = 2; d <= kTop; ++d) {
        const double Td = fma(tt, Tm1, -Tm2);
        rr[d] = fma(Td, ek, rr[d]);
        Tm2 = Tm1;
        Tm1 = Td;
      }
    }
  }
  if (!live) return;
  double* const o = ws + e * kWsStride + 64;
#pragma unroll
  for (int i = 0; i <= kTop; ++i) o[i] = rr[i];
}

// Refinement steps of the two-kernel path by the excess of collocation points over bubble
// coefficients: equispaced points with n ~ M-2 make the normal equations lose up to ten digits
// (3e-6 at M = 33, n = 31); each step of the corrected semi-normal equations wins back about three
// (scripts/proto/qr_nearsquare.py; measured envelope in DESIGN.md section 2).
int enhance_refine_steps(int M, int n) {
  const int excess = n - (M - 2);
  if (M <= kSmallMaxM || excess < 0) return 0;
  return excess <= 1 ? 3 : excess <= 4 ? 2 : excess <= 14 ? 1 : 0;
}

// The lane kernel (M <= 22): its normal equations are at 2e-17 from n = M - 2 on up to M = 16 and reach
// 3e-14 (h = 1/12) .. 2e-12 (h = 0.5) at M = 22, n = 20..22: one step of the corrected semi-normal equations
// up to an excess of 6 points, two at an excess <= 1 (measured envelope in DESIGN.md section 2).
int enhance_small_refine_steps(int M, int n) {
  const int excess = n - (M - 2);
  if (M < 14 || M > kSmallMaxM || excess < 0) return 0;
  return excess <= 1 ? 2 : excess <= 6 ? 1 : 0;
}

int64_t enhance_moment_ws_bytes(int64_t ne, int M, int n) {
  return ne * (kWsStride + (enhance_refine_steps(M, n) > 0 ? kZStride : 0)) * (int64_t)sizeof(double);
}

hipError_t enhance_large_split(const EnhanceArgs& a, void* work, hipStream_t s, const LaunchOpts* o) {
  if (a.M - 2 + 1 > kLP || a.a_values || !work) return hipErrorInvalidValue;
  double* const ws = static_cast<double*>(work);
  double* const zws = ws + a.ne * kWsStride;
  const int steps = enhance_refine_steps(a.M, a.n);
  const unsigned nxcd = xcd_count();
  const unsigned b1 = (unsigned)((a.ne + kMomBlock - 1) / kMomBlock);
  int64_t blocks = (a.ne + 4 * kS4Waves - 1) / (4 * kS4Waves);
  blocks = (blocks + nxcd - 1) / nxcd * nxcd;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 g1(b1), t1(kMomBlock), g2((unsigned)blocks), t2(64 * kS4Waves);
  const dim3 gr((unsigned)((a.ne + 255) / 256)), tr(256);                    // residual_kernel
  // profiled launches: the start stamp of the first kernel and the stop stamp of the last --
  // the duration reported is that of the whole sequence, gaps included
  const bool prof = o && o->start && o->stop;
  const bool sine = a.rhs_id == LSSVR_RHS_SIN;
  // (plain launches unless stamped: the hipExt entry only where an event is attached)
  const LaunchOpts first{prof ? o->start : nullptr, nullptr}, last{nullptr, prof ? o->stop : nullptr};
  const double* const cws = ws;
  const double* const czws = zws;
  hipError_t e = sine ? launch(moments_kernel<LSSVR_RHS_SIN>, g1, t1, s, &first, a, ws)
                      : launch(moments_kernel<LSSVR_RHS_ARRAY>, g1, t1, s, &first, a, ws);
  if (e != hipSuccess) return e;
  // ridge-dominated elements, from the finished workspace rows and BEFORE a refinement pass overwrites their
  // right-hand sides; the solve kernels below leave those elements alone
  if ((e = launch(ridge_fixup_kernel, gr, tr, s, nullptr, a, cws)) != hipSuccess) return e;
  if (steps == 0 && enhance_parity_applies(a.M, a.n)) return launch_solve4_parity(a, cws, s, &last);
  if (steps == 0) return launch(solve4_kernel<0>, g2, t2, s, &last, a, cws, (double*)nullptr, nxcd);
  EnhanceArgs quiet = a;           // failures are counted once, by the last pass
  quiet.fail_count = nullptr;
  if ((e = launch(solve4_kernel<1>, g2, t2, s, nullptr, quiet, cws, zws, nxcd)) != hipSuccess) return e;
  for (int it = 1; it <= steps; ++it) {
    e = sine ? launch(residual_kernel<LSSVR_RHS_SIN>, gr, tr, s, nullptr, a, ws, czws)
             : launch(residual_kernel<LSSVR_RHS_ARRAY>, gr, tr, s, nullptr, a, ws, czws);
    if (e != hipSuccess) return e;
    e = launch(solve4_kernel<2>, g2, t2, s, it == steps ? &last : nullptr, it == steps ? a : quiet, cws, zws, nxcd);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace lssvr
