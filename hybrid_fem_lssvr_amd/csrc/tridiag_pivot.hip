// Device tridiagonal solve WITH PIVOTING, for the P1 systems that tridiag.hip must not be given: negative or
// sign-changing reaction (Helmholtz, turning points), cell Peclet number above 1, a weak inflow Robin end -- any
// non-singular tridiagonal matrix, diagonally dominant or not.  Row i is
// lo[i] x[i-1] + d[i] x[i] + up[i] x[i+1] = r[i]; the symmetric caller passes `off` for both bands.
//
// Algorithm: a recursive partitioned solve with scaled partial pivoting inside every partition, after Klein and
// Strzodka, "Tridiagonal GPU solver with scaled partial pivoting at maximum bandwidth" (ICPP 2021).
//
// Partitions.  One thread owns kP consecutive rows i0 .. i0+kP-1 (the last partition of a level may be shorter).
// Its first and last unknown are the interface unknowns, the kP-2 between them the inner ones.
//
// Reduce.  A downward sweep carries ONE row with three coefficients -- on x[i0], x[k] and x[k+1] -- and its
// right-hand side, starting from row i0+1.  Step k eliminates x[k] between the carried row and row k+1: the row whose
// coefficient on x[k] is larger relative to that row's own largest entry is the pivot row (compared by cross
// multiplication, no division), the other row, updated, is carried on.  After the step that uses row i0+kP-1 the
// carried row couples x[i0], x[i0+kP-1] and x[i0+kP].  The mirrored upward sweep gives a row that couples x[i0-1],
// x[i0] and x[i0+kP-1].  In the order (first_0, last_0, first_1, last_1, ...) these rows are a tridiagonal system of
// two unknowns per partition (one for a last partition of a single row), which is reduced the same way until at most
// kPivBase unknowns remain.  No row is ever padded in: every step k has the real row k+1 to choose from, so with
// nonzero off-diagonals one of the two candidates is nonzero whatever the inner block looks like.  The inner
// (kP-2) x (kP-2) block may be exactly singular while the matrix is harmless (a Helmholtz wavenumber that is a
// Dirichlet eigenvalue of a run of kP-1 elements).  The sweeps survive that, the reduced system does not -- there is no
// Schur complement onto the two interface unknowns then --, so such a partition is shifted by one row first
// (piv_shift_wanted below).
//
// Coarsest level (<= kPivBase unknowns): the sequential elimination of LAPACK's dgtsv -- at every step the better of
// the current row and the next -- with the same scaled row choice, on a system held in LDS.  Lane q of the first
// wave runs it for case q; the matrix part is the same in every lane.  (The cyclic reduction of tridiag.hip's base
// level does not pivot and is not used.)
//
// Substitute.  With both interface values (and the next partition's first) known, a thread repeats the downward
// elimination over its rows i0+1 .. i0+kP-1 -- same data, same code, hence the same pivot decisions --, keeps the
// kP-2 pivot rows in registers (a pivot row that came from a swap has two upper coefficients) and substitutes back.
//
// Several right-hand sides.  The pivot decisions and multipliers depend on the matrix alone: they are taken once per
// partition, then the cases of a pass go through the right-hand-side recurrences one after the other, as in
// tri_condense_kernel<NC>.  The operations of a case do not depend on NC or on its slot (-ffp-contract=off): row q of
// a multi call has the bits of the one-case call on case q.
//
// Ends.  As in tridiag.hip's free solve: a free (Robin / Neumann) end keeps its node as an unknown, kappa joins its
// diagonal and g its right-hand side where the kernels read them; a Dirichlet end hands its neighbour's row
// coefficient * value.  kappa may have any sign.  The caller's bands are never written.
//
// Breakdown word.  Every pivot is checked after the row choice; one that is zero or not finite is counted and its
// reciprocal replaced by 0, so nothing divides by it.  Each thread writes its count to a flag of its own in the
// workspace, together with the flags of the four partitions of the level below that its rows came from; the coarsest
// level adds its own count and stores the total.  No atomics, and no kernel that only adds.  (A pivot that is tiny but
// nonzero is not counted: a matrix that is singular only up to rounding yields large finite values and info == 0.)
//
// No LDS outside the coarsest level, no atomics, no scratch; FP64; one reciprocal per pivot.
#include <cfloat>
#include <vector>

#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"

#define LSSVR_PIV_HD __host__ __device__ __forceinline__

namespace lssvr {

namespace {

// Rows per partition.  8 is the starting point the chunk measurements of tridiag.hip suggest for this access pattern
// (a thread's 64-byte run of each array, loaded back to back); other values are not measured yet.  Each level
// shrinks the system by kP / 2.
constexpr int kP = 8;
// Unknowns of the coarsest level: one lane walks them one after the other.  Measured on an MI355X, a call of that
// size alone (end-value kernel + this level): 42 us with 128 unknowns, 14 us with 32.  In a call of 1e6 unknowns the
// smaller level is paid for by one more level of three launches: 150.2 / 323.2 us (1 / 8 cases) with 128 against
// 150.3 / 333.5 us with 32 -- no gain there; 32 keeps the serial part small for the small systems of the facade.
constexpr int kPivBase = 32;

// The m unknowns of one level for the cases of one pass.  r is the right-hand side of the first case, case c is
// c * rs doubles further on.  Top level only: bl / br the coefficient that ties row 0 / row m-1 to a Dirichlet end
// (NULL at a free end), f0 / f1 a free end, whose row gets k0 / k1 on the diagonal and the end value of the case on the
// right-hand side; bc[c][2] the end values (NULL: zeros).  Reduced levels have none of these.  1 <= nlive <= NC cases
// are live; slot q >= nlive repeats case nlive-1 (loads in bounds) and stores nothing.
struct PivSys {
  const double* lo;
  const double* d;
  const double* up;
  const double* r;
  const double* bl;
  const double* br;
  const double* bc;
  double k0, k1;
  int f0, f1;
  int64_t m, rs;
  int nlive;
};

LSSVR_PIV_HD double lo_at(const PivSys& s, int64_t i) { return i == 0 ? 0.0 : s.lo[i]; }
LSSVR_PIV_HD double up_at(const PivSys& s, int64_t i) { return i == s.m - 1 ? 0.0 : s.up[i]; }
LSSVR_PIV_HD double d_at(const PivSys& s, int64_t i) {
  double v = s.d[i];
  if (i == 0 && s.f0) v += s.k0;
  if (i == s.m - 1 && s.f1) v += s.k1;
  return v;
}
LSSVR_PIV_HD double r_at(const PivSys& s, int c, int64_t i) {
  double v = s.r[c * s.rs + i];
  if (i == 0 && (s.bl || s.f0)) {
    const double e = s.bc ? s.bc[2 * c] : 0.0;
    v = s.bl ? v - s.bl[0] * e : v + e;
  }
  if (i == s.m - 1 && (s.br || s.f1)) {
    const double e = s.bc ? s.bc[2 * c + 1] : 0.0;
    v = s.br ? v - s.br[0] * e : v + e;
  }
  return v;
}
template <int NC>
LSSVR_PIV_HD int case_of(const PivSys& s, int q) {
  if constexpr (NC == 1)
    return 0;
  else
    return q < s.nlive ? q : s.nlive - 1;
}

// The carried row of a sweep: a on the partition's far interface unknown, b on x[k], c on the unknown after x[k] in
// the direction of the sweep.
struct Carry {
  double a, b, c;
};
// The pivot row of a step: (pa on the far interface unknown,) the pivot on x[k], pc and pe on the next two unknowns;
// rp = 1 / pivot, or 0 for a pivot that is zero or not finite.
struct PivRow {
  double pa, pc, pe, rp;
};

// One elimination step: x[k] between the carried row and the next row (l on x[k], d and u on the two unknowns after
// it).  Scaled partial pivoting: the carried row is the pivot row when |b| / max|carried| >= |l| / max|next|.  The
// other row minus f times the pivot row is carried on; f is returned, the right-hand sides follow with
//   swap ? (pivot rhs = r_next, carried rhs = g - f r_next) : (pivot rhs = g, carried rhs = r_next - f g).
LSSVR_PIV_HD double piv_step(Carry& cr, double l, double d, double u, bool& swap, PivRow& pr, int& bad) {
  const double s1 = fmax(fmax(fabs(cr.a), fabs(cr.b)), fabs(cr.c));
  const double s2 = fmax(fmax(fabs(l), fabs(d)), fabs(u));
  swap = !(fabs(cr.b) * s2 >= fabs(l) * s1);
  const double p = swap ? l : cr.b;
  const bool ok = fabs(p) > 0.0 && fabs(p) <= DBL_MAX;
  bad += ok ? 0 : 1;
  pr.rp = ok ? 1.0 / p : 0.0;
  const double f = (swap ? cr.b : l) * pr.rp;
  pr.pa = swap ? 0.0 : cr.a;
  pr.pc = swap ? d : cr.c;
  pr.pe = swap ? u : 0.0;
  const double oa = swap ? cr.a : 0.0, oc = swap ? cr.c : d, oe = swap ? 0.0 : u;
  cr.a = oa - f * pr.pa;
  cr.b = oc - f * pr.pc;
  cr.c = oe - f * pr.pe;
  return f;
}

// the rows of partition j, i0 .. i0+len-1, back to back into registers (the reason is in tridiag.hip's ChunkRows);
// entries t >= len copy row i0 and are never used
struct PartRows {
  double lo[kP], d[kP], up[kP];
};
LSSVR_PIV_HD void load_rows(const PivSys& s, int64_t i0, int len, PartRows& rb) {
#pragma unroll
  for (int t = 0; t < kP; ++t) {
    const int64_t i = t < len ? i0 + t : i0;
    rb.lo[t] = lo_at(s, i);
    rb.d[t] = d_at(s, i);
    rb.up[t] = up_at(s, i);
  }
}
LSSVR_PIV_HD void load_case_rows(const PivSys& s, int c, int64_t i0, int len, double (&r)[kP]) {
#pragma unroll
  for (int t = 0; t < kP; ++t) r[t] = r_at(s, c, t < len ? i0 + t : i0);
}

// A partition whose inner block is singular, or nearly so, has no usable Schur complement onto its two interface
// unknowns: both sweeps then return (nearly) the same combination of the inner rows, and the rows i0 and i0+len-1 are
// lost to the reduced system in the measure in which the block is singular.  Such a partition can be SHIFTED: x[i0]
// is eliminated with its own row (pivot d[i0]), row i0+1 takes over as the partition's first row -- its lower
// coefficient now ties it to x[i0-1], the last unknown of the partition before -- and the rows i0+1 .. i0+len-1 are
// reduced as usual.  Two consecutive minors of a tridiagonal matrix with nonzero off-diagonals never vanish together,
// so the shifted partition's inner block is sound when the full one is singular.
// The choice has no gap.  The QUALITY of a partition is what the last step of its upward sweep finds: the carried
// row's coefficient on x[i0+1] relative to that row's largest entry, over the same ratio of row i0 -- the weight with
// which row i0 enters the reduced row, 1 at best, rounding level for a singular inner block; the solve loses about
// 1 / quality of its accuracy in that partition.  At kShiftTry or above the partition stays as it is (at most 8 bits).
// Below it the shifted partition's quality -- the smaller of |d[i0]| relative to row i0's largest entry and of the
// same last-step ratio of the shifted rows -- is computed too, and the better of the two is taken.
// x[i0] = c0 + e0 x[i0-1] + e1 x[i0+1]; the partition before has x[i0] in its last reduced row and in its back
// substitution, and replaces it by that expression (piv_fixup_kernel, and xn in piv_subst_partition).
constexpr double kShiftTry = 0x1p-8;

// numerator and denominator of the quality of rows 0 .. len-1 (len >= 3): |b| max|row 0| and |up[0]| max|carried|
LSSVR_PIV_HD void piv_up_quality(const PartRows& rb, int len, double& num, double& den) {
  Carry cu{0.0, 0.0, 0.0};
  int bad = 0;
#pragma unroll
  for (int t = kP - 2; t >= 1; --t) {
    if (t == len - 2) cu = Carry{rb.up[t], rb.d[t], rb.lo[t]};
    if (t >= 2 && t <= len - 2) {
      bool sw;
      PivRow pr;
      piv_step(cu, rb.up[t - 1], rb.d[t - 1], rb.lo[t - 1], sw, pr, bad);
    }
  }
  const double s1 = fmax(fmax(fabs(cu.a), fabs(cu.b)), fabs(cu.c));
  const double s2 = fmax(fmax(fabs(rb.up[0]), fabs(rb.d[0])), fabs(rb.lo[0]));
  num = fabs(cu.b) * s2;
  den = fabs(rb.up[0]) * s1;
}

// x[i0] = c0 + e0 x[i0-1] + e1 x[i0+1] with c0 = r[i0] rp0; w = lo[i0+1] rp0 is the multiplier of row i0 in row i0+1
struct ShiftRow {
  double e0, e1, w, rp0;
};
// rows 1 .. kP-1 move to 0 .. kP-2, the new row 0 with x[i0] eliminated
LSSVR_PIV_HD ShiftRow piv_shift_rows(PartRows& rb) {
  ShiftRow sr;
  sr.rp0 = 1.0 / rb.d[0];
  sr.e0 = -(rb.lo[0] * sr.rp0);
  sr.e1 = -(rb.up[0] * sr.rp0);
  sr.w = rb.lo[1] * sr.rp0;
  const double lo0 = -(sr.w * rb.lo[0]), d0 = rb.d[1] - sr.w * rb.up[0];
#pragma unroll
  for (int t = 0; t < kP - 1; ++t) {
    rb.lo[t] = rb.lo[t + 1];
    rb.d[t] = rb.d[t + 1];
    rb.up[t] = rb.up[t + 1];
  }
  rb.lo[0] = lo0;
  rb.d[0] = d0;
  return sr;
}
// the right-hand sides follow; returns c0
LSSVR_PIV_HD double piv_shift_case(const ShiftRow& sr, double (&r)[kP]) {
  const double c0 = r[0] * sr.rp0, r0 = r[1] - sr.w * r[0];
#pragma unroll
  for (int t = 0; t < kP - 1; ++t) r[t] = r[t + 1];
  r[0] = r0;
  return c0;
}

LSSVR_PIV_HD bool piv_shift_wanted(const PartRows& rb, int len) {
  if (len < 3) return false;
  double n0, d0;
  piv_up_quality(rb, len, n0, d0);
  if (!(n0 < kShiftTry * d0)) return false;
  const double s2 = fmax(fmax(fabs(rb.up[0]), fabs(rb.d[0])), fabs(rb.lo[0]));
  if (!(fabs(rb.d[0]) > 0.0 && fabs(rb.d[0]) <= DBL_MAX)) return false;
  double q1 = fabs(rb.d[0]) / s2;
  if (len - 1 >= 3) {
    PartRows sb = rb;
    piv_shift_rows(sb);
    double n1, d1;
    piv_up_quality(sb, len - 1, n1, d1);
    if (n1 < q1 * d1) q1 = n1 / d1;
  }
  return q1 > n0 / d0;
}

// What a level keeps about its shifted partitions: on[np], e0[np], e1[np], c0[nlive][np] (the last three written and
// read for shifted partitions only).
struct ShiftStore {
  int* on;
  double* e0;
  double* e1;
  double* c0;
  int64_t np;
};

// Partition j of np: its two interface rows into rows 2j (first) and 2j+1 (last) of the reduced system LO, D, UP [M],
// R[nlive][M]; a last partition of one row hands that row on as row 2j.  flag[j] = the pivots of this thread that
// were zero or not finite + child[4j .. 4j+3], the flags of the partitions of the level below that rows i0 .. i0+7
// came from (flag NULL: not counted).
template <int NC>
LSSVR_PIV_HD void piv_reduce_partition(const PivSys& s, int64_t j, int64_t M, double* LO, double* D, double* UP,
                                       double* R, const int* child, int64_t nchild, int* flag,
                                       const ShiftStore& ss) {
  const int64_t i0 = j * kP;
  const int len0 = s.m - i0 < kP ? (int)(s.m - i0) : kP;
  int len = len0;
  PartRows rb;
  load_rows(s, i0, len, rb);
  const bool shift = piv_shift_wanted(rb, len);
  ShiftRow sr{0.0, 0.0, 0.0, 0.0};
  if (shift) {
    sr = piv_shift_rows(rb);
    len = len0 - 1;
    ss.e0[j] = sr.e0;
    ss.e1[j] = sr.e1;
  }
  ss.on[j] = shift ? 1 : 0;
  int bad = 0;
  double fd[kP - 2], fu[kP - 2];       // multipliers of the downward and of the upward sweep
  unsigned md = 0, mu = 0;             // their swap bits
  Carry cd{rb.lo[1], rb.d[1], rb.up[1]};
#pragma unroll
  for (int t = 1; t <= kP - 2; ++t) {
    fd[t - 1] = 0.0;
    if (t + 1 < len) {
      bool sw;
      PivRow pr;
      fd[t - 1] = piv_step(cd, rb.lo[t + 1], rb.d[t + 1], rb.up[t + 1], sw, pr, bad);
      md |= (sw ? 1u : 0u) << (t - 1);
    }
  }
  Carry cu{0.0, 0.0, 0.0};
#pragma unroll
  for (int t = kP - 2; t >= 0; --t) {
    if (t == len - 2) cu = Carry{rb.up[t], rb.d[t], rb.lo[t]};
    if (t >= 1) {
      fu[t - 1] = 0.0;
      if (t <= len - 2) {
        bool sw;
        PivRow pr;
        fu[t - 1] = piv_step(cu, rb.up[t - 1], rb.d[t - 1], rb.lo[t - 1], sw, pr, bad);
        mu |= (sw ? 1u : 0u) << (t - 1);
      }
    }
  }
  const int64_t k = 2 * j;
  if (len >= 2) {
    LO[k] = cu.c;
    D[k] = cu.b;
    UP[k] = cu.a;
    LO[k + 1] = cd.a;
    D[k + 1] = cd.b;
    UP[k + 1] = cd.c;
  } else {
    LO[k] = rb.lo[0];
    D[k] = rb.d[0];
    UP[k] = rb.up[0];
  }
  if (flag) {
#pragma unroll
    for (int t = 0; t < kP / 2; ++t)
      if ((kP / 2) * j + t < nchild) bad += child[(kP / 2) * j + t];
    flag[j] = bad;
  }
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    double r[kP];
    load_case_rows(s, case_of<NC>(s, q), i0, len0, r);
    double c0 = 0.0;
    if (shift) c0 = piv_shift_case(sr, r);
    double gd = r[1];
#pragma unroll
    for (int t = 1; t <= kP - 2; ++t)
      if (t + 1 < len) gd = ((md >> (t - 1)) & 1u) ? gd - fd[t - 1] * r[t + 1] : r[t + 1] - fd[t - 1] * gd;
    double gu = 0.0;
#pragma unroll
    for (int t = kP - 2; t >= 0; --t) {
      if (t == len - 2) gu = r[t];
      if (t >= 1 && t <= len - 2)
        gu = ((mu >> (t - 1)) & 1u) ? gu - fu[t - 1] * r[t - 1] : r[t - 1] - fu[t - 1] * gu;
    }
    if (q < s.nlive) {
      if (shift) ss.c0[q * ss.np + j] = c0;
      if (len >= 2) {
        R[q * M + k] = gu;
        R[q * M + k + 1] = gd;
      } else {
        R[q * M + k] = r[0];
      }
    }
  }
}

// Partition j >= 1 is shifted: the last reduced row of partition j-1, row 2j-1, has its upper coefficient on x[i0];
// x[i0] = c0 + e0 x[i0-1] + e1 x[i0+1], and x[i0-1], x[i0+1] are the reduced unknowns 2j-1 and 2j.
LSSVR_PIV_HD void piv_fixup_partition(int64_t j, int64_t M, double* D, double* UP, double* R, int nlive,
                                      const ShiftStore& ss) {
  if (!ss.on[j]) return;
  const int64_t k = 2 * j - 1;
  const double c = UP[k];
  D[k] = D[k] + c * ss.e0[j];
  UP[k] = c * ss.e1[j];
  for (int q = 0; q < nlive; ++q) R[q * M + k] = R[q * M + k] - c * ss.c0[q * ss.np + j];
}

// Partition j with its interface values X[nlive][M] known: the downward elimination again, the kP-2 pivot rows kept,
// then back substitution; x + q*xs (length m) receives the whole level's solution of case q.
template <int NC>
LSSVR_PIV_HD void piv_subst_partition(const PivSys& s, int64_t j, int64_t M, const double* X, double* x, int64_t xs,
                                      const ShiftStore& ss) {
  int64_t i0 = j * kP;
  const int len0 = s.m - i0 < kP ? (int)(s.m - i0) : kP;
  int len = len0;
  PartRows rb;
  load_rows(s, i0, len, rb);
  const bool shift = ss.on[j] != 0;
  const bool next_shift = j + 1 < ss.np && ss.on[j + 1] != 0;
  ShiftRow sr{0.0, 0.0, 0.0, 0.0};
  if (shift) {
    sr = piv_shift_rows(rb);
    len = len0 - 1;
  }
  const int64_t i1 = shift ? i0 + 1 : i0;      // the first row of the partition as it is reduced
  int bad = 0;                         // (counted by the reduce kernel: the same pivots)
  double f[kP - 2];
  PivRow pr[kP - 2];
  unsigned msk = 0;
  Carry cd{rb.lo[1], rb.d[1], rb.up[1]};
#pragma unroll
  for (int t = 1; t <= kP - 2; ++t) {
    f[t - 1] = 0.0;
    pr[t - 1] = PivRow{0.0, 0.0, 0.0, 0.0};
    if (t + 1 < len) {
      bool sw;
      f[t - 1] = piv_step(cd, rb.lo[t + 1], rb.d[t + 1], rb.up[t + 1], sw, pr[t - 1], bad);
      msk |= (sw ? 1u : 0u) << (t - 1);
    }
  }
  const int64_t k = 2 * j;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const int c = case_of<NC>(s, q);
    const double xf = X[c * M + k];
    const double xl = len >= 2 ? X[c * M + k + 1] : 0.0;
    double xn = k + 2 < M ? X[c * M + k + 2] : 0.0;
    if (next_shift) xn = (ss.c0[c * ss.np + j + 1] + ss.e0[j + 1] * xl) + ss.e1[j + 1] * xn;
    double r[kP];
    load_case_rows(s, c, i0, len0, r);
    double c0 = 0.0;
    if (shift) c0 = piv_shift_case(sr, r);
    double y[kP - 2];
    double g = r[1];
#pragma unroll
    for (int t = 1; t <= kP - 2; ++t) {
      y[t - 1] = 0.0;
      if (t + 1 < len) {
        const bool sw = (msk >> (t - 1)) & 1u;
        y[t - 1] = sw ? r[t + 1] : g;
        g = sw ? g - f[t - 1] * r[t + 1] : r[t + 1] - f[t - 1] * g;
      }
    }
    if (q < s.nlive) {
      double* xq = x + q * xs;
      if (shift) xq[i0] = (c0 + sr.e0 * (j > 0 ? X[c * M + k - 1] : 0.0)) + sr.e1 * xf;
      xq[i1] = xf;
      if (len >= 2) xq[i1 + len - 1] = xl;
      double xa = xl, xb = xn;         // x[t+1] and x[t+2]
#pragma unroll
      for (int t = kP - 2; t >= 1; --t) {
        if (t + 1 < len) {
          const PivRow& p = pr[t - 1];
          const double xt = (((y[t - 1] - p.pa * xf) - p.pc * xa) - p.pe * xb) * p.rp;
          xq[i1 + t] = xt;
          xb = xa;
          xa = xt;
        }
      }
    }
  }
}

// Coarsest level, one lane and one case: lo, d, up, r hold the m rows.  Forward: the pivot row of step k replaces row k
// (d <- 1/pivot, up <- pc, lo <- pe; write_matrix: only one lane writes them, they are the same in all) and r[k] its
// right-hand side; the last carried row gives x[m-1].  Returns the zero / non-finite pivots; g and rp_last go on to
// the back substitution.
LSSVR_PIV_HD int piv_base_forward(double* lo, double* d, double* up, double* r, int m, bool write_matrix, double& g,
                                  double& rp_last) {
  int bad = 0;
  Carry cr{0.0, d[0], up[0]};
  g = r[0];
  for (int k = 0; k + 1 < m; ++k) {
    const double l2 = lo[k + 1], d2 = d[k + 1], u2 = up[k + 1], r2 = r[k + 1];
    bool sw;
    PivRow pr;
    const double f = piv_step(cr, l2, d2, u2, sw, pr, bad);
    r[k] = sw ? r2 : g;
    g = sw ? g - f * r2 : r2 - f * g;
    if (write_matrix) {
      d[k] = pr.rp;
      up[k] = pr.pc;
      lo[k] = pr.pe;
    }
  }
  const double p = cr.b;
  const bool ok = fabs(p) > 0.0 && fabs(p) <= DBL_MAX;
  bad += ok ? 0 : 1;
  rp_last = ok ? 1.0 / p : 0.0;
  return bad;
}
// x[k] = (r[k] - pc x[k+1] - pe x[k+2]) / pivot from the rows piv_base_forward left; x: nullptr stores nothing
LSSVR_PIV_HD void piv_base_backward(const double* lo, const double* d, const double* up, const double* r, int m,
                                    double g, double rp_last, double* x) {
  double xa = g * rp_last, xb = 0.0;
  if (x) x[m - 1] = xa;
  for (int k = m - 2; k >= 0; --k) {
    const double xt = ((r[k] - up[k] * xa) - lo[k] * xb) * d[k];
    if (x) x[k] = xt;
    xb = xa;
    xa = xt;
  }
}

template <int NC>
__global__ __launch_bounds__(kBlock) void piv_reduce_kernel(PivSys s, int64_t np, int64_t M, double* __restrict__ LO,
                                                            double* __restrict__ D, double* __restrict__ UP,
                                                            double* __restrict__ R, const int* __restrict__ child,
                                                            int64_t nchild, int* __restrict__ flag, ShiftStore ss) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= np) return;
  piv_reduce_partition<NC>(s, j, M, LO, D, UP, R, child, nchild, flag, ss);
}

// after the reduce kernel: the rows 2j-1 that lie before a shifted partition j = 1 .. np-1
__global__ __launch_bounds__(kBlock) void piv_fixup_kernel(int64_t M, double* __restrict__ D, double* __restrict__ UP,
                                                           double* __restrict__ R, int nlive, ShiftStore ss) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x + 1;
  if (j >= ss.np) return;
  piv_fixup_partition(j, M, D, UP, R, nlive, ss);
}

template <int NC>
__global__ __launch_bounds__(kBlock) void piv_subst_kernel(PivSys s, int64_t np, int64_t M,
                                                           const double* __restrict__ X, double* __restrict__ x,
                                                           int64_t xs, ShiftStore ss) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= np) return;
  piv_subst_partition<NC>(s, j, M, X, x, xs, ss);
}

// One workgroup of kPivBase threads loads the m <= kPivBase rows and the NC right-hand sides into LDS,
// (3 + NC) * 256 bytes, and the flags of the level below; lane q < NC then solves case q.  info (NULL: not counted)
// receives this level's count + child[0 .. nchild).
template <int NC>
__global__ __launch_bounds__(kPivBase) void piv_base_kernel(PivSys s, double* __restrict__ x, int64_t xs,
                                                            const int* __restrict__ child, int nchild,
                                                            int* __restrict__ info) {
  __shared__ double lo[kPivBase], d[kPivBase], up[kPivBase], r[NC][kPivBase];
  __shared__ int cf[kPivBase];
  const int i = threadIdx.x;
  const int m = (int)s.m;
  if (i < m) {
    lo[i] = lo_at(s, i);
    d[i] = d_at(s, i);
    up[i] = up_at(s, i);
#pragma unroll
    for (int q = 0; q < NC; ++q) r[q][i] = r_at(s, case_of<NC>(s, q), i);
  }
  cf[i] = (info && i < nchild) ? child[i] : 0;
  __syncthreads();
  double g = 0.0, rp_last = 0.0;
  int bad = 0;
  if (i < NC) bad = piv_base_forward(lo, d, up, r[i], m, i == 0, g, rp_last);
  __syncthreads();
  if (i < NC) piv_base_backward(lo, d, up, r[i], m, g, rp_last, i < s.nlive ? x + i * xs : nullptr);
  if (i == 0 && info) {
    for (int t = 0; t < nchild; ++t) bad += cf[t];
    info[0] = bad;
  }
}

// only a Dirichlet end (f0 / f1 zero) has its value written, a free end is an unknown of the solve (bc NULL: zeros)
__global__ void piv_ends_kernel(double* u, int64_t ne, int nc, const double* bc, int f0, int f1) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nc) return;
  if (!f0) u[q * (ne + 1)] = bc ? bc[2 * q] : 0.0;
  if (!f1) u[q * (ne + 1) + ne] = bc ? bc[2 * q + 1] : 0.0;
}

// partitions and reduced unknowns of a level of m unknowns
int64_t piv_parts(int64_t m) { return (m + kP - 1) / kP; }
int64_t piv_reduced(int64_t m) { return 2 * piv_parts(m) - (m % kP == 1 ? 1 : 0); }
// doubles that hold np int flags
int64_t piv_flag_doubles(int64_t np) { return (np + 1) / 2; }

// workspace (in doubles) of the levels above the coarsest with K cases in a pass: LO, D, UP [3*M] + R, X [K][2*M] +
// the flags + the shifted partitions' on, e0, e1 [np] and c0 [K][np]
int64_t piv_level_doubles(int64_t m, int64_t K) {
  int64_t tot = 0;
  while (m > kPivBase) {
    const int64_t M = piv_reduced(m);
    const int64_t np = piv_parts(m);
    tot += (3 + 2 * K) * M + 2 * piv_flag_doubles(np) + (2 + K) * np + 16;
    m = M;
  }
  return tot + 16;
}

// one level for the NC slots of a pass; child / nchild: the flags of the level below; info NULL: nothing is counted
template <int NC>
hipError_t piv_level(const PivSys& s, double* x, int64_t xs, double* work, const int* child, int64_t nchild,
                     int* info, hipStream_t st) {
  if (s.m <= kPivBase) {
    hipLaunchKernelGGL((piv_base_kernel<NC>), dim3(1), dim3((unsigned)kPivBase), 0, st, s, x, xs, child, (int)nchild,
                       info);
    return hipGetLastError();
  }
  const int64_t np = piv_parts(s.m), M = piv_reduced(s.m);
  const int64_t K = s.nlive;
  double* LO = work;
  double* D = LO + M;
  double* UP = D + M;
  double* R = UP + M;
  double* X = R + K * M;
  int* flag = reinterpret_cast<int*>(X + K * M);
  double* e0 = X + K * M + piv_flag_doubles(np);
  const ShiftStore ss{reinterpret_cast<int*>(e0 + (2 + K) * np), e0, e0 + np, e0 + 2 * np, np};
  double* next = e0 + (2 + K) * np + piv_flag_doubles(np) + 16;
  const unsigned grid = (unsigned)((np + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((piv_reduce_kernel<NC>), dim3(grid), dim3(kBlock), 0, st, s, np, M, LO, D, UP, R, child, nchild,
                     info ? flag : nullptr, ss);
  if (np > 1)
    hipLaunchKernelGGL(piv_fixup_kernel, dim3((unsigned)((np - 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, M, D,
                       UP, R, s.nlive, ss);
  const PivSys red{LO, D, UP, R, nullptr, nullptr, nullptr, 0.0, 0.0, 0, 0, M, M, s.nlive};
  const hipError_t err = piv_level<NC>(red, X, M, next, flag, np, info, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((piv_subst_kernel<NC>), dim3(grid), dim3(kBlock), 0, st, s, np, M, X, x, xs, ss);
  return hipGetLastError();
}

// The same level on the host, partition by partition through the routines the kernels call: what tridiag_pivot_host
// below runs, and what the tests without a GPU check.
template <int NC>
void piv_level_host(const PivSys& s, double* x, int64_t xs, const int* child, int64_t nchild, int* info) {
  if (s.m <= kPivBase) {
    const int m = (int)s.m;
    int total = 0;
    std::vector<double> lo(m), d(m), up(m), r(m);
    for (int q = 0; q < s.nlive; ++q) {
      for (int i = 0; i < m; ++i) {
        lo[i] = lo_at(s, i);
        d[i] = d_at(s, i);
        up[i] = up_at(s, i);
        r[i] = r_at(s, q, i);
      }
      double g, rp;
      const int bad = piv_base_forward(lo.data(), d.data(), up.data(), r.data(), m, true, g, rp);
      piv_base_backward(lo.data(), d.data(), up.data(), r.data(), m, g, rp, x + q * xs);
      if (q == 0) total = bad;
    }
    for (int64_t t = 0; t < nchild; ++t) total += child[t];
    if (info) info[0] = total;
    return;
  }
  const int64_t np = piv_parts(s.m), M = piv_reduced(s.m);
  const int64_t K = s.nlive;
  std::vector<double> LO(M), D(M), UP(M), R(K * M), X(K * M), e0(np), e1(np), c0(K * np);
  std::vector<int> flag(np), on(np);
  const ShiftStore ss{on.data(), e0.data(), e1.data(), c0.data(), np};
  for (int64_t j = 0; j < np; ++j)
    piv_reduce_partition<NC>(s, j, M, LO.data(), D.data(), UP.data(), R.data(), child, nchild, flag.data(), ss);
  for (int64_t j = 1; j < np; ++j) piv_fixup_partition(j, M, D.data(), UP.data(), R.data(), s.nlive, ss);
  const PivSys red{LO.data(), D.data(), UP.data(), R.data(), nullptr, nullptr, nullptr, 0.0, 0.0, 0, 0, M, M, s.nlive};
  piv_level_host<NC>(red, X.data(), M, flag.data(), np, info);
  for (int64_t j = 0; j < np; ++j) piv_subst_partition<NC>(s, j, M, X.data(), x, xs, ss);
}

}  // namespace

// tridiag_pivot_solve on HOST arrays (bc and info included), without a device: the same partition routines, levels
// and passes.  For checking the arithmetic where there is no GPU; it is not a fast path.
void tridiag_pivot_host(const double* diag, const double* sub, const double* sup, const double* load, int64_t ne,
                        int nc, bool f0, bool f1, double k0, double k1, const double* bc, double* u, int32_t* info) {
  for (int q = 0; q < nc; ++q) {
    if (!f0) u[q * (ne + 1)] = bc ? bc[2 * q] : 0.0;
    if (!f1) u[q * (ne + 1) + ne] = bc ? bc[2 * q + 1] : 0.0;
  }
  if (info) info[0] = 0;
  const int sh = f0 ? 0 : 1;
  const int64_t m = ne - 1 + (f0 ? 1 : 0) + (f1 ? 1 : 0);
  if (m <= 0) return;
  const PivSys all{sub + sh - 1, diag + sh, sup + sh, load + sh, f0 ? nullptr : sub, f1 ? nullptr : sup + (ne - 1),
                   bc,           k0,        k1,       f0 ? 1 : 0, f1 ? 1 : 0, m, ne + 1, 0};
  const int64_t stride = ne + 1;
  for (int q0 = 0; q0 < nc; q0 += kTriMultiCases) {
    PivSys s = all;
    s.nlive = nc - q0 < kTriMultiCases ? nc - q0 : kTriMultiCases;
    if (s.bc) s.bc += 2 * (int64_t)q0;
    s.r += q0 * stride;
    double* xq = u + sh + q0 * stride;
    int* cnt = q0 == 0 ? reinterpret_cast<int*>(info) : nullptr;
    if (s.nlive == 1)
      piv_level_host<1>(s, xq, stride, nullptr, 0, cnt);
    else
      piv_level_host<kTriMultiCases>(s, xq, stride, nullptr, 0, cnt);
  }
}

// sized for two free ends, ne + 1 unknowns, whatever the kinds of a call are; it grows with nc up to kTriMultiCases
int64_t tridiag_pivot_work_bytes(int64_t ne, int nc) {
  return 8 * piv_level_doubles(ne + 1, nc < kTriMultiCases ? (nc > 1 ? nc : 1) : kTriMultiCases) + 256;
}

// The bands diag[ne+1], sub[ne], sup[ne] (sub[i]: u_i in row i+1, sup[i]: u_{i+1} in row i) and load[nc][ne+1] ->
// u[nc][ne+1], with the unknowns, shifts and end terms of tridiag.hip's free_solve.  The cases run in passes of
// kTriMultiCases; the pivots are counted in the first pass only (they are the same in every pass).
hipError_t tridiag_pivot_solve(const double* diag, const double* sub, const double* sup, const double* load,
                               int64_t ne, int nc, bool f0, bool f1, double k0, double k1, const double* bc, double* u,
                               int32_t* info, void* work, hipStream_t st) {
  if (!f0 || !f1)
    hipLaunchKernelGGL(piv_ends_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, st, u, ne, nc, bc, (int)f0,
                       (int)f1);
  const int sh = f0 ? 0 : 1;
  const int64_t m = ne - 1 + (f0 ? 1 : 0) + (f1 ? 1 : 0);
  if (m <= 0) {
    if (info) {
      const hipError_t err = hipMemsetAsync(info, 0, sizeof(int32_t), st);
      if (err != hipSuccess) return err;
    }
    return hipGetLastError();
  }
  const PivSys all{sub + sh - 1, diag + sh, sup + sh, load + sh, f0 ? nullptr : sub, f1 ? nullptr : sup + (ne - 1),
                   bc,           k0,        k1,       f0 ? 1 : 0, f1 ? 1 : 0, m, ne + 1, 0};
  const int64_t stride = ne + 1;
  for (int q0 = 0; q0 < nc; q0 += kTriMultiCases) {
    PivSys s = all;
    s.nlive = nc - q0 < kTriMultiCases ? nc - q0 : kTriMultiCases;
    if (s.bc) s.bc += 2 * (int64_t)q0;
    s.r += q0 * stride;
    double* xq = u + sh + q0 * stride;
    int* cnt = q0 == 0 ? reinterpret_cast<int*>(info) : nullptr;
    const hipError_t err =
        s.nlive == 1 ? piv_level<1>(s, xq, stride, reinterpret_cast<double*>(work), nullptr, 0, cnt, st)
                     : piv_level<kTriMultiCases>(s, xq, stride, reinterpret_cast<double*>(work), nullptr, 0, cnt, st);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace lssvr
