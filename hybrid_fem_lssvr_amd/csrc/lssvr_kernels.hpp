// Internal launch interface between the C-ABI layer (capi.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include "../../include/lssvr_hip.h"
#include "../../include/lssvr_hip_bench.h"   // (measurement entries of the same library)
#include "lssvr_device.hpp"

namespace lssvr {

constexpr int kSmallMaxM = 22;   // lane-per-element path: (M-2)(M-1)/2 Gram entries in VGPRs + AGPRs
// Coefficient tiles up to this many doubles (16 MiB) are stored WRITE-THROUGH (system-scope stores: sc0 sc1):
// an eagerly launched kernel ends with a write-back of its dirty lines before the next dispatch may start, and
// at BASELINE's 1e5 elements (7.2 MB of W) that tail was 0.6 of the kernel's 9.7 us; written through, the lines
// drain while other waves still compute.  Larger outputs keep non-temporal stores (measured: equal from 3e5 to
// 3e6 elements, write-through 2-4 % slower at 1e7).
constexpr int64_t kWriteThroughMaxDoubles = int64_t(1) << 21;
constexpr int kLargeMaxM = 33;   // wave-per-element MFMA path: M-2 bubble coefficients + rhs <= 32

struct EnhanceArgs {
  const double* x;
  const double* u;
  int64_t ne, elem_offset, ne_global;
  double gxmin, gxmax, bc_left, bc_right, gamma;
  double inv_gamma;         // 1 / gamma, rounded on the host (the scalar-gamma path divides nowhere)
  int M, n;
  int refine;               // lane kernel, Poisson rows: refinement steps of the near-square regime (0: none)
  int rhs_id;
  double rhs_amp, rhs_omega;
  const double* rhs_values;
  const double* a_values;   // non-null => variable-coefficient rows
  const double* da_values;
  // tabulated arrays (rhs_values, a_values, da_values): entry (element e of the launch, point k)
  // is t[e * tab_es + k * tab_ps] -- element-major (n, 1) or point-major (1, launch count)
  int64_t tab_es, tab_ps;
  // heterogeneous launches (lssvr_enhance_subset): local element k of the launch is mesh
  // element elem_ids[k] (NULL: k itself) -- node / nodal-value / gamma_values / status / W
  // rows are addressed by the MESH index, the tabulated arrays (rhs_values, a_values,
  // da_values) by k; gamma_values[mesh index] replaces gamma when non-NULL; W rows are ldw
  // doubles apart (0 = M)
  // An id outside [0, ne_mesh) touches NOTHING (no load, no store; status has no slot for
  // it): the element is skipped and counted in fail_count.
  const int64_t* elem_ids;
  int64_t ne_mesh;          // elements of the mesh the ids index (== ne when elem_ids is NULL)
  const double* gamma_values;
  int64_t ldw;
  double* W;
  int32_t* status;
  int32_t* fail_count;
  TrigTables trig;          // sin / cos polynomial coefficients (SGPR operands), set by capi.hip
};

// reaction rows -(a u')' + c u = f: the variable-coefficient arguments plus the c table (same layout as the other
// three).  A struct of its own: the kernels that take EnhanceArgs keep their argument block.
struct EnhanceReactArgs : EnhanceArgs {
  const double* c_values;
};

// several load cases on one mesh (lssvr_enhance_multi, enhance_multi.hip): u, rhs_values, W and status are
// case-major ([case][ne+1], [case][ne*n], [case][ne*M], [case][ne]) and point at the first case of the pass;
// bc_values[case][2] = {left, right} lives on the DEVICE (NULL: zeros) and replaces bc_left / bc_right; c_values
// may be NULL (variable-coefficient rows)
struct EnhanceMultiArgs : EnhanceReactArgs {
  const double* bc_values;
  int nc;                   // cases of this pass (set by enhance_multi)
};

// Optional per-launch profiling: a kernel with an event attached (start, stop, or both; either may be
// NULL) goes through hipExtLaunchKernelGGL, which stamps them with the dispatch's own begin/end times.
struct LaunchOpts {
  hipEvent_t start = nullptr;
  hipEvent_t stop = nullptr;
};

template <typename K, typename... Args>
inline hipError_t launch(K kernel, dim3 grid, dim3 block, hipStream_t s, const LaunchOpts* o,
                         Args... args) {
  if (o && (o->start || o->stop))
    hipExtLaunchKernelGGL(kernel, grid, block, 0, s, o->start, o->stop, 0, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
  return hipGetLastError();
}

// XCDs (L2 domains) of the current device, hipDeviceAttributeNumberOfXccs (8 on MI355X); cached
// per device, 1 when the runtime cannot say.  Used only for L2-affine workgroup numbering.
inline unsigned xcd_count() {
  static thread_local int cached_dev = -1;
  static thread_local unsigned cached = 1;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  if (dev != cached_dev) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess || v < 1) v = 1;
    cached = (unsigned)v;
    cached_dev = dev;
  }
  return cached;
}

// compute units of the current device (256 on MI355X), cached like xcd_count(); sizes persistent grids
inline unsigned cu_count() {
  static thread_local int cached_dev = -1;
  static thread_local unsigned cached = 1;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  if (dev != cached_dev) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 1;
    cached = (unsigned)v;
    cached_dev = dev;
  }
  return cached;
}

hipError_t enhance_small(const EnhanceArgs& a, hipStream_t s, const LaunchOpts* o = nullptr);
hipError_t enhance_large(const EnhanceArgs& a, hipStream_t s, const LaunchOpts* o = nullptr);
// reaction rows (a.a_values, a.da_values, a.c_values, a.rhs_values non-null), primal solve, n >= M - 2: the lane
// kernel up to kReactSmallMaxM (the degrees it holds in registers without scratch), the MFMA kernel above
constexpr int kReactSmallMaxM = 16;
hipError_t enhance_small_react(const EnhanceReactArgs& a, hipStream_t s, const LaunchOpts* o = nullptr);
hipError_t enhance_large_react(const EnhanceReactArgs& a, hipStream_t s, const LaunchOpts* o = nullptr);
// ncases load cases, M <= kReactSmallMaxM: one factorisation per element and pass, enhance_multi_rc(M) cases a pass
int enhance_multi_rc(int M);
hipError_t enhance_multi(const EnhanceMultiArgs& a, int ncases, hipStream_t s, const LaunchOpts* o = nullptr);
// Poisson rows, any M <= 33: Chebyshev-moment Gram (enhance_large_cheb.hip, enhance_large_parity.hip): a
// sequence of kernels with a workspace of enhance_moment_ws_bytes(ne, M, n) bytes in between
int enhance_refine_steps(int M, int n);
int enhance_small_refine_steps(int M, int n);   // the lane kernel's rule (M <= kSmallMaxM)
int64_t enhance_moment_ws_bytes(int64_t ne, int M, int n);
hipError_t enhance_large_split(const EnhanceArgs& a, void* work, hipStream_t s, const LaunchOpts* o = nullptr);
// the well-posed regime (n >= 2 (M-2)) of the two-kernel path: parity-split solve (enhance_large_parity.hip)
constexpr int kMomentWsStride = 96;   // workspace doubles per element: m_0..m_60, a, b, g_l, r_0..r_30, g_r
bool enhance_parity_applies(int M, int n);
hipError_t launch_solve4_parity(const EnhanceArgs& a, const double* ws, hipStream_t s, const LaunchOpts* o);
hipError_t enhance_dual(const EnhanceArgs& a, hipStream_t s, const LaunchOpts* o = nullptr);
constexpr int kSharedMaxM = 33;  // shared-operator path (uniform meshes): coefficients in VGPRs
hipError_t enhance_shared(const EnhanceArgs& a, const double* op, hipStream_t s,
                          const LaunchOpts* o = nullptr);

hipError_t colloc_points(const double* x, int64_t ne, int n, double* xc, hipStream_t s, bool point_major = false);
// the same abscissae for the nsub elements ids[0..nsub) of a mesh of ne_mesh elements (ids NULL: all, in order), by
// position in the list; an id outside [0, ne_mesh) writes nothing
hipError_t colloc_points_subset(const double* x, int64_t ne_mesh, const int64_t* ids, int64_t nsub, int n, double* xc,
                                hipStream_t s, bool point_major);

struct QuadRule {
  double xi[5];
  double wt[5];
};

struct P1Args {
  const double* x;
  int64_t ne;
  int nquad;
  int rhs_id;
  double rhs_amp, rhs_omega;
  const double* rhs_quad;
  const double* a_quad;
  double* diag;
  double* off;
  double* load;
  double* kloc;
  double* floc;
};
hipError_t p1_assemble(const P1Args& a, hipStream_t s);
// -(a u')' + c u: P1Args plus c at the quadrature points; the consistent mass matrix joins diag and off
struct P1ReactArgs : P1Args {
  const double* c_quad;
};
hipError_t p1_assemble_react(const P1ReactArgs& a, hipStream_t s);
// -(a u')' + b u' + c u (p1_conv.hip): plus b at the quadrature points; the matrix is no longer symmetric, so `off`
// is unused and the two off-diagonal bands are sub[ne] (u_i in row i+1) and sup[ne] (u_{i+1} in row i).  a_quad,
// c_quad and b_quad may each be NULL.
struct P1ConvArgs : P1ReactArgs {
  const double* b_quad;
  double* sub;
  double* sup;
};
hipError_t p1_assemble_conv(const P1ConvArgs& a, hipStream_t s);
// The same equation with the hierarchic bubbles of degree 2 .. order condensed out of every element (p1_bubble.hip,
// DESIGN.md section 37): R tabulated right-hand sides rhs_quad[R][ne][nquad] -> the bands of P1ConvArgs and
// load[R][ne+1]; kloc4[ne][4] (the condensed element matrices S00, S01, S10, S11) and floc[R][ne][2] may be NULL.
// work: p1_bubble_work_bytes(ne, R) bytes.  order in 2 .. 4, nquad in order+1 .. 5 (anything else: hipErrorInvalidValue
// / false).  The host form runs the same routines on host arrays, bit for bit.
struct P1BubbleArgs {
  const double* x;
  int64_t ne;
  int order, nquad, R;
  const double* rhs_quad;
  const double* a_quad;
  const double* c_quad;
  const double* b_quad;
  double* diag;
  double* sub;
  double* sup;
  double* load;
  double* kloc4;
  double* floc;
  double* work;
};
int64_t p1_bubble_work_bytes(int64_t ne, int R);
hipError_t p1_assemble_bubble(const P1BubbleArgs& a, hipStream_t s);
bool p1_assemble_bubble_host(const P1BubbleArgs& a);
// assembly + enhancement of the same mesh in ONE launch (lane-per-element path, in-kernel rhs); memo: the plan's
// memo of the mesh-only loop results (read and validated, never written; NULL: none)
hipError_t step_small(const EnhanceArgs& e, const P1Args& a, hipStream_t s,
                      const LaunchOpts* o = nullptr, const double* memo = nullptr);
// The step memo: step_memo_planes(M) = 3 (M-2) - 2 planes of step_memo_ne_pad(ne) doubles
// (mom[1..MR-1], P[1..MR-1], rv[0..MR-1] of enhance_small_body_cheb, plane[q * ne_pad + e]), then the key plane,
// the ne + 1 node coordinates they were computed from.  M = 2 has no loop: its memo is the key plane alone.
__host__ __device__ constexpr int step_memo_planes(int M) { return M > 2 ? 3 * (M - 2) - 2 : 0; }
__host__ __device__ constexpr int64_t step_memo_ne_pad(int64_t ne) { return (ne + 63) & ~(int64_t)63; }
constexpr int64_t step_memo_doubles(int M, int64_t ne) { return step_memo_planes(M) * step_memo_ne_pad(ne) + ne + 1; }
// one launch that fills `memo` from e.x (the enhancement half of step_small's grid, run to the end of the loop)
hipError_t step_small_memo_fill(const EnhanceArgs& e, double* memo, hipStream_t s);
constexpr int kStepVarcoefFusedMaxM = 12;   // lssvr_step_varcoef: one launch up to here, two above
hipError_t step_small_vc(const EnhanceArgs& e, const P1Args& a, hipStream_t s, const LaunchOpts* o = nullptr);
hipError_t quad_points(const double* x, int64_t ne, int nquad, double* xq, hipStream_t s);

// tridiag.hip: recursive substructuring, no pivoting (diagonally dominant rows).  One set of kernels for the
// symmetric bands (off) and the non-symmetric ones (sub, sup); only the second ends its base level with a step of
// iterative refinement.  nc right-hand sides load[nc][ne+1] on one set of bands -> u[nc][ne+1]; the end values of case
// q are bc[q][0], bc[q][1] of the device array bc[nc][2] or, with bc NULL, u0 and u1 for every case (by value: the
// single-RHS C entries are nc = 1 with bc NULL).  The bands are read and the pivots computed once per pass of
// kTriMultiCases cases; row q does not depend on nc, bit for bit.
constexpr int kTriMultiCases = 8;
int64_t tridiag_multi_work_bytes(int64_t ne, int nc);
int64_t tridiag_work_bytes(int64_t ne);       // tridiag_multi_work_bytes(ne, 1)
hipError_t tridiag_dirichlet_solve(const double* diag, const double* off, const double* load, int64_t ne, int nc,
                                   const double* bc, double u0, double u1, double* u, void* work, hipStream_t s);
hipError_t tridiag_ns_dirichlet_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                      int64_t ne, int nc, const double* bc, double u0, double u1, double* u,
                                      void* work, hipStream_t s);
// The same solves with free ends: f0 / f1 make node 0 / node ne an unknown whose row gets k0 /
// k1 on the diagonal and bc[q][0] / bc[q][1] on the right-hand side, inside the kernels (a Robin end a du/dn +
// kappa u = g); an end that is not free is a Dirichlet end with the value bc[q][.].  bc NULL: zeros.  The bands are
// read only.  tridiag_bc_work_bytes is sized for two free ends.
int64_t tridiag_bc_work_bytes(int64_t ne, int nc);
hipError_t tridiag_bc_solve(const double* diag, const double* off, const double* load, int64_t ne, int nc, bool f0,
                            bool f1, double k0, double k1, const double* bc, double* u, void* work, hipStream_t s);
hipError_t tridiag_ns_bc_solve(const double* diag, const double* sub, const double* sup, const double* load,
                               int64_t ne, int nc, bool f0, bool f1, double k0, double k1, const double* bc,
                               double* u, void* work, hipStream_t s);
// The same solves with periodic ends: node ne is node 0, the rows of node 0 and node ne add up
// to the seam row.  ne >= 2.  u[q][0] == u[q][ne], bit for bit; the bands and loads are read only; row q does not
// depend on nc.  work: tridiag_periodic_work_bytes(ne, nc) bytes.
int64_t tridiag_periodic_work_bytes(int64_t ne, int nc);
hipError_t tridiag_periodic_solve(const double* diag, const double* off, const double* load, int64_t ne, int nc,
                                  double* u, void* work, hipStream_t s);
hipError_t tridiag_ns_periodic_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                     int64_t ne, int nc, double* u, void* work, hipStream_t s);
// tridiag_pivot.hip: the solve with free ends above for tridiagonal matrices that need not be dominant -- a recursive partitioned
// solve with scaled partial pivoting at every level.  Same unknowns, end terms and passes as
// tridiag_ns_bc_solve; k0 / k1 of any sign; the symmetric caller passes off for sub and sup.  info (device, may be
// NULL): the number of pivots, over all levels, that were zero or not finite after the row choice -- 0 for a matrix
// that is non-singular to working precision.  Row q does not depend on nc, bit for bit.
int64_t tridiag_pivot_work_bytes(int64_t ne, int nc);
hipError_t tridiag_pivot_solve(const double* diag, const double* sub, const double* sup, const double* load,
                               int64_t ne, int nc, bool f0, bool f1, double k0, double k1, const double* bc,
                               double* u, int32_t* info, void* work, hipStream_t s);
// the same solve on host arrays, without a device, through the routines the kernels call (for tests without a GPU)
void tridiag_pivot_host(const double* diag, const double* sub, const double* sup, const double* load, int64_t ne,
                        int nc, bool f0, bool f1, double k0, double k1, const double* bc, double* u, int32_t* info);
// fem_eval.hip: the load of p1_assemble / _react / _conv for nc tabulated right-hand sides rhs_quad[nc][ne*nquad] ->
// load[nc][ne+1], no bands
hipError_t p1_load_multi(const double* x, int64_t ne, int nquad, const double* rhs_quad, int nc, double* load,
                         hipStream_t s);

int64_t flux_work_bytes(int64_t ne);
hipError_t flux_dirichlet_solve(const double* kloc, const double* load, int64_t ne, double u0,
                                double u1, double* u, void* work, hipStream_t s);

hipError_t eval_points(const double* x, const double* W, int64_t ne, int M, const double* xq,
                       int64_t P, double* uq, int64_t* elem, hipStream_t s);

hipError_t flux_aggregate(const double* kloc, const double* load, int64_t ne, bool first_global,
                          void* work, double* agg3, hipStream_t s);
hipError_t flux_finish(const double* kloc, const double* load, int64_t ne, bool first_global,
                       bool last_global, const void* work, const double* prefix3,
                       const double* grand3, double u0, double u1, double* u, hipStream_t s);

hipError_t eval_error(const double* x, const double* W, int64_t ne, int M, const double* xq,
                      int64_t P, double amp, double omega, double* out, hipStream_t s);

// a posteriori estimator and h-refinement (adapt.hip)
constexpr int kAdaptMaxNq = 32;     // Gauss points per element of lssvr_estimate
constexpr int kAdaptMaxM = 33;
struct GaussRuleN {                 // Gauss-Legendre on [-1, 1], by value in the kernel arguments
  double xi[kAdaptMaxNq];
  double wt[kAdaptMaxNq];
};
struct EstimateArgs {
  const double* x;
  const double* W;
  int64_t ne;
  int M, nq, ms;                    // ms: LDS row stride of the staged W rows (set by estimate())
  double rhs_amp, rhs_omega;
  const double* rhs_values;
  double* eta2;
  double* jump;
  double* work;
};
// variable coefficients: EstimateArgs with rhs_values = the f table, plus the a and a' tables at the same points
// (same layout) and a_ends[2*ne] = {a at the left end, a at the right end} of every element, seen from inside it
struct EstimateVcArgs : EstimateArgs {
  const double* a_values;
  const double* da_values;
  const double* a_ends;
};
// -(a u')' + c u = f: plus the c table at the same points, same layout
struct EstimateReactArgs : EstimateVcArgs {
  const double* c_values;
};
bool gauss_rule(int nq, double* xi, double* wt);       // host; false: nq outside [1, kAdaptMaxNq]
int64_t adapt_work_bytes(int64_t ne);
hipError_t eval_deriv(const double* x, const double* W, int64_t ne, int M, int order, const double* xq,
                      int64_t P, double* out, int64_t* elem, hipStream_t s);
hipError_t estimate_points(const double* x, int64_t ne, int nq, double* xq, hipStream_t s);
// rhs_mode: 0 = table element-major, 1 = amp*sin(omega x) in-kernel, 2 = table point-major
hipError_t estimate(EstimateArgs a, int rhs_mode, double* out3, hipStream_t s);
hipError_t estimate_varcoef(EstimateVcArgs a, bool point_major, double* out3, hipStream_t s);
hipError_t estimate_react(EstimateReactArgs a, bool point_major, double* out3, hipStream_t s);
// the boundary term of a Robin end, added to eta2 and out3 after any of the three estimators (adapt.hip)
struct EstimateEndsArgs {
  const double* x;
  const double* W;
  int64_t ne;
  int M;
  int kind[2];                      // 0 Dirichlet (nothing added), 1 Robin
  double kappa[2], g[2], a[2];      // per end; a = the coefficient a at x_0 and x_ne
  double* eta2;
  double* out3;
};
hipError_t estimate_ends(const EstimateEndsArgs& a, hipStream_t s);
// the flux jump across the seam of a periodic domain, added to eta2 and out3 in the same way (adapt.hip)
struct EstimateSeamArgs {
  const double* x;
  const double* W;
  int64_t ne;
  int M;
  double a[2];                      // a at x_ne seen from element ne-1, a at x_0 seen from element 0
  double* eta2;
  double* out3;
};
hipError_t estimate_seam(const EstimateSeamArgs& a, hipStream_t s);
hipError_t refine(const double* x, int64_t ne, const double* eta2, const double* eta2_max, double theta,
                  double h_min, void* work, double* x_new, int64_t* parent, int64_t* ne_new, hipStream_t s);

// goal-oriented estimator (adapt_goal.hip): the residual of Wu weighted with the dual solution Wz, both [ne, M]
struct GoalArgs {
  const double* x;
  const double* Wu;
  const double* Wz;
  int64_t ne;
  int M, nq, ms;                    // ms: LDS row stride of the staged rows (set by estimate_goal())
  const double* a_values;           // a, a', c (or nullptr), f and j at lssvr_estimate_points, one layout
  const double* da_values;
  const double* c_values;
  const double* rhs_values;
  const double* goal_values;
  const double* a_ends;             // [ne, 2], as EstimateVcArgs
  int kind[2];                      // per end of the domain, as EstimateEndsArgs: 0 Dirichlet, 1 Robin
  int jump_free;                    // 1: weight with z_e minus its linear interpolant at the element's nodes
  double kappa[2], g[2], a_bnd[2];
  double* eta;                      // [ne] signed
  double* eta2;                     // [ne] eta^2
  double* q;                        // [ne] int_e j u_e, or nullptr
  double* work;                     // goal_work_bytes(ne)
};
int64_t goal_work_bytes(int64_t ne);
// out4 = {sum of eta over the elements whose eta^2 is finite, max finite eta^2, non-finite count, sum of finite q_e}
hipError_t estimate_goal(GoalArgs a, bool point_major, double* out4, hipStream_t s);

// hp-adaptive refinement (adapt_hp.hip; refine_hp: adapt.hip, the kernels of refine)
hipError_t smoothness(const double* W, int ldw, const int32_t* deg, int64_t ne, double* sigma, hipStream_t s);
hipError_t refine_hp(const double* x, int64_t ne, const double* eta2, const double* eta2_max, double theta,
                     double h_min, const double* sigma, const int32_t* deg, double sigma_min, int dM, int M_max,
                     void* work, double* x_new, int32_t* deg_new, int64_t* parent, int64_t* ne_new, int64_t* counts2,
                     hipStream_t s);
int64_t group_work_bytes(int64_t ne);
hipError_t group_by_degree(const int32_t* deg, int64_t ne, int64_t* ids, int64_t* offsets, void* work,
                           hipStream_t s);

// eigen.hip: block inverse iteration for -(a u')' + c u = lambda rho u.  K = (kdiag, koff) and
// M = (mdiag, moff) are P1 bands, read only; f0 / f1 make node 0 / node ne an unknown whose K diagonal gets k0 / k1.
// Vectors are [nb][ne+1], nb <= 8; rows outside the unknowns are written as 0 and not read.
struct EigArgs {
  const double* kdiag;
  const double* koff;
  const double* mdiag;
  const double* moff;
  int64_t ne;
  int nb;
  bool f0, f1;
  double k0, k1;
};
int64_t eig_work_bytes(int64_t ne, int nb);
// MZ = M Z, KZ = K Z, gram = {A = Z^T K Z, B = Z^T M Z} (two full nb x nb matrices)
hipError_t eig_apply(const EigArgs& a, const double* Z, double* MZ, double* KZ, double* gram, void* work,
                     hipStream_t s);
// theta[nb] ascending in |theta - sigma|, Q[nb][nb] with Q^T A Q = diag theta, Q^T B Q = I; info: dependent columns
hipError_t eig_ritz_device(const double* A, const double* B, int nb, double sigma, double* theta, double* Q,
                           int32_t* info, hipStream_t s);
int eig_ritz_host(const double* A, const double* B, int nb, double sigma, double* theta, double* Q);
// X = Z Q, Y = (MZ) Q, each column signed; res2[2*nb] = {|(KZ) Q_j - theta_j (MZ) Q_j|^2, |X_j|^2}
hipError_t eig_rotate(const double* Z, const double* MZ, const double* KZ, const double* Q, const double* theta,
                      int64_t ne, int nb, bool f0, bool f1, double* X, double* Y, double* res2, void* work,
                      hipStream_t s);
// counts[t] = negative pivots of LDL^T (K - shifts[t] M), pivots below pivmin in size taken as -pivmin
hipError_t eig_count_device(const EigArgs& a, const double* shifts, int ns, double pivmin, int32_t* counts,
                            hipStream_t s);
void eig_count_host(const EigArgs& a, const double* shifts, int ns, double pivmin, int32_t* counts);
struct EigRayleighArgs {
  const double* x;
  const double* W;
  int64_t ne;
  int M, nq;
  const double* a_values;           // a, c and rho at lssvr_estimate_points, one layout
  const double* c_values;
  const double* rho_values;
  int kind[2];                      // per end of the domain: 0 Dirichlet, 1 Robin
  double kappa[2];
  void* work;                       // eig_work_bytes(ne, 1)
};
// out3 = {sum_e int (a u_e'^2 + c u_e^2) + sum_ends kappa u(x_end)^2, sum_e int rho u_e^2, sum |terms| of the first}
hipError_t eig_rayleigh(const EigRayleighArgs& a, bool point_major, double* out3, hipStream_t s);

// timestep.hip: BDF1 / BDF2 steps of rho u_t - (a u')' + c u = f.  Vectors are case-major
// [nc][ne+1]; the host forms (ts_*_host) run the same inline routines on host arrays, bit for bit.
struct TsRhsArgs {
  const double* mdiag;              // the mass bands of rho: [ne+1], [ne]
  const double* moff;
  const double* U0;                 // u^n [nc][ne+1]
  const double* U1;                 // u^{n-1} [nc][ne+1]; not read when beta1 == 0
  const double* loads;              // [R][ne+1], shared by the cases
  const double* phi;                // [nc][R]
  int64_t ne;
  int nc, R;
  double beta0, beta1, inv_dt;
};
// out[j][i] = inv_dt (M (beta0 U0[j] + beta1 U1[j]))_i + sum_r phi[j][r] loads[r][i]
hipError_t ts_rhs(const TsRhsArgs& a, double* out, hipStream_t s);
void ts_rhs_host(const TsRhsArgs& a, double* out);
struct TsSourceArgs {
  const double* U2;                 // u^{n+1}, u^n, u^{n-1} [ne+1]; U1 not read when beta1 == 0
  const double* U0;
  const double* U1;
  const double* ftab;               // [R] tables of ne * n_colloc, one layout
  const double* rho_tab;
  const double* phi;                // [R]
  int64_t ne;
  int n_colloc, R;
  double alpha, beta0, beta1, inv_dt;
};
// out(e, k) = sum_r phi[r] ftab[r](e, k) - rho_tab(e, k) (w_e + (w_{e+1} - w_e) k / (n_colloc - 1))
hipError_t ts_source_table(const TsSourceArgs& a, bool point_major, double* out, hipStream_t s);
void ts_source_table_host(const TsSourceArgs& a, bool point_major, double* out);

// timestep_adapt.hip: what an attempt of variable-step BDF2 with error control adds to the above (DESIGN.md section
// 30).  One case; the host forms run the same inline routines on host arrays, bit for bit.
struct TsStepArgs {
  TsRhsArgs rhs;                    // nc = 1; inv_dt = 1 / h of the attempt
  const double* kdiag;              // the bands of -(a u')' + c u: [ne+1], [ne]
  const double* koff;
  double s;                         // alpha / h
  int write_bands;                  // 0: s is the previous attempt's, adiag and aoff are left as they are
  double* adiag;                    // K + s M: [ne+1], [ne]
  double* aoff;
};
// adiag = kdiag + s mdiag, aoff = koff + s moff (with write_bands), b = the row of ts_rhs
hipError_t ts_step(const TsStepArgs& a, double* b, hipStream_t s);
void ts_step_host(const TsStepArgs& a, double* b);
struct TsErrArgs {
  const double* U3;                 // the trial u^{n+1}, then u^n, u^{n-1}, u^{n-2} [ne+1]; U1 / U0 not read when
  const double* U2;                 // w1 / w0 == 0
  const double* U1;
  const double* U0;
  int64_t ne;
  int kind[2];                      // per end of the domain: 0 Dirichlet (row skipped), 1 Robin
  double w3, w2, w1, w0;            // the weights of the divided difference, its scalar factor folded in
  double atol, rtol;
};
int64_t ts_error_work_bytes(int64_t ne);
// out4 = {max |e| / sc, max |e|, max |U3|, count of rows whose e or sc is not finite}
hipError_t ts_error(const TsErrArgs& a, double* out4, void* work, hipStream_t s);
void ts_error_host(const TsErrArgs& a, double* out4);

// nonlinear.hip: the Newton iteration of -(a u')' + b u' + c u + g(x, u) = f.  The host forms
// (nl_*_host) run the same inline routines on host arrays, bit for bit except for exp (libm there).
struct NlLinArgs {
  const double* u;                  // nodal iterate [ne+1]
  const double* t_local;            // [n] local coordinates in [0, 1] of the n points of every element
  const double* q_tabs;             // [nterm] tables of ne * n, one layout; EXP: q_0, q_1
  const double* c_tab;              // nullptr: c = 0
  const double* f_tab;
  int64_t ne;
  int n, kind, nterm;
  double* c_eff;                    // c + g_u                    (each output: nullptr = not written)
  double* f_eff;                    // (f - g) + g_u u_h
  double* f_res;                    // f - g
};
hipError_t nl_linearize(const NlLinArgs& a, bool point_major, hipStream_t s);
void nl_linearize_host(const NlLinArgs& a, bool point_major);
struct NlResArgs {
  const double* diag;               // the bands of the LINEAR operator: [ne+1], [ne], [ne]; symmetric: sub == sup
  const double* sub;
  const double* sup;
  const double* load;               // F - G(u) [ne+1]
  const double* u;                  // the iterate and the candidate [ne+1]
  const double* u_new;
  const double* end_values;         // [2]: g of a Robin end; not read at a Dirichlet end
  int64_t ne;
  int kind[2];                      // per end of the domain: 0 Dirichlet, 1 Robin
  double kappa[2];
};
int64_t nl_residual_work_bytes(int64_t ne);
// out4 = {max |r|, max |u_new - u|, max |u_new|, count of non-finite entries met}
hipError_t nl_residual(const NlResArgs& a, double* out4, void* work, hipStream_t s);
void nl_residual_host(const NlResArgs& a, double* out4);
// out = u + lambda (u_new - u) [ne+1]
hipError_t nl_step(const double* u, const double* u_new, double lambda, int64_t ne, double* out, hipStream_t s);
void nl_step_host(const double* u, const double* u_new, double lambda, int64_t ne, double* out);

// timestep_nl.hip: the Newton matrix and right-hand side of one iteration of a semilinear time step (DESIGN.md
// section 28).  All tables are [ne][nquad], element-major, at quad_points.
struct TsNlArgs {
  const double* x;                  // nodes [ne+1]
  const double* u;                  // the Newton iterate v_k [ne+1]
  const double* a_quad;             // nullptr: a = 1
  const double* cs_quad;            // c + alpha rho / dt
  const double* q_quad;             // [nterm] tables; EXP: q_0, q_1
  const double* r;                  // the step's vector of ts_rhs [ne+1]
  int64_t ne;
  int nquad, kind, nterm;
  double* diag;                     // [ne+1], [ne], [ne+1]
  double* off;
  double* rhs;
};
hipError_t ts_nl_assemble(const TsNlArgs& a, hipStream_t s);
bool ts_nl_assemble_host(const TsNlArgs& a);      // false: no rule of a.nquad points

// timestep_nl_adjoint.hip: the backward step of the semilinear BDF loop.  ONE launch per level
// n writes the bands of the Jacobian J_n = K + M(cs + g_u(., u^n_h)), the adjoint right-hand side B_n and the end
// entries of J_n.  `nl` is read as by ts_nl_assemble with u = u^n (nl.r and nl.rhs are not used); `rhs` as by ts_rhs
// with nc = 1: U0 = lambda^{n+1}, U1 = lambda^{n+2}, loads [R][ne+1] and phi [R] the rows p_n with their weights.
struct TsNlAdjArgs {
  TsNlArgs nl;
  TsRhsArgs rhs;
  double* B;                        // [ne+1]: the row of ts_rhs
  double* band_ends;                // [2] = {off[0], off[ne-1]}: the chunk's row of this level
};
hipError_t ts_nl_adjoint_step(const TsNlAdjArgs& a, hipStream_t s);
bool ts_nl_adjoint_step_host(const TsNlAdjArgs& a);      // false: no rule of a.nl.nquad points

// wave.hip: Newmark steps of rho u_tt + d u_t - (a u')' + c u = f.  Vectors are case-major
// [nc][ne+1]; the host form runs the same inline routines on host arrays, bit for bit.
struct WaveArgs {
  const double* U_new;              // the solve's result [nc][ne+1]; nullptr: (U, V, Acc) is the state already
  const double* U;                  // [nc][ne+1] each
  const double* V;
  const double* Acc;
  const double* mdiag;              // the mass bands of rho: [ne+1], [ne]
  const double* moff;
  const double* ddiag;              // the mass bands of d; ddiag == nullptr: d = 0, neither is read
  const double* doff;
  const double* loads;              // [R][ne+1], shared by the cases; read with rhs_out only, like phi [nc][R]
  const double* phi;
  int64_t ne;
  int nc, R;
  double dt, c_u2, c_v1, c_m, c_d, c_va;      // set by wave_coefficients
};
// the scalars of the kernel from (dt, beta, gamma), once, on the host, for the device and the host form alike
void wave_coefficients(WaveArgs& a, double dt, double beta, double gamma);
// V_out, Acc_out (written when a.U_new is given) and rhs_out (written unless nullptr), each [nc][ne+1]
hipError_t wave_advance(const WaveArgs& a, double* V_out, double* Acc_out, double* rhs_out, hipStream_t s);
void wave_advance_host(const WaveArgs& a, double* V_out, double* Acc_out, double* rhs_out);

// sensitivity.hip: adjoint sensitivities of the P1 solve.  From nc pairs (U[j], Z[j]) of a primal
// and an adjoint nodal solution, case-major [nc][ne+1] (U [1][ne+1] with nu == 1: one primal for all cases), the
// gradients of J with respect to the tables a_quad, b_quad, c_quad, rhs_quad, each [nc][ne*nquad] in the tables' own
// layout, and with respect to the end data.  The tables themselves are not arguments: given u and z the gradient does
// not depend on them.  A nullptr output is skipped, stores included.
struct SensArgs {
  const double* x;                  // nodes [ne+1]
  const double* U;                  // [nu][ne+1]
  const double* Z;                  // [nc][ne+1]
  const double* P;                  // dJ/du [nc][ne+1], read for out_ends at a Dirichlet end; nullptr: zero
  const double* band_ends;          // the raw sub[0] and sup[ne-1]; read for out_ends only
  int64_t ne;
  int nquad, nu, nc;
  int kind[2];                      // LSSVR_END_*; read for out_ends only
  double* ga;                       // dJ/da_quad, dJ/db_quad, dJ/dc_quad, dJ/drhs_quad
  double* gb;
  double* gc;
  double* gf;
  double* out_ends;                 // [nc][4] = dJ/dg_0, dJ/dg_ne, dJ/dkappa_0, dJ/dkappa_ne; nullptr: not wanted
};
hipError_t p1_sensitivity(const SensArgs& a, hipStream_t s);
bool p1_sensitivity_host(const SensArgs& a);     // false: no such quadrature rule

// nl_sensitivity.hip: adjoint sensitivities of the semilinear P1 solve.  `s` holds everything of
// p1_sensitivity, with U the converged u* and Z the adjoint of the Newton Jacobian (all four of its tables may be nullptr
// here); gq [nc][nterm][ne*nquad] receives dJ/dq_k for the tables of g(x, u), nullptr: skipped, stores included; q_tabs
// [nterm][ne*nquad] is read for LSSVR_NL_EXP only.
struct NlSensArgs {
  SensArgs s;
  const double* q_tabs;
  int kind, nterm;                  // LSSVR_NL_*; POLY 1 <= nterm <= 6, EXP nterm == 2
  double* gq;
};
hipError_t nl_sensitivity(const NlSensArgs& a, hipStream_t s);
bool nl_sensitivity_host(const NlSensArgs& a);   // false: no such quadrature rule

// newmark_adjoint.hip: the adjoint advance of the Newmark loop.  One case; nodal vectors
// [ne+1].  The scalars are those of wave_coefficients.
struct NmAdjArgs {
  const double* lam;                // lambda^{n+1}; nullptr: the first call of a sweep, B_out from (P, Vbar, Abar) alone
  const double* Vbar;               // the bars (vbar, abar) of level n+1
  const double* Abar;
  const double* P;                  // the row p_n; nullptr: zero
  const double* mdiag;              // the mass bands of rho: [ne+1], [ne]; read with lam
  const double* moff;
  const double* ddiag;              // the mass bands of d; ddiag == nullptr: d = 0, neither is read
  const double* doff;
  int64_t ne;
  double dt, c_u2, c_v1, c_m, c_d, c_va;
  double* V_out;                    // the bars (vbar, abar) of level n; written with lam
  double* A_out;
  double* U_out;                    // ubar of level n; nullptr: not written
  double* B_out;                    // B_n = ubar + c_m (abar + c_va vbar); nullptr: not written
};
hipError_t newmark_adjoint_advance(const NmAdjArgs& a, hipStream_t s);
void newmark_adjoint_advance_host(const NmAdjArgs& a);

// chunk_sens.hip: the chunk pass of the adjoint sensitivities of the BDF loop and of the Newmark
// loop (section 34).  One chunk of m <= 8 consecutive levels n0 .. n0+m-1 of the backward sweep, summed over the chunk
// into the tables.  Every array that runs over time is handed over whole and indexed with the level n: the
// trajectories, phi, out_g.  The rows of Z and Brows (and what a scheme adds per step row) stand in the order of the
// sweep: row i belongs to level n0 + m - 1 - i.
constexpr int kChunkSensMaxSteps = 8;   // levels per chunk
constexpr int kChunkSensMaxTerms = 8;   // terms of the separable forcing (TS_MAX_TERMS of the forward loops)
struct ChunkSensArgs {
  const double* x;                  // nodes [ne+1]
  const double* Utraj;              // the forward trajectory [N+1][ne+1]: row n = u^n
  const double* Z;                  // [m][ne+1]: the adjoint states of the chunk
  const double* Brows;              // [m][ne+1]: their right-hand sides; read for out_g at a Dirichlet end
  const double* phi;                // [.][R]: the scheme says which row is phi(t_n); gf only
  const double* band_ends;          // rows {sub[0], sup[ne-1]} of the chunk's matrices; read for out_g only
  int64_t ne, n0;
  int nquad, m, R, accumulate;      // accumulate: the sums continue from what the outputs hold (0: from 0)
  int kind[2];                      // LSSVR_END_*; read for out_g only
  double* ga;                       // dJ/da_quad, dJ/dc_quad, dJ/drho_quad [ne*nquad]; nullptr: skipped
  double* gc;
  double* grho;
  double* gf;                       // dJ/df_quad [R][ne*nquad]
  double* out_g;                    // [N+1][2]: rows n0 .. n0+m-1 are written; nullptr: no end gradients
  double* out_kappa;                // [2]
};
// BDF (n0 >= 1): rows n0-2 .. n0+m-1 of Utraj are read; phi [N][R], row n-1 = phi(t_n), the table the forward loop feeds
// ts_rhs from; band_ends [2][2], two step matrices
struct TsSensArgs : ChunkSensArgs {
  int band_row[kChunkSensMaxSteps];    // which row of band_ends is step row i's matrix
  double inv_dt;
  double coef[kChunkSensMaxSteps][3];  // (alpha, beta0, beta1) of step row i
};
// Newmark (n0 >= 0): Utraj is read for ga, gc and out_kappa; phi [N+1][R], row n = phi(t_n); band_ends [2], one matrix
struct NmSensArgs : ChunkSensArgs {
  const double* Vtraj;              // [N+1][ne+1]: row n = v^n; read for gd only
  const double* Atraj;              // row n = acc^n; read for grho only
  double* gd;                       // dJ/dd_quad [ne*nquad]; nullptr: skipped
};
// semilinear BDF (section 36): the BDF scheme, with one matrix per level -- band_ends [m][2], band_row[i] = i -- and the
// tables of g(x, u): gq [nterm][ne*nquad] receives dJ/dq_k summed over the chunk (nullptr: skipped); q_tabs
// [nterm][ne*nquad] is read for LSSVR_NL_EXP only
struct TsNlSensArgs : TsSensArgs {
  const double* q_tabs;
  int law, nterm;                   // LSSVR_NL_*; POLY 1 <= nterm <= 6, EXP nterm == 2
  double* gq;
};
// Args: TsSensArgs, NmSensArgs or TsNlSensArgs
template <class Args> hipError_t chunk_sensitivity(const Args& a, hipStream_t s);
template <class Args> bool chunk_sensitivity_host(const Args& a);   // false: no such quadrature rule

// enhance_adjoint.hip: the adjoint of the element solve.  From W and Wbar = dJ/dW, per element one
// more solve with the forward matrix and a second sweep over the points: the pair (dJ/dg_l, dJ/dg_r) of every element
// into `pairs`, the table gradients (element-major, a nullptr one is skipped, stores included), then gu and gbc from the
// pairs in a fixed order.  Degrees kEnhAdjMinM .. kEnhAdjMaxM, the range of the reaction lane kernel.
constexpr int kEnhAdjMinM = 3;
constexpr int kEnhAdjMaxM = kReactSmallMaxM;
constexpr int kEnhAdjMaxColloc = 64;
struct EnhAdjArgs {
  const double* x;                  // nodes [ne+1]
  int64_t ne, elem_offset, ne_global;
  double gxmin, gxmax, gamma;
  int M, n;
  const double* a_values;           // [ne*n] element-major; nullptr: a = 1 (then da_values is nullptr too)
  const double* da_values;          // nullptr: 0
  const double* c_values;           // nullptr: 0
  const double* rhs_values;
  const double* W;                  // [ne*M], the forward call's output
  const int32_t* status;            // the forward call's; nullptr: no fallback element
  const double* Wbar;               // [ne*M]
  double* gu;                       // [ne+1]
  double* gbc;                      // [2]
  double* ga;                       // [ne*n] each
  double* gda;
  double* gc;
  double* gf;
  double* pairs;                    // workspace [ne][2]
};
hipError_t enhance_adjoint(const EnhAdjArgs& a, hipStream_t s);
bool enhance_adjoint_host(const EnhAdjArgs& a);  // false: no such degree

hipError_t fp64_probe(double* out, int blocks, int iters, int use_mfma, hipStream_t s);
hipError_t stream_probe(const double* src, double* dst, int64_t n, hipStream_t s);
hipError_t row_chunk_probe(const double* src, double* dst, int64_t nrows, int rowlen, int chunk, hipStream_t s);

}  // namespace lssvr
