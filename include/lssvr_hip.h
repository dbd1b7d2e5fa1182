/*
 * lssvr_hip.h -- C ABI of the MI355X (gfx950) per-element LSSVR enhancement path.
 *
 * The reference (maryambabaei/hybrid-FEM-LSSVR) is pure Python and has no FFI; the
 * "reference interface" each entry point replaces is therefore a Python call
 * site in /root/reference/1D-Possion/Hybrid-FEM-LSSVR-Dual.py ("Dual.py").  The
 * ctypes binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in _host;
 *   - the caller owns every buffer; the library allocates nothing and keeps no
 *     state besides a thread-local last-error string;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream) and is safe to capture in a hipGraph;
 *   - return value: 0 = launched, <0 = argument error (see lssvr_last_error());
 *   - all floating point is IEEE binary64; element/node indices are int64.
 *   - element e of a mesh shard has end points x[e], x[e+1] and nodal values
 *     u[e], u[e+1] (Dual.py:143-147: element i <-> nodes (i, i+1)).
 */
#ifndef LSSVR_HIP_H
#define LSSVR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSSVR_ABI_VERSION 7

/* error codes */
#define LSSVR_OK              0
#define LSSVR_ERR_NULL      (-1)  /* a required pointer is NULL                   */
#define LSSVR_ERR_SIZE      (-2)  /* ne / P / n_colloc out of range               */
#define LSSVR_ERR_DEGREE    (-3)  /* M outside the supported range                */
#define LSSVR_ERR_RHS       (-4)  /* unknown rhs_id or missing rhs data           */
#define LSSVR_ERR_SOLVER    (-5)  /* unknown solver_id                            */
#define LSSVR_ERR_LAUNCH    (-6)  /* hipLaunch / runtime error                    */
#define LSSVR_ERR_QUAD      (-7)  /* unsupported quadrature order                 */

/* right-hand side f(x) of -u'' = f (Dual.py:11-12 `poisson_rhs`, passed as the
 * callable `rhs_func` at Dual.py:20,157).  A Python callable cannot cross the
 * ABI, so f is either tabulated by the host facade or named: */
#define LSSVR_RHS_ARRAY  0  /* rhs_values[e*n_colloc + k] = f(x_k of element e)   */
#define LSSVR_RHS_SIN    1  /* f(x) = p[0] * sin(p[1] * x), rounded like numpy's
                               `amp * np.sin(omega * x)`; Poisson: p = {pi^2, pi} */
#define LSSVR_RHS_ARRAY_PM 2 /* the same table POINT-major: rhs_values[k*ne + e] (ne = the launch's
                               element count; lssvr_enhance_subset: nsub, e = position in elem_ids).
                               The layout the lane-per-element kernels (M <= 22) read at full
                               HBM rate -- consecutive lanes = consecutive elements, no staging;
                               element-major rows reach them as 64-byte half-line requests, which
                               the memory system serves at ~3.3 TB/s.  ABI 4 */

/* layout of the tabulated arrays of lssvr_enhance_varcoef_ws (a_values, da_values, rhs_values) */
#define LSSVR_TABLE_ELEMENT_MAJOR 0  /* t[e*n_colloc + k]: what lssvr_colloc_points produces       */
#define LSSVR_TABLE_POINT_MAJOR   1  /* t[k*ne + e]: see LSSVR_RHS_ARRAY_PM                         */

/* per-element solver */
#define LSSVR_SOLVER_PRIMAL 0 /* BC-eliminated primal normal equations, (M-2) SPD, LDL^T
                                 (default; <=1e-15 of the exact minimiser on every BASELINE
                                 config).  When n_colloc < M-2 the primal Gram is rank
                                 deficient and the call is routed to LSSVR_SOLVER_DUAL (its
                                 limits then apply)                                      */
#define LSSVR_SOLVER_DUAL   1 /* north_star's dual Gram form (K + I/gamma) alpha = y: kernel
                                 Gram matrix of the collocation rows (boundary rows eliminated
                                 as a 2x2 block pivot), Jacobi-equilibrated, LU with partial
                                 pivoting, up to 3 safeguarded steps of iterative refinement
                                 (operator-form residual in compensated arithmetic).  n_colloc <= 64,
                                 M <= 33, Poisson and variable-coefficient rows.  Measured against the
                                 exact minimiser: <= 1e-12 on BASELINE configs 1-3, <= 5e-11 at degree
                                 32 / 64 points (config 4), 1e-8 where n_colloc ~ M .. M+6 (DESIGN.md
                                 section 3.2b).  FP64 vector FMAs only, no MFMA; 40x slower than
                                 LSSVR_SOLVER_PRIMAL: the cross-check solver                      */
#define LSSVR_SOLVER_PRIMAL_MOMENT 3 /* same algorithm as PRIMAL as the kernel sequence of
                                 csrc/enhance_large_cheb.hip (Chebyshev-moment Gram, four systems
                                 per wave in the LDL^T) for ANY M, Poisson rows -- what PRIMAL
                                 itself runs above M = 22 with a workspace; for A/B
                                 measurements below.  lssvr_enhance_ws only: it needs the
                                 workspace of lssvr_enhance_work_bytes() (LSSVR_ERR_SOLVER
                                 without one) */
#define LSSVR_SOLVER_PRIMAL_WAVE 2 /* same algorithm as PRIMAL, forced onto the
                                 wave-per-element / f64-MFMA Gram mapping whatever M is
                                 (PRIMAL picks lane-per-element for M <= 22); for A/B
                                 measurements of the two mappings */

/* per-element status written to status[e] */
#define LSSVR_ST_OK        0
#define LSSVR_ST_FALLBACK  1  /* factorisation broke down / non-finite: the element got
                                 the linear interpolant of (g_l, g_r) -- Dual.py:164-169 */

/* ABI version, == LSSVR_ABI_VERSION of the header the library was built from. */
int lssvr_version(void);

/* Message for the last <0 return on this thread ("" if none). */
const char* lssvr_last_error(void);

/*
 * lssvr_enhance -- the hot path.  Replaces the serial loop
 * `solve_lssvr_subproblems` (Dual.py:139-169) and every `lssvr_primal` call in it
 * (Dual.py:20-98): one independent QP per element, solved in closed form.
 *
 *   x[ne+1], u[ne+1]  node coordinates / FEM nodal values of this shard
 *                     (Dual.py:144-147; fem_nodes / fem_values, Dual.py:134-135)
 *   ne                elements in this shard (>= 0; 0 is a no-op)
 *   elem_offset       global index of the shard's first element, ne_global = total
 *                     elements: element is_left/is_right_boundary iff its global
 *                     index is 0 / ne_global-1 (Dual.py:150-151)
 *   gxmin, gxmax      global_domain (Dual.py:101,161); the Dirichlet value bc_left /
 *                     bc_right replaces u on a boundary element only if its end
 *                     point == gxmin / gxmax exactly (Dual.py:65,72)
 *   M                 number of Legendre coefficients (`lssvr_M`, Dual.py:47), 2..33
 *   n_colloc          collocation points per element, end points included, >= 2
 *                     (hard-coded 12 at Dual.py:40)
 *   gamma             `lssvr_gamma` (Dual.py:49)
 *   rhs_id/rhs_params/rhs_values   see LSSVR_RHS_* (rhs_params is a HOST pointer)
 *   W[ne*M]           out: row e = Legendre coefficients of element e on domain
 *                     [x[e], x[e+1]], window [-1,1] (`Legendre(res.x[:M], domain)`,
 *                     Dual.py:95)
 *   status[ne]        out (may be NULL): LSSVR_ST_*
 *   fail_count        in/out (may be NULL): device int32, incremented once per
 *                     fallback element (the reference prints per element instead,
 *                     Dual.py:165)
 */
int lssvr_enhance(const double* x, const double* u, int64_t ne,
                  int64_t elem_offset, int64_t ne_global,
                  double gxmin, double gxmax, double bc_left, double bc_right,
                  int M, int n_colloc, double gamma,
                  int rhs_id, const double* rhs_params_host, const double* rhs_values,
                  int solver_id,
                  double* W, int32_t* status, int32_t* fail_count, void* stream);

/*
 * lssvr_enhance_ws -- lssvr_enhance with a caller-provided device workspace (the library still
 * allocates nothing).  Poisson rows above M = 22 then run as TWO kernels -- Chebyshev moments of
 * the collocation points (96 doubles per element into `work`), then the four-systems-per-wave
 * solve -- twice the speed of the single f64-MFMA kernel lssvr_enhance launches without a
 * workspace.  Where n_colloc - (M-2) <= 14 (about as many equispaced
 * points as bubble coefficients: normal equations lose up to ten digits) the pair is followed by
 * 1-3 refinement steps with the residual taken through the collocation rows (32 more doubles per
 * element; 5e-14 instead of 1e-6 at M = 33, n_colloc = 31 -- DESIGN.md section 2).  Every other
 * case behaves exactly like lssvr_enhance.
 *   lssvr_enhance_work_bytes(ne, M, n_colloc, solver_id)   bytes `work` must hold (0: none needed)
 *   work / work_bytes      device scratch, contents undefined afterwards.  NULL: the workspace-free
 *                          kernels run (above M = 22 the single f64-MFMA kernel: about half the
 *                          speed, no near-square refinement).  Non-NULL but smaller than
 *                          lssvr_enhance_work_bytes(): LSSVR_ERR_SIZE (ABI 4; ABI 3 fell back
 *                          silently)
 *   kernel_ms_host != NULL BLOCKING measurement aid like lssvr_enhance_profiled: the duration of
 *                          the launch (of the PAIR of kernels, gap included, on the split path)
 */
int64_t lssvr_enhance_work_bytes(int64_t ne, int M, int n_colloc, int solver_id);
int lssvr_enhance_ws(const double* x, const double* u, int64_t ne,
                     int64_t elem_offset, int64_t ne_global,
                     double gxmin, double gxmax, double bc_left, double bc_right,
                     int M, int n_colloc, double gamma,
                     int rhs_id, const double* rhs_params_host, const double* rhs_values,
                     int solver_id,
                     double* W, int32_t* status, int32_t* fail_count,
                     void* work, int64_t work_bytes, void* stream, float* kernel_ms_host);

/*
 * lssvr_step -- one whole step of the hot path on one mesh shard in ONE launch:
 * lssvr_p1_assemble (in-kernel rhs, nquad-point Gauss) + lssvr_enhance (primal
 * solver, in-kernel rhs).  For M <= 22 the two run as disjoint block ranges of a single
 * grid; arguments as in the two separate calls.  PRIMAL SOLVER ONLY: n_colloc < M-2 (rank-
 * deficient primal normal equations) returns LSSVR_ERR_SOLVER -- use lssvr_p1_assemble +
 * lssvr_enhance, which routes that regime to the dual solver.
 */
int lssvr_step(const double* x, const double* u, int64_t ne,
               int64_t elem_offset, int64_t ne_global,
               double gxmin, double gxmax, double bc_left, double bc_right,
               int M, int n_colloc, double gamma, const double* rhs_params_host, int nquad,
               double* diag, double* off, double* load,
               double* W, int32_t* status, int32_t* fail_count, void* stream);

/*
 * lssvr_step_plan_* -- lssvr_step bound once, launched many times.  A time-stepping caller issues the
 * same step on the same resident buffers over and over (the reference's loop, Dual.py:139-169, re-run
 * after every FEM solve); validating and marshalling 21 arguments per call costs a host more than the
 * 3 us the launch itself does, and at 7-8 us per step that is what decides whether a stream stays fed.
 *   create : the arguments of lssvr_step (without the stream), checked exactly as lssvr_step checks
 *            them; *plan receives an opaque handle (a small HOST allocation: no device memory, no
 *            HIP call).  The buffers are referenced, not copied: their CONTENTS may change between
 *            launches, their addresses and sizes may not.
 *   launch : what lssvr_step would enqueue, on `stream`; asynchronous.  A plan may be launched on any
 *            stream, and concurrently from several threads (it is read-only after create).
 *   destroy: frees the handle (NULL is allowed); launches already enqueued are not affected.
 */
typedef struct lssvr_step_plan lssvr_step_plan;
int lssvr_step_plan_create(lssvr_step_plan** plan, const double* x, const double* u, int64_t ne,
                           int64_t elem_offset, int64_t ne_global,
                           double gxmin, double gxmax, double bc_left, double bc_right,
                           int M, int n_colloc, double gamma, const double* rhs_params_host, int nquad,
                           double* diag, double* off, double* load,
                           double* W, int32_t* status, int32_t* fail_count);
int lssvr_step_plan_launch(const lssvr_step_plan* plan, void* stream);
int lssvr_step_plan_destroy(lssvr_step_plan* plan);

/*
 * The step memo -- ADDITIVE to ABI 7 (two new symbols; no existing entry, struct or constant changes,
 * LSSVR_ABI_VERSION stays 7).  Between the launches of a plan u changes and the mesh x usually does not, and
 * half of the fused step's work -- the collocation loop -- depends on x, n_colloc and rhs_params only.  A memo
 * keeps the loop's results per element (3 (M-2) - 2 doubles: the Chebyshev power sums, the upper-moment
 * products and the right-hand-side sums) in CALLER-OWNED device memory; a launch with a memo bound reads them
 * instead of running the loop.
 *   memo_bytes : pure host arithmetic.  The bytes a memo of this plan needs,
 *                  8 * ((3 (M-2) - 2) * ne_pad + ne + 1),  ne_pad = ne rounded up to a multiple of 64
 *                (3 (M-2) - 2 planes of ne_pad doubles, plane[q * ne_pad + e], then the key plane: a copy of
 *                the ne + 1 node coordinates the planes were computed from; M = 2 has no loop and no planes),
 *                or 0 where the plan cannot use one: M > 22, the near-square regime that runs refinement steps
 *                (lssvr_step then issues two launches), or a NULL plan.
 *   memo_bind  : checks the buffer (memo_bytes below lssvr_step_plan_memo_bytes or a pointer that is not 8-byte
 *                aligned: LSSVR_ERR_SIZE; a plan whose memo_bytes is 0: LSSVR_ERR_SOLVER; NULL plan:
 *                LSSVR_ERR_NULL -- all before any HIP call), enqueues ONE fill launch on `stream` (it reads x as
 *                it is when that launch runs) and records the pointer in the plan.  memo == NULL unbinds (no
 *                launch).  Call it again after moving the mesh to refresh the memo.  Launches of the plan must be
 *                ordered after the fill (same stream, or an event).
 * VALIDATION: every launch compares each element's live (x[e], x[e+1]) with the memo's key plane, bit for bit;
 * a wave with any element that differs runs the loop on the live x, exactly as without a memo.  W, status and
 * the bands are therefore bit-identical with and without a memo, for any contents of x -- a stale memo costs
 * time, never correctness -- PROVIDED the memo's contents are what a fill launch of this plan wrote: the caller
 * must not write the buffer, nor share it between plans with different (ne, M, n_colloc, rhs_params).
 * A step launch never writes the memo.  Binding is set-up: it modifies the plan and is NOT thread-safe against
 * concurrent launches or other binds of the same plan; after it returns the plan is read-only again and may be
 * launched on any stream and from several threads.  destroy does not free the memo.
 */
int64_t lssvr_step_plan_memo_bytes(const lssvr_step_plan* plan);
int lssvr_step_plan_memo_bind(lssvr_step_plan* plan, void* memo, int64_t memo_bytes, void* stream);

/*
 * lssvr_enhance_varcoef -- BASELINE config 5, -(a u')' = f (no reference
 * counterpart: Dual.py:44,119 hard-code -u'').  PDE row k of element e is
 *   -a_k (2/h)^2 L_p''(t_k) - da_k (2/h) L_p'(t_k),
 * with a_values/da_values/rhs_values tabulated at the collocation points
 * ([ne*n_colloc], row-major per element).  Other arguments as lssvr_enhance.
 * n_colloc < M-2 is routed to the dual solver (n_colloc <= 64), like lssvr_enhance.
 * Convection: da_values is read only as the coefficient of the first-derivative row, and
 * -(a u')' + b u' = -a u'' - (a' - b) u', so a table holding a' - b (one subtraction per
 * point) gives the rows of -(a u')' + b u' = f; see "Convection term" at the end.
 */
int lssvr_enhance_varcoef(const double* x, const double* u, int64_t ne,
                          int64_t elem_offset, int64_t ne_global,
                          double gxmin, double gxmax, double bc_left, double bc_right,
                          int M, int n_colloc, double gamma,
                          const double* a_values, const double* da_values,
                          const double* rhs_values,
                          double* W, int32_t* status, int32_t* fail_count, void* stream);

/*
 * lssvr_enhance_varcoef_ws -- lssvr_enhance_varcoef with a caller workspace and the measurement aid
 * of lssvr_enhance_ws (ABI 4).  lssvr_enhance_varcoef_work_bytes(ne, M, n_colloc) bytes (0: none
 * needed); work == NULL runs the workspace-free kernels; too small: LSSVR_ERR_SIZE.
 * table_layout: LSSVR_TABLE_* of a_values / da_values / rhs_values (all three alike).
 * kernel_ms_host != NULL: BLOCKING, the duration of the launch (bench.py's roofline).
 */
int64_t lssvr_enhance_varcoef_work_bytes(int64_t ne, int M, int n_colloc);
int lssvr_enhance_varcoef_ws(const double* x, const double* u, int64_t ne,
                             int64_t elem_offset, int64_t ne_global,
                             double gxmin, double gxmax, double bc_left, double bc_right,
                             int M, int n_colloc, double gamma,
                             const double* a_values, const double* da_values,
                             const double* rhs_values, int table_layout,
                             double* W, int32_t* status, int32_t* fail_count,
                             void* work, int64_t work_bytes, void* stream, float* kernel_ms_host);

/*
 * lssvr_step_varcoef -- one whole step of BASELINE config 5 on one mesh shard: the a-weighted P1
 * assembly (lssvr_p1_assemble with LSSVR_RHS_ARRAY tables rhs_quad / a_quad at the nquad Gauss points,
 * lssvr_quad_points) + lssvr_enhance_varcoef (a_values / da_values / rhs_values at the collocation
 * points, table_layout = LSSVR_TABLE_*), as disjoint block ranges of ONE grid for M <= 12 (two
 * launches above).  Primal solver only (n_colloc >= M-2).  Arguments as in the two calls.  ABI 4.
 */
int lssvr_step_varcoef(const double* x, const double* u, int64_t ne,
                       int64_t elem_offset, int64_t ne_global,
                       double gxmin, double gxmax, double bc_left, double bc_right,
                       int M, int n_colloc, double gamma,
                       const double* a_values, const double* da_values, const double* rhs_values,
                       int table_layout, int nquad, const double* rhs_quad, const double* a_quad,
                       double* diag, double* off, double* load,
                       double* W, int32_t* status, int32_t* fail_count, void* stream);

/*
 * lssvr_enhance_subset -- heterogeneous meshes (per-element gamma, degree and
 * collocation count; the reference has one lssvr_M / lssvr_gamma for the whole mesh,
 * Dual.py:101).  Enhances the nsub elements elem_ids[0..nsub) of a shard of ne_mesh elements
 * with ONE (M, n_colloc); a p-adaptive mesh is one call per distinct (M, n_colloc) group.
 *   elem_ids[nsub]       device int64 mesh indices, each in [0, ne_mesh) and distinct
 *                        (NULL = all elements in order; nsub must then equal ne_mesh)
 *   gamma_values[ne_mesh] device, indexed by MESH element (NULL = the scalar gamma)
 *   rhs_values[nsub*n_colloc]  (LSSVR_RHS_ARRAY) indexed by position k in elem_ids
 *   W, ldw               row of mesh element id starts at W + id*ldw (ldw >= M; 0 = M): with
 *                        ldw = max M of the mesh and W zeroed beforehand every row is a valid
 *                        Legendre series for lssvr_eval (trailing zeros change nothing)
 *   status[ne_mesh]      indexed by mesh element (may be NULL)
 * Primal solver only (n_colloc >= M-2).  x, u, elem_offset, ne_global, ... as lssvr_enhance.
 */
int lssvr_enhance_subset(const double* x, const double* u, int64_t ne_mesh,
                         const int64_t* elem_ids, int64_t nsub,
                         int64_t elem_offset, int64_t ne_global,
                         double gxmin, double gxmax, double bc_left, double bc_right,
                         int M, int n_colloc, double gamma, const double* gamma_values,
                         int rhs_id, const double* rhs_params_host, const double* rhs_values,
                         double* W, int64_t ldw, int32_t* status, int32_t* fail_count,
                         void* stream);

/*
 * lssvr_enhance_subset_ws -- lssvr_enhance_subset with a caller workspace (ABI 4): above M = 22 the
 * group then runs as the moment / solve kernel pair of lssvr_enhance_ws (twice the speed of the
 * single f64-MFMA kernel, and the near-square refinement) -- rows, status and gamma_values by mesh
 * index, tables and the workspace by position in elem_ids.
 *   work / work_bytes   lssvr_enhance_work_bytes(nsub, M, n_colloc, LSSVR_SOLVER_PRIMAL) bytes of device
 *                       scratch (0 below M = 23); NULL: as lssvr_enhance_subset; too small: LSSVR_ERR_SIZE
 */
int lssvr_enhance_subset_ws(const double* x, const double* u, int64_t ne_mesh,
                            const int64_t* elem_ids, int64_t nsub,
                            int64_t elem_offset, int64_t ne_global,
                            double gxmin, double gxmax, double bc_left, double bc_right,
                            int M, int n_colloc, double gamma, const double* gamma_values,
                            int rhs_id, const double* rhs_params_host, const double* rhs_values,
                            double* W, int64_t ldw, int32_t* status, int32_t* fail_count,
                            void* work, int64_t work_bytes, void* stream);

/*
 * lssvr_enhance_shared -- UNIFORM meshes only; a separate, faster form of the hot path, never
 * chosen implicitly.  On a uniform mesh every element has the same system matrix, so the
 * coefficients are a linear map of the element's data:
 *     W[e,:] = sum_k op[k,:] f(x_k)/scl_e^2 + op[n,:] g_l + op[n+1,:] g_r .
 * op[(n_colloc+2)*M] (device, row-major) is built by the caller with lssvr_enhance itself on a
 * few elements of the mesh's spacing h: rows k < n = response to rhs_values = scl^2 e_k with zero
 * nodal values, row n / n+1 = response to (g_l, g_r) = (1,0) / (0,1) with zero rhs
 * (hybrid_fem_lssvr_amd.ops.build_shared_operator does exactly that; gamma enters only there).
 * Per element the abscissae, f, scl and the boundary rule of lssvr_enhance stay exact; shared
 * is the operator: relative L2 distance from lssvr_enhance ~ (|x|/h) * 2e-16 (1e-11 at 1e5
 * elements of h = 1/12).  M <= 33;
 * LSSVR_RHS_SIN needs |omega x| < 3e9 (beyond: status = LSSVR_ST_FALLBACK).
 * kernel_ms_host != NULL: blocking, returns the dispatch's own duration (measurement aid).
 * The caller is responsible for the mesh being uniform.
 */
int lssvr_enhance_shared(const double* x, const double* u, int64_t ne,
                         int64_t elem_offset, int64_t ne_global,
                         double gxmin, double gxmax, double bc_left, double bc_right,
                         int M, int n_colloc,
                         int rhs_id, const double* rhs_params_host, const double* rhs_values,
                         const double* op,
                         double* W, int32_t* status, int32_t* fail_count, void* stream,
                         float* kernel_ms_host);

/*
 * lssvr_colloc_points -- x_k of every element exactly as `np.linspace(xmin, xmax, n)`
 * produces them (Dual.py:40): xc[e*n + k] = fl(fl(k*step)+x[e]), last = x[e+1].
 * Lets the host tabulate an arbitrary `rhs_func` for LSSVR_RHS_ARRAY.
 */
int lssvr_colloc_points(const double* x, int64_t ne, int n_colloc, double* xc, void* stream);
/* the same abscissae POINT-major, xc[k*ne + e] (ABI 4): tabulate a function on it and the table is
 * in LSSVR_RHS_ARRAY_PM / LSSVR_TABLE_POINT_MAJOR layout */
int lssvr_colloc_points_pm(const double* x, int64_t ne, int n_colloc, double* xc, void* stream);

/*
 * lssvr_p1_assemble -- element-local P1 stiffness and load and their scatter to
 * the global tridiagonal system.  Replaces `laplace.assemble(basis)` /
 * `load.assemble(basis)` (Dual.py:117-128) for ElementLineP1 on a MeshLine:
 *   k_e = abar_e/h_e [[1,-1],[-1,1]],  f_e[j] = sum_q w_q h_e f(x_q) phi_j(xi_q),
 * Gauss-Legendre with `nquad` points per element (scikit-fem's default for P1 is
 * 2).  abar_e = quadrature mean of a (1 when a_quad is NULL).
 *   rhs_id = LSSVR_RHS_SIN: f evaluated in-kernel; LSSVR_RHS_ARRAY:
 *   rhs_quad[e*nquad + q] = f(x_q).   a_quad[e*nquad + q] likewise (may be NULL).
 *   diag[ne+1], off[ne], load[ne+1]  out: assembled bands (off[i] couples i,i+1)
 *   kloc[ne], floc[2*ne]             out, may be NULL: element-local k_e scale and
 *                                    the two load entries
 */
int lssvr_p1_assemble(const double* x, int64_t ne, int nquad,
                      int rhs_id, const double* rhs_params_host, const double* rhs_quad,
                      const double* a_quad,
                      double* diag, double* off, double* load,
                      double* kloc, double* floc, void* stream);

/*
 * lssvr_quad_points -- quadrature abscissae xq[e*nquad + q] used by
 * lssvr_p1_assemble (for host tabulation of rhs / a).
 */
int lssvr_quad_points(const double* x, int64_t ne, int nquad, double* xq, void* stream);

/*
 * lssvr_tridiag_dirichlet_solve -- `enforce(A, b, D=all boundary dofs)` + `solve`
 * (Dual.py:129-130) for the assembled P1 bands: u[0]=u0, u[ne]=u1, interior by a
 * device tridiagonal solve.  work: device scratch of lssvr_tridiag_work_bytes(ne).
 * lssvr_tridiag_work_bytes(ne) == lssvr_tridiag_ns_work_bytes(ne): one solver runs behind both entries.  The value
 * is smaller than earlier builds of ABI 7 returned (they also charged one double per unknown and level that no
 * kernel touched); a buffer sized by the earlier value is large enough.
 */
int64_t lssvr_tridiag_work_bytes(int64_t ne);
int lssvr_tridiag_dirichlet_solve(const double* diag, const double* off, const double* load,
                                  int64_t ne, double u0, double u1,
                                  double* u, void* work, void* stream);

/*
 * lssvr_p1_flux_solve -- the same `enforce` + `solve` (Dual.py:129-130) for the P1 system
 * that lssvr_p1_assemble produces, from the element stiffnesses kloc[ne] (k_e = abar_e/h_e)
 * and the assembled load[ne+1]: A = D^T K D, so u follows from one prefix scan of the
 * element fluxes (no elimination, no amplification by cond(A) ~ ne^2).  u[0] = u0,
 * u[ne] = u1.  work: device scratch of lssvr_p1_flux_work_bytes(ne).  This is what the
 * Python facade's solve_fem uses; lssvr_tridiag_dirichlet_solve takes arbitrary bands.
 */
int64_t lssvr_p1_flux_work_bytes(int64_t ne);
int lssvr_p1_flux_solve(const double* kloc, const double* load, int64_t ne, double u0, double u1,
                        double* u, void* work, void* stream);

/*
 * Sharded form of lssvr_p1_flux_solve (one process per GPU, contiguous element shards).
 * The scan operator is associative, so a shard is summarised by ONE aggregate:
 *   lssvr_p1_flux_aggregate  -> agg3[3] (device) for the shard's ne elements; `work` (same
 *                               size rule) keeps the block scan for the second call;
 *   (caller: all-gather the 24-byte aggregates, combine those of the lower ranks in rank
 *    order into prefix3 and all of them into grand3 with
 *    (a1,r1,g1) o (a2,r2,g2) = (a1+a2, r1+r2, g1+g2 + r2*a1) )
 *   lssvr_p1_flux_finish     -> u[ne+1] of the shard's nodes.
 * first_global / last_global: the shard holds the mesh's first / last element.  kloc[ne],
 * load[ne+1] are the shard's slices (load[i] must be complete for i < ne: assemble with one
 * halo node on the left).  prefix3 / grand3 are DEVICE double[3]; NULL = empty / own total.
 */
int lssvr_p1_flux_aggregate(const double* kloc, const double* load, int64_t ne, int first_global,
                            void* work, double* agg3, void* stream);
int lssvr_p1_flux_finish(const double* kloc, const double* load, int64_t ne, int first_global,
                         int last_global, const void* work, const double* prefix3,
                         const double* grand3, double u0, double u1, double* u, void* stream);

/*
 * lssvr_eval -- `evaluate_solution` (Dual.py:176-203): for each query point the
 * first element j with x[j] <= xq <= x[j+1] (points on an interior node take the
 * LEFT element; below/above the mesh -> element 0 / ne-1, polynomial
 * extrapolation; NaN -> elem -1, value 0), then Clenshaw evaluation in numpy's
 * operation order (legendre.py `legval`).
 *   uq[P] out; elem[P] out (may be NULL), int64 element indices.
 */
int lssvr_eval(const double* x, const double* W, int64_t ne, int M,
               const double* xq, int64_t P, double* uq, int64_t* elem, void* stream);

/*
 * lssvr_eval_error -- error norms of the hybrid solution against the exact solution
 * ex(x) = p[0] * sin(p[1] * x) on the query points (Dual.py:216-217 evaluates
 * `computed_solution` and `exact_solution = true_solution(test_points)`, Dual.py:8-9:
 * p = {1, pi}); reductions on the device, the query values never leave HBM:
 *   out3[0] += sum (u - ex)^2,  out3[1] += sum ex^2,  out3[2] = max(out3[2], max |u - ex|).
 * out3 is a DEVICE double[3] the caller zeroes first (accumulates across calls / shards);
 * NaN query points are skipped, like in lssvr_eval.
 */
int lssvr_eval_error(const double* x, const double* W, int64_t ne, int M,
                     const double* xq, int64_t P, const double* exact_params_host,
                     double* out3, void* stream);

/*
 * A posteriori error indicator and h-refinement (ABI 6; no reference counterpart: Dual.py has no
 * error measure that does not need the exact solution).  lssvr_estimate is for -u'' = f,
 * lssvr_estimate_varcoef (ABI 7) for -(a u')' = f; lssvr_refine serves both.
 *
 * lssvr_eval_deriv -- d^order u_h / dx^order at the query points, order in {0, 1, 2}, with
 * lssvr_eval's element rule (interior node -> left element, outside -> extrapolation, NaN -> elem -1
 * and value 0).  order 0 IS lssvr_eval (bit-equal); orders 1, 2 take the chain-rule factor scl^order,
 * scl = 2/(x[j+1]-x[j]) as lssvr_eval's mapdomain computes it.  Any M >= 1.
 */
int lssvr_eval_deriv(const double* x, const double* W, int64_t ne, int M, int order,
                     const double* xq, int64_t P, double* out, int64_t* elem, void* stream);

/*
 * lssvr_gauss_rule -- HOST: the nq-point Gauss-Legendre rule on [-1, 1] (1 <= nq <= 32), nodes
 * ascending, by Newton iteration on P_nq (matches numpy.polynomial.legendre.leggauss to 1e-15).
 */
int lssvr_gauss_rule(int nq, double* xi_host, double* wt_host);

/*
 * lssvr_estimate_points -- the estimator's abscissae, element-major:
 *   xq[e*nq + q] = 0.5*(x[e]+x[e+1]) + 0.5*(x[e+1]-x[e]) * xi_q      (xi of lssvr_gauss_rule)
 * so that the host can tabulate a callable f for LSSVR_RHS_ARRAY (or, transposed, _ARRAY_PM).
 */
int lssvr_estimate_points(const double* x, int64_t ne, int nq, double* xq, void* stream);

/*
 * lssvr_estimate -- per-element residual indicator of the enhanced solution u_e (row e of W):
 *   eta2[e] = h_e^2 * int_e (f + u_e'')^2 dx + h_e/2 * (J_e^2 + J_{e+1}^2),
 *   J_i = u_{i-1}'(x_i) - u_i'(x_i) at interior nodes, J_0 = J_ne = 0 (Dirichlet ends),
 * the integral by the nq-point Gauss rule (1 <= nq <= 32).
 *   W[ne*M]         1 <= M <= 33; zero-padded rows (lssvr_enhance_subset, ldw = max M) work unchanged
 *   rhs_id          LSSVR_RHS_SIN (in-kernel), LSSVR_RHS_ARRAY (rhs_values[e*nq + q]) or
 *                   LSSVR_RHS_ARRAY_PM (rhs_values[q*ne + e]), f at lssvr_estimate_points
 *   eta2[ne]        out
 *   jump[ne+1]      out, may be NULL: the J_i
 *   out3[3]         out (device): {sum of the finite eta2, max of the finite eta2 (0 if none),
 *                   count of non-finite eta2}; per-workgroup partials in `work`, then one finishing
 *                   workgroup: no atomics, bitwise reproducible from run to run
 *   work            device scratch of lssvr_adapt_work_bytes(ne) bytes
 */
int64_t lssvr_adapt_work_bytes(int64_t ne);
int lssvr_estimate(const double* x, const double* W, int64_t ne, int M, int nq,
                   int rhs_id, const double* rhs_params_host, const double* rhs_values,
                   double* eta2, double* jump, double* out3, void* work, void* stream);

/*
 * lssvr_estimate_varcoef -- lssvr_estimate for -(a u')' = f (ABI 7):
 *   eta2[e] = h_e^2 * int_e (f + a u_e'' + a' u_e')^2 dx + h_e/2 * (J_e^2 + J_{e+1}^2),
 *   J_i = aR_{i-1} u_{i-1}'(x_i) - aL_i u_i'(x_i) at interior nodes, J_0 = J_ne = 0,
 * J the jump of the flux a u'.  Same Gauss rule, W, eta2, out3 and work as lssvr_estimate.
 *   a_values, da_values, rhs_values   a, a' and f at lssvr_estimate_points, all three in table_layout:
 *                   LSSVR_TABLE_ELEMENT_MAJOR (t[e*nq + q]) or LSSVR_TABLE_POINT_MAJOR (t[q*ne + e])
 *   a_ends[2*ne]    {aL_e, aR_e}: a at the left / right end of element e, seen from inside it (a coefficient
 *                   that jumps at a node gives a flux-continuous solution J = 0)
 *   jump[ne+1]      out, may be NULL: the J_i
 * work must hold lssvr_adapt_work_bytes(ne) bytes (not checkable here: no size argument).
 * da_values holding a' - b: the residual f + a u_e'' + (a' - b) u_e' of -(a u')' + b u' = f; J uses a alone.
 */
int lssvr_estimate_varcoef(const double* x, const double* W, int64_t ne, int M, int nq,
                           const double* a_values, const double* da_values, const double* rhs_values,
                           int table_layout, const double* a_ends,
                           double* eta2, double* jump, double* out3, void* work, void* stream);

/*
 * lssvr_refine -- threshold marking and bisection.  Element e is marked iff
 *   (eta2[e] is non-finite, or max > 0 and eta2[e] >= theta^2 * max)  and  x[e+1]-x[e] >= 2*h_min,
 * max = *eta2_max_dev (DEVICE pointer, typically out3 + 1 of lssvr_estimate: no host round trip).
 * theta in [0, 1], h_min >= 0.  A marked element is split at 0.5 * (x[e] + x[e+1]).
 *   x_new[2*ne+1]   out: the new nodes, ascending (capacity 2*ne+1; *ne_new_dev + 1 are written)
 *   parent[2*ne]    out, may be NULL: old element of every new element
 *   ne_new_dev      out (device int64): the new element count
 *   work            device scratch of lssvr_adapt_work_bytes(ne) bytes
 * Three launches (block counts, a one-workgroup scan, scatter): the output is deterministic.
 */
int lssvr_refine(const double* x, int64_t ne, const double* eta2, const double* eta2_max_dev,
                 double theta, double h_min, void* work, double* x_new, int64_t* parent,
                 int64_t* ne_new_dev, void* stream);

/*
 * Reaction term: -(a u')' + c u = f, a > 0 (no reference counterpart, like the variable coefficient).
 * ADDITIVE to ABI 7: the four entries below are new symbols, no existing entry, struct or constant changes, and
 * LSSVR_ABI_VERSION stays 7.  A caller that needs them tests for the symbol (dlsym / hasattr).
 *
 * lssvr_enhance_react -- lssvr_enhance_varcoef plus c_values, tabulated at the collocation points like a_values.
 * With s = 2/h, PDE row k of element e is
 *   -a_k s^2 L_p''(t_k) - da_k s L_p'(t_k) + c_k L_p(t_k).
 * The boundary rows, gamma, the BC-eliminated solve and the fallback status are those of lssvr_enhance_varcoef.
 * Primal solve only: n_colloc < M-2 is LSSVR_ERR_SOLVER (no dual form of these rows).  M <= 16 runs the lane
 * kernel, 17 <= M <= 33 the wave-cooperative MFMA kernel.  c of either sign is accepted here (the rows stay a
 * least-squares fit); the P1 solve is what needs c >= 0.  da_values holding a' - b: the rows of
 * -(a u')' + b u' + c u = f ("Convection term" at the end).
 * lssvr_enhance_react_ws -- with table_layout (LSSVR_TABLE_*, all FOUR tables alike), a workspace argument pair
 * kept for symmetry with lssvr_enhance_varcoef_ws (lssvr_enhance_varcoef_work_bytes() = 0 bytes are needed) and
 * kernel_ms_host (BLOCKING measurement aid).
 */
int lssvr_enhance_react(const double* x, const double* u, int64_t ne,
                        int64_t elem_offset, int64_t ne_global,
                        double gxmin, double gxmax, double bc_left, double bc_right,
                        int M, int n_colloc, double gamma,
                        const double* a_values, const double* da_values, const double* c_values,
                        const double* rhs_values,
                        double* W, int32_t* status, int32_t* fail_count, void* stream);
int lssvr_enhance_react_ws(const double* x, const double* u, int64_t ne,
                           int64_t elem_offset, int64_t ne_global,
                           double gxmin, double gxmax, double bc_left, double bc_right,
                           int M, int n_colloc, double gamma,
                           const double* a_values, const double* da_values, const double* c_values,
                           const double* rhs_values, int table_layout,
                           double* W, int32_t* status, int32_t* fail_count,
                           void* work, int64_t work_bytes, void* stream, float* kernel_ms_host);

/*
 * lssvr_p1_assemble_react -- lssvr_p1_assemble plus c_quad[e*nquad + q] (c at lssvr_quad_points): the consistent
 * mass matrix
 *   m_e[i][j] = h_e sum_q w_q c(x_q) phi_i(xi_q) phi_j(xi_q)
 * joins the bands: diag[i] += m_i[0][0] + m_{i-1}[1][1], off[i] = -abar_i/h_i + m_i[0][1].  load, kloc (= abar/h)
 * and floc are those of lssvr_p1_assemble.  c_quad == NULL IS lssvr_p1_assemble (same launch, same bits).
 * lssvr_tridiag_dirichlet_solve takes the bands as they are; it does not pivot, so the caller keeps the matrix
 * SPD (c >= 0).  lssvr_p1_flux_solve does not apply (it factors A = D^T K D, which a mass matrix breaks).
 */
int lssvr_p1_assemble_react(const double* x, int64_t ne, int nquad,
                            int rhs_id, const double* rhs_params_host, const double* rhs_quad,
                            const double* a_quad, const double* c_quad,
                            double* diag, double* off, double* load,
                            double* kloc, double* floc, void* stream);

/*
 * lssvr_estimate_react -- lssvr_estimate_varcoef plus c_values at lssvr_estimate_points (same table_layout):
 *   eta2[e] = h_e^2 * int_e (f + a u_e'' + a' u_e' - c u_e)^2 dx + h_e/2 * (J_e^2 + J_{e+1}^2),
 * J the jump of the flux a u' as in lssvr_estimate_varcoef.  Same reduction: no atomics, bitwise reproducible.
 * da_values holding a' - b: the residual f + a u_e'' + (a' - b) u_e' - c u_e of -(a u')' + b u' + c u = f; the
 * flux jump uses a alone and does not change.
 */
int lssvr_estimate_react(const double* x, const double* W, int64_t ne, int M, int nq,
                         const double* a_values, const double* da_values, const double* c_values,
                         const double* rhs_values, int table_layout, const double* a_ends,
                         double* eta2, double* jump, double* out3, void* work, void* stream);

/*
 * Several load cases on one mesh: factor once, many right-hand sides.  ADDITIVE to ABI 7 like the reaction entries
 * (a new symbol; LSSVR_ABI_VERSION stays 7).
 *
 * lssvr_enhance_multi -- lssvr_enhance_react_ws (c_values given) or lssvr_enhance_varcoef_ws (c_values == NULL) for
 * ncases right-hand sides, nodal vectors and Dirichlet pairs at once.  The element system S = G + eps (I + C^T C)
 * depends on the mesh, the a / a' / c tables, gamma, M and n_colloc only, so for M <= 16 one lane kernel forms and
 * factors it ONCE per element and pass and runs the two triangular solves per case; a pass holds up to RC(M) cases
 * in registers (8 at M = 2, 4 at M = 3..6 and 9..13, 3 at 7, 2 at 8 and 14, 1 at 15 and 16)
 * and ceil(ncases / RC) passes are launched, each of which reads the coefficient tables once.  17 <= M <= 33 runs
 * the single-case entry's kernel once per case: correct, no faster than separate calls, and a shard that holds an
 * end of the global domain reads bc_values back to the host first (one stream synchronisation).
 * All pointers are DEVICE pointers, case-major and contiguous:
 *   u[ncases][ne+1]            nodal values of every case
 *   bc_values[ncases][2]       {left, right} Dirichlet value of every case; NULL: all zero.  The boundary rule is
 *                              that of lssvr_enhance with the case's own pair
 *   a_values, da_values        required, shared by the cases; c_values may be NULL (no reaction term)
 *   rhs_values[ncases][ne*n_colloc]   every slab in table_layout (LSSVR_TABLE_*), like the coefficient tables
 *   W[ncases][ne][M]           out
 *   status[ncases][ne]         out, may be NULL
 *   fail_count                 one counter, may be NULL: +1 per (case, element) fallback
 * Fallback (Dual.py:164-169) per case: a breakdown of the factorisation gives EVERY case of that element the linear
 * interpolant of its own (g_l, g_r) and status 1; a case whose own right-hand side or solution is not finite falls
 * back alone.  Primal solve only: n_colloc < M-2 is LSSVR_ERR_SOLVER; ncases < 1 is LSSVR_ERR_SIZE; ne == 0 is a
 * successful no-op.  kernel_ms_host != NULL: BLOCKING, the duration from the first pass's begin to the last one's
 * end (above M = 16: the sum over the cases).
 * da_values holding a' - b: the rows of -(a u')' + b u' + c u = f for every case ("Convection term" at the end).
 */
int lssvr_enhance_multi(const double* x, const double* u, int64_t ne,
                        int64_t elem_offset, int64_t ne_global,
                        double gxmin, double gxmax, const double* bc_values, int ncases,
                        int M, int n_colloc, double gamma,
                        const double* a_values, const double* da_values, const double* c_values,
                        const double* rhs_values, int table_layout,
                        double* W, int32_t* status, int32_t* fail_count,
                        void* stream, float* kernel_ms_host);

/*
 * hp-adaptive refinement: raise the degree where the solution is smooth, bisect where it is not (no reference
 * counterpart).  ADDITIVE to ABI 7 like the reaction entries (four new symbols;
 * LSSVR_ABI_VERSION stays 7).  Together with lssvr_enhance_subset_ws (one degree per group of elements) and
 * lssvr_estimate / lssvr_eval (zero-padded rows) they close the loop: estimate, lssvr_smoothness, lssvr_refine_hp,
 * lssvr_group_by_degree, one lssvr_enhance_subset_ws per non-empty degree.
 *
 * lssvr_smoothness -- decay rate of every element's Legendre coefficients.
 *   W[ne*ldw]       zero-padded rows, 2 <= ldw <= 33
 *   deg[ne]         device int32: the degree parameter M of every element, 2 <= deg[e] <= ldw
 *   sigma[ne]       out.  With M = deg[e], c_p = |W[e*ldw + p]| (p < M), mx = max_p c_p and the envelope
 *                   env_p = max_{p <= q < M} c_q for p = 1 .. M-1 (it absorbs the parity zeros of a symmetric
 *                   solution), sigma[e] is minus the least-squares slope of ln env_p against p over the points with
 *                   env_p >= 2^-52 * mx (and env_p > 0):
 *                     sigma = -sum (p - pbar)(y_p - ybar) / sum (p - pbar)^2,  y_p = ln env_p,
 *                   pbar, ybar the means over the kept points.  NaN when one of the M coefficients is not finite
 *                   (or deg[e] is outside [2, ldw]: nothing of the row is read); otherwise +inf when mx == 0,
 *                   M < 3 or fewer than two points are kept.
 * The window is [-1, 1] for every element, so sigma does not depend on the element's length.  A lane per element,
 * W staged through LDS, at most 4096 workgroups of 128 elements per pass; no atomics, bitwise reproducible.
 */
int lssvr_smoothness(const double* W, int64_t ldw, const int32_t* deg, int64_t ne, double* sigma, void* stream);

/*
 * lssvr_refine_hp -- lssvr_refine's marking, then p or h.  Element e is marked iff
 *   eta2[e] is non-finite, or max > 0 and eta2[e] >= theta^2 * max          (max = *eta2_max_dev, a DEVICE pointer)
 * -- lssvr_refine's predicate without the length condition.  A marked element
 *   is RAISED (deg_new = deg[e] + dM, not split)  iff  sigma[e] >= sigma_min and deg[e] + dM <= M_max
 *                                                     (a NaN sigma or sigma_min compares false),
 *   otherwise is BISECTED at 0.5 * (x[e] + x[e+1])  iff  x[e+1] - x[e] >= 2*h_min; both children inherit deg[e],
 *   otherwise stays as it is.
 * theta in [0, 1], h_min >= 0 and finite, dM >= 1, 2 <= M_max <= 33.
 *   sigma[ne]       lssvr_smoothness of the solution the indicator belongs to
 *   deg[ne]         device int32
 *   x_new[2*ne+1]   out: the new nodes, ascending (capacity 2*ne+1; *ne_new_dev + 1 are written)
 *   deg_new[2*ne]   out (device int32): degree of every new element
 *   parent[2*ne]    out, may be NULL: old element of every new element
 *   ne_new_dev      out (device int64): the new element count
 *   counts2_dev     out (device int64[2]): {elements bisected, elements raised}
 *   work            device scratch of lssvr_adapt_work_bytes(ne) bytes
 * The three kernels of lssvr_refine (block counts, a one-workgroup scan, scatter) in their hp instance: deterministic,
 * and x_new and parent equal lssvr_refine's bit for bit when nothing is raised.
 */
int lssvr_refine_hp(const double* x, int64_t ne, const double* eta2, const double* eta2_max_dev,
                    double theta, double h_min, const double* sigma, const int32_t* deg,
                    double sigma_min, int dM, int M_max, void* work,
                    double* x_new, int32_t* deg_new, int64_t* parent, int64_t* ne_new_dev,
                    int64_t* counts2_dev, void* stream);

/*
 * lssvr_group_by_degree -- stable counting sort of the element indices by degree: the elem_ids of
 * lssvr_enhance_subset(_ws) for every degree of a p-adaptive mesh, grouped on the device.
 *   deg[ne]         device int32
 *   ids[ne]         out (device int64): the elements of degree M are ids[offsets[M] .. offsets[M+1]) in ascending
 *                   mesh order
 *   offsets[35]     out (device int64): offsets[0] = offsets[1] = offsets[2] = 0 (no degree below 2),
 *                   offsets[34] = the number of elements sorted
 *   work            device scratch of lssvr_group_work_bytes(ne) bytes
 * An element whose degree is outside [2, 33] is in no group: nothing is written for it, offsets[34] counts the
 * others, the trailing ids stay unwritten and the call still succeeds -- validate the degrees first.
 * Per-workgroup histograms of the 32 degrees, one scanning workgroup, a scatter by ballot rank: no atomics, the
 * output is deterministic.
 */
int64_t lssvr_group_work_bytes(int64_t ne);
int lssvr_group_by_degree(const int32_t* deg, int64_t ne, int64_t* ids, int64_t* offsets,
                          void* work, void* stream);

/*
 * Convection term: -(a u')' + b u' + c u = f (no reference counterpart).  ADDITIVE to ABI 7 like the reaction entries:
 * three new symbols, no existing entry, struct or constant changes, LSSVR_ABI_VERSION stays 7.
 *
 * Enhancement and indicator need no new entry.  -(a u')' + b u' = -a u'' - (a' - b) u', and lssvr_enhance_varcoef(_ws),
 * lssvr_enhance_react(_ws), lssvr_enhance_multi, lssvr_estimate_varcoef and lssvr_estimate_react read da_values only
 * as the coefficient of the first-derivative term (the flux jump of the indicator uses a alone).  THE CONVENTION: a
 * caller with a convection coefficient b passes da_values[k] = a'(x_k) - b(x_k) at the same points, in the same
 * layout; everything else is as documented at those entries.
 *
 * What changes is the P1 half: the Galerkin matrix of b u' is not symmetric.
 *
 * lssvr_p1_assemble_conv -- lssvr_p1_assemble_react plus b_quad[e*nquad + q] (b at lssvr_quad_points).  Per element
 *   C_e[i][j] = sum_q w_q b(x_q) phi_i(xi_q) * s_j,   s_0 = -1, s_1 = +1   (h_e phi_j' = -+1),
 * joins the element matrix.  With beta0_e = sum_q w_q b_q (1 - xi_q), beta1_e = sum_q w_q b_q xi_q:
 *   diag[ne+1]   diag[i] = (abar_i/h_i + m_i[0][0] - beta0_i) + (abar_{i-1}/h_{i-1} + m_{i-1}[1][1] + beta1_{i-1})
 *   sub[ne]      the coefficient of u_i in row i+1:   -abar_i/h_i + m_i[0][1] - beta1_i
 *   sup[ne]      the coefficient of u_{i+1} in row i: -abar_i/h_i + m_i[0][1] + beta0_i
 *   load[ne+1], kloc[ne], floc[2*ne] (the last two may be NULL): those of lssvr_p1_assemble
 * (constant coefficients on a uniform mesh: sub, sup = -a/h -+ b/2 + c h/6, diag = 2a/h + 2ch/3).  a_quad, c_quad and
 * b_quad may each be NULL (a = 1, c = 0, b = 0).  b_quad == NULL gives sub == sup == the `off` of
 * lssvr_p1_assemble_react and its diag and load, bit for bit.  A thread per node gathers its two elements: no atomics,
 * bitwise reproducible.
 *
 * lssvr_tridiag_ns_dirichlet_solve -- lssvr_tridiag_dirichlet_solve for these bands: u[0] = u0, u[ne] = u1 and, for
 * 0 < i < ne,  sub[i-1] u[i-1] + diag[i] u[i] + sup[i] u[i+1] = load[i].  Same recursive substructuring (every 8th
 * unknown a separator; condense, reduce, expand; parallel cyclic reduction in LDS at <= 512 unknowns), both
 * off-diagonal bands carried through every level.  work: device scratch of lssvr_tridiag_ns_work_bytes(ne), which
 * equals lssvr_tridiag_work_bytes(ne): the two entries share their kernels, and a buffer sized by either function
 * serves both.  This entry alone ends the <= 512-unknown level with one step of iterative refinement.
 * NO PIVOTING.  That is safe when every row is diagonally dominant, |sub[i-1]| + |sup[i]| <= diag[i]: elimination
 * keeps row dominance, so every Schur complement of every level has it and no divisor vanishes.  The rows of
 * lssvr_p1_assemble_conv are dominant when c >= 0 and the cell Peclet number |bbar_e| h_e / (2 abar_e) <= 1 on every
 * element (bbar, abar: quadrature means; exact for coefficients constant on each element, DESIGN.md section 18 for
 * the rest).  Above that the P1 solution oscillates and the solve may lose accuracy without notice: refine the mesh
 * until the bound holds (there is no upwinding here).  The caller checks; this entry does not look at the values.
 */
int lssvr_p1_assemble_conv(const double* x, int64_t ne, int nquad,
                           int rhs_id, const double* rhs_params_host, const double* rhs_quad,
                           const double* a_quad, const double* c_quad, const double* b_quad,
                           double* diag, double* sub, double* sup, double* load,
                           double* kloc, double* floc, void* stream);
int64_t lssvr_tridiag_ns_work_bytes(int64_t ne);
int lssvr_tridiag_ns_dirichlet_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                     int64_t ne, double u0, double u1,
                                     double* u, void* work, void* stream);

/*
 * Several load cases on one mesh and one operator, the P1 half (additive to ABI 7; lssvr_enhance_multi is the other
 * half).  nc >= 1 cases; case j's arrays lie j * (their single-case length) doubles after case 0's.
 *
 * lssvr_p1_load_multi -- load[nc][ne+1] from rhs_quad[nc][ne*nquad] (f at lssvr_quad_points, case by case) in one
 * launch that reads x once and writes no matrix bands.  Replaces nc calls of lssvr_p1_assemble / _react / _conv with
 * LSSVR_RHS_ARRAY as far as `load` goes: load[j] is bit-identical to theirs for rhs_quad[j] (the load does not depend
 * on a_quad, c_quad or b_quad).  The bands come from ONE call of those entries with any right-hand side.
 *
 * lssvr_tridiag_dirichlet_solve_multi -- replaces nc calls of lssvr_tridiag_dirichlet_solve on the same diag and off,
 * bit-identical: u[j][0] = bc_values[j][0], u[j][ne] = bc_values[j][1] and the interior of case j from load[j].
 * bc_values is a DEVICE array [nc][2] (NULL: zeros), the convention of lssvr_enhance_multi: nothing is read back and
 * no stream is synchronised, so the call can be captured in a graph.  The cases run 8
 * to a pass; in a pass the bands are read and the pivots of every level computed once (the single entry is the pass of
 * one case of the same kernels, with its end values by value).  work: device scratch of
 * work_bytes >= lssvr_tridiag_multi_work_bytes(ne, nc) bytes; that value equals lssvr_tridiag_work_bytes(ne) at
 * nc = 1, grows with nc up to the 8 cases of one pass and with ne.  ne == 1 writes only the two end values of every
 * case.  Same no-pivoting rule as the single entry.
 *
 * lssvr_tridiag_ns_dirichlet_solve_multi -- replaces nc calls of lssvr_tridiag_ns_dirichlet_solve on the same diag,
 * sub and sup, bit-identical (the step of iterative refinement of the <= 512-unknown level included, once per case).
 * Arguments and workspace as above.
 */
int lssvr_p1_load_multi(const double* x, int64_t ne, int nquad, const double* rhs_quad, int nc, double* load,
                        void* stream);
int64_t lssvr_tridiag_multi_work_bytes(int64_t ne, int nc);
int lssvr_tridiag_dirichlet_solve_multi(const double* diag, const double* off, const double* load,
                                        int64_t ne, int nc, const double* bc_values,
                                        double* u, void* work, int64_t work_bytes, void* stream);
int lssvr_tridiag_ns_dirichlet_solve_multi(const double* diag, const double* sub, const double* sup,
                                           const double* load, int64_t ne, int nc, const double* bc_values,
                                           double* u, void* work, int64_t work_bytes, void* stream);

/*
 * Neumann and Robin boundary conditions (no reference counterpart).  ADDITIVE to ABI 7: four new
 * symbols and two constants, no existing entry, struct or constant changes, LSSVR_ABI_VERSION stays 7.
 *
 * At each end of the domain, independently, LSSVR_END_DIRICHLET (u = g, what every other entry does) or
 * LSSVR_END_ROBIN:  a du/dn + kappa u = g  with the outward normal (du/dn = -u' at x_0, +u' at x_ne), kappa >= 0;
 * Neumann is kappa = 0.  A Robin end adds kappa u(x_end) v(x_end) to the bilinear form and g v(x_end) to the load, so
 * its node stays an unknown and its row is  (diag[end] + kappa) u[end] + (neighbour) = load[end] + g.
 *
 * lssvr_tridiag_bc_solve_multi -- lssvr_tridiag_dirichlet_solve_multi with that choice at each end.  kind_left,
 * kind_right: LSSVR_END_*; kappa_host[2]: host array, read at a Robin end (finite, >= 0); end_values: DEVICE array
 * [nc][2] (NULL: zeros), g of case j at a Robin end and the value itself at a Dirichlet end.  kappa and g are added
 * inside the kernels where they read the end row: diag, off and load are read only, as assembled by lssvr_p1_assemble
 * / _react.  A single right-hand side is nc = 1.  Both ends Dirichlet gives the bits of
 * lssvr_tridiag_dirichlet_solve_multi.  work: device scratch of work_bytes >= lssvr_tridiag_bc_work_bytes(ne, nc),
 * which is sized for two free ends (ne + 1 unknowns) whatever the kinds are.  Same no-pivoting rule: kappa >= 0 keeps
 * an SPD matrix SPD.  Two Neumann ends without a reaction term make the matrix singular; the caller checks.
 * (lssvr_tridiag_pivot_solve_multi, below, is the solve that pivots.)
 *
 * lssvr_tridiag_ns_bc_solve_multi -- the same for the bands of lssvr_p1_assemble_conv; both ends Dirichlet gives the
 * bits of lssvr_tridiag_ns_dirichlet_solve_multi.  Row dominance at a Robin end needs kappa + b(x_end) n / 2 >= 0
 * (n = -1 left, +1 right); the caller checks.
 *
 * lssvr_estimate_ends -- the boundary term of the indicator, after lssvr_estimate, lssvr_estimate_varcoef or
 * lssvr_estimate_react on the same stream: at a Robin end, with the end element's row of W[ne][M] (M: the row
 * length; zero-padded rows of mixed degree are fine),
 *   J = g - kappa u_e(x_end) - a du_e/dn,   eta2[end element] += h/2 J^2,
 * and out3 follows: sum += the added term, max = max(max, new eta2); a value that becomes non-finite raises the
 * non-finite count instead.  g_host[2], a_ends_host[2] (a at x_0 and at x_ne), kappa_host[2]: host arrays.  A
 * Dirichlet end adds nothing; two Dirichlet ends launch nothing.  One thread, no atomics: reproducible.
 */
#define LSSVR_END_DIRICHLET 0
#define LSSVR_END_ROBIN 1
int64_t lssvr_tridiag_bc_work_bytes(int64_t ne, int nc);
int lssvr_tridiag_bc_solve_multi(const double* diag, const double* off, const double* load,
                                 int kind_left, int kind_right, const double* end_values,
                                 const double* kappa_host, int64_t ne, int nc,
                                 double* u, void* work, int64_t work_bytes, void* stream);
int lssvr_tridiag_ns_bc_solve_multi(const double* diag, const double* sub, const double* sup, const double* load,
                                    int kind_left, int kind_right, const double* end_values,
                                    const double* kappa_host, int64_t ne, int nc,
                                    double* u, void* work, int64_t work_bytes, void* stream);
int lssvr_estimate_ends(const double* x, const double* W, int M, int64_t ne, int kind_left, int kind_right,
                        const double* kappa_host, const double* g_host, const double* a_ends_host,
                        double* eta2, double* out3, void* stream);

/*
 * Pivoting tridiagonal solve.  ADDITIVE to ABI 7: two new symbols, no existing entry, struct or
 * constant changes, LSSVR_ABI_VERSION stays 7.
 *
 * lssvr_tridiag_pivot_solve_multi -- lssvr_tridiag_ns_bc_solve_multi for well-conditioned tridiagonal matrices whose
 * rows need not be diagonally dominant (negative or sign-changing reaction, cell Peclet number above 1,
 * kappa + b n / 2 < 0 at a Robin end); what is not covered is in DESIGN.md section 24.  A recursive partitioned solve
 * with scaled partial pivoting inside every partition and at the coarsest level.  diag, sub, sup, load, kind_left,
 * kind_right, end_values, kappa_host,
 * ne, nc and u as in lssvr_tridiag_ns_bc_solve_multi, except that kappa_host may have either sign (finite); a
 * symmetric caller passes `off` for both sub and sup.  The bands and loads are read only.  ne == 1 and systems of one
 * or two unknowns are handled.  Row j of u is bit-identical to the nc = 1 call on case j.
 *   info   DEVICE int32 (NULL: not wanted): the number of pivots, over all levels, that were zero or not finite after
 *          the row choice.  0: no such pivot was met -- no more than that: a matrix that is singular only up to
 *          rounding gives large finite values and 0.  > 0: the matrix is singular; the entry still returns
 *          LSSVR_OK, u then holds finite garbage -- such a pivot's reciprocal is replaced by 0, nothing is divided by
 *          it.  Read it after synchronising the stream.
 *   work   device scratch of work_bytes >= lssvr_tridiag_pivot_work_bytes(ne, nc), sized for two free ends.
 * Above cell Peclet number 1 this returns the Galerkin solution, oscillations included: pivoting is not stabilisation.
 * lssvr_tridiag_pivot_solve_host -- the same solve on HOST arrays (diag, sub, sup, load, end_values, u and info all in
 * host memory), partition by partition through the routines the kernels are made of, with the same levels and passes.
 * No device is touched: it exists so that the arithmetic can be checked where there is no GPU, and it is not fast.
 */
int64_t lssvr_tridiag_pivot_work_bytes(int64_t ne, int nc);
int lssvr_tridiag_pivot_solve_multi(const double* diag, const double* sub, const double* sup, const double* load,
                                    int kind_left, int kind_right, const double* end_values,
                                    const double* kappa_host, int64_t ne, int nc,
                                    double* u, int32_t* info, void* work, int64_t work_bytes, void* stream);
int lssvr_tridiag_pivot_solve_host(const double* diag, const double* sub, const double* sup, const double* load,
                                   int kind_left, int kind_right, const double* end_values,
                                   const double* kappa_host, int64_t ne, int nc, double* u, int32_t* info);

/*
 * Goal-oriented error estimation (dual-weighted residual).  ADDITIVE to ABI 7 (new symbols; LSSVR_ABI_VERSION stays 7).
 *
 * lssvr_estimate_goal -- for a quantity of interest J(u) = int j u dx of -(a u')' + c u = f (no convection term: the
 * adjoint then has the primal's matrix), the residual of the enhanced primal solution u_e (row e of Wu[ne][M])
 * weighted with the enhanced dual solution z_e (row e of Wz[ne][M], the solution for the right-hand side j with zero
 * end data; same M and row length):
 *   eta[e]  = int_e R z_e dx - 1/2 (J_e z_e(x_e) + J_{e+1} z_e(x_{e+1}))
 *             + at a Robin end of the domain, in its end element: (g - kappa u_e(x_end) - a du_e/dn) z_e(x_end)
 *   R = f + a u_e'' + a' u_e' - c u_e (lssvr_estimate_react's residual; c_values == NULL drops the c term),
 *   J_i = aR_{i-1} u_{i-1}'(x_i) - aL_i u_i'(x_i) the flux jump of lssvr_estimate_varcoef, J_0 = J_ne = 0,
 *   eta2[e] = eta[e]^2 (what lssvr_refine marks from),   q[e] = int_e j u_e dx (q may be NULL).
 * eta is SIGNED: for a continuous u_e that takes the Dirichlet values and the exact z, sum_e eta[e] = J(u) - J(u_e),
 * so sum eta + sum q is a corrected value of J.  The integrals are the nq-point Gauss rule of lssvr_gauss_rule.
 *   a_values, da_values, c_values, rhs_values, goal_values   a, a', c, f and j at lssvr_estimate_points, all in
 *                   table_layout (LSSVR_TABLE_ELEMENT_MAJOR t[e*nq + q] or LSSVR_TABLE_POINT_MAJOR t[q*ne + e])
 *   a_ends          [ne][2] as in lssvr_estimate_varcoef
 *   kind_left, kind_right, kappa_host[2], g_host[2], a_bnd_host[2]   the ends of the domain as in lssvr_estimate_ends
 *                   (g of the PRIMAL problem; a_bnd = a at x_0 and x_ne); a Dirichlet end adds nothing
 *   jump_free       0: as above.  1: the weight is z_e - I_h z_e, I_h z_e the linear interpolant of z_e at the element's
 *                   two nodes; it vanishes there, so the jump and end terms drop out: eta[e] = int_e R (z_e - I_h z_e).
 *                   This is the form to MARK from (a bisection of element e reduces it; half a jump at a node shared
 *                   with a coarse neighbour it does not); its sum is the correction only where the residual is
 *                   orthogonal to the piecewise linears.  q and out4[3] do not depend on it.
 *   out4            device double[4] = {sum of eta over the elements whose eta^2 is finite, max of the finite eta2,
 *                   number of non-finite eta2, sum of the finite q}
 *   work            device scratch of lssvr_goal_work_bytes(ne) bytes
 * 1 <= M <= 33, 1 <= nq <= 32.  A non-finite row of Wu makes its own eta and, through the flux jumps, both
 * neighbours' non-finite.  No atomics: every output is bitwise reproducible.
 */
int64_t lssvr_goal_work_bytes(int64_t ne);
int lssvr_estimate_goal(const double* x, const double* Wu, const double* Wz, int64_t ne, int M, int nq,
                        const double* a_values, const double* da_values, const double* c_values,
                        const double* rhs_values, const double* goal_values, int table_layout,
                        const double* a_ends, int kind_left, int kind_right, const double* kappa_host,
                        const double* g_host, const double* a_bnd_host, int jump_free,
                        double* eta, double* eta2, double* q, double* out4, void* work, void* stream);

/*
 * Periodic boundary conditions (no reference counterpart).  ADDITIVE to ABI 7: four new symbols,
 * no existing entry, struct or constant changes, LSSVR_ABI_VERSION stays 7.
 *
 * u(x_0) = u(x_ne) and a u'(x_0) = a u'(x_ne): node ne is node 0.  Its value s is one unknown, and the rows that the
 * assembly entries write for node 0 and for node ne are the two halves of its row:
 *   (diag[0] + diag[ne]) s + sup[0] u[1] + sub[ne-1] u[ne-1] = load[0] + load[ne]
 * (off[0] and off[ne-1] for the symmetric bands); the rows 0 < i < ne are those of the Dirichlet entries with
 * u[0] = u[ne] = s.  The matrix is cyclic tridiagonal: two corner entries.
 *
 * lssvr_tridiag_periodic_solve_multi -- nc >= 1 right-hand sides load[nc][ne+1] on the bands of lssvr_p1_assemble /
 * _react -> u[nc][ne+1] with u[j][0] == u[j][ne] == s_j, bit for bit.  A single right-hand side is nc = 1.  By
 * linearity u_int = y_j + s_j z: y_j the Dirichlet solve of case j with end values (0, 0), z the Dirichlet solve with
 * zero load and end values (1, 1) -- independent of the load, solved once per call -- and
 *   s_j = (load_j[0] + load_j[ne] - sup[0] y_j[1] - sub[ne-1] y_j[ne-1])
 *         / (diag[0] + diag[ne] + sup[0] z[1] + sub[ne-1] z[ne-1]),
 * the Schur complement on the seam.  y and z run through the kernels of lssvr_tridiag_dirichlet_solve_multi (8 cases to
 * a pass, z a pass of its own); one thread per case computes s_j, one pass writes u = y + s z in place.  Row j does not
 * depend on nc, bit for bit.  diag, off and load are read only.  ne >= 2.  work: device scratch of
 * work_bytes >= lssvr_tridiag_periodic_work_bytes(ne, nc), which is lssvr_tridiag_multi_work_bytes(ne, nc) plus z, its
 * zero load and the s_j (host arithmetic only).  Same no-pivoting rule as the Dirichlet entries: the cyclic matrix of
 * an SPD / row-dominant problem is SPD / row-dominant, and so is its Schur complement.  The denominator vanishes for a
 * singular problem (no reaction term: u is determined up to a constant); the caller checks, this entry does not.
 *
 * lssvr_tridiag_ns_periodic_solve_multi -- the same for the bands of lssvr_p1_assemble_conv, through the kernels of
 * lssvr_tridiag_ns_dirichlet_solve_multi (the step of iterative refinement of the <= 512-unknown level included).
 *
 * lssvr_estimate_seam -- the seam term of the indicator, after lssvr_estimate, lssvr_estimate_varcoef or
 * lssvr_estimate_react on the same stream (they set J_0 = J_ne = 0): with row ne-1 and row 0 of W[ne][M],
 *   J = a_seam[0] u_{ne-1}'(x_ne) - a_seam[1] u_0'(x_0),   eta2[ne-1] += h_{ne-1}/2 J^2,   eta2[0] += h_0/2 J^2,
 * a_seam_host[2] (host) = a at x_ne seen from element ne-1 and a at x_0 seen from element 0.  out3 follows as in
 * lssvr_estimate_ends: sum += the added terms, max = max(max, new eta2); a value that becomes non-finite raises the
 * non-finite count instead.  ne >= 2.  One thread (element ne-1, then element 0), no atomics: reproducible.
 *
 * The enhancement needs no new entry: with elem_offset = 1 and ne_global = ne + 2 no Dirichlet flag fires, and the
 * elements 0 and ne-1 take s as their nodal constraint like any interior value.
 */
int64_t lssvr_tridiag_periodic_work_bytes(int64_t ne, int nc);
int lssvr_tridiag_periodic_solve_multi(const double* diag, const double* off, const double* load,
                                       int64_t ne, int nc, double* u, void* work, int64_t work_bytes, void* stream);
int lssvr_tridiag_ns_periodic_solve_multi(const double* diag, const double* sub, const double* sup,
                                          const double* load, int64_t ne, int nc,
                                          double* u, void* work, int64_t work_bytes, void* stream);
int lssvr_estimate_seam(const double* x, const double* W, int M, int64_t ne, const double* a_seam_host,
                        double* eta2, double* out3, void* stream);

/*
 * Element lists for the table kernels: hp refinement of -(a u')' + b u' + c u = f.  ADDITIVE to
 * ABI 7: two new symbols, no existing entry, struct, constant or kernel instantiation changes, LSSVR_ABI_VERSION stays 7.
 *
 * lssvr_enhance_react_subset -- lssvr_enhance_react_ws for the nsub elements elem_ids[0..nsub) of a shard of ne_mesh
 * elements, with the element-list conventions of lssvr_enhance_subset: ONE (M, n_colloc) per call, a p-adaptive mesh
 * is one call per degree that occurs (lssvr_group_by_degree supplies the lists).
 *   x[ne_mesh+1], u[ne_mesh+1], gamma_values[ne_mesh] (NULL = the scalar gamma), status[ne_mesh] (may be NULL)
 *                        indexed by MESH element
 *   elem_ids[nsub]       device int64 mesh indices, distinct (NULL = all elements in order; nsub must equal ne_mesh)
 *   a_values, da_values, c_values, rhs_values   a, a', c, f at the n_colloc abscissae of the LISTED elements
 *                        (lssvr_colloc_points_subset), indexed by POSITION in elem_ids: LSSVR_TABLE_ELEMENT_MAJOR
 *                        t[pos*n_colloc + k] or LSSVR_TABLE_POINT_MAJOR t[k*nsub + pos].  da_values = a' - b gives the
 *                        convection rows (the convention above)
 *   c_values == NULL     the variable-coefficient rows -(a u')' = f: the kernels lssvr_enhance_varcoef_ws picks for
 *                        this (M, n_colloc) -- the lane kernel up to M = 22, the f64-MFMA kernel above.  Otherwise the
 *                        reaction rows: the lane kernel up to M = 16, the f64-MFMA kernel above
 *   W, ldw               row of mesh element id starts at W + id*ldw (ldw >= M; 0 = M), as in lssvr_enhance_subset;
 *                        rows that are not listed are not written
 * An id outside [0, ne_mesh) touches nothing -- no row, no status, no table entry is used for a store -- and is
 * counted in fail_count.  Primal solve only: n_colloc < M-2 is LSSVR_ERR_SOLVER (a list launch has no dual route).
 * elem_ids == NULL with nsub != ne_mesh, nsub > ne_mesh and 0 < ldw < M are LSSVR_ERR_SIZE; nsub == 0 succeeds and
 * launches nothing.  With elem_ids == NULL, gamma_values == NULL and ldw 0 or M the call issues the launch of
 * lssvr_enhance_react_ws (c_values == NULL: lssvr_enhance_varcoef_ws) and gives its bits.  The rows of the lane
 * kernels do not depend on what else is in the launch, bit for bit; the f64-MFMA kernel picks the series or the
 * recurrence for its boundary rows per PAIR of launch neighbours, so there a row may differ in the last bits with its
 * neighbour.
 *
 * lssvr_colloc_points_subset -- the abscissae of lssvr_colloc_points(_pm) for the listed elements only, by position:
 * xc[pos*n_colloc + k] (LSSVR_TABLE_ELEMENT_MAJOR) or xc[k*nsub + pos] (LSSVR_TABLE_POINT_MAJOR), bit for bit the
 * entries of element elem_ids[pos] of the whole-mesh call.  elem_ids == NULL: all elements in order (nsub must equal
 * ne_mesh).  Nothing is written for an id outside [0, ne_mesh).
 */
int lssvr_enhance_react_subset(const double* x, const double* u, int64_t ne_mesh,
                               const int64_t* elem_ids, int64_t nsub,
                               int64_t elem_offset, int64_t ne_global,
                               double gxmin, double gxmax, double bc_left, double bc_right,
                               int M, int n_colloc, double gamma, const double* gamma_values,
                               const double* a_values, const double* da_values, const double* c_values,
                               const double* rhs_values, int table_layout,
                               double* W, int64_t ldw, int32_t* status, int32_t* fail_count, void* stream);
int lssvr_colloc_points_subset(const double* x, int64_t ne_mesh, const int64_t* elem_ids, int64_t nsub,
                               int n_colloc, int table_layout, double* xc, void* stream);

/*
 * Eigenproblems: -(a u')' + c u = lambda rho u, a > 0, rho > 0, with u = 0 or a du/dn + kappa u = 0 at each end (no
 * reference counterpart).  ADDITIVE to ABI 7: nine new symbols, no existing entry, struct, constant
 * or kernel changes, LSSVR_ABI_VERSION stays 7.
 *
 * The kernels of block inverse iteration with a fixed shift sigma and a Rayleigh-Ritz step.  K = (kdiag[ne+1], koff[ne])
 * are the bands of lssvr_p1_assemble_react with c_quad = c, M = (mdiag, moff) those of the same entry with an a_quad of
 * zeros and c_quad = rho (the consistent mass matrix weighted by rho); one more call with c_quad = c - sigma rho gives
 * the bands of the shifted solve Z = (K - sigma M)^-1 Y, which is lssvr_tridiag_bc_solve_multi (c - sigma rho >= 0) or
 * lssvr_tridiag_pivot_solve_multi (any sigma) with nc = nb.  The bands are read only.  kind_left, kind_right and
 * kappa_host[2] as in lssvr_tridiag_pivot_solve_multi: a Robin end keeps its node as an unknown and adds kappa (finite,
 * either sign) to K's end diagonal by value; a Dirichlet end's node is no unknown.  Block vectors are DEVICE arrays
 * [nb][ne+1], 1 <= nb <= 8, the layout of the multi solvers; rows outside the unknowns are written as exactly 0 and are
 * not read.  ne == 0 succeeds and launches nothing.  Every reduction runs in a fixed order -- lanes of a wave, waves of
 * a workgroup, workgroups in index order by one finishing workgroup --, no atomics: bitwise reproducible.
 *
 * lssvr_eig_apply -- MZ = M Z, KZ = K Z and gram[2*nb*nb] = {A = Z^T K Z, B = Z^T M Z}, two full symmetric row-major
 * matrices.  The vector outputs of case j do not depend on nb, bit for bit.  work: device scratch of
 * work_bytes >= lssvr_eig_work_bytes(ne, nb).
 *
 * lssvr_eig_ritz -- the nb x nb pencil (A, B), device arrays (gram and gram + nb*nb): theta[nb] ascending in
 * |theta - sigma| (ties by index) and Q[nb*nb] row-major, column j the vector of theta[j], with Q^T A Q = diag theta and
 * Q^T B Q = I.  Cholesky of B, C = L^-1 A L^-T, cyclic Jacobi (at most 20 sweeps), Q = L^-T V; one thread.  info (device
 * int32, may be NULL): the number of dependent columns of B -- a Cholesky pivot at or below 2^-46 of B's diagonal entry.
 * Such a column is replaced by zeros (nothing is divided by the pivot), its theta is 0 and it is ordered last.
 * lssvr_eig_ritz_host -- the same routine on HOST arrays (info too), bit for bit: no device is touched.
 *
 * lssvr_eig_rotate -- X = Z Q, Y = (MZ) Q and res2[2*nb] = {|(KZ) Q_j - theta_j (MZ) Q_j|_2^2, j < nb; |X_j|_2^2, j < nb}.
 * Column j of X and Y is signed so that X's value at the first unknown is >= 0.  Q and theta are device arrays, as
 * lssvr_eig_ritz leaves them.  X and Y must not overlap Z, MZ or KZ.  work as in lssvr_eig_apply.
 *
 * lssvr_eig_count -- counts[t] (device int32[ns]) = the number of negative pivots of LDL^T (K - shifts[t] M) over the
 * unknowns, d_i = alpha_i - beta_{i-1}^2 / d_{i-1}, a pivot with |d| < pivmin taken as -pivmin (LAPACK dstebz): the
 * number of eigenvalues of the pencil below shifts[t] (Sylvester).  shifts: device double[ns]; pivmin > 0, typically
 * DBL_MIN * max(1, max beta^2).  One lane per shift, serial over the rows: not for the inner loop.
 * lssvr_eig_count_host -- the same on HOST arrays (counts too), bit for bit.
 *
 * lssvr_eig_rayleigh -- for an enhanced mode W[ne][M] (1 <= M <= 33; zero-padded rows of mixed degree are fine) and
 * a_values, c_values, rho_values at lssvr_estimate_points (1 <= nq <= 32; table_layout as in lssvr_estimate_react):
 *   out3[0] = sum_e int_e (a u_e'^2 + c u_e^2) dx + sum over the Robin ends of kappa u_e(x_end)^2,
 *   out3[1] = sum_e int_e rho u_e^2 dx,     out3[2] = the sum of the absolute values of the terms of out3[0],
 * so that out3[0] / out3[1] is the Rayleigh quotient and out3[2] the scale of its rounding.  work: device scratch of
 * lssvr_eig_work_bytes(ne, 1) bytes (not checkable here: no size argument).
 */
int64_t lssvr_eig_work_bytes(int64_t ne, int nb);
int lssvr_eig_apply(const double* kdiag, const double* koff, const double* mdiag, const double* moff,
                    int kind_left, int kind_right, const double* kappa_host, int64_t ne, int nb,
                    const double* Z, double* MZ, double* KZ, double* gram,
                    void* work, int64_t work_bytes, void* stream);
int lssvr_eig_ritz(const double* A, const double* B, int nb, double sigma, double* theta, double* Q, int32_t* info,
                   void* stream);
int lssvr_eig_ritz_host(const double* A_host, const double* B_host, int nb, double sigma, double* theta_host,
                        double* Q_host, int32_t* info);
int lssvr_eig_rotate(const double* Z, const double* MZ, const double* KZ, const double* Q, const double* theta,
                     int kind_left, int kind_right, int64_t ne, int nb, double* X, double* Y, double* res2,
                     void* work, int64_t work_bytes, void* stream);
int lssvr_eig_count(const double* kdiag, const double* koff, const double* mdiag, const double* moff,
                    int kind_left, int kind_right, const double* kappa_host, int64_t ne,
                    const double* shifts, int ns, double pivmin, int32_t* counts, void* stream);
int lssvr_eig_count_host(const double* kdiag_host, const double* koff_host, const double* mdiag_host,
                         const double* moff_host, int kind_left, int kind_right, const double* kappa_host, int64_t ne,
                         const double* shifts_host, int ns, double pivmin, int32_t* counts);
int lssvr_eig_rayleigh(const double* x, const double* W, int64_t ne, int M, int nq,
                       const double* a_values, const double* c_values, const double* rho_values, int table_layout,
                       int kind_left, int kind_right, const double* kappa_host,
                       double* out3, void* work, void* stream);

/*
 * Transient problems: rho u_t - (a u')' + c u = f(x, t), rho > 0, BDF1 / BDF2 with a fixed step dt (no reference
 * counterpart).  ADDITIVE to ABI 7: four new symbols, no existing entry, struct, constant or
 * kernel changes, LSSVR_ABI_VERSION stays 7.
 *
 * Step n+1 solves  A_alpha u^{n+1} = (1/dt) M (beta0 u^n + beta1 u^{n-1}) + load(t_{n+1})  with alpha, (beta0, beta1)
 * = 1, (1, 0) for BDF1 and 3/2, (2, -1/2) for BDF2.  M = (mdiag[ne+1], moff[ne]) are the bands of
 * lssvr_p1_assemble_react with an a_quad of zeros and c_quad = rho, A_alpha those of the same entry with
 * c_quad = c + alpha rho / dt; the solve is lssvr_tridiag_bc_solve_multi, whose end_values of the step (g(t_{n+1}) per
 * end) are a device row.  The forcing is separable, f(x, t) = sum_{r<R} phi_r(t) f_r(x), 1 <= R <= 8: the R loads come
 * from lssvr_p1_load_multi once, and phi of every step lives in a device table.  Nothing here synchronises or copies:
 * a time loop is launches on one stream.  No reduction, no atomics: bitwise reproducible.
 *
 * lssvr_ts_rhs -- out[j*(ne+1) + i] = inv_dt (M (beta0 U0[j] + beta1 U1[j]))_i + sum_r phi[j*R + r] loads[r*(ne+1) + i]
 * for the nc cases (1 <= nc <= 8) U0, U1, out [nc][ne+1], loads [R][ne+1] shared by the cases, phi [nc][R], all DEVICE
 * arrays; ne >= 1.  beta1 == 0 does not read U1 (may be NULL).  Rows 0 and ne are the natural end rows (the full mass
 * row of the end node); the solvers ignore them at a Dirichlet end.  out must not be U0 or U1.  The order of the sums:
 * v = beta0 U0 + beta1 U1;  m = (moff[i-1] v[i-1] + mdiag[i] v[i]) + moff[i] v[i+1];  then inv_dt m, plus the terms
 * phi[r] loads[r] one by one, r ascending.
 *
 * lssvr_ts_source_table -- for one snapshot, the right-hand-side table of its elliptic enhancement problem
 * -(a u')' + c u = f(., t) - rho I_h w, in either LSSVR_TABLE_* layout:
 *   out(e, k) = sum_r phi[r] ftab[r](e, k) - rho_tab(e, k) (w_e + (w_{e+1} - w_e) (k / (n_colloc - 1))),
 *   w_i = inv_dt ((alpha U2_i - beta0 U0_i) - beta1 U1_i)      (the nodal BDF difference of u^{n+1} = U2),
 * with ftab [R] tables and rho_tab one table of ne * n_colloc doubles at lssvr_colloc_points(_pm), phi [R], U2, U0, U1
 * [ne+1], all DEVICE arrays; 2 <= n_colloc <= 4096.  beta1 == 0 does not read U1 (may be NULL).  The sum over r runs
 * r ascending.
 *
 * lssvr_ts_rhs_host, lssvr_ts_source_table_host -- the same routines on HOST arrays, bit for bit: no device is touched.
 */
int lssvr_ts_rhs(const double* mdiag, const double* moff, const double* U0, const double* U1, const double* loads,
                 const double* phi, int64_t ne, int nc, int R, double beta0, double beta1, double inv_dt,
                 double* out, void* stream);
int lssvr_ts_rhs_host(const double* mdiag_host, const double* moff_host, const double* U0_host, const double* U1_host,
                      const double* loads_host, const double* phi_host, int64_t ne, int nc, int R, double beta0,
                      double beta1, double inv_dt, double* out_host);
int lssvr_ts_source_table(const double* U2, const double* U0, const double* U1, const double* ftab,
                          const double* rho_tab, const double* phi, int64_t ne, int n_colloc, int R, int table_layout,
                          double alpha, double beta0, double beta1, double inv_dt, double* out, void* stream);
int lssvr_ts_source_table_host(const double* U2_host, const double* U0_host, const double* U1_host,
                               const double* ftab_host, const double* rho_tab_host, const double* phi_host, int64_t ne,
                               int n_colloc, int R, int table_layout, double alpha, double beta0, double beta1,
                               double inv_dt, double* out_host);

/*
 * Adaptive time stepping for the transient problem above: variable-step BDF2 with a local error estimate (no reference
 * counterpart).  ADDITIVE to ABI 7: five new symbols, no existing entry, struct, constant or
 * kernel changes, LSSVR_ABI_VERSION stays 7.
 *
 * With h the trial step, h_p the last accepted one and omega = h / h_p, an attempt solves
 *   (K + s M) u^{n+1} = (1/h) M (beta0 u^n + beta1 u^{n-1}) + load(t_{n+1}),     s = alpha / h,
 *   alpha = (1 + 2 omega) / (1 + omega),  beta0 = 1 + omega,  beta1 = -omega^2 / (1 + omega)
 * (1, 1, 0 for the first step), K = (kdiag[ne+1], koff[ne]) the bands of lssvr_p1_assemble_react with c_quad = c and
 * M = (mdiag, moff) those of the same entry with an a_quad of zeros and c_quad = rho: both are assembled once, and the
 * solve is lssvr_tridiag_bc_solve_multi on (adiag, aoff).  The host owns the controller: it reads out4 after every
 * attempt.  No atomics: bitwise reproducible.
 *
 * lssvr_ts_step -- one pass over the nodes, one case:
 *   adiag[i] = kdiag[i] + s mdiag[i] (i <= ne),  aoff[i] = koff[i] + s moff[i] (i < ne)      the product first;
 *   b[i]     = the value lssvr_ts_rhs writes for nc = 1 from (mdiag, moff, U0, U1, loads, phi, R, beta0, beta1, inv_dt),
 *              by the same routine, bit for bit.
 * write_bands = 0 skips the two band writes (s is the previous attempt's; kdiag, koff, adiag, aoff are not touched and
 * may be NULL), write_bands = 1 makes them.  All arrays are DEVICE arrays; no output may be an input.  Return codes:
 * ne < 1, R outside [1, 8], a scalar that is not finite, write_bands other than 0 / 1, an array not aligned to 8 bytes
 * and aliased arguments are LSSVR_ERR_SIZE; a missing pointer is LSSVR_ERR_NULL.
 *
 * lssvr_ts_error -- out4 (DEVICE, four doubles) = { max_i |e_i| / sc_i, max_i |e_i|, max_i |U3_i|, the count of rows
 * whose e_i or sc_i is not finite } over the rows i = 0 .. ne except a LSSVR_END_DIRICHLET end row (its value is data):
 *   e_i  = ((w3 U3_i + w2 U2_i) + w1 U1_i) + w0 U0_i          w1 == 0 reads no U1, w0 == 0 reads no U0 (may be NULL)
 *   sc_i = atol + rtol max(|U3_i|, |U2_i|)                    max(x, y) = x > y ? x : y
 * U3 is the trial u^{n+1}, U2, U1, U0 the accepted u^n, u^{n-1}, u^{n-2}, all DEVICE arrays [ne+1]; the weights are those
 * of a divided difference with the estimate's scalar factor folded in, computed by the caller.  A counted row joins
 * neither of the first two maxima; |U3_i| joins the third when it is finite.  atol, rtol >= 0, atol + rtol > 0.
 * Per-workgroup partials go to work (DEVICE, work_bytes >= lssvr_ts_error_work_bytes(ne)), a second launch of one
 * workgroup merges them.  Return codes as above; bad end kinds are LSSVR_ERR_SIZE.
 *
 * lssvr_ts_step_host, lssvr_ts_error_host -- the same routines on HOST arrays, bit for bit: no device is touched.
 */
int lssvr_ts_step(const double* kdiag, const double* koff, const double* mdiag, const double* moff, const double* U0,
                  const double* U1, const double* loads, const double* phi, int64_t ne, int R, double s, double beta0,
                  double beta1, double inv_dt, int write_bands, double* adiag, double* aoff, double* b, void* stream);
int lssvr_ts_step_host(const double* kdiag_host, const double* koff_host, const double* mdiag_host,
                       const double* moff_host, const double* U0_host, const double* U1_host, const double* loads_host,
                       const double* phi_host, int64_t ne, int R, double s, double beta0, double beta1, double inv_dt,
                       int write_bands, double* adiag_host, double* aoff_host, double* b_host);
int64_t lssvr_ts_error_work_bytes(int64_t ne);
int lssvr_ts_error(const double* U3, const double* U2, const double* U1, const double* U0, int kind_left,
                   int kind_right, int64_t ne, double w3, double w2, double w1, double w0, double atol, double rtol,
                   double* out4, void* work, int64_t work_bytes, void* stream);
int lssvr_ts_error_host(const double* U3_host, const double* U2_host, const double* U1_host, const double* U0_host,
                        int kind_left, int kind_right, int64_t ne, double w3, double w2, double w1, double w0,
                        double atol, double rtol, double* out4_host);

/*
 * Semilinear problems: -(a u')' + b u' + c u + g(x, u) = f by a damped Newton iteration (no reference counterpart;
 * DESIGN.md section 27).  ADDITIVE to ABI 7: seven new symbols and two constants, no existing entry, struct, constant
 * or kernel changes, LSSVR_ABI_VERSION stays 7.
 *
 * One Newton step from the nodal iterate u is the LINEAR problem with the reaction c + g_u(x, u_h) and the right-hand
 * side f - g(x, u_h) + g_u(x, u_h) u_h, u_h the P1 interpolant of u, solved for the new iterate itself: lssvr_nl_linearize
 * at the quadrature points writes those two tables, lssvr_p1_assemble_react / _conv assembles them and any of the
 * lssvr_tridiag_*_solve_multi entries solves, with the boundary conditions of the linear problem.  The merit function
 * is |R(v)|_inf, R(v) = K v + G(v) - F with K the bands of a, b, c: lssvr_nl_linearize (f_res only), lssvr_p1_load_multi
 * (one case) and lssvr_nl_residual.  Nothing here synchronises or copies; no atomics: bitwise reproducible.
 *
 * g comes from a tabulated family, q_tabs = [nterm] tables stacked, each of ne * n doubles in the layout of the call:
 *   LSSVR_NL_POLY  g(x, u) = sum_{k < nterm} q_k(x) u^k, 1 <= nterm <= 6.  With K = nterm - 1, by Horner:
 *                  g = q_K, then g = g u + q_k for k = K-1 .. 0;  g_u: d = (double)K q_K, then d = d u + (double)k q_k
 *                  for k = K-1 .. 1;  nterm = 1: g_u = 0.
 *   LSSVR_NL_EXP   g(x, u) = q_0(x) exp(q_1(x) u), nterm = 2:  E = exp(q_1 u), g = q_0 E, g_u = (q_0 q_1) E.
 *
 * lssvr_nl_linearize -- for the n points (1 <= n <= 64) of every element, a thread per table entry (e, k) in memory
 * order, either LSSVR_TABLE_* layout:
 *   u_h = u_e + (u_{e+1} - u_e) t_local[k],
 *   c_eff(e, k) = c + g_u,   f_eff(e, k) = (f - g) + g_u u_h,   f_res(e, k) = f - g,
 * g and g_u at (point, u_h) as above.  u [ne+1], t_local [n] (the local coordinates in [0, 1] of the points: the rule
 * of lssvr_quad_points, k / (n - 1) for lssvr_colloc_points(_pm), the Gauss points of lssvr_estimate_points), q_tabs,
 * c_tab (NULL: c = 0) and f_tab are DEVICE arrays; an output that is NULL is not written, at least one must be given.
 * No output may alias an input.  Return codes: an unknown kind is LSSVR_ERR_RHS (the family of g is data of the
 * right-hand side, like rhs_id); nterm outside the kind's range, n outside [1, 64], ne < 1, an unknown table_layout and
 * aliased arguments are LSSVR_ERR_SIZE; a missing pointer, or no output at all, is LSSVR_ERR_NULL.
 *
 * lssvr_nl_residual -- out4 (DEVICE, four doubles) = { max_i |r_i|, max_i |u_new_i - u_i|, max_i |u_new_i|, the count of
 * entries among the 3 (ne + 1) that are not finite } for the bands diag [ne+1], sub [ne], sup [ne] of the linear
 * operator (a symmetric caller passes off twice), load = F - G(u) [ne+1], u and u_new [ne+1]:
 *   r_i = ((sub[i-1] u[i-1] + diag[i] u[i]) + sup[i] u[i+1]) - load[i]     (rows 0 and ne: the term of the missing
 *   neighbour is left out);  at a LSSVR_END_ROBIN end  r_i = r_i + (kappa u_i - g),  g = end_values[end] (DEVICE array
 * of two doubles; may be NULL with two Dirichlet ends);  at a LSSVR_END_DIRICHLET end  r_i = 0.  kappa_host[2]: host
 * array, finite, either sign.  An entry that is not finite raises the count and joins no maximum.  Per-workgroup
 * partials go to work (DEVICE, work_bytes >= lssvr_nl_residual_work_bytes(ne)), a second launch of one workgroup
 * merges them: a maximum of finite numbers does not depend on the order, and the count is a sum of integers in a fixed
 * tree, so out4 is bitwise reproducible.
 *
 * lssvr_nl_step -- out_i = u_i + lambda (u_new_i - u_i), i = 0 .. ne, lambda finite; u, u_new and out are DEVICE arrays [ne+1], and
 * out must be neither u nor u_new.
 *
 * lssvr_nl_linearize_host, lssvr_nl_residual_host, lssvr_nl_step_host -- the same routines on HOST arrays: no device
 * is touched.  Bit for bit the device's values, except that exp of LSSVR_NL_EXP is the host's libm there.
 */
#define LSSVR_NL_POLY 0
#define LSSVR_NL_EXP 1
int lssvr_nl_linearize(const double* u, const double* t_local, const double* q_tabs, const double* c_tab,
                       const double* f_tab, int64_t ne, int n, int table_layout, int kind, int nterm,
                       double* c_eff, double* f_eff, double* f_res, void* stream);
int lssvr_nl_linearize_host(const double* u_host, const double* t_local_host, const double* q_tabs_host,
                            const double* c_tab_host, const double* f_tab_host, int64_t ne, int n, int table_layout,
                            int kind, int nterm, double* c_eff_host, double* f_eff_host, double* f_res_host);
int64_t lssvr_nl_residual_work_bytes(int64_t ne);
int lssvr_nl_residual(const double* diag, const double* sub, const double* sup, const double* load, const double* u,
                      const double* u_new, int kind_left, int kind_right, const double* end_values,
                      const double* kappa_host, int64_t ne, double* out4, void* work, int64_t work_bytes,
                      void* stream);
int lssvr_nl_residual_host(const double* diag_host, const double* sub_host, const double* sup_host,
                           const double* load_host, const double* u_host, const double* u_new_host, int kind_left,
                           int kind_right, const double* end_values_host, const double* kappa_host, int64_t ne,
                           double* out4_host);
int lssvr_nl_step(const double* u, const double* u_new, double lambda, int64_t ne, double* out, void* stream);
int lssvr_nl_step_host(const double* u_host, const double* u_new_host, double lambda, int64_t ne, double* out_host);

/*
 * Semilinear transient problems: rho u_t - (a u')' + c u + g(x, u) = f(x, t), BDF1 / BDF2 with a fixed step and a fixed
 * number of Newton iterations per step (no reference counterpart).  ADDITIVE to ABI 7: two new
 * symbols, no existing entry, struct or constant changes, LSSVR_ABI_VERSION stays 7.
 *
 * Step n+1 solves  (alpha / dt) M v + K v + G(v) = r  for v = u^{n+1}, r the vector lssvr_ts_rhs writes (once per
 * step).  The Newton iterate v_k -> v_{k+1} is the LINEAR problem with the reaction cs + g_u(x, v_k,h),
 * cs = c + alpha rho / dt, and the right-hand side r + L(-g + g_u v_k,h), v_k,h the P1 interpolant of v_k and L the P1
 * load assembly, solved for v_{k+1} itself by lssvr_tridiag_bc_solve_multi with the end values g(t_{n+1}) of the step.
 * lssvr_nl_residual on the iteration's own bands and right-hand side with u = v_k, u_new = v_{k+1} is the monitor: its
 * first number is the nonlinear residual at v_k (M(g_u) v_k = L(g_u v_k,h) under one quadrature), its second the
 * increment.  The start is lssvr_nl_step(u^{n-1}, u^n, 2) for BDF2 and u^n otherwise.  Nothing here synchronises or
 * copies: a time loop is launches on one stream.
 *
 * lssvr_ts_nl_assemble -- the bands diag [ne+1], off [ne] and the right-hand side rhs [ne+1] of one Newton iteration
 * in ONE launch: what lssvr_nl_linearize (f_tab = 0, c_tab = cs_quad) -> lssvr_p1_assemble_react -> r + load gives, bit
 * for bit, without its two [ne][nquad] tables.  x, u, r [ne+1]; a_quad (NULL: a = 1), cs_quad and the nterm tables
 * q_quad are [ne][nquad], element-major, at lssvr_quad_points; kind / nterm as for lssvr_nl_linearize; all DEVICE
 * arrays.  One thread per node gathers its right and its left element; no atomics: bitwise reproducible.  Per
 * quadrature point (xi, w) of an element of length h, idx = e nquad + k:
 *   u_h = u_e + (u_{e+1} - u_e) xi;  g, g_u as for lssvr_nl_linearize;  c_eff = cs + g_u;  f_eff = (0 - g) + g_u u_h;
 *   sl += (w (1 - xi)) f_eff;  sr += (w xi) f_eff;  am += w a;
 *   ll += (w c_eff) ((1 - xi)(1 - xi));  lr += (w c_eff) ((1 - xi) xi);  rr += (w c_eff) (xi xi);
 * then k = am / h (a_quad NULL: 1 / h), fl = h sl, fr = h sr, m_ll = h ll, m_lr = h lr, m_rr = h rr, and per node i
 *   d = 0;  d += k + m_ll (right element);  d += k + m_rr (left element);   l = 0;  l += fl (right);  l += fr (left);
 *   diag[i] = d;  off[i] = m_lr - k (right element);  rhs[i] = r[i] + l.
 * Return codes: an unknown kind is LSSVR_ERR_RHS; nterm outside the kind's range, ne < 1 and an output that is one of
 * the inputs or another output are LSSVR_ERR_SIZE; nquad outside [1, 5] is LSSVR_ERR_QUAD; a missing pointer is
 * LSSVR_ERR_NULL.
 *
 * lssvr_ts_nl_assemble_host -- the same routine on HOST arrays: no device is touched.  Bit for bit the device's values,
 * except that exp of LSSVR_NL_EXP is the host's libm there.
 */
int lssvr_ts_nl_assemble(const double* x, const double* u, const double* a_quad, const double* cs_quad,
                         const double* q_quad, const double* r, int64_t ne, int nquad, int kind, int nterm,
                         double* diag, double* off, double* rhs, void* stream);
int lssvr_ts_nl_assemble_host(const double* x_host, const double* u_host, const double* a_quad_host,
                              const double* cs_quad_host, const double* q_quad_host, const double* r_host, int64_t ne,
                              int nquad, int kind, int nterm, double* diag_host, double* off_host, double* rhs_host);

/*
 * Wave problems: rho u_tt + d u_t - (a u')' + c u = f(x, t), Newmark (beta, gamma) in displacement form with a fixed
 * step dt (no reference counterpart).  ADDITIVE to ABI 7: two new symbols, no existing entry,
 * struct, constant or kernel instantiation changes, LSSVR_ABI_VERSION stays 7.
 *
 * With the predictors  ut = u + dt v + dt^2 (1/2 - beta) acc,  vt = v + dt (1 - gamma) acc  step n+1 solves
 *   A u' = load(t_{n+1}) + M_rho (ut / (beta dt^2)) + M_d ((gamma / (beta dt)) ut - vt)
 * with A the bands of lssvr_p1_assemble_react for c_quad = c + rho / (beta dt^2) + gamma d / (beta dt) (assembled once),
 * M_rho = (mdiag, moff) and M_d = (ddiag, doff) those of the same entry with a_quad = 0 and c_quad = rho, d; the solve
 * is lssvr_tridiag_bc_solve_multi with a device row of end data.  The correctors are  acc' = (u' - ut) / (beta dt^2),
 * v' = vt + gamma dt acc'.
 *
 * lssvr_wave_advance -- ONE launch per step: the correctors of the step just solved and the right-hand side of the
 * next.  U_new, U, V, Acc, V_out, Acc_out, rhs_out are [nc][ne+1], case-major, 1 <= nc <= 8; loads [R][ne+1]
 * (1 <= R <= 8, shared by the cases) and phi [nc][R] as for lssvr_ts_rhs; ddiag == NULL means d = 0, and then
 * neither ddiag nor doff is read; all DEVICE arrays.  With  c_u2 = (dt dt)(1/2 - beta), c_v1 = dt (1 - gamma),
 * c_m = 1 / (beta (dt dt)), c_d = gamma / (beta dt), c_va = gamma dt  (computed once on the host), per entry:
 *   ut = (U + dt V) + c_u2 Acc;  vt = V + c_v1 Acc;  Acc_out = (U_new - ut) c_m;  V_out = vt + c_va Acc_out;
 * and from the NEW state (u, v, acc) = (U_new, V_out, Acc_out) at i-1, i, i+1:
 *   ut = (u + dt v) + c_u2 acc;  p = c_m ut;  q = c_d ut - (v + c_v1 acc);
 *   m  = (moff[i-1] p[i-1] + mdiag[i] p[i]) + moff[i] p[i+1];   dd likewise from (ddiag, doff) and q;
 *   rhs_out[i] = (((m + dd) + phi[0] loads[0][i]) + phi[1] loads[1][i]) + ...     (d = 0: m in place of m + dd)
 * Rows 0 and ne leave the missing neighbour's term out.  A thread recomputes its neighbours' correctors from the old
 * arrays by the routine that computes its own, so the launch needs no barrier and the fused call equals the split pair
 * bit for bit.  Modes:
 *   U_new == NULL    (U, V, Acc) is the state already, nothing but rhs_out is written (the first step's right-hand
 *                    side; V_out, Acc_out are not read and may be NULL);
 *   rhs_out == NULL  the correctors only (the last step, or the first half of a split pair; the bands, loads and phi
 *                    are not read and may be NULL).
 * No reduction, no atomics, no synchronisation, no copy.  Return codes: LSSVR_ERR_SIZE when both U_new and rhs_out
 * are NULL, when V_out or Acc_out is V, Acc, U, U_new or the other output, when rhs_out is an input or another output,
 * when ne < 1, nc or R is outside [1, 8], or dt, beta or gamma is not finite and > 0; LSSVR_ERR_NULL for a missing
 * pointer that the mode reads or writes.  Every check comes before any launch.
 *
 * lssvr_wave_advance_host -- the same routine on HOST arrays: no device is touched.  Bit for bit the device's values.
 */
int lssvr_wave_advance(const double* U_new, const double* U, const double* V, const double* Acc, const double* mdiag,
                       const double* moff, const double* ddiag, const double* doff, const double* loads,
                       const double* phi, int64_t ne, int nc, int R, double dt, double beta, double gamma,
                       double* V_out, double* Acc_out, double* rhs_out, void* stream);
int lssvr_wave_advance_host(const double* U_new_host, const double* U_host, const double* V_host,
                            const double* Acc_host, const double* mdiag_host, const double* moff_host,
                            const double* ddiag_host, const double* doff_host, const double* loads_host,
                            const double* phi_host, int64_t ne, int nc, int R, double dt, double beta, double gamma,
                            double* V_out_host, double* Acc_out_host, double* rhs_out_host);

/*
 * Adjoint sensitivities of the P1 solve of -(a u')' + b u' + c u = f (no reference counterpart).
 * ADDITIVE to ABI 7: two new symbols, no existing entry, struct, constant or kernel instantiation changes,
 * LSSVR_ABI_VERSION stays 7.
 *
 * For a functional J(u) with p = dJ/du (a nodal vector) the adjoint z solves the TRANSPOSED bands with load p: hand
 * (diag, sup, sub) to lssvr_tridiag_ns_bc_solve_multi or lssvr_tridiag_pivot_solve_multi where the primal solve took
 * (diag, sub, sup) -- symmetric bands are their own transpose --, with the primal's end kinds and kappa and with zero
 * end data, so z = 0 at a Dirichlet end.  With h_e = x[e+1] - x[e], (xi_q, w_q) the nquad-point Gauss rule on [0, 1],
 * du_e = u[e+1] - u[e], dz_e likewise, u_eq = u[e] (1 - xi_q) + u[e+1] xi_q and z_eq likewise:
 *   dJ/da_quad[e][q]   = -(w_q / h_e) dz_e du_e        dJ/db_quad[e][q]   = -w_q z_eq du_e
 *   dJ/dc_quad[e][q]   = -h_e w_q z_eq u_eq            dJ/drhs_quad[e][q] = +h_e w_q z_eq
 *   Dirichlet end:  dJ/dg_0 = p_0 - sub[0] z_1,  dJ/dg_ne = p_ne - sup[ne-1] z_{ne-1},  dJ/dkappa = 0
 *   Robin end:      dJ/dg = z_end,  dJ/dkappa = -z_end u_end
 * (sub, sup: the bands as lssvr_p1_assemble_conv wrote them; for symmetric bands both are `off`).
 *
 * lssvr_p1_sensitivity -- ONE launch for nc pairs (U[j], Z[j]), 1 <= nc <= 8: x [ne+1], Z [nc][ne+1] case-major,
 * U [nu][ne+1] with nu == nc, or nu == 1 for one primal solution shared by all cases (several functionals: rows of a
 * Jacobian); all DEVICE arrays.  ga, gb, gc, gf receive the four gradients, each [nc][ne*nquad] in the layout of the
 * input tables; a NULL one is skipped, stores included, and at least one must be given.  NONE of the tables a_quad,
 * b_quad, c_quad, rhs_quad is an argument: given u and z the gradient does not depend on them.  out_ends [nc][4]
 * (may be NULL) receives (dJ/dg_0, dJ/dg_ne, dJ/dkappa_0, dJ/dkappa_ne) per case, written by the same launch; it needs
 * band_ends = {sub[0], sup[ne-1]} (device, 2 doubles) and the end kinds, and reads P [nc][ne+1] = dJ/du at a Dirichlet
 * end (NULL: taken as zero).  Without out_ends neither P, band_ends nor the kinds are read.  The order of every
 * operation is fixed (csrc/lssvr_sens.hpp), one thread per table entry, no reduction, no atomics, no synchronisation,
 * no copy.  No output may be one of the inputs or another output.
 * Return codes, each before any HIP call: LSSVR_ERR_SIZE for ne < 1, nc outside [1, 8], nu other than 1 or nc, or an
 * unknown end kind with out_ends; LSSVR_ERR_QUAD for nquad outside [1, 5]; LSSVR_ERR_NULL for a missing x, U or Z, for
 * four NULL outputs, and for out_ends without band_ends.
 *
 * lssvr_p1_sensitivity_host -- the same routines on HOST arrays: no device is touched.  Bit for bit the device's values.
 */
int lssvr_p1_sensitivity(const double* x, int64_t ne, int nquad, const double* U, int nu, const double* Z, int nc,
                         double* ga, double* gb, double* gc, double* gf, const double* P, const double* band_ends,
                         int kind_left, int kind_right, double* out_ends, void* stream);
int lssvr_p1_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* U_host, int nu,
                              const double* Z_host, int nc, double* ga_host, double* gb_host, double* gc_host,
                              double* gf_host, const double* P_host, const double* band_ends_host, int kind_left,
                              int kind_right, double* out_ends_host);

/*
 * Adjoint sensitivities of the BDF loop of rho u_t - (a u')' + c u = f(x, t) (no reference counterpart; DESIGN.md section
 * 32).  ADDITIVE to ABI 7: two new symbols, no existing entry, struct, constant or kernel instantiation changes,
 * LSSVR_ABI_VERSION stays 7.
 *
 * The forward loop is that of lssvr_ts_rhs: step n = 1 .. N solves A_n u^n = (1/dt) M (beta0_n u^{n-1} + beta1_n u^{n-2})
 * + sum_r phi_r(t_n) L_r + end terms with A_n = K + (alpha_n/dt) M.  For J = sum_n p_n . u^n the adjoint states run
 * backwards, lambda^{N+1} = lambda^{N+2} = 0:
 *   B_n = p_n + (1/dt) M (beta0_{n+1} lambda^{n+1} + beta1_{n+2} lambda^{n+2})      -- lssvr_ts_rhs with U0 = lambda^{n+1},
 *                                                   U1 = lambda^{n+2}, loads = the row p_n, phi = 1
 *   A_n lambda^n = B_n, the forward loop's end kinds and kappa, zero end data      -- lssvr_tridiag_bc_solve_multi
 * (K and M are symmetric: no transposition).  This entry turns a CHUNK of m <= 8 consecutive adjoint steps
 * n0 .. n0+m-1 into gradients, summed over the chunk.  With the notation of lssvr_p1_sensitivity and w^n = (alpha_n u^n -
 * beta0_n u^{n-1} - beta1_n u^{n-2}) / dt, the nodal BDF difference of lssvr_ts_source_table:
 *   dJ/da_quad[e][q]   = -sum_n (w_q / h_e) dlambda^n_e du^n_e      dJ/dc_quad[e][q]      = -sum_n h_e w_q lambda^n_eq u^n_eq
 *   dJ/drho_quad[e][q] = -sum_n h_e w_q lambda^n_eq w^n_eq          dJ/df_quad[r][e][q]   = +sum_n phi_r(t_n) h_e w_q lambda^n_eq
 *   Dirichlet end:  dJ/dg(t_n) = B_n[end] - aoff_n[end] lambda^n[inner],  dJ/dkappa = 0
 *   Robin end:      dJ/dg(t_n) = lambda^n[end],                           dJ/dkappa = -sum_n lambda^n[end] u^n[end]
 * (dJ/du0 and dJ/dg(t_0) are rows of B_0, one more lssvr_ts_rhs: no kernel.)
 *
 * lssvr_transient_sensitivity -- ONE launch per chunk.  DEVICE arrays: x [ne+1]; Utraj [N+1][ne+1], the whole stored trajectory
 * (row n = u^n; rows max(n0-2, 0) .. n0+m-1 are read, u^{-1} counts as 0); Z [m][ne+1] and Brows [m][ne+1], the adjoint
 * states of the chunk and their right-hand sides IN THE ORDER OF THE SWEEP: row i belongs to step n0+m-1-i; phi [N][R],
 * the whole table the forward loop fed lssvr_ts_rhs from (row n-1 = phi(t_n); read for gf only), 0 <= R <= 8, R = 0
 * only with gf NULL.  coef_host: a HOST array [m][3], (alpha_n, beta0_n, beta1_n) of step row i, copied into the launch's
 * arguments.  ga, gc, grho [ne*nquad] and gf [R][ne*nquad] receive the gradients in the layout of the input tables; a
 * NULL one is skipped, stores included.  accumulate = 0: every sum starts from 0 (the first chunk of a sweep needs no
 * memset); 1: it continues from what the output holds, so a sweep gives the same bits however it is cut into chunks.
 * out_g [N+1][2] and out_kappa [2] (both or neither) receive the end gradients, written by the same launch: rows
 * n0 .. n0+m-1 of out_g, and out_kappa under the same accumulate flag; they need Brows, the end kinds, band_ends [2][2]
 * = {sub[0], sup[ne-1]} of two step matrices (device; one per alpha) and band_mask, whose bit i says which of the two
 * is the matrix of step row i.  Without out_g none of these is read, and the four tables may then all be NULL only if
 * out_g is given.  The order of every operation is fixed (csrc/lssvr_chunk_sens.hpp: one routine for this entry and
 * lssvr_newmark_sensitivity, which differ in the scheme it is instantiated with), one thread per table entry, no
 * reduction, no atomics, no synchronisation, no copy.  No output may be one of the inputs or another output.
 * Return codes, each before any HIP call: LSSVR_ERR_SIZE for ne < 1, m outside [1, 8], n0 < 1, R outside [0, 8], R = 0
 * with gf, a band_mask with bits beyond m, an unknown end kind with out_g, or an output that is an input or another
 * output; LSSVR_ERR_QUAD for nquad outside [1, 5]; LSSVR_ERR_NULL for a missing x, Utraj, Z or coef_host, for no output at all, for gf without phi, for one of out_g and
 * out_kappa without the other, and for out_g without Brows or band_ends.
 *
 * lssvr_transient_sensitivity_host -- the same routines on HOST arrays: no device is touched.  Bit for bit the device's values.
 */
int lssvr_transient_sensitivity(const double* x, int64_t ne, int nquad, const double* Utraj, const double* Z,
                                int64_t n0, int m, double inv_dt, const double* coef_host, const double* phi, int R,
                                double* ga, double* gc, double* grho, double* gf, int accumulate, const double* Brows,
                                const double* band_ends, int band_mask, int kind_left, int kind_right, double* out_g,
                                double* out_kappa, void* stream);
int lssvr_transient_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* Utraj_host,
                                     const double* Z_host, int64_t n0, int m, double inv_dt, const double* coef_host,
                                     const double* phi_host, int R, double* ga_host, double* gc_host,
                                     double* grho_host, double* gf_host, int accumulate, const double* Brows_host,
                                     const double* band_ends_host, int band_mask, int kind_left, int kind_right,
                                     double* out_g_host, double* out_kappa_host);

/*
 * Adjoint sensitivities of the Newmark loop of rho u_tt + d u_t - (a u')' + c u = f(x, t) (no reference counterpart;
 * DESIGN.md section 34).  ADDITIVE to ABI 7: four new symbols, no existing entry, struct, constant or kernel
 * instantiation changes, LSSVR_ABI_VERSION stays 7.
 *
 * The forward loop is that of lssvr_wave_advance, n = 0 .. N-1, with the scalars c_u2 = dt^2 (1/2 - beta),
 * c_v1 = dt (1 - gamma), c_m = 1 / (beta dt^2), c_d = gamma / (beta dt), c_va = gamma dt:
 *   ut = u^n + dt v^n + c_u2 acc^n;   vt = v^n + c_v1 acc^n
 *   A u^{n+1} = sum_r phi_r(t_{n+1}) L_r + M_rho (c_m ut) + M_d (c_d ut - vt) + end terms,   A = K + c_m M_rho + c_d M_d
 *   acc^{n+1} = c_m (u^{n+1} - ut);   v^{n+1} = vt + c_va acc^{n+1}
 * and M_rho acc^0 = load(0) - M_d v^0 - K u^0.  For J = sum_{n=0..N} p_n . u^n the backward sweep carries the bars (ubar,
 * vbar, abar) of the state of level n+1 (at level N: ubar = p_N, vbar = abar = 0); for n+1 = N .. 1
 *   B_{n+1} = ubar + c_m (abar + c_va vbar)
 *   A lambda^{n+1} = B_{n+1}, the forward loop's end kinds and kappa, zero end data      -- lssvr_tridiag_bc_solve_multi
 *   y = M_rho lambda^{n+1},  z = M_d lambda^{n+1}                                       (all rows)
 *   ut_bar = c_m y + c_d z - c_m (abar + c_va vbar);   vt_bar = vbar - z
 *   ubar <- p_n + ut_bar;   vbar <- dt ut_bar + vt_bar;   abar <- c_u2 ut_bar + c_v1 vt_bar   (the bars of level n)
 * and at level 0  M_rho lambda^0 = abar (a Robin end: a natural row),  dJ/du0 = ubar - K lambda^0,
 * dJ/dv0 = vbar - M_d lambda^0 (lssvr_eig_apply with both ends as Robin rows).
 *
 * lssvr_newmark_adjoint_advance -- ONE launch between two backward solves, one thread per node, nodal DEVICE arrays
 * [ne+1]: from lam = lambda^{n+1}, (Vbar, Abar) of level n+1, the row P = p_n (NULL: zero), the mass bands
 * (mdiag [ne+1], moff [ne]) and the damping bands (ddiag, doff; both NULL: d = 0) it writes (V_out, A_out), the bars of
 * level n, U_out = ubar of level n (NULL: skipped; the last call of a sweep asks for it) and B_out = B_n, the next
 * right-hand side (NULL: skipped).  lam NULL is the first call of a sweep: B_out = P + c_m (Abar + c_va Vbar) alone, no
 * bands are read and V_out, A_out, U_out must be NULL.  lam is an input, so no thread reads what another writes; no
 * output may be one of the inputs or another output.  The order of every sum is fixed (csrc/lssvr_newmark_adj.hpp); at
 * rows 0 and ne the missing neighbour's term is left out.  Return codes, each before any HIP call: LSSVR_ERR_SIZE for
 * ne < 1, for dt, beta or gamma not finite and > 0, for V_out, A_out or U_out without lam, and for an output that is
 * an input or another output; LSSVR_ERR_NULL for a missing Vbar or Abar, B_out missing without lam, mdiag, moff, V_out
 * or A_out missing with lam, and one of ddiag, doff without the other.
 *
 * lssvr_newmark_sensitivity -- ONE launch per chunk of m <= 8 consecutive levels n0 .. n0+m-1, n0 >= 0, summed over the
 * chunk.  With the notation of lssvr_p1_sensitivity:
 *   dJ/da_quad[e][q]   = -sum_n (w_q / h_e) dlambda^n_e du^n_e      dJ/dc_quad[e][q]   = -sum_n h_e w_q lambda^n_eq u^n_eq
 *   dJ/drho_quad[e][q] = -sum_n h_e w_q lambda^n_eq acc^n_eq        dJ/dd_quad[e][q]   = -sum_n h_e w_q lambda^n_eq v^n_eq
 *   dJ/df_quad[r][e][q] = +sum_n phi_r(t_n) h_e w_q lambda^n_eq
 *   Dirichlet end:  dJ/dg(t_n) = B_n[end] - off[end] lambda^n[inner]       Robin end:  dJ/dg(t_n) = lambda^n[end],
 *                                                                          dJ/dkappa = -sum_n lambda^n[end] u^n[end]
 * DEVICE arrays: x [ne+1]; Utraj, Vtraj, Atraj [N+1][ne+1], the stored trajectories, whole (row n = u^n, v^n, acc^n);
 * Vtraj is read for gd only and Atraj for grho only, either may be NULL then; Z [m][ne+1] and Brows [m][ne+1], the
 * adjoint states of the chunk and the right-hand sides of their solves IN THE ORDER OF THE SWEEP: row i belongs to
 * level n0+m-1-i; phi [N+1][R] (row n = phi(t_n); read for gf only), 0 <= R <= 8, R = 0 only with gf NULL.  ga, gc,
 * grho, gd [ne*nquad] and gf [R][ne*nquad] receive the gradients in the layout of the input tables; a NULL one is
 * skipped, stores included.  accumulate = 0: every sum starts from 0; 1: it continues from what the output holds, so
 * a sweep gives the same bits however it is cut into chunks.  out_g [N+1][2] and out_kappa [2] (both or neither)
 * receive the end gradients, written by the first thread of the same launch: rows n0 .. n0+m-1 of out_g, and out_kappa
 * under the same accumulate flag; they need Brows, the end kinds and band_ends [2] = {sub[0], sup[ne-1]} of the matrix
 * of the chunk's solves (device).  Level 0 is a chunk of its own: its matrix is M_rho, and what a Dirichlet end's entry
 * of out_g row 0 then holds is dJ/d(acc^0_end).  The order of every operation is fixed (csrc/lssvr_chunk_sens.hpp),
 * one thread per table entry, no reduction, no atomics, no synchronisation, no copy.  Return codes, each before any HIP call: LSSVR_ERR_SIZE for ne < 1, m outside [1, 8],
 * n0 < 0, R outside [0, 8], R = 0 with gf, an unknown end kind with out_g, or an output that is an input or another
 * output; LSSVR_ERR_QUAD for nquad outside [1, 5]; LSSVR_ERR_NULL for a missing x, Utraj or Z, for no output at all,
 * for gf without phi, gd without Vtraj, grho without Atraj, one of out_g and out_kappa without the other, and out_g
 * without Brows or band_ends.
 *
 * The _host entries run the same routines on HOST arrays: no device is touched.  Bit for bit the device's values.
 */
int lssvr_newmark_adjoint_advance(const double* lam, const double* Vbar, const double* Abar, const double* P,
                                  const double* mdiag, const double* moff, const double* ddiag, const double* doff,
                                  int64_t ne, double dt, double beta, double gamma, double* V_out, double* A_out,
                                  double* U_out, double* B_out, void* stream);
int lssvr_newmark_adjoint_advance_host(const double* lam_host, const double* Vbar_host, const double* Abar_host,
                                       const double* P_host, const double* mdiag_host, const double* moff_host,
                                       const double* ddiag_host, const double* doff_host, int64_t ne, double dt,
                                       double beta, double gamma, double* V_out_host, double* A_out_host,
                                       double* U_out_host, double* B_out_host);
int lssvr_newmark_sensitivity(const double* x, int64_t ne, int nquad, const double* Utraj, const double* Vtraj,
                              const double* Atraj, const double* Z, int64_t n0, int m, const double* phi, int R,
                              double* ga, double* gc, double* grho, double* gd, double* gf, int accumulate,
                              const double* Brows, const double* band_ends, int kind_left, int kind_right,
                              double* out_g, double* out_kappa, void* stream);
int lssvr_newmark_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* Utraj_host,
                                   const double* Vtraj_host, const double* Atraj_host, const double* Z_host, int64_t n0,
                                   int m, const double* phi_host, int R, double* ga_host, double* gc_host,
                                   double* grho_host, double* gd_host, double* gf_host, int accumulate,
                                   const double* Brows_host, const double* band_ends_host, int kind_left,
                                   int kind_right, double* out_g_host, double* out_kappa_host);

/*
 * Adjoint of the element solve: sensitivities of the ENHANCEMENT (no reference counterpart).
 * ADDITIVE to ABI 7: three new symbols, no existing entry, struct, constant or kernel instantiation changes,
 * LSSVR_ABI_VERSION stays 7.
 *
 * The forward calls (lssvr_enhance_varcoef, lssvr_enhance_react and their _ws forms, element-major tables, primal
 * solve) map the nodal values, the Dirichlet values and the collocation tables a, da (which may hold a' - b), c, f to
 * the coefficients W [ne][M].  For a functional J with Wbar = dJ/dW this entry returns dJ/d(every one of them).  In the
 * notation of the per-element solve (scl = 2/h, Ahat = -a D2 - (da/scl) D1 + (c/scl^2) L, eps = 1/(gamma scl^4),
 * C = B1^-1 B2, S = Abar^T Abar + eps (I + C^T C)), per element:
 *   y  = S^-1 (Wbar_2 - C^T Wbar_1)        one solve with the forward matrix
 *   yh = (-C y, y),   q = Ahat yh,   e = f/scl^2 - Ahat w      (w: the stored row of W)
 *   dJ/df_k  =  q_k / scl^2                       dJ/da_k = -[ e_k (D2 yh)_k - q_k (D2 w)_k ]
 *   dJ/dda_k = -[ e_k (D1 yh)_k - q_k (D1 w)_k ] / scl        dJ/dc_k =  [ e_k (L yh)_k - q_k (L w)_k ] / scl^2
 *   (dJ/dg_l, dJ/dg_r) = B1^-T ( Wbar_1 + eps C y - Ahat1^T q )
 * An element whose forward status is LSSVR_ST_FALLBACK has dJ/dg_l = (Wbar_0 - Wbar_1)/2, dJ/dg_r = (Wbar_0 + Wbar_1)/2
 * and zero table rows.  gu[i] = dJ/dg_r(element i-1) + dJ/dg_l(element i), the left element's term first, no atomics;
 * where the forward call replaces a nodal value by the Dirichlet value (the global end element whose end point equals
 * gxmin / gxmax exactly) the term goes to gbc[side] and gu gets 0 there; gbc of an end that is not replaced is 0.  The
 * mesh and gamma are not differentiated.
 *
 * lssvr_enhance_adjoint -- DEVICE arrays: x [ne+1]; rhs_values, a_values, da_values, c_values [ne*n_colloc]
 * element-major (lssvr_colloc_points); W, Wbar [ne*M]; status [ne] (the forward call's; NULL: no fallback element).
 * a_values == NULL (then da_values must be NULL too) means a = 1, a' = 0; c_values == NULL means c = 0.  Neither u nor
 * the Dirichlet values are arguments: W carries them.  Outputs, each may be NULL (it then costs neither arithmetic nor a
 * store) but not all: gu [ne+1], gbc [2], ga, gda, gc, gf [ne*n_colloc].  gbc and gu are independent: a replaced end
 * without gbc is dropped.  work: lssvr_enhance_adjoint_work_bytes(ne) bytes on the device; after the call it holds the
 * pairs (dJ/dg_l, dJ/dg_r) [ne][2].  Two launches on `stream` (one without gu and gbc), no synchronisation, no copy.
 * 3 <= M <= 16 (one element per lane, direct Gram in every regime), max(2, M-2) <= n_colloc <= 64.  No output may be
 * one of the inputs or another output.
 * Return codes, each before any HIP call: LSSVR_ERR_SIZE for ne < 1, n_colloc outside [max(2, M-2), 64], a shard
 * outside ne_global, gamma not > 0 or work_bytes too small; LSSVR_ERR_DEGREE for M outside [3, 16]; LSSVR_ERR_NULL for a
 * missing x, rhs_values, W, Wbar or work, for no output at all, for ga or gda without a_values, gc without c_values and
 * da_values without a_values.
 *
 * lssvr_enhance_adjoint_host -- the same routines on HOST arrays: no device is touched.  Bit for bit the device's values.
 */
int64_t lssvr_enhance_adjoint_work_bytes(int64_t ne);
int lssvr_enhance_adjoint(const double* x, int64_t ne, int64_t elem_offset, int64_t ne_global, double gxmin,
                          double gxmax, int M, int n_colloc, double gamma, const double* a_values,
                          const double* da_values, const double* c_values, const double* rhs_values, const double* W,
                          const int32_t* status, const double* Wbar, double* gu, double* gbc, double* ga, double* gda,
                          double* gc, double* gf, void* work, int64_t work_bytes, void* stream);
int lssvr_enhance_adjoint_host(const double* x_host, int64_t ne, int64_t elem_offset, int64_t ne_global, double gxmin,
                               double gxmax, int M, int n_colloc, double gamma, const double* a_values_host,
                               const double* da_values_host, const double* c_values_host,
                               const double* rhs_values_host, const double* W_host, const int32_t* status_h,
                               const double* Wbar_host, double* gu_host, double* gbc_host, double* ga_host,
                               double* gda_host, double* gc_host, double* gf_host, void* work_h,
                               int64_t work_bytes);

/*
 * Adjoint sensitivities of the semilinear P1 solve of -(a u')' + b u' + c u + g(x, u) = f (no reference counterpart;
 * DESIGN.md section 35).  ADDITIVE to ABI 7: two new symbols, no existing entry, struct, constant or kernel
 * instantiation changes, LSSVR_ABI_VERSION stays 7.
 *
 * The discrete problem is R(u) = K u + G(u) - F = 0 on the free rows, G_i(u) = sum_e h_e sum_q w_q phi_i(xi_q)
 * g(x_eq, u_h(x_eq)).  Its Jacobian at the converged u* is K + M(g_u(., u*_h)): the bands of ONE lssvr_p1_assemble (or
 * _react / _conv) with c_quad = c_eff from ONE lssvr_nl_linearize AT u* (not the bands of the last Newton step, which
 * are linearised at the previous iterate).  For a functional J(u) with p = dJ/du the adjoint z solves the TRANSPOSED
 * Jacobian bands with load p, zero end data and the primal's end kinds and kappa, as for lssvr_p1_sensitivity.  The
 * gradients with respect to a_quad, b_quad, c_quad, rhs_quad and the end data are the formulas of lssvr_p1_sensitivity
 * with u = u* and band_ends = {sub[0], sup[ne-1]} of the JACOBIAN bands.  With s = (h_e w_q) z_eq and
 * u_eq = u[e] (1 - xi_q) + u[e+1] xi_q, formed exactly as lssvr_p1_sensitivity forms them, the order of every operation
 * of the gradients with respect to the tables q_k of the law:
 *   LSSVR_NL_POLY  p_0 = 1;  p_k = p_{k-1} u_eq;  dJ/dq_0 = -s;  dJ/dq_k = -(s p_k),  k = 1 .. nterm-1
 *                  (so dJ/dq_0 is -dJ/drhs_quad and dJ/dq_1 is dJ/dc_quad, bit for bit)
 *   LSSVR_NL_EXP   E = exp(q_1 u_eq);  dJ/dq_0 = -(s E);  dJ/dq_1 = -(s ((q_0 u_eq) E))
 *
 * lssvr_semilinear_sensitivity -- ONE launch; x, ne, nquad, U, nu, Z, nc, ga, gb, gc, gf, P, band_ends, the end kinds
 * and out_ends are the arguments of lssvr_p1_sensitivity, and ga, gb, gc, gf and out_ends receive its values bit for
 * bit.
 * kind / nterm as for lssvr_nl_linearize.  gq [nc][nterm][ne*nquad] (element-major tables, case-major) receives
 * dJ/dq_k.  q_tabs [nterm][ne*nquad], the tables lssvr_nl_linearize took at lssvr_quad_points, is read for LSSVR_NL_EXP
 * only: it may be NULL for LSSVR_NL_POLY.  All DEVICE arrays.  Each of ga, gb, gc, gf, gq, out_ends may be NULL (it then
 * costs neither arithmetic nor a store), but not all six.  One thread per table entry, no reduction, no atomics, no
 * synchronisation, no copy.  No output may be one of the inputs or another output.
 * Return codes, each before any HIP call: those of lssvr_p1_sensitivity for its arguments (LSSVR_ERR_SIZE for ne < 1, nc
 * outside [1, 8], nu other than 1 or nc, an unknown end kind with out_ends; LSSVR_ERR_QUAD for nquad outside [1, 5];
 * LSSVR_ERR_NULL for a missing x, U or Z and for out_ends without band_ends); LSSVR_ERR_NULL for six NULL outputs and for
 * LSSVR_NL_EXP without q_tabs; LSSVR_ERR_RHS for an unknown kind; LSSVR_ERR_SIZE for nterm outside [1, 6]
 * (LSSVR_NL_POLY) or other than 2 (LSSVR_NL_EXP).
 *
 * lssvr_semilinear_sensitivity_host -- the same routines on HOST arrays: no device is touched.  Bit for bit the device's
 * values for LSSVR_NL_POLY; for LSSVR_NL_EXP up to the two exp implementations (libm here, the device library's there).
 */
int lssvr_semilinear_sensitivity(const double* x, int64_t ne, int nquad, const double* U, int nu, const double* Z,
                                 int nc, const double* q_tabs, int kind, int nterm, double* ga, double* gb, double* gc,
                                 double* gf, double* gq, const double* P, const double* band_ends, int kind_left,
                                 int kind_right, double* out_ends, void* stream);
int lssvr_semilinear_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* U_host, int nu,
                                      const double* Z_host, int nc, const double* q_tabs_host, int kind, int nterm,
                                      double* ga_host, double* gb_host, double* gc_host, double* gf_host,
                                      double* gq_host, const double* P_host, const double* band_ends_host,
                                      int kind_left, int kind_right, double* out_ends_host);

/*
 * Adjoint sensitivities of the semilinear BDF loop of rho u_t - (a u')' + c u + g(x, u) = f(x, t) (no reference
 * counterpart).  ADDITIVE to ABI 7: four new symbols, no existing entry, struct or constant
 * changes, LSSVR_ABI_VERSION stays 7.
 *
 * The function differentiated is the CONVERGED implicit step: level n is the solution of
 *   F_n(u^n) = K u^n + M(c + alpha_n rho/dt) u^n + G(u^n) - (1/dt) M_rho (beta0_n u^{n-1} + beta1_n u^{n-2}) - L(f(t_n)) = 0
 * on the free rows (G as for lssvr_semilinear_sensitivity), which the Newton iteration of lssvr_ts_nl_assemble converges
 * to; a state whose last increment is |dv| differs from it by O(|dv|^2), and so does the gradient.  The Jacobian of
 * level n is J_n = K + M(c + alpha_n rho/dt + g_u(., u^n_h)), linearised AT u^n (not the last Newton matrix, which is
 * linearised one iterate earlier), symmetric.  With lambda^{N+1} = lambda^{N+2} = 0, for n = N .. 1:
 *   B_n = p_n + (1/dt) M_rho (beta0_{n+1} lambda^{n+1} + beta1_{n+2} lambda^{n+2})
 *   J_n lambda^n = B_n, the forward loop's end kinds and kappa, zero end data        -- lssvr_tridiag_bc_solve_multi
 *
 * lssvr_semilinear_adjoint_step -- ONE launch per level, one thread per node.  x, u = u^n, a_quad (NULL: a = 1),
 * cs_quad = c + alpha_n rho/dt, q_quad, ne, nquad, kind, nterm as for lssvr_ts_nl_assemble; mdiag, moff, U0 =
 * lambda^{n+1}, U1 = lambda^{n+2} (not read when beta1 == 0), loads [R][ne+1], phi [R], R, beta0, beta1, inv_dt as
 * for lssvr_ts_rhs with nc = 1 (for B_n: loads = the row p_n, phi = {1}, R = 1).  Writes diag [ne+1] and off [ne], the
 * bands of J_n -- bit for bit those of lssvr_ts_nl_assemble at u (its right-hand side is not formed) --, B [ne+1] -- bit
 * for bit lssvr_ts_rhs -- and band_ends [2] = {off[0], off[ne-1]}, the row of this level in the band_ends of the entry
 * below.  All DEVICE arrays.  No atomics, no synchronisation, no copy.  Return codes, each before any HIP call: those of
 * the two entries it fuses -- LSSVR_ERR_SIZE for ne < 1, R outside [1, 8], a non-finite beta0, beta1 or inv_dt, nterm
 * outside [1, 6] (LSSVR_NL_POLY) or other than 2 (LSSVR_NL_EXP), an output that is an input or another output;
 * LSSVR_ERR_QUAD for nquad outside [1, 5]; LSSVR_ERR_RHS for an unknown kind; LSSVR_ERR_NULL for a missing array (a_quad
 * may be NULL, U1 with beta1 == 0).
 *
 * lssvr_semilinear_transient_sensitivity -- lssvr_transient_sensitivity for this loop, ONE launch per chunk: x .. R, ga,
 * gc, grho, gf, accumulate, Brows, the end kinds, out_g and out_kappa are its arguments and receive its values bit for
 * bit, with one difference: every level has its own matrix, so band_ends is [m][2], row i = {off[0], off[ne-1]} of the
 * J_n of step row i, and there is no band_mask.  kind / nterm as for lssvr_nl_linearize.  gq [nterm][ne*nquad] receives
 * dJ/dq_k summed over the chunk under the same accumulate flag; NULL: skipped, arithmetic and stores.  With s = (h_e w_q)
 * lambda^n_eq and u_eq = u^n[e] (1 - xi_q) + u^n[e+1] xi_q, formed as for dJ/dc_quad, level by level, n descending, one
 * rounding per operation:
 *   LSSVR_NL_POLY  p_0 = 1;  p_k = p_{k-1} u_eq;  gq_0 = gq_0 - s;  gq_k = gq_k - (s p_k),  k = 1 .. nterm-1
 *                  (so gq_1 is gc and, with phi = 1, gq_0 is -gf, bit for bit)
 *   LSSVR_NL_EXP   E = exp(q_1 u_eq);  gq_0 = gq_0 - (s E);  gq_1 = gq_1 - (s ((q_0 u_eq) E))
 * q_tabs [nterm][ne*nquad] is read for LSSVR_NL_EXP with gq only: it may be NULL otherwise.  Return codes, each before
 * any HIP call: those of lssvr_transient_sensitivity for its arguments (gq counts as an output); LSSVR_ERR_NULL for
 * LSSVR_NL_EXP with gq and without q_tabs; LSSVR_ERR_RHS for an unknown kind; LSSVR_ERR_SIZE for nterm outside [1, 6]
 * (LSSVR_NL_POLY) or other than 2 (LSSVR_NL_EXP).
 *
 * The _host entries run the same routines on HOST arrays: no device is touched.  Bit for bit the device's values for
 * LSSVR_NL_POLY; for LSSVR_NL_EXP up to the two exp implementations (libm here, the device library's there).
 */
int lssvr_semilinear_adjoint_step(const double* x, const double* u, const double* a_quad, const double* cs_quad,
                                  const double* q_quad, int64_t ne, int nquad, int kind, int nterm,
                                  const double* mdiag, const double* moff, const double* U0, const double* U1,
                                  const double* loads, const double* phi, int R, double beta0, double beta1,
                                  double inv_dt, double* diag, double* off, double* B, double* band_ends,
                                  void* stream);
int lssvr_semilinear_adjoint_step_host(const double* x_host, const double* u_host, const double* a_quad_host,
                                       const double* cs_quad_host, const double* q_quad_host, int64_t ne, int nquad,
                                       int kind, int nterm, const double* mdiag_host, const double* moff_host,
                                       const double* U0_host, const double* U1_host, const double* loads_host,
                                       const double* phi_host, int R, double beta0, double beta1, double inv_dt,
                                       double* diag_host, double* off_host, double* B_host,
                                       double* band_ends_host);
int lssvr_semilinear_transient_sensitivity(const double* x, int64_t ne, int nquad, const double* Utraj,
                                           const double* Z, int64_t n0, int m, double inv_dt, const double* coef_host,
                                           const double* phi, int R, const double* q_tabs, int kind, int nterm,
                                           double* ga, double* gc, double* grho, double* gf, double* gq,
                                           int accumulate, const double* Brows, const double* band_ends,
                                           int kind_left, int kind_right, double* out_g, double* out_kappa,
                                           void* stream);
int lssvr_semilinear_transient_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* Utraj_host,
                                                const double* Z_host, int64_t n0, int m, double inv_dt,
                                                const double* coef_host, const double* phi_host, int R,
                                                const double* q_tabs_host, int kind, int nterm, double* ga_host,
                                                double* gc_host, double* grho_host, double* gf_host, double* gq_host,
                                                int accumulate, const double* Brows_host,
                                                const double* band_ends_host, int kind_left, int kind_right,
                                                double* out_g_host, double* out_kappa_host);

/*
 * Bubble-condensed P1 assembly: nodal values of order h^(2 order) for -(a u')' + b u' + c u = f (no reference
 * counterpart).  ADDITIVE to ABI 7: three new symbols, no existing entry, struct, constant or
 * kernel changes, LSSVR_ABI_VERSION stays 7.
 *
 * Every element carries, beside the P1 functions N_0 = 1 - t and N_1 = t on t in [0,1], the hierarchic bubbles
 *   N_k = (P_k(s) - P_{k-2}(s)) / sqrt(2 (2k - 1)),   s = 2t - 1,   k = 2 .. order      (P_k: Legendre)
 * which vanish at both ends.  With the rule of lssvr_quad_points (points t_q, weights w_q) and N' = dN/dt,
 *   K_ij  = sum_q w_q [ a_q N_i' N_j' / h + b_q N_i N_j' + c_q h N_i N_j ],      g_i^r = sum_q w_q h f^r_q N_i,
 * the bubble block is eliminated element by element (Gaussian elimination without pivoting, once per element for all
 * R cases) and what is assembled is tridiagonal on the nodes again:
 *   S = K_vv - K_vb K_bb^-1 K_bv  (2 x 2),       g^r_v - K_vb K_bb^-1 g^r_b  (2 per case),
 *   diag[ne+1]     diag[i] = S11[i-1] + S00[i]           (nodes 0 and ne: the term of the missing element left out)
 *   sub[ne]        sub[i] = S10[i]: the coefficient of u_i in row i+1
 *   sup[ne]        sup[i] = S01[i]: the coefficient of u_{i+1} in row i
 *   load[R][ne+1]  load[r][i] = g1^r[i-1] + g0^r[i]
 *   kloc4[ne][4]   (may be NULL) S00, S01, S10, S11 of every element
 *   floc[R][ne][2] (may be NULL) the condensed load pair of every element and case
 * -- the bands of lssvr_p1_assemble_conv, for lssvr_tridiag_ns_*_solve_multi and lssvr_tridiag_pivot_solve_multi.
 * The bands are not symmetric in general, even with b = 0 (then sub and sup agree to rounding, not to the bit).
 *
 *   order      2 .. 4 (else LSSVR_ERR_DEGREE; order 1 is lssvr_p1_assemble_conv, not served here)
 *   nquad      order+1 .. 5 (else LSSVR_ERR_QUAD)
 *   R          1 .. 8 right-hand sides rhs_quad[R][ne][nquad], tabulated at lssvr_quad_points (else LSSVR_ERR_SIZE)
 *   a_quad, c_quad, b_quad   [ne][nquad], each may be NULL: a = 1, c = 0, b = 0
 *   work       lssvr_p1_bubble_work_bytes(ne, R) = (4 + 2R) ne 8 bytes, 8-byte aligned: the condensed element
 *              quantities between the two passes (NULL: LSSVR_ERR_NULL; too small or misaligned: LSSVR_ERR_SIZE)
 * ne < 1 is LSSVR_ERR_SIZE, a missing x, rhs_quad, diag, sub, sup or load LSSVR_ERR_NULL -- each before any HIP call.
 * Two launches (a thread per element, a thread per node), no atomics, bitwise reproducible.  There is no info word:
 * a bubble pivot that is zero or not finite leaves non-finite entries in the bands of its element, which the caller
 * finds there.  No pivoting: for c >= 0 and a > 0 the bubble block is positive definite when b = 0; the caller
 * checks the bands (finite, rows dominant) before an unpivoted solve.
 *
 * lssvr_p1_assemble_bubble_host -- the same routines on HOST arrays (work included), bit for bit: no device is touched.
 */
int64_t lssvr_p1_bubble_work_bytes(int64_t ne, int R);
int lssvr_p1_assemble_bubble(const double* x, int64_t ne, int order, int nquad, int R, const double* rhs_quad,
                             const double* a_quad, const double* c_quad, const double* b_quad, double* diag,
                             double* sub, double* sup, double* load, double* kloc4, double* floc, void* work,
                             int64_t work_bytes, void* stream);
int lssvr_p1_assemble_bubble_host(const double* x_host, int64_t ne, int order, int nquad, int R,
                                  const double* rhs_quad_host, const double* a_quad_host, const double* c_quad_host,
                                  const double* b_quad_host, double* diag_host, double* sub_host, double* sup_host,
                                  double* load_host, double* kloc4_host, double* floc_host, void* work,
                                  int64_t work_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LSSVR_HIP_H */
