// extern "C" layer: argument validation, error strings, dispatch.  No torch,
// no Python types -- plain pointers and sizes (include/lssvr_hip.h).
#include <cstdarg>
#include <vector>
#include <cstdio>
#include <cstring>

#include <new>
#include "lssvr_kernels.hpp"

namespace {

thread_local char g_err[256] = {0};

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(hipError_t e, const char* what) {
  if (e == hipSuccess) return LSSVR_OK;
  return fail(LSSVR_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// The checks the entries compose, one per idea and one wording each (the ends and the sized
// workspace follow with the tridiagonal solves).  A new entry calls these; it does not spell them out again.
int check_ne(int64_t ne, int ne_min = 1, const char* why = "") {
  if (ne < ne_min) return fail(LSSVR_ERR_SIZE, "ne = %lld < %d%s", (long long)ne, ne_min, why);
  if (ne > (int64_t)1 << 40) return fail(LSSVR_ERR_SIZE, "ne = %lld too large", (long long)ne);
  return LSSVR_OK;
}

bool is_finite(double v) { return v > -INFINITY && v < INFINITY; }

int check_layout(int table_layout) {
  if (table_layout != LSSVR_TABLE_ELEMENT_MAJOR && table_layout != LSSVR_TABLE_POINT_MAJOR)
    return fail(LSSVR_ERR_SIZE, "unknown table_layout %d", table_layout);
  return LSSVR_OK;
}

int check_kinds(int kind_left, int kind_right) {
  if ((kind_left != LSSVR_END_DIRICHLET && kind_left != LSSVR_END_ROBIN) ||
      (kind_right != LSSVR_END_DIRICHLET && kind_right != LSSVR_END_ROBIN))
    return fail(LSSVR_ERR_SIZE, "end kinds (%d, %d) must be LSSVR_END_DIRICHLET or LSSVR_END_ROBIN", kind_left,
                kind_right);
  return LSSVR_OK;
}

// g(x, u) of the semilinear entries: sum_k q_k u^k with 1 .. 6 tables, or q_0 exp(q_1 u)
int check_nl_kind(int kind, int nterm) {
  if (kind != LSSVR_NL_POLY && kind != LSSVR_NL_EXP)
    return fail(LSSVR_ERR_RHS, "unknown kind %d (LSSVR_NL_POLY or LSSVR_NL_EXP)", kind);
  if (kind == LSSVR_NL_POLY && (nterm < 1 || nterm > 6))
    return fail(LSSVR_ERR_SIZE, "nterm = %d outside [1, 6]", nterm);
  if (kind == LSSVR_NL_EXP && nterm != 2) return fail(LSSVR_ERR_SIZE, "nterm = %d: LSSVR_NL_EXP has q_0 and q_1", nterm);
  return LSSVR_OK;
}

// the arguments every enhancement entry shares, validated and bound
int bind_enhance(lssvr::EnhanceArgs& a, const double* x, const double* u, int64_t ne, int64_t elem_offset,
                 int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right, int M,
                 int n_colloc, double gamma, double* W, int32_t* status, int32_t* fail_count) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne = %lld < 0", (long long)ne);
  if (ne > 0 && (!x || !u || !W)) return fail(LSSVR_ERR_NULL, "x, u and W must be non-NULL");
  if (elem_offset < 0 || ne_global < elem_offset + ne)
    return fail(LSSVR_ERR_SIZE, "shard [%lld, %lld) does not fit ne_global = %lld",
                (long long)elem_offset, (long long)(elem_offset + ne), (long long)ne_global);
  if (M < 2 || M > lssvr::kLargeMaxM)
    return fail(LSSVR_ERR_DEGREE, "M = %d outside [2, %d]", M, lssvr::kLargeMaxM);
  if (n_colloc < 2 || n_colloc > 4096)
    return fail(LSSVR_ERR_SIZE, "n_colloc = %d outside [2, 4096]", n_colloc);
  if (!(gamma > 0.0)) return fail(LSSVR_ERR_SIZE, "gamma must be > 0");
  if (ne * (int64_t)M / M != ne) return fail(LSSVR_ERR_SIZE, "ne*M overflows");
  a = lssvr::EnhanceArgs{};
  a.x = x;
  a.u = u;
  a.ne = ne;
  a.ne_mesh = ne;
  a.elem_offset = elem_offset;
  a.ne_global = ne_global;
  a.gxmin = gxmin;
  a.gxmax = gxmax;
  a.bc_left = bc_left;
  a.bc_right = bc_right;
  a.gamma = gamma;
  a.inv_gamma = 1.0 / gamma;
  a.M = M;
  a.n = n_colloc;
  a.refine = lssvr::enhance_small_refine_steps(M, n_colloc);     // (read by the Poisson lane kernel only)
  a.tab_es = n_colloc;      // tabulated arrays: element-major unless bind_rhs says otherwise
  a.tab_ps = 1;
  a.W = W;
  a.status = status;
  a.fail_count = fail_count;
  static const lssvr::TrigTables trig = lssvr::make_trig_tables();
  a.trig = trig;
  return LSSVR_OK;
}

// right-hand side of an enhancement call: named (in-kernel) or tabulated, element- or point-major
int bind_rhs(lssvr::EnhanceArgs& a, int rhs_id, const double* rhs_params_host, const double* rhs_values,
             bool need_values, const char* count_name) {
  a.rhs_id = rhs_id;
  if (rhs_id == LSSVR_RHS_SIN) {
    if (!rhs_params_host) return fail(LSSVR_ERR_RHS, "LSSVR_RHS_SIN needs rhs_params = {amp, omega}");
    a.rhs_amp = rhs_params_host[0];
    a.rhs_omega = rhs_params_host[1];
    return LSSVR_OK;
  }
  if (rhs_id == LSSVR_RHS_ARRAY || rhs_id == LSSVR_RHS_ARRAY_PM) {
    if (need_values && !rhs_values)
      return fail(LSSVR_ERR_RHS, "LSSVR_RHS_ARRAY needs rhs_values[%s*n_colloc]", count_name);
    a.rhs_id = LSSVR_RHS_ARRAY;
    a.rhs_values = rhs_values;
    if (rhs_id == LSSVR_RHS_ARRAY_PM) {     // rhs_values[k * count + e]
      a.tab_es = 1;
      a.tab_ps = a.ne > 0 ? a.ne : 1;
    }
    return LSSVR_OK;
  }
  return fail(LSSVR_ERR_RHS, "unknown rhs_id %d", rhs_id);
}

// the variable-coefficient triple (a, a', f): three tables in one layout
int check_varcoef_tables(const double* a_values, const double* da_values, const double* rhs_values,
                         int table_layout, bool need_values) {
  if (need_values && (!a_values || !da_values || !rhs_values))
    return fail(LSSVR_ERR_NULL, "a_values, da_values and rhs_values must be non-NULL");
  if (const int rc = check_layout(table_layout)) return rc;
  return LSSVR_OK;
}

int bind_varcoef(lssvr::EnhanceArgs& a, const double* a_values, const double* da_values, const double* rhs_values,
                 int table_layout, bool need_values) {
  const int rc = check_varcoef_tables(a_values, da_values, rhs_values, table_layout, need_values);
  if (rc != LSSVR_OK) return rc;
  a.a_values = a_values;
  a.da_values = da_values;
  return bind_rhs(a, table_layout == LSSVR_TABLE_POINT_MAJOR ? LSSVR_RHS_ARRAY_PM : LSSVR_RHS_ARRAY, nullptr,
                  rhs_values, false, "ne");
}

// a caller's workspace against the `need` bytes that `sizer` reports for the call
int check_work(const void* work, int64_t work_bytes, int64_t need, const char* sizer) {
  if (work_bytes < 0 || (work_bytes > 0 && !work)) return fail(LSSVR_ERR_NULL, "work / work_bytes inconsistent");
  // a workspace that is given but too small is an error, not a silent change of kernel (and, in
  // the near-square regime, of accuracy: the refinement needs its 32 extra doubles per element)
  if (work && work_bytes < need)
    return fail(LSSVR_ERR_SIZE, "work holds %lld bytes, %s() = %lld (pass work = NULL for the workspace-free "
                "kernels)", (long long)work_bytes, sizer, (long long)need);
  return LSSVR_OK;
}

// a workspace the entry requires, against the `need` bytes its public `sizer` reports for (ne) or, nc >= 0, (ne, nc)
int check_work_sized(const void* work, int64_t work_bytes, int64_t need, const char* sizer, int64_t ne, int nc = -1) {
  if (!work) return fail(LSSVR_ERR_NULL, "work must be non-NULL");
  if (work_bytes >= need) return LSSVR_OK;
  char tail[16] = "";
  if (nc >= 0) snprintf(tail, sizeof(tail), ", %d", nc);
  return fail(LSSVR_ERR_SIZE, "work holds %lld bytes, %s(%lld%s) = %lld", (long long)work_bytes, sizer, (long long)ne,
              tail, (long long)need);
}

// P1 assembly arguments shared by lssvr_step, lssvr_step_varcoef and lssvr_p1_assemble (rhs left to the caller)
int bind_p1(lssvr::P1Args& p, const double* x, int64_t ne, int nquad, double* diag, double* off, double* load) {
  if (!x || !diag || !off || !load) return fail(LSSVR_ERR_NULL, "x, diag, off, load must be non-NULL");
  if (nquad < 1 || nquad > 5) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  p = lssvr::P1Args{};
  p.x = x;
  p.ne = ne;
  p.nquad = nquad;
  p.diag = diag;
  p.off = off;
  p.load = load;
  return LSSVR_OK;
}

// right-hand side of an assembly: named (in-kernel) or tabulated at the quadrature points
int bind_p1_rhs(lssvr::P1Args& p, int rhs_id, const double* rhs_params_host, const double* rhs_quad) {
  p.rhs_id = rhs_id;
  if (rhs_id == LSSVR_RHS_SIN) {
    if (!rhs_params_host) return fail(LSSVR_ERR_RHS, "LSSVR_RHS_SIN needs rhs_params = {amp, omega}");
    p.rhs_amp = rhs_params_host[0];
    p.rhs_omega = rhs_params_host[1];
    return LSSVR_OK;
  }
  if (rhs_id != LSSVR_RHS_ARRAY) return fail(LSSVR_ERR_RHS, "unknown rhs_id %d", rhs_id);
  if (!rhs_quad) return fail(LSSVR_ERR_RHS, "LSSVR_RHS_ARRAY needs rhs_quad[ne*nquad]");
  p.rhs_quad = rhs_quad;
  return LSSVR_OK;
}

// the arguments lssvr_estimate and lssvr_estimate_varcoef share, validated and bound
int bind_estimate(lssvr::EstimateArgs& a, const double* x, const double* W, int64_t ne, int M, int nq, double* eta2,
                  double* jump, double* out3, void* work) {
  if (const int rc = check_ne(ne)) return rc;
  if (M < 1 || M > lssvr::kAdaptMaxM) return fail(LSSVR_ERR_DEGREE, "M = %d outside [1, %d]", M, lssvr::kAdaptMaxM);
  if (nq < 1 || nq > lssvr::kAdaptMaxNq)
    return fail(LSSVR_ERR_QUAD, "nq = %d outside [1, %d]", nq, lssvr::kAdaptMaxNq);
  if (!x || !W || !eta2 || !out3 || !work) return fail(LSSVR_ERR_NULL, "x, W, eta2, out3, work must be non-NULL");
  a.x = x;
  a.W = W;
  a.ne = ne;
  a.M = M;
  a.nq = nq;
  a.eta2 = eta2;
  a.jump = jump;
  a.work = static_cast<double*>(work);
  return LSSVR_OK;
}

// bind_estimate plus the (a, a', f) tables of lssvr_estimate_varcoef and lssvr_estimate_react
int bind_estimate_vc(lssvr::EstimateVcArgs& a, const double* x, const double* W, int64_t ne, int M, int nq,
                     const double* a_values, const double* da_values, const double* rhs_values, int table_layout,
                     double* eta2, double* jump, double* out3, void* work) {
  int rc = bind_estimate(a, x, W, ne, M, nq, eta2, jump, out3, work);
  if (rc == LSSVR_OK) rc = check_varcoef_tables(a_values, da_values, rhs_values, table_layout, true);
  if (rc != LSSVR_OK) return rc;
  a.rhs_values = rhs_values;
  a.a_values = a_values;
  a.da_values = da_values;
  return LSSVR_OK;
}

// what the three lssvr_eval* entries check first
int check_eval(int64_t ne, int64_t P, int M) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  if (P < 0) return fail(LSSVR_ERR_SIZE, "P < 0");
  if (M < 1) return fail(LSSVR_ERR_DEGREE, "M = %d < 1", M);
  return LSSVR_OK;
}

// shared tail of every enhancement entry but the shared-operator one
int enhance_dispatch(const lssvr::EnhanceArgs& a, int solver_id, hipStream_t s,
                     const lssvr::LaunchOpts* o, void* work = nullptr, int64_t work_bytes = 0) {
  // Fewer collocation points than bubble coefficients: the primal normal equations are rank
  // deficient (float64 returns O(1) errors there), the dual Gram system is well conditioned.
  if (solver_id != LSSVR_SOLVER_DUAL && a.n < a.M - 2) solver_id = LSSVR_SOLVER_DUAL;
  if (solver_id == LSSVR_SOLVER_DUAL) {
    if (a.n > 64) return fail(LSSVR_ERR_SIZE, "dual solver: n_colloc = %d > 64", a.n);
    if (a.elem_ids) return fail(LSSVR_ERR_SOLVER, "dual solver: no subset form");
    return check_launch(lssvr::enhance_dual(a, s, o), "enhance_dual");
  }
  if (a.M <= lssvr::kSmallMaxM && solver_id == LSSVR_SOLVER_PRIMAL)
    return check_launch(lssvr::enhance_small(a, s, o), "enhance_small");
  if (a.elem_ids && solver_id != LSSVR_SOLVER_PRIMAL)
    return fail(LSSVR_ERR_SOLVER, "subset launches take LSSVR_SOLVER_PRIMAL");
  // large degree, Poisson rows, workspace given: Chebyshev moments + four-systems-per-wave solve as
  // two kernels (twice the speed of the MFMA kernel)
  if (solver_id == LSSVR_SOLVER_PRIMAL && !a.a_values && work &&
      work_bytes >= lssvr::enhance_moment_ws_bytes(a.ne, a.M, a.n))
    return check_launch(lssvr::enhance_large_split(a, work, s, o), "enhance_large_split");
  // LSSVR_SOLVER_PRIMAL_MOMENT forces that sequence for any M (A/B against the lane kernel below M = 23)
  if (solver_id == LSSVR_SOLVER_PRIMAL_MOMENT) {
    if (a.a_values) return fail(LSSVR_ERR_SOLVER, "LSSVR_SOLVER_PRIMAL_MOMENT: Poisson rows only");
    if (a.elem_ids) return fail(LSSVR_ERR_SOLVER, "LSSVR_SOLVER_PRIMAL_MOMENT: no subset form");
    if (!work || work_bytes < lssvr::enhance_moment_ws_bytes(a.ne, a.M, a.n))
      return fail(LSSVR_ERR_SOLVER, "LSSVR_SOLVER_PRIMAL_MOMENT needs a workspace of "
                  "lssvr_enhance_work_bytes() bytes (lssvr_enhance_ws)");
    return check_launch(lssvr::enhance_large_split(a, work, s, o), "enhance_large_split");
  }
  // otherwise the direct Gram on the f64 matrix cores
  return check_launch(lssvr::enhance_large(a, s, o), "enhance_large");
}

// a begin / end event pair for one stamped launch
int create_events(lssvr::LaunchOpts& o) {
  if (hipEventCreate(&o.start) != hipSuccess || hipEventCreate(&o.stop) != hipSuccess)
    return fail(LSSVR_ERR_LAUNCH, "hipEventCreate failed");
  return LSSVR_OK;
}

void destroy_events(const lssvr::LaunchOpts& o) {
  if (o.start) (void)hipEventDestroy(o.start);
  if (o.stop) (void)hipEventDestroy(o.stop);
}

// go(const LaunchOpts*) -> LSSVR_* code: plain (go(nullptr)) when kernel_ms_host is NULL, otherwise BLOCKING and
// stamped with the dispatch's own begin / end times
template <typename Launch>
int timed_launch(Launch&& go, float* kernel_ms_host) {
  if (!kernel_ms_host) return go(nullptr);
  lssvr::LaunchOpts o;
  int rc = create_events(o);
  if (rc == LSSVR_OK) rc = go(&o);
  if (rc == LSSVR_OK) {
    hipError_t e = hipEventSynchronize(o.stop);
    if (e == hipSuccess) e = hipEventElapsedTime(kernel_ms_host, o.start, o.stop);
    if (e != hipSuccess) rc = fail(LSSVR_ERR_LAUNCH, "profiled launch: %s", hipGetErrorString(e));
  }
  destroy_events(o);
  return rc;
}

// `repeats` launches of go back to back, each with its own begin / end stamps, ONE synchronisation at the end
template <typename Launch>
int timed_sequence(Launch&& go, hipStream_t s, int repeats, float* kernel_ms_host) {
  std::vector<lssvr::LaunchOpts> ev((size_t)repeats);
  int rc = LSSVR_OK;
  for (int r = 0; r < repeats && rc == LSSVR_OK; ++r) rc = create_events(ev[r]);
  for (int r = 0; r < repeats && rc == LSSVR_OK; ++r) rc = go(&ev[r]);
  hipError_t e = hipStreamSynchronize(s);            // (also after a failed launch: earlier ones are in flight)
  if (rc == LSSVR_OK && e != hipSuccess) rc = fail(LSSVR_ERR_LAUNCH, "profiled sequence: %s", hipGetErrorString(e));
  for (int r = 0; r < repeats && rc == LSSVR_OK; ++r) {
    e = hipEventElapsedTime(&kernel_ms_host[r], ev[r].start, ev[r].stop);
    if (e != hipSuccess) rc = fail(LSSVR_ERR_LAUNCH, "profiled sequence: %s", hipGetErrorString(e));
  }
  for (const lssvr::LaunchOpts& o : ev) destroy_events(o);
  return rc;
}

// preconditions of the *_sequence entries, before their arguments are bound
int check_sequence(int64_t ne, int repeats, const float* kernel_ms_host) {
  if (!kernel_ms_host) return fail(LSSVR_ERR_NULL, "kernel_ms_host must be non-NULL (float[repeats])");
  if (repeats < 1 || repeats > 100000) return fail(LSSVR_ERR_SIZE, "repeats = %d outside [1, 100000]", repeats);
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "nothing to profile: ne = %lld", (long long)ne);
  return LSSVR_OK;
}

// the arguments of lssvr_enhance_ws / lssvr_enhance_ws_sequence, validated and bound
int bind_enhance_ws(lssvr::EnhanceArgs& a, const double* x, const double* u, int64_t ne, int64_t elem_offset,
                    int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right, int M,
                    int n_colloc, double gamma, int rhs_id, const double* rhs_params_host, const double* rhs_values,
                    int solver_id, double* W, int32_t* status, int32_t* fail_count, void* work,
                    int64_t work_bytes) {
  int rc = bind_enhance(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                        gamma, W, status, fail_count);
  if (rc == LSSVR_OK) rc = bind_rhs(a, rhs_id, rhs_params_host, rhs_values, ne > 0, "ne");
  if (rc != LSSVR_OK) return rc;
  if (solver_id != LSSVR_SOLVER_PRIMAL && solver_id != LSSVR_SOLVER_DUAL &&
      solver_id != LSSVR_SOLVER_PRIMAL_WAVE && solver_id != LSSVR_SOLVER_PRIMAL_MOMENT)
    return fail(LSSVR_ERR_SOLVER, "unknown solver_id %d", solver_id);
  return check_work(work, work_bytes, lssvr_enhance_work_bytes(ne, M, n_colloc, solver_id),
                    "lssvr_enhance_work_bytes");
}

// the arguments of lssvr_enhance_varcoef_ws / lssvr_enhance_varcoef_ws_sequence, validated and bound
int bind_varcoef_ws(lssvr::EnhanceArgs& a, const double* x, const double* u, int64_t ne, int64_t elem_offset,
                    int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right, int M,
                    int n_colloc, double gamma, const double* a_values, const double* da_values,
                    const double* rhs_values, int table_layout, double* W, int32_t* status, int32_t* fail_count,
                    void* work, int64_t work_bytes) {
  int rc = bind_enhance(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                        gamma, W, status, fail_count);
  if (rc == LSSVR_OK) rc = bind_varcoef(a, a_values, da_values, rhs_values, table_layout, ne > 0);
  if (rc != LSSVR_OK) return rc;
  return check_work(work, work_bytes, lssvr_enhance_varcoef_work_bytes(ne, M, n_colloc),
                    "lssvr_enhance_varcoef_work_bytes");
}

// the arguments of lssvr_enhance_react_ws, validated and bound: the variable-coefficient ones plus the c table
int bind_react_ws(lssvr::EnhanceReactArgs& a, const double* x, const double* u, int64_t ne, int64_t elem_offset,
                  int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right, int M,
                  int n_colloc, double gamma, const double* a_values, const double* da_values,
                  const double* c_values, const double* rhs_values, int table_layout, double* W, int32_t* status,
                  int32_t* fail_count, void* work, int64_t work_bytes) {
  a = lssvr::EnhanceReactArgs{};
  int rc = bind_varcoef_ws(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, gamma,
                           a_values, da_values, rhs_values, table_layout, W, status, fail_count, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  if (ne > 0 && !c_values) return fail(LSSVR_ERR_NULL, "c_values must be non-NULL");
  if (n_colloc < M - 2)
    return fail(LSSVR_ERR_SOLVER, "lssvr_enhance_react: n_colloc = %d < M-2 = %d (the reaction rows have no dual "
                                  "solver)", n_colloc, M - 2);
  a.c_values = c_values;
  return LSSVR_OK;
}

int react_dispatch(const lssvr::EnhanceReactArgs& a, hipStream_t s, const lssvr::LaunchOpts* o) {
  if (a.M <= lssvr::kReactSmallMaxM) return check_launch(lssvr::enhance_small_react(a, s, o), "enhance_small_react");
  return check_launch(lssvr::enhance_large_react(a, s, o), "enhance_large_react");
}

// the one body of lssvr_colloc_points and lssvr_colloc_points_pm
int colloc_points_entry(const double* x, int64_t ne, int n_colloc, double* xc, void* stream, bool point_major) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne < 0");
  if (n_colloc < 2) return fail(LSSVR_ERR_SIZE, "n_colloc < 2");
  if (ne > 0 && (!x || !xc)) return fail(LSSVR_ERR_NULL, "x and xc must be non-NULL");
  return check_launch(lssvr::colloc_points(x, ne, n_colloc, xc, reinterpret_cast<hipStream_t>(stream), point_major),
                      point_major ? "colloc_points(point-major)" : "colloc_points");
}

}  // namespace

extern "C" {

int lssvr_version(void) { return LSSVR_ABI_VERSION; }

const char* lssvr_last_error(void) { return g_err; }

int lssvr_enhance(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                  int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right,
                  int M, int n_colloc, double gamma, int rhs_id, const double* rhs_params_host,
                  const double* rhs_values, int solver_id, double* W, int32_t* status,
                  int32_t* fail_count, void* stream) {
  return lssvr_enhance_ws(x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, gamma,
                          rhs_id, rhs_params_host, rhs_values, solver_id, W, status, fail_count, nullptr, 0, stream,
                          nullptr);
}

int64_t lssvr_enhance_work_bytes(int64_t ne, int M, int n_colloc, int solver_id) {
  if (ne <= 0) return 0;
  if (solver_id == LSSVR_SOLVER_PRIMAL_MOMENT) return lssvr::enhance_moment_ws_bytes(ne, M, n_colloc);
  if (solver_id != LSSVR_SOLVER_PRIMAL || M <= lssvr::kSmallMaxM) return 0;
  return lssvr::enhance_moment_ws_bytes(ne, M, n_colloc);
}

int lssvr_enhance_ws(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                     int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right,
                     int M, int n_colloc, double gamma, int rhs_id, const double* rhs_params_host,
                     const double* rhs_values, int solver_id, double* W, int32_t* status,
                     int32_t* fail_count, void* work, int64_t work_bytes, void* stream,
                     float* kernel_ms_host) {
  lssvr::EnhanceArgs a;
  const int rc = bind_enhance_ws(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                                 gamma, rhs_id, rhs_params_host, rhs_values, solver_id, W, status, fail_count, work,
                                 work_bytes);
  if (rc != LSSVR_OK || ne == 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return timed_launch([&](const lssvr::LaunchOpts* o) { return enhance_dispatch(a, solver_id, s, o, work, work_bytes); },
                      kernel_ms_host);
}

int lssvr_enhance_ws_sequence(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                              int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right,
                              int M, int n_colloc, double gamma, int rhs_id, const double* rhs_params_host,
                              const double* rhs_values, int solver_id, double* W, int32_t* status,
                              int32_t* fail_count, void* work, int64_t work_bytes, void* stream,
                              int repeats, float* kernel_ms_host) {
  lssvr::EnhanceArgs a;
  int rc = check_sequence(ne, repeats, kernel_ms_host);
  if (rc == LSSVR_OK)
    rc = bind_enhance_ws(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, gamma,
                         rhs_id, rhs_params_host, rhs_values, solver_id, W, status, fail_count, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return timed_sequence([&](const lssvr::LaunchOpts* o) { return enhance_dispatch(a, solver_id, s, o, work, work_bytes); },
                        s, repeats, kernel_ms_host);
}

int lssvr_enhance_profiled(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                           int64_t ne_global, double gxmin, double gxmax, double bc_left,
                           double bc_right, int M, int n_colloc, double gamma, int rhs_id,
                           const double* rhs_params_host, const double* rhs_values, int solver_id,
                           double* W, int32_t* status, void* stream, float* kernel_ms_host) {
  if (!kernel_ms_host) return fail(LSSVR_ERR_NULL, "kernel_ms_host must be non-NULL");
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "nothing to profile: ne = %lld", (long long)ne);
  return lssvr_enhance_ws(x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, gamma,
                          rhs_id, rhs_params_host, rhs_values, solver_id, W, status, nullptr, nullptr, 0, stream,
                          kernel_ms_host);
}

// lssvr_step's arguments, validated and turned into the kernels' argument blocks: what a plan keeps
struct lssvr_step_plan {
  lssvr::EnhanceArgs a;
  lssvr::P1Args p;
  const double* memo = nullptr;     // lssvr_step_plan_memo_bind: caller-owned, read by the fused step only
};

// bytes of a plan's memo; 0 where the plan cannot use one: no fused step (M > kSmallMaxM, refinement), or loop
// results that are not functions of the mesh and the plan's constants alone (gamma_values, a tabulated rhs)
static int64_t step_memo_bytes(const lssvr_step_plan& b) {
  const lssvr::EnhanceArgs& a = b.a;
  if (a.M > lssvr::kSmallMaxM || a.refine > 0 || a.gamma_values || a.rhs_id != LSSVR_RHS_SIN || a.ne < 1) return 0;
  return 8 * lssvr::step_memo_doubles(a.M, a.ne);
}

static int bind_step(lssvr_step_plan& b, const double* x, const double* u, int64_t ne, int64_t elem_offset,
                     int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right,
                     int M, int n_colloc, double gamma, const double* rhs_params_host, int nquad,
                     double* diag, double* off, double* load, double* W, int32_t* status,
                     int32_t* fail_count) {
  lssvr::EnhanceArgs& a = b.a;
  int rc = bind_enhance(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, gamma,
                        W, status, fail_count);
  if (rc != LSSVR_OK) return rc;
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  rc = bind_p1(b.p, x, ne, nquad, diag, off, load);
  if (rc == LSSVR_OK) rc = bind_rhs(a, LSSVR_RHS_SIN, rhs_params_host, nullptr, false, "ne");
  if (rc != LSSVR_OK) return rc;
  if (n_colloc < M - 2)
    return fail(LSSVR_ERR_SOLVER, "lssvr_step: n_colloc = %d < M-2 = %d: the primal normal equations are "
                                  "rank deficient; use lssvr_p1_assemble + lssvr_enhance (dual solver)",
                n_colloc, M - 2);
  return bind_p1_rhs(b.p, LSSVR_RHS_SIN, rhs_params_host, nullptr);
}

static int run_step(const lssvr_step_plan& b, hipStream_t s) {
  const lssvr::EnhanceArgs& a = b.a;
  const lssvr::P1Args& p = b.p;
  // (near-square regime, a.refine > 0: the refinement lives in a kernel of its own -- two launches)
  if (a.M <= lssvr::kSmallMaxM && a.refine == 0)
    return check_launch(lssvr::step_small(a, p, s, nullptr, b.memo), "step_small");
  int rc = check_launch(lssvr::p1_assemble(p, s), "p1_assemble");
  if (rc != LSSVR_OK) return rc;
  if (a.M <= lssvr::kSmallMaxM) return check_launch(lssvr::enhance_small(a, s), "enhance_small(refine)");
  // large degree: the enhancement is long enough that a fused launch buys nothing
  return check_launch(lssvr::enhance_large(a, s), "enhance_large");
}

int lssvr_step(const double* x, const double* u, int64_t ne, int64_t elem_offset,
               int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right,
               int M, int n_colloc, double gamma, const double* rhs_params_host, int nquad,
               double* diag, double* off, double* load, double* W, int32_t* status,
               int32_t* fail_count, void* stream) {
  lssvr_step_plan b;
  const int rc = bind_step(b, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                           gamma, rhs_params_host, nquad, diag, off, load, W, status, fail_count);
  if (rc != LSSVR_OK) return rc;
  return run_step(b, reinterpret_cast<hipStream_t>(stream));
}

int lssvr_step_plan_create(lssvr_step_plan** plan, const double* x, const double* u, int64_t ne,
                           int64_t elem_offset, int64_t ne_global, double gxmin, double gxmax,
                           double bc_left, double bc_right, int M, int n_colloc, double gamma,
                           const double* rhs_params_host, int nquad, double* diag, double* off,
                           double* load, double* W, int32_t* status, int32_t* fail_count) {
  if (!plan) return fail(LSSVR_ERR_NULL, "plan must be non-NULL");
  *plan = nullptr;
  lssvr_step_plan* b = new (std::nothrow) lssvr_step_plan;
  if (!b) return fail(LSSVR_ERR_LAUNCH, "out of host memory");
  const int rc = bind_step(*b, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                           gamma, rhs_params_host, nquad, diag, off, load, W, status, fail_count);
  if (rc != LSSVR_OK) {
    delete b;
    return rc;
  }
  *plan = b;
  return LSSVR_OK;
}

int lssvr_step_plan_launch(const lssvr_step_plan* plan, void* stream) {
  if (!plan) return fail(LSSVR_ERR_NULL, "plan must be non-NULL");
  return run_step(*plan, reinterpret_cast<hipStream_t>(stream));
}

int64_t lssvr_step_plan_memo_bytes(const lssvr_step_plan* plan) { return plan ? step_memo_bytes(*plan) : 0; }

int lssvr_step_plan_memo_bind(lssvr_step_plan* plan, void* memo, int64_t memo_bytes, void* stream) {
  if (!plan) return fail(LSSVR_ERR_NULL, "plan must be non-NULL");
  if (!memo) {                       // unbind: the plan runs the loop again
    plan->memo = nullptr;
    return LSSVR_OK;
  }
  const int64_t need = step_memo_bytes(*plan);
  if (need == 0)
    return fail(LSSVR_ERR_SOLVER, "this plan cannot use a memo (lssvr_step_plan_memo_bytes is 0: M = %d, n_colloc = %d)",
                plan->a.M, plan->a.n);
  if (memo_bytes < need)
    return fail(LSSVR_ERR_SIZE, "memo_bytes = %lld < lssvr_step_plan_memo_bytes = %lld", (long long)memo_bytes,
                (long long)need);
  if (reinterpret_cast<uintptr_t>(memo) % 8 != 0) return fail(LSSVR_ERR_SIZE, "memo must be 8-byte aligned");
  plan->memo = nullptr;              // (a failed fill leaves the plan on the loop)
  const int rc = check_launch(lssvr::step_small_memo_fill(plan->a, static_cast<double*>(memo),
                                                          reinterpret_cast<hipStream_t>(stream)),
                              "step_memo_fill");
  if (rc == LSSVR_OK) plan->memo = static_cast<const double*>(memo);
  return rc;
}

int lssvr_step_plan_destroy(lssvr_step_plan* plan) {
  delete plan;
  return LSSVR_OK;
}

int lssvr_enhance_varcoef(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                          int64_t ne_global, double gxmin, double gxmax, double bc_left,
                          double bc_right, int M, int n_colloc, double gamma,
                          const double* a_values, const double* da_values,
                          const double* rhs_values, double* W, int32_t* status,
                          int32_t* fail_count, void* stream) {
  return lssvr_enhance_varcoef_ws(x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M,
                                  n_colloc, gamma, a_values, da_values, rhs_values, LSSVR_TABLE_ELEMENT_MAJOR,
                                  W, status, fail_count, nullptr, 0, stream, nullptr);
}

int lssvr_step_varcoef(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                       int64_t ne_global, double gxmin, double gxmax, double bc_left, double bc_right,
                       int M, int n_colloc, double gamma, const double* a_values,
                       const double* da_values, const double* rhs_values, int table_layout, int nquad,
                       const double* rhs_quad, const double* a_quad, double* diag, double* off,
                       double* load, double* W, int32_t* status, int32_t* fail_count, void* stream) {
  lssvr::EnhanceArgs a;
  int rc = bind_enhance(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, gamma,
                        W, status, fail_count);
  if (rc != LSSVR_OK) return rc;
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  rc = bind_varcoef(a, a_values, da_values, rhs_values, table_layout, true);
  if (rc != LSSVR_OK) return rc;
  if (!rhs_quad || !a_quad) return fail(LSSVR_ERR_NULL, "rhs_quad and a_quad must be non-NULL");
  lssvr::P1Args p;
  rc = bind_p1(p, x, ne, nquad, diag, off, load);
  if (rc != LSSVR_OK) return rc;
  if (n_colloc < M - 2)
    return fail(LSSVR_ERR_SOLVER, "lssvr_step_varcoef: n_colloc = %d < M-2 = %d: use lssvr_p1_assemble + "
                                  "lssvr_enhance_varcoef (dual solver)", n_colloc, M - 2);
  p.rhs_id = LSSVR_RHS_ARRAY;
  p.rhs_quad = rhs_quad;
  p.a_quad = a_quad;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (M <= lssvr::kStepVarcoefFusedMaxM) return check_launch(lssvr::step_small_vc(a, p, s), "step_small_vc");
  rc = check_launch(lssvr::p1_assemble(p, s), "p1_assemble");
  if (rc != LSSVR_OK) return rc;
  return enhance_dispatch(a, LSSVR_SOLVER_PRIMAL, s, nullptr);
}

int lssvr_enhance_react(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                        int64_t ne_global, double gxmin, double gxmax, double bc_left,
                        double bc_right, int M, int n_colloc, double gamma,
                        const double* a_values, const double* da_values, const double* c_values,
                        const double* rhs_values, double* W, int32_t* status,
                        int32_t* fail_count, void* stream) {
  return lssvr_enhance_react_ws(x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M,
                                n_colloc, gamma, a_values, da_values, c_values, rhs_values,
                                LSSVR_TABLE_ELEMENT_MAJOR, W, status, fail_count, nullptr, 0, stream, nullptr);
}

int lssvr_enhance_react_ws(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                           int64_t ne_global, double gxmin, double gxmax, double bc_left,
                           double bc_right, int M, int n_colloc, double gamma,
                           const double* a_values, const double* da_values, const double* c_values,
                           const double* rhs_values, int table_layout, double* W, int32_t* status,
                           int32_t* fail_count, void* work, int64_t work_bytes, void* stream,
                           float* kernel_ms_host) {
  lssvr::EnhanceReactArgs a;
  const int rc = bind_react_ws(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                               gamma, a_values, da_values, c_values, rhs_values, table_layout, W, status,
                               fail_count, work, work_bytes);
  if (rc != LSSVR_OK || ne == 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return timed_launch([&](const lssvr::LaunchOpts* o) { return react_dispatch(a, s, o); }, kernel_ms_host);
}

int lssvr_enhance_multi(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                        int64_t ne_global, double gxmin, double gxmax, const double* bc_values, int ncases,
                        int M, int n_colloc, double gamma, const double* a_values, const double* da_values,
                        const double* c_values, const double* rhs_values, int table_layout, double* W,
                        int32_t* status, int32_t* fail_count, void* stream, float* kernel_ms_host) {
  lssvr::EnhanceMultiArgs a{};
  // the shard / ne / M / n_colloc / gamma / table rules of lssvr_enhance_react_ws (c_values may be NULL here)
  int rc = bind_varcoef_ws(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, 0.0, 0.0, M, n_colloc, gamma,
                           a_values, da_values, rhs_values, table_layout, W, status, fail_count, nullptr, 0);
  if (rc != LSSVR_OK) return rc;
  if (ncases < 1) return fail(LSSVR_ERR_SIZE, "ncases = %d < 1", ncases);
  if (n_colloc < M - 2)
    return fail(LSSVR_ERR_SOLVER, "lssvr_enhance_multi: n_colloc = %d < M-2 = %d (primal solve only)", n_colloc,
                M - 2);
  const int64_t per_case = ne * (int64_t)(M > n_colloc ? M : n_colloc);
  if (per_case > 0 && per_case * ncases / ncases != per_case) return fail(LSSVR_ERR_SIZE, "ncases*ne*M overflows");
  if (ne == 0) return LSSVR_OK;
  a.c_values = c_values;
  a.bc_values = bc_values;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (M <= lssvr::kReactSmallMaxM)
    return timed_launch(
        [&](const lssvr::LaunchOpts* o) { return check_launch(lssvr::enhance_multi(a, ncases, s, o), "enhance_multi"); },
        kernel_ms_host);
  // Above the lane kernels: the wave kernel of the single-case entry, once per case -- correct, no faster.  Those
  // kernels take the Dirichlet pair by value, so a shard that holds an end of the global domain reads bc_values
  // back first (the stream is synchronised).
  std::vector<double> bc((size_t)ncases * 2, 0.0);
  if (bc_values && (elem_offset == 0 || elem_offset + ne == ne_global)) {
    hipError_t e = hipMemcpyAsync(bc.data(), bc_values, bc.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(LSSVR_ERR_LAUNCH, "lssvr_enhance_multi: bc_values: %s", hipGetErrorString(e));
  }
  if (kernel_ms_host) *kernel_ms_host = 0.0f;
  for (int j = 0; j < ncases; ++j) {
    lssvr::EnhanceReactArgs r = a;
    r.u = u + (int64_t)j * (ne + 1);
    r.rhs_values = rhs_values + (int64_t)j * ne * n_colloc;
    r.W = W + (int64_t)j * ne * M;
    r.status = status ? status + (int64_t)j * ne : nullptr;
    r.bc_left = bc[2 * (size_t)j];
    r.bc_right = bc[2 * (size_t)j + 1];
    float ms = 0.0f;
    rc = timed_launch(
        [&](const lssvr::LaunchOpts* o) {
          return c_values ? react_dispatch(r, s, o) : enhance_dispatch(r, LSSVR_SOLVER_PRIMAL, s, o);
        },
        kernel_ms_host ? &ms : nullptr);
    if (rc != LSSVR_OK) return rc;
    if (kernel_ms_host) *kernel_ms_host += ms;
  }
  return LSSVR_OK;
}

// (no variable-coefficient kernel takes a workspace: always 0, kept for ABI 6)
int64_t lssvr_enhance_varcoef_work_bytes(int64_t ne, int M, int n_colloc) {
  (void)ne; (void)M; (void)n_colloc;
  return 0;
}

int lssvr_enhance_varcoef_ws(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                             int64_t ne_global, double gxmin, double gxmax, double bc_left,
                             double bc_right, int M, int n_colloc, double gamma,
                             const double* a_values, const double* da_values,
                             const double* rhs_values, int table_layout, double* W, int32_t* status,
                             int32_t* fail_count, void* work, int64_t work_bytes, void* stream,
                             float* kernel_ms_host) {
  lssvr::EnhanceArgs a;
  const int rc = bind_varcoef_ws(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                                 gamma, a_values, da_values, rhs_values, table_layout, W, status, fail_count, work,
                                 work_bytes);
  if (rc != LSSVR_OK || ne == 0) return rc;
  // (n_colloc < M-2: rank-deficient primal normal equations -> the dual Gram solver)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return timed_launch(
      [&](const lssvr::LaunchOpts* o) { return enhance_dispatch(a, LSSVR_SOLVER_PRIMAL, s, o, work, work_bytes); },
      kernel_ms_host);
}

int lssvr_enhance_varcoef_ws_sequence(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                                      int64_t ne_global, double gxmin, double gxmax, double bc_left,
                                      double bc_right, int M, int n_colloc, double gamma,
                                      const double* a_values, const double* da_values,
                                      const double* rhs_values, int table_layout, double* W, int32_t* status,
                                      int32_t* fail_count, void* work, int64_t work_bytes, void* stream,
                                      int repeats, float* kernel_ms_host) {
  lssvr::EnhanceArgs a;
  int rc = check_sequence(ne, repeats, kernel_ms_host);
  if (rc == LSSVR_OK)
    rc = bind_varcoef_ws(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, gamma,
                         a_values, da_values, rhs_values, table_layout, W, status, fail_count, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return timed_sequence(
      [&](const lssvr::LaunchOpts* o) { return enhance_dispatch(a, LSSVR_SOLVER_PRIMAL, s, o, work, work_bytes); },
      s, repeats, kernel_ms_host);
}

int lssvr_enhance_subset(const double* x, const double* u, int64_t ne_mesh,
                         const int64_t* elem_ids, int64_t nsub, int64_t elem_offset,
                         int64_t ne_global, double gxmin, double gxmax, double bc_left,
                         double bc_right, int M, int n_colloc, double gamma,
                         const double* gamma_values, int rhs_id, const double* rhs_params_host,
                         const double* rhs_values, double* W, int64_t ldw, int32_t* status,
                         int32_t* fail_count, void* stream) {
  return lssvr_enhance_subset_ws(x, u, ne_mesh, elem_ids, nsub, elem_offset, ne_global, gxmin, gxmax, bc_left,
                                 bc_right, M, n_colloc, gamma, gamma_values, rhs_id, rhs_params_host, rhs_values,
                                 W, ldw, status, fail_count, nullptr, 0, stream);
}

int lssvr_enhance_subset_ws(const double* x, const double* u, int64_t ne_mesh,
                            const int64_t* elem_ids, int64_t nsub, int64_t elem_offset,
                            int64_t ne_global, double gxmin, double gxmax, double bc_left,
                            double bc_right, int M, int n_colloc, double gamma,
                            const double* gamma_values, int rhs_id, const double* rhs_params_host,
                            const double* rhs_values, double* W, int64_t ldw, int32_t* status,
                            int32_t* fail_count, void* work, int64_t work_bytes, void* stream) {
  if (ne_mesh < 0 || nsub < 0) return fail(LSSVR_ERR_SIZE, "ne_mesh / nsub < 0");
  if (!elem_ids && nsub != ne_mesh)
    return fail(LSSVR_ERR_SIZE, "elem_ids == NULL means every element: nsub must equal ne_mesh");
  if (elem_ids && nsub > ne_mesh) return fail(LSSVR_ERR_SIZE, "nsub = %lld > ne_mesh = %lld",
                                              (long long)nsub, (long long)ne_mesh);
  if (ldw != 0 && ldw < M) return fail(LSSVR_ERR_SIZE, "ldw = %lld < M = %d", (long long)ldw, M);
  if (ne_global < elem_offset + ne_mesh)
    return fail(LSSVR_ERR_SIZE, "shard [%lld, %lld) does not fit ne_global = %lld",
                (long long)elem_offset, (long long)(elem_offset + ne_mesh), (long long)ne_global);
  lssvr::EnhanceArgs a;
  // (the shard check of bind_enhance is on the subset size here: done above for the mesh)
  int rc = bind_enhance(a, x, u, nsub, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                        gamma_values ? 1.0 : gamma, W, status, fail_count);
  if (rc != LSSVR_OK) return rc;
  if (n_colloc < M - 2)
    return fail(LSSVR_ERR_SOLVER, "lssvr_enhance_subset: n_colloc < M-2 needs the dual solver, "
                                  "which has no subset form");
  a.gamma = gamma;
  a.inv_gamma = 1.0 / gamma;
  a.elem_ids = elem_ids;
  a.ne_mesh = ne_mesh;
  a.gamma_values = gamma_values;
  a.ldw = ldw;
  rc = bind_rhs(a, rhs_id, rhs_params_host, rhs_values, nsub > 0, "nsub");
  if (rc == LSSVR_OK)
    rc = check_work(work, work_bytes, lssvr_enhance_work_bytes(nsub, M, n_colloc, LSSVR_SOLVER_PRIMAL),
                    "lssvr_enhance_work_bytes");
  if (rc != LSSVR_OK || nsub == 0) return rc;
  // (M <= 22: the lane kernel; above, with a workspace: moments + solve kernels, without: the MFMA kernel)
  return enhance_dispatch(a, LSSVR_SOLVER_PRIMAL, reinterpret_cast<hipStream_t>(stream), nullptr, work, work_bytes);
}

int lssvr_enhance_react_subset(const double* x, const double* u, int64_t ne_mesh,
                               const int64_t* elem_ids, int64_t nsub, int64_t elem_offset,
                               int64_t ne_global, double gxmin, double gxmax, double bc_left,
                               double bc_right, int M, int n_colloc, double gamma,
                               const double* gamma_values, const double* a_values, const double* da_values,
                               const double* c_values, const double* rhs_values, int table_layout,
                               double* W, int64_t ldw, int32_t* status, int32_t* fail_count, void* stream) {
  // the element-list rules of lssvr_enhance_subset_ws ...
  if (ne_mesh < 0 || nsub < 0) return fail(LSSVR_ERR_SIZE, "ne_mesh / nsub < 0");
  if (!elem_ids && nsub != ne_mesh)
    return fail(LSSVR_ERR_SIZE, "elem_ids == NULL means every element: nsub must equal ne_mesh");
  if (elem_ids && nsub > ne_mesh) return fail(LSSVR_ERR_SIZE, "nsub = %lld > ne_mesh = %lld",
                                              (long long)nsub, (long long)ne_mesh);
  if (ldw != 0 && ldw < M) return fail(LSSVR_ERR_SIZE, "ldw = %lld < M = %d", (long long)ldw, M);
  if (ne_global < elem_offset + ne_mesh)
    return fail(LSSVR_ERR_SIZE, "shard [%lld, %lld) does not fit ne_global = %lld",
                (long long)elem_offset, (long long)(elem_offset + ne_mesh), (long long)ne_global);
  // ... then the one validation path of lssvr_enhance_react_ws / lssvr_enhance_varcoef_ws, on the launch count (the
  // tables are indexed by position: point-major stride nsub)
  lssvr::EnhanceReactArgs a{};
  int rc;
  if (c_values) {
    rc = bind_react_ws(a, x, u, nsub, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                       gamma_values ? 1.0 : gamma, a_values, da_values, c_values, rhs_values, table_layout, W, status,
                       fail_count, nullptr, 0);
  } else {
    rc = bind_varcoef_ws(a, x, u, nsub, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc,
                         gamma_values ? 1.0 : gamma, a_values, da_values, rhs_values, table_layout, W, status,
                         fail_count, nullptr, 0);
    if (rc == LSSVR_OK && n_colloc < M - 2)
      return fail(LSSVR_ERR_SOLVER, "lssvr_enhance_react_subset: n_colloc = %d < M-2 = %d needs the dual solver, "
                                    "which has no subset form", n_colloc, M - 2);
  }
  if (rc != LSSVR_OK || nsub == 0) return rc;
  a.gamma = gamma;
  a.inv_gamma = 1.0 / gamma;
  a.elem_ids = elem_ids;
  a.ne_mesh = ne_mesh;
  a.gamma_values = gamma_values;
  a.ldw = ldw;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (c_values == NULL: the lane kernel up to M = 22, the MFMA kernel above; else react_dispatch's pair)
  return c_values ? react_dispatch(a, s, nullptr) : enhance_dispatch(a, LSSVR_SOLVER_PRIMAL, s, nullptr);
}

int lssvr_colloc_points_subset(const double* x, int64_t ne_mesh, const int64_t* elem_ids, int64_t nsub,
                               int n_colloc, int table_layout, double* xc, void* stream) {
  if (ne_mesh < 0 || nsub < 0) return fail(LSSVR_ERR_SIZE, "ne_mesh / nsub < 0");
  if (n_colloc < 2) return fail(LSSVR_ERR_SIZE, "n_colloc < 2");
  if (const int rc = check_layout(table_layout)) return rc;
  if (!elem_ids && nsub != ne_mesh)
    return fail(LSSVR_ERR_SIZE, "elem_ids == NULL means every element: nsub must equal ne_mesh");
  if (elem_ids && nsub > ne_mesh) return fail(LSSVR_ERR_SIZE, "nsub = %lld > ne_mesh = %lld",
                                              (long long)nsub, (long long)ne_mesh);
  if (nsub * (int64_t)n_colloc / n_colloc != nsub) return fail(LSSVR_ERR_SIZE, "nsub*n_colloc overflows");
  if (nsub > 0 && (!x || !xc)) return fail(LSSVR_ERR_NULL, "x and xc must be non-NULL");
  return check_launch(lssvr::colloc_points_subset(x, ne_mesh, elem_ids, nsub, n_colloc, xc,
                                                  reinterpret_cast<hipStream_t>(stream),
                                                  table_layout == LSSVR_TABLE_POINT_MAJOR),
                      "colloc_points_subset");
}

int lssvr_enhance_shared(const double* x, const double* u, int64_t ne, int64_t elem_offset,
                         int64_t ne_global, double gxmin, double gxmax, double bc_left,
                         double bc_right, int M, int n_colloc, int rhs_id,
                         const double* rhs_params_host, const double* rhs_values, const double* op,
                         double* W, int32_t* status, int32_t* fail_count, void* stream,
                         float* kernel_ms_host) {
  lssvr::EnhanceArgs a;
  int rc = bind_enhance(a, x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left, bc_right, M, n_colloc, 1.0,
                        W, status, fail_count);
  if (rc != LSSVR_OK) return rc;
  if (M > lssvr::kSharedMaxM)
    return fail(LSSVR_ERR_DEGREE, "shared-operator path: M = %d > %d", M, lssvr::kSharedMaxM);
  if (ne > 0 && !op) return fail(LSSVR_ERR_NULL, "op[(n_colloc+2)*M] must be non-NULL");
  rc = bind_rhs(a, rhs_id, rhs_params_host, rhs_values, ne > 0, "ne");
  if (rc != LSSVR_OK || ne == 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return timed_launch(
      [&](const lssvr::LaunchOpts* o) { return check_launch(lssvr::enhance_shared(a, op, s, o), "enhance_shared"); },
      kernel_ms_host);
}

int lssvr_colloc_points(const double* x, int64_t ne, int n_colloc, double* xc, void* stream) {
  return colloc_points_entry(x, ne, n_colloc, xc, stream, false);
}

int lssvr_colloc_points_pm(const double* x, int64_t ne, int n_colloc, double* xc, void* stream) {
  return colloc_points_entry(x, ne, n_colloc, xc, stream, true);
}

int lssvr_p1_assemble(const double* x, int64_t ne, int nquad, int rhs_id,
                      const double* rhs_params_host, const double* rhs_quad, const double* a_quad,
                      double* diag, double* off, double* load, double* kloc, double* floc,
                      void* stream) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  lssvr::P1Args a;
  int rc = bind_p1(a, x, ne, nquad, diag, off, load);
  if (rc == LSSVR_OK) rc = bind_p1_rhs(a, rhs_id, rhs_params_host, rhs_quad);
  if (rc != LSSVR_OK) return rc;
  a.a_quad = a_quad;
  a.kloc = kloc;
  a.floc = floc;
  return check_launch(lssvr::p1_assemble(a, reinterpret_cast<hipStream_t>(stream)), "p1_assemble");
}

int lssvr_p1_assemble_react(const double* x, int64_t ne, int nquad, int rhs_id,
                            const double* rhs_params_host, const double* rhs_quad, const double* a_quad,
                            const double* c_quad, double* diag, double* off, double* load, double* kloc,
                            double* floc, void* stream) {
  // no reaction term: the very launch of lssvr_p1_assemble
  if (!c_quad)
    return lssvr_p1_assemble(x, ne, nquad, rhs_id, rhs_params_host, rhs_quad, a_quad, diag, off, load, kloc, floc,
                             stream);
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  lssvr::P1ReactArgs a{};
  int rc = bind_p1(a, x, ne, nquad, diag, off, load);
  if (rc == LSSVR_OK) rc = bind_p1_rhs(a, rhs_id, rhs_params_host, rhs_quad);
  if (rc != LSSVR_OK) return rc;
  a.a_quad = a_quad;
  a.c_quad = c_quad;
  a.kloc = kloc;
  a.floc = floc;
  return check_launch(lssvr::p1_assemble_react(a, reinterpret_cast<hipStream_t>(stream)), "p1_assemble_react");
}

int lssvr_p1_assemble_conv(const double* x, int64_t ne, int nquad, int rhs_id,
                           const double* rhs_params_host, const double* rhs_quad, const double* a_quad,
                           const double* c_quad, const double* b_quad, double* diag, double* sub, double* sup,
                           double* load, double* kloc, double* floc, void* stream) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  if (!sub || !sup) return fail(LSSVR_ERR_NULL, "sub and sup must be non-NULL");
  lssvr::P1ConvArgs a{};
  int rc = bind_p1(a, x, ne, nquad, diag, sub, load);
  if (rc == LSSVR_OK) rc = bind_p1_rhs(a, rhs_id, rhs_params_host, rhs_quad);
  if (rc != LSSVR_OK) return rc;
  a.off = nullptr;                // one band no longer: sub and sup
  a.a_quad = a_quad;
  a.c_quad = c_quad;
  a.b_quad = b_quad;
  a.sub = sub;
  a.sup = sup;
  a.kloc = kloc;
  a.floc = floc;
  return check_launch(lssvr::p1_assemble_conv(a, reinterpret_cast<hipStream_t>(stream)), "p1_assemble_conv");
}

// Bubble-condensed assembly (p1_bubble.hip).  The device and the host entry share one validated binding.
static int bind_p1_bubble(lssvr::P1BubbleArgs& a, const double* x, int64_t ne, int order, int nquad, int R,
                          const double* rhs_quad, const double* a_quad, const double* c_quad, const double* b_quad,
                          double* diag, double* sub, double* sup, double* load, double* kloc4, double* floc,
                          void* work, int64_t work_bytes) {
  if (const int rc = check_ne(ne)) return rc;
  if (order < 2 || order > 4)
    return fail(LSSVR_ERR_DEGREE, "order = %d outside [2, 4] (order 1 is lssvr_p1_assemble_conv)", order);
  if (nquad < order + 1 || nquad > 5)
    return fail(LSSVR_ERR_QUAD, "nquad = %d outside [order+1, 5] = [%d, 5]", nquad, order + 1);
  if (R < 1 || R > 8) return fail(LSSVR_ERR_SIZE, "R = %d outside [1, 8]", R);
  if (!x || !rhs_quad || !diag || !sub || !sup || !load)
    return fail(LSSVR_ERR_NULL, "x, rhs_quad, diag, sub, sup, load must be non-NULL");
  if (const int rc = check_work_sized(work, work_bytes, lssvr::p1_bubble_work_bytes(ne, R),
                                      "lssvr_p1_bubble_work_bytes", ne, R))
    return rc;
  if (reinterpret_cast<uintptr_t>(work) % alignof(double) != 0)
    return fail(LSSVR_ERR_SIZE, "work must be aligned to 8 bytes");
  a = lssvr::P1BubbleArgs{x,    ne,  order, nquad, R,     rhs_quad, a_quad, c_quad,
                          b_quad, diag, sub,   sup,   load,  kloc4,    floc,   static_cast<double*>(work)};
  return LSSVR_OK;
}

int64_t lssvr_p1_bubble_work_bytes(int64_t ne, int R) {
  return ne < 1 || R < 1 || R > 8 ? 0 : lssvr::p1_bubble_work_bytes(ne, R);
}

int lssvr_p1_assemble_bubble(const double* x, int64_t ne, int order, int nquad, int R, const double* rhs_quad,
                             const double* a_quad, const double* c_quad, const double* b_quad, double* diag,
                             double* sub, double* sup, double* load, double* kloc4, double* floc, void* work,
                             int64_t work_bytes, void* stream) {
  lssvr::P1BubbleArgs a{};
  const int rc = bind_p1_bubble(a, x, ne, order, nquad, R, rhs_quad, a_quad, c_quad, b_quad, diag, sub, sup, load,
                                kloc4, floc, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::p1_assemble_bubble(a, reinterpret_cast<hipStream_t>(stream)), "p1_assemble_bubble");
}

int lssvr_p1_assemble_bubble_host(const double* x_host, int64_t ne, int order, int nquad, int R,
                                  const double* rhs_quad_host, const double* a_quad_host, const double* c_quad_host,
                                  const double* b_quad_host, double* diag_host, double* sub_host, double* sup_host,
                                  double* load_host, double* kloc4_host, double* floc_host, void* work,
                                  int64_t work_bytes) {
  lssvr::P1BubbleArgs a{};
  const int rc = bind_p1_bubble(a, x_host, ne, order, nquad, R, rhs_quad_host, a_quad_host, c_quad_host, b_quad_host,
                                diag_host, sub_host, sup_host, load_host, kloc4_host, floc_host, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  if (!lssvr::p1_assemble_bubble_host(a)) return fail(LSSVR_ERR_QUAD, "no rule for order = %d, nquad = %d", order, nquad);
  return LSSVR_OK;
}

int lssvr_quad_points(const double* x, int64_t ne, int nquad, double* xq, void* stream) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne < 0");
  if (nquad < 1 || nquad > 5) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  if (ne > 0 && (!x || !xq)) return fail(LSSVR_ERR_NULL, "x and xq must be non-NULL");
  return check_launch(lssvr::quad_points(x, ne, nquad, xq, reinterpret_cast<hipStream_t>(stream)),
                      "quad_points");
}

// several load cases on one mesh: the loads in one launch, the solves with the bands read once per pass
int lssvr_p1_load_multi(const double* x, int64_t ne, int nquad, const double* rhs_quad, int nc, double* load,
                        void* stream) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  if (nc < 1) return fail(LSSVR_ERR_SIZE, "nc = %d < 1", nc);
  if (!x || !rhs_quad || !load) return fail(LSSVR_ERR_NULL, "x, rhs_quad, load must be non-NULL");
  if (nquad < 1 || nquad > 5) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  return check_launch(lssvr::p1_load_multi(x, ne, nquad, rhs_quad, nc, load, reinterpret_cast<hipStream_t>(stream)),
                      "p1_load_multi");
}

// The tridiagonal solves (tridiag.hip, tridiag_pivot.hip).  One row per family holds what its entries check before they
// launch (the table of DESIGN.md section 19 and of ops._TRIDIAG): the fewest elements and what follows "ne = .. <
// ne_min" in the message, the public sizer the "work holds" message names, whether a Robin kappa may have either sign.
struct TriFamily { int ne_min; const char* ne_why; const char* sizer; int64_t (*need)(int64_t, int); bool any_sign; };
#define TRI_SIZER(f) "lssvr_" #f, lssvr::f
static const TriFamily kTriDirichlet = {1, "", TRI_SIZER(tridiag_multi_work_bytes), false};
static const TriFamily kTriBc = {1, "", TRI_SIZER(tridiag_bc_work_bytes), false};
static const TriFamily kTriPivot = {1, "", TRI_SIZER(tridiag_pivot_work_bytes), true};
static const TriFamily kTriPeriodic = {2, ": a periodic mesh has at least two elements",
                                       TRI_SIZER(tridiag_periodic_work_bytes), false};

int64_t lssvr_tridiag_work_bytes(int64_t ne) { return lssvr::tridiag_work_bytes(ne); }       // (the multi formula, nc = 1)
int64_t lssvr_tridiag_ns_work_bytes(int64_t ne) { return lssvr::tridiag_work_bytes(ne); }
int64_t lssvr_tridiag_multi_work_bytes(int64_t ne, int nc) { return lssvr::tridiag_multi_work_bytes(ne, nc); }
int64_t lssvr_tridiag_bc_work_bytes(int64_t ne, int nc) { return lssvr::tridiag_bc_work_bytes(ne, nc); }
int64_t lssvr_tridiag_pivot_work_bytes(int64_t ne, int nc) { return lssvr::tridiag_pivot_work_bytes(ne, nc); }
int64_t lssvr_tridiag_periodic_work_bytes(int64_t ne, int nc) { return lssvr::tridiag_periodic_work_bytes(ne, nc); }

// (any_sign: the pivoting solve takes a kappa of either sign)
static int check_end_kinds(int kind_left, int kind_right, const double* kappa_host, bool any_sign = false) {
  if (const int rc = check_kinds(kind_left, kind_right)) return rc;
  if (!kappa_host) return fail(LSSVR_ERR_NULL, "kappa_host must be non-NULL");
  for (int i = 0; i < 2; ++i)
    if ((i ? kind_right : kind_left) == LSSVR_END_ROBIN) {
      if (any_sign && !is_finite(kappa_host[i]))
        return fail(LSSVR_ERR_SIZE, "kappa[%d] = %g must be finite", i, kappa_host[i]);
      if (!any_sign && !(kappa_host[i] >= 0.0 && is_finite(kappa_host[i])))
        return fail(LSSVR_ERR_SIZE, "kappa[%d] = %g must be finite and >= 0", i, kappa_host[i]);
    }
  return LSSVR_OK;
}

// Two free ends as an entry gets them and, once check_ends has checked them, as the launchers take them: f = the end is
// a Robin end, k = its kappa (0 at a Dirichlet end, whose kappa is not read).
struct Ends { int kind_left, kind_right; const double* kappa_host; bool f0, f1; double k0, k1; };

static int check_ends(Ends& e, bool any_sign) {
  if (const int rc = check_end_kinds(e.kind_left, e.kind_right, e.kappa_host, any_sign)) return rc;
  e.f0 = e.kind_left == LSSVR_END_ROBIN, e.f1 = e.kind_right == LSSVR_END_ROBIN;
  e.k0 = e.f0 ? e.kappa_host[0] : 0.0, e.k1 = e.f1 ? e.kappa_host[1] : 0.0;
  return LSSVR_OK;
}
enum TriWork { kTriNoWork, kTriWorkUnsized, kTriWorkSized };

// What every tridiagonal entry checks before it launches, in this order: ne, nc, the NULL list (sup == NULL: a symmetric
// entry, whose one band `off` arrives as sub), the end kinds (`ends` given), work_bytes against the family's sizer.
// kTriWorkUnsized: the single-RHS Dirichlet entries, which have no work_bytes argument; kTriNoWork: the host entry.
static int tridiag_check(const TriFamily& fam, bool sym, const double* diag, const double* sub, const double* sup,
                         const double* load, int64_t ne, int nc, const double* u, TriWork mode, const void* work,
                         int64_t work_bytes, Ends* ends = nullptr) {
  if (ne < fam.ne_min) return fail(LSSVR_ERR_SIZE, "ne = %lld < %d%s", (long long)ne, fam.ne_min, fam.ne_why);
  if (nc < 1) return fail(LSSVR_ERR_SIZE, "nc = %d < 1", nc);
  if (!diag || !sub || (!sym && !sup) || !load || !u || (mode != kTriNoWork && !work))
    return fail(LSSVR_ERR_NULL, "diag, %s, load, u%s must be non-NULL", sym ? "off" : "sub, sup",
                mode != kTriNoWork ? ", work" : "");
  if (ends)
    if (const int rc = check_ends(*ends, fam.any_sign)) return rc;
  if (mode == kTriWorkSized) return check_work_sized(work, work_bytes, fam.need(ne, nc), fam.sizer, ne, nc);
  return LSSVR_OK;
}

// Two Dirichlet ends.  The single-RHS entries are nc = 1 with the end values u0, u1 by value (bc NULL).
static int tridiag_solve(const double* diag, const double* sub, const double* sup, const double* load, int64_t ne,
                         int nc, const double* bc, double u0, double u1, double* u, void* work, int64_t work_bytes,
                         void* stream, bool sym, bool multi) {
  const int rc = tridiag_check(kTriDirichlet, sym, diag, sub, sup, load, ne, nc, u,
                               multi ? kTriWorkSized : kTriWorkUnsized, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (sym)
    return check_launch(lssvr::tridiag_dirichlet_solve(diag, sub, load, ne, nc, bc, u0, u1, u, work, st),
                        multi ? "tridiag_dirichlet_solve_multi" : "tridiag_dirichlet_solve");
  return check_launch(lssvr::tridiag_ns_dirichlet_solve(diag, sub, sup, load, ne, nc, bc, u0, u1, u, work, st),
                      multi ? "tridiag_ns_dirichlet_solve_multi" : "tridiag_ns_dirichlet_solve");
}

int lssvr_tridiag_dirichlet_solve(const double* diag, const double* off, const double* load, int64_t ne, double u0,
                                  double u1, double* u, void* work, void* stream) {
  return tridiag_solve(diag, off, nullptr, load, ne, 1, nullptr, u0, u1, u, work, 0, stream, true, false);
}

int lssvr_tridiag_ns_dirichlet_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                     int64_t ne, double u0, double u1, double* u, void* work, void* stream) {
  return tridiag_solve(diag, sub, sup, load, ne, 1, nullptr, u0, u1, u, work, 0, stream, false, false);
}

int lssvr_tridiag_dirichlet_solve_multi(const double* diag, const double* off, const double* load, int64_t ne, int nc,
                                        const double* bc_values, double* u, void* work, int64_t work_bytes,
                                        void* stream) {
  return tridiag_solve(diag, off, nullptr, load, ne, nc, bc_values, 0.0, 0.0, u, work, work_bytes, stream, true, true);
}

int lssvr_tridiag_ns_dirichlet_solve_multi(const double* diag, const double* sub, const double* sup,
                                           const double* load, int64_t ne, int nc, const double* bc_values, double* u,
                                           void* work, int64_t work_bytes, void* stream) {
  return tridiag_solve(diag, sub, sup, load, ne, nc, bc_values, 0.0, 0.0, u, work, work_bytes, stream, false, true);
}

// Free ends: Dirichlet or Robin at each end.
static int tridiag_bc_solve(const double* diag, const double* sub, const double* sup, const double* load,
                            int kind_left, int kind_right, const double* end_values, const double* kappa_host,
                            int64_t ne, int nc, double* u, void* work, int64_t work_bytes, void* stream, bool sym) {
  Ends e{kind_left, kind_right, kappa_host};
  const int rc = tridiag_check(kTriBc, sym, diag, sub, sup, load, ne, nc, u, kTriWorkSized, work, work_bytes, &e);
  if (rc != LSSVR_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (sym)
    return check_launch(lssvr::tridiag_bc_solve(diag, sub, load, ne, nc, e.f0, e.f1, e.k0, e.k1, end_values, u, work,
                                                st),
                        "tridiag_bc_solve_multi");
  return check_launch(lssvr::tridiag_ns_bc_solve(diag, sub, sup, load, ne, nc, e.f0, e.f1, e.k0, e.k1, end_values, u,
                                                 work, st),
                      "tridiag_ns_bc_solve_multi");
}

int lssvr_tridiag_bc_solve_multi(const double* diag, const double* off, const double* load, int kind_left,
                                 int kind_right, const double* end_values, const double* kappa_host, int64_t ne,
                                 int nc, double* u, void* work, int64_t work_bytes, void* stream) {
  return tridiag_bc_solve(diag, off, nullptr, load, kind_left, kind_right, end_values, kappa_host, ne, nc, u, work,
                          work_bytes, stream, true);
}

int lssvr_tridiag_ns_bc_solve_multi(const double* diag, const double* sub, const double* sup, const double* load,
                                    int kind_left, int kind_right, const double* end_values,
                                    const double* kappa_host, int64_t ne, int nc, double* u, void* work,
                                    int64_t work_bytes, void* stream) {
  return tridiag_bc_solve(diag, sub, sup, load, kind_left, kind_right, end_values, kappa_host, ne, nc, u, work,
                          work_bytes, stream, false);
}

// The pivoting solve: the ends of lssvr_tridiag_ns_bc_solve_multi, any non-singular matrix.
int lssvr_tridiag_pivot_solve_multi(const double* diag, const double* sub, const double* sup, const double* load,
                                    int kind_left, int kind_right, const double* end_values,
                                    const double* kappa_host, int64_t ne, int nc, double* u, int32_t* info,
                                    void* work, int64_t work_bytes, void* stream) {
  Ends e{kind_left, kind_right, kappa_host};
  const int rc = tridiag_check(kTriPivot, false, diag, sub, sup, load, ne, nc, u, kTriWorkSized, work, work_bytes, &e);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::tridiag_pivot_solve(diag, sub, sup, load, ne, nc, e.f0, e.f1, e.k0, e.k1, end_values, u,
                                                 info, work, reinterpret_cast<hipStream_t>(stream)),
                      "tridiag_pivot_solve_multi");
}

// the same on host arrays, no device involved
int lssvr_tridiag_pivot_solve_host(const double* diag, const double* sub, const double* sup, const double* load,
                                   int kind_left, int kind_right, const double* end_values,
                                   const double* kappa_host, int64_t ne, int nc, double* u, int32_t* info) {
  Ends e{kind_left, kind_right, kappa_host};
  const int rc = tridiag_check(kTriPivot, false, diag, sub, sup, load, ne, nc, u, kTriNoWork, nullptr, 0, &e);
  if (rc != LSSVR_OK) return rc;
  lssvr::tridiag_pivot_host(diag, sub, sup, load, ne, nc, e.f0, e.f1, e.k0, e.k1, end_values, u, info);
  return LSSVR_OK;
}

// Periodic ends.
static int tridiag_periodic_solve(const double* diag, const double* sub, const double* sup, const double* load,
                                  int64_t ne, int nc, double* u, void* work, int64_t work_bytes, void* stream,
                                  bool sym) {
  const int rc = tridiag_check(kTriPeriodic, sym, diag, sub, sup, load, ne, nc, u, kTriWorkSized, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (sym)
    return check_launch(lssvr::tridiag_periodic_solve(diag, sub, load, ne, nc, u, work, st),
                        "tridiag_periodic_solve_multi");
  return check_launch(lssvr::tridiag_ns_periodic_solve(diag, sub, sup, load, ne, nc, u, work, st),
                      "tridiag_ns_periodic_solve_multi");
}

int lssvr_tridiag_periodic_solve_multi(const double* diag, const double* off, const double* load, int64_t ne, int nc,
                                       double* u, void* work, int64_t work_bytes, void* stream) {
  return tridiag_periodic_solve(diag, off, nullptr, load, ne, nc, u, work, work_bytes, stream, true);
}

int lssvr_tridiag_ns_periodic_solve_multi(const double* diag, const double* sub, const double* sup,
                                          const double* load, int64_t ne, int nc, double* u, void* work,
                                          int64_t work_bytes, void* stream) {
  return tridiag_periodic_solve(diag, sub, sup, load, ne, nc, u, work, work_bytes, stream, false);
}

int64_t lssvr_p1_flux_work_bytes(int64_t ne) { return lssvr::flux_work_bytes(ne); }

int lssvr_p1_flux_solve(const double* kloc, const double* load, int64_t ne, double u0, double u1,
                        double* u, void* work, void* stream) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  if (!kloc || !load || !u || !work) return fail(LSSVR_ERR_NULL, "kloc, load, u, work must be non-NULL");
  return check_launch(lssvr::flux_dirichlet_solve(kloc, load, ne, u0, u1, u, work,
                                                  reinterpret_cast<hipStream_t>(stream)),
                      "flux_dirichlet_solve");
}

int lssvr_p1_flux_aggregate(const double* kloc, const double* load, int64_t ne, int first_global,
                            void* work, double* agg3, void* stream) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  if (!kloc || !load || !work || !agg3) return fail(LSSVR_ERR_NULL, "kloc, load, work, agg3 must be non-NULL");
  return check_launch(lssvr::flux_aggregate(kloc, load, ne, first_global != 0, work, agg3,
                                            reinterpret_cast<hipStream_t>(stream)),
                      "flux_aggregate");
}

int lssvr_p1_flux_finish(const double* kloc, const double* load, int64_t ne, int first_global,
                         int last_global, const void* work, const double* prefix3,
                         const double* grand3, double u0, double u1, double* u, void* stream) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  if (!kloc || !load || !work || !u) return fail(LSSVR_ERR_NULL, "kloc, load, work, u must be non-NULL");
  return check_launch(lssvr::flux_finish(kloc, load, ne, first_global != 0, last_global != 0, work,
                                         prefix3, grand3, u0, u1, u,
                                         reinterpret_cast<hipStream_t>(stream)),
                      "flux_finish");
}

int lssvr_eval(const double* x, const double* W, int64_t ne, int M, const double* xq, int64_t P,
               double* uq, int64_t* elem, void* stream) {
  const int rc = check_eval(ne, P, M);
  if (rc != LSSVR_OK) return rc;
  if (!x || !W || (P > 0 && (!xq || !uq))) return fail(LSSVR_ERR_NULL, "x, W, xq, uq must be non-NULL");
  return check_launch(lssvr::eval_points(x, W, ne, M, xq, P, uq, elem,
                                         reinterpret_cast<hipStream_t>(stream)),
                      "eval_points");
}

int lssvr_eval_error(const double* x, const double* W, int64_t ne, int M, const double* xq,
                     int64_t P, const double* exact_params_host, double* out3, void* stream) {
  const int rc = check_eval(ne, P, M);
  if (rc != LSSVR_OK) return rc;
  if (!x || !W || !out3 || !exact_params_host || (P > 0 && !xq))
    return fail(LSSVR_ERR_NULL, "x, W, xq, exact_params, out3 must be non-NULL");
  return check_launch(lssvr::eval_error(x, W, ne, M, xq, P, exact_params_host[0],
                                        exact_params_host[1], out3,
                                        reinterpret_cast<hipStream_t>(stream)),
                      "eval_error");
}

int lssvr_eval_deriv(const double* x, const double* W, int64_t ne, int M, int order, const double* xq,
                     int64_t P, double* out, int64_t* elem, void* stream) {
  const int rc = check_eval(ne, P, M);
  if (rc != LSSVR_OK) return rc;
  if (order < 0 || order > 2) return fail(LSSVR_ERR_DEGREE, "order = %d outside {0, 1, 2}", order);
  if (!x || !W || (P > 0 && (!xq || !out))) return fail(LSSVR_ERR_NULL, "x, W, xq, out must be non-NULL");
  return check_launch(lssvr::eval_deriv(x, W, ne, M, order, xq, P, out, elem,
                                        reinterpret_cast<hipStream_t>(stream)),
                      "eval_deriv");
}

int lssvr_gauss_rule(int nq, double* xi_host, double* wt_host) {
  if (nq < 1 || nq > lssvr::kAdaptMaxNq)
    return fail(LSSVR_ERR_QUAD, "nq = %d outside [1, %d]", nq, lssvr::kAdaptMaxNq);
  if (!xi_host || !wt_host) return fail(LSSVR_ERR_NULL, "xi and wt must be non-NULL");
  lssvr::gauss_rule(nq, xi_host, wt_host);
  return LSSVR_OK;
}

int lssvr_estimate_points(const double* x, int64_t ne, int nq, double* xq, void* stream) {
  if (ne < 1) return fail(LSSVR_ERR_SIZE, "ne = %lld < 1", (long long)ne);
  if (nq < 1 || nq > lssvr::kAdaptMaxNq)
    return fail(LSSVR_ERR_QUAD, "nq = %d outside [1, %d]", nq, lssvr::kAdaptMaxNq);
  if (!x || !xq) return fail(LSSVR_ERR_NULL, "x and xq must be non-NULL");
  return check_launch(lssvr::estimate_points(x, ne, nq, xq, reinterpret_cast<hipStream_t>(stream)),
                      "estimate_points");
}

int64_t lssvr_adapt_work_bytes(int64_t ne) { return lssvr::adapt_work_bytes(ne); }

int lssvr_estimate(const double* x, const double* W, int64_t ne, int M, int nq, int rhs_id,
                   const double* rhs_params_host, const double* rhs_values, double* eta2, double* jump,
                   double* out3, void* work, void* stream) {
  lssvr::EstimateArgs a{};
  const int rc = bind_estimate(a, x, W, ne, M, nq, eta2, jump, out3, work);
  if (rc != LSSVR_OK) return rc;
  int mode;
  if (rhs_id == LSSVR_RHS_SIN) {
    if (!rhs_params_host) return fail(LSSVR_ERR_RHS, "LSSVR_RHS_SIN needs rhs_params = {amp, omega}");
    a.rhs_amp = rhs_params_host[0];
    a.rhs_omega = rhs_params_host[1];
    mode = 1;
  } else if (rhs_id == LSSVR_RHS_ARRAY || rhs_id == LSSVR_RHS_ARRAY_PM) {
    if (!rhs_values) return fail(LSSVR_ERR_RHS, "LSSVR_RHS_ARRAY needs rhs_values[ne*nq]");
    a.rhs_values = rhs_values;
    mode = rhs_id == LSSVR_RHS_ARRAY ? 0 : 2;
  } else {
    return fail(LSSVR_ERR_RHS, "unknown rhs_id %d", rhs_id);
  }
  return check_launch(lssvr::estimate(a, mode, out3, reinterpret_cast<hipStream_t>(stream)), "estimate");
}

int lssvr_estimate_varcoef(const double* x, const double* W, int64_t ne, int M, int nq, const double* a_values,
                           const double* da_values, const double* rhs_values, int table_layout, const double* a_ends,
                           double* eta2, double* jump, double* out3, void* work, void* stream) {
  lssvr::EstimateVcArgs a{};
  const int rc = bind_estimate_vc(a, x, W, ne, M, nq, a_values, da_values, rhs_values, table_layout, eta2, jump, out3,
                                  work);
  if (rc != LSSVR_OK) return rc;
  if (!a_ends) return fail(LSSVR_ERR_NULL, "a_ends must be non-NULL");
  a.a_ends = a_ends;
  return check_launch(lssvr::estimate_varcoef(a, table_layout == LSSVR_TABLE_POINT_MAJOR, out3,
                                              reinterpret_cast<hipStream_t>(stream)),
                      "estimate_varcoef");
}

int lssvr_estimate_react(const double* x, const double* W, int64_t ne, int M, int nq, const double* a_values,
                         const double* da_values, const double* c_values, const double* rhs_values, int table_layout,
                         const double* a_ends, double* eta2, double* jump, double* out3, void* work, void* stream) {
  lssvr::EstimateReactArgs a{};
  const int rc = bind_estimate_vc(a, x, W, ne, M, nq, a_values, da_values, rhs_values, table_layout, eta2, jump, out3,
                                  work);
  if (rc != LSSVR_OK) return rc;
  if (!c_values) return fail(LSSVR_ERR_NULL, "c_values must be non-NULL");     // (checked before a_ends, as ever)
  if (!a_ends) return fail(LSSVR_ERR_NULL, "a_ends must be non-NULL");
  a.c_values = c_values;
  a.a_ends = a_ends;
  return check_launch(lssvr::estimate_react(a, table_layout == LSSVR_TABLE_POINT_MAJOR, out3,
                                            reinterpret_cast<hipStream_t>(stream)),
                      "estimate_react");
}

int lssvr_estimate_ends(const double* x, const double* W, int M, int64_t ne, int kind_left, int kind_right,
                        const double* kappa_host, const double* g_host, const double* a_ends_host, double* eta2,
                        double* out3, void* stream) {
  if (const int rc = check_ne(ne)) return rc;
  if (M < 1 || M > lssvr::kAdaptMaxM) return fail(LSSVR_ERR_DEGREE, "M = %d outside [1, %d]", M, lssvr::kAdaptMaxM);
  if (!x || !W || !eta2 || !out3) return fail(LSSVR_ERR_NULL, "x, W, eta2, out3 must be non-NULL");
  const int rc = check_end_kinds(kind_left, kind_right, kappa_host);
  if (rc != LSSVR_OK) return rc;
  if (!g_host || !a_ends_host) return fail(LSSVR_ERR_NULL, "g_host and a_ends_host must be non-NULL");
  lssvr::EstimateEndsArgs a{};
  a.x = x;
  a.W = W;
  a.ne = ne;
  a.M = M;
  a.kind[0] = kind_left;
  a.kind[1] = kind_right;
  for (int i = 0; i < 2; ++i) {
    a.kappa[i] = a.kind[i] == LSSVR_END_ROBIN ? kappa_host[i] : 0.0;
    a.g[i] = g_host[i];
    a.a[i] = a_ends_host[i];
  }
  a.eta2 = eta2;
  a.out3 = out3;
  return check_launch(lssvr::estimate_ends(a, reinterpret_cast<hipStream_t>(stream)), "estimate_ends");
}

int lssvr_estimate_seam(const double* x, const double* W, int M, int64_t ne, const double* a_seam_host, double* eta2,
                        double* out3, void* stream) {
  if (const int rc = check_ne(ne, 2, ": a periodic mesh has at least two elements")) return rc;
  if (M < 1 || M > lssvr::kAdaptMaxM) return fail(LSSVR_ERR_DEGREE, "M = %d outside [1, %d]", M, lssvr::kAdaptMaxM);
  if (!x || !W || !eta2 || !out3) return fail(LSSVR_ERR_NULL, "x, W, eta2, out3 must be non-NULL");
  if (!a_seam_host) return fail(LSSVR_ERR_NULL, "a_seam_host must be non-NULL");
  lssvr::EstimateSeamArgs a{};
  a.x = x;
  a.W = W;
  a.ne = ne;
  a.M = M;
  a.a[0] = a_seam_host[0];
  a.a[1] = a_seam_host[1];
  a.eta2 = eta2;
  a.out3 = out3;
  return check_launch(lssvr::estimate_seam(a, reinterpret_cast<hipStream_t>(stream)), "estimate_seam");
}

int64_t lssvr_goal_work_bytes(int64_t ne) { return lssvr::goal_work_bytes(ne); }

int lssvr_estimate_goal(const double* x, const double* Wu, const double* Wz, int64_t ne, int M, int nq,
                        const double* a_values, const double* da_values, const double* c_values,
                        const double* rhs_values, const double* goal_values, int table_layout, const double* a_ends,
                        int kind_left, int kind_right, const double* kappa_host, const double* g_host,
                        const double* a_bnd_host, int jump_free, double* eta, double* eta2, double* q, double* out4,
                        void* work, void* stream) {
  // the checks of bind_estimate_vc, on this entry's own argument names
  if (const int rc = check_ne(ne)) return rc;
  if (M < 1 || M > lssvr::kAdaptMaxM) return fail(LSSVR_ERR_DEGREE, "M = %d outside [1, %d]", M, lssvr::kAdaptMaxM);
  if (nq < 1 || nq > lssvr::kAdaptMaxNq)
    return fail(LSSVR_ERR_QUAD, "nq = %d outside [1, %d]", nq, lssvr::kAdaptMaxNq);
  if (!x || !Wu || !Wz || !eta || !eta2 || !out4 || !work)
    return fail(LSSVR_ERR_NULL, "x, Wu, Wz, eta, eta2, out4, work must be non-NULL");
  int rc = check_varcoef_tables(a_values, da_values, rhs_values, table_layout, true);
  if (rc != LSSVR_OK) return rc;
  if (!goal_values) return fail(LSSVR_ERR_NULL, "goal_values must be non-NULL");
  if (!a_ends) return fail(LSSVR_ERR_NULL, "a_ends must be non-NULL");
  rc = check_end_kinds(kind_left, kind_right, kappa_host);
  if (rc != LSSVR_OK) return rc;
  if (!g_host || !a_bnd_host) return fail(LSSVR_ERR_NULL, "g_host and a_bnd_host must be non-NULL");
  if (jump_free != 0 && jump_free != 1) return fail(LSSVR_ERR_SIZE, "jump_free = %d must be 0 or 1", jump_free);
  lssvr::GoalArgs a{};
  a.x = x;
  a.Wu = Wu;
  a.Wz = Wz;
  a.ne = ne;
  a.M = M;
  a.nq = nq;
  a.a_values = a_values;
  a.da_values = da_values;
  a.c_values = c_values;
  a.rhs_values = rhs_values;
  a.goal_values = goal_values;
  a.a_ends = a_ends;
  a.kind[0] = kind_left;
  a.kind[1] = kind_right;
  for (int i = 0; i < 2; ++i) {
    a.kappa[i] = a.kind[i] == LSSVR_END_ROBIN ? kappa_host[i] : 0.0;
    a.g[i] = g_host[i];
    a.a_bnd[i] = a_bnd_host[i];
  }
  a.jump_free = jump_free;
  a.eta = eta;
  a.eta2 = eta2;
  a.q = q;
  a.work = static_cast<double*>(work);
  return check_launch(lssvr::estimate_goal(a, table_layout == LSSVR_TABLE_POINT_MAJOR, out4,
                                           reinterpret_cast<hipStream_t>(stream)),
                      "estimate_goal");
}

int lssvr_refine(const double* x, int64_t ne, const double* eta2, const double* eta2_max_dev, double theta,
                 double h_min, void* work, double* x_new, int64_t* parent, int64_t* ne_new_dev, void* stream) {
  if (const int rc = check_ne(ne)) return rc;
  if (!(theta >= 0.0 && theta <= 1.0)) return fail(LSSVR_ERR_SIZE, "theta = %g outside [0, 1]", theta);
  if (!(h_min >= 0.0) || !(h_min < INFINITY)) return fail(LSSVR_ERR_SIZE, "h_min = %g must be finite and >= 0", h_min);
  if (!x || !eta2 || !eta2_max_dev || !work || !x_new || !ne_new_dev)
    return fail(LSSVR_ERR_NULL, "x, eta2, eta2_max, work, x_new, ne_new must be non-NULL");
  return check_launch(lssvr::refine(x, ne, eta2, eta2_max_dev, theta, h_min, work, x_new, parent, ne_new_dev,
                                    reinterpret_cast<hipStream_t>(stream)),
                      "refine");
}

int lssvr_smoothness(const double* W, int64_t ldw, const int32_t* deg, int64_t ne, double* sigma, void* stream) {
  if (const int rc = check_ne(ne)) return rc;
  if (ldw < 2 || ldw > lssvr::kAdaptMaxM)
    return fail(LSSVR_ERR_DEGREE, "ldw = %lld outside [2, %d]", (long long)ldw, lssvr::kAdaptMaxM);
  if (!W || !deg || !sigma) return fail(LSSVR_ERR_NULL, "W, deg and sigma must be non-NULL");
  return check_launch(lssvr::smoothness(W, (int)ldw, deg, ne, sigma, reinterpret_cast<hipStream_t>(stream)),
                      "smoothness");
}

int lssvr_refine_hp(const double* x, int64_t ne, const double* eta2, const double* eta2_max_dev, double theta,
                    double h_min, const double* sigma, const int32_t* deg, double sigma_min, int dM, int M_max,
                    void* work, double* x_new, int32_t* deg_new, int64_t* parent, int64_t* ne_new_dev,
                    int64_t* counts2_dev, void* stream) {
  if (const int rc = check_ne(ne)) return rc;
  if (!(theta >= 0.0 && theta <= 1.0)) return fail(LSSVR_ERR_SIZE, "theta = %g outside [0, 1]", theta);
  if (!(h_min >= 0.0) || !(h_min < INFINITY)) return fail(LSSVR_ERR_SIZE, "h_min = %g must be finite and >= 0", h_min);
  if (dM < 1) return fail(LSSVR_ERR_DEGREE, "dM = %d < 1", dM);
  if (M_max < 2 || M_max > lssvr::kAdaptMaxM)
    return fail(LSSVR_ERR_DEGREE, "M_max = %d outside [2, %d]", M_max, lssvr::kAdaptMaxM);
  if (!x || !eta2 || !eta2_max_dev || !sigma || !deg || !work || !x_new || !deg_new || !ne_new_dev || !counts2_dev)
    return fail(LSSVR_ERR_NULL, "x, eta2, eta2_max, sigma, deg, work, x_new, deg_new, ne_new, counts2 must be "
                "non-NULL");
  return check_launch(lssvr::refine_hp(x, ne, eta2, eta2_max_dev, theta, h_min, sigma, deg, sigma_min, dM, M_max,
                                       work, x_new, deg_new, parent, ne_new_dev, counts2_dev,
                                       reinterpret_cast<hipStream_t>(stream)),
                      "refine_hp");
}

int64_t lssvr_group_work_bytes(int64_t ne) { return lssvr::group_work_bytes(ne); }

int lssvr_group_by_degree(const int32_t* deg, int64_t ne, int64_t* ids, int64_t* offsets, void* work, void* stream) {
  if (const int rc = check_ne(ne)) return rc;
  if (!deg || !ids || !offsets || !work) return fail(LSSVR_ERR_NULL, "deg, ids, offsets and work must be non-NULL");
  return check_launch(lssvr::group_by_degree(deg, ne, ids, offsets, work, reinterpret_cast<hipStream_t>(stream)),
                      "group_by_degree");
}

int lssvr_stream_probe(const double* src, double* dst, int64_t n, void* stream) {
  if (!src || !dst) return fail(LSSVR_ERR_NULL, "src and dst must be non-NULL");
  if (n < 1) return fail(LSSVR_ERR_SIZE, "n must be >= 1");
  return check_launch(lssvr::stream_probe(src, dst, n, reinterpret_cast<hipStream_t>(stream)),
                      "stream_probe");
}

int lssvr_row_chunk_probe(const double* src, double* dst, int64_t nrows, int rowlen, int chunk, void* stream) {
  if (!src || !dst) return fail(LSSVR_ERR_NULL, "src and dst must be non-NULL");
  if (nrows < 1 || rowlen < 1) return fail(LSSVR_ERR_SIZE, "nrows and rowlen must be >= 1");
  if (chunk != 8 && chunk != 16) return fail(LSSVR_ERR_SIZE, "chunk must be 8 or 16");
  return check_launch(lssvr::row_chunk_probe(src, dst, nrows, rowlen, chunk, reinterpret_cast<hipStream_t>(stream)),
                      "row_chunk_probe");
}

int lssvr_fp64_probe(double* out, int blocks, int iters, int use_mfma, void* stream) {
  if (!out) return fail(LSSVR_ERR_NULL, "out must be non-NULL");
  if (blocks < 1 || iters < 1) return fail(LSSVR_ERR_SIZE, "blocks and iters must be >= 1");
  return check_launch(lssvr::fp64_probe(out, blocks, iters, use_mfma,
                                        reinterpret_cast<hipStream_t>(stream)),
                      "fp64_probe");
}

// Eigenproblems (eigen.hip).  What the entries share beyond the common checks: nb, the four bands, the sizer.
static int bind_eig(lssvr::EigArgs& a, const double* kdiag, const double* koff, const double* mdiag,
                    const double* moff, int kind_left, int kind_right, const double* kappa_host, int64_t ne, int nb) {
  if (const int rc = check_ne(ne)) return rc;
  if (nb < 1 || nb > 8) return fail(LSSVR_ERR_SIZE, "nb = %d outside [1, 8]", nb);
  if (!kdiag || !koff || !mdiag || !moff) return fail(LSSVR_ERR_NULL, "kdiag, koff, mdiag, moff must be non-NULL");
  Ends e{kind_left, kind_right, kappa_host};
  if (const int rc = check_ends(e, true)) return rc;
  a.kdiag = kdiag;
  a.koff = koff;
  a.mdiag = mdiag;
  a.moff = moff;
  a.ne = ne;
  a.nb = nb;
  a.f0 = e.f0;
  a.f1 = e.f1;
  a.k0 = e.k0;
  a.k1 = e.k1;
  return LSSVR_OK;
}

static int check_eig_work(const void* work, int64_t work_bytes, int64_t ne, int nb) {
  return check_work_sized(work, work_bytes, lssvr::eig_work_bytes(ne, nb), "lssvr_eig_work_bytes", ne, nb);
}

int64_t lssvr_eig_work_bytes(int64_t ne, int nb) { return lssvr::eig_work_bytes(ne, nb); }

int lssvr_eig_apply(const double* kdiag, const double* koff, const double* mdiag, const double* moff, int kind_left,
                    int kind_right, const double* kappa_host, int64_t ne, int nb, const double* Z, double* MZ,
                    double* KZ, double* gram, void* work, int64_t work_bytes, void* stream) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne = %lld < 0", (long long)ne);
  if (ne == 0) return LSSVR_OK;
  lssvr::EigArgs a{};
  int rc = bind_eig(a, kdiag, koff, mdiag, moff, kind_left, kind_right, kappa_host, ne, nb);
  if (rc != LSSVR_OK) return rc;
  if (!Z || !MZ || !KZ || !gram) return fail(LSSVR_ERR_NULL, "Z, MZ, KZ, gram must be non-NULL");
  rc = check_eig_work(work, work_bytes, ne, nb);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::eig_apply(a, Z, MZ, KZ, gram, work, reinterpret_cast<hipStream_t>(stream)), "eig_apply");
}

static int check_ritz(const double* A, const double* B, int nb, double sigma, const double* theta, const double* Q) {
  if (nb < 1 || nb > 8) return fail(LSSVR_ERR_SIZE, "nb = %d outside [1, 8]", nb);
  if (!A || !B || !theta || !Q) return fail(LSSVR_ERR_NULL, "A, B, theta, Q must be non-NULL");
  if (!is_finite(sigma)) return fail(LSSVR_ERR_SIZE, "sigma = %g must be finite", sigma);
  return LSSVR_OK;
}

int lssvr_eig_ritz(const double* A, const double* B, int nb, double sigma, double* theta, double* Q, int32_t* info,
                   void* stream) {
  const int rc = check_ritz(A, B, nb, sigma, theta, Q);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::eig_ritz_device(A, B, nb, sigma, theta, Q, info, reinterpret_cast<hipStream_t>(stream)),
                      "eig_ritz");
}

int lssvr_eig_ritz_host(const double* A_host, const double* B_host, int nb, double sigma, double* theta_host,
                        double* Q_host, int32_t* info) {
  const int rc = check_ritz(A_host, B_host, nb, sigma, theta_host, Q_host);
  if (rc != LSSVR_OK) return rc;
  const int bad = lssvr::eig_ritz_host(A_host, B_host, nb, sigma, theta_host, Q_host);
  if (info) info[0] = bad;
  return LSSVR_OK;
}

int lssvr_eig_rotate(const double* Z, const double* MZ, const double* KZ, const double* Q, const double* theta,
                     int kind_left, int kind_right, int64_t ne, int nb, double* X, double* Y, double* res2, void* work,
                     int64_t work_bytes, void* stream) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne = %lld < 0", (long long)ne);
  if (ne == 0) return LSSVR_OK;
  if (const int rc = check_ne(ne)) return rc;
  if (nb < 1 || nb > 8) return fail(LSSVR_ERR_SIZE, "nb = %d outside [1, 8]", nb);
  if (!Z || !MZ || !KZ || !Q || !theta || !X || !Y || !res2)
    return fail(LSSVR_ERR_NULL, "Z, MZ, KZ, Q, theta, X, Y, res2 must be non-NULL");
  if (const int rc = check_kinds(kind_left, kind_right)) return rc;
  const int rc = check_eig_work(work, work_bytes, ne, nb);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::eig_rotate(Z, MZ, KZ, Q, theta, ne, nb, kind_left == LSSVR_END_ROBIN,
                                        kind_right == LSSVR_END_ROBIN, X, Y, res2, work,
                                        reinterpret_cast<hipStream_t>(stream)),
                      "eig_rotate");
}

static int bind_eig_count(lssvr::EigArgs& a, const double* kdiag, const double* koff, const double* mdiag,
                          const double* moff, int kind_left, int kind_right, const double* kappa_host, int64_t ne,
                          const double* shifts, int ns, double pivmin, const int32_t* counts) {
  if (ns < 0) return fail(LSSVR_ERR_SIZE, "ns = %d < 0", ns);
  const int rc = bind_eig(a, kdiag, koff, mdiag, moff, kind_left, kind_right, kappa_host, ne, 1);
  if (rc != LSSVR_OK) return rc;
  if (ns > 0 && (!shifts || !counts)) return fail(LSSVR_ERR_NULL, "shifts and counts must be non-NULL");
  if (!(pivmin > 0.0 && is_finite(pivmin))) return fail(LSSVR_ERR_SIZE, "pivmin = %g must be finite and > 0", pivmin);
  return LSSVR_OK;
}

int lssvr_eig_count(const double* kdiag, const double* koff, const double* mdiag, const double* moff, int kind_left,
                    int kind_right, const double* kappa_host, int64_t ne, const double* shifts, int ns, double pivmin,
                    int32_t* counts, void* stream) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne = %lld < 0", (long long)ne);
  if (ne == 0) return LSSVR_OK;
  lssvr::EigArgs a{};
  const int rc = bind_eig_count(a, kdiag, koff, mdiag, moff, kind_left, kind_right, kappa_host, ne, shifts, ns, pivmin,
                                counts);
  if (rc != LSSVR_OK) return rc;
  if (ns == 0) return LSSVR_OK;
  return check_launch(lssvr::eig_count_device(a, shifts, ns, pivmin, counts, reinterpret_cast<hipStream_t>(stream)),
                      "eig_count");
}

int lssvr_eig_count_host(const double* kdiag_host, const double* koff_host, const double* mdiag_host,
                         const double* moff_host, int kind_left, int kind_right, const double* kappa_host, int64_t ne,
                         const double* shifts_host, int ns, double pivmin, int32_t* counts) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne = %lld < 0", (long long)ne);
  if (ne == 0) return LSSVR_OK;
  lssvr::EigArgs a{};
  const int rc = bind_eig_count(a, kdiag_host, koff_host, mdiag_host, moff_host, kind_left, kind_right, kappa_host, ne,
                                shifts_host, ns, pivmin, counts);
  if (rc != LSSVR_OK) return rc;
  lssvr::eig_count_host(a, shifts_host, ns, pivmin, counts);
  return LSSVR_OK;
}

int lssvr_eig_rayleigh(const double* x, const double* W, int64_t ne, int M, int nq, const double* a_values,
                       const double* c_values, const double* rho_values, int table_layout, int kind_left,
                       int kind_right, const double* kappa_host, double* out3, void* work, void* stream) {
  if (ne < 0) return fail(LSSVR_ERR_SIZE, "ne = %lld < 0", (long long)ne);
  if (ne == 0) return LSSVR_OK;
  if (const int rc = check_ne(ne)) return rc;
  if (M < 1 || M > lssvr::kAdaptMaxM) return fail(LSSVR_ERR_DEGREE, "M = %d outside [1, %d]", M, lssvr::kAdaptMaxM);
  if (nq < 1 || nq > lssvr::kAdaptMaxNq)
    return fail(LSSVR_ERR_QUAD, "nq = %d outside [1, %d]", nq, lssvr::kAdaptMaxNq);
  if (!x || !W || !out3 || !work) return fail(LSSVR_ERR_NULL, "x, W, out3, work must be non-NULL");
  if (!a_values || !c_values || !rho_values)
    return fail(LSSVR_ERR_NULL, "a_values, c_values and rho_values must be non-NULL");
  if (const int rc = check_layout(table_layout)) return rc;
  Ends e{kind_left, kind_right, kappa_host};
  if (const int rc = check_ends(e, true)) return rc;
  lssvr::EigRayleighArgs a{};
  a.x = x;
  a.W = W;
  a.ne = ne;
  a.M = M;
  a.nq = nq;
  a.a_values = a_values;
  a.c_values = c_values;
  a.rho_values = rho_values;
  a.kind[0] = kind_left;
  a.kind[1] = kind_right;
  a.kappa[0] = e.k0;
  a.kappa[1] = e.k1;
  a.work = work;
  return check_launch(lssvr::eig_rayleigh(a, table_layout == LSSVR_TABLE_POINT_MAJOR, out3,
                                          reinterpret_cast<hipStream_t>(stream)),
                      "eig_rayleigh");
}

// Transient problems (timestep.hip).  The device and the host entry of each pair share one validated binding, made of
// the common checks above and the entry's own NULL list and aliasing rules.
static int bind_ts_rhs(lssvr::TsRhsArgs& a, const double* mdiag, const double* moff, const double* U0,
                       const double* U1, const double* loads, const double* phi, int64_t ne, int nc, int R,
                       double beta0, double beta1, double inv_dt, const double* out) {
  if (const int rc = check_ne(ne)) return rc;
  if (nc < 1 || nc > 8) return fail(LSSVR_ERR_SIZE, "nc = %d outside [1, 8]", nc);
  if (R < 1 || R > 8) return fail(LSSVR_ERR_SIZE, "R = %d outside [1, 8]", R);
  if (!is_finite(beta0) || !is_finite(beta1) || !is_finite(inv_dt))
    return fail(LSSVR_ERR_SIZE, "beta0 = %g, beta1 = %g, inv_dt = %g must be finite", beta0, beta1, inv_dt);
  if (!mdiag || !moff || !U0 || !loads || !phi || !out)
    return fail(LSSVR_ERR_NULL, "mdiag, moff, U0, loads, phi, out must be non-NULL");
  if (beta1 != 0.0 && !U1) return fail(LSSVR_ERR_NULL, "U1 must be non-NULL when beta1 != 0");
  if (out == U0 || (beta1 != 0.0 && out == U1)) return fail(LSSVR_ERR_SIZE, "out must not be U0 or U1");
  a = lssvr::TsRhsArgs{mdiag, moff, U0, U1, loads, phi, ne, nc, R, beta0, beta1, inv_dt};
  return LSSVR_OK;
}

int lssvr_ts_rhs(const double* mdiag, const double* moff, const double* U0, const double* U1, const double* loads,
                 const double* phi, int64_t ne, int nc, int R, double beta0, double beta1, double inv_dt, double* out,
                 void* stream) {
  lssvr::TsRhsArgs a{};
  const int rc = bind_ts_rhs(a, mdiag, moff, U0, U1, loads, phi, ne, nc, R, beta0, beta1, inv_dt, out);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::ts_rhs(a, out, reinterpret_cast<hipStream_t>(stream)), "ts_rhs");
}

int lssvr_ts_rhs_host(const double* mdiag_host, const double* moff_host, const double* U0_host, const double* U1_host,
                      const double* loads_host, const double* phi_host, int64_t ne, int nc, int R, double beta0,
                      double beta1, double inv_dt, double* out_host) {
  lssvr::TsRhsArgs a{};
  const int rc = bind_ts_rhs(a, mdiag_host, moff_host, U0_host, U1_host, loads_host, phi_host, ne, nc, R, beta0, beta1,
                             inv_dt, out_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::ts_rhs_host(a, out_host);
  return LSSVR_OK;
}

static int bind_ts_source(lssvr::TsSourceArgs& a, const double* U2, const double* U0, const double* U1,
                          const double* ftab, const double* rho_tab, const double* phi, int64_t ne, int n_colloc,
                          int R, int table_layout, double alpha, double beta0, double beta1, double inv_dt,
                          const double* out) {
  if (const int rc = check_ne(ne)) return rc;
  if (n_colloc < 2 || n_colloc > 4096) return fail(LSSVR_ERR_SIZE, "n_colloc = %d outside [2, 4096]", n_colloc);
  if (R < 1 || R > 8) return fail(LSSVR_ERR_SIZE, "R = %d outside [1, 8]", R);
  if (const int rc = check_layout(table_layout)) return rc;
  if (!is_finite(alpha) || !is_finite(beta0) || !is_finite(beta1) || !is_finite(inv_dt))
    return fail(LSSVR_ERR_SIZE, "alpha = %g, beta0 = %g, beta1 = %g, inv_dt = %g must be finite", alpha, beta0, beta1,
                inv_dt);
  if (!U2 || !U0 || !ftab || !rho_tab || !phi || !out)
    return fail(LSSVR_ERR_NULL, "U2, U0, ftab, rho_tab, phi, out must be non-NULL");
  if (beta1 != 0.0 && !U1) return fail(LSSVR_ERR_NULL, "U1 must be non-NULL when beta1 != 0");
  a = lssvr::TsSourceArgs{U2, U0, U1, ftab, rho_tab, phi, ne, n_colloc, R, alpha, beta0, beta1, inv_dt};
  return LSSVR_OK;
}

int lssvr_ts_source_table(const double* U2, const double* U0, const double* U1, const double* ftab,
                          const double* rho_tab, const double* phi, int64_t ne, int n_colloc, int R, int table_layout,
                          double alpha, double beta0, double beta1, double inv_dt, double* out, void* stream) {
  lssvr::TsSourceArgs a{};
  const int rc = bind_ts_source(a, U2, U0, U1, ftab, rho_tab, phi, ne, n_colloc, R, table_layout, alpha, beta0, beta1,
                                inv_dt, out);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::ts_source_table(a, table_layout == LSSVR_TABLE_POINT_MAJOR, out,
                                             reinterpret_cast<hipStream_t>(stream)),
                      "ts_source_table");
}

int lssvr_ts_source_table_host(const double* U2_host, const double* U0_host, const double* U1_host,
                               const double* ftab_host, const double* rho_tab_host, const double* phi_host, int64_t ne,
                               int n_colloc, int R, int table_layout, double alpha, double beta0, double beta1,
                               double inv_dt, double* out_host) {
  lssvr::TsSourceArgs a{};
  const int rc = bind_ts_source(a, U2_host, U0_host, U1_host, ftab_host, rho_tab_host, phi_host, ne, n_colloc, R,
                                table_layout, alpha, beta0, beta1, inv_dt, out_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::ts_source_table_host(a, table_layout == LSSVR_TABLE_POINT_MAJOR, out_host);
  return LSSVR_OK;
}

// Adaptive time stepping (timestep_adapt.hip).  The device and the host entry of each pair share one validated binding.
static int ts_misaligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % alignof(double) != 0) return 1;
  return 0;
}

static int bind_ts_step(lssvr::TsStepArgs& a, const double* kdiag, const double* koff, const double* mdiag,
                        const double* moff, const double* U0, const double* U1, const double* loads,
                        const double* phi, int64_t ne, int R, double s, double beta0, double beta1, double inv_dt,
                        int write_bands, double* adiag, double* aoff, const double* b) {
  const int rc = bind_ts_rhs(a.rhs, mdiag, moff, U0, U1, loads, phi, ne, 1, R, beta0, beta1, inv_dt, b);
  if (rc != LSSVR_OK) return rc;
  if (!is_finite(s)) return fail(LSSVR_ERR_SIZE, "s = %g must be finite", s);
  if (write_bands != 0 && write_bands != 1) return fail(LSSVR_ERR_SIZE, "write_bands = %d must be 0 or 1", write_bands);
  if (write_bands && (!kdiag || !koff || !adiag || !aoff))
    return fail(LSSVR_ERR_NULL, "kdiag, koff, adiag, aoff must be non-NULL with write_bands");
  if (ts_misaligned({kdiag, koff, mdiag, moff, U0, U1, loads, phi, adiag, aoff, b}))
    return fail(LSSVR_ERR_SIZE, "every array must be aligned to 8 bytes");
  if (write_bands) {
    for (const double* o : {(const double*)adiag, (const double*)aoff, b})
      if (o == kdiag || o == koff || o == mdiag || o == moff || o == loads || o == phi || o == U0 ||
          (beta1 != 0.0 && o == U1))
        return fail(LSSVR_ERR_SIZE, "an output must not be one of the inputs");
    if (adiag == aoff || adiag == b || aoff == b) return fail(LSSVR_ERR_SIZE, "adiag, aoff, b must be distinct");
  } else if (b == mdiag || b == moff || b == loads || b == phi) {
    return fail(LSSVR_ERR_SIZE, "an output must not be one of the inputs");
  }
  a.kdiag = kdiag;
  a.koff = koff;
  a.s = s;
  a.write_bands = write_bands;
  a.adiag = adiag;
  a.aoff = aoff;
  return LSSVR_OK;
}

int lssvr_ts_step(const double* kdiag, const double* koff, const double* mdiag, const double* moff, const double* U0,
                  const double* U1, const double* loads, const double* phi, int64_t ne, int R, double s, double beta0,
                  double beta1, double inv_dt, int write_bands, double* adiag, double* aoff, double* b, void* stream) {
  lssvr::TsStepArgs a{};
  const int rc = bind_ts_step(a, kdiag, koff, mdiag, moff, U0, U1, loads, phi, ne, R, s, beta0, beta1, inv_dt,
                              write_bands, adiag, aoff, b);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::ts_step(a, b, reinterpret_cast<hipStream_t>(stream)), "ts_step");
}

int lssvr_ts_step_host(const double* kdiag_host, const double* koff_host, const double* mdiag_host,
                       const double* moff_host, const double* U0_host, const double* U1_host, const double* loads_host,
                       const double* phi_host, int64_t ne, int R, double s, double beta0, double beta1, double inv_dt,
                       int write_bands, double* adiag_host, double* aoff_host, double* b_host) {
  lssvr::TsStepArgs a{};
  const int rc = bind_ts_step(a, kdiag_host, koff_host, mdiag_host, moff_host, U0_host, U1_host, loads_host, phi_host,
                              ne, R, s, beta0, beta1, inv_dt, write_bands, adiag_host, aoff_host, b_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::ts_step_host(a, b_host);
  return LSSVR_OK;
}

int64_t lssvr_ts_error_work_bytes(int64_t ne) { return lssvr::ts_error_work_bytes(ne); }

static int bind_ts_error(lssvr::TsErrArgs& a, const double* U3, const double* U2, const double* U1, const double* U0,
                         int kind_left, int kind_right, int64_t ne, double w3, double w2, double w1, double w0,
                         double atol, double rtol, const double* out4) {
  if (const int rc = check_ne(ne)) return rc;
  if (const int rc = check_kinds(kind_left, kind_right)) return rc;
  if (!is_finite(w3) || !is_finite(w2) || !is_finite(w1) || !is_finite(w0))
    return fail(LSSVR_ERR_SIZE, "w3 = %g, w2 = %g, w1 = %g, w0 = %g must be finite", w3, w2, w1, w0);
  if (!is_finite(atol) || !is_finite(rtol) || atol < 0.0 || rtol < 0.0 || !(atol + rtol > 0.0))
    return fail(LSSVR_ERR_SIZE, "atol = %g, rtol = %g must be finite and >= 0, their sum > 0", atol, rtol);
  if (!U3 || !U2 || !out4) return fail(LSSVR_ERR_NULL, "U3, U2, out4 must be non-NULL");
  if (w1 != 0.0 && !U1) return fail(LSSVR_ERR_NULL, "U1 must be non-NULL when w1 != 0");
  if (w0 != 0.0 && !U0) return fail(LSSVR_ERR_NULL, "U0 must be non-NULL when w0 != 0");
  if (ts_misaligned({U3, U2, U1, U0, out4})) return fail(LSSVR_ERR_SIZE, "every array must be aligned to 8 bytes");
  a = lssvr::TsErrArgs{U3, U2, U1, U0, ne, {kind_left, kind_right}, w3, w2, w1, w0, atol, rtol};
  return LSSVR_OK;
}

int lssvr_ts_error(const double* U3, const double* U2, const double* U1, const double* U0, int kind_left,
                   int kind_right, int64_t ne, double w3, double w2, double w1, double w0, double atol, double rtol,
                   double* out4, void* work, int64_t work_bytes, void* stream) {
  lssvr::TsErrArgs a{};
  int rc = bind_ts_error(a, U3, U2, U1, U0, kind_left, kind_right, ne, w3, w2, w1, w0, atol, rtol, out4);
  if (rc != LSSVR_OK) return rc;
  if (ts_misaligned({work})) return fail(LSSVR_ERR_SIZE, "work must be aligned to 8 bytes");      // (NULL is aligned)
  rc = check_work_sized(work, work_bytes, lssvr::ts_error_work_bytes(ne), "lssvr_ts_error_work_bytes", ne);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::ts_error(a, out4, work, reinterpret_cast<hipStream_t>(stream)), "ts_error");
}

int lssvr_ts_error_host(const double* U3_host, const double* U2_host, const double* U1_host, const double* U0_host,
                        int kind_left, int kind_right, int64_t ne, double w3, double w2, double w1, double w0,
                        double atol, double rtol, double* out4_host) {
  lssvr::TsErrArgs a{};
  const int rc = bind_ts_error(a, U3_host, U2_host, U1_host, U0_host, kind_left, kind_right, ne, w3, w2, w1, w0, atol,
                               rtol, out4_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::ts_error_host(a, out4_host);
  return LSSVR_OK;
}

// Semilinear problems (nonlinear.hip).  The device and the host entry of each pair share one validated binding.
static int bind_nl_linearize(lssvr::NlLinArgs& a, const double* u, const double* t_local, const double* q_tabs,
                             const double* c_tab, const double* f_tab, int64_t ne, int n, int table_layout, int kind,
                             int nterm, double* c_eff, double* f_eff, double* f_res) {
  if (const int rc = check_ne(ne)) return rc;
  if (n < 1 || n > 64) return fail(LSSVR_ERR_SIZE, "n = %d outside [1, 64]", n);
  if (const int rc = check_layout(table_layout)) return rc;
  if (const int rc = check_nl_kind(kind, nterm)) return rc;
  if (!u || !t_local || !q_tabs || !f_tab) return fail(LSSVR_ERR_NULL, "u, t_local, q_tabs, f_tab must be non-NULL");
  if (!c_eff && !f_eff && !f_res) return fail(LSSVR_ERR_NULL, "one of c_eff, f_eff, f_res must be non-NULL");
  for (const double* o : {(const double*)c_eff, (const double*)f_eff, (const double*)f_res})
    if (o && (o == u || o == t_local || o == q_tabs || o == c_tab || o == f_tab))
      return fail(LSSVR_ERR_SIZE, "an output must not be one of the inputs");
  if ((c_eff && (c_eff == f_eff || c_eff == f_res)) || (f_eff && f_eff == f_res))
    return fail(LSSVR_ERR_SIZE, "c_eff, f_eff, f_res must be distinct");
  a = lssvr::NlLinArgs{u, t_local, q_tabs, c_tab, f_tab, ne, n, kind, nterm, c_eff, f_eff, f_res};
  return LSSVR_OK;
}

int lssvr_nl_linearize(const double* u, const double* t_local, const double* q_tabs, const double* c_tab,
                       const double* f_tab, int64_t ne, int n, int table_layout, int kind, int nterm, double* c_eff,
                       double* f_eff, double* f_res, void* stream) {
  lssvr::NlLinArgs a{};
  const int rc = bind_nl_linearize(a, u, t_local, q_tabs, c_tab, f_tab, ne, n, table_layout, kind, nterm, c_eff, f_eff,
                                   f_res);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::nl_linearize(a, table_layout == LSSVR_TABLE_POINT_MAJOR,
                                          reinterpret_cast<hipStream_t>(stream)),
                      "nl_linearize");
}

int lssvr_nl_linearize_host(const double* u_host, const double* t_local_host, const double* q_tabs_host,
                            const double* c_tab_host, const double* f_tab_host, int64_t ne, int n, int table_layout,
                            int kind, int nterm, double* c_eff_host, double* f_eff_host, double* f_res_host) {
  lssvr::NlLinArgs a{};
  const int rc = bind_nl_linearize(a, u_host, t_local_host, q_tabs_host, c_tab_host, f_tab_host, ne, n, table_layout,
                                   kind, nterm, c_eff_host, f_eff_host, f_res_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::nl_linearize_host(a, table_layout == LSSVR_TABLE_POINT_MAJOR);
  return LSSVR_OK;
}

int64_t lssvr_nl_residual_work_bytes(int64_t ne) { return lssvr::nl_residual_work_bytes(ne); }

static int bind_nl_residual(lssvr::NlResArgs& a, const double* diag, const double* sub, const double* sup,
                            const double* load, const double* u, const double* u_new, int kind_left, int kind_right,
                            const double* end_values, const double* kappa_host, int64_t ne, const double* out4) {
  if (const int rc = check_ne(ne)) return rc;
  Ends e{kind_left, kind_right, kappa_host};
  if (const int rc = check_ends(e, true)) return rc;
  if (!diag || !sub || !sup || !load || !u || !u_new || !out4)
    return fail(LSSVR_ERR_NULL, "diag, sub, sup, load, u, u_new, out4 must be non-NULL");
  if ((e.f0 || e.f1) && !end_values) return fail(LSSVR_ERR_NULL, "end_values must be non-NULL with a Robin end");
  a = lssvr::NlResArgs{diag, sub, sup, load, u, u_new, end_values, ne, {kind_left, kind_right}, {e.k0, e.k1}};
  return LSSVR_OK;
}

int lssvr_nl_residual(const double* diag, const double* sub, const double* sup, const double* load, const double* u,
                      const double* u_new, int kind_left, int kind_right, const double* end_values,
                      const double* kappa_host, int64_t ne, double* out4, void* work, int64_t work_bytes,
                      void* stream) {
  lssvr::NlResArgs a{};
  int rc = bind_nl_residual(a, diag, sub, sup, load, u, u_new, kind_left, kind_right, end_values, kappa_host, ne, out4);
  if (rc != LSSVR_OK) return rc;
  rc = check_work_sized(work, work_bytes, lssvr::nl_residual_work_bytes(ne), "lssvr_nl_residual_work_bytes", ne);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::nl_residual(a, out4, work, reinterpret_cast<hipStream_t>(stream)), "nl_residual");
}

int lssvr_nl_residual_host(const double* diag_host, const double* sub_host, const double* sup_host,
                           const double* load_host, const double* u_host, const double* u_new_host, int kind_left,
                           int kind_right, const double* end_values_host, const double* kappa_host, int64_t ne,
                           double* out4_host) {
  lssvr::NlResArgs a{};
  const int rc = bind_nl_residual(a, diag_host, sub_host, sup_host, load_host, u_host, u_new_host, kind_left,
                                  kind_right, end_values_host, kappa_host, ne, out4_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::nl_residual_host(a, out4_host);
  return LSSVR_OK;
}

static int check_nl_step(const double* u, const double* u_new, double lambda, int64_t ne, const double* out) {
  if (const int rc = check_ne(ne)) return rc;
  if (!is_finite(lambda)) return fail(LSSVR_ERR_SIZE, "lambda = %g must be finite", lambda);
  if (!u || !u_new || !out) return fail(LSSVR_ERR_NULL, "u, u_new, out must be non-NULL");
  if (out == u || out == u_new) return fail(LSSVR_ERR_SIZE, "out must not be u or u_new");
  return LSSVR_OK;
}

int lssvr_nl_step(const double* u, const double* u_new, double lambda, int64_t ne, double* out, void* stream) {
  const int rc = check_nl_step(u, u_new, lambda, ne, out);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::nl_step(u, u_new, lambda, ne, out, reinterpret_cast<hipStream_t>(stream)), "nl_step");
}

int lssvr_nl_step_host(const double* u_host, const double* u_new_host, double lambda, int64_t ne, double* out_host) {
  const int rc = check_nl_step(u_host, u_new_host, lambda, ne, out_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::nl_step_host(u_host, u_new_host, lambda, ne, out_host);
  return LSSVR_OK;
}

// Semilinear transient problems (timestep_nl.hip).  The device and the host entry share one validated binding.
static int bind_ts_nl_assemble(lssvr::TsNlArgs& a, const double* x, const double* u, const double* a_quad,
                               const double* cs_quad, const double* q_quad, const double* r, int64_t ne, int nquad,
                               int kind, int nterm, double* diag, double* off, double* rhs) {
  if (const int rc = check_ne(ne)) return rc;
  if (nquad < 1 || nquad > 5) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  if (const int rc = check_nl_kind(kind, nterm)) return rc;
  if (!x || !u || !cs_quad || !q_quad || !r || !diag || !off || !rhs)
    return fail(LSSVR_ERR_NULL, "x, u, cs_quad, q_quad, r, diag, off, rhs must be non-NULL");
  for (const double* o : {(const double*)diag, (const double*)off, (const double*)rhs})
    if (o == x || o == u || o == a_quad || o == cs_quad || o == q_quad || o == r)
      return fail(LSSVR_ERR_SIZE, "an output must not be one of the inputs");
  if (diag == off || diag == rhs || off == rhs) return fail(LSSVR_ERR_SIZE, "diag, off, rhs must be distinct");
  a = lssvr::TsNlArgs{x, u, a_quad, cs_quad, q_quad, r, ne, nquad, kind, nterm, diag, off, rhs};
  return LSSVR_OK;
}

int lssvr_ts_nl_assemble(const double* x, const double* u, const double* a_quad, const double* cs_quad,
                         const double* q_quad, const double* r, int64_t ne, int nquad, int kind, int nterm,
                         double* diag, double* off, double* rhs, void* stream) {
  lssvr::TsNlArgs a{};
  const int rc = bind_ts_nl_assemble(a, x, u, a_quad, cs_quad, q_quad, r, ne, nquad, kind, nterm, diag, off, rhs);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::ts_nl_assemble(a, reinterpret_cast<hipStream_t>(stream)), "ts_nl_assemble");
}

int lssvr_ts_nl_assemble_host(const double* x_host, const double* u_host, const double* a_quad_host,
                              const double* cs_quad_host, const double* q_quad_host, const double* r_host, int64_t ne,
                              int nquad, int kind, int nterm, double* diag_host, double* off_host, double* rhs_host) {
  lssvr::TsNlArgs a{};
  const int rc = bind_ts_nl_assemble(a, x_host, u_host, a_quad_host, cs_quad_host, q_quad_host, r_host, ne, nquad, kind,
                                     nterm, diag_host, off_host, rhs_host);
  if (rc != LSSVR_OK) return rc;
  if (!lssvr::ts_nl_assemble_host(a)) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  return LSSVR_OK;
}

// Wave problems (wave.hip).  The device and the host entry share one validated binding.
static int bind_wave_advance(lssvr::WaveArgs& a, const double* U_new, const double* U, const double* V,
                             const double* Acc, const double* mdiag, const double* moff, const double* ddiag,
                             const double* doff, const double* loads, const double* phi, int64_t ne, int nc, int R,
                             double dt, double beta, double gamma, const double* V_out, const double* Acc_out,
                             const double* rhs_out) {
  if (const int rc = check_ne(ne)) return rc;
  if (nc < 1 || nc > 8) return fail(LSSVR_ERR_SIZE, "nc = %d outside [1, 8]", nc);
  if (R < 1 || R > 8) return fail(LSSVR_ERR_SIZE, "R = %d outside [1, 8]", R);
  if (!(is_finite(dt) && dt > 0.0) || !(is_finite(beta) && beta > 0.0) || !(is_finite(gamma) && gamma > 0.0))
    return fail(LSSVR_ERR_SIZE, "dt = %g, beta = %g, gamma = %g must be finite and > 0", dt, beta, gamma);
  if (!U_new && !rhs_out)
    return fail(LSSVR_ERR_SIZE, "U_new and rhs_out are both NULL: there is nothing to compute");
  if (!U || !V || !Acc) return fail(LSSVR_ERR_NULL, "U, V, Acc must be non-NULL");
  if (U_new && (!V_out || !Acc_out)) return fail(LSSVR_ERR_NULL, "V_out, Acc_out must be non-NULL with U_new");
  if (rhs_out && (!mdiag || !moff || !loads || !phi))
    return fail(LSSVR_ERR_NULL, "mdiag, moff, loads, phi must be non-NULL with rhs_out");
  if (rhs_out && ddiag && !doff) return fail(LSSVR_ERR_NULL, "doff must be non-NULL with ddiag");
  if (U_new) {
    // a thread recomputes its neighbours' correctors from the old arrays while their owners write the new ones
    if (V_out == V || V_out == Acc || Acc_out == V || Acc_out == Acc || V_out == U || Acc_out == U ||
        V_out == U_new || Acc_out == U_new)
      return fail(LSSVR_ERR_SIZE, "V_out, Acc_out must not be V, Acc, U or U_new (neighbours read the old values)");
    if (V_out == Acc_out) return fail(LSSVR_ERR_SIZE, "V_out and Acc_out must differ");
  }
  if (rhs_out) {
    if (rhs_out == U || rhs_out == V || rhs_out == Acc || rhs_out == U_new || rhs_out == loads)
      return fail(LSSVR_ERR_SIZE, "rhs_out must not be U_new, U, V, Acc or loads");
    if (U_new && (rhs_out == V_out || rhs_out == Acc_out))
      return fail(LSSVR_ERR_SIZE, "rhs_out must not be V_out or Acc_out");
  }
  a = lssvr::WaveArgs{U_new, U, V, Acc, mdiag, moff, ddiag, ddiag ? doff : nullptr, loads, phi, ne, nc, R};
  lssvr::wave_coefficients(a, dt, beta, gamma);
  return LSSVR_OK;
}

int lssvr_wave_advance(const double* U_new, const double* U, const double* V, const double* Acc, const double* mdiag,
                       const double* moff, const double* ddiag, const double* doff, const double* loads,
                       const double* phi, int64_t ne, int nc, int R, double dt, double beta, double gamma,
                       double* V_out, double* Acc_out, double* rhs_out, void* stream) {
  lssvr::WaveArgs a{};
  const int rc = bind_wave_advance(a, U_new, U, V, Acc, mdiag, moff, ddiag, doff, loads, phi, ne, nc, R, dt, beta,
                                   gamma, V_out, Acc_out, rhs_out);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::wave_advance(a, V_out, Acc_out, rhs_out, reinterpret_cast<hipStream_t>(stream)),
                      "wave_advance");
}

int lssvr_wave_advance_host(const double* U_new_host, const double* U_host, const double* V_host,
                            const double* Acc_host, const double* mdiag_host, const double* moff_host,
                            const double* ddiag_host, const double* doff_host, const double* loads_host,
                            const double* phi_host, int64_t ne, int nc, int R, double dt, double beta, double gamma,
                            double* V_out_host, double* Acc_out_host, double* rhs_out_host) {
  lssvr::WaveArgs a{};
  const int rc = bind_wave_advance(a, U_new_host, U_host, V_host, Acc_host, mdiag_host, moff_host, ddiag_host,
                                   doff_host, loads_host, phi_host, ne, nc, R, dt, beta, gamma, V_out_host,
                                   Acc_out_host, rhs_out_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::wave_advance_host(a, V_out_host, Acc_out_host, rhs_out_host);
  return LSSVR_OK;
}

// Adjoint sensitivities (sensitivity.hip).  The device and the host entry share one validated binding.
// (tables_optional: an entry with outputs of its own, which checks that one of them is given)
static int bind_sens(lssvr::SensArgs& a, const double* x, int64_t ne, int nquad, const double* U, int nu,
                     const double* Z, int nc, double* ga, double* gb, double* gc, double* gf, const double* P,
                     const double* band_ends, int kind_left, int kind_right, double* out_ends,
                     bool tables_optional = false) {
  if (const int rc = check_ne(ne)) return rc;
  if (nc < 1 || nc > 8) return fail(LSSVR_ERR_SIZE, "nc = %d outside [1, 8]", nc);
  if (nu != 1 && nu != nc) return fail(LSSVR_ERR_SIZE, "nu = %d must be 1 or nc = %d", nu, nc);
  if (nquad < 1 || nquad > 5) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  if (!x || !U || !Z) return fail(LSSVR_ERR_NULL, "x, U, Z must be non-NULL");
  if (!tables_optional && !ga && !gb && !gc && !gf)
    return fail(LSSVR_ERR_NULL, "one of ga, gb, gc, gf must be non-NULL");
  if (out_ends) {
    if (!band_ends) return fail(LSSVR_ERR_NULL, "band_ends must be non-NULL with out_ends");
    if (const int rc = check_kinds(kind_left, kind_right)) return rc;
  }
  a = lssvr::SensArgs{x, U, Z, P, band_ends, ne, nquad, nu, nc, {kind_left, kind_right}, ga, gb, gc, gf, out_ends};
  return LSSVR_OK;
}

int lssvr_p1_sensitivity(const double* x, int64_t ne, int nquad, const double* U, int nu, const double* Z, int nc,
                         double* ga, double* gb, double* gc, double* gf, const double* P, const double* band_ends,
                         int kind_left, int kind_right, double* out_ends, void* stream) {
  lssvr::SensArgs a{};
  const int rc = bind_sens(a, x, ne, nquad, U, nu, Z, nc, ga, gb, gc, gf, P, band_ends, kind_left, kind_right,
                           out_ends);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::p1_sensitivity(a, reinterpret_cast<hipStream_t>(stream)), "p1_sensitivity");
}

int lssvr_p1_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* U_host, int nu,
                              const double* Z_host, int nc, double* ga_host, double* gb_host, double* gc_host,
                              double* gf_host, const double* P_host, const double* band_ends_host, int kind_left,
                              int kind_right, double* out_ends_host) {
  lssvr::SensArgs a{};
  const int rc = bind_sens(a, x_host, ne, nquad, U_host, nu, Z_host, nc, ga_host, gb_host, gc_host, gf_host, P_host,
                           band_ends_host, kind_left, kind_right, out_ends_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::p1_sensitivity_host(a);          // (nquad is checked above: the rule exists)
  return LSSVR_OK;
}

// Adjoint sensitivities of the semilinear solve (nl_sensitivity.hip): the binding above, then the law and its tables.
static int bind_nl_sens(lssvr::NlSensArgs& a, const double* x, int64_t ne, int nquad, const double* U, int nu,
                        const double* Z, int nc, const double* q_tabs, int kind, int nterm, double* ga, double* gb,
                        double* gc, double* gf, double* gq, const double* P, const double* band_ends, int kind_left,
                        int kind_right, double* out_ends) {
  if (const int rc = bind_sens(a.s, x, ne, nquad, U, nu, Z, nc, ga, gb, gc, gf, P, band_ends, kind_left, kind_right,
                               out_ends, true))
    return rc;
  if (!ga && !gb && !gc && !gf && !gq && !out_ends)
    return fail(LSSVR_ERR_NULL, "one of ga, gb, gc, gf, gq, out_ends must be non-NULL");
  if (const int rc = check_nl_kind(kind, nterm)) return rc;
  if (kind == LSSVR_NL_EXP && !q_tabs) return fail(LSSVR_ERR_NULL, "q_tabs must be non-NULL with LSSVR_NL_EXP");
  a.q_tabs = q_tabs;
  a.kind = kind;
  a.nterm = nterm;
  a.gq = gq;
  return LSSVR_OK;
}

int lssvr_semilinear_sensitivity(const double* x, int64_t ne, int nquad, const double* U, int nu, const double* Z,
                                 int nc, const double* q_tabs, int kind, int nterm, double* ga, double* gb, double* gc,
                                 double* gf, double* gq, const double* P, const double* band_ends, int kind_left,
                                 int kind_right, double* out_ends, void* stream) {
  lssvr::NlSensArgs a{};
  const int rc = bind_nl_sens(a, x, ne, nquad, U, nu, Z, nc, q_tabs, kind, nterm, ga, gb, gc, gf, gq, P, band_ends,
                              kind_left, kind_right, out_ends);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::nl_sensitivity(a, reinterpret_cast<hipStream_t>(stream)), "nl_sensitivity");
}

int lssvr_semilinear_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* U_host, int nu,
                                      const double* Z_host, int nc, const double* q_tabs_host, int kind, int nterm,
                                      double* ga_host, double* gb_host, double* gc_host, double* gf_host,
                                      double* gq_host, const double* P_host, const double* band_ends_host,
                                      int kind_left, int kind_right, double* out_ends_host) {
  lssvr::NlSensArgs a{};
  const int rc = bind_nl_sens(a, x_host, ne, nquad, U_host, nu, Z_host, nc, q_tabs_host, kind, nterm, ga_host, gb_host,
                              gc_host, gf_host, gq_host, P_host, band_ends_host, kind_left, kind_right, out_ends_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::nl_sensitivity_host(a);          // (nquad is checked above: the rule exists)
  return LSSVR_OK;
}

// an output (NULL: not given) that is another output or one of the inputs
static bool aliased(const void* const* outs, int nout, const void* const* ins, int nin) {
  for (int i = 0; i < nout; ++i) {
    if (!outs[i]) continue;
    for (int j = i + 1; j < nout; ++j)
      if (outs[j] == outs[i]) return true;
    for (int j = 0; j < nin; ++j)
      if (ins[j] == outs[i]) return true;
  }
  return false;
}


// The chunk pass of the time-loop adjoint sensitivities (chunk_sens.hip).  The two schemes share one validated binding,
// and the device and the host entry of a scheme share its front.
// what a scheme says to the shared checks: the words of its messages, and what it has of its own
struct ChunkSensScheme {
  int64_t n0_min;              // the lowest first level of a chunk
  const char* level;           // what n0 counts
  const char* inputs;          // the inputs that must be given, by name, and whether the scheme's own among them are
  bool inputs_given;
  const char* tables;          // the table outputs and out_g, by name
  double* gd;                  // the scheme's own table output; NULL: none, or not wanted
  const char* own_null;        // the scheme's own "X must be non-NULL with Y" that applies; NULL: none does
  const void* own_in[2];       // the scheme's own device inputs (NULL: not given)
};

static int bind_chunk_sens(lssvr::ChunkSensArgs& a, const ChunkSensScheme& sch, const double* x, int64_t ne, int nquad,
                           const double* Utraj, const double* Z, int64_t n0, int m, const double* phi, int R,
                           double* ga, double* gc, double* grho, double* gf, int accumulate, const double* Brows,
                           const double* band_ends, int kind_left, int kind_right, double* out_g, double* out_kappa) {
  if (const int rc = check_ne(ne)) return rc;
  if (m < 1 || m > lssvr::kChunkSensMaxSteps) return fail(LSSVR_ERR_SIZE, "m = %d outside [1, 8]", m);
  if (n0 < sch.n0_min)
    return fail(LSSVR_ERR_SIZE, "n0 = %lld: the first %s of a chunk is >= %lld", (long long)n0, sch.level,
                (long long)sch.n0_min);
  if (R < 0 || R > lssvr::kChunkSensMaxTerms) return fail(LSSVR_ERR_SIZE, "R = %d outside [0, 8]", R);
  if (R == 0 && gf) return fail(LSSVR_ERR_SIZE, "R = 0 is allowed only with gf NULL");
  if (nquad < 1 || nquad > 5) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  if (!x || !Utraj || !Z || !sch.inputs_given) return fail(LSSVR_ERR_NULL, "%s must be non-NULL", sch.inputs);
  if (!ga && !gc && !grho && !sch.gd && !gf && !out_g)
    return fail(LSSVR_ERR_NULL, "one of %s must be non-NULL", sch.tables);
  if (gf && !phi) return fail(LSSVR_ERR_NULL, "phi must be non-NULL with gf");
  if (sch.own_null) return fail(LSSVR_ERR_NULL, "%s", sch.own_null);
  if (!out_g != !out_kappa) return fail(LSSVR_ERR_NULL, "out_g and out_kappa go together: both or neither");
  if (out_g) {
    if (!Brows || !band_ends) return fail(LSSVR_ERR_NULL, "Brows and band_ends must be non-NULL with out_g");
    if (const int rc = check_kinds(kind_left, kind_right)) return rc;
  }
  const void* outs[] = {ga, gc, grho, sch.gd, gf, out_g, out_kappa};
  const void* ins[] = {x, Utraj, sch.own_in[0], sch.own_in[1], Z, phi, Brows, band_ends};
  if (aliased(outs, 7, ins, 8))
    return fail(LSSVR_ERR_SIZE, "%s, out_kappa must be distinct and none of them an input", sch.tables);
  a = lssvr::ChunkSensArgs{x, Utraj, Z, Brows, phi, band_ends, ne, n0, nquad, m, R, accumulate != 0,
                           {kind_left, kind_right}, ga, gc, grho, gf, out_g, out_kappa};
  return LSSVR_OK;
}

// BDF: n0 >= 1, coef_host and band_mask
static int bind_ts_sens(lssvr::TsSensArgs& a, const double* x, int64_t ne, int nquad, const double* Utraj,
                        const double* Z, int64_t n0, int m, double inv_dt, const double* coef_host, const double* phi,
                        int R, double* ga, double* gc, double* grho, double* gf, int accumulate, const double* Brows,
                        const double* band_ends, int band_mask, int kind_left, int kind_right,
                        double* out_g, double* out_kappa) {
  const ChunkSensScheme sch{1, "adjoint step", "x, Utraj, Z, coef_host", coef_host != nullptr,
                            "ga, gc, grho, gf, out_g", nullptr, nullptr, {nullptr, nullptr}};
  a = lssvr::TsSensArgs{};
  if (const int rc = bind_chunk_sens(a, sch, x, ne, nquad, Utraj, Z, n0, m, phi, R, ga, gc, grho, gf, accumulate, Brows,
                                     band_ends, kind_left, kind_right, out_g, out_kappa))
    return rc;
  if (out_g) {
    if (band_mask < 0 || band_mask >> m)
      return fail(LSSVR_ERR_SIZE, "band_mask = %d has bits beyond the m = %d steps", band_mask, m);
    for (int i = 0; i < m; ++i) a.band_row[i] = (band_mask >> i) & 1;
  }
  a.inv_dt = inv_dt;
  for (int i = 0; i < m; ++i)
    for (int k = 0; k < 3; ++k) a.coef[i][k] = coef_host[3 * i + k];
  return LSSVR_OK;
}

int lssvr_transient_sensitivity(const double* x, int64_t ne, int nquad, const double* Utraj, const double* Z,
                                int64_t n0, int m, double inv_dt, const double* coef_host, const double* phi, int R,
                                double* ga, double* gc, double* grho, double* gf, int accumulate, const double* Brows,
                                const double* band_ends, int band_mask, int kind_left, int kind_right, double* out_g,
                                double* out_kappa, void* stream) {
  lssvr::TsSensArgs a;
  const int rc = bind_ts_sens(a, x, ne, nquad, Utraj, Z, n0, m, inv_dt, coef_host, phi, R, ga, gc, grho, gf, accumulate,
                              Brows, band_ends, band_mask, kind_left, kind_right, out_g, out_kappa);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::chunk_sensitivity(a, reinterpret_cast<hipStream_t>(stream)), "ts_sensitivity");
}

int lssvr_transient_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* Utraj_host,
                                     const double* Z_host, int64_t n0, int m, double inv_dt, const double* coef_host,
                                     const double* phi_host, int R, double* ga_host, double* gc_host,
                                     double* grho_host, double* gf_host, int accumulate, const double* Brows_host,
                                     const double* band_ends_host, int band_mask, int kind_left, int kind_right,
                                     double* out_g_host, double* out_kappa_host) {
  lssvr::TsSensArgs a;
  const int rc = bind_ts_sens(a, x_host, ne, nquad, Utraj_host, Z_host, n0, m, inv_dt, coef_host, phi_host, R, ga_host,
                              gc_host, grho_host, gf_host, accumulate, Brows_host, band_ends_host, band_mask,
                              kind_left, kind_right, out_g_host, out_kappa_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::chunk_sensitivity_host(a);       // (nquad is checked above: the rule exists)
  return LSSVR_OK;
}

// semilinear BDF: the BDF binding with one matrix per level (band_ends [m][2], no band_mask) and
// the law with its tables
static int bind_ts_nl_sens(lssvr::TsNlSensArgs& a, const double* x, int64_t ne, int nquad, const double* Utraj,
                           const double* Z, int64_t n0, int m, double inv_dt, const double* coef_host,
                           const double* phi, int R, const double* q_tabs, int kind, int nterm, double* ga, double* gc,
                           double* grho, double* gf, double* gq, int accumulate, const double* Brows,
                           const double* band_ends, int kind_left, int kind_right, double* out_g,
                           double* out_kappa) {
  const ChunkSensScheme sch{1, "adjoint step", "x, Utraj, Z, coef_host", coef_host != nullptr,
                            "ga, gc, grho, gf, gq, out_g", gq,
                            gq && kind == LSSVR_NL_EXP && !q_tabs ? "q_tabs must be non-NULL with LSSVR_NL_EXP and gq"
                                                                  : nullptr,
                            {q_tabs, nullptr}};
  a = lssvr::TsNlSensArgs{};
  if (const int rc = bind_chunk_sens(a, sch, x, ne, nquad, Utraj, Z, n0, m, phi, R, ga, gc, grho, gf, accumulate, Brows,
                                     band_ends, kind_left, kind_right, out_g, out_kappa))
    return rc;
  if (const int rc = check_nl_kind(kind, nterm)) return rc;
  for (int i = 0; i < m; ++i) a.band_row[i] = i;
  a.inv_dt = inv_dt;
  for (int i = 0; i < m; ++i)
    for (int k = 0; k < 3; ++k) a.coef[i][k] = coef_host[3 * i + k];
  a.q_tabs = q_tabs, a.law = kind, a.nterm = nterm, a.gq = gq;
  return LSSVR_OK;
}

int lssvr_semilinear_transient_sensitivity(const double* x, int64_t ne, int nquad, const double* Utraj,
                                           const double* Z, int64_t n0, int m, double inv_dt, const double* coef_host,
                                           const double* phi, int R, const double* q_tabs, int kind, int nterm,
                                           double* ga, double* gc, double* grho, double* gf, double* gq,
                                           int accumulate, const double* Brows, const double* band_ends,
                                           int kind_left, int kind_right, double* out_g, double* out_kappa,
                                           void* stream) {
  lssvr::TsNlSensArgs a;
  const int rc = bind_ts_nl_sens(a, x, ne, nquad, Utraj, Z, n0, m, inv_dt, coef_host, phi, R, q_tabs, kind, nterm, ga,
                                 gc, grho, gf, gq, accumulate, Brows, band_ends, kind_left, kind_right, out_g,
                                 out_kappa);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::chunk_sensitivity(a, reinterpret_cast<hipStream_t>(stream)), "ts_nl_sensitivity");
}

int lssvr_semilinear_transient_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* Utraj_host,
                                                const double* Z_host, int64_t n0, int m, double inv_dt,
                                                const double* coef_host, const double* phi_host, int R,
                                                const double* q_tabs_host, int kind, int nterm, double* ga_host,
                                                double* gc_host, double* grho_host, double* gf_host, double* gq_host,
                                                int accumulate, const double* Brows_host,
                                                const double* band_ends_host, int kind_left, int kind_right,
                                                double* out_g_host, double* out_kappa_host) {
  lssvr::TsNlSensArgs a;
  const int rc = bind_ts_nl_sens(a, x_host, ne, nquad, Utraj_host, Z_host, n0, m, inv_dt, coef_host, phi_host, R,
                                 q_tabs_host, kind, nterm, ga_host, gc_host, grho_host, gf_host, gq_host, accumulate,
                                 Brows_host, band_ends_host, kind_left, kind_right, out_g_host, out_kappa_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::chunk_sensitivity_host(a);       // (nquad is checked above: the rule exists)
  return LSSVR_OK;
}

// The backward step of the semilinear BDF loop (timestep_nl_adjoint.hip): the checks of lssvr_ts_nl_assemble on the
// Jacobian's side and of lssvr_ts_rhs (one case) on the right-hand side's.  The device and the host entry share one
// validated binding.
static int bind_ts_nl_adjoint(lssvr::TsNlAdjArgs& a, const double* x, const double* u, const double* a_quad,
                              const double* cs_quad, const double* q_quad, int64_t ne, int nquad, int kind, int nterm,
                              const double* mdiag, const double* moff, const double* U0, const double* U1,
                              const double* loads, const double* phi, int R, double beta0, double beta1, double inv_dt,
                              double* diag, double* off, double* B, double* band_ends) {
  if (const int rc = check_ne(ne)) return rc;
  if (nquad < 1 || nquad > 5) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  if (const int rc = check_nl_kind(kind, nterm)) return rc;
  if (R < 1 || R > 8) return fail(LSSVR_ERR_SIZE, "R = %d outside [1, 8]", R);
  if (!is_finite(beta0) || !is_finite(beta1) || !is_finite(inv_dt))
    return fail(LSSVR_ERR_SIZE, "beta0 = %g, beta1 = %g, inv_dt = %g must be finite", beta0, beta1, inv_dt);
  if (!x || !u || !cs_quad || !q_quad || !diag || !off || !B || !band_ends)
    return fail(LSSVR_ERR_NULL, "x, u, cs_quad, q_quad, diag, off, B, band_ends must be non-NULL");
  if (!mdiag || !moff || !U0 || !loads || !phi)
    return fail(LSSVR_ERR_NULL, "mdiag, moff, U0, loads, phi must be non-NULL");
  if (beta1 != 0.0 && !U1) return fail(LSSVR_ERR_NULL, "U1 must be non-NULL when beta1 != 0");
  const void* outs[] = {diag, off, B, band_ends};
  const void* ins[] = {x, u, a_quad, cs_quad, q_quad, mdiag, moff, U0, beta1 != 0.0 ? U1 : nullptr, loads, phi};
  if (aliased(outs, 4, ins, 11))
    return fail(LSSVR_ERR_SIZE, "diag, off, B, band_ends must be distinct and none of them an input");
  a.nl = lssvr::TsNlArgs{x, u, a_quad, cs_quad, q_quad, nullptr, ne, nquad, kind, nterm, diag, off, nullptr};
  a.rhs = lssvr::TsRhsArgs{mdiag, moff, U0, U1, loads, phi, ne, 1, R, beta0, beta1, inv_dt};
  a.B = B;
  a.band_ends = band_ends;
  return LSSVR_OK;
}

int lssvr_semilinear_adjoint_step(const double* x, const double* u, const double* a_quad, const double* cs_quad,
                                  const double* q_quad, int64_t ne, int nquad, int kind, int nterm,
                                  const double* mdiag, const double* moff, const double* U0, const double* U1,
                                  const double* loads, const double* phi, int R, double beta0, double beta1,
                                  double inv_dt, double* diag, double* off, double* B, double* band_ends,
                                  void* stream) {
  lssvr::TsNlAdjArgs a{};
  const int rc = bind_ts_nl_adjoint(a, x, u, a_quad, cs_quad, q_quad, ne, nquad, kind, nterm, mdiag, moff, U0, U1,
                                    loads, phi, R, beta0, beta1, inv_dt, diag, off, B, band_ends);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::ts_nl_adjoint_step(a, reinterpret_cast<hipStream_t>(stream)), "ts_nl_adjoint_step");
}

int lssvr_semilinear_adjoint_step_host(const double* x_host, const double* u_host, const double* a_quad_host,
                                       const double* cs_quad_host, const double* q_quad_host, int64_t ne, int nquad,
                                       int kind, int nterm, const double* mdiag_host, const double* moff_host,
                                       const double* U0_host, const double* U1_host, const double* loads_host,
                                       const double* phi_host, int R, double beta0, double beta1, double inv_dt,
                                       double* diag_host, double* off_host, double* B_host,
                                       double* band_ends_host) {
  lssvr::TsNlAdjArgs a{};
  const int rc = bind_ts_nl_adjoint(a, x_host, u_host, a_quad_host, cs_quad_host, q_quad_host, ne, nquad, kind, nterm,
                                    mdiag_host, moff_host, U0_host, U1_host, loads_host, phi_host, R, beta0, beta1,
                                    inv_dt, diag_host, off_host, B_host, band_ends_host);
  if (rc != LSSVR_OK) return rc;
  if (!lssvr::ts_nl_adjoint_step_host(a)) return fail(LSSVR_ERR_QUAD, "nquad = %d outside [1,5]", nquad);
  return LSSVR_OK;
}

// Newmark: n0 >= 0, Vtraj with gd, Atraj with grho
static int bind_nm_sens(lssvr::NmSensArgs& a, const double* x, int64_t ne, int nquad, const double* Utraj,
                        const double* Vtraj, const double* Atraj, const double* Z, int64_t n0, int m, const double* phi,
                        int R, double* ga, double* gc, double* grho, double* gd, double* gf, int accumulate,
                        const double* Brows, const double* band_ends, int kind_left, int kind_right, double* out_g,
                        double* out_kappa) {
  const ChunkSensScheme sch{0, "level", "x, Utraj, Z", true, "ga, gc, grho, gd, gf, out_g", gd,
                            gd && !Vtraj      ? "Vtraj must be non-NULL with gd"
                            : grho && !Atraj ? "Atraj must be non-NULL with grho"
                                              : nullptr,
                            {Vtraj, Atraj}};
  a = lssvr::NmSensArgs{};
  if (const int rc = bind_chunk_sens(a, sch, x, ne, nquad, Utraj, Z, n0, m, phi, R, ga, gc, grho, gf, accumulate, Brows,
                                     band_ends, kind_left, kind_right, out_g, out_kappa))
    return rc;
  a.Vtraj = Vtraj, a.Atraj = Atraj, a.gd = gd;
  return LSSVR_OK;
}

int lssvr_newmark_sensitivity(const double* x, int64_t ne, int nquad, const double* Utraj, const double* Vtraj,
                              const double* Atraj, const double* Z, int64_t n0, int m, const double* phi, int R,
                              double* ga, double* gc, double* grho, double* gd, double* gf, int accumulate,
                              const double* Brows, const double* band_ends, int kind_left, int kind_right,
                              double* out_g, double* out_kappa, void* stream) {
  lssvr::NmSensArgs a;
  const int rc = bind_nm_sens(a, x, ne, nquad, Utraj, Vtraj, Atraj, Z, n0, m, phi, R, ga, gc, grho, gd, gf, accumulate,
                              Brows, band_ends, kind_left, kind_right, out_g, out_kappa);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::chunk_sensitivity(a, reinterpret_cast<hipStream_t>(stream)), "newmark_sensitivity");
}

int lssvr_newmark_sensitivity_host(const double* x_host, int64_t ne, int nquad, const double* Utraj_host,
                                   const double* Vtraj_host, const double* Atraj_host, const double* Z_host, int64_t n0,
                                   int m, const double* phi_host, int R, double* ga_host, double* gc_host,
                                   double* grho_host, double* gd_host, double* gf_host, int accumulate,
                                   const double* Brows_host, const double* band_ends_host, int kind_left,
                                   int kind_right, double* out_g_host, double* out_kappa_host) {
  lssvr::NmSensArgs a;
  const int rc = bind_nm_sens(a, x_host, ne, nquad, Utraj_host, Vtraj_host, Atraj_host, Z_host, n0, m, phi_host, R,
                              ga_host, gc_host, grho_host, gd_host, gf_host, accumulate, Brows_host, band_ends_host,
                              kind_left, kind_right, out_g_host, out_kappa_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::chunk_sensitivity_host(a);       // (nquad is checked above: the rule exists)
  return LSSVR_OK;
}

// The adjoint advance of the Newmark loop (newmark_adjoint.hip).  The device and the host entry share one validated
// binding.
static int bind_nm_adj(lssvr::NmAdjArgs& a, const double* lam, const double* Vbar, const double* Abar, const double* P,
                       const double* mdiag, const double* moff, const double* ddiag, const double* doff, int64_t ne,
                       double dt, double beta, double gamma, double* V_out, double* A_out, double* U_out,
                       double* B_out) {
  if (const int rc = check_ne(ne)) return rc;
  if (!(is_finite(dt) && dt > 0.0) || !(is_finite(beta) && beta > 0.0) || !(is_finite(gamma) && gamma > 0.0))
    return fail(LSSVR_ERR_SIZE, "dt = %g, beta = %g, gamma = %g must be finite and > 0", dt, beta, gamma);
  if (!Vbar || !Abar) return fail(LSSVR_ERR_NULL, "Vbar, Abar must be non-NULL");
  if (!lam) {
    if (!B_out) return fail(LSSVR_ERR_NULL, "B_out must be non-NULL without lam: the first call of a sweep writes it");
    if (V_out || A_out || U_out)
      return fail(LSSVR_ERR_SIZE, "V_out, A_out, U_out must be NULL without lam: the first call writes B_out alone");
  } else {
    if (!mdiag || !moff) return fail(LSSVR_ERR_NULL, "mdiag, moff must be non-NULL with lam");
    if (!ddiag != !doff) return fail(LSSVR_ERR_NULL, "ddiag and doff go together: both or neither");
    if (!V_out || !A_out) return fail(LSSVR_ERR_NULL, "V_out, A_out must be non-NULL with lam");
  }
  const void* outs[] = {V_out, A_out, U_out, B_out};
  const void* ins[] = {lam, Vbar, Abar, P, mdiag, moff, ddiag, doff};
  if (aliased(outs, 4, ins, 8))
    return fail(LSSVR_ERR_SIZE, "V_out, A_out, U_out, B_out must be distinct and none of them an input");
  lssvr::WaveArgs w{};
  lssvr::wave_coefficients(w, dt, beta, gamma);
  a = lssvr::NmAdjArgs{lam, Vbar, Abar, P, mdiag, moff, lam ? ddiag : nullptr, lam ? doff : nullptr, ne,
                       w.dt, w.c_u2, w.c_v1, w.c_m, w.c_d, w.c_va, V_out, A_out, U_out, B_out};
  return LSSVR_OK;
}

int lssvr_newmark_adjoint_advance(const double* lam, const double* Vbar, const double* Abar, const double* P,
                                  const double* mdiag, const double* moff, const double* ddiag, const double* doff,
                                  int64_t ne, double dt, double beta, double gamma, double* V_out, double* A_out,
                                  double* U_out, double* B_out, void* stream) {
  lssvr::NmAdjArgs a{};
  const int rc = bind_nm_adj(a, lam, Vbar, Abar, P, mdiag, moff, ddiag, doff, ne, dt, beta, gamma, V_out, A_out, U_out,
                             B_out);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::newmark_adjoint_advance(a, reinterpret_cast<hipStream_t>(stream)),
                      "newmark_adjoint_advance");
}

int lssvr_newmark_adjoint_advance_host(const double* lam_host, const double* Vbar_host, const double* Abar_host,
                                       const double* P_host, const double* mdiag_host, const double* moff_host,
                                       const double* ddiag_host, const double* doff_host, int64_t ne, double dt,
                                       double beta, double gamma, double* V_out_host, double* A_out_host,
                                       double* U_out_host, double* B_out_host) {
  lssvr::NmAdjArgs a{};
  const int rc = bind_nm_adj(a, lam_host, Vbar_host, Abar_host, P_host, mdiag_host, moff_host, ddiag_host, doff_host,
                             ne, dt, beta, gamma, V_out_host, A_out_host, U_out_host, B_out_host);
  if (rc != LSSVR_OK) return rc;
  lssvr::newmark_adjoint_advance_host(a);
  return LSSVR_OK;
}

// Adjoint of the element solve (enhance_adjoint.hip).  The device and the host entry share one validated binding.
int64_t lssvr_enhance_adjoint_work_bytes(int64_t ne) { return ne < 1 ? 0 : ne * (int64_t)(2 * sizeof(double)); }

static int bind_enh_adj(lssvr::EnhAdjArgs& a, const double* x, int64_t ne, int64_t elem_offset, int64_t ne_global,
                        double gxmin, double gxmax, int M, int n_colloc, double gamma, const double* a_values,
                        const double* da_values, const double* c_values, const double* rhs_values, const double* W,
                        const int32_t* status, const double* Wbar, double* gu, double* gbc, double* ga, double* gda,
                        double* gc, double* gf, void* work, int64_t work_bytes) {
  if (const int rc = check_ne(ne)) return rc;
  if (M < lssvr::kEnhAdjMinM || M > lssvr::kEnhAdjMaxM)
    return fail(LSSVR_ERR_DEGREE, "M = %d outside [%d, %d]", M, lssvr::kEnhAdjMinM, lssvr::kEnhAdjMaxM);
  const int n_min = M - 2 > 2 ? M - 2 : 2;
  if (n_colloc < n_min || n_colloc > lssvr::kEnhAdjMaxColloc)
    return fail(LSSVR_ERR_SIZE, "n_colloc = %d outside [%d, %d]", n_colloc, n_min, lssvr::kEnhAdjMaxColloc);
  if (elem_offset < 0 || ne_global < elem_offset + ne)
    return fail(LSSVR_ERR_SIZE, "shard [%lld, %lld) does not fit ne_global = %lld", (long long)elem_offset,
                (long long)(elem_offset + ne), (long long)ne_global);
  if (!(gamma > 0.0)) return fail(LSSVR_ERR_SIZE, "gamma must be > 0");
  if (!x || !rhs_values || !W || !Wbar) return fail(LSSVR_ERR_NULL, "x, rhs_values, W, Wbar must be non-NULL");
  if (!gu && !gbc && !ga && !gda && !gc && !gf)
    return fail(LSSVR_ERR_NULL, "one of gu, gbc, ga, gda, gc, gf must be non-NULL");
  if (da_values && !a_values) return fail(LSSVR_ERR_NULL, "da_values needs a_values");
  if ((ga || gda) && !a_values) return fail(LSSVR_ERR_NULL, "ga and gda need a_values");
  if (gc && !c_values) return fail(LSSVR_ERR_NULL, "gc needs c_values");
  if (const int rc = check_work_sized(work, work_bytes, lssvr_enhance_adjoint_work_bytes(ne),
                                      "lssvr_enhance_adjoint_work_bytes", ne))
    return rc;
  a = lssvr::EnhAdjArgs{x,         ne,       elem_offset, ne_global,  gxmin, gxmax,  gamma, M,  n_colloc,
                        a_values,  da_values, c_values,   rhs_values, W,     status, Wbar,  gu, gbc,
                        ga,        gda,      gc,          gf,         static_cast<double*>(work)};
  return LSSVR_OK;
}

int lssvr_enhance_adjoint(const double* x, int64_t ne, int64_t elem_offset, int64_t ne_global, double gxmin,
                          double gxmax, int M, int n_colloc, double gamma, const double* a_values,
                          const double* da_values, const double* c_values, const double* rhs_values, const double* W,
                          const int32_t* status, const double* Wbar, double* gu, double* gbc, double* ga, double* gda,
                          double* gc, double* gf, void* work, int64_t work_bytes, void* stream) {
  lssvr::EnhAdjArgs a{};
  const int rc = bind_enh_adj(a, x, ne, elem_offset, ne_global, gxmin, gxmax, M, n_colloc, gamma, a_values, da_values,
                              c_values, rhs_values, W, status, Wbar, gu, gbc, ga, gda, gc, gf, work, work_bytes);
  if (rc != LSSVR_OK) return rc;
  return check_launch(lssvr::enhance_adjoint(a, reinterpret_cast<hipStream_t>(stream)), "enhance_adjoint");
}

int lssvr_enhance_adjoint_host(const double* x_host, int64_t ne, int64_t elem_offset, int64_t ne_global, double gxmin,
                               double gxmax, int M, int n_colloc, double gamma, const double* a_values_host,
                               const double* da_values_host, const double* c_values_host,
                               const double* rhs_values_host, const double* W_host, const int32_t* status_h,
                               const double* Wbar_host, double* gu_host, double* gbc_host, double* ga_host,
                               double* gda_host, double* gc_host, double* gf_host, void* work_h,
                               int64_t work_bytes) {
  lssvr::EnhAdjArgs a{};
  const int rc = bind_enh_adj(a, x_host, ne, elem_offset, ne_global, gxmin, gxmax, M, n_colloc, gamma, a_values_host,
                              da_values_host, c_values_host, rhs_values_host, W_host, status_h, Wbar_host, gu_host,
                              gbc_host, ga_host, gda_host, gc_host, gf_host, work_h, work_bytes);
  if (rc != LSSVR_OK) return rc;
  lssvr::enhance_adjoint_host(a);         // (M is checked above: the degree is instantiated)
  return LSSVR_OK;
}

}  // extern "C"
