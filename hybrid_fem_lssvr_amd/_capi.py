"""ctypes binding of ``csrc/liblssvr_hip.so`` (C ABI: ``include/lssvr_hip.h``).

The library is the product; there is no CPU fallback.  Loading fails loudly when
the shared object is missing, and every compute entry point needs device
pointers on a visible MI355X.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
IN_TREE_LIB = os.path.join(_HERE, "csrc", "liblssvr_hip.so")
# LSSVR_HIP_LIB selects another build of the same ABI -- for kernel A/B experiments in
# scripts/ only: __graft_entry__.build() and tests/conftest.py refuse to run with it set, so the
# test suite and the benchmark always exercise the one in-tree library.
LIB_PATH = os.environ.get("LSSVR_HIP_LIB") or IN_TREE_LIB

ABI_VERSION = 7

RHS_ARRAY = 0
RHS_SIN = 1
RHS_ARRAY_PM = 2
TABLE_ELEMENT_MAJOR = 0
TABLE_POINT_MAJOR = 1
SOLVER_PRIMAL = 0
SOLVER_DUAL = 1
SOLVER_PRIMAL_WAVE = 2
SOLVER_PRIMAL_MOMENT = 3
END_DIRICHLET = 0
END_ROBIN = 1
NL_POLY = 0
NL_EXP = 1
ST_OK = 0
ST_FALLBACK = 1

_c_dp = C.c_void_p      # device pointers travel as integers
_c_i64 = C.c_int64
_c_int = C.c_int
_c_dbl = C.c_double

_c_hd = C.POINTER(_c_dbl)   # host double*: rhs parameters, Gauss rules
_c_hf = C.POINTER(C.c_float)   # host float*: kernel durations in ms

# the argument groups the header's declarations are made of
_SHARD = [_c_dp, _c_dp, _c_i64, _c_i64, _c_i64,      # x, u, ne, elem_offset, ne_global
          _c_dbl, _c_dbl, _c_dbl, _c_dbl,            # gxmin, gxmax, bc_left, bc_right
          _c_int, _c_int, _c_dbl]                    # M, n_colloc, gamma
_SUBSET = [_c_dp, _c_dp, _c_i64, _c_dp, _c_i64, _c_i64, _c_i64,     # x, u, ne_mesh, elem_ids, nsub, offset, ne_global
           _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_int, _c_int, _c_dbl, _c_dp]    # ..., M, n_colloc, gamma, gamma_values
_RHS = [_c_int, _c_hd, _c_dp]                        # rhs_id, rhs_params_host, rhs_values / rhs_quad
_VC_TABLES = [_c_dp, _c_dp, _c_dp]                   # a_values, da_values, rhs_values
_REACT_TABLES = [_c_dp, _c_dp, _c_dp, _c_dp]         # a_values, da_values, c_values, rhs_values
_OUT = [_c_dp, _c_dp, _c_dp]                         # W, status, fail_count
_WS = [_c_dp, _c_i64]                                # work, work_bytes
_BANDS = [_c_dp, _c_dp, _c_dp]                       # diag, off, load
_LOCAL = [_c_dp, _c_dp]                              # kloc, floc
_STREAM = [_c_dp]
_TIMED = [_c_hf]                                     # kernel_ms_host
_SEQ = [_c_int, _c_hf]                               # repeats, kernel_ms_host[repeats]
_MESH = [_c_dp, _c_i64, _c_int]                      # x, ne, n_colloc / nquad / nq
_SOLN = [_c_dp, _c_dp, _c_i64, _c_int]               # x, W, ne, M
_EST_OUT = [_c_dp, _c_dp, _c_dp, _c_dp]              # eta2, jump, out3, work
_ENDS = [_c_int, _c_int, _c_dp, _c_hd]                # kind_left, kind_right, end_values, kappa_host
_STEP = _SHARD + [_c_hd, _c_int] + _BANDS + _OUT     # ..., rhs_params_host, nquad, bands, outputs
_EIG_BANDS = [_c_dp] * 4 + [_c_int, _c_int, _c_hd]   # kdiag, koff, mdiag, moff, kind_left, kind_right, kappa_host


def _sig(*groups, res=_c_int):
    return res, [t for g in groups for t in g]


# name -> (restype, argtypes); mirrors include/lssvr_hip.h declaration by declaration, one argument group each
# (tests/test_capi_cpu.py parses the headers and compares every entry with this table)
SIGNATURES = {
    "lssvr_version": _sig(),
    "lssvr_last_error": _sig(res=C.c_char_p),
    "lssvr_enhance": _sig(_SHARD, _RHS, [_c_int], _OUT, _STREAM),
    "lssvr_enhance_work_bytes": _sig([_c_i64, _c_int, _c_int, _c_int], res=_c_i64),
    "lssvr_enhance_ws": _sig(_SHARD, _RHS, [_c_int], _OUT, _WS, _STREAM, _TIMED),
    "lssvr_enhance_ws_sequence": _sig(_SHARD, _RHS, [_c_int], _OUT, _WS, _STREAM, _SEQ),
    "lssvr_enhance_profiled": _sig(_SHARD, _RHS, [_c_int], _OUT[:2], _STREAM, _TIMED),
    "lssvr_step": _sig(_STEP, _STREAM),
    "lssvr_step_plan_create": _sig([C.POINTER(C.c_void_p)], _STEP),
    "lssvr_step_plan_launch": _sig([C.c_void_p], _STREAM),
    "lssvr_step_plan_destroy": _sig([C.c_void_p]),
    # the step memo (additive to ABI 7): plan; plan, memo, memo_bytes, stream
    "lssvr_step_plan_memo_bytes": _sig([C.c_void_p], res=_c_i64),
    "lssvr_step_plan_memo_bind": _sig([C.c_void_p, _c_dp, _c_i64], _STREAM),
    "lssvr_enhance_varcoef": _sig(_SHARD, _VC_TABLES, _OUT, _STREAM),
    "lssvr_enhance_varcoef_work_bytes": _sig([_c_i64, _c_int, _c_int], res=_c_i64),
    "lssvr_enhance_varcoef_ws": _sig(_SHARD, _VC_TABLES, [_c_int], _OUT, _WS, _STREAM, _TIMED),
    "lssvr_enhance_varcoef_ws_sequence": _sig(_SHARD, _VC_TABLES, [_c_int], _OUT, _WS, _STREAM, _SEQ),
    "lssvr_step_varcoef": _sig(_SHARD, _VC_TABLES, [_c_int, _c_int, _c_dp, _c_dp], _BANDS, _OUT, _STREAM),
    "lssvr_enhance_subset": _sig(_SUBSET, _RHS, [_c_dp, _c_i64, _c_dp, _c_dp], _STREAM),
    "lssvr_enhance_subset_ws": _sig(_SUBSET, _RHS, [_c_dp, _c_i64, _c_dp, _c_dp], _WS, _STREAM),
    "lssvr_enhance_shared": _sig(_SHARD[:-1], _RHS, [_c_dp], _OUT, _STREAM, _TIMED),
    "lssvr_colloc_points": _sig(_MESH, [_c_dp], _STREAM),
    "lssvr_colloc_points_pm": _sig(_MESH, [_c_dp], _STREAM),
    "lssvr_p1_assemble": _sig(_MESH, _RHS, [_c_dp], _BANDS, _LOCAL, _STREAM),
    "lssvr_quad_points": _sig(_MESH, [_c_dp], _STREAM),
    "lssvr_tridiag_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_tridiag_dirichlet_solve": _sig(_BANDS, [_c_i64, _c_dbl, _c_dbl, _c_dp, _c_dp], _STREAM),
    "lssvr_p1_flux_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_p1_flux_solve": _sig([_c_dp, _c_dp, _c_i64, _c_dbl, _c_dbl, _c_dp, _c_dp], _STREAM),
    "lssvr_p1_flux_aggregate": _sig([_c_dp, _c_dp, _c_i64, _c_int, _c_dp, _c_dp], _STREAM),
    "lssvr_p1_flux_finish": _sig([_c_dp, _c_dp, _c_i64, _c_int, _c_int, _c_dp, _c_dp, _c_dp, _c_dbl, _c_dbl, _c_dp],
                                 _STREAM),
    "lssvr_eval": _sig(_SOLN, [_c_dp, _c_i64, _c_dp, _c_dp], _STREAM),
    "lssvr_eval_error": _sig(_SOLN, [_c_dp, _c_i64, _c_hd, _c_dp], _STREAM),
    "lssvr_eval_deriv": _sig(_SOLN, [_c_int, _c_dp, _c_i64, _c_dp, _c_dp], _STREAM),
    "lssvr_gauss_rule": _sig([_c_int, _c_hd, _c_hd]),
    "lssvr_estimate_points": _sig(_MESH, [_c_dp], _STREAM),
    "lssvr_adapt_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_estimate": _sig(_SOLN, [_c_int], _RHS, _EST_OUT, _STREAM),
    "lssvr_estimate_varcoef": _sig(_SOLN, [_c_int], _VC_TABLES, [_c_int, _c_dp], _EST_OUT, _STREAM),
    "lssvr_refine": _sig([_c_dp, _c_i64, _c_dp, _c_dp, _c_dbl, _c_dbl, _c_dp, _c_dp, _c_dp, _c_dp], _STREAM),
    # reaction term -(a u')' + c u = f (additive to ABI 7)
    "lssvr_enhance_react": _sig(_SHARD, _REACT_TABLES, _OUT, _STREAM),
    "lssvr_enhance_react_ws": _sig(_SHARD, _REACT_TABLES, [_c_int], _OUT, _WS, _STREAM, _TIMED),
    "lssvr_p1_assemble_react": _sig(_MESH, _RHS, [_c_dp, _c_dp], _BANDS, _LOCAL, _STREAM),
    "lssvr_estimate_react": _sig(_SOLN, [_c_int], _REACT_TABLES, [_c_int, _c_dp], _EST_OUT, _STREAM),
    # several load cases on one mesh (additive to ABI 7): ..., gxmin, gxmax, bc_values, ncases, M, n_colloc, gamma
    "lssvr_enhance_multi": _sig(_SHARD[:7], [_c_dp, _c_int], _SHARD[9:], _REACT_TABLES, [_c_int], _OUT, _STREAM,
                                _TIMED),
    # convection term -(a u')' + b u' + c u = f (additive to ABI 7): ..., a_quad, c_quad, b_quad, diag, sub, sup, load
    "lssvr_p1_assemble_conv": _sig(_MESH, _RHS, [_c_dp, _c_dp, _c_dp], [_c_dp], _BANDS, _LOCAL, _STREAM),
    "lssvr_tridiag_ns_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_tridiag_ns_dirichlet_solve": _sig([_c_dp], _BANDS, [_c_i64, _c_dbl, _c_dbl, _c_dp, _c_dp], _STREAM),
    # the P1 half of several load cases (additive to ABI 7): ..., ne, nc, bc_values, u, work, work_bytes
    "lssvr_p1_load_multi": _sig(_MESH, [_c_dp, _c_int, _c_dp], _STREAM),
    "lssvr_tridiag_multi_work_bytes": _sig([_c_i64, _c_int], res=_c_i64),
    "lssvr_tridiag_dirichlet_solve_multi": _sig(_BANDS, [_c_i64, _c_int, _c_dp, _c_dp], _WS, _STREAM),
    "lssvr_tridiag_ns_dirichlet_solve_multi": _sig([_c_dp], _BANDS, [_c_i64, _c_int, _c_dp, _c_dp], _WS, _STREAM),
    # Neumann / Robin ends (additive to ABI 7): ..., kind_left, kind_right, end_values, kappa_host, ne, nc, u, work
    "lssvr_tridiag_bc_work_bytes": _sig([_c_i64, _c_int], res=_c_i64),
    "lssvr_tridiag_bc_solve_multi": _sig(_BANDS, _ENDS, [_c_i64, _c_int, _c_dp], _WS, _STREAM),
    "lssvr_tridiag_ns_bc_solve_multi": _sig([_c_dp], _BANDS, _ENDS, [_c_i64, _c_int, _c_dp], _WS, _STREAM),
    # pivoting solve (additive to ABI 7): the _ns_bc_ arguments with info between u and work
    "lssvr_tridiag_pivot_work_bytes": _sig([_c_i64, _c_int], res=_c_i64),
    "lssvr_tridiag_pivot_solve_multi": _sig([_c_dp], _BANDS, _ENDS, [_c_i64, _c_int, _c_dp, _c_dp], _WS, _STREAM),
    "lssvr_tridiag_pivot_solve_host": _sig([_c_dp], _BANDS, _ENDS, [_c_i64, _c_int, _c_dp, _c_dp]),
    "lssvr_estimate_ends": _sig([_c_dp, _c_dp, _c_int, _c_i64, _c_int, _c_int, _c_hd, _c_hd, _c_hd, _c_dp, _c_dp],
                                _STREAM),
    # goal-oriented estimator (additive to ABI 7): x, Wu, Wz, ne, M, nq, a, a', c, f, j, layout, a_ends, kinds,
    # kappa_host, g_host, a_bnd_host, jump_free, eta, eta2, q, out4, work
    "lssvr_goal_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_estimate_goal": _sig([_c_dp, _c_dp, _c_dp, _c_i64, _c_int, _c_int], _REACT_TABLES, [_c_dp, _c_int, _c_dp],
                                [_c_int, _c_int, _c_hd, _c_hd, _c_hd, _c_int], [_c_dp] * 5, _STREAM),
    # periodic ends (additive to ABI 7): ..., ne, nc, u, work, work_bytes; x, W, M, ne, a_seam_host, eta2, out3
    "lssvr_tridiag_periodic_work_bytes": _sig([_c_i64, _c_int], res=_c_i64),
    "lssvr_tridiag_periodic_solve_multi": _sig(_BANDS, [_c_i64, _c_int, _c_dp], _WS, _STREAM),
    "lssvr_tridiag_ns_periodic_solve_multi": _sig([_c_dp], _BANDS, [_c_i64, _c_int, _c_dp], _WS, _STREAM),
    "lssvr_estimate_seam": _sig([_c_dp, _c_dp, _c_int, _c_i64, _c_hd, _c_dp, _c_dp], _STREAM),
    # element lists for the table kernels (additive to ABI 7): ..., gamma_values, a, a', c, f, layout, W, ldw, status,
    # fail_count; x, ne_mesh, elem_ids, nsub, n_colloc, layout, xc
    "lssvr_enhance_react_subset": _sig(_SUBSET, _REACT_TABLES, [_c_int], [_c_dp, _c_i64, _c_dp, _c_dp], _STREAM),
    "lssvr_colloc_points_subset": _sig([_c_dp, _c_i64, _c_dp, _c_i64, _c_int, _c_int, _c_dp], _STREAM),
    # hp-adaptive refinement (additive to ABI 7)
    "lssvr_smoothness": _sig([_c_dp, _c_i64, _c_dp, _c_i64, _c_dp], _STREAM),
    "lssvr_refine_hp": _sig([_c_dp, _c_i64, _c_dp, _c_dp, _c_dbl, _c_dbl, _c_dp, _c_dp, _c_dbl, _c_int, _c_int, _c_dp,
                             _c_dp, _c_dp, _c_dp, _c_dp, _c_dp], _STREAM),
    "lssvr_group_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_group_by_degree": _sig([_c_dp, _c_i64, _c_dp, _c_dp, _c_dp], _STREAM),
    # eigenproblems (additive to ABI 7): kdiag, koff, mdiag, moff, kind_left, kind_right, kappa_host, ne, ...
    "lssvr_eig_work_bytes": _sig([_c_i64, _c_int], res=_c_i64),
    "lssvr_eig_apply": _sig(_EIG_BANDS, [_c_i64, _c_int], [_c_dp] * 4, _WS, _STREAM),
    "lssvr_eig_ritz": _sig([_c_dp, _c_dp, _c_int, _c_dbl, _c_dp, _c_dp, _c_dp], _STREAM),
    "lssvr_eig_ritz_host": _sig([_c_hd, _c_hd, _c_int, _c_dbl, _c_hd, _c_hd, _c_dp]),
    "lssvr_eig_rotate": _sig([_c_dp] * 5, [_c_int, _c_int, _c_i64, _c_int], [_c_dp] * 3, _WS, _STREAM),
    "lssvr_eig_count": _sig(_EIG_BANDS, [_c_i64, _c_dp, _c_int, _c_dbl, _c_dp], _STREAM),
    "lssvr_eig_count_host": _sig([_c_hd] * 4, [_c_int, _c_int, _c_hd], [_c_i64, _c_hd, _c_int, _c_dbl, _c_dp]),
    "lssvr_eig_rayleigh": _sig(_SOLN, [_c_int], [_c_dp] * 3, [_c_int], [_c_int, _c_int, _c_hd], [_c_dp, _c_dp],
                               _STREAM),
    # transient problems (additive to ABI 7): mdiag, moff, U0, U1, loads, phi, ne, nc, R, beta0, beta1, inv_dt, out;
    # U2, U0, U1, ftab, rho_tab, phi, ne, n_colloc, R, layout, alpha, beta0, beta1, inv_dt, out
    "lssvr_ts_rhs": _sig([_c_dp] * 6, [_c_i64, _c_int, _c_int], [_c_dbl] * 3, [_c_dp], _STREAM),
    "lssvr_ts_rhs_host": _sig([_c_hd] * 6, [_c_i64, _c_int, _c_int], [_c_dbl] * 3, [_c_hd]),
    "lssvr_ts_source_table": _sig([_c_dp] * 6, [_c_i64, _c_int, _c_int, _c_int], [_c_dbl] * 4, [_c_dp], _STREAM),
    "lssvr_ts_source_table_host": _sig([_c_hd] * 6, [_c_i64, _c_int, _c_int, _c_int], [_c_dbl] * 4, [_c_hd]),
    # adaptive time stepping (additive to ABI 7): kdiag, koff, mdiag, moff, U0, U1, loads, phi, ne, R, s, beta0, beta1,
    # inv_dt, write_bands, adiag, aoff, b; U3, U2, U1, U0, kind_left, kind_right, ne, w3 .. w0, atol, rtol, out4, work
    "lssvr_ts_step": _sig([_c_dp] * 8, [_c_i64, _c_int], [_c_dbl] * 4, [_c_int], [_c_dp] * 3, _STREAM),
    "lssvr_ts_step_host": _sig([_c_hd] * 8, [_c_i64, _c_int], [_c_dbl] * 4, [_c_int], [_c_hd] * 3),
    "lssvr_ts_error_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_ts_error": _sig([_c_dp] * 4, [_c_int, _c_int, _c_i64], [_c_dbl] * 6, [_c_dp], _WS, _STREAM),
    "lssvr_ts_error_host": _sig([_c_hd] * 4, [_c_int, _c_int, _c_i64], [_c_dbl] * 6, [_c_hd]),
    # semilinear problems (additive to ABI 7): u, t_local, q_tabs, c_tab, f_tab, ne, n, layout, kind, nterm, c_eff,
    # f_eff, f_res; diag, sub, sup, load, u, u_new, kind_left, kind_right, end_values, kappa_host, ne, out4, work;
    # u, u_new, lambda, ne, out
    "lssvr_nl_linearize": _sig([_c_dp] * 5, [_c_i64, _c_int, _c_int, _c_int, _c_int], [_c_dp] * 3, _STREAM),
    "lssvr_nl_linearize_host": _sig([_c_hd] * 5, [_c_i64, _c_int, _c_int, _c_int, _c_int], [_c_hd] * 3),
    "lssvr_nl_residual_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_nl_residual": _sig([_c_dp] * 6, _ENDS, [_c_i64, _c_dp], _WS, _STREAM),
    "lssvr_nl_residual_host": _sig([_c_hd] * 6, [_c_int, _c_int, _c_hd, _c_hd], [_c_i64, _c_hd]),
    "lssvr_nl_step": _sig([_c_dp, _c_dp, _c_dbl, _c_i64, _c_dp], _STREAM),
    "lssvr_nl_step_host": _sig([_c_hd, _c_hd, _c_dbl, _c_i64, _c_hd]),
    # semilinear transient problems (additive to ABI 7): x, u, a_quad, cs_quad, q_quad, r, ne, nquad, kind, nterm, diag,
    # off, rhs
    "lssvr_ts_nl_assemble": _sig([_c_dp] * 6, [_c_i64, _c_int, _c_int, _c_int], [_c_dp] * 3, _STREAM),
    "lssvr_ts_nl_assemble_host": _sig([_c_hd] * 6, [_c_i64, _c_int, _c_int, _c_int], [_c_hd] * 3),
    # wave problems (additive to ABI 7): U_new, U, V, Acc, mdiag, moff, ddiag, doff, loads, phi, ne, nc, R, dt, beta,
    # gamma, V_out, Acc_out, rhs_out
    "lssvr_wave_advance": _sig([_c_dp] * 10, [_c_i64, _c_int, _c_int], [_c_dbl] * 3, [_c_dp] * 3, _STREAM),
    "lssvr_wave_advance_host": _sig([_c_hd] * 10, [_c_i64, _c_int, _c_int], [_c_dbl] * 3, [_c_hd] * 3),
    # adjoint sensitivities (additive to ABI 7): x, ne, nquad, U, nu, Z, nc, ga, gb, gc, gf, P, band_ends, kind_left,
    # kind_right, out_ends
    "lssvr_p1_sensitivity": _sig(_MESH, [_c_dp, _c_int, _c_dp, _c_int], [_c_dp] * 6, [_c_int, _c_int, _c_dp], _STREAM),
    "lssvr_p1_sensitivity_host": _sig([_c_hd, _c_i64, _c_int, _c_hd, _c_int, _c_hd, _c_int], [_c_hd] * 6,
                                      [_c_int, _c_int, _c_hd]),
    # adjoint sensitivities of the BDF loop (additive to ABI 7): x, ne, nquad, Utraj, Z, n0, m, inv_dt, coef_host, phi,
    # R, ga, gc, grho, gf, accumulate, Brows, band_ends, band_mask, kind_left, kind_right, out_g, out_kappa
    "lssvr_transient_sensitivity": _sig(_MESH, [_c_dp, _c_dp, _c_i64, _c_int, _c_dbl, _c_hd, _c_dp, _c_int],
                                        [_c_dp] * 4, [_c_int, _c_dp, _c_dp, _c_int, _c_int, _c_int, _c_dp, _c_dp],
                                        _STREAM),
    "lssvr_transient_sensitivity_host": _sig([_c_hd, _c_i64, _c_int, _c_hd, _c_hd, _c_i64, _c_int, _c_dbl, _c_hd,
                                              _c_hd, _c_int], [_c_hd] * 4,
                                             [_c_int, _c_hd, _c_hd, _c_int, _c_int, _c_int, _c_hd, _c_hd]),
    # adjoint of the element solve (additive to ABI 7): x, ne, elem_offset, ne_global, gxmin, gxmax, M, n_colloc, gamma,
    # a, da, c, f, W, status, Wbar, gu, gbc, ga, gda, gc, gf, work, work_bytes
    "lssvr_enhance_adjoint_work_bytes": _sig([_c_i64], res=_c_i64),
    "lssvr_enhance_adjoint": _sig([_c_dp, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _c_int, _c_int, _c_dbl],
                                  _REACT_TABLES, [_c_dp] * 3, [_c_dp] * 6, _WS, _STREAM),
    "lssvr_enhance_adjoint_host": _sig([_c_hd, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _c_int, _c_int, _c_dbl],
                                       [_c_hd] * 5, [_c_dp, _c_hd], [_c_hd] * 6, _WS),
    # adjoint sensitivities of the Newmark loop (additive to ABI 7).  advance: lam, Vbar, Abar, P, mdiag, moff, ddiag,
    # doff, ne, dt, beta, gamma, V_out, A_out, U_out, B_out; sensitivity: x, ne, nquad, Utraj, Vtraj, Atraj, Z, n0, m,
    # phi, R, ga, gc, grho, gd, gf, accumulate, Brows, band_ends, kind_left, kind_right, out_g, out_kappa
    "lssvr_newmark_adjoint_advance": _sig([_c_dp] * 8, [_c_i64, _c_dbl, _c_dbl, _c_dbl], [_c_dp] * 4, _STREAM),
    "lssvr_newmark_adjoint_advance_host": _sig([_c_hd] * 8, [_c_i64, _c_dbl, _c_dbl, _c_dbl], [_c_hd] * 4),
    "lssvr_newmark_sensitivity": _sig(_MESH, [_c_dp] * 4, [_c_i64, _c_int, _c_dp, _c_int], [_c_dp] * 5,
                                      [_c_int, _c_dp, _c_dp, _c_int, _c_int, _c_dp, _c_dp], _STREAM),
    "lssvr_newmark_sensitivity_host": _sig([_c_hd, _c_i64, _c_int], [_c_hd] * 4, [_c_i64, _c_int, _c_hd, _c_int],
                                           [_c_hd] * 5, [_c_int, _c_hd, _c_hd, _c_int, _c_int, _c_hd, _c_hd]),
    # adjoint sensitivities of the semilinear solve (additive to ABI 7): x, ne, nquad, U, nu, Z, nc, q_tabs, kind, nterm,
    # ga, gb, gc, gf, gq, P, band_ends, kind_left, kind_right, out_ends
    "lssvr_semilinear_sensitivity": _sig(_MESH, [_c_dp, _c_int, _c_dp, _c_int, _c_dp, _c_int, _c_int], [_c_dp] * 7,
                                         [_c_int, _c_int, _c_dp], _STREAM),
    "lssvr_semilinear_sensitivity_host": _sig([_c_hd, _c_i64, _c_int, _c_hd, _c_int, _c_hd, _c_int, _c_hd, _c_int,
                                               _c_int], [_c_hd] * 7, [_c_int, _c_int, _c_hd]),
    # adjoint sensitivities of the semilinear BDF loop (additive to ABI 7).  sensitivity: x, ne, nquad, Utraj, Z, n0, m,
    # inv_dt, coef_host, phi, R, q_tabs, kind, nterm, ga, gc, grho, gf, gq, accumulate, Brows, band_ends, kind_left,
    # kind_right, out_g, out_kappa; step: x, u, a_quad, cs_quad, q_quad, ne, nquad, kind, nterm, mdiag, moff, U0, U1,
    # loads, phi, R, beta0, beta1, inv_dt, diag, off, B, band_ends
    "lssvr_semilinear_transient_sensitivity": _sig(_MESH, [_c_dp, _c_dp, _c_i64, _c_int, _c_dbl, _c_hd, _c_dp, _c_int,
                                                           _c_dp, _c_int, _c_int], [_c_dp] * 5,
                                                   [_c_int, _c_dp, _c_dp, _c_int, _c_int, _c_dp, _c_dp], _STREAM),
    "lssvr_semilinear_transient_sensitivity_host": _sig([_c_hd, _c_i64, _c_int, _c_hd, _c_hd, _c_i64, _c_int, _c_dbl,
                                                         _c_hd, _c_hd, _c_int, _c_hd, _c_int, _c_int], [_c_hd] * 5,
                                                        [_c_int, _c_hd, _c_hd, _c_int, _c_int, _c_hd, _c_hd]),
    "lssvr_semilinear_adjoint_step": _sig([_c_dp] * 5, [_c_i64, _c_int, _c_int, _c_int], [_c_dp] * 6, [_c_int],
                                          [_c_dbl] * 3, [_c_dp] * 4, _STREAM),
    "lssvr_semilinear_adjoint_step_host": _sig([_c_hd] * 5, [_c_i64, _c_int, _c_int, _c_int], [_c_hd] * 6, [_c_int],
                                               [_c_dbl] * 3, [_c_hd] * 4),
    # bubble-condensed assembly (additive to ABI 7): x, ne, order, nquad, R, rhs_quad, a_quad, c_quad, b_quad, diag,
    # sub, sup, load, kloc4, floc, work, work_bytes
    "lssvr_p1_bubble_work_bytes": _sig([_c_i64, _c_int], res=_c_i64),
    "lssvr_p1_assemble_bubble": _sig([_c_dp, _c_i64, _c_int, _c_int, _c_int], [_c_dp] * 10, _WS, _STREAM),
    "lssvr_p1_assemble_bubble_host": _sig([_c_hd, _c_i64, _c_int, _c_int, _c_int], [_c_hd] * 10, _WS),
    "lssvr_fp64_probe":_sig([_c_dp, _c_int, _c_int, _c_int], _STREAM),
    "lssvr_stream_probe": _sig([_c_dp, _c_dp, _c_i64], _STREAM),
    "lssvr_row_chunk_probe": _sig([_c_dp, _c_dp, _c_i64, _c_int, _c_int], _STREAM),
}

_lib = None


class LssvrHipError(RuntimeError):
    """A C-ABI entry point returned a negative status."""


def load():
    """dlopen the HIP library once; raise if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C hybrid_fem_lssvr_amd/csrc` (there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    ver = lib.lssvr_version()
    if ver != ABI_VERSION:
        raise ImportError(f"liblssvr_hip.so has ABI {ver}, binding expects {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc, what):
    if rc < 0:
        msg = load().lssvr_last_error().decode("utf-8", "replace")
        raise LssvrHipError(f"{what} failed ({rc}): {msg}")
    return rc


def rhs_params(amp, omega):
    return (_c_dbl * 2)(float(amp), float(omega))
