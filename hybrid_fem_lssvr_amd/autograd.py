"""``loss.backward()`` through the P1 solve on the GPU.

:func:`p1_solve` is the forward path of ``FEMLSSVRPrimalSolver.solve_fem`` -- ``ops.p1_assemble`` plus the tridiagonal
solve -- as a ``torch.autograd.Function`` over device tensors.  Its backward is the adjoint method: one solve of the
transposed bands (``ops.adjoint_bands``) with the incoming gradient as the load, then one ``ops.p1_sensitivity`` for the
tables whose inputs require a gradient.  All arithmetic runs in the HIP kernels; there is no eager fall-back.

:func:`enhance` is the enhancement -- ``ops.enhance_varcoef`` -- the same way: its backward is one
``ops.enhance_adjoint``, so ``p1_solve(...)`` -> ``enhance(...)`` -> ``loss.backward()`` runs end to end on the device.

Limits: first derivatives only (the backward is ``once_differentiable``), and the mesh ``x`` is not differentiated --
its gradient is ``None``.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import ops

_TABLES = ("f", "a", "b", "c")      # the order of the table arguments of _P1Solve.apply after x


def _solve(fem_solver, bands, load, kinds, kappa, end_values):
    """u [1, ne+1] of the bands (diag, sub, sup | off) and the load [1, ne+1] with the solver of the facade's
    ``fem_solver``: "bands" (no pivoting) or "pivot"."""
    if fem_solver == "pivot":
        sub, sup = (bands["sub"], bands["sup"]) if "sub" in bands else (bands["off"], bands["off"])
        u, info = ops.tridiag_pivot_solve_multi(bands["diag"], sub, sup, load, kinds, kappa, end_values,
                                                return_info=True)
        bad = int(info.item())
        if bad:
            raise RuntimeError(f"P1 system singular to working precision: the pivoting tridiagonal solve met {bad} "
                               "pivot(s) that were zero or not finite")
        return u
    if "sub" in bands:
        return ops.tridiag_ns_bc_solve_multi(bands["diag"], bands["sub"], bands["sup"], load, kinds, kappa, end_values)
    return ops.tridiag_bc_solve_multi(bands["diag"], bands["off"], load, kinds, kappa, end_values)


class _P1Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rhs_quad, a_quad, b_quad, c_quad, end_values, kappa, end_kinds, nquad, fem_solver):
        tabs = {k: None if t is None else t.detach().contiguous() for k, t in zip(_TABLES, (rhs_quad, a_quad, b_quad,
                                                                                          c_quad))}
        x = x.detach().contiguous()
        kap = tuple(float(k) for k in (kappa.detach().tolist() if isinstance(kappa, torch.Tensor) else kappa))
        ev = None
        if end_values is not None:
            ev = end_values.detach() if isinstance(end_values, torch.Tensor) else torch.as_tensor(end_values)
            ev = ev.to(device=x.device, dtype=torch.float64).reshape(1, 2).contiguous()
        bands = ops.p1_assemble(x, nquad, rhs_quad=tabs["f"], a_quad=tabs["a"], b_quad=tabs["b"], c_quad=tabs["c"])
        u = _solve(fem_solver, bands, bands["load"].view(1, -1), end_kinds, kap, ev)
        ctx.bands = {k: bands[k] for k in ("diag", "off", "sub", "sup") if k in bands}
        ctx.save_for_backward(x, u)
        ctx.meta = (end_kinds, kap, nquad, fem_solver,
                    end_values if isinstance(end_values, torch.Tensor) else None,
                    kappa if isinstance(kappa, torch.Tensor) else None)
        return u[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_u):
        x, u = ctx.saved_tensors
        end_kinds, kap, nquad, fem_solver, ev_in, kappa_in = ctx.meta
        need = dict(zip(_TABLES, ctx.needs_input_grad[1:5]))
        need_ev, need_kappa = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
        P = grad_u.to(torch.float64).contiguous().view(1, -1)
        Z = _solve(fem_solver, ops.adjoint_bands(ctx.bands), P, end_kinds, kap, None)
        ends = need_ev or need_kappa
        # (the entry writes at least one table: with end gradients alone it is the load's, the cheapest)
        want = tuple(k for k in ops.SENS_TABLES if need[k]) or ("f",)
        res = ops.p1_sensitivity(x, u, Z, nquad, want=want, P=P if ends else None, bands=ctx.bands if ends else None,
                                 end_kinds=end_kinds)
        grads = [res[k][0] if need[k] else None for k in _TABLES]
        g_ev = res["ends"][0, :2].to(device=ev_in.device, dtype=ev_in.dtype).reshape(ev_in.shape) if need_ev else None
        g_kappa = (res["ends"][0, 2:].to(device=kappa_in.device, dtype=kappa_in.dtype).reshape(kappa_in.shape)
                   if need_kappa else None)
        return (None, *grads, g_ev, g_kappa, None, None, None)


def p1_solve(x, rhs_quad, *, a_quad=None, b_quad=None, c_quad=None, end_kinds=(ops.END_DIRICHLET, ops.END_DIRICHLET),
             kappa=(0.0, 0.0), end_values=None, nquad=2, fem_solver="bands"):
    """The nodal P1 solution u float64[ne+1] of -(a u')' + b u' + c u = f on the mesh ``x`` float64[ne+1], differentiable
    with respect to its data.  ``rhs_quad``, ``a_quad``, ``b_quad``, ``c_quad`` float64[ne, nquad]: f, a, b, c at
    ``ops.quad_points(x, nquad)`` (``None``: a = 1, b = 0, c = 0); ``end_kinds`` = (left, right), each
    ``ops.END_DIRICHLET`` or ``ops.END_ROBIN``; ``kappa`` a pair of floats or a float64 tensor [2] (read at a Robin end;
    its values are read back to the host, which waits for the device when it lives there); ``end_values`` a pair or a
    float64 tensor [2]: the value at a Dirichlet end, g of a Neumann or Robin end (``None``: zeros); ``fem_solver``:
    "bands" (no pivoting: the conditions of the facade apply -- cell Peclet number <= 1, c >= 0, kappa >= 0) or "pivot".
    All tensors but ``kappa`` live on the device.

    ``backward`` gives the gradients for ``rhs_quad``, ``a_quad``, ``b_quad``, ``c_quad``, ``end_values`` and ``kappa``
    -- only the tables whose inputs require a gradient are computed and stored -- and ``None`` for ``x``: the mesh is
    not differentiated.  No double backward."""
    if fem_solver not in ("bands", "pivot"):
        raise ValueError("fem_solver must be 'bands' or 'pivot'")
    kinds = tuple(int(k) for k in end_kinds)
    return _P1Solve.apply(x, rhs_quad, a_quad, b_quad, c_quad, end_values, kappa, kinds, int(nquad), fem_solver)


class _Enhance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, rhs_values, a_values, da_values, c_values, M, gamma, n_colloc, global_domain, bc):
        x, u, f = (t.detach().contiguous() for t in (x, u, rhs_values))
        a, da, c = (None if t is None else t.detach().contiguous() for t in (a_values, da_values, c_values))
        if a is None and da is not None:
            raise ValueError("da_values needs a_values")
        if global_domain is None:
            ends = torch.stack([x[0], x[-1]]).cpu()
            global_domain = (float(ends[0]), float(ends[1]))
        # (the forward entry reads tables: a = 1, a' = 0 as such; the adjoint takes None for them)
        fa = torch.ones_like(f) if a is None else a
        fda = torch.zeros_like(f) if da is None else da
        W, status = ops.enhance_varcoef(x, u, M, gamma, n_colloc, fa, fda, f, c_values=c, global_domain=global_domain,
                                        bc=bc)
        ctx.save_for_backward(x, f, W, status, *(t for t in (a, da, c) if t is not None))
        ctx.meta = (M, gamma, n_colloc, global_domain, a is not None, da is not None, c is not None)
        return W.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_W):
        M, gamma, n_colloc, global_domain, has_a, has_da, has_c = ctx.meta
        x, f, W, status, *rest = ctx.saved_tensors
        rest = list(rest)
        a = rest.pop(0) if has_a else None
        da = rest.pop(0) if has_da else None
        c = rest.pop(0) if has_c else None
        need = dict(zip(("u", "f", "a", "da", "c"), ctx.needs_input_grad[1:6]))
        want = tuple(k for k in ops.ENH_ADJ_OUTPUTS if need.get(k)) or ("u",)
        res = ops.enhance_adjoint(x, W, grad_W.to(torch.float64).contiguous(), M, gamma, n_colloc, f, a_values=a,
                                  da_values=da, c_values=c, status=status, want=want, global_domain=global_domain)
        return (None, *(res[k] if need[k] else None for k in ("u", "f", "a", "da", "c")), None, None, None, None, None)


def enhance(x, u, rhs_values, *, M, gamma, n_colloc, a_values=None, da_values=None, c_values=None, global_domain=None,
            bc=(0.0, 0.0)):
    """The enhancement coefficients W float64[ne, M] of the nodal values ``u`` float64[ne+1] on the mesh ``x``,
    differentiable with respect to their data: ``ops.enhance_varcoef`` (with ``c_values`` the reaction entry) as it is,
    element-major tables float64[ne, n_colloc] at ``ops.colloc_points(x, n_colloc)``; ``a_values=None`` means a = 1,
    a' = 0 (then ``da_values`` must be None), ``da_values`` holds a' - b with convection, ``c_values=None`` c = 0.
    ``global_domain`` (``None``: the ends of ``x``, read back) and ``bc`` as in ``ops.enhance_varcoef``: at a global end the
    forward call puts ``bc`` in place of the nodal value, and the gradient for ``u`` is 0 there.  3 <= M <= 16,
    max(2, M - 2) <= n_colloc <= 64.

    ``backward`` is ONE ``ops.enhance_adjoint`` with only the outputs whose inputs require a gradient: ``u``,
    ``rhs_values``, ``a_values``, ``da_values``, ``c_values``; ``None`` for ``x``.  An element the forward call reports
    as a fallback (the linear interpolant) differentiates by that rule.  No double backward."""
    M, n_colloc = int(M), int(n_colloc)
    if not ops.ENH_ADJ_MIN_M <= M <= ops.ENH_ADJ_MAX_M:
        raise ValueError(f"M must be in {ops.ENH_ADJ_MIN_M} .. {ops.ENH_ADJ_MAX_M}, got {M}")
    if not max(2, M - 2) <= n_colloc <= ops.ENH_ADJ_MAX_COLLOC:
        raise ValueError(f"n_colloc must be in {max(2, M - 2)} .. {ops.ENH_ADJ_MAX_COLLOC}, got {n_colloc}")
    dom = None if global_domain is None else (float(global_domain[0]), float(global_domain[1]))
    return _Enhance.apply(x, u, rhs_values, a_values, da_values, c_values, M, float(gamma), n_colloc, dom,
                          (float(bc[0]), float(bc[1])))
