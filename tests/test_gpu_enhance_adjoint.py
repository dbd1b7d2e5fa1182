"""The adjoint of the element solve on the device: lssvr_enhance_adjoint against its host mirror
(bit for bit) and against the complex step of the numpy prototype (10x the prototype's own reading on the same case),
the gather and the shards, autograd.enhance, and the facade's solve_sensitivity(of="enhanced")."""
import numpy as np
import pytest
import torch

import enhance_adjoint_rules as R
from enhance_adjoint_rules import proto

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _d(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def device_adjoint(c, want, rows=None, status=None, f=None, **kw):
    """ops.enhance_adjoint on the case (or a shard of it) -> dict of numpy arrays, canary where not wanted."""
    from hybrid_fem_lssvr_amd import ops
    sl = slice(None) if rows is None else slice(*rows)
    x = c.x if rows is None else c.x[rows[0]:rows[1] + 1]
    ne = len(x) - 1
    bufs = {k: torch.full((ne, c.n), R.CANARY, dtype=torch.float64, device=DEV) for k in R.TABLES}
    bufs.update(u=torch.full((ne + 1,), R.CANARY, dtype=torch.float64, device=DEV),
                bc=torch.full((2,), R.CANARY, dtype=torch.float64, device=DEV))
    work = torch.full((ne, 2), R.CANARY, dtype=torch.float64, device=DEV)
    cut = lambda t: None if t is None else _d(t[sl])       # noqa: E731
    ops.enhance_adjoint(_d(x), cut(c.W), cut(c.Wbar), c.M, c.gamma, c.n, cut(c.f if f is None else f), a_values=cut(c.a),
                        da_values=cut(c.da), c_values=cut(c.c), status=_d(status, torch.int32), want=want,
                        global_domain=R.DOMAIN, out={k: bufs[k] for k in want}, work=work, **kw)
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    out["pairs"] = work.cpu().numpy()
    return out


@pytest.mark.parametrize("c", R.all_cases(), ids=lambda c: c.id)
def test_device_equals_mirror_and_holds_the_bar(c):
    want = c.wants()
    got = device_adjoint(c, want)
    _, host = R.adjoint_host(c, want)
    R.check_against(got, want, host)
    assert np.array_equal(got["pairs"], host["pairs"])
    R.check_against(got, want, c.restatement)
    dev = R.deviation(dict(g=got["pairs"], **{k: got[k] for k in R.TABLES if k in want}), c)
    print(f"{c.id}: deviation {dev:.2e}, bar {c.bar:.2e}")
    assert dev <= c.bar


@pytest.mark.parametrize("want", (("f",), ("u",), ("bc", "a"), ("da", "c"), ("u", "f")), ids="-".join)
def test_null_outputs_are_left_untouched(want):
    c = R.case(65, 9, 16, True, True)
    got = device_adjoint(c, want)
    R.check_against(got, want, R.adjoint_host(c, want)[1])


def test_gather_order_and_shards():
    c = R.case(300, 9, 16, True, True)
    full = device_adjoint(c, ("u", "bc", "f"))
    gu, gbc = proto.gather(full["pairs"], True, True)
    assert np.array_equal(full["u"], gu) and np.array_equal(full["bc"], gbc)
    lo = device_adjoint(c, ("u", "bc", "f"), rows=(0, 150), elem_offset=0, ne_global=300)
    hi = device_adjoint(c, ("u", "bc", "f"), rows=(150, 300), elem_offset=150, ne_global=300)
    assert np.array_equal(np.concatenate([lo["pairs"], hi["pairs"]]), full["pairs"])
    assert np.array_equal(np.concatenate([lo["f"], hi["f"]]), full["f"])
    assert lo["bc"][1] == 0.0 and hi["bc"][0] == 0.0 and lo["bc"][0] == gbc[0] and hi["bc"][1] == gbc[1]
    assert lo["u"][150] == full["pairs"][149, 1] and hi["u"][0] == full["pairs"][150, 0]


def test_interior_shard_replaces_no_end():
    c = R.case(65, 4, 8, True, True)
    got = device_adjoint(c, c.wants(), rows=(10, 40), elem_offset=10, ne_global=65)
    _, host = R.adjoint_host(c, c.wants(), rows=(10, 40), elem_offset=10, ne_global=65)
    R.check_against(got, c.wants(), host)
    assert np.all(got["bc"] == 0.0)
    assert got["u"][0] == got["pairs"][0, 0] and got["u"][-1] == got["pairs"][-1, 1]


def test_fallback_element():
    from hybrid_fem_lssvr_amd import ops
    c = R.case(7, 9, 16, True, True)
    f = c.f.copy()
    f[3] = np.nan
    W, st = ops.enhance_varcoef(_d(c.x), _d(c.u), c.M, c.gamma, c.n, _d(c.a), _d(c.da), _d(f), c_values=_d(c.c),
                                global_domain=R.DOMAIN, bc=c.bc)
    status = st.cpu().numpy()
    assert status[3] == 1 and status.sum() == 1
    from types import SimpleNamespace
    cf = SimpleNamespace(**{k: getattr(c, k) for k in ("x", "M", "n", "gamma", "a", "da", "c", "Wbar", "f")},
                         W=W.cpu().numpy())
    got = device_adjoint(cf, R.OUTPUTS, status=status, f=f)
    assert np.array_equal(got["pairs"][3], [0.5 * (c.Wbar[3, 0] - c.Wbar[3, 1]), 0.5 * (c.Wbar[3, 0] + c.Wbar[3, 1])])
    for k in R.TABLES:
        assert np.all(got[k][3] == 0.0) and np.all(np.isfinite(got[k]))
    assert np.all(np.isfinite(got["u"])) and np.all(np.isfinite(got["pairs"]))
    _, host = R.adjoint_host(cf, R.OUTPUTS, status=status, f=f)
    R.check_against(got, R.OUTPUTS, host)


# ---- autograd.enhance ---------------------------------------------------------------------------------------------------
def _leaf(a):
    return _d(a).requires_grad_(True)


def test_autograd_gradcheck():
    from hybrid_fem_lssvr_amd import autograd
    c = R.case(3, 5, 8, True, True)
    x = _d(c.x)
    u, f, a, da, cc = (_leaf(t) for t in (c.u, c.f, c.a, c.da, c.c))
    fn = lambda u, f, a, da, cc: autograd.enhance(x, u, f, M=c.M, gamma=c.gamma, n_colloc=c.n, a_values=a,    # noqa: E731
                                                  da_values=da, c_values=cc, global_domain=R.DOMAIN, bc=c.bc)
    assert torch.autograd.gradcheck(fn, (u, f, a, da, cc), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


def test_autograd_backward_equals_ops():
    from hybrid_fem_lssvr_amd import autograd, ops
    c = R.case(65, 9, 16, True, True)
    x = _d(c.x)
    u, f, a, da, cc = (_leaf(t) for t in (c.u, c.f, c.a, c.da, c.c))
    W = autograd.enhance(x, u, f, M=c.M, gamma=c.gamma, n_colloc=c.n, a_values=a, da_values=da, c_values=cc,
                         global_domain=R.DOMAIN, bc=c.bc)
    Wbar = _d(c.Wbar)
    (W * Wbar).sum().backward()
    _, st = ops.enhance_varcoef(x, u.detach(), c.M, c.gamma, c.n, a.detach(), da.detach(), f.detach(),
                                c_values=cc.detach(), global_domain=R.DOMAIN, bc=c.bc)
    ref = ops.enhance_adjoint(x, W.detach(), Wbar, c.M, c.gamma, c.n, f.detach(), a_values=a.detach(),
                              da_values=da.detach(), c_values=cc.detach(), status=st, want=("u", "a", "da", "c", "f"),
                              global_domain=R.DOMAIN)
    for k, t in (("u", u), ("f", f), ("a", a), ("da", da), ("c", cc)):
        assert torch.equal(t.grad, ref[k]), k


# ---- the facade -------------------------------------------------------------------------------------------------------
def _facade(kinds, functional, **kw):
    ch, read, adj, cs, value = R.chain(kinds, functional)
    s = R.facade_solver(ch)
    arg = dict(goal=R.p1proto.goal_density) if functional == "goal" else dict(observe=R.p1proto.observations(ch.x))
    return ch, read, cs, value, s, s.solve_sensitivity(of="enhanced", **arg)


@pytest.mark.parametrize("functional", ("goal", "observe"))
@pytest.mark.parametrize("kinds", R.CHAIN_KINDS, ids=lambda k: "".join("DR"[i] for i in k))
def test_facade_enhanced_holds_the_bars(kinds, functional):
    ch, read, cs, value, _, sens = _facade(kinds, functional)
    got = R.facade_gradients(sens)
    assert abs(sens.value - value) <= 1e-12 * max(1.0, abs(value))
    # the reading of the whole chain is ONE number, the largest over its groups (as proto.reading is for the kernel);
    # every set of groups is held to 10x it.  (The facade's W is the forward KERNEL's, the complex step is taken at the
    # prototype's: a misfit's Wbar moves with W, so a set whose own reading is far below the chain's does not hold 10x
    # its own -- measured on the device: DD-observe collocation 3.7e-14 against 10 x 3.4e-15.)
    bar = R.MARGIN * max(read.values())
    for name, keys in proto.GROUP_SETS.items():
        dev = max(proto.deviation({k: got[k]}, {k: cs[k]}) for k in keys if k in cs)
        print(f"{name}: deviation {dev:.2e}, own reading {read[name]:.2e}, bar {bar:.2e}")
        assert dev <= bar, name
    assert np.array_equal(sens.d_convection_colloc, -sens.d_dcoef_colloc)


def test_facade_call_sequence(monkeypatch):
    from hybrid_fem_lssvr_amd import ops, solver as solver_mod
    calls = []
    for mod, name in ((ops, "enhance_adjoint"), (ops, "p1_sensitivity"), (ops, "tridiag_ns_bc_solve_multi"),
                      (ops, "tridiag_bc_solve_multi"), (ops, "tridiag_pivot_solve_multi"), (solver_mod, "_read_back")):
        def wrap(*a, _f=getattr(mod, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(mod, name, wrap)
    ch = R.chain(R.CHAIN_KINDS[0], "goal")[0]
    s = R.facade_solver(ch)
    s.solve_fem()
    calls.clear()
    monkeypatch.setattr(s, "solve_fem", lambda: None)
    s.solve_sensitivity(goal=R.p1proto.goal_density, of="enhanced")
    assert calls == ["enhance_adjoint", "tridiag_ns_bc_solve_multi", "p1_sensitivity", "_read_back"]


def test_autograd_chain_equals_facade():
    from hybrid_fem_lssvr_amd import autograd, ops
    kinds = R.CHAIN_KINDS[0]
    ch, _, _, _, s, sens = _facade(kinds, "goal")
    x = _d(ch.x)
    xq, xc = ops.quad_points(x, ch.nq), ops.colloc_points(x, ch.n)
    P = R.p1proto
    tab = lambda fn, pts: _leaf(np.asarray(fn(pts.cpu().numpy()), dtype=np.float64))     # noqa: E731
    fq, aq, bq, cq = (tab(fn, xq) for fn in (P.rhs, P.coef_a, P.convection(R.CHAIN_NE), P.reaction))
    fc, ac, cc = (tab(fn, xc) for fn in (P.rhs, P.coef_a, P.reaction))
    dac = _leaf(P.coef_da(xc.cpu().numpy()) - P.convection(R.CHAIN_NE)(xc.cpu().numpy()))
    ev = _leaf(np.array(ch.g))
    u = autograd.p1_solve(x, fq, a_quad=aq, b_quad=bq, c_quad=cq, end_kinds=kinds, end_values=ev, nquad=ch.nq)
    W = autograd.enhance(x, u, fc, M=ch.M, gamma=ch.gamma, n_colloc=ch.n, a_values=ac, da_values=dac, c_values=cc,
                         global_domain=R.DOMAIN, bc=ch.g)
    # Both routes run the same kernels on the same tables with the facade's own Wbar.  They may differ by how u reaches
    # the enhancement (the facade's solve_fem against autograd.p1_solve: an ulp or two in u), which the element solve
    # amplifies by its conditioning, about 1e3 at M = 9: 1e-12 of the largest entry of every group.
    assert np.max(np.abs(W.detach().cpu().numpy() - sens.enhanced)) <= 1e-12 * np.max(np.abs(sens.enhanced))
    Wbar = _d(s._check_sensitivity_enhanced(R.p1proto.goal_density, None)[1](sens.enhanced)[1])
    (W * Wbar).sum().backward()
    for got, ref in ((fq.grad, sens.d_rhs), (aq.grad, sens.d_coef), (bq.grad, sens.d_convection),
                     (cq.grad, sens.d_reaction), (fc.grad, sens.d_rhs_colloc), (ac.grad, sens.d_coef_colloc),
                     (dac.grad, sens.d_dcoef_colloc), (cc.grad, sens.d_reaction_colloc)):
        ref = np.asarray(ref)
        assert np.max(np.abs(got.cpu().numpy() - ref)) <= 1e-12 * np.max(np.abs(ref))
