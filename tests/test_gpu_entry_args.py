"""GPU: the argument checks of the public ``ops`` wrappers of the eigen, time, Newton and wave entries, one table over
all fourteen.  Each function has one valid call -- compared bit for bit with the library's host mirror where it has
one, every legal ``None`` included -- and one row per single mistake: the exception class and a fragment of the
message, as the wrappers raised them when each still carried its own copy of these checks.  ne = 4, nc = R = nb = 2 and
3 points per element: one block, and shapes that coincide where an output is to alias an input."""
import numpy as np
import pytest

import eigen_rules as er
import semilinear_rules as sr
import transient_adaptive_rules as ta
import transient_nl_rules as nr
import transient_rules as tr
import wave_rules as wr

pytestmark = pytest.mark.gpu

NE, NC, R, NB, N, NQUAD, NS = 4, 2, 2, 2, 3, 2, 3
INF, NAN = float("inf"), float("nan")
EPS = 2.0 ** -52

# function -> (positional arguments, keyword arguments) by name, in the wrapper's order
SIG = {
    "eig_apply": ("kdiag koff mdiag moff Z end_kinds kappa", "MZ KZ gram work"),
    "eig_ritz": ("gram sigma", "theta Q info"),
    "eig_rotate": ("Z MZ KZ Q theta end_kinds", "X Y res2 work"),
    "eig_count": ("kdiag koff mdiag moff shifts pivmin end_kinds kappa", "out"),
    "eig_rayleigh": ("x W nq a_values c_values rho_values", "point_major end_kinds kappa out work"),
    "ts_rhs": ("mdiag moff U0 U1 loads phi beta0 beta1 inv_dt", "out"),
    "ts_source_table": ("U2 U0 U1 ftab rho_tab phi alpha beta0 beta1 inv_dt", "point_major out"),
    "ts_step": ("kdiag koff mdiag moff U0 U1 loads phi s beta0 beta1 inv_dt", "adiag aoff write_bands out"),
    "ts_error": ("U3 U2 U1 U0 weights atol rtol end_kinds", "out4 work"),
    "nl_linearize": ("u t_local kind q_tabs f_tab", "c_tab point_major c_eff f_eff f_res"),
    "nl_residual": ("diag sub sup load u u_new end_kinds kappa end_values", "out4 work"),
    "nl_step": ("u u_new lam", "out"),
    "ts_nl_assemble": ("x u cs_quad kind q_quad r", "a_quad out"),
    "wave_advance": ("U_new U V Acc mdiag moff ddiag doff loads phi dt beta gamma", "V_out Acc_out rhs_out rhs"),
}


def _host_inputs(name):
    """The valid call of ``name``: numpy arrays and scalars by argument name (``None``: an output left to the wrapper)."""
    rng = np.random.default_rng(41)
    t = tr.kernel_inputs(NE, NC, R, N)
    kd, ko = 2.0 + 0.1 * np.arange(NE + 1), -1.0 + 0.05 * np.arange(NE)
    eig = dict(kdiag=kd, koff=ko, mdiag=t["md"], moff=t["mo"], end_kinds=(0, 1), kappa=(0.0, 0.5))
    if name == "eig_apply":
        return dict(eig, Z=rng.standard_normal((NB, NE + 1)), MZ=None, KZ=None, gram=None, work=None)
    if name == "eig_ritz":
        Z = rng.standard_normal((NB, 6))
        return dict(gram=np.stack([(Z * np.linspace(1.0, 3.0, 6)) @ Z.T, Z @ Z.T]), sigma=0.25, theta=None, Q=None,
                    info=None)
    if name == "eig_rotate":
        Z, MZ, KZ = rng.standard_normal((3, NB, NE + 1))
        return dict(Z=Z, MZ=MZ, KZ=KZ, Q=rng.standard_normal((NB, NB)), theta=np.array([0.5, 1.5]), end_kinds=(0, 1),
                    X=None, Y=None, res2=None, work=None)
    if name == "eig_count":
        return dict(eig, shifts=np.array([-1.0, 3.0, 1e6]), pivmin=1e-300, out=None)
    if name == "eig_rayleigh":
        return dict(x=np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, NE))]), W=rng.standard_normal((NE, 9)),
                    nq=N, a_values=rng.uniform(0.5, 2.0, (NE, N)), c_values=rng.uniform(0.0, 1.0, (NE, N)),
                    rho_values=rng.uniform(0.5, 2.0, (NE, N)), point_major=False, end_kinds=(0, 1), kappa=(0.0, 0.5),
                    out=None, work=None)
    if name == "ts_rhs":
        return dict(mdiag=t["md"], moff=t["mo"], U0=t["U0"], U1=t["U1"], loads=t["loads"], phi=t["phi"], beta0=2.0,
                    beta1=-0.5, inv_dt=10.0, out=None)
    if name == "ts_source_table":
        return dict(U2=t["U2"], U0=t["U0"][0], U1=t["U1"][0], ftab=t["ftab"], rho_tab=t["rho_tab"], phi=t["phi"][0],
                    alpha=1.5, beta0=2.0, beta1=-0.5, inv_dt=10.0, point_major=False, out=None)
    if name == "ts_step":
        return dict(kdiag=kd, koff=ko, mdiag=t["md"], moff=t["mo"], U0=t["U0"][:1], U1=t["U1"][:1], loads=t["loads"],
                    phi=t["phi"][:1], s=15.0, beta0=2.0, beta1=-0.5, inv_dt=10.0, adiag=np.zeros(NE + 1),
                    aoff=np.zeros(NE), write_bands=True, out=None)
    if name == "ts_error":
        Us, w2, _ = ta.error_inputs(NE)
        return dict(U3=Us[0], U2=Us[1], U1=Us[2], U0=Us[3], weights=tuple(float(v) for v in w2), atol=1e-6, rtol=1e-4,
                    end_kinds=(0, 1), out4=None, work=None)
    if name in ("nl_linearize", "nl_residual", "nl_step"):
        d = sr.kernel_inputs(NE, N, sr.POLY, 2)
        if name == "nl_linearize":
            return dict(u=d["u"], t_local=d["t"], kind="poly", q_tabs=d["q"], f_tab=d["f"], c_tab=d["c"],
                        point_major=False, c_eff=True, f_eff=True, f_res=False)
        if name == "nl_residual":
            return dict(diag=d["diag"], sub=d["sub"], sup=d["sup"], load=d["load"], u=d["u"], u_new=d["u_new"],
                        end_kinds=(0, 1), kappa=d["kappa"], end_values=d["g"], out4=None, work=None)
        return dict(u=d["u"], u_new=d["u_new"], lam=0.5, out=None)
    if name == "ts_nl_assemble":
        d = nr.kernel_inputs(NE, NQUAD, sr.POLY, 2)
        return dict(x=d["x"], u=d["u"], cs_quad=d["cs"], kind="poly", q_quad=d["q"], r=d["r"], a_quad=d["a"], out=None)
    assert name == "wave_advance"
    d = wr.kernel_inputs(NE, NC, R)
    return dict(U_new=d["U_new"], U=d["U"], V=d["V"], Acc=d["Acc"], mdiag=d["md"], moff=d["mo"], ddiag=d["dd"],
                doff=d["do"], loads=d["loads"], phi=d["phi"], dt=wr.KERNEL_DT, beta=0.25, gamma=0.5, V_out=None,
                Acc_out=None, rhs_out=None, rhs=True)


def _device(a, dev):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(v), device=dev) if isinstance(v, np.ndarray) else v
            for k, v in a.items()}


def _call(name, a):
    from hybrid_fem_lssvr_amd import ops
    pos, kw = (s.split() for s in SIG[name])
    assert set(a) == set(pos) | set(kw), name
    return getattr(ops, name)(*[a[k] for k in pos], **{k: a[k] for k in kw})


# ---- one mistake: a function (a, dev) that changes the valid arguments in place ------------------------------------------
def host(nm):
    return lambda a, dev: a.update({nm: a[nm].cpu()})


def f32(nm):
    return lambda a, dev: a.update({nm: a[nm].float()})


def strided(nm):
    def go(a, dev):
        import torch
        t = a[nm]
        a[nm] = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=dev)[..., ::2]
        assert a[nm].shape == t.shape and not a[nm].is_contiguous()
    return go


def shape(nm, *dims, int32=False):
    def go(a, dev):
        import torch
        a[nm] = torch.ones(dims, dtype=torch.int32 if int32 else torch.float64, device=dev)
    return go


def put(**kv):
    return lambda a, dev: a.update(kv)


def view_of(t, dims):
    """A contiguous view of ``t``'s first doubles in the shape ``dims``: the same ``data_ptr()``."""
    count = int(np.prod(dims))
    assert t.numel() >= count
    return t.reshape(-1)[:count].view(*dims)


def alias(out, src, *dims):
    return lambda a, dev: a.update({out: view_of(a[src], dims)})


def short(sizer, *sargs):
    def go(a, dev):
        import torch
        from hybrid_fem_lssvr_amd import _capi
        need = getattr(_capi.load(), sizer)(*sargs)
        assert need >= 8
        a["work"] = torch.zeros((need - 1) // 8, dtype=torch.float64, device=dev)
    return go


def other_device(nm, dims=None):
    def go(a, dev):
        import torch
        if torch.cuda.device_count() < 2:
            pytest.skip("needs a second device")
        a[nm] = (a[nm] if dims is None else torch.zeros(dims, dtype=torch.float64)).to("cuda:1")
    return go


def out_dict(**src):
    """``out`` of ts_nl_assemble: fresh buffers, but ``key=(name of an input | of another key)``."""
    def go(a, dev):
        import torch
        want = {"diag": (NE + 1,), "off": (NE,), "rhs": (NE + 1,)}
        out = {k: torch.zeros(s, dtype=torch.float64, device=dev) for k, s in want.items()}
        for k, s in src.items():
            out[k] = view_of(out[s] if s in out else a[s], want[k])
        a["out"] = out
    return go


V, T, RT = ValueError, TypeError, RuntimeError
_KINDS = [("kinds", put(end_kinds=(0, 2)), V, "end_kinds must be END_DIRICHLET")]
_KAPPA = [("kappa-nan", put(kappa=(0.0, NAN)), V, "kappa must be finite"),
          ("kappa-inf", put(kappa=(INF, 0.0)), V, "kappa must be finite")]


def _common(h, f, s):
    return [("host-" + h, host(h), RT, "no CPU fallback"), ("f32-" + f, f32(f), T, f + ": expected torch.float64"),
            ("strided-" + s, strided(s), V, s + ": must be contiguous")]


def _scalars(*names):
    return [("%s-%r" % (nm, v), put(**{nm: v}), V, nm + " must be finite") for nm in names for v in (INF, NAN)]


def _eig_bands():
    return [("short-" + nm, shape(nm, n), V, r"band lengths must be ne\+1, ne, ne\+1, ne \(kdiag, koff, mdiag, moff\)")
            for nm, n in (("kdiag", NE), ("koff", NE - 1), ("mdiag", NE), ("moff", NE - 1))] + \
        [("no-element", lambda a, dev: [shape(nm, n)(a, dev) for nm, n in (("kdiag", 1), ("koff", 0), ("mdiag", 1),
                                                                            ("moff", 0))], V, "need at least one element")]


def _block(nm, words, cols=NE + 1):
    return [("%s-%dx%d" % (nm, r, c), shape(nm, r, c), V, words) for r, c in ((0, cols), (9, cols), (2, cols - 1))]


_LOADS = _block("loads", r"loads must be \[R, ne\+1\] = \[1 \.\. 8, 5\]")
_U1 = [("U1-missing", put(U1=None), V, "U1 is needed when beta1 != 0")]
_INPUT = "must be distinct and none of them an input"
_THREE = "adiag, aoff and out must be three buffers of their own, none of them an input"

ROWS = {
    "eig_apply": _common("kdiag", "Z", "koff") + _eig_bands() + _block("Z", r"Z must be \[nb, ne\+1\] = \[1 \.\. 8, 5\]") +
    _KINDS + _KAPPA + [
        ("MZ-shape", shape("MZ", NB, NE), V, r"MZ must be \[2, 5\]"),
        ("KZ-shape", shape("KZ", 1, NE + 1), V, r"KZ must be \[2, 5\]"),
        ("gram-shape", shape("gram", 2, NB, 3), V, r"gram must be \[2, 2, 2\]"),
        ("work-short", short("lssvr_eig_work_bytes", NE, NB), V, r"work holds \d+ bytes, lssvr_eig_work_bytes\(4, 2\) = "),
        ("work-host", lambda a, dev: shape("work", 4096)(a, "cpu"), RT, "no CPU fallback"),
        ("device", other_device("koff"), RT, "koff lives on")],
    "eig_ritz": _common("gram", "gram", "gram") + _scalars("sigma") + [
        ("gram-%s" % "x".join(map(str, s)), shape("gram", *s), V, r"gram must be \[2, nb, nb\] with nb in 1 \.\. 8")
        for s in ((2, 0, 0), (2, 9, 9), (3, 2, 2), (2, 2, 3), (2, 2))] + [
        ("theta-shape", shape("theta", 3), V, r"theta must be \[2\]"),
        ("Q-shape", shape("Q", 2, 3), V, r"Q must be \[2, 2\]"),
        ("info-dtype", shape("info", 1), T, "info: expected torch.int32"),
        ("info-shape", shape("info", 2, int32=True), V, r"info must be \[1\]"),
        ("device", other_device("theta", (NB,)), RT, "theta lives on")],
    "eig_rotate": _common("Z", "MZ", "KZ") + _KINDS + [
        ("Z-one-node", shape("Z", NB, 1), V, r"Z must be \[nb, ne\+1\] with ne >= 1"),
        ("Z-1d", shape("Z", NE + 1), V, r"Z must be \[nb, ne\+1\] with ne >= 1"),
        ("Z-0-rows", lambda a, dev: [shape(nm, 0, NE + 1)(a, dev) for nm in ("Z", "MZ", "KZ")], V,
         r"Z must be \[nb, ne\+1\] = \[1 \.\. 8, 5\]"),
        ("Z-9-rows", lambda a, dev: [shape(nm, 9, NE + 1)(a, dev) for nm in ("Z", "MZ", "KZ")], V,
         r"Z must be \[nb, ne\+1\] = \[1 \.\. 8, 5\]"),
        ("MZ-rows", shape("MZ", 1, NE + 1), V, "MZ must hold nb = 2 vectors, got 1"),
        ("KZ-cols", shape("KZ", NB, NE), V, r"KZ must be \[nb, ne\+1\]"),
        ("Q-shape", shape("Q", NB, 3), V, r"Q must be \[2, 2\] and theta \[2\]"),
        ("theta-shape", shape("theta", 3), V, r"Q must be \[2, 2\] and theta \[2\]"),
        ("X-shape", shape("X", NB, NE), V, r"X must be \[2, 5\]"),
        ("res2-shape", shape("res2", 2, 3), V, r"res2 must be \[2, 2\]"),
        ("work-short", short("lssvr_eig_work_bytes", NE, NB), V, r"work holds \d+ bytes, lssvr_eig_work_bytes\(4, 2\) = "),
        ("device", other_device("MZ"), RT, "MZ lives on")] + [
        ("%s-is-%s" % (o, i), alias(o, i, NB, NE + 1), V, o + " must not be Z, MZ or KZ")
        for o in ("X", "Y") for i in ("Z", "MZ", "KZ")],
    "eig_count": _common("shifts", "shifts", "shifts") + _eig_bands() + _KINDS + _KAPPA + [
        ("shifts-2d", shape("shifts", 1, NS), V, "shifts must be 1-D"),
        ("out-shape", shape("out", NS + 1, int32=True), V, r"out must be \[3\]"),
        ("out-dtype", shape("out", NS), T, "out: expected torch.int32"),
        ("device", other_device("shifts"), RT, "shifts lives on")] + [
        ("pivmin-%r" % v, put(pivmin=v), V, "pivmin must be finite and > 0") for v in (0.0, -1.0, INF, NAN)],
    "eig_rayleigh": _common("x", "W", "a_values") + _KINDS + _KAPPA + [
        ("x-one-node", shape("x", 1), V, "x must be 1-D with at least two nodes"),
        ("x-2d", shape("x", 1, NE + 1), V, "x must be 1-D with at least two nodes"),
        ("W-rows", shape("W", NE - 1, 9), V, r"W must be \[ne, M\]"),
        ("a-shape", shape("a_values", NE, N - 1), V, r"a_values must be \[ne, nq\] = \[4, 3\]"),
        ("c-shape", shape("c_values", N, NE), V, r"c_values must be \[ne, nq\] = \[4, 3\]"),
        ("rho-shape", shape("rho_values", NE * N), V, r"rho_values must be \[ne, nq\] = \[4, 3\]"),
        ("pm-shape", put(point_major=True), V, r"a_values must be \[nq, ne\] = \[3, 4\]"),
        ("out-shape", shape("out", 4), V, r"out must be \[3\]"),
        ("work-short", short("lssvr_eig_work_bytes", NE, 1), V, r"work holds \d+ bytes, lssvr_eig_work_bytes\(4, 1\) = "),
        ("device", other_device("W"), RT, "W lives on")],
    "ts_rhs": _common("mdiag", "U0", "loads") + _scalars("beta0", "beta1", "inv_dt") + _LOADS + _U1 +
    _block("U0", r"U0 must be \[nc, ne\+1\] = \[1 \.\. 8, 5\]") + [
        ("mdiag-short", shape("mdiag", NE), V, r"band lengths must be ne\+1, ne \(mdiag, moff\)"),
        ("moff-short", shape("moff", NE - 1), V, r"band lengths must be ne\+1, ne \(mdiag, moff\)"),
        ("no-element", shape("moff", 0), V, "need at least one element"),
        ("phi-cols", shape("phi", NC, R + 1), V, r"phi must be \[nc, R\] = \[2, 2\]"),
        ("phi-rows", shape("phi", NC + 1, R), V, r"phi must be \[nc, R\] = \[2, 2\]"),
        ("U1-shape", shape("U1", NC, NE), V, r"U1 must have the shape of U0 \[2, 5\]"),
        ("U1-host", host("U1"), RT, "no CPU fallback"),
        ("out-is-U0", alias("out", "U0", NC, NE + 1), V, "out must not be U0 or U1"),
        ("out-is-U1", alias("out", "U1", NC, NE + 1), V, "out must not be U0 or U1"),
        ("out-shape", shape("out", NC, NE), V, r"out must be \[2, 5\]"),
        ("device", other_device("moff"), RT, "moff lives on")],
    "ts_source_table": _common("U2", "ftab", "rho_tab") + _scalars("alpha", "beta0", "beta1", "inv_dt") + _U1 + [
        ("U2-one-node", shape("U2", 1), V, "U2 must be 1-D with at least two nodes"),
        ("rho-rows", shape("rho_tab", NE - 1, N), V, r"rho_tab must be \[ne, n_colloc\] with ne = 4"),
        ("rho-pm", put(point_major=True), V, r"rho_tab must be \[n_colloc, ne\] with ne = 4"),
        ("one-point", lambda a, dev: (shape("rho_tab", NE, 1)(a, dev), shape("ftab", R, NE, 1)(a, dev)), V,
         "n_colloc must be >= 2, got 1"),
        ("ftab-0", shape("ftab", 0, NE, N), V, r"ftab must be \[R, \.\.\.\] = \[1 \.\. 8, 4, 3\]"),
        ("ftab-9", shape("ftab", 9, NE, N), V, r"ftab must be \[R, \.\.\.\] = \[1 \.\. 8, 4, 3\]"),
        ("ftab-points", shape("ftab", R, NE, N - 1), V, r"ftab must be \[R, \.\.\.\] = \[1 \.\. 8, 4, 3\]"),
        ("phi-shape", shape("phi", R + 1), V, r"phi must be \[R\] = \[2\]"),
        ("U0-shape", shape("U0", NE), V, r"U0 must have the shape of U2 \[5\]"),
        ("U1-shape", shape("U1", NE), V, r"U1 must have the shape of U2 \[5\]"),
        ("out-shape", shape("out", NE, N - 1), V, r"out must be \[4, 3\]"),
        ("device", other_device("U0"), RT, "U0 lives on")],
    "ts_step": _common("kdiag", "U0", "loads") + _scalars("s", "beta0", "beta1", "inv_dt") + _LOADS + _U1 + [
        ("short-" + nm, shape(nm, n), V, r"band lengths must be ne\+1 \(kdiag, mdiag, adiag\) and ne \(koff, moff, aoff\)")
        for nm, n in (("kdiag", NE), ("koff", NE - 1), ("mdiag", NE), ("moff", NE - 1), ("adiag", NE), ("aoff", NE - 1))] + [
        ("no-element", shape("moff", 0), V, "need at least one element"),
        ("U0-two-cases", shape("U0", 2, NE + 1), V, r"U0 must be \[1, ne\+1\] = \[1, 5\]"),
        ("U0-1d", shape("U0", NE + 1), V, r"U0 must be \[1, ne\+1\] = \[1, 5\]"),
        ("phi-rows", shape("phi", 2, R), V, r"phi must be \[nc, R\] = \[1, 2\]"),
        ("U1-shape", shape("U1", 1, NE), V, r"U1 must have the shape of U0 \[1, 5\]"),
        ("out-is-U0", alias("out", "U0", 1, NE + 1), V, "out must not be U0 or U1"),
        ("out-is-U1", alias("out", "U1", 1, NE + 1), V, "out must not be U0 or U1"),
        ("out-shape", shape("out", NE + 1), V, r"out must be \[1, 5\]"),
        ("aoff-is-adiag", alias("aoff", "adiag", NE), V, _THREE),
        ("out-is-adiag", alias("out", "adiag", 1, NE + 1), V, _THREE),
        ("device", other_device("koff"), RT, "koff lives on")] + [
        ("adiag-is-" + i, alias("adiag", i, NE + 1), V, _THREE) for i in ("kdiag", "mdiag", "U0", "U1", "loads")] + [
        ("aoff-is-" + i, alias("aoff", i, NE), V, _THREE)
        for i in ("kdiag", "koff", "mdiag", "moff", "U0", "U1", "loads")] + [
        ("out-is-" + i, alias("out", i, 1, NE + 1), V, _THREE) for i in ("kdiag", "mdiag", "loads")],
    "ts_error": _common("U3", "U2", "U1") + _KINDS + _scalars("atol", "rtol") + [
        ("weights-3", put(weights=(1.0, -2.0, 1.0)), V, r"weights must be \(w3, w2, w1, w0\), got 3 values")] + [
        ("w%d-nan" % (3 - i), lambda a, dev, i=i: a.update(weights=tuple(NAN if j == i else w for j, w in
                                                                           enumerate(a["weights"]))), V,
         "w%d must be finite" % (3 - i)) for i in range(4)] + [
        ("atol-negative", put(atol=-1e-6), V, "atol and rtol must be >= 0 and their sum > 0"),
        ("rtol-negative", put(rtol=-1e-4), V, "atol and rtol must be >= 0 and their sum > 0"),
        ("tol-zero", put(atol=0.0, rtol=0.0), V, "atol and rtol must be >= 0 and their sum > 0"),
        ("U3-one-node", shape("U3", 1), V, "U3 must be 1-D with at least two nodes"),
        ("U2-shape", shape("U2", NE), V, r"U2 must have the shape of U3 \[5\]"),
        ("U0-shape", shape("U0", NE), V, r"U0 must have the shape of U3 \[5\]"),
        ("U1-missing", put(U1=None), V, "U1 is needed when w1 != 0"),
        ("U0-missing", put(U0=None), V, "U0 is needed when w0 != 0"),
        ("out4-shape", shape("out4", 3), V, r"out4 must be \[4\]"),
        ("work-short", short("lssvr_ts_error_work_bytes", NE), V,
         r"work holds \d+ bytes, lssvr_ts_error_work_bytes\(4\) = "),
        ("device", other_device("U2"), RT, "U2 lives on")],
    "nl_linearize": _common("u", "q_tabs", "f_tab") + [
        ("u-one-node", shape("u", 1), V, "u must be 1-D with at least two nodes"),
        ("f-rows", shape("f_tab", NE - 1, N), V, r"f_tab must be \[ne, n\] with ne = 4"),
        ("f-pm", put(point_major=True), V, r"f_tab must be \[n, ne\] with ne = 4"),
        ("n-65", shape("f_tab", NE, 65), V, r"n = 65 points per element outside 1 \.\. 64"),
        ("n-0", shape("f_tab", NE, 0), V, r"n = 0 points per element outside 1 \.\. 64"),
        ("t-shape", shape("t_local", N + 1), V, r"t_local must be \[n\] = \[3\]"),
        ("q-points", shape("q_tabs", 2, NE, N - 1), V, r"q_tabs must be \[nterm, 4, 3\]"),
        ("kind-unknown", put(kind=7), V, r"kind must be 'poly' \(NL_POLY\) or 'exp' \(NL_EXP\), got 7"),
        ("kind-bool", put(kind=True), V, "kind must be 'poly'"),
        ("poly-7", shape("q_tabs", 7, NE, N), V, r"nterm = 7 outside 1 \.\. 6"),
        ("poly-0", shape("q_tabs", 0, NE, N), V, r"nterm = 0 outside 1 \.\. 6"),
        ("exp-3", lambda a, dev: (put(kind="exp")(a, dev), shape("q_tabs", 3, NE, N)(a, dev)), V,
         "kind 'exp' takes the two tables q_0, q_1, got 3"),
        ("c-shape", shape("c_tab", NE, N - 1), V, r"c_tab must have the shape of f_tab \[4, 3\]"),
        ("no-output", put(c_eff=False, f_eff=None), V, "one of c_eff, f_eff, f_res must be asked for"),
        ("c_eff-shape", shape("c_eff", NE, N - 1), V, r"c_eff must be \[4, 3\]"),
        ("f_res-host", lambda a, dev: shape("f_res", NE, N)(a, "cpu"), RT, "no CPU fallback"),
        ("device", other_device("t_local"), RT, "t_local lives on")] + [
        # the library refuses these, before it launches
        ("%s-is-%s" % (o, i), alias(o, i, NE, N), RT, "an output must not be one of the inputs")
        for o, i in (("c_eff", "f_tab"), ("f_eff", "c_tab"), ("f_res", "q_tabs"), ("f_res", "f_tab"))] + [
        ("c_eff-is-f_eff", lambda a, dev: (shape("c_eff", NE, N)(a, dev), a.update(f_eff=a["c_eff"])), RT,
         "c_eff, f_eff, f_res must be distinct")],
    "nl_residual": _common("diag", "load", "u_new") + _KINDS + _KAPPA + [
        ("short-" + nm, shape(nm, n), V, r"lengths must be ne\+1 \(diag, load, u, u_new\) and ne \(sub, sup\)")
        for nm, n in (("diag", NE), ("sub", NE - 1), ("sup", NE - 1), ("load", NE), ("u", NE), ("u_new", NE))] + [
        ("no-element", shape("sub", 0), V, "need at least one element"),
        ("robin-no-values", put(end_values=None), V, r"end_values \(device float64\[2\]\) is needed with a Robin end"),
        ("values-3", shape("end_values", 3), V, "end_values must hold 2 doubles, got 3"),
        ("out4-shape", shape("out4", 3), V, r"out4 must be \[4\]"),
        ("work-short", short("lssvr_nl_residual_work_bytes", NE), V,
         r"work holds \d+ bytes, lssvr_nl_residual_work_bytes\(4\) = "),
        ("device", other_device("sub"), RT, "sub lives on")],
    "nl_step": _common("u", "u_new", "u") + _scalars("lam") + [
        ("one-node", lambda a, dev: (shape("u", 1)(a, dev), shape("u_new", 1)(a, dev)), V,
         r"u and u_new must be 1-D of one length ne\+1 >= 2"),
        ("u_new-shape", shape("u_new", NE), V, r"u and u_new must be 1-D of one length ne\+1 >= 2"),
        ("u-2d", lambda a, dev: (shape("u", 1, NE + 1)(a, dev), shape("u_new", 1, NE + 1)(a, dev)), V,
         r"u and u_new must be 1-D of one length ne\+1 >= 2"),
        ("out-is-u", alias("out", "u", NE + 1), V, "out must not be u or u_new"),
        ("out-is-u_new", alias("out", "u_new", NE + 1), V, "out must not be u or u_new"),
        ("out-shape", shape("out", NE), V, r"out must be \[5\]"),
        ("device", other_device("u_new"), RT, "u_new lives on")],
    "ts_nl_assemble": _common("x", "cs_quad", "q_quad") + [
        ("x-one-node", shape("x", 1), V, "x must be 1-D with at least two nodes"),
        ("u-shape", shape("u", NE), V, r"u must be \[ne\+1\] = \[5\]"),
        ("r-shape", shape("r", NE + 2), V, r"r must be \[ne\+1\] = \[5\]"),
        ("cs-rows", shape("cs_quad", NE - 1, NQUAD), V, r"cs_quad must be \[ne, nquad\] = \[4, 1 \.\. 5\]"),
        ("nquad-6", shape("cs_quad", NE, 6), V, r"cs_quad must be \[ne, nquad\] = \[4, 1 \.\. 5\]"),
        ("nquad-0", shape("cs_quad", NE, 0), V, r"cs_quad must be \[ne, nquad\] = \[4, 1 \.\. 5\]"),
        ("q-points", shape("q_quad", 2, NE, NQUAD + 1), V, r"q_quad must be \[nterm, 4, 2\]"),
        ("kind-unknown", put(kind="cubic"), V, "kind must be 'poly'"),
        ("poly-7", shape("q_quad", 7, NE, NQUAD), V, r"nterm = 7 outside 1 \.\. 6"),
        ("exp-3", lambda a, dev: (put(kind="exp")(a, dev), shape("q_quad", 3, NE, NQUAD)(a, dev)), V,
         "kind 'exp' takes the two tables q_0, q_1, got 3"),
        ("a-shape", shape("a_quad", NE, NQUAD + 1), V, r"a_quad must have the shape of cs_quad \[4, 2\]"),
        ("out-no-dict", put(out=[1, 2, 3]), V, "out must be a dict with diag, off and rhs"),
        ("out-no-rhs", lambda a, dev: (out_dict()(a, dev), a["out"].pop("rhs")), V,
         "out must be a dict with diag, off and rhs"),
        ("diag-shape", lambda a, dev: (out_dict()(a, dev), shape("diag", NE)(a["out"], dev)), V, r"diag must be \[5\]"),
        ("device", other_device("u"), RT, "u lives on")] + [
        ("%s-is-%s" % (o, i), out_dict(**{o: i}), V, _INPUT)
        for o in ("diag", "off", "rhs") for i in ("x", "u", "cs_quad", "q_quad", "r", "a_quad")] + [
        ("%s-is-%s" % (o, i), out_dict(**{o: i}), V, _INPUT) for o, i in (("off", "diag"), ("rhs", "diag"), ("off", "rhs"))],
    "wave_advance": _common("U", "V", "Acc") + _scalars("dt", "beta", "gamma") + _LOADS + [
        ("nothing", put(U_new=None, rhs=False), V, "U_new=None with rhs=False leaves nothing to compute")] + [
        ("%s-%r" % (nm, v), put(**{nm: v}), V, "dt, beta and gamma must be > 0")
        for nm in ("dt", "beta", "gamma") for v in (0.0, -0.1)] + [
        ("U-%dx%d" % s, lambda a, dev, s=s: [shape(nm, *s)(a, dev) for nm in ("U_new", "U", "V", "Acc")], V,
         r"U must be \[nc, ne\+1\] with nc in 1 \.\. 8 and ne >= 1") for s in ((0, NE + 1), (9, NE + 1), (NC, 1))] + [
        ("%s-shape" % nm, shape(nm, NC, NE), V, nm + r" must have the shape of U \[2, 5\]")
        for nm in ("V", "Acc", "U_new")] + [
        ("%s-missing" % nm, put(**{nm: None}), V, nm + " is needed for the right-hand side")
        for nm in ("mdiag", "moff", "loads", "phi")] + [
        ("mdiag-short", shape("mdiag", NE), V, r"band lengths must be ne\+1, ne = 5, 4 \(mdiag, moff\)"),
        ("moff-short", shape("moff", NE - 1), V, r"band lengths must be ne\+1, ne = 5, 4 \(mdiag, moff\)"),
        ("ddiag-short", shape("ddiag", NE), V, r"band lengths must be ne\+1, ne = 5, 4 \(ddiag, doff\)"),
        ("doff-short", shape("doff", NE - 1), V, r"band lengths must be ne\+1, ne = 5, 4 \(ddiag, doff\)"),
        ("doff-missing", put(doff=None), V, "doff is needed with ddiag"),
        ("phi-cols", shape("phi", NC, R + 1), V, r"phi must be \[nc, R\] = \[2, 2\]"),
        ("V_out-shape", shape("V_out", NC, NE), V, r"V_out must be \[2, 5\]"),
        ("rhs_out-shape", shape("rhs_out", NE + 1), V, r"rhs_out must be \[2, 5\]"),
        ("Acc_out-is-V_out", lambda a, dev: (shape("V_out", NC, NE + 1)(a, dev), a.update(Acc_out=a["V_out"])), V, _INPUT),
        ("rhs_out-is-V_out", lambda a, dev: (shape("V_out", NC, NE + 1)(a, dev), a.update(rhs_out=a["V_out"])), V, _INPUT),
        ("device", other_device("V"), RT, "V lives on")] + [
        ("%s-is-%s" % (o, i), alias(o, i, NC, NE + 1), V, _INPUT)
        for o in ("V_out", "Acc_out", "rhs_out") for i in ("U_new", "U", "V", "Acc", "loads")],
}

CASES = [pytest.param(name, go, exc, words, id="%s-%s" % (name, rid)) for name, rows in ROWS.items()
         for rid, go, exc, words in rows]


@pytest.mark.parametrize("name,go,exc,words", CASES)
def test_one_mistake(dev, name, go, exc, words):
    a = _device(_host_inputs(name), dev)
    go(a, dev)
    with pytest.raises(exc, match=words):
        _call(name, a)


def test_row_ids_are_unique_and_every_wrapper_has_rows():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)) and set(ROWS) == set(SIG) and all(len(r) >= 10 for r in ROWS.values())


# ---- the valid calls, each legal None included, against the host mirrors ------------------------------------------------
def _np(t):
    return None if t is None else t.cpu().numpy()


def _same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


def _run(name, dev, **change):
    h = dict(_host_inputs(name), **change)
    return h, _call(name, _device(h, dev))


def test_valid_eig_apply(dev):
    """No host mirror: the dense products, each sum of n terms within 2 n eps of the sum of the sizes of its terms."""
    h, (MZ, KZ, gram) = _run("eig_apply", dev)
    n = NE + 1
    K = np.diag(h["kdiag"]) + np.diag(h["koff"], 1) + np.diag(h["koff"], -1)
    M = np.diag(h["mdiag"]) + np.diag(h["moff"], 1) + np.diag(h["moff"], -1)
    K[n - 1, n - 1] += h["kappa"][1]
    free = np.arange(1, n)                                    # a Dirichlet left end: node 0 is no unknown
    Z = np.zeros_like(h["Z"])
    Z[:, free] = h["Z"][:, free]
    for got, A in ((_np(MZ), M), (_np(KZ), K)):
        assert np.all(got[:, 0] == 0.0)
        assert np.all(np.abs(got[:, free] - (Z @ A)[:, free]) <= 8 * EPS * (np.abs(Z) @ np.abs(A))[:, free])
    for got, A in zip(_np(gram), (K, M)):
        assert np.all(np.abs(got - Z @ A @ Z.T) <= 4 * n * EPS * (np.abs(Z) @ np.abs(A) @ np.abs(Z).T))


def test_valid_eig_ritz(dev):
    h, (theta, Q, info) = _run("eig_ritz", dev)
    th, Qh, bad = er.ritz_host(h["gram"][0], h["gram"][1], h["sigma"])
    assert _same(_np(theta), th) and _same(_np(Q), Qh) and int(info.item()) == bad == 0


def test_valid_eig_rotate(dev):
    """No host mirror: X = Z Q and Y = (MZ) Q at the interior nodes up to the sign of each column, two-term sums."""
    import torch
    h, (X, Y, res2) = _run("eig_rotate", dev)
    for got, B in ((_np(X), h["Z"]), (_np(Y), h["MZ"])):
        want, size = h["Q"].T @ B, np.abs(h["Q"].T) @ np.abs(B)
        assert got.shape == (NB, NE + 1)
        assert np.all(np.abs(np.abs(got[:, 1:NE]) - np.abs(want[:, 1:NE])) <= 4 * EPS * size[:, 1:NE])
    assert tuple(res2.shape) == (2, NB) and bool(torch.isfinite(res2).all()) and bool((res2[1] > 0).all())
    a = _device(h, dev)
    a.update(X=torch.zeros_like(X), Y=torch.zeros_like(Y), res2=torch.zeros_like(res2))
    X2, Y2, r2 = _call("eig_rotate", a)
    assert X2.data_ptr() == a["X"].data_ptr() and torch.equal(X2, X) and torch.equal(Y2, Y) and torch.equal(r2, res2)


def test_valid_eig_count(dev):
    h, out = _run("eig_count", dev)
    want = er.count_host((h["kdiag"], h["koff"], h["mdiag"], h["moff"]), h["end_kinds"], h["kappa"], h["shifts"],
                         h["pivmin"])
    assert _same(_np(out), want) and want[0] == 0 and want[-1] == NE


def test_valid_eig_rayleigh(dev):
    """No host mirror: both layouts, and the caller's buffers, give the same three sums; the mass term is positive."""
    import torch
    from hybrid_fem_lssvr_amd import _capi
    h, out = _run("eig_rayleigh", dev)
    assert tuple(out.shape) == (3,) and bool(torch.isfinite(out).all()) and float(out[1]) > 0.0
    pm = {k: np.ascontiguousarray(h[k].T) for k in ("a_values", "c_values", "rho_values")}
    out_pm = _run("eig_rayleigh", dev, point_major=True, **pm)[1]          # the same NE * N terms per sum
    assert bool((torch.abs(out_pm - out) <= 4 * NE * N * EPS * out[2]).all())
    a = _device(h, dev)
    need = _capi.load().lssvr_eig_work_bytes(NE, 1)
    a.update(out=torch.zeros(3, dtype=torch.float64, device=dev),
             work=torch.zeros((need + 7) // 8, dtype=torch.float64, device=dev))
    out2 = _call("eig_rayleigh", a)
    assert out2.data_ptr() == a["out"].data_ptr() and torch.equal(out2, out)


def test_valid_ts_rhs(dev):
    for change in ({}, dict(U1=None, beta1=0.0), dict(beta1=0.0)):
        h, out = _run("ts_rhs", dev, **change)
        want = tr.rhs_host(h["mdiag"], h["moff"], h["U0"], h["U1"], h["loads"], h["phi"], h["beta0"], h["beta1"],
                           h["inv_dt"])[1]
        assert _same(_np(out), want), change


def test_valid_ts_source_table(dev):
    for pm in (False, True):
        for change in ({}, dict(U1=None, beta1=0.0)):
            h = _host_inputs("ts_source_table")
            if pm:
                change = dict(change, point_major=True, ftab=np.ascontiguousarray(np.transpose(h["ftab"], (0, 2, 1))),
                              rho_tab=np.ascontiguousarray(h["rho_tab"].T))
            h, out = _run("ts_source_table", dev, **change)
            want = tr.source_host(h["U2"], h["U0"], h["U1"], h["ftab"], h["rho_tab"], h["phi"], h["alpha"], h["beta0"],
                                  h["beta1"], h["inv_dt"], pm)[1]
            assert _same(_np(out), want), (pm, change)


def test_valid_ts_step(dev):
    import torch
    for change in ({}, dict(U1=None, beta1=0.0), dict(write_bands=False)):
        h = dict(_host_inputs("ts_step"), **change)
        a = _device(h, dev)
        a["adiag"].fill_(-7.0)
        a["aoff"].fill_(-7.0)
        out = _call("ts_step", a)
        _, adiag, aoff, b = ta.step_host(h["kdiag"], h["koff"], h["mdiag"], h["moff"], h["U0"][0],
                                         None if h["U1"] is None else h["U1"][0], h["loads"], h["phi"][0], h["s"],
                                         h["beta0"], h["beta1"], h["inv_dt"], write_bands=h["write_bands"], sentinel=-7.0)
        assert tuple(out.shape) == (1, NE + 1) and _same(_np(out)[0], b), change
        assert _same(_np(a["adiag"]), adiag) and _same(_np(a["aoff"]), aoff), change
        assert h["write_bands"] or bool((a["adiag"] == -7.0).all())
    assert torch.equal(out, _run("ts_rhs", dev, U0=h["U0"], U1=h["U1"], phi=h["phi"])[1])


def test_valid_ts_error(dev):
    for change in ({}, dict(U0=None, w0=0.0), dict(U1=None, U0=None, w1=0.0, w0=0.0)):
        h = _host_inputs("ts_error")
        w = list(h["weights"])
        for k, i in (("w1", 2), ("w0", 3)):
            if k in change:
                w[i] = change[k]
        h.update({k: v for k, v in change.items() if k in h}, weights=tuple(w))
        out4 = _call("ts_error", _device(h, dev))
        want = ta.error_host(h["U3"], h["U2"], h["U1"], h["U0"], h["weights"], h["atol"], h["rtol"], h["end_kinds"])[1]
        assert _same(_np(out4), want) and want[3] == 0.0, change


def test_valid_nl_linearize(dev):
    for pm in (False, True):
        for change in ({}, dict(c_tab=None), dict(c_eff=False, f_eff=None, f_res=True)):
            h = dict(_host_inputs("nl_linearize"), **change)
            if pm:
                q, c, f = sr.layout(dict(q=h["q_tabs"], c=np.zeros((NE, N)) if h["c_tab"] is None else h["c_tab"],
                                         f=h["f_tab"]), True)
                h.update(point_major=True, q_tabs=q, f_tab=f, c_tab=None if h["c_tab"] is None else c)
            outs = _call("nl_linearize", _device(h, dev))
            asked = [bool(h[k]) for k in ("c_eff", "f_eff", "f_res")]
            want = sr.linearize_host(h["u"], h["t_local"], sr.POLY, h["q_tabs"], h["c_tab"], h["f_tab"], pm, asked)[1:]
            assert sorted(outs) == sorted(k for k, on in zip(("c_eff", "f_eff", "f_res"), asked) if on)
            for k, w in zip(("c_eff", "f_eff", "f_res"), want):
                assert w is None or _same(_np(outs[k]), w), (pm, change, k)


def test_valid_nl_residual(dev):
    for change in ({}, dict(end_kinds=(0, 0), end_values=None), dict(kappa=(0.0, -0.75))):
        h, out4 = _run("nl_residual", dev, **change)
        g = (0.0, 0.0) if h["end_values"] is None else h["end_values"]
        want = sr.residual_host(h["diag"], h["sub"], h["sup"], h["load"], h["u"], h["u_new"], h["end_kinds"], h["kappa"],
                                g)[1]
        assert _same(_np(out4), want) and want[3] == 0.0, change


def test_valid_nl_step(dev):
    h, out = _run("nl_step", dev)
    assert _same(_np(out), sr.step_host(h["u"], h["u_new"], h["lam"])[1])


def test_valid_ts_nl_assemble(dev):
    import torch
    for change in ({}, dict(a_quad=None)):
        h, res = _run("ts_nl_assemble", dev, **change)
        want = nr.assemble_host(h["x"], h["u"], h["a_quad"], h["cs_quad"], h["q_quad"], h["r"], sr.POLY)[1:]
        assert list(res) == ["diag", "off", "rhs"]
        for k, w in zip(res, want):
            assert _same(_np(res[k]), w), (change, k)
    a = _device(h, dev)
    out_dict()(a, dev)
    again = _call("ts_nl_assemble", a)
    assert all(again[k].data_ptr() == a["out"][k].data_ptr() and torch.equal(again[k], res[k]) for k in res)


def test_valid_wave_advance(dev):
    off = dict(mdiag=None, moff=None, ddiag=None, doff=None, loads=None, phi=None)
    for change in ({}, dict(ddiag=None, doff=None), dict(U_new=None), dict(rhs=False), dict(rhs=False, **off)):
        h, got = _run("wave_advance", dev, **change)
        rhs = h["rhs"]
        want = wr.advance_host(h["U_new"], h["U"], h["V"], h["Acc"], *(h[k] if rhs else None for k in off), h["dt"],
                               h["beta"], h["gamma"], rhs=rhs)[1:]
        for k, g, w in zip(("V_out", "Acc_out", "rhs_out"), got, want):
            wrote = (k == "rhs_out" and rhs) or (k != "rhs_out" and h["U_new"] is not None)
            assert (g is not None) == wrote, (change, k)
            assert g is None or _same(_np(g), w), (change, k)
