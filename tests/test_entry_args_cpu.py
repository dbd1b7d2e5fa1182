"""CPU: the refusals of the C entries behind the eigen, time, Newton and wave wrappers, one table over all of them.
Each row is the valid call of its entry with ONE argument changed, and holds the return code and a fragment of
``lssvr_last_error()``.  A device entry and its ``_host`` mirror get the same rows (the device entries validate before
they launch, so host addresses stand in); rows that an entry accepts (code 0: a legal NULL, an empty mesh) are run on
the host mirrors and on the device entries that return before a launch only.  The table runs in a child process that
sees no GPU, so a check that had moved behind a launch would fail there instead of reaching a device."""
import ctypes
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NE, NC, R, NB, N, NQUAD = 4, 2, 2, 2, 3, 2
BIG = (1 << 40) + 1
INF, NAN = math.inf, math.nan
P = "<array>"              # a pointer argument: an array of 128 doubles of its own


class Alias(str):
    """The address of another argument's array."""


class Off4(str):
    """The argument's own array, 4 bytes on: not aligned to a double."""


K_OK, K_NAN, K_NEG = "K_OK", "K_NAN", "K_NEG"          # kappa_host = (0.5, 0.25), (0.5, nan), (-0.5, -0.25)
SHORT = "SHORT"            # work_bytes: 8 bytes less than the entry's sizer asks for


def _args(spec):
    """'a b c=3' -> {a: P, b: P, c: 3}."""
    out = {}
    for tok in spec.split():
        k, _, v = tok.partition("=")
        out[k] = P if not v else (v if v.startswith("K_") else (float(v) if "." in v or "e" in v else int(v)))
    return out


_WS = " work work_bytes=1073741824 stream=0"
ARGS = {
    "eig_apply": _args("kdiag koff mdiag moff kind_left=0 kind_right=1 kappa=K_OK ne=4 nb=2 Z MZ KZ gram" + _WS),
    "eig_ritz": _args("A B nb=2 sigma=0.0 theta Q info stream=0"),
    "eig_ritz_host": _args("A B nb=2 sigma=0.0 theta Q info"),
    "eig_rotate": _args("Z MZ KZ Q theta kind_left=0 kind_right=1 ne=4 nb=2 X Y res2" + _WS),
    "eig_count": _args("kdiag koff mdiag moff kind_left=0 kind_right=1 kappa=K_OK ne=4 shifts ns=3 pivmin=1e-300 "
                       "counts stream=0"),
    "eig_rayleigh": _args("x W ne=4 M=9 nq=3 a_values c_values rho_values table_layout=0 kind_left=0 kind_right=1 "
                          "kappa=K_OK out3 work stream=0"),
    "ts_rhs": _args("mdiag moff U0 U1 loads phi ne=4 nc=2 R=2 beta0=2.0 beta1=-0.5 inv_dt=10.0 out"),
    "ts_source_table": _args("U2 U0 U1 ftab rho_tab phi ne=4 n_colloc=3 R=2 table_layout=0 alpha=1.5 beta0=2.0 "
                             "beta1=-0.5 inv_dt=10.0 out"),
    "ts_step": _args("kdiag koff mdiag moff U0 U1 loads phi ne=4 R=2 s=15.0 beta0=2.0 beta1=-0.5 inv_dt=10.0 "
                     "write_bands=1 adiag aoff b"),
    "ts_error": _args("U3 U2 U1 U0 kind_left=0 kind_right=1 ne=4 w3=1.0 w2=-3.0 w1=3.0 w0=-1.0 atol=1e-6 rtol=1e-3 "
                      "out4"),
    "nl_linearize": _args("u t_local q_tabs c_tab f_tab ne=4 n=3 table_layout=0 kind=0 nterm=2 c_eff f_eff f_res"),
    "nl_residual": _args("diag sub sup load u u_new kind_left=0 kind_right=1 end_values kappa=K_OK ne=4 out4"),
    "nl_step": _args("u u_new lam=0.5 ne=4 out"),
    "ts_nl_assemble": _args("x u a_quad cs_quad q_quad r ne=4 nquad=2 kind=0 nterm=2 diag off rhs"),
    "wave_advance": _args("U_new U V Acc mdiag moff ddiag doff loads phi ne=4 nc=2 R=2 dt=0.1 beta=0.25 gamma=0.5 "
                          "V_out Acc_out rhs_out"),
    "tridiag_bc_solve_multi": _args("diag off load kind_left=0 kind_right=1 end_values kappa=K_OK ne=4 nc=2 u" + _WS),
}
# (entry, its host mirror or None, what the device entry has after the shared arguments)
PAIRS = [("eig_apply", None, ""), ("eig_ritz", None, ""), ("eig_ritz_host", None, ""), ("eig_rotate", None, ""),
         ("eig_count", "eig_count_host", " stream=0"), ("eig_rayleigh", None, ""),
         ("ts_rhs", "ts_rhs_host", " stream=0"), ("ts_source_table", "ts_source_table_host", " stream=0"),
         ("ts_step", "ts_step_host", " stream=0"), ("ts_error", "ts_error_host", _WS),
         ("nl_linearize", "nl_linearize_host", " stream=0"), ("nl_residual", "nl_residual_host", _WS),
         ("nl_step", "nl_step_host", " stream=0"), ("ts_nl_assemble", "ts_nl_assemble_host", " stream=0"),
         ("wave_advance", "wave_advance_host", " stream=0"), ("tridiag_bc_solve_multi", None, "")]
SIZER = {"eig_apply": ("lssvr_eig_work_bytes", (NE, NB)), "eig_rotate": ("lssvr_eig_work_bytes", (NE, NB)),
         "ts_error": ("lssvr_ts_error_work_bytes", (NE,)), "nl_residual": ("lssvr_nl_residual_work_bytes", (NE,)),
         "tridiag_bc_solve_multi": ("lssvr_tridiag_bc_work_bytes", (NE, NC))}


def _each(names, code, frag, value=None):
    return [({nm: value}, code, frag) for nm in names.split()]


def _aliases(outs, ins, frag):
    return [({o: Alias(i)}, -2, frag) for o in outs.split() for i in ins.split()]


def _pairs(outs, frag):
    outs = outs.split()
    return [({a: Alias(b)}, -2, frag) for i, a in enumerate(outs) for b in outs[:i]]


def _range(name, lo, hi, code=-2):
    return [({name: v}, code, "%s = %d" % (name, v)) for v in (lo, hi)]


def _finite(names, frag="must be finite"):
    return [({nm: v}, -2, frag) for nm in names.split() for v in (INF, NAN)]


_NE = [({"ne": 0}, -2, "ne = 0 < 1"), ({"ne": BIG}, -2, "too large")]
_NE_EIG = [({"ne": -1}, -2, "ne = -1 < 0"), ({"ne": BIG}, -2, "too large"), ({"ne": 0}, 0, "")]
_KINDS = [({"kind_left": 2}, -2, "end kinds (2, 1) must be LSSVR_END_DIRICHLET or LSSVR_END_ROBIN"),
          ({"kind_right": -1}, -2, "end kinds (0, -1) must be LSSVR_END_DIRICHLET or LSSVR_END_ROBIN")]
_KAPPA = [({"kappa": None}, -1, "kappa_host must be non-NULL"), ({"kappa": K_NAN}, -2, "kappa[1] = nan must be finite")]
_LAYOUT = [({"table_layout": 2}, -2, "unknown table_layout 2"), ({"table_layout": -1}, -2, "unknown table_layout -1")]
_NL = [({"kind": 2}, -4, "unknown kind 2 (LSSVR_NL_POLY or LSSVR_NL_EXP)"), ({"kind": -1}, -4, "unknown kind -1"),
       ({"nterm": 0}, -2, "nterm = 0 outside [1, 6]"), ({"nterm": 7}, -2, "nterm = 7 outside [1, 6]"),
       ({"kind": 1, "nterm": 3}, -2, "nterm = 3: LSSVR_NL_EXP has q_0 and q_1"), ({"kind": 1, "nterm": 2}, 0, "")]
_EIG_BANDS = _NE_EIG + _each("kdiag koff mdiag moff", -1, "kdiag, koff, mdiag, moff must be non-NULL") + _KINDS + \
    _KAPPA + [({"kappa": K_NEG}, 0, "")]
_EIG_WORK = [({"work": None}, -1, "work must be non-NULL"),
             ({"work_bytes": SHORT}, -2, "bytes, lssvr_eig_work_bytes(4, 2) = ")]
_RITZ = _range("nb", 0, 9) + _each("A B theta Q", -1, "A, B, theta, Q must be non-NULL") + \
    _finite("sigma", "must be finite")
_TS_RHS = _NE + _range("R", 0, 9) + _finite("beta0 beta1 inv_dt") + [
    ({"U1": None}, -1, "U1 must be non-NULL when beta1 != 0"), ({"U1": None, "beta1": 0.0}, 0, "")]
_TS_RHS_NULL = "mdiag, moff, U0, loads, phi, out must be non-NULL"
_ALIGN = "every array must be aligned to 8 bytes"

ROWS = {
    "eig_apply": _EIG_BANDS + _range("nb", 0, 9) + _each("Z MZ KZ gram", -1, "Z, MZ, KZ, gram must be non-NULL") +
    _EIG_WORK,
    "eig_ritz": _RITZ,
    "eig_ritz_host": _RITZ,
    "eig_rotate": _NE_EIG + _range("nb", 0, 9) + _KINDS + _EIG_WORK +
    _each("Z MZ KZ Q theta X Y res2", -1, "Z, MZ, KZ, Q, theta, X, Y, res2 must be non-NULL"),
    "eig_count": _EIG_BANDS + [({"ns": -1}, -2, "ns = -1 < 0"), ({"ns": 0}, 0, "")] +
    _each("shifts counts", -1, "shifts and counts must be non-NULL") +
    [({"pivmin": v}, -2, "must be finite and > 0") for v in (0.0, -1.0, INF, NAN)],
    "eig_rayleigh": _NE_EIG + _range("M", 0, 34, -3) + _range("nq", 0, 33, -7) +
    _each("x W out3 work", -1, "x, W, out3, work must be non-NULL") +
    _each("a_values c_values rho_values", -1, "a_values, c_values and rho_values must be non-NULL") + _LAYOUT + _KINDS +
    _KAPPA,
    "ts_rhs": _TS_RHS + _range("nc", 0, 9) + _each("mdiag moff U0 loads phi out", -1, _TS_RHS_NULL) +
    _aliases("out", "U0 U1", "out must not be U0 or U1"),
    "ts_source_table": _NE + [({"n_colloc": v}, -2, "n_colloc = %d outside [2, 4096]" % v) for v in (1, 4097)] +
    _range("R", 0, 9) + _LAYOUT + _finite("alpha beta0 beta1 inv_dt") +
    _each("U2 U0 ftab rho_tab phi out", -1, "U2, U0, ftab, rho_tab, phi, out must be non-NULL") +
    [({"U1": None}, -1, "U1 must be non-NULL when beta1 != 0"), ({"U1": None, "beta1": 0.0}, 0, "")],
    "ts_step": _TS_RHS + _each("mdiag moff U0 loads phi b", -1, _TS_RHS_NULL) +
    _aliases("b", "U0 U1", "out must not be U0 or U1") + _finite("s", "must be finite") +
    [({"write_bands": 2}, -2, "write_bands = 2 must be 0 or 1"), ({"write_bands": -1}, -2, "write_bands = -1")] +
    _each("kdiag koff adiag aoff", -1, "kdiag, koff, adiag, aoff must be non-NULL with write_bands") +
    [({nm: Off4(nm)}, -2, _ALIGN) for nm in "kdiag koff mdiag moff U0 U1 loads phi adiag aoff b".split()] +
    _aliases("adiag aoff", "kdiag koff mdiag moff U0 U1 loads phi", "an output must not be one of the inputs") +
    _aliases("b", "kdiag koff mdiag moff loads phi", "an output must not be one of the inputs") +
    _pairs("adiag aoff b", "adiag, aoff, b must be distinct") +
    [({"write_bands": 0, "b": Alias(i)}, -2, "an output must not be one of the inputs")
     for i in "mdiag moff loads phi".split()] +
    [({"write_bands": 0, "kdiag": None, "koff": None, "adiag": None, "aoff": None}, 0, "")],
    "ts_error": _NE + _KINDS + _finite("w3 w2 w1 w0") + _finite("atol rtol", "must be finite and >= 0") +
    [({"atol": -1e-6}, -2, "must be finite and >= 0, their sum > 0"), ({"rtol": -1e-3}, -2, "their sum > 0"),
     ({"atol": 0.0, "rtol": 0.0}, -2, "atol = 0, rtol = 0 must be finite and >= 0, their sum > 0")] +
    _each("U3 U2 out4", -1, "U3, U2, out4 must be non-NULL") +
    [({"U1": None}, -1, "U1 must be non-NULL when w1 != 0"), ({"U0": None}, -1, "U0 must be non-NULL when w0 != 0"),
     ({"U1": None, "w1": 0.0}, 0, ""), ({"U0": None, "w0": 0.0}, 0, "")] +
    [({nm: Off4(nm)}, -2, _ALIGN) for nm in "U3 U2 U1 U0 out4".split()],
    "nl_linearize": _NE + _range("n", 0, 65) + _LAYOUT + _NL +
    _each("u t_local q_tabs f_tab", -1, "u, t_local, q_tabs, f_tab must be non-NULL") + [({"c_tab": None}, 0, "")] +
    [({"c_eff": None, "f_eff": None, "f_res": None}, -1, "one of c_eff, f_eff, f_res must be non-NULL"),
     ({"c_eff": None, "f_res": None}, 0, "")] +
    _aliases("c_eff f_eff f_res", "u t_local q_tabs c_tab f_tab", "an output must not be one of the inputs") +
    _pairs("c_eff f_eff f_res", "c_eff, f_eff, f_res must be distinct"),
    "nl_residual": _NE + _KINDS + _KAPPA + [({"kappa": K_NEG}, 0, "")] +
    _each("diag sub sup load u u_new out4", -1, "diag, sub, sup, load, u, u_new, out4 must be non-NULL") +
    [({"end_values": None}, -1, "end_values must be non-NULL with a Robin end"),
     ({"end_values": None, "kind_right": 0}, 0, "")],
    "nl_step": _NE + _finite("lam", "must be finite") + _each("u u_new out", -1, "u, u_new, out must be non-NULL") +
    _aliases("out", "u u_new", "out must not be u or u_new"),
    "ts_nl_assemble": _NE + [({"nquad": v}, -7, "nquad = %d outside [1,5]" % v) for v in (0, 6)] + _NL +
    _each("x u cs_quad q_quad r diag off rhs", -1, "x, u, cs_quad, q_quad, r, diag, off, rhs must be non-NULL") +
    [({"a_quad": None}, 0, "")] +
    _aliases("diag off rhs", "x u a_quad cs_quad q_quad r", "an output must not be one of the inputs") +
    _pairs("diag off rhs", "diag, off, rhs must be distinct"),
    "wave_advance": _NE + _range("nc", 0, 9) + _range("R", 0, 9) +
    [({nm: v}, -2, "must be finite and > 0") for nm in ("dt", "beta", "gamma") for v in (0.0, -0.1, INF, NAN)] +
    [({"U_new": None, "V_out": None, "Acc_out": None, "rhs_out": None}, -2, "there is nothing to compute")] +
    _each("U V Acc", -1, "U, V, Acc must be non-NULL") +
    _each("V_out Acc_out", -1, "V_out, Acc_out must be non-NULL with U_new") +
    _each("mdiag moff loads phi", -1, "mdiag, moff, loads, phi must be non-NULL with rhs_out") +
    [({"doff": None}, -1, "doff must be non-NULL with ddiag")] +
    _aliases("V_out Acc_out", "V Acc U U_new", "V_out, Acc_out must not be V, Acc, U or U_new (neighbours read") +
    [({"V_out": Alias("Acc_out")}, -2, "V_out and Acc_out must differ")] +
    _aliases("rhs_out", "U V Acc U_new loads", "rhs_out must not be U_new, U, V, Acc or loads") +
    _aliases("rhs_out", "V_out Acc_out", "rhs_out must not be V_out or Acc_out") +
    [({"ddiag": None, "doff": None}, 0, ""), ({"rhs_out": None}, 0, ""),
     ({"rhs_out": None, "mdiag": None, "moff": None, "ddiag": None, "doff": None, "loads": None, "phi": None}, 0, ""),
     ({"U_new": None, "V_out": None, "Acc_out": None}, 0, "")],
    # one entry of the other half, whose ends go through the same check with any_sign = false
    "tridiag_bc_solve_multi": _KINDS + _KAPPA + [({"kappa": K_NEG}, -2, "kappa[1] = -0.25 must be finite and >= 0"),
                                                 ({"work_bytes": SHORT}, -2, "lssvr_tridiag_bc_work_bytes(4, 2) = ")],
}
# the sized work of the two entries whose host mirror takes none
ROWS_DEVICE = {
    "ts_error": [({"work": None}, -1, "work must be non-NULL"), ({"work": Off4("work")}, -2, "work must be aligned"),
                 ({"work_bytes": SHORT}, -2, "lssvr_ts_error_work_bytes(4) = ")],
    "nl_residual": [({"work": None}, -1, "work must be non-NULL"),
                    ({"work_bytes": SHORT}, -2, "lssvr_nl_residual_work_bytes(4) = ")],
}
# device entries whose accepted rows return before a launch: the empty mesh, the empty list of shifts
NO_LAUNCH = [({"ne": 0}, 0, ""), ({"ns": 0}, 0, "")]


def table():
    """[(C name, the valid arguments, the override, code, fragment)] in a fixed order."""
    out = []
    for name, host, tail in PAIRS:
        dev_args = dict(ARGS[name], **_args(tail)) if host else ARGS[name]
        is_host = name.endswith("_host")
        for over, code, frag in [({}, 0, "")] * is_host + ROWS[name] + ROWS_DEVICE.get(name, []):
            if code == 0 and not is_host and (over, code, frag) not in NO_LAUNCH:
                continue
            out.append(("lssvr_" + name, dev_args, over, code, frag))
        if host:
            out += [("lssvr_" + host, ARGS[name], over, code, frag) for over, code, frag in [({}, 0, "")] + ROWS[name]]
    return out


def _run_table():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    kap = {K_OK: (0.5, 0.25), K_NAN: (0.5, NAN), K_NEG: (-0.5, -0.25)}
    dptr = ctypes.POINTER(ctypes.c_double)
    got = []
    for cname, args, over, _, _ in table():
        assert set(over) <= set(args), (cname, over)
        fn = getattr(lib, cname)
        keep = {k: (ctypes.c_double * 128)(*([1.0] * 128)) for k, v in args.items() if v == P}
        vals = []
        for (k, v), ctype in zip({**args, **over}.items(), fn.argtypes):
            if isinstance(v, Alias):
                v = ctypes.addressof(keep[v])
            elif isinstance(v, Off4):
                v = ctypes.addressof(keep[v]) + 4
            elif v == P:
                v = ctypes.addressof(keep[k])
            elif v in kap:
                v = ctypes.addressof(keep.setdefault("kappa values", (ctypes.c_double * 2)(*kap[v])))
            elif v == SHORT:
                sizer, sargs = SIZER[cname[len("lssvr_"):]]
                v = getattr(lib, sizer)(*sargs) - 8
            if ctype is dptr and isinstance(v, int):
                v = ctypes.cast(ctypes.c_void_p(v), dptr)
            vals.append(v)
        rc = fn(*vals)
        got.append((rc, lib.lssvr_last_error().decode() if rc else ""))
    return got


def test_every_single_mistake_is_refused_with_its_code_and_words():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="4096", ROCR_VISIBLE_DEVICES="4096")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--table"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = table()
    assert len(got) == len(want) and len(want) > 500
    bad = [(name, over, rc, msg, code, frag) for (rc, msg), (name, _, over, code, frag) in zip(got, want)
           if rc != code or frag not in msg]
    assert not bad, "\n".join(map(repr, bad))
    print(f"{len(want)} rows, {sum(1 for w in want if w[3] == 0)} of them accepted")


def test_every_entry_of_the_half_has_rows():
    from hybrid_fem_lssvr_amd import _capi
    names = {t[0] for t in table()}
    half = [n for n in _capi.SIGNATURES if n.split("_")[1] in ("eig", "ts", "nl", "wave") and "work_bytes" not in n]
    assert sorted(n for n in half if n not in names) == []


if __name__ == "__main__" and sys.argv[1:] == ["--table"]:
    print(json.dumps(_run_table()))
