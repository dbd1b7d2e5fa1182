"""CPU: the C-ABI library loads without a GPU and exports every symbol that
include/lssvr_hip.h declares; argument errors are reported before any HIP call."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssvr_hip.h")
BENCH_HEADER = os.path.join(ROOT, "include", "lssvr_hip_bench.h")      # measurement entries of the same library
MEASUREMENT_ONLY = ("lssvr_enhance_profiled", "lssvr_enhance_ws_sequence", "lssvr_enhance_varcoef_ws_sequence",
                    "lssvr_fp64_probe", "lssvr_stream_probe", "lssvr_row_chunk_probe")


def _uncommented(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared_in(path):
    return sorted(set(re.findall(r"\b(lssvr_[a-z0-9_]+)\s*\(", _uncommented(path))))


def _declared():
    return sorted(set(_declared_in(HEADER)) | set(_declared_in(BENCH_HEADER)))


def test_product_header_holds_no_measurement_entries():
    """Round-3 review: the product ABI header exported the measurement-only entries beside it.  They live in
    include/lssvr_hip_bench.h now (same library); the two headers are disjoint."""
    prod, bench = set(_declared_in(HEADER)), set(_declared_in(BENCH_HEADER))
    assert bench == set(MEASUREMENT_ONLY) and not (prod & bench)
    assert not any(("probe" in n or "profiled" in n or "sequence" in n) for n in prod)


def test_header_symbols_exported_and_bound():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    names = _declared()
    assert "lssvr_enhance" in names and "lssvr_eval" in names and len(names) >= 11
    for nm in names:
        assert hasattr(lib, nm), f"{nm} declared in the header but not exported"
        assert nm in _capi.SIGNATURES, f"{nm} has no ctypes signature"
    assert sorted(_capi.SIGNATURES) == names
    assert lib.lssvr_version() == _capi.ABI_VERSION
    hdr_ver = int(re.search(r"#define LSSVR_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert hdr_ver == _capi.ABI_VERSION


def _ctype_of(decl):
    """ctypes class of one C parameter declaration ("const double* rhs_params_host", "int M", ...)."""
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\**)\s*(\w+)", decl.strip())
    assert m, decl
    base, stars, name = m.groups()
    if stars == "**":
        assert base == "lssvr_step_plan", decl
        return ctypes.POINTER(ctypes.c_void_p)
    if stars == "*":
        if name.endswith("_host"):                      # read or written by the host: a typed pointer
            return ctypes.POINTER({"double": ctypes.c_double, "float": ctypes.c_float}[base])
        return ctypes.c_void_p                          # device pointers, plans and streams travel as integers
    return {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double}[base]


def test_signatures_match_header_prototypes():
    """Every prototype of the two headers against _capi.SIGNATURES: return type, arity and the ctypes class of
    each argument.  A wrong argtypes entry is silent stack corruption, and nothing else compares the two."""
    from hybrid_fem_lssvr_amd import _capi
    protos = {}
    for path in (HEADER, BENCH_HEADER):
        for ret, name, params in re.findall(r"^(int|int64_t|const char\*)\s+(lssvr_\w+)\s*\(([^)]*)\)\s*;",
                                            _uncommented(path), flags=re.M):
            assert name not in protos, name
            params = " ".join(params.split())
            protos[name] = (ret, [] if params == "void" else params.split(","))
    assert sorted(protos) == _declared() == sorted(_capi.SIGNATURES)
    restypes = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
    bad = []
    for name, (ret, params) in protos.items():
        res, argtypes = _capi.SIGNATURES[name]
        want = [_ctype_of(d) for d in params]
        if res is not restypes[ret] or len(argtypes) != len(want):
            bad.append((name, ret, len(params), len(argtypes)))
            continue
        bad += [(name, i, d.strip(), got) for i, (d, w, got) in enumerate(zip(params, want, argtypes)) if got is not w]
    assert not bad, "\n".join(map(repr, bad))


def test_header_constants_match_binding():
    from hybrid_fem_lssvr_amd import _capi
    txt = open(HEADER).read()
    for c_name, py_val in (("LSSVR_RHS_ARRAY", _capi.RHS_ARRAY), ("LSSVR_RHS_SIN", _capi.RHS_SIN),
                           ("LSSVR_SOLVER_PRIMAL", _capi.SOLVER_PRIMAL),
                           ("LSSVR_SOLVER_DUAL", _capi.SOLVER_DUAL),
                           ("LSSVR_SOLVER_PRIMAL_WAVE", _capi.SOLVER_PRIMAL_WAVE),
                           ("LSSVR_ST_OK", _capi.ST_OK), ("LSSVR_ST_FALLBACK", _capi.ST_FALLBACK)):
        m = re.search(r"#define %s\s+(\d+)" % c_name, txt)
        assert m and int(m.group(1)) == py_val, c_name


def test_argument_errors_without_gpu():
    """Validation happens on the host, before any launch: safe to call on a CPU-only box."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    p = _capi.rhs_params(1.0, 1.0)
    fake = ctypes.c_void_p(4096)
    rc = lib.lssvr_enhance(fake, fake, -1, 0, 0, 0.0, 1.0, 0.0, 0.0, 9, 16, 1e4, 1, p, None, 0,
                           fake, None, None, None)
    assert rc == -2 and b"ne" in lib.lssvr_last_error()
    rc = lib.lssvr_enhance(fake, fake, 10, 0, 10, 0.0, 1.0, 0.0, 0.0, 99, 16, 1e4, 1, p, None, 0,
                           fake, None, None, None)
    assert rc == -3 and b"M = 99" in lib.lssvr_last_error()
    rc = lib.lssvr_enhance(fake, fake, 10, 0, 10, 0.0, 1.0, 0.0, 0.0, 9, 16, 1e4, 7, p, None, 0,
                           fake, None, None, None)
    assert rc == -4
    rc = lib.lssvr_enhance(fake, fake, 10, 0, 10, 0.0, 1.0, 0.0, 0.0, 9, 16, 1e4, 0, None, None, 0,
                           fake, None, None, None)
    assert rc == -4 and b"rhs_values" in lib.lssvr_last_error()
    rc = lib.lssvr_enhance(None, fake, 10, 0, 10, 0.0, 1.0, 0.0, 0.0, 9, 16, 1e4, 1, p, None, 0,
                           fake, None, None, None)
    assert rc == -1
    rc = lib.lssvr_enhance(fake, fake, 10, 5, 12, 0.0, 1.0, 0.0, 0.0, 9, 16, 1e4, 1, p, None, 0,
                           fake, None, None, None)
    assert rc == -2 and b"shard" in lib.lssvr_last_error()
    rc = lib.lssvr_enhance(fake, fake, 10, 0, 10, 0.0, 1.0, 0.0, 0.0, 9, 16, 1e4, 1, p, None, 9,
                           fake, None, None, None)
    assert rc == -5
    # empty shard: success without touching the device
    rc = lib.lssvr_enhance(None, None, 0, 0, 0, 0.0, 1.0, 0.0, 0.0, 9, 16, 1e4, 1, p, None, 0,
                           None, None, None, None)
    assert rc == 0
    assert lib.lssvr_p1_assemble(fake, 10, 9, 1, p, None, None, fake, fake, fake, None, None, None) == -7
    assert lib.lssvr_eval(fake, fake, 0, 9, fake, 1, fake, None, None) == -2
    assert lib.lssvr_tridiag_work_bytes(100000) > 8 * 100000
    with pytest.raises(_capi.LssvrHipError):
        _capi.check(-3, "demo")


def test_ops_reject_host_tensors():
    import torch
    from hybrid_fem_lssvr_amd import ops
    x = torch.linspace(0, 1, 5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.enhance(x, x, 5, 1e4, 12, global_domain=(0.0, 1.0))
    with pytest.raises(TypeError):
        ops.enhance([0.0, 1.0], x, 5, 1e4, 12)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under the package may import it."""
    pkg = os.path.join(ROOT, "hybrid_fem_lssvr_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_enhance_work_bytes_is_host_arithmetic():
    """lssvr_enhance_work_bytes touches no device: the workspace of the kernel sequence above M = 22
    (96 doubles per element; 32 more where refinement steps follow: n_colloc - (M-2) <= 14), nothing
    for the lane kernel, the sequence on request for any M (LSSVR_SOLVER_PRIMAL_MOMENT)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    wb = lib.lssvr_enhance_work_bytes
    assert wb(1000, 33, 64, _capi.SOLVER_PRIMAL) == 1000 * 96 * 8            # BASELINE config 4's shape
    assert wb(1000, 33, 45, _capi.SOLVER_PRIMAL) == 1000 * 128 * 8           # excess 14: one refinement step
    assert wb(1000, 33, 46, _capi.SOLVER_PRIMAL) == 1000 * 96 * 8
    assert wb(1000, 23, 21, _capi.SOLVER_PRIMAL) == 1000 * 128 * 8
    assert wb(1000, 22, 40, _capi.SOLVER_PRIMAL) == 0                        # lane kernel: no workspace
    assert wb(1000, 9, 16, _capi.SOLVER_PRIMAL) == 0
    assert wb(1000, 9, 16, _capi.SOLVER_PRIMAL_MOMENT) == 1000 * 96 * 8
    assert wb(1000, 33, 64, _capi.SOLVER_DUAL) == 0 and wb(1000, 33, 64, _capi.SOLVER_PRIMAL_WAVE) == 0
    assert wb(0, 33, 64, _capi.SOLVER_PRIMAL) == 0


def test_step_plan_binds_and_validates_without_gpu():
    """lssvr_step_plan_create is host arithmetic (validation + a small host allocation, no HIP call): it runs here.
    Same checks as lssvr_step; a failed create leaves a NULL handle; destroy accepts NULL."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    rhs = _capi.rhs_params(9.869604401089358, 3.141592653589793)
    fake = [0x10000 * (i + 1) for i in range(8)]            # never dereferenced: the plan is not launched

    def create(ne=100, M=9, n=16, nquad=2, diag=fake[2]):
        h = ctypes.c_void_p()
        rc = lib.lssvr_step_plan_create(ctypes.byref(h), fake[0], fake[1], ne, 0, ne, -1.0, 1.0, 0.0, 0.0, M, n, 1e4,
                                        rhs, nquad, diag, fake[3], fake[4], fake[5], fake[6], None)
        return rc, h

    rc, h = create()
    assert rc == 0 and h.value
    assert lib.lssvr_step_plan_destroy(h) == 0
    for kw in ({"nquad": 9}, {"ne": 0}, {"M": 40}, {"n": 3}, {"diag": None}):
        rc, h = create(**kw)
        assert rc < 0 and not h.value, kw
        assert lib.lssvr_last_error().decode()
    assert lib.lssvr_step_plan_destroy(None) == 0
    assert lib.lssvr_step_plan_launch(None, None) < 0         # NULL plan: an argument error, no HIP call


# --- single-fault table: every enhancement entry, one broken rule at a time ------------------------------
# Each case starts from a valid argument set of fake (never dereferenced) device pointers and breaks ONE rule;
# the table holds failing cases only, never the valid baseline, so no case may reach a launch.  The table runs
# in a child process that sees no GPU: a check moved behind a launch fails there with a HIP error, on the host.
_F = [0x10000 * (i + 1) for i in range(12)]
_ENH = dict(x=_F[0], u=_F[1], ne=10, elem_offset=0, ne_global=10, gxmin=0.0, gxmax=1.0, bc_left=0.0, bc_right=0.0,
            M=9, n_colloc=16, gamma=1e4)
_RHS = dict(rhs_id=1, rhs_params="P", rhs_values=None)
_OUT = dict(W=_F[2], status=_F[3], fail_count=_F[4])
_VC = dict(a_values=_F[5], da_values=_F[6], rhs_values=_F[7])
_BANDS = dict(diag=_F[8], off=_F[9], load=_F[10])
_ARGS = {       # entry -> its arguments in declaration order with valid values ("P": rhs params, "MS": float[4])
    "lssvr_enhance": dict(**_ENH, **_RHS, solver_id=0, **_OUT, stream=None),
    "lssvr_enhance_ws": dict(**_ENH, **_RHS, solver_id=0, **_OUT, work=None, work_bytes=0, stream=None,
                             kernel_ms=None),
    "lssvr_enhance_ws_sequence": dict(**_ENH, **_RHS, solver_id=0, **_OUT, work=None, work_bytes=0, stream=None,
                                      repeats=4, kernel_ms="MS"),
    "lssvr_enhance_profiled": dict(**_ENH, **_RHS, solver_id=0, W=_F[2], status=_F[3], stream=None,
                                   kernel_ms="MS"),
    "lssvr_step": dict(**_ENH, rhs_params="P", nquad=2, **_BANDS, **_OUT, stream=None),
    "lssvr_step_plan_create": dict(plan="H", **_ENH, rhs_params="P", nquad=2, **_BANDS, **_OUT),
    "lssvr_enhance_varcoef": dict(**_ENH, **_VC, **_OUT, stream=None),
    "lssvr_enhance_varcoef_ws": dict(**_ENH, **_VC, table_layout=0, **_OUT, work=None, work_bytes=0, stream=None,
                                     kernel_ms=None),
    "lssvr_enhance_varcoef_ws_sequence": dict(**_ENH, **_VC, table_layout=0, **_OUT, work=None, work_bytes=0,
                                              stream=None, repeats=4, kernel_ms="MS"),
    "lssvr_step_varcoef": dict(**_ENH, **_VC, table_layout=0, nquad=2, rhs_quad=_F[11], a_quad=_F[11],
                               **_BANDS, **_OUT, stream=None),
    "lssvr_enhance_subset": dict(x=_F[0], u=_F[1], ne_mesh=10, elem_ids=_F[11], nsub=5, elem_offset=0,
                                 ne_global=10, gxmin=0.0, gxmax=1.0, bc_left=0.0, bc_right=0.0, M=9, n_colloc=16,
                                 gamma=1e4, gamma_values=None, **_RHS, W=_F[2], ldw=0, status=_F[3],
                                 fail_count=_F[4], stream=None),
    "lssvr_enhance_subset_ws": dict(x=_F[0], u=_F[1], ne_mesh=10, elem_ids=_F[11], nsub=5, elem_offset=0,
                                    ne_global=10, gxmin=0.0, gxmax=1.0, bc_left=0.0, bc_right=0.0, M=9,
                                    n_colloc=16, gamma=1e4, gamma_values=None, **_RHS, W=_F[2], ldw=0,
                                    status=_F[3], fail_count=_F[4], work=None, work_bytes=0, stream=None),
    "lssvr_enhance_shared": dict({k: v for k, v in _ENH.items() if k != "gamma"}, **_RHS, op=_F[5], **_OUT,
                                 stream=None, kernel_ms=None),
    "lssvr_p1_assemble": dict(x=_F[0], ne=10, nquad=2, rhs_id=1, rhs_params="P", rhs_quad=None, a_quad=None,
                              **_BANDS, kloc=None, floc=None, stream=None),
}
_BIG = dict(M=33, n_colloc=64)          # valid on its own; a workspace is then required to hold 96 doubles/element
_COMMON = [   # (overrides, rc, message substring) for the arguments every enhancement entry shares
    ({"ne": -1}, -2, "ne"), ({"ne": 11}, -2, "shard"), ({"elem_offset": -1}, -2, "shard"),
    ({"ne_global": 9}, -2, "shard"), ({"M": 99}, -3, "M = 99"), ({"M": 1}, -3, "M = 1"),
    ({"n_colloc": 1}, -2, "n_colloc"), ({"n_colloc": 5000}, -2, "n_colloc"), ({"x": None}, -1, "non-NULL"),
    ({"u": None}, -1, "non-NULL"), ({"W": None}, -1, "non-NULL"),
]
_GAMMA = [({"gamma": 0.0}, -2, "gamma"), ({"gamma": float("nan")}, -2, "gamma")]
_NAMED_RHS = [({"rhs_id": 7}, -4, "unknown rhs_id"), ({"rhs_id": -1}, -4, "unknown rhs_id"),
              ({"rhs_params": None}, -4, "rhs_params"), ({"rhs_id": 0}, -4, "rhs_values"),
              ({"rhs_id": 2}, -4, "rhs_values")]
_SOLVER = [({"solver_id": 9}, -5, "unknown solver_id"), ({"solver_id": -1}, -5, "unknown solver_id")]
_WORK = [({"work_bytes": -1}, -1, "work / work_bytes inconsistent"),
         ({"work_bytes": 8}, -1, "work / work_bytes inconsistent")]
_WORK_SMALL = [(dict(_BIG, work=_F[11], work_bytes=8), -2, "work holds")]
_SEQ = [({"kernel_ms": None}, -1, "kernel_ms_host"), ({"repeats": 0}, -2, "repeats"),
        ({"repeats": 100001}, -2, "repeats"), ({"ne": 0, "ne_global": 0}, -2, "ne")]
_TABLES = [({"a_values": None}, -1, "non-NULL"), ({"da_values": None}, -1, "non-NULL"),
           ({"rhs_values": None}, -1, "non-NULL"), ({"table_layout": 2}, -2, "unknown table_layout"),
           ({"table_layout": -1}, -2, "unknown table_layout")]
_STEP = [({"ne": 0, "ne_global": 0}, -2, "ne"), ({"rhs_params": None}, -4, "rhs_params"),
         ({"nquad": 0}, -7, "nquad"), ({"nquad": 6}, -7, "nquad"), ({"diag": None}, -1, "non-NULL"),
         ({"off": None}, -1, "non-NULL"), ({"load": None}, -1, "non-NULL"),
         ({"M": 20, "n_colloc": 16}, -5, "n_colloc")]
_STEP_VC = [({"ne": 0, "ne_global": 0}, -2, "ne"), ({"nquad": 0}, -7, "nquad"), ({"nquad": 6}, -7, "nquad"),
            ({"rhs_quad": None}, -1, "non-NULL"), ({"a_quad": None}, -1, "non-NULL"),
            ({"diag": None}, -1, "non-NULL"), ({"off": None}, -1, "non-NULL"), ({"load": None}, -1, "non-NULL"),
            ({"M": 20, "n_colloc": 16}, -5, "n_colloc")]
_SUBSET = [({"ne_mesh": -1}, -2, "ne_mesh"), ({"nsub": -1}, -2, "nsub"), ({"elem_ids": None}, -2, "nsub"),
           ({"nsub": 11}, -2, "nsub"), ({"ldw": 5}, -2, "ldw"), ({"ne_global": 9}, -2, "shard"),
           ({"elem_offset": -1}, -2, "shard"), ({"M": 99}, -3, "M = 99"), ({"M": 1}, -3, "M = 1"),
           ({"n_colloc": 1}, -2, "n_colloc"), ({"gamma": 0.0}, -2, "gamma"), ({"x": None}, -1, "non-NULL"),
           ({"u": None}, -1, "non-NULL"), ({"W": None}, -1, "non-NULL"), ({"M": 20, "n_colloc": 16}, -5, "n_colloc")]
_PROFILED = [({"kernel_ms": None}, -1, "kernel_ms_host"), ({"ne": 0, "ne_global": 0}, -2, "ne")]
FAULTS = {
    "lssvr_enhance": _COMMON + _GAMMA + _NAMED_RHS + _SOLVER,
    "lssvr_enhance_ws": _COMMON + _GAMMA + _NAMED_RHS + _SOLVER + _WORK + _WORK_SMALL,
    "lssvr_enhance_ws_sequence": _COMMON + _GAMMA + _NAMED_RHS + _SOLVER + _WORK + _WORK_SMALL + _SEQ,
    "lssvr_enhance_profiled": _COMMON + _GAMMA + _NAMED_RHS + _SOLVER + _PROFILED,
    "lssvr_step": _COMMON + _GAMMA + _STEP,
    "lssvr_step_plan_create": _COMMON + _GAMMA + _STEP + [({"plan": None}, -1, "plan")],
    "lssvr_enhance_varcoef": _COMMON + _GAMMA + _TABLES[:3],
    "lssvr_enhance_varcoef_ws": _COMMON + _GAMMA + _TABLES + _WORK,
    "lssvr_enhance_varcoef_ws_sequence": _COMMON + _GAMMA + _TABLES + _WORK + _SEQ,
    "lssvr_step_varcoef": _COMMON + _GAMMA + _TABLES + _STEP_VC,
    "lssvr_enhance_subset": _SUBSET + _NAMED_RHS,
    "lssvr_enhance_subset_ws": _SUBSET + _NAMED_RHS + _WORK + _WORK_SMALL,
    "lssvr_enhance_shared": _COMMON + _NAMED_RHS + [({"op": None}, -1, "op"), ({"M": 34}, -3, "M = 34")],
    "lssvr_p1_assemble": [({"ne": 0}, -2, "ne"), ({"ne": -1}, -2, "ne"), ({"x": None}, -1, "non-NULL"),
                          ({"diag": None}, -1, "non-NULL"), ({"off": None}, -1, "non-NULL"),
                          ({"load": None}, -1, "non-NULL"), ({"nquad": 0}, -7, "nquad"), ({"nquad": 6}, -7, "nquad"),
                          ({"rhs_id": 7}, -4, "unknown rhs_id"), ({"rhs_params": None}, -4, "rhs_params"),
                          ({"rhs_id": 0}, -4, "rhs_quad")],
}


def _run_fault_table():
    """Child side: call every case, return [(entry, overrides, rc, message)]."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    out = []
    for name, faults in FAULTS.items():
        for over, _, _ in faults:
            args = dict(_ARGS[name], **over)
            assert list(args) == list(_ARGS[name]), (name, over)      # overrides name existing arguments only
            handle = ctypes.c_void_p()
            conv = {"P": _capi.rhs_params(1.0, 1.0), "MS": (ctypes.c_float * 4)(), "H": ctypes.byref(handle)}
            vals = [conv[v] if isinstance(v, str) else v for v in args.values()]
            rc = getattr(lib, name)(*vals)
            assert not handle.value, (name, over)                      # a failed plan create leaves NULL
            out.append((name, over, rc, lib.lssvr_last_error().decode()))
    return out


def test_single_fault_table_without_gpu():
    """Every enhancement entry rejects each single broken rule with its own code and message, on the host:
    the table runs in a child process with no GPU visible."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="4096", ROCR_VISIBLE_DEVICES="4096")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--faults"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = [(name, over, rc, sub) for name, faults in FAULTS.items() for over, rc, sub in faults]
    assert len(got) == len(want) and len(want) > 200
    bad = [(n, o, rc, msg, w_rc, sub) for (n, o, rc, msg), (_, _, w_rc, sub) in zip(got, want)
           if rc != w_rc or sub not in msg]
    assert not bad, "\n".join(map(repr, bad))


if __name__ == "__main__" and sys.argv[1:] == ["--faults"]:
    sys.path.insert(0, ROOT)
    print(json.dumps(_run_fault_table()))
