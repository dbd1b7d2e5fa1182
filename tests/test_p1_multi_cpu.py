"""CPU: the P1 half of several load cases in the C ABI -- the four entries are declared, exported and bound, the
workspace size is host arithmetic, and every argument error is reported before any HIP call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssvr_hip.h")
ENTRIES = ("lssvr_p1_load_multi", "lssvr_tridiag_multi_work_bytes", "lssvr_tridiag_dirichlet_solve_multi",
           "lssvr_tridiag_ns_dirichlet_solve_multi")


def _lib():
    from hybrid_fem_lssvr_amd import _capi
    return _capi.load()


def test_entries_declared_exported_and_bound():
    from hybrid_fem_lssvr_amd import _capi
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib()
    for nm in ENTRIES:
        assert re.search(r"\b%s\s*\(" % nm, code), f"{nm} is not declared in include/lssvr_hip.h"
        assert hasattr(lib, nm), f"{nm} is not exported"
        assert nm in _capi.SIGNATURES, f"{nm} has no ctypes signature"
    assert lib.lssvr_version() == _capi.ABI_VERSION == 7            # additive: the ABI version stays


def test_multi_work_bytes_is_host_arithmetic():
    """One case needs what the single entry needs; the size never shrinks with more cases or more elements, stops
    growing at the cases of one pass (ops.TRIDIAG_MULTI_CASES, which this pins to the library's constant), and is
    finite and positive for one element."""
    from hybrid_fem_lssvr_amd import ops
    lib = _lib()
    wb, rc = lib.lssvr_tridiag_multi_work_bytes, ops.TRIDIAG_MULTI_CASES
    sizes = [1, 2, 3, 513, 514, 521, 4098, 4105, 33000, 1000000]
    for ne in sizes:
        assert wb(ne, 1) >= lib.lssvr_tridiag_work_bytes(ne) > 0
        per_nc = [wb(ne, nc) for nc in range(1, 2 * rc + 3)]
        assert all(a <= b for a, b in zip(per_nc, per_nc[1:])), ne
        assert per_nc[rc - 1] == per_nc[-1], ne                     # passes reuse the workspace
    for nc in (1, 2, rc, rc + 1):
        per_ne = [wb(ne, nc) for ne in sizes]
        assert all(a <= b for a, b in zip(per_ne, per_ne[1:])), nc
    assert 0 < wb(1, 1) < 1 << 20 and 0 < wb(1, 2 * rc + 1) < 1 << 20
    assert rc >= 2 and wb(1000000, rc - 1) < wb(1000000, rc)        # below one full pass it does grow


def test_argument_errors_without_gpu():
    """Fake, never dereferenced device pointers: one broken rule at a time, each with its code and message."""
    lib = _lib()
    F = [0x10000 * (i + 1) for i in range(8)]
    big = 1 << 40

    def load(x=F[0], ne=10, nquad=2, rhs=F[1], nc=3, out=F[2]):
        return lib.lssvr_p1_load_multi(x, ne, nquad, rhs, nc, out, None)

    def sym(diag=F[0], off=F[1], ld=F[2], ne=10, nc=3, bc=None, u=F[3], work=F[4], wb=big):
        return lib.lssvr_tridiag_dirichlet_solve_multi(diag, off, ld, ne, nc, bc, u, work, wb, None)

    def ns(diag=F[0], sub=F[1], sup=F[5], ld=F[2], ne=10, nc=3, bc=None, u=F[3], work=F[4], wb=big):
        return lib.lssvr_tridiag_ns_dirichlet_solve_multi(diag, sub, sup, ld, ne, nc, bc, u, work, wb, None)

    def err():
        return lib.lssvr_last_error().decode()

    for kw in (dict(x=None), dict(rhs=None), dict(out=None)):
        assert load(**kw) == -1 and "non-NULL" in err(), kw
    for kw, word in ((dict(ne=0), "ne"), (dict(ne=-1), "ne"), (dict(nc=0), "nc"), (dict(nc=-2), "nc")):
        assert load(**kw) == -2 and word in err(), kw
    for nq in (0, 6):
        assert load(nquad=nq) == -7 and "nquad" in err()
    for fn, bands in ((sym, ("diag", "off", "ld")), (ns, ("diag", "sub", "sup", "ld"))):
        for nm in bands + ("u", "work"):
            assert fn(**{nm: None}) == -1 and "non-NULL" in err(), (fn.__name__, nm)
        for kw, word in ((dict(ne=0), "ne"), (dict(nc=0), "nc")):
            assert fn(**kw) == -2 and word in err(), (fn.__name__, kw)
        need = lib.lssvr_tridiag_multi_work_bytes(10, 3)
        assert fn(wb=need - 1) == -2 and "work holds" in err() and "lssvr_tridiag_multi_work_bytes" in err()
        assert fn(wb=0) == -2 and fn(wb=-8) == -2
        # the order of the checks: ne, nc, NULL, work_bytes
        assert fn(ne=0, nc=0) == -2 and "ne = 0 < 1" in err()
        assert fn(nc=0, diag=None) == -2 and "nc = 0 < 1" in err()
        nulls = "diag, %s, load, u, work must be non-NULL" % ", ".join(bands[1:-1])
        assert fn(diag=None, wb=0) == -1 and nulls in err()
        assert fn(wb=need - 1) == -2 and "work holds %d bytes, lssvr_tridiag_multi_work_bytes(10, 3) = %d" % (
            need - 1, need) in err()

    # the single-RHS entries: the same checks, and no work_bytes to check
    def sym1(diag=F[0], off=F[1], ld=F[2], ne=10, u=F[3], work=F[4]):
        return lib.lssvr_tridiag_dirichlet_solve(diag, off, ld, ne, 0.0, 0.0, u, work, None)

    def ns1(diag=F[0], sub=F[1], sup=F[5], ld=F[2], ne=10, u=F[3], work=F[4]):
        return lib.lssvr_tridiag_ns_dirichlet_solve(diag, sub, sup, ld, ne, 0.0, 0.0, u, work, None)

    for fn, bands in ((sym1, ("diag", "off", "ld")), (ns1, ("diag", "sub", "sup", "ld"))):
        nulls = "diag, %s, load, u, work must be non-NULL" % ", ".join(bands[1:-1])
        for nm in bands + ("u", "work"):
            assert fn(**{nm: None}) == -1 and nulls in err(), nm
        for ne in (0, -1):
            assert fn(ne=ne) == -2 and "ne = %d < 1" % ne in err()
        assert fn(ne=0, diag=None) == -2
