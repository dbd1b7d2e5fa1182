"""What the bubble-condensed assembly tests share: the numpy prototype
(scripts/proto/bubble_proto.py), the meshes and tables of the cases, the host entry through ctypes, and the bars.

THE BARS.  A rounding bar is 10x what the float64 prototype itself reads on the same case against an np.longdouble
run of the same formulas (the project's rule), both relative to the largest entry of the
quantity.  The prototype's reading has a floor of one float64 eps of that scale: a reading below one unit of the last
place of the scale is chance (it is 0 on the smallest cases, where every sum has one term), and a value that is
rounded once already differs from the longdouble one by up to half of that.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "proto"))
import bubble_proto as proto      # noqa: E402

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
QUANTITIES = ("diag", "sub", "sup", "load", "kloc4", "floc")


def mesh(ne, seed=0):
    """h uniform in [0.5, 1.5], rescaled to [-1, 1] (as tests/test_gpu_conv.py)."""
    rng = np.random.default_rng(1000 * ne + seed)
    h = rng.uniform(0.5, 1.5, ne)
    return np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])


def tables(x, nquad, R, with_b=True, with_c=True, const_a=None):
    """(fq [R, ne, nquad], aq, cq, bq) at the quadrature points: a in [1, 1.6], c in [0.2, 1.4] (None without),
    b = amp * shape with amp = 0.4 / mean h and |shape| <= 1.3, so that with a >= 1 and h <= 1.5 mean h the cell
    Peclet number stays below 0.39 (None without)."""
    xq = proto.quad_points(x, nquad)
    ne = x.size - 1
    fq = np.stack([np.sin((2.0 + r) * xq + 0.3 * r) + 0.5 * r * xq for r in range(R)])
    aq = np.full_like(xq, const_a) if const_a is not None else 1.3 + 0.3 * np.sin(3.0 * xq + 0.2)
    cq = 0.8 + 0.6 * np.cos(2.0 * xq) if with_c else None
    bq = (0.4 * ne / 2.0) * (1.3 * np.sin(5.0 * xq + 1.0)) if with_b else None
    return np.ascontiguousarray(fq), aq, cq, bq


def _hd(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def host_assemble(x, order, nquad, fq, aq=None, cq=None, bq=None):
    """lssvr_p1_assemble_bubble_host on numpy arrays -> the dict of bubble_proto.assemble (float64)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    ne, R = x.size - 1, fq.shape[0]
    x, fq, aq, cq, bq = (None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in (x, fq, aq, cq, bq))
    out = dict(diag=np.zeros(ne + 1), sub=np.zeros(ne), sup=np.zeros(ne), load=np.zeros((R, ne + 1)),
               kloc4=np.zeros((ne, 4)), floc=np.zeros((R, ne, 2)))
    nbytes = lib.lssvr_p1_bubble_work_bytes(ne, R)
    assert nbytes == (4 + 2 * R) * ne * 8
    work = np.zeros(nbytes // 8)
    rc = lib.lssvr_p1_assemble_bubble_host(_hd(x), ne, order, nquad, R, _hd(fq), _hd(aq), _hd(cq), _hd(bq),
                                           *(_hd(out[k]) for k in QUANTITIES), work.ctypes.data, nbytes)
    _capi.check(rc, "lssvr_p1_assemble_bubble_host")
    return out


def reading(value, ref_ld, scale=None):
    """max |value - ref| / scale; scale: the largest |ref| unless given."""
    ref_ld = np.asarray(ref_ld, dtype=LD)
    scale = float(np.max(np.abs(ref_ld))) if scale is None else float(scale)
    if scale == 0.0:
        scale = 1.0
    return float(np.max(np.abs(np.asarray(value, dtype=LD) - ref_ld))) / scale


def rounding_bar(proto64, ref_ld, scale=None):
    """10x the float64 prototype's own reading against the longdouble run, with the floor of one eps (see above)."""
    return 10.0 * max(reading(proto64, ref_ld, scale), EPS)
