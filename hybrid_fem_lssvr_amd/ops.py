"""Device operators: thin, typed wrappers over the C ABI.

PyTorch-ROCm tensors are used as device buffers only (``data_ptr()`` + the
current HIP stream); all arithmetic happens in the hand-written gfx950 kernels
behind ``liblssvr_hip.so``.  Every function requires float64 CUDA tensors and
raises otherwise -- there is no CPU path.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import math
import os
import threading

import numpy as np
import torch

from . import _capi
from ._capi import (RHS_ARRAY, RHS_ARRAY_PM, RHS_SIN, SOLVER_DUAL, SOLVER_PRIMAL,  # noqa: F401
                    SOLVER_PRIMAL_MOMENT, SOLVER_PRIMAL_WAVE, TABLE_ELEMENT_MAJOR, TABLE_POINT_MAJOR)

SOLVER_SHARED = 100      # facade-level choice for UNIFORM meshes: routed to lssvr_enhance_shared

POISSON_AMP = float(math.pi ** 2)     # Dual.py:12  np.pi**2
POISSON_OMEGA = float(math.pi)


def _dev(t, name, dtype=torch.float64):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor device buffer, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: must live in MI355X device memory (got {t.device}); "
                           "the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _shard(x, u, elem_offset, ne_global):
    """(ne, ne_global) of the shard (x, u): float64[ne+1] device tensors of one length; ``ne_global``
    defaults to the shard's end."""
    _dev(x, "x")
    _dev(u, "u")
    if x.numel() != u.numel() or x.dim() != 1:
        raise ValueError("x and u must be 1-D with equal length ne+1")
    ne = x.numel() - 1
    return ne, (elem_offset + ne if ne_global is None else ne_global)


def _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma):
    """The twelve arguments every shard entry starts with (x, u, ne, elem_offset, ne_global, gxmin, gxmax, bc_left,
    bc_right, M, n_colloc, gamma); ``global_domain=None`` reads the shard's own ends back from the device."""
    ne = x.numel() - 1
    if global_domain is None:
        if ne == 0:
            global_domain = (0.0, 0.0)
        else:
            ends = torch.stack([x[0], x[-1]]).cpu()
            global_domain = (float(ends[0]), float(ends[1]))
    return (_ptr(x), _ptr(u), ne, int(elem_offset), int(ne_global), float(global_domain[0]), float(global_domain[1]),
            float(bc[0]), float(bc[1]), int(M), int(n_colloc), float(gamma))


def _layout(point_major):
    return TABLE_POINT_MAJOR if point_major else TABLE_ELEMENT_MAJOR


def _tables(ne, k, point_major=False, *, shape=False, **named):
    """Caller tables of ``k`` values per element become raw device pointers: each is a float64 device tensor of
    ne*k doubles or, with ``shape`` (the estimators), exactly [ne, k] / ``point_major`` [k, ne]."""
    want = (k, ne) if point_major else (ne, k)
    for nm, t in named.items():
        _dev(t, nm)
        if shape and tuple(t.shape) != want:
            raise ValueError(f"{nm} must be {'[nq, ne]' if point_major else '[ne, nq]'} = {list(want)}, "
                             f"got {list(t.shape)}")
        if t.numel() != ne * k:
            raise ValueError(f"{nm} must hold {ne * k} doubles, got {t.numel()}")


def _fold(da_values, b_values):
    """The first-derivative table of -(a u')' + b u' = -a u'' - (a' - b) u': ``da_values - b_values`` (one float64
    subtraction per entry; same shape and layout), or ``da_values`` itself without ``b_values``."""
    if b_values is None:
        return da_values
    _dev(da_values, "da_values")
    _dev(b_values, "b_values")
    if b_values.shape != da_values.shape or b_values.device != da_values.device:
        raise ValueError(f"b_values must have the shape and device of da_values {list(da_values.shape)}, "
                         f"got {list(b_values.shape)} on {b_values.device}")
    return da_values - b_values


def _variant(a_values, da_values, rhs_values, c_values):
    """("varcoef" | "react", the table pointers in that entry's order): the optional c table is all that
    separates ``lssvr_*_varcoef*`` from ``lssvr_*_react*``."""
    if c_values is None:
        return "varcoef", (_ptr(a_values), _ptr(da_values), _ptr(rhs_values))
    return "react", (_ptr(a_values), _ptr(da_values), _ptr(c_values), _ptr(rhs_values))


def _scratch(work, nbytes, device):
    """``work`` when it holds ``nbytes``, else a fresh buffer that does."""
    if work is None or work.numel() * work.element_size() < nbytes:
        work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
    return work


def _rhs(rhs, values, count, what, point_major=False, name="rhs_values"):
    """(rhs_id, params) of a right-hand side: ``rhs`` = (amp, omega) evaluated in-kernel, or the table
    ``values`` of ``count`` (= ``what``) doubles, element-major or ``point_major``."""
    if values is None:
        return RHS_SIN, _capi.rhs_params(*rhs)
    _dev(values, name)
    if values.numel() != count:
        raise ValueError(f"{name} must hold {what} = {count} doubles, got {values.numel()}")
    return (RHS_ARRAY_PM if point_major else RHS_ARRAY), None


def _bands(x, ne, bands=None, local=False, offdiag=("off",)):
    """P1 bands {diag[ne+1], off[ne], load[ne+1]} (+ kloc[ne], floc[ne, 2] with ``local``), allocated
    when not given; a caller's bands become raw device pointers, so they are checked.  ``offdiag``: the names of
    the off-diagonal bands, ("sub", "sup") for the non-symmetric assembly."""
    if not bands:
        shapes = {"diag": ne + 1, **{k: ne for k in offdiag}, "load": ne + 1}
        if local:
            shapes.update(kloc=ne, floc=(ne, 2))
        return {k: torch.empty(s, dtype=torch.float64, device=x.device) for k, s in shapes.items()}
    for k, cnt in (("diag", ne + 1), *((k, ne) for k in offdiag), ("load", ne + 1)):
        _dev(bands[k], k)
        if bands[k].numel() != cnt:
            raise ValueError(f"bands[{k!r}] must hold {cnt} doubles")
    return bands


def _timed(lib, name, args, repeats=None):
    """The ``profiled`` convention: ``name(*args, kernel_ms_host)`` BLOCKING -> the launch duration in
    seconds; ``repeats=k``: ``name_sequence(*args, k, kernel_ms_host)`` -> the list of k durations."""
    if repeats is not None:
        arr = (ctypes.c_float * int(repeats))()
        _capi.check(getattr(lib, name + "_sequence")(*args, int(repeats), arr), name + "_sequence")
        return [v * 1e-3 for v in arr]
    ms = ctypes.c_float(0.0)
    _capi.check(getattr(lib, name)(*args, ctypes.byref(ms)), name + "(profiled)")
    return ms.value * 1e-3


def _check_fail_count(fail_count):
    if fail_count is not None:
        _dev(fail_count, "fail_count", torch.int32)
        if fail_count.numel() < 1:
            raise ValueError("fail_count must hold one int32")


def _check_buffers(ne, M, n_colloc, x, *, out=None, status=None, fail_count=None):
    """Caller-supplied buffers become raw device pointers: a wrong-sized tensor would be an
    out-of-bounds device access, so sizes are checked here.  Returns (out, status), allocated
    when not given."""
    if out is None:
        out = torch.empty((ne, M), dtype=torch.float64, device=x.device)
    else:
        _dev(out, "out")
        if out.numel() != ne * M:
            raise ValueError(f"out must hold ne*M = {ne * M} doubles, got {out.numel()}")
    if status is None:
        status = torch.empty((ne,), dtype=torch.int32, device=x.device)
    else:
        _dev(status, "status", torch.int32)
        if status.numel() != ne:
            raise ValueError(f"status must hold ne = {ne} int32, got {status.numel()}")
    _check_fail_count(fail_count)
    return out, status


def _stream(stream):
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, torch.cuda.Stream):
        return stream.cuda_stream
    return int(stream)


_WORK = {}                     # device index -> {"buf", "event", "stream"}: ONE shared scratch buffer per device
_WORK_LOCK = threading.Lock()


def _torch_stream(handle, device):
    """torch view of a raw hipStream_t handle (0 = the device's default stream)."""
    if not handle:
        return torch.cuda.default_stream(device)
    return torch.cuda.ExternalStream(int(handle), device=device)


class workspace:
    """Context manager around ONE launch that needs the scratch of ``lssvr_enhance_ws``
    (``lssvr_enhance_work_bytes``; None inside the ``with`` when no workspace is needed).

    One buffer per DEVICE, grown on demand, shared by every stream: a launch on another stream than the previous
    user first waits (on the device, ``hipStreamWaitEvent``) for the event recorded after that user's launch, so
    launches above M = 22 that go through this default workspace are serialised ACROSS streams (pass your own
    ``work=`` buffers, as :class:`StepPlan` does, for concurrent streams).  Memory: 96-128 doubles per element of
    the largest launch so far (0.8-1 GB per 1e6 elements), once per device -- round 3 kept one such buffer per
    (device, stream handle) for the life of the process, and a destroyed-and-reused handle could alias another
    stream's buffer.  The lock is held from hand-out to the recorded event, so host threads cannot
    interleave between the two."""

    def __init__(self, lib, device, ne, M, n_colloc, solver, stream=None):
        self.nbytes = int(lib.lssvr_enhance_work_bytes(int(ne), int(M), int(n_colloc), int(solver)))
        self.device, self.handle, self.locked = device, _stream(stream), False

    def __enter__(self):
        if self.nbytes <= 0:
            return None
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _WORK_LOCK.acquire()
        self.locked = True
        ent = _WORK.get(idx)
        self.ts = _torch_stream(self.handle, self.device)
        if ent is not None and ent["event"] is not None and ent["stream"] != self.handle:
            self.ts.wait_event(ent["event"])            # the previous user's kernels are done before ours start
        if ent is None or ent["buf"].numel() * 8 < self.nbytes:
            # (a replaced buffer's last use is ordered before this stream's work by the wait above)
            if ent is not None:
                ent["buf"].record_stream(self.ts)
            ent = {"buf": torch.empty((self.nbytes + 7) // 8, dtype=torch.float64, device=self.device), "event": None}
            _WORK[idx] = ent
        ent["stream"] = self.handle
        self.ent = ent
        return ent["buf"]

    def __exit__(self, *exc):
        if self.locked:
            try:
                ev = torch.cuda.Event()
                ev.record(self.ts)
                self.ent["event"] = ev
            finally:
                self.locked = False
                _WORK_LOCK.release()
        return False


def release_workspaces():
    """Drop every cached workspace (one per device otherwise, for the life of the process).  The device is
    synchronised first: no stream handle that may have been destroyed meanwhile is touched."""
    with _WORK_LOCK:
        if _WORK:
            torch.cuda.synchronize()
        _WORK.clear()


def _work_arg(work, lib, x, ne, M, n_colloc, solver, stream):
    """(context manager yielding the workspace tensor or None) for the ``work=`` convention of the wrappers:
    None = the shared per-device buffer, False = no workspace, a tensor = the caller's own."""
    if work is None:
        return workspace(lib, x.device, ne, M, n_colloc, solver, stream)
    if work is False:
        return contextlib.nullcontext(None)
    _dev(work, "work")
    return contextlib.nullcontext(work)


def enhance(x, u, M, gamma, n_colloc=12, *, rhs=(POISSON_AMP, POISSON_OMEGA), rhs_values=None,
            elem_offset=0, ne_global=None, global_domain=None, bc=(0.0, 0.0),
            solver=SOLVER_PRIMAL, out=None, status=None, fail_count=None, stream=None, work=None,
            point_major=False):
    """``solve_lssvr_subproblems`` (Dual.py:139-169) for the shard (x, u).

    x, u: float64[ne+1] device tensors.  Returns (W float64[ne, M], status int32[ne]).
    ``rhs`` = (amp, omega) evaluates f = amp*sin(omega*x) in-kernel; ``rhs_values``
    float64[ne, n_colloc] (f tabulated at ``colloc_points``) overrides it;
    ``point_major=True``: ``rhs_values`` is float64[n_colloc, ne] instead (f tabulated at
    ``colloc_points(..., point_major=True)``) -- the layout the lane kernels (M <= 22) read at
    full HBM rate.
    ``work``: device scratch for the two-kernel path above M = 22 (default: the buffer
    :func:`workspace` keeps for this device AND stream; ``work=False`` runs the workspace-free
    kernels -- above M = 22 the single f64-MFMA kernel, about half the speed).  A caller-supplied
    ``work`` must not be shared by launches that can run concurrently.
    """
    lib = _capi.load()
    ne, ne_global = _shard(x, u, elem_offset, ne_global)
    if ne < 0:
        raise ValueError("need at least one node")
    pre = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma)
    out, status = _check_buffers(ne, M, n_colloc, x, out=out, status=status, fail_count=fail_count)
    rhs_id, params = _rhs(rhs, rhs_values, ne * n_colloc, "ne*n_colloc", point_major)
    with _work_arg(work, lib, x, ne, M, n_colloc, solver, stream) as wk:
        rc = lib.lssvr_enhance_ws(*pre, rhs_id, params, _ptr(rhs_values), int(solver),
                                  _ptr(out), _ptr(status), _ptr(fail_count),
                                  _ptr(wk), 0 if wk is None else wk.numel() * 8, _stream(stream), None)
    _capi.check(rc, "lssvr_enhance_ws")
    return out, status


def enhance_subset(x, u, M, gamma, n_colloc, W, *, elem_ids=None, gamma_values=None,
                   rhs=(POISSON_AMP, POISSON_OMEGA), rhs_values=None, elem_offset=0, ne_global=None,
                   global_domain, bc=(0.0, 0.0), status=None, fail_count=None, stream=None,
                   point_major=False, work=None):
    """``lssvr_enhance_subset_ws``: the elements ``elem_ids`` (int64 device tensor of mesh indices;
    None = all) of the shard (x, u) with one (M, n_colloc); per-element ``gamma_values``
    (float64[ne], indexed by mesh element) optional.  Rows go to ``W[id, :M]`` of the caller's
    float64[ne, ldw] array (ldw = W.shape[1] >= M; zero it first when ldw > M).  ``work``: as in
    :func:`enhance` (above M = 22 the group runs as the moment / solve kernel pair; ``False``: the
    single f64-MFMA kernel)."""
    lib = _capi.load()
    ne, ne_global = _shard(x, u, elem_offset, ne_global)
    _dev(W, "W")
    if W.dim() != 2 or W.shape[0] != ne or W.shape[1] < M or not W.is_contiguous():
        raise ValueError("W must be a contiguous float64[ne, ldw >= M] tensor")
    if elem_ids is not None:
        _dev(elem_ids, "elem_ids", torch.int64)
        nsub = elem_ids.numel()
    else:
        nsub = ne
    if gamma_values is not None:
        _dev(gamma_values, "gamma_values")
        if gamma_values.numel() != ne:
            raise ValueError("gamma_values must hold one value per mesh element")
    if status is not None:
        _dev(status, "status", torch.int32)
        if status.numel() != ne:
            raise ValueError("status is indexed by mesh element: int32[ne]")
    _check_fail_count(fail_count)
    # (rows indexed by position in elem_ids)
    rhs_id, params = _rhs(rhs, rhs_values, nsub * n_colloc, "nsub*n_colloc", point_major)
    pre = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma)
    with _work_arg(work, lib, x, nsub, M, n_colloc, SOLVER_PRIMAL, stream) as wk:
        # (the subset entry takes elem_ids and nsub after ne, gamma_values after gamma)
        rc = lib.lssvr_enhance_subset_ws(*pre[:3], _ptr(elem_ids), int(nsub), *pre[3:],
                                         _ptr(gamma_values), rhs_id, params, _ptr(rhs_values),
                                         _ptr(W), int(W.shape[1]), _ptr(status), _ptr(fail_count),
                                         _ptr(wk), 0 if wk is None else wk.numel() * 8, _stream(stream))
    _capi.check(rc, "lssvr_enhance_subset_ws")
    return W


def build_shared_operator(h, M, gamma, n_colloc, *, device="cuda:0", stream=None):
    """Response table of ONE canonical element of length ``h`` for :func:`enhance_shared`:
    float64[n_colloc + 2, M], built by the general per-element kernel (``lssvr_enhance``) on a
    (n_colloc + 2)-element auxiliary mesh of the same spacing centred on 0 -- unit right-hand
    sides for rows k < n, unit boundary values for the last two rows."""
    n = int(n_colloc)
    h = float(h)
    nel = n + 2
    nodes = (torch.arange(nel + 1, dtype=torch.float64) - 0.5 * nel) * h
    scl = 2.0 / float(nodes[1] - nodes[0])
    f = torch.zeros((nel, n), dtype=torch.float64)
    f[torch.arange(n), torch.arange(n)] = scl * scl          # f~ = f / scl^2 = e_k
    uu = torch.zeros(nel + 1, dtype=torch.float64)
    uu[n + 1] = 1.0                # element n: (g_l, g_r) = (0, 1); element n+1: (1, 0)
    x = nodes.to(device)
    W, st = enhance(x, uu.to(device), int(M), float(gamma), n, rhs_values=f.to(device),
                    elem_offset=1, ne_global=nel + 2, global_domain=(float(nodes[0]) - h, float(nodes[-1]) + h),
                    stream=stream)
    op = torch.empty((nel, M), dtype=torch.float64, device=device)
    op[:n] = W[:n]
    op[n] = W[n + 1]               # response to g_l
    op[n + 1] = W[n]               # response to g_r
    if int(st.sum().item()) != 0:
        raise _capi.LssvrHipError("build_shared_operator: the canonical element's factorisation broke down")
    return op


def enhance_shared(x, u, op, M, n_colloc, *, rhs=(POISSON_AMP, POISSON_OMEGA), rhs_values=None,
                   elem_offset=0, ne_global=None, global_domain, bc=(0.0, 0.0), out=None, status=None,
                   fail_count=None, stream=None, profiled=False, point_major=False):
    """``lssvr_enhance_shared`` (uniform meshes; the caller vouches for uniformity).  Returns
    (W, status), or the kernel duration in seconds when ``profiled``."""
    lib = _capi.load()
    ne, ne_global = _shard(x, u, elem_offset, ne_global)
    _dev(op, "op")
    if op.dim() != 2 or op.shape[0] != n_colloc + 2 or op.shape[1] != M or not op.is_contiguous():
        raise ValueError("op must be a contiguous float64[(n_colloc+2), M] tensor")
    out, status = _check_buffers(ne, M, n_colloc, x, out=out, status=status, fail_count=fail_count)
    rhs_id, params = _rhs(rhs, rhs_values, ne * n_colloc, "ne*n_colloc", point_major)
    # (no gamma: it is part of the operator)
    args = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, 1.0)[:-1] + (
        rhs_id, params, _ptr(rhs_values), _ptr(op), _ptr(out), _ptr(status), _ptr(fail_count), _stream(stream))
    if profiled:
        return _timed(lib, "lssvr_enhance_shared", args)
    _capi.check(lib.lssvr_enhance_shared(*args, None), "lssvr_enhance_shared")
    return out, status


def enhance_profiled(x, u, M, gamma, n_colloc=12, *, rhs=(POISSON_AMP, POISSON_OMEGA),
                     elem_offset=0, ne_global=None, global_domain, bc=(0.0, 0.0),
                     solver=SOLVER_PRIMAL, out=None, status=None, stream=None, work=None, repeats=None):
    """Same launch as :func:`enhance` but BLOCKING and stamped with the dispatch's own
    begin/end timestamps; returns the kernel duration in seconds (roofline measurement; on the
    two-kernel path above M = 22 the duration of the pair, gap included).  ``repeats=k``: k launches
    back to back, one synchronisation at the end (``lssvr_enhance_ws_sequence``): the list of the k
    durations inside a running sequence instead of one duration in isolation."""
    lib = _capi.load()
    ne, ne_global = _shard(x, u, elem_offset, ne_global)
    out, status = _check_buffers(ne, M, n_colloc, x, out=out, status=status)
    with _work_arg(work, lib, x, ne, M, n_colloc, solver, stream) as wk:
        args = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma) + (
            RHS_SIN, _capi.rhs_params(*rhs), None, int(solver), _ptr(out), _ptr(status), None,
            _ptr(wk), 0 if wk is None else wk.numel() * 8, _stream(stream))
        return _timed(lib, "lssvr_enhance_ws", args, repeats)


def _bind(lib, name, args):
    """(bound foreign function, arguments pre-converted to the ctypes of its signature): a plan is launched many
    times, and converting ~20 Python values per call is a third of the host's ~7 us per launch of an ~8 us step."""
    argtypes = _capi.SIGNATURES[name][1]
    ready = (ctypes.Array, ctypes._SimpleCData, ctypes._Pointer, type(ctypes.byref(ctypes.c_int())))
    conv = tuple(a if (a is None or isinstance(a, ready)) else tp(a) for tp, a in zip(argtypes, args))
    return getattr(lib, name), conv


# The step memo's switches, read ONCE at import: LSSVR_STEP_MEMO=0 makes ``StepPlan(memo=None)`` mean off (an A/B run
# of an unchanged caller); LSSVR_STEP_MEMO_MAX_BYTES replaces the size cap (measurement runs beyond it).
STEP_MEMO_DEFAULT = os.environ.get("LSSVR_STEP_MEMO", "1") != "0"
# Largest memo a plan allocates.  MEASURED at degree 8: the memo wins up to 1 250 001 elements
# (200.0 MB: -4 %; -7 % at 1e6, -23 % at 1e5) and loses at 1e7 (1.6 GB: +13 %, the step is issue-bound there and the
# memo triples its traffic); the cap sits just above the largest size measured to win.
STEP_MEMO_MAX_BYTES = int(os.environ.get("LSSVR_STEP_MEMO_MAX_BYTES", 208 << 20))


class StepPlan:
    """One step of the hot path (element-local P1 assembly + per-element enhancement of
    the same resident mesh shard) bound once, launched many times: the argument tuple of
    ``lssvr_step`` is built at construction so that a launch is a single ctypes call.

    ``memo`` (None: on unless ``LSSVR_STEP_MEMO=0``): keep the mesh-only results of the collocation loop in a
    buffer of the plan's (``lssvr_step_plan_memo_*``; at most ``STEP_MEMO_MAX_BYTES``, and only where the library
    has a memo for the plan -- otherwise the plan silently runs without).  Construction then enqueues one fill
    launch on the current stream and synchronises it.  Every launch checks the memo against the live ``x``, so
    rewriting ``x`` in place keeps the results right and only costs the gain; :meth:`refresh_memo` restores it."""

    def __init__(self, x, u, M, gamma, n_colloc=12, *, rhs=(POISSON_AMP, POISSON_OMEGA), nquad=2,
                 elem_offset=0, ne_global=None, global_domain, bc=(0.0, 0.0), bands=None,
                 out=None, status=None, fail_count=None, memo=None):
        self.lib = _capi.load()
        ne, ne_global = _shard(x, u, elem_offset, ne_global)
        self.bands = _bands(x, ne, bands)
        self.W, self.status = _check_buffers(ne, M, n_colloc, x, out=out, status=status,
                                             fail_count=fail_count)
        self.fail_count = fail_count
        # above M = 22 lssvr_step is assembly + the workspace-free enhancement kernel (two launches);
        # with a workspace the enhancement runs as the faster moment / solve pair: three launches
        # (a private buffer: plans may run concurrently on different streams)
        nb = int(self.lib.lssvr_enhance_work_bytes(ne, int(M), int(n_colloc), SOLVER_PRIMAL))
        self._work = torch.empty((nb + 7) // 8, dtype=torch.float64, device=x.device) if nb > 0 else None
        self._keep = (x, u, _capi.rhs_params(*rhs))
        pre = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma)
        bands = (_ptr(self.bands["diag"]), _ptr(self.bands["off"]), _ptr(self.bands["load"]))
        outs = (_ptr(self.W), _ptr(self.status), _ptr(fail_count))
        self._args = pre + (self._keep[2], int(nquad)) + bands + outs
        self._step, self._cargs = _bind(self.lib, "lssvr_step", self._args)
        # the library's own plan (lssvr_step_plan_*): the 20 arguments validated and bound once on the C side, a
        # launch is a two-argument call (host cost 4.4 -> ~2 us per launch; with the stream handle passed in, since
        # torch.cuda.current_stream() alone costs 3 us)
        self._handle = ctypes.c_void_p()
        create, cargs = _bind(self.lib, "lssvr_step_plan_create", (ctypes.byref(self._handle),) + self._args)
        rc = create(*cargs)
        if rc < 0:
            self._handle = None
            _capi.check(rc, "lssvr_step_plan_create")
        self._launch = self.lib.lssvr_step_plan_launch
        # the memo: a buffer of the plan's own, like the workspace above (the library allocates nothing)
        self._memo = None
        self.memo_bytes = 0
        if (STEP_MEMO_DEFAULT if memo is None else memo) and self._work is None:
            nb = int(self.lib.lssvr_step_plan_memo_bytes(self._handle))
            if 0 < nb <= STEP_MEMO_MAX_BYTES:
                self._memo = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
                self.memo_bytes = nb
                self.refresh_memo()
                torch.cuda.current_stream(x.device).synchronize()   # construction is no hot path; afterwards any stream

        if self._work is not None:
            self._asm_args = (_ptr(x), ne, int(nquad), RHS_SIN, self._keep[2], None, None) + bands + (None, None)
            self._enh_args = pre + (RHS_SIN, self._keep[2], None, SOLVER_PRIMAL) + outs + (
                _ptr(self._work), self._work.numel() * 8)

    def launch(self, stream=None):
        st = _stream(stream)
        if self._work is not None:
            rc = self.lib.lssvr_p1_assemble(*self._asm_args, st)
            if rc >= 0:
                rc = self.lib.lssvr_enhance_ws(*self._enh_args, st, None)
        else:
            rc = self._launch(self._handle, st)
        if rc < 0:
            _capi.check(rc, "lssvr_step")
        return self.W, self.status

    def refresh_memo(self, stream=None):
        """Fill the memo again from ``x`` as it is now (one launch on ``stream``; None: the current stream of x's
        device) -- after the mesh has been moved in place.  Not needed for correctness: launches validate the memo
        against ``x`` themselves and run the full step where it is stale.  Set-up, like construction: no launch
        of this plan may be in flight on ANOTHER stream, and later launches must be ordered after ``stream``.
        A plan without a memo does nothing."""
        if self._memo is None:
            return
        st = _stream(torch.cuda.current_stream(self._memo.device) if stream is None else stream)
        _capi.check(self.lib.lssvr_step_plan_memo_bind(self._handle, _ptr(self._memo), self.memo_bytes, st),
                    "lssvr_step_plan_memo_bind")

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                self.lib.lssvr_step_plan_destroy(h)
            except Exception:
                pass
            self._handle = None


def enhance_varcoef(x, u, M, gamma, n_colloc, a_values, da_values, rhs_values, *, elem_offset=0,
                    ne_global=None, global_domain=None, bc=(0.0, 0.0), out=None, status=None,
                    fail_count=None, stream=None, profiled=False, point_major=False, repeats=None,
                    c_values=None, b_values=None):
    """BASELINE config 5: rows -a (2/h)^2 L'' - a' (2/h) L' (no reference counterpart; the
    operator it generalises is Dual.py:43-44).  ``profiled``: BLOCKING, returns the launch
    duration in seconds (the dispatch's own begin / end stamps) instead of (W, status); with
    ``repeats=k`` the list of the durations of k launches back to back, one synchronisation at the end.
    ``point_major``: the three tables are float64[n_colloc, ne] (``t[k, e]``) instead of
    float64[ne, n_colloc] -- see :func:`colloc_points`; the fast layout for M <= 22.
    ``c_values`` (same shape as the other tables): the reaction rows of -(a u')' + c u = f
    (``lssvr_enhance_react_ws``: primal solve only, ``n_colloc >= M - 2``, no ``repeats``); ``None`` is the
    call without it.
    ``b_values`` (shape and layout of ``da_values``): the convection coefficient of -(a u')' + b u' (+ c u) = f;
    the kernels read ``da_values`` only as the coefficient of the first-derivative row, so they are handed
    ``da_values - b_values``; ``None`` is the call without it."""
    lib = _capi.load()
    ne, ne_global = _shard(x, u, elem_offset, ne_global)
    da_values = _fold(da_values, b_values)
    _tables(ne, n_colloc, a_values=a_values, da_values=da_values, rhs_values=rhs_values,
            **({} if c_values is None else {"c_values": c_values}))
    if c_values is not None and repeats is not None:
        raise ValueError("repeats is not available with c_values (lssvr_enhance_react_ws has no sequence form)")
    pre = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma)
    out, status = _check_buffers(ne, M, n_colloc, x, out=out, status=status, fail_count=fail_count)
    kind, tabs = _variant(a_values, da_values, rhs_values, c_values)
    name = f"lssvr_enhance_{kind}_ws"
    args = pre + tabs + (_layout(point_major), _ptr(out), _ptr(status), _ptr(fail_count), None, 0, _stream(stream))
    if profiled:
        return _timed(lib, name, args, repeats)
    _capi.check(getattr(lib, name)(*args, None), name)
    return out, status


def _elem_list(elem_ids, ne, x):
    """nsub of an element list: ``elem_ids`` a 1-D int64 device tensor on x's device with at most ne entries, or None
    for all ne elements in order."""
    if elem_ids is None:
        return ne
    _dev(elem_ids, "elem_ids", torch.int64)
    if elem_ids.dim() != 1 or elem_ids.numel() > ne:
        raise ValueError(f"elem_ids must be int64[nsub <= ne = {ne}], got {list(elem_ids.shape)}")
    if elem_ids.device != x.device:
        raise RuntimeError(f"elem_ids lives on {elem_ids.device}, x on {x.device}")
    return elem_ids.numel()


def enhance_varcoef_subset(x, u, M, gamma, n_colloc, W, a_values, da_values, rhs_values, *, elem_ids=None,
                           gamma_values=None, c_values=None, b_values=None, point_major=False, elem_offset=0,
                           ne_global=None, global_domain, bc=(0.0, 0.0), status=None, fail_count=None, stream=None):
    """``lssvr_enhance_react_subset``: :func:`enhance_varcoef` for the elements ``elem_ids`` (int64 device tensor of
    mesh indices; None = all) of the shard (x, u) with one (M, n_colloc) -- what :func:`enhance_subset` is to
    :func:`enhance`.  The tables hold nsub * n_colloc doubles, indexed by POSITION in ``elem_ids``: float64[nsub,
    n_colloc], or [n_colloc, nsub] with ``point_major`` (tabulate on :func:`colloc_points_subset`); ``c_values``
    and ``b_values`` as in :func:`enhance_varcoef`.  ``gamma_values`` (float64[ne]) and ``status`` (int32[ne]) are
    indexed by mesh element; rows go to ``W[id, :M]`` of the caller's float64[ne, ldw >= M] array (zero it first when
    ldw > M), rows that are not listed are not written.  Primal solve only (``n_colloc >= M - 2``)."""
    lib = _capi.load()
    M, n_colloc = int(M), int(n_colloc)
    ne, ne_global = _shard(x, u, elem_offset, ne_global)
    _dev(W, "W")
    if W.dim() != 2 or W.shape[0] != ne or W.shape[1] < M:
        raise ValueError("W must be a contiguous float64[ne, ldw >= M] tensor")
    nsub = _elem_list(elem_ids, ne, x)
    da_values = _fold(da_values, b_values)
    named = dict(a_values=a_values, da_values=da_values, rhs_values=rhs_values)
    if c_values is not None:
        named["c_values"] = c_values
    _tables(nsub, n_colloc, **named)
    if gamma_values is not None:
        _dev(gamma_values, "gamma_values")
        if gamma_values.numel() != ne:
            raise ValueError("gamma_values must hold one value per mesh element")
    if status is not None:
        _dev(status, "status", torch.int32)
        if status.numel() != ne:
            raise ValueError("status is indexed by mesh element: int32[ne]")
    _check_fail_count(fail_count)
    _same_device(x, u=u, W=W, gamma_values=gamma_values, status=status, fail_count=fail_count, **named)
    pre = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma)
    # (the subset entry takes elem_ids and nsub after ne, gamma_values after gamma; it has one table order: c third)
    rc = lib.lssvr_enhance_react_subset(*pre[:3], _ptr(elem_ids), int(nsub), *pre[3:], _ptr(gamma_values),
                                        _ptr(a_values), _ptr(da_values), _ptr(c_values), _ptr(rhs_values),
                                        _layout(point_major), _ptr(W), int(W.shape[1]), _ptr(status),
                                        _ptr(fail_count), _stream(stream))
    _capi.check(rc, "lssvr_enhance_react_subset")
    return W


def enhance_multi(x, U, M, gamma, n_colloc, a_values, da_values, rhs_values, *, c_values=None, bc=None,
                  point_major=False, elem_offset=0, ne_global=None, global_domain, out=None, status=None,
                  fail_count=None, stream=None, timed=False, b_values=None):
    """``ncases`` load cases on one mesh in one call (``lssvr_enhance_multi``): the element systems of
    ``-(a u')' + c u = f`` are formed and factored once per element, every case brings its own nodal values
    ``U[ncases, ne+1]``, right-hand side ``rhs_values[ncases, ne, n_colloc]`` (``point_major``:
    ``[ncases, n_colloc, ne]``, like the coefficient tables ``[n_colloc, ne]``) and Dirichlet pair
    ``bc[ncases, 2]`` (a float64 device tensor, or an array-like that is copied to the device; ``None``: zeros).
    ``c_values=None``: the variable-coefficient rows.  ``global_domain`` is required (no read-back of the shard's
    ends).  Returns (W float64[ncases, ne, M], status int32[ncases, ne]); ``fail_count`` counts (case, element)
    fallbacks; ``status=False`` passes NULL (no status written, None returned).  ``timed``: BLOCKING, returns the
    duration of all passes in seconds instead.  Primal solve only (``n_colloc >= M - 2``); M <= 16 is the
    one-factorisation lane kernel, above it the single-case kernel runs once per case.
    ``b_values`` (shape and layout of ``da_values``): the convection coefficient b of -(a u')' + b u' + c u = f, as in
    :func:`enhance_varcoef` -- the kernels are handed ``da_values - b_values``; ``None``: no such term."""
    lib = _capi.load()
    M, n_colloc = int(M), int(n_colloc)
    da_values = _fold(da_values, b_values)
    named = dict(x=x, U=U, a_values=a_values, da_values=da_values, rhs_values=rhs_values)
    if c_values is not None:
        named["c_values"] = c_values
    for nm, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{nm}: expected a torch.Tensor device buffer, got {type(t).__name__}")
    # shapes first (metadata only), then dtype / device / contiguity of every buffer
    if x.dim() != 1 or x.numel() < 1 or U.dim() != 2 or U.shape[1] != x.numel() or U.shape[0] < 1:
        raise ValueError(f"U must be [ncases, ne+1] = [>= 1, {x.numel()}] for x of {x.numel()} nodes, "
                         f"got {list(U.shape)}")
    ncases, ne = int(U.shape[0]), x.numel() - 1
    tab = (n_colloc, ne) if point_major else (ne, n_colloc)
    for nm in list(named)[2:]:
        want = (ncases,) + tab if nm == "rhs_values" else tab
        if tuple(named[nm].shape) != want:
            raise ValueError(f"{nm} must be {list(want)} ({'point' if point_major else 'element'}-major), "
                             f"got {list(named[nm].shape)}")
    for nm, t in named.items():
        _dev(t, nm)
    ne_global = elem_offset + ne if ne_global is None else ne_global
    if bc is not None:
        if not isinstance(bc, torch.Tensor):
            bc = torch.as_tensor(np.ascontiguousarray(np.asarray(bc, dtype=np.float64)), device=x.device)
        _dev(bc, "bc")
        if tuple(bc.shape) != (ncases, 2):
            raise ValueError(f"bc must be [ncases, 2] = [{ncases}, 2], got {list(bc.shape)}")
    for nm, t in (("U", U), ("a_values", a_values), ("da_values", da_values), ("rhs_values", rhs_values),
                  ("c_values", c_values), ("bc", bc), ("out", out), ("status", status), ("fail_count", fail_count)):
        if isinstance(t, torch.Tensor) and t.device != x.device:
            raise RuntimeError(f"{nm} lives on {t.device}, x on {x.device}")
    if out is None:
        out = torch.empty((ncases, ne, M), dtype=torch.float64, device=x.device)
    else:
        _dev(out, "out")
        if out.numel() != ncases * ne * M:
            raise ValueError(f"out must hold ncases*ne*M = {ncases * ne * M} doubles, got {out.numel()}")
    if status is None:
        status = torch.empty((ncases, ne), dtype=torch.int32, device=x.device)
    elif status is not False:
        _dev(status, "status", torch.int32)
        if status.numel() != ncases * ne:
            raise ValueError(f"status must hold ncases*ne = {ncases * ne} int32, got {status.numel()}")
    else:
        status = None                        # status=False: the entry's NULL (no status is written)
    _check_fail_count(fail_count)
    args = (_ptr(x), _ptr(U), ne, int(elem_offset), int(ne_global), float(global_domain[0]),
            float(global_domain[1]), _ptr(bc), ncases, M, n_colloc, float(gamma), _ptr(a_values), _ptr(da_values),
            _ptr(c_values), _ptr(rhs_values), _layout(point_major), _ptr(out), _ptr(status), _ptr(fail_count),
            _stream(stream))
    if timed:
        return _timed(lib, "lssvr_enhance_multi", args)
    _capi.check(lib.lssvr_enhance_multi(*args, None), "lssvr_enhance_multi")
    return out, status


class StepGraph:
    """``steps`` launches of a bound plan (:class:`StepPlan`, :class:`StepPlanVarcoef`) captured ONCE in a
    hipGraph and replayed: a loop of steps on fixed buffers without the host in it.  On the MI355X a replayed
    step of BASELINE config 2 takes 7.7-8.0 us against 8.7 us issued call by call (``bench.py``'s
    ``graph_replay``).  The plan's buffers (x, u, W, status, bands) are the graph's:
    write new nodal values into ``u`` in place (``u.copy_(...)``) and replay."""

    def __init__(self, plan, steps=1):
        self.plan = plan
        self.steps = int(steps)
        side = torch.cuda.Stream(device=plan.W.device)
        side.wait_stream(torch.cuda.current_stream(plan.W.device))
        with torch.cuda.stream(side):
            plan.launch()                               # warm-up outside the capture
        torch.cuda.current_stream(plan.W.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: other threads of the process (torch.distributed's watchdog polls events) may keep
        # calling the runtime while this thread captures
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            for _ in range(self.steps):
                plan.launch()

    def replay(self):
        """Enqueue the captured steps on the current stream; returns the plan's (W, status)."""
        self.graph.replay()
        return self.plan.W, self.plan.status


class StepPlanVarcoef:
    """One step of BASELINE config 5 (a-weighted P1 assembly from tabulated quadrature values +
    variable-coefficient enhancement from tabulated a, a', f) bound once, launched many times:
    ``lssvr_step_varcoef`` -- one launch for M <= 12."""

    def __init__(self, x, u, M, gamma, n_colloc, a_values, da_values, rhs_values, rhs_quad, a_quad, *,
                 nquad=2, point_major=False, elem_offset=0, ne_global=None, global_domain, bc=(0.0, 0.0),
                 bands=None, out=None, status=None, fail_count=None):
        self.lib = _capi.load()
        ne, ne_global = _shard(x, u, elem_offset, ne_global)
        _tables(ne, n_colloc, a_values=a_values, da_values=da_values, rhs_values=rhs_values)
        _tables(ne, nquad, rhs_quad=rhs_quad, a_quad=a_quad)
        self.bands = _bands(x, ne, bands)
        self.W, self.status = _check_buffers(ne, M, n_colloc, x, out=out, status=status, fail_count=fail_count)
        self._keep = (x, u, a_values, da_values, rhs_values, rhs_quad, a_quad, fail_count)
        self._args = _prefix(x, u, elem_offset, ne_global, global_domain, bc, M, n_colloc, gamma) + (
            _ptr(a_values), _ptr(da_values), _ptr(rhs_values), _layout(point_major), int(nquad),
            _ptr(rhs_quad), _ptr(a_quad),
            _ptr(self.bands["diag"]), _ptr(self.bands["off"]), _ptr(self.bands["load"]),
            _ptr(self.W), _ptr(self.status), _ptr(fail_count))
        self._step, self._cargs = _bind(self.lib, "lssvr_step_varcoef", self._args)

    def launch(self, stream=None):
        rc = self._step(*self._cargs, _stream(stream))
        if rc < 0:
            _capi.check(rc, "lssvr_step_varcoef")
        return self.W, self.status


def colloc_points(x, n_colloc, *, stream=None, point_major=False):
    """``np.linspace(x[e], x[e+1], n)`` for every element (Dual.py:40) -> float64[ne, n], or
    float64[n, ne] with ``point_major`` (the same values transposed: tabulate ``rhs_func`` / a / a'
    on it and pass the tables with ``point_major=True``)."""
    lib = _capi.load()
    _dev(x, "x")
    ne = x.numel() - 1
    name = "lssvr_colloc_points_pm" if point_major else "lssvr_colloc_points"
    xc = torch.empty((n_colloc, ne) if point_major else (ne, n_colloc), dtype=torch.float64, device=x.device)
    _capi.check(getattr(lib, name)(_ptr(x), ne, int(n_colloc), _ptr(xc), _stream(stream)), name)
    return xc


def colloc_points_subset(x, elem_ids, n_colloc, *, stream=None, point_major=False):
    """:func:`colloc_points` for the elements ``elem_ids`` (int64 device tensor of mesh indices; None = all) only, by
    position in the list (``lssvr_colloc_points_subset``) -> float64[nsub, n], or float64[n, nsub] with
    ``point_major``: bit for bit ``colloc_points(x, n)[elem_ids]``, without the whole-mesh table.  The row of an id
    outside the mesh is left unwritten."""
    lib = _capi.load()
    _dev(x, "x")
    n_colloc = int(n_colloc)
    if x.dim() != 1 or x.numel() < 1:
        raise ValueError("x must be float64[ne+1]")
    if n_colloc < 2:
        raise ValueError(f"n_colloc must be >= 2, got {n_colloc}")
    ne = x.numel() - 1
    nsub = _elem_list(elem_ids, ne, x)
    xc = torch.empty((n_colloc, nsub) if point_major else (nsub, n_colloc), dtype=torch.float64, device=x.device)
    rc = lib.lssvr_colloc_points_subset(_ptr(x), ne, _ptr(elem_ids), int(nsub), n_colloc, _layout(point_major),
                                        _ptr(xc), _stream(stream))
    _capi.check(rc, "lssvr_colloc_points_subset")
    return xc


def quad_points(x, nquad=2, *, stream=None):
    lib = _capi.load()
    _dev(x, "x")
    ne = x.numel() - 1
    xq = torch.empty((ne, nquad), dtype=torch.float64, device=x.device)
    _capi.check(lib.lssvr_quad_points(_ptr(x), ne, int(nquad), _ptr(xq), _stream(stream)),
                "lssvr_quad_points")
    return xq


def p1_assemble(x, nquad=2, *, rhs=(POISSON_AMP, POISSON_OMEGA), rhs_quad=None, a_quad=None,
                want_local=False, out=None, stream=None, c_quad=None, b_quad=None):
    """Element-local P1 stiffness/load and the assembled tridiagonal bands
    (Dual.py:117-128).  Returns dict(diag[ne+1], off[ne], load[ne+1][, kloc, floc]).
    ``c_quad`` float64[ne, nquad] (c at :func:`quad_points`): the consistent mass matrix of the reaction term
    joins ``diag`` and ``off`` (``lssvr_p1_assemble_react``); ``None`` is the call without it.
    ``b_quad`` float64[ne, nquad] (b at :func:`quad_points`): the convection term b u' joins the bands
    (``lssvr_p1_assemble_conv``) and makes them non-symmetric -- the dict then holds ``sub[ne]`` (the coefficient of
    u_i in row i+1) and ``sup[ne]`` (that of u_{i+1} in row i) instead of ``off``, for
    :func:`tridiag_ns_dirichlet_solve`; ``None`` is the call without it."""
    lib = _capi.load()
    _dev(x, "x")
    ne = x.numel() - 1
    offdiag = ("off",) if b_quad is None else ("sub", "sup")
    out = _bands(x, ne, out, want_local, offdiag)
    rhs_id, params = _rhs(rhs, rhs_quad, ne * nquad, "ne*nquad", name="rhs_quad")
    if a_quad is not None:
        _dev(a_quad, "a_quad")
    name, coefs = "lssvr_p1_assemble", (_ptr(a_quad),)
    if c_quad is not None:
        _tables(ne, nquad, c_quad=c_quad)
        name, coefs = "lssvr_p1_assemble_react", (_ptr(a_quad), _ptr(c_quad))
    if b_quad is not None:
        _tables(ne, nquad, b_quad=b_quad)
        name, coefs = "lssvr_p1_assemble_conv", (_ptr(a_quad), _ptr(c_quad), _ptr(b_quad))
    rc = getattr(lib, name)(_ptr(x), ne, int(nquad), rhs_id, params, _ptr(rhs_quad), *coefs,
                            _ptr(out["diag"]), *(_ptr(out[k]) for k in offdiag), _ptr(out["load"]),
                            _ptr(out.get("kloc")), _ptr(out.get("floc")), _stream(stream))
    _capi.check(rc, name)
    return out


END_DIRICHLET, END_ROBIN = _capi.END_DIRICHLET, _capi.END_ROBIN      # LSSVR_END_*: the kind of one end of the domain


def _end_kinds(end_kinds, kappa, any_sign=False):
    """((kind_left, kind_right), host double[2] kappa) of a call with free ends: kinds in {0, 1}, kappa finite and
    >= 0 (``ValueError`` otherwise; read at a Robin end only, but checked at both).  ``any_sign``: the pivoting solve
    takes a finite kappa of either sign."""
    try:
        kinds = tuple(end_kinds)
        kap = tuple(float(k) for k in kappa)
    except TypeError:
        raise TypeError("end_kinds and kappa must be pairs (left, right)") from None
    if len(kinds) != 2 or len(kap) != 2:
        raise ValueError("end_kinds and kappa must be pairs (left, right)")
    if any(isinstance(k, bool) or k not in (END_DIRICHLET, END_ROBIN) for k in kinds):
        raise ValueError(f"end_kinds must be END_DIRICHLET (0) or END_ROBIN (1), got {kinds!r}")
    if any_sign and not all(math.isfinite(k) for k in kap):
        raise ValueError(f"kappa must be finite, got {kap!r}")
    if not any_sign and not all(math.isfinite(k) and k >= 0.0 for k in kap):
        raise ValueError(f"kappa must be finite and >= 0, got {kap!r}")
    return (int(kinds[0]), int(kinds[1])), (ctypes.c_double * 2)(*kap)


# The tridiagonal solves: one row per family, and `_tridiag` behind all 14 public functions (a new
# family is a row here, a row of the library's table in capi.hip, and its public functions below).
#   entries      (symmetric, non-symmetric) ``*_multi`` entry; the single forms are its nc = 1 call ...
#   by_value     ... except the Dirichlet ones: (symmetric, non-symmetric) single entry that takes u0, u1 by value
#   sizer        the scratch of (ne, nc), named in the "work holds" message
#   min_ne       fewest elements, and the message below that
#   ends         how the end values reach the entry: "bc" a [nc, 2] device tensor (or None) after nc, named ``bc``;
#                "kinds" the same tensor, named ``end_values``, after the end kinds and before kappa; None: no ends
#   any_sign     "kinds": kappa of either sign
#   info         the entry takes the int32 singularity count
#   strict_work  the single form raises on a short ``work`` as the multi forms do (the others replace it).  Only the
#                pivoting solve does; nobody chose that difference, and levelling it is a change of behaviour.
_Tri = collections.namedtuple("_Tri", "entries by_value sizer min_ne too_few ends any_sign info strict_work")
_ONE_ELEMENT = "need at least one element"
_TRIDIAG = {
    "dirichlet": _Tri(("lssvr_tridiag_dirichlet_solve_multi", "lssvr_tridiag_ns_dirichlet_solve_multi"),
                      ("lssvr_tridiag_dirichlet_solve", "lssvr_tridiag_ns_dirichlet_solve"),
                      "lssvr_tridiag_multi_work_bytes", 1, _ONE_ELEMENT, "bc", False, False, False),
    "bc": _Tri(("lssvr_tridiag_bc_solve_multi", "lssvr_tridiag_ns_bc_solve_multi"), None,
               "lssvr_tridiag_bc_work_bytes", 1, _ONE_ELEMENT, "kinds", False, False, False),
    "pivot": _Tri((None, "lssvr_tridiag_pivot_solve_multi"), None,
                  "lssvr_tridiag_pivot_work_bytes", 1, _ONE_ELEMENT, "kinds", True, True, True),
    "periodic": _Tri(("lssvr_tridiag_periodic_solve_multi", "lssvr_tridiag_ns_periodic_solve_multi"), None,
                     "lssvr_tridiag_periodic_work_bytes", 2, "a periodic mesh needs at least two elements", None,
                     False, False, False),
}
# (the names of the bands, the message for bands of other lengths by [multi]) by [non-symmetric]
_TRI_BANDS = ((("diag", "off", "load"), ("band lengths must be ne+1, ne, ne+1",
                                         "band lengths must be ne+1, ne and load [nc, ne+1]")),
              (("diag", "sub", "sup", "load"), ("band lengths must be ne+1, ne, ne, ne+1 (diag, sub, sup, load)",
                                                "band lengths must be ne+1, ne, ne and load [nc, ne+1] (diag, sub, "
                                                "sup, load)")))


def _tridiag(family, multi, bands, out, work, stream, end_values=None, ends=None, return_info=False):
    """The entry of ``family`` (a row of ``_TRIDIAG``) on ``bands`` = (diag, off, load) or (diag, sub, sup, load) ->
    u[nc, ne+1] with ``multi`` (load [nc, ne+1], ``out`` may hold more than nc cases: the first nc are written and
    returned, a ``work`` that is given must be large enough), else u[ne+1] (load [ne+1], ``end_values`` a host pair).
    ``ends`` = (end_kinds, kappa) for the families with free ends; ``return_info``: the pair (u, info)."""
    row = _TRIDIAG[family]
    lib = _capi.load()
    ns = len(bands) == 4
    names, lengths = _TRI_BANDS[ns]
    for nm, t in zip(names, bands):
        _dev(t, nm)
    diag, load = bands[0], bands[-1]
    ne = bands[1].numel()
    # the single Dirichlet forms, the hot call of the facade: at 1e5 elements they are bound by the host, so they skip
    # what they can -- no bc tensor, no look at ``work`` beyond its size, no same-device loop (2.6 us) -- and they take
    # a load of any shape that holds ne+1 doubles
    by_value = row.by_value is not None and not multi
    if by_value:
        fits = load.numel() == ne + 1
    else:
        fits = load.dim() == (2 if multi else 1) and load.shape[-1] == ne + 1
    if diag.numel() != ne + 1 or bands[-2].numel() != ne or not fits:
        raise ValueError(lengths[multi])
    if ne < row.min_ne:
        raise ValueError(row.too_few)
    nc = int(load.shape[0]) if multi else 1
    if nc < 1:
        raise ValueError("need at least one case")
    if row.ends == "kinds":
        kinds, kap = _end_kinds(*ends, any_sign=row.any_sign)
    if out is None:
        out = torch.empty((nc, ne + 1) if multi else (ne + 1,), dtype=torch.float64, device=diag.device)
    else:
        _dev(out, "out")
        if multi and (out.dim() != 2 or out.shape[1] != ne + 1 or out.shape[0] < nc):
            raise ValueError(f"out must be [>= {nc}, ne+1 = {ne + 1}], got {list(out.shape)}")
        if not multi and out.numel() != ne + 1:
            raise ValueError(f"out must hold ne+1 = {ne + 1} doubles, got {out.numel()}")
    need = getattr(lib, row.sizer)(ne, nc)
    if work is not None and not by_value:
        _dev(work, "work")
        if (multi or row.strict_work) and work.numel() * work.element_size() < need:
            raise ValueError(f"work holds {work.numel() * work.element_size()} bytes, "
                             f"{row.sizer}({ne}, {nc}) = {need}")
    work = _scratch(work, need, diag.device)         # (the other single forms replace a work that is too small)
    if by_value:
        rc = getattr(lib, row.by_value[ns])(*map(_ptr, bands), ne, float(end_values[0]), float(end_values[1]),
                                            _ptr(out), _ptr(work), _stream(stream))
        _capi.check(rc, row.by_value[ns])
        return out
    ev, ev_name = end_values, "bc" if row.ends == "bc" else "end_values"
    if ev is not None:
        if not isinstance(ev, torch.Tensor):
            ev = np.asarray(ev, dtype=np.float64)
            ev = torch.as_tensor(np.ascontiguousarray(ev if multi else ev.reshape(-1, 2)), device=diag.device)
        _dev(ev, ev_name)
        if tuple(ev.shape) != (nc, 2):
            raise ValueError(f"{ev_name} must be [nc, 2] = [{nc}, 2], got {list(ev.shape)}")
    info = torch.zeros(1, dtype=torch.int32, device=diag.device) if return_info else None
    for nm, t in (*zip(names, bands), (ev_name, ev), ("out", out), ("work", work)):
        if t is not None and t.device != diag.device:
            raise RuntimeError(f"{nm} lives on {t.device}, diag on {diag.device}")
    args = (ne, nc, *((_ptr(ev),) if row.ends == "bc" else ()), _ptr(out), *((_ptr(info),) if row.info else ()),
            _ptr(work), work.numel() * work.element_size(), _stream(stream))
    if row.ends == "kinds":
        args = (*kinds, _ptr(ev), kap, *args)
    rc = getattr(lib, row.entries[ns])(*map(_ptr, bands), *args)
    _capi.check(rc, row.entries[ns])
    u = out[:nc] if multi else out.view(ne + 1)
    return (u, info) if return_info else u


def tridiag_dirichlet_solve(diag, off, load, u0=0.0, u1=0.0, *, out=None, work=None, stream=None):
    """``enforce`` + ``solve`` (Dual.py:129-130) on the assembled bands -> u[ne+1]."""
    return _tridiag("dirichlet", False, (diag, off, load), out, work, stream, (u0, u1))


def tridiag_ns_dirichlet_solve(diag, sub, sup, load, u0=0.0, u1=0.0, *, out=None, work=None, stream=None):
    """:func:`tridiag_dirichlet_solve` for bands that are not symmetric (``lssvr_tridiag_ns_dirichlet_solve``):
    row i is sub[i-1] u[i-1] + diag[i] u[i] + sup[i] u[i+1] = load[i] -> u[ne+1].  No pivoting: the rows must be
    diagonally dominant (cell Peclet number <= 1 and c >= 0 for the bands of ``p1_assemble(..., b_quad=...)``);
    :func:`tridiag_pivot_solve` pivots."""
    return _tridiag("dirichlet", False, (diag, sub, sup, load), out, work, stream, (u0, u1))


# cases per pass of the multi-RHS tridiagonal solve (kTriMultiCases of the library): lssvr_tridiag_multi_work_bytes
# grows with nc up to here
TRIDIAG_MULTI_CASES = 8


def tridiag_dirichlet_solve_multi(diag, off, load, bc=None, *, out=None, work=None, stream=None):
    """``load.shape[0]`` calls of :func:`tridiag_dirichlet_solve` on the same bands in one
    (``lssvr_tridiag_dirichlet_solve_multi``), bit-identical to them: load float64[nc, ne+1] -> u[nc, ne+1] with
    u[j, 0], u[j, ne] = bc[j] (a float64 device tensor [nc, 2], or an array-like that is copied to the device;
    ``None``: zeros).  The bands are read and the pivots computed once per pass of ``TRIDIAG_MULTI_CASES`` cases.
    ``out`` [>= nc, ne+1]: its first nc rows are written and returned; ``work``: at least
    ``lssvr_tridiag_multi_work_bytes(ne, nc)`` bytes (``ValueError`` otherwise)."""
    return _tridiag("dirichlet", True, (diag, off, load), out, work, stream, bc)


def tridiag_ns_dirichlet_solve_multi(diag, sub, sup, load, bc=None, *, out=None, work=None, stream=None):
    """:func:`tridiag_dirichlet_solve_multi` for the non-symmetric bands: ``load.shape[0]`` calls of
    :func:`tridiag_ns_dirichlet_solve` in one (``lssvr_tridiag_ns_dirichlet_solve_multi``), bit-identical to them."""
    return _tridiag("dirichlet", True, (diag, sub, sup, load), out, work, stream, bc)


def tridiag_bc_solve_multi(diag, off, load, end_kinds, kappa, end_values=None, *, out=None, work=None, stream=None):
    """:func:`tridiag_dirichlet_solve_multi` with a Dirichlet or a Robin condition at each end
    (``lssvr_tridiag_bc_solve_multi``).  ``end_kinds`` = (left, right), each ``END_DIRICHLET`` or ``END_ROBIN``;
    ``kappa`` = (left, right), finite and >= 0, read at a Robin end (Neumann: 0); ``end_values`` float64[nc, 2] (a
    device tensor, or an array-like that is copied to the device; ``None``: zeros): g of case j at a Robin end
    ``a du/dn + kappa u = g`` (outward normal), the value itself at a Dirichlet end.  kappa and g join the end row
    inside the kernels; ``diag``, ``off`` and ``load`` are left as they are.  Row j is bit-identical to the call with
    that case alone, and two Dirichlet ends give the bits of :func:`tridiag_dirichlet_solve_multi`.  ``work``: at
    least ``lssvr_tridiag_bc_work_bytes(ne, nc)`` bytes (``ValueError`` otherwise)."""
    return _tridiag("bc", True, (diag, off, load), out, work, stream, end_values, (end_kinds, kappa))


def tridiag_bc_solve(diag, off, load, end_kinds, kappa, end_values=(0.0, 0.0), *, out=None, work=None, stream=None):
    """One right-hand side of :func:`tridiag_bc_solve_multi` (the nc = 1 call of the same entry): load float64[ne+1],
    ``end_values`` a pair (left, right) -> u[ne+1]."""
    return _tridiag("bc", False, (diag, off, load), out, work, stream, end_values, (end_kinds, kappa))


def tridiag_ns_bc_solve_multi(diag, sub, sup, load, end_kinds, kappa, end_values=None, *, out=None, work=None,
                              stream=None):
    """:func:`tridiag_bc_solve_multi` for the non-symmetric bands (``lssvr_tridiag_ns_bc_solve_multi``); two Dirichlet
    ends give the bits of :func:`tridiag_ns_dirichlet_solve_multi`.  No pivoting: at a Robin end the row is dominant
    when kappa + b(x_end) n / 2 >= 0 (n = -1 left, +1 right)."""
    return _tridiag("bc", True, (diag, sub, sup, load), out, work, stream, end_values, (end_kinds, kappa))


def tridiag_ns_bc_solve(diag, sub, sup, load, end_kinds, kappa, end_values=(0.0, 0.0), *, out=None, work=None,
                        stream=None):
    """One right-hand side of :func:`tridiag_ns_bc_solve_multi` (the nc = 1 call of the same entry)."""
    return _tridiag("bc", False, (diag, sub, sup, load), out, work, stream, end_values, (end_kinds, kappa))


def tridiag_pivot_solve_multi(diag, sub, sup, load, end_kinds=(END_DIRICHLET, END_DIRICHLET), kappa=(0.0, 0.0),
                              end_values=None, *, out=None, work=None, stream=None, return_info=False):
    """:func:`tridiag_ns_bc_solve_multi` for tridiagonal matrices that are not diagonally dominant but well conditioned
    (``lssvr_tridiag_pivot_solve_multi``): a recursive partitioned solve with scaled partial
    pivoting at every level, so the rows need not be diagonally dominant -- negative or sign-changing reaction, cell
    Peclet number above 1 (the Galerkin solution, oscillations included), a Robin end with ``kappa`` of either sign.
    Symmetric bands: pass ``off`` for both ``sub`` and ``sup``.  Arguments as in :func:`tridiag_ns_bc_solve_multi`;
    row j is bit-identical to the call with that case alone; the bands and loads are left as they are.  ``work``: at
    least ``lssvr_tridiag_pivot_work_bytes(ne, nc)`` bytes.  ``return_info=True``: ``(u, info)`` with ``info`` an
    int32 device tensor [1], the number of pivots that were zero or not finite after the row choice -- nonzero means
    the matrix is singular and ``u`` is not a solution; zero says only that no such pivot was met."""
    return _tridiag("pivot", True, (diag, sub, sup, load), out, work, stream, end_values, (end_kinds, kappa),
                    return_info)


def tridiag_pivot_solve(diag, sub, sup, load, end_kinds=(END_DIRICHLET, END_DIRICHLET), kappa=(0.0, 0.0),
                        end_values=(0.0, 0.0), *, out=None, work=None, stream=None, return_info=False):
    """One right-hand side of :func:`tridiag_pivot_solve_multi` (the nc = 1 call of the same entry): load
    float64[ne+1], ``end_values`` a pair (left, right) -> u[ne+1]."""
    return _tridiag("pivot", False, (diag, sub, sup, load), out, work, stream, end_values, (end_kinds, kappa),
                    return_info)


def tridiag_periodic_solve_multi(diag, off, load, *, out=None, work=None, stream=None):
    """:func:`tridiag_dirichlet_solve_multi` with periodic ends (``lssvr_tridiag_periodic_solve_multi``): node ne is
    node 0, the rows 0 and ne of the bands are the two halves of the seam row
    (diag[0] + diag[ne]) s + off[0] u[1] + off[ne-1] u[ne-1] = load[0] + load[ne].  load float64[nc, ne+1] ->
    u[nc, ne+1] with u[j, 0] == u[j, ne] bit for bit; ne >= 2.  ``diag``, ``off`` and ``load`` are left as they are;
    row j is bit-identical to the call with that case alone.  The matrix must not be singular (a reaction term that
    is positive somewhere); no pivoting.  ``work``: at least ``lssvr_tridiag_periodic_work_bytes(ne, nc)`` bytes
    (``ValueError`` otherwise)."""
    return _tridiag("periodic", True, (diag, off, load), out, work, stream)


def tridiag_periodic_solve(diag, off, load, *, out=None, work=None, stream=None):
    """One right-hand side of :func:`tridiag_periodic_solve_multi` (the nc = 1 call of the same entry): load
    float64[ne+1] -> u[ne+1]."""
    return _tridiag("periodic", False, (diag, off, load), out, work, stream)


def tridiag_ns_periodic_solve_multi(diag, sub, sup, load, *, out=None, work=None, stream=None):
    """:func:`tridiag_periodic_solve_multi` for the non-symmetric bands (``lssvr_tridiag_ns_periodic_solve_multi``):
    the seam row is (diag[0] + diag[ne]) s + sup[0] u[1] + sub[ne-1] u[ne-1] = load[0] + load[ne]."""
    return _tridiag("periodic", True, (diag, sub, sup, load), out, work, stream)


def tridiag_ns_periodic_solve(diag, sub, sup, load, *, out=None, work=None, stream=None):
    """One right-hand side of :func:`tridiag_ns_periodic_solve_multi` (the nc = 1 call of the same entry)."""
    return _tridiag("periodic", False, (diag, sub, sup, load), out, work, stream)


def p1_load_multi(x, rhs_quad, nquad=2, *, out=None, stream=None):
    """The ``load`` of :func:`p1_assemble` for ``nc`` tabulated right-hand sides in one launch
    (``lssvr_p1_load_multi``): rhs_quad float64[nc, ne, nquad] (f at :func:`quad_points`, case by case) ->
    load[nc, ne+1], each row bit-identical to ``p1_assemble(x, nquad, rhs_quad=rhs_quad[j], ...)["load"]`` with or
    without ``a_quad`` / ``c_quad`` / ``b_quad``.  No matrix bands are written.  ``out`` [>= nc, ne+1]: its first nc
    rows are written and returned."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(rhs_quad, "rhs_quad")
    ne, nquad = x.numel() - 1, int(nquad)
    if x.dim() != 1 or ne < 1:
        raise ValueError("x must be 1-D with at least two nodes")
    if rhs_quad.dim() != 3 or tuple(rhs_quad.shape[1:]) != (ne, nquad) or rhs_quad.shape[0] < 1:
        raise ValueError(f"rhs_quad must be [nc >= 1, ne, nquad] = [nc, {ne}, {nquad}], got {list(rhs_quad.shape)}")
    nc = int(rhs_quad.shape[0])
    if out is None:
        out = torch.empty((nc, ne + 1), dtype=torch.float64, device=x.device)
    else:
        _dev(out, "out")
        if out.dim() != 2 or out.shape[1] != ne + 1 or out.shape[0] < nc:
            raise ValueError(f"out must be [>= {nc}, ne+1 = {ne + 1}], got {list(out.shape)}")
    for nm, t in (("rhs_quad", rhs_quad), ("out", out)):
        if t.device != x.device:
            raise RuntimeError(f"{nm} lives on {t.device}, x on {x.device}")
    rc = lib.lssvr_p1_load_multi(_ptr(x), ne, nquad, _ptr(rhs_quad), nc, _ptr(out), _stream(stream))
    _capi.check(rc, "lssvr_p1_load_multi")
    return out[:nc]


BUBBLE_ORDERS = (2, 3, 4)      # lssvr_p1_assemble_bubble: the degree of the condensed element space
BUBBLE_MAX_CASES = 8


def p1_assemble_bubble(x, order, nquad, rhs_quad, *, a_quad=None, c_quad=None, b_quad=None, want_local=False,
                       out=None, work=None, stream=None):
    """The bands of -(a u')' + b u' + c u = f with the hierarchic bubbles of degree 2 .. ``order`` (2, 3 or 4)
    condensed out of every element (``lssvr_p1_assemble_bubble``): tridiagonal on the nodes
    like those of :func:`p1_assemble`, with nodal values of order h^(2 order).  ``nquad`` in order+1 .. 5;
    ``rhs_quad`` float64[ne, nquad] or [R, ne, nquad] (R in 1 .. 8; f at :func:`quad_points`), ``a_quad``, ``c_quad``,
    ``b_quad`` float64[ne, nquad] or None (a = 1, c = 0, b = 0).  Returns dict(diag[ne+1], sub[ne], sup[ne], load) --
    always ``sub`` and ``sup``, never ``off`` -- with ``load`` [ne+1] or [R, ne+1] to match ``rhs_quad``, plus, with
    ``want_local``, kloc4[ne, 4] (the condensed element matrices S00, S01, S10, S11) and floc [ne, 2] or [R, ne, 2].
    ``out``: a dict of those buffers to write into; ``work``: scratch of ``lssvr_p1_bubble_work_bytes(ne, R)``."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(rhs_quad, "rhs_quad")
    ne, order, nquad = x.numel() - 1, int(order), int(nquad)
    if x.dim() != 1 or ne < 1:
        raise ValueError("x must be 1-D with at least two nodes")
    if order not in BUBBLE_ORDERS:
        raise ValueError(f"order must be one of {BUBBLE_ORDERS}, got {order} (order 1 is p1_assemble)")
    if not order + 1 <= nquad <= 5:
        raise ValueError(f"nquad must be in order+1 .. 5 = {order + 1} .. 5, got {nquad}")
    single = rhs_quad.dim() == 2
    if rhs_quad.dim() not in (2, 3) or tuple(rhs_quad.shape[-2:]) != (ne, nquad) or \
            not (single or 1 <= rhs_quad.shape[0] <= BUBBLE_MAX_CASES):
        raise ValueError(f"rhs_quad must be [ne, nquad] or [R, ne, nquad] = [1 .. {BUBBLE_MAX_CASES}, {ne}, {nquad}], "
                         f"got {list(rhs_quad.shape)}")
    R = 1 if single else int(rhs_quad.shape[0])
    _tables(ne, nquad, **{k: t for k, t in (("a_quad", a_quad), ("c_quad", c_quad), ("b_quad", b_quad))
                          if t is not None})
    lead = () if single else (R,)
    shapes = {"diag": (ne + 1,), "sub": (ne,), "sup": (ne,), "load": lead + (ne + 1,)}
    if want_local:
        shapes.update(kloc4=(ne, 4), floc=lead + (ne, 2))
    out = {k: _out(None if out is None else out.get(k), k, s, x) for k, s in shapes.items()}
    work = _sized_work(work, x, "lssvr_p1_bubble_work_bytes", ne, R)
    _same_device(x, rhs_quad=rhs_quad, a_quad=a_quad, c_quad=c_quad, b_quad=b_quad)
    rc = lib.lssvr_p1_assemble_bubble(_ptr(x), ne, order, nquad, R, _ptr(rhs_quad), _ptr(a_quad), _ptr(c_quad),
                                      _ptr(b_quad), _ptr(out["diag"]), _ptr(out["sub"]), _ptr(out["sup"]),
                                      _ptr(out["load"]), _ptr(out.get("kloc4")), _ptr(out.get("floc")), _ptr(work),
                                      work.numel() * work.element_size(), _stream(stream))
    _capi.check(rc, "lssvr_p1_assemble_bubble")
    return out


def band_dominance(diag, sub, sup, free=(False, False), kappa=(0.0, 0.0), periodic=False):
    """The hypothesis of the unpivoted tridiagonal solves, checked on the device with ONE read-back: every band
    entry finite and every row of the system dominant, |sub[i-1]| + |sup[i]| <= diag[i].  Rows 0 and ne belong to
    the system only at a ``free`` (Neumann or Robin) end, where the missing neighbour is left out and ``kappa`` joins
    the diagonal, or with ``periodic``, where the two are one row, the seam's.  Returns (finite, worst row, its margin
    diag - |sub| - |sup|): the row with the smallest margin, dominant when the margin is >= 0 (a margin that is not
    finite counts as -inf).  Plain tensor arithmetic on 3 ne doubles before a solve, not a hot path."""
    for nm, t in (("diag", diag), ("sub", sub), ("sup", sup)):
        _dev(t, nm)
    ne = sub.numel()
    if diag.numel() != ne + 1 or sup.numel() != ne or ne < 1:
        raise ValueError("band lengths must be ne+1, ne, ne (diag, sub, sup)")
    d = diag.clone()
    d[1:] -= sub.abs()
    d[:-1] -= sup.abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, -math.inf))
    if periodic:
        seam = d[0] + d[ne]
        d[0], d[ne] = seam, seam
    else:
        for i, f, k in ((0, free[0], kappa[0]), (ne, free[1], kappa[1])):
            if f:
                d[i] += float(k)
            else:
                d[i] = math.inf
    finite = torch.isfinite(diag).all() & torch.isfinite(sub).all() & torch.isfinite(sup).all()
    margin, row = torch.min(d, dim=0)
    got = torch.stack([finite.to(torch.float64), row.to(torch.float64), margin]).cpu()
    return bool(got[0]), int(got[1]), float(got[2])


def p1_flux_solve(kloc, load, u0=0.0, u1=0.0, *, out=None, work=None, stream=None):
    """``enforce`` + ``solve`` (Dual.py:129-130) for the assembled P1 system through the
    element-flux prefix scan (A = D^T K D); kloc[ne], load[ne+1] from :func:`p1_assemble`."""
    lib = _capi.load()
    _dev(kloc, "kloc")
    _dev(load, "load")
    ne = kloc.numel()
    if load.numel() != ne + 1:
        raise ValueError("load must have ne+1 entries")
    if out is None:
        out = torch.empty(ne + 1, dtype=torch.float64, device=kloc.device)
    work = _scratch(work, lib.lssvr_p1_flux_work_bytes(ne), kloc.device)
    rc = lib.lssvr_p1_flux_solve(_ptr(kloc), _ptr(load), ne, float(u0), float(u1), _ptr(out),
                                 _ptr(work), _stream(stream))
    _capi.check(rc, "lssvr_p1_flux_solve")
    return out


def p1_flux_aggregate(kloc, load, *, first_global, work=None, stream=None):
    """Shard summary of the flux scan: returns (agg3 device double[3], work) -- see
    ``lssvr_p1_flux_aggregate``; ``work`` must be passed on to :func:`p1_flux_finish`."""
    lib = _capi.load()
    _dev(kloc, "kloc")
    _dev(load, "load")
    ne = kloc.numel()
    if load.numel() < ne + 1:
        raise ValueError("load must have at least ne+1 entries")
    work = _scratch(work, lib.lssvr_p1_flux_work_bytes(ne), kloc.device)
    agg = torch.empty(3, dtype=torch.float64, device=kloc.device)
    rc = lib.lssvr_p1_flux_aggregate(_ptr(kloc), _ptr(load), ne, int(bool(first_global)), _ptr(work),
                                     _ptr(agg), _stream(stream))
    _capi.check(rc, "lssvr_p1_flux_aggregate")
    return agg, work


def p1_flux_finish(kloc, load, work, *, first_global, last_global, prefix=None, grand=None,
                   u0=0.0, u1=0.0, out=None, stream=None):
    """Second half of the sharded flux solve: nodal values u[ne+1] of this shard.  ``work`` is the buffer
    :func:`p1_flux_aggregate` returned for the same ``kloc`` and ``load``; it becomes a raw device pointer that the
    kernel reads ``lssvr_p1_flux_work_bytes(ne)`` bytes of, so it is checked here and never replaced."""
    lib = _capi.load()
    _dev(kloc, "kloc")
    _dev(load, "load")
    _dev(work, "work")
    ne = kloc.numel()
    if ne < 1:
        raise ValueError("kloc must hold at least one element")
    if load.numel() < ne + 1:
        raise ValueError("load must have at least ne+1 entries")
    nbytes = lib.lssvr_p1_flux_work_bytes(ne)
    if work.numel() * work.element_size() < nbytes:
        raise ValueError(f"work must hold lssvr_p1_flux_work_bytes({ne}) = {nbytes} bytes, got "
                         f"{work.numel() * work.element_size()}")
    if out is None:
        out = torch.empty(ne + 1, dtype=torch.float64, device=kloc.device)
    else:
        _dev(out, "out")
        if out.numel() < ne + 1:
            raise ValueError("out must have at least ne+1 entries")
    for t, nm in ((prefix, "prefix"), (grand, "grand")):
        if t is not None:
            _dev(t, nm)
            if t.numel() < 3:
                raise ValueError(f"{nm} must hold 3 doubles")
    for nm, t in (("load", load), ("work", work), ("out", out), ("prefix", prefix), ("grand", grand)):
        if t is not None and t.device != kloc.device:
            raise RuntimeError(f"{nm} lives on {t.device}, kloc on {kloc.device}")
    rc = lib.lssvr_p1_flux_finish(_ptr(kloc), _ptr(load), ne, int(bool(first_global)),
                                  int(bool(last_global)), _ptr(work), _ptr(prefix), _ptr(grand),
                                  float(u0), float(u1), _ptr(out), _stream(stream))
    _capi.check(rc, "lssvr_p1_flux_finish")
    return out


def evaluate(x, W, xq, *, want_elem=True, out=None, stream=None, deriv=0):
    """``evaluate_solution`` (Dual.py:176-203) -> (u float64[P], elem int64[P] | None).
    ``out``: optional preallocated float64[P] for u.  ``deriv`` = 1 or 2: the first / second
    x-derivative of the enhanced solution instead (``lssvr_eval_deriv``; same element rule)."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    _dev(xq, "xq")
    ne = x.numel() - 1
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, M]")
    if deriv not in (0, 1, 2):
        raise ValueError(f"deriv must be 0, 1 or 2, got {deriv!r}")
    M = W.shape[1]
    P = xq.numel()
    if out is None:
        uq = torch.empty(P, dtype=torch.float64, device=x.device)
    else:
        uq = _dev(out, "out")
        if uq.numel() != P or not uq.is_contiguous():
            raise ValueError("out must be a contiguous float64[P] tensor")
    elem = torch.empty(P, dtype=torch.int64, device=x.device) if want_elem else None
    if deriv == 0:
        rc = lib.lssvr_eval(_ptr(x), _ptr(W), ne, int(M), _ptr(xq), P, _ptr(uq), _ptr(elem),
                            _stream(stream))
        _capi.check(rc, "lssvr_eval")
    else:
        rc = lib.lssvr_eval_deriv(_ptr(x), _ptr(W), ne, int(M), int(deriv), _ptr(xq), P, _ptr(uq),
                                  _ptr(elem), _stream(stream))
        _capi.check(rc, "lssvr_eval_deriv")
    return uq, elem


def eval_error(x, W, xq, *, exact=(1.0, math.pi), out=None, stream=None):
    """Device-side error norms of the hybrid solution vs exact(x) = amp*sin(omega*x) on xq
    (Dual.py:216-217 + 8-9): returns a device double[3] = [sum (u-ex)^2, sum ex^2, max |u-ex|]
    (accumulated into ``out`` when given, e.g. across shards)."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    _dev(xq, "xq")
    ne = x.numel() - 1
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, M]")
    if out is None:
        out = torch.zeros(3, dtype=torch.float64, device=x.device)
    else:
        _dev(out, "out")
    rc = lib.lssvr_eval_error(_ptr(x), _ptr(W), ne, int(W.shape[1]), _ptr(xq), xq.numel(),
                              _capi.rhs_params(*exact), _ptr(out), _stream(stream))
    _capi.check(rc, "lssvr_eval_error")
    return out


def gauss_rule(nq):
    """Gauss-Legendre nodes (ascending) and weights on [-1, 1] (host; ``lssvr_gauss_rule``)."""
    lib = _capi.load()
    xi = (ctypes.c_double * max(int(nq), 1))()
    wt = (ctypes.c_double * max(int(nq), 1))()
    _capi.check(lib.lssvr_gauss_rule(int(nq), xi, wt), "lssvr_gauss_rule")
    return np.array(xi[:nq], dtype=np.float64), np.array(wt[:nq], dtype=np.float64)


def _adapt_scratch(work, x, ne, entry="lssvr_adapt_work_bytes"):
    """The device scratch of ``entry(ne)`` bytes an adaptive entry takes: a fresh buffer on ``x``'s device, or the
    caller's ``work`` once it is a device buffer of that size."""
    nbytes = getattr(_capi.load(), entry)(int(ne))
    if work is None:
        return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    _dev(work, "work")
    if work.numel() * 8 < nbytes:
        raise ValueError(f"work is smaller than {entry}(ne)")
    return work


def adapt_work(x, ne):
    """Device scratch of ``lssvr_adapt_work_bytes(ne)`` bytes for :func:`estimate` / :func:`refine`."""
    return _adapt_scratch(None, x, ne)


def goal_work(x, ne):
    """Device scratch of ``lssvr_goal_work_bytes(ne)`` bytes for :func:`estimate_goal`."""
    return _adapt_scratch(None, x, ne, "lssvr_goal_work_bytes")


def tridiag_work(x, ne, nc, *families):
    """Device scratch on ``x``'s device for the ``tridiag_*`` solves of nc cases on ne elements of every family named
    ("dirichlet", "bc", "pivot", "periodic"): the largest of their sizers, ``lssvr_tridiag_multi_work_bytes(ne, nc)``,
    ``lssvr_tridiag_bc_work_bytes``, ``lssvr_tridiag_pivot_work_bytes``, ``lssvr_tridiag_periodic_work_bytes``."""
    if not families:
        raise ValueError("name at least one family of " + ", ".join(_TRIDIAG))
    lib = _capi.load()
    return _scratch(None, max(getattr(lib, _TRIDIAG[f].sizer)(int(ne), int(nc)) for f in families), x.device)


def _pair(name, v):
    """A (left, right) argument as the C ABI takes it: double[2]."""
    v = tuple(float(t) for t in v)
    if len(v) != 2:
        raise ValueError(f"{name} must be a pair (left, right)")
    return (ctypes.c_double * 2)(*v)


def _same_device(x, **tensors):
    """Every given tensor lives where ``x`` does (``None`` entries: arguments not given)."""
    for nm, t in tensors.items():
        if t is not None and t.device != x.device:
            raise RuntimeError(f"{nm} lives on {t.device}, x on {x.device}")


def _estimate_out(x, ne, want_jump):
    """(eta2[ne], jump[ne+1] | None, out3[3]) of the estimators, uninitialised."""
    eta2 = torch.empty(ne, dtype=torch.float64, device=x.device)
    jump = torch.empty(ne + 1, dtype=torch.float64, device=x.device) if want_jump else None
    return eta2, jump, torch.empty(3, dtype=torch.float64, device=x.device)


def estimate_points(x, nq, *, stream=None):
    """The estimator's abscissae float64[ne, nq] (tabulate a callable f on it for :func:`estimate`)."""
    lib = _capi.load()
    _dev(x, "x")
    ne = x.numel() - 1
    xq = torch.empty((ne, int(nq)), dtype=torch.float64, device=x.device)
    _capi.check(lib.lssvr_estimate_points(_ptr(x), ne, int(nq), _ptr(xq), _stream(stream)),
                "lssvr_estimate_points")
    return xq


def estimate(x, W, nq, *, rhs=(POISSON_AMP, POISSON_OMEGA), rhs_values=None, point_major=False,
             want_jump=False, work=None, stream=None):
    """Per-element residual indicator of the enhanced solution (``lssvr_estimate``):
    eta2[e] = h^2 int_e (f + u_e'')^2 + h/2 (J_e^2 + J_{e+1}^2).  ``rhs`` = (amp, omega) evaluates
    f in-kernel; ``rhs_values`` float64[ne, nq] (f at :func:`estimate_points`) or, with
    ``point_major``, float64[nq, ne] overrides it.  Returns (eta2 float64[ne], jump float64[ne+1] |
    None, out3 device float64[3] = {sum, max of the finite eta2, non-finite count})."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    ne = x.numel() - 1
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, M]")
    rhs_id, params = _rhs(rhs, rhs_values, ne * int(nq), "ne*nq", point_major)
    eta2, jump, out3 = _estimate_out(x, ne, want_jump)
    work = _adapt_scratch(work, x, ne)
    rc = lib.lssvr_estimate(_ptr(x), _ptr(W), ne, int(W.shape[1]), int(nq), rhs_id, params,
                            _ptr(rhs_values), _ptr(eta2), _ptr(jump), _ptr(out3), _ptr(work),
                            _stream(stream))
    _capi.check(rc, "lssvr_estimate")
    return eta2, jump, out3


def estimate_varcoef(x, W, nq, a_values, da_values, rhs_values, a_ends, *, point_major=False, want_jump=False,
                     work=None, stream=None, c_values=None, b_values=None):
    """:func:`estimate` for -(a u')' = f (``lssvr_estimate_varcoef``):
    eta2[e] = h^2 int_e (f + a u_e'' + a' u_e')^2 + h/2 (J_e^2 + J_{e+1}^2), J the jump of the flux a u'.
    ``a_values``, ``da_values``, ``rhs_values``: a, a' and f at :func:`estimate_points`, float64[ne, nq] or,
    with ``point_major``, float64[nq, ne]; ``a_ends`` float64[ne, 2]: a at the left and right end of every
    element, seen from inside it.  Returns (eta2 float64[ne], jump float64[ne+1] | None, out3 device
    float64[3] = {sum, max of the finite eta2, non-finite count}).
    ``c_values`` (shape of the other tables): the residual of -(a u')' + c u = f, f + a u_e'' + a' u_e' - c u_e
    (``lssvr_estimate_react``); ``None`` is the call without it.
    ``b_values`` (shape and layout of ``da_values``): the convection coefficient of -(a u')' + b u' (+ c u) = f -- the
    residual becomes f + a u_e'' + (a' - b) u_e' (- c u_e): the kernels are handed ``da_values - b_values``, the flux
    jump uses a alone; ``None`` is the call without it."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    da_values = _fold(da_values, b_values)
    ne = x.numel() - 1
    nq = int(nq)
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, M]")
    _tables(ne, nq, point_major, shape=True, a_values=a_values, da_values=da_values, rhs_values=rhs_values,
            **({} if c_values is None else {"c_values": c_values}))
    _dev(a_ends, "a_ends")
    if tuple(a_ends.shape) != (ne, 2):
        raise ValueError(f"a_ends must be [ne, 2] = [{ne}, 2], got {list(a_ends.shape)}")
    eta2, jump, out3 = _estimate_out(x, ne, want_jump)
    work = _adapt_scratch(work, x, ne)
    kind, tabs = _variant(a_values, da_values, rhs_values, c_values)
    name = f"lssvr_estimate_{kind}"
    rc = getattr(lib, name)(_ptr(x), _ptr(W), ne, int(W.shape[1]), nq, *tabs, _layout(point_major), _ptr(a_ends),
                            _ptr(eta2), _ptr(jump), _ptr(out3), _ptr(work), _stream(stream))
    _capi.check(rc, name)
    return eta2, jump, out3


def estimate_ends(x, W, end_kinds, kappa, g, a_ends, eta2, out3, *, stream=None):
    """The boundary term of the indicator at Robin ends (``lssvr_estimate_ends``), IN PLACE on the ``eta2`` [ne] and
    ``out3`` [3] that :func:`estimate` or :func:`estimate_varcoef` returned: at a Robin end
    J = g - kappa u_e(x_end) - a du_e/dn from the end element's row of ``W`` [ne, M], eta2[end element] += h/2 J^2,
    out3 = {sum + the added terms, max with the new values, non-finite count + 1 for a value that stops being
    finite}.  ``end_kinds``, ``kappa``: as in :func:`tridiag_bc_solve_multi`; ``g`` = (left, right); ``a_ends`` =
    (a(x_0), a(x_ne)).  A Dirichlet end adds nothing.  Returns (eta2, out3)."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    _dev(eta2, "eta2")
    _dev(out3, "out3")
    ne = x.numel() - 1
    if x.dim() != 1 or ne < 1:
        raise ValueError("x must be 1-D with at least two nodes")
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, M]")
    if eta2.numel() != ne or out3.numel() != 3:
        raise ValueError(f"eta2 must hold ne = {ne} doubles and out3 three, got {eta2.numel()} and {out3.numel()}")
    kinds, kap = _end_kinds(end_kinds, kappa)
    pairs = _pair("g", g), _pair("a_ends", a_ends)
    _same_device(x, W=W, eta2=eta2, out3=out3)
    rc = lib.lssvr_estimate_ends(_ptr(x), _ptr(W), int(W.shape[1]), ne, kinds[0], kinds[1], kap, *pairs, _ptr(eta2),
                                 _ptr(out3), _stream(stream))
    _capi.check(rc, "lssvr_estimate_ends")
    return eta2, out3


def estimate_seam(x, W, a_seam, eta2, out3, *, stream=None):
    """The seam term of the indicator on a periodic domain (``lssvr_estimate_seam``), IN PLACE on the ``eta2`` [ne]
    and ``out3`` [3] that :func:`estimate` or :func:`estimate_varcoef` returned: J = a_seam[0] u_{ne-1}'(x_ne) -
    a_seam[1] u_0'(x_0) from the last and the first row of ``W`` [ne, M], eta2[ne-1] += h_{ne-1}/2 J^2 and
    eta2[0] += h_0/2 J^2; out3 follows as in :func:`estimate_ends`.  ``a_seam`` = (a at x_ne seen from element ne-1,
    a at x_0 seen from element 0); ne >= 2.  Returns (eta2, out3)."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    _dev(eta2, "eta2")
    _dev(out3, "out3")
    ne = x.numel() - 1
    if x.dim() != 1 or ne < 2:
        raise ValueError("x must be 1-D with at least three nodes: a periodic mesh has at least two elements")
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, M]")
    if eta2.numel() != ne or out3.numel() != 3:
        raise ValueError(f"eta2 must hold ne = {ne} doubles and out3 three, got {eta2.numel()} and {out3.numel()}")
    a = _pair("a_seam", a_seam)
    _same_device(x, W=W, eta2=eta2, out3=out3)
    rc = lib.lssvr_estimate_seam(_ptr(x), _ptr(W), int(W.shape[1]), ne, a, _ptr(eta2), _ptr(out3), _stream(stream))
    _capi.check(rc, "lssvr_estimate_seam")
    return eta2, out3


def estimate_goal(x, Wu, Wz, nq, a_values, da_values, rhs_values, goal_values, a_ends, *, c_values=None,
                  point_major=False, end_kinds=(0, 0), kappa=(0, 0), g=(0, 0), a_bnd=(1, 1), work=None, stream=None,
                  q=None, jump_free=False):
    """Dual-weighted residual of the enhanced solution ``Wu`` [ne, M] for the quantity J(u) = int j u dx of
    -(a u')' + c u = f, weighted with the enhanced dual solution ``Wz`` [ne, M] (``lssvr_estimate_goal``):
    eta[e] = int_e (f + a u_e'' + a' u_e' - c u_e) z_e - 1/2 (J_e z_e(x_e) + J_{e+1} z_e(x_{e+1})), J the jump of the
    flux a u', plus (g - kappa u_e - a du_e/dn) z_e at a Robin end of the domain (``end_kinds``, ``kappa``, ``g`` =
    (left, right) of the primal problem as in :func:`estimate_ends`, ``a_bnd`` = (a(x_0), a(x_ne))).
    ``a_values``, ``da_values``, ``rhs_values``, ``goal_values``, ``c_values``: a, a', f, j and c (or ``None``) at
    :func:`estimate_points`, float64[ne, nq] or, with ``point_major``, float64[nq, ne]; ``a_ends`` float64[ne, 2] as
    in :func:`estimate_varcoef`.  Returns (eta float64[ne] SIGNED, eta2 = eta^2 float64[ne], out4 device float64[4] =
    {sum of eta where eta2 is finite, max finite eta2, non-finite count, sum of the finite q_e}), q_e = int_e j u_e:
    out4[0] + out4[3] is the corrected value of J.  ``q``: a float64[ne] device tensor that receives q_e.
    ``work``: :func:`goal_work`.  ``jump_free``: weight with z_e minus its linear interpolant at the element's nodes
    instead -- the jump and end terms drop out, eta[e] = int_e R (z_e - I_h z_e): the form to mark from, since bisecting
    element e reduces it (half a jump at a node shared with a coarse neighbour it does not)."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(Wu, "Wu")
    _dev(Wz, "Wz")
    ne = x.numel() - 1
    nq = int(nq)
    if x.dim() != 1 or ne < 1:
        raise ValueError("x must be 1-D with at least two nodes")
    if Wu.dim() != 2 or Wu.shape[0] != ne:
        raise ValueError("Wu must be [ne, M]")
    if Wz.shape != Wu.shape:
        raise ValueError(f"Wz must have the shape of Wu {list(Wu.shape)}, got {list(Wz.shape)}")
    _tables(ne, nq, point_major, shape=True, a_values=a_values, da_values=da_values, rhs_values=rhs_values,
            goal_values=goal_values, **({} if c_values is None else {"c_values": c_values}))
    _dev(a_ends, "a_ends")
    if tuple(a_ends.shape) != (ne, 2):
        raise ValueError(f"a_ends must be [ne, 2] = [{ne}, 2], got {list(a_ends.shape)}")
    kinds, kap = _end_kinds(end_kinds, kappa)
    pairs = _pair("g", g), _pair("a_bnd", a_bnd)
    if q is not None:
        _dev(q, "q")
        if q.numel() != ne:
            raise ValueError(f"q must hold ne = {ne} doubles, got {q.numel()}")
    work = _adapt_scratch(work, x, ne, "lssvr_goal_work_bytes")
    _same_device(x, Wu=Wu, Wz=Wz, a_values=a_values, da_values=da_values, rhs_values=rhs_values,
                 goal_values=goal_values, a_ends=a_ends, work=work, c_values=c_values, q=q)
    eta = torch.empty(ne, dtype=torch.float64, device=x.device)
    eta2 = torch.empty(ne, dtype=torch.float64, device=x.device)
    out4 = torch.empty(4, dtype=torch.float64, device=x.device)
    rc = lib.lssvr_estimate_goal(_ptr(x), _ptr(Wu), _ptr(Wz), ne, int(Wu.shape[1]), nq, _ptr(a_values),
                                 _ptr(da_values), _ptr(c_values), _ptr(rhs_values), _ptr(goal_values),
                                 _layout(point_major), _ptr(a_ends), kinds[0], kinds[1], kap, *pairs,
                                 1 if jump_free else 0, _ptr(eta), _ptr(eta2), _ptr(q), _ptr(out4), _ptr(work),
                                 _stream(stream))
    _capi.check(rc, "lssvr_estimate_goal")
    return eta, eta2, out4


def _refine(x, eta2, eta2_max, theta, h_min, want_parent, work, stream, hp=None):
    """What :func:`refine` and :func:`refine_hp` share: the checks, the outputs sized for the case that every element
    is bisected, the launch, ONE synchronisation for the device counters and the trim to the new length.  ``hp`` =
    (sigma, deg, sigma_min, dM, M_max) selects ``lssvr_refine_hp``.  Returns (x_new, deg_new | None, parent | None,
    the counters after ne_new)."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(eta2, "eta2")
    _dev(eta2_max, "eta2_max")
    ne = x.numel() - 1
    if hp is None:
        if eta2.numel() != ne:
            raise ValueError("eta2 must hold ne doubles")
    else:
        sigma, deg, sigma_min, dM, M_max = hp
        _dev(sigma, "sigma")
        if ne < 1:
            raise ValueError("need at least one element")
        if eta2.numel() != ne or sigma.numel() != ne:
            raise ValueError("eta2 and sigma must hold ne doubles")
        if eta2_max.numel() < 1:
            raise ValueError("eta2_max must hold one double")
        _degrees(deg, ne)
    theta = float(theta)
    if not 0.0 <= theta <= 1.0:
        raise ValueError(f"theta must be in [0, 1], got {theta}")
    if hp is not None:
        if int(dM) != dM or dM < 1:
            raise ValueError(f"dM must be a positive integer, got {dM!r}")
        if int(M_max) != M_max or not MIN_DEGREE <= M_max <= MAX_DEGREE:
            raise ValueError(f"M_max must be in [2, 33], got {M_max!r}")
    x_new = torch.empty(2 * ne + 1, dtype=torch.float64, device=x.device)
    deg_new = torch.empty(2 * ne, dtype=torch.int32, device=x.device) if hp is not None else None
    parent = torch.empty(2 * ne, dtype=torch.int64, device=x.device) if want_parent else None
    cnt = torch.empty(1 if hp is None else 3, dtype=torch.int64, device=x.device)    # {ne_new [, bisected, raised]}
    work = _adapt_scratch(work, x, ne)
    head = (_ptr(x), ne, _ptr(eta2), _ptr(eta2_max), theta, float(h_min))
    if hp is None:
        name = "lssvr_refine"
        rc = lib.lssvr_refine(*head, _ptr(work), _ptr(x_new), _ptr(parent), _ptr(cnt), _stream(stream))
    else:
        name = "lssvr_refine_hp"
        rc = lib.lssvr_refine_hp(*head, _ptr(sigma), _ptr(deg), float(sigma_min), int(dM), int(M_max), _ptr(work),
                                 _ptr(x_new), _ptr(deg_new), _ptr(parent), _ptr(cnt[0:1]), _ptr(cnt[1:3]),
                                 _stream(stream))
    _capi.check(rc, name)
    n, *counts = (int(v) for v in cnt.cpu())
    return (x_new[:n + 1], deg_new[:n] if hp is not None else None, parent[:n] if parent is not None else None,
            tuple(counts))


def refine(x, eta2, eta2_max, theta, *, h_min=0.0, want_parent=False, work=None, stream=None):
    """Mark (eta2 non-finite, or eta2 >= theta^2 * max with max > 0; element >= 2 h_min long) and
    bisect (``lssvr_refine``).  ``eta2_max``: device float64 holding max (e.g. ``out3[1:2]`` of
    :func:`estimate`).  Returns (x_new float64[ne_new+1], parent int64[ne_new] | None), trimmed to
    the new length -- one synchronisation, for the count."""
    x_new, _, parent, _ = _refine(x, eta2, eta2_max, theta, h_min, want_parent, work, stream)
    return x_new, parent


MIN_DEGREE, MAX_DEGREE = 2, 33       # the degree parameter M of an element (lssvr_enhance: 2 <= M <= 33)


def _degrees(deg, ne, name="deg"):
    """``deg`` as the kernels take it: a contiguous device int32[ne]."""
    _dev(deg, name, torch.int32)
    if deg.dim() != 1 or deg.numel() != ne:
        raise ValueError(f"{name} must be int32[ne] = [{ne}], got {list(deg.shape)}")
    return deg


def smoothness(x, W, deg, *, out=None, stream=None):
    """Decay rate of every element's Legendre coefficients (``lssvr_smoothness``): minus the least-squares slope
    of ln(envelope of |W[e, p]|) against p = 1 .. deg[e]-1.  ``W`` float64[ne, ldw] (zero-padded rows, 2 <= ldw
    <= 33), ``deg`` int32[ne] with 2 <= deg[e] <= ldw (not checked here: a degree outside that range gives NaN).
    ``x`` float64[ne+1] only fixes ne -- the window of every element is [-1, 1], so the rate does not depend on
    its length.  Returns sigma float64[ne]: +inf for a zero row or fewer than two usable points, NaN for a
    non-finite row."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    ne = x.numel() - 1
    if ne < 1:
        raise ValueError("need at least one element")
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, ldw]")
    ldw = int(W.shape[1])
    if not MIN_DEGREE <= ldw <= MAX_DEGREE:
        raise ValueError(f"W must have 2 <= ldw <= 33 columns, got {ldw}")
    _degrees(deg, ne)
    if out is None:
        out = torch.empty(ne, dtype=torch.float64, device=x.device)
    else:
        _dev(out, "out")
        if out.numel() != ne:
            raise ValueError(f"out must hold ne = {ne} doubles, got {out.numel()}")
    _capi.check(lib.lssvr_smoothness(_ptr(W), ldw, _ptr(deg), ne, _ptr(out), _stream(stream)), "lssvr_smoothness")
    return out


def refine_hp(x, eta2, eta2_max, theta, sigma, deg, *, sigma_min=1.0, dM=2, M_max=MAX_DEGREE, h_min=0.0,
              want_parent=False, work=None, stream=None):
    """:func:`refine`'s marking, then p or h (``lssvr_refine_hp``): a marked element (eta2 non-finite, or eta2 >=
    theta^2 * max with max > 0) gets ``deg + dM`` when ``sigma >= sigma_min`` and ``deg + dM <= M_max``, else is
    bisected when it is at least 2 ``h_min`` long (both halves keep ``deg``), else stays.  ``sigma`` float64[ne]
    from :func:`smoothness`, ``deg`` int32[ne].  Returns (x_new float64[ne_new+1], deg_new int32[ne_new], parent
    int64[ne_new] | None, (bisected, raised)), trimmed to the new length -- one synchronisation, for the counts."""
    return _refine(x, eta2, eta2_max, theta, h_min, want_parent, work, stream, (sigma, deg, sigma_min, dM, M_max))


def group_by_degree(deg, *, work=None, stream=None):
    """Stable counting sort of the element indices by degree (``lssvr_group_by_degree``).  ``deg`` int32[ne].
    Returns (ids int64[ne], offsets int64[35]), both on the device: the elements of degree M are
    ``ids[offsets[M]:offsets[M+1]]`` in ascending mesh order -- a slice that :func:`enhance_subset` takes as
    ``elem_ids``; ``offsets[34]`` counts the elements sorted.  An element whose degree is outside 2 .. 33 is in no
    group (then ``offsets[34] < ne`` and the tail of ``ids`` is unwritten)."""
    lib = _capi.load()
    _dev(deg, "deg", torch.int32)
    ne = deg.numel()
    if deg.dim() != 1 or ne < 1:
        raise ValueError("deg must be int32[ne] with ne >= 1")
    ids = torch.empty(ne, dtype=torch.int64, device=deg.device)
    offsets = torch.empty(MAX_DEGREE + 2, dtype=torch.int64, device=deg.device)
    work = _scratch(None if work is None else _dev(work, "work"), lib.lssvr_group_work_bytes(ne), deg.device)
    rc = lib.lssvr_group_by_degree(_ptr(deg), ne, _ptr(ids), _ptr(offsets), _ptr(work), _stream(stream))
    _capi.check(rc, "lssvr_group_by_degree")
    return ids, offsets


# --------------------------------------------------------------------------
# eigenproblems -(a u')' + c u = lambda rho u
# --------------------------------------------------------------------------
EIG_MAX_BLOCK = TRIDIAG_MULTI_CASES      # widest block of iteration vectors: one pass of the multi solvers


# What the wrappers from here to ``wave_advance`` check, one helper per idea: a new wrapper
# composes these.  ``_dev`` (a contiguous device tensor of the dtype) comes first in every wrapper; these look at shapes.
def _out(t, name, shape, like, dtype=torch.float64):
    """The output buffer ``t`` (allocated when None) of ``shape`` on ``like``'s device."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    _dev(t, name, dtype)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    _same_device(like, **{name: t})
    return t


def _finite(**named):
    """The named scalars as floats, each finite."""
    out = []
    for nm, v in named.items():
        v = float(v)
        if not math.isfinite(v):
            raise ValueError(f"{nm} must be finite, got {v!r}")
        out.append(v)
    return out


def _band_pair(message, diag, off, ne=None):
    """ne of the bands diag[ne+1], off[ne] of one tridiagonal matrix; with ``ne`` given, the check that they have it."""
    if ne is None:
        ne = off.numel()
        if ne < 1:
            raise ValueError("need at least one element")
    if diag.dim() != 1 or off.dim() != 1 or diag.numel() != ne + 1 or off.numel() != ne:
        raise ValueError(message)
    return ne


def _nodes(t, name):
    """ne of the nodal vector ``t`` [ne+1]."""
    if t.dim() != 1 or t.numel() < 2:
        raise ValueError(f"{name} must be 1-D with at least two nodes")
    return t.numel() - 1


def _nodal(ne, message=None, **vectors):
    """Each vector is [ne+1]."""
    for nm, t in vectors.items():
        if t.dim() != 1 or t.numel() != ne + 1:
            raise ValueError(message or f"{nm} must be [ne+1] = [{ne + 1}], got {list(t.shape)}")


def _block(ne, rows, **vectors):
    """The row count of the blocks [rows, ne+1], 1 .. 8 rows and one count for all of them."""
    n = None
    for nm, t in vectors.items():
        if t.dim() != 2 or t.shape[1] != ne + 1 or not 1 <= t.shape[0] <= TRIDIAG_MULTI_CASES:
            raise ValueError(f"{nm} must be [{rows}, ne+1] = [1 .. {TRIDIAG_MULTI_CASES}, {ne + 1}], "
                             f"got {list(t.shape)}")
        if n is not None and t.shape[0] != n:
            raise ValueError(f"{nm} must hold {rows} = {n} vectors, got {t.shape[0]}")
        n = int(t.shape[0])
    return n


def _loads_phi(ne, nc, loads, phi):
    """R of the separable forcing: loads [R, ne+1] with R in 1 .. 8 and phi [nc, R]."""
    if loads.dim() != 2 or loads.shape[1] != ne + 1 or not 1 <= loads.shape[0] <= TS_MAX_TERMS:
        raise ValueError(f"loads must be [R, ne+1] = [1 .. {TS_MAX_TERMS}, {ne + 1}], got {list(loads.shape)}")
    R = int(loads.shape[0])
    if tuple(phi.shape) != (nc, R):
        raise ValueError(f"phi must be [nc, R] = [{nc}, {R}], got {list(phi.shape)}")
    return R


def _lagged(U1, beta1, like, like_name):
    """The array of the step before last: needed when its coefficient is not zero, a device tensor of ``like``'s shape
    when given."""
    if U1 is None:
        if beta1 != 0.0:
            raise ValueError("U1 is needed when beta1 != 0")
        return
    _dev(U1, "U1")
    if U1.shape != like.shape:
        raise ValueError(f"U1 must have the shape of {like_name} {list(like.shape)}, got {list(U1.shape)}")


def _sized_work(work, like, sizer, *args):
    """The scratch of ``sizer(*args)`` bytes on ``like``'s device: the caller's ``work`` once it holds that many (a
    smaller one raises), else a fresh buffer."""
    need = getattr(_capi.load(), sizer)(*args)
    if work is not None:
        _dev(work, "work")
        if work.numel() * work.element_size() < need:
            raise ValueError(f"work holds {work.numel() * work.element_size()} bytes, "
                             f"{sizer}({', '.join(map(str, args))}) = {need}")
        _same_device(like, work=work)
    return _scratch(work, need, like.device)


def _no_alias(message, outs, ins):
    """No output is one of the inputs (``None``: not given), and the outputs are buffers of their own."""
    ptrs = [t.data_ptr() for t in outs]
    taken = {t.data_ptr() for t in ins if t is not None}
    if len(set(ptrs)) != len(ptrs) or not taken.isdisjoint(ptrs):
        raise ValueError(message)


_EIG_BANDS = "band lengths must be ne+1, ne, ne+1, ne (kdiag, koff, mdiag, moff)"


def _eig_bands(kdiag, koff, mdiag, moff):
    """ne of the four bands K = (kdiag[ne+1], koff[ne]), M = (mdiag[ne+1], moff[ne]), checked."""
    for nm, t in (("kdiag", kdiag), ("koff", koff), ("mdiag", mdiag), ("moff", moff)):
        _dev(t, nm)
    ne = _band_pair(_EIG_BANDS, kdiag, koff)
    _band_pair(_EIG_BANDS, mdiag, moff, ne)
    _same_device(kdiag, koff=koff, mdiag=mdiag, moff=moff)
    return ne


def eig_apply(kdiag, koff, mdiag, moff, Z, end_kinds=(END_DIRICHLET, END_DIRICHLET), kappa=(0.0, 0.0), *, MZ=None,
              KZ=None, gram=None, work=None, stream=None):
    """``lssvr_eig_apply``: MZ = M Z, KZ = K Z and gram float64[2, nb, nb] = (Z^T K Z, Z^T M Z) for the block
    ``Z`` float64[nb, ne+1] and the P1 bands K = (kdiag, koff), M = (mdiag, moff).  ``end_kinds``, ``kappa`` as in
    :func:`tridiag_pivot_solve_multi`: a Robin end's node is an unknown and kappa joins K's end diagonal; rows outside
    the unknowns are written as 0 and not read.  The Gram sums run in a fixed order: bitwise reproducible.  Returns
    (MZ, KZ, gram)."""
    lib = _capi.load()
    ne = _eig_bands(kdiag, koff, mdiag, moff)
    _dev(Z, "Z")
    nb = _block(ne, "nb", Z=Z)
    _same_device(kdiag, Z=Z)
    kinds, kap = _end_kinds(end_kinds, kappa, any_sign=True)
    MZ = _out(MZ, "MZ", (nb, ne + 1), kdiag)
    KZ = _out(KZ, "KZ", (nb, ne + 1), kdiag)
    gram = _out(gram, "gram", (2, nb, nb), kdiag)
    work = _sized_work(work, kdiag, "lssvr_eig_work_bytes", ne, nb)
    rc = lib.lssvr_eig_apply(_ptr(kdiag), _ptr(koff), _ptr(mdiag), _ptr(moff), kinds[0], kinds[1], kap, ne, nb, _ptr(Z),
                             _ptr(MZ), _ptr(KZ), _ptr(gram), _ptr(work), work.numel() * work.element_size(),
                             _stream(stream))
    _capi.check(rc, "lssvr_eig_apply")
    return MZ, KZ, gram


def eig_ritz(gram, sigma=0.0, *, theta=None, Q=None, info=None, stream=None):
    """``lssvr_eig_ritz`` on ``gram`` float64[2, nb, nb] = (A, B) as :func:`eig_apply` leaves it: theta float64[nb]
    ascending in |theta - sigma| and Q float64[nb, nb] (column j the vector of theta[j]) with Q^T A Q = diag theta,
    Q^T B Q = I, on the device; info int32[1]: the number of dependent columns of B (zero vectors, ordered last).
    Returns (theta, Q, info)."""
    lib = _capi.load()
    _dev(gram, "gram")
    if gram.dim() != 3 or gram.shape[0] != 2 or gram.shape[1] != gram.shape[2] or \
            not 1 <= gram.shape[1] <= EIG_MAX_BLOCK:
        raise ValueError(f"gram must be [2, nb, nb] with nb in 1 .. {EIG_MAX_BLOCK}, got {list(gram.shape)}")
    (sigma,) = _finite(sigma=sigma)
    nb = int(gram.shape[1])
    theta = _out(theta, "theta", (nb,), gram)
    Q = _out(Q, "Q", (nb, nb), gram)
    info = _out(info, "info", (1,), gram, torch.int32)
    rc = lib.lssvr_eig_ritz(_ptr(gram[0]), _ptr(gram[1]), nb, sigma, _ptr(theta), _ptr(Q), _ptr(info),
                            _stream(stream))
    _capi.check(rc, "lssvr_eig_ritz")
    return theta, Q, info


def eig_rotate(Z, MZ, KZ, Q, theta, end_kinds=(END_DIRICHLET, END_DIRICHLET), *, X=None, Y=None, res2=None,
               work=None, stream=None):
    """``lssvr_eig_rotate``: X = Z Q, Y = (MZ) Q and res2 float64[2, nb] = (|(KZ) Q_j - theta_j (MZ) Q_j|^2, |X_j|^2)
    for the blocks float64[nb, ne+1] and the device arrays ``Q`` [nb, nb], ``theta`` [nb] of :func:`eig_ritz`.  Each
    column is signed so that X's value at the first unknown is >= 0; X and Y must not be Z, MZ or KZ.  Returns
    (X, Y, res2)."""
    lib = _capi.load()
    for nm, t in (("Z", Z), ("MZ", MZ), ("KZ", KZ), ("Q", Q), ("theta", theta)):
        _dev(t, nm)
    if Z.dim() != 2 or Z.shape[1] < 2:
        raise ValueError(f"Z must be [nb, ne+1] with ne >= 1, got {list(Z.shape)}")
    ne = int(Z.shape[1]) - 1
    nb = _block(ne, "nb", Z=Z, MZ=MZ, KZ=KZ)
    if tuple(Q.shape) != (nb, nb) or tuple(theta.shape) != (nb,):
        raise ValueError(f"Q must be [{nb}, {nb}] and theta [{nb}], got {list(Q.shape)} and {list(theta.shape)}")
    _same_device(Z, MZ=MZ, KZ=KZ, Q=Q, theta=theta)
    kinds, _ = _end_kinds(end_kinds, (0.0, 0.0))
    X = _out(X, "X", (nb, ne + 1), Z)
    Y = _out(Y, "Y", (nb, ne + 1), Z)
    for nm, t in (("X", X), ("Y", Y)):
        _no_alias(f"{nm} must not be Z, MZ or KZ", (t,), (Z, MZ, KZ))
    res2 = _out(res2, "res2", (2, nb), Z)
    work = _sized_work(work, Z, "lssvr_eig_work_bytes", ne, nb)
    rc = lib.lssvr_eig_rotate(_ptr(Z), _ptr(MZ), _ptr(KZ), _ptr(Q), _ptr(theta), kinds[0], kinds[1], ne, nb, _ptr(X),
                              _ptr(Y), _ptr(res2), _ptr(work), work.numel() * work.element_size(), _stream(stream))
    _capi.check(rc, "lssvr_eig_rotate")
    return X, Y, res2


def eig_count(kdiag, koff, mdiag, moff, shifts, pivmin, end_kinds=(END_DIRICHLET, END_DIRICHLET), kappa=(0.0, 0.0),
              *, out=None, stream=None):
    """``lssvr_eig_count``: for every entry of ``shifts`` float64[ns] (device) the number of negative pivots of
    LDL^T (K - s M) over the unknowns -- the number of eigenvalues of the pencil below s -- as int32[ns] on the device.
    ``pivmin`` > 0: a pivot smaller in size becomes -pivmin (dstebz).  One lane per shift, serial over the rows."""
    lib = _capi.load()
    ne = _eig_bands(kdiag, koff, mdiag, moff)
    _dev(shifts, "shifts")
    if shifts.dim() != 1:
        raise ValueError("shifts must be 1-D")
    _same_device(kdiag, shifts=shifts)
    ns = int(shifts.numel())
    pivmin = float(pivmin)
    if not (pivmin > 0.0 and math.isfinite(pivmin)):
        raise ValueError(f"pivmin must be finite and > 0, got {pivmin!r}")
    kinds, kap = _end_kinds(end_kinds, kappa, any_sign=True)
    out = _out(out, "out", (ns,), kdiag, torch.int32)
    rc = lib.lssvr_eig_count(_ptr(kdiag), _ptr(koff), _ptr(mdiag), _ptr(moff), kinds[0], kinds[1], kap, ne,
                             _ptr(shifts), ns, pivmin, _ptr(out), _stream(stream))
    _capi.check(rc, "lssvr_eig_count")
    return out


def eig_rayleigh(x, W, nq, a_values, c_values, rho_values, *, point_major=False,
                 end_kinds=(END_DIRICHLET, END_DIRICHLET), kappa=(0.0, 0.0), out=None, work=None, stream=None):
    """``lssvr_eig_rayleigh``: for the enhanced mode ``W`` [ne, M] on the nodes ``x`` and the tables of a, c and rho at
    :func:`estimate_points` (float64[ne, nq] or, with ``point_major``, [nq, ne]) the device array out3 =
    {sum_e int (a u_e'^2 + c u_e^2) + kappa u(x_end)^2 at the Robin ends, sum_e int rho u_e^2, sum |terms| of the
    first}: out3[0] / out3[1] is the Rayleigh quotient.  Fixed-order sums: bitwise reproducible."""
    lib = _capi.load()
    _dev(x, "x")
    _dev(W, "W")
    ne = _nodes(x, "x")
    nq = int(nq)
    if W.dim() != 2 or W.shape[0] != ne:
        raise ValueError("W must be [ne, M]")
    _tables(ne, nq, point_major, shape=True, a_values=a_values, c_values=c_values, rho_values=rho_values)
    kinds, kap = _end_kinds(end_kinds, kappa, any_sign=True)
    out = _out(out, "out", (3,), x)
    work = _sized_work(work, x, "lssvr_eig_work_bytes", ne, 1)
    _same_device(x, W=W, a_values=a_values, c_values=c_values, rho_values=rho_values)
    rc = lib.lssvr_eig_rayleigh(_ptr(x), _ptr(W), ne, int(W.shape[1]), nq, _ptr(a_values), _ptr(c_values),
                                _ptr(rho_values), _layout(point_major), kinds[0], kinds[1], kap, _ptr(out), _ptr(work),
                                _stream(stream))
    _capi.check(rc, "lssvr_eig_rayleigh")
    return out


# --------------------------------------------------------------------------
# transient problems rho u_t - (a u')' + c u = f
# --------------------------------------------------------------------------
TS_MAX_TERMS = 8       # most terms phi_r(t) f_r(x) of a separable forcing
BDF = {"bdf1": (1.0, 1.0, 0.0), "bdf2": (1.5, 2.0, -0.5)}      # scheme -> (alpha, beta0, beta1)


def _bdf_state(ne, like, U0, U1, loads, phi, beta1, out):
    """What :func:`ts_rhs` and :func:`ts_step` check alike once ne is known -> (nc, R, out): U0 [nc, ne+1], loads and
    phi, the lagged U1, and an ``out`` [nc, ne+1] that is neither U0 nor U1."""
    nc = _block(ne, "nc", U0=U0)
    R = _loads_phi(ne, nc, loads, phi)
    _lagged(U1, beta1, U0, "U0")
    out = _out(out, "out", (nc, ne + 1), like)
    _no_alias("out must not be U0 or U1", (out,), (U0, U1))
    return nc, R, out


def ts_rhs(mdiag, moff, U0, U1, loads, phi, beta0, beta1, inv_dt, *, out=None, stream=None):
    """``lssvr_ts_rhs``: the right-hand side of one BDF step for ``nc`` cases,
    out[j] = inv_dt M (beta0 U0[j] + beta1 U1[j]) + sum_r phi[j, r] loads[r], with the mass bands M = (mdiag[ne+1],
    moff[ne]), U0, U1 float64[nc, ne+1] (nc <= 8), loads float64[R, ne+1] (R <= 8, shared by the cases) and phi
    float64[nc, R], all on the device.  ``beta1 == 0`` reads no U1 (``None`` allowed).  Rows 0 and ne are the natural
    end rows.  No synchronisation and no copy; the sums run in a fixed order (bitwise reproducible).  Returns out
    float64[nc, ne+1]; ``out`` must not be U0 or U1."""
    lib = _capi.load()
    for nm, t in (("mdiag", mdiag), ("moff", moff), ("U0", U0), ("loads", loads), ("phi", phi)):
        _dev(t, nm)
    beta0, beta1, inv_dt = _finite(beta0=beta0, beta1=beta1, inv_dt=inv_dt)
    ne = _band_pair("band lengths must be ne+1, ne (mdiag, moff)", mdiag, moff)
    nc, R, out = _bdf_state(ne, mdiag, U0, U1, loads, phi, beta1, out)
    _same_device(mdiag, moff=moff, U0=U0, loads=loads, phi=phi, **({} if U1 is None else {"U1": U1}))
    rc = lib.lssvr_ts_rhs(_ptr(mdiag), _ptr(moff), _ptr(U0), _ptr(U1), _ptr(loads), _ptr(phi), ne, nc, R, beta0, beta1,
                          inv_dt, _ptr(out), _stream(stream))
    _capi.check(rc, "lssvr_ts_rhs")
    return out


def ts_source_table(U2, U0, U1, ftab, rho_tab, phi, alpha, beta0, beta1, inv_dt, *, point_major=False, out=None,
                    stream=None):
    """``lssvr_ts_source_table``: the right-hand-side table of the elliptic enhancement problem of one snapshot,
    out(e, k) = sum_r phi[r] ftab[r](e, k) - rho_tab(e, k) (w_e + (w_{e+1} - w_e) k / (n_colloc - 1)) with the nodal
    BDF difference w = inv_dt (alpha U2 - beta0 U0 - beta1 U1) formed in the kernel.  U2, U0, U1 float64[ne+1];
    ftab float64[R, ne, n_colloc] and rho_tab float64[ne, n_colloc] at :func:`colloc_points` (``point_major``:
    [R, n_colloc, ne] and [n_colloc, ne]); phi float64[R]; all on the device.  ``beta1 == 0`` reads no U1 (``None``
    allowed).  Returns out in rho_tab's shape."""
    lib = _capi.load()
    for nm, t in (("U2", U2), ("U0", U0), ("ftab", ftab), ("rho_tab", rho_tab), ("phi", phi)):
        _dev(t, nm)
    alpha, beta0, beta1, inv_dt = _finite(alpha=alpha, beta0=beta0, beta1=beta1, inv_dt=inv_dt)
    ne = _nodes(U2, "U2")
    if rho_tab.dim() != 2 or rho_tab.shape[1 if point_major else 0] != ne:
        raise ValueError(f"rho_tab must be {'[n_colloc, ne]' if point_major else '[ne, n_colloc]'} with ne = {ne}, "
                         f"got {list(rho_tab.shape)}")
    n = int(rho_tab.shape[0 if point_major else 1])
    if n < 2:
        raise ValueError(f"n_colloc must be >= 2, got {n}")
    if ftab.dim() != 3 or tuple(ftab.shape[1:]) != tuple(rho_tab.shape) or not 1 <= ftab.shape[0] <= TS_MAX_TERMS:
        raise ValueError(f"ftab must be [R, ...] = [1 .. {TS_MAX_TERMS}, {', '.join(map(str, rho_tab.shape))}], "
                         f"got {list(ftab.shape)}")
    R = int(ftab.shape[0])
    if tuple(phi.shape) != (R,):
        raise ValueError(f"phi must be [R] = [{R}], got {list(phi.shape)}")
    if U0.shape != U2.shape:
        raise ValueError(f"U0 must have the shape of U2 {list(U2.shape)}, got {list(U0.shape)}")
    _lagged(U1, beta1, U2, "U2")
    out = _out(out, "out", tuple(rho_tab.shape), U2)
    _same_device(U2, U0=U0, U1=U1, ftab=ftab, rho_tab=rho_tab, phi=phi)
    rc = lib.lssvr_ts_source_table(_ptr(U2), _ptr(U0), _ptr(U1), _ptr(ftab), _ptr(rho_tab), _ptr(phi), ne, n, R,
                                   _layout(point_major), alpha, beta0, beta1, inv_dt, _ptr(out), _stream(stream))
    _capi.check(rc, "lssvr_ts_source_table")
    return out


# ---- adaptive time stepping: variable-step BDF2 with a local error estimate -------------------
def ts_step(kdiag, koff, mdiag, moff, U0, U1, loads, phi, s, beta0, beta1, inv_dt, *, adiag, aoff, write_bands=True,
            out=None, stream=None):
    """``lssvr_ts_step``: the matrix AND the right-hand side of one attempt of variable-step BDF2, in one pass:
    adiag = kdiag + s mdiag, aoff = koff + s moff (s = alpha / h; skipped with ``write_bands=False``, when s is the
    previous attempt's) and out = what :func:`ts_rhs` writes for the one case U0, U1 float64[1, ne+1], loads
    float64[R, ne+1], phi float64[1, R], bit for bit.  K = (kdiag[ne+1], koff[ne]) are the bands of -(a u')' + c u,
    M = (mdiag, moff) the mass bands; ``adiag`` [ne+1] and ``aoff`` [ne] are the caller's buffers.  All on the
    device; ``beta1 == 0`` reads no U1 (``None`` allowed).  No synchronisation and no copy.  Returns out
    float64[1, ne+1]; no output may be an input."""
    lib = _capi.load()
    for nm, t in (("kdiag", kdiag), ("koff", koff), ("mdiag", mdiag), ("moff", moff), ("U0", U0), ("loads", loads),
                  ("phi", phi), ("adiag", adiag), ("aoff", aoff)):
        _dev(t, nm)
    s, beta0, beta1, inv_dt = _finite(s=s, beta0=beta0, beta1=beta1, inv_dt=inv_dt)
    bands = "band lengths must be ne+1 (kdiag, mdiag, adiag) and ne (koff, moff, aoff)"
    ne = _band_pair(bands, mdiag, moff)
    _band_pair(bands, kdiag, koff, ne)
    _band_pair(bands, adiag, aoff, ne)
    if tuple(U0.shape) != (1, ne + 1):
        raise ValueError(f"U0 must be [1, ne+1] = [1, {ne + 1}], got {list(U0.shape)}")
    _, R, out = _bdf_state(ne, mdiag, U0, U1, loads, phi, beta1, out)
    ins = dict(kdiag=kdiag, koff=koff, moff=moff, U0=U0, loads=loads, phi=phi, U1=U1)
    _no_alias("adiag, aoff and out must be three buffers of their own, none of them an input", (adiag, aoff, out),
              (mdiag, *ins.values()))
    _same_device(mdiag, adiag=adiag, aoff=aoff, **ins)
    rc = lib.lssvr_ts_step(_ptr(kdiag), _ptr(koff), _ptr(mdiag), _ptr(moff), _ptr(U0), _ptr(U1), _ptr(loads),
                           _ptr(phi), ne, R, s, beta0, beta1, inv_dt, int(bool(write_bands)), _ptr(adiag), _ptr(aoff),
                           _ptr(out), _stream(stream))
    _capi.check(rc, "lssvr_ts_step")
    return out


def ts_error(U3, U2, U1, U0, weights, atol, rtol, end_kinds=(END_DIRICHLET, END_DIRICHLET), *, out4=None, work=None,
             stream=None):
    """``lssvr_ts_error``: out4 float64[4] on the device = (max |e| / sc, max |e|, max |U3|, the count of rows whose e
    or sc is not finite) with e = ((w3 U3 + w2 U2) + w1 U1) + w0 U0, ``weights`` = (w3, w2, w1, w0) those of a divided
    difference with the estimate's factor folded in, and sc = atol + rtol max(|U3|, |U2|); a Dirichlet end row of
    ``end_kinds`` is skipped.  U3 (the trial), U2, U1, U0 float64[ne+1] on the device; a zero w1 / w0 reads no U1 / U0
    (``None`` allowed).  Bitwise reproducible; no synchronisation -- reading out4 is the caller's."""
    lib = _capi.load()
    _dev(U3, "U3")
    _dev(U2, "U2")
    if len(weights) != 4:
        raise ValueError(f"weights must be (w3, w2, w1, w0), got {len(weights)} values")
    w3, w2, w1, w0, atol, rtol = _finite(w3=weights[0], w2=weights[1], w1=weights[2], w0=weights[3], atol=atol,
                                         rtol=rtol)
    if atol < 0.0 or rtol < 0.0 or not atol + rtol > 0.0:
        raise ValueError(f"atol and rtol must be >= 0 and their sum > 0, got atol = {atol!r}, rtol = {rtol!r}")
    ne = _nodes(U3, "U3")
    named = {"U2": U2}
    for nm, t, w in (("U1", U1, w1), ("U0", U0, w0)):
        if t is None:
            if w != 0.0:
                raise ValueError(f"{nm} is needed when w{nm[1]} != 0")
        else:
            named[nm] = t
    for nm, t in named.items():
        _dev(t, nm)
        if t.shape != U3.shape:
            raise ValueError(f"{nm} must have the shape of U3 {list(U3.shape)}, got {list(t.shape)}")
    kinds, _ = _end_kinds(end_kinds, (0.0, 0.0), any_sign=True)
    out4 = _out(out4, "out4", (4,), U3)
    work = _sized_work(work, U3, "lssvr_ts_error_work_bytes", ne)
    _same_device(U3, **named)
    rc = lib.lssvr_ts_error(_ptr(U3), _ptr(U2), _ptr(named.get("U1")), _ptr(named.get("U0")), kinds[0], kinds[1], ne,
                            w3, w2, w1, w0, atol, rtol, _ptr(out4), _ptr(work), work.numel() * work.element_size(),
                            _stream(stream))
    _capi.check(rc, "lssvr_ts_error")
    return out4


# ---- semilinear problems -(a u')' + b u' + c u + g(x, u) = f ----------------------------------
NL_POLY, NL_EXP = _capi.NL_POLY, _capi.NL_EXP      # LSSVR_NL_*: g = sum_k q_k u^k (1 .. 6 terms); g = q_0 exp(q_1 u)
NL_MAX_TERMS = 6
NL_MAX_POINTS = 64


def nl_kind(kind, nterm):
    """(LSSVR_NL_* id, nterm) of a kind given as the id or as "poly" / "exp"; ``ValueError`` for an unknown kind or a
    term count the kind does not have (POLY: 1 .. 6, EXP: 2)."""
    ids = {"poly": NL_POLY, "exp": NL_EXP, NL_POLY: NL_POLY, NL_EXP: NL_EXP}
    if isinstance(kind, bool) or kind not in ids:
        raise ValueError(f"kind must be 'poly' (NL_POLY) or 'exp' (NL_EXP), got {kind!r}")
    kind, nterm = ids[kind], int(nterm)
    if kind == NL_POLY and not 1 <= nterm <= NL_MAX_TERMS:
        raise ValueError(f"nterm = {nterm} outside 1 .. {NL_MAX_TERMS}")
    if kind == NL_EXP and nterm != 2:
        raise ValueError(f"kind 'exp' takes the two tables q_0, q_1, got {nterm}")
    return kind, nterm


def nl_linearize(u, t_local, kind, q_tabs, f_tab, *, c_tab=None, point_major=False, c_eff=True, f_eff=True,
                 f_res=False, stream=None):
    """``lssvr_nl_linearize``: the tables of one Newton step around the nodal iterate ``u`` float64[ne+1], at the n
    points per element (n <= 64) whose local coordinates in [0, 1] are ``t_local`` float64[n]: with
    u_h = u_e + (u_{e+1} - u_e) t_k,

        c_eff = c + g_u(x, u_h),   f_eff = (f - g(x, u_h)) + g_u(x, u_h) u_h,   f_res = f - g(x, u_h).

    ``kind``: ``NL_POLY`` / "poly" (g = sum_k q_k u^k by Horner) or ``NL_EXP`` / "exp" (g = q_0 exp(q_1 u));
    ``q_tabs`` float64[nterm, ne, n], ``f_tab`` and ``c_tab`` (``None``: c = 0) float64[ne, n] -- ``point_major``:
    [nterm, n, ne] and [n, ne] --, all on the device.  Each of ``c_eff``, ``f_eff``, ``f_res``: True (allocated), a
    tensor of f_tab's shape (written), or False / None (not computed).  Returns the dict of those written.  No
    synchronisation and no copy."""
    lib = _capi.load()
    for nm, t in (("u", u), ("t_local", t_local), ("q_tabs", q_tabs), ("f_tab", f_tab)):
        _dev(t, nm)
    ne = _nodes(u, "u")
    if f_tab.dim() != 2 or f_tab.shape[1 if point_major else 0] != ne:
        raise ValueError(f"f_tab must be {'[n, ne]' if point_major else '[ne, n]'} with ne = {ne}, "
                         f"got {list(f_tab.shape)}")
    n = int(f_tab.shape[0 if point_major else 1])
    if not 1 <= n <= NL_MAX_POINTS:
        raise ValueError(f"n = {n} points per element outside 1 .. {NL_MAX_POINTS}")
    if tuple(t_local.shape) != (n,):
        raise ValueError(f"t_local must be [n] = [{n}], got {list(t_local.shape)}")
    if q_tabs.dim() != 3 or tuple(q_tabs.shape[1:]) != tuple(f_tab.shape):
        raise ValueError(f"q_tabs must be [nterm, {', '.join(map(str, f_tab.shape))}], got {list(q_tabs.shape)}")
    kind, nterm = nl_kind(kind, q_tabs.shape[0])
    if c_tab is not None:
        _dev(c_tab, "c_tab")
        if c_tab.shape != f_tab.shape:
            raise ValueError(f"c_tab must have the shape of f_tab {list(f_tab.shape)}, got {list(c_tab.shape)}")
    outs = {}
    for nm, o in (("c_eff", c_eff), ("f_eff", f_eff), ("f_res", f_res)):
        if o is None or o is False:
            continue
        outs[nm] = _out(None if o is True else o, nm, tuple(f_tab.shape), u)
    if not outs:
        raise ValueError("one of c_eff, f_eff, f_res must be asked for")
    _same_device(u, t_local=t_local, q_tabs=q_tabs, f_tab=f_tab, c_tab=c_tab)
    rc = lib.lssvr_nl_linearize(_ptr(u), _ptr(t_local), _ptr(q_tabs), _ptr(c_tab), _ptr(f_tab), ne, n,
                                _layout(point_major), kind, nterm, _ptr(outs.get("c_eff")), _ptr(outs.get("f_eff")),
                                _ptr(outs.get("f_res")), _stream(stream))
    _capi.check(rc, "lssvr_nl_linearize")
    return outs


def nl_residual(diag, sub, sup, load, u, u_new, end_kinds=(END_DIRICHLET, END_DIRICHLET), kappa=(0.0, 0.0),
                end_values=None, *, out4=None, work=None, stream=None):
    """``lssvr_nl_residual``: out4 float64[4] on the device = (max |r|, max |u_new - u|, max |u_new|, the count of
    non-finite entries met) with r = K u + (Robin end terms) - load on the free rows, 0 on a Dirichlet end row; K the
    bands diag[ne+1], sub[ne], sup[ne] of the LINEAR operator (symmetric: pass ``off`` twice), load = F - G(u).
    ``end_values`` float64[2] on the device: g of a Robin end (needed with one).  Bitwise reproducible; no
    synchronisation -- reading out4 is the caller's."""
    lib = _capi.load()
    for nm, t in (("diag", diag), ("sub", sub), ("sup", sup), ("load", load), ("u", u), ("u_new", u_new)):
        _dev(t, nm)
    lengths = "lengths must be ne+1 (diag, load, u, u_new) and ne (sub, sup)"
    ne = _band_pair(lengths, diag, sub)
    _band_pair(lengths, diag, sup, ne)
    _nodal(ne, lengths, load=load, u=u, u_new=u_new)
    kinds, kap = _end_kinds(end_kinds, kappa, any_sign=True)
    if end_values is not None:
        _dev(end_values, "end_values")
        if end_values.numel() != 2:
            raise ValueError(f"end_values must hold 2 doubles, got {end_values.numel()}")
    elif END_ROBIN in kinds:
        raise ValueError("end_values (device float64[2]) is needed with a Robin end")
    out4 = _out(out4, "out4", (4,), diag)
    work = _sized_work(work, diag, "lssvr_nl_residual_work_bytes", ne)
    _same_device(diag, sub=sub, sup=sup, load=load, u=u, u_new=u_new, end_values=end_values)
    rc = lib.lssvr_nl_residual(_ptr(diag), _ptr(sub), _ptr(sup), _ptr(load), _ptr(u), _ptr(u_new), kinds[0], kinds[1],
                               _ptr(end_values), kap, ne, _ptr(out4), _ptr(work),
                               work.numel() * work.element_size(), _stream(stream))
    _capi.check(rc, "lssvr_nl_residual")
    return out4


def nl_step(u, u_new, lam, *, out=None, stream=None):
    """``lssvr_nl_step``: out = u + lam (u_new - u), the trial point of the line search; float64[ne+1] device
    tensors, ``out`` neither u nor u_new."""
    lib = _capi.load()
    _dev(u, "u")
    _dev(u_new, "u_new")
    (lam,) = _finite(lam=lam)
    if u.dim() != 1 or u.numel() < 2 or u_new.shape != u.shape:
        raise ValueError("u and u_new must be 1-D of one length ne+1 >= 2")
    out = _out(out, "out", tuple(u.shape), u)
    _no_alias("out must not be u or u_new", (out,), (u, u_new))
    _same_device(u, u_new=u_new)
    _capi.check(lib.lssvr_nl_step(_ptr(u), _ptr(u_new), lam, u.numel() - 1, _ptr(out), _stream(stream)),
                "lssvr_nl_step")
    return out


# ---- semilinear transient problems rho u_t - (a u')' + c u + g(x, u) = f ----------------------
def ts_nl_assemble(x, u, cs_quad, kind, q_quad, r, *, a_quad=None, out=None, stream=None):
    """``lssvr_ts_nl_assemble``: the bands and the right-hand side of one Newton iteration of a semilinear time step
    in ONE launch -- bit for bit what :func:`nl_linearize` (``f_tab`` = 0, ``c_tab`` = cs_quad) ->
    :func:`p1_assemble` (``c_quad`` = c_eff, ``rhs_quad`` = f_eff) -> ``r + load`` gives, without its two tables.
    ``x``, ``u`` (the iterate) and ``r`` (the step's vector of :func:`ts_rhs`) float64[ne+1]; ``cs_quad``
    (= c + alpha rho / dt), ``a_quad`` (``None``: a = 1) float64[ne, nquad] and ``q_quad`` float64[nterm, ne, nquad] at
    :func:`quad_points`, nquad 1 .. 5; ``kind``: ``NL_POLY`` / "poly" or ``NL_EXP`` / "exp"; all on the device.
    ``out``: a dict with diag[ne+1], off[ne], rhs[ne+1] to write into (``None``: allocated); none of them may be an
    input.  Returns that dict.  No synchronisation and no copy; bitwise reproducible."""
    lib = _capi.load()
    for nm, t in (("x", x), ("u", u), ("cs_quad", cs_quad), ("q_quad", q_quad), ("r", r)):
        _dev(t, nm)
    ne = _nodes(x, "x")
    _nodal(ne, u=u, r=r)
    if cs_quad.dim() != 2 or cs_quad.shape[0] != ne or not 1 <= cs_quad.shape[1] <= 5:
        raise ValueError(f"cs_quad must be [ne, nquad] = [{ne}, 1 .. 5], got {list(cs_quad.shape)}")
    nquad = int(cs_quad.shape[1])
    if q_quad.dim() != 3 or tuple(q_quad.shape[1:]) != (ne, nquad):
        raise ValueError(f"q_quad must be [nterm, {ne}, {nquad}], got {list(q_quad.shape)}")
    kind, nterm = nl_kind(kind, q_quad.shape[0])
    if a_quad is not None:
        _dev(a_quad, "a_quad")
        if a_quad.shape != cs_quad.shape:
            raise ValueError(f"a_quad must have the shape of cs_quad {list(cs_quad.shape)}, got {list(a_quad.shape)}")
    want = {"diag": (ne + 1,), "off": (ne,), "rhs": (ne + 1,)}
    if out is None:
        out = {}
    elif not isinstance(out, dict) or any(k not in out for k in want):
        raise ValueError("out must be a dict with diag, off and rhs")
    res = {k: _out(out.get(k), k, shape, x) for k, shape in want.items()}
    _no_alias("diag, off and rhs must be distinct and none of them an input", res.values(),
              (x, u, cs_quad, q_quad, r, a_quad))
    _same_device(x, u=u, cs_quad=cs_quad, q_quad=q_quad, r=r, a_quad=a_quad)
    rc = lib.lssvr_ts_nl_assemble(_ptr(x), _ptr(u), _ptr(a_quad), _ptr(cs_quad), _ptr(q_quad), _ptr(r), ne, nquad, kind,
                                  nterm, _ptr(res["diag"]), _ptr(res["off"]), _ptr(res["rhs"]), _stream(stream))
    _capi.check(rc, "lssvr_ts_nl_assemble")
    return res


# ---- wave problems rho u_tt + d u_t - (a u')' + c u = f, Newmark --------------------------------
def wave_advance(U_new, U, V, Acc, mdiag, moff, ddiag, doff, loads, phi, dt, beta, gamma, *, V_out=None, Acc_out=None,
                 rhs_out=None, rhs=True, stream=None):
    """``lssvr_wave_advance``: ONE launch of a Newmark step for ``nc`` cases -- the correctors of the step just solved,
    Acc_out = (U_new - ut) / (beta dt^2), V_out = vt + gamma dt Acc_out with ut = U + dt V + dt^2 (1/2 - beta) Acc,
    vt = V + dt (1 - gamma) Acc, and the right-hand side of the next step from the new state (u, v, acc),
    rhs_out[j] = M_rho (ut / (beta dt^2)) + M_d ((gamma / (beta dt)) ut - vt) + sum_r phi[j, r] loads[r].  U_new, U, V,
    Acc float64[nc, ne+1] (nc <= 8), the mass bands M_rho = (mdiag[ne+1], moff[ne]) and M_d = (ddiag, doff)
    (``ddiag=None``: d = 0, neither is read), loads float64[R, ne+1] (R <= 8), phi float64[nc, R], all on the device.
    ``U_new=None``: (U, V, Acc) is the state already and only rhs_out is written (the first step);  ``rhs=False``: the
    correctors only (the last step, or a split call; the bands, loads and phi may be ``None``).  V_out and Acc_out
    must not be V, Acc, U or U_new: every thread recomputes its neighbours' correctors from the old arrays, which is
    what lets one launch do both without a barrier.  No synchronisation and no copy; the sums run in a fixed order
    (bitwise reproducible, and the fused call equals the split pair bit for bit).  Returns (V_out, Acc_out, rhs_out),
    ``None`` for what the mode does not write."""
    lib = _capi.load()
    if U_new is None and not rhs:
        raise ValueError("U_new=None with rhs=False leaves nothing to compute")
    for nm, t in (("U", U), ("V", V), ("Acc", Acc)):
        _dev(t, nm)
    dt, beta, gamma = _finite(dt=dt, beta=beta, gamma=gamma)
    if not (dt > 0.0 and beta > 0.0 and gamma > 0.0):
        raise ValueError(f"dt, beta and gamma must be > 0, got {dt!r}, {beta!r}, {gamma!r}")
    if U.dim() != 2 or U.shape[1] < 2 or not 1 <= U.shape[0] <= TRIDIAG_MULTI_CASES:
        raise ValueError(f"U must be [nc, ne+1] with nc in 1 .. {TRIDIAG_MULTI_CASES} and ne >= 1, got {list(U.shape)}")
    nc, ne = int(U.shape[0]), int(U.shape[1]) - 1
    named = {"V": V, "Acc": Acc}
    if U_new is not None:
        _dev(U_new, "U_new")
        named["U_new"] = U_new
    for nm, t in named.items():
        if t.shape != U.shape:
            raise ValueError(f"{nm} must have the shape of U {list(U.shape)}, got {list(t.shape)}")
    R = 1
    if rhs:
        for nm, t in (("mdiag", mdiag), ("moff", moff), ("loads", loads), ("phi", phi)):
            if t is None:
                raise ValueError(f"{nm} is needed for the right-hand side")
            _dev(t, nm)
        _band_pair(f"band lengths must be ne+1, ne = {ne + 1}, {ne} (mdiag, moff)", mdiag, moff, ne)
        R = _loads_phi(ne, nc, loads, phi)
        named.update(mdiag=mdiag, moff=moff, loads=loads, phi=phi)
        if ddiag is not None:
            if doff is None:
                raise ValueError("doff is needed with ddiag")
            for nm, t in (("ddiag", ddiag), ("doff", doff)):
                _dev(t, nm)
            _band_pair(f"band lengths must be ne+1, ne = {ne + 1}, {ne} (ddiag, doff)", ddiag, doff, ne)
            named.update(ddiag=ddiag, doff=doff)
    else:
        mdiag = moff = ddiag = doff = loads = phi = None
    if ddiag is None:
        doff = None
    outs = {}
    if U_new is not None:
        outs["V_out"] = _out(V_out, "V_out", tuple(U.shape), U)
        outs["Acc_out"] = _out(Acc_out, "Acc_out", tuple(U.shape), U)
    if rhs:
        outs["rhs_out"] = _out(rhs_out, "rhs_out", tuple(U.shape), U)
    _no_alias("V_out, Acc_out and rhs_out must be distinct and none of them an input (neighbours read the old values)",
              outs.values(), (U, *named.values()))
    _same_device(U, **named)
    rc = lib.lssvr_wave_advance(_ptr(U_new), _ptr(U), _ptr(V), _ptr(Acc), _ptr(mdiag), _ptr(moff), _ptr(ddiag),
                                _ptr(doff), _ptr(loads), _ptr(phi), ne, nc, R, dt, beta, gamma,
                                _ptr(outs.get("V_out")), _ptr(outs.get("Acc_out")), _ptr(outs.get("rhs_out")),
                                _stream(stream))
    _capi.check(rc, "lssvr_wave_advance")
    return outs.get("V_out"), outs.get("Acc_out"), outs.get("rhs_out")


# ---- adjoint sensitivities of the P1 solve -------------------------------------------------------
SENS_TABLES = ("a", "b", "c", "f")      # d/d a_quad, b_quad, c_quad, rhs_quad: the keys of ``want`` and of the result


def adjoint_bands(bands):
    """The band dict of the TRANSPOSED matrix: ``sub`` and ``sup`` exchanged (in csrc/p1_conv.hip sub[i] multiplies u_i
    in row i+1 and sup[i] multiplies u_{i+1} in row i), every other entry -- ``diag``, ``load``, a symmetric ``off`` --
    as it is.  A new dict of the same tensors: nothing is copied.  The adjoint solve of :func:`p1_sensitivity` is the
    primal's solve on these bands."""
    out = dict(bands)
    if ("sub" in bands) != ("sup" in bands):
        raise ValueError("bands must hold both sub and sup, or neither (symmetric: off)")
    if "sub" in bands:
        out["sub"], out["sup"] = bands["sup"], bands["sub"]
    return out


def _sens_bind(x, U, Z, nquad, want, tables, P, bands, end_kinds, out, nterm=None):
    """The host checks and the output buffers :func:`p1_sensitivity` and :func:`nl_sensitivity` share -> (ne, nquad, nu,
    nc, res, band_ends, kinds, ins): ``tables`` the keys ``want`` may name (an empty ``want`` passes only with
    ``bands`` and ``nterm``: the end gradients alone), ``res`` the dict of the outputs -- [nc, ne, nquad] per table,
    [nc, nterm, ne, nquad] for "q", "ends" [nc, 4] with ``bands`` --, ``band_ends`` the pair (sub[0], sup[ne-1]) on the
    device or None, ``ins`` the inputs by name for the alias and device checks."""
    for nm, t in (("x", x), ("U", U), ("Z", Z)):
        _dev(t, nm)
    ne = _nodes(x, "x")
    nquad = int(nquad)
    if not 1 <= nquad <= 5:
        raise ValueError(f"nquad must be in 1 .. 5, got {nquad}")
    want = tuple(want)
    ends_only = not want and nterm is not None and bands is not None
    if (not want and not ends_only) or len(set(want)) != len(want) or any(k not in tables for k in want):
        raise ValueError(f"want must name at least one of {tables}, each once, got {want!r}")
    U2, Z2 = (t.view(1, -1) if t.dim() == 1 else t for t in (U, Z))
    nc = _block(ne, "nc", Z=Z2)
    nu = _block(ne, "nu", U=U2)
    if nu not in (1, nc):
        raise ValueError(f"U must hold 1 or nc = {nc} vectors, got {nu}")
    ins = {"U": U, "Z": Z}
    if P is not None:
        _dev(P, "P")
        if P.numel() != Z.numel():
            raise ValueError(f"P must have the shape of Z {list(Z.shape)}, got {list(P.shape)}")
        ins["P"] = P
    out = {} if out is None else out
    res = {k: _out(out.get(k), f"out[{k!r}]", (nc, nterm, ne, nquad) if k == "q" else (nc, ne, nquad), x)
           for k in want}
    band_ends = None
    if bands is not None:
        kinds, _ = _end_kinds(end_kinds, (0.0, 0.0))
        sub, sup = (bands["sub"], bands["sup"]) if "sub" in bands else (bands["off"], bands["off"])
        for nm, t in (("sub", sub), ("sup", sup)):
            _dev(t, nm)
            if t.numel() != ne:
                raise ValueError(f"{nm} must hold ne = {ne} doubles, got {t.numel()}")
        band_ends = torch.stack((sub.reshape(-1)[0], sup.reshape(-1)[ne - 1]))
        ins.update(sub=sub, sup=sup)
        res["ends"] = _out(out.get("ends"), "out['ends']", (nc, 4), x)
    else:
        kinds = (END_DIRICHLET, END_DIRICHLET)
    return ne, nquad, nu, nc, res, band_ends, kinds, ins


def p1_sensitivity(x, U, Z, nquad=2, *, want=SENS_TABLES, P=None, bands=None,
                   end_kinds=(END_DIRICHLET, END_DIRICHLET), out=None, stream=None):
    """``lssvr_p1_sensitivity``: from ``nc`` pairs of a primal solution U[j] and an adjoint solution Z[j] (the solve of
    :func:`adjoint_bands` with load dJ/du, zero end data, the primal's end kinds and kappa) the gradients of J with
    respect to the tables of :func:`p1_assemble`, in ONE launch.  x float64[ne+1]; Z float64[nc, ne+1] (nc <= 8; a
    1-D vector is one case); U float64[nc, ne+1], or [1, ne+1] / 1-D for one primal solution shared by all cases.
    ``want``: which of "a", "b", "c", "f" (a_quad, b_quad, c_quad, rhs_quad) to compute, at least one; a table left
    out is neither computed nor stored.  The tables themselves are not arguments: given u and z the gradient does not
    depend on them.  ``bands`` (the RAW primal bands of :func:`p1_assemble`, with ``sub``/``sup`` or ``off``) asks for
    the end gradients too, for the ends ``end_kinds``; ``P`` float64 like Z is dJ/du, read at a Dirichlet end
    (``None``: zero).  Returns a dict: every wanted key -> float64[nc, ne, nquad], and with ``bands`` "ends" ->
    float64[nc, 4] = (dJ/dg_0, dJ/dg_ne, dJ/dkappa_0, dJ/dkappa_ne).  ``out``: a dict of buffers to write into, by
    those keys.  No synchronisation and no copy; every value is computed in a fixed order (bitwise reproducible)."""
    lib = _capi.load()
    ne, nquad, nu, nc, res, band_ends, kinds, ins = _sens_bind(x, U, Z, nquad, want, SENS_TABLES, P, bands, end_kinds,
                                                               out)
    _no_alias("the outputs must be distinct and none of them an input", res.values(), (x, *ins.values()))
    _same_device(x, **ins)
    rc = lib.lssvr_p1_sensitivity(_ptr(x), ne, nquad, _ptr(U), nu, _ptr(Z), nc, *(_ptr(res.get(k)) for k in SENS_TABLES),
                                  _ptr(P), _ptr(band_ends), *kinds, _ptr(res.get("ends")), _stream(stream))
    _capi.check(rc, "lssvr_p1_sensitivity")
    return res


# ---- adjoint sensitivities of the semilinear P1 solve -----------------------------------------
NL_SENS_TABLES = SENS_TABLES + ("q",)      # "q": d/d q_tabs, the tables of g(x, u)


def nl_sensitivity(x, U, Z, nquad, kind, nterm, *, q_tabs=None, want=NL_SENS_TABLES, P=None, bands=None,
                   end_kinds=(END_DIRICHLET, END_DIRICHLET), out=None, stream=None):
    """``lssvr_semilinear_sensitivity``: :func:`p1_sensitivity` for the semilinear problem with g(x, u) of ``kind``
    ("poly" / ``NL_POLY``, "exp" / ``NL_EXP``) and ``nterm`` tables, in ONE launch.  U is the CONVERGED solution u* and Z
    the adjoint of the Jacobian AT u*: the solve of :func:`adjoint_bands` of ONE :func:`p1_assemble` with c_quad = c_eff
    of ONE :func:`nl_linearize` at u*.  ``want`` names any of "a", "b", "c", "f" -- float64[nc, ne, nquad], bit for bit
    the values of :func:`p1_sensitivity` -- and "q" -- float64[nc, nterm, ne, nquad] = dJ/dq_k at every quadrature
    point; "q" of "poly" has q[:, 0] == -f and q[:, 1] == c bit for bit.  It may be empty with ``bands`` (the end
    gradients alone).  ``q_tabs`` float64[nterm, ne, nquad], the tables :func:`nl_linearize` took, is read for "exp"
    only and must be given then.  ``bands`` are the raw JACOBIAN bands; ``P``, ``end_kinds``, ``out`` and the result as
    for :func:`p1_sensitivity`.  No synchronisation and no copy."""
    lib = _capi.load()
    kind, nterm = nl_kind(kind, nterm)
    ne, nquad, nu, nc, res, band_ends, kinds, ins = _sens_bind(x, U, Z, nquad, want, NL_SENS_TABLES, P, bands,
                                                               end_kinds, out, nterm)
    if q_tabs is not None:
        _dev(q_tabs, "q_tabs")
        if tuple(q_tabs.shape) != (nterm, ne, nquad):
            raise ValueError(f"q_tabs must be [nterm, ne, nquad] = [{nterm}, {ne}, {nquad}], got {list(q_tabs.shape)}")
        ins["q_tabs"] = q_tabs
    elif kind == NL_EXP:
        raise ValueError("kind 'exp' needs q_tabs: dJ/dq_k depends on q_0 and q_1")
    _no_alias("the outputs must be distinct and none of them an input", res.values(), (x, *ins.values()))
    _same_device(x, **ins)
    rc = lib.lssvr_semilinear_sensitivity(_ptr(x), ne, nquad, _ptr(U), nu, _ptr(Z), nc, _ptr(q_tabs), kind, nterm,
                                  *(_ptr(res.get(k)) for k in NL_SENS_TABLES), _ptr(P), _ptr(band_ends), *kinds,
                                  _ptr(res.get("ends")), _stream(stream))
    _capi.check(rc, "lssvr_semilinear_sensitivity")
    return res


# ---- adjoint of the element solve ----------------------------------------------------------------
ENH_ADJ_OUTPUTS = ("u", "bc", "a", "da", "c", "f")      # the keys of ``want`` and of the result
ENH_ADJ_MIN_M, ENH_ADJ_MAX_M, ENH_ADJ_MAX_COLLOC = 3, 16, 64


def enhance_adjoint(x, W, Wbar, M, gamma, n_colloc, rhs_values, *, a_values=None, da_values=None, c_values=None,
                    status=None, want=("u", "f"), elem_offset=0, ne_global=None, global_domain=None, out=None,
                    work=None, stream=None):
    """``lssvr_enhance_adjoint``: the backward of :func:`enhance_varcoef` (element-major tables, primal solve).  From
    the forward call's ``W`` float64[ne, M] (and ``status`` int32[ne]; ``None``: no fallback element) and
    ``Wbar`` = dJ/dW float64[ne, M], the gradients of J named in ``want``: "u" float64[ne+1] (nodal values), "bc"
    float64[2] (the Dirichlet values, where the forward call put them in place of a nodal value; "u" is 0 there), and
    "a", "da", "c", "f" float64[ne, n_colloc] (the tables; ``da_values`` is what the forward kernel was handed, a' - b
    with convection).  ``a_values=None`` (then ``da_values`` must be None) means a = 1, a' = 0 and ``c_values=None``
    c = 0; "a" and "da" need ``a_values``, "c" needs ``c_values``.  Neither u nor the Dirichlet values are arguments:
    W carries them.  ``elem_offset``, ``ne_global``, ``global_domain`` as in :func:`enhance_varcoef`.  3 <= M <= 16,
    max(2, M - 2) <= n_colloc <= 64.  Returns a dict of the wanted keys; ``out``: a dict of buffers to write into, by
    those keys; ``work``: float64[ne, 2], receives the per-element pairs (dJ/dg_l, dJ/dg_r).  One lane kernel and, with
    "u" or "bc", one gather kernel; no synchronisation and no copy (but the read-back of the shard's ends when
    ``global_domain`` is None); every value is computed in a fixed order (bitwise reproducible)."""
    lib = _capi.load()
    M, n_colloc = int(M), int(n_colloc)
    _dev(x, "x")
    ne = _nodes(x, "x")
    if not ENH_ADJ_MIN_M <= M <= ENH_ADJ_MAX_M:
        raise ValueError(f"M must be in {ENH_ADJ_MIN_M} .. {ENH_ADJ_MAX_M}, got {M}")
    if not max(2, M - 2) <= n_colloc <= ENH_ADJ_MAX_COLLOC:
        raise ValueError(f"n_colloc must be in {max(2, M - 2)} .. {ENH_ADJ_MAX_COLLOC}, got {n_colloc}")
    want = tuple(want)
    if not want or len(set(want)) != len(want) or any(k not in ENH_ADJ_OUTPUTS for k in want):
        raise ValueError(f"want must name at least one of {ENH_ADJ_OUTPUTS}, each once, got {want!r}")
    if a_values is None and da_values is not None:
        raise ValueError("da_values needs a_values")
    if a_values is None and ("a" in want or "da" in want):
        raise ValueError('want "a" and "da" need a_values')
    if c_values is None and "c" in want:
        raise ValueError('want "c" needs c_values')
    tabs = {k: t for k, t in (("rhs_values", rhs_values), ("a_values", a_values), ("da_values", da_values),
                              ("c_values", c_values)) if t is not None or k == "rhs_values"}
    _tables(ne, n_colloc, **tabs)
    rows = {"W": W, "Wbar": Wbar}
    for nm, t in rows.items():
        _dev(t, nm)
        if t.numel() != ne * M:
            raise ValueError(f"{nm} must hold ne*M = {ne * M} doubles, got {t.numel()}")
    ins = dict(tabs, **rows)
    if status is not None:
        _dev(status, "status", torch.int32)
        if status.numel() != ne:
            raise ValueError(f"status must be int32[ne = {ne}], got {list(status.shape)}")
        ins["status"] = status
    out = {} if out is None else out
    shapes = {"u": (ne + 1,), "bc": (2,)}
    res = {k: _out(out.get(k), f"out[{k!r}]", shapes.get(k, (ne, n_colloc)), x) for k in want}
    work = _out(work, "work", (ne, 2), x)
    _no_alias("the outputs and work must be distinct and none of them an input", (*res.values(), work),
              (x, *ins.values()))
    _same_device(x, **ins)
    ne_global = elem_offset + ne if ne_global is None else ne_global
    if global_domain is None:
        ends = torch.stack([x[0], x[-1]]).cpu()
        global_domain = (float(ends[0]), float(ends[1]))
    rc = lib.lssvr_enhance_adjoint(_ptr(x), ne, int(elem_offset), int(ne_global), float(global_domain[0]),
                                   float(global_domain[1]), M, n_colloc, float(gamma), _ptr(a_values), _ptr(da_values),
                                   _ptr(c_values), _ptr(rhs_values), _ptr(W), _ptr(status), _ptr(Wbar),
                                   *(_ptr(res.get(k)) for k in ENH_ADJ_OUTPUTS), _ptr(work), work.numel() * 8,
                                   _stream(stream))
    _capi.check(rc, "lssvr_enhance_adjoint")
    return res


# ---- the chunk pass of the time-loop adjoint sensitivities (DESIGN.md sections 32 and 34) ------------------------------
def _chunk_sens(tables, n0_min, phi_rows, band_shape, x, Utraj, Z, n0, nquad, want, trajs, phi, Brows, band_ends,
                end_kinds, accumulate, out, leading=None):
    """What :func:`ts_sensitivity`, :func:`newmark_sensitivity` and :func:`ts_nl_sensitivity` share: every check of the
    chunk's arguments, the ``accumulate`` rule, the allocation of the outputs and the alias and device checks.  ``tables``: the scheme's keys of
    ``want``; ``n0_min``: its lowest first level; ``phi_rows``: how many rows more than N its phi has; ``band_shape``:
    the shape of its ``band_ends`` (-1: the chunk's m); ``trajs``: {name: (table, tensor)}, its own trajectories, each
    needed for one table; ``leading``: {table: n}, its tables that are [n, ne, nquad].  Returns (ne, nquad, n0, m, R, kinds, ins, res): ``ins`` the inputs given, by name, and ``res`` the
    outputs."""
    for nm, t in (("x", x), ("Utraj", Utraj), ("Z", Z)):
        _dev(t, nm)
    ne = _nodes(x, "x")
    nquad, n0 = int(nquad), int(n0)
    if not 1 <= nquad <= 5:
        raise ValueError(f"nquad must be in 1 .. 5, got {nquad}")
    want = tuple(want)
    if len(set(want)) != len(want) or any(k not in tables for k in want):
        raise ValueError(f"want must name tables of {tables}, each once, got {want!r}")
    if not want and Brows is None:
        raise ValueError("nothing to compute: want is empty and Brows is not given")
    m = _block(ne, "m", Z=Z)
    if n0 < n0_min:
        raise ValueError(f"n0 must be >= {n0_min}, got {n0}")
    ins, R = {"Utraj": Utraj, "Z": Z}, 0
    for nm, (key, t) in trajs.items():
        if key in want:
            if t is None:
                raise ValueError(f"{nm} is needed for the table {key!r}")
            _dev(t, nm)
            ins[nm] = t
    for nm in ("Utraj", *trajs):
        t = ins.get(nm)
        if t is not None and (t.dim() != 2 or t.shape[1] != ne + 1 or t.shape[0] < n0 + m or t.shape != Utraj.shape):
            raise ValueError(f"{nm} must be [N+1, ne+1] with N >= n0+m-1 = {n0 + m - 1} and ne+1 = {ne + 1}, one N for "
                             f"all trajectories, got {list(t.shape)}")
    N = int(Utraj.shape[0]) - 1
    if "f" in want:
        if phi is None:
            raise ValueError("phi is needed for the table 'f'")
        _dev(phi, "phi")
        if phi.dim() != 2 or phi.shape[0] != N + phi_rows or not 1 <= phi.shape[1] <= TS_MAX_TERMS:
            raise ValueError(f"phi must be [N{'+1' * phi_rows}, R] = [{N + phi_rows}, 1 .. {TS_MAX_TERMS}], got "
                             f"{list(phi.shape)}")
        R = int(phi.shape[1])
        ins["phi"] = phi
    out = {} if out is None else out
    shapes = {k: ((R, ne, nquad) if k == "f" else (ne, nquad)) for k in want}
    shapes.update({k: (n, ne, nquad) for k, n in (leading or {}).items() if k in want})
    kinds = (END_DIRICHLET, END_DIRICHLET)
    if Brows is not None:
        if band_ends is None:
            raise ValueError("band_ends is needed with Brows")
        for nm, t in (("Brows", Brows), ("band_ends", band_ends)):
            _dev(t, nm)
        if Brows.shape != Z.shape:
            raise ValueError(f"Brows must have the shape of Z {list(Z.shape)}, got {list(Brows.shape)}")
        band_shape = tuple(m if n == -1 else n for n in band_shape)
        if tuple(band_ends.shape) != band_shape:
            raise ValueError(f"band_ends must be {list(band_shape)}, got {list(band_ends.shape)}")
        kinds, _ = _end_kinds(end_kinds, (0.0, 0.0))
        ins.update(Brows=Brows, band_ends=band_ends)
        if out.get("g") is None:
            raise ValueError("out['g'] (float64[N+1, 2]) is needed with Brows: the chunk writes its rows of it")
        shapes.update(g=(N + 1, 2), kappa=(2,))
    if accumulate and any(out.get(k) is None for k in shapes):
        raise ValueError("accumulate needs every buffer it continues from in out")
    res = {k: _out(out.get(k), f"out[{k!r}]", shape, x) for k, shape in shapes.items()}
    _no_alias("the outputs must be distinct and none of them an input", res.values(), (x, *ins.values()))
    _same_device(x, **ins)
    return ne, nquad, n0, m, R, kinds, ins, res


# ---- adjoint sensitivities of the BDF loop -------------------------------------------------------
TS_SENS_TABLES = ("a", "c", "rho", "f")     # d/d a_quad, c_quad, rho_quad, f_quad[r]: the keys of ``want`` and the result
TS_SENS_CHUNK = 8                           # most adjoint steps of one launch


def ts_sensitivity(x, Utraj, Z, n0, coef, inv_dt, nquad=2, *, want=TS_SENS_TABLES, phi=None, Brows=None, band_ends=None,
                   band_rows=None, end_kinds=(END_DIRICHLET, END_DIRICHLET), accumulate=False, out=None, stream=None):
    """``lssvr_transient_sensitivity``: the gradients of J with respect to the tables of the BDF loop of :func:`ts_rhs`, summed
    over a CHUNK of m <= 8 consecutive adjoint steps n0 .. n0+m-1, in ONE launch.  x float64[ne+1]; Utraj
    float64[N+1, ne+1] the whole stored trajectory (row n = u^n, N >= n0+m-1); Z float64[m, ne+1] the adjoint states of
    the chunk IN THE ORDER OF THE SWEEP: row i belongs to step n0+m-1-i; ``coef``: m triples (alpha, beta0, beta1), the
    BDF coefficients of step row i (host numbers: they travel in the launch's arguments); phi float64[N, R] the whole
    table of the forward loop (row n-1 = phi(t_n)), needed for "f" only.  ``want``: which of "a", "c", "rho", "f" to
    compute; a table left out is neither computed nor stored, and ``want=()`` is allowed with the end gradients.
    ``Brows`` (float64[m, ne+1], the adjoint right-hand sides of the chunk, in Z's order) asks for the end gradients
    too: with ``band_ends`` float64[2, 2] = {sub[0], sup[ne-1]} of two step matrices, ``band_rows`` (m values 0 / 1:
    which of the two is step row i's; ``None``: 0) and ``end_kinds``, rows n0 .. n0+m-1 of "g" float64[N+1, 2] and
    "kappa" float64[2] are written by the same launch.  ``accumulate``: every sum (the tables and "kappa") continues
    from what ``out`` holds instead of from 0 -- a sweep gives the same bits however it is cut into chunks -- and then
    ``out`` must hold every wanted buffer.  Returns a dict: "a", "c", "rho" -> float64[ne, nquad], "f" ->
    float64[R, ne, nquad], "g", "kappa".  ``out``: a dict of buffers to write into, by those keys ("g" is never
    allocated here: its other rows are the caller's).  No synchronisation and no copy; every value is computed in a
    fixed order (bitwise reproducible)."""
    lib = _capi.load()
    ne, nquad, n0, m, R, kinds, ins, res = _chunk_sens(TS_SENS_TABLES, 1, 0, (2, 2), x, Utraj, Z, n0, nquad, want, {},
                                                       phi, Brows, band_ends, end_kinds, accumulate, out)
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64))
    if coef.shape != (m, 3) or not np.all(np.isfinite(coef)):
        raise ValueError(f"coef must be m = {m} finite triples (alpha, beta0, beta1), got shape {list(coef.shape)}")
    (inv_dt,) = _finite(inv_dt=inv_dt)
    rows = [0] * m if band_rows is None or Brows is None else [int(r) for r in band_rows]
    if len(rows) != m or any(r not in (0, 1) for r in rows):
        raise ValueError(f"band_rows must be m = {m} values 0 or 1, got {band_rows!r}")
    rc = lib.lssvr_transient_sensitivity(_ptr(x), ne, nquad, _ptr(Utraj), _ptr(Z), n0, m, inv_dt,
                                         coef.ctypes.data_as(_capi._c_hd), _ptr(ins.get("phi")), R,
                                         *(_ptr(res.get(k)) for k in TS_SENS_TABLES), int(bool(accumulate)),
                                         _ptr(Brows), _ptr(band_ends), sum(r << i for i, r in enumerate(rows)), *kinds,
                                         _ptr(res.get("g")), _ptr(res.get("kappa")), _stream(stream))
    _capi.check(rc, "lssvr_transient_sensitivity")
    return res


# ---- adjoint sensitivities of the semilinear BDF loop --------------------------------------------
TS_NL_SENS_TABLES = TS_SENS_TABLES + ("q",)     # "q": d/d q_quad, the tables of g(x, u)


def ts_nl_sensitivity(x, Utraj, Z, n0, coef, inv_dt, nquad, kind, nterm, *, q_tabs=None, want=TS_NL_SENS_TABLES,
                      phi=None, Brows=None, band_ends=None, end_kinds=(END_DIRICHLET, END_DIRICHLET), accumulate=False,
                      out=None, stream=None):
    """``lssvr_semilinear_transient_sensitivity``: :func:`ts_sensitivity` for the semilinear loop of
    :func:`ts_nl_assemble` with g(x, u) of ``kind`` ("poly" / ``NL_POLY``, "exp" / ``NL_EXP``) and ``nterm`` tables, in
    ONE launch per chunk.  Utraj holds the CONVERGED states u^n and Z the adjoint states of the Jacobians J_n AT u^n
    (:func:`ts_nl_adjoint_step` and one :func:`tridiag_bc_solve_multi` per level).  ``want`` names any of "a", "c",
    "rho", "f" -- bit for bit the values of :func:`ts_sensitivity` -- and "q" -- float64[nterm, ne, nquad] = dJ/dq_k at
    every quadrature point, summed over the chunk's levels; "q" of "poly" has q[1] == c bit for bit, and q[0] == -f[0]
    where phi is 1.  ``q_tabs`` float64[nterm, ne, nquad], the tables :func:`ts_nl_assemble` took, is read for "exp"
    with "q" only and must be given then.  ``band_ends`` float64[m, 2]: every level has its own matrix, row i =
    {off[0], off[ne-1]} of step row i's J_n (there are no ``band_rows``).  Everything else -- the order of the rows,
    ``coef``, ``phi``, ``Brows``, ``end_kinds``, ``accumulate``, ``out`` and the result -- as for
    :func:`ts_sensitivity`.  No synchronisation and no copy; bitwise reproducible."""
    lib = _capi.load()
    kind, nterm = nl_kind(kind, nterm)
    ne, nquad, n0, m, R, kinds, ins, res = _chunk_sens(TS_NL_SENS_TABLES, 1, 0, (-1, 2), x, Utraj, Z, n0, nquad, want,
                                                       {}, phi, Brows, band_ends, end_kinds, accumulate, out,
                                                       leading={"q": nterm})
    if q_tabs is not None:
        _dev(q_tabs, "q_tabs")
        if tuple(q_tabs.shape) != (nterm, ne, nquad):
            raise ValueError(f"q_tabs must be [nterm, ne, nquad] = [{nterm}, {ne}, {nquad}], got {list(q_tabs.shape)}")
        _no_alias("the outputs must be distinct and none of them an input", res.values(), (q_tabs,))
        _same_device(x, q_tabs=q_tabs)
    elif kind == NL_EXP and "q" in res:
        raise ValueError("kind 'exp' needs q_tabs: dJ/dq_k depends on q_0 and q_1")
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64))
    if coef.shape != (m, 3) or not np.all(np.isfinite(coef)):
        raise ValueError(f"coef must be m = {m} finite triples (alpha, beta0, beta1), got shape {list(coef.shape)}")
    (inv_dt,) = _finite(inv_dt=inv_dt)
    rc = lib.lssvr_semilinear_transient_sensitivity(_ptr(x), ne, nquad, _ptr(Utraj), _ptr(Z), n0, m, inv_dt,
                                                    coef.ctypes.data_as(_capi._c_hd), _ptr(ins.get("phi")), R,
                                                    _ptr(q_tabs), kind, nterm,
                                                    *(_ptr(res.get(k)) for k in TS_NL_SENS_TABLES),
                                                    int(bool(accumulate)), _ptr(Brows), _ptr(band_ends), *kinds,
                                                    _ptr(res.get("g")), _ptr(res.get("kappa")), _stream(stream))
    _capi.check(rc, "lssvr_semilinear_transient_sensitivity")
    return res


def ts_nl_adjoint_step(x, u, cs_quad, kind, q_quad, mdiag, moff, U0, U1, loads, phi, beta0, beta1, inv_dt, *,
                       a_quad=None, out=None, stream=None):
    """``lssvr_semilinear_adjoint_step``: everything one level of the backward sweep of the semilinear BDF loop needs
    before its solve, in ONE launch -- the bands of the Jacobian J_n = K + M(cs + g_u(., u_h)) AT ``u`` = u^n, bit for
    bit "diag" and "off" of :func:`ts_nl_assemble` there (whose right-hand side is not formed); the adjoint right-hand
    side "B" float64[1, ne+1], bit for bit :func:`ts_rhs` of (mdiag, moff, U0 = lambda^{n+1}, U1 = lambda^{n+2}, loads,
    phi, beta0, beta1, inv_dt) with one case; and "band_ends" float64[2] = {off[0], off[ne-1]}, the level's row of
    :func:`ts_nl_sensitivity`'s ``band_ends``.  ``x``, ``u``, ``cs_quad``, ``kind``, ``q_quad``, ``a_quad`` as for
    :func:`ts_nl_assemble`; U0, U1 float64[1, ne+1] (``beta1 == 0`` reads no U1, ``None`` allowed), loads
    float64[R, ne+1], phi float64[1, R].  ``out``: a dict of buffers to write into, by those four keys (a missing one is
    allocated); none of them may be an input.  Returns that dict.  No synchronisation and no copy; bitwise
    reproducible."""
    lib = _capi.load()
    for nm, t in (("x", x), ("u", u), ("cs_quad", cs_quad), ("q_quad", q_quad), ("mdiag", mdiag), ("moff", moff),
                  ("U0", U0), ("loads", loads), ("phi", phi)):
        _dev(t, nm)
    ne = _nodes(x, "x")
    _nodal(ne, u=u)
    if cs_quad.dim() != 2 or cs_quad.shape[0] != ne or not 1 <= cs_quad.shape[1] <= 5:
        raise ValueError(f"cs_quad must be [ne, nquad] = [{ne}, 1 .. 5], got {list(cs_quad.shape)}")
    nquad = int(cs_quad.shape[1])
    if q_quad.dim() != 3 or tuple(q_quad.shape[1:]) != (ne, nquad):
        raise ValueError(f"q_quad must be [nterm, {ne}, {nquad}], got {list(q_quad.shape)}")
    kind, nterm = nl_kind(kind, q_quad.shape[0])
    if a_quad is not None:
        _dev(a_quad, "a_quad")
        if a_quad.shape != cs_quad.shape:
            raise ValueError(f"a_quad must have the shape of cs_quad {list(cs_quad.shape)}, got {list(a_quad.shape)}")
    beta0, beta1, inv_dt = _finite(beta0=beta0, beta1=beta1, inv_dt=inv_dt)
    _band_pair("band lengths must be ne+1, ne (mdiag, moff)", mdiag, moff, ne)
    out = {} if out is None else out
    nc, R, B = _bdf_state(ne, x, U0, U1, loads, phi, beta1, out.get("B"))
    if nc != 1:
        raise ValueError(f"U0 must be [1, ne+1]: the backward step has one case, got {list(U0.shape)}")
    res = {k: _out(out.get(k), f"out[{k!r}]", shape, x) for k, shape in (("diag", (ne + 1,)), ("off", (ne,)),
                                                                          ("band_ends", (2,)))}
    res["B"] = B
    ins = (x, u, cs_quad, q_quad, a_quad, mdiag, moff, U0, U1, loads, phi)
    _no_alias("diag, off, B and band_ends must be distinct and none of them an input", res.values(), ins)
    _same_device(x, u=u, cs_quad=cs_quad, q_quad=q_quad, a_quad=a_quad, mdiag=mdiag, moff=moff, U0=U0, loads=loads,
                 phi=phi, **({} if U1 is None else {"U1": U1}))
    rc = lib.lssvr_semilinear_adjoint_step(_ptr(x), _ptr(u), _ptr(a_quad), _ptr(cs_quad), _ptr(q_quad), ne, nquad, kind,
                                           nterm, _ptr(mdiag), _ptr(moff), _ptr(U0), _ptr(U1), _ptr(loads), _ptr(phi),
                                           R, beta0, beta1, inv_dt, _ptr(res["diag"]), _ptr(res["off"]), _ptr(B),
                                           _ptr(res["band_ends"]), _stream(stream))
    _capi.check(rc, "lssvr_semilinear_adjoint_step")
    return res


# ---- adjoint sensitivities of the Newmark loop ---------------------------------------------------
NM_SENS_TABLES = ("a", "c", "rho", "d", "f")    # d/d a_quad, c_quad, rho_quad, d_quad, f_quad[r]: the keys of ``want``
NM_SENS_CHUNK = 8                               # most levels of one launch


def newmark_adjoint_advance(lam, Vbar, Abar, mdiag, moff, ddiag, doff, dt, beta, gamma, *, P=None, want_u=False,
                            want_b=True, out=None, stream=None):
    """``lssvr_newmark_adjoint_advance``: ONE launch between two backward solves of the Newmark adjoint.  From lam =
    lambda^{n+1}, the bars (Vbar, Abar) of level n+1 and the row P = p_n (``None``: zero), all float64[ne+1] on the
    device, with the mass bands (mdiag[ne+1], moff[ne]) and the damping bands (ddiag, doff; both ``None``: d = 0):
    as = Abar + gamma dt Vbar, ut = c_m M_rho lam + c_d M_d lam - c_m as, vt = Vbar - M_d lam, then "u" = P + ut,
    "v" = dt ut + vt, "a" = c_u2 ut + c_v1 vt, the bars of level n, and "b" = u + c_m (a + gamma dt v), the next
    right-hand side.  ``lam=None`` is the first call of a sweep: "b" = P + c_m (Abar + gamma dt Vbar) alone (the bands
    may be ``None``).  ``want_u``: write "u" (the last call of a sweep); ``want_b=False``: no "b".  Returns a dict by
    those keys; ``out``: a dict of buffers to write into.  No output may be an input or another output.  No
    synchronisation and no copy; every sum in a fixed order (bitwise reproducible)."""
    lib = _capi.load()
    for nm, t in (("Vbar", Vbar), ("Abar", Abar)):
        _dev(t, nm)
    ne = _nodes(Vbar, "Vbar")
    dt, beta, gamma = _finite(dt=dt, beta=beta, gamma=gamma)
    if not (dt > 0.0 and beta > 0.0 and gamma > 0.0):
        raise ValueError(f"dt, beta and gamma must be > 0, got {dt!r}, {beta!r}, {gamma!r}")
    ins = {"Abar": Abar}
    if P is not None:
        _dev(P, "P")
        ins["P"] = P
    if lam is None:
        if want_u or not want_b:
            raise ValueError("lam=None (the first call of a sweep) writes 'b' alone: want_u=False, want_b=True")
        mdiag = moff = ddiag = doff = None
        keys = ("b",)
    else:
        _dev(lam, "lam")
        ins["lam"] = lam
        if (ddiag is None) != (doff is None):
            raise ValueError("ddiag and doff go together: both or neither")
        for nm, t in (("mdiag", mdiag), ("moff", moff)):
            if t is None:
                raise ValueError(f"{nm} is needed with lam")
            _dev(t, nm)
        _band_pair(f"band lengths must be ne+1, ne = {ne + 1}, {ne} (mdiag, moff)", mdiag, moff, ne)
        ins.update(mdiag=mdiag, moff=moff)
        if ddiag is not None:
            for nm, t in (("ddiag", ddiag), ("doff", doff)):
                _dev(t, nm)
            _band_pair(f"band lengths must be ne+1, ne = {ne + 1}, {ne} (ddiag, doff)", ddiag, doff, ne)
            ins.update(ddiag=ddiag, doff=doff)
        keys = ("v", "a") + (("u",) if want_u else ()) + (("b",) if want_b else ())
    _nodal(ne, **{k: ins[k] for k in ("Abar", "P", "lam") if k in ins})
    out = {} if out is None else out
    res = {k: _out(out.get(k), f"out[{k!r}]", (ne + 1,), Vbar) for k in keys}
    _no_alias("the outputs must be distinct and none of them an input", res.values(), (Vbar, *ins.values()))
    _same_device(Vbar, **ins)
    rc = lib.lssvr_newmark_adjoint_advance(_ptr(lam), _ptr(Vbar), _ptr(Abar), _ptr(P), _ptr(mdiag), _ptr(moff),
                                           _ptr(ddiag), _ptr(doff), ne, dt, beta, gamma,
                                           *(_ptr(res.get(k)) for k in ("v", "a", "u", "b")), _stream(stream))
    _capi.check(rc, "lssvr_newmark_adjoint_advance")
    return res


def newmark_sensitivity(x, Utraj, Z, n0, nquad=2, *, want=NM_SENS_TABLES, Vtraj=None, Atraj=None, phi=None, Brows=None,
                        band_ends=None, end_kinds=(END_DIRICHLET, END_DIRICHLET), accumulate=False, out=None,
                        stream=None):
    """``lssvr_newmark_sensitivity``: the gradients of J with respect to the tables of the Newmark loop of
    :func:`wave_advance`, summed over a CHUNK of m <= 8 consecutive levels n0 .. n0+m-1 (n0 >= 0), in ONE launch.
    x float64[ne+1]; Utraj (and Vtraj for "d", Atraj for "rho") float64[N+1, ne+1] the whole stored trajectories (row
    n = u^n, v^n, acc^n; N >= n0+m-1); Z float64[m, ne+1] the adjoint states of the chunk IN THE ORDER OF THE SWEEP: row
    i belongs to level n0+m-1-i; phi float64[N+1, R] (row n = phi(t_n)), needed for "f" only.  ``want``: which of "a",
    "c", "rho", "d", "f" to compute; a table left out is neither computed nor stored, and ``want=()`` is allowed with
    the end gradients.  ``Brows`` (float64[m, ne+1], the right-hand sides of the chunk's solves, in Z's order) asks for
    the end gradients too: with ``band_ends`` float64[2] = {sub[0], sup[ne-1]} of the solves' matrix and
    ``end_kinds``, rows n0 .. n0+m-1 of "g" float64[N+1, 2] and "kappa" float64[2] are written by the same launch.
    ``accumulate``: every sum (the tables and "kappa") continues from what ``out`` holds instead of from 0 -- a sweep
    gives the same bits however it is cut into chunks -- and then ``out`` must hold every wanted buffer.  Returns a
    dict: "a", "c", "rho", "d" -> float64[ne, nquad], "f" -> float64[R, ne, nquad], "g", "kappa".  ``out``: a dict of
    buffers to write into, by those keys ("g" is never allocated here: its other rows are the caller's).  No
    synchronisation and no copy; every value is computed in a fixed order (bitwise reproducible)."""
    lib = _capi.load()
    ne, nquad, n0, m, R, kinds, ins, res = _chunk_sens(NM_SENS_TABLES, 0, 1, (2,), x, Utraj, Z, n0, nquad, want,
                                                       {"Vtraj": ("d", Vtraj), "Atraj": ("rho", Atraj)}, phi, Brows,
                                                       band_ends, end_kinds, accumulate, out)
    rc = lib.lssvr_newmark_sensitivity(_ptr(x), ne, nquad, _ptr(Utraj), _ptr(ins.get("Vtraj")), _ptr(ins.get("Atraj")),
                                       _ptr(Z), n0, m, _ptr(ins.get("phi")), R,
                                       *(_ptr(res.get(k)) for k in NM_SENS_TABLES), int(bool(accumulate)), _ptr(Brows),
                                       _ptr(band_ends), *kinds, _ptr(res.get("g")), _ptr(res.get("kappa")),
                                       _stream(stream))
    _capi.check(rc, "lssvr_newmark_sensitivity")
    return res


def fp64_probe(blocks=4096, iters=4096, use_mfma=False, *, device="cuda:0", reps=5):
    """Measured FP64 FMA (use_mfma False), v_mfma_f64_16x16x4 (True / 1) or v_mfma_f64_4x4x4_4b (3)
    rate in TFLOP/s -- what the roofline's 78.6 TFLOP/s peak sustains in a pure loop."""
    lib = _capi.load()
    out = torch.empty(blocks * 256, dtype=torch.float64, device=device)
    st = _stream(None)
    _capi.check(lib.lssvr_fp64_probe(_ptr(out), blocks, iters, int(use_mfma), st), "probe")
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        e0.record()
        _capi.check(lib.lssvr_fp64_probe(_ptr(out), blocks, iters, int(use_mfma), st), "probe")
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3)
    if int(use_mfma) == 3:
        flops = 8.0 * 512.0 * iters * blocks * 4      # 8 MFMAs/iter/wave, 4 blocks x 4x4x4 x 2 flop
    elif use_mfma:
        flops = 4.0 * 2048.0 * iters * blocks * 4     # 4 MFMAs/iter/wave, 16x16x4x2 flop, 4 waves/block
    else:
        flops = 2.0 * 8.0 * iters * blocks * 256
    return flops / best / 1e12
