"""GPU: the flux prefix-scan Dirichlet solve (csrc/flux_solve.hip) against the blocked long-double sums of
tests/flux_rules.py, on meshes graded over six orders of magnitude and coefficients that jump from element to element,
at the sizes where the scan changes level -- single shard and sharded (all shards on the one GPU, no processes).

The bar everywhere: |u[m] - u_ref[m]| <= BAR_C * EPS * scale_m (flux_rules)."""
import numpy as np
import pytest
import torch

import flux_rules as fr

pytestmark = pytest.mark.gpu

LD = np.longdouble
U0, U1 = fr.U0, fr.U1


def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a), device=dev)          # a copy: the shared cases are read-only


def _bits(t):
    return t.detach().cpu().numpy().view(np.int64)


@pytest.mark.parametrize("ne", fr.SIZES)
@pytest.mark.parametrize("name", fr.NAMES)
def test_flux_solve_vs_reference(dev, note, name, ne):
    """lssvr_p1_flux_solve on every problem at every size of the matrix.  load[0] and load[ne] are NaN: the first must
    not count, the last is never read."""
    from hybrid_fem_lssvr_amd import ops
    kloc, load, u_ref, scale = fr.case(ne, name)
    u = ops.p1_flux_solve(_t(kloc, dev), _t(load, dev), U0, U1).cpu().numpy()
    r = fr.ratio(u, u_ref, scale)
    note("%s ne=%d err/(eps*scale)" % (name, ne), r, fr.BAR_C)
    assert u.shape == (ne + 1,) and not np.isnan(u).any()
    assert u[0] == U0 and u[ne] == U1
    assert r <= fr.BAR_C
    if name == "zero_load":
        rz = fr.ratio(u, fr.zero_load_formula(kloc, U0, U1), scale)
        note("%s ne=%d err/(eps*scale) vs closed formula" % (name, ne), rz, fr.BAR_C)
        assert rz <= fr.BAR_C


@pytest.mark.parametrize("ne,name,kind", fr.shard_matrix())
def test_flux_shards_vs_reference(dev, note, ne, name, kind):
    """lssvr_p1_flux_aggregate per shard, the aggregates combined on the device as distributed.solve_fem_sharded
    combines them, lssvr_p1_flux_finish per shard.  The load at every shard's first node is x 1e3, so a later shard
    that dropped its load[0] would stand far above the bar; the last entry of every shard's load is NaN (never
    read).  The tile-edge cut lists do not exist at ne = 9."""
    from hybrid_fem_lssvr_amd import ops
    from hybrid_fem_lssvr_amd.distributed import combine_flux
    kloc, load, u_ref, scale = fr.case(ne, name, fr.shard_boost(ne))
    bounds = (0,) + fr.cuts(ne, kind) + (ne,)
    shards, worst_agg = [], 0.0
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        k_s = kloc[s0:s1].copy()
        l_s = load[s0:s1 + 1].copy()
        want = fr.shard_aggregate(k_s, l_s, s0 == 0)
        absum = fr.shard_aggregate_abs(k_s, l_s, s0 == 0)
        l_s[-1] = np.nan
        k_d, l_d = _t(k_s, dev), _t(l_s, dev)
        agg, work = ops.p1_flux_aggregate(k_d, l_d, first_global=(s0 == 0))
        shards.append((s0, s1, k_d, l_d, agg, work))
        got = agg.cpu().numpy()
        assert got.shape == (3,) and not np.isnan(got).any()
        for g, w, sc in zip(got, want, absum):
            err = abs(LD(g) - w)
            if sc > 0:
                worst_agg = max(worst_agg, float(err / (fr.EPS * sc)))
            assert err <= fr.BAR_C * fr.EPS * sc, (s0, s1)
    allagg = torch.stack([s[4] for s in shards])
    prefixes = []
    grand = torch.zeros(3, dtype=torch.float64, device=dev)
    for r in range(len(shards)):
        prefixes.append(grand.clone())
        grand = combine_flux(grand, allagg[r])
    worst = 0.0
    for (s0, s1, k_d, l_d, agg, work), prefix in zip(shards, prefixes):
        u = ops.p1_flux_finish(k_d, l_d, work, first_global=(s0 == 0), last_global=(s1 == ne), prefix=prefix,
                               grand=grand, u0=U0, u1=U1).cpu().numpy()
        assert u.shape == (s1 - s0 + 1,) and not np.isnan(u).any()
        # the node two shards share is written by both, each within the bar (they associate differently)
        r = fr.ratio(u, u_ref[s0:s1 + 1], scale[s0:s1 + 1])
        worst = max(worst, r)
        assert r <= fr.BAR_C, (s0, s1, r)
        if s0 == 0:
            assert u[0] == U0
        if s1 == ne:
            assert u[-1] == U1
        else:
            assert u[-1] != U1          # a middle shard's last node is computed, not overwritten
    note("%s ne=%d %s shard aggregates err/(eps*sum|terms|)" % (name, ne, kind), worst_agg, fr.BAR_C)
    note("%s ne=%d %s shards err/(eps*scale)" % (name, ne, kind), worst, fr.BAR_C)


def test_flux_power_of_two_scaling_is_exact(dev, note):
    """Every operation of the scan commutes with a scaling by a power of two: k and load x 2^10 leave u bit-identical,
    load, u0, u1 x 2^-7 scale u by 2^-7 bit for bit.  A stray unscaled constant or a mis-paired operand breaks it."""
    from hybrid_fem_lssvr_amd import ops
    ne = 2049
    kloc, load, u_ref, scale = fr.case(ne, "layered")
    u = ops.p1_flux_solve(_t(kloc, dev), _t(load, dev), U0, U1)
    note("layered ne=%d err/(eps*scale)" % ne, fr.ratio(u.cpu().numpy(), u_ref, scale), fr.BAR_C)
    a = ops.p1_flux_solve(_t(kloc * 2.0 ** 10, dev), _t(load * 2.0 ** 10, dev), U0, U1)
    assert np.array_equal(_bits(a), _bits(u))
    b = ops.p1_flux_solve(_t(kloc, dev), _t(load * 2.0 ** -7, dev), U0 * 2.0 ** -7, U1 * 2.0 ** -7)
    assert np.array_equal(_bits(b), _bits(u * 2.0 ** -7))
    assert not torch.isnan(u).any()


GUARD = 64
SENTINEL = -7.25


def _guarded(n, dev):
    """A float64[n] view with GUARD sentinel doubles before and behind it, and the allocation it lives in."""
    big = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    return big[GUARD:GUARD + n], big


def _guards_intact(big):
    g = big.cpu().numpy()
    return bool(np.all(g[:GUARD] == SENTINEL) and np.all(g[-GUARD:] == SENTINEL))


@pytest.mark.parametrize("ne", [1025, 263170])
def test_flux_buffers(dev, note, ne):
    """work of exactly lssvr_p1_flux_work_bytes(ne) and out of exactly ne+1 doubles inside larger allocations keep the
    sentinels around them; the inputs are not written; the call is reproducible bit for bit; a work buffer that last
    served 263170 elements gives the bits of a fresh one (no stale tile aggregate is read)."""
    from hybrid_fem_lssvr_amd import _capi, ops
    lib = _capi.load()
    kloc, load, u_ref, scale = fr.case(ne, "layered")
    k_d, l_d = _t(kloc, dev), _t(load, dev)
    nbytes = lib.lssvr_p1_flux_work_bytes(ne)
    assert nbytes % 8 == 0
    work, work_big = _guarded(nbytes // 8, dev)
    out, out_big = _guarded(ne + 1, dev)
    u = ops.p1_flux_solve(k_d, l_d, U0, U1, out=out, work=work)
    assert u.data_ptr() == out.data_ptr()
    first = _bits(u).copy()
    assert _guards_intact(work_big) and _guards_intact(out_big)
    note("layered ne=%d err/(eps*scale)" % ne, fr.ratio(u.cpu().numpy(), u_ref, scale), fr.BAR_C)
    assert fr.ratio(u.cpu().numpy(), u_ref, scale) <= fr.BAR_C
    assert np.array_equal(_bits(k_d), kloc.view(np.int64)) and np.array_equal(_bits(l_d), load.view(np.int64))
    again = ops.p1_flux_solve(k_d, l_d, U0, U1, out=out, work=work)
    assert np.array_equal(_bits(again), first)
    assert _guards_intact(work_big) and _guards_intact(out_big)
    # a buffer that last served the largest size, reused for this one
    big_ne = 263170
    kb, lb = fr.case(big_ne, "layered")[:2]
    used = torch.empty(lib.lssvr_p1_flux_work_bytes(big_ne) // 8, dtype=torch.float64, device=dev)
    ops.p1_flux_solve(_t(kb, dev), _t(lb, dev), U0, U1, work=used)
    ptr = used.data_ptr()
    reused = ops.p1_flux_solve(k_d, l_d, U0, U1, work=used)
    assert used.data_ptr() == ptr
    assert np.array_equal(_bits(reused), first)


class _NoLaunch:
    """The loaded library with the flux launches taken out: a wrapper that reaches one has not rejected its
    arguments."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in ("lssvr_p1_flux_solve", "lssvr_p1_flux_aggregate", "lssvr_p1_flux_finish"):
            raise AssertionError(name + " reached with arguments that had to be rejected")
        return getattr(self._lib, name)


def test_flux_wrappers_reject(dev, monkeypatch):
    """Wrong lengths, host or float32 buffers and a work buffer shorter than lssvr_p1_flux_work_bytes(ne) are
    refused by the wrappers before anything is launched: in lssvr_p1_flux_finish a short or host ``work`` would be an
    out-of-bounds device read."""
    from hybrid_fem_lssvr_amd import _capi, ops
    lib = _capi.load()
    ne = 1025
    kloc, load = fr.problems(ne, "layered")
    k_d, l_d = _t(kloc, dev), _t(load, dev)
    agg, work = ops.p1_flux_aggregate(k_d, l_d, first_global=True)          # a good buffer, before the launches go
    torch.cuda.synchronize()
    monkeypatch.setattr(_capi, "load", lambda: _NoLaunch(lib))
    with pytest.raises(ValueError):
        ops.p1_flux_solve(k_d, l_d[:ne], U0, U1)
    with pytest.raises(ValueError):
        ops.p1_flux_solve(k_d, _t(np.zeros(ne + 2), dev), U0, U1)
    with pytest.raises(ValueError):
        ops.p1_flux_aggregate(k_d, l_d[:ne], first_global=True)
    kw = dict(first_global=True, last_global=True, u0=U0, u1=U1)
    nwork = lib.lssvr_p1_flux_work_bytes(ne) // 8
    with pytest.raises(ValueError):
        ops.p1_flux_finish(k_d, l_d[:ne], work, **kw)
    with pytest.raises(ValueError):
        ops.p1_flux_finish(k_d, l_d, work[:nwork - 1], **kw)
    with pytest.raises(ValueError):
        ops.p1_flux_finish(k_d, l_d, work[:nwork][::2], **kw)                  # not contiguous
    with pytest.raises(ValueError):
        ops.p1_flux_finish(k_d, l_d, work, out=torch.empty(ne, dtype=torch.float64, device=dev), **kw)
    with pytest.raises(ValueError):
        ops.p1_flux_finish(k_d, l_d, work, prefix=agg[:2], **kw)
    for bad in (work.cpu(), None, work.to(torch.float32)):
        with pytest.raises((RuntimeError, TypeError)):
            ops.p1_flux_finish(k_d, l_d, bad, **kw)
    with pytest.raises(RuntimeError):
        ops.p1_flux_finish(k_d.cpu(), l_d, work, **kw)
    with pytest.raises(TypeError):
        ops.p1_flux_finish(k_d, l_d.to(torch.float32), work, **kw)
    with pytest.raises(AssertionError):                                      # the guard itself: good arguments do launch
        ops.p1_flux_finish(k_d, l_d, work, **kw)
