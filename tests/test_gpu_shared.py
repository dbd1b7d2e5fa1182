"""GPU tests of the shared-operator shortcut for uniform meshes (lssvr_enhance_shared).
Checked against the general per-element kernel, the float64 oracle and the reference's golden
output on the same uniform mesh; the bar is north_star's 1e-10 (measured ~1e-13 .. 1e-12), not
the 1e-13 of the general path."""
import numpy as np
import pytest

from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", [(24, 9, 16, 1e4, -1.0, 1.0), (8, 5, 5, 1e4, -1.0, 1.0),
                                 (24, 8, 12, 1e4, -1.0, 1.0), (4, 12, 12, 1e6, -1.0, 1.0),
                                 (4096, 9, 16, 1e4, -1.0, 1.0), (3000, 16, 24, 1e3, -125.0, 125.0),
                                 (24, 33, 64, 1e4, -1.0, 1.0), (2000, 33, 64, 1e4, -1.0, 1.0),
                                 (1500, 24, 48, 1e5, -60.0, 65.0)])
def test_shared_matches_general_and_oracle(dev, cfg):
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    ne, M, n, gamma, lo, hi = cfg
    nodes = np.linspace(lo, hi, ne + 1)
    values = orc.fem_p1_solve(nodes) if lo == -1.0 else np.sin(np.pi * nodes)
    gen = pkg.enhance_elements(nodes, values, M, gamma, n_colloc=n, global_domain=(lo, hi))
    sh = pkg.enhance_elements(nodes, values, M, gamma, n_colloc=n, global_domain=(lo, hi),
                              solver=ops.SOLVER_SHARED)
    Wg, Ws = gen.W.cpu().numpy(), sh.W.cpu().numpy()
    assert sh.n_fallback == 0
    assert orc.rel_l2_coef(Ws, Wg).max() <= 1e-11
    Wo = orc.enhance_all_vec(nodes, values, M, gamma, n, global_domain=(lo, hi))
    assert orc.rel_l2_coef(Ws, Wo).max() <= 1e-11


def test_shared_golden_reference(dev, golden):
    """Against the reference's own SLSQP output (fixture G3: 24 elements, M=9, n=16)."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    g = golden("G3_ne24_M9_n16")
    ne, M, n, gamma = int(g["ne"]), int(g["M"]), int(g["n"]), float(g["gamma"])
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    values = orc.fem_p1_solve(nodes)
    values[g["elements"]] = g["values_sel"][:, 0]
    values[g["elements"] + 1] = g["values_sel"][:, 1]
    sh = pkg.enhance_elements(nodes, values, M, gamma, n_colloc=n, solver=ops.SOLVER_SHARED)
    W = sh.W.cpu().numpy()[g["elements"]]
    assert orc.rel_l2_coef(W, g["coef_ref"]).max() <= 1e-10
    assert orc.rel_l2_coef(W, g["coef_truth"]).max() <= 1e-11


def test_shared_rejects_nonuniform_mesh(dev):
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    nodes = np.linspace(-1, 1, 33)
    nodes[7] += 1e-6
    with pytest.raises(ValueError):
        pkg.enhance_elements(nodes, np.sin(np.pi * nodes), 9, 1e4, n_colloc=16, solver=ops.SOLVER_SHARED)


def test_shared_tabulated_rhs_and_full_size(dev):
    """rhs as an array + BASELINE config 2's size on the wide domain: sampled elements against the oracle,
    all elements against the general kernel."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    ne, M, n = 100008, 9, 16
    lo, hi = -4167.0, 4167.0
    nodes = np.arange(ne + 1, dtype=np.float64) * ((hi - lo) / ne) + lo
    nodes[-1] = hi
    values = np.sin(np.pi * nodes)
    values[0] = values[-1] = 0.0
    x = torch.as_tensor(nodes, device=dev)
    u = torch.as_tensor(values, device=dev)
    op = ops.build_shared_operator(1.0 / 12.0, M, 1e4, n, device=dev)
    W1, st1 = ops.enhance_shared(x, u, op, M, n, global_domain=(lo, hi))
    xc = ops.colloc_points(x, n).cpu().numpy()
    f = torch.as_tensor((np.pi ** 2) * np.sin(np.pi * xc), device=dev)
    W2, st2 = ops.enhance_shared(x, u, op, M, n, rhs_values=f, global_domain=(lo, hi))
    torch.cuda.synchronize()
    assert int(st1.sum()) == 0 and int(st2.sum()) == 0
    W1h, W2h = W1.cpu().numpy(), W2.cpu().numpy()
    sel = np.unique(np.linspace(0, ne - 1, 40).astype(np.int64))
    Wo = np.array([orc.solve_primal_kkt(orc.element_system(
        nodes[i], nodes[i + 1], *orc.boundary_values(int(i), ne, nodes[i], nodes[i + 1], values[i],
                                                     values[i + 1], (lo, hi)), M, 1e4, n)) for i in sel])
    assert orc.rel_l2_coef(W1h[sel], Wo).max() <= 1e-10
    assert orc.rel_l2_coef(W2h[sel], Wo).max() <= 1e-10
    Wg, _ = ops.enhance(x, u, M, 1e4, n, global_domain=(lo, hi))
    assert orc.rel_l2_coef(W1h, Wg.cpu().numpy()).max() <= 1e-10


# ---------------------------------------------------------------------------------------------------------------------
# The kernel across its degrees, tails, rhs paths and fallback, against tests/shared_rules.py: a numpy restatement of
# the same operation, with bars of MARGIN x the restatement's own distance from the float64 oracle (floor 1e-13; read
# on the CPU, tests/test_shared_cpu.py) or the existing 1e-11 -- none read from the kernel.  Everything goes through
# ops.build_shared_operator / ops.enhance_shared; inputs are tiny (default: 130 elements of [-1, 1], two waves and a
# tail of two).
# ---------------------------------------------------------------------------------------------------------------------
import functools                                     # noqa: E402

import shared_rules as sr                            # noqa: E402

GD = (sr.LO, sr.HI)
CANARY, ICANARY, GUARD = -1234.5, -7, 64


def _t(dev, a):
    import torch
    return torch.as_tensor(np.array(a, order="C"), device=dev)              # (a copy: cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def _op(dev, h0, M, n, gamma=sr.GAMMA):
    from hybrid_fem_lssvr_amd import ops
    return ops.build_shared_operator(h0, M, gamma, n, device=dev)


def _shared(dev, nodes, values, M, n, f=None, pm=False, h0=None, gamma=sr.GAMMA, global_domain=GD, **kw):
    """One launch of ops.enhance_shared -> (W, status) as numpy; ``f`` float64[ne, n] is passed element-major, or
    transposed as the point-major table with ``pm``."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    op = _op(dev, sr.spacing(nodes) if h0 is None else h0, M, n, gamma)
    if f is not None:
        kw.update(rhs_values=_t(dev, f.T if pm else f), point_major=pm)
    W, st = ops.enhance_shared(_t(dev, nodes), _t(dev, values), op, M, n, global_domain=global_domain, **kw)
    torch.cuda.synchronize()
    return W.cpu().numpy().reshape(-1, M), st.cpu().numpy()


def _general(dev, nodes, values, M, n, gamma=sr.GAMMA, global_domain=GD, **kw):
    import torch
    from hybrid_fem_lssvr_amd import ops
    W, st = ops.enhance(_t(dev, nodes), _t(dev, values), M, gamma, n, global_domain=global_domain, **kw)
    torch.cuda.synchronize()
    return W.cpu().numpy(), st.cpu().numpy()


def _guarded(dev, ne, M):
    """(Wbuf, W, sbuf, status): ``W`` and ``status`` are leading slices of canary-filled buffers with GUARD entries
    behind them."""
    import torch
    Wbuf = torch.full((ne * M + GUARD,), CANARY, dtype=torch.float64, device=dev)
    sbuf = torch.full((ne + GUARD,), ICANARY, dtype=torch.int32, device=dev)
    return Wbuf, Wbuf[:ne * M], sbuf, sbuf[:ne]


def _guards_intact(Wbuf, sbuf, ne, M):
    return bool((Wbuf[ne * M:] == CANARY).all()) and bool((sbuf[ne:] == ICANARY).all())


# Measured on the MI355X, largest over M = 2..33 (sine and tables alike): 3.2e-16 against the restatement (bars 2.4e-13 ..
# 2.5e-13, from readings of 2.4e-14 .. 2.5e-14), 2.5e-14 against ops.enhance (bar 1e-11); bubble 2.9e-14 (noted only).
@pytest.mark.parametrize("M,n", sr.DEGREES)
def test_shared_every_degree_all_rhs_kinds(dev, note, M, n):
    """Gap 1: every instantiated degree, with the in-kernel sine, the element-major table of the same f and the
    point-major table."""
    nodes, values, f, read = sr.degree_case(M, n)
    bar = sr.bar(read[0])
    Wr = sr.restate(nodes, values, M, sr.GAMMA, n, f, GD)
    Wg, _ = _general(dev, nodes, values, M, n)
    Ws, st_s = _shared(dev, nodes, values, M, n)
    We, st_e = _shared(dev, nodes, values, M, n, f)
    Wp, st_p = _shared(dev, nodes, values, M, n, f, pm=True)
    assert not st_s.any() and not st_e.any() and not st_p.any()
    assert np.array_equal(We, Wp)
    note("restatement reading M=%d n=%d" % (M, n), read[0], bar)
    for name, W in (("sine", Ws), ("table", We)):
        d_r, d_g = orc.rel_l2_coef(W, Wr).max(), orc.rel_l2_coef(W, Wg).max()
        note("%s vs restatement" % name, d_r, bar)
        note("%s vs ops.enhance" % name, d_g, 1e-11)
        note("%s bubble vs restatement" % name, orc.rel_l2_bubble(W, Wr).max())
        assert d_r <= bar, (name, d_r, bar)
        assert d_g <= 1e-11, (name, d_g)


@pytest.mark.parametrize("M,n", sr.TAIL_CFG)
def test_shared_tails_with_guards(dev, M, n):
    """Gap 2: launches of 1 .. 300 elements into buffers with canaries behind W and status; every row equals the row
    of the same element in the 300-element launch, bit for bit, for the in-kernel sine and a staged table."""
    nodes = sr.mesh(300)
    values = sr.nodal(nodes)
    h0 = sr.spacing(nodes)
    f = sr.distinct_table(300, n)
    whole = {None: _shared(dev, nodes, values, M, n)[0], "table": _shared(dev, nodes, values, M, n, f)[0]}
    for ne in sr.TAILS:
        for kind in (None, "table"):
            Wbuf, W, sbuf, status = _guarded(dev, ne, M)
            Wn, st = _shared(dev, nodes[:ne + 1], values[:ne + 1], M, n, None if kind is None else f[:ne], h0=h0,
                             ne_global=300, out=W, status=status)
            assert _guards_intact(Wbuf, sbuf, ne, M), (ne, kind)
            assert not st.any() and st.shape == (ne,)
            assert np.array_equal(Wn, whole[kind][:ne]), (ne, kind)


# Measured: at most 4.1e-16 against the restatement (bars 2.5e-13).
@pytest.mark.parametrize("n,M", sr.STAGING)
def test_shared_table_staging_any_point_count(dev, note, n, M):
    """Gap 3: the element-major table goes through LDS eight points at a time; n below, at and off multiples of 8, with
    a table whose every entry is distinct."""
    nodes, values, f, read = sr.degree_case(M, n, "distinct")
    bar = sr.bar(read[0])
    We, st = _shared(dev, nodes, values, M, n, f)
    Wp, _ = _shared(dev, nodes, values, M, n, f, pm=True)
    assert not st.any()
    assert np.array_equal(We, Wp)
    d = orc.rel_l2_coef(We, sr.restate(nodes, values, M, sr.GAMMA, n, f, GD)).max()
    note("staged table n=%d vs restatement" % n, d, bar)
    assert d <= bar


def _trig_bar(dev, note, case, f_ref, rows=slice(None)):
    """(restatement on the extended-precision sine, bar): max(MARGIN x the general kernel's distance from the same
    reference, the case's restatement bar)."""
    Wr = sr.restate(case.nodes, case.values, case.M, sr.GAMMA, case.n, f_ref, GD)
    read = sr.reading(case.nodes, case.values, case.M, sr.GAMMA, case.n, f_ref, GD)
    Wg, stg = _general(dev, case.nodes, case.values, case.M, case.n, rhs=(case.amp, case.omega))
    assert not stg.any()
    d_gen = orc.rel_l2_coef(Wg[rows], Wr[rows]).max()
    bar = max(sr.MARGIN * d_gen, sr.bar(read[0]))
    note("%s: restatement reading" % case.name, read[0])
    note("%s: ops.enhance vs reference" % case.name, d_gen, bar)
    return Wr, bar


# Measured, shared kernel vs reference / ops.enhance vs reference / bar:  a1 1.6e-16 / 2.1e-16 / 1.0e-13,
# a2 2.2e-16 / 2.5e-14 / 2.5e-13,  a3 2.2e-16 / 2.5e-14 / 2.5e-13,  b 2.2e-16 / 5.0e-14 / 5.0e-13 (small, straddling and
# large wave alike),  c 2.5e-15 / 2.5e-14 / 2.5e-13,  d (status 0) 2.2e-16 / 5.0e-16 / 2.5e-13 with 34 of 130 elements in
# the fallback.
@pytest.mark.parametrize("case", sr.TRIG, ids=repr)
def test_shared_in_kernel_sine_branches(dev, note, case):
    """Gap 4 (a)-(c): the step angle through the table (|dth| >= 0.5) on both paths, another (amp, omega), waves on
    either side of |th0| + n|dth| = 64 and across it, and arguments of order 1e9 where both restores of the per-point
    argument run.  The reference is the restatement fed with amp * sin(fl(omega x_k)), sine in extended precision."""
    reach = sr.trig_reaches(case)
    assert all(reach.values()), reach                 # the inputs reach the branch (host arithmetic, before the launch)
    f_ref = sr.sine_exact(case.nodes, case.n, case.amp, case.omega)
    Wr, bar = _trig_bar(dev, note, case, f_ref)
    W, st = _shared(dev, case.nodes, case.values, case.M, case.n, rhs=(case.amp, case.omega))
    assert not st.any()
    d = orc.rel_l2_coef(W, Wr)
    note("%s: shared vs reference" % case.name, d.max(), bar)
    assert d.max() <= bar, (case.name, d.max(), bar)
    if case.branch == "b":                           # the waves either side of 64 and the straddling wave, each on its own
        p = sr.trig_predicates(case.nodes, case.n, case.omega)
        for kind in ("small", "mixed", "large"):
            w = p["waves"][p[kind].index(True)]
            note("%s: %s wave" % (case.name, kind), d[w].max(), bar)
            assert d[w].max() <= bar, kind


def test_shared_in_kernel_sine_beyond_3e9_falls_back(dev, note):
    """Gap 4 (d): where every |omega x_k| of an element is below 2.9e9 the result meets the bar with status 0; where
    every one is above 3.1e9 the row is the linear interpolant with status 1; in between either, but the status says
    which; fail_count counts the non-zero statuses."""
    import torch
    case = sr.TRIG_D
    reach = sr.trig_reaches(case)
    assert all(reach.values()), reach
    ok, nan = sr.d_split(case)
    f_ref = sr.sine_exact(case.nodes, case.n, case.amp, case.omega)
    Wr, bar = _trig_bar(dev, note, case, f_ref, rows=ok)
    fc = torch.zeros(1, dtype=torch.int32, device=dev)
    W, st = _shared(dev, case.nodes, case.values, case.M, case.n, rhs=(case.amp, case.omega), fail_count=fc)
    lin = sr.linear_rows(case.nodes, case.values, case.M, GD)
    assert not st[ok].any() and np.all(st[nan] == 1)
    assert set(np.unique(st)) <= {0, 1}
    d = orc.rel_l2_coef(W[st == 0], Wr[st == 0]).max()
    note("%s: shared vs reference, status 0" % case.name, d, bar)
    note("%s: elements ok / fallback / between" % case.name, ok.sum())
    note("%s: fallbacks" % case.name, (st != 0).sum())
    assert d <= bar
    assert np.array_equal(W[st != 0], lin[st != 0])
    is_lin = np.all(W == lin, axis=1)
    assert np.array_equal(is_lin, st != 0)            # status is non-zero exactly where the row is the interpolant
    assert int(fc.item()) == int((st != 0).sum())


def _shared_no_status(dev, nodes, values, M, n, f, bc):
    """The C entry with status = fail_count = NULL (the wrapper always allocates a status)."""
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    ne = len(nodes) - 1
    x, u = _t(dev, nodes), _t(dev, values)
    ft = None if f is None else _t(dev, f)
    W = torch.full((ne, M), CANARY, dtype=torch.float64, device=dev)
    rhs_id, params = ops._rhs((ops.POISSON_AMP, ops.POISSON_OMEGA), ft, ne * n, "ne*n_colloc", False)
    args = ops._prefix(x, u, 0, ne, GD, bc, M, n, 1.0)[:-1] + (
        rhs_id, params, ops._ptr(ft), ops._ptr(_op(dev, sr.spacing(nodes), M, n)), ops._ptr(W), None, None,
        ops._stream(None))
    _capi.check(_capi.load().lssvr_enhance_shared(*args, None), "lssvr_enhance_shared")
    torch.cuda.synchronize()
    return W.cpu().numpy()


@pytest.mark.parametrize("M", sr.FALLBACK_M)
@pytest.mark.parametrize("ne", sr.FALLBACK_NE)
def test_shared_fallback_on_non_finite_data(dev, ne, M):
    """Gap 5: NaN in a nodal value (two elements), inf in a table entry at an even and at an odd point, NaN in the
    table of the LAST element (a partly filled wave: counted once, not once per duplicate lane), NaN in either end of
    bc.  Status 1 and the linear interpolant exactly on the affected elements, every other row bit-equal to the clean
    run, fail_count = the number of affected elements; with and without status / fail_count."""
    import torch
    n = sr.n_for(M)
    nodes = sr.mesh(ne)
    values = sr.nodal(nodes)
    f = sr.sine_table(nodes, n)
    clean = {k: _shared(dev, nodes, values, M, n, **kw)[0]
             for k, kw in (("sine", {}), ("em", dict(f=f)), ("pm", dict(f=f, pm=True)))}
    assert np.array_equal(clean["em"], clean["pm"])

    def bad_f(e, k, v):
        g = f.copy()
        g[e, k] = v
        return g

    bad_u = values.copy()
    bad_u[64] = np.nan
    nan = np.nan
    # (name, rhs kinds, values, table, bc, affected elements)
    cases = (("node", ("sine", "em"), bad_u, f, (0.0, 0.0), [63, 64]),
             ("inf_even_k", ("em", "pm"), values, bad_f(5, 2, np.inf), (0.0, 0.0), [5]),
             ("inf_odd_k", ("em", "pm"), values, bad_f(ne - 3, 3, -np.inf), (0.0, 0.0), [ne - 3]),
             ("nan_last_element", ("em", "pm"), values, bad_f(ne - 1, n // 2, nan), (0.0, 0.0), [ne - 1]),
             ("bc_left", ("sine", "em"), values, f, (nan, 0.0), [0]),
             ("bc_right", ("sine", "pm"), values, f, (0.0, nan), [ne - 1]))
    for name, kinds, u, ftab, bc, hit in cases:
        lin = sr.linear_rows(nodes, u, M, GD, bc)
        for kind in kinds:
            want = clean[kind].copy()
            want[hit] = lin[hit]
            want_st = np.zeros(ne, dtype=np.int32)
            want_st[hit] = 1
            kw = {} if kind == "sine" else dict(f=ftab, pm=(kind == "pm"))
            fc = torch.zeros(1, dtype=torch.int32, device=dev)
            W, st = _shared(dev, nodes, u, M, n, bc=bc, fail_count=fc, **kw)
            assert np.array_equal(st, want_st), (name, kind, np.flatnonzero(st))
            assert np.array_equal(W, want, equal_nan=True), (name, kind)
            assert int(fc.item()) == len(hit), (name, kind, int(fc.item()))
            W2, st2 = _shared(dev, nodes, u, M, n, bc=bc, **kw)                   # no fail_count
            assert np.array_equal(st2, want_st) and np.array_equal(W2, want, equal_nan=True), (name, kind)
            if kind != "pm":                                                       # neither status nor fail_count
                W3 = _shared_no_status(dev, nodes, u, M, n, None if kind == "sine" else ftab, bc)
                assert np.array_equal(W3, want, equal_nan=True), (name, kind)


# Measured: 2.5e-16 against the restatement, end rows meet bc to 7.1e-16 x |w|_1 (bars 1.0e-13).
def test_shared_shards_and_boundary_values(dev, note):
    """Gap 6: shards with elem_offset / ne_global concatenate bit for bit to the single launch; the global end rows
    interpolate a non-zero bc, interior shard ends keep their nodal values, and so does a shard with elem_offset = 0
    whose first node is not gxmin (Dual.py:65)."""
    ne, M, n = sr.SHARD_NE, 9, 16
    nodes = sr.mesh(ne)
    values = sr.nodal(nodes)
    h0 = sr.spacing(nodes)
    sign = (-1.0) ** np.arange(M)
    assert abs(values[0] - sr.BC[0]) > 0.1 and abs(values[-1] - sr.BC[1]) > 0.1
    tables = {"sine": sr.sine_table(nodes, n), "table": sr.distinct_table(ne, n)}
    for kind, f in tables.items():
        fk = (lambda a, b: None) if kind == "sine" else (lambda a, b: f[a:b])
        whole, st = _shared(dev, nodes, values, M, n, fk(0, ne), bc=sr.BC)
        assert not st.any()
        read = sr.reading(nodes, values, M, sr.GAMMA, n, f, GD, sr.BC)
        bar = sr.bar(read[0])
        d = orc.rel_l2_coef(whole, sr.restate(nodes, values, M, sr.GAMMA, n, f, GD, sr.BC)).max()
        note("%s: single launch vs restatement" % kind, d, bar)
        assert d <= bar
        parts = [_shared(dev, nodes[a:b + 1], values[a:b + 1], M, n, fk(a, b), h0=h0, bc=sr.BC, elem_offset=a,
                         ne_global=ne)[0] for a, b in zip(sr.SHARD_CUTS[:-1], sr.SHARD_CUTS[1:])]
        assert np.array_equal(np.concatenate(parts), whole), kind
        ends = (abs(whole[0] @ sign - sr.BC[0]) / np.abs(whole[0]).sum(),
                abs(whole[-1].sum() - sr.BC[1]) / np.abs(whole[-1]).sum())
        note("%s: end rows vs bc" % kind, max(ends), bar)
        assert max(ends) <= bar
        a = sr.SHARD_CUTS[1]
        assert abs(parts[1][0] @ sign - values[a]) <= bar * np.abs(parts[1][0]).sum()
        # elem_offset = 0 but the first node is not gxmin: the nodal value stays
        loose, _ = _shared(dev, nodes[a:], values[a:], M, n, fk(a, ne), h0=h0, bc=sr.BC)
        assert np.array_equal(loose, whole[a:]), kind
        # ... and a shard that ends at gxmax but is not the last of ne_global keeps its right nodal value
        inner, _ = _shared(dev, nodes, values, M, n, fk(0, ne), bc=sr.BC, ne_global=ne + 1)
        assert np.array_equal(inner[:-1], whole[:-1])
        assert abs(inner[-1].sum() - values[-1]) <= bar * np.abs(inner[-1]).sum()


# Measured: 7.4e-15 against ops.enhance (bar 1e-11); last rows 1.1e-16 against the restatement (reading 7.2e-15, bar
# 1.0e-13).
def test_shared_both_store_paths(dev, note):
    """Gap 7: M = 32 with 65536 elements is exactly 2^21 doubles, the last write-through size; 65537 elements take
    the nontemporal store.  Same nodes, guards behind both outputs."""
    M, n, ne = sr.STORE_M, sr.STORE_N, sr.STORE_NE
    nodes = sr.mesh(ne + 1)
    values = sr.nodal(nodes)
    h0 = sr.spacing(nodes)
    assert ne * M == 1 << 21
    Wb1, W1, sb1, st1 = _guarded(dev, ne, M)
    small, s1 = _shared(dev, nodes[:ne + 1], values[:ne + 1], M, n, h0=h0, ne_global=ne + 1, out=W1, status=st1)
    Wb2, W2, sb2, st2 = _guarded(dev, ne + 1, M)
    large, s2 = _shared(dev, nodes, values, M, n, out=W2, status=st2)
    assert _guards_intact(Wb1, sb1, ne, M) and _guards_intact(Wb2, sb2, ne + 1, M)
    assert not s1.any() and not s2.any()
    assert np.array_equal(small, large[:ne])
    Wg, _ = _general(dev, nodes, values, M, n)
    d = orc.rel_l2_coef(large, Wg).max()
    note("65537 x 32 vs ops.enhance", d, 1e-11)
    assert d <= 1e-11
    k = 8                                                  # the last rows against the restatement
    sub, vsub = nodes[-k - 1:], values[-k - 1:]
    f = sr.sine_table(sub, n)
    Wr = sr.restate(sub, vsub, M, sr.GAMMA, n, f, GD, elem_offset=ne + 1 - k, ne_global=ne + 1, h0=h0)
    Wo = sr.oracle(sub, vsub, M, sr.GAMMA, n, f, GD)       # (a sub-mesh that ends at gxmax: the same end rule)
    read = orc.rel_l2_coef(Wr, Wo).max()
    bar = sr.bar(read)
    d = orc.rel_l2_coef(large[-k:], Wr).max()
    note("last rows: restatement reading", read)
    note("last rows vs restatement", d, bar)
    assert d <= bar


# Measured rel_l2_bubble: 1.1e-14 at ne = 4096 (restatement 1.1e-14, bar 1.1e-13), 2.3e-13 at ne = 3000 (restatement
# 2.2e-13, bar 2.2e-12).  Before the in-kernel sine restored numpy's argument on its |omega x| < 64 path the first read
# 2.1e-13 on the last element, where f is next to a zero.
@pytest.mark.parametrize("cfg", sr.BUBBLE)
def test_shared_bubble_against_oracle(dev, note, cfg):
    """Gap 8: the enhancement on its own (p >= 2), which rel_l2_coef cannot see on fine meshes."""
    ne, M, n, gamma, lo, hi = cfg
    nodes = np.linspace(lo, hi, ne + 1)
    values = orc.fem_p1_solve(nodes) if lo == -1.0 else np.sin(np.pi * nodes)
    f = sr.sine_table(nodes, n)
    read = sr.reading(nodes, values, M, gamma, n, f, (lo, hi))
    bar = sr.bar(read[1])
    Wo = sr.oracle(nodes, values, M, gamma, n, f, (lo, hi))
    for kind, kw in (("sine", {}), ("table", dict(f=f))):
        W, st = _shared(dev, nodes, values, M, n, gamma=gamma, global_domain=(lo, hi), **kw)
        assert not st.any()
        d = orc.rel_l2_bubble(W, Wo).max()
        note("%s ne=%d: rel_l2_bubble vs oracle (restatement reads %.2e)" % (kind, ne, read[1]), d, bar)
        assert d <= bar, (kind, d, bar)


def test_shared_caller_buffers_and_profiled(dev):
    """Gap 9: out=, status= and fail_count= are used and returned as they are, with the bits of the allocating call;
    profiled=True writes the same bits and returns a plausible duration."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    M, n = 9, 16
    nodes, values, f, _ = sr.degree_case(M, n)
    x, u = _t(dev, nodes), _t(dev, values)
    op = _op(dev, sr.spacing(nodes), M, n)
    for kw in ({}, dict(rhs_values=_t(dev, f))):
        W0, st0 = ops.enhance_shared(x, u, op, M, n, global_domain=GD, **kw)
        out = torch.full((sr.NE0, M), CANARY, dtype=torch.float64, device=dev)
        status = torch.full((sr.NE0,), ICANARY, dtype=torch.int32, device=dev)
        fc = torch.zeros(1, dtype=torch.int32, device=dev)
        W1, st1 = ops.enhance_shared(x, u, op, M, n, global_domain=GD, out=out, status=status, fail_count=fc, **kw)
        torch.cuda.synchronize()
        assert W1 is out and st1 is status
        assert torch.equal(out, W0) and torch.equal(status, st0) and int(fc.item()) == 0
        out2 = torch.full((sr.NE0, M), CANARY, dtype=torch.float64, device=dev)
        dt = ops.enhance_shared(x, u, op, M, n, global_domain=GD, out=out2, profiled=True, **kw)
        assert torch.equal(out2, W0)
        assert 1e-7 < dt < 1e-2
