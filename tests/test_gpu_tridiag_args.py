"""GPU: the argument checks of the 14 public ``ops.tridiag_*`` functions, one table over all of them.  Every function
raises the same class with the same words for the same mistake, checks in the same order, and differs from its
neighbours only where the families differ on purpose: the fewest elements, the end values it takes, the sign of kappa,
and what it does with a ``work`` that is too small.  The expectations are those of the four dispatchers these functions
had, one per family, before they shared one; nothing here is read off the shared one."""
import numpy as np
import pytest

import periodic_rules as pr

pytestmark = pytest.mark.gpu

NE, NC = 4, 2

# (function, family, non-symmetric bands, multi).  What a family decides:
#   dirichlet  ne >= 1; single forms take u0, u1 by value and replace a short work; multi forms take bc [nc, 2]
#   bc         ne >= 1; end_kinds, kappa >= 0, end_values (a pair / [nc, 2]); the single forms replace a short work
#   pivot      as bc with kappa of either sign; BOTH forms raise on a short work
#   periodic   ne >= 2; no end values; the single forms replace a short work
FORMS = [
    ("tridiag_dirichlet_solve", "dirichlet", False, False),
    ("tridiag_ns_dirichlet_solve", "dirichlet", True, False),
    ("tridiag_dirichlet_solve_multi", "dirichlet", False, True),
    ("tridiag_ns_dirichlet_solve_multi", "dirichlet", True, True),
    ("tridiag_bc_solve", "bc", False, False),
    ("tridiag_ns_bc_solve", "bc", True, False),
    ("tridiag_bc_solve_multi", "bc", False, True),
    ("tridiag_ns_bc_solve_multi", "bc", True, True),
    ("tridiag_pivot_solve", "pivot", True, False),
    ("tridiag_pivot_solve_multi", "pivot", True, True),
    ("tridiag_periodic_solve", "periodic", False, False),
    ("tridiag_ns_periodic_solve", "periodic", True, False),
    ("tridiag_periodic_solve_multi", "periodic", False, True),
    ("tridiag_ns_periodic_solve_multi", "periodic", True, True),
]
SIZER = {"dirichlet": "lssvr_tridiag_multi_work_bytes", "bc": "lssvr_tridiag_bc_work_bytes",
         "pivot": "lssvr_tridiag_pivot_work_bytes", "periodic": "lssvr_tridiag_periodic_work_bytes"}
MIN_NE = {"dirichlet": (1, "need at least one"), "bc": (1, "need at least one"), "pivot": (1, "need at least one"),
          "periodic": (2, "two elements")}
U0, U1 = 0.25, -0.5

form = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
ends_form = pytest.mark.parametrize("form", [f for f in FORMS if f[1] in ("bc", "pivot")],
                                    ids=[f[0] for f in FORMS if f[1] in ("bc", "pivot")])


def _host(ne, ns, multi):
    """Diagonally dominant bands of ``ne`` elements and a load (one case, or NC of them): float64 host arrays."""
    rng = np.random.default_rng(100 * ne + 10 * ns + multi)
    diag, sub = np.full(ne + 1, 4.0) + 0.1 * np.arange(ne + 1), np.full(ne, -1.0)
    sup = np.full(ne, -1.5) if ns else sub
    return diag, sub, sup, rng.standard_normal((NC, ne + 1) if multi else ne + 1)


def _reference(family, diag, sub, sup, load):
    """The dense solve of one case: rows 0 and ne are u = U0, u = U1 (two Dirichlet ends), or the cyclic system."""
    if family == "periodic":
        return pr.dense_solve(diag, sub, sup, load)
    n = diag.size
    A = np.diag(diag) + np.diag(sub, -1) + np.diag(sup, 1)
    b = load.copy()
    A[0], A[-1], b[0], b[-1] = 0.0, 0.0, U0, U1
    A[0, 0] = A[n - 1, n - 1] = 1.0
    return np.linalg.solve(A, b)


def _call(ops, dev, form, ne=NE, kinds=(0, 0), kappa=(0.0, 0.0), values="default", **over):
    """The function of ``form`` on valid arguments; ``over`` replaces a band by name (diag, off | sub, sup, load) or
    passes out / work; ``kinds``, ``kappa``, ``values`` are the ends of the forms that take them (``values``: bc of
    the Dirichlet multi forms, end_values of bc and pivot)."""
    import torch
    name, family, ns, multi = form
    diag, sub, sup, load = (torch.as_tensor(a, device=dev) for a in _host(ne, ns, multi))
    bands = {"diag": diag, **({"sub": sub, "sup": sup} if ns else {"off": sub}), "load": load}
    kw = {k: over.pop(k) for k in ("out", "work") if k in over}
    assert set(over) <= set(bands), over
    bands.update(over)
    if isinstance(values, str):
        values = torch.tensor([[U0, U1]] * NC, dtype=torch.float64, device=dev) if multi else (U0, U1)
    if family == "dirichlet":
        ends = (values,) if multi else values
    else:
        ends = () if family == "periodic" else (kinds, kappa, values)
    return getattr(ops, name)(*bands.values(), *ends, **kw)


def _check_answer(form, u, ne=NE):
    """u against the dense solve.  The systems are strictly diagonally dominant (|diag| >= 4, off-diagonals sum to at
    most 2.5: condition number below 4), ne = 4: a backward-stable solve is within a few eps of it; 1e-14 relative is
    45 eps."""
    name, family, ns, multi = form
    diag, sub, sup, load = _host(ne, ns, multi)
    got = u.cpu().numpy().reshape(-1, ne + 1)
    assert got.shape[0] == (NC if multi else 1)
    for q, ld in enumerate(load.reshape(-1, ne + 1)):
        ref = _reference(family, diag, sub, sup, ld)
        assert np.max(np.abs(got[q] - ref)) <= 1e-14 * np.max(np.abs(ref)), (name, q)


def _short(need, dev):
    """The largest float64 buffer that does not hold ``need`` bytes (``work`` is a float64 tensor)."""
    import torch
    return torch.zeros((need - 1) // 8, dtype=torch.float64, device=dev)


@form
def test_valid_call_and_out(dev, form):
    """The valid call of the table solves the system; a single form given ``out`` returns a 1-D view of it, a multi
    form given nc + 1 rows writes and returns the first nc."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    multi = form[3]
    _check_answer(form, _call(ops, dev, form))
    out = torch.full((NC + 1, NE + 1) if multi else (NE + 1,), -777.0, dtype=torch.float64, device=dev)
    u = _call(ops, dev, form, out=out)
    assert u.data_ptr() == out.data_ptr() and tuple(u.shape) == ((NC, NE + 1) if multi else (NE + 1,))
    assert not multi or bool((out[NC] == -777.0).all())
    _check_answer(form, u)


@form
def test_bands_and_load(dev, form):
    import torch
    from hybrid_fem_lssvr_amd import ops
    name, family, ns, multi = form
    off = "sub" if ns else "off"
    one = torch.ones(2 * (NE + 1), dtype=torch.float64, device=dev)
    for band, n in (("diag", NE), (off, NE - 1), (off, NE + 1)) + ((("sup", NE + 1),) if ns else ()):
        with pytest.raises(ValueError, match="band lengths"):
            _call(ops, dev, form, **{band: one[:n]})
    # a load of the other form's shape, and one of the wrong length
    wrong = (one[:NE + 1], one[:NC * NE].reshape(NC, NE)) if multi else (one.reshape(2, NE + 1), one[:NE])
    for load in wrong:
        with pytest.raises(ValueError, match="band lengths"):
            _call(ops, dev, form, load=load)
    if not multi and family != "dirichlet":       # (the Dirichlet single forms count the doubles of the load)
        with pytest.raises(ValueError, match="band lengths"):
            _call(ops, dev, form, load=one[:NE + 1].reshape(1, NE + 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call(ops, dev, form, diag=torch.ones(NE + 1, dtype=torch.float64))
    with pytest.raises(TypeError, match="expected torch.float64"):
        _call(ops, dev, form, load=(one[:NC * (NE + 1)].reshape(NC, NE + 1) if multi else one[:NE + 1]).float())
    with pytest.raises(TypeError, match="expected a torch.Tensor"):
        _call(ops, dev, form, **{off: [1.0] * NE})


@form
def test_too_few_elements(dev, form):
    from hybrid_fem_lssvr_amd import ops
    ne_min, words = MIN_NE[form[1]]
    with pytest.raises(ValueError, match=words):
        _call(ops, dev, form, ne=ne_min - 1)
    _check_answer(form, _call(ops, dev, form, ne=ne_min), ne=ne_min)


@form
def test_out_of_the_wrong_shape(dev, form):
    import torch
    from hybrid_fem_lssvr_amd import ops
    multi = form[3]
    shapes = ((NC, NE), (NC - 1, NE + 1), (NC * (NE + 1),)) if multi else ((NE,), (NE + 2,), (2, NE + 1))
    for shape in shapes:
        with pytest.raises(ValueError, match="out must be" if multi else "out must hold"):
            _call(ops, dev, form, out=torch.zeros(shape, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call(ops, dev, form, out=torch.zeros((NC, NE + 1) if multi else NE + 1, dtype=torch.float64))


@form
def test_end_values_of_the_wrong_shape(dev, form):
    """bc [nc, 2] of the Dirichlet multi forms, end_values of bc and pivot: a pair on the single forms, [nc, 2] on the
    multi forms; ``None`` is zeros.  (The Dirichlet single forms take two floats, the periodic forms nothing.)"""
    import torch
    from hybrid_fem_lssvr_amd import ops
    name, family, ns, multi = form
    if family == "periodic" or (family == "dirichlet" and not multi):
        return
    words = r"bc must be \[nc, 2\]" if family == "dirichlet" else r"end_values must be \[nc, 2\]"
    bad = [np.zeros((NC + 1, 2)), torch.zeros((NC, 3), dtype=torch.float64, device=dev)] if multi else \
        [(0.0, 0.0, 0.0, 0.0), torch.zeros(2, dtype=torch.float64, device=dev)]
    for values in bad:
        with pytest.raises(ValueError, match=words):
            _call(ops, dev, form, values=values)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call(ops, dev, form, values=torch.zeros((NC if multi else 1, 2), dtype=torch.float64))
    if multi:
        zeros = _call(ops, dev, form, values=None)
        assert torch.equal(zeros, _call(ops, dev, form, values=np.zeros((NC, 2))))


@ends_form
def test_end_kinds_and_kappa(dev, form):
    """``_end_kinds`` behind bc and pivot: pairs of END_DIRICHLET / END_ROBIN, kappa finite -- and >= 0 for bc, of
    either sign for pivot."""
    from hybrid_fem_lssvr_amd import ops
    pivot = form[1] == "pivot"
    with pytest.raises(TypeError, match="must be pairs"):
        _call(ops, dev, form, kinds=0)
    with pytest.raises(ValueError, match="must be pairs"):
        _call(ops, dev, form, kappa=(0.0, 0.0, 0.0))
    for kinds in ((0, 2), (True, 0), (-1, 1)):
        with pytest.raises(ValueError, match="end_kinds must be END_DIRICHLET"):
            _call(ops, dev, form, kinds=kinds)
    for kappa in ((float("inf"), 0.0), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="kappa must be finite"):
            _call(ops, dev, form, kinds=(1, 1), kappa=kappa)
    if pivot:
        _call(ops, dev, form, kinds=(1, 0), kappa=(-0.5, 0.0))
    else:
        with pytest.raises(ValueError, match="kappa must be finite and >= 0"):
            _call(ops, dev, form, kinds=(1, 0), kappa=(-0.5, 0.0))


@form
def test_short_work(dev, form):
    """A ``work`` one double short of the sizer: the multi forms and both pivot forms raise, the other single forms
    replace it and solve; a ``work`` of exactly the sizer is used."""
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    name, family, ns, multi = form
    need = getattr(_capi.load(), SIZER[family])(NE, NC if multi else 1)
    assert need >= 8
    if multi or family == "pivot":
        with pytest.raises(ValueError, match=r"work holds \d+ bytes, %s\(%d, %d\)" % (SIZER[family], NE,
                                                                                      NC if multi else 1)):
            _call(ops, dev, form, work=_short(need, dev))
    else:
        short = _short(need, dev)
        _check_answer(form, _call(ops, dev, form, work=short))
        assert bool((short == 0.0).all())
    _check_answer(form, _call(ops, dev, form, work=torch.zeros((need + 7) // 8, dtype=torch.float64, device=dev)))
    if family != "dirichlet" or multi:            # (the Dirichlet single forms look at the size of work alone)
        with pytest.raises(TypeError, match="work: expected torch.float64"):
            _call(ops, dev, form, work=torch.zeros(need, dtype=torch.uint8, device=dev))


@form
def test_order_of_the_checks(dev, form):
    """Two mistakes in one call raise what the earlier check raises: bands, ne, end kinds, out, work, end values."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    name, family, ns, multi = form

    def t(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=dev)

    bad_out, short, has_kinds = t(NE + 3), t(1), family in ("bc", "pivot")
    with pytest.raises(ValueError, match="band lengths"):
        _call(ops, dev, form, diag=t(NE), out=bad_out, kinds=(5, 5))
    with pytest.raises(ValueError, match=MIN_NE[family][1]):
        _call(ops, dev, form, ne=MIN_NE[family][0] - 1, out=bad_out, kinds=(5, 5))
    with pytest.raises(ValueError, match="end_kinds must be" if has_kinds else "out must"):
        _call(ops, dev, form, kinds=(5, 5), out=bad_out, work=short)
    with pytest.raises(ValueError, match="out must"):
        _call(ops, dev, form, out=bad_out, work=short, values=np.zeros((NC + 3, 2)) if multi else "default")
    if multi and family != "periodic":
        with pytest.raises(ValueError, match="work holds"):
            _call(ops, dev, form, work=short, values=np.zeros((NC + 3, 2)))


def test_tridiag_work_holds_every_family_named(dev):
    """``ops.tridiag_work``: a float64 scratch on the tensor's device, at least the largest of the named sizers."""
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    lib, x = _capi.load(), torch.zeros(3, dtype=torch.float64, device=dev)
    for ne, nc in ((1, 1), (NE, NC), (600, 9), (100000, 6)):
        for families in (("dirichlet",), ("bc",), ("pivot", "bc"), ("periodic", "dirichlet"), tuple(SIZER)):
            w = ops.tridiag_work(x, ne, nc, *families)
            assert w.device == x.device and w.dtype == torch.float64 and w.is_contiguous()
            assert w.numel() * 8 >= max(getattr(lib, SIZER[f])(ne, nc) for f in families), (ne, nc, families)
    with pytest.raises(KeyError):
        ops.tridiag_work(x, NE, NC, "robin")
    with pytest.raises(ValueError, match="at least one family"):
        ops.tridiag_work(x, NE, NC)
    # the scratch of the named families is one the multi forms take
    u = _call(ops, dev, FORMS[9], work=ops.tridiag_work(x, NE, NC, "pivot", "bc"))
    _check_answer(FORMS[9], u)
