"""CPU: the round loop every ``solve_adaptive`` mode runs (``FEMLSSVRPrimalSolver._adapt_rounds``), driven by scripted
rounds -- no GPU, no library: each stop rule, what it leaves in ``adapt_history`` and whether ``mesh`` moves."""
import numpy as np
import pytest

from hybrid_fem_lssvr_amd import FEMLSSVRPrimalSolver


class Script:
    """A mode made of canned rounds: round i reports ``ests[i]`` on the solver's current mesh and, asked to refine,
    answers ``refines[i]`` -- a veto (None) or (number of elements to add at the left end, the counts)."""

    def __init__(self, solver, ests, refines, fields=None):
        self.s, self.ests, self.refines = solver, ests, refines
        self.fields = dict(marked=0) if fields is None else fields
        self.rounds = self.refined = 0

    def __call__(self):
        i = self.rounds
        self.rounds += 1
        nodes = self.s.mesh.p[0]
        ne = nodes.size - 1

        def refine():
            self.refined += 1
            out = self.refines[i]
            if out is None:
                return None
            add, counts = out
            left = np.linspace(nodes[0], nodes[1], add + 2)
            return np.concatenate([left, nodes[2:]]), counts
        return ne, self.ests[i], dict(self.fields), refine


def _solver(n=5):
    return FEMLSSVRPrimalSolver(n, lssvr_M=5, global_domain=(0.0, 1.0))


def test_default_mesh_and_stop_at_tol():
    s = _solver()
    assert s.mesh is None
    sc = Script(s, [1.0, 0.5, 0.1], [(2, dict(marked=2)), (1, dict(marked=1)), (3, dict(marked=3))])
    assert s._adapt_rounds(0.5, 100, 10, sc) == 0.5
    assert s.adapt_history == [dict(ne=4, estimate=1.0, marked=2), dict(ne=6, estimate=0.5, marked=0)]
    assert (sc.rounds, sc.refined) == (2, 1)          # the round that meets tol is not refined
    assert s.mesh.nelements == 6
    assert np.array_equal(s.mesh.p[0], [0.0, 0.25 / 3, 0.5 / 3, 0.25, 0.5, 0.75, 1.0])


def test_tol_none_runs_to_max_iter_and_last_round_is_not_refined():
    s = _solver()
    s.adapt_history = ["stale"]
    sc = Script(s, [3.0, 2.0, 1.0, 0.5], [(1, dict(marked=1))] * 4)
    assert s._adapt_rounds(None, 100, 3, sc) == 1.0
    assert s.adapt_history == [dict(ne=4, estimate=3.0, marked=1), dict(ne=5, estimate=2.0, marked=1),
                               dict(ne=6, estimate=1.0, marked=0)]
    assert (sc.rounds, sc.refined) == (3, 2) and s.mesh.nelements == 6


def test_nonfinite_estimate_never_meets_tol():
    s = _solver()
    sc = Script(s, [float("inf"), float("nan"), 0.0], [(1, dict(marked=1))] * 3)
    assert s._adapt_rounds(1e300, 100, 5, sc) == 0.0
    assert [r["ne"] for r in s.adapt_history] == [4, 5, 6]


def test_stop_when_nothing_is_marked():
    s = _solver()
    sc = Script(s, [1.0, 1.0, 1.0], [(1, dict(marked=1)), (0, dict(marked=0)), (1, dict(marked=1))])
    assert s._adapt_rounds(0.0, 100, 10, sc) == 1.0
    assert s.adapt_history == [dict(ne=4, estimate=1.0, marked=1), dict(ne=5, estimate=1.0, marked=0)]
    assert (sc.rounds, sc.refined) == (2, 2) and s.mesh.nelements == 5


def test_stop_when_refinement_would_exceed_max_elements():
    s = _solver()
    sc = Script(s, [1.0, 1.0, 1.0], [(2, dict(marked=2)), (2, dict(marked=2)), (1, dict(marked=1))])
    assert s._adapt_rounds(None, 7, 10, sc) == 1.0          # 4 -> 6 -> (8 > 7)
    assert s.adapt_history == [dict(ne=4, estimate=1.0, marked=2), dict(ne=6, estimate=1.0, marked=0)]
    assert s.mesh.nelements == 6 and sc.rounds == 2         # the mesh is the one of the last record
    s = _solver()
    sc = Script(s, [1.0, 1.0], [(3, dict(marked=3)), (1, dict(marked=1))])
    assert s._adapt_rounds(None, 7, 2, sc) == 1.0           # exactly max_elements is allowed
    assert s.mesh.nelements == 7 and s.adapt_history[0]["marked"] == 3


def test_initial_mesh_above_max_elements():
    s = _solver(9)
    s.adapt_history = ["stale"]
    sc = Script(s, [1.0], [(1, dict(marked=1))])
    with pytest.raises(ValueError, match="the initial mesh has 8 elements > max_elements = 7"):
        s._adapt_rounds(None, 7, 3, sc)
    assert sc.rounds == 0 and s.adapt_history == ["stale"]
    s = FEMLSSVRPrimalSolver(3, mesh=np.linspace(0.0, 1.0, 9))          # a given mesh is checked, not replaced
    with pytest.raises(ValueError, match="8 elements > max_elements = 4"):
        s._adapt_rounds(None, 4, 3, sc)
    assert s._adapt_rounds(None, 8, 1, sc) == 1.0 and s.adapt_history == [dict(ne=8, estimate=1.0, marked=0)]


HP = dict(marked=0, raised=0, dof=20)


def test_hp_raise_alone_goes_on_and_no_change_stops():
    s = _solver()
    sc = Script(s, [1.0] * 4, [(0, dict(marked=0, raised=3)), (1, dict(marked=1, raised=0)),
                               (0, dict(marked=0, raised=0)), (1, dict(marked=1, raised=1))], HP)
    assert s._adapt_rounds(None, 100, 10, sc) == 1.0
    assert s.adapt_history == [dict(ne=4, estimate=1.0, marked=0, raised=3, dof=20),
                               dict(ne=4, estimate=1.0, marked=1, raised=0, dof=20),
                               dict(ne=5, estimate=1.0, marked=0, raised=0, dof=20)]
    assert list(s.adapt_history[0]) == ["ne", "estimate", "marked", "raised", "dof"]
    assert (sc.rounds, sc.refined) == (3, 3) and s.mesh.nelements == 5


def test_hp_veto_stops_and_leaves_mesh_and_record():
    s = _solver()
    sc = Script(s, [1.0] * 3, [(1, dict(marked=1, raised=2)), None, (1, dict(marked=1, raised=0))], HP)
    assert s._adapt_rounds(None, 100, 10, sc) == 1.0          # the mode says no: sum M_e would exceed max_dof
    assert s.adapt_history == [dict(ne=4, estimate=1.0, marked=1, raised=2, dof=20),
                               dict(ne=5, estimate=1.0, marked=0, raised=0, dof=20)]
    assert (sc.rounds, sc.refined) == (2, 2) and s.mesh.nelements == 5


def test_start_runs_after_the_mesh_check_and_before_the_reset():
    s = _solver()
    s.adapt_history = ["stale"]
    seen = []

    def start(ne):
        seen.append((ne, list(s.adapt_history)))
        raise ValueError("the initial mesh has 20 coefficients > max_dof = 19")

    sc = Script(s, [1.0], [None])
    with pytest.raises(ValueError, match="max_elements"):
        s._adapt_rounds(None, 3, 1, sc, start)
    assert seen == []
    with pytest.raises(ValueError, match="max_dof"):
        s._adapt_rounds(None, 4, 1, sc, start)
    assert seen == [(4, ["stale"])] and sc.rounds == 0 and s.adapt_history == ["stale"]
