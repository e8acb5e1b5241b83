"""CPU: the reference trace of the iterative refinement (tests/ir_ref.py) against the oracle's own solve(), and the hard
conditions of the fixtures of tests/ir_fixtures.py on which tests/test_ir_decisions_gpu.py rests: every decision a factor
2 from its threshold, every norm 1e3 times its rounding bound, the accepted iterate 100 * TOL away from every other
iterate of its right-hand side, no pivot regularised dynamically.  The oracle factors under the permutation the package
takes (a host-only handle), as the GPU cases do."""
import numpy as np
import pytest

from tests import ir_fixtures as F
from tests import ir_ref

NAMES = [n for fam in F.FAMILIES.values() for n in fam]
_REFS = {}


def _ref(hip, oracle, name):
    if name not in _REFS:
        pr = F.problem(name)
        ref = F.Reference(oracle, pr, perm=F.host_perm(hip, pr))
        sc, k = F.scenarios(ref)
        seen = []
        for sid, (kind, ir) in sc.items():
            tr = ref.trace(ref.full(*F.rhs(pr, kind)), ir)
            seen.append((sid, kind, ir, tr))
        _REFS[name] = (ref, k, seen)
    return _REFS[name]


def test_trace_on_a_small_dense_system():
    """ir_ref.trace by hand: K = diag(1, -0.5) solved with diag(1.25, -0.2): the first entry's error contracts by 0.2 per
    round, the second's grows by 1.5"""
    rows = ir_ref.full_rows(2, [0, 1, 2], [0, 1], [1.0, -0.5])
    assert [(c.tolist(), v.tolist()) for c, v in rows] == [([0], [1.0]), ([1], [-0.5])]
    solve = lambda r: np.asarray(r) / np.array([1.25, -0.2])
    tr = ir_ref.trace(rows, solve, np.array([1.0, 0.0]), max_iter=3, reltol=0.0, abstol=0.0, stop_ratio=0.0)
    assert tr["rounds"] == 3 and tr["accepted"] == 3 and tr["why_stopped"] == "limit"
    np.testing.assert_allclose([it[0] for it in tr["iterates"]], [0.8, 0.96, 0.992, 0.9984], rtol=1e-15)
    np.testing.assert_allclose([r[1] for r in tr["rounds_list"]], [5.0, 5.0, 5.0], rtol=1e-12)
    tr = ir_ref.trace(rows, solve, np.array([1.0, 0.0]), max_iter=3, reltol=0.0, abstol=0.0, stop_ratio=8.0)
    assert (tr["rounds"], tr["accepted"], tr["why_stopped"]) == (1, 1, "stop_ratio")
    assert ir_ref.margins(tr, stop_ratio=8.0)[0] == pytest.approx(1.6)
    tr = ir_ref.trace(rows, solve, np.array([0.0, 1.0]), max_iter=3, reltol=0.0, abstol=0.0, stop_ratio=5.0)
    assert (tr["rounds"], tr["accepted"], tr["why_stopped"]) == (1, 0, "stop_ratio")  # (|e| 1.5 -> 2.25: rejected)
    assert tr["rounds_list"][0][2] is False
    tr = ir_ref.trace(rows, solve, np.array([1.0, 0.0]), max_iter=5, reltol=0.1, abstol=0.0, stop_ratio=4.0)
    assert (tr["rounds"], tr["why_stopped"]) == (1, "tolerance")  # (0.2 > 0.1 >= 0.04)
    assert ir_ref.margins(tr, stop_ratio=4.0)[0] == pytest.approx(1.25)  # (improved 5 against 4; the norms 2 and 2.5 from 0.1)
    tr = ir_ref.trace(rows, solve, np.array([1.0, 0.0]), enable=False)
    assert (tr["rounds"], tr["why_stopped"]) == (0, "disabled")


@pytest.mark.parametrize("name", NAMES)
def test_reference_trace_matches_the_oracle_and_fixture_conditions_hold(hip, oracle, name):
    ref, k, seen = _ref(hip, oracle, name)
    want = F.expected(k)
    assert set(want) == {s[0] for s in seen}
    for sid, kind, ir, tr in seen:
        dec, rnd, sep = F.check_conditions(ref, sid, kind, ir, tr, want[sid])
        xo, rounds = ref.oracle_solve(ref.full(*F.rhs(ref.pr, kind)), ir)
        xa = tr["iterates"][tr["accepted"]]
        err = np.max(np.abs(xo - xa)) / max(1.0, np.max(np.abs(xa)))
        print("%s / %s: rounds %d accepted %d (%s)  margin %.3g  norm / bound %.3g  separation %.3g  oracle %.2e"
              % (name, sid, tr["rounds"], tr["accepted"], tr["why_stopped"], dec, rnd, sep, err))
        assert rounds == tr["rounds"], (sid, rounds, tr["rounds"])
        assert err <= F.TOL, (sid, err)
    # the solve after each scenario: its own x0 under the settings of tol0
    kind, ir = "other", dict(seen[0][2])
    assert seen[0][0] == "tol0"
    tr = ref.trace(ref.full(*F.rhs(ref.pr, kind)), ir)
    F.check_conditions(ref, "tol0 / other", kind, ir, tr, (0, 0, "tolerance"))


@pytest.mark.parametrize("family", list(F.FAMILIES))
def test_every_branch_occurs_in_every_family(hip, oracle, family):
    for name in F.FAMILIES[family]:
        _, _, seen = _ref(hip, oracle, name)
        whys = {tr["why_stopped"] for _, _, _, tr in seen}
        assert whys == {"tolerance", "limit", "stop_ratio", "disabled"}, (name, whys)
        outcomes = {r[2] for _, _, _, tr in seen for r in tr["rounds_list"]}
        assert outcomes == {True, False}, (name, outcomes)
        stops = {(r[2], r[3]) for _, _, _, tr in seen for r in tr["rounds_list"] if r[3]}
        # accepted and stopped (1 < improved < stop_ratio), rejected, accepted although worse up to the limit
        assert {(True, "stop_ratio"), (False, "stop_ratio"), (True, "limit"), (True, "tolerance")} <= stops, (name, stops)


def test_slowly_contracting_fixture(hip, oracle):
    """qp_3000_slow: 17 rounds that each improve by 1.4 (stop_ratio 0.6: margin 2.3), the norms falling 300-fold"""
    pr = F.problem("qp_3000_slow")
    ref = F.Reference(oracle, pr, perm=F.host_perm(hip, pr))
    b = ref.full(*F.rhs(pr, "late"))
    tr = ref.trace(b, F.SLOW_IR)
    dec, rnd, sep = F.check_conditions(ref, "slow", "late", F.SLOW_IR, tr, (F.MANY, F.MANY, "limit"))
    norms = [tr["norme0"]] + [r[0] for r in tr["rounds_list"]]
    print("slow: margin %.3g  norm / bound %.3g  separation %.3g  norms %.3g .. %.3g" % (dec, rnd, sep, norms[0], norms[-1]))
    # what the reuse of a norm set must not let through: the norm of round it - 13 instead of round it's, it = 15 .. 17
    for it in (15, 16, 17):
        assert norms[it - 1] / norms[it - 13] < 0.5 * 0.6 and norms[it - 13] / norms[it] > 50.0, (it, norms)
    xo, rounds = ref.oracle_solve(b, F.SLOW_IR)
    assert rounds == F.MANY and np.max(np.abs(xo - tr["iterates"][F.MANY])) <= F.TOL * np.max(np.abs(xo))
