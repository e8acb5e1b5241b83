"""tests/eq_ref.py on the CPU (no GPU, no package): the exact family's sums are exact in any order, the wide family's
reference stays inside its own bound whichever way its sums are taken, every case shows what it was built to show, and
the restatement reproduces ruiz() of tests/test_solver_gpu.py on that module's fixtures."""
import math

import numpy as np
import pytest

from tests import eq_ref as R

SMALL_CASES = [k for k in R.RUIZ_CASES if k != "n262145"]


def _other_sums(fn):
    """fn(summer) -> a dict of arrays, with each of the three ways to sum"""
    return {name: fn(s) for name, s in R.SUMMERS.items()}


@pytest.mark.parametrize("name", list(R.RUIZ_CASES))
def test_exact_family_step_is_the_same_in_any_order(name):
    st = R.RUIZ_CASES[name]("exact")
    smin, smax = R.scaling("exact")
    ref = R.check_state_sums(st, smin, smax)
    if name in R.RUIZ_KINDS:
        assert ref["kind"] in R.RUIZ_KINDS[name], (name, ref["kind"])
    for v in (smin, smax, st["c"]):
        assert math.frexp(v)[0] == 0.5  # powers of two
    for key in ("d", "e"):
        assert np.all(np.frexp(st[key])[0] == 0.5)
    if name == "n262145":
        return
    got = _other_sums(lambda s: R.ruiz_step(st, smin, smax, s))
    for other in ("sequential", "pairwise"):
        for key in ("q", "b", "d", "e"):
            assert R.same_bits(got[other][key], got["fsum"][key]), (name, other, key)
        assert R.same_bits(got[other]["P"][2], got["fsum"]["P"][2]) and got[other]["c"] == got["fsum"]["c"]


@pytest.mark.parametrize("name", SMALL_CASES)
def test_wide_family_step_stays_inside_its_bound_in_any_order(name):
    st = R.RUIZ_CASES[name]("wide")
    smin, smax = R.scaling("wide")
    got = _other_sums(lambda s: R.ruiz_step(st, smin, smax, s))
    ref = got["fsum"]
    if name in R.RUIZ_KINDS:
        assert ref["kind"] in R.RUIZ_KINDS[name], (name, ref["kind"])
    for other in ("sequential", "pairwise"):
        o = got[other]
        ratios, fails = R.compare_step(ref, dict(Px=o["P"][2], Ax=o["A"][2], q=o["q"], b=o["b"], d=o["d"], e=o["e"],
                                                 c=o["c"], factor=o["factor"]), st["c"], False)
        assert not fails, (name, other, fails)
        assert max(ratios.values()) <= 1.0


def test_cases_show_what_they_are_built_for():
    smin, smax = R.scaling("exact")
    st = R.case_offdiagonal("exact")
    ref = R.ruiz_step(st, smin, smax)
    big = abs(st["P"][2][1])
    # d: the off-diagonal entry is the norm of row 0 and of column 1; the cost mean takes it for column 1 alone
    assert ref["dw"][0] == ref["dw"][1] == 1.0 / math.sqrt(big)
    assert ref["pcol"][1] == 1.0 and ref["pcol"][0] < 1.0 and ref["kind"] == "mean"
    for fam in ("exact", "wide"):
        smin, smax = R.scaling(fam)
        st = R.case_zero_row_and_column(fam)
        ref = R.ruiz_step(st, smin, smax)
        assert np.any(np.signbit(st["P"][2]) & (st["P"][2] == 0.0)) and np.any(np.signbit(st["A"][2]) & (st["A"][2] == 0.0))
        for j in (7, 11):
            assert ref["dw"][j] == 1.0 and ref["d"][j] == st["d"][j]
        for i in (5, 9):
            assert ref["ew"][i] == 1.0 and ref["e"][i] == st["e"][i]
        st = R.case_clipped_factors(fam)
        ref = R.ruiz_step(st, smin, smax)
        for w, cum in ((ref["dw"], st["d"]), (ref["ew"], st["e"])):
            assert np.sum(w == smin / cum) > 0 and np.sum(w == smax / cum) > 0
        ref = R.ruiz_step(R.case_factor_one_by_arithmetic(fam), smin, smax)
        assert ref["factor"] == 1.0 and ref["kind"] == "mean" and ref["mean"] == 1.0
        for row in (True, False):
            for desc in (False, True):
                st = R._dense_line(fam, row, desc)
                Ap, Ai, Ax = st["A"]
                line = np.abs(Ax[(Ai == 1) if row else (R.cols_of(Ap) == 1)])
                assert len(line) == 20000 and np.all(np.diff(line) <= 0 if desc else np.diff(line) >= 0)


@pytest.mark.parametrize("name", R.RECT_CASES)
def test_rectification_sums(name):
    n, m, A, b, e, segs = R.rect_case(name, "exact")
    assert name == "one_segment" or (segs[0][0] == 0 and segs[-1][1] == m)
    for beg, end in segs:
        R.assert_exact(e[beg:end], "cone %d:%d" % (beg, end))
    got = _other_sums(lambda s: R.rectify(m, A, b, e, segs, s))
    for other in ("sequential", "pairwise"):
        for k in range(3):
            assert R.same_bits(got[other][k], got["fsum"][k])
    if name == "lengths":
        assert [end - beg for beg, end in segs] == R.RECT_LENGTHS
        assert np.sum(np.bincount(A[1], minlength=m) == 0) >= 3  # rows of A without entries
    if name == "split":
        assert len(A[1]) == 100
    n, m, A, b, e, segs = R.rect_case(name, "wide")
    got = _other_sums(lambda s: R.rectify(m, A, b, e, segs, s))
    for other in ("sequential", "pairwise"):
        worst, fails = R.compare_rectified(got["fsum"], got[other][:3], A[1], False)
        assert not fails and worst <= 1.0, (name, other, fails)
    outside = got["fsum"][4] == 0
    assert np.any(outside) or name in ("1000_of_3",)
    assert R.same_bits(got["fsum"][1][outside], b[outside]) and R.same_bits(got["fsum"][2][outside], e[outside])


@pytest.mark.parametrize("n", R.WNORM_SIZES)
def test_sums_of_squares(n):
    v, w = R.wnorm_vectors(n, "exact", n)
    t = v * w
    R.assert_exact(t * t, "sum of squares, n = %d" % n)
    v, w = R.wnorm_vectors(n, "wide", n)
    want, bound = R.wsumsq(v, w)
    for other in (R.seq_sum, R.pairwise_sum):
        assert abs(R.wsumsq(v, w, other)[0] - want) <= bound


def test_unscale_is_the_reference_order():
    rng = np.random.default_rng(3)
    x, z, s = (R.wide(rng, 50) for _ in range(3))
    d, e = 10.0 ** rng.uniform(-3, 3, 50), 10.0 ** rng.uniform(-3, 3, 50)
    einv, c, tau = 1.0 / e, 0.37, 1.9
    xo, zo, so = R.unscale_solution(x, z, s, d, e, einv, c, tau)
    scaleinv, cinv = 1.0 / tau, 1.0 / c
    assert R.same_bits(xo, (x * d) * scaleinv) and R.same_bits(zo, (z * e) * (scaleinv * cinv))
    assert R.same_bits(so, (s * einv) * scaleinv)
    assert not R.same_bits(zo, (z * e) * scaleinv)


def _fixture_problems():
    from tests import test_solver_gpu as T
    return T, T.fixtures() + [("random_all", T.random_problem(600, 5)), ("random_nn", T.random_problem(500, 6, cones_kind="nn")),
                              ("random_q0", T.random_problem(600, 7, q_zero=True))]


def test_restatement_reproduces_ruiz_of_test_solver_gpu():
    """with numpy's own sums in place of fsum eq_ref.equilibrate is ruiz() bit for bit; with fsum the two agree within
    1e-13, the tolerance the existing tests hold the device to"""
    T, problems = _fixture_problems()

    def np_sum(a):
        return float(np.sum(np.asarray(a, dtype=float))) if len(a) else 0.0

    for name, pr in problems:
        for iters in (1, 3, 10):
            d0, e0, c0 = T.ruiz(pr, max_iter=iters)
            got = R.equilibrate(pr, iters, summer=np_sum)
            assert R.same_bits(got["d"], d0) and R.same_bits(got["e"], e0) and got["c"] == c0, (name, iters)
            ref = R.equilibrate(pr, iters)
            assert T._rel(ref["d"], d0) <= 1e-13 and T._rel(ref["e"], e0) <= 1e-13 and T._rel(ref["c"], c0) <= 1e-13
        assert R.rect_segments(pr["cones"]) == [(s, s + T.numel(c)) for s, c in zip(
            np.cumsum([0] + [T.numel(c) for c in pr["cones"]][:-1]).tolist(), pr["cones"]) if c[0] >= T.SOC and T.numel(c)]
