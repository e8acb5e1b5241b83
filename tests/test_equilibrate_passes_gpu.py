"""The 13 kernels of clarabel.rs_amd/csrc/equilibrate.hip on the MI355X, each launcher alone through the runners of
csrc/equilibrate_debug.cpp (one launch on host arrays) and then through a HipSolver, against tests/eq_ref.py
(tests/test_eq_ref_host.py checks that on the CPU).  Both families of eq_ref wherever a family applies: the exact family
and everything that involves no sum must come back bit for bit, a quantity behind a sum of L terms within
(L + 4) 2^-53 of the exact-sum reference (derived in eq_ref); no flat tolerance.  Every test prints its largest
error / bound before it asserts (pytest -s).  Output buffers of eq_invert, wnorm_batch and unscale hold NaN before the
call; the other runners update their arrays in place.

Paths (WG = 256, wavefront 64):

    k_eq_norms, k_eq_scale     nnzP = 100: the P | A split inside the second wavefront; nnzP = 0; nnzA = 0, m = 0; an
                               off-diagonal entry of P (row AND column for d, column only for the cost mean); stored 0.0
                               and -0.0, an empty row and column; one row / one column of A of 20000 entries with
                               ascending and descending magnitudes (the skip-before-atomic of amax_bits under contention)
    k_eq_factors               n = 100: the d | e split inside a wavefront; norm 0 -> factor 1; clipped below and above
                               against the cumulative d and e, rows and columns
    k_eq_cost_partial / final  n = 1, 255 | 256 | 257 (one thread's worth | a second block), 65535 | 65536 | 65537 (a
                               second trip of the 256 x 256 partition), with q so small that the SUM decides the factor;
                               mean = 0 and q = 0 (skipped, cstate[1] == 1.0); c clipped below and above; a factor that
                               is 1.0 by arithmetic (k_eq_cost_apply returns at once)
    stream_grid                n = 262145, m = 262144: nnzP + nnzA, n + m and nnzP + n one past 2048 x 256, the second
                               grid-stride trip of k_eq_norms, k_eq_factors, k_eq_scale and k_eq_cost_apply;
                               n + 2 m = 524288 | 524289 for k_unscale, n + m = 524289 for k_eq_invert
    k_eq_rect_seg              cones of 1, 2, 3, 63 | 64 | 65, 255 | 256 | 257 and 513 rows (`i += WG`: a second and a
                               third trip), the first at row 0 and the last ending at m; one cone; 1000 cones of 3
    k_eq_fill_one, rect_apply  rows between the cones keep their bytes; rows of A without entries; nnzA = 100: the
                               nnzA | m split inside a wavefront
    k_wnorm_partial / final    count 1 and 8, slots permuted, a different n per spec (one of them 0), n = 1,
                               255 | 256 | 257, 65535 | 65536 | 65537, v and w the same array
    the handle                 equilibrate_max_iter 1, 2, 3, 10 on every cone type, in the three regimes where no sum
                               decides a step (q = 0, no P, q above the mean at every step; c != 1 in the third): scaled
                               P, A, q, b, d, e, c; a drifted SOCP stopped at iteration 3: x, z, s through eq_ref's
                               unscale, 1 / d and 1 / e, and the IpmInfo from eight sums of squares taken on the host

Largest error / bound on one MI355X (exact family: 0 everywhere, every output bit for bit):
                                  exact     wide
    one Ruiz step, sum-free steps  0 (=)     0 (=)    (skipped, ||q||inf decides, c clipped: 23 of the 44 cases)
    one Ruiz step, the mean decides 0 (=)    0.28     offdiagonal (n = 3): factor 0.19, c 0.23, P 0.23, q 0.28; n = 256:
                                                      0.015; n = 65536 | 65537 | 262145: 6e-5, 3e-5, 1e-5; the others 0 (=)
    rectification                  0 (=)     0.64     1000 cones of 3 rows (bound 7 u); 1 .. 513 rows: 0.015; the others 0 (=)
    sums of squares                0 (=)     0.0064   n = 255; 256: 0.006; 65535 .. 65537: 2e-5; count 8: 0.0044
    1 / d, 1 / e, unscale          --        0 (=)
    handle, rectified rows         --        0.46     q = 0, 10 steps; no P: 0.26; q decides: 0.36 (c = 0.69 .. 0.0011);
                                                      everything else of the handle 0 (=)
    handle, IpmInfo                --        inside   res_primal, res_dual, res_primal_inf, res_dual_inf inside intervals of
                                                      relative width 1.7e-12, 1.0e-14, 8.0e-15, 7.0e-15 (values 8.9e-4, 84, 84,
                                                      0.98); costs, gaps, ktratio, x, z, s, 1 / d, 1 / e 0 (=)
(0 (=): the reference's bits.  A sum of n terms errs by a few roundings where the bound allows n + 4 of them.)

Wrong kernels (each a one-line change that stays in bounds, built in a scratch copy and run once on the MI355X against this
module and against the equilibration tests of tests/test_solver_gpu.py, tests/test_problem_update_gpu.py and
tests/test_reequilibrate_gpu.py):
    * k_eq_norms not raising the ROW of an entry of P: test_one_ruiz_step fails in 14 cases (those whose P has
      off-diagonal entries that are the largest of their rows: offdiagonal, split_in_wavefront, unconstrained, clipped_factors,
      c_clipped_below, q_zero in both families, zero_row_and_column and c_clipped_above in the wide one), with
      test_a_second_step_from_the_first_steps_state and test_handle_setup_against_reference_steps[q_zero-*, q_dominates-*];
      of the existing tests test_equilibration_matches_restatement_random[12000, 40000] and
      test_equilibration_bitwise_without_cost_scaling_or_rectification[1, 3, 10, 25] fail too, the eleven fixtures pass
    * k_eq_cost_partial losing its second trip (`i += n`): test_one_ruiz_step[n65537, n262145] fail in both families
      (n65537: factor 1.0015958 for 1.0015805, one column norm of 65537 missing; n262145: 6.56 for 1.63); n <= 65536
      passes, as it must: 65536 threads take one entry each.  Every existing test passes
    * k_eq_rect_seg summing only its first 256 rows (`i += b1`): test_rectification[lengths, one_segment] fail in both
      families (the cones of 257 and 513 rows: e 3.98 for 9.67); cones of up to 256 rows pass.  Every existing test passes
    * k_wnorm_final adding 255 of the 256 partials: test_wnorm_one_spec[65535, 65536, 65537] and test_wnorm_eight_specs fail
      in both families (n = 65535: 10127094.6 for 10163056.0); n <= 65280 leaves the last partial 0 and passes.  Every
      existing test passes
    * the z spec of residuals_and_info weighted by einv: test_handle_solution_and_info_on_a_drifted_problem fails
      (res_dual 267.07 above its interval's 83.97); every existing test passes,
      test_same_loop_as_harness_without_equilibration included (its weights are 1)
    * post_process passing scaleinv for scale_z: test_handle_solution_and_info_on_a_drifted_problem fails (the returned z is
      not eq_ref's unscale of the scaled z); every existing test selected passes (the end-to-end solves were not run)"""
import math

import numpy as np
import pytest

from tests import eq_ref as R
from tests import spmv_ref as S

pytestmark = pytest.mark.gpu

FAMILIES = ("exact", "wide")


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


# ---- 1. one Ruiz step ----------------------------------------------------------------------------------------------------
def run_step(hip, st, family):
    smin, smax = R.scaling(family)
    ref = R.ruiz_step(st, smin, smax)
    if family == "exact":
        R.assert_exact(ref["pcol"], "column norms of the scaled P")
    got = hip.debug_eq_ruiz_step(st["n"], st["m"], st["P"], st["A"], st["q"], st["b"], st["d"], st["e"], st["c"], smin,
                                 smax)
    return ref, got


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", list(R.RUIZ_CASES))
def test_one_ruiz_step(hipdev, name, family):
    st = R.RUIZ_CASES[name](family)
    ref, got = run_step(hipdev, st, family)
    ratios, fails = R.compare_step(ref, got, st["c"], family == "exact")
    print("  %s, %s family (n = %d, m = %d, nnzP = %d, nnzA = %d, %s, factor %r): largest error / bound  %s"
          % (name, family, st["n"], st["m"], len(st["P"][2]), len(st["A"][2]), ref["kind"], got["factor"],
             "  ".join("%s %.3g" % kv for kv in ratios.items())))
    assert not fails, (name, family, fails)
    if name in R.RUIZ_KINDS:
        assert ref["kind"] in R.RUIZ_KINDS[name]
    if ref["kind"] == "skipped":  # cstate[1] == 1.0 exactly; c and P keep their bytes
        assert got["factor"] == 1.0 and got["c"] == st["c"] and R.same_bits(got["Px"], ref["before"][0])
    if name == "split_in_wavefront":
        assert len(st["P"][2]) == 100 and st["n"] == 100
    if name == "offdiagonal":  # row 0 and column 1 take the off-diagonal entry for d, column 1 alone for the mean
        w = 1.0 / math.sqrt(abs(st["P"][2][1]))
        assert got["d"][0] == w and got["d"][1] == w and ref["pcol"][1] == 1.0 and ref["pcol"][0] < 1.0
    if name == "zero_row_and_column":
        assert np.all(got["d"][[7, 11]] == st["d"][[7, 11]]) and np.all(got["e"][[5, 9]] == st["e"][[5, 9]])
    if name == "clipped_factors":
        smin, smax = R.scaling(family)
        for key in ("d", "e"):
            assert np.sum(got[key] == st[key] * (smin / st[key])) > 0 and np.sum(got[key] == st[key] * (smax / st[key])) > 0
    if name == "factor_one_by_arithmetic":
        assert got["factor"] == 1.0 and ref["kind"] == "mean"
    if name == "n262145":
        n = st["n"]
        assert 2 * n - 1 == st["n"] + st["m"] == len(st["P"][2]) + len(st["A"][2]) == 2048 * 256 + 1


def test_a_second_step_from_the_first_steps_state(hipdev):
    """the runner's output is a state: a second and a third step from it, with q = 0 so that no step sums anything"""
    st = R.case_q_zero("wide")
    smin, smax = R.scaling("wide")
    for k in range(3):
        ref, got = run_step(hipdev, st, "wide")
        ratios, fails = R.compare_step(ref, got, st["c"], False)
        assert not fails and ref["kind"] == "skipped", (k, fails)
        st = dict(st, P=(st["P"][0], st["P"][1], got["Px"]), A=(st["A"][0], st["A"][1], got["Ax"]), q=got["q"],
                  b=got["b"], d=got["d"], e=got["e"], c=got["c"])


# ---- 2. the rectification ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", R.RECT_CASES)
def test_rectification(hipdev, name, family):
    n, m, A, b, e, segs = R.rect_case(name, family)
    ref = R.rectify(m, A, b, e, segs)
    if family == "exact":
        for beg, end in segs:
            R.assert_exact(e[beg:end], "cone %d:%d" % (beg, end))
    got = hipdev.debug_eq_rectify(n, m, A, b, e, segs)
    worst, fails = R.compare_rectified(ref, got, A[1], family == "exact")
    print("  %s, %s family (m = %d, nnzA = %d, %d cones of %d .. %d rows): largest error / bound %.3g"
          % (name, family, m, len(A[1]), len(segs), min(s[1] - s[0] for s in segs), max(s[1] - s[0] for s in segs), worst))
    assert not fails, (name, family, fails)
    outside = ref[4] == 0  # Zero / Nonnegative rows: the bytes they had
    assert R.same_bits(got[1][outside], b[outside]) and R.same_bits(got[2][outside], e[outside])
    assert R.same_bits(got[0][outside[A[1]]], A[2][outside[A[1]]])
    for beg, end in segs:  # a rectified cone has ONE scaling
        assert np.max(got[2][beg:end]) - np.min(got[2][beg:end]) <= 8 * R.U * np.max(got[2][beg:end])


def test_rectification_without_segments_or_rows(hipdev):
    n, m, A, b, e, _ = R.rect_case("split", "wide")
    got = hipdev.debug_eq_rectify(n, m, A, b, e, [])
    assert R.same_bits(got[0], A[2]) and R.same_bits(got[1], b) and R.same_bits(got[2], e)


# ---- 3. the inverses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(100, 150), (100, 0), (1, 1), (262145, 262144)])
def test_invert(hipdev, n, m):
    rng = np.random.default_rng(n + m)
    d, e = 10.0 ** rng.uniform(-6, 6, n), 10.0 ** rng.uniform(-6, 6, m)
    dinv, einv = hipdev.debug_eq_invert(d, e)
    want = R.invert(d, e)
    assert R.same_bits(dinv, want[0]) and R.same_bits(einv, want[1])


# ---- 4. the weighted sums of squares -------------------------------------------------------------------------------------
def check_wnorm(label, family, specs, nslots, out):
    worst = 0.0
    named = set()
    for v, w, slot in specs:
        want, bound = R.wsumsq(v, w)
        if family == "exact":
            R.assert_exact((v * w) ** 2, "sum of squares, n = %d" % len(v))
        err = abs(out[slot] - want)
        worst = max(worst, 0.0 if err == 0.0 else err / bound if bound > 0.0 else math.inf)
        assert err <= bound and (family == "wide" or out[slot] == want), (label, slot, len(v), out[slot], want, bound)
        named.add(slot)
    assert all(math.isnan(out[k]) for k in range(nslots) if k not in named), (label, out)
    print("  %s, %s family: largest error / bound %.3g" % (label, family, worst))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", R.WNORM_SIZES)
def test_wnorm_one_spec(hipdev, n, family):
    v, w = R.wnorm_vectors(n, family, 400 + n % 89)
    out = hipdev.debug_wnorm_batch([(v, w, 0)], 1)
    check_wnorm("count 1, n = %d" % n, family, [(v, w, 0)], 1, out)
    out = hipdev.debug_wnorm_batch([(v, v, 1)], 3)  # v and w the same array, slots 0 and 2 untouched
    check_wnorm("v = w, n = %d" % n, family, [(v, v, 1)], 3, out)


@pytest.mark.parametrize("family", FAMILIES)
def test_wnorm_eight_specs(hipdev, family):
    """count = WNORM_MAX with another n per spec (one of them 0, one v = w) into permuted slots of ten"""
    sizes = [257, 0, 65537, 1, 256, 65536, 255, 1000]
    slots = [7, 2, 9, 0, 5, 3, 8, 1]
    specs = []
    for k, (n, slot) in enumerate(zip(sizes, slots)):
        v, w = R.wnorm_vectors(n, family, 500 + k)
        specs.append((v, v if k == 4 else w, slot))
    out = hipdev.debug_wnorm_batch(specs, 10)
    check_wnorm("count 8", family, specs, 10, out)
    assert out[2] == 0.0  # the empty spec
    # every spec alone gives the bits it gave in the batch: a slot does not depend on what shares the launch
    for v, w, slot in specs:
        assert hipdev.debug_wnorm_batch([(v, w, 0)], 1)[0] == out[slot]
    assert np.all(np.isnan(hipdev.debug_wnorm_batch([], 4)))


# ---- 5. unscale ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(100, 150), (100, 0), (0, 70), (2, 262143), (3, 262143)])
def test_unscale(hipdev, n, m):
    rng = np.random.default_rng(n + 3 * m)
    x, d = R.wide(rng, n), 10.0 ** rng.uniform(-5, 5, n)
    z, s, e = R.wide(rng, m), R.wide(rng, m), 10.0 ** rng.uniform(-5, 5, m)
    einv = 1.0 / e
    sx, sz, ss = 1.0 / 1.7, (1.0 / 1.7) * (1.0 / 0.013), 1.0 / 2.9  # three different factors: a swap shows
    got = hipdev.debug_unscale(x, d, sx, z, e, sz, s, einv, ss)
    want = R.unscale(x, d, sx, z, e, sz, s, einv, ss)
    for k, name in enumerate(("x", "z", "s")):
        assert R.same_bits(got[k], want[k]), (name, n, m)


# ---- 6. the handle -------------------------------------------------------------------------------------------------------
def _solver(hip, pr, **kw):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    return hip.HipSolver(P, pr["q"], A, pr["b"], pr["cones"], hip.SolverSettings.default(**kw))


def _regime(name):
    from tests import test_solver_gpu as T
    if name == "q_zero":
        return T.random_problem(300, 21, q_zero=True)
    if name == "no_P":
        pr = T.random_problem(300, 22)
        return dict(pr, P=(np.zeros(301, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)))
    pr = T.random_problem(300, 23)  # q above the mean of P's column norms at every step, c inside its bounds
    return dict(pr, q=np.asarray(pr["q"]) * 1e-3)


_PROBLEMS = {}


@pytest.mark.parametrize("iters", [1, 2, 3, 10])
@pytest.mark.parametrize("regime", ["q_zero", "no_P", "q_dominates"])
def test_handle_setup_against_reference_steps(hipdev, regime, iters):
    """what setup leaves in a handle -- scaled P, A, q, b and d, e, c -- against `iters` reference steps and the
    rectification: bit for bit except the rows of the rectified cones, which are held to their cone's bound"""
    if regime not in _PROBLEMS:
        _PROBLEMS[regime] = _regime(regime)
    pr = _PROBLEMS[regime]
    assert {c[0] for c in pr["cones"]} == set(range(7)) and 200 <= pr["m"] <= 1000
    ref = R.equilibrate(pr, iters)
    want_kind = {"q_zero": "skipped", "no_P": "skipped", "q_dominates": "q"}[regime]
    assert ref["kinds"] == [want_kind] * iters, ref["kinds"]  # no sum decides anything before the rectification
    h = _solver(hipdev, pr, equilibrate_max_iter=iters)
    Px, Ax, q, b = h.scaled_data()
    d, e, c = h.equilibration()
    assert R.same_bits(d, ref["d"]) and c == ref["c"] and R.same_bits(Px, ref["Px"]) and R.same_bits(q, ref["q"])
    assert (c != 1.0) == (regime == "q_dominates")
    worst, fails = R.compare_rectified((ref["Ax"], ref["b"], ref["e"], None, ref["L"]), (Ax, b, e), pr["A"][1], False)
    print("  %s, %d steps: d, c, P, q and the unrectified rows bit for bit; rectified rows of A, b, e: largest error / "
          "bound %.3g (c = %r)" % (regime, iters, worst, c))
    assert not fails, (regime, iters, fails)
    assert np.sum(ref["L"] > 0) > 50 and np.sum(ref["L"] == 0) > 500


def _norm_interval(v, w, vbound):
    """[lo, hi] for the device's sqrt(sum (v' w)^2) when its v' is within vbound of v, entry by entry"""
    n = len(v)
    nrm = math.sqrt(R.wsumsq(v, w)[0])
    delta = math.sqrt(R.wsumsq(vbound, w)[0]) if vbound is not None else 0.0
    eps = float(R.rel_bound(n))  # the sum's (n + 4) u, which is more than its square root's share and the two roots'
    return max(0.0, nrm - delta) * (1.0 - eps), (nrm + delta) * (1.0 + eps)


def test_handle_solution_and_info_on_a_drifted_problem(hipdev):
    """rows and columns scaled by powers of two over 2^-20 .. 2^20, stopped by max_iter = 3: the returned x, z, s are
    eq_ref's unscale of the handle's scaled iterate bit for bit (scale_z carries 1 / c), dinv and einv are 1 / d and
    1 / e, and res_primal, res_dual, res_primal_inf, res_dual_inf lie between DefaultInfo::update of host sums of squares
    taken at both ends of their bounds (numerators up and denominators down, and the reverse); the costs, gaps and
    ktratio, which depend on the dots alone, are the same bits"""
    from tests import e2e_problems as E
    from tests.test_reequilibrate_gpu import drift
    pr = drift(E.basic_socp(), 7)
    h = _solver(hipdev, pr, max_iter=3)
    sol = h.solve()
    assert sol.status == "MaxIterations" and sol.iterations == 3, sol
    st = h.scaled_state()
    d, e, c = h.equilibration()
    assert c != 1.0 and d.max() / d.min() > 1e3 and e.max() / e.min() > 1e3
    assert R.same_bits(st["dinv"], 1.0 / d) and R.same_bits(st["einv"], 1.0 / e)
    x, z, s, tau, kappa = st["x"], st["z"], st["s"], st["tau"], st["kappa"]
    xo, zo, so = R.unscale_solution(x, z, s, d, e, st["einv"], c, tau)
    assert R.same_bits(sol.x, xo) and R.same_bits(sol.z, zo) and R.same_bits(sol.s, so)
    assert not R.same_bits(sol.z, (z * e) * (1.0 / tau))  # (what scale_z without 1 / c would give)
    # the residual vectors of the scaled problem at the scaled iterate, per entry with their bounds
    Px, Ax, q, b = h.scaled_data()
    scaled = dict(n=pr["n"], m=pr["m"], P=(np.asarray(pr["P"][0]), np.asarray(pr["P"][1]), Px),
                  A=(np.asarray(pr["A"][0]), np.asarray(pr["A"][1]), Ax), q=q, b=b)
    rt = S.row_terms(scaled, x, z, s, tau)
    dinv, einv = st["dinv"], st["einv"]
    specs = [(x, d, None), (z, e, None), (s, einv, None), (rt["rx_inf"][0], dinv, rt["rx_inf"][1]),
             (rt["Px"][0], dinv, rt["Px"][1]), (rt["rz_inf"][0], einv, rt["rz_inf"][1]),
             (rt["rz"][0], einv, rt["rz"][1]), (rt["rx"][0], dinv, rt["rx"][1])]
    iv = [_norm_interval(v, w, vb) for v, w, vb in specs]
    low = [iv[k][1] ** 2 if k < 3 else iv[k][0] ** 2 for k in range(8)]   # denominators up, numerators down
    high = [iv[k][0] ** 2 if k < 3 else iv[k][1] ** 2 for k in range(8)]
    normq = float(np.max(np.abs(pr["q"])))
    normb = float(np.max(np.abs(np.minimum(pr["b"], 1e20))))
    info = st["info"]
    lo = hipdev.debug_ipm_info_update(info, low, tau, kappa, c, normq, normb)
    hi = hipdev.debug_ipm_info_update(info, high, tau, kappa, c, normq, normb)
    names = ("cost_primal", "cost_dual", "res_primal", "res_dual", "res_primal_inf", "res_dual_inf", "gap_abs",
             "gap_rel", "ktratio")
    slack = 8 * R.U  # the handful of roundings of DefaultInfo::update itself
    for k in (2, 3, 4, 5):
        width = (hi[k] - lo[k]) / hi[k]
        print("  %s = %.17g in [%.17g, %.17g]: relative width %.3g" % (names[k], info[k], lo[k], hi[k], width))
        assert lo[k] * (1.0 - slack) <= info[k] <= hi[k] * (1.0 + slack), names[k]
        assert 0.0 <= width <= 1e-9 and info[k] > 1e-9, names[k]  # tight, at residuals that are far from 0
    for k in (0, 1, 6, 7, 8):
        assert R.same_bits([info[k]], [lo[k]]) and R.same_bits([info[k]], [hi[k]]), names[k]
    assert sol.r_prim == info[2] and sol.r_dual == info[3]
