"""-m gpu: k_bundle_irs_fixed, the instance of the fused solve kernel with the usual switches folded at compile time
(csrc/bundle_ir.hip: irs_body, FIXED; the choice is made per launch, kkt_step.cpp: fused_choose), against the CPU oracle on
the same inputs and the same permutation, and against the general kernel on the same build (CHIP_IRS_FLAGS bit 8).  The
shapes are those of tests/test_irs_ahead_gpu.py: the smallest bundle the kernel takes, levels around the batch of 1024
entries, a bundle that fills all 12 slots of a thread, grids of 5 and 19 workgroups (fewer than the barrier's sub-groups,
no multiple of 8), two classes of bundles."""
import numpy as np
import pytest

from tests import problems
from tests.bundle_pattern_problems import two_sizes
from tests.test_bundle_pattern_gpu import TOL, TOL_ORDER, _references, _run, _solvers, relerr

pytestmark = pytest.mark.gpu

PROBLEMS = [(5, 170), (19, 341), (5, 512), (19, 1023), "two_sizes"]
SETTINGS = {
    "default": None,
    "bench": dict(iterative_refinement_max_iter=1, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0),
    "three_rounds": dict(iterative_refinement_max_iter=3, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0,
                         iterative_refinement_stop_ratio=0.0),
}


def _problem(prob):
    return two_sizes(600, 700) if prob == "two_sizes" else problems.portfolio_socp(prob[0], prob[1], seed=11)


def _fixed(hip, ks):
    return hip.debug_counter(ks, "irs_fixed_launches")


def _nan_is_refused(hip, ks, pr, label):
    rx, rz = np.ones(pr["n"]), np.ones(pr["m"])
    rx[pr["n"] // 2] = np.nan
    d_rx, d_rz, out = hip.DeviceArray(rx), hip.DeviceArray(rz), hip.DeviceArray(pr["n"] + pr["m"])
    ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
    assert not ks.solve_dev(out.ptr, out.ptr + 8 * pr["n"]), label


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("prob", PROBLEMS, ids=lambda p: p if isinstance(p, str) else "%dx%d" % p)
def test_fixed_instance_takes_the_solves(hip, oracle, prob, setting, monkeypatch):
    """at two scaling points: every solve launches k_bundle_irs_fixed, no fallback; solutions within 1e-8 of the oracle's
    with the oracle's refinement rounds; within 1e-10 of a handle created under CHIP_IRS_FLAGS=11 (the general kernel, whose
    counter stays 0); a right-hand side with a NaN is refused by both."""
    pr = _problem(prob)
    kw = SETTINGS[setting]
    st = hip.Settings.default(**kw) if kw else None
    paired = setting == "bench"
    label = "%s / %s" % (prob, setting)
    ks, ko, cones = _solvers(hip, oracle, pr, st)
    refs = _references(oracle, ko, cones, pr, 3 if paired else 2)
    if setting == "three_rounds":
        assert all(p[3] == 3 for _, _, pts in refs for p in pts)
    nb = ks.work_model()["n_bundles"]
    assert hip.debug_counter(ks, "irs_desc_bundles") == nb, label
    assert _fixed(hip, ks) == 0, label
    sols = _run(hip, ks, pr, refs, True, paired, label)
    # (_run per scaling point: two single solves, or the paired call + one solve + the paired right-hand sides again)
    solves = 2 * (5 if paired else 2)
    print("%s: irs_fixed_launches %d of %d solves" % (label, _fixed(hip, ks), solves))
    assert _fixed(hip, ks) == solves, label
    _nan_is_refused(hip, ks, pr, label)
    assert _fixed(hip, ks) == solves + 1, label
    assert ks.fused_fallbacks() == 0, label
    monkeypatch.setenv("CHIP_IRS_FLAGS", "11")  # (3: the defaults, 8: the general kernel; read at creation)
    ks0, _, _ = _solvers(hip, oracle, pr, st)
    assert hip.debug_counter(ks0, "irs_desc_bundles") == nb, label
    sols0 = _run(hip, ks0, pr, refs, True, paired, label + " / general")
    _nan_is_refused(hip, ks0, pr, label + " / general")
    assert _fixed(hip, ks0) == 0, label
    for a, b in zip(sols, sols0):
        print("%s: fixed against general %.3e" % (label, relerr(a, b)))
        assert relerr(a, b) <= TOL_ORDER, (label, relerr(a, b))


def test_no_refinement_keeps_the_general_kernel(hip, oracle):
    pr = _problem((5, 170))
    st = hip.Settings.default(iterative_refinement_enable=False)
    ks, ko, cones = _solvers(hip, oracle, pr, st)
    _run(hip, ks, pr, _references(oracle, ko, cones, pr, 2), True, False, "no refinement")
    assert _fixed(hip, ks) == 0


def test_chained_prologue_keeps_the_general_kernel(hip, oracle, monkeypatch):
    pr = _problem((5, 170))
    monkeypatch.setenv("CHIP_IRS_FLAGS", "7")
    ks, ko, cones = _solvers(hip, oracle, pr, None)
    assert hip.debug_counter(ks, "irs_desc_bundles") == 0
    _run(hip, ks, pr, _references(oracle, ko, cones, pr, 2), True, False, "chained")
    assert _fixed(hip, ks) == 0


def test_results_over_the_right_hand_side_keep_the_general_kernel(hip, oracle):
    """lhs == rhs: the last candidate cannot be written ahead of its verdict (IrView::spec_out)"""
    pr = _problem((5, 170))
    n = pr["n"]
    ks, ko, cones = _solvers(hip, oracle, pr, None)
    assert ks.step_kernels() & 4
    for s_, z_, pts in _references(oracle, ko, cones, pr, 2):
        assert ks.update_scaling(s_, z_) and ks.update()
        for rx, rz, ref, rounds in pts:
            buf = hip.DeviceArray(np.concatenate([rx, rz]))
            ks.setrhs_dev(buf.ptr, buf.ptr + 8 * n)
            assert ks.solve_dev(buf.ptr, buf.ptr + 8 * n)
            assert ks.linear_solver_info().last_ir_iterations == rounds
            err = relerr(buf.numpy(), ref)
            print("in place: rel. err against the oracle %.3e (rounds %d)" % (err, rounds))
            assert err <= TOL, err
    assert _fixed(hip, ks) == 0
    assert ks.fused_fallbacks() == 0


def test_small_bundles_keep_k_bundle_ir(hip, oracle):
    pr = problems.portfolio_socp(3, 200, seed=11)
    n = pr["n"]
    ks, ko, cones = _solvers(hip, oracle, pr, None)
    assert not ks.step_kernels() & 4  # (bundles below the size k_bundle_irs takes)
    for s_, z_, pts in _references(oracle, ko, cones, pr, 2):
        assert ks.update_scaling(s_, z_) and ks.update()
        for rx, rz, ref, rounds in pts:
            d_rx, d_rz, out = hip.DeviceArray(rx), hip.DeviceArray(rz), hip.DeviceArray(n + pr["m"])
            ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
            assert ks.solve_dev(out.ptr, out.ptr + 8 * n)
            assert relerr(out.numpy(), ref) <= TOL
    assert _fixed(hip, ks) == 0


def test_refinement_switched_between_solves(hip, oracle):
    """set_settings between two solves of ONE handle: the choice is made per launch, the counter advances only for the
    solves with refinement"""
    pr = _problem((19, 341))
    n = pr["n"]
    ks, ko, cones = _solvers(hip, oracle, pr, None)
    off = hip.Settings.default(iterative_refinement_enable=False)
    _, ko_off, cones_off = _solvers(hip, oracle, pr, off)  # (for the oracle without refinement)
    refs = {True: _references(oracle, ko, cones, pr, 1)[0], False: _references(oracle, ko_off, cones_off, pr, 1)[0]}
    s_, z_, _ = refs[True]
    assert ks.update_scaling(s_, z_) and ks.update()
    want = 0
    for on in (True, False, True, True, False, True):
        ks.set_settings(hip.Settings.default() if on else off)
        rx, rz, ref, rounds = refs[on][2][0]
        d_rx, d_rz, out = hip.DeviceArray(rx), hip.DeviceArray(rz), hip.DeviceArray(n + pr["m"])
        ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
        assert ks.solve_dev(out.ptr, out.ptr + 8 * n)
        assert ks.linear_solver_info().last_ir_iterations == rounds
        assert relerr(out.numpy(), ref) <= TOL, (on, relerr(out.numpy(), ref))
        want += 1 if on else 0
        assert _fixed(hip, ks) == want, (on, want)
    assert ks.fused_fallbacks() == 0
