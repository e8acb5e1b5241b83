"""-m gpu: the fused solve kernel k_bundle_irs with one record per bundle (csrc/kernels.hpp: IrsDesc) and its phases' first
loads requested a phase ahead, against the CPU oracle on the same inputs and the same permutation, and against the same
kernel with the chained prologue and no loads ahead (CHIP_IRS_FLAGS bit 4) on the same build.  The bundle shapes are the
edge cases tests/test_irs_descriptor_host.py establishes on the host: the smallest bundle the kernel takes, levels of 1023,
1024 and 1025 entries around the batch of 1024, a bundle that fills every thread's slots and the leaf limit."""
import numpy as np
import pytest

from tests import problems
from tests.bundle_pattern_problems import two_sizes
from tests.test_bundle_pattern_gpu import TOL, TOL_ORDER, _references, _run, _solvers, relerr

pytestmark = pytest.mark.gpu

# (5 and 19 workgroups: fewer than the grid barrier's sub-groups, 19 no multiple of 8)
PROBLEMS = [(nblocks, bs) for bs in (170, 341, 512, 1023) for nblocks in (5, 19)] + ["two_sizes"]
SETTINGS = {
    "default": None,  # ends by tolerance behind a speculative forward sweep: the requests made for it are dropped
    "no_refinement": dict(iterative_refinement_enable=False),
    "bench": dict(iterative_refinement_max_iter=1, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0),
    "three_rounds": dict(iterative_refinement_max_iter=3, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0,
                         iterative_refinement_stop_ratio=0.0),  # candidates through xa / xb
}


def _nan_is_refused(hip, ks, pr, label):
    rx, rz = np.ones(pr["n"]), np.ones(pr["m"])
    rx[pr["n"] // 2] = np.nan
    d_rx, d_rz, out = hip.DeviceArray(rx), hip.DeviceArray(rz), hip.DeviceArray(pr["n"] + pr["m"])
    ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
    assert not ks.solve_dev(out.ptr, out.ptr + 8 * pr["n"]), label


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("prob", PROBLEMS, ids=lambda p: p if isinstance(p, str) else "%dx%d" % p)
def test_fused_solve_with_loads_ahead(hip, oracle, prob, setting, monkeypatch):
    """at two scaling points: k_bundle_irs takes the solves without a fallback; solutions within 1e-8 of the oracle's with
    the oracle's refinement rounds; within 1e-10 of a handle of the same kind solving with the chained form; a right-hand
    side with a NaN is refused by both forms."""
    pr = two_sizes(600, 700) if prob == "two_sizes" else problems.portfolio_socp(prob[0], prob[1], seed=11)
    kw = SETTINGS[setting]
    st = hip.Settings.default(**kw) if kw else None
    paired = setting == "bench"
    label = "%s / %s" % (prob, setting)
    ks, ko, cones = _solvers(hip, oracle, pr, st)
    refs = _references(oracle, ko, cones, pr, 3 if paired else 2)
    if setting == "three_rounds":
        assert all(p[3] == 3 for _, _, pts in refs for p in pts)
    nb = ks.work_model()["n_bundles"]
    assert hip.debug_counter(ks, "irs_desc_bundles") == nb, label  # (the records are read, the loads go ahead)
    sols = _run(hip, ks, pr, refs, True, paired, label)
    _nan_is_refused(hip, ks, pr, label)
    monkeypatch.setenv("CHIP_IRS_FLAGS", "7")  # (3: the defaults, 4: chained prologue, no loads ahead; read at creation)
    ks0, _, _ = _solvers(hip, oracle, pr, st)
    assert hip.debug_counter(ks0, "irs_desc_bundles") == 0, label
    sols0 = _run(hip, ks0, pr, refs, True, paired, label + " / chained")
    _nan_is_refused(hip, ks0, pr, label + " / chained")
    for a, b in zip(sols, sols0):
        print("%s: loads ahead against chained %.3e" % (label, relerr(a, b)))
        assert relerr(a, b) <= TOL_ORDER, (label, relerr(a, b))
