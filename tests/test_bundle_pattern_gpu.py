"""-m gpu: the fused solve kernel k_bundle_irs reading ONE shared copy of the 16-bit index pattern of identical bundles
(host.hpp: PatternShare; the host side: tests/test_bundle_pattern_host.py) against the CPU oracle on the same inputs and
the same permutation, and against the same kernel reading every bundle's own copy (CHIP_NO_SHARED_PATTERN)."""
import numpy as np
import pytest

from tests import problems
from tests.bundle_pattern_problems import two_sizes

pytestmark = pytest.mark.gpu

TOL = 1e-8        # the suite's bound on the refined KKT solution against the oracle (tests/test_gpu_parity.py)
TOL_ORDER = 1e-10  # two orders of the same LDS atomics (test_paired_solves_match_separate_solves)


def relerr(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def _solvers(hip, oracle, pr, settings):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=settings)
    cones = oracle.Cones(pr["cones"])
    ost = oracle.Settings.default()
    if settings is not None:
        ost.ir_max_iter = settings.iterative_refinement_max_iter
        ost.ir_reltol = settings.iterative_refinement_reltol
        ost.ir_abstol = settings.iterative_refinement_abstol
        ost.ir_enable = settings.iterative_refinement_enable
        ost.ir_stop_ratio = settings.iterative_refinement_stop_ratio
    ko = oracle.KKTSolver(pr["n"], pr["m"], pr["P"], pr["A"], cones, settings=ost, perm=ks.perm)
    return ks, ko, cones


def _references(oracle, ko, cones, pr, nrhs):
    """the oracle's solutions and refinement rounds at the two scaling points, computed once per problem and settings"""
    rng = np.random.default_rng(3)
    out = []
    for it in range(2):
        s_, z_ = pr["s"] * (1.0 + 0.3 * it), pr["z"] / (1.0 + 0.2 * it)
        assert cones.update_scaling(s_, z_) and ko.update()
        pts = []
        for _ in range(nrhs):
            rx, rz = rng.standard_normal(pr["n"]), rng.standard_normal(pr["m"])
            ko.setrhs(rx, rz)
            ok, xo, zo = ko.solve()
            assert ok
            pts.append((rx, rz, np.concatenate([xo, zo]), ko.last_ir_iters))
        out.append((s_, z_, pts))
    return out


def _run(hip, ks, pr, refs, shared, paired, label):
    """the handle's solves at both scaling points against `refs`; -> its solutions"""
    n = pr["n"]
    nb = ks.work_model()["n_bundles"]
    assert ks.step_kernels() & 4, label
    assert hip.debug_counter(ks, "pattern_shared_bundles") == (nb if shared else 0), label
    sols = []
    for s_, z_, pts in refs:
        assert ks.update_scaling(s_, z_) and ks.update()
        dev = [(hip.DeviceArray(rx), hip.DeviceArray(rz), hip.DeviceArray(n + pr["m"])) for rx, rz, _, _ in pts]
        if paired:  # the shape of the benchmark's step: one paired call, one single solve, one collect
            (ra, za, la), (rb, zb, lb), (rc, zc, lc) = dev
            ks.solve2_dev_enqueue(ra.ptr, za.ptr, la.ptr, la.ptr + 8 * n, rb.ptr, zb.ptr, lb.ptr, lb.ptr + 8 * n)
            ks.setrhs_dev(rc.ptr, zc.ptr)
            ks.solve_dev_enqueue(lc.ptr, lc.ptr + 8 * n)
            uok, sok = ks.collect()
            assert uok and sok == [True, True, True], label
            assert ks.linear_solver_info().last_ir_iterations == pts[-1][3], label
            # (the ABI reports the rounds of the LAST solve only: the paired right-hand sides once more, one at a time)
            for (rx, rz, ref, rounds), (d_rx, d_rz, _) in zip(pts[:2], dev[:2]):
                again = hip.DeviceArray(n + pr["m"])
                ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
                assert ks.solve_dev(again.ptr, again.ptr + 8 * n)
                assert ks.linear_solver_info().last_ir_iterations == rounds, label
                assert relerr(again.numpy(), ref) <= TOL, label
        for (rx, rz, ref, rounds), (d_rx, d_rz, out) in zip(pts, dev):
            if not paired:
                ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
                assert ks.solve_dev(out.ptr, out.ptr + 8 * n)
                got_rounds = ks.linear_solver_info().last_ir_iterations
                assert got_rounds == rounds, (label, got_rounds, rounds)
            got = out.numpy()
            err = relerr(got, ref)
            print("%s: rel. err against the oracle %.3e (rounds %d)" % (label, err, rounds))
            assert err <= TOL, (label, err)
            sols.append(got)
    assert ks.fused_fallbacks() == 0, label
    assert hip.debug_counter(ks, "pattern_shared_bundles") == (nb if shared else 0), label
    return sols


@pytest.mark.parametrize("case", ["shared", "two_classes", "switch_off", "three_rounds", "bench_settings"])
def test_fused_solve_reads_one_shared_pattern(hip, oracle, case, monkeypatch):
    """shared: 6 x SOC(701), one class.  two_classes: 3 x SOC(601) + 3 x SOC(701) under one budget row (bundles of 1803 and
    2103 nodes: both inside the 512 .. 3072 nodes k_bundle_irs takes).  switch_off: CHIP_NO_SHARED_PATTERN, every bundle
    its own copy.  three_rounds: three forced refinement rounds, candidates through xa / xb.  bench_settings: one round
    fixed, a paired call + a single solve + one collect, like a step of the benchmark.  Each at two scaling points:
    k_bundle_irs takes the solves, all bundles read a shared copy (none with the switch), solutions within 1e-8 of the
    oracle's with the oracle's refinement rounds, no fallback; shared / two_classes also within 1e-10 of a handle with
    the switch set on the same inputs."""
    pr = two_sizes(600, 700) if case == "two_classes" else problems.portfolio_socp(6, 700, seed=11)
    kw = {}
    if case == "three_rounds":
        kw = dict(iterative_refinement_max_iter=3, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0,
                  iterative_refinement_stop_ratio=0.0)
    elif case == "bench_settings":
        kw = dict(iterative_refinement_max_iter=1, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0)
    st = hip.Settings.default(**kw) if kw else None
    paired = case == "bench_settings"
    if case == "switch_off":
        monkeypatch.setenv("CHIP_NO_SHARED_PATTERN", "1")
    ks, ko, cones = _solvers(hip, oracle, pr, st)
    assert hip.debug_counter(ks, "pattern_classes") == (2 if case == "two_classes" else 1)
    assert hip.debug_counter(ks, "pattern_mismatches") == 0
    refs = _references(oracle, ko, cones, pr, 3 if paired else 2)
    if case == "three_rounds":
        assert all(p[3] == 3 for _, _, pts in refs for p in pts)
    sols = _run(hip, ks, pr, refs, case != "switch_off", paired, case)
    if case in ("shared", "two_classes"):
        monkeypatch.setenv("CHIP_NO_SHARED_PATTERN", "1")  # (read when a handle is created)
        ks0, _, _ = _solvers(hip, oracle, pr, st)
        sols0 = _run(hip, ks0, pr, refs, False, paired, case + " / own copies")
        for a, b in zip(sols, sols0):
            print("%s: shared against own copies %.3e" % (case, relerr(a, b)))
            assert relerr(a, b) <= TOL_ORDER, (case, relerr(a, b))
