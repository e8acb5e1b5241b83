"""-m gpu: the accept / reject / stop decisions of the KKT solve's iterative refinement (directldlkktsolver.rs:266-321) on
the solve paths that each keep their own copy of them and their own bookkeeping of where the accepted iterate lives:

    irs_fixed     k_bundle_irs_fixed (bundle_ir.hip: irs_body, FIXED): x0 in registers, the last candidate written ahead
    irs_general   k_bundle_irs, the same handles under CHIP_IRS_FLAGS=11
    irs_inplace   k_bundle_irs with the result over the right-hand side: candidates through xa / xb
    bundle_ir     k_bundle_ir (ir_refine.hpp: ir_verdict): sel, curt / candt: tops of 7 rows (3 x 200) and 3 rows (CHIP_NO_IR_SF)
    gstep         k_gstep_solve on the ragged forest (ir_verdict); max_iter = 31 sends the launch to k_bundle_ir instead
    host          refine_begin / refine_finish (kkt_step.cpp) on a level-scheduled banded QP: renamed work vectors, the
                  norm sets wrapping round from round 14 on

against the traces of tests/ir_ref.py on the fixtures of tests/ir_fixtures.py, whose conditions (every decision a factor
2 from its threshold, norms 1e3 times their rounding bound, iterates 100 * TOL apart, no dynamic regularisation) are
asserted again here on the trace computed under the handle's own permutation.  Every solve must report success and the
trace's rounds exactly, return the accepted iterate's visible part within TOL, and be 4 times closer to it than to any
other iterate the loop can reach on that right-hand side (the fixtures keep those 100 * TOL apart: a result within TOL of
the right one is 99 times closer to it; 4 leaves room and is not a measured number).  After each scenario a second
right-hand side is solved on the same handle under the settings of tol0 and must return its own x0: sel, xk or a norm set
left over from the launch before would show there.  Each handle is built as the existing test of its path builds it, and
the path is asserted by that test's counter.

    l1            chip_ldl_solve_refined (the same host decisions on the L1 handle), three scenarios
    retry         the unfused retry of a fused solve (CHIP_IR_TEST_DROP, test_fused_solve_timeout_falls_back): the abandoned fused
                  launch, then refine_begin / refine_finish on the fused handle's vectors; fused_fallbacks() + 1 per solve; the six
                  scenarios in which something of the abandoned launch could be left behind
    pair          solve2_dev_enqueue on the level-scheduled and on a fused handle: members with different traces
    slow          test_reused_norm_sets_while_the_norms_fall: 17 improving rounds, see there

What no counter of the package tells, and this module therefore does not assert: WHICH kernel took a launch of the grouped
fold (limit_30 / limit_31: step_kernels() == 3 is the handle's; both must return the same iterate and rounds, which they would
also do if fused_choose ignored max_iter), and whether a pair ran as two contexts or one solve after the other (both orders
and both members are held to their own traces either way).  CHIP_IRS_FLAGS is read per launch from the switch table as last
parsed: every case sets its path's switches through hip.debug_set_switch around its solves and clears them again.

Wrong kernels, each one changed line that alters only WHICH iterate is returned (no done flag, barrier or loop bound touched),
built in a scratch copy and run once on the MI355X against this module's cases of the path and the path's existing tests:
    (a) irs_body's verdict with accept = true after a non-improving round: reject, reject_first, reject_at_limit, limit_30,
        limit_31 of all five irs paths and both pair-irs cases fail (27; distance 3.7e-3 resp. 3.33 from the accepted iterate);
        tests/test_irs_fixed_gpu.py, test_bundle_pattern_gpu.py, test_irs_ahead_gpu.py: 61 passed
    (b) irs_body's final write skipping the overwrite when spec_done and the candidate was rejected: reject_first and
        reject_at_limit of irs_fixed and irs_general fail (8: the candidate written ahead is the rejected one exactly there;
        irs_inplace has no such write and passes); the same 61 existing cases passed
    (c) ir_verdict without s.sel ^= 1: all 36 cases of bundle_ir (both tops) and gstep fail, tol0 included (round 0 is an
        accepted round); of the existing tests test_ir_fixed_one_round, test_fused_solve_iterates_on_chip[old_kernel],
        test_grouped_fold_ragged_forest (both), test_small_bundles_keep_k_bundle_ir fail too, 7 others pass
    (d) refine_finish renaming the vectors on a rejected round: reject, reject_first, reject_at_limit (and limit_30 / 31) of
        host and retry, l1 reject, both pair-host cases fail (11); test_l1_fast_path_..., test_c2_random_qp,
        test_fused_solve_timeout_falls_back, test_refactor_sequence_and_update_PA, test_paired_solves_...[qp_supernodes]: 8 passed
    (e) refine_finish without the memset of a reused norm set: NOTHING of the scenarios above fails (23 passed, many_rounds
        among them: its norms grow from round 3 on and the larger norm wins in a set, cleared or not), nor the 8 existing
        cases; hence the fixture qp_3000_slow, whose norms fall: with it both cases of
        test_reused_norm_sets_while_the_norms_fall fail (15 rounds for 17), the 23 others pass
"""
import numpy as np
import pytest

from tests import ir_fixtures as F
from tests import ir_ref

pytestmark = pytest.mark.gpu

SCENARIOS = ["tol0", "tol_late", "accept_stop", "reject", "reject_first", "reject_at_limit", "worse_accepted", "many_rounds",
             "limit_30", "limit_31", "off", "zero_iter"]


def _fixed(hip, ks):
    return hip.debug_counter(ks, "irs_fixed_launches")


# path -> (fixture, environment at creation, result over the right-hand side)
PATHS = {
    "irs_fixed-5x170": ("socp_5x170", {}, False),
    "irs_fixed-19x341": ("socp_19x341", {}, False),
    "irs_general-5x170": ("socp_5x170", {"CHIP_IRS_FLAGS": "11"}, False),
    "irs_general-19x341": ("socp_19x341", {"CHIP_IRS_FLAGS": "11"}, False),
    "irs_inplace-5x170": ("socp_5x170", {}, True),
    "bundle_ir-3x200": ("socp_3x200", {}, False),
    "bundle_ir-three_row_top": ("three_row_top", {"CHIP_NO_IR_SF": "1"}, False),  # (by default k_bundle_irs takes these bundles)
    "gstep-ragged_forest": ("ragged_forest", {}, False),
    "host-qp_3000": ("qp_3000", {}, False),
    # the unfused retry of a fused solve (test_fused_solve_timeout_falls_back): the last workgroup of every fused launch leaves at
    # once, the barrier times out (about 2 s), the solve is repeated launch by launch with the decisions on the host
    "retry-12x300": ("socp_12x300", {"CHIP_IR_TEST_DROP": "1"}, False),
}
# the retry waits out a time-out per solve: the scenarios whose result a leftover of the abandoned fused launch could spoil
RETRY_SCENARIOS = ["reject", "reject_first", "reject_at_limit", "worse_accepted", "many_rounds", "off"]
_STATE = {}


def _state(hip, oracle, path, monkeypatch):
    """the path's handle (factored once at the fixture's scaling point), the reference under its permutation, the
    scenarios and what they must do; asserts that the handle is of the path's kind"""
    if path not in _STATE:
        fixture, env, _ = PATHS[path]
        for k, v in env.items():
            # (the environment is parsed at every handle creation; CHIP_IR_TEST_DROP and CHIP_NO_IR_SF are kept by the handle,
            # CHIP_IRS_FLAGS is read per launch from the last parse: test_refinement_decisions sets it again around its solves)
            monkeypatch.setenv(k, v)
        pr = F.problem(fixture)
        P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
        A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
        ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=F.hip_settings(hip))
        assert ks.update_scaling(pr["s"], pr["z"]) and ks.update()
        ref = F.Reference(oracle, pr, perm=ks.perm)
        assert np.max(np.abs(ks.values() - ref.triu[2])) <= 1e-13 * np.max(np.abs(ref.triu[2]))
        assert ks.linear_solver_info().regularize_count == 0 and ref.ko.ldl_regularize_count() == 0
        assert abs(ks.linear_solver_info().last_regularizer - F.EPS) <= 1e-15
        kind = path.split("-")[0]
        wm = ks.work_model()
        if kind.startswith("irs"):
            assert ks.step_kernels() & 4, path
            assert hip.debug_counter(ks, "irs_desc_bundles") == wm["n_bundles"], path
        elif kind == "bundle_ir":
            assert wm["fused_threads"] > 0 and not ks.step_kernels() & 5, (path, wm, ks.step_kernels())
            # (rows of the folded top: 3 x 200 keeps its 7 last columns there, so both fixtures go through curt / candt)
            assert ks.N - ks.NF == (3 if fixture == "three_row_top" else 7) and not ks.supernodes(), (path, ks.N - ks.NF)
        elif kind == "gstep":
            assert wm["fold_groups"] >= 10 and ks.step_kernels() == 3, (path, wm, ks.step_kernels())
        elif kind == "retry":
            assert wm["fused_threads"] > 0 and ks.N - ks.NF == 1, (path, wm)
        else:
            assert wm["fused_threads"] == 0 and len(ks.supernodes()) > 0, (path, wm)
        sc, k = F.scenarios(ref)
        _STATE[path] = dict(pr=pr, ks=ks, ref=ref, sc=sc, want=F.expected(k), traces={}, worst=0.0)
    return _STATE[path]


def _solve(hip, ks, pr, rx, rz, inplace):
    n, m = pr["n"], pr["m"]
    if inplace:
        buf = hip.DeviceArray(np.concatenate([rx, rz]))
        ks.setrhs_dev(buf.ptr, buf.ptr + 8 * n)
        ok = ks.solve_dev(buf.ptr, buf.ptr + 8 * n)
        return ok, buf.numpy()
    d_rx, d_rz, out = hip.DeviceArray(rx), hip.DeviceArray(rz), hip.DeviceArray(n + m)
    ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
    ok = ks.solve_dev(out.ptr, out.ptr + 8 * n)
    return ok, out.numpy()


def _check(st, label, got, rounds, tr, kind):
    """the returned vector against the accepted iterate and against every other iterate of the right-hand side"""
    ref = st["ref"]
    nv = ref.nvis
    assert rounds == tr["rounds"], (label, rounds, tr["rounds"])
    base = ref.base(kind)["iterates"]
    xa = tr["iterates"][tr["accepted"]][:nv]
    scale = max(1.0, float(np.max(np.abs(xa))))
    d_acc = float(np.max(np.abs(got - xa)))
    d_other = min([float(np.max(np.abs(got - x[:nv]))) for j, x in enumerate(base) if j != tr["accepted"]])
    ratio = d_acc / d_other
    st["worst"] = max(st["worst"], ratio)
    print("%s: rounds %d, accepted iterate %d (%s); rel. err %.3e, distance ratio %.3e (worst of the path %.3e)"
          % (label, rounds, tr["accepted"], tr["why_stopped"], d_acc / scale, ratio, st["worst"]))
    assert d_acc <= F.TOL * scale, (label, d_acc / scale)
    assert 4.0 * d_acc <= d_other, (label, d_acc, d_other)


def _cases():
    return [(p, s) for p in PATHS for s in (RETRY_SCENARIOS if p.startswith("retry") else SCENARIOS)]


@pytest.mark.parametrize("path,scenario", _cases(), ids=lambda v: v)
def test_refinement_decisions(hip, oracle, path, scenario, monkeypatch):
    st = _state(hip, oracle, path, monkeypatch)
    try:
        for k, v in PATHS[path][1].items():
            hip.debug_set_switch(k, v)  # (the switch table as this path's launches must see it, whatever ran before)
        _scenario(hip, st, path, scenario)
    finally:
        for k in PATHS[path][1]:
            hip.debug_set_switch(k, None)


def _scenario(hip, st, path, scenario):
    ks, ref, pr = st["ks"], st["ref"], st["pr"]
    inplace = PATHS[path][2]
    kind, ir = st["sc"][scenario]
    label = "%s / %s" % (path, scenario)
    rx, rz = F.rhs(pr, kind)
    tr = ref.trace(ref.full(rx, rz), ir)
    F.check_conditions(ref, label, kind, ir, tr, st["want"][scenario])
    fixed0, fb0 = _fixed(hip, ks), ks.fused_fallbacks()
    ks.set_settings(F.hip_settings(hip, ir))
    ok, got = _solve(hip, ks, pr, rx, rz, inplace)
    assert ok, label
    _check(st, label, got, ks.linear_solver_info().last_ir_iterations, tr, kind)
    # the next launch on the same handle: another right-hand side that stops in round 0 with its own x0
    ir0 = st["sc"]["tol0"][1]
    ox, oz = F.rhs(pr, "other")
    if "other" not in st["traces"]:
        st["traces"]["other"] = ref.trace(ref.full(ox, oz), ir0)
        F.check_conditions(ref, path + " / other", "other", ir0, st["traces"]["other"], (0, 0, "tolerance"))
    ks.set_settings(F.hip_settings(hip, ir0))
    ok, got = _solve(hip, ks, pr, ox, oz, inplace)
    assert ok, label
    _check(st, label + " / then tol0", got, ks.linear_solver_info().last_ir_iterations, st["traces"]["other"], "other")
    # the path that ran
    name = path.split("-")[0]
    if name == "retry":  # one abandoned fused launch and one retry per solve
        assert ks.fused_fallbacks() - fb0 == 2, (label, ks.fused_fallbacks() - fb0)
    elif name != "host":
        assert ks.fused_fallbacks() == fb0 == 0, label
    enabled = dict(F.DEFAULT_IR, **ir)["enable"]
    if name == "irs_fixed":
        assert _fixed(hip, ks) - fixed0 == (2 if enabled else 1), (label, _fixed(hip, ks) - fixed0)
    else:
        assert _fixed(hip, ks) == 0, label


@pytest.mark.parametrize("scenario", ["reject", "accept_stop", "many_rounds"])
def test_l1_solve_refined_decisions(hip, oracle, scenario):
    """chip_ldl_solve_refined (refine_begin / refine_finish on the L1 handle): the banded QP's K with its signs, the static
    regulariser put on for the refactor and taken off again (test_l1_fast_path_registered_sets_and_device_refinement)"""
    if "l1" not in _STATE:
        pr = F.problem("qp_3000")
        ref = F.Reference(oracle, pr, perm=F.host_perm(hip, pr))
        N = ref.N
        ldl = hip.HipDirectLDLSolver(hip.CscMatrix(N, N, *ref.triu), ref.dsigns, hip.Settings.default(), perm=ref.ko_perm(hip))
        dfull = ref.ko.kkt.map("diag_full", N)
        ldl.offset_values(dfull, F.EPS, ref.dsigns)
        assert ldl.refactor()
        ldl.offset_values(dfull, -F.EPS, ref.dsigns)
        assert ldl.linear_solver_info().regularize_count == 0
        sc, k = F.scenarios(ref)
        _STATE["l1"] = dict(pr=pr, ks=ldl, ref=ref, sc=sc, want=F.expected(k), traces={}, worst=0.0)
    st = _STATE["l1"]
    ldl, ref, pr = st["ks"], st["ref"], st["pr"]
    kind, ir = st["sc"][scenario]
    label = "l1-qp_3000 / %s" % scenario
    b = ref.full(*F.rhs(pr, kind))
    tr = ref.trace(b, ir)
    F.check_conditions(ref, label, kind, ir, tr, st["want"][scenario])
    x = np.zeros(ref.N)
    ok, rounds = ldl.solve_refined(x, b, F.hip_settings(hip, ir))
    assert ok, label
    _check(st, label, x[:ref.nvis], rounds, tr, kind)
    assert np.max(np.abs(x - tr["iterates"][tr["accepted"]])) <= F.TOL * max(1.0, np.max(np.abs(x))), label
    # the next solve on the same handle: another right-hand side that stops in round 0 with its own x0
    ir0 = st["sc"]["tol0"][1]
    bo = ref.full(*F.rhs(pr, "other"))
    if "other" not in st["traces"]:
        st["traces"]["other"] = ref.trace(bo, ir0)
        F.check_conditions(ref, "l1 / other", "other", ir0, st["traces"]["other"], (0, 0, "tolerance"))
    ok, rounds = ldl.solve_refined(x, bo, F.hip_settings(hip, ir0))
    assert ok, label
    _check(st, label + " / then tol0", x[:ref.nvis], rounds, st["traces"]["other"], "other")


PAIRS = {"pair-host-qp_3000": "qp_3000", "pair-irs-12x300": "socp_12x300"}


@pytest.mark.parametrize("order", ["tol0_first", "reject_first"])
@pytest.mark.parametrize("path", list(PAIRS))
def test_pair_members_take_different_rounds(hip, oracle, path, order):
    """chip_kkt_solve2_dev_enqueue on the level-scheduled handle (refine_begin_pair: two contexts) and on a fused handle
    (tests/test_bundle_pattern_gpu.py: _run(..., paired=True)): one member stops on tolerance in round 0, the other is
    refined to its rejection, in both orders; each against its own trace, its rounds read from a single solve of it"""
    if path not in _STATE:
        pr = F.problem(PAIRS[path])
        P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
        A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
        ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=F.hip_settings(hip))
        assert ks.update_scaling(pr["s"], pr["z"]) and ks.update()
        ref = F.Reference(oracle, pr, perm=ks.perm)
        assert ks.linear_solver_info().regularize_count == 0
        if "irs" in path:
            assert ks.step_kernels() & 4, path
        else:
            assert ks.work_model()["fused_threads"] == 0 and len(ks.supernodes()) > 0, path
        ir, k = F.pair_settings(ref)
        traces = {}
        for kind, want in (("other", (0, 0, "tolerance")), ("big", (k + 1, k, "stop_ratio"))):
            traces[kind] = ref.trace(ref.full(*F.rhs(pr, kind)), ir)
            F.check_conditions(ref, "%s / %s" % (path, kind), kind, ir, traces[kind], want)
        ks.set_settings(F.hip_settings(hip, ir))
        _STATE[path] = dict(pr=pr, ks=ks, ref=ref, traces=traces, worst=0.0)
    st = _STATE[path]
    ks, pr = st["ks"], st["pr"]
    n, m = pr["n"], pr["m"]
    kinds = ["other", "big"] if order == "tol0_first" else ["big", "other"]
    dev = [tuple(hip.DeviceArray(v) for v in F.rhs(pr, kind)) + (hip.DeviceArray(n + m),) for kind in kinds]
    (ra, za, la), (rb, zb, lb) = dev
    ks.solve2_dev_enqueue(ra.ptr, za.ptr, la.ptr, la.ptr + 8 * n, rb.ptr, zb.ptr, lb.ptr, lb.ptr + 8 * n)
    uok, sok = ks.collect()
    assert uok and list(sok) == [True, True], (path, order)
    for kind, (d_rx, d_rz, out) in zip(kinds, dev):
        again = hip.DeviceArray(n + m)
        ks.setrhs_dev(d_rx.ptr, d_rz.ptr)
        assert ks.solve_dev(again.ptr, again.ptr + 8 * n)
        rounds = ks.linear_solver_info().last_ir_iterations
        _check(st, "%s / %s / %s alone" % (path, order, kind), again.numpy(), rounds, st["traces"][kind], kind)
        _check(st, "%s / %s / %s in the pair" % (path, order, kind), out.numpy(), rounds, st["traces"][kind], kind)
    if "irs" in path:
        assert ks.fused_fallbacks() == 0, path


@pytest.mark.parametrize("handle", ["kkt", "l1"])
def test_reused_norm_sets_while_the_norms_fall(hip, oracle, handle):
    """refine_finish reuses the norm sets from round 15 on.  On tests/ir_fixtures.py's qp_3000_slow every round improves by
    1.4 and round 15's norm is 80 times smaller than that of round 2, whose set it takes: a set not cleared first keeps the
    larger norm, round 15 is rejected and the solve ends with 15 rounds and iterate 14 (many_rounds cannot show this: its
    norms GROW, and the larger norm wins in a set either way)"""
    pr = F.problem("qp_3000_slow")
    if handle == "kkt":
        P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
        A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
        ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=F.hip_settings(hip, F.SLOW_IR))
        assert ks.update_scaling(pr["s"], pr["z"]) and ks.update()
        assert ks.work_model()["fused_threads"] == 0 and len(ks.supernodes()) > 0
        ref = F.Reference(oracle, pr, perm=ks.perm)
    else:
        ref = F.Reference(oracle, pr, perm=F.host_perm(hip, pr))
        ks = hip.HipDirectLDLSolver(hip.CscMatrix(ref.N, ref.N, *ref.triu), ref.dsigns, hip.Settings.default(), perm=ref.perm)
        dfull = ref.ko.kkt.map("diag_full", ref.N)
        ks.offset_values(dfull, F.EPS, ref.dsigns)
        assert ks.refactor()
        ks.offset_values(dfull, -F.EPS, ref.dsigns)
    assert ks.linear_solver_info().regularize_count == 0
    st = dict(ref=ref, worst=0.0)
    rx, rz = F.rhs(pr, "late")
    tr = ref.trace(ref.full(rx, rz), F.SLOW_IR)
    F.check_conditions(ref, "slow / " + handle, "late", F.SLOW_IR, tr, (F.MANY, F.MANY, "limit"))
    if handle == "kkt":
        ok, got = _solve(hip, ks, pr, rx, rz, False)
        rounds = ks.linear_solver_info().last_ir_iterations
    else:
        got = np.zeros(ref.N)
        ok, rounds = ks.solve_refined(got, ref.full(rx, rz), F.hip_settings(hip, F.SLOW_IR))
        got = got[:ref.nvis]
    assert ok
    _check(st, "slow / " + handle, got, rounds, tr, "late")
