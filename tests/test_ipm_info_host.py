"""The interior-point loop's scalar logic (csrc/ipm_info.hpp), shared by chip_solver and chip_batch, checked on the host
(no GPU needed) through chip_debug_ipm_termination / chip_debug_ipm_info_update: DefaultInfo's check_termination,
post_process and update (default/info.rs) on hand-built inputs, one per deciding branch.  Every expected status is a
literal of the SolverStatus numbering of include/clarabel_hip.h, written from the reference's text; the comment names
the line of info.rs that decides it."""
import ctypes as C

import pytest

# SolverStatus (clarabel_hip.h: CHIP_SOLVER_*)
UNSOLVED, SOLVED, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, ALMOST_SOLVED = 0, 1, 2, 3, 4
ALMOST_PRIMAL_INFEASIBLE, ALMOST_DUAL_INFEASIBLE, MAX_ITERATIONS, MAX_TIME = 5, 6, 7, 8
NUMERICAL_ERROR, INSUFFICIENT_PROGRESS = 9, 10

FIELDS = ["cost_primal", "cost_dual", "res_primal", "res_dual", "res_primal_inf", "res_dual_inf", "gap_abs", "gap_rel",
          "ktratio", "prev_cost_primal", "prev_cost_dual", "prev_res_primal", "prev_res_dual", "prev_gap_abs",
          "prev_gap_rel", "r_tau", "dot_qx", "dot_bz", "dot_sz", "dot_xPx", "status"]

# an iterate that meets no criterion: gaps and residuals of 1, no growth against the previous iterate, a moderate
# kappa / tau, dots that rule both infeasibility certificates out
NOTHING = dict(cost_primal=1.0, cost_dual=0.0, res_primal=1.0, res_dual=1.0, res_primal_inf=1.0, res_dual_inf=1.0,
               gap_abs=1.0, gap_rel=1.0, ktratio=0.5, prev_cost_primal=1.0, prev_cost_dual=0.0, prev_res_primal=10.0,
               prev_res_dual=10.0, prev_gap_abs=1.0, prev_gap_rel=1.0, r_tau=0.0, dot_qx=0.0, dot_bz=0.0, dot_sz=0.0,
               dot_xPx=0.0, status=float(UNSOLVED))
# meets the full tolerances below
CONVERGED = dict(NOTHING, gap_abs=1e-9, gap_rel=1e-9, res_primal=1e-9, res_dual=1e-9)
# meets only the reduced ones
NEARLY = dict(NOTHING, gap_abs=1e-5, gap_rel=1e-5, res_primal=1e-5, res_dual=1e-5)
# kappa / tau past 1000 / tol_ktratio = 1e9 (full), past 1000 / reduced_tol_ktratio = 1e7 only (reduced)
KT_FULL, KT_REDUCED = 1e10, 1e8


def _settings(hip, **kw):
    # the reference's default tolerances, spelled out so that the expectations below do not depend on the defaults
    base = dict(max_iter=200, time_limit=float("inf"), tol_gap_abs=1e-8, tol_gap_rel=1e-8, tol_feas=1e-8,
                tol_infeas_abs=1e-8, tol_infeas_rel=1e-8, tol_ktratio=1e-6, reduced_tol_gap_abs=5e-5,
                reduced_tol_gap_rel=5e-5, reduced_tol_feas=1e-4, reduced_tol_infeas_abs=5e-12,
                reduced_tol_infeas_rel=5e-5, reduced_tol_ktratio=1e-4)
    base.update(kw)
    return hip.SolverSettings.default(**base)


def _status(hip, info, iter=5, iterations=None, solve_time=1.0, post=False, **settings):
    L = hip.lib()
    L.chip_debug_ipm_termination.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_double,
                                             C.c_int32]
    L.chip_debug_ipm_termination.restype = C.c_int32
    assert sorted(info) == sorted(FIELDS)
    flat = (C.c_double * len(FIELDS))(*[info[f] for f in FIELDS])
    st = _settings(hip, **settings)
    return L.chip_debug_ipm_termination(C.byref(st), flat, iter, iter if iterations is None else iterations,
                                        solve_time, int(post))


TERMINATION = [
    # ---- check_convergence (info.rs:340-363)
    ("solved_by_gap_abs_alone", dict(CONVERGED, gap_rel=1.0), {}, SOLVED),  # info.rs:366, first operand of ||
    ("solved_by_gap_rel_alone", dict(CONVERGED, gap_abs=1.0), {}, SOLVED),  # info.rs:366, second operand
    ("not_solved_without_a_gap", dict(CONVERGED, gap_abs=1.0, gap_rel=1.0), {}, UNSOLVED),  # info.rs:366
    ("not_solved_res_primal", dict(CONVERGED, res_primal=1e-7), {}, UNSOLVED),  # info.rs:367
    ("not_solved_res_dual", dict(CONVERGED, res_dual=1e-7), {}, UNSOLVED),  # info.rs:368
    ("solved_at_ktratio_one", dict(CONVERGED, ktratio=1.0), {}, SOLVED),  # info.rs:353 (<=)
    ("not_solved_when_ktratio_above_one", dict(CONVERGED, ktratio=2.0), {}, UNSOLVED),  # info.rs:353
    ("primal_infeasible", dict(NOTHING, ktratio=KT_FULL, dot_bz=-1.0, res_primal_inf=1e-9), {},
     PRIMAL_INFEASIBLE),  # info.rs:357 with 377-378
    ("dual_infeasible", dict(NOTHING, ktratio=KT_FULL, dot_qx=-1.0, res_dual_inf=1e-9), {},
     DUAL_INFEASIBLE),  # info.rs:359 with 387-388
    ("primal_wins_when_both_qualify", dict(NOTHING, ktratio=KT_FULL, dot_bz=-1.0, res_primal_inf=1e-9, dot_qx=-1.0,
                                           res_dual_inf=1e-9), {}, PRIMAL_INFEASIBLE),  # info.rs:357 before 359
    ("no_certificate_at_moderate_ktratio", dict(NOTHING, ktratio=KT_REDUCED, dot_bz=-1.0, res_primal_inf=1e-9,
                                                dot_qx=-1.0, res_dual_inf=1e-9), {}, UNSOLVED),  # info.rs:356
    ("no_primal_certificate_small_bz", dict(NOTHING, ktratio=KT_FULL, dot_bz=-1e-9, res_primal_inf=0.0), {},
     UNSOLVED),  # info.rs:377
    ("no_dual_certificate_large_residual", dict(NOTHING, ktratio=KT_FULL, dot_qx=-1.0, res_dual_inf=1e-7), {},
     UNSOLVED),  # info.rs:388
    # ---- poor progress (info.rs:194-217): the residual grew, kappa / tau < 100 eps, the PREVIOUS gap was converged
    ("insufficient_progress_prev_gap_abs", dict(NOTHING, res_dual=2.0, prev_res_dual=1.0, ktratio=1e-15,
                                                prev_gap_abs=1e-9), {}, INSUFFICIENT_PROGRESS),  # info.rs:199-203
    ("insufficient_progress_prev_gap_rel", dict(NOTHING, res_primal=2.0, prev_res_primal=1.0, ktratio=1e-15,
                                                prev_gap_rel=1e-9), {}, INSUFFICIENT_PROGRESS),  # info.rs:201
    ("progress_rule_needs_a_converged_prev_gap", dict(NOTHING, res_dual=2.0, prev_res_dual=1.0, ktratio=1e-15), {},
     UNSOLVED),  # info.rs:200-201
    ("progress_rule_needs_a_tiny_ktratio", dict(NOTHING, res_dual=2.0, prev_res_dual=1.0, ktratio=1e-13,
                                                prev_gap_abs=1e-9), {}, UNSOLVED),  # info.rs:199 (100 eps = 2.2e-14)
    ("progress_rule_needs_growth", dict(NOTHING, ktratio=1e-15, prev_gap_abs=1e-9), {}, UNSOLVED),  # info.rs:196
    # ---- going backwards (info.rs:208-215): a residual above 100 tol_feas grew a hundredfold
    ("insufficient_progress_res_dual_x100", dict(NOTHING, res_dual=1.0, prev_res_dual=1e-3), {},
     INSUFFICIENT_PROGRESS),  # info.rs:209-210
    ("insufficient_progress_res_primal_x100", dict(NOTHING, res_primal=1.0, prev_res_primal=1e-3), {},
     INSUFFICIENT_PROGRESS),  # info.rs:211-212
    ("x100_rule_not_at_ktratio_one", dict(NOTHING, res_dual=1.0, prev_res_dual=1e-3, ktratio=1.0, gap_abs=1.0), {},
     UNSOLVED),  # info.rs:208
    ("x100_rule_needs_a_hundredfold", dict(NOTHING, res_dual=1.0, prev_res_dual=0.02), {}, UNSOLVED),  # info.rs:210
    ("x100_rule_needs_res_above_100_tol_feas", dict(NOTHING, res_dual=1e-7, prev_res_dual=1e-10), {},
     UNSOLVED),  # info.rs:209 (100 tol_feas = 1e-6)
    # ---- neither rule before the second iteration (info.rs:195)
    ("no_progress_rule_at_iter_1", dict(NOTHING, res_dual=2.0, prev_res_dual=1.0, ktratio=1e-15, prev_gap_abs=1e-9),
     dict(iter=1), UNSOLVED),
    ("no_x100_rule_at_iter_1", dict(NOTHING, res_dual=1.0, prev_res_dual=1e-3), dict(iter=1), UNSOLVED),
    ("no_x100_rule_at_iter_0", dict(NOTHING, res_primal=1.0, prev_res_primal=0.0), dict(iter=0), UNSOLVED),
    # ---- limits (info.rs:221-227)
    ("max_iterations", NOTHING, dict(iterations=200), MAX_ITERATIONS),  # info.rs:222
    ("max_iterations_is_an_equality", NOTHING, dict(iterations=201), UNSOLVED),  # info.rs:222 (==)
    ("max_time", NOTHING, dict(solve_time=2.0, time_limit=1.0), MAX_TIME),  # info.rs:224
    ("max_time_is_strict", NOTHING, dict(solve_time=1.0, time_limit=1.0), UNSOLVED),  # info.rs:224 (>)
    ("max_iterations_before_max_time", NOTHING, dict(iterations=200, solve_time=2.0, time_limit=1.0),
     MAX_ITERATIONS),  # info.rs:222 before the else of 224
    ("solved_before_the_limits", dict(CONVERGED), dict(iterations=200, solve_time=2.0, time_limit=1.0),
     SOLVED),  # info.rs:221
    ("insufficient_progress_before_the_limits", dict(NOTHING, res_dual=1.0, prev_res_dual=1e-3),
     dict(iterations=200), INSUFFICIENT_PROGRESS),  # info.rs:221
    # ---- check_termination uses the full tolerances only (info.rs:190)
    ("reduced_tolerances_do_not_terminate", NEARLY, {}, UNSOLVED),
    ("meets_nothing", NOTHING, {}, UNSOLVED),  # info.rs:230
]


@pytest.mark.parametrize("name,info,kw,expected", TERMINATION, ids=[t[0] for t in TERMINATION])
def test_check_termination(hip, name, info, kw, expected):
    assert _status(hip, info, **kw) == expected


ALMOST_PINF = dict(NOTHING, ktratio=KT_REDUCED, dot_bz=-1.0, res_primal_inf=1e-6)
ALMOST_DINF = dict(NOTHING, ktratio=KT_REDUCED, dot_qx=-1.0, res_dual_inf=1e-6)
POST_PROCESS = [
    # info.rs:99-103: an errored status (NumericalError, InsufficientProgress: core/solver.rs:57-63), MaxIterations or
    # MaxTime is checked again with the reduced tolerances (info.rs:314-323)
    ("max_iterations_becomes_almost_solved", dict(NEARLY, status=MAX_ITERATIONS), ALMOST_SOLVED),  # info.rs:100, 321
    ("max_time_becomes_almost_solved", dict(NEARLY, status=MAX_TIME), ALMOST_SOLVED),  # info.rs:101
    ("insufficient_progress_becomes_almost_solved", dict(NEARLY, status=INSUFFICIENT_PROGRESS),
     ALMOST_SOLVED),  # info.rs:99
    ("numerical_error_becomes_almost_primal_infeasible", dict(ALMOST_PINF, status=NUMERICAL_ERROR),
     ALMOST_PRIMAL_INFEASIBLE),  # info.rs:99, 322
    ("numerical_error_becomes_almost_dual_infeasible", dict(ALMOST_DINF, status=NUMERICAL_ERROR),
     ALMOST_DUAL_INFEASIBLE),  # info.rs:99, 323
    ("almost_primal_wins_when_both_qualify", dict(ALMOST_PINF, dot_qx=-1.0, res_dual_inf=1e-6, status=NUMERICAL_ERROR),
     ALMOST_PRIMAL_INFEASIBLE),  # info.rs:357 before 359
    ("max_iterations_stays_when_nothing_is_met", dict(NOTHING, status=MAX_ITERATIONS), MAX_ITERATIONS),
    ("numerical_error_stays_when_nothing_is_met", dict(NOTHING, status=NUMERICAL_ERROR), NUMERICAL_ERROR),
    # every other status is final: no second check
    ("solved_is_not_rechecked", dict(NEARLY, status=SOLVED), SOLVED),  # info.rs:99-101
    ("primal_infeasible_is_not_rechecked", dict(NEARLY, status=PRIMAL_INFEASIBLE), PRIMAL_INFEASIBLE),
    ("unsolved_is_not_rechecked", dict(NEARLY, status=UNSOLVED), UNSOLVED),
]


@pytest.mark.parametrize("name,info,expected", POST_PROCESS, ids=[t[0] for t in POST_PROCESS])
def test_post_process(hip, name, info, expected):
    assert _status(hip, info, post=True) == expected


def test_reduced_inputs_are_below_the_full_tolerances_only(hip):
    """the post-process inputs above decide nothing under check_termination: it is the reduced set that moves them"""
    for info in (NEARLY, ALMOST_PINF, ALMOST_DINF):
        assert _status(hip, info) == UNSOLVED


def test_info_update_powers_of_two(hip):
    """DefaultInfo::update (info.rs:121-176) on powers of two: every operation is exact, so the nine scalars are
    literals.  tau = 2, kappa = 4, c = 4; the hook takes the squared norms"""
    L = hip.lib()
    L.chip_debug_ipm_info_update.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)] + [C.c_double] * 5
    L.chip_debug_ipm_info_update.restype = C.c_int32
    info = dict(NOTHING, dot_qx=8.0, dot_bz=-32.0, dot_xPx=32.0)
    flat = (C.c_double * len(FIELDS))(*[info[f] for f in FIELDS])
    # the norms 4, 8, 2, 16, 2, 1, 8, 32 of (x, d), (z, e), (s, einv), (rx_inf, dinv), (Px, dinv), (rz_inf, einv),
    # (rz, einv), (rx, dinv)
    sq = (C.c_double * 8)(16.0, 64.0, 4.0, 256.0, 4.0, 1.0, 64.0, 1024.0)
    assert L.chip_debug_ipm_info_update(flat, sq, 2.0, 4.0, 4.0, 13.0, 5.0) == 0  # normq = 13, normb = 5
    got = dict(zip(FIELDS, flat))
    # xPx tinv^2 / 2 = 32 / 4 / 2 = 4 (info.rs:138)
    assert got["cost_primal"] == 2.0  # (8 / 2 + 4) / 4 (info.rs:139)
    assert got["cost_dual"] == 3.0  # (32 / 2 - 4) / 4 (info.rs:140)
    # normx = 4, normz = 8 / 4 = 2, norms = 2 (info.rs:145-147)
    assert got["res_primal_inf"] == 2.0  # (16 / 4) / max(1, 2) (info.rs:150)
    assert got["res_dual_inf"] == 0.5  # max(2 / max(1, 4), 1 / max(1, 4 + 2)) (info.rs:151-154)
    # normx = 2, normz = 1, norms = 1 (info.rs:157-159)
    assert got["res_primal"] == 0.5  # 8 / 2 / max(1, 5 + 2 + 1) (info.rs:162-163)
    assert got["res_dual"] == 0.25  # 32 / 2 / 4 / max(1, 13 + 2 + 1) (info.rs:164-165)
    assert got["gap_abs"] == 1.0  # |2 - 3| (info.rs:168)
    assert got["gap_rel"] == 0.5  # 1 / max(1, min(2, 3)) (info.rs:169-173)
    assert got["ktratio"] == 2.0  # 4 / 2 (info.rs:176)
    # the previous iterate's scalars and the dots are inputs only
    for f in FIELDS[9:]:
        assert got[f] == info[f], f


def test_hooks_are_absent_from_the_ship_build(hip):
    test, ship = C.CDLL(hip.LIB_PATH), C.CDLL(hip.SHIP_LIB_PATH)
    for sym in ("chip_debug_ipm_termination", "chip_debug_ipm_info_update"):
        assert hasattr(test, sym), sym
        assert not hasattr(ship, sym), sym
