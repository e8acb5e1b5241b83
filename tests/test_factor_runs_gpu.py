"""-m gpu: the flat bundle factorisation over run-coded update records (bundle_factor.hip: k_bundle_factor_runs; the host
side: tests/test_factor_runs_host.py) against the CPU oracle on the same inputs and the same permutation -- L and D entry
by entry, the pivot bookkeeping, a second refactor at other scalings, refined solves -- and against the same handle
built with CHIP_NO_FACTOR_RUNS (the plain records, k_bundle_factor_flat)."""
import ctypes as C

import numpy as np
import pytest

from tests import problems

pytestmark = pytest.mark.gpu

TOL = 1e-8               # the suite's bound on the refined KKT solution against the oracle (tests/test_gpu_parity.py)
TOL_D, TOL_L = 1e-10, 1e-9  # the factor-parity bounds of tests/test_gpu_parity.py (test_ldl_random_quasidefinite)

# name -> (problem, environment of the handle, the run kernel takes its refactors)
CASES = {
    "bs63": (lambda: problems.portfolio_socp(3, 63, seed=3), {}, False),
    "bs64": (lambda: problems.portfolio_socp(3, 64, seed=3), {}, True),
    "bs65": (lambda: problems.portfolio_socp(3, 65, seed=3), {}, True),
    "bs200": (lambda: problems.portfolio_socp(4, 200, seed=3), {}, True),
    "bs1100": (lambda: problems.portfolio_socp(2, 1100, seed=3), {"CHIP_TARGET_WG": "0"}, True),  # runs of 1100 > 1024 threads
    "bs20_min4": (lambda: problems.portfolio_socp(3, 20, seed=3), {"CHIP_FACTOR_RUN_MIN": "4"}, True),  # runs and records share a level
    "irregular": (lambda: problems.random_qp(3000, 6000, band=30), {}, False),
}


def relerr(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def _solvers(hip, oracle, pr, settings=None):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=settings)
    cones = oracle.Cones(pr["cones"])
    ost = oracle.Settings.default()
    if settings is not None:
        ost.dynamic_reg_eps = settings.dynamic_regularization_eps
        ost.dynamic_reg_delta = settings.dynamic_regularization_delta
    ko = oracle.KKTSolver(pr["n"], pr["m"], pr["P"], pr["A"], cones, settings=ost, perm=ks.perm)
    return ks, ko, cones


def _oracle_factor(oracle, ko):
    L = oracle.lib()
    L.orc_kktsolver_ldl.restype = C.c_void_p
    f = C.c_void_p(L.orc_kktsolver_ldl(ko._h))
    L.orc_qdldl_nnzL.restype = C.c_int64
    L.orc_qdldl_Lx.restype = C.POINTER(C.c_double)
    L.orc_qdldl_D.restype = C.POINTER(C.c_double)
    nnzL = int(L.orc_qdldl_nnzL(f))
    return (np.ctypeslib.as_array(L.orc_qdldl_Lx(f), shape=(nnzL,)).copy(), np.ctypeslib.as_array(L.orc_qdldl_D(f), shape=(ko.N,)).copy(),
            int(L.orc_qdldl_regularize_count(f)), int(L.orc_qdldl_positive_inertia(f)))


def _walk(hip, oracle, pr, settings, label, nrhs=1):
    """two refactors at different scalings on a fresh handle, each against the oracle: L, D, counts, refined solves;
    -> (run kernel?, [(Lx, D, regularize_count, positive_inertia, solutions), ...])"""
    ks, ko, cones = _solvers(hip, oracle, pr, settings)
    runs_on = int(hip.debug_counter(ks, "factor_run_kernel"))
    out = []
    rng = np.random.default_rng(7)
    for it in range(2):  # (the second refactor: other values through the same tables, nothing stale in the value store)
        s_, z_ = pr["s"] * (1.0 + 0.3 * it), pr["z"] / (1.0 + 0.2 * it)
        assert ks.update_scaling(s_, z_) and cones.update_scaling(s_, z_)
        assert ks.update() and ko.update()
        Lx, D = hip.debug_kkt_factors(ks)
        Lo, Do, reg_o, pos_o = _oracle_factor(oracle, ko)
        info = ks.linear_solver_info()
        eD, eL = relerr(D, Do), relerr(Lx, Lo) if len(Lo) == len(Lx) else float("nan")
        print("%s refactor %d: run kernel %d, rel. err of D %.3e, of L %.3e, regularised pivots %d (oracle %d)" %
              (label, it, runs_on, eD, eL, info.regularize_count, reg_o))
        if not ks.supernodes():  # (chain supernodes pad the pattern: the entries do not line up one to one)
            assert len(Lx) == len(Lo) and eL <= TOL_L, (label, it, eL)
        assert eD <= TOL_D, (label, it, eD)
        assert info.regularize_count == reg_o and info.positive_inertia == pos_o, (label, it)
        sols = []
        for _ in range(nrhs):
            rx, rz = rng.standard_normal(pr["n"]), rng.standard_normal(pr["m"])
            ks.setrhs(rx, rz)
            ko.setrhs(rx, rz)
            x, z = np.zeros(pr["n"]), np.zeros(pr["m"])
            assert ks.solve(x, z)
            ok, xo, zo = ko.solve()
            err = relerr(np.concatenate([x, z]), np.concatenate([xo, zo]))
            print("%s refactor %d: refined solve against the oracle %.3e" % (label, it, err))
            assert ok and err <= TOL, (label, it, err)
            sols.append(np.concatenate([x, z]))
        out.append((Lx, D, info.regularize_count, info.positive_inertia, sols))
    return runs_on, out


@pytest.mark.parametrize("case", sorted(CASES))
def test_run_coded_factorisation_against_oracle_and_plain_records(hip, oracle, case, monkeypatch):
    mk, env, has_runs = CASES[case]
    pr = mk()
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read when a handle is created)
    on, a = _walk(hip, oracle, pr, None, case)
    monkeypatch.setenv("CHIP_NO_FACTOR_RUNS", "1")
    off, b = _walk(hip, oracle, pr, None, case + " / plain records")
    assert off == 0 and on == (1 if has_runs else 0), (case, on, off)
    for (La, Da, ra, pa, sa), (Lb, Db, rb, pb, sb) in zip(a, b):
        assert ra == rb and pa == pb  # (equal pivot bookkeeping; every update call above returned true: clean status words)
        assert relerr(Da, Db) <= TOL_D and relerr(La, Lb) <= TOL_L  # (summation order only)
        for x, y in zip(sa, sb):
            assert relerr(x, y) <= TOL


def test_regularised_pivots_in_the_run_kernel(hip, oracle):
    """as test_zero_pivot_regularised (tests/test_gpu_parity.py), inside the run kernel.  This pattern has no exact zero
    pivot to offer, even with P = 0 and the static regulariser off: the columns of x are eliminated behind their
    Nonnegative rows and have received an update by then.  So the threshold of the pivot rule is raised instead: every
    pivot with d * sign < 0.3 is replaced by 0.5 * sign -- the branch a zero pivot takes -- as many as in the oracle, and
    the factor and the solves still agree with it."""
    pr = problems.portfolio_socp(3, 65, seed=3)
    st = hip.Settings.default(dynamic_regularization_eps=0.3, dynamic_regularization_delta=0.5)
    on, a = _walk(hip, oracle, pr, st, "regularised pivots")
    assert on == 1
    assert all(r[2] >= 1 for r in a)
