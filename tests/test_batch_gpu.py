"""The batched L4 solver (chip_batch_*, HipBatchSolver) on the MI355X: refusals, the per-member equilibration, batches
of one and of identical copies against HipSolver, a heterogeneous batch of feasible and infeasible members with their
own statuses and iteration counts, order independence, the attribution of a NaN to one member, host synchronisations
that do not grow with the batch, and config 4's member problem at scale."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import e2e_problems as E
from tests.test_create_refusals_host import raw_batch_create as _raw_create

pytestmark = pytest.mark.gpu

ZERO, NN, SOC, EXP, POW, GENPOW, PSD = range(7)


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def _csc(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return (M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64))


def member(hip, pr):
    n, m = pr["n"], pr["m"]
    return (hip.CscMatrix(n, n, *pr["P"]), pr["q"], hip.CscMatrix(m, n, *pr["A"]), pr["b"], pr["cones"])


def single(hip, pr, **kw):
    P, q, A, b, cones = member(hip, pr)
    return hip.HipSolver(P, q, A, b, cones, hip.SolverSettings.default(**kw))


def batch(hip, prs, **kw):
    return hip.HipBatchSolver([member(hip, p) for p in prs], hip.SolverSettings.default(**kw))


# ---- the problems (Zero / Nonnegative / SecondOrder only), restated from tests/test_solver_gpu.py -------------------
def _qp_dual_inf():
    return dict(n=2, m=2, P=_csc(sp.triu(sp.csc_matrix(np.ones((2, 2))))), A=_csc(np.array([[1.0, 1.0], [1.0, 0.0]])),
                q=[1.0, -1.0], b=[1.0, 1.0], cones=[(NN, 2)])


def primal_infeasible():
    qp = E.basic_qp()
    qp["b"] = list(qp["b"])
    qp["b"][0] = qp["b"][3] = -1.0
    lp = E.basic_lp()
    lp["b"] = list(lp["b"])
    lp["b"][0] = lp["b"][3] = -1.0
    socp = E.basic_socp()
    socp["b"] = list(socp["b"])
    socp["b"][6] = -10.0
    A2 = np.array([[0.0, 1.0, 1.0], [0.0, 1.0, -1.0], [1.0, 2.0, -1.0], [2.0, -1.0, 3.0]])
    eq = dict(n=3, m=4, P=_csc(sp.identity(3)), A=_csc(A2), q=[0.0] * 3, b=[1.0] * 4, cones=[(ZERO, 4)])
    return [("pinf_qp", qp), ("pinf_lp", lp), ("pinf_socp", socp), ("pinf_eq", eq)]


def dual_infeasible():
    lp = E.basic_lp()
    A = [np.array(a) for a in lp["A"]]
    A[2][1] = 1.0
    eq = dict(E.basic_eq_constrained(), P=(np.array([0, 1, 2, 3]), np.array([0, 1, 2]), np.array([0.0, 1.0, 1.0])),
              q=[1.0, 1.0, 1.0])
    unc = dict(n=3, m=0, P=(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)),
               A=(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)), q=[1.0, 0.0, 0.0], b=[],
               cones=[])
    return [("dinf_qp", _qp_dual_inf()), ("dinf_lp", dict(lp, A=tuple(A))), ("dinf_eq", eq), ("dinf_unc", unc)]


def feasible():
    return [("basic_qp", E.basic_qp()), ("basic_lp", E.basic_lp()), ("basic_socp", E.basic_socp()),
            ("basic_socp_sparse", E.basic_socp(sparse_soc=True)), ("basic_eq", E.basic_eq_constrained()),
            ("basic_unc", E.basic_unconstrained())]


def hetero():
    return feasible() + primal_infeasible() + dual_infeasible()


def _hs35():
    import os
    from tests import json_problem
    return json_problem.load(os.path.join(os.path.dirname(__file__), "golden", "hs35_reference.json"))


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    if not a.size:
        return 0.0
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _mats(pr):
    n, m = pr["n"], pr["m"]
    A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n))
    Pu = sp.csc_matrix((pr["P"][2], pr["P"][1], pr["P"][0]), shape=(n, n))
    return Pu + sp.triu(Pu, 1).T, A


def _numel(c):
    return c[1]


def _check_certificate(pr, sol):
    P, A = _mats(pr)
    if sol.status == "PrimalInfeasible":
        z = sol.z
        bz = float(np.dot(pr["b"], z))
        assert bz < 0.0
        assert np.linalg.norm(A.T @ z, np.inf) <= 1e-6 * abs(bz)
        k = 0
        for c in pr["cones"]:
            v = z[k:k + c[1]]
            if c[0] == NN:
                assert float(np.max(-v, initial=0.0)) <= 1e-8 * max(1.0, np.linalg.norm(z, np.inf))
            elif c[0] == SOC:
                assert np.linalg.norm(v[1:]) - v[0] <= 1e-8 * max(1.0, np.linalg.norm(z, np.inf))
            k += c[1]
    else:
        x = sol.x
        qx = float(np.dot(pr["q"], x))
        assert qx < 0.0
        k = 0
        ax = A @ x if pr["m"] else np.zeros(0)
        for c in pr["cones"]:
            seg = ax[k:k + c[1]]
            viol = np.abs(seg) if c[0] == ZERO else np.maximum(seg, 0.0)
            assert float(np.max(viol, initial=0.0)) <= 1e-6 * abs(qx)
            k += c[1]
        assert np.linalg.norm(P @ x, np.inf) <= 1e-6 * abs(qx)


# ---- 1. refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["basic_expcone", "basic_powcone", "basic_genpowcone", "basic_sdp"])
def test_refuses_unsupported_cones(hipdev, name):
    with pytest.raises(hipdev.ChipError) as e:
        batch(hipdev, [E.basic_qp(), getattr(E, name)()])
    assert e.value.code == hipdev.ERR_UNSUPPORTED


@pytest.mark.parametrize("field", ["presolve_enable", "chordal_decomposition_enable"])
def test_refuses_transforms(hipdev, field):
    with pytest.raises(hipdev.ChipError) as e:
        batch(hipdev, [E.basic_qp(), E.basic_lp()], **{field: 1})
    assert e.value.code == hipdev.ERR_UNSUPPORTED


def test_refuses_entries_and_cones_across_members(hipdev):
    prs = [E.basic_qp(), E.basic_qp()]
    st = hipdev.batch_stack([member(hipdev, p) for p in prs])
    assert _raw_create(hipdev, st, [2, 2], [6, 6]) == 0
    # a partition that puts the column boundary elsewhere: P (and A) entries cross two members' blocks
    assert _raw_create(hipdev, st, [1, 3], [6, 6]) == hipdev.ERR_ARG
    # rows split inside the first member's second NN cone: an A entry and a cone cross the boundary
    assert _raw_create(hipdev, st, [2, 2], [4, 8]) == hipdev.ERR_ARG
    # a cone crossing the member boundary (the rows of A stay put): NN(3), NN(6), NN(3)
    assert _raw_create(hipdev, st, [2, 2], [6, 6], cones=[(NN, 3), (NN, 6), (NN, 3)]) == hipdev.ERR_ARG
    assert _raw_create(hipdev, st, [2, 2], [6, 5]) == hipdev.ERR_ARG  # parts do not add up


def test_refuses_empty_batch(hipdev):
    with pytest.raises(hipdev.ChipError) as e:
        hipdev.HipBatchSolver([])
    assert e.value.code == hipdev.ERR_ARG


# ---- 2. equilibration per member ----------------------------------------------------------------------------------
def test_equilibration_per_member(hipdev):
    q0 = dict(E.basic_qp(), q=[0.0, 0.0])  # no cost scaling, NN cones only: bitwise
    lp0 = dict(E.basic_lp(), q=[0.0, 0.0, 0.0])
    prs = [q0, lp0, E.basic_qp(), E.basic_socp(), E.basic_eq_constrained(), _hs35()]
    bs = batch(hipdev, prs)
    for k, pr in enumerate(prs):
        d, e, c = bs.equilibration(k)
        d0, e0, c0 = single(hipdev, pr).equilibration()
        if k < 2:
            assert np.array_equal(d, d0) and np.array_equal(e, e0) and c == c0, k
        else:
            assert _rel(d, d0) <= 1e-13 and _rel(e, e0) <= 1e-13 and abs(c - c0) <= 1e-13 * abs(c0), (k, c, c0)


# the batch reduces in another order than the single solver (chunked segments against one fixed grid) and factors its
# members inside a larger elimination forest, so the two paths agree to rounding that the last iterations amplify to a
# few 1e-9 on basic_socp (solved to 1e-8): solutions are compared to 1e-7, statuses and iteration counts exactly
TOL_PATH = 1e-7


# ---- 3. a batch of one and of identical copies --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["basic_qp", "basic_socp", "hs35"])
def test_batch_of_one_and_copies(hipdev, name):
    pr = _hs35() if name == "hs35" else getattr(E, name)()
    ref = single(hipdev, pr).solve()
    for copies in (1, 5):
        sols = batch(hipdev, [pr] * copies).solve()
        assert len(sols) == copies
        _, A = _mats(pr)
        for sol in sols:
            assert sol.status == ref.status and sol.iterations == ref.iterations, (copies, sol, ref)
            for a, b in ((sol.x, ref.x), (sol.s, ref.s), (A.T @ sol.z, A.T @ ref.z)):
                assert _rel(a, b) <= TOL_PATH, (copies, a, b)
            # basic_qp holds the two parallel rows x1 + x2 >= 1 and x1 + x2 <= 1: its z is unique only up to a shift
            # of both multipliers, along which a rounding-level difference of the path moves it further (A'z and
            # z0 - z3 stay within 1e-9)
            assert _rel(sol.z, ref.z) <= (1e-6 if name == "basic_qp" else TOL_PATH), (copies, sol.z, ref.z)
        for sol in sols[1:]:
            assert _rel(sol.x, sols[0].x) <= 1e-12 and _rel(sol.z, sols[0].z) <= 1e-12


# ---- 4. a heterogeneous batch --------------------------------------------------------------------------------------
REF_STATUS = {"basic_qp": "Solved", "basic_lp": "Solved", "basic_socp": "Solved", "basic_socp_sparse": "Solved",
              "basic_eq": "Solved", "basic_unc": "Solved", "pinf_qp": "PrimalInfeasible",
              "pinf_lp": "PrimalInfeasible", "pinf_socp": "PrimalInfeasible", "pinf_eq": "PrimalInfeasible",
              "dinf_qp": "DualInfeasible", "dinf_lp": "DualInfeasible", "dinf_eq": "DualInfeasible",
              "dinf_unc": "DualInfeasible"}


def _check_member(hip, name, pr, sol, ref):
    assert sol.status == ref.status == REF_STATUS[name], (name, sol, ref)
    assert abs(sol.iterations - ref.iterations) <= 1, (name, sol.iterations, ref.iterations)
    if sol.status == "Solved":
        tol = pr.get("tol", 1e-6)
        if pr.get("x") is not None:
            assert np.linalg.norm(sol.x - np.asarray(pr["x"])) <= tol, (name, sol.x)
        if pr.get("obj") is not None:
            assert abs(sol.obj_val - pr["obj"]) <= tol, (name, sol.obj_val)
    else:
        assert np.isnan(sol.obj_val)
        _check_certificate(pr, sol)


def test_heterogeneous_batch(hipdev):
    prs = hetero()
    sols = batch(hipdev, [p for _, p in prs]).solve()
    iters = set()
    for (name, pr), sol in zip(prs, sols):
        ref = single(hipdev, pr).solve()
        _check_member(hipdev, name, pr, sol, ref)
        iters.add(sol.iterations)
    assert len(iters) > 1, iters  # each member stops on its own


# ---- 5. order and company do not matter ---------------------------------------------------------------------------
def test_permutation_and_company(hipdev):
    prs = hetero()
    base = batch(hipdev, [p for _, p in prs]).solve()
    perm = np.random.default_rng(3).permutation(len(prs))
    sols = batch(hipdev, [prs[i][1] for i in perm]).solve()
    for j, i in enumerate(perm):
        a, b = sols[j], base[i]
        assert a.status == b.status and a.iterations == b.iterations, (prs[i][0], a, b)
        for u, v in ((a.x, b.x), (a.s, b.s), (a.z, b.z)):
            if a.status == "Solved":
                assert _rel(u, v) <= TOL_PATH, prs[i][0]
    lp = E.basic_lp()
    alone = batch(hipdev, [lp]).solve()[0]
    inside = base[[n for n, _ in prs].index("basic_lp")]
    assert alone.status == inside.status and alone.iterations == inside.iterations
    assert _rel(alone.x, inside.x) <= TOL_PATH


# ---- 6. attribution of a NaN to its member ------------------------------------------------------------------------
def test_nan_attributed_to_one_member(hipdev):
    prs = hetero()
    k = [n for n, _ in prs].index("basic_socp")
    bs = batch(hipdev, [p for _, p in prs])
    clean = bs.solve()
    bs.debug_inject_nan(k, 3)
    sols = bs.solve()
    assert sols[k].status == "NumericalError", sols[k]
    assert np.all(np.isfinite(sols[k].x)) and np.all(np.isfinite(sols[k].s)) and np.all(np.isfinite(sols[k].z))
    for j, ((name, pr), sol) in enumerate(zip(prs, sols)):
        if j == k:
            continue
        assert sol.status == clean[j].status and sol.iterations == clean[j].iterations, (name, sol, clean[j])
        ref = single(hipdev, pr).solve()
        _check_member(hipdev, name, pr, sol, ref)


def test_nan_hook_absent_from_ship_build(hipdev):
    import ctypes as C
    L = C.CDLL(hipdev.SHIP_LIB_PATH)
    assert not hasattr(L, "chip_debug_batch_inject_nan") and hasattr(L, "chip_batch_solve")


# ---- 7. host synchronisations do not scale with the batch ---------------------------------------------------------
def test_syncs_per_iteration_do_not_depend_on_nprob(hipdev):
    pr = E.basic_socp()
    per = []
    for copies in (2, 256):
        bs = batch(hipdev, [pr] * copies)
        sols = bs.solve()
        assert all(s.status == "Solved" for s in sols)
        it = bs.debug_counter("loop_iterations")
        assert it > 0
        per.append((bs.debug_counter("host_syncs") / it, bs.debug_counter("launches") / it))
    assert per[0] == per[1], per


# ---- 8. config 4 at scale -------------------------------------------------------------------------------------------
def test_config4_members_at_scale(hipdev):
    from clarabel_rs_amd import synthetic
    prs = [synthetic.portfolio_problem(2, 1000, seed=100 + i) for i in range(1024)]
    bs = batch(hipdev, prs)
    sols = bs.solve()
    assert len(sols) == 1024
    assert all(s.status == "Solved" for s in sols), [s.status for s in sols if s.status != "Solved"][:5]
    for i in np.random.default_rng(0).choice(1024, 8, replace=False):
        pr, sol = prs[i], sols[i]
        ref = single(hipdev, pr).solve()
        assert ref.status == sol.status
        assert abs(sol.obj_val - ref.obj_val) <= 1e-6 * max(1.0, abs(ref.obj_val)), (i, sol.obj_val, ref.obj_val)
        P, A = _mats(pr)
        q, b = np.asarray(pr["q"]), np.asarray(pr["b"])
        inf = lambda v: float(np.linalg.norm(v, np.inf))  # noqa: E731
        Ax, Px, Atz = A @ sol.x, P @ sol.x, A.T @ sol.z
        rp = inf(Ax + sol.s - b) / max(1.0, inf(b), inf(Ax), inf(sol.s))
        rd = inf(Px + q + Atz) / max(1.0, inf(q), inf(Px), inf(Atz))
        assert rp <= 1e-7 and rd <= 1e-7, (i, rp, rd)
