"""The L4 data updates (chip_problem_*, HipSolver.update) on the MI355X: the reference's tests/data_updating.rs, the
scaled data against a numpy restatement of update_matrix / update_vector (bit for bit), refusals that change nothing,
an updated solver against a fresh one on the e2e problems, the device forms against the host forms, update_settings,
and the config-3 portfolio problem and a supernodal QP at scale."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import e2e_problems as E
from tests.test_solver_gpu import _host_residuals, _portfolio_problem, _random_qp_problem, solver

pytestmark = pytest.mark.gpu

NN = 1


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime; tests/conftest.py loads the package)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def _csc(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return (M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64))


def updating_test_data():
    """data_updating.rs:7-44: huge values so that the equilibration (and c) carry through the update"""
    P = sp.triu(sp.csc_matrix(np.array([[40000.0, 1.0], [1.0, 20000.0]])), format="csc")
    A = sp.vstack([-sp.identity(2), sp.identity(2)], format="csc")
    return dict(n=2, m=4, P=_csc(P), A=_csc(A), q=np.full(2, 10000.0), b=np.ones(4), cones=[(NN, 2), (NN, 2)])


def _with(pr, **kw):
    out = dict(pr)
    for k, v in kw.items():
        if k in ("P", "A"):
            out[k] = (pr[k][0], pr[k][1], np.asarray(v, dtype=np.float64))
        else:
            out[k] = np.asarray(v, dtype=np.float64)
    return out


def _mat(hip, pr, key, vals=None):
    n, m = pr["n"], pr["m"]
    p, i, x = pr[key]
    return hip.CscMatrix(n if key == "P" else m, n, p, i, x if vals is None else vals)


def _resolve_and_compare(hip, s1, pr2, tol=1e-7):
    sol1 = s1.solve()
    sol2 = solver(hip, pr2).solve()
    assert sol1.status == sol2.status == "Solved", (sol1, sol2)
    assert np.linalg.norm(sol1.x - sol2.x) <= tol, (sol1.x, sol2.x)
    return sol1


# ---- 1. tests/data_updating.rs ----------------------------------------------------------------------------------
def test_update_P_matrix_form(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    P2 = pr["P"][2].copy()
    P2[0] = 100.0
    s.update_P(_mat(hipdev, pr, "P", P2))
    _resolve_and_compare(hipdev, s, _with(pr, P=P2))


def test_update_P_vector_form(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    P2 = pr["P"][2].copy()
    P2[0] = 100.0
    s.update_P(P2)
    _resolve_and_compare(hipdev, s, _with(pr, P=P2))


def test_update_P_tuple(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    s.update_P(([1, 2], [3.0, 5.0]))
    _resolve_and_compare(hipdev, s, _with(pr, P=[pr["P"][2][0], 3.0, 5.0]))


def test_update_A_matrix_form(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)  # (the reference does not solve first here)
    A2 = pr["A"][2].copy()
    A2[2] = -1000.0
    assert sp.csc_matrix((A2, pr["A"][1], pr["A"][0]), shape=(4, 2))[1, 1] == -1000.0
    s.update_A(_mat(hipdev, pr, "A", A2))
    _resolve_and_compare(hipdev, s, _with(pr, A=A2))


def test_update_A_vector_form(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    A2 = pr["A"][2].copy()
    A2[2] = -1000.0
    s.update_A(A2)
    _resolve_and_compare(hipdev, s, _with(pr, A=A2))


def test_update_A_tuple_form(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    s.update_A(([1, 2], [0.5, -0.5]))
    A2 = pr["A"][2].copy()
    A2[1], A2[2] = 0.5, -0.5
    _resolve_and_compare(hipdev, s, _with(pr, A=A2))


def test_update_q(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    q2 = pr["q"].copy()
    q2[1] = 10.0
    s.update_q(q2)
    _resolve_and_compare(hipdev, s, _with(pr, q=q2))


def test_update_q_tuple(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    s.update_q(([1], [10.0]))
    _resolve_and_compare(hipdev, s, _with(pr, q=[10000.0, 10.0]))


def test_update_b(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    b2 = pr["b"].copy()
    b2[0] = 0.0
    s.update_b(b2)
    _resolve_and_compare(hipdev, s, _with(pr, b=b2))


def test_update_b_tuple(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    s.solve()
    s.update_b(([1, 3], [0.0, 0.0]))
    _resolve_and_compare(hipdev, s, _with(pr, b=[1.0, 0.0, 1.0, 0.0]))


def test_update_noops(hipdev):
    pr = updating_test_data()
    s = solver(hipdev, pr)
    first = s.solve()
    s.update_P([])
    s.update_A([])
    s.update_q([])
    s.update_b([])
    P2, A2, q2, b2 = _mat(hipdev, pr, "P"), _mat(hipdev, pr, "A"), pr["q"], pr["b"]
    b2zip = ([1, 3], [1.0, 1.0])  # (the reference's zip writes the values b already holds)
    s.update(P=[], q=[], A=[], b=[])
    s.update(P=P2, A=A2)
    s.update(P=P2.nzval, A=A2.nzval)
    s.update(P=P2, A=A2.nzval)
    s.update(q=q2, b=b2zip)
    s.update(P=P2.nzval, A=A2, b=b2zip)
    s.update(q=q2, b=b2)
    s.update(P=P2, q=q2)
    s.update(A=A2, b=b2)
    # (the original values rescaled in one step differ from setup's step-by-step Ruiz products only by rounding)
    again = s.solve()
    assert again.status == first.status == "Solved"
    assert np.linalg.norm(again.x - first.x) <= 1e-7


def test_data_update_allowed(hipdev):
    """data_updating.rs:311-349 without the presolve half: no presolve here, so every update is allowed"""
    s = solver(hipdev, updating_test_data())
    assert s.is_data_update_allowed()
    s.solve()
    assert s.is_data_update_allowed()


# ---- 2. the scaled data, bit for bit ------------------------------------------------------------------------------
def _eq_problem():
    """equilibration on, every row / column scaled differently, c != 1"""
    rng = np.random.default_rng(4)
    n, m = 60, 90
    M = sp.random(n, n, density=0.08, random_state=5)
    P = sp.triu(M @ M.T + sp.identity(n) * 1e3, format="csc")
    A = sp.random(m, n, density=0.1, random_state=6, format="csc") * 10.0 ** rng.uniform(-3, 3)
    A = sp.diags(10.0 ** rng.uniform(-3, 3, m)) @ A
    q = rng.standard_normal(n) * 1e4
    b = rng.uniform(0.5, 2.0, m)
    return dict(n=n, m=m, P=_csc(P), A=_csc(A.tocsc()), q=q, b=b, cones=[(NN, m)])


def _coords(pr, key):
    p, i, _ = pr[key]
    cols = np.repeat(np.arange(len(p) - 1), np.diff(p))
    return np.asarray(i), cols


@pytest.mark.parametrize("mk", [updating_test_data, _eq_problem], ids=["data_updating", "random"])
def test_scaled_data_bitwise(hipdev, mk):
    pr = mk()
    s = solver(hipdev, pr)
    s.solve()
    d, e, c = s.equilibration()
    assert c != 1.0
    Pr, Pc = _coords(pr, "P")
    Ar, Ac = _coords(pr, "A")
    rng = np.random.default_rng(11)
    nP, nA, n, m = len(Pr), len(Ar), pr["n"], pr["m"]
    # full forms
    vP, vA, vq, vb = (rng.standard_normal(k) * 100 for k in (nP, nA, n, m))
    s.update(P=vP, A=vA, q=vq, b=vb)
    Px, Ax, q, b = s.scaled_data()
    assert Px.tobytes() == ((vP * (d[Pr] * d[Pc])) * c).tobytes()
    assert Ax.tobytes() == (vA * (e[Ar] * d[Ac])).tobytes()
    assert q.tobytes() == ((vq * d) * c).tobytes()
    assert b.tobytes() == (vb * e).tobytes()
    # partial forms, with repeated indices: the last occurrence wins
    for key, ln in (("P", nP), ("A", nA), ("q", n), ("b", m)):
        idx = rng.integers(0, ln, 2 * ln + 3)
        vals = rng.standard_normal(len(idx)) * 100
        getattr(s, "update_" + key)((idx, vals))
        last = {int(i): v for i, v in zip(idx, vals)}
        ii = np.array(sorted(last))
        vv = np.array([last[i] for i in ii])
        if key == "P":
            Px[ii] = ((d[Pr[ii]] * d[Pc[ii]]) * c) * vv
        elif key == "A":
            Ax[ii] = (e[Ar[ii]] * d[Ac[ii]]) * vv
        elif key == "q":
            q[ii] = (vv * d[ii]) * c
        else:
            b[ii] = vv * e[ii]
        got = s.scaled_data()
        for x, y in zip(got, (Px, Ax, q, b)):
            assert x.tobytes() == y.tobytes(), key
    # b is not capped at 1e20 by an update (only ProblemData::new caps it)
    s.update_b(([0], [1e30]))
    assert s.scaled_data()[3][0] == 1e30 * e[0]
    d2, e2, c2 = s.equilibration()
    assert d2.tobytes() == d.tobytes() and e2.tobytes() == e.tobytes() and c2 == c


# ---- 3. refusals change nothing -----------------------------------------------------------------------------------
def test_refusals_change_nothing(hipdev):
    import ctypes as C

    import torch
    pr = _eq_problem()
    s = solver(hipdev, pr)
    before = [a.tobytes() for a in s.scaled_data()]
    lens = {"P": len(pr["P"][2]), "A": len(pr["A"][2]), "q": pr["n"], "b": pr["m"]}
    for key, ln in lens.items():
        with pytest.raises(hipdev.ChipError) as e:  # one bad index among good ones
            getattr(s, "update_" + key)(([0, 1, ln, 2], [1.0, 2.0, 3.0, 4.0]))
        assert e.value.code == hipdev.ERR_DIM
        with pytest.raises(hipdev.ChipError) as e:
            getattr(s, "update_" + key)(np.ones(ln + 1))
        assert e.value.code == hipdev.ERR_DIM
        # the library's own check of a full length (below the Python classifier)
        v = np.ones(ln - 1)
        rc = getattr(hipdev.lib(), "chip_problem_update_" + key)(s._h, None, v.ctypes.data_as(hipdev.P_F64),
                                                                   C.c_int64(ln - 1))
        assert rc == hipdev.ERR_DIM
        with pytest.raises(hipdev.ChipError) as e:  # a negative device index
            getattr(s, "update_" + key)((torch.tensor([0, -1], dtype=torch.int64, device="cuda"),
                                         torch.ones(2, dtype=torch.float64, device="cuda")))
        assert e.value.code == hipdev.ERR_DIM
        with pytest.raises(hipdev.ChipError) as e:
            getattr(s, "update_" + key)((torch.tensor([ln], dtype=torch.int64, device="cuda"),
                                         torch.ones(1, dtype=torch.float64, device="cuda")))
        assert e.value.code == hipdev.ERR_DIM
        assert [a.tobytes() for a in s.scaled_data()] == before, key
    sol = s.solve()
    fresh = solver(hipdev, pr).solve()
    assert sol.status == fresh.status == "Solved" and sol.iterations == fresh.iterations


# ---- 4. an updated solver against a fresh one ---------------------------------------------------------------------
def _new_data(pr, seed):
    """new finite values on the same patterns: P scaled (stays PSD), A, q, b perturbed"""
    rng = np.random.default_rng(seed)
    P2 = np.asarray(pr["P"][2], float) * 1.25
    A2 = np.asarray(pr["A"][2], float) * (1.0 + 0.02 * rng.uniform(-1, 1, len(pr["A"][2])))
    q2 = np.asarray(pr["q"], float) + 0.1 * rng.standard_normal(pr["n"])
    b2 = np.asarray(pr["b"], float) * (1.0 + 0.02 * rng.uniform(-1, 1, pr["m"]))
    return P2, A2, q2, b2


@pytest.mark.parametrize("name", ["basic_qp", "basic_lp", "basic_socp", "basic_sdp", "basic_expcone", "basic_powcone",
                                  "mixed_conic"])
def test_updated_matches_fresh_solver(hipdev, name):
    pr = getattr(E, name)()
    s = solver(hipdev, pr, equilibrate_enable=0)
    s.solve()
    P2, A2, q2, b2 = _new_data(pr, 7)
    rng = np.random.default_rng(8)
    # mixed forms: P as a matrix, A as a shuffled tuple of every entry, q full, b as two partial updates
    s.update(P=_mat(hipdev, pr, "P", P2))
    perm = rng.permutation(len(A2))
    s.update_A((perm, A2[perm]))
    s.update_q(list(q2))
    half = pr["m"] // 2
    s.update_b((np.arange(half), b2[:half]))
    s.update_b((np.arange(half, pr["m"]), b2[half:]))
    sol = s.solve()
    fresh = solver(hipdev, _with(pr, P=P2, A=A2, q=q2, b=b2), equilibrate_enable=0).solve()
    assert sol.status == fresh.status and sol.iterations == fresh.iterations, (sol, fresh)
    tol = 1e-10 * max(1.0, float(np.max(np.abs(fresh.x))))
    for a, f in ((sol.x, fresh.x), (sol.s, fresh.s), (sol.z, fresh.z)):
        assert np.max(np.abs(a - f)) <= tol, (name, np.max(np.abs(a - f)))


# ---- 5. the device forms ------------------------------------------------------------------------------------------
def test_device_forms_equal_host_forms(hipdev):
    import torch
    pr = _eq_problem()
    sh, sd = solver(hipdev, pr), solver(hipdev, pr)
    P2, A2, q2, b2 = _new_data(pr, 3)
    rng = np.random.default_rng(5)
    ib = rng.integers(0, pr["m"], 40)
    vb = rng.uniform(0.5, 2.0, 40)
    iP = rng.integers(0, len(P2), 10)
    vP = P2[iP] * 1.1
    sh.update(P=P2, A=A2, q=q2, b=(ib, vb))
    sh.update_P((iP, vP))
    dev = lambda a, t=torch.float64: torch.tensor(np.asarray(a), dtype=t, device="cuda")  # noqa: E731
    sd.update(P=dev(P2), A=dev(A2), q=dev(q2), b=(dev(ib, torch.int64), dev(vb)))
    sd.update_P((dev(iP, torch.int64), dev(vP)))
    for x, y in zip(sh.scaled_data(), sd.scaled_data()):
        assert x.tobytes() == y.tobytes()
    a, b = sh.solve(), sd.solve()
    assert a.status == b.status == "Solved" and a.iterations == b.iterations
    # (two handles: the factorisation's accumulation order is not fixed, so the solves agree to rounding)
    assert np.max(np.abs(a.x - b.x)) <= 1e-10 * max(1.0, float(np.max(np.abs(a.x))))


# ---- 6. settings ------------------------------------------------------------------------------------------------
def test_update_settings(hipdev):
    pr = _eq_problem()
    s = solver(hipdev, pr)
    base = s.solve()
    assert base.status == "Solved"
    s.update_settings(max_iter=2)
    assert s.solve().status == "MaxIterations"
    s.update_settings(max_iter=200)
    again = s.solve()
    assert again.status == "Solved" and again.iterations == base.iterations
    s.update(settings=hipdev.SolverSettings.from_buffer_copy(s.settings))  # the same settings: accepted
    s.update_settings(tol_gap_abs=1e-3, tol_gap_rel=1e-3, tol_feas=1e-3, tol_ktratio=1e-2)
    loose = s.solve()
    assert loose.status == "Solved" and loose.iterations < base.iterations
    s.update_settings(tol_gap_abs=1e-8, tol_gap_rel=1e-8, tol_feas=1e-8, tol_ktratio=1e-6)
    for kw in (dict(equilibrate_enable=0), dict(equilibrate_max_iter=3), dict(equilibrate_min_scaling=1e-3),
               dict(equilibrate_max_scaling=1e3), dict(static_regularization_constant=1e-7),
               dict(iterative_refinement_max_iter=3), dict(linesearch_backtrack_step=0.5),
               dict(min_terminate_step_length=1e-3)):
        old = bytes(s.settings)
        with pytest.raises(hipdev.ChipError) as e:
            s.update_settings(**kw)
        assert e.value.code == hipdev.ERR_ARG, kw
        assert bytes(s.settings) == old
    last = s.solve()  # the old settings stay in force
    assert last.status == "Solved" and last.iterations == base.iterations


# ---- 7. at scale ------------------------------------------------------------------------------------------------
def test_portfolio_update_at_scale(hipdev):
    pr = _portfolio_problem()
    s = solver(hipdev, pr)
    assert s.solve().status == "Solved"
    n, m = pr["n"], pr["m"]
    nblocks, dim = 1000, 1001
    rng = np.random.default_rng(77)
    q2 = -rng.uniform(0.0, 1.0, n)  # new returns
    ib = 1 + n + dim * np.arange(nblocks)  # the risk budgets
    gamma = rng.uniform(1.0, 2.5, nblocks) / np.sqrt(1000)
    s.update(q=q2, b=(ib, gamma))
    sol = s.solve()
    assert sol.status == "Solved", sol
    b2 = np.asarray(pr["b"], float).copy()
    b2[ib] = gamma
    pr2 = _with(pr, q=q2, b=b2)
    rp, rd, gap = _host_residuals(pr2, sol)
    assert rp <= 1e-7 and rd <= 1e-7 and gap <= 1e-7, (rp, rd, gap)
    fresh = solver(hipdev, pr2).solve()
    assert fresh.status == "Solved"
    assert abs(sol.obj_val - fresh.obj_val) <= 1e-6 * max(1.0, abs(fresh.obj_val)), (sol.obj_val, fresh.obj_val)


def test_random_qp_update_P_at_scale(hipdev):
    pr = _random_qp_problem()
    s = solver(hipdev, pr)
    assert s.solve().status == "Solved"
    P2 = np.asarray(pr["P"][2], float) * 2.0
    s.update_P(P2)
    sol = s.solve()
    assert sol.status == "Solved", sol
    rp, rd, gap = _host_residuals(_with(pr, P=P2), sol)
    assert rp <= 1e-7 and rd <= 1e-7 and gap <= 1e-7, (rp, rd, gap)
