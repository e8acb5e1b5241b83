"""The L4 solver (chip_solver_*, HipSolver) on the MI355X: the device equilibration against a numpy restatement of
default/problemdata.rs:231-312 + the cones' rectification, the reference's equilibration_bounds.rs and end-to-end
tests (tests/basic_*.rs, mixed_conic.rs, the HS35 fixture) with their asserted values and tolerances, infeasibility
certificates checked on the host, the loop against tests/ipm_device.py with identity equilibration, and the
config-3 portfolio problem and a supernodal QP at scale."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import e2e_problems as E
from tests import ipm_device, json_problem

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ZERO, NN, SOC, EXP, POW, GENPOW, PSD = range(7)


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime; tests/conftest.py loads the package)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def numel(c):
    if c[0] in (EXP, POW):
        return 3
    if c[0] == GENPOW:
        return c[1] + c[2]
    if c[0] == PSD:
        return c[1] * (c[1] + 1) // 2
    return c[1]


def solver(hip, pr, **kw):
    n, m = pr["n"], pr["m"]
    P = hip.CscMatrix(n, n, *pr["P"])
    A = hip.CscMatrix(m, n, *pr["A"])
    return hip.HipSolver(P, pr["q"], A, pr["b"], pr["cones"], hip.SolverSettings.default(**kw))


def solve(hip, pr, **kw):
    return solver(hip, pr, **kw).solve()


# ---------------------------------------------------------------------------------------------------------------
# numpy restatement of DefaultProblemData::equilibrate (problemdata.rs:231-312) and CompositeCone's rectification
# (compositecone.rs:183-195), multiplying in scale_data's order (lrscale: val *= l[row] * r[col])
# ---------------------------------------------------------------------------------------------------------------
def _clip(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def ruiz(pr, max_iter=10, smin=1e-4, smax=1e4):
    n, m = pr["n"], pr["m"]
    Pp, Pi, Px = (np.asarray(a) for a in pr["P"])
    Ap, Ai, Ax = (np.asarray(a) for a in pr["A"])
    Pi, Ai = Pi.astype(np.int64), Ai.astype(np.int64)
    Px, Ax = Px.astype(float).copy(), Ax.astype(float).copy()
    Pc = np.repeat(np.arange(n), np.diff(Pp))
    Ac = np.repeat(np.arange(n), np.diff(Ap))
    q = np.asarray(pr["q"], float).copy()
    b = np.minimum(np.asarray(pr["b"], float), 1e20)
    d, e, c = np.ones(n), np.ones(m), 1.0
    for _ in range(max_iter):
        dw, ew = np.zeros(n), np.zeros(m)
        np.maximum.at(dw, Pc, np.abs(Px))
        np.maximum.at(dw, Pi, np.abs(Px))
        np.maximum.at(dw, Ac, np.abs(Ax))
        np.maximum.at(ew, Ai, np.abs(Ax))
        dw[dw == 0.0] = 1.0
        ew[ew == 0.0] = 1.0
        dw, ew = 1.0 / np.sqrt(dw), 1.0 / np.sqrt(ew)
        dw, ew = _clip(dw, smin / d, smax / d), _clip(ew, smin / e, smax / e)
        Px = Px * (dw[Pi] * dw[Pc])
        Ax = Ax * (ew[Ai] * dw[Ac])
        q, b = q * dw, b * ew
        d, e = d * dw, e * ew
        pc = np.zeros(n)
        np.maximum.at(pc, Pc, np.abs(Px))
        mean = pc.sum() / n if n else 0.0
        qn = np.abs(q).max() if n else 0.0
        if mean != 0.0 and qn != 0.0:
            ct = _clip(np.array(1.0 / max(qn, mean)), smin / c, smax / c)[()]
            Px, q, c = Px * ct, q * ct, c * ct
    delta, changed, start = np.ones(m), False, 0
    for cone in pr["cones"]:
        k = numel(cone)
        if cone[0] >= SOC:
            changed = True
            if k:
                seg = e[start:start + k]
                delta[start:start + k] = (1.0 / seg) * seg.mean()
        start += k
    if changed:
        e = e * delta
    return d, e, c


def _csc(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return (M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64))


def random_problem(n, seed, q_zero=False, cones_kind="all"):
    """every cone type (or Zero / Nonnegative only), zero rows and columns, entries spread over 24 decades so that
    the scaling hits both bounds"""
    rng = np.random.default_rng(seed)
    if cones_kind == "all":
        cones = [(ZERO, 50), (NN, 400), (SOC, 7), (SOC, 40), (EXP, 3), (POW, 3, 0, 0.3), (GENPOW, 3, 2, [0.2, 0.3, 0.5]),
                 (PSD, 4), (NN, 300), (SOC, 3)] * max(1, n // 4000)
    else:
        cones = [(ZERO, 300), (NN, 900), (NN, 1)] * max(1, n // 2000)
    m = sum(numel(c) for c in cones)
    nnz = 4 * max(n, m)
    rows = rng.integers(0, m, nnz)
    cols = np.clip((rows * n) // m + rng.integers(-30, 31, nnz), 0, n - 1)  # banded: bounded fill-in
    vals = rng.standard_normal(nnz) * 10.0 ** rng.uniform(-12, 12, nnz)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsc()
    A.sum_duplicates()
    keep = ~np.isin(A.tocoo().row, rng.integers(0, m, 20)) & ~np.isin(A.tocoo().col, rng.integers(0, n, 10))
    Ac = A.tocoo()
    A = sp.coo_matrix((Ac.data[keep], (Ac.row[keep], Ac.col[keep])), shape=(m, n)).tocsc()  # zero rows and columns
    pr_ = rng.integers(0, n, 2 * n)
    pc_ = np.clip(pr_ + rng.integers(0, 31, 2 * n), 0, n - 1)
    Pv = rng.standard_normal(2 * n) * 10.0 ** rng.uniform(-8, 8, 2 * n)
    P = sp.coo_matrix((Pv, (np.minimum(pr_, pc_), np.maximum(pr_, pc_))), shape=(n, n)).tocsc()
    P.sum_duplicates()
    q = np.zeros(n) if q_zero else rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)
    b = rng.standard_normal(m)
    return dict(n=n, m=m, P=_csc(P), A=_csc(A), q=q, b=b, cones=cones)


def fixtures():
    out = [(nm, getattr(E, nm)()) for nm in ("basic_qp", "basic_lp", "basic_socp", "basic_expcone", "basic_powcone",
                                             "basic_sdp", "basic_genpowcone", "basic_eq_constrained", "mixed_conic",
                                             "basic_unconstrained")]
    out.append(("hs35", json_problem.load(os.path.join(GOLD, "hs35_reference.json"))))
    return out


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


@pytest.mark.parametrize("name,pr", fixtures(), ids=[f[0] for f in fixtures()])
def test_equilibration_matches_restatement_fixtures(hipdev, name, pr):
    d, e, c = solver(hipdev, pr).equilibration()
    d0, e0, c0 = ruiz(pr)
    assert _rel(d, d0) <= 1e-13 and _rel(e, e0) <= 1e-13 and _rel(c, c0) <= 1e-13, (name, d, d0, e, e0, c, c0)


@pytest.mark.parametrize("n,seed", [(12000, 1), (40000, 2)])
def test_equilibration_matches_restatement_random(hipdev, n, seed):
    pr = random_problem(n, seed)
    d, e, c = solver(hipdev, pr).equilibration()
    d0, e0, c0 = ruiz(pr)
    assert _rel(d, d0) <= 1e-13 and _rel(e, e0) <= 1e-13 and _rel(c, c0) <= 1e-13
    assert d.min() < 1e-3 and d.max() > 1e3  # the scaling reached far into both directions


@pytest.mark.parametrize("iters", [1, 3, 10, 25])
def test_equilibration_bitwise_without_cost_scaling_or_rectification(hipdev, iters):
    pr = random_problem(20000, 7, q_zero=True, cones_kind="nn")
    d, e, c = solver(hipdev, pr, equilibrate_max_iter=iters).equilibration()
    d0, e0, c0 = ruiz(pr, max_iter=iters)
    assert c == 1.0 and c0 == 1.0
    assert np.array_equal(d.view(np.uint64), d0.view(np.uint64))
    assert np.array_equal(e.view(np.uint64), e0.view(np.uint64))


# ---- tests/equilibration_bounds.rs -----------------------------------------------------------------------------
def _eq_bounds_data():
    pr = E.basic_qp()
    return dict(pr, P=tuple(np.array(a) for a in pr["P"]), A=tuple(np.array(a) for a in pr["A"]))


def _in_bounds(d, e, lo=1e-4, hi=1e4):
    return d.min() >= lo and e.min() >= lo and d.max() <= hi and e.max() <= hi


def test_equilibrate_lower_bound(hipdev):
    pr = _eq_bounds_data()
    # P = [4 1; 1 2] is given FULL in the reference test; its triu keeps (0,0), (0,1), (1,1): P.nzval[0] = (0,0)
    pr["P"][2][0] = 1e-15
    s = solver(hipdev, pr)
    s.solve()
    d, e, _ = s.equilibration()
    assert _in_bounds(d, e)


def test_equilibrate_upper_bound(hipdev):
    pr = _eq_bounds_data()
    pr["A"][2][0] = 1e15
    s = solver(hipdev, pr, max_iter=10)
    d, e, _ = s.equilibration()
    assert _in_bounds(d, e)
    assert s.solve().status == "MaxIterations"


def test_equilibrate_zero_rows(hipdev):
    pr = _eq_bounds_data()
    pr["A"][2][:] = 0.0
    s = solver(hipdev, pr)
    s.solve()
    _, e, _ = s.equilibration()
    assert np.all(e == 1.0)


# ---- the reference's end-to-end tests -----------------------------------------------------------------------------
def _check_solved(sol, x=None, obj=None, tol=1e-6):
    assert sol.status == "Solved", sol
    if x is not None:
        assert np.linalg.norm(sol.x - np.asarray(x)) <= tol, (sol.x, x)
    if obj is not None:
        assert abs(sol.obj_val - obj) <= tol and abs(sol.obj_val_dual - obj) <= tol, (sol.obj_val, sol.obj_val_dual, obj)


@pytest.mark.parametrize("name", ["basic_qp", "basic_lp", "basic_socp", "basic_sdp", "basic_unconstrained",
                                  "basic_eq_constrained"])
def test_e2e_feasible(hipdev, name):
    pr = getattr(E, name)()
    sol = solve(hipdev, pr)
    tol = pr["tol"]
    _check_solved(sol, pr["x"], pr["obj"], tol)


def test_qp_univariate(hipdev):
    pr = dict(n=1, m=1, P=_csc(sp.identity(1)), A=_csc(sp.identity(1)), q=[0.0], b=[1.0], cones=[(NN, 1)])
    sol = solve(hipdev, pr)
    assert sol.status == "Solved"
    assert abs(sol.x[0]) <= 1e-6 and abs(sol.obj_val) <= 1e-6 and abs(sol.obj_val_dual) <= 1e-6


def test_qp_singleton_constraints(hipdev):
    pr = E.basic_qp()
    s1 = solve(hipdev, pr)
    s2 = solve(hipdev, dict(pr, cones=[(NN, 1)] * 6))
    assert s1.status == s2.status == "Solved"
    # the reference asserts equal x and objective for NN(3)x2, NN(1)x6 and SOC(1)x6 (SOC(1) is refused here: dim >= 2)
    assert np.array_equal(s1.x, s2.x) and s1.obj_val == s2.obj_val


def test_socp_sparse(hipdev):
    # basic_socp.rs:75-89: one SOC(6) (its sparse expansion) instead of NN(3) + SOC(3); the status is asserted
    assert solve(hipdev, E.basic_socp(sparse_soc=True)).status == "Solved"


def test_expcone(hipdev):
    pr = E.basic_expcone()
    sol = solve(hipdev, pr)
    _check_solved(sol, pr["x"], pr["obj"], 1e-6)


@pytest.mark.parametrize("name", ["basic_powcone", "basic_genpowcone"])
def test_powcones(hipdev, name):
    pr = getattr(E, name)()
    sol = solve(hipdev, pr)
    assert sol.status == "Solved"
    assert abs(sol.obj_val - pr["obj"]) <= 1e-3 and abs(sol.obj_val_dual - pr["obj"]) <= 1e-3


def test_sdp_empty_cone(hipdev):
    pr = E.basic_sdp()
    sol = solve(hipdev, dict(pr, cones=pr["cones"] + [(PSD, 0)]))
    assert sol.status == "Solved"
    assert np.linalg.norm(sol.x - np.asarray(pr["x"])) <= 1e-6 and abs(sol.obj_val - pr["obj"]) <= 1e-6


def test_mixed_conic(hipdev):
    pr = E.mixed_conic()
    sol = solve(hipdev, pr)
    assert sol.status == "Solved"
    assert abs(sol.obj_val) <= 1e-8 and abs(sol.obj_val_dual) <= 1e-8


def test_hs35(hipdev):
    pr = json_problem.load(os.path.join(GOLD, "hs35_reference.json"))
    sol = solve(hipdev, pr)
    assert sol.status == "Solved"
    assert np.linalg.norm(sol.x - np.array([4.0 / 3.0, 7.0 / 9.0, 4.0 / 9.0])) <= 1e-6
    assert abs(sol.obj_val + 9.0 - 1.0 / 9.0) <= 1e-6


# ---- infeasible problems and their certificates -------------------------------------------------------------------
def _qp_dual_inf():  # basic_qp.rs:44-78: P = [1 1; 1 1] (triu), A = [1 1; 1 0], q = [1, -1], b = [1, 1], NN(2)
    return dict(n=2, m=2, P=_csc(sp.triu(sp.csc_matrix(np.ones((2, 2))))), A=_csc(np.array([[1.0, 1.0], [1.0, 0.0]])),
                q=[1.0, -1.0], b=[1.0, 1.0], cones=[(NN, 2)])


def primal_infeasible():
    qp = E.basic_qp()
    qp["b"] = list(qp["b"])
    qp["b"][0] = qp["b"][3] = -1.0  # basic_qp.rs:145-160
    lp = E.basic_lp()
    lp["b"] = list(lp["b"])
    lp["b"][0] = lp["b"][3] = -1.0  # basic_lp.rs:50-65
    socp = E.basic_socp()
    socp["b"] = list(socp["b"])
    socp["b"][6] = -10.0  # basic_socp.rs:92-107
    sdp = E.basic_sdp()  # basic_sdp.rs:78-100: x and -x both in the PSD cone, b = [b; 0]
    A = sp.csc_matrix((sdp["A"][2], sdp["A"][1], sdp["A"][0]), shape=(6, 6))
    sdp = dict(sdp, m=12, A=_csc(sp.vstack([A, -A])), b=list(sdp["b"]) + [0.0] * 6, cones=sdp["cones"] * 2)
    # basic_eq_constrained.rs: P = I, q = 0, A2 (4 x 3), b = 1, ZeroConeT(4)
    A2 = np.array([[0.0, 1.0, 1.0], [0.0, 1.0, -1.0], [1.0, 2.0, -1.0], [2.0, -1.0, 3.0]])
    eq = dict(n=3, m=4, P=_csc(sp.identity(3)), A=_csc(A2), q=[0.0] * 3, b=[1.0] * 4, cones=[(ZERO, 4)])
    return [("qp", qp), ("lp", lp), ("socp", socp), ("sdp", sdp), ("eq_constrained", eq)]


def dual_infeasible():
    lp = E.basic_lp()  # basic_lp.rs:68-83: A.nzval[1] = 1 (the lower bound on x1 becomes a redundant upper bound)
    A = [np.array(a) for a in lp["A"]]
    A[2][1] = 1.0
    lp_ill = E.basic_lp()  # basic_lp.rs:86-101
    B = [np.array(a) for a in lp_ill["A"]]
    B[2][0], B[2][1] = np.finfo(float).eps, 0.0
    qp_ill = dict(_qp_dual_inf(), m=1, A=(np.array([0, 1, 2]), np.array([0, 0]), np.array([1.0, 1.0])), b=[1.0],
                  cones=[(NN, 1)])  # basic_qp.rs:178-202
    # basic_eq_constrained.rs: P = I with P.nzval[0] = 0 (kept as a stored zero), q = 1, A1, b = [2, 0], ZeroConeT(2)
    eq = dict(E.basic_eq_constrained(), P=(np.array([0, 1, 2, 3]), np.array([0, 1, 2]), np.array([0.0, 1.0, 1.0])),
              q=[1.0, 1.0, 1.0])
    # basic_unconstrained.rs: P = 0 (no entries), q = [1, 0, 0], no constraints (m = 0)
    unc = dict(n=3, m=0, P=(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)),
               A=(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)), q=[1.0, 0.0, 0.0], b=[],
               cones=[])
    return [("qp", _qp_dual_inf()), ("qp_ill_cond", qp_ill), ("lp", dict(lp, A=tuple(A))),
            ("lp_ill_cond", dict(lp_ill, A=tuple(B))), ("eq_constrained", eq), ("unconstrained", unc)]


def _mats(pr):
    n, m = pr["n"], pr["m"]
    A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n))
    Pu = sp.csc_matrix((pr["P"][2], pr["P"][1], pr["P"][0]), shape=(n, n))
    P = Pu + sp.triu(Pu, 1).T
    return P, A


def _dual_cone_dist(z, cones):
    """distance of z from the (self-dual) NN / SOC / PSD cones of these fixtures, 0 for Zero rows (dual = free)"""
    dist, k = 0.0, 0
    for c in cones:
        v = np.asarray(z[k:k + numel(c)])
        if c[0] == NN:
            dist = max(dist, float(np.max(np.maximum(-v, 0.0), initial=0.0)))
        elif c[0] == SOC:
            dist = max(dist, max(0.0, float(np.linalg.norm(v[1:]) - v[0])))
        elif c[0] == PSD:
            nn = c[1]  # svec: the upper triangle by columns, off-diagonal entries scaled by sqrt(2)
            M = np.zeros((nn, nn))
            for t, (i, j) in enumerate((i, j) for j in range(nn) for i in range(j + 1)):
                M[i, j] = M[j, i] = v[t] if i == j else v[t] / np.sqrt(2.0)
            dist = max(dist, max(0.0, -float(np.linalg.eigvalsh(M).min())))
        k += numel(c)
    return dist


@pytest.mark.parametrize("name,pr", primal_infeasible(), ids=[p[0] for p in primal_infeasible()])
def test_primal_infeasible_certificate(hipdev, name, pr):
    sol = solve(hipdev, pr)
    assert sol.status == "PrimalInfeasible", sol
    assert np.isnan(sol.obj_val) and np.isnan(sol.obj_val_dual)
    _, A = _mats(pr)
    z = sol.z
    bz = float(np.dot(pr["b"], z))
    assert bz < 0.0
    assert np.linalg.norm(A.T @ z, np.inf) <= 1e-6 * abs(bz)
    assert _dual_cone_dist(z, pr["cones"]) <= 1e-8 * max(1.0, np.linalg.norm(z, np.inf))


@pytest.mark.parametrize("name,pr", dual_infeasible(), ids=[p[0] for p in dual_infeasible()])
def test_dual_infeasible_certificate(hipdev, name, pr):
    sol = solve(hipdev, pr)
    assert sol.status == "DualInfeasible", sol
    assert np.isnan(sol.obj_val) and np.isnan(sol.obj_val_dual)
    P, A = _mats(pr)
    x = sol.x
    qx = float(np.dot(pr["q"], x))
    assert qx < 0.0
    # -A x in the cone (Nonnegative: A x <= 0; Zero: A x = 0), to 1e-6 of |q'x| on every fixture
    k = 0
    for c in pr["cones"]:
        ax = (A @ x)[k:k + numel(c)]
        viol = np.abs(ax) if c[0] == ZERO else np.maximum(ax, 0.0)
        assert float(np.max(viol, initial=0.0)) <= 1e-6 * abs(qx), (c, ax)
        k += numel(c)
    # P x = 0: to 1e-6 of |q'x| on the well-conditioned fixtures.  On the ill-conditioned ones the reference's own test
    # (info.rs:383-389) divides ||P x|| by the norm of the homogeneous iterate, which grows without bound there, so the
    # normalised certificate is only a direction close to the null space of P: its angle to it is bounded instead,
    # ||P x|| <= 0.1 ||P||_2 ||x||_2 (a direction with a component of P's range comparable to its null-space part,
    # i.e. a wrong certificate, does not pass)
    if name.endswith("ill_cond"):
        normP = float(np.linalg.norm(P.toarray(), 2)) if P.nnz else 0.0
        assert np.linalg.norm(P @ x) <= 0.1 * normP * np.linalg.norm(x)
    else:
        assert np.linalg.norm(P @ x, np.inf) <= 1e-6 * abs(qx)


def test_expcone_primal_infeasible(hipdev):
    """basic_expcone.rs: the feasible problem with z == -1 (b[4] = -1)"""
    pr = E.basic_expcone()
    pr["b"] = list(pr["b"])
    pr["b"][4] = -1.0
    sol = solve(hipdev, pr)
    assert sol.status == "PrimalInfeasible", sol
    assert np.isnan(sol.obj_val) and np.isnan(sol.obj_val_dual)
    z = sol.z
    bz = float(np.dot(pr["b"], z))
    _, A = _mats(pr)
    assert bz < 0.0 and np.linalg.norm(A.T @ z, np.inf) <= 1e-6 * abs(bz)
    # z[0:3] in the dual exponential cone: u < 0, -u exp(v / u) <= e w (the Zero rows' dual is free)
    u, v, w = z[0:3]
    assert u < 0.0 and w > 0.0 and np.log(-u) + v / u <= 1.0 + np.log(w) + 1e-6


def test_expcone_dual_infeasible(hipdev):
    """basic_expcone.rs: max x s.t. y exp(x / y) <= z, without the equality constraints"""
    pr = dict(n=3, m=3, P=_csc(sp.csc_matrix((3, 3))), A=_csc(-np.eye(3)), q=[-1.0, 0.0, 0.0], b=[0.0] * 3,
              cones=[(EXP, 3)])
    sol = solve(hipdev, pr)
    assert sol.status == "DualInfeasible", sol
    assert np.isnan(sol.obj_val) and np.isnan(sol.obj_val_dual)
    x = sol.x
    assert float(np.dot(pr["q"], x)) < 0.0
    # -A x = x in the exponential cone: y > 0, y exp(x / y) <= z (in logarithms)
    assert x[1] > 0.0 and x[2] > 0.0 and np.log(x[1]) + x[0] / x[1] <= np.log(x[2]) + 1e-6


def test_solver_create_refuses_sizes_past_int32(hipdev):
    """the equilibration passes index P and A together in int32: a problem whose nnz(P) + nnz(A) reaches 2^31 is
    refused before any of its arrays are read (only the two colptr arrays are)"""
    hip = hipdev
    big = 1 << 30
    P = hip.CscMatrix(1, 1, [0, big], [0], [1.0])
    A = hip.CscMatrix(1, 1, [0, big], [0], [1.0])
    with pytest.raises(hip.ChipError) as e:
        hip.HipSolver(P, [1.0], A, [1.0], [(NN, 1)])
    assert e.value.code == hip.ERR_DIM


# ---- the same loop as the harness ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["basic_qp", "basic_lp", "basic_socp", "basic_sdp", "basic_expcone", "basic_powcone",
                                  "mixed_conic"])
def test_same_loop_as_harness_without_equilibration(hipdev, name):
    pr = getattr(E, name)()
    ref = ipm_device.solve_device(hipdev, pr["n"], pr["m"], pr["P"], pr["A"], pr["q"], pr["b"], pr["cones"])
    sol = solve(hipdev, pr, equilibrate_enable=0)
    assert ref["status"] == "Solved" and sol.status == "Solved"
    assert sol.iterations == ref["iterations"], (sol.iterations, ref["iterations"])
    for a, b in ((sol.x, ref["x"]), (sol.s, ref["s"]), (sol.z, ref["z"])):
        assert np.max(np.abs(a - b)) <= 1e-9 * max(1.0, np.max(np.abs(b)))


def test_dual_scaling_switch_matches_harness(hipdev):
    """min_switch_step_length = 0.999 makes the nonsymmetric problem switch to the dual scaling at once
    (core/solver.rs:630-654); the harness takes the same switch"""
    pr = E.mixed_conic()
    ref = ipm_device.solve_device(hipdev, pr["n"], pr["m"], pr["P"], pr["A"], pr["q"], pr["b"], pr["cones"],
                                  min_switch_step_length=0.999)
    sol = solve(hipdev, pr, equilibrate_enable=0, min_switch_step_length=0.999)
    assert sol.status == ref["status"] == "Solved"
    assert sol.iterations == ref["iterations"]
    assert np.max(np.abs(sol.x - ref["x"])) <= 1e-9


# ---- at scale ---------------------------------------------------------------------------------------------------
def _host_residuals(pr, sol):
    P, A = _mats(pr)
    q, b = np.asarray(pr["q"], float), np.asarray(pr["b"], float)
    x, s, z = sol.x, sol.s, sol.z
    Ax, Px, Atz = A @ x, P @ x, A.T @ z
    inf = lambda v: float(np.linalg.norm(v, np.inf)) if len(v) else 0.0  # noqa: E731
    rp = inf(Ax + s - b) / max(1.0, inf(b), inf(Ax), inf(s))
    rd = inf(Px + q + Atz) / max(1.0, inf(q), inf(Px), inf(Atz))
    xPx = float(x @ Px)
    pobj, dobj = 0.5 * xPx + float(q @ x), -0.5 * xPx - float(b @ z)
    gap = abs(pobj - dobj) / max(1.0, min(abs(pobj), abs(dobj)))
    return rp, rd, gap


def _random_qp_problem():
    from clarabel_rs_amd import synthetic
    pr = synthetic.random_qp(20000, 40000, band=40, seed=5)
    rng = np.random.default_rng(9)
    pr["q"] = rng.standard_normal(pr["n"])
    pr["b"] = rng.uniform(0.5, 1.5, pr["m"])  # x = 0 is strictly feasible
    return pr


def _portfolio_problem():
    from clarabel_rs_amd import synthetic
    return synthetic.portfolio_problem(1000, 1000, seed=3)


@pytest.mark.parametrize("make", [_portfolio_problem, _random_qp_problem], ids=["portfolio_1e6", "random_qp"])
def test_at_scale(hipdev, make):
    pr = make()
    s = solver(hipdev, pr)
    sol = s.solve()
    assert sol.status == "Solved", sol
    rp, rd, gap = _host_residuals(pr, sol)
    assert rp <= 1e-7 and rd <= 1e-7 and gap <= 1e-7, (rp, rd, gap)
    # a second solve restarts from default_start and takes the same path; the factorisation's on-chip accumulation
    # order is not fixed (no bit-equality test of the bundle kernels), so x agrees to rounding, not bitwise
    again = s.solve()
    assert again.status == "Solved" and again.iterations == sol.iterations
    assert np.max(np.abs(again.x - sol.x)) <= 1e-10 * max(1.0, np.max(np.abs(sol.x)))
