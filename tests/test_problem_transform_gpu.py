"""Presolve and chordal decomposition in the L4 solver on the MI355X: sdp_chordal.rs in all twelve settings, the
presolve.rs cases, the e2e SDP / mixed-conic problems with both transforms on, banded SDPs against the undecomposed
solve, the device reverse bit for bit against the host restatement (compact, standard, an infeasibility certificate),
the refusal of data updates, and a PSD cone of side 1000 that only decomposition makes solvable."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

from tests import e2e_problems as E
from tests.test_problem_transform_host import (MERGES, NN, PSD, SQ2, banded, csc, mask_sdp, presolve_data,
                                               sdp_chordal_data, tri, triu_index)
from tests.test_solver_gpu import solver as e2e_solver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def make(hip, P, q, A, b, cones, **kw):
    return hip.HipSolver(csc(hip, sp.triu(P)), q, csc(hip, A), b, cones, hip.SolverSettings.default(**kw))


def debug(hip, P, q, A, b, cones, **kw):
    return hip.TransformDebug(csc(hip, sp.triu(P)), q, csc(hip, A), b, cones, hip.SolverSettings.default(**kw))


def objective(P, q, x):
    return 0.5 * x @ (P @ x) + q @ x


def psd_checks(s, z, row, N, complete):
    S, Z = np.zeros((N, N)), np.zeros((N, N))
    for c in range(N):
        for r in range(c + 1):
            f = 1.0 if r == c else 1.0 / SQ2
            S[r, c] = S[c, r] = s[row + triu_index(r, c)] * f
            Z[r, c] = Z[c, r] = z[row + triu_index(r, c)] * f
    assert np.linalg.eigvalsh(S).min() >= -1e-7 * max(1.0, np.linalg.norm(S))
    if complete:
        assert np.linalg.eigvalsh(Z).min() >= -1e-7 * max(1.0, np.linalg.norm(Z))


# ---- 1. sdp_chordal.rs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("complete_dual", [0, 1])
@pytest.mark.parametrize("merge", MERGES)
def test_sdp_chordal_all_settings(hipdev, compact, complete_dual, merge):
    P, q, A, b, cones = sdp_chordal_data()
    plain = make(hipdev, P, q, A, b, cones, max_iter=50).solve()
    slv = make(hipdev, P, q, A, b, cones, max_iter=50, chordal_decomposition_enable=1,
               chordal_decomposition_compact=compact, chordal_decomposition_complete_dual=complete_dual,
               chordal_decomposition_merge_method=merge)
    sol = slv.solve()
    assert sol.status == "Solved" and plain.status == "Solved"
    assert np.linalg.norm(sol.x - plain.x, np.inf) <= 1e-6
    assert len(sol.s) == len(sol.z) == 28
    if merge != "parent_child":
        assert slv.transform_info()["psd_cones_decomposed"] == 1


# ---- 2. presolve.rs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["single", "single_2", "cone", "all"])
def test_presolve_cases(hipdev, case):
    P, q, A, b, cones = presolve_data()
    removed = {"single": [3], "single_2": [4], "cone": [0, 1, 2], "all": list(range(6))}[case]
    if case == "single_2":
        cones = [(0, 2), (NN, 4)]
    b[removed] = 1e30
    slv = make(hipdev, P, q, A, b, cones, presolve_enable=1)
    sol = slv.solve()
    assert sol.status == "Solved"
    assert slv.transform_info()["m_internal"] == 6 - len(removed)
    assert np.all(sol.s[removed] == 1e20) and np.all(sol.z[removed] == 0.0)
    ref = {"cone": np.array([-0.5, 2.0, -0.5]), "all": -q}.get(case)
    if ref is not None:
        assert np.linalg.norm(sol.x - ref) <= 1e-6
    # the same problem with the removed rows left out (the 1e20 rows themselves make the unpresolved solve fail)
    keep = [i for i in range(6) if i not in removed]
    reduced = {"single": [(NN, 3), (NN, 2)], "single_2": [(0, 2), (NN, 3)], "cone": [(NN, 3)], "all": []}[case]
    plain = make(hipdev, P, q, A[keep], b[keep], reduced).solve()
    assert plain.status == "Solved"
    assert np.linalg.norm(sol.x - plain.x) <= 1e-6


# ---- 3. the e2e problems with both transforms on ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["basic_sdp", "mixed_conic"])
def test_e2e_with_transforms_on(hipdev, name):
    pr = getattr(E, name)()
    sol = e2e_solver(hipdev, pr, presolve_enable=1, chordal_decomposition_enable=1).solve()
    assert sol.status == "Solved"
    assert np.linalg.norm(sol.x - np.array(pr["x"])) <= pr["tol"]
    assert abs(sol.obj_val - pr["obj"]) <= pr["tol"]


# ---- 4. banded SDPs against the undecomposed solve ----------------------------------------------------------------------
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("merge", MERGES)
def test_banded_sdp_matches_undecomposed(hipdev, compact, merge):
    N = 80
    P, q, A, b, cones = mask_sdp(banded(N, 3), N, seed=11)
    plain = make(hipdev, P, q, A, b, cones).solve()
    slv = make(hipdev, P, q, A, b, cones, chordal_decomposition_enable=1, chordal_decomposition_compact=compact,
               chordal_decomposition_merge_method=merge)
    sol = slv.solve()
    assert plain.status == "Solved" and sol.status == "Solved"
    info = slv.transform_info()
    assert info["psd_cones_decomposed"] == 1 and info["largest_clique"] < N
    f0 = objective(P, q, plain.x)
    assert abs(objective(P, q, sol.x) - f0) <= 1e-6 * max(1.0, abs(f0))
    assert np.linalg.norm(A @ sol.x + sol.s - b, np.inf) <= 1e-7 * max(1.0, np.linalg.norm(b, np.inf))
    psd_checks(sol.s, sol.z, 0, N, True)


# ---- 5. the device reverse bit for bit ---------------------------------------------------------------------------------
def _infeasible_banded(N):
    P, q, A, b, cones = mask_sdp(banded(N, 2), N, seed=4)
    j = A.shape[1]
    rows = sp.csc_matrix(([1.0, -1.0], ([0, 1], [0, 0])), shape=(2, j))  # x0 <= -1 and x0 >= 1
    return P, q, sp.vstack([rows, A]).tocsc(), np.concatenate([[-1.0, -1.0], b]), [(NN, 2)] + cones


@pytest.mark.parametrize("case", ["compact", "standard", "infeasible", "presolve_compact"])
def test_device_reverse_bitwise(hipdev, case):
    N = 30
    if case == "infeasible":
        P, q, A, b, cones = _infeasible_banded(N)
    elif case == "presolve_compact":
        P, q, A, b, cones = mask_sdp(banded(N, 2), N, seed=3, extra_nn=True)
    else:
        P, q, A, b, cones = mask_sdp(banded(N, 2), N, seed=3)
    kw = dict(presolve_enable=1, chordal_decomposition_enable=1,
              chordal_decomposition_compact=0 if case == "standard" else 1)
    slv = make(hipdev, P, q, A, b, cones, **kw)
    sol = slv.solve()
    if case == "infeasible":
        assert sol.status == "PrimalInfeasible"
    else:
        assert sol.status == "Solved"
    x2, s2, z2 = slv.internal_solution()
    t = debug(hipdev, P, q, A, b, cones, **kw)
    assert t.active and (t.n2, t.m2) == (len(x2), len(s2))
    x, s, z = t.reverse(x2, s2, z2)
    for got, want in ((sol.x, x), (sol.s, s), (sol.z, z)):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    xd, sd, zd = slv.solution_dev()
    assert np.array_equal(xd.numpy().view(np.uint64), x.view(np.uint64))
    assert np.array_equal(zd.numpy().view(np.uint64), z.view(np.uint64))


# ---- 6. updates -----------------------------------------------------------------------------------------------------------
def test_updates_refused_while_a_transform_is_active(hipdev):
    hip = hipdev
    P, q, A, b, cones = presolve_data()
    b[3] = 1e30
    slv = make(hip, P, q, A, b, cones, presolve_enable=1)
    before = slv.solve()
    assert not slv.is_data_update_allowed()
    scaled = slv.scaled_data()
    for key, data in (("P", np.ones(3)), ("A", np.ones(6)), ("q", np.ones(3)), ("b", np.ones(6))):
        with pytest.raises(hip.UpdateNotAllowedError) as e:
            getattr(slv, "update_" + key)(data)
        assert e.value.code == hip.ERR_UPDATE_NOT_ALLOWED
    import ctypes as C
    vals = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert hip.lib().chip_problem_update_q(slv._h, None, vals, C.c_int64(3)) == hip.ERR_UPDATE_NOT_ALLOWED
    assert hip.lib().chip_problem_update_q(slv._h, None, None, C.c_int64(0)) == hip.ERR_UPDATE_NOT_ALLOWED
    for a, c in zip(scaled, slv.scaled_data()):
        assert np.array_equal(a, c)
    again = slv.solve()
    assert np.array_equal(again.x, before.x)
    # the five transform fields are immutable
    for k, v in (("presolve_enable", 0), ("chordal_decomposition_enable", 1),
                 ("chordal_decomposition_merge_method", "none"), ("chordal_decomposition_compact", 0),
                 ("chordal_decomposition_complete_dual", 0)):
        with pytest.raises(hip.ChipError) as e:
            slv.update_settings(**{k: v})
        assert e.value.code == hip.ERR_ARG
    slv.update_settings(max_iter=100)  # the rest still changes


def test_updates_allowed_when_enabled_but_inactive(hipdev):
    P, q, A, b, cones = presolve_data()
    slv = make(hipdev, P, q, A, b, cones, presolve_enable=1, chordal_decomposition_enable=1)
    assert slv.is_data_update_allowed()
    info = slv.transform_info()
    assert info["m_internal"] == info["m_full"] == 6 and info["psd_cones_decomposed"] == 0
    slv.update_q(np.array([1.0, 1.0, 1.0]))
    assert slv.solve().status == "Solved"


# ---- 7. scale ---------------------------------------------------------------------------------------------------------------
def test_side_1000_psd_cone_solves_with_decomposition(hipdev):
    N = 1000
    P, q, A, b, cones = mask_sdp(banded(N, 2), N, seed=1)
    t0 = time.time()
    slv = make(hipdev, P, q, A, b, cones, chordal_decomposition_enable=1)
    sol = slv.solve()
    elapsed = time.time() - t0
    assert sol.status == "Solved", sol
    info = slv.transform_info()
    assert info["psd_cones_decomposed"] == 1 and info["largest_clique"] <= 40
    assert len(sol.s) == tri(N)
    assert np.linalg.norm(A @ sol.x + sol.s - b, np.inf) <= 1e-6 * max(1.0, np.linalg.norm(b, np.inf))
    assert elapsed < 300.0
