"""The batched solver's PSD members (chip_bsym_create, HipBatchSolver(cones="symmetric")) on the MI355X: batches of
one and of five copies of basic_sdp against HipSolver, a heterogeneous batch of Zero / Nonnegative / SecondOrder
members with three SDP members (feasible, primal infeasible, random with PSD(2) + PSD(1) + Nonnegative rows), a
permuted batch, the attribution of a NaN to the PSD member, launch and synchronisation counts that do not grow with
the batch, data updates and re-equilibration, derivatives of the other members of a mixed batch, and a handle of the
new entry without any PSD cone against chip_batch_create's, bit for bit.

The path tolerance of PSD members.  tests/test_batch_gpu.py's TOL_PATH = 1e-7 was derived for Nonnegative and
SecondOrder members.  For PSD members the relative difference of x, s and A'z between the batch and HipSolver on the
same data (two different paths: the batch reduces per member, factors the member inside the stack's elimination
forest and regularises over the stack) is measured by the tests below, which print every figure before they assert.
MEASURED_PSD_PATH holds the worst figure of the first run on one MI355X over the Solved SDP members of every case of
this file; the assertion is 10 x that figure for rounding headroom and never looser than the fixture's own 1e-6.
Measured on that run (iterations batch / HipSolver):
  basic_sdp, one copy and each of five copies        1.8e-16   (9 / 9)
  basic_sdp in the heterogeneous batch of 17         3.8e-15   (9 / 9)
  the random SDP (PSD(2), PSD(1), NN(3)) in it       1.6e-13   (7 / 7)
  the updated basic_sdp                              6.4e-16   (10 / 10)
  the eight projection SDPs of side 6                6.2e-15 .. 4.5e-14 (9 or 10 iterations each) and, for the member
                                                     of seed 307, 2.8e-12 (11 / 11)          -> MEASURED_PSD_PATH
  permuted against ordered batch, either SDP member  1.1e-15
  updated / re-equilibrated handle against a fresh one: 0 for basic_sdp, 1.4e-14 / 0 for the random SDP
(The side-6 case joined the file after the first run of the others, whose worst was the random SDP's 1.6e-13; its own
first run gave the figures above, and the constant is the worst of all of them.  The member of seed 307 is the one
HipSolver itself leaves least converged: r_prim 1e-13 against 1e-15 for the others.)
The iteration counts equalled HipSolver's for every member.  One that differs by more than 1 is a finding, not a bound
to widen."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import e2e_problems as E
from tests.test_batch_adjoint_gpu import GRAD_BOUND, incoming, worst_against_ref
from tests.test_batch_gpu import (REF_STATUS, TOL_PATH, _check_certificate, _mats, _rel, hetero, member, single)

pytestmark = pytest.mark.gpu

ZERO, NN, SOC, EXP, POW, GENPOW, PSD = range(7)

# worst relative difference of x, s, A'z between a batch member and HipSolver over the Solved SDP members (first run)
MEASURED_PSD_PATH = 2.758e-12
TOL_PSD = 1e-6 if MEASURED_PSD_PATH is None else min(1e-6, 10.0 * MEASURED_PSD_PATH)


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def sbatch(hip, prs, **kw):
    return hip.HipBatchSolver([member(hip, p) for p in prs], hip.SolverSettings.default(**kw), cones="symmetric")


# ---- the SDP members ------------------------------------------------------------------------------------------------
def sdp_primal_infeasible():
    """tests/basic_sdp.rs:78-95 of the reference: basic_sdp with A stacked on -A and b on zeros, two PSD(3) cones"""
    pr = E.basic_sdp()
    n, m = pr["n"], pr["m"]
    A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n))
    A2 = sp.vstack([A, -A], format="csc")
    return dict(n=n, m=2 * m, P=pr["P"], A=E._csc(A2), q=pr["q"], b=list(pr["b"]) + [0.0] * m,
                cones=[(PSD, 3), (PSD, 3)])


def _svec(M):
    n = M.shape[0]
    return np.array([M[j, k] * (1.0 if j == k else np.sqrt(2.0)) for k in range(n) for j in range(k + 1)])


def _smat(v, n):
    M = np.zeros((n, n))
    t = 0
    for k in range(n):
        for j in range(k + 1):
            M[j, k] = M[k, j] = v[t] * (1.0 if j == k else np.sqrt(0.5))
            t += 1
    return M


def sdp_random(seed=11):
    """min 1/2 x'Px + q'x, P = GG' + I (n = 4), s.t. Ax + s = b with s in PSD(2) x PSD(1) x NN(3); b = A x0 + s0 with
    s0 strictly inside the cones, so the problem is strictly feasible, and bounded because P is positive definite"""
    r = np.random.default_rng(seed)
    G = r.standard_normal((4, 4))
    A = r.standard_normal((7, 4))
    x0 = r.standard_normal(4)
    M = r.standard_normal((2, 2))
    s0 = np.concatenate([_svec(M @ M.T + np.eye(2)), [1.0 + abs(r.standard_normal())], 0.5 + np.abs(r.standard_normal(3))])
    return dict(n=4, m=7, P=E._triu(G @ G.T + np.eye(4)), A=E._csc(A), q=list(r.standard_normal(4)),
                b=list(A @ x0 + s0), cones=[(PSD, 2), (PSD, 1), (NN, 3)])


def sdp_members():
    return [("sdp", E.basic_sdp()), ("sdp_pinf", sdp_primal_infeasible()), ("sdp_rand", sdp_random())]


STATUS = dict(REF_STATUS, sdp="Solved", sdp_pinf="PrimalInfeasible", sdp_rand="Solved")


def all_members():
    return hetero() + sdp_members()


@pytest.fixture(scope="module")
def refs(hipdev):
    """every member solved once by HipSolver; shared and left unchanged"""
    return {name: single(hipdev, pr).solve() for name, pr in all_members()}


def _has_psd(pr):
    return any(c[0] == PSD for c in pr["cones"])


def _path_diff(pr, sol, ref):
    _, A = _mats(pr)
    return max(_rel(sol.x, ref.x), _rel(sol.s, ref.s), _rel(A.T @ sol.z, A.T @ ref.z))


def _check_psd_certificate(pr, sol):
    """tests/test_batch_gpu.py::_check_certificate (b'z < 0, A'z = 0, the Nonnegative and SecondOrder parts of z), and
    the PSD parts of z inside their (self-dual) cone"""
    _check_certificate(pr, sol)
    if sol.status != "PrimalInfeasible":
        return
    k = 0
    for c in pr["cones"]:
        rows = c[1] * (c[1] + 1) // 2 if c[0] == PSD else c[1]
        if c[0] == PSD:
            ev = np.linalg.eigvalsh(_smat(sol.z[k:k + rows], c[1]))
            assert -ev[0] <= 1e-8 * max(1.0, np.linalg.norm(sol.z, np.inf)), (ev, sol.z)
        k += rows


def _check(name, pr, sol, ref):
    """_check_member of tests/test_batch_gpu.py with the SDP members' statuses and certificates"""
    assert sol.status == ref.status == STATUS[name], (name, sol, ref)
    assert abs(sol.iterations - ref.iterations) <= 1, (name, sol.iterations, ref.iterations)
    if sol.status == "Solved":
        tol = pr.get("tol", 1e-6)
        if pr.get("x") is not None:
            assert np.linalg.norm(sol.x - np.asarray(pr["x"])) <= tol, (name, sol.x)
        if pr.get("obj") is not None:
            assert abs(sol.obj_val - pr["obj"]) <= tol, (name, sol.obj_val)
        if _has_psd(pr):
            d = _path_diff(pr, sol, ref)
            print("PSD path: %s batch vs HipSolver %.3e (bound %.3e), iterations %d / %d"
                  % (name, d, TOL_PSD, sol.iterations, ref.iterations))
            assert d <= TOL_PSD, (name, d)
    else:
        assert np.isnan(sol.obj_val)
        _check_psd_certificate(pr, sol)


# ---- 1. one and five copies ----------------------------------------------------------------------------------------
def test_one_and_five_copies(hipdev, refs):
    pr, ref = E.basic_sdp(), refs["sdp"]
    assert ref.status == "Solved"
    for copies in (1, 5):
        sols = sbatch(hipdev, [pr] * copies).solve()
        assert len(sols) == copies
        for sol in sols:
            assert sol.status == ref.status, (copies, sol, ref)
            assert np.linalg.norm(sol.x - np.asarray(pr["x"])) <= pr["tol"], (copies, sol.x)
            assert abs(sol.obj_val - pr["obj"]) <= pr["tol"], (copies, sol.obj_val)
            d = _path_diff(pr, sol, ref)
            print("PSD path: basic_sdp x %d batch vs HipSolver %.3e (bound %.3e), iterations %d / %d"
                  % (copies, d, TOL_PSD, sol.iterations, ref.iterations))
            assert abs(sol.iterations - ref.iterations) <= 1, (copies, sol.iterations, ref.iterations)
            assert d <= TOL_PSD, (copies, d)
        for sol in sols[1:]:
            assert _rel(sol.x, sols[0].x) <= 1e-12 and _rel(sol.z, sols[0].z) <= 1e-12


# ---- 2. a heterogeneous batch --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ordered(hipdev):
    prs = all_members()
    return prs, sbatch(hipdev, [p for _, p in prs]).solve()


def test_heterogeneous_batch(hipdev, refs, ordered):
    prs, sols = ordered
    for (name, pr), sol in zip(prs, sols):
        _check(name, pr, sol, refs[name])
    assert len({s.iterations for s in sols}) > 1  # each member stops on its own


def projection_sdp(side, seed):
    """min 1/2 x'x + q'x s.t. mat(b - x) PSD for a random symmetric mat(b): basic_sdp's form at another side"""
    r = np.random.default_rng(seed)
    m = side * (side + 1) // 2
    M = r.standard_normal((side, side))
    eye = sp.identity(m, format="csc")
    return dict(n=m, m=m, P=E._triu(eye), A=E._csc(eye), q=list(0.1 * r.standard_normal(m)),
                b=list(_svec(0.5 * (M + M.T))), cones=[(PSD, side)])


def test_members_that_finish_first_do_not_end_the_others(hipdev):
    """Eight projection SDPs of side 6 that HipSolver solves in 9, 10 and 11 iterations.  The members that finish first
    do so with mu near 1e-16, s and z on the cones' boundary within rounding: scaled again at that iterate their
    Cholesky factors break down, and the failure, which no member accounts for, ended the seven others as
    AlmostSolved after 9 iterations.  A member with PSD cones therefore leaves the stack with the unit vector in the
    place of its final iterate (batch.cpp), and every member must end as it does alone"""
    prs = [projection_sdp(6, 300 + i) for i in range(8)]
    singles = [single(hipdev, p).solve() for p in prs]
    assert len({s.iterations for s in singles}) > 1  # (they do finish at different iterations)
    sols = sbatch(hipdev, prs).solve()
    for k, (pr, sol, ref) in enumerate(zip(prs, sols, singles)):
        assert sol.status == ref.status == "Solved", (k, sol, ref)
        assert abs(sol.iterations - ref.iterations) <= 1, (k, sol.iterations, ref.iterations)
        d = _path_diff(pr, sol, ref)
        print("PSD path: projection_sdp(6, %d) batch vs HipSolver %.3e (bound %.3e), iterations %d / %d"
              % (300 + k, d, TOL_PSD, sol.iterations, ref.iterations))
        assert d <= TOL_PSD, (k, d)


# ---- 3. order does not matter --------------------------------------------------------------------------------------
def test_permuted_batch(hipdev, ordered):
    prs, base = ordered
    perm = np.random.default_rng(5).permutation(len(prs))
    assert not np.array_equal(perm, np.arange(len(prs)))
    sols = sbatch(hipdev, [prs[i][1] for i in perm]).solve()
    for j, i in enumerate(perm):
        a, b = sols[j], base[i]
        assert a.status == b.status and a.iterations == b.iterations, (prs[i][0], a, b)
        if a.status != "Solved":
            continue
        psd = _has_psd(prs[i][1])
        worst = max(_rel(a.x, b.x), _rel(a.s, b.s), _rel(a.z, b.z))
        if psd:
            print("PSD path: %s permuted vs ordered batch %.3e (bound %.3e)" % (prs[i][0], worst, TOL_PSD))
        assert worst <= (TOL_PSD if psd else TOL_PATH), (prs[i][0], worst)


# ---- 4. a NaN in the PSD member -------------------------------------------------------------------------------------
def test_nan_attributed_to_the_psd_member(hipdev, refs):
    prs = all_members()
    k = [n for n, _ in prs].index("sdp")
    bs = sbatch(hipdev, [p for _, p in prs])
    clean = bs.solve()
    assert clean[k].status == "Solved" and clean[k].iterations > 3
    bs.debug_inject_nan(k, 3)
    sols = bs.solve()
    assert sols[k].status == "NumericalError", sols[k]
    assert np.all(np.isfinite(sols[k].x)) and np.all(np.isfinite(sols[k].s)) and np.all(np.isfinite(sols[k].z))
    for j, ((name, pr), sol) in enumerate(zip(prs, sols)):
        if j == k:
            continue
        assert sol.status == clean[j].status and sol.iterations == clean[j].iterations, (name, sol, clean[j])
        _check(name, pr, sol, refs[name])


# ---- 5. launches and synchronisations per iteration ----------------------------------------------------------------
def _per_iteration(bs):
    it = bs.debug_counter("loop_iterations")
    assert it > 0
    return bs.debug_counter("host_syncs") / it, bs.debug_counter("launches") / it


def test_counters_do_not_depend_on_nprob(hipdev):
    """A solve's counters are affine in its iterations (host_syncs = 10 per iteration + 1 for the residual pass that
    ends the loop), so the quotient host_syncs / loop_iterations of two batches can only be compared at the same
    number of iterations: basic_sdp takes 9 and basic_socp 8 to Solved (91 / 9 against 81 / 8).  The comparison with
    the SecondOrder-only batch therefore stops both after max_iter = 5 iterations"""
    pr = E.basic_sdp()
    per = []
    for copies in (2, 256, 257):  # (257: the per-member fold's second workgroup, with one member in it)
        bs = sbatch(hipdev, [pr] * copies)
        sols = bs.solve()
        assert all(s.status == "Solved" for s in sols)
        assert _rel(sols[-1].x, sols[0].x) <= 1e-12 and _rel(sols[-1].z, sols[0].z) <= 1e-12
        per.append(_per_iteration(bs))
    assert per[0] == per[1] == per[2], per
    psd = sbatch(hipdev, [pr] * 2, max_iter=5)
    soc = hipdev.HipBatchSolver([member(hipdev, E.basic_socp())] * 2, hipdev.SolverSettings.default(max_iter=5))
    for bs in (psd, soc):
        assert all(s.status == "MaxIterations" for s in bs.solve())
    assert psd.debug_counter("loop_iterations") == soc.debug_counter("loop_iterations") == 5
    (psyncs, plaunches), (syncs, launches) = _per_iteration(psd), _per_iteration(soc)
    print("per iteration: PSD batch %r, SecondOrder batch %r" % ((psyncs, plaunches), (syncs, launches)))
    assert psyncs == syncs, (psyncs, syncs)  # the PSD passes add launches, no host synchronisation
    assert plaunches > launches


# ---- 6. data updates and re-equilibration ---------------------------------------------------------------------------
def _compare_with_fresh(prs, got, want, what):
    """statuses and iteration counts as a fresh handle's; the solutions at 1e-10 for the LP (one path, reproducing:
    tests/test_reequilibrate_gpu.py), at the PSD path tolerance for the members with PSD cones"""
    for k, (pr, a, f) in enumerate(zip(prs, got, want)):
        assert a.status == f.status == "Solved" and a.iterations == f.iterations, (what, k, a, f)
        worst = max(_rel(a.x, f.x), _rel(a.s, f.s), _rel(a.z, f.z))
        tol = TOL_PSD if _has_psd(pr) else 1e-10
        print("%s member %d: |handle - fresh| %.3e (bound %.3e)" % (what, k, worst, tol))
        assert worst <= tol, (what, k, worst)


def test_update_b_of_the_psd_member(hipdev):
    prs = [E.basic_lp(), E.basic_sdp(), sdp_random()]
    bs = sbatch(hipdev, prs, equilibrate_enable=0)
    first = bs.solve()
    newb = 1.1 * np.asarray(prs[1]["b"]) + 0.05
    bs.update(b=[None, newb, None])
    prs2 = [prs[0], dict(prs[1], b=list(newb), x=None, obj=None), prs[2]]
    fresh = sbatch(hipdev, prs2, equilibrate_enable=0)
    for x, y in zip(bs.scaled_data(), fresh.scaled_data()):  # the same data, so the same path
        assert x.tobytes() == y.tobytes()
    sols = bs.solve()
    _compare_with_fresh(prs2, sols, fresh.solve(), "updated")
    assert _rel(sols[1].x, first[1].x) > 1e-3  # (the update changed the member's answer)
    ref = single(hipdev, prs2[1], equilibrate_enable=0).solve()
    d = _path_diff(prs2[1], sols[1], ref)
    print("PSD path: updated basic_sdp batch vs HipSolver %.3e (bound %.3e), iterations %d / %d"
          % (d, TOL_PSD, sols[1].iterations, ref.iterations))
    assert ref.status == "Solved" and abs(sols[1].iterations - ref.iterations) <= 1 and d <= TOL_PSD


def _state(h):
    out = [np.asarray(a).tobytes() for a in h.scaled_data()]
    for d, e, c in (h.equilibration(k) for k in range(len(h))):
        out += [d.tobytes(), e.tobytes(), np.float64(c).tobytes()]
    return out


def test_reequilibrate(hipdev):
    prs = [E.basic_lp(), E.basic_sdp(), sdp_random()]
    # the drifted data: P x 1.3, q + 0.1, A x 0.9 with its columns spread over two decades, b x 1.2
    prs2 = []
    for j, pr in enumerate(prs):
        col = np.repeat(np.arange(pr["n"]), np.diff(pr["A"][0]))
        spread = 10.0 ** (((col + j) % 3) - 1.0)
        prs2.append(dict(pr, P=(pr["P"][0], pr["P"][1], 1.3 * np.asarray(pr["P"][2], float)),
                         q=list(np.asarray(pr["q"], float) + 0.1),
                         A=(pr["A"][0], pr["A"][1], 0.9 * spread * np.asarray(pr["A"][2], float)),
                         b=list(1.2 * np.asarray(pr["b"], float)), x=None, obj=None))
    stacked = [np.concatenate([np.asarray(p[key][2] if key in "PA" else p[key], float) for p in prs2]) for key in "PqAb"]
    h = sbatch(hipdev, prs)
    before = _state(h)
    fresh = sbatch(hipdev, prs2)
    want = _state(fresh)
    assert before != want  # (the scalings really change)
    h.solve()
    h.reequilibrate(*stacked)
    assert _state(h) == want
    _compare_with_fresh(prs2, h.solve(), fresh.solve(), "re-equilibrated")


# ---- 7. derivatives: the PSD members have none, the others keep theirs -----------------------------------------------
def test_backward_of_a_mixed_batch(hipdev):
    prs = [E.basic_lp(), E.basic_sdp(), E.basic_eq_constrained(), sdp_random()]
    bs = sbatch(hipdev, prs)
    sols = bs.solve()
    assert [s.status for s in sols] == ["Solved"] * 4
    gx, gz, gs = incoming(prs, 21)
    grad = bs.backward(gx, gz, gs)
    assert list(grad.valid) == [1, 0, 1, 0]
    for k in (1, 3):
        for v in grad.per_member(k):
            v = np.asarray(v)
            assert np.all(v == 0.0) and not np.any(np.signbit(v)), (k, v)
    worst = worst_against_ref(prs, sols, grad, gx, gz, gs, members=[0, 2])
    print("gradients of basic_lp and basic_eq beside PSD members vs adjoint_ref: %.3e (bound %.3e)" % (worst, GRAD_BOUND))
    assert worst <= GRAD_BOUND, worst
    again = bs.solve()  # a solve after the backward starts from default_start: the same answers
    for a, b in zip(again, sols):
        assert a.status == b.status and a.iterations == b.iterations


# ---- 8. no PSD cone: the old handle, bit for bit --------------------------------------------------------------------
def test_without_psd_cones_equals_the_old_entry(hipdev):
    """Two HANDLES are compared, so the bytes can only be asked of members whose solve reproduces between two fresh
    handles of chip_batch_create itself: basic_lp, basic_eq and basic_unc differ by exactly 0 there, the other members
    by the accumulation order of the factorisation's atomic adds (tests/test_batch_update_gpu.py::
    _reproducible_members).  Those three in one batch: bit-identical solutions and identical counters.  All of
    hetero(): identical counters, statuses and iteration counts, the solutions within TOL_PATH."""
    names = ("basic_lp", "basic_eq", "basic_unc")
    prs = [p for n, p in hetero() if n in names]
    assert len(prs) == 3
    old = hipdev.HipBatchSolver([member(hipdev, p) for p in prs])
    new = sbatch(hipdev, prs)
    for k, (a, b) in enumerate(zip(old.solve(), new.solve())):
        assert a.status == b.status == "Solved" and a.iterations == b.iterations, (k, a, b)
        for u, v in ((a.x, b.x), (a.s, b.s), (a.z, b.z)):
            assert u.tobytes() == v.tobytes(), (k, u, v)
        assert np.float64(a.obj_val).tobytes() == np.float64(b.obj_val).tobytes(), k
    for name in ("host_syncs", "launches", "loop_iterations"):
        assert old.debug_counter(name) == new.debug_counter(name), name
    prs = [p for _, p in hetero()]
    old = hipdev.HipBatchSolver([member(hipdev, p) for p in prs])
    new = sbatch(hipdev, prs)
    for k, (a, b) in enumerate(zip(old.solve(), new.solve())):
        assert a.status == b.status and a.iterations == b.iterations, (k, a, b)
        if a.status == "Solved":
            assert max(_rel(a.x, b.x), _rel(a.s, b.s)) <= TOL_PATH, k
    for name in ("host_syncs", "launches", "loop_iterations"):
        assert old.debug_counter(name) == new.debug_counter(name), name
