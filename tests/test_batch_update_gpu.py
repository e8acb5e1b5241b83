"""The batched solver's data updates (chip_bdata_*, HipBatchSolver.update) on the MI355X: the scaled stack against a
numpy restatement with one cost scale per member (bit for bit) and the members' norms, refusals that change nothing,
an updated batch against a fresh one on the same path and against fresh single solvers with the equilibration on,
members that an update does not touch, the device forms against the host forms, update_settings, launches and host
synchronisations that do not depend on the batch, and config 4's members at scale."""
import ctypes as C

import numpy as np
import pytest

from tests import e2e_problems as E
from tests.test_batch_gpu import (TOL_PATH, _check_certificate, _hs35, _mats, _rel, batch, feasible,
                                  primal_infeasible, single)
from tests.test_problem_update_gpu import _new_data, _with

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def _solved_members():
    """hetero()'s Solved members plus hs35"""
    return feasible() + [("hs35", _hs35())]


def _reproducible_members():
    """The members for the comparisons of two handles' solves to 1e-10 (the single solver's bound for two handles on
    one path).  That bound presumes that the reference -- a fresh HipBatchSolver -- reproduces its own solve far below
    it.  Measured on the batched solver as it was before the updates existed (fresh handles, one handle solved twice,
    equilibrate_enable=0, max |dx| / |ds| / |dz|): basic_lp, basic_eq, basic_unc 0, hs35 <= 2e-14, basic_qp <= 5e-15
    (but its z is not unique, see test_batch_of_one_and_copies: 4e-7 once the data is scaled with an older
    equilibration), basic_socp_sparse 2e-13 / 3e-11 / 7e-14 and basic_socp 1.6e-7 / 3.3e-7 / 1.3e-7: the last
    iterations amplify the accumulation order of the factorisation's atomic adds.  So these comparisons take the four
    members that reproduce to 1e-13; the SOC members' updates are held to the exact scaled data (test 1, and the
    byte comparison of test 3) and to the residual and objective checks of tests 4, 5 and 9."""
    keep = ("basic_lp", "basic_eq", "basic_unc", "hs35")
    return [(n, p) for n, p in _solved_members() if n in keep]


def _unique_members():
    """six members whose primal-dual solution is unique, for the comparison of an untouched member's solution before
    and after an update: feasible() with hs35 in the place of basic_qp, whose z is unique only up to a shift of the
    multipliers of its two parallel rows (test_batch_of_one_and_copies) and moves by 7e-7 along it when x and s move
    by 1e-13"""
    return [("hs35", _hs35())] + feasible()[1:]


def _stack_coords(bs, key):
    p, i, _ = bs.stack[key]
    cols = np.repeat(np.arange(len(p) - 1), np.diff(p.astype(np.int64)))
    return i.astype(np.int64), cols


def _stack_equilibration(bs):
    """(d, e, c per column, c per member) of the stack from equilibration(k) of every member"""
    ds, es, cs = zip(*(bs.equilibration(k) for k in range(len(bs))))
    ccol = np.concatenate([np.full(len(d), c) for d, c in zip(ds, cs)])
    return np.concatenate(ds), np.concatenate(es), ccol, np.array(cs)


def _member_max(v, parts):
    off = np.concatenate([[0], np.cumsum(parts)]).astype(int)
    return np.array([np.max(np.abs(v[off[k]:off[k + 1]]), initial=0.0) for k in range(len(parts))])


def _inf(v):
    return float(np.max(np.abs(v), initial=0.0))


def _check_against_fresh(hip, k, pr2, sol):
    """item 4's checks of one member on its UPDATED unscaled data: Solved, the relative primal and dual residuals of
    test_config4_members_at_scale <= 1e-7, the objective within 1e-6 of a fresh single solver's, which must itself
    report Solved"""
    ref = single(hip, pr2).solve()
    assert ref.status == "Solved", (k, ref)
    assert sol.status == "Solved", (k, sol)
    P, A = _mats(pr2)
    q, b = np.asarray(pr2["q"], float), np.asarray(pr2["b"], float)
    Ax, Px, Atz = A @ sol.x, P @ sol.x, A.T @ sol.z
    rp = _inf(Ax + sol.s - b) / max(1.0, _inf(b), _inf(Ax), _inf(sol.s))
    rd = _inf(Px + q + Atz) / max(1.0, _inf(q), _inf(Px), _inf(Atz))
    print("member %d: rp %.3e rd %.3e obj %.12g fresh %.12g" % (k, rp, rd, sol.obj_val, ref.obj_val))
    assert rp <= 1e-7 and rd <= 1e-7, (k, rp, rd)
    assert abs(sol.obj_val - ref.obj_val) <= 1e-6 * max(1.0, abs(ref.obj_val)), (k, sol.obj_val, ref.obj_val)


# ---- 1. the scaled stack and the members' norms, bit for bit --------------------------------------------------------
def test_scaled_stack_bitwise(hipdev):
    prs = [p for _, p in _solved_members()]
    bs = batch(hipdev, prs)
    bs.solve()
    d, e, ccol, cs = _stack_equilibration(bs)
    assert np.any(cs != 1.0), cs
    eq0 = [tuple(np.asarray(a).tobytes() for a in bs.equilibration(k)[:2]) + (bs.equilibration(k)[2],)
           for k in range(len(bs))]
    Pr, Pc = _stack_coords(bs, "P")
    Ar, Ac = _stack_coords(bs, "A")
    nP, nA, n, m = len(Pr), len(Ar), bs.stack["n"], bs.stack["m"]
    rng = np.random.default_rng(11)
    # the norms create took from the user's data
    got = bs.scaled_data()
    assert np.array_equal(got[4], _member_max(bs.stack["q"], bs.n_part))
    assert np.array_equal(got[5], _member_max(np.minimum(bs.stack["b"], 1e20), bs.m_part))  # (create caps b)
    # full forms
    vP, vA, vq, vb = (rng.standard_normal(k) * 100 for k in (nP, nA, n, m))
    bs.update(P=vP, A=vA, q=vq, b=vb)
    Px, Ax, q, b, nq, nb = bs.scaled_data()
    assert Px.tobytes() == ((vP * (d[Pr] * d[Pc])) * ccol[Pc]).tobytes()
    assert Ax.tobytes() == (vA * (e[Ar] * d[Ac])).tobytes()
    assert q.tobytes() == ((vq * d) * ccol).tobytes()
    assert b.tobytes() == (vb * e).tobytes()
    uq, ub = vq.copy(), vb.copy()  # the unscaled data as it stands
    assert np.array_equal(nq, _member_max(uq, bs.n_part)) and np.array_equal(nb, _member_max(ub, bs.m_part))
    # partial forms, with repeated indices: the last occurrence wins
    for key, ln in (("P", nP), ("A", nA), ("q", n), ("b", m)):
        idx = rng.integers(0, ln, 2 * ln + 3)
        vals = rng.standard_normal(len(idx)) * 100
        getattr(bs, "update_" + key)((idx, vals))
        last = {int(i): v for i, v in zip(idx, vals)}
        ii = np.array(sorted(last))
        vv = np.array([last[i] for i in ii])
        if key == "P":
            Px[ii] = ((d[Pr[ii]] * d[Pc[ii]]) * ccol[Pc[ii]]) * vv
        elif key == "A":
            Ax[ii] = (e[Ar[ii]] * d[Ac[ii]]) * vv
        elif key == "q":
            q[ii] = (vv * d[ii]) * ccol[ii]
            uq[ii] = vv
        else:
            b[ii] = vv * e[ii]
            ub[ii] = vv
        got = bs.scaled_data()
        for x, y in zip(got[:4], (Px, Ax, q, b)):
            assert x.tobytes() == y.tobytes(), key
        assert np.array_equal(got[4], _member_max(uq, bs.n_part)), key
        assert np.array_equal(got[5], _member_max(ub, bs.m_part)), key
    # an untouched entry keeps its place in the member's norm: one entry of member 0 made small, the rest decide
    bs.update_q(([0], [1e-3]))
    uq[0] = 1e-3
    assert np.array_equal(bs.scaled_data()[4], _member_max(uq, bs.n_part))
    # b is not capped at 1e20 by an update, and its norm follows the uncapped value
    bs.update_b(([0], [1e30]))
    ub[0] = 1e30
    got = bs.scaled_data()
    assert got[3][0] == 1e30 * e[0] and np.array_equal(got[5], _member_max(ub, bs.m_part))
    # a NaN written into one member's q shows in that member's normq only
    xoff = np.concatenate([[0], np.cumsum(bs.n_part)]).astype(int)
    bs.update_q(([xoff[2] + 1], [np.nan]))
    nq = bs.scaled_data()[4]
    want = _member_max(uq, bs.n_part)
    assert np.isnan(nq[2]) and np.array_equal(np.delete(nq, 2), np.delete(want, 2)), (nq, want)
    eq1 = [tuple(np.asarray(a).tobytes() for a in bs.equilibration(k)[:2]) + (bs.equilibration(k)[2],)
           for k in range(len(bs))]
    assert eq0 == eq1


# ---- 2. refusals change nothing -----------------------------------------------------------------------------------
def test_refusals_change_nothing(hipdev):
    import torch
    prs = [p for _, p in _solved_members()]
    bs = batch(hipdev, prs)
    before = [a.tobytes() for a in bs.scaled_data()]
    lens = {"P": len(bs.stack["P"][2]), "A": len(bs.stack["A"][2]), "q": bs.stack["n"], "b": bs.stack["m"]}
    for key, ln in lens.items():
        with pytest.raises(hipdev.ChipError) as e:  # one bad index among good ones
            getattr(bs, "update_" + key)(([0, 1, ln, 2], [1.0, 2.0, 3.0, 4.0]))
        assert e.value.code == hipdev.ERR_DIM
        with pytest.raises(hipdev.ChipError) as e:
            getattr(bs, "update_" + key)(np.ones(ln + 1))
        assert e.value.code == hipdev.ERR_DIM
        # the library's own check of a full length (below the Python classifier)
        v = np.ones(ln - 1)
        rc = getattr(hipdev.lib(), "chip_bdata_update_" + key)(bs._h, None, v.ctypes.data_as(hipdev.P_F64),
                                                                 C.c_int64(ln - 1))
        assert rc == hipdev.ERR_DIM
        vd = torch.ones(ln + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = getattr(hipdev.lib(), "chip_bdata_update_%s_dev" % key)(bs._h, None, C.c_void_p(vd.data_ptr()),
                                                                       C.c_int64(ln + 1))
        assert rc == hipdev.ERR_DIM
        with pytest.raises(hipdev.ChipError) as e:  # a negative device index
            getattr(bs, "update_" + key)((torch.tensor([0, -1], dtype=torch.int64, device="cuda"),
                                          torch.ones(2, dtype=torch.float64, device="cuda")))
        assert e.value.code == hipdev.ERR_DIM
        with pytest.raises(hipdev.ChipError) as e:  # a too-large one
            getattr(bs, "update_" + key)((torch.tensor([1, ln], dtype=torch.int64, device="cuda"),
                                          torch.ones(2, dtype=torch.float64, device="cuda")))
        assert e.value.code == hipdev.ERR_DIM
        assert [a.tobytes() for a in bs.scaled_data()] == before, key
        # k == 0 is CHIP_OK and changes nothing
        assert getattr(hipdev.lib(), "chip_bdata_update_" + key)(bs._h, None, None, C.c_int64(0)) == 0
        assert [a.tobytes() for a in bs.scaled_data()] == before, key
    sols = bs.solve()
    clean = batch(hipdev, prs).solve()
    for a, b in zip(sols, clean):
        assert a.status == b.status and a.iterations == b.iterations, (a, b)


# ---- 3. updated against fresh, same path --------------------------------------------------------------------------
def _new_members(prs, recipe):
    return [_with(pr, **dict(zip(("P", "A", "q", "b"), recipe(pr)))) for pr in prs]


def _stacked(prs2, key):
    return np.concatenate([np.asarray(p[key][2] if key in "PA" else p[key], float) for p in prs2])


def test_updated_matches_fresh_batch(hipdev):
    prs = [p for _, p in _reproducible_members()]
    bs = batch(hipdev, prs, equilibrate_enable=0)
    bs.solve()
    prs2 = _new_members(prs, lambda pr: _new_data(pr, 7))
    P2, A2, q2, b2 = (_stacked(prs2, k) for k in ("P", "A", "q", "b"))
    rng = np.random.default_rng(8)
    # mixed forms: P as the stack's matrix, A as a shuffled tuple of every entry, q as a list with one vector per
    # member, b as two partial updates
    n, m = bs.stack["n"], bs.stack["m"]
    bs.update(P=hipdev.CscMatrix(n, n, bs.stack["P"][0], bs.stack["P"][1], P2))
    perm = rng.permutation(len(A2))
    bs.update_A((perm, A2[perm]))
    bs.update_q([np.asarray(p["q"], float) for p in prs2])
    half = m // 2
    bs.update_b((np.arange(half), b2[:half]))
    bs.update_b((np.arange(half, m), b2[half:]))
    sols = bs.solve()
    fb = batch(hipdev, prs2, equilibrate_enable=0)
    for x, y in zip(bs.scaled_data(), fb.scaled_data()):  # the same data, so the same path
        assert x.tobytes() == y.tobytes()
    fresh = fb.solve()
    for k, (sol, fr) in enumerate(zip(sols, fresh)):
        assert sol.status == fr.status and sol.iterations == fr.iterations, (k, sol, fr)
        tol = 1e-10 * max(1.0, _inf(fr.x))
        for a, f in ((sol.x, fr.x), (sol.s, fr.s), (sol.z, fr.z)):
            print("member %d: |updated - fresh| %.3e (bound %.3e)" % (k, _inf(a - f), tol))
            assert _inf(a - f) <= tol, (k, _inf(a - f))


# ---- 4. updated against the truth, equilibration on ---------------------------------------------------------------
def _feasible_recipe(pr):
    """new data that keeps a feasible member feasible: P times 1.25, A times 0.9 and b times 1.1 uniformly (a
    feasible (x, s) of the old data scaled by 1.1 / 0.9 is feasible for the new: the cones are cones), q perturbed as
    _new_data does"""
    return (np.asarray(pr["P"][2], float) * 1.25, np.asarray(pr["A"][2], float) * 0.9, _new_data(pr, 7)[2],
            np.asarray(pr["b"], float) * 1.1)


def test_updated_matches_fresh_single_solvers(hipdev):
    prs = [p for _, p in _solved_members()]
    bs = batch(hipdev, prs)
    first = bs.solve()
    assert all(s.status == "Solved" for s in first), first
    prs2 = _new_members(prs, _feasible_recipe)
    bs.update(P=_stacked(prs2, "P"), q=_stacked(prs2, "q"), A=_stacked(prs2, "A"), b=_stacked(prs2, "b"))
    sols = bs.solve()
    assert len(sols) == len(prs2) == 7
    for k, (pr2, sol) in enumerate(zip(prs2, sols)):
        _check_against_fresh(hipdev, k, pr2, sol)


# ---- 5. only the touched members move -----------------------------------------------------------------------------
def test_only_touched_members_move(hipdev):
    prs = [p for _, p in _unique_members()]
    bs = batch(hipdev, prs)
    first = bs.solve()
    assert all(s.status == "Solved" for s in first), first
    touched = (1, 4)
    newq = {k: _new_data(prs[k], 7)[2] for k in touched}
    bs.update_q([newq.get(k) for k in range(len(prs))])
    sols = bs.solve()
    for k, (pr, a, b) in enumerate(zip(prs, sols, first)):
        if k in touched:
            _check_against_fresh(hipdev, k, _with(pr, q=newq[k]), a)
            continue
        assert a.status == b.status and abs(a.iterations - b.iterations) <= 1, (k, a, b)
        for u, v in ((a.x, b.x), (a.s, b.s), (a.z, b.z)):
            print("member %d: untouched, moved by %.3e" % (k, _rel(u, v)))
            assert _rel(u, v) <= TOL_PATH, (k, u, v)


def test_update_to_infeasible_and_back(hipdev):
    prs = [p for _, p in feasible()]
    k = [n for n, _ in feasible()].index("basic_lp")
    pinf = dict(primal_infeasible())["pinf_lp"]
    bs = batch(hipdev, prs)
    first = bs.solve()
    assert all(s.status == "Solved" for s in first), first
    bs.update_b([([0, 3], [-1.0, -1.0]) if j == k else None for j in range(len(prs))])
    sols = bs.solve()
    assert sols[k].status == "PrimalInfeasible", sols[k]
    assert np.isnan(sols[k].obj_val)
    _check_certificate(pinf, sols[k])
    for j, s in enumerate(sols):
        assert j == k or s.status == "Solved", (j, s)
    old = np.asarray(prs[k]["b"], float)
    bs.update_b([([0, 3], old[[0, 3]]) if j == k else None for j in range(len(prs))])
    third = bs.solve()
    assert all(s.status == "Solved" for s in third), third
    assert abs(third[k].iterations - first[k].iterations) <= 1, (third[k], first[k])
    print("back to feasible: x moved by %.3e" % _rel(third[k].x, first[k].x))
    assert _rel(third[k].x, first[k].x) <= TOL_PATH


# ---- 6. the device forms ------------------------------------------------------------------------------------------
def _host_and_device_updated(hip, prs):
    import torch
    bh, bd = batch(hip, prs), batch(hip, prs)
    prs2 = _new_members(prs, _feasible_recipe)
    P2, A2, q2, b2 = (_stacked(prs2, k) for k in ("P", "A", "q", "b"))
    rng = np.random.default_rng(5)
    ib = rng.integers(0, len(b2), 40)
    vb = b2[ib] * rng.uniform(1.0, 1.05, 40)
    iP = rng.integers(0, len(P2), 10)
    vP = P2[iP] * 1.1
    iA = rng.integers(0, len(A2), 10)
    iq = rng.integers(0, len(q2), 5)
    bh.update(P=P2, A=A2, q=q2, b=(ib, vb))
    bh.update(P=(iP, vP), A=(iA, A2[iA]), q=(iq, q2[iq]), b=b2)
    dev = lambda a, t=torch.float64: torch.tensor(np.asarray(a), dtype=t, device="cuda")  # noqa: E731
    i64 = torch.int64
    bd.update(P=dev(P2), A=dev(A2), q=dev(q2), b=(dev(ib, i64), dev(vb)))
    bd.update(P=(dev(iP, i64), dev(vP)), A=(dev(iA, i64), dev(A2[iA])), q=(dev(iq, i64), dev(q2[iq])), b=dev(b2))
    for x, y in zip(bh.scaled_data(), bd.scaled_data()):
        assert x.tobytes() == y.tobytes()
    return bh, bd


def test_device_forms_equal_host_forms(hipdev):
    bh, bd = _host_and_device_updated(hipdev, [p for _, p in _reproducible_members()])
    for k, (a, b) in enumerate(zip(bh.solve(), bd.solve())):
        assert a.status == b.status and a.iterations == b.iterations, (k, a, b)
        print("member %d: |host - device| %.3e" % (k, _inf(a.x - b.x)))
        assert _inf(a.x - b.x) <= 1e-10 * max(1.0, _inf(a.x)), (k, _inf(a.x - b.x))


def test_device_forms_equal_host_forms_data_of_every_member(hipdev):
    """the byte comparison of the two handles' data on the whole set of members, second-order cones included (their
    solves are compared above only for the members _reproducible_members() names)"""
    bh, bd = _host_and_device_updated(hipdev, [p for _, p in _solved_members()])
    for k, (a, b) in enumerate(zip(bh.solve(), bd.solve())):
        assert a.status == b.status == "Solved" and a.iterations == b.iterations, (k, a, b)


# ---- 7. settings ------------------------------------------------------------------------------------------------
def test_update_settings(hipdev):
    prs = [p for _, p in _solved_members()]
    bs = batch(hipdev, prs)
    base = bs.solve()
    assert all(s.status == "Solved" for s in base)
    assert any(s.iterations > 2 for s in base)
    bs.update_settings(max_iter=2)
    for k, (s, b0) in enumerate(zip(bs.solve(), base)):
        assert s.status == ("MaxIterations" if b0.iterations > 2 else "Solved"), (k, s, b0)
    bs.update_settings(max_iter=200)
    for s, b0 in zip(bs.solve(), base):
        assert s.status == "Solved" and s.iterations == b0.iterations
    bs.update(settings=hipdev.SolverSettings.from_buffer_copy(bs.settings))  # the same settings: accepted
    for kw in (dict(equilibrate_enable=0), dict(equilibrate_max_iter=3), dict(equilibrate_min_scaling=1e-3),
               dict(equilibrate_max_scaling=1e3), dict(static_regularization_constant=1e-7),
               dict(iterative_refinement_max_iter=3), dict(linesearch_backtrack_step=0.5),
               dict(min_terminate_step_length=1e-3), dict(presolve_enable=1), dict(chordal_decomposition_enable=1)):
        old = bytes(bs.settings)
        with pytest.raises(hipdev.ChipError) as e:
            bs.update_settings(**kw)
        assert e.value.code == hipdev.ERR_ARG, kw
        assert bytes(bs.settings) == old
    for s, b0 in zip(bs.solve(), base):  # the old settings stay in force
        assert s.status == "Solved" and s.iterations == b0.iterations


# ---- 8. the cost of an update does not depend on the batch ----------------------------------------------------------
def test_update_cost_does_not_depend_on_nprob(hipdev):
    pr = E.basic_socp()
    cost = []
    for copies in (2, 256):
        bs = batch(hipdev, [pr] * copies)
        per = []
        for _ in range(2):  # the first update (it sets the work buffers up) and a later one
            bs.update_q(np.tile(np.asarray(pr["q"], float), copies) * 1.01)
            per.append((bs.debug_counter("update_launches"), bs.debug_counter("update_host_syncs")))
        assert per[0][1] == 1 and per[1][1] == 1, per
        # a partial update that touches every member, and one that touches a single member
        bs.update_b((np.arange(copies) * pr["m"], np.full(copies, pr["b"][0])))
        per.append((bs.debug_counter("update_launches"), bs.debug_counter("update_host_syncs")))
        bs.update_b(([0], [pr["b"][0]]))
        per.append((bs.debug_counter("update_launches"), bs.debug_counter("update_host_syncs")))
        assert per[2] == per[3] and per[2][1] == 1, per
        assert all(s.status == "Solved" for s in bs.solve())
        cost.append(per)
    assert cost[0] == cost[1], cost
    with pytest.raises(hipdev.ChipError) as e:
        bs.debug_counter("no_such_counter")
    assert e.value.code == hipdev.ERR_ARG


# ---- 9. config 4 at scale -------------------------------------------------------------------------------------------
def test_config4_update_at_scale(hipdev):
    import torch
    from clarabel_rs_amd import synthetic
    nprob, nblocks, dim = 1024, 2, 1001
    prs = [synthetic.portfolio_problem(nblocks, 1000, seed=100 + i) for i in range(nprob)]
    bs = batch(hipdev, prs)
    sols = bs.solve()
    assert all(s.status == "Solved" for s in sols), [s.status for s in sols if s.status != "Solved"][:5]
    zoff = np.concatenate([[0], np.cumsum(bs.m_part)]).astype(np.int64)
    q2, ib, gam = [], [], []
    for i, pr in enumerate(prs):  # the recipe of test_portfolio_update_at_scale, per member
        rng = np.random.default_rng(77 + i)
        q2.append(-rng.uniform(0.0, 1.0, pr["n"]))  # new returns
        ib.append(1 + pr["n"] + dim * np.arange(nblocks))  # the member's risk budgets
        gam.append(rng.uniform(1.0, 2.5, nblocks) / np.sqrt(1000))
    bs.update_q(torch.tensor(np.concatenate(q2), dtype=torch.float64, device="cuda"))
    bs.update_b((np.concatenate([zoff[i] + ib[i] for i in range(nprob)]), np.concatenate(gam)))
    sols = bs.solve()
    assert len(sols) == nprob
    assert all(s.status == "Solved" for s in sols), [(i, s.status) for i, s in enumerate(sols) if s.status != "Solved"][:5]
    for i in np.random.default_rng(0).choice(nprob, 8, replace=False):
        b2 = np.asarray(prs[i]["b"], float).copy()
        b2[ib[i]] = gam[i]
        _check_against_fresh(hipdev, int(i), _with(prs[i], q=q2[i], b=b2), sols[i])
