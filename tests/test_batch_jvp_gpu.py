"""The batched solver's forward-mode derivatives (chip_bjvp_*, HipBatchSolver.jvp, layer.BatchQPFunction.jvp) on the
MI355X: the device tangents against the numpy restatement of tests/tangent_ref.py evaluated at the device's own
solution, against their transpose (backward) on the device, against central differences through update + re-solve, a
heterogeneous batch with members that have no derivative, the input forms and refusals, the handle's state around an
apply (reuse of the factorisation, a solve after an apply, backward between applies), launch counts that do not grow
with the batch, the right-hand side pass alone on rows of every length class, and the torch layer.

TAN_BOUND, DUAL_BOUND and FD_BOUND are ten times the worst figure measured on the MI355X over the members below, and
never looser than their ceilings: 1e-6 (device against restatement, and duality on the device: anything worse is an
error, not rounding) and 1e-4 (central differences: the CPU bound of tests/test_batch_jvp_host.py).  While a
MEASURED_* constant is None its ceiling applies.  Measured on the first run of this file (one MI355X):
  device against tangent_ref at the device's own (x, s, z), eight members: host and device form 3.5e-14 (dq only) and
  2.2e-13 (all four inputs; 2.0e-13 in a second run: another solve), the list form 8.3e-14, the 8-byte aligned
  inputs 6.3e-14, the heterogeneous batch's valid members 9.2e-14                                    -> MEASURED_TAN
  g.(dx, dz, ds) against (dq, db, dP, dA).d of one backward and one jvp of one solve, and A dx + ds = db - dA x on the
  Nonnegative rows: 1.1e-15 (6.2e-16 in a second run)                                              -> MEASURED_DUAL
  (dx, dz, ds) of random_qp_1 against central differences (h = 1e-4) through update + re-solve: 1.5e-7 / 4.2e-7 /
  1.7e-7                                                                                           -> MEASURED_FD
  (not asserted against figures of their own: a backward between two applies against a backward alone 3.4e-15, the
  second apply against the first 7.1e-15, the layer's tangents against jvp() 7.7e-18; the right-hand side pass used
  0.41 (x space) and 0.20 (z space) of its derived bound at worst)
The right-hand side pass is held to the rounding bound of any summation order, which is derived, not measured."""
import math

import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import e2e_problems as E
from tests import tangent_ref as T
from tests.test_batch_adjoint_gpu import REPEAT_BOUND
from tests.test_batch_gpu import dual_infeasible, member, primal_infeasible

pytestmark = pytest.mark.gpu

# worst relative difference device / tangent_ref over the members, every form and input set
MEASURED_TAN = 2.197e-13
TAN_BOUND = 1e-6 if MEASURED_TAN is None else min(1e-6, 10.0 * MEASURED_TAN)
# worst duality gap |g.t - grad.d| / max(1, |.|) per member, and worst residual of A dx + ds = db - dA x
MEASURED_DUAL = 1.123e-15
DUAL_BOUND = 1e-6 if MEASURED_DUAL is None else min(1e-6, 10.0 * MEASURED_DUAL)
# worst relative difference of dx, dz, ds against central differences (h = 1e-4) through update + re-solve
MEASURED_FD = 4.214e-7
FD_BOUND = 1e-4 if MEASURED_FD is None else min(1e-4, 10.0 * MEASURED_FD)
# two results of one solve that the factorisation's atomic adds tell apart: the adjoint test's bound, ceiling 1e-6
REPEAT_CEILING = 1e-6

KEYS = ("q", "b", "P", "A")


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def batch(hip, prs, **kw):
    return hip.HipBatchSolver([member(hip, p) for p in prs], hip.SolverSettings.default(**kw))


def members():
    return [pr for _, pr in T.gpu_members()]


def length(pr, key):
    return {"q": pr["n"], "b": pr["m"], "P": len(pr["P"][2]), "A": len(pr["A"][2])}[key]


def directions(prs, seed, only_dq=False):
    """one random direction per member, stacked: [dq, db, dP, dA] (None where absent)"""
    per = [T.direction(pr, seed + 17 * k) for k, pr in enumerate(prs)]
    out = [np.concatenate([d[i] for d in per]) for i in range(4)]
    return [out[0], None, None, None] if only_dq else out


def split(prs, v, key):
    if v is None:
        return [None] * len(prs)
    off = np.concatenate([[0], np.cumsum([length(pr, key) for pr in prs])]).astype(int)
    return [v[off[k]:off[k + 1]] for k in range(len(prs))]


def to_host(v):
    return v.detach().cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def worst_against_ref(prs, sols, tan, d, only=None):
    """the worst relative difference of the members' three tangents against tangent_ref at the device's own solution"""
    pieces = [split(prs, v, key) for v, key in zip(d, KEYS)]
    worst = 0.0
    for k, pr in enumerate(prs):
        if only is not None and k not in only:
            continue
        want = T.tangent(pr, sols[k].x, sols[k].s, sols[k].z, *[p[k] for p in pieces])
        got = [to_host(v) for v in tan.per_member(k)]
        for w, g in zip(want, got):
            worst = max(worst, R.rel(g, w))
        nn = T.nn_rows(pr)
        assert np.all(got[2][~nn] == 0.0) and not np.any(np.signbit(got[2][~nn])), k  # ds on Zero rows: exact +0.0
    return worst


@pytest.fixture(scope="module")
def solved(hipdev):
    """one batch of the eight members, solved once, shared by the tests that only apply"""
    prs = members()
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols] == ["Solved"] * len(prs)
    return prs, b, sols


# ---- 1. the device tangents against the unscaled numpy restatement -------------------------------------------------
@pytest.mark.parametrize("only_dq", [True, False], ids=["dq_only", "dq_db_dP_dA"])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_tangents_match_reference(solved, form, only_dq):
    prs, b, sols = solved
    d = directions(prs, 5, only_dq)
    if form == "dev":
        import torch
        tan = b.jvp(*[None if v is None else torch.tensor(v, dtype=torch.float64, device="cuda") for v in d])
        assert all(hasattr(v, "is_cuda") and v.is_cuda for v in (tan.dx, tan.dz, tan.ds))
    else:
        tan = b.jvp(*d)
    assert list(tan.valid) == [1] * len(prs)
    worst = worst_against_ref(prs, sols, tan, d)
    print("tangents vs tangent_ref (%s, %s): worst %.3e" % (form, "dq" if only_dq else "dq db dP dA", worst))
    assert worst <= TAN_BOUND, worst


# ---- 2. duality with backward on the device ------------------------------------------------------------------------
def test_jvp_is_the_transpose_of_backward(hipdev):
    prs = members()
    b = batch(hipdev, prs)
    sols = b.solve()
    g = [np.concatenate([R.incoming(pr, 7 + 17 * k)[i] for k, pr in enumerate(prs)]) for i in range(3)]
    d = directions(prs, 23)
    grad = b.backward(*g)
    tan = b.jvp(*d)
    gs_ = [split(prs, v, key) for v, key in zip(g, ("q", "b", "b"))]
    ds_ = [split(prs, v, key) for v, key in zip(d, KEYS)]
    worst = 0.0
    for k, pr in enumerate(prs):
        dx, dz, ds = tan.per_member(k)
        lhs = float(gs_[0][k] @ dx + gs_[1][k] @ dz + gs_[2][k] @ ds)
        rhs = float(sum(a @ c[k] for a, c in zip(grad.per_member(k), ds_)))
        gap = abs(lhs - rhs) / max(1.0, abs(lhs))
        _, A = R.dense(pr)
        _, dA = T.direction_matrices(pr, None, ds_[3][k])
        nn = T.nn_rows(pr)
        want = (ds_[1][k] - dA @ sols[k].x)[nn]
        res = R.rel((A @ dx + ds)[nn], want)
        assert np.all(ds[~nn] == 0.0) and not np.any(np.signbit(ds[~nn])), k
        print("member %d: duality %.3e, A dx + ds = db - dA x on Nonnegative rows %.3e" % (k, gap, res))
        worst = max(worst, gap, res)
    print("duality on the device: worst %.3e" % worst)
    assert worst <= DUAL_BOUND, worst


# ---- 3. central differences through update + re-solve --------------------------------------------------------------
def test_tangent_against_central_differences(hipdev):
    prs = members()
    kidx = 4  # random_qp_1
    pr = prs[kidx]
    assert pr["n"] == 8 and pr["m"] == 14
    b = batch(hipdev, prs)
    b.solve()
    d = T.direction(pr, 3)
    lst = lambda v: [v if k == kidx else None for k in range(len(prs))]  # noqa: E731
    tan = b.jvp(*[lst(v) for v in d])
    others = [np.max(np.abs(v), initial=0.0) for k in range(len(prs)) if k != kidx for v in tan.per_member(k)]
    assert max(others) == 0.0  # members without a direction: independent problems, zero tangents
    base = dict(q=np.array(pr["q"], float), b=np.array(pr["b"], float), P=np.array(pr["P"][2], float),
                A=np.array(pr["A"][2], float))
    h = 1e-4
    side = []
    for sgn in (1.0, -1.0):
        b.update(**{key: lst(base[key] + sgn * h * v) for key, v in zip(KEYS, d)})
        sol = b.solve()[kidx]
        assert sol.status == "Solved"
        side.append(sol)
    worst = 0.0
    for name, got in zip(("x", "z", "s"), tan.per_member(kidx)):
        fd = (getattr(side[0], name) - getattr(side[1], name)) / (2 * h)
        err = R.rel(got, fd)
        print("d%s vs central differences through update + re-solve: %.3e" % (name, err))
        worst = max(worst, err)
    assert worst <= FD_BOUND, worst


# ---- 4. members without a derivative -------------------------------------------------------------------------------
def hetero():
    prs = members()
    extra = [E.basic_socp(), dict(primal_infeasible())["pinf_lp"], dict(dual_infeasible())["dinf_lp"]]
    return prs + extra, [1] * len(prs) + [0] * len(extra)


def test_members_without_a_derivative(hipdev):
    prs, want_valid = hetero()
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols[-3:]] == ["Solved", "PrimalInfeasible", "DualInfeasible"]
    d = directions(prs, 21)
    nval = sum(want_valid)
    for v, key in zip(d, KEYS):  # NaN in the parts of the members without a derivative, in all four inputs
        v[sum(length(pr, key) for pr in prs[:nval]):] = np.nan
    tan = b.jvp(*d)
    assert list(tan.valid) == want_valid
    for v in (tan.dx, tan.dz, tan.ds):
        assert np.all(np.isfinite(v))
    for k, v in enumerate(want_valid):
        if not v:
            for piece in tan.per_member(k):
                assert np.all(piece == 0.0) and not np.any(np.signbit(piece)), k
    worst = worst_against_ref(prs, sols, tan, d, only=set(range(nval)))
    print("heterogeneous batch, valid members vs tangent_ref: worst %.3e" % worst)
    assert worst <= TAN_BOUND, worst


# ---- 5. input forms and refusals -----------------------------------------------------------------------------------
def test_list_form_refusals_and_no_inputs(hipdev, solved):
    prs, b, sols = solved
    d = directions(prs, 9)
    pieces = [split(prs, v, key) for v, key in zip(d, KEYS)]
    pieces[1][2] = None  # a member without a db: zeros
    d2 = [v.copy() for v in d]
    off = np.concatenate([[0], np.cumsum([pr["m"] for pr in prs])])
    d2[1][off[2]:off[3]] = 0.0
    tan = b.jvp(dq=pieces[0], db=pieces[1], dP=pieces[2], dA=pieces[3])
    stacked = b.jvp(*d2)
    worst = worst_against_ref(prs, sols, tan, d2)
    print("list form vs tangent_ref: worst %.3e" % worst)
    assert worst <= TAN_BOUND, worst
    for a, c in zip((tan.dx, tan.dz, tan.ds), (stacked.dx, stacked.dz, stacked.ds)):
        assert R.rel(a, c) <= REPEAT_CEILING
    for bad in (dict(dq=pieces[0][:-1]), dict(dq=d[0][:-1]), dict(dP=d[2][:-1]), dict(dA=np.concatenate([d[3], [1.0]])),
                dict(db=d[0])):
        with pytest.raises(hipdev.ChipError) as e:
            b.jvp(**bad)
        assert e.value.code == hipdev.ERR_DIM
    import torch
    with pytest.raises(TypeError):  # host and device inputs do not mix
        b.jvp(dq=d[0], db=torch.tensor(d[1], dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        b.jvp(dq=torch.tensor(d[0], dtype=torch.float32, device="cuda"))
    zero = b.jvp()
    assert list(zero.valid) == [1] * len(prs)
    for v in (zero.dx, zero.dz, zero.ds):  # (a valid member's zero is the solve's: it may carry a sign)
        assert np.all(v == 0.0)


def test_device_inputs_that_are_not_16_byte_aligned(solved):
    import torch
    prs, b, sols = solved
    d = directions(prs, 13)
    for shifted in ((False, False, False, True), (True, True, True, True)):
        args = []
        for v, sh in zip(d, shifted):
            t = torch.tensor(np.concatenate([[0.0] * (3 if sh else 2), v]), dtype=torch.float64, device="cuda")
            t = t[3:] if sh else t[2:]
            assert t.is_contiguous() and (t.data_ptr() % 16 == 8) == sh
            args.append(t)
        tan = b.jvp(*args)
        worst = worst_against_ref(prs, sols, tan, d)
        print("device inputs at 8-byte alignment %s: worst %.3e" % (shifted, worst))
        assert worst <= TAN_BOUND, worst


# ---- 6. the handle's state around an apply -------------------------------------------------------------------------
def test_jvp_needs_a_solve_on_the_current_data(hipdev):
    prs = members()[:3]
    b = batch(hipdev, prs)
    d = directions(prs, 1)
    L = hipdev.lib()
    with pytest.raises(hipdev.ChipError) as e:  # before the first solve
        b.jvp(*d)
    assert e.value.code == hipdev.ERR_ARG
    assert L.chip_bjvp_get(b._h, None, None, None, None) == hipdev.ERR_ARG
    sols = b.solve()
    assert L.chip_bjvp_get(b._h, None, None, None, None) == hipdev.ERR_ARG  # solved, no apply yet
    first = b.jvp(*d)
    assert worst_against_ref(prs, sols, first, d) <= TAN_BOUND
    keep = np.zeros(b.stack["n"])
    assert L.chip_bjvp_get(b._h, keep.ctypes.data_as(hipdev.P_F64), None, None, None) == 0
    b.update(q=[np.array(prs[0]["q"]) * 1.5, None, None])
    with pytest.raises(hipdev.ChipError) as e:  # the data changed and was not solved
        b.jvp(*d)
    assert e.value.code == hipdev.ERR_ARG
    again = np.zeros(b.stack["n"])  # ... and the refusal changed nothing: the last apply's result is still there
    assert L.chip_bjvp_get(b._h, again.ctypes.data_as(hipdev.P_F64), None, None, None) == 0
    assert np.array_equal(keep, again) and np.array_equal(keep, first.dx)
    prs2 = [dict(prs[0], q=list(np.array(prs[0]["q"]) * 1.5))] + prs[1:]
    sols = b.solve()
    assert L.chip_bjvp_get(b._h, None, None, None, None) == hipdev.ERR_ARG  # a new solve: no apply yet
    assert worst_against_ref(prs2, sols, b.jvp(*d), d) <= TAN_BOUND


def test_solve_after_jvp_equals_solve_without(hipdev):
    prs, _ = hetero()
    a, c = batch(hipdev, prs), batch(hipdev, prs)
    a.solve()
    c.solve()
    a.jvp(*directions(prs, 2))
    sa, sc = a.solve(), c.solve()
    assert [s.status for s in sa] == [s.status for s in sc]
    assert [s.iterations for s in sa] == [s.iterations for s in sc]
    for u, v in zip(sa[:8], sc[:8]):
        assert R.rel(u.x, v.x) <= 1e-7 and R.rel(u.z, v.z) <= 1e-6


def test_jvp_backward_jvp_and_the_reuse_of_the_factorisation(hipdev):
    prs = members()
    a, c = batch(hipdev, prs), batch(hipdev, prs)
    g = [np.concatenate([R.incoming(pr, 4 + 17 * k)[i] for k, pr in enumerate(prs)]) for i in range(3)]
    d = directions(prs, 6)
    L = hipdev.lib()
    # ---- handle a: the refactors applies pay.  Two applies of one solve: one; the next solve's first apply: one more
    sols = a.solve()
    assert a.debug_counter("jvp_refactors") == 0.0
    t1 = a.jvp(*d)
    first = (a.debug_counter("jvp_launches"), a.debug_counter("jvp_host_syncs"))
    t2 = a.jvp(*d)
    reuse = (a.debug_counter("jvp_launches"), a.debug_counter("jvp_host_syncs"))
    assert a.debug_counter("jvp_refactors") == 1.0
    print("apply (launches, host syncs): first %s, reusing the factorisation %s" % (first, reuse))
    # (the reusing apply saves the scaling update and the refactor with its synchronisation; left: the KKT solve's
    # and the final one)
    assert reuse[0] == first[0] - 2 and reuse[1] == first[1] - 1 == 2.0
    assert max(worst_against_ref(prs, sols, t, d) for t in (t1, t2)) <= TAN_BOUND
    sols = a.solve()
    t3 = a.jvp(*d)
    assert a.debug_counter("jvp_refactors") == 2.0
    assert worst_against_ref(prs, sols, t3, d) <= TAN_BOUND
    # ---- handle c, ONE solve: a backward alone (the handle has never run an apply), then jvp, backward, jvp
    sols = c.solve()
    alone = c.backward(*g)
    t1 = c.jvp(*d)
    assert c.debug_counter("jvp_refactors") == 0.0  # (the apply found K factored by the backward)
    dq = np.zeros(c.stack["n"])  # the apply left backward's buffers alone
    assert L.chip_bgrad_get(c._h, dq.ctypes.data_as(hipdev.P_F64), None, None, None, None) == 0
    assert np.array_equal(dq, alone.dq)
    grad = c.backward(*g)
    dx = np.zeros(c.stack["n"])  # ... and the backward the apply's
    assert L.chip_bjvp_get(c._h, dx.ctypes.data_as(hipdev.P_F64), None, None, None) == 0
    assert np.array_equal(dx, t1.dx)
    t2 = c.jvp(*d)
    worst = max(R.rel(x, y) for x, y in zip((grad.dq, grad.db, grad.dP, grad.dA),
                                            (alone.dq, alone.db, alone.dP, alone.dA)))
    print("backward between two applies vs backward alone: worst %.3e" % worst)
    assert worst <= REPEAT_BOUND, worst
    again = max(R.rel(x, y) for x, y in zip((t2.dx, t2.dz, t2.ds), (t1.dx, t1.dz, t1.ds)))
    print("second apply vs first: worst %.3e" % again)
    assert again <= REPEAT_CEILING, again
    assert worst_against_ref(prs, sols, t2, d) <= TAN_BOUND


# ---- 7. launches and host synchronisations do not depend on the number of members ----------------------------------
def test_jvp_cost_does_not_depend_on_nprob(hipdev):
    import torch
    counts = {}
    for reps in (2, 256):
        prs = [R.random_qp(1)] * reps
        b = batch(hipdev, prs)
        sols = b.solve()
        assert all(s.status == "Solved" for s in sols)
        d = directions(prs, 6)
        tan = b.jvp(*d)
        host = (b.debug_counter("jvp_launches"), b.debug_counter("jvp_host_syncs"))
        if reps == 2:
            assert worst_against_ref(prs, sols, tan, d) <= TAN_BOUND
        b.jvp(*[torch.tensor(v, dtype=torch.float64, device="cuda") for v in d])
        dev = (b.debug_counter("jvp_launches"), b.debug_counter("jvp_host_syncs"))
        counts[reps] = (host, dev)
    print("jvp (launches, host syncs), first host form / reusing device form:", counts)
    assert counts[2] == counts[256]
    assert counts[2][0][1] == 3.0 and counts[2][1][1] == 2.0


# ---- 8. the right-hand side pass alone, on rows of every length class ----------------------------------------------
ROW_LENGTHS = [1, 32, 33, 64, 65, 4097, 16384, 16385]  # 32 | 33: lane / wavefront; 16384 | 16385: wavefront / workgroup


def long_row_members():
    """member 0: n = 16 500, P = a diagonal plus a dense first row (its symmetric row 0 has 16 500 entries), A with
    Nonnegative rows of ROW_LENGTHS entries; member 1: n = 3, 16 500 Nonnegative rows, A's columns hold 16 500, 33 and
    1 entries, column 2 of P is empty"""
    r = np.random.default_rng(12)
    n0 = 16500
    colptr = np.concatenate([[0, 1], 1 + 2 * np.arange(1, n0)]).astype(np.int64)  # column j > 0: (0, j) and (j, j)
    rowval = np.zeros(2 * n0 - 1, dtype=np.int64)
    rowval[2::2] = np.arange(1, n0)
    nzval = 0.01 * r.standard_normal(2 * n0 - 1)
    nzval[0] = 5.0
    nzval[2::2] = 1.0 + r.random(n0 - 1)
    A0 = np.zeros((len(ROW_LENGTHS), n0))
    for i, ln in enumerate(ROW_LENGTHS):
        A0[i, r.choice(n0, size=ln, replace=False)] = r.standard_normal(ln)
    m0 = dict(n=n0, m=len(ROW_LENGTHS), P=(colptr, rowval, nzval), A=E._csc(A0), q=list(r.standard_normal(n0)),
              b=list(r.standard_normal(len(ROW_LENGTHS))), cones=[(T.NN, len(ROW_LENGTHS))])
    m1n = 16500
    A1 = np.zeros((m1n, 3))
    A1[:, 0] = r.standard_normal(m1n)
    A1[r.choice(m1n, size=33, replace=False), 1] = r.standard_normal(33)
    A1[77, 2] = 1.5
    P1 = (np.array([0, 1, 2, 2], dtype=np.int64), np.array([0, 1], dtype=np.int64), np.array([2.0, 3.0]))
    m1 = dict(n=3, m=m1n, P=P1, A=E._csc(A1), q=[1.0, -1.0, 0.5], b=list(1.0 + r.random(m1n)), cones=[(T.NN, m1n)])
    return [m0, m1]


def rhs_reference(prs, scales, x, z, valid, d):
    """per entry: math.fsum of the row's terms times the scale, and the rounding bound of any summation order,
    (L + 4) 2^-53 |scale| sum |terms| with L the row's term count"""
    ref_x, bnd_x, ref_z, bnd_z = [], [], [], []
    xs, zs = split(prs, x, "q"), split(prs, z, "b")
    pieces = [split(prs, v, key) for v, key in zip(d, KEYS)]
    u = 2.0 ** -53
    for k, pr in enumerate(prs):
        dd, ee, cc = scales[k]
        n, m = pr["n"], pr["m"]
        if not valid[k]:
            for lst, ln in ((ref_x, n), (bnd_x, n), (ref_z, m), (bnd_z, m)):
                lst.append(np.zeros(ln))
            continue
        dq, db, dP, dA = [p[k] for p in pieces]
        tx = [[] if dq is None else [dq[j]] for j in range(n)]
        tz = [[] if db is None else [db[i]] for i in range(m)]
        if dP is not None:
            cp, ri = pr["P"][0], pr["P"][1]
            for col in range(n):
                for p in range(cp[col], cp[col + 1]):
                    row = ri[p]
                    tx[row].append(dP[p] * xs[k][col])
                    if row != col:
                        tx[col].append(dP[p] * xs[k][row])
        if dA is not None:
            cp, ri = pr["A"][0], pr["A"][1]
            for col in range(n):
                for p in range(cp[col], cp[col + 1]):
                    row = ri[p]
                    tx[col].append(dA[p] * zs[k][row])
                    tz[row].append(-(dA[p] * xs[k][col]))
        sx = cc * dd
        ref_x.append(np.array([sx[j] * -math.fsum(tx[j]) for j in range(n)]))
        bnd_x.append(np.array([(len(tx[j]) + 4) * u * abs(sx[j]) * math.fsum(abs(t) for t in tx[j]) for j in range(n)]))
        ref_z.append(np.array([ee[i] * math.fsum(tz[i]) for i in range(m)]))
        bnd_z.append(np.array([(len(tz[i]) + 4) * u * abs(ee[i]) * math.fsum(abs(t) for t in tz[i]) for i in range(m)]))
    return np.concatenate(ref_x), np.concatenate(bnd_x), np.concatenate(ref_z), np.concatenate(bnd_z)


def test_rhs_pass_on_rows_of_every_length(hipdev):
    """chip_debug_batch_jvp_rhs on a created handle (no solve): thread, wavefront and workgroup rows in both spaces"""
    prs = long_row_members()
    b = batch(hipdev, prs)
    scales = [b.equilibration(k) for k in range(2)]
    r = np.random.default_rng(5)
    n, m = b.stack["n"], b.stack["m"]
    x, z = r.standard_normal(n), r.standard_normal(m)
    d = [r.standard_normal(b._len[key]) for key in KEYS]
    assert int(np.sum(prs[0]["P"][1] == 0)) == 16500  # the symmetric row 0 of member 0's P
    assert sorted(np.bincount(prs[0]["A"][1], minlength=len(ROW_LENGTHS))) == ROW_LENGTHS
    assert list(np.diff(prs[1]["A"][0])) == [16500, 33, 1] and list(np.diff(prs[1]["P"][0])) == [1, 1, 0]
    # both members valid
    rx, rz = b.debug_jvp_rhs(x, z, [1, 1], *d)
    wx, bx, wz, bz = rhs_reference(prs, scales, x, z, [1, 1], d)
    ex, ez = np.abs(rx - wx), np.abs(rz - wz)
    print("rhs pass: worst error / bound %.3f (x space), %.3f (z space)"
          % (float(np.max(ex / np.maximum(bx, 1e-300))), float(np.max(ez / np.maximum(bz, 1e-300)))))
    assert np.all(ex <= bx) and np.all(ez <= bz)
    again = b.debug_jvp_rhs(x, z, [1, 1], *d)
    assert np.array_equal(again[0], rx) and np.array_equal(again[1], rz)  # bit for bit
    # without dP and dA every row is empty and still receives its dq / db term
    rx0, rz0 = b.debug_jvp_rhs(x, z, [1, 1], d[0], d[1], None, None)
    wx0, bx0, wz0, bz0 = rhs_reference(prs, scales, x, z, [1, 1], [d[0], d[1], None, None])
    assert np.all(np.abs(rx0 - wx0) <= bx0) and np.all(np.abs(rz0 - wz0) <= bz0)
    assert np.all(rx0 != 0.0) and np.all(rz0 != 0.0)
    # member 1 invalid, NaN in everything of it that could be read
    xn, zn, dn = x.copy(), z.copy(), [v.copy() for v in d]
    xn[prs[0]["n"]:] = np.nan
    zn[prs[0]["m"]:] = np.nan
    for v, key in zip(dn, KEYS):
        v[length(prs[0], key):] = np.nan
    rx1, rz1 = b.debug_jvp_rhs(xn, zn, [1, 0], *dn)
    n0, m0 = prs[0]["n"], prs[0]["m"]
    assert np.array_equal(rx1[:n0], rx[:n0]) and np.array_equal(rz1[:m0], rz[:m0])
    for v in (rx1[n0:], rz1[m0:]):
        assert np.all(v == 0.0) and not np.any(np.signbit(v))


# ---- 9. the torch layer --------------------------------------------------------------------------------------------
def test_layer_forward_mode_and_backward(hipdev):
    import torch
    import torch.autograd.forward_ad as fwAD
    from clarabel_rs_amd.layer import BatchQPFunction
    prs = members()
    b = batch(hipdev, prs)
    st = b.stack
    dev = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device="cuda")  # noqa: E731
    vals = [dev(st["q"] * 1.01), dev(st["b"]), dev(st["P"][2]), dev(st["A"][2])]
    d = directions(prs, 8)
    with fwAD.dual_level():
        duals = [fwAD.make_dual(v, dev(t)) for v, t in zip(vals, d)]
        out = BatchQPFunction.apply(*duals, b)
        tangents = [fwAD.unpack_dual(o).tangent for o in out]
    assert all(t is not None and t.is_cuda for t in tangents)
    direct = b.jvp(*[dev(t) for t in d])
    worst = max(R.rel(to_host(t), to_host(w)) for t, w in zip(tangents, (direct.dx, direct.dz, direct.ds)))
    print("layer tangents vs jvp(): worst %.3e" % worst)
    assert worst <= REPEAT_CEILING, worst
    # the tangents are those of the perturbed q the layer was given
    prs2 = [dict(pr, q=list(np.array(pr["q"], dtype=float) * 1.01)) for pr in prs]
    sols = b.solve()
    assert worst_against_ref(prs2, sols, b.jvp(*d), d) <= TAN_BOUND
    # only q dual: the other tangents are None / zeros
    with fwAD.dual_level():
        out = BatchQPFunction.apply(fwAD.make_dual(vals[0], dev(d[0])), None, None, None, b)
        tx = fwAD.unpack_dual(out[0]).tangent
    assert R.rel(to_host(tx), to_host(b.jvp(dq=d[0]).dx)) <= REPEAT_CEILING
    # .backward() of the same layer still fills the gradients
    req = [v.clone().requires_grad_(True) for v in vals]
    x, z, s = BatchQPFunction.apply(*req, b)
    w = [dev(np.concatenate([R.incoming(pr, 8 + 17 * k)[i] for k, pr in enumerate(prs)])) for i in range(3)]
    ((w[0] * x).sum() + (w[1] * z).sum() + (w[2] * s).sum()).backward()
    want = b.backward(*w)
    worst = 0.0
    for got, ref in zip(req, (want.dq, want.db, want.dP, want.dA)):
        assert got.grad is not None and got.grad.is_cuda and got.grad.shape == ref.shape
        worst = max(worst, R.rel(to_host(got.grad), to_host(ref)))
    print("layer gradients vs backward(): worst %.3e" % worst)
    assert worst <= REPEAT_BOUND, worst
