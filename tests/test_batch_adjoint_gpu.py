"""The batched solver's gradients (chip_bgrad_*, HipBatchSolver.backward, layer.BatchQPFunction) on the MI355X: the
device gradients against the numpy restatement of tests/adjoint_ref.py evaluated at the device's own solution, against
finite differences through update + re-solve, a heterogeneous batch with members that have no gradient, order
independence, refusals, a solve after a backward, launch counts that do not grow with the batch, and the torch layer.

GRAD_BOUND and FD_BOUND are ten times the worst figure measured on the MI355X over the members below, and never looser
than 1e-6 (device against restatement: the agreement of the restatement with finite differences on the CPU; anything
worse is an error, not rounding) and 1e-4 (finite differences: the CPU bound of tests/test_batch_adjoint_host.py).
Measured on the first run of this file (one MI355X):
  device against adjoint_ref at the device's own (x, s, z), seven members: host form 3.7e-14 (gx only) and 8.0e-14
  (gx, gz, gs), device form 3.7e-14 and 7.8e-14; the heterogeneous batch's valid members 5.1e-14   -> MEASURED_GRAD
  dq / db of random_qp_1 against central differences (h = 1e-4) through update + re-solve: 3.8e-9 / 2.0e-9 -> MEASURED_FD
  the permuted batch against the batch in order, gradient by gradient: 9.8e-13 (two different solves, see test 3)
                                                                                                -> MEASURED_PERM
  two backwards of ONE solve, the layer's gradients against backward(): 1.0e-15                     -> MEASURED_REPEAT
  (the other comparison of two backwards of one solve, with and without NaN in the incoming gradients of the members
  without a gradient, has no measured figure of its own yet: it prints it, and is held to 2 x GRAD_BOUND, which is
  what two results within GRAD_BOUND of one reference can differ by)
(`profiles/l4_batch_adjoint_scale_*.json` hold the same comparison at scale.)"""
import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import e2e_problems as E
from tests.test_batch_gpu import dual_infeasible, member, primal_infeasible

pytestmark = pytest.mark.gpu

# worst relative difference device / adjoint_ref over the seven members, both forms, both input sets: MEASURED_GRAD
MEASURED_GRAD = 8.004e-14
GRAD_BOUND = 1e-6 if MEASURED_GRAD is None else min(1e-6, 10.0 * MEASURED_GRAD)
# worst relative difference of dq, db against central differences (h = 1e-4) through update + re-solve: MEASURED_FD
MEASURED_FD = 3.802e-9
FD_BOUND = 1e-4 if MEASURED_FD is None else min(1e-4, 10.0 * MEASURED_FD)
# worst relative difference, gradient by gradient, between a batch and the same members in another order (two solves)
MEASURED_PERM = 9.849e-13
PERM_BOUND = min(1e-6, 10.0 * MEASURED_PERM)
# worst relative difference between two backwards of one solve of one handle (the factorisation's atomic adds)
MEASURED_REPEAT = 1.021e-15
REPEAT_BOUND = 1e-6 if MEASURED_REPEAT is None else min(1e-6, 10.0 * MEASURED_REPEAT)


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def batch(hip, prs, **kw):
    return hip.HipBatchSolver([member(hip, p) for p in prs], hip.SolverSettings.default(**kw))


def incoming(prs, seed, only_gx=False):
    gs_ = [R.incoming(pr, seed + 17 * k) for k, pr in enumerate(prs)]
    gx = np.concatenate([g[0] for g in gs_])
    if only_gx:
        return gx, None, None
    return gx, np.concatenate([g[1] for g in gs_]), np.concatenate([g[2] for g in gs_])


def split(prs, v, key):
    if v is None:
        return [None] * len(prs)
    off = np.concatenate([[0], np.cumsum([pr[key] for pr in prs])])
    return [v[off[k]:off[k + 1]] for k in range(len(prs))]


def to_host(v):
    return v.detach().cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def worst_against_ref(prs, sols, grad, gx, gz, gs, members=None):
    """the worst relative difference of the members' four gradients against adjoint_ref at the device's own solution"""
    gxs, gzs, gss = split(prs, gx, "n"), split(prs, gz, "m"), split(prs, gs, "m")
    worst = 0.0
    for k, pr in enumerate(prs):
        if members is not None and k not in members:
            continue
        want = R.adjoint(pr, sols[k].x, sols[k].s, sols[k].z, gxs[k], gzs[k], gss[k])
        got = [to_host(v) for v in grad.per_member(k)]
        for w, g in zip(want, got):
            worst = max(worst, R.rel(g, w))
    return worst


def valid_members():
    return [pr for _, pr in R.gpu_members()]


# ---- 1. the device gradients against the unscaled numpy restatement ------------------------------------------------
@pytest.mark.parametrize("only_gx", [True, False], ids=["gx_only", "gx_gz_gs"])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_gradients_match_reference(hipdev, form, only_gx):
    prs = valid_members()
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols] == ["Solved"] * len(prs)
    gx, gz, gs = incoming(prs, 5, only_gx)
    if form == "dev":
        import torch
        args = [None if g is None else torch.tensor(g, dtype=torch.float64, device="cuda") for g in (gx, gz, gs)]
        grad = b.backward(*args)
        assert all(hasattr(v, "is_cuda") and v.is_cuda for v in (grad.dq, grad.db, grad.dP, grad.dA))
    else:
        grad = b.backward(gx, gz, gs)
    assert list(grad.valid) == [1] * len(prs)
    worst = worst_against_ref(prs, sols, grad, gx, gz, gs)
    print("gradients vs adjoint_ref (%s, %s): worst %.3e" % (form, "gx" if only_gx else "gx gz gs", worst))
    assert worst <= GRAD_BOUND, worst


def test_list_form_equals_stacked_form(hipdev):
    prs = valid_members()
    b = batch(hipdev, prs)
    sols = b.solve()
    gx, gz, gs = incoming(prs, 9)
    pieces = [split(prs, gx, "n"), split(prs, gz, "m"), split(prs, gs, "m")]
    pieces[1][2] = None  # a member without an incoming gz: zeros
    gz2 = gz.copy()
    off = np.concatenate([[0], np.cumsum([pr["m"] for pr in prs])])
    gz2[off[2]:off[3]] = 0.0
    grad = b.backward(gx=pieces[0], gz=pieces[1], gs=pieces[2])
    assert worst_against_ref(prs, sols, grad, gx, gz2, gs) <= GRAD_BOUND
    with pytest.raises(hipdev.ChipError) as e:
        b.backward(gx=pieces[0][:-1])
    assert e.value.code == hipdev.ERR_DIM
    with pytest.raises(hipdev.ChipError) as e:
        b.backward(gx=gx[:-1])
    assert e.value.code == hipdev.ERR_DIM


def test_device_inputs_that_are_not_16_byte_aligned(hipdev):
    """gs (and gx, gz) as slices at an odd offset of longer tensors: 8-byte aligned only, so the vector pass takes its
    one-entry-per-lane form (k_ba_grad_vec<false>); the result is held to the same bound"""
    import torch
    prs = valid_members()
    b = batch(hipdev, prs)
    sols = b.solve()
    gx, gz, gs = incoming(prs, 13)
    for shifted in ((False, False, True), (True, True, True)):
        args = []
        for g, sh in zip((gx, gz, gs), shifted):
            t = torch.tensor(np.concatenate([[0.0] * (3 if sh else 2), g]), dtype=torch.float64, device="cuda")
            t = t[3:] if sh else t[2:]
            assert t.is_contiguous() and (t.data_ptr() % 16 == 8) == sh
            args.append(t)
        grad = b.backward(*args)
        worst = worst_against_ref(prs, sols, grad, gx, gz, gs)
        print("device inputs at 8-byte alignment %s: worst %.3e" % (shifted, worst))
        assert worst <= GRAD_BOUND, worst


# ---- 2. finite differences through update + re-solve ---------------------------------------------------------------
def test_dq_db_against_finite_differences(hipdev):
    prs = valid_members()
    kidx = 4  # random_qp_1
    pr = prs[kidx]
    assert pr["n"] == 8 and pr["m"] == 14
    b = batch(hipdev, prs)
    b.solve()
    gx, gz, gs = R.incoming(pr, 3)
    lst = lambda g: [g if k == kidx else None for k in range(len(prs))]  # noqa: E731
    grad = b.backward(gx=lst(gx), gz=lst(gz), gs=lst(gs))
    dq, db, _, _ = grad.per_member(kidx)
    others = [np.max(np.abs(v), initial=0.0) for k in range(len(prs)) if k != kidx for v in grad.per_member(k)]
    assert max(others) == 0.0  # members without an incoming gradient: independent problems, zero gradients
    h = 1e-4
    worst = 0.0
    for key, got in (("q", dq), ("b", db)):
        off = int(b._offsets[key][kidx])
        v0 = np.array(pr[key], dtype=float)
        fd = np.zeros(len(v0))
        for i in range(len(v0)):
            vals = []
            for sgn in (1.0, -1.0):
                b.update(**{key: (np.array([off + i]), np.array([v0[i] + sgn * h]))})
                sol = b.solve()[kidx]
                assert sol.status == "Solved"
                vals.append(float(gx @ sol.x + gz @ sol.z + gs @ sol.s))
            b.update(**{key: (np.array([off + i]), np.array([v0[i]]))})
            fd[i] = (vals[0] - vals[1]) / (2 * h)
        err = R.rel(got, fd)
        print("d%s vs finite differences through update + re-solve: %.3e" % (key, err))
        worst = max(worst, err)
    assert worst <= FD_BOUND, worst


# ---- 3. members without a gradient; order independence -------------------------------------------------------------
def hetero():
    prs = valid_members()
    extra = [E.basic_socp(), dict(primal_infeasible())["pinf_lp"], dict(dual_infeasible())["dinf_lp"]]
    return prs + extra, [1] * len(prs) + [0] * len(extra)


def test_members_without_a_gradient_and_order_independence(hipdev):
    """The permuted batch is a solve of its own: the stack-wide regularisers, the refinement stop and the order of the
    factorisation's atomic adds change with the order of the members, so its final iterates differ from the ordered
    batch's in their last digits.  Its gradients are held to GRAD_BOUND against adjoint_ref at ITS OWN solution, and
    the direct difference between the two batches, gradient by gradient, to a fixed number of its own, set by the
    same protocol as GRAD_BOUND: ten times the figure measured on the MI355X (9.8e-13), never looser than 1e-6."""
    prs, want_valid = hetero()
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols[-3:]] == ["Solved", "PrimalInfeasible", "DualInfeasible"]
    gx, gz, gs = incoming(prs, 21)  # the members without a gradient get incoming values too: they are ignored
    grad = b.backward(gx, gz, gs)
    assert list(grad.valid) == want_valid
    for k, v in enumerate(want_valid):
        if not v:
            for piece in grad.per_member(k):
                assert np.all(piece == 0.0) and not np.any(np.signbit(piece)), k
    nval = sum(want_valid)
    worst = worst_against_ref(prs, sols, grad, gx, gz, gs, members=set(range(nval)))
    print("heterogeneous batch, valid members vs adjoint_ref: worst %.3e" % worst)
    assert worst <= GRAD_BOUND, worst
    # a NaN in an incoming gradient (gx, gz or gs) of a member without a gradient reaches nobody: the second backward
    # of the same solve repeats the first
    gx_nan, gz_nan, gs_nan = gx.copy(), gz.copy(), gs.copy()
    gx_nan[sum(pr["n"] for pr in prs[:nval]):] = np.nan
    gz_nan[sum(pr["m"] for pr in prs[:nval]):] = np.nan
    gs_nan[sum(pr["m"] for pr in prs[:nval]):] = np.nan
    g2 = b.backward(gx_nan, gz_nan, gs_nan)
    repeat = 0.0
    for a, c in zip((g2.dq, g2.db, g2.dP, g2.dA), (grad.dq, grad.db, grad.dP, grad.dA)):
        assert np.all(np.isfinite(a))
        repeat = max(repeat, R.rel(a, c))
    print("backward with NaN for the members without a gradient vs without: worst %.3e" % repeat)
    assert repeat <= 2 * GRAD_BOUND, repeat  # (both are within GRAD_BOUND of one reference; no figure of its own yet)
    # any permutation of the members gives the permuted result
    perm = np.random.default_rng(4).permutation(len(prs))
    assert list(perm) != sorted(perm)
    prs_p = [prs[i] for i in perm]
    gxs, gzs, gss = split(prs, gx, "n"), split(prs, gz, "m"), split(prs, gs, "m")
    bp = batch(hipdev, prs_p)
    sols_p = bp.solve()
    cat = lambda parts: np.concatenate([parts[i] for i in perm])  # noqa: E731
    gp = bp.backward(cat(gxs), cat(gzs), cat(gss))
    assert list(gp.valid) == [want_valid[i] for i in perm]
    own = worst_against_ref(prs_p, sols_p, gp, cat(gxs), cat(gzs), cat(gss),
                            members={pos for pos, i in enumerate(perm) if want_valid[i]})
    print("permuted batch, valid members vs adjoint_ref at its own solution: worst %.3e" % own)
    assert own <= GRAD_BOUND, own
    for pos, i in enumerate(perm):
        got_p, got_o = gp.per_member(pos), grad.per_member(i)
        if not want_valid[i]:
            assert all(np.all(v == 0.0) for v in got_p)
            continue
        direct = max(R.rel(a, c) for a, c in zip(got_p, got_o))
        print("member %d (at %d): permuted vs ordered %.3e" % (i, pos, direct))
        assert direct <= PERM_BOUND, (i, direct)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------
def test_backward_needs_a_solve_on_the_current_data(hipdev):
    prs = valid_members()[:3]
    b = batch(hipdev, prs)
    gx, _, _ = incoming(prs, 1, only_gx=True)
    L = hipdev.lib()
    with pytest.raises(hipdev.ChipError) as e:  # before the first solve
        b.backward(gx)
    assert e.value.code == hipdev.ERR_ARG
    assert L.chip_bgrad_get(b._h, None, None, None, None, None) == hipdev.ERR_ARG
    sols = b.solve()
    assert L.chip_bgrad_get(b._h, None, None, None, None, None) == hipdev.ERR_ARG  # solved, no backward yet
    first = b.backward(gx)
    assert worst_against_ref(prs, sols, first, gx, None, None) <= GRAD_BOUND
    b.update(q=[np.array(prs[0]["q"]) * 1.5, None, None])
    with pytest.raises(hipdev.ChipError) as e:  # the data changed and was not solved
        b.backward(gx)
    assert e.value.code == hipdev.ERR_ARG
    with pytest.raises(hipdev.ChipError):  # a refused update (index out of range) changes nothing, this one neither
        b.update(q=(np.array([10 ** 6]), np.array([1.0])))
    with pytest.raises(hipdev.ChipError) as e:
        b.backward(gx)
    assert e.value.code == hipdev.ERR_ARG
    prs2 = [dict(prs[0], q=list(np.array(prs[0]["q"]) * 1.5))] + prs[1:]
    sols = b.solve()
    g = b.backward(gx)
    assert worst_against_ref(prs2, sols, g, gx, None, None) <= GRAD_BOUND
    with pytest.raises(hipdev.ChipError):  # a refused update after a solve changes nothing: backward still runs
        b.update(b=(np.array([10 ** 6]), np.array([1.0])))
    g = b.backward(gx)
    assert worst_against_ref(prs2, sols, g, gx, None, None) <= GRAD_BOUND


# ---- 5. a solve after a backward behaves as if backward had not been called ----------------------------------------
def test_solve_after_backward_equals_solve_without(hipdev):
    prs, _ = hetero()
    a, c = batch(hipdev, prs), batch(hipdev, prs)
    a.solve()
    c.solve()
    gx, gz, gs = incoming(prs, 2)
    a.backward(gx, gz, gs)
    sa, sc = a.solve(), c.solve()
    assert [s.status for s in sa] == [s.status for s in sc]
    assert [s.iterations for s in sa] == [s.iterations for s in sc]
    for u, v in zip(sa[:7], sc[:7]):
        assert R.rel(u.x, v.x) <= 1e-7 and R.rel(u.z, v.z) <= 1e-6


# ---- 6. launches and host synchronisations do not depend on the number of members ----------------------------------
def test_backward_cost_does_not_depend_on_nprob(hipdev):
    import torch
    pair = [R.random_qp(1), E.basic_lp()]
    counts = {}
    for reps in (1, 128):
        prs = pair * reps
        b = batch(hipdev, prs)
        sols = b.solve()
        assert all(s.status == "Solved" for s in sols)
        gx, gz, gs = incoming(prs, 6)
        grad = b.backward(gx, gz, gs)
        host = (b.debug_counter("backward_launches"), b.debug_counter("backward_host_syncs"))
        if reps == 1:
            assert worst_against_ref(prs, sols, grad, gx, gz, gs) <= GRAD_BOUND
        b.backward(*[torch.tensor(g, dtype=torch.float64, device="cuda") for g in (gx, gz, gs)])
        dev = (b.debug_counter("backward_launches"), b.debug_counter("backward_host_syncs"))
        counts[reps] = (host, dev)
    print("backward (launches, host syncs), host form / device form:", counts)
    assert counts[1] == counts[128]
    assert counts[1][0][1] == counts[1][1][1] == 3.0  # the KKT update's, the KKT solve's, and the final one


# ---- 7. the torch layer --------------------------------------------------------------------------------------------
def test_layer_backward_gives_the_gradients_of_backward(hipdev):
    import torch
    from clarabel_rs_amd.layer import BatchQPFunction
    prs = valid_members()
    b = batch(hipdev, prs)
    st = b.stack
    mk = lambda v: torch.tensor(np.asarray(v, dtype=float), dtype=torch.float64, device="cuda",  # noqa: E731
                                requires_grad=True)
    q, bb, Px, Ax = mk(st["q"] * 1.01), mk(st["b"]), mk(st["P"][2]), mk(st["A"][2])
    x, z, s = BatchQPFunction.apply(q, bb, Px, Ax, b)
    assert x.is_cuda and x.shape == (st["n"],) and z.shape == s.shape == (st["m"],)
    assert [i.status for i in b.infos()] == [1] * len(prs)
    wx, wz, ws = [torch.tensor(g, dtype=torch.float64, device="cuda") for g in incoming(prs, 8)]
    loss = (wx * x).sum() + (wz * z).sum() + (ws * s).sum()
    loss.backward()
    direct = b.backward(wx, wz, ws)
    worst = 0.0
    for got, want in ((q.grad, direct.dq), (bb.grad, direct.db), (Px.grad, direct.dP), (Ax.grad, direct.dA)):
        assert got is not None and got.is_cuda and got.shape == want.shape
        worst = max(worst, R.rel(to_host(got), to_host(want)))
    # (two backwards of one solve differ in the last bits: the factorisation accumulates with floating-point atomics)
    print("layer gradients vs backward(): worst %.3e" % worst)
    assert worst <= REPEAT_BOUND, worst
    # the layer's solution is the solver's, and its gradient is that of the perturbed q it was given
    prs2 = []
    off = np.concatenate([[0], np.cumsum([pr["n"] for pr in prs])])
    for k, pr in enumerate(prs):
        prs2.append(dict(pr, q=list(np.array(pr["q"], dtype=float) * 1.01)))
    sols = b.solve()
    assert R.rel(to_host(x), np.concatenate([s_.x for s_ in sols])) <= 1e-9
    assert off[-1] == st["n"]
    g = b.backward(*[to_host(w) for w in (wx, wz, ws)])
    assert worst_against_ref(prs2, sols, g, *[to_host(w) for w in (wx, wz, ws)]) <= GRAD_BOUND
    # only q given: the other pieces keep their values and get no gradient
    q2 = mk(st["q"])
    x2, _, _ = BatchQPFunction.apply(q2, None, None, None, b)
    x2.sum().backward()
    assert q2.grad is not None and float(q2.grad.abs().max()) > 0.0
    # a backward that no longer meets its own solve is refused
    q3 = mk(st["q"])
    x3, _, _ = BatchQPFunction.apply(q3, None, None, None, b)
    b.solve()
    with pytest.raises(RuntimeError):
        x3.sum().backward()
