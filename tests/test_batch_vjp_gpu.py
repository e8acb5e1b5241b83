"""The batched solver's blocks of cotangents and Jacobian rows (chip_bvjp_*, HipBatchSolver.backward_block /
member_jacobian_rows, layer.batch_vjp_block / batch_jacobian_rows) on the MI355X: the block's passes bit for bit
against the single passes of backward(), the unit right-hand sides against the explicit unit vectors, the block's
gradients against tests/adjoint_ref.py at the device's own solution and against backward() of the same cotangent, the
members' Jacobians row by row and against the columns of member_jacobians(), members without a derivative, the handle's
state around a block, and its cost in launches and host synchronisations.

A cotangent of a block is the computation of a single backward, so the bounds are those of
tests/test_batch_adjoint_gpu.py (GRAD_BOUND: ten times the worst figure measured there); a block against backward() of
the same cotangent is held to 2 GRAD_BOUND, both being within GRAD_BOUND of one reference, and a row of dx/dq or dx/db
against the transposed column of member_jacobians() to GRAD_BOUND + TAN_BOUND, each path being within its own bound
of the one matrix.

The launches of one block, read from the host code (one per kernel, copy or call into the KKT layer, as the batched
solver counts everywhere): valid flags (1), right-hand side (1), per cotangent one enqueued solve (ndir) and, only when
gs is given or the units are those of s, one A' product (ndir), one output launch for dq / db when either is wanted
(1) and one for dP / dA when either is wanted (1) = 2 + ndir (1 + [gs]) + [q or b] + [P or A], and 2 more (scaling
update, refactor) when K is not factored at the final iterates; the host form adds one copy per given input.  Host
synchronisations: the collect (1), the refactor's when it is paid, and one per repeat at the collect.

Measured on the first run of this file (one MI355X), none of them a bound of its own: a block's cotangents against
adjoint_ref 7.1e-14 at worst (the single backwards of the same cotangents, in the same test, 7.1e-14), against
backward() 6.0e-15; the Jacobians' rows 1.4e-14; the rows of dx/dq, dx/db against the transposed columns of
member_jacobians() 4.2e-15; the heterogeneous batch's valid members 5.8e-14; 8-byte aligned inputs against aligned
ones 4.1e-17."""
import ctypes as C

import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import e2e_problems as E
from tests import tangent_ref as T
from tests.test_batch_adjoint_gpu import GRAD_BOUND
from tests.test_batch_jvp_gpu import TAN_BOUND, batch, directions, hetero, members, to_host

pytestmark = pytest.mark.gpu

KEYS = ("q", "b", "P", "A")
IN_KEYS = ("q", "b", "b")  # the spaces of gx, gz, gs


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def length(pr, key):
    return {"q": pr["n"], "b": pr["m"], "P": len(pr["P"][2]), "A": len(pr["A"][2])}[key]


def block_cotangents(prs, K, seed, only_gx=False):
    """K random cotangents, row t of every piece = cotangent t: [gx [K, n], gz [K, m], gs [K, m]] (None where absent)"""
    per = [[R.incoming(pr, seed + 1000 * t + 17 * k) for k, pr in enumerate(prs)] for t in range(K)]
    out = [np.stack([np.concatenate([g[i] for g in row]) for row in per]) for i in range(3)]
    return [out[0], None, None] if only_gx else out


def on_device(vs):
    import torch
    return [None if v is None else torch.tensor(v, dtype=torch.float64, device="cuda") for v in vs]


def split(prs, v, key):
    if v is None:
        return [None] * len(prs)
    off = np.concatenate([[0], np.cumsum([length(pr, key) for pr in prs])]).astype(int)
    return [v[off[k]:off[k + 1]] for k in range(len(prs))]


def worst_against_ref(prs, sols, blk, t, g, only=None):
    """the worst relative difference of cotangent t's wanted gradients of the members against adjoint_ref at the
    device's own solution; g: the three inputs of cotangent t (None where absent)"""
    pieces = [split(prs, v, key) for v, key in zip(g, IN_KEYS)]
    worst = 0.0
    for k, pr in enumerate(prs):
        if only is not None and k not in only:
            continue
        want = R.adjoint(pr, sols[k].x, sols[k].s, sols[k].z, *[p[k] for p in pieces])
        for w, got in zip(want, blk.per_member(k)):
            if got is not None:
                worst = max(worst, R.rel(to_host(got[t]), w))
    return worst


@pytest.fixture(scope="module")
def solved(hipdev):
    """one batch of the seven members of the adjoint tests, solved once, shared by the tests that only apply"""
    prs = [pr for _, pr in R.gpu_members()]
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols] == ["Solved"] * len(prs)
    return prs, b, sols


# ---- 1. the block's passes are bit for bit the single passes -------------------------------------------------------
def hook_members(parity):
    """even: stacked n = 3 + 3 + 8 = 14 and m = 6 + 0 + 14 = 20, every cotangent's slice 16-byte aligned (two entries
    per lane); odd: with hs35 and wide_qp(1) n = 87 and m = 47, so every other slice is only 8-byte aligned (one entry
    per lane).  Either holds basic_lp (no stored P) and basic_unconstrained (no rows), and ends with random_qp(1), the
    member the test makes invalid"""
    prs = [E.basic_lp(), E.basic_unconstrained()]
    if parity == "odd":
        prs += [R.hs35(), T.wide_qp(1)]
    prs.append(R.random_qp(1))
    n, m = sum(pr["n"] for pr in prs), sum(pr["m"] for pr in prs)
    assert (n % 2, m % 2) == ((1, 1) if parity == "odd" else (0, 0))
    return prs, n, m


@pytest.fixture(scope="module", params=["odd", "even"])
def hook_batch(request, hipdev):
    prs, n, m = hook_members(request.param)
    b = batch(hipdev, prs)
    assert (n, m) == (b.stack["n"], b.stack["m"])
    assert len(prs[0]["P"][2]) == 0 and prs[1]["m"] == 0
    return request.param, prs, b


@pytest.mark.parametrize("with_gs", [True, False], ids=["gs", "no_gs"])
@pytest.mark.parametrize("ndir", [1, 3, 4, 5, 16])
def test_block_passes_are_bitwise_the_single_passes(hook_batch, ndir, with_gs):
    """form 1 (the block launchers once) against form 0 (the single launchers of backward() once per cotangent) on the
    same inputs: np.array_equal.  The last member is invalid and holds NaN in everything of it that could be read."""
    parity, prs, b = hook_batch
    n, m = b.stack["n"], b.stack["m"]
    assert (n % 2, m % 2) == ((1, 1) if parity == "odd" else (0, 0))
    r = np.random.default_rng(100 + ndir)
    valid = [1] * len(prs)
    valid[-1] = 0
    nl, ml = prs[-1]["n"], prs[-1]["m"]
    x, z, s = r.standard_normal(n), r.standard_normal(m), r.random(m) + 0.5
    gx, gz, gs = r.standard_normal((ndir, n)), r.standard_normal((ndir, m)), r.standard_normal((ndir, m))
    vx, vz = r.standard_normal((ndir, n)), r.standard_normal((ndir, m))
    for v in (x, gx, vx):
        v[..., n - nl:] = np.nan
    for v in (z, s, gz, gs, vz):
        v[..., m - ml:] = np.nan
    gs_in = gs if with_gs else None
    # the right-hand side pass
    one = b.debug_vjp_rhs(0, ndir, s, z, valid, gx, gz, gs_in)
    blk = b.debug_vjp_rhs(1, ndir, s, z, valid, gx, gz, gs_in)
    for u, v, dead in zip(blk, one, (nl, ml, ml)):
        assert np.array_equal(u, v)
        tail = u[:, u.shape[1] - dead:]
        assert np.all(tail == 0.0) and not np.any(np.signbit(tail))  # the invalid member: exact +0.0
        assert np.all(np.isfinite(u))
    assert np.count_nonzero(blk[0]) == ndir * (n - nl) and np.count_nonzero(blk[2]) == ndir * (m - ml)
    assert np.count_nonzero(blk[1]) == (ndir * (m - ml) if with_gs else 0)
    only_gz = b.debug_vjp_rhs(1, ndir, s, z, valid, None, gz, None)
    assert np.array_equal(only_gz[2], one[2]) and not np.any(only_gz[0]) and not np.any(only_gz[1])
    # the output passes: every want, the unwanted pieces keep the sentinel they went in with
    nP, nA = b._len["P"], b._len["A"]
    dead = dict(q=nl, b=ml, P=len(prs[-1]["P"][2]), A=len(prs[-1]["A"][2]))
    for want in ("q", "qb", "PA", "qbPA"):
        one = b.debug_vjp_out(0, ndir, want, x, z, valid, vx, vz, gs_in, fill=-7.5)
        blk = b.debug_vjp_out(1, ndir, want, x, z, valid, vx, vz, gs_in, fill=-7.5)
        for key, u, v in zip(KEYS, blk, one):
            assert u.shape == (ndir, b._len[key])
            if key not in want:
                assert np.all(u == -7.5) and np.all(v == -7.5), (want, key)
                continue
            assert np.array_equal(u, v), (want, key)
            assert np.all(np.isfinite(u)), (want, key)
            tail = u[:, u.shape[1] - dead[key]:]
            assert np.all(tail == 0.0) and not np.any(np.signbit(tail)), (want, key)
            assert np.count_nonzero(u) == ndir * (b._len[key] - dead[key]), (want, key)
    assert nP > 0 and nA > 0


# ---- 2. the unit right-hand sides are those of the explicit unit vectors -------------------------------------------
@pytest.mark.parametrize("valid", [[1, 1], [1, 0], [0, 1]], ids=["both", "first", "second"])
@pytest.mark.parametrize("piece,first,ndir", [(0, 0, 16), (0, 2, 3), (0, 8, 2), (1, 0, 16), (1, 4, 5), (1, 14, 1),
                                              (2, 0, 16), (2, 5, 3), (2, 20, 4)])
def test_unit_rhs_equals_the_explicit_units(hipdev, piece, first, ndir, valid):
    """basic_lp (n = 3, m = 6) and random_qp(1) (n = 8, m = 14): at first = 2 / 4 / 5 the smaller member runs out of
    entries inside the block, at first = 8 / 14 / 20 the block starts past the end of every member and is zero"""
    prs = [E.basic_lp(), R.random_qp(1)]
    b = batch(hipdev, prs)
    key = "q" if piece == 0 else "b"
    off = b._offsets[key]
    e = np.zeros((ndir, b._len[key]))
    for t in range(ndir):
        for k in range(2):
            if first + t < off[k + 1] - off[k]:
                e[t, off[k] + first + t] = 1.0
    past = first >= max(off[k + 1] - off[k] for k in range(2))
    assert (np.count_nonzero(e) == 0) == past and np.count_nonzero(e) < 2 * ndir
    r = np.random.default_rng(3)
    s, z = r.random(b.stack["m"]) + 0.5, r.random(b.stack["m"]) + 0.5
    got = b.debug_vjp_units(piece, first, ndir, valid)
    want = b.debug_vjp_rhs(1, ndir, s, z, valid, *[e if i == piece else None for i in range(3)])
    single = b.debug_vjp_rhs(0, ndir, s, z, valid, *[e if i == piece else None for i in range(3)])
    hits = sum(int(valid[k]) * int(np.count_nonzero(e[:, off[k]:off[k + 1]])) for k in range(2))
    for i, (u, v, w) in enumerate(zip(got, want, single)):
        assert np.array_equal(u, v) and np.array_equal(u, w), i
        assert not np.any(np.signbit(u[u == 0.0])), i
        assert np.count_nonzero(u) == (hits if i == (0, 2, 1)[piece] else 0), i


# ---- 3. the block's gradients against the reference and against backward() -----------------------------------------
@pytest.mark.parametrize("only_gx", [True, False], ids=["gx_only", "gx_gz_gs"])
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("K", [1, 2, 16, 17])
def test_block_gradients_match_reference_and_backward(hipdev, solved, K, form, only_gx):
    prs, b, sols = solved
    g = block_cotangents(prs, K, 5, only_gx)
    blk = b.backward_block(*(on_device(g) if form == "dev" else g))
    outs = (blk.dq, blk.db, blk.dP, blk.dA)
    if form == "dev":
        assert all(hasattr(v, "is_cuda") and v.is_cuda for v in outs)
    assert [tuple(v.shape) for v in outs] == [(K, b._len[key]) for key in KEYS]
    assert list(blk.valid) == [1] * len(prs)
    assert [tuple(v.shape) for v in blk.per_member(4)] == [(K, 8), (K, 14), (K, 36), (K, 112)]
    worst = against = single = 0.0
    for t in range(K):
        gt = [None if v is None else v[t] for v in g]
        worst = max(worst, worst_against_ref(prs, sols, blk, t, gt))
        one = b.backward(*(on_device(gt) if form == "dev" else gt))
        for k, pr in enumerate(prs):  # the single backward of the same cotangent against the same reference
            want = R.adjoint(pr, sols[k].x, sols[k].s, sols[k].z, *[p[k] for p in
                                                                     [split(prs, v, key) for v, key in zip(gt, IN_KEYS)]])
            single = max([single] + [R.rel(to_host(u), w) for u, w in zip(one.per_member(k), want)])
        against = max([against] + [R.rel(to_host(u[t]), to_host(v))
                                   for u, v in zip(outs, (one.dq, one.db, one.dP, one.dA))])
    print("block of %d (%s, %s): worst vs adjoint_ref %.3e (single backwards %.3e), vs backward() %.3e"
          % (K, form, "gx" if only_gx else "gx gz gs", worst, single, against))
    assert worst <= GRAD_BOUND, (worst, single)
    assert against <= 2.0 * GRAD_BOUND, against


def test_want_selects_the_pieces(hipdev, solved):
    prs, b, sols = solved
    g = block_cotangents(prs, 3, 7)
    full = b.backward_block(*g)
    for want in ("q", "b", "qb", "PA", "A", "bP"):
        for form in ("host", "dev"):
            blk = b.backward_block(*(on_device(g) if form == "dev" else g), want=want)
            for name, key in zip(("dq", "db", "dP", "dA"), KEYS):
                got = getattr(blk, name)
                if key not in want:
                    assert got is None, (want, name)
                    continue
                assert R.rel(to_host(got), getattr(full, name)) <= 2.0 * GRAD_BOUND, (want, name)
            assert worst_against_ref(prs, sols, blk, 2, [v[2] for v in g]) <= GRAD_BOUND
    # the C ABI itself: nothing is written through the pointer of an unwanted piece, and get_dev hands out NULL
    L = hipdev.lib()
    blk = b.backward_block(*g, want="qA")
    keep = [np.full((3, b._len[key]), -7.5) for key in KEYS]
    assert L.chip_bvjp_get(b._h, *[v.ctypes.data_as(hipdev.P_F64) for v in keep], None) == 0
    assert np.array_equal(keep[0], blk.dq) and np.array_equal(keep[3], blk.dA)
    assert np.all(keep[1] == -7.5) and np.all(keep[2] == -7.5)
    ptr = [C.c_void_p(1) for _ in KEYS]
    assert L.chip_bvjp_get_dev(b._h, *[C.byref(p) for p in ptr], None) == 0
    assert ptr[0].value and ptr[3].value and ptr[1].value is None and ptr[2].value is None
    with pytest.raises(ValueError):
        b.backward_block(*g, want="")
    with pytest.raises(ValueError):
        b.backward_block(*g, want="qx")


# ---- 4. the rows of the members' Jacobians -------------------------------------------------------------------------
def jacobian_members():
    """different n and m; the blocks of 16 pass the end of the small members while wide_qp(1) goes on"""
    return [E.basic_lp(), T.wide_qp(1), R.random_qp(1), R.hs35()]


@pytest.fixture(scope="module")
def jac_solved(hipdev):
    prs = jacobian_members()
    assert [pr["n"] for pr in prs][:3] == [3, 70, 8] and [pr["m"] for pr in prs][:3] == [6, 23, 14]
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols] == ["Solved"] * len(prs)
    return prs, b, sols


@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
@pytest.mark.parametrize("of", ["x", "z", "s"])
def test_member_jacobian_rows_row_by_row(hipdev, jac_solved, of, as_torch):
    prs, b, sols = jac_solved
    height = max(pr["n" if of == "x" else "m"] for pr in prs)
    calls = b.debug_counter("vjp_calls")
    if as_torch:
        from clarabel_rs_amd.layer import batch_jacobian_rows
        jac = batch_jacobian_rows(b, of, "qbPA")
        assert all(v.is_cuda for mats in jac for v in mats.values())
    else:
        jac = b.member_jacobian_rows(of, "qbPA")
    assert b.debug_counter("vjp_calls") - calls == -(-height // 16)
    worst = 0.0
    for k, pr in enumerate(prs):
        h = pr["n"] if of == "x" else pr["m"]
        got = {key: to_host(v) for key, v in jac[k].items()}
        assert sorted(got) == sorted(KEYS)
        assert [got[key].shape for key in KEYS] == [(h, length(pr, key)) for key in KEYS]
        for row in range(h):
            e = np.zeros(h)
            e[row] = 1.0
            want = R.adjoint(pr, sols[k].x, sols[k].s, sols[k].z, **{"g" + of: e})
            worst = max([worst] + [R.rel(got[key][row], w) for key, w in zip(KEYS, want)])
    print("member_jacobian_rows(%s, torch=%s): worst row vs adjoint_ref %.3e" % (of, as_torch, worst))
    assert worst <= GRAD_BOUND, worst


def test_rows_equal_the_transposed_columns(hipdev, jac_solved):
    """dx/dq and dx/db by rows (cotangents) and by columns (tangents): two independent device paths to one matrix"""
    prs, b, _ = jac_solved
    rows = b.member_jacobian_rows("x", "qb")
    worst = 0.0
    for wrt in ("q", "b"):
        cols = b.member_jacobians(wrt)
        for k in range(len(prs)):
            assert sorted(rows[k]) == ["b", "q"]
            worst = max(worst, R.rel(rows[k][wrt], cols[k][0]))
    print("rows of dx/dq, dx/db vs the columns of member_jacobians(): worst %.3e" % worst)
    assert worst <= GRAD_BOUND + TAN_BOUND, worst
    for bad in (dict(of="q"), dict(wrt=""), dict(wrt="x")):
        with pytest.raises(ValueError):
            b.member_jacobian_rows(**bad)


def test_members_without_jacobian_rows(hipdev):
    prs = [R.random_qp(1), E.basic_socp(), R.random_qp(2)]
    b = batch(hipdev, prs)
    b.solve()
    jac = b.member_jacobian_rows("x", "qA")
    assert [m is not None for m in jac] == [True, False, True]  # a SecondOrder cone: no derivative
    c = batch(hipdev, prs[::2], max_iter=2)
    assert [s.status for s in c.solve()] == ["MaxIterations"] * 2
    assert c.member_jacobian_rows("z", "b") == [None, None]


# ---- 5. members without a derivative -------------------------------------------------------------------------------
def test_members_without_a_derivative_in_a_block(hipdev):
    prs, want_valid = hetero()
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols[-3:]] == ["Solved", "PrimalInfeasible", "DualInfeasible"]
    K = 3
    g = block_cotangents(prs, K, 21)
    nval = sum(want_valid)
    for v, key in zip(g, IN_KEYS):  # NaN in the parts of the members without a derivative, in all three inputs
        v[:, sum(length(pr, key) for pr in prs[:nval]):] = np.nan
    blk = b.backward_block(*g)
    assert list(blk.valid) == want_valid
    worst = 0.0
    for v in (blk.dq, blk.db, blk.dP, blk.dA):
        assert np.all(np.isfinite(v))
    for t in range(K):
        for k, v in enumerate(want_valid):
            if not v:
                for piece in blk.per_member(k):
                    assert np.all(piece[t] == 0.0) and not np.any(np.signbit(piece[t])), (t, k)
        worst = max(worst, worst_against_ref(prs, sols, blk, t, [v[t] for v in g], only=set(range(nval))))
    print("heterogeneous batch, block of %d, valid members vs adjoint_ref: worst %.3e" % (K, worst))
    assert worst <= GRAD_BOUND, worst
    for of in ("x", "s"):
        jac = b.member_jacobian_rows(of, "qb")
        assert [m is not None for m in jac] == [bool(v) for v in want_valid]


# ---- 6. the handle's state around a block --------------------------------------------------------------------------
def test_state_around_a_block(hipdev):
    prs = members()[:3]
    b = batch(hipdev, prs)
    g = block_cotangents(prs, 2, 1)
    g1 = [v[0] for v in g]
    d = directions(prs, 1)
    L = hipdev.lib()
    F = hipdev.P_F64
    units = lambda piece, first, ndir, want=15: L.chip_bvjp_units(  # noqa: E731
        b._h, C.c_int32(piece), C.c_int64(first), C.c_int32(ndir), C.c_int32(want))
    get = lambda: L.chip_bvjp_get(b._h, None, None, None, None, None)  # noqa: E731
    with pytest.raises(hipdev.ChipError) as e:  # before the first solve
        b.backward_block(*g)
    assert e.value.code == hipdev.ERR_ARG
    assert units(0, 0, 1) == hipdev.ERR_ARG and get() == hipdev.ERR_ARG
    sols = b.solve()
    assert get() == hipdev.ERR_ARG  # solved, no block yet
    for ndir in (0, 17):
        assert L.chip_bvjp_apply_dev(b._h, C.c_int32(ndir), C.c_int32(15), None, None, None) == hipdev.ERR_ARG
        assert L.chip_bvjp_apply(b._h, C.c_int32(ndir), C.c_int32(15), None, None, None) == hipdev.ERR_ARG
        assert units(0, 0, ndir) == hipdev.ERR_ARG
    for want in (0, 16, -1):
        assert L.chip_bvjp_apply_dev(b._h, C.c_int32(1), C.c_int32(want), None, None, None) == hipdev.ERR_ARG
        assert L.chip_bvjp_apply(b._h, C.c_int32(1), C.c_int32(want), None, None, None) == hipdev.ERR_ARG
        assert units(0, 0, 1, want) == hipdev.ERR_ARG
    assert units(3, 0, 1) == units(-1, 0, 1) == units(0, -1, 1) == hipdev.ERR_ARG
    assert get() == hipdev.ERR_ARG  # the refusals left no result
    assert b.debug_counter("vjp_calls") == 0.0
    # a block first: it pays the refactor, the apply after it pays none; neither touches the other's results
    blk = b.backward_block(*g)
    assert b.debug_counter("vjp_refactors") == 1.0
    for t in range(2):
        assert worst_against_ref(prs, sols, blk, t, [v[t] for v in g]) <= GRAD_BOUND
    one = b.jvp(*d)
    assert b.debug_counter("jvp_refactors") == 0.0
    jb = b.jvp_block(*[np.stack([v, 2.0 * v]) for v in d])
    assert b.debug_counter("jac_refactors") == 0.0
    keep = np.zeros((2, b.stack["n"]))
    assert L.chip_bvjp_get(b._h, keep.ctypes.data_as(F), None, None, None, None) == 0
    assert np.array_equal(keep, blk.dq)  # the apply and the block of tangents left the block's results alone
    single = b.backward(*g1)
    b.backward_block(*[2.0 * v for v in g])
    assert b.debug_counter("vjp_refactors") == 1.0  # (the backward between them refactored for itself)
    dx, dq, jx = np.zeros(b.stack["n"]), np.zeros(b.stack["n"]), np.zeros((2, b.stack["n"]))
    assert L.chip_bjvp_get(b._h, dx.ctypes.data_as(F), None, None, None) == 0
    assert L.chip_bgrad_get(b._h, dq.ctypes.data_as(F), None, None, None, None) == 0
    assert L.chip_bjac_get(b._h, jx.ctypes.data_as(F), None, None, None) == 0
    assert np.array_equal(dx, one.dx) and np.array_equal(dq, single.dq) and np.array_equal(jx, jb.dx)
    # data that changed and was not solved: refused, and the last block's result is still there
    assert L.chip_bvjp_get(b._h, keep.ctypes.data_as(F), None, None, None, None) == 0
    b.update(q=[np.array(prs[0]["q"]) * 1.5, None, None])
    with pytest.raises(hipdev.ChipError) as e:
        b.backward_block(*g)
    assert e.value.code == hipdev.ERR_ARG
    assert units(0, 0, 1) == hipdev.ERR_ARG
    again = np.zeros((2, b.stack["n"]))
    assert L.chip_bvjp_get(b._h, again.ctypes.data_as(F), None, None, None, None) == 0
    assert np.array_equal(keep, again)
    prs2 = [dict(prs[0], q=list(np.array(prs[0]["q"]) * 1.5))] + prs[1:]
    sols = b.solve()
    assert get() == hipdev.ERR_ARG  # a new solve: no block yet
    blk = b.backward_block(*g)
    assert b.debug_counter("vjp_refactors") == 2.0
    assert worst_against_ref(prs2, sols, blk, 1, [v[1] for v in g]) <= GRAD_BOUND
    # after a re-equilibration: refused until the next solve
    st = b.stack
    b.reequilibrate(P=st["P"][2], q=st["q"], A=st["A"][2], b=st["b"])
    with pytest.raises(hipdev.ChipError) as e:
        b.backward_block(*g)
    assert e.value.code == hipdev.ERR_ARG
    assert units(1, 0, 1) == hipdev.ERR_ARG and get() == hipdev.ERR_ARG
    # a block after a backward, and after a jvp, of a fresh solve finds K factored
    for first in ("backward", "jvp"):
        c = batch(hipdev, prs)
        sols = c.solve()
        if first == "backward":
            c.backward(*g1)
        else:
            c.jvp(*d)
        blk = c.backward_block(*g)
        assert c.debug_counter("vjp_refactors") == 0.0 and c.debug_counter("vjp_host_syncs") == 1.0
        assert worst_against_ref(prs, sols, blk, 0, g1) <= GRAD_BOUND


def test_solve_after_a_block_equals_solve_without(hipdev):
    prs, _ = hetero()
    a, c = batch(hipdev, prs), batch(hipdev, prs)
    a.solve()
    c.solve()
    a.backward_block(*block_cotangents(prs, 16, 2))
    a.member_jacobian_rows("s", "bA")
    sa, sc = a.solve(), c.solve()
    assert [s.status for s in sa] == [s.status for s in sc]
    assert [s.iterations for s in sa] == [s.iterations for s in sc]
    for u, v in zip(sa[:8], sc[:8]):
        assert R.rel(u.x, v.x) <= 1e-7 and R.rel(u.z, v.z) <= 1e-6


# ---- 7. the cost of a block ----------------------------------------------------------------------------------------
def test_block_cost_in_launches_and_host_syncs(hipdev):
    counts = {}
    for reps in (2, 64):
        prs = [R.random_qp(1)] * reps
        b = batch(hipdev, prs)
        sols = b.solve()
        assert all(s.status == "Solved" for s in sols)
        got = []
        # the first block after the solve pays the refactor; then with and without gs, 16 and 1, and want without matrices
        for ndir, only_gx, want in ((16, False, "qbPA"), (16, False, "qbPA"), (16, True, "qbPA"), (1, False, "qbPA"),
                                    (1, True, "qbPA"), (16, True, "qb"), (1, True, "q"), (16, False, "PA")):
            g = block_cotangents(prs, ndir, 6, only_gx)
            before = b.debug_counter("vjp_repeats")
            blk = b.backward_block(*on_device(g), want=want)
            repeats = b.debug_counter("vjp_repeats") - before
            outs = int("q" in want or "b" in want) + int("P" in want or "A" in want)
            # (a repeat at the collect issues the output launches again and synchronises once more)
            got.append((ndir, b.debug_counter("vjp_launches") - repeats * outs,
                        b.debug_counter("vjp_host_syncs") - repeats))
            if reps == 2:
                t = ndir - 1
                assert worst_against_ref(prs, sols, blk, t, [None if v is None else v[t] for v in g]) <= GRAD_BOUND
        assert b.debug_counter("vjp_refactors") == 1.0 and b.debug_counter("vjp_calls") == 8.0
        counts[reps] = got
    print("block (cotangents, launches, host syncs; both less those of repeats):", counts)
    assert counts[2] == counts[64]
    # valid flags and right-hand side: 2; per cotangent a solve, and an A' product with gs; the output launches wanted;
    # the refactor: 2 launches and 1 synchronisation
    assert counts[2] == [(16, 2.0 + 32 + 2 + 2, 2.0), (16, 2.0 + 32 + 2, 1.0), (16, 2.0 + 16 + 2, 1.0),
                         (1, 2.0 + 2 + 2, 1.0), (1, 2.0 + 1 + 2, 1.0), (16, 2.0 + 16 + 1, 1.0), (1, 2.0 + 1 + 1, 1.0),
                         (16, 2.0 + 32 + 1, 1.0)]


# ---- 8. device inputs that are not 16-byte aligned -----------------------------------------------------------------
def test_device_inputs_at_an_8_byte_offset(hipdev, solved):
    import torch
    prs, b, sols = solved
    K = 3
    g = block_cotangents(prs, K, 13)
    base = b.backward_block(*on_device(g))
    for shifted in ((False, False, True), (True, True, True)):
        args = []
        for v, sh in zip(g, shifted):
            pad = 3 if sh else 2
            t = torch.tensor(np.concatenate([[0.0] * pad, v.ravel()]), dtype=torch.float64, device="cuda")
            t = t[pad:].view(K, v.shape[1])
            assert t.is_contiguous() and (t.data_ptr() % 16 == 8) == sh
            args.append(t)
        blk = b.backward_block(*args)
        worst = max(R.rel(to_host(u), to_host(v)) for u, v in zip((blk.dq, blk.db, blk.dP, blk.dA),
                                                                  (base.dq, base.db, base.dP, base.dA)))
        print("device inputs at 8-byte alignment %s: worst vs the aligned ones %.3e" % (shifted, worst))
        assert worst <= 2.0 * GRAD_BOUND, worst  # (both are within GRAD_BOUND of one reference)
        assert worst_against_ref(prs, sols, blk, K - 1, [v[K - 1] for v in g]) <= GRAD_BOUND


# ---- 9. the input refusals of backward_block -----------------------------------------------------------------------
def test_block_input_refusals(hipdev, solved):
    import torch
    prs, b, _ = solved
    g = block_cotangents(prs, 3, 9)
    calls = b.debug_counter("vjp_calls")
    for bad in (dict(), dict(gx=g[0][0]), dict(gx=g[0][:, :-1]), dict(gx=g[0], gz=g[1][:2]), dict(gz=g[0]),
                dict(gs=g[0]), dict(gx=np.zeros((0, b.stack["n"])))):
        with pytest.raises(hipdev.ChipError) as e:
            b.backward_block(**bad)
        assert e.value.code == hipdev.ERR_DIM
    with pytest.raises(TypeError):  # host and device inputs do not mix
        b.backward_block(gx=g[0], gz=torch.tensor(g[1], dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        b.backward_block(gx=torch.tensor(g[0], dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        b.backward_block(gx=g[0].astype(np.float32))
    assert b.debug_counter("vjp_calls") == calls  # every refusal came before the library was called
    from clarabel_rs_amd.layer import batch_vjp_block
    blk = batch_vjp_block(b, *on_device(g), want="qb")
    assert blk.dq.is_cuda and blk.db.is_cuda and blk.dP is None and blk.dA is None
