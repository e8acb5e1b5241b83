"""The batched solver's blocks of tangents and member Jacobians (chip_bjac_*, HipBatchSolver.jvp_block /
member_jacobians, layer.batch_jacobians) on the MI355X: the block's right-hand side pass bit for bit against the single
pass on rows of every length class, the unit right-hand sides against the explicit unit vectors, the block's tangents
against tests/tangent_ref.py at the device's own solution and against jvp() of the same direction, the members'
Jacobians column by column, members without a derivative, the handle's state around a block, and its cost in launches
and host synchronisations.

A direction of a block is the computation of a single apply, so the bounds are those of tests/test_batch_jvp_gpu.py
(TAN_BOUND: ten times the worst figure measured there, REPEAT_CEILING: two results of one factorisation); a block
against jvp() of the same direction is held to 2 TAN_BOUND, both being within TAN_BOUND of one reference.

The launches of one block, read from the host code (one per kernel, copy or call into the KKT layer, as the batched
solver counts everywhere): valid flags (1), right-hand side (1), per direction one enqueued solve and one A product
(2 ndir), the output pass (1) = 3 + 2 ndir, and 2 more (scaling update, refactor) when K is not factored at the final
iterates; host synchronisations: the collect (1), the refactor's when it is paid, and one per repeat at the collect."""
import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import e2e_problems as E
from tests import tangent_ref as T
from tests.test_batch_jvp_gpu import (KEYS, REPEAT_CEILING, ROW_LENGTHS, TAN_BOUND, batch, directions, hetero, length,
                                      long_row_members, members, to_host, worst_against_ref)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def block_directions(prs, K, seed, only_dq=False):
    """K random directions, row t of every piece = direction t: [dq [K, n], db, dP, dA] (None where absent)"""
    per = [directions(prs, seed + 1000 * t, only_dq) for t in range(K)]
    return [None if per[0][i] is None else np.stack([d[i] for d in per]) for i in range(4)]


def on_device(vs):
    import torch
    return [None if v is None else torch.tensor(v, dtype=torch.float64, device="cuda") for v in vs]


def direction_of(hip, b, blk, t):
    """direction t of a block as a BatchTangent (what worst_against_ref takes)"""
    return hip.BatchTangent(blk.dx[t], blk.dz[t], blk.ds[t], blk.valid, b._offsets)


@pytest.fixture(scope="module")
def solved(hipdev):
    """one batch of the eight members, solved once, shared by the tests that only apply"""
    prs = members()
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols] == ["Solved"] * len(prs)
    return prs, b, sols


@pytest.fixture(scope="module")
def rows(hipdev):
    """the two members with rows of every length class, created once (the right-hand side passes need no solve)"""
    prs = long_row_members()
    b = batch(hipdev, prs)
    assert sorted(np.bincount(prs[0]["A"][1], minlength=len(ROW_LENGTHS))) == ROW_LENGTHS
    r = np.random.default_rng(5)
    return prs, b, r.standard_normal(b.stack["n"]), r.standard_normal(b.stack["m"])


# ---- 1. the block's right-hand side pass is bit for bit the single pass --------------------------------------------
@pytest.mark.parametrize("invalid", [1, 0])
@pytest.mark.parametrize("ndir", [1, 3, 16])
def test_block_rhs_is_bitwise_the_single_rhs(rows, ndir, invalid):
    """rows owned by a lane, a wavefront and the workgroup in both spaces (32 | 33, 16384 | 16385, 16 500), a partial
    tile, one tile and a full block; one member invalid with NaN in everything of it that could be read"""
    prs, b, x, z = rows
    r = np.random.default_rng(100 + ndir)
    d = [r.standard_normal((ndir, b._len[key])) for key in KEYS]
    valid = [1, 1]
    valid[invalid] = 0
    x, z = x.copy(), z.copy()
    n0, m0 = prs[0]["n"], prs[0]["m"]
    part = (lambda ln: slice(ln, None)) if invalid == 1 else (lambda ln: slice(0, ln))
    x[part(n0)] = np.nan
    z[part(m0)] = np.nan
    for v, key in zip(d, KEYS):
        v[:, part(length(prs[0], key))] = np.nan
    rx, rz = b.debug_jac_rhs(ndir, x, z, valid, *d)
    assert rx.shape == (ndir, b.stack["n"]) and rz.shape == (ndir, b.stack["m"])
    for t in range(ndir):
        sx, sz = b.debug_jvp_rhs(x, z, valid, *[v[t] for v in d])
        assert np.array_equal(rx[t], sx) and np.array_equal(rz[t], sz), t
        live = np.concatenate([rx[t][part(n0)], rz[t][part(m0)]])
        assert np.all(live == 0.0) and not np.any(np.signbit(live)), t  # the invalid member: exact +0.0
        other = np.concatenate([sx, sz])
        assert np.all(np.isfinite(other)) and np.count_nonzero(other) == other.size - live.size
    # a block without dP and dA: every row is empty and still receives its dq / db term
    rx0, rz0 = b.debug_jac_rhs(ndir, x, z, valid, d[0], d[1], None, None)
    for t in range(ndir):
        sx, sz = b.debug_jvp_rhs(x, z, valid, d[0][t], d[1][t], None, None)
        assert np.array_equal(rx0[t], sx) and np.array_equal(rz0[t], sz), t


# ---- 2. the unit right-hand sides are those of the explicit unit vectors -------------------------------------------
@pytest.mark.parametrize("valid", [[1, 1], [1, 0], [0, 1]], ids=["both", "first", "second"])
@pytest.mark.parametrize("piece,first,ndir", [(0, 0, 16), (0, 2, 3), (0, 16496, 16), (1, 0, 16), (1, 7, 2),
                                              (1, 16499, 1)])
def test_unit_rhs_equals_the_explicit_units(rows, piece, first, ndir, valid):
    """the members have 16 500 and 3 entries of q, 8 and 16 500 of b: in every case but one a member runs out of
    entries inside the block, and past the end of the longer one the direction is zero everywhere"""
    prs, b, x, z = rows
    key = "q" if piece == 0 else "b"
    off = b._offsets[key]
    e = np.zeros((ndir, b._len[key]))
    for t in range(ndir):
        for k in range(2):
            if first + t < off[k + 1] - off[k]:
                e[t, off[k] + first + t] = 1.0
    assert 0 < np.count_nonzero(e) < 2 * ndir
    ux, uz = b.debug_jac_units(piece, first, ndir, valid)
    wx, wz = b.debug_jac_rhs(ndir, x, z, valid, dq=e if piece == 0 else None, db=e if piece == 1 else None)
    assert np.array_equal(ux, wx) and np.array_equal(uz, wz)
    hit = ux if piece == 0 else uz
    want = sum(int(valid[k]) * int(np.count_nonzero(e[:, off[k]:off[k + 1]])) for k in range(2))
    assert np.count_nonzero(hit) == want and np.count_nonzero(uz if piece == 0 else ux) == 0
    assert not np.any(np.signbit(ux[ux == 0.0])) and not np.any(np.signbit(uz[uz == 0.0]))


# ---- 3. the block's tangents against the reference and against jvp() -----------------------------------------------
@pytest.mark.parametrize("only_dq", [True, False], ids=["dq_only", "dq_db_dP_dA"])
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("K", [1, 2, 16, 17])
def test_block_tangents_match_reference_and_jvp(hipdev, solved, K, form, only_dq):
    prs, b, sols = solved
    d = block_directions(prs, K, 5, only_dq)
    blk = b.jvp_block(*(on_device(d) if form == "dev" else d))
    if form == "dev":
        assert all(hasattr(v, "is_cuda") and v.is_cuda for v in (blk.dx, blk.dz, blk.ds))
    assert tuple(blk.dx.shape) == (K, b.stack["n"]) and tuple(blk.dz.shape) == tuple(blk.ds.shape) == (K, b.stack["m"])
    assert list(blk.valid) == [1] * len(prs)
    assert [tuple(v.shape) for v in blk.per_member(7)] == [(K, 70), (K, 23), (K, 23)]
    worst = against = 0.0
    for t in range(K):
        dt = [None if v is None else v[t] for v in d]
        worst = max(worst, worst_against_ref(prs, sols, direction_of(hipdev, b, blk, t), dt))
        one = b.jvp(*(on_device(dt) if form == "dev" else dt))
        against = max([against] + [R.rel(to_host(u[t]), to_host(v))
                                   for u, v in zip((blk.dx, blk.dz, blk.ds), (one.dx, one.dz, one.ds))])
    print("block of %d (%s, %s): worst vs tangent_ref %.3e, vs jvp() %.3e"
          % (K, form, "dq" if only_dq else "dq db dP dA", worst, against))
    assert worst <= TAN_BOUND, worst
    assert against <= 2.0 * TAN_BOUND, against


def test_block_input_refusals(hipdev, solved):
    import torch
    prs, b, _ = solved
    d = block_directions(prs, 3, 9)
    calls = b.debug_counter("jac_calls")
    for bad in (dict(), dict(dq=d[0][0]), dict(dq=d[0][:, :-1]), dict(dq=d[0], db=d[1][:2]), dict(db=d[0]),
                dict(dq=np.zeros((0, b.stack["n"])))):
        with pytest.raises(hipdev.ChipError) as e:
            b.jvp_block(**bad)
        assert e.value.code == hipdev.ERR_DIM
    with pytest.raises(TypeError):  # host and device inputs do not mix
        b.jvp_block(dq=d[0], db=torch.tensor(d[1], dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        b.jvp_block(dq=torch.tensor(d[0], dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        b.jvp_block(dq=d[0].astype(np.float32))
    assert b.debug_counter("jac_calls") == calls  # every refusal came before the library was called


# ---- 4. the members' Jacobians -------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("wrt", ["q", "b"])
def test_member_jacobians_column_by_column(hipdev, jac_solved, wrt, as_torch):
    prs, b, sols = jac_solved
    width = max(pr["n" if wrt == "q" else "m"] for pr in prs)
    calls = b.debug_counter("jac_calls")
    if as_torch:
        from clarabel_rs_amd.layer import batch_jacobians
        jac = batch_jacobians(b, wrt)
        assert all(v.is_cuda for mats in jac for v in mats)
    else:
        jac = b.member_jacobians(wrt)
    assert b.debug_counter("jac_calls") - calls == -(-width // 16)
    worst = sym = 0.0
    for k, pr in enumerate(prs):
        w = pr["n"] if wrt == "q" else pr["m"]
        got = [to_host(v) for v in jac[k]]
        assert [v.shape for v in got] == [(pr["n"], w), (pr["m"], w), (pr["m"], w)]
        nn = T.nn_rows(pr)
        for col in range(w):
            e = np.zeros(w)
            e[col] = 1.0
            want = T.tangent(pr, sols[k].x, sols[k].s, sols[k].z, **{"d" + wrt: e})
            worst = max([worst] + [R.rel(g[:, col], v) for g, v in zip(got, want)])
        assert np.all(got[2][~nn] == 0.0) and not np.any(np.signbit(got[2][~nn])), k  # ds on Zero rows: exact +0.0
        if wrt == "q":  # dx/dq = -(K^-1)_xx: symmetric
            sym = max(sym, R.rel(got[0], got[0].T))
    print("member_jacobians(%s, torch=%s): worst column vs tangent_ref %.3e, asymmetry of dx/dq %.3e"
          % (wrt, as_torch, worst, sym))
    assert worst <= TAN_BOUND, worst
    assert sym <= 2.0 * TAN_BOUND, sym


# ---- 5. members without a derivative -------------------------------------------------------------------------------
def test_members_without_a_derivative_in_a_block(hipdev):
    prs, want_valid = hetero()
    b = batch(hipdev, prs)
    sols = b.solve()
    assert [s.status for s in sols[-3:]] == ["Solved", "PrimalInfeasible", "DualInfeasible"]
    K = 3
    d = block_directions(prs, K, 21)
    nval = sum(want_valid)
    for v, key in zip(d, KEYS):  # NaN in the parts of the members without a derivative, in all four inputs
        v[:, sum(length(pr, key) for pr in prs[:nval]):] = np.nan
    blk = b.jvp_block(*d)
    assert list(blk.valid) == want_valid
    worst = 0.0
    for t in range(K):
        one = direction_of(hipdev, b, blk, t)
        for v in (one.dx, one.dz, one.ds):
            assert np.all(np.isfinite(v))
        for k, v in enumerate(want_valid):
            if not v:
                for piece in one.per_member(k):
                    assert np.all(piece == 0.0) and not np.any(np.signbit(piece)), (t, k)
        worst = max(worst, worst_against_ref(prs, sols, one, [v[t] for v in d], only=set(range(nval))))
    print("heterogeneous batch, block of %d, valid members vs tangent_ref: worst %.3e" % (K, worst))
    assert worst <= TAN_BOUND, worst
    for wrt in ("q", "b"):
        jac = b.member_jacobians(wrt)
        assert [m is not None for m in jac] == [bool(v) for v in want_valid]


# ---- 6. the handle's state around a block --------------------------------------------------------------------------
def test_state_around_a_block(hipdev):
    import ctypes as C
    prs = members()[:3]
    b = batch(hipdev, prs)
    d = block_directions(prs, 2, 1)
    d1 = [v[0] for v in d]
    L = hipdev.lib()
    units = lambda piece, first, ndir: L.chip_bjac_units(b._h, C.c_int32(piece), C.c_int64(first), C.c_int32(ndir))  # noqa: E731
    with pytest.raises(hipdev.ChipError) as e:  # before the first solve
        b.jvp_block(*d)
    assert e.value.code == hipdev.ERR_ARG
    assert units(0, 0, 1) == hipdev.ERR_ARG
    assert L.chip_bjac_get(b._h, None, None, None, None) == hipdev.ERR_ARG
    sols = b.solve()
    assert L.chip_bjac_get(b._h, None, None, None, None) == hipdev.ERR_ARG  # solved, no block yet
    for ndir in (0, 17):
        assert L.chip_bjac_apply_dev(b._h, C.c_int32(ndir), None, None, None, None) == hipdev.ERR_ARG
        assert L.chip_bjac_apply(b._h, C.c_int32(ndir), None, None, None, None) == hipdev.ERR_ARG
        assert units(0, 0, ndir) == hipdev.ERR_ARG
    assert units(2, 0, 1) == units(-1, 0, 1) == units(0, -1, 1) == hipdev.ERR_ARG
    assert L.chip_bjac_get(b._h, None, None, None, None) == hipdev.ERR_ARG  # the refusals left no result
    # a block first: it pays the refactor, the apply after it pays none; neither touches the other's results
    blk = b.jvp_block(*d)
    assert b.debug_counter("jac_refactors") == 1.0
    for t in range(2):
        assert worst_against_ref(prs, sols, direction_of(hipdev, b, blk, t), [v[t] for v in d]) <= TAN_BOUND
    one = b.jvp(*d1)
    assert b.debug_counter("jvp_refactors") == 0.0
    keep = np.zeros((2, b.stack["n"]))
    assert L.chip_bjac_get(b._h, keep.ctypes.data_as(hipdev.P_F64), None, None, None) == 0
    assert np.array_equal(keep, blk.dx)  # the apply left the block's results alone
    b.jvp_block(*[2.0 * v for v in d])
    dx = np.zeros(b.stack["n"])
    assert L.chip_bjvp_get(b._h, dx.ctypes.data_as(hipdev.P_F64), None, None, None) == 0
    assert np.array_equal(dx, one.dx)  # ... and the block the apply's
    assert b.debug_counter("jac_refactors") == 1.0
    # data that changed and was not solved: refused, and the last block's result is still there
    assert L.chip_bjac_get(b._h, keep.ctypes.data_as(hipdev.P_F64), None, None, None) == 0
    b.update(q=[np.array(prs[0]["q"]) * 1.5, None, None])
    with pytest.raises(hipdev.ChipError) as e:
        b.jvp_block(*d)
    assert e.value.code == hipdev.ERR_ARG
    assert units(0, 0, 1) == hipdev.ERR_ARG
    again = np.zeros((2, b.stack["n"]))
    assert L.chip_bjac_get(b._h, again.ctypes.data_as(hipdev.P_F64), None, None, None) == 0
    assert np.array_equal(keep, again)
    prs2 = [dict(prs[0], q=list(np.array(prs[0]["q"]) * 1.5))] + prs[1:]
    sols = b.solve()
    assert L.chip_bjac_get(b._h, None, None, None, None) == hipdev.ERR_ARG  # a new solve: no block yet
    blk = b.jvp_block(*d)
    assert b.debug_counter("jac_refactors") == 2.0
    assert worst_against_ref(prs2, sols, direction_of(hipdev, b, blk, 1), [v[1] for v in d]) <= TAN_BOUND
    # a block after a backward of a fresh solve finds K factored
    c = batch(hipdev, prs)
    sols = c.solve()
    c.backward(*[np.concatenate([R.incoming(pr, 4 + 17 * k)[i] for k, pr in enumerate(prs)]) for i in range(3)])
    blk = c.jvp_block(*d)
    assert c.debug_counter("jac_refactors") == 0.0
    assert worst_against_ref(prs, sols, direction_of(hipdev, c, blk, 0), d1) <= TAN_BOUND


def test_solve_after_a_block_equals_solve_without(hipdev):
    prs, _ = hetero()
    a, c = batch(hipdev, prs), batch(hipdev, prs)
    a.solve()
    c.solve()
    a.jvp_block(*block_directions(prs, 16, 2))
    a.member_jacobians("b")
    sa, sc = a.solve(), c.solve()
    assert [s.status for s in sa] == [s.status for s in sc]
    assert [s.iterations for s in sa] == [s.iterations for s in sc]
    for u, v in zip(sa[:8], sc[:8]):
        assert R.rel(u.x, v.x) <= 1e-7 and R.rel(u.z, v.z) <= 1e-6


# ---- 7. the cost of a block ----------------------------------------------------------------------------------------
def test_block_cost_in_launches_and_host_syncs(hipdev):
    counts = {}
    for reps in (2, 16):
        prs = [R.random_qp(1)] * reps
        b = batch(hipdev, prs)
        sols = b.solve()
        assert all(s.status == "Solved" for s in sols)
        got = []
        for ndir in (16, 16, 1):  # the first block after the solve pays the refactor
            d = block_directions(prs, ndir, 6)
            before = b.debug_counter("jac_repeats")
            blk = b.jvp_block(*on_device(d))
            repeats = b.debug_counter("jac_repeats") - before
            # (a repeat at the collect issues the products and the output pass again and synchronises once more)
            got.append((ndir, b.debug_counter("jac_launches") - repeats * (ndir + 1),
                        b.debug_counter("jac_host_syncs") - repeats))
            if reps == 2:
                t = ndir - 1
                assert worst_against_ref(prs, sols, direction_of(hipdev, b, blk, t), [v[t] for v in d]) <= TAN_BOUND
        assert b.debug_counter("jac_refactors") == 1.0 and b.debug_counter("jac_calls") == 3.0
        counts[reps] = got
    print("block (directions, launches, host syncs; both less those of repeats), first / reusing / reusing:", counts)
    assert counts[2] == counts[16]
    # valid flags, right-hand side and output pass: 3; per direction a solve and a product: 2; the refactor: 2 and 1
    assert counts[2] == [(16, 3.0 + 2 * 16 + 2, 2.0), (16, 3.0 + 2 * 16, 1.0), (1, 3.0 + 2 * 1, 1.0)]


# ---- 8. device inputs that are not 16-byte aligned -----------------------------------------------------------------
def test_device_inputs_at_an_8_byte_offset(hipdev, solved):
    import torch
    prs, b, sols = solved
    K = 3
    d = block_directions(prs, K, 13)
    base = b.jvp_block(*on_device(d))
    for shifted in ((False, False, False, True), (True, True, True, True)):
        args = []
        for v, sh in zip(d, shifted):
            pad = 3 if sh else 2
            t = torch.tensor(np.concatenate([[0.0] * pad, v.ravel()]), dtype=torch.float64, device="cuda")
            t = t[pad:].view(K, v.shape[1])
            assert t.is_contiguous() and (t.data_ptr() % 16 == 8) == sh
            args.append(t)
        blk = b.jvp_block(*args)
        worst = max(R.rel(to_host(u), to_host(v)) for u, v in zip((blk.dx, blk.dz, blk.ds), (base.dx, base.dz, base.ds)))
        print("device inputs at 8-byte alignment %s: worst vs the aligned ones %.3e" % (shifted, worst))
        assert worst <= REPEAT_CEILING, worst
        assert worst_against_ref(prs, sols, direction_of(hipdev, b, blk, K - 1), [v[K - 1] for v in d]) <= TAN_BOUND
