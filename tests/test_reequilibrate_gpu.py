"""Re-equilibration of a live handle on the MI355X (chip_reequilibrate_problem / chip_reequilibrate_bdata,
HipSolver.reequilibrate / HipBatchSolver.reequilibrate).  The yardstick is always a FRESH handle created on the same
new data, never the code under test:

1. bytes: after reequilibrate(Y) the scaled data, d, e, c / c_k (and the batch's normq / normb) are those of a fresh
   handle on Y, byte for byte -- after two fresh handles were seen to agree byte for byte themselves;
2. solves: equal statuses and iteration counts; solutions to 1e-10 on the members tests/test_batch_update_gpu.py names
   as reproducing to 1e-13 (here: basic_lp); a second reequilibrate back to X reproduces the handle's first solve;
3. later calls use the new scalings: a partial update_b and a full update_q give a fresh handle's bytes; backward and
   jvp after a solve agree with the fresh handle's, and are refused before that solve;
4. the cap of b at 1e20, host and device form;
5. the load pass on every size and alignment path;
6. refusals that change nothing;
7. the cost: enqueues that do not depend on nprob, one host synchronisation, no chip_kkt_create / chip_kktsystem_create.

Y is X with the rows of A / b and the columns of P / q / A multiplied by powers of two spread over 2^-20 .. 2^20 (one
factor per second-order cone, so that Y stays X in other coordinates): the products are exact and the scalings of Y
are far from those of X."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import e2e_problems as E
from tests.test_batch_adjoint_gpu import GRAD_BOUND, incoming, valid_members
from tests.test_batch_gpu import batch, single
from tests.test_batch_jvp_gpu import TAN_BOUND, directions
from tests.test_problem_update_gpu import _with

pytestmark = pytest.mark.gpu

ZERO, NN, SOC = 0, 1, 2


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


# ---- the problems and their drifted copies ------------------------------------------------------------------------
def zero_nn():
    """basic_qp with the equality x1 + x2 = 1 (which its solution satisfies) in front: Zero + Nonnegative cones"""
    pr = E.basic_qp()
    A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(pr["m"], pr["n"]))
    A = sp.vstack([sp.csc_matrix(np.ones((1, 2))), A]).tocsc()
    A.sort_indices()
    return dict(pr, m=pr["m"] + 1, A=(A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy()),
                b=[1.0] + list(pr["b"]), cones=[(ZERO, 1)] + list(pr["cones"]))


def _spread(count, rng):
    """`count` powers of two with exponents spread evenly over -20 .. 20, in random order"""
    return np.ldexp(1.0, rng.permutation(np.round(np.linspace(-20, 20, count)).astype(int)))


def drift(pr, seed):
    """Y of the module docstring: A <- R A C, b <- R b, P <- C P C, q <- C q with R, C diagonal powers of two"""
    rng = np.random.default_rng(seed)
    n = pr["n"]
    col = _spread(n, rng)
    groups = sum(1 if c[0] == SOC else c[1] for c in pr["cones"])
    f = _spread(groups, rng)
    row, g = [], 0
    for c in pr["cones"]:
        k = 1 if c[0] == SOC else c[1]
        row.append(np.full(c[1], f[g]) if c[0] == SOC else f[g:g + k])
        g += k
    row = np.concatenate(row) if row else np.zeros(0)

    def cols_of(p):
        return np.repeat(np.arange(n), np.diff(np.asarray(p, dtype=np.int64)))
    Pp, Pi, Px = pr["P"]
    Ap, Ai, Ax = pr["A"]
    Pi, Ai = np.asarray(Pi, dtype=np.int64), np.asarray(Ai, dtype=np.int64)
    return _with(pr, P=np.asarray(Px, float) * col[Pi] * col[cols_of(Pp)],
                 A=np.asarray(Ax, float) * row[Ai] * col[cols_of(Ap)], q=np.asarray(pr["q"], float) * col,
                 b=np.asarray(pr["b"], float) * row)


def _vals(pr):
    return (np.asarray(pr["P"][2], float), np.asarray(pr["q"], float), np.asarray(pr["A"][2], float),
            np.asarray(pr["b"], float))


def _stacked(prs):
    return tuple(np.concatenate([_vals(p)[i] for p in prs]) for i in range(4))


def _state(h):
    """everything check 1 compares, as bytes: scaled_data() (with the batch's norms) and the equilibration"""
    out = [np.asarray(a).tobytes() for a in h.scaled_data()]
    eqs = [h.equilibration(k) for k in range(len(h))] if hasattr(h, "n_part") else [h.equilibration()]
    for d, e, c in eqs:
        out += [d.tobytes(), e.tobytes(), np.float64(c).tobytes()]
    return out


def _inf(v):
    return float(np.max(np.abs(v), initial=0.0))


SINGLES = {"zero_nn": zero_nn, "soc": E.basic_socp, "lp": E.basic_lp}
BATCH = (E.basic_lp, E.basic_qp, E.basic_socp)  # an LP with no stored P, a QP, an SOCP
REPRODUCING = {"lp": True, "zero_nn": False, "soc": False}  # (tests/test_batch_update_gpu.py: _reproducible_members)
BATCH_REPRODUCING = (0,)


def _case(hip, case, drifted, **kw):
    """(a handle on X or Y, the four value arrays of the same data)"""
    if case == "batch":
        prs = [drift(f(), 40 + k) if drifted else f() for k, f in enumerate(BATCH)]
        return batch(hip, prs, **kw), _stacked(prs)
    pr = SINGLES[case]()
    pr = drift(pr, 7) if drifted else pr
    return single(hip, pr, **kw), _vals(pr)


def _solutions(h):
    s = h.solve()
    return s if isinstance(s, list) else [s]


def _compare_solves(got, want, reproducing, what):
    for k, (a, f) in enumerate(zip(got, want)):
        print("%s member %d: %s / %s, %d / %d iterations" % (what, k, a.status, f.status, a.iterations, f.iterations))
        assert a.status == f.status and a.iterations == f.iterations, (what, k, a, f)
        tol = 1e-10 * max(1.0, _inf(f.x))
        worst = max(_inf(a.x - f.x), _inf(a.s - f.s), _inf(a.z - f.z))
        print("%s member %d: |re-equilibrated - fresh| %.3e (bound %.3e%s)"
              % (what, k, worst, tol, "" if k in reproducing else ", not asserted"))
        if k in reproducing:
            assert worst <= tol, (what, k, worst)


CASES = ["zero_nn", "soc", "batch"]


# ---- 1. bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("case", CASES)
def test_reequilibrated_handle_is_a_fresh_handle_byte_for_byte(hipdev, case, form):
    h, x_vals = _case(hipdev, case, False)
    f1, y_vals = _case(hipdev, case, True)
    f2, _ = _case(hipdev, case, True)
    fresh = _state(f1)
    assert fresh == _state(f2), "two fresh handles on the same data differ"
    before = _state(h)
    assert before != fresh  # (the scalings really change)
    if form == "dev":
        import torch
        h.reequilibrate(*[torch.tensor(v, dtype=torch.float64, device="cuda") for v in y_vals])
    else:
        h.reequilibrate(*y_vals)
    got = _state(h)
    names = ["Px", "Ax", "q", "b"] + (["normq", "normb"] if case == "batch" else [])
    for k, (a, b) in enumerate(zip(got, fresh)):
        assert a == b, (case, form, names[k] if k < len(names) else "equilibration piece %d" % (k - len(names)))
    # ... and back: the handle's first state again
    h.reequilibrate(*x_vals)
    assert _state(h) == before


def test_batch_list_and_matrix_forms(hipdev):
    """the per-member list form and the matrices on the handle's pattern give the stacked vectors' bytes"""
    prs = [drift(f(), 40 + k) for k, f in enumerate(BATCH)]
    h, _ = _case(hipdev, "batch", False)
    fresh = _state(batch(hipdev, prs))
    gen = h.generation
    n, m = h.stack["n"], h.stack["m"]
    P, q, A, b = _stacked(prs)
    h.reequilibrate(P=[_vals(p)[0] for p in prs], q=[_vals(p)[1] for p in prs],
                    A=sp.csc_matrix((A, h.stack["A"][1].astype(np.int64), h.stack["A"][0].astype(np.int64)), shape=(m, n)),
                    b=b)
    assert _state(h) == fresh and h.generation == gen + 1


# ---- 2. solves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + ["lp"])
def test_solves_of_a_reequilibrated_handle(hipdev, case):
    h, x_vals = _case(hipdev, case, False)
    first = _solutions(h)
    f, y_vals = _case(hipdev, case, True)
    h.reequilibrate(*y_vals)
    repro = BATCH_REPRODUCING if case == "batch" else ((0,) if REPRODUCING[case] else ())
    _compare_solves(_solutions(h), _solutions(f), repro, case + " on Y")
    h.reequilibrate(*x_vals)
    _compare_solves(_solutions(h), first, repro, case + " back on X")


# ---- 3. later calls use the new scalings -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["zero_nn", "batch"])
def test_updates_after_a_reequilibration_scale_with_the_new_factors(hipdev, case):
    h, _ = _case(hipdev, case, False)
    f, y_vals = _case(hipdev, case, True)
    h.reequilibrate(*y_vals)
    rng = np.random.default_rng(3)
    m, n = len(y_vals[3]), len(y_vals[1])
    idx = np.array([m - 1, 0, m // 2])
    vb = y_vals[3][idx] * 1.5 + 0.25
    vq = y_vals[1] * rng.uniform(0.5, 2.0, n)
    for s in (h, f):
        s.update_b((idx, vb))
        s.update_q(vq)
    assert _state(h) == _state(f)


def test_backward_and_jvp_after_a_reequilibration(hipdev):
    """GRAD_BOUND / TAN_BOUND are the bounds tests/test_batch_adjoint_gpu.py / test_batch_jvp_gpu.py hold an updated
    handle's derivatives to; here they bound the difference from the fresh handle's derivatives"""
    from tests import adjoint_ref as R
    prs = valid_members()[:3]
    prs2 = [drift(p, 60 + k) for k, p in enumerate(prs)]
    h, f = batch(hipdev, prs), batch(hipdev, prs2)
    gx, gz, gs = incoming(prs2, 4)
    d = directions(prs2, 6)
    h.solve()
    h.backward(gx, gz, gs)  # (the handle has derivative state from before)
    h.reequilibrate(*_stacked(prs2))
    assert _state(h) == _state(f)
    for call in (lambda: h.backward(gx, gz, gs), lambda: h.jvp(*d)):
        with pytest.raises(hipdev.ChipError) as e:  # before the next solve
            call()
        assert e.value.code == hipdev.ERR_ARG
    sa, sf = h.solve(), f.solve()
    assert [s.status for s in sa] == [s.status for s in sf] and [s.iterations for s in sa] == [s.iterations for s in sf]
    ga, gf = h.backward(gx, gz, gs), f.backward(gx, gz, gs)
    assert list(ga.valid) == list(gf.valid)
    worst = max(R.rel(np.asarray(x), np.asarray(y)) for x, y in zip((ga.dq, ga.db, ga.dP, ga.dA),
                                                                    (gf.dq, gf.db, gf.dP, gf.dA)))
    print("backward, re-equilibrated against fresh: %.3e (bound %.3e)" % (worst, GRAD_BOUND))
    assert worst <= GRAD_BOUND, worst
    ta, tf = h.jvp(*d), f.jvp(*d)
    worst = max(R.rel(np.asarray(x), np.asarray(y)) for x, y in zip((ta.dx, ta.dz, ta.ds), (tf.dx, tf.dz, tf.ds)))
    print("jvp, re-equilibrated against fresh: %.3e (bound %.3e)" % (worst, TAN_BOUND))
    assert worst <= TAN_BOUND, worst


# ---- 4. the cap ------------------------------------------------------------------------------------------------------
def _capped():
    """zero_nn() with b = 1e20, 2e20 and +inf on the rows that are inactive at its solution (-x1 <= 0, -x2 <= 0,
    x1 <= 0.7).  On the CPU, tests/ipm_driver.py over the oracle backend (no equilibration, b capped) ends Solved on
    it after 68 iterations; on the MI355X fresh handles end AlmostSolved after 49 iterations (single solver) and
    Solved after 67 (batch) -- all to the accuracy a norm of b of 1e20 leaves (without presolve the three rows stay in
    the problem), which is why the yardstick is the fresh handle and not the known answer.  basic_lp, basic_qp and
    basic_socp with their inactive rows capped end InsufficientProgress or DualInfeasible within 6 iterations"""
    pr = zero_nn()
    b = np.asarray(pr["b"], float).copy()
    b[[2, 3, 5]] = [1e20, 2e20, np.inf]
    return pr, _with(pr, b=b)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", ["single", "batch"])
def test_b_is_capped_as_create_caps_it(hipdev, kind, form):
    pr, pr2 = _capped()
    make = (lambda p: single(hipdev, p)) if kind == "single" else (lambda p: batch(hipdev, [p, E.basic_lp()]))
    h, f = make(pr), make(pr2)
    vals = _vals(pr2) if kind == "single" else _stacked([pr2, E.basic_lp()])
    if form == "dev":
        import torch
        vals = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in vals]
    h.reequilibrate(*vals)
    assert _state(h) == _state(f)
    sb = h.scaled_data()
    assert np.all(np.isfinite(sb[3]))
    if kind == "batch":
        assert sb[5][0] == 1e20  # normb of the capped member
    _compare_solves(_solutions(h), _solutions(f), (0, 1), "capped " + kind)


# ---- 5. the load pass on every size and alignment path ---------------------------------------------------------------
GRID_PASS = 2048 * 256  # lanes of the widest launch: two entries each on the 16-byte path
LENGTHS = [0, 1, 2, 3, 511, 512, 513, 2 * GRID_PASS + 5]


@pytest.mark.parametrize("misalign", [0, 1, 2, 4, 7], ids=["aligned", "dst+8", "raw+8", "src+8", "all+8"])
def test_load_pass_sizes_and_alignments(hipdev, misalign):
    rng = np.random.default_rng(misalign)
    for ln in LENGTHS:
        src = rng.standard_normal(ln)
        if ln:
            src[rng.integers(0, ln, 3)] = [1e20, 2e20, np.inf]
            src[-1] = 3e20  # (the odd tail of the 16-byte path)
        for cap in (False, True):
            for raw in (False, True):
                if (misalign & 2) and not raw:
                    continue
                dst, rw, od, orw = hipdev.debug_reload_pass(src, cap=cap, raw=raw, misalign=misalign)
                want = np.minimum(src, 1e20) if cap else src
                for buf, o in ((dst, od),) + (((rw, orw),) if raw else ()):
                    assert buf[o:o + ln].tobytes() == want.tobytes(), (ln, cap, raw)
                    assert np.all(buf[:o] == -7.0) and np.all(buf[o + ln:] == -7.0), (ln, cap, raw)


@pytest.mark.parametrize("kind", ["single", "batch"])
def test_device_inputs_8_bytes_past_a_16_byte_boundary(hipdev, kind):
    """each of the four inputs in turn (and all at once) as a slice at an odd offset of a longer tensor; with the
    equilibration off the handle's data are then the inputs themselves, b capped"""
    import torch
    if kind == "single":
        h, vals = _case(hipdev, "soc", False, equilibrate_enable=0)
    else:
        h, vals = _case(hipdev, "batch", False, equilibrate_enable=0)
    rng = np.random.default_rng(1)
    for shifted in ([0], [1], [2], [3], [0, 1, 2, 3], []):
        new = [v * rng.uniform(0.5, 2.0, len(v)) for v in vals]
        new[3][0] = 5e20
        args = []
        for j, v in enumerate(new):
            pad = 3 if j in shifted else 2
            t = torch.tensor(np.concatenate([np.zeros(pad), v]), dtype=torch.float64, device="cuda")[pad:]
            assert t.is_contiguous() and (t.data_ptr() % 16 == 8) == (j in shifted)
            args.append(t)
        h.reequilibrate(*args)
        got = h.scaled_data()
        want = (new[0], new[2], new[1], np.minimum(new[3], 1e20))  # (scaled_data: Px, Ax, q, b)
        for a, w in zip(got[:4], want):
            assert a.tobytes() == w.tobytes(), shifted
        eqs = [h.equilibration(k) for k in range(len(h))] if kind == "batch" else [h.equilibration()]
        assert all(np.all(d == 1.0) and np.all(e == 1.0) and c == 1.0 for d, e, c in eqs)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "batch"])
def test_a_null_array_is_refused_and_changes_nothing(hipdev, kind):
    import torch
    h, vals = _case(hipdev, "soc" if kind == "single" else "batch", False)
    before = _state(h)
    name = "chip_reequilibrate_problem" if kind == "single" else "chip_reequilibrate_bdata"
    L = hipdev.lib()
    host = [v.ctypes.data_as(hipdev.P_F64) for v in vals]
    dev_t = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in vals]
    torch.cuda.synchronize()
    dev = [C.c_void_p(t.data_ptr()) for t in dev_t]
    for j in range(4):
        for fn, args in ((name, host), (name + "_dev", dev)):
            a = list(args)
            a[j] = None
            assert getattr(L, fn)(h._h, *a) == hipdev.ERR_ARG, (fn, j)
    assert _state(h) == before
    assert getattr(L, name)(h._h, *host) == 0  # (the same call with nothing missing is taken)


@pytest.mark.parametrize("transform", ["presolve", "chordal"])
def test_refused_while_a_transform_is_active(hipdev, transform):
    import torch
    from tests.test_problem_transform_gpu import make
    from tests.test_problem_transform_host import presolve_data, sdp_chordal_data
    if transform == "presolve":
        P, q, A, b, cones = presolve_data()
        b[3] = 1e30
        slv = make(hipdev, P, q, A, b, cones, presolve_enable=1)
    else:
        P, q, A, b, cones = sdp_chordal_data()
        slv = make(hipdev, P, q, A, b, cones, chordal_decomposition_enable=1)
    assert not slv.is_data_update_allowed()
    before = _state(slv)
    vals = [np.ones(max(slv._len[k], 1)) for k in "PqAb"]  # (an empty torch tensor's pointer is NULL: another refusal)
    with pytest.raises(hipdev.UpdateNotAllowedError):
        slv.reequilibrate(*vals)
    L = hipdev.lib()
    rc = L.chip_reequilibrate_problem(slv._h, *[v.ctypes.data_as(hipdev.P_F64) for v in vals])
    assert rc == hipdev.ERR_UPDATE_NOT_ALLOWED
    dev_t = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in vals]
    torch.cuda.synchronize()
    rc = L.chip_reequilibrate_problem_dev(slv._h, *[C.c_void_p(t.data_ptr()) for t in dev_t])
    assert rc == hipdev.ERR_UPDATE_NOT_ALLOWED
    assert _state(slv) == before


# ---- 7. the cost -----------------------------------------------------------------------------------------------------
def test_cost_does_not_depend_on_nprob_and_has_no_setup_in_it(hipdev):
    import torch
    pr = E.basic_socp()
    pr2 = drift(pr, 9)
    cost = []
    for copies in (2, 64):
        bs = batch(hipdev, [pr] * copies)
        vals = _stacked([pr2] * copies)
        dev = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in vals]
        creates = (hipdev.debug_create_count(0), hipdev.debug_create_count(1))
        per = []
        for args in (vals, vals, dev):  # the first call (it sets the work buffers up), a later one, the device form
            bs.reequilibrate(*args)
            per.append((bs.debug_counter("update_launches"), bs.debug_counter("update_host_syncs")))
        assert (hipdev.debug_create_count(0), hipdev.debug_create_count(1)) == creates
        assert per[1][1] == 1 and per[2][1] == 1, per
        assert per[1][0] == per[2][0] + 4, per  # (the host form's four uploads)
        assert all(s.status == "Solved" for s in bs.solve())
        cost.append(per[1:])
    assert cost[0] == cost[1], cost
    s = single(hipdev, pr)  # the single solver's call makes no create either
    creates = (hipdev.debug_create_count(0), hipdev.debug_create_count(1))
    s.reequilibrate(*_vals(pr2))
    assert (hipdev.debug_create_count(0), hipdev.debug_create_count(1)) == creates
    assert creates[0] >= 3 and creates[1] >= 3  # (the counters do count: the three handles above)
