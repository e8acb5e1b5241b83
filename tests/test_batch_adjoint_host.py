"""The batched solver's gradients, host side (no GPU needed): the chip_bgrad_* symbols of both builds, the refusal of a
NULL handle before any device is touched, the formulas of tests/adjoint_ref.py against finite differences of the CPU
oracle's interior-point loop, the portfolio QP generator, and the spill / occupancy audit of batch_adjoint.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import ipm_driver as ipm
from tests.test_solver_host import HIPCC, ROOT, _resources

BGRAD_SYMBOLS = ["chip_bgrad_backward", "chip_bgrad_backward_dev", "chip_bgrad_get", "chip_bgrad_get_dev"]


def test_bgrad_symbols_in_both_builds(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_bgrad_[a-zA-Z_]+)\s*\(", hdr))) == sorted(BGRAD_SYMBOLS)
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in BGRAD_SYMBOLS:
            assert hasattr(L, sym), (path, sym)


def test_null_handle_is_refused(hip):
    """CHIP_ERR_ARG before any HIP call: these return the same on a machine without a GPU"""
    L = hip.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    valid = (C.c_int32 * 4)()
    p = C.c_void_p()
    assert L.chip_bgrad_backward(None, None, None, None) == hip.ERR_ARG
    assert L.chip_bgrad_backward(None, g, g, g) == hip.ERR_ARG
    assert L.chip_bgrad_backward_dev(None, None, None, None) == hip.ERR_ARG
    assert L.chip_bgrad_backward_dev(None, g, None, None) == hip.ERR_ARG
    assert L.chip_bgrad_get(None, None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bgrad_get(None, g, g, g, g, valid) == hip.ERR_ARG
    assert L.chip_bgrad_get_dev(None, None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bgrad_get_dev(None, C.byref(p), None, None, None, None) == hip.ERR_ARG
    assert p.value is None and list(valid) == [0, 0, 0, 0]


@pytest.mark.parametrize("name,pr", R.fd_problems(), ids=[n for n, _ in R.fd_problems()])
def test_adjoint_ref_against_finite_differences(oracle, name, pr):
    """adjoint_ref.adjoint against central differences (h = 1e-4) of the oracle loop in every entry of q, b, A and P,
    random gx, gz, gs.  Bound 1e-4 relative: the error is the finite-difference noise of a loop that stops at 1e-8
    (the worst measured here with these gx, gz, gs is 1.3e-6, on random_qp_2's A; with other incoming gradients
    6.0e-6 was seen on random_qp_3 when the formulas were derived), not the formula."""
    def solve(q, b, A, P):
        be = ipm.OracleBackend(oracle, pr["n"], pr["m"], P, A, q, b, pr["cones"])
        out = ipm.solve(be, pr["cones"], q, b)
        assert out["status"] == "Solved", (name, out["status"])
        return out

    out = solve(np.array(pr["q"], float), np.array(pr["b"], float), pr["A"], pr["P"])
    gx, gz, gs = R.incoming(pr, 11)
    dq, db, dP, dA = R.adjoint(pr, out["x"], out["s"], out["z"], gx, gz, gs)
    fd = R.finite_differences(solve, pr, gx, gz, gs, h=1e-4)
    errs = {k: R.rel(a, fd[k]) for k, a in (("q", dq), ("b", db), ("A", dA), ("P", dP))}
    print(name, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1e-4, (name, errs)


def test_random_qps_are_strictly_complementary(oracle):
    """the three random QPs end Solved with some but not all inequalities active and min(s_i + z_i) well away from 0:
    their gradient is well defined"""
    for seed in (1, 2, 3):
        pr = R.random_qp(seed)
        be = ipm.OracleBackend(oracle, pr["n"], pr["m"], pr["P"], pr["A"], pr["q"], pr["b"], pr["cones"])
        out = ipm.solve(be, pr["cones"], pr["q"], pr["b"])
        assert out["status"] == "Solved"
        s, z = out["s"][2:], out["z"][2:]
        active = int(np.sum(s < 1e-6))
        assert 0 < active < 12, (seed, active)
        assert float(np.min(s + z)) >= 4.5e-2, (seed, float(np.min(s + z)))


def test_portfolio_qp_generator(hip, oracle):
    """synthetic.portfolio_qp: the documented layout, and a small instance solves to a long-only fully invested x"""
    import clarabel_rs_amd.synthetic as syn
    na, nf = 12, 3
    pr = syn.portfolio_qp(na, nf, seed=4)
    assert pr["n"] == na + nf and pr["m"] == nf + 1 + 2 * na
    assert [tuple(c) for c in pr["cones"]] == [(R.ZERO, nf + 1), (R.NN, 2 * na)]
    again = syn.portfolio_qp(na, nf, seed=4)
    assert all(np.array_equal(a, b) for a, b in zip(pr["A"], again["A"])) and np.array_equal(pr["q"], again["q"])
    P, A = R.dense(pr)
    assert np.all(np.diag(P) > 0) and np.count_nonzero(P - np.diag(np.diag(P))) == 0
    be = ipm.OracleBackend(oracle, pr["n"], pr["m"], pr["P"], pr["A"], pr["q"], pr["b"], pr["cones"])
    out = ipm.solve(be, pr["cones"], pr["q"], pr["b"])
    assert out["status"] == "Solved"
    x = out["x"][:na]
    assert abs(float(np.sum(x)) - 1.0) <= 1e-6 and float(np.min(x)) >= -1e-6 and float(np.max(x)) <= pr["cap"] + 1e-6
    assert np.max(np.abs(pr["F"].T @ x - out["x"][na:])) <= 1e-6


# every kernel of batch_adjoint.hip: no scratch, eight waves per SIMD (256-thread workgroups, streaming passes)
BA_KERNELS = ["k_ba_rhs", "k_ba_grad_vec", "k_ba_grad_mat"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_adjoint_kernels_do_not_spill():
    res = _resources("batch_adjoint.hip")
    seen = 0
    for k in BA_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert names, (k, sorted(res))
        for nm in names:
            r = res[nm]
            assert r["ScratchSize"] == 0, (k, r)
            assert r["Occupancy"] >= 8, (k, r)
        seen += len(names)
    assert seen == len(res), sorted(res)
