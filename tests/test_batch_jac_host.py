"""The batched solver's blocks of tangents and member Jacobians, host side (no GPU needed): the chip_bjac_* symbols of
both builds and the test hooks of the test build alone, the refusal of a NULL handle before any device is touched, the
spill audit of batch_jacobian.hip, and the unit conventions of tests/tangent_ref.py that member_jacobians() relies on:
a unit direction in q gives minus a column of K^-1, one in b gives a column of K^-1."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import tangent_ref as T
from tests.test_batch_jvp_host import oracle_solve
from tests.test_solver_host import HIPCC, ROOT, _resources

BJAC_SYMBOLS = ["chip_bjac_apply", "chip_bjac_apply_dev", "chip_bjac_units", "chip_bjac_get", "chip_bjac_get_dev"]
HOOKS = ["chip_debug_batch_jac_rhs", "chip_debug_batch_jac_units"]
PROBLEMS = T.host_problems()
IDS = [n for n, _ in PROBLEMS]


def test_bjac_symbols_in_both_builds_and_the_hooks_in_the_test_build_only(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_bjac_[a-zA-Z_]+)\s*\(", hdr))) == sorted(BJAC_SYMBOLS)
    assert re.search(r"#define\s+CHIP_BJAC_MAX_DIR\s+16\b", hdr)
    assert hip.BJAC_MAX_DIR == 16
    testing = open(os.path.join(ROOT, "include", "clarabel_hip_testing.h")).read()
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in BJAC_SYMBOLS:
            assert hasattr(L, sym), (path, sym)
    for hook in HOOKS:
        assert hook not in hdr and hook in testing
        assert hasattr(C.CDLL(hip.LIB_PATH), hook)
        assert not hasattr(C.CDLL(hip.SHIP_LIB_PATH), hook)


def test_null_handle_is_refused(hip):
    """CHIP_ERR_ARG before any HIP call: these return the same on a machine without a GPU"""
    L = hip.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    valid = (C.c_int32 * 4)()
    p = C.c_void_p()
    first = C.c_int64(0)
    assert L.chip_bjac_apply(None, 1, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjac_apply(None, 1, g, g, g, g) == hip.ERR_ARG
    assert L.chip_bjac_apply_dev(None, 1, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjac_apply_dev(None, 16, g, None, None, None) == hip.ERR_ARG
    assert L.chip_bjac_units(None, 0, first, 1) == hip.ERR_ARG
    assert L.chip_bjac_units(None, 1, first, 16) == hip.ERR_ARG
    assert L.chip_bjac_get(None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjac_get(None, g, g, g, valid) == hip.ERR_ARG
    assert L.chip_bjac_get_dev(None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjac_get_dev(None, C.byref(p), None, None, None) == hip.ERR_ARG
    assert L.chip_debug_batch_jac_rhs(None, 1, g, g, valid, g, g, g, g, g, g) == hip.ERR_ARG
    assert L.chip_debug_batch_jac_units(None, 0, first, 1, valid, g, g) == hip.ERR_ARG
    assert p.value is None and list(valid) == [0, 0, 0, 0] and list(g) == [1.0, 2.0, 3.0, 4.0]


# every kernel of batch_jacobian.hip: no scratch (the accumulators of a tile of directions stay in registers)
BJ_KERNELS = ["k_bj_rhs", "k_bj_units", "k_bj_out"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_jacobian_kernels_do_not_spill():
    res = _resources("batch_jacobian.hip")
    seen = 0
    for k in BJ_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert names, (k, sorted(res))
        for nm in names:
            assert res[nm]["ScratchSize"] == 0, (k, res[nm])
        seen += len(names)
    assert seen == len(res), sorted(res)


@pytest.fixture(scope="module")
def solutions(oracle):
    """the oracle's solution of each of the nine problems, computed once"""
    return {name: oracle_solve(oracle, pr, np.array(pr["q"], float), np.array(pr["b"], float), pr["A"], pr["P"], name)
            for name, pr in PROBLEMS}


@pytest.mark.parametrize("name,pr", PROBLEMS, ids=IDS)
def test_unit_directions_give_the_columns_of_the_inverse(solutions, name, pr):
    """tangent(dq = e_j) is -K^-1[:, j] and tangent(db = e_i) is K^-1[:, n + i], against np.linalg.inv of the same
    dense K: two dense factorisations of one matrix of at most 93 x 93, so the bound is rounding, 1e-12 relative (the
    bound of test_batch_jvp_host.py's transpose identity).  ds = -A dx (piece q) and e_i - A dx (piece b) on the
    Nonnegative rows, an exact +0.0 on the Zero rows."""
    out = solutions[name]
    x, s, z = (np.asarray(out[key], dtype=float) for key in "xsz")
    n, m = pr["n"], pr["m"]
    P, A = R.dense(pr)
    K = np.block([[P, A.T], [A, -R.hmat(pr["cones"], s, z)]])
    Kinv = np.linalg.inv(K)
    nn = T.nn_rows(pr)
    worst = 0.0
    for col in range(n + m):
        e = np.zeros(n + m)
        e[col] = 1.0
        if col < n:
            dx, dz, ds = T.tangent(pr, x, s, z, dq=e[:n])
            want, rz = -Kinv[:, col], np.zeros(m)
        else:
            dx, dz, ds = T.tangent(pr, x, s, z, db=e[n:])
            want, rz = Kinv[:, col], e[n:]
        worst = max(worst, R.rel(np.concatenate([dx, dz]), want))
        assert np.array_equal(ds[nn], (rz - A @ dx)[nn]), (name, col)
        assert np.all(ds[~nn] == 0.0) and not np.any(np.signbit(ds[~nn])), (name, col)
    print(name, "unit tangents vs columns of inv(K): %.2e" % worst)
    assert worst <= 1e-12, (name, worst)
