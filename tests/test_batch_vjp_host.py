"""The batched solver's blocks of cotangents and Jacobian rows, host side (no GPU needed): the chip_bvjp_* symbols of
both builds and the test hooks of the test build alone, the refusals that come before any device is touched, the
resource audit of batch_cotangent.hip, and the unit conventions of tests/adjoint_ref.py that member_jacobian_rows()
relies on: a unit cotangent in x gives minus a row of K^-1 as the gradient in q and a row of K^-1 as the one in b."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import adjoint_ref as R
from tests.test_batch_jvp_host import oracle_solve
from tests.test_solver_host import HIPCC, ROOT, _resources

BVJP_SYMBOLS = ["chip_bvjp_apply", "chip_bvjp_apply_dev", "chip_bvjp_units", "chip_bvjp_get", "chip_bvjp_get_dev"]
HOOKS = ["chip_debug_batch_vjp_rhs", "chip_debug_batch_vjp_units", "chip_debug_batch_vjp_out"]
PROBLEMS = R.fd_problems()
IDS = [n for n, _ in PROBLEMS]


def test_bvjp_symbols_in_both_builds_and_the_hooks_in_the_test_build_only(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_bvjp_[a-zA-Z_]+)\s*\(", hdr))) == sorted(BVJP_SYMBOLS)
    assert re.search(r"#define\s+CHIP_BVJP_MAX_DIR\s+16\b", hdr)
    assert hip.BVJP_MAX_DIR == 16
    testing = open(os.path.join(ROOT, "include", "clarabel_hip_testing.h")).read()
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in BVJP_SYMBOLS:
            assert hasattr(L, sym), (path, sym)
    for hook in HOOKS:
        assert hook not in hdr and hook in testing
        assert hasattr(C.CDLL(hip.LIB_PATH), hook)
        assert not hasattr(C.CDLL(hip.SHIP_LIB_PATH), hook)


def test_null_handle_and_bad_scalars_are_refused(hip):
    """CHIP_ERR_ARG before any HIP call: these return the same on a machine without a GPU.  (The scalar checks of a
    live handle -- ndir outside 1..16, want 0 or beyond bit 3, piece outside 0..2, first < 0 -- are made on the GPU by
    tests/test_batch_vjp_gpu.py: a handle cannot be created without a device.)"""
    L = hip.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    valid = (C.c_int32 * 4)()
    p = C.c_void_p()
    i64 = C.c_int64
    for ndir in (1, 16, 0, 17, -1):
        for want in (15, 1, 0, 16, -1):
            assert L.chip_bvjp_apply(None, ndir, want, None, None, None) == hip.ERR_ARG
            assert L.chip_bvjp_apply(None, ndir, want, g, g, g) == hip.ERR_ARG
            assert L.chip_bvjp_apply_dev(None, ndir, want, None, None, None) == hip.ERR_ARG
            assert L.chip_bvjp_apply_dev(None, ndir, want, g, None, None) == hip.ERR_ARG
            for piece in (0, 1, 2, 3, -1):
                for first in (0, 5, -1):
                    assert L.chip_bvjp_units(None, piece, i64(first), ndir, want) == hip.ERR_ARG
    assert L.chip_bvjp_get(None, None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bvjp_get(None, g, g, g, g, valid) == hip.ERR_ARG
    assert L.chip_bvjp_get_dev(None, None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bvjp_get_dev(None, C.byref(p), None, None, None, None) == hip.ERR_ARG
    for form in (0, 1):
        assert L.chip_debug_batch_vjp_rhs(None, form, 1, g, g, valid, g, g, g, g, g, g) == hip.ERR_ARG
        assert L.chip_debug_batch_vjp_out(None, form, 1, 15, g, g, valid, g, g, g, g, g, g, g) == hip.ERR_ARG
    assert L.chip_debug_batch_vjp_units(None, 0, i64(0), 1, valid, g, g, g) == hip.ERR_ARG
    assert p.value is None and list(valid) == [0, 0, 0, 0] and list(g) == [1.0, 2.0, 3.0, 4.0]


# every kernel of batch_cotangent.hip with the occupancy the build reports for it, as a floor: the loops over the
# cotangents hold no private array, so nothing is in scratch and every kernel stays at 8 waves per SIMD (at most 33
# VGPRs)
BC_KERNELS = {"k_bc_rhs": 8, "k_bc_units": 8, "k_bc_grad_vec": 8, "k_bc_grad_mat": 8}
BC_INSTANCES = 5  # k_bc_grad_vec<true> and <false>


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_cotangent_kernels_do_not_spill():
    res = _resources("batch_cotangent.hip")
    seen = 0
    for k, floor in BC_KERNELS.items():
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert names, (k, sorted(res))
        for nm in names:
            assert res[nm]["ScratchSize"] == 0, (k, res[nm])
            assert res[nm]["Occupancy"] >= floor, (k, res[nm])
        seen += len(names)
    assert seen == len(res) == BC_INSTANCES, sorted(res)


@pytest.fixture(scope="module")
def solutions(oracle):
    """the oracle's solution of each of the six problems, computed once"""
    return {name: oracle_solve(oracle, pr, np.array(pr["q"], float), np.array(pr["b"], float), pr["A"], pr["P"], name)
            for name, pr in PROBLEMS}


@pytest.mark.parametrize("name,pr", PROBLEMS, ids=IDS)
def test_unit_cotangents_give_the_rows_of_the_inverse(solutions, name, pr):
    """With gx = e_j the adjoint pair is column j of K^-1, so row j of dx/dq is dq = -K^-1[:n, j]' and row j of dx/db
    is db = K^-1[n:, j]'; with gz = e_i likewise column n + i.  Stacked, the rows are the transposed columns of
    np.linalg.inv of the same dense K: two dense factorisations of one matrix of at most 22 x 22, so the bound is
    rounding, 1e-12 relative.  The rows with respect to P and A are the outer-product formulas on the same pair."""
    out = solutions[name]
    x, s, z = (np.asarray(out[key], dtype=float) for key in "xsz")
    n, m = pr["n"], pr["m"]
    P, A = R.dense(pr)
    K = np.block([[P, A.T], [A, -R.hmat(pr["cones"], s, z)]])
    Kinv = np.linalg.inv(K)
    rows_q, rows_b = np.zeros((n + m, n)), np.zeros((n + m, m))
    worst_mat = 0.0
    for r in range(n + m):
        e = np.zeros(n + m)
        e[r] = 1.0
        dq, db, dP, dA = R.adjoint(pr, x, s, z, gx=e[:n], gz=e[n:])
        rows_q[r], rows_b[r] = dq, db
        vx, vz = Kinv[:n, r], Kinv[n:, r]
        full = -np.outer(vx, x)
        wantP = R.on_pattern(pr["P"], np.triu(full + full.T) - np.diag(np.diag(full)))
        wantA = R.on_pattern(pr["A"], -(np.outer(z, vx) + np.outer(vz, x)))
        worst_mat = max(worst_mat, R.rel(dP, wantP), R.rel(dA, wantA))
    worst = max(R.rel(rows_q, -Kinv[:n, :].T), R.rel(rows_b, Kinv[n:, :].T))
    print(name, "unit cotangents vs transposed columns of inv(K): %.2e (dq, db), %.2e (dP, dA)" % (worst, worst_mat))
    assert worst <= 1e-12, (name, worst)
    assert worst_mat <= 1e-12, (name, worst_mat)
