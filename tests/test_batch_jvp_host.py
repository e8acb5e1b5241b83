"""The batched solver's forward-mode derivatives, host side (no GPU needed): the chip_bjvp_* symbols of both builds and
the test hook of the test build alone, the refusal of a NULL handle before any device is touched, the formulas of
tests/tangent_ref.py against finite differences of the CPU oracle's interior-point loop and against their transpose
(tests/adjoint_ref.py), the wide QPs, and the spill audit of batch_tangent.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import ipm_driver as ipm
from tests import tangent_ref as T
from tests.test_solver_host import HIPCC, ROOT, _resources

BJVP_SYMBOLS = ["chip_bjvp_apply", "chip_bjvp_apply_dev", "chip_bjvp_get", "chip_bjvp_get_dev"]
HOOK = "chip_debug_batch_jvp_rhs"
PROBLEMS = T.host_problems()
IDS = [n for n, _ in PROBLEMS]


def test_bjvp_symbols_in_both_builds_and_the_hook_in_the_test_build_only(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_bjvp_[a-zA-Z_]+)\s*\(", hdr))) == sorted(BJVP_SYMBOLS)
    assert HOOK not in hdr
    assert HOOK in open(os.path.join(ROOT, "include", "clarabel_hip_testing.h")).read()
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in BJVP_SYMBOLS:
            assert hasattr(L, sym), (path, sym)
    assert hasattr(C.CDLL(hip.LIB_PATH), HOOK)
    assert not hasattr(C.CDLL(hip.SHIP_LIB_PATH), HOOK)


def test_null_handle_is_refused(hip):
    """CHIP_ERR_ARG before any HIP call: these return the same on a machine without a GPU"""
    L = hip.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    valid = (C.c_int32 * 4)()
    p = C.c_void_p()
    assert L.chip_bjvp_apply(None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjvp_apply(None, g, g, g, g) == hip.ERR_ARG
    assert L.chip_bjvp_apply_dev(None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjvp_apply_dev(None, g, None, None, None) == hip.ERR_ARG
    assert L.chip_bjvp_get(None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjvp_get(None, g, g, g, valid) == hip.ERR_ARG
    assert L.chip_bjvp_get_dev(None, None, None, None, None) == hip.ERR_ARG
    assert L.chip_bjvp_get_dev(None, C.byref(p), None, None, None) == hip.ERR_ARG
    assert L.chip_debug_batch_jvp_rhs(None, g, g, valid, g, g, g, g, g, g) == hip.ERR_ARG
    assert p.value is None and list(valid) == [0, 0, 0, 0] and list(g) == [1.0, 2.0, 3.0, 4.0]


def oracle_solve(oracle, pr, q, b, A, P, name):
    be = ipm.OracleBackend(oracle, pr["n"], pr["m"], P, A, q, b, pr["cones"])
    out = ipm.solve(be, pr["cones"], q, b)
    assert out["status"] == "Solved", (name, out["status"])
    return out


@pytest.fixture(scope="module")
def solutions(oracle):
    """the oracle's solution of each of the nine problems, computed once"""
    return {name: oracle_solve(oracle, pr, np.array(pr["q"], float), np.array(pr["b"], float), pr["A"], pr["P"], name)
            for name, pr in PROBLEMS}


@pytest.mark.parametrize("name,pr", PROBLEMS, ids=IDS)
def test_tangent_ref_against_finite_differences(oracle, solutions, name, pr):
    """tangent_ref.tangent against central differences (h = 1e-4) of the oracle loop along ONE random direction in q,
    b, P and A at once (two oracle solves).  Bound 1e-4 relative, the finite-difference bound of
    tests/test_batch_adjoint_host.py: the error is the noise of a loop that stops at 1e-8, not the formula (the worst
    measured when the formulas were derived: 1.5e-6, random_qp_2's s)."""
    out = solutions[name]
    dq, db, dP, dA = T.direction(pr, 31)
    want = T.tangent(pr, out["x"], out["s"], out["z"], dq, db, dP, dA)
    h = 1e-4
    side = []
    for sgn in (1.0, -1.0):
        P = (pr["P"][0], pr["P"][1], np.array(pr["P"][2], float) + sgn * h * dP)
        A = (pr["A"][0], pr["A"][1], np.array(pr["A"][2], float) + sgn * h * dA)
        side.append(oracle_solve(oracle, pr, np.array(pr["q"], float) + sgn * h * dq,
                                 np.array(pr["b"], float) + sgn * h * db, A, P, name))
    errs = {}
    for key, w in zip("xzs", want):
        fd = (np.asarray(side[0][key]) - np.asarray(side[1][key])) / (2 * h)
        errs[key] = R.rel(w, fd)
    print(name, " ".join("d%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1e-4, (name, errs)


@pytest.mark.parametrize("name,pr", PROBLEMS, ids=IDS)
def test_tangent_ref_is_the_transpose_of_adjoint_ref(solutions, name, pr):
    """g.(dx, dz, ds) = (dL/dq, dL/db, dL/dP, dL/dA).d for random g and d: two dense solves with one matrix of at most
    93 x 93, so the bound is rounding, 1e-12 on |lhs - rhs| / max(1, |lhs|) (measured: 1.4e-14 at worst)"""
    out = solutions[name]
    x, s, z = out["x"], out["s"], out["z"]
    d = T.direction(pr, 41)
    g = R.incoming(pr, 43)
    dx, dz, ds = T.tangent(pr, x, s, z, *d)
    grads = R.adjoint(pr, x, s, z, *g)
    lhs = float(g[0] @ dx + g[1] @ dz + g[2] @ ds)
    rhs = float(sum(a @ b for a, b in zip(grads, d)))
    err = abs(lhs - rhs) / max(1.0, abs(lhs))
    print(name, "duality %.2e" % err)
    assert err <= 1e-12, (name, lhs, rhs)
    nn = T.nn_rows(pr)
    assert np.all(ds[~nn] == 0.0) and not np.any(np.signbit(ds[~nn]))


def test_wide_qps_are_strictly_complementary(solutions):
    """the three wide QPs end Solved with some but not all inequalities active and min(s_i + z_i) well away from 0:
    their derivative is well defined.  Their dense rows are longer than a wavefront."""
    for seed in (1, 2, 3):
        pr = T.wide_qp(seed)
        P, A = R.dense(pr)
        assert np.count_nonzero(A[0]) == np.count_nonzero(A[3]) == np.count_nonzero(P[0]) == 70 > 64
        assert np.count_nonzero(A[:, 5]) == 23
        out = solutions["wide_qp_%d" % seed]
        s, z = out["s"][3:], out["z"][3:]
        active = int(np.sum(s < 1e-6))
        print("wide_qp(%d): %d of 20 active, min(s + z) %.2e" % (seed, active, float(np.min(s + z))))
        assert 0 < active < 20, (seed, active)
        assert float(np.min(s + z)) >= 4.5e-2, (seed, float(np.min(s + z)))


# every kernel of batch_tangent.hip: no scratch (k_bt_rhs holds 33 pointers: its occupancy is bounded by scalar
# registers, not asserted here)
BT_KERNELS = ["k_bt_rhs", "k_bt_out"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_tangent_kernels_do_not_spill():
    res = _resources("batch_tangent.hip")
    seen = 0
    for k in BT_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert names, (k, sorted(res))
        for nm in names:
            r = res[nm]
            assert r["ScratchSize"] == 0, (k, r)
        seen += len(names)
    assert seen == len(res), sorted(res)
