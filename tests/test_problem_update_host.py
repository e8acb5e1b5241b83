"""The L4 data updates' host side (no GPU needed): the chip_problem_* symbols of both builds, the header's unchanged
chip_solver_* list, the refusal of a NULL handle or pointer before any device is touched, the Python classifier of
the update forms, and the occupancy audit of problem_update.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_solver_host import HIPCC, ROOT, SOLVER_SYMBOLS, _resources

PROBLEM_SYMBOLS = ["chip_problem_update_P", "chip_problem_update_A", "chip_problem_update_q", "chip_problem_update_b",
                   "chip_problem_update_P_dev", "chip_problem_update_A_dev", "chip_problem_update_q_dev",
                   "chip_problem_update_b_dev", "chip_problem_update_settings", "chip_problem_update_allowed",
                   "chip_problem_get_scaled"]


def _header():
    return open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()


def test_problem_symbols_in_both_builds(hip):
    declared = sorted(set(re.findall(r"\b(chip_problem_[a-zA-Z_]+)\s*\(", _header())))
    assert declared == sorted(PROBLEM_SYMBOLS)
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in PROBLEM_SYMBOLS:
            assert hasattr(L, sym), (path, sym)


def test_no_new_solver_symbols():
    declared = sorted(set(re.findall(r"\b(chip_solver_[a-z_]+)\s*\(", _header())))
    assert declared == sorted(SOLVER_SYMBOLS)


def test_null_handle_or_pointer_is_refused(hip):
    """CHIP_ERR_ARG before any HIP call: these return the same on a machine without a GPU"""
    L = hip.lib()
    vals = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    idx = (C.c_uint64 * 4)(0, 1, 2, 3)
    for key in "PAqb":
        fn = getattr(L, "chip_problem_update_" + key)
        assert fn(None, None, vals, C.c_int64(4)) == hip.ERR_ARG
        assert fn(None, idx, vals, C.c_int64(4)) == hip.ERR_ARG
        assert fn(None, None, None, C.c_int64(0)) == hip.ERR_ARG
        fd = getattr(L, "chip_problem_update_%s_dev" % key)
        assert fd(None, None, vals, C.c_int64(4)) == hip.ERR_ARG
    s = hip.SolverSettings.default()
    assert L.chip_problem_update_settings(None, C.byref(s)) == hip.ERR_ARG
    allowed = C.c_int32(7)
    assert L.chip_problem_update_allowed(None, C.byref(allowed)) == hip.ERR_ARG
    assert allowed.value == 7
    assert L.chip_problem_get_scaled(None, None, None, None, None) == hip.ERR_ARG


def _pattern(hip):
    # 3 x 3 triu P with 4 entries
    P = hip.CscMatrix(3, 3, [0, 1, 2, 4], [0, 1, 0, 2], [1.0, 2.0, 0.5, 3.0])
    return P, (P.m, P.n, P.colptr.copy(), P.rowval.copy())


def test_classify_accepts_every_form(hip):
    P, pat = _pattern(hip)
    cl = hip.classify_update
    assert cl("P", None, 4, pat) == ("none",)
    assert cl("P", [], 4, pat) == ("none",)
    assert cl("q", np.zeros(0), 3) == ("none",)
    assert cl("q", ([], []), 3) == ("none",)
    kind, idx, vals = cl("P", hip.CscMatrix(3, 3, P.colptr, P.rowval, [4.0, 3.0, 2.0, 1.0]), 4, pat)
    assert kind == "full" and idx is None and vals.dtype == np.float64 and list(vals) == [4.0, 3.0, 2.0, 1.0]
    kind, idx, vals = cl("A", [1, 2, 3, 4], 4, pat)  # integers are real values
    assert kind == "full" and vals.dtype == np.float64
    kind, idx, vals = cl("q", ([2, 0, 2], [1.0, 2.0, 3.0]), 3)
    assert kind == "partial" and idx.dtype == np.uint64 and list(idx) == [2, 0, 2] and list(vals) == [1.0, 2.0, 3.0]
    kind, idx, vals = cl("b", (np.array([1], dtype=np.int32), np.array([5.0], dtype=np.float32)), 3)
    assert kind == "partial" and list(idx) == [1] and vals.dtype == np.float64
    # a negative host index is passed on as out of range (the library refuses it, nothing written)
    kind, idx, vals = cl("b", ([-1], [5.0]), 3)
    assert kind == "partial" and int(idx[0]) >= 3


def test_classify_refuses_bad_forms(hip):
    P, pat = _pattern(hip)
    cl = hip.classify_update
    # check_equal_sparsity: another pattern (rowval, colptr or shape) is IncompatibleDimension
    for other in (hip.CscMatrix(3, 3, [0, 1, 2, 4], [0, 1, 1, 2], [1.0] * 4),
                  hip.CscMatrix(3, 3, [0, 1, 3, 4], [0, 0, 1, 2], [1.0] * 4),
                  hip.CscMatrix(4, 3, [0, 1, 2, 4], [0, 1, 0, 2], [1.0] * 4)):
        with pytest.raises(hip.ChipError) as e:
            cl("P", other, 4, pat)
        assert e.value.code == hip.ERR_DIM
    for bad in ([1.0, 2.0, 3.0], np.ones(5)):  # a full vector of the wrong length
        with pytest.raises(hip.ChipError) as e:
            cl("P", bad, 4, pat)
        assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:
        cl("q", ([0, 1], [1.0]), 3)  # index / value count mismatch
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:
        cl("q", np.ones((3, 1)), 3)
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(TypeError):
        cl("q", ([0.0, 1.0], [1.0, 2.0]), 3)  # float indices
    with pytest.raises(TypeError):
        cl("q", np.array([1 + 2j, 0, 0]), 3)  # complex values
    with pytest.raises(TypeError):
        cl("b", np.array(["a", "b", "c"]), 3)
    with pytest.raises(TypeError):
        cl("q", P, 3)  # a matrix for a vector
    with pytest.raises(TypeError):
        cl("q", ([0], [1.0], [2.0]), 3)


def test_classify_torch_forms(hip):
    torch = pytest.importorskip("torch")
    P, pat = _pattern(hip)
    cl = hip.classify_update
    # CPU tensors are host arrays
    kind, idx, vals = cl("q", (torch.tensor([2, 1]), torch.tensor([1.0, 2.0], dtype=torch.float64)), 3)
    assert kind == "partial" and list(idx) == [2, 1] and list(vals) == [1.0, 2.0]
    kind, _, vals = cl("P", torch.arange(4, dtype=torch.float32), 4, pat)
    assert kind == "full" and vals.dtype == np.float64
    kind, idx, vals = cl("b", (np.array([0]), torch.zeros(1, dtype=torch.float64)), 3)
    assert kind == "partial" and list(idx) == [0]


PU_KERNELS = ["k_pu_validate", "k_pu_full_mat", "k_pu_full_vec", "k_pu_claim", "k_pu_write", "k_pu_release",
              "k_pu_scatter", "k_pu_norm_partial", "k_pu_norm_final"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_problem_update_kernels_do_not_spill():
    res = _resources("problem_update.hip")
    seen = 0
    for k in PU_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert names, (k, sorted(res))
        for nm in names:
            r = res[nm]
            assert r["ScratchSize"] == 0, (k, r)
            assert r["Occupancy"] >= 8, (k, r)
        seen += len(names)
    assert seen == len(res), sorted(res)
