"""Re-equilibration of a live handle, host side (no GPU needed): the four entry points in both builds and the test
hooks in the test build only, the refusal of a NULL handle before any device is touched, what HipSolver.reequilibrate /
HipBatchSolver.reequilibrate refuse before they call the library, and the spill / occupancy audit of reequilibrate.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import e2e_problems as E
from tests.test_solver_host import HIPCC, ROOT, _resources

SYMBOLS = ["chip_reequilibrate_problem", "chip_reequilibrate_problem_dev", "chip_reequilibrate_bdata",
           "chip_reequilibrate_bdata_dev"]
HOOKS = ["chip_debug_reload_pass", "chip_debug_create_count"]


def test_symbols_in_both_builds_and_the_hooks_in_the_test_build_only(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_reequilibrate_[a-zA-Z_]+)\s*\(", hdr))) == sorted(SYMBOLS)
    testing = open(os.path.join(ROOT, "include", "clarabel_hip_testing.h")).read()
    for hook in HOOKS:
        assert hook not in hdr and hook in testing
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in SYMBOLS:
            assert hasattr(L, sym), (path, sym)
    ship, test = C.CDLL(hip.SHIP_LIB_PATH), C.CDLL(hip.LIB_PATH)
    for hook in HOOKS:
        assert hasattr(test, hook) and not hasattr(ship, hook), hook


def test_null_handle_is_refused(hip):
    """CHIP_ERR_ARG before any HIP call: the same on a machine without a GPU"""
    L = hip.lib()
    v = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    for sym in SYMBOLS:
        assert getattr(L, sym)(None, v, v, v, v) == hip.ERR_ARG, sym
        assert getattr(L, sym)(None, None, None, None, None) == hip.ERR_ARG, sym
    out = C.c_double()
    assert L.chip_debug_create_count(C.c_int32(2), C.byref(out)) == hip.ERR_ARG
    assert L.chip_debug_create_count(C.c_int32(0), None) == hip.ERR_ARG
    assert L.chip_debug_reload_pass(None, None, v, C.c_int64(4), C.c_int32(0), C.c_int32(0)) == hip.ERR_ARG
    assert L.chip_debug_reload_pass(v, None, v, C.c_int64(-1), C.c_int32(0), C.c_int32(0)) == hip.ERR_ARG
    assert L.chip_debug_reload_pass(v, None, v, C.c_int64(0), C.c_int32(0), C.c_int32(8)) == hip.ERR_ARG


def _handle_without_a_device(hip):
    """a HipBatchSolver as its constructor leaves it, minus the C handle: what reequilibrate() classifies against"""
    prs = [E.basic_lp(), E.basic_qp(), E.basic_socp()]
    mem = [(hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"], p["cones"])
           for p in prs]
    st = hip.batch_stack(mem)
    b = object.__new__(hip.HipBatchSolver)
    n, m = st["n"], st["m"]
    b.stack, b.n_part, b.m_part, b.generation, b._h = st, st["n_part"], st["m_part"], 0, None
    b._len = {"P": len(st["P"][2]), "A": len(st["A"][2]), "q": n, "b": m}
    b._pattern = {"P": (n, n, st["P"][0], st["P"][1]), "A": (m, n, st["A"][0], st["A"][1])}
    part = {"P": [x[0].nnz for x in mem], "A": [x[2].nnz for x in mem], "q": b.n_part, "b": b.m_part}
    b._offsets = {k: np.concatenate([[0], np.cumsum(np.asarray(v, dtype=np.int64))]).astype(np.int64)
                  for k, v in part.items()}
    b._mpattern = {"P": [(x[0].m, x[0].n, x[0].colptr.copy(), x[0].rowval.copy()) for x in mem],
                   "A": [(x[2].m, x[2].n, x[2].colptr.copy(), x[2].rowval.copy()) for x in mem]}
    return b, st, mem


def test_python_refuses_before_any_c_call(hip, monkeypatch):
    b, st, mem = _handle_without_a_device(hip)
    n, m = st["n"], st["m"]
    good = dict(P=st["P"][2].copy(), q=st["q"].copy(), A=st["A"][2].copy(), b=st["b"].copy())

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(hip, "lib", no_library)
    for key in "PqAb":  # a wrong length
        bad = dict(good)
        bad[key] = np.ones(len(good[key]) + 1)
        with pytest.raises(hip.ChipError) as e:
            b.reequilibrate(**bad)
        assert e.value.code == hip.ERR_DIM, key
        bad[key] = np.ones(0)  # (what an update takes as a no-op)
        with pytest.raises(hip.ChipError) as e:
            b.reequilibrate(**bad)
        assert e.value.code == hip.ERR_DIM, key
        bad[key] = None
        with pytest.raises(TypeError):
            b.reequilibrate(**bad)
        bad[key] = (np.array([0]), np.array([1.0]))  # a partial form
        with pytest.raises(TypeError):
            b.reequilibrate(**bad)
    # a scipy matrix with another pattern (A's first stored entry moved to another row of its column)
    Ap, Ai, Ax = st["A"]
    A = sp.csc_matrix((Ax, Ai.astype(np.int64), Ap.astype(np.int64)), shape=(m, n))
    col0 = set(int(r) for r in Ai[:int(Ap[1])])
    Ai2 = Ai.astype(np.int64)
    Ai2[0] = next(r for r in range(int(st["m_part"][0])) if r not in col0)
    other = sp.csc_matrix((Ax, Ai2, Ap.astype(np.int64)), shape=(m, n))
    with pytest.raises(hip.ChipError) as e:
        b.reequilibrate(**dict(good, A=other))
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:  # member 1's matrix in member 0's place of the list form
        b.reequilibrate(**dict(good, P=[mem[1][0], mem[1][0], mem[2][0]]))
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:  # two list entries for three members
        b.reequilibrate(**dict(good, q=[np.ones(3), np.ones(2)]))
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(TypeError):  # a list that leaves a member out is not the full data
        b.reequilibrate(**dict(good, q=[np.ones(3), None, np.ones(3)]))
    # what passes the classifier reaches the library (here: the stand-in), so the refusals above came before it
    for ok in (good, dict(good, A=A), dict(good, q=[np.ones(int(k)) for k in st["n_part"]])):
        with pytest.raises(AssertionError, match="the library was called"):
            b.reequilibrate(**ok)
    assert b.generation == 0


def test_python_refuses_a_mix_of_host_and_device_tensors(hip, monkeypatch):
    """a GPU tensor is recognised by its type, so a stand-in with the same surface classifies without a device"""
    b, st, _ = _handle_without_a_device(hip)
    import torch

    class OnGpu(torch.Tensor):
        is_cuda = True
    OnGpu.__module__ = "torch"

    def fake(v):
        return torch.as_tensor(np.asarray(v, dtype=np.float64)).as_subclass(OnGpu)

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(hip, "lib", no_library)
    good = dict(P=st["P"][2].copy(), q=st["q"].copy(), A=st["A"][2].copy(), b=st["b"].copy())
    for key in "PqAb":
        with pytest.raises(TypeError, match="all be host arrays or all GPU tensors"):
            b.reequilibrate(**dict(good, **{key: fake(good[key])}))
    with pytest.raises(hip.ChipError) as e:  # a GPU tensor of the wrong length
        b.reequilibrate(**dict({k: fake(v) for k, v in good.items()}, q=fake(np.ones(len(good["q"]) + 1))))
    assert e.value.code == hip.ERR_DIM


# every kernel of reequilibrate.hip: no scratch, eight waves per SIMD (256-thread workgroups, streaming passes)
RE_KERNELS = ["k_re_load", "k_re_absmax_partial", "k_re_absmax_final"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_reequilibrate_kernels_do_not_spill():
    res = _resources("reequilibrate.hip")
    seen = 0
    for k in RE_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert names, (k, sorted(res))
        for nm in names:
            r = res[nm]
            assert r["ScratchSize"] == 0, (k, r)
            assert r["Occupancy"] >= 8, (k, r)
        seen += len(names)
    assert seen == len(res) and seen == 8 + 2, sorted(res)  # (the load pass: 16-byte or not, capped or not, raw or not)
