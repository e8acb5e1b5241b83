"""The batched L4 solver's host side (no GPU needed): the chip_batch_* symbols of both builds, NULL refusals without a
device, the refusal without a device, the stack HipBatchSolver builds, and the spill / occupancy audit of batch.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import e2e_problems as E
from tests.test_solver_host import HIPCC, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH_SYMBOLS = ["chip_batch_create", "chip_batch_destroy", "chip_batch_solve", "chip_batch_get_info",
                 "chip_batch_get_solution", "chip_batch_get_solution_dev", "chip_batch_get_equilibration"]


def member(hip, pr):
    n, m = pr["n"], pr["m"]
    return (hip.CscMatrix(n, n, *pr["P"]), pr["q"], hip.CscMatrix(m, n, *pr["A"]), pr["b"], pr["cones"])


def test_batch_symbols_in_both_builds(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_batch_[a-z_]+)\s*\(", hdr))) == sorted(BATCH_SYMBOLS)
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in BATCH_SYMBOLS:
            assert hasattr(L, sym), (path, sym)
    assert hasattr(C.CDLL(hip.LIB_PATH), "chip_debug_batch_inject_nan")
    assert not hasattr(C.CDLL(hip.SHIP_LIB_PATH), "chip_debug_batch_inject_nan")


def test_null_handles_and_pointers(hip):
    L = hip.lib()
    infos = (hip.SolutionInfo * 1)()
    assert L.chip_batch_solve(None) == hip.ERR_ARG
    assert L.chip_batch_get_info(None, infos) == hip.ERR_ARG
    assert L.chip_batch_get_solution(None, C.c_int64(0), None, None, None, None) == hip.ERR_ARG
    assert L.chip_batch_get_solution_dev(None, None, None, None) == hip.ERR_ARG
    assert L.chip_batch_get_equilibration(None, C.c_int64(0), None, None, None) == hip.ERR_ARG
    L.chip_batch_destroy(None)
    h = C.c_void_p()
    z = np.zeros(4, dtype=np.uint64)
    # nprob = 0, and NULL partition arrays, are refused before any device is looked at
    assert L.chip_batch_create(C.byref(h), C.c_int64(0), None, None, C.c_int64(0), C.c_int64(0), hip._pu(z), None,
                               None, None, hip._pu(z), None, None, None, C.c_int64(0), None, None, None, None, None,
                               None) == hip.ERR_ARG
    assert L.chip_batch_create(None, C.c_int64(1), None, None, C.c_int64(0), C.c_int64(0), hip._pu(z), None, None,
                               None, hip._pu(z), None, None, None, C.c_int64(0), None, None, None, None, None,
                               None) == hip.ERR_ARG


def test_batch_refuses_without_device(hip):
    prs = [member(hip, E.basic_qp()), member(hip, E.basic_lp())]
    with pytest.raises(hip.ChipError) as e:
        hip.HipBatchSolver(prs, hip.SolverSettings.default(device=hip.DEVICE_HOST_ONLY))
    assert e.value.code == hip.ERR_NO_DEVICE
    # the host-side refusals come first: an unsupported cone is refused as such even without a device
    with pytest.raises(hip.ChipError) as e:
        hip.HipBatchSolver(prs + [member(hip, E.basic_expcone())],
                           hip.SolverSettings.default(device=hip.DEVICE_HOST_ONLY))
    assert e.value.code == hip.ERR_UNSUPPORTED


def test_stack_and_partition(hip):
    import scipy.sparse as sp
    prs = [E.basic_qp(), E.basic_lp(), E.basic_socp(), E.basic_unconstrained()]
    st = hip.batch_stack([member(hip, p) for p in prs])
    assert list(st["n_part"]) == [p["n"] for p in prs] and list(st["m_part"]) == [p["m"] for p in prs]
    assert st["n"] == sum(p["n"] for p in prs) and st["m"] == sum(p["m"] for p in prs)
    mats = lambda key, rows: [sp.csc_matrix((p[key][2], p[key][1], p[key][0]), shape=(p[rows], p["n"]))  # noqa: E731
                              for p in prs]
    for key, rows in (("P", "n"), ("A", "m")):
        want = sp.block_diag(mats(key, rows), format="csc")
        got = sp.csc_matrix((st[key][2], st[key][1], st[key][0]), shape=want.shape)
        assert st[key][0].dtype == np.uint64 and st[key][1].dtype == np.uint64
        assert np.array_equal(got.toarray(), want.toarray()), key
    assert np.array_equal(st["q"], np.concatenate([np.asarray(p["q"], float) for p in prs]))
    assert np.array_equal(st["b"], np.concatenate([np.asarray(p["b"], float) for p in prs]))
    assert st["cones"] == [tuple(c) for p in prs for c in p["cones"]]
    with pytest.raises(ValueError):
        hip.batch_stack([(hip.CscMatrix(2, 2, [0, 1, 2], [0, 1], [1.0, 1.0]), [1.0], hip.CscMatrix(0, 2, [0, 0, 0], [], []),
                          [], [])])


# every kernel of batch.hip: no scratch, and the eight waves per SIMD its header comment designs for (256-thread
# workgroups, __launch_bounds__(256), a 16-slot LDS reduction array)
BATCH_KERNELS = ["k_seg_partial", "k_seg_final", "k_cone_items", "k_cone_final", "k_blin", "k_bresid",
                 "k_bunit_shift", "k_bunit_reset", "k_bunscale", "k_beq_norms", "k_beq_factors", "k_beq_scale",
                 "k_beq_cost_final", "k_beq_cost_apply"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_kernels_do_not_spill():
    res = _resources("batch.hip")
    for k in BATCH_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert len(names) == 1, (k, names)
        r = res[names[0]]
        assert r["ScratchSize"] == 0, (k, r)
        assert r["Occupancy"] >= 8, (k, r)
    assert len(res) == len(BATCH_KERNELS), sorted(res)
