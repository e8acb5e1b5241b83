"""The batched solver's data updates, host side (no GPU needed): the chip_bdata_* symbols of both builds, the refusal
of a NULL handle or pointer before any device is touched, the translation of the per-member list form into stack
positions, and the spill / occupancy audit of batch_update.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import e2e_problems as E
from tests.test_solver_host import HIPCC, ROOT, _resources

BDATA_SYMBOLS = ["chip_bdata_update_P", "chip_bdata_update_A", "chip_bdata_update_q", "chip_bdata_update_b",
                 "chip_bdata_update_P_dev", "chip_bdata_update_A_dev", "chip_bdata_update_q_dev",
                 "chip_bdata_update_b_dev", "chip_bdata_update_settings", "chip_bdata_get_scaled"]


def test_bdata_symbols_in_both_builds(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_bdata_[a-zA-Z_]+)\s*\(", hdr))) == sorted(BDATA_SYMBOLS)
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in BDATA_SYMBOLS:
            assert hasattr(L, sym), (path, sym)


def test_null_handle_or_pointer_is_refused(hip):
    """CHIP_ERR_ARG before any HIP call: these return the same on a machine without a GPU"""
    L = hip.lib()
    vals = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    idx = (C.c_uint64 * 4)(0, 1, 2, 3)
    for key in "PAqb":
        fn = getattr(L, "chip_bdata_update_" + key)
        assert fn(None, None, vals, C.c_int64(4)) == hip.ERR_ARG
        assert fn(None, idx, vals, C.c_int64(4)) == hip.ERR_ARG
        assert fn(None, None, None, C.c_int64(0)) == hip.ERR_ARG
        assert fn(None, None, vals, C.c_int64(-1)) == hip.ERR_ARG
        fd = getattr(L, "chip_bdata_update_%s_dev" % key)
        assert fd(None, None, vals, C.c_int64(4)) == hip.ERR_ARG
        assert fd(None, None, None, C.c_int64(4)) == hip.ERR_ARG
        assert fd(None, None, vals, C.c_int64(-1)) == hip.ERR_ARG
    s = hip.SolverSettings.default()
    assert L.chip_bdata_update_settings(None, C.byref(s)) == hip.ERR_ARG
    assert L.chip_bdata_get_scaled(None, None, None, None, None, None, None) == hip.ERR_ARG


def _members(hip):
    prs = [E.basic_qp(), E.basic_lp(), E.basic_socp(), E.basic_unconstrained()]
    return prs, [(hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"],
                  p["cones"]) for p in prs]


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def test_list_form_translates_to_stack_positions(hip):
    prs, mem = _members(hip)
    st = hip.batch_stack(mem)
    rng = np.random.default_rng(2)
    for key, counts in (("q", [p["n"] for p in prs]), ("b", [p["m"] for p in prs]),
                        ("P", [len(p["P"][2]) for p in prs]), ("A", [len(p["A"][2]) for p in prs])):
        off = _offsets(counts)
        pats = None
        if key in "PA":
            j = 0 if key == "P" else 2
            pats = [(m_[j].m, m_[j].n, m_[j].colptr, m_[j].rowval) for m_ in mem]
        # member 0: a full vector; member 1: untouched; member 2: member-local (index, values) with a repeat;
        # member 3: an empty vector (a no-op)
        v0 = rng.standard_normal(counts[0])
        i2 = np.array([counts[2] - 1, 0, counts[2] - 1])
        v2 = np.array([1.0, 2.0, 3.0])
        kind, idx, vals = hip.batch_list_update(key, [v0, None, (i2, v2), []], off, pats)
        assert kind == "partial" and idx.dtype == np.uint64 and vals.dtype == np.float64
        # the numpy restatement: positions in the stacked vector, members in order
        want_idx = np.concatenate([off[0] + np.arange(counts[0]), off[2] + i2])
        assert np.array_equal(idx, want_idx.astype(np.uint64)), key
        assert np.array_equal(vals, np.concatenate([v0, v2])), key
        # applied in order (the last occurrence wins) it changes exactly those members' entries of the stack
        stacked = np.array(st[key][2] if key in "PA" else st[key], dtype=float)
        want = stacked.copy()
        want[off[0]:off[1]] = v0
        for i, v in zip(i2, v2):
            want[off[2] + i] = v
        got = stacked.copy()
        for i, v in zip(idx, vals):
            got[int(i)] = v
        assert np.array_equal(got, want), key
        assert hip.batch_list_update(key, [None, None, [], ([], [])], off, pats) == ("none",)
    # a member's matrix with its own pattern is a full vector of that member
    kind, idx, vals = hip.batch_list_update("P", [None, None, mem[2][0], None], _offsets([len(p["P"][2]) for p in prs]),
                                            [(m_[0].m, m_[0].n, m_[0].colptr, m_[0].rowval) for m_ in mem])
    o = _offsets([len(p["P"][2]) for p in prs])
    assert kind == "partial" and np.array_equal(idx, np.arange(o[2], o[3]).astype(np.uint64))
    assert np.array_equal(vals, mem[2][0].nzval)


def test_list_form_refuses_wrong_lengths(hip):
    prs, mem = _members(hip)
    off = _offsets([p["n"] for p in prs])
    bl = hip.batch_list_update
    with pytest.raises(hip.ChipError) as e:  # three entries for four members
        bl("q", [None, None, None], off)
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:  # a member's vector of another member's length
        bl("q", [np.ones(prs[0]["n"] + 1), None, None, None], off)
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:  # index / value count mismatch
        bl("q", [None, ([0, 1], [1.0]), None, None], off)
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:  # a member-local index must not reach the next member
        bl("q", [([prs[0]["n"]], [1.0]), None, None, None], off)
    assert e.value.code == hip.ERR_DIM
    with pytest.raises(hip.ChipError) as e:
        bl("q", [None, ([-1], [1.0]), None, None], off)
    assert e.value.code == hip.ERR_DIM
    pats = [(m_[0].m, m_[0].n, m_[0].colptr, m_[0].rowval) for m_ in mem]
    with pytest.raises(hip.ChipError) as e:  # member 0's matrix handed to member 2
        bl("P", [None, None, mem[0][0], None], _offsets([len(p["P"][2]) for p in prs]), pats)
    assert e.value.code == hip.ERR_DIM


# every kernel of batch_update.hip: no scratch, eight waves per SIMD (256-thread workgroups, streaming passes)
BU_KERNELS = ["k_bu_full_mat", "k_bu_full_vec", "k_bu_claim", "k_bu_write", "k_bu_release", "k_bu_norm_partial",
              "k_bu_norm_final"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_update_kernels_do_not_spill():
    res = _resources("batch_update.hip")
    seen = 0
    for k in BU_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert names, (k, sorted(res))
        for nm in names:
            r = res[nm]
            assert r["ScratchSize"] == 0, (k, r)
            assert r["Occupancy"] >= 8, (k, r)
        seen += len(names)
    assert seen == len(res), sorted(res)
