"""The batched solver's PSD members, host side (no GPU needed): chip_bsym_create in both builds, its refusals without
a device (bad arguments, Exponential / Power / GenPower cones, presolve and chordal decomposition, a PSD cone across
two members), the old entry points that keep refusing a PSD cone, the plan's PSD arrays from the sibling debug hook
chip_debug_bsymplan_create (host_plan_build, csrc/batch.cpp), and the resource audit of batch_psd.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import e2e_problems as E
from tests.test_create_refusals_host import raw_batch_create
from tests.test_solver_host import HIPCC, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO, NN, SOC, EXP, POW, GENPOW, PSD = range(7)
ONLY = "chip_bsym_create: only Zero, Nonnegative, SecondOrder and PSDTriangle cones"


def member(hip, pr):
    n, m = pr["n"], pr["m"]
    return (hip.CscMatrix(n, n, *pr["P"]), pr["q"], hip.CscMatrix(m, n, *pr["A"]), pr["b"], pr["cones"])


def raw_bsym_create(hip, st, n_part, m_part, cones=None, settings=None, nprob=None, null_out=False):
    """tests/test_create_refusals_host.py::raw_batch_create for chip_bsym_create: the same argument list"""
    Pp, Pi, Px = st["P"]
    Ap, Ai, Ax = st["A"]
    tags, dims, dims2, alphas = hip._cone_arrays(cones if cones is not None else st["cones"])
    n_part = np.asarray(n_part, dtype=np.int64)
    m_part = np.asarray(m_part, dtype=np.int64)
    h = C.c_void_p()
    s = settings if settings is not None else hip.SolverSettings.default()
    rc = hip.lib().chip_bsym_create(None if null_out else C.byref(h),
                                    C.c_int64(len(n_part) if nprob is None else nprob), n_part.ctypes.data_as(hip.P_I64),
                                    m_part.ctypes.data_as(hip.P_I64), C.c_int64(st["n"]), C.c_int64(st["m"]),
                                    hip._pu(Pp), hip._pu(Pi), hip._pf(Px), hip._pf(st["q"]), hip._pu(Ap), hip._pu(Ai),
                                    hip._pf(Ax), hip._pf(st["b"]), C.c_int64(len(tags)), tags.ctypes.data_as(hip.P_I32),
                                    dims.ctypes.data_as(hip.P_I64), dims2.ctypes.data_as(hip.P_I64), hip._pf(alphas),
                                    None, C.byref(s))
    if rc == 0:
        hip.lib().chip_batch_destroy(h)
    return rc


def _refused(hip, code, text, *args, **kw):
    assert raw_bsym_create(hip, *args, **kw) == code
    assert hip.lib().chip_last_error().decode() == text


@pytest.fixture(scope="module")
def stack(hip):
    """basic_sdp (n = 6, one PSD(3) = 6 rows) and basic_qp (n = 2, NN(3), NN(3))"""
    st = hip.batch_stack([member(hip, E.basic_sdp()), member(hip, E.basic_qp())])
    assert (st["n"], st["m"]) == (8, 12) and st["cones"] == [(PSD, 3), (NN, 3), (NN, 3)]
    return st


# ---- 1. the symbols ------------------------------------------------------------------------------------------------
def test_symbols_in_both_builds(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert sorted(set(re.findall(r"\b(chip_bsym_[a-z_]+)\s*\(", hdr))) == ["chip_bsym_create"]
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        assert hasattr(C.CDLL(path), "chip_bsym_create"), path
    assert hasattr(C.CDLL(hip.LIB_PATH), "chip_debug_bsymplan_create")
    assert not hasattr(C.CDLL(hip.SHIP_LIB_PATH), "chip_debug_bsymplan_create")


# ---- 2. refusals that need no device --------------------------------------------------------------------------------
def test_bad_arguments(hip, stack):
    bad = "chip_bsym_create: bad argument"
    _refused(hip, hip.ERR_ARG, bad, stack, [6, 2], [6, 6], null_out=True)
    _refused(hip, hip.ERR_ARG, bad, stack, [6, 2], [6, 6], nprob=0)
    h = C.c_void_p()
    z = np.zeros(4, dtype=np.uint64)
    L = hip.lib()
    assert L.chip_bsym_create(C.byref(h), C.c_int64(1), None, None, C.c_int64(0), C.c_int64(0), hip._pu(z), None, None,
                              None, hip._pu(z), None, None, None, C.c_int64(0), None, None, None, None, None,
                              None) == hip.ERR_ARG
    assert not h.value
    _refused(hip, hip.ERR_ARG, "chip_bsym_create: negative part", stack, [-1, 9], [6, 6])
    _refused(hip, hip.ERR_ARG, "chip_bsym_create: the parts do not add up to n, m", stack, [6, 2], [6, 5])


@pytest.mark.parametrize("cone", [(EXP, 3), (POW, 3, 0, 0.5), (GENPOW, 2, 1, [0.6, 0.4])], ids=["exp", "pow", "genpow"])
def test_refuses_nonsymmetric_cones(hip, stack, cone):
    _refused(hip, hip.ERR_UNSUPPORTED, ONLY, stack, [6, 2], [6, 6], cones=[(PSD, 3), (NN, 3), cone])


@pytest.mark.parametrize("field", ["presolve_enable", "chordal_decomposition_enable"])
def test_refuses_transforms(hip, stack, field):
    text = "chip_bsym_create: presolve and chordal decomposition are not supported"
    _refused(hip, hip.ERR_UNSUPPORTED, text, stack, [6, 2], [6, 6], settings=hip.SolverSettings.default(**{field: 1}))
    # the settings are looked at before the cones and the partition, as chip_batch_create does
    _refused(hip, hip.ERR_UNSUPPORTED, text, stack, [6, 2], [6, 5], cones=[(PSD, 3), (NN, 3), (EXP, 3)],
             settings=hip.SolverSettings.default(**{field: 1}))


def test_refuses_a_psd_cone_across_two_members(hip):
    crosses = "chip_bsym_create: a cone crosses a member's rows"
    # two members with diagonal A, so that no entry of A crosses when the rows are split elsewhere: member 0 is
    # basic_sdp without its last row, member 1 one Nonnegative row more -- and the cones still say PSD(3), NN(1)
    I5 = E._csc(np.eye(5))
    a = dict(n=5, m=5, P=E._triu(np.eye(5)), A=I5, q=[0.0] * 5, b=[1.0] * 5, cones=[(NN, 5)])
    b = dict(n=2, m=2, P=E._triu(np.eye(2)), A=E._csc(np.eye(2)), q=[0.0] * 2, b=[1.0] * 2, cones=[(NN, 2)])
    st = hip.batch_stack([member(hip, a), member(hip, b)])
    _refused(hip, hip.ERR_ARG, crosses, st, [5, 2], [5, 2], cones=[(PSD, 3), (NN, 1)])
    _refused(hip, hip.ERR_ARG, crosses, st, [5, 2], [5, 2], cones=[(NN, 4), (PSD, 2)])
    # the same cones inside the members are taken as far as the device
    rc = raw_bsym_create(hip, st, [5, 2], [5, 2], cones=[(NN, 2), (PSD, 2), (PSD, 1), (NN, 1)])
    assert rc == (0 if hip.device_count() > 0 else hip.ERR_NO_DEVICE)
    # a refused cone is reported only after the entries were checked (rows split inside member 0's A block)
    _refused(hip, hip.ERR_ARG, "chip_bsym_create: an entry of A crosses two members' blocks", st, [5, 2], [4, 3],
             cones=[(PSD, 3), (NN, 1)])


def test_accepted_members_ask_for_a_device(hip):
    """a PSD member passes every host check of the new entry; without a device that is where it stops"""
    prs = [member(hip, E.basic_sdp()), member(hip, E.basic_socp()), member(hip, E.basic_lp())]
    with pytest.raises(hip.ChipError) as e:
        hip.HipBatchSolver(prs, hip.SolverSettings.default(device=hip.DEVICE_HOST_ONLY), cones="symmetric")
    assert e.value.code == hip.ERR_NO_DEVICE
    assert hip.lib().chip_last_error().decode() == "chip_bsym_create: no HIP device (the product has no CPU fallback)"
    with pytest.raises(hip.ChipError) as e:
        hip.HipBatchSolver(prs + [member(hip, E.basic_expcone())],
                           hip.SolverSettings.default(device=hip.DEVICE_HOST_ONLY), cones="symmetric")
    assert e.value.code == hip.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        hip.HipBatchSolver(prs, cones="all")


# ---- 3. the old entry points keep refusing ------------------------------------------------------------------------
def test_old_entries_still_refuse_psd(hip, stack):
    assert raw_batch_create(hip, stack, [6, 2], [6, 6]) == hip.ERR_UNSUPPORTED
    assert hip.lib().chip_last_error().decode() == "chip_batch_create: only Zero, Nonnegative and SecondOrder cones"
    with pytest.raises(hip.ChipError) as e:  # the default of HipBatchSolver is the old entry
        hip.HipBatchSolver([member(hip, E.basic_sdp())], hip.SolverSettings.default(device=hip.DEVICE_HOST_ONLY))
    assert e.value.code == hip.ERR_UNSUPPORTED
    with pytest.raises(hip.ChipError) as e:
        hip.BatchPlanDebug([6, 2], [6, 6], [(PSD, 3), (NN, 6)])
    assert e.value.code == hip.ERR_UNSUPPORTED
    with pytest.raises(hip.ChipError) as e:
        hip.BatchPlanDebug([6, 2], [6, 6], [(PSD, 3), (EXP, 3), (NN, 3)], symmetric=True)
    assert e.value.code == hip.ERR_UNSUPPORTED
    assert hip.lib().chip_last_error().decode() == ONLY
    L = hip.lib()
    assert L.chip_debug_bsymplan_create(None, C.c_int64(1), None, None, C.c_int64(0), None, None) == hip.ERR_ARG


# ---- 4. the plan -----------------------------------------------------------------------------------------------------
def tri(n):
    return n * (n + 1) // 2


def expected(m_part, cones):
    """the PSD arrays restated from the sizes alone"""
    zoff = np.concatenate([[0], np.cumsum(m_part)])
    owner = lambda r: int(np.searchsorted(zoff, r, side="right") - 1)  # noqa: E731
    out = dict(psd_mem=[], psd_start=[], psd_dim=[], psd_view=[], psd_diag=[], degree=[0] * len(m_part),
               rtype=[0] * int(zoff[-1]))
    row = view = 0
    for c in cones:
        tag, dim = c[0], c[1]
        rows = tri(dim) if tag == PSD else dim
        if rows:
            k = owner(row)
            if tag == NN:
                out["degree"][k] += dim
                out["rtype"][row:row + rows] = [1] * rows
            elif tag == SOC:
                out["degree"][k] += 1
                out["rtype"][row:row + rows] = [2] + [3] * (rows - 1)
            elif tag == PSD:
                out["degree"][k] += dim
                out["rtype"][row:row + rows] = [4] * rows
                out["psd_mem"].append(k)
                out["psd_start"].append(row)
                out["psd_dim"].append(dim)
                out["psd_view"].append(view)
                out["psd_diag"] += [row + tri(j) + j for j in range(dim)]
        view += tag == PSD
        row += rows
    out["psd_first"] = [int(np.sum(np.asarray(out["psd_mem"], dtype=int) < k)) for k in range(len(m_part) + 1)]
    out["psd_sizes"] = [len(out["psd_mem"]), len(out["psd_diag"]), view]
    return out


PLANS = {
    # sides 1, 2 and 3, one member each
    "sides": ([1, 1, 1], [1, 3, 6], [(PSD, 1), (PSD, 2), (PSD, 3)]),
    # two PSD cones in one member, between members without any
    "two_in_one": ([2, 3, 1], [3, 9, 2], [(NN, 3), (PSD, 3), (PSD, 2), (ZERO, 2)]),
    # a PSD cone as the first and as the last cone of a member
    "first_and_last": ([2, 2], [8, 7], [(PSD, 2), (NN, 2), (SOC, 3), (ZERO, 1), (NN, 3), (PSD, 2)]),
    # PSD(0) at a member boundary: it belongs to nobody, and the later cones' view indices count it
    "empty_at_boundary": ([1, 0, 2], [3, 0, 7], [(PSD, 2), (PSD, 0), (NN, 0), (PSD, 1), (PSD, 3)]),
    # one member with Nonnegative + SecondOrder + PSD cones, then a member without rows
    "mixed": ([4, 1], [4 + 3 + 6 + 2, 0], [(NN, 4), (SOC, 3), (PSD, 3), (ZERO, 2)]),
    # no PSD cone at all: every PSD array is empty, the old arrays are the old plan's
    "none": ([2, 2], [5, 3], [(NN, 2), (SOC, 3), (NN, 3)]),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_psd_arrays(hip, name):
    n_part, m_part, cones = PLANS[name]
    pl = hip.BatchPlanDebug(n_part, m_part, cones, symmetric=True)
    want = expected(m_part, cones)
    for key in pl.PSD_NAMES + ("rtype",):
        assert pl.get(key).tolist() == list(want[key]), (name, key)
    # every diagonal row lies inside its cone and its member; no item covers a PSD row
    zmem, rt = pl.get("zmem"), pl.get("rtype")
    for c, (k, r0, n) in enumerate(zip(want["psd_mem"], want["psd_start"], want["psd_dim"])):
        d = want["psd_diag"][sum(want["psd_dim"][:c]):sum(want["psd_dim"][:c + 1])]
        assert len(d) == n and d[0] == r0 and d[-1] == r0 + tri(n) - 1
        assert np.all(zmem[r0:r0 + tri(n)] == k)
    for b, e in zip(pl.get("it_beg"), pl.get("it_end")):
        assert np.all(rt[b:e] != pl.ROW_PSD)
    first = pl.get("psd_first")
    assert first[0] == 0 and first[-1] == len(want["psd_mem"]) and np.all(np.diff(first) >= 0)


def test_plan_without_psd_is_the_old_plan(hip):
    n_part, m_part, cones = PLANS["none"]
    old = hip.BatchPlanDebug(n_part, m_part, cones)
    new = hip.BatchPlanDebug(n_part, m_part, cones, symmetric=True)
    for key in old.NAMES + old.PSD_NAMES + ("sizes",):
        assert np.array_equal(old.get(key), new.get(key)), key
    assert new.get("psd_sizes").tolist() == [0, 0, 0] and new.get("degree").tolist() == [2 + 1, 3]


# ---- 5. the kernels' resources -------------------------------------------------------------------------------------
# every kernel of batch_psd.hip: no scratch, no LDS, eight waves per SIMD (256-thread workgroups)
BP_KERNELS = ["k_bp_fold", "k_bp_diag"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_batch_psd_kernels_do_not_spill():
    res = _resources("batch_psd.hip")
    for k in BP_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert len(names) == 1, (k, names)
        r = res[names[0]]
        assert r["ScratchSize"] == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)
        assert r["Occupancy"] >= 8, (k, r)
    assert len(res) == len(BP_KERNELS), sorted(res)
    src = open(os.path.join(ROOT, "clarabel.rs_amd", "csrc", "batch_psd.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src)
