"""What chip_batch_create and chip_solver_create refuse on the host, pinned by return code AND chip_last_error() text:
the batch checks its arguments, settings, cones, sizes, partition and every entry of P and A before it asks for a
device, so the order and wording of those refusals can be asserted on a machine without one.  chip_solver_create asks
for the device first.  Every batch case is the stack of two basic_qp members (n = 4, m = 12) with one thing wrong."""
import ctypes as C

import numpy as np
import pytest

from tests import e2e_problems as E

ZERO, NN, SOC, EXP = range(4)
BAD_ARG = "chip_batch_create: bad argument"
P_CROSSES = "chip_batch_create: an entry of P crosses two members' blocks"
A_CROSSES = "chip_batch_create: an entry of A crosses two members' blocks"
CONE_CROSSES = "chip_batch_create: a cone crosses a member's rows"
NO_TRANSFORMS = "chip_batch_create: presolve and chordal decomposition are not supported"


def raw_batch_create(hip, st, n_part, m_part, cones=None, settings=None, nprob=None, null_out=False):
    """chip_batch_create through ctypes on a stack as hip.batch_stack() gives it, with a partition, cones, settings
    and member count of the caller's choice; a handle that was created is destroyed.  Returns the code."""
    Pp, Pi, Px = st["P"]
    Ap, Ai, Ax = st["A"]
    tags, dims, dims2, alphas = hip._cone_arrays(cones if cones is not None else st["cones"])
    n_part = np.asarray(n_part, dtype=np.int64)
    m_part = np.asarray(m_part, dtype=np.int64)
    h = C.c_void_p()
    s = settings if settings is not None else hip.SolverSettings.default()
    rc = hip.lib().chip_batch_create(None if null_out else C.byref(h),
                                     C.c_int64(len(n_part) if nprob is None else nprob), n_part.ctypes.data_as(hip.P_I64),
                                     m_part.ctypes.data_as(hip.P_I64), C.c_int64(st["n"]), C.c_int64(st["m"]),
                                     hip._pu(Pp), hip._pu(Pi), hip._pf(Px), hip._pf(st["q"]), hip._pu(Ap), hip._pu(Ai),
                                     hip._pf(Ax), hip._pf(st["b"]), C.c_int64(len(tags)), tags.ctypes.data_as(hip.P_I32),
                                     dims.ctypes.data_as(hip.P_I64), dims2.ctypes.data_as(hip.P_I64), hip._pf(alphas),
                                     None, C.byref(s))
    if rc == 0:
        hip.lib().chip_batch_destroy(h)
    return rc


def _member(hip, pr):
    n, m = pr["n"], pr["m"]
    return (hip.CscMatrix(n, n, *pr["P"]), pr["q"], hip.CscMatrix(m, n, *pr["A"]), pr["b"], pr["cones"])


@pytest.fixture(scope="module")
def stack(hip):
    """two basic_qp members: P's columns hold rows (0), (0, 1), (2), (2, 3); A's hold four rows of the member each"""
    st = hip.batch_stack([_member(hip, E.basic_qp()), _member(hip, E.basic_qp())])
    assert (st["n"], st["m"]) == (4, 12) and list(st["P"][1]) == [0, 0, 1, 2, 2, 3]
    return st


def _refused(hip, code, text, *args, **kw):
    assert raw_batch_create(hip, *args, **kw) == code
    assert hip.lib().chip_last_error().decode() == text


def _with(st, key, colptr=None, rowval=None):
    """a copy of the stack whose P or A has another colptr and / or rowval"""
    p, i, x = st[key]
    out = dict(st)
    out[key] = (p if colptr is None else np.array(colptr, dtype=p.dtype),
                i if rowval is None else np.array(rowval, dtype=i.dtype), x)
    return out


def test_bad_arguments(hip, stack):
    _refused(hip, hip.ERR_ARG, BAD_ARG, stack, [2, 2], [6, 6], null_out=True)
    _refused(hip, hip.ERR_ARG, BAD_ARG, stack, [2, 2], [6, 6], nprob=0)


def test_bad_partition(hip, stack):
    _refused(hip, hip.ERR_ARG, "chip_batch_create: negative part", stack, [-1, 5], [6, 6])
    _refused(hip, hip.ERR_ARG, "chip_batch_create: negative part", stack, [2, 2], [6, -1])
    _refused(hip, hip.ERR_ARG, "chip_batch_create: the parts exceed n or m", stack, [3, 2], [6, 6])
    _refused(hip, hip.ERR_ARG, "chip_batch_create: the parts exceed n or m", stack, [2, 2], [6, 7])
    _refused(hip, hip.ERR_ARG, "chip_batch_create: the parts do not add up to n, m", stack, [2, 2], [6, 5])
    _refused(hip, hip.ERR_ARG, "chip_batch_create: the parts do not add up to n, m", stack, [2, 1], [6, 6])


def test_unsupported(hip, stack):
    _refused(hip, hip.ERR_UNSUPPORTED, "chip_batch_create: only Zero, Nonnegative and SecondOrder cones", stack, [2, 2],
             [6, 6], cones=[(NN, 3), (NN, 3), (NN, 3), (EXP, 3)])
    _refused(hip, hip.ERR_UNSUPPORTED, NO_TRANSFORMS, stack, [2, 2], [6, 6],
             settings=hip.SolverSettings.default(presolve_enable=1))
    # the settings are looked at before the partition
    _refused(hip, hip.ERR_UNSUPPORTED, NO_TRANSFORMS, stack, [2, 2], [6, 5],
             settings=hip.SolverSettings.default(presolve_enable=1))


def test_p_not_upper_triangular(hip, stack):
    _refused(hip, hip.ERR_NOT_TRIU, "P is not upper triangular", _with(stack, "P", rowval=[1, 0, 1, 2, 2, 3]), [2, 2],
             [6, 6])
    # column 2 (the second member's first) with a sub-diagonal entry (row 3) and one in the first member's block
    # (row 1): the sub-diagonal one is reported.  Entries are checked in storage order, each for triangularity and
    # then for crossing
    two = dict(colptr=[0, 1, 3, 5, 6])
    _refused(hip, hip.ERR_NOT_TRIU, "P is not upper triangular", _with(stack, "P", rowval=[0, 0, 1, 3, 1, 3], **two),
             [2, 2], [6, 6])
    _refused(hip, hip.ERR_ARG, P_CROSSES, _with(stack, "P", rowval=[0, 0, 1, 1, 3, 3], **two), [2, 2], [6, 6])


def test_entries_across_members(hip, stack):
    # column 1 now belongs to the second member: its entries of P and of A all cross, and P's are checked first
    _refused(hip, hip.ERR_ARG, P_CROSSES, stack, [1, 3], [6, 6])
    # rows split inside the first member's second cone: the entry of A is reported, not the cone
    _refused(hip, hip.ERR_ARG, A_CROSSES, stack, [2, 2], [4, 8])
    # columns are checked in order: column 0's entry of A comes before column 1's entry of P
    _refused(hip, hip.ERR_ARG, A_CROSSES, stack, [1, 3], [4, 8])


def test_a_row_out_of_range(hip, stack):
    rows = list(stack["A"][1])
    rows[-1] = stack["m"]
    _refused(hip, hip.ERR_DIM, "A row index out of range", _with(stack, "A", rowval=rows), [2, 2], [6, 6])


def test_cones(hip, stack):
    _refused(hip, hip.ERR_ARG, CONE_CROSSES, stack, [2, 2], [6, 6], cones=[(NN, 3), (NN, 6), (NN, 3)])
    _refused(hip, hip.ERR_DIM, "chip_batch_create: cone dimensions do not add up to m", stack, [2, 2], [6, 6],
             cones=[(NN, 3), (NN, 3), (NN, 3)])
    # a refused cone is reported only after the entries were checked
    _refused(hip, hip.ERR_ARG, A_CROSSES, stack, [2, 2], [4, 8], cones=[(NN, 3), (NN, 3), (NN, 3)])


NEEDS_NO_GPU = "the device check is reached only on a host without a GPU"


def test_valid_stack_asks_for_a_device(hip, stack):
    if hip.device_count() > 0:
        pytest.skip(NEEDS_NO_GPU)
    _refused(hip, hip.ERR_NO_DEVICE, "chip_batch_create: no HIP device (the product has no CPU fallback)", stack, [2, 2],
             [6, 6])


@pytest.mark.parametrize("rows", [[0, 0, 1], [1, 0, 1]], ids=["triu", "lower"])
def test_single_solver_asks_for_a_device_first(hip, rows):
    if hip.device_count() > 0:
        pytest.skip(NEEDS_NO_GPU)
    pr = E.basic_qp()
    P, q, A, b, cones = _member(hip, dict(pr, P=(pr["P"][0], np.array(rows), pr["P"][2])))
    with pytest.raises(hip.ChipError) as e:
        hip.HipSolver(P, q, A, b, cones)
    assert e.value.code == hip.ERR_NO_DEVICE
    assert hip.lib().chip_last_error().decode() == "chip_solver_create: no HIP device (the product has no CPU fallback)"
