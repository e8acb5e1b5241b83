"""The absolute number of enqueues and host synchronisations of one chip_bgrad_backward and one chip_bjvp_apply
(the debug counters backward_* and jvp_*), on a batch of two small members.  tests/test_batch_adjoint_gpu.py and
tests/test_batch_jvp_gpu.py compare the counts between batch sizes; this file pins them, so that a launch that is
reordered away, dropped or added does not pass unnoticed.

The counts are read from the host code (one per kernel, copy or call into the KKT layer, as the batched solver counts
everywhere):
  backward: valid flags + right-hand side (2), A' product (1), scaling update + refactor (2), KKT solve (1), the two
            gradient passes (2) = 8; synchronisations: refactor, KKT solve, end = 3;
  apply:    valid flags + right-hand side (2), scaling update + refactor (2, only when K is not factored at the final
            iterates), KKT solve (1), A product + output pass (2) = 7 or 5; synchronisations 3 or 2;
  a host input that is given and has entries costs one copy more; one that is given and empty costs none."""
import numpy as np
import pytest

from tests import adjoint_ref as R
from tests import e2e_problems as E
from tests import tangent_ref as T
from tests.test_batch_gpu import batch
from tests.test_batch_jvp_gpu import REPEAT_CEILING

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


def solved(hip, prs):
    b = batch(hip, prs)
    assert [s.status for s in b.solve()] == ["Solved"] * len(prs)
    return b


def stacked(prs, make, seed):
    per = [make(pr, seed + 17 * k) for k, pr in enumerate(prs)]
    return [np.concatenate([p[i] for p in per]) for i in range(len(per[0]))]


def on_device(vs):
    import torch
    return [None if v is None else torch.tensor(v, dtype=torch.float64, device="cuda") for v in vs]


def backward_counts(b):
    return b.debug_counter("backward_launches"), b.debug_counter("backward_host_syncs")


def jvp_counts(b):
    return b.debug_counter("jvp_launches"), b.debug_counter("jvp_host_syncs")


def test_absolute_counts_of_backward_and_apply(hipdev):
    prs = [R.random_qp(1), E.basic_lp()]
    g = stacked(prs, R.incoming, 3)
    d = stacked(prs, T.direction, 5)
    assert all(v.size > 0 for v in g + d)
    got = {}
    # ---- handle a, one solve: the applies first (the first one pays the refactor), then the backwards
    a = solved(hipdev, prs)
    assert a.debug_counter("jvp_refactors") == 0.0
    a.jvp(*on_device(d))
    got["first apply, device inputs"] = jvp_counts(a)
    assert a.debug_counter("jvp_refactors") == 1.0
    a.jvp(*on_device(d))
    got["apply again, device inputs"] = jvp_counts(a)
    a.jvp(*d)
    got["apply again, host inputs, all four"] = jvp_counts(a)
    a.jvp(dq=d[0])
    got["apply again, host inputs, dq only"] = jvp_counts(a)
    assert a.debug_counter("jvp_refactors") == 1.0
    a.backward(*on_device(g))
    got["backward, device inputs"] = backward_counts(a)
    a.backward(*g)
    got["backward, host inputs, all three"] = backward_counts(a)
    a.backward(gx=g[0])
    got["backward, host inputs, gx only"] = backward_counts(a)
    # ---- handle c, one solve: an apply straight after a backward finds K factored
    c = solved(hipdev, prs)
    c.backward(*on_device(g))
    c.jvp(*on_device(d))
    got["apply after a backward of a fresh solve"] = jvp_counts(c)
    assert c.debug_counter("jvp_refactors") == 0.0
    print("(launches, host syncs):", got)
    assert got == {
        "first apply, device inputs": (7.0, 3.0),
        "apply again, device inputs": (5.0, 2.0),
        "apply again, host inputs, all four": (9.0, 2.0),
        "apply again, host inputs, dq only": (6.0, 2.0),
        "backward, device inputs": (8.0, 3.0),
        "backward, host inputs, all three": (11.0, 3.0),
        "backward, host inputs, gx only": (9.0, 3.0),
        "apply after a backward of a fresh solve": (5.0, 2.0),
    }


def test_an_empty_host_input_is_given_and_costs_no_copy(hipdev):
    prs = [E.basic_lp(), E.basic_lp()]  # nnz(P) = 0
    b = solved(hipdev, prs)
    assert b._len["P"] == 0
    dq, db, _, dA = stacked(prs, T.direction, 7)
    empty = np.zeros(0)
    got = {}
    with_none = b.jvp(dq, db, None, dA)
    got["first, dP=None"] = jvp_counts(b)
    with_empty = b.jvp(dq, db, empty, dA)
    got["again, dP empty"] = jvp_counts(b)
    b.jvp(dq, db, None, dA)
    got["again, dP=None"] = jvp_counts(b)
    b.jvp(dP=empty)
    got["again, dP empty alone"] = jvp_counts(b)
    print("(launches, host syncs):", got)
    assert got == {"first, dP=None": (10.0, 3.0), "again, dP empty": (8.0, 2.0), "again, dP=None": (8.0, 2.0),
                   "again, dP empty alone": (5.0, 2.0)}
    assert list(with_empty.valid) == [1, 1]
    for u, v in zip((with_empty.dx, with_empty.dz, with_empty.ds), (with_none.dx, with_none.dz, with_none.ds)):
        assert R.rel(u, v) <= REPEAT_CEILING  # (two solves with one factorisation: atomic adds tell them apart)
