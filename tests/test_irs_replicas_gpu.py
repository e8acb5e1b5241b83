"""-m gpu: the replica slots of the fused solve kernels (csrc/kernels.hpp: IRS_REP_R; csrc/bundle_ir.hip: RepView) -- the
updates of a level's entries into the two expansion columns of a second-order cone are spread over 8 LDS slots each and
folded before anything reads the columns -- against the CPU oracle on the same inputs and the same permutation, and against
a handle created under CHIP_IRS_FLAGS bit 16 (no replica ids, the same kernels on the same build).  Only the order of the
sums into those columns differs between the two.

Shapes: bundles of 3 b + 3 nodes.  b = 200 (603 nodes, the fused kernel's, a level of 600 entries: no multiple of the
batch), two classes of bundles (600 / 700), and the sizes around the rule's threshold of 64 entries, b = 63 / 64 / 65:
those bundles (192 .. 198 nodes) and the three large bundles of portfolio_socp(3, 1000) (a grouped fold) are not the
fused kernel's, so they must come out with no replica slots and their own kernel; the threshold itself is tested on the
host (tests/test_irs_replicas_host.py)."""
import numpy as np
import pytest

from tests import problems
from tests.bundle_pattern_problems import two_sizes
from tests.test_bundle_pattern_gpu import TOL, TOL_ORDER, _references, _run, _solvers, relerr
from tests.test_irs_fixed_gpu import SETTINGS, _fixed, _nan_is_refused

pytestmark = pytest.mark.gpu

FUSED = [(4, 200), "two_sizes"]
OTHER = [(4, 63), (4, 64), (4, 65), (3, 1000)]
NOREP = "19"  # CHIP_IRS_FLAGS: 3, the defaults, + 16; read when a handle is created


def _problem(prob):
    return two_sizes(600, 700) if prob == "two_sizes" else problems.portfolio_socp(prob[0], prob[1], seed=11)


def _id(p):
    return p if isinstance(p, str) else "%dx%d" % p


def _replicas(hip, ks):
    return hip.debug_counter(ks, "irs_replica_bundles"), hip.debug_counter(ks, "irs_replica_nodes")


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("prob", FUSED, ids=_id)
def test_replica_slots_against_oracle_and_switch(hip, oracle, prob, setting, monkeypatch):
    """two scaling points with an update between them; "bench": the paired call + a single solve + the paired right-hand
    sides one at a time (tests/test_bundle_pattern_gpu.py: _run), so a paired call is compared with separate calls.
    Every solve takes k_bundle_irs_fixed; u and v of every bundle have slots; 1e-8 against the oracle with its rounds;
    1e-10 against the handle without replica ids; a NaN in the right-hand side is refused by both."""
    pr = _problem(prob)
    kw = SETTINGS[setting]
    st = hip.Settings.default(**kw) if kw else None
    paired = setting == "bench"
    label = "%s / %s" % (_id(prob), setting)
    ks, ko, cones = _solvers(hip, oracle, pr, st)
    refs = _references(oracle, ko, cones, pr, 3 if paired else 2)
    nb = ks.work_model()["n_bundles"]
    assert _replicas(hip, ks) == (nb, 2 * nb), label
    sols = _run(hip, ks, pr, refs, True, paired, label)
    solves = 2 * (5 if paired else 2)
    assert _fixed(hip, ks) == solves, label
    _nan_is_refused(hip, ks, pr, label)
    assert _fixed(hip, ks) == solves + 1 and ks.fused_fallbacks() == 0, label
    monkeypatch.setenv("CHIP_IRS_FLAGS", NOREP)
    ks0, _, _ = _solvers(hip, oracle, pr, st)
    assert _replicas(hip, ks0) == (0, 0), label
    sols0 = _run(hip, ks0, pr, refs, True, paired, label + " / no replicas")
    assert _fixed(hip, ks0) == solves, label
    _nan_is_refused(hip, ks0, pr, label + " / no replicas")
    for a, b in zip(sols, sols0):
        print("%s: replica slots against none %.3e" % (label, relerr(a, b)))
        assert relerr(a, b) <= TOL_ORDER, (label, relerr(a, b))


def test_general_kernel_with_replica_slots(hip, oracle, monkeypatch):
    """CHIP_IRS_FLAGS = 11: k_bundle_irs (the instance with the run-time switches) reads the same replica ids"""
    pr = _problem((4, 200))
    monkeypatch.setenv("CHIP_IRS_FLAGS", "11")
    ks, ko, cones = _solvers(hip, oracle, pr, None)
    refs = _references(oracle, ko, cones, pr, 2)
    assert _replicas(hip, ks) == (4, 8)
    sols = _run(hip, ks, pr, refs, True, False, "general")
    assert _fixed(hip, ks) == 0
    monkeypatch.setenv("CHIP_IRS_FLAGS", "27")
    ks0, _, _ = _solvers(hip, oracle, pr, None)
    assert _replicas(hip, ks0) == (0, 0)
    for a, b in zip(sols, _run(hip, ks0, pr, refs, True, False, "general / no replicas")):
        assert relerr(a, b) <= TOL_ORDER, relerr(a, b)


def test_chained_prologue_ignores_the_replica_ids(hip, oracle, monkeypatch):
    """a handle created WITH replica ids in its shared copies, launched under CHIP_IRS_FLAGS = 7 (no records, hence no
    slots: a later handle's creation re-reads the switches for every handle): the kernel masks the ids"""
    pr = _problem((4, 200))
    ks, ko, cones = _solvers(hip, oracle, pr, None)
    refs = _references(oracle, ko, cones, pr, 2)
    assert hip.debug_kkt_ints(ks, "irs_rep").reshape(-1, 4)[:, 0].tolist() == [2 | 8 << 8] * 4
    monkeypatch.setenv("CHIP_IRS_FLAGS", "7")
    _solvers(hip, oracle, problems.portfolio_socp(3, 20, seed=1), None)  # (any creation reloads the switches)
    assert _replicas(hip, ks) == (0, 0)
    _run(hip, ks, pr, refs, True, False, "chained")
    assert _fixed(hip, ks) == 0


@pytest.mark.parametrize("prob", OTHER + ["banded_qp"], ids=_id)
def test_other_handles_keep_their_kernel(hip, oracle, prob, monkeypatch):
    """bundles the fused kernel does not take (under 512 nodes; a grouped fold; a banded QP with a level-scheduled top): no
    replica slots, no launch of k_bundle_irs_fixed, the oracle's solution, and the same under the switch bit"""
    pr = problems.random_qp(3000, 6000, band=30, seed=2) if prob == "banded_qp" else _problem(prob)
    n = pr["n"]
    ks, ko, cones = _solvers(hip, oracle, pr, None)
    refs = _references(oracle, ko, cones, pr, 1)
    assert not ks.step_kernels() & 4 and _replicas(hip, ks) == (0, 0)
    monkeypatch.setenv("CHIP_IRS_FLAGS", NOREP)
    ks0, _, _ = _solvers(hip, oracle, pr, None)
    for s_, z_, pts in refs:
        got = []
        for k_ in (ks, ks0):
            assert k_.update_scaling(s_, z_) and k_.update()
            rx, rz, ref, rounds = pts[0]
            d_rx, d_rz, out = hip.DeviceArray(rx), hip.DeviceArray(rz), hip.DeviceArray(n + pr["m"])
            k_.setrhs_dev(d_rx.ptr, d_rz.ptr)
            assert k_.solve_dev(out.ptr, out.ptr + 8 * n)
            got.append(out.numpy())
            assert relerr(got[-1], ref) <= TOL, (prob, relerr(got[-1], ref))
        assert relerr(got[0], got[1]) <= TOL_ORDER
    assert _fixed(hip, ks) == 0 and _fixed(hip, ks0) == 0 and _replicas(hip, ks0) == (0, 0)
