"""Verdicts without a copy launch (csrc/engine.hpp: Engine::mb_mirror): on a handle whose update ends in the top pivot's
launch and whose solves k_bundle_irs takes, those launches store their verdict words into the page-locked host mirror
of the mailbox as well, and collect() only waits for the stream.  CHIP_NO_HOST_MAILBOX keeps the copy.  Both ways must
tell the host exactly the same: update verdict, regulariser, regularised-pivot count, inertia, the solves' verdicts and
results -- for good steps, failed cone scalings, regularised pivots, failed solves and a verdict ring that wraps.
The counters "mailbox_copies" / "mailbox_mirror_reads" (chip_debug_counter) say which way a collect went.

portfolio_socp(4, 200): four bundles of 603 nodes, one folded top column, fused solves by k_bundle_irs.  (With THREE
blocks of 200 the analysis cuts the blocks into 8 smaller bundles to fill more workgroups, below the 512 nodes
k_bundle_irs asks of a bundle, and no launch of that handle writes the mirror; four blocks are the smallest count at this
block size whose handle takes the path under test.  The three-block handle is among those that must keep the copy.)"""
import numpy as np
import pytest

from tests import problems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


class Step:
    def __init__(self, hip, pr, settings=None):
        self.hip, self.pr = hip, pr
        P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
        A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
        self.ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=settings)
        D = hip.DeviceArray
        self.d_s, self.d_z = D(pr["m"]), D(pr["m"])
        self.rx, self.rz, self.lx, self.lz = D(pr["n"]), D(pr["m"]), D(pr["n"]), D(pr["m"])

    def counters(self):
        return tuple(int(self.hip.debug_counter(self.ks, k)) for k in ("mailbox_copies", "mailbox_mirror_reads"))

    def run(self, s, z, rhs, nsolves=1, update=True):
        """one update (optional) and nsolves solves of rhs[k], ONE collect -> everything the host learns from it"""
        if update:
            self.d_s.copy_from(s)
            self.d_z.copy_from(z)
            self.ks.update_scaled_enqueue(self.d_s.ptr, self.d_z.ptr)
        sols = []
        lhs = [(self.hip.DeviceArray(self.pr["n"]), self.hip.DeviceArray(self.pr["m"])) for _ in range(nsolves)]
        for k in range(nsolves):
            bx, bz = self.hip.DeviceArray(rhs[k][0]), self.hip.DeviceArray(rhs[k][1])
            sols.append((bx, bz))  # (borrowed until the solve has run)
            self.ks.setrhs_dev(bx.ptr, bz.ptr)
            self.ks.solve_dev_enqueue(lhs[k][0].ptr, lhs[k][1].ptr)
        uok, sok = self.ks.collect()
        info = self.ks.linear_solver_info()
        out = dict(uok=uok, sok=sok, repeated=list(self.ks.repeated_solves), reg=int(info.regularize_count),
                   inertia=int(info.positive_inertia), eps=float(info.last_regularizer))
        out["x"] = [np.concatenate([a.numpy(), b.numpy()]) if ok else None for (a, b), ok in zip(lhs, sok)]
        return out


def same(a, b, label):
    for k in ("uok", "sok", "repeated", "reg", "inertia", "eps"):
        assert a[k] == b[k], (label, k, a[k], b[k])
    for x, y in zip(a["x"], b["x"]):
        assert (x is None) == (y is None), label
        if x is not None:  # (two factorisations of the same K: their LDS atomics may add in another order)
            assert float(np.max(np.abs(x - y))) <= 1e-10 * max(1.0, float(np.max(np.abs(y)))), label


def both_ways(st, label, *args, **kw):
    """the same enqueues with the mirror and with CHIP_NO_HOST_MAILBOX; the counters must say which way each went"""
    hip = st.hip
    c0 = st.counters()
    a = st.run(*args, **kw)
    c1 = st.counters()
    hip.debug_set_switch("CHIP_NO_HOST_MAILBOX", "1")
    try:
        b = st.run(*args, **kw)
    finally:
        hip.debug_set_switch("CHIP_NO_HOST_MAILBOX", None)
    c2 = st.counters()
    print("  %s: copies / mirror reads %s -> %s -> %s; update %s solves %s regularised %d inertia %d eps %.3e" %
          (label, c0, c1, c2, a["uok"], a["sok"], a["reg"], a["inertia"], a["eps"]))
    assert c1 == (c0[0], c0[1] + 1), (label, "the mirror was not read", c0, c1)
    assert c2 == (c1[0] + 1, c1[1]), (label, "CHIP_NO_HOST_MAILBOX did not copy", c1, c2)
    same(a, b, label)
    return a


@pytest.fixture(scope="module")
def step(hipdev):
    st = Step(hipdev, problems.portfolio_socp(4, 200, seed=3))
    assert hipdev.debug_counter(st.ks, "mailbox_mirror_on") == 1
    yield st  # (that k_bundle_irs takes its solves shows in the counters: both_ways insists on a mirror read)
    del st


def rhs_of(pr, seed, count=1):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(pr["n"]), rng.standard_normal(pr["m"])) for _ in range(count)]


def test_good_step(step):
    pr = step.pr
    a = both_ways(step, "good step", pr["s"], pr["z"], rhs_of(pr, 1))
    assert a["uok"] and a["sok"] == [True] and a["repeated"] == [] and a["eps"] > 0.0


def test_non_interior_s(step):
    """s0 of the second cone halved below its tail's norm: update_ok is 0 either way, and the good step after it passes"""
    pr = step.pr
    n, dim = 4 * 200, 201
    s = pr["s"].copy()
    o = 1 + n + dim
    s[o] = 0.5 * np.linalg.norm(s[o + 1:o + dim])
    a = both_ways(step, "non-interior s", s, pr["z"], [], nsolves=0)
    assert not a["uok"]
    b = both_ways(step, "good step after it", pr["s"], pr["z"], rhs_of(pr, 2))
    assert b["uok"] and b["sok"] == [True]


def test_nan_right_hand_side(step):
    pr = step.pr
    rhs = rhs_of(pr, 3)
    rhs[0][1][5] = np.nan
    a = both_ways(step, "NaN rhs", pr["s"], pr["z"], rhs)
    assert a["uok"] and a["sok"] == [False]


def test_ring_wraps(step):
    """20 solves in groups of 4 behind one update: the ring of 16 verdict slots wraps in the fifth group"""
    pr = step.pr
    rhs = rhs_of(pr, 4, 20)
    rhs[17][0][0] = np.nan  # (a failure whose slot has been used before)
    both_ways(step, "update", pr["s"], pr["z"], [], nsolves=0)
    for g in range(5):
        grp = rhs[4 * g:4 * g + 4]
        a = both_ways(step, "group %d" % g, None, None, grp, nsolves=4, update=False)
        assert a["sok"] == [not np.isnan(r[0][0]) for r in grp], (g, a["sok"])


def test_regularised_pivots(hipdev):
    """pivot thresholds raised as in tests/test_factor_runs_gpu.py (eps 0.3, delta 0.5): the count of regularised pivots
    and the inertia reach the host through the mirror as through the copy"""
    pr = problems.portfolio_socp(4, 200, seed=3)
    st = Step(hipdev, pr, hipdev.Settings.default(dynamic_regularization_eps=0.3, dynamic_regularization_delta=0.5))
    a = both_ways(st, "raised thresholds", pr["s"], pr["z"], rhs_of(pr, 5))
    assert a["uok"] and a["reg"] >= 1


def test_other_handles_keep_the_copy(hipdev):
    """systems whose launches do not write the mirror -- a banded QP with chain supernodes (no fused solve), three blocks
    of 200 (fused solves by k_bundle_ir, not k_bundle_irs), and a use_graph handle of a level-scheduled system: every
    collect copies, none reads the mirror"""
    for label, pr, stg in (("banded QP", problems.random_qp(3000, 6000, band=30, seed=2), None),
                           ("3 x 200", problems.portfolio_socp(3, 200, seed=3), None),
                           ("banded QP, use_graph", problems.random_qp(3000, 6000, band=30, seed=2), hipdev.Settings.default(use_graph=1))):
        st = Step(hipdev, pr, stg)
        assert hipdev.debug_counter(st.ks, "mailbox_mirror_on") == 0, label
        c0 = st.counters()
        a = st.run(pr["s"], pr["z"], rhs_of(pr, 6))
        c1 = st.counters()
        print("  %s: copies / mirror reads %s -> %s" % (label, c0, c1))
        assert a["uok"] and a["sok"] == [True], label
        assert c1[1] == 0 and c1[0] > c0[0], (label, c0, c1)

