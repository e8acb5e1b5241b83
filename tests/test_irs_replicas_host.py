"""CPU-side test of the replica ids of the fused solve kernel's shared index copies (csrc/host.hpp: PatternShare::Rep,
csrc/symbolic.cpp: encode_replicas, csrc/kernels.hpp: IRS_REP_R).  A dense target -- one of a bundle's last four nodes that
at least 64 entries of one level of the forward stream, or of the residual's flat range, add into -- gets R - 1 further LDS
slots, and the top 4 bits of the entries of the SHARED Li16 / Ucol16 say which slot an entry uses.  Host-only handles; the
arrays come through include/clarabel_hip_testing.h: chip_debug_kkt_ints.

The rule's threshold lies at bundles of 3 * 64 + 3 nodes, under the 512 nodes the kernel takes: for those sizes the test
reads "replica_plan", what the rule says about the system's bundles by itself (no handle uses it)."""
import numpy as np
import pytest

from tests import problems
from tests.bundle_pattern_problems import two_sizes

R, MASK, BITS, WAVE = 8, 0xFFF, 12, 64
CHAIN = ("bundle_ptr", "blvl_ptr", "blvl", "Lp", "Up", "pat_off", "irs_rep", "pat_Li16", "pat_Ucol16", "pat_Urow16", "Li16", "Ucol16")


def _mk(hip, pr):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    return hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=hip.Settings.default(device=hip.DEVICE_HOST_ONLY))


def _arrays(hip, ks):
    return {k: hip.debug_kkt_ints(ks, k).astype(np.int64) for k in CHAIN}


def _groups_ok(node, r, first, nloc):
    """in every aligned group of 64 consecutive stream positions no (node, r) occurs more than ceil(c / R) times, c being
    the node's entries in the group"""
    for g in range(0, len(node), WAVE):
        nd, rr = node[g:g + WAVE], r[g:g + WAVE]
        for t in np.unique(nd[(nd >= first) & (nd < nloc)]):
            cnt = np.bincount(rr[nd == t], minlength=R)
            if cnt.max() > -(-int(cnt.sum()) // R):
                return False
    return True


def _check_bundle(c, b):
    """everything the kernel relies on, for bundle b; returns (ND, first, fold)"""
    s0, s1 = c["bundle_ptr"][b], c["bundle_ptr"][b + 1]
    nloc = s1 - s0
    lv = c["blvl"][c["blvl_ptr"][b]:c["blvl_ptr"][b + 1]]
    nl, nleaf = len(lv) - 1, lv[1] - s0
    dl, du = c["pat_off"][2 * b:2 * b + 2]
    w = c["irs_rep"][4 * b:4 * b + 4]
    nd, first, fold = w[0] & 0xFF, w[1], w[2]
    l0, l1, u0, u1 = c["Lp"][s0], c["Lp"][s1], c["Up"][s0], c["Up"][s1]
    li, uc, ur = c["pat_Li16"][l0 + dl:l1 + dl], c["pat_Ucol16"][u0 + du:u1 + du], c["pat_Urow16"][u0 + du:u1 + du]
    # the masked copies are the bundle's own slices
    assert np.array_equal(li & MASK, c["Li16"][l0:l1]) and np.array_equal(uc & MASK, c["Ucol16"][u0:u1]), b
    assert (ur >> BITS == 0).all()
    if nd == 0:
        assert (li >> BITS == 0).all() and (uc >> BITS == 0).all() and w[0] == 0
        return 0, 0, 0
    # the record: R, the nodes first .. nloc - 1 among the last four and no leaves, fold = the level of node `first`
    assert w[0] >> 8 == R and 1 <= nd <= 4 and first == nloc - nd and first >= nleaf and w[3] == 0
    assert lv[fold] - s0 <= first < lv[fold + 1] - s0 and 0 < fold < nl
    # forward stream: ids only on entries into replicated nodes, only in levels in front of the fold level
    node, r = li & MASK, li >> BITS
    assert (r[(node < first) | (node >= nloc)] == 0).all()
    assert (r[c["Lp"][lv[fold]] - l0:] == 0).all()
    for l in range(fold):
        e0, e1 = c["Lp"][lv[l]] - l0, c["Lp"][lv[l + 1]] - l0
        assert _groups_ok(node[e0:e1], r[e0:e1], first, nloc), (b, l)
    head = slice(0, c["Lp"][lv[fold]] - l0)
    for t in range(first, nloc):
        cnt = np.bincount(r[head][node[head] == t], minlength=R)
        assert cnt.max() - cnt.min() <= 1, (b, t, cnt)
    # residual: ids only in the flat range (rows of the non-leaf nodes), only off the diagonal, only into replicated nodes
    f0 = c["Up"][s0 + nleaf] - u0
    col, ru = uc & MASK, uc >> BITS
    assert (ru[:f0] == 0).all()
    assert (ru[(col < first) | (col >= nloc) | (col == ur)] == 0).all()
    assert _groups_ok(np.where(col[f0:] == ur[f0:], -1, col[f0:]), ru[f0:], first, nloc), b  # (a diagonal entry adds into no column)
    for t in range(first, nloc):
        sel = (col[f0:] == t) & (ur[f0:] != t)
        cnt = np.bincount(ru[f0:][sel], minlength=R)
        assert cnt.max() - cnt.min() <= 1, (b, t, cnt)
    return nd, first, fold


def _dense_levels(c, b, first):
    """entries per forward level that add into each of the nodes first .. nloc - 1 (own slices)"""
    s0, s1 = c["bundle_ptr"][b], c["bundle_ptr"][b + 1]
    lv = c["blvl"][c["blvl_ptr"][b]:c["blvl_ptr"][b + 1]]
    out = []
    for l in range(len(lv) - 1):
        i = c["Li16"][c["Lp"][lv[l]]:c["Lp"][lv[l + 1]]]
        out.append([int((i == t).sum()) for t in range(first, s1 - s0)])
    return out


@pytest.mark.parametrize("bs", [170, 200, 341])
def test_u_and_v_of_every_bundle_are_replicated(hip, bs):
    """portfolio_socp(4, bs): 3 bs + 3 nodes per bundle, levels of bs + 1 / bs / bs / 1 / 1 nodes; level 2 of the forward
    stream adds bs entries into u and bs into v (the last two nodes), the flat range of the residual likewise"""
    ks = _mk(hip, problems.portfolio_socp(4, bs, seed=3))
    c = _arrays(hip, ks)
    nb = len(c["bundle_ptr"]) - 1
    assert nb == 4 and hip.debug_counter(ks, "pattern_classes") == 1
    for b in range(nb):
        assert _check_bundle(c, b) == (2, 3 * bs + 1, 3), b
    assert _dense_levels(c, 0, 3 * bs + 1)[2] == [bs, bs]
    assert hip.debug_counter(ks, "irs_replica_bundles") == nb and hip.debug_counter(ks, "irs_replica_nodes") == 2 * nb


@pytest.mark.parametrize("bs,nd", [(63, 0), (64, 2), (65, 2)])
def test_threshold_of_64_entries(hip, bs, nd):
    """the rule by itself ("replica_plan"): 63 entries of a level on one node do not make it a dense target, 64 do"""
    ks = _mk(hip, problems.portfolio_socp(4, bs, seed=3))
    plan = hip.debug_kkt_ints(ks, "replica_plan").reshape(-1, 4)
    assert len(plan) == 4
    want = [nd | R << 8, 3 * bs + 1, 3, 0] if nd else [0, 0, 0, 0]
    assert (plan == want).all(), plan
    # (bundles of under 512 nodes: the kernel does not take them, so no handle carries the plan)
    assert hip.debug_counter(ks, "irs_replica_bundles") == 0 and len(hip.debug_kkt_ints(ks, "irs_rep")) == 0


def test_two_classes_have_their_own_assignments(hip):
    ks = _mk(hip, two_sizes(600, 700))
    c = _arrays(hip, ks)
    assert hip.debug_counter(ks, "pattern_classes") == 2
    got = {_check_bundle(c, b) for b in range(6)}
    assert got == {(2, 1801, 3), (2, 2101, 3)}
    assert hip.debug_counter(ks, "irs_replica_bundles") == 6 and hip.debug_counter(ks, "irs_replica_nodes") == 12


def test_full_scale_workload(hip):
    """the benchmark's problem: one class, u and v of every bundle, and the shared arrays are the bytes they were"""
    ks = _mk(hip, problems.portfolio_socp(1000, 1000, seed=3))
    rep = hip.debug_kkt_ints(ks, "irs_rep").reshape(-1, 4)
    assert len(rep) == 1000 and (rep == [2 | R << 8, 3001, 3, 0]).all()
    assert hip.debug_counter(ks, "pattern_index_bytes") == 56048 and hip.debug_counter(ks, "pattern_classes") == 1
    assert hip.debug_counter(ks, "pattern_verified_bundles") == 1000 and hip.debug_counter(ks, "pattern_mismatches") == 0
    assert hip.debug_counter(ks, "irs_replica_bundles") == 1000 and hip.debug_counter(ks, "irs_replica_nodes") == 2000
    li = hip.debug_kkt_ints(ks, "pat_Li16").astype(np.int64)
    assert [int(x) for x in np.bincount(li >> BITS, minlength=R)[1:]] == [250] * 7  # (2 x 1000 entries over 8 slots)


@pytest.mark.parametrize("env", [{"CHIP_IRS_FLAGS": "19"}, {"CHIP_NO_SHARED_PATTERN": "1"}])
def test_switches_leave_no_replica_ids(hip, monkeypatch, env):
    """CHIP_IRS_FLAGS bit 16 (19 = the defaults + 16) and CHIP_NO_SHARED_PATTERN, read when a handle is created"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ks = _mk(hip, problems.portfolio_socp(4, 200, seed=3))
    rep = hip.debug_kkt_ints(ks, "irs_rep")
    assert len(rep) == 16 and (rep == 0).all()
    assert hip.debug_counter(ks, "irs_replica_bundles") == 0 and hip.debug_counter(ks, "irs_replica_nodes") == 0
    for name in ("pat_Li16", "pat_Ucol16"):
        assert (hip.debug_kkt_ints(ks, name).astype(np.int64) >> BITS == 0).all()
