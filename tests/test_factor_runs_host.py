"""CPU-side test of the run-coded update records of the flat bundle factorisation (csrc/host.hpp: Symbolic::fr_desc;
symbolic.cpp codes them right behind the plain records): per (bundle, level) the runs expanded plus the records left
outside runs must be the plain records as multisets, every run has the minimum length, a run with a target stride has
pairwise distinct targets, and the switch turns all of it off.  Host-only handles (include/clarabel_hip_testing.h:
chip_debug_factor_updates)."""
from collections import Counter

import numpy as np
import pytest

from tests import problems

RUN_MIN = 64  # Symbolic::FU_RUN_MIN


def _mk(hip, pr):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    return hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=hip.Settings.default(device=hip.DEVICE_HOST_ONLY))


def _expand(runs):
    """rows {level, a, b, k, target} of every element of every run"""
    out = []
    for lvl, a, b, k, t, sa, sb, sk, st, cnt in runs:
        e = np.arange(cnt)
        out.append(np.stack([np.full(cnt, lvl), a + sa * e, b + sb * e, k + sk * e, t + st * e], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 5), dtype=np.int64)


def _check_bundle(hip, ks, b, run_min):
    rec = hip.debug_factor_updates(ks, b, "records").astype(np.int64)
    runs = hip.debug_factor_updates(ks, b, "runs").astype(np.int64)
    left = hip.debug_factor_updates(ks, b, "leftover").astype(np.int64)
    if int(hip.debug_counter(ks, "factor_runs")) == 0:
        assert len(runs) == 0 and len(left) == 0  # (a handle without runs keeps the plain records alone)
        return rec, runs, left
    assert (runs[:, 9] >= run_min).all(), runs[runs[:, 9] < run_min]
    lim = rec[:, 1:].max(axis=0) if len(rec) else np.zeros(4)  # (every address a run touches is one a plain record touches)
    for r in runs:
        first, stride, cnt = r[1:5], r[5:9], r[9]
        last = first + stride * (cnt - 1)
        assert (first >= 0).all() and (last >= 0).all() and (first <= lim).all() and (last <= lim).all(), r
        assert stride[3] >= 0, r
        if stride[3] != 0:
            tg = first[3] + stride[3] * np.arange(cnt)
            assert len(np.unique(tg)) == cnt, r
    both = np.concatenate([_expand(runs), left])
    assert len(both) == len(rec)
    assert Counter(map(tuple, both)) == Counter(map(tuple, rec))  # (the level is part of the row: per (bundle, level))
    return rec, runs, left


def _counters(hip, ks):
    return {k: int(hip.debug_counter(ks, "factor_" + k)) for k in ("runs", "run_leftover", "run_max_leftover", "run_invalid")}


def _nbundles(hip, ks):
    return int(hip.debug_counter(ks, "factor_record_bundles"))


@pytest.mark.parametrize("nblocks,bs,target_wg,expect_runs", [(3, 63, None, False), (3, 64, None, True), (3, 65, None, True),
                                                              (4, 200, None, True), (2, 1100, None, True), (2, 1100, "0", True)])
def test_runs_and_leftovers_are_the_records(hip, nblocks, bs, target_wg, expect_runs, monkeypatch):
    """portfolio_socp(nblocks, bs): bs = 63 has no stretch of 64 records (no runs: the handle keeps the plain records), 64
    and 65 are the first sizes with runs, 200 an ordinary one.  (2, 1100): the analysis cuts two blocks into 26 bundles
    for a device of 1024 workgroup slots, with runs of 85; with CHIP_TARGET_WG=0 (never refine) it keeps the two bundles
    of 3303 nodes, whose runs of 1100 are longer than the kernel's 1024 threads (their 9 bs + 9 doubles still fit the LDS
    of half a CU)."""
    if target_wg is not None:
        monkeypatch.setenv("CHIP_TARGET_WG", target_wg)  # (read when a handle is created)
    ks = _mk(hip, problems.portfolio_socp(nblocks, bs, seed=3))
    c = _counters(hip, ks)
    nb = _nbundles(hip, ks)
    assert nb >= 1 and c["run_invalid"] == 0
    total_runs = total_left = 0
    for b in range(nb):
        rec, runs, left = _check_bundle(hip, ks, b, RUN_MIN)
        total_runs += len(runs)
        total_left += len(left)
        if b == 0:
            print("portfolio_socp(%d, %d) bundle 0 of %d: %d records, %d runs (lengths %s), %d left over" %
                  (nblocks, bs, nb, len(rec), len(runs), sorted(set(runs[:, 9])) if len(runs) else [], len(left)))
    assert (total_runs > 0) == expect_runs
    assert c["runs"] == total_runs and c["run_leftover"] == total_left
    if target_wg == "0":
        assert nb == 2 and max(hip.debug_factor_updates(ks, 0, "runs")[:, 9]) == 1100 > 1024


def test_irregular_problem(hip):
    """random_qp: a banded pattern with random entries -- whatever runs the scan finds must still be the records; a handle
    whose runs cover less than half of its records keeps none"""
    ks = _mk(hip, problems.random_qp(3000, 6000, band=30))
    c = _counters(hip, ks)
    nb = _nbundles(hip, ks)
    assert c["run_invalid"] == 0
    nrec = 0
    for b in range(nb):
        rec, runs, left = _check_bundle(hip, ks, b, RUN_MIN)
        nrec += len(rec)
    print("random_qp(3000, 6000, band=30): %d bundles, %d records, %d runs, %d left over" % (nb, nrec, c["runs"], c["run_leftover"]))
    assert c["runs"] == 0 or 2 * c["run_leftover"] <= nrec


def test_short_runs_share_a_level_with_leftovers(hip, monkeypatch):
    monkeypatch.setenv("CHIP_FACTOR_RUN_MIN", "4")  # (read when a handle is created)
    ks = _mk(hip, problems.portfolio_socp(3, 20, seed=3))
    shared = 0
    for b in range(_nbundles(hip, ks)):
        rec, runs, left = _check_bundle(hip, ks, b, 4)
        shared += len(set(runs[:, 0]) & set(left[:, 0]))
    assert shared > 0  # (some level has both)


def test_switch_turns_runs_off(hip, monkeypatch):
    monkeypatch.setenv("CHIP_NO_FACTOR_RUNS", "1")
    ks = _mk(hip, problems.portfolio_socp(4, 200, seed=3))
    assert _counters(hip, ks) == {"runs": 0, "run_leftover": 0, "run_max_leftover": 0, "run_invalid": 0}
    for b in range(_nbundles(hip, ks)):
        assert len(hip.debug_factor_updates(ks, b, "records")) > 0
        assert len(hip.debug_factor_updates(ks, b, "runs")) == 0 and len(hip.debug_factor_updates(ks, b, "leftover")) == 0


def test_flagship_bundle_has_ten_runs(hip):
    """portfolio_socp(1000, 1000), the benchmark's config 3: bundle 0 has 3003 nodes in levels of 1001 / 1000 / 1000 / 1 / 1
    columns and 10 007 records, of which 10 runs cover 10 000: one of 1000 in level 0 (strides 1, 1, 1, 1), three of 1000
    in level 1 (2, 2, 1, then 3 / 1 / 0 for the target) and six reductions of 1000 in level 2 (3, 3, 1, 0); 7 records are
    left.  (A scan that drops the whole stretch when it is too short finds 999 + 8: here the last record of a short
    stretch may open the next one, which gives level 0 its thousandth element.)  Every bundle has the same tables."""
    ks = _mk(hip, problems.portfolio_socp(1000, 1000, seed=3))
    rec, runs, left = _check_bundle(hip, ks, 0, RUN_MIN)
    print("bundle 0: %d records, runs %s, %d left over" % (len(rec), [tuple(r[[0, 5, 6, 7, 8, 9]]) for r in runs], len(left)))
    assert len(rec) == 10007 and len(runs) == 10 and len(left) == 7
    by_level = {l: sorted(tuple(r[5:10]) for r in runs if r[0] == l) for l in set(runs[:, 0])}
    assert by_level == {0: [(1, 1, 1, 1, 1000)],
                        1: [(2, 2, 1, 0, 1000), (2, 2, 1, 1, 1000), (2, 2, 1, 3, 1000)],
                        2: [(3, 3, 1, 0, 1000)] * 6}
    c = _counters(hip, ks)
    assert c == {"runs": 10000, "run_leftover": 7000, "run_max_leftover": 7, "run_invalid": 0}
    for b in (1, 499, 999):
        for what in ("runs", "leftover"):
            assert np.array_equal(hip.debug_factor_updates(ks, b, what), hip.debug_factor_updates(ks, 0, what))
    desc, arr = _class_slices(hip, ks)
    assert int(hip.debug_counter(ks, "factor_classes")) == 1 and int(hip.debug_counter(ks, "factor_class_mismatches")) == 0
    assert int(hip.debug_counter(ks, "factor_class_verified")) == 1000
    chain = {k: hip.debug_kkt_ints(ks, k).astype(np.int64) for k in ("bundle_ptr", "blvl_ptr", "blvl", "Lp", "Up")}
    for b in (0, 1, 999):
        _check_bundle_against_class(hip, ks, b, desc[b], arr, chain)


def _class_slices(hip, ks):
    """-> (per-bundle records, the shared arrays) of the kernel's index data (csrc/host.hpp: fr_bdesc, fc_*)"""
    nb = _nbundles(hip, ks)
    desc = hip.debug_kkt_ints(ks, "factor_bundle_desc").astype(np.int64).reshape(nb, 64)
    arr = {k: hip.debug_kkt_ints(ks, "factor_class_" + k) for k in ("usr", "col", "sgn", "desc", "rec")}
    arr["usr"], arr["col"] = arr["usr"].view(np.uint32).astype(np.int64), arr["col"].view(np.uint32).astype(np.int64)
    return desc, arr


def _check_bundle_against_class(hip, ks, b, d, arr, chain):
    """what bundle b's record reaches in the shared arrays against the bundle's own data"""
    nl = d[6]
    assert 1 <= nl <= 17
    runs = hip.debug_factor_updates(ks, b, "runs").astype(np.int64)
    left = hip.debug_factor_updates(ks, b, "leftover").astype(np.int64)
    got = arr["desc"][8 * d[44]:8 * d[44 + nl]].astype(np.int64).reshape(-1, 8)
    lvl = np.repeat(np.arange(nl), np.diff(d[44:45 + nl]))
    s16 = lambda w: ((w & 0xFFFF) ^ 0x8000) - 0x8000  # noqa: E731  (signed 16 bit)
    mine = np.stack([lvl, got[:, 0], got[:, 1], got[:, 2], got[:, 3], s16(got[:, 4]), s16(got[:, 4] >> 16), s16(got[:, 5]),
                     s16(got[:, 5] >> 16), got[:, 6]], axis=1) if len(got) else np.zeros((0, 10), dtype=np.int64)
    assert np.array_equal(mine, runs), b
    rec = arr["rec"][4 * d[26]:4 * d[26 + nl]].astype(np.int64).reshape(-1, 4)
    rl = np.repeat(np.arange(nl), np.diff(d[26:27 + nl]))
    assert np.array_equal(np.concatenate([rl[:, None], rec], axis=1) if len(rec) else np.zeros((0, 5), dtype=np.int64), left), b
    assert d[8] == 0 and d[8 + nl] == d[1] and (np.diff(d[8:9 + nl]) > 0).all()
    if chain is not None:  # (handles that keep the arrays of the chain the record replaces)
        s0, s1 = chain["bundle_ptr"][b], chain["bundle_ptr"][b + 1]
        Lp, Up = chain["Lp"], chain["Up"]
        lv = chain["blvl"][chain["blvl_ptr"][b]:chain["blvl_ptr"][b + 1]]
        assert list(d[0:6]) == [s0, s1 - s0, Lp[s0], Lp[s1] - Lp[s0], Up[s0], Up[s1]]
        assert len(lv) == nl + 1 and list(d[8:9 + nl]) == list(lv - s0)
        col = arr["col"][d[62]:d[62] + d[1]]
        assert np.array_equal(col & 0xFFFF, Lp[s0:s1] - Lp[s0]) and np.array_equal(col >> 16, np.diff(Lp[s0:s1 + 1]))
        usr = arr["usr"][d[7]:d[7] + d[5] - d[4]]
        diag = Up[s0:s1] - Up[s0]  # (the first U entry of every row is its diagonal: slot 0xFFFF, row = the node)
        assert ((usr[diag] & 0xFFFF) == 0xFFFF).all() and np.array_equal(usr[diag] >> 16, np.arange(s1 - s0))
        assert ((np.delete(usr, diag) & 0xFFFF) < d[3]).all()
    assert set(arr["sgn"][d[62]:d[62] + d[1]]) <= {1, -1}


@pytest.mark.parametrize("nblocks,bs,shared", [(3, 64, True), (5, 341, True), (5, 341, False)])
def test_every_bundle_reads_its_classs_slices(hip, nblocks, bs, shared, monkeypatch):
    """the kernel's per-bundle record and the one copy of the index data per class of identical bundles: every bundle's
    runs, records outside runs, level tables, column table and U landing slots, read through its record, are its own;
    identical blocks make few classes, CHIP_NO_SHARED_PATTERN one per bundle"""
    if not shared:
        monkeypatch.setenv("CHIP_NO_SHARED_PATTERN", "1")  # (read when a handle is created)
    ks = _mk(hip, problems.portfolio_socp(nblocks, bs, seed=3))
    nb = _nbundles(hip, ks)
    desc, arr = _class_slices(hip, ks)
    chain = {k: hip.debug_kkt_ints(ks, k).astype(np.int64) for k in ("bundle_ptr", "blvl_ptr", "blvl", "Lp", "Up")}
    assert (len(chain["bundle_ptr"]) > 0) == (bs == 341)
    for b in range(nb):
        _check_bundle_against_class(hip, ks, b, desc[b], arr, chain if bs == 341 else None)
    ncls = int(hip.debug_counter(ks, "factor_classes"))
    print("portfolio_socp(%d, %d): %d bundles in %d classes" % (nblocks, bs, nb, ncls))
    assert int(hip.debug_counter(ks, "factor_class_verified")) == nb and int(hip.debug_counter(ks, "factor_class_mismatches")) == 0
    assert sorted(set(desc[:, 63])) == list(range(ncls))
    assert ncls == nb if not shared else ncls < nb
    if bs == 341 and shared:
        assert ncls == 1 and len(arr["desc"]) == 8 * (10 + 1)  # (one copy of ten runs + padding)
