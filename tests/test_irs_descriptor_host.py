"""CPU-side test of the per-bundle records of the fused solve kernel k_bundle_irs (csrc/kernels.hpp: IrsDesc; built once per
handle by kkt_create.cpp: irs_descriptors): every record must say exactly what the kernel's chained prologue finds by walking
bundle_ptr, blvl_ptr -> blvl -> Lp, Up, run_ptr -> runs and the pattern offsets.  Host-only handles: the records and the
arrays of the chain are host analysis (include/clarabel_hip_testing.h: chip_debug_kkt_ints)."""
import numpy as np
import pytest

from tests import problems
from tests.bundle_pattern_problems import two_sizes

DESC_INTS = 128                     # sizeof(IrsDesc) / 4
HEAD, LEVELS, RUNS = 12, 20, 32     # ints of the head, level entries, runs a record holds
CHAIN = ("bundle_ptr", "blvl_ptr", "blvl", "Lp", "Up", "run_ptr", "runs", "pat_off")


def _mk(hip, pr):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    return hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=hip.Settings.default(device=hip.DEVICE_HOST_ONLY))


def _from_chain(c, b):
    """the record of bundle b as the chained prologue of the kernel (and irs_symv / the sweeps behind it) reads it"""
    d = np.zeros(DESC_INTS, dtype=np.int64)
    s0, s1 = c["bundle_ptr"][b], c["bundle_ptr"][b + 1]
    lv = c["blvl"][c["blvl_ptr"][b]:c["blvl_ptr"][b + 1]]
    nl = len(lv) - 1
    nleaf = lv[1] - s0
    r0, r1 = c["run_ptr"][b], c["run_ptr"][b + 1]
    assert 1 <= nl <= LEVELS - 1 and 1 <= r1 - r0 <= RUNS
    d[0:4] = (s0, s1 - s0, nleaf, nl)
    if len(c["pat_off"]):
        d[4:6] = c["pat_off"][2 * b:2 * b + 2]
    d[6:8] = (c["Up"][s0 + nleaf], c["Up"][s1])
    d[8] = r1 - r0
    d[HEAD:HEAD + nl + 1] = c["Lp"][lv]
    d[HEAD + LEVELS:HEAD + LEVELS + 3 * (r1 - r0)] = c["runs"][3 * r0:3 * r1]
    return d


def _check(hip, ks, shared):
    c = {k: hip.debug_kkt_ints(ks, k).astype(np.int64) for k in CHAIN}
    nb = len(c["bundle_ptr"]) - 1
    assert nb >= 1 and (len(c["pat_off"]) == 2 * nb) == shared
    desc = hip.debug_kkt_ints(ks, "irs_desc").astype(np.int64).reshape(nb, DESC_INTS)
    for b in range(nb):
        want = _from_chain(c, b)
        assert np.array_equal(desc[b], want), (b, np.nonzero(desc[b] != want)[0])
    return c, desc


def _levels(desc):
    """entries of L per level of bundle 0"""
    nl = desc[0, 3]
    return list(np.diff(desc[0, HEAD:HEAD + nl + 1]))


@pytest.mark.parametrize("bs", [170, 341, 512, 1023])
def test_records_equal_the_chain(hip, bs):
    """portfolio_socp(nblocks, bs): a bundle has 3 bs + 3 nodes, the first bs + 1 of them leaves; its five levels hold
    bs + 2, 2 bs, 3 bs, 2 and 1 entries of L (printed below; the elimination order decides it).  The edge cases the GPU
    test (tests/test_irs_ahead_gpu.py) relies on, with batches of 256 threads x 4 = 1024 entries:
    bs = 170: the smallest bundle k_bundle_irs takes (513 >= 512 nodes);
    bs = 341: a level of 1023 entries, one slot of the batch empty;
    bs = 512: a level of exactly 1024 entries, so the batch after it belongs to the next level;
    bs = 1023: a level of 1025 entries, one entry in a second batch; 3072 nodes, every thread's 12 slots full; 1024 leaves,
    all the kernel allows."""
    ks = _mk(hip, problems.portfolio_socp(5, bs, seed=3))
    assert hip.debug_counter(ks, "pattern_classes") == 1
    c, desc = _check(hip, ks, shared=True)
    lev = _levels(desc)
    print("bs = %d: nodes %d, leaves %d, entries per level %s, runs %d" % (bs, desc[0, 1], desc[0, 2], lev, desc[0, 8]))
    assert desc[0, 1] == 3 * bs + 3 and desc[0, 2] == bs + 1
    assert lev == [bs + 2, 2 * bs, 3 * bs, 2, 1]
    edge = {170: desc[0, 1] == 513, 341: 1023 in lev, 512: 1024 in lev,
            1023: 1025 in lev and desc[0, 1] == 12 * 256 and desc[0, 2] == 4 * 256}
    assert edge[bs]
    assert (desc[:, 1] == desc[0, 1]).all() and len(set(map(tuple, desc[:, 4:6]))) == len(desc)  # (one class, own offsets)


def test_two_classes_have_different_records(hip):
    ks = _mk(hip, two_sizes(600, 700))
    assert hip.debug_counter(ks, "pattern_classes") == 2
    c, desc = _check(hip, ks, shared=True)
    assert sorted(set(desc[:, 1])) == [1803, 2103] and sorted(set(desc[:, 2])) == [601, 701]


def test_own_copies_have_zero_offsets(hip, monkeypatch):
    monkeypatch.setenv("CHIP_NO_SHARED_PATTERN", "1")  # (read when a handle is created)
    ks = _mk(hip, problems.portfolio_socp(5, 341, seed=3))
    c, desc = _check(hip, ks, shared=False)
    assert (desc[:, 4:6] == 0).all()
