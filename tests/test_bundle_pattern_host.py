"""CPU-side tests of the pattern classes of the bundles (symbolic.cpp: bundle_pattern_classes; host.hpp: PatternShare):
bundles whose node count, level table and 16-bit index slices are byte-equal share ONE copy of those slices in the fused
solve kernel.  Host-only handles: the classes, the size of the shared arrays and the byte-for-byte verification of every
bundle's offsets are host analysis."""
import pytest

from tests import problems
from tests.bundle_pattern_problems import two_sizes


def _mk(hip, pr):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    return hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=hip.Settings.default(device=hip.DEVICE_HOST_ONLY))


def _figures(hip, ks):
    names = ("classes", "bundles", "index_bytes", "full_index_bytes", "verified_bundles", "mismatches", "shared_bundles")
    return {k: int(hip.debug_counter(ks, "pattern_" + k)) for k in names}


def _block_entries(bs):
    """entries of L and of the U rows (K by rows, upper triangle) in the bundle of ONE block of `bs` variables, from the
    problem, not from the library's counters.  The bundle's 3 bs + 3 nodes: the variables, their Nonnegative rows, the
    bs + 1 rows of the cone and the two columns (u, v) of its sparse expansion.  K: 3 bs + 3 diagonal entries; per
    variable its entries in the budget row, its Nonnegative row and its cone row (3 bs); u and v against the bs + 1 cone
    rows (2 bs + 2): 8 bs + 5 (config 3: nnz(K) = 8 005 001 = 1000 x 8005 + the budget row's diagonal).  L: 6 bs + 5
    (config 3: nnz(L) = 6 005 000 = 1000 x 6005; the ordering's fill is the same per variable at every
    block size)."""
    return 6 * bs + 5, 8 * bs + 5


def _shared_bytes(block_sizes):
    """four 16-bit arrays (row and column of every entry of L, column and row of every entry of the U rows) over one
    bundle per distinct block size, each array with one entry of padding"""
    nl = sum(_block_entries(bs)[0] for bs in block_sizes)
    nu = sum(_block_entries(bs)[1] for bs in block_sizes)
    return 2 * (2 * (nl + 1) + 2 * (nu + 1))


def test_identical_blocks_are_one_class(hip):
    f = _figures(hip, _mk(hip, problems.portfolio_socp(6, 700, seed=11)))
    assert f["bundles"] == 6 and f["classes"] == 1, f
    assert f["index_bytes"] == _shared_bytes([700]), f
    assert f["full_index_bytes"] == 2 * (2 * (6 * _block_entries(700)[0] + 1) + 2 * (6 * _block_entries(700)[1] + 1)), f
    assert f["verified_bundles"] == 6 and f["mismatches"] == 0, f  # every bundle compared through its offsets
    assert f["shared_bundles"] == 0  # (a host-only handle launches nothing)


@pytest.mark.parametrize("shape", [(40, 1000), (12, 300)])
def test_other_shapes_of_the_workload_are_one_class(hip, shape):
    f = _figures(hip, _mk(hip, problems.portfolio_socp(shape[0], shape[1], seed=3)))
    assert f["bundles"] == shape[0] and f["classes"] == 1 and f["index_bytes"] == _shared_bytes([shape[1]]), f
    assert f["verified_bundles"] == shape[0] and f["mismatches"] == 0, f


def test_two_block_sizes_are_two_classes(hip):
    f = _figures(hip, _mk(hip, two_sizes(600, 700)))
    assert f["bundles"] == 6 and f["classes"] == 2, f
    assert f["index_bytes"] == _shared_bytes([600, 700]), f  # one bundle of each size
    assert f["verified_bundles"] == 6 and f["mismatches"] == 0, f


def test_a_banded_qp_shares_nothing(hip):
    """no bundles + folded top (no 16-bit index arrays at all), or bundles that all differ: nothing is built"""
    f = _figures(hip, _mk(hip, problems.random_qp(3000, 6000, band=30, seed=2)))
    assert f["index_bytes"] == 0 and f["shared_bundles"] == 0 and f["verified_bundles"] == 0, f
    assert f["classes"] in (0, f["bundles"]), f


def test_full_scale_workload_is_one_class(hip):
    """the benchmark's problem (config 3: 1000 x SOC(1001)): 1000 bundles, one pattern"""
    f = _figures(hip, _mk(hip, problems.portfolio_socp(1000, 1000, seed=3)))
    assert f["bundles"] == 1000 and f["classes"] == 1, f
    assert f["index_bytes"] == _shared_bytes([1000]) == 56048, f
    assert f["verified_bundles"] == 1000 and f["mismatches"] == 0, f
