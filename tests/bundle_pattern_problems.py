"""problems for the pattern classes of the bundles (tests/test_bundle_pattern_host.py, tests/test_bundle_pattern_gpu.py)"""
import numpy as np
import scipy.sparse as sp

from tests import problems


def portfolio_socp_sizes(sizes, seed=3):
    """problems.portfolio_socp with a size per block: cones [Zero(1) budget, NN(n), SOC(size + 1) per block] under ONE
    budget row -- blocks of different sizes give bundles of different index patterns"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    m = 1 + n + int((sizes + 1).sum())
    blk = np.repeat(np.arange(len(sizes)), sizes)         # block of every variable
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])  # first variable of every block
    row0 = 1 + n + np.concatenate([[0], np.cumsum(sizes + 1)[:-1]])  # first row of every block's cone
    j = np.arange(n)
    d = rng.uniform(0.5, 1.5, n)
    soc_rows = row0[blk] + 1 + (j - first[blk])
    rows = np.concatenate([np.zeros(n, dtype=np.int64), 1 + j, soc_rows])
    cols = np.concatenate([j, j, j])
    vals = np.concatenate([np.ones(n), -np.ones(n), -d])
    A = sp.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsc()
    cones = [(problems.ZERO, 1), (problems.NN, n)] + [(problems.SOC, int(s) + 1) for s in sizes]
    s, z = problems._interior(rng, cones, False)
    return dict(n=n, m=m, P=problems._csc(sp.csc_matrix((n, n))), A=problems._csc(A), cones=cones, s=s, z=z)


def two_sizes(small=600, large=700, seed=3):
    """3 blocks of `small` and 3 of `large` under one budget row: two pattern classes"""
    return portfolio_socp_sizes([small] * 3 + [large] * 3, seed=seed)
