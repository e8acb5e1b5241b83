"""tests/spmv_ref.py on the CPU: the term lists against dense products, the symmetric use of P's off-diagonals, the
exactness of the integer family, the row lengths the problem builders declare, and compare() itself -- it accepts a plain
numpy evaluation of the pass in another summation order and refuses the wrong passes that
tests/test_residual_passes_gpu.py is there to catch."""
import math

import numpy as np
import pytest

from tests import spmv_ref as R


def small_problem(n, m, seed, with_p=True):
    """random patterns with an empty row and column of P, empty rows and an empty column of A"""
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((n, n)) < 0.4)
    mask[:, n // 2] = mask[n // 2, :] = False
    if not with_p:
        mask[:] = False
    r, c = np.nonzero(mask)
    P = R._csc(n, n, r, c)
    amask = rng.random((m, n)) < 0.5
    amask[m // 3, :] = False
    amask[:, n - 1] = False
    r, c = np.nonzero(amask)
    return R._problem(n, m, P, R._csc(m, n, r, c))


def numpy_pass(pr, v, rows_dropped=(), skip_empty=False, ignore_alpha=False, zero_aux_rows=()):
    """the residual pass in plain numpy (np.bincount accumulates entry by entry, np.dot pairwise: other orders than
    fsum's), with the device pass's ways of being wrong on request"""
    n, m = pr["n"], pr["m"]
    x, z, s, tau = v["x"], v["z"], v["s"], v["tau"]
    pr_, pc_ = pr["P"][1], R._cols_of(pr["P"][0])
    ar, ac = pr["A"][1], R._cols_of(pr["A"][0])
    off = pr_ != pc_
    Px = np.bincount(np.concatenate([pr_, pc_[off]]), np.concatenate([v["Pv"] * x[pc_], v["Pv"][off] * x[pr_[off]]]), n).astype(float)
    atz = np.bincount(ac, v["Av"] * z[ar], n)
    keep = np.ones(len(ar), dtype=bool)
    for i in rows_dropped:  # the last entry of row i of A is left out
        keep[np.flatnonzero(ar == i)[-1]] = False
    ax = np.bincount(ar[keep], (v["Av"] * x[ac])[keep], m)
    aux = s.copy()
    aux[list(zero_aux_rows)] = 0.0
    got = dict(Px=Px, rx_inf=0.0 + (atz if ignore_alpha else -atz), rz_inf=ax + aux)
    if skip_empty:  # what the caller's buffer held before stays in the empty rows
        got["Px"] = np.where(R.psym_row_lengths(pr) == 0, np.nan, got["Px"])
        got["rx_inf"] = np.where(R.a_col_lengths(pr) == 0, np.nan, got["rx_inf"])
        got["rz_inf"] = np.where(R.a_row_lengths(pr) == 0, np.nan, got["rz_inf"])
    got["rx"] = got["rx_inf"] - got["Px"] - tau * v["q"]
    got["rz"] = got["rz_inf"] - tau * v["b"]
    got.update(dot_qx=float(np.dot(v["q"], x)), dot_bz=float(np.dot(v["b"], z)), dot_sz=float(np.dot(s, z)),
               dot_xPx=float(np.dot(x, Px)) if len(pr_) else 0.0)
    got["rtau"] = got["dot_qx"] + got["dot_bz"] + v["kappa"] + got["dot_xPx"] / tau
    got["norms"] = tuple(math.sqrt(float(np.dot(a, a))) for a in (x, z, s, got["rz"], got["rx"]))
    return got


@pytest.fixture(scope="module")
def rows_pr():
    return R.rows_problem()


@pytest.mark.parametrize("seed", range(4))
def test_term_lists_against_dense_products(seed):
    pr = small_problem(9 + seed, 7 + 2 * seed, seed)
    for exact, v in ((True, R.integer_point(pr, seed)), (False, R.wide_point(pr, seed))):
        P, A = R.dense(pr, v)
        x, z, s, tau = v["x"], v["z"], v["s"], v["tau"]
        dense = {"Px": P @ x, "rx_inf": -(A.T @ z), "rz_inf": A @ x + s, "rx": -(A.T @ z) - P @ x - tau * v["q"],
                 "rz": A @ x + s - tau * v["b"]}
        ref = R.reference(pr, v)
        for key in R.OUTPUTS:
            want, bound, L = ref[key]
            assert want.shape == dense[key].shape
            if exact:
                assert R.same_bits(want, dense[key] + 0.0), key
            else:
                assert np.all(np.abs(want - dense[key]) <= bound), key
        # the counts: entries of the row (P symmetric) and the aux / q / b terms
        full = (P != 0).sum(axis=1)
        arow, acol = (A != 0).sum(axis=1), (A != 0).sum(axis=0)
        assert list(ref["Px"][2]) == list(full) and list(ref["rx_inf"][2]) == list(acol)
        assert list(ref["rz_inf"][2]) == list(arow + 1) and list(ref["rx"][2]) == list(acol + full + 1)
        assert list(ref["rz"][2]) == list(arow + 2)
        assert full[pr["n"] // 2] == 0 and acol[-1] == 0 and arow[pr["m"] // 3] == 0  # the empty ones are there


def test_offdiagonal_of_p_is_used_twice():
    # P = [[1, 2], [2, 3]] stored as its upper triangle; A = [[5, 0]]
    pr = R._problem(2, 1, (np.array([0, 1, 3]), np.array([0, 0, 1])), (np.array([0, 1, 1]), np.array([0])))
    assert list(R.psym_row_lengths(pr)) == [2, 2]
    x, z, s = np.array([10.0, 100.0]), np.array([7.0]), np.array([0.5])
    full = R.with_values(pr, dict(Pv=np.array([1.0, 2.0, 3.0]), Av=np.array([5.0]), q=np.array([1.0, 1.0]), b=np.array([4.0])))
    terms, ptr = R.term_lists(full, x, z, s, 2.0)["Px"]
    assert list(ptr) == [0, 2, 4]
    assert sorted(terms[0:2]) == [10.0, 200.0] and sorted(terms[2:4]) == [20.0, 300.0]
    ref = R.row_terms(full, x, z, s, 2.0)
    assert list(ref["Px"][0]) == [210.0, 320.0] and list(ref["rx_inf"][0]) == [-35.0, 0.0]
    assert list(ref["rz_inf"][0]) == [50.5] and list(ref["rx"][0]) == [-247.0, -322.0] and list(ref["rz"][0]) == [42.5]
    assert list(ref["rx_inf"][2]) == [1, 0] and ref["rx_inf"][1][1] == 0.0  # an empty row: no term, no allowance


def test_fsum_groups_is_fsum():
    rng = np.random.default_rng(3)
    lens = np.array([0, 1, 2, 3, 2, 0, 7, 1, 40])
    ptr = np.concatenate([[0], np.cumsum(lens)])
    t = rng.standard_normal(ptr[-1]) * 10.0 ** rng.uniform(-12, 12, ptr[-1])
    assert list(R.fsum_groups(t, ptr)) == [math.fsum(t[a:b].tolist()) for a, b in zip(ptr[:-1], ptr[1:])]


def test_integer_family_is_exact(rows_pr):
    for pr in (rows_pr, R.cols_problem(), R.vector_problem(257, 257)):
        v = R.integer_point(pr, 5)
        for key in ("Pv", "Av", "q", "b", "x", "z", "s"):
            assert np.all(np.isin(np.abs(v[key]), (1.0, 2.0, 3.0, 4.0))), key
        assert v["tau"] == 2.0 and all(v[k][-1] == 4.0 for k in ("q", "b", "x", "z", "s"))
        full = R.with_values(pr, v)
        lists = R.term_lists(full, v["x"], v["z"], v["s"], v["tau"])
        ref = R.row_terms(full, v["x"], v["z"], v["s"], v["tau"])
        for key, (terms, ptr) in lists.items():
            assert np.all(terms == np.round(terms))
            ints = np.add.reduceat(np.concatenate([terms.astype(np.int64), [0]]), ptr[:-1])  # exact integer sums
            ints[np.diff(ptr) == 0] = 0
            assert np.array_equal(ref[key][0], ints.astype(float)), key
            assert np.max(np.add.reduceat(np.concatenate([np.abs(terms), [0.0]]), ptr[:-1])) < 2.0 ** 30
        for a, b in (("q", "x"), ("b", "z"), ("s", "z"), ("x", "x")):
            assert R.dot_ref(v[a], v[b])[0] == float(sum(int(p) * int(q) for p, q in zip(v[a], v[b])))


def test_last_entry_of_every_long_row_weighs_most(rows_pr):
    """the last entry of every row of more than T_MAX entries -- rows of A, columns of A, rows of the symmetric P --
    is +-4 and contributes +4 |x_j| (or +4 |z_i|)"""
    seen = 0
    for pr in (rows_pr, R.cols_problem(), R.vector_problem(5, 400)):
        v = R.integer_point(pr, 9)
        ar, ac = pr["A"][1], R._cols_of(pr["A"][0])
        for i in np.flatnonzero(R.a_row_lengths(pr) > R.T_MAX):
            k = np.flatnonzero(ar == i)
            last = k[np.argmax(ac[k])]
            assert abs(v["Av"][last]) == 4.0 and v["Av"][last] * v["x"][ac[last]] == 4.0 * abs(v["x"][ac[last]])
            seen += 1
        for j in np.flatnonzero(R.a_col_lengths(pr) > R.T_MAX):
            last = pr["A"][0][j + 1] - 1  # rows ascend inside a column
            assert abs(v["Av"][last]) == 4.0 and v["Av"][last] * v["z"][ar[last]] == 4.0 * abs(v["z"][ar[last]])
            seen += 1
        r, c = pr["P"][1], R._cols_of(pr["P"][0])
        for i in np.flatnonzero(R.psym_row_lengths(pr) > R.T_MAX) if len(r) else ():
            k = np.flatnonzero((r == i) | (c == i))
            other = np.where(r[k] == i, c[k], r[k])
            last = k[np.argmax(other)]
            assert abs(v["Pv"][last]) == 4.0 and v["Pv"][last] * v["x"][np.max(other)] == 4.0 * abs(v["x"][np.max(other)])
            seen += 1
    assert seen == 21 + 2 + 4 + 5  # rows of A and of P in rows_problem, columns of A in cols_problem and in the 400 x 5


def test_declared_row_lengths_are_produced(rows_pr):
    pr = rows_pr
    assert (pr["n"], pr["m"]) == (21600, 26)
    assert list(R.a_row_lengths(pr)) == R.ROW_LENGTHS  # counted from rowval
    assert int(np.max(R.a_col_lengths(pr))) <= 26
    ps = R.psym_row_lengths(pr)
    assert ps[0] == pr["n"] - 1 and ps[R.P_WAVE_ROW] == 2 + R.P_WAVE_OFFDIAG and ps[R.P_EMPTY] == 0
    assert sorted(set(ps)) == [0, 2, 3, 302, 21599]
    r, c = pr["P"][1], R._cols_of(pr["P"][0])
    assert not np.any(r == R.P_EMPTY) and not np.any(c == R.P_EMPTY) and np.all(r <= c)
    # the classes and the chunks of the workgroup rows: one chunk of a single entry, one of exactly B_CHUNK, a ragged one
    assert [R.row_class(k) for k in (0, 32, 33, 16384, 16385)] == ["thread", "thread", "wavefront", "wavefront", "workgroup"]
    assert R.chunk_lengths(16385)[-1] == 1 and R.chunk_lengths(20480) == [4096] * 5 and R.chunk_lengths(21503)[-1] == 1023
    assert R.chunk_lengths(21599)[-1] == 1119 and R.chunk_lengths(16384) == []
    # thread rows of the symmetric P behind chunk and wavefront blocks: not a multiple of 8 workgroups of 256
    assert int(np.sum(ps <= R.T_MAX)) == 21598 and 21598 % (8 * 256) != 0
    pc = R.cols_problem()
    assert (pc["n"], pc["m"]) == (6, 21600) and list(R.a_col_lengths(pc)) == R.COL_LENGTHS  # from colptr
    assert len(pc["P"][1]) == 0 and list(pc["P"][0]) == [0] * 7
    rl = R.a_row_lengths(pc)
    assert int(np.max(rl)) <= 6 and int(np.sum(rl == 0)) > 0 and len(rl) == 21600
    for n in (1, 257):
        pv = R.vector_problem(n, n)
        assert list(R.a_row_lengths(pv)) == [1] * n and list(R.a_col_lengths(pv)) == [1] * n
        assert list(R.psym_row_lengths(pv)) == [1] * n
    pv = R.vector_problem(3, 7)
    assert list(R.a_row_lengths(pv)) == [1] * 7 and list(R.a_col_lengths(pv)) == [3, 2, 2]


@pytest.mark.parametrize("which", ["rows", "cols", "vector"])
def test_compare_accepts_another_summation_order(rows_pr, which):
    pr = rows_pr if which == "rows" else R.cols_problem() if which == "cols" else R.vector_problem(1000, 1000)
    for exact, v in ((True, R.integer_point(pr, 1)), (False, R.wide_point(pr, 2))):
        ratios, fails = R.compare(pr, v, numpy_pass(pr, v), exact)
        assert not fails, fails
        assert set(ratios) == set(R.OUTPUTS) | {"dot_qx", "dot_bz", "dot_sz", "dot_xPx"} | {"norm_" + k for k in R.NORMS}
        assert all(0.0 <= r <= 1.0 for r in ratios.values())
        if exact:
            assert all(r == 0.0 for r in ratios.values())


@pytest.mark.parametrize("wrong", [dict(rows_dropped=(9, 21)), dict(skip_empty=True), dict(ignore_alpha=True),
                                   dict(zero_aux_rows=(21, 25))], ids=lambda d: next(iter(d)))
def test_compare_refuses_a_wrong_pass(rows_pr, wrong):
    """the last entry of a wavefront row (192 entries) and of a workgroup row (16385: the chunk of one entry) dropped; empty
    rows never written; alpha ignored; aux missing from two workgroup rows.  The integer family shows each of them; the
    wide family those that do not hide below a long row's rounding (a lost entry of 1e-6 beside entries of 1e6 does)"""
    pr = rows_pr
    for exact, v in ((True, R.integer_point(pr, 1)), (False, R.wide_point(pr, 2))):
        ratios, fails = R.compare(pr, v, numpy_pass(pr, v, **wrong), exact)
        key = "rx_inf" if "ignore_alpha" in wrong else "rz_inf"
        if exact or "skip_empty" in wrong or "ignore_alpha" in wrong:
            assert any(f.startswith(key) for f in fails), (wrong, fails)
        if "skip_empty" in wrong:
            assert any(f.startswith("Px[%d]" % R.P_EMPTY) for f in fails) and any(f.startswith("rz_inf[0]") for f in fails)


def test_compare_refuses_wrong_scalars(rows_pr):
    pr = rows_pr
    v = R.wide_point(pr, 2)
    good = numpy_pass(pr, v)
    for name in ("dot_qx", "dot_bz", "dot_sz", "dot_xPx", "rtau"):
        bad = dict(good, **{name: good[name] * (1.0 + 1e-9)})
        fails = R.compare(pr, v, bad, False)[1]
        assert any(f.startswith(name) or (name != "dot_sz" and f.startswith("rtau")) for f in fails), (name, fails)
    for k, name in enumerate(R.NORMS):
        nrm = list(good["norms"])
        nrm[k] *= 1.0 + 1e-9
        fails = R.compare(pr, v, dict(good, norms=tuple(nrm)), False)[1]
        assert [f.split(":")[0] for f in fails] == ["norm_" + name]
    pc = R.cols_problem()
    vc = R.integer_point(pc, 1)
    good = numpy_pass(pc, vc)
    assert not R.compare(pc, vc, good, True)[1]
    neg = good["Px"].copy()
    neg[0] = -0.0
    assert R.compare(pc, vc, dict(good, Px=neg), True)[1]  # a signed zero is not the reference's bits
