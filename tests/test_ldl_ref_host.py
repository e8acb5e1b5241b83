"""tests/ldl_ref.py checked on the CPU: a plain float64 LDL' and substitution (sums in a shuffled order, pivots by
reciprocal and multiplication) stay inside the bounds; factors and solves that are wrong in ONE term leave them at the
entry concerned -- while the suite's max-norm check (relerr <= 1e-9, tests/test_gpu_parity.py) still accepts the same
factors: the gap that tests/test_ldl_backward_gpu.py closes.  No device: the handles are host-only (pattern and
permutation), the KKT values come from the CPU oracle.

Worst ratio of error to bound of the plain float64 LDL' (pytest -s prints them):

    fixture                                N     factor (c + 2) u T    dense form (bound doubled)   solve (rmax + cmax + 4) u t
    _rand_quasidef(30, 20, 0.1)            50    0.25                  0.15                         0.037
    _rand_quasidef(400, 300, 0.01)         700   0.32                  0.25                         0.011
    portfolio_socp(3, 65)                  595   0.31                  0.21                         0.0046
    portfolio_socp(3, 65, late=True)       595   0.27                  0.17                         0.0059

solve_check_visible on the two KKT fixtures (N = n + m + 6, another right-hand side): 0.0040 and 0.0040 with the hidden
components re-solved, 0.0044 and 0.0057 for solve_check on the full vector; a dropped visible contribution that the full
check sees at 9e9 / 1e13 of its bound shows at 9e9 / 2e12 in the visible rows: the form is sound, the fused cases of the
GPU tests use it.

The wrong factors (late-iterate fixture, max|L| = 9.1e5; ratio at the entry, then what the max norm of the suite sees):
one entry of L^ moved by 1e-12 relative 1.5e3, L 9e-13; one term left out / applied twice 7e4, L 2e-16, D 8e-16; D_j + 4 ulp
on a column without updates 1.33 (the bound there is 6 u |D_j|, 4 ulp are at most 8 u |D_j|), D 3e-17.  The wrong solves:
a forward contribution dropped 1.5e3 (max norm against the right solve 6e-11), a backward one 1.3e6 (3e-9)."""
import numpy as np
import pytest

from tests import ldl_ref as R
from tests import problems
from tests.test_gpu_parity import _rand_quasidef

TOL_X = 1e-6                # the tighter of the suite's two bounds on an unrefined solve (tests/test_gpu_parity.py)
TOL_L, TOL_D = 1e-9, 1e-10  # the factor-parity bounds of the suite (tests/test_gpu_parity.py, tests/test_factor_runs_gpu.py)


class Fixture:
    """K (lower, permuted), the pattern of its factor, a plain factor and a right-hand side over eight decades"""

    def __init__(self, name, Kl, Lp, Li, hidden=None):
        self.name, self.K, self.Lp, self.Li, self.N = name, Kl, Lp, Li, Kl.shape[0]
        self.hidden = hidden
        self.rng = np.random.default_rng(5)
        self.Lx, self.D = R.plain_ldl(Kl, Lp, Li, self.rng)
        self.cols = np.repeat(np.arange(self.N), np.diff(Lp))
        self.b = self.rng.standard_normal(self.N) * 10.0 ** self.rng.uniform(-4, 4, self.N)

    def factor_check(self, Lx=None, D=None, **kw):
        return R.factor_check(self.N, self.Lp, self.Li, self.Lx if Lx is None else Lx, self.D if D is None else D, self.K, **kw)

    def ratio_at(self, fc, i, j):
        return float(fc["ratio"][(fc["rows"] == i) & (fc["cols"] == j)][0])


def _l1(hip, n1, n2, density, seed):
    K, ds = _rand_quasidef(np.random.default_rng(seed), n1, n2, density)
    Kc = hip.CscMatrix.from_scipy(K)
    f = hip.HipDirectLDLSolver(Kc, ds, hip.Settings.default(device=hip.DEVICE_HOST_ONLY))
    _, Lp, Li, _ = f.symbolic()
    return Fixture("quasidef(%d, %d)" % (n1, n2), R.lower_permuted(n1 + n2, Kc.colptr, Kc.rowval, Kc.nzval, f.perm), Lp, Li)


def _kkt(hip, oracle, name, pr):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=hip.Settings.default(device=hip.DEVICE_HOST_ONLY))
    cones = oracle.Cones(pr["cones"])
    assert cones.update_scaling(pr["s"], pr["z"])
    ko = oracle.KKTSolver(pr["n"], pr["m"], pr["P"], pr["A"], cones, perm=ks.perm)
    assert ko.update()
    K, mp = ks.kkt_matrix(), ks.maps()
    assert np.array_equal(K.colptr, ko.kkt.colptr) and np.array_equal(K.rowval, ko.kkt.rowval)
    v = np.array(ko.kkt.nzval)
    v[mp["diag_full"]] = v[mp["diag_full"]] + mp["dsigns"] * ko.regularizer
    _, Lp, Li, _ = ks.symbolic()
    iperm = np.empty(ks.N, dtype=np.int64)
    iperm[ks.perm] = np.arange(ks.N)
    return Fixture(name, R.lower_permuted(ks.N, K.colptr, K.rowval, v, ks.perm), Lp, Li, hidden=iperm[ks.n + ks.m:])


@pytest.fixture(scope="module")
def fixtures(hip, oracle):
    return {"q30": _l1(hip, 30, 20, 0.1, 0), "q400": _l1(hip, 400, 300, 0.01, 1),
            "socp": _kkt(hip, oracle, "portfolio_socp(3, 65)", problems.portfolio_socp(3, 65, seed=3)),
            "late": _kkt(hip, oracle, "portfolio_socp(3, 65, late)", problems.portfolio_socp(3, 65, seed=3, late=True))}


@pytest.mark.parametrize("which", ["q30", "q400", "socp", "late"])
def test_plain_ldl_stays_within_the_bounds(fixtures, which):
    fx = fixtures[which]
    fc, fd = fx.factor_check(), fx.factor_check(dense=True)
    x = R.plain_solve(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, fx.rng)
    sc = R.solve_check(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, x)
    print("%s: N %d, nnz(L) %d, max|L| %.2e: factor %.3f at %s, dense form %.3f, solve %.4f (rmax %d, cmax %d)"
          % (fx.name, fx.N, len(fx.Li), np.abs(fx.Lx).max(), fc["worst"], fc["at"], fd["worst"], sc["worst"], sc["rmax"], sc["cmax"]))
    assert fc["worst"] < 1.0 and fd["worst"] < 1.0 and sc["worst"] < 1.0
    assert len(fc["ratio"]) == fx.N + len(fx.Li) and np.all(fc["c"] >= 1)


def _update_terms(fx, j):
    """the update terms L_ik D_k L_jk, k < j, of the entries (i, j) of column j -> [(|term|, i, k), ...]"""
    L = R.unit_lower(fx.N, fx.Lp, fx.Li, fx.Lx).tocsr()
    out = []
    ks = L[j].indices[L[j].indices < j]
    for i in np.concatenate([[j], fx.Li[fx.Lp[j]:fx.Lp[j + 1]]]):
        for k in np.intersect1d(ks, L[i].indices):
            out.append((abs(L[i, k] * fx.D[k] * L[j, k]), int(i), int(k)))
    return out


def _a_small_term(fx, fc):
    """a column whose smallest update term is far above the bound of its entry and far below what the max norm sees"""
    lmax = max(1.0, np.abs(fx.Lx).max())
    for j in np.argsort(-np.diff(fx.Lp)):
        terms = [t for t in _update_terms(fx, j) if t[0] > 0.0]
        if len(terms) < 2:
            continue
        size, i, k = min(terms)
        sel = (fc["rows"] == i) & (fc["cols"] == j)
        bound = float(((fc["c"][sel] + 2.0) * R.U * fc["T"][sel])[0])
        if size > 100.0 * bound and size / abs(fx.D[j]) < 1e-3 * TOL_L * lmax and size < 1e-3 * TOL_D * max(1.0, np.abs(fx.D).max()):
            return i, int(j), k, size
    raise AssertionError("no column with a term between the two checks")


def _max_norm_accepts(fx, Lx, D):
    return R.relerr(Lx, fx.Lx) <= TOL_L and R.relerr(D, fx.D) <= TOL_D


@pytest.mark.parametrize("wrong", ["entry_1e-12", "term_left_out", "term_twice", "pivot_4ulp"])
def test_wrong_factors_are_caught_where_the_max_norm_is_blind(fixtures, wrong):
    fx = fixtures["late"]
    fc0 = fx.factor_check()
    Lx, D = fx.Lx.copy(), fx.D.copy()
    if wrong == "entry_1e-12":
        p = int(np.argmax(np.abs(fx.Lx) * (np.diff(fx.Lp)[fx.cols] > 1)))
        i, j = int(fx.Li[p]), int(fx.cols[p])
        Lx[p] *= 1.0 + 1e-12
    elif wrong == "pivot_4ulp":
        # (a column without updates: c = 1, D_j = K_jj, T_jj = 2 |D_j|, the bound 6 u |D_j|; 4 ulp are 8 u |D_j| over the
        # mantissa of D_j in [1, 2): the column with the smallest mantissa, where they are nearly 8 u |D_j|)
        leaves = np.flatnonzero(fc0["c"][:fx.N] == 1)
        j = int(leaves[np.argmin(np.frexp(np.abs(D[leaves]))[0])])
        i = j
        assert 2.0 * np.frexp(abs(D[j]))[0] < 1.25
        D[j] += 4.0 * np.spacing(D[j])
    else:
        i, j, k, size = _a_small_term(fx, fc0)
        kw = {"skip": (i, j, k)} if wrong == "term_left_out" else {"twice": (i, j, k)}
        Lx, D = R.plain_ldl(fx.K, fx.Lp, fx.Li, np.random.default_rng(5), **kw)
    fc = fx.factor_check(Lx, D)
    here = fx.ratio_at(fc, i, j)
    print("%s at (%d, %d): ratio %.3g there (%.3g before), worst %.3g at %s; max norm: L %.2e, D %.2e"
          % (wrong, i, j, here, fx.ratio_at(fc0, i, j), fc["worst"], fc["at"], R.relerr(Lx, fx.Lx), R.relerr(D, fx.D)))
    assert fc0["worst"] < 1.0
    assert here > 1.0 and fc["worst"] > 1.0
    assert _max_norm_accepts(fx, Lx, D)


@pytest.mark.parametrize("sweep", ["forward", "backward"])
def test_wrong_solves_are_caught(fixtures, sweep):
    """one contribution of a sweep dropped: far above the bound of its row, and within TOL_X of the right solve in the
    max norm"""
    fx = fixtures["late"]
    x0 = R.plain_solve(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, np.random.default_rng(1))
    found = None
    for p in np.argsort(np.abs(fx.Lx)):
        if fx.Lx[p] == 0.0:
            continue
        kw = {"skip_fwd": int(p)} if sweep == "forward" else {"skip_bwd": int(p)}
        x = R.plain_solve(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, np.random.default_rng(1), **kw)
        sc = R.solve_check(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, x)
        if sc["worst"] > 1.0 and R.relerr(x, x0) <= TOL_X:
            found = (p, sc, R.relerr(x, x0))
            break
    assert found is not None, "no dropped contribution between the two checks"
    p, sc, err = found
    row = int(fx.Li[p]) if sweep == "forward" else int(fx.cols[p])
    print("%s sweep without L[%d, %d] = %.3e: ratio %.3g at row %d (worst %.3g at %d); max norm against the right solve %.2e"
          % (sweep, fx.Li[p], fx.cols[p], fx.Lx[p], sc["ratio"][row], row, sc["worst"], sc["at"], err))
    assert R.solve_check(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, x0)["worst"] < 1.0
    assert sc["ratio"][row] > 1.0


@pytest.mark.parametrize("which", ["socp", "late"])
def test_visible_form_agrees_with_the_full_one(fixtures, which):
    fx = fixtures[which]
    N, H = fx.N, np.sort(fx.hidden)
    assert len(H) == 6  # two per sparse second-order cone
    V = np.setdiff1d(np.arange(N), H)
    rng = np.random.default_rng(9)
    b = rng.standard_normal(N) * 10.0 ** rng.uniform(-4, 4, N)
    b[H] = 0.0  # (as setrhs leaves the hidden rows)
    x = R.plain_solve(N, fx.Lp, fx.Li, fx.Lx, fx.D, b, np.random.default_rng(2))
    full = R.solve_check(N, fx.Lp, fx.Li, fx.Lx, fx.D, b, x)
    vis = R.solve_check_visible(N, fx.Lp, fx.Li, fx.Lx, fx.D, b, x[V], H)
    print("%s: full %.4f, visible rows with the hidden components re-solved %.4f" % (fx.name, full["worst"], vis["worst"]))
    assert full["worst"] < 1.0 and vis["worst"] < 1.0
    # a visible contribution dropped: the first sweep entry, smallest first, that the full check catches at a visible row
    for p in np.argsort(np.abs(fx.Lx)):
        if fx.Lx[p] == 0.0 or fx.Li[p] in H or fx.cols[p] in H:
            continue
        xw = R.plain_solve(N, fx.Lp, fx.Li, fx.Lx, fx.D, b, np.random.default_rng(2), skip_fwd=int(p))
        fw = R.solve_check(N, fx.Lp, fx.Li, fx.Lx, fx.D, b, xw)
        if fw["ratio"][fx.Li[p]] > 4.0:
            break
    else:
        raise AssertionError("no dropped contribution above the bound")
    vw = R.solve_check_visible(N, fx.Lp, fx.Li, fx.Lx, fx.D, b, xw[V], H)
    print("%s: forward sweep without L[%d, %d]: full %.3g, visible %.3g" % (fx.name, fx.Li[p], fx.cols[p], fw["worst"], vw["worst"]))
    assert vw["worst"] > 1.0


@pytest.mark.parametrize("what", ["one_L", "one_D", "all"])
@pytest.mark.parametrize("dense", [False, True])
def test_non_finite_factor_entries_are_caught(fixtures, what, dense):
    """a NaN or Inf left in a factor is an error of any size: ratio inf at its entry, never a pass"""
    fx = fixtures["q400"]
    for bad in (np.nan, np.inf):
        Lx, D = fx.Lx.copy(), fx.D.copy()
        p, j = len(Lx) // 2, fx.N // 3
        if what == "one_L":
            Lx[p] = bad
            i, j = int(fx.Li[p]), int(fx.cols[p])
        elif what == "one_D":
            D[j] = bad
            i = j
        else:
            Lx[:], D[:] = bad, bad
            i = j
        fc = fx.factor_check(Lx, D, dense=dense)
        assert fc["worst"] == np.inf and fx.ratio_at(fc, i, j) == np.inf, (what, bad, fc["worst"])


@pytest.mark.parametrize("what", ["one", "all"])
def test_non_finite_solution_components_are_caught(fixtures, what):
    fx = fixtures["late"]
    H = np.sort(fx.hidden)
    V = np.setdiff1d(np.arange(fx.N), H)
    x0 = R.plain_solve(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, np.random.default_rng(1))
    for bad in (np.nan, -np.inf):
        x = x0.copy()
        k = int(V[len(V) // 2])
        if what == "one":
            x[k] = bad
        else:
            x[:] = bad
        sc = R.solve_check(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, x)
        assert sc["worst"] == np.inf and sc["ratio"][k] == np.inf, (what, bad, sc["worst"])
        vis = R.solve_check_visible(fx.N, fx.Lp, fx.Li, fx.Lx, fx.D, fx.b, x[V], H)
        assert vis["worst"] == np.inf, (what, bad, vis["worst"])
