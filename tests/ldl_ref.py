"""Componentwise backward-error bounds for an LDL' factor and for the substitutions through it (numpy and scipy only, no
device; tests/test_ldl_ref_host.py checks this module on the CPU, tests/test_ldl_backward_gpu.py uses it on the handles).

Notation: (Lp, Li) the CSC pattern of the strictly lower triangle of L^ in the permuted numbering, Lx its values, D^ the
pivots, L^ with a unit diagonal, K the matrix the handle was given in the same numbering (lower triangle), u = 2^-53.
Everything is measured against the handle's OWN factor, so no second factorisation's rounding enters, and every bound is
per entry: no flat tolerance, no norm over the factor.

factor_check: for every stored position (i, j), i >= j, of the pattern (diagonal included)

    R_ij = |K_ij - sum_{k <= j} L^_ik D^_k L^_jk|           (K_ij = 0 where K stores nothing)
    T_ij = |K_ij| + sum_{k <= j} |L^_ik| |D^_k| |L^_jk|
    c_ij = number of structural k in that sum                (pattern . pattern', the diagonal counts)
    ratio_ij = R_ij / ((c_ij + 2) u T_ij)

Derivation (Higham, Accuracy and Stability of Numerical Algorithms, ch. 8 and 10; first order in u): the entry is computed
as L^_ij = fl(fl(K_ij - sum_{k < j} fl(fl(L^_jk D^_k) L^_ik)) fl(1 / D^_j)), D^_j likewise without the pivot step.  At
most c additions in any order (c - 1 update terms onto K_ij, so every term carries at most c - 1 of them: atomics and
trees are covered), two multiplications per term, one reciprocal and one multiplication for the pivot: no term of T
carries more than (c - 1) + 2 roundings, the K entry no more than c - 1, the k = j term (L^_ij D^_j) two.  (c + 2) u T
covers all of them.  A kernel that rounds more often per term has to state its count beside the constant it uses.  Counted
from the code: bundle_factor.hip, bundle_gstep.hip and the column kernels multiply L^_jk D^_k once, then by L^_ik (two);
the matrix-core tiles of snode.hip stage fl(D^_k L^_jk) and accumulate fma by fma from zero before one subtraction (two,
and the same number of additions); k_snode_rows scales x_q first and multiplies by the staged d_q L_jq (two); the panel
kernels k_snode_panel and k_snode_panel2 carry the unscaled u_ik = L_ik D_k, from which L^_ik = fl(u_ik fl(1 / D^_k)),
through a column: a term is fl(L^_jk u_ik), three roundings away from L^_ik D^_k L^_jk -- (c - 1) + 3 = c + 2, still the
constant as it stands.

R is accumulated in np.longdouble (63 mantissa bits asserted): at most (c + 2) 2^-64 T, below 2^-10 of the bound.  For
ONE dense front (order 2300) the longdouble product is too slow: dense=True evaluates R in float64 BLAS, whose own error
is within the same (c + 2) u T, and DOUBLES the bound.  A residual that is not finite -- a NaN or Inf left in the factor
or in a solution -- has ratio inf in every check of this module.

solve_check: for an unrefined solve x^ of L^ D^ L^' x = b (permuted numbering, full length N)

    r = |b - L^ (D^ (L^' x^))|,   t = |L^| (|D^| (|L^'| |x^|)),   ratio_i = r_i / ((rmax + cmax + 4) u t_i)

rmax, cmax the longest row and column of L^, diagonal included: gamma_rmax for the forward sweep (row i of L^ is what the
sum of y_i runs over), gamma_cmax for the backward sweep, gamma_2 for the pivots (reciprocal, multiplication), first
order; two more for the slack of the first-order argument.

solve_check_visible: for KKT handles with sparse second-order cones (N > n + m), whose fused kernels return only the
first n + m components.  With M = L^ D^ L^', H the hidden indices: solve M_HH x~_H = b_H - M_HV x^_V in longdouble (the
float64 inverse of the small dense M_HH, refined with longdouble residuals until the hidden rows are met to 2^-10 of
their bound), then
|b_V - M_VV x^_V - M_VH x~_H| <= 1.01 (bound_V + |M_VH| |M_HH^-1| bound_H), t evaluated at [x^_V; x~_H]: the device's
own hidden components satisfy their rows within bound_H, so they differ from x~_H by at most |M_HH^-1| bound_H (1.01:
the second-order terms, t being taken at x~_H instead of the device's x^_H).
"""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa here: the residuals would round like the factor"


def relerr(a, b):
    """the max-norm check of the suite (tests/test_gpu_parity.py), for showing what it does not see"""
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def lower_permuted(N, colptr, rowval, nzval, perm):
    """the upper-triangle CSC (colptr, rowval, nzval) of a symmetric K -> the lower triangle of K[perm][:, perm] as a
    float64 scipy CSC with sorted indices (new index i is old index perm[i]); explicit zeros are kept"""
    colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    iperm = np.empty(N, dtype=np.int64)
    iperm[perm] = np.arange(N)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    a, b = iperm[rowval[:colptr[N]]], iperm[cols]
    i, j = np.maximum(a, b), np.minimum(a, b)
    order = np.lexsort((i, j))
    i, j, v = i[order], j[order], np.asarray(nzval, dtype=np.float64)[:colptr[N]][order]
    assert not np.any((i[1:] == i[:-1]) & (j[1:] == j[:-1])), "duplicate entries"
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(j, minlength=N), out=ptr[1:])
    return sp.csc_matrix((v, i, ptr), shape=(N, N))


def kkt_lower(ks, values=None):
    """the K a HipKKTSolver handle factors, lower triangle, permuted numbering: the value store with the static
    regulariser of the last refactor put on in float64 as the device applies it, fl(K_jj + dsigns_j * last_regularizer)
    on diag_full"""
    K = ks.kkt_matrix()
    v = np.array(ks.values() if values is None else values, dtype=np.float64)
    mp = ks.maps()
    eps = float(ks.linear_solver_info().last_regularizer)
    v[mp["diag_full"]] = v[mp["diag_full"]] + mp["dsigns"].astype(np.float64) * eps
    return lower_permuted(ks.N, K.colptr, K.rowval, v, ks.perm)


def _keys(N, ptr, idx):
    return np.repeat(np.arange(N, dtype=np.int64), np.diff(ptr)) * N + idx


def _at(M, N, keys):
    """the values of the sparse M at the positions keys = column * N + row (0 where M stores nothing)"""
    M = sp.csc_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    out = np.zeros(len(keys), dtype=M.dtype)
    mk = _keys(N, M.indptr.astype(np.int64), M.indices.astype(np.int64))
    if len(mk):
        pos = np.minimum(np.searchsorted(mk, keys), len(mk) - 1)
        hit = mk[pos] == keys
        out[hit] = M.data[pos[hit]]
    return out


def unit_lower(N, Lp, Li, Lx, dtype=np.float64):
    """L^ with its unit diagonal as a scipy CSC"""
    Lp, Li = np.asarray(Lp, dtype=np.int64), np.asarray(Li, dtype=np.int64)
    L = sp.csc_matrix((np.asarray(Lx, dtype=dtype), Li, Lp), shape=(N, N))
    return (L + sp.identity(N, dtype=dtype, format="csc")).tocsc()


def _ratio(err, bound):
    """error over bound per entry; 0 where the error is exactly 0, inf where either is not finite: a NaN or Inf in a factor
    or a solution is an error of any size, never a pass"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ratio = np.where(err > 0.0, err / np.where(bound > 0.0, bound, np.finfo(np.float64).tiny), 0.0)
    return np.where(np.isfinite(err) & np.isfinite(bound), ratio, np.inf)


DENSE_TERMS_MAX = 4096  # up to this order T and c come from dense BLAS products (exact counts in float32 up to 2^24)


def factor_check(N, Lp, Li, Lx, D, Klow, dense=False):
    """-> dict(ratio per stored position (the N diagonal positions, then the entries of Li in their order), rows, cols,
    worst, at=(i, j), R, T, c); see the module docstring.  A position whose residual is not finite has ratio inf.
    (T, which only scales the bound, and the counts c are taken from dense float64 / float32 BLAS products up to order
    DENSE_TERMS_MAX -- T is then off by at most N u relative --, from sparse products above; R is longdouble either way
    unless dense=True.)"""
    Lp, Li = np.asarray(Lp, dtype=np.int64), np.asarray(Li, dtype=np.int64)
    Lx, D = np.asarray(Lx, dtype=np.float64), np.asarray(D, dtype=np.float64)
    assert len(Lx) == len(Li) == Lp[N] and len(D) == N
    cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(Lp))
    assert np.all(Li > cols), "the pattern is not strictly lower triangular"
    rows = np.concatenate([np.arange(N, dtype=np.int64), Li])
    cols = np.concatenate([np.arange(N, dtype=np.int64), cols])
    keys = cols * N + rows
    Kij = _at(Klow, N, keys)
    assert np.count_nonzero(Kij) == np.count_nonzero(Klow.data), "K has entries outside the pattern of the factor"
    with np.errstate(invalid="ignore", over="ignore"):
        if dense or N <= DENSE_TERMS_MAX:
            La = np.abs(unit_lower(N, Lp, Li, Lx).toarray())
            T = ((La * np.abs(D)) @ La.T)[rows, cols]
            B = np.zeros((N, N), dtype=np.float32)
            B[rows, cols] = 1.0
            c = (B @ B.T)[rows, cols].astype(np.float64)
        else:
            La = abs(unit_lower(N, Lp, Li, Lx))
            T = _at((La @ sp.diags(np.abs(D), format="csc")) @ La.T.tocsc(), N, keys)
            B = unit_lower(N, Lp, Li, np.ones(len(Li)))
            c = _at(B @ B.T.tocsc(), N, keys)
        if dense:  # float64 BLAS, the bound doubled (module docstring)
            L = unit_lower(N, Lp, Li, Lx).toarray()
            R = np.abs(Kij - ((L * D) @ L.T)[rows, cols])
        else:
            L = unit_lower(N, Lp, Li, Lx, LD)
            S = _at((L @ sp.diags(D.astype(LD), format="csc")) @ L.T.tocsc(), N, keys)
            R = np.abs(Kij.astype(LD) - S).astype(np.float64)
    T = np.abs(Kij) + T
    ratio = _ratio(R, (2.0 if dense else 1.0) * (c + 2.0) * U * T)
    w = int(np.argmax(ratio))
    return dict(ratio=ratio, rows=rows, cols=cols, worst=float(ratio[w]), at=(int(rows[w]), int(cols[w])), R=R, T=T, c=c)


class Substitution:
    """L^ D^ L^' of one factor for any number of vectors: the residual in longdouble, t and the bound per row"""

    def __init__(self, N, Lp, Li, Lx, D):
        Lp, Li = np.asarray(Lp, dtype=np.int64), np.asarray(Li, dtype=np.int64)
        self.N = N
        self.L = unit_lower(N, Lp, Li, Lx, LD)
        self.Lt = self.L.T.tocsr()
        self.D = np.asarray(D, dtype=LD)
        self.La = abs(unit_lower(N, Lp, Li, Lx))
        self.Lat = self.La.T.tocsr()
        self.Da = np.abs(np.asarray(D, dtype=np.float64))
        # the longest row and column of L^, diagonal included
        self.cmax = int(np.max(np.diff(Lp), initial=0)) + 1
        self.rmax = int(np.max(np.bincount(Li, minlength=N), initial=0)) + 1

    def product(self, x):
        """L^ (D^ (L^' x)) in longdouble"""
        return self.L @ (self.D * (self.Lt @ np.asarray(x, dtype=LD)))

    def bound(self, x):
        """(rmax + cmax + 4) u t per row, t = |L^| (|D^| (|L^'| |x|))"""
        with np.errstate(invalid="ignore", over="ignore"):
            t = self.La @ (self.Da * (self.Lat @ np.abs(np.asarray(x, dtype=np.float64))))
        return (self.rmax + self.cmax + 4) * U * np.asarray(t, dtype=np.float64)

    def check(self, b, x):
        with np.errstate(invalid="ignore", over="ignore"):
            r = np.abs(np.asarray(b, dtype=LD) - self.product(x)).astype(np.float64)
        bound = self.bound(x)
        ratio = _ratio(r, bound)
        w = int(np.argmax(ratio))
        return dict(ratio=ratio, worst=float(ratio[w]), at=w, r=r, bound=bound, rmax=self.rmax, cmax=self.cmax)


def solve_check(N, Lp, Li, Lx, D, b, x):
    """-> dict(ratio per row, worst, at, r, bound); b, x in the permuted numbering, full length N.  A row whose residual is
    not finite (a NaN or Inf component of x^) has ratio inf."""
    return Substitution(N, Lp, Li, Lx, D).check(b, x)


class VisibleSolveCheck:
    """solve_check_visible for several right-hand sides through one factor: M = L^ D^ L^' and |M_HH^-1| are formed once.
    `hidden` in the permuted numbering"""

    def __init__(self, N, Lp, Li, Lx, D, hidden):
        self.N = N
        self.sub = Substitution(N, Lp, Li, Lx, D)
        self.H = np.sort(np.asarray(hidden, dtype=np.int64))
        self.V = np.setdiff1d(np.arange(N, dtype=np.int64), self.H)
        self.M = ((self.sub.L @ sp.diags(self.sub.D, format="csc")) @ self.sub.L.T.tocsc()).tocsr()
        MH = self.M[self.H]
        self.MHV, self.MHH = MH[:, self.V].tocsr(), MH[:, self.H].toarray()
        self.MVH = abs(self.M[self.V][:, self.H]).astype(np.float64).tocsr()
        # (float64: |M_HH^-1| only scales a bound; the hidden components themselves are refined in longdouble below)
        self.MHHinv = np.linalg.inv(self.MHH.astype(np.float64))

    def check(self, b, xV):
        """-> dict(ratio per visible row, worst, at (permuted index), xH); b of full length N in the permuted numbering,
        xV the components at the visible indices (ascending permuted index).  Not finite xV: ratio inf."""
        N, H, V = self.N, self.H, self.V
        assert len(xV) == len(V) and len(b) == N
        if not np.all(np.isfinite(np.asarray(xV, dtype=np.float64))):
            bad = ~np.isfinite(np.asarray(xV, dtype=np.float64))
            return dict(ratio=np.where(bad, np.inf, 0.0), worst=np.inf, at=int(V[np.argmax(bad)]), xH=None, r=None, bound=None)
        b, xV = np.asarray(b, dtype=LD), np.asarray(xV, dtype=LD)
        rhs = b[H] - self.MHV @ xV
        xH = np.zeros(len(H), dtype=LD)
        for _ in range(8):  # M_HH x~_H = rhs by refinement of the float64 inverse, residuals in longdouble
            res = rhs - self.MHH @ xH
            xH = xH + self.MHHinv.astype(LD) @ res
        x = np.zeros(N, dtype=LD)
        x[V], x[H] = xV, xH
        r = np.abs(b - self.M @ x).astype(np.float64)
        bound = self.sub.bound(x.astype(np.float64))
        assert np.all(r[H] <= 2.0 ** -10 * bound[H]), "the hidden components did not converge"
        ratio = _ratio(r[V], 1.01 * (bound[V] + self.MVH @ (np.abs(self.MHHinv) @ bound[H])))
        w = int(np.argmax(ratio))
        return dict(ratio=ratio, worst=float(ratio[w]), at=int(V[w]), xH=xH.astype(np.float64), r=r[V])


def solve_check_visible(N, Lp, Li, Lx, D, b, xV, hidden):
    """one right-hand side through VisibleSolveCheck; see the module docstring"""
    return VisibleSolveCheck(N, Lp, Li, Lx, D, hidden).check(b, xV)


# ---- a plain float64 LDL' and substitution, the sums taken in a shuffled order ------------------------------------
def plain_ldl(Klow, Lp, Li, rng, skip=None, twice=None):
    """left-looking float64 LDL' on the pattern (Lp, Li), reciprocal-multiply pivots, the update terms of a column in
    a shuffled order -> (Lx, D).  skip / twice = (i, j, k): the term L_ik D_k L_jk of entry (i, j) left out / applied
    twice (the wrong factors of tests/test_ldl_ref_host.py)"""
    N = Klow.shape[0]
    A = Klow.toarray()
    L = np.zeros((N, N))
    D = np.zeros(N)
    rows_of = [Li[Lp[j]:Lp[j + 1]] for j in range(N)]
    cols_in_row = [[] for _ in range(N)]
    for j in range(N):
        col = A[:, j].copy()
        ks = np.array(cols_in_row[j], dtype=np.int64)
        rng.shuffle(ks)
        for k in ks:
            upd = L[:, k] * (L[j, k] * D[k])
            for wrong, f in ((skip, 0.0), (twice, 2.0)):
                if wrong is not None and wrong[1:] == (j, int(k)):
                    upd[wrong[0]] *= f
            col[j:] -= upd[j:]
        D[j] = col[j]
        dinv = 1.0 / D[j]
        L[rows_of[j], j] = col[rows_of[j]] * dinv
        for i in rows_of[j]:
            cols_in_row[i].append(j)
    cols = np.repeat(np.arange(N), np.diff(Lp))
    return L[Li, cols], D


def plain_solve(N, Lp, Li, Lx, D, b, rng, skip_fwd=None, skip_bwd=None):
    """float64 substitution through L^ D^ L^', every row's sum in a shuffled order, the pivots by reciprocal and
    multiplication -> x.  skip_fwd / skip_bwd = position p of Lx whose contribution the forward / backward sweep drops"""
    L = sp.csc_matrix((Lx, Li, Lp), shape=(N, N))
    Lr = L.tocsr()
    Lr.sort_indices()
    cols = np.repeat(np.arange(N), np.diff(Lp))
    y = np.array(b, dtype=np.float64)
    for i in range(N):
        a, e = Lr.indptr[i], Lr.indptr[i + 1]
        order = rng.permutation(e - a) + a
        for p in order:
            k = Lr.indices[p]
            if skip_fwd is not None and (Li[skip_fwd], cols[skip_fwd]) == (i, k):
                continue
            y[i] -= Lr.data[p] * y[k]
    y = y * (1.0 / D)
    for j in range(N - 1, -1, -1):
        order = rng.permutation(Lp[j + 1] - Lp[j]) + Lp[j]
        for p in order:
            if skip_bwd is not None and p == skip_bwd:
                continue
            y[j] -= Lx[p] * y[Li[p]]
    return y
