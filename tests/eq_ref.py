"""References, bounds and inputs for the passes of clarabel.rs_amd/csrc/equilibrate.hip: no GPU, no package.

Restated per step, with numpy element operations in the kernels' and the reference's order and every sum by math.fsum:
    ruiz_step()   problemdata.rs:246-297: the inf-norms of [P A; A' 0] (a stored entry of the upper triangle of P counts
                  for its column and its row), zeros -> 1, 1 / sqrt, clip(w, smin / cum, smax / cum), val * (l[row] * r[col]),
                  q d, b e, the cumulative d and e, the mean of the column norms of the scaled (triu) P, ||q||inf, the
                  cost factor clip(1 / max(||q||inf, mean), smin / c, smax / c) and P, q, c times it
    rectify()     compositecone.rs:183-195 with socone.rs:97-101: delta = (1.0 / e) * mean(e) over each cone that takes a
                  scalar scaling, 1 elsewhere; A <- diag(delta) A, b <- delta b, e <- delta e
    unscale()     variables.rs:262-285: (x * d) * sx, (z * e) * sz, (s * einv) * ss with sx = ss = 1 / tau, sz = sx * (1 / c)
    wsumsq()      the sums of (v w)^2 behind the scaled norms of info.rs:142-165

What is bit for bit, and what has a bound.  A maximum is exact in any order, and every other operation above except the
three sums (the column-norm mean, a cone's mean, a sum of squares) is one correctly rounded IEEE operation per entry in
a fixed order, so the device must return the reference's bits for: the norms, the factors, d, e, A, b, P and q before the
cost factor, 1 / d and 1 / e, unscale.  A quantity behind a sum of L non-negative terms is held to
    (L + 4) 2^-53 |reference|,
u = 2^-53: L terms added in any tree lose at most (L - 1) u of their sum to first order (all terms have one sign, so the
sum of the magnitudes is the sum); the division by the count, the reciprocal or the product with 1 / e, and the product
with the value it scales are one rounding each, and the reference's own correctly rounded fsum is the last u.  That is c
and the cost-scaled P and q with L = n, the rows of a rectified cone with L its length, and a weighted sum of squares with
L = n: its terms (v w)^2 are taken by the device and by the reference with the same two products, so their roundings
cancel, and a device that fused the square into the addition would only remove one rounding per term, which is u of the
sum once squared out and is covered by the + 4.  Second-order terms (L u)^2 at L = 262145 are 1e-21 of the sum.

The cost factor is free of any sum in four situations, which ruiz_step reports as `kind`: "skipped" (mean or ||q||inf
is 0: the factor is exactly 1 and c, P, q keep their bytes), "q" (||q||inf exceeds the mean by more than twice that
bound: the factor is 1 / ||q||inf), "clip_lo" / "clip_hi" (the unclipped value is outside the bounds by more than twice
the bound).  Such steps are held bit for bit; "mean" steps to the bound.

Two data families.  Exact: every entry of P, A, q, b is a signed power of 4 (its root is a power of 2), d, e, c, the vectors
of the norms and min_scaling / max_scaling are powers of 2, with exponents so narrow that every sum is exact in any order;
assert_exact() checks that of each summed list by comparing math.fsum with a sequential and a pairwise sum.  Then mean,
factor and everything after them are the same correctly rounded operations on the same exact sum: ONE step, the
rectification and the sums of squares come back bit for bit.  Wide: standard_normal * 10^uniform(-6, 6)."""
import math

import numpy as np

U = 2.0 ** -53
WG, WAVE = 256, 64
EXACT_SCALING = (2.0 ** -13, 2.0 ** 13)
WIDE_SCALING = (1e-4, 1e4)
SUM_FREE = ("skipped", "q", "clip_lo", "clip_hi")


# ---- sums ------------------------------------------------------------------------------------------------------------
def seq_sum(a):
    t = 0.0
    for v in a:
        t += v
    return t


def pairwise_sum(a):
    a = list(a)
    if not a:
        return 0.0
    while len(a) > 1:
        a = [a[i] + a[i + 1] if i + 1 < len(a) else a[i] for i in range(0, len(a), 2)]
    return a[0]


SUMMERS = {"fsum": math.fsum, "sequential": seq_sum, "pairwise": pairwise_sum}


def assert_exact(terms, what=""):
    """the sum of `terms` is exact in any order (taken here: fsum against a sequential and a pairwise sum)"""
    t = np.asarray(terms, dtype=float).tolist()
    want = math.fsum(t)
    assert seq_sum(t) == want and pairwise_sum(t) == want and seq_sum(t[::-1]) == want, "sum not exact: " + what
    return want


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=float), np.ascontiguousarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def rel_bound(L):
    return (np.asarray(L, dtype=float) + 4.0) * U


def ratio(have, want, L):
    """largest |have - want| / ((L + 4) u |want|) and where; an error where the reference is 0, or a NaN, is infinite"""
    have, want = np.atleast_1d(np.asarray(have, dtype=float)), np.atleast_1d(np.asarray(want, dtype=float))
    if not have.size:
        return 0.0, 0
    err, bound = np.abs(have - want), rel_bound(L) * np.abs(want)
    r = np.where(have.view(np.int64) == want.view(np.int64), 0.0,
                 np.where((bound > 0.0) & np.isfinite(err), err / np.where(bound > 0.0, bound, 1.0), np.inf))
    k = int(np.argmax(r))
    return float(r[k]), k


def clip(x, lo, hi):
    """x < lo ? lo : (x > hi ? hi : x), the order of T::clip and of the kernels"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def cols_of(colptr):
    return np.repeat(np.arange(len(colptr) - 1, dtype=np.int64), np.diff(np.asarray(colptr, dtype=np.int64)))


def _amax(count, index, values):
    out = np.zeros(count)
    if len(values):
        np.maximum.at(out, index, np.abs(values))
    return out


# ---- one Ruiz step -----------------------------------------------------------------------------------------------------
def ruiz_step(st, smin, smax, summer=math.fsum):
    """st: dict(n, m, P=(colptr, rowval, nzval), A=(...), q, b, d, e, c) -> the state after ONE step (same keys) plus
    report keys: dw, ew (this step's factors), before = (Px, q) ahead of the cost factor, pcol (the summed column norms),
    mean, qn, factor, kind (module docstring)"""
    n, m = st["n"], st["m"]
    Pp, Pi, Px = (np.asarray(a) for a in st["P"])
    Ap, Ai, Ax = (np.asarray(a) for a in st["A"])
    Pi, Ai = Pi.astype(np.int64), Ai.astype(np.int64)
    Pc, Ac = cols_of(Pp), cols_of(Ap)
    q, b, d, e = (np.asarray(st[k], dtype=float) for k in ("q", "b", "d", "e"))
    c = float(st["c"])
    dn = np.maximum(np.maximum(_amax(n, Pc, Px), _amax(n, Pi, Px)), _amax(n, Ac, Ax))
    en = _amax(m, Ai, Ax)
    dn[dn == 0.0] = 1.0
    en[en == 0.0] = 1.0
    dw = clip(1.0 / np.sqrt(dn), smin / d, smax / d)
    ew = clip(1.0 / np.sqrt(en), smin / e, smax / e)
    Px1 = Px * (dw[Pi] * dw[Pc])
    Ax1 = Ax * (ew[Ai] * dw[Ac])
    q1, b1, d1, e1 = q * dw, b * ew, d * dw, e * ew
    pcol = _amax(n, Pc, Px1)
    mean = summer(pcol.tolist()) / n if n else 0.0
    qn = float(np.max(np.abs(q1))) if n else 0.0
    factor, kind = 1.0, "skipped"
    Px2, q2, c2 = Px1, q1, c
    if mean != 0.0 and qn != 0.0:
        lo, hi = smin / c, smax / c
        t = 1.0 / max(qn, mean)
        factor = float(clip(np.float64(t), lo, hi))
        slack = 2.0 * float(rel_bound(n))
        if t * (1.0 + slack) < lo:
            kind = "clip_lo"
        elif t * (1.0 - slack) > hi:
            kind = "clip_hi"
        elif qn > mean * (1.0 + slack):
            kind = "q"
        else:
            kind = "mean"
        Px2, q2, c2 = Px1 * factor, q1 * factor, c * factor
    out = dict(st, P=(st["P"][0], st["P"][1], Px2), A=(st["A"][0], st["A"][1], Ax1), q=q2, b=b1, d=d1, e=e1, c=c2)
    out.update(dw=dw, ew=ew, before=(Px1, q1), pcol=pcol, mean=mean, qn=qn, factor=factor, kind=kind)
    return out


def compare_step(ref, got, c_in, exact):
    """got: what the runner returned (Px, Ax, q, b, d, e, c, factor); ref: ruiz_step of the same state, whose c was
    c_in.  -> (ratios, failures).  Bit for bit always: Ax, b, d, e, and P, q, c as the reference's values before the
    cost factor times the factor the DEVICE reports (its own products).  The factor, c and the cost-scaled P and q:
    bit for bit in the exact family and when no sum decides, else (n + 4) u."""
    fails, ratios = [], {}
    n = ref["n"]

    def bits(name, have, want):
        if not same_bits(have, want):
            have, want = np.atleast_1d(np.asarray(have, float)), np.atleast_1d(np.asarray(want, float))
            k = int(np.flatnonzero(have.view(np.int64) != want.view(np.int64))[0]) if have.shape == want.shape else -1
            fails.append("%s[%d] of %d: %r, reference %r (bit for bit)" % (name, k, len(want), have[k], want[k]))

    bits("Ax", got["Ax"], ref["A"][2])
    for k in ("b", "d", "e"):
        bits(k, got[k], ref[k])
    f = got["factor"]
    if ref["kind"] == "skipped":
        bits("factor (skipped)", [f], [1.0])
    if f == 1.0:  # k_eq_cost_apply returns at once: the bytes of before the cost factor, -0.0 included
        bits("Px (factor 1)", got["Px"], ref["before"][0])
        bits("q (factor 1)", got["q"], ref["before"][1])
        bits("c (factor 1)", [got["c"]], [c_in])
    else:
        bits("Px = before * device factor", got["Px"], ref["before"][0] * f)
        bits("q = before * device factor", got["q"], ref["before"][1] * f)
        bits("c = c * device factor", [got["c"]], [c_in * f])
    sum_free = exact or ref["kind"] in SUM_FREE
    for name, have, want in (("factor", [f], [ref["factor"]]), ("c", [got["c"]], [ref["c"]]),
                             ("Px", got["Px"], ref["P"][2]), ("q", got["q"], ref["q"])):
        ratios[name], k = ratio(have, want, n)
        if sum_free:
            bits(name, have, want)
        elif ratios[name] > 1.0:
            fails.append("%s[%d]: %r, reference %r, error / bound %.3g (L = %d)"
                         % (name, k, np.atleast_1d(have)[k], np.atleast_1d(want)[k], ratios[name], n))
    return ratios, fails


# ---- the rectification, the inverses, unscale, the sums of squares ----------------------------------------------------
def rectify(m, A, b, e, segments, summer=math.fsum):
    """-> (Ax, b, e, delta, L): L[i] = the length of the rectified cone row i belongs to, 0 outside every cone"""
    Ap, Ai, Ax = (np.asarray(a) for a in A)
    Ai = Ai.astype(np.int64)
    b, e = np.asarray(b, dtype=float), np.asarray(e, dtype=float)
    delta, L = np.ones(m), np.zeros(m, dtype=np.int64)
    for beg, end in segments:
        seg = e[beg:end]
        mean = summer(seg.tolist()) / (end - beg)
        delta[beg:end] = (1.0 / seg) * mean
        L[beg:end] = end - beg
    return Ax * delta[Ai], b * delta, e * delta, delta, L


def compare_rectified(ref, got, Ai, exact):
    """ref = rectify(...), got = (Ax, b, e) -> (largest error / bound, failures): rows outside the cones (L = 0) and the
    exact family bit for bit, rows of a cone of L rows within (L + 4) u"""
    L = ref[4]
    worst, fails = 0.0, []
    for name, have, want, Lk in (("Ax", got[0], ref[0], L[np.asarray(Ai, dtype=np.int64)]), ("b", got[1], ref[1], L),
                                 ("e", got[2], ref[2], L)):
        have, want = np.asarray(have, float), np.asarray(want, float)
        free = np.ones(len(want), dtype=bool) if exact else Lk == 0
        if not same_bits(have[free], want[free]):
            k = int(np.flatnonzero(free & (have.view(np.int64) != want.view(np.int64)))[0])
            fails.append("%s[%d] (cone of %d): %r, reference %r (bit for bit)" % (name, k, Lk[k], have[k], want[k]))
        r, k = ratio(have, want, Lk)
        worst = max(worst, r)
        if r > 1.0:
            fails.append("%s[%d] (cone of %d): %r, reference %r, error / bound %.3g" % (name, k, Lk[k], have[k], want[k], r))
    return worst, fails


def invert(d, e):
    return 1.0 / np.asarray(d, dtype=float), 1.0 / np.asarray(e, dtype=float)


def unscale(x, d, sx, z, e, sz, s, einv, ss):
    """the kernel's operands: ((x d) sx, (z e) sz, (s einv) ss)"""
    return (np.asarray(x) * d) * sx, (np.asarray(z) * e) * sz, (np.asarray(s) * einv) * ss


def unscale_solution(x, z, s, d, e, einv, c, tau):
    """variables.rs:262-285 for a status that is not an infeasibility: scaleinv = 1 / tau, z also by 1 / c"""
    scaleinv, cinv = 1.0 / tau, 1.0 / c
    return unscale(x, d, scaleinv, z, e, scaleinv * cinv, s, einv, scaleinv)


def wsumsq(v, w, summer=math.fsum):
    """-> (the sum of (v w)^2, its bound (n + 4) u times it)"""
    t = np.asarray(v, dtype=float) * np.asarray(w, dtype=float)
    sq = summer((t * t).tolist())
    return sq, float(rel_bound(len(t))) * sq


# ---- K steps and the rectification: what a handle's setup leaves --------------------------------------------------------
def cone_numel(c):
    return 3 if c[0] in (3, 4) else c[1] + c[2] if c[0] == 5 else c[1] * (c[1] + 1) // 2 if c[0] == 6 else c[1]


def rect_segments(cones):
    """the row ranges of the cones that take a scalar scaling (SecondOrder and everything after it)"""
    out, start = [], 0
    for c in cones:
        k = cone_numel(c)
        if c[0] >= 2 and k > 0:
            out.append((start, start + k))
        start += k
    return out


def equilibrate(pr, max_iter, smin=WIDE_SCALING[0], smax=WIDE_SCALING[1], summer=math.fsum):
    """pr: dict(n, m, P, A, q, b, cones) -> (d, e, c, Px, Ax, q, b, kinds of the steps, L per row): DefaultProblemData::
    equilibrate from d = e = 1, c = 1 with b capped at 1e20"""
    st = dict(n=pr["n"], m=pr["m"], P=tuple(np.asarray(a) for a in pr["P"]), A=tuple(np.asarray(a) for a in pr["A"]),
              q=np.asarray(pr["q"], dtype=float), b=np.minimum(np.asarray(pr["b"], dtype=float), 1e20),
              d=np.ones(pr["n"]), e=np.ones(pr["m"]), c=1.0)
    kinds = []
    for _ in range(max_iter):
        st = ruiz_step(st, smin, smax, summer)
        kinds.append(st["kind"])
    segs = rect_segments(pr["cones"])
    Ax, b, e, L = st["A"][2], st["b"], st["e"], np.zeros(pr["m"], dtype=np.int64)
    if segs:
        Ax, b, e, _, L = rectify(pr["m"], st["A"], st["b"], st["e"], segs, summer)
    return dict(d=st["d"], e=e, c=st["c"], Px=st["P"][2], Ax=Ax, q=st["q"], b=b, kinds=kinds, L=L)


# ---- patterns ----------------------------------------------------------------------------------------------------------
def _csc(m, n, rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((rows, cols))
    colptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=colptr[1:])
    return colptr, rows[order]


def _empty(n):
    return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)


def diag_pattern(n, m):
    """P the n x n diagonal, A m x n with one entry per row, row i in column i mod n"""
    P = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64))
    A = _csc(m, n, np.arange(m), np.arange(m) % n) if m else _empty(n)
    return dict(n=n, m=m, P=P, A=A)


def random_pattern(n, m, nnzP, nnzA, seed):
    """nnzP distinct entries of the upper triangle (two fifths of them on the diagonal), nnzA distinct entries of A"""
    rng = np.random.default_rng(seed)
    pk = np.zeros(0, dtype=np.int64)
    if nnzP:
        ndiag = min(n, max(1, (2 * nnzP) // 5))
        diag = rng.permutation(n)[:ndiag].astype(np.int64) * (n + 1)
        r_, c_ = np.triu_indices(n, 1)
        pk = np.concatenate([diag, rng.permutation(r_ * n + c_)[:nnzP - ndiag]])
        assert len(pk) == nnzP
    ak = rng.choice(m * n, nnzA, replace=False) if nnzA else np.zeros(0, dtype=np.int64)
    return dict(n=n, m=m, P=_csc(n, n, pk // n, pk % n) if nnzP else _empty(n),
                A=_csc(m, n, ak // n, ak % n) if nnzA else _empty(n))


# ---- values ------------------------------------------------------------------------------------------------------------
def _pow(rng, k, base_exp, lo, hi, signed=True):
    v = np.ldexp(1.0, base_exp * rng.integers(lo, hi + 1, k))
    return v * rng.choice([-1.0, 1.0], k) if signed else v


def wide(rng, k):
    return rng.standard_normal(k) * 10.0 ** rng.uniform(-6.0, 6.0, k)


def state(pat, family, seed):
    """a Ruiz state on a pattern.  exact: P, A, q, b signed powers of 4 in 4^-3 .. 4^3, d, e in 2^-2 .. 2^2, c = 2;
    wide: P, A, q, b wide(), d, e = 10^uniform(-2, 2), c = 10^uniform(-1, 1)"""
    rng = np.random.default_rng(seed)
    n, m, nP, nA = pat["n"], pat["m"], len(pat["P"][1]), len(pat["A"][1])
    if family == "exact":
        vals = [_pow(rng, k, 2, -3, 3) for k in (nP, nA, n, m)]
        d, e, c = _pow(rng, n, 1, -2, 2, False), _pow(rng, m, 1, -2, 2, False), 2.0
    else:
        vals = [wide(rng, k) for k in (nP, nA, n, m)]
        d, e, c = 10.0 ** rng.uniform(-2, 2, n), 10.0 ** rng.uniform(-2, 2, m), float(10.0 ** rng.uniform(-1, 1))
    return dict(n=n, m=m, P=(pat["P"][0], pat["P"][1], vals[0]), A=(pat["A"][0], pat["A"][1], vals[1]), q=vals[2],
                b=vals[3], d=d, e=e, c=c)


def scaling(family):
    return EXACT_SCALING if family == "exact" else WIDE_SCALING


def check_state_sums(st, smin, smax):
    """exact family: the one sum of a step, the column norms of the scaled P, is exact in any order"""
    ref = ruiz_step(st, smin, smax)
    assert_exact(ref["pcol"], "column norms of the scaled P")
    return ref


# ---- the cases of one Ruiz step (tests/test_equilibrate_passes_gpu.py runs them on the device,
# tests/test_eq_ref_host.py checks their sums and their premises on the CPU) -------------------------------------------
def _sorted_magnitudes(v, descending):
    mag = np.sort(np.abs(v))
    return (mag[::-1] if descending else mag) * np.sign(v)


def case_split_in_wavefront(family):
    """nnzP = 100: entries 64 .. 99 of the second wavefront are P's, 100 .. 127 A's; n = 100: the d | e split of
    k_eq_factors at lane 36 of the second wavefront"""
    return state(random_pattern(100, 150, 100, 700, 1), family, 101)


def case_lp(family):
    """no stored P: mean 0, the cost scaling skipped"""
    return state(random_pattern(100, 150, 0, 700, 2), family, 102)


def case_unconstrained(family):
    """m = 0, nnzA = 0"""
    return state(random_pattern(100, 0, 300, 0, 3), family, 103)


def case_offdiagonal(family):
    """P = [[p00, big], [., p11]] plus a third column: the off-diagonal entry (0, 1) is larger than both diagonals, so
    it is the norm of column 1 AND of row 0 for d, and for the cost mean the norm of column 1 alone"""
    pat = dict(n=3, m=2, P=_csc(3, 3, [0, 0, 1, 2], [0, 1, 1, 2]), A=_csc(2, 3, [0, 1], [0, 2]))
    st = state(pat, family, 104)
    big = 4.0 ** 3 if family == "exact" else 3.7e5
    small = 4.0 ** -2 if family == "exact" else 2.3e-3
    st["P"] = (pat["P"][0], pat["P"][1], np.array([small, -big, small, 1.0]))  # (0,0), (0,1), (1,1), (2,2)
    st["A"] = (pat["A"][0], pat["A"][1], np.array([small, small]))
    st["d"], st["e"] = np.ones(3), np.ones(2)
    st["q"] = st["q"] * _small(family)  # the mean decides the cost factor
    return st


def case_zero_row_and_column(family):
    """row 5 and column 7 hold only a stored 0.0 and a stored -0.0; row 9 and column 11 hold nothing: norm 0, factor 1"""
    pat = random_pattern(40, 50, 90, 400, 5)
    st = state(pat, family, 105)
    Pp, Pi, Px = st["P"]
    Ap, Ai, Ax = st["A"]
    Pc, Ac = cols_of(Pp), cols_of(Ap)
    keepP = ~np.isin(Pi, (11,)) & ~np.isin(Pc, (11,))
    keepA = (Ai != 9) & (Ac != 11)
    st["P"] = _csc(40, 40, Pi[keepP], Pc[keepP]) + (Px[keepP],)  # (Px is in CSC order already)
    st["A"] = _csc(50, 40, Ai[keepA], Ac[keepA]) + (Ax[keepA],)
    Pp, Pi, Px = st["P"]
    Ap, Ai, Ax = st["A"]
    Pc, Ac = cols_of(Pp), cols_of(Ap)
    zp = np.flatnonzero((Pi == 7) | (Pc == 7))
    za = np.flatnonzero((Ai == 5) | (Ac == 7))
    Px, Ax = Px.copy(), Ax.copy()
    Px[zp] = np.where(np.arange(len(zp)) % 2 == 0, 0.0, -0.0)
    Ax[za] = np.where(np.arange(len(za)) % 2 == 0, -0.0, 0.0)
    st["P"], st["A"] = (Pp, Pi, Px), (Ap, Ai, Ax)
    return st


def _dense_line(family, row, descending):
    n_long = 20000
    if row:  # row 1 of 3 holds all of 20000 columns
        pat = dict(n=n_long, m=3, P=diag_pattern(n_long, 0)["P"],
                   A=_csc(3, n_long, np.concatenate([np.ones(n_long, dtype=np.int64), [0, 2]]),
                          np.concatenate([np.arange(n_long), [5, 19999]])))
        line = lambda Ai, Ac: Ai == 1  # noqa: E731
    else:  # column 1 of 3 holds all of 20000 rows
        pat = dict(n=3, m=n_long, P=diag_pattern(3, 0)["P"],
                   A=_csc(n_long, 3, np.concatenate([np.arange(n_long), [5, 19999]]),
                          np.concatenate([np.ones(n_long, dtype=np.int64), [0, 2]])))
        line = lambda Ai, Ac: Ac == 1  # noqa: E731
    st = state(pat, family, 106 + 2 * row + descending)
    Ap, Ai, Ax = st["A"]
    sel = np.flatnonzero(line(Ai, cols_of(Ap)))  # storage order
    Ax = Ax.copy()
    Ax[sel] = _sorted_magnitudes(Ax[sel], descending)
    st["A"] = (Ap, Ai, Ax)
    return st


def case_dense_row_ascending(family):
    """one row of A over all of 20000 columns, magnitudes ascending in storage order: every entry could raise the slot"""
    return _dense_line(family, True, False)


def case_dense_row_descending(family):
    """... descending: only the first entry raises it, the others must skip or lose the atomic"""
    return _dense_line(family, True, True)


def case_dense_column_ascending(family):
    return _dense_line(family, False, False)


def case_dense_column_descending(family):
    return _dense_line(family, False, True)


def case_clipped_factors(family):
    """cumulative d and e far down, at 1 and far up, so that rows and columns are clipped below and above"""
    st = state(random_pattern(100, 150, 300, 700, 6), family, 110)
    rng = np.random.default_rng(111)
    # exact: norms are mostly 4^2 or 4^3, factors 1/4 or 1/8: below smin / 2^-11 = 1/4, above smax / 2^16 = 1/8
    lo_, hi_ = (-11, 16) if family == "exact" else (-3.7, 3.7)
    base = 2.0 if family == "exact" else 10.0
    st["d"] = base ** rng.choice([lo_, 0, hi_], 100)
    st["e"] = base ** rng.choice([lo_, 0, hi_], 150)
    if family == "wide":  # norms on both sides of 1, so that 1 / sqrt meets both bounds
        st["P"] = (st["P"][0], st["P"][1], st["P"][2] * 1e-5)
        st["A"] = (st["A"][0], st["A"][1], st["A"][2] * 1e-5)
    return st


def case_c_clipped_below(family):
    """c so small that smin / c is above 1 / max(||q||inf, mean)"""
    st = state(random_pattern(100, 150, 300, 700, 7), family, 112)
    st["c"] = 2.0 ** -12 if family == "exact" else 2e-4
    st["q"] = st["q"] * (4.0 ** 3 if family == "exact" else 1e3)
    return st


def case_c_clipped_above(family):
    st = state(random_pattern(100, 150, 300, 700, 8), family, 113)
    st["c"] = 2.0 ** 12 if family == "exact" else 5e3
    scale = 4.0 ** -6 if family == "exact" else 1e-9
    st["q"] = st["q"] * scale
    st["P"] = (st["P"][0], st["P"][1], st["P"][2] * scale)
    return st


def case_q_zero(family):
    """q = 0: the cost scaling is skipped, cstate[1] == 1.0 exactly and c, P keep their bytes"""
    st = state(random_pattern(100, 150, 300, 700, 9), family, 114)
    st["q"] = np.zeros(100)
    return st


def case_factor_one_by_arithmetic(family):
    """diagonal P = 16 above every entry of its column of A and |q| small: the scaled diagonal is 1, the mean 1 and
    the factor 1 / max(||q||inf, 1) = 1.0 without being skipped (both families take these values)"""
    st = state(diag_pattern(100, 150), "exact", 115)
    st["P"] = (st["P"][0], st["P"][1], np.full(100, 16.0))
    st["A"] = (st["A"][0], st["A"][1], np.clip(st["A"][2], -4.0, 4.0))
    st["q"] = st["q"] * 4.0 ** -4
    st["d"], st["e"] = np.ones(100), np.ones(150)
    return st


def _small(family):
    """times q: ||q||inf far below the mean of the column norms, so that the SUM decides the cost factor"""
    return 4.0 ** -8 if family == "exact" else 1e-13


def sized_case(n, m):
    def case(family):
        st = state(diag_pattern(n, m), family, 200 + n % 97)
        st["q"] = st["q"] * _small(family)
        return st
    case.__doc__ = "diagonal P, one entry per row of A, n = %d, m = %d; q so small that the mean decides" % (n, m)
    return case


RUIZ_CASES = {
    "split_in_wavefront": case_split_in_wavefront, "lp": case_lp, "unconstrained": case_unconstrained,
    "offdiagonal": case_offdiagonal, "zero_row_and_column": case_zero_row_and_column,
    "dense_row_ascending": case_dense_row_ascending, "dense_row_descending": case_dense_row_descending,
    "dense_column_ascending": case_dense_column_ascending, "dense_column_descending": case_dense_column_descending,
    "clipped_factors": case_clipped_factors, "c_clipped_below": case_c_clipped_below,
    "c_clipped_above": case_c_clipped_above, "q_zero": case_q_zero,
    "factor_one_by_arithmetic": case_factor_one_by_arithmetic,
}
# n = 1, 255 | 256 | 257: one block | two of the 256; 65535 | 65536 | 65537: the second trip of the 256 x 256 partition
# of k_eq_cost_partial; 262145 / 262144: nnzP + nnzA, n + m and nnzP + n all one past 2048 x 256
RUIZ_SIZES = [(1, 1), (255, 255), (256, 256), (257, 257), (65535, 300), (65536, 300), (65537, 300), (262145, 262144)]
for _n, _m in RUIZ_SIZES:
    RUIZ_CASES["n%d" % _n] = sized_case(_n, _m)
# what a case must show in the reference's report, checked on the CPU and again where the device runs it
RUIZ_KINDS = {"lp": ("skipped",), "q_zero": ("skipped",), "c_clipped_below": ("clip_lo",), "c_clipped_above": ("clip_hi",),
              "offdiagonal": ("mean",), "factor_one_by_arithmetic": ("mean",), "unconstrained": ("q", "clip_lo")}
RUIZ_KINDS.update({"n%d" % _n: ("mean",) for _n, _m in RUIZ_SIZES})


# ---- the cases of the rectification ------------------------------------------------------------------------------------
RECT_LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 513]


def rect_layout(lengths, gap=(3, 0, 5)):
    """segments of the given lengths with gap[k % 3] unrectified rows between them: the first starts at row 0 and the
    last ends at m -> (m, segments)"""
    segs, row = [], 0
    for k, ln in enumerate(lengths):
        segs.append((row, row + ln))
        row += ln
        if k + 1 < len(lengths):
            row += gap[k % len(gap)]
    return row, segs


def rect_case(name, family):
    """-> (n, m, A with values, b, e, segments)"""
    if name == "lengths":
        m, segs = rect_layout(RECT_LENGTHS)
        n, nnzA = 60, 4 * m
    elif name == "one_segment":
        m, segs, n, nnzA = 300, [(20, 277)], 60, 900
    elif name == "1000_of_3":
        m, segs = rect_layout([3] * 1000, gap=(0, 1, 0))
        n, nnzA = 60, 2 * m
    else:  # "split": nnzA = 100, so entries 100 .. 127 of the second wavefront of k_eq_rect_apply are rows
        m, segs, n, nnzA = 90, [(0, 40), (50, 90)], 30, 100
    rng = np.random.default_rng(len(name))
    pat = random_pattern(n, m, 0, nnzA, 300 + len(name))
    A = pat["A"]
    Ac = cols_of(A[0])
    if name != "split":  # rows of A without entries: two inside the first long cone, one outside every cone
        inside = [s for s in segs if s[1] - s[0] >= 3][0]
        drop = np.isin(A[1], (inside[0], inside[0] + 2)) | (A[1] == (segs[0][1] if segs[0][1] < segs[-1][0] else -1))
        A = _csc(m, n, A[1][~drop], Ac[~drop])
    nA = len(A[1])
    if family == "exact":
        Ax, b, e = _pow(rng, nA, 1, -4, 4), _pow(rng, m, 1, -4, 4), _pow(rng, m, 1, -6, 6, False)
    else:
        Ax, b, e = wide(rng, nA), wide(rng, m), 10.0 ** rng.uniform(-4, 4, m)
    return n, m, (A[0], A[1], Ax), b, e, segs


RECT_CASES = ("lengths", "one_segment", "1000_of_3", "split")


# ---- the cases of the sums of squares ----------------------------------------------------------------------------------
WNORM_SIZES = [1, 255, 256, 257, 65535, 65536, 65537]


def wnorm_vectors(n, family, seed):
    rng = np.random.default_rng(seed)
    if family == "exact":  # (v w)^2 in 2^-12 .. 2^12 and n <= 2^17: every partial sum fits in 42 bits
        v, w = _pow(rng, n, 1, -3, 3), _pow(rng, n, 1, -3, 3, False)
        if n:
            v[-1], w[-1] = 8.0, 8.0  # the entry most easily dropped weighs most
        return v, w
    return wide(rng, n), 10.0 ** rng.uniform(-4, 4, n)
