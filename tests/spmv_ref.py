"""References and inputs for the residual pass of the single solver (kktsystem.cpp residuals_pass): no GPU, no package.

The pass computes, from the caller's P (upper triangle, CSC), A (CSC), q, b and a point (x, z, s, tau):
    Px = P x (P symmetric: every off-diagonal entry is used twice), rx_inf = -A'z, rz_inf = A x + s,
    rx = rx_inf - Px - tau q, rz = rz_inf - tau b,
the dots q.x, b.z, s.z, x.Px and the norms of x, z, s, rz, rx.

row_terms() lists, per output entry, the double-precision terms whose exact sum the entry is (each product rounded
once, as every double evaluation without contraction has it), and returns math.fsum of each list with the bound
    (L + 4) 2^-53 fsum(|terms|),   L the number of terms.
Why it holds for any order of summation: the products' roundings add up to at most u S (u = 2^-53, S = fsum|terms|; a
fused multiply-add only removes them), L terms summed in any tree lose at most (L - 1) u S to first order, alpha = +-1 is
exact, the aux step and the reference's own product roundings and final rounding are u S and 1.5 u S more: (L + 2.5) u S,
second-order terms (L u)^2 S at L = 21600 far below the remaining 1.5 u S.  The chunks of a workgroup row meet in atomic
adds in arrival order: still a summation tree over the same L terms.  rx and rz are computed from the rounded rx_inf, Px
and rz_inf with three and two more roundings of at most u S each; their L counts the terms of all their parts plus the
q or b term, which leaves room for them as soon as one part has a term (and an entry without any is exact).

Dots: (n + 4) u fsum|a_i b_i| by the same argument.  A norm is the square root of such a sum of squares, whose terms are
all positive: with e = (n + 4) u the device's sum is within (1 +- e) of the exact one, the root within
sqrt(1 +- e) <= 1 +- e (1 + e) / 2, and the two square roots (device, reference) round once each: norm_ref().

Two input families per problem.  integer_point(): every value of P, A, q, b, x, z, s in {-4..4} \\ {0}, tau = 2 -- all
partial sums are integers far below 2^53, so every output is exact in every order and the device must return the
reference's bits; the last entry of every long row of every operator is +-4 with the sign that makes its product
positive and the last entry of every vector is +4, so the element most easily dropped weighs most.  wide_point():
standard_normal * 10^uniform(-6, 6) per entry, for the per-entry bound (a norm-wise comparison hides its small rows)."""
import math

import numpy as np

U = 2.0 ** -53
T_MAX, B_MIN, B_CHUNK = 32, 16384, 4096  # the row classes of build_spmat (kktsystem.cpp)

ROW_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 4095, 4096, 4097, 16383, 16384, 16385,
               20480, 20481, 21503, 21600]
ROWS_N = 21600
P_WAVE_ROW, P_WAVE_OFFDIAG, P_EMPTY = 100, 300, 7777  # rows_problem's P: the wavefront row, the empty row and column
COL_LENGTHS = [0, 1, 33, 257, 16385, 21503]
COLS_M = 21600
VECTOR_SIZES = [1, 255, 256, 257, 131072, 131073, 524288, 524289]


# ---- problems ------------------------------------------------------------------------------------------------------
def _csc(m, n, rows, cols):
    """pattern (colptr, rowval) of the entries (rows[k], cols[k]), sorted by column, then row"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((rows, cols))
    colptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=colptr[1:])
    return colptr, rows[order]


def _problem(n, m, P, A):
    return dict(n=n, m=m, P=P, A=A, cones=[(1, m)])  # one Nonnegative cone


def rows_problem(seed=11):
    """n = 21600, one row of A per length in ROW_LENGTHS (columns at random).  P: the diagonal, a dense first row and
    P_WAVE_OFFDIAG off-diagonals in row P_WAVE_ROW, without anything in row and column P_EMPTY: the symmetric row 0 has
    n - 1 entries (workgroup class), row P_WAVE_ROW 302 (wavefront), P_EMPTY none, every other row two or three"""
    rng = np.random.default_rng(seed)
    n, m = ROWS_N, len(ROW_LENGTHS)
    ar, ac = [], []
    for i, ln in enumerate(ROW_LENGTHS):
        ar.append(np.full(ln, i))
        ac.append(np.sort(rng.choice(n, ln, replace=False)))
    A = _csc(m, n, np.concatenate(ar), np.concatenate(ac))
    keep = np.array([j for j in range(n) if j != P_EMPTY])
    others = keep[keep > P_WAVE_ROW]
    wave = np.sort(rng.choice(others, P_WAVE_OFFDIAG, replace=False))
    pr_ = np.concatenate([keep, np.zeros(len(keep) - 1, dtype=np.int64), np.full(P_WAVE_OFFDIAG, P_WAVE_ROW)])
    pc_ = np.concatenate([keep, keep[1:], wave])
    P = _csc(n, n, pr_, pc_)
    return _problem(n, m, P, A)


def cols_problem(seed=12):
    """n = 6, m = 21600: one column of A per length in COL_LENGTHS (rows at random), P without entries"""
    rng = np.random.default_rng(seed)
    n, m = len(COL_LENGTHS), COLS_M
    ar, ac = [], []
    for j, ln in enumerate(COL_LENGTHS):
        ar.append(np.sort(rng.choice(m, ln, replace=False)))
        ac.append(np.full(ln, j))
    A = _csc(m, n, np.concatenate(ar), np.concatenate(ac))
    P = (np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64))
    return _problem(n, m, P, A)


def vector_problem(n, m):
    """P the n x n diagonal, A m x n with one entry per row, row i in column i mod n"""
    P = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64))
    A = _csc(m, n, np.arange(m), np.arange(m) % n)
    return _problem(n, m, P, A)


def a_row_lengths(pr):
    return np.bincount(pr["A"][1], minlength=pr["m"])


def a_col_lengths(pr):
    return np.diff(pr["A"][0])


def psym_row_lengths(pr):
    """rows of the full symmetric P: an entry (r, c) of the upper triangle counts in row r and, off the diagonal, in c"""
    r, c = pr["P"][1], _cols_of(pr["P"][0])
    assert np.all(r <= c)
    return np.bincount(r, minlength=pr["n"]) + np.bincount(c[r != c], minlength=pr["n"])


def row_class(length):
    return "workgroup" if length > B_MIN else "wavefront" if length > T_MAX else "thread"


def chunk_lengths(length):
    """the pieces build_spmat cuts a workgroup row into"""
    return [min(B_CHUNK, length - b) for b in range(0, length, B_CHUNK)] if length > B_MIN else []


def _cols_of(colptr):
    return np.repeat(np.arange(len(colptr) - 1, dtype=np.int64), np.diff(colptr))


# ---- inputs --------------------------------------------------------------------------------------------------------
def _ints(rng, k):
    return (rng.integers(1, 5, k) * rng.choice([-1, 1], k)).astype(float)


def _last_of_long_groups(group, other, count):
    """positions (into entry arrays ordered by column, then row) of the last entry -- the largest `other` index -- of
    every group with more than T_MAX entries"""
    lens = np.bincount(group, minlength=count)
    order = np.lexsort((other, group))
    ends = np.cumsum(lens)[lens > T_MAX] - 1
    return order[ends]


def integer_point(pr, seed):
    """-> dict(Pv, Av, q, b, x, z, s, tau, kappa) of the integer family"""
    rng = np.random.default_rng(seed)
    n, m = pr["n"], pr["m"]
    v = dict(q=_ints(rng, n), b=_ints(rng, m), x=_ints(rng, n), z=_ints(rng, m), s=_ints(rng, m), tau=2.0, kappa=3.0)
    for k in ("q", "b", "x", "z", "s"):
        v[k][-1] = 4.0
    Pv, Av = _ints(rng, len(pr["P"][1])), _ints(rng, len(pr["A"][1]))
    x, z = v["x"], v["z"]
    ar, ac = pr["A"][1], _cols_of(pr["A"][0])
    t = _last_of_long_groups(ar, ac, m)  # long rows of A: the product with x positive
    Av[t] = 4.0 * np.sign(x[ac[t]])
    t = _last_of_long_groups(ac, ar, n)  # long columns of A: the product with z positive
    Av[t] = 4.0 * np.sign(z[ar[t]])
    r, c = pr["P"][1], _cols_of(pr["P"][0])
    if len(r):  # long rows of the symmetric P: entry (r, c) serves row r (with x_c) and, off the diagonal, row c (with x_r)
        off = r != c
        grp, oth = np.concatenate([r, c[off]]), np.concatenate([c, r[off]])
        src = np.concatenate([np.arange(len(r)), np.arange(len(r))[off]])
        t = _last_of_long_groups(grp, oth, n)
        Pv[src[t]] = 4.0 * np.sign(x[oth[t]])
    v.update(Pv=Pv, Av=Av)
    return v


def wide_point(pr, seed):
    """-> the same dict, every entry standard_normal * 10^uniform(-6, 6)"""
    rng = np.random.default_rng(seed)

    def wide(k):
        return rng.standard_normal(k) * 10.0 ** rng.uniform(-6.0, 6.0, k)

    n, m = pr["n"], pr["m"]
    return dict(q=wide(n), b=wide(m), x=wide(n), z=wide(m), s=wide(m), tau=1.3, kappa=0.7, Pv=wide(len(pr["P"][1])),
                Av=wide(len(pr["A"][1])))


# ---- references ----------------------------------------------------------------------------------------------------
def fsum_groups(terms, ptr):
    """math.fsum of terms[ptr[i]:ptr[i + 1]] per i.  (A group of one term is that term and a group of two is their
    correctly rounded sum, which IEEE addition is too: those are taken without the loop.)"""
    ptr = np.asarray(ptr, dtype=np.int64)
    lens = np.diff(ptr)
    out = np.zeros(len(lens))
    one, two = lens == 1, lens == 2
    out[one] = terms[ptr[:-1][one]]
    out[two] = terms[ptr[:-1][two]] + terms[ptr[:-1][two] + 1]
    rest = np.flatnonzero(lens > 2)
    if len(rest):
        tl = terms.tolist()
        out[rest] = [math.fsum(tl[a:b]) for a, b in zip(ptr[rest].tolist(), ptr[rest + 1].tolist())]
    return out


def _grouped(n_out, groups, values):
    """the terms `values`, each belonging to output `groups[k]`, ordered by output -> (terms, ptr)"""
    groups = np.concatenate(groups)
    values = np.concatenate(values)
    order = np.argsort(groups, kind="stable")
    ptr = np.zeros(n_out + 1, dtype=np.int64)
    np.cumsum(np.bincount(groups, minlength=n_out), out=ptr[1:])
    return values[order], ptr


def with_values(pr, v):
    """the problem as the caller holds it: P = (colptr, rowval, nzval) upper triangle, A likewise, q, b"""
    return dict(pr, P=(pr["P"][0], pr["P"][1], v["Pv"]), A=(pr["A"][0], pr["A"][1], v["Av"]), q=v["q"], b=v["b"])


def term_lists(pr, x, z, s, tau):
    """-> {output: (terms, ptr)}: the double-precision terms of every entry of Px, rx_inf, rz_inf, rx, rz"""
    n, m = pr["n"], pr["m"]
    pr_, pc_, Pv = pr["P"][1], _cols_of(pr["P"][0]), pr["P"][2]
    ar, ac, Av = pr["A"][1], _cols_of(pr["A"][0]), pr["A"][2]
    off = pr_ != pc_
    # P x: entry (r, c) gives P_rc x_c to row r and, off the diagonal, P_rc x_r to row c
    pg = [pr_, pc_[off]]
    pv = [Pv * x[pc_], Pv[off] * x[pr_[off]]]
    atz = -(Av * z[ar])  # -(A'z)_c: alpha = -1 is exact
    ax = Av * x[ac]
    jn, im = np.arange(n), np.arange(m)
    return {"Px": _grouped(n, pg, pv),
            "rx_inf": _grouped(n, [ac], [atz]),
            "rz_inf": _grouped(m, [ar, im], [ax, s]),
            "rx": _grouped(n, [ac] + pg + [jn], [atz] + [-t for t in pv] + [-(tau * pr["q"])]),
            "rz": _grouped(m, [ar, im, im], [ax, s, -(tau * pr["b"])])}


def row_terms(pr, x, z, s, tau):
    """pr with values (with_values) -> {output: (reference, bound, L)} for Px, rx_inf, rz_inf, rx, rz: math.fsum of each
    entry's terms, (L + 4) 2^-53 fsum(|terms|) and the term counts L"""
    out = {}
    for key, (terms, ptr) in term_lists(pr, x, z, s, tau).items():
        L = np.diff(ptr)
        out[key] = (fsum_groups(terms, ptr), (L + 4) * U * fsum_groups(np.abs(terms), ptr), L)
    return out


def reference(pr, v):
    return row_terms(with_values(pr, v), v["x"], v["z"], v["s"], v["tau"])


def dot_ref(a, b):
    """-> (fsum of the rounded products, (n + 4) 2^-53 fsum|a_i b_i|)"""
    t = np.asarray(a, dtype=float) * np.asarray(b, dtype=float)
    return math.fsum(t.tolist()), (len(t) + 4) * U * math.fsum(np.abs(t).tolist())


def norm_ref(a):
    """-> (sqrt of the fsum of squares, its bound): see the module docstring"""
    sq, _ = dot_ref(a, a)
    e = (len(a) + 4) * U
    nrm = math.sqrt(sq)
    return nrm, nrm * (0.5 * e * (1.0 + e) + 2.0 * U)


def rtau_host(qx, bz, kappa, xPx, tau):
    """residuals_pass composes rtau on the host from the device's dots, in this order"""
    return qx + bz + kappa + xPx / tau


# ---- dense restatement, for the host tests -------------------------------------------------------------------------
def dense(pr, v):
    """-> (P full symmetric, A) as dense arrays"""
    n, m = pr["n"], pr["m"]
    P, A = np.zeros((n, n)), np.zeros((m, n))
    r, c = pr["P"][1], _cols_of(pr["P"][0])
    P[r, c] = v["Pv"]
    P[c, r] = v["Pv"]
    A[pr["A"][1], _cols_of(pr["A"][0])] = v["Av"]
    return P, A


# ---- the comparison both test modules use ----------------------------------------------------------------------------
OUTPUTS = ("Px", "rx_inf", "rz_inf", "rx", "rz")
DOTS = (("dot_qx", "q", "x"), ("dot_bz", "b", "z"), ("dot_sz", "s", "z"))
NORMS = ("x", "z", "s", "rz", "rx")  # the order of residuals_update(norms=True)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=float), np.ascontiguousarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def _ratio(err, bound):
    """largest err / bound; an error where the bound is 0 (or a NaN) counts as infinite"""
    err, bound = np.atleast_1d(np.asarray(err, dtype=float)), np.atleast_1d(np.asarray(bound, dtype=float))
    r = np.where(err == 0.0, 0.0, np.where((bound > 0.0) & np.isfinite(err), err / np.where(bound > 0.0, bound, 1.0), np.inf))
    k = int(np.argmax(r)) if len(r) else 0
    return (float(r[k]) if len(r) else 0.0), k


def compare(pr, v, got, exact):
    """got: what the pass returned for the point v -- the five vectors of OUTPUTS, dot_qx, dot_bz, dot_sz, dot_xPx, rtau
    and norms in the order of NORMS.  -> (ratios, failures): per output the largest error / bound, and a line per output
    that is outside its bound or -- exact: the integer family -- not the reference's bits.  x.Px and the norms of rz and
    rx are referred to the Px, rz and rx that were returned (their entries are compared on their own)."""
    ratios, fails = {}, []
    ref = reference(pr, v)
    for key in OUTPUTS:
        want, bound, L = ref[key]
        have = np.asarray(got[key], dtype=float)
        ratios[key], k = _ratio(np.abs(have - want), bound)
        if ratios[key] > 1.0 or (exact and not same_bits(have, want)):
            k = k if ratios[key] > 0.0 else int(np.flatnonzero(have.view(np.int64) != want.view(np.int64))[0])
            fails.append("%s[%d] (%d terms): %r, reference %r, bound %.3e" % (key, k, L[k], have[k], want[k], bound[k]))

    def scalar(name, have, want, bound):
        ratios[name], _ = _ratio(abs(have - want), bound)
        if ratios[name] > 1.0 or (exact and not same_bits([have], [want])):
            fails.append("%s: %r, reference %r, bound %.3e" % (name, have, want, bound))

    for name, a, b in DOTS:
        scalar(name, got[name], *dot_ref(v[a], v[b]))
    if len(pr["P"][1]):
        scalar("dot_xPx", got["dot_xPx"], *dot_ref(v["x"], got["Px"]))
    else:  # without P the pass zeroes Px and reports 0
        scalar("dot_xPx", got["dot_xPx"], 0.0, 0.0)
        if not same_bits(got["Px"], np.zeros(pr["n"])):
            fails.append("Px is not +0 everywhere although P has no entries")
    want = rtau_host(got["dot_qx"], got["dot_bz"], v["kappa"], got["dot_xPx"], v["tau"])
    if not same_bits([got["rtau"]], [want]):
        fails.append("rtau: %r, composed from the returned dots %r" % (got["rtau"], want))
    for k, name in enumerate(NORMS):
        scalar("norm_" + name, got["norms"][k], *norm_ref(got[name] if name in got else v[name]))
    return ratios, fails
