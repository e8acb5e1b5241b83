"""Plain references of the batched solver's device passes (clarabel.rs_amd/csrc/batch.hip) for
tests/test_batch_plan_host.py and tests/test_batch_passes_gpu.py: the partitions the tests share, the partition
restated from the sizes alone, exact sums (math.fsum on exact products, fractions for the squares), the cone minima and
margins in numpy and mpmath, the second-order cone's step length (socone.rs:421-495) restated sequentially and solved
in mpmath, and the element-wise passes in the kernels' operation order.  Nothing here touches a GPU."""
import math
from fractions import Fraction

import numpy as np

ZERO, NN, SOC = 0, 1, 2
CHUNK = 4096
ROW_ZERO, ROW_NN, ROW_SOC_HEAD, ROW_SOC_TAIL = range(4)
ITEM_NN, ITEM_SOC = 0, 1
EPS = 2.0 ** -53
DBL_MAX = np.finfo(np.float64).max
EDGE_SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 8193]
SOC_DIMS = [2, 3, 255, 256, 257, 258, 513, 5000]  # (a second-order cone of one row is refused: dim >= 2)


# ---- the partitions: (n_part, m_part, cones) ----------------------------------------------------------------------
def _fill(m, pattern):
    """cones of one member with m rows: pattern 0 all Nonnegative, 1 all Zero, 2 Zero / Nonnegative / SOC mixed"""
    if m == 0:
        return []
    if pattern == 0:
        return [(NN, m)]
    if pattern == 1:
        return [(ZERO, m)]
    a = m // 3
    out = [(ZERO, a), (NN, a), (SOC if m - 2 * a >= 2 else NN, m - 2 * a)]
    return [c for c in out if c[1] > 0]


def part_edges():
    """every size at which a chunk, an item or a 256-lane stride changes shape, ordered differently in x and in z"""
    n_part = list(EDGE_SIZES)
    m_part = [4097, 0, 8193, 1, 4096, 257, 255, 4095, 256]
    cones = []
    for k, m in enumerate(m_part):
        cones += _fill(m, k % 3)
    return n_part, m_part, cones


def part_cones():
    """Nonnegative cones of 1, 4096, 4097 and 9000 rows, second-order cones of 2, 257 and 5000 rows, members of
    Zero rows only (one of them over two chunks) and a member without rows"""
    members = [[(NN, 9000)], [(ZERO, 5)], [(SOC, 5000), (NN, 1)], [(NN, 4096), (SOC, 2)],
               [(ZERO, 3), (NN, 4097), (SOC, 257), (SOC, 2), (ZERO, 2)], [], [(ZERO, 4097)], [(SOC, 2)], [(NN, 1)]]
    n_part = [3, 0, 4097, 1, 256, 7, 2, 5, 4096]
    return n_part, [sum(c[1] for c in mb) for mb in members], [c for mb in members for c in mb]


def assemble(members):
    """(n_part, m_part, cones) of a list of members (columns, [cones])"""
    return ([mb[0] for mb in members], [sum(c[1] for c in mb[1]) for mb in members],
            [c for mb in members for c in mb[1]])


def tiny_members(nprob):
    """nprob members of at most 3 columns and 6 rows, second-order cones of at most 3 rows (a tail of two entries adds
    up the same in any order): the per-member kernels run a second (from 257) and a third (600) workgroup"""
    kinds = [[(NN, 2)], [], [(ZERO, 1), (NN, 3)], [(SOC, 3)], [(NN, 1), (SOC, 2), (NN, 2)], [(ZERO, 2)], [(SOC, 2)],
             [(ZERO, 1), (SOC, 3), (NN, 2)]]
    return [((k * 7 + 1) % 4, kinds[(k * 5 + k // 8) % len(kinds)]) for k in range(nprob)]


def part_tiny(nprob):
    return assemble(tiny_members(nprob))


def part_socs(dims=SOC_DIMS):
    """one second-order cone per member"""
    return [1] * len(dims), list(dims), [(SOC, d) for d in dims]


def part_nn(sizes):
    """one Nonnegative cone per member (0: a member without rows)"""
    return [1] * len(sizes), list(sizes), [(NN, s) for s in sizes if s]


def part_large():
    """n + 2 m above 2048 * 256 entries, so that the element-wise kernels' grid-stride loops take a second trip"""
    n_part, m_part = [60000, 1, 40003], [9000, 100000, 110001]
    return n_part, m_part, [(NN, 9000), (ZERO, 50000), (SOC, 50000), (NN, 110001)]


# ---- the partition restated from the sizes -------------------------------------------------------------------------
def offsets(part):
    return np.concatenate([[0], np.cumsum(np.asarray(part, dtype=np.int64))]).astype(np.int64)


def members_of(part):
    return np.repeat(np.arange(len(part)), np.asarray(part, dtype=np.int64))


def row_types(m_part, cones):
    rt = np.full(int(sum(m_part)), ROW_ZERO, dtype=np.int32)
    r = 0
    for tag, dim in cones:
        if tag == NN:
            rt[r:r + dim] = ROW_NN
        elif tag == SOC and dim:
            rt[r] = ROW_SOC_HEAD
            rt[r + 1:r + dim] = ROW_SOC_TAIL
        r += dim
    return rt


def cone_ranges(cones):
    """[(tag, first row, end row)] of the cones with rows"""
    out, r = [], 0
    for tag, dim in cones:
        if dim:
            out.append((tag, r, r + dim))
        r += dim
    return out


# ---- data ----------------------------------------------------------------------------------------------------------
def f32_exact(rng, size, lo=-3.0, hi=3.0):
    """doubles with a 24-bit significand and magnitudes 10^lo .. 10^hi: the product of two is exact in float64"""
    mant = rng.standard_normal(size).astype(np.float32).astype(np.float64)
    mant[mant == 0.0] = 1.0
    expo = np.floor(rng.uniform(lo, hi, size) * math.log2(10.0))
    return np.ldexp(mant, expo.astype(np.int64))


def cancelling(rng, size):
    """pairs (v, -v) of magnitudes up to 1e6 in random positions, a few pairs (and an odd entry) replaced by small
    independent values: the sum is tiny against the sum of magnitudes"""
    v = f32_exact(rng, size, 0.0, 6.0)
    half = size // 2
    v[half:2 * half] = -v[:half]
    if half:
        idx = rng.integers(0, half, max(1, half // 25))
        v[idx] = f32_exact(rng, len(idx), -6.0, -3.0)
        v[half + idx] = f32_exact(rng, len(idx), -6.0, -3.0)
    v[2 * half:] = f32_exact(rng, size - 2 * half, -6.0, -3.0)
    return v[rng.permutation(size)]


# ---- exact sums ------------------------------------------------------------------------------------------------------
def seg_exact(kind, a, b, off):
    """per member: (the correctly rounded sum, S = the sum of the terms' magnitudes, L).  kind "dot": sum a b with
    exact products; "wsq": sum (a b)^2 in fractions; "sum": sum a"""
    exact, mags, lens = [], [], []
    for k in range(len(off) - 1):
        av = a[off[k]:off[k + 1]]
        if kind == "sum":
            t = av
        else:
            t = av * b[off[k]:off[k + 1]]
        if kind == "wsq":
            tot = sum((Fraction(float(v)) ** 2 for v in t), Fraction(0))
            exact.append(float(tot))
            mags.append(float(tot))
        else:
            exact.append(math.fsum(t))
            mags.append(math.fsum(np.abs(t)))
        lens.append(len(t))
    return np.array(exact), np.array(mags), np.array(lens)


def sum_bound(lens, mags):
    """|any-order float64 sum - exact| <= (L - 1) u S to first order, the products of "wsq" add 2 u S, the reference's
    own rounding u S: (L + 4) 2^-53 S covers them with the second-order terms for every L here"""
    return (np.asarray(lens) + 4) * EPS * np.asarray(mags)


def count_nonfinite(a, b, off):
    bad = ~np.isfinite(a)
    cnt = bad.astype(np.float64)
    if b is not None:
        cnt = cnt + (~np.isfinite(b)).astype(np.float64)
    return np.array([cnt[off[k]:off[k + 1]].sum() for k in range(len(off) - 1)])


# ---- cones -----------------------------------------------------------------------------------------------------------
def nn_step(z, dz, s, ds, amax, m_part, cones):
    """nonnegativecone.rs:128-153 per member over its Nonnegative rows, from amax[k]"""
    zoff, rt = offsets(m_part), row_types(m_part, cones)
    out = np.array(amax, dtype=np.float64).copy()
    for k in range(len(m_part)):
        sl = slice(zoff[k], zoff[k + 1])
        nn = rt[sl] == ROW_NN
        for v, dv in ((z[sl][nn], dz[sl][nn]), (s[sl][nn], ds[sl][nn])):
            neg = dv < 0.0
            if neg.any():
                out[k] = min(out[k], float(np.min(-v[neg] / dv[neg])))
    return out


def soc_margin_mp(x, prec=300):
    """x0 - ||x1|| and |x0| + ||x1|| in mpmath"""
    import mpmath
    with mpmath.workprec(prec):
        nrm = mpmath.sqrt(mpmath.fsum(mpmath.mpf(float(v)) ** 2 for v in x[1:]))
        return float(mpmath.mpf(float(x[0])) - nrm), float(abs(mpmath.mpf(float(x[0]))) + nrm)


def soc_margin_tol(dim, scale):
    """the scaled norm of dim - 1 entries in any order, its square root and the subtraction"""
    return (dim + 4) * EPS * scale


def soc_step_roots(x0, y0, x1n, y1n, x1y1, amax):
    """socone.rs:421-495 (batch.hip's soc_step_roots) in Python floats, from the reduced quantities"""
    if x0 >= 0.0 and y0 < 0.0:
        amax = min(amax, -x0 / y0)
    a = (y0 - y1n) * (y0 + y1n)
    b = 2.0 * (x0 * y0 - x1y1)
    cres = (x0 - x1n) * (x0 + x1n)
    c = cres if cres > 0.0 else 0.0
    d = b * b - 4.0 * a * c
    if (a > 0.0 and b > 0.0) or d < 0.0:
        return amax
    if a == 0.0:
        return amax
    if c == 0.0:
        return amax if a >= 0.0 else 0.0
    t = (-b - math.sqrt(d)) if b >= 0.0 else (-b + math.sqrt(d))
    r1, r2 = (2.0 * c) / t, t / (2.0 * a)
    if r1 < 0.0:
        r1 = math.inf
    if r2 < 0.0:
        r2 = math.inf
    return min(amax, min(r1, r2))


def soc_step_seq(x, y, amax):
    """the step length of one pair (x, y) with sequential float64 norms and dot (numpy), socone.rs:289-302"""
    x, y = np.asarray(x, float), np.asarray(y, float)
    x1n = float(np.sqrt(np.sum(x[1:] * x[1:]))) if len(x) > 1 else 0.0
    y1n = float(np.sqrt(np.sum(y[1:] * y[1:]))) if len(x) > 1 else 0.0
    x1y1 = float(np.sum(x[1:] * y[1:])) if len(x) > 1 else 0.0
    return soc_step_roots(float(x[0]), float(y[0]), x1n, y1n, x1y1, amax)


def soc_step_mp(x, y, amax, prec=400):
    """the largest alpha in [0, amax] with x + alpha y in the cone, for x strictly inside, in mpmath: the linear cap
    and the smallest positive root of (x0 + alpha y0)^2 = ||x1 + alpha y1||^2"""
    import mpmath
    with mpmath.workprec(prec):
        X = [mpmath.mpf(float(v)) for v in x]
        Y = [mpmath.mpf(float(v)) for v in y]
        a = Y[0] ** 2 - mpmath.fsum(v ** 2 for v in Y[1:])
        b = 2 * (X[0] * Y[0] - mpmath.fsum(u * v for u, v in zip(X[1:], Y[1:])))
        c = X[0] ** 2 - mpmath.fsum(v ** 2 for v in X[1:])
        assert c > 0
        best = mpmath.mpf(float(amax))
        if Y[0] < 0:
            best = min(best, -X[0] / Y[0])
        if a == 0:
            roots = [-c / b] if b != 0 else []
        else:
            d = b * b - 4 * a * c
            assert d >= 0  # the reversed Cauchy-Schwarz inequality for x inside the cone
            sq = mpmath.sqrt(d)
            roots = [(-b - sq) / (2 * a), (-b + sq) / (2 * a)]
        for r in roots:
            if r > 0:
                best = min(best, r)
        return float(best), float(c / X[0] ** 2)


def soc_step_cases(rng, dim, count):
    """`count` strictly interior z and s of one cone of `dim` rows with random directions; x0^2 - ||x1||^2 is kept at
    or above 5% of x0^2 (||x1|| <= 0.97 x0), and |y0^2 - ||y1||^2| at or above 5% of y0^2, so the quadratic's
    coefficients are well conditioned"""
    out = []
    for _ in range(count):
        vecs = []
        for _ in range(2):
            x = rng.standard_normal(dim)
            nrm = float(np.linalg.norm(x[1:])) if dim > 1 else 0.0
            x[0] = (nrm if nrm > 0.0 else 1.0) / rng.uniform(0.1, 0.97)
            x *= 10.0 ** rng.uniform(-2, 2)
            y = rng.standard_normal(dim) * float(np.abs(x[0])) * 10.0 ** rng.uniform(-1, 1)
            ynrm = float(np.linalg.norm(y[1:]))
            while True:  # both signs of a = y0^2 - ||y1||^2, and a at or above 5% of y0^2 in magnitude
                y0 = ynrm * rng.uniform(0.2, 1.5) * rng.choice([-1.0, 1.0])
                if abs(1.0 - (ynrm / y0) ** 2) >= 0.05:
                    break
            y[0] = y0
            vecs += [x, y]
        out.append(tuple(vecs))  # (z, dz, s, ds)
    return out


# ---- the element-wise passes in the kernels' operation order ---------------------------------------------------------
def blin_ref(w, x, y, sa, sb, ca, cb, mem, mask, mode):
    """k_blin: returns the new w (w, x, y may be the same array)"""
    out = w.copy()
    ak = sa[mem] if sa is not None else np.full(len(mem), ca)
    on = np.ones(len(mem), bool) if mask is None else (np.asarray(mask)[mem] != 0)
    with np.errstate(all="ignore"):
        if y is not None:
            bk = sb[mem] if sb is not None else np.full(len(mem), cb)
            val = ak * x + bk * y
        else:
            val = ak * x
    out[on] = val[on]
    if mode == 0:
        out[~on] = 0.0
    elif mode == 1:
        out[~on] = y[~on]
    return out


def bresid_ref(rx_inf, Px, q, rz_inf, b, tau, xmem, zmem):
    with np.errstate(all="ignore"):
        rx = 1.0 * rx_inf + -1.0 * Px + (-tau[xmem]) * q
        rz = 1.0 * rz_inf + (-tau[zmem]) * b
    return rx, rz


def bunit_shift_ref(z, alpha, primal, mask, zmem, rt):
    out = z.copy()
    on = np.ones(len(z), bool) if mask is None else (np.asarray(mask)[zmem] != 0)
    head = on & ((rt == ROW_NN) | (rt == ROW_SOC_HEAD))
    with np.errstate(all="ignore"):
        out[head] = z[head] + alpha[zmem][head]
    if primal:
        out[on & (rt == ROW_ZERO)] = 0.0
    return out


def bunit_reset_ref(x, s, z, flag, xmem, zmem, rt):
    flag = np.asarray(flag)
    xo, so, zo = x.copy(), s.copy(), z.copy()
    xo[flag[xmem] != 0] = 0.0
    on = flag[zmem] != 0
    e = np.where((rt == ROW_NN) | (rt == ROW_SOC_HEAD), 1.0, 0.0)
    so[on] = e[on]
    zo[on] = e[on]
    return xo, so, zo


def bunscale_ref(x, d, z, e, s, einv, sx, sz, xmem, zmem):
    with np.errstate(all="ignore"):
        return (x * d) * sx[xmem], (z * e) * sz[zmem], (s * einv) * sx[zmem]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
