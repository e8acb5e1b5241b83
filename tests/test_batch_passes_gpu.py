"""The device passes of the batched L4 solver (clarabel.rs_amd/csrc/batch.hip) on the MI355X, each launched alone
through the chip_debug_bplan_* hooks on the plan chip_batch_create builds, against the references of
tests/batch_pass_ref.py: segmented sums against exact sums, cone minima bitwise against numpy and against mpmath,
the element-wise passes bitwise against numpy in the kernels' operation order, and the Ruiz step of a stack against the
numpy restatement of tests/test_solver_gpu.py.  The partitions put member, chunk and item boundaries at every size where
a kernel changes shape (tests/test_batch_plan_host.py checks the partitions themselves)."""
import functools
import math

import numpy as np
import pytest

from tests import batch_pass_ref as R
from tests import e2e_problems as E

pytestmark = pytest.mark.gpu

ZERO, NN, SOC = R.ZERO, R.NN, R.SOC
bits = R.bits


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


_PLANS = {}


def plan_of(hip, name, make):
    """one BatchPlanDebug (and its partition) per named partition for the whole module"""
    if name not in _PLANS:
        part = make()
        _PLANS[name] = (hip.BatchPlanDebug(*part), part)
    return _PLANS[name]


# ---- segmented sums ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seg_data():
    """the operands of the sums on part_edges(), per space: plain (24-bit significands), heavily cancelling, and spread
    over 1e-150 .. 1e150; and the exact results per (kind, space, data)"""
    n_part, m_part, _ = R.part_edges()
    rng = np.random.default_rng(20240)
    data = {}
    for sp_, part in ((0, n_part), (1, m_part)):
        size = int(sum(part))
        data[sp_] = dict(a=R.f32_exact(rng, size), b=R.f32_exact(rng, size),
                         cancel=np.concatenate([R.cancelling(rng, p) for p in part]),
                         wide=R.f32_exact(rng, size, -150.0, 150.0), off=R.offsets(part))
        data[sp_]["cabs"] = np.abs(data[sp_]["cancel"])  # v |v| and (-v) |v| cancel as v and -v do
    return data


@functools.lru_cache(maxsize=None)
def seg_ref(kind, sp_, an, bn):
    d = seg_data()[sp_]
    return R.seg_exact(kind, d[an], d[bn] if bn else None, d["off"])


KIND = {"dot": 0, "wsq": 1, "sum": 2}
# (kind, a, b): the cancelling and the wide data only where a single product cannot overflow
SEG_CASES = [("dot", "a", "b"), ("wsq", "a", "b"), ("sum", "a", None), ("sum", "cancel", None), ("dot", "cancel", "cabs"),
             ("sum", "wide", None), ("dot", "wide", "b"), ("wsq", "cancel", "b")]


def check_sum(got, kind, sp_, an, bn, what):
    exact, mags, lens = seg_ref(kind, sp_, an, bn)
    tol = R.sum_bound(lens, mags)
    err = np.abs(got - exact)
    print(what, "max err / bound: %.3g" % float(np.max(err / np.where(tol > 0, tol, 1.0), initial=0.0)))
    assert np.all(err <= tol), (what, np.nonzero(err > tol)[0], err, tol)
    empty = lens == 0
    assert np.array_equal(bits(got[empty]), bits(np.zeros(int(empty.sum())))), what  # an empty member gives +0


@pytest.mark.parametrize("sp_", [0, 1], ids=["x", "z"])
@pytest.mark.parametrize("kind,an,bn", SEG_CASES, ids=["%s-%s" % (c[0], c[1]) for c in SEG_CASES])
def test_seg_one_spec_against_exact_sum(hipdev, kind, an, bn, sp_):
    pl, _ = plan_of(hipdev, "edges", R.part_edges)
    d = seg_data()[sp_]
    out = pl.seg_reduce([(KIND[kind], sp_, 0, d[an], d[bn] if bn else None)], 1, fill=np.nan)
    check_sum(out[0], kind, sp_, an, bn, (kind, an, sp_))
    if an == "cancel" and kind != "wsq":  # the data do cancel: the sums are far below the sums of magnitudes
        exact, mags, lens = seg_ref(kind, sp_, an, bn)
        big = lens >= 255
        assert np.all(np.abs(exact[big]) <= 1e-8 * mags[big])


def test_seg_sixteen_specs_in_one_batch(hipdev):
    """SEG_MAX specs of mixed kinds and both spaces into non-contiguous slots: every spec against its exact sum and
    bitwise equal to the same spec run alone; slots no spec names stay untouched"""
    pl, _ = plan_of(hipdev, "edges", R.part_edges)
    d = seg_data()
    cases = [(c, sp_) for c in SEG_CASES for sp_ in (1, 0)]
    assert len(cases) == pl.SEG_MAX
    slots = [37, 2, 11, 0, 5, 30, 23, 8, 3, 19, 14, 39, 26, 6, 33, 17]
    specs = [(KIND[k], sp_, sl, d[sp_][an], d[sp_][bn] if bn else None) for ((k, an, bn), sp_), sl in zip(cases, slots)]
    out = pl.seg_reduce(specs, 40, fill=-7.0)
    for ((k, an, bn), sp_), sl, spec in zip(cases, slots, specs):
        check_sum(out[sl], k, sp_, an, bn, (k, an, sp_, sl))
        alone = pl.seg_reduce([spec[:2] + (0,) + spec[3:]], 1)
        assert np.array_equal(bits(out[sl]), bits(alone[0])), (k, an, sp_)
    rest = sorted(set(range(40)) - set(slots))
    assert np.all(out[rest] == -7.0)
    assert np.array_equal(bits(pl.seg_reduce(specs, 40, fill=-7.0)), bits(out))  # two runs are bitwise equal


def test_seg_nonfinite_counts(hipdev):
    pl, (n_part, m_part, _) = plan_of(hipdev, "edges", R.part_edges)
    d = seg_data()
    bad = [np.nan, np.inf, -np.inf]
    for sp_, part in ((0, n_part), (1, m_part)):
        off = R.offsets(part)
        a, b = d[sp_]["a"].copy(), d[sp_]["wide"].copy()
        k8 = part.index(8193)
        spots = [off[k8] + i for i in (0, 255, 256, 4095, 4096, 8192)]
        for k in (part.index(4097), part.index(4096), part.index(257), part.index(1)):  # their first and last entries
            spots += [off[k], off[k + 1] - 1]
        spots = list(dict.fromkeys(int(i) for i in spots))
        for j, i in enumerate(spots):
            a[i] = bad[j % 3]
        for j, i in enumerate(spots[::2] + [off[k8] + 1000, off[part.index(255)] + 254]):
            b[i] = bad[(j + 1) % 3]
        out = pl.seg_reduce([(pl.SEG_NONFINITE, sp_, 0, a, None), (pl.SEG_NONFINITE, sp_, 2, a, b),
                             (pl.SEG_NONFINITE, sp_, 1, d[sp_]["wide"], None)], 3, fill=np.nan)
        assert np.array_equal(out[0], R.count_nonfinite(a, None, off)), sp_
        assert np.array_equal(out[2], R.count_nonfinite(a, b, off)), sp_
        assert np.array_equal(bits(out[1]), bits(np.zeros(len(part)))), sp_  # huge and tiny values are finite
        assert out[0].sum() == len(spots) and out[2].sum() == len(spots) + len(spots[::2]) + 2


def test_seg_member_alone_in_company_and_elsewhere(hipdev):
    """the partition of a member depends on its own size alone: its sums are bitwise the same when it is the whole
    batch, when it follows 300 of 600 tiny members, and when it comes first"""
    rng = np.random.default_rng(7)
    big = (8193, [(NN, 4097), (SOC, 4000)])
    tiny = R.tiny_members(600)
    ax, bx = R.f32_exact(rng, 8193), R.cancelling(rng, 8193)
    az, bz = R.f32_exact(rng, 8097), R.cancelling(rng, 8097)
    res = []
    for where in (None, 300, 0):
        members = [big] if where is None else tiny[:where] + [big] + tiny[where:]
        part = R.assemble(members)
        pl = hipdev.BatchPlanDebug(*part)
        k = 0 if where is None else where
        xo, zo = R.offsets(part[0]), R.offsets(part[1])
        vec = {}
        for nm, v, off, ln in (("ax", ax, xo, pl.n), ("bx", bx, xo, pl.n), ("az", az, zo, pl.m), ("bz", bz, zo, pl.m)):
            full = R.f32_exact(np.random.default_rng(99), ln)
            full[off[k]:off[k + 1]] = v
            vec[nm] = full
        specs = [(kind, sp_, 2 * kind + sp_, vec["a" + c], vec["b" + c]) for kind in (0, 1, 2)
                 for sp_, c in ((0, "x"), (1, "z"))]
        out = pl.seg_reduce(specs, 6)
        assert np.array_equal(bits(pl.seg_reduce(specs, 6)), bits(out))
        res.append(out[:, k].copy())
    assert np.all(res[0] != 0.0)
    assert np.array_equal(bits(res[0]), bits(res[1])) and np.array_equal(bits(res[0]), bits(res[2])), res


# ---- cone minima: Nonnegative rows ------------------------------------------------------------------------------------
WALK = [0, 255, 256, 4095, 4096, 8999]


def part_walk():
    return R.part_nn([9000] * 6 + [1, 4096, 0, 3])


def test_nn_minimum_at_every_stride_and_item_boundary(hipdev):
    """six Nonnegative cones of 9000 rows (three items each) whose minimum sits at row 0, 255, 256, 4095, 4096 and 8999:
    step lengths, minimal margins and the interior check are minima, so they are bitwise those of numpy"""
    pl, (n_part, m_part, cones) = plan_of(hipdev, "walk", part_walk)
    rng = np.random.default_rng(3)
    m, off = pl.m, R.offsets(m_part)
    z, s = rng.uniform(1.0, 2.0, m), rng.uniform(1.0, 2.0, m)
    dz, ds = rng.uniform(-1.0, 1.0, m), rng.uniform(-1.0, 1.0, m)
    dz[rng.integers(0, m, 2000)] = 0.0  # no bound from a zero direction, of either sign
    dz[rng.integers(0, m, 2000)] = -0.0
    ds[rng.integers(0, m, 2000)] = -0.0
    amax = np.full(pl.nprob, 100.0) + np.arange(pl.nprob)
    zm, sm = z.copy(), s.copy()
    for j, p in enumerate(WALK):
        i = off[j] + p
        if j % 2 == 0:
            dz[i], zm[i] = -64.0, -3.0 - j  # the smallest ratio of the member (1/64 .. 1/32), its smallest margin
        else:
            ds[i], sm[i] = -64.0, -3.0 - j
    dz[off[6]], ds[off[6]] = -1.0 / 1024, 0.0  # the one-row member: its ratio is above amax, the result is amax[k]
    dz[off[9]:off[10]], ds[off[9]:off[10]] = [0.0, -0.0, 0.5], [-0.0, 0.0, 2.0]  # nothing bounds the step: amax[k]
    want = R.nn_step(z, dz, s, ds, amax, m_part, cones)
    assert want[6] == amax[6] and want[9] == amax[9] and want[8] == amax[8] and np.all(want[:6] < 1.0 / 16)
    got, gsum = pl.cone_minima(pl.CONE_STEP, z, sv=s, dz=dz, ds=ds, amax=amax)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert np.array_equal(bits(gsum), bits(np.zeros(pl.nprob)))
    # the pair of the other side: the same ratios with (z, dz) and (s, ds) exchanged
    got2, _ = pl.cone_minima(pl.CONE_STEP, s, sv=z, dz=ds, ds=dz, amax=amax, want_sum=False)
    assert np.array_equal(bits(got2), bits(want))
    # margins of z: the minimum bitwise, the sum of the positive parts within the summation bound; member 8 is empty
    seg = lambda v, k: v[off[k]:off[k + 1]]  # noqa: E731
    for v in (zm, sm):
        mn, sm_ = pl.cone_minima(pl.CONE_MARGINS, v)
        wmin = np.array([seg(v, k).min() if m_part[k] else R.DBL_MAX for k in range(pl.nprob)])
        assert np.array_equal(bits(mn), bits(wmin)), (mn, wmin)
        pos = [np.maximum(seg(v, k), 0.0) for k in range(pl.nprob)]
        exact = np.array([math.fsum(p) for p in pos])
        assert np.all(np.abs(sm_ - exact) <= R.sum_bound(m_part, exact)), (sm_, exact)
        assert sm_[8] == 0.0 and np.all(sm_[:8] > 0.0)
    mn, _ = pl.cone_minima(pl.CONE_INTERIOR, zm, sv=sm, want_sum=False)
    wmin = np.array([min(seg(zm, k).min(), seg(sm, k).min()) if m_part[k] else R.DBL_MAX for k in range(pl.nprob)])
    assert np.array_equal(bits(mn), bits(wmin))
    assert [int(np.argmin(np.minimum(seg(zm, j), seg(sm, j)))) for j in range(6)] == WALK


def test_members_without_cone_rows(hipdev):
    """no Nonnegative or second-order row: the step length is amax[k], the margins DBL_MAX with sum 0 -- in a batch
    without any item (k_cone_items is not launched) and beside members that have items"""
    amax3 = np.array([0.5, 0.99, 1e-3])
    pl = hipdev.BatchPlanDebug([2, 0, 1], [3, 0, 4097], [(ZERO, 3), (ZERO, 4097)])
    assert pl.nitems == 0
    v = np.random.default_rng(1).standard_normal(pl.m)
    for op, wmin in ((pl.CONE_STEP, amax3), (pl.CONE_MARGINS, np.full(3, R.DBL_MAX)),
                     (pl.CONE_INTERIOR, np.full(3, R.DBL_MAX))):
        mn, sm = pl.cone_minima(op, v, sv=v, dz=-np.abs(v), ds=-np.abs(v), amax=amax3)
        assert np.array_equal(bits(mn), bits(wmin)) and np.array_equal(bits(sm), bits(np.zeros(3))), op
    pl, (n_part, m_part, cones) = plan_of(hipdev, "cones", R.part_cones)
    none = [k for k in range(pl.nprob) if not np.any(R.row_types(m_part, cones)[R.members_of(m_part) == k])]
    assert none == [1, 5, 6]
    v = np.abs(np.random.default_rng(2).standard_normal(pl.m)) + 0.5
    v[R.row_types(m_part, cones) == R.ROW_SOC_HEAD] += 200.0  # inside the second-order cones
    amax = 0.25 + np.arange(pl.nprob) / 64.0
    mn, sm = pl.cone_minima(pl.CONE_STEP, v, sv=v, dz=-v * 1e-6, ds=-v * 1e-6, amax=amax)
    assert np.array_equal(bits(mn), bits(amax))  # (every ratio is 1e6)
    for op in (pl.CONE_MARGINS, pl.CONE_INTERIOR):
        mn, sm = pl.cone_minima(op, v, sv=v)
        assert np.all(mn[none] == R.DBL_MAX) and np.all(sm[none] == 0.0)
        assert np.all(np.delete(mn, none) < 1e3)


def scaled_norm(t):
    """block_norm_tail's formula; a tail of at most two entries adds up the same in any order"""
    t = np.abs(np.asarray(t, float))
    amax = float(t.max()) if t.size else 0.0
    if amax == 0.0:
        return 0.0
    assert t.size <= 2
    return amax * math.sqrt(float(np.sum((t / amax) * (t / amax))))


def tiny_reference(m_part, cones, z, dz, s, ds, amax):
    """step, min margin of z, interior minimum per member for cones of at most 3 rows, as the kernels compute them"""
    zmem = R.members_of(m_part)
    step = R.nn_step(z, dz, s, ds, amax, m_part, cones)
    marg, inter = np.full(len(m_part), R.DBL_MAX), np.full(len(m_part), R.DBL_MAX)
    for tag, r0, r1 in R.cone_ranges(cones):
        k = zmem[r0]
        if tag == NN:
            marg[k] = min(marg[k], z[r0:r1].min())
            inter[k] = min(inter[k], z[r0:r1].min(), s[r0:r1].min())
        elif tag == SOC:
            zn, sn = scaled_norm(z[r0 + 1:r1]), scaled_norm(s[r0 + 1:r1])
            marg[k] = min(marg[k], z[r0] - zn)
            inter[k] = min(inter[k], z[r0] - zn, s[r0] - sn)
            for x, y, xn in ((z, dz, zn), (s, ds, sn)):
                dot = float(np.sum(x[r0 + 1:r1] * y[r0 + 1:r1]))
                step[k] = min(step[k], R.soc_step_roots(x[r0], y[r0], xn, scaled_norm(y[r0 + 1:r1]), dot, amax[k]))
    return step, marg, inter


@pytest.mark.parametrize("nprob", [257, 600])
def test_cone_minima_of_many_members(hipdev, nprob):
    """one thread per member in k_cone_final: a second workgroup from 257 members, a third at 600, every member with
    its own amax[k]"""
    pl, (n_part, m_part, cones) = plan_of(hipdev, "tiny%d" % nprob, lambda: R.part_tiny(nprob))
    rng = np.random.default_rng(nprob)
    m = pl.m
    rt = R.row_types(m_part, cones)
    z, s = rng.uniform(0.5, 2.0, m), rng.uniform(0.5, 2.0, m)
    head = rt == R.ROW_SOC_HEAD
    z[head], s[head] = z[head] + 3.0, s[head] + 3.0  # inside the second-order cones
    dz, ds = rng.standard_normal(m), rng.standard_normal(m)
    amax = 0.5 + np.arange(nprob) / 512.0
    step, marg, inter = tiny_reference(m_part, cones, z, dz, s, ds, amax)
    got, _ = pl.cone_minima(pl.CONE_STEP, z, sv=s, dz=dz, ds=ds, amax=amax, want_sum=False)
    assert np.array_equal(bits(got), bits(step)), np.nonzero(got != step)
    assert np.sum(step < amax) > nprob // 8 and np.sum(step == amax) > nprob // 8 and len(set(got.tolist())) > nprob // 2
    zneg = np.where(rng.uniform(size=m) < 0.2, -z, z)  # negative margins too
    step, marg, inter = tiny_reference(m_part, cones, zneg, dz, s, ds, amax)
    mn, sm = pl.cone_minima(pl.CONE_MARGINS, zneg)
    assert np.array_equal(bits(mn), bits(marg))
    # the sum of the positive margins: each term as the kernel forms it, added up exactly, within the summation bound
    zmem, terms = R.members_of(m_part), [[] for _ in range(nprob)]
    for tag, r0, r1 in R.cone_ranges(cones):
        if tag == NN:
            terms[zmem[r0]] += list(np.maximum(zneg[r0:r1], 0.0))
        elif tag == SOC:
            terms[zmem[r0]].append(max(0.0, zneg[r0] - scaled_norm(zneg[r0 + 1:r1])))
    exact = np.array([math.fsum(t) for t in terms])
    assert np.all(np.abs(sm - exact) <= R.sum_bound([len(t) for t in terms], exact))
    mn, _ = pl.cone_minima(pl.CONE_INTERIOR, zneg, sv=s, want_sum=False)
    assert np.array_equal(bits(mn), bits(inter))


# ---- cone minima: second-order cones ----------------------------------------------------------------------------------
def test_soc_margins_against_mpmath(hipdev):
    """x0 - ||x1|| at every dim around the 256-lane stride, for plain entries, entries of 1e200 (a plain sum of squares
    overflows), of 1e-200 (it underflows to 0) and both mixed; each cone inside, outside or near the boundary"""
    dims = R.SOC_DIMS * 4
    pl, (n_part, m_part, cones) = plan_of(hipdev, "socs4", lambda: R.part_socs(dims))
    rng = np.random.default_rng(11)
    off = R.offsets(m_part)

    def draw():
        v = rng.standard_normal(pl.m)
        for k, dim in enumerate(dims):
            t = v[off[k] + 1:off[k + 1]]
            kind = k // len(R.SOC_DIMS)
            if kind == 1:
                t *= 1e200
            elif kind == 2:
                t *= 1e-200
            elif kind == 3:
                t *= np.where(rng.uniform(size=dim - 1) < 0.5, 1e200, 1e-200)
                t[0] = 1e200  # (at least one large entry)
            v[off[k]] = float(np.max(np.abs(t))) * math.sqrt(dim) * rng.choice([0.01, 0.7, 1.0, 1.5])
        return v
    z, s = draw(), draw()
    ref = [[R.soc_margin_mp(v[off[k]:off[k + 1]]) for k in range(pl.nprob)] for v in (z, s)]
    mz, sz = np.array([r[0] for r in ref[0]]), np.array([r[1] for r in ref[0]])
    ms, ss = np.array([r[0] for r in ref[1]]), np.array([r[1] for r in ref[1]])
    assert np.all(np.isfinite(mz)) and np.any(mz < 0) and np.any(mz > 0)
    tz, ts = R.soc_margin_tol(np.array(dims), sz), R.soc_margin_tol(np.array(dims), ss)
    mn, sm = pl.cone_minima(pl.CONE_MARGINS, z)
    print("margins: max err / bound %.3g" % float(np.max(np.abs(mn - mz) / tz)))
    assert np.all(np.abs(mn - mz) <= tz), (mn, mz, tz)
    assert np.all(np.abs(sm - np.maximum(mz, 0.0)) <= tz)
    mn, _ = pl.cone_minima(pl.CONE_INTERIOR, z, sv=s, want_sum=False)
    assert np.all(np.abs(mn - np.minimum(mz, ms)) <= np.maximum(tz, ts)), (mn, mz, ms)


# socone.rs:421-495 branch by branch on small integers: the scaled norms (tails with one non-zero entry, or multiples of
# (3, 4), (1, 2, 2), (2, -1, 2) whose squares over the largest add up to 1.5625 or 2.25), the discriminant's root and
# both quotients are exact, so the result is the exact root.  (x, y, the step of the pair from amax = 16)
BRANCH_CASES = [
    ((7, 0), (10, -3), 16.0),              # a > 0 and b > 0: no positive root
    ((2, 1), (1, 1), 16.0),                # a == 0
    ((2, 1), (-1, 1), 2.0),                # a == 0, the linear cap -x0/y0 binds
    ((1, 1), (-2, 1), 0.5),                # c == 0, a >= 0: the cap binds
    ((0, 4), (12, 0), 16.0),               # c clamped to 0 (x outside), a >= 0
    ((1, 1), (1, 2), 0.0),                 # c == 0, a < 0
    ((10, 4), (-4, 0), 1.5),               # two positive roots, b < 0
    ((12, 0), (-3, 0), 4.0),               # a double root that equals the cap
    ((3, 0), (-1, 2), 1.0),                # b < 0, the negative root discarded
    ((3, 0), (1, 2), 3.0),                 # b >= 0, the negative root discarded
    ((11, 4), (0, 4), 1.75), ((11, 4), (-1, -3), 3.75),
    ((7, 0, 2), (9, 3, 4), 16.0), ((-1, 3, 4), (-2, 0, 2), 16.0), ((2, 0, 2), (-2, 0, 2), 1.0),
    ((4, 8, 6), (-4, 0, 2), 1.0), ((-2, 8, 6), (8, 6, -8), 0.0), ((11, 0, 2), (-8, 0, 0), 1.125),
    ((15, 0, 0), (-5, 6, 8), 1.0), ((9, 0, 0), (-4, -4, 3), 1.0), ((7, 0, 0), (3, -4, 3), 3.5), ((5, 0, 0), (-2, 0, 0), 2.5),
    ((4, -4, -2, 4), (11, 2, 4, 4), 16.0), ((7, 1, 2, 2), (6, -4, -2, 4), 16.0), ((12, -4, -2, 4), (-6, -4, -2, 4), 2.0),
    ((1, 0, 3, 4), (10, 1, 2, 2), 16.0), ((-2, -4, -2, 4), (-4, -4, -2, 4), 0.0), ((10, 1, 2, 2), (-5, 1, 2, 2), 0.875),
    ((9, 2, -1, 2), (-2, -4, -2, 4), 1.0), ((6, 0, 0, 0), (0, 1, 2, 2), 2.0), ((10, 0, 0, 0), (-8, 0, 0, 0), 1.25)]
# d < 0 cannot happen in exact arithmetic (for x in the cone, (x0 y0 - x1.y1)^2 >= (x0^2 - |x1|^2)(y0^2 - |y1|^2)):
# rounding alone reaches the branch, with y = -k x.  At dim 2 the norms and the dot are single operations, so the
# kernel's arithmetic is the restatement's and the comparison stays bitwise
ROUNDED_CASES = [(("0x1.6891b33292392p+0", "-0x1.2720a50e942c2p+0"), ("-0x1.e3a200981566bp-1", "0x1.8bdb100f8381ap-1")),
                 (("0x1.ffca01812618cp+0", "0x1.18bb265720edbp-1"), ("-0x1.51fb5acca6a3dp+1", "-0x1.72c91aa86513ap-1")),
                 (("0x1.457dda33e74c8p+0", "0x1.bcdd209e53290p-1"), ("-0x1.d7cce9524bf5fp-1", "-0x1.426a4e782d2e0p-1"))]


def _branch(x, y, amax):
    """(which exit of soc_step_roots, its result) from exact integer norms"""
    x1n, y1n = math.isqrt(sum(v * v for v in x[1:])), math.isqrt(sum(v * v for v in y[1:]))
    assert x1n ** 2 == sum(v * v for v in x[1:]) and y1n ** 2 == sum(v * v for v in y[1:])
    dot = sum(u * v for u, v in zip(x[1:], y[1:]))
    a, b = (y[0] - y1n) * (y[0] + y1n), 2 * (x[0] * y[0] - dot)
    c = max(0, (x[0] - x1n) * (x[0] + x1n))
    d = b * b - 4 * a * c
    assert d >= 0
    exit_ = ("none" if a > 0 and b > 0 else "a0" if a == 0 else ("c0+" if a >= 0 else "c0-") if c == 0 else
             "roots b%s" % (">=0" if b >= 0 else "<0"))
    if exit_.startswith("roots"):
        assert math.isqrt(d) ** 2 == d
    return exit_, R.soc_step_roots(float(x[0]), float(y[0]), float(x1n), float(y1n), float(dot), amax)


def test_soc_step_every_branch_on_exact_data(hipdev):
    exits = set()
    members = []  # (z, dz, s, ds, amax, want)
    for x, y, want in BRANCH_CASES:
        exit_, r = _branch(x, y, 16.0)
        exits.add(exit_)
        assert r == want, (x, y, r, want)
        unit = (1,) + (0,) * (len(x) - 1)  # s = e with ds = 0 bounds nothing (a == 0): the pair under test decides
        zero = (0,) * len(x)
        members.append((x, y, unit, zero, 16.0, want))
        members.append((unit, zero, x, y, 16.0, want))
    assert exits == {"none", "a0", "c0+", "c0-", "roots b>=0", "roots b<0"}
    # amax[k] below the root; both pairs bounded, the smaller one wins
    members.append(((10, 4), (-4, 0), (1, 0), (0, 0), 0.25, 0.25))
    members.append(((10, 4), (-4, 0), (3, 0), (-1, 2), 16.0, 1.0))
    members.append(((3, 0, 0), (1, 2, 0), (11, 0, 2), (-8, 0, 0), 16.0, 1.125))
    for (x, y) in ROUNDED_CASES:
        x, y = [float.fromhex(v) for v in x], [float.fromhex(v) for v in y]
        a = (y[0] - abs(y[1])) * (y[0] + abs(y[1]))
        b, c = 2.0 * (x[0] * y[0] - x[1] * y[1]), (x[0] - abs(x[1])) * (x[0] + abs(x[1]))
        assert b * b - 4.0 * a * c < 0.0 and not (a > 0.0 and b > 0.0)
        want = R.soc_step_roots(x[0], y[0], abs(x[1]), abs(y[1]), x[1] * y[1], 16.0)
        members.append((x, y, (1, 0), (0, 0), 16.0, want))
        members.append(((1, 0), (0, 0), x, y, 16.0, want))
    dims = [len(mb[0]) for mb in members]
    pl = hipdev.BatchPlanDebug(*R.part_socs(dims))
    cat = lambda j: np.concatenate([np.asarray(mb[j], float) for mb in members])  # noqa: E731
    got, _ = pl.cone_minima(pl.CONE_STEP, cat(0), dz=cat(1), sv=cat(2), ds=cat(3), amax=np.array([mb[4] for mb in members]),
                            want_sum=False)
    want = np.array([mb[5] for mb in members])
    assert np.array_equal(bits(got), bits(want)), [(members[i], got[i]) for i in np.nonzero(got != want)[0]]


# The closed form is not exactly rounded.  E_SEQ: the worst relative error of the sequential float64 restatement
# (batch_pass_ref.soc_step_seq) against the mpmath solution of the same quadratic on the 48 cases of
# soc_step_cases(seed 2024), measured on the CPU: 1.70e-15 (at dim 513; 1.1e-15 at dim 257, below 6e-16 at the other
# dims).  The test measures it again and refuses a larger one.  The kernel may differ from the restatement by its
# 256-lane tree against the sequential order and by its scaled norm: it is allowed 16 * max(E_SEQ, dim * 2^-53)
# relative, which is 2.7e-14 up to dim 15, 4.5e-13 at dim 255, 9.1e-13 at dim 513 and 8.9e-12 at dim 5000.
E_SEQ = 1.7e-15
STEP_CASES_PER_DIM = 6


@functools.lru_cache(maxsize=None)
def step_cases():
    rng = np.random.default_rng(2024)
    out = []
    for dim in R.SOC_DIMS:
        for (z, dz, s, ds) in R.soc_step_cases(rng, dim, STEP_CASES_PER_DIM):
            amax = 1e3  # (never binding: the cases compare roots)
            (rz, cz), (rs, cs) = R.soc_step_mp(z, dz, amax), R.soc_step_mp(s, ds, amax)
            seq = min(R.soc_step_seq(z, dz, amax), R.soc_step_seq(s, ds, amax))
            out.append(dict(dim=dim, v=(z, dz, s, ds), amax=amax, exact=min(rz, rs), seq=seq, cond=min(cz, cs)))
    return out


def test_soc_step_against_mpmath(hipdev):
    cases = step_cases()
    assert len(cases) == len(R.SOC_DIMS) * STEP_CASES_PER_DIM
    assert all(c["cond"] >= 0.05 for c in cases)  # x0^2 - ||x1||^2 at or above 5% of x0^2: a well-conditioned reference
    exact, seq = np.array([c["exact"] for c in cases]), np.array([c["seq"] for c in cases])
    dims = np.array([c["dim"] for c in cases])
    assert np.sum(exact < 1e3) >= len(cases) // 2  # most cases are decided by a root, not by amax
    e_seq = float(np.max(np.abs(seq - exact) / exact))
    print("E of the sequential restatement: %.3g" % e_seq)
    assert e_seq <= E_SEQ
    pl, _ = plan_of(hipdev, "socstep", lambda: R.part_socs(list(dims)))
    cat = lambda j: np.concatenate([c["v"][j] for c in cases])  # noqa: E731
    got, _ = pl.cone_minima(pl.CONE_STEP, cat(0), dz=cat(1), sv=cat(2), ds=cat(3), amax=np.array([c["amax"] for c in cases]),
                            want_sum=False)
    rel = np.abs(got - exact) / exact
    tol = 16.0 * np.maximum(E_SEQ, dims * R.EPS)
    print("kernel: max relative error %.3g, max error / bound %.3g" % (float(rel.max()), float(np.max(rel / tol))))
    assert np.all(rel <= tol), (dims[rel > tol], rel[rel > tol])


# ---- the element-wise passes ------------------------------------------------------------------------------------------
def elem_setup(hip, name="cones", make=R.part_cones, seed=5):
    pl, (n_part, m_part, cones) = plan_of(hip, name, make)
    rng = np.random.default_rng(seed)
    xmem, zmem, rt = R.members_of(n_part), R.members_of(m_part), R.row_types(m_part, cones)
    return pl, rng, xmem, zmem, rt


def mixed_mask(rng, nprob):
    mask = (rng.uniform(size=nprob) < 0.5).astype(np.int32)
    mask[:4] = [1, 0, 0, 1]
    return mask * np.where(np.arange(nprob) % 3 == 0, 5, 1).astype(np.int32)  # any non-zero value selects


@pytest.mark.parametrize("sp_", [0, 1], ids=["x", "z"])
def test_blin_scalars_masks_and_aliases(hipdev, sp_):
    pl, rng, xmem, zmem, _ = elem_setup(hipdev)
    mem = zmem if sp_ else xmem
    ln, k = len(mem), pl.nprob
    x, y, w0 = rng.standard_normal(ln), rng.standard_normal(ln), rng.standard_normal(ln)
    sa, sb = rng.standard_normal(k), rng.standard_normal(k)
    ca, cb = 0.7, -1.3
    for use_sa in (True, False):
        for use_sb in (True, False, None):  # None: y is NULL
            a_, b_ = (sa if use_sa else None), (sb if use_sb else None)
            y_ = None if use_sb is None else y
            got = pl.blin(w0.copy(), x, y_, sa=a_, sb=b_, ca=ca, cb=cb, space=sp_)
            want = R.blin_ref(w0, x, y_, a_, b_, ca, cb, mem, None, 0)
            assert np.array_equal(bits(got), bits(want)), (use_sa, use_sb)
    # a mixed mask; NaN planted where the mask is off: in x it must stay out in every mode, in y it comes through under
    # MASK_Y alone, in w it stays under MASK_KEEP alone
    mask = mixed_mask(rng, k)
    off = mask[mem] == 0
    assert off.any() and (~off).any()
    xn, yn, wn = x.copy(), y.copy(), w0.copy()
    xn[off], yn[off], wn[off] = np.nan, np.nan, np.nan
    for mode in (pl.MASK_ZERO, pl.MASK_Y, pl.MASK_KEEP):
        for y_, w_ in ((y, w0), (yn, w0), (y, wn)):
            got = pl.blin(w_.copy(), xn, y_, sa=sa, sb=None, ca=ca, cb=cb, space=sp_, mask=mask, mask_mode=mode)
            want = R.blin_ref(w_, xn, y_, sa, None, ca, cb, mem, mask, mode)
            assert np.array_equal(bits(got), bits(want)), mode
            assert np.all(np.isfinite(got[~off]))
            nan_in = (mode == pl.MASK_Y and y_ is yn) or (mode == pl.MASK_KEEP and w_ is wn)
            assert np.all(np.isnan(got[off])) if nan_in else np.all(np.isfinite(got[off])), (mode, nan_in)
        if mode != pl.MASK_Y:  # y NULL with a mask
            got = pl.blin(w0.copy(), xn, None, sa=sa, space=sp_, mask=mask, mask_mode=mode)
            assert np.array_equal(bits(got), bits(R.blin_ref(w0, xn, None, sa, None, ca, cb, mem, mask, mode)))
    # w aliasing x, and w aliasing y (with a mask under MASK_Y: the entries that are off keep y = w)
    w = x.copy()
    assert np.array_equal(bits(pl.blin(w, w, y, sa=sa, sb=sb, space=sp_)), bits(R.blin_ref(x, x, y, sa, sb, 0, 0, mem, None, 0)))
    w = y.copy()
    got = pl.blin(w, x, w, sa=None, sb=sb, ca=ca, space=sp_, mask=mask, mask_mode=pl.MASK_Y)
    assert np.array_equal(bits(got), bits(R.blin_ref(y, x, y, None, sb, ca, 0, mem, mask, 1)))


def test_bresid_bunscale_bitwise(hipdev):
    pl, rng, xmem, zmem, _ = elem_setup(hipdev)
    n, m, k = pl.n, pl.m, pl.nprob
    v = lambda ln: rng.standard_normal(ln) * 10.0 ** rng.uniform(-3, 3, ln)  # noqa: E731
    rx_inf, Px, q, rz_inf, b, tau = v(n), v(n), v(n), v(m), v(m), v(k)
    rx, rz = pl.bresid(rx_inf, Px, q, rz_inf, b, tau)
    wx, wz = R.bresid_ref(rx_inf, Px, q, rz_inf, b, tau, xmem, zmem)
    assert np.array_equal(bits(rx), bits(wx)) and np.array_equal(bits(rz), bits(wz))
    x, d, z, e, s, einv, sx, sz = v(n), v(n), v(m), v(m), v(m), v(m), v(k), v(k)
    got = pl.bunscale(x, d, z, e, s, einv, sx, sz)
    want = R.bunscale_ref(x, d, z, e, s, einv, sx, sz, xmem, zmem)
    for g, w_ in zip(got, want):
        assert np.array_equal(bits(g), bits(w_))
    # s is scaled by sx, z by sz: with sz = 2 sx the two outputs of equal inputs differ by that factor exactly
    _, zo, so = pl.bunscale(x, d, z, e, z, e, sx, 2.0 * sx)
    assert np.array_equal(bits(zo), bits(2.0 * so))


def test_bunit_shift_and_reset(hipdev):
    pl, rng, xmem, zmem, rt = elem_setup(hipdev)
    m, k = pl.m, pl.nprob
    z, alpha = rng.standard_normal(m), rng.standard_normal(k)
    mask = mixed_mask(rng, k)
    for primal in (0, 1):
        for mk in (None, mask):
            zz = z.copy()
            if mk is not None:
                zz[mk[zmem] == 0] = np.nan  # members that are off are left alone, NaN and all
            got = pl.bunit_shift(zz, alpha, primal, mk)
            want = R.bunit_shift_ref(zz, alpha, primal, mk, zmem, rt)
            assert np.array_equal(bits(got), bits(want)), (primal, mk is None)
            tail = rt == R.ROW_SOC_TAIL
            assert tail.sum() > 5000 and np.array_equal(bits(got[tail]), bits(zz[tail]))  # SOC tails are untouched
            if mk is None:
                zero = rt == R.ROW_ZERO
                assert np.all(got[zero] == 0.0) if primal else np.array_equal(got[zero], z[zero])
    x, s = rng.standard_normal(pl.n), rng.standard_normal(m)
    x[mask[xmem] == 0], s[mask[zmem] == 0] = np.nan, np.nan
    got = pl.bunit_reset(x, s, z, mask)
    want = R.bunit_reset_ref(x, s, z, mask, xmem, zmem, rt)
    for g, w_ in zip(got, want):
        assert np.array_equal(bits(g), bits(w_))
    on = mask[zmem] != 0
    assert np.all(np.isnan(got[1][~on])) and np.all(got[1][on & (rt == R.ROW_SOC_HEAD)] == 1.0)
    assert np.all(got[2][on & (rt == R.ROW_SOC_TAIL)] == 0.0) and np.all(got[0][mask[xmem] != 0] == 0.0)


def test_grid_stride_above_one_trip(hipdev):
    """n + 2 m = 538006 entries against the 2048 x 256 threads of the largest grid: the loops' second trip"""
    pl, rng, xmem, zmem, rt = elem_setup(hipdev, "large", R.part_large)
    n, m, k = pl.n, pl.m, pl.nprob
    assert n + 2 * m > 2048 * 256
    v = lambda ln: rng.standard_normal(ln)  # noqa: E731
    x, d, z, e, s, einv, sx, sz = v(n), v(n), v(m), v(m), v(m), v(m), v(k), v(k)
    for g, w_ in zip(pl.bunscale(x, d, z, e, s, einv, sx, sz), R.bunscale_ref(x, d, z, e, s, einv, sx, sz, xmem, zmem)):
        assert np.array_equal(bits(g), bits(w_))
    rx, rz = pl.bresid(x, d, x, z, e, sx)
    wx, wz = R.bresid_ref(x, d, x, z, e, sx, xmem, zmem)
    assert np.array_equal(bits(rx), bits(wx)) and np.array_equal(bits(rz), bits(wz))
    flag = np.array([1, 0, 1], dtype=np.int32)
    for g, w_ in zip(pl.bunit_reset(x, s, z, flag), R.bunit_reset_ref(x, s, z, flag, xmem, zmem, rt)):
        assert np.array_equal(bits(g), bits(w_))
    assert np.array_equal(bits(pl.bunit_shift(z, sz, 1, flag)), bits(R.bunit_shift_ref(z, sz, 1, flag, zmem, rt)))
    got = pl.blin(s.copy(), z, e, sa=sx, sb=sz, space=1, mask=flag, mask_mode=pl.MASK_KEEP)
    assert np.array_equal(bits(got), bits(R.blin_ref(s, z, e, sx, sz, 0, 0, zmem, flag, 2)))


# ---- the Ruiz step of the stack ---------------------------------------------------------------------------------------
def test_ruiz_of_a_stack_matches_the_restatement(hipdev):
    """HipBatchSolver.equilibration(k) against the numpy restatement of tests/test_solver_gpu.py per member: column-norm
    means over two (n = 5000) and three (n = 9000) chunks, a second-order cone, q = 0 (bitwise: no cost scaling, no
    rectification), an empty P (mean 0: no cost scaling), zero columns, and 300 small members behind them
    (k_beq_cost_final's second workgroup)"""
    from tests.test_solver_gpu import random_problem, ruiz

    def member(hip, pr):
        n, m = pr["n"], pr["m"]
        return (hip.CscMatrix(n, n, *pr["P"]), pr["q"], hip.CscMatrix(m, n, *pr["A"]), pr["b"], pr["cones"])

    def rel(a, b):
        a, b = np.asarray(a, float), np.asarray(b, float)
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0
    q0 = random_problem(5000, 13, q_zero=True, cones_kind="nn")
    noP = random_problem(2000, 14, cones_kind="nn")
    noP["P"] = (np.zeros(noP["n"] + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    zcol = E.basic_qp()
    zcol = dict(zcol, n=3, P=(np.append(zcol["P"][0], zcol["P"][0][-1]), zcol["P"][1], zcol["P"][2]),
                A=(np.append(zcol["A"][0], zcol["A"][0][-1]), zcol["A"][1], zcol["A"][2]), q=list(zcol["q"]) + [0.5])
    prs = [random_problem(5000, 11, cones_kind="nn"), random_problem(9000, 12, cones_kind="nn"), E.basic_socp(), q0, noP,
           zcol] + [E.basic_qp()] * 300
    bs = hipdev.HipBatchSolver([member(hipdev, p) for p in prs])
    cache = {}
    for k, pr in enumerate(prs):
        d, e, c = bs.equilibration(k)
        if k < 6 or 6 not in cache:
            cache[min(k, 6)] = ruiz(pr)
        d0, e0, c0 = cache[min(k, 6)]
        if k == 3:
            assert c == 1.0 and c0 == 1.0
            assert np.array_equal(bits(d), bits(d0)) and np.array_equal(bits(e), bits(e0))
        else:
            assert rel(d, d0) <= 1e-13 and rel(e, e0) <= 1e-13 and rel(c, c0) <= 1e-13, (k, c, c0)
    assert bs.equilibration(4)[2] == 1.0 and bs.equilibration(0)[2] != 1.0 and bs.equilibration(1)[2] != 1.0
