"""The exponential, power and generalised power cone kernels (clarabel.rs_amd/csrc/cones.hip) on the MI355X through the
public HipKKTSolver API, against the references of tests/nonsym_ref.py (tests/test_nonsym_ref_host.py checks those on the
CPU), on both sides of every size at which a kernel changes its code path:

    exp / pow cones per handle
    1                    the smallest handle
    42 | 43              k_ns3_write_hs (cones.hip:588-590 `t = blockIdx.x * WG + threadIdx.x`, `c = t / 6, k = t - 6 * c`; grid
                         (6 n + 255) / 256, :2310): 6 n crosses 256, cone 42 has its entries 0..3 in workgroup 0 and 4, 5 in
                         workgroup 1
    255 | 256 | 257      the second workgroup of k_ns3_update_scaling (:469-470 `c = blockIdx.x * WG + threadIdx.x; if (c >=
                         v.ncones) return`), k_ns3_mul_hs (:595-596) and k_ns3_step_ops (:1703-1709 `live`, `out = OP == 3 ? sc :
                         0.0`; ns3_blocks :2124): one or two partials of step_length and compute_barrier; 255 idle threads
                         of the last workgroup enter block_max / block_sum (:1745-1751)
    GenPow (dim1, dim2), one 256-thread workgroup per cone
    (2, 0), (2, 1)       the smallest; no w part; the barrier's `norm_r > eps` or not (:1995)
    (64, 64) | (65, 65)  a second wave holds a non-trivial value in block_prod (:1814-1824 `t *= red[i]`), block_sum and
                         block_max (k_gpw_update_scaling :1845-1846, gpw_feasible :1907-1908, k_gpw_ops<0> :1949-1951, <4>
                         :1987-1993)
    (256, 256) | (257, 257)   the second trip of every `for (k = tid; k < a; k += WG)` loop (:1843-1867, 1881-1889, 1897-1905,
                         1915-1923, 1946-1956, 1984-2017, 2023)
    (200, 100)           n = a + b crosses 256 while neither part does: `k < a ? ... : ...` of k_gpw_ops<0> (:1953-1956) and the p
                         run of k_gpw_write_kkt (:1889 `k < a + b`)
    (3, 300), (300, 3), (257, 0)   one loop takes two trips while the other takes one; a finite barrier on two trips

Handles: n = 1, P = [1], A one dense column of ones, one handle per layout for the whole module.  (a) every family and
size alone; (b) one mixed handle, not sorted by size: 257 exp / pow cones in three runs, every GenPow size, Zero(3),
Nonnegative(300), SOC(4) and SOC(66) between them.  Exp and pow cones alternate, each pow cone with its own alpha; cone c
takes pool point c mod 7 of its kind (7 is coprime to 2, 6 and 256: cone c and cone c - 256 never share a point, nor do
two cones whose Hs entries meet at a workgroup edge).  Cones that share a point must agree bitwise; one cone per point
is compared with mpmath.  A cone's outputs in (a) and (b) must be bitwise equal.  There is no getter for the cones'
state; it is read through the operations: values() after update() is -Hs (strategy 1: -mu Hd; GenPow: the diagonal, the
columns -sqrt(mu) (q | r | p) and D), combined_ds_shift of zero steps is sigma_mu grad, of steps of relative size 0.05 the
third-order correction.  Before every case another pair is scaled with the other strategy and another mu.

Tolerances: nonsym_ref.tol(E, n, kappa) = 16 max(E, n 2^-53, kappa 2^-53) per cone; step_length and unit_initialization bit
for bit.  Every figure is printed before it is asserted (pytest -s), E beside the device's error.

Measured on one MI355X, largest E (device error) over all sizes and both strategies, per late set (delta, mu) = (1, 1) /
(1e-2, 1e-3) / (1e-4, 1e-6) / (1e-6, 1e-8):
    exp / pow  Hs                  2.5e-14 (2.5e-14) / 4.4e-13 (4.4e-13) / 3.3e-11 (3.3e-11) / 2.0e-9 (2.2e-9)
               sigma_mu grad       1.8e-16 (1.8e-16) / 2.5e-14 (1.3e-14) / 2.3e-12 (1.2e-12) / 2.2e-10 (1.1e-10)
               mul_Hs              2.9e-14 (2.9e-14) / 1.2e-12 (1.2e-12) / 6.1e-11 (6.1e-11) / 2.3e-8 (2.3e-8)
               third-order shift   1.7e-16 (1.7e-16) / 2.6e-14 (1.3e-14) / 1.2e-11 (1.2e-11) / 1.2e-9 (1.2e-9) at its last set,
                                   (1e-5, 1e-7): "inward 0", which stands for (1e-6, 1e-8) for this output alone
                                   (nonsym_ref.THIRD_ORDER_MOVED_FROM has the reason and the E that decided it)
               the other outputs at (1e-5, 1e-7): Hs 4.9e-10 (4.9e-10), sigma_mu grad 2.0e-11 (9.7e-12), mul_Hs 4.8e-10 (4.8e-10)
               central pairs (1, 1) / (1e-2, 1e-3): Hs 3.8e-16 (3.8e-16) / 5.1e-14 (3.4e-14); branch points: every output within
               9.6e-14 (9.6e-14); compute_barrier 1.4e-15 (3.5e-16)
    GenPow     -mu d1, -mu d2      1.5e-16 (1.5e-16) / 7.7e-14 (1.0e-13) / 1.9e-11 (2.3e-11) / 2.9e-9 (2.3e-9)
               -sqrt(mu) q         2.3e-16 (2.3e-16) / 8.2e-14 (1.2e-13) / 9.3e-12 (1.2e-11) / 1.4e-9 (1.1e-9)
               -sqrt(mu) r         0 (0: w = 0)      / 8.3e-14 (1.2e-13) / 9.3e-12 (1.2e-11) / 1.4e-9 (1.1e-9)
               -sqrt(mu) p         2.3e-16 (2.3e-16) / 1.6e-13 (2.4e-13) / 1.9e-11 (2.4e-11) / 2.9e-9 (2.3e-9)
               sigma_mu grad       1.4e-16 (1.4e-16) / 7.7e-14 (1.0e-13) / 1.9e-11 (2.3e-11) / 2.9e-9 (2.3e-9)
               mul_Hs              1.2e-16 (1.4e-16) / 3.0e-13 (4.7e-13) / 3.7e-11 (4.7e-11) / 5.8e-9 (4.5e-9)
               D = [-1, -1, +1] exactly; compute_barrier on the finite-barrier pairs 1.9e-15 (4.4e-16)
The exp / pow kernels gave the bits of oracle.Cones in most outputs (E and the device error coincide).  All 101 step-length
cases (5 of them on the mixed handle) returned the expected candidate bit for bit (1 - 2^-26, 0.8^4 (1 - 2^-26) = 0.40959999389648449, 0.0, and the
candidates 0.0038 .. 0.33 of the GenPow cases in which one element moves).  Every exp / pow and GenPow cone of the mixed
handle was bitwise equal to the cone in its own handle; values() and the SOC / nonnegative observations were bitwise
unchanged by the GenPow barrier call and by a further update_scaling.  The largest E, 2.3e-8, is under the cap 1e-7.

The largest share of a tolerance any device error reached is 0.67: mul_Hs of GenPow (300, 3) at (1e-2, 1e-3) (E 4.1e-15, device
4.7e-13, allowed 7.1e-13), and 0.67 again at (1e-4, 1e-6) (E 3.5e-12, device 4.7e-11, allowed 7.1e-11).  The device error there
is about 100 times the oracle's E, and the cause is not the conditioning of zeta alone.  phi is a product of 300 pow()
values (block_prod), each factor and each multiplication rounded, so phi's own relative error grows with n: 300 such
factors multiplied in double on the CPU were 2.5e-15 (median of 200 orders; sequential 3.3e-15, the workgroup's tree 2.9e-15;
4.5e-15 at most) from the 60-digit phi, where exp of the sum of the logarithms was 1.0e-16.  kappa = 398 multiplies that
error in everything divided by zeta: an n kappa effect, which the max() of tol cannot express (n 2^-53 and kappa 2^-53 are
alternatives there, not factors).  The case passes because 16 kappa 2^-53 = 7.1e-13 happens to cover about 12 u kappa, not
because the tolerance models it; with kappa taken as phi / zeta (half of nonsym_ref's componentwise condition number)
the same device error would stand at 1.3 of its tolerance.  The reference forms phi by the same product
(genpowcone.rs:366-369), and parity with it is the contract, so the kernel keeps the product; a sum of logarithms, as
gpw_feasible uses for its sign test, would remove the excess and change every GenPow output in the last digits.

Wrong kernels against these tests (the first three were built in a scratch copy and run; none is committed):
  * block_prod combining only red[0] (`return t` before the loop over red[1..]): phi loses the factors of waves 1..3.
    test_genpow_scaling fails at (65, 65), (256, 256), (257, 257), (200, 100) and (300, 3) for every late set and passes at (64,
    64), (2, 0), (2, 1), (3, 300): exactly the sizes whose dim1 reaches a second wave; test_genpow_barrier,
    test_genpow_copies_unit_initialization_and_step_length and test_every_cone_in_one_handle fail at the same sizes.  (257, 0)
    passes by the mathematics, not by a gap: without a w part zeta = phi, and grad, d1, p, q depend on phi / zeta = 1 only;
  * `k < a - 1` as the bound of the grad / d1 loop of k_gpw_update_scaling: grad, d1, p, q of element dim1 - 1 keep what the
    scramble's pair left.  All 80 cases of test_genpow_scaling fail (diag, q, p, grad, mul_hs), (2, 0) included;
  * the fallback branch of k_ns3_update_scaling writing mu_in Hd instead of mu Hd: the handles are scaled with mu_in = 1.7
    times the set's mu, so test_exp_pow_scaling[*-central 0-0] and [*-central 1-0] fail at every size, and [*-branch 3-0]
    from 42 cones on (power cones whose alpha is 0.1 or 0.9 take the fallback there), 17 cases in all;
  * argued only: `t >> 3` for `t / 6` in k_ns3_write_hs (tests/test_nonsym_ref_host.py::
    test_the_split_of_write_hs_falls_inside_a_cone): cones 33..42 of 43 are never written and keep the scramble's Hs, every
    other cone gets entries of its neighbours: test_exp_pow_scaling fails from 42 cones on;
  * NOT CAUGHT: `c > v.ncones` as the guard of k_ns3_update_scaling.  The one extra thread, c == ncones, exists in the
    handles of 1, 42, 43, 255 and 257 cones (256 has no idle thread).  It reads start[ncones], tag[ncones] and alpha[ncones]
    past their arrays and writes 18 doubles past `state`, which is an allocation of its own (kkt_cones.cpp `zeroed(E, ns3.state, ncones *
    18)`): nothing that a test here reads lies behind it, and the cones' own outputs stay right.  It is an out-of-bounds
    access, not a wrong value, and no test of this file fails for it.
"""
import functools

import mpmath as mp
import numpy as np
import pytest

from tests import nonsym_ref as R
from tests import soc_ref as S

pytestmark = pytest.mark.gpu

EXP, POW, GENPOW, SOC, NN, ZERO = R.EXP, R.POW, R.GENPOW, R.SOC, R.NN, R.ZERO
NS3_ALONE = 257


def mixed_cones():
    ns3 = R.ns3_specs(NS3_ALONE)
    g = {sz: R.gpw_spec(*sz) for sz in R.GPW_SIZES}
    return (ns3[:100] + [(ZERO, 3), g[(64, 64)], (NN, 300), g[(2, 0)], (SOC, 4)] + ns3[100:200]
            + [g[(257, 257)], g[(3, 300)], (SOC, 66), g[(2, 1)], g[(65, 65)]] + ns3[200:]
            + [g[(256, 256)], g[(200, 100)], (ZERO, 3), g[(300, 3)], g[(257, 0)]])


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


class Layout:
    """one HipKKTSolver over n = 1, P = [1], A = a dense column of ones, and where each cone's rows and K entries are"""

    def __init__(self, hip, cones):
        self.hip, self.cones = hip, list(cones)
        self.info, start, h, col = [], 0, 0, 0
        for c in self.cones:
            tag, d = c[0], c[1]
            d2 = c[2] if tag == GENPOW else 0
            numel = 3 if tag in (EXP, POW) else d + d2
            sparse = (tag == SOC and d > 4) or tag == GENPOW
            blen = 6 if tag in (EXP, POW) else d * (d + 1) // 2 if tag == SOC and not sparse else numel
            self.info.append(dict(tag=tag, d1=d, d2=d2, numel=numel, rows=slice(start, start + numel), hs=slice(h, h + blen),
                                  start=start, col=col if sparse else None))
            start, h = start + numel, h + blen
            col += 3 if tag == GENPOW else 2 if sparse else 0
        m = self.m = start
        P = hip.CscMatrix(1, 1, [0, 1], [0], [1.0])
        A = hip.CscMatrix(m, 1, [0, m], np.arange(m), np.ones(m))
        self.ks = hip.HipKKTSolver(P, A, self.cones, m, 1)
        assert h == self.ks.nHs and self.ks.N == 1 + m + col
        self.colptr = self.ks.kkt_matrix().colptr.astype(np.int64)
        self.map_hs = self.ks.maps()["Hsblocks"]
        for c in self.info:
            if c["col"] is not None:
                c["col"] += 1 + m
        self.ns3 = [k for k, c in enumerate(self.info) if c["tag"] in (EXP, POW)]
        self.gpw = [k for k, c in enumerate(self.info) if c["tag"] == GENPOW]

    def fill(self, per_cone, other=0.0):
        """an m-vector from per_cone(k, info) -> array or None (None: `other`)"""
        out = np.full(self.m, float(other))
        for k, c in enumerate(self.info):
            v = per_cone(k, c)
            if v is not None:
                out[c["rows"]] = v
        return out

    def scale(self, s, z, mu, strategy):
        assert self.ks.update_scaling(s, z, mu, strategy) and self.ks.update()
        return self.ks.values()

    def _run(self, call, outs):
        call()
        self.ks.synchronize()
        return [o.numpy() for o in outs]

    def mul_hs(self, x):
        D = self.hip.DeviceArray
        y, dx = D(self.m), D(x)
        return self._run(lambda: self.ks.mul_Hs_dev(y.ptr, dx.ptr), [y])[0]

    def affine_ds(self, s):
        D = self.hip.DeviceArray
        out, ds = D(self.m), D(s)
        return self._run(lambda: self.ks.affine_ds_dev(out.ptr, ds.ptr), [out])[0]

    def combined_ds_shift(self, dz, ds, sigma_mu):
        D = self.hip.DeviceArray
        sh, tz, ts = D(self.m), D(dz), D(ds)
        return self._run(lambda: self.ks.combined_ds_shift_dev(sh.ptr, tz.ptr, ts.ptr, sigma_mu), [sh, tz, ts])

    def ds_from_dz_offset(self, ds, z):
        D = self.hip.DeviceArray
        out, a, b = D(self.m), D(ds), D(z)
        return self._run(lambda: self.ks.ds_from_dz_offset_dev(out.ptr, a.ptr, b.ptr), [out])[0]

    def step_length(self, dz, ds, z, s, amax):
        a = [self.hip.DeviceArray(v) for v in (dz, ds, z, s)]
        return self.ks.step_length_dev(a[0].ptr, a[1].ptr, a[2].ptr, a[3].ptr, amax)

    def barrier(self, z, s, dz, ds, alpha):
        a = [self.hip.DeviceArray(v) for v in (z, s, dz, ds)]
        return self.ks.compute_barrier_dev(a[0].ptr, a[1].ptr, a[2].ptr, a[3].ptr, alpha)

    def unit_initialization(self):
        D = self.hip.DeviceArray
        z, s = D(np.full(self.m, 7.0)), D(np.full(self.m, 7.0))
        return self._run(lambda: self.ks.unit_initialization_dev(z.ptr, s.ptr), [z, s])

    def gpw_k(self, vals, k):
        c = self.info[k]
        return R.gpw_read_k(vals, self.colptr, 1 + c["start"], c["col"], c["d1"], c["d2"])


_LAYOUTS, _ALONE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def release_handles():
    """the handles and device results cached for the module are released with it, not at interpreter exit"""
    yield
    _LAYOUTS.clear()
    _ALONE.clear()


def layout(hip, key):
    """key: ("ns3", n), ("gpw", d1, d2) or "mixed" """
    if key not in _LAYOUTS:
        cones = mixed_cones() if key == "mixed" else R.ns3_specs(key[1]) if key[0] == "ns3" else [R.gpw_spec(key[1], key[2])]
        _LAYOUTS[key] = Layout(hip, cones)
    return _LAYOUTS[key]


class Checks:
    """prints every figure, collects the failures, asserts at the end"""

    def __init__(self, label):
        self.label, self.fails = label, []

    def __call__(self, name, err, E, allowed):
        ok = err <= allowed
        print("  NSYM|%s|%s|E %.2e|err %.2e|allowed %.2e|share %.3f%s" % (self.label, name, E, err, allowed, err / allowed, "" if ok else "  <-- FAIL"))
        if not ok:
            self.fails.append((name, err, allowed))

    def done(self):
        assert not self.fails, (self.label, self.fails)


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), (what, float(np.max(np.abs(a - b))) if a.shape == b.shape else "shape")


def scramble_of(set_name):
    return "late 0" if set_name != "late 0" else "branch 1"


# ---- exp / pow: inputs of a whole handle -----------------------------------------------------------------------------
def ns3_inputs(ncones, set_name, strategy):
    cases = [R.ns3_case(set_name, EXP if c % 2 == 0 else POW, c % R.POOL, strategy) for c in range(ncones)]
    cat = lambda name: np.concatenate([c[name] if name in c else c["pt"][name] for c in cases])  # noqa: E731
    return dict(cases=cases, s=cat("s"), z=cat("z"), x=cat("x"), step_z=cat("step_z"), step_s=cat("step_s"), mu_in=R.set_mu_in(set_name))


def ns3_observe(lay, inp, strategy, set_name, ns3_vectors):
    """scramble, scale, and every output of the exp / pow cones: dict name -> list (per exp / pow cone) of arrays.
    ns3_vectors(name) -> the m-vector of the handle for input `name`"""
    scr = scramble_of(set_name)
    lay.scale(ns3_vectors(scr, "s"), ns3_vectors(scr, "z"), R.set_mu_in(scr), 1 - strategy)
    vals = lay.scale(ns3_vectors(set_name, "s"), ns3_vectors(set_name, "z"), inp["mu_in"], strategy)
    zero = np.zeros(lay.m)
    grad = lay.combined_ds_shift(zero, zero, R.SIGMA_MU)[0]
    hx = lay.mul_hs(ns3_vectors(set_name, "x"))
    out = dict(Hs=[-vals[lay.map_hs[lay.info[k]["hs"]]] for k in lay.ns3], grad=[grad[lay.info[k]["rows"]] for k in lay.ns3],
               mul_hs=[hx[lay.info[k]["rows"]] for k in lay.ns3])
    if set_name not in R.THIRD_ORDER_MOVED_FROM:
        sh = lay.combined_ds_shift(ns3_vectors(set_name, "step_z"), ns3_vectors(set_name, "step_s"), R.SIGMA_MU)[0]
        out["shift"] = [sh[lay.info[k]["rows"]] for k in lay.ns3]
    return out, vals


def ns3_alone_vectors(n, strategy):
    def vec(set_name, name):
        return ns3_inputs(n, set_name, strategy)[name]
    return vec


def ns3_alone(hip, n, set_name, strategy):
    key = ("ns3", n, set_name, strategy)
    if key not in _ALONE:
        lay = layout(hip, ("ns3", n))
        _ALONE[key] = ns3_observe(lay, ns3_inputs(n, set_name, strategy), strategy, set_name, ns3_alone_vectors(n, strategy))[0]
    return _ALONE[key]


def check_ns3(obs, inp, label):
    """cones that share a pool point agree bitwise; the first cone of every point against mpmath"""
    ck = Checks(label)
    first = {}
    for c, case in enumerate(inp["cases"]):
        key = (c % 2, c % R.POOL)
        if key in first:
            for name in obs:
                same_bits(obs[name][c], obs[name][first[key]], "%s: cone %d against cone %d, %s" % (label, c, first[key], name))
            continue
        first[key] = c
        assert max(case["E"].values()) <= R.E_CAP and case["margin"] >= R.MARGIN and case["newton_margin"] >= R.NEWTON_MARGIN
        for name in obs:
            ck("%s|cone %d %s" % (name, c, case["branch"]), S.rel_vec(obs[name][c], case["refs"][name]), case["E"][name],
               R.tol(case["E"][name], 3, R.ns3_kappa_of(case, name)))
    ck.done()


@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("set_name", R.NS3_SETS)
@pytest.mark.parametrize("n", R.NS3_SIZES)
def test_exp_pow_scaling(hipdev, n, set_name, strategy):
    """k_ns3_update_scaling, k_ns3_write_hs, k_ns3_mul_hs, k_ns3_step_ops<1>: Hs from values() (strategy 1: mu_in Hd, so Hd
    itself), sigma_mu grad, mul_Hs and the third-order correction of every cone, for the late sets, the central pairs
    (the fallback Hs = mu Hd with mu = <s, z> / 3, NOT the mu passed in) and the branch points"""
    inp = ns3_inputs(n, set_name, strategy)
    want = "dual" if strategy == 1 else R.STRATEGY0_BRANCH.get(set_name.split()[0])
    assert want is None or all(c["branch"] == want for c in inp["cases"])
    check_ns3(ns3_alone(hipdev, n, set_name, strategy), inp, "exp/pow %d|%s|strategy %d" % (n, set_name, strategy))


@pytest.mark.parametrize("n", R.NS3_SIZES)
def test_exp_pow_copies_and_unit_initialization(hipdev, n):
    """affine_ds and ds_from_dz_offset are copies (expcone.rs:134-151), unit_initialization the constants of expcone.rs:88-94
    and (sqrt(1 + alpha), sqrt(2 - alpha), 0) of powcone.rs:79-87: all compared exactly"""
    lay = layout(hipdev, ("ns3", n))
    inp = ns3_inputs(n, "late 1", 0)
    same_bits(lay.affine_ds(inp["s"]), inp["s"], "affine_ds")
    same_bits(lay.ds_from_dz_offset(inp["step_s"], inp["z"]), inp["step_s"], "ds_from_dz_offset")
    want = np.concatenate([R.ns3_unit(c["pt"]["isexp"], c["pt"]["a"]) for c in inp["cases"]])
    uz, us = lay.unit_initialization()
    same_bits(uz, want, "unit z")
    same_bits(us, want, "unit s")


@pytest.mark.parametrize("case", R.STEP_CASES)
@pytest.mark.parametrize("set_name", R.STEP_SETS)
@pytest.mark.parametrize("n", R.NS3_SIZES)
def test_exp_pow_step_length(hipdev, n, set_name, case):
    """k_ns3_step_ops<3> and the host's minimum over the partials: bit for bit the candidate nonsym_ref decides exactly"""
    lay = layout(hipdev, ("ns3", n))
    dz, ds, z, s, amax, _ = R.ns3_step_case(n, set_name, case)
    want, margin = R.ns3_step_expected(n, set_name, case)
    assert margin >= R.STEP_MARGIN
    got = lay.step_length(dz, ds, z, s, amax)
    print("  NSYM-STEP|exp/pow %d|%s|%s|got %.17g|want %.17g|margin %.1e" % (n, set_name, case, got, want, margin))
    assert got == want


@pytest.mark.parametrize("alpha", R.BARRIER_ALPHAS)
@pytest.mark.parametrize("set_name", R.BARRIER_SETS)
@pytest.mark.parametrize("n", R.NS3_SIZES)
def test_exp_pow_barrier(hipdev, oracle, n, set_name, alpha):
    """k_ns3_step_ops<4> (wright_omega, pow_newton_raphson) and the sum over the partials against the sum of the cones'
    60-digit barriers, absolutely over max(1, |barrier|)"""
    lay = layout(hipdev, ("ns3", n))
    inp = ns3_inputs(n, set_name, 0)
    per = [R.ns3_barrier_case(set_name, EXP if c % 2 == 0 else POW, c % R.POOL, alpha) for c in range(n)]
    with mp.workdps(R.DPS):
        ref = mp.fsum(p[0] for p in per)
    assert np.isfinite(float(ref)) and min(float(p[2]) for p in per) >= R.MARGIN and min(float(p[3]) for p in per) >= R.NEWTON_MARGIN
    cones = oracle.Cones(R.ns3_specs(n))
    den = max(1.0, abs(float(ref)))
    E = float(abs(mp.mpf(cones.compute_barrier(inp["z"], inp["s"], inp["step_z"], inp["step_s"], alpha)) - ref)) / den
    assert E <= R.E_CAP
    lay.scale(inp["s"], inp["z"], inp["mu_in"], 0)
    got = lay.barrier(inp["z"], inp["s"], inp["step_z"], inp["step_s"], alpha)
    ck = Checks("exp/pow %d|%s" % (n, set_name))
    ck("barrier alpha %.1f" % alpha, float(abs(mp.mpf(got) - ref)) / den, E, R.tol(E, 3 * n, max(p[1] for p in per)))
    ck.done()


# ---- GenPow ----------------------------------------------------------------------------------------------------------
GPW_OUTPUTS = ("diag", "q", "r", "p", "D", "grad", "mul_hs")


def gpw_observe(lay, k, vals, grad, hx):
    out = lay.gpw_k(vals, k)
    rows = lay.info[k]["rows"]
    out["grad"], out["mul_hs"] = grad[rows], hx[rows]
    return out


def gpw_alone(hip, d1, d2, set_name, strategy):
    key = ("gpw", d1, d2, set_name, strategy)
    if key not in _ALONE:
        lay = layout(hip, ("gpw", d1, d2))
        c, scr = R.gpw_case(d1, d2, set_name), R.gpw_case(d1, d2, scramble_of(set_name) if set_name != "late 0" else "late 2")
        lay.scale(scr["pt"]["s"], scr["pt"]["z"], scr["mu_in"], 1 - strategy)
        vals = lay.scale(c["pt"]["s"], c["pt"]["z"], c["mu_in"], strategy)
        zero = np.zeros(lay.m)
        _ALONE[key] = gpw_observe(lay, 0, vals, lay.combined_ds_shift(zero, zero, R.SIGMA_MU)[0], lay.mul_hs(c["x"]))
    return _ALONE[key]


@pytest.mark.parametrize("strategy", [1, 0])
@pytest.mark.parametrize("set_name", R.GPW_SETS)
@pytest.mark.parametrize("d1,d2", R.GPW_SIZES)
def test_genpow_scaling(hipdev, d1, d2, set_name, strategy):
    """k_gpw_update_scaling, k_gpw_write_kkt, k_gpw_ops<0>, <2>: the K entries -mu d1, -mu d2, -sqrt(mu) (q | r | p) and D =
    [-1, -1, +1], sigma_mu grad and mul_Hs; the cone has no primal-dual scaling, so both strategies give the same bits"""
    c = R.gpw_case(d1, d2, set_name)
    assert max(c["E"].values()) <= R.E_CAP
    obs = gpw_alone(hipdev, d1, d2, set_name, strategy)
    ck = Checks("genpow (%d, %d)|%s|strategy %d" % (d1, d2, set_name, strategy))
    for name in GPW_OUTPUTS:
        assert len(obs[name]) == len(c["refs"][name])
        if len(obs[name]):
            ck(name, S.rel_vec(obs[name], c["refs"][name]), c["E"][name], R.tol(c["E"][name], d1 + d2, c["kappa"]))
    ck.done()
    assert np.array_equal(obs["D"], [-1.0, -1.0, 1.0])
    if strategy == 0:
        for name in GPW_OUTPUTS:
            same_bits(obs[name], gpw_alone(hipdev, d1, d2, set_name, 1)[name], "strategies differ in " + name)


@pytest.mark.parametrize("d1,d2", R.GPW_SIZES)
def test_genpow_copies_unit_initialization_and_step_length(hipdev, d1, d2):
    """k_gpw_ops<1>, <5> exactly; k_gpw_ops<3> bit for bit: a direction that stays feasible, one that backtracks, one that
    ends at 0, one where only element dim1 - 1 moves and one where only element dim1 + dim2 - 1 moves"""
    lay = layout(hipdev, ("gpw", d1, d2))
    c = R.gpw_case(d1, d2, R.GPW_STEP_SET)
    pt = c["pt"]
    lay.scale(pt["s"], pt["z"], c["mu_in"], 1)
    same_bits(lay.affine_ds(pt["s"]), pt["s"], "affine_ds")
    same_bits(lay.ds_from_dz_offset(c["x"], pt["z"]), c["x"], "ds_from_dz_offset")
    uz, us = lay.unit_initialization()
    same_bits(uz, R.gpw_unit(pt["alpha"], d2), "unit z")
    same_bits(us, R.gpw_unit(pt["alpha"], d2), "unit s")
    fails = []
    for case in R.GPW_STEP_CASES:
        if d2 == 0 and case == "last w leaves":
            continue
        dz, ds, z, s, amax = R.gpw_step_case(d1, d2, R.GPW_STEP_SET, case)
        want, margin = R.gpw_step_expected(d1, d2, R.GPW_STEP_SET, case)
        assert margin >= R.STEP_MARGIN
        got = lay.step_length(dz, ds, z, s, amax)
        print("  NSYM-STEP|genpow (%d, %d)|%s|%s|got %.17g|want %.17g|margin %.1e" % (d1, d2, R.GPW_STEP_SET, case, got, want, margin))
        if got != want:
            fails.append((case, got, want))
    assert not fails, fails


def gpw_barrier_alone(hip, d1, d2, alpha):
    key = ("gpw barrier", d1, d2, alpha)
    if key not in _ALONE:
        _, _, _, _, pt, dz, ds = R.gpw_barrier_case(d1, d2, alpha)
        lay = layout(hip, ("gpw", d1, d2))
        lay.scale(pt["s"], pt["z"], 1.0, 1)
        _ALONE[key] = lay.barrier(pt["z"], pt["s"], dz, ds, alpha)
    return _ALONE[key]


@pytest.mark.parametrize("alpha", R.BARRIER_ALPHAS)
@pytest.mark.parametrize("d1,d2", R.GPW_SIZES)
def test_genpow_barrier(hipdev, d1, d2, alpha):
    """k_gpw_ops<4>: block_prod, the scaled norm, the Newton iteration over the workgroup and both barrier halves, as the
    reference computes them (the w part of the primal gradient from the cone's r: genpowcone.rs:427-429), on a pair whose
    barrier is finite, absolutely over max(1, |barrier|)"""
    ref, kap, margin, newton, pt, dz, ds = R.gpw_barrier_case(d1, d2, alpha)
    assert np.isfinite(float(ref)) and margin >= R.MARGIN and newton >= R.NEWTON_MARGIN
    orc = R.GpwOracle(pt)
    assert orc.cones.update_scaling(pt["s"], pt["z"], 1.0, 1)
    den = max(1.0, abs(float(ref)))
    E = float(abs(mp.mpf(orc.cones.compute_barrier(pt["z"], pt["s"], dz, ds, alpha)) - ref)) / den
    assert E <= R.E_CAP
    got = gpw_barrier_alone(hipdev, d1, d2, alpha)
    ck = Checks("genpow (%d, %d)|barrier point" % (d1, d2))
    ck("barrier alpha %.1f" % alpha, float(abs(mp.mpf(got) - ref)) / den, E, R.tol(E, d1 + d2, kap))
    ck.done()


# ---- the mixed handle ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_symmetric_inputs():
    """s, z of the symmetric cones of the mixed handle: SOC late pairs of soc_ref, nonnegative rows uniform, Zero rows 1"""
    rng = np.random.default_rng(5)
    out = {}
    for k, c in enumerate(mixed_cones()):
        if c[0] == SOC:
            p = S.late_case(c[1], 1)
            out[k] = (p["s"], p["z"])
        elif c[0] == NN:
            out[k] = (rng.uniform(0.5, 2.0, c[1]), rng.uniform(0.5, 2.0, c[1]))
        elif c[0] == ZERO:
            out[k] = (np.ones(c[1]), np.ones(c[1]))
    return out


def mixed_gpw_set(set_name):
    """the set of the GenPow cones of the mixed handle while its exp / pow cones are on `set_name`"""
    return set_name if set_name in R.GPW_SETS else "late 1"


def mixed_vector(lay, set_name, name, strategy):
    """the m-vector of the mixed handle for input `name` of the set: exp / pow cone number i as in the handle of 257"""
    ns3 = ns3_inputs(NS3_ALONE, set_name, strategy)[name].reshape(-1, 3)
    sym = mixed_symmetric_inputs()
    idx = {k: i for i, k in enumerate(lay.ns3)}

    def per_cone(k, c):
        if k in idx:
            return ns3[idx[k]]
        if c["tag"] == GENPOW:
            g = R.gpw_case(c["d1"], c["d2"], mixed_gpw_set(set_name))
            return g["pt"][name] if name in ("s", "z") else g["x"] if name == "x" else np.zeros(c["numel"])
        if name in ("s", "z"):
            return sym[k][0 if name == "s" else 1]
        return np.full(c["numel"], 0.25) if name == "x" else np.zeros(c["numel"])
    return lay.fill(per_cone)


def symmetric_observations(lay, vals):
    """what the operations show of the SOC and nonnegative state: W e, W^-1 e of the cones' identities, their K entries"""
    unit = lay.fill(lambda k, c: np.eye(1, c["numel"], 0)[0] if c["tag"] == SOC else np.ones(c["numel"]) if c["tag"] == NN else None)
    _, we, wie = lay.combined_ds_shift(unit, unit, 0.0)
    keep = [k for k, c in enumerate(lay.info) if c["tag"] in (SOC, NN)]
    return [np.concatenate([we[lay.info[k]["rows"]], wie[lay.info[k]["rows"]], vals[lay.map_hs[lay.info[k]["hs"]]]]) for k in keep]


@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("set_name", R.GPW_SETS + ("inward 0",))
def test_every_cone_in_one_handle(hipdev, set_name, strategy):
    """layout (b): the `start`, hs_start, state_off and map_ptr offsets, the cone's number against its blockIdx, exp / pow
    cones in three runs with other cones between them.  Every exp / pow cone's outputs BITWISE those of the same cone in
    the handle of 257, every GenPow cone's those of the cone alone.  The GenPow cones have no inward set: there they
    hold the points of mixed_gpw_set under the exp / pow set's mu, and only the exp / pow cones are compared"""
    lay = layout(hipdev, "mixed")
    inp = ns3_inputs(NS3_ALONE, set_name, strategy)
    vec = lambda sn, name: mixed_vector(lay, sn, name, strategy)  # noqa: E731
    obs, vals = ns3_observe(lay, inp, strategy, set_name, vec)
    alone = ns3_alone(hipdev, NS3_ALONE, set_name, strategy)
    for name in obs:
        for i in range(NS3_ALONE):
            same_bits(obs[name][i], alone[name][i], "exp/pow cone %d in the mixed handle: %s" % (i, name))
    zero = np.zeros(lay.m)
    grad, hx = lay.combined_ds_shift(zero, zero, R.SIGMA_MU)[0], lay.mul_hs(vec(set_name, "x"))
    for k in lay.gpw if set_name in R.GPW_SETS else ():
        c = lay.info[k]
        got, want = gpw_observe(lay, k, vals, grad, hx), gpw_alone(hipdev, c["d1"], c["d2"], set_name, strategy)
        for name in GPW_OUTPUTS:
            same_bits(got[name], want[name], "GenPow (%d, %d) in the mixed handle: %s" % (c["d1"], c["d2"], name))


@pytest.mark.parametrize("alpha", R.BARRIER_ALPHAS)
def test_genpow_barrier_scratch_leaves_the_symmetric_state(hipdev, alpha):
    """kkt_cones.cpp (KktCones::barrier) passes the handle's w buffer -- the nonnegative and second-order scaling state -- to gpw_barrier as
    scratch for the primal gradients (`g = work + off`: the GenPow cone's own rows).  On the mixed handle: the barrier of
    the whole handle with ONE GenPow cone moved from its pair to its barrier pair changes by exactly what the cone alone
    gives (within the rounding of the sum); the SOC and nonnegative observations (W e, W^-1 e, K entries) are bitwise
    unchanged by the barrier calls; and after a further update_scaling of the same pair they and values() are bitwise
    what they were before"""
    lay = layout(hipdev, "mixed")
    s, z = mixed_vector(lay, "late 1", "s", 1), mixed_vector(lay, "late 1", "z", 1)
    dz, ds = np.zeros(lay.m), np.zeros(lay.m)
    for k in lay.gpw:  # every GenPow cone on its barrier pair (finite barriers), the other cones at rest
        c = lay.info[k]
        _, _, _, _, pt, gdz, gds = R.gpw_barrier_case(c["d1"], c["d2"], alpha)
        s[c["rows"]], z[c["rows"]], dz[c["rows"]], ds[c["rows"]] = pt["s"], pt["z"], gdz, gds
    vals = lay.scale(s, z, 1.0, 1)
    before = symmetric_observations(lay, vals)
    total = lay.barrier(z, s, dz, ds, alpha)
    assert np.isfinite(total)
    after = symmetric_observations(lay, lay.ks.values())
    for a, b in zip(before, after):
        same_bits(a, b, "SOC / nonnegative state changed by the GenPow barrier")
    same_bits(lay.ks.values(), vals, "values() changed by the barrier")
    # the GenPow cones' share of the total: the handle's barrier with the GenPow directions against the cones alone
    rest = lay.barrier(z, s, np.zeros(lay.m), np.zeros(lay.m), 0.0)
    gp0 = sum(gpw_barrier_alone(hipdev, lay.info[k]["d1"], lay.info[k]["d2"], 0.0) for k in lay.gpw)
    gpa = sum(gpw_barrier_alone(hipdev, lay.info[k]["d1"], lay.info[k]["d2"], alpha) for k in lay.gpw)
    scale = sum(abs(gpw_barrier_alone(hipdev, lay.info[k]["d1"], lay.info[k]["d2"], alpha)) for k in lay.gpw) + abs(rest)
    err = abs((total - rest) - (gpa - gp0)) / scale
    print("  NSYM-MIXED|barrier alpha %.1f|total %.12g|GenPow cones alone %.12g|err %.2e" % (alpha, total, gpa, err))
    assert err <= R.tol(0.0, lay.m)  # (the same per-cone numbers summed in another order)
    vals2 = lay.scale(s, z, 1.0, 1)
    same_bits(vals2, vals, "values() after a further update_scaling of the same pair")
    for a, b in zip(before, symmetric_observations(lay, vals2)):
        same_bits(a, b, "SOC / nonnegative state after a further update_scaling of the same pair")


MIXED_STEP_CASES = (("every cone stays feasible", "stays feasible", None, None),
                    ("the last exp / pow cone limits", "last cone limits", None, None),
                    ("the last GenPow cone limits", "stays feasible", (257, 0), "last u leaves"),
                    ("GenPow (300, 3) limits", "stays feasible", (300, 3), "last w leaves"),
                    ("GenPow (64, 64) ends at 0", "stays feasible", (64, 64), "ends at 0"))


@pytest.mark.parametrize("label,ns3_case,gpw_size,gpw_case", MIXED_STEP_CASES, ids=[c[0] for c in MIXED_STEP_CASES])
def test_step_length_in_one_handle(hipdev, label, ns3_case, gpw_size, gpw_case):
    """step_length of the mixed handle: the symmetric cones at rest (their step is alpha_max), the exp / pow partials in
    d_partial[0 .. 1] and the GenPow cones' behind them (kkt_cones.cpp `d_partial + used`); one cone, or none, limits the step.
    Bit for bit the smallest of the cones' exactly decided candidates"""
    lay = layout(hipdev, "mixed")
    set_name = R.STEP_SETS[0]
    ndz, nds, nz, ns, amax, _ = R.ns3_step_case(NS3_ALONE, set_name, ns3_case)
    want, margin = R.ns3_step_expected(NS3_ALONE, set_name, ns3_case)
    idx = {k: i for i, k in enumerate(lay.ns3)}
    sym = mixed_symmetric_inputs()
    gp = {}
    for k in lay.gpw:
        c = lay.info[k]
        case = gpw_case if (c["d1"], c["d2"]) == gpw_size else "stays feasible"
        gp[k] = R.gpw_step_case(c["d1"], c["d2"], R.GPW_STEP_SET, case)
        w, m = R.gpw_step_expected(c["d1"], c["d2"], R.GPW_STEP_SET, case)
        want, margin = min(want, w), min(margin, m)
    assert margin >= R.STEP_MARGIN

    def vec(which):  # 0 dz, 1 ds, 2 z, 3 s
        def per_cone(k, c):
            if k in idx:
                return (ndz, nds, nz, ns)[which].reshape(-1, 3)[idx[k]]
            if k in gp:
                return gp[k][which]
            return None if which < 2 else sym[k][1 if which == 2 else 0]
        return lay.fill(per_cone)
    got = lay.step_length(vec(0), vec(1), vec(2), vec(3), amax)
    print("  NSYM-STEP|mixed|%s|got %.17g|want %.17g|margin %.1e" % (label, got, want, margin))
    assert got == want
    if gpw_size is not None:
        assert want < R.ns3_step_expected(NS3_ALONE, set_name, ns3_case)[0]  # (the GenPow cone is what limits)
