"""The second-order and nonnegative cone kernels (clarabel.rs_amd/csrc/cones.hip) on the MI355X through the public
HipKKTSolver API, against the references of tests/soc_ref.py (tests/test_soc_ref_host.py checks those on the CPU), on
both sides of every size at which a cone operation changes its code path.  The path is a function of the cone's
dimension alone:

    dim 1 | 2         refused at construction (kkt_assembly.cpp:51 `c.dim < 2`, socone.rs:48)
    dim 4 | 5         dense Hs block, packed triu | sparse expansion with the u, v, D columns (kkt_assembly.cpp:56
                      `c.sparse = c.dim > 4`; cones.hip soc_write_kkt_body `sidx >= 0`, soc_scaling_reg `sidx >= 0`)
    dim 65 | 66       tail element i is thread i - 1's: the tail fills one wave | the second wave joins block_sum /
                      block_max (cones.hip reg_norm_tail, block_norm_tail `i = 1 + threadIdx.x`)
    dim 257 | 258     one tail element per thread | the second register slot (cones.hip soc_scaling_reg `i = 1 + tid + u *
                      WG`, u = 1) and the second trip of every `i += WG` loop
    dim 1025 | 1026   the last register slot, soc_scaling_reg | the memory-walking soc_update_scaling_body, followed by
                      soc_write_kkt_body on the fused route (cones.hip soc_scaling_reg `n > 1 + SOC_RPT * WG`)
    nonnegative rows  2048 workgroups x 256 rows | a second trip of the grid-stride loop (cones.hip nn_blocks,
                      k_nn_step_ops); 1024 x 256 for cone_step_length, cone_margins, cone_barrier (`nb > 1024`)
    blockIdx          < ncones: a cone | >= ncones: a slab of nonnegative rows (k_sym_update_scaling, k_sym_write_kkt,
                      k_sym_scale_write)

Handles: n = 1, P = [1], A one dense column of ones -- the cheapest chip_kkt_create accepts -- with
static_regularization_proportional = 2^-10 (the default 2^-104 makes the diagonal maximum invisible in the regulariser);
one handle per layout for the whole module.  (a) every dimension alone; (b) all of them in one handle, not sorted by
size, with Zero(3) and Nonnegative(300) cones between them.  A cone's results in (a) and in (b) must be bitwise equal.
There is no getter for the cones' state; it is read through the operations: combined_ds_shift of the cones' identities
returns eta w and J w / eta, affine_ds (||lambda||^2, 2 lambda0 lambda1), mul_Hs of z must give s, and values() after
update() holds the (unregularised) Hs diagonal or dense triu, the columns -eta^2 u, -eta^2 v and D = [-eta^2, +eta^2].

Tolerances: soc_ref.tol(E, n, kappa) = 16 max(E, n 2^-53, kappa 2^-53), E the error of the double restatement
(oracle.Cones) against mpmath on the same input, kappa the conditioning named per output in soc_ref's docstring; never a
flat figure.  Every figure is printed before it is asserted (pytest -s), E beside the device's error.

Measured on one MI355X, largest over all dimensions, E (device) per late set (k, mu, t) = (1, 1, 0.3) / (2, 1e-3, 0.1) /
(3, 1e-6, 1e-2) / (4, 1e-8, 1e-3):
    eta w                2.2e-14 (5.0e-15) / 9.5e-13 (1.5e-13) / 2.9e-10 (1.7e-11) / 1.0e-8 (2.5e-9)
    J w / eta            1.0e-14 (5.7e-15) / 9.7e-13 (1.4e-13) / 2.6e-10 (2.0e-11) / 7.8e-9 (3.0e-9)
    lambda o lambda      1.6e-14 (4.9e-15) / 6.9e-13 (2.3e-13) / 2.1e-10 (1.3e-11) / 6.9e-9 (4.3e-9)
    Hs block             2.7e-14 (1.0e-14) / 1.9e-12 (2.9e-13) / 5.5e-10 (3.4e-11) / 1.8e-8 (5.0e-9)
    -eta^2 u             3.5e-14 (7.8e-15) / 1.9e-12 (3.0e-13) / 5.6e-10 (3.0e-11) / 1.9e-8 (4.7e-9)
    -eta^2 v, D          2.8e-14 (8.0e-15) / 1.9e-12 (2.9e-13) / 5.5e-10 (3.2e-11) / 1.8e-8 (4.5e-9)
    Hs z = s             8.0e-14 (1.5e-14) / 1.2e-12 (4.9e-13) / 1.3e-10 (3.4e-11) / 1.1e-8 (7.3e-9)
    static regulariser   2.7e-14 (9.9e-15) / 1.9e-12 (2.9e-13) / 5.5e-10 (3.4e-11) / 1.8e-8 (5.0e-9)
kappa 2^-53 = 2.8e-15 / 2.8e-13 / 2.8e-11 / 2.8e-9; the largest E, 1.9e-8, is under the cap 1e-7, the loosest tolerance is
3.0e-7, and no device error was above 0.13 of its tolerance.  Nonnegative rows: every output within 1.3e-16 (E the same).
The two scaling routes were bitwise equal in values(), in every operation output and in the static regulariser at every
dimension, 1026 and 2050 included.

Three wrong kernels these tests would catch (argued, not run):
  * `i < n - 1` as the bound of a tail loop (block_norm_tail, or `in[u] = i < n - 1` in soc_scaling_reg): the last tail
    element leaves the norm and w.  The exact inputs carry their largest entry, 4, at the last index, so
    test_step_length_exact_inputs gets 10 instead of 2 for the direction that leaves through that element and a positive
    step instead of 0 from the boundary point, test_non_interior_input_is_reported sees True for s0 = ||s1||, and every
    late case of test_scaling_of_late_pairs is off by O(1 / sqrt n), not by rounding;
  * `in[u]` dropped from the `sq` accumulation of soc_scaling_reg (`sq += wr[u] * wr[u]` for every slot): the slots past
    the cone hold what the clamped loads brought, element 0 of s and z, so w1sq gains (s0 / sscale - z0 / zscale)^2 /
    wscale^2 per empty slot and w0 = sqrt(1 + w1sq), Hs[0], d, u0, u1, v1 are wrong by O(1) at every dimension below
    1025 -- eta_w, hs, ku, kv of test_scaling_of_late_pairs fail on both routes, while 1025 (no empty slot) and 1026,
    2050 (the memory-walking body) pass, which points at the slots;
  * the register-path bound off by one, `n > 2 + SOC_RPT * WG`: dimension 1026 stays in registers and its last element,
    index 1025, belongs to no slot (the largest is 1 + 255 + 3 * 256 = 1024) -- it leaves the norms and w[1025],
    lambda[1025] and row 1025 of the K columns are never written: test_scaling_of_late_pairs[1026-*] fails in eta_w,
    affine_ds, hs, ku, kv, and test_non_interior_input_is_reported[1026] sees True for s0 = ||s1||, whose tail has its
    largest entry exactly there.  (`n >= 1 + SOC_RPT * WG` instead sends 1025 to the memory-walking body, which computes
    the same numbers: a slower kernel, not a wrong one.)"""
import functools
import time

import mpmath as mp
import numpy as np
import pytest

from tests import soc_ref as R

pytestmark = pytest.mark.gpu

SOC, NN, ZERO = R.SOC, R.NN, R.ZERO
MIXED = ((SOC, 66), (ZERO, 3), (SOC, 3), (NN, 300), (SOC, 2050), (SOC, 5), (ZERO, 3), (SOC, 257), (SOC, 2), (NN, 300),
         (SOC, 1026), (SOC, 64), (SOC, 4), (SOC, 1025), (ZERO, 3), (SOC, 258), (SOC, 65))
NN_BIG = 2048 * 256 + 1
ROUTES = ("update_scaling + update", "update_scaled_enqueue + collect")


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


class Layout:
    """one HipKKTSolver over n = 1, P = [1], A = a dense column of ones, and where each cone's entries of K are"""

    def __init__(self, hip, cones):
        self.hip, self.cones = hip, tuple(cones)
        m = self.m = sum(d for _, d in cones)
        P = hip.CscMatrix(1, 1, [0, 1], [0], [1.0])
        A = hip.CscMatrix(m, 1, [0, m], np.arange(m), np.ones(m))
        # (the default static_regularization_proportional, 2^-104, leaves c + p max|diag K| at c = 1e-8 to the last bit:
        # with 2^-10 the maximum the cone kernels fold decides the regulariser; nothing else the tests read depends on it)
        st = hip.Settings.default(static_regularization_proportional=2.0 ** -10)
        t0 = time.perf_counter()
        self.ks = hip.HipKKTSolver(P, A, list(cones), m, 1, settings=st)
        self.create_seconds = time.perf_counter() - t0
        self.colptr = self.ks.kkt_matrix().colptr.astype(np.int64)
        map_hs = self.ks.maps()["Hsblocks"]
        self.info, start, h, sidx = [], 0, 0, 0
        for tag, d in cones:
            sparse = tag == SOC and d > 4
            blen = d * (d + 1) // 2 if tag == SOC and not sparse else d
            self.info.append(dict(tag=tag, dim=d, rows=slice(start, start + d), hs=map_hs[h:h + blen], sparse=sparse,
                                  col=1 + m + 2 * sidx if sparse else None))
            start, h, sidx = start + d, h + blen, sidx + sparse
        assert h == self.ks.nHs and self.ks.N == 1 + m + 2 * sidx
        self.d_s, self.d_z = hip.DeviceArray(m), hip.DeviceArray(m)
        self.unit = np.zeros(m)  # the identity of every cone (Zero rows: 0)
        for c in self.info:
            if c["tag"] == SOC:
                self.unit[c["rows"].start] = 1.0
            elif c["tag"] == NN:
                self.unit[c["rows"]] = 1.0

    def socs(self):
        return [k for k, c in enumerate(self.info) if c["tag"] == SOC]

    def scale(self, s, z, route, scramble=True):
        """-> the verdict of the route (route 0: update_scaling's, update() only after a success).  scramble: first scale
        the swapped pair (z, s) through the two calls, so that no state and no entry of K the route ought to write can
        be right because an earlier call left it there"""
        if scramble:
            assert self.scale(z, s, 0, scramble=False)
        self.d_s.copy_from(s)
        self.d_z.copy_from(z)
        if route == 0:
            if not self.ks.update_scaling(s, z):
                return False
            return self.ks.update()
        self.ks.update_scaled_enqueue(self.d_s.ptr, self.d_z.ptr)
        uok, sok = self.ks.collect()
        assert sok == []
        return uok

    def _run(self, call, outs):
        call()
        self.ks.synchronize()
        return [o.numpy() for o in outs]

    def mul_hs(self, x):
        D = self.hip.DeviceArray
        y, dx = D(self.m), D(x)
        return self._run(lambda: self.ks.mul_Hs_dev(y.ptr, dx.ptr), [y])[0]

    def affine_ds(self):
        out = self.hip.DeviceArray(self.m)
        return self._run(lambda: self.ks.affine_ds_dev(out.ptr, self.d_s.ptr), [out])[0]

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

    def margins(self, z):
        a = self.hip.DeviceArray(z)
        return self.ks.margins_dev(a.ptr)

    def barrier(self, z, s, dz, ds, alpha):
        a = [self.hip.DeviceArray(v) for v in (z, s, dz, ds)]
        return self.ks.compute_barrier_dev(a[0].ptr, a[1].ptr, a[2].ptr, a[3].ptr, alpha)

    def observe(self):
        """everything the operations show of the state of ALL cones: (shift, W e, W^-1 e, affine_ds, values())"""
        sh, we, wie = self.combined_ds_shift(self.unit, self.unit, 0.0)
        return dict(we=we, wie=wie, aff=self.affine_ds(), vals=self.ks.values(), eps=self.ks.linear_solver_info().last_regularizer)

    def state(self, obs, k):
        """cone k's part of observe(), named like soc_ref.reference_state"""
        c, vals, cp = self.info[k], obs["vals"], self.colptr
        out = dict(eta_w=obs["we"][c["rows"]], Jw_eta=obs["wie"][c["rows"]], affine_ds=obs["aff"][c["rows"]], hs=-vals[c["hs"]])
        if c["sparse"]:
            col, d = c["col"], c["dim"]
            out.update(kv=vals[cp[col]:cp[col] + d], ku=vals[cp[col + 1]:cp[col + 1] + d],
                       D=np.array([vals[cp[col + 1] - 1], vals[cp[col + 2] - 1]]))
        return out


_LAYOUTS = {}


@pytest.fixture(scope="module", autouse=True)
def release_handles():
    """the handles and device results cached for the module are released with it, not at interpreter exit"""
    yield
    for cache in (_LAYOUTS, _SINGLE, _OPS):
        cache.clear()


def layout(hip, cones):
    cones = tuple(cones)
    if cones not in _LAYOUTS:
        _LAYOUTS[cones] = Layout(hip, cones)
        print("  (handle %s: %.3f s)" % (" ".join("%d:%d" % c for c in cones[:6]) + (" ..." if len(cones) > 6 else ""),
                                        _LAYOUTS[cones].create_seconds))
    return _LAYOUTS[cones]


def single(hip, n):
    return layout(hip, ((SOC, n),))


class Checks:
    """prints every figure, collects the failures, asserts at the end"""

    def __init__(self, label):
        self.label, self.fails = label, []

    def __call__(self, name, err, E, allowed):
        ok = err <= allowed
        print("  %s %-28s err %.2e  E %.2e  allowed %.2e%s" % (self.label, name, err, E, allowed, "" if ok else "  <-- FAIL"))
        if not ok:
            self.fails.append((name, err, allowed))

    def done(self):
        assert not self.fails, (self.label, self.fails)


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), (what, float(np.max(np.abs(a - b))) if a.shape == b.shape else "shape")


def expected_eps(lay, maxdiag):
    st = lay.ks.settings
    assert st.static_regularization_enable
    return st.static_regularization_constant + st.static_regularization_proportional * float(maxdiag)


def test_dimension_one_is_refused(hipdev):
    """socone.rs:48 asserts dim >= 2; chip_kkt_create reports the same instead of building a cone without a tail"""
    with pytest.raises(hipdev.ChipError):
        Layout(hipdev, ((SOC, 1),))


# ---- 1. the scaling of late pairs, both routes -----------------------------------------------------------------------
_SINGLE = {}


def single_scaled(hip, n, which):
    """the observations of cone n alone, scaled with late set `which`, per route (cached: the mixed handle is compared
    with them bitwise); also mul_Hs of z"""
    if (n, which) not in _SINGLE:
        c, lay, out = R.late_case(n, which), single(hip, n), []
        for route in (0, 1):
            ok = lay.scale(c["s"], c["z"], route)
            obs = lay.observe()
            st = lay.state(obs, 0)
            st["hs_z"] = lay.mul_hs(c["z"])
            out.append(dict(ok=ok, state=st, eps=obs["eps"]))
        _SINGLE[(n, which)] = out
    return _SINGLE[(n, which)]


@pytest.mark.parametrize("which", range(len(R.LATE_SETS)))
@pytest.mark.parametrize("n", R.DIMS)
def test_scaling_of_late_pairs(hipdev, n, which):
    """late pairs (s with eigenvalues 10^+-k, z = mu s^-1 turned by t; (k, mu, t) = soc_ref.LATE_SETS) at every dimension,
    through update_scaling + update (k_sym_update_scaling, k_sym_write_kkt) and through update_scaled_enqueue + collect
    (k_sym_scale_write: soc_scaling_reg<true> up to 1025 rows, soc_update_scaling_body + soc_write_kkt_body from 1026):
    eta w, J w / eta, lambda o lambda, the Hs block, the K columns -eta^2 u, -eta^2 v, D, Hs z = s and the static
    regulariser c + p max(1, max|diag Hs|, eta^2) of each route against mpmath within tol(E, n, kappa); the two routes
    bitwise equal to each other (they were, at every dimension: the memory-walking body sums the same partial sums as the
    registers).

    Largest E (device) over the dimensions for the four sets: Hs block 2.7e-14 (1.0e-14) / 1.9e-12 (2.9e-13) / 5.5e-10
    (3.4e-11) / 1.8e-8 (5.0e-9); the other outputs in the module docstring."""
    c = R.late_case(n, which)
    assert max(c["E"].values()) <= R.E_CAP  # a regenerated input cannot make the case vacuous
    runs = single_scaled(hipdev, n, which)
    ck = Checks("n=%d set=%d" % (n, which))
    E_hsz = R.rel_vec(c["cone"].mul_Hs(c["z"]), R.mpv(c["s"]))
    lay = single(hipdev, n)
    eps_ref = expected_eps(lay, max(mp.mpf(1), c["ref"].max_diag(c["sparse"])))
    for route, run in enumerate(runs):
        assert run["ok"], ROUTES[route]
        for name in sorted(c["state"]):
            ck("%s [route %d]" % (name, route), R.rel_vec(run["state"][name], c["state"][name]), c["E"][name],
               R.tol(c["E"][name], n, c["kappa"]))
        ck("Hs z = s [route %d]" % route, R.rel_vec(run["state"]["hs_z"], R.mpv(c["s"])), E_hsz, R.tol(E_hsz, n, c["kappa"]))
        ck("static regulariser [route %d]" % route, abs(run["eps"] - eps_ref) / eps_ref, c["E"]["hs"],
           4 * R.U53 + R.tol(c["E"]["hs"], n, c["kappa"]))
    ck.done()
    for name in runs[0]["state"]:
        same_bits(runs[0]["state"][name], runs[1]["state"][name], "routes differ in " + name)
    assert runs[0]["eps"] == runs[1]["eps"]


@functools.lru_cache(maxsize=None)
def mixed_inputs(which):
    """s, z of the mixed handle: every second-order cone the late pair of its dimension, nonnegative rows uniform in
    [0.5, 2], Zero rows 1"""
    rng = np.random.default_rng(40 + which)
    s, z = [], []
    for tag, d in MIXED:
        if tag == SOC:
            c = R.late_case(d, which)
            s.append(c["s"])
            z.append(c["z"])
        else:
            s.append(rng.uniform(0.5, 2.0, d) if tag == NN else np.ones(d))
            z.append(rng.uniform(0.5, 2.0, d) if tag == NN else np.ones(d))
    return np.concatenate(s), np.concatenate(z)


@pytest.mark.parametrize("which", range(len(R.LATE_SETS)))
def test_all_dimensions_in_one_handle(hipdev, which):
    """layout (b): all dimensions in one handle, unsorted, with Zero(3) and Nonnegative(300) cones between them -- the
    `start` offsets, the hs_start / sp_ptr offsets of the K maps and the cone | nonnegative-slab split of the grid.
    Every cone's observations are BITWISE those of the cone alone, for both routes; the nonnegative rows against the
    extended-precision reference; the static regulariser from the largest diagonal entry of all cones."""
    lay = layout(hipdev, MIXED)
    s, z = mixed_inputs(which)
    ck = Checks("mixed set=%d" % which)
    eps = []
    for route in (0, 1):
        assert lay.scale(s, z, route), ROUTES[route]
        obs = lay.observe()
        hs_z = lay.mul_hs(z)
        eps.append(obs["eps"])
        maxdiag, E_hs, kap = mp.mpf(1), 0.0, 1.0
        for k, info in enumerate(lay.info):
            if info["tag"] == SOC:
                n = info["dim"]
                alone, st = single_scaled(hipdev, n, which)[route], lay.state(obs, k)
                for name in st:
                    same_bits(st[name], alone["state"][name], "cone %d (dim %d) route %d: %s" % (k, n, route, name))
                same_bits(hs_z[info["rows"]], alone["state"]["hs_z"], "cone %d (dim %d) route %d: Hs z" % (k, n, route))
                c = R.late_case(n, which)
                maxdiag, E_hs, kap = max(maxdiag, c["ref"].max_diag(info["sparse"])), max(E_hs, c["E"]["hs"]), max(kap, c["kappa"])
            elif info["tag"] == NN:
                ref = R.NnScaling(s[info["rows"]], z[info["rows"]])
                st = lay.state(obs, k)
                sd, zd = s[info["rows"]], z[info["rows"]]
                for name, got, want, dbl in (("w", st["eta_w"], ref.w, np.sqrt(sd / zd)), ("1 / w", st["Jw_eta"], 1 / ref.w, 1 / np.sqrt(sd / zd)),
                                             ("lambda^2", st["affine_ds"], ref.affine_ds(), np.sqrt(sd * zd) ** 2),
                                             ("w^2 in K", st["hs"], ref.hs(), np.sqrt(sd / zd) ** 2),
                                             ("Hs z", hs_z[info["rows"]], ref.mul_hs(zd), np.sqrt(sd / zd) * (np.sqrt(sd / zd) * zd))):
                    E = R.rel_ld(dbl, want)
                    ck("NN cone %d %s [route %d]" % (k, name, route), R.rel_ld(got, want), E, R.tol(E, 1))
                maxdiag = max(maxdiag, mp.mpf(float(np.max(ref.hs()))))
            else:
                assert np.all(hs_z[info["rows"]] == 0.0) and np.all(obs["vals"][info["hs"]] == 0.0)
        eps_ref = expected_eps(lay, maxdiag)
        ck("static regulariser [route %d]" % route, abs(obs["eps"] - eps_ref) / eps_ref, E_hs, 4 * R.U53 + R.tol(E_hs, 2050, kap))
    ck.done()
    assert eps[0] == eps[1]


# ---- 2. the operations on a late scaling -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def op_inputs(n, which):
    """directions relative to the iterate (soc_ref.relative_direction: W dz and W^-1 ds stay of the size of lambda, as the
    solver's directions do; a direction that ignores the scaling of a late iterate makes ds_from_dz_offset cancel far
    beyond kappa and E leaves its cap from dimension 257 on), a random vector for mul_Hs, and a right-hand side for
    ds_from_dz_offset of the kind the solver passes: lambda o lambda plus half a shift, from the double restatement"""
    c = R.late_case(n, which)
    rng = np.random.default_rng(31 * n + which)
    dz, ds = R.relative_direction(c["z"], 200 + n), R.relative_direction(c["s"], 300 + n)
    smu = 0.37 * float(c["s"] @ c["z"])
    rhs = c["cone"].affine_ds(c["s"]) + 0.5 * c["cone"].combined_ds_shift(dz, ds, smu)[0]
    return dict(dz=dz, ds=ds, x=rng.standard_normal(n), sigma_mu=smu, rhs=rhs)


OP_SETS = (0, 3)
_OPS = {}


def single_ops(hip, n, which):
    """the operation outputs of cone n alone on late set `which` (route 0), cached for the mixed handle"""
    if (n, which) not in _OPS:
        c, inp, lay = R.late_case(n, which), op_inputs(n, which), single(hip, n)
        assert lay.scale(c["s"], c["z"], 0)
        sh, wz, ws = lay.combined_ds_shift(inp["dz"], inp["ds"], inp["sigma_mu"])
        aff = lay.affine_ds()
        _OPS[(n, which)] = dict(mul_hs=lay.mul_hs(inp["x"]), affine_ds=aff, shift=sh, wz=wz, ws=ws,
                                ds_from_dz_offset=lay.ds_from_dz_offset(inp["rhs"], c["z"]), chain=lay.ds_from_dz_offset(aff + sh, c["z"]))
    return _OPS[(n, which)]


@pytest.mark.parametrize("which", OP_SETS)
@pytest.mark.parametrize("n", R.DIMS)
def test_operations_on_late_scaling(hipdev, n, which):
    """mul_Hs, affine_ds, combined_ds_shift (shift, W dz, W^-1 ds), ds_from_dz_offset and the chain the solver runs,
    ds_from_dz_offset(affine_ds + shift), after update_scaling of a late pair (sets (1, 1, 0.3) and (4, 1e-8, 1e-3)),
    against the reference evaluated in 60 digits WITH THE EXACT SCALING of the same s, z, not with the device's state:
    the errors are the compound errors the solver sees.  E of oracle.Cones per output beside the device's error.

    Largest E (device) over the dimensions, sets (1, 1, 0.3) / (4, 1e-8, 1e-3): mul_Hs 4.0e-14 (1.0e-14) / 2.0e-8 (5.0e-9),
    shift 3.2e-15 (3.2e-15) / 3.0e-9 (3.0e-9), W dz 1.3e-14 (6.3e-15) / 9.8e-9 (9.8e-9), W^-1 ds 1.4e-14 (6.2e-15) / 8.6e-9
    (3.5e-9), ds_from_dz_offset 2.3e-14 (1.0e-14) / 3.3e-8 (7.9e-9), chain 1.3e-13 (3.8e-14) / 3.2e-8 (1.3e-8)."""
    c, inp, dev = R.late_case(n, which), op_inputs(n, which), single_ops(hipdev, n, which)
    assert max(c["E"].values()) <= R.E_CAP
    ref, cone = c["ref"], c["cone"]
    dz, ds, x, smu = inp["dz"], inp["ds"], inp["x"], inp["sigma_mu"]
    sh, wz, ws = ref.combined_ds_shift(dz, ds, smu)
    with mp.workdps(R.DPS):
        chain = ref.ds_from_dz_offset([a + b for a, b in zip(ref.affine_ds(), sh)], c["z"])
    refs = dict(mul_hs=ref.mul_hs(x), affine_ds=ref.affine_ds(), shift=sh, wz=wz, ws=ws,
                ds_from_dz_offset=ref.ds_from_dz_offset(inp["rhs"], c["z"]), chain=chain)
    osh, owz, ows = cone.combined_ds_shift(dz, ds, smu)
    oaff = cone.affine_ds(c["s"])
    orc = dict(mul_hs=cone.mul_Hs(x), affine_ds=oaff, shift=osh, wz=owz, ws=ows,
               ds_from_dz_offset=cone.ds_from_dz_offset(inp["rhs"], c["z"]), chain=cone.ds_from_dz_offset(oaff + osh, c["z"]))
    ck = Checks("n=%d set=%d" % (n, which))
    for name in refs:
        E = R.rel_vec(orc[name], refs[name])
        assert E <= R.E_CAP, name
        ck(name, R.rel_vec(dev[name], refs[name]), E, R.tol(E, n, c["kappa"]))
    ck.done()


@pytest.mark.parametrize("which", OP_SETS)
def test_operations_in_one_handle(hipdev, which):
    """the same operations on the mixed handle: every cone's outputs BITWISE those of the cone alone (a cone's arithmetic
    does not depend on its blockIdx, its `start` or its neighbours); nonnegative rows against extended precision"""
    lay = layout(hipdev, MIXED)
    s, z = mixed_inputs(which)
    rng = np.random.default_rng(77 + which)
    dz, ds, x, rhs = (rng.uniform(0.1, 1.0, lay.m) * rng.choice([-1.0, 1.0], lay.m) for _ in range(4))
    smu = 0.37
    for k in lay.socs():
        inp, rows = op_inputs(lay.info[k]["dim"], which), lay.info[k]["rows"]
        dz[rows], ds[rows], x[rows], rhs[rows] = inp["dz"], inp["ds"], inp["x"], inp["rhs"]
    assert lay.scale(s, z, 0)
    # (sigma mu is one number for the whole handle: the second-order cones are compared through a launch per value)
    aff, hx, off = lay.affine_ds(), lay.mul_hs(x), lay.ds_from_dz_offset(rhs, z)
    ck = Checks("mixed ops set=%d" % which)
    for k, info in enumerate(lay.info):
        rows = info["rows"]
        if info["tag"] == SOC:
            n = info["dim"]
            alone = single_ops(hipdev, n, which)
            sh, wz, ws = lay.combined_ds_shift(dz, ds, op_inputs(n, which)["sigma_mu"])
            got = dict(mul_hs=hx[rows], affine_ds=aff[rows], shift=sh[rows], wz=wz[rows], ws=ws[rows], ds_from_dz_offset=off[rows],
                       chain=lay.ds_from_dz_offset(aff + sh, z)[rows])
            for name in got:
                same_bits(got[name], alone[name], "cone %d (dim %d): %s" % (k, n, name))
        elif info["tag"] == NN:
            ref = R.NnScaling(s[rows], z[rows])
            sh, wz, ws = lay.combined_ds_shift(dz, ds, smu)
            rsh, rwz, rws = ref.combined_ds_shift(dz[rows], ds[rows], smu)
            w = np.sqrt(s[rows] / z[rows])
            dwz, dws = dz[rows] * w, ds[rows] / w
            for name, got, want, dbl in (("mul_hs", hx[rows], ref.mul_hs(x[rows]), w * (w * x[rows])), ("W dz", wz[rows], rwz, dwz),
                                         ("W^-1 ds", ws[rows], rws, dws), ("shift", sh[rows], rsh, dws * dwz - smu),
                                         ("ds_from_dz_offset", off[rows], ref.ds_from_dz_offset(rhs[rows], z[rows]), rhs[rows] / z[rows])):
                E = R.rel_ld(dbl, want)
                ck("NN cone %d %s" % (k, name), R.rel_ld(got, want), E, R.tol(E, 1))
        else:
            sh = lay.combined_ds_shift(dz, ds, smu)[0]
            assert np.all(hx[rows] == 0.0) and np.all(aff[rows] == 0.0) and np.all(off[rows] == 0.0) and np.all(sh[rows] == 0.0)
    ck.done()


# ---- 3. step_length --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", OP_SETS)
@pytest.mark.parametrize("n", R.DIMS)
def test_step_length_generic_directions(hipdev, n, which):
    """directions relative to the iterate, dz = P(z^1/2) g and ds = P(s^1/2) g' with g = (0.1, 0.4 v), |v| = 1 (the
    iterate leaves the cone at alpha = 1 / 0.3 whatever its conditioning), scaled 0.05 / 1 / 40, alpha_max = 1: the full
    step EXACTLY where the direction is interior by a wide margin (scales 0.05 and 1: the boundary is at 66.7 and 3.33),
    1 / 12 within tol for scale 40.  Margin from the reference's rounding-dependent branches (socone.rs:450-471): with x
    the iterate, a = det(x) det(g) scale^2 = -0.15 scale^2 det(x), b = 2 g0 scale det(x) = 0.2 scale det(x), c = det(x) and
    d = 4 ||g1||^2 scale^2 det(x)^2 = 0.64 scale^2 det(x)^2 = 16 b^2: a is negative and 15 times b^2 / (4 c) in size, d is 16 b^2,
    so neither a = 0 nor d = 0 is within reach of a rounding error of relative size kappa 2^-53 <= 3e-9.

    Largest E (device) of the scale-40 step over the dimensions: 1.8e-14 (8.2e-15) / 1.5e-8 (2.7e-9); scales 0.05 and 1 gave
    1.0 exactly at every dimension."""
    c = R.late_case(n, which)
    lay = single(hipdev, n)
    s, z = c["s"], c["z"]
    dz1, ds1 = R.relative_direction(z, 500 + n), R.relative_direction(s, 900 + n)
    ck = Checks("n=%d set=%d" % (n, which))
    for scale in (0.05, 1.0, 40.0):
        dz, ds = scale * dz1, scale * ds1
        want = R.soc_step_length(dz, ds, z, s, 1.0)
        got, orc = lay.step_length(dz, ds, z, s, 1.0), c["cone"].step_length(dz, ds, z, s, 1.0)
        E = R.rel_scalar(orc, want)
        assert E <= R.E_CAP
        kap = R.kappa_of(z, s, dz, ds)
        ck("step_length scale %g (exact %.6g)" % (scale, float(want)), R.rel_scalar(got, want), E, R.tol(E, n, kap))
        if scale <= 1.0:
            assert float(want) == 1.0 and got == 1.0
        else:
            assert abs(float(want) * 12.0 - 1.0) <= 1e-6  # (the direction itself is rounded: kappa 2^-53 <= 3e-9)
    ck.done()


def exact_step_cases(n):
    """-> list of (name, x, y, alpha_max, exact step) of soc_step_roots' branches on the integer inputs"""
    x, r = R.exact_tail(n)
    e0, last = np.zeros(n), np.zeros(n)
    e0[0], last[n - 1] = 1.0, 1.0
    on = x.copy()
    on[0] = r
    z2 = on + r * e0
    cases = [("a == 0: direction on the boundary", 2.0 * r * e0, on, 10.0, 10.0),
             ("a == 0 and the scalar bound 2 r / r", 2.0 * r * e0, -on, 10.0, 2.0),
             ("c == 0, direction inside", on, e0, 10.0, 10.0),
             ("c == 0, direction outside", on, -last, 10.0, 0.0),
             ("the scalar bound alone", 2.0 * e0, -e0, 10.0, 2.0),
             ("leaves through the last tail element", 2.0 * e0, last, 10.0, 2.0),
             ("dz = -z: a root exactly at the step limit", z2, -z2, 1.0, 1.0)]
    if R.has_ones_tail(n):
        o, ro = R.exact_tail(n, ones=True)
        bo = o.copy()
        bo[0] = ro
        cases += [("ones: c == 0, direction outside", bo, -last, 10.0, 0.0),
                  ("ones: dz = -z", bo + ro * e0, -(bo + ro * e0), 1.0, 1.0),
                  ("ones: a == 0 and the scalar bound", 2.0 * ro * e0, -bo, 10.0, 2.0)]
    return cases


@pytest.mark.parametrize("n", R.DIMS)
def test_step_length_exact_inputs(hipdev, n):
    """the branches of soc_step_roots no random direction reaches, on inputs whose norms, dot products and residuals are
    exact in double in any summation order (integer tails with nonzeros at indices 1, 64, 65, 256, 257, 1024, 1025 and
    the last one -- its largest entry; 1024 ones at dimension 1025): a == 0 (direction on the boundary -> alpha_max = 10;
    its negative -> the scalar bound 2), c == 0 (start on the boundary: direction inside -> 10, outside -> 0), the scalar
    bound alone (x = (2; 0), y = (-1; 0) -> 2), a direction that leaves through the tail element at the last index (-> 2;
    10 if that element is dropped), and dz = -z, ds = -s with alpha_max = 1: d = 0 exactly, both roots 1.  Each case on
    the z side and on the s side, the other side at rest (x = e, y = 0: a = b = d = 0 -> alpha_max).  The results are
    exact, so they are compared with == ; the root at the step limit within tol(0, n, 4 / 3) as well."""
    lay = single(hipdev, n)
    e0, zero = np.zeros(n), np.zeros(n)
    e0[0] = 1.0
    fails = []
    for name, x, y, amax, want in exact_step_cases(n):
        assert float(R.soc_step_component(x, y, amax)) == want, name
        for side, args in (("z", (y, zero, x, e0)), ("s", (zero, y, e0, x))):
            got = lay.step_length(*args, amax)
            print("  n=%d %-45s %s side: %.17g (exact %g)" % (n, name, side, got, want))
            if name.endswith("step limit"):
                assert abs(got - want) <= R.tol(0.0, n, 4.0 / 3.0), (name, side)
            if got != want:
                fails.append((name, side, got, want))
    assert not fails, fails


# ---- 4. margins and compute_barrier ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", OP_SETS)
@pytest.mark.parametrize("n", R.DIMS)
def test_margins_and_barrier(hipdev, n, which):
    """margins (z0 - ||z1||, its positive part) absolutely over z0, and compute_barrier at alpha = 0 and alpha = 0.7 along
    directions relative to the iterate, absolutely over max(1, |barrier|), on late iterates; the exact inputs ((2 r; tail):
    margin r exactly, barrier -log(3 r^2); (-2 r; tail): margin -3 r, negative) and one point outside the cone, whose
    barrier is +inf.

    Largest E (device) over the dimensions, sets (1, 1, 0.3) / (4, 1e-8, 1e-3): margins over z0 7.6e-16 (1.8e-16) / 5.6e-16
    (1.8e-16), barrier at alpha = 0 1.1e-14 (7.1e-15) / 9.7e-10 (3.2e-10), at alpha = 0.7 3.2e-14 (8.0e-15) / 2.0e-9 (3.0e-10);
    the exact inputs gave the exact margins and a barrier equal to -log(3 r^2) as numpy rounds it."""
    c = R.late_case(n, which)
    lay, cone = single(hipdev, n), c["cone"]
    s, z = c["s"], c["z"]
    ck = Checks("n=%d set=%d" % (n, which))
    for name, v in (("z", z), ("s", s)):
        a_ref, b_ref = R.soc_margins(v)
        (a, b), (ao, bo) = lay.margins(v), cone.margins(v)
        E = float(abs(mp.mpf(ao) - a_ref)) / v[0]
        ck("margin of " + name, float(abs(mp.mpf(a) - a_ref)) / v[0], E, R.tol(E, n))
        ck("positive part of " + name, float(abs(mp.mpf(b) - b_ref)) / v[0], E, R.tol(E, n))
        assert a > 0 and b == a
    dz, ds = R.relative_direction(z, 500 + n), R.relative_direction(s, 900 + n)
    for alpha in (0.0, 0.7):
        want, kap = R.soc_barrier(z, s, dz, ds, alpha)
        got, orc = lay.barrier(z, s, dz, ds, alpha), cone.compute_barrier(z, s, dz, ds, alpha)
        den = max(1.0, abs(float(want)))
        E = float(abs(mp.mpf(orc) - want)) / den
        assert E <= R.E_CAP
        ck("barrier alpha %.1f (%.6g)" % (alpha, float(want)), float(abs(mp.mpf(got) - want)) / den, E, R.tol(E, n, kap))
    out = np.zeros(n)
    out[0] = -0.9 * z[0]  # z + out: z0 -> 0.1 z0, below the norm of the tail for every late set
    assert R.soc_barrier(z, s, out, ds, 1.0)[0] == mp.inf
    out_s = np.zeros(n)
    out_s[0] = -0.9 * s[0]
    assert lay.barrier(z, s, out, ds, 1.0) == np.inf and lay.barrier(z, s, dz, out_s, 1.0) == np.inf
    a, b = lay.margins(z + out)
    a_ref = R.soc_margins(z + out)[0]
    ck("margin outside the cone", float(abs(mp.mpf(a) - a_ref)) / z[0], 0.0, R.tol(0.0, n))
    assert a < 0 and b == 0.0
    # the exact inputs
    x, r = R.exact_tail(n)
    e0 = np.zeros(n)
    e0[0] = 1.0
    z2 = x + 2.0 * r * e0
    assert lay.margins(z2) == (r, r) and lay.margins(x - 2.0 * r * e0) == (-3.0 * r, 0.0)
    zero = np.zeros(n)
    want = -np.log(3.0 * r * r)
    got = lay.barrier(z2, z2, zero, zero, 0.0)
    ck("barrier of the exact input", abs(got - want) / abs(want), 0.0, R.tol(0.0, n, 4.0 / 3.0))
    assert lay.barrier(z2, z2, -2.0 * r * e0, zero, 0.7) == np.inf  # z0 = 0.6 r < r
    ck.done()


# ---- 5. non-interior input -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 66, 1026])
def test_non_interior_input_is_reported(hipdev, n):
    """per scaling path (dense, registers, memory-walking): s0 = ||s1|| EXACTLY (the integer inputs), the same for z, and
    s0 < ||s1||.  update_scaling returns False (socone.rs:149-151) -- the ordinary return path through the failure flag
    -- and the fused route's verdict arrives with collect(); the verdict is not sticky: the next call with interior points
    succeeds and every state is right.  Nothing is pinned about the state after a failure."""
    lay, c = single(hipdev, n), R.late_case(n, 0)
    x, r = R.exact_tail(n)
    on, below = x.copy(), x.copy()
    on[0], below[0] = r, r - 1.0
    good = single_scaled(hipdev, n, 0)
    for route in (0, 1):
        for what, bad_s, bad_z in (("s0 = ||s1||", on, c["z"]), ("z0 = ||z1||", c["s"], on), ("s0 < ||s1||", below, c["z"]),
                                   ("z0 < ||z1||", c["s"], below)):
            verdict = lay.scale(bad_s, bad_z, route, scramble=False)
            print("  n=%d route %d %s -> %s" % (n, route, what, verdict))
            assert verdict is False, (ROUTES[route], what)
            assert lay.scale(c["s"], c["z"], route) is True, (ROUTES[route], what)
            obs = lay.observe()
            st = lay.state(obs, 0)
            for name in st:
                same_bits(st[name], good[route]["state"][name], "after a failure (%s, route %d): %s" % (what, route, name))
            assert obs["eps"] == good[route]["eps"]


# ---- 6. nonnegative rows ---------------------------------------------------------------------------------------------
def test_nonnegative_rows_past_the_grid_caps(hipdev):
    """SecondOrder(66), Nonnegative(2048 * 256 + 1), SecondOrder(5) in one handle: the row count is one past the 2048-block
    cap of nn_blocks / k_nn_step_ops (the last row is reached only by the second trip of the grid-stride loop) and far
    past the 1024-block cap of cone_step_length, cone_margins and cone_barrier; the nonnegative slab starts at blockIdx 2.
    Scaling through both routes (w, 1 / w, lambda^2, -w^2 in K), mul_Hs, combined_ds_shift, ds_from_dz_offset against
    longdouble (kappa = 1: a few roundings each), step_length and margins with the binding row the LAST one and row
    1024 * 256, barrier at alpha = 0 and 0.7.  The handle is created in 0.13 s on the MI355X machine, so the full
    2048 * 256 + 1 rows are kept; the whole test takes 0.9 s.  Measured: every elementwise output within 1.3e-16 of the
    reference (E the same), the sums within 9.4e-16 of the sum of their terms' magnitudes, the binding steps 0.25 and 0.125
    and the minima -3.25 and -3.125 exactly."""
    cones = ((SOC, 66), (NN, NN_BIG), (SOC, 5))
    lay = layout(hipdev, cones)
    print("  handle with Nonnegative(%d): created in %.2f s" % (NN_BIG, lay.create_seconds))
    rng = np.random.default_rng(6)
    c66, c5 = R.late_case(66, 0), R.late_case(5, 0)
    nn = lay.info[1]["rows"]
    s = np.concatenate([c66["s"], rng.uniform(0.5, 2.0, NN_BIG), c5["s"]])
    z = np.concatenate([c66["z"], rng.uniform(0.5, 2.0, NN_BIG), c5["z"]])
    ref = R.NnScaling(s[nn], z[nn])
    w = np.sqrt(s[nn] / z[nn])
    lam = np.sqrt(s[nn] * z[nn])
    ck = Checks("NN")
    states = []
    for route in (0, 1):
        assert lay.scale(s, z, route), ROUTES[route]
        obs = lay.observe()
        st = lay.state(obs, 1)
        states.append((obs, st))
        for name, got, want, dbl in (("w", st["eta_w"], ref.w, w), ("1 / w", st["Jw_eta"], 1 / ref.w, 1 / w),
                                     ("lambda^2", st["affine_ds"], ref.affine_ds(), lam * lam), ("w^2 in K", st["hs"], ref.hs(), w * w)):
            E = R.rel_ld(dbl, want)
            ck("%s [route %d]" % (name, route), R.rel_ld(got, want), E, R.tol(E, 1))
            assert np.max(np.abs(R.ld(got) / want - 1)) <= R.tol(E, 1), name  # row by row: no row left out or stale
        # the second-order cones either side of the slab are untouched by it
        for k, n in ((0, 66), (2, 5)):
            alone = single_scaled(hipdev, n, 0)[route]["state"]
            sk = lay.state(obs, k)
            for name in sk:
                same_bits(sk[name], alone[name], "cone of dim %d beside the slab, route %d: %s" % (n, route, name))
        maxdiag = max(c66["ref"].max_diag(True), c5["ref"].max_diag(True), mp.mpf(float(np.max(ref.hs()))), mp.mpf(1))
        eps_ref = expected_eps(lay, maxdiag)
        ck("static regulariser [route %d]" % route, abs(obs["eps"] - eps_ref) / eps_ref, 0.0, 4 * R.U53 + R.tol(0.0, 66, c66["kappa"]))
    for name in states[0][1]:
        same_bits(states[0][1][name], states[1][1][name], "routes differ in " + name)
    same_bits(states[0][0]["vals"], states[1][0]["vals"], "routes differ in values()")
    # operations
    dz, ds, x = (rng.uniform(0.1, 1.0, lay.m) * rng.choice([-1.0, 1.0], lay.m) for _ in range(3))
    smu = 0.37
    sh, wz, ws = lay.combined_ds_shift(dz, ds, smu)
    rsh, rwz, rws = ref.combined_ds_shift(dz[nn], ds[nn], smu)
    dwz, dws = dz[nn] * w, ds[nn] / w
    for name, got, want, dbl in (("mul_hs", lay.mul_hs(x)[nn], ref.mul_hs(x[nn]), w * (w * x[nn])), ("W dz", wz[nn], rwz, dwz),
                                 ("W^-1 ds", ws[nn], rws, dws), ("shift", sh[nn], rsh, dws * dwz - smu),
                                 ("ds_from_dz_offset", lay.ds_from_dz_offset(ds, z)[nn], ref.ds_from_dz_offset(ds[nn], z[nn]), ds[nn] / z[nn])):
        E = R.rel_ld(dbl, want)
        ck(name, R.rel_ld(got, want), E, R.tol(E, 1))
        if name != "shift":  # (the shift cancels row by row; its vector is compared above)
            assert np.max(np.abs(R.ld(got) / want - 1)) <= R.tol(E, 1), name
    # step_length and margins: the binding row the last one, and row 1024 * 256 (the first of the second trip there)
    for row, frac in ((NN_BIG - 1, 0.25), (1024 * 256, 0.125)):
        pdz, pds = np.zeros(lay.m), np.zeros(lay.m)
        pdz[nn] = 0.1
        pds[nn] = 0.1
        for side in ("z", "s"):
            a, b = pdz.copy(), pds.copy()
            (a if side == "z" else b)[nn.start + row] = -(z if side == "z" else s)[nn.start + row] / frac
            got = lay.step_length(a, b, z, s, 1.0)
            want = float(R.nn_step_length(a[nn], b[nn], z[nn], s[nn], 1.0))
            print("  NN step_length binding at row %d of %s: %.17g (exact %.17g)" % (row, side, got, want))
            assert abs(want - frac) <= 2 * R.U53 and abs(got - want) <= R.tol(0.0, 1) * want
        zz = z.copy()
        zz[nn.start + row] = -3.0 - frac
        a_ref, b_ref = R.nn_margins(zz[nn])
        b_ref = b_ref + sum(R.ld(float(R.soc_margins(zz[lay.info[k]["rows"]])[1])) for k in (0, 2))
        a, b = lay.margins(zz)
        E = abs(float(np.sum(np.maximum(zz[nn], 0.0)) - R.nn_margins(zz[nn])[1])) / float(b_ref)
        print("  NN margins with the minimum at row %d: %.17g %.17g (exact %.17g)" % (row, a, b, float(b_ref)))
        assert a == -3.0 - frac
        ck("sum of positive parts, minimum at row %d" % row, abs(float(R.ld(b) - b_ref)) / float(b_ref), E, R.tol(E, lay.m))
    small = 0.1 * np.concatenate([R.relative_direction(c66["z"], 1), rng.uniform(-1.0, 1.0, NN_BIG), R.relative_direction(c5["z"], 2)])
    small_s = 0.1 * np.concatenate([R.relative_direction(c66["s"], 3), rng.uniform(-1.0, 1.0, NN_BIG), R.relative_direction(c5["s"], 4)])
    for alpha in (0.0, 0.7):
        want = R.nn_barrier(z[nn], s[nn], small[nn], small_s[nn], alpha)
        scale = np.sum(np.abs(np.log((R.ld(s[nn]) + alpha * R.ld(small_s[nn])) * (R.ld(z[nn]) + alpha * R.ld(small[nn])))))
        for k in (0, 2):
            rows = lay.info[k]["rows"]
            want = want + R.ld(float(R.soc_barrier(z[rows], s[rows], small[rows], small_s[rows], alpha)[0]))
        got = lay.barrier(z, s, small, small_s, alpha)
        dbl = -np.sum(np.log((s[nn] + alpha * small_s[nn]) * (z[nn] + alpha * small[nn])))
        E = abs(float(R.ld(dbl) - R.nn_barrier(z[nn], s[nn], small[nn], small_s[nn], alpha))) / float(scale)
        ck("barrier alpha %.1f over the sum of its terms' magnitudes" % alpha, abs(float(R.ld(got) - want)) / float(scale), E,
           R.tol(E, lay.m, c66["kappa"]))
    bad = small.copy()
    bad[nn.start + NN_BIG - 1] = -2.0 * z[nn.start + NN_BIG - 1]
    assert lay.barrier(z, s, bad, small_s, 0.7) == np.inf
    ck.done()


# ---- 7. the diagonal maximum -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("boost", [258, 3, 1026], ids=["sparse_cone_258", "dense_cone_3", "cone_1026"])
def test_static_regulariser_from_the_diagonal_maximum(hipdev, boost):
    """fold_norm: the cone kernels leave the largest |diagonal entry| they write in slots, the static regulariser is c +
    p max|diag K| (directldlkktsolver.rs:324-329).  On the mixed handle every cone gets late set (1, 1, 0.3) (eta^2 = 1,
    dense diagonals below 101) and ONE cone is scaled s -> 100 s, z -> z / 100, so that its eta^2 = 1e4 carries the
    maximum: a sparse cone's eta^2 (dim 258, registers), a dense cone's eta^2 (2 w_0^2 - 1) (dim 3, read back by thread 0),
    a 1026-row cone's eta^2 (memory-walking body + soc_write_kkt_body).  last_regularizer of both routes equal to each
    other and to the formula on the exact maximum from the reference, within 4 2^-53 plus the error allowed to eta^2."""
    lay = layout(hipdev, MIXED)
    s, z = (v.copy() for v in mixed_inputs(0))
    k = [i for i in lay.socs() if lay.info[i]["dim"] == boost][0]
    rows = lay.info[k]["rows"]
    s[rows] *= 100.0
    z[rows] /= 100.0
    ref = R.mp_scaling(s[rows], z[rows])
    with mp.workdps(R.DPS):
        md = ref.max_diag(lay.info[k]["sparse"])
        others = max(R.late_case(i["dim"], 0)["ref"].max_diag(i["sparse"]) for j, i in enumerate(lay.info) if i["tag"] == SOC and j != k)
        nn_max = max(float(np.max(s[i["rows"]] / z[i["rows"]])) for i in lay.info if i["tag"] == NN)
        assert md >= 1e4 and others <= 101 and nn_max <= 4.0
        assert abs(md / (ref.eta2 if boost > 4 else ref.eta2 * (2 * ref.w[0] ** 2 - 1)) - 1) <= mp.mpf(10) ** -50
    eps_ref = expected_eps(lay, md)
    kap = R.kappa_of(s[rows], z[rows])
    eps = []
    for route in (0, 1):
        assert lay.scale(s, z, route), ROUTES[route]
        eps.append(lay.ks.linear_solver_info().last_regularizer)
        err = abs(eps[-1] - eps_ref) / eps_ref
        allowed = 4 * R.U53 + R.tol(0.0, boost, kap)
        print("  boost dim %d route %d: eps %.17g formula %.17g err %.2e allowed %.2e" % (boost, route, eps[-1], eps_ref, err, allowed))
        assert err <= allowed, ROUTES[route]
        got = -lay.ks.values()[lay.info[k]["hs"]]
        assert R.rel_vec(got, ref.hs_sparse() if boost > 4 else ref.hs_dense()) <= R.tol(0.0, boost, kap)
    assert eps[0] == eps[1]
