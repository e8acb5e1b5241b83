"""References for the second-order and nonnegative cone kernels (clarabel.rs_amd/csrc/cones.hip: k_sym_update_scaling,
k_sym_write_kkt, k_sym_scale_write, k_soc_mul_hs, k_soc_step_ops<0..4>, k_soc_barrier and the k_nn_* kernels) -- test
infrastructure only, used by tests/test_soc_passes_gpu.py and checked on its own by tests/test_soc_ref_host.py.

* an mpmath (60 digits) restatement of SecondOrderCone::update_scaling (socone.rs:134-211: w, eta, lambda and the
  rank-2 terms d, u0, u1, v1), get_Hs (socone.rs:217-246, dense packed triu and sparse diagonal), the expansion columns
  -eta^2 u, -eta^2 v, D = [-eta^2, +eta^2] (datamaps.rs:199-220), mul_Hs (socone.rs:248-256), affine_ds (:258-260),
  combined_ds_shift (symmetric_common.rs:53-84 with :504-530), ds_from_dz_offset (:266-287), step_length by the exact
  roots with the reference's case analysis (:421-495), margins (:104-108) and compute_barrier (:304-314), taking and
  returning what the kernels take and return;
* the nonnegative cone's versions (nonnegativecone.rs:58-166) in numpy longdouble (64-bit mantissa: 2^-11 of a double
  rounding per operation);
* late-iterate pairs `late_pair`: s with Jordan eigenvalues (10^k, 10^-k) along a random unit u, z = mu s^-1 with its
  axis turned by the angle t towards a second direction (none for n = 2);
* exactly representable edge inputs `exact_tail`: tails of a few small integers whose largest is a power of two and
  whose squares sum to a perfect square (3, 4 -> 5; 1, 2, 2 -> 3; ...), or a perfect-square count of ones (1024 ones ->
  32), so that every intermediate of the scaled norm amax sqrt(sum (x / amax)^2) is exact in double in ANY summation
  order; the nonzeros sit at the tail indices a wrong bound would drop (1, the last one, 64, 65, 256, 257, 1024, 1025).

Tolerance: tol(E, n, kappa) = 16 max(E, n 2^-53, kappa 2^-53).  16 and the floor n 2^-53 are psd_ref.tol's.  E is the
error of the DOUBLE restatement in the reference's sequential order (oracle.Cones, the project's C restatement) against
mpmath on the same input.  kappa is the first-order conditioning of the cancelling residual the output depends on,
evaluated in mpmath -- E is ONE draw of a rounding error and another summation order draws another, so E alone can be
far below the typical error (a prototype of w, eta, lambda in two summation orders: a sample E of 4e-14 beside a typical
4e-12; the reordered sum up to 0.24 of 16 E without the kappa floor, at most 0.06 of the tolerance with it):

    output                                                        kappa
    everything downstream of update_scaling (w, eta, lambda, Hs,  max(s0^2 / res(s), z0^2 / res(z)),
      u, v, D, mul_Hs, affine_ds, combined_ds_shift, the static     res(x) = x0^2 - ||x1||^2 = (x0 - ||x1||)(x0 + ||x1||)
      regulariser)
    ds_from_dz_offset(ds, z) and the chain through it             the same (its own residual is res(z) of the same z)
    step_length(dz, ds, z, s)                                     max(x0^2 / res(x), y0^2 / |res(y)|) over (x, y) =
                                                                    (z, dz), (s, ds): the coefficients c and a
    compute_barrier at (z, s) + alpha (dz, ds)                    max(x0^2 / res(x)) of the two shifted arguments; the
                                                                    error is taken absolutely over max(1, |barrier|)
    margins(z), absolutely over z0                                1: ||z1|| is a norm, nothing cancels before the
                                                                    difference, which is measured against z0
    nonnegative rows (w = sqrt(s / z), lambda = sqrt(s z), ...)   1: a few roundings

A late case counts only while E <= E_CAP = 1e-7 (asserted where it is used, so that a regenerated input cannot make a
case vacuous).  Vectors are compared in the relative 2-norm, scalars relatively."""
import functools
import itertools

import mpmath as mp
import numpy as np

DPS = 60
U53 = 2.0 ** -53
LATE_SETS = ((1, 1.0, 0.3), (2, 1e-3, 0.1), (3, 1e-6, 1e-2), (4, 1e-8, 1e-3))  # (k, mu, t)
E_CAP = 1e-7
DIMS = (2, 3, 4, 5, 64, 65, 66, 257, 258, 1025, 1026, 2050)  # (dimension 1 is refused at construction, socone.rs:48)
EDGE_TAIL_INDICES = (1, 64, 65, 256, 257, 1024, 1025)
SOC, NN, ZERO = 2, 1, 0  # SupportedConeT tags of the C ABI


def tol(E, n, kappa=1.0):
    """what a kernel may be off by: E the double restatement's error on the same input, n the length of the longest
    reduction, kappa the conditioning of the residual the output depends on (module docstring)"""
    return 16.0 * max(E, n * U53, kappa * U53)


# ---- mpmath helpers --------------------------------------------------------------------------------------------------
def mpv(x):
    return [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in x]


def mp_dot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def mp_res(x):
    """x0^2 - ||x1||^2 (socone.rs:388-394 without its rounding)"""
    return x[0] * x[0] - mp.fsum(v * v for v in x[1:])


def rel_vec(got, ref):
    """|| got - ref ||_2 / || ref ||_2 with ref a list of mpf (absolute where ref is zero)"""
    with mp.workdps(DPS):
        num = mp.sqrt(mp.fsum((mp.mpf(float(g)) - r) ** 2 for g, r in zip(got, ref)))
        den = mp.sqrt(mp.fsum(r * r for r in ref))
        return float(num / den) if den != 0 else float(num)


def rel_scalar(got, ref):
    with mp.workdps(DPS):
        ref = mp.mpf(ref)
        if not mp.isfinite(ref):
            return 0.0 if float(got) == float(ref) else float("inf")
        d = abs(mp.mpf(float(got)) - ref)
        return float(d / abs(ref)) if ref != 0 else float(d)


def kappa_of(*xs):
    """max x0^2 / |res(x)| over the given vectors, in mpmath"""
    with mp.workdps(DPS):
        out = mp.mpf(1)
        for x in xs:
            x = mpv(x)
            r = abs(mp_res(x))
            out = max(out, x[0] * x[0] / r) if r != 0 else mp.inf
        return float(out)


# ---- the second-order cone in mpmath ---------------------------------------------------------------------------------
class SocScaling:
    """socone.rs:134-211 in 60 digits: w, eta, lam (lists of mpf), d, u0, u1, v1; the inputs s, z as lists of mpf"""

    def __init__(self, s, z):
        with mp.workdps(DPS):
            s, z = mpv(s), mpv(z)
            n = len(s)
            zscale, sscale = mp.sqrt(mp_res(z)), mp.sqrt(mp_res(s))       # :145-146
            self.eta = mp.sqrt(sscale / zscale)                           # :154
            w = [a / sscale for a in s]                                   # :158-161
            w[0] += z[0] / zscale
            for i in range(1, n):
                w[i] -= z[i] / zscale
            wscale = mp.sqrt(mp_res(w))                                   # :163-168
            w = [a / wscale for a in w]
            w1sq = mp.fsum(a * a for a in w[1:])
            w[0] = mp.sqrt(1 + w1sq)                                      # :171-172 (an identity in exact arithmetic)
            g = wscale / 2                                                # :175-184
            ca, cb = (g + z[0] / zscale) / sscale, (g + s[0] / sscale) / zscale
            den = s[0] / sscale + z[0] / zscale + 2 * g
            q = mp.sqrt(sscale * zscale)
            self.lam = [g * q] + [(ca * s[i] + cb * z[i]) / den * q for i in range(1, n)]
            wsq = w[0] * w[0] + w1sq                                      # :189-202
            self.d = 1 / (2 * wsq)
            self.u0 = mp.sqrt(wsq - self.d)
            self.u1 = 2 * w[0] / self.u0
            self.v1 = mp.sqrt(2 * (2 + 1 / wsq) / (2 * wsq - 1 / wsq))
            self.n, self.s, self.z, self.w, self.eta2 = n, s, z, w, self.eta * self.eta

    # -- what update() writes into K (negated where the kernels negate)
    def hs_sparse(self):
        """get_Hs of the sparse form (socone.rs:218-223): the diagonal eta^2 [d, 1, ..., 1]"""
        with mp.workdps(DPS):
            return [self.eta2 * self.d] + [self.eta2] * (self.n - 1)

    def hs_dense(self):
        """get_Hs of the dense form (socone.rs:225-244): packed triu, by columns, of eta^2 (2 w w' - J)"""
        with mp.workdps(DPS):
            w, out = self.w, []
            for col in range(self.n):
                for row in range(col + 1):
                    h = 2 * w[row] * w[col]
                    if row == col:
                        h += -1 if col == 0 else 1
                    out.append(h * self.eta2)
            return out

    def u(self):
        with mp.workdps(DPS):
            return [self.u0] + [self.u1 * a for a in self.w[1:]]

    def v(self):
        with mp.workdps(DPS):
            return [mp.mpf(0)] + [self.v1 * a for a in self.w[1:]]

    def k_columns(self):
        """the sparse expansion as K holds it (datamaps.rs:199-220): -eta^2 u, -eta^2 v, D = [-eta^2, +eta^2]"""
        with mp.workdps(DPS):
            return [-self.eta2 * a for a in self.u()], [-self.eta2 * a for a in self.v()], [-self.eta2, self.eta2]

    def max_diag(self, sparse):
        """the largest |diagonal entry| this cone contributes to K"""
        with mp.workdps(DPS):
            if sparse:
                return max(abs(v) for v in self.hs_sparse() + [self.eta2])
            w = self.w
            return max(abs((2 * w[i] * w[i] + (-1 if i == 0 else 1)) * self.eta2) for i in range(self.n))

    # -- the operations (lists of mpf out)
    def mul_hs(self, x):
        with mp.workdps(DPS):
            x = mpv(x)
            c = 2 * mp_dot(self.w, x)
            return [(c * self.w[i] + (-x[0] if i == 0 else x[i])) * self.eta2 for i in range(self.n)]

    def affine_ds(self):
        with mp.workdps(DPS):
            return circ(self.lam, self.lam)

    def mul_W(self, x):
        with mp.workdps(DPS):
            x, w = mpv(x), self.w
            zeta = mp_dot(w[1:], x[1:])
            c = x[0] + zeta / (1 + w[0])
            return [self.eta * (w[0] * x[0] + zeta)] + [self.eta * (x[i] + c * w[i]) for i in range(1, self.n)]

    def mul_Winv(self, x):
        with mp.workdps(DPS):
            x, w = mpv(x), self.w
            zeta = mp_dot(w[1:], x[1:])
            c = -x[0] + zeta / (1 + w[0])
            return [(w[0] * x[0] - zeta) / self.eta] + [(x[i] + c * w[i]) / self.eta for i in range(1, self.n)]

    def combined_ds_shift(self, step_z, step_s, sigma_mu):
        """-> shift, W dz, W^-1 ds"""
        with mp.workdps(DPS):
            wz, ws = self.mul_W(step_z), self.mul_Winv(step_s)
            sh = circ(ws, wz)
            sh[0] -= mp.mpf(float(sigma_mu))
            return sh, wz, ws

    def ds_from_dz_offset(self, ds, z):
        with mp.workdps(DPS):
            ds, z, w, lam = mpv(ds), mpv(z), self.w, self.lam
            resz = mp_res(z)
            l1d1, w1d1 = mp_dot(lam[1:], ds[1:]), mp_dot(w[1:], ds[1:])
            scale = (lam[0] * ds[0] - l1d1) / resz
            out = [z[0] * scale + self.eta * w1d1]
            out += [-z[i] * scale + self.eta * (ds[i] + w1d1 / (1 + w[0]) * w[i]) for i in range(1, self.n)]
            return [o / lam[0] for o in out]


def circ(y, z):
    """socone.rs:360-367"""
    return [mp_dot(y, z)] + [y[0] * z[i] + z[0] * y[i] for i in range(1, len(y))]


@functools.lru_cache(maxsize=None)
def _scaling_cached(sb, zb):
    return SocScaling(np.frombuffer(sb), np.frombuffer(zb))


def mp_scaling(s, z):
    """the 60-digit scaling of (s, z), cached per input for the session"""
    s, z = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(z, dtype=np.float64)
    return _scaling_cached(s.tobytes(), z.tobytes())


def soc_step_component(x, y, amax):
    """socone.rs:421-495 with exact roots, the reference's case analysis kept"""
    with mp.workdps(DPS):
        x, y, amax = mpv(x), mpv(y), mp.mpf(float(amax))
        if x[0] >= 0 and y[0] < 0:
            amax = min(amax, -x[0] / y[0])
        a = mp_res(y)
        b = 2 * (x[0] * y[0] - mp_dot(x[1:], y[1:]))
        c = max(mp.mpf(0), mp_res(x))
        d = b * b - 4 * a * c
        if (a > 0 and b > 0) or d < 0:
            return amax
        if a == 0:
            return amax
        if c == 0:
            return amax if a >= 0 else mp.mpf(0)
        t = -b - mp.sqrt(d) if b >= 0 else -b + mp.sqrt(d)
        r1, r2 = 2 * c / t, t / (2 * a)
        r1 = mp.inf if r1 < 0 else r1
        r2 = mp.inf if r2 < 0 else r2
        return min(amax, r1, r2)


def soc_step_length(dz, ds, z, s, amax):
    with mp.workdps(DPS):
        return min(soc_step_component(z, dz, amax), soc_step_component(s, ds, amax))


def soc_margins(z):
    with mp.workdps(DPS):
        z = mpv(z)
        a = z[0] - mp.sqrt(mp.fsum(v * v for v in z[1:]))
        return a, max(mp.mpf(0), a)


def soc_barrier(z, s, dz, ds, alpha):
    """-> (barrier, kappa of the two shifted arguments); (+inf, 1) outside the cone"""
    with mp.workdps(DPS):
        a = mp.mpf(float(alpha))
        xs = [[p + a * q for p, q in zip(mpv(x), mpv(dx))] for x, dx in ((s, ds), (z, dz))]
        rs = [mp_res(x) for x in xs]
        if not all(r > 0 for r in rs):  # (the reference tests the residuals only, socone.rs:309)
            return mp.inf, 1.0
        return -mp.log(rs[0] * rs[1]) / 2, float(max(x[0] * x[0] / r for r, x in zip(rs, xs)))


def mp_sqrt_jordan(z):
    """z^(1/2) in the Jordan algebra of the cone, rounded to double: the spectral values sqrt(z0 +- ||z1||)"""
    with mp.workdps(DPS):
        z = mpv(z)
        t = mp.sqrt(mp.fsum(v * v for v in z[1:]))
        lp, lm = mp.sqrt(z[0] + t), mp.sqrt(z[0] - t)
        f = (lp - lm) / (2 * t) if t != 0 else mp.mpf(0)
        return np.array([float((lp + lm) / 2)] + [float(f * v) for v in z[1:]])


def relative_direction(z, seed):
    """dz = P(z^1/2) g with g = (0.1, 0.4 v), |v| = 1: z + alpha dz = P(z^1/2)(e + alpha g) leaves the cone at alpha =
    1 / 0.3, whatever the conditioning of z; det g = -0.15 and the discriminant 4 ||g1||^2 = 0.64 keep the quadratic of
    socone.rs:439-442 away from a = 0 and d = 0.  P(x) = 2 x x' - det(x) J."""
    n = len(z)
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n - 1)
    g = np.concatenate([[0.1], 0.4 * v / np.linalg.norm(v)])
    x = mp_sqrt_jordan(z)
    det = (x[0] - np.linalg.norm(x[1:])) * (x[0] + np.linalg.norm(x[1:]))
    Jg = g.copy()
    Jg[1:] = -Jg[1:]
    return 2.0 * x * (x @ g) - det * Jg


# ---- inputs ------------------------------------------------------------------------------------------------------
def late_pair(n, k, mu, t, seed):
    """(s, z) of a late interior-point iterate of one second-order cone"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(n - 1)
    u /= np.linalg.norm(u)
    a, b = 10.0 ** k, 10.0 ** -k
    s = np.concatenate([[0.5 * (a + b)], 0.5 * (a - b) * u])
    u2 = u
    if n > 2:  # (n = 2: the tail is one number, there is no second direction)
        v = rng.standard_normal(n - 1)
        v -= (v @ u) * u
        v /= np.linalg.norm(v)
        u2 = np.cos(t) * u + np.sin(t) * v
    za, zb = mu / b, mu / a  # the eigenvalues of mu s^-1, along -u
    z = np.concatenate([[0.5 * (za + zb)], -0.5 * (za - zb) * u2])
    return s, z


def late_seed(n, which):
    return 7 * n + LATE_SETS[which][0]


@functools.lru_cache(maxsize=None)
def _exact_values(p):
    """p positive integers, the largest of them 4 (a power of two), whose squares sum to a perfect square: every
    |x| / amax and its square are dyadic with a few bits, so all partial sums are exact in any order"""
    if p == 1:
        return (4,), 4
    for rest in itertools.combinations_with_replacement((1, 2, 3, 4), p - 1):
        ss = 16 + sum(v * v for v in rest)
        r = int(round(ss ** 0.5))
        if r * r == ss:
            return (4,) + rest, r
    raise AssertionError(p)


def edge_indices(n):
    """the tail indices (1-based positions in the cone) a wrong bound would drop, for a cone of n rows"""
    return sorted({i for i in EDGE_TAIL_INDICES + (n - 1,) if 1 <= i <= n - 1})


def exact_tail(n, ones=False):
    """-> (x (n doubles, x[0] = 0), the exact norm of x[1:]).  ones: every tail entry 1 (n - 1 must be a perfect square)"""
    x = np.zeros(n)
    if ones:
        r = int(round((n - 1) ** 0.5))
        assert r * r == n - 1
        x[1:] = 1.0
        return x, float(r)
    idx = edge_indices(n)
    vals, r = _exact_values(len(idx))
    # (the largest value last: at the last index, which a bound `i < n - 1` drops)
    for i, v in zip(idx, sorted(vals)):
        x[i] = float(v)
    return x, float(r)


def has_ones_tail(n):
    r = int(round((n - 1) ** 0.5))
    return r * r == n - 1


# ---- the double restatement, for E -----------------------------------------------------------------------------------
def oracle_cone(n):
    from oracle import oracle as orc
    orc.lib()
    return orc.Cones([(SOC, n)])


def observe_oracle(cone, sparse):
    """the state of a scaled oracle cone as the device shows it (tests/test_soc_passes_gpu.py observe): eta w, J w / eta,
    affine_ds, the Hs block and, for the sparse form, the K columns -eta^2 u, -eta^2 v and D"""
    n = cone.numel
    e0 = np.zeros(n)
    e0[0] = 1.0
    _, wz, ws = cone.combined_ds_shift(e0, e0, 0.0)
    st = cone.state(0)
    out = dict(eta_w=wz, Jw_eta=ws, affine_ds=cone.affine_ds(np.zeros(n)), hs=cone.get_Hs())
    if sparse:
        e2 = st["eta"] * st["eta"]
        out.update(ku=-e2 * np.array(st["u"]), kv=-e2 * np.array(st["v"]), D=np.array([-e2, e2]))
    return out


def reference_state(ref, sparse):
    """the same quantities from the 60-digit scaling"""
    with mp.workdps(DPS):
        out = dict(eta_w=[ref.eta * a for a in ref.w],
                   Jw_eta=[ref.w[0] / ref.eta] + [-a / ref.eta for a in ref.w[1:]],
                   affine_ds=ref.affine_ds(), hs=ref.hs_sparse() if sparse else ref.hs_dense())
        if sparse:
            out["ku"], out["kv"], out["D"] = ref.k_columns()
        return out


@functools.lru_cache(maxsize=None)
def late_case(n, which):
    """-> dict(n, s, z, ref (SocScaling), kappa, state (reference_state), E (dict: the oracle's error per quantity))"""
    k, mu, t = LATE_SETS[which]
    s, z = late_pair(n, k, mu, t, late_seed(n, which))
    ref = mp_scaling(s, z)
    sparse = n > 4
    state = reference_state(ref, sparse)
    cone = oracle_cone(n)
    assert cone.update_scaling(s, z)
    obs = observe_oracle(cone, sparse)
    E = {name: rel_vec(obs[name], state[name]) for name in state}
    return dict(n=n, which=which, s=s, z=z, ref=ref, kappa=kappa_of(s, z), state=state, E=E, cone=cone, sparse=sparse)


# ---- the nonnegative cone in extended precision ---------------------------------------------------------------------
def ld(x):
    return np.asarray(x, dtype=np.longdouble)


class NnScaling:
    """nonnegativecone.rs:77-166 on longdouble copies of the double inputs"""

    def __init__(self, s, z):
        self.s, self.z = ld(s), ld(z)
        self.w, self.lam = np.sqrt(self.s / self.z), np.sqrt(self.s * self.z)

    def hs(self):
        return self.w * self.w

    def mul_hs(self, x):
        return self.w * (self.w * ld(x))

    def affine_ds(self):
        return self.lam * self.lam

    def combined_ds_shift(self, step_z, step_s, sigma_mu):
        wz, ws = self.w * ld(step_z), ld(step_s) / self.w
        return ws * wz - np.longdouble(sigma_mu), wz, ws

    def ds_from_dz_offset(self, ds, z):
        return ld(ds) / ld(z)


def nn_step_length(dz, ds, z, s, amax):
    out = np.longdouble(amax)
    for x, dx in ((z, dz), (s, ds)):
        x, dx = ld(x), ld(dx)
        neg = dx < 0
        if neg.any():
            out = min(out, np.min(-x[neg] / dx[neg]))
    return out


def nn_margins(z):
    z = ld(z)
    return z.min(), np.sum(np.maximum(z, 0))


def nn_barrier(z, s, dz, ds, alpha):
    a = np.longdouble(alpha)
    p = (ld(s) + a * ld(ds)) * (ld(z) + a * ld(dz))
    return np.longdouble(np.inf) if (p <= 0).any() else -np.sum(np.log(p))


def rel_ld(got, ref):
    """|| got - ref ||_2 / || ref ||_2 in longdouble"""
    got, ref = ld(got), ld(ref)
    den = np.sqrt(np.sum(ref * ref))
    num = np.sqrt(np.sum((got - ref) ** 2))
    return float(num / den) if den != 0 else float(num)
