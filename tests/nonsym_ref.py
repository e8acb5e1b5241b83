"""References for the non-symmetric cone kernels (clarabel.rs_amd/csrc/cones.hip: k_ns3_update_scaling, k_ns3_write_hs,
k_ns3_mul_hs, k_ns3_step_ops<0..5>, k_gpw_update_scaling, k_gpw_write_kkt, k_gpw_ops<0..5>) -- test infrastructure only,
used by tests/test_nonsym_passes_gpu.py and checked on its own by tests/test_nonsym_ref_host.py.

* mpmath (60 digits) restatements of the exponential and power cones: the dual gradient and Hessian (expcone.rs:330-353,
  powcone.rs:354-386), the primal gradient (expcone.rs:361-373 through mp.lambertw(e^x); powcone.rs:394-420 through
  mp.findroot on the f of powcone.rs:447-491, and as the reference's one-sided Newton iteration leaves it: ns3_primal_grad), update_scaling for both strategies with the fallback
  (nonsymmetric_common.rs:53-143), get_Hs in the order [00, 01, 11, 02, 12, 22] and mul_Hs (expcone.rs:125-132), affine_ds
  and ds_from_dz_offset (copies, :134-151), combined_ds_shift with the third-order correction and its solve with the dual
  Hessian (expcone.rs:138-147, 256-328; powcone.rs:131-140, 263-352), feasibility (expcone.rs:200-226, powcone.rs:190-224),
  compute_barrier (expcone.rs:175-254, powcone.rs:168-261), unit_initialization (expcone.rs:88-94, powcone.rs:79-87);
* the generalised power cone: update_scaling (genpowcone.rs:360-401: phi, zeta, grad, d1, d2, p, q, r), the K entries
  -mu d1, -mu d2, the columns -sqrt(mu) (q | r | p) and D = [-1, -1, +1] (genpowcone.rs:169-176, datamaps.rs:322-343),
  mul_Hs (:178-202), combined_ds_shift = sigma_mu grad (:208-213), feasibility (:269-310) and compute_barrier (:248-261,
  312-354, 409-441).  compute_barrier is restated AS THE REFERENCE COMPUTES IT: the w part of its primal gradient is
  (g1 / ||s_w||) r with r the cone's vector built from z by update_scaling (genpowcone.rs:427-429), not from s.  Parity with
  the reference is the contract, so the restatement takes r from the scaling too, and the barrier is finite only where
  the w parts of s and z are parallel;
* step_length: the reference's backtracking (nonsymmetric_common.rs:164-192, compositecone.rs:326-337) decided exactly.
  From a0 = min(alpha_max, the symmetric cones' step, 1 - sqrt(eps)) the candidates a0, a0 * 0.8, (a0 * 0.8) * 0.8, ... are
  formed by the double multiplications the kernel performs; the answer is the first candidate at which the shifted
  point is feasible in exact arithmetic, 0.0 once a candidate falls below 1e-4: a double the device returns bit for bit.

Inputs.  late_point(kind, delta, mu, seed): a dual point z whose RELATIVE CONE RESIDUAL is delta -- r / (|z1| + |z0| +
|z0 l|) for the exponential cone (r = z1 - z0 - z0 l, l = log(-z2 / z0)), psi / phi for the power cone (psi = phi - z2^2),
zeta / phi for the generalised power cone (zeta = phi - ||w||^2) -- and s = -mu g*(z) rounded to double, times (1 + 0.1 p_i)
for a fixed p that points into the cone, checked to be primal-interior.  delta = 1 has nothing to cancel: l > 0 for the
exponential cone, z2 = 0 (w = 0) for the power cones.  LATE_SETS = (delta, mu).  The central pair is s = -mu g*(z) rounded,
unperturbed: |de1| is a few ulps against sqrt(eps), the fallback Hs = mu Hd.  Branch points are named for their branch
(BRANCH_POINTS).  GenPow alpha is non-uniform, normalised, the last entry 1 - sum(others); with dim2 > 0 the w parts of s
and z are parallel.

Tolerance: tol(E, n, kappa) = 16 max(E, n 2^-53, kappa 2^-53), soc_ref.tol itself.  E is the error of the project's double
restatement (oracle.Cones; oracle.KKTSolver for the K entries) against mpmath on the same input; kappa the first-order
conditioning, evaluated in mpmath, of the cancelling quantity the output depends on.  For a cone residual it is the
componentwise relative condition number sum_i |q_i d res / d q_i| / |res| of the residual as a function of the point
(ns3_cond): (|z1| + |z0| + |z0 l|) / r for the exponential cone, the reciprocal of the relative residual above, and 2 (phi +
z2^2) / psi, 2 (phi + ||w||^2) / zeta for the power cones, whose terms are homogeneous of degree 2 (about 4 / delta).  For de2
and dot_dsz it is sum |terms| / |value|.

    output                                                      kappa
    Hd, grad, strategy-1 Hs = mu Hd, the fallback Hs, sigma_mu    the cone residual of z: r, psi or zeta (its terms above)
      grad, the third-order correction, mul_Hs, GenPow d1, d2,
      p, q, r and every K entry
    the primal-dual Hs (strategy 0) and mul_Hs with it            additionally de2 = <zt, Hd zt> - 3 mut^2, dot_dsz = <ds, dz>
                                                                    and the primal residual of s
    compute_barrier at (z, s) + alpha (dz, ds)                    the dual residual of the shifted z and the primal residual
                                                                    of the shifted s; absolute error over max(1, |barrier|)
    step_length, unit_initialization                              none: compared bit for bit

Vectors are compared in the relative 2-norm PER CONE, scalars relatively.  Conditions, asserted where they are used: a
late case counts only while E <= E_CAP = 1e-7; every branch decision of the kernel (|de1| against sqrt(eps), |de2| against
eps, dot_dsz > 0, |s2| against eps, the Wright omega split at 1 + pi, the pivots of chol3_factor) is a factor 2^10 from its
threshold in mpmath; the stopping test |dx / x| < sqrt(eps) of the Newton iterations is held to a factor NEWTON_MARGIN = 4
under its own name, because its operand is known to about 1e-15 against a gap of at least 1.1e-8 (newton_onesided);
for every step-length case the exact feasibility function at the accepted candidate and at the rejected one before it is
at least 2^-30 of its largest term from zero.

Measured on the CPU (tests/test_nonsym_ref_host.py prints every figure), largest E of oracle.Cones / oracle.KKTSolver for
the four late sets: exponential and power cones Hs 2.5e-14 / 4.4e-13 / 3.3e-11 / 2.0e-9, Hd 3.5e-16 / 5.1e-14 / 4.6e-12 / 4.5e-10,
mul_Hs 2.9e-14 / 1.2e-12 / 6.1e-11 / 2.3e-8; GenPow K entries 2.3e-16 / 1.6e-13 / 1.9e-11 / 2.9e-9, mul_Hs 1.2e-16 / 3.0e-13 / 3.7e-11 /
5.8e-9: every family meets the cap at delta = 1e-6 for these outputs.  One output does not: the third-order correction
with steps of relative size 0.05, E 1.7e-16 / 2.6e-14 / 1.2e-11 / 1.02e-7 (power cone, pool point 3, alpha 0.2; the other 13 points
1.9e-11 .. 1.2e-8).  Its last set is therefore moved inward to INWARD_SETS = (1e-5, 1e-7), where E is 1.2e-9 at most
(THIRD_ORDER_MOVED_FROM), and every other output is compared at that set as well (Hs 4.9e-10, mul_Hs 4.8e-10).  The smallest
branch margin is 3.4e4; the smallest Newton margin of an input of the GPU file is 23 (the barrier pair of GenPow (3, 300);
2.4e5 for the power cones).
The reference's primal gradient of the power cone is not the conjugate gradient where alpha != 0.5: ns3_primal_grad."""
import functools

import mpmath as mp
import numpy as np

from tests.soc_ref import DPS, mpv, mp_dot, rel_vec, tol  # noqa: F401  (tol is soc_ref.tol itself)

EXP, POW, GENPOW = 3, 4, 5  # SupportedConeT tags of the C ABI
SOC, NN, ZERO = 2, 1, 0
EPS = 2.0 ** -52
LATE_SETS = ((1, 1), (1e-2, 1e-3), (1e-4, 1e-6), (1e-6, 1e-8))  # (delta, mu)
INWARD_SETS = ((1e-5, 1e-7),)  # the last set of the third-order correction, moved inward (THIRD_ORDER_MOVED_FROM)
SETS_OF = {"late": LATE_SETS, "central": LATE_SETS, "inward": INWARD_SETS}
E_CAP = 1e-7
MARGIN = 2.0 ** 10
NEWTON_MARGIN = 4.0  # of the Newton iterations' stopping test from its threshold (newton_onesided says why not 2^10)
STEP_MARGIN = 2.0 ** -30
POOL = 7
POW_ALPHAS = (0.5, 0.1, 0.9, 0.2, 0.6, 0.85, 0.35)  # per pool point, fixed when the handle is created
NS3_SIZES = (1, 42, 43, 255, 256, 257)
GPW_SIZES = ((2, 0), (2, 1), (64, 64), (65, 65), (256, 256), (257, 257), (200, 100), (3, 300), (300, 3), (257, 0))
IDX = ((0, 1, 3), (1, 2, 4), (3, 4, 5))  # packed triu [00, 01, 11, 02, 12, 22]
MIN_STEP, BACKTRACK = 1e-4, 0.8  # Settings: min_terminate_step_length, linesearch_backtrack_step


def mpf(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def kappa_sum(terms):
    """sum |terms| / |sum terms|"""
    tot = mp.fsum(terms)
    return mp.fsum(abs(t) for t in terms) / abs(tot) if tot != 0 else mp.inf


def sym3_mul(H, x):
    return [mp.fsum(H[IDX[i][j]] * x[j] for j in range(3)) for i in range(3)]


def away(value, threshold):
    """how many times |value| is from the positive threshold, as a factor >= 1 on either side"""
    value = abs(value)
    if value == 0:
        return mp.inf
    return max(value / threshold, threshold / value)


# ---- exponential and power cones ---------------------------------------------------------------------------------
def ns3_dual_terms(isexp, a, z):
    """the terms of the dual cone residual of z (positive sum inside the cone)"""
    z = mpv(z)
    if isexp:  # expcone.rs:215-226
        return [z[1], -z[0], -z[0] * mp.log(-z[2] / z[0])]
    a = mpf(a)  # powcone.rs:207-224
    return [(z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a), -z[2] * z[2]]


def ns3_primal_terms(isexp, a, s):
    s = mpv(s)
    if isexp:  # expcone.rs:200-213
        return [s[1] * mp.log(s[2] / s[1]), -s[0]]
    a = mpf(a)  # powcone.rs:190-205
    return [s[0] ** (2 * a) * s[1] ** (2 - 2 * a), -s[2] * s[2]]


def ns3_cond(isexp, dual, a, q):
    """the componentwise relative condition number sum_i |q_i d res / d q_i| / |res| of the cone residual as a function of
    the point.  Exponential cone, dual: (|z1| + |z0| + |z0 l|) / r, the reciprocal of late_point's relative residual;
    primal (res = s1 L - s0, L = log(s2 / s1)): (|s1 (L - 1)| + |s1| + |s0|) / res.  Power cones: phi and z2^2 (||w||^2) are
    homogeneous of degree 2 in their entries, so the sum is 2 (phi + z2^2) / psi, about 4 / delta."""
    q = mpv(q)
    if not isexp:
        terms = ns3_dual_terms(False, a, q) if dual else ns3_primal_terms(False, a, q)
        return 2 * kappa_sum(terms)
    if dual:
        return kappa_sum(ns3_dual_terms(True, a, q))
    L = mp.log(q[2] / q[1])
    return (abs(q[1] * (L - 1)) + abs(q[1]) + abs(q[0])) / abs(q[1] * L - q[0])


def ns3_feasibility(isexp, dual, a, q):
    """-> (feasible, value of the feasibility function / its largest term or None where a sign test decides, the
    smallest |component| a sign test looks at over the largest |component|)"""
    q = mpv(q)
    big = max(abs(v) for v in q)
    if isexp:
        signs = [q[2], -q[0]] if dual else [q[2], q[1]]
    else:
        signs = [q[0], q[1]]
    smin = min(signs) / big if big != 0 else mp.mpf(0)
    if not all(v > 0 for v in signs):
        return False, None, smin
    terms = ns3_dual_terms(isexp, a, q) if dual else ns3_primal_terms(isexp, a, q)
    val = mp.fsum(terms) / max(abs(t) for t in terms)
    return val > 0, val, smin


def ns3_dual_grad_hess(isexp, a, z):
    """-> grad[3], Hd[6] of the dual barrier at z"""
    z = mpv(z)
    if isexp:  # expcone.rs:330-353
        l = mp.log(-z[2] / z[0])
        r = -z[0] * l - z[0] + z[1]
        c2 = 1 / r
        grad = [c2 * l - 1 / z[0], -c2, (c2 * z[0] - 1) / z[2]]
        Hd = [(r * r - z[0] * r + l * l * z[0] * z[0]) / (r * z[0] * z[0] * r), -l / (r * r), 1 / (r * r),
              (z[1] - z[0]) / (r * r * z[2]), -z[0] / (r * r * z[2]), (r * r - z[0] * r + z[0] * z[0]) / (r * r * z[2] * z[2])]
        return grad, Hd
    a = mpf(a)  # powcone.rs:354-386
    phi = (z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a)
    psi = phi - z[2] * z[2]
    g0, g1, g2 = 2 * a * phi / (z[0] * psi), 2 * (1 - a) * phi / (z[1] * psi), -2 * z[2] / psi
    Hd = [g0 * g0 - 2 * a * (2 * a - 1) * phi / (z[0] * z[0] * psi) + (1 - a) / (z[0] * z[0]),
          g0 * g1 - 4 * a * (1 - a) * phi / (z[0] * z[1] * psi),
          g1 * g1 - 2 * (1 - a) * (1 - 2 * a) * phi / (z[1] * z[1] * psi) + a / (z[1] * z[1]),
          g0 * g2, g1 * g2, g2 * g2 + 2 / psi]
    grad = [-g0 - (1 - a) / z[0], -g1 - a / z[1], -g2]
    return grad, Hd


def wright_argument(s):
    """the argument of the Wright omega function of expcone.rs:361-373"""
    s = mpv(s)
    return 1 - s[0] / s[1] - mp.log(s[1] / s[2])


def pow_newton_f(s3, phi, a):
    """f and f' of powcone.rs:447-491"""
    t0 = -2 * a * mp.log(a) - 2 * (1 - a) * mp.log(1 - a)

    def f(x):
        t1, t2 = x * x, 2 * x / s3
        return (2 * a * mp.log(2 * a * t1 + (1 + a) * t2) + 2 * (1 - a) * mp.log(2 * (1 - a) * t1 + (2 - a) * t2)
                - mp.log(phi) - mp.log(t1 + t2) - 2 * mp.log(t2) + t0)

    def df(x):
        return (2 * a * a / (a * x + (1 + a) / s3) + 2 * (1 - a) * (1 - a) / ((1 - a) * x + (2 - a) / s3)
                - 2 * (x + 1 / s3) / (x * x + 2 * x / s3))

    x0 = -1 / s3 + (2 * s3 + mp.sqrt(phi * phi / (s3 * s3) + 3 * phi)) / (phi - s3 * s3)
    return f, df, x0


def newton_onesided(f, df, x0):
    """newton_raphson_onesided (nonsymmetric_common.rs:193-219) carried out in mpmath with the reference's own stopping
    tests -> (the x it returns, the smallest factor by which |dx / x| was from sqrt(eps) at any iterate: the NEWTON
    margin, held to NEWTON_MARGIN = 4 under its own name).  What it returns is the reference's primal gradient, NOT the
    root: the iteration halts at the first step that is not positive without taking it, and it leaves the last step
    below sqrt(eps) |x| untaken.
    Why 4 and not 2^10.  The iteration converges quadratically, so the |dx / x| of successive iterates run through
    1e-2, 1e-4, 1e-8, 1e-16: one of them within 2^10 of sqrt(eps) = 1.5e-8 (1.5e-11 .. 1.5e-5) is the rule, and no choice of
    inputs avoids it.  It need not be avoided.  A factor 4 leaves |dx / x| at least 0.75 sqrt(eps) = 1.1e-8 below the
    threshold or 3 sqrt(eps) above it, while dx / x in double is wrong by about u sum |terms of f| / |x f'| = 1e-15 .. 1e-14
    (f's terms and x f' are of order 1 to 10 here): the double iteration makes the same decision with six orders to
    spare.  The other two tests keep the general margin 2^10, asserted here: |f'| against eps, and dx < eps wherever it
    decides alone (a step that is small but positive is stopped by |dx / x| < sqrt(eps) as well)."""
    x, worst = x0, mp.inf
    for _ in range(100):
        d = df(x)
        dx = -f(x) / d
        assert abs(d) > MARGIN * EPS
        worst = min(worst, away(dx / x, mp.sqrt(EPS)))
        small = abs(dx / x) < mp.sqrt(EPS)
        assert small or dx < -MARGIN * EPS or dx > MARGIN * EPS
        if dx < EPS or small or abs(d) < EPS:
            break
        x += dx
    return x, worst


def ns3_primal_grad(isexp, a, s, exact=False):
    """-> (g(s), the smallest factor of a branch decision from its threshold, the Newton margin of newton_onesided or
    inf where no iteration runs).  Power cone: the reference's starting
    point x0 (powcone.rs:458-459) lies to the RIGHT of the root of its f whenever alpha != 0.5 (f(x0) < 0, against the
    comment of powcone.rs:454-456), so its one-sided Newton iteration halts at once and returns x0: a primal gradient
    up to 0.20 (relative 2-norm: 1.96e-1 at alpha = 0.1, s2 = +-v; tests/test_nonsym_ref_host.py::
    test_conjugate_gradient_identities prints each) from the conjugate gradient.  The kernel and oracle.Cones do the same and parity with the
    reference is the contract, so the restatement follows the reference's iteration in 60 digits (newton_onesided);
    exact=True gives the conjugate gradient itself, through mp.findroot on the same f, for the identities of
    tests/test_nonsym_ref_host.py."""
    s = mpv(s)
    if isexp:  # expcone.rs:361-373; omega(x) = W(e^x)
        x = wright_argument(s)
        om = mp.lambertw(mp.e ** x).real
        g0 = 1 / ((om - 1) * s[1])
        return [g0, g0 + g0 * mp.log(om * s[1] / s[2]) - 1 / s[1], om / ((1 - om) * s[2])], abs(x - (1 + mp.pi)) / EPS, mp.inf
    a = mpf(a)  # powcone.rs:394-420
    if abs(s[2]) > EPS:
        phi = s[0] ** (2 * a) * s[1] ** (2 - 2 * a)
        f, df, x0 = pow_newton_f(abs(s[2]), phi, a)
        g2, newton = newton_onesided(f, df, x0)
        if exact:
            g2 = mp.findroot(f, x0, solver="newton", df=df, tol=mp.mpf(10) ** -100, maxsteps=200)
            assert abs(f(g2)) < mp.mpf(10) ** -50
        assert g2 > 0
        g2 = -g2 if s[2] < 0 else g2
        return [-(a * g2 * s[2] + 1 + a) / s[0], -((1 - a) * g2 * s[2] + 2 - a) / s[1], g2], abs(s[2]) / EPS, newton
    return [-(1 + a) / s[0], -(2 - a) / s[1], mp.mpf(0)], mp.inf if s[2] == 0 else EPS / abs(s[2]), mp.inf


class Ns3Scaling:
    """update_scaling of one exponential or power cone in 60 digits: Hs, Hd (packed 6), grad, and the branch taken"""

    def __init__(self, isexp, a, s, z, mu_in, strategy, exact=False):
        with mp.workdps(DPS):
            self.isexp, self.a = isexp, a
            s, z = mpv(s), mpv(z)
            self.s, self.z = s, z
            self.grad, self.Hd = ns3_dual_grad_hess(isexp, a, z)
            self.kappa = self.kappa_dual = float(ns3_cond(isexp, True, a, z))
            self.margin = self.newton_margin = mp.inf
            if strategy == 1:  # nonsymmetric_common.rs:64-67
                self.branch = "dual"
                self.Hs = [mpf(mu_in) * h for h in self.Hd]
                return
            zt, self.margin, self.newton_margin = ns3_primal_grad(isexp, a, s, exact)
            st, Hd = self.grad, self.Hd
            dot_sz = mp_dot(s, z)
            mu, mut = dot_sz / 3, mp_dot(st, zt) / 3
            ds = [s[i] + mu * st[i] for i in range(3)]
            dz = [z[i] + mu * zt[i] for i in range(3)]
            dot_dsz = mp_dot(ds, dz)
            de1 = mu * mut - 1
            Hzt = sym3_mul(Hd, zt)
            q0 = mp_dot(zt, Hzt)
            de2 = q0 - 3 * mut * mut
            self.mu, self.zt, self.de1, self.de2, self.dot_dsz = mu, zt, de1, de2, dot_dsz
            k_dsz = kappa_sum([a_ * b_ for a_, b_ in zip(ds, dz)])
            assert dot_sz > 0
            if abs(de1) > mp.sqrt(EPS) and abs(de2) > EPS and dot_dsz > 0:  # nonsymmetric_common.rs:99-103
                self.branch = "primal-dual"
                self.margin = min(self.margin, abs(de1) / mp.sqrt(EPS), abs(de2) / EPS, 1 / (k_dsz * EPS))
                self.kappa = float(max(self.kappa, kappa_sum([q0, -3 * mut * mut]), k_dsz,
                                       ns3_cond(isexp, False, a, s)))
                tmp = [mut * st[i] - Hzt[i] for i in range(3)]
                W = list(Hd)
                for i in range(3):
                    for j in range(i, 3):
                        W[IDX[i][j]] -= st[i] * st[j] / 3 + tmp[i] * tmp[j] / de2
                t = mu * mp.sqrt(W[0] ** 2 + W[2] ** 2 + W[5] ** 2 + 2 * (W[1] ** 2 + W[3] ** 2 + W[4] ** 2))
                ax = [z[1] * zt[2] - z[2] * zt[1], z[2] * zt[0] - z[0] * zt[2], z[0] * zt[1] - z[1] * zt[0]]
                nrm = mp.sqrt(mp_dot(ax, ax))
                ax = [v / nrm for v in ax]
                self.Hs = [mp.mpf(0)] * 6
                for i in range(3):
                    for j in range(i, 3):
                        self.Hs[IDX[i][j]] = s[i] * s[j] / dot_sz + ds[i] * ds[j] / dot_dsz + t * ax[i] * ax[j]
            else:  # nonsymmetric_common.rs:138-141
                self.branch = "fallback"
                # (the decision stands while ONE failing test is far on its failing side)
                fails = [away(de1, mp.sqrt(EPS))] if abs(de1) <= mp.sqrt(EPS) else []
                fails += [away(de2, EPS)] if abs(de2) <= EPS else []
                fails += [1 / (k_dsz * EPS)] if dot_dsz <= 0 else []
                self.margin = min(self.margin, max(fails))
                self.Hs = [mu * h for h in Hd]

    def mul_hs(self, x):
        with mp.workdps(DPS):
            return sym3_mul(self.Hs, mpv(x))

    def higher_correction(self, ds, v):
        """expcone.rs:256-328, powcone.rs:263-352 -> (eta, the smallest pivot of the Cholesky factor of Hd over the sum
        of the magnitudes of its terms: chol3_factor's `t <= 0` tests, dense3x3/cholesky.rs:13-57)"""
        with mp.workdps(DPS):
            z, Hd, a = self.z, self.Hd, self.a
            ds, v = mpv(ds), mpv(v)
            u = list(mp.lu_solve(mp.matrix([[Hd[IDX[i][j]] for j in range(3)] for i in range(3)]), mp.matrix(ds)))
            L0 = mp.sqrt(Hd[0])
            L1, L3 = Hd[1] / L0, Hd[3] / L0
            t2 = Hd[2] - L1 * L1
            L2 = mp.sqrt(t2)
            L4 = (Hd[4] - L1 * L3) / L2
            t5 = Hd[5] - L3 * L3 - L4 * L4
            pivot = min(t2 / (abs(Hd[2]) + L1 * L1), t5 / (abs(Hd[5]) + L3 * L3 + L4 * L4))
            if self.isexp:
                eta = [mp.mpf(0), mp.mpf(1), -z[0] / z[2]]
                eta[0] = mp.log(eta[2])
                psi = z[0] * eta[0] - z[0] + z[1]
                dpu, dpv = mp_dot(u, eta), mp_dot(v, eta)
                coef = ((u[0] * (v[0] / z[0] - v[2] / z[2]) + u[2] * (z[0] * v[2] / z[2] - v[0]) / z[2]) * psi
                        - 2 * dpu * dpv) / (psi * psi * psi)
                eta = [e * coef for e in eta]
                ip2 = 1 / (psi * psi)
                eta[0] += ((1 / psi - 2 / z[0]) * u[0] * v[0] / (z[0] * z[0]) - u[2] * v[2] / (z[2] * z[2]) / psi
                           + dpu * ip2 * (v[0] / z[0] - v[2] / z[2]) + dpv * ip2 * (u[0] / z[0] - u[2] / z[2]))
                eta[2] += (2 * (z[0] / psi - 1) * u[2] * v[2] / (z[2] * z[2] * z[2])
                           - (u[2] * v[0] + u[0] * v[2]) / (z[2] * z[2]) / psi
                           + dpu * ip2 * (z[0] * v[2] / (z[2] * z[2]) - v[0] / z[2])
                           + dpv * ip2 * (z[0] * u[2] / (z[2] * z[2]) - u[0] / z[2]))
            else:
                a = mpf(a)
                phi = (z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a)
                psi = phi - z[2] * z[2]
                eta = [2 * a * phi / z[0], 2 * (1 - a) * phi / z[1], -2 * z[2]]
                Hp = [2 * a * (2 * a - 1) * phi / (z[0] * z[0]), 4 * a * (1 - a) * phi / (z[0] * z[1]),
                      2 * (1 - a) * (1 - 2 * a) * phi / (z[1] * z[1]), mp.mpf(0), mp.mpf(0), mp.mpf(-2)]
                dpu, dpv = mp_dot(u, eta), mp_dot(v, eta)
                Hv, Hu = sym3_mul(Hp, v), sym3_mul(Hp, u)
                coef = (mp_dot(u, Hv) * psi - 2 * dpu * dpv) / (psi * psi * psi)
                coef2 = 4 * a * (2 * a - 1) * (1 - a) * phi * (u[0] / z[0] - u[1] / z[1]) * (v[0] / z[0] - v[1] / z[1]) / psi
                ip2 = 1 / (psi * psi)
                eta = [coef * eta[0] - 2 * (1 - a) * u[0] * v[0] / z[0] ** 3 + coef2 / z[0] + Hv[0] * dpu * ip2,
                       coef * eta[1] - 2 * a * u[1] * v[1] / z[1] ** 3 - coef2 / z[1] + Hv[1] * dpu * ip2,
                       coef * eta[2] + Hv[2] * dpu * ip2]
                eta = [dpv * ip2 * Hu[i] + eta[i] for i in range(3)]
            return [e / 2 for e in eta], pivot

    def combined_ds_shift(self, step_z, step_s, sigma_mu):
        """expcone.rs:138-147: shift = sigma_mu grad - eta(ds = step_s, v = step_z) -> (shift, pivot margin)"""
        with mp.workdps(DPS):
            eta, pivot = self.higher_correction(step_s, step_z)
            return [self.grad[i] * mpf(sigma_mu) - eta[i] for i in range(3)], pivot


@functools.lru_cache(maxsize=None)
def _ns3_cached(isexp, a, sb, zb, mu_in, strategy):
    return Ns3Scaling(isexp, a, np.frombuffer(sb), np.frombuffer(zb), mu_in, strategy)


def ns3_scaling(isexp, a, s, z, mu_in, strategy):
    """the 60-digit scaling, cached per input for the session"""
    s, z = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(z, dtype=np.float64)
    return _ns3_cached(bool(isexp), float(a), s.tobytes(), z.tobytes(), float(mu_in), int(strategy))


def ns3_barrier(isexp, a, z, s):
    """compute_barrier of one cone at (z, s) (expcone.rs:228-254, powcone.rs:226-261) -> (barrier, kappa, margin, Newton margin)"""
    with mp.workdps(DPS):
        z, s = mpv(z), mpv(s)
        okz, okp = ns3_feasibility(isexp, True, a, z)[0], ns3_feasibility(isexp, False, a, s)[0]
        if not (okz and okp):
            return mp.inf, 1.0, mp.inf, mp.inf
        kap = float(max(ns3_cond(isexp, True, a, z), ns3_cond(isexp, False, a, s)))
        g, margin, newton = ns3_primal_grad(isexp, a, s)
        if isexp:
            bd = -mp.log(-z[2] * z[0]) - mp.log(mp.fsum(ns3_dual_terms(True, a, z)))
            om = mp.lambertw(mp.e ** wright_argument(s)).real
            bp = -mp.log((om - 1) ** 2 / om) - 2 * mp.log(s[1]) - mp.log(s[2]) - 3
        else:
            a = mpf(a)
            bd = -mp.log(mp.fsum(ns3_dual_terms(False, a, z))) - (1 - a) * mp.log(z[0]) - a * mp.log(z[1])
            bp = (mp.log(mp.fsum(ns3_dual_terms(False, a, [-g[0], -g[1], g[2]]))) + (1 - a) * mp.log(-g[0])
                  + a * mp.log(-g[1]) - 3)
        return bd + bp, kap, margin, newton


def ns3_unit(isexp, a):
    """expcone.rs:88-94 / powcone.rs:79-87 in double: the constants, and correctly rounded square roots"""
    if isexp:
        return np.array([-1.051383945322714, 0.556409619469370, 1.258967884768947])
    return np.array([np.sqrt(1.0 + a), np.sqrt(1.0 + (1.0 - a)), 0.0])


# ---- the generalised power cone ----------------------------------------------------------------------------------
def gpw_terms(alpha, q, dual):
    """[prod (q_k / alpha_k)^(2 alpha_k) (dual) or prod q_k^(2 alpha_k), -||w||^2] (genpowcone.rs:269-310)"""
    d1 = len(alpha)
    q = mpv(q)
    phi = mp.exp(mp.fsum(2 * mpf(a) * mp.log(x / mpf(a) if dual else x) for a, x in zip(alpha, q[:d1])))
    return [phi, -mp.fsum(x * x for x in q[d1:])]


def gpw_feasibility(alpha, dual, q):
    q = mpv(q)
    d1 = len(alpha)
    big = max(abs(v) for v in q)
    smin = min(q[:d1]) / big
    if not all(v > 0 for v in q[:d1]):
        return False, None, smin
    terms = gpw_terms(alpha, q, dual)
    val = mp.fsum(terms) / max(abs(t) for t in terms)
    return val > 0, val, smin


class GpwScaling:
    """genpowcone.rs:360-401 in 60 digits"""

    def __init__(self, alpha, d2, z, mu):
        with mp.workdps(DPS):
            al = self.alpha = [mpf(a) for a in alpha]
            d1 = self.d1n = len(al)
            self.d2n, self.mu = d2, mpf(mu)
            z = self.z = mpv(z)
            assert len(z) == d1 + d2
            terms = gpw_terms(alpha, z, True)
            phi, norm2w = terms[0], -terms[1]
            zeta = phi - norm2w
            assert zeta > 0
            self.phi, self.zeta, self.kappa = phi, zeta, float(2 * kappa_sum(terms))  # (ns3_cond: degree 2)
            tau = [2 * a / x for a, x in zip(al, z[:d1])]
            self.grad = [-t * phi / zeta - (1 - a) / x for t, a, x in zip(tau, al, z[:d1])] + [2 / zeta * w for w in z[d1:]]
            p0 = mp.sqrt(phi * (phi + norm2w) / 2)
            p1, q0, r1 = -2 * phi / p0, mp.sqrt(zeta * phi / 2), 2 * mp.sqrt(zeta / (phi + norm2w))
            self.d1 = [t * phi / (zeta * x) + (1 - a) / (x * x) for t, a, x in zip(tau, al, z[:d1])]
            self.d2 = 2 / zeta
            self.p = [p0 / zeta * t for t in tau] + [p1 / zeta * w for w in z[d1:]]
            self.q = [q0 / zeta * t for t in tau]
            self.r = [r1 / zeta * w for w in z[d1:]]

    def k_entries(self):
        """-> dict(diag = -mu [d1, d2 ...], q, r, p = -sqrt(mu) (q | r | p), D = [-1, -1, +1]) (datamaps.rs:322-343)"""
        with mp.workdps(DPS):
            sm = -mp.sqrt(self.mu)
            return dict(diag=[-self.mu * d for d in self.d1] + [-self.mu * self.d2] * self.d2n,
                        q=[sm * v for v in self.q], r=[sm * v for v in self.r], p=[sm * v for v in self.p],
                        D=[mp.mpf(-1), mp.mpf(-1), mp.mpf(1)])

    def mul_hs(self, x):
        """genpowcone.rs:178-202: mu (D x + p p'x - q q'x - r r'x)"""
        with mp.workdps(DPS):
            x, d1 = mpv(x), self.d1n
            cp, cq, cr = mp_dot(self.p, x), mp_dot(self.q, x[:d1]), mp_dot(self.r, x[d1:])
            y = [self.d1[k] * x[k] - cq * self.q[k] for k in range(d1)]
            y += [self.d2 * x[d1 + k] - cr * self.r[k] for k in range(self.d2n)]
            return [(cp * self.p[k] + y[k]) * self.mu for k in range(d1 + self.d2n)]

    def shift(self, sigma_mu):
        with mp.workdps(DPS):
            return [g * mpf(sigma_mu) for g in self.grad]

    def barrier(self, z, s):
        """compute_barrier at (z, s) with THIS scaling's r in the primal gradient (genpowcone.rs:427-429; module
        docstring) -> (barrier, kappa, margin of norm_r > eps, Newton margin)"""
        with mp.workdps(DPS):
            z, s, al, d1 = mpv(z), mpv(s), self.alpha, self.d1n
            if not (gpw_feasibility(self.alpha, True, z)[0] and gpw_feasibility(self.alpha, False, s)[0]):
                return mp.inf, 1.0, mp.inf, mp.inf
            kap = float(2 * max(kappa_sum(gpw_terms(al, z, True)), kappa_sum(gpw_terms(al, s, False))))
            bd = self._barrier_dual(z)
            g, margin, newton = gpw_primal_grad(al, s, self.r)
            mg = [-v for v in g]
            t = gpw_terms(al, mg, True)
            if mp.fsum(t) <= 0:
                return -mp.inf, kap, margin, newton  # (-g(s) outside the dual cone: the reference's -log of a negative number)
            kap = max(kap, float(2 * kappa_sum(t)))
            return -self._barrier_dual(mg) - (d1 + 1) + bd, kap, margin, newton

    def _barrier_dual(self, z):
        d1 = self.d1n
        return -mp.log(mp.fsum(gpw_terms(self.alpha, z, True))) - mp.fsum(mp.log(x) * (1 - a) for x, a in zip(z[:d1], self.alpha))


def gpw_primal_grad(alpha, s, w_dir=None, exact=False):
    """the primal gradient of genpowcone.rs:409-441 -> (g, margin of norm_r > eps, Newton margin).  w_dir: the vector the
    reference scales by g1 / ||s_w|| for the w part -- the cone's r (genpowcone.rs:427-429); None: s_w itself, which is
    the conjugate gradient's.  exact=True solves the root of the reference's f with mp.findroot instead of taking the
    reference's one-sided Newton iterate"""
    al, s = [mpf(a) for a in alpha], mpv(s)
    d1 = len(al)
    w_dir = s[d1:] if w_dir is None else w_dir
    norm_r = mp.sqrt(mp.fsum(x * x for x in s[d1:]))
    if not norm_r > EPS:
        return ([-(1 + a) / p for a, p in zip(al, s[:d1])] + [mp.mpf(0)] * (len(s) - d1),
                mp.inf if norm_r == 0 else EPS / norm_r, mp.inf)
    phi = gpw_terms(al, s, False)[0]
    psi = 1 / mp.fsum(a * a for a in al)

    def f(x):
        return (-mp.log(2 * x / norm_r + x * x)
                + mp.fsum(2 * a * (mp.log(x * norm_r + (1 + a) / a) - mp.log(p)) for a, p in zip(al, s[:d1])))

    def df(x):
        return (-(2 * x + 2 / norm_r) / (x * x + 2 * x / norm_r)
                + mp.fsum(2 * a * norm_r / (norm_r * x + (1 + a) / a) for a in al))

    x0 = -1 / norm_r + (psi * norm_r + mp.sqrt((phi / norm_r / norm_r + psi * psi - 1) * phi)) / (phi - norm_r * norm_r)
    g1, newton = newton_onesided(f, df, x0)  # (the reference's iterate, as for the power cone)
    if exact:
        g1 = mp.findroot(f, x0, solver="newton", df=df, tol=mp.mpf(10) ** -100, maxsteps=200)
        assert abs(f(g1)) < mp.mpf(10) ** -50
    assert g1 > 0
    g = [-(1 + a + a * g1 * norm_r) / p for a, p in zip(al, s[:d1])] + [g1 / norm_r * r for r in w_dir]
    return g, norm_r / EPS, newton


@functools.lru_cache(maxsize=None)
def _gpw_cached(ab, d2, zb, mu):
    return GpwScaling(np.frombuffer(ab), d2, np.frombuffer(zb), mu)


def gpw_scaling(alpha, d2, z, mu):
    alpha, z = np.ascontiguousarray(alpha, dtype=np.float64), np.ascontiguousarray(z, dtype=np.float64)
    return _gpw_cached(alpha.tobytes(), int(d2), z.tobytes(), float(mu))


def gpw_unit(alpha, d2):
    return np.concatenate([np.sqrt(1.0 + np.asarray(alpha)), np.zeros(d2)])


# ---- step_length -------------------------------------------------------------------------------------------------
def first_candidate(alpha_max, sym_step=np.inf):
    """compositecone.rs:329-330, in double as kkt_cones.cpp (KktCones::step_length) forms it"""
    return min(min(float(alpha_max), float(sym_step)), 1.0 - np.sqrt(EPS))


def backtrack(feas, q, dq, a0):
    """nonsymmetric_common.rs:164-192 with the feasibility decided exactly -> (the candidate (a double), the smallest
    margin seen at the accepted candidate and at the rejected one before it).  feas(point) -> (bool, value / largest
    term or None, the sign tests' margin)"""
    with mp.workdps(DPS):
        q, dq = mpv(q), mpv(dq)
        al, prev = float(a0), None
        while True:
            ok, val, smin = feas([x + mpf(al) * d for x, d in zip(q, dq)])
            m = abs(val) if val is not None else abs(smin)
            if val is not None:
                m = min(m, abs(smin))
            if ok:
                return al, float(m if prev is None else min(m, prev))
            prev = m
            al = al * BACKTRACK  # the kernel's own double multiplication
            if al < MIN_STEP:
                return 0.0, float(prev)


def ns3_step(isexp, a, dz, ds, z, s, a0):
    """-> (min of the dual and the primal backtracking, margin) for one cone (expcone.rs:153-173)"""
    az, mz = backtrack(lambda p: ns3_feasibility(isexp, True, a, p), z, dz, a0)
    as_, ms = backtrack(lambda p: ns3_feasibility(isexp, False, a, p), s, ds, a0)
    return min(az, as_), min(mz, ms)


def gpw_step(alpha, dz, ds, z, s, a0):
    az, mz = backtrack(lambda p: gpw_feasibility(alpha, True, p), z, dz, a0)
    as_, ms = backtrack(lambda p: gpw_feasibility(alpha, False, p), s, ds, a0)
    return min(az, as_), min(mz, ms)


def step_boundary_bisect(feas, q, dq, hi):
    """the exact crossing of the cone's boundary along q + t dq in (0, hi) by bisection (feasible at 0, not at hi)"""
    with mp.workdps(DPS):
        q, dq = mpv(q), mpv(dq)
        lo, hi = mp.mpf(0), mpf(hi)
        for _ in range(120):
            mid = (lo + hi) / 2
            if feas([x + mid * d for x, d in zip(q, dq)])[0]:
                lo = mid
            else:
                hi = mid
        return lo


# ---- inputs ------------------------------------------------------------------------------------------------------
P3 = {True: (0.0, 0.0, 1.0), False: (1.0, 0.5, -1.0)}  # the fixed perturbation of s: into the cone (module docstring)


def _round(v):
    return np.array([float(x) for x in v])


@functools.lru_cache(maxsize=None)
def ns3_dual_point(isexp, a, delta, seed):
    """a dual-interior z of relative cone residual delta"""
    rng = np.random.default_rng(1000 * seed + (17 if isexp else 29))
    if isexp:
        z0 = -rng.uniform(0.5, 2.0)
        if delta >= 1:  # every term of r positive: l > 0
            return np.array([z0, rng.uniform(0.5, 2.0), -z0 * np.exp(rng.uniform(0.3, 1.5))])
        l = -rng.uniform(1.5, 3.0)
        z2 = float(-z0 * np.exp(l))
        with mp.workdps(DPS):
            T = abs(mpf(z0) * mp.log(-mpf(z2) / mpf(z0)))
            d = mpf(delta)
            z1 = float(T * (1 + d) / (1 - d) - abs(mpf(z0)))
        return np.array([z0, z1, z2])
    z0, z1 = rng.uniform(0.5, 2.0, 2)
    sign = 1.0 if seed % 2 == 0 else -1.0
    with mp.workdps(DPS):
        phi = ns3_dual_terms(False, a, [z0, z1, 0.0])[0]
        z2 = sign * float(mp.sqrt(phi * (1 - mpf(delta))))
    return np.array([z0, z1, z2])


def relative_residual(terms):
    with mp.workdps(DPS):
        if len(terms) == 3:  # the exponential cone: r / (|z1| + |z0| + |z0 l|)
            return float(mp.fsum(terms) / mp.fsum(abs(t) for t in terms))
        return float(mp.fsum(terms) / terms[0])  # psi / phi, zeta / phi


@functools.lru_cache(maxsize=None)
def late_point(kind, delta, mu, seed, central=False):
    """kind: EXP or POW -> dict(isexp, a, s, z, mu, delta: the relative residual z really has)"""
    isexp = kind == EXP
    a = 0.5 if isexp else POW_ALPHAS[seed % POOL]
    z = ns3_dual_point(isexp, a, delta, seed)
    with mp.workdps(DPS):
        grad, _ = ns3_dual_grad_hess(isexp, a, z)
        s = _round([-mpf(mu) * g for g in grad])
        if not central:
            s = s * (1.0 + 0.1 * np.array(P3[isexp]))
        ok, val, _ = ns3_feasibility(isexp, False, a, s)
        assert ok, (kind, delta, mu, seed)
        got = relative_residual(ns3_dual_terms(isexp, a, z))
        assert 0.5 * delta <= got <= 2.0 * delta, (got, delta)
    return dict(isexp=isexp, a=a, s=s, z=z, mu=mu, delta=got, tag=kind)


def _exp_s_with_wright_argument(x, seed):
    rng = np.random.default_rng(seed)
    s1, s2 = rng.uniform(0.5, 2.0, 2)
    s0 = s1 * (1.0 - x - np.log(s1 / s2))
    return np.array([s0, s1, s2])


def _pair_from_s(isexp, a, s, mu):
    """z = -mu g(s) rounded, times (1 + 0.1 p') into the dual cone"""
    with mp.workdps(DPS):
        g = ns3_primal_grad(isexp, a, s)[0]
        z = _round([-mpf(mu) * v for v in g])
    z = z * (1.0 + 0.1 * np.array((0.0, 0.0, 1.0) if isexp else (1.0, 0.5, -1.0)))
    with mp.workdps(DPS):
        assert ns3_feasibility(isexp, True, a, z)[0] and ns3_feasibility(isexp, False, a, s)[0]
    return dict(isexp=isexp, a=a, s=np.asarray(s, dtype=np.float64), z=z, mu=mu, delta=None, tag=EXP if isexp else POW)


@functools.lru_cache(maxsize=None)
def branch_point(name, seed=0):
    """the inputs named for the branch they take; `seed` picks one of POOL variants"""
    mu = 0.5
    if name == "exp wright series below 1 + pi":
        return _pair_from_s(True, 0.5, _exp_s_with_wright_argument(1.3 + 0.3 * seed, 50 + seed), mu)
    if name == "exp wright asymptotic above 1 + pi":
        return _pair_from_s(True, 0.5, _exp_s_with_wright_argument(5.0 + 1.5 * seed, 60 + seed), mu)
    rng = np.random.default_rng(70 + seed)
    s0, s1 = rng.uniform(0.5, 2.0, 2)
    if name == "pow s2 = 0":
        return _pair_from_s(False, POW_ALPHAS[seed % POOL], np.array([s0, s1, 0.0]), mu)
    if name in ("pow s2 = +v", "pow s2 = -v"):
        a = POW_ALPHAS[seed % POOL]
        v = 0.6 * s0 ** a * s1 ** (1.0 - a)
        return _pair_from_s(False, a, np.array([s0, s1, v if name.endswith("+v") else -v]), mu)
    if name == "pow alpha away from 0.5":
        # (alpha belongs to the handle: the pool's.  Points 1 .. 6 are 0.1 or more from 0.5 and halt the reference's Newton
        # iteration at its starting point; point 0, alpha = 0.5, is the one that iterates: ns3_primal_grad)
        a = POW_ALPHAS[seed % POOL]
        return _pair_from_s(False, a, np.array([s0, s1, 0.4 * s0 ** a * s1 ** (1.0 - a)]), mu)
    raise KeyError(name)


BRANCH_POINTS = {EXP: ("exp wright series below 1 + pi", "exp wright asymptotic above 1 + pi"),
                 POW: ("pow s2 = 0", "pow s2 = +v", "pow s2 = -v", "pow alpha away from 0.5")}
# the branch every cone of a set takes under strategy 0 (asserted by both test files; the branch points take several)
STRATEGY0_BRANCH = {"late": "primal-dual", "inward": "primal-dual", "central": "fallback"}
# the sets of inputs of a whole handle: every cone of kind K takes its point from the set's list for K, cyclically
NS3_SETS = tuple("late %d" % k for k in range(len(LATE_SETS))) + ("inward 0", "central 0", "central 1", "branch 0", "branch 1", "branch 2", "branch 3")


def ns3_pool_point(set_name, kind, j):
    """pool point j (0 .. POOL - 1) of `kind` for the named set"""
    what, k = set_name.split()
    k = int(k)
    if what in SETS_OF:
        return late_point(kind, SETS_OF[what][k][0], SETS_OF[what][k][1], j, central=what == "central")
    names = BRANCH_POINTS[kind]
    return branch_point(names[k % len(names)], j)


def ns3_handle_points(ncones, set_name):
    """exp and pow cones alternate; cone c takes pool point c mod 7 of its kind (7 is coprime to 2, 6 and 256)"""
    return [ns3_pool_point(set_name, EXP if c % 2 == 0 else POW, c % POOL) for c in range(ncones)]


def ns3_specs(ncones):
    return [(EXP, 3) if c % 2 == 0 else (POW, 3, 0, POW_ALPHAS[c % POOL]) for c in range(ncones)]


@functools.lru_cache(maxsize=None)
def gpw_alpha(d1, seed):
    rng = np.random.default_rng(500 + 13 * d1 + seed)
    a = rng.uniform(0.2, 1.0, d1)
    a /= a.sum()
    a[-1] = 1.0 - a[:-1].sum()
    assert (a > 0).all() and len(set(a)) == d1
    return a


@functools.lru_cache(maxsize=None)
def gpw_point(d1, d2, delta, mu, seed=0, central=False):
    """-> dict(alpha, d1, d2, s, z, mu, delta): z of zeta / phi = delta (w = 0 at delta = 1), s = -mu g*(z) rounded, its
    first d1 entries times (1 + 0.1 p_k), p_k in (0.2, 1], its w part times 0.95 (parallel to that of z)"""
    alpha = gpw_alpha(d1, seed)
    rng = np.random.default_rng(900 + 31 * d1 + 7 * d2 + seed)
    u = rng.uniform(0.8, 2.0, d1)
    wdir = rng.standard_normal(d2)
    with mp.workdps(DPS):
        phi = gpw_terms(alpha, list(u) + [0.0] * d2, True)[0]
        nw = mp.sqrt(phi * (1 - mpf(delta))) if d2 else mp.mpf(0)
        if d2:
            wdir = wdir / np.linalg.norm(wdir)
        z = np.concatenate([u, _round([nw * mpf(w) for w in wdir])])
        ref = GpwScaling(alpha, d2, z, mu)
        s = _round([-mpf(mu) * g for g in ref.grad])
        if not central:
            p = 0.2 + 0.8 * ((np.arange(d1) * 5) % 7) / 6.0
            s[:d1] *= 1.0 + 0.1 * p
            s[d1:] *= 0.95
        assert gpw_feasibility(alpha, False, s)[0]
        got = relative_residual(gpw_terms(alpha, z, True))
        assert (d2 == 0 and got == 1.0) or 0.5 * delta <= got <= 2.0 * delta, (got, delta)
    return dict(alpha=alpha, d1=d1, d2=d2, s=s, z=z, mu=mu, delta=got, tag=GENPOW)


def gpw_spec(d1, d2, seed=0):
    return (GENPOW, d1, d2, list(gpw_alpha(d1, seed)))


# ---- the double restatement, for E -------------------------------------------------------------------------------
def oracle_mod():
    from oracle import oracle as orc
    orc.lib()
    return orc


def ns3_oracle(pt, mu_in, strategy):
    """oracle.Cones of the one cone, scaled"""
    cone = oracle_mod().Cones([(EXP, 3) if pt["isexp"] else (POW, 3, 0, pt["a"])])
    assert cone.update_scaling(pt["s"], pt["z"], mu_in, strategy)
    return cone


def ns3_state_E(pt, mu_in, strategy):
    """-> (ref, cone, dict(Hs, Hd, grad: the oracle's error))"""
    ref = ns3_scaling(pt["isexp"], pt["a"], pt["s"], pt["z"], mu_in, strategy)
    cone = ns3_oracle(pt, mu_in, strategy)
    st = cone.state(0)
    E = dict(Hs=rel_vec(st["Hs3"], ref.Hs), Hd=rel_vec(st["Hdual"], ref.Hd), grad=rel_vec(st["grad3"], ref.grad))
    return ref, cone, E


class GpwOracle:
    """oracle.Cones + oracle.KKTSolver of the one cone on n = 1, P = [1], A = a dense column of ones"""

    def __init__(self, pt):
        orc = oracle_mod()
        m = pt["d1"] + pt["d2"]
        self.m, self.pt = m, pt
        self.cones = orc.Cones([(GENPOW, pt["d1"], pt["d2"], list(pt["alpha"]))])
        P = ([0, 1], [0], [1.0])
        A = ([0, m], list(range(m)), [1.0] * m)
        self.kkt = orc.KKTSolver(1, m, P, A, self.cones)

    def k_entries(self, mu):
        pt = self.pt
        assert self.cones.update_scaling(pt["s"], pt["z"], mu, 1) and self.kkt.update()
        return gpw_read_k(np.array(self.kkt.kkt.nzval), np.array(self.kkt.kkt.colptr), 1, 1 + self.m, pt["d1"], pt["d2"])


def gpw_read_k(vals, cp, row0, col, d1, d2):
    """a GenPow cone's entries of the upper-triangular CSC K: rows row0 .. of the KKT matrix, extra columns col .. col + 2"""
    diag = np.array([vals[cp[row0 + k + 1] - 1] for k in range(d1 + d2)])
    return dict(diag=diag, q=vals[cp[col]:cp[col] + d1], r=vals[cp[col + 1]:cp[col + 1] + d2],
                p=vals[cp[col + 2]:cp[col + 2] + d1 + d2],
                D=np.array([vals[cp[col + 1] - 1], vals[cp[col + 2] - 1], vals[cp[col + 3] - 1]]))


# ---- the cases of tests/test_nonsym_passes_gpu.py, per pool point (checked by tests/test_nonsym_ref_host.py) ------
SIGMA_MU = 0.37
STEP_REL = 0.05
# the third-order correction cannot meet E_CAP at delta = 1e-6: a step of relative size 0.05 is 5e4 times the distance to
# the boundary, eta grows like 1 / psi^3, and the error E of oracle.Cones itself reached 1.02e-7 there (power cone, pool
# point 3).  So for this output the last set is INWARD_SETS[0] = (1e-5, 1e-7), the set "inward 0", where its E is 1.2e-9 at
# most (1.1e-13 .. 1.2e-9 over the 14 pool points); the sets named here run every output but this one.
THIRD_ORDER_MOVED_FROM = ("late 3",)


def set_mu_in(set_name):
    """the mu passed to update_scaling: NOT <s, z> / 3 of any pair, so that mu_in Hd (strategy 1) and mu Hd (the
    fallback of strategy 0) are different numbers"""
    what, k = set_name.split()
    return 1.7 * SETS_OF[what][int(k)][1] if what in SETS_OF else 0.9


def pool_vectors(kind, j, s, z):
    """the fixed vectors of pool point j: x for mul_Hs, steps of relative size 0.05 for the third-order correction"""
    rng = np.random.default_rng(300 + 10 * j + kind)
    x = rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    step_z = STEP_REL * np.abs(z) * rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    step_s = STEP_REL * np.abs(s) * rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    return x, step_z, step_s


@functools.lru_cache(maxsize=None)
def ns3_case(set_name, kind, j, strategy):
    """-> dict(pt, ref (Ns3Scaling), branch, kappa, margin, refs: Hs, Hd, grad (sigma_mu grad), mul_hs, shift (with the
    third-order correction), E: the oracle's error per output, x, step_z, step_s, sigma_mu)"""
    pt = ns3_pool_point(set_name, kind, j)
    mu_in = set_mu_in(set_name)
    ref, cone, E = ns3_state_E(pt, mu_in, strategy)
    x, step_z, step_s = pool_vectors(kind, j, pt["s"], pt["z"])
    with mp.workdps(DPS):
        sg = [g * mpf(SIGMA_MU) for g in ref.grad]
        refs = dict(Hs=ref.Hs, Hd=ref.Hd, grad=sg, mul_hs=ref.mul_hs(x))
        pivot = mp.inf
        if set_name not in THIRD_ORDER_MOVED_FROM:
            refs["shift"], pivot = ref.combined_ds_shift(step_z, step_s, SIGMA_MU)
    zero = np.zeros(3)
    E = dict(E)
    E["grad"] = rel_vec(cone.combined_ds_shift(zero, zero, SIGMA_MU)[0], sg)
    E["mul_hs"] = rel_vec(cone.mul_Hs(x), refs["mul_hs"])
    if "shift" in refs:
        E["shift"] = rel_vec(cone.combined_ds_shift(step_z, step_s, SIGMA_MU)[0], refs["shift"])
    return dict(pt=pt, ref=ref, branch=ref.branch, kappa=ref.kappa, kappa_dual=ref.kappa_dual,
                margin=float(min(ref.margin, pivot / EPS)), newton_margin=float(ref.newton_margin), refs=refs, E=E, x=x, step_z=step_z, step_s=step_s, mu_in=mu_in)


def ns3_kappa_of(case, name):
    """the kappa of the module docstring's table for the output `name`"""
    return case["kappa"] if name in ("Hs", "mul_hs") else case["kappa_dual"]


def tile_cones(ncones, per_point):
    """the handle's m-vector from per-pool-point 3-vectors: per_point(kind, j) -> 3 doubles"""
    return np.concatenate([per_point(EXP if c % 2 == 0 else POW, c % POOL) for c in range(ncones)])


# step_length: directions along the rays of the pair, d = c q, plus noise of relative size 0.02, on the benign sets
STEP_SETS = ("late 0", "branch 1")
STEP_CASES = ("stays feasible", "backtracks", "ends at 0", "last cone limits")


def ns3_step_direction(pt, kind, j, coef, side):
    """-> (dz, ds): coef times the point on `side` ("z" or "s"), + 0.1 of the point on the other, + noise"""
    rng = np.random.default_rng(700 + 10 * j + kind)
    out = []
    for name in ("z", "s"):
        q = pt[name]
        c = coef if name == side else 0.1
        out.append(c * q + 0.02 * np.abs(q) * rng.uniform(-1.0, 1.0, 3))
    return out


def ns3_step_case(ncones, set_name, case):
    """-> (dz, ds, z, s, alpha_max, per-cone coefficients).  -2.2 q: feasible below 1 / 2.2 = 0.4545, between the candidates
    0.512 a0 and 0.4096 a0; -1e5 q: every candidate down to 1e-4 is outside"""
    pts = ns3_handle_points(ncones, set_name)
    coefs = []
    for c in range(ncones):
        if case == "stays feasible":
            coefs.append(0.3)
        elif case == "backtracks":
            coefs.append(-2.2 if c % 3 == 0 else 0.3)
        elif case == "ends at 0":
            coefs.append(-1e5 if c == ncones // 2 else -2.2)
        else:
            coefs.append(-2.2 if c == ncones - 1 else 0.3)
    dz, ds = [], []
    for c, pt in enumerate(pts):
        a, b = ns3_step_direction(pt, pt["tag"], c % POOL, coefs[c], "z" if (c // 2) % 2 == 0 else "s")
        dz.append(a)
        ds.append(b)
    z, s = np.concatenate([p["z"] for p in pts]), np.concatenate([p["s"] for p in pts])
    return np.concatenate(dz), np.concatenate(ds), z, s, 1.0, coefs


@functools.lru_cache(maxsize=None)
def _ns3_step_cached(isexp, a, dzb, dsb, zb, sb, a0):
    f = np.frombuffer
    return ns3_step(isexp, a, f(dzb), f(dsb), f(zb), f(sb), a0)


def ns3_step_expected(ncones, set_name, case, sym_step=np.inf):
    """-> (the expected double, the smallest margin over the cones)"""
    dz, ds, z, s, amax, _ = ns3_step_case(ncones, set_name, case)
    pts = ns3_handle_points(ncones, set_name)
    a0 = first_candidate(amax, sym_step)
    out, margin = a0, np.inf
    for c, pt in enumerate(pts):
        r = slice(3 * c, 3 * c + 3)
        al, m = _ns3_step_cached(pt["isexp"], pt["a"], dz[r].tobytes(), ds[r].tobytes(), z[r].tobytes(), s[r].tobytes(), a0)
        out, margin = min(out, al), min(margin, m)
    return out, margin


BARRIER_SETS = ("late 0", "branch 1", "branch 3")  # (steps of relative size 0.05 leave the cone from delta = 1e-2 on)
BARRIER_ALPHAS = (0.0, 0.3)


@functools.lru_cache(maxsize=None)
def ns3_barrier_case(set_name, kind, j, alpha):
    """-> (barrier of pool point j at (z, s) + alpha (dz, ds), kappa, margin, Newton margin) with the third-order steps as directions"""
    pt = ns3_pool_point(set_name, kind, j)
    _, dz, ds = pool_vectors(kind, j, pt["s"], pt["z"])
    with mp.workdps(DPS):
        al = mpf(alpha)
        zz = [mpf(a) + al * mpf(b) for a, b in zip(pt["z"], dz)]
        ss = [mpf(a) + al * mpf(b) for a, b in zip(pt["s"], ds)]
        return ns3_barrier(pt["isexp"], pt["a"], zz, ss)


# GenPow: one cone per size
GPW_SETS = tuple("late %d" % k for k in range(len(LATE_SETS)))


def gpw_set_point(d1, d2, set_name):
    k = int(set_name.split()[1])
    return gpw_point(d1, d2, LATE_SETS[k][0], LATE_SETS[k][1])


def gpw_vectors(pt):
    rng = np.random.default_rng(40 + pt["d1"] + 3 * pt["d2"])
    n = pt["d1"] + pt["d2"]
    x = rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)
    return x


@functools.lru_cache(maxsize=None)
def gpw_case(d1, d2, set_name):
    """-> dict(pt, ref (GpwScaling), kappa, refs: diag, q, r, p, D, grad (sigma_mu grad), mul_hs, E: the oracle's error)"""
    pt = gpw_set_point(d1, d2, set_name)
    mu_in = set_mu_in(set_name)
    ref = gpw_scaling(pt["alpha"], d2, pt["z"], mu_in)
    x = gpw_vectors(pt)
    refs = ref.k_entries()
    refs["grad"], refs["mul_hs"] = ref.shift(SIGMA_MU), ref.mul_hs(x)
    orc = GpwOracle(pt)
    got = orc.k_entries(mu_in)
    zero = np.zeros(d1 + d2)
    got["grad"] = orc.cones.combined_ds_shift(zero, zero, SIGMA_MU)[0]
    got["mul_hs"] = orc.cones.mul_Hs(x)
    E = {name: rel_vec(got[name], refs[name]) for name in refs if len(refs[name])}
    return dict(pt=pt, ref=ref, kappa=ref.kappa, refs=refs, E=E, x=x, mu_in=mu_in, oracle=orc)


GPW_STEP_SET = "late 1"
GPW_STEP_CASES = ("stays feasible", "backtracks", "ends at 0", "last u leaves", "last w leaves")


def gpw_step_case(d1, d2, set_name, case):
    """-> (dz, ds, z, s, alpha_max).  Cases: "stays feasible", "backtracks" (-2.2 of the whole point on one side), "ends
    at 0", "last u leaves" (only element dim1 - 1 of dz moves, to -2.2 z: a sign test), "last w leaves" (only element
    dim1 + dim2 - 1 of ds moves, so that ||w||^2 crosses prod u^(2 alpha) at 1 / 2.2)"""
    pt = gpw_set_point(d1, d2, set_name)
    z, s, n = pt["z"], pt["s"], d1 + d2
    rng = np.random.default_rng(80 + d1 + 3 * d2)
    mask = np.concatenate([np.ones(d1), np.zeros(d2)])  # (noise in the u part only: the w part has zeta / phi = 1e-2 to spare)
    noise = lambda q: 0.002 * mask * np.abs(q) * rng.uniform(-1.0, 1.0, n)  # noqa: E731
    dz, ds = 0.3 * z + noise(z), 0.1 * s + noise(s)
    if case == "backtracks":
        ds = -2.2 * s + noise(s)
    elif case == "ends at 0":
        dz = -1e5 * z + noise(z)
    elif case == "last u leaves":
        dz, ds = np.zeros(n), np.zeros(n)
        dz[d1 - 1] = -2.2 * z[d1 - 1]
    elif case == "last w leaves":
        assert d2 > 0
        dz, ds = np.zeros(n), np.zeros(n)
        with mp.workdps(DPS):
            t = gpw_terms(pt["alpha"], s, False)
            rest = -t[1] - mpf(s[n - 1]) ** 2
            target = mp.sqrt(t[0] - rest)  # |w_last| on the boundary
            ds[n - 1] = float((target - mpf(s[n - 1])) * mp.mpf("2.2"))
    else:
        assert case == "stays feasible"
    return dz, ds, z, s, 1.0


@functools.lru_cache(maxsize=None)
def gpw_step_expected(d1, d2, set_name, case, sym_step=np.inf):
    dz, ds, z, s, amax = gpw_step_case(d1, d2, set_name, case)
    return gpw_step(gpw_set_point(d1, d2, set_name)["alpha"], dz, ds, z, s, first_candidate(amax, sym_step))


@functools.lru_cache(maxsize=None)
def gpw_barrier_point(d1, d2):
    """a pair for compute_barrier whose reference barrier is FINITE: z of zeta / phi = 0.5, s_w = c r with r the scaling's
    vector built from z (parallel to z_w; genpowcone.rs:427-429 scales THAT vector by g1 / ||s_w||, so -g(s) stays in the
    dual cone while ||r|| <= ||s_w||), s_u uniform in [1, 2] times 3 ||s_w||.  c is the first of 2, 3, 4, ... at which the
    stopping test of the reference's Newton iteration is a factor NEWTON_MARGIN from its threshold at both BARRIER_ALPHAS"""
    pt = gpw_point(d1, d2, 0.5, 1.0)
    if d2 == 0:
        return dict(pt), 1.0
    ref = GpwScaling(pt["alpha"], d2, pt["z"], 1.0)
    rng = np.random.default_rng(20 + d1 + 3 * d2)
    su = rng.uniform(1.0, 2.0, d1)
    for c in range(2, 40):
        sw = c * _round(ref.r)
        out = dict(pt)
        out["s"] = np.concatenate([3.0 * np.linalg.norm(sw) * su, sw])
        at = [_gpw_barrier_at(out, al) for al in BARRIER_ALPHAS]
        if all(float(b[2]) >= MARGIN and float(b[3]) >= NEWTON_MARGIN for b in at):
            return out, float(c)
    raise AssertionError((d1, d2))


def _gpw_barrier_dirs(pt):
    d1, n = pt["d1"], pt["d1"] + pt["d2"]
    rng = np.random.default_rng(60 + d1 + 3 * pt["d2"])
    dz = STEP_REL * pt["z"] * rng.uniform(-1.0, 1.0, n)
    ds = STEP_REL * pt["s"] * rng.uniform(-1.0, 1.0, n)
    dz[d1:], ds[d1:] = -0.5 * STEP_REL * pt["z"][d1:], -0.25 * STEP_REL * pt["s"][d1:]
    return dz, ds


def _gpw_barrier_at(pt, alpha):
    dz, ds = _gpw_barrier_dirs(pt)
    ref = gpw_scaling(pt["alpha"], pt["d2"], pt["z"], 1.0)
    with mp.workdps(DPS):
        al = mpf(alpha)
        zz = [mpf(a) + al * mpf(b) for a, b in zip(pt["z"], dz)]
        ss = [mpf(a) + al * mpf(b) for a, b in zip(pt["s"], ds)]
        return ref.barrier(zz, ss)


@functools.lru_cache(maxsize=None)
def gpw_barrier_case(d1, d2, alpha):
    """-> (barrier, kappa, margin, Newton margin, pt, dz, ds): directions of relative size 0.05 in the u parts; the w parts of dz and ds
    are multiples of those of z and s, so that they stay parallel"""
    pt, _ = gpw_barrier_point(d1, d2)
    dz, ds = _gpw_barrier_dirs(pt)
    return _gpw_barrier_at(pt, alpha) + (pt, dz, ds)
