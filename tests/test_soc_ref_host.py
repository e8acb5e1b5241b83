"""Self-checks of tests/soc_ref.py (the references of tests/test_soc_passes_gpu.py), on the CPU: the 60-digit scaling
satisfies its own invariants to 1e-50, the exact edge inputs give the hand-derived values, the error E of the double
restatement (oracle.Cones) and the floor kappa 2^-53 are printed for every case and size and E lies under its cap --
so that a regenerated input cannot make a GPU test vacuous -- and a second double restatement that sums in another
order (256 strided partial sums folded by a tree, as a workgroup does) lies within the tolerance the kernels get."""
import mpmath as mp
import numpy as np
import pytest

from tests import soc_ref as R

SETS = range(len(R.LATE_SETS))


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("n", R.DIMS)
def test_mp_scaling_invariants_and_caps(n, which):
    """Hs z = s, W z = W^-1 s = lambda, W W^-1 = I, and Hs = eta^2 (2 w w' - J) = eta^2 (D + u u' - v v') for the sparse
    form, in 60 digits; E of the double restatement and the floor kappa 2^-53 printed, E under the cap.  Measured: the
    largest E over all sizes and outputs is 3.5e-14 / 1.9e-12 / 5.6e-10 / 1.9e-8 for the four sets (cap 1e-7), kappa 2^-53 =
    2.8e-15 / 2.8e-13 / 2.8e-11 / 2.8e-9."""
    c = R.late_case(n, which)
    ref, s, z = c["ref"], c["s"], c["z"]
    k, mu, t = R.LATE_SETS[which]
    with mp.workdps(R.DPS):
        eps = mp.mpf(10) ** -50
        assert R.rel_vec(s, ref.mul_hs(z)) <= eps
        assert mp.sqrt(sum((a - b) ** 2 for a, b in zip(ref.mul_hs(z), ref.s))) <= eps * abs(ref.s[0])
        lam_n = mp.sqrt(sum(a * a for a in ref.lam))
        for got in (ref.mul_W(ref.z), ref.mul_Winv(ref.s)):
            assert mp.sqrt(sum((a - b) ** 2 for a, b in zip(got, ref.lam))) <= eps * lam_n
        x = R.mpv(np.random.default_rng(n).standard_normal(n))
        back = ref.mul_W(ref.mul_Winv(x))
        assert mp.sqrt(sum((a - b) ** 2 for a, b in zip(back, x))) <= eps * mp.sqrt(sum(a * a for a in x))
        # the sparse form against the dense one, through a product (and entry by entry where that is cheap)
        u, v, w = ref.u(), ref.v(), ref.w
        dg = [ref.d] + [mp.mpf(1)] * (n - 1)
        ux, vx = R.mp_dot(u, x), R.mp_dot(v, x)
        sp = [ref.eta2 * (dg[i] * x[i] + u[i] * ux - v[i] * vx) for i in range(n)]
        hx = ref.mul_hs(x)
        assert mp.sqrt(sum((a - b) ** 2 for a, b in zip(sp, hx))) <= eps * mp.sqrt(sum(a * a for a in hx))
        if n <= 66:
            dense = ref.hs_dense()
            p = 0
            for col in range(n):
                for row in range(col + 1):
                    e = ref.eta2 * ((dg[row] if row == col else 0) + u[row] * u[col] - v[row] * v[col])
                    assert abs(e - dense[p]) <= eps * ref.eta2 * w[0] * w[0]
                    p += 1
        # the pair is what it claims to be: eigenvalues (10^k, 10^-k) of s, s o z ~ mu e up to the turn t
        sp_, sm_ = ref.s[0] + mp.sqrt(ref.s[0] ** 2 - R.mp_res(ref.s)), ref.s[0] - mp.sqrt(ref.s[0] ** 2 - R.mp_res(ref.s))
        assert abs(sp_ / mp.mpf(10) ** k - 1) <= 1e-9 and abs(sm_ * mp.mpf(10) ** k - 1) <= 1e-6
        assert R.mp_res(ref.z) > 0 and abs(R.mp_dot(ref.s, ref.z) / mu - 1) <= (10.0 ** (2 * k)) * t * t + 1e-6
    kf = c["kappa"] * R.U53
    print("late n=%d set=%d kappa 2^-53 = %.2e  E: %s" % (n, which, kf, "  ".join("%s %.2e" % (a, b) for a, b in sorted(c["E"].items()))))
    assert max(c["E"].values()) <= R.E_CAP, c["E"]
    assert 0.2 * 10.0 ** (2 * k) <= c["kappa"] <= 10.0 ** (2 * k)


def tree_sum(v):
    """256 strided partial sums (thread t: elements t, t + 256, ...), then a pairwise tree: the order a workgroup sums in"""
    p = np.zeros(256)
    for t in range(min(256, len(v))):
        acc = 0.0
        for a in v[t::256]:
            acc += a
        p[t] = acc
    while len(p) > 1:
        p = p[0::2] + p[1::2]
    return float(p[0])


def np_scaling(s, z, S):
    """socone.rs:134-184 in double with the sums taken by S: -> eta w, lambda o lambda"""
    def nrm(x):
        am = np.max(np.abs(x)) if len(x) else 0.0
        return 0.0 if am == 0 else am * np.sqrt(S((np.abs(x) / am) ** 2))

    def res(x):
        t = nrm(x[1:])
        return (x[0] - t) * (x[0] + t)

    zs, ss = np.sqrt(res(z)), np.sqrt(res(s))
    eta = np.sqrt(ss / zs)
    w = s / ss
    w[0] += z[0] / zs
    w[1:] -= z[1:] / zs
    ws = np.sqrt(res(w))
    w = w / ws
    w[0] = np.sqrt(1 + S(w[1:] ** 2))
    g = 0.5 * ws
    lam = np.empty_like(s)
    lam[0] = g
    lam[1:] = ((g + z[0] / zs) / ss * s[1:] + (g + s[0] / ss) / zs * z[1:]) / (s[0] / ss + z[0] / zs + 2 * g)
    lam *= np.sqrt(ss * zs)
    aff = np.concatenate([[S(lam * lam)], 2 * lam[0] * lam[1:]])
    return eta * w, aff


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("n", R.DIMS)
def test_double_restatement_in_another_order_within_tol(n, which):
    """eta w and lambda o lambda of a numpy restatement that sums like a workgroup, against mpmath within tol(E, n,
    kappa) with E the oracle's error: the tolerance the kernels get holds for a correct double evaluation in another
    summation order (measured: at most 0.062 of the tolerance)"""
    c = R.late_case(n, which)
    ew, aff = np_scaling(c["s"].copy(), c["z"].copy(), tree_sum)
    for name, got in (("eta_w", ew), ("affine_ds", aff)):
        err, allowed = R.rel_vec(got, c["state"][name]), R.tol(c["E"][name], n, c["kappa"])
        print("n=%d set=%d %-9s reordered %.2e  E %.2e  allowed %.2e  ratio %.3f" % (n, which, name, err, c["E"][name], allowed, err / allowed))
        assert err <= allowed


@pytest.mark.parametrize("n", R.DIMS)
def test_exact_edge_inputs(n):
    """the integer tails: nonzeros at the edge indices, the norm an integer, every scaled intermediate exact in any order;
    the step lengths, margins and barriers the GPU tests expect of them, derived by hand, from the exact-root reference"""
    x, r = R.exact_tail(n)
    idx = R.edge_indices(n)
    assert list(np.nonzero(x)[0]) == idx and idx[0] == 1 and idx[-1] == n - 1
    assert x[n - 1] == np.max(x) == 4.0 and float(np.sum(x * x)) == r * r
    q = (np.abs(x[1:]) / 4.0) ** 2
    for order in (np.arange(n - 1), np.arange(n - 1)[::-1], np.random.default_rng(n).permutation(n - 1)):
        acc = 0.0
        for v in q[order]:
            acc += v
        assert 4.0 * np.sqrt(acc) == r and tree_sum(q) == acc
    if R.has_ones_tail(n):
        o, ro = R.exact_tail(n, ones=True)
        assert ro * ro == n - 1 and np.sqrt(tree_sum(o[1:] ** 2)) == ro
    e0 = np.zeros(n)
    e0[0] = 1.0
    zero = np.zeros(n)
    on, last = x.copy(), zero.copy()
    on[0] = r          # exactly on the boundary
    last[n - 1] = 1.0
    A = 10.0
    step = lambda dz, z: float(R.soc_step_length(dz, zero, z, e0, A))
    assert step(on, 2.0 * r * e0) == A                    # a == 0: the direction on the boundary
    assert step(-on, 2.0 * r * e0) == 2.0                 # ... of -K: the scalar bound 2 r / r, a == 0 again
    assert step(e0, on) == A                              # c == 0, direction inside
    assert step(-last, on) == 0.0                         # c == 0, direction outside (a = -1)
    assert step(-e0, 2.0 * e0) == 2.0                     # the scalar bound alone: b^2 = 4 a c, both roots 2
    assert step(last, 2.0 * e0) == 2.0                    # leaves through the last tail element: a = -1, b = 0, c = 4
    z2 = on + r * e0                                      # (2 r; tail): res = 3 r^2
    assert float(R.soc_step_length(-z2, -z2, z2, z2, 1.0)) == 1.0   # d = 36 r^4 - 36 r^4 = 0: the double root 1
    a, b = R.soc_margins(z2)
    assert float(a) == r and float(b) == r
    a, b = R.soc_margins(on - 3.0 * r * e0)               # (-2 r; tail): outside
    assert float(a) == -3.0 * r and float(b) == 0.0
    bar, kap = R.soc_barrier(z2, z2, zero, zero, 0.0)
    assert abs(float(bar) + np.log(3.0 * r * r)) <= 4 * R.U53 * np.log(3.0 * r * r) and abs(kap - 4.0 / 3.0) <= 1e-12
    bar, _ = R.soc_barrier(z2, z2, -2.0 * r * e0, zero, 0.7)   # z0 = 0.6 r < r: outside
    assert bar == mp.inf


def test_nn_reference_on_hand_values():
    sc = R.NnScaling([4.0, 9.0], [9.0, 4.0])
    assert np.all(sc.lam == 6.0) and abs(float(sc.w[0]) - 2.0 / 3.0) <= R.U53 and float(sc.w[1]) == 1.5
    sh, wz, ws = sc.combined_ds_shift([3.0, 2.0], [2.0, 3.0], 0.5)
    assert abs(float(wz[0]) - 2.0) <= 4 * R.U53 and float(wz[1]) == 3.0 and float(ws[1]) == 2.0 and float(sh[1]) == 5.5
    assert float(R.nn_step_length([-2.0, 1.0], [1.0, -12.0], [1.0, 1.0], [1.0, 3.0], 1.0)) == 0.25
    assert float(R.nn_step_length([2.0, 1.0], [1.0, 1.0], [1.0, 1.0], [1.0, 3.0], 1.0)) == 1.0
    assert [float(v) for v in R.nn_margins([3.0, -2.0, 1.5])] == [-2.0, 4.5]
    assert abs(float(R.nn_barrier([1.0, 2.0], [3.0, 4.0], [0.0, 0.0], [0.0, 0.0], 0.0)) + np.log(24.0)) <= 1e-15
    assert R.nn_barrier([1.0, 2.0], [3.0, 4.0], [-2.0, 0.0], [0.0, 0.0], 0.7) == np.inf
