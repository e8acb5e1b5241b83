"""The PSD cone kernels (clarabel.rs_amd/csrc/cones.hip: k_psd_update_scaling, k_psd_ops<0..6> with psd_gemm,
lds_cholesky, psd_eig_min, psd_eig_tridiag) on the MI355X, each launched alone through the chip_debug_psd_* hooks on the
view chip_kkt_create's sizing function builds, against the references of tests/psd_ref.py (tests/test_psd_ref_host.py
checks those on the CPU), on both sides of every size at which a PSD operation changes its code path:

    n 11 | 12        eigenvalues by two-sided Jacobi | Householder tridiagonalisation + Sturm bisection
    n 15 | 16        scalar psd_gemm | MFMA tiles with clamped edge loads
    maxdim 64 | 65   work matrices in LDS (gs = 0) | in an HBM scratch slice (gs = 1), for ALL cones of the view
    maxdim 100 | 101 the SVD's M, V staged in LDS (jacobi_lds = 2 maxdim^2) | iterated in HBM (0)
    maxdim 140 | 141 eigenvalue iteration on an LDS copy (jacobi_lds = maxdim^2 + 3 maxdim + 16) | in HBM (0)
    n 256 | 257      last side of the tridiagonal path | back to Jacobi

Every test asserts through the hooks' counters which mechanism its launch got; the eigenvalue method is the kernel's
choice by n alone (12 <= n <= 256: tridiagonal) and is named per size in PATHS.  Tolerances: psd_ref.tol -- 16 max(E,
n 2^-53) with E the error of the double restatement against the same reference on the same input, never a flat figure.
Every figure is printed before it is asserted (pytest -s).

Three wrong kernels these tests would catch (argued, not run):
  * an MFMA edge clamp off by one (min(i0 + l15, n - 2), or the mask `<= n`) at n = 17: the second tile row / column holds
    the single row 16, so M = L2' L1, L1 V, B = R R' and B X B get a wrong or missing last row --
    test_update_scaling_late_pairs[17-*] (B against mpmath, R R' = B) and test_operations_on_late_scaling[17-*] (mul_hs)
    fail by O(1), not by rounding; n = 16 beside it passes, which points at the edge;
  * the Sturm count compared with `>=` (cnt >= tid): thread t then converges to eigenvalue t - 1, thread 0 to the lower
    Gershgorin bound -- test_eigenvalues_known_spectra[12 .. 256] fails on the smallest eigenvalue of every non-trivial
    spectrum (hadamard_integer: -3 exactly) and on the sum;
  * `lis` taken from the unsorted sig (lis[p] instead of lis[rank[p]]): lambda^-1/2 no longer belongs to the sorted
    lambda -- check_small_scaling compares lambda^-1/2 with 1 / sqrt(lambda) of mpmath (descending) in every late pair,
    and step_length of test_operations_on_late_scaling scales with it; the exact Hadamard cases catch it at 64 / 128."""
import functools

import mpmath as mp
import numpy as np
import pytest

from tests import psd_ref as R

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


_VIEWS = {}


def view_of(hip, dims):
    """one PsdConesDebug per tuple of sides for the whole module"""
    dims = tuple(dims)
    if dims not in _VIEWS:
        _VIEWS[dims] = hip.PsdConesDebug(dims)
    return _VIEWS[dims]


def svd_lds(maxdim):
    """doubles of LDS update_scaling is expected to stage M and V in: both fit below 158 KiB up to side 100"""
    return 2 * maxdim * maxdim if 64 < maxdim <= 100 else 0


def eig_lds(maxdim):
    """doubles of LDS step_length / margins are expected to iterate in: the copy fits up to side 140"""
    return maxdim * maxdim + 3 * maxdim + 16 if 64 < maxdim <= 140 else 0


def assert_path(d, gs, jacobi_lds):
    assert d.counter("gs") == gs and d.counter("jacobi_lds") == jacobi_lds, \
        (d.dims, d.counter("gs"), d.counter("jacobi_lds"), gs, jacobi_lds)


def cat(parts):
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]) if parts else np.zeros(0)


def ident(n):
    return R.svec(np.eye(n))


def rel64(got, ref):
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(np.asarray(got) - np.asarray(ref)) / (den if den else 1.0))


# ---- a. the eigenvalue kernels alone ---------------------------------------------------------------------------------
# side -> (gs, LDS doubles of the eigenvalue iteration, method)
PATHS = {1: (0, 0, "jacobi"), 2: (0, 0, "jacobi"), 3: (0, 0, "jacobi"), 11: (0, 0, "jacobi"), 12: (0, 0, "tridiagonal"),
         13: (0, 0, "tridiagonal"), 16: (0, 0, "tridiagonal"), 17: (0, 0, "tridiagonal"), 21: (0, 0, "tridiagonal"),
         24: (0, 0, "tridiagonal"), 64: (0, 0, "tridiagonal"), 65: (1, 65 * 65 + 3 * 65 + 16, "tridiagonal"),
         140: (1, 140 * 140 + 3 * 140 + 16, "tridiagonal"), 141: (1, 0, "tridiagonal"), 256: (1, 0, "tridiagonal"),
         257: (1, 0, "jacobi")}
AMAX = 1e300


def check_alpha(alpha, c, n, what):
    """a step length at the identity scaling is min(amax, -1 / lambda_min): the eigenvalue it implies against the exact
    one, absolutely over ||A||_2"""
    t = R.tol(c["E_min"], n) * c["norm"]
    if alpha == AMAX:  # the kernel saw no negative eigenvalue (or one below 1 / amax)
        print("  %s %-26s alpha = amax, exact lambda_min %.3e, allowed %.3e" % (what, c["name"], c["emin"], t))
        assert c["emin"] >= -1.0 / AMAX - t, (what, c["name"])
    else:
        g = -1.0 / alpha
        print("  %s %-26s lambda_min %.17g exact %.17g err/||A|| %.2e allowed %.2e"
              % (what, c["name"], g, c["emin"], abs(g - c["emin"]) / (c["norm"] or 1.0), t / (c["norm"] or 1.0)))
        assert alpha > 0 and abs(g - c["emin"]) <= t + 4 * R.U53 * abs(c["emin"]), (what, c["name"])
    if c["emin"] > t:
        assert alpha == AMAX, (what, c["name"])  # a positive definite direction: the full step, exactly


@pytest.mark.parametrize("n", R.EIG_SIZES)
def test_eigenvalues_known_spectra(hipdev, n):
    """margins (smallest eigenvalue, sum of the positive ones) and step_length at S = Z = I (min(amax, -1 / lambda_min)
    of each direction) on matrices whose spectra are known exactly -- diagonal with a smallest eigenvalue of -1e-14 ||A||,
    zero, c I, c I + u u', an exactly singular rank-2 update, the (2, -1) Toeplitz matrix (already tridiagonal: the
    s2 == 0 branch), Hadamard-similar integer / clustered (1, 1 + j 2^-43, -2^-30) / -2^-45 spectra and the clustered one
    scaled by 2^+-200 -- and, up to side 24, rotated clustered spectra and the Wilkinson matrix (side 21: W21+) against
    mpmath's eigsy.  One cone per matrix, all in one launch per side.

    E of numpy.linalg.eigvalsh on the same svec input, over ||A||_2, is at most 2.9e-15 (smallest eigenvalue) and 5.7e-14
    (sum) over all cases and sides, mostly below the floor n 2^-53; tests/test_psd_ref_host.py prints it per case.  The
    device on one MI355X: 4.6e-15 and 1.1e-13.  Before the fix of psd_eig_min's rotations side 257 gave a sum off by
    8.1e-12 ||A|| (toeplitz_tridiagonal) and 4.2e-12 ||A|| (hadamard_clustered) against 4.6e-13 allowed."""
    gs, lds, method = PATHS[n]
    assert method == ("tridiagonal" if 12 <= n <= 256 else "jacobi")
    cases = R.spectra(n)
    d = view_of(hipdev, [n] * len(cases))
    z = cat([c["x"] for c in cases])
    pmin, psum = d.margins(z)
    assert_path(d, gs, lds)
    print("n = %d (%s, gs = %d, eigenvalue LDS = %d)" % (n, method, gs, lds))
    for c, a, b in zip(cases, pmin, psum):
        tm, ts = R.tol(c["E_min"], n) * c["norm"], R.tol(c["E_sum"], n) * c["norm"]
        nrm = c["norm"] or 1.0
        print("  margins %-26s min err/||A|| %.2e (allowed %.2e, E %.2e)  sum err/||A|| %.2e (allowed %.2e, E %.2e)"
              % (c["name"], abs(a - c["emin"]) / nrm, tm / nrm, c["E_min"], abs(b - c["esum"]) / nrm, ts / nrm, c["E_sum"]))
    for c, a, b in zip(cases, pmin, psum):
        tm, ts = R.tol(c["E_min"], n) * c["norm"], R.tol(c["E_sum"], n) * c["norm"]
        assert abs(mp.mpf(float(a)) - c["emin_mp"]) <= tm, c["name"]
        assert abs(mp.mpf(float(b)) - c["esum_mp"]) <= ts, c["name"]
    # identity scaling: R = Rinv = B = I, lambda = 1, exactly
    e = cat([ident(n)] * len(cases))
    assert d.update_scaling(e, e)
    assert_path(d, gs, svd_lds(n))
    B, lam, lis, Rm, Ri = d.state(len(cases) - 1)
    I = np.eye(n)
    assert np.array_equal(B, I) and np.array_equal(Rm, I) and np.array_equal(Ri, I)
    assert np.array_equal(lam, np.ones(n)) and np.array_equal(lis, np.ones(n))
    for what, alphas in (("dz", d.step_length(z, e, AMAX)), ("ds", d.step_length(e, z, AMAX))):
        assert_path(d, gs, lds)
        for c, al in zip(cases, alphas):
            check_alpha(al, c, n, what)


# ---- b. update_scaling -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def companion(n):
    """a well-conditioned (1e4) generic cone of side n: svec inputs and the double restatement"""
    S, Z = R.well_pair(n, 50 + n)
    s, z = R.svec(S), R.svec(Z)
    cone, B = R.numpy_scaling(s, z, n)
    return dict(n=n, s=s, z=z, S=R.unsvec(s, n), Z=R.unsvec(z, n), cone=cone, B=B)


def check_small_scaling(state, c, label):
    """B, lambda, lambda^-1/2 of a cone against the 60-digit scaling, R and Rinv through the invariants evaluated in
    mpmath from the device's output (clustered singular values leave V free: no entry-by-entry check)"""
    n, ref, cone = c["n"], c["ref"], c["cone"]
    B, lam, lis, Rm, Ri = state
    with mp.workdps(R.DPS):
        lis_ref = [1 / mp.sqrt(v) for v in ref.lam]
    eB, el, ei = R.rel_mat(B, ref.B), R.rel_vec(lam, ref.lam), R.rel_vec(lis, lis_ref)
    E_lis = R.rel_vec(cone.lisqrt, lis_ref)
    print("  %s n=%d B %.2e (E %.2e) lambda %.2e (E %.2e) lambda^-1/2 %.2e (E %.2e)"
          % (label, n, eB, c["E_B"], el, c["E_lam"], ei, E_lis))
    inv = ref.invariants(Rm, Ri, lam, B)
    for k in sorted(inv):
        print("    %-7s %.2e (E %.2e)" % (k, inv[k], c["E_inv"][k]))
    assert eB <= R.tol(c["E_B"], n) and el <= R.tol(c["E_lam"], n) and ei <= R.tol(E_lis, n), label
    for k in inv:
        assert inv[k] <= R.tol(c["E_inv"][k], n), (label, k)
    assert np.all(np.diff(lam) <= 0)  # descending, like the reference's SVD


LATE_SIZES = (3, 8, 11, 12, 15, 16, 17, 24)


@pytest.mark.parametrize("which", range(len(R.LATE_SETS)))
@pytest.mark.parametrize("n", LATE_SIZES)
def test_update_scaling_late_pairs(hipdev, n, which):
    """late-iterate pairs (a = logspace(-k, k), S Z ~ mu I: (k, mu, t) = (2, 1, 0.3), (3, 1e-6, 1e-2), (4, 1e-8, 1e-3))
    either side of the scalar | MFMA product (15 | 16, 17 with clamped edge tiles), scaled alone (work matrices in
    LDS), beside a side-70 cone (HBM scratch, SVD staged in LDS) and beside a side-101 and a side-144 cone (SVD
    iterated in HBM).  The small cone's state is checked against mpmath in the first company and must be bitwise the
    same in the others: where the work matrices live changes no operation and no order of operations.

    E of the double restatement (oracle/psd_numpy.py), measured: E(B) <= 7.5e-14 / 1.2e-11 / 5.2e-10 and E(lambda) <=
    7.0e-15 / 1.7e-12 / 1.7e-10 for the three sets (per case: tests/test_psd_ref_host.py -s); cap 1e-8.  The device on one
    MI355X: B 4.2e-14 / 1.1e-11 / 5.1e-10, lambda 6.8e-15 / 1.9e-12 / 3.3e-10."""
    c = R.late_case(n, which)
    assert c["E_B"] <= R.E_CAP and c["E_lam"] <= R.E_CAP  # a regenerated input cannot make the case vacuous
    states = []
    for comp, gs in (((), 0), ((70,), 1), ((101, 144), 1)):
        dims = (n,) + comp
        d = view_of(hipdev, dims)
        s = cat([c["s"]] + [companion(m)["s"] for m in comp])
        z = cat([c["z"]] + [companion(m)["z"] for m in comp])
        assert d.update_scaling(s, z)
        assert_path(d, gs, svd_lds(max(dims)))
        assert d.counter("jacobi_lds") == {(): 0, (70,): 2 * 70 * 70, (101, 144): 0}[comp]
        states.append(d.state(0))
    check_small_scaling(states[0], c, "alone")
    for other, label in ((states[1], "beside 70"), (states[2], "beside 101 and 144")):
        for a, b, what in zip(states[0], other, ("B", "lambda", "lambda^-1/2", "R", "Rinv")):
            assert np.array_equal(a, b), (label, what, float(np.max(np.abs(a - b))))


def ld(M):
    return np.asarray(M, dtype=np.longdouble)


def big_residuals(S, Z, B, Rm, Ri, lam):
    """B Z B = S, R Rinv = I, R' Z R = Lambda, R R' = B: relative residuals, evaluated in extended precision"""
    S, Z, B, Rm, Ri, L = ld(S), ld(Z), ld(B), ld(Rm), ld(Ri), np.diag(ld(lam))
    f = lambda M: float(np.sqrt(np.sum(M * M)))
    n = S.shape[0]
    return dict(BZB=f(B @ Z @ B - S) / f(S), RRinv=f(Rm @ Ri - np.eye(n)) / np.sqrt(n), RtZR=f(Rm.T @ Z @ Rm - L) / f(L),
                RRt=f(Rm @ Rm.T - B) / f(B))


def check_big_scaling(state, S, Z, B_ref, lam_ref, E_B, E_lam, cone, label):
    n = S.shape[0]
    B, lam, lis, Rm, Ri = state
    eB, el = rel64(B, B_ref), rel64(lam, lam_ref)
    res = big_residuals(S, Z, B, Rm, Ri, lam)
    res_np = big_residuals(S, Z, cone.R @ cone.R.T, cone.R, cone.Rinv, cone.lam)
    print("  %s n=%d B %.2e (E %.2e) lambda %.2e (E %.2e)" % (label, n, eB, E_B, el, E_lam))
    for k in sorted(res):
        print("    %-7s %.2e (double restatement %.2e)" % (k, res[k], res_np[k]))
    assert eB <= R.tol(E_B, n) and el <= R.tol(E_lam, n), label
    for k in res:
        assert res[k] <= R.tol(res_np[k], n), (label, k)
    assert rel64(lis, 1.0 / np.sqrt(lam)) <= 4 * R.U53 and np.all(np.diff(lam) <= 0)


@pytest.mark.parametrize("dims", [(65, 100), (70,), (128,), (101, 144)], ids=lambda d: "+".join(map(str, d)))
def test_update_scaling_big_cones(hipdev, dims):
    """generic cones of condition 1e4 on the HBM-scratch path, both sides of the SVD staging limit (100 | 101), against
    the double restatement and the invariants B Z B = S, R Rinv = I, R' Z R = Lambda, R R' = B (residuals evaluated in
    extended precision).  No mpmath at these sides (a 60-digit SVD of side 144 takes minutes), so E is the distance
    between two independent double evaluations -- psd_numpy (Cholesky + LAPACK SVD) and B = Z^-1/2 (Z^1/2 S Z^1/2)^1/2
    Z^-1/2, lambda^2 = eig(L2' S L2) by symmetric eigendecompositions: measured E(B) 2e-12 .. 7e-12 (the second evaluation is the
    less accurate one; the device is within 4.3e-14 of psd_numpy), E(lambda) 1e-15 .. 2e-15 (device 2.0e-14) -- and the invariants are
    allowed 16 x the residual the double restatement leaves."""
    d = view_of(hipdev, dims)
    comps = [companion(n) for n in dims]
    assert d.update_scaling(cat([c["s"] for c in comps]), cat([c["z"] for c in comps]))
    assert_path(d, 1, svd_lds(max(dims)))
    assert d.counter("jacobi_lds") == {(65, 100): 20000, (70,): 9800, (128,): 0, (101, 144): 0}[dims]
    for k, c in enumerate(comps):
        S, Z = c["S"], c["Z"]
        w, Q = np.linalg.eigh(Z)
        Zh, Zih = (Q * np.sqrt(w)) @ Q.T, (Q / np.sqrt(w)) @ Q.T
        w2, Q2 = np.linalg.eigh(R.sym(Zh @ S @ Zh))
        B_alt = Zih @ ((Q2 * np.sqrt(w2)) @ Q2.T) @ Zih
        L2 = np.linalg.cholesky(Z)
        lam_alt = np.sqrt(np.sort(np.linalg.eigvalsh(R.sym(L2.T @ S @ L2)))[::-1])
        check_big_scaling(d.state(k), S, Z, c["B"], c["cone"].lam, rel64(B_alt, c["B"]), rel64(lam_alt, c["cone"].lam),
                          c["cone"], "side %d of %s" % (c["n"], dims))


@pytest.mark.parametrize("n", [64, 128])
def test_update_scaling_exact_hadamard(hipdev, n):
    """S = H diag(4^k) H / n, Z = H diag(4^m) H / n: B = H diag(2^(k - m)) H / n and lambda = 2^(k + m) are exact, the
    singular values come in clusters of equal values (V is free inside a cluster; B and lambda are not).  Side 64 is the
    last with the work matrices in LDS, side 128 runs in HBM scratch with nothing staged for the SVD.  E of the double
    restatement at side 64: E(B) = 2.3e-15, E(lambda) = 6.5e-16 (both under the floor n 2^-53); the device: 1.2e-14, 8.7e-15."""
    S, Z, B_ex, lam_ex = R.hadamard_pair(n)
    s, z = R.svec(S), R.svec(Z)
    cone, B_np = R.numpy_scaling(s, z, n)
    d = view_of(hipdev, (n,))
    assert d.update_scaling(s, z)
    assert_path(d, int(n > 64), 0)
    check_big_scaling(d.state(0), S, Z, B_ex, lam_ex, rel64(B_np, B_ex), rel64(cone.lam, lam_ex), cone, "hadamard")


def test_update_scaling_reports_indefinite_cone(hipdev):
    """one cone without a Cholesky factor among three good ones: update_scaling reports the failure, for S as for Z
    (psdtrianglecone.rs:165-169 returns false; the composite stops at the first failing cone and the solver ends the
    solve, so neither the reference nor include/clarabel_hip.h promises anything about the other cones' scalings --
    nothing is pinned for them), and the verdict is not sticky: the next update_scaling with interior points succeeds
    and leaves every state right."""
    dims = (8, 12, 8, 16)
    cases = [R.late_case(8, 0), R.late_case(12, 0), R.late_case(8, 1), R.late_case(16, 0)]
    d = view_of(hipdev, dims)
    s, z = cat([c["s"] for c in cases]), cat([c["z"] for c in cases])
    bad = R.late_pair(12, 0)[0].copy()
    w, Q = np.linalg.eigh(bad)
    w[0] = -1e-3 * w[-1]
    bad = R.svec(R.sym((Q * w) @ Q.T))  # one negative eigenvalue
    for which in ("s", "z"):
        s2, z2 = s.copy(), z.copy()
        (s2 if which == "s" else z2)[d.rows_of(1)] = bad
        assert d.update_scaling(s2, z2) is False
        assert_path(d, 0, 0)
        assert d.update_scaling(s, z) is True
        for k, c in enumerate(cases):
            check_small_scaling(d.state(k), c, "cone %d after a failed scaling of %s" % (k, which))


# ---- c. the operations on a late scaling -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def op_inputs(n, which):
    """directions for the operations on late_case(n, which): symmetric, a tenth of the iterate in norm"""
    c = R.late_case(n, which)
    rng = np.random.default_rng(31 * n + which)
    S, Z = R.unsvec(c["s"], n), R.unsvec(c["z"], n)
    G1, G2, G3 = (R.sym(rng.standard_normal((n, n))) for _ in range(3))
    dz = R.svec(0.1 * np.linalg.norm(Z) / np.linalg.norm(G1) * G1)
    ds = R.svec(0.1 * np.linalg.norm(S) / np.linalg.norm(G2) * G2)
    x = R.svec(G3)
    # directions relative to the iterate: Z + alpha dzi = L2 (I + 0.3 alpha G / ||G||_2) L2' stays interior up to alpha = 3.3
    L1, L2 = np.linalg.cholesky(S), np.linalg.cholesky(Z)
    dzi = R.svec(R.sym(L2 @ (0.3 / np.linalg.norm(G1, 2) * G1) @ L2.T))
    dsi = R.svec(R.sym(L1 @ (0.3 / np.linalg.norm(G2, 2) * G2) @ L1.T))
    return dict(dz=dz, ds=ds, dzi=dzi, dsi=dsi, x=x, sigma_mu=0.37 * float(c["s"] @ c["z"]) / n)


def scalar_err(got, ref):
    with mp.workdps(R.DPS):
        return float(abs(mp.mpf(float(got)) - ref) / abs(ref)) if ref != 0 else abs(float(got))


def mp_eigs(v, n):
    with mp.workdps(R.DPS):
        ev = mp.eigsy(R.mp_unsvec(v, n), eigvals_only=True)
        return [ev[i] for i in range(n)]


def np_eigs(v, n):
    return np.linalg.eigvalsh(R.unsvec(v, n))


OP_SIZES = (11, 12, 16, 17, 24)


@pytest.mark.parametrize("which", [0, 2])
@pytest.mark.parametrize("n", OP_SIZES)
def test_operations_on_late_scaling(hipdev, n, which):
    """mul_hs, affine_ds, combined_ds_shift, ds_from_dz_offset, step_length (directions relative to the iterate scaled 0.05 / 1 / 40,
    a generic one that cuts the step, and one that ends exactly on the boundary: dz = -z, ds = -s, step 1) and barrier (two interior points and one outside the cone:
    +inf) after update_scaling of a late pair (set 0: separated singular values; set 2: a = logspace(-4, 4), mu = 1e-8,
    singular values within 1e-3 of each other), alone (LDS) and beside a side-70 and a side-144 cone (HBM scratch,
    nothing staged).  The reference evaluates every operation in 60 digits WITH THE EXACT SCALING of the same S, Z, not
    with the device's state: the errors are the compound errors the solver sees.

    W x depends on the sign of each singular pair, and with close singular values on the basis of the cluster: wz, ws
    and shift are compared entry by entry (signs aligned with the device's R) for set 0 only, through their eigenvalues
    (invariant under a change of basis) for both sets, and through the chain the solver uses them in,
    ds_from_dz_offset(affine_ds + shift), which does not depend on V at all.  E of the double restatement per output is
    printed beside the device's error; measured E (device) for sets 0 / 2: chain 1.4e-13 (1.4e-13) / 9.6e-9 (4.8e-9),
    step_length 2.2e-13 (1.6e-13) / 2.1e-9 (1.9e-9), barrier over its terms 1.8e-14 (1.0e-14) / 1.6e-11 (1.3e-11)."""
    c, inp = R.late_case(n, which), op_inputs(n, which)
    assert c["E_B"] <= R.E_CAP and c["E_lam"] <= R.E_CAP
    ref0, cone = c["ref"], c["cone"]
    dz, ds, x, smu = inp["dz"], inp["ds"], inp["x"], inp["sigma_mu"]
    dzi, dsi = inp["dzi"], inp["dsi"]
    steps = [(0.05 * dzi, 0.05 * dsi), (dzi, dsi), (40.0 * dzi, 40.0 * dsi), (dz, ds), (-c["z"], -c["s"])]
    bars = [(dzi, dsi, 0.0), (dzi, dsi, 0.7), (-2.0 * c["z"], dsi, 1.0)]
    # the double restatement, for E
    sh_np, wz_np, ws_np = cone.combined_ds_shift(dz, ds, smu)
    np_out = dict(mul_hs=cone.mul_Hs(x), affine_ds=cone.affine_ds(), shift=sh_np, wz=wz_np, ws=ws_np,
                  chain=cone.ds_from_dz_offset(cone.affine_ds() + sh_np),
                  steps=[cone.step_length(a, b, 1.0) for a, b in steps],
                  bars=[cone.compute_barrier(c["z"], c["s"], a, b, al) for a, b, al in bars])
    results = []
    for comp in ((), (70, 144)):
        dims = (n,) + comp
        d = view_of(hipdev, dims)
        rng = np.random.default_rng(5)
        full = lambda v, sc=0.0: cat([v] + [sc * rng.standard_normal(m * (m + 1) // 2) for m in comp])
        s = cat([c["s"]] + [companion(m)["s"] for m in comp])
        z = cat([c["z"]] + [companion(m)["z"] for m in comp])
        assert d.update_scaling(s, z)
        assert_path(d, int(bool(comp)), 0)
        sl = d.rows_of(0)
        sh, wz, ws = d.combined_ds_shift(full(dz, 0.01), full(ds, 0.01), smu)
        aff = d.affine_ds()
        out = dict(mul_hs=d.mul_hs(full(x, 1.0))[sl], affine_ds=aff[sl], shift=sh[sl], wz=wz[sl], ws=ws[sl],
                   chain=d.ds_from_dz_offset(aff + sh)[sl], steps=[], bars=[])
        for a, b in steps:
            out["steps"].append(d.step_length(full(a), full(b), 1.0)[0])
            assert_path(d, int(bool(comp)), 0)  # (maxdim 144: the eigenvalue iteration is not staged either)
        for a, b, al in bars:
            out["bars"].append(d.barrier(z, s, full(a), full(b), al)[0])
        out["R"] = d.state(0)[3]
        results.append(out)
    dev = results[0]
    # the references, with the signs of the device's / the restatement's singular pairs
    refs = {}
    for who, Rd in (("dev", dev["R"]), ("np", cone.R)):
        ref = ref0.aligned(Rd)
        sh, wz, ws = ref.combined_ds_shift(dz, ds, smu)
        with mp.workdps(R.DPS):
            chain = ref.ds_from_dz_offset([a + b for a, b in zip(ref.affine_ds(), sh)])
        refs[who] = dict(mul_hs=ref.mul_hs(x), affine_ds=ref.affine_ds(), shift=sh, wz=wz, ws=ws, chain=chain)
    step_ref = [ref0.step_length(a, b, 1.0) for a, b in steps]
    bar_ref = [ref0.barrier(c["z"], c["s"], a, b, al) for a, b, al in bars]
    fails = []

    def check(name, err, E):
        ok = err <= R.tol(E, n)
        print("  n=%d set=%d %-22s err %.2e  E %.2e  allowed %.2e%s" % (n, which, name, err, E, R.tol(E, n),
                                                                        "" if ok else "  <-- FAIL"))
        if not ok:
            fails.append(name)

    for name in ("mul_hs", "affine_ds", "chain") + (("wz", "ws", "shift") if which == 0 else ()):
        check(name, R.rel_vec(dev[name], refs["dev"][name]), R.rel_vec(np_out[name], refs["np"][name]))
    for name in ("wz", "ws", "shift"):
        ev = sorted(mp_eigs(refs["dev"][name], n))
        check(name + " eigenvalues", R.rel_vec(np.sort(np_eigs(dev[name], n)), ev),
              R.rel_vec(np.sort(np_eigs(np_out[name], n)), ev))
    for k, (a, r, e) in enumerate(zip(dev["steps"], step_ref, np_out["steps"])):
        check("step_length[%d]" % k, scalar_err(a, r), scalar_err(e, r))
    assert float(step_ref[0]) == 1.0 and float(step_ref[1]) == 1.0 and float(step_ref[2]) < 0.2 and float(step_ref[3]) < 1.0
    assert dev["steps"][0] == 1.0 and dev["steps"][1] == 1.0  # (interior by a wide margin: the full step, exactly)
    assert float(step_ref[4]) == 1.0  # the boundary direction: exactly the full step in exact arithmetic
    for k, (a, r, e) in enumerate(zip(dev["bars"][:2], bar_ref[:2], np_out["bars"][:2])):
        check("barrier[%d]" % k, float(abs(mp.mpf(float(a)) - r[0]) / r[1]), float(abs(mp.mpf(float(e)) - r[0]) / r[1]))
    assert bar_ref[2][0] == mp.inf and dev["bars"][2] == np.inf and results[1]["bars"][2] == np.inf
    assert not fails, fails
    # beside the big cones the small cone's arithmetic is the same, operation for operation
    for name in ("mul_hs", "affine_ds", "shift", "wz", "ws", "chain", "steps", "bars"):
        assert np.array_equal(np.asarray(dev[name]), np.asarray(results[1][name])), name


# ---- d. edge sizes ---------------------------------------------------------------------------------------------------
def test_mixed_sides_in_one_launch(hipdev):
    """cones of sides 2, 12, 16 and 64 in ONE launch (LDS sized by the largest; Jacobi | tridiagonal eigenvalues and
    scalar | MFMA products side by side): update_scaling of late pairs (64: the exact Hadamard case), then margins of a
    Hadamard-similar integer spectrum per cone"""
    dims = (2, 12, 16, 64)
    d = view_of(hipdev, dims)
    small = [R.late_case(n, 1) for n in dims[:3]]
    S, Z, B_ex, lam_ex = R.hadamard_pair(64)
    s64, z64 = R.svec(S), R.svec(Z)
    cone64, B_np = R.numpy_scaling(s64, z64, 64)
    assert d.update_scaling(cat([c["s"] for c in small] + [s64]), cat([c["z"] for c in small] + [z64]))
    assert_path(d, 0, 0)
    for k, c in enumerate(small):
        check_small_scaling(d.state(k), c, "side %d of %s" % (c["n"], dims))
    check_big_scaling(d.state(3), S, Z, B_ex, lam_ex, rel64(B_np, B_ex), rel64(cone64.lam, lam_ex), cone64, "side 64")
    sp = [[c for c in R.spectra(n) if c["name"] == "hadamard_integer"][0] for n in dims]
    pmin, psum = d.margins(cat([c["x"] for c in sp]))
    assert_path(d, 0, 0)
    for n, c, a, b in zip(dims, sp, pmin, psum):
        print("  side %d min %.17g (exact %g) sum %.17g (exact %g)" % (n, a, c["emin"], b, c["esum"]))
        assert abs(a - c["emin"]) <= R.tol(c["E_min"], n) * c["norm"]
        assert abs(b - c["esum"]) <= R.tol(c["E_sum"], n) * c["norm"]


def test_smallest_sides(hipdev):
    """the cone constructor accepts side 1 (a scalar: B = sqrt(s / z), lambda = sqrt(s z)) and side 0 (an empty cone,
    which the reference bails out of early: margins (max, 0), psdtrianglecone.rs:108-110; full step; barrier 0)"""
    d = view_of(hipdev, (0, 1, 0))
    assert d.rows == 1
    assert d.update_scaling([4.0], [9.0])
    assert_path(d, 0, 0)
    B, lam, lis, Rm, Ri = d.state(1)
    # sqrt(4) / sqrt(6) and its reciprocal forms, in double: a few roundings of sqrt and of the division
    assert abs(B[0, 0] - 2.0 / 3.0) <= 8 * R.U53 and abs(lam[0] - 6.0) <= 8 * R.U53
    assert abs(Rm[0, 0] * Ri[0, 0] - 1.0) <= 4 * R.U53 and abs(lis[0] * np.sqrt(lam[0]) - 1.0) <= 4 * R.U53
    pmin, psum = d.margins([-2.5])
    assert pmin[1] == -2.5 and psum[1] == 0.0 and pmin[0] >= FMAX and pmin[2] >= FMAX and psum[0] == 0 and psum[2] == 0
    pmin, psum = d.margins([3.0])
    assert pmin[1] == 3.0 and psum[1] == 3.0
    al = d.step_length([-18.0], [1.0], 1.0)  # W dz = dz / 1.5 = -12, lambda = 6: lambda^-1/2 . lambda^-1/2 = -2 -> 1/2
    assert abs(al[1] - 0.5) <= 16 * R.U53 and al[0] == 1.0 and al[2] == 1.0
    bar = d.barrier([9.0], [4.0], [1.0], [1.0], 0.0)
    assert abs(bar[1] + np.log(36.0)) <= 16 * R.U53 * np.log(36.0) and bar[0] == 0.0 and bar[2] == 0.0
    assert d.barrier([9.0], [4.0], [-10.0], [1.0], 1.0)[1] == np.inf
