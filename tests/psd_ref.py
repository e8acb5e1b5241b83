"""References for the PSD cone kernels (clarabel.rs_amd/csrc/cones.hip: k_psd_update_scaling, k_psd_ops<0..6>) --
test infrastructure only, used by tests/test_psd_passes_gpu.py and checked on its own by tests/test_psd_ref_host.py.

* an mpmath (60 digits) restatement of PSDTriangleCone::update_scaling (psdtrianglecone.rs:144-204: two Cholesky
  factors, svd_r of L2' L1, R = L1 V Sigma^-1/2, Rinv = Sigma^-1/2 U' L2', B = R R') and of the operations either side of
  the solve, for sides up to 24;
* exact dyadic scalings at sides 64 and 128: S = H diag(4^k) H / n, Z = H diag(4^m) H / n with H the Sylvester Hadamard
  matrix -- every entry of S, Z, B = H diag(2^(k - m)) H / n is exact in double, lambda = 2^(k + m);
* symmetric matrices with known spectra for the eigenvalue kernels (psd_eig_min, psd_eig_tridiag);
* late-iterate pairs S = Q diag(a) Q', Z = Q2 diag(mu / a) Q2', a = logspace(-k, k), Q2 = Q expm(t K).

The kernels are allowed 16 max(E, n 2^-53) where E is the error of the DOUBLE restatement (oracle/psd_numpy.py,
numpy.linalg.eigvalsh) against the same reference on the same input: `tol`.  Matrices and vectors are compared in the
relative Frobenius norm, eigenvalue results absolutely over ||A||_2.

The references take what the kernels take: the svec vector.  Entry (i, j), i != j, of the matrix is s_t / sqrt(2) as a
real number; the kernels and the double restatement round that product, which is part of E like every other rounding."""
import functools

import mpmath as mp
import numpy as np

from oracle import psd_numpy

DPS = 60
U53 = 2.0 ** -53
LATE_SETS = ((2, 1.0, 0.3), (3, 1e-6, 1e-2), (4, 1e-8, 1e-3))  # (k, mu, t)
E_CAP = 1e-8  # a late pair counts only while the double restatement itself is this accurate


def tol(E, n):
    """what a kernel may be off by, from the double restatement's error E on the same input"""
    return 16.0 * max(E, n * U53)


def svec(M):
    return psd_numpy.mat_to_svec(np.asarray(M, dtype=np.float64))


def unsvec(x, n):
    return psd_numpy.svec_to_mat(np.asarray(x, dtype=np.float64), n)


def sym(M):
    return 0.5 * (M + M.T)


# ---- mpmath helpers --------------------------------------------------------------------------------------------------
def mp_mat(A):
    return mp.matrix(np.asarray(A, dtype=np.float64).tolist())


def mp_unsvec(x, n):
    """the symmetric matrix an svec vector stands for (dense/matrix_math.rs:165-183), off-diagonals divided by sqrt(2)
    in the working precision"""
    M = mp.zeros(n, n)
    r2 = mp.sqrt(mp.mpf(2))
    t = 0
    for j in range(n):
        for i in range(j + 1):
            v = x[t] if isinstance(x[t], mp.mpf) else mp.mpf(float(x[t]))
            if i != j:
                v = v / r2
            M[i, j] = v
            M[j, i] = v
            t += 1
    return M


def mp_svec(M):
    n = M.rows
    r2 = mp.sqrt(mp.mpf(2))
    return [M[i, j] if i == j else (M[i, j] + M[j, i]) / r2 for j in range(n) for i in range(j + 1)]


def mp_fro(M):
    return mp.sqrt(sum(v * v for v in M))


def rel_mat(got, ref):
    """|| got - ref ||_F / || ref ||_F with ref an mp matrix, got a float array of the same shape (or an mp matrix)"""
    with mp.workdps(DPS):
        G = got if isinstance(got, mp.matrix) else mp_mat(got)
        den = mp_fro(ref)
        return float(mp_fro(G - ref) / den) if den != 0 else float(mp_fro(G - ref))


def rel_vec(got, ref):
    """|| got - ref ||_2 / || ref ||_2 with ref a list of mpf"""
    with mp.workdps(DPS):
        num = mp.sqrt(sum((mp.mpf(float(g)) - r) ** 2 for g, r in zip(got, ref)))
        den = mp.sqrt(sum(r * r for r in ref))
        return float(num / den) if den != 0 else float(num)


def mp_diag(v):
    n = len(v)
    D = mp.zeros(n, n)
    for i in range(n):
        D[i, i] = v[i]
    return D


# ---- inputs ------------------------------------------------------------------------------------------------------
def hadamard(n):
    assert n >= 1 and n & (n - 1) == 0
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def orth(n, seed):
    rng = np.random.default_rng(seed)
    Q, Rr = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(Rr))


def expm_skew(K, t):
    """expm(t K) of a skew matrix of unit spectral norm by its Taylor series (t <= 0.3: forty terms are far past double)"""
    n = K.shape[0]
    E, term = np.eye(n), np.eye(n)
    for j in range(1, 40):
        term = term @ (t * K) / j
        E = E + term
    return E


@functools.lru_cache(maxsize=None)
def late_pair(n, which):
    """(S, Z) of a late interior-point iterate: S Z ~ mu I up to the rotation expm(t K) between their eigenvectors"""
    k, mu, t = LATE_SETS[which]
    rng = np.random.default_rng(1000 * which + n)
    Q = orth(n, 7000 + 10 * n + which)
    K = rng.standard_normal((n, n))
    K = K - K.T
    nk = np.linalg.norm(K, 2)
    K = K / nk if nk > 0 else K
    Q2 = Q @ expm_skew(K, t)
    a = np.logspace(-k, k, n) if n > 1 else np.array([10.0 ** k])
    S = sym((Q * a) @ Q.T)
    Z = sym((Q2 * (mu / a)) @ Q2.T)
    return S, Z


def well_pair(n, seed, cond=1e4):
    """a well-conditioned generic pair (condition number cond each) for the big companions"""
    rng = np.random.default_rng(seed)
    a = np.logspace(-0.5 * np.log10(cond), 0.5 * np.log10(cond), n)
    Q, Q2 = orth(n, seed + 1), orth(n, seed + 2)
    S = sym((Q * a) @ Q.T)
    Z = sym((Q2 * rng.permutation(a)) @ Q2.T)
    return S, Z


def hadamard_pair(n):
    """exact dyadic scaling: -> S, Z, B, lambda (descending) -- all exact in double; the exponents repeat, so the
    singular values 2^(k + m) come in clusters"""
    H = hadamard(n)
    i = np.arange(n)
    k = (i % 5) - 2          # 4^k: 1/16 .. 16
    m = ((i // 3) % 4) - 1   # 4^m: 1/4 .. 16
    S = (H * 4.0 ** k) @ H / n
    Z = (H * 4.0 ** m) @ H / n
    B = (H * 2.0 ** (k - m)) @ H / n
    lam = np.sort(2.0 ** (k + m))[::-1]
    return S, Z, B, lam


# ---- the scaling in mpmath -------------------------------------------------------------------------------------------
class Scaling:
    """R, Rinv, B (mp matrices), lam (list of mpf, descending) and the inputs S, Z as the svec vectors define them"""

    def __init__(self, n, S, Z, R, Rinv, lam):
        self.n, self.S, self.Z, self.R, self.Rinv, self.lam = n, S, Z, R, Rinv, lam
        self.B = R * R.T

    def aligned(self, R_double):
        """the same scaling with the sign of every singular pair chosen like R_double's columns (a singular pair is
        determined up to a common sign of u_i, v_i; W x depends on it, B and everything that reaches the KKT system do
        not)"""
        with mp.workdps(DPS):
            n = self.n
            Rd = mp_mat(R_double)
            sg = [1 if sum(Rd[i, j] * self.R[i, j] for i in range(n)) >= 0 else -1 for j in range(n)]
            D = mp_diag(sg)
            return Scaling(n, self.S, self.Z, self.R * D, D * self.Rinv, self.lam)

    def invariants(self, R=None, Rinv=None, lam=None, B=None):
        """relative residuals of R' Z R = Lambda, Rinv S Rinv' = Lambda, R Rinv = I, R R' = B, B Z B = S for the given
        double arrays (default: this scaling's own)"""
        with mp.workdps(DPS):
            n = self.n
            R = self.R if R is None else mp_mat(R)
            Rinv = self.Rinv if Rinv is None else mp_mat(Rinv)
            lam = self.lam if lam is None else [mp.mpf(float(v)) for v in lam]
            B = self.B if B is None else mp_mat(B)
            L = mp_diag(lam)
            nl, nI = mp_fro(L), mp.sqrt(n)
            return dict(RtZR=float(mp_fro(R.T * self.Z * R - L) / nl),
                        RiSRit=float(mp_fro(Rinv * self.S * Rinv.T - L) / nl),
                        RRinv=float(mp_fro(R * Rinv - mp.eye(n)) / nI),
                        RRt=float(mp_fro(R * R.T - B) / mp_fro(B)),
                        BZB=float(mp_fro(B * self.Z * B - self.S) / mp_fro(self.S)))

    def lam_gap(self):
        """smallest relative gap between neighbouring singular values: W x is only comparable while it is far above the
        accuracy of a double SVD"""
        lam = self.lam
        return float(min([(lam[i] - lam[i + 1]) / lam[i] for i in range(self.n - 1)] or [mp.mpf(1)]))

    # -- the operations (psdtrianglecone.rs:214-303, symmetric_common.rs:53-95), svec in, lists of mpf out
    def mul_hs(self, x):
        with mp.workdps(DPS):
            return mp_svec(self.B * mp_unsvec(x, self.n) * self.B)

    def affine_ds(self):
        with mp.workdps(DPS):
            return mp_svec(mp_diag([v * v for v in self.lam]))

    def combined_ds_shift(self, step_z, step_s, sigma_mu):
        with mp.workdps(DPS):
            n = self.n
            wz = self.R.T * mp_unsvec(step_z, n) * self.R
            ws = self.Rinv * mp_unsvec(step_s, n) * self.Rinv.T
            sh = (ws * wz + wz * ws) / 2 - mp.mpf(float(sigma_mu)) * mp.eye(n)
            return mp_svec(sh), mp_svec(wz), mp_svec(ws)

    def ds_from_dz_offset(self, ds):
        with mp.workdps(DPS):
            n = self.n
            X = mp_unsvec(ds, n)
            for i in range(n):
                for j in range(n):
                    X[i, j] = 2 * X[i, j] / (self.lam[i] + self.lam[j])
            return mp_svec(self.R * X * self.R.T)

    def step_length(self, dz, ds, amax):
        with mp.workdps(DPS):
            n = self.n
            li = mp_diag([1 / mp.sqrt(v) for v in self.lam])
            out = mp.mpf(float(amax))
            for M in (self.R.T * mp_unsvec(dz, n) * self.R, self.Rinv * mp_unsvec(ds, n) * self.Rinv.T):
                D = li * M * li
                g = min(mp.eigsy((D + D.T) / 2, eigvals_only=True))
                if g < 0:
                    out = min(out, -1 / g)
            return out

    def barrier(self, z, s, dz, ds, alpha):
        """-> (-logdet(Z + alpha dZ) - logdet(S + alpha dS), the sum of the magnitudes of its 2 n terms -- the scale of
        its rounding errors: at mu = 1 the barrier itself is about 0); (+inf, 1) outside the cone"""
        with mp.workdps(DPS):
            n, a, bar, scale = self.n, mp.mpf(float(alpha)), mp.mpf(0), mp.mpf(0)
            for x, dx in ((z, dz), (s, ds)):
                Q = mp_unsvec(x, n) + a * mp_unsvec(dx, n)
                if min(mp.eigsy(Q, eigvals_only=True)) <= 0:
                    return mp.inf, mp.mpf(1)
                L = mp.cholesky(Q)
                bar -= 2 * sum(mp.log(L[i, i]) for i in range(n))
                scale += 2 * sum(abs(mp.log(L[i, i])) for i in range(n))
            return bar, scale


_SCALINGS = {}


def mp_scaling(s, z, n):
    """psdtrianglecone.rs:144-204 in 60 digits on the svec vectors s, z (cached per input for the session)"""
    s, z = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(z, dtype=np.float64)
    key = (n, s.tobytes(), z.tobytes())
    if key not in _SCALINGS:
        with mp.workdps(DPS):
            S, Z = mp_unsvec(s, n), mp_unsvec(z, n)
            L1, L2 = mp.cholesky(S), mp.cholesky(Z)
            U, sig, Vt = mp.svd_r(L2.T * L1)  # = U diag(sig) Vt, sig descending
            lam = [sig[i] for i in range(n)]
            lis = mp_diag([1 / mp.sqrt(v) for v in lam])
            _SCALINGS[key] = Scaling(n, S, Z, L1 * Vt.T * lis, lis * U.T * L2.T, lam)
    return _SCALINGS[key]


def numpy_scaling(s, z, n):
    """the double restatement: oracle/psd_numpy.py -> the cone (R, Rinv, lam, lisqrt) and B"""
    cone = psd_numpy.PSDCone(n)
    assert cone.update_scaling(np.asarray(s, dtype=np.float64), np.asarray(z, dtype=np.float64))
    return cone, cone.R @ cone.R.T


@functools.lru_cache(maxsize=None)
def late_case(n, which):
    """-> dict(s, z, ref (Scaling), E_B, E_lam, E_inv (the invariants' residuals of the double restatement))"""
    S, Z = late_pair(n, which)
    s, z = svec(S), svec(Z)
    ref = mp_scaling(s, z, n)
    cone, Bd = numpy_scaling(s, z, n)
    return dict(n=n, s=s, z=z, ref=ref, E_B=rel_mat(Bd, ref.B), E_lam=rel_vec(cone.lam, ref.lam),
                E_inv=ref.invariants(cone.R, cone.Rinv, cone.lam, Bd), cone=cone)


# ---- matrices with known spectra -------------------------------------------------------------------------------------
def _pow2_parts(n):
    parts, p = [], 1 << (max(n, 1).bit_length() - 1)
    while n:
        if n >= p:
            parts.append(p)
            n -= p
        p >>= 1
    return parts


def _mix_perm(n):
    return np.random.default_rng(4242 + n).permutation(n)


def hadamard_similar(lams):
    """P (H_p diag(.) H_p / p  (+)  ...) P' over the binary decomposition of n, P a fixed permutation: orthogonally
    similar to diag(lams), and exact in double when the lams are multiples of 2^-q bounded by 2^(52 - q) / n"""
    lams = np.asarray(lams, dtype=np.float64)
    n = len(lams)
    A = np.zeros((n, n))
    o = 0
    for p in _pow2_parts(n):
        H = hadamard(p)
        A[o:o + p, o:o + p] = (H * lams[o:o + p]) @ H / p
        o += p
    pm = _mix_perm(n)
    return A[np.ix_(pm, pm)]


def _cycle(vals, n):
    return np.array([vals[i % len(vals)] for i in range(n)], dtype=np.float64)


def spectra_cases(n):
    """-> list of (name, A, eigs): A symmetric n x n, eigs its exact eigenvalues (floats that ARE the exact values, or
    mpf), None where the truth is mpmath's eigsy of the matrix the svec vector defines (n <= 24 only)"""
    out = []
    d = _cycle([3.0, 1.0, 2.0, 2.0, 5.0, 1.0, 4.0], n)
    d[-1] = -1e-14 * d.max() if n > 1 else -1e-14  # the step-length-deciding case: -1e-14 ||A||
    out.append(("diag_tiny_negative", np.diag(d), d))
    out.append(("zero", np.zeros((n, n)), np.zeros(n)))
    out.append(("c_identity", 3.0 * np.eye(n), np.full(n, 3.0)))
    u = _cycle([1.0, -2.0, 3.0, 0.0, 2.0], n)
    out.append(("c_identity_plus_rank1", 2.0 * np.eye(n) + np.outer(u, u), np.array([2.0] * (n - 1) + [2.0 + u @ u])))
    if n >= 2:
        v = _cycle([1.0, -1.0], n)
        if n % 2:
            v[-1] = 0.0
        one, c = np.ones(n), float(v @ v)  # one'v = 0: eigenvalues c + n, c - c = 0 (exactly singular), c
        out.append(("singular_rank2", c * np.eye(n) + np.outer(one, one) - np.outer(v, v),
                    np.array([c] * (n - 2) + [c + n, 0.0])))
        T = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)  # already tridiagonal, analytic spectrum
        with mp.workdps(DPS):
            out.append(("toeplitz_tridiagonal", T, [2 - 2 * mp.cos(mp.pi * (j + 1) / (n + 1)) for j in range(n)]))
    lam_i = _cycle([-3.0, 1.0, 1.0, 4.0, 4.0, 4.0, 7.0, 0.0], n)
    out.append(("hadamard_integer", hadamard_similar(lam_i), lam_i))
    # clusters: half the spectrum at 1, a ladder 1 + j 2^-43 (1.1e-13 apart), the rest at -2^-30 (-9.3e-10)
    nneg = max(1, min(6, n // 4))
    nlad = max(0, min(8, n - nneg - n // 2))
    lam_c = np.array([1.0] * (n - nneg - nlad) + [1.0 + (j + 1) * 2.0 ** -43 for j in range(nlad)] + [-2.0 ** -30] * nneg)
    lam_c = lam_c[np.random.default_rng(99 + n).permutation(n)]
    Ac = hadamard_similar(lam_c)
    out.append(("hadamard_clustered", Ac, lam_c))
    out.append(("hadamard_clustered_2^200", Ac * 2.0 ** 200, lam_c * 2.0 ** 200))
    out.append(("hadamard_clustered_2^-200", Ac * 2.0 ** -200, lam_c * 2.0 ** -200))
    lam_t = np.ones(n)
    lam_t[n // 2] = -2.0 ** -45  # -2.8e-14 ||A||, exact
    out.append(("hadamard_tiny_negative", hadamard_similar(lam_t), lam_t))
    if 4 <= n <= 24:
        Q = orth(n, 300 + n)
        n1 = n // 2
        nng = min(6, n // 4)
        dr = np.array([1.0] * n1 + [1.0 + 1e-13 * (j + 1) for j in range(n - n1 - nng)] + [-1e-9] * nng)
        out.append(("rotated_clustered", sym((Q * dr) @ Q.T), None))
        dt = np.array([1.0] * (n - 1) + [-1e-14])
        out.append(("rotated_tiny_negative", sym((Q * dt) @ Q.T), None))
        W = np.diag(np.abs(np.arange(n) - (n - 1) / 2.0)) + np.eye(n, k=1) + np.eye(n, k=-1)  # Wilkinson W_n^+
        out.append(("wilkinson", W, None))
    return out


@functools.lru_cache(maxsize=None)
def spectra(n):
    """-> list of dict(name, x (svec), norm (||A||_2), emin, esum (floats of the exact smallest eigenvalue and sum of the
    positive ones), E_min, E_sum (errors of the double restatement over ||A||_2))"""
    cases = spectra_cases(n)
    if n == 21:  # the Wilkinson matrix W21+ proper
        cases = [c for c in cases if c[0] == "wilkinson"]
    out = []
    for name, A, eigs in cases:
        x = svec(A)
        with mp.workdps(DPS):
            if eigs is None:
                ev = mp.eigsy(mp_unsvec(x, n), eigvals_only=True)
                ev = [ev[i] for i in range(n)]
            else:
                ev = [mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in eigs]
            emin, esum = min(ev), sum(v for v in ev if v > 0)
            norm = max(abs(v) for v in ev)
            a_np, b_np = psd_numpy.PSDCone(n).margins(x)
            den = norm if norm != 0 else mp.mpf(1)
            E_min, E_sum = float(abs(mp.mpf(a_np) - emin) / den), float(abs(mp.mpf(b_np) - esum) / den)
            out.append(dict(name=name, A=A, x=x, norm=float(norm), emin=float(emin), esum=float(esum), E_min=E_min,
                            E_sum=E_sum, emin_mp=emin, esum_mp=esum))
    return out


EIG_SIZES = (1, 2, 3, 11, 12, 13, 16, 17, 21, 24, 64, 65, 140, 141, 256, 257)
