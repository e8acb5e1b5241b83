"""Self-checks of tests/psd_ref.py (the references of tests/test_psd_passes_gpu.py), on the CPU: the mpmath scaling
satisfies its own invariants to 1e-50, the dyadic cases are exact, the claimed spectra are the spectra, and the error E of
the double restatement is computed for every case and lies under its cap -- so that a regenerated input cannot make a
GPU test vacuous.  Also the sizing of the PSD view (host only: the function chip_kkt_create calls)."""
import mpmath as mp
import numpy as np
import pytest

from tests import psd_ref as R

LATE_SIZES = (3, 8, 11, 12, 15, 16, 17, 24)


@pytest.mark.parametrize("which", range(len(R.LATE_SETS)))
@pytest.mark.parametrize("n", LATE_SIZES)
def test_mp_scaling_invariants_and_caps(n, which):
    """the 60-digit scaling of every late pair: R' Z R = Rinv S Rinv' = Lambda, R Rinv = I, B Z B = S to 1e-50; the
    double restatement's error under the cap (measured: E(B) <= 7.5e-14 / 1.2e-11 / 5.2e-10, E(lambda) <= 7.0e-15 /
    1.7e-12 / 1.7e-10 for the three parameter sets)"""
    c = R.late_case(n, which)
    inv = c["ref"].invariants()
    assert max(inv.values()) <= 1e-50, inv
    print("late n=%d set=%d E_B=%.2e E_lam=%.2e gap=%.2e" % (n, which, c["E_B"], c["E_lam"], c["ref"].lam_gap()))
    assert c["E_B"] <= R.E_CAP and c["E_lam"] <= R.E_CAP
    assert max(c["E_inv"].values()) <= R.E_CAP, c["E_inv"]
    k, mu, _ = R.LATE_SETS[which]
    S, Z = R.late_pair(n, which)
    assert np.array_equal(S, S.T) and np.array_equal(Z, Z.T)
    if n > 1:
        assert 0.5 * 10.0 ** (2 * k) <= np.linalg.cond(S) <= 2.0 * 10.0 ** (2 * k)
    assert abs(np.linalg.slogdet(S)[1] + np.linalg.slogdet(Z)[1] - n * np.log(mu)) <= 1e-6 * n  # det(S Z) = mu^n


@pytest.mark.parametrize("n", [64, 128])
def test_hadamard_pair_is_exact(n):
    """S, Z, B of the dyadic cases against integer arithmetic: entries exact in double, B Z B = S exactly, lambda^2 the
    eigenvalues of ... = 4^(k + m); repeated exponents give clusters"""
    S, Z, B, lam = R.hadamard_pair(n)
    H = R.hadamard(n).astype(np.int64)
    i = np.arange(n)
    k, m = (i % 5) - 2, ((i // 3) % 4) - 1
    Si = (H * (4 ** (k + 2))) @ H            # = 16 n S
    Zi = (H * (4 ** (m + 1))) @ H            # = 4 n Z
    Bi = (H * (2 ** (k - m + 4))) @ H        # = 16 n B
    assert np.array_equal(S * (16 * n), Si) and np.array_equal(Z * (4 * n), Zi) and np.array_equal(B * (16 * n), Bi)
    # (16 n B)(4 n Z)(16 n B) = 1024 n^3 B Z B = 1024 n^3 S = 64 n^2 (16 n S)
    assert np.array_equal(Bi @ Zi @ Bi, 64 * n * n * Si)
    assert np.array_equal(np.sort(lam), np.sort(2.0 ** (k + m))) and len(set(lam.tolist())) < n // 4
    assert np.all(np.linalg.eigvalsh(S) > 0) and np.all(np.linalg.eigvalsh(Z) > 0)


@pytest.mark.parametrize("n", R.EIG_SIZES)
def test_spectra_are_what_they_claim(n):
    """every matrix with a claimed spectrum: exact construction where claimed (integer arithmetic), the spectrum itself
    against mpmath's eigsy up to side 24 and against LAPACK beyond; E of the double restatement for every case"""
    for name, A, eigs in R.spectra_cases(n):
        assert np.array_equal(A, A.T), name
        if eigs is None:
            continue
        if name.startswith("hadamard"):
            sc = 2.0 ** 45 if "clustered" in name or "tiny" in name else 1.0
            if "2^200" in name:
                sc *= 2.0 ** -200
            elif "2^-200" in name:
                sc *= 2.0 ** 200
            li = np.asarray(eigs, dtype=np.float64) * sc
            assert np.array_equal(li, np.round(li))
            li, Ai, o = li.astype(np.int64), np.zeros((n, n), dtype=np.int64), 0
            pm = R._mix_perm(n)
            scale = np.zeros(n)
            for p in R._pow2_parts(n):
                Hp = R.hadamard(p).astype(np.int64)
                Ai[o:o + p, o:o + p] = (Hp * li[o:o + p]) @ Hp
                scale[o:o + p] = p
                o += p
            Ai, scale = Ai[np.ix_(pm, pm)], scale[pm]
            assert np.array_equal(A * sc * scale[:, None], Ai.astype(np.float64)), name
        ev = np.sort(np.array([float(v) for v in eigs]))
        if n <= 24:
            with mp.workdps(R.DPS):
                ref = mp.eigsy(R.mp_mat(A), eigvals_only=True)
                want = sorted(mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in eigs)
                nrm = max(abs(v) for v in want) or 1
                assert max(abs(ref[i] - want[i]) for i in range(n)) <= mp.mpf(10) ** -45 * nrm, name
        else:
            nrm = np.max(np.abs(ev)) or 1.0
            assert np.max(np.abs(np.linalg.eigvalsh(A) - ev)) <= 64 * n * R.U53 * nrm, name
    for c in R.spectra(n):
        print("spectrum n=%d %-26s E_min=%.2e E_sum=%.2e (n 2^-53 = %.2e)" % (n, c["name"], c["E_min"], c["E_sum"],
                                                                              n * R.U53))
        assert c["E_min"] <= 1e-12 and c["E_sum"] <= 1e-11, c["name"]


def test_psd_view_sizing(hip):
    """the sizing chip_kkt_create uses for its PSD cones: state of 3 n^2 + 2 n doubles per cone, and ONE decision for all
    cones of a view -- a largest side above 64 moves the work matrices of every cone to HBM scratch slices of
    4 maxdim^2 + 4 maxdim + 16 doubles"""
    for dims, gs in (([1], 0), ([2, 12, 16, 64], 0), ([64], 0), ([65], 1), ([3, 70], 1), ([11, 101, 144], 1), ([257], 1)):
        d = hip.PsdConesDebug(dims)
        mx = max(dims)
        assert d.counter("gs") == gs and d.counter("maxdim") == mx
        assert d.counter("rows") == sum(n * (n + 1) // 2 for n in dims)
        assert d.counter("state_doubles") == sum(3 * n * n + 2 * n for n in dims)
        assert d.counter("scratch_stride") == (4 * mx * mx + 4 * mx + 16 if gs else 0)
        assert d.counter("jacobi_lds") == 0  # nothing launched
    e = hip.PsdConesDebug([0])  # the cone constructor accepts an empty cone (psdtrianglecone.rs:151-154 bails early)
    assert e.rows == 0 and e.counter("gs") == 0
    with pytest.raises(hip.ChipError):
        hip.PsdConesDebug([])
    with pytest.raises(hip.ChipError):
        hip.PsdConesDebug([-1])
