"""The numpy restatement (dense, unscaled) of the forward-mode derivative of a conic QP's solution with respect to
its data, for Zero / Nonnegative cones -- what chip_bjvp_* computes on the device; the transpose of
tests/adjoint_ref.py.

Problem: min 1/2 x'Px + q'x  s.t.  Ax + s = b, s in K, multipliers z.  At a solution (x, s, z), with
H = diag(s_i / z_i) on the Nonnegative rows and 0 on the Zero rows, K = [P A'; A -H], and a direction dq, db, dP (values
on P's stored triu pattern; a stored (i, j), i < j, stands for both triangles: dP_sym) and dA (values on A's pattern):

    rx = -(dq + dP_sym x + dA' z)        rz = db - dA x
    [dx; dz] = K^-1 [rx; rz]
    ds = rz - A dx   on the Nonnegative rows, an exact +0.0 on the Zero rows

Also here: wide_qp, a QP whose rows are longer than a wavefront (the other shared problems are adjoint_ref's)."""
import numpy as np
import scipy.sparse as sp

from tests import adjoint_ref as R
from tests import e2e_problems as E

ZERO, NN = R.ZERO, R.NN


def direction_matrices(pr, dP, dA):
    """the dense dP_sym and dA of the values on the stored patterns (None = zeros)"""
    n, m = pr["n"], pr["m"]
    if dP is None:
        dPs = np.zeros((n, n))
    else:
        U = sp.csc_matrix((np.asarray(dP, dtype=float), pr["P"][1], pr["P"][0]), shape=(n, n))
        dPs = (U + sp.triu(U, 1).T).toarray()
    if dA is None:
        dAd = np.zeros((m, n))
    else:
        dAd = sp.csc_matrix((np.asarray(dA, dtype=float), pr["A"][1], pr["A"][0]), shape=(m, n)).toarray()
    return dPs, dAd


def nn_rows(pr):
    mask = np.zeros(pr["m"], dtype=bool)
    k = 0
    for c in pr["cones"]:
        if c[0] == NN:
            mask[k:k + c[1]] = True
        k += c[1]
    return mask


def tangent(pr, x, s, z, dq=None, db=None, dP=None, dA=None):
    """-> dx[n], dz[m], ds[m]"""
    n, m = pr["n"], pr["m"]
    x, s, z = (np.asarray(v, dtype=float) for v in (x, s, z))
    dq = np.zeros(n) if dq is None else np.asarray(dq, dtype=float)
    db = np.zeros(m) if db is None else np.asarray(db, dtype=float)
    dPs, dAd = direction_matrices(pr, dP, dA)
    P, A = R.dense(pr)
    K = np.block([[P, A.T], [A, -R.hmat(pr["cones"], s, z)]])
    rx = -(dq + dPs @ x + dAd.T @ z)
    rz = db - dAd @ x
    v = np.linalg.solve(K, np.concatenate([rx, rz]))
    dx, dz = v[:n], v[n:]
    ds = np.where(nn_rows(pr), rz - A @ dx, 0.0)
    return dx, dz, ds


def direction(pr, seed):
    """one random direction in all four pieces"""
    r = np.random.default_rng(seed)
    return (r.standard_normal(pr["n"]), r.standard_normal(pr["m"]), r.standard_normal(len(pr["P"][2])),
            r.standard_normal(len(pr["A"][2])))


def wide_qp(seed):
    """n = 70, 3 Zero + 20 Nonnegative rows; two rows of A, one column of A and one row / column of P are dense, so
    the rows the device sums are longer than a wavefront.  Strictly feasible; strictly complementary for the seeds
    1, 2, 3."""
    r = np.random.default_rng(seed)
    n, nz, nn = 70, 3, 20
    m = nz + nn
    A = np.zeros((m, n))
    mask = r.random((m, n)) < 0.15
    A[mask] = r.standard_normal(mask.sum())
    A[0, :] = r.standard_normal(n)
    A[nz, :] = r.standard_normal(n)
    A[:, 5] = r.standard_normal(m)
    M = np.zeros((n, n))
    mk = r.random((n, n)) < 0.05
    M[mk] = r.standard_normal(mk.sum())
    P = M @ M.T + np.eye(n)
    P[0, :] = 0.1 * r.standard_normal(n)
    P[:, 0] = P[0, :]
    P[0, 0] = 5.0 + 0.1 * n
    x0 = r.standard_normal(n)
    b = A @ x0
    b[nz:] += 0.3 * np.abs(r.standard_normal(nn))
    q = r.standard_normal(n)
    return dict(n=n, m=m, P=E._triu(P), A=E._csc(A), q=list(q), b=list(b), cones=[(ZERO, nz), (NN, nn)])


def host_problems():
    """the nine problems the formulas are checked on: adjoint_ref's six and the wide QPs"""
    return R.fd_problems() + [("wide_qp_%d" % s, wide_qp(s)) for s in (1, 2, 3)]


def gpu_members():
    """the members of the device tests: adjoint_ref's seven and wide_qp(1)"""
    return R.gpu_members() + [("wide_qp_1", wide_qp(1))]
