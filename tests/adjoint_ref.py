"""The numpy restatement (dense, unscaled) of the gradients of a conic QP's solution with respect to its data, for
Zero / Nonnegative cones -- what chip_bgrad_* computes on the device.

Problem: min 1/2 x'Px + q'x  s.t.  Ax + s = b, s in K, multipliers z.  At a solution (x, s, z), with
H = diag(s_i / z_i) on the Nonnegative rows and 0 on the Zero rows, K = [P A'; A -H], and the incoming gradients
gx, gz, gs of a loss with respect to x, z, s:

    [vx; vz] = K^-1 [gx - A' gs; gz]
    dL/dq = -vx
    dL/db =  vz + gs
    dL/dA_ij = -(z_i vx_j + vz_i x_j) - gs_i x_j          on A's pattern
    dL/dP_ij = -(vx_i x_j + vx_j x_i)  (i < j),  -vx_i x_i  (i = j)   on P's stored triu pattern

Also here: the problems the gradient tests share (the random QPs of the issue, rebuilt from their seeds) and the
finite differences of the CPU oracle's interior-point loop they are checked against."""
import os

import numpy as np
import scipy.sparse as sp

from tests import e2e_problems as E

ZERO, NN, SOC = 0, 1, 2


def dense(pr):
    n, m = pr["n"], pr["m"]
    Pu = sp.csc_matrix((pr["P"][2], pr["P"][1], pr["P"][0]), shape=(n, n))
    P = (Pu + sp.triu(Pu, 1).T).toarray()
    A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n)).toarray()
    return P, A


def hmat(cones, s, z):
    H = np.zeros((len(s), len(s)))
    k = 0
    for c in cones:
        sl = slice(k, k + c[1])
        if c[0] == NN:
            H[sl, sl] = np.diag(s[sl] / z[sl])
        elif c[0] != ZERO:
            raise ValueError("adjoint_ref: Zero and Nonnegative cones only")
        k += c[1]
    return H


def on_pattern(pat, dense_mat):
    """the entries of a dense matrix on a CSC pattern (colptr, rowval, ...), in nzval order"""
    colptr, rowval = np.asarray(pat[0]), np.asarray(pat[1])
    out = np.zeros(len(rowval))
    for col in range(len(colptr) - 1):
        for p in range(colptr[col], colptr[col + 1]):
            out[p] = dense_mat[rowval[p], col]
    return out


def adjoint(pr, x, s, z, gx=None, gz=None, gs=None):
    """-> dq[n], db[m], dP[nnz(P)], dA[nnz(A)] (the matrices on the stored patterns, nzval order)"""
    n, m = pr["n"], pr["m"]
    x, s, z = (np.asarray(v, dtype=float) for v in (x, s, z))
    gx = np.zeros(n) if gx is None else np.asarray(gx, dtype=float)
    gz = np.zeros(m) if gz is None else np.asarray(gz, dtype=float)
    gs = np.zeros(m) if gs is None else np.asarray(gs, dtype=float)
    P, A = dense(pr)
    K = np.block([[P, A.T], [A, -hmat(pr["cones"], s, z)]])
    v = np.linalg.solve(K, np.concatenate([gx - A.T @ gs, gz]))
    vx, vz = v[:n], v[n:]
    dq = -vx
    db = vz + gs
    dA = -(np.outer(z, vx) + np.outer(vz, x)) - np.outer(gs, x)
    dPfull = -np.outer(vx, x)
    dPu = np.triu(dPfull + dPfull.T) - np.diag(np.diag(dPfull))  # a stored entry (i < j) stands for both triangles
    return dq, db, on_pattern(pr["P"], dPu), on_pattern(pr["A"], dA)


def rel(a, f):
    """max abs difference / max(1, max abs reference)"""
    a, f = np.asarray(a, dtype=float), np.asarray(f, dtype=float)
    if not f.size:
        return 0.0
    return float(np.max(np.abs(a - f)) / max(1.0, float(np.max(np.abs(f)))))


# ---- the problems -------------------------------------------------------------------------------------------------
def random_qp(seed):
    """n = 8, 2 Zero + 12 Nonnegative rows, P = MM' + I, b = A x0 + [0; 0.3 |g|]: strictly feasible, strictly
    complementary for the seeds 1, 2, 3"""
    r = np.random.default_rng(seed)
    M = r.standard_normal((8, 8))
    A = r.standard_normal((14, 8))
    x0 = r.standard_normal(8)
    b = A @ x0
    b[2:] += 0.3 * np.abs(r.standard_normal(12))
    q = r.standard_normal(8)
    P = M @ M.T + np.eye(8)
    return dict(n=8, m=14, P=E._triu(P), A=E._csc(A), q=list(q), b=list(b), cones=[(ZERO, 2), (NN, 12)])


def hs35():
    from tests import json_problem
    return json_problem.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hs35.json"))


def fd_problems():
    """the six problems the formulas are checked on against finite differences"""
    return [("basic_lp", E.basic_lp()), ("basic_eq_constrained", E.basic_eq_constrained()), ("hs35", hs35()),
            ("random_qp_1", random_qp(1)), ("random_qp_2", random_qp(2)), ("random_qp_3", random_qp(3))]


def gpu_members():
    """the members of the device tests: the six above and basic_unconstrained (no rows at all)"""
    pr = fd_problems()
    return pr[:3] + [("basic_unconstrained", E.basic_unconstrained())] + pr[3:]


def incoming(pr, seed):
    r = np.random.default_rng(seed)
    return r.standard_normal(pr["n"]), r.standard_normal(pr["m"]), r.standard_normal(pr["m"])


# ---- finite differences of a solve ---------------------------------------------------------------------------------
def loss(out, gx, gz, gs):
    return float(gx @ out["x"] + gz @ out["z"] + gs @ out["s"])


def finite_differences(solve, pr, gx, gz, gs, h=1e-4, keys="qbAP"):
    """central differences of loss(solve(q=, b=, A=, P=)) in every entry of the pieces named in `keys`; solve takes
    the four pieces as keywords (matrices as (colptr, rowval, nzval)) and returns a dict with x, s, z"""
    base = dict(q=np.array(pr["q"], dtype=float), b=np.array(pr["b"], dtype=float), A=pr["A"], P=pr["P"])
    out = {}
    for key in keys:
        mat = key in "AP"
        v0 = np.array(base[key][2] if mat else base[key], dtype=float)
        g = np.zeros(len(v0))
        for i in range(len(v0)):
            vals = []
            for sgn in (1.0, -1.0):
                v = v0.copy()
                v[i] += sgn * h
                piece = (base[key][0], base[key][1], v) if mat else v
                vals.append(loss(solve(**dict(base, **{key: piece})), gx, gz, gs))
            g[i] = (vals[0] - vals[1]) / (2 * h)
        out[key] = g
    return out
