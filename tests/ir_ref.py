"""Reference trace of the KKT solve's iterative refinement (directldlkktsolver.rs:266-321): no GPU, no package.

trace() restates the loop on a full symmetric K (the oracle's own KKT store after update(): unregularised, as the
reference restores it) with a solve callback (the oracle's factor of the REGULARISED matrix, refinement disabled) and
keeps what the loop throws away: every iterate, every norm, every decision and why the loop ended.  Residuals are
e_i = fsum(b_i, -K_ij x_j ...) per row, each product rounded once, the sum exact (as tests/spmv_ref.py has it), so a
norm of the trace differs from any double evaluation's by at most the row-wise bound
    (L_i + 4) u (|b_i| + sum_j |K_ij x_j|),   L_i the number of terms of row i, u = 2^-53.
margins() tells how far every quantity that decided something is from its threshold, and how far every norm of the trace
is above that bound: a fixture whose margins are large has ONE right sequence of decisions, whatever the order of a
kernel's sums, and so one right iterate to return.

The reference's loop, for it in 0 .. max_iter:
    norme <= abstol + reltol * normb                     -> stop ("tolerance"), x stays
    candidate = x + K_reg^-1 e;  improved = lastnorme / norme(candidate)
    improved < stop_ratio:  accepted iff improved > 1    -> stop ("stop_ratio")
    otherwise accepted (better or not)
and "limit" when the rounds run out.  Refinement switched off: "disabled"."""
import math

import numpy as np

U = 2.0 ** -53


def full_rows(n, colptr, rowval, nzval):
    """rows of the symmetric matrix whose upper triangle is the CSC triple: [(columns, values)] per row"""
    colptr, rowval, nzval = np.asarray(colptr), np.asarray(rowval), np.asarray(nzval, dtype=np.float64)
    cols = np.repeat(np.arange(n), np.diff(colptr))
    off = rowval != cols
    r = np.concatenate([rowval, cols[off]])
    c = np.concatenate([cols, rowval[off]])
    v = np.concatenate([nzval, nzval[off]])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    return [(c[ptr[i]:ptr[i + 1]], v[ptr[i]:ptr[i + 1]]) for i in range(n)]


def residual(rows, b, x):
    """e = b - K x with exactly rounded row sums, and the row-wise rounding bound of any double evaluation of it"""
    n = len(b)
    e, bound = np.zeros(n), np.zeros(n)
    for i, (c, v) in enumerate(rows):
        t = v * x[c]  # (each product rounded once)
        e[i] = math.fsum([b[i]] + (-t).tolist())
        bound[i] = (len(c) + 1 + 4) * U * math.fsum([abs(b[i])] + np.abs(t).tolist())
    return e, bound


def trace(rows, solve, b, enable=True, max_iter=10, reltol=1e-13, abstol=1e-12, stop_ratio=5.0):
    """-> dict(normb, norme0, rounds_list=[(norme, improved, accepted, why_stopped)], iterates=[x_0 ..], bounds=[..],
    accepted=index into iterates, rounds, why_stopped, ok).  why_stopped of a round is None while the loop goes on."""
    b = np.asarray(b, dtype=np.float64)
    x = np.asarray(solve(b), dtype=np.float64)
    out = dict(normb=float(np.max(np.abs(b))), norme0=None, rounds_list=[], iterates=[x], bounds=[], accepted=0, rounds=0,
               why_stopped="disabled", ok=bool(np.all(np.isfinite(x))), tol_checks=[])
    if not enable:
        return out
    e, bound = residual(rows, b, x)
    norme = float(np.max(np.abs(e)))
    out["norme0"] = norme
    out["bounds"].append(float(np.max(bound)))
    if not math.isfinite(norme):
        out["ok"] = False
        return out
    thr = abstol + reltol * out["normb"]
    out["why_stopped"] = "limit"
    for it in range(max_iter):
        out["tol_checks"].append((norme, thr))
        if norme <= thr:
            out["why_stopped"] = "tolerance"
            break
        lastnorme = norme
        cand = x + np.asarray(solve(e), dtype=np.float64)
        e, bound = residual(rows, b, cand)
        norme = float(np.max(np.abs(e)))
        out["iterates"].append(cand)
        out["bounds"].append(float(np.max(bound)))
        out["rounds"] += 1
        if not math.isfinite(norme):
            out["ok"] = False
            return out
        improved = lastnorme / norme
        if improved < stop_ratio:
            accepted = improved > 1.0
            out["rounds_list"].append((norme, improved, accepted, "stop_ratio"))
            out["why_stopped"] = "stop_ratio"
            if accepted:
                x = cand
                out["accepted"] = out["rounds"]
            break
        x = cand
        out["accepted"] = out["rounds"]
        out["rounds_list"].append((norme, improved, True, None))
    why = out["why_stopped"]
    if out["rounds_list"] and out["rounds_list"][-1][3] is None:
        out["rounds_list"][-1] = out["rounds_list"][-1][:3] + (why,)
    return out


def _away(a, b):
    if a == b:
        return 1.0
    if a <= 0.0 or b <= 0.0:
        return math.inf
    return max(a / b, b / a)


def margins(tr, stop_ratio=5.0, **_):
    """-> (decisions, rounding): the smallest factor by which a quantity that DECIDED something is away from its threshold
    (improved against stop_ratio; against 1 where the reference looks at that, below stop_ratio; norme against
    abstol + reltol * normb where that is positive), and the smallest ratio of a norm of the trace to the rounding bound
    of its own residual"""
    dec = math.inf
    for norme, thr in tr["tol_checks"]:
        if thr > 0.0:
            dec = min(dec, _away(norme, thr))
    for norme, improved, _, _ in tr["rounds_list"]:
        if stop_ratio > 0.0:
            dec = min(dec, _away(improved, stop_ratio))
        if improved < stop_ratio:
            dec = min(dec, _away(improved, 1.0))
    norms = ([tr["norme0"]] if tr["norme0"] is not None else []) + [r[0] for r in tr["rounds_list"]]
    rnd = min([nm / bd for nm, bd in zip(norms, tr["bounds"]) if bd > 0.0], default=math.inf)
    return dec, rnd


def separation(iterates, accepted, others=None, visible=None):
    """inf-norm distance from iterates[accepted] to the nearest OTHER iterate (of `others`, default the same list), over
    the first `visible` entries, relative to max(1, |x_acc|_inf)"""
    vis = slice(0, visible)
    xa = iterates[accepted][vis]
    pool = [x for k, x in enumerate(iterates) if k != accepted] if others is None else others
    if not pool:
        return math.inf
    return min(float(np.max(np.abs(x[vis] - xa))) for x in pool) / max(1.0, float(np.max(np.abs(xa))))
