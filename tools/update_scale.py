#!/usr/bin/env python3
"""The L4 data updates (HipSolver.update == chip_problem_*) on the config-3-shaped portfolio problem
(synthetic.portfolio_problem, n = 10^6 at the default size), beside tools/solve_scale.py: setup and a first solve, then
a full q update (new returns, host and device forms), a partial b update (the nblocks risk budgets) and a full A
update (the same values), and the re-solve.  Prints one JSON line: setup_ms, the first solve_ms, the ms of the
handle's first update (one-time allocations included) and the median ms of each form, the re-solve's solve_ms and
iterations, and the residuals of the NEW data's KKT conditions computed on the host from the returned x, s, z.

usage: python tools/update_scale.py [nblocks blocksize]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp

import __graft_entry__ as g


def main():
    import torch  # (shares its HIP runtime with the extension; must be imported first)
    hip = g.load_package()
    import clarabel_rs_amd.synthetic as problems
    if hip.device_count() < 1:
        raise SystemExit("update_scale: no HIP device (the product has no CPU fallback)")
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    nb, bs = (nums + [1000, 1000])[:2] if len(nums) >= 2 else (1000, 1000)
    pr = problems.portfolio_problem(nb, bs, seed=3)
    n, m = pr["n"], pr["m"]
    out = dict(workload="portfolio problem %d x SOC(%d), n=%d, m=%d" % (nb, bs + 1, n, m))
    P = hip.CscMatrix(n, n, *pr["P"])
    A = hip.CscMatrix(m, n, *pr["A"])
    s = hip.HipSolver(P, pr["q"], A, pr["b"], pr["cones"], hip.SolverSettings.default())
    sol = s.solve()
    out.update(setup_ms=round(1e3 * sol.setup_time, 2), solve_ms=round(1e3 * (sol.solve_time - sol.setup_time), 2),
               status=sol.status, iterations=sol.iterations)
    rng = np.random.default_rng(11)
    q2 = -rng.uniform(0.0, 1.0, n)
    ib = (1 + n + (bs + 1) * np.arange(nb)).astype(np.uint64)
    gamma = rng.uniform(1.0, 2.5, nb) / np.sqrt(bs)
    A2 = np.asarray(pr["A"][2], dtype=np.float64)

    def timed(fn, reps=1):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return round(float(np.median(ts)), 3)

    # the first update of a handle allocates its work buffers and staging (once); the forms are then timed as the
    # median of 5 calls each, host arrays in pageable memory (the upload included), and q once more from the device
    out["first_update_ms"] = timed(lambda: s.update_q(q2))
    out["update_q_full_ms"] = timed(lambda: s.update_q(q2), 5)
    out["update_b_partial_ms"] = timed(lambda: s.update_b((ib, gamma)), 5)
    out["update_A_full_ms"] = timed(lambda: s.update_A(A2), 5)
    q2_dev = torch.tensor(q2, dtype=torch.float64, device="cuda")
    out["update_q_full_dev_ms"] = timed(lambda: s.update_q(q2_dev), 5)
    sol2 = s.solve()
    out.update(resolve_ms=round(1e3 * (sol2.solve_time - sol2.setup_time), 2), resolve_status=sol2.status,
               resolve_iterations=sol2.iterations)
    # the KKT conditions of the NEW data, on the host (numpy / scipy only)
    Am = sp.csc_matrix((A2, pr["A"][1], pr["A"][0]), shape=(m, n))
    Pu = sp.csc_matrix((pr["P"][2], pr["P"][1], pr["P"][0]), shape=(n, n))
    Pm = Pu + sp.triu(Pu, 1).T
    b2 = np.asarray(pr["b"], dtype=np.float64).copy()
    b2[ib.astype(np.int64)] = gamma
    x, sv, z = sol2.x, sol2.s, sol2.z
    Ax, Px, Atz = Am @ x, Pm @ x, Am.T @ z
    inf = lambda v: float(np.linalg.norm(v, np.inf))  # noqa: E731
    xPx = float(x @ Px)
    pobj, dobj = 0.5 * xPx + float(q2 @ x), -0.5 * xPx - float(b2 @ z)
    out["host_check"] = dict(
        rel_primal=inf(Ax + sv - b2) / max(1.0, inf(b2), inf(Ax), inf(sv)),
        rel_dual=inf(Px + q2 + Atz) / max(1.0, inf(q2), inf(Px), inf(Atz)),
        rel_gap=abs(pobj - dobj) / max(1.0, min(abs(pobj), abs(dobj))))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
