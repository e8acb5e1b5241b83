#!/usr/bin/env python3
"""The whole solve through the L4 entry point (HipSolver == chip_solver_*: device equilibration, the interior-point
loop, termination, unscaling) on the config-3-shaped portfolio problem (synthetic.portfolio_problem, n = 10^6 at the
default size), beside tools/ipm_scale.py, which runs the same loop as a Python harness with identity equilibration.
Prints one JSON line: setup / equilibration ms, iterations, ms per iteration, status, and the residuals of the
UNEQUILIBRATED KKT conditions computed on the host from the returned x, s, z.

usage: python tools/solve_scale.py [nblocks blocksize] [--max-iter K]"""
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
    import torch  # noqa: F401  (shares its HIP runtime with the extension; must be imported first)
    hip = g.load_package()
    import clarabel_rs_amd.synthetic as problems
    if hip.device_count() < 1:
        raise SystemExit("solve_scale: no HIP device (the product has no CPU fallback)")
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    nb, bs = (nums + [1000, 1000])[:2] if len(nums) >= 2 else (1000, 1000)
    kw = {}
    if "--max-iter" in sys.argv:
        kw["max_iter"] = int(sys.argv[sys.argv.index("--max-iter") + 1])
    t0 = time.time()
    pr = problems.portfolio_problem(nb, bs, seed=3)
    out = dict(workload="portfolio problem %d x SOC(%d), n=%d, m=%d" % (nb, bs + 1, pr["n"], pr["m"]),
               generate_s=round(time.time() - t0, 2))
    n, m = pr["n"], pr["m"]
    P = hip.CscMatrix(n, n, *pr["P"])
    A = hip.CscMatrix(m, n, *pr["A"])
    s = hip.HipSolver(P, pr["q"], A, pr["b"], pr["cones"], hip.SolverSettings.default(**kw))
    sol = s.solve()
    loop_s = sol.iteration_time  # (the loop alone, as tools/ipm_scale.py's loop_ms)
    out.update(status=sol.status, iterations=sol.iterations, setup_ms=round(1e3 * sol.setup_time, 2),
               equilibration_ms=round(1e3 * sol.equilibration_time, 3),
               solve_ms=round(1e3 * (sol.solve_time - sol.setup_time), 2), loop_ms=round(1e3 * loop_s, 2),
               ms_per_iteration=round(1e3 * loop_s / max(1, sol.iterations), 3), obj_val=sol.obj_val,
               r_prim=sol.r_prim, r_dual=sol.r_dual)
    # the KKT conditions of the ORIGINAL data, on the host (numpy / scipy only)
    Am = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n))
    Pu = sp.csc_matrix((pr["P"][2], pr["P"][1], pr["P"][0]), shape=(n, n))
    Pm = Pu + sp.triu(Pu, 1).T
    q, b = np.asarray(pr["q"]), np.asarray(pr["b"])
    x, sv, z = sol.x, sol.s, sol.z
    Ax, Px, Atz = Am @ x, Pm @ x, Am.T @ z
    inf = lambda v: float(np.linalg.norm(v, np.inf))  # noqa: E731
    xPx = float(x @ Px)
    pobj, dobj = 0.5 * xPx + float(q @ x), -0.5 * xPx - float(b @ z)
    out["host_check"] = dict(
        rel_primal=inf(Ax + sv - b) / max(1.0, inf(b), inf(Ax), inf(sv)),
        rel_dual=inf(Px + q + Atz) / max(1.0, inf(q), inf(Px), inf(Atz)),
        rel_gap=abs(pobj - dobj) / max(1.0, min(abs(pobj), abs(dobj))))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
