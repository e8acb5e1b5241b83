#!/usr/bin/env python3
"""Chordal decomposition in the L4 solver (HipSolver with chordal_decomposition_enable) on banded-pattern SDPs
(synthetic.banded_sdp, half-bandwidth 2), beside tools/update_scale.py: for each side, setup (with the host transform
inside it), the iterations and solve time, the device reverse and the PSD completion, with decomposition on and, up to
side 200, off.  Side 1000 and 2000 run with decomposition only: undecomposed, their dense Hs block would need
tri(side)^2 entries (about 1 TB at side 1000).  Prints one JSON line per run.

usage: python tools/chordal_scale.py [side ...]   (default: 120 200 1000 2000)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp

import __graft_entry__ as g

UNDECOMPOSED_MAX_SIDE = 200


def run(hip, pr, side, decompose):
    n, m = pr["n"], pr["m"]
    P = hip.CscMatrix(n, n, *pr["P"])
    A = hip.CscMatrix(m, n, *pr["A"])
    t0 = time.perf_counter()
    s = hip.HipSolver(P, pr["q"], A, pr["b"], pr["cones"],
                      hip.SolverSettings.default(chordal_decomposition_enable=int(decompose)))
    create_ms = 1e3 * (time.perf_counter() - t0)
    sol = s.solve()
    info = s.transform_info()
    Am = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n))
    inf = lambda v: float(np.linalg.norm(v, np.inf))  # noqa: E731
    out = dict(side=side, decomposed=bool(decompose), n=n, m=m, status=sol.status, iterations=sol.iterations,
               obj_val=sol.obj_val, setup_ms=round(1e3 * sol.setup_time, 2), create_ms=round(create_ms, 2),
               transform_ms=round(1e3 * info["transform_time"], 2),
               equilibration_ms=round(1e3 * sol.equilibration_time, 2),
               iteration_ms=round(1e3 * sol.iteration_time, 2),
               ms_per_iteration=round(1e3 * sol.iteration_time / max(1, sol.iterations), 3),
               solve_ms=round(1e3 * (sol.solve_time - sol.setup_time), 2),
               completion_ms=round(1e3 * info["completion_time"], 2),
               n_internal=info["n_internal"], m_internal=info["m_internal"],
               psd_cones_added=info["psd_cones_added"], psd_cones_added_premerge=info["psd_cones_added_premerge"],
               largest_clique=info["largest_clique"],
               rel_primal=inf(Am @ sol.x + sol.s - pr["b"]) / max(1.0, inf(pr["b"])))
    # what the solve spends outside the iterations: default start, the device reverse and the completion
    out["post_ms"] = round(out["solve_ms"] - out["iteration_ms"], 2)
    print(json.dumps(out), flush=True)
    return out


def main():
    import torch  # noqa: F401  (shares its HIP runtime with the extension; must be imported first)
    hip = g.load_package()
    import clarabel_rs_amd.synthetic as problems
    if hip.device_count() < 1:
        raise SystemExit("chordal_scale: no HIP device (the product has no CPU fallback)")
    sides = [int(a) for a in sys.argv[1:] if a.isdigit()] or [120, 200, 1000, 2000]
    for side in sides:
        pr = problems.banded_sdp(side, band=2, seed=1)
        run(hip, pr, side, True)
        if side <= UNDECOMPOSED_MAX_SIDE:
            run(hip, pr, side, False)


if __name__ == "__main__":
    main()
