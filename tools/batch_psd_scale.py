"""Scale run of the batched solver with PSD members (HipBatchSolver(cones="symmetric"), chip_bsym_create) on batches
of a small SDP: the projection of a random symmetric matrix of side --side onto the PSD cone with a linear term,
    min 1/2 x'x + q'x  s.t.  mat(b - x) PSD     (n = m = side (side + 1) / 2, one PSDTriangle cone),
basic_sdp's form at another side: nprob copies of the member of --seed, or with --distinct the members of seed + i.
For every batch size, in ONE process with host clocks around synchronised calls:
setup, solve, iterations, ms per iteration, launches and host synchronisations per iteration; then --single members
solved one by one with HipSolver (setup + solve each), the comparison DESIGN.md 4.13 makes for its members, and the
worst relative difference of x between the batch and those single solves.  Prints one JSON object per batch size and,
with --out FILE, rewrites FILE after every size (a run that is cut short leaves the sizes it finished)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PSD = 6


def small_sdp(side, seed):
    r = np.random.default_rng(seed)
    m = side * (side + 1) // 2
    M = r.standard_normal((side, side))
    M = 0.5 * (M + M.T)
    b = np.array([M[j, k] * (1.0 if j == k else np.sqrt(2.0)) for k in range(side) for j in range(k + 1)])
    eye = sp.identity(m, format="csc")
    csc = lambda A: (A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64))  # noqa: E731
    return dict(n=m, m=m, P=csc(eye), A=csc(eye), q=list(0.1 * r.standard_normal(m)), b=list(b), cones=[(PSD, side)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--side", type=int, default=10)
    ap.add_argument("--seed", type=int, default=301)
    ap.add_argument("--distinct", action="store_true", help="member i from seed + i instead of copies of one member")
    ap.add_argument("--single", type=int, default=16, help="members solved one by one with HipSolver")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    import __graft_entry__ as g
    hip = g.load_package()

    def member(p):
        return (hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"], p["cones"])

    hip.HipBatchSolver([member(small_sdp(a.side, 299))], cones="symmetric").solve()  # warm-up: module load, first launch
    res = {"problem": "small_sdp(side=%d, seed=%d%s): n = m = %d, one PSDTriangle(%d)"
                      % (a.side, a.seed, "+i" if a.distinct else ", copies", a.side * (a.side + 1) // 2, a.side),
           "runs": []}
    for nprob in a.nprob:
        prs = [small_sdp(a.side, a.seed + (i if a.distinct else 0)) for i in range(nprob)]
        mem = [member(p) for p in prs]
        t0 = time.perf_counter()
        bs = hip.HipBatchSolver(mem, cones="symmetric")
        t1 = time.perf_counter()
        sols = bs.solve()
        t2 = time.perf_counter()
        iters = max(s.iterations for s in sols)
        run = {"nprob": nprob, "n": int(bs.stack["n"]), "m": int(bs.stack["m"]), "setup_s": t1 - t0, "solve_s": t2 - t1,
               "iterations_max": iters, "iterations_min": min(s.iterations for s in sols),
               "solved": sum(s.status == "Solved" for s in sols), "iteration_time_s": sols[0].iteration_time,
               "ms_per_iteration": 1e3 * sols[0].iteration_time / max(iters, 1)}
        try:
            it = bs.debug_counter("loop_iterations")
            run["host_syncs_per_iteration"] = bs.debug_counter("host_syncs") / it
            run["launches_per_iteration"] = bs.debug_counter("launches") / it
        except Exception:  # (a library without the test hooks)
            pass
        k = min(a.single, nprob)
        t0 = time.perf_counter()
        singles = []
        for p in mem[:k]:
            singles.append(hip.HipSolver(*p).solve())
        t1 = time.perf_counter()
        run["single_members"] = k
        run["single_one_by_one_s"] = t1 - t0
        run["single_solve_only_s"] = float(sum(s.solve_time - s.setup_time for s in singles))
        run["single_iterations_max"] = max(s.iterations for s in singles)
        run["single_status_equal"] = all(s.status == b.status for s, b in zip(singles, sols))
        run["worst_x_difference"] = max(float(np.max(np.abs(s.x - b.x)) / max(1.0, float(np.max(np.abs(s.x)))))
                                        for s, b in zip(singles, sols))
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        del bs


if __name__ == "__main__":
    main()
