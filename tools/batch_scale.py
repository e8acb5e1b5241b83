"""Scale run of the batched L4 solver (HipBatchSolver) on config 4's member problem,
synthetic.portfolio_problem(2, 1000, seed=100+i) (n = 2000, m = 4003): setup time, iterations (max over members), solve
time and milliseconds per iteration for nprob in {1, 16, 256, 1024}, and the time of solving 16 of the same members one
by one with HipSolver.  Prints one JSON object; --out FILE also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256,1024")
    ap.add_argument("--singles", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    hip = g.load_package()
    from clarabel_rs_amd import synthetic
    sizes = [int(v) for v in a.sizes.split(",")]
    prs = [synthetic.portfolio_problem(2, 1000, seed=100 + i) for i in range(max(sizes + [a.singles]))]
    mem = [(hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"], p["cones"])
           for p in prs]
    res = {"problem": "portfolio_problem(2, 1000, seed=100+i)", "n": prs[0]["n"], "m": prs[0]["m"], "batch": []}
    for k in sizes:
        t0 = time.perf_counter()
        bs = hip.HipBatchSolver(mem[:k])
        t1 = time.perf_counter()
        sols = bs.solve()
        t2 = time.perf_counter()
        its = max(s.iterations for s in sols)
        res["batch"].append({"nprob": k, "setup_s": t1 - t0, "solve_s": t2 - t1, "iterations_max": its,
                             "ms_per_iteration": 1e3 * sols[0].iteration_time / max(its, 1),
                             "solved": sum(s.status == "Solved" for s in sols)})
        print(json.dumps(res["batch"][-1]), file=sys.stderr)
        del bs
    t0 = time.perf_counter()
    for P, q, A, b, cones in mem[:a.singles]:
        hip.HipSolver(P, q, A, b, cones).solve()
    res["singles"] = {"count": a.singles, "setup_and_solve_s": time.perf_counter() - t0}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
