"""Scale run of the batched solver's data updates (HipBatchSolver.update) on config 4's batch: nprob members
synthetic.portfolio_problem(2, 1000, seed=100+i).  In ONE process, with host clocks around synchronised calls and after
one warm-up update (the first update allocates the handle's work buffers): a full q from the host and from the device,
a partial b with one entry per member, a full A; then update + re-solve against create + solve of a fresh handle on
the same new data.  Prints one JSON object; --out FILE also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    hip = g.load_package()
    from clarabel_rs_amd import synthetic
    nprob, nblocks, dim = a.nprob, 2, 1001
    prs = [synthetic.portfolio_problem(nblocks, 1000, seed=100 + i) for i in range(nprob)]
    mem = lambda ps: [(hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]),  # noqa: E731
                       p["b"], p["cones"]) for p in ps]

    def clock(fn, repeats=a.repeats):
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * float(np.median(ts))}

    t0 = time.perf_counter()
    bs = hip.HipBatchSolver(mem(prs))
    t1 = time.perf_counter()
    sols = bs.solve()
    t2 = time.perf_counter()
    res = {"problem": "portfolio_problem(2, 1000, seed=100+i)", "nprob": nprob, "n": bs.stack["n"], "m": bs.stack["m"],
           "nnzA": len(bs.stack["A"][2]),
           "first": {"setup_s": t1 - t0, "solve_s": t2 - t1, "iterations_max": max(s.iterations for s in sols),
                     "solved": sum(s.status == "Solved" for s in sols)}}
    # the new data: new returns and risk budgets per member (tests/test_batch_update_gpu.py's recipe)
    zoff = np.concatenate([[0], np.cumsum(bs.m_part)]).astype(np.int64)
    q2, ib, gam = [], [], []
    for i, pr in enumerate(prs):
        rng = np.random.default_rng(77 + i)
        q2.append(-rng.uniform(0.0, 1.0, pr["n"]))
        ib.append(zoff[i] + 1 + pr["n"] + dim * np.arange(nblocks))
        gam.append(rng.uniform(1.0, 2.5, nblocks) / np.sqrt(1000))
    q2s, ibs, gams = np.concatenate(q2), np.concatenate(ib), np.concatenate(gam)
    q2d = torch.tensor(q2s, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    A0 = bs.stack["A"][2].copy()
    b_one = (zoff[:-1].copy(), np.full(nprob, float(nblocks)))  # one entry per member: its budget row, unchanged
    bs.update_q(bs.stack["q"])  # warm-up
    res["updates"] = {"q_full_host": clock(lambda: bs.update_q(q2s)), "q_full_device": clock(lambda: bs.update_q(q2d)),
                      "b_partial_one_per_member": clock(lambda: bs.update_b(b_one)),
                      "A_full_host": clock(lambda: bs.update_A(A0))}
    runs = []
    for _ in range(2):  # update + re-solve, twice (the same data the second time)
        t0 = time.perf_counter()
        bs.update(q=q2d, b=(ibs, gams))
        t1 = time.perf_counter()
        sols = bs.solve()
        t2 = time.perf_counter()
        runs.append({"update_s": t1 - t0, "solve_s": t2 - t1, "iterations_max": max(s.iterations for s in sols),
                     "iteration_time_s": sols[0].iteration_time,
                     "solved": sum(s.status == "Solved" for s in sols)})
    res["update_and_resolve"] = runs
    del bs
    prs2 = []
    for i, pr in enumerate(prs):
        b2 = np.asarray(pr["b"], float).copy()
        b2[ib[i] - zoff[i]] = gam[i]
        prs2.append(dict(pr, q=q2[i], b=b2))
    m2 = mem(prs2)
    t0 = time.perf_counter()
    fresh = hip.HipBatchSolver(m2)
    t1 = time.perf_counter()
    sols = fresh.solve()
    t2 = time.perf_counter()
    res["fresh_on_new_data"] = {"setup_s": t1 - t0, "solve_s": t2 - t1,
                                "iterations_max": max(s.iterations for s in sols),
                                "iteration_time_s": sols[0].iteration_time,
                                "solved": sum(s.status == "Solved" for s in sols)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
