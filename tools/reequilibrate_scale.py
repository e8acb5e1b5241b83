"""Scale run of the re-equilibration (HipSolver.reequilibrate / HipBatchSolver.reequilibrate) on config 4's batch
(nprob members synthetic.portfolio_problem(2, 1000, seed=100+i)) and on the config-3 problem
(synthetic.portfolio_problem(1000, 1000, seed=3)).  In ONE process per workload, with host clocks around calls that end
in a synchronisation and after one warm-up call (the first call allocates the handle's work buffers): the call from
pageable host memory and from device tensors, medians of --repeats, beside the create of a fresh handle on the same
data.  The data is a drifted copy of the handle's: rows of A / b and columns of P / q / A times powers of two drawn from
2^-20 .. 2^20 (one factor per second-order cone).  On it, the iterations and statuses of three solves: with the stale
scalings (plain full updates), re-equilibrated, and on a fresh handle.  Prints one JSON object; --out FILE also writes
it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOC = 2


def drifted(pr, seed):
    """(P.nzval, q, A.nzval, b) of pr in other coordinates: A <- R A C, b <- R b, P <- C P C, q <- C q"""
    rng = np.random.default_rng(seed)
    n = pr["n"]
    col = np.ldexp(1.0, rng.integers(-20, 21, n))
    row = []
    for c in pr["cones"]:
        e = rng.integers(-20, 21, 1 if c[0] == SOC else c[1])
        row.append(np.ldexp(1.0, np.repeat(e, c[1]) if c[0] == SOC else e))
    row = np.concatenate(row) if row else np.zeros(0)
    cols_of = lambda p: np.repeat(np.arange(n), np.diff(np.asarray(p, dtype=np.int64)))  # noqa: E731
    (Pp, Pi, Px), (Ap, Ai, Ax) = pr["P"], pr["A"]
    Pi, Ai = np.asarray(Pi, dtype=np.int64), np.asarray(Ai, dtype=np.int64)
    return (np.asarray(Px, float) * col[Pi] * col[cols_of(Pp)], np.asarray(pr["q"], float) * col,
            np.asarray(Ax, float) * row[Ai] * col[cols_of(Ap)], np.asarray(pr["b"], float) * row)


def with_values(pr, v):
    return dict(pr, P=(pr["P"][0], pr["P"][1], v[0]), q=v[1], A=(pr["A"][0], pr["A"][1], v[2]), b=v[3])


def solve_figures(sols):
    sols = sols if isinstance(sols, list) else [sols]
    status = {}
    for s in sols:
        status[s.status] = status.get(s.status, 0) + 1
    return {"iterations_max": max(s.iterations for s in sols), "iterations_min": min(s.iterations for s in sols),
            "statuses": status, "iteration_time_s": sols[0].iteration_time}


def run(make, stacked, prs, repeats):
    import torch

    def clock(fn):
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * float(np.median(ts))}

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0
    prs2 = [with_values(p, drifted(p, 500 + i)) for i, p in enumerate(prs)]
    y = stacked(prs2)
    yd = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in y]
    torch.cuda.synchronize()
    h, t_create = timed(lambda: make(prs))
    sols, t_solve = timed(h.solve)
    res = {"first": dict(solve_figures(sols), setup_s=t_create, solve_s=t_solve),
           "values": {k: int(len(v)) for k, v in zip("PqAb", y)}}
    _, t_upd = timed(lambda: h.update(P=y[0], q=y[1], A=y[2], b=y[3]))
    sols, t_solve = timed(h.solve)
    res["stale_scalings"] = dict(solve_figures(sols), update_s=t_upd, solve_s=t_solve)
    _, t_first = timed(lambda: h.reequilibrate(*y))  # warm-up: the work buffers and the staging are allocated here
    res["reequilibrate"] = {"first_call_ms": 1e3 * t_first, "host": clock(lambda: h.reequilibrate(*y)),
                            "device": clock(lambda: h.reequilibrate(*yd))}
    if hasattr(h, "debug_counter"):
        res["reequilibrate"]["enqueues"] = h.debug_counter("update_launches")
        res["reequilibrate"]["host_syncs"] = h.debug_counter("update_host_syncs")
    sols, t_solve = timed(h.solve)
    res["reequilibrated"] = dict(solve_figures(sols), solve_s=t_solve)
    del h
    f, t_create = timed(lambda: make(prs2))
    sols, t_solve = timed(f.solve)
    res["fresh_on_drifted_data"] = dict(solve_figures(sols), setup_s=t_create, solve_s=t_solve)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=1000, help="the config-3 problem's number of blocks")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (shares its HIP runtime with the extension; must be imported first)
    import __graft_entry__ as g
    hip = g.load_package()
    from clarabel_rs_amd import synthetic
    if hip.device_count() < 1:
        raise SystemExit("reequilibrate_scale: no HIP device (the product has no CPU fallback)")
    mem = lambda p: (hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"],  # noqa: E731
                     p["cones"])
    vals = lambda p: (np.asarray(p["P"][2], float), np.asarray(p["q"], float), np.asarray(p["A"][2], float),  # noqa: E731
                      np.asarray(p["b"], float))
    res = {}
    prs = [synthetic.portfolio_problem(2, 1000, seed=100 + i) for i in range(a.nprob)]
    res["config4_batch"] = dict(
        run(lambda ps: hip.HipBatchSolver([mem(p) for p in ps]),
            lambda ps: tuple(np.concatenate([vals(p)[i] for p in ps]) for i in range(4)), prs, a.repeats),
        problem="portfolio_problem(2, 1000, seed=100+i)", nprob=a.nprob)
    del prs
    pr = synthetic.portfolio_problem(a.blocks, 1000, seed=3)
    res["config3_single"] = dict(run(lambda ps: hip.HipSolver(*mem(ps[0])), lambda ps: vals(ps[0]), [pr], a.repeats),
                                 problem="portfolio_problem(%d, 1000, seed=3)" % a.blocks, n=pr["n"], m=pr["m"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
