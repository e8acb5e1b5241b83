"""Scale run of the batched solver's gradients (HipBatchSolver.backward) on batches of the long-only factor-model
portfolio QP synthetic.portfolio_qp(n_assets, n_factors, seed=200+i): for every batch size, in ONE process with host
clocks around synchronised calls: setup, solve, iterations, ms per iteration, ms per backward with host and with device
inputs (after one warm-up backward: the first one allocates the handle's gradient buffers), and the worst relative
difference of the gradients against the dense numpy restatement tests/adjoint_ref.py on up to 8 sampled members,
evaluated at the device's own solution.  The output also carries the figures the GPU tests measured on their small
members (the MEASURED_* constants of tests/test_batch_adjoint_gpu.py), so that they sit beside the figures at scale.
Prints one JSON object per batch size and, with --out FILE, rewrites FILE after every size (a run that is cut short
leaves the sizes it finished)."""
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
    ap.add_argument("--nprob", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--assets", type=int, default=2000)
    ap.add_argument("--factors", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", type=int, default=8, help="members compared with the dense restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    hip = g.load_package()
    from clarabel_rs_amd import synthetic
    from tests import adjoint_ref as R

    def clock(fn):
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * float(np.median(ts))}

    # beside the runs: the figures tests/test_batch_adjoint_gpu.py measured on the small members and asserts 10 x of
    from tests import test_batch_adjoint_gpu as T
    res = {"problem": "portfolio_qp(%d, %d, seed=200+i)" % (a.assets, a.factors),
           "gpu_test_measured": {"source": "the constants of tests/test_batch_adjoint_gpu.py",
                                 "gradients_vs_adjoint_ref": T.MEASURED_GRAD,
                                 "dq_db_vs_finite_differences": T.MEASURED_FD,
                                 "permuted_vs_ordered_batch": T.MEASURED_PERM,
                                 "two_backwards_of_one_solve": T.MEASURED_REPEAT},
           "runs": []}
    for nprob in a.nprob:
        prs = [synthetic.portfolio_qp(a.assets, a.factors, seed=200 + i) for i in range(nprob)]
        mem = [(hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"],
                p["cones"]) for p in prs]
        t0 = time.perf_counter()
        bs = hip.HipBatchSolver(mem)
        t1 = time.perf_counter()
        sols = bs.solve()
        t2 = time.perf_counter()
        iters = max(s.iterations for s in sols)
        n, m = bs.stack["n"], bs.stack["m"]
        rng = np.random.default_rng(1)
        gx, gz, gs = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
        dgx, dgz, dgs = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in (gx, gz, gs)]
        torch.cuda.synchronize()
        grad = bs.backward(gx, gz, gs)  # warm-up, and the result that is checked
        run = {"nprob": nprob, "n": n, "m": m, "nnzP": len(bs.stack["P"][2]), "nnzA": len(bs.stack["A"][2]),
               "setup_s": t1 - t0, "solve_s": t2 - t1, "iterations_max": iters,
               "solved": sum(s.status == "Solved" for s in sols), "valid": int(np.sum(grad.valid)),
               "iteration_time_s": sols[0].iteration_time,
               "ms_per_iteration": 1e3 * sols[0].iteration_time / max(iters, 1)}
        L = hip.lib()
        ptr = [hip._pf(v) for v in (gx, gz, gs)]
        dptr = [hip.C.c_void_p(t.data_ptr()) for t in (dgx, dgz, dgs)]
        # the C calls alone (Python's result copies are not part of a backward)
        run["backward_host_inputs"] = clock(lambda: hip._check(L.chip_bgrad_backward(bs._h, *ptr), "backward"))
        run["backward_device_inputs"] = clock(lambda: hip._check(L.chip_bgrad_backward_dev(bs._h, *dptr), "backward"))
        run["backward_python_device"] = clock(lambda: bs.backward(dgx, dgz, dgs))
        run["backward_over_iteration"] = run["backward_device_inputs"]["median_ms"] / run["ms_per_iteration"]
        try:
            run["backward_launches"] = bs.debug_counter("backward_launches")
            run["backward_host_syncs"] = bs.debug_counter("backward_host_syncs")
        except Exception:  # (a library without the test hooks)
            pass
        xo = np.concatenate([[0], np.cumsum(bs.n_part)])
        zo = np.concatenate([[0], np.cumsum(bs.m_part)])
        picks = sorted(set(np.linspace(0, nprob - 1, min(a.check, nprob)).astype(int).tolist()))
        worst = 0.0
        for k in picks:
            if sols[k].status != "Solved":
                continue
            want = R.adjoint(prs[k], sols[k].x, sols[k].s, sols[k].z, gx[xo[k]:xo[k + 1]], gz[zo[k]:zo[k + 1]],
                             gs[zo[k]:zo[k + 1]])
            for w, got in zip(want, grad.per_member(k)):
                worst = max(worst, R.rel(got, w))
        run["checked_members"] = picks
        run["worst_gradient_difference"] = worst
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        del bs, grad


if __name__ == "__main__":
    main()
