"""Scale run of the batched solver's forward-mode derivatives (HipBatchSolver.jvp) on batches of the long-only
factor-model portfolio QP synthetic.portfolio_qp(n_assets, n_factors, seed=200+i), the batches of
tools/batch_adjoint_scale.py: for every batch size, in ONE process with host clocks around synchronised calls: setup,
solve, iterations, ms per iteration, and on the same handle in the same run the first apply after a solve (it pays the
scaling update and the refactor at the final iterates; timed once per solve, over --repeats re-solves), an apply that
reuses the factorisation (host and device inputs) and a backward, with the two ratios apply / iteration and reusing
apply / first apply, and the worst relative difference of the tangents against the dense numpy restatement
tests/tangent_ref.py on up to 8 sampled members, evaluated at the device's own solution.  The output also carries the
figures the GPU tests measured on their small members (the MEASURED_* constants of tests/test_batch_jvp_gpu.py).
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
    from tests import tangent_ref as T
    from tests import test_batch_jvp_gpu as G

    def stats(ts):
        return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * float(np.median(ts))}

    def clock(fn, repeats=None):
        ts = []
        for _ in range(repeats or a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return stats(ts)

    res = {"problem": "portfolio_qp(%d, %d, seed=200+i)" % (a.assets, a.factors),
           "gpu_test_measured": {"source": "the constants of tests/test_batch_jvp_gpu.py",
                                 "tangents_vs_tangent_ref": G.MEASURED_TAN,
                                 "duality_with_backward": G.MEASURED_DUAL,
                                 "tangents_vs_central_differences": G.MEASURED_FD},
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
        n, m, nP, nA = bs.stack["n"], bs.stack["m"], len(bs.stack["P"][2]), len(bs.stack["A"][2])
        rng = np.random.default_rng(1)
        d = [rng.standard_normal(k) for k in (n, m, nP, nA)]
        gin = [rng.standard_normal(k) for k in (n, m, m)]
        dd = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in d]
        dg = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in gin]
        torch.cuda.synchronize()
        tan = bs.jvp(*d)  # warm-up (it allocates the handle's tangent buffers), and the result that is checked
        bs.backward(*gin)  # warm-up of the gradient buffers
        run = {"nprob": nprob, "n": n, "m": m, "nnzP": nP, "nnzA": nA, "setup_s": t1 - t0, "solve_s": t2 - t1,
               "iterations_max": iters, "solved": sum(s.status == "Solved" for s in sols),
               "valid": int(np.sum(tan.valid)), "iteration_time_s": sols[0].iteration_time,
               "ms_per_iteration": 1e3 * sols[0].iteration_time / max(iters, 1)}
        L = hip.lib()
        ptr = [hip._pf(v) for v in d]
        dptr = [hip.C.c_void_p(t.data_ptr()) for t in dd]
        gptr = [hip.C.c_void_p(t.data_ptr()) for t in dg]
        # the C calls alone (Python's result copies are not part of an apply).  K is factored at the final iterates
        # now: these applies reuse it
        run["apply_reusing_host_inputs"] = clock(lambda: hip._check(L.chip_bjvp_apply(bs._h, *ptr), "apply"))
        run["apply_reusing_device_inputs"] = clock(lambda: hip._check(L.chip_bjvp_apply_dev(bs._h, *dptr), "apply"))
        run["apply_python_device"] = clock(lambda: bs.jvp(*dd))
        run["backward_device_inputs"] = clock(lambda: hip._check(L.chip_bgrad_backward_dev(bs._h, *gptr), "backward"))
        # the first apply after a solve: one timing per re-solve of the same handle
        first, refactors = [], []
        for _ in range(a.repeats):
            hip._check(L.chip_batch_solve(bs._h), "solve")
            t0 = time.perf_counter()
            hip._check(L.chip_bjvp_apply_dev(bs._h, *dptr), "apply")
            first.append(time.perf_counter() - t0)
            try:
                refactors.append(bs.debug_counter("jvp_refactors"))
            except Exception:  # (a library without the test hooks)
                pass
        run["apply_first_device_inputs"] = stats(first)
        run["apply_over_iteration"] = run["apply_reusing_device_inputs"]["median_ms"] / run["ms_per_iteration"]
        run["first_apply_over_iteration"] = run["apply_first_device_inputs"]["median_ms"] / run["ms_per_iteration"]
        run["reusing_over_first_apply"] = (run["apply_reusing_device_inputs"]["median_ms"]
                                           / run["apply_first_device_inputs"]["median_ms"])
        run["apply_over_backward"] = (run["apply_reusing_device_inputs"]["median_ms"]
                                      / run["backward_device_inputs"]["median_ms"])
        try:
            run["jvp_launches_first"] = bs.debug_counter("jvp_launches")
            run["jvp_host_syncs_first"] = bs.debug_counter("jvp_host_syncs")
            run["jvp_refactors_after_each_first_apply"] = refactors  # (cumulative; the warm-up apply paid the first)
            hip._check(L.chip_bjvp_apply_dev(bs._h, *dptr), "apply")
            run["jvp_launches_reusing"] = bs.debug_counter("jvp_launches")
            run["jvp_host_syncs_reusing"] = bs.debug_counter("jvp_host_syncs")
        except Exception:
            pass
        off = {k: np.concatenate([[0], np.cumsum([G.length(p, k) for p in prs])]).astype(int) for k in G.KEYS}
        picks = sorted(set(np.linspace(0, nprob - 1, min(a.check, nprob)).astype(int).tolist()))
        worst = 0.0
        for k in picks:
            if sols[k].status != "Solved":
                continue
            want = T.tangent(prs[k], sols[k].x, sols[k].s, sols[k].z,
                             *[v[off[key][k]:off[key][k + 1]] for v, key in zip(d, G.KEYS)])
            for w, got in zip(want, tan.per_member(k)):
                worst = max(worst, R.rel(got, w))
        run["checked_members"] = picks
        run["worst_tangent_difference"] = worst
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        del bs, tan


if __name__ == "__main__":
    main()
