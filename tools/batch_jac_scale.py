"""Scale run of the batched solver's blocks of tangents (chip_bjac_*, HipBatchSolver.jvp_block / member_jacobians) on
the batches of tools/batch_jvp_scale.py: synthetic.portfolio_qp(n_assets, n_factors, seed=200+i).  For every batch size,
on ONE handle in ONE process with host clocks around synchronised calls, medians of --repeats after a warm-up:
  a 16-direction block with device inputs (chip_bjac_apply_dev), as ms per direction;
  a single apply that reuses the factorisation, device inputs (chip_bjvp_apply_dev): the yardstick;
  the device work of member_jacobians("q"): the ceil(max n_k / 16) calls of chip_bjac_units, against max n_k single
  applies; and, for batches of at most --python-max members, member_jacobians("q", torch=True) itself (with its
  per-member result copies);
the bytes of the block's buffers, its launch and synchronisation counts, and the worst relative difference of a
block's directions against the dense numpy restatement tests/tangent_ref.py on up to 8 sampled members at the device's
own solution.  Prints one JSON object per batch size and, with --out FILE, rewrites FILE after every size."""
import argparse
import ctypes as C
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
    ap.add_argument("--python-max", type=int, default=16, help="largest batch member_jacobians() itself is timed on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    hip = g.load_package()
    from clarabel_rs_amd import synthetic
    from tests import adjoint_ref as R
    from tests import tangent_ref as T
    from tests import test_batch_jvp_gpu as G

    def clock(fn):
        fn()  # warm-up
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * float(np.median(ts))}

    K = hip.BJAC_MAX_DIR
    res = {"problem": "portfolio_qp(%d, %d, seed=200+i)" % (a.assets, a.factors), "directions_per_block": K, "runs": []}
    for nprob in a.nprob:
        prs = [synthetic.portfolio_qp(a.assets, a.factors, seed=200 + i) for i in range(nprob)]
        mem = [(hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"],
                p["cones"]) for p in prs]
        bs = hip.HipBatchSolver(mem)
        sols = bs.solve()
        iters = max(s.iterations for s in sols)
        n, m, nP, nA = bs.stack["n"], bs.stack["m"], len(bs.stack["P"][2]), len(bs.stack["A"][2])
        even = lambda v: (v + 1) // 2 * 2  # noqa: E731
        run = {"nprob": nprob, "n": n, "m": m, "nnzP": nP, "nnzA": nA, "iterations_max": iters,
               "solved": sum(s.status == "Solved" for s in sols),
               "ms_per_iteration": 1e3 * sols[0].iteration_time / max(iters, 1),
               "block_bytes_per_direction": 8 * (n + 2 * m + 2 * even(n) + 3 * even(m)),
               "block_bytes": 8 * K * (n + 2 * m + 2 * even(n) + 3 * even(m))}
        gen = torch.Generator(device="cuda").manual_seed(1)  # (16 directions of the stack: drawn where they are used)
        dd = [torch.randn((K, k), dtype=torch.float64, device="cuda", generator=gen) for k in (n, m, nP, nA)]
        torch.cuda.synchronize()
        blk = bs.jvp_block(*dd)  # allocates the block's buffers, factors K at the final iterates; the result checked
        run["valid"] = int(np.sum(blk.valid))
        L = hip.lib()
        bptr = [C.c_void_p(t.data_ptr()) for t in dd]
        sptr = [C.c_void_p(t[0].data_ptr()) for t in dd]
        run["block16_device_inputs"] = clock(lambda: hip._check(L.chip_bjac_apply_dev(bs._h, K, *bptr), "block"))
        run["apply_reusing_device_inputs"] = clock(lambda: hip._check(L.chip_bjvp_apply_dev(bs._h, *sptr), "apply"))
        # (alternating once more: the two are compared, so neither should own the quieter moment)
        again_block = clock(lambda: hip._check(L.chip_bjac_apply_dev(bs._h, K, *bptr), "block"))
        again_apply = clock(lambda: hip._check(L.chip_bjvp_apply_dev(bs._h, *sptr), "apply"))
        run["block16_device_inputs_again"], run["apply_reusing_device_inputs_again"] = again_block, again_apply
        per_dir = run["block16_device_inputs"]["median_ms"] / K
        run["block_ms_per_direction"] = per_dir
        run["apply_over_block_direction"] = run["apply_reusing_device_inputs"]["median_ms"] / per_dir
        width = int(max(bs.n_part))

        def units_calls():
            for first in range(0, width, K):
                hip._check(L.chip_bjac_units(bs._h, 0, C.c_int64(first), min(K, width - first)), "units")
        run["jacobian_q_columns"] = width
        run["jacobian_q_units_calls"] = clock(units_calls)
        run["jacobian_q_as_single_applies_ms"] = width * run["apply_reusing_device_inputs"]["median_ms"]
        run["single_applies_over_units_calls"] = (run["jacobian_q_as_single_applies_ms"]
                                                  / run["jacobian_q_units_calls"]["median_ms"])
        if nprob <= a.python_max:
            run["member_jacobians_q_torch"] = clock(lambda: bs.member_jacobians("q", torch=True))
        try:
            hip._check(L.chip_bjac_apply_dev(bs._h, K, *bptr), "block")
            run["jac_launches_reusing"] = bs.debug_counter("jac_launches")
            run["jac_host_syncs_reusing"] = bs.debug_counter("jac_host_syncs")
            run["jac_repeats"] = bs.debug_counter("jac_repeats")
            run["jac_refactors"] = bs.debug_counter("jac_refactors")
        except Exception:  # (a library without the test hooks)
            pass
        off = {k: np.concatenate([[0], np.cumsum([G.length(p, k) for p in prs])]).astype(int) for k in G.KEYS}
        picks = sorted(set(np.linspace(0, nprob - 1, min(a.check, nprob)).astype(int).tolist()))
        worst = 0.0
        for k in picks:
            if sols[k].status != "Solved":
                continue
            for t in ((0, K - 1) if k == picks[0] else (K - 1,)):  # (a dense solve of n_k + m_k unknowns each)
                want = T.tangent(prs[k], sols[k].x, sols[k].s, sols[k].z,
                                 *[v[t, off[key][k]:off[key][k + 1]].cpu().numpy() for v, key in zip(dd, G.KEYS)])
                for w, got in zip(want, blk.per_member(k)):
                    worst = max(worst, R.rel(got[t].cpu().numpy(), w))
        run["checked_members"] = picks
        run["worst_tangent_difference"] = worst
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        del bs, blk, dd


if __name__ == "__main__":
    main()
